"""CPU: the device-side top-k infill sampler's generator and draw rule as restated by tests/sampler_oracle.py (Philox4x32-10
known answers, the rule's corner cases), and the new export's place in the C ABI (declared, bound, ABI number unchanged)."""
import ctypes
import os
import re
import sys

import numpy as np
import torch
import torch.nn.functional as F

from sgam_neurips22_amd import _lib

sys.path.insert(0, os.path.dirname(__file__))
import sampler_oracle as SO  # noqa: E402

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))


def _words(out):
    return [int(np.asarray(v).reshape(-1)[0]) for v in out]


def test_philox4x32_10_known_answers():
    """Random123 kat_vectors, philox4x32 with 10 rounds"""
    assert _words(SO.philox4x32_10((0, 0, 0, 0), (0, 0))) == [0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8]
    f = 0xffffffff
    assert _words(SO.philox4x32_10((f, f, f, f), (f, f))) == [0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd]
    assert _words(SO.philox4x32_10((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0))) == \
        [0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1]


def test_philox_vectorised_equals_scalar_and_uniforms_follow_the_counter_layout():
    u = SO.uniforms(seed=(7 << 32) | 5, stream_ids=[3, 9], call=(2 << 32) | 11, T=6, S=4)
    assert u.shape == (2, 6, 4) and u.dtype == np.float32 and (u >= 0).all() and (u < 1).all()
    for b, sid in enumerate((3, 9)):
        for t in (0, 5):
            for s in (0, 3):
                w0 = _words(SO.philox4x32_10((t * 4 + s, sid, 11, 2), (5, 7)))[0]
                assert u[b, t, s] == np.float32((w0 >> 8) * 2.0 ** -24)
    # a different call number, stream or seed moves every draw's counter / key
    assert not np.array_equal(u, SO.uniforms((7 << 32) | 5, [3, 9], (2 << 32) | 12, 6, 4))
    assert not np.array_equal(u[0], u[1])


def test_new_export_is_declared_bound_and_additive():
    text = open(os.path.join(ROOT, "include", "sgam_hip.h")).read()
    assert re.search(r"\bint sgam_vq_sample_topk_f32\s*\(", text)
    for needle in ("Philox4x32-10", "0xD2511F53", "0xCD9E8D57", "0x9E3779B9", "0xBB67AE85", "(word0 >> 8) * 2^-24",
                   "u * total < c_j"):
        assert needle in text, needle
    assert "sgam_vq_sample_topk_f32" in _lib.PROTOTYPES
    lib = _lib.load()
    assert lib.sgam_abi_version() == _lib.ABI_VERSION == 10
    assert hasattr(ctypes.CDLL(_lib.LIB_PATH), "sgam_vq_sample_topk_f32")
    # argument validation without a GPU: NULL operands, k beyond 32, a non-positive temperature
    n = None
    assert lib.sgam_vq_sample_topk_f32(n, n, n, n, n, 0, n, n, n, n, 1, 1, 16, 16, 256, 4096, 4, 0, 0, 0, 1.0, n) == -1
    one = ctypes.c_void_p(8)        # never dereferenced: the checks below fail before any launch
    assert lib.sgam_vq_sample_topk_f32(one, one, n, one, one, 0, one, one, one, one, 1, 1, 16, 16, 256, 4096, 33, 0, 0, 0, 1.0, n) == -1
    assert lib.sgam_vq_sample_topk_f32(one, one, n, one, one, 0, one, one, one, one, 1, 1, 16, 16, 256, 4096, 4, 0, 0, 0, 0.0, n) == -1
    assert lib.sgam_vq_sample_topk_f32(one, one, n, one, one, 0, one, one, one, one, 1, 1, 16, 16, 254, 4096, 4, 0, 0, 0, 1.0, n) == -1


def _candidates(B, T, k, seed, n_e=4096):
    rs = np.random.RandomState(seed)
    vals = np.sort(rs.uniform(1.0, 3.0, size=(B * T, k)).astype(np.float32), axis=1)
    inds = np.stack([rs.choice(n_e, size=k, replace=False) for _ in range(B * T)]).astype(np.int64)
    return vals, inds


def test_oracle_topk1_is_the_argmin_everywhere():
    vals, inds = _candidates(2, 64, 1, 0)
    o = SO.sample(vals, inds, (8, 8), 3, seed=1, stream_ids=[0, 1], call=0, mask=np.ones((2, 32, 32), bool))
    assert (o["indices"] == inds.reshape(2, 1, 8, 8)).all() and not o["band"].any()


def test_oracle_mask_all_zero_gives_slot_zero_everywhere():
    vals, inds = _candidates(2, 64, 4, 1)
    o = SO.sample(vals, inds, (8, 8), 2, seed=1, stream_ids=[0, 1], call=5, mask=np.zeros((2, 32, 32), bool))
    assert (o["slots"] == 0).all() and (o["indices"] == inds[:, 0].reshape(2, 1, 8, 8)).all()
    # with the hole open the draws are not all slot 0 (the case above is the mask's doing)
    assert (SO.sample(vals, inds, (8, 8), 2, 1, [0, 1], 5, mask=np.ones((2, 32, 32), bool))["slots"] != 0).any()


def test_oracle_reference_mode_uses_row_zero_and_per_token_mode_row_t():
    B, T, k = 2, 64, 4
    vals, inds = _candidates(B, T, k, 2)
    # row 0 of each item: slot 0 overwhelmingly likely; every other row: uniform over the slots
    v = vals.reshape(B, T, k).copy()
    v[:, 0] = [1.0, 60.0, 61.0, 62.0]
    v[:, 1:] = 2.0
    ref = SO.sample(v.reshape(-1, k), inds, (8, 8), 8, seed=3, stream_ids=[0, 1], call=0)
    tok = SO.sample(v.reshape(-1, k), inds, (8, 8), 8, seed=3, stream_ids=[0, 1], call=0, per_token=True)
    assert (ref["slots"] == 0).all()                       # every token drew from row 0's distribution
    assert (tok["slots"][:, 0] == 0).all()                 # token 0 still does
    counts = np.bincount(tok["slots"][:, 1:].reshape(-1), minlength=k)
    assert (counts > 0.15 * counts.sum()).all()            # the others from their own (uniform) rows
    # and the cumulative weights are the sequential fp32 sums of step 3
    c = SO.cumulative_weights(np.array([[1.0, 1.5, 2.0]], np.float32), 0.5)[0]
    e = [np.float32(1.0), np.exp(np.float32(-1.0)), np.exp(np.float32(-2.0))]
    assert c[0] == e[0] and c[1] == np.float32(e[0] + e[1]) and c[2] == np.float32(np.float32(e[0] + e[1]) + e[2])


def test_oracle_mask_resize_is_interpolate_nearest():
    rs = np.random.RandomState(4)
    for (H, W), (h, w) in (((256, 256), (16, 16)), ((256, 256), (32, 32)), ((250, 100), (32, 32)), ((37, 53), (32, 32)),
                           ((16, 16), (32, 32))):
        m = rs.rand(2, H, W) > 0.5
        want = F.interpolate(torch.from_numpy(m[:, None].astype(np.float32)), size=(h, w))[:, 0].numpy() != 0
        assert np.array_equal(SO.resize_mask_nearest(m, h, w), want), ((H, W), (h, w))


def test_slot_probabilities_sum_to_one_and_follow_the_softmax():
    v = np.array([1.0, 1.25, 1.5, 3.0], np.float32)
    p = SO.slot_probabilities(v, 0.5)
    want = torch.softmax(-torch.from_numpy(v).double() / 0.5, 0).numpy()
    assert abs(p.sum() - 1.0) < 1e-12 and np.abs(p - want).max() < 1e-6
