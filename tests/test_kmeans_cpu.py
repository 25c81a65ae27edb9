"""CPU: the host restatement of the device k-means refresh (tests/kmeans_oracle.py) is pinned to the reference's OWN host call,
scipy.cluster.vq.kmeans2; the Philox point picker gives distinct, reproducible picks; the countdown restatement fires like
OnlineCodebookRefresh; the C ABI of csrc/kmeans.hip is declared, bound and validates its arguments without a GPU."""
import ctypes
import os
import sys
import warnings

import numpy as np
import pytest
import torch

from sgam_neurips22_amd import _lib

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import kmeans_oracle as KO  # noqa: E402

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
# scipy accumulates the means in float32, the oracle in fp64: 4 x the largest difference measured between the two (4.6e-6) on
# data of unit noise scale
CENTRE_TOL = 2e-5


def _cases():
    """(name, x, init)"""
    x, init = KO.mixture(8192, 256, 64, 4.0, 0)
    yield "mixture", x, init
    x, init = KO.mixture(8192, 256, 64, 0.0, 0)
    yield "noise", x, init
    x, init = KO.mixture(4096, 256, 96, 4.0, 0)
    init[5] = init[4]              # a duplicated row: the tie goes to the lower index, the higher one gets no members
    init[9] = 50.0                 # a far-away row that never gets members
    yield "duplicate+far", x, init


@pytest.mark.parametrize("case", ["mixture", "noise", "duplicate+far"])
def test_oracle_lloyd_is_scipy_kmeans2(case):
    from scipy.cluster.vq import kmeans2
    x, init = next((x, i) for n, x, i in _cases() if n == case)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")            # "One of the clusters is empty": missing='warn' is the reference's mode
        c32, l32 = kmeans2(x, init.copy(), iter=10, minit="matrix", missing="warn")
    c64, l64, _ = KO.lloyd(x, init, 10)
    empty = len(init) - len(np.unique(l64))
    err = np.abs(c32.astype(np.float64) - c64).max()
    print(f"{case}: label mismatches {(l32 != l64).sum()}, max|dcentre| {err:.2e}, empty clusters {empty}")
    assert np.array_equal(l32, l64)
    assert err <= CENTRE_TOL
    if case == "duplicate+far":
        assert empty >= 1
        # empty clusters keep their previous value, in scipy and in the oracle
        assert np.array_equal(c64[9], np.full(256, 50.0)) and np.array_equal(c32[9], np.full(256, 50.0, np.float32))
        assert 9 not in l64


def test_oracle_update_keeps_empty_centres_and_counts_members():
    x = np.arange(24, dtype=np.float32).reshape(6, 4)
    c0 = np.full((4, 4), -7.0, np.float32)
    new, count = KO.update(x, np.array([2, 0, 2, 2, 0, 0], np.int32), c0)
    assert count.tolist() == [3, 0, 3, 0]
    assert np.array_equal(new[1], c0[1]) and np.array_equal(new[3], c0[3])
    assert np.allclose(new[0], x[[1, 4, 5]].mean(0)) and np.allclose(new[2], x[[0, 2, 3]].mean(0))


def test_oracle_argmin_takes_the_first_of_ties():
    x = np.zeros((3, 4), np.float32)
    c = np.ones((5, 4), np.float32)
    c[0] = 2.0
    lab, margin = KO.assign(x, c)
    assert lab.tolist() == [1, 1, 1] and (margin == 0).all()


@pytest.mark.parametrize("N,k", [(1, 1), (5, 5), (16, 16), (17, 4), (4096, 96), (65536, 1639), (262144, 16384), (1000003, 64)])
def test_point_picker_is_distinct_reproducible_and_keyed(N, k):
    a = KO.pick_points(N, k, seed=7, refresh=3)
    assert a.dtype == np.int32 and a.shape == (k,)
    assert a.min() >= 0 and a.max() < N and len(np.unique(a)) == k
    assert np.array_equal(a, KO.pick_points(N, k, seed=7, refresh=3))
    if N >= 4096:
        assert not np.array_equal(a, KO.pick_points(N, k, seed=7, refresh=4))       # another refresh number, other rows
        assert not np.array_equal(a, KO.pick_points(N, k, seed=8, refresh=3))
        # a prefix of the same permutation: asking for fewer rows gives the first of the same picks
        assert np.array_equal(a[:k // 2], KO.pick_points(N, k // 2, seed=7, refresh=3))


def test_point_picker_is_a_permutation_and_roughly_uniform():
    N = 1000                                      # 4^5 = 1024 >= 1000: 24 values are walked past
    p = KO.pick_points(N, N, seed=1, refresh=0)
    assert sorted(p.tolist()) == list(range(N))
    # the first pick over many refresh numbers covers [0, N) evenly: chi-square over 10 bins of 100 (9 degrees of freedom; 27.9 is
    # the 0.1 % point)
    first = np.array([KO.pick_points(N, 1, seed=1, refresh=r)[0] for r in range(2000)])
    obs = np.bincount(first // 100, minlength=10)
    assert ((obs - 200.0) ** 2 / 200.0).sum() < 27.9


def test_countdown_restatement_fires_like_the_host_refresh(monkeypatch):
    """drive OnlineCodebookRefresh and the restatement of the device bookkeeping with the same index stream: same fire steps, same
    dead lists (the refreshed centres themselves are the GPU tests' matter)"""
    import scipy.cluster.vq
    from sgam_neurips22_amd.training import OnlineCodebookRefresh
    n, D, T = 64, 4, 6

    class _Q:
        def __init__(self):
            self.embedding = torch.nn.Embedding(n, D)
            self.calls = []

        def update_codebook(self, feats, idx):
            self.calls.append(list(idx))

    class _M(torch.nn.Module):
        def __init__(self):
            super().__init__()
            self.quantize = _Q()

    monkeypatch.setattr(scipy.cluster.vq, "kmeans2", lambda data, k, minit="points": (np.zeros((k, data.shape[1]), np.float32), None))
    rs = np.random.RandomState(0)
    total_fires = 0
    for timeout in (2, 3, 5, 10):
        cfg = {"do_online_kmeans_clustering": True, "online_kmeans_word_timeout": timeout, "inactive_threshold": 0.3,
               "train_feature_buffer_size": 3, "frequency": 4, "start_global_step": 2}
        m = _M()
        host, dev = OnlineCodebookRefresh(m, cfg), KO.Countdown(n, cfg)
        fires = []
        for step in range(40):
            before = len(m.quantize.calls)
            got = host.before_step(step)
            dead = dev.before_step(step)
            assert got == len(dead)
            if got:
                assert m.quantize.calls[before] == dead
                fires.append(step)
            # a narrow band of words is in use, drifting: the others die and are refreshed again and again
            idx = (rs.randint(0, 12, size=(2, T)) + step // 8 * 5) % n
            host.after_forward(step, idx, np.zeros((D, 2, 3), np.float32))
            dev.after_forward(step, idx[0])
            assert [host.countdown[j] for j in range(n)] == dev.countdown.tolist()
            assert len(host.features) == min(dev.stored, cfg["train_feature_buffer_size"] + 1)
        assert fires and all(s % 4 == 0 and s >= 2 for s in fires), (timeout, fires)
        total_fires += len(fires)
    assert total_fires >= 8


def test_margin_guard_keeps_the_mixture_within_its_caps():
    """the fixture generator of the GPU tests: at most 2 % of the points dropped, at most 5 rounds (asserted inside), and what is
    left has a top-2 margin of at least 1e-4 at every iteration"""
    x, init = KO.mixture(4096, 256, 96, 4.0, 1)
    gx, c, lab, rounds = KO.guarded(x, init)
    print(f"margin guard: {len(x) - len(gx)} of {len(x)} points dropped in {rounds} round(s)")
    assert KO.lloyd(gx, init)[2].min() >= KO.MARGIN


def test_kmeans_abi_validates_without_gpu():
    lib = _lib.load()
    assert lib.sgam_kmeans_chunk_points(262144, 256, 16384) == 4096            # 256 MiB of dot products
    assert lib.sgam_kmeans_chunk_points(262144, 256, 1639) % 128 == 0
    assert lib.sgam_kmeans_chunk_points(100, 256, 7) == 128
    assert lib.sgam_kmeans_chunk_points(100, 250, 7) == -1                     # D % 32 != 0
    ws = lib.sgam_kmeans_assign_workspace_bytes(262144, 256, 16384, 4096)
    assert 4096 * 16384 * 4 + 16384 * 256 * 4 <= ws < 2 * 4096 * 16384 * 4     # never [N][k]
    assert lib.sgam_kmeans_assign_workspace_bytes(1000, 256, 96, 0) == -1
    assert lib.sgam_kmeans_update_workspace_bytes(262144, 16384, 0) >= 256 * 16384 * 4 + 262144 * 4
    assert lib.sgam_kmeans_update_workspace_bytes(1000, 8, 100) == -1          # block_points: a multiple of 256
    assert lib.sgam_kmeans_assign_f32(None, None, None, 8, 32, 2, 8, None, 0, None) == -1
    assert lib.sgam_kmeans_update_f32(None, None, None, None, 8, 32, 2, 0, None, 0, None) == -1
    assert lib.sgam_kmeans_init_points_f32(None, None, None, 8, 32, 2, 0, 0, None) == -1
    assert lib.sgam_codebook_countdown_i32(None, 4, None, 8, 2, None, None, None) == -1
    assert lib.sgam_codebook_scatter_rows_f32(None, None, None, 2, 32, 8, None, 2, None) == -1


def test_backend_selection_is_validated():
    """online_kmeans_config['backend']: absent = 'host' (the shipped YAMLs do not have the key); anything but host / device raises"""
    import inspect
    from sgam_neurips22_amd import training
    src = inspect.getsource(training.AutoencoderTrainer.__init__)
    assert 'kcfg.get("backend", "host")' in src
    assert training.DeviceCodebookRefresh.device_inputs is True
    for name in ("may_fire", "before_step", "after_forward", "_started"):
        assert callable(getattr(training.DeviceCodebookRefresh, name)) and callable(getattr(training.OnlineCodebookRefresh, name))
