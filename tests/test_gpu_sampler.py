"""GPU: the device-side top-k infill sampler (csrc/vq.hip: sgam_vq_sample_topk_f32; VQModel.set_infill_sampler("device")) —
draw for draw against the CPU restatement of its rule (tests/sampler_oracle.py), the distribution of its draws, capture and
replay of a sampling forward, and the scene loops that sit on it.

What is compared how.  Candidates (values and indices against ops.vq_topk), the mask resize and the gather are exact, with no
exclusions.  A DRAW is compared where the oracle's u*total is further than BAND*total (4e-6: 32 terms x 2 ulp x 2^-24, rounded
up) from every cumulative weight — the device's expf and numpy's exp may differ in the last bits — and the oracle alone must
show that at most 0.5 % of a case's draws fall in that band before anything is compared (expected share ~ 2*4e-6*k <= 3e-4).
Inside the band the device's code must still be one of the token's candidates."""
import os
import sys

import numpy as np
import pytest
import torch

from sgam_neurips22_amd import ops, testing
from sgam_neurips22_amd.config import default_params
from sgam_neurips22_amd.distributed import LockstepScenes
from sgam_neurips22_amd.generative_sensing_module.model import VQModel
from sgam_neurips22_amd.inference_pipeline import InfiniteSceneGeneration, synthetic_seed_frame

sys.path.insert(0, os.path.dirname(__file__))
import sampler_oracle as SO  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda"
MAX_BAND_SHARE = 5e-3


def _ge_model(golden):
    g = golden("vqgan_full_ge256.npz")
    p = default_params("google_earth")
    m = VQModel(**p)
    sd = testing.synthetic_state_dict(m.state_dict(), seed=0)
    sd["quantize.embedding.weight"] = testing.codebook_from_stats(float(g["zmean"]), float(g["zstd"]), 4096, 256, int(g["cb_seed"]))
    m.load_state_dict(sd)
    return m.to(DEV).eval(), sd


def _quantiser(codebook):
    from sgam_neurips22_amd.generative_sensing_module.modules.vqvae.quantize import VectorQuantizer2
    q = VectorQuantizer2(codebook.shape[0], codebook.shape[1], beta=0.25)
    q.embedding.weight.data.copy_(codebook)
    return q.to(DEV).eval()


def _install(q, seed, per_token=False, temperature=1.0, call=0, streams=None):
    from sgam_neurips22_amd.generative_sensing_module.modules.vqvae.quantize import DeviceInfillSampler
    q.device_sampler = DeviceInfillSampler(seed, per_token, temperature)
    q.device_sampler.call, q.device_sampler.streams = call, streams
    return q


def _masks(B, kind, seed):
    """rectangular: a 256 x 256 mask with one rectangular hole per item; ragged: an irregular hole on a 250 x 100 mask (neither
    side a multiple of the latent's)"""
    rs = np.random.RandomState(seed)
    if kind == "rect":
        m = np.zeros((B, 1, 256, 256), bool)
        for b in range(B):
            y0, x0 = rs.randint(0, 100, 2)
            m[b, 0, y0:y0 + 140, x0:x0 + 120] = True
        return m
    yy, xx = np.mgrid[0:250, 0:100]
    m = np.stack([((np.sin(yy / (7.0 + b)) + np.cos(xx / (5.0 + b)) + rs.rand(250, 100) * 0.8) > 0.6) for b in range(B)])
    return m[:, None]


def _check_case(q, z, k, S, mask, seed, per_token, temperature, call, streams, what):
    """one draw-exact case: sample_nhwc on the device sampler against the oracle on the device's own top-k candidates"""
    B, h, w, D = z.shape
    cb, cb_sq = q._codebook()
    _install(q, seed, per_token, temperature, call, streams)
    zq, idx = q.sample_nhwc(z, k, S, None if mask is None else torch.from_numpy(mask).to(DEV))
    assert q.device_sampler.call == call + 1                     # a direct call is its own sampling forward
    # step 1: the candidates of the fused entry are ops.vq_topk's, bit for bit
    _, _, dist = ops.vq_nearest(z.reshape(B * h * w, D), cb, cb_sq, want_dist=True, want_zq=False)
    vals, inds = ops.vq_topk(dist, k)
    sid = torch.tensor(list(range(B)) if streams is None else streams, dtype=torch.int32, device=DEV)
    cbuf = torch.tensor([call], dtype=torch.int64, device=DEV)
    zq2, idx2, vals2, inds2 = ops.vq_sample_topk(dist, cb, k, S, (h, w), sid, cbuf, seed=seed,
                                                 mask=None if mask is None else torch.from_numpy(mask).to(DEV),
                                                 per_token=per_token, temperature=temperature)
    assert torch.equal(vals2.view(torch.int32), vals.view(torch.int32)) and torch.equal(inds2, inds), what
    assert torch.equal(idx2, idx) and torch.equal(zq2.view(torch.int32), zq.view(torch.int32)), what
    # step 6: a pure gather
    assert idx.shape == (B, S, h, w) and idx.dtype == torch.int64 and zq.shape == (B, S, h, w, D)
    assert torch.equal(zq.view(torch.int32), cb[idx].view(torch.int32)), what
    # steps 2 - 5 against the oracle
    o = SO.sample(vals.cpu().numpy(), inds.cpu().numpy(), (h, w), S, seed, list(range(B)) if streams is None else streams, call,
                  mask=None if mask is None else mask[:, 0], per_token=per_token, temperature=temperature)
    band = o["band"].transpose(0, 2, 1).reshape(B, S, h, w)
    share = float(band.mean())
    assert share <= MAX_BAND_SHARE, (what, share)                # the condition of the comparison, from the oracle alone
    got = idx.cpu().numpy()
    differ = got != o["indices"]
    assert not (differ & ~band).any(), (what, int((differ & ~band).sum()), int(differ.sum()))
    cand = inds.cpu().numpy().reshape(B, 1, h, w, k)
    assert (got[..., None] == cand).any(-1).all(), what          # inside the band: still one of the token's candidates
    return share, int(differ.sum()), float((o["slots"] != 0).mean())


def test_draw_exact_on_the_topk4_s2_fixture_latent(golden):
    """the latent of tests/golden/vqgan_topk4_s2.npz's input (GoogleEarth model, 256 x 256, rectangular hole; n_e = 4096, 16 x 16)"""
    m, sd = _ge_model(golden)
    x, mask = testing.rect_hole_input(1, 256, 256, seed=3)
    with torch.no_grad():
        z = m._encode_nhwc(x.to(DEV), mask.to(DEV)).contiguous()
    assert z.shape == (1, 16, 16, 256)
    q = m.quantize
    rows, sampled = [], 0.0
    for k in (2, 4, 10, 32):
        for S in (1, 4):
            for per_token in (False, True):
                for temperature in (1.0, 0.5):
                    r = _check_case(q, z, k, S, mask.numpy(), seed=1000 + k, per_token=per_token, temperature=temperature,
                                    call=S + 7, streams=None, what=(k, S, per_token, temperature))
                    rows.append(r)
                    sampled = max(sampled, r[2])
    q.device_sampler = None
    print(f"fixture latent: {len(rows)} cases, max band share {max(r[0] for r in rows):.2e}, in-band differences {sum(r[1] for r in rows)}")
    assert sampled > 0, "no case drew anything but slot 0: the comparison would show nothing"


@pytest.mark.parametrize("k", [2, 4, 10, 32])
def test_draw_exact_synthetic_latent_16384_codes(golden, k):
    """32 x 32 latent, n_e = 16384 (the CLEVR quantiser's size): S in {1, 4}, B in {1, 3}, rectangular and ragged masks, both
    modes, temperature 1 and 0.5 — the full cross product for this k"""
    g = golden("vqgan_full_clevr256_topk1.npz")
    zmean, zstd = float(g["zmean"]), float(g["zstd"])
    cb = testing.codebook_from_stats(zmean, zstd, 16384, 256, int(g["cb_seed"]))
    q = _quantiser(cb)
    gen = torch.Generator().manual_seed(77)
    z_all = (torch.randn((3, 32, 32, 256), generator=gen) * zstd + zmean).to(DEV)
    n, worst, nonzero = 0, 0.0, 0.0
    for B in (1, 3):
        z = z_all[:B].contiguous()
        for S in (1, 4):
            for kind in ("rect", "ragged"):
                mask = _masks(B, kind, seed=B * 10 + S)
                for per_token in (False, True):
                    for temperature in (1.0, 0.5):
                        streams = None if B == 1 else [11, 4, 2 ** 31 - 1]
                        share, _, nz = _check_case(q, z, k, S, mask, seed=(k << 33) + 5 * B + S, per_token=per_token,
                                                   temperature=temperature, call=(3 << 32) + n, streams=streams,
                                                   what=(k, B, S, kind, per_token, temperature))
                        n, worst, nonzero = n + 1, max(worst, share), max(nonzero, nz)
    print(f"n_e=16384 k={k}: {n} cases, max band share {worst:.2e}")
    assert n == 32 and nonzero > 0


def _chi2(counts, probs):
    n = counts.sum()
    e = probs * n
    assert e.min() >= 5, e.min()          # the chi-square approximation's usual validity condition
    return float(((counts - e) ** 2 / e).sum())


@pytest.mark.parametrize("k", [4, 10])
def test_draws_follow_the_distribution(golden, k):
    """Per-token mode on a latent whose tokens are all the same vector: every draw is from ONE known distribution, so the slot
    counts of 262144 draws (fixed seed: deterministic) must pass Pearson's chi-square against the oracle's probabilities at
    1 - 1e-6, and so must the k x k table of horizontally adjacent token pairs against the product distribution (independence
    of neighbouring counters).  Pairs are the DISJOINT ones (columns 2i, 2i+1): overlapping pairs share a draw, and their
    table's statistic would not follow chi-square with k^2 - 1 degrees of freedom."""
    from scipy.stats import chi2
    g = golden("vqgan_full_ge256.npz")
    zmean, zstd = float(g["zmean"]), float(g["zstd"])
    cb = testing.codebook_from_stats(zmean, zstd, 4096, 256, int(g["cb_seed"]))
    q = _quantiser(cb)
    gen = torch.Generator().manual_seed(5)
    tok = (torch.randn((256,), generator=gen) * zstd + zmean).to(DEV)
    B, S, h, w = 4, 64, 32, 32
    z = tok.expand(B, h, w, 256).contiguous()
    cbd, cb_sq = q._codebook()
    _, _, dist = ops.vq_nearest(z.reshape(B * h * w, 256), cbd, cb_sq, want_dist=True, want_zq=False)
    vals, inds = ops.vq_topk(dist, k)
    v = vals[0].cpu().numpy()
    # a temperature that spreads the mass over the slots (weights from 1 down to e^-1.5) whatever the codebook's scale: chosen
    # from the candidates' distances, not from any draw
    temperature = float((v[-1] - v[0]) / 1.5)
    p = SO.slot_probabilities(v, temperature)
    _install(q, seed=20221128, per_token=True, temperature=temperature, call=9)
    _, idx = q.sample_nhwc(z, k, S, None)                        # no mask: every token inside the hole
    hit = idx[..., None] == inds.view(B, 1, h, w, k)              # every code is one of its token's candidates ...
    assert bool(hit.any(-1).all())
    slots = hit.int().argmax(-1)                                 # ... and this is its slot, (B,S,h,w)
    assert int(slots.min()) >= 0
    n = slots.numel()
    assert n >= 200000
    counts = torch.bincount(slots.reshape(-1), minlength=k).cpu().numpy().astype(np.float64)
    stat = _chi2(counts, p)
    bound = float(chi2.ppf(1 - 1e-6, k - 1))
    print(f"k={k}: {n} draws, chi2 {stat:.2f} (bound {bound:.2f}, df {k - 1}), p {np.round(p, 4).tolist()}")
    assert stat < bound, (stat, bound, counts.tolist())
    if k == 4:
        pair = (slots[..., 0::2] * k + slots[..., 1::2]).reshape(-1)
        pc = torch.bincount(pair, minlength=k * k).cpu().numpy().astype(np.float64)
        stat2 = _chi2(pc, np.outer(p, p).reshape(-1))
        bound2 = float(chi2.ppf(1 - 1e-6, k * k - 1))
        print(f"k={k}: {pair.numel()} adjacent pairs, chi2 {stat2:.2f} (bound {bound2:.2f}, df {k * k - 1})")
        assert stat2 < bound2, (stat2, bound2)


def _resized_hole(mask, h=16, w=16):
    return torch.from_numpy(SO.resize_mask_nearest(mask.cpu().numpy()[:, 0], h, w))


def test_sampling_forward_replays_as_a_graph(golden):
    m, sd = _ge_model(golden)
    x, mask = testing.rect_hole_input(1, 256, 256, seed=3)
    x, mask = x.to(DEV), mask.to(DEV)
    m.set_infill_sampler("device", seed=42)
    assert m.infill_call == 0
    m.enable_hip_graph(True)
    replays = []
    with torch.no_grad():
        for j in range(3):
            decs, _, idx = m(x, topk=4, extrapolation_mask=mask, get_codebook_count=True)
            replays.append((decs[0].clone(), idx.clone()))
            assert m.infill_call == j + 1                        # advanced by one per sampling forward
        assert len(m._graphs) == 1, "a sampling forward on the device sampler must go through the captured graph"
        m.enable_hip_graph(False)
        for j in range(3):
            m.infill_call = j
            decs, _, idx = m(x, topk=4, extrapolation_mask=mask, get_codebook_count=True)
            assert torch.equal(idx, replays[j][1]), j
            assert torch.equal(decs[0].view(torch.int32), replays[j][0].view(torch.int32)), j
    hole = _resized_hole(mask)[0]
    i0, i1 = replays[0][1][0, 0].cpu(), replays[1][1][0, 0].cpu()
    assert torch.equal(i0[~hole], i1[~hole]) and bool((i0[hole] != i1[hole]).any())
    # topk = 1: the arg-min shortcut, with either sampler
    mh, _ = _ge_model(golden)
    with torch.no_grad():
        for graphed in (False, True):
            m.enable_hip_graph(graphed)
            a = m(x, topk=1, extrapolation_mask=mask, get_codebook_count=True)
            b = mh(x, topk=1, extrapolation_mask=mask, get_codebook_count=True)
            assert torch.equal(a[2], b[2]) and torch.equal(a[0][0].view(torch.int32), b[0][0].view(torch.int32))
    m.enable_hip_graph(False)
    # the host sampler is what a model without set_infill_sampler uses, and what "host" restores
    assert mh.quantize.device_sampler is None and mh.infill_call is None
    assert m.set_infill_sampler("host").quantize.device_sampler is None


def _oracle_step(cb_dev, pre, mask, feature, seed, streams, call, k=4, per_token=False):
    """a scene-loop step against the oracle: the draws on the step's OWN top-k candidates (from its own latent) and mask.
    pre (B,D,h,w), mask (B,1,H,W), feature (B,D,h,w) = the codes the step decoded.  Returns the band share."""
    B, D, h, w = pre.shape
    z = pre.permute(0, 2, 3, 1).reshape(B * h * w, D).contiguous()
    _, _, dist = ops.vq_nearest(z, cb_dev, ops.row_sumsq(cb_dev), want_dist=True, want_zq=False)
    vals, inds = ops.vq_topk(dist, k)
    o = SO.sample(vals.cpu().numpy(), inds.cpu().numpy(), (h, w), 1, seed, streams, call, mask=mask.cpu().numpy()[:, 0],
                  per_token=per_token)
    band = torch.from_numpy(o["band"].reshape(B, h, w))
    assert float(band.float().mean()) <= MAX_BAND_SHARE
    want = cb_dev[torch.from_numpy(o["indices"][:, 0]).to(DEV)]                      # (B,h,w,D)
    same = (feature.permute(0, 2, 3, 1).contiguous().view(torch.int32) == want.view(torch.int32)).all(-1).cpu()
    assert bool((same | band).all()), int((~(same | band)).sum())
    sampled = (torch.from_numpy(o["slots"].reshape(B, h, w)) != 0).sum()
    return int(sampled)


def _run_scene(m, cb_dev, infill_seed, seed_index=3, steps=6, check=True, per_token=False):
    scene = InfiniteSceneGeneration(m, "google_earth", topk=4, seed_index=seed_index, output_dim=(steps + 1, 1),
                                    seed_frame=synthetic_seed_frame("google_earth", seed_index), infill_sampler="device",
                                    infill_seed=infill_seed, infill_per_token=per_token)
    sampled = 0
    for _ in range(steps):
        tgt = scene.next_pose(scene.curr)
        res = scene.one_step_prediction(tgt, keep_results=True)
        if check:
            sampled += _oracle_step(cb_dev, res["pre_quantized_features"][None], res["extrapolation_mask"], res["feature"][None],
                                    infill_seed, [seed_index], scene.curr, per_token=per_token)
        scene.curr += 1
    if check:
        assert sampled > 0, "no token of six frames drew anything but slot 0"
    return scene


def _frames_equal(a, b):
    return a.keys() == b.keys() and all(torch.equal(a[c]["rgb_u8"], b[c]["rgb_u8"]) and
                                        torch.equal(a[c]["depth"].view(torch.int32), b[c]["depth"].view(torch.int32)) for c in a)


def test_scene_loop_on_the_device_sampler(golden):
    """6 generated frames of the GoogleEarth loop, topk = 4, graphs on: reproducible from (infill_seed, seed_index, frame
    index), every step's codes = the oracle's draws on that step's own candidates and mask, another seed gives other frames,
    and a forced rewind regenerates the dropped frames bit for bit."""
    m, sd = _ge_model(golden)
    m.enable_hip_graph(True)
    cb_dev = sd["quantize.embedding.weight"].to(DEV).contiguous()
    a = _run_scene(m, cb_dev, infill_seed=11)
    assert len(m._graphs) >= 1
    first = {c: dict(fr) for c, fr in a.frames.items()}
    b = _run_scene(m, cb_dev, infill_seed=11, check=False)
    assert _frames_equal(first, b.frames)
    c = _run_scene(m, cb_dev, infill_seed=12, check=False)
    assert not _frames_equal(first, c.frames)
    t = _run_scene(m, cb_dev, infill_seed=11, per_token=True)      # per-token mode through the same loop
    assert not _frames_equal(first, t.frames)
    # forced rewind: frames 4 .. 6 are dropped and generated again (other forwards have run in between: the draws do not care)
    assert a.curr == 7
    a.curr = a._rewind_to(4)
    assert a.curr == 4 and len(a.frames) == 4
    m.set_infill_sampler("device", seed=11)                        # (the scenes above re-configured the shared model)
    while a.curr < 7:
        a.one_step_prediction(a.next_pose(a.curr))
        a.curr += 1
    assert _frames_equal(first, a.frames)
    m.enable_hip_graph(False)


def test_lockstep_scenes_draw_what_they_draw_alone(golden):
    """4 lock-stepped scenes (stream ids = their seed indices, deliberately not their batch positions): every scene's codes at
    every step are the oracle's draws for (infill_seed, seed_index, frame index) on that run's own candidates and mask; the
    same holds for each scene run alone.  (Frames are not compared across the two runs: batched and solo forwards differ by
    up to 5e-5, which moves candidates.)"""
    m, sd = _ge_model(golden)
    m.enable_hip_graph(True)
    cb_dev = sd["quantize.embedding.weight"].to(DEV).contiguous()
    seed_indices = [5, 2, 7, 3]
    seeds = [synthetic_seed_frame("google_earth", i) for i in seed_indices]
    L = LockstepScenes(m, "google_earth", seeds, seed_indices=seed_indices, output_dim=(5, 1), topk=4, infill_sampler="device",
                       infill_seed=99)
    sampled = 0
    for step in range(3):
        call = L.curr
        r = L.step(keep_results=True)
        assert r["indices"].shape == (4, 1, 16, 16)
        quant = m.quantize.get_codebook_entry(r["indices"].reshape(-1), (4, 16, 16, 256))
        # scene i of the batch is checked against stream id seed_indices[i] — its own, whatever its batch position
        sampled += _oracle_step(cb_dev, r["pre_quantized_features"], r["extrapolation_mask"], quant, 99, seed_indices, call)
    assert sampled > 0
    for si in seed_indices[:2]:
        _run_scene(m, cb_dev, infill_seed=99, seed_index=si, steps=3)
    m.enable_hip_graph(False)
