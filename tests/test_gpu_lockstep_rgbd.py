"""GPU: lock-stepped scenes on the rgbd_integration branch (distributed.LockstepScenes(..., use_rgbd_integration=True)) — S fused
volumes advanced by the scene-batched TSDF kernels, one inverse warp and one forward at B = S — must produce, scene by scene, what
each scene produces alone.  Margins and tolerances are those of tests/test_gpu_lockstep.py."""
import os

import numpy as np
import pytest
import torch

from sgam_neurips22_amd import testing
from sgam_neurips22_amd.config import default_params
from sgam_neurips22_amd.distributed import LockstepScenes
from sgam_neurips22_amd.generative_sensing_module.model import VQModel
from sgam_neurips22_amd.inference_pipeline import InfiniteSceneGeneration, synthetic_seed_frame

pytestmark = pytest.mark.gpu
DEV = "cuda"
DATA = "google_earth"
POOL = 1 << 30          # brick pool per scene where the test is not about the default


def _maxerr(a, b):
    return (a.detach().cpu().double() - b.detach().cpu().double()).abs().max().item()


def _model(golden):
    g = golden("vqgan_full_ge256.npz")
    p = default_params(DATA)
    m = VQModel(**p)
    sd = testing.synthetic_state_dict(m.state_dict(), seed=0)
    sd["quantize.embedding.weight"] = testing.codebook_from_stats(float(g["zmean"]), float(g["zstd"]), 4096, 256, int(g["cb_seed"]))
    m.load_state_dict(sd)
    return m.to(DEV).eval(), sd


def _seeds(S):
    return [synthetic_seed_frame(DATA, i) for i in range(S)]


def test_lockstep_constructs_on_the_rgbd_branch(golden):
    m, _ = _model(golden)
    L = LockstepScenes(m, DATA, _seeds(2), output_dim=(4, 1), use_rgbd_integration=True, tsdf_memory_budget_bytes=POOL)
    vols = [sc.volume for sc in L.scenes]
    assert all(v is not None and v.brick_color is None for v in vols) and vols[0] is not vols[1]
    assert all(sc._tsdf_log == [] for sc in L.scenes) and L.scenes[0]._tsdf_log is not L.scenes[1]._tsdf_log


@pytest.mark.parametrize("graphed", [False, True], ids=["eager", "graph"])
def test_lockstep_rgbd_scenes_reproduce_their_solo_steps(golden, graphed):
    """Every step of every lock-stepped scene against the SAME step of a solo rgbd_integration scene started from the lock-stepped
    scene's frame store, with the volume that scene's logged integrations build (replayed like colour_volume replays them): target
    depth, model input and hole mask bit for bit (the conditioning does not depend on the batch); latent within 5e-5, codebook
    indices equal wherever the top-2 margin is >= 1e-4, RGB-D within 5e-5 and stored uint8 within the 1-LSB truncation boundary
    when the codes agree."""
    S = 2
    mL, sd = _model(golden)
    mS, _ = _model(golden)
    mL.enable_hip_graph(graphed)
    seeds = _seeds(S)
    L = LockstepScenes(mL, DATA, seeds, output_dim=(5, 1), use_rgbd_integration=True, tsdf_memory_budget_bytes=POOL)
    solos = [InfiniteSceneGeneration(mS, DATA, seed_index=i, output_dim=(5, 1), seed_frame=seeds[i], use_rgbd_integration=True,
                                     tsdf_memory_budget_bytes=POOL) for i in range(S)]
    cb = sd["quantize.embedding.weight"]
    tol = 5e-5
    flips = 0
    for step in range(3):
        for i, solo in enumerate(solos):           # the solo scene starts this step from the lock-stepped scene's store and volume
            sc = L.scenes[i]
            solo.frames = {c: dict(fr) for c, fr in sc.frames.items()}
            assert solo.curr == sc.curr
            solo.volume = None                     # (free the previous step's pool first)
            solo.volume = solo._make_volume()
            solo._tsdf_log = []
            for coords in sc._tsdf_log:
                nodes = [solo.transform_grid[c[0]][c[1]] for c in coords]
                solo.volume.integrate_many([solo.frames[c]["depth"] for c in coords], solo.K, [n["T"] for n in nodes],
                                           Ts_c2w=[n["T_inv"] for n in nodes])
        r = L.step(keep_results=True)
        assert r["x"].shape == (S, 4, 256, 256) and r["indices"].shape[0] == S and r["tgt_depth"].shape == (S, 256, 256)
        assert all(len(sc._tsdf_log) == step + 1 for sc in L.scenes)
        tgt = tuple(r["tgt"])
        for i, solo in enumerate(solos):
            res = solo.one_step_prediction(tgt)
            solo.curr += 1
            assert [tuple(c) for c in res["src_coords"]] == [tuple(c) for c in r["src_coords"][i]] == [tuple(c) for c in L.scenes[i]._tsdf_log[-1]]
            node = solo.transform_grid[tgt[0]][tgt[1]]
            z0, z1 = solo._Z_RANGE[DATA]
            tgt_depth = solo.volume.render_depth(solo.K, node["T"], 256, 256, z0, z1, T_c2w=node["T_inv"])   # what the step conditioned on
            assert (tgt_depth > 0).float().mean().item() > 0.5
            assert torch.equal(tgt_depth, r["tgt_depth"][i]), "the fused volume and its ray cast must not depend on the batch"
            assert torch.equal(res["x"], r["x"][i:i + 1]), "the conditioning must not depend on the batch"
            assert torch.equal(res["extrapolation_mask"], r["extrapolation_mask"][i:i + 1])
            pre_s = res["pre_quantized_features"]
            assert _maxerr(pre_s, r["pre_quantized_features"][i]) <= tol
            idx_s = torch.cdist(res["feature"].reshape(256, -1).t().double().cpu(), cb.double()).argmin(1)
            idx_l = r["indices"][i].reshape(-1).cpu()
            differ = idx_s != idx_l
            gap = testing.top2_relative_gap(pre_s.reshape(256, -1).t(), cb)
            assert not bool((differ & (gap >= 1e-4)).any()), gap[differ].tolist()
            flips += int(differ.sum())
            if not bool(differ.any()):
                assert _maxerr(res["rgbd"], r["rgbd"][i]) <= tol
                a = solo.frames[tgt]
                b = L.scenes[i].frames[tgt]
                du8 = (a["rgb_u8"].cpu().numpy().astype(np.int16) - b["rgb_u8"].cpu().numpy().astype(np.int16))
                assert np.abs(du8).max() <= 1
                assert (du8 != 0).mean() < 5e-3 and _maxerr(a["depth"], b["depth"]) <= 1e-3
    print(f"lockstep rgbd S={S}: near-tie flips over 3 steps: {flips}")
    assert not torch.equal(r["x"][0], r["x"][1])
    for i in range(S):
        assert len(L.scenes[i].frames) == 4 and L.scenes[i].curr == 4
    mL.enable_hip_graph(False)


def test_lockstep_rgbd_expand_and_run_tail(golden, tmp_path):
    m, _ = _model(golden)
    m.enable_hip_graph(True)
    L = LockstepScenes(m, DATA, _seeds(2), output_dim=(6, 1), use_rgbd_integration=True, tsdf_memory_budget_bytes=POOL)
    frames = L.expand()
    assert all(len(f) == 6 for f in frames)
    assert all(torch.isfinite(fr["depth"]).all() for f in frames for fr in f.values())
    assert not torch.equal(frames[0][(5, 0)]["rgb_u8"], frames[1][(5, 0)]["rgb_u8"])
    assert len(m._graphs) == 1
    assert all(len(sc._tsdf_log) == 5 and sc.volume.stats()[0] > 0 for sc in L.scenes)
    out = L.scenes[1].export_point_clouds(str(tmp_path))
    assert out["rgbd_integrated_mesh.ply"] > 0 and os.path.getsize(tmp_path / "rgbd_integrated_mesh.ply") > 1000
    m.enable_hip_graph(False)


def test_lockstep_rgbd_refusals(golden):
    m, _ = _model(golden)
    kw = dict(output_dim=(4, 1), use_rgbd_integration=True, tsdf_memory_budget_bytes=POOL)
    with pytest.raises(ValueError, match="raycast"):
        LockstepScenes(m, DATA, _seeds(2), rgbd_depth_render="mesh", **kw)
    with pytest.raises(ValueError, match="ConcurrentScenes"):
        LockstepScenes(m, DATA, _seeds(2), tgt_depth_provider=lambda *a: None, **kw)
    with pytest.raises(ValueError, match="num_src <= 8"):
        LockstepScenes(m, DATA, _seeds(2), num_src=9, **kw)


def test_lockstep_rgbd_shares_out_the_default_pool(golden):
    m, _ = _model(golden)
    free = torch.cuda.mem_get_info(m.device)[0]
    L = LockstepScenes(m, DATA, _seeds(2), output_dim=(4, 1), use_rgbd_integration=True)
    per_scene = min(48 << 30, free // 4) // 2
    for sc in L.scenes:
        assert sc.tsdf_memory_budget_bytes <= per_scene
        assert 0 < sc.volume.max_bricks <= per_scene // (16 ** 3 * 8)
