"""GPU: direct RGB-D odometry (csrc/rgbd_odometry.hip through geometry.rgbd_pyramid / rgbd_odometry / multiway_rgbd) against the
numpy twin (tests/odometry_oracle.py): the pyramid bit for bit; the sums of a Gauss-Newton step within the reordering bound of
their own summands, the counts exactly; the update within the bounds tests/test_gpu_icp.py uses for the rule it repeats; the loops
against the TRUTH on the analytic scenes within the constants tests/test_odometry_cpu.py measured of the twin; batches against
single pairs bit for bit; and the scene-level callers on both warp branches."""
import copy
import os
import sys

import numpy as np
import pytest
import torch

from sgam_neurips22_amd import geometry, testing

sys.path.insert(0, os.path.dirname(__file__))
import icp_oracle as IO  # noqa: E402
import odometry_oracle as OO  # noqa: E402
from test_gpu_consistency import TAU, Z_RANGE, pairs_of, same_bits, seeded_frames  # noqa: E402
from test_odometry_cpu import CASES, FACTOR, HAND_TAU, HAND_Z, MEASURED, analytic, five_frames  # noqa: E402
from test_odometry_cpu import TAU as SCENE_TAU  # noqa: E402
from test_odometry_cpu import Z_RANGE as SCENE_Z  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda"
U = 2.0 ** -53
SIZES = [(2, 2), (5, 7), (16, 16), (17, 19), (33, 64)]


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def levels_of(H, W):
    """as many levels as the size allows, three at the most"""
    n = 1
    while n < 3 and min((H + (1 << n) - 1) >> n, (W + (1 << n) - 1) >> n) >= 2:
        n += 1
    return n


def device_pyramid(depths, rgbs, K, levels):
    return geometry.rgbd_pyramid([_t(d) for d in depths], [_t(c) for c in rgbs], K, levels)


# ---------------------------------------------------------------- pyramid
@pytest.mark.parametrize("H,W", SIZES)
def test_pyramid_bits_against_the_twin(H, W):
    K, depths, rgbs, _ = seeded_frames(H, W)
    levels = levels_of(H, W)
    assert levels == (1 if H == 2 else 3)
    got, want = device_pyramid(depths, rgbs, K, levels), OO.pyramid(depths, rgbs, levels)
    assert got["levels"] == levels and got["frames"] == 4 and got["sizes"] == OO.level_sizes(H, W, levels)
    for l in range(levels):
        assert same_bits(got["intensity"][l], want[l][0]) and same_bits(got["depth"][l], want[l][1]), l
        assert np.array_equal(got["K"][l], OO.level_K(K, l))


# ---------------------------------------------------------------- accumulate
def pairs_with_a_bad_one(P):
    """test_gpu_consistency's pairs ((3, 0): a camera turned by 180 degrees), one of them replaced by an index outside [0, F)"""
    pairs = pairs_of(P)
    if P >= 3:
        pairs[1] = (0, 4) if P == 3 else (-1, 2)
    return pairs


def start_poses(Ts, pairs):
    """T_t T_s^-1 of the nominal poses (the identity for a pair outside the frames), moved a little so that residuals are not tiny"""
    nudge = OO.se3_exp(0.05 * OO.TRUE_XI)
    ok = lambda s, t: 0 <= s < len(Ts) and 0 <= t < len(Ts)  # noqa: E731
    return np.stack([nudge @ Ts[t] @ np.linalg.inv(Ts[s]) if ok(s, t) else np.eye(4) for s, t in pairs])


@pytest.mark.parametrize("P", [1, 3, 70])
@pytest.mark.parametrize("H,W", SIZES)
def test_accumulate_within_the_reordering_bound(H, W, P):
    K, depths, rgbs, Ts = seeded_frames(H, W)
    levels = levels_of(H, W)
    pairs = pairs_with_a_bad_one(P)
    init = start_poses(Ts, pairs)
    frames = np.stack([np.linalg.inv(Ts[t]) if 0 <= t < 4 else np.eye(4) for _, t in pairs])
    pyr, want_pyr = device_pyramid(depths, rgbs, K, levels), OO.pyramid(depths, rgbs, levels)
    run = geometry._RgbdOdometry(pyr, pairs, init, *Z_RANGE, TAU, 0.968, frames=frames)
    run.workspace_for(P)
    worst, covisible = 0.0, 0
    for level in range(levels):
        for info in (False, True):
            I, D = want_pyr[level]
            cache = {}
            want, mag = np.zeros((P, 32)), np.zeros((P, 32))
            for p, (s, t) in enumerate(pairs):
                if not (0 <= s < 4 and 0 <= t < 4):
                    continue                                               # a pair outside the frames: zero sums
                if (s, t) not in cache:
                    part, m = OO.accumulate(I[s], D[s], I[t], D[t], OO.level_K(K, level), init[p], *Z_RANGE, TAU, 0.968, info,
                                            frames[p][:3].reshape(12).astype(np.float32) if info else None)
                    cache[(s, t)] = (OO.fold(part), OO.fold(m))
                want[p], mag[p] = cache[(s, t)]
            got = torch.full((P, 32), -7.0, dtype=torch.float64, device=DEV)
            run.accumulate(level, 0, P, True, information=info)
            run.fold(level, 0, P, got)
            first = got.cpu().numpy()
            assert np.array_equal(first[:, 29:31], want[:, 29:31]) and (first[:, 31] == 0).all()
            bound = 2.0 * want[:, 29:30] * U * mag
            err = np.abs(first - want)
            assert (err[:, :29] <= bound[:, :29]).all(), (level, info, np.argwhere(err[:, :29] > bound[:, :29])[:4])
            ratio = np.where(bound > 0, err / np.where(bound > 0, bound, 1.0), 0.0)
            worst, covisible = max(worst, ratio[:, :29].max()), covisible + int(want[:, 29].sum())
            if info:
                assert (first[:, 21:29] == 0).all()
            run.accumulate(level, 0, P, True, information=info)            # equal run to run
            again = torch.empty_like(got)
            run.fold(level, 0, P, again)
            assert same_bits(again, got)
    print(f"odometry accumulate {H}x{W} P={P}: largest error / bound {worst:.3g}; covisible pixels summed {covisible}")
    if H * W >= 256:
        assert covisible > 0
    bad = [p for p, (s, t) in enumerate(pairs) if not (0 <= s < 4 and 0 <= t < 4)]
    assert (P < 3) == (not bad) and not first[bad].any()


# ---------------------------------------------------------------- update
def degenerate_frames(H, W):
    """the hand case at another size: depth 2 and grey = 4 * column seen twice leaves v_y free"""
    depth = np.full((H, W), 2.0, np.float32)
    grey = np.broadcast_to((4 * np.arange(W)).astype(np.uint8)[None, :, None], (H, W, 3)).copy()
    return depth, grey


def mixed_batch():
    """17 x 19: frames 0, 1 the degenerate ramp, frames 2, 3 the analytic plane pair -> a degenerate pair, a pair that converges (a
    frame against itself: the second iteration moves nothing) and a running pair"""
    d, c, K, T = analytic("plane", 17, 19)
    dd, gg = degenerate_frames(17, 19)
    return [dd, dd, d[0], d[1]], [gg, gg, c[0], c[1]], K, [(0, 1), (2, 2), (2, 3)], T


def test_update_equals_the_twin_on_every_path():
    depths, rgbs, K, pairs, _ = mixed_batch()
    rows = 4                                                               # (the twin's running pair is still running after four)
    want_pyr = OO.pyramid(depths, rgbs, 1)
    run = geometry._RgbdOdometry(device_pyramid(depths, rgbs, K, 1), pairs, None, *SCENE_Z, SCENE_TAU, 0.968, rows=rows)
    run.workspace_for(3)
    run.history.fill_(-7.0)
    states = np.stack([IO.new_state() for _ in pairs])
    sums = torch.empty((3, 32), dtype=torch.float64, device=DEV)
    worst = 0.0
    for it in range(rows):
        before = run.state.cpu().numpy().copy()
        run.accumulate(0, 0, 3, it == 0)
        run.update(0, 0, 3, it, it == 0, 1e-6, 1e-6, sums=sums)
        got, hist, folded = run.state.cpu().numpy(), run.history.cpu().numpy(), sums.cpu().numpy()
        assert (hist[:, it + 1:] == -7.0).all()                            # only its own row
        for p in range(3):
            # the twin's rule on the DEVICE's sums and the device's previous state: the update alone is compared
            want_s, want_r = OO.update(folded[p][None], it == 0, 1e-6, 1e-6, before[p])
            worst = max(worst, np.abs(got[p][:16] - want_s[:16]).max())
            assert np.abs(got[p][:16] - want_s[:16]).max() <= 1e-9 and np.array_equal(got[p][12:16], [0, 0, 0, 1])
            assert np.array_equal(got[p][18:21], want_s[18:21]) and np.array_equal(hist[p, it][[2, 6, 7]], want_r[[2, 6, 7]])
            assert np.allclose(got[p][[16, 17, 21]], want_s[[16, 17, 21]], rtol=1e-12, atol=0)
            assert np.allclose(hist[p, it], want_r, rtol=1e-9, atol=1e-12)
            if before[p][18] != 0.0:                                        # a frozen pair stays bit-identical
                assert np.array_equal(got[p].view(np.uint64), before[p].view(np.uint64))
                assert np.array_equal(hist[p, it], [before[p][16], before[p][17], before[p][20], before[p][21], 0, 0, before[p][18], 0])
        states = got
    print("update: largest |T - T_twin|", worst, "statuses", states[:, 18], "steps", states[:, 19])
    assert states[0, 18] == 2.0 and states[0, 19] == 0 and np.array_equal(states[0, :16], np.eye(4).reshape(16))
    assert states[1, 18] == 1.0 and states[1, 19] == 1 and hist[1, 1, 6] == 1.0
    assert states[2, 18] == 0.0 and states[2, 19] == rows
    # the whole loop against the twin's loop: each pair on its own path
    twin = OO.odometry(depths, rgbs, K, pairs, *SCENE_Z, SCENE_TAU, iterations=(rows,), pyr=want_pyr)
    assert np.array_equal(twin["status"], states[:, 18]) and np.array_equal(twin["iterations"], states[:, 19])
    assert np.abs(twin["transformation"].reshape(3, 16) - states[:, :16]).max() <= 1e-9
    # the next level's first iteration: the converged pair runs again, the degenerate one does not
    run.accumulate(0, 0, 3, True)
    run.update(0, 0, 3, 0, True, 1e-6, 1e-6)
    after = run.state.cpu().numpy()
    assert after[0, 18] == 2.0 and np.array_equal(after[0].view(np.uint64), states[0].view(np.uint64))
    assert after[1, 18] == 0.0 and after[1, 19] == 2 and after[2, 19] == rows + 1


# ---------------------------------------------------------------- loops
def on_device(depths, rgbs, K, pairs, z, tau, **kw):
    return geometry.rgbd_odometry([_t(d) for d in depths], [_t(c) for c in rgbs], K, pairs, z[0], z[1], tau, **kw)


def test_hand_case_on_the_device():
    depth, grey, K = OO.hand_case()
    res = on_device([depth, depth], [grey, grey], K, [(0, 1)], HAND_Z, HAND_TAU, iterations=(3,))
    assert res["status"].tolist() == [2.0] and res["iterations"].tolist() == [0.0]
    assert same_bits(res["transformation"][0], np.eye(4)) and res["transformation"].dtype == torch.float64
    h = res["history"][0].cpu().numpy()
    assert h.shape == (3, 8) and (h[:, 6] == 2.0).all() and (h[:, 2] == 105).all() and (h[:, 0] == 105 / 128).all() and not h[:, 3].any()
    info = res["information"][0].cpu().numpy()
    part = OO.accumulate(OO.intensity0(grey), depth, OO.intensity0(grey), depth, K, np.eye(4), *HAND_Z, HAND_TAU, information=True)[0]
    assert np.array_equal(info, OO.information_matrix(OO.fold(part))) and info[5, 5] == 105      # (dyadic summands: any order is exact)


@pytest.mark.parametrize("case", sorted(CASES))
def test_loop_converges_to_the_truth(case):
    surface, H, W = case
    d, c, K, T = analytic(surface, H, W)
    res = on_device(d, c, K, [(0, 1)], SCENE_Z, SCENE_TAU, iterations=CASES[case])
    end = OO.pose_error(res["transformation"][0].cpu().numpy(), T)
    print(f"{surface} {H}x{W} on the device: {end[0]:.6g} deg / {end[1]:.6g} from the truth (the twin's measured {MEASURED[case]}); "
          f"status {res['status'].tolist()}, steps {res['iterations'].tolist()}")
    assert res["status"][0].item() != 2.0 and not (res["history"][0][:, 6] == 2.0).any().item()
    assert end[0] <= FACTOR * MEASURED[case][0] + 1e-9 and end[1] <= FACTOR * MEASURED[case][1] + 1e-9
    assert res["history"].shape == (1, sum(CASES[case]), 8)


def test_batches_chunks_and_runs_give_the_same_bits():
    K, depths, rgbs, Ts = seeded_frames(33, 64)          # (at 17 x 19 the coarsest level leaves every pair of these frames degenerate)
    pairs = [(s, t) for s in range(4) for t in range(4) if s != t] + [(1, 1)]
    init = start_poses(Ts, pairs)
    frames = np.stack([np.linalg.inv(Ts[t]) for _, t in pairs])
    d, c = [_t(x) for x in depths], [_t(x) for x in rgbs]
    kw = dict(iterations=(4, 3, 2), information_frames=frames)
    keys = ("transformation", "status", "fitness", "rmse", "iterations", "history", "information")
    whole = geometry.rgbd_odometry(d, c, K, pairs, *Z_RANGE, TAU, init=init, **kw)
    assert whole["pairs"] == pairs and whole["history"].shape == (13, 9, 8) and whole["information"].shape == (13, 6, 6)
    again = geometry.rgbd_odometry(d, c, K, pairs, *Z_RANGE, TAU, init=init, **kw)
    assert all(same_bits(whole[k], again[k]) for k in keys)                # two runs: identical history bits
    for chunk in (1, 5):
        part = geometry.rgbd_odometry(d, c, K, pairs, *Z_RANGE, TAU, init=init, _max_pairs=chunk, **kw)
        assert all(same_bits(whole[k], part[k]) for k in keys), chunk
    pyr = geometry.rgbd_pyramid(d, c, K, 3)
    for p in (0, 5, 11, 12):                                               # one at a time, on a pyramid built once
        one = geometry.rgbd_odometry(None, None, K, [pairs[p]], *Z_RANGE, TAU, init=init[p:p + 1], iterations=(4, 3, 2),
                                     information_frames=frames[p:p + 1], pyramid=pyr)
        assert all(same_bits(whole[k][p:p + 1], one[k]) for k in keys), p
    status = whole["status"].cpu().numpy()
    info = whole["information"].cpu().numpy()
    assert np.array_equal(info, info.transpose(0, 2, 1)) and set(status) <= {0.0, 1.0, 2.0}
    # the pairs with the camera turned by 180 degrees see nothing: degenerate at once, the pose untouched
    for p, (s, t) in enumerate(pairs):
        if (s == 3) != (t == 3):
            assert status[p] == 2.0 and same_bits(whole["transformation"][p], init[p]) and info[p, 5, 5] == 0
    assert (status != 2.0).sum() >= 4
    without = geometry.rgbd_odometry(d, c, K, pairs[:2], *Z_RANGE, TAU, init=init[:2], iterations=(4, 3, 2), information=False)
    assert "information" not in without and same_bits(without["history"], whole["history"][:2])


def test_multiway_rgbd_against_the_twin_scenario():
    """test_odometry_cpu's five frames, one nominal pose wrong: the device recovers it within the same bound"""
    depths, rgbs, K, true, nominal = five_frames()
    out = geometry.multiway_rgbd([_t(d) for d in depths], [_t(c) for c in rgbs], K, nominal, *SCENE_Z, SCENE_TAU, loop_closure_stride=3)
    assert out["edges"] == [(0, 1, False), (1, 2, False), (2, 3, False), (3, 4, False), (0, 3, True), (1, 4, True)]
    assert out["missing_odometry"] == [] and out["kept"].all().item() and len(out["registrations"]) == 6 and len(out["graph"]) == 6
    assert set(out) >= {"poses", "line_weights", "kept", "history", "status", "iterations", "cost", "converged", "graph", "edges",
                        "registrations", "missing_odometry"}
    rot, trans = MEASURED[("paraboloid", 33, 64)]
    poses = out["poses"].cpu().numpy()
    for i in range(5):
        err = OO.pose_error(nominal[i] @ np.linalg.inv(poses[i]), true[i])
        print(f"frame {i}: corrected pose {err[0]:.4g} deg / {err[1]:.4g} from the truth")
        assert err[0] <= FACTOR * rot * 4 + 1e-9 and err[1] <= FACTOR * trans * 4 + 1e-9
    # an information matrix of an edge is the twin's, in the world frame
    k = 1
    info = out["graph"].tensors()[3][k].cpu().numpy()
    M = out["registrations"][k]["transformation"].cpu().numpy()
    pyr = OO.pyramid(depths, rgbs, 1)
    part, mag = OO.accumulate(pyr[0][0][1], pyr[0][1][1], pyr[0][0][2], pyr[0][1][2], K, M, *SCENE_Z, SCENE_TAU, information=True,
                              frame=np.linalg.inv(nominal[2])[:3].reshape(12).astype(np.float32))
    want = OO.information_matrix(OO.fold(part))
    assert info[5, 5] == want[5, 5] > 1000 and (np.abs(info - want) <= 2.0 * want[5, 5] * U * OO.information_matrix(OO.fold(mag))).all()


# ---------------------------------------------------------------- scenes
@pytest.fixture(scope="module")
def model(golden):
    """the synthetic-weights model of test_gpu_consistency"""
    from sgam_neurips22_amd.config import default_params
    from sgam_neurips22_amd.generative_sensing_module.model import VQModel
    g = golden("vqgan_full_ge256.npz")
    m = VQModel(**default_params("google_earth"))
    sd = testing.synthetic_state_dict(m.state_dict(), seed=0)
    sd["quantize.embedding.weight"] = testing.codebook_from_stats(float(g["zmean"]), float(g["zstd"]), 4096, 256, int(g["cb_seed"]))
    m.load_state_dict(sd)
    return m.to(DEV).eval()


@pytest.fixture(scope="module", params=["splat", "rgbd"])
def scene(request, model):
    """a 3-frame GoogleEarth scene, generated once per branch and left unchanged by every test"""
    from sgam_neurips22_amd.inference_pipeline import InfiniteSceneGeneration, synthetic_seed_frame
    kw = dict(use_rgbd_integration=True) if request.param == "rgbd" else {}
    s = InfiniteSceneGeneration(model, "google_earth", output_dim=(3, 1), seed_frame=synthetic_seed_frame("google_earth", 0),
                                tsdf_memory_budget_bytes=4 << 30, **kw)
    s.scene_expansion()
    assert len(s.frames) == 3
    s.branch = request.param
    return s


WRONG = OO.se3_exp(0.3 * OO.TRUE_XI[[1, 2, 0, 4, 5, 3]])                     # what the last frame's stored pose is off by


def analytic_scene(scene):
    """A copy of the scene whose frames are hand-made: the paraboloid rendered at the scene's size and intrinsics from the cameras
    exp(k TRUE_XI / 2); the LAST frame's stored pose is WRONG times the true one, its pixels those of the true pose."""
    coords = [c for c, _ in sorted(scene.frames.items(), key=lambda kv: (kv[1]["index"], kv[0]))]
    H, W = scene.image_resolution
    K = np.asarray(scene.K, np.float64)
    s = copy.copy(scene)
    s.frames = dict(scene.frames)
    s.transform_grid = copy.deepcopy(scene.transform_grid)
    true = [OO.se3_exp(0.5 * k * OO.TRUE_XI) for k in range(len(coords))]
    for k, c in enumerate(coords):
        depth, rgb = OO.render("paraboloid", true[k], K, H, W)
        s.frames[c] = dict(scene.frames[c], depth=_t(depth), rgb_u8=_t(rgb))
        s.transform_grid[c[0]][c[1]]["T"] = true[k].copy()
    last = coords[-1]
    s.transform_grid[last[0]][last[1]]["T"] = WRONG @ true[-1]
    return s, coords, true


def test_scene_odometry_and_pose_optimisation(scene):
    s, coords, true = analytic_scene(scene)
    frames_before, volume_before = dict(s.frames), s.volume
    # the constants of the largest measured case of this surface; the frames here are finer (256 x 256), which leaves less
    rot, trans = (FACTOR * v for v in MEASURED[("paraboloid", 64, 64)])
    res = s.rgbd_odometry(SCENE_TAU)
    assert res["coords"] == coords and res["pairs"] == [(1, 0), (2, 0), (2, 1)] and res["transformation"].shape == (3, 4, 4)
    stored = [WRONG @ true[2] if k == 2 else true[k] for k in range(3)]
    for e in res["per_pair"]:
        a, b = e["pair"]
        want = (true[b] @ np.linalg.inv(true[a])) @ np.linalg.inv(stored[b] @ np.linalg.inv(stored[a]))
        want_rot, want_trans = OO.pose_error(want, np.eye(4))
        print(scene.branch, "pair", e["pair"], "residual motion", e["rotation_deg"], "deg /", e["translation"], "expected", want_rot, want_trans,
              "status", e["status"], "steps", e["iterations"], "fitness", e["fitness"])
        assert e["status"] != 2 and abs(e["rotation_deg"] - want_rot) <= rot + 1e-9 and abs(e["translation"] - want_trans) <= trans + 1e-9
        assert (want_rot > 10 * rot) == (a == 2)                           # the wrong frame's pairs report its motion, the other ~0
    assert [(f["coord"], f["index"]) for f in res["per_frame"]] == [(c, s.frames[c]["index"]) for c in coords[1:]]
    assert res["per_frame"][0]["rotation_deg"] == res["per_pair"][0]["rotation_deg"]
    assert res["per_frame"][1]["translation"] == np.mean([res["per_pair"][1]["translation"], res["per_pair"][2]["translation"]])
    assert s.rgbd_odometry(SCENE_TAU, pairs="consecutive", iterations=(2,))["pairs"] == [(1, 0), (2, 1)]
    assert s.rgbd_odometry(SCENE_TAU, pairs=[(coords[2], coords[1])], frames=coords[1:], iterations=(2,))["pairs"] == [(1, 0)]
    with pytest.raises(ValueError, match="pairs"):
        s.rgbd_odometry(SCENE_TAU, pairs="later")
    with pytest.raises(ValueError, match="no pairs"):
        s.rgbd_odometry(SCENE_TAU, frames=coords[:1])
    # ---- the corrections
    fix = s.optimize_poses_rgbd(SCENE_TAU)
    assert set(fix) == {"coords", "corrections", "Ts_w2c", "edges", "line_weights", "kept", "missing_odometry", "converged", "status",
                        "iterations", "cost"}
    assert fix["coords"] == coords and fix["edges"] == [(0, 1, False), (1, 2, False), (0, 2, True)] and fix["missing_odometry"] == []
    for k in range(3):
        err = OO.pose_error(fix["Ts_w2c"][k], true[k])
        print(scene.branch, "frame", k, "corrected pose", err[0], "deg /", err[1], "from the truth")
        assert err[0] <= 2 * rot + 1e-9 and err[1] <= 2 * trans + 1e-9     # (a chain of two edges)
    off, on = s.view_consistency(SCENE_TAU), s.view_consistency(SCENE_TAU, pose_corrections=fix)
    right = off["per_pair"][0]["color_mae"]                                 # (1, 0): no wrong pose in it
    for k in (1, 2):
        print(scene.branch, "pair", off["pairs"][k], "color_mae uncorrected", off["per_pair"][k]["color_mae"], "corrected",
              on["per_pair"][k]["color_mae"], "; the correct pair's", right)
        assert on["per_pair"][k]["covisible"] > 10000 and on["per_pair"][k]["color_mae"] <= FACTOR * right
        assert off["per_pair"][k]["color_mae"] > 2 * FACTOR * right
    cloud = s.merged_point_cloud(pose_corrections=fix)
    assert cloud["points"].shape == (3 * 256 * 256, 3)
    vol = s.fuse_frames(pose_corrections=fix)
    assert vol.extract_triangle_mesh()["triangles"].shape[0] > 0
    assert list(s.frames) == list(frames_before) and all(s.frames[c] is frames_before[c] for c in coords) and s.volume is volume_before
