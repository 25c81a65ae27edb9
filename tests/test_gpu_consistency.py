"""GPU: reprojection view consistency (csrc/view_consistency.hip through geometry.view_consistency) against the numpy twin
(tests/consistency_oracle.py) bit for bit, the hand-derived cases of tests/test_consistency_cpu.py on the device, determinism and
plumbing, the scene-level caller on both warp branches, and fuse_frames / export_fused_mesh: the stored frames fused once with
corrected poses."""
import copy
import ctypes
import functools
import os
import sys

import numpy as np
import pytest
import torch

from sgam_neurips22_amd import _lib, geometry, pointcloud, testing
from sgam_neurips22_amd.ops import _p, _stream, check
from sgam_neurips22_amd.tsdf import UNIT, VOLUME_PARAMS, TsdfVolume, frustum_bounds

sys.path.insert(0, os.path.dirname(__file__))
import consistency_oracle as CO  # noqa: E402
from test_consistency_cpu import (H_HAND, K_HAND, TAU_HAND, TX, TX_WRONG, W_HAND, Z_HAND, camera_at, class_picture, hand_frames,  # noqa: E402
                                  predicted_class)

pytestmark = pytest.mark.gpu
DEV = "cuda"
U = 2.0 ** -53
Z_RANGE = (0.5, 6.0)
TAU = 0.1
F32_MAX = np.float32(3.4028234663852886e38)


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _rot(axis, deg):
    a = np.asarray(axis, np.float64) / np.linalg.norm(axis)
    Kx = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    r = np.deg2rad(deg)
    return np.eye(3) + np.sin(r) * Kx + (1 - np.cos(r)) * Kx @ Kx


def _pose(R, t):
    T = np.eye(4)
    T[:3, :3], T[:3, 3] = R, t
    return T


@functools.lru_cache(maxsize=None)
def seeded_frames(H, W):
    """F = 4 frames: a smooth surface with holes of every kind; small random motions, frame 2 with frame 1's pose, frame 3 turned
    180 degrees (all of its points have Z < 0 in the others, and theirs in it)"""
    rs = np.random.RandomState(100 * H + W)
    K = np.array([[0.9 * W, 0, (W - 1) / 2.0], [0, 0.9 * W, (H - 1) / 2.0], [0, 0, 1]])
    yy, xx = np.meshgrid(np.linspace(0, 1, H), np.linspace(0, 1, W), indexing="ij")
    holes = [np.nan, np.inf, -np.inf, 0.0, -1.5, np.nextafter(np.float32(Z_RANGE[0]), np.float32(0)),
             np.nextafter(np.float32(Z_RANGE[1]), np.float32(7)), F32_MAX]
    depths, rgbs = [], []
    base = 2.5 + 0.3 * np.sin(2 * np.pi * (1.3 * xx + 0.7 * yy))             # one surface, seen by every frame ...
    for f in range(4):
        d = (base + 0.04 * np.sin(2 * np.pi * (rs.uniform(0.5, 2) * xx + rs.uniform(0.5, 2) * yy) + rs.uniform(0, 6))).astype(np.float32)
        n = max(1, H * W // 16) if H * W > 4 or f % 2 else 0                  # ... each with its own ripple and its own holes
        at = rs.choice(H * W, size=n, replace=False)
        d.reshape(-1)[at] = np.asarray([holes[(k + f) % len(holes)] for k in range(n)], np.float32)
        if H * W > 64:
            d[H // 3:H // 3 + 2, W // 2:W // 2 + 3] = 1.2 + f        # a step: occlusions and violations between the frames
        depths.append(d)
        rgbs.append(rs.randint(0, 256, size=(H, W, 3)).astype(np.uint8))
    Ts = [np.eye(4), _pose(_rot(rs.standard_normal(3), 1.5), rs.uniform(-0.04, 0.04, 3))]
    Ts.append(Ts[1].copy())
    Ts.append(_pose(_rot([0, 1, 0], 180.0) @ _rot(rs.standard_normal(3), 1.0), rs.uniform(-0.04, 0.04, 3)))
    return K, depths, rgbs, np.stack(Ts)


def pairs_of(P):
    if P == 1:
        return [(0, 1)]
    if P == 3:
        return [(0, 1), (1, 2), (3, 0)]
    rs = np.random.RandomState(P)
    return [(int(s), int(t)) for s, t in rs.randint(0, 4, size=(P, 2))]       # (repeats and s == t among them)


def on_device(K, depths, rgbs, Ts, z, tau, **kw):
    return geometry.view_consistency([_t(d) for d in depths], [_t(c) for c in rgbs], K, Ts, z[0], z[1], tau, **kw)


def same_bits(a, b):
    a, b = a.cpu().numpy() if isinstance(a, torch.Tensor) else a, b.cpu().numpy() if isinstance(b, torch.Tensor) else b
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def sums_within_the_bound(got, want):
    """counts equal; S1..S5 within n_cov * 2^-53 relative: every term is >= 0, so the rounding of a sum of n terms in ANY order is at
    most (n - 1) 2^-53 of it.  Returns the largest |got - want| / (n_cov 2^-53 want) seen."""
    assert np.array_equal(got[:, :7], want[:, :7])
    worst = 0.0
    for g, w in zip(got, want):
        for k in range(7, 12):
            if w[k] == 0:
                assert g[k] == 0
                continue
            ratio = abs(g[k] - w[k]) / (w[6] * U * w[k])
            worst = max(worst, ratio)
            assert ratio <= 1.0, (k, g[k], w[k], w[6])
    return worst


@pytest.mark.parametrize("P", [1, 3, 70])
@pytest.mark.parametrize("H,W", [(2, 2), (5, 7), (16, 16), (17, 19), (33, 64)])
def test_bits_against_the_twin(H, W, P):
    K, depths, rgbs, Ts = seeded_frames(H, W)
    pairs = pairs_of(P)
    want = CO.view_consistency(depths, rgbs, K, Ts, *Z_RANGE, TAU, pairs=pairs)
    got = on_device(K, depths, rgbs, Ts, Z_RANGE, TAU, pairs=pairs, maps=True)
    assert got["pairs"] == pairs and got["sums"].is_cuda and got["sums"].dtype == torch.float64 and got["sums"].shape == (P, 12)
    assert same_bits(got["class_map"], want["class_map"])
    assert same_bits(got["color_error"], want["color_error"]) and same_bits(got["depth_error"], want["depth_error"])
    worst = sums_within_the_bound(got["sums"].cpu().numpy(), want["sums"])
    seen = np.bincount(want["class_map"].reshape(-1), minlength=7)
    print(f"view consistency {H}x{W} P={P}: largest sum ratio {worst:.3g} of the n_cov 2^-53 bound; classes {seen.tolist()}")
    if H * W >= 256 and P == 70:
        assert (seen > 0).all()                                            # every class occurs among these inputs


def test_hand_derived_cases_on_the_device():
    depth, src, tgt = hand_frames()
    T_t, T_wrong = camera_at(x=TX), camera_at(x=TX + TX_WRONG)
    C = np.linalg.inv(T_t) @ T_wrong
    n_moved = (H_HAND - 1) * (W_HAND - 3)
    for name, frames, Ts, n_cov, err in (("identical", (src, src), [np.eye(4), np.eye(4)], (H_HAND - 1) * (W_HAND - 1), 0.0),
                                         ("moved", (src, tgt), [np.eye(4), T_t], n_moved, 0.0),
                                         ("wrong", (src, tgt), [np.eye(4), T_wrong], None, 2.0),
                                         ("corrected", (src, tgt), [np.eye(4), T_wrong @ np.linalg.inv(C)], n_moved, 0.0)):
        got = on_device(K_HAND, [depth, depth], list(frames), np.stack(Ts), Z_HAND, TAU_HAND, pairs=[(0, 1)], maps=True)
        cls, ce, ez = (got[k][0].cpu().numpy() for k in ("class_map", "color_error", "depth_error"))
        sums = got["sums"][0].cpu().numpy()
        cov = cls == CO.COVISIBLE
        assert sums[6] == cov.sum() > 0 and sums[:7].sum() == H_HAND * W_HAND and not ez.any() and not sums[9:].any(), name
        if n_cov is not None:
            assert cov.sum() == n_cov, name
        assert (ce[cov] == err).all() and not ce[~cov].any() and sums[7] == err * cov.sum() and sums[8] == err * err * cov.sum(), name
        if name == "identical":
            assert sums[1] == H_HAND + W_HAND - 1 and (cls[-1] == 1).all() and (cls[:, -1] == 1).all()
    # the tie |Z - D| == tau is covisible, from either side
    for target, want in ((2.5, -0.5), (1.5, 0.5)):
        got = on_device(K_HAND, [depth, np.full_like(depth, target)], [src, src], np.stack([np.eye(4)] * 2), Z_HAND, 0.5, pairs=[(0, 1)], maps=True)
        sums = got["sums"][0].cpu().numpy()
        assert sums[6] == (H_HAND - 1) * (W_HAND - 1) and (got["depth_error"][0, :-1, :-1] == want).all()
        assert sums[9] == 0.5 * sums[6] and sums[10] == 0.25 * sums[6] and sums[11] == 0.25 * sums[6]
    # the class picture of the CPU test
    H, W, target = class_picture()
    flat = np.full((H, W), 2.0, np.float32)
    rgb = np.zeros((H, W, 3), np.uint8)
    got = on_device(K_HAND, [flat, target], [rgb, rgb], np.stack([np.eye(4)] * 2), Z_HAND, TAU_HAND, pairs=[(0, 1)], maps=True)
    want = np.array([[predicted_class(target, i, j, H, W, TAU_HAND) for j in range(W)] for i in range(H)], np.uint8)
    assert np.array_equal(got["class_map"][0].cpu().numpy(), want)


def test_determinism_and_plumbing():
    K, depths, rgbs, Ts = seeded_frames(17, 19)
    every = [(s, t) for s in range(4) for t in range(4) if s != t]
    a = on_device(K, depths, rgbs, Ts, Z_RANGE, TAU, maps=True)
    b = on_device(K, depths, rgbs, Ts, Z_RANGE, TAU, maps=True)
    assert a["pairs"] == every and same_bits(a["sums"], b["sums"]) and all(same_bits(a[k], b[k]) for k in ("class_map", "color_error", "depth_error"))
    plain = on_device(K, depths, rgbs, Ts, Z_RANGE, TAU)
    assert set(plain) == {"pairs", "sums"} and same_bits(plain["sums"], a["sums"])
    assert same_bits(on_device(K, depths, rgbs, Ts, Z_RANGE, TAU, pairs=every)["sums"], a["sums"])
    for chunk in (1, 5, 12):
        c = on_device(K, depths, rgbs, Ts, Z_RANGE, TAU, maps=True, _max_pairs=chunk)
        assert same_bits(c["sums"], a["sums"]) and all(same_bits(a[k], c[k]) for k in ("class_map", "color_error", "depth_error")), chunk
    # the C entry's own safety: a pair outside [0, F) reads nothing and gets a zero row
    d, c = [_t(x) for x in depths], [_t(x) for x in rgbs]
    F, H, W, dev, ptrs = geometry.frame_store(d, c, "test")
    pairs = _t(np.array([[0, 1], [0, 4], [-1, 2]], np.int32))
    T = _t(np.stack([CO.relative_pose(Ts[0], Ts[1])] * 3))
    sums = torch.full((3, 12), 7.0, dtype=torch.float64, device=DEV)
    cmap = torch.full((3, H, W), 9, dtype=torch.uint8, device=DEV)
    ws, nbytes = geometry.workspace("sgam_view_consistency_workspace_bytes", DEV, H, W, 3)
    kinv = geometry.inverse_intrinsics(K)
    check(_lib.load().sgam_view_consistency_f32(_p(ptrs[:F]), _p(ptrs[F:]), F, H, W, ctypes.c_void_p(kinv.ctypes.data), float(np.float32(K[0, 0])),
                                                float(np.float32(K[1, 1])), float(np.float32(K[0, 2])), float(np.float32(K[1, 2])), Z_RANGE[0],
                                                Z_RANGE[1], TAU, _p(pairs), _p(T), 3, _p(sums), _p(cmap), None, None, _p(ws), nbytes,
                                                _stream()), "sgam_view_consistency_f32")
    assert same_bits(sums[0], a["sums"][0]) and not sums[1:].any() and not cmap[1:].any() and same_bits(cmap[0], a["class_map"][0])


# ---------------------------------------------------------------- scenes
@pytest.fixture(scope="module")
def model(golden):
    """the synthetic-weights model of test_gpu_posegraph"""
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
    assert len(s.frames) == 3 and (s.volume is not None) == (request.param == "rgbd")
    s.branch = request.param
    return s


def stored(scene):
    return [c for c, _ in sorted(scene.frames.items(), key=lambda kv: (kv[1]["index"], kv[0]))]


PLANE_DEPTH = 2.0
RAMP_SLOPE = 4.0                  # grey levels of red per column (green: one per row; blue constant)
WINDOW = (96, 156)                # the world columns (in frame 0's pixels) that hold the plane: 4 * 60 = 240 grey levels


def plane_scene(scene, step_px, windowed, wrong=None, wrong_along=0):
    """A copy of the scene whose frames are hand-made: the plane z = 2 with a colour ramp attached to the WORLD, seen from cameras
    without rotation at x = k * step (step_px pixels of disparity per frame, a multiple of 1/4 so that the ramp's uint8 values are
    exact).  windowed: only the world columns WINDOW hold depth (elsewhere 0, below the z range), so the ramp never clips.
    wrong: the LAST frame's stored pose has its camera centre off by this much along axis wrong_along; its pixels stay those of
    the true pose.  Returns (copy, coords, the last frame's true pose)."""
    coords = stored(scene)
    H, W = scene.image_resolution
    fx = float(scene.K[0, 0])
    step = step_px * PLANE_DEPTH / fx
    s = copy.copy(scene)
    s.frames = dict(scene.frames)
    s.transform_grid = copy.deepcopy(scene.transform_grid)
    for k, c in enumerate(coords):
        w = np.arange(W) + k * step_px                                       # the world column pixel j of frame k sees
        depth = np.full((H, W), PLANE_DEPTH, np.float32)
        if windowed:
            depth[:, ~((w >= WINDOW[0]) & (w <= WINDOW[1]))] = 0.0
        red = RAMP_SLOPE * (w - WINDOW[0])
        assert (red == np.round(red)).all()
        rgb = np.empty((H, W, 3), np.uint8)
        rgb[..., 0] = np.clip(red, 0, 255)[None, :]
        rgb[..., 1] = np.arange(H)[:, None]
        rgb[..., 2] = 77
        s.frames[c] = dict(scene.frames[c], depth=_t(depth), rgb_u8=_t(rgb))
        s.transform_grid[c[0]][c[1]]["T"] = camera_at(x=k * step)
    T_true = camera_at(x=(len(coords) - 1) * step)
    if wrong is not None:
        centre = [(len(coords) - 1) * step, 0.0, 0.0]
        centre[wrong_along] += wrong
        last = coords[-1]
        s.transform_grid[last[0]][last[1]]["T"] = camera_at(*centre)
    return s, coords, T_true


def test_scene_view_consistency(scene):
    coords = stored(scene)
    z0, z1 = scene._Z_RANGE[scene.data]
    frames_before = dict(scene.frames)
    res = scene.view_consistency(0.05, maps=True)
    assert res["coords"] == coords and res["pairs"] == [(1, 0), (2, 0), (2, 1)]
    direct = geometry.view_consistency([scene.frames[c]["depth"] for c in coords], [scene.frames[c]["rgb_u8"] for c in coords], scene.K,
                                       np.stack(scene._corrected_poses(coords, None, "test")), z0, z1, 0.05, pairs=res["pairs"], maps=True)
    for k in ("sums", "class_map", "color_error", "depth_error"):
        assert same_bits(res[k], direct[k]), k
    for again in (scene.view_consistency(0.05, pose_corrections=None), scene.view_consistency(0.05, pose_corrections={c: np.eye(4) for c in coords})):
        assert same_bits(again["sums"], res["sums"]) and "class_map" not in again
    rows = res["sums"].cpu().numpy()
    assert res["per_pair"] == [geometry.consistency_summary(r) for r in rows] and res["total"] == geometry.consistency_summary(rows)
    assert [(f["coord"], f["index"]) for f in res["per_frame"]] == [(c, scene.frames[c]["index"]) for c in coords[1:]]
    strip = lambda f: {k: v for k, v in f.items() if k not in ("coord", "index")}  # noqa: E731
    same = lambda a, b: all(a[k] == b[k] or (a[k] != a[k] and b[k] != b[k]) for k in a) and set(a) == set(b)  # noqa: E731
    assert same(strip(res["per_frame"][0]), geometry.consistency_summary(rows[0])) and same(strip(res["per_frame"][1]), geometry.consistency_summary(rows[1:]))
    total = res["total"]
    assert total["invalid"] + total["n_valid"] == 3 * 256 * 256 and total["covisible"] > 0
    print(scene.branch, "generated scene: covisibility", total["covisibility"], "violation rate", total["violation_rate"], "colour MAE",
          total["color_mae"], "depth MAE", total["depth_mae"])
    every = scene.view_consistency(0.05, pairs="all")
    assert every["pairs"] == [(s, t) for s in range(3) for t in range(3) if s != t]
    named = scene.view_consistency(0.05, pairs=[(coords[2], coords[1])], frames=coords[1:])
    assert named["coords"] == coords[1:] and named["pairs"] == [(1, 0)] and same_bits(named["sums"][0], res["sums"][2])
    with pytest.raises(ValueError, match="pairs"):
        scene.view_consistency(0.05, pairs="later")
    with pytest.raises(ValueError, match="no stored frame"):
        scene.view_consistency(0.05, pairs=[(coords[0], (9, 9))])
    with pytest.raises(ValueError, match="no pairs"):
        scene.view_consistency(0.05, frames=coords[:1])
    assert list(scene.frames) == list(frames_before) and all(scene.frames[c] is frames_before[c] for c in coords)
    # ---- hand-made frames: a plane with a colour ramp from translated cameras, the last pose wrong by half a pixel
    fx = float(scene.K[0, 0])
    plane, coords, T_true = plane_scene(scene, 8.25, True, wrong=0.5 * PLANE_DEPTH / fx)
    last = coords[-1]
    C = np.linalg.inv(T_true) @ plane.transform_grid[last[0]][last[1]]["T"]
    off = plane.view_consistency(0.05)
    on = plane.view_consistency(0.05, pose_corrections={last: C})
    # The bound on the corrected colour error, from the rounding of u at the dataset's intrinsics (u2 = 2^-24, one fp32 rounding):
    #   a = (kinv0 j + kinv1 i) + kinv2: |a| <= 0.52, kinv's own rounding and three operations: 4 u2 absolute; x = a d, d = 2: 8 u2;
    #   X = x + T3 (rotation exactly the identity, so the other terms are exact zeros): T3's rounding and the sum's, |X| < 2: 2 u2
    #   more: 10 u2; Z = d = 2 exactly.  u = (fx X) / Z + cx: the error of X times fx / Z, two roundings of a value |u - cx| <= 128
    #   (3 u2 |u - cx| with the rounding of fx), and the last sum's half ulp of a value below 256, 2^-17 = 128 u2:
    #       du <= (10 fx / 2 + 3 * 128 + 128) u2        (fx = 248.9: 1.05e-4 pixels);  dv alike.
    #   The bilinear colour: three sums of values below 256, 128 u2 each, and the products' roundings below them: 4 * 128 u2 per channel.
    #   Red has slope 4 per column, green 1 per row, blue is constant (its lerp is exact):
    #       color_mae <= (4 du + 1 dv + 2 * 512 u2) / 3.
    # Uncorrected, every covisible pixel is half a column off: |er| = slope / 2, so color_mae = slope / 2 / 3 within the same bound.
    u2 = 2.0 ** -24
    du = (10 * fx / 2 + 3 * 128 + 128) * u2
    bound = (RAMP_SLOPE * du + 1.0 * du + 2 * 512 * u2) / 3
    wrong_pair, right_pair = off["per_pair"][2], on["per_pair"][2]            # (2, 1): the frame with the wrong pose into its neighbour
    assert off["pairs"][2] == (2, 1) and wrong_pair["covisible"] > 1000 and right_pair["covisible"] > 1000
    print(scene.branch, "plane with a ramp: color_mae uncorrected", wrong_pair["color_mae"], "(slope / 2 / 3 =", RAMP_SLOPE / 6,
          ") corrected", right_pair["color_mae"], "bound", bound, "; first pair (no wrong pose)", off["per_pair"][0]["color_mae"])
    assert abs(wrong_pair["color_mae"] - RAMP_SLOPE / 2 / 3) <= bound
    assert right_pair["color_mae"] <= bound and off["per_pair"][0]["color_mae"] <= bound
    assert wrong_pair["color_mae"] > 100 * bound >= 100 * right_pair["color_mae"]
    assert right_pair["depth_mae"] == 0.0 and right_pair["violation"] == 0 and right_pair["occluded"] == 0


def units_of(vol):
    """(which units are open, their flags, their bricks' tsdf / weight / colour in unit order) — brick numbers are allocation
    order and not part of the result"""
    table = vol.unit_table
    used = table >= 0
    brick = (table[used] & 0x3FFFFFFF).long()
    return used, (table[used] & 0x40000000), vol.brick_tsdf[brick], vol.brick_weight[brick], None if vol.brick_color is None else vol.brick_color[brick]


def same_volume(a, b):
    if not (np.array_equal(a.base, b.base) and np.array_equal(a.dims, b.dims)):
        return False
    ua, ub = units_of(a), units_of(b)
    return all((x is None and y is None) or same_bits(x, y) for x, y in zip(ua, ub))


def same_mesh(a, b):
    ma, mb = a.extract_mesh_device(), b.extract_mesh_device()
    nv, nt = ma.n_vertices, ma.n_triangles
    return (nv, nt) == (mb.n_vertices, mb.n_triangles) and nt > 0 and same_bits(ma.vertices[:nv], mb.vertices[:nv]) and \
        same_bits(ma.triangles[:nt], mb.triangles[:nt]) and same_bits(ma.vertex_colors[:nv], mb.vertex_colors[:nv])


def test_fuse_frames_equals_a_volume_integrated_by_hand(scene):
    coords = stored(scene)
    volume_before, log_before = scene.volume, [list(c) for c in scene._tsdf_log]
    fused = scene.fuse_frames()
    voxel, trunc = VOLUME_PARAMS[scene.data]
    H, W = scene.image_resolution
    Ts = [scene.transform_grid[c[0]][c[1]]["T"] for c in coords]
    lo, hi = frustum_bounds(scene.K, Ts, H, W, scene._Z_RANGE[scene.data][1], margin=trunc + voxel * UNIT)
    hand = TsdfVolume(voxel, trunc, lo, hi, DEV, color=True, memory_budget_bytes=scene.tsdf_memory_budget_bytes)
    for c, T in zip(coords, Ts):
        hand.integrate(scene.frames[c]["depth"], scene.K, T, rgb_u8=scene.frames[c]["rgb_u8"])
    assert fused is not scene.volume and fused.brick_color is not None and fused.frame_id == 3
    assert same_volume(fused, hand) and same_mesh(fused, hand)
    identity = scene.fuse_frames(pose_corrections={c: np.eye(4) for c in coords})
    assert same_volume(identity, fused) and same_mesh(identity, fused)
    assert scene.fuse_frames(color=False, frames=coords[:2]).brick_color is None
    assert scene.volume is volume_before and [list(c) for c in scene._tsdf_log] == log_before


def test_fused_plane_with_a_pose_pushed_along_the_optical_axis(scene, tmp_path):
    voxel = VOLUME_PARAMS[scene.data][0]
    push = 3 * voxel
    # 24.75 pixels of disparity per frame: the last frame sees a strip of the plane (20 voxels wide) that no other frame sees
    plane, coords, T_true = plane_scene(scene, 24.75, False, wrong=-push, wrong_along=2)
    last = coords[-1]
    C = np.linalg.inv(T_true) @ plane.transform_grid[last[0]][last[1]]["T"]
    # the tolerance tests/test_gpu_tsdf.py states for a fused surface against the depth it was fused from: half a voxel
    tolerance = 0.5 * voxel
    off = np.abs(plane.fuse_frames().extract_triangle_mesh()["vertices"][:, 2].astype(np.float64) - PLANE_DEPTH)
    fixed_volume = plane.fuse_frames(pose_corrections={last: C})
    on = np.abs(fixed_volume.extract_triangle_mesh()["vertices"][:, 2].astype(np.float64) - PLANE_DEPTH)
    print(scene.branch, f"fused plane, one pose pushed by {push}: uncorrected vertices off the plane by up to", off.max(), ", within half a voxel of the push:",
          int((np.abs(off - push) <= tolerance).sum()), "of", off.size, "; corrected: up to", on.max(), "tolerance", tolerance)
    assert on.size > 1000 and on.max() <= tolerance
    assert (np.abs(off - push) <= tolerance).sum() > 100 and off.max() > 4 * tolerance
    # the export: on either branch (a forward-splat scene has no volume of its own)
    out = plane.export_fused_mesh(str(tmp_path), pose_corrections={last: C}, clean={"min_triangles": 16})
    assert set(out) == {"fused_triangle_mesh.ply", "fused_triangle_mesh_clean.ply"}
    for name, n in out.items():
        back = pointcloud.read_triangle_mesh(os.path.join(str(tmp_path), name))
        assert back["triangles"].shape[0] == n > 0
    assert out["fused_triangle_mesh.ply"] == fixed_volume.extract_triangle_mesh()["triangles"].shape[0]
    assert np.abs(pointcloud.read_triangle_mesh(os.path.join(str(tmp_path), "fused_triangle_mesh.ply"))["vertices"][:, 2] - PLANE_DEPTH).max() <= tolerance
    with pytest.raises(ValueError, match="clean"):
        plane.export_fused_mesh(str(tmp_path), clean={"nonsense": 1})
