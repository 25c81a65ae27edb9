"""CPU: the point-splat RGB-D render's numpy twin (tests/points_oracle.py) — a frame seen from its own pose reproduces itself, the
z-test, the 3x3 fill rule — pointview.relative_transforms, and sgam_points_render_rgbd_f32's argument checks through raw ctypes.
The cases built here are the ones tests/test_gpu_pointview.py runs on the device."""
import ctypes
import os
import sys

import numpy as np
import pytest

from sgam_neurips22_amd import _lib, pointview
from sgam_neurips22_amd.inference_pipeline import InfiniteSceneGeneration, intrinsics

sys.path.insert(0, os.path.dirname(__file__))
import points_oracle as PO  # noqa: E402

f32 = np.float32


def _bits(a):
    return np.ascontiguousarray(a, dtype=f32).view(np.uint32)


def k4(K):
    """fx, fy, cx, cy as the launcher receives them: fp32"""
    return tuple(f32(v) for v in (K[0, 0], K[1, 1], K[0, 2], K[1, 2]))


def small_pose(rs, rot=0.06, trans=0.15):
    """a world -> camera 4x4 near the identity: small random rotation (axis-angle) and translation"""
    w = rs.uniform(-rot, rot, 3)
    th = np.linalg.norm(w)
    k = w / th
    Kx = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    T = np.eye(4)
    T[:3, :3] = np.eye(3) + np.sin(th) * Kx + (1 - np.cos(th)) * Kx @ Kx
    T[:3, 3] = rs.uniform(-trans, trans, 3)
    return T


def identity_case(data, Hs, Ws, seed=0):
    """one frame at its own pose: depths inside the dataset's z range, seeded with values that must be skipped"""
    rs = np.random.RandomState(seed)
    z0, z1 = InfiniteSceneGeneration._Z_RANGE[data]
    depth = rs.uniform(z0 * 1.05, z1 * 0.95, (Hs, Ws)).astype(f32)
    flat = depth.reshape(-1)
    bad = rs.choice(flat.size, 12, replace=False)
    flat[bad] = np.array([0, -1.5, np.nan, np.inf, -np.inf, z0 * 0.5, z1 * 1.5, 0, np.nan, z1 * 2, -0.0, z0 * 0.9], dtype=f32)
    flat[rs.choice(flat.size, 4, replace=False)] = [f32(z0), f32(z1), np.nextafter(f32(z0), f32(0)), np.nextafter(f32(z1), f32(np.inf))]
    rgb = rs.randint(0, 256, (Hs, Ws, 3)).astype(np.uint8)
    K = intrinsics(data, (Hs, Ws))
    T = small_pose(rs, 0.5, 3.0)
    return dict(depths=[depth], rgbs=[rgb], K_src=K, K_view=K, Ts_src=[T], Ts_view=[T], H=Hs, W=Ws, z_near=z0, z_far=z1)


def check_identity(case, out):
    """every valid in-range pixel returns its own depth bits, colour and index; every other sample is empty"""
    d, rgb = case["depths"][0], case["rgbs"][0]
    Hs, Ws = d.shape
    with np.errstate(invalid="ignore"):
        valid = np.isfinite(d) & (d > 0) & (d >= f32(case["z_near"])) & (d <= f32(case["z_far"]))
    assert valid.sum() >= d.size - 16 and (~valid).sum() >= 8
    q = np.arange(Hs * Ws, dtype=np.int32).reshape(Hs, Ws)
    assert np.array_equal(out["index"][0], np.where(valid, q, -1))
    assert np.array_equal(_bits(out["depth"][0]), _bits(np.where(valid, d, f32(0))))
    assert np.array_equal(out["rgb_u8"][0], np.where(valid[..., None], rgb, 0))
    assert np.array_equal(_bits(out["rgb"][0]), _bits(np.where(valid[..., None], rgb, 0).astype(f32)))


def twin(case, radius=0, hole_fill=False, T_rel=None):
    if T_rel is None:
        T_rel = pointview.relative_transforms(case["Ts_view"], case["Ts_src"])
    return PO.render(case["depths"], case["rgbs"], PO.kinv32(case["K_src"]), T_rel, case["H"], case["W"], *k4(case["K_view"]),
                     case["z_near"], case["z_far"], radius, hole_fill)


def edge_case(F=3, Hs=24, Ws=40, P=2, H=37, W=53, seed=3):
    """F sources and P views near each other, no size a multiple of 16; the view's K is the source's scaled to the view size; the
    depths are seeded with 0, negative, NaN, +inf, values that land outside [z_near, z_far] and values that land behind the camera"""
    rs = np.random.RandomState(seed)
    K = np.array([[31.0, 0, (Ws - 1) / 2], [0, 29.5, (Hs - 1) / 2], [0, 0, 1]])
    Kv = np.diag([W / Ws, H / Hs, 1.0]) @ K
    depths, rgbs = [], []
    yy, xx = np.meshgrid(np.linspace(0, 1, Hs), np.linspace(0, 1, Ws), indexing="ij")
    for f in range(F):
        d = (2.2 + 0.8 * np.sin(3 * xx + f) * np.cos(2 * yy - f) + rs.uniform(-0.05, 0.05, (Hs, Ws))).astype(f32)
        flat = d.reshape(-1)
        bad = rs.choice(flat.size, 40, replace=False)
        flat[bad] = np.resize(np.array([0, -2.0, np.nan, np.inf, 0.6, 9.0, 0.2, 0.1], dtype=f32), 40)
        depths.append(d)
        rgbs.append(rs.randint(0, 256, (Hs, Ws, 3)).astype(np.uint8))
    Ts_src = [small_pose(rs) for _ in range(F)]
    Ts_view = [small_pose(rs) for _ in range(P)]
    Ts_view[-1][2, 3] -= 0.45             # the last view stands 0.45 ahead: the points seeded at depth 0.1 / 0.2 are behind it
    return dict(depths=depths, rgbs=rgbs, K_src=K, K_view=Kv, Ts_src=Ts_src, Ts_view=Ts_view, H=H, W=W, z_near=1.0, z_far=5.0)


@pytest.mark.parametrize("data", ["google_earth", "clevr-infinite"])
@pytest.mark.parametrize("size", [(256, 256), (128, 128), (48, 40)])
def test_twin_reproduces_a_frame_at_its_own_pose(data, size):
    case = identity_case(data, *size)
    T_rel = pointview.relative_transforms(case["Ts_view"], case["Ts_src"])
    assert np.array_equal(T_rel[0, 0], np.eye(4, dtype=f32)[:3])
    check_identity(case, twin(case, T_rel=T_rel))


def test_twin_keeps_the_nearer_of_two_planes():
    Hs, Ws = 20, 28
    K = np.array([[25.0, 0, 13.5], [0, 25.0, 9.5], [0, 0, 1]])
    rs = np.random.RandomState(1)
    rgbs = [rs.randint(0, 256, (Hs, Ws, 3)).astype(np.uint8) for _ in range(2)]
    for near in (0, 1):
        depths = [np.full((Hs, Ws), 2.0 if f == near else 3.0, dtype=f32) for f in range(2)]
        case = dict(depths=depths, rgbs=rgbs, K_src=K, K_view=K, Ts_src=[np.eye(4)] * 2, Ts_view=[np.eye(4)], H=Hs, W=Ws, z_near=0.5,
                    z_far=5.0)
        out = twin(case)
        q = np.arange(Hs * Ws).reshape(Hs, Ws)
        assert (out["depth"][0] == f32(2.0)).all() and np.array_equal(out["index"][0], near * Hs * Ws + q)
        assert np.array_equal(out["rgb_u8"][0], rgbs[near])


def test_edge_case_twin_has_hits_holes_and_skipped_points():
    case = edge_case()
    plain, filled = twin(case), twin(case, hole_fill=True)
    hit = plain["index"] >= 0
    assert 0.2 < hit.mean() < 0.9                                     # hits and holes
    assert np.array_equal(filled["index"], plain["index"])
    assert np.array_equal(_bits(filled["depth"][hit]), _bits(plain["depth"][hit])) and np.array_equal(filled["rgb"][hit], plain["rgb"][hit])
    assert ((filled["depth"] > 0) & ~hit).sum() > 20                  # the fill closes holes, and only holes change
    assert (plain["depth"][hit] >= f32(1.0)).all() and (plain["depth"][hit] <= f32(5.0)).all()
    wide = twin(case, radius=2)
    assert (wide["index"] >= 0).mean() > hit.mean() + 0.1
    # the seeded points are skipped: none of their ids is seen
    seen = set(np.unique(wide["index"][wide["index"] >= 0]).tolist())
    Hs, Ws = case["depths"][0].shape
    for f, d in enumerate(case["depths"]):
        with np.errstate(invalid="ignore"):
            never = ~(np.isfinite(d) & (d > 0)) | (d > 8)
        assert never.sum() >= 25 and not seen & set((f * Hs * Ws + np.flatnonzero(never.ravel())).tolist())


def test_fill_rule_on_hand_made_windows():
    def run(hits, H=3, W=3):
        """hits: {(y, x): value}; channels r, g, b, depth = value, value + 1, value + 2, value / 100"""
        depth, rgb, empty = np.zeros((H, W), f32), np.zeros((H, W, 3), f32), np.ones((H, W), bool)
        for (y, x), v in hits.items():
            depth[y, x], rgb[y, x], empty[y, x] = v / 100, (v, v + 1, v + 2), False
        d, c = PO.fill(depth, rgb, empty)
        for (y, x), v in hits.items():                                  # hit samples untouched
            assert d[y, x] == f32(v / 100) and tuple(c[y, x]) == (v, v + 1, v + 2)
        return d, c

    ring = [(0, 0), (0, 1), (0, 2), (1, 0), (1, 2), (2, 0), (2, 1), (2, 2)]
    d, c = run({p: 10 * (k + 1) for k, p in enumerate(ring[:4])})       # 4 hit neighbours: stays 0
    assert d[1, 1] == 0 and (c[1, 1] == 0).all()
    d, c = run({p: 10 * (k + 1) for k, p in enumerate(ring[:5])})       # 5 hit neighbours: 4 zeros below them -> the smallest hit
    assert d[1, 1] == f32(0.1) and tuple(c[1, 1]) == (10, 11, 12)
    d, c = run({p: 10 * (8 - k) for k, p in enumerate(ring)})           # 8 hit neighbours: one zero, then the 4th smallest hit
    assert d[1, 1] == f32(0.4) and tuple(c[1, 1]) == (40, 41, 42)
    # per channel: the medians of different channels may come from different neighbours
    depth, rgb, empty = np.zeros((3, 3), f32), np.zeros((3, 3, 3), f32), np.ones((3, 3), bool)
    for k, (y, x) in enumerate(ring[:5]):
        depth[y, x], rgb[y, x], empty[y, x] = 1 + k, (50 - k, 7, 9 + k), False
    d, c = PO.fill(depth, rgb, empty)
    assert d[1, 1] == 1 and tuple(c[1, 1]) == (46, 7, 9)
    # borders: a corner has at most 3 neighbours (stays 0); an edge sample with all 5 of its neighbours hit takes the smallest
    full = {(y, x): 10 + 3 * y + x for y in range(4) for x in range(4)}
    corner = dict(full)
    del corner[(0, 0)]
    d, c = run(corner, 4, 4)
    assert d[0, 0] == 0 and (c[0, 0] == 0).all()
    edge = dict(full)
    del edge[(0, 2)]
    d, c = run(edge, 4, 4)
    assert d[0, 2] == f32(0.11) and tuple(c[0, 2]) == (11, 12, 13)
    del edge[(1, 2)]                                                    # now 4 of them: stays 0, and so does the new hole (7 hits, two zeros -> the 3rd smallest hit)
    d, c = run(edge, 4, 4)
    assert d[0, 2] == 0 and d[1, 2] == f32(0.14)


def test_relative_transforms():
    rs = np.random.RandomState(5)
    src = [small_pose(rs, 0.8, 4.0) for _ in range(5)]
    view = [small_pose(rs, 0.8, 4.0) for _ in range(3)] + [src[3].copy()]
    got = pointview.relative_transforms(view, src)
    assert got.shape == (4, 5, 3, 4) and got.dtype == f32
    for p, V in enumerate(view):
        for f, S in enumerate(src):
            if p == 3 and f == 3:
                assert np.array_equal(got[p, f], np.eye(4, dtype=f32)[:3])          # the exact identity, not a rounded product
            else:
                assert np.array_equal(got[p, f], (V @ np.linalg.inv(S))[:3].astype(f32))
    assert np.array_equal(pointview.relative_transforms(np.stack(view), np.stack(src)), got)


def test_points_render_argument_validation_without_gpu():
    lib = _lib.load()
    assert lib.sgam_abi_version() == 10                                 # additive: the ABI version stays
    for name in ("sgam_points_render_rgbd_workspace_bytes", "sgam_points_render_rgbd_f32"):
        assert name in _lib.PROTOTYPES and hasattr(lib, name)
    size = lib.sgam_points_render_rgbd_workspace_bytes
    assert size(2, 37, 53, 0) == size(2, 37, 53, 1) == 2 * 37 * 53 * 8
    assert size(65535, 4, 4, 1) == 65535 * 4 * 4 * 8
    for bad in ((0, 8, 8, 0), (65536, 8, 8, 0), (-1, 8, 8, 0), (1, 0, 8, 0), (1, 8, 0, 0), (1, 8, -3, 1), (1, 8, 8, 2), (1, 8, 8, -1),
                (1, 1 << 16, 1 << 15, 0)):
        assert size(*bad) == -1, bad
    raw = ctypes.CDLL(_lib.LIB_PATH).sgam_points_render_rgbd_f32          # raw ctypes: own prototypes
    raw.restype = ctypes.c_int
    vp, i32, fl = ctypes.c_void_p, ctypes.c_int32, ctypes.c_float
    raw.argtypes = [vp, vp, i32, i32, i32, vp, vp, i32, i32, i32, fl, fl, fl, fl, fl, fl, i32, i32, vp, vp, vp, vp, vp, ctypes.c_int64, vp]
    # fake non-null pointers are never dereferenced: every check comes before the first device call (and before Kinv is read)
    p = vp(64)
    ws = 2 * 8 * 8 * 8

    def call(depth_ptrs=p, rgb_ptrs=p, F=3, Hs=6, Ws=5, Kinv=p, T_rel=p, P=2, H=8, W=8, z_near=0.1, z_far=4.0, radius=1, hole_fill=1,
             depth_out=p, workspace=p, ws_bytes=ws):
        return raw(depth_ptrs, rgb_ptrs, F, Hs, Ws, Kinv, T_rel, P, H, W, 10.0, 10.0, 4.0, 4.0, z_near, z_far, radius, hole_fill,
                   depth_out, None, None, None, workspace, ws_bytes, None)

    bad = [dict(P=0), dict(P=-2), dict(P=65536, ws_bytes=1 << 40), dict(F=0), dict(F=-1), dict(Hs=0), dict(Ws=-4), dict(H=0), dict(W=0),
           dict(F=1 << 16, Hs=1 << 8, Ws=1 << 8),                       # F * Hs * Ws = 2^32: the point id would not fit 32 bits
           dict(F=70000, Hs=300, Ws=300), dict(radius=-1), dict(radius=3), dict(z_near=0.0), dict(z_near=-1.0), dict(z_near=float("nan")),
           dict(z_far=0.1), dict(z_far=0.05), dict(z_far=float("nan")), dict(hole_fill=2), dict(depth_ptrs=None), dict(rgb_ptrs=None),
           dict(Kinv=None), dict(T_rel=None), dict(depth_out=None), dict(workspace=None), dict(ws_bytes=ws - 1), dict(ws_bytes=0),
           dict(workspace=vp(68))]                                      # not 8-byte aligned
    for kw in bad:
        assert call(**kw) == -1, kw
