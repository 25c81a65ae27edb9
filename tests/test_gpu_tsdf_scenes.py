"""GPU: the scene-batched TSDF kernels (tsdf.integrate_many_scenes / render_depth_scenes; csrc/tsdf.hip) — S volumes on one grid
advanced through one launch sequence must be left, scene by scene, with what each volume's own integrate_many / render_depth
leaves: bit for bit (bricks may sit at other pool indices, so volumes are compared through their key-sorted zero crossings and
ray casts, not through the raw pools)."""
import os
import sys

import numpy as np
import pytest
import torch

from sgam_neurips22_amd import ops, tsdf
from sgam_neurips22_amd.tsdf import TsdfVolume, frustum_bounds

sys.path.insert(0, os.path.dirname(__file__))
from test_tsdf_cpu import _K, _pose  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda"
VOXEL, TRUNC = 0.05, 0.5              # CLEVR's volume (tsdf.VOLUME_PARAMS)
Z_NEAR, Z_FAR = 1.0, 16.5             # InfiniteSceneGeneration._Z_RANGE["clevr-infinite"]
STEPS = 2                             # the second step meets units the first one opened (stamp logic, no new brick)
POOL = 64 << 20                       # 2048 bricks: several times what two steps open


def _intr(H, W):
    K = _K(120.0, 0.0)
    K[0, 2], K[1, 2] = (W - 1) / 2, (H - 1) / 2
    return K


def _src_pose(s, k, step):
    return _pose(tx=0.25 * k - 0.3 + 0.11 * s, ty=0.07 * s - 0.05 * step, tz=0.1 * step, yaw=0.04 * (k - 1) + 0.03 * s)


def _view_poses(s):
    return [_pose(tx=0.05 + 0.1 * s, ty=0.02, yaw=0.02), _pose(tx=-0.2, ty=0.1 * s, yaw=-0.05), _pose(tx=0.3, tz=0.2, yaw=0.06 - 0.02 * s)]


def _depth(s, k, step, H, W):
    """a tilted plane per scene + seeded bumps, inside the z range; some pixels 0 (no measurement), some beyond depth_trunc"""
    rs = np.random.RandomState(1000 * s + 10 * k + step)
    v, u = np.meshgrid(np.arange(H, dtype=np.float64), np.arange(W, dtype=np.float64), indexing="ij")
    d = 7.0 + 0.9 * s + 0.015 * (1 + 0.4 * s) * u - 0.01 * (s + 1) * v
    for _ in range(3):
        cu, cv, sig = rs.uniform(0, W), rs.uniform(0, H), rs.uniform(4, 10)
        d += rs.uniform(-0.4, 0.4) * np.exp(-((u - cu) ** 2 + (v - cv) ** 2) / (2 * sig ** 2))
    r = rs.rand(H, W)
    d[r < 0.03] = 0.0
    d[r > 0.98] = tsdf.DEPTH_TRUNC + 5.0
    assert Z_NEAR < d[(d > 0) & (d < tsdf.DEPTH_TRUNC)].min() and d[d < tsdf.DEPTH_TRUNC].max() < Z_FAR
    return d.astype(np.float32)


def _rgb(s, k, step, H, W):
    return np.random.RandomState(77 + 1000 * s + 10 * k + step).randint(0, 256, (H, W, 3)).astype(np.uint8)


def _box(H, W):
    poses = [_src_pose(s, k, t) for s in range(3) for k in range(5) for t in range(STEPS)] + [T for s in range(3) for T in _view_poses(s)]
    return frustum_bounds(_intr(H, W), poses, H, W, Z_FAR, margin=TRUNC + 16 * VOXEL)


def _volume(H, W, color=False, **kw):
    lo, hi = _box(H, W)
    kw.setdefault("memory_budget_bytes", POOL * (3 if color else 1))
    return TsdfVolume(VOXEL, TRUNC, lo, hi, DEV, color=color, **kw)


def _step_inputs(s, n, step, H, W, color=False):
    d = [torch.from_numpy(_depth(s, k, step, H, W)).to(DEV) for k in range(n)]
    T = [_src_pose(s, k, step) for k in range(n)]
    c = [torch.from_numpy(_rgb(s, k, step, H, W)).to(DEV) for k in range(n)] if color else None
    return d, T, c


_SOLO = {}


def _solo(s, n, H, W, color=False):
    """scene s fused by the per-volume entry point: the reference, made once per (scene, n, size) and only read afterwards"""
    key = (s, n, H, W, color)
    if key not in _SOLO:
        vol = _volume(H, W, color)
        for step in range(STEPS):
            d, T, c = _step_inputs(s, n, step, H, W, color)
            vol.integrate_many(d, _intr(H, W), T, rgbs_u8=c)
        _SOLO[key] = vol
    return _SOLO[key]


def _batched(scenes, n, H, W, color=False, volumes=None):
    vols = volumes or [_volume(H, W, color) for _ in scenes]
    for step in range(STEPS):
        ins = [_step_inputs(s, n, step, H, W, color) for s in scenes]
        tsdf.integrate_many_scenes(vols, [i[0] for i in ins], _intr(H, W), [i[1] for i in ins],
                                   rgbs_u8_per_scene=[i[2] for i in ins] if color else None)
    assert all(v.frame_id == STEPS for v in vols)
    return vols


def _bits(a):
    return np.ascontiguousarray(a.cpu().numpy() if torch.is_tensor(a) else a)


def _assert_same_volume(got, want, s, H, W):
    assert got.stats()[0] == want.stats()[0] > 0 and got.stats()[2:] == want.stats()[2:] == (0, 0)
    a, b = got.extract_point_cloud(), want.extract_point_cloud()
    assert len(b["keys"]) > 100
    assert np.array_equal(a["keys"], b["keys"])
    for name in ("points", "normals") + (("colors",) if "colors" in b else ()):
        assert np.array_equal(a[name].view(np.uint32), b[name].view(np.uint32)), name
    assert ("colors" in a) == ("colors" in b)
    K = _intr(H, W)
    for T in _view_poses(s):
        ra, rb = _bits(got.render_depth(K, T, H, W, Z_NEAR, Z_FAR)), _bits(want.render_depth(K, T, H, W, Z_NEAR, Z_FAR))
        assert (rb > 0).mean() > 0.3                 # (the reference sees the surface at all)
        assert np.array_equal(ra.view(np.uint32), rb.view(np.uint32))


@pytest.mark.parametrize("n", [1, 3, 5])
@pytest.mark.parametrize("S", [1, 3])
def test_batched_scenes_equal_their_own_volumes(S, n):
    H = W = 64
    vols = _batched(range(S), n, H, W)
    for s, v in enumerate(vols):
        _assert_same_volume(v, _solo(s, n, H, W), s, H, W)
    # one ray-cast launch for the S volumes at S different poses against S single ray casts
    K = _intr(H, W)
    for j in range(3):
        Ts = [_view_poses(s)[(j + s) % 3] for s in range(S)]
        got = tsdf.render_depth_scenes(vols, K, Ts, H, W, Z_NEAR, Z_FAR)
        assert got.shape == (S, H, W)
        for s in range(S):
            want = _bits(_solo(s, n, H, W).render_depth(K, Ts[s], H, W, Z_NEAR, Z_FAR))
            assert np.array_equal(_bits(got[s]).view(np.uint32), want.view(np.uint32)), (j, s)
    out = torch.empty((S, H, W), device=DEV)
    assert tsdf.render_depth_scenes(vols, K, Ts, H, W, Z_NEAR, Z_FAR, Ts_c2w=[np.linalg.inv(T) for T in Ts], out=out) is out
    assert torch.equal(out, got)


def test_colour_is_fused_per_scene():
    H = W = 64
    vols = _batched(range(2), 2, H, W, color=True)
    for s, v in enumerate(vols):
        _assert_same_volume(v, _solo(s, 2, H, W, color=True), s, H, W)
    with pytest.raises(ValueError, match="colour"):
        tsdf.integrate_many_scenes([vols[0], _volume(H, W)], [[], []], _intr(H, W), [[], []])


def test_an_exhausted_pool_stays_its_own_scenes_problem():
    H = W = 64
    vols = [_volume(H, W), _volume(H, W, max_bricks=5), _volume(H, W)]
    _batched(range(3), 3, H, W, volumes=vols)
    assert vols[1].stats()[0] >= 5 and vols[1].stats()[3] > 0
    with pytest.raises(ops.SgamHipError, match="pool exhausted"):
        vols[1].check()
    for s in (0, 2):
        assert vols[s].check() == _solo(s, 3, H, W).stats()[0]
        _assert_same_volume(vols[s], _solo(s, 3, H, W), s, H, W)


def test_scene_indexing_on_non_square_frames():
    """48 x 64 frames, every scene with its own depths and its own poses: a scene index used for the wrong table, or a plane
    offset computed with the wrong extent, changes some scene's result"""
    H, W, S, n = 48, 64, 3, 3
    for step in range(STEPS):
        for a in range(S):
            for b in range(a + 1, S):
                for k in range(n):
                    assert not np.array_equal(_depth(a, k, step, H, W), _depth(b, k, step, H, W))
                    assert np.abs(_src_pose(a, k, step) - _src_pose(b, k, step)).max() > 0.01
    vols = _batched(range(S), n, H, W)
    for s, v in enumerate(vols):
        _assert_same_volume(v, _solo(s, n, H, W), s, H, W)
    K = _intr(H, W)
    Ts = [_view_poses(s)[0] for s in range(S)]
    got = tsdf.render_depth_scenes(vols, K, Ts, H, W, Z_NEAR, Z_FAR)
    for s in range(S):
        assert np.array_equal(_bits(got[s]).view(np.uint32), _bits(_solo(s, n, H, W).render_depth(K, Ts[s], H, W, Z_NEAR, Z_FAR)).view(np.uint32))
    assert not torch.equal(got[0], got[1]) and not torch.equal(got[1], got[2])


def test_validation():
    H = W = 64
    K = _intr(H, W)
    a = _volume(H, W, max_bricks=16)
    lo, hi = _box(H, W)
    b = TsdfVolume(VOXEL, TRUNC, lo, hi + 2.0, DEV, max_bricks=16)               # another box of units
    c = TsdfVolume(VOXEL, 0.4, lo, hi, DEV, max_bricks=16)                       # another truncation
    d1, T1, _ = _step_inputs(0, 1, 0, H, W)
    for other in (b, c):
        with pytest.raises(ValueError, match="must share"):
            tsdf.integrate_many_scenes([a, other], [d1, d1], K, [T1, T1])
        with pytest.raises(ValueError, match="must share"):
            tsdf.render_depth_scenes([a, other], K, [T1[0], T1[0]], H, W, Z_NEAR, Z_FAR)
    with pytest.raises(ops.SgamHipError, match="SGAM_EINVAL"):                   # the library's n_src <= 8
        tsdf.integrate_many_scenes([a], [d1 * 9], K, [T1 * 9])
    with pytest.raises(ops.SgamHipError):                                        # S = 0: refused before anything is launched
        tsdf.integrate_many_scenes([], [], K, [])
    with pytest.raises(ops.SgamHipError):
        tsdf.render_depth_scenes([], K, [], H, W, Z_NEAR, Z_FAR)
    assert a.frame_id == 0 and a.stats() == (0, 0, 0, 0)                         # nothing ran, no step was counted
