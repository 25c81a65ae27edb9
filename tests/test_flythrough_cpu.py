"""CPU: the fly-through's host side — flythrough_poses (end points, orthonormality, count, slerp), the coloured rasteriser's
numpy restatement (tests/mesh_color_oracle.py) against tests/mc_oracle.py, and sgam_mesh_render_rgbd_f32's argument checks.
The fixtures here are shared with tests/test_gpu_flythrough.py."""
import ctypes
import os
import sys

import numpy as np

from sgam_neurips22_amd import _lib
from sgam_neurips22_amd.inference_pipeline import InfiniteSceneGeneration, _quat_from_rot, _rot_from_quat, _slerp, intrinsics

sys.path.insert(0, os.path.dirname(__file__))
import mc_oracle  # noqa: E402
import mesh_color_oracle  # noqa: E402
from test_tsdf_cpu import _K, _pose  # noqa: E402


# ---------------------------------------------------------------- fixtures
def random_meshes():
    """the three random meshes of test_gpu_mesh.test_rasteriser_is_bit_exact_against_numpy_on_small_meshes (40 x 48, 60 vertices,
    <= 80 triangles, the third with z_near = 0.5 cutting through), with random vertex colours in 0..255 (a generator of their
    own: the geometry stream is that test's)"""
    H, W = 40, 48
    K = _K(40.0, 20.0)
    K[0, 2] = 23.5
    rs, rc = np.random.RandomState(3), np.random.RandomState(7)
    T = _pose(tx=0.1, ty=-0.05, yaw=0.03)
    out = []
    for trial in range(3):
        n = 60
        v = np.stack([rs.uniform(-1.5, 1.5, n), rs.uniform(-1.2, 1.2, n), rs.uniform(0.2 if trial else 1.0, 4.0, n)], 1).astype(np.float32)
        tri = rs.randint(0, n, size=(80, 3)).astype(np.int32)
        tri = tri[(tri[:, 0] != tri[:, 1]) & (tri[:, 1] != tri[:, 2]) & (tri[:, 0] != tri[:, 2])]
        col = rc.uniform(0, 255, size=(n, 3)).astype(np.float32)
        out.append(dict(v=v, col=col, tri=tri, T=T, K=K, H=H, W=W, z_near=0.5 if trial == 2 else 0.1, z_far=3.5))
    return out


PLANE_COLOUR = np.array([[127.5, 100.0, 50.0], [100.0, -60.0, 40.0], [30.0, 20.0, -10.0]])      # channel = c0 + cx * x + cy * y


def plane_fixture():
    """one quad in the world plane z = 2 whose vertex colours are a linear function of world x and y, seen at a 30 degree yaw
    from a camera that looks at its centre (view-space z from 1.6 to 2.4 across it), 32 x 32, nothing clipped at z_near = 0.1"""
    H = W = 32
    K = _K(24.0, 15.5)
    yaw = np.pi / 6
    T = _pose(tx=-2.0 * np.sin(yaw), tz=2.0 - 2.0 * np.cos(yaw), yaw=yaw)
    v = np.array([[-0.8, -0.8, 2.0], [0.8, -0.8, 2.0], [0.8, 0.8, 2.0], [-0.8, 0.8, 2.0]], dtype=np.float32)
    col = (PLANE_COLOUR[:, 0][None] + v[:, :1].astype(np.float64) * PLANE_COLOUR[:, 1][None]
           + v[:, 1:2].astype(np.float64) * PLANE_COLOUR[:, 2][None]).astype(np.float32)
    tri = np.array([[0, 1, 2], [0, 2, 3]], dtype=np.int32)
    return dict(v=v, col=col, tri=tri, T=T, K=K, H=H, W=W, z_near=0.1, z_far=10.0)


def plane_colour_fp64(fx):
    """the fp64 colour at the intersection of every sample's ray with the plane z = 2, for the pose as the kernel gets it (fp32)"""
    T = np.asarray(fx["T"], dtype=np.float32).astype(np.float64)
    K = np.asarray(fx["K"], dtype=np.float32).astype(np.float64)
    c2w = np.linalg.inv(T)
    v, u = np.meshgrid(np.arange(fx["H"]), np.arange(fx["W"]), indexing="ij")
    d = np.stack([(u - K[0, 2]) / K[0, 0], (v - K[1, 2]) / K[1, 1], np.ones(u.shape)], -1) @ c2w[:3, :3].T
    t = (2.0 - c2w[2, 3]) / d[..., 2]
    p = c2w[:3, 3] + t[..., None] * d
    return PLANE_COLOUR[:, 0] + p[..., :1] * PLANE_COLOUR[:, 1] + p[..., 1:2] * PLANE_COLOUR[:, 2]


def oracle(fx, T=None, **kw):
    return mesh_color_oracle.rasterise_rgbd(fx["v"], fx["col"], fx["tri"], fx["T"] if T is None else T, fx["K"], fx["H"], fx["W"],
                                            fx["z_near"], fx["z_far"], **kw)


# ---------------------------------------------------------------- flythrough_poses
def _bare(data="google_earth", dims=(5, 1)):
    s = InfiniteSceneGeneration.__new__(InfiniteSceneGeneration)
    s.data, s.step_size_denom, s.K, s.output_dim = data, 2, intrinsics(data), dims
    s.anchor_poses, s.grid_transform_path, s.trajectory_shape = {}, None, "grid"
    return s


def test_flythrough_poses_end_points_count_and_orthonormality():
    s = _bare(dims=(6, 1))
    s.prepare_ring((6, 1), {}, horizontal_offset=0.002)          # a pose set whose rotation changes from node to node
    s._ordered_grid_coords = s.zig_zag_order()
    for c in s._ordered_grid_coords[:4]:
        s.transform_grid[c[0]][c[1]]["visited"] = True
    for n_between in (0, 1, 4):
        P = s.flythrough_poses(n_between=n_between)
        assert P.shape == ((4 - 1) * (n_between + 1) + 1, 4, 4) and P.dtype == np.float64
        for k, c in enumerate(s._ordered_grid_coords[:4]):
            assert np.array_equal(P[k * (n_between + 1)], s.transform_grid[c[0]][c[1]]["T"])       # bit for bit
        # every interpolated pose is orthonormal to 1e-12 (the end points are the nodes' own matrices, bit for bit as asserted
        # above: the pose set's start pose is orthonormal to ~1e-8 only, and they are not re-normalised)
        for k, T in enumerate(P):
            if k % (n_between + 1):
                assert np.abs(T[:3, :3] @ T[:3, :3].T - np.eye(3)).max() <= 1e-12 and abs(np.linalg.det(T[:3, :3]) - 1) <= 1e-12
            assert np.array_equal(T[3], [0, 0, 0, 1])
    # in between: the camera centre moves on the chord, the rotation on the arc, both monotonically
    P = s.flythrough_poses(n_between=3)
    a, b = P[0], P[4]
    ca, cb = -a[:3, :3].T @ a[:3, 3], -b[:3, :3].T @ b[:3, 3]
    assert not np.allclose(a[:3, :3], b[:3, :3])
    for k in range(1, 4):
        c = -P[k][:3, :3].T @ P[k][:3, 3]
        assert np.allclose(c, ca + k / 4 * (cb - ca), atol=1e-12, rtol=0)
        ang = np.arccos(np.clip((np.trace(a[:3, :3].T @ P[k][:3, :3]) - 1) / 2, -1, 1))
        full = np.arccos(np.clip((np.trace(a[:3, :3].T @ b[:3, :3]) - 1) / 2, -1, 1))
        assert abs(ang - k / 4 * full) <= 1e-6          # (the end points' own 1e-8)
    # an explicit order
    order = [(3, 0), (0, 0)]
    P = s.flythrough_poses(n_between=2, order=order)
    assert len(P) == 4 and np.array_equal(P[0], s.transform_grid[3][0]["T"]) and np.array_equal(P[-1], s.transform_grid[0][0]["T"])


def test_slerp_between_equal_rotations_is_that_rotation():
    rs = np.random.RandomState(0)
    for _ in range(20):
        q = rs.randn(4)
        R = _rot_from_quat(q / np.linalg.norm(q))
        qa = _quat_from_rot(R)
        assert np.abs(_rot_from_quat(qa) - R).max() <= 1e-12
        for s in (0.0, 0.3, 1.0):
            assert np.abs(_rot_from_quat(_slerp(qa, qa.copy(), s)) - R).max() <= 1e-12
            assert np.abs(_rot_from_quat(_slerp(qa, -qa, s)) - R).max() <= 1e-12           # q and -q: the same rotation
    # half way between the identity and a quarter turn about y: an eighth turn
    Ry = lambda a: np.array([[np.cos(a), 0, np.sin(a)], [0, 1, 0], [-np.sin(a), 0, np.cos(a)]])  # noqa: E731
    mid = _rot_from_quat(_slerp(_quat_from_rot(np.eye(3)), _quat_from_rot(Ry(np.pi / 2)), 0.5))
    assert np.abs(mid - Ry(np.pi / 4)).max() <= 1e-12


# ---------------------------------------------------------------- the coloured oracle
def test_coloured_oracle_depth_equals_the_depth_oracle():
    for trial, fx in enumerate(random_meshes()):
        want = mc_oracle.rasterise(fx["v"], fx["tri"], fx["T"], fx["K"], fx["H"], fx["W"], fx["z_near"], fx["z_far"])
        depth, rgb, win = oracle(fx)
        assert (want > 0).mean() > 0.2
        assert np.array_equal(depth.view(np.uint32), want.view(np.uint32)), trial
        assert np.array_equal(win >= 0, depth > 0) and (rgb[win < 0] == 0).all()
        # every colour lies within its triangle's vertex colours
        t = win[win >= 0] >> 1
        c = fx["col"][fx["tri"][t]]
        assert (rgb[win >= 0] >= c.min(1)).all() and (rgb[win >= 0] <= c.max(1)).all()
    assert (win[win >= 0] & 1).any()                 # the clipping trial shows second halves of clipped quads


def test_coloured_oracle_takes_every_sample_of_a_shared_edge_from_one_triangle():
    K = np.array([[10.0, 0, 4.0], [0, 10.0, 4.0], [0, 0, 1]])
    z = 2.0
    sq = np.array([[-0.8, -0.8, z], [0.8, -0.8, z], [0.8, 0.8, z], [-0.8, 0.8, z]], dtype=np.float32)
    v = sq[[0, 1, 2, 0, 2, 3]]                        # two triangles sharing the diagonal through the samples (k, k)
    red, blue = np.array([255.0, 0, 0], dtype=np.float32), np.array([0, 0, 255.0], dtype=np.float32)
    col = np.stack([red] * 3 + [blue] * 3)
    depth, rgb, win = mesh_color_oracle.rasterise_rgbd(v, col, np.array([[0, 1, 2], [3, 4, 5]]), np.eye(4), K, 9, 9, 0.1, 10.0)
    assert (depth[0:8, 0:8] == np.float32(z)).all() and (depth[8, :] == 0).all() and (depth[:, 8] == 0).all()
    is_red, is_blue = (rgb == red).all(-1), (rgb == blue).all(-1)
    assert ((is_red ^ is_blue) == (depth > 0)).all()             # exactly one triangle's colour, never a mixture
    assert np.array_equal(is_red, win == 0) and np.array_equal(is_blue, win == 2)
    assert is_red.sum() > 10 and is_blue.sum() > 10
    # an exact z tie (the same triangle twice): the lower index keeps the sample
    col2 = np.stack([red] * 3 + [blue] * 3)
    _, rgb2, win2 = mesh_color_oracle.rasterise_rgbd(sq[[0, 1, 2, 0, 1, 2]], col2, np.array([[0, 1, 2], [3, 4, 5]]), np.eye(4), K, 9, 9, 0.1, 10.0)
    assert (win2[win2 >= 0] == 0).all() and (rgb2[win2 >= 0] == red).all()


def test_affine_interpolation_fails_the_analytic_plane():
    """the fixture of the GPU test tells perspective-correct from screen-space interpolation: the oracle's affine variant is off
    by more than 1.0 of 255 somewhere, the perspective-correct one stays within 1e-3 * 255"""
    fx = plane_fixture()
    want = plane_colour_fp64(fx)
    depth, rgb, _ = oracle(fx)
    hit = depth > 0
    assert hit.sum() > 200
    err = np.abs(rgb.astype(np.float64) - want)[hit].max()
    _, affine, _ = oracle(fx, perspective=False)
    err_affine = np.abs(affine.astype(np.float64) - want)[hit].max()
    print(f"analytic plane (oracle): perspective-correct max |err| {err:.3e}, affine {err_affine:.3f}")
    assert err <= 1e-3 * 255 and err_affine > 1.0


# ---------------------------------------------------------------- argument checks
def test_rgbd_render_argument_validation_without_gpu():
    lib = _lib.load()
    assert lib.sgam_mesh_render_rgbd_workspace_bytes(2, 40, 48) == 2 * 40 * 48 * 8
    assert lib.sgam_mesh_render_rgbd_workspace_bytes(0, 40, 48) == -1
    assert lib.sgam_mesh_render_rgbd_workspace_bytes(1, 0, 48) == -1
    # a fake non-null device pointer is never dereferenced: argument checks come first
    p = ctypes.c_void_p(16)
    ws = 2 * 8 * 8 * 8

    def call(P=2, max_t=16, ws_bytes=ws, colors=p, rgb=p, z_near=0.1, workspace=p):
        return lib.sgam_mesh_render_rgbd_f32(p, colors, 16, p, max_t, p, P, 8, 8, 10.0, 10.0, 4.0, 4.0, p, z_near, 4.0, p, rgb, None, None,
                                             workspace, ws_bytes, None)

    assert call(P=0) == -1
    assert call(ws_bytes=ws - 1) == -1                  # a workspace that is too small
    assert call(workspace=None) == -1
    assert call(max_t=1 << 30) == -1                    # the fragment id would not fit 31 bits
    assert call(max_t=(1 << 30) + 5) == -1
    assert call(colors=None) == -1                      # colour asked of a mesh without colours
    assert call(z_near=0.0) == -1
    assert lib.sgam_mesh_render_rgbd_f32(None, None, 16, None, 16, None, 1, 8, 8, 10.0, 10.0, 4.0, 4.0, None, 0.1, 4.0, None, None, None,
                                         None, None, 0, None) == -1
    assert lib.sgam_abi_version() == 10                 # additive: the ABI version stays
