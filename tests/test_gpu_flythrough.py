"""GPU: the coloured RGB-D mesh render (csrc/mesh_raster.hip: sgam_mesh_render_rgbd_f32 through tsdf.render_mesh_rgbd) — bit-equal
to the depth render and to the numpy restatement (tests/mesh_color_oracle.py), the tie rule, perspective-correct interpolation
against an analytic plane, near clipping of colours, a fused colour volume, and the scene-level fly-through (render_views)."""
import os
import sys

import numpy as np
import pytest
import torch

from sgam_neurips22_amd import _lib, ops, testing, tsdf
from sgam_neurips22_amd.tsdf import DeviceMesh, TsdfVolume, frustum_bounds, render_mesh_rgbd

sys.path.insert(0, os.path.dirname(__file__))
import mesh_color_oracle  # noqa: E402
from test_flythrough_cpu import oracle, plane_colour_fp64, plane_fixture, random_meshes  # noqa: E402
from test_gpu_mesh import _look_at  # noqa: E402
from test_gpu_tsdf import sphere_depth  # noqa: E402
from test_tsdf_cpu import _K, _pose  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda"


def _mesh(v, col, tri):
    vd = torch.from_numpy(np.ascontiguousarray(v, dtype=np.float32)).to(DEV)
    cd = None if col is None else torch.from_numpy(np.ascontiguousarray(col, dtype=np.float32)).to(DEV)
    td = torch.from_numpy(np.ascontiguousarray(tri, dtype=np.int32)).to(DEV)
    counts = torch.tensor([len(v), len(tri), 0, 0], dtype=torch.int32, device=DEV)
    return DeviceMesh(vd, cd, td, counts, len(v), len(tri))


def _render(fx, poses, **kw):
    out = render_mesh_rgbd(_mesh(fx["v"], fx["col"], fx["tri"]), fx["K"], poses, fx["H"], fx["W"], fx["z_near"], fx["z_far"], **kw)
    return {k: t.cpu().numpy() for k, t in out.items()}


def _depth_render(mesh, K, T, H, W, z_near, z_far):
    """sgam_mesh_render_depth_f32 on the mesh's own buffers: the whole mesh, no frustum culling"""
    out = torch.empty((H, W), dtype=torch.float32, device=DEV)
    M = np.ascontiguousarray(T, dtype=np.float32)
    _lib.check(_lib.load().sgam_mesh_render_depth_f32(
        ops._p(mesh.vertices), mesh.vertices.shape[0], ops._p(mesh.triangles), mesh.triangles.shape[0], ops._p(mesh.counts), H, W,
        float(K[0, 0]), float(K[1, 1]), float(K[0, 2]), float(K[1, 2]), M.ctypes.data, z_near, z_far, ops._p(out), ops._stream()),
        "sgam_mesh_render_depth_f32")
    return out.cpu().numpy()


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def test_rgbd_render_is_bit_exact_on_small_meshes():
    for trial, fx in enumerate(random_meshes()):
        poses = [fx["T"], _pose(tx=0.1, ty=-0.05, yaw=0.2)]
        got = _render(fx, poses, normals=True, u8=True)
        assert got["depth"].shape == (2, 40, 48) and got["rgb"].shape == got["normal"].shape == got["rgb_u8"].shape == (2, 40, 48, 3)
        mesh = _mesh(fx["v"], None, fx["tri"])
        for p, T in enumerate(poses):
            d = _depth_render(mesh, fx["K"], T, fx["H"], fx["W"], fx["z_near"], fx["z_far"])
            assert (d > 0).mean() > 0.2
            assert np.array_equal(_bits(got["depth"][p]), _bits(d)), (trial, p)
            depth, rgb, win = oracle(fx, T=T)
            assert np.array_equal(_bits(depth), _bits(d))
            assert np.array_equal(_bits(got["rgb"][p]), _bits(rgb)), (trial, p)
            hit = d > 0
            n = got["normal"][p]
            assert np.allclose(np.linalg.norm(n[hit], axis=1), 1.0, atol=1e-5) and (n[~hit] == 0).all()
        assert np.array_equal(got["rgb_u8"], np.clip(got["rgb"], 0, 255).astype(np.uint8))
        again = _render(fx, poses, normals=True, u8=True)                    # fresh buffers: the same bits
        assert all(np.array_equal(got[k].view(np.uint8), again[k].view(np.uint8)) for k in got), trial
        if trial == 2:
            assert (oracle(fx)[2] & 1)[oracle(fx)[0] > 0].any()                 # second halves of near-clipped quads are seen


def test_exact_z_ties_go_to_the_lower_triangle_index():
    H = W = 16
    K = _K(12.0, 7.5)
    front = np.array([[-0.9, -0.8, 2.0], [0.9, -0.7, 2.5], [0.1, 0.9, 1.8]], dtype=np.float32)
    back = np.array([[-3.0, -3.0, 3.0], [3.0, -3.0, 3.0], [0.0, 4.0, 3.0]], dtype=np.float32)
    red, blue, grey = [250.0, 10.0, 20.0], [5.0, 30.0, 240.0], [90.0, 90.0, 90.0]
    v = np.concatenate([front, front, back])
    tri = np.array([[0, 1, 2], [3, 4, 5], [6, 7, 8]], dtype=np.int32)
    for first, second in ((red, blue), (blue, red)):
        col = np.array([first] * 3 + [second] * 3 + [grey] * 3, dtype=np.float32)
        fx = dict(v=v, col=col, tri=tri, K=K, H=H, W=W, z_near=0.1, z_far=10.0)
        got = _render(fx, [np.eye(4)])
        only_front = mesh_color_oracle.rasterise_rgbd(front, col[:3], tri[:1], np.eye(4), K, H, W, 0.1, 10.0)[0] > 0
        assert only_front.sum() > 20
        assert (got["rgb"][0][only_front] == np.float32(first)).all()
        assert (got["rgb"][0][(got["depth"][0] > 0) & ~only_front] == np.float32(grey)).all()
        assert ((got["depth"][0] > 0) & ~only_front).sum() > 5


# max |rendered colour - fp64 colour at the ray-plane intersection| over the covered samples of plane_fixture(), first GPU run
# (equal to the numpy restatement's figure): 2.171e-2 of 255.  It is not fp32 rounding alone: the rasteriser snaps the projected
# vertices to 1/256 px, which moves the interpolated field by up to the colour gradient (~8 per px here) times ~1/512 px per
# axis.  The bound is 4 x the measured value, far below 1e-3 * 255 = 0.255.
PLANE_MEASURED = 2.171e-2


def test_analytic_plane_is_interpolated_perspective_correctly():
    fx = plane_fixture()
    got = _render(fx, [fx["T"]])
    hit = got["depth"][0] > 0
    assert hit.sum() > 200
    want = plane_colour_fp64(fx)
    err = np.abs(got["rgb"][0].astype(np.float64) - want)[hit].max()
    print(f"analytic plane: max |colour - fp64| {err:.3e} of 255 over {hit.sum()} samples")
    assert err <= 4 * PLANE_MEASURED
    assert 4 * PLANE_MEASURED < 1e-3 * 255
    # and the depth is the plane's
    T = np.asarray(fx["T"], dtype=np.float32).astype(np.float64)
    c2w = np.linalg.inv(T)
    v, u = np.meshgrid(np.arange(fx["H"]), np.arange(fx["W"]), indexing="ij")
    d = np.stack([(u - fx["K"][0, 2]) / fx["K"][0, 0], (v - fx["K"][1, 2]) / fx["K"][1, 1], np.ones(u.shape)], -1) @ c2w[:3, :3].T
    z = (2.0 - c2w[2, 3]) / d[..., 2]
    assert np.abs(got["depth"][0] - z)[hit].max() < 2e-3


def test_near_clipped_coloured_triangle():
    H = W = 24
    K = _K(18.0, 11.5)
    v = np.array([[-0.7, -0.5, 1.4], [0.8, -0.3, 1.1], [0.1, 0.6, 0.2]], dtype=np.float32)       # the last vertex is behind z_near
    col = np.array([[250.0, 20.0, 130.0], [40.0, 200.0, 10.0], [90.0, 60.0, 255.0]], dtype=np.float32)
    fx = dict(v=v, col=col, tri=np.array([[0, 1, 2]], dtype=np.int32), T=np.eye(4), K=K, H=H, W=W, z_near=0.5, z_far=10.0)
    got = _render(fx, [fx["T"]])
    depth, rgb, win = oracle(fx)
    assert (win == 0).sum() > 10 and (win == 1).sum() > 10                  # both triangles of the clipped quad are seen
    assert np.array_equal(_bits(got["depth"][0]), _bits(depth)) and np.array_equal(_bits(got["rgb"][0]), _bits(rgb))
    assert (got["depth"][0][depth > 0] >= np.float32(0.5)).all()
    ulp = float(np.spacing(np.float32(255.0)))
    c = got["rgb"][0][depth > 0]
    assert (c >= col.min(0) - ulp).all() and (c <= col.max(0) + ulp).all()


def _colour_sphere(colour, voxel=0.05, trunc=0.5, radius=1.5, H=96, W=96, f=110.0):
    """test_gpu_mesh._sphere_volume with colour: every view fuses a frame of one constant colour"""
    K = _K(f, (H - 1) / 2)
    centre = np.array([0.3, -0.2, 0.1])
    dirs = [np.array((a, b, c), dtype=np.float64) for a in (-1, 0, 1) for b in (-1, 0, 1) for c in (-1, 0, 1) if (a, b, c) != (0, 0, 0)]
    eyes = [centre + 5.0 * (d / np.linalg.norm(d) + np.array([0.013, 0.021, -0.017])) for d in dirs]
    poses = [_look_at(e, centre) for e in eyes]
    lo, hi = frustum_bounds(K, poses, H, W, 8.0, margin=trunc + 16 * voxel)
    vol = TsdfVolume(voxel, trunc, lo, hi, DEV, memory_budget_bytes=2 << 30, color=True)
    rgb = torch.from_numpy(np.broadcast_to(np.array(colour, dtype=np.uint8), (H, W, 3)).copy()).to(DEV)
    for T in poses:
        vol.integrate(torch.from_numpy(sphere_depth(K, T, H, W, centre, radius)).to(DEV), K, T, rgb_u8=rgb)
    return vol, K, centre


def test_volume_mesh_renders_its_fused_colour():
    colour = (200, 120, 40)
    vol, K, centre = _colour_sphere(colour)
    H = W = 96
    mesh = vol.extract_mesh_device()
    host = vol.extract_triangle_mesh()
    assert mesh.n_vertices == len(host["vertices"]) and mesh.n_triangles == len(host["triangles"]) > 1000
    assert np.array_equal(mesh.vertices[:mesh.n_vertices].cpu().numpy(), host["vertices"])
    assert np.array_equal(mesh.triangles[:mesh.n_triangles].cpu().numpy(), host["triangles"])
    small = vol.extract_mesh_device(max_vertices=64, max_triangles=64)          # the second, counted pass
    assert small.n_triangles == mesh.n_triangles and small.triangles.shape[0] == mesh.n_triangles
    poses = [_look_at(centre + np.array([0.4, 3.2, -2.9]), centre), _look_at(centre + np.array([-2.5, 0.3, 3.4]), centre + np.array([0.2, 0.1, 0]))]
    out = render_mesh_rgbd(mesh, K, poses, H, W, 0.5, 8.0, normals=True, u8=True)
    for p, T in enumerate(poses):
        d = _depth_render(mesh, K, T, H, W, 0.5, 8.0)
        assert (d > 0).sum() > 1000
        assert np.array_equal(_bits(out["depth"][p].cpu().numpy()), _bits(d))
        hit = d > 0
        rgb = out["rgb"][p].cpu().numpy()
        assert np.abs(rgb[hit] - np.float32(colour)).max() <= 1.0
        n = out["normal"][p].cpu().numpy()
        assert (n[hit] @ np.array([0.0, 0.0, -1.0]) > 0).all()
        assert np.allclose(np.linalg.norm(n[hit], axis=1), 1.0, atol=1e-5)
    # a mesh without colours: depth and normals, and a refusal for colour
    bare = DeviceMesh(mesh.vertices, None, mesh.triangles, mesh.counts, mesh.n_vertices, mesh.n_triangles)
    geo = render_mesh_rgbd(bare, K, poses, H, W, 0.5, 8.0, normals=True)
    assert set(geo) == {"depth", "normal"} and torch.equal(geo["depth"], out["depth"]) and torch.equal(geo["normal"], out["normal"])
    with pytest.raises(ops.SgamHipError, match="no vertex colours"):
        render_mesh_rgbd(bare, K, poses, H, W, 0.5, 8.0, rgb=True)
    with pytest.raises(ops.SgamHipError, match="no vertex colours"):
        render_mesh_rgbd(bare, K, poses, H, W, 0.5, 8.0, u8=True)
    # P chunked by the key budget: the same views
    budget = tsdf.RGBD_KEY_BUDGET
    try:
        tsdf.RGBD_KEY_BUDGET = H * W * 8
        one = render_mesh_rgbd(mesh, K, poses, H, W, 0.5, 8.0)
    finally:
        tsdf.RGBD_KEY_BUDGET = budget
    assert torch.equal(one["depth"], out["depth"]) and torch.equal(one["rgb"], out["rgb"])


def test_scene_fly_through(golden, tmp_path):
    from PIL import Image

    from sgam_neurips22_amd.config import default_params
    from sgam_neurips22_amd.generative_sensing_module.model import VQModel
    from sgam_neurips22_amd.inference_pipeline import InfiniteSceneGeneration, synthetic_seed_frame
    data = "google_earth"
    g = golden("vqgan_full_ge256.npz")
    m = VQModel(**default_params(data))
    sd = testing.synthetic_state_dict(m.state_dict(), seed=0)
    sd["quantize.embedding.weight"] = testing.codebook_from_stats(float(g["zmean"]), float(g["zstd"]), 4096, 256, int(g["cb_seed"]))
    m.load_state_dict(sd)
    m = m.to(DEV).eval()
    seed = synthetic_seed_frame(data, 0)
    scene = InfiniteSceneGeneration(m, data, output_dim=(4, 1), seed_frame=seed, use_rgbd_integration=True,
                                    tsdf_memory_budget_bytes=1 << 30)
    scene.scene_expansion()
    assert len(scene.frames) == 4
    poses = scene.flythrough_poses(n_between=1)
    assert poses.shape == (7, 4, 4)
    out = scene.render_views(poses, out_dir=str(tmp_path))
    assert out["rgb"].shape == (7, 256, 256, 3) and out["depth"].shape == (7, 256, 256) and out["rgb_u8"].dtype == torch.uint8
    assert all(t.is_cuda for t in out.values())
    z0, z1 = scene._Z_RANGE[data]
    voxel = tsdf.VOLUME_PARAMS[data][0]
    cv = scene.colour_volume()
    coords = scene._ordered_grid_coords
    for k, c in enumerate(coords):
        node = scene.transform_grid[c[0]][c[1]]
        assert np.array_equal(poses[2 * k], node["T"])
        want = cv.render_mesh_depth(scene.K, node["T"], 256, 256, z0, z1).cpu().numpy()
        got = out["depth"][2 * k].cpu().numpy()
        both = (want > 0) & (got > 0)
        assert both.mean() > 0.3 and ((want > 0) == (got > 0)).mean() > 0.999
        assert np.array_equal(_bits(got[both]), _bits(want[both]))
        # The rendered colour at the node's own pose against the stored frames, on the samples where the node's stored depth is
        # the rendered one (within a voxel): closer to the node's own frame than to another node's.  A sanity direction, not a
        # tolerance — asserted for the nodes whose frame was fused (the last frame of a run is never a source: the volume holds
        # nothing of it), reported for all.
        rgb = out["rgb"][2 * k].cpu().numpy()
        other = coords[(k + 2) % 4]
        near = (got > 0) & (np.abs(scene.frames[c]["depth"].cpu().numpy() - got) < voxel)
        mads = {c2: float(np.abs(rgb[near] - scene.frames[c2]["rgb_u8"].cpu().numpy()[near].astype(np.float32)).mean()) for c2 in (c, other)}
        fused = any(c in entry for entry in scene._tsdf_log)
        print(f"fly-through node {c} (fused: {fused}): {int(near.sum())} samples within a voxel of the stored depth, mean |rendered - "
              f"own frame| {mads[c]:.2f}, against frame {other} {mads[other]:.2f}")
        if fused:
            assert near.sum() > 0 and mads[c] < mads[other]
    for p in range(7):
        img = np.array(Image.open(tmp_path / f"view_{p:04d}.png"))
        assert img.shape == (256, 256, 3) and img.dtype == np.uint8
        assert np.array_equal(img, out["rgb_u8"][p].cpu().numpy())
        assert np.array_equal(np.load(tmp_path / f"view_depth_{p:04d}.npy"), out["depth"][p].cpu().numpy())
    # the comparison path: the ray cast's nearest-voxel colour at the same poses
    ray = scene.render_views(poses[:2], source="raycast")
    assert ray["rgb"].shape == (2, 256, 256, 3) and ((ray["depth"][0] > 0) & (out["depth"][0] > 0)).float().mean().item() > 0.3
    # a fused source overwritten after the fact: the replay would not be the run's volume
    scene.save_to_store(coords[0], *[scene.frames[coords[0]][k] for k in ("rgb_u8", "rgb_f", "depth")])
    with pytest.raises(ValueError, match="overwritten"):
        scene.render_views(poses)
    # a scene on the splat branch has no volume to render
    splat = InfiniteSceneGeneration(m, data, output_dim=(4, 1), seed_frame=seed)
    with pytest.raises(ValueError, match="rgbd_integration branch"):
        splat.render_views(poses)


def test_views_of_one_lockstepped_scene(golden):
    """render_views touches only the scene's own log and frame store: it works on a scene that was advanced in lock step"""
    from sgam_neurips22_amd.config import default_params
    from sgam_neurips22_amd.distributed import LockstepScenes
    from sgam_neurips22_amd.generative_sensing_module.model import VQModel
    from sgam_neurips22_amd.inference_pipeline import synthetic_seed_frame
    data = "google_earth"
    g = golden("vqgan_full_ge256.npz")
    m = VQModel(**default_params(data))
    sd = testing.synthetic_state_dict(m.state_dict(), seed=0)
    sd["quantize.embedding.weight"] = testing.codebook_from_stats(float(g["zmean"]), float(g["zstd"]), 4096, 256, int(g["cb_seed"]))
    m.load_state_dict(sd)
    m = m.to(DEV).eval()
    L = LockstepScenes(m, data, [synthetic_seed_frame(data, i) for i in range(2)], output_dim=(4, 1), use_rgbd_integration=True,
                       tsdf_memory_budget_bytes=1 << 30)
    L.expand()
    views = []
    for sc in L.scenes:
        poses = sc.flythrough_poses(n_between=0)
        assert poses.shape == (4, 4, 4)
        views.append(sc.render_views(poses[:2], H=128, W=128))
        assert views[-1]["rgb"].shape == (2, 128, 128, 3) and (views[-1]["depth"] > 0).float().mean().item() > 0.2
    assert not torch.equal(views[0]["rgb_u8"], views[1]["rgb_u8"])
    # the half-size view is the full-size one's field of view: the depth at the centre sample agrees with its neighbourhood there
    full = L.scenes[0].render_views(poses[:1])["depth"][0]
    half = views[0]["depth"][0]
    both = (half > 0) & (full[::2, ::2] > 0)
    assert both.float().mean().item() > 0.2
    assert (half[both] - full[::2, ::2][both]).abs().median().item() < 0.05
