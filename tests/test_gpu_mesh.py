"""Marching-cubes mesh of the fused TSDF (csrc/tsdf.hip: sgam_tsdf_extract_mesh_f32) and its depth render
(csrc/mesh_raster.hip: sgam_mesh_render_depth_f32) on the GPU: array-equal to the numpy oracle (tests/mc_oracle.py) on the
dense grid assembled from the bricks, closed on an all-round sphere, the rasteriser bit-exact against its numpy restatement,
the measured bound between the ray cast and the mesh render, and the scene loop's "mesh" mode end to end."""
import os
import sys

import numpy as np
import pytest
import torch

from sgam_neurips22_amd import testing
from sgam_neurips22_amd.tsdf import VOLUME_PARAMS, TsdfVolume, frustum_bounds

sys.path.insert(0, os.path.dirname(__file__))
import mc_oracle  # noqa: E402
from test_gpu_tsdf import _textured, sphere_depth  # noqa: E402
from test_tsdf_cpu import _K, _pose, plane_depth  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda"


def _look_at(eye, target):
    """world -> camera 4x4 looking from eye at target (camera +z forward, +y down)"""
    eye, target = np.asarray(eye, dtype=np.float64), np.asarray(target, dtype=np.float64)
    z = target - eye
    z /= np.linalg.norm(z)
    up = np.array([0.0, 1.0, 0.0]) if abs(z[1]) < 0.9 else np.array([1.0, 0.0, 0.0])
    x = np.cross(up, z)
    x /= np.linalg.norm(x)
    y = np.cross(z, x)
    T = np.eye(4)
    T[:3, :3] = np.stack([x, y, z])
    T[:3, 3] = -T[:3, :3] @ eye
    return T


def _volume(voxel, trunc, K, H, W, poses, depth_fn, z_far, color=False, **kw):
    lo, hi = frustum_bounds(K, poses, H, W, z_far, margin=trunc + 16 * voxel)
    vol = TsdfVolume(voxel, trunc, lo, hi, DEV, memory_budget_bytes=2 << 30, color=color, **kw)
    for i, T in enumerate(poses):
        d = torch.from_numpy(depth_fn(T)).to(DEV)
        rgb = torch.from_numpy(_textured(H, W, i)).to(DEV) if color else None
        vol.integrate(d, K, T, rgb_u8=rgb)
    return vol


def _dense(vol):
    """the bricks as one dense fp32 grid (NaN = unobserved) + colours, origin (global lattice) and the device key function"""
    dims = [int(d) for d in vol.dims]
    table = vol.unit_table.cpu().numpy().reshape(dims[2], dims[1], dims[0])
    zs, ys, xs = np.nonzero(table >= 0)
    lo = np.array([xs.min(), ys.min(), zs.min()])
    hi = np.array([xs.max(), ys.max(), zs.max()]) + 2              # + the upper neighbour unit, kept unobserved if absent
    n = (hi - lo) * 16
    g = np.full((n[2], n[1], n[0]), np.nan, dtype=np.float32)
    col = np.zeros((n[2], n[1], n[0], 3), dtype=np.float32) if vol.brick_color is not None else None
    t = vol.brick_tsdf.cpu().numpy()
    c = vol.brick_color.cpu().numpy() if col is not None else None
    for z, y, x in zip(zs, ys, xs):
        b = table[z, y, x] & 0x3FFFFFFF
        sl = (slice((z - lo[2]) * 16, (z - lo[2] + 1) * 16), slice((y - lo[1]) * 16, (y - lo[1] + 1) * 16),
              slice((x - lo[0]) * 16, (x - lo[0] + 1) * 16))
        v = t[b].reshape(16, 16, 16)
        g[sl] = np.where(v <= 1.0, v, np.nan)
        if col is not None:
            col[sl] = c[b].reshape(16, 16, 16, 3)
    base = np.array([int(v) for v in vol.base])
    origin = (lo + base) * 16

    def key_fn(ix, iy, iz):
        ux, uy, uz = (ix >> 4) - base[0], (iy >> 4) - base[1], (iz >> 4) - base[2]
        slot = (uz.astype(np.int64) * dims[1] + uy) * dims[0] + ux
        return slot * 4096 + ((iz & 15) << 8) + ((iy & 15) << 4) + (ix & 15)

    return g, col, origin, key_fn


def _raw_mesh(vol, colors=True, cull=None, nv=1 << 18, nt=1 << 19):
    bufs = {"vertices": torch.empty((nv, 3), dtype=torch.float32, device=DEV), "keys": torch.empty((nv,), dtype=torch.int64, device=DEV),
            "triangles": torch.empty((nt, 3), dtype=torch.int32, device=DEV), "counts": torch.zeros((4,), dtype=torch.int32, device=DEV),
            "ws": vol._mesh_ws()}
    col = torch.empty((nv, 3), dtype=torch.float32, device=DEV) if colors and vol.brick_color is not None else None
    vol._extract_mesh(bufs, col, cull=cull)
    fv, ft, over, _ = (int(v) for v in bufs["counts"].cpu())
    assert over == 0
    out = {"vertices": bufs["vertices"][:fv].cpu().numpy(), "keys": bufs["keys"][:fv].cpu().numpy(),
           "triangles": bufs["triangles"][:ft].cpu().numpy()}
    if col is not None:
        out["vertex_colors"] = col[:fv].cpu().numpy()
    return out


@pytest.mark.parametrize("data", ["clevr-infinite", "google_earth"])
def test_device_mesh_equals_the_oracle_on_the_bricks(data):
    voxel, trunc = VOLUME_PARAMS[data]
    H = W = 64
    K = _K(120.0, 31.5)
    poses = [_pose(), _pose(tx=0.21, yaw=0.07), _pose(tx=-0.13, ty=0.05, yaw=-0.05)]
    zp = 8.0 if voxel > 0.02 else 2.2
    # a wavy plane: the surface crosses unit faces in all three axes
    fn = lambda T: plane_depth(K, T, H, W, zp) + np.float32(6 * voxel) * np.sin(np.arange(W, dtype=np.float32) / 5.0)[None, :]  # noqa: E731
    vol = _volume(voxel, trunc, K, H, W, poses, fn, 16.5 if voxel > 0.02 else 4.8, color=True)
    got = _raw_mesh(vol)
    g, col, origin, key_fn = _dense(vol)
    want = mc_oracle.marching_cubes(g, voxel, origin, col, key_fn)
    assert len(want["triangles"]) > 1000
    assert np.array_equal(got["keys"], want["keys"])
    assert np.array_equal(got["vertices"].view(np.uint32), want["vertices"].view(np.uint32))
    assert np.array_equal(got["vertex_colors"].view(np.uint32), want["vertex_colors"].view(np.uint32))
    assert np.array_equal(got["triangles"], want["triangles"])
    # units of the mesh span several units along every axis
    ukeys = np.unique(got["keys"] // 3 // 4096)
    assert len(ukeys) > 4
    again = _raw_mesh(vol)
    assert all(np.array_equal(got[k].view(np.uint8), again[k].view(np.uint8)) for k in got)
    # the public export: the same arrays, colours in 0..1, normals of unit length
    m = vol.extract_triangle_mesh()
    assert np.array_equal(m["vertices"], got["vertices"]) and np.array_equal(m["triangles"], got["triangles"])
    assert np.allclose(m["vertex_colors"] * 255.0, got["vertex_colors"], atol=1e-4)
    assert np.allclose(np.linalg.norm(m["vertex_normals"], axis=1), 1.0)
    # vertices on an edge the point extractor also emits: bit-identical positions and colours
    pc = vol.extract_point_cloud()
    common, im, ip = np.intersect1d(m["keys"], pc["keys"], return_indices=True)
    assert len(common) > 0.5 * len(pc["keys"])
    assert np.array_equal(m["vertices"][im].view(np.uint32), pc["points"][ip].view(np.uint32))
    assert np.array_equal(m["vertex_colors"][im].view(np.uint32), pc["colors"][ip].view(np.uint32))


def _sphere_volume(voxel=0.05, trunc=0.5, radius=1.5, H=96, W=96, f=110.0):
    K = _K(f, (H - 1) / 2)
    centre = np.array([0.3, -0.2, 0.1])
    # the 26 directions of a cube's faces, edges and corners (slightly rotated off the axes): every part of the band observed
    dirs = [np.array((a, b, c), dtype=np.float64) for a in (-1, 0, 1) for b in (-1, 0, 1) for c in (-1, 0, 1) if (a, b, c) != (0, 0, 0)]
    eyes = [centre + 5.0 * (d / np.linalg.norm(d) + np.array([0.013, 0.021, -0.017])) for d in dirs]
    poses = [_look_at(e, centre) for e in eyes]
    vol = _volume(voxel, trunc, K, H, W, poses, lambda T: sphere_depth(K, T, H, W, centre, radius), 8.0)
    return vol, K, centre, radius, poses


def test_all_round_sphere_mesh_is_closed_and_close_to_the_sphere():
    voxel = 0.05
    vol, K, centre, radius, _ = _sphere_volume(voxel)
    m = vol.extract_triangle_mesh()
    chi, (uk, ucount), (dk, dcount) = mc_oracle.euler_and_edges(m["triangles"])
    assert (ucount == 2).all() and (dcount == 1).all()          # closed, consistently oriented 2-manifold
    # the sphere is its largest connected component, of genus 0; projective fusion also leaves a few small closed bubbles in
    # the band, reported here
    lab = _components(m["triangles"], len(m["vertices"]))
    big = np.bincount(lab[m["triangles"][:, 0]]).argmax()
    t = m["triangles"][lab[m["triangles"][:, 0]] == big]
    chi_big = mc_oracle.euler_and_edges(t)[0]
    print(f"sphere mesh: chi {chi} over {len(np.unique(lab[m['triangles'][:, 0]]))} components; the largest: {len(t)} of "
          f"{len(m['triangles'])} triangles, chi {chi_big}")
    assert chi_big == 2 and len(t) > 0.9 * len(m["triangles"])
    v = m["vertices"].astype(np.float64)
    fn = np.cross(v[t[:, 1]] - v[t[:, 0]], v[t[:, 2]] - v[t[:, 0]])
    # face normals point away from the centre; the exceptions are marching cubes' slivers (a vertex on or next to a lattice
    # point, where |tsdf| ~ 0: a near-zero area whose normal is rounding), measured by their share of the area
    out = (fn * (v[t].mean(1) - centre)).sum(1) > 0
    area = np.linalg.norm(fn, axis=1)
    print(f"sphere faces pointing inward: {(~out).sum()} of {len(t)}, {area[~out].sum() / area.sum():.2e} of the area")
    assert (~out).mean() < 0.01 and area[~out].sum() < 1e-3 * area.sum()
    d = np.abs(np.linalg.norm(v[np.unique(t)] - centre, axis=1) - radius) / voxel      # (the sphere component's vertices)
    print(f"sphere mesh: {len(v)} vertices, {len(t)} triangles, |dist| mean {d.mean():.3f} max {d.max():.3f} voxel")
    # (the fused surface itself sits off the sphere by this much: 26 all-round views fuse projective distances from grazing
    # rays too — the extraction is array-equal to the oracle on the same bricks, test_device_mesh_equals_the_oracle_on_the_bricks)
    assert d.mean() <= 0.5 and d.max() <= 2.0


def _components(tris, n):
    """connected-component label per vertex (min-label propagation over the triangle edges)"""
    lab = np.arange(n)
    e = np.concatenate([tris[:, [0, 1]], tris[:, [1, 2]], tris[:, [2, 0]]]).astype(np.int64)
    while True:
        m = np.minimum(lab[e[:, 0]], lab[e[:, 1]])
        new = lab.copy()
        np.minimum.at(new, e[:, 0], m)
        np.minimum.at(new, e[:, 1], m)
        new = new[new]
        if np.array_equal(new, lab):
            return lab
        lab = new


def test_rasteriser_is_bit_exact_against_numpy_on_small_meshes():
    H, W = 40, 48
    K = _K(40.0, 20.0)
    K[0, 2] = 23.5
    rs = np.random.RandomState(3)
    T = _pose(tx=0.1, ty=-0.05, yaw=0.03)
    for trial in range(3):
        n = 60
        v = np.stack([rs.uniform(-1.5, 1.5, n), rs.uniform(-1.2, 1.2, n), rs.uniform(0.2 if trial else 1.0, 4.0, n)], 1).astype(np.float32)
        tri = rs.randint(0, n, size=(80, 3)).astype(np.int32)
        tri = tri[(tri[:, 0] != tri[:, 1]) & (tri[:, 1] != tri[:, 2]) & (tri[:, 0] != tri[:, 2])]
        z_near = 0.5 if trial == 2 else 0.1
        want = mc_oracle.rasterise(v, tri, T, K, H, W, z_near, 3.5)
        got = _render(v, tri, T, K, H, W, z_near, 3.5)
        assert (want > 0).mean() > 0.2
        assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), trial
        assert (got[got > 0] >= np.float32(z_near)).all()          # near-plane clipping never yields z < z_near


def _render(v, tri, T, K, H, W, z_near, z_far):
    from sgam_neurips22_amd import _lib, ops
    vd = torch.from_numpy(np.ascontiguousarray(v, dtype=np.float32)).to(DEV)
    td = torch.from_numpy(np.ascontiguousarray(tri, dtype=np.int32)).to(DEV)
    counts = torch.tensor([len(v), len(tri), 0, 0], dtype=torch.int32, device=DEV)
    out = torch.empty((H, W), dtype=torch.float32, device=DEV)
    M = np.ascontiguousarray(T, dtype=np.float32)
    _lib.check(_lib.load().sgam_mesh_render_depth_f32(ops._p(vd), len(v), ops._p(td), len(tri), ops._p(counts), H, W, float(K[0, 0]),
                                                      float(K[1, 1]), float(K[0, 2]), float(K[1, 2]), M.ctypes.data, z_near, z_far,
                                                      ops._p(out), ops._stream()), "sgam_mesh_render_depth_f32")
    return out.cpu().numpy()


def test_sphere_render_has_no_holes_and_culling_changes_nothing():
    vol, K, centre, radius, poses = _sphere_volume()
    H = W = 96
    T = _look_at(centre + np.array([0.4, 3.2, -2.9]), centre)
    got = vol.render_mesh_depth(K, T, H, W, 0.5, 8.0).cpu().numpy()
    sd = sphere_depth(K, T, H, W, centre, radius) > 0
    silhouette1 = np.zeros_like(sd)
    # samples more than 1 px inside the analytic silhouette: every 3 x 3 neighbourhood inside it
    from numpy.lib.stride_tricks import sliding_window_view
    silhouette1[1:-1, 1:-1] = sliding_window_view(sd, (3, 3)).all(axis=(2, 3))
    assert silhouette1.sum() > 500
    assert (got[silhouette1] > 0).all()
    m = vol.extract_triangle_mesh()
    full = _render(m["vertices"], m["triangles"], T, K, H, W, 0.5, 8.0)
    assert np.array_equal(full.view(np.uint32), got.view(np.uint32))          # frustum-culled == unculled, bit for bit
    # a near plane through the sphere: clipped, nothing nearer than z_near
    zc = float(np.linalg.norm(T[:3, :3] @ centre + T[:3, 3]))
    clipped = vol.render_mesh_depth(K, T, H, W, zc - 0.5, 8.0).cpu().numpy()
    assert (clipped[clipped > 0] >= np.float32(zc - 0.5)).all() and (clipped > 0).sum() > 100


def _bound(vol, K, T, H, W, z0, z1, voxel):
    a = vol.render_depth(K, T, H, W, z0, z1).cpu().numpy()
    b = vol.render_mesh_depth(K, T, H, W, z0, z1).cpu().numpy()
    both = (a > 0) & (b > 0)
    dz = np.abs(a[both] - b[both]) / voxel
    one = ((a > 0) != (b > 0)).sum() / max(1, ((a > 0) | (b > 0)).sum())
    return float(np.median(dz)), float(np.percentile(dz, 99)), float(one), int(both.sum())


# ray cast vs mesh render on the same volume, |dz| in voxels over the pixels both hit, and the fraction of the pixels hit by
# only one of them ("ray cast vs mesh depth": thresholds from the first GPU run, not loosened since)
# first run: plane 0.0001 / 0.0008 / 0.0015, sphere 0.122 / 0.79 / 0.0041, loop (noise scene, worst of 3 steps) 0.132 / 209 / 0.38
BOUND = {"plane": (0.01, 0.01, 0.005), "sphere": (0.15, 1.0, 0.01), "loop": (0.2, 250.0, 0.45)}


def test_raycast_against_mesh_depth_bound():
    H = W = 96
    K = _K(110.0, 47.5)
    stats = {}
    voxel, trunc = 0.05, 0.5
    poses = [_pose(), _pose(tx=0.3, yaw=0.05), _pose(tx=-0.25, ty=0.15, yaw=-0.04)]
    vol = _volume(voxel, trunc, K, H, W, poses, lambda T: plane_depth(K, T, H, W, 8.0), 16.5)
    stats["plane"] = _bound(vol, K, _pose(tx=0.1, ty=0.05, yaw=0.02), H, W, 1.0, 16.5, voxel)
    svol, sK, centre, radius, _ = _sphere_volume()
    stats["sphere"] = _bound(svol, sK, _look_at(centre + np.array([0.4, 3.2, -2.9]), centre), 96, 96, 0.5, 8.0, 0.05)
    loop = []
    scene = _scene_loop("raycast", steps=3)
    voxel = VOLUME_PARAMS["google_earth"][0]
    z0, z1 = scene._Z_RANGE["google_earth"]
    for c in scene._ordered_grid_coords[1:4]:
        node = scene.transform_grid[c[0]][c[1]]
        loop.append(_bound(scene.volume, scene.K, node["T"], 256, 256, z0, z1, voxel))
    stats["loop"] = tuple(float(np.max([s[k] for s in loop])) for k in range(3)) + (int(sum(s[3] for s in loop)),)
    for name, s in stats.items():
        print(f"ray cast vs mesh [{name}]: median |dz| {s[0]:.4f} voxel, p99 {s[1]:.4f} voxel, one-sided {s[2]:.4f} of {s[3]} px")
    for name, (med, p99, one) in BOUND.items():
        s = stats[name]
        assert s[3] > 1000, name
        assert s[0] <= med and s[1] <= p99 and s[2] <= one, (name, s)


def _scene_loop(mode, steps=3, **kw):
    from sgam_neurips22_amd.config import default_params
    from sgam_neurips22_amd.generative_sensing_module.model import VQModel
    from sgam_neurips22_amd.inference_pipeline import InfiniteSceneGeneration, synthetic_seed_frame
    p = default_params("google_earth")
    m = VQModel(**p)
    sd = testing.synthetic_state_dict(m.state_dict(), seed=0)
    sd["quantize.embedding.weight"] = testing.codebook_from_stats(0.0, 0.5, p["n_embed"], 256, 1)
    m.load_state_dict(sd)
    m = m.to(DEV).eval()
    scene = InfiniteSceneGeneration(m, "google_earth", output_dim=(steps + 2, 1), seed_frame=synthetic_seed_frame("google_earth", 0, 256),
                                    use_rgbd_integration=True, rgbd_depth_render=mode)
    scene._outs = []
    for _ in range(steps):
        scene._outs.append(scene.one_step_prediction(scene.next_pose(scene.curr)))
        scene.curr += 1
    return scene


def test_scene_loop_conditions_on_the_mesh_depth(tmp_path):
    from sgam_neurips22_amd import pointcloud
    scene = _scene_loop("mesh")
    for out in scene._outs:
        assert torch.isfinite(out["rgbd"]).all()
        cover = float((~out["extrapolation_mask"]).float().mean())
        assert cover > 0.4, cover
    scene.volume.check()
    assert scene.volume._mesh is not None and int(scene.volume._mesh["counts"][1]) > 0
    # one more step of the conditioning branch by hand: the mesh depth at the next pose
    node = scene.transform_grid[scene.curr][0]
    d = scene.rgbd_integration([scene.transform_grid[scene.curr - 1][0]], node).cpu().numpy()
    assert (d > 0).mean() > 0.3
    # a tiny mesh budget: the overflow is reported by check(), not silently dropped
    small = scene._make_volume()
    small.mesh_budget_bytes = 4096
    for coords in scene._tsdf_log:
        nodes = [scene.transform_grid[c[0]][c[1]] for c in coords]
        small.integrate_many([scene.frames[c]["depth"] for c in coords], scene.K, [n["T"] for n in nodes])
    small.render_mesh_depth(scene.K, node["T"], 256, 256, 0.05, 4.8)
    with pytest.raises(Exception, match="mesh buffers exhausted"):
        small.check()
    # the run tail's coloured triangle mesh
    n = scene.export_triangle_mesh(str(tmp_path))
    back = pointcloud.read_triangle_mesh(str(tmp_path / "rgbd_integrated_triangle_mesh.ply"))
    want = scene.colour_volume().extract_triangle_mesh()
    assert n == len(want["triangles"]) > 1000
    assert np.array_equal(back["vertices"], want["vertices"].astype(np.float64))
    assert np.array_equal(back["triangles"], want["triangles"])
    assert np.array_equal(back["normals"], want["vertex_normals"])
    assert np.array_equal(back["colors_u8"], np.round(np.clip(want["vertex_colors"].astype(np.float64), 0, 1) * 255).astype(np.uint8))
