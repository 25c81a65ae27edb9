"""TSDF fusion of the generated RGB-D frames and the depth render at the next target pose — the
``rgbd_integration`` conditioning branch (reference sgam/inference_pipeline.py:119-133 and 745-838, which
delegates to Open3D 0.15.2).  Device side: csrc/tsdf.hip; this file sizes and owns the state.

State for one scene, all in HBM and allocated once (no growth, no host round trip per frame):
  unit table   int32 [dz][dy][dx]   direct-mapped over the scene's bounding box (units of 16 voxels)
  brick pool   fp32 tsdf + fp32 weight, 16^3 voxels per brick, bump-allocated on the device
"""
import ctypes
import math
import weakref

import numpy as np
import torch

from . import _lib, ops
from ._lib import TsdfGrid, check

UNIT = 16
# (voxel_length, sdf_trunc) per dataset: reference inference_pipeline.py:119-133
VOLUME_PARAMS = {"clevr-infinite": (0.05, 0.5), "google_earth": (0.01, 0.03)}
DEPTH_TRUNC = 20.0          # RGBDImage.create_from_color_and_depth(depth_trunc=20), :772


def frustum_bounds(K, poses_w2c, H, W, z_far, margin):
    """Axis-aligned world box of the camera frusta (apex + far-plane corners) of all poses, grown by `margin`."""
    fx, fy, cx, cy = K[0, 0], K[1, 1], K[0, 2], K[1, 2]
    corners = np.array([[(u - cx) / fx * z_far, (v - cy) / fy * z_far, z_far, 1.0]
                        for u in (0.0, W - 1.0) for v in (0.0, H - 1.0)] + [[0.0, 0.0, 0.0, 1.0]])
    pts = []
    for T in poses_w2c:
        pts.append((np.linalg.inv(np.asarray(T, dtype=np.float64)) @ corners.T).T[:, :3])
    pts = np.concatenate(pts)
    return pts.min(0) - margin, pts.max(0) + margin


class TsdfVolume:
    def __init__(self, voxel_length, sdf_trunc, lo, hi, device, max_bricks=None, memory_budget_bytes=None, color=False,
                 mesh_budget_bytes=None):
        """lo / hi: world-space box the scene can occupy (see frustum_bounds).  max_bricks defaults to what
        `memory_budget_bytes` of brick pool holds (32 KB per brick, 80 KB with colour), capped at the number of units in
        the box; the budget defaults to a quarter of the device memory that is free right now (not more than 48 GiB).
        color: also fuse RGB8 colour (TSDFVolumeColorType.RGB8, reference :123-131).  mesh_budget_bytes: the marching-cubes
        mesh buffers of render_mesh_depth (allocated on its first call, never resized; default 512 MiB: 12 B per triangle, 20 B
        per vertex, one vertex per two triangles)."""
        self.voxel_length, self.sdf_trunc = float(voxel_length), float(sdf_trunc)
        unit_len = np.float32(voxel_length) * np.float32(UNIT)
        base = np.floor(np.asarray(lo, dtype=np.float64) / float(unit_len)).astype(np.int64)
        top = np.floor(np.asarray(hi, dtype=np.float64) / float(unit_len)).astype(np.int64)
        dims = top - base + 1
        n_units = int(dims.prod())
        if n_units >= 2 ** 31:
            raise ops.SgamHipError(f"TSDF box of {tuple(dims)} units does not fit the int32 unit table; shrink the scene box")
        if memory_budget_bytes is None:
            free = torch.cuda.mem_get_info(device)[0] if torch.device(device).type == "cuda" else 1 << 30
            memory_budget_bytes = min(48 << 30, free // 4)
        if max_bricks is None:
            max_bricks = max(1, min(n_units, memory_budget_bytes // (UNIT ** 3 * (20 if color else 8))))
        self.base, self.dims, self.max_bricks, self.device = base, dims, int(max_bricks), device
        self.grid = TsdfGrid(np.float32(voxel_length), np.float32(sdf_trunc), (ctypes.c_int32 * 3)(*map(int, base)),
                             (ctypes.c_int32 * 3)(*map(int, dims)))
        self.unit_table = torch.full((n_units,), -1, dtype=torch.int32, device=device)
        self.unit_stamp = torch.zeros((n_units,), dtype=torch.int32, device=device)
        self.counters = torch.zeros((4 * 32,), dtype=torch.int32, device=device)        # counter k at index 32 k (a cache line each)
        self.brick_tsdf = torch.full((self.max_bricks, UNIT ** 3), 2.0, dtype=torch.float32, device=device)   # 2 = unobserved
        self.brick_weight = torch.zeros((self.max_bricks, UNIT ** 3), dtype=torch.float32, device=device)
        self.brick_color = torch.zeros((self.max_bricks, UNIT ** 3, 3), dtype=torch.float32, device=device) if color else None
        self.max_list = int(min(n_units, 1 << 22))
        self.brick_list = torch.empty((self.max_list,), dtype=torch.int32, device=device)
        self.frame_id = 0
        self.mesh_budget_bytes = int(512 << 20 if mesh_budget_bytes is None else mesh_budget_bytes)
        self._mesh = None        # render_mesh_depth's buffers (see _mesh_buffers)
        self._ray_mult = {}      # (H, W, fx, fy, cx, cy) -> (H,W) table of the rule's depth -> camera-distance multiplier

    @staticmethod
    def _k4(K):
        K = np.asarray(K, dtype=np.float32)
        return float(K[0, 0]), float(K[1, 1]), float(K[0, 2]), float(K[1, 2])

    def integrate(self, depth, K, T_w2c, rgb_u8=None):
        """depth (H,W) fp32 device tensor, K 3x3, T_w2c 4x4 world->camera (the reference's extrinsic [R|t]); rgb_u8 (H,W,3)
        uint8 device tensor: the frame's colour, fused when the volume was built with color=True."""
        self.integrate_many([depth], K, [T_w2c], None if rgb_u8 is None else [rgb_u8])

    def integrate_many(self, depths, K, Ts_w2c, rgbs_u8=None, Ts_c2w=None):
        """The source frames of ONE step (reference :757-790: one volume.integrate per source) in one pass over the union of
        the units they open — the same voxel values as integrate() per source in list order.  Ts_c2w: the inverses, when the
        caller holds them already (float64 4x4s)."""
        n = len(depths)
        if not 0 < n <= 8 or len(Ts_w2c) != n:
            raise ops.SgamHipError("TsdfVolume.integrate_many: 1 .. 8 source frames, one pose each")
        H, W = depths[0].shape
        srcs = (_lib.TsdfSrc * n)()
        keep = []
        for k in range(n):
            d = depths[k]
            ops._need_cuda(d)
            if tuple(d.shape) != (H, W) or d.dtype != torch.float32:
                raise ops.SgamHipError("TsdfVolume.integrate_many: depth maps must be (H,W) fp32 of one size")
            d = d.contiguous()
            rgb = None
            if self.brick_color is not None:
                rgb = None if rgbs_u8 is None else rgbs_u8[k]
                if rgb is None or rgb.dtype != torch.uint8 or tuple(rgb.shape) != (H, W, 3):
                    raise ops.SgamHipError("TsdfVolume(color=True).integrate needs the frame's (H,W,3) uint8 colour")
                rgb = rgb.contiguous()
            keep.append((d, rgb))
            T = np.asarray(Ts_w2c[k], dtype=np.float64)
            Ti = np.linalg.inv(T) if Ts_c2w is None else np.asarray(Ts_c2w[k], dtype=np.float64)
            srcs[k].depth, srcs[k].rgb_u8 = ops._p(d), ops._p(rgb)
            srcs[k].cam2world[:] = Ti.astype(np.float32).ravel().tolist()       # host 4x4s: passed by value to the kernels
            srcs[k].world2cam[:] = T.astype(np.float32).ravel().tolist()
        self.frame_id += 1
        fx, fy, cx, cy = self._k4(K)
        rm = self._ray_mult_table(H, W, fx, fy, cx, cy)
        check(_lib.load().sgam_tsdf_integrate_srcs_f32(
            ctypes.byref(self.grid), srcs, n, H, W, fx, fy, cx, cy, DEPTH_TRUNC, self.frame_id,
            ops._p(self.unit_table), ops._p(self.unit_stamp), ops._p(self.counters), ops._p(self.brick_list), self.max_list,
            ops._p(self.brick_tsdf), ops._p(self.brick_weight), self.max_bricks, ops._p(self.brick_color),
            ops._p(rm), ops._stream()), "sgam_tsdf_integrate_srcs_f32")

    def _ray_mult_table(self, H, W, fx, fy, cx, cy):
        key = (H, W, fx, fy, cx, cy)
        if key not in self._ray_mult:
            rm = torch.empty((H, W), dtype=torch.float32, device=self.device)
            check(_lib.load().sgam_tsdf_ray_mult_f32(H, W, fx, fy, cx, cy, ops._p(rm), ops._stream()), "sgam_tsdf_ray_mult_f32")
            self._ray_mult[key] = rm
        return self._ray_mult[key]

    def render_depth(self, K, T_w2c, H, W, z_near, z_far, want_color=False, T_c2w=None, out=None):
        """View-space z of the fused surface at the pose, (H,W) fp32, 0 where nothing is hit; with want_color also the
        fused colour at the hit, (H,W,3) fp32 in 0..255.  T_c2w: the inverse pose when the caller holds it; out: destination."""
        T = np.asarray(T_w2c, dtype=np.float64)
        c2w = np.ascontiguousarray(np.linalg.inv(T) if T_c2w is None else T_c2w, dtype=np.float32)
        if out is None:
            out = torch.empty((H, W), dtype=torch.float32, device=self.device)
        assert out.shape == (H, W) and out.dtype == torch.float32 and out.is_contiguous()
        fx, fy, cx, cy = self._k4(K)
        check(_lib.load().sgam_tsdf_raycast_depth_f32(
            ctypes.byref(self.grid), H, W, fx, fy, cx, cy, c2w.ctypes.data, float(z_near), float(z_far), ops._p(self.unit_table),
            ops._p(self.brick_tsdf), ops._p(out), ops._p(self.brick_color if want_color else None),
            ops._p(col := (torch.empty((H, W, 3), dtype=torch.float32, device=self.device) if want_color else None)), ops._stream()),
            "sgam_tsdf_raycast_depth_f32")
        return (out, col) if want_color else out

    def extract_point_cloud(self):
        """`volume.extract_point_cloud()` of the reference's run tail (inference_pipeline.py:446-450): the zero crossings of the
        fused TSDF as points (float32 (n,3) world coordinates), normals (n,3) and — when colour was fused — colours (n,3) in
        0..1, in a run-independent order (sorted by (unit, voxel, axis)).  Two launches (count, then fill) and one host sync:
        an export step after the run, not part of the loop."""
        lib = _lib.load()
        counter = torch.zeros((1,), dtype=torch.int64, device=self.device)
        check(lib.sgam_tsdf_extract_points_f32(ctypes.byref(self.grid), ops._p(self.unit_table), ops._p(self.brick_tsdf), None,
                                               ops._p(counter), 0, None, None, None, None, ops._stream()), "sgam_tsdf_extract_points_f32")
        n = int(counter.item())
        pts = torch.empty((max(n, 1), 3), dtype=torch.float32, device=self.device)
        nrm = torch.empty_like(pts)
        col = torch.empty_like(pts) if self.brick_color is not None else None
        keys = torch.empty((max(n, 1),), dtype=torch.int64, device=self.device)
        counter.zero_()
        check(lib.sgam_tsdf_extract_points_f32(ctypes.byref(self.grid), ops._p(self.unit_table), ops._p(self.brick_tsdf),
                                               ops._p(self.brick_color), ops._p(counter), n, ops._p(pts), ops._p(nrm), ops._p(col),
                                               ops._p(keys), ops._stream()), "sgam_tsdf_extract_points_f32")
        if int(counter.item()) != n:
            raise ops.SgamHipError("TSDF point extraction: the volume changed between the counting and the filling pass")
        order = torch.argsort(keys[:n])
        out = {"points": pts[:n][order].cpu().numpy(), "normals": nrm[:n][order].cpu().numpy(), "keys": keys[:n][order].cpu().numpy()}
        if col is not None:
            out["colors"] = (col[:n][order] / 255.0).cpu().numpy()
        return out

    # ---------------------------------------------------------------- marching-cubes mesh (csrc/tsdf.hip, csrc/mesh_raster.hip)
    def _mesh_ws(self):
        n = int(_lib.load().sgam_tsdf_mesh_workspace_bytes(ctypes.byref(self.grid), self.max_bricks))
        if n < 0:
            raise ops.SgamHipError("sgam_tsdf_mesh_workspace_bytes: bad grid")
        return torch.empty((max(n, 1),), dtype=torch.uint8, device=self.device)

    def _mesh_buffers(self):
        """device buffers of the loop's mesh, sized once from mesh_budget_bytes: vertices, keys, triangles, counts, workspace"""
        if self._mesh is None:
            max_t = max(16, self.mesh_budget_bytes // (12 + 10))
            max_v = max(16, max_t // 2)
            self._mesh = {"vertices": torch.empty((max_v, 3), dtype=torch.float32, device=self.device),
                          "keys": torch.empty((max_v,), dtype=torch.int64, device=self.device),
                          "triangles": torch.empty((max_t, 3), dtype=torch.int32, device=self.device),
                          "counts": torch.zeros((4,), dtype=torch.int32, device=self.device),
                          "ws": self._mesh_ws()}
        return self._mesh

    def _extract_mesh(self, bufs, colors=None, cull=None):
        """one sgam_tsdf_extract_mesh_f32 call into `bufs`; cull = (T_w2c float32 4x4, H, W, K, z_near, z_far) or None"""
        if cull is None:
            w2c, H, W, fx, fy, cx, cy, zn, zf = None, 0, 0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0
        else:
            T, H, W, K, zn, zf = cull
            w2c = np.ascontiguousarray(T, dtype=np.float32)
            fx, fy, cx, cy = self._k4(K)
        check(_lib.load().sgam_tsdf_extract_mesh_f32(
            ctypes.byref(self.grid), ops._p(self.unit_table), ops._p(self.counters), ops._p(self.brick_tsdf),
            ops._p(self.brick_color if colors is not None else None), self.max_bricks, None if w2c is None else w2c.ctypes.data,
            H, W, fx, fy, cx, cy, float(zn), float(zf), ops._p(bufs["vertices"]), ops._p(colors), ops._p(bufs["keys"]),
            bufs["vertices"].shape[0], ops._p(bufs["triangles"]), bufs["triangles"].shape[0], ops._p(bufs["counts"]),
            ops._p(bufs["ws"]), bufs["ws"].numel(), ops._stream()), "sgam_tsdf_extract_mesh_f32")

    def _extract_mesh_sized(self, nv, nt):
        """marching cubes of the whole volume into fresh buffers of nv vertices / nt triangles, a second pass with the counted
        sizes when the first did not fit: (bufs, colours or None, vertices found, triangles found).  Syncs."""
        for _ in range(2):
            bufs = {"vertices": torch.empty((nv, 3), dtype=torch.float32, device=self.device),
                    "keys": torch.empty((nv,), dtype=torch.int64, device=self.device),
                    "triangles": torch.empty((nt, 3), dtype=torch.int32, device=self.device),
                    "counts": torch.zeros((4,), dtype=torch.int32, device=self.device), "ws": self._mesh_ws()}
            col = torch.empty((nv, 3), dtype=torch.float32, device=self.device) if self.brick_color is not None else None
            self._extract_mesh(bufs, col)
            fv, ft, over, _ = (int(v) for v in bufs["counts"].cpu())
            if over == 0:
                return bufs, col, fv, ft
            nv, nt = max(fv, 1), max(ft, 1)
        raise ops.SgamHipError("TSDF mesh extraction: the volume changed between the two passes")

    def extract_triangle_mesh(self):
        """`volume.extract_triangle_mesh()` (reference :777-826; the run tail's coloured mesh): marching cubes on the device
        (generated tables, not Open3D's — csrc/mc_tables.h), host numpy arrays: vertices (n,3) f32, triangles (m,3) int32 (vertices
        in key order, triangles in (cell, table) order: run-independent), keys (n,) int64 (the point extractor's), vertex_normals
        (n,3) — Open3D's compute_vertex_normals rule as recalled (unnormalised face cross products summed per vertex, then
        normalised), unpinned — and, when colour was fused, vertex_colors (n,3) in 0..1.  An export step: it syncs, and sizes its
        buffers to the mesh (a second pass when the first one did not fit)."""
        bufs, col, fv, ft = self._extract_mesh_sized(1 << 16, 1 << 17)
        v = bufs["vertices"][:fv].cpu().numpy()
        t = bufs["triangles"][:ft].cpu().numpy()
        out = {"vertices": v, "triangles": t, "keys": bufs["keys"][:fv].cpu().numpy(), "vertex_normals": vertex_normals(v, t)}
        if col is not None:
            out["vertex_colors"] = (col[:fv] / 255.0).cpu().numpy()
        return out

    def extract_mesh_device(self, max_vertices=None, max_triangles=None):
        """extract_triangle_mesh()'s mesh left on the device, for render_mesh_rgbd: a DeviceMesh (vertex colours in 0..255,
        None without fused colour).  max_vertices / max_triangles: the first pass's buffer sizes (default: those of
        extract_triangle_mesh; a second pass with the counted sizes when they do not fit).  An export-time call: it syncs."""
        bufs, col, fv, ft = self._extract_mesh_sized(int(max_vertices or 1 << 16), int(max_triangles or 1 << 17))
        return DeviceMesh(bufs["vertices"], col, bufs["triangles"], bufs["counts"], fv, ft)

    def render_mesh_depth(self, K, T_w2c, H, W, z_near, z_far, T_c2w=None, out=None):
        """The reference's per-step depth render (:777-826): extract_triangle_mesh() of the units in the view frustum, then the
        mesh's view-space z at the pose (render_to_depth_image(z_in_view_space=True), inf -> 0).  (H,W) fp32 device tensor; no
        host sync (mesh sizes stay on the device; an overflow of the mesh buffers is reported by check()).  T_c2w: unused (the
        signature of render_depth)."""
        T = np.ascontiguousarray(T_w2c, dtype=np.float32)
        if out is None:
            out = torch.empty((H, W), dtype=torch.float32, device=self.device)
        assert out.shape == (H, W) and out.dtype == torch.float32 and out.is_contiguous()
        bufs = self._mesh_buffers()
        self._extract_mesh(bufs, None, cull=(T, H, W, K, z_near, z_far))
        fx, fy, cx, cy = self._k4(K)
        check(_lib.load().sgam_mesh_render_depth_f32(
            ops._p(bufs["vertices"]), bufs["vertices"].shape[0], ops._p(bufs["triangles"]), bufs["triangles"].shape[0],
            ops._p(bufs["counts"]), H, W, fx, fy, cx, cy, T.ctypes.data, float(z_near), float(z_far), ops._p(out), ops._stream()),
            "sgam_mesh_render_depth_f32")
        return out

    def stats(self):
        """(bricks allocated, last frame's brick count, samples outside the box, pool overflows) — host sync."""
        return tuple(int(v) for v in self.counters[::32].cpu())

    def check(self):
        """Raise when the fusion silently lost geometry: units that could not be opened because the brick pool was
        exhausted, or depth samples that fell outside the scene box (the rendered target depth then has holes there).
        One host sync: call at checkpoints of the loop, not per frame."""
        bricks, _, outside, overflow = self.stats()
        if overflow > 0:
            raise ops.SgamHipError(f"TSDF brick pool exhausted: {overflow} unit openings dropped (pool of {self.max_bricks} "
                                   f"bricks, {min(bricks, self.max_bricks)} used); raise memory_budget_bytes / max_bricks")
        if self._mesh is not None:
            dropped = int(self._mesh["counts"][3])
            if dropped > 0:
                raise ops.SgamHipError(f"TSDF mesh buffers exhausted: {dropped} vertices / triangles dropped by render_mesh_depth "
                                       f"(buffers of {self._mesh['vertices'].shape[0]} vertices, {self._mesh['triangles'].shape[0]} "
                                       "triangles); raise mesh_budget_bytes")
        if outside > 0:
            import warnings
            warnings.warn(f"TSDF: {outside} depth samples fell outside the scene box and were not fused", RuntimeWarning)
        return bricks


# ---------------------------------------------------------------- coloured views of a device mesh (csrc/mesh_raster.hip)
class DeviceMesh:
    """the device buffers of a marching-cubes mesh (TsdfVolume.extract_mesh_device): vertices (capacity,3) fp32, vertex_colors
    (capacity,3) fp32 0..255 or None, triangles (capacity,3) int32, counts int32[4] (the extractor's mesh_counts: the kernels
    read the sizes there); n_vertices / n_triangles: the sizes as counted at extraction"""

    def __init__(self, vertices, vertex_colors, triangles, counts, n_vertices, n_triangles):
        self.vertices, self.vertex_colors, self.triangles, self.counts = vertices, vertex_colors, triangles, counts
        self.n_vertices, self.n_triangles = int(n_vertices), int(n_triangles)


RGBD_KEY_BUDGET = 64 << 20        # bytes of visibility keys per call of the kernel (8 B per sample and pose): 128 poses at 256 x 256


def render_mesh_rgbd(mesh, K, Ts_w2c, H, W, z_near, z_far, normals=False, u8=False, out=None, rgb=None):
    """Coloured RGB-D views of a DeviceMesh at the P world -> camera poses Ts_w2c (P,4,4), the pose as a grid dimension
    (sgam_mesh_render_rgbd_f32; P is chunked so that the key buffer stays within RGBD_KEY_BUDGET).  Returns device tensors
    {"depth" (P,H,W) fp32 view-space z, 0 = nothing hit; "rgb" (P,H,W,3) fp32 0..255, perspective-correct vertex colours;
    "normal" (P,H,W,3) with normals=True: the hit triangle's unit normal in view space, facing the camera; "rgb_u8" (P,H,W,3)
    uint8 with u8=True}.  Per pose the depth is bit for bit TsdfVolume.render_mesh_depth's on the same triangles.  rgb: None =
    when the mesh has colours; a mesh without colours renders depth and normals only and raises when asked for colour.
    out: a dict of destination tensors under the same names."""
    Ts = np.ascontiguousarray(np.asarray(Ts_w2c, dtype=np.float32).reshape(-1, 4, 4))
    P = Ts.shape[0]
    if P == 0:
        raise ops.SgamHipError("render_mesh_rgbd: no poses")
    has_col = mesh.vertex_colors is not None
    rgb = has_col if rgb is None else bool(rgb)
    if (rgb or u8) and not has_col:
        raise ops.SgamHipError("render_mesh_rgbd: the mesh has no vertex colours (extracted from a volume without color=True); "
                               "it renders depth and normals only")
    ops._need_cuda(mesh.vertices)
    dev = mesh.vertices.device
    want = {"depth": ((P, H, W), torch.float32)}
    if rgb:
        want["rgb"] = ((P, H, W, 3), torch.float32)
    if normals:
        want["normal"] = ((P, H, W, 3), torch.float32)
    if u8:
        want["rgb_u8"] = ((P, H, W, 3), torch.uint8)
    res = {}
    for name, (shape, dtype) in want.items():
        t = None if out is None else out.get(name)
        if t is None:
            t = torch.empty(shape, dtype=dtype, device=dev)
        assert tuple(t.shape) == shape and t.dtype == dtype and t.is_contiguous(), name
        res[name] = t
    lib = _lib.load()
    chunk = max(1, min(P, RGBD_KEY_BUDGET // (H * W * 8), 65535))
    ws = torch.empty((chunk * H * W,), dtype=torch.int64, device=dev)             # the keys: no initialisation needed
    poses = torch.from_numpy(Ts.reshape(P, 16)).pin_memory().to(dev, non_blocking=True)      # a DEVICE array: P poses do not fit the arguments
    fx, fy, cx, cy = TsdfVolume._k4(K)
    for p0 in range(0, P, chunk):
        n = min(chunk, P - p0)
        part = {k: ops._p(v[p0:p0 + n]) for k, v in res.items()}
        check(lib.sgam_mesh_render_rgbd_f32(
            ops._p(mesh.vertices), ops._p(mesh.vertex_colors), mesh.vertices.shape[0], ops._p(mesh.triangles), mesh.triangles.shape[0],
            ops._p(mesh.counts), n, H, W, fx, fy, cx, cy, ops._p(poses[p0:p0 + n]), float(z_near), float(z_far), part["depth"],
            part.get("rgb"), part.get("normal"), part.get("rgb_u8"), ops._p(ws), ws.numel() * 8, ops._stream()),
            "sgam_mesh_render_rgbd_f32")
    return res


# ---------------------------------------------------------------- scene-batched forms (lock-stepped scenes)
class _SceneSet:
    """Device tables of S volumes that advance together (sgam_tsdf_integrate_scenes_f32 / sgam_tsdf_raycast_scenes_f32): the
    scene table — the volumes' state pointers — is uploaded once; the per-step part (S x n sources, S target poses) goes through a
    ring of pinned staging buffers and one non-blocking copy into a persistent device buffer (no allocation, no sync per step:
    copies and launches are ordered by the stream, the ring keeps the host off a slot whose copy may still be in flight)."""
    RING = 4

    def __init__(self, volumes):
        v0 = volumes[0]
        for v in volumes[1:]:
            if (v.voxel_length, v.sdf_trunc) != (v0.voxel_length, v0.sdf_trunc) or tuple(v.base) != tuple(v0.base) or \
                    tuple(v.dims) != tuple(v0.dims) or torch.device(v.device) != torch.device(v0.device):
                raise ValueError("scene-batched TSDF: the volumes must share voxel length, truncation and the box of units "
                                 "(base, dims) on one device; integrate / render differing volumes one by one")
        if any((v.brick_color is None) != (v0.brick_color is None) for v in volumes):
            raise ValueError("scene-batched TSDF: colour volumes and geometry-only volumes cannot be mixed")
        self.refs = [weakref.ref(v) for v in volumes]
        self.S, self.device, self.color = len(volumes), v0.device, v0.brick_color is not None
        table = (_lib.TsdfScene * self.S)()
        for e, v in zip(table, volumes):
            for name in ("unit_table", "unit_stamp", "counters", "brick_list", "brick_tsdf", "brick_weight", "brick_color"):
                t = getattr(v, name)
                setattr(e, name, None if t is None else t.data_ptr())
            e.max_bricks, e.max_list = v.max_bricks, v.max_list
        self.scenes = torch.frombuffer(bytearray(bytes(table)), dtype=torch.uint8).to(self.device)
        nbytes = self.S * 8 * ctypes.sizeof(_lib.TsdfSrc)                      # the larger of the two per-step tables (8 sources)
        self.stage = [torch.empty(nbytes, dtype=torch.uint8).pin_memory() for _ in range(self.RING)]
        self.done = [None] * self.RING
        self.turn = 0
        self.dev_srcs = torch.empty(nbytes, dtype=torch.uint8, device=self.device)
        self.dev_poses = torch.empty(self.S * 64, dtype=torch.uint8, device=self.device)

    def matches(self, volumes):
        return len(volumes) == self.S and all(r() is v for r, v in zip(self.refs, volumes))

    def upload(self, dst, c_array):
        """host ctypes array -> the persistent device buffer `dst`, asynchronously"""
        n = ctypes.sizeof(c_array)
        i = self.turn
        self.turn = (i + 1) % self.RING
        if self.done[i] is not None:
            self.done[i].synchronize()                   # only ever waits when the host is a whole ring ahead
        ctypes.memmove(self.stage[i].data_ptr(), c_array, n)
        dst[:n].copy_(self.stage[i][:n], non_blocking=True)
        self.done[i] = torch.cuda.Event()
        self.done[i].record()
        return dst


def _scene_set(volumes):
    """the cached _SceneSet of exactly these volume objects (kept on the first one: a restarted volume is a new object, so a
    rewind of the loop rebuilds the table)"""
    volumes = list(volumes)
    if not volumes:
        raise ops.SgamHipError("scene-batched TSDF: no volumes")
    ss = getattr(volumes[0], "_scene_set", None)
    if ss is None or not ss.matches(volumes):
        ss = volumes[0]._scene_set = _SceneSet(volumes)
    return ss


def integrate_many_scenes(volumes, depths_per_scene, K, Ts_w2c_per_scene, Ts_c2w_per_scene=None, rgbs_u8_per_scene=None):
    """TsdfVolume.integrate_many for S volumes on one grid in one launch sequence (clear, open, integrate — whatever S): scene s
    fuses depths_per_scene[s] (n maps each, the same n for all) at Ts_w2c_per_scene[s], and is left with the values its own
    integrate_many call would leave.  Every volume's step counter advances."""
    ss = _scene_set(volumes)
    S = ss.S
    n = len(depths_per_scene[0])
    if len(depths_per_scene) != S or len(Ts_w2c_per_scene) != S or any(len(d) != n for d in depths_per_scene) or \
            any(len(T) != n for T in Ts_w2c_per_scene) or n == 0:
        raise ops.SgamHipError("integrate_many_scenes: one list of n >= 1 depth maps and n poses per scene, the same n for all")
    H, W = depths_per_scene[0][0].shape
    srcs = (_lib.TsdfSrc * (S * n))()
    keep = []
    if n <= 8:                                       # (more: the library's SGAM_EINVAL below, with nothing packed past the buffer)
        for s in range(S):
            for k in range(n):
                d = depths_per_scene[s][k]
                ops._need_cuda(d)
                if tuple(d.shape) != (H, W) or d.dtype != torch.float32:
                    raise ops.SgamHipError("integrate_many_scenes: depth maps must be (H,W) fp32 of one size")
                d = d.contiguous()
                rgb = None
                if ss.color:
                    rgb = None if rgbs_u8_per_scene is None else rgbs_u8_per_scene[s][k]
                    if rgb is None or rgb.dtype != torch.uint8 or tuple(rgb.shape) != (H, W, 3):
                        raise ops.SgamHipError("TsdfVolume(color=True).integrate needs the frame's (H,W,3) uint8 colour")
                    rgb = rgb.contiguous()
                keep.append((d, rgb))
                T = np.asarray(Ts_w2c_per_scene[s][k], dtype=np.float64)
                Ti = np.linalg.inv(T) if Ts_c2w_per_scene is None else np.asarray(Ts_c2w_per_scene[s][k], dtype=np.float64)
                e = srcs[s * n + k]
                e.depth, e.rgb_u8 = d.data_ptr(), None if rgb is None else rgb.data_ptr()
                e.cam2world[:] = Ti.astype(np.float32).ravel().tolist()
                e.world2cam[:] = T.astype(np.float32).ravel().tolist()
        ss.upload(ss.dev_srcs, srcs)
    v0 = volumes[0]
    fx, fy, cx, cy = v0._k4(K)
    rm = v0._ray_mult_table(H, W, fx, fy, cx, cy)
    step = max(v.frame_id for v in volumes) + 1       # one stamp for the launch: newer than any step a volume has seen
    check(_lib.load().sgam_tsdf_integrate_scenes_f32(
        ctypes.byref(v0.grid), ops._p(ss.scenes), ops._p(ss.dev_srcs), S, n, H, W, fx, fy, cx, cy, DEPTH_TRUNC, step,
        int(ss.color), ops._p(rm), ops._stream()), "sgam_tsdf_integrate_scenes_f32")
    for v in volumes:
        v.frame_id = step


def render_depth_scenes(volumes, K, Ts_w2c, H, W, z_near, z_far, Ts_c2w=None, out=None):
    """TsdfVolume.render_depth for S volumes on one grid at S poses in one launch: (S,H,W) fp32, 0 where nothing is hit."""
    ss = _scene_set(volumes)
    if len(Ts_w2c) != ss.S:
        raise ops.SgamHipError("render_depth_scenes: one pose per volume")
    poses = (ctypes.c_float * (ss.S * 16))()
    for s in range(ss.S):
        c2w = np.linalg.inv(np.asarray(Ts_w2c[s], dtype=np.float64)) if Ts_c2w is None else Ts_c2w[s]
        poses[s * 16:(s + 1) * 16] = np.asarray(c2w, dtype=np.float32).ravel().tolist()
    ss.upload(ss.dev_poses, poses)
    if out is None:
        out = torch.empty((ss.S, H, W), dtype=torch.float32, device=ss.device)
    assert out.shape == (ss.S, H, W) and out.dtype == torch.float32 and out.is_contiguous()
    v0 = volumes[0]
    fx, fy, cx, cy = v0._k4(K)
    check(_lib.load().sgam_tsdf_raycast_scenes_f32(
        ctypes.byref(v0.grid), ops._p(ss.scenes), ops._p(ss.dev_poses), ss.S, H, W, fx, fy, cx, cy, float(z_near), float(z_far),
        ops._p(out), None, ops._stream()), "sgam_tsdf_raycast_scenes_f32")
    return out


def vertex_normals(vertices, triangles):
    """Open3D's TriangleMesh.compute_vertex_normals rule as recalled (unpinned): the unnormalised cross product
    (v1 - v0) x (v2 - v0) of every face summed into its three vertices, then normalised (float64 on the host: an export step;
    meshops.vertex_normals is the same rule on the device with the summation order pinned)"""
    v = np.asarray(vertices, dtype=np.float64)
    t = np.asarray(triangles, dtype=np.int64).reshape(-1, 3)
    n = np.zeros_like(v)
    if len(t):
        fn = np.cross(v[t[:, 1]] - v[t[:, 0]], v[t[:, 2]] - v[t[:, 0]])
        for k in range(3):
            np.add.at(n, t[:, k], fn)
    ln = np.linalg.norm(n, axis=1, keepdims=True)
    return np.where(ln > 0, n / np.where(ln > 0, ln, 1.0), 0.0)
