"""Point-splat RGB-D views of stored frames (csrc/point_raster.hip: sgam_points_render_rgbd_f32): every pixel of every frame
unprojected with its own depth, moved into the view camera and splatted with a z-test, at all poses in one call.  The frames
are read where the frame store keeps them (one allocation per frame, through device tables of addresses); nothing comes back to
the host.  `InfiniteSceneGeneration.render_views(poses, source="points")` is the scene-level caller."""
import ctypes

import numpy as np
import torch

from . import _lib, ops
from .geometry import frame_store, inverse_intrinsics

KEY_BUDGET = 64 << 20        # bytes of visibility keys per call of the kernel (8 B per sample and pose): 128 poses at 256 x 256


def relative_transforms(Ts_view_w2c, Ts_src_w2c):
    """(P,F,3,4) fp32: T_view @ inv(T_src) (source camera -> view camera) in float64, rounded once.  A view whose 4x4 equals a
    source's gets the exact identity, so a frame seen from its own pose reproduces itself."""
    Tv = np.asarray(Ts_view_w2c, dtype=np.float64).reshape(-1, 4, 4)
    Ts = np.asarray(Ts_src_w2c, dtype=np.float64).reshape(-1, 4, 4)
    inv = [np.linalg.inv(S) for S in Ts]
    out = np.empty((len(Tv), len(Ts), 3, 4), dtype=np.float32)
    for p, V in enumerate(Tv):
        for f, S in enumerate(Ts):
            out[p, f] = (np.eye(4) if np.array_equal(V, S) else V @ inv[f])[:3]       # (the pipeline's T_tgt @ inv(T_src))
    return out


def render_points_rgbd(depths, rgbs_u8, K_src, Ts_src_w2c, K_view, Ts_view_w2c, H, W, z_near, z_far, radius=0, hole_fill=False,
                       T_rel=None, index=False, out=None):
    """RGB-D views of F frames at P poses.  depths: F device tensors (Hs,Ws) fp32; rgbs_u8: F device tensors (Hs,Ws,3) uint8 (each
    contiguous, read in place); K_src / K_view 3x3 (zero skew); Ts_src_w2c (F,4,4), Ts_view_w2c (P,4,4) world -> camera.  radius:
    0, 1 or 2 — every point covers (2 radius + 1)^2 samples; hole_fill: the 3x3 median fill of the samples nothing landed on.
    T_rel (P,F,3,4) fp32 replaces relative_transforms(Ts_view_w2c, Ts_src_w2c).  Returns device tensors {"depth" (P,H,W) fp32
    view-space z, 0 = nothing; "rgb" (P,H,W,3) fp32 0..255; "rgb_u8" (P,H,W,3) uint8; with index=True "index" (P,H,W) int32: the
    winning point f * Hs * Ws + q, -1 = nothing}.  out: a dict of destination tensors under the same names."""
    F, Hs, Ws, dev, ptrs = frame_store(depths, rgbs_u8, "render_points_rgbd")
    if T_rel is None:
        T_rel = relative_transforms(Ts_view_w2c, Ts_src_w2c)
    T_rel = np.ascontiguousarray(T_rel, dtype=np.float32)
    if T_rel.ndim != 4 or T_rel.shape[1:] != (F, 3, 4) or T_rel.shape[0] == 0:
        raise ops.SgamHipError(f"render_points_rgbd: T_rel is (P,{F},3,4), not {T_rel.shape}")
    P = T_rel.shape[0]
    H, W, radius = int(H), int(W), int(radius)
    Kinv = inverse_intrinsics(K_src)
    Kv = np.asarray(K_view, dtype=np.float64)
    fx, fy, cx, cy = float(Kv[0, 0]), float(Kv[1, 1]), float(Kv[0, 2]), float(Kv[1, 2])
    want = {"depth": ((P, H, W), torch.float32), "rgb": ((P, H, W, 3), torch.float32), "rgb_u8": ((P, H, W, 3), torch.uint8)}
    if index:
        want["index"] = ((P, H, W), torch.int32)
    res = {}
    for name, (shape, dtype) in want.items():
        t = None if out is None else out.get(name)
        if t is None:
            t = torch.empty(shape, dtype=dtype, device=dev)
        assert tuple(t.shape) == shape and t.dtype == dtype and t.is_contiguous() and t.device == dev, name
        res[name] = t
    rel = torch.from_numpy(T_rel.reshape(P, F * 12)).pin_memory().to(dev, non_blocking=True)
    lib = _lib.load()
    chunk = max(1, min(P, KEY_BUDGET // (H * W * 8), 65535))
    ws = torch.empty((chunk * H * W,), dtype=torch.int64, device=dev)             # the keys: no initialisation needed
    for p0 in range(0, P, chunk):
        n = min(chunk, P - p0)
        part = {k: ops._p(v[p0:p0 + n]) for k, v in res.items()}
        _lib.check(lib.sgam_points_render_rgbd_f32(
            ops._p(ptrs[:F]), ops._p(ptrs[F:]), F, Hs, Ws, ctypes.c_void_p(Kinv.ctypes.data), ops._p(rel[p0:p0 + n]), n, H, W, fx, fy,
            cx, cy, float(z_near), float(z_far), radius, int(bool(hole_fill)), part["depth"], part["rgb"], part["rgb_u8"],
            part.get("index"), ops._p(ws), ws.numel() * 8, ops._stream()), "sgam_points_render_rgbd_f32")
    return res
