"""numpy restatement of the point-splat RGB-D render (csrc/point_raster.hip: sgam_points_render_rgbd_f32) for tests: float32
arrays, one numpy operation per operator of the kernel's stated arithmetic, np.minimum.at on uint64 keys, the same resolve and
the same 3x3 fill.  The GPU outputs are compared with it bit for bit."""
import numpy as np

f32 = np.float32
KEY_CLEAR = np.uint64(0xFFFFFFFFFFFFFFFF)


def project_keys(depths, Kinv, T_rel, H, W, fx, fy, cx, cy, z_near, z_far, radius):
    """keys (P,H,W) uint64 after every point's atomicMin.  depths: F arrays (Hs,Ws) fp32; Kinv fp32[9]; T_rel (P,F,3,4) fp32."""
    Kinv = np.asarray(Kinv, dtype=f32).reshape(9)
    T_rel = np.asarray(T_rel, dtype=f32)
    P, F = T_rel.shape[:2]
    Hs, Ws = depths[0].shape
    assert F == len(depths) and F * Hs * Ws < 1 << 32
    fx, fy, cx, cy, z_near, z_far = (f32(v) for v in (fx, fy, cx, cy, z_near, z_far))
    i, j = np.meshgrid(np.arange(Hs), np.arange(Ws), indexing="ij")
    q = (i * Ws + j).ravel().astype(np.uint64)
    fi, fj = i.ravel().astype(f32), j.ravel().astype(f32)
    keys = np.full((P, H * W), KEY_CLEAR, dtype=np.uint64)
    lo, hi_u, hi_v = f32(-(radius + 1)), f32(W + radius), f32(H + radius)
    with np.errstate(all="ignore"):
        a = (Kinv[0] * fj + Kinv[1] * fi) + Kinv[2]
        b = (Kinv[3] * fj + Kinv[4] * fi) + Kinv[5]
        c = (Kinv[6] * fj + Kinv[7] * fi) + Kinv[8]
        for p in range(P):
            for f in range(F):
                d = np.asarray(depths[f], dtype=f32).ravel()
                T = T_rel[p, f].reshape(12)
                ok = np.isfinite(d) & (d > 0)
                x, y, z = a * d, b * d, c * d
                X = ((T[0] * x + T[1] * y) + T[2] * z) + T[3]
                Y = ((T[4] * x + T[5] * y) + T[6] * z) + T[7]
                Z = ((T[8] * x + T[9] * y) + T[10] * z) + T[11]
                assert X.dtype == Y.dtype == Z.dtype == f32
                ok &= (z_near <= Z) & (Z <= z_far)
                u = (fx * X) / Z + cx
                v = (fy * Y) / Z + cy
                uf, vf = np.floor(u + f32(0.5)), np.floor(v + f32(0.5))
                assert uf.dtype == f32
                ok &= (lo < uf) & (uf < hi_u) & (lo < vf) & (vf < hi_v)
                px, py = uf[ok].astype(np.int64), vf[ok].astype(np.int64)
                key = (Z[ok].view(np.uint32).astype(np.uint64) << np.uint64(32)) | (np.uint64(f * Hs * Ws) + q[ok])
                for dy in range(-radius, radius + 1):
                    for dx in range(-radius, radius + 1):
                        xx, yy = px + dx, py + dy
                        inside = (xx >= 0) & (xx < W) & (yy >= 0) & (yy < H)
                        np.minimum.at(keys[p], yy[inside] * W + xx[inside], key[inside])
    return keys.reshape(P, H, W)


def fill(depth, rgb, empty):
    """the 3x3 fill of one view: empty samples get, per channel, the 5th smallest of the nine window values of the UNFILLED image
    (outside the image and empty samples = 0).  depth (H,W), rgb (H,W,3) fp32 with zeros at the empty samples."""
    H, W = depth.shape
    img = np.concatenate([rgb, depth[..., None]], axis=-1).astype(f32)
    pad = np.zeros((H + 2, W + 2, 4), dtype=f32)
    pad[1:-1, 1:-1] = img
    win = np.stack([pad[dy:dy + H, dx:dx + W] for dy in range(3) for dx in range(3)])
    med = np.sort(win, axis=0)[4]
    out = np.where(empty[..., None], med, img)
    return out[..., 3].copy(), out[..., :3].copy()


def resolve(keys, rgbs_u8, hole_fill):
    """{"depth" (P,H,W) f32, "rgb" (P,H,W,3) f32, "rgb_u8" (P,H,W,3) u8, "index" (P,H,W) i32} of the keys"""
    colours = np.concatenate([np.asarray(c, dtype=np.uint8).reshape(-1, 3) for c in rgbs_u8])
    empty = keys == KEY_CLEAR
    ids = (keys & np.uint64(0xFFFFFFFF)).astype(np.int64)
    depth = np.where(empty, f32(0), (keys >> np.uint64(32)).astype(np.uint32).view(f32)).astype(f32)
    rgb = np.where(empty[..., None], f32(0), colours[np.where(empty, 0, ids)].astype(f32)).astype(f32)
    index = np.where(empty, -1, ids.astype(np.uint32).view(np.int32)).astype(np.int32)
    if hole_fill:
        for p in range(keys.shape[0]):
            depth[p], rgb[p] = fill(depth[p], rgb[p], empty[p])
    return {"depth": depth, "rgb": rgb, "rgb_u8": rgb.astype(np.uint8), "index": index}


def render(depths, rgbs_u8, Kinv, T_rel, H, W, fx, fy, cx, cy, z_near, z_far, radius=0, hole_fill=False):
    keys = project_keys(depths, Kinv, T_rel, H, W, fx, fy, cx, cy, z_near, z_far, radius)
    return resolve(keys, rgbs_u8, hole_fill)


def kinv32(K):
    """what the launcher is given: the float64 inverse of the intrinsics rounded once"""
    return np.linalg.inv(np.asarray(K, dtype=np.float64)).astype(f32).reshape(9)
