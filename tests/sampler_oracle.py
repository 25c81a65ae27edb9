"""CPU restatement of the device-side top-k infill sampler (include/sgam_hip.h, sgam_vq_sample_topk_f32): the six steps of the
draw rule in numpy, integer Philox4x32-10 in uint64 arithmetic.  Test infrastructure only — the product path never imports it."""
import numpy as np

M0, M1 = 0xD2511F53, 0xCD9E8D57
W0, W1 = 0x9E3779B9, 0xBB67AE85
MASK32 = 0xFFFFFFFF
# a draw is compared with the device's only where u*total is at least this far (relative to total) from every cumulative
# weight: device expf and numpy exp may differ in the last bits of each of up to 32 terms (32 terms x 2 ulp x 2^-24, rounded up)
BAND = 4e-6


def philox4x32_10(ctr, key):
    """ctr: 4 arrays (or ints) of 32-bit words, key: 2.  Returns the 4 output words as uint64 arrays holding 32-bit values."""
    c = [np.asarray(v, dtype=np.uint64) & np.uint64(MASK32) for v in ctr]
    c = list(np.broadcast_arrays(*c))
    k0, k1 = int(key[0]) & MASK32, int(key[1]) & MASK32
    for _ in range(10):
        p0 = np.uint64(M0) * c[0]            # 32 x 32 -> 64 bits: exact in uint64
        p1 = np.uint64(M1) * c[2]
        hi0, lo0 = p0 >> np.uint64(32), p0 & np.uint64(MASK32)
        hi1, lo1 = p1 >> np.uint64(32), p1 & np.uint64(MASK32)
        c = [hi1 ^ c[1] ^ np.uint64(k0), lo1, hi0 ^ c[3] ^ np.uint64(k1), lo0]
        k0, k1 = (k0 + W0) & MASK32, (k1 + W1) & MASK32
    return c


def uniforms(seed, stream_ids, call, T, S):
    """step 4: u[b][t][s] float32 in [0, 1) = (word0 >> 8) * 2^-24"""
    seed, call = int(seed) & 0xFFFFFFFFFFFFFFFF, int(call) & 0xFFFFFFFFFFFFFFFF
    c0 = (np.arange(T, dtype=np.uint64)[:, None] * np.uint64(S) + np.arange(S, dtype=np.uint64)[None, :])[None]   # (1,T,S)
    c1 = (np.asarray(stream_ids, dtype=np.int64) & MASK32).astype(np.uint64)[:, None, None]                        # (B,1,1)
    w0 = philox4x32_10((c0, c1, call & MASK32, call >> 32), (seed & MASK32, seed >> 32))[0]
    return ((w0 >> np.uint64(8)).astype(np.float32) * np.float32(2.0 ** -24)).astype(np.float32)


def resize_mask_nearest(mask, h, w):
    """step 5's resize: (B,H,W) -> (B,h,w) with src = floor(dst * H / h) (F.interpolate(mode='nearest'))"""
    B, H, W = mask.shape
    sy = np.minimum((np.arange(h, dtype=np.int64) * H) // h, H - 1)
    sx = np.minimum((np.arange(w, dtype=np.int64) * W) // w, W - 1)
    return mask[:, sy][:, :, sx]


def cumulative_weights(vals_rows, temperature):
    """step 3 on rows (..., k) of ascending distances: c (..., k) float32, sequential fp32 sums in slot order"""
    v = np.asarray(vals_rows, dtype=np.float32)
    x = (-(v - v[..., :1])).astype(np.float32) / np.float32(temperature)
    e = np.exp(x.astype(np.float32)).astype(np.float32)
    c = np.empty_like(e)
    run = np.zeros(e.shape[:-1], dtype=np.float32)
    for j in range(e.shape[-1]):
        run = (run + e[..., j]).astype(np.float32)
        c[..., j] = run
    return c


def sample(vals, inds, hw, S, seed, stream_ids, call, mask=None, per_token=False, temperature=1.0, codebook=None):
    """vals / inds (B*T, k) as ops.vq_topk returns them (step 1 is the caller's), mask (B,H,W) bool or None.
    Returns dict(indices (B,S,h,w) int64, slots (B,T,S), band (B,T,S) bool: draws inside the expf band (not comparable),
    zq (B,S,h,w,D) when a codebook is given)."""
    h, w = hw
    T = h * w
    vals = np.asarray(vals, dtype=np.float32)
    inds = np.asarray(inds, dtype=np.int64)
    k = vals.shape[1]
    B = vals.shape[0] // T
    vals, inds = vals.reshape(B, T, k), inds.reshape(B, T, k)
    rows = vals if per_token else np.broadcast_to(vals[:, :1], vals.shape)          # step 2
    c = cumulative_weights(rows, temperature)                                        # (B,T,k)
    total = c[..., -1]
    u = uniforms(seed, stream_ids, call, T, S)                                       # (B,T,S)
    ut = (u * total[..., None]).astype(np.float32)
    below = ut[..., None] < c[:, :, None, :]                                         # (B,T,S,k)
    slots = np.where(below.any(-1), below.argmax(-1), k - 1)                         # first j with u*total < c_j, else the last
    band = (np.abs(ut[..., None].astype(np.float64) - c[:, :, None, :].astype(np.float64))
            <= BAND * total[:, :, None, None].astype(np.float64)).any(-1)
    if k == 1:
        band[:] = False
    if mask is not None:
        hole = resize_mask_nearest(np.asarray(mask).reshape(B, *np.asarray(mask).shape[-2:]) != 0, h, w).reshape(B, T)
        slots = np.where(hole[..., None], slots, 0)
        band = band & hole[..., None]
    idx = np.take_along_axis(inds, slots, axis=2)                                    # (B,T,S)
    out = {"indices": idx.transpose(0, 2, 1).reshape(B, S, h, w), "slots": slots, "band": band, "cum": c}
    if codebook is not None:
        out["zq"] = np.asarray(codebook)[out["indices"]]
    return out


def slot_probabilities(vals_row, temperature=1.0):
    """the distribution the draws follow, in float64, from the fp32 cumulative weights the rule defines"""
    c = cumulative_weights(np.asarray(vals_row, dtype=np.float32)[None], temperature)[0].astype(np.float64)
    return np.diff(np.concatenate([[0.0], c])) / c[-1]
