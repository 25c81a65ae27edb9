// view_consistency.hip — reprojection (warping) error between stored frames (sgam_view_consistency_f32): the pixels of frame s put
// into camera t with their own depth, and compared with the depths and colours frame t holds there.  What frame_drift measures as a
// rigid residual between clouds, measured in the image: per ordered pair (s, t) a class per source pixel — which tells a hidden
// surface (harmless) from a free-space violation (t sees through a point s claims) — and the colour and depth errors of the pixels
// both frames see.  Reads the frame store in place through the DEVICE address tables geometry.frame_store builds.
//
// Per pair p = (s, t) and source pixel (row i, column j); T_rel[p] = the top 3 x 4 of T_t T_s^-1 (float64 on the host, rounded
// once).  Every operator below is ONE IEEE fp32 operation, in the written order, nothing fused (points_common.h states the rule
// and holds the unprojection):
//     valid(x) := fabsf(x) <= F32_MAX && z_near <= x && x <= z_far                     (NaN fails; unproject_frames' rule)
//     d = depth_s[i][j]                                        class 0 INVALID      unless valid(d)
//     (X, Y, Z) = points_common.h's unprojection of (i, j, d) with T_rel[p]
//                                                              class 1 OUT_OF_VIEW  unless z_near <= Z && Z <= z_far
//     u = (fx * X) / Z + cx        v = (fy * Y) / Z + cy       (point_raster.hip's projection)
//     x0f = floorf(u)   y0f = floorf(v)                        class 1 OUT_OF_VIEW  unless 0 <= x0f && x0f <= W - 2 && 0 <= y0f && y0f <= H - 2
//     wx = u - x0f   wy = v - y0f   x0 = (int)x0f   y0 = (int)y0f                      (float compares: the last row and column of t
//                                                                                       never receive a footprint; u == W - 1 is out)
//     D00 D01 D10 D11 = depth_t at (y0, x0) (y0, x0 + 1) (y0 + 1, x0) (y0 + 1, x0 + 1)
//     Dn = the corner at (y0 + (wy >= 0.5f), x0 + (wx >= 0.5f))
//                                                              class 2 TARGET_HOLE  unless valid(Dn)
//     e = Z - Dn                                               class 3 OCCLUDED     if  e > tau   (the point is behind what t sees)
//                                                              class 4 VIOLATION    if -e > tau   (t sees through the point)
//                                                              class 5 EDGE         unless every corner Dk is valid and fabsf(Z - Dk) <= tau
//     class 6 COVISIBLE:
//       lerp(p00, p01, p10, p11) = top + wy * (bot - top),  top = p00 + wx * (p01 - p00),  bot = p10 + wx * (p11 - p10)
//       ez = Z - lerp(D..)                                     depth_error = ez
//       per channel c: ec = (float)rgb_s[i][j][c] - lerp((float) of the four uint8 corners of rgb_t)
//       color_error = (|er| + |eg|) + |eb|                     (units of 0..255)
// sums[p][0..11], fp64: [0..6] the seven class counts, and over the covisible pixels [7] S1 = sum color_error, [8] S2 = sum
// (er^2 + eg^2) + eb^2 (each e converted to double before squaring), [9] S3 = sum |ez|, [10] S4 = sum ez^2 (in double), [11] S5 =
// sum |ez| / Z (the division in fp32).  Order of summation: a lane holds one pixel; block_sum_f64<12> per workgroup; the pair's
// workgroups folded in block order from 0.0 by a second small launch.  No atomics: two calls give the same bits.
// tests/consistency_oracle.py restates all of this in numpy; the maps are compared bit for bit.
//
// Launch shape (latency-bound gathers, no MFMA): one lane per (pair, source pixel) on a grid (blocks over H W, P); consecutive
// lanes take consecutive pixels, so the source reads coalesce and pairs[p], T_rel[p] are wave-uniform.  Dn is one of the four
// corners, so a lane in view needs four depth gathers and twelve colour bytes (two runs of six) — addresses known once (x0, y0) is.
// They are all requested together, with the source colour, BEFORE the classification, which is written as selects: a lane in
// view pays one memory round trip after its own depth, not one per class test.  Lanes that are invalid or out of view request
// nothing.
#include "points_common.h"

namespace {

constexpr int VC_SUMS = 12;
constexpr int FOLD_BATCH = 16;            // workgroup sums the fold requests before it adds the first

struct ViewCheck {
    float kinv[9];                        // the shared intrinsics, inverted in float64 and rounded once (host)
    float fx, fy, cx, cy, zn, zf, tau;
    int H, W, F;
};

__device__ __forceinline__ bool depth_valid(float x, float zn, float zf) { return fabsf(x) <= F32_MAX && zn <= x && x <= zf; }

__device__ __forceinline__ float lerp4(float p00, float p01, float p10, float p11, float wx, float wy) {
    const float top = __fadd_rn(p00, __fmul_rn(wx, __fsub_rn(p01, p00)));
    const float bot = __fadd_rn(p10, __fmul_rn(wx, __fsub_rn(p11, p10)));
    return __fadd_rn(top, __fmul_rn(wy, __fsub_rn(bot, top)));
}

// grid (blocks over the H W source pixels, P): one lane per (pair, source pixel); partial [P][gridDim.x][12]
__global__ __launch_bounds__(256) void view_consistency_kernel(ViewCheck V, const float *const *__restrict__ depth_ptrs,
                                                               const uint8_t *const *__restrict__ rgb_ptrs,
                                                               const int32_t *__restrict__ pairs, const float *__restrict__ T_rel,
                                                               double *__restrict__ partial, uint8_t *__restrict__ class_map,
                                                               float *__restrict__ color_error, float *__restrict__ depth_error) {
    const int64_t hw = (int64_t)V.H * V.W;
    const int64_t q = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int p = blockIdx.y;
    const int s = pairs[2 * p], t = pairs[2 * p + 1];                          // wave-uniform
    const bool pair_ok = s >= 0 && s < V.F && t >= 0 && t < V.F;               // (the Python front checks; a bad pair reads nothing)
    const bool live = q < hw && pair_ok;
    // the four frame addresses, read with the pair (scalar loads): none of them waits behind the projection
    const float *__restrict__ depth_s = pair_ok ? depth_ptrs[s] : nullptr, *__restrict__ depth_t = pair_ok ? depth_ptrs[t] : nullptr;
    const uint8_t *__restrict__ rgb_s = pair_ok ? rgb_ptrs[s] : nullptr, *__restrict__ rgb_t = pair_ok ? rgb_ptrs[t] : nullptr;
    int cls = 0;
    float ce = 0.0f, ez = 0.0f, er = 0.0f, eg = 0.0f, eb = 0.0f, rel = 0.0f;
    if (live) {
        const int i = (int)(q / V.W), j = (int)(q - (int64_t)i * V.W);
        const float d = depth_s[q];
        if (depth_valid(d, V.zn, V.zf)) {
            float a, b, c, X, Y, Z;
            pixel_ray(V.kinv, i, j, a, b, c);
            transform34(T_rel + (int64_t)p * 12, __fmul_rn(a, d), __fmul_rn(b, d), __fmul_rn(c, d), X, Y, Z);
            const float u = __fadd_rn(__fdiv_rn(__fmul_rn(V.fx, X), Z), V.cx);
            const float v = __fadd_rn(__fdiv_rn(__fmul_rn(V.fy, Y), Z), V.cy);
            const float x0f = floorf(u), y0f = floorf(v);
            cls = 1;
            if (V.zn <= Z && Z <= V.zf && 0.0f <= x0f && x0f <= (float)(V.W - 2) && 0.0f <= y0f && y0f <= (float)(V.H - 2)) {
                const float wx = __fsub_rn(u, x0f), wy = __fsub_rn(v, y0f);
                const int x0 = (int)x0f, y0 = (int)y0f;                         // 0 <= x0 <= W - 2, 0 <= y0 <= H - 2
                const int64_t o = (int64_t)y0 * V.W + x0;                       // o + W + 1 <= H W - 1
                const float *__restrict__ dt = depth_t + o;
                const uint8_t *__restrict__ ct = rgb_t + o * 3, *__restrict__ cb = ct + (int64_t)V.W * 3;
                const uint8_t *__restrict__ cs = rgb_s + q * 3;
                // every gather of the lane, requested before anything looks at a value
                const float D00 = dt[0], D01 = dt[1], D10 = dt[V.W], D11 = dt[V.W + 1];
                uint8_t top[6], bot[6], src[3];
#pragma unroll
                for (int k = 0; k < 6; ++k) { top[k] = ct[k]; bot[k] = cb[k]; }
#pragma unroll
                for (int k = 0; k < 3; ++k) src[k] = cs[k];
                // the classification, as selects
                const bool right = wx >= 0.5f, down = wy >= 0.5f;
                const float Dn = down ? (right ? D11 : D10) : (right ? D01 : D00);
                const float e = __fsub_rn(Z, Dn);
                const bool all_ok = depth_valid(D00, V.zn, V.zf) && depth_valid(D01, V.zn, V.zf) && depth_valid(D10, V.zn, V.zf) &&
                                    depth_valid(D11, V.zn, V.zf) && fabsf(__fsub_rn(Z, D00)) <= V.tau && fabsf(__fsub_rn(Z, D01)) <= V.tau &&
                                    fabsf(__fsub_rn(Z, D10)) <= V.tau && fabsf(__fsub_rn(Z, D11)) <= V.tau;
                cls = !depth_valid(Dn, V.zn, V.zf) ? 2 : e > V.tau ? 3 : -e > V.tau ? 4 : !all_ok ? 5 : 6;
                const bool cov = cls == 6;
                float ech[3];
#pragma unroll
                for (int k = 0; k < 3; ++k)
                    ech[k] = __fsub_rn((float)src[k], lerp4((float)top[k], (float)top[3 + k], (float)bot[k], (float)bot[3 + k], wx, wy));
                const float z_err = __fsub_rn(Z, lerp4(D00, D01, D10, D11, wx, wy));
                er = cov ? ech[0] : 0.0f; eg = cov ? ech[1] : 0.0f; eb = cov ? ech[2] : 0.0f;
                ez = cov ? z_err : 0.0f;
                ce = __fadd_rn(__fadd_rn(fabsf(er), fabsf(eg)), fabsf(eb));
                rel = cov ? __fdiv_rn(fabsf(z_err), Z) : 0.0f;
            }
        }
    }
    if (q < hw) {
        const int64_t o = (int64_t)p * hw + q;
        if (class_map) class_map[o] = (uint8_t)cls;
        if (color_error) color_error[o] = ce;
        if (depth_error) depth_error[o] = ez;
    }
    double sum[VC_SUMS];
#pragma unroll
    for (int k = 0; k < 7; ++k) sum[k] = (live && cls == k) ? 1.0 : 0.0;
    const double dr = (double)er, dg = (double)eg, db = (double)eb, dz = (double)ez;
    sum[7] = (double)ce;
    sum[8] = (dr * dr + dg * dg) + db * db;
    sum[9] = (double)fabsf(ez);
    sum[10] = dz * dz;
    sum[11] = (double)rel;
    block_sum_f64<VC_SUMS>(sum, partial + (int64_t)p * gridDim.x * VC_SUMS);
}

// one lane per (pair, slot): sums[p][c] = the pair's nb workgroup sums folded in block order from 0.0
__global__ __launch_bounds__(256) void view_consistency_fold_kernel(const double *__restrict__ partial, int nb, int64_t n,
                                                                    double *__restrict__ sums) {
    const int64_t k = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= n) return;
    const int64_t p = k / VC_SUMS;
    const int c = (int)(k - p * VC_SUMS);
    const double *__restrict__ src = partial + p * nb * VC_SUMS + c;
    double acc = 0.0;
    int b = 0;
    for (; b + FOLD_BATCH <= nb; b += FOLD_BATCH) {                             // the loads of a batch in flight together, added in order
        double v[FOLD_BATCH];
#pragma unroll
        for (int k2 = 0; k2 < FOLD_BATCH; ++k2) v[k2] = src[(int64_t)(b + k2) * VC_SUMS];
#pragma unroll
        for (int k2 = 0; k2 < FOLD_BATCH; ++k2) acc += v[k2];
    }
    for (; b < nb; ++b) acc += src[(int64_t)b * VC_SUMS];
    sums[k] = acc;
}

}  // namespace

extern "C" int64_t sgam_view_consistency_workspace_bytes(int32_t H, int32_t W, int32_t P) {
    if (H < 2 || W < 2 || P < 1 || P > 65535 || (int64_t)H * W >= (1ll << 31)) return SGAM_EINVAL;
    return r16((int64_t)P * blocks_of((int64_t)H * W) * VC_SUMS * 8);        // the per-workgroup partial sums
}

extern "C" int sgam_view_consistency_f32(const void *depth_ptrs, const void *rgb_ptrs, int32_t F, int32_t H, int32_t W, const float *kinv9,
                                         float fx, float fy, float cx, float cy, float z_near, float z_far, float depth_tolerance,
                                         const int32_t *pairs, const float *T_rel, int32_t P, double *sums, uint8_t *class_map,
                                         float *color_error, float *depth_error, void *workspace, int64_t workspace_bytes, void *stream) {
    if (!depth_ptrs || !rgb_ptrs || !kinv9 || !pairs || !T_rel || !sums || F < 1 || !(depth_tolerance >= 0.0f) ||
        !(z_near <= z_far))                                                     // (a NaN fails both compares)
        return SGAM_EINVAL;
    if (!workspace_fits(workspace, workspace_bytes, sgam_view_consistency_workspace_bytes(H, W, P))) return SGAM_EINVAL;
    ViewCheck V;
    for (int i = 0; i < 9; ++i) V.kinv[i] = kinv9[i];
    V.fx = fx; V.fy = fy; V.cx = cx; V.cy = cy; V.zn = z_near; V.zf = z_far; V.tau = depth_tolerance;
    V.H = H; V.W = W; V.F = F;
    hipStream_t s = sgam_stream(stream);
    const unsigned nb = blocks_of((int64_t)H * W);
    double *partial = (double *)workspace;
    SGAM_KLAUNCH(view_consistency_kernel, dim3(nb, (unsigned)P), dim3(256), 0, s, V, (const float *const *)depth_ptrs,
                 (const uint8_t *const *)rgb_ptrs, pairs, T_rel, partial, class_map, color_error, depth_error);
    const int64_t n = (int64_t)P * VC_SUMS;
    SGAM_KLAUNCH(view_consistency_fold_kernel, dim3(blocks_of(n)), dim3(256), 0, s, (const double *)partial, (int)nb, n, sums);
    SGAM_LAUNCH_CHECK();
    return SGAM_OK;
}
