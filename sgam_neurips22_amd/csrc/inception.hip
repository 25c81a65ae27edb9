// inception.hip — what the FID evaluation (sgam_neurips22_amd/fid.py: the reference's modules/misc/pytorch_fid) needs next to the
// fp32-in MFMA convolution of conv_gemm.hip: the input preprocessing (ToTensor scaling, bilinear resize to 299 x 299, 2x - 1), the
// three 3 x 3 pools of the FID Inception, the global average and the streaming fp64 activation statistics.  gfx950 only.
//
// Conventions of eval.hip: NHWC fp32, the caller owns every buffer, launches go on the passed stream without a sync or an
// allocation, no float atomics (every result is run-to-run identical).  Built with -ffp-contract=off: every fused multiply-add
// below is an explicit fma().
//
// The statistics run on the fp64 VALU, not on v_mfma_f64: on CDNA4 the two have the same peak (the fp64 matrix rate was halved
// against CDNA3), and the update is a (d x n) x (n x d) product with n <= a batch of images (2048^2 x 50 x 2 = 0.4 GFLOP), far
// below a millisecond either way; the VALU form keeps the summation order of a tile the plain row order.
#include "sgam_common.h"

namespace {

// ---- preprocessing: (B,H,W,3) uint8 or fp32 in [0,1] -> (B,Ho,Wo,4) fp32, channel 3 = 0.  PyTorch's bilinear rule with
// align_corners = False and no antialiasing (upsample_bilinear2d): scale = (float)in / out, src = max((dst + 0.5) * scale - 0.5, 0),
// i0 = (int)src, i1 = i0 + (i0 < in - 1), l1 = src - i0, l0 = 1 - l1; out = h0 * (w0 * v00 + w1 * v01) + h1 * (w0 * v10 + w1 * v11).
// Ho = H, Wo = W gives l1 = 0 everywhere: an exact copy (resize_input = False).
template <bool U8>
__device__ __forceinline__ float pp_load(const void *in, int64_t i) {
    if constexpr (U8) return (float)((const uint8_t *)in)[i] / 255.0f;
    return ((const float *)in)[i];
}

template <bool U8>
__global__ __launch_bounds__(256) void preprocess_kernel(const void *__restrict__ in, float *__restrict__ out, int B, int H, int W, int Ho,
                                                         int Wo, float sy, float sx, int normalize) {
    const int64_t q = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (q >= (int64_t)B * Ho * Wo) return;
    const int ox = (int)(q % Wo);
    const int oy = (int)((q / Wo) % Ho);
    const int b = (int)(q / ((int64_t)Wo * Ho));
    const float fy = fmaxf(((float)oy + 0.5f) * sy - 0.5f, 0.0f);
    const float fx = fmaxf(((float)ox + 0.5f) * sx - 0.5f, 0.0f);
    const int y0 = min((int)fy, H - 1), x0 = min((int)fx, W - 1);
    const int y1 = y0 + (y0 < H - 1 ? 1 : 0), x1 = x0 + (x0 < W - 1 ? 1 : 0);
    const float h1 = fy - (float)y0, w1 = fx - (float)x0;
    const float h0 = 1.0f - h1, w0 = 1.0f - w1;
    const int64_t r0 = ((int64_t)b * H + y0) * W, r1 = ((int64_t)b * H + y1) * W;
    f32x4 o;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const float v00 = pp_load<U8>(in, (r0 + x0) * 3 + c), v01 = pp_load<U8>(in, (r0 + x1) * 3 + c);
        const float v10 = pp_load<U8>(in, (r1 + x0) * 3 + c), v11 = pp_load<U8>(in, (r1 + x1) * 3 + c);
        float v = h0 * (w0 * v00 + w1 * v01) + h1 * (w0 * v10 + w1 * v11);
        if (normalize) v = 2.0f * v - 1.0f;
        o[c] = v;
    }
    o[3] = 0.0f;
    *reinterpret_cast<f32x4 *>(out + q * 4) = o;
}

// ---- 3 x 3 pools.  mode 0: max, stride 2, no padding; 1: max, stride 1, padding 1 (padding never wins: taps outside the map are
// skipped); 2: average, stride 1, padding 1, count_include_pad = False: the valid taps summed in (ky, kx) order in fp32, divided
// by their count.  One thread per (output pixel, channel); channel pitches of both sides are free (concat slices).
__global__ __launch_bounds__(256) void pool3x3_kernel(const float *__restrict__ x, float *__restrict__ out, int B, int H, int W, int C, int ldx,
                                                      int Ho, int Wo, int ldo, int mode) {
    const int64_t q = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (q >= (int64_t)B * Ho * Wo * C) return;
    const int c = (int)(q % C);
    const int64_t pix = q / C;
    const int ox = (int)(pix % Wo);
    const int oy = (int)((pix / Wo) % Ho);
    const int b = (int)(pix / ((int64_t)Wo * Ho));
    const int stride = mode == 0 ? 2 : 1, pad = mode == 0 ? 0 : 1;
    float m = -__builtin_inff(), s = 0.0f;
    int cnt = 0;
    for (int ky = 0; ky < 3; ++ky) {
        const int iy = oy * stride - pad + ky;
        if (iy < 0 || iy >= H) continue;
        for (int kx = 0; kx < 3; ++kx) {
            const int ix = ox * stride - pad + kx;
            if (ix < 0 || ix >= W) continue;
            const float v = x[(((int64_t)b * H + iy) * W + ix) * ldx + c];
            m = fmaxf(m, v);
            s += v;
            ++cnt;
        }
    }
    out[pix * ldo + c] = mode == 2 ? s / (float)cnt : m;
}

// ---- global average: (B,HW,C) -> (B,C), fp64 accumulation, one rounding to fp32.  Workgroup = (64 channels, image): four
// pixel phases of 64 channel lanes, each a serial fp64 sum over its pixels p = phase, phase + 4, ..., joined in phase order.
__global__ __launch_bounds__(256) void global_avgpool_kernel(const float *__restrict__ x, float *__restrict__ out, int HW, int C, int ldx) {
    __shared__ double sh[256];
    const int c = blockIdx.x * 64 + (threadIdx.x & 63), phase = threadIdx.x >> 6, b = blockIdx.y;
    double s = 0.0;
    if (c < C)
        for (int p = phase; p < HW; p += 4) s += (double)x[((int64_t)b * HW + p) * ldx + c];
    sh[threadIdx.x] = s;
    __syncthreads();
    if (phase == 0 && c < C) {
        const double t = ((sh[threadIdx.x] + sh[threadIdx.x + 64]) + sh[threadIdx.x + 128]) + sh[threadIdx.x + 192];
        out[(int64_t)b * C + c] = (float)(t / (double)HW);
    }
}

// ---- streaming activation statistics.  state (fp64): [0] count, [1 .. d] sum of (x - shift), [1 + d .. 2d] shift,
// [1 + 2d ..] the d x d Gram of (x - shift), of which only the 64 x 64 tiles on and above the tile diagonal are kept.  The first
// batch fixes shift to its own column mean, so the centred values stay of the size of the spread and the subtraction
// gram - sum sum^T / N of the finalize loses nothing to a large mean.
constexpr int ST_T = 64, ST_K = 16;

__global__ __launch_bounds__(256) void stats_sum_kernel(const float *__restrict__ x, int n, int d, int ldx, double *__restrict__ state,
                                                        int first) {
    const int j = blockIdx.x * 256 + threadIdx.x;
    if (j == 0) state[0] = (first ? 0.0 : state[0]) + (double)n;
    if (j >= d) return;
    double *sum = state + 1, *shift = state + 1 + d;
    double sh = shift[j], acc = sum[j];
    if (first) {
        double s = 0.0;
        for (int r = 0; r < n; ++r) s += (double)x[(int64_t)r * ldx + j];
        sh = s / (double)n;
        shift[j] = sh;
        acc = 0.0;
    }
    for (int r = 0; r < n; ++r) acc += (double)x[(int64_t)r * ldx + j] - sh;
    sum[j] = acc;
}

// Workgroup = one 64 x 64 tile (bi <= bj) of the Gram; a thread owns a 4 x 4 patch and walks the batch rows in order, 16 rows of
// centred fp64 values per LDS stage: gram[i][j] = fma(a_r[i], a_r[j], gram[i][j]) for r = 0 .. n - 1, continuing from the stored
// value.  The product is commutative, so a diagonal tile is symmetric bit for bit.
__global__ __launch_bounds__(256) void stats_gram_kernel(const float *__restrict__ x, int n, int d, int ldx, double *__restrict__ state,
                                                         int first) {
    const int bi = blockIdx.y, bj = blockIdx.x;
    if (bi > bj) return;
    __shared__ double As[ST_K][ST_T], Bs[ST_K][ST_T];
    const double *shift = state + 1 + d;
    double *gram = state + 1 + 2 * (int64_t)d;
    const int ty = threadIdx.x >> 4, tx = threadIdx.x & 15;
    const int i0 = bi * ST_T + ty * 4, j0 = bj * ST_T + tx * 4;
    double acc[4][4];
#pragma unroll
    for (int a = 0; a < 4; ++a)
#pragma unroll
        for (int b = 0; b < 4; ++b)
            acc[a][b] = (first || i0 + a >= d || j0 + b >= d) ? 0.0 : gram[(int64_t)(i0 + a) * d + j0 + b];
    // staging: thread -> (row r = tid / 16 + 0, four columns (tid % 16) * 4 ..) of both tiles
    const int sr = threadIdx.x >> 4, sc = (threadIdx.x & 15) * 4;
    double sha[4], shb[4];
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        const int ca = bi * ST_T + sc + e, cb = bj * ST_T + sc + e;
        sha[e] = ca < d ? shift[ca] : 0.0;
        shb[e] = cb < d ? shift[cb] : 0.0;
    }
    for (int r0 = 0; r0 < n; r0 += ST_K) {
        const int r = r0 + sr;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const int ca = bi * ST_T + sc + e, cb = bj * ST_T + sc + e;
            As[sr][sc + e] = (r < n && ca < d) ? (double)x[(int64_t)r * ldx + ca] - sha[e] : 0.0;
            Bs[sr][sc + e] = (r < n && cb < d) ? (double)x[(int64_t)r * ldx + cb] - shb[e] : 0.0;
        }
        __syncthreads();
#pragma unroll 4
        for (int k = 0; k < ST_K; ++k) {
            double av[4], bv[4];
#pragma unroll
            for (int e = 0; e < 4; ++e) av[e] = As[k][ty * 4 + e], bv[e] = Bs[k][tx * 4 + e];
#pragma unroll
            for (int a = 0; a < 4; ++a)
#pragma unroll
                for (int b = 0; b < 4; ++b) acc[a][b] = fma(av[a], bv[b], acc[a][b]);
        }
        __syncthreads();
    }
#pragma unroll
    for (int a = 0; a < 4; ++a)
#pragma unroll
        for (int b = 0; b < 4; ++b)
            if (i0 + a < d && j0 + b < d) gram[(int64_t)(i0 + a) * d + j0 + b] = acc[a][b];
}

// mu = shift + sum / N; sigma[i][j] = (gram[i][j] - sum[i] sum[j] / N) / (N - 1), gram read from the kept (upper) tile of the
// pair, so sigma[i][j] and sigma[j][i] come from the same stored value and the same commutative product: equal bit for bit.
__global__ __launch_bounds__(256) void stats_finalize_kernel(const double *__restrict__ state, int d, double *__restrict__ mu,
                                                             double *__restrict__ sigma) {
    const int64_t q = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (q >= (int64_t)d * d) return;
    const int i = (int)(q / d), j = (int)(q % d);
    const double N = state[0];
    const double *sum = state + 1, *shift = state + 1 + d, *gram = state + 1 + 2 * (int64_t)d;
    if (i == 0) mu[j] = shift[j] + sum[j] / N;
    const bool upper = i / ST_T <= j / ST_T;
    const double g = upper ? gram[(int64_t)i * d + j] : gram[(int64_t)j * d + i];
    sigma[q] = (g - (sum[i] * sum[j]) / N) / (N - 1.0);
}

}  // namespace

extern "C" int sgam_inception_preprocess_f32(const void *in, int32_t in_is_u8, int32_t B, int32_t H, int32_t W, float *out, int32_t Ho,
                                             int32_t Wo, int32_t normalize, void *stream) {
    if (!in || !out || B <= 0 || H <= 0 || W <= 0 || Ho <= 0 || Wo <= 0) return SGAM_EINVAL;
    if ((int64_t)B * H * W * 3 >= (1ll << 40) || (int64_t)B * Ho * Wo >= (1ll << 31) * 256) return SGAM_EINVAL;
    if (!sgam_aligned16(out)) return SGAM_EALIGN;
    const float sy = (float)H / (float)Ho, sx = (float)W / (float)Wo;
    const dim3 grid(sgam_cdiv((int64_t)B * Ho * Wo, 256));
    if (in_is_u8) {
        SGAM_KLAUNCH(preprocess_kernel<true>, grid, dim3(256), 0, sgam_stream(stream), in, out, B, H, W, Ho, Wo, sy, sx, normalize ? 1 : 0);
    } else {
        SGAM_KLAUNCH(preprocess_kernel<false>, grid, dim3(256), 0, sgam_stream(stream), in, out, B, H, W, Ho, Wo, sy, sx, normalize ? 1 : 0);
    }
    SGAM_LAUNCH_CHECK();
    return SGAM_OK;
}

extern "C" int sgam_pool3x3_out_size(int32_t H, int32_t W, int32_t mode, int32_t *Ho, int32_t *Wo) {
    if (H <= 0 || W <= 0 || mode < 0 || mode > 2 || (mode == 0 && (H < 3 || W < 3))) return SGAM_EINVAL;
    if (Ho) *Ho = mode == 0 ? (H - 3) / 2 + 1 : H;
    if (Wo) *Wo = mode == 0 ? (W - 3) / 2 + 1 : W;
    return SGAM_OK;
}

extern "C" int sgam_pool3x3_nhwc_f32(const float *x, int32_t B, int32_t H, int32_t W, int32_t C, int32_t ldx, float *out, int32_t ldo,
                                     int32_t mode, void *stream) {
    int32_t Ho = 0, Wo = 0;
    if (!x || !out || B <= 0 || C <= 0 || ldx < C || ldo < C) return SGAM_EINVAL;
    if (sgam_pool3x3_out_size(H, W, mode, &Ho, &Wo) != SGAM_OK) return SGAM_EINVAL;
    const int64_t total = (int64_t)B * Ho * Wo * C;
    if (total >= (1ll << 31) * 256) return SGAM_EINVAL;
    SGAM_KLAUNCH(pool3x3_kernel, dim3(sgam_cdiv(total, 256)), dim3(256), 0, sgam_stream(stream), x, out, B, H, W, C, ldx, Ho, Wo, ldo,
                 mode);
    SGAM_LAUNCH_CHECK();
    return SGAM_OK;
}

extern "C" int sgam_global_avgpool_nhwc_f32(const float *x, int32_t B, int32_t HW, int32_t C, int32_t ldx, float *out, void *stream) {
    if (!x || !out || B <= 0 || B > 65535 || HW <= 0 || C <= 0 || ldx < C) return SGAM_EINVAL;
    SGAM_KLAUNCH(global_avgpool_kernel, dim3(sgam_cdiv(C, 64), B), dim3(256), 0, sgam_stream(stream), x, out, HW, C, ldx);
    SGAM_LAUNCH_CHECK();
    return SGAM_OK;
}

extern "C" int64_t sgam_activation_stats_state_doubles(int32_t d) {
    if (d <= 0 || d > 32768) return SGAM_EINVAL;
    return 1 + 2 * (int64_t)d + (int64_t)d * d;
}

extern "C" int sgam_activation_stats_update_f64(const float *x, int32_t n, int32_t d, int32_t ldx, double *state, int32_t first,
                                                void *stream) {
    if (!x || !state || n <= 0 || d <= 0 || d > 32768 || ldx < d) return SGAM_EINVAL;
    hipStream_t s = sgam_stream(stream);
    SGAM_KLAUNCH(stats_sum_kernel, dim3(sgam_cdiv(d, 256)), dim3(256), 0, s, x, n, d, ldx, state, first ? 1 : 0);
    SGAM_LAUNCH_CHECK();
    const int t = sgam_cdiv(d, ST_T);
    SGAM_KLAUNCH(stats_gram_kernel, dim3(t, t), dim3(256), 0, s, x, n, d, ldx, state, first ? 1 : 0);
    SGAM_LAUNCH_CHECK();
    return SGAM_OK;
}

extern "C" int sgam_activation_stats_finalize_f64(const double *state, int32_t d, double *mu, double *sigma, void *stream) {
    if (!state || !mu || !sigma || d <= 0 || d > 32768) return SGAM_EINVAL;
    SGAM_KLAUNCH(stats_finalize_kernel, dim3(sgam_cdiv((int64_t)d * d, 256)), dim3(256), 0, sgam_stream(stream), state, d, mu, sigma);
    SGAM_LAUNCH_CHECK();
    return SGAM_OK;
}
