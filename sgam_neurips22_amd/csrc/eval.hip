// eval.hip — the kernels of the reference's validation step (VQModel.evaluation_loop, sgam/generative_sensing_module/model.py:356-410)
// and of its image metrics (modules/misc/metrics.py: PSNR, SSIM, each with an optional visibility mask).  gfx950 only.
//
// Conventions of train.hip: the caller owns every buffer, launches go on the passed stream without a sync or an allocation, the
// reductions leave per-workgroup fp64 partial sums that the host folds (no float atomics: results are run-to-run identical);
// the histogram uses integer atomics, which are order-independent.
#include <math.h>

#include "sgam_common.h"

namespace {

// clip((v + 1) * 127.5, 0, 255) in fp32: [-1, 1] network range -> the 0..255 scale of the metrics (no uint8 truncation)
__device__ __forceinline__ float to255(float v) { return fminf(fmaxf((v + 1.0f) * 127.5f, 0.0f), 255.0f); }

// block-wide sum of one double per thread (256 threads) through `sh`; the total is returned to thread 0
__device__ __forceinline__ double block_sum_256(double v, double *sh) {
    __syncthreads();            // (sh may still be read from a previous use)
    sh[threadIdx.x] = v;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if ((int)threadIdx.x < o) sh[threadIdx.x] += sh[threadIdx.x + o];
        __syncthreads();
    }
    return sh[0];
}

// ---- reconstruction statistics: one pass over rec / target, no gradient.  Workgroup = (chunk of RS_PIX pixels, image);
// partial[(b * chunks + chunk) * 6 + k]:  0 sum|d| over all C channels, 1 sum|d| over channels 0..2, 2 sum|d| over channels >= 3,
// 3 sum d255^2 over channels 0..2, 4 the same times mask, 5 sum mask (3..5 only with `sq`; d255 = the difference on the 0..255 scale)
constexpr int RS_PIX = 1024;
__global__ __launch_bounds__(256) void recon_stats_kernel(const float *__restrict__ rec, const float *__restrict__ target,
                                                          const float *__restrict__ mask, double *__restrict__ partial, int HW, int C,
                                                          int ld_rec, int sq, int map255) {
    const int b = blockIdx.y;
    const int p0 = blockIdx.x * RS_PIX;
    double a_rgb = 0.0, a_rest = 0.0, s_sq = 0.0, s_sqm = 0.0, s_m = 0.0;
    for (int p = p0 + threadIdx.x; p < min(p0 + RS_PIX, HW); p += 256) {
        const int64_t r = (int64_t)b * HW + p;
        const float m = (sq && mask) ? mask[r] : 0.f;
        double e = 0.0;
        for (int c = 0; c < C; ++c) {
            const float x = rec[r * ld_rec + c], t = target[r * C + c];
            const double ad = (double)fabsf(x - t);
            if (c < 3) {
                a_rgb += ad;
                if (sq) {
                    const double d = map255 ? (double)to255(x) - (double)to255(t) : (double)x - (double)t;
                    e += d * d;
                }
            } else {
                a_rest += ad;
            }
        }
        s_sq += e;
        s_sqm += e * (double)m;
        s_m += (double)m;
    }
    __shared__ double sh[256];
    double *out = partial + ((int64_t)b * gridDim.x + blockIdx.x) * 6;
    const double v[6] = {a_rgb + a_rest, a_rgb, a_rest, s_sq, s_sqm, s_m};
    for (int k = 0; k < 6; ++k) {
        const double t = block_sum_256(v[k], sh);
        if (threadIdx.x == 0) out[k] = t;
    }
}

// ---- SSIM (metrics.py:59-83): 11 x 11 Gaussian window (sigma 1.5) as two separable passes, "valid" region (H-10) x (W-10).
// Workgroup = (16 x 16 tile of the valid region, channel, image): the 26 x 26 input patch of both images is staged in LDS
// (fp32, 5.3 KB), the row pass leaves the five moments x, y, x^2, y^2, xy of 26 rows x 16 columns in LDS as fp64 (16.3 KB), the
// column pass gives each thread the five filtered values of its output pixel, the SSIM value is formed in fp64 and the tile
// is reduced.  The filtered maps never leave the workgroup.  All moment arithmetic is fp64 (the inputs are fp32, so x^2 and
// xy are exact in fp64): E[x^2] - mu^2 at the 0..255 scale keeps ~1e-11 absolute, against C2 = 58.5.
constexpr int SS_T = 16, SS_R = 5, SS_IN = SS_T + 2 * SS_R;      // 26
struct SsimWin {
    double w[2 * SS_R + 1];
};
__global__ __launch_bounds__(256) void ssim_kernel(const float *__restrict__ img1, const float *__restrict__ img2, int ld1, int ld2,
                                                   const float *__restrict__ mask, double *__restrict__ partial, int H, int W,
                                                   int tiles_x, int map255, SsimWin win) {
    __shared__ float sx[SS_IN * SS_IN], sy[SS_IN * SS_IN];
    __shared__ double row[5][SS_IN * SS_T];
    const int tile = blockIdx.x, c = blockIdx.y, b = blockIdx.z;
    const int ty0 = (tile / tiles_x) * SS_T, tx0 = (tile % tiles_x) * SS_T;     // origin of the tile in the valid region = of its patch in the image
    for (int i = threadIdx.x; i < SS_IN * SS_IN; i += 256) {
        const int iy = ty0 + i / SS_IN, ix = tx0 + i % SS_IN;
        float x = 0.f, y = 0.f;
        if (iy < H && ix < W) {           // (outside: only read by outputs outside the valid region, which are not summed)
            const int64_t p = ((int64_t)b * H + iy) * W + ix;
            x = img1[p * ld1 + c];
            y = img2[p * ld2 + c];
            if (map255) x = to255(x), y = to255(y);
        }
        sx[i] = x;
        sy[i] = y;
    }
    __syncthreads();
    for (int i = threadIdx.x; i < SS_IN * SS_T; i += 256) {
        const int r = i / SS_T, q = i % SS_T;
        double m1 = 0.0, m2 = 0.0, s11 = 0.0, s22 = 0.0, s12 = 0.0;
#pragma unroll
        for (int k = 0; k <= 2 * SS_R; ++k) {
            const double x = (double)sx[r * SS_IN + q + k], y = (double)sy[r * SS_IN + q + k], w = win.w[k];
            m1 += w * x;
            m2 += w * y;
            s11 += w * (x * x);
            s22 += w * (y * y);
            s12 += w * (x * y);
        }
        row[0][i] = m1;
        row[1][i] = m2;
        row[2][i] = s11;
        row[3][i] = s22;
        row[4][i] = s12;
    }
    __syncthreads();
    const int oy = threadIdx.x / SS_T, ox = threadIdx.x % SS_T;
    double v = 0.0, vm = 0.0, ms = 0.0;
    if (ty0 + oy < H - 2 * SS_R && tx0 + ox < W - 2 * SS_R) {
        double m[5] = {0.0, 0.0, 0.0, 0.0, 0.0};
#pragma unroll
        for (int k = 0; k <= 2 * SS_R; ++k) {
            const double w = win.w[k];
#pragma unroll
            for (int j = 0; j < 5; ++j) m[j] += w * row[j][(oy + k) * SS_T + ox];
        }
        const double C1 = (0.01 * 255) * (0.01 * 255), C2 = (0.03 * 255) * (0.03 * 255);
        const double mu1_sq = m[0] * m[0], mu2_sq = m[1] * m[1], mu12 = m[0] * m[1];
        const double sig1 = m[2] - mu1_sq, sig2 = m[3] - mu2_sq, sig12 = m[4] - mu12;
        v = ((2.0 * mu12 + C1) * (2.0 * sig12 + C2)) / ((mu1_sq + mu2_sq + C1) * (sig1 + sig2 + C2));
        if (mask) {
            ms = (double)mask[((int64_t)b * H + ty0 + oy + SS_R) * W + tx0 + ox + SS_R];
            vm = v * ms;
        }
    }
    double *sh = &row[0][0];
    double *out = partial + (((int64_t)b * gridDim.y + c) * gridDim.x + tile) * 3;
    const double t0 = block_sum_256(v, sh);
    if (threadIdx.x == 0) out[0] = t0;
    const double t1 = block_sum_256(vm, sh);
    if (threadIdx.x == 0) out[1] = t1;
    const double t2 = block_sum_256(ms, sh);
    if (threadIdx.x == 0) out[2] = t2;
}

// ---- use counts of codebook indices, accumulated (hist is NOT cleared): integer atomics; an index outside [0, n_embed) is skipped
__global__ __launch_bounds__(256) void index_histogram_kernel(const int64_t *__restrict__ idx, int64_t n, int32_t *__restrict__ hist,
                                                              int n_embed) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const int64_t k = idx[i];
    if (k >= 0 && k < n_embed) atomicAdd(&hist[k], 1);
}

}  // namespace

extern "C" int64_t sgam_recon_stats_partials(int32_t B, int32_t HW) {
    if (B <= 0 || HW <= 0) return SGAM_EINVAL;
    return (int64_t)B * sgam_cdiv(HW, RS_PIX) * 6;
}

extern "C" int sgam_recon_stats_f32(const float *rec, const float *target, const float *mask, double *partial, int32_t B, int32_t HW,
                                    int32_t C, int32_t ld_rec, int32_t with_sq, int32_t map255, void *stream) {
    if (!rec || !target || !partial || B <= 0 || HW <= 0 || C <= 0 || ld_rec < C || B > 65535) return SGAM_EINVAL;
    if (mask && !with_sq) return SGAM_EINVAL;
    SGAM_KLAUNCH(recon_stats_kernel, dim3(sgam_cdiv(HW, RS_PIX), B), dim3(256), 0, sgam_stream(stream), rec, target, mask, partial, HW, C,
                 ld_rec, with_sq ? 1 : 0, map255 ? 1 : 0);
    SGAM_LAUNCH_CHECK();
    return SGAM_OK;
}

extern "C" int64_t sgam_ssim_partials(int32_t B, int32_t H, int32_t W, int32_t C) {
    if (B <= 0 || C <= 0 || H < 2 * SS_R + 1 || W < 2 * SS_R + 1) return SGAM_EINVAL;
    return (int64_t)B * C * sgam_cdiv(H - 2 * SS_R, SS_T) * sgam_cdiv(W - 2 * SS_R, SS_T) * 3;
}

extern "C" int sgam_ssim_f32(const float *img1, const float *img2, const float *mask, double *partial, int32_t B, int32_t H, int32_t W,
                             int32_t C, int32_t ld1, int32_t ld2, int32_t map255, void *stream) {
    if (!img1 || !img2 || !partial || B <= 0 || C <= 0 || H < 2 * SS_R + 1 || W < 2 * SS_R + 1 || ld1 < C || ld2 < C || B > 65535 ||
        C > 65535)
        return SGAM_EINVAL;
    SsimWin win;                     // the normalised 1-D Gaussian exp(-(i - 5)^2 / (2 * 1.5^2)), i = 0..10
    double s = 0.0;
    for (int i = 0; i <= 2 * SS_R; ++i) s += win.w[i] = exp(-(double)((i - SS_R) * (i - SS_R)) / (2.0 * 1.5 * 1.5));
    for (int i = 0; i <= 2 * SS_R; ++i) win.w[i] /= s;
    const int tx = sgam_cdiv(W - 2 * SS_R, SS_T), ty = sgam_cdiv(H - 2 * SS_R, SS_T);
    SGAM_KLAUNCH(ssim_kernel, dim3(tx * ty, C, B), dim3(256), 0, sgam_stream(stream), img1, img2, ld1, ld2, mask, partial, H, W, tx,
                 map255 ? 1 : 0, win);
    SGAM_LAUNCH_CHECK();
    return SGAM_OK;
}

extern "C" int sgam_index_histogram_i32(const int64_t *indices, int64_t n, int32_t *hist, int32_t n_embed, void *stream) {
    if (!indices || !hist || n <= 0 || n_embed <= 0) return SGAM_EINVAL;
    SGAM_KLAUNCH(index_histogram_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, sgam_stream(stream), indices, n, hist, n_embed);
    SGAM_LAUNCH_CHECK();
    return SGAM_OK;
}
