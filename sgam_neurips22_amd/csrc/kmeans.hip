// kmeans.hip — device-resident online k-means codebook refresh (VQModel.training_step, sgam/generative_sensing_module/model.py:274-295
// and :313-323; scipy.cluster.vq.kmeans2 on the host in the reference).  gfx950 only.
//
// Conventions of train.hip / eval.hip: the caller owns every buffer, launches go on the passed stream without a sync or an
// allocation, and nothing here uses float atomics — every floating-point sum is folded in an order that depends on the data alone
// (ascending point id inside a cluster), never on launch geometry.  Integer atomics (the label histogram) are order-independent.
#include <math.h>

#include "sgam_common.h"

namespace {

constexpr int KM_PAD = 128;          // centre table rows are padded to a multiple of this (whole 128-column GEMM tiles)
constexpr int KM_ALIGN = 256;        // byte alignment of every workspace section

inline int64_t km_up(int64_t v, int64_t m) { return (v + m - 1) / m * m; }
inline int km_kpad(int k) { return (int)km_up(k, KM_PAD); }

// ---- assignment ----------------------------------------------------------------------------------------------------------
// padded centre table + |c|^2: one wavefront per row.  Rows >= k are zero with |c|^2 = +inf, so they never win the arg-min.
// The sum of squares is the fmaf chain of row_sumsq_kernel (vq.hip): the quantiser's own e_sq.
__global__ __launch_bounds__(256) void km_pad_centres_kernel(const float *__restrict__ centres, float *__restrict__ tab,
                                                             float *__restrict__ c_sq, int k, int kpad, int D) {
    const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= kpad) return;
    const int lane = threadIdx.x & 63;
    float s = 0.f;
    for (int c = lane; c < D; c += 64) {
        const float v = row < k ? centres[(int64_t)row * D + c] : 0.f;
        tab[(int64_t)row * D + c] = v;
        s = __fmaf_rn(v, v, s);
    }
    s = sgam_wave_sum(s);
    if (lane == 0) c_sq[row] = row < k ? s : INFINITY;
}

__device__ __forceinline__ void km_argmin_combine(float &d, int &j, float od, int oj) {
    if (od < d || (od == d && oj < j)) {
        d = od;
        j = oj;
    }
}

// one workgroup per point: d_j = (|x|^2 + |c_j|^2) - 2 x.c_j in the quantiser's order (vq_argmin_kernel), first index of ties
__global__ __launch_bounds__(256) void km_argmin_kernel(const float *__restrict__ x, const float *__restrict__ c_sq,
                                                        const float *__restrict__ dots, int32_t *__restrict__ labels, int D,
                                                        int kpad) {
    const int t = blockIdx.x;
    const float *xr = x + (int64_t)t * D;
    __shared__ float red_f[4];
    __shared__ int red_i[4];
    __shared__ float bc_f;

    float xx = 0.f;
    for (int c = threadIdx.x; c < D; c += 256) xx = __fmaf_rn(xr[c], xr[c], xx);
    xx = sgam_wave_sum(xx);
    if ((threadIdx.x & 63) == 0) red_f[threadIdx.x >> 6] = xx;
    __syncthreads();
    if (threadIdx.x == 0) bc_f = (red_f[0] + red_f[1]) + (red_f[2] + red_f[3]);
    __syncthreads();
    xx = bc_f;
    __syncthreads();

    const float *dr = dots + (int64_t)t * kpad;
    float best = INFINITY;
    int bj = 0x7fffffff;
    for (int j = threadIdx.x; j < kpad; j += 256) {
        const float d = __fsub_rn(__fadd_rn(xx, c_sq[j]), __fmul_rn(2.0f, dr[j]));
        if (d < best) {  // strict: the lowest j among equal distances survives within a lane
            best = d;
            bj = j;
        }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const float od = __shfl_xor(best, o, 64);
        const int oj = __shfl_xor(bj, o, 64);
        km_argmin_combine(best, bj, od, oj);
    }
    if ((threadIdx.x & 63) == 0) {
        red_f[threadIdx.x >> 6] = best;
        red_i[threadIdx.x >> 6] = bj;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        float d = red_f[0];
        int j = red_i[0];
        for (int w = 1; w < 4; ++w) km_argmin_combine(d, j, red_f[w], red_i[w]);
        labels[t] = (j == 0x7fffffff) ? 0 : j;  // a row without a finite distance
    }
}

sgam_conv_desc km_dot_desc(int32_t T, int32_t D, int32_t kpad) {
    // dots[t][j] = x[t] . c[j]: the quantiser's 1x1 "conv" over T pixels with the centre table as the weight matrix (vq.hip)
    sgam_conv_desc d = {};
    d.B = 1; d.Hi = 1; d.Wi = T; d.Cin = D; d.Ho = 1; d.Wo = T; d.N = kpad;
    d.KH = 1; d.KW = 1; d.stride = 1; d.pad_t = 0; d.pad_l = 0; d.upsample2x = 0;
    d.lda = D; d.ldb = D; d.ldc = kpad; d.ldr = 0; d.n_valid = kpad; d.bias_per_row = 0;
    return d;
}

bool km_shape_ok(int32_t N, int32_t D, int32_t k) { return N > 0 && k > 0 && D > 0 && D % 32 == 0 && k <= (1 << 24); }

struct AssignLayout {
    int64_t tab, c_sq, dots, conv, total, conv_bytes;
};

bool km_assign_layout(int32_t N, int32_t D, int32_t k, int32_t chunk, AssignLayout *L) {
    if (!km_shape_ok(N, D, k) || chunk <= 0) return false;
    const int kpad = km_kpad(k);
    const int rows = chunk < N ? chunk : N;
    int64_t conv = 0;
    const int parts[2] = {rows, N % rows};              // the whole chunks and the ragged last one
    for (int i = 0; i < 2; ++i) {
        if (parts[i] == 0) continue;
        const sgam_conv_desc d = km_dot_desc(parts[i], D, kpad);
        const int64_t b = sgam_conv2d_workspace_bytes(&d);
        if (b < 0) return false;
        conv = b > conv ? b : conv;
    }
    L->tab = 0;
    L->c_sq = km_up(L->tab + (int64_t)kpad * D * 4, KM_ALIGN);
    L->dots = km_up(L->c_sq + (int64_t)kpad * 4, KM_ALIGN);
    L->conv = km_up(L->dots + (int64_t)rows * kpad * 4, KM_ALIGN);
    L->conv_bytes = conv;
    L->total = km_up(L->conv + conv, KM_ALIGN);
    return true;
}

// ---- update: stable counting sort of the point ids by label, then one workgroup per centre -------------------------------
// histogram of one block of `pb` consecutive points: hist[block][label] (zeroed by the caller; integer atomics)
__global__ __launch_bounds__(256) void km_block_hist_kernel(const int32_t *__restrict__ labels, int32_t *__restrict__ hist, int N, int k,
                                                            int pb) {
    const int64_t p0 = (int64_t)blockIdx.x * pb;
    for (int i = threadIdx.x; i < pb && p0 + i < N; i += 256) {
        const int l = labels[p0 + i];
        if (l >= 0 && l < k) atomicAdd(&hist[(int64_t)blockIdx.x * k + l], 1);
    }
}

// per label: exclusive scan down the blocks (hist[b][j] becomes the number of members in blocks < b), total into count[j]
__global__ __launch_bounds__(256) void km_scan_blocks_kernel(int32_t *__restrict__ hist, int32_t *__restrict__ count, int nblk, int k) {
    const int j = blockIdx.x * 256 + threadIdx.x;
    if (j >= k) return;
    int run = 0;
    for (int b = 0; b < nblk; ++b) {
        const int t = hist[(int64_t)b * k + j];
        hist[(int64_t)b * k + j] = run;
        run += t;
    }
    count[j] = run;
}

// start[j] = sum of count[0..j), start[k] = the number of labelled points.  One workgroup; thread t owns a contiguous range.
__global__ __launch_bounds__(256) void km_scan_counts_kernel(const int32_t *__restrict__ count, int32_t *__restrict__ start, int k) {
    __shared__ int part[256];
    const int per = (k + 255) / 256;
    const int j0 = threadIdx.x * per, j1 = min(j0 + per, k);
    int s = 0;
    for (int j = j0; j < j1; ++j) s += count[j];
    part[threadIdx.x] = s;
    __syncthreads();
    if (threadIdx.x == 0) {
        int run = 0;
        for (int t = 0; t < 256; ++t) {
            const int v = part[t];
            part[t] = run;
            run += v;
        }
        start[k] = run;
    }
    __syncthreads();
    int run = part[threadIdx.x];
    for (int j = j0; j < j1; ++j) {
        start[j] = run;
        run += count[j];
    }
}

constexpr int KM_PB_MAX = 4096;
// order[start[l] + members of l in earlier blocks + members of l earlier in this block] = point id: ascending ids per label
__global__ __launch_bounds__(256) void km_place_kernel(const int32_t *__restrict__ labels, const int32_t *__restrict__ hist,
                                                       const int32_t *__restrict__ start, int32_t *__restrict__ order, int N, int k,
                                                       int pb) {
    __shared__ int lab[KM_PB_MAX];
    const int64_t p0 = (int64_t)blockIdx.x * pb;
    const int n = (int)min((int64_t)pb, (int64_t)N - p0);
    for (int i = threadIdx.x; i < n; i += 256) lab[i] = labels[p0 + i];
    __syncthreads();
    for (int i = threadIdx.x; i < n; i += 256) {
        const int l = lab[i];
        if (l < 0 || l >= k) continue;
        int r = 0;
        for (int q = 0; q < i; ++q) r += (lab[q] == l) ? 1 : 0;
        order[start[l] + hist[(int64_t)blockIdx.x * k + l] + r] = (int)(p0 + i);
    }
}

// one workgroup per centre.  Wavefront w sums the members s = w, w + 4, ... of the segment (ascending point ids) in fp64, a lane
// owns four channels; the four partial sums are joined as (s0 + s1) + (s2 + s3); mean = fp32(sum / count).  An empty centre is
// left as it is.
__global__ __launch_bounds__(256) void km_centre_mean_kernel(const float *__restrict__ x, const int32_t *__restrict__ order,
                                                             const int32_t *__restrict__ start, float *__restrict__ centres, int D) {
    const int j = blockIdx.x;
    const int s0 = start[j], s1 = start[j + 1];
    if (s1 <= s0) return;
    __shared__ double part[4][256];
    const int w = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const double cnt = (double)(s1 - s0);
    for (int c0 = 0; c0 < D; c0 += 256) {
        const int c = c0 + lane * 4;
        double a0 = 0.0, a1 = 0.0, a2 = 0.0, a3 = 0.0;
        if (c < D) {
#pragma unroll 4
            for (int s = s0 + w; s < s1; s += 4) {
                const f32x4 v = *reinterpret_cast<const f32x4 *>(x + (int64_t)order[s] * D + c);
                a0 += (double)v[0];
                a1 += (double)v[1];
                a2 += (double)v[2];
                a3 += (double)v[3];
            }
        }
        __syncthreads();  // (part may still be read from the previous slab)
        part[w][lane * 4 + 0] = a0;
        part[w][lane * 4 + 1] = a1;
        part[w][lane * 4 + 2] = a2;
        part[w][lane * 4 + 3] = a3;
        __syncthreads();
        const int cc = c0 + (int)threadIdx.x;
        if (cc < D) {
            const double tot = (part[0][threadIdx.x] + part[1][threadIdx.x]) + (part[2][threadIdx.x] + part[3][threadIdx.x]);
            centres[(int64_t)j * D + cc] = (float)(tot / cnt);
        }
    }
}

struct UpdateLayout {
    int64_t hist, start, order, total, hist_bytes;
    int nblk;
};

bool km_update_layout(int32_t N, int32_t k, int32_t pb, UpdateLayout *L) {
    if (N <= 0 || k <= 0 || pb < 256 || pb > KM_PB_MAX || pb % 256 != 0) return false;
    L->nblk = sgam_cdiv(N, pb);
    L->hist = 0;
    L->hist_bytes = (int64_t)L->nblk * k * 4;
    L->start = km_up(L->hist_bytes, KM_ALIGN);
    L->order = km_up(L->start + ((int64_t)k + 1) * 4, KM_ALIGN);
    L->total = km_up(L->order + (int64_t)N * 4, KM_ALIGN);
    return true;
}

// ---- minit = 'points' ------------------------------------------------------------------------------------------------------
__device__ __forceinline__ uint32_t km_philox_word0(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0, uint32_t k1) {
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        const uint32_t hi0 = __umulhi(0xD2511F53u, c0), lo0 = 0xD2511F53u * c0;
        const uint32_t hi1 = __umulhi(0xCD9E8D57u, c2), lo1 = 0xCD9E8D57u * c2;
        c0 = hi1 ^ c1 ^ k0;
        c1 = lo1;
        c2 = hi0 ^ c3 ^ k1;
        c3 = lo0;
        k0 += 0x9E3779B9u;
        k1 += 0xBB67AE85u;
    }
    return c0;
}

// one wavefront per slot: every lane walks the same permutation cycle, then the 64 lanes copy the picked row
__global__ __launch_bounds__(256) void km_init_points_kernel(const float *__restrict__ x, float *__restrict__ centres,
                                                             int32_t *__restrict__ picks, int N, int D, int k, int half_bits,
                                                             uint32_t seed_lo, uint32_t seed_hi, uint32_t ref_lo, uint32_t ref_hi) {
    const int slot = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (slot >= k) return;
    const int lane = threadIdx.x & 63;
    const uint32_t mask = (1u << half_bits) - 1u;
    uint32_t v = (uint32_t)slot;
    do {
        uint32_t L = v >> half_bits, R = v & mask;
#pragma unroll
        for (uint32_t r = 0; r < 4; ++r) {
            const uint32_t f = km_philox_word0(R, r, ref_lo, ref_hi, seed_lo, seed_hi) & mask;
            const uint32_t nr = L ^ f;
            L = R;
            R = nr;
        }
        v = (L << half_bits) | R;
    } while (v >= (uint32_t)N);
    if (lane == 0 && picks) picks[slot] = (int32_t)v;
    for (int c = lane; c < D; c += 64) centres[(int64_t)slot * D + c] = x[(int64_t)v * D + c];
}

// ---- codeword countdowns (model.py:313-323) and the row scatter of update_codebook -----------------------------------------
// ONE workgroup: (1) countdown[idx] = timeout for the T indices, (2) countdown[:] -= 1, (3) the words at <= 0 counted and listed
// in ascending order (thread t owns a contiguous range of words, the ranges are joined by an exclusive scan over the threads).
__global__ __launch_bounds__(1024) void km_countdown_kernel(const int64_t *__restrict__ indices, int T, int32_t *__restrict__ countdown,
                                                            int n, int timeout, int32_t *__restrict__ n_dead, int32_t *__restrict__ dead) {
    __shared__ int part[1024];
    for (int t = threadIdx.x; t < T; t += 1024) {
        const int64_t i = indices[t];
        if (i >= 0 && i < n) countdown[i] = timeout;
    }
    __syncthreads();
    const int per = (n + 1023) / 1024;
    const int j0 = min((int)threadIdx.x * per, n), j1 = min(j0 + per, n);
    int c = 0;
    for (int j = j0; j < j1; ++j) {
        const int v = countdown[j] - 1;
        countdown[j] = v;
        c += v <= 0 ? 1 : 0;
    }
    part[threadIdx.x] = c;
    __syncthreads();
    if (threadIdx.x == 0) {
        int run = 0;
        for (int t = 0; t < 1024; ++t) {
            const int v = part[t];
            part[t] = run;
            run += v;
        }
        n_dead[0] = run;
    }
    __syncthreads();
    int o = part[threadIdx.x];
    for (int j = j0; j < j1; ++j)
        if (countdown[j] <= 0) dead[o++] = j;
}

__global__ __launch_bounds__(256) void km_scatter_rows_kernel(float *__restrict__ codebook, const float *__restrict__ centres,
                                                              const int32_t *__restrict__ dead, int32_t *__restrict__ countdown,
                                                              int rows, int D, int n, int timeout) {
    const int i = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (i >= rows) return;
    const int lane = threadIdx.x & 63;
    const int j = dead[i];
    if (j < 0 || j >= n) return;
    for (int c = lane; c < D; c += 64) codebook[(int64_t)j * D + c] = centres[(int64_t)i * D + c];
    if (lane == 0 && countdown) countdown[j] = timeout;
}

}  // namespace

extern "C" int32_t sgam_kmeans_chunk_points(int32_t N, int32_t D, int32_t k) {
    if (!km_shape_ok(N, D, k)) return -1;
    // the [chunk][k_pad] dot products stay within 256 MiB; whole 128-row GEMM tiles, at least one
    int64_t c = ((int64_t)64 << 20) / km_kpad(k);
    c = c / 128 * 128;
    if (c < 128) c = 128;
    const int64_t n_up = km_up(N, 128);
    return (int32_t)(c < n_up ? c : n_up);
}

extern "C" int64_t sgam_kmeans_assign_workspace_bytes(int32_t N, int32_t D, int32_t k, int32_t chunk) {
    AssignLayout L;
    return km_assign_layout(N, D, k, chunk, &L) ? L.total : -1;
}

extern "C" int sgam_kmeans_assign_f32(const float *x, const float *centres, int32_t *labels, int32_t N, int32_t D, int32_t k,
                                      int32_t chunk, void *workspace, int64_t workspace_bytes, void *stream) {
    if (!x || !centres || !labels) return SGAM_EINVAL;
    AssignLayout L;
    if (!km_assign_layout(N, D, k, chunk, &L)) return SGAM_EINVAL;
    if (!workspace || workspace_bytes < L.total) return SGAM_EWORKSPACE;
    if (!sgam_aligned16(x) || (((uintptr_t)workspace) & (KM_ALIGN - 1)) != 0) return SGAM_EALIGN;
    char *ws = (char *)workspace;
    float *tab = (float *)(ws + L.tab), *c_sq = (float *)(ws + L.c_sq), *dots = (float *)(ws + L.dots);
    void *conv_ws = L.conv_bytes ? (void *)(ws + L.conv) : nullptr;
    const int kpad = km_kpad(k);
    hipStream_t s = sgam_stream(stream);
    SGAM_KLAUNCH(km_pad_centres_kernel, dim3(sgam_cdiv(kpad, 4)), dim3(256), 0, s, centres, tab, c_sq, k, kpad, D);
    SGAM_LAUNCH_CHECK();
    const int rows = chunk < N ? chunk : N;
    for (int64_t p0 = 0; p0 < N; p0 += rows) {
        const int T = (int)(N - p0 < rows ? N - p0 : rows);
        const sgam_conv_desc d = km_dot_desc(T, D, kpad);
        const float *xc = x + p0 * D;
        const int rc = sgam_conv2d_nhwc_f32(&d, xc, tab, nullptr, nullptr, dots, conv_ws, L.conv_bytes, stream);
        if (rc != SGAM_OK) return rc;
        SGAM_KLAUNCH(km_argmin_kernel, dim3(T), dim3(256), 0, s, xc, c_sq, dots, labels + p0, D, kpad);
        SGAM_LAUNCH_CHECK();
    }
    return SGAM_OK;
}

extern "C" int64_t sgam_kmeans_update_workspace_bytes(int32_t N, int32_t k, int32_t block_points) {
    UpdateLayout L;
    return km_update_layout(N, k, block_points > 0 ? block_points : 1024, &L) ? L.total : -1;
}

extern "C" int sgam_kmeans_update_f32(const float *x, const int32_t *labels, float *centres, int32_t *count, int32_t N, int32_t D,
                                      int32_t k, int32_t block_points, void *workspace, int64_t workspace_bytes, void *stream) {
    if (!x || !labels || !centres || !count || D <= 0 || D % 4 != 0) return SGAM_EINVAL;
    UpdateLayout L;
    const int pb = block_points > 0 ? block_points : 1024;
    if (!km_update_layout(N, k, pb, &L)) return SGAM_EINVAL;
    if (!workspace || workspace_bytes < L.total) return SGAM_EWORKSPACE;
    if (!sgam_aligned16(x) || (((uintptr_t)workspace) & (KM_ALIGN - 1)) != 0) return SGAM_EALIGN;
    char *ws = (char *)workspace;
    int32_t *hist = (int32_t *)(ws + L.hist), *start = (int32_t *)(ws + L.start), *order = (int32_t *)(ws + L.order);
    hipStream_t s = sgam_stream(stream);
    const hipError_t e = hipMemsetAsync(hist, 0, (size_t)L.hist_bytes, s);
    if (e != hipSuccess) return (int)e;
    SGAM_KLAUNCH(km_block_hist_kernel, dim3(L.nblk), dim3(256), 0, s, labels, hist, N, k, pb);
    SGAM_LAUNCH_CHECK();
    SGAM_KLAUNCH(km_scan_blocks_kernel, dim3(sgam_cdiv(k, 256)), dim3(256), 0, s, hist, count, L.nblk, k);
    SGAM_LAUNCH_CHECK();
    SGAM_KLAUNCH(km_scan_counts_kernel, dim3(1), dim3(256), 0, s, count, start, k);
    SGAM_LAUNCH_CHECK();
    SGAM_KLAUNCH(km_place_kernel, dim3(L.nblk), dim3(256), 0, s, labels, hist, start, order, N, k, pb);
    SGAM_LAUNCH_CHECK();
    SGAM_KLAUNCH(km_centre_mean_kernel, dim3(k), dim3(256), 0, s, x, order, start, centres, D);
    SGAM_LAUNCH_CHECK();
    return SGAM_OK;
}

extern "C" int sgam_kmeans_init_points_f32(const float *x, float *centres, int32_t *picks, int32_t N, int32_t D, int32_t k,
                                           uint64_t seed, uint64_t refresh, void *stream) {
    if (!x || !centres || N <= 0 || D <= 0 || k <= 0 || k > N) return SGAM_EINVAL;
    int half_bits = 1;
    while (half_bits < 16 && ((int64_t)1 << (2 * half_bits)) < (int64_t)N) ++half_bits;
    SGAM_KLAUNCH(km_init_points_kernel, dim3(sgam_cdiv(k, 4)), dim3(256), 0, sgam_stream(stream), x, centres, picks, N, D, k,
                 half_bits, (uint32_t)(seed & 0xffffffffu), (uint32_t)(seed >> 32), (uint32_t)(refresh & 0xffffffffu),
                 (uint32_t)(refresh >> 32));
    SGAM_LAUNCH_CHECK();
    return SGAM_OK;
}

extern "C" int sgam_codebook_countdown_i32(const int64_t *indices, int32_t T, int32_t *countdown, int32_t n_embed, int32_t timeout,
                                           int32_t *n_dead, int32_t *dead, void *stream) {
    if (!countdown || !n_dead || !dead || n_embed <= 0 || T < 0 || (T > 0 && !indices)) return SGAM_EINVAL;
    SGAM_KLAUNCH(km_countdown_kernel, dim3(1), dim3(1024), 0, sgam_stream(stream), indices, T, countdown, n_embed, timeout, n_dead,
                 dead);
    SGAM_LAUNCH_CHECK();
    return SGAM_OK;
}

extern "C" int sgam_codebook_scatter_rows_f32(float *codebook, const float *centres, const int32_t *dead, int32_t n_rows, int32_t D,
                                              int32_t n_embed, int32_t *countdown, int32_t timeout, void *stream) {
    if (!codebook || !centres || !dead || n_rows <= 0 || D <= 0 || n_embed <= 0 || n_rows > n_embed) return SGAM_EINVAL;
    SGAM_KLAUNCH(km_scatter_rows_kernel, dim3(sgam_cdiv(n_rows, 4)), dim3(256), 0, sgam_stream(stream), codebook, centres, dead,
                 countdown, n_rows, D, n_embed, timeout);
    SGAM_LAUNCH_CHECK();
    return SGAM_OK;
}
