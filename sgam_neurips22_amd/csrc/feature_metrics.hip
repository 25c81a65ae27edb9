// feature_metrics.hip — the set metrics on Inception features next to FID (sgam_neurips22_amd/feature_metrics.py): the fp64 Gram
// G = Z Z^T of the stacked feature rows, KID's subset choice and polynomial-kernel MMD^2 sums, and the k-th-neighbour radii and
// membership counts of improved precision / recall and density / coverage.  gfx950 only.
//
// Conventions of inception.hip: the caller owns every buffer, launches go on the passed stream without a sync or an allocation,
// no float atomics (every result is run-to-run identical; the four PRDC counts are integer atomics).  Built with
// -ffp-contract=off: every fused multiply-add below is an explicit one (the MFMA's).
#include "sgam_common.h"

namespace {

typedef double f64x4 __attribute__((ext_vector_type(4)));

// ---- Gram.  Workgroup = one 64 x 64 tile of G with bi <= bj, four wavefronts of 32 x 32 (2 x 2 blocks of v_mfma_f64_16x16x4_f64:
// lane l holds A[row l & 15][k = l >> 4] and B[k = l >> 4][col l & 15], one f64 each; C/D col = l & 15, row = (l >> 4) + 4 reg).
// Both operands are rows of z: A[i][k] = z[i0 + i][k], B[k][j] = z[j0 + j][k], staged as fp32 in LDS, 32 columns of K per stage
// (the next stage's global loads are in registers while this one multiplies), converted to fp64 on the way to the registers.
// K order: k = 0, 4, 8, ... in steps of one MFMA, for every tile alike; no split-K.  An entry with i <= j is stored at (i, j) and
// at (j, i); entries of a diagonal tile with i > j are not stored at all: G == G^T bit for bit by construction.  Products of two
// fp32 values are exact in fp64 and commute, and the chain over k is the same for every entry, so an entry depends on the values
// of its two rows only.  Rows >= n are zeros in LDS (never read from memory) and never stored.
constexpr int GT = 64, GK = 32, GLD = GK + 4;        // row pitch 36 floats: (row * 36 + k) mod 64 distinct over 16 rows x 4 k

template <bool VEC>
__device__ __forceinline__ f32x4 gram_load(const float *__restrict__ z, int n, int d, int64_t ldz, int row, int k) {
    f32x4 v = {0.0f, 0.0f, 0.0f, 0.0f};
    if (row < n && k < d) {                           // d % 4 == 0: the four columns k .. k + 3 are inside the row together
        const float *p = z + (int64_t)row * ldz + k;
        if constexpr (VEC) {
            v = *reinterpret_cast<const f32x4 *>(p);
        } else {
            v[0] = p[0], v[1] = p[1], v[2] = p[2], v[3] = p[3];
        }
    }
    return v;
}

template <bool VEC>
__global__ __launch_bounds__(256) void feature_gram_kernel(const float *__restrict__ z, int n, int d, int64_t ldz, double *__restrict__ G) {
    const int bi = blockIdx.y, bj = blockIdx.x;
    if (bi > bj) return;
    __shared__ __attribute__((aligned(16))) float As[GT][GLD], Bs[GT][GLD];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wm = wave >> 1, wn = wave & 1;
    // staging: thread -> rows tid / 8 and tid / 8 + 32, columns (tid % 8) * 4 .. + 3 of both tiles
    const int sr = tid >> 3, sc = (tid & 7) * 4;
    f32x4 ra[2], rb[2];
#pragma unroll
    for (int h = 0; h < 2; ++h) {
        ra[h] = gram_load<VEC>(z, n, d, ldz, bi * GT + sr + 32 * h, sc);
        rb[h] = gram_load<VEC>(z, n, d, ldz, bj * GT + sr + 32 * h, sc);
    }
    f64x4 acc[2][2];
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
        for (int b = 0; b < 2; ++b) acc[a][b] = f64x4{0.0, 0.0, 0.0, 0.0};
    const int fr = lane & 15, fk = lane >> 4;
    for (int k0 = 0; k0 < d; k0 += GK) {
        __syncthreads();                              // the previous stage has been read
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            *reinterpret_cast<f32x4 *>(&As[sr + 32 * h][sc]) = ra[h];
            *reinterpret_cast<f32x4 *>(&Bs[sr + 32 * h][sc]) = rb[h];
        }
        __syncthreads();
        if (k0 + GK < d) {
#pragma unroll
            for (int h = 0; h < 2; ++h) {
                ra[h] = gram_load<VEC>(z, n, d, ldz, bi * GT + sr + 32 * h, k0 + GK + sc);
                rb[h] = gram_load<VEC>(z, n, d, ldz, bj * GT + sr + 32 * h, k0 + GK + sc);
            }
        }
        const int steps = min(GK, d - k0) >> 2;
        for (int s = 0; s < steps; ++s) {
            double a[2], b[2];
#pragma unroll
            for (int e = 0; e < 2; ++e) {
                a[e] = (double)As[wm * 32 + e * 16 + fr][s * 4 + fk];
                b[e] = (double)Bs[wn * 32 + e * 16 + fr][s * 4 + fk];
            }
#pragma unroll
            for (int ea = 0; ea < 2; ++ea)
#pragma unroll
                for (int eb = 0; eb < 2; ++eb) acc[ea][eb] = __builtin_amdgcn_mfma_f64_16x16x4f64(a[ea], b[eb], acc[ea][eb], 0, 0, 0);
        }
    }
#pragma unroll
    for (int ea = 0; ea < 2; ++ea)
#pragma unroll
        for (int eb = 0; eb < 2; ++eb)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int gi = bi * GT + wm * 32 + ea * 16 + fk + 4 * r;
                const int gj = bj * GT + wn * 32 + eb * 16 + fr;
                if (gi < n && gj < n && gi <= gj) {
                    const double v = acc[ea][eb][r];
                    G[(int64_t)gi * n + gj] = v;
                    if (gi != gj) G[(int64_t)gj * n + gi] = v;
                }
            }
}

// ---- KID subsets.  key(i) = word 0 of Philox4x32-10 at counter (i, s, side, 0) under key (seed_lo, seed_hi); subset s of a side
// with N rows = the m indices with the smallest pairs (key, i), ascending.  Rank by counting: a thread owns one i and walks all
// j in tiles of 256 keys (one Philox call per thread and tile), counting the pairs below its own; flag[i] = rank < m.
__device__ __forceinline__ uint32_t kid_key(uint32_t i, uint32_t s, uint32_t side, uint32_t k0, uint32_t k1) {
    uint32_t c[4] = {i, s, side, 0u};
    sgam_philox4x32_10(c, k0, k1);
    return c[0];
}

__global__ __launch_bounds__(256) void kid_rank_kernel(int n1, int n2, int nmax, int m, uint32_t k0, uint32_t k1, uint8_t *__restrict__ flag) {
    __shared__ uint32_t keys[256];
    const int side = blockIdx.y, s = blockIdx.z;
    const int N = side == 0 ? n1 : n2;
    if (blockIdx.x * 256 >= N) return;                // (uniform over the workgroup)
    const int i = blockIdx.x * 256 + threadIdx.x;
    const uint32_t mine = kid_key((uint32_t)i, (uint32_t)s, (uint32_t)side, k0, k1);
    int rank = 0;
    for (int j0 = 0; j0 < N; j0 += 256) {
        __syncthreads();
        keys[threadIdx.x] = kid_key((uint32_t)(j0 + threadIdx.x), (uint32_t)s, (uint32_t)side, k0, k1);
        __syncthreads();
        const int cnt = min(256, N - j0);
        for (int t = 0; t < cnt; ++t) {
            const uint32_t kj = keys[t];
            rank += (kj < mine || (kj == mine && j0 + t < i)) ? 1 : 0;
        }
    }
    if (i < N) flag[((int64_t)s * 2 + side) * nmax + i] = rank < m ? 1 : 0;
}

// one workgroup per (side, subset): the flagged indices in ascending order (a block-wide prefix count per 256 indices)
__global__ __launch_bounds__(256) void kid_compact_kernel(int n1, int n2, int nmax, int m, const uint8_t *__restrict__ flag,
                                                          int32_t *__restrict__ idx) {
    __shared__ int wave_total[4];
    const int side = blockIdx.x, s = blockIdx.y;
    const int N = side == 0 ? n1 : n2;
    const uint8_t *f = flag + ((int64_t)s * 2 + side) * nmax;
    int32_t *out = idx + ((int64_t)s * 2 + side) * m;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    int base = 0;
    for (int i0 = 0; i0 < N; i0 += 256) {
        const int i = i0 + threadIdx.x;
        const bool on = i < N && f[i] != 0;
        const unsigned long long b = __ballot(on);
        const int before = __popcll(b & ((1ull << lane) - 1ull));
        __syncthreads();
        if (lane == 0) wave_total[wave] = __popcll(b);
        __syncthreads();
        int off = base;
        for (int w = 0; w < wave; ++w) off += wave_total[w];
        if (on && off + before < m) out[off + before] = i;
        base += wave_total[0] + wave_total[1] + wave_total[2] + wave_total[3];
    }
}

// ---- KID values.  K(i, j) = t t t with t = gamma G_ij + c0 (a product, a sum, two products, each rounded once).  A wavefront
// owns row r of subset s: three sums over the subset's columns, lane l taking columns l, l + 64, ... in order, joined by the fixed
// wave sum; partial[(s m + r) 3 + {0: a-a without j == r, 1: b-b without j == r, 2: a-b}].
__device__ __forceinline__ double kid_kernel_value(double g, double gamma, double c0) {
    const double t = gamma * g + c0;
    return (t * t) * t;
}

__global__ __launch_bounds__(256) void kid_rows_kernel(const double *__restrict__ G, int n, int n1, const int32_t *__restrict__ idx, int m,
                                                       double gamma, double c0, double *__restrict__ partial) {
    const int lane = threadIdx.x & 63, r = blockIdx.x * 4 + (threadIdx.x >> 6), s = blockIdx.y;
    if (r >= m) return;                               // (uniform over the wavefront)
    const int32_t *ia = idx + (int64_t)s * 2 * m, *ib = ia + m;
    const double *ga = G + (int64_t)ia[r] * n, *gb = G + (int64_t)(n1 + ib[r]) * n;
    double saa = 0.0, sbb = 0.0, sab = 0.0;
    for (int j = lane; j < m; j += 64) {
        const int ca = ia[j], cb = n1 + ib[j];
        if (j != r) {
            saa += kid_kernel_value(ga[ca], gamma, c0);
            sbb += kid_kernel_value(gb[cb], gamma, c0);
        }
        sab += kid_kernel_value(ga[cb], gamma, c0);
    }
    saa = sgam_wave_sum_f64(saa);
    sbb = sgam_wave_sum_f64(sbb);
    sab = sgam_wave_sum_f64(sab);
    if (lane == 0) {
        double *p = partial + ((int64_t)s * m + r) * 3;
        p[0] = saa, p[1] = sbb, p[2] = sab;
    }
}

// the rows joined in row order (one thread per sum), then mmd^2 = aa / (m (m - 1)) + bb / (m (m - 1)) - 2 ab / m^2
__global__ __launch_bounds__(64) void kid_join_kernel(const double *__restrict__ partial, int m, double *__restrict__ out) {
    __shared__ double sums[3];
    const int s = blockIdx.x;
    if (threadIdx.x < 3) {
        const double *p = partial + (int64_t)s * m * 3 + threadIdx.x;
        double t = 0.0;
        for (int r = 0; r < m; ++r) t += p[(int64_t)r * 3];
        sums[threadIdx.x] = t;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        const double mm = (double)m, off = mm * (mm - 1.0);
        out[s] = (sums[0] / off + sums[1] / off) - (2.0 * sums[2]) / (mm * mm);
    }
}

// ---- precision / recall / density / coverage.  Rows 0 .. nr - 1 of G are the reference set, nr .. nr + nf - 1 the scene's.
// d2(i, j) = (G_ii + G_jj) - 2 G_ij, in that order (the sum of the two diagonal entries commutes, so d2(i, j) == d2(j, i) in bits).
__device__ __forceinline__ double prdc_d2(double gii, double gjj, double gij) { return (gii + gjj) - 2.0 * gij; }

// smaller of two (value, index) pairs over the wavefront, returned to every lane
__device__ __forceinline__ void prdc_wave_min(double &v, int &ix) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const double ov = __shfl_xor(v, o, 64);
        const int oi = __shfl_xor(ix, o, 64);
        if (ov < v || (ov == v && oi < ix)) v = ov, ix = oi;
    }
}

// radius2[i] = the k-th smallest d2(i, j) over the rows j != i of i's own set (exclusion by index: a duplicate row is a neighbour
// at distance 0).  One wavefront per row; k passes, pass t taking the smallest pair (d2, j) above the pair of pass t - 1.
__global__ __launch_bounds__(256) void prdc_radius_kernel(const double *__restrict__ G, int nr, int nf, int k, double *__restrict__ radius2,
                                                          unsigned long long *__restrict__ counts) {
    const int n = nr + nf, lane = threadIdx.x & 63, i = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (blockIdx.x == 0 && threadIdx.x < 4) counts[threadIdx.x] = 0ull;
    if (i >= n) return;                               // (uniform over the wavefront)
    const int lo = i < nr ? 0 : nr, hi = i < nr ? nr : n;
    const double *row = G + (int64_t)i * n;
    const double gii = row[i];
    double pv = -__builtin_inf();
    int pi = -1;
    for (int t = 0; t < k; ++t) {
        double bv = __builtin_inf();
        int bx = 0x7fffffff;
        for (int j = lo + lane; j < hi; j += 64) {
            if (j == i) continue;
            const double v = prdc_d2(gii, G[(int64_t)j * n + j], row[j]);
            const bool above = v > pv || (v == pv && j > pi);
            if (above && (v < bv || (v == bv && j < bx))) bv = v, bx = j;
        }
        prdc_wave_min(bv, bx);
        pv = bv, pi = bx;
    }
    if (lane == 0) radius2[i] = pv;
}

// counts[0] precision: scene rows j inside the ball of some reference row (d2(i, j) <= radius2[i]); [1] recall: reference rows i
// inside the ball of some scene row (d2(i, j) <= radius2[j]); [2] density: pairs (i, j) with d2(i, j) <= radius2[i]; [3] coverage:
// reference rows i whose nearest scene row is inside their own ball.  One wavefront per row of G, integer atomics only.
__global__ __launch_bounds__(256) void prdc_count_kernel(const double *__restrict__ G, int nr, int nf, const double *__restrict__ radius2,
                                                         unsigned long long *__restrict__ counts) {
    const int n = nr + nf, lane = threadIdx.x & 63, q = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (q >= n) return;                               // (uniform over the wavefront)
    const double *row = G + (int64_t)q * n;
    const double gqq = row[q];
    if (q >= nr) {                                    // a scene row against every reference ball
        int inside = 0;
        for (int i = lane; i < nr; i += 64) inside += prdc_d2(G[(int64_t)i * n + i], gqq, row[i]) <= radius2[i] ? 1 : 0;
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) inside += __shfl_xor(inside, o, 64);
        if (lane == 0 && inside > 0) {
            atomicAdd(&counts[0], 1ull);
            atomicAdd(&counts[2], (unsigned long long)inside);
        }
    } else {                                          // a reference row against every scene row
        const double rq = radius2[q];
        int in_other = 0, ix = 0;
        double nearest = __builtin_inf();
        for (int j = nr + lane; j < n; j += 64) {
            const double v = prdc_d2(gqq, G[(int64_t)j * n + j], row[j]);
            in_other |= v <= radius2[j] ? 1 : 0;
            nearest = v < nearest ? v : nearest;
        }
        prdc_wave_min(nearest, ix);
        const bool any = __ballot(in_other != 0) != 0ull;
        if (lane == 0) {
            if (any) atomicAdd(&counts[1], 1ull);
            if (nearest <= rq) atomicAdd(&counts[3], 1ull);
        }
    }
}

}  // namespace

#define SGAM_FEATURE_ROWS_MAX 16384

extern "C" int sgam_feature_gram_f64(const float *z, int32_t n, int32_t d, int32_t ldz, double *G, void *stream) {
    if (!z || !G || n <= 0 || n > SGAM_FEATURE_ROWS_MAX || d <= 0 || (d & 3) != 0 || ldz < d) return SGAM_EINVAL;
    const int t = sgam_cdiv(n, GT);
    const bool vec = sgam_aligned16(z) && (ldz & 3) == 0;
    if (sgam_i_prof_on) sgam_i_prof_work(2.0 * d * ((double)n * (n + 1) / 2.0), 4.0 * n * d + 8.0 * n * n);
    if (vec) {
        SGAM_KLAUNCH(feature_gram_kernel<true>, dim3(t, t), dim3(256), 0, sgam_stream(stream), z, n, d, (int64_t)ldz, G);
    } else {
        SGAM_KLAUNCH(feature_gram_kernel<false>, dim3(t, t), dim3(256), 0, sgam_stream(stream), z, n, d, (int64_t)ldz, G);
    }
    SGAM_LAUNCH_CHECK();
    return SGAM_OK;
}

extern "C" int sgam_kid_subsets_u32(int32_t n1, int32_t n2, int32_t m, int32_t subsets, uint64_t seed, void *workspace,
                                    int64_t workspace_bytes, int32_t *idx, void *stream) {
    if (!idx || n1 <= 0 || n2 <= 0 || n1 > SGAM_FEATURE_ROWS_MAX || n2 > SGAM_FEATURE_ROWS_MAX || m <= 0 || m > n1 || m > n2 ||
        subsets <= 0 || subsets > 65535)
        return SGAM_EINVAL;
    const int nmax = n1 > n2 ? n1 : n2;
    if (!workspace || workspace_bytes < 2 * (int64_t)subsets * nmax) return SGAM_EWORKSPACE;
    hipStream_t s = sgam_stream(stream);
    uint8_t *flag = (uint8_t *)workspace;
    SGAM_KLAUNCH(kid_rank_kernel, dim3(sgam_cdiv(nmax, 256), 2, subsets), dim3(256), 0, s, n1, n2, nmax, m, (uint32_t)seed,
                 (uint32_t)(seed >> 32), flag);
    SGAM_LAUNCH_CHECK();
    SGAM_KLAUNCH(kid_compact_kernel, dim3(2, subsets), dim3(256), 0, s, n1, n2, nmax, m, (const uint8_t *)flag, idx);
    SGAM_LAUNCH_CHECK();
    return SGAM_OK;
}

extern "C" int sgam_kid_mmd_f64(const double *G, int32_t n1, int32_t n2, const int32_t *idx, int32_t m, int32_t subsets, double gamma,
                                double coef0, void *workspace, int64_t workspace_bytes, double *out, void *stream) {
    if (!G || !idx || !out || n1 <= 0 || n2 <= 0 || (int64_t)n1 + n2 > SGAM_FEATURE_ROWS_MAX || m < 2 || m > n1 || m > n2 ||
        subsets <= 0 || subsets > 65535)
        return SGAM_EINVAL;
    if (!workspace || workspace_bytes < 24 * (int64_t)subsets * m) return SGAM_EWORKSPACE;
    if ((((uintptr_t)workspace) & 7u) != 0) return SGAM_EALIGN;
    hipStream_t s = sgam_stream(stream);
    double *partial = (double *)workspace;
    SGAM_KLAUNCH(kid_rows_kernel, dim3(sgam_cdiv(m, 4), subsets), dim3(256), 0, s, G, n1 + n2, n1, idx, m, gamma, coef0, partial);
    SGAM_LAUNCH_CHECK();
    SGAM_KLAUNCH(kid_join_kernel, dim3(subsets), dim3(64), 0, s, (const double *)partial, m, out);
    SGAM_LAUNCH_CHECK();
    return SGAM_OK;
}

extern "C" int sgam_feature_prdc_f64(const double *G, int32_t nr, int32_t nf, int32_t k, double *radius2, int64_t *counts, void *stream) {
    if (!G || !radius2 || !counts || nr <= 0 || nf <= 0 || (int64_t)nr + nf > SGAM_FEATURE_ROWS_MAX || k < 1 || k > 32 || k + 1 > nr ||
        k + 1 > nf)
        return SGAM_EINVAL;
    hipStream_t s = sgam_stream(stream);
    const int n = nr + nf;
    unsigned long long *c = (unsigned long long *)counts;
    SGAM_KLAUNCH(prdc_radius_kernel, dim3(sgam_cdiv(n, 4)), dim3(256), 0, s, G, nr, nf, k, radius2, c);
    SGAM_LAUNCH_CHECK();
    SGAM_KLAUNCH(prdc_count_kernel, dim3(sgam_cdiv(n, 4)), dim3(256), 0, s, G, nr, nf, (const double *)radius2, c);
    SGAM_LAUNCH_CHECK();
    return SGAM_OK;
}
