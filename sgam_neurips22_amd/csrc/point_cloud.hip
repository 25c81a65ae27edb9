// point_cloud.hip — clean-up of a scene's merged cloud on top of the k-nearest-neighbour search of point_nn.hip: uniform voxel
// sampling (sgam_points_voxel_sample_f32), the mean neighbour distance and the sums of the statistical outlier rule
// (sgam_points_knn_mean_distance, sgam_points_md_reduce) and normals from the neighbourhood's covariance (sgam_points_normals_f32).
// The arithmetic rules (one IEEE fp32 operation per operator, in the written order) and d2, "not a point" and the reduction's fold
// are points_common.h's; tests/cloud_oracle.py restates the rules in numpy.  A point that is "not a point" belongs to no voxel, has
// no mean distance (NaN) and no normal (NaN).  DESIGN §4.4.5.
//
// Voxel sampling (PCL's UniformSampling rule: every occupied voxel keeps ONE of its points, never a mean).  Per axis, in fp32:
//     v = floorf((p - o) / voxel)              the voxel of p (o: the caller's origin, usually the minimum corner of the cloud)
//     c = o + (v + 0.5f) * voxel               its centre
// d2 = dist2(p, c): dx = p.x - c.x (dy, dz alike), d2 = (dx * dx + dy * dy) + dz * dz.  The kept point of a voxel
// is its member of least (d2 bits, index): an exact tie goes to the lower index.  count = the voxel's number of members.
// The voxel key packs the three v, biased by 2^20 and clamped to 21 bits each (the caller refuses boxes of 2^20 voxels or more along
// an axis), into 63 bits; the table is open addressing with linear probing over T = a power of two >= 2 N slots (hash_table_size and
// mix64 of points_common.h, which mesh_ops.hip's triangle table uses too), keys claimed with
// a 64-bit atomicCAS (empty = all ones: no key has bit 63), per slot a 64-bit atomicMin of (d2 bits << 32) | index and an integer
// atomicAdd of the count.  Which slot a voxel lands in depends on arrival; no output does; there are no float atomics.  The probe
// loop visits at most T slots — it terminates for every input — and a point that found none (impossible with T >= 2 N and an
// intact table) raises the caller's int32 overflow flag instead of waiting.  A second pass writes keep[i] = 1 and count[i] where
// the winner of i's slot is i.  sgam_points_voxel_assign_f32 (vertex clustering of a mesh, mesh_ops.hip / DESIGN §4.4.7) is the same
// table, key and pick and also writes rep[i] = the winner of i's slot (-1 for a point that is not a point).
//
// Mean neighbour distance: md_i = the mean over the valid entries (index >= 0) of row i of a k-NN result of sqrt((double)d2),
// summed in ascending column order in fp64; a row without a valid entry: NaN.  sgam_points_md_reduce: per block of 4096 values
// {sum of md - shift, or of its square, over the finite md; their number} in fp64, a fixed order; the caller folds the blocks.
//
// Normals: the neighbourhood of point i = the valid entries of row i of a k-NN index table (the point itself is among them when the
// table was made without exclude_self).  With e_j = (double)p_j - (double)p_i (the table is read once, every neighbour gathered
// once), in ascending column order in fp64: S = sum e_j, Q = sum e_j e_j^T, m = their number; mean = S / m, covariance
// C = Q / m - mean mean^T.  C is diagonalised by cyclic Jacobi rotations — pairs (0,1), (0,2), (1,2) per sweep, JACOBI_SWEEPS sweeps,
// a fixed number — the normal is the eigenvector of the least eigenvalue (the lowest axis on a tie), normalised in fp64, oriented,
// and rounded to fp32 once.  Orientation: with viewpoints, flipped where n . (viewpoint[view_of[i]] - p_i) < 0; without (or with a
// view_of outside [0, V)), flipped so that its component of largest magnitude (the lowest axis on a tie) is positive.  Fewer than
// 3 valid neighbours: NaN.
#include "jacobi3.h"
#include "points_common.h"

#include <algorithm>
#include <cmath>

namespace {

constexpr int MD_CHUNK = 4096;                // values per workgroup of the reduction (256 lanes x 16)
constexpr uint64_t VOXEL_EMPTY = ~0ull;

// ---------------------------------------------------------------- voxel sampling
struct Voxels {
    float ox, oy, oz, voxel;
};

__device__ __forceinline__ float voxel_of(float p, float o, float voxel) { return floorf(__fdiv_rn(__fsub_rn(p, o), voxel)); }

__device__ __forceinline__ uint64_t voxel_bits(float v) {
    return (uint64_t)(int)fminf(fmaxf(__fadd_rn(v, 1048576.0f), 0.0f), 2097151.0f);       // biased by 2^20, clamped as a float
}

struct VoxelWorkspace {
    unsigned long long *keys, *best;
    int32_t *count, *slot;
};

__global__ __launch_bounds__(256) void voxel_clear_kernel(VoxelWorkspace w, int64_t T) {
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < T; i += (int64_t)gridDim.x * blockDim.x) {
        w.keys[i] = VOXEL_EMPTY;
        w.best[i] = VOXEL_EMPTY;
        w.count[i] = 0;
    }
}

__global__ __launch_bounds__(256) void voxel_insert_kernel(Voxels V, const float *__restrict__ points, int N, VoxelWorkspace w, int64_t T,
                                                           int32_t *__restrict__ overflow) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= N) return;
    const float x = points[i * 3], y = points[i * 3 + 1], z = points[i * 3 + 2];
    int found = -1;
    if (finite3(x, y, z)) {
        const float vx = voxel_of(x, V.ox, V.voxel), vy = voxel_of(y, V.oy, V.voxel), vz = voxel_of(z, V.oz, V.voxel);
        const float cx = __fadd_rn(V.ox, __fmul_rn(__fadd_rn(vx, 0.5f), V.voxel));
        const float cy = __fadd_rn(V.oy, __fmul_rn(__fadd_rn(vy, 0.5f), V.voxel));
        const float cz = __fadd_rn(V.oz, __fmul_rn(__fadd_rn(vz, 0.5f), V.voxel));
        const float d2 = dist2(x, y, z, cx, cy, cz);
        const unsigned long long key = (voxel_bits(vz) << 42) | (voxel_bits(vy) << 21) | voxel_bits(vx);
        int64_t s = (int64_t)(mix64(key) & (uint64_t)(T - 1));
        for (int64_t probe = 0; probe < T; ++probe) {                        // bounded by the table: ends for every input
            const unsigned long long prev = atomicCAS(w.keys + s, VOXEL_EMPTY, key);
            if (prev == VOXEL_EMPTY || prev == key) { found = (int)s; break; }
            s = (s + 1) & (T - 1);
        }
        if (found >= 0) {
            atomicMin(w.best + found, ((unsigned long long)__float_as_uint(d2) << 32) | (uint32_t)i);
            atomicAdd(w.count + found, 1);
        } else {
            atomicOr(overflow, 1);
        }
    }
    w.slot[i] = found;
}

// rep (sgam_points_voxel_assign_f32; else nullptr): the kept point of i's voxel, -1 for a point that is in none
__global__ __launch_bounds__(256) void voxel_pick_kernel(int N, VoxelWorkspace w, uint8_t *__restrict__ keep, int32_t *__restrict__ count_out,
                                                         int32_t *__restrict__ rep) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= N) return;
    const int s = w.slot[i];
    const uint32_t winner = s >= 0 ? (uint32_t)w.best[s] : 0xffffffffu;
    const bool won = s >= 0 && winner == (uint32_t)i;
    keep[i] = won ? 1 : 0;
    count_out[i] = won ? w.count[s] : 0;
    if (rep) rep[i] = s >= 0 ? (int32_t)winner : -1;
}

// ---------------------------------------------------------------- statistical outliers
__global__ __launch_bounds__(256) void knn_mean_distance_kernel(const float *__restrict__ d2, const int32_t *__restrict__ index, int N, int k,
                                                                double *__restrict__ md) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= N) return;
    double s = 0.0;
    int m = 0;
    for (int c = 0; c < k; ++c) {
        if (index[i * k + c] >= 0) { s += sqrt((double)d2[i * k + c]); ++m; }
    }
    md[i] = m ? s / (double)m : __longlong_as_double(0x7ff8000000000000ll);
}

// one workgroup per MD_CHUNK values: partial[blk] = {sum over the finite md of (md - shift) or its square, their number}
__global__ __launch_bounds__(256) void md_reduce_kernel(const double *__restrict__ md, int64_t n, double shift, int squared,
                                                        double *__restrict__ partial) {
    const int64_t base = (int64_t)blockIdx.x * MD_CHUNK;
    double s[2] = {0.0, 0.0};
#pragma unroll 4
    for (int c = 0; c < MD_CHUNK / 256; ++c) {
        const int64_t i = base + c * 256 + threadIdx.x;
        if (i >= n) break;
        const double v = md[i];
        if (finite_f64(v)) {
            const double e = v - shift;
            s[0] += squared ? e * e : e;
            s[1] += 1.0;
        }
    }
    block_sum_f64(s, partial);
}

// ---------------------------------------------------------------- normals
// one lane per point
__global__ __launch_bounds__(256) void normals_kernel(const float *__restrict__ points, int N, const int32_t *__restrict__ knn_index, int k,
                                                      const float *__restrict__ viewpoints, int V, const int32_t *__restrict__ view_of,
                                                      float *__restrict__ normals) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= N) return;
    const double px = (double)points[i * 3], py = (double)points[i * 3 + 1], pz = (double)points[i * 3 + 2];
    double sx = 0.0, sy = 0.0, sz = 0.0, qxx = 0.0, qxy = 0.0, qxz = 0.0, qyy = 0.0, qyz = 0.0, qzz = 0.0;
    int m = 0;
    for (int c = 0; c < k; ++c) {
        const int j = knn_index[i * k + c];
        if (j < 0 || j >= N) continue;
        const double ex = (double)points[(int64_t)j * 3] - px, ey = (double)points[(int64_t)j * 3 + 1] - py,
                     ez = (double)points[(int64_t)j * 3 + 2] - pz;
        sx += ex; sy += ey; sz += ez;
        qxx += ex * ex; qxy += ex * ey; qxz += ex * ez; qyy += ey * ey; qyz += ey * ez; qzz += ez * ez;
        ++m;
    }
    const float nanf_ = __uint_as_float(0x7fc00000u);
    float nx = nanf_, ny = nanf_, nz = nanf_;
    if (m >= 3) {
        const double im = 1.0 / (double)m;
        const double mx = sx * im, my = sy * im, mz = sz * im;
        double a00 = qxx * im - mx * mx, a01 = qxy * im - mx * my, a02 = qxz * im - mx * mz, a11 = qyy * im - my * my,
               a12 = qyz * im - my * mz, a22 = qzz * im - mz * mz;
        double v00 = 1.0, v01 = 0.0, v02 = 0.0, v10 = 0.0, v11 = 1.0, v12 = 0.0, v20 = 0.0, v21 = 0.0, v22 = 1.0;
        for (int sweep = 0; sweep < JACOBI_SWEEPS; ++sweep) {                 // a fixed count: no convergence test
            jacobi_rotate(a00, a11, a01, a02, a12, v00, v01, v10, v11, v20, v21);         // (p, q, r) = (0, 1, 2)
            jacobi_rotate(a00, a22, a02, a01, a12, v00, v02, v10, v12, v20, v22);         // (0, 2, 1)
            jacobi_rotate(a11, a22, a12, a01, a02, v01, v02, v11, v12, v21, v22);         // (1, 2, 0)
        }
        const bool s1 = a11 < a00;                                            // the least eigenvalue, the lowest axis on a tie
        const bool s2 = a22 < (s1 ? a11 : a00);                               // (selects of values: nothing indexed, no private memory)
        double ex = s2 ? v02 : (s1 ? v01 : v00), ey = s2 ? v12 : (s1 ? v11 : v10), ez = s2 ? v22 : (s1 ? v21 : v20);
        const double inv = 1.0 / sqrt((ex * ex + ey * ey) + ez * ez);
        ex *= inv; ey *= inv; ez *= inv;
        bool flip;
        const int view = view_of ? view_of[i] : -1;
        if (viewpoints && view >= 0 && view < V) {
            const double dx = (double)viewpoints[view * 3] - px, dy = (double)viewpoints[view * 3 + 1] - py,
                         dz = (double)viewpoints[view * 3 + 2] - pz;
            flip = (ex * dx + ey * dy) + ez * dz < 0.0;
        } else {
            double big = ex;
            if (fabs(ey) > fabs(big)) big = ey;
            if (fabs(ez) > fabs(big)) big = ez;
            flip = big < 0.0;
        }
        if (flip) { ex = -ex; ey = -ey; ez = -ez; }
        nx = (float)ex; ny = (float)ey; nz = (float)ez;
    }
    normals[i * 3] = nx; normals[i * 3 + 1] = ny; normals[i * 3 + 2] = nz;
}

}  // namespace

extern "C" int64_t sgam_points_voxel_workspace_bytes(int32_t N) {
    if (N < 1 || N > (1 << 29)) return SGAM_EINVAL;                           // (a slot number stays an int32)
    const int64_t T = hash_table_size(N);
    return 8 * T + 8 * T + 4 * T + r16(4 * (int64_t)N);
}

// the table, the insertion and the pick of both voxel entry points; rep_out: sgam_points_voxel_assign_f32's extra output, or nullptr
static int voxel_sample_launch(const float *points, int32_t N, float ox, float oy, float oz, float voxel_size, void *workspace,
                               int64_t workspace_bytes, uint8_t *keep_out, int32_t *count_out, int32_t *rep_out, int32_t *overflow_flag,
                               void *stream) {
    if (!points || !keep_out || !count_out || !overflow_flag || N < 1 ||
        !(std::fabs(ox) <= F32_MAX && std::fabs(oy) <= F32_MAX && std::fabs(oz) <= F32_MAX) || !(voxel_size > 0.f && voxel_size <= F32_MAX))
        return SGAM_EINVAL;
    if (!workspace_fits(workspace, workspace_bytes, sgam_points_voxel_workspace_bytes(N))) return SGAM_EINVAL;
    const int64_t T = hash_table_size(N);
    char *p = (char *)workspace;
    VoxelWorkspace w;
    w.keys = (unsigned long long *)p;       p += 8 * T;
    w.best = (unsigned long long *)p;       p += 8 * T;
    w.count = (int32_t *)p;                 p += 4 * T;
    w.slot = (int32_t *)p;
    Voxels V{ox, oy, oz, voxel_size};
    hipStream_t s = sgam_stream(stream);
    const unsigned pblocks = blocks_of(N);
    SGAM_KLAUNCH(voxel_clear_kernel, dim3((unsigned)std::min<int64_t>(T / 256, 1 << 16)), dim3(256), 0, s, w, T);
    SGAM_KLAUNCH(voxel_insert_kernel, dim3(pblocks), dim3(256), 0, s, V, points, N, w, T, overflow_flag);
    SGAM_KLAUNCH(voxel_pick_kernel, dim3(pblocks), dim3(256), 0, s, N, w, keep_out, count_out, rep_out);
    SGAM_LAUNCH_CHECK();
    return SGAM_OK;
}

extern "C" int sgam_points_voxel_sample_f32(const float *points, int32_t N, float ox, float oy, float oz, float voxel_size, void *workspace,
                                            int64_t workspace_bytes, uint8_t *keep_out, int32_t *count_out, int32_t *overflow_flag,
                                            void *stream) {
    return voxel_sample_launch(points, N, ox, oy, oz, voxel_size, workspace, workspace_bytes, keep_out, count_out, nullptr, overflow_flag, stream);
}

extern "C" int sgam_points_voxel_assign_f32(const float *points, int32_t N, float ox, float oy, float oz, float voxel_size, void *workspace,
                                            int64_t workspace_bytes, uint8_t *keep_out, int32_t *count_out, int32_t *rep_out,
                                            int32_t *overflow_flag, void *stream) {
    if (!rep_out) return SGAM_EINVAL;
    return voxel_sample_launch(points, N, ox, oy, oz, voxel_size, workspace, workspace_bytes, keep_out, count_out, rep_out, overflow_flag, stream);
}

extern "C" int sgam_points_knn_mean_distance(const float *d2, const int32_t *index, int32_t N, int32_t k, double *md_out, void *stream) {
    if (!d2 || !index || !md_out || N < 1 || k < 1 || k > KNN_MAX_K) return SGAM_EINVAL;
    SGAM_KLAUNCH(knn_mean_distance_kernel, dim3(blocks_of(N)), dim3(256), 0, sgam_stream(stream), d2, index, N, k, md_out);
    SGAM_LAUNCH_CHECK();
    return SGAM_OK;
}

extern "C" int64_t sgam_points_md_reduce_partials(int64_t n) {
    if (n < 1) return SGAM_EINVAL;
    return 2 * ((n + MD_CHUNK - 1) / MD_CHUNK);
}

extern "C" int sgam_points_md_reduce(const double *md, int64_t n, double shift, int32_t squared, double *partials, void *stream) {
    if (!md || !partials || n < 1 || (n + MD_CHUNK - 1) / MD_CHUNK > 0x7fffffffll || !finite_f64(shift) ||
        (squared != 0 && squared != 1))
        return SGAM_EINVAL;
    SGAM_KLAUNCH(md_reduce_kernel, dim3((unsigned)((n + MD_CHUNK - 1) / MD_CHUNK)), dim3(256), 0, sgam_stream(stream), md, n, shift, squared,
                 partials);
    SGAM_LAUNCH_CHECK();
    return SGAM_OK;
}

extern "C" int sgam_points_normals_f32(const float *points, int32_t N, const int32_t *knn_index, int32_t k, const float *viewpoints, int32_t V,
                                       const int32_t *view_of, float *normals_out, void *stream) {
    if (!points || !knn_index || !normals_out || N < 1 || k < 1 || k > KNN_MAX_K || (viewpoints != nullptr) != (view_of != nullptr) ||
        (viewpoints && V < 1) || (!viewpoints && V != 0))
        return SGAM_EINVAL;
    SGAM_KLAUNCH(normals_kernel, dim3(blocks_of(N)), dim3(256), 0, sgam_stream(stream), points, N, knn_index, k, viewpoints,
                 V, view_of, normals_out);
    SGAM_LAUNCH_CHECK();
    return SGAM_OK;
}
