// points_common.h — what the point-cloud units (point_raster.hip, point_nn.hip, point_cloud.hip) share: ONE definition of each piece
// of exact arithmetic their numpy twins (tests/points_oracle.py, geometry_oracle.py, cloud_oracle.py) restate, so that a fix reaches
// every caller.  The arithmetic rules, stated once for the three units:
//   - every fp32 operator is ONE IEEE operation in the written order, nothing fused: the units are built with -ffp-contract=off
//     and the operations are spelled out (__fadd_rn, __fmul_rn, ...); the outputs are compared with the twins bit for bit;
//   - a point with a coordinate that is not finite is "not a point" (finite3); a double that is not finite: finite_f64;
//   - distance of a point p and a query q:  dx = p.x - q.x (dy, dz alike);  d2 = (dx * dx + dy * dy) + dz * dz   (dist2);
//   - unprojection of pixel (row i, column j) with depth d, then a 3 x 4 transform T (row-major):
//         a = (Kinv[0] * j + Kinv[1] * i) + Kinv[2]          b: Kinv[3..5], c: Kinv[6..8]      (j, i converted to float)  (pixel_ray)
//         x = a * d    y = b * d    z = c * d
//         X = ((T[0] * x + T[1] * y) + T[2] * z) + T[3]      Y: T[4..7]    Z: T[8..11]                                    (transform34)
//   - fp64 sums over a chunk of values: per lane in index order, then the DPP wave sum of sgam_common.h, then the four waves of the
//     workgroup folded as ((w0 + w1) + w2) + w3: a fixed order (block_sum_f64).
// And the host-side rules every geometry unit (the three above, point_icp.hip, mesh_ops.hip, mesh_query.hip) states the same way:
// the launch size of one lane per item (blocks_of), whether a caller's workspace fits (workspace_fits), the size and the hash of
// the open-addressing tables (hash_table_size, mix64), and the one kernel that fills an int32 array (fill_kernel).
#pragma once
#include "sgam_common.h"

constexpr float F32_MAX = 3.4028234663852886e38f;
constexpr int KNN_MAX_K = 32;                 // slots of the largest k-NN list the kernels are compiled for

static inline int64_t r16(int64_t n) { return (n + 15) & ~(int64_t)15; }

// workgroups of 256 lanes that give n items one lane each
static inline unsigned blocks_of(int64_t n) { return (unsigned)((n + 255) / 256); }

// a caller's workspace holds the `need` bytes its *_workspace_bytes entry computed (negative: that entry refused the sizes)
static inline bool workspace_fits(const void *workspace, int64_t bytes, int64_t need) {
    return need >= 0 && workspace && bytes >= need && sgam_aligned16(workspace);
}

// the open-addressing tables (voxels: point_cloud.hip; clustered triangles: mesh_ops.hip): T = the power of two >= max(256, 2 n)
// slots, probed linearly from mix64(key) & (T - 1)
static inline int64_t hash_table_size(int64_t n) {
    int64_t T = 256;
    while (T < 2 * n) T <<= 1;
    return T;
}

__device__ __forceinline__ uint64_t mix64(uint64_t x) {                                   // (the finaliser of MurmurHash3)
    x ^= x >> 33; x *= 0xff51afd7ed558ccdull;
    x ^= x >> 33; x *= 0xc4ceb9fe1a85ec53ull;
    return x ^ (x >> 33);
}

namespace {
// v[0..n) = value, by any number of workgroups (a template, so that a unit that fills nothing carries no copy of the kernel)
template <typename T>
__global__ __launch_bounds__(256) void fill_kernel(T *__restrict__ v, int64_t n, T value) {
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) v[i] = value;
}
}  // namespace

__device__ __forceinline__ bool finite3(float x, float y, float z) {
    return fabsf(x) <= F32_MAX && fabsf(y) <= F32_MAX && fabsf(z) <= F32_MAX;            // (NaN fails)
}

// a finite double, on the device and in the host-side argument checks alike (NaN fails)
__host__ __device__ __forceinline__ bool finite_f64(double v) { return __builtin_fabs(v) <= 1.7976931348623157e308; }

__device__ __forceinline__ float dist2(float px, float py, float pz, float qx, float qy, float qz) {
    const float dx = __fsub_rn(px, qx), dy = __fsub_rn(py, qy), dz = __fsub_rn(pz, qz);
    return __fadd_rn(__fadd_rn(__fmul_rn(dx, dx), __fmul_rn(dy, dy)), __fmul_rn(dz, dz));
}

// the ray of pixel (row i, column j): the point at depth d is (a * d, b * d, c * d)
__device__ __forceinline__ void pixel_ray(const float (&kinv)[9], int i, int j, float &a, float &b, float &c) {
    const float fj = (float)j, fi = (float)i;
    a = __fadd_rn(__fadd_rn(__fmul_rn(kinv[0], fj), __fmul_rn(kinv[1], fi)), kinv[2]);
    b = __fadd_rn(__fadd_rn(__fmul_rn(kinv[3], fj), __fmul_rn(kinv[4], fi)), kinv[5]);
    c = __fadd_rn(__fadd_rn(__fmul_rn(kinv[6], fj), __fmul_rn(kinv[7], fi)), kinv[8]);
}

__device__ __forceinline__ void transform34(const float *__restrict__ T, float x, float y, float z, float &X, float &Y, float &Z) {
    X = __fadd_rn(__fadd_rn(__fadd_rn(__fmul_rn(T[0], x), __fmul_rn(T[1], y)), __fmul_rn(T[2], z)), T[3]);
    Y = __fadd_rn(__fadd_rn(__fadd_rn(__fmul_rn(T[4], x), __fmul_rn(T[5], y)), __fmul_rn(T[6], z)), T[7]);
    Z = __fadd_rn(__fadd_rn(__fadd_rn(__fmul_rn(T[8], x), __fmul_rn(T[9], y)), __fmul_rn(T[10], z)), T[11]);
}

// the tail of a chunk reduction by a workgroup of 256 lanes: partial[blockIdx.x * C + c] = the workgroup's sum of s[c]
template <int C>
__device__ __forceinline__ void block_sum_f64(const double (&s)[C], double *__restrict__ partial) {
    __shared__ double lds[4][C];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
#pragma unroll
    for (int c = 0; c < C; ++c) {
        const double t = sgam_wave_sum_f64(s[c]);
        if (lane == 0) lds[w][c] = t;
    }
    __syncthreads();
    if (threadIdx.x < C) partial[(int64_t)blockIdx.x * C + threadIdx.x] =
        ((lds[0][threadIdx.x] + lds[1][threadIdx.x]) + lds[2][threadIdx.x]) + lds[3][threadIdx.x];
}
