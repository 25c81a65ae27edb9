// point_nn.hip — geometry metrics of a scene's point cloud: the frame store unprojected into ONE cloud
// (sgam_points_unproject_f32), exact nearest neighbours between two clouds — brute force through LDS tiles
// (sgam_points_nn_brute_f32) and a uniform grid searched in growing shells (sgam_points_grid_build, sgam_points_nn_grid_f32) — and
// the fp64 sums the metrics are made of (sgam_points_nn_reduce).  A sibling of point_raster.hip: the same device address tables, the
// same unprojection.  points_common.h states the arithmetic rules (one IEEE fp32 operation per operator, in the written order) and
// holds the shared pieces: the unprojection, d2, "not a point", the reduction's fold.  tests/geometry_oracle.py restates all of it
// in numpy and the outputs are compared bit for bit.
//
// Unprojection, frame f, pixel q = i * Ws + j, d = depth_f[i][j]: points_common.h's with T = T_c2w[f] (camera -> world, 3 x 4), and
//     unless d is finite and z_near <= d && d <= z_far:  X = Y = Z = NaN          (the colour is copied either way)
//
// The neighbour of a query q is the reference point p of least (d2 bits, index) among those with d2 <= max_d2 (max_d2 = +inf: all) — so an exact tie
// goes to the lower index; a d2 that is NaN or +inf is never chosen; no candidate: index -1, d2 +inf.
//
// Brute force: one lane per query, the reference set staged through LDS in tiles of 1024 points (12 KB) that every lane of the
// workgroup walks in index order (all lanes read the same LDS address: a broadcast); `d2 < best` keeps the first of equal distances.
//
// Grid: cells of edge h over the box of the valid reference points, cell (cx, cy, cz) = clamp(floorf((p - origin) / h), 0, g - 1)
// per axis in fp32.  Build = count (integer atomics) -> exclusive scan over the cells -> scatter of (x, y, z, id) records into
// cell-sorted order (the order inside a cell depends on arrival; the (d2, index) winner does not).  Query: one lane per query;
// shell r = the cells at Chebyshev distance r from the query's (clamped) cell; after shell r the visited block is
// [c - r, c + r] per axis, cut to the grid.  A point not yet visited lies, on some axis, in a cell beyond a face of that block
// which is NOT a grid border (beyond a border there are no cells: points outside the box were clamped INTO the border cells, which
// only moves them towards the block, so their true distance is even larger).  Its distance to q is therefore at least the distance
// from q to that face, up to the fp32 rounding of its cell assignment.  With m = the least SIGNED distance from q to those faces
// (face position origin + k * h in fp32; negative when rounding put q beyond a face: no stop), the search ends after shell r when
//     ms = (m - margin) * (1 - 2^-18) > 0   and   (best < ms * ms   or   ms * ms > max_d2),
// margin = 2^-16 * (largest |coordinate| of the grid's corners + its longest edge): 2^6 times the worst sum of the rounding of
// (p - origin) / h, of origin + k * h and of the subtraction from q, each at most 2^-22 of that scale; the factor 1 - 2^-18
// covers the relative rounding of the face distance itself (far-away queries), of the square and of an fp32 d2 (below 2^-20).  The
// comparison is strict, so an unvisited point can neither win nor tie.  The shell loop also ends when the block covers the grid,
// after at most max(gx, gy, gz) shells: it terminates for every input.  DESIGN §4.4.4 has the derivation.
//
// k nearest neighbours (sgam_points_knn_brute_f32, sgam_points_knn_grid_f32; 1 <= k <= 32): the same d2, the same candidates, row i
// of the output = the k least (d2 bits, index) pairs of query i in ascending order, the tail of a row with fewer candidates
// index -1 / d2 +inf; with exclude_self the candidate whose index equals the query's is skipped (query and ref are one cloud).
// A pair is ONE 64-bit key (d2 bits << 32) | index — d2 is a sum of squares, never negative, so its bits order like its value —
// and the empty key (+inf bits, index 0xffffffff) sorts after every candidate.  Each lane keeps its sorted list of k keys in LDS,
// laid out [slot][lane] (8 B per slot: consecutive lanes read consecutive 8-byte words, no bank conflict; a dynamically indexed
// register array would live in scratch); the kernels are compiled for lists of 8, 16 and 32 slots (16 / 32 / 64 KB per 256-lane
// workgroup).  A candidate not below the lane's k-th key (kept in a register) is rejected with one compare, anything else is
// inserted by shifting the larger keys up.  The grid kernel is the shell search above with `best` = the d2 of the k-th key, +inf
// until k candidates are held: an unvisited point is strictly farther than the k-th held one, so the proof carries over; the
// shell loop keeps its bound.  k = 1 gives the nearest-neighbour kernels' bits.
//
// The shell search is written ONCE (grid_search, in grid_common.h with the grid descriptor, the cell rule, the scan, the tables in
// the caller's workspace and the six launches that build them; mesh_query.hip runs the same build and the same walk over cells of
// triangles) over a sink that takes the candidates: NearestSink (best, bi; in point_cells.h with the cells' records, which
// point_segment.hip's fixed-radius walks share) or KnnSink (the
// lane's list); offer(d2, id, max_d2) applies the rules above, bound() is the `best` the stop rule reads.  The brute-force tile walk
// stays two kernels: written over the same sinks it was measured 12 - 36 % slower for the nearest neighbour (whose loop is one
// compare per pair; the sink's index tie-break is a second) and 5 % slower at k <= 16.
#include "point_cells.h"

namespace {

constexpr int BRUTE_TILE = 1024;              // reference points per LDS tile (12 KB)
constexpr int REDUCE_CHUNK = 4096;            // d2 values per workgroup of the reduction (256 lanes x 16)
constexpr uint64_t KNN_EMPTY = 0x7f800000ffffffffull;                         // d2 +inf, index -1: after every candidate

// ---------------------------------------------------------------- unprojection
struct Unproject {
    float kinv[9];
    float zn, zf;
    int Hs, Ws;
};

// grid (blocks over a frame's pixels, frames (strided)): one lane per (frame, pixel)
__global__ __launch_bounds__(256) void points_unproject_kernel(Unproject U, const float *const *__restrict__ depth_ptrs,
                                                               const uint8_t *const *__restrict__ rgb_ptrs, int F,
                                                               const float *__restrict__ T_c2w, float *__restrict__ points,
                                                               uint8_t *__restrict__ colors) {
    const int64_t hw = (int64_t)U.Hs * U.Ws;
    const int64_t q = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (q >= hw) return;
    const int i = (int)(q / U.Ws), j = (int)(q - (int64_t)i * U.Ws);
    float a, b, c;
    pixel_ray(U.kinv, i, j, a, b, c);
    const float nan = __uint_as_float(0x7fc00000u);
    for (int f = blockIdx.y; f < F; f += gridDim.y) {                         // (block-uniform)
        const float d = depth_ptrs[f][q];
        const float *__restrict__ T = T_c2w + (int64_t)f * 12;                 // wave-uniform
        float X, Y, Z;
        transform34(T, __fmul_rn(a, d), __fmul_rn(b, d), __fmul_rn(c, d), X, Y, Z);
        if (!(fabsf(d) <= F32_MAX && U.zn <= d && d <= U.zf)) X = Y = Z = nan;
        const int64_t o = ((int64_t)f * hw + q) * 3;
        points[o] = X; points[o + 1] = Y; points[o + 2] = Z;
        if (colors) {
            const uint8_t *__restrict__ s = rgb_ptrs[f] + q * 3;
            colors[o] = s[0]; colors[o + 1] = s[1]; colors[o + 2] = s[2];
        }
    }
}

// ---------------------------------------------------------------- candidates: the k-NN list and its sink (NearestSink: point_cells.h)
__device__ __forceinline__ uint64_t knn_key(float d2, int id) { return ((uint64_t)__float_as_uint(d2) << 32) | (uint32_t)id; }

// the lane's sorted list: list[s * 256 + lane], s < k; kth = list[(k - 1) * 256 + lane] mirrored in a register
__device__ __forceinline__ void knn_offer(uint64_t *__restrict__ list, int k, uint64_t &kth, float d2, int id, float max_d2) {
    if (!(d2 <= max_d2) || !(d2 <= F32_MAX)) return;                          // (NaN fails; +inf never enters)
    const uint64_t key = knn_key(d2, id);
    if (key >= kth) return;
    int j = k - 1;
    while (j > 0) {
        const uint64_t below = list[(j - 1) * 256];
        if (below <= key) break;
        list[j * 256] = below;
        --j;
    }
    list[j * 256] = key;
    kth = list[(k - 1) * 256];
}

struct KnnSink {
    uint64_t *list;                                                           // the lane's column of the workgroup's LDS lists
    int k, self;                                                              // self: the index never offered (-1: none)
    uint64_t kth = KNN_EMPTY;
    __device__ __forceinline__ KnnSink(uint64_t *list_, int k_, int self_) : list(list_), k(k_), self(self_) {
        for (int s = 0; s < k; ++s) list[s * 256] = KNN_EMPTY;
    }
    __device__ __forceinline__ void offer(float d2, int id, float max_d2) {
        if (id != self) knn_offer(list, k, kth, d2, id, max_d2);
    }
    __device__ __forceinline__ float bound() const { return __uint_as_float((uint32_t)(kth >> 32)); }        // (+inf until k are held)
};

__device__ __forceinline__ void knn_write(const uint64_t *__restrict__ list, int k, int64_t i, float *__restrict__ d2_out,
                                          int32_t *__restrict__ index_out) {
    for (int s = 0; s < k; ++s) {
        const uint64_t key = list[s * 256];
        d2_out[i * k + s] = __uint_as_float((uint32_t)(key >> 32));
        index_out[i * k + s] = (int32_t)(uint32_t)key;
    }
}

// ---------------------------------------------------------------- brute force
// grid (blocks over the queries, B): one lane per query; the reference tile is walked by all lanes together
__global__ __launch_bounds__(256) void points_nn_brute_kernel(const float *__restrict__ query, const float *__restrict__ ref, int Nq,
                                                              int Nr, float max_d2, float *__restrict__ d2_out,
                                                              int32_t *__restrict__ index_out) {
    __shared__ float tile[BRUTE_TILE * 3];
    const int64_t b = blockIdx.y;
    query += b * Nq * 3;
    ref += b * Nr * 3;
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const bool live = i < Nq;
    float qx = 0.f, qy = 0.f, qz = 0.f;
    if (live) { qx = query[i * 3]; qy = query[i * 3 + 1]; qz = query[i * 3 + 2]; }
    float best = __uint_as_float(0x7f800000u);
    int bi = -1;
    for (int t0 = 0; t0 < Nr; t0 += BRUTE_TILE) {                             // (block-uniform)
        const int n = min(BRUTE_TILE, Nr - t0);
        __syncthreads();
        for (int k = threadIdx.x; k < n * 3; k += blockDim.x) tile[k] = ref[(int64_t)t0 * 3 + k];
        __syncthreads();
        for (int k = 0; k < n; ++k) {
            const float d2 = dist2(tile[k * 3], tile[k * 3 + 1], tile[k * 3 + 2], qx, qy, qz);
            if (d2 <= max_d2 && d2 < best) { best = d2; bi = t0 + k; }         // index order: the first of equal distances stays
        }
    }
    if (live) { d2_out[b * Nq + i] = best; index_out[b * Nq + i] = bi; }
}

// grid (blocks over the queries): one lane per query, the reference tiles of the brute-force kernel
template <int KB>
__global__ __launch_bounds__(256) void points_knn_brute_kernel(const float *__restrict__ query, const float *__restrict__ ref, int Nq, int Nr,
                                                               int k, float max_d2, int exclude_self, float *__restrict__ d2_out,
                                                               int32_t *__restrict__ index_out) {
    __shared__ float tile[BRUTE_TILE * 3];
    __shared__ uint64_t lists[KB * 256];
    uint64_t *list = lists + threadIdx.x;
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const bool live = i < Nq;
    const float nan = __uint_as_float(0x7fc00000u);
    float qx = nan, qy = nan, qz = nan;                                       // (a lane without a query offers nothing)
    if (live) { qx = query[i * 3]; qy = query[i * 3 + 1]; qz = query[i * 3 + 2]; }
    for (int s = 0; s < k; ++s) list[s * 256] = KNN_EMPTY;
    uint64_t kth = KNN_EMPTY;
    const int self = exclude_self && live ? (int)i : -1;
    for (int t0 = 0; t0 < Nr; t0 += BRUTE_TILE) {                             // (block-uniform)
        const int n = min(BRUTE_TILE, Nr - t0);
        __syncthreads();
        for (int c = threadIdx.x; c < n * 3; c += blockDim.x) tile[c] = ref[(int64_t)t0 * 3 + c];
        __syncthreads();
        for (int c = 0; c < n; ++c) {
            const float d2 = dist2(tile[c * 3], tile[c * 3 + 1], tile[c * 3 + 2], qx, qy, qz);
            if (t0 + c != self) knn_offer(list, k, kth, d2, t0 + c, max_d2);
        }
    }
    if (live) knn_write(list, k, i, d2_out, index_out);
}

// ---------------------------------------------------------------- uniform grid
__global__ __launch_bounds__(256) void points_grid_count_kernel(Grid G, const float *__restrict__ ref, int Nr, int32_t *__restrict__ count) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= Nr) return;
    const float x = ref[i * 3], y = ref[i * 3 + 1], z = ref[i * 3 + 2];
    if (!finite3(x, y, z)) return;
    atomicAdd(count + cell_index(G, x, y, z), 1);
}

__global__ __launch_bounds__(256) void points_grid_scatter_kernel(Grid G, const float *__restrict__ ref, int Nr, int32_t *__restrict__ cursor,
                                                                  float4 *__restrict__ sorted) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= Nr) return;
    const float x = ref[i * 3], y = ref[i * 3 + 1], z = ref[i * 3 + 2];
    if (!finite3(x, y, z)) return;
    const int pos = atomicAdd(cursor + cell_index(G, x, y, z), 1);           // inside [start[c], start[c + 1]): counted by the same rule
    sorted[pos] = make_float4(x, y, z, __int_as_float((int)i));
}

// one lane per query
__global__ __launch_bounds__(256) void points_nn_grid_kernel(Grid G, const float *__restrict__ query, int Nq, const float4 *__restrict__ sorted,
                                                             const int32_t *__restrict__ start, float max_d2, float *__restrict__ d2_out,
                                                             int32_t *__restrict__ index_out) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= Nq) return;
    const float qx = query[i * 3], qy = query[i * 3 + 1], qz = query[i * 3 + 2];
    NearestSink sink;
    if (finite3(qx, qy, qz)) grid_search(G, PointCells{sorted}, start, qx, qy, qz, max_d2, sink);
    d2_out[i] = sink.best;
    index_out[i] = sink.bi;
}

// one lane per query
template <int KB>
__global__ __launch_bounds__(256) void points_knn_grid_kernel(Grid G, const float *__restrict__ query, int Nq, const float4 *__restrict__ sorted,
                                                              const int32_t *__restrict__ start, int k, float max_d2, int exclude_self,
                                                              float *__restrict__ d2_out, int32_t *__restrict__ index_out) {
    __shared__ uint64_t lists[KB * 256];
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= Nq) return;                                                      // (no barrier below)
    const float qx = query[i * 3], qy = query[i * 3 + 1], qz = query[i * 3 + 2];
    KnnSink sink(lists + threadIdx.x, k, exclude_self ? (int)i : -1);
    if (finite3(qx, qy, qz)) grid_search(G, PointCells{sorted}, start, qx, qy, qz, max_d2, sink);
    knn_write(sink.list, k, i, d2_out, index_out);
}

// ---------------------------------------------------------------- reduction
// one workgroup per REDUCE_CHUNK values: partial[blk] = {sum d2, sum sqrt(d2), count finite, count d2 <= tau^2} in fp64, fixed order
__global__ __launch_bounds__(256) void points_nn_reduce_kernel(const float *__restrict__ d2, int64_t n, double tau2, double *__restrict__ partial) {
    const int64_t base = (int64_t)blockIdx.x * REDUCE_CHUNK;
    double s[4] = {0.0, 0.0, 0.0, 0.0};
#pragma unroll 4
    for (int k = 0; k < REDUCE_CHUNK / 256; ++k) {
        const int64_t i = base + k * 256 + threadIdx.x;
        if (i >= n) break;
        const float v = d2[i];
        if (fabsf(v) <= F32_MAX) {
            const double dv = (double)v;
            s[0] += dv;
            s[1] += sqrt(dv);
            s[2] += 1.0;
            if (dv <= tau2) s[3] += 1.0;
        }
    }
    block_sum_f64(s, partial);
}

// what the two grid queries ask of their arguments; G and w are what the build derived from the same numbers
bool grid_query_setup(const float *query, int Nq, int Nr, float ox, float oy, float oz, float h, int gx, int gy, int gz, const void *workspace,
                      int64_t workspace_bytes, float max_d2, const float *d2_out, const int32_t *index_out, Grid &G, GridTables &w) {
    return query && d2_out && index_out && Nq >= 1 && Nr >= 1 && max_d2 >= 0.f && make_grid(ox, oy, oz, h, gx, gy, gz, G) &&
           grid_tables(workspace, workspace_bytes, Nr, POINT_RECORD, gx, gy, gz, w);
}

bool knn_args_ok(int Nq, int Nr, int k, int exclude_self) {
    return k >= 1 && k <= KNN_MAX_K && (exclude_self == 0 || exclude_self == 1) && !(exclude_self && Nq != Nr);
}

// a k-NN kernel is compiled for lists of 8, 16 and 32 slots: the launch of the smallest that holds k, one lane per query
#define KNN_LAUNCH(kern, k, Nq, stream, ...)                                                              \
    do {                                                                                                  \
        const dim3 grid_(blocks_of(Nq));                                                                  \
        hipStream_t s_ = sgam_stream(stream);                                                             \
        if ((k) <= 8) SGAM_KLAUNCH(kern<8>, grid_, dim3(256), 0, s_, __VA_ARGS__);                        \
        else if ((k) <= 16) SGAM_KLAUNCH(kern<16>, grid_, dim3(256), 0, s_, __VA_ARGS__);                 \
        else SGAM_KLAUNCH(kern<32>, grid_, dim3(256), 0, s_, __VA_ARGS__);                                \
    } while (0)

}  // namespace

extern "C" int sgam_points_unproject_f32(const void *depth_ptrs, const void *rgb_ptrs, int32_t F, int32_t Hs, int32_t Ws, const float *Kinv,
                                         const float *T_c2w, float z_near, float z_far, float *points_out, uint8_t *colors_out,
                                         void *stream) {
    if (!depth_ptrs || !Kinv || !T_c2w || !points_out || F < 1 || Hs <= 0 || Ws <= 0 || (int64_t)F * Hs * Ws >= (1ll << 31) ||
        (colors_out != nullptr) != (rgb_ptrs != nullptr) || !(z_near <= z_far))
        return SGAM_EINVAL;
    Unproject U;
    for (int i = 0; i < 9; ++i) U.kinv[i] = Kinv[i];
    U.zn = z_near; U.zf = z_far; U.Hs = Hs; U.Ws = Ws;
    const int64_t hw = (int64_t)Hs * Ws;
    SGAM_KLAUNCH(points_unproject_kernel, dim3(blocks_of(hw), (unsigned)std::min(F, 65535)), dim3(256), 0,
                 sgam_stream(stream), U, (const float *const *)depth_ptrs, (const uint8_t *const *)rgb_ptrs, F, T_c2w, points_out, colors_out);
    SGAM_LAUNCH_CHECK();
    return SGAM_OK;
}

extern "C" int sgam_points_nn_brute_f32(const float *query, const float *ref, int32_t B, int32_t Nq, int32_t Nr, float max_d2,
                                        float *d2_out, int32_t *index_out, void *stream) {
    if (!query || !ref || !d2_out || !index_out || B < 1 || B > 65535 || Nq < 1 || Nr < 1 || !(max_d2 >= 0.f)) return SGAM_EINVAL;
    SGAM_KLAUNCH(points_nn_brute_kernel, dim3(blocks_of(Nq), B), dim3(256), 0, sgam_stream(stream), query, ref, Nq, Nr,
                 max_d2, d2_out, index_out);
    SGAM_LAUNCH_CHECK();
    return SGAM_OK;
}

extern "C" int64_t sgam_points_grid_workspace_bytes(int32_t Nr, int32_t gx, int32_t gy, int32_t gz) {
    return grid_tables_bytes(Nr, POINT_RECORD, gx, gy, gz);
}

extern "C" int sgam_points_grid_build(const float *ref, int32_t Nr, float ox, float oy, float oz, float cell_size, int32_t gx, int32_t gy,
                                      int32_t gz, void *workspace, int64_t workspace_bytes, void *stream) {
    Grid G;
    GridTables w;
    if (!ref || Nr < 1 || !make_grid(ox, oy, oz, cell_size, gx, gy, gz, G) ||
        !grid_tables(workspace, workspace_bytes, Nr, POINT_RECORD, gx, gy, gz, w))
        return SGAM_EINVAL;
    hipStream_t s = sgam_stream(stream);
    grid_build(
        w, s, [&] { SGAM_KLAUNCH(points_grid_count_kernel, dim3(blocks_of(Nr)), dim3(256), 0, s, G, ref, Nr, w.cursor); },
        [&] { SGAM_KLAUNCH(points_grid_scatter_kernel, dim3(blocks_of(Nr)), dim3(256), 0, s, G, ref, Nr, w.cursor, w.records); });
    SGAM_LAUNCH_CHECK();
    return SGAM_OK;
}

extern "C" int sgam_points_nn_grid_f32(const float *query, int32_t Nq, int32_t Nr, float ox, float oy, float oz, float cell_size, int32_t gx,
                                       int32_t gy, int32_t gz, const void *workspace, int64_t workspace_bytes, float max_d2, float *d2_out,
                                       int32_t *index_out, void *stream) {
    Grid G;
    GridTables w;
    if (!grid_query_setup(query, Nq, Nr, ox, oy, oz, cell_size, gx, gy, gz, workspace, workspace_bytes, max_d2, d2_out, index_out, G, w))
        return SGAM_EINVAL;
    SGAM_KLAUNCH(points_nn_grid_kernel, dim3(blocks_of(Nq)), dim3(256), 0, sgam_stream(stream), G, query, Nq, w.records, w.start, max_d2, d2_out,
                 index_out);
    SGAM_LAUNCH_CHECK();
    return SGAM_OK;
}

extern "C" int sgam_points_knn_brute_f32(const float *query, const float *ref, int32_t Nq, int32_t Nr, int32_t k, float max_d2,
                                         int32_t exclude_self, float *d2_out, int32_t *index_out, void *stream) {
    if (!query || !ref || !d2_out || !index_out || Nq < 1 || Nr < 1 || !(max_d2 >= 0.f) || !knn_args_ok(Nq, Nr, k, exclude_self))
        return SGAM_EINVAL;
    KNN_LAUNCH(points_knn_brute_kernel, k, Nq, stream, query, ref, Nq, Nr, k, max_d2, exclude_self, d2_out, index_out);
    SGAM_LAUNCH_CHECK();
    return SGAM_OK;
}

extern "C" int sgam_points_knn_grid_f32(const float *query, int32_t Nq, int32_t Nr, float ox, float oy, float oz, float cell_size, int32_t gx,
                                        int32_t gy, int32_t gz, const void *workspace, int64_t workspace_bytes, int32_t k, float max_d2,
                                        int32_t exclude_self, float *d2_out, int32_t *index_out, void *stream) {
    Grid G;
    GridTables w;
    if (!knn_args_ok(Nq, Nr, k, exclude_self) ||
        !grid_query_setup(query, Nq, Nr, ox, oy, oz, cell_size, gx, gy, gz, workspace, workspace_bytes, max_d2, d2_out, index_out, G, w))
        return SGAM_EINVAL;
    KNN_LAUNCH(points_knn_grid_kernel, k, Nq, stream, G, query, Nq, w.records, w.start, k, max_d2, exclude_self, d2_out, index_out);
    SGAM_LAUNCH_CHECK();
    return SGAM_OK;
}

extern "C" int64_t sgam_points_nn_reduce_partials(int64_t n) {
    if (n < 1) return SGAM_EINVAL;
    return 4 * ((n + REDUCE_CHUNK - 1) / REDUCE_CHUNK);
}

extern "C" int sgam_points_nn_reduce(const float *d2, int64_t n, float tau, double *partials, void *stream) {
    if (!d2 || !partials || n < 1 || (n + REDUCE_CHUNK - 1) / REDUCE_CHUNK > 0x7fffffffll || !(tau >= 0.f)) return SGAM_EINVAL;
    SGAM_KLAUNCH(points_nn_reduce_kernel, dim3((unsigned)((n + REDUCE_CHUNK - 1) / REDUCE_CHUNK)), dim3(256), 0, sgam_stream(stream), d2, n,
                 (double)tau * (double)tau, partials);
    SGAM_LAUNCH_CHECK();
    return SGAM_OK;
}
