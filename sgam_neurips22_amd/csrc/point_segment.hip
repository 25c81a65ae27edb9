// point_segment.hip — what is IN a scene's cloud: the points within a radius of each point (sgam_points_radius_count_*), DBSCAN
// clusters (sgam_points_dbscan_*), the dominant planes by RANSAC with a least-squares refit (sgam_points_segment_planes_f32, its
// hot kernel alone: sgam_points_plane_score_f32) and the box of every cluster (sgam_points_cluster_boxes_f32).  The unit composes
// what its siblings have: the uniform grid and its shell walk (grid_common.h, point_cells.h), the least-index union-find
// (union_find.h), Philox draws in point_global.hip's style, the 3 x 3 Jacobi rotation (jacobi3.h) and the fixed-order fp64 block
// sums (points_common.h), whose arithmetic rules it follows: one IEEE fp32 operation per operator in the written order, "not a
// point" = !finite3, integer atomics only, every loop bounded by a size, a loop that reaches its bound ORs 1 into the caller's flag
// word and returns, no lane ever waits for another.  tests/segmentation_oracle.py restates every rule in numpy; the outputs are
// compared bit for bit (the refit: to one fp32 ulp).  DESIGN §4.4.14.
//
// Fixed radius.  j is a neighbour of i iff both are points and dist2(p_j, p_i) <= max_d2 (j == i included).  count[i] = the number
// of neighbours, 0 for a non-point.  ONE walk (radius_walk_kernel) offers every candidate of a point to a sink, by brute force —
// the LDS tiles of points_nn_brute_kernel, non-points staged as NaN — or through the grid: grid_search with a sink whose bound()
// is +inf, so the stop rule of point_nn.hip ends the walk when its lower bound exceeds max_d2 or the block covers the grid; its
// proof carries over unchanged (an unvisited point is strictly farther than max_d2).  A neighbour either way is decided by the
// same fp32 d2 against the same max_d2: brute force, the grid and every cell size give the same bits.
//
// DBSCAN.  core: count >= min_points.  A cluster is a connected component of the core points under the neighbour relation; its
// root is its least core index — the union-find's fixed point whatever the interleaving — and clusters are numbered 0, 1, ... in
// ascending root order.  A border point (not core, a core neighbour) joins the cluster of the core neighbour of least
// (d2 bits, index); everything else, non-points included, is noise: label -1.  Launches: count -> parent[i] = i -> link (the sink
// of core point i unites i with every core neighbour j < i: each core-core edge is seen once, from its higher end) -> flatten
// (root of every core point, a launch of its own: parent is read-only there) -> border (the walk with a NearestSink that is
// offered core candidates only; root = the winner's) -> root flags -> the three scan kernels of grid_common.h -> labels = rank of
// the root, sizes by integer atomicAdd, n_clusters a device int32.
//
// Planes.  Round r = 0 .. max_planes - 1 of a fixed launch sequence without a host read; active = a point no plane has taken.
//   list     the ascending list of the active points: flag -> scan -> ordered scatter (no atomics: index order); n_active on the device
//   draw     one lane per hypothesis h: three distinct positions of the list, candidate = mulhi(w0, n_active) with w0 = word 0 of
//            Philox4x32-10 at counter (h, draw, r, 0) under key seed, a repeated candidate drawn again, at most PLANE_MAX_DRAWS
//            draws in all.  In fp64: n = (p1 - p0) x (p2 - p0), |n|^2 = (nx nx + ny ny) + nz nz, n scaled by 1 / sqrt(|n|^2),
//            d = -((nx p0x + ny p0y) + nz p0z); stored as four fp32.  Invalid (plane NaN): a failed pick, n_active < 3, |n|^2 zero
//            or not finite.
//   score    inlier iff fabsf(((a x + b y) + c z) + d) <= threshold (plane_inlier, the inlier pass's too).  Lane <-> hypothesis, R
//            hypotheses per lane in registers; the points stream through LDS as float4 tiles, inactive points and non-points
//            staged as NaN, so the inner loop has no other test and every lane reads the same 16 bytes (a broadcast).  int32
//            counts in registers, one integer atomicAdd per hypothesis and point chunk: no cross-lane reduction, exact whatever
//            the arrival order.  Grid = hypothesis tiles x point chunks, the chunk chosen for >= 2 workgroups per CU.
//   select   one workgroup: the greatest count, a tie to the lowest h; below max(min_inliers, 3) or nothing valid: the round's
//            planes are NaN, its count 0, nothing is assigned, and the later rounds run harmlessly.
//   inliers  active points within the threshold of the winner: labels[i] = r.
//   refit    the least-squares plane through those inliers: centroid, then centred second moments, as fp64 block partials
//            (block_sum_f64 over chunks of 4096 points) folded in block order by one workgroup; the moments' Jacobi sweeps; the
//            normal = the eigenvector of the least eigenvalue (lowest axis on a tie) normalised in fp64, flipped so that its dot
//            product with the RANSAC normal is >= 0; d = -n . centroid; stored as fp32.
//
// Boxes: per label the point count and the axis-aligned box by integer atomicMin / atomicMax on order-preserving keys of the fp32
// coordinates (min and max do not depend on order; no centroid: an atomic fp sum would not be reproducible).
#include "jacobi3.h"
#include "point_cells.h"
#include "union_find.h"

namespace {

constexpr int WALK_TILE = 1024;               // points per LDS tile of the brute-force walk (12 KB)
constexpr int SCORE_TILE = 1024;              // points per LDS tile of the plane score (float4: 16 KB)
constexpr int SCORE_MIN_WORKGROUPS = 512;     // two workgroups for each of the MI355X's 256 CUs
constexpr int PLANE_MAX_DRAWS = 16;           // Philox draws a hypothesis may use for its three distinct picks
constexpr int FIT_CHUNK = 4096;               // points per workgroup of the refit's sums (256 lanes x 16)
constexpr int FLAG_BOUND = 1;                 // a loop ran into its bound

// ---------------------------------------------------------------- the fixed-radius walk and its sinks
struct CountSink {
    int n = 0;
    __device__ __forceinline__ void offer(float d2, int, float max_d2) { n += d2 <= max_d2 ? 1 : 0; }
    __device__ __forceinline__ float bound() const { return __uint_as_float(0x7f800000u); }
};

// core point i unites with every core neighbour below it
struct LinkSink {
    int32_t *parent;
    const int32_t *__restrict__ count;
    int i, N, min_points;
    bool ok = true;
    __device__ __forceinline__ void offer(float d2, int id, float max_d2) {
        if (d2 <= max_d2 && id < i && count[id] >= min_points) ok = uf_unite(parent, i, id, N) && ok;
    }
    __device__ __forceinline__ float bound() const { return __uint_as_float(0x7f800000u); }
};

// the nearest core neighbour, by (d2 bits, index)
struct BorderSink {
    const int32_t *__restrict__ count;
    int min_points;
    NearestSink nearest;
    __device__ __forceinline__ void offer(float d2, int id, float max_d2) {
        if (d2 <= max_d2 && count[id] >= min_points) nearest.offer(d2, id, max_d2);
    }
    __device__ __forceinline__ float bound() const { return __uint_as_float(0x7f800000u); }
};

// every candidate of the point (qx, qy, qz) of a lane is offered to its sink: through the grid (sorted != nullptr), or from LDS
// tiles that the whole workgroup walks in index order (block-uniform: every lane of the workgroup comes here, `walks` or not)
template <class Sink>
__device__ __forceinline__ void radius_walk(const Grid &G, const float4 *__restrict__ sorted, const int32_t *__restrict__ start,
                                            const float *__restrict__ points, int N, bool walks, float qx, float qy, float qz, float max_d2,
                                            Sink &sink, float *tile) {
    if (sorted) {
        if (walks) grid_search(G, PointCells{sorted}, start, qx, qy, qz, max_d2, sink);
        return;
    }
    const float nan = __uint_as_float(0x7fc00000u);
    for (int t0 = 0; t0 < N; t0 += WALK_TILE) {                               // (block-uniform)
        const int n = min(WALK_TILE, N - t0);
        __syncthreads();
        for (int k = threadIdx.x; k < n; k += blockDim.x) {
            const float x = points[(int64_t)(t0 + k) * 3], y = points[(int64_t)(t0 + k) * 3 + 1], z = points[(int64_t)(t0 + k) * 3 + 2];
            const bool p = finite3(x, y, z);
            tile[k * 3] = p ? x : nan; tile[k * 3 + 1] = p ? y : nan; tile[k * 3 + 2] = p ? z : nan;
        }
        __syncthreads();
        if (walks)
            for (int k = 0; k < n; ++k) sink.offer(dist2(tile[k * 3], tile[k * 3 + 1], tile[k * 3 + 2], qx, qy, qz), t0 + k, max_d2);
    }
}

struct Walk {
    Grid G;
    const float4 *sorted;                     // nullptr: brute force
    const int32_t *start;
    const float *points;
    int N;
    float max_d2;
};

// MODE 0: count_out[i] = neighbours.  1: link.  2: root[i] of a border point (or -1); core points keep theirs.
template <int MODE>
__global__ __launch_bounds__(256) void radius_walk_kernel(Walk W, int min_points, int32_t *count, int32_t *parent, int32_t *root,
                                                          int32_t *__restrict__ flag) {
    __shared__ float tile[WALK_TILE * 3];
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const bool live = i < W.N;
    const float nan = __uint_as_float(0x7fc00000u);
    float qx = nan, qy = nan, qz = nan;
    if (live) { qx = W.points[i * 3]; qy = W.points[i * 3 + 1]; qz = W.points[i * 3 + 2]; }
    const bool point = live && finite3(qx, qy, qz);
    if (MODE == 0) {
        CountSink sink;
        radius_walk(W.G, W.sorted, W.start, W.points, W.N, point, qx, qy, qz, W.max_d2, sink, tile);
        if (live) count[i] = sink.n;
    } else if (MODE == 1) {
        const bool core = point && count[i] >= min_points;
        LinkSink sink{parent, count, (int)i, W.N, min_points};
        radius_walk(W.G, W.sorted, W.start, W.points, W.N, core, qx, qy, qz, W.max_d2, sink, tile);
        if (!sink.ok) atomicOr(flag, FLAG_BOUND);
    } else {
        const bool border = point && count[i] < min_points;
        BorderSink sink{count, min_points};
        radius_walk(W.G, W.sorted, W.start, W.points, W.N, border, qx, qy, qz, W.max_d2, sink, tile);
        if (live && !(point && count[i] >= min_points)) root[i] = sink.nearest.bi >= 0 ? root[sink.nearest.bi] : -1;   // (a core's: not written here)
    }
}

__global__ __launch_bounds__(256) void iota_kernel(int32_t *__restrict__ v, int N) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < N) v[i] = (int32_t)i;
}

// (a launch of its own: parent is read-only here, every chain ends at the cluster's least core index) root[i] of a core point, else -1
__global__ __launch_bounds__(256) void dbscan_flatten_kernel(const int32_t *__restrict__ parent, const int32_t *__restrict__ count, int N,
                                                             int min_points, int32_t *__restrict__ root, uint8_t *__restrict__ core_out,
                                                             int32_t *__restrict__ flag) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= N) return;
    const bool core = count[i] >= min_points;
    core_out[i] = core ? 1 : 0;
    if (!core) { root[i] = -1; return; }
    int32_t x = (int32_t)i;
    int step = 0;
    for (; step <= N; ++step) {
        const int32_t p = parent[x];
        if (p == x || (uint32_t)p >= (uint32_t)N) break;
        x = p;
    }
    if (step > N) atomicOr(flag, FLAG_BOUND);
    root[i] = x;
}

__global__ __launch_bounds__(256) void root_flag_kernel(const int32_t *__restrict__ root, int N, int32_t *__restrict__ is_root,
                                                        int32_t *__restrict__ sizes) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= N) return;
    is_root[i] = root[i] == (int32_t)i ? 1 : 0;
    sizes[i] = 0;
}

// rank [N + 1]: the exclusive scan of the root flags; rank[N] = the number of clusters
__global__ __launch_bounds__(256) void dbscan_label_kernel(const int32_t *__restrict__ root, const int32_t *__restrict__ rank, int N,
                                                           int32_t *__restrict__ labels, int32_t *__restrict__ sizes,
                                                           int32_t *__restrict__ n_clusters) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= N) return;
    if (i == 0) *n_clusters = rank[N];
    const int32_t r = root[i];
    const int32_t l = (uint32_t)r < (uint32_t)N ? rank[r] : -1;
    labels[i] = l;
    // one atomicAdd per distinct label of the wavefront, not per lane (a few large clusters: every lane would hit the same words):
    // the first lane still to be counted names its label, the lanes that share it are counted by that lane at once.  At most 64
    // rounds, each retiring at least the naming lane; an integer sum, exact whatever the order.
    bool todo = l >= 0;
    const int lane = threadIdx.x & 63;
    for (int round = 0; round < 64; ++round) {
        const unsigned long long live = __ballot(todo);
        if (!live) break;
        const int leader = __ffsll(live) - 1;
        const int32_t named = __shfl(l, leader, 64);
        const unsigned long long same = __ballot(todo && l == named);
        if (lane == leader) atomicAdd(sizes + named, (int)__popcll(same));
        if (l == named) todo = false;
    }
}

// exclusive scan of v [n] (0 / 1 flags; overwritten with the starts) -> start [n + 1]: the three kernels of the grid build
void scan_flags(int32_t *v, int n, int32_t *start, int32_t *tile_sum, hipStream_t s) {
    const int ntile = (n + SCAN_TILE - 1) / SCAN_TILE;
    SGAM_KLAUNCH(points_grid_tilesum_kernel, dim3(ntile), dim3(256), 0, s, v, n, tile_sum);
    SGAM_KLAUNCH(points_grid_tilescan_kernel, dim3(1), dim3(1024), 0, s, tile_sum, ntile);
    SGAM_KLAUNCH(points_grid_starts_kernel, dim3(ntile), dim3(256), 0, s, n, tile_sum, start, v);
}

int64_t scan_bytes(int64_t n) { return r16(4 * n) + r16(4 * (n + 1)) + r16(4 * ((n + SCAN_TILE - 1) / SCAN_TILE)); }

struct ScanTables {
    int32_t *flags, *start, *tile_sum;
};

char *carve_scan(char *p, int64_t n, ScanTables &t) {
    t.flags = (int32_t *)p;                 p += r16(4 * n);
    t.start = (int32_t *)p;                 p += r16(4 * (n + 1));
    t.tile_sum = (int32_t *)p;              p += r16(4 * ((n + SCAN_TILE - 1) / SCAN_TILE));
    return p;
}

int64_t dbscan_bytes(int64_t N) {
    if (N < 1 || N > 0x7ffffffell) return SGAM_EINVAL;
    return 2 * r16(4 * N) + scan_bytes(N);
}

// the grid a walk goes through (grid != nullptr: the arguments of sgam_points_grid_build, whose tables the workspace holds)
struct GridArgs {
    int32_t Nr;
    float ox, oy, oz, cell_size;
    int32_t gx, gy, gz;
    const void *workspace;
    int64_t workspace_bytes;
};

bool make_walk(const float *points, int32_t N, const GridArgs *grid, float max_d2, Walk &W) {
    if (!points || N < 1 || !(max_d2 >= 0.f)) return false;
    W.points = points; W.N = N; W.max_d2 = max_d2; W.sorted = nullptr; W.start = nullptr;
    W.G = Grid{0.f, 0.f, 0.f, 1.f, 0.f, 1, 1, 1};
    if (!grid) return true;
    GridTables w;
    if (grid->Nr != N || !make_grid(grid->ox, grid->oy, grid->oz, grid->cell_size, grid->gx, grid->gy, grid->gz, W.G) ||
        !grid_tables(grid->workspace, grid->workspace_bytes, N, POINT_RECORD, grid->gx, grid->gy, grid->gz, w))
        return false;
    W.sorted = w.records; W.start = w.start;
    return true;
}

int radius_count(const float *points, int32_t N, const GridArgs *grid, float max_d2, int32_t *count_out, void *stream) {
    Walk W;
    if (!count_out || !make_walk(points, N, grid, max_d2, W)) return SGAM_EINVAL;
    SGAM_KLAUNCH(radius_walk_kernel<0>, dim3(blocks_of(N)), dim3(256), 0, sgam_stream(stream), W, 0, count_out, (int32_t *)nullptr,
                 (int32_t *)nullptr, (int32_t *)nullptr);
    SGAM_LAUNCH_CHECK();
    return SGAM_OK;
}

int dbscan(const float *points, int32_t N, const GridArgs *grid, float max_d2, int32_t min_points, void *workspace, int64_t workspace_bytes,
           int32_t *count_out, uint8_t *core_out, int32_t *labels_out, int32_t *sizes_out, int32_t *n_clusters_out, int32_t *flag,
           void *stream) {
    Walk W;
    if (!count_out || !core_out || !labels_out || !sizes_out || !n_clusters_out || !flag || min_points < 1 ||
        !make_walk(points, N, grid, max_d2, W))
        return SGAM_EINVAL;
    if (!workspace_fits(workspace, workspace_bytes, dbscan_bytes(N))) return SGAM_EWORKSPACE;
    char *p = (char *)workspace;
    int32_t *parent = (int32_t *)p;         p += r16(4 * (int64_t)N);
    int32_t *root = (int32_t *)p;           p += r16(4 * (int64_t)N);
    ScanTables t;
    carve_scan(p, N, t);
    hipStream_t s = sgam_stream(stream);
    const dim3 grid_(blocks_of(N)), blk(256);
    SGAM_KLAUNCH(radius_walk_kernel<0>, grid_, blk, 0, s, W, min_points, count_out, parent, root, flag);
    SGAM_KLAUNCH(iota_kernel, grid_, blk, 0, s, parent, N);
    SGAM_KLAUNCH(radius_walk_kernel<1>, grid_, blk, 0, s, W, min_points, count_out, parent, root, flag);
    SGAM_KLAUNCH(dbscan_flatten_kernel, grid_, blk, 0, s, parent, count_out, N, min_points, root, core_out, flag);
    SGAM_KLAUNCH(radius_walk_kernel<2>, grid_, blk, 0, s, W, min_points, count_out, parent, root, flag);
    SGAM_KLAUNCH(root_flag_kernel, grid_, blk, 0, s, root, N, t.flags, sizes_out);
    scan_flags(t.flags, N, t.start, t.tile_sum, s);
    SGAM_KLAUNCH(dbscan_label_kernel, grid_, blk, 0, s, root, t.start, N, labels_out, sizes_out, n_clusters_out);
    SGAM_LAUNCH_CHECK();
    return SGAM_OK;
}

// ---------------------------------------------------------------- planes
__device__ __forceinline__ bool plane_inlier(float a, float b, float c, float d, float x, float y, float z, float thr) {
    return fabsf(__fadd_rn(__fadd_rn(__fadd_rn(__fmul_rn(a, x), __fmul_rn(b, y)), __fmul_rn(c, z)), d)) <= thr;       // (NaN fails)
}

__device__ __forceinline__ bool active_point(const float *__restrict__ points, const int32_t *__restrict__ labels, int64_t i, float &x,
                                             float &y, float &z) {
    x = points[i * 3]; y = points[i * 3 + 1]; z = points[i * 3 + 2];
    return finite3(x, y, z) && (!labels || labels[i] < 0);
}

__global__ __launch_bounds__(256) void active_flag_kernel(const float *__restrict__ points, const int32_t *__restrict__ labels, int N,
                                                          int32_t *__restrict__ flags) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= N) return;
    float x, y, z;
    flags[i] = active_point(points, labels, i, x, y, z) ? 1 : 0;
}

// start: the exclusive scan of the flags, so list is ascending
__global__ __launch_bounds__(256) void active_scatter_kernel(const float *__restrict__ points, const int32_t *__restrict__ labels, int N,
                                                             const int32_t *__restrict__ start, int32_t *__restrict__ list) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= N) return;
    float x, y, z;
    if (!active_point(points, labels, i, x, y, z)) return;
    const int32_t pos = start[i];
    if ((uint32_t)pos < (uint32_t)N) list[pos] = (int32_t)i;
}

// one lane per hypothesis; n_active = start[N] on the device
__global__ __launch_bounds__(256) void plane_hypotheses_kernel(const float *__restrict__ points, int N, const int32_t *__restrict__ list,
                                                               const int32_t *__restrict__ n_active_p, int H, int round, uint32_t seed_lo,
                                                               uint32_t seed_hi, float4 *__restrict__ planes, int32_t *__restrict__ counts) {
    const int64_t h = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (h >= H) return;
    const float nan = __uint_as_float(0x7fc00000u);
    float4 plane = make_float4(nan, nan, nan, nan);
    counts[h] = 0;
    const int n_active = min(max(*n_active_p, 0), N);
    int pick[3] = {-1, -1, -1};
    int draws = 0;
    bool ok = n_active >= 3;
#pragma unroll
    for (int s = 0; s < 3; ++s) {
        int got = -1;
        while (ok && draws < PLANE_MAX_DRAWS) {
            uint32_t w[4] = {(uint32_t)h, (uint32_t)draws, (uint32_t)round, 0u};
            sgam_philox4x32_10(w, seed_lo, seed_hi);
            ++draws;
            const int cand = (int)(((uint64_t)w[0] * (uint64_t)(uint32_t)n_active) >> 32);
            bool dup = false;
#pragma unroll
            for (int t = 0; t < s; ++t) dup = dup || pick[t] == cand;
            if (!dup) { got = cand; break; }
        }
        pick[s] = got;
        ok = ok && got >= 0;
    }
    if (ok) {
        double p[3][3];
#pragma unroll
        for (int s = 0; s < 3; ++s) {
            const int64_t i = min(max(list[pick[s]], 0), N - 1);
#pragma unroll
            for (int a = 0; a < 3; ++a) p[s][a] = (double)points[i * 3 + a];
        }
        const double ux = p[1][0] - p[0][0], uy = p[1][1] - p[0][1], uz = p[1][2] - p[0][2];
        const double vx = p[2][0] - p[0][0], vy = p[2][1] - p[0][1], vz = p[2][2] - p[0][2];
        double nx = uy * vz - uz * vy, ny = uz * vx - ux * vz, nz = ux * vy - uy * vx;
        const double nn = (nx * nx + ny * ny) + nz * nz;
        if (nn > 0.0 && finite_f64(nn)) {
            const double inv = 1.0 / sqrt(nn);
            nx *= inv; ny *= inv; nz *= inv;
            const double d = -((nx * p[0][0] + ny * p[0][1]) + nz * p[0][2]);
            plane = make_float4((float)nx, (float)ny, (float)nz, (float)d);
        }
    }
    planes[h] = plane;
}

// grid (hypothesis tiles of 256 R, point chunks): lane <-> R hypotheses, the chunk's points through LDS
template <int R>
__global__ __launch_bounds__(256) void plane_score_kernel(const float *__restrict__ points, const int32_t *__restrict__ labels, int N,
                                                          const float4 *__restrict__ planes, int H, float thr, int chunk,
                                                          int32_t *__restrict__ counts) {
    __shared__ float4 tile[SCORE_TILE];
    const float nan = __uint_as_float(0x7fc00000u);
    const int64_t h0 = (int64_t)blockIdx.x * (256 * R) + threadIdx.x;
    float4 pl[R];
    int cnt[R];
#pragma unroll
    for (int r = 0; r < R; ++r) {
        const int64_t h = h0 + r * 256;
        pl[r] = h < H ? planes[h] : make_float4(nan, nan, nan, nan);
        cnt[r] = 0;
    }
    const int64_t p0 = (int64_t)blockIdx.y * chunk, p1 = min((int64_t)N, p0 + chunk);
    for (int64_t t0 = p0; t0 < p1; t0 += SCORE_TILE) {                        // (block-uniform)
        const int n = (int)min((int64_t)SCORE_TILE, p1 - t0);
        __syncthreads();
        for (int k = threadIdx.x; k < n; k += blockDim.x) {
            float x, y, z;
            const bool a = active_point(points, labels, t0 + k, x, y, z);
            tile[k] = a ? make_float4(x, y, z, 0.f) : make_float4(nan, nan, nan, nan);
        }
        __syncthreads();
#pragma unroll 4
        for (int k = 0; k < n; ++k) {
            const float4 p = tile[k];                                         // one 16-byte address for the wavefront: a broadcast
#pragma unroll
            for (int r = 0; r < R; ++r) cnt[r] += plane_inlier(pl[r].x, pl[r].y, pl[r].z, pl[r].w, p.x, p.y, p.z, thr) ? 1 : 0;
        }
    }
#pragma unroll
    for (int r = 0; r < R; ++r) {
        const int64_t h = h0 + r * 256;
        if (h < H && cnt[r]) atomicAdd(counts + h, cnt[r]);
    }
}

// one workgroup: the winner of the round -> best [4] = (a, b, c, d) (NaN: none), ransac_planes[round], counts_out[round]
__global__ __launch_bounds__(256) void plane_select_kernel(const float4 *__restrict__ planes, const int32_t *__restrict__ counts, int H,
                                                           int min_inliers, int round, float *__restrict__ best,
                                                           float *__restrict__ ransac_planes, int32_t *__restrict__ counts_out) {
    __shared__ int sc[256], sh[256];
    int bc = -1, bh = -1;
    for (int h = threadIdx.x; h < H; h += 256) {                              // ascending: the first of equal counts stays
        const float4 p = planes[h];
        const int c = counts[h];
        if (finite3(p.x, p.y, p.z) && fabsf(p.w) <= F32_MAX && c > bc) { bc = c; bh = h; }
    }
    sc[threadIdx.x] = bc; sh[threadIdx.x] = bh;
    __syncthreads();
    if (threadIdx.x != 0) return;
    for (int l = 1; l < 256; ++l)
        if (sc[l] > bc || (sc[l] == bc && sh[l] >= 0 && sh[l] < bh)) { bc = sc[l]; bh = sh[l]; }
    const float nan = __uint_as_float(0x7fc00000u);
    float4 p = make_float4(nan, nan, nan, nan);
    int c = 0;
    if (bh >= 0 && bc >= max(min_inliers, 3)) { p = planes[bh]; c = bc; }
    best[0] = p.x; best[1] = p.y; best[2] = p.z; best[3] = p.w;
    ransac_planes[round * 4] = p.x; ransac_planes[round * 4 + 1] = p.y; ransac_planes[round * 4 + 2] = p.z; ransac_planes[round * 4 + 3] = p.w;
    counts_out[round] = c;
}

__global__ __launch_bounds__(256) void plane_inliers_kernel(const float *__restrict__ points, int N, const float *__restrict__ best, float thr,
                                                            int round, int32_t *__restrict__ labels) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= N) return;
    float x, y, z;
    if (!active_point(points, labels, i, x, y, z)) return;
    if (plane_inlier(best[0], best[1], best[2], best[3], x, y, z, thr)) labels[i] = round;
}

// one workgroup per FIT_CHUNK points.  centroid == nullptr: partial[blk] = {sum x, sum y, sum z, number} over the round's inliers;
// else the centred second moments {xx, xy, xz, yy, yz, zz} about centroid [3]
__global__ __launch_bounds__(256) void plane_fit_sums_kernel(const float *__restrict__ points, const int32_t *__restrict__ labels, int N, int round,
                                                             const double *__restrict__ centroid, double *__restrict__ partial) {
    const int64_t base = (int64_t)blockIdx.x * FIT_CHUNK;
    double s[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    double cx = 0.0, cy = 0.0, cz = 0.0;
    if (centroid) { cx = centroid[0]; cy = centroid[1]; cz = centroid[2]; }
    for (int c = 0; c < FIT_CHUNK / 256; ++c) {
        const int64_t i = base + c * 256 + threadIdx.x;
        if (i >= N) break;
        if (labels[i] != round) continue;
        const double x = (double)points[i * 3], y = (double)points[i * 3 + 1], z = (double)points[i * 3 + 2];
        if (!centroid) {
            s[0] += x; s[1] += y; s[2] += z; s[3] += 1.0;
        } else {
            const double ex = x - cx, ey = y - cy, ez = z - cz;
            s[0] += ex * ex; s[1] += ex * ey; s[2] += ex * ez; s[3] += ey * ey; s[4] += ey * ez; s[5] += ez * ez;
        }
    }
    block_sum_f64(s, partial);
}

// one workgroup: the block partials folded in block order (lane c folds column c).  Pass 0: fit[0..2] = centroid, fit[3] = number.
// Pass 1: the plane of the moments -> planes_out[round]
__global__ __launch_bounds__(64) void plane_fit_fold_kernel(const double *__restrict__ partial, int blocks, int pass, double *__restrict__ fit,
                                                            const float *__restrict__ best, int round, float *__restrict__ planes_out) {
    __shared__ double m[6];
    if (threadIdx.x < 6) {
        double s = 0.0;
        for (int b = 0; b < blocks; ++b) s += partial[(int64_t)b * 6 + threadIdx.x];
        m[threadIdx.x] = s;
    }
    __syncthreads();
    if (threadIdx.x != 0) return;
    if (pass == 0) {
        const double n = m[3];
        fit[0] = m[0] / n; fit[1] = m[1] / n; fit[2] = m[2] / n; fit[3] = n;      // (no inlier: NaN, and pass 1 writes NaN)
        return;
    }
    const float nanf_ = __uint_as_float(0x7fc00000u);
    float4 out = make_float4(nanf_, nanf_, nanf_, nanf_);
    if (fit[3] >= 3.0 && finite3(best[0], best[1], best[2])) {
        double a00 = m[0], a01 = m[1], a02 = m[2], a11 = m[3], a12 = m[4], a22 = m[5];
        double v00 = 1.0, v01 = 0.0, v02 = 0.0, v10 = 0.0, v11 = 1.0, v12 = 0.0, v20 = 0.0, v21 = 0.0, v22 = 1.0;
        for (int sweep = 0; sweep < JACOBI_SWEEPS; ++sweep) {                 // a fixed count: no convergence test
            jacobi_rotate(a00, a11, a01, a02, a12, v00, v01, v10, v11, v20, v21);         // (p, q, r) = (0, 1, 2)
            jacobi_rotate(a00, a22, a02, a01, a12, v00, v02, v10, v12, v20, v22);         // (0, 2, 1)
            jacobi_rotate(a11, a22, a12, a01, a02, v01, v02, v11, v12, v21, v22);         // (1, 2, 0)
        }
        const bool s1 = a11 < a00;                                            // the least eigenvalue, the lowest axis on a tie
        const bool s2 = a22 < (s1 ? a11 : a00);
        double ex = s2 ? v02 : (s1 ? v01 : v00), ey = s2 ? v12 : (s1 ? v11 : v10), ez = s2 ? v22 : (s1 ? v21 : v20);
        const double inv = 1.0 / sqrt((ex * ex + ey * ey) + ez * ez);
        ex *= inv; ey *= inv; ez *= inv;
        if ((ex * (double)best[0] + ey * (double)best[1]) + ez * (double)best[2] < 0.0) { ex = -ex; ey = -ey; ez = -ez; }
        const double d = -((ex * fit[0] + ey * fit[1]) + ez * fit[2]);
        out = make_float4((float)ex, (float)ey, (float)ez, (float)d);
    }
    planes_out[round * 4] = out.x; planes_out[round * 4 + 1] = out.y; planes_out[round * 4 + 2] = out.z; planes_out[round * 4 + 3] = out.w;
}

int64_t fit_blocks(int64_t N) { return (N + FIT_CHUNK - 1) / FIT_CHUNK; }

int64_t planes_bytes(int64_t N, int64_t H) {
    if (N < 1 || N > 0x7ffffffell || H < 1 || H > (1 << 24)) return SGAM_EINVAL;
    return scan_bytes(N) + r16(4 * N) + 16 * H + r16(4 * H) + r16(8 * 6 * fit_blocks(N)) + 64;
}

bool score_launch(const float *points, const int32_t *labels, int32_t N, const float4 *planes, int32_t H, float thr, int R, int32_t *counts,
                  hipStream_t s) {
    if (R == 0) R = H <= 256 ? 1 : H <= 512 ? 2 : 4;                      // the least R whose one tile holds H, else 4
    if (R != 1 && R != 2 && R != 4) return false;
    const int htiles = (H + 256 * R - 1) / (256 * R);
    const int want = std::max(1, (SCORE_MIN_WORKGROUPS + htiles - 1) / htiles);          // point chunks for two workgroups per CU
    int64_t chunk = ((int64_t)N + want - 1) / want;
    chunk = std::min<int64_t>(std::max<int64_t>((chunk + SCORE_TILE - 1) / SCORE_TILE * SCORE_TILE, SCORE_TILE), 1 << 30);
    int64_t nchunk = ((int64_t)N + chunk - 1) / chunk;
    while (nchunk > 65535) { chunk *= 2; nchunk = ((int64_t)N + chunk - 1) / chunk; }
    const dim3 grid((unsigned)htiles, (unsigned)nchunk), blk(256);
    if (R == 1) SGAM_KLAUNCH(plane_score_kernel<1>, grid, blk, 0, s, points, labels, N, planes, H, thr, (int)chunk, counts);
    else if (R == 2) SGAM_KLAUNCH(plane_score_kernel<2>, grid, blk, 0, s, points, labels, N, planes, H, thr, (int)chunk, counts);
    else SGAM_KLAUNCH(plane_score_kernel<4>, grid, blk, 0, s, points, labels, N, planes, H, thr, (int)chunk, counts);
    return true;
}

// ---------------------------------------------------------------- boxes
// a key of an fp32 that orders like its value as an unsigned integer
__device__ __forceinline__ uint32_t ordered_key(float v) {
    const uint32_t u = __float_as_uint(v);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float ordered_value(uint32_t k) { return __uint_as_float((k & 0x80000000u) ? (k & 0x7fffffffu) : ~k); }

__global__ __launch_bounds__(256) void boxes_init_kernel(int n, int32_t *__restrict__ count, uint32_t *__restrict__ lo, uint32_t *__restrict__ hi) {
    const int64_t c = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= n) return;
    count[c] = 0;
    for (int a = 0; a < 3; ++a) { lo[c * 3 + a] = 0xffffffffu; hi[c * 3 + a] = 0u; }
}

__global__ __launch_bounds__(256) void boxes_accumulate_kernel(const float *__restrict__ points, const int32_t *__restrict__ labels, int N, int n,
                                                               int32_t *__restrict__ count, uint32_t *__restrict__ lo, uint32_t *__restrict__ hi) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= N) return;
    const int32_t l = labels[i];
    if ((uint32_t)l >= (uint32_t)n) return;
    const float p[3] = {points[i * 3], points[i * 3 + 1], points[i * 3 + 2]};
    if (!finite3(p[0], p[1], p[2])) return;
    atomicAdd(count + l, 1);
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        const uint32_t k = ordered_key(p[a]);
        atomicMin(lo + (int64_t)l * 3 + a, k);
        atomicMax(hi + (int64_t)l * 3 + a, k);
    }
}

// keys -> values in place; a label without a point: lo +inf, hi -inf
__global__ __launch_bounds__(256) void boxes_decode_kernel(int n, const int32_t *__restrict__ count, uint32_t *lo, uint32_t *hi) {
    const int64_t c = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= n) return;
    const bool any = count[c] > 0;
    for (int a = 0; a < 3; ++a) {
        const float l = any ? ordered_value(lo[c * 3 + a]) : __uint_as_float(0x7f800000u);
        const float h = any ? ordered_value(hi[c * 3 + a]) : __uint_as_float(0xff800000u);
        lo[c * 3 + a] = __float_as_uint(l);
        hi[c * 3 + a] = __float_as_uint(h);
    }
}

}  // namespace

extern "C" int sgam_points_radius_count_brute_f32(const float *points, int32_t N, float max_d2, int32_t *count_out, void *stream) {
    return radius_count(points, N, nullptr, max_d2, count_out, stream);
}

extern "C" int sgam_points_radius_count_grid_f32(const float *points, int32_t Nr, float ox, float oy, float oz, float cell_size, int32_t gx,
                                                 int32_t gy, int32_t gz, const void *grid_workspace, int64_t grid_workspace_bytes, float max_d2,
                                                 int32_t *count_out, void *stream) {
    const GridArgs g{Nr, ox, oy, oz, cell_size, gx, gy, gz, grid_workspace, grid_workspace_bytes};
    return radius_count(points, Nr, &g, max_d2, count_out, stream);
}

extern "C" int64_t sgam_points_dbscan_workspace_bytes(int32_t N) { return dbscan_bytes(N); }

extern "C" int sgam_points_dbscan_brute_f32(const float *points, int32_t N, float max_d2, int32_t min_points, void *workspace,
                                            int64_t workspace_bytes, int32_t *count_out, uint8_t *core_out, int32_t *labels_out,
                                            int32_t *sizes_out, int32_t *n_clusters_out, int32_t *flag, void *stream) {
    return dbscan(points, N, nullptr, max_d2, min_points, workspace, workspace_bytes, count_out, core_out, labels_out, sizes_out, n_clusters_out,
                  flag, stream);
}

extern "C" int sgam_points_dbscan_grid_f32(const float *points, int32_t Nr, float ox, float oy, float oz, float cell_size, int32_t gx, int32_t gy,
                                           int32_t gz, const void *grid_workspace, int64_t grid_workspace_bytes, float max_d2,
                                           int32_t min_points, void *workspace, int64_t workspace_bytes, int32_t *count_out, uint8_t *core_out,
                                           int32_t *labels_out, int32_t *sizes_out, int32_t *n_clusters_out, int32_t *flag, void *stream) {
    const GridArgs g{Nr, ox, oy, oz, cell_size, gx, gy, gz, grid_workspace, grid_workspace_bytes};
    return dbscan(points, Nr, &g, max_d2, min_points, workspace, workspace_bytes, count_out, core_out, labels_out, sizes_out, n_clusters_out,
                  flag, stream);
}

extern "C" int sgam_points_plane_score_f32(const float *points, const int32_t *labels, int32_t N, const float *planes, int32_t H,
                                           float threshold, int32_t R, int32_t *counts_out, void *stream) {
    if (!points || !planes || !counts_out || N < 1 || H < 1 || H > (1 << 24) || !(threshold >= 0.f) || !sgam_aligned16(planes) ||
        !(R == 0 || R == 1 || R == 2 || R == 4))
        return SGAM_EINVAL;
    hipStream_t s = sgam_stream(stream);
    SGAM_KLAUNCH(fill_kernel<int32_t>, dim3(std::min(blocks_of(H), 1u << 16)), dim3(256), 0, s, counts_out, (int64_t)H, 0);
    score_launch(points, labels, N, (const float4 *)planes, H, threshold, R, counts_out, s);
    SGAM_LAUNCH_CHECK();
    return SGAM_OK;
}

extern "C" int64_t sgam_points_planes_workspace_bytes(int32_t N, int32_t H) { return planes_bytes(N, H); }

extern "C" int sgam_points_segment_planes_f32(const float *points, int32_t N, int32_t H, int32_t max_planes, float threshold,
                                              int32_t min_inliers, uint64_t seed, void *workspace, int64_t workspace_bytes,
                                              int32_t *labels_out, float *planes_out, float *ransac_planes_out, int32_t *counts_out,
                                              void *stream) {
    if (!points || !labels_out || !planes_out || !ransac_planes_out || !counts_out || N < 1 || H < 1 || max_planes < 1 ||
        max_planes > 65536 || min_inliers < 0 || !(threshold >= 0.f) || planes_bytes(N, H) < 0)
        return SGAM_EINVAL;
    if (!workspace_fits(workspace, workspace_bytes, planes_bytes(N, H))) return SGAM_EWORKSPACE;
    ScanTables t;
    char *p = carve_scan((char *)workspace, N, t);
    int32_t *list = (int32_t *)p;           p += r16(4 * (int64_t)N);
    float4 *hyp = (float4 *)p;              p += 16 * (int64_t)H;
    int32_t *hcount = (int32_t *)p;         p += r16(4 * (int64_t)H);
    double *partial = (double *)p;          p += r16(8 * 6 * fit_blocks(N));
    double *fit = (double *)p;              // [4]
    float *best = (float *)(p + 32);        // [4]
    const uint32_t lo = (uint32_t)(seed & 0xffffffffull), hi = (uint32_t)(seed >> 32);
    hipStream_t s = sgam_stream(stream);
    const dim3 over_n(blocks_of(N)), blk(256);
    const int blocks = (int)fit_blocks(N);
    SGAM_KLAUNCH(fill_kernel<int32_t>, dim3(std::min(blocks_of(N), 1u << 16)), blk, 0, s, labels_out, (int64_t)N, -1);
    for (int r = 0; r < max_planes; ++r) {
        SGAM_KLAUNCH(active_flag_kernel, over_n, blk, 0, s, points, labels_out, N, t.flags);
        scan_flags(t.flags, N, t.start, t.tile_sum, s);
        SGAM_KLAUNCH(active_scatter_kernel, over_n, blk, 0, s, points, labels_out, N, t.start, list);
        SGAM_KLAUNCH(plane_hypotheses_kernel, dim3(blocks_of(H)), blk, 0, s, points, N, list, t.start + N, H, r, lo, hi, hyp, hcount);
        score_launch(points, labels_out, N, hyp, H, threshold, 0, hcount, s);
        SGAM_KLAUNCH(plane_select_kernel, dim3(1), blk, 0, s, hyp, hcount, H, min_inliers, r, best, ransac_planes_out, counts_out);
        SGAM_KLAUNCH(plane_inliers_kernel, over_n, blk, 0, s, points, N, best, threshold, r, labels_out);
        SGAM_KLAUNCH(plane_fit_sums_kernel, dim3(blocks), blk, 0, s, points, labels_out, N, r, (const double *)nullptr, partial);
        SGAM_KLAUNCH(plane_fit_fold_kernel, dim3(1), dim3(64), 0, s, partial, blocks, 0, fit, best, r, planes_out);
        SGAM_KLAUNCH(plane_fit_sums_kernel, dim3(blocks), blk, 0, s, points, labels_out, N, r, (const double *)fit, partial);
        SGAM_KLAUNCH(plane_fit_fold_kernel, dim3(1), dim3(64), 0, s, partial, blocks, 1, fit, best, r, planes_out);
    }
    SGAM_LAUNCH_CHECK();
    return SGAM_OK;
}

extern "C" int sgam_points_cluster_boxes_f32(const float *points, const int32_t *labels, int32_t N, int32_t n_clusters, int32_t *count_out,
                                             float *lo_out, float *hi_out, void *stream) {
    if (!points || !labels || !count_out || !lo_out || !hi_out || N < 1 || n_clusters < 1) return SGAM_EINVAL;
    hipStream_t s = sgam_stream(stream);
    SGAM_KLAUNCH(boxes_init_kernel, dim3(blocks_of(n_clusters)), dim3(256), 0, s, n_clusters, count_out, (uint32_t *)lo_out, (uint32_t *)hi_out);
    SGAM_KLAUNCH(boxes_accumulate_kernel, dim3(blocks_of(N)), dim3(256), 0, s, points, labels, N, n_clusters, count_out, (uint32_t *)lo_out,
                 (uint32_t *)hi_out);
    SGAM_KLAUNCH(boxes_decode_kernel, dim3(blocks_of(n_clusters)), dim3(256), 0, s, n_clusters, count_out, (uint32_t *)lo_out,
                 (uint32_t *)hi_out);
    SGAM_LAUNCH_CHECK();
    return SGAM_OK;
}
