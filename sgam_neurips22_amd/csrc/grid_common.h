// grid_common.h — the uniform grid that point_nn.hip (cells of points) and mesh_query.hip (cells of triangles) share: the grid
// descriptor and its cell rule, the exclusive scan of the per-cell counts, the shell search, and the tables in a caller's workspace
// with the launches that build them, each written ONCE over what a cell's records are.  point_nn.hip's header has the search's
// stop rule and its proof for points, mesh_query.hip's the changes for triangles.
//
// grid_search is a template over the sink that takes the candidates and over `Cells`, which knows the records:
//     cells.scan(s, e, qx, qy, qz, max_d2, sink)   offers the records [s, e) of the cell-sorted table to the sink
//     Cells::shrink()                              the factor below 1 of the stop rule (relative rounding of a distance)
// G.margin is the stop rule's absolute term; make_grid takes it as a multiple of the grid's coordinate scale.
#pragma once
#include "points_common.h"

#include <algorithm>
#include <cmath>

namespace {

constexpr int SCAN_TILE = 1024;               // cells per workgroup of the scan (256 lanes x 4)
constexpr int64_t GRID_MAX_CELLS = 1ll << 24; // 2 x 64 MB of cell tables at most

struct Grid {
    float ox, oy, oz, h, margin;
    int gx, gy, gz;
};

__device__ __forceinline__ int cell_of(float p, float o, float h, int g) {
    float t = floorf(__fdiv_rn(__fsub_rn(p, o), h));
    t = fminf(fmaxf(t, 0.0f), (float)(g - 1));                                // clamped as a float: no integer overflow
    return (int)t;
}

__device__ __forceinline__ int cell_index(const Grid &G, float x, float y, float z) {
    return (cell_of(z, G.oz, G.h, G.gz) * G.gy + cell_of(y, G.oy, G.h, G.gy)) * G.gx + cell_of(x, G.ox, G.h, G.gx);
}

// exclusive scan of one value per lane over a workgroup of NW waves; total = the workgroup's sum (fixed order: integers)
template <int NW>
__device__ __forceinline__ int block_exclusive_scan(int v, int *lds, int &total) {
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    int inc = v;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const int t = __shfl_up(inc, o, 64);
        if (lane >= o) inc += t;
    }
    if (lane == 63) lds[w] = inc;
    __syncthreads();
    int base = 0;
    total = 0;
#pragma unroll
    for (int k = 0; k < NW; ++k) {
        const int s = lds[k];
        if (k < w) base += s;
        total += s;
    }
    __syncthreads();
    return base + inc - v;
}

// pass 1: the sum of every tile of SCAN_TILE cells
__global__ __launch_bounds__(256) void points_grid_tilesum_kernel(const int32_t *__restrict__ count, int ncell, int32_t *__restrict__ tile_sum) {
    __shared__ int lds[4];
    const int c0 = blockIdx.x * SCAN_TILE + threadIdx.x * 4;
    int s = 0;
#pragma unroll
    for (int k = 0; k < 4; ++k) s += c0 + k < ncell ? count[c0 + k] : 0;
    int total;
    block_exclusive_scan<4>(s, lds, total);
    if (threadIdx.x == 0) tile_sum[blockIdx.x] = total;
}

// pass 2 (one workgroup): tile sums -> exclusive offsets, in place
__global__ __launch_bounds__(1024) void points_grid_tilescan_kernel(int32_t *__restrict__ tile_sum, int ntile) {
    __shared__ int lds[16];
    const int per = (ntile + 1023) / 1024;
    const int t0 = threadIdx.x * per;
    int s = 0;
    for (int k = 0; k < per; ++k) s += t0 + k < ntile ? tile_sum[t0 + k] : 0;
    int total;
    int run = block_exclusive_scan<16>(s, lds, total);
    for (int k = 0; k < per; ++k) {
        if (t0 + k >= ntile) break;
        const int v = tile_sum[t0 + k];
        tile_sum[t0 + k] = run;
        run += v;
    }
}

// pass 3: start[c] = cursor[c] = records in the cells before c; start[ncell] = all of them
// (`cursor` holds the counts on entry: every lane reads its four before it writes them)
__global__ __launch_bounds__(256) void points_grid_starts_kernel(int ncell, const int32_t *__restrict__ tile_sum, int32_t *__restrict__ start,
                                                                 int32_t *cursor) {
    __shared__ int lds[4];
    const int c0 = blockIdx.x * SCAN_TILE + threadIdx.x * 4;
    int v[4], s = 0;
#pragma unroll
    for (int k = 0; k < 4; ++k) { v[k] = c0 + k < ncell ? cursor[c0 + k] : 0; s += v[k]; }
    int total;
    int run = tile_sum[blockIdx.x] + block_exclusive_scan<4>(s, lds, total);
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        if (c0 + k < ncell) { start[c0 + k] = run; cursor[c0 + k] = run; }
        run += v[k];
        if (c0 + k == ncell - 1) start[ncell] = run;
    }
}

// the shell search for one finite query: shells of cells around the query's cell are offered to the sink until the stop rule
// holds against sink.bound() or the block covers the grid
template <class Sink, class Cells>
__device__ __forceinline__ void grid_search(const Grid &G, const Cells &cells, const int32_t *__restrict__ start, float qx, float qy, float qz,
                                            float max_d2, Sink &sink) {
    const int cx = cell_of(qx, G.ox, G.h, G.gx), cy = cell_of(qy, G.oy, G.h, G.gy), cz = cell_of(qz, G.oz, G.h, G.gz);
    for (int r = 0;; ++r) {
        const int x0 = max(cx - r, 0), x1 = min(cx + r, G.gx - 1);
        const int y0 = max(cy - r, 0), y1 = min(cy + r, G.gy - 1);
        const int z0 = max(cz - r, 0), z1 = min(cz + r, G.gz - 1);
        for (int z = z0; z <= z1; ++z) {
            const bool zface = z == cz - r || z == cz + r;
            for (int y = y0; y <= y1; ++y) {
                const int row = (z * G.gy + y) * G.gx;
                if (zface || y == cy - r || y == cy + r) {                    // a whole row of the shell: its cells are contiguous
                    cells.scan(start[row + x0], start[row + x1 + 1], qx, qy, qz, max_d2, sink);
                } else {                                                      // (r >= 1 here) the two end cells of the row
                    if (cx - r >= 0) cells.scan(start[row + cx - r], start[row + cx - r + 1], qx, qy, qz, max_d2, sink);
                    if (cx + r < G.gx) cells.scan(start[row + cx + r], start[row + cx + r + 1], qx, qy, qz, max_d2, sink);
                }
            }
        }
        const bool lo_x = cx - r > 0, hi_x = cx + r < G.gx - 1, lo_y = cy - r > 0, hi_y = cy + r < G.gy - 1, lo_z = cz - r > 0,
                   hi_z = cz + r < G.gz - 1;                                  // faces of the block that are not grid borders
        if (!(lo_x || hi_x || lo_y || hi_y || lo_z || hi_z)) break;           // the block is the grid: everything was visited
        float m = __uint_as_float(0x7f800000u);
        if (lo_x) m = fminf(m, __fsub_rn(qx, __fadd_rn(G.ox, __fmul_rn((float)(cx - r), G.h))));
        if (hi_x) m = fminf(m, __fsub_rn(__fadd_rn(G.ox, __fmul_rn((float)(cx + r + 1), G.h)), qx));
        if (lo_y) m = fminf(m, __fsub_rn(qy, __fadd_rn(G.oy, __fmul_rn((float)(cy - r), G.h))));
        if (hi_y) m = fminf(m, __fsub_rn(__fadd_rn(G.oy, __fmul_rn((float)(cy + r + 1), G.h)), qy));
        if (lo_z) m = fminf(m, __fsub_rn(qz, __fadd_rn(G.oz, __fmul_rn((float)(cz - r), G.h))));
        if (hi_z) m = fminf(m, __fsub_rn(__fadd_rn(G.oz, __fmul_rn((float)(cz + r + 1), G.h)), qz));
        const float ms = __fmul_rn(__fsub_rn(m, G.margin), Cells::shrink());
        if (ms > 0.0f) {
            const float lb = __fmul_rn(ms, ms);
            if (sink.bound() < lb || lb > max_d2) break;
        }
    }
}

// the grid descriptor both the build and the query derive from the caller's numbers (so they cannot disagree);
// margin = margin_factor * (largest |coordinate| of the grid's corners + its longest edge)
bool make_grid(float ox, float oy, float oz, float h, int gx, int gy, int gz, Grid &G, double margin_factor = 1.0 / 65536.0) {
    if (!(std::fabs(ox) <= F32_MAX && std::fabs(oy) <= F32_MAX && std::fabs(oz) <= F32_MAX) || !(h > 0.f && h <= F32_MAX)) return false;
    if (gx < 1 || gy < 1 || gz < 1 || (int64_t)gx * gy > GRID_MAX_CELLS || (int64_t)gx * gy * gz > GRID_MAX_CELLS) return false;
    const double o[3] = {ox, oy, oz};
    const int g[3] = {gx, gy, gz};
    double corner = 0.0, edge = 0.0;
    for (int a = 0; a < 3; ++a) {
        corner = std::max(corner, std::max(std::fabs(o[a]), std::fabs(o[a] + (double)g[a] * h)));
        edge = std::max(edge, (double)g[a] * h);
    }
    const double margin = (corner + edge) * margin_factor;
    if (!(margin <= F32_MAX)) return false;
    G.ox = ox; G.oy = oy; G.oz = oz; G.h = h; G.margin = (float)margin;
    G.gx = gx; G.gy = gy; G.gz = gz;
    return true;
}

// ---------------------------------------------------------------- the grid's tables and their build (host side)
// A caller's workspace, carved: the cell-sorted records (16 B per point, 48 B per triangle entry), start [ncell + 1], cursor [ncell]
// (the counts until the scan has turned them into starts, then each cell's write position), tile_sum [ntile].
struct GridTables {
    float4 *records;
    int32_t *start, *cursor, *tile_sum;
    int ncell, ntile;
};

// bytes of the tables of n_records records of record_bytes each; SGAM_EINVAL for sizes the grid does not take
int64_t grid_tables_bytes(int64_t n_records, int record_bytes, int gx, int gy, int gz) {
    if (n_records < 1 || n_records > 0x7fffffffll || gx < 1 || gy < 1 || gz < 1 || (int64_t)gx * gy > GRID_MAX_CELLS ||
        (int64_t)gx * gy * gz > GRID_MAX_CELLS)
        return SGAM_EINVAL;
    const int64_t ncell = (int64_t)gx * gy * gz;
    return record_bytes * n_records + r16(4 * (ncell + 1)) + r16(4 * ncell) + r16(4 * ((ncell + SCAN_TILE - 1) / SCAN_TILE));
}

// the tables inside a caller's workspace; false: the sizes are refused or the workspace does not hold them
bool grid_tables(const void *workspace, int64_t workspace_bytes, int64_t n_records, int record_bytes, int gx, int gy, int gz, GridTables &w) {
    if (!workspace_fits(workspace, workspace_bytes, grid_tables_bytes(n_records, record_bytes, gx, gy, gz))) return false;
    w.ncell = gx * gy * gz;
    w.ntile = (w.ncell + SCAN_TILE - 1) / SCAN_TILE;
    char *p = (char *)const_cast<void *>(workspace);
    w.records = (float4 *)p;                p += record_bytes * n_records;
    w.start = (int32_t *)p;                 p += r16(4 * ((int64_t)w.ncell + 1));
    w.cursor = (int32_t *)p;                p += r16(4 * (int64_t)w.ncell);
    w.tile_sum = (int32_t *)p;
    return true;
}

// the six launches of a build: clear -> count(w.cursor) -> tile sums -> tile scan -> starts -> scatter(w.cursor, w.records); count
// and scatter are the caller's launches, the two that know what a record is
template <class Count, class Scatter>
void grid_build(const GridTables &w, hipStream_t s, Count count, Scatter scatter) {
    SGAM_KLAUNCH(fill_kernel<int32_t>, dim3(std::min(blocks_of(w.ncell), 1u << 16)), dim3(256), 0, s, w.cursor, (int64_t)w.ncell, 0);
    count();
    SGAM_KLAUNCH(points_grid_tilesum_kernel, dim3(w.ntile), dim3(256), 0, s, w.cursor, w.ncell, w.tile_sum);
    SGAM_KLAUNCH(points_grid_tilescan_kernel, dim3(1), dim3(1024), 0, s, w.tile_sum, w.ntile);
    SGAM_KLAUNCH(points_grid_starts_kernel, dim3(w.ntile), dim3(256), 0, s, w.ncell, w.tile_sum, w.start, w.cursor);
    scatter();
}

}  // namespace
