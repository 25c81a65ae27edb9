// mesh_query.hip — what is measured against a triangle mesh (vertices [nv][3] fp32, triangles [nt][3] int32): the exact distance
// from a point to the mesh — brute force through LDS tiles (sgam_mesh_distance_brute_f32) and a uniform grid of triangles searched
// in growing shells (sgam_mesh_grid_count, sgam_mesh_grid_build, sgam_mesh_distance_grid_f32) — and points drawn uniformly by area
// (sgam_mesh_triangle_area2_f32, sgam_mesh_sample_f32).  points_common.h's rules hold: every fp32 operator is ONE IEEE operation in
// the written order (the unit is built with -ffp-contract=off and the operations are spelled out), "not a point" is finite3, and
// tests/meshquery_oracle.py restates everything in numpy; the outputs are compared bit for bit.  DESIGN §4.4.8.
//
// dot(u, v) = (u.x * v.x + u.y * v.y) + u.z * v.z.   A triangle (a, b, c) is a CANDIDATE when its nine coordinates are finite and
// its normal n = ab x ac (ab = b - a, ac = c - a; n.x = ab.y * ac.z - ab.z * ac.y, n.y = ab.z * ac.x - ab.x * ac.z, n.z = ab.x *
// ac.y - ab.y * ac.x: two products and one difference each) has dot(n, n) > 0; anything else is "not a triangle" and never wins.
// A triangle that names a vertex outside [0, nv) ORs 2 into the caller's flag word and is skipped (mesh_common.h: the flag bits, the
// corner load and the range check, shared with mesh_ops.hip; dot3, the candidate rule and the record layout, shared with mesh_ray.hip;
// point_triangle and MeshSink live in mesh_rules.h, which mesh_bvh.hip includes too).
//
// Closest point of a candidate to a query q (Ericson, Real-Time Collision Detection §5.1.5: the seven Voronoi regions):
//     ap = q - a, bp = q - b, cp = q - c
//     p1 = dot(ab, ap)  p2 = dot(ac, ap)  p3 = dot(ab, bp)  p4 = dot(ac, bp)  p5 = dot(ab, cp)  p6 = dot(ac, cp)
//     vc = p1 * p4 - p3 * p2      vb = p5 * p2 - p1 * p6      va = p3 * p6 - p5 * p4      e43 = p4 - p3      e56 = p5 - p6
// The region is the FIRST of these tests that holds, in this order (code: 0 1 2 vertices a b c, 3 4 5 edges ab bc ca, 6 the face):
//     0: p1 <= 0 && p2 <= 0        1: p3 >= 0 && p4 <= p3        3: vc <= 0 && p1 >= 0 && p3 <= 0        2: p6 >= 0 && p5 <= p6
//     5: vb <= 0 && p2 >= 0 && p6 <= 0        4: va <= 0 && e43 >= 0 && e56 >= 0        6: otherwise
// and the closest point is, per coordinate, ONE expression for every region, so that no lane branches:
//     x = (base + e1 * (n1 / m1)) + ac * (n2 / m2)
//     region   base  e1          n1 / m1                n2 / m2
//     0 1 2    a b c ab          0 / 1                  0 / 1
//     3        a     ab          p1 / (p1 - p3)         0 / 1
//     5        a     ac          p2 / (p2 - p6)         0 / 1
//     4        b     bc = c - b  e43 / (e43 + e56)      0 / 1
//     6        a     ab          vb / ((va + vb) + vc)  vc / ((va + vb) + vc)
// d2 = dist2(x, q).  The edge parameters lie in [0, 1] by their tests; a 0 / 0 (possible only where rounding has wiped out an edge)
// gives NaN, which never wins.
//
// The winner of a query is the candidate of least (d2 bits, triangle index) among those with d2 <= max_d2: an exact tie — the
// rule for a query nearest a shared edge or vertex — goes to the lower index; NaN and +inf never win; without a winner, and for a
// query that is not a point, triangle = -1, d2 = +inf, closest = NaN.
//
// Brute force: one lane per query; the triangles staged through LDS in tiles of 256 (nine gathered coordinates and the candidate
// mark, 10 KB; one lane gathers one triangle, once per tile) that every lane of the workgroup walks in index order (a broadcast
// read); `d2 < best` keeps the first of equal distances.
//
// Grid: grid_common.h's grid (point_nn.hip's cell rule, tables and build) over the box of the candidates' vertices.  A candidate is entered into
// EVERY cell of the block [cell_of(min), cell_of(max)] per axis of its bounding box: count (integer atomics) -> exclusive scan ->
// scatter of records (the nine coordinates and the id, 48 B: a cell's candidates are then one contiguous read, where records of
// ids alone would cost three dependent gathers per candidate; the choice is argued, not measured: DESIGN §4.4.8).  The order
// inside a cell depends on arrival and a triangle is met in several cells; the (d2, index) winner depends on neither.  The query is
// grid_common.h's shell walk — the one the nearest-neighbour kernels run — by one WAVEFRONT per query: the 64 lanes walk the same
// cells, share each row's records among them, and fold their winners at the end; with the stop rule
//     ms = (m - margin) * (1 - 2^-14) > 0   and   (best < ms * ms   or   ms * ms > max_d2),      margin = 2^-14 * the grid's scale.
// Convexity: a triangle that was not visited has its whole cell block outside the visited block on some axis, so its three
// vertices — and with them every point of it — lie beyond that face of the block (which is not a grid border: clamping moved
// outside vertices only towards the block).  Rounding: a computed point–triangle distance differs from the true one by K 2^-23 of
// (distance + grid scale), an ABSOLUTE term the point rule (2^-16, 1 - 2^-18) was not sized for; K is measured (2.32, DESIGN
// §4.4.8) and the wider margin and factor cover every K <= 2^8.
//
// Sampling: A2[t] = sqrt(dot(n, n)), twice the area (0 for "not a triangle").  The caller turns A2 into integer weights and their
// inclusive int64 sums cdf (integer plumbing; W = cdf[nt - 1]).  Sample i: the four words w0..w3 of Philox4x32-10 at counter
// (i lo32, i hi32, 0, 0), key (seed lo32, seed hi32); target = mulhi64((w0 << 32) | w1, W); triangle = the first t with
// cdf[t] > target (binary search); r1 = (w2 >> 8) * 2^-24, r2 = (w3 >> 8) * 2^-24; s = sqrt(r1), wa = 1 - s, wb = s * (1 - r2),
// wc = s * r2; per coordinate P = (wa * A + wb * B) + wc * C, colours alike; normal = n / sqrt(dot(n, n)) per component.
#include "grid_common.h"
#include "mesh_rules.h"

namespace {

// ---------------------------------------------------------------- brute force
// grid (blocks over the queries): one lane per query; the triangle tile is gathered once and walked by all lanes together
__global__ __launch_bounds__(256) void mesh_distance_brute_kernel(const float *__restrict__ vertices, int nv, const int32_t *__restrict__ triangles,
                                                                  int nt, const float *__restrict__ query, int Nq, float max_d2,
                                                                  float *__restrict__ d2_out, int32_t *__restrict__ tri_out,
                                                                  float *__restrict__ closest, int32_t *__restrict__ flag) {
    __shared__ float tile[TRI_TILE * 10];
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const bool live = i < Nq;
    const float nan = __uint_as_float(0x7fc00000u);
    float qx = nan, qy = nan, qz = nan;                                       // (a lane without a query, or with one that is not a point, takes nothing)
    if (live) { qx = query[i * 3]; qy = query[i * 3 + 1]; qz = query[i * 3 + 2]; }
    if (!finite3(qx, qy, qz)) qx = qy = qz = nan;
    MeshSink sink;
    for (int t0 = 0; t0 < nt; t0 += TRI_TILE) {                               // (block-uniform)
        const int n = min(TRI_TILE, nt - t0);
        __syncthreads();
        if ((int)threadIdx.x < n) {
            Tri T;
            float *__restrict__ rec = tile + threadIdx.x * 10;
            const bool ok = load_tri(vertices, nv, triangles, (int64_t)t0 + threadIdx.x, T, flag) && is_candidate(T);
            rec[9] = ok ? 1.0f : 0.0f;
            if (ok) { rec[0] = T.ax; rec[1] = T.ay; rec[2] = T.az; rec[3] = T.bx; rec[4] = T.by; rec[5] = T.bz; rec[6] = T.cx; rec[7] = T.cy; rec[8] = T.cz; }
        }
        __syncthreads();
        for (int k = 0; k < n; ++k) {
            const float *__restrict__ rec = tile + k * 10;
            if (rec[9] == 0.0f) continue;                                     // (block-uniform)
            const Tri T = {rec[0], rec[1], rec[2], rec[3], rec[4], rec[5], rec[6], rec[7], rec[8]};
            float x, y, z;
            int region;
            const float d2 = point_triangle(T, qx, qy, qz, x, y, z, region);
            if (d2 <= max_d2 && d2 < sink.best) { sink.best = d2; sink.bi = t0 + k; sink.x = x; sink.y = y; sink.z = z; }        // index order: the first of equal distances stays
        }
    }
    if (live) sink.write(i, d2_out, tri_out, closest);
}

// ---------------------------------------------------------------- the triangle grid
// the block of cells a candidate is entered into: [lo, hi] per axis
__device__ __forceinline__ void cell_block(const Grid &G, const Tri &T, int (&lo)[3], int (&hi)[3]) {
    lo[0] = cell_of(fminf(fminf(T.ax, T.bx), T.cx), G.ox, G.h, G.gx); hi[0] = cell_of(fmaxf(fmaxf(T.ax, T.bx), T.cx), G.ox, G.h, G.gx);
    lo[1] = cell_of(fminf(fminf(T.ay, T.by), T.cy), G.oy, G.h, G.gy); hi[1] = cell_of(fmaxf(fmaxf(T.ay, T.by), T.cy), G.oy, G.h, G.gy);
    lo[2] = cell_of(fminf(fminf(T.az, T.bz), T.cz), G.oz, G.h, G.gz); hi[2] = cell_of(fmaxf(fmaxf(T.az, T.bz), T.cz), G.oz, G.h, G.gz);
}

// totals[0] += the entries of the lane's triangle, totals[1] += 1 per candidate (64-bit integer atomics: order-free)
__global__ __launch_bounds__(256) void mesh_grid_total_kernel(Grid G, const float *__restrict__ vertices, int nv, const int32_t *__restrict__ triangles,
                                                              int nt, unsigned long long *__restrict__ totals, int32_t *__restrict__ flag) {
    const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= nt) return;
    Tri T;
    if (!load_tri(vertices, nv, triangles, t, T, flag) || !is_candidate(T)) return;
    int lo[3], hi[3];
    cell_block(G, T, lo, hi);
    atomicAdd(totals, (unsigned long long)(hi[0] - lo[0] + 1) * (unsigned long long)(hi[1] - lo[1] + 1) * (unsigned long long)(hi[2] - lo[2] + 1));
    atomicAdd(totals + 1, 1ull);
}

// SCATTER false: count[cell] += 1 for every cell of every candidate's block; true: the record is written at the cell's cursor
// (a position at or beyond n_entries — the mesh changed since it was counted — is not written: flag bit 1)
template <bool SCATTER>
__global__ __launch_bounds__(256) void mesh_grid_enter_kernel(Grid G, const float *__restrict__ vertices, int nv, const int32_t *__restrict__ triangles,
                                                              int nt, int32_t *__restrict__ cursor, float4 *__restrict__ records, int n_entries,
                                                              int32_t *__restrict__ flag) {
    const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= nt) return;
    Tri T;
    if (!load_tri(vertices, nv, triangles, t, T, flag) || !is_candidate(T)) return;
    int lo[3], hi[3];
    cell_block(G, T, lo, hi);
    for (int z = lo[2]; z <= hi[2]; ++z)
        for (int y = lo[1]; y <= hi[1]; ++y)
            for (int x = lo[0]; x <= hi[0]; ++x) {
                const int pos = atomicAdd(cursor + (z * G.gy + y) * G.gx + x, 1);
                if (!SCATTER) continue;
                if ((uint32_t)pos >= (uint32_t)n_entries) { atomicOr(flag, FLAG_BOUND); continue; }
                records[(int64_t)pos * 3] = make_float4(T.ax, T.ay, T.az, __int_as_float((int)t));
                records[(int64_t)pos * 3 + 1] = make_float4(T.bx, T.by, T.bz, 0.0f);
                records[(int64_t)pos * 3 + 2] = make_float4(T.cx, T.cy, T.cz, 0.0f);
            }
}

// a cell's records are candidates: three float4 (a, id), (b, 0), (c, 0); the stop rule's factor 1 - 2^-14 (the unit's header)
struct TriangleCells {
    const float4 *__restrict__ records;
    int n_entries;
    static __device__ __forceinline__ float shrink() { return 0.99993896484375f; }
    __device__ __forceinline__ void scan(int s, int e, float qx, float qy, float qz, float max_d2, MeshSink &sink) const {
        s = max(s, 0);
        e = min(e, n_entries);                                                // (a table that is not this grid's still reads inside the workspace)
        for (int k = s + (int)(threadIdx.x & 63); k < e; k += 64) {             // the wave's lanes share the cells' records
            const float4 a = records[(int64_t)k * 3], b = records[(int64_t)k * 3 + 1], c = records[(int64_t)k * 3 + 2];
            const Tri T = {a.x, a.y, a.z, b.x, b.y, b.z, c.x, c.y, c.z};
            float x, y, z;
            int region;
            const float d2 = point_triangle(T, qx, qy, qz, x, y, z, region);
            sink.offer(d2, __float_as_int(a.w), max_d2, x, y, z);
        }
    }
};

// one wavefront per query (four queries per workgroup): a query near a large or distant part of the surface meets thousands of
// candidates, and one lane walking them alone (three dependent 16-byte loads and some 300 operations each) held its whole
// wave for milliseconds; shared among 64 lanes the records of a row of cells are one coalesced read
__global__ __launch_bounds__(256) void mesh_distance_grid_kernel(Grid G, const float *__restrict__ query, int Nq, const float4 *__restrict__ records,
                                                                 int n_entries, const int32_t *__restrict__ start, float max_d2,
                                                                 float *__restrict__ d2_out, int32_t *__restrict__ tri_out, float *__restrict__ closest) {
    const int64_t i = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (i >= Nq) return;                                                      // (wave-uniform; no barrier below)
    const float qx = query[i * 3], qy = query[i * 3 + 1], qz = query[i * 3 + 2];
    MeshSink sink;
    if (finite3(qx, qy, qz)) grid_search(G, TriangleCells{records, n_entries}, start, qx, qy, qz, max_d2, sink);
    sink.fold_wave();
    if ((threadIdx.x & 63) == 0) sink.write(i, d2_out, tri_out, closest);
}

// ---------------------------------------------------------------- area-uniform sampling
__global__ __launch_bounds__(256) void mesh_area2_kernel(const float *__restrict__ vertices, int nv, const int32_t *__restrict__ triangles, int nt,
                                                         float *__restrict__ area2, int32_t *__restrict__ flag) {
    const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= nt) return;
    Tri T;
    float a2 = 0.0f;
    if (load_tri(vertices, nv, triangles, t, T, flag) && finite3(T.ax, T.ay, T.az) && finite3(T.bx, T.by, T.bz) && finite3(T.cx, T.cy, T.cz)) {
        float nx, ny, nz;
        const float nn = normal_of(T, nx, ny, nz);
        if (nn > 0.0f) a2 = sqrt_rn(nn);
    }
    area2[t] = a2;
}

__device__ __forceinline__ float mix3(float wa, float a, float wb, float b, float wc, float c) {
    return __fadd_rn(__fadd_rn(__fmul_rn(wa, a), __fmul_rn(wb, b)), __fmul_rn(wc, c));
}

// one lane per sample
__global__ __launch_bounds__(256) void mesh_sample_kernel(const float *__restrict__ vertices, const float *__restrict__ colors, int nv,
                                                          const int32_t *__restrict__ triangles, int nt, const int64_t *__restrict__ cdf,
                                                          uint32_t seed_lo, uint32_t seed_hi, int64_t n, float *__restrict__ points,
                                                          int32_t *__restrict__ tri_out, float *__restrict__ colors_out, float *__restrict__ normals_out,
                                                          int32_t *__restrict__ flag) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    uint32_t w[4] = {(uint32_t)i, (uint32_t)((uint64_t)i >> 32), 0u, 0u};
    sgam_philox4x32_10(w, seed_lo, seed_hi);
    const uint64_t W = (uint64_t)cdf[nt - 1];
    const int64_t target = (int64_t)__umul64hi(((uint64_t)w[0] << 32) | w[1], W);          // < W
    int lo = 0, hi = nt - 1;                                                  // the first t with cdf[t] > target lies in [lo, hi]
    while (lo < hi) {                                                         // (at most 28 rounds: nt <= 2^28)
        const int mid = lo + ((hi - lo) >> 1);
        if (cdf[mid] > target) hi = mid; else lo = mid + 1;
    }
    const float r1 = __fmul_rn((float)(w[2] >> 8), 5.9604644775390625e-8f), r2 = __fmul_rn((float)(w[3] >> 8), 5.9604644775390625e-8f);
    const float s = sqrt_rn(r1);
    const float wa = __fsub_rn(1.0f, s), wb = __fmul_rn(s, __fsub_rn(1.0f, r2)), wc = __fmul_rn(s, r2);
    const float nan = __uint_as_float(0x7fc00000u);
    int32_t a, b, c;
    const bool ok = corners_checked(triangles, lo, nv, a, b, c, flag);
    tri_out[i] = lo;
    float A[3], B[3], C[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        A[k] = ok ? vertices[(int64_t)a * 3 + k] : nan; B[k] = ok ? vertices[(int64_t)b * 3 + k] : nan; C[k] = ok ? vertices[(int64_t)c * 3 + k] : nan;
        points[i * 3 + k] = mix3(wa, A[k], wb, B[k], wc, C[k]);
        if (colors_out)
            colors_out[i * 3 + k] = ok ? mix3(wa, colors[(int64_t)a * 3 + k], wb, colors[(int64_t)b * 3 + k], wc, colors[(int64_t)c * 3 + k]) : nan;
    }
    if (normals_out) {
        const Tri T = {A[0], A[1], A[2], B[0], B[1], B[2], C[0], C[1], C[2]};
        float nx, ny, nz;
        const float l = sqrt_rn(normal_of(T, nx, ny, nz));
        normals_out[i * 3] = __fdiv_rn(nx, l); normals_out[i * 3 + 1] = __fdiv_rn(ny, l); normals_out[i * 3 + 2] = __fdiv_rn(nz, l);
    }
}

}  // namespace

extern "C" int sgam_mesh_distance_brute_f32(const float *vertices, int32_t nv, const int32_t *triangles, int32_t nt, const float *query,
                                            int32_t Nq, float max_d2, float *d2_out, int32_t *triangle_out, float *closest_out, int32_t *flag,
                                            void *stream) {
    if (!mesh_args_ok(vertices, nv, triangles, nt, flag) || !query || !d2_out || !triangle_out || Nq < 1 || !(max_d2 >= 0.f)) return SGAM_EINVAL;
    SGAM_KLAUNCH(mesh_distance_brute_kernel, dim3(blocks_of(Nq)), dim3(256), 0, sgam_stream(stream), vertices, nv, triangles, nt, query, Nq, max_d2,
                 d2_out, triangle_out, closest_out, flag);
    SGAM_LAUNCH_CHECK();
    return SGAM_OK;
}

extern "C" int64_t sgam_mesh_grid_workspace_bytes(int64_t n_entries, int32_t gx, int32_t gy, int32_t gz) {
    return grid_tables_bytes(n_entries, TRIANGLE_RECORD, gx, gy, gz);
}

extern "C" int sgam_mesh_grid_count(const float *vertices, int32_t nv, const int32_t *triangles, int32_t nt, float ox, float oy, float oz,
                                    float cell_size, int32_t gx, int32_t gy, int32_t gz, int64_t *totals_out, int32_t *flag, void *stream) {
    Grid G;
    if (!mesh_args_ok(vertices, nv, triangles, nt, flag) || !totals_out || !make_grid(ox, oy, oz, cell_size, gx, gy, gz, G, MESH_MARGIN))
        return SGAM_EINVAL;
    hipStream_t s = sgam_stream(stream);
    SGAM_KLAUNCH(fill_kernel<int32_t>, dim3(1), dim3(256), 0, s, (int32_t *)totals_out, (int64_t)4, 0);        // the two int64 totals
    SGAM_KLAUNCH(mesh_grid_total_kernel, dim3(blocks_of(nt)), dim3(256), 0, s, G, vertices, nv, triangles, nt, (unsigned long long *)totals_out,
                 flag);
    SGAM_LAUNCH_CHECK();
    return SGAM_OK;
}

extern "C" int sgam_mesh_grid_build(const float *vertices, int32_t nv, const int32_t *triangles, int32_t nt, float ox, float oy, float oz,
                                    float cell_size, int32_t gx, int32_t gy, int32_t gz, int64_t n_entries, void *workspace,
                                    int64_t workspace_bytes, int32_t *flag, void *stream) {
    Grid G;
    GridTables w;
    if (!mesh_args_ok(vertices, nv, triangles, nt, flag) || !make_grid(ox, oy, oz, cell_size, gx, gy, gz, G, MESH_MARGIN) ||
        !grid_tables(workspace, workspace_bytes, n_entries, TRIANGLE_RECORD, gx, gy, gz, w))
        return SGAM_EINVAL;
    hipStream_t s = sgam_stream(stream);
    grid_build(
        w, s,
        [&] {
            SGAM_KLAUNCH(mesh_grid_enter_kernel<false>, dim3(blocks_of(nt)), dim3(256), 0, s, G, vertices, nv, triangles, nt, w.cursor, w.records,
                         (int)n_entries, flag);
        },
        [&] {
            SGAM_KLAUNCH(mesh_grid_enter_kernel<true>, dim3(blocks_of(nt)), dim3(256), 0, s, G, vertices, nv, triangles, nt, w.cursor, w.records,
                         (int)n_entries, flag);
        });
    SGAM_LAUNCH_CHECK();
    return SGAM_OK;
}

extern "C" int sgam_mesh_distance_grid_f32(const float *query, int32_t Nq, int64_t n_entries, float ox, float oy, float oz, float cell_size,
                                           int32_t gx, int32_t gy, int32_t gz, const void *workspace, int64_t workspace_bytes, float max_d2,
                                           float *d2_out, int32_t *triangle_out, float *closest_out, void *stream) {
    Grid G;
    GridTables w;
    if (!query || !d2_out || !triangle_out || Nq < 1 || !(max_d2 >= 0.f) || !make_grid(ox, oy, oz, cell_size, gx, gy, gz, G, MESH_MARGIN) ||
        !grid_tables(workspace, workspace_bytes, n_entries, TRIANGLE_RECORD, gx, gy, gz, w))
        return SGAM_EINVAL;
    SGAM_KLAUNCH(mesh_distance_grid_kernel, dim3((unsigned)(((int64_t)Nq + 3) / 4)), dim3(256), 0, sgam_stream(stream), G, query, Nq, w.records,
                 (int)n_entries, w.start, max_d2, d2_out, triangle_out, closest_out);
    SGAM_LAUNCH_CHECK();
    return SGAM_OK;
}

extern "C" int sgam_mesh_triangle_area2_f32(const float *vertices, int32_t nv, const int32_t *triangles, int32_t nt, float *area2_out,
                                            int32_t *flag, void *stream) {
    if (!mesh_args_ok(vertices, nv, triangles, nt, flag) || !area2_out) return SGAM_EINVAL;
    SGAM_KLAUNCH(mesh_area2_kernel, dim3(blocks_of(nt)), dim3(256), 0, sgam_stream(stream), vertices, nv, triangles, nt, area2_out, flag);
    SGAM_LAUNCH_CHECK();
    return SGAM_OK;
}

extern "C" int sgam_mesh_sample_f32(const float *vertices, const float *vertex_colors, int32_t nv, const int32_t *triangles, int32_t nt,
                                    const int64_t *cdf, uint64_t seed, int64_t n, float *points_out, int32_t *triangle_out, float *colors_out,
                                    float *normals_out, int32_t *flag, void *stream) {
    if (!mesh_args_ok(vertices, nv, triangles, nt, flag) || !cdf || !points_out || !triangle_out || n < 1 || n > 0x7fffffffll ||
        (colors_out != nullptr && vertex_colors == nullptr))
        return SGAM_EINVAL;
    SGAM_KLAUNCH(mesh_sample_kernel, dim3(blocks_of(n)), dim3(256), 0, sgam_stream(stream), vertices, vertex_colors, nv, triangles, nt, cdf,
                 (uint32_t)seed, (uint32_t)(seed >> 32), n, points_out, triangle_out, colors_out, normals_out, flag);
    SGAM_LAUNCH_CHECK();
    return SGAM_OK;
}
