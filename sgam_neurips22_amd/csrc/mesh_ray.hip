// mesh_ray.hip — rays against a triangle mesh (vertices [nv][3] fp32, triangles [nt][3] int32): the nearest hit and the any-hit
// (occlusion) query by brute force through LDS tiles (sgam_mesh_raycast_brute_f32) and by a walk through mesh_query.hip's triangle
// grid (sgam_mesh_raycast_grid_f32: the tables sgam_mesh_grid_build writes, nothing built here), the visibility of points from a
// set of pinhole cameras with the mesh as the occluder (sgam_mesh_visibility_grid_f32 / _brute_f32: the N x P rays are formed in
// registers, never stored), and the rays of pinhole images (sgam_rays_pinhole_f32).  points_common.h's rules hold: every fp32
// operator is ONE IEEE operation in the written order (the unit is built with -ffp-contract=off and the operations are spelled
// out), finite3 decides what is a point, dot(u, v) = (u.x * v.x + u.y * v.y) + u.z * v.z, a cross product's component is a
// difference of two products.  tests/raycast_oracle.py restates everything in numpy; the outputs are compared bit for bit.
// DESIGN §4.4.9.  The rule's code (ray_triangle, the sinks, the camera) lives in mesh_rules.h, which mesh_bvh.hip includes too.
//
// A RAY is six numbers (o, d); d is not normalised, so t is in units of |d|.  A ray with a component that is not finite or with
// d = 0 is "not a ray" and gets the no-hit answer.  A triangle is a CANDIDATE by mesh_common.h's rule (finite corners, dot(n, n) > 0).
//
// The intersection rule of a candidate (a, b, c) — Möller–Trumbore, two-sided, no culling:
//     e1 = b - a    e2 = c - a    p = d x e2    det = dot(e1, p)    s = o - a
//     u = dot(s, p) / det    q = s x e1    v = dot(d, q) / det    t = dot(e2, q) / det + 0.0f          (-0 becomes 0)
//     P = o + t * d per coordinate (one product, one sum)
//     lo = min(min(a, b), c) - guard    hi = max(max(a, b), c) + guard per coordinate
// It is a HIT iff det != 0, u >= 0, v >= 0, u + v <= 1, tnear <= t <= tfar and lo <= P <= hi on every axis (the GUARD).  NaN fails
// every test, so NaN never hits.  The rule is not watertight: a ray through a shared edge or vertex may hit both triangles, one,
// or (rarely) neither, as rounding has it — the twin defines the truth.  The guard is part of the rule, in both kernels and in
// the twin: `guard` is an absolute length the caller passes, meshops.py passes 2^-15 of the largest |coordinate| of the
// candidates' vertices.  It discards a hit whose computed point lies off its triangle's bounding box — which rounding produces
// only for origins further than some 2^8 coordinate scales away (the error of P, 2^-24 |o|, then reaches the guard): such rays
// may lose hits, in both kernels alike.
//
// Nearest hit: the winner is the hit of least (t bits, triangle index) — t >= 0 (tnear >= 0 is required), so the bits order as
// integers; an exact tie goes to the lower index.  t_out = t (+inf without a hit), triangle_out = the index (-1), uv_out = (u, v)
// (NaN), normal_out = the winner's n / sqrt(dot(n, n)) per component, n = e1 x e2, not turned towards the ray (NaN).
// Any hit: hit_out = 1 iff some candidate hits; the walk is left at the first one.
//
// Brute force: one lane per ray; the triangles staged through LDS in tiles of TRI_TILE as in mesh_query.hip and walked in index
// order; `t < best` keeps the first of equal t.
//
// Grid: one lane per ray (a cell holds a handful of records: too few for a wavefront to share).  The walk covers the window in
// STEPS [ta, tb] that follow each other without a gap (the next ta IS the last tb, the first ta is tnear): along the axis m of
// the largest |d| a step ends where the ray leaves a layer of cells (tb = (plane - o_m) / d_m; any tb >= ta serves, the choice
// only decides the cost).  A step visits every cell of the box
//     [cell(min(P_j(ta), P_j(tb)) - margin), cell(max(P_j(ta), P_j(tb)) + margin)]    on each of the three axes j,
// P_j(t) = o_j + t * d_j as in the rule, cell() the grid's clamped cell rule, margin = G.margin (2^-14 of the grid's scale), and
// offers ALL records of those cells to the full window (cells of the previous step's box are not read twice).  Why the winner is
// never missed — by monotonicity, not by an error bound:
//   - t -> P_j(t) is monotone in fp32 (a product with a constant and a sum are, under round-to-nearest), so for every fp32 t in
//     [ta, tb] P_j(t) lies between P_j(ta) and P_j(tb), exactly;
//   - a hit at such a t has lo_j <= P_j(t) <= hi_j by the guard, and fl(max_j + guard) - margin <= max_j in exact arithmetic as
//     long as guard * (1 + 2^-9) <= margin (the entry points refuse 2 * guard > margin), so fl(P_j(t) - margin) <= max_j and, alike,
//     fl(P_j(t) + margin) >= min_j; cell() is monotone too, so the step's cell interval and the triangle's block [cell(min_j),
//     cell(max_j)] share a cell on every axis — and both being boxes, they share a cell;
//   - hence every candidate with a hit at a t inside a covered step has been offered.  STOP RULE: after a step, stop when
//     best <= tb (any hit not yet offered has t > tb >= best: it neither wins nor ties), when tb reached tfar, or when P_m(tb)
//     lies beyond the grid's far face by more than 2 margin (every later t lies further, and a counted hit lies within margin of
//     the box of the candidates' vertices).  The same forward test lets the walk start at the grid instead of at tnear.
// Domain: the grid's box holds the candidates' vertices (meshops.TriangleGrid builds it so) and 2 guard <= margin.  Then brute
// force and grid agree in every bit for every ray and every cell size; no measured constant enters.
//
// Visibility of a point x from pose M (4 x 4 row-major, world -> camera, rotation R = M[0..2][0..2], translation T = M[0..2][3]):
//     X = transform34(M, x)    c_k = -((R[0][k] * T[0] + R[1][k] * T[1]) + R[2][k] * T[2])      (the camera centre, R orthonormal)
//     in the frustum iff z_near <= X.z <= z_far and, with u = (fx * X.x) / X.z + cx, v = (fy * X.y) / X.z + cy, uf = floorf(u + 0.5f),
//     vf = floorf(v + 0.5f) (the point-splat view's pixel rule), 0 <= uf < W and 0 <= vf < H as float compares (NaN fails)
//     unoccluded iff the ray o = c, d = x - c has no hit in [0, 1 - tolerance]          (t = 1 is x itself)
// count_out[i] = the poses that see point i: one lane per point walks the poses, integers only.
//
// Pinhole rays of pose M, pixel (row i, column j): o = c as above; dc = ((j - cx) / fx, (i - cy) / fy, 1);
// d_k = (R[0][k] * dc.x + R[1][k] * dc.y) + R[2][k]: camera z = 1, so t is the view-space depth.
#include "grid_common.h"
#include "mesh_rules.h"

#include <type_traits>

namespace {

// ---------------------------------------------------------------- brute force
// the tile [t0, t0 + n) of the triangles into LDS (mesh_query.hip's layout: nine coordinates and the candidate mark); between two barriers
__device__ __forceinline__ void stage_tile(float *__restrict__ tile, const float *__restrict__ vertices, int nv, const int32_t *__restrict__ triangles,
                                           int t0, int n, int32_t *__restrict__ flag) {
    __syncthreads();
    if ((int)threadIdx.x < n) {
        Tri T;
        float *__restrict__ rec = tile + threadIdx.x * 10;
        const bool ok = load_tri(vertices, nv, triangles, (int64_t)t0 + threadIdx.x, T, flag) && is_candidate(T);
        rec[9] = ok ? 1.0f : 0.0f;
        if (ok) { rec[0] = T.ax; rec[1] = T.ay; rec[2] = T.az; rec[3] = T.bx; rec[4] = T.by; rec[5] = T.bz; rec[6] = T.cx; rec[7] = T.cy; rec[8] = T.cz; }
    }
    __syncthreads();
}

// a staged tile against one ray, in index order
template <class Sink>
__device__ __forceinline__ void walk_tile(const float *__restrict__ tile, int t0, int n, const Ray &r, const Window &w, Sink &sink) {
    for (int k = 0; k < n; ++k) {
        const float *__restrict__ rec = tile + k * 10;
        if (rec[9] == 0.0f) continue;                                         // (block-uniform)
        const Tri T = {rec[0], rec[1], rec[2], rec[3], rec[4], rec[5], rec[6], rec[7], rec[8]};
        float t, u, v;
        const bool hit = ray_triangle(T, r, w, t, u, v);
        sink.offer(hit, t, u, v, t0 + k, t0 + k);                             // index order: `t < best` keeps the first of equal t
    }
}

template <int MODE>
__global__ __launch_bounds__(256) void mesh_raycast_brute_kernel(const float *__restrict__ vertices, int nv, const int32_t *__restrict__ triangles,
                                                                 int nt, const float *__restrict__ rays, int Nr, Window w,
                                                                 float *__restrict__ t_out, int32_t *__restrict__ tri_out,
                                                                 float *__restrict__ uv_out, float *__restrict__ normal_out,
                                                                 uint8_t *__restrict__ hit_out, int32_t *__restrict__ flag) {
    __shared__ float tile[TRI_TILE * 10];
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const bool live = i < Nr;
    Ray r = not_a_ray();                                                      // (a lane without a ray, or with what is not one, hits nothing)
    if (live) r = {rays[i * 6], rays[i * 6 + 1], rays[i * 6 + 2], rays[i * 6 + 3], rays[i * 6 + 4], rays[i * 6 + 5]};
    if (!is_ray(r)) r = not_a_ray();
    typename std::conditional<MODE == MODE_ANY, AnySink, NearestSink>::type sink;
    for (int t0 = 0; t0 < nt; t0 += TRI_TILE) {                               // (block-uniform)
        const int n = min(TRI_TILE, nt - t0);
        stage_tile(tile, vertices, nv, triangles, t0, n, flag);
        walk_tile(tile, t0, n, r, w, sink);
    }
    if (!live) return;
    if constexpr (MODE == MODE_ANY) {
        hit_out[i] = sink.found ? 1 : 0;
    } else {
        write_nearest(sink, i, t_out, tri_out, uv_out);
        if (normal_out) {
            const float nan = __uint_as_float(0x7fc00000u);
            Tri T = {nan, nan, nan, nan, nan, nan, nan, nan, nan};
            if (sink.bi >= 0) load_tri(vertices, nv, triangles, sink.bi, T, flag);          // (a winner was loaded before: its corners are in the mesh)
            write_normal(T, normal_out + i * 3);
        }
    }
}

// ---------------------------------------------------------------- the walk through the triangle grid
struct RayGrid {
    Grid G;
    const float4 *__restrict__ records;
    const int32_t *__restrict__ start;
    int n_entries;
};

// the records of the cells [c0, c1] of one row (contiguous in the table) against the ray
template <class Sink>
__device__ __forceinline__ void scan_cells(const RayGrid &R, int row, int c0, int c1, const Ray &r, const Window &w, Sink &sink) {
    const int s = max(R.start[row + c0], 0), e = min(R.start[row + c1 + 1], R.n_entries);   // (a table that is not this grid's still reads inside the workspace)
    for (int k = s; k < e; ++k) {
        const float4 a = R.records[(int64_t)k * 3], b = R.records[(int64_t)k * 3 + 1], c = R.records[(int64_t)k * 3 + 2];
        const Tri T = {a.x, a.y, a.z, b.x, b.y, b.z, c.x, c.y, c.z};
        float t, u, v;
        const bool hit = ray_triangle(T, r, w, t, u, v);
        sink.offer(hit, t, u, v, __float_as_int(a.w), k);
        if (sink.full()) return;
    }
}

// the unit header's walk for one ray that is a ray; false: the walk ran into its bound (never, by the count of layers)
template <class Sink>
__device__ __forceinline__ bool ray_walk(const RayGrid &R, const Ray &r, const Window &w, Sink &sink) {
    const Grid &G = R.G;
    const float adx = fabsf(r.dx), ady = fabsf(r.dy), adz = fabsf(r.dz);
    const int m = (adx >= ady && adx >= adz) ? 0 : (ady >= adz ? 1 : 2);
    const float om = m == 0 ? r.ox : m == 1 ? r.oy : r.oz, dm = m == 0 ? r.dx : m == 1 ? r.dy : r.dz;
    const float Om = m == 0 ? G.ox : m == 1 ? G.oy : G.oz;
    const int gm = m == 0 ? G.gx : m == 1 ? G.gy : G.gz;
    const float W = G.margin, W2 = __fmul_rn(2.0f, W), W3 = __fmul_rn(3.0f, W);
    // the grid's box widened by 2 margin: no counted hit lies outside it
    const float lox = __fsub_rn(G.ox, W2), loy = __fsub_rn(G.oy, W2), loz = __fsub_rn(G.oz, W2);
    const float hix = __fadd_rn(__fadd_rn(G.ox, __fmul_rn((float)G.gx, G.h)), W2), hiy = __fadd_rn(__fadd_rn(G.oy, __fmul_rn((float)G.gy, G.h)), W2),
                hiz = __fadd_rn(__fadd_rn(G.oz, __fmul_rn((float)G.gz, G.h)), W2);
    const float lom = m == 0 ? lox : m == 1 ? loy : loz, him = m == 0 ? hix : m == 1 ? hiy : hiz;
    const bool fwd = dm > 0.0f;
    const float tend = fminf(w.tfar, F32_MAX);
    float ta = w.tnear;
    {   // start at the grid: a later start is taken only when the forward test shows that everything before it lies outside
        const float tc = __fdiv_rn(__fsub_rn(fwd ? __fsub_rn(lom, W2) : __fadd_rn(him, W2), om), dm);
        const float pm = along(om, dm, tc);
        if (tc > ta && (fwd ? pm < lom : pm > him)) ta = tc;
    }
    if (!(ta <= tend)) return true;
    int k = cell_of(along(om, dm, ta), Om, G.h, gm);
    int px0 = 1, px1 = 0, py0 = 1, py1 = 0, pz0 = 1, pz1 = 0;                  // the previous step's box (empty)
    for (int step = 0; step <= gm; ++step) {
        const bool last = fwd ? k >= gm - 1 : k <= 0;
        float tb;
        if (!last) {                                                          // a little past the plane between layer k and the next
            const float plane = __fadd_rn(Om, __fmul_rn((float)(fwd ? k + 1 : k), G.h));
            tb = __fdiv_rn(__fsub_rn(fwd ? __fadd_rn(plane, W3) : __fsub_rn(plane, W3), om), dm);
        } else {                                                              // past the grid's far face
            tb = __fdiv_rn(__fsub_rn(fwd ? __fadd_rn(him, W2) : __fsub_rn(lom, W2), om), dm);
        }
        tb = fminf(fmaxf(tb, ta), tend);
        if (last && tb < tend) {
            const float pm = along(om, dm, tb);
            if (!(fwd ? pm > him : pm < lom)) tb = tend;                      // (not shown to be outside: the rest of the window in one step)
        }
        const float x0 = along(r.ox, r.dx, ta), x1 = along(r.ox, r.dx, tb), y0 = along(r.oy, r.dy, ta), y1 = along(r.oy, r.dy, tb);
        const float z0 = along(r.oz, r.dz, ta), z1 = along(r.oz, r.dz, tb);
        const float mnx = fminf(x0, x1), mxx = fmaxf(x0, x1), mny = fminf(y0, y1), mxy = fmaxf(y0, y1), mnz = fminf(z0, z1), mxz = fmaxf(z0, z1);
        const bool outside = (mxx < lox) | (mnx > hix) | (mxy < loy) | (mny > hiy) | (mxz < loz) | (mnz > hiz);
        if (!outside) {
            const int cx0 = cell_of(__fsub_rn(mnx, W), G.ox, G.h, G.gx), cx1 = cell_of(__fadd_rn(mxx, W), G.ox, G.h, G.gx);
            const int cy0 = cell_of(__fsub_rn(mny, W), G.oy, G.h, G.gy), cy1 = cell_of(__fadd_rn(mxy, W), G.oy, G.h, G.gy);
            const int cz0 = cell_of(__fsub_rn(mnz, W), G.oz, G.h, G.gz), cz1 = cell_of(__fadd_rn(mxz, W), G.oz, G.h, G.gz);
            for (int z = cz0; z <= cz1; ++z)
                for (int y = cy0; y <= cy1; ++y) {
                    const int row = (z * G.gy + y) * G.gx;
                    if (z >= pz0 && z <= pz1 && y >= py0 && y <= py1) {       // a row of the previous box: only the cells beside it
                        if (cx0 < px0) scan_cells(R, row, cx0, min(cx1, px0 - 1), r, w, sink);
                        if (cx1 > px1 && !sink.full()) scan_cells(R, row, max(cx0, px1 + 1), cx1, r, w, sink);
                    } else {
                        scan_cells(R, row, cx0, cx1, r, w, sink);
                    }
                    if (sink.full()) return true;
                }
            px0 = cx0; px1 = cx1; py0 = cy0; py1 = cy1; pz0 = cz0; pz1 = cz1;
        }
        if (sink.done(tb) || tb >= tend || last) return true;
        ta = tb;
        k += fwd ? 1 : -1;
    }
    return false;
}

template <int MODE>
__global__ __launch_bounds__(256) void mesh_raycast_grid_kernel(RayGrid R, const float *__restrict__ rays, int Nr, Window w, float *__restrict__ t_out,
                                                                int32_t *__restrict__ tri_out, float *__restrict__ uv_out,
                                                                float *__restrict__ normal_out, uint8_t *__restrict__ hit_out,
                                                                int32_t *__restrict__ flag) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= Nr) return;                                                      // (no barrier below)
    const Ray r = {rays[i * 6], rays[i * 6 + 1], rays[i * 6 + 2], rays[i * 6 + 3], rays[i * 6 + 4], rays[i * 6 + 5]};
    typename std::conditional<MODE == MODE_ANY, AnySink, NearestSink>::type sink;
    if (is_ray(r) && !ray_walk(R, r, w, sink)) atomicOr(flag, FLAG_BOUND);
    if constexpr (MODE == MODE_ANY) {
        hit_out[i] = sink.found ? 1 : 0;
    } else {
        write_nearest(sink, i, t_out, tri_out, uv_out);
        if (normal_out) {
            const float nan = __uint_as_float(0x7fc00000u);
            Tri T = {nan, nan, nan, nan, nan, nan, nan, nan, nan};
            if (sink.where >= 0) {
                const float4 a = R.records[(int64_t)sink.where * 3], b = R.records[(int64_t)sink.where * 3 + 1], c = R.records[(int64_t)sink.where * 3 + 2];
                T = {a.x, a.y, a.z, b.x, b.y, b.z, c.x, c.y, c.z};
            }
            write_normal(T, normal_out + i * 3);
        }
    }
}

// ---------------------------------------------------------------- visibility
// one lane per point, the poses in turn
__global__ __launch_bounds__(256) void mesh_visibility_grid_kernel(RayGrid R, const float *__restrict__ points, int N, const float *__restrict__ poses,
                                                                   int P, Camera C, Window w, int32_t *__restrict__ count_out,
                                                                   int32_t *__restrict__ flag) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= N) return;
    const float x = points[i * 3], y = points[i * 3 + 1], z = points[i * 3 + 2];
    int count = 0;
    for (int p = 0; p < P; ++p) {
        Ray r;
        if (!in_frustum(C, poses + (int64_t)p * 16, x, y, z, r) || !is_ray(r)) continue;
        AnySink sink;
        if (!ray_walk(R, r, w, sink)) atomicOr(flag, FLAG_BOUND);
        count += sink.found ? 0 : 1;
    }
    count_out[i] = count;
}

// parity and small meshes: for every pose the triangle tiles are staged again (block-uniform loops)
__global__ __launch_bounds__(256) void mesh_visibility_brute_kernel(const float *__restrict__ vertices, int nv, const int32_t *__restrict__ triangles,
                                                                    int nt, const float *__restrict__ points, int N, const float *__restrict__ poses,
                                                                    int P, Camera C, Window w, int32_t *__restrict__ count_out,
                                                                    int32_t *__restrict__ flag) {
    __shared__ float tile[TRI_TILE * 10];
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const bool live = i < N;
    const float nan = __uint_as_float(0x7fc00000u);
    float x = nan, y = nan, z = nan;
    if (live) { x = points[i * 3]; y = points[i * 3 + 1]; z = points[i * 3 + 2]; }
    int count = 0;
    for (int p = 0; p < P; ++p) {
        Ray r;
        const bool seen = in_frustum(C, poses + (int64_t)p * 16, x, y, z, r) && is_ray(r);
        if (!seen) r = not_a_ray();
        AnySink sink;
        for (int t0 = 0; t0 < nt; t0 += TRI_TILE) {
            const int n = min(TRI_TILE, nt - t0);
            stage_tile(tile, vertices, nv, triangles, t0, n, flag);
            walk_tile(tile, t0, n, r, w, sink);
        }
        count += (seen && !sink.found) ? 1 : 0;
    }
    if (live) count_out[i] = count;
}

// one lane per pixel of every pose
__global__ __launch_bounds__(256) void rays_pinhole_kernel(const float *__restrict__ poses, int P, float fx, float fy, float cx, float cy, int H, int W,
                                                           float *__restrict__ rays) {
    const int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int64_t hw = (int64_t)H * W;
    if (idx >= hw * P) return;
    const int p = (int)(idx / hw), q = (int)(idx - (int64_t)p * hw), i = q / W, j = q - i * W;
    const float *__restrict__ M = poses + (int64_t)p * 16;
    float ox, oy, oz;
    camera_centre(M, ox, oy, oz);
    const float a = __fdiv_rn(__fsub_rn((float)j, cx), fx), b = __fdiv_rn(__fsub_rn((float)i, cy), fy);
    float *__restrict__ out = rays + idx * 6;
    out[0] = ox; out[1] = oy; out[2] = oz;
    out[3] = __fadd_rn(__fadd_rn(__fmul_rn(M[0], a), __fmul_rn(M[4], b)), M[8]);
    out[4] = __fadd_rn(__fadd_rn(__fmul_rn(M[1], a), __fmul_rn(M[5], b)), M[9]);
    out[5] = __fadd_rn(__fadd_rn(__fmul_rn(M[2], a), __fmul_rn(M[6], b)), M[10]);
}

// ---------------------------------------------------------------- host side
bool ray_grid(int64_t n_entries, float ox, float oy, float oz, float h, int gx, int gy, int gz, const void *workspace, int64_t workspace_bytes,
              float guard, RayGrid &R) {
    GridTables w;
    if (!make_grid(ox, oy, oz, h, gx, gy, gz, R.G, MESH_MARGIN) || !grid_tables(workspace, workspace_bytes, n_entries, TRIANGLE_RECORD, gx, gy, gz, w))
        return false;
    if (!(2.0 * (double)guard <= (double)R.G.margin)) return false;           // the walk's proof needs guard * (1 + 2^-9) <= margin
    R.records = w.records; R.start = w.start; R.n_entries = (int)n_entries;
    return true;
}

}  // namespace

extern "C" int sgam_mesh_raycast_brute_f32(const float *vertices, int32_t nv, const int32_t *triangles, int32_t nt, const float *rays, int32_t n_rays,
                                           int32_t mode, float tnear, float tfar, float guard, float *t_out, int32_t *triangle_out, float *uv_out,
                                           float *normal_out, uint8_t *hit_out, int32_t *flag, void *stream) {
    if (!mesh_args_ok(vertices, nv, triangles, nt, flag) || !rays || n_rays < 1 || !window_ok(tnear, tfar, guard) ||
        !outputs_ok(mode, t_out, triangle_out, hit_out))
        return SGAM_EINVAL;
    const Window w = {tnear, tfar, guard};
    if (mode == MODE_ANY)
        SGAM_KLAUNCH(mesh_raycast_brute_kernel<MODE_ANY>, dim3(blocks_of(n_rays)), dim3(256), 0, sgam_stream(stream), vertices, nv, triangles, nt, rays,
                     n_rays, w, t_out, triangle_out, uv_out, normal_out, hit_out, flag);
    else
        SGAM_KLAUNCH(mesh_raycast_brute_kernel<MODE_NEAREST>, dim3(blocks_of(n_rays)), dim3(256), 0, sgam_stream(stream), vertices, nv, triangles, nt,
                     rays, n_rays, w, t_out, triangle_out, uv_out, normal_out, hit_out, flag);
    SGAM_LAUNCH_CHECK();
    return SGAM_OK;
}

extern "C" int sgam_mesh_raycast_grid_f32(const float *rays, int32_t n_rays, int64_t n_entries, float ox, float oy, float oz, float cell_size,
                                          int32_t gx, int32_t gy, int32_t gz, const void *workspace, int64_t workspace_bytes, int32_t mode,
                                          float tnear, float tfar, float guard, float *t_out, int32_t *triangle_out, float *uv_out,
                                          float *normal_out, uint8_t *hit_out, int32_t *flag, void *stream) {
    RayGrid R;
    if (!rays || !flag || n_rays < 1 || !window_ok(tnear, tfar, guard) || !outputs_ok(mode, t_out, triangle_out, hit_out) ||
        !ray_grid(n_entries, ox, oy, oz, cell_size, gx, gy, gz, workspace, workspace_bytes, guard, R))
        return SGAM_EINVAL;
    const Window w = {tnear, tfar, guard};
    if (mode == MODE_ANY)
        SGAM_KLAUNCH(mesh_raycast_grid_kernel<MODE_ANY>, dim3(blocks_of(n_rays)), dim3(256), 0, sgam_stream(stream), R, rays, n_rays, w, t_out,
                     triangle_out, uv_out, normal_out, hit_out, flag);
    else
        SGAM_KLAUNCH(mesh_raycast_grid_kernel<MODE_NEAREST>, dim3(blocks_of(n_rays)), dim3(256), 0, sgam_stream(stream), R, rays, n_rays, w, t_out,
                     triangle_out, uv_out, normal_out, hit_out, flag);
    SGAM_LAUNCH_CHECK();
    return SGAM_OK;
}

extern "C" int sgam_mesh_visibility_grid_f32(const float *points, int32_t N, const float *poses_w2c, int32_t P, float fx, float fy, float cx,
                                             float cy, int32_t H, int32_t W, float z_near, float z_far, float tolerance, float guard,
                                             int64_t n_entries, float ox, float oy, float oz, float cell_size, int32_t gx, int32_t gy, int32_t gz,
                                             const void *workspace, int64_t workspace_bytes, int32_t *count_out, int32_t *flag, void *stream) {
    RayGrid R;
    Camera C;
    if (!points || !poses_w2c || !count_out || !flag || N < 1 || P < 1 || !(tolerance >= 0.f && tolerance <= 1.f) || !(guard >= 0.f && guard <= F32_MAX) ||
        !camera_ok(fx, fy, cx, cy, H, W, z_near, z_far, C) || !ray_grid(n_entries, ox, oy, oz, cell_size, gx, gy, gz, workspace, workspace_bytes, guard, R))
        return SGAM_EINVAL;
    const Window w = {0.0f, 1.0f - tolerance, guard};
    SGAM_KLAUNCH(mesh_visibility_grid_kernel, dim3(blocks_of(N)), dim3(256), 0, sgam_stream(stream), R, points, N, poses_w2c, P, C, w, count_out, flag);
    SGAM_LAUNCH_CHECK();
    return SGAM_OK;
}

extern "C" int sgam_mesh_visibility_brute_f32(const float *vertices, int32_t nv, const int32_t *triangles, int32_t nt, const float *points,
                                              int32_t N, const float *poses_w2c, int32_t P, float fx, float fy, float cx, float cy, int32_t H,
                                              int32_t W, float z_near, float z_far, float tolerance, float guard, int32_t *count_out,
                                              int32_t *flag, void *stream) {
    Camera C;
    if (!mesh_args_ok(vertices, nv, triangles, nt, flag) || !points || !poses_w2c || !count_out || N < 1 || P < 1 ||
        !(tolerance >= 0.f && tolerance <= 1.f) || !(guard >= 0.f && guard <= F32_MAX) || !camera_ok(fx, fy, cx, cy, H, W, z_near, z_far, C))
        return SGAM_EINVAL;
    const Window w = {0.0f, 1.0f - tolerance, guard};
    SGAM_KLAUNCH(mesh_visibility_brute_kernel, dim3(blocks_of(N)), dim3(256), 0, sgam_stream(stream), vertices, nv, triangles, nt, points, N, poses_w2c,
                 P, C, w, count_out, flag);
    SGAM_LAUNCH_CHECK();
    return SGAM_OK;
}

extern "C" int sgam_rays_pinhole_f32(const float *poses_w2c, int32_t P, float fx, float fy, float cx, float cy, int32_t H, int32_t W,
                                     float *rays_out, void *stream) {
    if (!poses_w2c || !rays_out || P < 1 || H < 1 || W < 1 || (int64_t)H * W * P > 0x7fffffffll || fx == 0.f || fy == 0.f ||
        !(std::fabs(fx) <= F32_MAX && std::fabs(fy) <= F32_MAX && std::fabs(cx) <= F32_MAX && std::fabs(cy) <= F32_MAX))
        return SGAM_EINVAL;
    SGAM_KLAUNCH(rays_pinhole_kernel, dim3(blocks_of((int64_t)H * W * P)), dim3(256), 0, sgam_stream(stream), poses_w2c, P, fx, fy, cx, cy, H, W, rays_out);
    SGAM_LAUNCH_CHECK();
    return SGAM_OK;
}
