// mesh_simplify.hip — quadric-error decimation of an indexed triangle mesh (vertices [nv][3] fp32, triangles [nt][3] int32) in
// parallel rounds: the vertex quadrics, the evaluation of every edge (the contraction target, its cost, the flip and link tests,
// the number of triangles it removes), the choice of an independent set of edges by two minimum passes over a scrambled edge id,
// and the application of the chosen collapses.  The rules are stated in include/sgam_hip.h and restated in numpy by
// tests/decimation_oracle.py; DESIGN §4.4.15.  No atomics but the flag word's: every minimum and every sum is a gather over a CSR
// segment by one lane, in the segment's order; all arithmetic is fp64 from widened fp32 inputs, one IEEE operation at a time in
// the written order (the unit is built with -ffp-contract=off), and a position is rounded to fp32 once.
//
// Every kernel checks a triangle's corners against nv (mesh_common.h), a CSR segment against its item count, an item against its
// range and an edge's ends against nv: no input makes a kernel read or write outside the caller's buffers.  Every loop has a bound
// taken from the sizes; a segment or an entry that does not belong to the mesh ORs FLAG_BOUND into the caller's flag word.
#include "mesh_common.h"

#include <cmath>

namespace {

constexpr uint32_t PRIORITY_NONE = 0xffffffffu;

// the 32-bit bijection that orders the edges of a round (every step is invertible: xor-shift, multiplication by an odd constant)
__device__ __forceinline__ uint32_t edge_priority(uint32_t x) {
    x ^= x >> 16; x *= 0x7feb352du;
    x ^= x >> 15; x *= 0x846ca68bu;
    return x ^ (x >> 16);
}

__device__ __forceinline__ bool segment_of(const int32_t *__restrict__ offsets, int64_t v, int64_t n_items, int64_t &beg, int64_t &end) {
    beg = offsets[v];
    end = offsets[v + 1];
    return beg >= 0 && beg <= end && end <= n_items;
}

struct P3 {
    double x, y, z;
};

__device__ __forceinline__ P3 load_p3(const float *__restrict__ vertices, int32_t v) {
    return {(double)vertices[(int64_t)v * 3], (double)vertices[(int64_t)v * 3 + 1], (double)vertices[(int64_t)v * 3 + 2]};
}

__device__ __forceinline__ P3 sub(const P3 &a, const P3 &b) { return {a.x - b.x, a.y - b.y, a.z - b.z}; }
__device__ __forceinline__ P3 cross(const P3 &u, const P3 &w) { return {u.y * w.z - u.z * w.y, u.z * w.x - u.x * w.z, u.x * w.y - u.y * w.x}; }
__device__ __forceinline__ double dot(const P3 &a, const P3 &b) { return (a.x * b.x + a.y * b.y) + a.z * b.z; }

// Q += w [p; d][p; d]^T, entry (i, j) = (w * p_i) * p_j: xx xy xz xw yy yz yw zz zw ww
__device__ __forceinline__ void add_plane(double (&Q)[10], const P3 &p, double d, double w) {
    const double wx = w * p.x, wy = w * p.y, wz = w * p.z, wd = w * d;
    Q[0] += wx * p.x; Q[1] += wx * p.y; Q[2] += wx * p.z; Q[3] += wx * d;
    Q[4] += wy * p.y; Q[5] += wy * p.z; Q[6] += wy * d;
    Q[7] += wz * p.z; Q[8] += wz * d;
    Q[9] += wd * d;
}

// the unit normal and the area of (a, b, c); false: no area (or a corner that is not finite)
__device__ __forceinline__ bool unit_normal(const P3 &a, const P3 &b, const P3 &c, P3 &n, double &area) {
    const P3 m = cross(sub(b, a), sub(c, a));
    const double len = sqrt(dot(m, m));
    if (!(len > 0.0) || !finite_f64(len)) return false;
    n = {m.x / len, m.y / len, m.z / len};
    area = 0.5 * len;
    return true;
}

__device__ __forceinline__ bool has_corner(int32_t a, int32_t b, int32_t c, int32_t v) { return a == v || b == v || c == v; }

// the triangles of v's segment [beg, end) that name u
__device__ __forceinline__ int shared_triangles(const int32_t *__restrict__ triangles, int nt, int nv, const int32_t *__restrict__ items, int64_t beg,
                                                int64_t end, int32_t u) {
    int n = 0;
    for (int64_t e = beg; e < end; ++e) {
        const int32_t t = items[e];
        if ((uint32_t)t >= (uint32_t)nt) continue;
        int32_t a, b, c;
        load_corners(triangles, t, a, b, c);
        if (corners_in_mesh(a, b, c, nv) && has_corner(a, b, c, u)) ++n;
    }
    return n;
}

// v is an end of an edge that exactly one triangle uses: some item of its vertex segment [vbeg, vend) shares one triangle with it
__device__ __forceinline__ bool on_boundary(const int32_t *__restrict__ triangles, int nt, int nv, const int32_t *__restrict__ tri_items, int64_t tbeg,
                                            int64_t tend, const int32_t *__restrict__ vert_items, int64_t vbeg, int64_t vend) {
    for (int64_t j = vbeg; j < vend; ++j)
        if (shared_triangles(triangles, nt, nv, tri_items, tbeg, tend, vert_items[j]) == 1) return true;
    return false;
}

// ---------------------------------------------------------------- vertex quadrics
// one lane per vertex: the planes of its triangles in segment order, then the boundary planes in segment order, edge k = (corner k,
// corner k + 1) of each triangle
__global__ __launch_bounds__(256) void quadric_init_kernel(const float *__restrict__ vertices, int nv, const int32_t *__restrict__ triangles, int nt,
                                                           const int32_t *__restrict__ offsets, const int32_t *__restrict__ items, int64_t n_items,
                                                           double boundary_weight, double *__restrict__ quadrics, int32_t *__restrict__ flag) {
    const int64_t v = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (v >= nv) return;
    double Q[10] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    int64_t beg, end;
    if (!segment_of(offsets, v, n_items, beg, end)) { atomicOr(flag, FLAG_BOUND); beg = end = 0; }
    for (int pass = 0; pass < 2; ++pass) {
        for (int64_t e = beg; e < end; ++e) {
            const int32_t t = items[e];
            if ((uint32_t)t >= (uint32_t)nt) { atomicOr(flag, FLAG_BOUND); continue; }
            int32_t idx[3];
            if (!corners_checked(triangles, t, nv, idx[0], idx[1], idx[2], flag)) continue;
            const P3 p[3] = {load_p3(vertices, idx[0]), load_p3(vertices, idx[1]), load_p3(vertices, idx[2])};
            P3 n;
            double area;
            if (!unit_normal(p[0], p[1], p[2], n, area)) continue;
            if (pass == 0) {
                add_plane(Q, n, -dot(n, p[0]), area);
                continue;
            }
#pragma unroll
            for (int k = 0; k < 3; ++k) {
                const int32_t from = idx[k], to = idx[(k + 1) % 3];
                if (from == to || (from != v && to != v)) continue;
                if (shared_triangles(triangles, nt, nv, items, beg, end, from == v ? to : from) != 1) continue;
                const P3 m = cross(sub(p[(k + 1) % 3], p[k]), n);
                const double len = sqrt(dot(m, m));
                if (!(len > 0.0) || !finite_f64(len)) continue;
                const P3 u = {m.x / len, m.y / len, m.z / len};
                add_plane(Q, u, -dot(u, p[k]), boundary_weight * area);
            }
        }
    }
#pragma unroll
    for (int i = 0; i < 10; ++i) quadrics[v * 10 + i] = Q[i];
}

// ---------------------------------------------------------------- edges
// v^T Q v for v = (p, 1)
__device__ __forceinline__ double quadric_value(const double (&Q)[10], const P3 &p) {
    const double sq = (p.x * (Q[0] * p.x) + p.y * (Q[4] * p.y)) + p.z * (Q[7] * p.z);
    const double mixed = (p.x * (Q[1] * p.y) + p.x * (Q[2] * p.z)) + p.y * (Q[5] * p.z);
    const double lin = (Q[3] * p.x + Q[6] * p.y) + Q[8] * p.z;
    return (sq + 2.0 * mixed) + (2.0 * lin + Q[9]);
}

__device__ __forceinline__ double clamped_cost(const double (&Q)[10], const P3 &p) {
    const double c = quadric_value(Q, p);
    return c > 0.0 ? c : (c <= 0.0 ? 0.0 : c);                             // (NaN stays NaN)
}

// the contraction target of the edge (lo, hi) with Q = Q_lo + Q_hi, and its clamped cost
__device__ __forceinline__ P3 contraction_target(const double (&Q)[10], const P3 &lo, const P3 &hi, double &cost) {
    const P3 mid = {(lo.x + hi.x) * 0.5, (lo.y + hi.y) * 0.5, (lo.z + hi.z) * 0.5};
    const double c00 = Q[4] * Q[7] - Q[5] * Q[5], c01 = Q[1] * Q[7] - Q[5] * Q[2], c02 = Q[1] * Q[5] - Q[4] * Q[2];
    const double det = (Q[0] * c00 - Q[1] * c01) + Q[2] * c02;
    const double tr3 = ((Q[0] + Q[4]) + Q[7]) / 3.0;
    if (fabs(det) > 1e-8 * ((tr3 * tr3) * tr3)) {
        const double r0 = -Q[3], r1 = -Q[6], r2 = -Q[8];
        const double dx = (r0 * c00 - Q[1] * (r1 * Q[7] - Q[5] * r2)) + Q[2] * (r1 * Q[5] - Q[4] * r2);
        const double dy = (Q[0] * (r1 * Q[7] - r2 * Q[5]) - r0 * c01) + Q[2] * (Q[1] * r2 - r1 * Q[2]);
        const double dz = (Q[0] * (Q[4] * r2 - Q[5] * r1) - Q[1] * (Q[1] * r2 - Q[2] * r1)) + r0 * c02;
        const P3 s = {dx / det, dy / det, dz / det};
        const P3 off = sub(s, mid), edge = sub(hi, lo);
        if (dot(off, off) <= 4.0 * dot(edge, edge)) {                      // (false for a solution that is not finite)
            cost = clamped_cost(Q, s);
            return s;
        }
    }
    const double cl = clamped_cost(Q, lo), ch = clamped_cost(Q, hi), cm = clamped_cost(Q, mid);
    if (cl <= ch && cl <= cm) { cost = cl; return lo; }
    if (ch <= cm) { cost = ch; return hi; }
    cost = cm;
    return mid;
}

// every triangle of `moved`'s segment that does not name `other` keeps dot(n_before, n_after) > 0 with `moved` at `to`
__device__ __forceinline__ bool keeps_orientation(const float *__restrict__ vertices, int nv, const int32_t *__restrict__ triangles, int nt,
                                                  const int32_t *__restrict__ items, int64_t beg, int64_t end, int32_t moved, int32_t other,
                                                  const P3 &to) {
    for (int64_t e = beg; e < end; ++e) {
        const int32_t t = items[e];
        if ((uint32_t)t >= (uint32_t)nt) return false;
        int32_t a, b, c;
        load_corners(triangles, t, a, b, c);
        if (!corners_in_mesh(a, b, c, nv)) return false;
        if (has_corner(a, b, c, other)) continue;
        const P3 pa = load_p3(vertices, a), pb = load_p3(vertices, b), pc = load_p3(vertices, c);
        const P3 before = cross(sub(pb, pa), sub(pc, pa));
        const P3 qa = a == moved ? to : pa, qb = b == moved ? to : pb, qc = c == moved ? to : pc;
        const P3 after = cross(sub(qb, qa), sub(qc, qa));
        if (!(dot(before, after) > 0.0)) return false;
    }
    return true;
}

__device__ __forceinline__ void sort3(int32_t &a, int32_t &b, int32_t &c) {
    int32_t t;
    if (a > b) { t = a; a = b; b = t; }
    if (b > c) { t = b; b = c; c = t; }
    if (a > b) { t = a; a = b; b = t; }
}

// one lane per edge
__global__ __launch_bounds__(256) void edge_evaluate_kernel(const float *__restrict__ vertices, const float *__restrict__ colors, int nv,
                                                            const int32_t *__restrict__ triangles, int nt, const double *__restrict__ quadrics,
                                                            const int32_t *__restrict__ tri_offsets, const int32_t *__restrict__ tri_items,
                                                            int64_t n_tri_items, const int32_t *__restrict__ vert_offsets,
                                                            const int32_t *__restrict__ vert_items, int64_t n_vert_items,
                                                            const int32_t *__restrict__ edges, int ne, float *__restrict__ cost_out,
                                                            int32_t *__restrict__ removed_out, float *__restrict__ position_out,
                                                            float *__restrict__ color_out, int32_t *__restrict__ flag) {
    const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= ne) return;
    const int32_t lo = edges[e * 2], hi = edges[e * 2 + 1];
    float cost32 = INFINITY, px = NAN, py = NAN, pz = NAN, cr = NAN, cg = NAN, cb = NAN;
    int removed = 0;
    int64_t tlo0, tlo1, thi0, thi1, vlo0, vlo1, vhi0, vhi1;
    if ((uint32_t)lo >= (uint32_t)nv || (uint32_t)hi >= (uint32_t)nv || lo == hi || !segment_of(tri_offsets, lo, n_tri_items, tlo0, tlo1) ||
        !segment_of(tri_offsets, hi, n_tri_items, thi0, thi1) || !segment_of(vert_offsets, lo, n_vert_items, vlo0, vlo1) ||
        !segment_of(vert_offsets, hi, n_vert_items, vhi0, vhi1)) {
        atomicOr(flag, FLAG_BOUND);
    } else {
        double Q[10];
#pragma unroll
        for (int i = 0; i < 10; ++i) Q[i] = quadrics[(int64_t)lo * 10 + i] + quadrics[(int64_t)hi * 10 + i];
        const P3 plo = load_p3(vertices, lo), phi = load_p3(vertices, hi);
        double cost;
        const P3 target = contraction_target(Q, plo, phi, cost);
        px = (float)target.x; py = (float)target.y; pz = (float)target.z;
        if (colors) {
            const P3 edge = sub(phi, plo);
            const double l2 = dot(edge, edge);
            double t = l2 > 0.0 ? dot(sub(target, plo), edge) / l2 : 0.0;
            t = t >= 0.0 ? (t <= 1.0 ? t : 1.0) : 0.0;                     // (NaN: 0)
            const double s = 1.0 - t;
            cr = (float)(s * (double)colors[(int64_t)lo * 3] + t * (double)colors[(int64_t)hi * 3]);
            cg = (float)(s * (double)colors[(int64_t)lo * 3 + 1] + t * (double)colors[(int64_t)hi * 3 + 1]);
            cb = (float)(s * (double)colors[(int64_t)lo * 3 + 2] + t * (double)colors[(int64_t)hi * 3 + 2]);
        }
        removed = shared_triangles(triangles, nt, nv, tri_items, tlo0, tlo1, hi);
        // link, the vertices: the common neighbours of lo and hi (two ascending segments) are as many as the triangles on the edge
        int common = 0;
        for (int64_t i = vlo0, j = vhi0; i < vlo1 && j < vhi1;) {
            const int32_t x = vert_items[i], y = vert_items[j];
            if (x == y) { ++common; ++i; ++j; }
            else if (x < y) ++i;
            else ++j;
        }
        bool legal = removed > 0 && common == removed && (float)cost <= F32_MAX;
        // link, the border: an edge inside the surface does not join two vertices of the border
        if (legal && removed != 1)
            legal = !(on_boundary(triangles, nt, nv, tri_items, tlo0, tlo1, vert_items, vlo0, vlo1) &&
                      on_boundary(triangles, nt, nv, tri_items, thi0, thi1, vert_items, vhi0, vhi1));
        // link, the edges: no triangle of lo without hi becomes, with hi in lo's place, the corner set of a triangle of hi
        for (int64_t i = tlo0; legal && i < tlo1; ++i) {
            const int32_t t = tri_items[i];
            if ((uint32_t)t >= (uint32_t)nt) { legal = false; break; }
            int32_t a, b, c;
            load_corners(triangles, t, a, b, c);
            if (!corners_in_mesh(a, b, c, nv)) { legal = false; break; }
            if (has_corner(a, b, c, hi)) continue;
            a = a == lo ? hi : a; b = b == lo ? hi : b; c = c == lo ? hi : c;
            sort3(a, b, c);
            for (int64_t j = thi0; j < thi1; ++j) {
                const int32_t s = tri_items[j];
                if ((uint32_t)s >= (uint32_t)nt) { legal = false; break; }
                int32_t x, y, z;
                load_corners(triangles, s, x, y, z);
                sort3(x, y, z);
                if (x == a && y == b && z == c) { legal = false; break; }
            }
        }
        if (legal) {
            const P3 to = {(double)px, (double)py, (double)pz};
            legal = keeps_orientation(vertices, nv, triangles, nt, tri_items, tlo0, tlo1, lo, hi, to) &&
                    keeps_orientation(vertices, nv, triangles, nt, tri_items, thi0, thi1, hi, lo, to);
        }
        if (legal) cost32 = (float)cost;
    }
    cost_out[e] = cost32;
    removed_out[e] = removed;
    position_out[e * 3] = px; position_out[e * 3 + 1] = py; position_out[e * 3 + 2] = pz;
    if (color_out) { color_out[e * 3] = cr; color_out[e * 3 + 1] = cg; color_out[e * 3 + 2] = cb; }
}

// ---------------------------------------------------------------- the independent set
// the edge id of entry j of v's segment: edge_of_entry[j] when the item is the higher end, else the entry of v in the item's own
// (ascending) segment, found by bisection; -1: no such entry
__device__ __forceinline__ int32_t edge_of(const int32_t *__restrict__ offsets, const int32_t *__restrict__ items, int64_t n_items,
                                           const int32_t *__restrict__ edge_of_entry, int nv, int32_t v, int64_t j) {
    const int32_t u = items[j];
    if ((uint32_t)u >= (uint32_t)nv || u == v) return -1;
    if (u > v) return edge_of_entry[j];
    int64_t beg, end;
    if (!segment_of(offsets, u, n_items, beg, end)) return -1;
    for (int step = 0; step < 40 && beg < end; ++step) {                   // (a segment has fewer than 2^31 entries)
        const int64_t mid = beg + (end - beg) / 2;
        const int32_t x = items[mid];
        if (x == v) return edge_of_entry[mid];
        if (x < v) beg = mid + 1;
        else end = mid;
    }
    return -1;
}

// p1[v] = the least priority over v's candidate edges (legal, cost <= tau)
__global__ __launch_bounds__(256) void priority_vertex_kernel(int nv, const int32_t *__restrict__ offsets, const int32_t *__restrict__ items,
                                                              int64_t n_items, const int32_t *__restrict__ edge_of_entry,
                                                              const float *__restrict__ cost, int ne, float tau, uint32_t *__restrict__ p1,
                                                              int32_t *__restrict__ flag) {
    const int64_t v = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (v >= nv) return;
    uint32_t best = PRIORITY_NONE;
    int64_t beg, end;
    if (!segment_of(offsets, v, n_items, beg, end)) { atomicOr(flag, FLAG_BOUND); beg = end = 0; }
    for (int64_t j = beg; j < end; ++j) {
        const int32_t e = edge_of(offsets, items, n_items, edge_of_entry, nv, (int32_t)v, j);
        if ((uint32_t)e >= (uint32_t)ne) { atomicOr(flag, FLAG_BOUND); continue; }
        if (cost[e] <= tau) best = min(best, edge_priority((uint32_t)e));
    }
    p1[v] = best;
}

// p2[v] = min(p1[v], p1 of v's neighbours)
__global__ __launch_bounds__(256) void priority_ring_kernel(int nv, const int32_t *__restrict__ offsets, const int32_t *__restrict__ items,
                                                            int64_t n_items, const uint32_t *__restrict__ p1, uint32_t *__restrict__ p2) {
    const int64_t v = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (v >= nv) return;
    uint32_t best = p1[v];
    int64_t beg, end;
    if (segment_of(offsets, v, n_items, beg, end)) {
        for (int64_t j = beg; j < end; ++j) {
            const int32_t u = items[j];
            if ((uint32_t)u < (uint32_t)nv) best = min(best, p1[u]);
        }
    }
    p2[v] = best;
}

// key[e] = (cost bits << 32) | priority for a selected edge, else -1
__global__ __launch_bounds__(256) void edge_select_kernel(const int32_t *__restrict__ edges, int ne, int nv, const float *__restrict__ cost, float tau,
                                                          const uint32_t *__restrict__ p2, int64_t *__restrict__ key_out) {
    const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= ne) return;
    const int32_t lo = edges[e * 2], hi = edges[e * 2 + 1];
    const float c = cost[e];
    int64_t key = -1;
    if ((uint32_t)lo < (uint32_t)nv && (uint32_t)hi < (uint32_t)nv && c <= tau && c >= 0.0f) {
        const uint32_t p = edge_priority((uint32_t)e);
        if (p == p2[lo] && p == p2[hi]) key = (int64_t)(((uint64_t)__float_as_uint(c) << 32) | (uint64_t)p);
    }
    key_out[e] = key;
}

// ---------------------------------------------------------------- apply
// one lane per chosen edge: lo takes the new position, colour and Q_lo + Q_hi; hi is dropped and merged into lo; the triangles
// that name both are dropped.  The chosen edges are independent (no vertex of one is a neighbour of another's): no two lanes touch
// one vertex or one triangle.
__global__ __launch_bounds__(256) void collapse_apply_kernel(float *__restrict__ vertices, float *__restrict__ colors, double *__restrict__ quadrics,
                                                             int nv, const int32_t *__restrict__ triangles, int nt,
                                                             const int32_t *__restrict__ tri_offsets, const int32_t *__restrict__ tri_items,
                                                             int64_t n_tri_items, const int32_t *__restrict__ edges,
                                                             const float *__restrict__ position, const float *__restrict__ color, int ne,
                                                             const int32_t *__restrict__ chosen, int m, int32_t *__restrict__ merge,
                                                             int32_t *__restrict__ vertex_keep, int32_t *__restrict__ triangle_keep,
                                                             int32_t *__restrict__ flag) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= m) return;
    const int32_t e = chosen[i];
    if ((uint32_t)e >= (uint32_t)ne) { atomicOr(flag, FLAG_BOUND); return; }
    const int32_t lo = edges[(int64_t)e * 2], hi = edges[(int64_t)e * 2 + 1];
    int64_t beg, end;
    if ((uint32_t)lo >= (uint32_t)nv || (uint32_t)hi >= (uint32_t)nv || lo == hi || !segment_of(tri_offsets, lo, n_tri_items, beg, end)) {
        atomicOr(flag, FLAG_BOUND);
        return;
    }
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        vertices[(int64_t)lo * 3 + k] = position[(int64_t)e * 3 + k];
        if (colors) colors[(int64_t)lo * 3 + k] = color[(int64_t)e * 3 + k];
    }
#pragma unroll
    for (int k = 0; k < 10; ++k) quadrics[(int64_t)lo * 10 + k] = quadrics[(int64_t)lo * 10 + k] + quadrics[(int64_t)hi * 10 + k];
    merge[hi] = lo;
    vertex_keep[hi] = 0;
    for (int64_t j = beg; j < end; ++j) {
        const int32_t t = tri_items[j];
        if ((uint32_t)t >= (uint32_t)nt) { atomicOr(flag, FLAG_BOUND); continue; }
        int32_t a, b, c;
        load_corners(triangles, t, a, b, c);
        if (has_corner(a, b, c, hi)) triangle_keep[t] = 0;
    }
}

bool csr_args_ok(const int32_t *offsets, const int32_t *items, int64_t n_items, int32_t nt, int per_triangle) {
    return offsets && items && n_items >= 1 && n_items <= (int64_t)per_triangle * nt;
}

}  // namespace

extern "C" int sgam_mesh_quadric_init_f64(const float *vertices, int32_t nv, const int32_t *triangles, int32_t nt, const int32_t *tri_offsets,
                                          const int32_t *tri_items, int64_t n_tri_items, double boundary_weight, double *quadrics_out,
                                          int32_t *flag, void *stream) {
    if (!mesh_args_ok(vertices, nv, triangles, nt, flag) || !csr_args_ok(tri_offsets, tri_items, n_tri_items, nt, 3) || !quadrics_out ||
        !finite_f64(boundary_weight) || boundary_weight < 0.0)
        return SGAM_EINVAL;
    SGAM_KLAUNCH(quadric_init_kernel, dim3(blocks_of(nv)), dim3(256), 0, sgam_stream(stream), vertices, nv, triangles, nt, tri_offsets, tri_items,
                 n_tri_items, boundary_weight, quadrics_out, flag);
    SGAM_LAUNCH_CHECK();
    return SGAM_OK;
}

extern "C" int sgam_mesh_collapse_evaluate_f64(const float *vertices, const float *colors, int32_t nv, const int32_t *triangles, int32_t nt,
                                               const double *quadrics, const int32_t *tri_offsets, const int32_t *tri_items, int64_t n_tri_items,
                                               const int32_t *vert_offsets, const int32_t *vert_items, int64_t n_vert_items, const int32_t *edges,
                                               int32_t ne, float *cost_out, int32_t *removed_out, float *position_out, float *color_out,
                                               int32_t *flag, void *stream) {
    if (!mesh_args_ok(vertices, nv, triangles, nt, flag) || !quadrics || !csr_args_ok(tri_offsets, tri_items, n_tri_items, nt, 3) ||
        !csr_args_ok(vert_offsets, vert_items, n_vert_items, nt, 6) || !edges || ne < 1 || 2 * (int64_t)ne > n_vert_items || !cost_out ||
        !removed_out || !position_out || (colors != nullptr) != (color_out != nullptr))
        return SGAM_EINVAL;
    SGAM_KLAUNCH(edge_evaluate_kernel, dim3(blocks_of(ne)), dim3(256), 0, sgam_stream(stream), vertices, colors, nv, triangles, nt, quadrics,
                 tri_offsets, tri_items, n_tri_items, vert_offsets, vert_items, n_vert_items, edges, ne, cost_out, removed_out, position_out,
                 color_out, flag);
    SGAM_LAUNCH_CHECK();
    return SGAM_OK;
}

extern "C" int64_t sgam_mesh_collapse_workspace_bytes(int32_t nv) {
    if (nv < 1) return SGAM_EINVAL;
    return 2 * r16(4 * (int64_t)nv);
}

extern "C" int sgam_mesh_collapse_select_i32(int32_t nv, const int32_t *vert_offsets, const int32_t *vert_items, int64_t n_vert_items,
                                             const int32_t *edge_of_entry, const int32_t *edges, const float *cost, int32_t ne, float tau,
                                             void *workspace, int64_t workspace_bytes, int64_t *key_out, int32_t *flag, void *stream) {
    if (nv < 1 || !vert_offsets || !vert_items || n_vert_items < 1 || n_vert_items >= ((int64_t)1 << 31) || !edge_of_entry || !edges || !cost ||
        ne < 1 || 2 * (int64_t)ne > n_vert_items || !(tau >= 0.0f && tau <= F32_MAX) || !key_out || !flag)
        return SGAM_EINVAL;
    if (!workspace_fits(workspace, workspace_bytes, sgam_mesh_collapse_workspace_bytes(nv))) return SGAM_EINVAL;
    uint32_t *p1 = (uint32_t *)workspace, *p2 = (uint32_t *)((char *)workspace + r16(4 * (int64_t)nv));
    hipStream_t s = sgam_stream(stream);
    SGAM_KLAUNCH(priority_vertex_kernel, dim3(blocks_of(nv)), dim3(256), 0, s, nv, vert_offsets, vert_items, n_vert_items, edge_of_entry, cost, ne,
                 tau, p1, flag);
    SGAM_KLAUNCH(priority_ring_kernel, dim3(blocks_of(nv)), dim3(256), 0, s, nv, vert_offsets, vert_items, n_vert_items, p1, p2);
    SGAM_KLAUNCH(edge_select_kernel, dim3(blocks_of(ne)), dim3(256), 0, s, edges, ne, nv, cost, tau, p2, key_out);
    SGAM_LAUNCH_CHECK();
    return SGAM_OK;
}

extern "C" int sgam_mesh_collapse_apply_f64(float *vertices, float *colors, double *quadrics, int32_t nv, const int32_t *triangles, int32_t nt,
                                            const int32_t *tri_offsets, const int32_t *tri_items, int64_t n_tri_items, const int32_t *edges,
                                            const float *position, const float *color, int32_t ne, const int32_t *chosen, int32_t m,
                                            int32_t *merge, int32_t *vertex_keep, int32_t *triangle_keep, int32_t *flag, void *stream) {
    if (!mesh_args_ok(vertices, nv, triangles, nt, flag) || !quadrics || !csr_args_ok(tri_offsets, tri_items, n_tri_items, nt, 3) || !edges ||
        !position || (colors != nullptr) != (color != nullptr) || ne < 1 || !chosen || m < 1 || m > ne || !merge || !vertex_keep ||
        !triangle_keep)
        return SGAM_EINVAL;
    SGAM_KLAUNCH(collapse_apply_kernel, dim3(blocks_of(m)), dim3(256), 0, sgam_stream(stream), vertices, colors, quadrics, nv, triangles, nt,
                 tri_offsets, tri_items, n_tri_items, edges, position, color, ne, chosen, m, merge, vertex_keep, triangle_keep, flag);
    SGAM_LAUNCH_CHECK();
    return SGAM_OK;
}
