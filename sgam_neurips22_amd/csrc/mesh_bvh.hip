// mesh_bvh.hip — a bounding-volume hierarchy over the candidate triangles of a mesh (vertices [nv][3] fp32, triangles [nt][3] int32),
// built on the device (sgam_mesh_bvh_keys, sgam_mesh_bvh_build) and walked by the three queries the grid serves: the exact distance
// from a point (sgam_mesh_distance_bvh_f32), the nearest / any hit of a ray (sgam_mesh_raycast_bvh_f32) and the visibility of points
// from pinhole cameras (sgam_mesh_visibility_bvh_f32).  Its cost does not depend on the triangles being near one scale: a triangle
// is ONE leaf however many cells of a grid it would span.  The arithmetic of a triangle is mesh_rules.h's, the one the brute-force
// and grid kernels run, and every triangle of a visited leaf goes to the same sink, so the answers are the brute-force answers in
// every bit as long as no node that holds the winner (or a tie with it) is skipped: the two PRUNING RULES below are the whole
// argument.  points_common.h's rules hold: every fp32 operator is ONE IEEE operation in the written order (built with
// -ffp-contract=off, the operations spelled out).  tests/bvh_oracle.py restates everything in numpy.  DESIGN §4.4.10.
//
// CANDIDATES are mesh_common.h's (finite corners, dot(n, n) > 0); a triangle that names a vertex outside [0, nv) ORs FLAG_INDEX into
// the flag word and is skipped.  n = their number.
//
// KEY (sgam_mesh_bvh_keys, one lane per triangle).  The caller passes the box [lo, hi] of the candidates' corners.  Per axis j:
//     c = 0.5 * min_j + 0.5 * max_j        (min / max over the three corners; two products, one sum)
//     s = (c - lo_j) / (hi_j - lo_j)       (one difference each, one division)
//     q = s >= 0 ? min(floor(s * 2048), 2047) : 0        (NaN — a box without extent — gives 0)
// code = the 33-bit Morton interleave, bit i of q_x at 3 i + 2, of q_y at 3 i + 1, of q_z at 3 i; key = (code << 28) | t, t the
// triangle's index (< 2^28 = MAX_TRIANGLES): 61 bits, a non-negative int64, UNIQUE.  What is not a candidate gets INT64_MAX and
// sorts last; count_out = the candidates.  The caller sorts the keys (integer plumbing); the order is a pure function of the keys,
// and the index is read back from a key's low bits, so no permutation is carried along.  The key decides only the SHAPE of the
// tree, never an answer.
//
// HIERARCHY (sgam_mesh_bvh_build; Karras, "Maximizing Parallelism in the Construction of BVHs, Octrees, and k-d Trees", 2012).  The
// leaves are the n sorted candidates, stored as TRIANGLE_RECORD records (nine coordinates and the id, 48 B: a leaf is one contiguous
// read, the grid's record).  Internal node i of 0 .. n - 2 finds, from the sorted keys alone, delta(a, b) = clz(key_a ^ key_b)
// (-1 outside [0, n)): its direction d = sign(delta(i, i + 1) - delta(i, i - 1)), its range's other end j by doubling and then
// halving steps while delta(i, .) > delta(i, i - d), and its split by halving steps while delta(i, .) > delta(i, j).  Node 0 is the
// root.  The nodes are independent: nothing is handed between lanes.  Nodes are numbered in one space: internal i is i, leaf k is
// n - 1 + k; children [i] = (left, right).  A child's common prefix is longer than its parent's and prefixes have 3 .. 63 bits, so
// the HEIGHT is at most 61, the key width: the bound of the traversal stack and of the box rounds.  n = 1 is a single leaf (node
// 0) and no internal node.
//
// BOXES.  boxes [2 n - 1][6] = (lo, hi) per node: a leaf's is min / max of its three corners, an internal node's min / max of its
// children's — comparisons only, no rounding enters, so a node's box is EXACTLY the box of its leaves' corners.  They are filled
// by ONE LAUNCH PER ROUND: in round r = 1, 2, ... a node whose two children were ready before the launch (a leaf, or ready[child]
// in 1 .. r - 1) computes its box and sets ready[i] = r; a ready[child] it reads while that child's lane writes it is 0 or r, "not
// ready" either way, so the outcome does not depend on timing, and a box is only read in a later launch than the one that wrote
// it: the launch boundary is the only visibility the pass needs.  Chosen over the atomic-counter bottom-up pass because it needs
// no fence, no agent-scope atomics and no reasoning about the per-XCD L2s — the alternative saves launches (min(61, n - 1) short
// ones here, a few microseconds each), not work.  ready[i] ends as node i's height; ready[0] is the tree's.  A node that is not
// ready in the last round raises FLAG_BOUND (never, by the height bound).
//
// TRAVERSAL: one lane per query or ray (as in the grid's ray kernel).  An explicit stack of node indices with the `near` value each
// was pushed with, 64 entries (> the height bound 61: a pop pushes at most two and every level of the path holds at most one
// pending sibling), in PRIVATE memory: 2 x 256 B of scratch per lane, addressed dynamically, so it costs scratch traffic (cached in
// L1 / L2) but neither LDS nor registers — in LDS it would be 128 KB per workgroup of 256 lanes and hold a CU to one workgroup.
// (As built: 58 - 68 VGPRs and 528 B of scratch per lane, 7 - 8 waves per SIMD.)
// A popped internal node tests both children's boxes against the current best, pushes those that pass, the nearer one on top (so
// it is visited first); a popped node is tested once more against the best of that moment — the same test: only `best` moved.
// Every node is pushed at most once, so the loop is bounded by 2 n - 1 pops; running into that bound, a child index outside the
// tree or a full stack raises FLAG_BOUND and ends the walk (tables that are not this tree's; reads stay inside the workspace).
//
// PRUNING, DISTANCE.  m = sqrt(dot(e, e)), e_j = max(max(lo_j - q_j, q_j - hi_j), 0): the fp32 distance from q to the node's box;
//     ms = (m - margin) * (1 - 2^-14);   SKIP iff ms > 0 and (best < ms * ms or ms * ms > max_d2)
// margin = 2^-14 * (the largest |coordinate| of the candidates' box + its longest edge): mesh_query.hip's stop rule with the node's
// box in place of the visited block.  Why no winner is skipped: every point of every triangle of the node lies in its box, so the
// true distance D of each is >= the true distance to the box, which is >= m (1 - 2^-21) (three roundings of differences, three of
// the dot product, one of the root, all relative; an underflow only lowers m).  A computed point-triangle distance differs from D
// by at most K 2^-23 (D + scale), K measured 2.32 and covered up to 2^8 (mesh_query.hip): it is >= D (1 - 2^-15) -
// 2^-15 scale > (m - 2^-14 scale) (1 - 2^-14) >= ms, with 2^-15 relative to spare for the rounding of ms and ms * ms.  So a
// skipped node's triangles all have d2 > best (they neither win nor tie: the compare is strict) or d2 > max_d2.
//
// PRUNING, RAYS.  A hit of a triangle T of the node at the fp32 parameter t has, by the guard of the intersection rule,
// fl(min_T - guard) <= P_j(t) <= fl(max_T + guard) on every axis j, P_j(t) = fl(o_j + fl(t * d_j)); x -> fl(x - guard) is monotone
// and the node's box holds T's corners, so L_j <= P_j(t) <= H_j with L_j = fl(lo_j - guard), H_j = fl(hi_j + guard).  The test must
// accept whenever such a t exists in the window [tnear, min(tfar, best)].  Per axis:
//     M = max(|L|, |H|)    E = (|o| + M) * 2^-21 + 2^-100    A = L - E    B = H + E
//     d = 0 (or -0):  the axis passes iff A <= o <= B
//     otherwise:      s1 = (A - o) / d    s2 = (B - o) / d    lo = min(s1, s2)    hi = max(s1, s2)
//                     lo' = lo - (|lo| * 2^-21 + 2^-100)    hi' = hi + (|hi| * 2^-21 + 2^-100)
// enter = max(tnear, the lo' of the axes with d != 0), exit = min(window's end, the hi'); ACCEPT iff every axis with d = 0 passes
// and not (enter > exit); min and max are fminf / fmaxf, which drop a NaN (inf - inf), i.e. drop that constraint.  Proof that a
// node with a hit is accepted, in exact arithmetic over the computed numbers, no measured constant:
//   - P = fl(o + y), y = fl(t d) = t d (1 + e1) + u1, |e1| <= 2^-24, |u1| <= 2^-150, and a sum has only a relative error: the real
//     point r = o + t d has |r - P| <= 2^-24 |P| / (1 - 2^-24) + 2^-24 |t d| + 2^-150 and |t d| <= |o| + |r|, hence |r - P| <= 2^-22
//     (|o| + |P|) + 2^-140 =: E0, and |P| <= M.  The computed E (a sum, a product by a power of two, a sum: two relative roundings
//     and an underflow) is at least E0 + 2^-22 (|o| + M) (1 - 2^-21) + 2^-101, and the roundings of fl(L - E), fl(H + E) are at most
//     2^-24 (M + E), which is less than E - E0: A <= L - E0 <= r <= H + E0 <= B.  With d = 0, t d = +-0 and P = o itself.
//   - r = o + t d in [A, B] puts t between the real quotients (A - o) / d and (B - o) / d; a computed quotient s has the relative
//     error of one difference and one division and an underflow, |s - real| <= 2^-22 |s| + 2^-149, and lo', hi' move by at least
//     |s| 2^-21 (1 - 2^-23) + 2^-101 less one rounding of 2^-24 (|s| (1 + 2^-20) + 2^-99): more.  An overflow gives +-inf on the
//     side that only widens, or a NaN that drops the constraint.  So lo' <= t <= hi' on every axis with d != 0, tnear <= t <= the
//     window's end, enter <= t <= exit: accepted.
// The nearest-hit walk prunes with best in the window's end: t <= best, not <, so a node that holds an exact tie with the held
// winner is still visited and the lower index wins.  The any-hit walk leaves at the first hit.
#include "mesh_rules.h"

#include <algorithm>
#include <type_traits>

namespace {

constexpr int BVH_KEY_BITS = 61;              // 33 bits of Morton code above 28 bits of triangle index
constexpr int BVH_STACK = 64;                 // > the height bound BVH_KEY_BITS
constexpr int64_t BVH_ID_MASK = ((int64_t)1 << 28) - 1;
constexpr int64_t BVH_NO_KEY = 0x7fffffffffffffffll;

struct Box6 {
    float lx, ly, lz, hx, hy, hz;
};

// the tree inside a caller's workspace
struct Bvh {
    float4 *records;          // [n] x 3
    float *boxes;             // [2 n - 1][6]
    int2 *children;           // [max(n - 1, 1)]
    int32_t *ready;           // [max(n - 1, 1)]
    int n;
};

__device__ __forceinline__ Box6 load_box(const float *__restrict__ boxes, int c) {
    const float2 *__restrict__ p = (const float2 *)(boxes + (int64_t)c * 6);
    const float2 a = p[0], b = p[1], d = p[2];
    return {a.x, a.y, b.x, b.y, d.x, d.y};
}

__device__ __forceinline__ void store_box(float *__restrict__ boxes, int c, const Box6 &b) {
    float2 *__restrict__ p = (float2 *)(boxes + (int64_t)c * 6);
    p[0] = make_float2(b.lx, b.ly); p[1] = make_float2(b.lz, b.hx); p[2] = make_float2(b.hy, b.hz);
}

// ---------------------------------------------------------------- keys
__device__ __forceinline__ uint32_t morton_axis(float mn, float mx, float lo, float hi) {
    const float c = __fadd_rn(__fmul_rn(0.5f, mn), __fmul_rn(0.5f, mx));
    const float s = __fdiv_rn(__fsub_rn(c, lo), __fsub_rn(hi, lo));
    return s >= 0.0f ? (uint32_t)fminf(floorf(__fmul_rn(s, 2048.0f)), 2047.0f) : 0u;
}

__global__ __launch_bounds__(256) void mesh_bvh_keys_kernel(const float *__restrict__ vertices, int nv, const int32_t *__restrict__ triangles, int nt,
                                                            Box6 box, int64_t *__restrict__ keys, unsigned long long *__restrict__ count,
                                                            int32_t *__restrict__ flag) {
    const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= nt) return;
    Tri T;
    if (!load_tri(vertices, nv, triangles, t, T, flag) || !is_candidate(T)) { keys[t] = BVH_NO_KEY; return; }
    const uint32_t qx = morton_axis(fminf(fminf(T.ax, T.bx), T.cx), fmaxf(fmaxf(T.ax, T.bx), T.cx), box.lx, box.hx);
    const uint32_t qy = morton_axis(fminf(fminf(T.ay, T.by), T.cy), fmaxf(fmaxf(T.ay, T.by), T.cy), box.ly, box.hy);
    const uint32_t qz = morton_axis(fminf(fminf(T.az, T.bz), T.cz), fmaxf(fmaxf(T.az, T.bz), T.cz), box.lz, box.hz);
    uint64_t code = 0;
#pragma unroll
    for (int i = 0; i < 11; ++i)
        code |= ((uint64_t)((qx >> i) & 1u) << (3 * i + 2)) | ((uint64_t)((qy >> i) & 1u) << (3 * i + 1)) | ((uint64_t)((qz >> i) & 1u) << (3 * i));
    keys[t] = (int64_t)((code << 28) | (uint64_t)t);
    atomicAdd(count, 1ull);
}

// ---------------------------------------------------------------- leaves, hierarchy, boxes
// leaf k = the candidate of sorted key k: its record and its box (a key that is not one of this mesh's: NaN record, empty box, flag)
__global__ __launch_bounds__(256) void mesh_bvh_leaves_kernel(const float *__restrict__ vertices, int nv, const int32_t *__restrict__ triangles, int nt,
                                                              const int64_t *__restrict__ sorted, Bvh B, int32_t *__restrict__ flag) {
    const int64_t k = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= B.n) return;
    const int64_t key = sorted[k];
    const int64_t id = key & BVH_ID_MASK;
    const float nan = __uint_as_float(0x7fc00000u), inf = __uint_as_float(0x7f800000u);
    Tri T = {nan, nan, nan, nan, nan, nan, nan, nan, nan};
    Box6 b = {inf, inf, inf, -inf, -inf, -inf};
    const bool ok = key >= 0 && (key >> BVH_KEY_BITS) == 0 && id < nt && load_tri(vertices, nv, triangles, id, T, flag) && is_candidate(T);
    if (ok) {
        b = {fminf(fminf(T.ax, T.bx), T.cx), fminf(fminf(T.ay, T.by), T.cy), fminf(fminf(T.az, T.bz), T.cz),
             fmaxf(fmaxf(T.ax, T.bx), T.cx), fmaxf(fmaxf(T.ay, T.by), T.cy), fmaxf(fmaxf(T.az, T.bz), T.cz)};
    } else {
        T = {nan, nan, nan, nan, nan, nan, nan, nan, nan};
        atomicOr(flag, FLAG_BOUND);
    }
    B.records[k * 3] = make_float4(T.ax, T.ay, T.az, __int_as_float((int)id));
    B.records[k * 3 + 1] = make_float4(T.bx, T.by, T.bz, 0.0f);
    B.records[k * 3 + 2] = make_float4(T.cx, T.cy, T.cz, 0.0f);
    store_box(B.boxes, B.n - 1 + (int)k, b);
}

// delta(i, j) of the header: the common prefix of keys i and j, -1 when j lies outside the keys
__device__ __forceinline__ int key_delta(const int64_t *__restrict__ sorted, int n, uint64_t ki, int64_t j) {
    if (j < 0 || j >= n) return -1;
    const uint64_t x = ki ^ (uint64_t)sorted[j];
    return x ? __clzll((long long)x) : 64;
}

// internal node i: its two children from the sorted keys (Karras 2012, figure 4); every loop bounded by the bits of n
__global__ __launch_bounds__(256) void mesh_bvh_hierarchy_kernel(const int64_t *__restrict__ sorted, Bvh B, int32_t *__restrict__ flag) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int n = B.n;
    if (i >= n - 1) return;
    const uint64_t ki = (uint64_t)sorted[i];
    const int d = key_delta(sorted, n, ki, i + 1) > key_delta(sorted, n, ki, i - 1) ? 1 : -1;
    const int dmin = key_delta(sorted, n, ki, i - d);
    int64_t lmax = 2;
    int rounds = 0;
    while (key_delta(sorted, n, ki, i + lmax * d) > dmin) {                  // (delta is -1 beyond the keys: lmax < 2 n)
        lmax <<= 1;
        if (++rounds > 32) { atomicOr(flag, FLAG_BOUND); break; }
    }
    int64_t l = 0;
    for (int64_t t = lmax >> 1; t >= 1; t >>= 1)
        if (key_delta(sorted, n, ki, i + (l + t) * d) > dmin) l += t;
    const int64_t j = i + l * d;
    const int dnode = key_delta(sorted, n, ki, j);
    int64_t s = 0, t = l;
    for (rounds = 0; rounds < 34; ++rounds) {                                // t halves, rounded up, until it was 1
        t = (t + 1) >> 1;
        if (key_delta(sorted, n, ki, i + (s + t) * d) > dnode) s += t;
        if (t <= 1) break;
    }
    if (l < 1 || rounds >= 34) atomicOr(flag, FLAG_BOUND);                   // (keys that are not sorted and unique)
    int64_t g = i + s * d + (d < 0 ? -1 : 0);
    g = g < 0 ? 0 : g > n - 2 ? n - 2 : g;                                   // (inside the tree whatever the keys were)
    const int64_t first = i < j ? i : j, last = i < j ? j : i;
    B.children[i] = make_int2(first == g ? n - 1 + (int)g : (int)g, last == g + 1 ? n - 1 + (int)(g + 1) : (int)(g + 1));
    B.ready[i] = 0;
}

// one round of the header's box pass
__global__ __launch_bounds__(256) void mesh_bvh_boxes_kernel(Bvh B, int round, int last, int32_t *__restrict__ flag) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int n = B.n;
    if (i >= n - 1 || B.ready[i] != 0) return;
    const int2 ch = B.children[i];
    bool ok = (uint32_t)ch.x < (uint32_t)(2 * n - 1) && (uint32_t)ch.y < (uint32_t)(2 * n - 1);
    if (ok && ch.x < n - 1) { const int r = B.ready[ch.x]; ok = r > 0 && r < round; }
    if (ok && ch.y < n - 1) { const int r = B.ready[ch.y]; ok = r > 0 && r < round; }
    if (!ok) {
        if (round == last) atomicOr(flag, FLAG_BOUND);
        return;
    }
    const Box6 a = load_box(B.boxes, ch.x), b = load_box(B.boxes, ch.y);
    store_box(B.boxes, (int)i, {fminf(a.lx, b.lx), fminf(a.ly, b.ly), fminf(a.lz, b.lz), fmaxf(a.hx, b.hx), fmaxf(a.hy, b.hy), fmaxf(a.hz, b.hz)});
    B.ready[i] = round;
}

// ---------------------------------------------------------------- the two node tests (the header's pruning rules)
constexpr float BVH_REL = 4.76837158203125e-7f;          // 2^-21
constexpr float BVH_ABS = 7.888609052210118e-31f;        // 2^-100

// the header's distance rule; false: skip the node; lb = ms * ms (0 while ms <= 0)
__device__ __forceinline__ bool distance_node(const Box6 &b, float qx, float qy, float qz, float margin, float max_d2, float best, float &lb) {
    const float ex = fmaxf(fmaxf(__fsub_rn(b.lx, qx), __fsub_rn(qx, b.hx)), 0.0f);
    const float ey = fmaxf(fmaxf(__fsub_rn(b.ly, qy), __fsub_rn(qy, b.hy)), 0.0f);
    const float ez = fmaxf(fmaxf(__fsub_rn(b.lz, qz), __fsub_rn(qz, b.hz)), 0.0f);
    const float m = sqrt_rn(dot3(ex, ey, ez, ex, ey, ez));
    const float ms = __fmul_rn(__fsub_rn(m, margin), 0.99993896484375f);
    lb = ms > 0.0f ? __fmul_rn(ms, ms) : 0.0f;
    return !(ms > 0.0f && (best < lb || lb > max_d2));
}

// one axis of the header's ray rule; false: the axis has d = 0 and o lies outside [A, B]
__device__ __forceinline__ bool ray_axis(float lo, float hi, float o, float d, float guard, float &enter, float &exit) {
    const float L = __fsub_rn(lo, guard), H = __fadd_rn(hi, guard);
    const float M = fmaxf(fabsf(L), fabsf(H));
    const float E = __fadd_rn(__fmul_rn(__fadd_rn(fabsf(o), M), BVH_REL), BVH_ABS);
    const float A = __fsub_rn(L, E), B = __fadd_rn(H, E);
    if (d == 0.0f) return (o >= A) & (o <= B);
    const float s1 = __fdiv_rn(__fsub_rn(A, o), d), s2 = __fdiv_rn(__fsub_rn(B, o), d);
    const float a = fminf(s1, s2), b = fmaxf(s1, s2);
    enter = fmaxf(enter, __fsub_rn(a, __fadd_rn(__fmul_rn(fabsf(a), BVH_REL), BVH_ABS)));
    exit = fminf(exit, __fadd_rn(b, __fadd_rn(__fmul_rn(fabsf(b), BVH_REL), BVH_ABS)));
    return true;
}

// the header's ray rule against the window [tnear, tend]; false: skip the node; enter: where the ray may first be inside
__device__ __forceinline__ bool ray_node(const Box6 &b, const Ray &r, float guard, float tnear, float tend, float &enter) {
    float exit = tend;
    enter = tnear;
    const bool okx = ray_axis(b.lx, b.hx, r.ox, r.dx, guard, enter, exit), oky = ray_axis(b.ly, b.hy, r.oy, r.dy, guard, enter, exit),
               okz = ray_axis(b.lz, b.hz, r.oz, r.dz, guard, enter, exit);
    return okx && oky && okz && !(enter > exit);
}

// ---------------------------------------------------------------- what is walked for: a point's distance, a ray's hits
__device__ __forceinline__ Tri record_tri(const float4 *__restrict__ records, int k, int &id) {
    const float4 a = records[(int64_t)k * 3], b = records[(int64_t)k * 3 + 1], c = records[(int64_t)k * 3 + 2];
    id = __float_as_int(a.w);
    return {a.x, a.y, a.z, b.x, b.y, b.z, c.x, c.y, c.z};
}

struct DistanceWalk {
    float qx, qy, qz, margin, max_d2;
    MeshSink sink;
    __device__ __forceinline__ bool test(const Box6 &b, float &near) const { return distance_node(b, qx, qy, qz, margin, max_d2, sink.best, near); }
    __device__ __forceinline__ bool still(float near) const { return !(sink.best < near); }
    __device__ __forceinline__ bool leaf(const float4 *__restrict__ records, int k) {
        int id, region;
        float x, y, z;
        const Tri T = record_tri(records, k, id);
        const float d2 = point_triangle(T, qx, qy, qz, x, y, z, region);
        sink.offer(d2, id, max_d2, x, y, z);
        return false;
    }
};

__device__ __forceinline__ float window_end(const NearestSink &s, float tfar) { return fminf(tfar, s.best); }
__device__ __forceinline__ float window_end(const AnySink &, float tfar) { return tfar; }

template <class Sink>
struct RayWalk {
    Ray r;
    Window w;
    Sink sink;
    __device__ __forceinline__ bool test(const Box6 &b, float &near) const { return ray_node(b, r, w.guard, w.tnear, window_end(sink, w.tfar), near); }
    __device__ __forceinline__ bool still(float near) const { return !(near > window_end(sink, w.tfar)); }
    __device__ __forceinline__ bool leaf(const float4 *__restrict__ records, int k) {
        int id;
        float t, u, v;
        const Tri T = record_tri(records, k, id);
        const bool hit = ray_triangle(T, r, w, t, u, v);
        sink.offer(hit, t, u, v, id, k);
        return sink.full();
    }
};

// the header's traversal; false: it ran into a bound (tables that are not this tree's)
template <class Walk>
__device__ __forceinline__ bool bvh_walk(const Bvh &B, Walk &q) {
    int stack[BVH_STACK];
    float nears[BVH_STACK];
    const int total = 2 * B.n - 1, first_leaf = B.n - 1;
    int sp = 0;
    float near;
    if (q.test(load_box(B.boxes, 0), near)) { stack[0] = 0; nears[0] = near; sp = 1; }
    for (int pops = 0; pops < total && sp > 0; ++pops) {
        --sp;
        const int c = stack[sp];
        if (!q.still(nears[sp])) continue;
        if (c >= first_leaf) {
            if (q.leaf(B.records, c - first_leaf)) return true;
            continue;
        }
        const int2 ch = B.children[c];
        if ((uint32_t)ch.x >= (uint32_t)total || (uint32_t)ch.y >= (uint32_t)total || sp + 2 > BVH_STACK) return false;
        float nl, nr;
        const bool pl = q.test(load_box(B.boxes, ch.x), nl), pr = q.test(load_box(B.boxes, ch.y), nr);
        const bool right_first = pl & pr & (nr < nl);                         // the nearer child on top; equal: the left one
        if (pl & pr) {
            stack[sp] = right_first ? ch.x : ch.y; nears[sp] = right_first ? nl : nr; ++sp;
            stack[sp] = right_first ? ch.y : ch.x; nears[sp] = right_first ? nr : nl; ++sp;
        } else if (pl | pr) {
            stack[sp] = pl ? ch.x : ch.y; nears[sp] = pl ? nl : nr; ++sp;
        }
    }
    return sp == 0;
}

__global__ __launch_bounds__(256) void mesh_distance_bvh_kernel(Bvh B, const float *__restrict__ query, int Nq, float margin, float max_d2,
                                                                float *__restrict__ d2_out, int32_t *__restrict__ tri_out,
                                                                float *__restrict__ closest, int32_t *__restrict__ flag) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= Nq) return;                                                      // (no barrier below)
    DistanceWalk q = {query[i * 3], query[i * 3 + 1], query[i * 3 + 2], margin, max_d2, MeshSink()};
    if (finite3(q.qx, q.qy, q.qz) && !bvh_walk(B, q)) atomicOr(flag, FLAG_BOUND);
    q.sink.write(i, d2_out, tri_out, closest);
}

template <int MODE>
__global__ __launch_bounds__(256) void mesh_raycast_bvh_kernel(Bvh B, const float *__restrict__ rays, int Nr, Window w, float *__restrict__ t_out,
                                                               int32_t *__restrict__ tri_out, float *__restrict__ uv_out,
                                                               float *__restrict__ normal_out, uint8_t *__restrict__ hit_out,
                                                               int32_t *__restrict__ flag) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= Nr) return;                                                      // (no barrier below)
    using Sink = typename std::conditional<MODE == MODE_ANY, AnySink, NearestSink>::type;
    RayWalk<Sink> q = {{rays[i * 6], rays[i * 6 + 1], rays[i * 6 + 2], rays[i * 6 + 3], rays[i * 6 + 4], rays[i * 6 + 5]}, w, Sink()};
    if (is_ray(q.r) && !bvh_walk(B, q)) atomicOr(flag, FLAG_BOUND);
    if constexpr (MODE == MODE_ANY) {
        hit_out[i] = q.sink.found ? 1 : 0;
    } else {
        write_nearest(q.sink, i, t_out, tri_out, uv_out);
        if (normal_out) {
            const float nan = __uint_as_float(0x7fc00000u);
            Tri T = {nan, nan, nan, nan, nan, nan, nan, nan, nan};
            int id;
            if (q.sink.where >= 0) T = record_tri(B.records, q.sink.where, id);
            write_normal(T, normal_out + i * 3);
        }
    }
}

// one lane per point, the poses in turn (mesh_ray.hip's visibility rule)
__global__ __launch_bounds__(256) void mesh_visibility_bvh_kernel(Bvh B, const float *__restrict__ points, int N, const float *__restrict__ poses, int P,
                                                                  Camera C, Window w, int32_t *__restrict__ count_out, int32_t *__restrict__ flag) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= N) return;
    const float x = points[i * 3], y = points[i * 3 + 1], z = points[i * 3 + 2];
    int count = 0;
    for (int p = 0; p < P; ++p) {
        RayWalk<AnySink> q = {Ray(), w, AnySink()};
        if (!in_frustum(C, poses + (int64_t)p * 16, x, y, z, q.r) || !is_ray(q.r)) continue;
        if (!bvh_walk(B, q)) atomicOr(flag, FLAG_BOUND);
        count += q.sink.found ? 0 : 1;
    }
    count_out[i] = count;
}

// ---------------------------------------------------------------- host side
int64_t bvh_bytes(int64_t n) {
    if (n < 1 || n > MAX_TRIANGLES) return SGAM_EINVAL;
    const int64_t ni = std::max<int64_t>(n - 1, 1);
    return TRIANGLE_RECORD * n + r16(24 * (2 * n - 1)) + r16(8 * ni) + r16(4 * ni);
}

// the tree inside a caller's workspace; false: the size is refused or the workspace does not hold it
bool bvh_tables(const void *workspace, int64_t workspace_bytes, int64_t n, Bvh &B) {
    if (!workspace_fits(workspace, workspace_bytes, bvh_bytes(n))) return false;
    const int64_t ni = std::max<int64_t>(n - 1, 1);
    char *p = (char *)const_cast<void *>(workspace);
    B.records = (float4 *)p;                p += TRIANGLE_RECORD * n;
    B.boxes = (float *)p;                   p += r16(24 * (2 * n - 1));
    B.children = (int2 *)p;                 p += r16(8 * ni);
    B.ready = (int32_t *)p;
    B.n = (int)n;
    return true;
}

bool box_ok(float lx, float ly, float lz, float hx, float hy, float hz) {
    return std::fabs(lx) <= F32_MAX && std::fabs(ly) <= F32_MAX && std::fabs(lz) <= F32_MAX && hx >= lx && hx <= F32_MAX && hy >= ly && hy <= F32_MAX &&
           hz >= lz && hz <= F32_MAX;
}

}  // namespace

extern "C" int64_t sgam_mesh_bvh_workspace_bytes(int64_t n_candidates) { return bvh_bytes(n_candidates); }

extern "C" int sgam_mesh_bvh_keys(const float *vertices, int32_t nv, const int32_t *triangles, int32_t nt, float lox, float loy, float loz, float hix,
                                  float hiy, float hiz, int64_t *keys_out, int64_t *count_out, int32_t *flag, void *stream) {
    if (!mesh_args_ok(vertices, nv, triangles, nt, flag) || !keys_out || !count_out || !box_ok(lox, loy, loz, hix, hiy, hiz)) return SGAM_EINVAL;
    hipStream_t s = sgam_stream(stream);
    SGAM_KLAUNCH(fill_kernel<int32_t>, dim3(1), dim3(256), 0, s, (int32_t *)count_out, (int64_t)2, 0);          // the int64 count
    SGAM_KLAUNCH(mesh_bvh_keys_kernel, dim3(blocks_of(nt)), dim3(256), 0, s, vertices, nv, triangles, nt, Box6{lox, loy, loz, hix, hiy, hiz}, keys_out,
                 (unsigned long long *)count_out, flag);
    SGAM_LAUNCH_CHECK();
    return SGAM_OK;
}

extern "C" int sgam_mesh_bvh_build(const float *vertices, int32_t nv, const int32_t *triangles, int32_t nt, const int64_t *sorted_keys,
                                   int64_t n_candidates, void *workspace, int64_t workspace_bytes, int32_t *flag, void *stream) {
    Bvh B;
    if (!mesh_args_ok(vertices, nv, triangles, nt, flag) || !sorted_keys || n_candidates > nt || !bvh_tables(workspace, workspace_bytes, n_candidates, B))
        return SGAM_EINVAL;
    hipStream_t s = sgam_stream(stream);
    SGAM_KLAUNCH(mesh_bvh_leaves_kernel, dim3(blocks_of(B.n)), dim3(256), 0, s, vertices, nv, triangles, nt, sorted_keys, B, flag);
    if (B.n > 1) {
        SGAM_KLAUNCH(mesh_bvh_hierarchy_kernel, dim3(blocks_of(B.n - 1)), dim3(256), 0, s, sorted_keys, B, flag);
        const int rounds = std::min(BVH_KEY_BITS, B.n - 1);                   // the height bound
        for (int r = 1; r <= rounds; ++r) SGAM_KLAUNCH(mesh_bvh_boxes_kernel, dim3(blocks_of(B.n - 1)), dim3(256), 0, s, B, r, rounds, flag);
    }
    SGAM_LAUNCH_CHECK();
    return SGAM_OK;
}

extern "C" int sgam_mesh_distance_bvh_f32(const float *query, int32_t Nq, int64_t n_candidates, float lox, float loy, float loz, float hix, float hiy,
                                          float hiz, const void *workspace, int64_t workspace_bytes, float max_d2, float *d2_out,
                                          int32_t *triangle_out, float *closest_out, int32_t *flag, void *stream) {
    Bvh B;
    if (!query || !d2_out || !triangle_out || !flag || Nq < 1 || !(max_d2 >= 0.f) || !box_ok(lox, loy, loz, hix, hiy, hiz) ||
        !bvh_tables(workspace, workspace_bytes, n_candidates, B))
        return SGAM_EINVAL;
    const double lo[3] = {lox, loy, loz}, hi[3] = {hix, hiy, hiz};
    double corner = 0.0, edge = 0.0;
    for (int a = 0; a < 3; ++a) {
        corner = std::max(corner, std::max(std::fabs(lo[a]), std::fabs(hi[a])));
        edge = std::max(edge, hi[a] - lo[a]);
    }
    const double margin = (corner + edge) * MESH_MARGIN;
    if (!(margin <= F32_MAX)) return SGAM_EINVAL;
    SGAM_KLAUNCH(mesh_distance_bvh_kernel, dim3(blocks_of(Nq)), dim3(256), 0, sgam_stream(stream), B, query, Nq, (float)margin, max_d2, d2_out,
                 triangle_out, closest_out, flag);
    SGAM_LAUNCH_CHECK();
    return SGAM_OK;
}

extern "C" int sgam_mesh_raycast_bvh_f32(const float *rays, int32_t n_rays, int64_t n_candidates, const void *workspace, int64_t workspace_bytes,
                                         int32_t mode, float tnear, float tfar, float guard, float *t_out, int32_t *triangle_out, float *uv_out,
                                         float *normal_out, uint8_t *hit_out, int32_t *flag, void *stream) {
    Bvh B;
    if (!rays || !flag || n_rays < 1 || !window_ok(tnear, tfar, guard) || !outputs_ok(mode, t_out, triangle_out, hit_out) ||
        !bvh_tables(workspace, workspace_bytes, n_candidates, B))
        return SGAM_EINVAL;
    const Window w = {tnear, tfar, guard};
    if (mode == MODE_ANY)
        SGAM_KLAUNCH(mesh_raycast_bvh_kernel<MODE_ANY>, dim3(blocks_of(n_rays)), dim3(256), 0, sgam_stream(stream), B, rays, n_rays, w, t_out,
                     triangle_out, uv_out, normal_out, hit_out, flag);
    else
        SGAM_KLAUNCH(mesh_raycast_bvh_kernel<MODE_NEAREST>, dim3(blocks_of(n_rays)), dim3(256), 0, sgam_stream(stream), B, rays, n_rays, w, t_out,
                     triangle_out, uv_out, normal_out, hit_out, flag);
    SGAM_LAUNCH_CHECK();
    return SGAM_OK;
}

extern "C" int sgam_mesh_visibility_bvh_f32(const float *points, int32_t N, const float *poses_w2c, int32_t P, float fx, float fy, float cx, float cy,
                                            int32_t H, int32_t W, float z_near, float z_far, float tolerance, float guard, int64_t n_candidates,
                                            const void *workspace, int64_t workspace_bytes, int32_t *count_out, int32_t *flag, void *stream) {
    Bvh B;
    Camera C;
    if (!points || !poses_w2c || !count_out || !flag || N < 1 || P < 1 || !(tolerance >= 0.f && tolerance <= 1.f) || !(guard >= 0.f && guard <= F32_MAX) ||
        !camera_ok(fx, fy, cx, cy, H, W, z_near, z_far, C) || !bvh_tables(workspace, workspace_bytes, n_candidates, B))
        return SGAM_EINVAL;
    const Window w = {0.0f, 1.0f - tolerance, guard};
    SGAM_KLAUNCH(mesh_visibility_bvh_kernel, dim3(blocks_of(N)), dim3(256), 0, sgam_stream(stream), B, points, N, poses_w2c, P, C, w, count_out, flag);
    SGAM_LAUNCH_CHECK();
    return SGAM_OK;
}
