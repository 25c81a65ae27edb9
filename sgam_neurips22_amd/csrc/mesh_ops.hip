// mesh_ops.hip — clean-up of an indexed triangle mesh (vertices [nv][3] fp32, triangles [nt][3] int32) on the device: connected
// components, selection of triangles, vertex / triangle incidence as CSR, vertex normals, the Taubin smoothing step, and the
// triangle side of vertex clustering (the vertex side is sgam_points_voxel_assign_f32 of point_cloud.hip).  The rules are stated in
// include/sgam_hip.h and restated in numpy by tests/meshops_oracle.py; DESIGN §4.4.7.  Integer atomics only; every floating-point
// sum runs in an order the data fixes (ascending CSR entries, one lane per vertex); the unit is built with -ffp-contract=off.
//
// Every kernel that reads a triangle checks its three indices against nv (mesh_common.h's corner load and range check, shared with
// mesh_query.hip: flag bit 2, the triangle is skipped) and every kernel
// that walks a CSR segment checks the segment against the item count and every item against its range: no input makes a kernel
// read or write outside the caller's buffers.  No lane ever waits for another: every loop has a bound taken from the sizes, and a
// loop that reaches it ORs 1 into the caller's flag word and returns.
//
// Components: the lock-free least-index union-find of union_find.h (its invariants are stated there) over parent [nv] (the
// workspace).
#include "mesh_common.h"
#include "union_find.h"

#include <algorithm>
#include <cmath>

namespace {

// ---------------------------------------------------------------- components
__global__ __launch_bounds__(256) void components_init_kernel(int32_t *__restrict__ parent, int32_t *__restrict__ count, int nv) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= nv) return;
    parent[i] = (int32_t)i;
    count[i] = 0;
}

__global__ __launch_bounds__(256) void components_link_kernel(const int32_t *__restrict__ triangles, int nt, int nv, int32_t *parent,
                                                              int32_t *__restrict__ flag) {
    const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= nt) return;
    int32_t a, b, c;
    if (!corners_checked(triangles, t, nv, a, b, c, flag)) return;
    bool ok = true;
    if (a != b) ok = uf_unite(parent, a, b, nv);
    if (ok && a != c && b != c) ok = uf_unite(parent, a, c, nv);
    if (!ok) atomicOr(flag, FLAG_BOUND);
}

// (a launch of its own: parent is read-only here, every chain ends at the component's least index)
__global__ __launch_bounds__(256) void components_flatten_kernel(const int32_t *__restrict__ parent, int nv, int32_t *__restrict__ label,
                                                                 int32_t *__restrict__ flag) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= nv) return;
    int32_t x = (int32_t)i;
    int step = 0;
    for (; step <= nv; ++step) {
        const int32_t p = parent[x];
        if (p == x || (uint32_t)p >= (uint32_t)nv) break;
        x = p;
    }
    if (step > nv) atomicOr(flag, FLAG_BOUND);
    label[i] = x;
}

__global__ __launch_bounds__(256) void components_count_kernel(const int32_t *__restrict__ triangles, int nt, int nv,
                                                               const int32_t *__restrict__ label, int32_t *__restrict__ tri_label,
                                                               int32_t *__restrict__ count, int32_t *__restrict__ flag) {
    const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= nt) return;
    int32_t a, b, c;
    if (!corners_checked(triangles, t, nv, a, b, c, flag)) { tri_label[t] = -1; return; }
    const int32_t l = label[a];
    tri_label[t] = l;
    if ((uint32_t)l < (uint32_t)nv) atomicAdd(count + l, 1);
}

// ---------------------------------------------------------------- selection
__global__ __launch_bounds__(256) void mark_vertices_kernel(const int32_t *__restrict__ triangles, int nt, int nv, const uint8_t *__restrict__ keep,
                                                            int32_t *__restrict__ used, int32_t *__restrict__ flag) {
    const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= nt || (keep && !keep[t])) return;
    int32_t a, b, c;
    if (!corners_checked(triangles, t, nv, a, b, c, flag)) return;
    used[a] = 1; used[b] = 1; used[c] = 1;                                 // (every writer writes the same value)
}

__global__ __launch_bounds__(256) void remap_triangles_kernel(const int32_t *__restrict__ triangles, int nt, const int32_t *__restrict__ index,
                                                              int m, const int32_t *__restrict__ vertex_map, int nv, int32_t *__restrict__ out,
                                                              int32_t *__restrict__ flag) {
    const int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= m) return;
    const int32_t t = index[j];
    int32_t a, b, c;
    if ((uint32_t)t >= (uint32_t)nt) { atomicOr(flag, FLAG_INDEX); a = b = c = -1; }
    else if (corners_checked(triangles, t, nv, a, b, c, flag)) { a = vertex_map[a]; b = vertex_map[b]; c = vertex_map[c]; }
    else a = b = c = -1;
    out[j * 3] = a; out[j * 3 + 1] = b; out[j * 3 + 2] = c;
}

// ---------------------------------------------------------------- incidence
// The raw entries of triangle (a, b, c).  kind 0: the triangle's id at each DISTINCT corner.  kind 1: at each corner position the
// other two corners that differ from it (repetitions are dropped after the sort).  `emit(vertex, item)`.
template <typename F>
__device__ __forceinline__ void incidence_entries(int kind, int32_t t, int32_t a, int32_t b, int32_t c, F emit) {
    if (kind == 0) {
        emit(a, t);
        if (b != a) emit(b, t);
        if (c != a && c != b) emit(c, t);
    } else {
        if (b != a) emit(a, b);
        if (c != a) emit(a, c);
        if (a != b) emit(b, a);
        if (c != b) emit(b, c);
        if (a != c) emit(c, a);
        if (b != c) emit(c, b);
    }
}

__global__ __launch_bounds__(256) void incidence_count_kernel(const int32_t *__restrict__ triangles, int nt, int nv, int kind,
                                                              int32_t *__restrict__ count, int32_t *__restrict__ flag) {
    const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= nt) return;
    int32_t a, b, c;
    if (!corners_checked(triangles, t, nv, a, b, c, flag)) return;
    incidence_entries(kind, (int32_t)t, a, b, c, [&](int32_t v, int32_t) { atomicAdd(count + v, 1); });
}

__global__ __launch_bounds__(256) void incidence_fill_kernel(const int32_t *__restrict__ triangles, int nt, int nv, int kind,
                                                             const int32_t *__restrict__ raw_offsets, int64_t n_raw, int32_t *__restrict__ items,
                                                             int32_t *__restrict__ cursor, int32_t *__restrict__ flag) {
    const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= nt) return;
    int32_t a, b, c;
    if (!corners_checked(triangles, t, nv, a, b, c, flag)) return;
    incidence_entries(kind, (int32_t)t, a, b, c, [&](int32_t v, int32_t item) {
        const int64_t beg = raw_offsets[v], end = raw_offsets[v + 1];
        const int64_t at = beg + atomicAdd(cursor + v, 1);                 // arrival order: arbitrary, the sort below removes it
        if (beg >= 0 && at < end && end <= n_raw) items[at] = item;
        else atomicOr(flag, FLAG_BOUND);                                   // (offsets that do not belong to these triangles)
    });
}

__device__ __forceinline__ void sift_down(int32_t *__restrict__ x, int root, int n) {
    const int32_t v = x[root];
    for (;;) {
        int child = 2 * root + 1;
        if (child >= n) break;
        if (child + 1 < n && x[child + 1] > x[child]) ++child;
        if (x[child] <= v) break;
        x[root] = x[child];
        root = child;
    }
    x[root] = v;
}

// one lane per vertex: heap sort of its own segment in place (ascending), then the first of equal entries kept, the rest -1
__global__ __launch_bounds__(256) void incidence_sort_kernel(int nv, const int32_t *__restrict__ raw_offsets, int64_t n_raw,
                                                             int32_t *__restrict__ items, int32_t *__restrict__ degree, int32_t *__restrict__ flag) {
    const int64_t v = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (v >= nv) return;
    const int64_t beg = raw_offsets[v], end = raw_offsets[v + 1];
    if (beg < 0 || end < beg || end > n_raw || degree[v] != end - beg) {   // the cursor must have filled the segment exactly
        atomicOr(flag, FLAG_BOUND);
        degree[v] = 0;
        return;
    }
    int32_t *x = items + beg;
    const int n = (int)(end - beg);
    for (int i = n / 2 - 1; i >= 0; --i) sift_down(x, i, n);
    for (int m = n - 1; m > 0; --m) {
        const int32_t top = x[0];
        x[0] = x[m];
        x[m] = top;
        sift_down(x, 0, m);
    }
    int kept = 0;
    int32_t last = -1;                                                     // (entries are >= 0)
    for (int i = 0; i < n; ++i) {
        const int32_t e = x[i];
        if (e == last) x[i] = -1;
        else { last = e; ++kept; }
    }
    degree[v] = kept;
}

// ---------------------------------------------------------------- normals and the smoothing step
__device__ __forceinline__ bool segment(const int32_t *__restrict__ offsets, int64_t v, int64_t n_items, int64_t &beg, int64_t &end) {
    beg = offsets[v];
    end = offsets[v + 1];
    return beg >= 0 && beg <= end && end <= n_items;
}

__global__ __launch_bounds__(256) void vertex_normals_kernel(const float *__restrict__ vertices, int nv, const int32_t *__restrict__ triangles, int nt,
                                                             const int32_t *__restrict__ offsets, const int32_t *__restrict__ items, int64_t n_items,
                                                             float *__restrict__ normals) {
    const int64_t v = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (v >= nv) return;
    double sx = 0.0, sy = 0.0, sz = 0.0;
    int64_t beg, end;
    if (segment(offsets, v, n_items, beg, end)) {
        for (int64_t e = beg; e < end; ++e) {
            const int32_t t = items[e];
            if ((uint32_t)t >= (uint32_t)nt) continue;
            int32_t a, b, c;
            load_corners(triangles, t, a, b, c);
            if (!corners_in_mesh(a, b, c, nv)) continue;
            const double ax = (double)vertices[(int64_t)a * 3], ay = (double)vertices[(int64_t)a * 3 + 1], az = (double)vertices[(int64_t)a * 3 + 2];
            const double ux = (double)vertices[(int64_t)b * 3] - ax, uy = (double)vertices[(int64_t)b * 3 + 1] - ay,
                         uz = (double)vertices[(int64_t)b * 3 + 2] - az;
            const double wx = (double)vertices[(int64_t)c * 3] - ax, wy = (double)vertices[(int64_t)c * 3 + 1] - ay,
                         wz = (double)vertices[(int64_t)c * 3 + 2] - az;
            sx += uy * wz - uz * wy;
            sy += uz * wx - ux * wz;
            sz += ux * wy - uy * wx;
        }
    }
    const double len = sqrt((sx * sx + sy * sy) + sz * sz);
    float nx = 0.f, ny = 0.f, nz = 0.f;
    if (len > 0.0) { nx = (float)(sx / len); ny = (float)(sy / len); nz = (float)(sz / len); }
    normals[v * 3] = nx; normals[v * 3 + 1] = ny; normals[v * 3 + 2] = nz;
}

__global__ __launch_bounds__(256) void smooth_step_kernel(const float *__restrict__ src, float *__restrict__ dst, int nv,
                                                          const int32_t *__restrict__ offsets, const int32_t *__restrict__ items, int64_t n_items,
                                                          double weight) {
    const int64_t v = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (v >= nv) return;
    const float fx = src[v * 3], fy = src[v * 3 + 1], fz = src[v * 3 + 2];
    double sx = 0.0, sy = 0.0, sz = 0.0;
    int m = 0;
    int64_t beg, end;
    if (segment(offsets, v, n_items, beg, end)) {
        for (int64_t e = beg; e < end; ++e) {
            const int32_t j = items[e];
            if ((uint32_t)j >= (uint32_t)nv) continue;
            sx += (double)src[(int64_t)j * 3]; sy += (double)src[(int64_t)j * 3 + 1]; sz += (double)src[(int64_t)j * 3 + 2];
            ++m;
        }
    }
    float ox = fx, oy = fy, oz = fz;
    if (m > 0) {
        const double px = (double)fx, py = (double)fy, pz = (double)fz, dm = (double)m;
        ox = (float)(px + weight * (sx / dm - px));
        oy = (float)(py + weight * (sy / dm - py));
        oz = (float)(pz + weight * (sz / dm - pz));
    }
    dst[v * 3] = ox; dst[v * 3 + 1] = oy; dst[v * 3 + 2] = oz;
}

// ---------------------------------------------------------------- clustered triangles: degenerate and duplicate ones dropped
constexpr int32_t SLOT_EMPTY = 0x7fffffff;    // (no triangle id: nt <= 2^28, and atomicMin moves a slot only downwards)

// the new triple of triangle t; false: degenerate (two corners in one cluster, a corner in none, an index out of range)
__device__ __forceinline__ bool new_triple(const int32_t *__restrict__ triangles, int64_t t, const int32_t *__restrict__ cluster_of, int nv,
                                           int32_t &a, int32_t &b, int32_t &c) {
    load_corners(triangles, t, a, b, c);
    if (!corners_in_mesh(a, b, c, nv)) { a = b = c = -1; return false; }
    a = cluster_of[a]; b = cluster_of[b]; c = cluster_of[c];
    return a >= 0 && b >= 0 && c >= 0 && a != b && b != c && a != c;
}

// the least index rotated to the front, orientation kept
__device__ __forceinline__ void rotate_least_first(int32_t &a, int32_t &b, int32_t &c) {
    if (b < a && b < c) { const int32_t t = a; a = b; b = c; c = t; }
    else if (c < a && c < b) { const int32_t t = c; c = b; b = a; a = t; }
}

__global__ __launch_bounds__(256) void dedup_insert_kernel(const int32_t *__restrict__ triangles, int nt, const int32_t *__restrict__ cluster_of,
                                                           int nv, int32_t *table, int64_t T, int32_t *__restrict__ slot_of,
                                                           int32_t *__restrict__ triangles_out, int32_t *__restrict__ flag) {
    const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= nt) return;
    int32_t a, b, c;
    const bool live = new_triple(triangles, t, cluster_of, nv, a, b, c);
    triangles_out[t * 3] = a; triangles_out[t * 3 + 1] = b; triangles_out[t * 3 + 2] = c;
    int found = -1;
    if (live) {
        rotate_least_first(a, b, c);
        int64_t s = (int64_t)(mix64(((uint64_t)(uint32_t)a << 42) ^ ((uint64_t)(uint32_t)b << 21) ^ (uint64_t)(uint32_t)c) & (uint64_t)(T - 1));
        for (int64_t probe = 0; probe < T; ++probe) {                        // bounded by the table: ends for every input
            int32_t holder = atomicCAS(table + s, SLOT_EMPTY, (int32_t)t);
            if (holder == SLOT_EMPTY) { found = (int)s; break; }
            // the slot holds a triangle id (it may be lowered meanwhile, to another triangle of the SAME triple): whose triple?
            int32_t ha, hb, hc;
            if ((uint32_t)holder < (uint32_t)nt && new_triple(triangles, holder, cluster_of, nv, ha, hb, hc)) {
                rotate_least_first(ha, hb, hc);
                if (ha == a && hb == b && hc == c) {
                    atomicMin(table + s, (int32_t)t);
                    found = (int)s;
                    break;
                }
            }
            s = (s + 1) & (T - 1);
        }
        if (found < 0) atomicOr(flag, FLAG_BOUND);
    }
    slot_of[t] = found;
}

__global__ __launch_bounds__(256) void dedup_pick_kernel(int nt, const int32_t *__restrict__ table, const int32_t *__restrict__ slot_of,
                                                         uint8_t *__restrict__ keep) {
    const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= nt) return;
    const int s = slot_of[t];
    keep[t] = s >= 0 && table[s] == (int32_t)t ? 1 : 0;
}

}  // namespace

extern "C" int64_t sgam_mesh_components_workspace_bytes(int32_t nv) {
    if (nv < 1) return SGAM_EINVAL;
    return r16(4 * (int64_t)nv);
}

extern "C" int sgam_mesh_components_i32(const int32_t *triangles, int32_t nt, int32_t nv, void *workspace, int64_t workspace_bytes,
                                        int32_t *vertex_label_out, int32_t *triangle_label_out, int32_t *triangle_count_out, int32_t *flag,
                                        void *stream) {
    if (!triangles || !vertex_label_out || !triangle_label_out || !triangle_count_out || !flag || nt < 1 || nt > MAX_TRIANGLES || nv < 1)
        return SGAM_EINVAL;
    if (!workspace_fits(workspace, workspace_bytes, sgam_mesh_components_workspace_bytes(nv))) return SGAM_EINVAL;
    int32_t *parent = (int32_t *)workspace;
    hipStream_t s = sgam_stream(stream);
    SGAM_KLAUNCH(components_init_kernel, dim3(blocks_of(nv)), dim3(256), 0, s, parent, triangle_count_out, nv);
    SGAM_KLAUNCH(components_link_kernel, dim3(blocks_of(nt)), dim3(256), 0, s, triangles, nt, nv, parent, flag);
    SGAM_KLAUNCH(components_flatten_kernel, dim3(blocks_of(nv)), dim3(256), 0, s, parent, nv, vertex_label_out, flag);
    SGAM_KLAUNCH(components_count_kernel, dim3(blocks_of(nt)), dim3(256), 0, s, triangles, nt, nv, vertex_label_out, triangle_label_out,
                 triangle_count_out, flag);
    SGAM_LAUNCH_CHECK();
    return SGAM_OK;
}

extern "C" int sgam_mesh_mark_vertices_i32(const int32_t *triangles, int32_t nt, int32_t nv, const uint8_t *keep, int32_t *used_out,
                                           int32_t *flag, void *stream) {
    if (!triangles || !used_out || !flag || nt < 1 || nt > MAX_TRIANGLES || nv < 1) return SGAM_EINVAL;
    hipStream_t s = sgam_stream(stream);
    SGAM_KLAUNCH(fill_kernel<int32_t>, dim3(blocks_of(nv)), dim3(256), 0, s, used_out, (int64_t)nv, 0);
    SGAM_KLAUNCH(mark_vertices_kernel, dim3(blocks_of(nt)), dim3(256), 0, s, triangles, nt, nv, keep, used_out, flag);
    SGAM_LAUNCH_CHECK();
    return SGAM_OK;
}

extern "C" int sgam_mesh_remap_triangles_i32(const int32_t *triangles, int32_t nt, const int32_t *triangle_index, int32_t m,
                                             const int32_t *vertex_map, int32_t nv, int32_t *triangles_out, int32_t *flag, void *stream) {
    if (!triangles || !triangle_index || !vertex_map || !triangles_out || !flag || nt < 1 || nt > MAX_TRIANGLES || nv < 1 || m < 1 || m > nt)
        return SGAM_EINVAL;
    SGAM_KLAUNCH(remap_triangles_kernel, dim3(blocks_of(m)), dim3(256), 0, sgam_stream(stream), triangles, nt, triangle_index, m, vertex_map, nv,
                 triangles_out, flag);
    SGAM_LAUNCH_CHECK();
    return SGAM_OK;
}

extern "C" int sgam_mesh_incidence_count_i32(const int32_t *triangles, int32_t nt, int32_t nv, int32_t kind, int32_t *count_out, int32_t *flag,
                                             void *stream) {
    if (!triangles || !count_out || !flag || nt < 1 || nt > MAX_TRIANGLES || nv < 1 || (kind != 0 && kind != 1)) return SGAM_EINVAL;
    hipStream_t s = sgam_stream(stream);
    SGAM_KLAUNCH(fill_kernel<int32_t>, dim3(blocks_of(nv)), dim3(256), 0, s, count_out, (int64_t)nv, 0);
    SGAM_KLAUNCH(incidence_count_kernel, dim3(blocks_of(nt)), dim3(256), 0, s, triangles, nt, nv, kind, count_out, flag);
    SGAM_LAUNCH_CHECK();
    return SGAM_OK;
}

extern "C" int sgam_mesh_incidence_fill_i32(const int32_t *triangles, int32_t nt, int32_t nv, int32_t kind, const int32_t *raw_offsets,
                                            int64_t n_raw, int32_t *items_out, int32_t *degree_out, int32_t *flag, void *stream) {
    if (!triangles || !raw_offsets || !items_out || !degree_out || !flag || nt < 1 || nt > MAX_TRIANGLES || nv < 1 || (kind != 0 && kind != 1) ||
        n_raw < 1 || n_raw > 6 * (int64_t)nt)
        return SGAM_EINVAL;
    hipStream_t s = sgam_stream(stream);
    SGAM_KLAUNCH(fill_kernel<int32_t>, dim3(blocks_of(nv)), dim3(256), 0, s, degree_out, (int64_t)nv, 0);
    SGAM_KLAUNCH(incidence_fill_kernel, dim3(blocks_of(nt)), dim3(256), 0, s, triangles, nt, nv, kind, raw_offsets, n_raw, items_out, degree_out,
                 flag);
    SGAM_KLAUNCH(incidence_sort_kernel, dim3(blocks_of(nv)), dim3(256), 0, s, nv, raw_offsets, n_raw, items_out, degree_out, flag);
    SGAM_LAUNCH_CHECK();
    return SGAM_OK;
}

extern "C" int sgam_mesh_vertex_normals_f32(const float *vertices, int32_t nv, const int32_t *triangles, int32_t nt, const int32_t *offsets,
                                            const int32_t *items, int64_t n_items, float *normals_out, void *stream) {
    if (!vertices || !triangles || !offsets || !items || !normals_out || nv < 1 || nt < 1 || nt > MAX_TRIANGLES || n_items < 0) return SGAM_EINVAL;
    SGAM_KLAUNCH(vertex_normals_kernel, dim3(blocks_of(nv)), dim3(256), 0, sgam_stream(stream), vertices, nv, triangles, nt, offsets, items, n_items,
                 normals_out);
    SGAM_LAUNCH_CHECK();
    return SGAM_OK;
}

extern "C" int sgam_mesh_smooth_step_f32(const float *src, float *dst, int32_t nv, const int32_t *offsets, const int32_t *items, int64_t n_items,
                                         double weight, void *stream) {
    if (!src || !dst || src == dst || !offsets || !items || nv < 1 || n_items < 0 || !(std::fabs(weight) <= 1.7976931348623157e308))
        return SGAM_EINVAL;
    SGAM_KLAUNCH(smooth_step_kernel, dim3(blocks_of(nv)), dim3(256), 0, sgam_stream(stream), src, dst, nv, offsets, items, n_items, weight);
    SGAM_LAUNCH_CHECK();
    return SGAM_OK;
}

extern "C" int64_t sgam_mesh_dedup_workspace_bytes(int32_t nt) {
    if (nt < 1 || nt > MAX_TRIANGLES) return SGAM_EINVAL;
    return 4 * hash_table_size(nt) + r16(4 * (int64_t)nt);
}

extern "C" int sgam_mesh_cluster_triangles_i32(const int32_t *triangles, int32_t nt, const int32_t *cluster_of, int32_t nv, void *workspace,
                                               int64_t workspace_bytes, int32_t *triangles_out, uint8_t *keep_out, int32_t *flag, void *stream) {
    if (!triangles || !cluster_of || !triangles_out || !keep_out || !flag || nt < 1 || nt > MAX_TRIANGLES || nv < 1) return SGAM_EINVAL;
    if (!workspace_fits(workspace, workspace_bytes, sgam_mesh_dedup_workspace_bytes(nt))) return SGAM_EINVAL;
    const int64_t T = hash_table_size(nt);
    int32_t *table = (int32_t *)workspace, *slot_of = table + T;
    hipStream_t s = sgam_stream(stream);
    SGAM_KLAUNCH(fill_kernel<int32_t>, dim3(blocks_of(T)), dim3(256), 0, s, table, T, SLOT_EMPTY);
    SGAM_KLAUNCH(dedup_insert_kernel, dim3(blocks_of(nt)), dim3(256), 0, s, triangles, nt, cluster_of, nv, table, T, slot_of, triangles_out, flag);
    SGAM_KLAUNCH(dedup_pick_kernel, dim3(blocks_of(nt)), dim3(256), 0, s, nt, table, slot_of, keep_out);
    SGAM_LAUNCH_CHECK();
    return SGAM_OK;
}
