// mesh_common.h — what the mesh units (mesh_ops.hip, mesh_query.hip) share about an indexed triangle mesh (vertices [nv][3] fp32,
// triangles [nt][3] int32): the bits of the caller's flag word, the triangle cap, and how a triangle's corners are read and checked
// against nv.  What a kernel does with a triangle that names a vertex outside the mesh — skip it, write -1, give NaN, raise the
// flag or not — stays with the kernel: the numpy twins pin each.
#pragma once
#include "points_common.h"

constexpr int FLAG_BOUND = 1;                 // a loop ran into its bound, or a position fell outside its table
constexpr int FLAG_INDEX = 2;                 // a triangle names a vertex outside [0, nv)
constexpr int32_t MAX_TRIANGLES = 1 << 28;    // 6 nt raw incidence entries and 2 nt table slots stay int32

__device__ __forceinline__ void load_corners(const int32_t *__restrict__ triangles, int64_t t, int32_t &a, int32_t &b, int32_t &c) {
    a = triangles[t * 3]; b = triangles[t * 3 + 1]; c = triangles[t * 3 + 2];
}

// every corner in [0, nv): (uint32_t)a < (uint32_t)nv && ... (a negative index is a large unsigned one), as one compare of the largest
__device__ __forceinline__ bool corners_in_mesh(int32_t a, int32_t b, int32_t c, int nv) {
    return max(max((uint32_t)a, (uint32_t)b), (uint32_t)c) < (uint32_t)nv;
}

// the corners of triangle t; false, and FLAG_INDEX in the caller's flag word, when one is outside the mesh
__device__ __forceinline__ bool corners_checked(const int32_t *__restrict__ triangles, int64_t t, int nv, int32_t &a, int32_t &b, int32_t &c,
                                                int32_t *__restrict__ flag) {
    load_corners(triangles, t, a, b, c);
    if (corners_in_mesh(a, b, c, nv)) return true;
    atomicOr(flag, FLAG_INDEX);
    return false;
}
