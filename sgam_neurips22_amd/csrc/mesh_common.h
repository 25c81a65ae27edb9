// mesh_common.h — what the mesh units (mesh_ops.hip, mesh_query.hip, mesh_ray.hip, mesh_bvh.hip; the rules of a query against one triangle: mesh_rules.h) share about an indexed triangle mesh (vertices [nv][3] fp32,
// triangles [nt][3] int32): the bits of the caller's flag word, the triangle cap, and how a triangle's corners are read and checked
// against nv; and, for the units that measure against the surface, the exact arithmetic of a triangle (dot3, the normal, the
// candidate rule), the LDS tile and the 48-byte record of the triangle grid.  What a kernel does with a triangle that names a vertex outside the mesh — skip it, write -1, give NaN, raise the
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

// ---------------------------------------------------------------- the exact arithmetic of a triangle (mesh_query.hip, mesh_ray.hip, mesh_bvh.hip)
namespace {

constexpr int TRI_TILE = 256;                 // triangles per LDS tile of the brute-force kernel (10 floats each)
constexpr int TRIANGLE_RECORD = 48;           // bytes of a record of the grid's cell-sorted table: (a, id), (b, 0), (c, 0)
constexpr double MESH_MARGIN = 1.0 / 16384.0; // 2^-14 of the grid's scale

__device__ __forceinline__ float dot3(float ax, float ay, float az, float bx, float by, float bz) {
    return __fadd_rn(__fadd_rn(__fmul_rn(ax, bx), __fmul_rn(ay, by)), __fmul_rn(az, bz));
}

// the correctly rounded square root: sqrtf under the compiler's default -fhip-fp32-correctly-rounded-divide-sqrt (this toolchain's
// __fsqrt_rn is the native instruction, an approximation, unless OCML's rounded operations are compiled in)
__device__ __forceinline__ float sqrt_rn(float x) { return sqrtf(x); }

__device__ __forceinline__ float diff_of_products(float a, float b, float c, float d) { return __fsub_rn(__fmul_rn(a, b), __fmul_rn(c, d)); }

struct Tri {
    float ax, ay, az, bx, by, bz, cx, cy, cz;
};

// the corners of triangle t; false (flag bit 2) when it names a vertex outside the mesh
__device__ __forceinline__ bool load_tri(const float *__restrict__ vertices, int nv, const int32_t *__restrict__ triangles, int64_t t, Tri &T,
                                         int32_t *__restrict__ flag) {
    int32_t a, b, c;
    if (!corners_checked(triangles, t, nv, a, b, c, flag)) return false;
    T.ax = vertices[(int64_t)a * 3]; T.ay = vertices[(int64_t)a * 3 + 1]; T.az = vertices[(int64_t)a * 3 + 2];
    T.bx = vertices[(int64_t)b * 3]; T.by = vertices[(int64_t)b * 3 + 1]; T.bz = vertices[(int64_t)b * 3 + 2];
    T.cx = vertices[(int64_t)c * 3]; T.cy = vertices[(int64_t)c * 3 + 1]; T.cz = vertices[(int64_t)c * 3 + 2];
    return true;
}

// dot(n, n) of the normal n = ab x ac, and n itself
__device__ __forceinline__ float normal_of(const Tri &T, float &nx, float &ny, float &nz) {
    const float abx = __fsub_rn(T.bx, T.ax), aby = __fsub_rn(T.by, T.ay), abz = __fsub_rn(T.bz, T.az);
    const float acx = __fsub_rn(T.cx, T.ax), acy = __fsub_rn(T.cy, T.ay), acz = __fsub_rn(T.cz, T.az);
    nx = diff_of_products(aby, acz, abz, acy);
    ny = diff_of_products(abz, acx, abx, acz);
    nz = diff_of_products(abx, acy, aby, acx);
    return dot3(nx, ny, nz, nx, ny, nz);
}

__device__ __forceinline__ bool is_candidate(const Tri &T) {
    float nx, ny, nz;
    return finite3(T.ax, T.ay, T.az) && finite3(T.bx, T.by, T.bz) && finite3(T.cx, T.cy, T.cz) && normal_of(T, nx, ny, nz) > 0.0f;
}

// host side: the mesh arguments every sgam_mesh_* entry point refuses before a launch
bool mesh_args_ok(const float *vertices, int nv, const int32_t *triangles, int nt, const int32_t *flag) {
    return vertices && triangles && flag && nv >= 1 && nt >= 1 && nt <= MAX_TRIANGLES;
}

}  // namespace
