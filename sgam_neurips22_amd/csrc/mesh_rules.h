// mesh_rules.h — the rules of a query against ONE triangle and the sinks that hold a query's winner, shared by the units that walk
// the triangles by brute force or through the grid (mesh_query.hip, mesh_ray.hip) and by the unit that walks them through the
// bounding-volume hierarchy (mesh_bvh.hip): each is written ONCE, so the three accelerators cannot disagree about a bit.  The rules
// themselves are stated where they were first argued: the closest point of a triangle and the (d2 bits, index) winner in
// mesh_query.hip's header, the intersection rule with its guard, the (t bits, index) winner and the visibility rule in
// mesh_ray.hip's header; tests/meshquery_oracle.py and tests/raycast_oracle.py restate them in numpy.
#pragma once
#include "mesh_common.h"

#include <cmath>

namespace {

// ---------------------------------------------------------------- the distance from a point (mesh_query.hip's header)
// the closest point (x, y, z) of candidate T to q by the unit header's rule; returns d2; region: the code 0..6
__device__ __forceinline__ float point_triangle(const Tri &T, float qx, float qy, float qz, float &x, float &y, float &z, int &region) {
    const float abx = __fsub_rn(T.bx, T.ax), aby = __fsub_rn(T.by, T.ay), abz = __fsub_rn(T.bz, T.az);
    const float acx = __fsub_rn(T.cx, T.ax), acy = __fsub_rn(T.cy, T.ay), acz = __fsub_rn(T.cz, T.az);
    const float apx = __fsub_rn(qx, T.ax), apy = __fsub_rn(qy, T.ay), apz = __fsub_rn(qz, T.az);
    const float bpx = __fsub_rn(qx, T.bx), bpy = __fsub_rn(qy, T.by), bpz = __fsub_rn(qz, T.bz);
    const float cpx = __fsub_rn(qx, T.cx), cpy = __fsub_rn(qy, T.cy), cpz = __fsub_rn(qz, T.cz);
    const float p1 = dot3(abx, aby, abz, apx, apy, apz), p2 = dot3(acx, acy, acz, apx, apy, apz);
    const float p3 = dot3(abx, aby, abz, bpx, bpy, bpz), p4 = dot3(acx, acy, acz, bpx, bpy, bpz);
    const float p5 = dot3(abx, aby, abz, cpx, cpy, cpz), p6 = dot3(acx, acy, acz, cpx, cpy, cpz);
    const float vc = diff_of_products(p1, p4, p3, p2), vb = diff_of_products(p5, p2, p1, p6), va = diff_of_products(p3, p6, p5, p4);
    const float e43 = __fsub_rn(p4, p3), e56 = __fsub_rn(p5, p6);
    const bool t0 = (p1 <= 0.0f) & (p2 <= 0.0f);
    const bool t1 = (p3 >= 0.0f) & (p4 <= p3);
    const bool t3 = (vc <= 0.0f) & (p1 >= 0.0f) & (p3 <= 0.0f);
    const bool t2 = (p6 >= 0.0f) & (p5 <= p6);
    const bool t5 = (vb <= 0.0f) & (p2 >= 0.0f) & (p6 <= 0.0f);
    const bool t4 = (va <= 0.0f) & (e43 >= 0.0f) & (e56 >= 0.0f);
    region = t0 ? 0 : t1 ? 1 : t3 ? 3 : t2 ? 2 : t5 ? 5 : t4 ? 4 : 6;
    const float sum = __fadd_rn(__fadd_rn(va, vb), vc);
    const float n1 = region == 3 ? p1 : region == 5 ? p2 : region == 4 ? e43 : region == 6 ? vb : 0.0f;
    const float m1 = region == 3 ? __fsub_rn(p1, p3) : region == 5 ? __fsub_rn(p2, p6) : region == 4 ? __fadd_rn(e43, e56) : region == 6 ? sum : 1.0f;
    const float n2 = region == 6 ? vc : 0.0f, m2 = region == 6 ? sum : 1.0f;
    const float s1 = __fdiv_rn(n1, m1), s2 = __fdiv_rn(n2, m2);
    const bool from_b = (region == 1) | (region == 4), from_c = region == 2;
    const float ox = from_b ? T.bx : from_c ? T.cx : T.ax, oy = from_b ? T.by : from_c ? T.cy : T.ay, oz = from_b ? T.bz : from_c ? T.cz : T.az;
    const bool along_ac = region == 5, along_bc = region == 4;
    const float ex = along_ac ? acx : along_bc ? __fsub_rn(T.cx, T.bx) : abx;
    const float ey = along_ac ? acy : along_bc ? __fsub_rn(T.cy, T.by) : aby;
    const float ez = along_ac ? acz : along_bc ? __fsub_rn(T.cz, T.bz) : abz;
    x = __fadd_rn(__fadd_rn(ox, __fmul_rn(ex, s1)), __fmul_rn(acx, s2));
    y = __fadd_rn(__fadd_rn(oy, __fmul_rn(ey, s1)), __fmul_rn(acy, s2));
    z = __fadd_rn(__fadd_rn(oz, __fmul_rn(ez, s1)), __fmul_rn(acz, s2));
    return dist2(x, y, z, qx, qy, qz);
}

// the held winner of a query: least (d2 bits, triangle index), its closest point carried along
struct MeshSink {
    float best = __uint_as_float(0x7f800000u);
    int bi = -1;
    float x = __uint_as_float(0x7fc00000u), y = __uint_as_float(0x7fc00000u), z = __uint_as_float(0x7fc00000u);
    __device__ __forceinline__ void offer(float d2, int id, float max_d2, float cx, float cy, float cz) {
        const bool take = (d2 <= max_d2) & ((d2 < best) | ((d2 == best) & (id < bi)));        // (+inf == +inf: id < -1 never holds)
        best = take ? d2 : best;
        bi = take ? id : bi;
        x = take ? cx : x; y = take ? cy : y; z = take ? cz : z;
    }
    // the grid kernel gives a query a whole wavefront, every lane holding the winner of its share of the candidates: the `best` the
    // stop rule reads is the least over the 64 lanes (the same number in every lane, so the walk stays wave-uniform)
    __device__ __forceinline__ float bound() const {
        float b = best;
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) b = fminf(b, __shfl_xor(b, o, 64));
        return b;
    }
    // the lanes' winners folded into the wave's: the least (d2 bits, index) key, the closest point of the first lane that holds it
    __device__ __forceinline__ void fold_wave() {
        uint32_t hi = bi >= 0 ? __float_as_uint(best) : 0x7f800000u, lo = (uint32_t)bi;
        const uint64_t mine = ((uint64_t)hi << 32) | lo;
        uint64_t least = mine;
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            const uint64_t other = ((uint64_t)(uint32_t)__shfl_xor((int)(least >> 32), o, 64) << 32) | (uint32_t)__shfl_xor((int)(uint32_t)least, o, 64);
            least = other < least ? other : least;
        }
        const int src = __ffsll((unsigned long long)__ballot(mine == least)) - 1;
        x = __shfl(x, src, 64); y = __shfl(y, src, 64); z = __shfl(z, src, 64);
        best = __uint_as_float((uint32_t)(least >> 32));
        bi = (int)(uint32_t)least;
    }
    __device__ __forceinline__ void write(int64_t i, float *__restrict__ d2_out, int32_t *__restrict__ tri_out, float *__restrict__ closest) const {
        d2_out[i] = best;
        tri_out[i] = bi;
        if (closest) { closest[i * 3] = x; closest[i * 3 + 1] = y; closest[i * 3 + 2] = z; }
    }
};

// ---------------------------------------------------------------- rays (mesh_ray.hip's header)
constexpr int MODE_NEAREST = 0, MODE_ANY = 1;

struct Ray {
    float ox, oy, oz, dx, dy, dz;
};

__device__ __forceinline__ bool is_ray(const Ray &r) {
    return finite3(r.ox, r.oy, r.oz) && finite3(r.dx, r.dy, r.dz) && !(r.dx == 0.0f && r.dy == 0.0f && r.dz == 0.0f);
}

__device__ __forceinline__ Ray not_a_ray() {
    const float nan = __uint_as_float(0x7fc00000u);
    return {nan, nan, nan, nan, nan, nan};
}

// P_j(t) of the unit's header
__device__ __forceinline__ float along(float o, float d, float t) { return __fadd_rn(o, __fmul_rn(t, d)); }

struct Window {
    float tnear, tfar, guard;
};

// the unit header's intersection rule; true: a hit, with its t, u, v
__device__ __forceinline__ bool ray_triangle(const Tri &T, const Ray &r, const Window &w, float &t, float &u, float &v) {
    const float e1x = __fsub_rn(T.bx, T.ax), e1y = __fsub_rn(T.by, T.ay), e1z = __fsub_rn(T.bz, T.az);
    const float e2x = __fsub_rn(T.cx, T.ax), e2y = __fsub_rn(T.cy, T.ay), e2z = __fsub_rn(T.cz, T.az);
    const float px = diff_of_products(r.dy, e2z, r.dz, e2y), py = diff_of_products(r.dz, e2x, r.dx, e2z), pz = diff_of_products(r.dx, e2y, r.dy, e2x);
    const float det = dot3(e1x, e1y, e1z, px, py, pz);
    const float sx = __fsub_rn(r.ox, T.ax), sy = __fsub_rn(r.oy, T.ay), sz = __fsub_rn(r.oz, T.az);
    u = __fdiv_rn(dot3(sx, sy, sz, px, py, pz), det);
    const float qx = diff_of_products(sy, e1z, sz, e1y), qy = diff_of_products(sz, e1x, sx, e1z), qz = diff_of_products(sx, e1y, sy, e1x);
    v = __fdiv_rn(dot3(r.dx, r.dy, r.dz, qx, qy, qz), det);
    t = __fadd_rn(__fdiv_rn(dot3(e2x, e2y, e2z, qx, qy, qz), det), 0.0f);
    bool hit = (det != 0.0f) & (u >= 0.0f) & (v >= 0.0f) & (__fadd_rn(u, v) <= 1.0f) & (t >= w.tnear) & (t <= w.tfar);
    const float Px = along(r.ox, r.dx, t), Py = along(r.oy, r.dy, t), Pz = along(r.oz, r.dz, t);
    const float lox = __fsub_rn(fminf(fminf(T.ax, T.bx), T.cx), w.guard), hix = __fadd_rn(fmaxf(fmaxf(T.ax, T.bx), T.cx), w.guard);
    const float loy = __fsub_rn(fminf(fminf(T.ay, T.by), T.cy), w.guard), hiy = __fadd_rn(fmaxf(fmaxf(T.ay, T.by), T.cy), w.guard);
    const float loz = __fsub_rn(fminf(fminf(T.az, T.bz), T.cz), w.guard), hiz = __fadd_rn(fmaxf(fmaxf(T.az, T.bz), T.cz), w.guard);
    hit &= (Px >= lox) & (Px <= hix) & (Py >= loy) & (Py <= hiy) & (Pz >= loz) & (Pz <= hiz);
    return hit;
}

// the held winner of a ray: least (t bits, triangle index); `where` = the winner's position (its record in the grid's table)
struct NearestSink {
    float best = __uint_as_float(0x7f800000u);
    int bi = -1, where = -1;
    float u = __uint_as_float(0x7fc00000u), v = __uint_as_float(0x7fc00000u);
    __device__ __forceinline__ void offer(bool hit, float t, float hu, float hv, int id, int k) {
        const bool take = hit & ((t < best) | ((t == best) & (id < bi)));
        best = take ? t : best;
        bi = take ? id : bi;
        where = take ? k : where;
        u = take ? hu : u; v = take ? hv : v;
    }
    __device__ __forceinline__ bool full() const { return false; }                     // every record of a visited cell is offered
    __device__ __forceinline__ bool done(float tb) const { return best <= tb; }
};

struct AnySink {
    bool found = false;
    __device__ __forceinline__ void offer(bool hit, float, float, float, int, int) { found |= hit; }
    __device__ __forceinline__ bool full() const { return found; }
    __device__ __forceinline__ bool done(float) const { return found; }
};

__device__ __forceinline__ void write_normal(const Tri &T, float *__restrict__ out) {
    float nx, ny, nz;
    const float l = sqrt_rn(normal_of(T, nx, ny, nz));
    out[0] = __fdiv_rn(nx, l); out[1] = __fdiv_rn(ny, l); out[2] = __fdiv_rn(nz, l);
}

__device__ __forceinline__ void write_nearest(const NearestSink &s, int64_t i, float *__restrict__ t_out, int32_t *__restrict__ tri_out,
                                              float *__restrict__ uv_out) {
    t_out[i] = s.best;
    tri_out[i] = s.bi;
    if (uv_out) { uv_out[i * 2] = s.u; uv_out[i * 2 + 1] = s.v; }
}

// ---------------------------------------------------------------- visibility
struct Camera {
    float fx, fy, cx, cy, zn, zf, fw, fh;                                     // fw, fh: W and H as floats
};

// the camera centre of pose M (world -> camera, 4 x 4 row-major) by the unit header's rule
__device__ __forceinline__ void camera_centre(const float *__restrict__ M, float &cx, float &cy, float &cz) {
    cx = -__fadd_rn(__fadd_rn(__fmul_rn(M[0], M[3]), __fmul_rn(M[4], M[7])), __fmul_rn(M[8], M[11]));
    cy = -__fadd_rn(__fadd_rn(__fmul_rn(M[1], M[3]), __fmul_rn(M[5], M[7])), __fmul_rn(M[9], M[11]));
    cz = -__fadd_rn(__fadd_rn(__fmul_rn(M[2], M[3]), __fmul_rn(M[6], M[7])), __fmul_rn(M[10], M[11]));
}

// x in the frustum of pose M; r: the ray from the camera centre to x
__device__ __forceinline__ bool in_frustum(const Camera &C, const float *__restrict__ M, float x, float y, float z, Ray &r) {
    float X, Y, Z;
    transform34(M, x, y, z, X, Y, Z);                                         // (rows of 4: the first twelve numbers of M)
    camera_centre(M, r.ox, r.oy, r.oz);
    r.dx = __fsub_rn(x, r.ox); r.dy = __fsub_rn(y, r.oy); r.dz = __fsub_rn(z, r.oz);
    if (!(C.zn <= Z && Z <= C.zf)) return false;
    const float u = __fadd_rn(__fdiv_rn(__fmul_rn(C.fx, X), Z), C.cx), v = __fadd_rn(__fdiv_rn(__fmul_rn(C.fy, Y), Z), C.cy);
    const float uf = floorf(__fadd_rn(u, 0.5f)), vf = floorf(__fadd_rn(v, 0.5f));
    return 0.0f <= uf && uf < C.fw && 0.0f <= vf && vf < C.fh;
}

// ---------------------------------------------------------------- host side: what every ray entry point refuses before a launch
bool window_ok(float tnear, float tfar, float guard) {
    return tnear >= 0.f && tnear <= F32_MAX && tfar >= tnear && guard >= 0.f && guard <= F32_MAX;      // (NaN fails; tfar may be +inf)
}

bool outputs_ok(int mode, const float *t_out, const int32_t *triangle_out, const uint8_t *hit_out) {
    return mode == MODE_NEAREST ? (t_out && triangle_out) : mode == MODE_ANY ? hit_out != nullptr : false;
}

bool camera_ok(float fx, float fy, float cx, float cy, int H, int W, float z_near, float z_far, Camera &C) {
    if (!(std::fabs(fx) <= F32_MAX && std::fabs(fy) <= F32_MAX && std::fabs(cx) <= F32_MAX && std::fabs(cy) <= F32_MAX) || fx == 0.f || fy == 0.f) return false;
    if (H < 1 || W < 1 || (int64_t)H * W > 0x7fffffffll || !(z_near > 0.f && z_far >= z_near && z_far <= F32_MAX)) return false;
    C = {fx, fy, cx, cy, z_near, z_far, (float)W, (float)H};
    return true;
}

}  // namespace
