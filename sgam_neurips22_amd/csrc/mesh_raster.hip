// mesh_raster.hip — depth render of a triangle mesh at a pose: the counterpart of the reference's Filament
// `render_to_depth_image(z_in_view_space=True)` with inf -> 0 (sgam/inference_pipeline.py:777-826) on the marching-cubes mesh
// of the fused volume (tsdf.hip: sgam_tsdf_extract_mesh_f32).  Output: view-space z per sample, 0 where nothing is hit.
//   * samples at integer pixel coordinates (the ray cast's convention, so that the two renders compare; whether Filament
//     samples at +0.5 is unpinned);
//   * vertices world -> camera, clipped against z = z_near in view space (a triangle with one vertex in front keeps a
//     triangle, with two a quad = two triangles; the new vertices are computed from the inside end of each edge, so the two
//     triangles sharing a clipped edge get the same point);
//   * coverage on 24.8 fixed-point screen coordinates with exact int64 edge functions and a top-left tie rule: a sample on an
//     edge two triangles share is covered exactly once, a closed mesh shows no cracks; both windings are rendered;
//   * depth perspective-correct: 1/z interpolated with the screen barycentrics; fragments with z outside [z_near, z_far]
//     are dropped;
//   * nearest fragment by atomicMin on the bits of the positive fp32 z (order-independent, deterministic), then a
//     finalising pass inf -> 0.
// Thread mapping: one lane per triangle; a triangle whose sample box exceeds SMALL samples is rasterised by its whole
// wavefront (lanes over the samples) after the lanes' own small ones — marching-cubes triangles are mostly below a pixel,
// the few large ones (near views) would otherwise serialise their wavefront behind one lane.
// Built with -ffp-contract=off: tests/mc_oracle.py restates every expression in numpy and the outputs are compared bit for bit.
//
// Coloured RGB-D render at P poses (sgam_mesh_render_rgbd_f32): the same transform, clipping, coverage and depth — the device
// functions below are shared, the pose is grid dimension y — with an attribute-carrying visibility pass:
//   * one 64-bit atomicMin per covered sample on key = (bits of z << 32) | fragment id, fragment id = 2 * triangle index + sub
//     (sub = 1 for the second triangle of a near-clipped quad; the id fits 31 bits: max_triangles < 2^30).  The minimum over a
//     set does not depend on the order: deterministic; an exact z tie goes to the lower triangle index; cleared key = all ones;
//   * a resolve pass, one lane per sample: depth = the key's z bits (what the depth render's atomicMin keeps, bit for bit);
//     the winning fragment's triangle is fetched, transformed, clipped and set up again, its edge values E[0..2] at the sample
//     come from the same int64 edge functions, and with iz[j] = 1 / z of vertex j (after setup's winding swap) and C[j] its colour
//         a0 = fl(E[1]) * iz[0],  a1 = fl(E[2]) * iz[1],  a2 = fl(E[0]) * iz[2]          (the products of the depth's w)
//         rgb = ((a0 * C[0] + a1 * C[1]) + a2 * C[2]) / ((a0 + a1) + a2)                  (fp32, every operation rounded, this order)
//         rgb = min(max(rgb, min(C[0], C[1], C[2])), max(C[0], C[1], C[2]))               (rounding never leaves the vertices' range)
//     per channel; a near-clipped vertex's colour is Ca + t * (Cb - Ca) with the t of its position (near_t);
//   * normal: cross(P1 - P0, P2 - P0) of the winning triangle's view-space vertices, normalised, negated when it points away
//     from the camera (n . P0 > 0); rgb_u8: min(max(rgb, 0), 255) truncated (the frame codec's rule, layout.hip).
// tests/mesh_color_oracle.py restates the colour in numpy.
#include "sgam_common.h"

#include <algorithm>

namespace {

constexpr int SMALL = 16;                 // samples of a triangle's box a lane covers alone
constexpr float LIM = 1048576.0f;         // |screen coordinate| < 2^20 px: the int64 edge functions cannot overflow
constexpr unsigned ZINF = 0x7f800000u;

struct View {
    float m[12];                          // world -> camera rows 0..2, row-major
    float fx, fy, cx, cy, zn, zf;
    int H, W;
};

struct Tri {
    int X[3], Y[3];                       // 24.8 fixed point
    float iz[3];                          // 1 / z
    long long area;                       // > 0 (winding normalised)
    int u0, u1, v0, v1;                   // sample box (inclusive); empty when u0 > u1 or v0 > v1
    bool flip;                            // setup exchanged vertices 1 and 2 (read by the resolve pass only)
};

__device__ __forceinline__ bool setup(const View &V, const float *a, const float *b, const float *c, Tri &T) {
    const float *P[3] = {a, b, c};
    for (int i = 0; i < 3; ++i) {
        const float xs = __fadd_rn(__fdiv_rn(__fmul_rn(V.fx, P[i][0]), P[i][2]), V.cx);
        const float ys = __fadd_rn(__fdiv_rn(__fmul_rn(V.fy, P[i][1]), P[i][2]), V.cy);
        if (!(fabsf(xs) < LIM && fabsf(ys) < LIM)) return false;
        T.X[i] = (int)rintf(__fmul_rn(xs, 256.0f));
        T.Y[i] = (int)rintf(__fmul_rn(ys, 256.0f));
        T.iz[i] = __fdiv_rn(1.0f, P[i][2]);
    }
    long long area = (long long)(T.X[1] - T.X[0]) * (T.Y[2] - T.Y[0]) - (long long)(T.Y[1] - T.Y[0]) * (T.X[2] - T.X[0]);
    if (area == 0) return false;
    T.flip = area < 0;
    if (area < 0) {
        int t = T.X[1]; T.X[1] = T.X[2]; T.X[2] = t;
        t = T.Y[1]; T.Y[1] = T.Y[2]; T.Y[2] = t;
        const float f = T.iz[1]; T.iz[1] = T.iz[2]; T.iz[2] = f;
        area = -area;
    }
    T.area = area;
    const int xmin = min(T.X[0], min(T.X[1], T.X[2])), xmax = max(T.X[0], max(T.X[1], T.X[2]));
    const int ymin = min(T.Y[0], min(T.Y[1], T.Y[2])), ymax = max(T.Y[0], max(T.Y[1], T.Y[2]));
    T.u0 = max(0, -((-xmin) >> 8));       // ceil(x / 256)
    T.u1 = min(V.W - 1, xmax >> 8);       // floor(x / 256)
    T.v0 = max(0, -((-ymin) >> 8));
    T.v1 = min(V.H - 1, ymax >> 8);
    return T.u0 <= T.u1 && T.v0 <= T.v1;
}

// the edge values of sample (u, v); false when the sample is not covered
__device__ __forceinline__ bool edges(const Tri &T, int u, int v, long long E[3]) {
    const int px = u * 256, py = v * 256;
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        const int a = i, b = i == 2 ? 0 : i + 1;
        const int dx = T.X[b] - T.X[a], dy = T.Y[b] - T.Y[a];
        E[i] = (long long)dx * (py - T.Y[a]) - (long long)dy * (px - T.X[a]);
        const bool own = dy < 0 || (dy == 0 && dx > 0);          // top-left: the reversed edge never owns
        if (E[i] < 0 || (E[i] == 0 && !own)) return false;
    }
    return true;
}

// Sink(u, v, z, fragment id): what becomes of a covered sample with z in range
template <class Sink>
__device__ __forceinline__ void cover(const View &V, const Tri &T, int u, int v, int64_t frag, const Sink &sink) {
    long long E[3];
    if (!edges(T, u, v, E)) return;
    // E[i] is the weight of the vertex opposite edge i: (i + 2) % 3
    const float w = __fdiv_rn(__fadd_rn(__fadd_rn(__fmul_rn((float)(double)E[1], T.iz[0]), __fmul_rn((float)(double)E[2], T.iz[1])),
                                        __fmul_rn((float)(double)E[0], T.iz[2])),
                              (float)(double)T.area);
    const float z = __fdiv_rn(1.0f, w);
    if (z >= V.zn && z <= V.zf) sink(u, v, z, frag);
}

struct DepthSink {                        // the depth render: nearest z
    unsigned *__restrict__ zbits;
    int W;
    __device__ __forceinline__ void operator()(int u, int v, float z, int64_t) const { atomicMin(&zbits[v * W + u], __float_as_uint(z)); }
};

struct KeySink {                          // the coloured render: nearest z, then lowest fragment id
    unsigned long long *__restrict__ keys;
    int W;
    __device__ __forceinline__ void operator()(int u, int v, float z, int64_t frag) const {
        atomicMin(&keys[(int64_t)v * W + u], ((unsigned long long)__float_as_uint(z) << 32) | (unsigned long long)frag);
    }
};

__device__ __forceinline__ float near_t(const float *a, const float *b, float zn) {
    return __fdiv_rn(__fsub_rn(zn, a[2]), __fsub_rn(b[2], a[2]));
}

__device__ __forceinline__ void near_point(const float *a, const float *b, float zn, float *o) {
    const float t = near_t(a, b, zn);
    o[0] = __fadd_rn(a[0], __fmul_rn(t, __fsub_rn(b[0], a[0])));
    o[1] = __fadd_rn(a[1], __fmul_rn(t, __fsub_rn(b[1], a[1])));
    o[2] = zn;
}

__device__ __forceinline__ void share(Tri &T, int l) {
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        T.X[i] = __shfl(T.X[i], l, 64);
        T.Y[i] = __shfl(T.Y[i], l, 64);
        T.iz[i] = __shfl(T.iz[i], l, 64);
    }
    const int lo = __shfl((int)(T.area & 0xffffffffll), l, 64), hi = __shfl((int)(T.area >> 32), l, 64);
    T.area = ((long long)hi << 32) | (unsigned)lo;
    T.u0 = __shfl(T.u0, l, 64); T.u1 = __shfl(T.u1, l, 64);
    T.v0 = __shfl(T.v0, l, 64); T.v1 = __shfl(T.v1, l, 64);
}

__global__ __launch_bounds__(256) void mesh_zclear_kernel(unsigned *__restrict__ zbits, int n) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) zbits[i] = ZINF;
}

// triangle t in view space (and its vertices' colours when C and colors are given); false when an index is out of range
__device__ __forceinline__ bool fetch(const View &V, const float *__restrict__ verts, const float *__restrict__ colors,
                                      const int *__restrict__ tris, int64_t nv, int64_t t, float P[3][3], float (*C)[3]) {
    bool valid = true;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const int vi = tris[t * 3 + k];
        valid &= vi >= 0 && vi < nv;
        const int64_t vs = valid ? vi : 0;
        const float x = verts[vs * 3], y = verts[vs * 3 + 1], z = verts[vs * 3 + 2];
#pragma unroll
        for (int r = 0; r < 3; ++r)
            P[k][r] = __fadd_rn(__fadd_rn(__fadd_rn(__fmul_rn(V.m[r * 4], x), __fmul_rn(V.m[r * 4 + 1], y)), __fmul_rn(V.m[r * 4 + 2], z)),
                                V.m[r * 4 + 3]);
        if (C)
#pragma unroll
            for (int r = 0; r < 3; ++r) C[k][r] = colors ? colors[vs * 3 + r] : 0.0f;
    }
    return valid;
}

// Near clip of the view-space triangle P (a triangle with one vertex in front keeps a triangle, with two a quad = two
// triangles) and the set-up of what is left: S[k] / ok[k].  With SRC also where the clipped polygon's vertices come from: vertex
// j is P[src[j][0]] when src[j][1] < 0, else the point of the edge P[src[j][0]] (inside) -> P[src[j][1]] (outside) on z = zn;
// S[0] is the polygon's 0 1 2, S[1] its 0 2 3.
template <bool SRC>
__device__ __forceinline__ void clip_setup(const View &V, const float P[3][3], Tri S[2], bool ok[2], int src[4][2]) {
    const bool in0 = P[0][2] >= V.zn, in1 = P[1][2] >= V.zn, in2 = P[2][2] >= V.zn;
    const int n_in = (int)in0 + (int)in1 + (int)in2;
    if (n_in == 3) {
        ok[0] = setup(V, P[0], P[1], P[2], S[0]);
        if (SRC)
#pragma unroll
            for (int j = 0; j < 3; ++j) src[j][0] = j, src[j][1] = -1;
    } else if (n_in == 1) {
        const int i = in0 ? 0 : (in1 ? 1 : 2);
        const float *a = P[i], *b = P[i == 2 ? 0 : i + 1], *c = P[i == 0 ? 2 : i - 1];
        float ab[3], ac[3];
        near_point(a, b, V.zn, ab);
        near_point(a, c, V.zn, ac);
        ok[0] = setup(V, a, ab, ac, S[0]);
        if (SRC) {
            src[0][0] = i, src[0][1] = -1;
            src[1][0] = i, src[1][1] = i == 2 ? 0 : i + 1;
            src[2][0] = i, src[2][1] = i == 0 ? 2 : i - 1;
        }
    } else if (n_in == 2) {
        const int o = !in0 ? 0 : (!in1 ? 1 : 2);
        const float *c = P[o], *a = P[o == 2 ? 0 : o + 1], *b = P[o == 0 ? 2 : o - 1];
        float bc[3], ac[3];
        near_point(b, c, V.zn, bc);
        near_point(a, c, V.zn, ac);
        ok[0] = setup(V, a, b, bc, S[0]);
        ok[1] = setup(V, a, bc, ac, S[1]);
        if (SRC) {
            src[0][0] = o == 2 ? 0 : o + 1, src[0][1] = -1;
            src[1][0] = o == 0 ? 2 : o - 1, src[1][1] = -1;
            src[2][0] = src[1][0], src[2][1] = o;
            src[3][0] = src[0][0], src[3][1] = o;
        }
    }
}

// the rasteriser's body: every sample of every triangle that passes coverage and the z range goes to `sink`
template <class Sink>
__device__ __forceinline__ void raster(const View &V, const float *__restrict__ verts, const int *__restrict__ tris,
                                       const int *__restrict__ counts, int64_t max_v, int64_t max_t, const Sink &sink) {
    const int64_t nv = min((int64_t)counts[0], max_v);
    const int64_t nt = min((int64_t)counts[1], max_t);
    const int lane = threadIdx.x & 63;
    const int64_t wave = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6, n_waves = ((int64_t)gridDim.x * blockDim.x) >> 6;
    for (int64_t base = wave * 64; base < nt; base += n_waves * 64) {          // (wave-uniform trip count)
        const int64_t t = base + lane;
        Tri S[2];
        bool ok[2] = {false, false};
        if (t < nt) {
            float P[3][3];
            if (fetch(V, verts, nullptr, tris, nv, t, P, nullptr)) clip_setup<false>(V, P, S, ok, nullptr);
        }
#pragma unroll
        for (int k = 0; k < 2; ++k) {
            const int bw = S[k].u1 - S[k].u0 + 1, bh = S[k].v1 - S[k].v0 + 1;
            const bool small = ok[k] && (int64_t)bw * bh <= SMALL;
            if (small)
                for (int v = S[k].v0; v <= S[k].v1; ++v)
                    for (int u = S[k].u0; u <= S[k].u1; ++u) cover(V, S[k], u, v, 2 * t + k, sink);
            // the large ones: the whole wavefront, one triangle at a time, lanes over its samples
            unsigned long long big = __builtin_amdgcn_ballot_w64(ok[k] && !small);
            while (big) {
                const int l = __builtin_ctzll(big);
                big &= big - 1;
                Tri T = S[k];
                share(T, l);
                const int w = T.u1 - T.u0 + 1;
                const int64_t n = (int64_t)w * (T.v1 - T.v0 + 1);
                for (int64_t i = lane; i < n; i += 64) cover(V, T, T.u0 + (int)(i % w), T.v0 + (int)(i / w), 2 * (base + l) + k, sink);
            }
        }
    }
}

__global__ __launch_bounds__(256) void mesh_raster_kernel(View V, const float *__restrict__ verts, const int *__restrict__ tris,
                                                          const int *__restrict__ counts, int64_t max_v, int64_t max_t,
                                                          unsigned *__restrict__ zbits) {
    raster(V, verts, tris, counts, max_v, max_t, DepthSink{zbits, V.W});
}

__global__ __launch_bounds__(256) void mesh_zfinal_kernel(unsigned *__restrict__ zbits, int n) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n && zbits[i] == ZINF) zbits[i] = 0u;          // nothing hit -> 0 (the reference's inf -> 0)
}

// ---------------------------------------------------------------- coloured RGB-D render at P poses
constexpr unsigned long long KEY_CLEAR = ~0ull;

// V0 (intrinsics, range, size) with pose p of the DEVICE array poses [P][16]
__device__ __forceinline__ View pose_view(View V, const float *__restrict__ poses, int p) {
#pragma unroll
    for (int i = 0; i < 12; ++i) V.m[i] = poses[(int64_t)p * 16 + i];
    return V;
}

__global__ __launch_bounds__(256) void mesh_keyclear_kernel(unsigned long long *__restrict__ keys, int64_t n) {
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) keys[i] = KEY_CLEAR;
}

// grid (blocks over the triangles, P)
__global__ __launch_bounds__(256) void mesh_raster_keys_kernel(View V0, const float *__restrict__ poses, const float *__restrict__ verts,
                                                               const int *__restrict__ tris, const int *__restrict__ counts,
                                                               int64_t max_v, int64_t max_t, unsigned long long *__restrict__ keys) {
    const View V = pose_view(V0, poses, blockIdx.y);
    raster(V, verts, tris, counts, max_v, max_t, KeySink{keys + (int64_t)blockIdx.y * V.H * V.W, V.W});
}

// grid (blocks over the samples, P): one lane per sample
__global__ __launch_bounds__(256) void mesh_resolve_kernel(View V0, const float *__restrict__ poses, const float *__restrict__ verts,
                                                           const float *__restrict__ colors, const int *__restrict__ tris,
                                                           const int *__restrict__ counts, int64_t max_v, int64_t max_t,
                                                           const unsigned long long *__restrict__ keys, float *__restrict__ depth,
                                                           float *__restrict__ rgb, float *__restrict__ normal,
                                                           uint8_t *__restrict__ rgb_u8) {
    const int64_t hw = (int64_t)V0.H * V0.W;
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= hw) return;
    const int64_t o = (int64_t)blockIdx.y * hw + i;
    const unsigned long long key = keys[o];
    float z = 0.0f, c[3] = {0.0f, 0.0f, 0.0f}, nr[3] = {0.0f, 0.0f, 0.0f};
    if (key != KEY_CLEAR) {
        const View V = pose_view(V0, poses, blockIdx.y);
        const int64_t nv = min((int64_t)counts[0], max_v);
        const int64_t nt = min((int64_t)counts[1], max_t);
        const int64_t t = (int64_t)((key & 0xffffffffull) >> 1);
        const int sub = (int)(key & 1ull);
        float P[3][3], C[3][3];
        // (the visibility pass wrote this id from the same buffers: the checks below hold, they only keep a stale key harmless)
        if (t < nt && fetch(V, verts, colors, tris, nv, t, P, C)) {
            Tri S[2];
            bool ok[2] = {false, false};
            int src[4][2];
            clip_setup<true>(V, P, S, ok, src);
            const Tri &T = S[sub];
            long long E[3];
            const int u = (int)(i % V.W), v = (int)(i / V.W);
            if (ok[sub] && edges(T, u, v, E)) {
                float QC[3][3];
#pragma unroll
                for (int k = 0; k < 3; ++k) {
                    const int *s = src[k == 0 ? 0 : k + sub];
                    if (s[1] < 0) {
#pragma unroll
                        for (int r = 0; r < 3; ++r) QC[k][r] = C[s[0]][r];
                    } else {
                        const float tt = near_t(P[s[0]], P[s[1]], V.zn);
#pragma unroll
                        for (int r = 0; r < 3; ++r) QC[k][r] = __fadd_rn(C[s[0]][r], __fmul_rn(tt, __fsub_rn(C[s[1]][r], C[s[0]][r])));
                    }
                }
                z = __uint_as_float((unsigned)(key >> 32));
                const int k1 = T.flip ? 2 : 1, k2 = T.flip ? 1 : 2;
                const float a0 = __fmul_rn((float)(double)E[1], T.iz[0]), a1 = __fmul_rn((float)(double)E[2], T.iz[1]),
                            a2 = __fmul_rn((float)(double)E[0], T.iz[2]);
                const float sum = __fadd_rn(__fadd_rn(a0, a1), a2);
#pragma unroll
                for (int r = 0; r < 3; ++r) {
                    const float c0 = QC[0][r], c1 = QC[k1][r], c2 = QC[k2][r];
                    const float x = __fdiv_rn(__fadd_rn(__fadd_rn(__fmul_rn(a0, c0), __fmul_rn(a1, c1)), __fmul_rn(a2, c2)), sum);
                    c[r] = fminf(fmaxf(x, fminf(c0, fminf(c1, c2))), fmaxf(c0, fmaxf(c1, c2)));
                }
                const float e1[3] = {P[1][0] - P[0][0], P[1][1] - P[0][1], P[1][2] - P[0][2]};
                const float e2[3] = {P[2][0] - P[0][0], P[2][1] - P[0][1], P[2][2] - P[0][2]};
                float n[3] = {e1[1] * e2[2] - e1[2] * e2[1], e1[2] * e2[0] - e1[0] * e2[2], e1[0] * e2[1] - e1[1] * e2[0]};
                const float len = sqrtf(n[0] * n[0] + n[1] * n[1] + n[2] * n[2]);
                if (len > 0.0f) {
                    const float sgn = (n[0] * P[0][0] + n[1] * P[0][1] + n[2] * P[0][2]) > 0.0f ? -1.0f : 1.0f;
#pragma unroll
                    for (int r = 0; r < 3; ++r) nr[r] = sgn * n[r] / len;
                }
            }
        }
    }
    depth[o] = z;
#pragma unroll
    for (int r = 0; r < 3; ++r) {
        if (rgb) rgb[o * 3 + r] = c[r];
        if (normal) normal[o * 3 + r] = nr[r];
        if (rgb_u8) {
            const float x = fminf(fmaxf(c[r], 0.0f), 255.0f);
            rgb_u8[o * 3 + r] = (uint8_t)((x != x) ? 0u : (unsigned)x);          // clamp -> truncate, like the frame codec
        }
    }
}

}  // namespace

extern "C" int sgam_mesh_render_depth_f32(const float *vertices, int64_t max_vertices, const int32_t *triangles, int64_t max_triangles,
                                          const int32_t *mesh_counts, int32_t H, int32_t W, float fx, float fy, float cx, float cy,
                                          const float *world2cam, float z_near, float z_far, float *depth_out, void *stream) {
    if (!vertices || !triangles || !mesh_counts || !world2cam || !depth_out || max_vertices <= 0 || max_triangles <= 0 || H <= 0 ||
        W <= 0 || (int64_t)H * W >= (1ll << 31) || !(fx > 0.f) || !(fy > 0.f) || !(z_near > 0.f) || !(z_far > z_near))
        return SGAM_EINVAL;
    View V;
    for (int i = 0; i < 12; ++i) V.m[i] = world2cam[i];
    V.fx = fx; V.fy = fy; V.cx = cx; V.cy = cy; V.zn = z_near; V.zf = z_far; V.H = H; V.W = W;
    hipStream_t s = sgam_stream(stream);
    unsigned *zb = (unsigned *)depth_out;       // the output doubles as the depth buffer (bits of positive fp32 z)
    const int n = H * W;
    SGAM_KLAUNCH(mesh_zclear_kernel, dim3(sgam_cdiv(n, 256)), dim3(256), 0, s, zb, n);
    SGAM_KLAUNCH(mesh_raster_kernel, dim3(2048), dim3(256), 0, s, V, vertices, triangles, mesh_counts, max_vertices, max_triangles, zb);
    SGAM_KLAUNCH(mesh_zfinal_kernel, dim3(sgam_cdiv(n, 256)), dim3(256), 0, s, zb, n);
    SGAM_LAUNCH_CHECK();
    return SGAM_OK;
}

extern "C" int64_t sgam_mesh_render_rgbd_workspace_bytes(int32_t P, int32_t H, int32_t W) {
    if (P <= 0 || P > 65535 || H <= 0 || W <= 0 || (int64_t)H * W >= (1ll << 31)) return SGAM_EINVAL;
    return (int64_t)P * H * W * 8;
}

extern "C" int sgam_mesh_render_rgbd_f32(const float *vertices, const float *vertex_colors, int64_t max_vertices, const int32_t *triangles,
                                         int64_t max_triangles, const int32_t *mesh_counts, int32_t P, int32_t H, int32_t W, float fx,
                                         float fy, float cx, float cy, const float *world2cam, float z_near, float z_far,
                                         float *depth_out, float *rgb_out, float *normal_out, uint8_t *rgb_u8_out, void *workspace,
                                         int64_t workspace_bytes, void *stream) {
    if (!vertices || !triangles || !mesh_counts || !world2cam || !depth_out || max_vertices <= 0 || max_triangles <= 0 ||
        max_triangles >= (1ll << 30) ||                       // fragment id = 2 * triangle + sub in 31 bits
        ((rgb_out || rgb_u8_out) && !vertex_colors) || !(fx > 0.f) || !(fy > 0.f) || !(z_near > 0.f) || !(z_far > z_near))
        return SGAM_EINVAL;
    const int64_t need = sgam_mesh_render_rgbd_workspace_bytes(P, H, W);
    if (need < 0) return SGAM_EINVAL;
    if (!workspace || workspace_bytes < need || ((uintptr_t)workspace & 7)) return SGAM_EINVAL;
    View V;
    for (int i = 0; i < 12; ++i) V.m[i] = 0.f;                // (the kernels read pose p from world2cam)
    V.fx = fx; V.fy = fy; V.cx = cx; V.cy = cy; V.zn = z_near; V.zf = z_far; V.H = H; V.W = W;
    hipStream_t s = sgam_stream(stream);
    unsigned long long *keys = (unsigned long long *)workspace;
    const int64_t hw = (int64_t)H * W, n = hw * P;
    SGAM_KLAUNCH(mesh_keyclear_kernel, dim3((unsigned)std::min<int64_t>((n + 255) / 256, 1 << 16)), dim3(256), 0, s, keys, n);
    // the depth render's 2048 blocks shared out over the poses (at least 32 each: 8192 triangles per sweep)
    SGAM_KLAUNCH(mesh_raster_keys_kernel, dim3(std::max(2048 / P, 32), P), dim3(256), 0, s, V, world2cam, vertices, triangles, mesh_counts,
                 max_vertices, max_triangles, keys);
    SGAM_KLAUNCH(mesh_resolve_kernel, dim3((unsigned)((hw + 255) / 256), P), dim3(256), 0, s, V, world2cam, vertices, vertex_colors,
                 triangles, mesh_counts, max_vertices, max_triangles, keys, depth_out, rgb_out, normal_out, rgb_u8_out);
    SGAM_LAUNCH_CHECK();
    return SGAM_OK;
}
