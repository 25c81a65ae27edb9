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
#include "sgam_common.h"

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

__device__ __forceinline__ void cover(const View &V, const Tri &T, int u, int v, unsigned *__restrict__ zbits) {
    const int px = u * 256, py = v * 256;
    long long E[3];
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        const int a = i, b = i == 2 ? 0 : i + 1;
        const int dx = T.X[b] - T.X[a], dy = T.Y[b] - T.Y[a];
        E[i] = (long long)dx * (py - T.Y[a]) - (long long)dy * (px - T.X[a]);
        const bool own = dy < 0 || (dy == 0 && dx > 0);          // top-left: the reversed edge never owns
        if (E[i] < 0 || (E[i] == 0 && !own)) return;
    }
    // E[i] is the weight of the vertex opposite edge i: (i + 2) % 3
    const float w = __fdiv_rn(__fadd_rn(__fadd_rn(__fmul_rn((float)(double)E[1], T.iz[0]), __fmul_rn((float)(double)E[2], T.iz[1])),
                                        __fmul_rn((float)(double)E[0], T.iz[2])),
                              (float)(double)T.area);
    const float z = __fdiv_rn(1.0f, w);
    if (z >= V.zn && z <= V.zf) atomicMin(&zbits[v * V.W + u], __float_as_uint(z));
}

__device__ __forceinline__ void near_point(const float *a, const float *b, float zn, float *o) {
    const float t = __fdiv_rn(__fsub_rn(zn, a[2]), __fsub_rn(b[2], a[2]));
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

__global__ __launch_bounds__(256) void mesh_raster_kernel(View V, const float *__restrict__ verts, const int *__restrict__ tris,
                                                          const int *__restrict__ counts, int64_t max_v, int64_t max_t,
                                                          unsigned *__restrict__ zbits) {
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
            }
            const bool in0 = P[0][2] >= V.zn, in1 = P[1][2] >= V.zn, in2 = P[2][2] >= V.zn;
            const int n_in = (int)in0 + (int)in1 + (int)in2;
            if (valid && n_in == 3) {
                ok[0] = setup(V, P[0], P[1], P[2], S[0]);
            } else if (valid && n_in == 1) {
                const int i = in0 ? 0 : (in1 ? 1 : 2);
                const float *a = P[i], *b = P[i == 2 ? 0 : i + 1], *c = P[i == 0 ? 2 : i - 1];
                float ab[3], ac[3];
                near_point(a, b, V.zn, ab);
                near_point(a, c, V.zn, ac);
                ok[0] = setup(V, a, ab, ac, S[0]);
            } else if (valid && n_in == 2) {
                const int o = !in0 ? 0 : (!in1 ? 1 : 2);
                const float *c = P[o], *a = P[o == 2 ? 0 : o + 1], *b = P[o == 0 ? 2 : o - 1];
                float bc[3], ac[3];
                near_point(b, c, V.zn, bc);
                near_point(a, c, V.zn, ac);
                ok[0] = setup(V, a, b, bc, S[0]);
                ok[1] = setup(V, a, bc, ac, S[1]);
            }
        }
#pragma unroll
        for (int k = 0; k < 2; ++k) {
            const int bw = S[k].u1 - S[k].u0 + 1, bh = S[k].v1 - S[k].v0 + 1;
            const bool small = ok[k] && (int64_t)bw * bh <= SMALL;
            if (small)
                for (int v = S[k].v0; v <= S[k].v1; ++v)
                    for (int u = S[k].u0; u <= S[k].u1; ++u) cover(V, S[k], u, v, zbits);
            // the large ones: the whole wavefront, one triangle at a time, lanes over its samples
            unsigned long long big = __builtin_amdgcn_ballot_w64(ok[k] && !small);
            while (big) {
                const int l = __builtin_ctzll(big);
                big &= big - 1;
                Tri T = S[k];
                share(T, l);
                const int w = T.u1 - T.u0 + 1;
                const int64_t n = (int64_t)w * (T.v1 - T.v0 + 1);
                for (int64_t i = lane; i < n; i += 64) cover(V, T, T.u0 + (int)(i % w), T.v0 + (int)(i / w), zbits);
            }
        }
    }
}

__global__ __launch_bounds__(256) void mesh_zfinal_kernel(unsigned *__restrict__ zbits, int n) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n && zbits[i] == ZINF) zbits[i] = 0u;          // nothing hit -> 0 (the reference's inf -> 0)
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
