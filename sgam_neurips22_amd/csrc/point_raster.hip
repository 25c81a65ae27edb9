// point_raster.hip — RGB-D views of a set of stored frames as a z-tested point splat (sgam_points_render_rgbd_f32): every pixel of
// every frame unprojected with its own depth, moved into the view camera, splatted onto the view's pixel grid with a depth test,
// at P poses in one call.  The scene loop's own conditioning is the same operation for one target (warp.hip: forward splat + 3x3
// median hole fill); this one is view-correct across MANY frames — the nearest point wins, not the largest index — and reads the
// frame store in place through DEVICE tables of addresses (one allocation per frame, any number of frames).  It is a sibling of
// mesh_raster.hip and shares its visibility idea: one 64-bit atomicMin per covered sample on (z bits << 32) | id, then a resolve.
//
// Per source point: frame f, pixel q = i * Ws + j, d = depth_f[i][j].  Every operator below is ONE IEEE fp32 operation, in the
// written order, nothing fused (points_common.h states the rule and holds the unprojection):
//     skip unless d is finite and d > 0
//     (X, Y, Z) = points_common.h's unprojection of (i, j, d) with T = T_rel[p][f] (source -> view)
//     skip unless z_near <= Z && Z <= z_far               (NaN fails)
//     u = (fx * X) / Z + cx        v = (fy * Y) / Z + cy
//     uf = floorf(u + 0.5f)        vf = floorf(v + 0.5f)
//     skip unless -(radius + 1) < uf && uf < W + radius && -(radius + 1) < vf && vf < H + radius      (float compares; NaN fails)
//     px = (int)uf   py = (int)vf
//     for dy, dx in [-radius, radius]:  if 0 <= px + dx < W and 0 <= py + dy < H:
//         atomicMin(keys[p][py + dy][px + dx], (uint64(bits of Z) << 32) | uint32(f * Hs * Ws + q))
// Keys start as all ones = "empty"; Z is positive and finite, so a real key never is.  The minimum over a set does not depend on
// the order: deterministic; an exact z tie goes to the lower id = the earlier frame, then the lower pixel.
// Resolve (one lane per output sample): empty -> depth 0, rgb 0, index -1; else depth = the float whose bits are key >> 32, rgb =
// the winning point's three uint8 values as fp32 0..255, index = the key's low 32 bits.
// Hole fill (hole_fill = 1): only EMPTY samples change; each of r, g, b, depth becomes the 5th smallest of the nine values of its
// 3 x 3 window in the UNFILLED image, where positions outside the image and empty samples count as 0 — the conditioning's median
// fill with "hole" = "nothing landed": a sample with fewer than five hit neighbours stays 0.  Hit samples and index_out are
// unchanged.  The unfilled window is rebuilt from the keys, so the fill needs no second image and no second pass.
// tests/points_oracle.py restates all of this in numpy; the outputs are compared bit for bit.
//
// Launch shape (latency- and atomic-bound, no MFMA): ONE projection launch over (pixel blocks, frames, poses); consecutive lanes
// take consecutive pixels of one frame, so the depth reads coalesce, T_rel[p][f] is wave-uniform and a near-identity view sends
// whole 512-byte runs of keys per wave instruction.  The atomics are non-returning, relaxed, agent scope; they execute at the
// memory side (warp.hip, "Forward splat, target-owned tiles"), so the key is first read with a relaxed load and the atomic is
// skipped when the new key is not smaller: keys only decrease, a stale read is never smaller than the key — the result is the same.
#include "points_common.h"

#include <algorithm>

namespace {

constexpr unsigned long long KEY_CLEAR = ~0ull;
constexpr bool PREREAD = true;            // read the key before the atomic (measured against the plain form)

struct PointView {
    float kinv[9];                        // source intrinsics, inverted in float64 and rounded once (host)
    float fx, fy, cx, cy, zn, zf;
    int Hs, Ws, H, W, radius;
};

__global__ __launch_bounds__(256) void points_keyclear_kernel(unsigned long long *__restrict__ keys, int64_t n) {
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) keys[i] = KEY_CLEAR;
}

// grid (blocks over a frame's pixels, frames (strided), P): one lane per (pose, frame, pixel)
__global__ __launch_bounds__(256) void points_project_kernel(PointView V, const float *const *__restrict__ depth_ptrs, int F,
                                                             const float *__restrict__ T_rel, unsigned long long *__restrict__ keys) {
    const unsigned hw_s = (unsigned)V.Hs * (unsigned)V.Ws;
    const int64_t q64 = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (q64 >= (int64_t)hw_s) return;
    const unsigned q = (unsigned)q64;
    const int p = blockIdx.z;
    const int i = (int)(q / (unsigned)V.Ws), j = (int)(q - (unsigned)i * (unsigned)V.Ws);
    float a, b, c;
    pixel_ray(V.kinv, i, j, a, b, c);
    unsigned long long *__restrict__ kp = keys + (int64_t)p * V.H * V.W;
    const float lo = (float)(-(V.radius + 1)), hi_u = (float)((int64_t)V.W + V.radius), hi_v = (float)((int64_t)V.H + V.radius);
    for (int f = blockIdx.y; f < F; f += gridDim.y) {                         // (block-uniform)
        const float d = depth_ptrs[f][q];
        if (!(d > 0.0f && d <= F32_MAX)) continue;                            // finite and positive (NaN fails)
        const float *__restrict__ T = T_rel + ((int64_t)p * F + f) * 12;       // wave-uniform
        float X, Y, Z;
        transform34(T, __fmul_rn(a, d), __fmul_rn(b, d), __fmul_rn(c, d), X, Y, Z);
        if (!(V.zn <= Z && Z <= V.zf)) continue;
        const float u = __fadd_rn(__fdiv_rn(__fmul_rn(V.fx, X), Z), V.cx);
        const float v = __fadd_rn(__fdiv_rn(__fmul_rn(V.fy, Y), Z), V.cy);
        const float uf = floorf(__fadd_rn(u, 0.5f)), vf = floorf(__fadd_rn(v, 0.5f));
        if (!(lo < uf && uf < hi_u && lo < vf && vf < hi_v)) continue;
        const int px = (int)uf, py = (int)vf;                                  // within (-radius - 1, size + radius): no overflow
        const unsigned id = (unsigned)f * hw_s + q;                            // F * Hs * Ws < 2^32 (checked by the launcher)
        const unsigned long long key = ((unsigned long long)__float_as_uint(Z) << 32) | (unsigned long long)id;
        for (int dy = -V.radius; dy <= V.radius; ++dy) {
            const int yy = py + dy;
            if (yy < 0 || yy >= V.H) continue;
            for (int dx = -V.radius; dx <= V.radius; ++dx) {
                const int xx = px + dx;
                if (xx < 0 || xx >= V.W) continue;
                unsigned long long *k = kp + (int64_t)yy * V.W + xx;
                if (PREREAD && __hip_atomic_load(k, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) <= key) continue;
                __hip_atomic_fetch_min(k, key, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            }
        }
    }
}

#define SGAM_PS2(a, b)                  \
    {                                   \
        const float lo_ = fminf(a, b);  \
        (b) = fmaxf(a, b);              \
        (a) = lo_;                      \
    }
// 5th smallest of 9 (no NaN reaches it: depths are finite, colours integers).  19-exchange network, as warp.hip's median9.
__device__ __forceinline__ float fifth_of_9(float *p) {
    SGAM_PS2(p[1], p[2]); SGAM_PS2(p[4], p[5]); SGAM_PS2(p[7], p[8]);
    SGAM_PS2(p[0], p[1]); SGAM_PS2(p[3], p[4]); SGAM_PS2(p[6], p[7]);
    SGAM_PS2(p[1], p[2]); SGAM_PS2(p[4], p[5]); SGAM_PS2(p[7], p[8]);
    SGAM_PS2(p[0], p[3]); SGAM_PS2(p[5], p[8]); SGAM_PS2(p[4], p[7]);
    SGAM_PS2(p[3], p[6]); SGAM_PS2(p[1], p[4]); SGAM_PS2(p[2], p[5]);
    SGAM_PS2(p[4], p[7]); SGAM_PS2(p[4], p[2]); SGAM_PS2(p[6], p[4]);
    SGAM_PS2(p[4], p[2]);
    return p[4];
}

// (r, g, b, z) of a key's point; zeros for an empty key
__device__ __forceinline__ void point_of(unsigned long long key, unsigned hw_s, const uint8_t *const *__restrict__ rgb_ptrs, int F,
                                         float o[4]) {
    o[0] = o[1] = o[2] = o[3] = 0.0f;
    if (key == KEY_CLEAR) return;
    const unsigned id = (unsigned)(key & 0xffffffffull);
    const unsigned f = id / hw_s, q = id - f * hw_s;
    if (f >= (unsigned)F) return;            // (the projection wrote this id from the same tables: it holds; keeps a stale key harmless)
    const uint8_t *__restrict__ c = rgb_ptrs[f] + (int64_t)q * 3;
    o[0] = (float)c[0]; o[1] = (float)c[1]; o[2] = (float)c[2];
    o[3] = __uint_as_float((unsigned)(key >> 32));
}

// grid (blocks over the samples, P): one lane per output sample
__global__ __launch_bounds__(256) void points_resolve_kernel(PointView V, const uint8_t *const *__restrict__ rgb_ptrs, int F, int hole_fill,
                                                             const unsigned long long *__restrict__ keys, float *__restrict__ depth,
                                                             float *__restrict__ rgb, uint8_t *__restrict__ rgb_u8,
                                                             int32_t *__restrict__ index) {
    const int64_t hw = (int64_t)V.H * V.W;
    const int64_t s = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (s >= hw) return;
    const int64_t o = (int64_t)blockIdx.y * hw + s;
    const unsigned long long *__restrict__ kp = keys + (int64_t)blockIdx.y * hw;
    const unsigned hw_s = (unsigned)V.Hs * (unsigned)V.Ws;
    const unsigned long long key = kp[s];
    float val[4];
    point_of(key, hw_s, rgb_ptrs, F, val);
    if (key == KEY_CLEAR && hole_fill) {
        const int y = (int)(s / V.W), x = (int)(s - (int64_t)y * V.W);
        float win[4][9];
#pragma unroll
        for (int dy = -1; dy <= 1; ++dy)
#pragma unroll
            for (int dx = -1; dx <= 1; ++dx) {
                const int yy = y + dy, xx = x + dx, k = (dy + 1) * 3 + dx + 1;
                const bool in = yy >= 0 && yy < V.H && xx >= 0 && xx < V.W;
                float pt[4];
                point_of(in ? kp[(int64_t)yy * V.W + xx] : KEY_CLEAR, hw_s, rgb_ptrs, F, pt);
#pragma unroll
                for (int ch = 0; ch < 4; ++ch) win[ch][k] = pt[ch];
            }
#pragma unroll
        for (int ch = 0; ch < 4; ++ch) val[ch] = fifth_of_9(win[ch]);
    }
    depth[o] = val[3];
    if (index) index[o] = key == KEY_CLEAR ? -1 : (int32_t)(unsigned)(key & 0xffffffffull);
#pragma unroll
    for (int ch = 0; ch < 3; ++ch) {
        if (rgb) rgb[o * 3 + ch] = val[ch];
        if (rgb_u8) rgb_u8[o * 3 + ch] = (uint8_t)(unsigned)val[ch];          // an integer in 0..255 already
    }
}

}  // namespace

extern "C" int64_t sgam_points_render_rgbd_workspace_bytes(int32_t P, int32_t H, int32_t W, int32_t hole_fill) {
    if (P < 1 || P > 65535 || H <= 0 || W <= 0 || (int64_t)H * W >= (1ll << 31) || (hole_fill != 0 && hole_fill != 1)) return SGAM_EINVAL;
    return (int64_t)P * H * W * 8;            // the keys; the fill reads its window from them (no second image)
}

extern "C" int sgam_points_render_rgbd_f32(const void *depth_ptrs, const void *rgb_ptrs, int32_t F, int32_t Hs, int32_t Ws,
                                           const float *Kinv_src, const float *T_rel, int32_t P, int32_t H, int32_t W, float fx, float fy,
                                           float cx, float cy, float z_near, float z_far, int32_t radius, int32_t hole_fill,
                                           float *depth_out, float *rgb_out, uint8_t *rgb_u8_out, int32_t *index_out, void *workspace,
                                           int64_t workspace_bytes, void *stream) {
    if (!depth_ptrs || !rgb_ptrs || !Kinv_src || !T_rel || !depth_out || F < 1 || Hs <= 0 || Ws <= 0 ||
        (int64_t)F * Hs * Ws >= (1ll << 32) ||                   // point id = f * Hs * Ws + q in 32 bits
        radius < 0 || radius > 2 || !(z_near > 0.f) || !(z_far > z_near))
        return SGAM_EINVAL;
    const int64_t need = sgam_points_render_rgbd_workspace_bytes(P, H, W, hole_fill);
    if (need < 0) return SGAM_EINVAL;
    if (!workspace || workspace_bytes < need || ((uintptr_t)workspace & 7)) return SGAM_EINVAL;
    PointView V;
    for (int i = 0; i < 9; ++i) V.kinv[i] = Kinv_src[i];
    V.fx = fx; V.fy = fy; V.cx = cx; V.cy = cy; V.zn = z_near; V.zf = z_far;
    V.Hs = Hs; V.Ws = Ws; V.H = H; V.W = W; V.radius = radius;
    hipStream_t s = sgam_stream(stream);
    unsigned long long *keys = (unsigned long long *)workspace;
    const int64_t hw = (int64_t)H * W, n = hw * P, hw_s = (int64_t)Hs * Ws;
    SGAM_KLAUNCH(points_keyclear_kernel, dim3((unsigned)std::min<int64_t>((n + 255) / 256, 1 << 16)), dim3(256), 0, s, keys, n);
    SGAM_KLAUNCH(points_project_kernel, dim3((unsigned)((hw_s + 255) / 256), (unsigned)std::min(F, 65535), P), dim3(256), 0, s, V,
                 (const float *const *)depth_ptrs, F, T_rel, keys);
    SGAM_KLAUNCH(points_resolve_kernel, dim3((unsigned)((hw + 255) / 256), P), dim3(256), 0, s, V, (const uint8_t *const *)rgb_ptrs, F,
                 hole_fill, keys, depth_out, rgb_out, rgb_u8_out, index_out);
    SGAM_LAUNCH_CHECK();
    return SGAM_OK;
}
