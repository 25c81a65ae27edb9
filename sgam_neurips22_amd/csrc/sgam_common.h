// Shared helpers for the gfx950 kernels of libsgam_hip.so.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/sgam_hip.h"

#define SGAM_LAUNCH_CHECK()                          \
    do {                                             \
        hipError_t e__ = hipGetLastError();          \
        if (e__ != hipSuccess) return (int)e__;      \
    } while (0)

static inline hipStream_t sgam_stream(void *s) { return (hipStream_t)s; }

// ---- in-library kernel timeline (sgam_prof_* in include/sgam_hip.h; implemented in layout.hip) ----
// Every kernel launch of the library goes through SGAM_KLAUNCH.  When profiling is enabled (bench.py's untimed
// roofline pass, never inside a captured graph) the launch is bracketed by two HIP events recorded on the launch
// stream, tagged with the kernel's name as written at the launch site (+ the enclosing function's signature, which
// resolves symbolic template arguments) and the algorithmic work announced through sgam_i_prof_work().
extern "C" int sgam_i_prof_on;
extern "C" void sgam_i_prof_begin(const char *kernel, const char *where, hipStream_t s);
extern "C" void sgam_i_prof_end(hipStream_t s);
extern "C" void sgam_i_prof_work(double flops, double bytes);
extern "C" void sgam_i_prof_shape(int m, int n, int k, int ksplit);
#define SGAM_KLAUNCH(kern, grid, blk, shm, st, ...)                            \
    do {                                                                       \
        if (sgam_i_prof_on) sgam_i_prof_begin(#kern, __PRETTY_FUNCTION__, st); \
        hipLaunchKernelGGL(kern, grid, blk, shm, st, __VA_ARGS__);             \
        if (sgam_i_prof_on) sgam_i_prof_end(st);                               \
    } while (0)
static inline int sgam_cdiv(int64_t a, int64_t b) { return (int)((a + b - 1) / b); }
static inline bool sgam_aligned16(const void *p) { return (((uintptr_t)p) & 15u) == 0; }

// ---- split-fp32 range guard (sgam_f32x_set_range_flag): a device int32 the split-fp32 kernels OR 1 into when a result
// is not finite — which is what an activation beyond fp16's range (|x| >= 65520 -> inf in the hi half) turns into.
extern "C" int32_t *sgam_i_range_flag;
__device__ __forceinline__ bool sgam_not_finite(float t) { return !(__builtin_fabsf(t) <= 3.4028234663852886e38f); }

typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef float f32x16 __attribute__((ext_vector_type(16)));

// CDNA wavefront = 64 lanes.
#define SGAM_WAVE 64

__device__ __forceinline__ float sgam_wave_sum(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}
// fp64 sum over the 64 lanes on the DPP data path (row shifts, then the two row broadcasts of wave64): six dependent
// steps of a few cycles each, where the butterfly of ds_bpermute exchanges costs 24 LDS round trips.  Fixed order:
// inclusive scan inside each row of 16, rows 0+1 / 2+3 joined by row_bcast:15, the halves by row_bcast:31; the total
// (lane 63) is returned to every lane.
template <int CTRL, int ROW_MASK>
__device__ __forceinline__ double sgam_dpp_add_f64(double v) {
    const long long b = __builtin_bit_cast(long long, v);
    const int lo = __builtin_amdgcn_update_dpp(0, (int)b, CTRL, ROW_MASK, 0xf, true);
    const int hi = __builtin_amdgcn_update_dpp(0, (int)(b >> 32), CTRL, ROW_MASK, 0xf, true);
    const double o = __builtin_bit_cast(double, ((long long)hi << 32) | (unsigned)lo);
    return v + o;            // lanes outside the row mask / without a source read 0.0
}
__device__ __forceinline__ double sgam_wave_sum_f64(double v) {
    v = sgam_dpp_add_f64<0x111, 0xf>(v);      // row_shr:1
    v = sgam_dpp_add_f64<0x112, 0xf>(v);      // row_shr:2
    v = sgam_dpp_add_f64<0x114, 0xf>(v);      // row_shr:4
    v = sgam_dpp_add_f64<0x118, 0xf>(v);      // row_shr:8   -> lane 15 of every row holds the row total
    v = sgam_dpp_add_f64<0x142, 0xa>(v);      // row_bcast:15 into rows 1 and 3
    v = sgam_dpp_add_f64<0x143, 0xc>(v);      // row_bcast:31 into rows 2 and 3
    const long long t = __builtin_bit_cast(long long, v);
    const int lo = __builtin_amdgcn_readlane((int)t, 63), hi = __builtin_amdgcn_readlane((int)(t >> 32), 63);
    return __builtin_bit_cast(double, ((long long)hi << 32) | (unsigned)lo);
}
__device__ __forceinline__ float sgam_wave_max(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o, 64));
    return v;
}

// Philox4x32-10 (Salmon et al., SC'11), all four output words: counter (c[0..3]) in, words out, key (k0, k1).  The generators of
// vq.hip and kmeans.hip are this with only word 0 kept; tests/sampler_oracle.py restates it in integers.
__device__ __forceinline__ void sgam_philox4x32_10(uint32_t (&c)[4], uint32_t k0, uint32_t k1) {
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        const uint32_t hi0 = __umulhi(0xD2511F53u, c[0]), lo0 = 0xD2511F53u * c[0];
        const uint32_t hi1 = __umulhi(0xCD9E8D57u, c[2]), lo1 = 0xCD9E8D57u * c[2];
        c[0] = hi1 ^ c[1] ^ k0;
        c[1] = lo1;
        c[2] = hi0 ^ c[3] ^ k1;
        c[3] = lo0;
        k0 += 0x9E3779B9u;
        k1 += 0xBB67AE85u;
    }
}

// swish(x) = x * sigmoid(x) on the hardware transcendentals: sigmoid = rcp(1 + exp2(-x*log2e)).
// v_exp_f32 / v_rcp_f32 are 1-ulp instructions; the result differs from the libm-based expression of the
// reference by a few 1e-7 relative — far inside the 1e-4 fp32 parity budget — at ~1/5 of the VALU cost,
// which is what lets the fused GroupNorm prologue hide behind the MFMA stream.
__device__ __forceinline__ float sgam_swish(float v) {
    const float e = __builtin_amdgcn_exp2f(v * -1.4426950408889634f);
    return v * __builtin_amdgcn_rcpf(1.0f + e);
}
