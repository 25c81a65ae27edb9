// Training data path: what the reference's datasets do to a decoded frame on the host, on the device.
//   sgam_resize_lanczos_u8   Pillow's uint8 LANCZOS resize, bit for bit: two separable fixed-point passes (horizontal first, uint8
//                            intermediate, then vertical), int32 coefficients with 22 fractional bits computed by the host, each
//                            output clip((2^21 + sum pixel * k) >> 22, 0, 255).  No floating point in the kernel; the fp32 result is
//                            a 256-entry table look-up (lut[u] = float32(u / 127.5 - 1.0)).
//   sgam_resize_nearest_f32  F.interpolate(mode='nearest') of depth maps, with the 65504 -> -99999 rewrite and the != 65504 mask.
//   sgam_resize_bicubic_u8   the same two passes over the host's BICUBIC tables (Image.resize's default filter, what the codebook
//                            phase's single-frame dataset calls), fp32 only, into an interleaved output of 3 or 4 floats a pixel.
//   sgam_frame_depth_codec_f32  that dataset's depth channel: nearest resize, then its inverse-depth arithmetic with every
//                            operation rounded on its own in the precision numpy used (half, fp32, or fp64 with ray -> z).
// One workgroup per output tile: the input patch the tile needs is staged in LDS with 16-byte global loads, the horizontal pass
// writes a uint8 tile to LDS, the vertical pass reads it from there — the intermediate image never reaches HBM.
#include "sgam_common.h"

namespace {

constexpr int kPrec = 22;                   // Pillow's PRECISION_BITS for 8-bit channels (32 - 8 - 2)
constexpr int kThreads = 256;
constexpr int kLdsBudget = 64 * 1024;

__device__ __forceinline__ int clip8(int acc) {
    const int v = acc >> kPrec;             // arithmetic shift, like the reference's C
    return v < 0 ? 0 : (v > 255 ? 255 : v);
}

struct LanczosLds {                         // byte offsets into the dynamic LDS block, fixed by the host for the chosen tile
    int hk, vk, patch, inter;               // int32 [TW][KH] | int32 [TH][KV] | uint8 [PH][pitch_p] | uint8 [PH][pitch_i]
    int pitch_p, pitch_i;
};

__global__ __launch_bounds__(kThreads) void lanczos_u8_kernel(
    const uint8_t *__restrict__ src, int64_t src_bytes, int Hin, int Win, int Hout, int Wout,
    const int2 *__restrict__ hb, const int32_t *__restrict__ hk, int KH,
    const int2 *__restrict__ vb, const int32_t *__restrict__ vk, int KV,
    int TH, int TW, int PH, int PW, LanczosLds L, const float *__restrict__ lut,
    uint8_t *__restrict__ out_u8, float *__restrict__ out_f32, int fstride) {
    extern __shared__ uint4 smem_v[];
    uint8_t *smem = reinterpret_cast<uint8_t *>(smem_v);
    int32_t *s_hk = reinterpret_cast<int32_t *>(smem + L.hk);
    int32_t *s_vk = reinterpret_cast<int32_t *>(smem + L.vk);
    uint8_t *s_patch = smem + L.patch;
    uint8_t *s_inter = smem + L.inter;

    const int tid = threadIdx.x, m = blockIdx.z;
    const int ox0 = blockIdx.x * TW, oy0 = blockIdx.y * TH;
    const int tw = min(TW, Wout - ox0), th = min(TH, Hout - oy0);
    // the input window of this tile: bounds are non-decreasing along an axis (validated by the host), so first and last suffice
    const int2 hb0 = hb[ox0], hb1 = hb[ox0 + tw - 1], vb0 = vb[oy0], vb1 = vb[oy0 + th - 1];
    const int ix0 = min(max(hb0.x, 0), Win - 1), iy0 = min(max(vb0.x, 0), Hin - 1);
    const int pw = min(min(hb1.x + hb1.y, Win) - ix0, PW), ph = min(min(vb1.x + vb1.y, Hin) - iy0, PH);

    for (int i = tid; i < tw * KH; i += kThreads) s_hk[i] = hk[(int64_t)ox0 * KH + i];
    for (int i = tid; i < th * KV; i += kThreads) s_vk[i] = vk[(int64_t)oy0 * KV + i];

    // ---- stage the patch: every row as whole 16-byte vectors from its aligned-down address (rows of a 3-byte pixel image start
    // anywhere); a vector that would leave the source buffer is assembled from guarded byte loads instead
    const uintptr_t buf0 = reinterpret_cast<uintptr_t>(src), buf1 = buf0 + (uintptr_t)src_bytes;
    const uintptr_t img = buf0 + (uintptr_t)m * Hin * Win * 3;
    const int nvec = L.pitch_p >> 4;
    for (int i = tid; i < ph * nvec; i += kThreads) {
        const int r = i / nvec, v = i - r * nvec;
        const uintptr_t row = img + ((uintptr_t)(iy0 + r) * Win + ix0) * 3;
        const uintptr_t va = (row & ~(uintptr_t)15) + 16u * v;
        if (va >= row + (uintptr_t)pw * 3) continue;
        uint4 d;
        if (va >= buf0 && va + 16 <= buf1) {
            d = *reinterpret_cast<const uint4 *>(va);
        } else {
            uint32_t w[4] = {0, 0, 0, 0};
            for (int b = 0; b < 16; ++b) {
                const uintptr_t a = va + b;
                if (a >= buf0 && a < buf1) w[b >> 2] |= (uint32_t)(*reinterpret_cast<const uint8_t *>(a)) << (8 * (b & 3));
            }
            d = make_uint4(w[0], w[1], w[2], w[3]);
        }
        *reinterpret_cast<uint4 *>(s_patch + r * L.pitch_p + 16 * v) = d;
    }
    __syncthreads();

    // ---- horizontal pass: patch -> uint8 tile [ph][tw * 3]
    const int tw3 = tw * 3;
    for (int i = tid; i < ph * tw3; i += kThreads) {
        const int r = i / tw3, q = i - r * tw3, ox = q / 3, c = q - ox * 3;
        const int2 b = hb[ox0 + ox];
        const int x = max(b.x - ix0, 0), taps = min(min(b.y, KH), pw - x);
        const int shift = (int)((img + ((uintptr_t)(iy0 + r) * Win + ix0) * 3) & 15u);
        const uint8_t *p = s_patch + r * L.pitch_p + shift + x * 3 + c;
        const int32_t *k = s_hk + ox * KH;
        int acc = 1 << (kPrec - 1);
        for (int t = 0; t < taps; ++t) acc += (int)p[3 * t] * k[t];
        s_inter[r * L.pitch_i + q] = (uint8_t)clip8(acc);
    }
    __syncthreads();

    // ---- vertical pass: uint8 tile -> output (uint8 and / or fp32 through the table)
    for (int i = tid; i < th * tw3; i += kThreads) {
        const int oy = i / tw3, q = i - oy * tw3;
        const int2 b = vb[oy0 + oy];
        const int y = max(b.x - iy0, 0), taps = min(min(b.y, KV), ph - y);
        const uint8_t *p = s_inter + y * L.pitch_i + q;
        const int32_t *k = s_vk + oy * KV;
        int acc = 1 << (kPrec - 1);
        for (int t = 0; t < taps; ++t) acc += (int)p[t * L.pitch_i] * k[t];
        const int v = clip8(acc);
        const int64_t px = ((int64_t)m * Hout + oy0 + oy) * Wout + ox0;
        if (out_u8) out_u8[px * 3 + q] = (uint8_t)v;
        if (out_f32) {                      // fstride floats a pixel: 3 = dense RGB, 4 = the RGB channels of an RGB-D batch tensor
            const int ox = q / 3;
            out_f32[(px + ox) * fstride + (q - ox * 3)] = lut[v];
        }
    }
}

// same size in, same size out: the table conversion alone (the CLEVR case), four values per thread
__global__ __launch_bounds__(kThreads) void u8_table_kernel(const uint8_t *__restrict__ src, int64_t n, const float *__restrict__ lut,
                                                           uint8_t *__restrict__ out_u8, float *__restrict__ out_f32, int fstride) {
    const int64_t i0 = ((int64_t)blockIdx.x * kThreads + threadIdx.x) * 4;
    for (int j = 0; j < 4; ++j) {
        const int64_t i = i0 + j;
        if (i >= n) return;
        const uint8_t v = src[i];
        if (out_u8) out_u8[i] = v;
        if (out_f32) out_f32[(i / 3) * fstride + i % 3] = lut[v];
    }
}

__global__ __launch_bounds__(kThreads) void nearest_f32_kernel(const float *__restrict__ src, int M, int Hin, int Win, int Hout, int Wout,
                                                              float scale_h, float scale_w, float *__restrict__ out, int replace,
                                                              float sentinel, float replacement, float *__restrict__ mask) {
    const int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    const int64_t n = (int64_t)M * Hout * Wout;
    if (i >= n) return;
    const int x = (int)(i % Wout), y = (int)((i / Wout) % Hout), m = (int)(i / ((int64_t)Wout * Hout));
    // F.interpolate(mode='nearest'): min(int(floorf(dst * scale)), in - 1), scale = (float)in / out
    const int sy = min((int)floorf((float)y * scale_h), Hin - 1), sx = min((int)floorf((float)x * scale_w), Win - 1);
    float v = src[((int64_t)m * Hin + sy) * Win + sx];
    if (mask) mask[i] = (v != sentinel) ? 1.0f : 0.0f;
    if (replace && v == sentinel) v = replacement;
    if (out) out[i] = v;
}

// the single-frame dataset's depth arithmetic (data/base.py:76-88, 104-115).  The constants come from the host already rounded to
// the precision of the mode; every operation below is one IEEE operation of that precision (the TU builds with -ffp-contract=off).
struct CodecConsts {
    double add, sub, div;                   // d + add (GoogleEarth: 10), (1 / d - sub) / div
    double k00, k00sq, k02, k12;            // fp64 mode: z = d * k00 / sqrt(k00sq + (k02 - y - 0.5)^2 + (k12 - x - 0.5)^2)
};
enum { kCodecHalf = 0, kCodecF32 = 1, kCodecF64Ray = 2 };

__device__ __forceinline__ float rh(float v) { return (float)(_Float16)v; }     // round to half, nearest even (subnormals kept)
// hides from the optimiser that a value is a half in fp32 clothes: it would otherwise narrow `rh(1.0f / t)` to the half-precision
// reciprocal instruction, which is not correctly rounded
__device__ __forceinline__ float opaque(float v) {
    asm volatile("" : "+v"(v));
    return v;
}

__global__ __launch_bounds__(kThreads) void depth_codec_kernel(const float *__restrict__ src, int M, int Hin, int Win, int Hout, int Wout,
                                                              float scale_h, float scale_w, int mode, CodecConsts c,
                                                              float *__restrict__ out, int stride, int channel) {
    const int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    const int64_t n = (int64_t)M * Hout * Wout;
    if (i >= n) return;
    const int x = (int)(i % Wout), y = (int)((i / Wout) % Hout), m = (int)(i / ((int64_t)Wout * Hout));
    const int sy = min((int)floorf((float)y * scale_h), Hin - 1), sx = min((int)floorf((float)x * scale_w), Win - 1);
    const float d = src[((int64_t)m * Hin + sy) * Win + sx];
    float r;
    if (mode == kCodecHalf) {               // half operands are exact in fp32, and fp32 -> half of one +, -, *, / rounds once
        const float t = rh(d + (float)c.add);
        const float inv = rh(1.0f / opaque(t));
        const float s = rh(opaque(rh(inv - (float)c.sub)) / (float)c.div);
        r = rh(rh(2.0f * s) - 1.0f);
    } else if (mode == kCodecF32) {
        const float t = d + (float)c.add;
        const float inv = 1.0f / t;
        const float s = (inv - (float)c.sub) / (float)c.div;
        r = 2.0f * s - 1.0f;
    } else {
        const double a = (c.k02 - (double)y) - 0.5, b = (c.k12 - (double)x) - 0.5;   // K02 with the row, K12 with the column
        const double z = ((double)d * c.k00) / sqrt((c.k00sq + a * a) + b * b);
        const double inv = 1.0 / z;
        const double s = (inv - c.sub) / c.div;
        r = (float)(2.0 * s - 1.0);
    }
    out[i * stride + channel] = r;
}

// bounds of one axis as the host computed them: inside the input, at most K taps, non-decreasing (what the kernel's window relies on)
bool bounds_ok(const int32_t *b, int n_out, int n_in, int K) {
    int px = 0, pe = 0;
    for (int i = 0; i < n_out; ++i) {
        const int x = b[2 * i], t = b[2 * i + 1];
        if (x < 0 || t < 1 || t > K || x + t > n_in || x < px || x + t < pe) return false;
        px = x;
        pe = x + t;
    }
    return true;
}

// largest input extent any tile of T outputs needs
int max_extent(const int32_t *b, int n_out, int T) {
    int e = 0;
    for (int i0 = 0; i0 < n_out; i0 += T) {
        const int i1 = (i0 + T < n_out ? i0 + T : n_out) - 1;
        const int w = b[2 * i1] + b[2 * i1 + 1] - b[2 * i0];
        e = w > e ? w : e;
    }
    return e;
}

int round_up(int v, int m) { return (v + m - 1) / m * m; }

// the two-pass resize over whichever filter's tables the host computed; `fstride` floats per pixel in out_f32
int resize_u8_tables(const uint8_t *src, int32_t M, int32_t Hin, int32_t Win, int32_t Hout, int32_t Wout,
                     const int32_t *hbounds_host, const int32_t *hbounds, const int32_t *hcoef, int32_t KH,
                     const int32_t *vbounds_host, const int32_t *vbounds, const int32_t *vcoef, int32_t KV,
                     const float *lut256, uint8_t *out_u8, float *out_f32, int fstride, void *stream) {
    if (!src || M <= 0 || Hin <= 0 || Win <= 0 || Hout <= 0 || Wout <= 0 || M > 65535) return SGAM_EINVAL;
    if (!out_u8 && !out_f32) return SGAM_EINVAL;
    if (out_f32 && !lut256) return SGAM_EINVAL;
    if ((int64_t)Hin * Win * 3 > INT32_MAX || (int64_t)Hout * Wout * 3 > INT32_MAX) return SGAM_EINVAL;
    hipStream_t st = sgam_stream(stream);
    if (Hin == Hout && Win == Wout) {
        const int64_t n = (int64_t)M * Hin * Win * 3;
        SGAM_KLAUNCH(u8_table_kernel, dim3(sgam_cdiv(n, kThreads * 4)), dim3(kThreads), 0, st, src, n, lut256, out_u8, out_f32, fstride);
        SGAM_LAUNCH_CHECK();
        return SGAM_OK;
    }
    if (!hbounds_host || !hbounds || !hcoef || !vbounds_host || !vbounds || !vcoef || KH < 1 || KV < 1) return SGAM_EINVAL;
    if (!bounds_ok(hbounds_host, Wout, Win, KH) || !bounds_ok(vbounds_host, Hout, Hin, KV)) return SGAM_EINVAL;
    // the largest tile whose patch, intermediate tile and coefficients fit the LDS budget
    static const int tiles[][2] = {{32, 32}, {16, 32}, {16, 16}, {8, 16}, {8, 8}, {4, 8}, {4, 4}, {2, 4}, {1, 4}, {1, 2}, {1, 1}};
    for (const auto &t : tiles) {
        const int TH = t[0], TW = t[1];
        const int PH = max_extent(vbounds_host, Hout, TH), PW = max_extent(hbounds_host, Wout, TW);
        LanczosLds L;
        L.pitch_p = round_up(15 + PW * 3, 16);
        L.pitch_i = round_up(TW * 3, 4);
        L.hk = 0;
        L.vk = L.hk + TW * KH * 4;
        L.patch = round_up(L.vk + TH * KV * 4, 16);
        L.inter = L.patch + PH * L.pitch_p;
        const int64_t bytes = (int64_t)L.inter + (int64_t)PH * L.pitch_i;
        if (bytes > kLdsBudget) continue;
        const dim3 grid(sgam_cdiv(Wout, TW), sgam_cdiv(Hout, TH), M);
        if (grid.y > 65535) return SGAM_EINVAL;
        SGAM_KLAUNCH(lanczos_u8_kernel, grid, dim3(kThreads), (size_t)bytes, st, src, (int64_t)M * Hin * Win * 3, Hin, Win, Hout, Wout,
                     reinterpret_cast<const int2 *>(hbounds), hcoef, KH, reinterpret_cast<const int2 *>(vbounds), vcoef, KV, TH, TW, PH,
                     PW, L, lut256, out_u8, out_f32, fstride);
        SGAM_LAUNCH_CHECK();
        return SGAM_OK;
    }
    return SGAM_EINVAL;         // a single output's taps do not fit in LDS (reduction far beyond anything the datasets ask for)
}

}  // namespace

extern "C" int sgam_resize_lanczos_u8(const uint8_t *src, int32_t M, int32_t Hin, int32_t Win, int32_t Hout, int32_t Wout,
                                      const int32_t *hbounds_host, const int32_t *hbounds, const int32_t *hcoef, int32_t KH,
                                      const int32_t *vbounds_host, const int32_t *vbounds, const int32_t *vcoef, int32_t KV,
                                      const float *lut256, uint8_t *out_u8, float *out_f32, void *stream) {
    return resize_u8_tables(src, M, Hin, Win, Hout, Wout, hbounds_host, hbounds, hcoef, KH, vbounds_host, vbounds, vcoef, KV, lut256,
                            out_u8, out_f32, 3, stream);
}

extern "C" int sgam_resize_bicubic_u8(const uint8_t *src, int32_t M, int32_t Hin, int32_t Win, int32_t Hout, int32_t Wout,
                                      const int32_t *hbounds_host, const int32_t *hbounds, const int32_t *hcoef, int32_t KH,
                                      const int32_t *vbounds_host, const int32_t *vbounds, const int32_t *vcoef, int32_t KV,
                                      const float *lut256, float *out_f32, int32_t pixel_stride, void *stream) {
    if (!out_f32 || (pixel_stride != 3 && pixel_stride != 4)) return SGAM_EINVAL;
    return resize_u8_tables(src, M, Hin, Win, Hout, Wout, hbounds_host, hbounds, hcoef, KH, vbounds_host, vbounds, vcoef, KV, lut256,
                            nullptr, out_f32, pixel_stride, stream);
}

extern "C" int sgam_resize_nearest_f32(const float *src, int32_t M, int32_t Hin, int32_t Win, int32_t Hout, int32_t Wout, float *out,
                                       int32_t replace, float sentinel, float replacement, float *mask_out, void *stream) {
    if (!src || (!out && !mask_out) || M <= 0 || Hin <= 0 || Win <= 0 || Hout <= 0 || Wout <= 0) return SGAM_EINVAL;
    const int64_t n = (int64_t)M * Hout * Wout;
    if (n > (int64_t)INT32_MAX * kThreads) return SGAM_EINVAL;
    const float scale_h = (float)Hin / (float)Hout, scale_w = (float)Win / (float)Wout;
    SGAM_KLAUNCH(nearest_f32_kernel, dim3(sgam_cdiv(n, kThreads)), dim3(kThreads), 0, sgam_stream(stream), src, M, Hin, Win, Hout, Wout,
                 scale_h, scale_w, out, replace, sentinel, replacement, mask_out);
    SGAM_LAUNCH_CHECK();
    return SGAM_OK;
}

extern "C" int sgam_frame_depth_codec_f32(const float *src, int32_t M, int32_t Hin, int32_t Win, int32_t Hout, int32_t Wout, int32_t mode,
                                          const double *consts7, float *out, int32_t pixel_stride, int32_t channel, void *stream) {
    if (!src || !out || !consts7 || M <= 0 || Hin <= 0 || Win <= 0 || Hout <= 0 || Wout <= 0) return SGAM_EINVAL;
    if (mode != kCodecHalf && mode != kCodecF32 && mode != kCodecF64Ray) return SGAM_EINVAL;
    if (pixel_stride < 1 || pixel_stride > 4 || channel < 0 || channel >= pixel_stride) return SGAM_EINVAL;
    const int64_t n = (int64_t)M * Hout * Wout;
    if (n > (int64_t)INT32_MAX * kThreads) return SGAM_EINVAL;
    const CodecConsts c = {consts7[0], consts7[1], consts7[2], consts7[3], consts7[4], consts7[5], consts7[6]};
    if (c.div == 0.0) return SGAM_EINVAL;
    const float scale_h = (float)Hin / (float)Hout, scale_w = (float)Win / (float)Wout;
    SGAM_KLAUNCH(depth_codec_kernel, dim3(sgam_cdiv(n, kThreads)), dim3(kThreads), 0, sgam_stream(stream), src, M, Hin, Win, Hout, Wout,
                 scale_h, scale_w, mode, c, out, pixel_stride, channel);
    SGAM_LAUNCH_CHECK();
    return SGAM_OK;
}
