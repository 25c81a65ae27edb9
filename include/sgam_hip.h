/*
 * sgam_hip.h — C ABI of libsgam_hip.so, the MI355X (gfx950) backend of SGAM's per-step
 * generative-sensing hot path.
 *
 * Conventions (SURVEY.md §8b "lower boundary"):
 *   - extern "C", plain device pointers + sizes, no torch / C++ types;
 *   - the CALLER owns every buffer (the Python side allocates them with torch);
 *   - every call is asynchronous on `stream` (a hipStream_t passed as void*; NULL = the
 *     null stream), never synchronises, never allocates device memory;
 *   - return 0 on success, a negative SGAM_E* code on a bad argument, or a positive
 *     hipError_t if the launch itself failed;
 *   - activations inside the VQGAN are NHWC ("pixel-major") fp32: [B][H][W][C];
 *     the NCHW <-> NHWC hops at the module boundary are sgam_nchw_to_nhwc / _nhwc_to_nchw.
 *
 * Each entry point cites the reference op (file:line under /root/reference) it replaces.
 */
#ifndef SGAM_HIP_H
#define SGAM_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SGAM_OK 0
#define SGAM_EINVAL (-1)   /* bad shape / unsupported size */
#define SGAM_EALIGN (-2)   /* pointer or stride not aligned as required */
#define SGAM_EWORKSPACE (-3)

/* ABI version of this header; bumped on any signature change. */
int sgam_abi_version(void);
/* Human-readable build string ("gfx950 ... commit <c>; digest <d>"). */
const char *sgam_build_info(void);
/* (ABI v10) The build stamp alone: the last commit that touched the library's sources ("+dirty" when the tree differed), and the
 * first 12 hex digits of a sha256 over every source, header and compile flag (sgam_neurips22_amd/build.py). */
const char *sgam_build_commit(void);
const char *sgam_build_digest(void);

/* ------------------------------------------------------------------------------------------
 * Kernel timeline (measurement; no reference counterpart — the reference has no profiling).  While
 * enabled, every kernel launch of the library is bracketed by two HIP events recorded on the launch stream.  Not usable
 * inside stream capture; the caller synchronises the device before reading.  sgam_prof_get(i): kernel name as written at
 * the launch site, the enclosing function's signature (resolves symbolic template arguments), elapsed ms, and the
 * algorithmic FLOP / bytes the launch site announced (0 when it announced none).  sgam_prof_mark_empty records a
 * bracket around nothing (the cost of the bracket itself, to be subtracted).
 * ------------------------------------------------------------------------------------------ */
int sgam_prof_enable(int32_t on);
int sgam_prof_mark_empty(void *stream);
int32_t sgam_prof_count(void);
int sgam_prof_get(int32_t i, const char **kernel, const char **where, float *ms, double *flops, double *bytes);
/* GEMM view of record i where the launch site announced one: mnks[4] = {M, N, K, split-K factor}, zeros otherwise */
int sgam_prof_get_shape(int32_t i, int32_t *mnks);

/* ------------------------------------------------------------------------------------------
 * K1/K2/K3/K6 — convolution as implicit GEMM on the matrix cores (fp32-in/fp32-acc MFMA).
 * Replaces torch.nn.Conv2d in ResnetBlock/Upsample/Downsample/AttnBlock/VQModel:
 *   sgam/generative_sensing_module/modules/diffusionmodules/model.py:43-53 (nearest x2 + 3x3),
 *   :63-75 (pad (0,1,0,1) + 3x3 stride 2), :88-116 (3x3 / 1x1 nin_shortcut), :146-165 (1x1 q,k,v,proj)
 *   sgam/generative_sensing_module/model.py:54,62,63 (1x1 conv_in, quant_conv, post_quant_conv).
 *
 *   out[m][n] = bias[n] + residual[m][n] + sum_{ky,kx,c} X[b][iy][ix][c] * Wp[n][(ky*KW+kx)*Cin + c]
 *   with m = (b*Ho + oy)*Wo + ox, iy = oy*stride + ky - pad_t, ix = ox*stride + kx - pad_l,
 *   zero outside the (logical) input; when `upsample2x` != 0 the logical input is the nearest-
 *   neighbour 2x enlargement of the physical [Hi][Wi] map (X[b][iy>>1][ix>>1]).
 *
 *   x        [B][Hi][Wi] pixels, `lda` floats apart, first Cin floats used (Cin % 4 == 0; 32-wide K slabs, ragged tail masked)
 *   w_packed [N] rows, `ldb` floats apart, K = KH*KW*Cin contiguous (see sgam_pack_conv_weight)
 *   bias     [N] or NULL;  residual [M] rows `ldr` apart or NULL
 *   out      [M] rows `ldc` apart; only columns n < n_valid are written
 *   workspace: sgam_conv2d_workspace_bytes(...) bytes (split-K partial sums), may be NULL if 0.
 * ------------------------------------------------------------------------------------------ */
typedef struct sgam_conv_desc {
    int32_t B, Hi, Wi, Cin;       /* physical input */
    int32_t Ho, Wo, N;            /* output spatial size and channel count */
    int32_t KH, KW, stride;
    int32_t pad_t, pad_l;         /* top/left zero padding (bottom/right implied by Ho/Wo) */
    int32_t upsample2x;           /* 1: fuse F.interpolate(scale 2, nearest) in front of the conv */
    int32_t lda, ldb, ldc, ldr;   /* row strides in floats of x, w_packed, out, residual */
    int32_t n_valid;              /* columns actually stored (<= N) */
    int32_t bias_per_row;         /* 0: bias[n]; 1: bias[m] (used for the transposed V projection) */
    /* optional plan override (autotuner, sgam_neurips22_amd/tune.py); 0 = built-in heuristic.
     * (plan_bm, plan_bn) in {(128,128), (64,128), (64,64)}; plan_ksplit >= 1. */
    int32_t plan_bm, plan_bn, plan_ksplit;
} sgam_conv_desc;

int64_t sgam_conv2d_workspace_bytes(const sgam_conv_desc *d);
/* which kernel instantiation a descriptor maps to: workgroup tile BMxBN and split-K factor (for profiling). */
int sgam_conv2d_plan(const sgam_conv_desc *d, int32_t *bm, int32_t *bn, int32_t *ksplit);
int sgam_conv2d_nhwc_f32(const sgam_conv_desc *d, const float *x, const float *w_packed,
                         const float *bias, const float *residual, float *out, void *workspace,
                         int64_t workspace_bytes, void *stream);
/* Same, with the GroupNorm(+swish) of the INPUT fused into the operand staging (ResnetBlock norm1/norm2,
 * AttnBlock.norm, norm_out: diffusionmodules/model.py:119-127, 170, 429-430, 536-537): x is the RAW activation,
 * gn_scale_shift the [B][Cin][2] table of sgam_groupnorm_stats_nhwc_f32 (NULL = plain conv), gn_swish 0/1.
 * Zero padding stays zero (it pads the normalised map, as in the reference). */
int sgam_conv2d_gn_nhwc_f32(const sgam_conv_desc *d, const float *x, const float *gn_scale_shift,
                            int32_t gn_swish, const float *w_packed, const float *bias, const float *residual,
                            float *out, void *workspace, int64_t workspace_bytes, void *stream);

/* [Cout][Cin][KH][KW] (torch Conv2d.weight) -> [Cout_pad][KH*KW][Cin_pad], zero padded. */
int sgam_pack_conv_weight(const float *w_oihw, float *w_packed, int32_t Cout, int32_t Cin, int32_t KH,
                          int32_t KW, int32_t Cout_pad, int32_t Cin_pad, void *stream);

/* ------------------------------------------------------------------------------------------
 * "Split" fp32 path (conv_f32x.hip): the same fp32 convolution / GEMM as sgam_conv2d_nhwc_f32 (same descriptor, fp32
 * activations in and out) evaluated on the fp16 matrix cores with fp32-class accuracy: every operand is split
 * exactly into hi + lo fp16 pieces and a.b = a_hi.b_hi + a_hi.b_lo + a_lo.b_hi is accumulated in fp32 (products of
 * fp16 values are exact in fp32; the dropped term is <= 2^-22 |a||b|).  Held to the same parity tests as the
 * fp32-MFMA path.  Weights are pre-split by sgam_pack_conv_weight_f32x into fp16 hi / lo halves of w_scale * w
 * (w_scale a power of two lifting max|w| into (512, 1024]) stored in MFMA-fragment order: [N / 32][ldb / 32][256][8]
 * halfs, per (32-row tile, 32-element K slab) 256 pieces of 16 bytes with piece = ((plane * 2 + k-step) * 2 + k-half)
 * * 32 + row (plane 0 = hi, 1 = lo; k-step = 16 elements, k-half = 8), so the B operand of one
 * v_mfma_f32_32x32x16_f16 is one contiguous kilobyte (N rounded up to 32 rows); activations are split while staged,
 * after multiplication by the power of two a_scale (1 for ordinary activations, 1024 for softmax probabilities).
 * ldb = K elements per row, % 32 == 0 (the buffer holds 2 * ldb halfs per row of the 32-row-padded matrix); Cin % 8 == 0, and % 32 == 0 when
 * KH * KW > 1; |a_scale * x| must stay below 65504.
 * ------------------------------------------------------------------------------------------ */
/* Range guard of the split path.  An activation with |a_scale * x| >= 65520 becomes inf in its fp16 hi half, and the
 * output it feeds becomes inf / NaN.  Every split-fp32 kernel that produces final outputs (conv / GEMM epilogue, split-K
 * combine, fused-attention combine) ORs 1 into *device_flag when it writes a non-finite value.  The caller owns the int32
 * (zero it, read it at a synchronisation point); on 1 the results since the last check are invalid in this mode and
 * must be recomputed on the fp32-in MFMA path (sgam_conv2d_nhwc_f32), which has no range precondition — the Python
 * side does exactly that (VQModel.forward, InfiniteSceneGeneration.scene_expansion).  NULL (default) disables the
 * reporting.  This pointer is the library's only mutable global: one flag per process (= per GPU). */
int sgam_f32x_set_range_flag(int32_t *device_flag);
int64_t sgam_conv2d_f32x_workspace_bytes(const sgam_conv_desc *d);
int sgam_conv2d_f32x_plan(const sgam_conv_desc *d, int32_t *bm, int32_t *bn, int32_t *ksplit);
int sgam_conv2d_nhwc_f32x(const sgam_conv_desc *d, const float *x, float a_scale, const void *w_planes,
                          float w_scale, const float *bias, const float *residual, float *out, void *workspace,
                          int64_t workspace_bytes, void *stream);
int sgam_pack_conv_weight_f32x(const float *w_oihw, void *w_planes, float w_scale, int32_t Cout, int32_t Cin,
                               int32_t KH, int32_t KW, int32_t Cout_pad, int32_t Cin_pad, void *stream);
/* Same convolution, additionally delivering the GroupNorm statistics of its OUTPUT (32 groups) as per-chunk {sum, sumsq}
 * partial sums: gn_partial holds [B][chunks][32][2] doubles, chunks = sgam_conv2d_f32x_stats_chunks(d) per image — one
 * per (tile, wavefront row) from the conv epilogue when the plan has no split-K, one per 1024 outputs from the split-K
 * combine otherwise; 0 = not available for this shape (N % 128 != 0, n_valid != N, tiles straddling images, N / 32 not a
 * divisor of 32 without split-K — N = 384, 768, 2048 — N not a divisor of 1024 under split-K).  sgam_groupnorm_stats_from_partials_f32 folds them (one 32-workgroup launch);
 * sgam_conv2d_f32x_stats_mode(d) = chunks > 0. */
int32_t sgam_conv2d_f32x_stats_chunks(const sgam_conv_desc *d);
int32_t sgam_conv2d_f32x_stats_mode(const sgam_conv_desc *d);
int sgam_conv2d_stats_nhwc_f32x(const sgam_conv_desc *d, const float *x, float a_scale, const void *w_planes,
                                float w_scale, const float *bias, const float *residual, float *out,
                                double *gn_partial, void *workspace, int64_t workspace_bytes, void *stream);
int sgam_groupnorm_from_partials_f32(const float *x, const double *partial, int32_t nchunk, const float *gamma,
                                     const float *beta, float *y, int32_t B, int32_t HW, int32_t C, int32_t groups,
                                     float eps, int32_t fuse_swish, void *workspace, int64_t workspace_bytes, void *stream);
/* GroupNorm(+swish) of the INPUT fused into the operand staging: x is normalised with the per-(image, group)
 * {mean, rstd} gn_mean_rstd [B][32][2] and the affine parameters gn_gamma / gn_beta [Cin] (16-byte aligned) while the
 * 3x3 kernel stages each channel slab of its input patch — once per slab, shared by the nine taps — so no normalised
 * copy of the activation is ever written.  Zero padding applies to the normalised tensor, as in Conv2d(GroupNorm(x)).
 * Available when sgam_conv2d_f32x_gn_fusable(d) == 1 (3x3, stride 1, pad 1, no upsampling, Ho % 8 == 0, Wo % 8 (16)
 * == 0, Cin % 128 == 0, a halo-kernel tile plan).  {mean, rstd} come from sgam_groupnorm_stats_from_partials_f32 (the
 * producing convolution's partial sums) or from sgam_groupnorm_meanrstd_nhwc_f32 (any tensor).
 * gn_partial as in sgam_conv2d_stats_nhwc_f32x, may be NULL. */
int32_t sgam_conv2d_f32x_gn_fusable(const sgam_conv_desc *d);
/* 1 when the descriptor runs on a halo-staged 3x3 kernel (3x3 / stride 1 / pad 1 on the input or on its nearest-2x
 * upsampling), 0 when it runs on the generic implicit-GEMM kernel (diagnostic: profiling labels) */
int32_t sgam_conv2d_f32x_uses_halo(const sgam_conv_desc *d);
int sgam_conv2d_gn_nhwc_f32x(const sgam_conv_desc *d, const float *x, const float *gn_mean_rstd, const float *gn_gamma,
                             const float *gn_beta, int32_t gn_swish, const void *w_planes, float w_scale, const float *bias,
                             const float *residual, float *out, double *gn_partial, void *workspace, int64_t workspace_bytes,
                             void *stream);
/* The same with the statistics of x still as its PRODUCER's chunk partials ([B][chunks_in][32][2] fp64 {sum, sumsq}, what
 * sgam_conv2d_stats_nhwc_f32x / the split-K combine leave): the convolution folds them itself, no fold launch in between.  Offered
 * where the fold is cheap — sgam_conv2d_f32x_gn_foldable(d, chunks_in) == 1: at most 16 chunks (the group-major combine of the
 * 16^2 / 32^2 maps leaves 8 - 16) and at most two channel slabs per workgroup. */
int32_t sgam_conv2d_f32x_gn_foldable(const sgam_conv_desc *d, int32_t chunks_in);
int sgam_conv2d_gnp_nhwc_f32x(const sgam_conv_desc *d, const float *x, const double *gn_partial_in, int32_t chunks_in, float eps,
                              const float *gn_gamma, const float *gn_beta, int32_t gn_swish, const void *w_planes, float w_scale,
                              const float *bias, const float *residual, float *out, double *gn_partial, void *workspace,
                              int64_t workspace_bytes, void *stream);
int sgam_groupnorm_stats_from_partials_f32(const double *partial, int32_t nchunk, float *mean_rstd, int32_t B, int32_t HW,
                                           int32_t C, int32_t groups, float eps, void *stream);
int sgam_groupnorm_meanrstd_nhwc_f32(const float *x, float *mean_rstd, int32_t B, int32_t HW, int32_t C, int32_t groups,
                                     float eps, void *workspace, int64_t workspace_bytes, void *stream);
/* split a row-major fp32 matrix [N][K] (row stride ld) into the fragment-ordered B-operand layout over [Np][Kp], both
 * rounded up to 32 (zero filled): the B operand when it is an activation (ldb = Kp) */
int sgam_split_rows_f32x(const float *x, void *planes, float scale, int32_t N, int32_t K, int32_t ld, void *stream);

/* ------------------------------------------------------------------------------------------
 * 16-bit THROUGHPUT path (h16.hip): the same operators on bf16 (`ht` = 0) or fp16 (`ht` = 1) activations and
 * weights, fp32 accumulation on v_mfma_f32_32x32x16_{bf16,f16}; statistics / softmax / bias / residual math in
 * fp32.  Strides (lda, ldb, ldc, ldr) are in ELEMENTS of the respective buffer; Cin % 8 == 0.  `out_f32` != 0
 * keeps the result in fp32 (attention scores, the latent handed to the fp32 quantiser, the final RGB-D).
 * Not a parity path: index agreement with the fp32 path is reported, not guaranteed.
 * ------------------------------------------------------------------------------------------ */
int64_t sgam_conv2d_h16_workspace_bytes(const sgam_conv_desc *d);
int sgam_conv2d_h16_plan(const sgam_conv_desc *d, int32_t *bm, int32_t *bn, int32_t *ksplit);
int sgam_conv2d_nhwc_h16(const sgam_conv_desc *d, int32_t ht, const void *x, const void *w_packed,
                         const float *bias, const void *residual, void *out, int32_t out_f32, void *workspace,
                         int64_t workspace_bytes, void *stream);
/* (ABI v5) The same launch with the GroupNorm statistics of the OUTPUT left as per-chunk partial sums (gn_partial
 * [B][sgam_conv2d_h16_generic_stats_chunks(d)][32][2] doubles, the layout of sgam_conv2d_h16_stats_chunks): the 1x1 / strided
 * convolutions and the attention block's proj_out (diffusionmodules/model.py:63-75, 168-192) then feed the next Normalize
 * without a statistics pass.  Available (chunks > 0) when the kernel runs whole-K workgroups with its direct epilogue:
 * n_valid == N, N % 128 == 0, even row strides, no per-row bias, Ho * Wo a multiple of half the tile's rows. */
int32_t sgam_conv2d_h16_generic_stats_chunks(const sgam_conv_desc *d);
int sgam_conv2d_stats_nhwc_h16(const sgam_conv_desc *d, int32_t ht, const void *x, const void *w_packed, const float *bias,
                               const void *residual, void *out, int32_t out_f32, double *gn_partial, void *workspace,
                               int64_t workspace_bytes, void *stream);
/* The 3x3 / stride 1 / pad 1 convolutions of the 16-bit mode on a halo-staged kernel (csrc/h16_halo.hip; ResnetBlock
 * conv1 / conv2, Upsample.conv, conv_out: diffusionmodules/model.py:43-53, 88-102, 117-137): input patch staged once per
 * 32-channel slab, weights in MFMA-fragment order straight to registers, optional GroupNorm(+swish) of the INPUT applied
 * while staging (gn_mean_rstd [B][32][2] or NULL, gn_gamma / gn_beta [Cin]), the product computed transposed so that a lane
 * stores 16 consecutive channels of one pixel, optional statistics of the OUTPUT as per-chunk partial sums (gn_partial
 * [B][sgam_conv2d_h16_stats_chunks(d)][32][2] doubles or NULL).  Available when sgam_conv2d_h16_uses_halo(d) == 1 (3x3 s1 p1
 * on the input or its nearest-2x upsampling, Ho % 8 == 0, Wo % 8 == 0, Cin % 32 == 0, N % 128 == 0).  Maps too small to fill
 * the chip split the K slabs over grid.y (plan_ksplit, or chosen by the library): fp32 partial tiles go to `workspace`
 * (sgam_conv2d_halo_h16_workspace_bytes(d) bytes, 0 without split-K) and a combine launch adds them in a fixed order, applies
 * bias / residual, rounds and leaves the statistics.  w_frag from sgam_pack_conv_weight_h16_frag:
 * [Cout_pad / 32][KH*KW*Cin_pad / 32][128 pieces][8 halfs], piece = (k-step * 2 + k-half) * 32 + row', where row' = 8 (e / 4)
 * + 4 half + e % 4 for channel 16 half + e of the 32-channel tile (the accumulator slot order of the transposed product). */
int32_t sgam_conv2d_h16_uses_halo(const sgam_conv_desc *d);
int32_t sgam_conv2d_h16_stats_chunks(const sgam_conv_desc *d);
int64_t sgam_conv2d_halo_h16_workspace_bytes(const sgam_conv_desc *d);
int sgam_pack_conv_weight_h16_frag(const float *w_oihw, void *w_frag, int32_t ht, int32_t Cout, int32_t Cin, int32_t KH, int32_t KW,
                                   int32_t Cout_pad, int32_t Cin_pad, void *stream);
int sgam_conv2d_halo_nhwc_h16(const sgam_conv_desc *d, int32_t ht, const void *x, const float *gn_mean_rstd,
                              const float *gn_gamma, const float *gn_beta, int32_t gn_swish, const void *w_frag,
                              const float *bias, const void *residual, void *out, int32_t out_f32, double *gn_partial,
                              void *workspace, int64_t workspace_bytes, void *stream);
/* (ABI v5) The same launch with the statistics of the INPUT still as its producer's chunk partials (gn_partial_in
 * [B][chunks_in][32][2] doubles — what sgam_conv2d_halo_nhwc_h16 leaves in `gn_partial` — instead of folded {mean, rstd}): the
 * kernel folds them itself while it stages (no fold launch between two convolutions of a ResnetBlock).  Offered where
 * sgam_conv2d_h16_gn_foldable(d, chunks_in) == 1: the 64-row tile walking <= 2 channel slabs per workgroup (the split-K plans
 * of the 16 x 16 / 32 x 32 maps), Cin % 256 == 0, chunks_in <= 16 — which is what the group-major split-K combine of those
 * maps produces (sgam_conv2d_h16_stats_chunks). */
int32_t sgam_conv2d_h16_gn_foldable(const sgam_conv_desc *d, int32_t chunks_in);
int sgam_conv2d_halo_gnp_nhwc_h16(const sgam_conv_desc *d, int32_t ht, const void *x, const double *gn_partial_in,
                                  int32_t chunks_in, float gn_eps, const float *gn_gamma, const float *gn_beta, int32_t gn_swish,
                                  const void *w_frag, const float *bias, const void *residual, void *out, int32_t out_f32,
                                  double *gn_partial, void *workspace, int64_t workspace_bytes, void *stream);
/* GroupNorm of 16-bit tensors from the partial statistics the halo kernel left / {mean, rstd} of any 16-bit tensor */
int sgam_groupnorm_from_partials_h16(const void *x, const double *partial, int32_t nchunk, const float *gamma, const float *beta,
                                     void *y, int32_t ht, int32_t B, int32_t HW, int32_t C, int32_t groups, float eps,
                                     int32_t fuse_swish, void *workspace, int64_t workspace_bytes, void *stream);
int sgam_groupnorm_meanrstd_nhwc_h16(const void *x, float *mean_rstd, int32_t ht, int32_t B, int32_t HW, int32_t C, int32_t groups,
                                     float eps, void *workspace, int64_t workspace_bytes, void *stream);
int sgam_pack_conv_weight_h16(const float *w_oihw, void *w_packed, int32_t ht, int32_t Cout, int32_t Cin,
                              int32_t KH, int32_t KW, int32_t Cout_pad, int32_t Cin_pad, void *stream);
int sgam_cast_f32_h16(const float *x, void *y, int32_t ht, int64_t n, void *stream);
int sgam_cast_h16_f32(const void *x, float *y, int32_t ht, int64_t n, void *stream);
int64_t sgam_groupnorm_h16_workspace_bytes(int32_t B, int32_t HW, int32_t C);
int sgam_groupnorm_nhwc_h16(const void *x, const float *gamma, const float *beta, void *y, int32_t ht, int32_t B,
                            int32_t HW, int32_t C, int32_t groups, float eps, int32_t fuse_swish, void *workspace,
                            int64_t workspace_bytes, void *stream);
/* p_out[r][:] (16-bit) = softmax(scale * s_in[r][:]) (fp32 scores) */
int sgam_softmax_rows_h16(const float *s_in, void *p_out, int32_t ht, int32_t rows, int32_t cols, int32_t lds,
                          int32_t ldp, float scale, void *stream);
/* (ABI v5) block-diagonal form: row r keeps the columns of its own block [r / block * block, + block), the others become
 * exact zeros — the attention of B images whose tokens do not fill the fused kernel (16 x 16 maps, C = 512) as ONE
 * (B n) x (B n) score matrix instead of B small GEMM / softmax / GEMM chains. */
int sgam_softmax_rows_blockdiag_h16(const float *s_in, void *p_out, int32_t ht, int32_t rows, int32_t cols, int32_t lds,
                                    int32_t ldp, float scale, int32_t block, void *stream);
int sgam_encode_head_h16(const float *x, const uint8_t *mask, const float *w, const float *bias, void *y,
                         int32_t ht, int32_t B, int32_t HW, int32_t ldy, void *stream);
/* y[c][p] = x[p][c] for a [HW][ldx] 16-bit matrix (v -> v^T for the P.V product) */
int sgam_transpose_h16(const void *x, void *y, int32_t ht, int32_t C, int32_t HW, int32_t ldx, void *stream);

/* ------------------------------------------------------------------------------------------
 * K4 — GroupNorm(32 groups, eps, affine) with optional fused swish, NHWC.
 * Replaces Normalize + nonlinearity: diffusionmodules/model.py:29-35, used at :119-127, :170,
 * :429-430, :536-537.  Biased variance, fp32 data, fp64 cross-thread accumulation.
 *   x,y [B][HW][C]; gamma,beta [C]; C % 128 == 0 (4 channels per lane, groups never straddle a lane)
 *   workspace: sgam_groupnorm_workspace_bytes(B, HW, C).
 * ------------------------------------------------------------------------------------------ */
int64_t sgam_groupnorm_workspace_bytes(int32_t B, int32_t HW, int32_t C);
int sgam_groupnorm_nhwc_f32(const float *x, const float *gamma, const float *beta, float *y, int32_t B,
                            int32_t HW, int32_t C, int32_t groups, float eps, int32_t fuse_swish,
                            void *workspace, int64_t workspace_bytes, void *stream);

/* Statistics half of K4 for the FUSED path: writes the per-(batch, channel) table
 *   scale_shift[b][c] = { rstd[b,g(c)] * gamma[c],  beta[c] - mean[b,g(c)] * rstd[b,g(c)] * gamma[c] }   ([B][C][2] floats)
 * which sgam_conv2d_gn_nhwc_f32 applies (with optional swish) to its A operand while staging it — the
 * normalised activation is never written to HBM.  Same constraints / workspace as sgam_groupnorm_nhwc_f32. */
int sgam_groupnorm_stats_nhwc_f32(const float *x, const float *gamma, const float *beta, float *scale_shift,
                                  int32_t B, int32_t HW, int32_t C, int32_t groups, float eps, void *workspace,
                                  int64_t workspace_bytes, void *stream);

/* ------------------------------------------------------------------------------------------
 * K5 — row softmax of the attention scores, in place: s[r][:] = softmax(scale * s[r][:]).
 * Replaces `w_ * c**-0.5` + softmax(dim=2): diffusionmodules/model.py:181-182.
 * ------------------------------------------------------------------------------------------ */
int sgam_softmax_rows_f32(float *s, int32_t rows, int32_t cols, int32_t ld, float scale, void *stream);
int sgam_softmax_rows_blockdiag_f32(float *s, int32_t rows, int32_t cols, int32_t ld, float scale, int32_t block,
                                    void *stream);   /* (ABI v5) see sgam_softmax_rows_blockdiag_h16 */

/* ------------------------------------------------------------------------------------------
 * K4-K6 fused — single-head self-attention of the AttnBlock in one pass over the keys (attention.hip):
 *   out[i][:] = sum_j softmax_j(scale * q_i . k_j) v_j,   q, k, v : [n][C] fp32 with row stride ld (the column
 *   slices of the fused q|k|v projection), out : [n][C] with row stride ldo.
 * Replaces torch.bmm(q, k) / `w_ * c**-0.5` / softmax(dim=2) / torch.bmm(v, w_) of AttnBlock.forward
 * (modules/diffusionmodules/model.py:176-187) without materialising the n x n scores.  Split-fp32 arithmetic as
 * sgam_conv2d_nhwc_f32x (three fp16 MFMAs per product, fp32 accumulation), fp32 online soft-max.
 * Supported: C == 256, n % 256 == 0, scale an exact power of two (C^-1/2 = 1/16); anything else -> SGAM_EINVAL and
 * the caller keeps the GEMM / softmax / GEMM chain.  workspace: sgam_attention_f32x_workspace_bytes(n, C) bytes,
 * 16-byte aligned (-1 = unsupported shape).
 * ------------------------------------------------------------------------------------------ */
int64_t sgam_attention_f32x_workspace_bytes(int32_t n, int32_t C);
int sgam_attention_f32x(const float *q, const float *k, const float *v, int32_t ld, int32_t n, int32_t C, float scale,
                        float *out, int32_t ldo, void *workspace, int64_t workspace_bytes, void *stream);

/* 16-bit throughput variant of the fused attention (`ht` = 0 bf16 / 1 fp16; q, k, v, out 16-bit with strides in elements;
 * one MFMA per product, fp32 scores / statistics / accumulation; same shape limits; scale need not be a power of two) */
int64_t sgam_attention_h16_workspace_bytes(int32_t n, int32_t C);
int sgam_attention_h16(const void *q, const void *k, const void *v, int32_t ht, int32_t ld, int32_t n, int32_t C, float scale,
                       void *out, int32_t ldo, void *workspace, int64_t workspace_bytes, void *stream);

/* Batched forms (ABI v4): B images of n tokens each, stacked along the rows — q, k, v, out are [B * n][...] and every query
 * attends to the keys of ITS image only (the AttnBlock at batch B, e.g. B lock-stepped scenes or B warp candidates: one
 * launch sequence instead of B).  The number of key ranges per image is chosen from (n, B) so that the launch fills the chip
 * with as few partial outputs as possible, at most 2048 keys per range (8 ranges for one 64 x 64 image, 2 from four images on); B = 1 is exactly the
 * unbatched entry point.  workspace: the matching *_batched_workspace_bytes(n, C, B). */
int64_t sgam_attention_f32x_batched_workspace_bytes(int32_t n, int32_t C, int32_t B);
int sgam_attention_f32x_batched(const float *q, const float *k, const float *v, int32_t ld, int32_t n, int32_t C, int32_t B,
                                float scale, float *out, int32_t ldo, void *workspace, int64_t workspace_bytes, void *stream);
/* (ABI v8) sgam_attention_f32x_batched followed by AttnBlock.proj_out (+ residual) — reference modules/diffusionmodules/model.py:176-191,
 * `h_ = bmm(v, w_); h_ = self.proj_out(h_); return x + h_` — with the merge of the key ranges fused into the projection: no [B n][C]
 * attention output is written and read back, one launch fewer.  w_planes / w_scale: proj_out's [C][C] weight as sgam_split_rows_f32x
 * returns it; bias [C] or NULL; residual [B n][ldr] or NULL; out [B n][ldc]; gn_partial (optional): [B][n / 32][32][2] fp64 {sum, sumsq}
 * of `out` per (32-row tile, group of C / 32 channels) for the GroupNorm that follows (fold with sgam_groupnorm_stats_from_partials_f32,
 * nchunk = n / 32).  Same shape limits and workspace as sgam_attention_f32x_batched. */
int sgam_attention_proj_f32x_batched(const float *q, const float *k, const float *v, int32_t ld, int32_t n, int32_t C, int32_t B,
                                     float scale, const void *w_planes, float w_scale, const float *bias, const float *residual,
                                     int32_t ldr, float *out, int32_t ldc, double *gn_partial, void *workspace,
                                     int64_t workspace_bytes, void *stream);
int64_t sgam_attention_h16_batched_workspace_bytes(int32_t n, int32_t C, int32_t B);
int sgam_attention_h16_batched(const void *q, const void *k, const void *v, int32_t ht, int32_t ld, int32_t n, int32_t C,
                               int32_t B, float scale, void *out, int32_t ldo, void *workspace, int64_t workspace_bytes,
                               void *stream);

/* (ABI v9) The AttnBlock of the 16-bit mode ahead of proj_out in ONE call of four launches — reference
 * modules/diffusionmodules/model.py:168-187: `h_ = self.norm(x); q = self.q(h_); k = self.k(h_); v = self.v(h_)`, then the attention
 * of sgam_attention_h16_batched.  GroupNorm is applied while the projection stages its operand (y = x scale + shift from the
 * per-channel table, fp32, one rounding to 16 bits — the arithmetic of sgam_groupnorm_from_partials_h16), the stacked q | k | v
 * projection writes q row-major and K / V^T directly in the fused attention's MFMA-fragment order: the stand-alone normalise pass, the
 * generic 1 x 1 GEMM and the fragment-split launch disappear.
 *   x          [B n][ldx] 16-bit block input (ldx % 8 == 0), C == 256, n % 256 == 0 (sgam_attention_h16_batched's shapes)
 *   gn_partial the chunk statistics x's producer left: [B][nchunk][32][2] fp64 {sum, sumsq}; gamma, beta [C] of AttnBlock.norm; eps
 *   w_frag     sgam_pack_qkv_weight_h16 of the stacked [3 C][C] fp32 weight (rows: q.weight, k.weight, v.weight): 3 C C 2 bytes
 *   bias       [3 C] fp32 (q.bias | k.bias | v.bias), 16-byte aligned
 *   out        [B n][ldo] 16-bit attention output (the operand of proj_out)
 *   workspace  sgam_attn_block_h16_workspace_bytes(n, C, B)
 * sgam_groupnorm_table_from_partials is the finalize half of sgam_groupnorm_from_partials_* on its own: the {scale, shift} table
 * [B][C][2] fp32 (scale = rstd gamma, shift = beta - mean scale) for a consumer that normalises while staging. */
/* (ABI v9) The whole AttnBlock of the split-fp32 path in three launches — reference modules/diffusionmodules/model.py:168-192,
 * `h_ = self.norm(x); q, k, v = self.q(h_), self.k(h_), self.v(h_); ...; return x + self.proj_out(h_)`: the fused front end (GroupNorm in
 * the operand staging of the stacked q | k | v projection, q row-major, K / V^T written straight in the attention's hi / lo fragment order —
 * the arithmetic of sgam_gemm_gn_f32x + the split launch it replaces, equal to fp32 round-off), the one-pass attention, and sgam_attention_proj_f32x_batched's merge +
 * proj_out + residual (= x).  mean_rstd [B][32][2] (sgam_groupnorm_stats_from_partials_f32); wqkv_planes / wqkv_scale: sgam_split_rows_f32x of
 * the stacked [3 C][C] weight with the rows of every 32-row tile permuted so that row 8 j + 4 h + i holds channel 16 h + 4 j + i; bqkv [3 C] in
 * natural order; wp_planes / wp_scale / bp: proj_out as for sgam_attention_proj_f32x_batched; gn_partial as there.  C == 256,
 * n % 256 == 0, scale a power of two; workspace: sgam_attn_block_f32x_workspace_bytes(n, C, B). */
int64_t sgam_attn_block_f32x_workspace_bytes(int32_t n, int32_t C, int32_t B);
int sgam_attn_block_f32x(const float *x, int32_t ldx, const float *mean_rstd, const float *gamma, const float *beta, const void *wqkv_planes,
                         float wqkv_scale, const float *bqkv, int32_t n, int32_t C, int32_t B, float scale, const void *wp_planes,
                         float wp_scale, const float *bp, float *out, int32_t ldc, double *gn_partial, void *workspace,
                         int64_t workspace_bytes, void *stream);
/* (ABI v9) The attention of the SMALL AttnBlocks in one launch — the 16 x 16 mid blocks (n = 256 tokens per image, C = 512; n = 128 too):
 * model.py:176-187, `w_ = bmm(q, k) * c**-0.5; w_ = softmax(w_, dim=2); h_ = bmm(v, w_)` — what otherwise runs as v^T transpose, operand
 * splits, the q k^T GEMM (+ split-K combine), sgam_softmax_rows_f32 and the P v GEMM: seven launches.  A workgroup holds a query tile's whole
 * score row (every query attends to the n keys of ITS image; B images stacked along the rows); the soft-max is sgam_softmax_rows_f32's
 * arithmetic; equal to the chain to fp32 round-off.  q, k, v: [B n][ld] fp32 (ld % 4 == 0), out [B n][ldo]; no workspace. */
int32_t sgam_attention_small_f32x_fits(int32_t n, int32_t C, int32_t B);
int sgam_attention_small_f32x(const float *q, const float *k, const float *v, int32_t ld, int32_t n, int32_t C, int32_t B, float scale,
                              float *out, int32_t ldo, void *stream);
/* 16-bit twin (`ht` = 0 bf16 / 1 fp16; q, k, v, out 16-bit, ld % 8 == 0): replaces sgam_transpose_h16 + the q k^T GEMM + sgam_softmax_rows_h16
 * + the P v GEMM; fp32 scores and soft-max (sgam_softmax_rows_h16's arithmetic), probabilities rounded once, fp32 accumulation. */
int sgam_attention_small_h16(const void *q, const void *k, const void *v, int32_t ht, int32_t ld, int32_t n, int32_t C, int32_t B, float scale,
                             void *out, int32_t ldo, void *stream);
int sgam_groupnorm_table_from_partials(const double *partial, int32_t nchunk, const float *gamma, const float *beta,
                                       float *scale_shift, int32_t B, int32_t HW, int32_t C, int32_t groups, float eps, void *stream);
int sgam_pack_qkv_weight_h16(const float *w, void *w_frag, int32_t ht, int32_t C, void *stream);
/* sgam_pack_weight_tp_h16: any [rows][C] 1 x 1 weight in that fragment order (rows % 32 == 0); sgam_attn_block_proj_h16: the WHOLE block —
 * sgam_attn_block_h16 with the merge of the key ranges fused into proj_out + residual (= x), model.py:187-191: out = x + proj_out(h_),
 * [B n][ldo] 16-bit, ldo % 8 == 0; wp_frag = sgam_pack_weight_tp_h16(proj_out.weight, rows = C); bp [C] or NULL; gn_partial_out (optional)
 * [B][n / 32][32][2] fp64 chunk statistics of the STORED output for the GroupNorm that follows. */
int sgam_pack_weight_tp_h16(const float *w, void *w_frag, int32_t ht, int32_t rows, int32_t C, void *stream);
int sgam_attn_block_proj_h16(const void *x, int32_t ldx, const double *gn_partial, int32_t nchunk, const float *gamma, const float *beta,
                             float eps, const void *w_frag, const float *bias, int32_t ht, int32_t n, int32_t C, int32_t B, float scale,
                             const void *wp_frag, const float *bp, double *gn_partial_out, void *out, int32_t ldo, void *workspace,
                             int64_t workspace_bytes, void *stream);
int64_t sgam_attn_block_h16_workspace_bytes(int32_t n, int32_t C, int32_t B);
int sgam_attn_block_h16(const void *x, int32_t ldx, const double *gn_partial, int32_t nchunk, const float *gamma, const float *beta,
                        float eps, const void *w_frag, const float *bias, int32_t ht, int32_t n, int32_t C, int32_t B, float scale,
                        void *out, int32_t ldo, void *workspace, int64_t workspace_bytes, void *stream);

/* ------------------------------------------------------------------------------------------
 * K7/K8 — nearest-codeword quantiser.  Replaces VectorQuantizer2.forward
 * (modules/vqvae/quantize.py:285-307): d = (|z|^2 + |e|^2) - 2 z.e (that expression order, fp32),
 * arg-min with first-index-of-ties, embedding gather, straight-through value z + (e - z).
 *   z        [T][D] tokens (NHWC latent), D % 32 == 0
 *   codebook [n_e][D], n_e % 64 == 0;  e_sq [n_e] = sgam_row_sumsq(codebook)
 *   dots     [T][n_e] scratch (z . e^T), caller-allocated
 *   idx_out  [T] int64;  zq_out [T][D] (may be NULL);  dist_out [T][n_e] optional (NULL to skip)
 *   workspace: sgam_vq_workspace_bytes(T, D, n_e) bytes (split-K partials for small T), may be 0
 * ------------------------------------------------------------------------------------------ */
int sgam_row_sumsq_f32(const float *x, float *out, int32_t rows, int32_t cols, void *stream);
int64_t sgam_vq_workspace_bytes(int32_t T, int32_t D, int32_t n_e);
int sgam_vq_nearest_f32(const float *z, const float *codebook, const float *e_sq, float *dots,
                        int64_t *idx_out, float *zq_out, float *dist_out, int32_t T, int32_t D,
                        int32_t n_e, int32_t straight_through, void *workspace, int64_t workspace_bytes,
                        void *stream);
/* commitment loss of VectorQuantizer2.forward (quantize.py:296-301, legacy = True):
 *   loss = mean((e[idx] - z)^2) + beta * mean((e[idx] - z)^2)   — the scalar VQModel.forward returns as `diff`
 * (model.py:144-147).  partial [T] doubles (scratch: per-token sums, folded in a fixed order); loss [1] float. */
int sgam_vq_commit_loss_f32(const float *z, const float *codebook, const int64_t *idx, double *partial, float *loss,
                            int32_t T, int32_t D, int32_t n_e, float beta, void *stream);
/* pure gather (quantize.py:368, get_codebook_entry :321-335): out[t][:] = codebook[idx[t]][:] */
int sgam_vq_gather_f32(const float *codebook, const int64_t *idx, float *out, int32_t T, int32_t D,
                       int32_t n_e, void *stream);
/* k smallest distances per token (ascending, ties -> lower index first), for the top-k infill
 * sampler (quantize.py:352-354).  vals [T][k], inds [T][k] int64; k <= 64. */
int sgam_vq_topk_f32(const float *dist, float *vals, int64_t *inds, int32_t T, int32_t n_e, int32_t k,
                     void *stream);
/* Device-side top-k infill sampler: the whole of get_multiple_codewords (quantize.py:344-381) after the distance
 * matrix, with a counter-based generator — no host round trip, nothing written but the outputs, so a sampling forward can be
 * captured once and replayed.  Two launches: the kernel of sgam_vq_topk_f32, then one wavefront per (b, s, t).
 * For batch item b, token t (T = h*w), sample s (S samples):
 *   1. candidates: the k smallest distances of token t exactly as sgam_vq_topk_f32 orders them (ascending, ties by lower
 *      index); written to vals / inds [B*T][k] (outputs).
 *   2. distribution row r = 0 (token 0 of item b: the reference's quirk at quantize.py:358) when per_token == 0, r = t otherwise.
 *   3. weights, fp32, in this order: e_j = expf(-(v[r][j] - v[r][0]) / temperature), c_j = c_{j-1} + e_j (round to nearest,
 *      sequential), total = c_{k-1}.
 *   4. uniform: Philox4x32-10 (multipliers 0xD2511F53, 0xCD9E8D57; Weyl 0x9E3779B9, 0xBB67AE85), key = (seed lo32, seed hi32),
 *      counter = (t*S + s, stream_id[b], call lo32, call hi32), u = (word0 >> 8) * 2^-24.
 *   5. slot = the first j with u * total < c_j (the last slot if none); slot 0 wherever the extrapolation mask, nearest-resized
 *      to (h, w) like F.interpolate(mode='nearest') (src = floor(dst * mask_h / h)), is 0.  mask [B][mask_h][mask_w] bool
 *      bytes; NULL = every token is inside the hole.
 *   6. idx_out [B][S][h][w] int64 = inds[b*T + t][slot];  zq_out [B][S][h][w][D] = that codebook row (pure gather, :381).
 * stream_id [B] int32 and call [1] (64-bit) are DEVICE arrays read at run time: a captured graph draws new values at each
 * replay once the caller has updated them.  k <= 32, D % 4 == 0, temperature > 0. */
int sgam_vq_sample_topk_f32(const float *dist, const float *codebook, const uint8_t *mask, const int32_t *stream_id,
                            const uint64_t *call, uint64_t seed, float *vals, int64_t *inds, int64_t *idx_out,
                            float *zq_out, int32_t B, int32_t S, int32_t h, int32_t w, int32_t D, int32_t n_e,
                            int32_t k, int32_t mask_h, int32_t mask_w, int32_t per_token, float temperature,
                            void *stream);

/* ------------------------------------------------------------------------------------------
 * Layout hops at the nn.Module boundary.
 * ------------------------------------------------------------------------------------------ */
int sgam_nchw_to_nhwc_f32(const float *x, float *y, int32_t B, int32_t C, int32_t HW, int32_t ldy,
                          void *stream); /* y[b][p][c] (row stride ldy >= C; columns >= C untouched) */
int sgam_nhwc_to_nchw_f32(const float *x, float *y, int32_t B, int32_t C, int32_t HW, int32_t ldx,
                          void *stream);
/* VQModel.encode head (model.py:107-113): cat(x, mask) -> 1x1 conv 5->4 -> NHWC with the pixel
 * stride padded to `ldy` floats (channels 4..ldy-1 zeroed) so the 3x3 conv_in runs on the MFMA path.
 *   x [B][4][HW] NCHW fp32, mask [B][HW] uint8 (0/1) or NULL (all zero), w [4][5], bias [4]. */
int sgam_encode_head_f32(const float *x, const uint8_t *mask, const float *w, const float *bias,
                         float *y, int32_t B, int32_t HW, int32_t ldy, void *stream);

/* ------------------------------------------------------------------------------------------
 * K9/K10/K12 — forward splat + 3x3 median hole fill + extrapolation mask (+ inverse-depth
 * normalisation).  Replaces render_projection_from_srcs_fast (sgam/point_rendering/warp.py:193-286,
 * pixel2cam :28-40, median_blur :306-347) and the depth normalisation of VQModel.get_x
 * (sgam/generative_sensing_module/model.py:210-229).
 *
 * Deterministic "largest linear point index wins" scatter (point p = pixel*N + src), the
 * semantics of the reference's sequential parallel=False loop (warp.py:246-249).
 *   src_feats   (B,N) images of 3 channels: element (b,n,c,pix) at
 *               src_feats[((b*N+n)*HW)*3... ] via strides: feat_cs (channel stride), feat_ps (pixel stride)
 *               - (B,N,3,H,W) tensors: feat_cs = HW, feat_ps = 1;  (B,N,H,W,3): feat_cs = 1, feat_ps = 3
 *   src_depths  [B][N][HW];  tgt_K [B][9];  src_Kinv [B*N][9] (inverse source intrinsics);
 *   T [B*N][16] source->target rigid transforms (row-major 4x4)
 *   winner      [B][HW] int32 scratch
 *   depth_range NULL at inference (mask = merge_depth <= 0, warp.py:285) or 2 floats (host pointer)
 *   dataset_norm 0: none, 1: google_earth, 2: clevr-infinite (model.py:210-229)
 * Outputs (any may be NULL): merge_depths [B][HW], merge_feats [B][3][HW], extrap [B][HW] uint8,
 *   x_out [B][4][HW] = cat(merge_feats, normalised inverse depth with holes = -2),
 *   proj_feats [B][3][HW], proj_depth [B][HW] (pre-fill planes), inb_mask [B][HW][N] uint8,
 *   pix_xy [B][HW][N][2] int32 (target pixel of every point, valid where inb_mask).
 * ------------------------------------------------------------------------------------------ */
int sgam_forward_splat_f32(const float *src_feats, int64_t feat_cs, int64_t feat_ps,
                           const float *src_depths, const float *tgt_K, const float *src_Kinv,
                           const float *T, int32_t B, int32_t N, int32_t H, int32_t W,
                           const float *depth_range, int32_t dataset_norm, int32_t *winner,
                           float *merge_depths, float *merge_feats, uint8_t *extrap, float *x_out,
                           float *proj_feats, float *proj_depth, uint8_t *inb_mask, int32_t *pix_xy,
                           void *stream);
/* Same splat with the sources addressed through a table of device pointers instead of one stacked tensor: the scene
 * loop (prepare_batch_data, inference_pipeline.py:534-537) keeps every generated frame as its own HBM allocation and
 * the warp reads them in place.  src_feat_ptrs / src_depth_ptrs: HOST arrays of B*N device pointers (entry b*N+n: the
 * [HW] x 3 features of that source, strides feat_cs / feat_ps, and its [HW] depth map); B*N <= 64 (the table travels by
 * value in the kernel arguments: no upload).  Everything else as sgam_forward_splat_f32. */
int sgam_forward_splat_srcs_f32(const float *const *src_feat_ptrs, const float *const *src_depth_ptrs, int64_t feat_cs,
                                int64_t feat_ps, const float *tgt_K, const float *src_Kinv, const float *T, int32_t B,
                                int32_t N, int32_t H, int32_t W, const float *depth_range, int32_t dataset_norm,
                                int32_t *winner, float *merge_depths, float *merge_feats, uint8_t *extrap, float *x_out,
                                float *proj_feats, float *proj_depth, uint8_t *inb_mask, int32_t *pix_xy, void *stream);

/* (ABI v6) The same forward splat WITHOUT global atomics — target-owned tiles with an LDS z-tile (csrc/warp.hip):
 * pass 1 caches every source point's target pixel and registers each 8 x 32 source bin with the target tiles its bounding
 * box meets, pass 2 gives a workgroup a 32 x 32 (16 x 16 for small launches) tile of the target image + 1-pixel halo, resolves
 * "largest point index wins" (warp.py:217-262) with LDS atomicMax over the registered bins, and finishes median fill / merge / mask /
 * depth normalisation (warp.py:264-286, model.py:210-229) from LDS.  Results are bit-identical to sgam_forward_splat_f32
 * for any geometry; the by-products inb_mask / pix_xy are only offered by the two-pass form above.
 *   workspace: sgam_forward_splat_workspace_bytes(B, N, H, W) bytes, 16-byte aligned: the per-tile bitmaps of registered
 *   source bins, then the cached target pixels [B][N][HW] int32.  Its first sgam_forward_splat_workspace_zero_bytes(B, N, H, W)
 *   bytes (the bitmaps) must be ZERO when the workspace is first used; every call leaves them zero again (no memset per
 *   call).  H, W <= 32767, N <= 64.  -1 from the queries: shape refused. */
int64_t sgam_forward_splat_workspace_bytes(int32_t B, int32_t N, int32_t H, int32_t W);
int64_t sgam_forward_splat_workspace_zero_bytes(int32_t B, int32_t N, int32_t H, int32_t W);
int sgam_forward_splat_tiled_f32(const float *src_feats, int64_t feat_cs, int64_t feat_ps, const float *src_depths,
                                 const float *tgt_K, const float *src_Kinv, const float *T, int32_t B, int32_t N, int32_t H,
                                 int32_t W, const float *depth_range, int32_t dataset_norm, void *workspace,
                                 int64_t workspace_bytes, float *merge_depths, float *merge_feats, uint8_t *extrap,
                                 float *x_out, float *proj_feats, float *proj_depth, void *stream);
int sgam_forward_splat_tiled_srcs_f32(const float *const *src_feat_ptrs, const float *const *src_depth_ptrs, int64_t feat_cs,
                                      int64_t feat_ps, const float *tgt_K, const float *src_Kinv, const float *T, int32_t B,
                                      int32_t N, int32_t H, int32_t W, const float *depth_range, int32_t dataset_norm,
                                      void *workspace, int64_t workspace_bytes, float *merge_depths, float *merge_feats,
                                      uint8_t *extrap, float *x_out, float *proj_feats, float *proj_depth, void *stream);

/* K12 standalone (VQModel.get_x, model.py:196-199 + 210-229, when the warped view is supplied by the
 * caller): compute_mask=1: extrap = depth <= 0, out = normalised inverse depth with holes = -2;
 * compute_mask=0: out = 2*norm(depth)-1 only (the ground-truth branch x_scaled_inverse_depth). */
int sgam_depth_normalise_f32(const float *depth, int32_t compute_mask, uint8_t *extrap, float *out,
                             int32_t dataset_norm, int64_t n, void *stream);

/* ------------------------------------------------------------------------------------------
 * K11 — target-depth-driven inverse warp with best-source selection.  Replaces
 * InfiniteSceneGeneration.inverse_warping (sgam/inference_pipeline.py:662-743).
 *   src_imgs [B][N][3][HW], src_depths [B][N][HW], tgt_depth [B][HW], src_K [B*N][9],
 *   tgt_Kinv [B][9], T_tgt2src [B*N][16];  warped [B][3][HW];  zbuf [B][HW] optional.
 * ------------------------------------------------------------------------------------------ */
int sgam_inverse_warp_f32(const float *src_imgs, const float *src_depths, const float *tgt_depth,
                          const float *src_K, const float *tgt_Kinv, const float *T_tgt2src, int32_t B,
                          int32_t N, int32_t H, int32_t W, float *warped, float *zbuf, void *stream);
/* Same with a pointer table (HOST arrays of B*N <= 64 device pointers) and free channel / pixel strides of the source
 * images: (3,H,W) planes: img_cs = HW, img_ps = 1; the frame store's (H,W,3): img_cs = 1, img_ps = 3. */
int sgam_inverse_warp_srcs_f32(const float *const *src_img_ptrs, const float *const *src_depth_ptrs, int64_t img_cs,
                               int64_t img_ps, const float *tgt_depth, const float *src_K, const float *tgt_Kinv,
                               const float *T_tgt2src, int32_t B, int32_t N, int32_t H, int32_t W, float *warped,
                               float *zbuf, void *stream);

/* ------------------------------------------------------------------------------------------
 * Frame feedback codec (inference_pipeline.py:898-911 then :534-537): decoder output (B,4,HW)
 * in [-1,1] -> RGB quantised to uint8 by truncation and re-expanded with the host-built 256-entry
 * table lut[u] = float32(u / 127.5 - 1.0), metric depth from the normalised inverse depth.
 *   rgb_u8 [B][HW][3] (HWC, optional), rgb_f [B][HW][3] (HWC fp32, what prepare_batch_data reloads),
 *   depth [B][HW].
 * ------------------------------------------------------------------------------------------ */
int sgam_frame_feedback_f32(const float *dec, const float *lut256, int32_t dataset_norm, uint8_t *rgb_u8,
                            float *rgb_f, float *depth, int32_t B, int32_t HW, void *stream);
/* the re-read half alone, for frames that arrive as uint8 (the seed frame): rgb_f[i] = lut256[rgb_u8[i]], n values */
int sgam_rgb_u8_to_f32(const uint8_t *rgb_u8, const float *lut256, float *rgb_f, int64_t n, void *stream);

/* Fused q | k | v projection of AttnBlock on the split-fp32 path (diffusionmodules/model.py:168-175: norm -> three 1x1
 * convolutions): out[M][N] = GroupNorm(x)[M][K] . W[N][K]^T + bias with the normalisation applied while the 64 x 256 operand
 * panel is staged (mean_rstd [B][32][2] from sgam_groupnorm_stats_*; no swish), w_planes / w_scale = a SplitWeight of the
 * stacked weights (sgam_split_rows_f32x).  sgam_gemm_gn_f32x_fits: M % 64 == 0 inside whole images of HW rows, N % 128 == 0,
 * K % 256 == 0 (K = 128 without normalisation). */
int32_t sgam_gemm_gn_f32x_fits(int32_t M, int32_t N, int32_t K, int32_t HW);
/* the same kernel for the other 1x1 convolutions / GEMMs that fit (proj_out, nin_shortcut, quant_conv): mean_rstd / gamma /
 * beta NULL = no normalisation (then K = 128 is accepted too); optional residual [M][ldr]; optional gn_partial
 * [B][HW / 64][32][2] fp64 = per-chunk statistics of `out` for the next GroupNorm (N / 32 a power of two <= 32) */
int sgam_gemm_panel_f32x(const float *x, int32_t lda, const float *mean_rstd, const float *gamma, const float *beta,
                         const void *w_planes, float w_scale, const float *bias, const float *residual, int32_t ldr, float *out,
                         int32_t ldc, double *gn_partial, int32_t M, int32_t N, int32_t K, int32_t HW, void *stream);
int sgam_gemm_gn_f32x(const float *x, int32_t lda, const float *mean_rstd, const float *gamma, const float *beta, const void *w_planes,
                      float w_scale, const float *bias, float *out, int32_t ldc, int32_t M, int32_t N, int32_t K, int32_t HW,
                      void *stream);

/* ------------------------------------------------------------------------------------------
 * f1 — TSDF fusion of the generated RGB-D frames + depth render at the target pose.  Replaces
 * InfiniteSceneGeneration.rgbd_integration (sgam/inference_pipeline.py:119-133, 745-838: Open3D 0.15.2
 * ScalableTSDFVolume.integrate / extract_triangle_mesh / OffscreenRenderer.render_to_depth_image).
 * Integration is Open3D's published rule (16^3-voxel units, stride-4 unit opening, running weighted mean of
 * min(1, sdf / sdf_trunc)); the depth render is a direct ray cast of the fused surface (first +/- zero crossing of the
 * trilinear TSDF, view-space z, 0 = nothing hit).  Colour (TSDFVolumeColorType::RGB8, :123-131, 777-790) is fused
 * with the same running mean — color <- (color * w + rgb(u, v)) / (w + 1) per channel, 0..255 — when rgb_u8 [H][W][3] and
 * brick_color [max_bricks][16*16*16][3] fp32 (0-initialised) are given (both or neither), and the ray cast can return the
 * colour of the nearest voxel at the hit (color_out [H][W][3] fp32, 0 = nothing hit); the conditioning path itself only
 * consumes the depth.
 *   unit_table [dims.z][dims.y][dims.x] int32, -1 = closed, else brick index | 0x40000000 once the brick holds part of
 *   the truncation band (the ray cast only marches those); unit_stamp same shape, 0-initialised;
 *   counters int32[4 * 32], zero-initialised: counter k at index 32 k (one 128-byte line each: same-line atomics are serialised)
 *   = {bricks allocated, length of this step's brick list, samples outside the box, pool overflows};
 *   brick_tsdf [max_bricks][16*16*16] fp32 initialised to 2.0 (= unobserved: observed values are <= 1, so the ray cast
 *   needs no weight loads), brick_weight same shape, 0-initialised; brick_list int32[max_list] scratch.
 *   cam2world / world2cam: row-major 4x4 HOST values (copied into the kernel arguments: no upload, no device allocation
 *   per frame); intrinsics by value.
 * All state is caller-owned; nothing is synchronised or read back.
 * ------------------------------------------------------------------------------------------ */
typedef struct sgam_tsdf_grid {
    float voxel_length, sdf_trunc;
    int32_t unit_base[3];    /* unit index (floor(world / (16 * voxel_length))) of the box's low corner, x y z */
    int32_t unit_dims[3];    /* units per axis */
} sgam_tsdf_grid;
/* (ABI v10) One source frame of a step: depth [H][W] fp32 and (with brick_color) rgb_u8 [H][W][3] DEVICE pointers; cam2world /
 * world2cam row-major 4x4 by value.  The array of n_src <= 8 of them is a HOST array, copied into the kernel arguments. */
typedef struct sgam_tsdf_src {
    const float *depth;
    const uint8_t *rgb_u8;
    float cam2world[16], world2cam[16];
} sgam_tsdf_src;
/* Integrates the n_src source frames of ONE step of the scene loop (reference :757-790 calls volume.integrate once per source)
 * in ONE pass over the union of the units they open: a voxel is loaded once, takes the sources' updates in array order and is
 * stored once — the same values as n_src single-source calls in that order.  step_id in 1 .. 2^23 - 1, distinct per call
 * (unit_stamp holds (step_id << 8) | mask of the step's sources that opened the unit). */
int sgam_tsdf_integrate_srcs_f32(const sgam_tsdf_grid *grid, const sgam_tsdf_src *srcs, int32_t n_src, int32_t H, int32_t W, float fx,
                                 float fy, float cx, float cy, float depth_trunc, int32_t step_id, int32_t *unit_table,
                                 int32_t *unit_stamp, int32_t *counters, int32_t *brick_list, int32_t max_list, float *brick_tsdf,
                                 float *brick_weight, int32_t max_bricks, float *brick_color, const float *ray_mult, void *stream);
/* ray_mult [H][W] fp32 = sqrt(((u - cx) / fx)^2 + ((v - cy) / fy)^2 + 1), the rule's depth -> camera-distance multiplier of a
 * pixel: tabulated once per (intrinsics, size) by this call, gathered by the integration beside the depth. */
int sgam_tsdf_ray_mult_f32(int32_t H, int32_t W, float fx, float fy, float cx, float cy, float *ray_mult, void *stream);
int sgam_tsdf_raycast_depth_f32(const sgam_tsdf_grid *grid, int32_t H, int32_t W, float fx, float fy, float cx, float cy,
                                const float *cam2world, float z_near, float z_far, const int32_t *unit_table,
                                const float *brick_tsdf, float *depth_out, const float *brick_color, float *color_out,
                                void *stream);

/* Scene-batched forms: S volumes that share ONE grid (and the step's intrinsics, size and n_src) advance through one launch per
 * pass, the scene being a grid dimension.  S x n_src descriptors do not fit the kernel arguments, so the tables are DEVICE
 * arrays the caller fills and uploads per step (on `stream`, before the call): scenes [S], srcs [S][n_src] (scene-major),
 * cam2world [S][16].  The library reads them on the device only; on the host it checks what it can see. */
typedef struct sgam_tsdf_scene {
    int32_t *unit_table, *unit_stamp, *counters, *brick_list;     /* DEVICE pointers: one scene's state, as above */
    float *brick_tsdf, *brick_weight, *brick_color;              /* brick_color NULL = geometry only */
    int32_t max_bricks, max_list;
} sgam_tsdf_scene;
/* What sgam_tsdf_integrate_srcs_f32 does for one volume, for S: per scene the values its own call would leave (every voxel
 * takes its scene's sources in array order; bricks may sit at other pool indices).  Three launches whatever S: a clear of the
 * S list lengths, the unit opening, the integration.  color != 0: every scene has brick_color and every source rgb_u8; 0:
 * none is read (both or neither, the same for all scenes — the caller's contract, the tables being device memory). */
int sgam_tsdf_integrate_scenes_f32(const sgam_tsdf_grid *grid, const sgam_tsdf_scene *scenes, const sgam_tsdf_src *srcs,
                                   int32_t n_scenes, int32_t n_src, int32_t H, int32_t W, float fx, float fy, float cx, float cy,
                                   float depth_trunc, int32_t step_id, int32_t color, const float *ray_mult, void *stream);
/* One launch: depth_out [S][H][W] (and color_out [S][H][W][3], optional: needs the scenes' brick_color) from S volumes at S poses;
 * per ray the computation of sgam_tsdf_raycast_depth_f32. */
int sgam_tsdf_raycast_scenes_f32(const sgam_tsdf_grid *grid, const sgam_tsdf_scene *scenes, const float *cam2world,
                                 int32_t n_scenes, int32_t H, int32_t W, float fx, float fy, float cx, float cy, float z_near,
                                 float z_far, float *depth_out, float *color_out, void *stream);

/* (ABI v6) Zero-crossing point extraction from the fused bricks: `volume.extract_point_cloud()` of the reference's run tail
 * (sgam/inference_pipeline.py:446-450 -> rgbd_integrated_mesh.ply), Open3D's published ScalableTSDFVolume::ExtractPointCloud
 * rule: per observed voxel with |tsdf| < 0.98 and each +x / +y / +z neighbour (same test) with the opposite sign, one point on
 * the edge at the |tsdf|-weighted position; colour weighted the same way (0..255, needs brick_color); normal = normalised
 * central difference of the trilinear field, one voxel each way.
 *   counter: device uint64, zero on entry; holds the number of points FOUND on return (a first call with points = NULL only
 *   counts).  points / normals / colors [max_points][3] fp32, keys [max_points] int64 = ((unit slot * 4096 + voxel) * 3 + axis)
 *   — the points arrive in no particular order, sorting by key gives a run-independent one.  Parity unpinned vs Open3D. */
int sgam_tsdf_extract_points_f32(const sgam_tsdf_grid *grid, const int32_t *unit_table, const float *brick_tsdf,
                                 const float *brick_color, uint64_t *counter, int64_t max_points, float *points,
                                 float *normals, float *colors, int64_t *keys, void *stream);

/* Marching-cubes triangle mesh of the fused bricks: `volume.extract_triangle_mesh()` (reference :777-826), Open3D's published
 * ScalableTSDFVolume::ExtractTriangleMesh rule on generated tables (csrc/mc_tables.h; not Open3D's table: the same surface on
 * non-ambiguous faces, the ambiguous-face choice unpinned).  A cell (its low lattice point) is processed when its 8 corners
 * are observed (tsdf <= 1); one vertex per lattice edge, keyed like sgam_tsdf_extract_points_f32 and at the same fp32
 * position / colour (0..255, vertex_colors needs brick_color); vertices in key order, triangles in (cell key, table order):
 * deterministic, no sorting, no host round trip.  counters: the volume's counters (bricks allocated = counters[0]).
 *   cull_world2cam: NULL = the whole volume; else a HOST row-major 4x4 and (H, W, fx, fy, cx, cy, z_near, z_far): units whose
 *   box grown by one voxel lies outside the view frustum are skipped (what the mesh depth render needs).
 *   vertices [max_vertices][3] fp32, vertex_colors [max_vertices][3] (optional), keys [max_vertices] int64 (optional),
 *   triangles [max_triangles][3] int32 (indices into vertices; both winding and order deterministic).
 *   mesh_counts int32[4] device, zero-initialised once: {vertices found, triangles found, entries dropped by this call
 *   (found beyond the capacities), running total of the dropped entries} — overflow is never silent.
 *   workspace: sgam_tsdf_mesh_workspace_bytes(grid, max_bricks) bytes, no initialisation. */
int64_t sgam_tsdf_mesh_workspace_bytes(const sgam_tsdf_grid *grid, int32_t max_bricks);
int sgam_tsdf_extract_mesh_f32(const sgam_tsdf_grid *grid, const int32_t *unit_table, const int32_t *counters, const float *brick_tsdf,
                               const float *brick_color, int32_t max_bricks, const float *cull_world2cam, int32_t H, int32_t W,
                               float fx, float fy, float cx, float cy, float z_near, float z_far, float *vertices,
                               float *vertex_colors, int64_t *keys, int64_t max_vertices, int32_t *triangles, int64_t max_triangles,
                               int32_t *mesh_counts, void *workspace, int64_t workspace_bytes, void *stream);
/* Depth render of a triangle mesh (csrc/mesh_raster.hip): the reference's render_to_depth_image(z_in_view_space=True) with
 * inf -> 0.  Samples at integer pixel coordinates; near clipping in view space; 24.8 fixed-point coverage with a top-left
 * rule (no cracks, no double coverage on shared edges); perspective-correct z; fragments outside [z_near, z_far] dropped;
 * nearest by atomicMin on the z bits (deterministic).  The triangle count is read from mesh_counts[1] (device; clamped to
 * max_triangles, indices checked against min(mesh_counts[0], max_vertices)): no sync after the extraction.
 * world2cam: HOST row-major 4x4.  depth_out [H][W] fp32 (also the depth buffer: no workspace). */
int sgam_mesh_render_depth_f32(const float *vertices, int64_t max_vertices, const int32_t *triangles, int64_t max_triangles,
                               const int32_t *mesh_counts, int32_t H, int32_t W, float fx, float fy, float cx, float cy,
                               const float *world2cam, float z_near, float z_far, float *depth_out, void *stream);
/* Coloured RGB-D render of a device mesh at P poses in one call (a fly-through: the pose is a grid dimension).  Transform,
 * near clip, 24.8 coverage, top-left rule, perspective-correct z and the z range are sgam_mesh_render_depth_f32's (shared
 * device functions): per pose, depth_out is bit for bit what that call writes.  Visibility: one 64-bit atomicMin per covered
 * sample on (z bits << 32) | (2 * triangle index + sub), sub = the second triangle of a near-clipped quad — an exact z tie goes
 * to the lower triangle index, order-independent and deterministic; max_triangles must be < 2^30 (SGAM_EINVAL otherwise).  A
 * resolve pass (one lane per sample) interpolates the winner's vertex_colors perspective-correctly — the fp32 expression is
 * stated at the top of csrc/mesh_raster.hip — and writes its geometric normal.
 *   vertex_colors [max_vertices][3] fp32 0..255, NULL for a mesh without colours (then rgb_out and rgb_u8_out must be NULL).
 *   world2cam: DEVICE [P][16] fp32 row-major 4x4s.  The counts are read from mesh_counts on the device, as above.
 *   depth_out [P][H][W] fp32: view-space z, 0 where nothing is hit.   rgb_out [P][H][W][3] fp32 0..255 (optional), 0 = no hit.
 *   normal_out [P][H][W][3] fp32 (optional): the winning triangle's unit normal in view space, facing the camera; 0 = no hit.
 *   rgb_u8_out [P][H][W][3] uint8 (optional): rgb clamped to 0..255 and truncated (the frame codec's rule).
 *   workspace: sgam_mesh_render_rgbd_workspace_bytes(P, H, W) = P * H * W * 8 bytes (the keys), 8-byte aligned, caller-owned,
 *   no initialisation (the call clears it).  P <= 65535. */
int64_t sgam_mesh_render_rgbd_workspace_bytes(int32_t P, int32_t H, int32_t W);
int sgam_mesh_render_rgbd_f32(const float *vertices, const float *vertex_colors, int64_t max_vertices, const int32_t *triangles,
                              int64_t max_triangles, const int32_t *mesh_counts, int32_t P, int32_t H, int32_t W, float fx, float fy,
                              float cx, float cy, const float *world2cam, float z_near, float z_far, float *depth_out,
                              float *rgb_out, float *normal_out, uint8_t *rgb_u8_out, void *workspace, int64_t workspace_bytes,
                              void *stream);
/* RGB-D views of F stored frames as a z-tested point splat at P poses in one call (csrc/point_raster.hip) — the view of a
 * finished scene that needs no volume: it reads the frame store in place.  Per source point (frame f, pixel q = i * Ws + j,
 * d = depth_f[i][j]); every operator is one IEEE fp32 operation in the written order, nothing fused:
 *     skip unless d is finite and d > 0
 *     a = (Kinv[0] * j + Kinv[1] * i) + Kinv[2]      b, c: rows 1, 2 likewise      (j, i as float)
 *     x = a * d   y = b * d   z = c * d
 *     X = ((T[0] * x + T[1] * y) + T[2] * z) + T[3]      Y: T[4..7]      Z: T[8..11]      (T = T_rel[p][f])
 *     skip unless z_near <= Z && Z <= z_far      (NaN fails)
 *     u = (fx * X) / Z + cx      v = (fy * Y) / Z + cy      uf = floorf(u + 0.5f)      vf = floorf(v + 0.5f)
 *     skip unless -(radius + 1) < uf && uf < W + radius && -(radius + 1) < vf && vf < H + radius      (float compares)
 *     px = (int)uf   py = (int)vf;   for dy, dx in [-radius, radius], where (px + dx, py + dy) is inside the view:
 *         atomicMin(keys[p][py + dy][px + dx], (uint64(bits of Z) << 32) | uint32(f * Hs * Ws + q))
 * Keys start as all ones (empty); an exact z tie goes to the lower id (the earlier frame, then the lower pixel): order-independent,
 * deterministic.  Resolve: empty -> depth 0, rgb 0, index -1; else depth = the float with the bits key >> 32, rgb = the winning
 * point's uint8 colour as fp32 0..255, index = the key's low 32 bits.  hole_fill = 1: every EMPTY sample's r, g, b and depth become
 * the 5th smallest of the nine values of its 3 x 3 window in the unfilled image (outside the image and empty = 0; fewer than five
 * hit neighbours: stays 0); hit samples and index_out do not change.
 *   depth_ptrs, rgb_ptrs: DEVICE arrays of F 64-bit addresses: depth [Hs][Ws] fp32 and colour [Hs][Ws][3] uint8 of each frame
 *   (F is not bounded by SGAM_MAX_SRCS; F * Hs * Ws < 2^32).   Kinv_src: HOST fp32[9], the float64 inverse of the source
 *   intrinsics rounded once.   T_rel: DEVICE [P][F][12] fp32, row-major 3 x 4, source camera -> view camera.
 *   fx, fy, cx, cy: the view's intrinsics (zero skew).   0 < z_near < z_far.   radius 0, 1 or 2: a (2 radius + 1)^2 footprint.
 *   hole_fill 0 or 1.
 *   depth_out [P][H][W] fp32;  rgb_out [P][H][W][3] fp32, rgb_u8_out [P][H][W][3] uint8, index_out [P][H][W] int32: optional.
 *   workspace: sgam_points_render_rgbd_workspace_bytes(P, H, W, hole_fill) bytes (the keys), 8-byte aligned, caller-owned, no
 *   initialisation (the call clears it).  1 <= P <= 65535.  Bad arguments: SGAM_EINVAL before any device call. */
int64_t sgam_points_render_rgbd_workspace_bytes(int32_t P, int32_t H, int32_t W, int32_t hole_fill);
int sgam_points_render_rgbd_f32(const void *depth_ptrs, const void *rgb_ptrs, int32_t F, int32_t Hs, int32_t Ws, const float *Kinv_src,
                                const float *T_rel, int32_t P, int32_t H, int32_t W, float fx, float fy, float cx, float cy,
                                float z_near, float z_far, int32_t radius, int32_t hole_fill, float *depth_out, float *rgb_out,
                                uint8_t *rgb_u8_out, int32_t *index_out, void *workspace, int64_t workspace_bytes, void *stream);

/* ------------------------------------------------------------------------------------------
 * f4 — backward / optimiser kernels of the training step: VQModel.training_step
 * (sgam/generative_sensing_module/model.py:271-345) with VQLPIPSWithDiscriminator.forward(optimizer_idx = 0)
 * (modules/losses/vqperceptual.py:77-110) at perceptual_weight = 0 and global_step < disc_start, i.e.
 * loss = mean|x - xrec| + codebook_weight * qloss, torch.optim.Adam(betas = (0.5, 0.9)) (model.py:414-428).
 * Every product of the backward pass runs on the forward's MFMA GEMM (sgam_conv2d_gn_nhwc_f32, fp32-in mode):
 *   data gradient    dcol[M][KH*KW*cin_pad] = dy[M][Cout] . W[Cout][KH*KW*cin_pad],   dx = sgam_col2im_gather_f32(dcol)
 *   weight gradient  dW[Cout][KH*KW*cin_pad] = dy^T[Cout][M] . col^T[KH*KW*cin_pad][M]^T,   col^T = sgam_im2col_t_f32(x)
 *                    (rows ld_m >= M apart: M is rounded up to the GEMM's K granule with a zero tail)
 * for every convolution of the model through ONE pair of index kernels driven by the forward's descriptor (3x3 / 1x1,
 * stride 1, Downsample's stride 2 with (0,1,0,1) padding, Upsample's nearest-2x folded into the conv); k = tap * cin_pad
 * + channel as in sgam_pack_conv_weight.  The PatchGAN and LPIPS pieces follow below.
 * ------------------------------------------------------------------------------------------ */
int sgam_im2col_t_f32(const sgam_conv_desc *d, const float *x, float *col_t, int32_t cin_pad, int64_t ld_m, void *stream);
int sgam_col2im_gather_f32(const sgam_conv_desc *d, const float *dcol, float *dx, int32_t cin_pad, void *stream);
int sgam_unpack_conv_weight_grad_f32(const float *grad_packed, int32_t ld, float *grad_oihw, int32_t Cout, int32_t Cin,
                                     int32_t KH, int32_t KW, int32_t Cin_pad, void *stream);
/* bias gradient: out[N] = column sums of a[M][N] (two launches, fixed order) */
int64_t sgam_colsum_workspace_bytes(int32_t M, int32_t N);
int sgam_colsum_f32(const float *a, int32_t lda, float *out, int32_t M, int32_t N, void *workspace, int64_t workspace_bytes,
                    void *stream);
/* GroupNorm(32, eps)(+swish) backward (Normalize + nonlinearity, diffusionmodules/model.py:30-40): x = the layer's input,
 * dy = gradient of its output, mean_rstd [B][groups][2] from sgam_groupnorm_stats_*; dx like x; dgamma_b / dbeta_b [B][C]
 * per-image sums (the caller adds the images); group_means [B][groups][2] scratch */
int64_t sgam_groupnorm_bwd_workspace_bytes(int32_t B, int32_t HW, int32_t C);
int sgam_groupnorm_bwd_nhwc_f32(const float *x, const float *dy, const float *mean_rstd, const float *gamma, const float *beta,
                                int32_t swish, float *dx, float *dgamma_b, float *dbeta_b, float *group_means, int32_t B,
                                int32_t HW, int32_t C, int32_t groups, void *workspace, int64_t workspace_bytes, void *stream);
/* p = softmax(scale * s) over rows (AttnBlock, model.py:176-181): ds = scale * p * (dp - sum_j dp_j p_j) */
int sgam_softmax_bwd_rows_f32(const float *p, const float *dp, float *ds, int32_t rows, int32_t cols, int32_t ld, float scale,
                              void *stream);
/* rec_loss = |inputs - reconstructions| (vqperceptual.py:79): grad[rows][ld_grad] = sign(rec - target) * grad_scale on the C
 * real columns (0 on the padding), partial[ceil(rows * ld_grad / 256)] doubles = sums of |rec - target| */
int sgam_l1_loss_grad_f32(const float *rec, const float *target, float *grad, double *partial, int64_t rows, int32_t C,
                          int32_t ld_rec, int32_t ld_grad, float grad_scale, void *stream);
/* VectorQuantizer2 backward (quantize.py:296-304, legacy form): dz = dzq + two_c * (z - zq) with two_c = 2 * codebook_weight /
 * numel; d_codebook[k] = two_c_beta * sum_{t: indices[t] = k} (zq_t - z_t) */
int sgam_vq_bwd_f32(const float *dzq, const float *z, const float *zq, float *dz, int64_t n, float two_c, void *stream);
int sgam_vq_codebook_grad_f32(const int64_t *indices, const float *z, const float *zq, float *d_codebook, int32_t T, int32_t n_e,
                              int32_t D, float two_c_beta, void *stream);
/* out = alpha * a + beta * b (b may be NULL): gradient fan-in of the residual connections */
int sgam_axpby_f32(const float *a, const float *b, float *out, int64_t n, float alpha, float beta, void *stream);
/* torch.optim.Adam step (no weight decay / amsgrad) on one tensor; step = 1, 2, ... */
int sgam_adam_step_f32(float *param, const float *grad, float *exp_avg, float *exp_avg_sq, int64_t n, float lr, float beta1,
                       float beta2, float eps, int32_t step, void *stream);
/* The same step for a whole parameter set in ONE launch (`opt.step()` over the 159 / 345 tensors of a phase).  All seven arrays are
 * DEVICE arrays: per tensor t the four pointers and numels[t]; per workgroup b the tensor block_tensor[b] it works on and the
 * first element block_off[b] of its 4096-element chunk (the host lists ceil(numel / 4096) workgroups per tensor, n_blocks in all). */
int sgam_adam_multi_step_f32(float *const *params, const float *const *grads, float *const *exp_avgs, float *const *exp_avg_sqs,
                             const int64_t *numels, const int32_t *block_tensor, const int64_t *block_off, int32_t n_blocks, float lr,
                             float beta1, float beta2, float eps, int32_t step, void *stream);

/* PatchGAN discriminator pieces (modules/discriminator/model.py:17-67; hinge loss and adaptive weight,
 * modules/losses/vqperceptual.py:17-21, 63-75): nn.BatchNorm2d in training mode over [rows = B*H*W][C] NHWC matrices
 * (mean_rstd [C][2] from the batch, biased variance; running_mean / running_var updated with the unbiased one), fused with
 * LeakyReLU; mean_rstd = NULL: LeakyReLU alone (the first layer).  Workspace: sgam_batchnorm_workspace_bytes. */
int64_t sgam_batchnorm_workspace_bytes(int32_t rows, int32_t C);
int sgam_batchnorm_stats_f32(const float *x, float *mean_rstd, float *running_mean, float *running_var, int32_t rows, int32_t C,
                             float eps, float momentum, void *workspace, int64_t workspace_bytes, void *stream);
int sgam_bn_lrelu_fwd_f32(const float *x, const float *mean_rstd, const float *gamma, const float *beta, float *y, int32_t rows,
                          int32_t C, float slope, void *stream);
int sgam_bn_lrelu_bwd_f32(const float *x, const float *dy, const float *mean_rstd, const float *gamma, const float *beta, float *dx,
                          float *dgamma, float *dbeta, float *gbuf, float *means, int32_t rows, int32_t C, float slope,
                          void *workspace, int64_t workspace_bytes, void *stream);
/* mode +1: relu(1 + l), -1: relu(1 - l) (hinge_d_loss); +2: softplus(l), -2: softplus(-l) (vanilla_d_loss, vqperceptual.py:17-28); 0: l;
 * grad = d(term)/dl * grad_scale, partial[ceil(n / 256)] = sums of the terms */
int sgam_hinge_terms_f32(const float *logits, float *grad, double *partial, int64_t n, int32_t mode, float grad_scale, void *stream);
int sgam_sumsq_partial_f32(const float *a, double *partial, int64_t n, void *stream);

/* LPIPS pieces (modules/losses/lpips.py:10-123): MaxPool2d(2, 2) of the VGG16 trunk and its backward (gradient to the first
 * maximum of the window), ScalingLayer ((x - shift) / scale on the RGB channels into a zero-padded NHWC tensor; with shift 0 the
 * same kernel is its backward), and one feature level of the metric: val_b = mean_p sum_c w_c (f0/(|f0|+eps) - f1/(|f1|+eps))^2
 * (normalize_tensor -> squared difference -> NetLinLayer -> spatial_average) with its gradient w.r.t. f0. */
int sgam_maxpool2x2_f32(const float *x, float *y, int32_t B, int32_t H, int32_t W, int32_t C, void *stream);
int sgam_maxpool2x2_bwd_f32(const float *x, const float *dy, float *dx, int32_t B, int32_t H, int32_t W, int32_t C, void *stream);
int sgam_channel_affine_f32(const float *x, int32_t ldx, float *y, int32_t ldy, int64_t rows, int32_t n, const float *shift4,
                            const float *inv_scale4, void *stream);
int sgam_lpips_level_f32(const float *f0, const float *f1, const float *lin_w, double *partial, float *df0, int32_t B, int32_t HW,
                         int32_t C, float eps, float grad_scale, void *stream);

/* Validation step and image metrics (csrc/eval.hip; VQModel.evaluation_loop, model.py:356-410, and modules/misc/metrics.py).
 * Like the training kernels: caller-owned buffers, launches on `stream`, no sync, per-workgroup fp64 partial sums that the
 * caller folds on the host (deterministic: no float atomics).
 *
 * sgam_recon_stats_f32: ONE pass over reconstruction rec[B*HW][ld_rec] and target[B*HW][C] (NHWC fp32, C real channels), no
 * gradient.  partial[B][chunks][6] with chunks = ceil(HW / 1024) (sgam_recon_stats_partials = B * chunks * 6 doubles):
 *   0 sum|d| over all channels (rec_loss), 1 sum|d| over channels 0..2 (val/rgb_l1), 2 sum|d| over channels >= 3
 *   (val/disparity_l1); with with_sq: 3 sum d^2 over channels 0..2, 4 sum d^2 * mask[pixel], 5 sum mask[pixel] (PSNR and its
 *   visible form; mask [B*HW] fp32 or NULL -> 4 and 5 are 0; an all-zero mask leaves 4 = 5 = 0 and the caller's 0 / 0 is a NaN
 *   by definition, see metrics.psnr).  map255: the squared error is taken after clip((v + 1) * 127.5, 0, 255) of both sides. */
int64_t sgam_recon_stats_partials(int32_t B, int32_t HW);
int sgam_recon_stats_f32(const float *rec, const float *target, const float *mask, double *partial, int32_t B, int32_t HW, int32_t C,
                         int32_t ld_rec, int32_t with_sq, int32_t map255, void *stream);
/* SSIM._ssim (metrics.py:59-83) per image and channel: 11 x 11 Gaussian window (sigma 1.5, separable), valid region
 * (H - 10) x (W - 10), C1 = (0.01 * 255)^2, C2 = (0.03 * 255)^2, moments accumulated in fp64.  img1 / img2 [B][H][W][ld] NHWC fp32
 * (channels 0..C-1 are used), on the 0..255 scale or, with map255, mapped from [-1, 1] as above.  partial[B][C][tiles][3] with
 * tiles = ceil((H-10)/16) * ceil((W-10)/16) (sgam_ssim_partials doubles in all): sum ssim_map, sum ssim_map * mask[5:-5, 5:-5],
 * sum mask[5:-5, 5:-5] (mask [B][H][W] fp32 or NULL -> the last two are 0).  H < 11 or W < 11: SGAM_EINVAL. */
int64_t sgam_ssim_partials(int32_t B, int32_t H, int32_t W, int32_t C);
int sgam_ssim_f32(const float *img1, const float *img2, const float *mask, double *partial, int32_t B, int32_t H, int32_t W, int32_t C,
                  int32_t ld1, int32_t ld2, int32_t map255, void *stream);
/* hist[k] += number of indices equal to k (int32 [n_embed], NOT cleared: it accumulates over the batches of a validation
 * epoch; integer atomics, order-independent); indices outside [0, n_embed) are skipped */
int sgam_index_histogram_i32(const int64_t *indices, int64_t n, int32_t *hist, int32_t n_embed, void *stream);

/* ------------------------------------------------------------------------------------------
 * Device-resident online k-means codebook refresh (csrc/kmeans.hip; VQModel.training_step, model.py:274-295 and :313-323, whose
 * host call is scipy.cluster.vq.kmeans2(features, n_dead, minit='points')).  Added to ABI v10 (new symbols only, no signature
 * changed).  Like the training kernels: caller-owned buffers, launches on `stream`, no sync, no float atomics — every
 * floating-point sum is folded in an order fixed by the data (ascending point id), so results are run-to-run identical and do not
 * depend on chunk / block sizes.  The Lloyd loop itself (assign, update, ... a fixed number of times) is sequenced by the caller.
 *   x [N][D] points (fp32, 16-byte aligned), centres [k][D], labels [N] int32, count [k] int32.
 *
 * sgam_kmeans_assign_f32: labels[i] = arg-min_j d_ij, d_ij = (|x_i|^2 + |c_j|^2) - 2 x_i.c_j in the quantiser's expression order
 *   (sgam_vq_nearest_f32: the same GEMM kernel for x.c^T, the same fmaf chains for the squared norms), first index among exact
 *   ties.  Tiled over N: the dot products of `chunk` points at a time ([chunk][k_pad] floats, never [N][k]); k need not be a
 *   multiple of anything: the centre table is copied into the workspace padded to k_pad = 128 * ceil(k / 128) rows whose |c|^2 is
 *   +inf, so they never win.  D % 32 == 0.  chunk: any positive value, sgam_kmeans_chunk_points(N, D, k) is the default
 *   (at most 256 MiB of dot products); labels do not depend on it.  workspace: sgam_kmeans_assign_workspace_bytes(N, D, k,
 *   chunk) bytes, 256-byte aligned.
 *
 * sgam_kmeans_update_f32: centres[j] = fp32(sum of the points labelled j / count[j]), count[j] written; a centre WITHOUT members
 *   keeps its previous value (kmeans2(..., missing='warn')).  Stable counting sort of the point ids by label (per-block integer
 *   histograms of block_points consecutive points, scans, placement), then one workgroup per centre: wavefront w = 0..3 adds the
 *   members number w, w + 4, ... of the cluster (members in ascending point id) in fp64, the four sums are joined as
 *   (s0 + s1) + (s2 + s3), divided by the count in fp64 and rounded once to fp32.  block_points: 0 = 1024, else a multiple of 256 up to
 *   4096; the result does not depend on it.  Labels outside [0, k) are ignored.  D % 4 == 0.  workspace:
 *   sgam_kmeans_update_workspace_bytes(N, k, block_points) bytes, 256-byte aligned.
 *
 * sgam_kmeans_init_points_f32 (minit='points'): centres[s] = x[pick(s)] for k DISTINCT rows, picks [k] int32 (may be NULL).
 *   The picks are the first k values of a keyed pseudo-random permutation of [0, N) — distinct by construction, no sort, no redraw:
 *     h = the smallest integer >= 1 with 4^h >= N (at most 16), mask = 2^h - 1;
 *     P(v): (L, R) = (v >> h, v & mask); four times, r = 0..3: F = word 0 of Philox4x32-10 (multipliers 0xD2511F53, 0xCD9E8D57;
 *           Weyl 0x9E3779B9, 0xBB67AE85) with key = (seed lo32, seed hi32) and counter = (R, r, refresh lo32, refresh hi32);
 *           (L, R) = (R, L ^ (F & mask));  P(v) = (L << h) | R   — a Feistel network, hence a bijection of [0, 4^h);
 *     pick(s): v = P(s); while v >= N: v = P(v)   (cycle walking: the restriction of P to [0, N) is again a bijection).
 *   `refresh` is the caller's refresh number: another number, another permutation.  k <= N.
 *
 * sgam_codebook_countdown_i32 (model.py:313-323, train_codebook_map) in ONE launch of one workgroup: countdown[indices[t]] = timeout
 *   for the T indices (the first image's), then countdown[j] -= 1 for every word; n_dead[0] = #{j: countdown[j] <= 0} AFTER the
 *   decrement — what the next step's firing test reads (model.py:278) — and dead[0 .. n_dead) = those words in ascending order
 *   (dead has room for n_embed entries).  countdown [n_embed] int32.
 *
 * sgam_codebook_scatter_rows_f32 (VectorQuantizer2.update_codebook): codebook[dead[i]][:] = centres[i][:] for i < n_rows; with
 *   countdown != NULL also countdown[dead[i]] = timeout (model.py:290-291).
 * ------------------------------------------------------------------------------------------ */
int32_t sgam_kmeans_chunk_points(int32_t N, int32_t D, int32_t k);
int64_t sgam_kmeans_assign_workspace_bytes(int32_t N, int32_t D, int32_t k, int32_t chunk);
int sgam_kmeans_assign_f32(const float *x, const float *centres, int32_t *labels, int32_t N, int32_t D, int32_t k, int32_t chunk,
                           void *workspace, int64_t workspace_bytes, void *stream);
int64_t sgam_kmeans_update_workspace_bytes(int32_t N, int32_t k, int32_t block_points);
int sgam_kmeans_update_f32(const float *x, const int32_t *labels, float *centres, int32_t *count, int32_t N, int32_t D, int32_t k,
                           int32_t block_points, void *workspace, int64_t workspace_bytes, void *stream);
int sgam_kmeans_init_points_f32(const float *x, float *centres, int32_t *picks, int32_t N, int32_t D, int32_t k, uint64_t seed,
                                uint64_t refresh, void *stream);
int sgam_codebook_countdown_i32(const int64_t *indices, int32_t T, int32_t *countdown, int32_t n_embed, int32_t timeout,
                                int32_t *n_dead, int32_t *dead, void *stream);
int sgam_codebook_scatter_rows_f32(float *codebook, const float *centres, const int32_t *dead, int32_t n_rows, int32_t D,
                                   int32_t n_embed, int32_t *countdown, int32_t timeout, void *stream);

/* ---------------------------------------------------------------------------------------------
 * Training data path (csrc/imageio.hip): what the reference's datasets do to a decoded frame (data/google_earth.py:162-183).
 *
 * sgam_resize_lanczos_u8: PIL `Image.resize(..., LANCZOS)` of M uint8 RGB images src [M][Hin][Win][3] -> [M][Hout][Wout][3] in one
 *   launch, bit for bit: horizontal pass, uint8 intermediate, vertical pass, each output clip((2^21 + sum pixel * k) >> 22, 0, 255).
 *   The caller computes the tables of an axis once per (in, out) size in float64: bounds [out][2] int32 = (first input index, taps),
 *   coef [out][K] int32 = the normalised Lanczos-3 weights rounded half away from zero to 22 fractional bits, zero past `taps`.
 *   `*_host` are host copies of the bounds (validated and used to size the tile), the others device pointers.  Bounds must be
 *   non-decreasing in both their start and their end, inside the input, taps in [1, K]; otherwise SGAM_EINVAL.
 *   Outputs (either or both): out_u8 [M][Hout][Wout][3], out_f32 the same shape in fp32 = lut256[u8] (lut256 [256] device floats,
 *   float32(u / 127.5 - 1.0)) — a dense slice of the caller's batch tensor.  Hin == Hout and Win == Wout: the table conversion
 *   alone, the tables of both axes may be NULL.
 *
 * sgam_resize_nearest_f32: `F.interpolate(mode='nearest')` of M depth maps src [M][Hin][Win] -> out [M][Hout][Wout]: source index
 *   min(int(floorf(dst * (float)in / out)), in - 1) per axis.  mask_out (optional) [M][Hout][Wout] = (value != sentinel) as 0 / 1
 *   floats; with `replace` != 0, values equal to `sentinel` are written as `replacement` (65504 -> -99999 on source depths).  `out`
 *   may be NULL when only the mask is wanted.
 *
 * sgam_resize_bicubic_u8: `Image.resize(size)` with Pillow's default filter (BICUBIC, a = -0.5, support 2), what the codebook phase's
 *   single-frame dataset calls (data/base.py:68, 96).  The same two fixed-point passes as sgam_resize_lanczos_u8 over tables the
 *   caller computed with the bicubic filter (same layout, same validation).  fp32 output only, lut256[u8], written to
 *   out_f32[((m * Hout + y) * Wout + x) * pixel_stride + c], c in 0..2, pixel_stride 3 or 4: with 4, the RGB channels of an
 *   [M][Hout][Wout][4] RGB-D batch tensor, whose fourth channel is left untouched.
 *
 * sgam_frame_depth_codec_f32: that dataset's depth channel (data/base.py:76-88, 104-115) for M maps src [M][Hin][Win] (fp32; half
 *   files are staged as fp32, which is lossless) in one launch: nearest resize by the index rule of sgam_resize_nearest_f32, then
 *     mode 0 (half steps)  t = d + add; i = 1 / t; s = (i - sub) / div; r = 2 * s - 1, each operation computed in fp32 and rounded
 *                          to half (numpy's arithmetic on a float16 file);
 *     mode 1 (fp32 steps)  the same operations in fp32 (a float32 file);
 *     mode 2 (fp64, rays)  z = d * k00 / sqrt(k00sq + (k02 - y - 0.5)^2 + (k12 - x - 0.5)^2) with y the output row and x the output
 *                          column, then i = 1 / z; s = (i - sub) / div; r = 2 * s - 1, all in fp64, cast to fp32 (CLEVR-infinite).
 *   consts7 (HOST pointer, 7 doubles) = {add, sub, div, k00, k00sq, k02, k12}, rounded by the caller to the precision of the mode;
 *   the kernel derives none of them.  Every operation is one correctly rounded IEEE operation.  The result goes to
 *   out[((m * Hout + y) * Wout + x) * pixel_stride + channel], 0 <= channel < pixel_stride <= 4; nothing else is written.
 *   SGAM_EINVAL for NULL pointers, empty shapes, an unknown mode, div == 0 or a channel outside the stride: nothing is launched.
 * ------------------------------------------------------------------------------------------ */
int sgam_resize_lanczos_u8(const uint8_t *src, int32_t M, int32_t Hin, int32_t Win, int32_t Hout, int32_t Wout,
                           const int32_t *hbounds_host, const int32_t *hbounds, const int32_t *hcoef, int32_t KH,
                           const int32_t *vbounds_host, const int32_t *vbounds, const int32_t *vcoef, int32_t KV,
                           const float *lut256, uint8_t *out_u8, float *out_f32, void *stream);
int sgam_resize_nearest_f32(const float *src, int32_t M, int32_t Hin, int32_t Win, int32_t Hout, int32_t Wout, float *out,
                            int32_t replace, float sentinel, float replacement, float *mask_out, void *stream);
int sgam_resize_bicubic_u8(const uint8_t *src, int32_t M, int32_t Hin, int32_t Win, int32_t Hout, int32_t Wout,
                           const int32_t *hbounds_host, const int32_t *hbounds, const int32_t *hcoef, int32_t KH,
                           const int32_t *vbounds_host, const int32_t *vbounds, const int32_t *vcoef, int32_t KV,
                           const float *lut256, float *out_f32, int32_t pixel_stride, void *stream);
int sgam_frame_depth_codec_f32(const float *src, int32_t M, int32_t Hin, int32_t Win, int32_t Hout, int32_t Wout, int32_t mode,
                               const double *consts7, float *out, int32_t pixel_stride, int32_t channel, void *stream);

/* ---------------------------------------------------------------------------------------------
 * Scene geometry metrics (csrc/point_nn.hip): the frame store as one cloud, exact nearest neighbours, the sums of the metrics.
 * Every fp32 operator is one IEEE operation in the written order (restated in tests/geometry_oracle.py, compared bit for bit).
 * A point with a coordinate that is not finite is "not a point": never a neighbour, and as a query it has none.
 *
 * sgam_points_unproject_f32: F stored frames -> points_out [F * Hs * Ws][3] fp32 (world) and colors_out [F * Hs * Ws][3] uint8,
 *   frame-major then row-major pixels, in one launch.  depth_ptrs / rgb_ptrs: DEVICE tables of F addresses (the tables of
 *   sgam_points_render_rgbd_f32); Kinv [9] HOST (the float64 inverse rounded once); T_c2w [F][12] DEVICE (camera -> world, float64
 *   inverse rounded once).  Pixel (i, j), depth d:
 *     a = (Kinv[0] * j + Kinv[1] * i) + Kinv[2]   (b: Kinv[3..5], c: Kinv[6..8]);   x = a * d, y = b * d, z = c * d
 *     X = ((T[0] * x + T[1] * y) + T[2] * z) + T[3]   (Y: T[4..7], Z: T[8..11])
 *   unless d is finite and z_near <= d <= z_far: X = Y = Z = NaN (the colour is copied all the same).  rgb_ptrs and colors_out
 *   are given together or both NULL (geometry only).  F * Hs * Ws < 2^31.
 *
 * Distance: dx = p.x - q.x (dy, dz alike), d2 = (dx * dx + dy * dy) + dz * dz.  The neighbour of a query is the reference point
 *   of least (d2, index) among those with d2 <= max_d2 (+inf: no limit; the caller squares its distance limit in fp32): an exact
 *   tie goes to the lower index.  No such point: index -1, d2 +inf.
 *
 * sgam_points_nn_brute_f32: query [B][Nq][3] against ref [B][Nr][3] (independent clouds) -> d2_out [B][Nq], index_out [B][Nq];
 *   every pair is evaluated (reference tiles of 1024 points through LDS, one lane per query).  B <= 65535.
 *
 * sgam_points_grid_build / sgam_points_nn_grid_f32: the same results from a uniform grid of gx x gy x gz cubic cells of edge
 *   cell_size with its low corner at (ox, oy, oz) — the caller passes the box of the valid reference points and chooses the cells;
 *   a point's cell is clamp(floorf((p - origin) / cell_size), 0, g - 1) per axis, so ANY box gives the exact result and the box
 *   only decides the speed.  At most 2^24 cells.  The build sorts the valid reference points by cell into the workspace
 *   (sgam_points_grid_workspace_bytes(Nr, gx, gy, gz) = 16 Nr + r16(4 (C + 1)) + r16(4 C) + r16(4 ceil(C / 1024)) bytes, C the cell
 *   count, r16 = rounded up to 16; 16-byte aligned); the query reads that workspace and must be given the same Nr and grid.  It
 *   visits the cells in growing shells around the query's (clamped) cell and stops when no unvisited point can win or tie
 *   (the rule and its margin: csrc/point_nn.hip); results do not depend on the cells chosen.
 *
 * sgam_points_nn_reduce: d2 [n] -> partials [sgam_points_nn_reduce_partials(n) = 4 * ceil(n / 4096)] doubles, per block of 4096
 *   values {sum d2, sum sqrt(d2), number of finite d2, number of finite d2 with d2 <= tau * tau (in fp64: sqrt(d2) <= tau)}, in a
 *   fixed order; the caller adds the blocks up.
 *
 * SGAM_EINVAL, nothing launched: NULL pointers, counts < 1, a grid above the cell cap, a cell_size or origin that is not finite
 *   and positive / finite, a workspace that is missing, short or unaligned, max_d2 or tau negative or NaN.
 * ------------------------------------------------------------------------------------------ */
int sgam_points_unproject_f32(const void *depth_ptrs, const void *rgb_ptrs, int32_t F, int32_t Hs, int32_t Ws, const float *Kinv,
                              const float *T_c2w, float z_near, float z_far, float *points_out, uint8_t *colors_out, void *stream);
int sgam_points_nn_brute_f32(const float *query, const float *ref, int32_t B, int32_t Nq, int32_t Nr, float max_d2, float *d2_out,
                             int32_t *index_out, void *stream);
int64_t sgam_points_grid_workspace_bytes(int32_t Nr, int32_t gx, int32_t gy, int32_t gz);
int sgam_points_grid_build(const float *ref, int32_t Nr, float ox, float oy, float oz, float cell_size, int32_t gx, int32_t gy,
                           int32_t gz, void *workspace, int64_t workspace_bytes, void *stream);
int sgam_points_nn_grid_f32(const float *query, int32_t Nq, int32_t Nr, float ox, float oy, float oz, float cell_size, int32_t gx,
                            int32_t gy, int32_t gz, const void *workspace, int64_t workspace_bytes, float max_d2, float *d2_out,
                            int32_t *index_out, void *stream);
int64_t sgam_points_nn_reduce_partials(int64_t n);
int sgam_points_nn_reduce(const float *d2, int64_t n, float tau, double *partials, void *stream);

/* ---------------------------------------------------------------------------------------------
 * Cloud clean-up (csrc/point_nn.hip, csrc/point_cloud.hip): k nearest neighbours, uniform voxel sampling, the
 * sums of the statistical outlier rule, normals.  Distances, "not a point" and max_d2 as above; restated in tests/cloud_oracle.py.
 *
 * sgam_points_knn_brute_f32 / sgam_points_knn_grid_f32: query [Nq][3] against ref [Nr][3] -> d2_out [Nq][k], index_out [Nq][k]:
 *   row i = the k least (d2 bits, index) pairs among the candidates of query i (d2 <= max_d2, d2 finite), ascending; a row with
 *   fewer candidates ends in index -1 / d2 +inf.  1 <= k <= 32.  exclude_self = 1 (Nq == Nr, query and ref the same cloud) skips
 *   the candidate whose index is the query's.  k = 1 gives the bits of sgam_points_nn_brute_f32 / sgam_points_nn_grid_f32.  The
 *   grid form reads the workspace sgam_points_grid_build made and must be given the same Nr and grid.
 *
 * sgam_points_voxel_sample_f32: points [N][3] -> keep_out [N] (1 for the ONE kept point of every occupied voxel, else 0) and
 *   count_out [N] (the voxel's number of members at its kept point, else 0).  Per axis in fp32: v = floorf((p - o) / voxel_size),
 *   centre c = o + (v + 0.5f) * voxel_size; kept: the member of least (d2(p, c) bits, index).  The caller keeps every |v| below
 *   2^20 (v is clamped into 21 bits).  workspace: sgam_points_voxel_workspace_bytes(N) = 20 T + r16(4 N) bytes, T = the least
 *   power of two >= max(2 N, 256), 16-byte aligned; N <= 2^29.  overflow_flag: one DEVICE int32 the caller zeroed; set to 1 if a
 *   point found no slot within T probes (the probe loop is bounded; cannot happen with an intact workspace).
 *
 * sgam_points_knn_mean_distance: d2 [N][k], index [N][k] (a k-NN result) -> md_out [N] double: the mean of sqrt((double)d2) over the
 *   entries with index >= 0, ascending column order; none: NaN.
 * sgam_points_md_reduce: md [n] -> partials [sgam_points_md_reduce_partials(n) = 2 * ceil(n / 4096)] doubles, per block of 4096
 *   values {sum of (md - shift) (squared = 0) or of (md - shift)^2 (squared = 1) over the finite md, their number}.
 *
 * sgam_points_normals_f32: points [N][3], knn_index [N][k] (entries < 0 skipped) -> normals_out [N][3]: the unit eigenvector of the
 *   least eigenvalue of the neighbourhood's fp64 covariance (cyclic Jacobi, a fixed number of sweeps), rounded to fp32 once; fewer
 *   than 3 neighbours: NaN.  viewpoints [V][3] + view_of [N] (both or neither; V = 0 without): flipped towards
 *   viewpoints[view_of[i]]; otherwise (or view_of[i] outside [0, V)) the component of largest magnitude is made positive.
 *
 * SGAM_EINVAL, nothing launched: NULL pointers, counts < 1, k outside 1..32, exclude_self with Nq != Nr, a voxel_size or origin that
 *   is not finite and positive / finite, a workspace that is missing, short or unaligned, viewpoints without view_of.
 * ------------------------------------------------------------------------------------------ */
int sgam_points_knn_brute_f32(const float *query, const float *ref, int32_t Nq, int32_t Nr, int32_t k, float max_d2, int32_t exclude_self,
                              float *d2_out, int32_t *index_out, void *stream);
int sgam_points_knn_grid_f32(const float *query, int32_t Nq, int32_t Nr, float ox, float oy, float oz, float cell_size, int32_t gx,
                             int32_t gy, int32_t gz, const void *workspace, int64_t workspace_bytes, int32_t k, float max_d2,
                             int32_t exclude_self, float *d2_out, int32_t *index_out, void *stream);
int64_t sgam_points_voxel_workspace_bytes(int32_t N);
int sgam_points_voxel_sample_f32(const float *points, int32_t N, float ox, float oy, float oz, float voxel_size, void *workspace,
                                 int64_t workspace_bytes, uint8_t *keep_out, int32_t *count_out, int32_t *overflow_flag, void *stream);
int sgam_points_knn_mean_distance(const float *d2, const int32_t *index, int32_t N, int32_t k, double *md_out, void *stream);
int64_t sgam_points_md_reduce_partials(int64_t n);
int sgam_points_md_reduce(const double *md, int64_t n, double shift, int32_t squared, double *partials, void *stream);
int sgam_points_normals_f32(const float *points, int32_t N, const int32_t *knn_index, int32_t k, const float *viewpoints, int32_t V,
                            const int32_t *view_of, float *normals_out, void *stream);

/* ------------------------------------------------------------------------------------------
 * Rigid registration (csrc/point_icp.hip): ICP of a source cloud onto a target cloud on top of the searches above.
 * One iteration = sgam_points_transform_f32, a nearest-neighbour search (sgam_points_nn_brute_f32 / sgam_points_nn_grid_f32 with
 * max_d2 = the squared correspondence distance), sgam_points_icp_accumulate, sgam_points_icp_update: the pose, the stop state and
 * the history are DEVICE memory, nothing is read back.  "not a point" as above; no float atomics; every output is a function of
 * the inputs only and equal run to run; restated in tests/icp_oracle.py.
 *
 * sgam_points_transform_f32: points [N][3] -> out [N][3].  T: 16 DEVICE doubles, a row-major 4 x 4; T[0..11] are rounded to fp32
 *   once and applied in fp32 as  X = ((T[0] * x + T[1] * y) + T[2] * z) + T[3]  (Y: T[4..7], Z: T[8..11]), one IEEE operation per
 *   operator: the unprojection's expression.  A point that is not a point comes out NaN.
 *
 * sgam_points_icp_accumulate: moved [N][3] (the transformed source), target [Nr][3], target_normals [Nr][3] or NULL, index [N] and
 *   d2 [N] (the search's result for `moved`) -> partials [sgam_points_icp_partials(N) = 32 * ceil(N / 4096)] doubles: 32 sums per
 *   chunk of 4096 source points.  Entry i is a CORRESPONDENCE iff 0 <= index[i] < Nr and, with normals, the normal at index[i] is a
 *   point (all three finite).  Per correspondence in fp64 on the widened fp32 inputs, one IEEE operation per operator in the written
 *   order: p = moved[i], q = target[index[i]], n = the normal, e = (p.x - q.x, p.y - q.y, p.z - q.z).
 *     point-to-plane (normals given):  c = (p.y n.z - p.z n.y, p.z n.x - p.x n.z, p.x n.y - p.y n.x), J = (c.x, c.y, c.z, n.x, n.y, n.z),
 *       r = (e.x n.x + e.y n.y) + e.z n.z;  summands: J[a] * J[b] (slot of (a, b)), J[a] * r (slot 21 + a), r * r (slot 27).
 *     point-to-point (NULL): the rows J = [-[p]x | I] with the residuals e, the three rows' products summed per point:
 *       (0,0) p.y p.y + p.z p.z  (0,1) -(p.x p.y)  (0,2) -(p.x p.z)  (1,1) p.x p.x + p.z p.z  (1,2) -(p.y p.z)  (2,2) p.x p.x + p.y p.y
 *       (0,4) -p.z  (0,5) p.y  (1,3) p.z  (1,5) -p.x  (2,3) -p.y  (2,4) p.x  (3,3) (4,4) (5,5) 1, every other entry 0;
 *       slots 21..23: p.y e.z - p.z e.y, p.z e.x - p.x e.z, p.x e.y - p.y e.x;  slots 24..26: e.x, e.y, e.z;
 *       slot 27: (e.x e.x + e.y e.y) + e.z e.z.
 *   Slots 0..20: the upper triangle of J^T J row-major ((0,0..5) = 0..5, (1,1..5) = 6..10, (2,2..5) = 11..14, (3,3..5) = 15..17,
 *   (4,4..5) = 18..19, (5,5) = 20); 21..26: J^T r; 27: sum r^2 (sum |e|^2); 28: sum (double)d2[i]; 29: the number of
 *   correspondences; 30: the number of source points of the chunk that are points; 31: 0.  A lane sums its points in index order
 *   (i = chunk base + c * 256 + lane, ascending c), the lanes are folded as in sgam_points_md_reduce: a fixed order.
 *
 * sgam_points_icp_update: partials [blocks][32] (blocks = ceil(N / 4096)) -> one Gauss-Newton step on state, one row of history.
 *   state: 24 DEVICE doubles: [0..15] T (row-major 4 x 4, source -> target), [16] previous fitness, [17] previous RMSE, [18] status
 *   (0 running, 1 converged, 2 degenerate), [19] iterations applied, [20] correspondences and [21] sum r^2 of the iteration
 *   evaluated last, [22..23] 0.  The caller starts with T = its initial pose and zeros.  history [rows][8] doubles, row `iteration` =
 *   {fitness, RMSE, correspondences, sum r^2, |omega|, |v|, status after this call, 0}.  All in fp64:
 *     1. status != 0: the row is {state[16], state[17], state[20], state[21], 0, 0, status, 0}; nothing else changes (the state is
 *        frozen: the host loop never has to look).
 *     2. the chunks are folded in ascending order.  fitness = count / points, rmse = sqrt(sum d2 / count) (Open3D's definition:
 *        point distances whatever the estimation); they and count, sum r^2 go to state[16], [17], [20], [21] in each case below.
 *     3. count < 6: status 2, T untouched.
 *     4. iteration > 0 and |fitness - previous| < relative_fitness and |rmse - previous| < relative_rmse: status 1, T untouched
 *        (Open3D too stops before the update).
 *     5. A = J^T J = L L^T by Cholesky; a pivot A_jj - sum_k<j L_jk^2 that is not finite or <= 1e-12 * A_jj (ICP_PIVOT_REL, relative
 *        to the matrix's own diagonal entry: a plane sliding along itself must not produce a huge step): status 2, T untouched.
 *     6. xi = -A^-1 J^T r, omega = xi[0..2], v = xi[3..5]; theta^2 = omega . omega; a = sin(theta) / theta, b = (1 - cos(theta)) /
 *        theta^2, or 1 and 1/2 when theta^2 < 1e-16; dR = I + a [omega]x + b (omega omega^T - theta^2 I); T <- [dR | v] T;
 *        iterations += 1.
 *
 * Coloured ICP (Park, Zhou, Koltun, ICCV 2017; Open3D's registration_colored_icp as documented, unpinned): the colours of the two
 * clouds pin the pose where the geometry leaves it free (a plane).  Intensity of a point with the uint8 colour (r, g, b):
 * I = (double)(r + g + b) / 765.0, the sum an integer.  Restated in tests/colored_icp_oracle.py.
 *
 * sgam_points_color_gradient_f32: points [N][3], normals [N][3], colors [N][3] uint8, knn_index [N][k] (a k-NN row of the cloud
 *   against itself, the point excluded; entries outside [0, N) are skipped) -> gradient_out [N][3]: the least-squares gradient of
 *   the intensity in the tangent plane.  One lane per point p with normal n, the row in ascending column order, in fp64 on the
 *   widened inputs, one IEEE operation per operator in the written order:
 *     e = p_j - p;  en = (e.x n.x + e.y n.y) + e.z n.z;  u = (e.x - en * n.x, e.y - en * n.y, e.z - en * n.z);
 *     A_ab += u_a * u_b (a <= b);  b_a += u_a * (I_j - I_p);  m += 1.
 *   Then the tangent-plane constraint (Open3D's extra row m * n with right-hand side 0):  A_ab += (double)(m * m) * (n_a * n_b).
 *   A g = b by A = L L^T, column by column, and the two triangular solves, in sgam_points_icp_update's order and with its pivot
 *   rule (a pivot A_jj - sum_k<j L_jk^2 that is not finite or <= 1e-12 * A_jj fails).  NaN x 3 where p is not a point, n is not
 *   finite, m < 3 or the factorisation failed; otherwise g rounded to fp32 once.
 *
 * sgam_points_icp_accumulate_colored: sgam_points_icp_accumulate's chunks, fold and 32 slots (so sgam_points_icp_update is used
 *   unchanged) with source_colors [N][3], target_colors [Nr][3] uint8, target_gradient [Nr][3] and lambda_geometric in [0, 1].
 *   Entry i is a CORRESPONDENCE iff 0 <= index[i] < Nr and the normal and the gradient at index[i] are both finite.  With
 *   p = moved[i], q, n, d the target's point, normal and gradient at index[i], I_s = I(source_colors[i]), I_t = I(target_colors[index[i]]),
 *   e = (p.x - q.x, p.y - q.y, p.z - q.z), sg = sqrt(lambda_geometric), sp = sqrt(1 - lambda_geometric),
 *   en = (e.x n.x + e.y n.y) + e.z n.z:
 *     geometric row:    c = (p.y n.z - p.z n.y, p.z n.x - p.x n.z, p.x n.y - p.y n.x),
 *                       J_G = (sg * c.x, sg * c.y, sg * c.z, sg * n.x, sg * n.y, sg * n.z),  r_G = sg * en
 *     photometric row:  w = (e.x - en * n.x, e.y - en * n.y, e.z - en * n.z)  (the source point in the tangent plane, relative to q)
 *                       I_proj = ((d.x w.x + d.y w.y) + d.z w.z) + I_t;  dn = (d.x n.x + d.y n.y) + d.z n.z;
 *                       dM = (-d.x + dn * n.x, -d.y + dn * n.y, -d.z + dn * n.z);
 *                       c = (p.y dM.z - p.z dM.y, p.z dM.x - p.x dM.z, p.x dM.y - p.y dM.x),
 *                       J_I = (sp * c.x, sp * c.y, sp * c.z, sp * dM.x, sp * dM.y, sp * dM.z),  r_I = sp * (I_s - I_proj)
 *   Slot of (a, b) += J_G[a] * J_G[b], then += J_I[a] * J_I[b];  slot 21 + a += J_G[a] * r_G, then += J_I[a] * r_I;  slot 27 +=
 *   r_G * r_G, then += r_I * r_I;  slots 28..31 as in sgam_points_icp_accumulate.  lambda_geometric = 1 gives point-to-plane's sums
 *   bit for bit over the same correspondences.
 *
 * SGAM_EINVAL, nothing launched: NULL pointers (sgam_points_icp_accumulate's target_normals excepted), counts or blocks < 1,
 *   iteration < 0, a relative_fitness or relative_rmse that is negative or NaN, k outside 1..32, a lambda_geometric outside [0, 1]
 *   or NaN.
 * ------------------------------------------------------------------------------------------ */
int sgam_points_transform_f32(const float *points, int32_t N, const double *T, float *out, void *stream);
int64_t sgam_points_icp_partials(int64_t n);
int sgam_points_icp_accumulate(const float *moved, const float *target, const float *target_normals, const int32_t *index, const float *d2,
                               int32_t N, int32_t Nr, double *partials, void *stream);
int sgam_points_icp_update(const double *partials, int64_t blocks, int32_t iteration, double relative_fitness, double relative_rmse,
                           double *state, double *history, void *stream);
int sgam_points_color_gradient_f32(const float *points, const float *normals, const uint8_t *colors, int32_t N, const int32_t *knn_index,
                                   int32_t k, float *gradient_out, void *stream);
int sgam_points_icp_accumulate_colored(const float *moved, const uint8_t *source_colors, const float *target, const float *target_normals,
                                       const uint8_t *target_colors, const float *target_gradient, const int32_t *index, const float *d2,
                                       int32_t N, int32_t Nr, double lambda_geometric, double *partials, void *stream);

/* ------------------------------------------------------------------------------------------
 * Mesh clean-up (csrc/mesh_ops.hip, one entry point in csrc/point_cloud.hip): connected components, selection,
 * vertex / triangle incidence, vertex normals, Taubin smoothing steps and vertex clustering of an indexed triangle mesh: vertices
 * [nv][3] fp32, triangles [nt][3] int32.  Integer atomics only; every output is a function of the inputs only, equal run to run
 * and independent of the launch geometry; restated in tests/meshops_oracle.py.  The caller scans and compacts (integer plumbing)
 * between the calls.  flag: one DEVICE int32 the caller zeroed; a kernel ORs 1 into it when a loop ran into its bound (cannot
 * happen with intact inputs) and 2 when a triangle names a vertex outside [0, nv) (such a triangle is skipped, nothing is read
 * or written out of bounds).
 *
 * sgam_mesh_components_i32: two vertices are connected when a triangle uses both.  vertex_label_out [nv] = the least vertex index
 *   of the vertex's component (an unreferenced vertex: its own index), triangle_label_out [nt] = the label of corner 0,
 *   triangle_count_out [nv] = at a label, the number of triangles of its component, else 0.  Four launches: parent[i] = i; one
 *   lane per triangle unites its corners in a lock-free union-find (the larger root is linked under the smaller by atomicCAS, so
 *   parent[x] <= x always and a component's final root is its least index; parent words are read with relaxed agent-scope atomic
 *   loads; a find follows at most nv links, a unite retries at most nv times, the larger root strictly decreasing); one lane per
 *   vertex finds its root; one lane per triangle counts with an integer atomicAdd.  workspace:
 *   sgam_mesh_components_workspace_bytes(nv) = r16(4 nv) bytes (the parent array), 16-byte aligned.
 *
 * sgam_mesh_mark_vertices_i32: used_out [nv] = 1 where a triangle t with keep[t] != 0 (keep NULL: every triangle) names the
 *   vertex, else 0.  sgam_mesh_remap_triangles_i32: out [m][3] = vertex_map[triangles[triangle_index[j]][c]] for j < m
 *   (triangle_index [m] in [0, nt), vertex_map [nv]).
 *
 * sgam_mesh_incidence_count_i32 / sgam_mesh_incidence_fill_i32: kind 0 = for every vertex the triangles that use it (each once),
 *   kind 1 = for every vertex the other vertices it shares a triangle with.  count_out [nv] = the raw number of entries (kind 1:
 *   with repetitions).  The caller scans count_out into raw_offsets [nv + 1] (exclusive, raw_offsets[nv] = n_raw); fill writes
 *   every entry through a per-vertex atomic cursor (degree_out is the cursor), then one lane per vertex heap-sorts its segment
 *   ascending in place, keeps the first of equal entries and overwrites the others with -1, and writes degree_out [nv] = the
 *   number of entries kept.  The caller drops the -1 entries and scans degree_out into the final CSR offsets.
 *
 * sgam_mesh_vertex_normals_f32: offsets [nv + 1] / items [n_items]: the kind 0 CSR.  normals_out [nv][3] = the sum over the
 *   vertex's triangles in CSR order of (v1 - v0) x (v2 - v0), from the fp32 positions widened to fp64, differences of products,
 *   nothing fused, divided by sqrt((x * x + y * y) + z * z) in fp64 (a zero sum: the zero vector), rounded to fp32 once.
 * sgam_mesh_smooth_step_f32: offsets / items: the kind 1 CSR.  dst[i] = fp32(p + weight * (s / m - p)) per component in fp64, p =
 *   src[i], s = the sum of the m neighbours' positions in CSR order; m = 0: dst[i] = src[i].  src and dst do not overlap.
 *
 * sgam_points_voxel_assign_f32: sgam_points_voxel_sample_f32 (same arguments, workspace and outputs) which also writes rep_out [N]:
 *   the index of the kept point of point i's voxel, -1 for a point that is not a point.
 *
 * sgam_mesh_cluster_triangles_i32: cluster_of [nv]: a vertex's new index (-1: none).  Triangle t becomes (cluster_of[a],
 *   cluster_of[b], cluster_of[c]) in triangles_out [nt][3]; keep_out [nt] = 1 iff its three new indices are distinct (and none is
 *   -1) and no triangle with a lower index has the same triple after rotating the least index to the front (orientation kept).
 *   An insert-only open-addressing table of triangle ids over T = the least power of two >= max(2 nt, 256) slots: a slot is
 *   claimed by atomicCAS from empty; a lane that finds a slot holding a triangle of its own rotated triple does atomicMin(slot, t),
 *   otherwise probes on, at most T slots; a second launch keeps t iff its slot holds t.  workspace:
 *   sgam_mesh_dedup_workspace_bytes(nt) = 4 T + r16(4 nt) bytes, 16-byte aligned.
 *
 * SGAM_EINVAL, nothing launched: NULL pointers (keep, colours excepted), nv or nt < 1 (m, n_raw, n_items < 0), nt above 2^28, a
 *   kind that is not 0 or 1, a weight that is not finite, a voxel_size or origin that is not finite and positive / finite, a
 *   workspace that is missing, short or unaligned.
 * ------------------------------------------------------------------------------------------ */
int64_t sgam_mesh_components_workspace_bytes(int32_t nv);
int sgam_mesh_components_i32(const int32_t *triangles, int32_t nt, int32_t nv, void *workspace, int64_t workspace_bytes,
                             int32_t *vertex_label_out, int32_t *triangle_label_out, int32_t *triangle_count_out, int32_t *flag,
                             void *stream);
int sgam_mesh_mark_vertices_i32(const int32_t *triangles, int32_t nt, int32_t nv, const uint8_t *keep, int32_t *used_out, int32_t *flag,
                                void *stream);
int sgam_mesh_remap_triangles_i32(const int32_t *triangles, int32_t nt, const int32_t *triangle_index, int32_t m, const int32_t *vertex_map,
                                  int32_t nv, int32_t *triangles_out, int32_t *flag, void *stream);
int sgam_mesh_incidence_count_i32(const int32_t *triangles, int32_t nt, int32_t nv, int32_t kind, int32_t *count_out, int32_t *flag,
                                  void *stream);
int sgam_mesh_incidence_fill_i32(const int32_t *triangles, int32_t nt, int32_t nv, int32_t kind, const int32_t *raw_offsets, int64_t n_raw,
                                 int32_t *items_out, int32_t *degree_out, int32_t *flag, void *stream);
int sgam_mesh_vertex_normals_f32(const float *vertices, int32_t nv, const int32_t *triangles, int32_t nt, const int32_t *offsets,
                                 const int32_t *items, int64_t n_items, float *normals_out, void *stream);
int sgam_mesh_smooth_step_f32(const float *src, float *dst, int32_t nv, const int32_t *offsets, const int32_t *items, int64_t n_items,
                              double weight, void *stream);
int sgam_points_voxel_assign_f32(const float *points, int32_t N, float ox, float oy, float oz, float voxel_size, void *workspace,
                                 int64_t workspace_bytes, uint8_t *keep_out, int32_t *count_out, int32_t *rep_out, int32_t *overflow_flag,
                                 void *stream);
int64_t sgam_mesh_dedup_workspace_bytes(int32_t nt);
int sgam_mesh_cluster_triangles_i32(const int32_t *triangles, int32_t nt, const int32_t *cluster_of, int32_t nv, void *workspace,
                                    int64_t workspace_bytes, int32_t *triangles_out, uint8_t *keep_out, int32_t *flag, void *stream);

/* ------------------------------------------------------------------------------------------
 * Quadric-error decimation (csrc/mesh_simplify.hip): edge collapses in parallel rounds on the mesh and the two
 * incidence CSRs of the clean-up above (tri_*: kind 0, vert_*: kind 1, both ascending).  Garland-Heckbert / Open3D's
 * simplify_quadric_decimation as recalled, unpinned; the departures are marked.  Arithmetic: fp64 from the fp32 inputs widened,
 * every operator ONE IEEE operation in the written order, nothing fused; dot(u, v) = (u.x * v.x + u.y * v.y) + u.z * v.z; cross(u,
 * w) = (u.y * w.z - u.z * w.y, u.z * w.x - u.x * w.z, u.x * w.y - u.y * w.x); unit(m) = m / sqrt(dot(m, m)) per component, usable
 * when the length is positive and finite; a position is rounded to fp32 once.  No atomics but the flag word's; restated in
 * tests/decimation_oracle.py and compared bit for bit.  flag as above (1: a segment, an entry or an edge that does not belong to
 * the mesh; 2: a triangle names a vertex outside [0, nv)).  The caller rebuilds the CSRs, lists the edges, takes the k-th smallest
 * cost and compacts between the calls (integer plumbing).
 *
 * A quadric is 10 doubles, the upper triangle of a symmetric 4 x 4 matrix in the order xx xy xz xw yy yz yw zz zw ww.  Adding the
 * plane (p, d) with weight w adds (w * p_i) * p_j at (i, j), (p_3 = d).  "t names v": v is one of t's corners.
 *
 * 1. sgam_mesh_quadric_init_f64: quadrics_out [nv][10].  One lane per vertex v walks its kind 0 segment twice, ascending.  First
 *    every triangle (a, b, c) with n = unit(cross(b - a, c - a)) usable adds the plane (n, -dot(n, a)) with weight A = 0.5 *
 *    length.  Then every such triangle, for k = 0, 1, 2 with the edge from corner k to corner k + 1 (mod 3) when the two differ, v
 *    is one of them and exactly ONE triangle of v's segment names the other: u = unit(cross(p[k + 1] - p[k], n)) usable adds the
 *    plane (u, -dot(u, p[k])) with weight boundary_weight * A.  A triangle without area adds nothing.
 * 2. A round works on the current, compacted mesh.  edges [ne][2]: the kind 1 entries with item > owner, (lo, hi) = (owner, item),
 *    in CSR order — the id of an edge is its rank among them; edge_of_entry [n_vert_items]: that id at those entries (elsewhere
 *    unread).
 * 3. sgam_mesh_collapse_evaluate_f64, one lane per edge: Q = Q_lo + Q_hi entry by entry; mid = (lo + hi) * 0.5;
 *      c00 = Q4 Q7 - Q5 Q5, c01 = Q1 Q7 - Q5 Q2, c02 = Q1 Q5 - Q4 Q2, det = (Q0 c00 - Q1 c01) + Q2 c02, tr3 = ((Q0 + Q4) + Q7) / 3.
 *    DEPARTURE from Open3D: the singularity test is relative, |det| > 1e-8 * ((tr3 * tr3) * tr3), because an area-weighted quadric
 *    at voxel 0.01 has det ~ 1e-12.  When it holds, with r = (-Q3, -Q6, -Q8), s = (dx, dy, dz) / det by Cramer's rule:
 *      dx = (r0 c00 - Q1 (r1 Q7 - Q5 r2)) + Q2 (r1 Q5 - Q4 r2)
 *      dy = (Q0 (r1 Q7 - r2 Q5) - r0 c01) + Q2 (Q1 r2 - r1 Q2)
 *      dz = (Q0 (Q4 r2 - Q5 r1) - Q1 (Q1 r2 - Q2 r1)) + r0 c02
 *    and s is the target when dot(s - mid, s - mid) <= 4 * dot(hi - lo, hi - lo).  Otherwise the target is whichever of lo, hi,
 *    mid has the least clamped value, a tie going in that order.  value(p) = (sq + 2 * mixed) + (2 * lin + Q9), sq = (x (Q0 x) +
 *    y (Q4 y)) + z (Q7 z), mixed = (x (Q1 y) + x (Q2 z)) + y (Q5 z), lin = (Q3 x + Q6 y) + Q8 z; clamped: max(value, 0).  cost_out
 *    = fp32(clamped value at the target), position_out = fp32(target); color_out = fp32((1 - t) * c_lo + t * c_hi), t = dot(target
 *    - lo, hi - lo) / dot(hi - lo, hi - lo) clamped to [0, 1] (0 for ends that coincide).  removed_out = the triangles of lo's kind
 *    0 segment that name hi.
 * 4. Legality, same kernel; cost_out = +inf for an edge that is not legal.  Flip: every triangle of lo's segment that does not
 *    name hi, and every one of hi's that does not name lo, keeps dot(cross(b - a, c - a), the same with the end moved to
 *    position_out widened) > 0 — "> 0" also refuses a collapse onto zero area and any edge next to a triangle without area.
 *    Link (DEPARTURE: Open3D does not test it): the common items of lo's and hi's kind 1 segments are exactly as many as
 *    removed_out (> 0), and no triangle of lo's segment that does not name hi has, with hi in lo's place, the corner set of a
 *    triangle of hi's segment; and an edge with removed_out != 1 does not join two border vertices (a vertex is one when some item
 *    of its kind 1 segment shares exactly one triangle with it).  So a manifold, closed or with a border, stays one, no triangle
 *    is doubled and no vertex loses its last triangle but a lone triangle's (the count alone lets a tetrahedron fold flat and the
 *    corner of a sheet be cut off).
 *    A cost that is not finite in fp32 is not legal.
 * 5. The caller: need = ceil((nt - target) / 2); tau = the ceil(oversample * need)-th smallest legal cost (the largest when there
 *    are fewer), capped by the largest fp32 <= max_error.  Candidates: cost <= tau.
 * 6. sgam_mesh_collapse_select_i32, three launches: priority(e) = the bijection x ^= x >> 16; x *= 0x7feb352d; x ^= x >> 15; x *=
 *    0x846ca68b; x ^= x >> 16 of the edge id in uint32 — not the cost: a smooth cost field or the exact ties of a flat region
 *    have almost no local minima, and raw ids on a regular grid form one monotone wave.  One lane per vertex: p1[v] = the least
 *    priority over its candidate edges (0xffffffff without one; the id of an entry whose item is below its owner is found by
 *    bisection of the item's own segment); one lane per vertex: p2[v] = min(p1[v], p1 of its kind 1 items); one lane per edge:
 *    selected iff candidate and priority = p2[lo] = p2[hi].  No vertex of a selected edge is a neighbour of (or is) a vertex of
 *    another, so no triangle is touched by two collapses and step 4's tests hold under simultaneous application.  key_out [ne]
 *    int64 = (cost bits << 32) | priority, -1 when not selected.  workspace: sgam_mesh_collapse_workspace_bytes(nv) = 2 r16(4 nv)
 *    bytes (p1, p2), 16-byte aligned.
 * 7. The caller: when applying every selected edge would take nt below target, the edges in ascending key are applied while the
 *    running count (nt minus the removed_out of those before) is > target.
 * 8. sgam_mesh_collapse_apply_f64, one lane per entry of chosen [m] (edge ids, an independent set): IN PLACE vertices[lo] =
 *    position[e], colors[lo] = color[e], quadrics[lo] += quadrics[hi]; merge[hi] = lo, vertex_keep[hi] = 0, triangle_keep[t] = 0
 *    for the triangles of lo's segment that name hi (the caller filled merge with 0 .. nv - 1 and the keeps with 1).  The caller
 *    compacts: vertices, colours and quadrics at the kept vertices, sgam_mesh_remap_triangles_i32 over the kept triangles with
 *    vertex_map = (the rank of merge[v] among the kept vertices); both orders are kept.
 *
 * SGAM_EINVAL, nothing launched: NULL pointers (colours excepted; colors and color_out / color are given together), nv, nt, ne, m
 *   or an item count < 1, nt above 2^28, n_tri_items > 3 nt, n_vert_items > 6 nt, 2 ne > n_vert_items, m > ne, a boundary_weight
 *   that is negative or not finite, a tau that is negative or not finite, a workspace that is missing, short or unaligned.
 * ------------------------------------------------------------------------------------------ */
int sgam_mesh_quadric_init_f64(const float *vertices, int32_t nv, const int32_t *triangles, int32_t nt, const int32_t *tri_offsets,
                               const int32_t *tri_items, int64_t n_tri_items, double boundary_weight, double *quadrics_out, int32_t *flag,
                               void *stream);
int sgam_mesh_collapse_evaluate_f64(const float *vertices, const float *colors, int32_t nv, const int32_t *triangles, int32_t nt,
                                    const double *quadrics, const int32_t *tri_offsets, const int32_t *tri_items, int64_t n_tri_items,
                                    const int32_t *vert_offsets, const int32_t *vert_items, int64_t n_vert_items, const int32_t *edges,
                                    int32_t ne, float *cost_out, int32_t *removed_out, float *position_out, float *color_out, int32_t *flag,
                                    void *stream);
int64_t sgam_mesh_collapse_workspace_bytes(int32_t nv);
int sgam_mesh_collapse_select_i32(int32_t nv, const int32_t *vert_offsets, const int32_t *vert_items, int64_t n_vert_items,
                                  const int32_t *edge_of_entry, const int32_t *edges, const float *cost, int32_t ne, float tau, void *workspace,
                                  int64_t workspace_bytes, int64_t *key_out, int32_t *flag, void *stream);
int sgam_mesh_collapse_apply_f64(float *vertices, float *colors, double *quadrics, int32_t nv, const int32_t *triangles, int32_t nt,
                                 const int32_t *tri_offsets, const int32_t *tri_items, int64_t n_tri_items, const int32_t *edges,
                                 const float *position, const float *color, int32_t ne, const int32_t *chosen, int32_t m, int32_t *merge,
                                 int32_t *vertex_keep, int32_t *triangle_keep, int32_t *flag, void *stream);

/* ------------------------------------------------------------------------------------------
 * Queries against a triangle mesh (csrc/mesh_query.hip): the exact distance from points to the mesh's surface and
 * points drawn uniformly by area.  vertices [nv][3] fp32, triangles [nt][3] int32, flag as in the mesh clean-up above (2: a
 * triangle names a vertex outside [0, nv); it is skipped).  Arithmetic: every fp32 operator is ONE IEEE operation in the written
 * order, nothing fused; dot(u, v) = (u.x * v.x + u.y * v.y) + u.z * v.z; restated in tests/meshquery_oracle.py and compared bit
 * for bit.
 *
 * Candidates: a triangle (a, b, c) whose nine coordinates are finite and whose normal n = ab x ac (each component a * b - c * d:
 *   two products, one difference) has dot(n, n) > 0.  Anything else is "not a triangle" and never wins.
 * Closest point of a candidate to q (Ericson, Real-Time Collision Detection §5.1.5), ap = q - a, bp = q - b, cp = q - c:
 *     p1 = dot(ab, ap)  p2 = dot(ac, ap)  p3 = dot(ab, bp)  p4 = dot(ac, bp)  p5 = dot(ab, cp)  p6 = dot(ac, cp)
 *     vc = p1 * p4 - p3 * p2    vb = p5 * p2 - p1 * p6    va = p3 * p6 - p5 * p4    e43 = p4 - p3    e56 = p5 - p6
 *   region = the first test that holds, in this order (0 1 2: vertices a b c; 3 4 5: edges ab bc ca; 6: the face):
 *     0: p1 <= 0 && p2 <= 0      1: p3 >= 0 && p4 <= p3      3: vc <= 0 && p1 >= 0 && p3 <= 0      2: p6 >= 0 && p5 <= p6
 *     5: vb <= 0 && p2 >= 0 && p6 <= 0      4: va <= 0 && e43 >= 0 && e56 >= 0      6: otherwise
 *   per coordinate x = (base + e1 * (n1 / m1)) + ac * (n2 / m2), with
 *     0, 1, 2: base a, b, c; e1 = ab; 0 / 1; 0 / 1          3: a; ab; p1 / (p1 - p3); 0 / 1          5: a; ac; p2 / (p2 - p6); 0 / 1
 *     4: b; c - b; e43 / (e43 + e56); 0 / 1                 6: a; ab; vb / ((va + vb) + vc); vc / ((va + vb) + vc)
 *   d2 = (dx * dx + dy * dy) + dz * dz of x - q (the point clouds' d2).
 * Winner of a query: the candidate of least (d2 bits, triangle index) among those with d2 <= max_d2 (+inf: all); NaN and +inf
 *   never win; no winner, or a query with a coordinate that is not finite: triangle -1, d2 +inf, closest NaN.
 *   d2_out [Nq] fp32, triangle_out [Nq] int32, closest_out [Nq][3] fp32 or NULL (not written).
 *
 * sgam_mesh_distance_brute_f32: one lane per query, the triangles gathered once per tile of 256 into LDS and walked in index order.
 * The triangle grid: cells of edge cell_size, origin (ox, oy, oz), gx x gy x gz cells, cell = clamp(floorf((p - origin) /
 *   cell_size), 0, g - 1) per axis (the point grid's rule); a candidate is entered into every cell of the block [cell(min),
 *   cell(max)] per axis of its bounding box.
 *   sgam_mesh_grid_count: totals_out (DEVICE int64[2]) = {entries of all candidates, number of candidates}: what the caller
 *     sizes the workspace by (and judges the cell size by) after one synchronisation.
 *   sgam_mesh_grid_workspace_bytes(n_entries, gx, gy, gz) = 48 n_entries + r16(4 (cells + 1)) + r16(4 cells) + r16(4 ceil(cells /
 *     1024)) bytes, 16-byte aligned, caller-owned; n_entries in 1 .. 2^31 - 1, cells <= 2^24.
 *   sgam_mesh_grid_build: count per cell (integer atomics) -> exclusive scan -> scatter of the records (nine coordinates and the
 *     id, 48 B) into the workspace; n_entries is sgam_mesh_grid_count's total for the same mesh and grid (a record that would fall
 *     beyond it is not written: flag bit 1).
 *   sgam_mesh_distance_grid_f32: one wavefront per query walks the cells in growing shells (the point grid's walk, the 64 lanes
 *     sharing each row's records and folding their winners by the (d2 bits, index) key at the end) and stops after
 *     shell r when ms = (m - margin) * (1 - 2^-14) > 0 and (best < ms * ms or ms * ms > max_d2), m = the least signed distance from
 *     q to the faces of the visited block that are not grid borders, margin = 2^-14 * (largest |coordinate| of the grid's corners
 *     + its longest edge).  Same bits as brute force for every cell size.
 *
 * sgam_mesh_triangle_area2_f32: area2_out [nt] = sqrt(dot(n, n)), twice the area; 0 for what is not a triangle.
 * sgam_mesh_sample_f32: cdf [nt] int64 on the device: the inclusive sums of the caller's integer weights, W = cdf[nt - 1] > 0.
 *   Sample i < n: w0..w3 = Philox4x32-10(counter (i lo32, i hi32, 0, 0), key (seed lo32, seed hi32)); target = mulhi64((w0 << 32)
 *   | w1, W); triangle_out [n] = the first t with cdf[t] > target; r1 = (w2 >> 8) * 2^-24, r2 = (w3 >> 8) * 2^-24; s = sqrt(r1),
 *   wa = 1 - s, wb = s * (1 - r2), wc = s * r2; points_out [n][3] = (wa * A + wb * B) + wc * C per coordinate; colors_out [n][3] (or
 *   NULL) the same of vertex_colors [nv][3]; normals_out [n][3] (or NULL) = n / sqrt(dot(n, n)) per component.  A pure function of
 *   (mesh, cdf, seed, i).
 *
 * SGAM_EINVAL, nothing launched: NULL pointers (closest_out, vertex_colors, colors_out, normals_out excepted; colors_out without
 *   vertex_colors), nv, nt, Nq or n < 1, nt above 2^28, n above 2^31 - 1, a max_d2 that is negative or NaN, a grid the point
 *   grid would refuse, a workspace that is missing, short or unaligned.
 * ------------------------------------------------------------------------------------------ */
int sgam_mesh_distance_brute_f32(const float *vertices, int32_t nv, const int32_t *triangles, int32_t nt, const float *query, int32_t Nq,
                                 float max_d2, float *d2_out, int32_t *triangle_out, float *closest_out, int32_t *flag, void *stream);
int64_t sgam_mesh_grid_workspace_bytes(int64_t n_entries, int32_t gx, int32_t gy, int32_t gz);
int sgam_mesh_grid_count(const float *vertices, int32_t nv, const int32_t *triangles, int32_t nt, float ox, float oy, float oz,
                         float cell_size, int32_t gx, int32_t gy, int32_t gz, int64_t *totals_out, int32_t *flag, void *stream);
int sgam_mesh_grid_build(const float *vertices, int32_t nv, const int32_t *triangles, int32_t nt, float ox, float oy, float oz,
                         float cell_size, int32_t gx, int32_t gy, int32_t gz, int64_t n_entries, void *workspace, int64_t workspace_bytes,
                         int32_t *flag, void *stream);
int sgam_mesh_distance_grid_f32(const float *query, int32_t Nq, int64_t n_entries, float ox, float oy, float oz, float cell_size,
                                int32_t gx, int32_t gy, int32_t gz, const void *workspace, int64_t workspace_bytes, float max_d2,
                                float *d2_out, int32_t *triangle_out, float *closest_out, void *stream);
int sgam_mesh_triangle_area2_f32(const float *vertices, int32_t nv, const int32_t *triangles, int32_t nt, float *area2_out, int32_t *flag,
                                 void *stream);
int sgam_mesh_sample_f32(const float *vertices, const float *vertex_colors, int32_t nv, const int32_t *triangles, int32_t nt,
                         const int64_t *cdf, uint64_t seed, int64_t n, float *points_out, int32_t *triangle_out, float *colors_out,
                         float *normals_out, int32_t *flag, void *stream);

/* ------------------------------------------------------------------------------------------
 * Rays against a triangle mesh (csrc/mesh_ray.hip): the nearest hit, the any-hit (occlusion) query, the visibility
 * of points from pinhole cameras, and the rays of pinhole images.  Mesh, candidates, flag and arithmetic as in "Queries against a
 * triangle mesh" above; restated in tests/raycast_oracle.py and compared bit for bit.  The ABI version is unchanged: additions only.
 *
 * rays [n_rays][6] fp32 = (o, d); d is not normalised (t is in units of |d|).  A ray with a component that is not finite or with
 *   d = 0 is "not a ray": the no-hit answer.
 * Intersection of a candidate (a, b, c) — Moeller-Trumbore, two-sided, no culling; a cross product's component is a * b - c * d:
 *     e1 = b - a    e2 = c - a    p = d x e2    det = dot(e1, p)    s = o - a
 *     u = dot(s, p) / det    q = s x e1    v = dot(d, q) / det    t = dot(e2, q) / det + 0.0f
 *     P = o + t * d    lo = min(min(a, b), c) - guard    hi = max(max(a, b), c) + guard      (per coordinate)
 *   a hit iff det != 0, u >= 0, v >= 0, u + v <= 1, tnear <= t <= tfar and lo <= P <= hi on every axis; NaN never hits.  Not
 *   watertight along shared edges.  guard: an absolute length >= 0, part of the rule (sgam_neurips22_amd.meshops passes 2^-15 of the
 *   largest |coordinate| of the candidates' vertices); it is what makes the grid walk exact, and it may discard hits of rays whose
 *   origin lies further than some 2^8 coordinate scales from the mesh.
 * mode 0, nearest: the hit of least (t bits, triangle index).  t_out [n] fp32 (+inf without a hit), triangle_out [n] int32 (-1),
 *   uv_out [n][2] fp32 or NULL (NaN), normal_out [n][3] fp32 or NULL: n / sqrt(dot(n, n)) per component, n = e1 x e2, not turned
 *   towards the ray (NaN).  hit_out is not written.
 * mode 1, any: hit_out [n] uint8 = 1 iff some candidate hits; the other outputs are not written.
 *
 * sgam_mesh_raycast_brute_f32: one lane per ray, the triangles through LDS in tiles of 256, in index order.
 * sgam_mesh_raycast_grid_f32: one lane per ray walks the tables sgam_mesh_grid_build wrote (same grid arguments, n_entries and
 *   workspace) in steps [ta, tb] that cover the window without a gap; a step visits the cells [cell(min(P(ta), P(tb)) - margin),
 *   cell(max(P(ta), P(tb)) + margin)] per axis (margin: sgam_mesh_distance_grid_f32's) and offers all their records; it stops
 *   when best <= tb, at tfar, or once the ray has left the grid's box by 2 margin.  Requires 2 guard <= margin and a grid whose box
 *   holds the candidates' vertices; then the same bits as brute force for every ray and cell size (csrc/mesh_ray.hip has the
 *   argument).  flag bit 1: a walk ran into its bound (never, by the count of layers).
 *
 * Visibility: points [N][3], poses_w2c [P][4][4] row-major world -> camera (R = the upper 3 x 3, T = the last column), intrinsics fx,
 *   fy, cx, cy of an H x W image.  Per point x and pose: X = ((M[r][0] * x + M[r][1] * y) + M[r][2] * z) + M[r][3] per row;
 *   c_k = -((R[0][k] * T[0] + R[1][k] * T[1]) + R[2][k] * T[2]); in the frustum iff z_near <= X.z <= z_far and uf = floorf(((fx *
 *   X.x) / X.z + cx) + 0.5f), vf alike with fy, X.y, cy, satisfy 0 <= uf < W, 0 <= vf < H (float compares); unoccluded iff the ray
 *   o = c, d = x - c has no hit in [0, 1 - tolerance].  count_out [N] int32 = the poses that see the point.
 *   sgam_mesh_visibility_grid_f32 walks the grid, sgam_mesh_visibility_brute_f32 (parity, small meshes) every triangle.
 * sgam_rays_pinhole_f32: rays_out [P][H][W][6]: o = c; dc = ((j - cx) / fx, (i - cy) / fy, 1) for row i, column j;
 *   d_k = (R[0][k] * dc.x + R[1][k] * dc.y) + R[2][k] — camera z = 1, so t is the view-space depth.
 *
 * SGAM_EINVAL, nothing launched: NULL pointers (uv_out, normal_out and the outputs of the other mode excepted), counts < 1, nt above
 *   2^28, mode not 0 / 1, tnear negative or not finite, tfar < tnear or NaN, guard negative or not finite, 2 guard > margin, tolerance
 *   outside [0, 1], fx or fy zero, intrinsics that are not finite, z_near <= 0, z_far < z_near, P * H * W above 2^31 - 1, a grid or
 *   workspace sgam_mesh_distance_grid_f32 would refuse.
 * ------------------------------------------------------------------------------------------ */
int sgam_mesh_raycast_brute_f32(const float *vertices, int32_t nv, const int32_t *triangles, int32_t nt, const float *rays, int32_t n_rays,
                                int32_t mode, float tnear, float tfar, float guard, float *t_out, int32_t *triangle_out, float *uv_out,
                                float *normal_out, uint8_t *hit_out, int32_t *flag, void *stream);
int sgam_mesh_raycast_grid_f32(const float *rays, int32_t n_rays, int64_t n_entries, float ox, float oy, float oz, float cell_size,
                               int32_t gx, int32_t gy, int32_t gz, const void *workspace, int64_t workspace_bytes, int32_t mode, float tnear,
                               float tfar, float guard, float *t_out, int32_t *triangle_out, float *uv_out, float *normal_out,
                               uint8_t *hit_out, int32_t *flag, void *stream);
int sgam_mesh_visibility_grid_f32(const float *points, int32_t N, const float *poses_w2c, int32_t P, float fx, float fy, float cx, float cy,
                                  int32_t H, int32_t W, float z_near, float z_far, float tolerance, float guard, int64_t n_entries, float ox,
                                  float oy, float oz, float cell_size, int32_t gx, int32_t gy, int32_t gz, const void *workspace,
                                  int64_t workspace_bytes, int32_t *count_out, int32_t *flag, void *stream);
int sgam_mesh_visibility_brute_f32(const float *vertices, int32_t nv, const int32_t *triangles, int32_t nt, const float *points, int32_t N,
                                   const float *poses_w2c, int32_t P, float fx, float fy, float cx, float cy, int32_t H, int32_t W,
                                   float z_near, float z_far, float tolerance, float guard, int32_t *count_out, int32_t *flag, void *stream);
int sgam_rays_pinhole_f32(const float *poses_w2c, int32_t P, float fx, float fy, float cx, float cy, int32_t H, int32_t W, float *rays_out,
                          void *stream);

/* ------------------------------------------------------------------------------------------
 * A bounding-volume hierarchy over a mesh's candidate triangles (csrc/mesh_bvh.hip): the accelerator whose cost
 * does not depend on the triangles being near one scale.  It serves the three queries above — distance, rays, visibility — with
 * the same per-triangle arithmetic, the same sinks and therefore the same bits as brute force; restated in tests/bvh_oracle.py.
 * The ABI version is unchanged: additions only.
 *
 * sgam_mesh_bvh_keys: keys_out [nt] int64 (DEVICE): per candidate the 33-bit Morton code (11 bits per axis: q = min(floor(((0.5 min
 *   + 0.5 max) - lo) / (hi - lo) * 2048), 2047) of its bounding box's centre inside the caller's box [lo, hi] — the box of the
 *   candidates' corners) shifted left by 28, the triangle's index below it; INT64_MAX for what is not a candidate.  count_out
 *   (DEVICE int64[1]) = the candidates.  The caller sorts keys_out ascending (integer plumbing); the first count keys are the leaves.
 * sgam_mesh_bvh_workspace_bytes(n) = 48 n + r16(24 (2 n - 1)) + r16(8 max(n - 1, 1)) + r16(4 max(n - 1, 1)) bytes, 16-byte aligned,
 *   caller-owned: records [n] (nine coordinates and the id, 48 B, in key order), boxes [2 n - 1][6] fp32 (lo, hi), children
 *   [n - 1][2] int32, ready [n - 1] int32 (a node's height); n in 1 .. 2^28.  Nodes: internal i is i (0 the root), leaf k is n - 1 + k.
 * sgam_mesh_bvh_build: sorted_keys [>= n_candidates] int64, ascending and unique (sgam_mesh_bvh_keys' output, sorted) -> the tables:
 *   leaves, Karras's hierarchy (every internal node from the keys alone), then the boxes in min(61, n - 1) launches, one per round
 *   (a node computes once both children were ready before the launch; no fence, nothing handed between workgroups).  A node's box
 *   is exactly min / max of its leaves' corners.  flag bit 1: a key that is not one of this mesh's candidates, or a loop's bound.
 * sgam_mesh_distance_bvh_f32: one lane per query walks the tree, the nearer child first, and skips a node iff ms = (m - margin) *
 *   (1 - 2^-14) > 0 and (best < ms * ms or ms * ms > max_d2), m the fp32 distance from q to the node's box, margin = 2^-14 * (largest
 *   |coordinate| of [lo, hi] + its longest edge), [lo, hi] the box passed to sgam_mesh_bvh_keys.  Outputs as sgam_mesh_distance_grid_f32.
 * sgam_mesh_raycast_bvh_f32: one lane per ray; a node is visited unless its box, inflated by guard and by the rounding of P (2^-21
 *   (|o| + largest |coordinate|) + 2^-100 per axis), is missed by every t of [tnear, min(tfar, best)] in a slab test whose two
 *   parameters per axis are pushed apart by 2^-21 |s| + 2^-100 (csrc/mesh_bvh.hip has the proof).  Modes and outputs as
 *   sgam_mesh_raycast_grid_f32; no condition ties guard to the tree.
 * sgam_mesh_visibility_bvh_f32: sgam_mesh_visibility_grid_f32 through the tree; the N x P rays are formed in registers.
 * flag bit 1 from a query: the walk ran into a bound (a workspace that does not hold this tree); reads stay inside the workspace.
 *
 * SGAM_EINVAL, nothing launched: what the grid forms refuse, n_candidates outside 1 .. 2^28 (or above nt), a box that is not finite
 *   or has hi < lo, a workspace that is missing, short or unaligned.
 * ------------------------------------------------------------------------------------------ */
int64_t sgam_mesh_bvh_workspace_bytes(int64_t n_candidates);
int sgam_mesh_bvh_keys(const float *vertices, int32_t nv, const int32_t *triangles, int32_t nt, float lox, float loy, float loz, float hix,
                       float hiy, float hiz, int64_t *keys_out, int64_t *count_out, int32_t *flag, void *stream);
int sgam_mesh_bvh_build(const float *vertices, int32_t nv, const int32_t *triangles, int32_t nt, const int64_t *sorted_keys,
                        int64_t n_candidates, void *workspace, int64_t workspace_bytes, int32_t *flag, void *stream);
int sgam_mesh_distance_bvh_f32(const float *query, int32_t Nq, int64_t n_candidates, float lox, float loy, float loz, float hix, float hiy,
                               float hiz, const void *workspace, int64_t workspace_bytes, float max_d2, float *d2_out, int32_t *triangle_out,
                               float *closest_out, int32_t *flag, void *stream);
int sgam_mesh_raycast_bvh_f32(const float *rays, int32_t n_rays, int64_t n_candidates, const void *workspace, int64_t workspace_bytes,
                              int32_t mode, float tnear, float tfar, float guard, float *t_out, int32_t *triangle_out, float *uv_out,
                              float *normal_out, uint8_t *hit_out, int32_t *flag, void *stream);
int sgam_mesh_visibility_bvh_f32(const float *points, int32_t N, const float *poses_w2c, int32_t P, float fx, float fy, float cx, float cy,
                                 int32_t H, int32_t W, float z_near, float z_far, float tolerance, float guard, int64_t n_candidates,
                                 const void *workspace, int64_t workspace_bytes, int32_t *count_out, int32_t *flag, void *stream);

/* ------------------------------------------------------------------------------------------
 * FID evaluation (csrc/inception.hip, csrc/conv_gemm.hip; sgam_neurips22_amd/fid.py): the kernels of the reference's
 * modules/misc/pytorch_fid next to the fp32-in MFMA convolution.  NHWC fp32, caller-owned buffers, no sync, no float atomics.
 *
 * sgam_conv2d_relu_nhwc_f32: the convolution of sgam_conv2d_nhwc_f32 (same descriptor, planner and workspace query) with
 *   out = max(0, acc + bias[n]) and no residual: conv + folded BatchNorm + ReLU.  `out` may point at a column offset inside a
 *   wider row (ldc = channels of a concatenated block output, n_valid = channels of this branch).
 * sgam_inception_preprocess_f32: in (B,H,W,3), uint8 (in_is_u8: v / 255 in fp32, ToTensor) or fp32 in [0,1] -> out (B,Ho,Wo,4):
 *   bilinear, align_corners = False, no antialiasing, PyTorch's index rule (scale = (float)in / out, src = max((dst + 0.5) *
 *   scale - 0.5, 0), i1 = i0 + (i0 < in - 1)); then 2 x - 1 with `normalize`; channel 3 = 0.  Ho = H, Wo = W: an exact copy.
 * sgam_pool3x3_nhwc_f32: mode 0 max / stride 2 / no padding (H, W >= 3; Ho = (H - 3) / 2 + 1), 1 max / stride 1 / padding 1,
 *   2 average / stride 1 / padding 1 over the valid taps only (count_include_pad = False; summed in (ky, kx) order in fp32, divided
 *   by their count).  Max is exact.  ldx / ldo >= C: channel pitches, so either side may be a slice of a concatenated map.
 *   sgam_pool3x3_out_size: the output size of a mode (SGAM_EINVAL for a map mode 0 does not fit).
 * sgam_global_avgpool_nhwc_f32: (B,HW,C) pitch ldx -> (B,C) dense; fp64 accumulation in a fixed order, one rounding to fp32.
 * sgam_activation_stats_*: streaming statistics of (n, d) fp32 feature batches (pitch ldx) in a caller-owned fp64 `state` of
 *   sgam_activation_stats_state_doubles(d) = 1 + 2 d + d^2 doubles: [0] count, then sum[d] of (x - shift), shift[d] (the column
 *   mean of the FIRST batch, fixed from then on) and the d x d Gram of (x - shift), kept in the 64 x 64 tiles on and above the tile
 *   diagonal.  `first` != 0 starts a new accumulation (the state need not be cleared).  Rows are added in order with fp64 fma: the
 *   result depends on the batch boundaries only through `shift`.  finalize: mu[d] = shift + sum / N, sigma[d][d] = (gram - sum
 *   sum^T / N) / (N - 1) (np.cov), sigma[i][j] == sigma[j][i] bit for bit; N = 1 gives a non-finite sigma, as np.cov does.
 * ------------------------------------------------------------------------------------------ */
int sgam_conv2d_relu_nhwc_f32(const sgam_conv_desc *d, const float *x, const float *w_packed, const float *bias, float *out,
                              void *workspace, int64_t workspace_bytes, void *stream);
int sgam_inception_preprocess_f32(const void *in, int32_t in_is_u8, int32_t B, int32_t H, int32_t W, float *out, int32_t Ho, int32_t Wo,
                                  int32_t normalize, void *stream);
int sgam_pool3x3_out_size(int32_t H, int32_t W, int32_t mode, int32_t *Ho, int32_t *Wo);
int sgam_pool3x3_nhwc_f32(const float *x, int32_t B, int32_t H, int32_t W, int32_t C, int32_t ldx, float *out, int32_t ldo, int32_t mode,
                          void *stream);
int sgam_global_avgpool_nhwc_f32(const float *x, int32_t B, int32_t HW, int32_t C, int32_t ldx, float *out, void *stream);
int64_t sgam_activation_stats_state_doubles(int32_t d);
int sgam_activation_stats_update_f64(const float *x, int32_t n, int32_t d, int32_t ldx, double *state, int32_t first, void *stream);
int sgam_activation_stats_finalize_f64(const double *state, int32_t d, double *mu, double *sigma, void *stream);

/* ------------------------------------------------------------------------------------------
 * Set metrics on features (csrc/feature_metrics.hip; sgam_neurips22_amd/feature_metrics.py): KID and precision / recall /
 * density / coverage, all read off one fp64 Gram matrix.  Caller-owned buffers, no sync, no float atomics; every entry point
 * refuses NULL pointers and bad shapes with SGAM_EINVAL before any launch.  At most 16384 rows (a 2 GiB Gram).
 *
 * sgam_feature_gram_f64: z (n, d) fp32 rows of pitch ldz >= d, d % 4 == 0, 1 <= n <= 16384 -> G (n, n) fp64 dense,
 *   G_ij = sum_k (double) z_ik * (double) z_jk (products of fp32 values are exact in fp64).  v_mfma_f64_16x16x4_f64 on 64 x 64
 *   tiles; K runs k = 0, 4, 8, ... in the same order for every tile, no split-K, no atomics: run-to-run identical; only tiles
 *   with bi <= bj are computed and every entry is stored at (i, j) and (j, i): G == G^T bit for bit; an entry is a function of
 *   the values of its two rows only (equal rows give equal entries).  Rows beyond n are masked, not read.
 * sgam_kid_subsets_u32: subset s (0 .. subsets - 1) of side 0 / 1 with N = n1 / n2 rows holds the m indices i with the smallest
 *   pairs (key, i), key = word 0 of Philox4x32-10 at counter (i, s, side, 0) under key (seed & 0xffffffff, seed >> 32); an equal
 *   key goes to the lower index; m == N is every index.  idx (subsets, 2, m) int32, each list ascending.  workspace: at least
 *   2 * subsets * max(n1, n2) bytes (SGAM_EWORKSPACE otherwise).  1 <= m <= min(n1, n2), n1, n2 <= 16384, subsets <= 65535.
 * sgam_kid_mmd_f64: G is the Gram of the n1 rows of the first set followed by the n2 rows of the second (n1 + n2 <= 16384); with
 *   the lists a = idx[s][0], b = idx[s][1] (b offset by n1 into G) and K_ij = t t t, t = gamma G_ij + coef0, in fp64:
 *   out[s] = sum_{i != j} K(a_i, a_j) / (m (m - 1)) + sum_{i != j} K(b_i, b_j) / (m (m - 1)) - 2 sum_{i, j} K(a_i, b_j) / m^2.
 *   fp64 sums in a fixed order: per row (64 interleaved column chains, joined in a fixed order), the rows joined in row order.
 *   m >= 2.  workspace: at least 24 * subsets * m bytes, 8-byte aligned.  The indices are trusted to be in range.
 * sgam_feature_prdc_f64: G is the Gram of nr reference rows followed by nf scene rows (nr + nf <= 16384), 1 <= k <= 32,
 *   k + 1 <= min(nr, nf).  d2(i, j) = (G_ii + G_jj) - 2 G_ij, evaluated in exactly this order in fp64.  radius2 (nr + nf) fp64
 *   out: the k-th smallest d2(i, j) over the rows j != i of i's own set (exclusion by index: a duplicate row is a neighbour at
 *   distance 0).  counts (4) int64 out, integer atomics: [0] scene rows j with d2(i, j) <= radius2[i] for some reference i
 *   (precision * nf), [1] reference rows i with d2(i, j) <= radius2[j] for some scene j (recall * nr), [2] pairs (i, j) with
 *   d2(i, j) <= radius2[i] (density * k * nf), [3] reference rows i with min_j d2(i, j) <= radius2[i] (coverage * nr).
 * ------------------------------------------------------------------------------------------ */
int sgam_feature_gram_f64(const float *z, int32_t n, int32_t d, int32_t ldz, double *G, void *stream);
int sgam_kid_subsets_u32(int32_t n1, int32_t n2, int32_t m, int32_t subsets, uint64_t seed, void *workspace, int64_t workspace_bytes,
                         int32_t *idx, void *stream);
int sgam_kid_mmd_f64(const double *G, int32_t n1, int32_t n2, const int32_t *idx, int32_t m, int32_t subsets, double gamma, double coef0,
                     void *workspace, int64_t workspace_bytes, double *out, void *stream);
int sgam_feature_prdc_f64(const double *G, int32_t nr, int32_t nf, int32_t k, double *radius2, int64_t *counts, void *stream);

/* ------------------------------------------------------------------------------------------
 * Global registration (csrc/point_global.hip; geometry.fpfh / match_features / register_ransac / register_global; DESIGN
 * §4.4.6): FPFH features, the nearest feature, and RANSAC over feature correspondences — the pose ICP starts from when the two
 * clouds share no frame.  Open3D's compute_fpfh_feature and registration_ransac_based_on_feature_matching as documented,
 * unpinned against Open3D; tests/global_registration_oracle.py restates every expression.  -ffp-contract=off, one IEEE
 * operation per operator in the written order, integer atomics only, every output a function of the inputs only.  Every entry
 * point refuses NULL pointers and sizes out of range with SGAM_EINVAL before any launch.
 *
 * sgam_points_fpfh_counts: points, normals [N][3] fp32, knn_index [N][k] (row i of the k-NN search of the cloud in itself, the
 *   point itself among its neighbours; 1 <= k <= 32) -> counts [N][34] int32: 33 histogram counts and, in [33], the number m of
 *   pairs counted.  A point that is not a point or whose normal is not finite counts nothing (m = 0).  Per column c in ascending
 *   order with j = knn_index[i][c], skipped when j < 0, j >= N, j == i or normal j is not finite; in fp64 on the widened inputs:
 *     dp = p_j - p_i;  d = sqrt((dp.x dp.x + dp.y dp.y) + dp.z dp.z), skipped when d == 0;
 *     a1 = ((n_i.x dp.x + n_i.y dp.y) + n_i.z dp.z) / d,  a2 alike with n_j;
 *     |a1| < |a2|:  (n1, n2, dp) = (n_j, n_i, -dp), f2 = -a2;  otherwise (n1, n2) = (n_i, n_j), f2 = a1;
 *     v = dp x n1 = (dp.y n1.z - dp.z n1.y, dp.z n1.x - dp.x n1.z, dp.x n1.y - dp.y n1.x);  |v| by the expression of d, skipped
 *     when 0;  v = v / |v| per component;  w = n1 x v (the same three expressions);  f1 = (v.x n2.x + v.y n2.y) + v.z n2.z;
 *     x = n1 . n2, y = w . n2 (theta = atan2(y, x), never evaluated).
 *   Bins, 11 per feature: [0..10] theta, [11..21] f1, [22..32] f2 (Open3D's order).  f: (int)floor((11.0 * (f + 1.0)) * 0.5)
 *   clamped to 0..10.  theta: with the edge directions (c_b, s_b) = (cos, sin)(-pi + 2 pi b / 11), b = 1..10, the fp64 literals
 *   of point_global.hip, and cross_b = c_b * y - s_b * x:  x == 0 and y == 0: 5;  y < 0: the number of b in 1..5 with
 *   cross_b >= 0;  otherwise 5 + the number of b in 6..10 with cross_b >= 0.
 * sgam_points_fpfh_combine_f32: counts, knn_index and knn_d2 [N][k] (the search's fp32 squared distances) -> features [N][33];
 *   points and normals only say which rows are NaN.
 *   SPFH_b(i) = (double)count_b * (100.0 / (double)m_i), 0 where m_i == 0.  Per block of 11 bins, over the columns c >= 1 in
 *   ascending order with j = knn_index[i][c] in [0, N), knn_d2[i][c] > 0 (and finite) and m_j > 0:
 *   A_b += SPFH_b(j) / (double)knn_d2[i][c];  S = the 11 A_b added in ascending b;  feature = (100.0 * A_b) / S + SPFH_b(i), or
 *   SPFH_b(i) alone where S == 0; rounded to fp32 once.  A point that is not a point or has no finite normal: 33 NaN.
 * sgam_features_match_f32: source [Ns][33], target [Nt][33] fp32 (dim must be 33) -> per source row the target row of least
 *   (d2 bits, index): d2 = the fp32 sum of (a_j - b_j)^2, j = 0..32 in ascending order, starting from the first square; a
 *   candidate needs d2 < +inf (a NaN never compares): a row without one gets index -1, d2 +inf.  Brute force, target rows
 *   through LDS in tiles of 256.
 * sgam_points_ransac_hypotheses: source [Ns][3], target [Nt][3], corr [C][2] int32 (source row, target row), H hypotheses,
 *   ransac_n 3 or 4 -> samples [H][4] int32 (-1 past ransac_n and for a draw that failed), valid [H] int32 (1 / 0), poses
 *   [H][12] fp64, a row-major 3 x 4 (zeros when not valid).
 *   Draw: slot s = 0 .. ransac_n - 1 in order; draw number q counts from 0 through the whole hypothesis; w = word 0 of
 *   Philox4x32-10 at counter (h, q, 0, 0) under key (seed & 0xffffffff, seed >> 32); pick = (w * C) >> 32 (64-bit product); a
 *   pick equal to an earlier slot's is drawn again with the next q; after 16 draws in all without ransac_n distinct picks the
 *   hypothesis is void.  Void too: a picked row of corr outside [0, Ns) x [0, Nt), or a picked point that is not a point.
 *   Checks, fp64 on the widened points p_s (source) and q_s (target): for the slot pairs (a, b), a < b, b ascending then a
 *   ascending: la = |p_a - p_b|, lb = |q_a - q_b| (sqrt of (dx dx + dy dy) + dz dz); void unless la >= similarity * lb and
 *   lb >= similarity * la.  Then Horn's closed form: cs = ((p_0 + p_1) + p_2 (+ p_3)) / n, ct alike; S_ab = sum over the slots
 *   in order of (p - cs)_a (q - ct)_b; the symmetric N = [[Sxx + Syy + Szz, Syz - Szy, Szx - Sxz, Sxy - Syx], [., (Sxx - Syy) -
 *   Szz, Sxy + Syx, Szx + Sxz], [., ., (Syy - Sxx) - Szz, Syz + Szy], [., ., ., (Szz - Sxx) - Syy]]; 8 sweeps of cyclic Jacobi
 *   rotations over (0,1), (0,2), (0,3), (1,2), (1,3), (2,3) (the rotation of sgam_points_normals_f32); the eigenvector of the
 *   largest diagonal entry (the lowest index on a tie), normalised, as the quaternion (w, x, y, z); R = [[1 - 2 (yy + zz),
 *   2 (xy - wz), 2 (xz + wy)], [2 (xy + wz), 1 - 2 (xx + zz), 2 (yz - wx)], [2 (xz - wy), 2 (yz + wx), 1 - 2 (xx + yy)]];
 *   t = ct - R cs.  Void unless all twelve are finite and every slot has |R p + t - q|^2 <= max_distance * max_distance.
 * sgam_points_ransac_score: poses and valid as above -> counts [H] int32: the correspondences c with
 *   d2(transform34(fp32(pose), source[corr[c][0]]), target[corr[c][1]]) <= max_d2 (fp32; sgam_points_transform_f32's and the
 *   search's expressions; a row of corr out of range or a point that is not a point is no inlier), -1 for a hypothesis that is
 *   not valid; best [1] uint64: the maximum over the valid h of (count << 32) | (0xffffffff - h) — the largest count, the lowest
 *   h on a tie — by one 64-bit integer atomic maximum; 0: no valid hypothesis.  compact != 0: the valid hypotheses are gathered
 *   first (an integer atomic counter: the order of the list varies, no output does) so that no lane idles on a void one;
 *   workspace: sgam_points_ransac_score_workspace_bytes(H) bytes, 16-byte aligned (SGAM_EWORKSPACE otherwise).
 * sgam_points_ransac_inliers: the winner of `best` unpacked on the device, nothing read back: mask [C] uint8 (1: inlier of the
 *   best pose, by the score's rule), index [Ns] int32: for a source point with an inlier correspondence the largest target row
 *   among them (an integer atomic maximum), -1 elsewhere: the fixed correspondences of the refit; state [16] fp64: the best
 *   pose as a row-major 4 x 4, UNTOUCHED when best == 0; info [2] int32: the hypothesis (-1: none) and its count (0).
 * ------------------------------------------------------------------------------------------ */
int sgam_points_fpfh_counts(const float *points, const float *normals, int32_t N, const int32_t *knn_index, int32_t k, int32_t *counts,
                            void *stream);
int sgam_points_fpfh_combine_f32(const int32_t *counts, const float *points, const float *normals, int32_t N, const int32_t *knn_index,
                                 const float *knn_d2, int32_t k, float *features, void *stream);
int sgam_features_match_f32(const float *source, int32_t Ns, const float *target, int32_t Nt, int32_t dim, float *d2, int32_t *index,
                            void *stream);
int sgam_points_ransac_hypotheses(const float *source, int32_t Ns, const float *target, int32_t Nt, const int32_t *corr, int32_t C,
                                  int32_t H, int32_t ransac_n, double edge_length_similarity, double max_distance, uint64_t seed,
                                  int32_t *samples, int32_t *valid, double *poses, void *stream);
int64_t sgam_points_ransac_score_workspace_bytes(int32_t H);
int sgam_points_ransac_score(const float *source, int32_t Ns, const float *target, int32_t Nt, const int32_t *corr, int32_t C,
                             const double *poses, const int32_t *valid, int32_t H, float max_d2, int32_t compact, void *workspace,
                             int64_t workspace_bytes, int32_t *counts, uint64_t *best, void *stream);
int sgam_points_ransac_inliers(const float *source, int32_t Ns, const float *target, int32_t Nt, const int32_t *corr, int32_t C,
                               const double *poses, int32_t H, const uint64_t *best, float max_d2, uint8_t *mask, int32_t *index,
                               double *state, int32_t *info, void *stream);

/* ------------------------------------------------------------------------------------------
 * Multiway registration (csrc/pose_graph.hip): the pose graph over pairwise registrations, optimised on the device
 * by Levenberg-Marquardt with a line process on the uncertain edges (Choi, Zhou, Koltun, CVPR 2015; the structure of Open3D's
 * GlobalOptimizationLevenbergMarquardt after Madsen-Nielsen, recalled and unpinned), and the dense fp64 SPD solve it needs.  Poses,
 * state and history are DEVICE memory; an attempt is a fixed sequence of launches and reads nothing back.  No atomics; every output
 * is a function of the inputs only and equal run to run.  Everything but the solve is restated in tests/posegraph_oracle.py and is
 * compared with it bit for bit: all fp64, one IEEE operation per operator in the written order (the unit is built without
 * contraction).
 *
 * The model.  N <= 1024 nodes; node i has the pose P_i, 16 doubles, a row-major rigid 4 x 4 (row 3 is never read and is copied).
 *   One node, `fixed`, never moves.  E <= 65536 edges e = (s, t, T_st, Lambda_e, uncertain_e): T_st the registration of cloud s
 *   onto cloud t (16 doubles), Lambda_e a symmetric 6 x 6 information matrix (36 doubles, every entry read), ordered (omega, v)
 *   like sgam_points_icp_update; s != t; a pair may have several edges.
 *   inverse of a rigid X = [R | t]:  [R^T | u],  u_r = -((R[0][r] * t[0] + R[1][r] * t[1]) + R[2][r] * t[2]).
 *   product of rigid X, Y:  Z[r][c] = (X[r][0] * Y[0][c] + X[r][1] * Y[1][c]) + X[r][2] * Y[2][c],  and Z[r][3] = that + X[r][3].
 *   sum6(m, v) = ((((m_0 * v_0 + m_1 * v_1) + m_2 * v_2) + m_3 * v_3) + m_4 * v_4) + m_5 * v_5.
 *   Residual:  A = P_t^-1,  B = P_s * T_st^-1,  M = A * B  (the error in the target's frame, where ICP's J^T J measures a left
 *     perturbation of T_st);  r = ((M21 - M12) * 0.5, (M02 - M20) * 0.5, (M10 - M01) * 0.5, M03, M13, M23).
 *   Jacobian for P_i <- exp(delta_i) P_i:  dr / d delta_s = J, dr / d delta_t = -J, exact to first order.  Column k < 3 (rotation
 *     about axis k, k1 = (k + 1) % 3, k2 = (k + 2) % 3):  Q[r][c] = A[r][k2] * B[k1][c] - A[r][k1] * B[k2][c]  (c = 0..3),
 *     J[.][k] = ((Q21 - Q12) * 0.5, (Q02 - Q20) * 0.5, (Q10 - Q01) * 0.5, Q03, Q13, Q23).  Column 3 + k: (0, 0, 0, A[0][k], A[1][k],
 *     A[2][k]).
 *   Line process:  y_a = sum6(Lambda[a][.], r),  q = sum6(r, y);  l = 1 on a certain edge, t * t with t = mu / (mu + q) on an
 *     uncertain one;  cost_e = l * q, on an uncertain edge + mu * (d * d) with d = sqrt(l) - 1.  F = the fold of cost_e.
 *   Normal equations, n = 6 N, dense:  W = l * Lambda (per entry),  wr_a = sum6(W[a][.], r),  wj_a = sum6(W[a][.], J[.][k]),
 *     K[j][k] = sum6(J[.][j], wj),  g_j = sum6(J[.][j], wr).  H_ss += K, H_tt += K, H_st -= K, H_ts -= K^T, b_s -= g, b_t += g:
 *     every 6 x 6 block and every b_i starts from 0.0 and takes its edges in ASCENDING EDGE INDEX (a gather over incidence lists, no
 *     atomics); block (a, c), a < c, is summed once and stored at (a, c) and transposed at (c, a).  The fixed node's rows and columns
 *     are the identity and its b is 0.
 *   The fold (cost, and delta . (lambda delta + b)): one workgroup; lane t of 256 sums the items t, t + 256, ... in ascending order
 *     from 0.0, then s[t] = s[t] + s[t + h] for h = 128, 64, ..., 1.
 *
 * state: 16 DEVICE doubles: [0] lambda, [1] nu, [2] F, [3] status (0 running, 1 converged, 2 degenerate), [4] accepted iterations,
 *   [5] attempts that reached the solve, [6] live and [7] accepted (flags of the current attempt), [8] the fold's F', [9] the fold's
 *   delta . (lambda delta + b), [10] max |b|, [11] mu (set by the caller), [12..15] 0.  The caller starts with zeros and mu.
 *   history [rows][8] doubles, row `attempt` = {F, lambda, rho, max |b|, accepted, F', status, nu} after the attempt.
 *
 * sgam_pose_graph_check: HOST arrays src, dst [E] -> SGAM_OK, or SGAM_EINVAL for N outside 1..1024, E outside 0..65536, fixed
 *   outside [0, N), an index outside [0, N) or s == t.  The device entry points trust their index arrays: check them first.
 * sgam_pose_graph_linearize: poses [N][16], src, dst [E], transforms [E][16], information [E][36], uncertain [E] uint8, mu =
 *   state[11] -> r [E][6], J [E][36], q, l, cost [E], K [E][36], g [E][6]; one lane per edge.
 * sgam_pose_graph_assemble: K, g and the block lists -> H [6N][6N] (zeroed first), b [6N].  blocks >= N: block i < N is the
 *   diagonal block of node i, the others the pairs (block_row < block_col) that have an edge, each once; block_ptr [blocks + 1]
 *   into block_entry, whose entries are 2 e + flag in ascending e: on a diagonal block flag = 1 where the node is e's target (b += g,
 *   else b -= g), on a pair flag = 1 where e's source is the larger node (the block takes -K^T, else -K).  gated != 0: nothing is
 *   written unless state[7] is 1 (an attempt's reassembly after an accepted trial).
 * sgam_pose_graph_fold: cost [E] -> state[8]; with delta and b [n] also state[9] (delta NULL: 0).
 * sgam_pose_graph_gate: rules 1 and 2 of attempt k.  sgam_pose_graph_trial: rule 4's poses.  sgam_pose_graph_decide: mode 0 the
 *   prologue (F = state[8], lambda = 1e-5 * max_i H_ii over the free rows, nu = 2, l <- l_trial), mode 1 rules 5 and 6.
 *
 * The optimiser.  Prologue: linearize at the initial poses, fold, assemble (gated = 0), decide (mode 0).  Attempt k, every kernel
 * of which returns at once when status != 0 (the host loop issues max_iterations attempts and never looks):
 *   1. status != 0: the row is {F, lambda, 0, 0, 0, 0, status, nu}; nothing else changes.
 *   2. max |b| < gradient_tolerance: status 1, the row {F, lambda, 0, max |b|, 0, 0, 1, nu}.
 *   3. (H + lambda I) delta = b by sgam_spd_solve_f64 with status = state + 3; a failed pivot gives status 2.
 *   4. P'_i = [dR(omega_i) | v_i] P_i, (omega_i, v_i) = delta[6 i .. 6 i + 5], dR by rule 6 of sgam_points_icp_update (sin and cos of
 *      the device library); linearize at P' gives l' and, folded, F'.
 *   5. rho = (F - F') / den, den = the fold of delta_i * (lambda * delta_i + b_i); a den that is not finite or <= 0 is a rejection.
 *   6. rho > 0: accept.  lambda <- lambda * max(1 / 3, 1 - (s * s) * s) with s = 2 * rho - 1, nu <- 2, iterations += 1; F - F' <=
 *      relative_cost * F: status 1; then P, l, F take the trial's values and H, b are assembled from the trial's K, g (gated = 1).
 *      Otherwise: reject.  |F - F'| <= relative_cost * F: status 1, lambda and nu stay (the trial's cost cannot be told from F, so
 *      rounding decides the sign of rho, not the model: without this rule a run that has converged to the precision of its cost
 *      but not to gradient_tolerance rejects until lambda overflows).  Else lambda <- lambda * nu, nu <- 2 * nu; a lambda that is
 *      not finite: status 2.
 *
 * sgam_spd_solve_f64: A [n][ld] fp64 (the lower triangle is read), n <= 6144, lambda a DEVICE double or NULL (0), b [n] -> x [n]
 *   with (A + lambda I) x = b, by A + lambda I = L L^T.  workspace: sgam_spd_solve_workspace_doubles(n) doubles.  status: one DEVICE
 *   double; every launch returns at once when it is not 0; a pivot that is not finite or <= 1e-12 * the damped diagonal entry it
 *   started from (sgam_points_icp_update's rule) sets it to 2, and x is then not written.  Right-looking in 64-column panels on a
 *   copy padded to a multiple of 64 with the identity: the diagonal tile by one workgroup in LDS, the tiles below it by a
 *   triangular solve (one lane per row), the trailing lower tiles by v_mfma_f64_16x16x4_f64, then blocked forward and back
 *   substitution.  No atomics: equal run to run.  The MFMA's and the explicit fused multiply-adds round once per step, so the
 *   result is NOT bit-equal to a plain-IEEE restatement; it meets the backward-error bound of Cholesky.
 *
 * SGAM_EINVAL, nothing launched: NULL pointers (lambda, and sgam_pose_graph_fold's delta, excepted), N outside 1..1024, E outside
 *   1..65536 (sgam_pose_graph_check: 0..65536), n outside 1..6144, ld < n, fixed outside [0, N), blocks outside N..N + 65536, a
 *   workspace that is too small, attempt < 0, a tolerance that is negative or NaN, a mode other than 0 and 1.
 * ------------------------------------------------------------------------------------------ */
int sgam_pose_graph_check(const int32_t *src_host, const int32_t *dst_host, int32_t E, int32_t N, int32_t fixed);
int sgam_pose_graph_linearize(const double *poses, int32_t N, const int32_t *src, const int32_t *dst, const double *transforms,
                              const double *information, const uint8_t *uncertain, int32_t E, const double *state, double *r, double *J,
                              double *q, double *l, double *cost, double *K, double *g, void *stream);
int sgam_pose_graph_assemble(const double *K, const double *g, int32_t N, int32_t fixed, const int32_t *block_row,
                             const int32_t *block_col, const int32_t *block_ptr, const int32_t *block_entry, int32_t blocks,
                             const double *state, int32_t gated, double *H, double *b, void *stream);
int sgam_pose_graph_fold(const double *cost, int32_t E, const double *delta, const double *b, int32_t n, double *state, void *stream);
int sgam_pose_graph_gate(const double *b, int32_t n, int32_t attempt, double gradient_tolerance, double *state, double *history,
                         void *stream);
int sgam_pose_graph_trial(const double *poses, const double *delta, int32_t N, const double *state, double *trial, void *stream);
int sgam_pose_graph_decide(int32_t mode, int32_t attempt, const double *H, int32_t N, int32_t fixed, double relative_cost, double *poses,
                           const double *trial, double *l, const double *l_trial, int32_t E, double *state, double *history,
                           void *stream);
int64_t sgam_spd_solve_workspace_doubles(int32_t n);
int sgam_spd_solve_f64(const double *A, int32_t n, int64_t ld, const double *lambda, const double *b, double *workspace,
                       int64_t workspace_doubles, double *x, double *status, void *stream);

/* ------------------------------------------------------------------------------------------
 * Reprojection view consistency (csrc/view_consistency.hip; restated in tests/consistency_oracle.py).
 *
 * For each of P ordered pairs (s, t) of F stored frames of one size (H, W) and one set of intrinsics: every pixel of frame s put
 * into camera t with its own depth and T_rel[p] = the top 3 x 4 of T_t T_s^-1 (float64 on the host, rounded once), classified
 * against what frame t holds there, and the colour and depth errors of the pixels both frames see.  Every fp32 operator is ONE
 * IEEE operation in the written order, nothing fused:
 *     valid(x) := fabsf(x) <= F32_MAX && z_near <= x && x <= z_far                     (NaN fails)
 *     d = depth_s[i][j]                                        class 0 INVALID      unless valid(d)
 *     a = (kinv[0] * j + kinv[1] * i) + kinv[2]   b: kinv[3..5]   c: kinv[6..8]     x = a * d   y = b * d   z = c * d
 *     X = ((T[0] * x + T[1] * y) + T[2] * z) + T[3]   Y: T[4..7]   Z: T[8..11]
 *                                                              class 1 OUT_OF_VIEW  unless z_near <= Z && Z <= z_far
 *     u = (fx * X) / Z + cx        v = (fy * Y) / Z + cy
 *     x0f = floorf(u)   y0f = floorf(v)                        class 1 OUT_OF_VIEW  unless 0 <= x0f && x0f <= W - 2 && 0 <= y0f && y0f <= H - 2
 *     wx = u - x0f   wy = v - y0f   x0 = (int)x0f   y0 = (int)y0f      (the last row and column of t never receive a footprint)
 *     D00 D01 D10 D11 = depth_t at (y0, x0) (y0, x0 + 1) (y0 + 1, x0) (y0 + 1, x0 + 1)
 *     Dn = the corner at (y0 + (wy >= 0.5f), x0 + (wx >= 0.5f))
 *                                                              class 2 TARGET_HOLE  unless valid(Dn)
 *     e = Z - Dn                                               class 3 OCCLUDED     if  e > tau
 *                                                              class 4 VIOLATION    if -e > tau
 *                                                              class 5 EDGE         unless every corner Dk is valid and fabsf(Z - Dk) <= tau
 *     class 6 COVISIBLE:  lerp(p00, p01, p10, p11) = top + wy * (bot - top),  top = p00 + wx * (p01 - p00),  bot = p10 + wx * (p11 - p10)
 *       ez = Z - lerp(D..)          ec = (float)rgb_s[i][j][c] - lerp((float) of the four uint8 corners of rgb_t), c = r, g, b
 *       color_error = (|er| + |eg|) + |eb|  (units of 0..255)         depth_error = ez
 * sums [P][12] DEVICE doubles: [0..6] the class counts; over the covisible pixels [7] sum color_error, [8] sum (er^2 + eg^2) + eb^2
 *   (each e converted to double first), [9] sum |ez|, [10] sum ez^2 (in double), [11] sum |ez| / Z (the division in fp32).  A lane
 *   holds one pixel; a workgroup's 256 are summed in a fixed order, the pair's workgroups in block order: equal bits run to run.
 * class_map uint8, color_error, depth_error fp32, each [P][H][W] or NULL (not written); the errors are 0 where the class is not 6.
 * depth_ptrs / rgb_ptrs: DEVICE tables of F addresses ((H,W) fp32, (H,W,3) uint8).  pairs [P][2] int32 DEVICE: a pair with an
 *   index outside [0, F) reads nothing and gets a zero row (class 0 in the map).  kinv9: HOST.  T_rel [P][12] DEVICE.
 * workspace: sgam_view_consistency_workspace_bytes(H, W, P) bytes, 16-byte aligned; negative for refused sizes.
 * SGAM_EINVAL, nothing launched: a NULL required pointer, F < 1, H < 2, W < 2, P outside 1..65535, H W >= 2^31, a tolerance that is
 *   negative or NaN, z_near > z_far or either NaN, a workspace that is too small or misaligned.
 * ------------------------------------------------------------------------------------------ */
int64_t sgam_view_consistency_workspace_bytes(int32_t H, int32_t W, int32_t P);
int sgam_view_consistency_f32(const void *depth_ptrs, const void *rgb_ptrs, int32_t F, int32_t H, int32_t W, const float *kinv9, float fx,
                              float fy, float cx, float cy, float z_near, float z_far, float depth_tolerance, const int32_t *pairs,
                              const float *T_rel, int32_t P, double *sums, uint8_t *class_map, float *color_error, float *depth_error,
                              void *workspace, int64_t workspace_bytes, void *stream);

/* ------------------------------------------------------------------------------------------
 * Direct RGB-D odometry of P frame pairs in lock step (csrc/rgbd_odometry.hip; restated in
 * tests/odometry_oracle.py).  The step that minimises the image error the view consistency above measures: per pair (s, t) the pose
 * T (source camera -> target camera) is refined by Gauss-Newton steps on a photometric and a geometric residual of the pixels
 * both frames see, coarse to fine over an image pyramid.  Open3D's hybrid RGB-D odometry (compute_rgbd_odometry with the hybrid
 * term, as recalled; unpinned against Open3D) with two deliberate differences:
 *   - correspondences are the view consistency's COVISIBLE class with bilinear reads, where Open3D rounds to the nearest pixel and
 *     z-buffers: no atomics and no z-buffer are needed;
 *   - the image gradients are the exact derivatives of that bilinear interpolant, where Open3D uses Sobel images: Gauss-Newton
 *     differentiates the function it minimises, and no gradient image is stored.
 *
 * Pyramid (sgam_rgbd_pyramid_f32), fp32, one IEEE operation per operator in the written order:
 *   level 0:    I = (float)(r + g + b) / 765.0f (the sum an integer),  D = the stored depth
 *   level l+1:  rows r_k = clamp(2 i + k - 1, 0, H_l - 1), columns c_k = clamp(2 j + k - 1, 0, W_l - 1), k = 0, 1, 2 (clamped borders)
 *               h(r) = (I[r][c_0] + 2 * I[r][c_1]) + I[r][c_2]        I' = ((h(r_0) + 2 * h(r_1)) + h(r_2)) * 0.0625f
 *               (the 3 x 3 binomial filter at (2 i, 2 j); the weights are dyadic)
 *               D' = D[2 i][2 j]: no filtering, validity is never averaged.
 *   H_{l+1} = (H_l + 1) / 2, W_{l+1} = (W_l + 1) / 2.  The intrinsics of level l are K_l = diag(2^-l, 2^-l, 1) K (fx, fy, cx, cy
 *   each halved per level, exact); kinv9 of a level is inv(K_l) in float64 rounded once.  At most 4 levels; a level smaller than
 *   2 x 2 is refused.
 *   intensity, depth: DEVICE fp32, the levels one after the other, level l being [F][H_l][W_l] at offset F * sum_{k<l} H_k W_k.
 *
 * Accumulate (sgam_rgbd_odometry_accumulate_f32), per pair p = (s, t) on one level with its H, W, kinv9, fx, fy, cx, cy;
 * T = state[p][0..11] rounded to fp32 once (as in sgam_points_transform_f32).  Every source pixel (i, j) goes through the view
 * consistency's expressions unchanged, on the level's depth planes with tau = max_depth_diff: valid(d), the ray, (X, Y, Z) = p',
 * u, v, x0f, y0f, wx, wy, the four corners D00 D01 D10 D11, Dn, and the class tests.  Only class 6 pixels contribute.  For such a
 * pixel, in fp64 on the widened fp32 values (wx, wy, X, Y, Z, the corners of the target's depth D and intensity I, the source's
 * intensity I_s), one IEEE operation per operator:
 *     L(c)   = top + wy * (bot - top),  top = c00 + wx * (c01 - c00),  bot = c10 + wx * (c11 - c10)          (the lerp above)
 *     L_u(c) = (c01 - c00) + wy * ((c11 - c10) - (c01 - c00))              L_v(c) = bot - top
 *     iz = 1 / Z;  ux = fx * iz;  uz = -((ux * X) * iz);  vy = fy * iz;  vz = -((vy * Y) * iz)
 *                                                           (du/dp' = (ux, 0, uz) = (fx / Z, 0, -fx X / Z^2), dv/dp' = (0, vy, vz))
 *     photometric row:  g = (-(L_u(I) * ux), -(L_v(I) * vy), -(L_u(I) * uz + L_v(I) * vz))            r_I = sp * (I_s - L(I))
 *     geometric row:    g = (-(L_u(D) * ux), -(L_v(D) * vy), 1 - (L_u(D) * uz + L_v(D) * vz))         r_Z = sg * (Z - L(D))
 *     either row:       c = (Y g.z - Z g.y,  Z g.x - X g.z,  X g.y - Y g.x)     J = (w c.x, w c.y, w c.z, w g.x, w g.y, w g.z), w = sp or sg
 *     sg = sqrt(lambda_geometric), sp = sqrt(1 - lambda_geometric)
 *   The pose update is the left perturbation T <- exp(xi) T in the (omega, v) order and c = p x n shape of
 *   sgam_points_icp_accumulate, whose 32 slots these are: slot of (a, b), a <= b: J_I[a] * J_I[b] then + J_Z[a] * J_Z[b];
 *   21 + a: J_I[a] * r_I then + J_Z[a] * r_Z;  27: r_I^2 then + r_Z^2;  28: (Z - L(D))^2, unweighted (rmse is a depth RMSE);
 *   29: 1 per covisible pixel;  30: 1 per source pixel of class != 0;  31: 0.
 *   information != 0 (the information matrix of a pose-graph edge, the same kernel): over the covisible pixels at the pose of
 *   state[p], q = p' where frames is NULL, else q = the fp32 expression X = ((F[0] x + F[1] y) + F[2] z) + F[3] ... of p' with
 *   F = frames[p] (a 3 x 4, fp32); slots 0..20 are the point-to-point sums of sgam_points_icp_accumulate on q (G = [-[q]x | I]),
 *   21..28 are 0, 29..31 as above: mirrored, Lambda[5][5] is the covisible count.  The pair's status is not looked at.
 *   Order of summation: a workgroup takes 1024 consecutive pixels, a lane the pixels base + c * 256 + lane in ascending c; the
 *   workgroup's sums go to the workspace ([P][ceil(H W / 1024)][32] doubles) in a fixed order; no atomics.
 *   information == 0: a pair whose state[p][18] is 2, or 1 unless level_first != 0, reads nothing and gets zero sums (the update
 *   does not look at them).  A pair with an index outside [0, F) reads nothing and gets zero sums.
 *
 * Update (sgam_rgbd_odometry_update): per pair the workgroup sums are folded per slot in block order from 0.0 (equal bits run to
 * run; written to sums [P][32] where sums is not NULL, unless the pair is frozen), then with row >= 0 rules 1-6 of
 * sgam_points_icp_update are applied word for word to state [P][24] and history [P][rows][8] at row `row`: fitness = slot 29 /
 * slot 30, rmse = sqrt(slot 28 / slot 29), count < 6 -> status 2, the stop test, the Cholesky pivot rule, the exponential.  One
 * addition for the pyramid: with level_first != 0 (the first iteration of a level; the very first iteration is one) a status 1 left
 * by the coarser level returns to 0 before rule 1 and the stop test of rule 4 is skipped (rule 4's `iteration > 0` reads
 * `level_first == 0`).  Status 2 is final at every level.  History rows are numbered across levels, coarse to fine; the host issues
 * every iteration of every level and never looks.  row == -1: the fold alone, into sums (required then); state and history unused.
 *
 * depth_ptrs / rgb_ptrs / intensity_ptrs: DEVICE tables of F addresses.  pairs [P][2] int32 DEVICE.  kinv9: HOST.
 * workspace: sgam_rgbd_odometry_workspace_bytes(H, W, P) bytes of the level, 16-byte aligned; negative for refused sizes.
 * SGAM_EINVAL, nothing launched: a NULL required pointer, F < 1, H or W < 2, P outside 1..65535, levels outside 1..4 or a level
 *   smaller than 2 x 2, a max_depth_diff that is negative or NaN, a lambda_geometric outside [0, 1] or NaN, z_near > z_far or either
 *   NaN, frames without information, a row outside -1..rows - 1, a criterion that is negative or NaN, a workspace that is too
 *   small or misaligned.
 * ------------------------------------------------------------------------------------------ */
int sgam_rgbd_pyramid_f32(const void *depth_ptrs, const void *rgb_ptrs, int32_t F, int32_t H, int32_t W, int32_t levels, float *intensity,
                          float *depth, void *stream);
int64_t sgam_rgbd_odometry_workspace_bytes(int32_t H, int32_t W, int32_t P);
int sgam_rgbd_odometry_accumulate_f32(const void *depth_ptrs, const void *intensity_ptrs, int32_t F, int32_t H, int32_t W, const float *kinv9,
                                      float fx, float fy, float cx, float cy, float z_near, float z_far, float max_depth_diff,
                                      double lambda_geometric, const int32_t *pairs, const double *state, int32_t P, int32_t level_first,
                                      int32_t information, const float *frames, void *workspace, int64_t workspace_bytes, void *stream);
int sgam_rgbd_odometry_update(const void *workspace, int64_t workspace_bytes, int32_t H, int32_t W, int32_t P, int32_t row, int32_t rows,
                              int32_t level_first, double relative_fitness, double relative_rmse, double *state, double *history,
                              double *sums, void *stream);

/* ------------------------------------------------------------------------------------------
 * Segmentation of a cloud (csrc/point_segment.hip; restated in tests/segmentation_oracle.py): the points within a
 * radius, DBSCAN clusters, RANSAC planes with a least-squares refit, and the box of every cluster.  points [N][3] fp32 DEVICE; the
 * arithmetic rules of the point-cloud units hold (one IEEE fp32 operation per operator in the written order; a point with a
 * coordinate that is not finite is "not a point"); integer atomics only; every output has the same bits run to run.
 *
 * sgam_points_radius_count_brute_f32 / _grid_f32: count_out [N] = the number of neighbours of point i: the points j (i itself
 *   included) with d2 = (dx * dx + dy * dy) + dz * dz <= max_d2, dx = p_j.x - p_i.x (dy, dz alike); 0 for a non-point.  The grid
 *   form takes the arguments and the workspace of sgam_points_grid_build over the SAME cloud (Nr = N) and walks its shells until the
 *   stop rule's lower bound exceeds max_d2; both forms and every cell size give the same bits.
 *
 * sgam_points_dbscan_brute_f32 / _grid_f32: count_out as above; core_out [N] = 1 where count >= min_points.  A cluster is a connected
 *   component of the core points under the neighbour relation, its root its least core index; clusters are numbered 0, 1, ... in
 *   ascending root order.  A point that is not core joins the cluster of its core neighbour of least (d2 bits, index) — an exact
 *   tie goes to the lower core index; Open3D's rule is first come, first served —, without one it is noise.  labels_out [N]: the
 *   cluster, -1 for noise and non-points; sizes_out [N]: the members of cluster l at [l], 0 from n_clusters on; n_clusters_out: one
 *   DEVICE int32.  flag: a DEVICE int32 the caller zeroes; bit 0 is set where a union-find loop reached its bound (never with an
 *   intact workspace).  workspace: sgam_points_dbscan_workspace_bytes(N) bytes, 16-byte aligned.
 *
 * sgam_points_segment_planes_f32: max_planes rounds r of plane RANSAC over the points no earlier round took, as one launch sequence.
 *   Hypothesis h < H of round r: three distinct positions of the ascending list of the n_active active points, candidate =
 *   (w0 * n_active) >> 32 with w0 = word 0 of Philox4x32-10 at counter (h, draw, r, 0) under key (seed low word, seed high word), a
 *   repeated candidate drawn again, 16 draws at most.  In fp64: n = (p1 - p0) x (p2 - p0), nn = (nx nx + ny ny) + nz nz,
 *   n *= 1 / sqrt(nn), d = -((nx p0x + ny p0y) + nz p0z), rounded to four fp32 (a, b, c, d).  Invalid: a failed pick, n_active < 3,
 *   nn zero or not finite.  Inlier: fabsf(((a * x + b * y) + c * z) + d) <= threshold in fp32.  The winner is the valid hypothesis
 *   of the greatest inlier count over the active points, a tie to the lowest h (no RMSE tie-break and no early exit, unlike Open3D);
 *   with a count below max(min_inliers, 3) or no valid hypothesis the round's planes are NaN, its count 0 and nothing is taken.
 *   labels_out [N] = the round whose winner took the point, else -1; ransac_planes_out [max_planes][4] the winners; counts_out
 *   [max_planes] their inlier counts; planes_out [max_planes][4] the least-squares plane through each winner's inliers: the
 *   centroid, then the centred second moments about it, in fp64 — per lane over the points base + c * 256 + lane of a block of 4096
 *   in ascending c, the lanes folded as in sgam_points_md_reduce, the blocks folded in block order —, the eigenvector of the least
 *   eigenvalue of the moments by the Jacobi sweeps of sgam_points_normals_f32 (the lowest axis on a tie), normalised, flipped so that
 *   its dot product with the winner's normal is >= 0, d = -n . centroid, rounded to fp32.
 *   workspace: sgam_points_planes_workspace_bytes(N, H) bytes, 16-byte aligned.  H <= 2^24.
 * sgam_points_plane_score_f32: the score kernel alone: counts_out [H] = the inliers of planes [H][4] (16-byte aligned; a NaN plane
 *   scores 0) among the points whose labels entry is negative (labels NULL: all points).  R = hypotheses per lane, 1, 2 or 4;
 *   0 = the library's choice.  The counts do not depend on R.
 *
 * sgam_points_cluster_boxes_f32: over the points with 0 <= labels[i] < n_clusters: count_out [n_clusters], lo_out / hi_out
 *   [n_clusters][3] the least / greatest coordinate per axis (integer atomics on order-preserving keys); a label without a
 *   point: lo +inf, hi -inf.
 *
 * SGAM_EINVAL, nothing launched: a NULL required pointer, N < 1, H < 1, max_planes < 1, min_points < 1, min_inliers < 0, n_clusters
 *   < 1, a max_d2 or threshold that is negative or NaN, a grid that sgam_points_grid_build would refuse or with Nr != N, an R other
 *   than 0, 1, 2, 4.  SGAM_EWORKSPACE: a workspace that is NULL, too small or misaligned.
 * ------------------------------------------------------------------------------------------ */
int sgam_points_radius_count_brute_f32(const float *points, int32_t N, float max_d2, int32_t *count_out, void *stream);
int sgam_points_radius_count_grid_f32(const float *points, int32_t Nr, float ox, float oy, float oz, float cell_size, int32_t gx, int32_t gy,
                                      int32_t gz, const void *grid_workspace, int64_t grid_workspace_bytes, float max_d2,
                                      int32_t *count_out, void *stream);
int64_t sgam_points_dbscan_workspace_bytes(int32_t N);
int sgam_points_dbscan_brute_f32(const float *points, int32_t N, float max_d2, int32_t min_points, void *workspace, int64_t workspace_bytes,
                                 int32_t *count_out, uint8_t *core_out, int32_t *labels_out, int32_t *sizes_out, int32_t *n_clusters_out,
                                 int32_t *flag, void *stream);
int sgam_points_dbscan_grid_f32(const float *points, int32_t Nr, float ox, float oy, float oz, float cell_size, int32_t gx, int32_t gy,
                                int32_t gz, const void *grid_workspace, int64_t grid_workspace_bytes, float max_d2, int32_t min_points,
                                void *workspace, int64_t workspace_bytes, int32_t *count_out, uint8_t *core_out, int32_t *labels_out,
                                int32_t *sizes_out, int32_t *n_clusters_out, int32_t *flag, void *stream);
int64_t sgam_points_planes_workspace_bytes(int32_t N, int32_t H);
int sgam_points_segment_planes_f32(const float *points, int32_t N, int32_t H, int32_t max_planes, float threshold, int32_t min_inliers,
                                   uint64_t seed, void *workspace, int64_t workspace_bytes, int32_t *labels_out, float *planes_out,
                                   float *ransac_planes_out, int32_t *counts_out, void *stream);
int sgam_points_plane_score_f32(const float *points, const int32_t *labels, int32_t N, const float *planes, int32_t H, float threshold,
                                int32_t R, int32_t *counts_out, void *stream);
int sgam_points_cluster_boxes_f32(const float *points, const int32_t *labels, int32_t N, int32_t n_clusters, int32_t *count_out,
                                  float *lo_out, float *hi_out, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* SGAM_HIP_H */
