/*
 * diffsal.h -- C ABI of libdiffsal_hip.so: the MI355X (gfx950) operator library for
 * DiffSal's per-step denoiser (SalUNet) hot path.
 *
 * Conventions:
 *   - plain pointers and sizes only; every pointer is a DEVICE pointer unless said otherwise;
 *   - activations are channels-last: images [N,H,W,C], tokens [M,C]; fp32 by default.  Forward operators that take a
 *     `dtype` argument (DIFFSAL_F32 / DIFFSAL_BF16 / DIFFSAL_F16, declared below) read and write their `void*`
 *     activation tensors in that storage type; `float*` arguments (norm parameters, biases, depthwise weights,
 *     the timestep path, the sampler state) are always fp32, and all arithmetic / statistics are fp32;
 *   - every entry point enqueues work on `stream` (a hipStream_t) and returns immediately:
 *       0 on success, a negative DIFFSAL_E_* code on failure (diffsal_last_error() has the text);
 *   - no allocation, no synchronisation, no host-visible side effect inside an entry point,
 *     so every call is legal under HIP-graph capture;
 *   - re-entrant; the only global state is a thread-local error string (arithmetic mode and storage type are
 *     per-call arguments: diffsal_conv_desc.precision / .dtype and the `dtype` argument of the other operators).
 *
 * Each entry point cites the reference interface it replaces (R/ = junwenxiong/diff_sal).
 */
#ifndef DIFFSAL_H
#define DIFFSAL_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef void* diffsal_stream_t; /* hipStream_t */

enum {
  DIFFSAL_OK = 0,
  DIFFSAL_E_SHAPE = -1,   /* unsupported / inconsistent dimensions */
  DIFFSAL_E_ALIGN = -2,   /* pointer not 16-byte aligned */
  DIFFSAL_E_LAUNCH = -3,  /* hipGetLastError() after launch */
  DIFFSAL_E_ARG = -4      /* null pointer / bad enum */
};

enum { DIFFSAL_ACT_NONE = 0, DIFFSAL_ACT_RELU = 1, DIFFSAL_ACT_GELU_ERF = 2, DIFFSAL_ACT_SIGMOID = 3,
       /* training only, fp32 diffsal_conv_igemm only: out = (product + bias ...) * gelu'(residual[m, co]) -- `residual` carries the
        * pre-activation of the erf-GELU in front of the layer whose data gradient this product is, and is NOT added */
       DIFFSAL_ACT_GELU_GRAD = 5 };

/* Bumped whenever a signature or struct in this header changes.  diffsal_version() returns the value the binary was compiled
 * with; a binding compares it with the header it reads, so a stale libdiffsal_hip.so is refused instead of being called with
 * other argument lists. */
#define DIFFSAL_ABI_VERSION 53
int diffsal_version(void);
const char* diffsal_last_error(void);
/* Name and tile plan of the kernel the last diffsal_conv_igemm / diffsal_linear_pair / diffsal_conv_wino4 call of THIS thread
 * launched (e.g. "gemm_dma_kernel<96x96,3 stages>", "igemm_linear_kernel<64x64>", "igemm_kernel<128x96> split-K 2"): lets a
 * profiler attribute HIP-event times to kernels without a tracing tool (bench.py's roofline.dominant_kernel).  Thread-local,
 * never NULL; not part of the reference's surface. */
const char* diffsal_last_gemm_kernel(void);

/* Test / tuning switches (kernel-variant selection for bit-equality tests and tile sweeps; none changes results beyond
 * summation order).  The DIFFSAL_* environment variables of the same names are read ONCE when the library is loaded; afterwards
 * only this call changes a switch (value < 0 = unset).  Names: DIFFSAL_NO_PERSIST, DIFFSAL_NO_XCD_ORDER, DIFFSAL_NO_HALO,
 * DIFFSAL_FORCE_HALO, DIFFSAL_IGEMM_CFG, DIFFSAL_IGEMM16_CFG, DIFFSAL_PLAN_DEBUG, DIFFSAL_WGRAD_CFG, DIFFSAL_WGRAD_SPLITS,
 * DIFFSAL_WGRAD_VERBOSE, DIFFSAL_NO_FUSED_BLOCK, ... (the full list: DIFFSAL_TUNE_KEYS in csrc/common.h); round 6:
 * DIFFSAL_NO_STREAM16 = 1 routes 16-bit storage back to the 8-byte forms of the HBM-bound kernels and to the kernels the planner took before
 * conv16_dma / gemm16_dma2; DIFFSAL_FORCE_HALO = 2 and DIFFSAL_GEMM_DMA16 = 3 / 4 take those two (gemm16_dma2 with its 256 x 96 / 192 x 192
 * tile) on every shape they can run; DIFFSAL_CONV16_TILE = 0 / 1 keeps conv16_dma off / on its 8 x 24 x 192-channel tile, DIFFSAL_CONV16_HALF = 0 / 1 off / on its 128-pixel tiles; DIFFSAL_FRONT_FOLD_WGS = 1 runs diffsal_block_front_fold as one workgroup per CU with a next-tile look-ahead;
 * DIFFSAL_BLOCK16_WAVES = 4 / 8 fixes the wavefronts per workgroup of the fused C = 96 block; DIFFSAL_TAPSUM_ROWS_FORM = 1 .. 4 takes the
 * row-streamed head gather (and its lane mapping) instead of the LDS-staged one; DIFFSAL_NO_ATTN16_MFMA = 1 keeps the 16-bit attention core
 * of head dims 192 / 384 off the matrix cores.
 * Not part of the reference's surface (it has no such knobs). */
int diffsal_set_tuning(const char* name, int value);
int diffsal_get_tuning(const char* name);   /* current value, -1 if unset or unknown */

/* ---- K1: timestep embedding + MLP ------------------------------------------------------
 * R/models/saliency_decoder/sal_unet.py:15-33 (get_timestep_embedding) and :304-307.
 * t: [B] int64 (t_is_f32 == 0) or float (t_is_f32 == 1); freq: [ch/2] table exp(-j*ln(1e4)/(ch/2-1)).
 * temb_out[B,4ch] = W1 * swish(W0 * [sin(t f), cos(t f)] + b0) + b1 */
int diffsal_temb_mlp(const void* t, int t_is_f32, int B, int ch, const float* freq,
                     const float* w0, const float* b0, const float* w1, const float* b1,
                     float* hidden_ws /* scratch [B,4ch] */, float* temb_out, diffsal_stream_t stream);

/* out[B,N] = W[N,K] * f(in[B,K]) + bias, f = swish if swish_in.  ResnetBlock.temb_proj of all
 * blocks in one call (weights concatenated along N).  R/.../sal_unet.py:107,129. */
int diffsal_dense_small(const float* in, int B, int K, int swish_in, const float* w, const float* bias,
                        int N, float* out, diffsal_stream_t stream);

/* ---- K12 / K14 restructured: a 3x3 convolution (dilation dil) of a bilinearly up-sampled map, or of a SUM of up-sampled
 * maps, without forming the up-sampled map (csrc/tapsum.hip):
 *   conv3x3( sum_i up_i(z_i) )[p] = sum_i sum_tap up_i( W_tap z_i )[p + dil * delta_tap]       (1x1 mixing commutes with bilerp)
 * The nine channel mixings of every source run as ONE diffsal_conv_igemm at the SOURCE resolution,
 * Y_i [N, h_i, w_i, 9*C] = z_i x Wcat^T with Wcat[tap*C + co][ci] = W[co][ci][ky][kx]; this entry gathers
 *   out[n,Y,X,c] = act(scale[c] * (bias[c] + sum_i sum_tap [p' inside] bilerp_i(Y_i[..., tap*C + c]; p')) + shift[c])
 * with p' = (Y,X) + dil*(ky-1,kx-1) (taps outside the image are the convolution's zero padding).  Sources: 1..4, each a
 * power-of-two factor (>= 1) smaller than H x W; act NONE or RELU.  UpEmbed's first convolution
 * (bilinear x2 + 3x3 dilation 2, common_block.py:196-216): 4x fewer FLOPs; mt_proj on the 4-scale sum (sal_unet.py:480-489,
 * :407): 3x fewer.  Exact up to summation order. */
int diffsal_tapsum(const void* const* srcs, const int* hs, const int* ws, int n_src, void* out, int N, int H, int W, int C,
                   int dil, const float* bias, const float* scale, const float* shift, int act, int dtype,
                   diffsal_stream_t stream);
/* The same gather with MLPHead folded into its epilogue (common_block.py:111-122: 1x1 convolution C -> 1 + sigmoid; C <= 128):
 *   head_out[n, Y, X] = sigmoid( head_b[0] + sum_c head_w[c] * out[n, Y, X, c] ),   fp32 [N, H, W]
 * the C-channel map `out` is never stored (mt_proj -> BN -> ReLU -> logits of sal_unet.py:489 + :320 in one launch). */
int diffsal_tapsum_head(const void* const* srcs, const int* hs, const int* ws, int n_src, int N, int H, int W, int C, int dil,
                        const float* bias, const float* scale, const float* shift, int act, const float* head_w,
                        const float* head_b, float* head_out, int dtype, diffsal_stream_t stream);
/* Training: the adjoint of diffsal_tapsum (act NONE, no affine) with respect to ONE source's tap products,
 *   dy [N,h,w,9*C] (fp32) from du [N,H,W,C]; ws: diffsal_tapsum_bwd_ws_bytes(N, W, C, h) bytes of scratch (the three row passes).
 * Gather form, deterministic; replaces the full-resolution dgrad + wgrad of the convolution behind nn.Upsample in training
 * (common_block.py:196-216, sal_unet.py:480-489). */
long diffsal_tapsum_bwd_ws_bytes(int N, int W, int C, int h);
int diffsal_tapsum_bwd(const float* du, float* dy, float* ws, int N, int H, int W, int C, int h, int w, int dil,
                       diffsal_stream_t stream);

/* ---- K2 fused: conv_in followed directly by Downsample4x4's 3x3 stride-4 convolution (sal_unet.py:240,292 + :67-84) as ONE
 * 5x5 stride-4 convolution of the single-channel input; w25 [25][C] (tap-major) and bias [C] are the composed weights
 * W_eff[co][dy][dx] = sum_ci sum_{ky2+ky1=dy, kx2+kx1=dx} W2[co,ci,ky2,kx2] W1[ci,ky1,kx1], b_eff = b2 + sum W2 b1 (host side).
 * Exact for H, W multiples of 4.  x NCHW [B,1,H,W] fp32 -> out NHWC [B,H/4,W/4,C] in `dtype`. */
int diffsal_conv_in_s4(const float* x, const float* w25, const float* bias, void* out, int B, int H, int W, int C, int dtype,
                       diffsal_stream_t stream);

/* ---- K2: conv_in (1 -> C, 3x3, pad 1), NCHW[B,1,H,W] -> NHWC[B,H,W,C] -----------------
 * R/.../sal_unet.py:240,292.  Only pixels with (y % skip_mod != skip_mod-1 && x % skip_mod != skip_mod-1)
 * are written when skip_mod > 0 (the stride-4 consumer never reads the others, sal_unet.py:67-84). */
int diffsal_conv_in(const float* x, const float* w /*[C,9]*/, const float* bias, void* out,
                    int B, int H, int W, int C, int skip_mod, int act /*DIFFSAL_ACT_NONE | RELU*/, int dtype,
                    diffsal_stream_t stream);

/* ---- K3: GroupNorm(groups, eps) + swish on NHWC ----------------------------------------
 * R/.../sal_unet.py:36-44.  ws: >= diffsal_groupnorm_ws_bytes(B, groups) bytes of scratch. */
size_t diffsal_groupnorm_ws_bytes(int B, int groups);
int diffsal_groupnorm_swish(const void* x, const float* gamma, const float* beta, void* out,
                            int B, int HW, int C, int groups, float eps, void* ws, size_t ws_bytes, int dtype,
                            diffsal_stream_t stream);

/* ---- K4/K5/K10/K12/K13/K14: implicit-GEMM convolution / linear on fp32 MFMA -------------
 * out[m, co] = act( ((sum_k A[m,k] * w[co,k]) + bias[co]) * scale[co] + shift[co] + rowvec[img(m), co] )
 *              + residual[m, co]
 * A is the im2col view of in[N,H,W,Cin] (never materialised): m = (n, oy, ox), k = (ci / 32, ky, kx, ci % 32),
 * iy = oy*stride_h - pad_t + ky*dil_h, ix = ox*stride_w - pad_l + kx*dil_w, zero outside.
 * w: packed [Cout][Cin/32][KH*KW][32] (= [Cout][K] in that k order).  bias/scale/shift: [Cout] or NULL.  rowvec: [N, rowvec_ld] or NULL.
 * residual: [M, Cout] or NULL.  Cin % 32 == 0.  A plain linear layer is KH=KW=1, H=1, W=rows.
 * Replaces torch.nn.Conv2d / Conv3d(k,1,1) / Linear call sites:
 *   R/.../sal_unet.py:104-142 (ResnetBlock), :47-84 (Downsample*), common_block.py:33-36,150-223,
 *   attention.py:78-83, common_block.py:125-147, transformer.py:122,131. */
typedef struct diffsal_conv_desc {
  int N, H, W, Cin;
  int Ho, Wo, Cout;
  int KH, KW, stride_h, stride_w, pad_t, pad_l, dil_h, dil_w;
  int act;        /* DIFFSAL_ACT_* */
  int rowvec_ld;  /* leading dimension of rowvec (>= Cout) */
  int w_format;   /* 0: fp32 [Cout][K] (k order above).  1: the same rows pre-split for the bf16x3 mode by
                   * diffsal_split_weight: per 32-k slice 16 dwords of bf16 hi halves then 16 dwords of lo halves (same
                   * size); only valid with precision == DIFFSAL_PREC_BF16X3 */
  int precision;  /* DIFFSAL_PREC_*: arithmetic of the matrix-core loop for fp32 storage (below) */
  int dtype;      /* DIFFSAL_F32 / DIFFSAL_BF16 / DIFFSAL_F16: storage type of in, w, residual and out (bias, scale,
                   * shift, rowvec are always fp32; accumulation is always fp32).  16-bit storage uses the native
                   * v_mfma_f32_32x32x16_{bf16,f16}; `precision` must then be DIFFSAL_PREC_FP32 (= "native") */
} diffsal_conv_desc;

/* Arithmetic of diffsal_conv_igemm's matrix-core loop for fp32 tensors, chosen PER CALL (diffsal_conv_desc.precision):
 *   DIFFSAL_PREC_FP32 (default): exact fp32, v_mfma_f32_32x32x2_f32;
 *   DIFFSAL_PREC_BF16X3: each fp32 operand is split into bf16 hi + lo on its way into LDS and the product is formed as
 *     hi*hi + hi*lo + lo*hi on v_mfma_f32_32x32x16_bf16 with fp32 accumulation (error ~2^-16 relative per product,
 *     ~4e-6 of the output maximum on the network's convolutions; well inside the 1e-3 parity bar, but not bit-equal
 *     to fp32).  Opt-in; benchmark numbers for it are reported separately from the headline. */
enum { DIFFSAL_PREC_FP32 = 0, DIFFSAL_PREC_BF16X3 = 1 };
/* Storage type of activations / weights (BASELINE configs[1] "bf16", configs[4] "fp16"): statistics of every
 * normalisation, softmax and all accumulations stay fp32; parameters of norms, biases and the timestep path stay fp32. */
enum { DIFFSAL_F32 = 0, DIFFSAL_BF16 = 1, DIFFSAL_F16 = 2 };

/* ---- scratch sizes, one entry point --------------------------------------------------------------------------
 * Bytes of caller-provided scratch the operator `op` needs for a shape: `d` for the operators described by a diffsal_conv_desc,
 * `dims` (n_dims integers, in the order of the typed function's arguments) for the others; 0 = the operator needs none for this
 * shape, or op / argument count unknown.  The typed functions below (diffsal_*_ws_bytes, ..._floats) are the same numbers with
 * named arguments; the library never allocates, a workspace is whatever the caller's allocator hands over. */
enum {
  DIFFSAL_WS_GROUPNORM = 0,      /* dims = {B, groups}                 diffsal_groupnorm_ws_bytes (also diffsal_gn_affine) */
  DIFFSAL_WS_CONV_IGEMM = 1,     /* d                                  diffsal_conv_igemm_ws_bytes */
                                 /* 2: retired (the F(2x2) Winograd path); answers 0 like any unknown operator */
  DIFFSAL_WS_CONV_WINO4 = 3,     /* d                                  diffsal_conv_wino4_ws_bytes */
  DIFFSAL_WS_CONV_WINO4_STATS = 4, /* d, dims = {groups}               diffsal_conv_wino4_stats_bytes */
  DIFFSAL_WS_CONV_WGRAD = 5,     /* d                                  diffsal_conv_wgrad_ws_bytes */
  DIFFSAL_WS_WGRAD_SEGMENTED = 6, /* dims = {segments, seg_rows, K, Cout}  diffsal_wgrad_segmented_ws_bytes */
  DIFFSAL_WS_TAPSUM_BWD = 7,     /* dims = {N, W, C, h}                diffsal_tapsum_bwd_ws_bytes */
  DIFFSAL_WS_SALIENCY_METRICS = 8, /* dims = {B}                       diffsal_saliency_metrics_ws_bytes */
  DIFFSAL_WS_ATTENTION_TAIL = 9, /* dims = {B, H, Lq, Lk, DV}          4 x diffsal_attention_general_tail_floats */
  DIFFSAL_WS_ATTENTION_BWD_QTAIL = 10, /* dims = {B, H, Lq, Lk, D, E}  4 x diffsal_attention_general_bwd_qtail_floats */
  DIFFSAL_WS_ATTENTION_BWD_DS = 11     /* dims = {B, H, Lq, Lk}        4 x diffsal_attention_general_bwd_ds_floats */
};
size_t diffsal_workspace_bytes(int op, const diffsal_conv_desc* d /*host, may be NULL*/, const long* dims /*host*/, int n_dims);

/* Bytes of scratch the call below can use for this descriptor: the largest workspace any candidate kernel could ask for, over all
 * candidates that can take the descriptor under any pointer alignment (csrc/igemm.hip walks the same ordered list as the launch).
 * 0 unless some candidate plans a split-K, which it does when the M x Cout grid alone cannot fill the 256 CUs. */
size_t diffsal_conv_igemm_ws_bytes(const diffsal_conv_desc* d /*host*/);
int diffsal_conv_igemm(const diffsal_conv_desc* d /*host*/, const void* in, const void* w,
                       const float* bias, const float* scale, const float* shift, const float* rowvec,
                       const void* residual, void* out, void* ws, size_t ws_bytes, diffsal_stream_t stream);

/* 16-bit storage in, fp32 out (plain products: KH = KW = 1, d->dtype bf16 / f16): out [M, Cout] fp32 = act(in x w^T + bias), the sums
 * leave without a rounding to the storage type -- for consumers that add many products (the nine interpolated tap products of
 * mt_proj, R/models/saliency_decoder/sal_unet.py:480-489).  K % 192 == 0, Cout % 4 == 0. */
int diffsal_linear_f32out(const diffsal_conv_desc* d /*host*/, const void* in, const void* w, const float* bias, float* out,
                          diffsal_stream_t stream);

/* Winograd F(4x4, 3x3) form of the same operator for fp32 3x3 stride-1 convolutions with padding = dilation in {1, 2} (or dilation
 * 1, padding 2, output (H + 2) x (W + 2): the extended grid diffsal_up2_conv_commute reads), Cin % 96 == 0, Cout % 4 == 0
 * (ResnetBlock.conv1 / conv2, R/models/saliency_decoder/sal_unet.py:104-142; UpEmbed's convolutions, common_block.py:196-216):
 * 4x fewer multiplications than the direct convolution; transform rounding ~1e-5 of the output maximum.  `U` is G g G^T as
 * [36][Cout][Cin] fp32 (ops.pack_wino4_weight).  Three launches: input transform, the 36 position products as one batched
 * plain product, output transform + epilogue.  ws: diffsal_conv_wino4_ws_bytes(d) = 36 * tiles * (Cin + Cout) floats.
 * diffsal_conv_wino4_supported: the shape qualifies and the planner expects a gain over diffsal_conv_igemm
 * (DIFFSAL_NO_WINOGRAD=1: never, DIFFSAL_FORCE_WINOGRAD=1: whenever the shape qualifies). */
int diffsal_conv_wino4_supported(const diffsal_conv_desc* d /*host*/);
/* U = G g G^T on the device, fp32 (training: the weights change every step).  w [Cout][Cin][3][3]; dgrad = 0 -> U [36][Cout][Cin] (the forward
 * convolution); dgrad = 1 -> U [36][Cin][Cout] of the flipped kernel: the data gradient dX = conv(dY, .) of a stride-1, padding = dilation
 * convolution runs on the same F(4x4) path with it. */
int diffsal_wino4_weight(const float* w, float* U, int Cout, int Cin, int dgrad, diffsal_stream_t stream);
size_t diffsal_conv_wino4_ws_bytes(const diffsal_conv_desc* d /*host*/);
/* diffsal_conv_wino4: epilogue and argument meaning as diffsal_conv_igemm, plus
 *   stages            which of the three launches run: bit 0 input transform, bit 1 position products, bit 2 output transform +
 *                     epilogue; 7 = the whole convolution.  Same arguments and workspace for every call of one convolution: for
 *                     profilers that bracket operator launches (bench.py attributes the transforms to the HBM-bound classes and
 *                     the products to the GEMM kernel).
 *   ext               (host, may be NULL) extras for a ResnetBlock (R/models/saliency_decoder/sal_unet.py:123-142: h =
 *                     conv1(swish(norm1(x))) + temb; out = nin_shortcut(x) + conv2(swish(norm2(h)))) and for UpEmbed, all optional
 *                     (zero / NULL = off):
 *   in_ab, in_swish   the input is read through y = a[n][c] x + b[n][c] (ab = [N][2][Cin]: scale row then shift row per image:
 *                     GroupNorm in affine form, diffsal_gn_affine / diffsal_gn_affine_wino4) and, if in_swish, y sigmoid(y), as the
 *                     input transform loads it: no normalised tensor in memory.  The zero padding applies to the normalised map.
 *   side_*            side_out [side_rows, Cout] = side_a [side_rows, Cin] x side_w [Cout, Cin]^T (no epilogue) computed by the SAME
 *                     launch as the 36 position products, as side_rows / tiles further problems of their shape (the block's 1x1
 *                     shortcut; diffsal_conv_wino4_side_supported: side_rows must be a multiple of the tile count).
 *   out_stats, out_groups   the output transform leaves per-(image, group) sums / sums of squares of the RESULT in out_stats
 *                     (diffsal_conv_wino4_stats_bytes bytes; 0 = not available for the shape) for diffsal_gn_affine_wino4:
 *                     the GroupNorm that follows needs no statistics pass.
 *   up2_c, up2_scale, up2_shift, up2_act   UpEmbed's second convolution (dilation 2) fed from the SOURCE-resolution result of the
 *                     first one (R/.../common_block.py:196-216): up2_c = conv3x3(z) on the extended grid [N][H/2 + 2][W/2 + 2][Cin]
 *                     (what diffsal_up2_conv_commute takes as c_ext); the input transform forms act(BN(interpolation of up2_c)) itself
 *                     -- the arithmetic of diffsal_up2_conv_commute's interior -- and reads from `x` only the 3-pixel border ring, which
 *                     diffsal_up2_conv_commute_ring must have written there.  dil = 2, H and W even, fp32; excludes in_ab. */
typedef struct diffsal_wino4_ext {
  const float* in_ab;
  const float* side_a;
  const float* side_w;
  float* side_out;
  double* out_stats;
  const float* up2_c;
  const float* up2_scale;
  const float* up2_shift;
  long long side_rows;
  int in_swish;
  int out_groups;
  int up2_act;
  int reserved;
} diffsal_wino4_ext;
size_t diffsal_conv_wino4_stats_bytes(const diffsal_conv_desc* d /*host*/, int groups);
int diffsal_conv_wino4_side_supported(const diffsal_conv_desc* d /*host*/, long side_rows);
int diffsal_conv_wino4(const diffsal_conv_desc* d /*host*/, const float* x, const float* U, const float* bias,
                       const float* scale, const float* shift, const float* rowvec, const float* residual, float* out,
                       void* ws, size_t ws_bytes, const diffsal_wino4_ext* ext /*host, may be NULL*/, int stages,
                       diffsal_stream_t stream);
/* GroupNorm(groups, eps; gamma, beta) in affine form: ab [B][2][C] with y = ab[b][0][c] x + ab[b][1][c] (statistics in fp64).
 * diffsal_gn_affine: from the tensor x [B, HW, C] (one statistics launch + a finishing launch; ws as diffsal_groupnorm_swish);
 * diffsal_gn_affine_wino4: from the sums a diffsal_conv_wino4 call left in ext.out_stats (same d, same groups).
 * R/models/saliency_decoder/sal_unet.py:41-44. */
int diffsal_gn_affine(const void* x, const float* gamma, const float* beta, float* ab, int B, int HW, int C, int groups,
                      float eps, void* ws, size_t ws_bytes, int dtype, diffsal_stream_t stream);
int diffsal_gn_affine_wino4(const diffsal_conv_desc* d /*host*/, const double* stats, const float* gamma, const float* beta,
                            int groups, float eps, float* ab, diffsal_stream_t stream);
/* zb [N][2 w + 2 h - 4][C] = the border pixels of z [N][h][w][C] in the order diffsal_up2_conv_commute reads their tap products
 * (top row, bottom row, left column, right column; the columns without their corner pixels).  C % 8 == 0. */
int diffsal_border_gather(const void* z, void* zb, int N, int h, int w, int C, int dtype, diffsal_stream_t stream);
/* conv3x3(dilation 2, padding 2)(bilinear_up2(z)) -> BN affine -> activation (UpEmbed's first convolution,
 * R/models/saliency_decoder/common_block.py:196-206) from c_ext = conv3x3(z) (dilation 1, zero padding) evaluated at the SOURCE
 * resolution on the grid extended by one pixel on every side ([N][h + 2][w + 2][C]: diffsal_conv_wino4 / diffsal_conv_igemm with
 * padding 2 and output (h + 2) x (w + 2)) and tap_border = the nine tap products W_tap z of the border pixels of z
 * ([N][2 w + 2 h - 4][9][C]: top row, bottom row, left column and right column without their corners; tap = 3 ky + kx).  A shift by two output pixels is a shift by
 * one source pixel: the result is the unclamped interpolation of c_ext plus corrections on a 3-pixel border ring (csrc/upconv.hip);
 * exact up to summation order.  c_ext, tap_border and out ([N][2 h][2 w][C]) are in the storage type `dtype` (fp32 arithmetic in
 * between); act: DIFFSAL_ACT_NONE or DIFFSAL_ACT_RELU. */
int diffsal_up2_conv_commute(const void* c_ext, const void* tap_border, const float* scale, const float* shift, void* out,
                             int N, int h, int w, int C, int act, int dtype, diffsal_stream_t stream);
/* the same, writing ONLY the 3-pixel border ring of `out` (for diffsal_conv_wino4 with ext.up2_c) */
int diffsal_up2_conv_commute_ring(const void* c_ext, const void* tap_border, const float* scale, const float* shift, void* out,
                             int N, int h, int w, int C, int act, int dtype, diffsal_stream_t stream);
/* Up to four independent convolutions / plain products (own descriptor, operands and output; bias + activation epilogue
 * only) in ONE launch: the four ReduceTemp products of a step (R/models/saliency_decoder/common_block.py:150-173,
 * sal_unet.py:480-487) have 336 .. 21504 rows and 3840 .. 480 columns of K, each alone fills a fraction of the chip.  fp32
 * problems that fit the LDS-DMA kernel (K a multiple of 96) share one grid, longest units first; anything else runs as n
 * diffsal_conv_igemm calls (same results).  `ws` / `ws_bytes`: the largest diffsal_conv_igemm_ws_bytes of the problems. */
int diffsal_conv_igemm_group(int n, const diffsal_conv_desc* const* descs, const void* const* in, const void* const* w,
                             const float* const* bias, void* const* out, void* ws, size_t ws_bytes, diffsal_stream_t stream);

/* Two plain products of ONE shape in one launch (grid z = 2): out_i [M,N] = in_i [M,K] x w_i [N,K]^T + bias_i.  The key and value
 * projections of a transformer block (attention.py:78-83: proj_k / proj_v on the 648 pooled tokens of a stage) are 8-26 us
 * launches at their latency floor; paired they are four launches per step instead of eight.  d: a 1x1 descriptor (KH = KW = 1,
 * act NONE, exact arithmetic, any storage type); ws: 2 x diffsal_conv_igemm_ws_bytes(d) bytes. */
int diffsal_linear_pair(const diffsal_conv_desc* d, const void* in0, const void* in1, const void* w0, const void* w1,
                        const float* bias0, const float* bias1, void* out0, void* out1, void* ws, size_t ws_bytes,
                        diffsal_stream_t stream);


/* ---- weight layout transforms (w: the reference's parameter layout [Cout][Cin][taps], taps = KH*KW or KT):
 *   mode 0: dst[co][(ci/32, tap, ci%32)] = w[co][ci][tap]            -- the `w` argument of diffsal_conv_igemm
 *   mode 1: dst[ci][(co/32, tap, co%32)] = w[co][ci][taps-1-tap]     -- `w` of the data-gradient conv (Cout % 32 == 0)
 *   mode 2: dst[co][ci][tap] = src[co][(ci/32, tap, ci%32)]          -- diffsal_conv_wgrad output back to parameter layout
 *   mode 3: dst[(tap, ci)][co] = w[co][ci][tap]                      -- GEMM weight of dXcols = dY W (Cout % 32 == 0)
 * Cin % 32 == 0, taps <= 25.
 * col2im_disjoint: data gradient of a convolution whose taps never overlap (stride >= kernel, e.g. the 3x3 stride-4
 * Downsample, sal_unet.py:47-84, and ReduceTemp's k=s=5 Conv3d, common_block.py:125-142): dx[n,iy,ix,:] = the one
 * cols[(n,oy,ox)][(ky,kx)][:] that maps there, else 0; cols [N*Ho*Wo, KH*KW*C] comes from one diffsal_conv_igemm GEMM. */
int diffsal_col2im_disjoint(const float* cols, float* dx, int N, int H, int W, int C, int Ho, int Wo, int KH, int KW,
                            int stride_h, int stride_w, int pad_t, int pad_l, diffsal_stream_t stream);
/* col2im_gather: the same for OVERLAPPING taps (1 < stride < kernel: the 3x3 stride-2 Downsample of the ResBlock encoder,
 * sal_unet.py:47-84): every input pixel sums, in (ky, kx) order, the column entries that map onto it.  With the mode-3
 * GEMM in front this is the strided data gradient at exactly the forward's MAC count. */
int diffsal_col2im_gather(const float* cols, float* dx, int N, int H, int W, int C, int Ho, int Wo, int KH, int KW,
                          int stride_h, int stride_w, int pad_t, int pad_l, diffsal_stream_t stream);
int diffsal_pack_weight(const float* src, float* dst, int Cout, int Cin, int taps, int mode, diffsal_stream_t stream);
/* Many repacks in one launch (training: every layer's layouts are rebuilt after each optimizer step).  jobs_dev: DEVICE array of
 * n_jobs entries sorted by tile0, tile0 = running sum of (Cin / 32) * ceil(Cout / 32); total_tiles = that sum over all jobs;
 * max_taps = largest taps of the batch.  Each job obeys diffsal_pack_weight's shape rules. */
typedef struct diffsal_pack_job {
  const void* src;
  void* dst;
  int Cout, Cin, taps, mode;
  int tile0, reserved;
} diffsal_pack_job;
int diffsal_pack_weight_many(const diffsal_pack_job* jobs_dev /*device*/, int n_jobs, int total_tiles, int max_taps,
                             diffsal_stream_t stream);
/* bf16x3 mode: split a packed fp32 weight [rows][K] (K % 32 == 0) into the w_format = 1 layout of diffsal_conv_desc
 * (hi = bf16(x), lo = bf16(x - hi)); n = rows * K.  Saves the kernel the conversion of its B operand. */
int diffsal_split_weight(const float* src, float* dst, long n, diffsal_stream_t stream);

/* ---- K16 (training): weight gradient of the layer above, in the SAME packed layout as `w`:
 * dw[co, k] = sum_m dy[m, co] * A[m, k].  Replaces the wgrad of autograd's conv / linear backward.
 * ws: >= diffsal_conv_wgrad_ws_bytes(d) bytes (partial slabs, summed in a fixed order).  Cout % 4 == 0.
 * dbias_part (optional, may be NULL): [diffsal_conv_wgrad_splits(d)][Cout] doubles receiving the column sums of dy per
 * M split -- the bias gradient rides along on the dY tiles the kernel stages anyway.  dbias_out (optional, needs dbias_part):
 * [Cout] floats, the finished bias gradient (split sums added in split order by the launch that sums the weight slabs, or
 * written directly when there is one split); without it finish with diffsal_reduce_partials(dbias_part, db, 1, splits, Cout, 0). */
size_t diffsal_conv_wgrad_ws_bytes(const diffsal_conv_desc* d /*host*/);
int diffsal_conv_wgrad_splits(const diffsal_conv_desc* d /*host*/);
int diffsal_conv_wgrad(const diffsal_conv_desc* d /*host*/, const float* in, const float* dy, float* dw_packed,
                       double* dbias_part, float* dbias_out, void* ws, size_t ws_bytes, diffsal_stream_t stream);
/* Batched form for token GEMMs: out[s][co][k] = sum over the seg_rows rows m of segment s of dy[m, co] * x[m, k]
 * (x: [segments*seg_rows, K], dy: [segments*seg_rows, Cout]).  Used by the attention backward (one segment per
 * image: dK = dS^T Q, dV = P^T dO; R/.../attention.py:97-108).  K % 32 == 0, Cout % 4 == 0. */
size_t diffsal_wgrad_segmented_ws_bytes(int segments, int seg_rows, int K, int Cout);
int diffsal_wgrad_segmented(const float* x, const float* dy, float* out, int segments, int seg_rows, int K, int Cout,
                            void* ws, size_t ws_bytes, diffsal_stream_t stream);
/* out[g, c] = sum of dy[m, c] over the rows of segment g (M / seg_rows segments): bias gradients (one segment)
 * and per-image vector gradients (one segment per image).  ws: >= (M/seg_rows) * 512 * C * 8 bytes (fp64 partials:
 * reductions across threads run in double so that heavily cancelling sums do not depend on the atomics order). */
int diffsal_colsum(const float* dy, float* out, int M, int C, int seg_rows, void* ws, size_t ws_bytes,
                   diffsal_stream_t stream);

/* dx = dy * act'(.): mode 1 ReLU (ref = output y), 2 GELU-erf (ref = pre-activation), 3 sigmoid (ref = output y).
 * Backward of the activations fused into the forward epilogues / nn.GELU (common_block.py:137). n % 4 == 0. */
int diffsal_act_bwd(const float* dy, const float* ref, float* dx, size_t n, int mode, diffsal_stream_t stream);

/* ---- K16 (training): normalisation layers ------------------------------------------------------
 * Per-channel dual sums over the rows of each segment -> part[segs][chunks][2][C] (fp64), chunks = diffsal_rowstats_chunks():
 *   mode 0 (x, x^2): BatchNorm (train) / GroupNorm statistics;  mode 1/2/3: (dz, dz*xhat) for BN+ReLU, GN+swish, plain.
 * diffsal_reduce_partials + diffsal_norm_finalize_* fold the partials into per-(segment, channel) vectors for the
 * element-wise kernels below.
 * Replace the forward / backward of nn.BatchNorm2d (train), nn.GroupNorm + swish (sal_unet.py:36-44,
 * common_block.py:33-36,196-216). */
int diffsal_rowstats_chunks(int M, int seg_rows);
int diffsal_rowstats(const float* x, const float* dy, const float* y, const float* mu, const float* rs,
                     const float* gamma, const float* beta, double* part, int M, int C, int seg_rows, int mode,
                     int stat_per_seg, diffsal_stream_t stream);
/* Sum fp64 per-workgroup partials part[segs][chunks][width] over the chunks, fixed order -> out[segs][width]
 * (double if out_is_f64, else float).  Every reduction kernel of the training step leaves such partials. */
int diffsal_reduce_partials(const double* part, void* out, int segs, int chunks, int width, int out_is_f64,
                            diffsal_stream_t stream);
/* GroupNorm / train-mode BatchNorm statistics -> the vectors the apply kernels consume.  sums[segs][2][C] = per-channel
 * (sum x, sum x^2); `groups` channel groups share statistics over n values each (BatchNorm: groups = C, segs = 1,
 * n = rows).  Writes mu, rs, scale = rs*gamma, shift = beta - mu*scale, each [segs][C].  BatchNorm extras, all optional:
 * bn_mean / bn_var [C] (batch mean, biased variance) and the nn.BatchNorm2d running-statistics update
 * run = (1-momentum) run + momentum * (mean | var * unbias)  (R/.../common_block.py:196-223 in train mode).
 * norm_finalize_bwd: t[segs][2][C] = (sum dz, sum dz*xhat) -> dbeta, dgamma [C] and k1, k2, k3 [segs][C] for
 * diffsal_norm_bwd_apply. */
int diffsal_norm_finalize_fwd(const double* sums, const float* gamma, const float* beta, float* mu, float* rs,
                              float* scale, float* shift, int segs, int C, int groups, double n, double eps,
                              float* bn_mean, float* bn_var, float* running_mean, float* running_var, float momentum,
                              float unbias, diffsal_stream_t stream);
int diffsal_norm_finalize_bwd(const double* t, const float* gamma, const float* rs, float* dgamma, float* dbeta, float* k1,
                              float* k2, float* k3, int segs, int C, int groups, double n, diffsal_stream_t stream);
/* out = act(x * scale[seg, c] + shift[seg, c]); act: DIFFSAL_ACT_NONE / RELU, or 4 = swish */
int diffsal_affine_act(const float* x, const float* scale, const float* shift, float* out, int M, int C, int seg_rows,
                       int act, diffsal_stream_t stream);
/* dx = k1*dz - k2 - k3*xhat with [seg, C] coefficient tables (dz, xhat as in rowstats modes 1..3) */
int diffsal_norm_bwd_apply(const float* x, const float* dy, const float* y, const float* mu, const float* rs,
                           const float* gamma, const float* beta, const float* k1, const float* k2, const float* k3,
                           float* dx, int M, int C, int seg_rows, int mode, diffsal_stream_t stream);
/* LayerNorm backward: dx (+ add[M, C] when given: the gradient arriving at x over the residual connection around the normalised
 * branch, so the tape needs no separate accumulation pass) and per-block partial (dgamma, dbeta) -> part[blocks][2][C],
 * blocks = diffsal_layernorm_bwd_blocks() */
int diffsal_layernorm_bwd_blocks(int M, int C);
/* n <= 3 tensors of one width in ONE launch (MViT's norm_q / norm_k / norm_v on the pooled tensors, R/models/mvit.py:562-570): host arrays of
 * n device pointers / row counts / eps; backward: part [n][blocks][2][C] with blocks = diffsal_layernorm_bwd_blocks(max M, C), finished by
 * diffsal_reduce_partials(part, out, n, blocks, 2*C, 0) -> [n][dgamma | dbeta]. */
int diffsal_layernorm_multi(const float* const* x, const float* const* gamma, const float* const* beta, float* const* out, const int* M,
                            int n, int C, const float* eps, diffsal_stream_t stream);
int diffsal_layernorm_bwd_multi(const float* const* x, const float* const* dy, const float* const* gamma, float* const* dx, double* part,
                                const int* M, int n, int C, const float* eps, diffsal_stream_t stream);
int diffsal_layernorm_bwd(const float* x, const float* dy, const float* gamma, const float* add, float* dx, double* part, int M, int C,
                          float eps, diffsal_stream_t stream);
/* out = x * keep / (1-p), keep from a counter-based hash of (seed, index); same call = its own backward.
 * Replaces nn.Dropout(0.1) of ResnetBlock in train mode (sal_unet.py:109,133). */
int diffsal_dropout(const float* x, float* out, size_t n, float p, uint64_t seed, diffsal_stream_t stream);

/* ---- K16 (training): depthwise projections and attention ---------------------------------------------
 * Plain depthwise k x k convolution on NHWC (w: [k*k][C]) and its two gradients; the training path runs
 * conv_proj_q/k/v (attention.py:36-76) as dwconv + LayerNorm so each half has an exact backward.
 * bwd_weight writes part[k*k][chunks][C], chunks = diffsal_dwconv_bwd_weight_chunks(); the caller sums the chunks. */
int diffsal_dwconv(const float* x, const float* w, float* out, int N, int H, int W, int C, int k, int stride, int pad,
                   diffsal_stream_t stream);
int diffsal_dwconv_bwd_data(const float* du, const float* w, float* dx, int N, int H, int W, int C, int k, int stride,
                            int pad, diffsal_stream_t stream);
int diffsal_dwconv_bwd_weight_chunks(int N, int H, int W, int k, int stride, int pad);
int diffsal_dwconv_bwd_weight(const float* x, const float* du, double* part, int N, int H, int W, int C, int k,
                              int stride, int pad, diffsal_stream_t stream);
/* Backward of diffsal_attention, pass 1: dq [N,Lq,C], plus the softmax P and dS = P (dP - <P,dP>) scale as
 * [N*Lq][ld] rows (column = head*Lk + t, ld >= heads*Lk, columns beyond heads*Lk untouched).  Pass 2 (dk, dv) is
 * diffsal_wgrad_segmented on (dS, q) and (P, dout): no atomics, deterministic. */
int diffsal_attention_bwd_blocks(int Lq, int C, int heads);
int diffsal_attention_bwd(const float* q, const float* k, const float* v, const float* dout, float* dq, float* p_out,
                          float* ds_out, int N, int Lq, int Lk, int C, int heads, int ld, float scale,
                          diffsal_stream_t stream);

/* ---- K16 (training): remaining backward kernels ----------------------------------------------------
 * adjoint of diffsal_resize_bilinear (dy [N,H,W,C] -> dx [N,h,w,C]); backward of pack_frames for the visual
 * features (frames [B,Tin,hw,C] -> NCTHW [B,C,Tv,hw]); head backward (dy = dpre w, part[blocks][C+1] holds
 * sum dpre*y and sum dpre); conv_in parameter gradients (part[10][chunks][C]: 9 taps + bias); dense_small backward. */
/* resize_bilinear_bwd: with ws >= N*h*W*C*4 bytes the adjoint runs as two one-axis passes (rows into ws, then
 * columns); ws may be NULL (single joint pass, much slower for large up-factors). */
int diffsal_resize_bilinear_bwd(const float* dy, float* dx, int N, int h, int w, int H, int W, int C, void* ws,
                                size_t ws_bytes, diffsal_stream_t stream);
int diffsal_unpack_frames(const float* frames, float* vis_grad, int B, int C, int Tv, int Tin, int hw,
                          diffsal_stream_t stream);
int diffsal_head_bwd(const float* y, const float* w, const float* s_out, const float* ds, float* dy, double* part,
                     int blocks, int M, int C, diffsal_stream_t stream);
int diffsal_conv_in_bwd(const float* x, const float* dy, double* part, int B, int H, int W, int C, int chunks,
                        diffsal_stream_t stream);
int diffsal_dense_small_bwd(const float* in, const float* w, const float* dout, float* dw, float* db, float* din,
                            int B, int K, int N, int swish_in, diffsal_stream_t stream);

/* backward of diffsal_audio_fuse: dout [B,C,T,H,W] -> dx [B,T,H,W,C] (frames layout) and the audio-map gradient as
 * per-output-row partials part[((b*T+t)*h + ys)*w + xs][dyr][c] (up = H/h rows per audio row, up <= 8): da_small is
 * diffsal_colsum(part viewed [B*T*h*w*up, C], seg_rows = up); with up == 1 part IS da_small [B*T, h*w, C]. */
int diffsal_audio_fuse_bwd(const float* a_small, const float* x, const float* dout, float* dx, float* part, int B,
                           int T, int H, int W, int C, int h, int w, diffsal_stream_t stream);

/* ---- K6: frame packing: visual features NCTHW[B,C,Tv,h,w] + noise NHWC[B,h,w,C] ->
 * NHWC frames [B,Tv+1,h,w,C] with the noise map as the LAST frame (quirk Q2).
 * Replaces torch.cat(dim=2) + rearrange().contiguous(), R/.../sal_unet.py:311-317,
 * transformer.py:273-279. noise may be NULL (then only Tv frames of a [B,Tout,...] buffer are written, and C may be any
 * positive count: the transpose is scalar; with a noise map C % 4 == 0, since that frame is copied 16 bytes at a time). */
int diffsal_pack_frames(const float* vis /*fp32: the module's input contract*/, const void* noise, void* out, int B,
                        int C, int Tv, int Tout, int hw, int dtype, diffsal_stream_t stream);
/* The same for up to four (vis, noise, out) triples of one batch size and storage type in ONE launch: the frame tensors of all
 * decoder stages (sal_unet.py:414-441 builds them stage by stage). */
int diffsal_pack_frames_multi(const float* const* vis, const void* const* noise, void* const* out, int n, int B, const int* C,
                              const int* Tv, const int* Tout, const int* hw, int dtype, diffsal_stream_t stream);


/* ---- bilinear resize, align_corners=False, NHWC ----------------------------------------
 * R/.../common_block.py:197 (nn.Upsample x2), sal_unet.py:325-327. */
int diffsal_resize_bilinear(const void* in, void* out, int N, int h, int w, int H, int W, int C, int dtype,
                            diffsal_stream_t stream);

/* out[n,Y,X,c] = sum_i bilinear(in_i[n, h_i, w_i, c] -> (H,W)), summed in order i = 0..n_in-1.
 * Replaces the per-stage F.interpolate + "+=" of R/.../sal_unet.py:482-487. n_in <= 4. */
int diffsal_resize_sum(const void* const* ins /*host array of device ptrs*/, const int* hs, const int* ws,
                       int n_in, void* out, int N, int H, int W, int C, int dtype, diffsal_stream_t stream);

/* ---- K7: audio fusion (after the align 1x1 conv) ----------------------------------------
 * R/.../transformer.py:133-146.  a_small: [B*T, h*w, C] tokens; x: NHWC frames [B,T,H,W,C];
 * out: contiguous [B,C,T,H,W] (the reference layout, which the caller then *reinterprets* as
 * [B*T, H*W, C] tokens -- quirk Q5).  up = H / h (nearest), 1 when no upsample. */
int diffsal_audio_fuse(const void* a_small, int a_ld /* elements between a_small's rows (>= C): the four stages' align
                       convolutions run as ONE product whose output rows hold all their channels side by side */,
                       const void* x, void* out, int B, int T, int H, int W, int C,
                       int h, int w, int dtype, diffsal_stream_t stream);

/* ---- K8: LayerNorm over C on tokens [M,C] ------------------------------------------------ */
int diffsal_layernorm(const void* x, const float* gamma, const float* beta, void* out, int M, int C,
                      float eps, int dtype, diffsal_stream_t stream);

/* ---- K9: depthwise projections + LayerNorm ----------------------------------------------
 * q: depthwise 3x3 (pad 1) on NHWC [N,H,W,C] then LN  -> [N, H*W, C].   R/.../attention.py:36-47,94
 * w9: [9][C] (centre temporal slice of the Conv3d weight, quirk Q8). */
int diffsal_dwconv3_ln(const void* x, const float* w9, const float* gamma, const float* beta, void* out,
                       int N, int H, int W, int C, float eps, int dtype, diffsal_stream_t stream);
/* k and v: depthwise kxk stride k (no pad) then LN -> [N, gh*gw, C] each; xk may differ from xv
 * (audio-fused K, attention.py:88-92).  wk, wv: [k*k][C]. */
int diffsal_dwpool_ln_kv(const void* xk, const void* xv, const float* wk, const float* wv,
                         const float* gk, const float* bk, const float* gv, const float* bv,
                         void* out_k, void* out_v, int N, int H, int W, int C, int k, float eps, int dtype,
                         diffsal_stream_t stream);
/* diffsal_dwconv3_ln (query branch) and diffsal_dwpool_ln_kv (key / value branch) of one transformer block in ONE launch: both
 * read the block's normalised frames and neither depends on the other (attention.py:86-95).  Same results as the two entries.
 * pre_gamma / pre_beta (or NULL): the block's own LayerNorm (transformer.py:110, x = self.norm(x)) is applied to every token as
 * it is loaded -- xq and xv are then the UN-normalised frames, xk too when pre_ln_k != 0 (visual-only: the key input is the same
 * normalised tensor; with audio it is the fused audio map, pre_ln_k = 0) -- so the normalised tensor is never written.  Bit-equal
 * with diffsal_layernorm followed by the plain form (the normalised value is rounded through the storage type). */
int diffsal_qkv_prep(const void* xq, const float* w9, const float* gq, const float* bq, void* out_q, const void* xk,
                     const void* xv, const float* wk, const float* wv, const float* gk, const float* bk, const float* gv,
                     const float* bv, void* out_k, void* out_v, int N, int H, int W, int C, int k, float eps,
                     const float* pre_gamma, const float* pre_beta, float pre_eps, int pre_ln_k, int dtype,
                     diffsal_stream_t stream);


/* ---- K8 + K10 fused for the finest stage (C = 96, hidden = 192: both MLP weights fit in LDS):
 *   x2 = x1 + fc2(gelu_erf(fc1(LayerNorm(x1; g2, be2, eps2)) + b1)) + b2 ... i.e. transformer.py:153-157's
 *        `x = x + mlp(norm2(x))` with Mlp of common_block.py:125-147;
 *   z  = LayerNorm(x2; gz, bez, epsz) (sal_unet.py:447,473 norm_mts), written only for tokens of frames < t_keep
 *        (token m belongs to frame (m / hw) % T; ReduceTemp reads frames 0..4 only) -- z may be NULL.
 * x1, x2, z: [M, C] fp32 tokens; w1 [hidden][C], w2 [C][hidden] as stored by nn.Linear.  One launch instead of four; the
 * hidden activations never leave registers.  x2 must not alias x1. */
int diffsal_mlp_block(const float* x1, const float* g2, const float* be2, float eps2, const float* w1, const float* b1,
                      const float* w2, const float* b2, float* x2, float* z, const float* gz, const float* bez, float epsz,
                      long M, int C, int hidden, int hw, int T, int t_keep, diffsal_stream_t stream);

/* The same stage on bf16 / fp16 storage: all three weight matrices fit in LDS, so proj + residual is fused in as well:
 *   x1 = x + o wp^T + bp;  x2 = x1 + fc2(gelu(fc1(LayerNorm(x1))));  z = LayerNorm(x2) on frames < t_keep
 * (attention.py:110, transformer.py:151-157, sal_unet.py:447).  o, x, wp, w1, w2, x2, z: 16-bit (dtype); vectors fp32. */
int diffsal_block16(const void* o, const void* x, const void* wp, const float* bp, const float* g2, const float* be2, float eps2,
                    const void* w1, const float* b1, const void* w2, const float* b2, void* x2, void* z, const float* gz,
                    const float* bez, float epsz, long M, int C, int hidden, int hw, int T, int t_keep, int dtype,
                    diffsal_stream_t stream);

/* ---- K11: attention core ------------------------------------------------------------------
 * o[n,l,:] = concat_h softmax_t( q[n,l,h,:] . k[n,t,h,:] * scale ) v[n,t,h,:],  Lk <= 32.
 * R/.../attention.py:97-108 (scale = C^-0.5, quirk Q6).
 * Accepted: any heads >= 1 with N * heads < 65536, head dim d = C / heads a multiple of 4, and K | V of one head in LDS as fp32 on
 * every storage type: 2 * Lk * d * 4 <= 160 KiB (anything else is DIFFSAL_E_SHAPE before a launch).  Tiles above 64 KiB run with the
 * kernel's dynamic LDS limit raised; the 160 KiB tile itself (Lk = 32, d = 640) launches on gfx950 (tests/test_gpu_instantiations.py). */
int diffsal_attention(const void* q, const void* k, const void* v, void* o, int N, int Lq, int Lk,
                      int C, int heads, float scale, int dtype, diffsal_stream_t stream);

/* ---- attention with proj_q and proj folded onto the key side (fp32, 2 heads; csrc/attn_fold.hip) ---------------------------
 * R/models/saliency_decoder/attention.py:86-113, transformer.py:150-152, re-associated (exact algebra, another summation order):
 *   S_h[l,t] = scale * (q_in[n,l,:] . G[n,t,h,:] + kp[n,t,:] . ukq[h,:]);  P_h = softmax_t(S_h);
 *   out[n,l,:] = x[n,l,:] + bias + sum_h sum_t P_h[l,t] U[n,t,h,:]
 * with G = kp Wkq_h, U = vp Wvp_h [N, Lk, 2, C] (the caller's paired GEMM on the pooled, LayerNorm-ed key / value rows kp, vp
 * [N, Lk, C]), ukq [2, C] and bias = bp + Wp bv [C] weight-only folds.  q_in, x, out [N, L, C].  The score terms that are the same
 * for every key of a head are left out (softmax is shift-invariant).  heads = 2, 1 <= Lk <= 32, C in {192, 384, 768}, any L >= 1.
 * Deterministic: no atomics, one summation order per token whatever N, L or the grid. */
int diffsal_attn_fold(const float* q_in, const float* G, const float* U, const float* kp, const float* ukq, const float* x,
                      const float* bias, float* out, int N, int L, int Lk, int C, int heads, float scale,
                      diffsal_stream_t stream);

/* ---- K14 tail: 1x1 conv C->1 + sigmoid on NHWC -> [N,H,W] --------------------------------
 * R/.../common_block.py:111-122. */
int diffsal_head_sigmoid(const void* x, const float* w /*[C]*/, const float* bias /*[1]*/, float* out /*fp32*/,
                         int NHW, int C, int dtype, diffsal_stream_t stream);

/* ---- fused first half of a TransformerBlock (C = 96, 2 heads; csrc/tblock.hip) --------------------------------------------
 * R/models/saliency_decoder/transformer.py:150-152, attention.py:36-47,87-110:
 *   xn = LayerNorm(x; g1, b1, eps1);  q = Linear_q( LayerNorm(dwconv3x3(xn; w9); gq, bq, epsq) );
 *   o  = softmax(q k^T * scale) v per head, with the block's PROJECTED keys / values k, v [N, Lk <= 32, C];
 *   fp32 storage:   out = x + Linear_p(o)      (x1; the rest of the block is diffsal_mlp_block)
 *   16-bit storage: out = o                    (the rest of the block is diffsal_block16)
 * x, out [N, H, W, C] channels-last in the storage type `dtype`; wq, wp [C, C] in the storage type, row = output feature; w9
 * [9, C] fp32, tap = 3 ky + kx (the centre temporal slice of the Conv3d weight, zero padding 1).  One persistent launch per
 * call instead of LayerNorm, depthwise-q + LayerNorm, the proj_q GEMM, the attention core and the proj GEMM. */
int diffsal_block_front(const void* x, const void* k, const void* v, const float* g1, const float* b1, float eps1,
                        const float* w9, const float* gq, const float* bq, float epsq, const void* wq, const float* bias_q,
                        const void* wp, const float* bias_p, void* out, int N, int H, int W, int C, int Lk, int heads,
                        float scale, int dtype, diffsal_stream_t stream);

/* The same block half on fp32 storage (C = 96, 2 heads) with proj_q and proj folded onto the key side, as diffsal_attn_fold does for
 * the coarser stages (exact algebra, another summation order):
 *   xn = LayerNorm(x; g1, b1, eps1);  q_in = LayerNorm(dwconv3x3(xn; w9); gq, bq, epsq);
 *   S_h[l,t] = scale * (q_in[l,:] . G[n,t,h,:] + kp[n,t,:] . ukq[h,:]);  P_h = softmax_t(S_h);
 *   out = x + bias + sum_h sum_t P_h[l,t] U[n,t,h,:]
 * G, U [N, Lk <= 32, 2 C]: the pooled key / value rows kp, vp [N, Lk, C] times the folded weights (one paired GEMM, N = 2 C);
 * ukq [2, C]; bias [C] = bp + Wp bv.  q, k, v and o are never formed and no C x C weight is read.  Two workgroups per CU;
 * diffsal_set_tuning("DIFFSAL_FRONT_FOLD_WGS", 1) selects the one-workgroup form with a next-tile look-ahead (bit-equal results). */
int diffsal_block_front_fold(const float* x, const float* G, const float* U, const float* kp, const float* ukq, const float* g1,
                             const float* b1, float eps1, const float* w9, const float* gq, const float* bq, float epsq,
                             const float* bias, float* out, int N, int H, int W, int C, int Lk, int heads, float scale,
                             diffsal_stream_t stream);

/* ---- storage-type conversion: dst[i] = (dst type) src[i], round to nearest even.  Used once per parameter version to
 * put packed convolution / linear weights into the 16-bit storage type of a reduced-precision module (the reference
 * has no counterpart: it is fp32-only, R/diffusion_trainer.py:212-218). */
int diffsal_cast(const void* src, int src_dtype, void* dst, int dst_dtype, long n, diffsal_stream_t stream);

/* ==== once-per-clip encoders around the denoiser =======================================================
 * ---- general softmax attention on the fp32 matrix cores (flash-style, one pass over the keys) -------------------------
 * out[b, l, h*DV + :] = softmax_t( scale * q[b,h,l,:] . k[b,h,t,:]  +  q_extra[b,h,l,:] . k_extra[t,:] ) v[b,h,t,:]
 *                       (+ residual[b,h,l,:], not on row 0 if skip_first)
 * q / k / v / residual are addressed through (batch, head, row) element strides, so slices of a fused qkv GEMM output
 * are read in place; q_extra [B,H,Lq,E] and k_extra [Lk,E] are contiguous and carry an additive attention bias as E
 * extra contraction columns (MViT: E = 48 or 32, see diffsal_relpos_project; otherwise E = 0 and both are NULL).
 * k_slots (optional, E > 0): the slot form of a ONE-HOT k_extra -- k_slots[t][0..2] = the columns of row t that are 1 (E = none, e.g. the
 * class token; [3] unused), 16-byte aligned.  With it the bias is three gathered q_extra values per (query, key) added on the vector unit
 * and the E extra contraction columns are not multiplied (a fifth fewer matrix instructions at E = 48); k_extra must still describe the
 * same matrix (the backward contracts with it).  The result differs from the contraction form by summation order only.
 * Built (D, E, DV): (96,48,96), (96,32,96), (96,0,96), (64,0,64), (32,0,32).  Replaces
 *   R/models/mvit.py:587-605 (MultiScaleAttention: attn = (q*scale) k^T, add_decomposed_rel_pos, softmax, attn v, + q),
 *   R/models/audio_attention.py:50-58 (dots, softmax, out). */
int diffsal_attention_general(const float* q, const float* q_extra, const float* k, const float* k_extra,
                              const int* k_slots /*[Lk][4] or NULL*/, const float* v, const float* residual, float* out, float* lse /*[B,H,Lq] row log-sum-exp, or NULL*/, int B,
                              int H, int Lq, int Lk, int D, int E, int DV, const long* q_strides /*host [3]*/,
                              const long* k_strides, const long* v_strides, const long* r_strides, float scale,
                              int skip_first, float* tail_ws, size_t tail_ws_floats, diffsal_stream_t stream);
/* tail_ws (optional): tail_ws_floats >= diffsal_attention_general_tail_floats(...) floats (a smaller buffer is ignored).  With it the blocks of the last, partly filled
 * round of workgroups are cut into pieces over the keys and a finishing launch merges the pieces' outputs by their
 * log-sum-exps; without it (NULL, or the function returned 0) every block runs whole. */
size_t diffsal_attention_general_tail_floats(int B, int H, int Lq, int Lk, int DV);
/* Backward (training of the encoders): P is recomputed from `lse`; delta_ws [B,H,Lq] is scratch.  Outputs are contiguous
 * head-major tensors: dq [B,H,Lq,D] (includes the residual path's dO when `residual` was given), dq_extra [B,H,Lq,E]
 * (NULL iff E == 0), dk [B,H,Lk,D], dv [B,H,Lk,DV]; k_extra is a constant table and gets no gradient.  No atomics. */
int diffsal_attention_general_bwd_splits(int B, int H, int Lq, int Lk); /* S; kv_part_ws needs S*B*H*Lk*(D+DV) floats if S > 1 */
/* q_tail_ws (optional): q_tail_ws_floats >= diffsal_attention_general_bwd_qtail_floats(...) floats (a smaller buffer is ignored).  With it the dq kernel cuts the blocks of its
 * last, partly filled round of workgroups into pieces over the keys and a finishing launch adds their partial rows (fixed
 * order); without it (NULL, or the function returned 0) every block runs whole. */
size_t diffsal_attention_general_bwd_qtail_floats(int B, int H, int Lq, int Lk, int D, int E);
/* ds_ws (optional): ds_ws_floats >= diffsal_attention_general_bwd_ds_floats(...) floats (NULL or a smaller buffer: ignored).  With it the dk / dv kernel leaves
 * dS [B*H][Lq][Lk rounded up to 32] there and dq is the one product dS K' (five tile products per query / key tile pair instead of seven: the recomputation of
 * S and dP in the dq kernel is traded for one write and one read of dS); same sums in the same order, dq bit-identical to the recomputing form. */
size_t diffsal_attention_general_bwd_ds_floats(int B, int H, int Lq, int Lk);
int diffsal_attention_general_bwd(const float* q, const float* q_extra, const float* k, const float* k_extra, const float* v,
                                  const float* residual, const float* out, const float* lse, const float* dout,
                                  float* delta_ws, float* kv_part_ws, float* q_tail_ws, size_t q_tail_ws_floats, float* ds_ws,
                                  size_t ds_ws_floats, float* dq, float* dq_extra, float* dk, float* dv, int B, int H, int Lq,
                                  int Lk, int D, int E, int DV, const long* q_strides, const long* k_strides,
                                  const long* v_strides, const long* r_strides, float scale, int skip_first,
                                  diffsal_stream_t stream);

/* ---- MViTv2 pieces that are not GEMMs / LayerNorms (R/models/mvit.py) -------------------------------------------------
 * im2col3d: columns of PatchEmbed3D's Conv3d (mvit.py:157-163, 983-989): x [B,C,T,H,W] -> cols [B*To*Ho*Wo][Kp],
 *   k = (c, kt, ky, kx) as in weight.reshape(Cout, -1), zero-padded to Kp (multiple of 32); the projection is one GEMM.
 * pool3d_ln: attention_pool (mvit.py:446-494): depthwise Conv3d 3x3x3 pad 1 stride (st,sh,sw) over the video tokens of
 *   every head + LayerNorm(D); class token (row 0) skips the conv.  in element (b, n, head, d) at
 *   in + b*in_stride_b + n*in_stride_n + head*D + d; w27 [27][D]; out [B, heads, 1 + To*Ho*Wo, D].
 * maxpool_tokens: the skip path's MaxPool3d (mvit.py:765-777) on tokens [B, 1+T*H*W, C], padding k/2, class token kept.
 * relpos_project: per query the E bias columns of add_decomposed_rel_pos (mvit.py:363-410), E = 48 or 32:
 *   E = 48: [0,kt) q.Rt[t], [8,8+kh) q.Rh[y], [24,24+kw) q.Rw[x]   (kt <= 8, kh <= 16, kw <= 24)
 *   E = 32: [0,kt) q.Rt[t], [8,8+kh) q.Rh[y], [16,16+kw) q.Rw[x]   (kt <= 8, kh <= 8, kw <= 16: every MViTv2-S stage at 224x384)
 *   rest 0, class-token row 0; Rt [qt][kt][D] etc. are the gathered tables (resize_decomposed_rel_pos, :330-361);
 *   q [BH, 1+qt*qh*qw, D] unscaled.  The key side of diffsal_attention_general carries one-hot rows in the same layout.
 * tokens_to_channels_first: [B, off+L, C] rows off.. -> [B, C, L] (the NCTHW maps MViT returns, :1128-1134). */
int diffsal_im2col3d(const float* x, float* cols, int B, int C, int T, int H, int W, int KT, int KH, int KW, int st, int sh,
                     int sw, int pt, int ph, int pw, int Kp, diffsal_stream_t stream);
int diffsal_pool3d_ln(const float* in, const float* w27, const float* gamma, const float* beta, float* out, int B, int heads,
                      int D, int T, int H, int W, int st, int sh, int sw, long in_stride_b, long in_stride_n, float eps,
                      diffsal_stream_t stream);
int diffsal_maxpool_tokens(const float* in, float* out, int B, int C, int T, int H, int W, int kt, int kh, int kw, int st,
                           int sh, int sw, diffsal_stream_t stream);
int diffsal_relpos_project(const float* q, const float* Rt, const float* Rh, const float* Rw, float* extra, int BH, int D,
                           int qt, int qh, int qw, int kt, int kh, int kw, int E, diffsal_stream_t stream);
int diffsal_tokens_to_channels_first(const float* in, float* out, int B, int C, int L, int off, diffsal_stream_t stream);
/* Training of the video encoder: backward of the pieces above (all gather form, no atomics, fixed summation order).
 * pool3d_ln with gamma = beta = NULL is the convolution alone (its LayerNorm then runs as diffsal_layernorm).
 * pool3d_bwd_data writes d_in through the forward input's strides (straight into the q / k / v slice of the qkv gradient);
 * pool3d_bwd_weight leaves part[chunks][27][D] doubles (chunks = diffsal_pool3d_bwd_weight_chunks()) for
 * diffsal_reduce_partials.  maxpool_tokens_idx also records the arg-max token (first maximum in (t,y,x) order, as
 * torch.nn.MaxPool3d); maxpool_tokens_bwd routes dy back through it.  relpos_project_bwd: dq (+)= dextra . R and per-chunk
 * partials of the three table gradients (chunks = diffsal_relpos_project_bwd_chunks(); finish with
 * diffsal_reduce_partials(part, out, 1, chunks, width, 0) -> dRt | dRh | dRw back to back). */
int diffsal_pool3d_bwd_data(const float* dy, const float* w27, float* din, int B, int heads, int D, int T, int H, int W, int st,
                            int sh, int sw, long in_stride_b, long in_stride_n, diffsal_stream_t stream);
int diffsal_pool3d_bwd_weight_chunks(void);
int diffsal_pool3d_bwd_weight(const float* in, const float* dy, double* part, int B, int heads, int D, int T, int H, int W,
                              int st, int sh, int sw, long in_stride_b, long in_stride_n, diffsal_stream_t stream);
int diffsal_maxpool_tokens_idx(const float* in, float* out, int* idx, int B, int C, int T, int H, int W, int kt, int kh, int kw,
                               int st, int sh, int sw, diffsal_stream_t stream);
int diffsal_maxpool_tokens_bwd(const float* dy, const int* idx, float* din, int B, int C, int T, int H, int W, int kt, int kh,
                               int kw, int st, int sh, int sw, diffsal_stream_t stream);
/* qkv_pool: the three attention_pool convolutions of one block in ONE launch, head dimension D = 96 (mvit.py:446-494, called
 * three times per block at :556-590): qkv is the fused projection [B][1+T*H*W][3][heads][96]; w27 / gamma / beta / eps / out
 * are arrays of three (q, k, v); gamma = beta = eps = NULL: convolutions only.  out[x]: [B*heads][1 + To*Ho*Wo][96] with the
 * strides of q (stride_q[3]) or of k and v (stride_kv[3]).  Bit-identical to three diffsal_pool3d_ln calls in the convolution;
 * the LayerNorm sums run over 8 lanes x 12 channels instead of 32 x 4.
 * qkv_pool_bwd_data: every element of dqkv [B][N][3][heads][96] from the three output gradients (temporal stride 1, equal
 * spatial strides); bit-identical to three diffsal_pool3d_bwd_data calls. */
int diffsal_qkv_pool(const void* qkv, const float* const* w27, const float* const* gamma, const float* const* beta,
                     const float* eps, float* const* out, int B, int heads, int D, int T, int H, int W, const int* stride_q,
                     const int* stride_kv, int dtype /* storage type of qkv; outputs are fp32 */,
                     int w_channel_major /* 1: filters in the parameter's [96][27] layout, 0: tap-major [27][96] */,
                     diffsal_stream_t stream);
int diffsal_qkv_pool_bwd_data(const float* const* dy, const float* const* w27, float* dqkv, int B, int heads, int D, int T,
                              int H, int W, const int* stride_q, const int* stride_kv, int w_channel_major,
                              diffsal_stream_t stream);
/* qkv_pool_bwd_weight: the three filter gradients in one launch: part[3][chunks][27*96] doubles (chunks =
 * diffsal_qkv_pool_bwd_weight_chunks(B, heads, T, H, W, stride_q): 512, or 170 on small stages), finished by diffsal_reduce_partials(part, out, 3, chunks, 27*96, 0). */
int diffsal_qkv_pool_bwd_weight_chunks(int B, int heads, int T, int H, int W, const int* stride_q);
int diffsal_qkv_pool_bwd_weight(const float* qkv, const float* const* dy, double* part, int B, int heads, int D, int T, int H,
                                int W, const int* stride_q, const int* stride_kv, int w_channel_major /* layout of each [27*96] row */,
                                diffsal_stream_t stream);
/* rel_tables: the three gathered relative-position tables of a block (resize_decomposed_rel_pos, mvit.py:330-361) as sparse
 * row maps built once per grid on the host: out_t[m] = w2_t[m][0] * rel_t[idx2_t[m][0]] + w2_t[m][1] * rel_t[idx2_t[m][1]],
 * m < M[t]; arrays of three (t, h, w).  rel_tables_bwd applies the transposed maps in CSR form (row starts [R[t] + 1],
 * columns = m, weights): drel_t[r] = sum of w * dout_t[m] in CSR order. */
int diffsal_rel_tables(const float* const* rel, const int* const* idx2, const float* const* w2, float* const* out, const int* M,
                       int D, diffsal_stream_t stream);
int diffsal_rel_tables_bwd(const float* const* dout, const int* const* csr_ptr, const int* const* csr_col,
                           const float* const* csr_w, float* const* drel, const int* R, int D, diffsal_stream_t stream);
int diffsal_relpos_project_bwd_chunks(void);
int diffsal_relpos_project_bwd(const float* dextra, const float* q, const float* Rt, const float* Rh, const float* Rw, float* dq,
                               int accumulate, double* part /*[chunks][(qt*kt + qh*kh + qw*kw) * D]: dRt | dRh | dRw partials*/,
                               int BH, int D, int qt, int qh, int qw, int kt, int kh, int kw, int E, diffsal_stream_t stream);

/* ---- legacy DDPM-style UNet of R/models/diffusion_decoder/diffusion.py (DiffusionModel :197-357; not instantiated by
 * any configuration of the reference, kept for completeness of the models/diffusion_decoder surface), fp32 NHWC.  Its
 * ResnetBlocks / Downsample / conv_out reuse diffsal_conv_igemm and K3; what it adds:
 *   groupnorm         GroupNorm with the activation optional (act 0: AttnBlock.norm :145,173; act 1 == groupnorm_swish)
 *   softmax_rows      out[r,:] = softmax(scale * x[r,:]) over the HW keys of the full self-attention (:166-168); the two
 *                     products around it are diffsal_conv_igemm calls with k / v^T of one image as the weight operand
 *   upsample_nearest2 Upsample :46-47;  avgpool2: Downsample without conv :69;  sigmoid_gate: feat_interact :318 */
int diffsal_groupnorm(const void* x, const float* gamma, const float* beta, void* out, int B, int HW, int C, int groups,
                      float eps, int act, void* ws, size_t ws_bytes, int dtype, diffsal_stream_t stream);
int diffsal_softmax_rows(const float* x, float* out, long rows, int cols, float scale, diffsal_stream_t stream);
int diffsal_upsample_nearest2(const float* in, float* out, int N, int H, int W, int C, diffsal_stream_t stream);
int diffsal_avgpool2(const float* in, float* out, int N, int H, int W, int C, diffsal_stream_t stream);
int diffsal_sigmoid_gate(const float* y, const float* x, float* out, long n, diffsal_stream_t stream);

/* ---- VGGish feature stack (R/models/vggish.py:70-106): 3x3 convs are diffsal_conv_in (1 input channel, act = ReLU) and
 * diffsal_conv_igemm (bias + ReLU epilogue); this is its MaxPool2d(k, stride) on NHWC (no padding, floor). */
int diffsal_maxpool2d(const void* in, void* out, int N, int H, int W, int C, int k, int stride, int dtype,
                      diffsal_stream_t stream);

/* ---- evaluation metrics on the device: CC, SIM, NSS, KL-div of predicted vs ground-truth saliency maps -----------
 * R/models/sal_losses.py:14-37 (nss2), :63-97 (cc_s2), :100-131 (kldiv2), :134-176 (normalize_map2, similarity2), as
 * called per validation batch by get_kl_cc_sim_loss_wo_weight (R/diffusion_trainer.py:741,797,868).
 * pred, gt: [B][n] fp32 (n = T*H*W values per image).  per_image (optional): [B][4] = (cc, sim, nss, kl);
 * mean_out: [4] batch means in the same order (what the reference functions return).  Two streaming passes, fp64
 * accumulation in a fixed order; ws >= diffsal_saliency_metrics_ws_bytes(B) bytes. */
size_t diffsal_saliency_metrics_ws_bytes(int B);
/* Training: gradient of  w_cc CC + w_sim SIM + w_nss NSS + w_kl KL  (the four batch means above) with respect to pred, from the
 * workspace the forward call left behind; weights4 = four floats on the device (upstream gradients x the configuration's loss
 * weights).  The differentiable terms of get_kl_cc_sim_loss / get_lossv2 (R/models/sal_losses.py:179-259). */
int diffsal_saliency_metrics_bwd(const float* pred, const float* gt, int B, long n, const void* ws, size_t ws_bytes,
                                 const float* weights4, float* dpred, diffsal_stream_t stream);
int diffsal_saliency_metrics(const float* pred, const float* gt, int B, long n, void* ws, size_t ws_bytes,
                             float* per_image, float* mean_out, diffsal_stream_t stream);

/* ---- benchmark metrics on the device: AUC-Judd, AUC-Borji, shuffled AUC, CC, NSS, SIM per image -----------
 * R/metrics/metrics.py:7-252 (same-shape case; resizing a prediction to the fixation map's resolution is diffsal_map_resize's, below), which
 * R/compute_metrics.py runs on PNG files in a pool of numpy processes.  pred [B][n] fp32 (n = H*W), fix [B][n] bytes (a pixel is
 * fixated iff its byte is non-zero), gt [B][n] fp32 (CC, SIM), other [B][n] bytes (sAUC: fixations of other images).
 * terms = sum of DIFFSAL_EVAL_*; out [6][B] fp64, row r = (judd, borji, sauc, cc, nss, sim)[r]; rows not asked for are left alone.
 *   S = (s - min) / (max - min) in fp32, one subtraction and one IEEE division (R/metrics/utils.py:47 on a float32 map, bit for
 *   bit); values that collapse to one float are ties.
 *   judd   above_i = #{j : S_j >= S_i} per fixated pixel i; k = i's position in the descending order of the fixation values
 *          (equal values consecutive); ROC points (0,0), ((above - k - 1) / (n - n_fix), (k + 1) / n_fix), (1,1); fp64 trapezoids
 *   borji  n_rep repetitions; thresholds k * step (fp64, k < ceil(max / step), max over the fixation values and the repetition's
 *          sampled values: numpy's arange length rule), compared in fp64; tp over the fixation values, fp over the sampled
 *          values, both / n_fix; one trapezoid sum per repetition, their mean in index order.  ceil(1 / step) <= 1024
 *   sauc   the same with the sampled locations taken from the fixated pixels of `other`
 *   cc     Pearson coefficient of pred and gt;  nss  mean over fixated pixels of (s - mean) / std, population std;
 *   sim    sum of min of the two maps after range, then sum normalisation -- all three in fp64 from the fp32 inputs
 * Sampled locations: rand_borji / rand_sauc [B][n_rep][cap] int32, -1 = unused slot (out-of-range entries are ignored), or NULL
 * for the device generator: Philox4x32-10, key and counter exactly as in "sampler noise" below, with
 *   id    = a caller-supplied non-negative 64-bit IMAGE id (ids [B], seed [1]: device memory, as there)
 *   draw  = 0x40000000 | purpose      bit 30 keeps evaluation apart from the sampler's draws 0, 1, 2, ... and the trainer's
 *                                     bit-31 draws under one seed
 *   purpose 0 jitter (DIFFSAL_EVAL_JITTER, metrics.py:44-45): element p (pixel index): s' = float(double(s) + u * 1e-7),
 *             u = (word >> 8) * 2^-24; the range normalisation then uses min / max of s'.  Judd only: a call with the jitter
 *             bit may not ask for borji / sauc (the reference does not jitter them)
 *   purpose 1 borji: element p * n_rep + rep, p = linear index of a fixated pixel -> location (uint64(word) * n) >> 32
 *   purpose 2 sauc:  element p * n_rep + rep, p = a fixated pixel of `other`, is that pixel's key for the repetition; the
 *             repetition uses the min(n_fix, n_other) pixels with the smallest (word, p) pairs (sampling without replacement,
 *             as the reference's permutation prefix)
 *   element e is word e % 4 of the call with q = e / 4; n * n_rep <= 2^34.
 * Deliberate definitions where the reference returns NaN or divides by zero: an image with no fixation, with every pixel
 * fixated or with a flat map (max == min) gets NaN in judd, borji, sauc and nss (sauc also when `other` has no fixation); cc
 * and sim are set to NaN for a flat pred or gt (the reference's 0 / 0; the kernel writes the NaN itself, since the fmin of the
 * SIM sum would drop it).  Such an image does not disturb the others of the batch.
 * Cost: judd makes n_fix * n compares and n_fix^2 rank compares per image; it is meant for eye-tracking maps with n_fix from a
 * few to a few thousand.  Denser maps give correct results at a cost that grows to O(n^2) per image (seconds at 360 x 640).
 * Integer counts and fixed-order fp64 sums: results are bit-reproducible.  ws >= diffsal_eval_metrics_ws_bytes(B, n, terms,
 * n_rep) bytes for the same terms (n_rep is ignored without borji / sauc), 16-byte aligned: cc / nss / sim need a few KB; judd,
 * borji and sauc need [B][n] 4-byte arrays (the normalised map, the fixation lists, the counts: 4, 3, 3 of them, 6 when all
 * three are asked for, i.e. 24 B n bytes, 354 MB at B = 64, 360 x 640).  No allocation, no synchronisation, graph-safe. */
#define DIFFSAL_EVAL_JUDD 1u
#define DIFFSAL_EVAL_BORJI 2u
#define DIFFSAL_EVAL_SAUC 4u
#define DIFFSAL_EVAL_CC 8u
#define DIFFSAL_EVAL_NSS 16u
#define DIFFSAL_EVAL_SIM 32u
#define DIFFSAL_EVAL_JITTER 64u
size_t diffsal_eval_metrics_ws_bytes(int B, long n, unsigned int terms, int n_rep);
int diffsal_eval_metrics(const float* pred, const unsigned char* fix, const float* gt, const unsigned char* other, int B, long n,
                         unsigned int terms, int n_rep, double step, const int* rand_borji, const int* rand_sauc, int cap,
                         const long long* ids, const unsigned long long* seed, void* ws, size_t ws_bytes, double* out,
                         diffsal_stream_t stream);

/* ---- benchmark post-processing: the 8-bit export and the spline resize to the annotation's resolution -----------
 * What stands between the sampler's fp32 map and the map R/metrics/metrics.py scores: R/diffusion_trainer.py:898-935 quantises
 * each prediction with normalize_data (R/util/utils.py:11-16) and writes a PNG; R/compute_metrics.py:9-26 reads it back with
 * plt.imread (float32 = byte / 255); R/metrics/metrics.py:41-42,102-103,195-196,218-219,243-244 resizes that map to the
 * annotation's shape with skimage `resize`: order=3, mode='reflect' for the AUCs, CC and SIM, the default order=1 for NSS.
 *
 * diffsal_map_to_u8: pred [B][n] fp32 (n = h*w) -> u8 [B][n] bytes and / or f [B][n] fp32 (either may be NULL, not both).  Per
 * image, in fp32, normalize_data bit for bit:
 *   mn, mx = min, max of the image;  s = fl32(255 / fl32(mx - mn))  (one IEEE division)
 *   q = (uint8) trunc(clamp(fl32(fl32(x - mn) * s), 0, 255));  f = fl32(q / 255)  (one IEEE division: imread of an 8-bit PNG)
 * Deliberate definition: a flat image (mx == mn; the reference divides by zero there) gives q = 0 everywhere.  A NaN in the
 * input is the caller's error and the result is then undefined.  ws >= diffsal_map_to_u8_ws_bytes(B, n) bytes, 16-byte aligned.
 * diffsal_map_from_u8: f[i] = fl32(u8[i] / 255) for `total` elements.
 *
 * diffsal_map_resize: in [B][h][w] fp32 -> out [B][H][W], fp32 (out_f64 = 0) or fp64 (out_f64 = 1: the same arithmetic before
 * its last rounding, for tests).  All arithmetic is fp64 from the fp32 inputs; the fp32 store is a single round-to-nearest.
 *   position per axis  x = (o + 0.5) * (n / N) - 0.5                      scipy.ndimage.zoom's grid_mode=True
 *   boundary           whole-sample mirror extension, period 2(n - 1):    j %= 2(n-1); if j > n-1: j = 2(n-1) - j
 *                      (scipy mode='mirror' = numpy.pad 'reflect' = what skimage's mode='reflect' means)
 *   order 1            linear between floor(x) and floor(x) + 1, separable
 *   order 3            interpolating cubic B-spline: coefficients c with (c[i-1] + 4 c[i] + c[i+1]) / 6 = s[i] per axis under
 *                      the same boundary, computed as c[i] = sqrt(3) * sum_{|k| <= 34} z^|k| s[mirror(i + k)], z = sqrt(3) - 2
 *                      (|z|^34 < 2^-64), x axis first; then out = sum_{k = f-1 .. f+2} beta3(x - k) c[mirror(k)] per axis,
 *                      f = floor(x), beta3(t) = (4 - 6 t^2 + 3 |t|^3) / 6 for |t| < 1, (2 - |t|)^3 / 6 for |t| < 2, else 0
 *                      (evaluated as 6 beta3 per axis and one division of the pixel's sum by 36)
 *   clip = 1           each output image is clamped to [min, max] of its own input image (skimage's clip=True default; the
 *                      cubic overshoots)
 * This is scipy.ndimage.zoom(in, (H/h, W/w), order=order, mode='mirror', grid_mode=True), which skimage (>= 0.19) runs for an
 * upscale before it clips.  An output axis shorter than the input is DIFFSAL_E_SHAPE (skimage adds an anti-aliasing Gaussian
 * there: diffsal_map_resize_aa, below), so is an input axis shorter than 2 or any axis above 32768; equal length is allowed (the same formula).
 * order other than 1 or 3: DIFFSAL_E_ARG.  All argument checks precede the first launch.
 * ws >= diffsal_map_resize_ws_bytes(B, h, w, order, clip) bytes, 16-byte aligned: order 3 keeps two [B][h][w] fp64 arrays
 * (88 MB at B = 64, 224 x 384), clip a few KB; order 1 without clip needs none (ws may be NULL).
 * min / max are exact and every sum has a fixed order: results are bit-reproducible and an image's result does not depend on
 * the batch it is in.  No floating-point atomics, no allocation, no synchronisation, graph-safe.
 *
 * diffsal_map_resize_aa: the same resize at ANY target size H, W >= 1, with the anti-aliasing Gaussian skimage (>= 0.19, its
 * default anti_aliasing rule) runs over the map first on every axis that shrinks.  For a target (H, W) with H < h or W < w:
 *   sigma    = (max(0, (h / H - 1) / 2), max(0, (w / W - 1) / 2))
 *   filtered = scipy.ndimage.gaussian_filter(in, sigma, mode='mirror')          fp32 in, fp32 out
 *   out      = scipy.ndimage.zoom(filtered, (H / h, W / w), order=order, mode='mirror', grid_mode=True)
 *   clip = 1   clamps to [min, max] of the UNFILTERED in
 * The caller computes the weights on the host and passes them: wy / wx point at ry + 1 / rx + 1 doubles in HOST memory, centre
 * first; they are copied into the launches' arguments (no device allocation, no copy: graph-safe).  Per axis with sigma > 1e-15
 *   r = int(4 sigma + 0.5);  g[k] = exp(-0.5 / sigma^2 * k^2), k = -r .. r, in fp64 with numpy.exp, divided by their sum
 * (diff_sal_amd.postprocess.gaussian_weights; one ulp in a weight changes output bits).  A radius of 0 means no pass on that axis
 * (the pointer is then not read and may be NULL); a radius above 64 (sigma >= 16, a factor of 33) is DIFFSAL_E_SHAPE.
 * One output sample of a pass, in fp64 with every operation rounded on its own (no fused multiply-add), then ONE rounding to fp32:
 *   acc = x[i] * g[0];  for k = r, r - 1, ..., 1:  acc = acc + (x[mirror(i - k)] + x[mirror(i + k)]) * g[k]
 * with the mirror of diffsal_map_resize (folded as often as r > n - 1 needs).  Axis 0 (rows) first; the pass along axis 1 reads
 * the fp32 result of the first.  This is scipy's correlate1d for a symmetric kernel, operation for operation: the filtered map
 * is bit-equal to scipy 1.15's.  With both radii 0 the result is diffsal_map_resize's bit for bit where that function takes the
 * shape.  Other checks as diffsal_map_resize (source axes 2..32768, target axes 1..32768), all before the first launch.
 * ws >= diffsal_map_resize_aa_ws_bytes(B, h, w, order, clip) bytes, 16-byte aligned, never NULL: diffsal_map_resize's layout plus
 * two [B][h][w] fp32 arrays.
 * diffsal_map_gauss: the Gaussian stage alone, in [B][h][w] fp32 -> out [B][h][w] fp32 (out != in; both radii 0: a copy).
 * ws >= diffsal_map_gauss_ws_bytes(B, h, w) bytes (one [B][h][w] fp32 array), read only when both radii are above 0. */
size_t diffsal_map_to_u8_ws_bytes(int B, long n);
int diffsal_map_to_u8(const float* pred, int B, long n, unsigned char* u8, float* f, void* ws, size_t ws_bytes,
                      diffsal_stream_t stream);
int diffsal_map_from_u8(const unsigned char* u8, long total, float* f, diffsal_stream_t stream);
size_t diffsal_map_resize_ws_bytes(int B, int h, int w, int order, int clip);
int diffsal_map_resize(const float* in, int B, int h, int w, int H, int W, int order, int clip, int out_f64, void* out, void* ws,
                       size_t ws_bytes, diffsal_stream_t stream);
size_t diffsal_map_resize_aa_ws_bytes(int B, int h, int w, int order, int clip);
int diffsal_map_resize_aa(const float* in, int B, int h, int w, int H, int W, int order, int clip, int out_f64, const double* wy,
                          int ry, const double* wx, int rx, void* out, void* ws, size_t ws_bytes, diffsal_stream_t stream);
size_t diffsal_map_gauss_ws_bytes(int B, int h, int w);
int diffsal_map_gauss(const float* in, int B, int h, int w, const double* wy, int ry, const double* wx, int rx, float* out, void* ws,
                      size_t ws_bytes, diffsal_stream_t stream);

/* ---- JPEG export: the 8-bit maps of the audio-visual sets -> the files the reference writes, and what it reads back -----------
 * For AVAD, Coutrot, DIEM, ETMD and SumMe R/diffusion_trainer.py:898-935 (save_img, av_data=True) writes pred_sal_%06d.jpg with
 * cv2.imwrite: 8-bit greyscale, baseline, quality 95, libjpeg's default slow-integer DCT, the standard tables.  Every step is
 * integer arithmetic; in = the bytes of diffsal_map_to_u8, [B][h][w], 1 <= h, w <= 65535, quality 1..100.
 *   geometry     8 x 8 blocks in raster order; the image is padded to multiples of 8 by repeating its last column, then its last row
 *   table        s = 5000 / q for q < 50, else 200 - 2 q;  t[k] = clamp((base[k] * s + 50) / 100, 1, 255), integer divisions;
 *                base = ITU-T T.81 Annex K.1 (luminance).  Quality 95: first row 2 1 1 2 2 4 5 6
 *   forward DCT  libjpeg's jfdctint on sample - 128: CONST_BITS = 13, PASS1_BITS = 2, rows (outputs 0 and 4 times 4, the others
 *                descaled by 11) then columns (outputs 0 and 4 descaled by 2, the others by 15), 32-bit integers,
 *                DESCALE(x, n) = (x + (1 << (n - 1))) >> n, constants 2446 3196 4433 6270 7373 9633 12299 15137 16069 16819 20995
 *                25172 (FIX(0.298631336) .. FIX(3.072711026)); the result carries a factor 8
 *   quantiser    d = 8 t[k];  |c| <- (|c| + d / 2) / d, the sign put back
 *   entropy      zig-zag order; DC as the difference from the block before it in the same image (0 before the first); Annex K.3
 *                luminance DC and AC codes; ZRL (F0) for every 16 zeros of a run, EOB (00) when the block ends in zeros; a value
 *                of category n is its low n bits, v - 1 for a negative v
 *   bit stream   MSB first; the last byte filled with 1-bits; 00 behind every FF byte, a filled last byte included
 *   file         SOI; APP0 JFIF 1.01, units 0, density 1 x 1, no thumbnail; DQT (table 0, 8-bit, zig-zag); SOF0 precision 8, h, w,
 *                one component 01 11 00; DHT class 0 id 0; DHT class 1 id 0; SOS 01 01 00 00 3F 00; the scan; EOI.  328 bytes
 *                stand in front of the scan.  Byte for byte what Pillow's Image.fromarray(u8).save(f, "JPEG", quality=q) writes.
 *   read-back    coefficient times t[k]; libjpeg's jidctint, columns (descale 11) then rows (descale 18); libjpeg's range limit:
 *                x + 128 clamped to 0..255, taken from a table indexed by the low 10 bits of x (the plain clamp for
 *                -512 <= x <= 511)
 * diffsal_jpeg_roundtrip: recon [B][h][w] = the read-back pixels, one launch, no workspace and no entropy coder: what scoring needs.
 * diffsal_jpeg_encode: out [B][cap] bytes, cap >= diffsal_jpeg_capacity(h, w); image b's file is out[b][0 .. lengths[b]), the
 * bytes behind it are undefined; recon as above or NULL; ws >= diffsal_jpeg_encode_ws_bytes(B, h, w) bytes, 16-byte aligned.
 * Capacity is a bound, not an estimate: a block codes to at most (9 + 11) + 63 * (16 + 10) = 1658 bits (the categories are capped
 * at 11 and 10, which no 8-bit image reaches), so with nblk = ceil(h / 8) * ceil(w / 8) and m = ceil(1658 nblk / 8)
 *   diffsal_jpeg_capacity(h, w) = 328 + 2 m + 2 + 2      (every scan byte stuffed, EOI, two spare)
 * and the workspace holds int16 [B][64][nblk] coefficients, per block a 32-bit AC bit count and a 64-bit bit offset, the bit
 * stream of ceil(m / 4) 32-bit words per image and two 32-bit counts per 2048 stream bytes.  No kernel writes outside out[b][0 .. cap)
 * or the workspace for any input bytes.  An image whose capacity passes 2^31 - 1 is DIFFSAL_E_SHAPE for encode (lengths are int32).
 * Launches of encode: a clear of the bit stream (hipMemsetAsync on `stream`, every call), block transform, bit offsets (exclusive
 * scan per image), pack (integer atomicOr into the shared words: order-independent), FF count, frame (scan of the counts, header,
 * EOI, length), stuff.  Results are bit-reproducible and an image's bytes do not depend on the batch it is in.  No allocation, no
 * synchronisation, no host copy, graph-safe; all argument checks precede the first launch. */
long diffsal_jpeg_capacity(int h, int w);      /* 0: bad argument */
size_t diffsal_jpeg_encode_ws_bytes(int B, int h, int w);
int diffsal_jpeg_encode(const unsigned char* u8, int B, int h, int w, int quality, unsigned char* out, long cap, int* lengths,
                        unsigned char* recon, void* ws, size_t ws_bytes, diffsal_stream_t stream);
int diffsal_jpeg_roundtrip(const unsigned char* u8, int B, int h, int w, int quality, unsigned char* recon,
                           diffsal_stream_t stream);

/* ---- JPEG decode: the frame files of the audio-visual sets -> the uint8 frames Pillow returns -----------
 * R/datasets/saliency_db.py:29-44 decodes img_%05d.jpg with Image.open(f).convert('RGB') (pil_loader) and eyeMap_%05d.jpg with
 * .convert('L') (pil_loader_sal).  Pillow's decoder is libjpeg-turbo with its defaults; every step is integer arithmetic, and the
 * result here is bit-equal.  Baseline sequential files only: 8-bit, one component or three read as YCbCr, luma sampling 1x1, 2x1
 * or 2x2 with chroma 1x1, one interleaved scan; everything else is refused by the caller's parser before a launch.
 *   (a) entropy   T.81 F.2: codes assigned in order of length (Annex C); DC is a difference from the previous block of the same
 *                 component, the predictor 0 at the scan start and behind every restart marker; EXTEND(v, n) = v for
 *                 v >= 2^(n-1), else v - 2^n + 1; AC symbol F0 (ZRL) skips 16 coefficients, 00 (EOB) ends the block; coefficient
 *                 k of the zig-zag order is stored in natural order; FF 00 in the scan is the byte FF; MCUs in raster order, an
 *                 MCU holds hs * vs luma blocks, rows first, then one block per chroma component; sizes are padded to whole MCUs
 *   (b) dequantise   coefficient times table entry, natural order
 *   (c) transform    the read-back of "JPEG export": libjpeg's jidctint (columns descale 11, rows descale 18) and range limit, in
 *                    32-bit wrap-around arithmetic (the bits of the int arithmetic wherever that does not overflow)
 *   (d) chroma    cw = ceil(W / hs), ch = ceil(H / vs): a chroma plane's real size; samples beyond it are never read.
 *                 hs = 1: none.  cw <= 2: every sample replicated hs x vs times (libjpeg leaves the fancy filters out).
 *                 2x1, cw > 2:  out[2i] = (3 x[i] + x[i-1] + 1) >> 2,  out[2i+1] = (3 x[i] + x[i+1] + 2) >> 2; the first output
 *                 column is x[0], the last (2 cw - 1) is x[cw-1].
 *                 2x2, cw > 2:  rows first, unrounded: r[2j] = 3 x[j] + x[j-1], r[2j+1] = 3 x[j] + x[j+1], the neighbour's row index
 *                 clamped to 0 .. ch-1; then out[2i] = (3 r[i] + r[i-1] + 8) >> 4, out[2i+1] = (3 r[i] + r[i+1] + 7) >> 4; the
 *                 first output column is (4 r[0] + 8) >> 4, the last (4 r[cw-1] + 7) >> 4.  The output is cropped to H x W.
 *   (e) colour    with cb, cr minus 128 and arithmetic shifts:  R = y + ((91881 cr + 32768) >> 16),
 *                 G = y + ((-22554 cb - 46802 cr + 32768) >> 16),  B = y + ((116130 cb + 32768) >> 16), each clamped to 0..255;
 *                 one component: R = G = B = y
 *   (f) L         one component: y.  Three: (19595 R + 38470 G + 7471 B + 32768) >> 16 of (e)'s RGB (Pillow's convert; not Y)
 * diffsal_jpeg_decode: N files of one size H x W, component count ncomp and luma sampling hs x vs, all in device memory:
 *   bytes     the files packed back to back, padded with zeros to nbytes, a multiple of 4 below 2^31; 4-byte aligned
 *   files     N records of 1392 bytes: uint32 scan_off, scan_len (the entropy-coded bytes in `bytes`; informative), restart (MCUs
 *             per interval, 0: none), seg0, nseg (the file's rows of `segments`), 3 unused; uint8 comp[4][4]: per component its
 *             quantisation table, DC table, AC table, 0; uint8 qt[4][64]: quantisation tables 0..3 in natural order;
 *             uint8 hbits[4][16], hvals[4][256]: Huffman tables DC 0, DC 1, AC 0, AC 1 as DHT carries them (counts per length, symbols)
 *   segments  nseg rows of int32 (file, begin, end, first_mcu): one restart interval each, bytes [begin, end) of `bytes` without the
 *             RSTn marker; the whole scan when the file has no restart interval.  max_file_seg: the most rows any file has
 *   out       [N][H][W][3] bytes (mode_l = 0) or [N][H][W] (mode_l = 1), indexed in 64 bits
 *   status    int32 [N]: 0 clean, else the OR of DIFFSAL_JPEG_BAD_CODE (no Huffman code matches), DIFFSAL_JPEG_BAD_INDEX (a run past
 *             coefficient 63) and DIFFSAL_JPEG_NO_BITS (a segment ended before its MCUs).  The pixels of such a file are
 *             unspecified; they lie inside its frame, and the other files of the call are unaffected.  libjpeg's error recovery is
 *             not reproduced
 *   ws        >= diffsal_jpeg_decode_ws_bytes(N, H, W, ncomp, hs, vs) bytes, 16-byte aligned: int32 [N] status, int16
 *             [N][blocks][64] coefficients, uint8 component planes at component resolution (MCU padding included)
 * For any contents of bytes, files and segments no kernel reads outside them or writes outside out, status and ws: byte ranges
 * and MCU counts are clamped, selectors masked, every loop bound is a constant or comes from N, H, W, hs, vs.
 * Launches: a clear of status and coefficients (hipMemsetAsync on `stream`, every call); entropy (a lane per segment, the file's
 * Huffman tables built in LDS per workgroup; a file without restart markers is decoded by one lane); transform (a lane per
 * block); colour (up-sampling, RGB, L).  Bit-reproducible; a file's pixels do not depend on the batch it is in.  No allocation, no
 * synchronisation, no host copy, graph-safe; all argument checks precede the first launch.  ws_bytes: 0 for a bad argument. */
#define DIFFSAL_JPEG_BAD_CODE 1
#define DIFFSAL_JPEG_BAD_INDEX 2
#define DIFFSAL_JPEG_NO_BITS 4
size_t diffsal_jpeg_decode_ws_bytes(int N, int H, int W, int ncomp, int hs, int vs);
int diffsal_jpeg_decode(const unsigned char* bytes, long nbytes, const void* files, const int* segments, int nseg, int max_file_seg,
                        int N, int H, int W, int ncomp, int hs, int vs, int mode_l, unsigned char* out, int* status, void* ws,
                        size_t ws_bytes, diffsal_stream_t stream);

/* ---- PNG decode: the frame and map files of the visual sets -> the uint8 frames Pillow returns -----------
 * R/datasets/dhf1k_data.py:78, R/datasets/ucf_dataset.py:68 and R/datasets/holly2wood_dataset.py:72 read every frame '%d.png' with
 * Image.open(f).convert('RGB'); R/datasets/meta_data.py:49-57 reads the annotation maps '%04d.png' with .convert('L');
 * R/compute_metrics.py:9-14 reads the .png files of maps/ and fixation/ back.  Every step is integer arithmetic and the result here is
 * bit-equal to Pillow 12.2.  Taken: non-interlaced files of bit depth 8 with colour type 0, 2, 3, 4 or 6 (Pillow's L, RGB, P, LA,
 * RGBA) and of depth 1, 2 or 4 with colour type 0 or 3; everything else is refused by the caller's parser before a launch.
 *   (a) inflate   RFC 1950 / 1951: the IDAT payloads end to end are one zlib stream (32 K window, no dictionary); stored, fixed and
 *                 dynamic blocks; its output is H rows of 1 + row_bytes bytes, row_bytes = ceil(W * channels * depth / 8)
 *   (b) filter    PNG 9.2: the first byte of a row is its filter, 0 None, 1 Sub, 2 Up, 3 Average (floor((a + b) / 2)), 4 Paeth
 *                 (p = a + b - c; the nearest of a, b, c, ties in that order); a: the byte one pixel to the left (one byte below 8
 *                 bits), b: above, c: above left; bytes outside the image are 0; sums modulo 256
 *   (c) samples   8 bits: as they are.  1, 2, 4 bits: most significant first in a byte; grey values times 255, 85, 17; a palette
 *                 index selects its PLTE entry (a short PLTE is padded with zeros)
 *   (d) RGB       grey: R = G = B = value; alpha is dropped; tRNS is ignored for every type
 *   (e) L         grey: the value.  RGB, RGBA and palette entries: (19595 R + 38470 G + 7471 B + 0x8000) >> 16
 * diffsal_png_decode: N files of one size H x W, colour type and bit depth, all in device memory:
 *   bytes     the files' zlib streams, each starting at a multiple of 16, padded with zeros to nbytes, a multiple of 16 below
 *             2^31; 16-byte aligned
 *   files     N records of 784 bytes: uint32 off, len (the stream in `bytes`), 2 unused; uint8 pal[768]: PLTE, zero-padded
 *   out       [N][H][W][3] bytes (mode_l = 0) or [N][H][W] (mode_l = 1), indexed in 64 bits
 *   status    int32 [N]: 0 clean, else the OR of the DIFFSAL_PNG_* bits below.  DIFFSAL_PNG_LONG alone leaves the pixels intact;
 *             with any other bit the pixels of that file are unspecified (they lie inside its frame and are the same in every
 *             call), and the other files of the call are unaffected.  DIFFSAL_PNG_SHORT is stricter than Pillow, which returns
 *             such a file without a word
 *   ws        >= diffsal_png_decode_ws_bytes(N, H, W, color_type, bit_depth) bytes, 16-byte aligned: 16 bytes of state per file,
 *             then per file its filtered scanlines, H * (1 + row_bytes) bytes padded to 16.  Every byte read is written first
 * For any contents of bytes and files no kernel reads outside them or writes outside out, status and ws: stream reads are clamped
 * to [off, off + len) inside nbytes, region writes to the file's region, and every loop is bounded by N, H, W or by the stream's
 * bits (every symbol consumes at least one).  Chunk CRCs are not looked at (they never reach the device); Adler-32 is verified.
 * Launches: inflate, then unfilter + convert + Adler-32; a wave per file in both.  W <= 8192.  Bit-reproducible; a file's pixels
 * do not depend on the batch it is in.  No allocation, no synchronisation, no host copy, graph-safe; all argument checks precede
 * the first launch (DIFFSAL_E_ARG / DIFFSAL_E_SHAPE with a message).  ws_bytes: 0 for a bad argument. */
#define DIFFSAL_PNG_BAD_BLOCK 1
#define DIFFSAL_PNG_BAD_STORED 2
#define DIFFSAL_PNG_BAD_LENGTHS 4
#define DIFFSAL_PNG_BAD_SYMBOL 8
#define DIFFSAL_PNG_BAD_DISTANCE 16
#define DIFFSAL_PNG_NO_INPUT 32
#define DIFFSAL_PNG_SHORT 64
#define DIFFSAL_PNG_LONG 128
#define DIFFSAL_PNG_BAD_FILTER 256
#define DIFFSAL_PNG_BAD_ADLER 512
size_t diffsal_png_decode_ws_bytes(int N, int H, int W, int color_type, int bit_depth);
int diffsal_png_decode(const void* bytes, long nbytes, const void* files, int N, int H, int W, int color_type, int bit_depth,
                       int mode_l, void* out, void* status, void* ws, size_t ws_bytes, diffsal_stream_t stream);

/* ---- PNG export: the 8-bit maps of the visual sets -> complete .png files -----------
 * For DHF1K, UCF-Sports and Hollywood-2 R/diffusion_trainer.py:898-935 (save_img) writes '<video>/<frame>.png'.  u8 = the bytes of
 * diffsal_map_to_u8, [B][H][W], 1 <= B <= 65535, 1 <= H <= 65535, 1 <= W <= 8192 (what "PNG decode" takes); anything else is
 * DIFFSAL_E_SHAPE.  The files are not Pillow's bytes: they are valid PNGs that decode to exactly the input, and their bytes are a
 * function of the pixels alone (tests/_png_encode_ref.py restates them in NumPy), whatever the launch shape, the order of the
 * atomics, the batch or the buffers' earlier contents.  Integer work throughout.
 *   file       the 8-byte signature; IHDR (W, H big-endian, depth 8, colour type 0, compression 0, filter 0, interlace 0); one
 *              IDAT; IEND.  Chunk CRC-32s are correct.  The file has 57 + len(IDAT payload) bytes
 *   IDAT       78 01; one deflate stream; the Adler-32, big-endian, of the filtered scanlines
 *   scanlines  H rows of 1 + W bytes: the filter type, then the filtered bytes.  For every row all five filters (PNG 9.2) are
 *              computed from the raw pixels (a: left, b: above, c: above left, 0 outside the image); the one kept has the least sum
 *              of min(v, 256 - v) over its W bytes, a tie goes to the lowest type
 *   segments   the H * (W + 1) bytes in pieces of 16384 (the last may be shorter), each exactly one block with dynamic codes
 *              (BTYPE 2), BFINAL on the last only; blocks follow each other bit by bit; the last byte is padded with zero bits
 *   tokens     distance 1 only.  At position p of a segment, r = the count of consecutive positions q >= p inside the segment whose
 *              byte equals the stream byte in front of it (which may lie in the segment before, never in front of the stream).
 *              r >= 3: a match of length min(r, 258) at distance 1, advance by it; else the literal, advance by one.  A run thus
 *              falls into pieces of 258 from its start and a rest of 1 or 2 is literals.  The block ends with symbol 256
 *   lengths    of a code from symbol counts with limit L (15: literal/length, 286 symbols; 7: code lengths, 19 symbols): the
 *              symbols with a count take part (symbols 0 and 1 too if fewer than two have one), in ascending order of (count,
 *              symbol).  Huffman's tree by the two-queue method, a leaf before an internal node of equal weight, gives the
 *              number of codes per length.  If a length exceeds L: all above L are counted at L; then, until the Kraft sum in
 *              units of 2^-L is 2^L: one code less at L, and at the largest length i < L that has a code one code less and two
 *              more at i + 1 (each round lowers the sum by exactly one unit).  The lengths are handed out along the order, the
 *              longest to the rarest.  The code is complete: Kraft sum exactly 1.  Codes are canonical (RFC 1951 3.2.2)
 *   distance   one code: symbol 0 with length 1 (HDIST = 0), sent in every block; a match spends one 0 bit on it
 *   header     HLIT = up to the last literal/length symbol with a length (at least 257).  The HLIT lengths and the distance length
 *              are one sequence, run-length coded: a run of zeros in pieces of 138 (symbol 18) while 11 or more are left, then
 *              17 for 3..10, else zeros one by one; another value once, then 16 in pieces of 6 while 3 or more are left, then the
 *              value itself.  HCLEN trimmed to the last code-length symbol with a length in the order 16 17 18 0 8 7 9 ...
 * diffsal_png_encode: data [B][cap] bytes, 16-byte aligned, cap a multiple of 16 and >= diffsal_png_encode_capacity(H, W); image b's
 * file is data[b][0 .. lengths[b]), lengths int32 [B]; the bytes behind a file are zero.
 * Capacity is a bound, not an estimate.  Every token spends at most 15 bits per stream byte it covers (a literal 15; a match at most
 * 15 + 5 + 1 for three bytes or more).  A block adds its header, at most 3 + 14 + 3 * 19 + 287 * (7 + 7) = 4092 bits (287 lengths,
 * each at most one code-length symbol of 7 bits and 7 extra bits), and an end symbol of at most 15 bits.  With S = H * (W + 1) and
 * n = ceil(S / 16384):  m = ceil((15 S + 4107 n) / 8) bytes of deflate stream, and
 *   diffsal_png_encode_capacity(H, W) = (63 + m) rounded up to 16      (63 = 57 + zlib's header and Adler-32; below 2^31)
 * so that every image's row of data starts on a 16-byte boundary.  ws >= diffsal_png_encode_ws_bytes(B, H, W) bytes, 16-byte
 * aligned, every array sized from the same geometry: the scanlines (S padded to 64) and a 16-bit token record per stream byte,
 * per segment 256 bit offsets, 288 codes, 128 header words, 16 bytes of sums and a 64-bit bit offset, per image a 64-bit bit
 * count.  Every byte read is written first.  No kernel writes outside data[b][0 .. cap), lengths or ws for any pixels, and every
 * loop is bounded by the geometry or a segment's size.
 * Launches: a clear of data (hipMemsetAsync on `stream`, every call); filter (a wave per row); segment (a workgroup per segment:
 * tokens, histogram, codes, header, bit counts, Adler-32 sums); frame (a workgroup per image: scan of the bit counts, everything
 * but the stream and IDAT's CRC); pack (integer atomicOr into the shared words: order-independent); crc (partial CRCs of 64
 * bytes combined by multiplication by x^(8 n) mod P).  No allocation, no synchronisation, no host copy, graph-safe; all argument
 * checks precede the first launch (DIFFSAL_E_ARG / DIFFSAL_E_SHAPE with a message).  capacity, ws_bytes: 0 for a bad argument. */
long diffsal_png_encode_capacity(int H, int W);
size_t diffsal_png_encode_ws_bytes(int B, int H, int W);
int diffsal_png_encode(const void* u8, int B, int H, int W, void* data, long cap, void* lengths, void* ws, size_t ws_bytes,
                       diffsal_stream_t stream);

/* ---- audio front end: PCM samples in device memory -> the audio tensor [B][1][9][h][w] forward_vggish reads -----------
 * What the reference does per clip on the host in numpy: R/datasets/saliency_db.py:449-497 (get_mel_feature) cuts
 * wav[starts[a] : ends[b] + 1] out of the video's waveform (the table of R/datasets/saliency_db.py:208-222), centres it in a
 * zero buffer of `window` samples and calls R/datasets/torchvggish/vggish_input.py:30-82 (waveform_to_examples), which frames
 * the log-mel spectrogram of R/datasets/torchvggish/mel_features.py:71-223 into examples; get_mel_feature repeats them to nine
 * and R/datasets/saliency_db.py:303-305,351-354 resizes each to half the frame size and stacks them.
 * diffsal_logmel takes input at 16000 Hz only and any other sample_rate is DIFFSAL_E_ARG there.  The reference reads a file at its
 * native rate, tabulates starts / ends at that rate and, per clip, resamples the padded buffer to 16000 Hz with resampy
 * (R/datasets/torchvggish/vggish_input.py:52-53): that step is diffsal_resample_excerpts, an opt-in launch in front of
 * diffsal_logmel, whose output [B][n_samples] fp64 is diffsal_logmel's wav with V = B, video[b] = b and window = n_samples.
 *
 * diffsal_logmel: wav [V][Lmax] of wav_dtype (int16 is divided by 32768, exactly; fp32; fp64), wav_len [V] valid samples per
 * video (NULL: Lmax), video [B] the video of each clip (NULL: 0), starts / ends [B] -> out [B][n_frames][64], fp32 (out_f64 = 0)
 * or fp64 (out_f64 = 1: the value before the rounding, for tests).  All arithmetic is fp64.  Per clip, with n = wav_len[video]:
 *   lo = min(starts, n), hi = min(ends + 1, n), v = max(hi - lo, 0)              numpy's slice clamping
 *   x[p] = wav[lo + p - off] for off <= p < off + v, else 0;  off = window/2 - v/2 (integer divisions; both parities of v)
 *   frame f, bin k:  X = sum_{i < 400} x[160 f + i] * hann[i] * exp(-2 pi j i k / 512),  hann[i] = 0.5 - 0.5 cos(2 pi i / 400)
 *   mel[f][m] = sum_k |X[f][k]| * M[k][m]        M: the 257 x 64 HTK mel matrix, 16 kHz, 125-7500 Hz (only bins 5..239 carry
 *                                                weight, a band at most 17 of them), summed in ascending k
 *   out[f][m] = log(mel[f][m] + 0.01)            frames 0 .. n_frames - 1 <= (window - 400) / 160
 * The transform is a direct DFT in ascending i (no FFT); the caller checks v <= window (the reference fails there); an
 * unchecked longer excerpt is centre-cropped, never read out of bounds.  `tables`: diffsal_logmel_table_doubles() fp64 values
 * on the device, 16-byte aligned, built once by the caller:
 *   [400][256][2]  hann[i] * (cos, sin)(2 pi i k / 512) for k = 5 + column, columns 235..255 zero
 *   [64][17]       M[first[m] + 5 + j][m], j = 0..16 (zero past the band's last bin)
 *   [64]           first[m]: the column of band m's first non-zero bin
 *
 * diffsal_audio_examples: logmel [B][n_frames][64] fp32, exists [B] bytes (NULL: all present) -> out [B][1][9][h][w] fp32.
 *   n_examples = 1 + ((window - 400) / 160 + 1 - 64) / 11 of the window the log-mel came from; < 1 is DIFFSAL_E_SHAPE
 *   output example j reads source example e = j if n_examples >= 9; otherwise, with r = 9 / n_examples,
 *   e = j / r for j < n_examples * r, else (j - n_examples * r) / r      (repeat_interleave, then cat with the head of the
 *                                                                         repeated list, then [:9])
 *   example e is log-mel frames 11 e .. 11 e + 63 (rows) x 64 bands (columns); n_frames >= 64 + 11 (min(n_examples, 9) - 1)
 *   resize 64 x 64 -> h x w as F.interpolate(mode="bilinear", align_corners=False) on the CPU computes it in fp32, per axis
 *     s = max(fma(fl32(64 / N), o + 0.5, -0.5), 0);  i0 = min(trunc(s), 63);  i1 = min(i0 + 1, 63);  w1 = s - i0;  w0 = 1 - w1
 *     value = fma(w0, a, fl32(w1 * b)), columns first, then rows           (h = w = 64 returns the examples unchanged)
 *     the plain form, with no anti-aliasing filter, for every h and w: for an upscale that is also what the antialiased form
 *     computes; for h or w below 64 a torchvision whose tensor Resize defaults to antialias=True gives other values
 *   a clip with exists[b] == 0 is zeros (the reference returns zeros, not log(0.01), for a video without audio)
 *
 * diffsal_resample_excerpts: wav, wav_dtype, V, Lmax, wav_len, video, starts, ends, B as for diffsal_logmel, at sr_orig Hz ->
 * out [B][n_samples] fp64: the first n_samples <= int(window * sr_new / sr_orig) (= diffsal_resample_length) samples of what
 * resampy 0.4.2 (resampy.core.resample, resampy.interp._resample_loop) returns for the clip's padded buffer x[0 .. window - 1]
 * (lo, v, off as above; x is never written to memory; the accumulation is fp64 for every wav_dtype, as the reference's buffer is):
 *   ratio = fp64(sr_new) / sr_orig;  scale = min(1, ratio);  inc = 1 / ratio;  step = int(scale * num_table)   (truncated: 371 at
 *                                                                              22050 -> 16000; the library's behaviour, kept)
 *   output t:  time = t * inc;  m = int(time);  frac = scale * (time - m)
 *              f = frac * num_table;  o = int(f);  eta = f - o
 *              for i = 0 .. min(m + 1, (nwin - o) / step) - 1:           y += (win[o + i step] + eta * delta[o + i step]) * x[m - i]
 *              frac = scale - frac;  f = frac * num_table;  o = int(f);  eta = f - o
 *              for k = 0 .. min(window - m - 1, (nwin - o) / step) - 1:  y += (win[o + k step] + eta * delta[o + k step]) * x[m + k + 1]
 * Every operation is one fp64 operation rounded to nearest, product then sum, nothing fused (the library is numba without
 * fast-math), in exactly this order: the left wing in ascending i, then the right wing in ascending k.  The result is therefore a
 * function of the inputs alone and equals a NumPy restatement of these lines bit for bit.  A tile of outputs that reads nothing
 * but padding is written as zeros without the sums (w * 0 is a signed zero and y + a signed zero is y: the bits are the same).
 * `table`: [nwin][2] fp64 on the device, 16-byte aligned, built by the caller in fp64: (win[j], delta[j]) with win the filter's
 * half window, num_table entries per zero crossing, multiplied by ratio if ratio < 1, and delta[j] = win[j + 1] - win[j],
 * delta[nwin - 1] = 0.  The kernel does not depend on the filter's design.  resampy's kaiser_best is
 *   win[j] = r sinc(r j / 512) kaiser(2 * 32768 + 1, beta)[32768 + j],  j = 0 .. 32768  (nwin 32769, num_table 512),
 *   r = 0.9475937167399596, beta = 14.769656459379492;  kaiser_fast: 16 zero crossings (nwin 8193), r = 0.85, beta = 8.555504641634386
 * DIFFSAL_E_ARG: a rate below 1, sr_orig == sr_new (the reference does not resample there), a bad wav_dtype, a null or
 * misaligned pointer.  DIFFSAL_E_SHAPE: n_samples outside 1 .. int(window * sr_new / sr_orig), nwin < 2, step < 1 or > nwin, a
 * tile of 256 outputs that reads more than 8192 inputs (255 * inc + 2 + 2 (nwin / step)).
 * diffsal_resample_length: int(n * sr_new / sr_orig), the product in integers, one fp64 division, truncated; -1 for a bad argument.
 *
 * All calls: every sum has a fixed order, results are bit-reproducible and a clip's result does not depend on the batch it is
 * in.  No atomics, no allocation, no synchronisation, graph-safe.  All argument checks precede the launch. */
#define DIFFSAL_WAV_I16 0
#define DIFFSAL_WAV_F32 1
#define DIFFSAL_WAV_F64 2
long diffsal_logmel_table_doubles(void);
int diffsal_logmel(const void* wav, int wav_dtype, int V, long Lmax, const long* wav_len, const int* video, const int* starts,
                   const int* ends, int B, int sample_rate, int window, int n_frames, const double* tables, int out_f64, void* out,
                   diffsal_stream_t stream);
int diffsal_audio_examples(const float* logmel, const unsigned char* exists, int B, int n_frames, int n_examples, int h, int w,
                           float* out, diffsal_stream_t stream);
long diffsal_resample_length(long n, int sr_orig, int sr_new);
int diffsal_resample_excerpts(const void* wav, int wav_dtype, int V, long Lmax, const long* wav_len, const int* video, const int* starts,
                              const int* ends, int B, int window, int sr_orig, int sr_new, const double* table, int nwin, int num_table,
                              int n_samples, double* out, diffsal_stream_t stream);

/* ---- video front end: decoded uint8 frames in device memory -> the clip tensor [B][3][T][h][w] MViT reads -----------
 * What the reference does per clip on the host with Pillow: R/datasets/saliency_db.py:29-36 (pil_loader) resizes every frame to
 * 320 x 240 with Image.resize's default filter (bicubic); :292-296 applies Scale(sample_size) (bilinear), ToTensor(norm_value)
 * and Normalize(mean, std); :382-394 stacks and permutes the frames.  R/datasets/meta_data.py:27-35 and
 * R/datasets/dhf1k_data.py:72-81 run transforms.Resize on the PIL image (bilinear), ToTensor and Normalize.  The targets
 * (saliency_db.py:298-301 target_transform, meta_data.py:32-35 sal_transform) are the same resize of an 'L' image and / 255.
 * JPEG decoding with convert('RGB' | 'L') is diffsal_jpeg_decode ("JPEG decode"), PNG decoding is diffsal_png_decode ("PNG decode").
 *
 * diffsal_resample_u8: in [N][H0][W0][C] bytes, C = 1 or 3 -> out [N][H1][W1][C] bytes: one Image.resize of Pillow's 8-bit path
 * (ImagingResample), bit for bit.  The coefficients are the caller's, built in float64 as precompute_coeffs builds them, per
 * axis (n_in -> n_out, filter support s0 = 1 bilinear, 2 bicubic with a = -0.5):
 *   scale = n_in / n_out;  fs = max(scale, 1);  s = s0 * fs;  ksize = 2 * ceil(s) + 1  (= diffsal_resample_ksize)
 *   output o:  c = (o + 0.5) * scale;  xmin = max(trunc(c - s + 0.5), 0);  count = min(trunc(c + s + 0.5), n_in) - xmin
 *              w[t] = filter((t + xmin - c + 0.5) / fs) for t < count, divided by their sum (if it is not zero)
 *   kk[o][t] = trunc(w[t] * 2^22 + 0.5)  (- 0.5 for a negative w[t]);  0 for count <= t < ksize
 *   bounds [n_out][2] = (xmin, count),  kk [n_out][ksize], both int32, in device memory
 * The kernels do integer work only.  Horizontal pass first, every channel alike:
 *   mid[y][o] = clip8((2^21 + sum_{t < count} in[y][xmin + t] * kk[o][t]) >> 22)      int32 sum, arithmetic shift, clip to 0..255
 * then the vertical pass the same way on the uint8 image `mid`.  An axis whose size does not change runs no pass (its tables may
 * be NULL); equal sizes make the call a copy.  All N frames share the source size (diffsal_resample_u8_groups: several sizes).
 * form: DIFFSAL_RESAMPLE_FUSED is one launch: a workgroup owns band_rows output rows over the full width, resamples the source
 * rows they need horizontally into LDS and runs the vertical pass out of LDS (band_rows = 0: the library picks it from the LDS
 * budget, diffsal_resample_u8_band_rows; at most 32; DIFFSAL_E_SHAPE if the band does not fit in 160 KB).
 * DIFFSAL_RESAMPLE_TWO_PASS keeps `mid` [N][H0][W1][C] in ws (diffsal_resample_u8_ws_bytes).  DIFFSAL_RESAMPLE_AUTO is the fused
 * form where a band fits and H0 * W0 >= 2 * H1 * W1 (where it measured faster), else two passes.  The forms agree bit for bit;
 * with a single pass they are the same launch.
 * The tables cannot be checked from the host: the kernels clamp xmin to the source, count to ksize and to the source, and a
 * band's row span to its LDS image, so a wrong table gives wrong pixels, never an access outside the buffers.
 *
 * diffsal_clip_gather_u8: frames [N][h][w][C] bytes, indices [B][T] int32 (NULL: frame b * T + t, B * T = N), table [C][256]
 * fp32 -> out [B][C][T][h][w] fp32 with out[b][c][t][y][x] = table[c][frames[indices[b][t]][y][x][c]].  The table is how
 * ToTensor and Normalize are matched bit for bit: the caller evaluates the reference's own float32 operations on the 256 byte
 * values per channel (x / norm_value, then - mean, then / std) and the kernel only indexes.  C = 1, T = 1, indices NULL and
 * table[v] = v / 255 is the target path.  An index outside [0, N) is clamped (check it on the host where it is known there).
 *
 * diffsal_resample_u8_groups: frames of G source sizes to one output size in one call.  `groups` is a HOST array of G blocks;
 * group g holds N frames [N][H0][W0][C] at its own device pointer `in` with its own tables (as for diffsal_resample_u8; NULL for
 * an axis that does not change).  C, (H1, W1) and the filter are shared.  out is [n_total][H1][W1][C] with n_total the sum of the
 * groups' N.  dst (device memory, int32 [n_total], or NULL) names the output frame of every input frame, the groups' frames
 * counted in group order; NULL: that order itself.  Group g's frames are, byte for byte, what diffsal_resample_u8 gives for that
 * group alone with band_rows = 0 and the same `form`; each group takes the form that call would take, so DIFFSAL_RESAMPLE_AUTO
 * may run some groups fused and others in two passes.
 * Launches: the group blocks travel by value in the launch arguments, DIFFSAL_RESAMPLE_MAX_GROUPS of them at most.  Every run of
 * that many groups takes at most one launch of each of three kernels, however many groups it holds: the fused bands of its fused
 * groups; the horizontal pass (two-pass groups into the workspace, groups whose height does not change into `out`, and groups
 * whose size does not change at all, which are copied there); the vertical pass (two-pass groups out of the workspace, groups
 * whose width does not change).  A workgroup finds its (group, frame, band or tile) through a prefix table of the groups'
 * workgroup counts; the fused launch holds the largest LDS of its groups' plans.  diffsal_resample_u8_groups_launches is that
 * count (-1: bad argument).  ws holds the two-pass groups' intermediate images, each rounded up to 16 bytes
 * (diffsal_resample_u8_groups_ws_bytes).
 * The clamping contract holds: dst cannot be checked by the host, so an entry is clamped to [0, n_total); an entry named twice
 * leaves one of the two frames there.  A wrong table or dst gives wrong pixels, never an access outside the buffers.
 *
 * All calls: no atomics, no allocation, no synchronisation, bit-reproducible, graph-safe; all argument checks precede the
 * launch. */
#define DIFFSAL_FILTER_BILINEAR 0
#define DIFFSAL_FILTER_BICUBIC 1
#define DIFFSAL_RESAMPLE_AUTO 0
#define DIFFSAL_RESAMPLE_FUSED 1
#define DIFFSAL_RESAMPLE_TWO_PASS 2
int diffsal_resample_ksize(int in_size, int out_size, int filter);      /* 0: bad argument */
int diffsal_resample_u8_band_rows(int H0, int W0, int C, int H1, int W1, int filter);      /* 0: no band fits, or a single pass */
size_t diffsal_resample_u8_ws_bytes(int N, int H0, int W0, int C, int H1, int W1, int filter, int form);
int diffsal_resample_u8(const unsigned char* in, int N, int H0, int W0, int C, int H1, int W1, int filter, const int* xbounds,
                        const int* xkk, int xks, const int* ybounds, const int* ykk, int yks, int form, int band_rows,
                        unsigned char* out, void* ws, size_t ws_bytes, diffsal_stream_t stream);
int diffsal_clip_gather_u8(const unsigned char* frames, int N, int h, int w, int C, const int* indices, int B, int T,
                           const float* table, float* out, diffsal_stream_t stream);
#define DIFFSAL_RESAMPLE_MAX_GROUPS 16      /* groups per launch; a call with more is split into runs of this many */
typedef struct diffsal_resample_group {
  const unsigned char* in;      /* [N][H0][W0][C], device memory */
  int N, H0, W0;
  const int* xbounds;           /* [W1][2], [W1][xks]; NULL where W0 == W1 */
  const int* xkk;
  int xks;
  const int* ybounds;           /* [H1][2], [H1][yks]; NULL where H0 == H1 */
  const int* ykk;
  int yks;
} diffsal_resample_group;
size_t diffsal_resample_u8_groups_ws_bytes(const diffsal_resample_group* groups, int G, int C, int H1, int W1, int filter, int form);
int diffsal_resample_u8_groups_launches(const diffsal_resample_group* groups, int G, int C, int H1, int W1, int filter, int form);
int diffsal_resample_u8_groups(const diffsal_resample_group* groups, int G, int C, int H1, int W1, int filter, int form,
                               const int* dst, int n_total, unsigned char* out, void* ws, size_t ws_bytes, diffsal_stream_t stream);

/* ---- K15: sampler elementwise update out = a*x + b*y + c*z  (y, z may be NULL) -----------
 * scalar-coefficient axpys of R/diffusion_trainer.py:459-478 and R/models/dpm_solver/sampler.py:548-593,816-853. */
int diffsal_axpbypcz(const float* x, const float* y, const float* z, float a, float b, float c, float* out,
                     size_t n, diffsal_stream_t stream);

/* ---- K14 tail + K15 fused: the end of a denoising step in one pass over the sampler state.
 *   x0 = bilinear(s_low [N,h,w] -> [N,H,W])          final resize of the sigmoid map, R/.../sal_unet.py:325-327
 *   m  = ex * x + e0 * x0                            wrapper's model-output conversion (x_start -> noise:
 *                                                    ex = 1/sigma_t, e0 = -alpha_t/sigma_t, R/models/dpm_solver/sampler.py:286-292;
 *                                                    ex = 0, e0 = 1 keeps x0)
 *   x_next = A * x + c0 * m + c1 * m_prev            multistep update, sampler.py:548-593, 797-853 (m_prev NULL: order 1)
 * x0_out and x_next may be NULL.  Same per-element arithmetic as diffsal_resize_bilinear + diffsal_axpbypcz (bit-equal). */
int diffsal_resize_update(const float* s_low, const float* x, const float* m_prev, float* x0_out, float* m_out, float* x_next,
                          int N, int h, int w, int H, int W, float ex, float e0, float A, float c0, float c1,
                          diffsal_stream_t stream);

/* ---- sampler noise from a counter-based generator (Philox4x32-10; beyond the reference, which draws x_T and the per-step
 * noise of its stochastic samplers from torch's stateful generator: R/diffusion_trainer.py:476 randn_like in sample_ddim,
 * :521 in p_sample, :119 x_T in prepare_data).  The value for (seed, clip id, draw, element) is a pure function, so a clip's noise
 * does not depend on the batch it sits in, its position there or the number of devices of a sweep:
 *   key     = (seed & 0xffffffff, seed >> 32)
 *   counter = (q, draw, id & 0xffffffff, id >> 32)      q = e / 4, e = element index inside the clip's `per` elements;
 *                                                       draw = 0 for x_T, s + 1 for the noise of step s
 *   multipliers 0xD2511F53 / 0xCD9E8D57, Weyl constants 0x9E3779B9 / 0xBB67AE85, ten rounds -> r0..r3 = elements 4q..4q+3
 *   normals: u1 = ((r0 >> 8) + 1) * 2^-24, u2 = (r1 >> 8) * 2^-24, z0 = sqrt(-2 ln u1) cos(2 pi u2), z1 = sqrt(-2 ln u1) sin(2 pi u2);
 *            z2, z3 from (r2, r3) in the same way; |z| <= 5.77
 * `seed` points to ONE 64-bit word and `ids` to N 64-bit clip ids IN DEVICE MEMORY: a captured graph is replayed for other
 * clips or another seed by rewriting those two buffers.  An id is used as its 64-bit pattern; callers keep ids non-negative
 * (the library cannot read them before the launch; the Python binding checks host-side ids).  1 <= per <= 2^34.
 *   philox_bits    out[N][per] raw 32-bit words (a test aid)
 *   philox_normal  out[N][per] = scale * z */
int diffsal_philox_bits(unsigned int* out, int N, long per, const long long* ids, const unsigned long long* seed,
                        unsigned int draw, diffsal_stream_t stream);
int diffsal_philox_normal(float* out, int N, long per, const long long* ids, const unsigned long long* seed,
                          unsigned int draw, float scale, diffsal_stream_t stream);
/* resize_update with a direct x0 term and in-kernel noise: the whole tail of a DDIM (eta >= 0) or DDPM ancestral step
 * (R/diffusion_trainer.py:459-478, :508-527) in the denoiser's last kernel.
 *   x0 = bilinear(s_low);  m = ex * x + e0 * x0;  x_next = b0 * x0 + A * x + cz * z + c0 * m + c1 * m_prev
 * summed in that order, a term whose coefficient is 0 left out, the first product rounded and every further term one fma;
 * z = the normals of (seed, ids[n], draw) for per = H * W, generated in place when cz != 0 (ids / seed may be NULL otherwise).
 * With b0 = cz = 0 this is diffsal_resize_update's A * x + c0 * m [+ c1 * m_prev], bit for bit; with cz != 0 it equals
 * diffsal_resize_update(x_next = NULL), diffsal_philox_normal(scale = 1) and diffsal_axpbypcz calls in the order above.
 *   DDIM: ex = r/rm1, e0 = -1/rm1, A = 0, b0 = sqrt(abar_next), cz = c1(eta), c0 = c2;  DDPM: ex = 0, e0 = 1, A = coef2,
 *   b0 = coef1, cz = exp(0.5 logvar) (0 at t = 0), c0 = 0. */
int diffsal_resize_update_noise(const float* s_low, const float* x, const float* m_prev, float* x0_out, float* m_out,
                                float* x_next, int N, int h, int w, int H, int W, float ex, float e0, float A, float b0,
                                float c0, float c1, float cz, const long long* ids, const unsigned long long* seed,
                                unsigned int draw, diffsal_stream_t stream);

/* ---- training noise: the training step's inputs from the same generator (K16; beyond the reference, which draws the two
 * noises from torch's stateful generator, t0 from numpy's global one and the dropout masks from torch's:
 * R/diffusion_trainer.py:106-117, 122-137, R/datasets/__init__.py:8-25, R/models/saliency_decoder/sal_unet.py:109,133).
 * Philox4x32-10, key, counter and Box-Muller exactly as in "sampler noise" above; only the meaning of the words is new:
 *   id    = a caller-supplied non-negative 64-bit SAMPLE id (e.g. the dataset index of the clip), not the position in the batch
 *   draw  = 0x80000000 | (step << 4) | purpose     step = optimizer steps completed before this one, < 2^27; bit 31 keeps
 *                                                  the stream apart from the sampler's draws 0, 1, 2, ... under one seed
 *   purpose 0 dequantisation noise, 1 forward-process noise, 2 timestep, 3 + i dropout site i (i < 13)
 *   timestep t = (uint64(r0) * T) >> 32, r0 = word 0 of the call (q = 0, purpose 2); T <= 2^31
 * `key` points to TWO consecutive 64-bit words IN DEVICE MEMORY, {seed, step}: the kernels form `draw` from the device step,
 * so a step takes no value from the host.  What a sample sees is a pure function of (seed, step, id): independent of the
 * batch it sits in, its position there and the rank count, and a run resumed from (seed, step) continues the stream.
 *
 * train_prepare: the whole of prepare_data in one launch.  sal [B][per], ids [B]; the two tables hold T floats each.
 *     x0 = sal + dq_scale * z0   (dq_scale = 0: x0 = sal, no draw)      z0 = normals of purpose 0
 *     x_t = a[t] * x0 + b[t] * z1                                        z1 = normals of purpose 1 (also written to `noise`,
 *                                                                        which may be NULL), a / b = the two tables
 *   t_mode 0: every sample draws its own t from its id; 1: every sample uses the draw of ids[0] (the reference's one t0 per
 *   rank batch -- by nature a function of the batch layout); 2: t = t_fixed for all.  t [B] int64 is written once per sample.
 *   Rounded as diffsal_axpbypcz rounds (first product, then one fma): bit-equal to diffsal_philox_normal(scale = 1) for the
 *   two draws followed by diffsal_axpbypcz(sal, 1, z0, dq_scale) and diffsal_axpbypcz(x0, a[t], z1, b[t]).  1 <= per <= 2^34;
 *   16-byte accesses when per % 4 == 0 and the pointers are aligned, element-wise otherwise.
 * dropout_keyed: out = x * keep / (1 - p) on x [B][per], per % 4 == 0 (DIFFSAL_E_SHAPE otherwise), 16-byte aligned.
 *   Element e of sample n is kept iff word e % 4 of the call (q = e / 4, purpose 3 + site, ids[n]) >= (unsigned)(p * 2^32),
 *   diffsal_dropout's threshold rule.  The same call on dy is the backward.
 * train_key_advance: key[1] += 1, one thread, in stream order: enqueue it after the last reader of the old step (the
 *   backward re-applies the dropout masks). */
int diffsal_train_prepare(const float* sal, const long long* ids, const unsigned long long* key, const float* sqrt_alphas_hat,
                          const float* sqrt_one_minus_alphas_hat, long T, float dq_scale, int t_mode, long t_fixed, float* x0,
                          float* x_t, long long* t, float* noise, int B, long per, diffsal_stream_t stream);
int diffsal_dropout_keyed(const float* x, float* out, int B, long per, float p, const long long* ids,
                          const unsigned long long* key, int site, diffsal_stream_t stream);
int diffsal_train_key_advance(unsigned long long* key, diffsal_stream_t stream);

/* ---- K16 tail: loss, gradient clipping and the optimizer, on flat fp32 buffers -------------
 * diffsal_reduce_blocks(): number of doubles the `part` scratch of the two reductions below must hold.
 *
 * mse_loss: loss[0] = loss_scale * sum (pred - target)^2 and, if dpred != NULL, dpred = 2 loss_scale (pred - target).
 *   With loss_scale = mse_weight / batch this is `mse_weight * (pred-gt).square().sum(dim=(1,2,3)).mean(dim=0)`
 *   (R/models/sal_losses.py:189-192) and its gradient.  Any n > 0 (a tail of 1 to 3 elements is read and written one by one);
 *   pred, target and dpred 16-byte aligned.
 * grad_norm: norm[0] = gscale * ||g||_2 over the flat gradient buffer -- total_norm of
 *   torch.nn.utils.clip_grad_norm_ (R/diffusion_trainer.py:228-233); gscale = 1/world_size folds in the DDP mean.
 * adam_step: torch.optim.Adam.step (R/util/utils.py:116-123, R/diffusion_trainer.py:235; amsgrad=false) on
 *   p, m (exp_avg), v (exp_avg_sq), with the gradient first multiplied by
 *   gscale * min(1, max_norm / (norm[0] + 1e-6)) (norm may be NULL or max_norm <= 0: no clipping).  `step` counts
 *   from 1.  store_clipped_grad != 0 writes the scaled gradient back into g as clip_grad_norm_ does.
 * adam_args (host code, no launch): fills the block of adam_args_size() bytes at `out` (HOST memory) with the numbers
 *   adam_step hands its kernel -- 1 - beta in fp32 rounded from double, the bias corrections 1 - pow(beta, step) formed
 *   in double as torch.optim.Adam forms them for a python-scalar step (R/util/utils.py:116-123), lr / bc1 and sqrt(bc2)
 *   rounded to fp32, gscale and max_norm.  adam_step itself calls it: one place forms these numbers.
 * adam_step_args: the update of adam_step with that block read from DEVICE memory (`args_dev`, 16-byte aligned; a copy
 *   of an adam_args block made in stream order before the launch) -- nothing of the step number, the learning rate or
 *   the clip bound is a launch argument, so a captured graph replays it for any step (R/diffusion_trainer.py:228-235
 *   once per replay).  Same grid, vector width, tail and arithmetic as adam_step: bit-identical results.
 * adam_ema_step / adam_ema_args / adam_ema_step_args: the three above with a shadow buffer `s` (an exponential moving average
 *   of p, R/models/diffusion_decoder/ema.py:4-48) updated in the same pass, from the NEW p:
 *   s = fmaf(mu, s, omm * p) with omm = (float)(1 - ema_mu) and mu = (float)ema_mu formed on the host -- the rounding
 *   sequence of axpbypcz(p, 1 - ema_mu, s, ema_mu), so the shadow is bit-equal to adam_step followed by that call, and p, g,
 *   m, v are bit-equal to adam_step's.  0 <= ema_mu <= 1.  The block of adam_ema_args_size() bytes is adam_args' block
 *   followed by the two floats omm, mu; adam_args_size() and its block are unchanged.
 * ema_swap: exchanges p and s in place, bit for bit (NaN payloads and -0 survive), one launch, no third buffer; the
 *   buffers must not overlap.  Its own inverse.
 * scale_by: out = x * s[0] with s a device scalar (the incoming d(loss) of the MSE backward); any n > 0.
 * multi_copy: dst[dst_offsets[i] .. +sizes[i]) = srcs[i][0 .. sizes[i]) for i < count, a few launches for any count
 *   (gathers the per-parameter gradients autograd produced into the flat gradient buffer; the three tables are HOST
 *   arrays, the pointers in them device pointers; dst_offsets multiples of 4 elements).
 * Reductions are fp64 with a fixed order: a step is bit-reproducible.  No host synchronisation. */
int diffsal_reduce_blocks(void);
int diffsal_multi_copy(const float* const* srcs, const long* dst_offsets, const long* sizes, int count, float* dst,
                       diffsal_stream_t stream);
int diffsal_scale_by(const float* x, const float* s, float* out, long n, diffsal_stream_t stream);
int diffsal_mse_loss(const float* pred, const float* target, float* dpred, float* loss, double* part, long n,
                     float loss_scale, diffsal_stream_t stream);
int diffsal_grad_norm(const float* g, long n, float gscale, float* norm, double* part, diffsal_stream_t stream);
int diffsal_adam_step(float* p, float* g, float* m, float* v, long n, double lr, double beta1, double beta2,
                      double eps, double weight_decay, int step, float gscale, const float* norm, float max_norm,
                      int store_clipped_grad, diffsal_stream_t stream);
size_t diffsal_adam_args_size(void);
int diffsal_adam_args(double lr, double beta1, double beta2, double eps, double weight_decay, int step, float gscale,
                      float max_norm, void* out /*host*/);
int diffsal_adam_step_args(float* p, float* g, float* m, float* v, long n, const void* args_dev, const float* norm,
                           int store_clipped_grad, diffsal_stream_t stream);
int diffsal_adam_ema_step(float* p, float* g, float* m, float* v, float* s, long n, double lr, double beta1, double beta2,
                          double eps, double weight_decay, int step, float gscale, const float* norm, float max_norm,
                          int store_clipped_grad, double ema_mu, diffsal_stream_t stream);
size_t diffsal_adam_ema_args_size(void);
int diffsal_adam_ema_args(double lr, double beta1, double beta2, double eps, double weight_decay, int step, float gscale,
                          float max_norm, double ema_mu, void* out /*host*/);
int diffsal_adam_ema_step_args(float* p, float* g, float* m, float* v, float* s, long n, const void* args_dev,
                               const float* norm, int store_clipped_grad, diffsal_stream_t stream);
int diffsal_ema_swap(float* p, float* s, long n, diffsal_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* DIFFSAL_H */
