// The GEMM / convolution family behind diffsal_conv_igemm, _group, diffsal_linear_pair and diffsal_linear_f32out: the host-side operand
// bundle, the descriptor's derived quantities, and the declaration -- once -- of every function one .hip file defines and another calls.
// Every candidate kernel exports the same three functions, which igemm.hip puts into its ordered lists:
//   *_takes(d, o, f)     does this kernel run d?  o == nullptr: the shape alone, "under some pointer alignment" (the workspace query)
//   *_ws_bytes(d, f)     the workspace it could use for d (kernels that use none have no such function)
//   *_launch(d, o, f, s) launch, after *_takes said yes for the same arguments: DIFFSAL_OK or an error code
// f is what the route switches say (igemm.hip, offer()): no candidate reads a switch that is about another kernel.
#pragma once
#include "common.h"

namespace diffsal {

struct GemmOperands {
  const void *in, *w;
  const float *bias, *scale, *shift, *rowvec;
  int rowvec_ld;                 // resolved: rowvec_ld(d)
  const void* residual;
  void *out, *ws;
  size_t ws_bytes;
  bool out_f32;                  // 16-bit storage in, fp32 out (diffsal_linear_f32out)
  const void *in2, *w2;          // second problem of a pair launch (diffsal_linear_pair: same descriptor), in2 == nullptr otherwise
  const float* bias2; void* out2;
};

// 1x1 / stride 1 / no padding: a plain [M, Cin] x [Cin, Cout] product
inline bool is_linear(const diffsal_conv_desc* d) {
  return d->KH == 1 && d->KW == 1 && d->stride_h == 1 && d->stride_w == 1 && d->pad_t == 0 && d->pad_l == 0 && d->Ho == d->H &&
         d->Wo == d->W;
}
inline long gemm_M(const diffsal_conv_desc* d) { return static_cast<long>(d->N) * d->Ho * d->Wo; }
inline int gemm_K(const diffsal_conv_desc* d) { return d->KH * d->KW * d->Cin; }
inline int rowvec_ld(const diffsal_conv_desc* d) { return d->rowvec_ld > 0 ? d->rowvec_ld : d->Cout; }

// descriptor and operands into the argument struct of a tiled kernel (IgemmArgs, Igemm16Args<T>: the same field names), unsplit so far
template <typename T, typename A>
void fill_tiled_args(A& a, const diffsal_conv_desc* d, const GemmOperands& o) {
  a.in = static_cast<const T*>(o.in); a.w = static_cast<const T*>(o.w); a.bias = o.bias; a.scale = o.scale; a.shift = o.shift;
  a.rowvec = o.rowvec; a.residual = static_cast<const T*>(o.residual); a.out = static_cast<T*>(o.out);
  a.pair = o.in2 ? 1 : 0; a.partial = a.partial2 = nullptr; a.xcd_order = 0;
  a.in2 = static_cast<const T*>(o.in2); a.w2 = static_cast<const T*>(o.w2); a.bias2 = o.bias2; a.out2 = static_cast<T*>(o.out2);
  a.M = static_cast<int>(gemm_M(d)); a.K = gemm_K(d);
  a.H = d->H; a.W = d->W; a.Cin = d->Cin; a.Ho = d->Ho; a.Wo = d->Wo; a.Cout = d->Cout;
  a.KW = d->KW; a.taps = d->KH * d->KW; a.stride_h = d->stride_h; a.stride_w = d->stride_w;
  a.pad_t = d->pad_t; a.pad_l = d->pad_l; a.dil_h = d->dil_h; a.dil_w = d->dil_w; a.act = d->act;
  a.rowvec_ld = o.rowvec_ld; a.linear = is_linear(d);
  a.in_bytes = static_cast<unsigned>(static_cast<long>(d->N) * d->H * d->W * d->Cin * sizeof(T));
  a.w_bytes = static_cast<unsigned>(static_cast<long>(d->Cout) * a.K * sizeof(T));
}

// cfg: gemm_dma's tile configuration; gemm16_dma2's tile (in: 0 its own choice and measured floor, 1 / 2 the 256 x 96 / 192 x 192 tile on
// every shape it can run; _takes leaves the tile chosen); the forced plan of a generic kernel (DIFFSAL_IGEMM*_CFG, < 0: the planner's).
// flag: conv16_*: on every shape the kernel can run, not only where it measured ahead; igemm16: no K split whatever the planner says.
struct Offer { int cfg; bool flag; };
#define DIFFSAL_CANDIDATE(name)                                                                  \
  bool name##_takes(const diffsal_conv_desc* d, const GemmOperands* o, Offer& f);                \
  int name##_launch(const diffsal_conv_desc* d, const GemmOperands& o, const Offer& f, hipStream_t s)
DIFFSAL_CANDIDATE(lin_stream);    // lin_stream.hip: barrier-free streaming kernel for short-K, huge-M fp32 linear layers
DIFFSAL_CANDIDATE(gemm_dma);      // gemm_dma.hip: LDS-DMA staging, 96-wide tiles (fp32; plain products also on 16-bit storage)
DIFFSAL_CANDIDATE(gemm16_dma2);   // gemm16_dma.hip: 16-bit plain products and ReduceTemp's row form, two workgroups per CU
DIFFSAL_CANDIDATE(conv16_dma);    // conv16_dma.hip: 3x3 stride-1 convolutions with an LDS-DMA halo patch, two workgroups per CU
DIFFSAL_CANDIDATE(conv16_halo);   // conv16_halo.hip: LDS-halo kernel for 3x3 stride-1 "same" convolutions
DIFFSAL_CANDIDATE(igemm16);       // igemm16.hip: the generic tiled kernel on bf16 / fp16 storage (takes everything)
#undef DIFFSAL_CANDIDATE
size_t gemm_dma_ws_bytes(const diffsal_conv_desc* d, const Offer& f);
size_t igemm16_ws_bytes(const diffsal_conv_desc* d, const Offer& f);
double gemm_dma_estimate(int cfg, long M, int K, int N);
// gemm_dma.hip: up to four fp32 problems in one launch (o[i]: in, w, bias, out of problem i); _batched: wino4.hip's 36 products (+ an
// optional side product) in one launch, 1 launched, 0 shape not handled, < 0 error
int gemm_dma_group_launch(int n, const diffsal_conv_desc* const* d, const GemmOperands* o, hipStream_t s);
int gemm_dma_batched(const float* a, const float* w, float* out, long M, int K, int N, int batch, long a_bs, long w_bs, long o_bs,
                     hipStream_t s, const float* side_a, const float* side_w, float* side_out, long side_rows);

// Outside the family, the same rule: mvit_pool.hip's head dimension 96 (8 lanes per query, 12 channels per lane), called from
// mvit.hip; attn16_mfma.hip, called from misc.hip (diffsal_attention)
int relpos_project96(const float* q, const float* Rt, const float* Rh, const float* Rw, float* extra, long rows, int qt, int qh,
                     int qw, int kt, int kh, int kw, int E, hipStream_t s);
int relpos_bwd_q96(const float* dE, const float* Rt, const float* Rh, const float* Rw, float* dq, long rows, int qt, int qh,
                   int qw, int kt, int kh, int kw, int accumulate, int E, hipStream_t s);
int try_attention16_mfma(const void* q, const void* k, const void* v, void* o, int N, int Lq, int Lk, int C, int heads, float scale,
                         int dtype, hipStream_t s);

}  // namespace diffsal
