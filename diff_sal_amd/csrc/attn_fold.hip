// Attention of a TransformerBlock with proj_q and proj folded onto the key side (fp32 storage, exact fp32 arithmetic, 2 heads, up to
// 32 pooled keys per frame): R/models/saliency_decoder/attention.py:86-113, transformer.py:150-152.
//
//   per frame n, head h:  G_h = kp Wkq_h   [Lk x C]     U_h = vp Wvp_h   [Lk x C]      (one paired GEMM before this kernel, N = 2C)
//   per token:            S_h = scale (q_in G_h^T + s0_h);  P_h = softmax(S_h);  x1 = x + bp' + sum_h P_h U_h
//
// q, k, v and o of the reference are never formed: see SalUNet.packed() for the weight-only folds and tools/attn_fold_algebra.py for
// the algebra.  s0_h[key] = kp[key] . ukq_h is computed in the workgroup's prologue on the VALU (2 Lk dot products of length C by
// 256 threads) rather than as an extra column block of the pair product: 2 C + 2 output columns would cost that GEMM a whole
// extra 96-wide tile column.
//
// Everything is transposed, as in block_front's phase D (tblock.hip): with v_mfma_f32_16x16x4_f32 the score product
// S^T = G q_in^T [2 Lk x tokens] leaves a lane with rows 4 g + i (g = lane / 16, i = register) of a 16-row block for token lane % 16,
// and the B operand of the output product X1^T = U^T P^T wants row k = g of a 4-row K step in the same lane.  The M row 4 g + i of
// score block b is therefore given the LOGICAL row 16 b + 4 i + g (head-major: row = h Lk + key), so that register i of block b is
// K step 4 b + i of the output product as it stands: P never leaves the registers, and the 2 x 18 keys of the shipped shapes are
// three score blocks and exactly nine K steps.  Score rows beyond 2 Lk are masked to -inf (weight 0) and their U operands are zero.
//
// Work split.  A wave owns 16 NT tokens and a 192-channel slice: C / 192 waves share one token group -- each takes its slice of the
// score contraction, the partial scores are summed through LDS in wave order (a fixed order per token: results do not depend on N,
// on the grid or on NT), every wave of the group repeats the small softmax, then writes its own 192 output channels.  So at
// C = 768 a workgroup is 16 NT tokens, at C = 192 it is 64 NT, and stage 0 of the headline batch (36 frames of 84 tokens) is 216
// workgroups.  No wave shares an operand element with another, so G, U and q_in go from L2 / HBM straight into the MFMA operand
// registers as 16-byte pieces (64 contiguous bytes per row and instruction): an LDS ring would only add a copy.  What the kernel
// waits for is memory latency, not bandwidth (a workgroup's chain of dependent loads; 2 workgroups per CU at most), so the loads
// of each phase are issued in batches ahead of their use: first form 47 / 55 / 66 us at the three stages of B = 4, batched 19 / 22 / 35.
// The 16 contraction channels of a 16-byte group are dealt to the K steps as (piece g, element j) for A and B alike; output
// channels are dealt to the four M blocks of a 64-channel pass so that a lane loads U, loads x and stores x1 as float4 and a store
// instruction writes 64 contiguous bytes per token.  Workgroups of a frame are contiguous in the XCD order: G_n / U_n are re-read
// from one L2.
#include "common.h"

namespace diffsal {
namespace {

typedef float f32x4 __attribute__((ext_vector_type(4)));

constexpr int kSlice = 192;      // channels of a wave: contraction slice of the score product, output slice of the second product
constexpr int kMaxBlocks = 4;    // 16-row score blocks: 2 * 32 keys
// 32 tokens per wave (two column blocks per A operand: half the G / U reads per token) from this many 16-token workgroups on.
// Measured at 36 / 72 frames: 396 workgroups of C = 384 27.1 -> 22.7 us, 756 of C = 192 37.2 -> 34.1, 432 of C = 768 27.2 -> 22.8
constexpr long kTwoBlockMinWgs = 300;

struct AttnFoldArgs {
  const float *q_in, *G, *U, *kp, *ukq, *x, *bias;
  float* out;
  int L, Lk, tiles;      // tokens per frame, keys per frame and head, workgroups per frame
  unsigned nwg;
  float scale;
};

__device__ __forceinline__ float4 zero4() { return make_float4(0.f, 0.f, 0.f, 0.f); }
__device__ __forceinline__ float el(const float4& v, int j) { return j == 0 ? v.x : j == 1 ? v.y : j == 2 ? v.z : v.w; }

template <int C, int NB, int NT>      // NB: 16-row score blocks (2 Lk <= 16 NB), NT: 16-token column blocks of a wave
__global__ __launch_bounds__(256) void attn_fold_kernel(const AttnFoldArgs a) {
  constexpr int WS = C / kSlice;            // waves that share a token group
  constexpr int TG = 4 / WS;                // token groups of a workgroup
  static_assert(C % kSlice == 0 && (WS == 1 || WS == 2 || WS == 4), "C = 192, 384 or 768");
  static_assert(NB >= 1 && NB <= kMaxBlocks, "at most 64 score rows");
  __shared__ float s0_lds[16 * NB];
  __shared__ f32x4 red[WS > 1 ? 4 * NB * NT * kWave : 1];

  const int tid = threadIdx.x, lane = tid & 63, wave = uniform_i(tid >> 6);
  const int m = lane & 15, g = lane >> 4;
  const int v = static_cast<int>(xcd_contiguous<unsigned>(a.nwg));
  const int n = v / a.tiles, tile = v - n * a.tiles;
  const int L = a.L, Lk = a.Lk, R = 2 * Lk;
  const int ks = (R + 3) >> 2;
  const int tgi = wave / WS, wsi = wave - tgi * WS;
  const int tok0 = (tile * TG + tgi) * 16 * NT;
  const size_t C2 = 2 * static_cast<size_t>(C);
  const float* Gn = a.G + static_cast<size_t>(n) * Lk * C2;
  const float* Un = a.U + static_cast<size_t>(n) * Lk * C2;
  // The kernel is latency-bound (one or two workgroups per CU at the shipped shapes), so every load is unconditional and the loads
  // of a phase are issued in batches ahead of their use, the next batch before the MFMAs of the current one.  A padded row reads
  // the last real row instead: in the score product its result is a padded score row, masked below; in the output product the
  // operand is zeroed after the load.
  auto row_off = [&](int lr) {              // element offset of logical row lr (head-major) inside G_n / U_n
    lr = min(lr, R - 1);
    const int h = lr >= Lk ? 1 : 0;
    return (lr - h * Lk) * C2 + h * C;
  };

  // ---- S^T partial over this wave's contraction slice: operand pointers and the first batch of 16-channel groups
  constexpr int GB = (NB + NT <= 4) ? 4 : 2, NBAT = kSlice / 16 / GB;
  const float* grow[NB];
#pragma unroll
  for (int b = 0; b < NB; ++b) grow[b] = Gn + row_off(16 * b + 4 * (m & 3) + (m >> 2)) + wsi * kSlice + 4 * g;
  const float* qrow[NT];
#pragma unroll
  for (int tb = 0; tb < NT; ++tb) {
    const int t = min(tok0 + tb * 16 + m, L - 1);      // tail: a valid row, never stored
    qrow[tb] = a.q_in + (static_cast<size_t>(n) * L + t) * C + wsi * kSlice + 4 * g;
  }
  float4 av[2][GB][NB], bv[2][GB][NT];
#define FOLD_LOAD_BATCH(BUF, BI)                                                              \
  _Pragma("unroll") for (int gi = 0; gi < GB; ++gi) {                                         \
    _Pragma("unroll") for (int b = 0; b < NB; ++b) av[BUF][gi][b] = ld4(grow[b] + ((BI) * GB + gi) * 16);   \
    _Pragma("unroll") for (int tb = 0; tb < NT; ++tb) bv[BUF][gi][tb] = ld4(qrow[tb] + ((BI) * GB + gi) * 16); \
  }
  FOLD_LOAD_BATCH(0, 0)

  // ---- s0[h Lk + key] = kp[n, key] . ukq[h]: C / 12 lanes per key, three interleaved 16-byte pieces per lane, both heads per load
  {
    constexpr int LPR = C / 12, RPW = kWave / LPR;      // lanes per key (16 / 32 / 64), keys of a wave per step
    constexpr int ITS = (8 * NB + 4 * RPW - 1) / (4 * RPW);      // Lk <= 8 NB keys, 4 RPW per step
    const int li = lane % LPR, rsub = lane / LPR;
    float4 u4[2][3], k4[ITS][3];
#pragma unroll
    for (int h = 0; h < 2; ++h)
#pragma unroll
      for (int j = 0; j < 3; ++j) u4[h][j] = ld4(a.ukq + h * C + (j * LPR + li) * 4);
#pragma unroll
    for (int it = 0; it < ITS; ++it) {
      const int key = min((it * 4 + wave) * RPW + rsub, Lk - 1);
#pragma unroll
      for (int j = 0; j < 3; ++j) k4[it][j] = ld4(a.kp + (static_cast<size_t>(n) * Lk + key) * C + (j * LPR + li) * 4);
    }
    __builtin_amdgcn_sched_barrier(0);
    float part[ITS][2];
#pragma unroll
    for (int it = 0; it < ITS; ++it)
#pragma unroll
      for (int h = 0; h < 2; ++h) {
        float p = 0.f;
#pragma unroll
        for (int j = 0; j < 3; ++j) {
          p = fmaf(k4[it][j].x, u4[h][j].x, p);
          p = fmaf(k4[it][j].y, u4[h][j].y, p);
          p = fmaf(k4[it][j].z, u4[h][j].z, p);
          p = fmaf(k4[it][j].w, u4[h][j].w, p);
        }
        part[it][h] = group_sum<LPR>(p);
      }
    if (li == 0) {
#pragma unroll
      for (int it = 0; it < ITS; ++it) {
        const int key = (it * 4 + wave) * RPW + rsub;
        if (key < Lk) {
          s0_lds[key] = part[it][0];
          s0_lds[Lk + key] = part[it][1];
        }
      }
    }
  }

  f32x4 s[NB][NT];
#pragma unroll
  for (int b = 0; b < NB; ++b)
#pragma unroll
    for (int tb = 0; tb < NT; ++tb) s[b][tb] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int bi = 0; bi < NBAT; ++bi) {
    if (bi + 1 < NBAT) {
      if (bi & 1) { FOLD_LOAD_BATCH(0, bi + 1) } else { FOLD_LOAD_BATCH(1, bi + 1) }
    }
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int gi = 0; gi < GB; ++gi)
#pragma unroll
      for (int j = 0; j < 4; ++j)
#pragma unroll
        for (int b = 0; b < NB; ++b)
#pragma unroll
          for (int tb = 0; tb < NT; ++tb)
            s[b][tb] = __builtin_amdgcn_mfma_f32_16x16x4f32(el(av[bi & 1][gi][b], j), el(bv[bi & 1][gi][tb], j), s[b][tb], 0, 0, 0);
  }
#undef FOLD_LOAD_BATCH

  // ---- operands of the first output pass: in flight across the barrier and the softmax
  // X1^T = U^T P^T on this wave's 192 output channels, 64 per pass; M block j, row mm holds channel 16 (mm & 3) + 4 (mm >> 2) + j
  const int coff = 16 * (m & 3) + 4 * (m >> 2);
  const float* urow[4 * NB];
#pragma unroll
  for (int kk = 0; kk < 4 * NB; ++kk) urow[kk] = Un + row_off(4 * kk + g) + wsi * kSlice + coff;
  size_t xoff[NT];
#pragma unroll
  for (int tb = 0; tb < NT; ++tb) xoff[tb] = (static_cast<size_t>(n) * L + min(tok0 + tb * 16 + m, L - 1)) * C + wsi * kSlice + 4 * g;
  float4 u4[4 * NB], xr[2][NT][4];      // U is re-loaded behind each pass's MFMAs (a second buffer costs a wave per SIMD), x one pass ahead
#define FOLD_LOAD_U(PASS) \
  _Pragma("unroll") for (int kk = 0; kk < 4 * NB; ++kk) u4[kk] = ld4(urow[kk] + (PASS) * 64);
#define FOLD_LOAD_X(BUF, PASS)                      \
  _Pragma("unroll") for (int tb = 0; tb < NT; ++tb) \
    _Pragma("unroll") for (int i = 0; i < 4; ++i) xr[BUF][tb][i] = ld4(a.x + xoff[tb] + (PASS) * 64 + 16 * i);
  FOLD_LOAD_U(0)
  FOLD_LOAD_X(0, 0)

  // ---- sum the slices in wave order
  if constexpr (WS > 1) {
#pragma unroll
    for (int b = 0; b < NB; ++b)
#pragma unroll
      for (int tb = 0; tb < NT; ++tb) red[((wave * NB + b) * NT + tb) * kWave + lane] = s[b][tb];
  }
  __syncthreads();
  if constexpr (WS > 1) {
#pragma unroll
    for (int b = 0; b < NB; ++b)
#pragma unroll
      for (int tb = 0; tb < NT; ++tb) {
        f32x4 t = red[(((tgi * WS) * NB + b) * NT + tb) * kWave + lane];
#pragma unroll
        for (int w = 1; w < WS; ++w) t += red[(((tgi * WS + w) * NB + b) * NT + tb) * kWave + lane];
        s[b][tb] = t;
      }
  }

  // ---- softmax per head over its Lk logical rows; register i of block b is logical row 16 b + 4 i + g
  {
    float s0[NB][4];
#pragma unroll
    for (int b = 0; b < NB; ++b)
#pragma unroll
      for (int i = 0; i < 4; ++i) s0[b][i] = s0_lds[min(16 * b + 4 * i + g, R - 1)];
    const float ninf = -__builtin_inff();
#pragma unroll
    for (int tb = 0; tb < NT; ++tb) {
      float mx0 = ninf, mx1 = ninf;
#pragma unroll
      for (int b = 0; b < NB; ++b)
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          const int lr = 16 * b + 4 * i + g;
          const float val = (s[b][tb][i] + s0[b][i]) * a.scale;
          s[b][tb][i] = val;
          mx0 = lr < Lk ? fmaxf(mx0, val) : mx0;
          mx1 = (lr >= Lk && lr < R) ? fmaxf(mx1, val) : mx1;
        }
      mx0 = fmaxf(mx0, lane_xor16(mx0));
      mx0 = fmaxf(mx0, lane_xor32(mx0));
      mx1 = fmaxf(mx1, lane_xor16(mx1));
      mx1 = fmaxf(mx1, lane_xor32(mx1));
      float sum0 = 0.f, sum1 = 0.f;
#pragma unroll
      for (int b = 0; b < NB; ++b)
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          const int lr = 16 * b + 4 * i + g;
          const float e = lr < R ? expf(s[b][tb][i] - (lr < Lk ? mx0 : mx1)) : 0.f;      // padded rows: -inf, i.e. weight 0
          s[b][tb][i] = e;
          sum0 += lr < Lk ? e : 0.f;
          sum1 += lr < Lk ? 0.f : e;
        }
      sum0 += lane_xor16(sum0);
      sum0 += lane_xor32(sum0);
      sum1 += lane_xor16(sum1);
      sum1 += lane_xor32(sum1);
#pragma unroll
      for (int b = 0; b < NB; ++b)
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          const int lr = 16 * b + 4 * i + g;
          s[b][tb][i] = s[b][tb][i] / (lr < Lk ? sum0 : sum1);
        }
    }
  }

  // ---- the output passes
#pragma unroll
  for (int pass = 0; pass < kSlice / 64; ++pass) {
    if (pass + 1 < kSlice / 64) {
      if (pass & 1) { FOLD_LOAD_X(0, pass + 1) } else { FOLD_LOAD_X(1, pass + 1) }
    }
    float4 bb[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) bb[i] = ld4(a.bias + wsi * kSlice + pass * 64 + 16 * i + 4 * g);
    __builtin_amdgcn_sched_barrier(0);
    f32x4 acc[4][NT];
#pragma unroll
    for (int j = 0; j < 4; ++j)
#pragma unroll
      for (int tb = 0; tb < NT; ++tb) acc[j][tb] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int kk = 0; kk < 4 * NB; ++kk)
      if (kk < ks) {
        const float4 uu = 4 * kk + g < R ? u4[kk] : zero4();
#pragma unroll
        for (int j = 0; j < 4; ++j)
#pragma unroll
          for (int tb = 0; tb < NT; ++tb)
            acc[j][tb] = __builtin_amdgcn_mfma_f32_16x16x4f32(el(uu, j), s[kk >> 2][tb][kk & 3], acc[j][tb], 0, 0, 0);
      }
    __builtin_amdgcn_sched_barrier(0);
    if (pass + 1 < kSlice / 64) { FOLD_LOAD_U(pass + 1) }
    // register i of M block j: channel 64 pass + 16 i + 4 g + j of the slice, token m
#pragma unroll
    for (int tb = 0; tb < NT; ++tb)
      if (tok0 + tb * 16 + m < L) {
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          const float4 xv = xr[pass & 1][tb][i];
          float4 o;
          o.x = acc[0][tb][i] + bb[i].x + xv.x;
          o.y = acc[1][tb][i] + bb[i].y + xv.y;
          o.z = acc[2][tb][i] + bb[i].z + xv.z;
          o.w = acc[3][tb][i] + bb[i].w + xv.w;
          st4(a.out + xoff[tb] + pass * 64 + 16 * i, o);
        }
      }
  }
#undef FOLD_LOAD_U
#undef FOLD_LOAD_X
}

template <int C, int NB>
void launch_fold(const AttnFoldArgs& a, int N, hipStream_t s) {
  constexpr int TG = 4 / (C / kSlice);
  AttnFoldArgs b = a;
  const long wg1 = static_cast<long>(N) * ((a.L + 16 * TG - 1) / (16 * TG));
  if (wg1 >= kTwoBlockMinWgs) {
    b.tiles = (a.L + 32 * TG - 1) / (32 * TG);
    b.nwg = static_cast<unsigned>(N) * b.tiles;
    hipLaunchKernelGGL((attn_fold_kernel<C, NB, 2>), dim3(b.nwg), dim3(256), 0, s, b);
  } else {
    b.tiles = (a.L + 16 * TG - 1) / (16 * TG);
    b.nwg = static_cast<unsigned>(N) * b.tiles;
    hipLaunchKernelGGL((attn_fold_kernel<C, NB, 1>), dim3(b.nwg), dim3(256), 0, s, b);
  }
}

template <int C>
void launch_fold_c(const AttnFoldArgs& a, int N, hipStream_t s) {
  switch ((2 * a.Lk + 15) / 16) {
    case 1: return launch_fold<C, 1>(a, N, s);
    case 2: return launch_fold<C, 2>(a, N, s);
    case 3: return launch_fold<C, 3>(a, N, s);
    default: return launch_fold<C, 4>(a, N, s);
  }
}

}  // namespace
}  // namespace diffsal

extern "C" int diffsal_attn_fold(const float* q_in, const float* G, const float* U, const float* kp, const float* ukq, const float* x,
                                 const float* bias, float* out, int N, int L, int Lk, int C, int heads, float scale,
                                 diffsal_stream_t stream) {
  using namespace diffsal;
  DS_REQUIRE(q_in && G && U && kp && ukq && x && bias && out, DIFFSAL_E_ARG, "attn_fold: null argument");
  DS_REQUIRE(heads == 2 && Lk >= 1 && Lk <= 32 && (C == 192 || C == 384 || C == 768), DIFFSAL_E_SHAPE,
             "attn_fold: heads=%d Lk=%d C=%d: built for 2 heads, 1..32 keys, C = 192 / 384 / 768", heads, Lk, C);
  DS_REQUIRE(N >= 1 && L >= 1 && static_cast<long>(N) * ((L + 15) / 16) < (1L << 30), DIFFSAL_E_SHAPE, "attn_fold: N=%d L=%d", N, L);
  DS_REQUIRE(aligned16(q_in) && aligned16(G) && aligned16(U) && aligned16(kp) && aligned16(ukq) && aligned16(x) && aligned16(bias) &&
                 aligned16(out), DIFFSAL_E_ALIGN, "attn_fold: misaligned pointer");
  AttnFoldArgs a{q_in, G, U, kp, ukq, x, bias, out, L, Lk, 0, 0u, scale};
  hipStream_t s = static_cast<hipStream_t>(stream);
  if (C == 192) launch_fold_c<192>(a, N, s);
  else if (C == 384) launch_fold_c<384>(a, N, s);
  else launch_fold_c<768>(a, N, s);
  return check_launch("attn_fold");
}
