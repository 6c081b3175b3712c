// Plain [M, K] x [N, K]^T products on bf16 / fp16 storage (token GEMMs, tap products, ReduceTemp's row products), two workgroups
// per CU: the plain-product sibling of conv16_dma.hip.
//
// gemm_dma.hip's 16-bit instantiation keeps ONE wavefront per SIMD busy with everything -- DMA issue, fragment reads, barrier --
// and the matrix pipe idles through each of them: 0.17 busy, 0.4-0.6 PF/s at 64 clips whatever the tile (96 x 96 and 192 x 192
// measured equal).  Here, as in conv16_dma.hip:
//   * a workgroup is 4 wavefronts and a 256 x 96 output tile (a wavefront: 64 rows x 96 columns = 2 x 3 accumulators of
//     v_mfma_f32_32x32x16); its LDS -- a three-slot ring of (256 + 96) rows x 64 bytes, 67 KB -- leaves room for a second,
//     independent workgroup per CU, whose matrix work covers this one's DMA issue, barriers, prologue and epilogue;
//   * both operands go memory -> LDS by LDS-DMA, 64-byte rows (one 32-element K chunk) with the four 16-byte slots XOR-swizzled by
//     (row >> 2) & 3 on the source side; rows past M / N are fetched out of range (zeros);
//   * a step is one K chunk: counted wait for the chunk issued two steps ago (every wavefront issues six DMA instructions per step),
//     one barrier, issue the chunk two ahead, 12 MFMAs per wavefront;
//   * epilogue through LDS, 16-byte (or, fp32 output, 32-byte) pieces per lane: bias, affine, per-image vector, activation,
//     residual in the order of the other 16-bit kernels.  Accumulation: K in order, fp32 -- the same sums as igemm16 / gemm_dma.
//
// R/models/saliency_decoder/attention.py:97-111 (proj_q / k / v, proj), common_block.py:125-147 (Mlp), transformer.py:150-157.
#include "gemm_family.h"

namespace diffsal {

template <typename T>
struct GdArgs {
  const T* a;
  const T* w;
  const float* bias;
  const float* scale;
  const float* shift;
  const float* rowvec;
  const T* residual;
  void* out;
  int M, N, K;
  int act, rowvec_ld, rows_per_img, out_f32;
  int tiles_m, tiles_n;
  // row form (ReduceTemp, R/models/saliency_decoder/sal_unet.py:300-318: a (kt, 1) kernel with stride (kt, 1) over [B, T, HW, C] that
  // leaves ONE frame): taps > 1: output row m = (image m / Wrow, position m % Wrow) reads input rows (image, t, position), t < taps;
  // K is ordered (32-channel chunk, tap, channel) as pack_conv_weight leaves it.  taps == 1: the plain product (Hrow = 1)
  int taps, Wrow, Hrow, Cin;
};

// Two tile shapes, four wavefronts each, a wavefront = TM x 3 accumulators of 32 x 32:
//   <2, 1>  256 x 96: the wavefronts stacked along M (64 rows x 96 columns each);
//   <3, 2>  192 x 192: the wavefronts 2 x 2 (96 x 96 each).  Per MFMA a wavefront reads (1 / TM + 1 / 3) KiB of fragments from LDS:
//           0.83 against 0.67 -- at one MFMA per 8 cycles and CU that is 81 % of the LDS's 128 bytes per cycle against 65 %, before the
//           DMA's own LDS writes -- and a tile's L2 -> LDS bytes per flop are 1 / 256 + 1 / 96 against 2 / 192 (-27 %).
// A ring slot holds BM rows of A and BN rows of W, one 32-element K chunk (64 bytes) each; (BM + BN) / 16 DMA instructions per step, shared
// out over the four wavefronts: six per wavefront in both shapes.
template <typename T, int TM, int WN>
__global__ __launch_bounds__(256, 2) void gemm16_dma2_kernel(GdArgs<T> p) {
  typedef typename Mfma32x16<T>::vec vec;
  constexpr int TN = 3, WM = 4 / WN, BM = WM * TM * 32, BN = WN * 96;
  constexpr int kGdSlot = (BM + BN) * 64;
  constexpr int ISS = ((BM + BN) / 16 + 3) / 4;   // DMA instructions per wavefront and step (256 x 96: the last one of waves 2, 3 is dead)
  constexpr int NA = BM / 64;                     // DMA instruction q of a wavefront: q < NA rows of A, else rows of W
  static_assert(BM % 64 == 0 && ISS <= 6, "at most six DMA instructions per wavefront and step");
  constexpr unsigned DEAD = 0x80000000u;
  extern __shared__ __attribute__((aligned(16))) unsigned char gd_smem[];
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  // XCD-aware order: an XCD takes a contiguous run of tiles; N tiles of one row block are neighbours (they share the A rows)
  const int b = xcd_contiguous<int>(gridDim.x);
  const int tn = b % p.tiles_n, tm = b / p.tiles_n;
  const int m0 = tm * BM, n0 = tn * BN;
  const int wm = wave / WN, wn = wave - wm * WN;
  const unsigned lds0 = static_cast<unsigned>(reinterpret_cast<uintptr_t>((lds_ptr_t)gd_smem));
  const unsigned lds_scratch = lds0 + 3 * kGdSlot;
  const int G = p.K >> 5;

  // ---- issue side: A instruction q (q < 4) of a wavefront covers rows (q * 4 + wave) * 16 + (lane >> 2), W instruction q (q < 2) rows
  // (q * 4 + wave) * 16 + (lane >> 2) of the N tile; physical slot lane & 3 receives logical slot (lane & 3) ^ ((row >> 2) & 3)
  // byte offset of output row m's first input row
  auto row_off = [&](int m) __attribute__((always_inline)) -> long {
    const int n = m / p.Wrow, pos = m - n * p.Wrow;
    return (static_cast<long>(n) * p.Hrow * p.Wrow + pos) * p.Cin * 2;
  };
  const long base_off = row_off(m0);
  const long total_b = static_cast<long>((p.M + p.Wrow - 1) / p.Wrow) * p.Hrow * p.Wrow * p.Cin * 2;
  const unsigned long pa = reinterpret_cast<unsigned long>(p.a) + static_cast<unsigned long>(base_off);
  const int rows_a = min(BM, p.M - m0), rows_w = min(BN, p.N - n0);
  const long rec_a = total_b - base_off;
  const i32x4 rs_a = dma_rsrc(pa, static_cast<int>(rec_a < 0x7FFFFFFFL ? rec_a : 0x7FFFFFFFL));
  const unsigned long pw = reinterpret_cast<unsigned long>(p.w + static_cast<long>(n0) * p.K);
  const i32x4 rs_w = dma_rsrc(pw, rows_w * p.K * 2);
  unsigned a_voff[NA], w_voff[ISS - NA];
#pragma unroll
  for (int q = 0; q < NA; ++q) {
    const int row = (q * 4 + wave) * 16 + (lane >> 2), ls = (lane & 3) ^ ((row >> 2) & 3);
    a_voff[q] = row < rows_a ? static_cast<unsigned>(row_off(m0 + row) - base_off + ls * 16) : DEAD;
  }
#pragma unroll
  for (int q = 0; q < ISS - NA; ++q) {
    const int row = (q * 4 + wave) * 16 + (lane >> 2), ls = (lane & 3) ^ ((row >> 2) & 3);
    w_voff[q] = row < rows_w ? static_cast<unsigned>((row * p.K + ls * 8) * 2) : DEAD;     // rows past BN (256 x 96: q = 1, waves 2, 3): past rows_w
  }
  const unsigned tap_stride = static_cast<unsigned>(p.Wrow) * p.Cin * 2u;
  auto issue = [&](int g) __attribute__((always_inline)) {             // K chunk g -> slot g % 3
    const bool live = g < G;
    const unsigned dst = lds0 + (g % 3) * kGdSlot, soff = static_cast<unsigned>(g) * 64u;
    const int ch = g / p.taps, tap = g - ch * p.taps;
    const unsigned soff_a = static_cast<unsigned>(tap) * tap_stride + static_cast<unsigned>(ch) * 64u;
#pragma unroll
    for (int q = 0; q < NA; ++q) dma_piece(live ? dst + (q * 4 + wave) * 1024 : lds_scratch, live ? a_voff[q] : DEAD, rs_a, soff_a);
#pragma unroll
    for (int q = 0; q < ISS - NA; ++q) {
      const bool in_tile = (q * 4 + wave) * 16 < BN;      // 256 x 96: the second W instruction of wavefronts 2, 3 has no rows
      dma_piece(live && in_tile ? dst + BM * 64 + (q * 4 + wave) * 1024 : lds_scratch, live && in_tile ? w_voff[q] : DEAD, rs_w, soff);
    }
  };

  // ---- fragment addressing: lane -> row lp of its 32-row MFMA tile, k half kh; logical slot of (kk, kh) = 2 kk + kh
  const int lp = lane & 31, kh = lane >> 5;
  int a_off[TM][2], b_off[TN][2];
#pragma unroll
  for (int i = 0; i < TM; ++i) {
    const int row = wm * (TM * 32) + i * 32 + lp;
#pragma unroll
    for (int kk = 0; kk < 2; ++kk) a_off[i][kk] = row * 64 + (((kk * 2 + kh) ^ ((row >> 2) & 3)) << 4);
  }
#pragma unroll
  for (int j = 0; j < TN; ++j) {
    const int row = wn * 96 + j * 32 + lp;
#pragma unroll
    for (int kk = 0; kk < 2; ++kk) b_off[j][kk] = BM * 64 + row * 64 + (((kk * 2 + kh) ^ ((row >> 2) & 3)) << 4);
  }

  issue(0);
  issue(1);
  f32x16 acc[TM][TN];
#pragma unroll
  for (int i = 0; i < TM; ++i)
#pragma unroll
    for (int j = 0; j < TN; ++j)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;

  for (int g = 0; g < G; ++g) {
    // this wavefront's pieces of chunk g have landed (the ISS of chunk g + 1 may be in flight) and its LDS reads of step g - 1 have
    // returned (see conv16_dma.hip); after the barrier everybody's have, and slot (g + 2) % 3 is free
    wait_vm_lgkm<ISS, 0>();
    __builtin_amdgcn_s_barrier();
    issue(g + 2);
    const unsigned char* S = gd_smem + (g % 3) * kGdSlot;
    vec fa[2][TM], fb[2][TN];
#pragma unroll
    for (int kk = 0; kk < 2; ++kk) {
#pragma unroll
      for (int i = 0; i < TM; ++i) fa[kk][i] = *reinterpret_cast<const vec*>(S + a_off[i][kk]);
#pragma unroll
      for (int j = 0; j < TN; ++j) fb[kk][j] = *reinterpret_cast<const vec*>(S + b_off[j][kk]);
    }
#pragma unroll
    for (int kk = 0; kk < 2; ++kk)
#pragma unroll
      for (int i = 0; i < TM; ++i)
#pragma unroll
        for (int j = 0; j < TN; ++j) acc[i][j] = Mfma32x16<T>::run(fb[kk][j], fa[kk][i], acc[i][j]);   // D^T: rows = columns of out, cols = rows of out
  }
  asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");
  __builtin_amdgcn_s_barrier();

  // ---- epilogue through LDS: per 32-row tile a wavefront parks [32 rows][96 + 4] fp32 in its own 12.8 KB and reads back
  // (row, column octet) items
  float* stage = reinterpret_cast<float*>(gd_smem) + wave * (32 * 100);
  const T* __restrict__ resid = p.residual;
#pragma unroll
  for (int i = 0; i < TM; ++i) {
    // the residual octets of this row tile are requested before the sums are parked (a round trip under the LDS traffic)
    uint4 rraw[6];
    if (resid) {
#pragma unroll
      for (int it = 0; it < 6; ++it) {
        const int item = it * 64 + lane;
        const int rr = item / 12, oc = item - rr * 12;
        const int n = n0 + wn * 96 + oc * 8, m = m0 + wm * (TM * 32) + i * 32 + rr;
        rraw[it] = (m < p.M && n < p.N) ? *reinterpret_cast<const uint4*>(resid + static_cast<long>(m) * p.N + n) : make_uint4(0, 0, 0, 0);
      }
    }
#pragma unroll
    for (int j = 0; j < TN; ++j)
#pragma unroll
      for (int q = 0; q < 4; ++q)
        st4(stage + lp * 100 + j * 32 + q * 8 + kh * 4, make_float4(acc[i][j][4 * q], acc[i][j][4 * q + 1], acc[i][j][4 * q + 2], acc[i][j][4 * q + 3]));
#pragma unroll
    for (int it = 0; it < 6; ++it) {
      const int item = it * 64 + lane;            // 32 rows x 12 octets
      const int rr = item / 12, oc = item - rr * 12;
      const int n = n0 + wn * 96 + oc * 8, m = m0 + wm * (TM * 32) + i * 32 + rr;
      const float4 s0 = ld4(stage + rr * 100 + oc * 8), s1 = ld4(stage + rr * 100 + oc * 8 + 4);
      if (m >= p.M || n >= p.N) continue;
      float v[8] = {s0.x, s0.y, s0.z, s0.w, s1.x, s1.y, s1.z, s1.w};
      epi_channels(v, p.bias, p.scale, p.shift, p.rowvec, [&] { return static_cast<long>(m / p.rows_per_img) * p.rowvec_ld; }, n);
      epi_act(v, p.act);
      const long o = static_cast<long>(m) * p.N + n;
      if (resid) epi_add(v, ld8(reinterpret_cast<const T*>(&rraw[it])).v);
      if (p.out_f32) {
        float* of = static_cast<float*>(p.out) + o;
        st4(of, make_float4(v[0], v[1], v[2], v[3]));
        st4(of + 4, make_float4(v[4], v[5], v[6], v[7]));
      } else {
        f8v ov;
#pragma unroll
        for (int e = 0; e < 8; ++e) ov.v[e] = v[e];
        st8(static_cast<T*>(p.out) + o, ov);
      }
    }
  }
}

// the row form (ReduceTemp): taps > 1 rows of one image feed an output row
static bool gd_rowform(const diffsal_conv_desc* d) { return d->KH > 1 && d->Ho == 1 && d->KH <= d->H; }   // one output frame: the stride does not matter

// f.cfg in: 0 the choice below, 1 / 2 the 256 x 96 / 192 x 192 tile on every shape it can run (DIFFSAL_GEMM_DMA16 = 3 / 4); out: the tile.
// false: not mine (the caller goes on to the other kernels).
bool gemm16_dma2_takes(const diffsal_conv_desc* d, const GemmOperands* o, Offer& f) {
  const int tile = f.cfg;
  const long M = gemm_M(d);
  const int K = gemm_K(d), N = d->Cout;
  if (d->dtype == DIFFSAL_F32 || d->KW != 1 || d->stride_w != 1 || d->pad_t != 0 || d->pad_l != 0 || d->dil_h != 1 || d->Wo != d->W) return 0;
  const bool plain = d->KH == 1 && d->stride_h == 1 && d->Ho == d->H;
  const bool rowform = gd_rowform(d);
  if (!plain && !rowform) return 0;
  const long in_bytes = static_cast<long>(d->N) * d->H * d->W * d->Cin * 2;
  if (K % 32 != 0 || d->Cin % 32 != 0 || K < 64 || N % 8 != 0 || M <= 0 || M >= (1L << 31) || 256L * K * 2 >= (1L << 31) || 96L * K * 2 >= (1L << 31))
    return 0;
  // row form: a tile's A rows are addressed with 32-bit byte offsets from the first image the tile touches, and BM consecutive output
  // rows span up to BM / W + 2 images (256 covers both tile heights)
  if (rowform && ((256 / d->W + 2) * (static_cast<long>(d->H) * d->W * d->Cin * 2) >= (1L << 31) || in_bytes >= (1L << 40))) return 0;
  if (o && (o->in2 || (o->out_f32 && o->residual) || !aligned16(o->in) || !aligned16(o->w) || !aligned16(o->out) || !aligned16(o->bias) || !aligned16(o->scale) || !aligned16(o->shift) ||
        !aligned16(o->rowvec) || !aligned16(o->residual) || (o->rowvec && o->rowvec_ld % 4 != 0) || ((o->scale == nullptr) != (o->shift == nullptr))))
    return false;
  const long tiles = ((M + 255) / 256) * ((N + 95) / 96);
  if (tiles >= (1L << 31)) return 0;
  // 192 x 192 tiles: from 400 tiles on (measured at 4 .. 64 clips: faster than
  // both the 256 x 96 tiles and gemm_dma.hip's 96 x 96 ones from ~500 tiles, slower at ~250), unless a quarter of the last tile column
  // lies past N -- or any of it on a short K walk (N = 864, K = 192: 70 -> 78 us; K = 768: 1006 -> 885)
  const long tiles_sq = ((M + 191) / 192) * ((N + 191) / 192);
  const int n_waste = ((N + 191) / 192) * 192 - N;
  const bool square = tile == 2 || (tile != 1 && tiles_sq >= 400 && (n_waste == 0 || (n_waste <= N / 4 && K >= 384)));
  // 256 x 96: from a chip's worth of tiles (two workgroups per CU) on; below that gemm_dma.hip's 96 x 96 tiles (and their K split) fill
  // the chip better
  if (!square && tile != 1 && tiles < 512) return 0;
  f.cfg = square ? 2 : 1;
  return true;
}

int gemm16_dma2_launch(const diffsal_conv_desc* d, const GemmOperands& o, const Offer& f, hipStream_t s) {
  const long M = gemm_M(d);
  const int K = gemm_K(d), N = d->Cout;
  const bool rowform = gd_rowform(d), square = f.cfg == 2;
  const int bm = square ? 192 : 256, bn = square ? 192 : 96;
  const size_t lds = 3 * static_cast<size_t>(bm + bn) * 64 + 1024;
#define GD_LAUNCH(T, TM_, WN_)                                                                                              \
  do {                                                                                                                      \
    GdArgs<T> g{static_cast<const T*>(o.in), static_cast<const T*>(o.w), o.bias, o.scale, o.shift, o.rowvec, static_cast<const T*>(o.residual), o.out, \
                static_cast<int>(M), N, K, d->act, o.rowvec_ld, d->Ho * d->Wo, o.out_f32 ? 1 : 0, static_cast<int>((M + bm - 1) / bm), (N + bn - 1) / bn, \
                rowform ? d->KH : 1, rowform ? d->W : static_cast<int>(M), rowform ? d->H : 1, d->Cin};                        \
    DS_RAISE_DYNAMIC_LDS((gemm16_dma2_kernel<T, TM_, WN_>), 160 * 1024);                                                    \
    hipLaunchKernelGGL((gemm16_dma2_kernel<T, TM_, WN_>), dim3(static_cast<unsigned>(g.tiles_m) * g.tiles_n), dim3(256), lds, s, g); \
  } while (0)
  if (square) {
    if (d->dtype == DIFFSAL_BF16) GD_LAUNCH(__bf16, 3, 2); else GD_LAUNCH(_Float16, 3, 2);
  } else {
    if (d->dtype == DIFFSAL_BF16) GD_LAUNCH(__bf16, 2, 1); else GD_LAUNCH(_Float16, 2, 1);
  }
#undef GD_LAUNCH
  note_kernel("gemm16_dma2_kernel<%s> [%dx%d tile, LDS-DMA, 2 workgroups per CU]", d->dtype == DIFFSAL_BF16 ? "__bf16" : "_Float16", bm, bn);
  return check_launch("diffsal_conv_igemm(16-bit DMA, 2 per CU)");
}

}  // namespace diffsal
