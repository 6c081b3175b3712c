// From decoded uint8 frames in device memory to the clip tensor VideoSaliencyModel.forward hands to MViT: the host pipeline of
// R/datasets/saliency_db.py:29-36 (pil_loader: Image.resize to 320 x 240, Pillow's default bicubic), :292-296 (Scale bilinear,
// ToTensor, Normalize), :382-394 (stack, permute) and R/datasets/meta_data.py:27-35, R/datasets/dhf1k_data.py:72-81 (Resize on a
// PIL image, ToTensor, Normalize).  include/diffsal.h ("video front end") states the arithmetic.  Pillow's 8-bit resample is
// integer work (22-bit fixed-point coefficients the HOST builds in float64, an int32 accumulator, an arithmetic shift, a clip, a
// uint8 image between the horizontal and the vertical pass), so the result is bit-equal to Pillow's, not merely close.
//   rs_fused_kernel   one launch per resize.  A workgroup owns a band of output rows over the full output width: it brings the
//                     source rows the band needs into LDS a few rows at a time (16-byte loads over the aligned body of the
//                     chunk, single bytes for its head and tail), resamples them horizontally into a uint8 LDS image and runs the
//                     vertical pass out of that image.  The intermediate image never reaches HBM.  Both coefficient tables are
//                     staged (and their bounds clamped) in LDS once per workgroup.  Adjacent bands overlap by the vertical
//                     support and redo that much horizontal work; rs_plan picks the band height from the LDS budget.
//   rs_h_kernel, rs_v_kernel   the two passes through an HBM workspace [N][H0][W1][C]: the form for sizes where not even a band
//                     of one output row fits in LDS; an axis whose size does not change runs no pass in either form.
//   rs_*_groups_kernel   the same three bodies (rs_fused_body, rs_h_body, rs_v_body) over frames of several source sizes: a
//                     workgroup finds its (group, frame, band or tile) through a prefix table of the groups' workgroup counts, and
//                     a dst table names the output frame of every input frame (diffsal_resample_u8_groups: at most one launch per
//                     form however many sizes a shuffled training batch holds).  The kernels above are the one-group callers.
//   vg_gather_kernel  uint8 [N][h][w][C] + index table [B][T] + look-up table [C][256] -> fp32 [B][C][T][h][w], 16-byte stores.
// The tables live in device memory and cannot be checked by the host: every bound read from them is clamped to the source, the
// tap count to the table's width and the band's row span to the LDS image, so a wrong table gives wrong pixels and no access
// outside the buffers.  No atomics, no allocation, no synchronisation: two calls give the same bits, graph-safe.
#include <cmath>

#include "common.h"

namespace diffsal {

constexpr int RS_THREADS = 512;
constexpr int RS_PREC = 22;                        // Pillow's PRECISION_BITS = 32 - 8 - 2
constexpr int RS_MAX_BAND = 32;
constexpr long RS_STAGE_BYTES = 16384;             // source rows brought into LDS per round
constexpr long RS_LDS_MAX = 160 * 1024;            // LDS a gfx950 workgroup can have
constexpr int RS_MAX_SIDE = 16384;

__device__ __forceinline__ int rs_clampi(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }
// clip8 of Pillow: (acc >> 22) clipped to 0 .. 255; the shift is arithmetic
__device__ __forceinline__ unsigned rs_clip8(int acc) { return static_cast<unsigned>(rs_clampi(acc >> RS_PREC, 0, 255)); }
// a pixel (0 .. 255) times a coefficient (|k| < 2^23 for any normalised filter row): the 24-bit multiply-add
__device__ __forceinline__ int rs_mad(unsigned p, int k, int acc) { return __mul24(static_cast<int>(p), k) + acc; }

// (xmin, count) of output index o as the kernels use it: inside the source and inside the table row
__device__ __forceinline__ void rs_bounds(const int* __restrict__ b, int o, int n_in, int ks, int& lo, int& cnt) {
  lo = rs_clampi(b[2 * o], 0, n_in - 1);
  const int room = n_in - lo < ks ? n_in - lo : ks;
  cnt = rs_clampi(b[2 * o + 1], 0, room);
}

// Output frame of a group's frame n: the group's slice of the dst table (in device memory, so the host could not check it: clamped
// to the output's slots), or n itself where the group's frames are consecutive in the output.
__device__ __forceinline__ long rs_slot(const int* __restrict__ dst, int nslots, long n) {
  return dst ? static_cast<long>(rs_clampi(dst[n], 0, nslots - 1)) : n;
}

// Horizontal pass of output pixel idx of in [rows][W0][C] -> out [..][W1][C].  The frames have Hf rows each and frame n goes to
// frame rs_slot(n) of out; xb = NULL: the width does not change and the pixel is copied.
template <int C>
__device__ __forceinline__ void rs_h_body(const unsigned char* __restrict__ in, long rows, int W0, int W1, const int* __restrict__ xb,
                                          const int* __restrict__ xk, int xks, unsigned char* __restrict__ out, long idx, int Hf,
                                          const int* __restrict__ dst, int nslots) {
  if (idx >= rows * W1) return;
  const long y = idx / W1;
  const int xo = static_cast<int>(idx - y * W1);
  long oidx = idx;
  if (dst) {
    const long n = y / Hf;
    oidx = (rs_slot(dst, nslots, n) * Hf + (y - n * Hf)) * W1 + xo;
  }
  if (!xb) {
#pragma unroll
    for (int c = 0; c < C; ++c) out[oidx * C + c] = in[idx * C + c];
    return;
  }
  int lo, cnt;
  rs_bounds(xb, xo, W0, xks, lo, cnt);
  const unsigned char* src = in + (y * W0 + lo) * C;
  const int* k = xk + static_cast<long>(xo) * xks;
  int acc[C];
#pragma unroll
  for (int c = 0; c < C; ++c) acc[c] = 1 << (RS_PREC - 1);
  for (int t = 0; t < cnt; ++t) {
    const int kv = k[t];
#pragma unroll
    for (int c = 0; c < C; ++c) acc[c] = rs_mad(src[t * C + c], kv, acc[c]);
  }
#pragma unroll
  for (int c = 0; c < C; ++c) out[oidx * C + c] = static_cast<unsigned char>(rs_clip8(acc[c]));
}

template <int C>
__global__ __launch_bounds__(256) void rs_h_kernel(const unsigned char* __restrict__ in, long rows, int W0, int W1,
                                                   const int* __restrict__ xb, const int* __restrict__ xk, int xks,
                                                   unsigned char* __restrict__ out) {
  rs_h_body<C>(in, rows, W0, W1, xb, xk, xks, out, static_cast<long>(blockIdx.x) * 256 + threadIdx.x, 1, nullptr, 0);
}

// four accumulators from one packed word of four bytes
__device__ __forceinline__ void rs_mad4(unsigned w, int k, int (&acc)[4]) {
  acc[0] = rs_mad(w & 255u, k, acc[0]);
  acc[1] = rs_mad((w >> 8) & 255u, k, acc[1]);
  acc[2] = rs_mad((w >> 16) & 255u, k, acc[2]);
  acc[3] = rs_mad(w >> 24, k, acc[3]);
}
// bytes x .. x + 3 of a row of WB bytes (those past the row's end: not written), as one word when the row allows it
__device__ __forceinline__ void rs_store4(unsigned char* row, int x, int WB, const int (&acc)[4], bool vec) {
  if (vec && x + 4 <= WB) {
    // The first byte is kept opaque until the word is put together.  Left to itself the compiler folds clip8(a) | clip8(b) << 8 into
    // one v_ashr_pk_u8_i32 and then ORs its whole destination register into the word, but the instruction writes 16 bits and leaves
    // the upper half as it was: the word was right only where the register allocator had left zeros there (seen on an MI355X:
    // bits 16 .. 31 of acc[0] in bytes 2 and 3 of every word, once the kernel's body moved into a function).
    unsigned b0 = rs_clip8(acc[0]);
    asm volatile("" : "+v"(b0));
    *reinterpret_cast<unsigned*>(row + x) = b0 | (rs_clip8(acc[1]) << 8) | (rs_clip8(acc[2]) << 16) | (rs_clip8(acc[3]) << 24);
  } else {
#pragma unroll
    for (int e = 0; e < 4; ++e)
      if (x + e < WB) row[x + e] = static_cast<unsigned char>(rs_clip8(acc[e]));
  }
}

// in [N][H0][WB] bytes -> out [..][H1][WB]; a thread owns four consecutive bytes of an output row (item idx), frame n goes to
// frame rs_slot(n) of out.  vec: WB % 4 == 0 and both pointers 4-byte aligned, so every row starts on a word.
__device__ __forceinline__ void rs_v_body(const unsigned char* __restrict__ in, int H0, int H1, int WB, int G, long total,
                                          const int* __restrict__ yb, const int* __restrict__ yk, int yks, unsigned char* __restrict__ out,
                                          int vec, long idx, const int* __restrict__ dst, int nslots) {
  if (idx >= total) return;
  const int g = static_cast<int>(idx % G);
  const long r = idx / G;
  const int yo = static_cast<int>(r % H1);
  const long n = r / H1;
  int lo, cnt;
  rs_bounds(yb, yo, H0, yks, lo, cnt);
  const unsigned char* src = in + (n * H0 + lo) * WB + 4 * g;
  const int* k = yk + static_cast<long>(yo) * yks;
  int acc[4];
#pragma unroll
  for (int e = 0; e < 4; ++e) acc[e] = 1 << (RS_PREC - 1);
  if (vec) {
    for (int t = 0; t < cnt; ++t) rs_mad4(*reinterpret_cast<const unsigned*>(src + static_cast<long>(t) * WB), k[t], acc);
  } else {
    const int nv = WB - 4 * g < 4 ? WB - 4 * g : 4;
    for (int t = 0; t < cnt; ++t) {
      const unsigned char* p = src + static_cast<long>(t) * WB;
      unsigned w = 0;
      for (int e = 0; e < nv; ++e) w |= static_cast<unsigned>(p[e]) << (8 * e);
      rs_mad4(w, k[t], acc);
    }
  }
  rs_store4(out + (rs_slot(dst, nslots, n) * H1 + yo) * WB, 4 * g, WB, acc, vec != 0);
}

__global__ __launch_bounds__(256) void rs_v_kernel(const unsigned char* __restrict__ in, int H0, int H1, int WB, int G, long total,
                                                   const int* __restrict__ yb, const int* __restrict__ yk, int yks,
                                                   unsigned char* __restrict__ out, int vec) {
  rs_v_body(in, H0, H1, WB, G, total, yb, yk, yks, out, vec, static_cast<long>(blockIdx.x) * 256 + threadIdx.x, nullptr, 0);
}

// What the host fixes per launch of the fused form (rs_plan): band rows, the LDS image's rows and pitch, source rows per round,
// and the byte offsets of the LDS regions.
struct RsPlan {
  int band, R, S, pitch;
  int off_yb, off_yk, off_tmp, off_stage;
  long lds;
};

// One band of the fused form: output rows y0 .. y0 + pl.band - 1 of frame n of `in`, written to frame `on` of `out`; rs_smem is
// the workgroup's pl.lds bytes of LDS, 16-byte aligned.
template <int C>
__device__ __forceinline__ void rs_fused_body(unsigned char* rs_smem, const unsigned char* __restrict__ in, int H0, int W0, int H1, int W1,
                                              const int* __restrict__ xb, const int* __restrict__ xk, int xks,
                                              const int* __restrict__ yb, const int* __restrict__ yk, int yks, const RsPlan& pl,
                                              unsigned char* __restrict__ out, int vec, int n, int y0, long on) {
  int* sxb = reinterpret_cast<int*>(rs_smem);                  // [W1][2]   clamped (xmin, count)
  int* sxk = sxb + 2 * W1;                                     // [W1][xks]
  int* syb = reinterpret_cast<int*>(rs_smem + pl.off_yb);      // [band][2]
  int* syk = reinterpret_cast<int*>(rs_smem + pl.off_yk);      // [band][yks]
  unsigned char* tmp = rs_smem + pl.off_tmp;                   // [R][pitch]  the horizontally resampled rows of this band
  unsigned char* stage = rs_smem + pl.off_stage;               // S source rows, at the global address's offset within 16 bytes
  const int t = threadIdx.x;
  const int nb = H1 - y0 < pl.band ? H1 - y0 : pl.band;
  const int WB = W1 * C;
  const long row_bytes = static_cast<long>(W0) * C;

  for (int i = t; i < W1; i += RS_THREADS) {
    int lo, cnt;
    rs_bounds(xb, i, W0, xks, lo, cnt);
    sxb[2 * i] = lo;
    sxb[2 * i + 1] = cnt;
  }
  for (int i = t; i < W1 * xks; i += RS_THREADS) sxk[i] = xk[i];
  for (int i = t; i < nb; i += RS_THREADS) {
    int lo, cnt;
    rs_bounds(yb, y0 + i, H0, yks, lo, cnt);
    syb[2 * i] = lo;
    syb[2 * i + 1] = cnt;
  }
  for (int i = t; i < nb * yks; i += RS_THREADS) syk[i] = yk[static_cast<long>(y0) * yks + i];
  __syncthreads();

  // source rows rlo .. rlo + nrows - 1 serve this band (the bounds rise with the output row; a table that breaks this is clamped)
  const int rlo = syb[0];
  const int nrows = rs_clampi(syb[2 * (nb - 1)] + syb[2 * (nb - 1) + 1] - rlo, 1, pl.R);
  for (int r0 = 0; r0 < nrows; r0 += pl.S) {
    const int ns = nrows - r0 < pl.S ? nrows - r0 : pl.S;
    const unsigned char* g = in + (static_cast<long>(n) * H0 + rlo + r0) * row_bytes;      // ns rows are one contiguous run
    const long len = ns * row_bytes;
    const int a = static_cast<int>(reinterpret_cast<uintptr_t>(g) & 15u);
    const long head = a ? (16 - a < len ? 16 - a : len) : 0;
    const long body = (len - head) >> 4;
    const long tail0 = head + (body << 4);
    for (long i = t; i < head; i += RS_THREADS) stage[a + i] = g[i];
    const uint4* gv = reinterpret_cast<const uint4*>(g + head);
    uint4* sv = reinterpret_cast<uint4*>(stage + a + head);      // a + head is 0 or 16
    for (long i = t; i < body; i += RS_THREADS) sv[i] = gv[i];
    for (long i = tail0 + t; i < len; i += RS_THREADS) stage[a + i] = g[i];
    __syncthreads();
    for (int i = t; i < ns * W1; i += RS_THREADS) {
      const int rr = i / W1, xo = i - rr * W1;
      const int lo = sxb[2 * xo], cnt = sxb[2 * xo + 1];
      const unsigned char* src = stage + a + rr * row_bytes + lo * C;
      const int* k = sxk + xo * xks;
      int acc[C];
#pragma unroll
      for (int c = 0; c < C; ++c) acc[c] = 1 << (RS_PREC - 1);
      for (int j = 0; j < cnt; ++j) {
        const int kv = k[j];
#pragma unroll
        for (int c = 0; c < C; ++c) acc[c] = rs_mad(src[j * C + c], kv, acc[c]);
      }
      unsigned char* d = tmp + (r0 + rr) * pl.pitch + xo * C;
#pragma unroll
      for (int c = 0; c < C; ++c) d[c] = static_cast<unsigned char>(rs_clip8(acc[c]));
    }
    __syncthreads();
  }

  const int G = (WB + 3) >> 2;
  for (int i = t; i < nb * G; i += RS_THREADS) {
    const int j = i / G, g4 = i - j * G;
    const int lo = syb[2 * j] - rlo, cnt = syb[2 * j + 1];
    const int* k = syk + j * yks;
    int acc[4];
#pragma unroll
    for (int e = 0; e < 4; ++e) acc[e] = 1 << (RS_PREC - 1);
    for (int q = 0; q < cnt; ++q) {
      const int row = rs_clampi(lo + q, 0, nrows - 1);
      rs_mad4(*reinterpret_cast<const unsigned*>(tmp + row * pl.pitch + 4 * g4), k[q], acc);      // the pitch is a multiple of 16
    }
    rs_store4(out + (on * H1 + y0 + j) * WB, 4 * g4, WB, acc, vec != 0);
  }
}

template <int C>
__global__ __launch_bounds__(RS_THREADS) void rs_fused_kernel(const unsigned char* __restrict__ in, int H0, int W0, int H1, int W1,
                                                              const int* __restrict__ xb, const int* __restrict__ xk, int xks,
                                                              const int* __restrict__ yb, const int* __restrict__ yk, int yks,
                                                              RsPlan pl, unsigned char* __restrict__ out, int vec) {
  extern __shared__ __align__(16) unsigned char rs_smem[];
  rs_fused_body<C>(rs_smem, in, H0, W0, H1, W1, xb, xk, xks, yb, yk, yks, pl, out, vec, blockIdx.y, blockIdx.x * pl.band, blockIdx.y);
}

// ---- the grouped forms: frames of several source sizes in one launch per form ------------------------------------------
// The parameter block of one group in one launch, and the launch's argument: the blocks travel by value, so a launch takes at most
// DIFFSAL_RESAMPLE_MAX_GROUPS of them.  first[g] is the first workgroup of group g (first[G]: the grid); a workgroup finds its
// group by walking that table, which is uniform over the workgroup.
struct RsGroup {
  const unsigned char* in;
  unsigned char* out;
  const int *xb, *xk, *yb, *yk;
  const int* dst;      // the group's slice of the dst table; NULL: `out` is already the group's first frame
  int N, H0, W0, xks, yks, vec;
  int per;             // fused: bands per frame
  RsPlan pl;           // fused only
};
struct RsGroups {
  int G, nslots, H1, W1;
  unsigned first[DIFFSAL_RESAMPLE_MAX_GROUPS + 1];
  RsGroup g[DIFFSAL_RESAMPLE_MAX_GROUPS];
};

__device__ __forceinline__ int rs_find_group(const RsGroups& a, unsigned wg) {
  int g = 0;
  while (g + 1 < a.G && wg >= a.first[g + 1]) ++g;
  return g;
}

template <int C>
__global__ __launch_bounds__(256) void rs_h_groups_kernel(const RsGroups a) {
  const int g = rs_find_group(a, blockIdx.x);
  const RsGroup& p = a.g[g];
  const long idx = static_cast<long>(blockIdx.x - a.first[g]) * 256 + threadIdx.x;
  rs_h_body<C>(p.in, static_cast<long>(p.N) * p.H0, p.W0, a.W1, p.xb, p.xk, p.xks, p.out, idx, p.H0, p.dst, a.nslots);
}

template <int C>
__global__ __launch_bounds__(256) void rs_v_groups_kernel(const RsGroups a) {
  const int g = rs_find_group(a, blockIdx.x);
  const RsGroup& p = a.g[g];
  const long idx = static_cast<long>(blockIdx.x - a.first[g]) * 256 + threadIdx.x;
  const int WB = a.W1 * C, G4 = (WB + 3) >> 2;
  rs_v_body(p.in, p.H0, a.H1, WB, G4, static_cast<long>(p.N) * a.H1 * G4, p.yb, p.yk, p.yks, p.out, p.vec, idx, p.dst, a.nslots);
}

template <int C>
__global__ __launch_bounds__(RS_THREADS) void rs_fused_groups_kernel(const RsGroups a) {
  extern __shared__ __align__(16) unsigned char rs_smem[];
  const int g = rs_find_group(a, blockIdx.x);
  const RsGroup& p = a.g[g];
  const unsigned local = blockIdx.x - a.first[g];
  const int n = static_cast<int>(local / p.per), band = static_cast<int>(local - static_cast<unsigned>(n) * p.per);
  rs_fused_body<C>(rs_smem, p.in, p.H0, p.W0, a.H1, a.W1, p.xb, p.xk, p.xks, p.yb, p.yk, p.yks, p.pl, p.out, p.vec, n, band * p.pl.band,
                   rs_slot(p.dst, a.nslots, n));
}

template <int C>
__global__ __launch_bounds__(256) void vg_gather_kernel(const unsigned char* __restrict__ frames, int N, long hw, const int* __restrict__ idx,
                                                        int T, const float* __restrict__ table, long groups, long total,
                                                        float* __restrict__ out, int vec) {
  __shared__ float lut[C * 256];
  for (int i = threadIdx.x; i < C * 256; i += 256) lut[i] = table[i];
  __syncthreads();
  const long item = static_cast<long>(blockIdx.x) * 256 + threadIdx.x;
  if (item >= total) return;
  const long bt = item / groups;
  const long p = (item - bt * groups) * 4;
  int f = idx ? idx[bt] : static_cast<int>(bt);
  f = rs_clampi(f, 0, N - 1);      // a device-resident table is not checked by the host
  const long b = bt / T, tt = bt - b * T;
  const unsigned char* src = frames + (static_cast<long>(f) * hw + p) * C;
  float* dst = out + ((b * C) * T + tt) * hw + p;      // channel c: + c * T * hw
  const long plane = static_cast<long>(T) * hw;
  if (vec) {      // hw % 4 == 0, frames 4-byte and out 16-byte aligned: 4 C source bytes are C words, each plane gets one float4
    unsigned w[C];
#pragma unroll
    for (int c = 0; c < C; ++c) w[c] = reinterpret_cast<const unsigned*>(src)[c];
#pragma unroll
    for (int c = 0; c < C; ++c) {
      float v[4];
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const int byte = e * C + c;      // pixel e, channel c
        v[e] = lut[c * 256 + ((w[byte >> 2] >> (8 * (byte & 3))) & 255u)];
      }
      st4(dst + c * plane, make_float4(v[0], v[1], v[2], v[3]));
    }
  } else {
    const int nv = hw - p < 4 ? static_cast<int>(hw - p) : 4;
    for (int e = 0; e < nv; ++e)
#pragma unroll
      for (int c = 0; c < C; ++c) dst[c * plane + e] = lut[c * 256 + src[e * C + c]];
  }
}

// ---- host side ----------------------------------------------------------------------------------------------------------

static inline double rs_support(int filter) { return filter == DIFFSAL_FILTER_BICUBIC ? 2.0 : 1.0; }
// Pillow's precompute_coeffs: filterscale = max(in / out, 1); support = filter support * filterscale; ksize = 2 ceil(support) + 1
static inline int rs_ksize(int n_in, int n_out, int filter) {
  double fs = static_cast<double>(n_in) / n_out;
  if (fs < 1.0) fs = 1.0;
  return static_cast<int>(std::ceil(rs_support(filter) * fs)) * 2 + 1;
}
static inline long rs_up16(long v) { return (v + 15) & ~15L; }

// LDS layout of the fused form for bands of `band` output rows.  The band's source rows: with c(y) = (y + 0.5) scale and
// s = support * max(scale, 1), the first row is trunc(c(y0) - s + 0.5) >= c(y0) - s - 0.5 and the row past the last is
// trunc(c(y1) + s + 0.5) <= c(y1) + s + 0.5, so a band spans at most (band - 1) scale + 2 s + 1 rows; one more for rounding.
static RsPlan rs_layout(int H0, int W0, int C, int H1, int W1, int filter, int band) {
  RsPlan p;
  const int xks = rs_ksize(W0, W1, filter), yks = rs_ksize(H0, H1, filter);
  const double scale = static_cast<double>(H0) / H1, sup = rs_support(filter) * (scale < 1.0 ? 1.0 : scale);
  const double span = std::floor((band - 1) * scale + 2.0 * sup + 1.0) + 1.0;
  p.band = band;
  p.R = span < H0 ? static_cast<int>(span) : H0;
  const long row_bytes = static_cast<long>(W0) * C;
  long S = RS_STAGE_BYTES / row_bytes;
  S = S < 1 ? 1 : (S > p.R ? p.R : S);
  p.S = static_cast<int>(S);
  p.pitch = static_cast<int>(rs_up16(static_cast<long>(W1) * C));
  long off = static_cast<long>(W1) * (2 + xks) * 4;
  p.off_yb = static_cast<int>(off);
  off += 2L * band * 4;
  p.off_yk = static_cast<int>(off);
  off = rs_up16(off + static_cast<long>(band) * yks * 4);
  p.off_tmp = static_cast<int>(off);
  off += static_cast<long>(p.R) * p.pitch;
  p.off_stage = static_cast<int>(off);
  off += rs_up16(S * row_bytes + 16);      // the run starts up to 15 bytes into the region
  p.lds = off;
  return p;
}

// The band height of the fused form; band = 0 in the result: not even one output row fits, the two-pass form serves.
// A taller band redoes less horizontal work (adjacent bands overlap by the vertical support) but holds more LDS, and the LDS a
// workgroup holds decides how many of them a CU runs at once (160 KB in all).  The tallest band (32 rows at most) is taken
// within the smallest of three budgets (a third, a half, all of the CU's LDS) at which the band's source rows are at most 1.35
// times the rows it alone owns; if none reaches that, the tallest band that fits in 160 KB.
static RsPlan rs_plan(int H0, int W0, int C, int H1, int W1, int filter) {
  const long budgets[3] = {RS_LDS_MAX / 3, RS_LDS_MAX / 2, RS_LDS_MAX};
  const int top = H1 < RS_MAX_BAND ? H1 : RS_MAX_BAND;
  const double scale = static_cast<double>(H0) / H1;
  RsPlan best;
  best.band = 0;
  best.lds = 0;
  for (int b = 0; b < 3; ++b) {
    for (int band = top; band >= 1; --band) {
      const RsPlan p = rs_layout(H0, W0, C, H1, W1, filter, band);
      if (p.lds > budgets[b]) continue;
      best = p;
      const double own = band * scale < 1.0 ? 1.0 : band * scale;
      if (p.R <= 1.35 * own || band == H1) return p;
      break;
    }
  }
  return best;
}

// DIFFSAL_RESAMPLE_AUTO: the fused form where a band fits and the source has at least twice the pixels of the output.  Measured on
// an MI355X ("Video front end"): fused is faster at 360x640 -> 240x320 and 1080x1920 -> 240x320, where the intermediate
// image it keeps out of HBM is larger than the output; at 240x320 -> 224x384 the two passes are faster.
static inline bool rs_auto_fused(int H0, int W0, int H1, int W1, const RsPlan& p) {
  return p.band > 0 && static_cast<long>(H0) * W0 >= 2L * H1 * W1;
}

static int rs_check_shape(const char* what, int N, int H0, int W0, int C, int H1, int W1, int filter) {
  DS_REQUIRE(C == 1 || C == 3, DIFFSAL_E_ARG, "%s: C = %d channels (1 or 3)", what, C);
  DS_REQUIRE(filter == DIFFSAL_FILTER_BILINEAR || filter == DIFFSAL_FILTER_BICUBIC, DIFFSAL_E_ARG,
             "%s: filter %d (DIFFSAL_FILTER_BILINEAR or DIFFSAL_FILTER_BICUBIC)", what, filter);
  DS_REQUIRE(N > 0 && N <= 65535 && H0 > 0 && W0 > 0 && H1 > 0 && W1 > 0 && H0 <= RS_MAX_SIDE && W0 <= RS_MAX_SIDE && H1 <= RS_MAX_SIDE &&
                 W1 <= RS_MAX_SIDE,
             DIFFSAL_E_SHAPE, "%s: bad shape N=%d (1..65535) %dx%d -> %dx%d (every side 1..%d)", what, N, H0, W0, H1, W1, RS_MAX_SIDE);
  return DIFFSAL_OK;
}

}  // namespace diffsal

using namespace diffsal;

extern "C" int diffsal_resample_ksize(int in_size, int out_size, int filter) {
  if (in_size <= 0 || out_size <= 0 || in_size > RS_MAX_SIDE || out_size > RS_MAX_SIDE) return 0;
  if (filter != DIFFSAL_FILTER_BILINEAR && filter != DIFFSAL_FILTER_BICUBIC) return 0;
  return rs_ksize(in_size, out_size, filter);
}

extern "C" int diffsal_resample_u8_band_rows(int H0, int W0, int C, int H1, int W1, int filter) {
  if (rs_check_shape("resample_u8_band_rows", 1, H0, W0, C, H1, W1, filter) != DIFFSAL_OK) return 0;
  if (H0 == H1 || W0 == W1) return 0;      // a single pass has no intermediate image
  return rs_plan(H0, W0, C, H1, W1, filter).band;
}

extern "C" size_t diffsal_resample_u8_ws_bytes(int N, int H0, int W0, int C, int H1, int W1, int filter, int form) {
  if (rs_check_shape("resample_u8_ws_bytes", N, H0, W0, C, H1, W1, filter) != DIFFSAL_OK) return 0;
  if (H0 == H1 || W0 == W1) return 0;
  if (form == DIFFSAL_RESAMPLE_FUSED) return 0;
  if (form == DIFFSAL_RESAMPLE_AUTO && rs_auto_fused(H0, W0, H1, W1, rs_plan(H0, W0, C, H1, W1, filter))) return 0;
  return static_cast<size_t>(N) * H0 * W1 * C;
}

template <int C>
static void rs_launch_h(hipStream_t s, const unsigned char* in, long rows, int W0, int W1, const int* xb, const int* xk, int xks,
                        unsigned char* out) {
  const long total = rows * W1;
  hipLaunchKernelGGL((rs_h_kernel<C>), dim3(static_cast<unsigned>((total + 255) / 256)), dim3(256), 0, s, in, rows, W0, W1, xb, xk, xks, out);
}

static void rs_launch_v(hipStream_t s, const unsigned char* in, int N, int H0, int H1, int WB, const int* yb, const int* yk, int yks,
                        unsigned char* out) {
  const int G = (WB + 3) / 4;
  const long total = static_cast<long>(N) * H1 * G;
  const int vec = WB % 4 == 0 && (reinterpret_cast<uintptr_t>(in) & 3u) == 0 && (reinterpret_cast<uintptr_t>(out) & 3u) == 0;
  hipLaunchKernelGGL(rs_v_kernel, dim3(static_cast<unsigned>((total + 255) / 256)), dim3(256), 0, s, in, H0, H1, WB, G, total, yb, yk, yks, out,
                     vec);
}

template <int C>
static void rs_launch_fused(hipStream_t s, const unsigned char* in, int N, int H0, int W0, int H1, int W1, const int* xb, const int* xk,
                            int xks, const int* yb, const int* yk, int yks, const RsPlan& pl, unsigned char* out) {
  DS_RAISE_DYNAMIC_LDS(rs_fused_kernel<C>, static_cast<int>(RS_LDS_MAX));
  const int vec = (W1 * C) % 4 == 0 && (reinterpret_cast<uintptr_t>(out) & 3u) == 0;
  hipLaunchKernelGGL((rs_fused_kernel<C>), dim3((H1 + pl.band - 1) / pl.band, N), dim3(RS_THREADS), static_cast<size_t>(pl.lds), s, in, H0, W0,
                     H1, W1, xb, xk, xks, yb, yk, yks, pl, out, vec);
}

extern "C" int diffsal_resample_u8(const unsigned char* in, int N, int H0, int W0, int C, int H1, int W1, int filter, const int* xbounds,
                                   const int* xkk, int xks, const int* ybounds, const int* ykk, int yks, int form, int band_rows,
                                   unsigned char* out, void* ws, size_t ws_bytes, diffsal_stream_t stream) {
  const int rc = rs_check_shape("resample_u8", N, H0, W0, C, H1, W1, filter);
  if (rc != DIFFSAL_OK) return rc;
  DS_REQUIRE(form == DIFFSAL_RESAMPLE_AUTO || form == DIFFSAL_RESAMPLE_FUSED || form == DIFFSAL_RESAMPLE_TWO_PASS, DIFFSAL_E_ARG,
             "resample_u8: form %d (DIFFSAL_RESAMPLE_AUTO, _FUSED or _TWO_PASS)", form);
  const bool do_x = W0 != W1, do_y = H0 != H1;
  DS_REQUIRE(static_cast<long>(N) * H0 * (W0 > W1 ? W0 : W1) < (1L << 38) && static_cast<long>(N) * H1 * W1 < (1L << 38), DIFFSAL_E_SHAPE,
             "resample_u8: %d frames of %dx%d -> %dx%d are more pixels than one launch takes (2^38)", N, H0, W0, H1, W1);
  DS_REQUIRE(!do_x || xks == rs_ksize(W0, W1, filter), DIFFSAL_E_SHAPE, "resample_u8: %d coefficients per output column, %d -> %d takes %d",
             xks, W0, W1, rs_ksize(W0, W1, filter));
  DS_REQUIRE(!do_y || yks == rs_ksize(H0, H1, filter), DIFFSAL_E_SHAPE, "resample_u8: %d coefficients per output row, %d -> %d takes %d", yks,
             H0, H1, rs_ksize(H0, H1, filter));
  DS_REQUIRE(band_rows >= 0 && band_rows <= RS_MAX_BAND, DIFFSAL_E_ARG, "resample_u8: band_rows %d (0: the library picks; at most %d)",
             band_rows, RS_MAX_BAND);
  RsPlan pl;
  pl.band = 0;
  if (do_x && do_y && form != DIFFSAL_RESAMPLE_TWO_PASS) {
    pl = band_rows ? rs_layout(H0, W0, C, H1, W1, filter, band_rows < H1 ? band_rows : H1) : rs_plan(H0, W0, C, H1, W1, filter);
    if (pl.lds > RS_LDS_MAX) pl.band = 0;
    if (form == DIFFSAL_RESAMPLE_AUTO && !rs_auto_fused(H0, W0, H1, W1, pl)) pl.band = 0;
    DS_REQUIRE(pl.band > 0 || form == DIFFSAL_RESAMPLE_AUTO, DIFFSAL_E_SHAPE,
               "resample_u8: a band of %d output rows of %dx%d -> %dx%d does not fit in %ld bytes of LDS: use the two-pass form",
               band_rows ? band_rows : 1, H0, W0, H1, W1, RS_LDS_MAX);
  }
  const bool two_pass = do_x && do_y && pl.band == 0;
  const size_t need = two_pass ? static_cast<size_t>(N) * H0 * W1 * C : 0;
  DS_REQUIRE(need == 0 || (ws_bytes >= need && ws), DIFFSAL_E_ARG, "resample_u8: workspace too small: %zu bytes, the two-pass form needs %zu",
             ws_bytes, need);
  DS_REQUIRE(in && out && (!do_x || (xbounds && xkk)) && (!do_y || (ybounds && ykk)), DIFFSAL_E_ARG, "resample_u8: null argument");
  DS_REQUIRE(in != out, DIFFSAL_E_ARG, "resample_u8: in place");
  hipStream_t s = static_cast<hipStream_t>(stream);
  const long rows = static_cast<long>(N) * H0;
  if (!do_x && !do_y) {
    const hipError_t e = hipMemcpyAsync(out, in, static_cast<size_t>(rows) * W0 * C, hipMemcpyDeviceToDevice, s);
    DS_REQUIRE(e == hipSuccess, DIFFSAL_E_LAUNCH, "resample_u8: copy failed: %s", hipGetErrorString(e));
    return DIFFSAL_OK;
  }
  if (!do_y) {
    if (C == 3) rs_launch_h<3>(s, in, rows, W0, W1, xbounds, xkk, xks, out);
    else rs_launch_h<1>(s, in, rows, W0, W1, xbounds, xkk, xks, out);
  } else if (!do_x) {
    rs_launch_v(s, in, N, H0, H1, W0 * C, ybounds, ykk, yks, out);
  } else if (two_pass) {
    unsigned char* mid = static_cast<unsigned char*>(ws);
    if (C == 3) rs_launch_h<3>(s, in, rows, W0, W1, xbounds, xkk, xks, mid);
    else rs_launch_h<1>(s, in, rows, W0, W1, xbounds, xkk, xks, mid);
    rs_launch_v(s, mid, N, H0, H1, W1 * C, ybounds, ykk, yks, out);
  } else {
    if (C == 3) rs_launch_fused<3>(s, in, N, H0, W0, H1, W1, xbounds, xkk, xks, ybounds, ykk, yks, pl, out);
    else rs_launch_fused<1>(s, in, N, H0, W0, H1, W1, xbounds, xkk, xks, ybounds, ykk, yks, pl, out);
  }
  return check_launch("resample_u8");
}

// ---- grouped call ---------------------------------------------------------------------------------------------------------

namespace diffsal {

enum RsKind { RS_COPY, RS_H, RS_V, RS_TWO, RS_FUSED };

// What one group of the grouped call runs and its checks, which are those of diffsal_resample_u8 with band_rows = 0.
static int rs_group_kind(const char* what, int g, const diffsal_resample_group& gr, int C, int H1, int W1, int filter, int form, RsKind& kind,
                         RsPlan& pl) {
  const int rc = rs_check_shape(what, gr.N, gr.H0, gr.W0, C, H1, W1, filter);
  if (rc != DIFFSAL_OK) return rc;
  const int H0 = gr.H0, W0 = gr.W0;
  const bool do_x = W0 != W1, do_y = H0 != H1;
  DS_REQUIRE(static_cast<long>(gr.N) * H0 * (W0 > W1 ? W0 : W1) < (1L << 38) && static_cast<long>(gr.N) * H1 * W1 < (1L << 38), DIFFSAL_E_SHAPE,
             "%s: group %d: %d frames of %dx%d -> %dx%d are more pixels than one launch takes (2^38)", what, g, gr.N, H0, W0, H1, W1);
  DS_REQUIRE(!do_x || gr.xks == rs_ksize(W0, W1, filter), DIFFSAL_E_SHAPE, "%s: group %d: %d coefficients per output column, %d -> %d takes %d",
             what, g, gr.xks, W0, W1, rs_ksize(W0, W1, filter));
  DS_REQUIRE(!do_y || gr.yks == rs_ksize(H0, H1, filter), DIFFSAL_E_SHAPE, "%s: group %d: %d coefficients per output row, %d -> %d takes %d",
             what, g, gr.yks, H0, H1, rs_ksize(H0, H1, filter));
  pl.band = 0;
  if (do_x && do_y && form != DIFFSAL_RESAMPLE_TWO_PASS) {
    pl = rs_plan(H0, W0, C, H1, W1, filter);
    if (pl.lds > RS_LDS_MAX) pl.band = 0;
    if (form == DIFFSAL_RESAMPLE_AUTO && !rs_auto_fused(H0, W0, H1, W1, pl)) pl.band = 0;
    DS_REQUIRE(pl.band > 0 || form == DIFFSAL_RESAMPLE_AUTO, DIFFSAL_E_SHAPE,
               "%s: group %d: a band of one output row of %dx%d -> %dx%d does not fit in %ld bytes of LDS: use the two-pass form", what, g, H0,
               W0, H1, W1, RS_LDS_MAX);
  }
  kind = !do_x && !do_y ? RS_COPY : !do_y ? RS_H : !do_x ? RS_V : pl.band == 0 ? RS_TWO : RS_FUSED;
  return DIFFSAL_OK;
}

static int rs_groups_check(const char* what, const diffsal_resample_group* groups, int G, int form) {
  DS_REQUIRE(groups && G > 0, DIFFSAL_E_ARG, "%s: %d groups (at least one)", what, G);
  DS_REQUIRE(form == DIFFSAL_RESAMPLE_AUTO || form == DIFFSAL_RESAMPLE_FUSED || form == DIFFSAL_RESAMPLE_TWO_PASS, DIFFSAL_E_ARG,
             "%s: form %d (DIFFSAL_RESAMPLE_AUTO, _FUSED or _TWO_PASS)", what, form);
  return DIFFSAL_OK;
}

// one launch of a grouped form; `blocks` counts the workgroups that a.first has been given so far
struct RsBatch {
  RsGroups a;
  long blocks;
  long lds;
  void reset(int nslots, int H1, int W1) {
    a.G = 0;
    a.nslots = nslots;
    a.H1 = H1;
    a.W1 = W1;
    a.first[0] = 0;
    blocks = 0;
    lds = 0;
  }
  void add(const RsGroup& p, long nblocks) {
    a.g[a.G] = p;
    blocks += nblocks;
    a.first[++a.G] = static_cast<unsigned>(blocks);
  }
};

}  // namespace diffsal

extern "C" size_t diffsal_resample_u8_groups_ws_bytes(const diffsal_resample_group* groups, int G, int C, int H1, int W1, int filter,
                                                      int form) {
  if (rs_groups_check("resample_u8_groups_ws_bytes", groups, G, form) != DIFFSAL_OK) return 0;
  size_t total = 0;
  for (int g = 0; g < G; ++g) {
    RsKind kind;
    RsPlan pl;
    if (rs_group_kind("resample_u8_groups_ws_bytes", g, groups[g], C, H1, W1, filter, form, kind, pl) != DIFFSAL_OK) return 0;
    if (kind == RS_TWO) total += static_cast<size_t>(rs_up16(static_cast<long>(groups[g].N) * groups[g].H0 * W1 * C));
  }
  return total;
}

extern "C" int diffsal_resample_u8_groups_launches(const diffsal_resample_group* groups, int G, int C, int H1, int W1, int filter, int form) {
  if (rs_groups_check("resample_u8_groups_launches", groups, G, form) != DIFFSAL_OK) return -1;
  int launches = 0;
  for (int g0 = 0; g0 < G; g0 += DIFFSAL_RESAMPLE_MAX_GROUPS) {
    bool fused = false, hpass = false, vpass = false;
    for (int g = g0; g < G && g < g0 + DIFFSAL_RESAMPLE_MAX_GROUPS; ++g) {
      RsKind kind;
      RsPlan pl;
      if (rs_group_kind("resample_u8_groups_launches", g, groups[g], C, H1, W1, filter, form, kind, pl) != DIFFSAL_OK) return -1;
      fused |= kind == RS_FUSED;
      hpass |= kind == RS_COPY || kind == RS_H || kind == RS_TWO;
      vpass |= kind == RS_V || kind == RS_TWO;
    }
    launches += fused + hpass + vpass;
  }
  return launches;
}

extern "C" int diffsal_resample_u8_groups(const diffsal_resample_group* groups, int G, int C, int H1, int W1, int filter, int form,
                                          const int* dst, int n_total, unsigned char* out, void* ws, size_t ws_bytes,
                                          diffsal_stream_t stream) {
  const char* what = "resample_u8_groups";
  int rc = rs_groups_check(what, groups, G, form);
  if (rc != DIFFSAL_OK) return rc;
  // every check of every group precedes the first launch
  long frames = 0, pixels = 0;
  size_t need = 0;
  for (int g = 0; g < G; ++g) {
    RsKind kind;
    RsPlan pl;
    rc = rs_group_kind(what, g, groups[g], C, H1, W1, filter, form, kind, pl);
    if (rc != DIFFSAL_OK) return rc;
    const diffsal_resample_group& gr = groups[g];
    DS_REQUIRE(gr.in && (gr.W0 == W1 || (gr.xbounds && gr.xkk)) && (gr.H0 == H1 || (gr.ybounds && gr.ykk)), DIFFSAL_E_ARG,
               "%s: group %d: null argument", what, g);
    if (kind == RS_TWO) need += static_cast<size_t>(rs_up16(static_cast<long>(gr.N) * gr.H0 * W1 * C));
    frames += gr.N;
    pixels += static_cast<long>(gr.N) * gr.H0 * (gr.W0 > W1 ? gr.W0 : W1);
  }
  DS_REQUIRE(frames == n_total, DIFFSAL_E_SHAPE, "%s: the groups hold %ld frames, the output has n_total = %d", what, frames, n_total);
  // so that no launch has 2^31 workgroups: a workgroup of the passes owns 256 pixels or more
  DS_REQUIRE(pixels < (1L << 38) && static_cast<long>(n_total) * H1 * W1 < (1L << 38), DIFFSAL_E_SHAPE,
             "%s: %d frames -> %dx%d are more pixels than one call takes (2^38)", what, n_total, H1, W1);
  DS_REQUIRE(need == 0 || (ws_bytes >= need && ws), DIFFSAL_E_ARG, "%s: workspace too small: %zu bytes, the two-pass groups need %zu", what,
             ws_bytes, need);
  DS_REQUIRE(out, DIFFSAL_E_ARG, "%s: null argument", what);
  const long frame_bytes = static_cast<long>(H1) * W1 * C;
  for (int g = 0; g < G; ++g) {
    const unsigned char* in = groups[g].in;
    const long in_bytes = static_cast<long>(groups[g].N) * groups[g].H0 * groups[g].W0 * C;
    DS_REQUIRE(in + in_bytes <= out || out + n_total * frame_bytes <= in, DIFFSAL_E_ARG, "%s: group %d overlaps the output", what, g);
  }
  hipStream_t s = static_cast<hipStream_t>(stream);
  const int WB = W1 * C, G4 = (WB + 3) / 4;
  const bool out_vec = WB % 4 == 0 && (reinterpret_cast<uintptr_t>(out) & 3u) == 0;
  RsBatch bf, bh, bv;      // ~2 KB each
  long base = 0;
  size_t ws_off = 0;
  for (int g0 = 0; g0 < G; g0 += DIFFSAL_RESAMPLE_MAX_GROUPS) {
    bf.reset(n_total, H1, W1);
    bh.reset(n_total, H1, W1);
    bv.reset(n_total, H1, W1);
    for (int g = g0; g < G && g < g0 + DIFFSAL_RESAMPLE_MAX_GROUPS; ++g) {
      const diffsal_resample_group& gr = groups[g];
      RsKind kind;
      RsPlan pl;
      (void)rs_group_kind(what, g, gr, C, H1, W1, filter, form, kind, pl);
      RsGroup p;
      p.in = gr.in;
      p.out = dst ? out : out + base * frame_bytes;
      p.xb = gr.W0 == W1 ? nullptr : gr.xbounds;
      p.xk = gr.W0 == W1 ? nullptr : gr.xkk;
      p.yb = gr.H0 == H1 ? nullptr : gr.ybounds;
      p.yk = gr.H0 == H1 ? nullptr : gr.ykk;
      p.dst = dst ? dst + base : nullptr;
      p.N = gr.N;
      p.H0 = gr.H0;
      p.W0 = gr.W0;
      p.xks = gr.xks;
      p.yks = gr.yks;
      p.vec = out_vec;
      p.per = 1;
      p.pl = pl;
      const long h_blocks = (static_cast<long>(gr.N) * gr.H0 * W1 + 255) / 256;
      const long v_blocks = (static_cast<long>(gr.N) * H1 * G4 + 255) / 256;
      if (kind == RS_FUSED) {
        p.per = (H1 + pl.band - 1) / pl.band;
        bf.add(p, static_cast<long>(gr.N) * p.per);
        if (pl.lds > bf.lds) bf.lds = pl.lds;
      } else if (kind == RS_COPY || kind == RS_H) {
        bh.add(p, h_blocks);
      } else if (kind == RS_V) {
        p.vec = out_vec && (reinterpret_cast<uintptr_t>(gr.in) & 3u) == 0;
        bv.add(p, v_blocks);
      } else {      // two passes through the group's slice of the workspace, whose offset is a multiple of 16
        unsigned char* mid = static_cast<unsigned char*>(ws) + ws_off;
        ws_off += static_cast<size_t>(rs_up16(static_cast<long>(gr.N) * gr.H0 * W1 * C));
        RsGroup ph = p;
        ph.out = mid;
        ph.dst = nullptr;
        bh.add(ph, h_blocks);
        p.in = mid;
        bv.add(p, v_blocks);
      }
      base += gr.N;
    }
    if (bf.a.G) {
      if (C == 3) {
        DS_RAISE_DYNAMIC_LDS(rs_fused_groups_kernel<3>, static_cast<int>(RS_LDS_MAX));
        hipLaunchKernelGGL((rs_fused_groups_kernel<3>), dim3(static_cast<unsigned>(bf.blocks)), dim3(RS_THREADS), static_cast<size_t>(bf.lds), s,
                           bf.a);
      } else {
        DS_RAISE_DYNAMIC_LDS(rs_fused_groups_kernel<1>, static_cast<int>(RS_LDS_MAX));
        hipLaunchKernelGGL((rs_fused_groups_kernel<1>), dim3(static_cast<unsigned>(bf.blocks)), dim3(RS_THREADS), static_cast<size_t>(bf.lds), s,
                           bf.a);
      }
    }
    if (bh.a.G) {
      if (C == 3) hipLaunchKernelGGL((rs_h_groups_kernel<3>), dim3(static_cast<unsigned>(bh.blocks)), dim3(256), 0, s, bh.a);
      else hipLaunchKernelGGL((rs_h_groups_kernel<1>), dim3(static_cast<unsigned>(bh.blocks)), dim3(256), 0, s, bh.a);
    }
    if (bv.a.G) {
      if (C == 3) hipLaunchKernelGGL((rs_v_groups_kernel<3>), dim3(static_cast<unsigned>(bv.blocks)), dim3(256), 0, s, bv.a);
      else hipLaunchKernelGGL((rs_v_groups_kernel<1>), dim3(static_cast<unsigned>(bv.blocks)), dim3(256), 0, s, bv.a);
    }
  }
  return check_launch(what);
}

extern "C" int diffsal_clip_gather_u8(const unsigned char* frames, int N, int h, int w, int C, const int* indices, int B, int T,
                                      const float* table, float* out, diffsal_stream_t stream) {
  DS_REQUIRE(C == 1 || C == 3, DIFFSAL_E_ARG, "clip_gather_u8: C = %d channels (1 or 3)", C);
  DS_REQUIRE(N > 0 && h > 0 && w > 0 && B > 0 && T > 0 && h <= RS_MAX_SIDE && w <= RS_MAX_SIDE, DIFFSAL_E_SHAPE,
             "clip_gather_u8: bad shape N=%d h=%d w=%d (1..%d) B=%d T=%d", N, h, w, RS_MAX_SIDE, B, T);
  DS_REQUIRE(indices || static_cast<long>(B) * T == N, DIFFSAL_E_SHAPE,
             "clip_gather_u8: without an index table frame b * T + t is read: B * T = %ld must be N = %d", static_cast<long>(B) * T, N);
  DS_REQUIRE(frames && table && out, DIFFSAL_E_ARG, "clip_gather_u8: null argument");
  const long hw = static_cast<long>(h) * w, groups = (hw + 3) / 4;
  const long total = static_cast<long>(B) * T * groups;
  DS_REQUIRE((total + 255) / 256 < (1L << 31), DIFFSAL_E_SHAPE, "clip_gather_u8: %ld outputs", total * 4 * C);
  const int vec = hw % 4 == 0 && aligned16(out) && (reinterpret_cast<uintptr_t>(frames) & 3u) == 0;
  const dim3 grid(static_cast<unsigned>((total + 255) / 256));
  hipStream_t s = static_cast<hipStream_t>(stream);
  if (C == 3) hipLaunchKernelGGL((vg_gather_kernel<3>), grid, dim3(256), 0, s, frames, N, hw, indices, T, table, groups, total, out, vec);
  else hipLaunchKernelGGL((vg_gather_kernel<1>), grid, dim3(256), 0, s, frames, N, hw, indices, T, table, groups, total, out, vec);
  return check_launch("clip_gather_u8");
}
