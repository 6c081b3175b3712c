// From the sampler's fp32 map to the map the benchmark scores: the 8-bit export of R/diffusion_trainer.py:898-935 (normalize_data,
// R/util/utils.py:11-16), the float map plt.imread gives back for that PNG (R/compute_metrics.py:9-26) and the spline resize to the
// annotation's resolution (R/metrics/metrics.py:41-42,102-103,195-196,218-219,243-244: skimage resize, order 3 or 1, mode
// 'reflect', clip).  include/diffsal.h ("benchmark post-processing") states the arithmetic; the launches, all on the caller's stream:
//   map_to_u8    minmax  per (image, chunk): fp32 min / max of 4096 pixels
//                quant   per (image, chunk): the image's min / max from the chunk partials, then the bytes (and byte / 255)
//   map_from_u8  one elementwise pass
//   map_resize   minmax  (clip only) as above, on the source
//                coef_x  (order 3) the B-spline prefilter along x: fp32 source -> fp64
//                coef_y  (order 3) the same along y: fp64 -> fp64 coefficients
//                interp  per output pixel: 2 x 2 source values (order 1) or 4 x 4 coefficients (order 3), fp64, clip, one rounding;
//                        a thread makes four rows of one output column
// The prefilter is the closed form c[i] = sqrt(3) * sum_k z^|k| s[mirror(i + k)], z = sqrt(3) - 2, |k| <= 34 (|z|^34 < 2^-64),
// summed from the far taps inwards in Horner form: no serial chain along a line, a fixed order per coefficient.  A workgroup
// first copies its stretch of the line, extended by 34 mirrored samples on both sides (the index folded by modulo: the period
// 2(n - 1) may be shorter than 34), to LDS; the tap loop then has no index arithmetic.
//   map_resize_aa  minmax (clip only) on the UNFILTERED source; gauss_y, gauss_x (each only where its axis shrinks): the
//                  anti-aliasing Gaussian, fp32 -> fp32 through fp64 sums (csrc/postprocess_gauss.h); then coef_x, coef_y, interp
//                  as above, reading the filtered map
//   map_gauss      gauss_y, gauss_x alone
// min / max are exact in any order, every sum has a fixed order: two calls give the same bits.  No floating-point atomics, no
// allocation, no synchronisation; what a launch reads from an earlier one it reads behind a kernel boundary.
#include "common.h"
#include "postprocess_gauss.h"

namespace diffsal {

constexpr int PP_CHUNK = 4096;      // pixels per workgroup of the min / max and quantise passes
constexpr int PP_K = 34;            // prefilter taps on each side: |z|^34 = 2^-64.6
constexpr int PP_SEG = 128;         // coefficients per workgroup of coef_x
constexpr int PP_TX = 64;           // coef_y tile: 64 columns x 32 rows of output, 32 + 2 * 34 rows of input in LDS (51 200 bytes)
constexpr int PP_TY = 32;
constexpr int PP_MAX_DIM = 32768;   // an axis of either map

struct PpWs {
  float* part;       // [B][C][2] min / max per chunk (clip)
  double* t1;        // [B][h][w] prefiltered along x (order 3)
  double* coef;      // [B][h][w] spline coefficients (order 3)
  float* g[2];       // `gauss` arrays [B][h][w]: the map after the Gaussian pass along y, then along x
  size_t bytes;
};

static inline long pp_chunks(long n) { return (n + PP_CHUNK - 1) / PP_CHUNK; }

static PpWs pp_layout(void* base, int B, long n, bool part, bool cubic, int gauss = 0) {
  PpWs w;
  char* p = static_cast<char*>(base);
  size_t off = 0;
  auto take = [&](size_t bytes) { char* r = p + off; off += (bytes + 15) & ~static_cast<size_t>(15); return r; };
  w.part = part ? reinterpret_cast<float*>(take(static_cast<size_t>(B) * pp_chunks(n) * 2 * 4)) : nullptr;
  w.t1 = cubic ? reinterpret_cast<double*>(take(static_cast<size_t>(B) * n * 8)) : nullptr;
  w.coef = cubic ? reinterpret_cast<double*>(take(static_cast<size_t>(B) * n * 8)) : nullptr;
  for (int i = 0; i < 2; ++i) w.g[i] = i < gauss ? reinterpret_cast<float*>(take(static_cast<size_t>(B) * n * 4)) : nullptr;
  w.bytes = off;
  return w;
}

// whole-sample mirror extension: period 2(n - 1), n >= 2; any integer j (one definition, shared with the host check)
__device__ __forceinline__ int pp_mirror(int j, int n) { return gauss::mirror(j, n); }

// min and max over the workgroup (blockDim.x a multiple of 64, at most 256); sh holds 8 floats
__device__ __forceinline__ void pp_block_minmax(float& mn, float& mx, float* sh) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    mn = fminf(mn, __shfl_xor(mn, o, kWave));
    mx = fmaxf(mx, __shfl_xor(mx, o, kWave));
  }
  const int nw = blockDim.x >> 6;
  __syncthreads();
  if ((threadIdx.x & 63) == 0) { sh[threadIdx.x >> 6] = mn; sh[4 + (threadIdx.x >> 6)] = mx; }
  __syncthreads();
  mn = sh[0]; mx = sh[4];
  for (int w = 1; w < nw; ++w) { mn = fminf(mn, sh[w]); mx = fmaxf(mx, sh[4 + w]); }
}

// min / max of image b from its chunk partials, in every thread of the workgroup
__device__ __forceinline__ void pp_image_minmax(const float* __restrict__ part, int b, long C, int tid, int nthreads, float& mn,
                                                float& mx, float* sh) {
  mn = __builtin_inff(); mx = -__builtin_inff();
  const float* p = part + static_cast<long>(b) * C * 2;
  for (long c = tid; c < C; c += nthreads) { mn = fminf(mn, p[2 * c]); mx = fmaxf(mx, p[2 * c + 1]); }
  pp_block_minmax(mn, mx, sh);
}

__global__ __launch_bounds__(256) void pp_minmax_kernel(const float* __restrict__ in, float* __restrict__ part, long n, int vec) {
  __shared__ float sh[8];
  const int b = blockIdx.y;
  const long C = gridDim.x, chunk = blockIdx.x;
  const long lo = chunk * PP_CHUNK, hi = lo + PP_CHUNK < n ? lo + PP_CHUNK : n;
  const float* pb = in + static_cast<long>(b) * n;
  float mn = __builtin_inff(), mx = -__builtin_inff();
  if (vec) {      // n % 4 == 0 and a 16-byte aligned base: every chunk is a whole number of float4
    for (long i = lo + 4 * threadIdx.x; i < hi; i += 4 * 256) {
      const float4 v = *reinterpret_cast<const float4*>(pb + i);
      mn = fminf(fminf(mn, v.x), fminf(fminf(v.y, v.z), v.w));
      mx = fmaxf(fmaxf(mx, v.x), fmaxf(fmaxf(v.y, v.z), v.w));
    }
  } else {
    for (long i = lo + threadIdx.x; i < hi; i += 256) { const float v = pb[i]; mn = fminf(mn, v); mx = fmaxf(mx, v); }
  }
  pp_block_minmax(mn, mx, sh);
  if (threadIdx.x == 0) {
    float* o = part + (static_cast<long>(b) * C + chunk) * 2;
    o[0] = mn; o[1] = mx;
  }
}

// normalize_data in fp32: one subtraction, one product with s = 255 / (max - min) (one IEEE division), clamp, truncation
__device__ __forceinline__ unsigned char pp_byte(float x, float mn, float s, bool flat) {
  const float v = fminf(fmaxf((x - mn) * s, 0.0f), 255.0f);
  return flat ? static_cast<unsigned char>(0) : static_cast<unsigned char>(static_cast<int>(v));
}
__device__ __forceinline__ float pp_unbyte(unsigned char q) { return static_cast<float>(q) / 255.0f; }      // plt.imread of an 8-bit PNG

__global__ __launch_bounds__(256) void pp_quant_kernel(const float* __restrict__ in, const float* __restrict__ part,
                                                       unsigned char* __restrict__ u8, float* __restrict__ f, long n, int vec) {
  __shared__ float sh[8];
  const int b = blockIdx.y;
  const long C = gridDim.x, chunk = blockIdx.x;
  float mn, mx;
  pp_image_minmax(part, b, C, threadIdx.x, 256, mn, mx, sh);
  const bool flat = !(mx > mn);
  const float s = 255.0f / (mx - mn);
  const long lo = chunk * PP_CHUNK, hi = lo + PP_CHUNK < n ? lo + PP_CHUNK : n;
  const long bo = static_cast<long>(b) * n;
  const float* pb = in + bo;
  if (vec) {
    for (long i = lo + 4 * threadIdx.x; i < hi; i += 4 * 256) {
      const float4 v = *reinterpret_cast<const float4*>(pb + i);
      uchar4 q;
      q.x = pp_byte(v.x, mn, s, flat); q.y = pp_byte(v.y, mn, s, flat); q.z = pp_byte(v.z, mn, s, flat); q.w = pp_byte(v.w, mn, s, flat);
      if (u8) *reinterpret_cast<uchar4*>(u8 + bo + i) = q;
      if (f) *reinterpret_cast<float4*>(f + bo + i) = make_float4(pp_unbyte(q.x), pp_unbyte(q.y), pp_unbyte(q.z), pp_unbyte(q.w));
    }
  } else {
    for (long i = lo + threadIdx.x; i < hi; i += 256) {
      const unsigned char q = pp_byte(pb[i], mn, s, flat);
      if (u8) u8[bo + i] = q;
      if (f) f[bo + i] = pp_unbyte(q);
    }
  }
}

__global__ __launch_bounds__(256) void pp_from_u8_kernel(const unsigned char* __restrict__ u8, float* __restrict__ f, long total, int vec) {
  const long i = (static_cast<long>(blockIdx.x) * 256 + threadIdx.x) * 4;
  if (i >= total) return;
  if (vec && i + 3 < total) {
    const uchar4 q = *reinterpret_cast<const uchar4*>(u8 + i);
    *reinterpret_cast<float4*>(f + i) = make_float4(pp_unbyte(q.x), pp_unbyte(q.y), pp_unbyte(q.z), pp_unbyte(q.w));
  } else {
    const long e = i + 4 < total ? i + 4 : total;
    for (long j = i; j < e; ++j) f[j] = pp_unbyte(u8[j]);
  }
}

// sqrt(3) - 2 and sqrt(3), correctly rounded
#define PP_Z (-0.26794919243112270647)
#define PP_SQRT3 (1.73205080756887729353)

// prefilter along x: workgroup = PP_SEG consecutive coefficients of one row
__global__ __launch_bounds__(PP_SEG) void pp_coef_x_kernel(const float* __restrict__ in, double* __restrict__ t1, int h, int w) {
  __shared__ float ext[PP_SEG + 2 * PP_K];
  const int x0 = blockIdx.x * PP_SEG, y = blockIdx.y, b = blockIdx.z;
  const long ro = (static_cast<long>(b) * h + y) * w;
  const float* row = in + ro;
  for (int j = threadIdx.x; j < PP_SEG + 2 * PP_K; j += PP_SEG) ext[j] = row[pp_mirror(x0 - PP_K + j, w)];
  __syncthreads();
  const int x = x0 + threadIdx.x;
  if (x >= w) return;
  const float* e = ext + threadIdx.x + PP_K;
  double acc = 0.0;
#pragma unroll
  for (int k = PP_K; k >= 1; --k) acc = (acc + (static_cast<double>(e[k]) + static_cast<double>(e[-k]))) * PP_Z;
  t1[ro + x] = PP_SQRT3 * (static_cast<double>(e[0]) + acc);
}

// prefilter along y: workgroup = a tile of PP_TX columns x PP_TY rows of coefficients; 256 threads = 64 columns x 4 row groups
__global__ __launch_bounds__(256) void pp_coef_y_kernel(const double* __restrict__ t1, double* __restrict__ coef, int h, int w) {
  __shared__ double tile[PP_TY + 2 * PP_K][PP_TX];
  const int tx = threadIdx.x & 63, tg = threadIdx.x >> 6;
  const int x = blockIdx.x * PP_TX + tx, y0 = blockIdx.y * PP_TY, b = blockIdx.z;
  const long io = static_cast<long>(b) * h * w;
  for (int r = tg; r < PP_TY + 2 * PP_K; r += 4) {
    const int yy = pp_mirror(y0 - PP_K + r, h);
    tile[r][tx] = x < w ? t1[io + static_cast<long>(yy) * w + x] : 0.0;
  }
  __syncthreads();
  if (x >= w) return;
  for (int ly = tg; ly < PP_TY; ly += 4) {
    const int y = y0 + ly;
    if (y >= h) break;
    double acc = 0.0;
#pragma unroll
    for (int k = PP_K; k >= 1; --k) acc = (acc + (tile[ly + PP_K + k][tx] + tile[ly + PP_K - k][tx])) * PP_Z;
    coef[io + static_cast<long>(y) * w + x] = PP_SQRT3 * (tile[ly + PP_K][tx] + acc);
  }
}

// The anti-aliasing Gaussian's weights of one axis, centre first, passed by value as a kernel argument: no device allocation, no
// copy, capturable.  Entries above the radius are zero.
struct PpGaussW {
  double g[gauss::kMaxRadius + 1];
};

// Gaussian along x: workgroup = kSeg consecutive samples of one row; the row segment with r mirrored samples on both sides in LDS
__global__ __launch_bounds__(gauss::kSeg) void pp_gauss_x_kernel(const float* __restrict__ in, float* __restrict__ out, int h, int w, int r,
                                                            const PpGaussW wt) {
  __shared__ float ext[gauss::kSeg + 2 * gauss::kMaxRadius];
  __shared__ double g[gauss::kMaxRadius + 1];
  const int x0 = blockIdx.x * gauss::kSeg, y = blockIdx.y, b = blockIdx.z;
  const long ro = (static_cast<long>(b) * h + y) * w;
  const float* row = in + ro;
  for (int j = threadIdx.x; j < gauss::kSeg + 2 * r; j += gauss::kSeg) ext[j] = row[gauss::mirror(x0 - r + j, w)];
  if (static_cast<int>(threadIdx.x) <= r) g[threadIdx.x] = wt.g[threadIdx.x];
  __syncthreads();
  const int x = x0 + threadIdx.x;
  if (x >= w) return;
  out[ro + x] = gauss::sample(ext + threadIdx.x + r, 1, r, g);
}

// Gaussian along y: workgroup = a tile of kTX columns x kTY rows; kTY + 2 r rows of input in LDS (at most 40 960 bytes);
// 256 threads = 64 columns x 4 row groups
__global__ __launch_bounds__(256) void pp_gauss_y_kernel(const float* __restrict__ in, float* __restrict__ out, int h, int w, int r,
                                                         const PpGaussW wt) {
  __shared__ float tile[gauss::kTY + 2 * gauss::kMaxRadius][gauss::kTX];
  __shared__ double g[gauss::kMaxRadius + 1];
  const int tx = threadIdx.x & 63, tg = threadIdx.x >> 6;
  const int x = blockIdx.x * gauss::kTX + tx, y0 = blockIdx.y * gauss::kTY, b = blockIdx.z;
  const long io = static_cast<long>(b) * h * w;
  for (int rr = tg; rr < gauss::kTY + 2 * r; rr += 4) {
    const int yy = gauss::mirror(y0 - r + rr, h);
    tile[rr][tx] = x < w ? in[io + static_cast<long>(yy) * w + x] : 0.0f;
  }
  if (static_cast<int>(threadIdx.x) <= r) g[threadIdx.x] = wt.g[threadIdx.x];
  __syncthreads();
  if (x >= w) return;
  for (int ly = tg; ly < gauss::kTY; ly += 4) {
    const int y = y0 + ly;
    if (y >= h) break;
    out[io + static_cast<long>(y) * w + x] = gauss::sample(&tile[ly + r][tx], gauss::kTX, r, g);
  }
}

// six times the cubic B-spline: 4 - 6 t^2 + 3 |t|^3 for |t| < 1, (2 - |t|)^3 for |t| < 2, else 0; the two factors 1 / 6 of a
// pixel's separable sum are taken out of it as one division by 36
__device__ __forceinline__ double pp_beta3x6(double t) {
  const double a = fabs(t);
  if (a < 1.0) return 4.0 - 6.0 * a * a + 3.0 * a * a * a;
  if (a < 2.0) { const double u = 2.0 - a; return u * u * u; }
  return 0.0;
}

// taps and weights of output coordinate o on an axis of n samples: position x = (o + 0.5) * ratio - 0.5, ratio = n / N (scipy's
// grid_mode), taps floor(x) .. floor(x) + 1 (order 1) or floor(x) - 1 .. floor(x) + 2 (order 3, weights x 6).  Only the border
// taps leave [0, n - 1]: the modulo of the mirror is off the common path
template <int ORDER>
__device__ __forceinline__ void pp_taps(int o, double ratio, int n, int* idx, double* wgt) {
  constexpr int T = ORDER == 3 ? 4 : 2;
  const double x = (o + 0.5) * ratio - 0.5;
  const double fd = floor(x);
  const int f = static_cast<int>(fd) - (ORDER == 3 ? 1 : 0);
  if (ORDER == 3) {
#pragma unroll
    for (int k = 0; k < T; ++k) wgt[k] = pp_beta3x6(x - (fd + (k - 1)));
  } else {
    wgt[1] = x - fd; wgt[0] = 1.0 - wgt[1];
  }
#pragma unroll
  for (int k = 0; k < T; ++k) { const int j = f + k; idx[k] = (j >= 0 && j < n) ? j : pp_mirror(j, n); }
}

constexpr int PP_ROWS = 4;      // output rows per thread of interp: the x taps are computed once for them

// Workgroup = 64 output columns x 16 output rows: thread (lane, wave) makes column X = 64 bx + lane of rows 16 by + 4 wave + 0..3.
// Order 1 reads the source, order 3 the coefficients.
template <int ORDER, typename SRC, typename DST>
__global__ __launch_bounds__(256) void pp_interp_kernel(const SRC* __restrict__ src, const float* __restrict__ part, DST* __restrict__ out,
                                                        int h, int w, int H, int W, double ry, double rx, long C) {
  __shared__ float sh[8];
  constexpr int T = ORDER == 3 ? 4 : 2;
  const int b = blockIdx.z;
  float mn = 0.f, mx = 0.f;
  if (part) pp_image_minmax(part, b, C, threadIdx.x, 256, mn, mx, sh);      // uniform: every thread reaches the barriers
  const int X = blockIdx.x * 64 + (threadIdx.x & 63), Y0 = (blockIdx.y * 4 + (threadIdx.x >> 6)) * PP_ROWS;
  if (X >= W || Y0 >= H) return;
  double wx[T], wy[T];
  int ix[T], iy[T];
  pp_taps<ORDER>(X, rx, w, ix, wx);
  const SRC* sb = src + static_cast<long>(b) * h * w;
  for (int r = 0; r < PP_ROWS; ++r) {
    const int Y = Y0 + r;
    if (Y >= H) break;
    pp_taps<ORDER>(Y, ry, h, iy, wy);
    double v = 0.0;
#pragma unroll
    for (int j = 0; j < T; ++j) {
      const SRC* row = sb + static_cast<long>(iy[j]) * w;
      double a = 0.0;
#pragma unroll
      for (int i = 0; i < T; ++i) a += wx[i] * static_cast<double>(row[ix[i]]);
      v += wy[j] * a;
    }
    if (ORDER == 3) v /= 36.0;
    if (part) v = fmin(fmax(v, static_cast<double>(mn)), static_cast<double>(mx));
    out[(static_cast<long>(b) * H + Y) * W + X] = static_cast<DST>(v);      // fp32: the one rounding of the whole path
  }
}

static int pp_minmax_launch(const float* in, float* part, int B, long n, hipStream_t s, const char* what) {
  const int vec = (n % 4 == 0 && aligned16(in)) ? 1 : 0;
  hipLaunchKernelGGL(pp_minmax_kernel, dim3(static_cast<unsigned>(pp_chunks(n)), B), dim3(256), 0, s, in, part, n, vec);
  return check_launch(what);
}

}  // namespace diffsal

using namespace diffsal;

extern "C" size_t diffsal_map_to_u8_ws_bytes(int B, long n) {
  if (B <= 0 || n <= 0) return 0;
  return pp_layout(nullptr, B, n, true, false).bytes;
}

extern "C" int diffsal_map_to_u8(const float* pred, int B, long n, unsigned char* u8, float* f, void* ws, size_t ws_bytes,
                                 diffsal_stream_t stream) {
  DS_REQUIRE(pred && ws && (u8 || f), DIFFSAL_E_ARG, "map_to_u8: null argument");
  DS_REQUIRE(B > 0 && B <= 65535 && n > 0 && n < (1L << 31), DIFFSAL_E_SHAPE, "map_to_u8: bad shape B=%d (1..65535) n=%ld (1..2^31-1)", B, n);
  const PpWs w = pp_layout(ws, B, n, true, false);
  DS_REQUIRE(ws_bytes >= w.bytes && aligned16(ws), DIFFSAL_E_ARG, "map_to_u8: workspace too small or misaligned");
  hipStream_t s = static_cast<hipStream_t>(stream);
  int rc = pp_minmax_launch(pred, w.part, B, n, s, "map_to_u8(minmax)");
  if (rc) return rc;
  const int vec = (n % 4 == 0 && aligned16(pred) && (!f || aligned16(f)) && (!u8 || (reinterpret_cast<uintptr_t>(u8) & 3u) == 0)) ? 1 : 0;
  hipLaunchKernelGGL(pp_quant_kernel, dim3(static_cast<unsigned>(pp_chunks(n)), B), dim3(256), 0, s, pred, w.part, u8, f, n, vec);
  return check_launch("map_to_u8(quant)");
}

extern "C" int diffsal_map_from_u8(const unsigned char* u8, long total, float* f, diffsal_stream_t stream) {
  DS_REQUIRE(u8 && f, DIFFSAL_E_ARG, "map_from_u8: null argument");
  DS_REQUIRE(total > 0 && total < (1L << 40), DIFFSAL_E_SHAPE, "map_from_u8: %ld elements (1..2^40-1)", total);
  const int vec = (aligned16(f) && (reinterpret_cast<uintptr_t>(u8) & 3u) == 0) ? 1 : 0;
  hipLaunchKernelGGL(pp_from_u8_kernel, dim3(static_cast<unsigned>((total + 1023) / 1024)), dim3(256), 0, static_cast<hipStream_t>(stream),
                     u8, f, total, vec);
  return check_launch("map_from_u8");
}

static int pp_resize_args(int B, int h, int w, int H, int W, int order, int clip, int out_f64) {
  DS_REQUIRE(order == 1 || order == 3, DIFFSAL_E_ARG, "map_resize: order %d (1 or 3)", order);
  DS_REQUIRE((clip == 0 || clip == 1) && (out_f64 == 0 || out_f64 == 1), DIFFSAL_E_ARG, "map_resize: clip and out_f64 are 0 or 1");
  DS_REQUIRE(B > 0 && B <= 65535, DIFFSAL_E_SHAPE, "map_resize: B=%d (1..65535)", B);
  DS_REQUIRE(h >= 2 && w >= 2, DIFFSAL_E_SHAPE, "map_resize: source %d x %d: the mirror boundary needs at least 2 samples per axis", h, w);
  DS_REQUIRE(H >= h && W >= w, DIFFSAL_E_SHAPE,
             "map_resize: %d x %d -> %d x %d shrinks an axis (a downscale needs an anti-aliasing filter, which is not built)", h, w, H, W);
  DS_REQUIRE(H <= PP_MAX_DIM && W <= PP_MAX_DIM, DIFFSAL_E_SHAPE, "map_resize: target %d x %d above %d", H, W, PP_MAX_DIM);
  return DIFFSAL_OK;
}

extern "C" size_t diffsal_map_resize_ws_bytes(int B, int h, int w, int order, int clip) {
  if (B <= 0 || h <= 0 || w <= 0 || (order != 1 && order != 3)) return 0;
  return pp_layout(nullptr, B, static_cast<long>(h) * w, clip != 0, order == 3).bytes;
}

// The launches of a resize behind the argument checks: the clip's range is `range`'s (the map as it came), the spline reads `in`
// (the same map, or the one the anti-aliasing Gaussian made of it)
static int pp_resize_launches(const float* range, const float* in, int B, int h, int w, int H, int W, bool cubic, int clip, int out_f64,
                              void* out, const PpWs& ww, hipStream_t s) {
  int rc;
  const long n = static_cast<long>(h) * w;
  const long C = pp_chunks(n);
  if (clip && (rc = pp_minmax_launch(range, ww.part, B, n, s, "map_resize(minmax)"))) return rc;
  if (cubic) {
    hipLaunchKernelGGL(pp_coef_x_kernel, dim3((w + PP_SEG - 1) / PP_SEG, h, B), dim3(PP_SEG), 0, s, in, ww.t1, h, w);
    if ((rc = check_launch("map_resize(coef_x)"))) return rc;
    hipLaunchKernelGGL(pp_coef_y_kernel, dim3((w + PP_TX - 1) / PP_TX, (h + PP_TY - 1) / PP_TY, B), dim3(256), 0, s, ww.t1, ww.coef, h, w);
    if ((rc = check_launch("map_resize(coef_y)"))) return rc;
  }
  const dim3 grid((W + 63) / 64, (H + 4 * PP_ROWS - 1) / (4 * PP_ROWS), B);
  const double ry = static_cast<double>(h) / static_cast<double>(H), rx = static_cast<double>(w) / static_cast<double>(W);
  const float* part = clip ? ww.part : nullptr;
  if (cubic && out_f64)
    hipLaunchKernelGGL((pp_interp_kernel<3, double, double>), grid, dim3(256), 0, s, ww.coef, part, static_cast<double*>(out), h, w, H, W, ry, rx, C);
  else if (cubic)
    hipLaunchKernelGGL((pp_interp_kernel<3, double, float>), grid, dim3(256), 0, s, ww.coef, part, static_cast<float*>(out), h, w, H, W, ry, rx, C);
  else if (out_f64)
    hipLaunchKernelGGL((pp_interp_kernel<1, float, double>), grid, dim3(256), 0, s, in, part, static_cast<double*>(out), h, w, H, W, ry, rx, C);
  else
    hipLaunchKernelGGL((pp_interp_kernel<1, float, float>), grid, dim3(256), 0, s, in, part, static_cast<float*>(out), h, w, H, W, ry, rx, C);
  return check_launch("map_resize(interp)");
}

extern "C" int diffsal_map_resize(const float* in, int B, int h, int w, int H, int W, int order, int clip, int out_f64, void* out,
                                  void* ws, size_t ws_bytes, diffsal_stream_t stream) {
  int rc = pp_resize_args(B, h, w, H, W, order, clip, out_f64);
  if (rc) return rc;
  const bool cubic = order == 3;
  DS_REQUIRE(in && out && (ws || !(clip || cubic)), DIFFSAL_E_ARG, "map_resize: null argument");
  const PpWs ww = pp_layout(ws, B, static_cast<long>(h) * w, clip != 0, cubic);
  DS_REQUIRE(ww.bytes == 0 || (ws_bytes >= ww.bytes && aligned16(ws)), DIFFSAL_E_ARG, "map_resize: workspace too small or misaligned");
  return pp_resize_launches(in, in, B, h, w, H, W, cubic, clip, out_f64, out, ww, static_cast<hipStream_t>(stream));
}

// ---- the anti-aliasing Gaussian in front of a downscale ----
static int pp_gauss_args(const char* what, int B, int h, int w, const double* wy, int ry, const double* wx, int rx) {
  DS_REQUIRE(B > 0 && B <= 65535, DIFFSAL_E_SHAPE, "%s: B=%d (1..65535)", what, B);
  DS_REQUIRE(h >= 2 && w >= 2 && h <= PP_MAX_DIM && w <= PP_MAX_DIM, DIFFSAL_E_SHAPE,
             "%s: source %d x %d: the mirror boundary needs at least 2 samples per axis, an axis has at most %d", what, h, w, PP_MAX_DIM);
  DS_REQUIRE(ry >= 0 && rx >= 0, DIFFSAL_E_ARG, "%s: negative radius (%d, %d)", what, ry, rx);
  DS_REQUIRE(ry <= gauss::kMaxRadius && rx <= gauss::kMaxRadius, DIFFSAL_E_SHAPE,
             "%s: radius (%d, %d) above %d: the anti-aliasing Gaussian is built for sigma < 16, a downscale factor below 33", what, ry, rx,
             gauss::kMaxRadius);
  DS_REQUIRE((ry == 0 || wy) && (rx == 0 || wx), DIFFSAL_E_ARG, "%s: a radius above 0 without its weights", what);
  return DIFFSAL_OK;
}

static PpGaussW pp_gauss_weights(const double* g, int r) {
  PpGaussW k = {};
  for (int i = 0; i <= r; ++i) k.g[i] = g ? g[i] : 1.0;
  return k;
}

// the passes of the Gaussian, y first: in -> ... -> the returned map, which is `in` itself when neither axis has a radius, else t[0]
// (one pass) or t[1] (two passes: t[0] holds the map between them)
static int pp_gauss_launches(const float* in, int B, int h, int w, const double* wy, int ry, const double* wx, int rx, float* const t[2],
                             hipStream_t s, const char* what_y, const char* what_x, const float** result) {
  int rc;
  const float* cur = in;
  int next = 0;
  if (ry > 0) {
    hipLaunchKernelGGL(pp_gauss_y_kernel, dim3((w + gauss::kTX - 1) / gauss::kTX, (h + gauss::kTY - 1) / gauss::kTY, B), dim3(256), 0, s, cur, t[next], h, w, ry,
                       pp_gauss_weights(wy, ry));
    if ((rc = check_launch(what_y))) return rc;
    cur = t[next++];
  }
  if (rx > 0) {
    hipLaunchKernelGGL(pp_gauss_x_kernel, dim3((w + gauss::kSeg - 1) / gauss::kSeg, h, B), dim3(gauss::kSeg), 0, s, cur, t[next], h, w, rx,
                       pp_gauss_weights(wx, rx));
    if ((rc = check_launch(what_x))) return rc;
    cur = t[next++];
  }
  *result = cur;
  return DIFFSAL_OK;
}

extern "C" size_t diffsal_map_gauss_ws_bytes(int B, int h, int w) {
  if (B <= 0 || h <= 0 || w <= 0) return 0;
  return pp_layout(nullptr, B, static_cast<long>(h) * w, false, false, 1).bytes;
}

extern "C" int diffsal_map_gauss(const float* in, int B, int h, int w, const double* wy, int ry, const double* wx, int rx, float* out,
                                 void* ws, size_t ws_bytes, diffsal_stream_t stream) {
  int rc = pp_gauss_args("map_gauss", B, h, w, wy, ry, wx, rx);
  if (rc) return rc;
  const bool both = ry > 0 && rx > 0;
  DS_REQUIRE(in && out && in != out && (ws || !both), DIFFSAL_E_ARG, "map_gauss: null argument, or out is in");
  const PpWs ww = pp_layout(ws, B, static_cast<long>(h) * w, false, false, 1);
  DS_REQUIRE(!both || (ws_bytes >= ww.bytes && aligned16(ws)), DIFFSAL_E_ARG, "map_gauss: workspace too small or misaligned");
  hipStream_t s = static_cast<hipStream_t>(stream);
  if (ry == 0 && rx == 0) {      // no axis shrinks: the identity, as one pass of weight 1 (x * 1.0 is exact)
    hipLaunchKernelGGL(pp_gauss_x_kernel, dim3((w + gauss::kSeg - 1) / gauss::kSeg, h, B), dim3(gauss::kSeg), 0, s, in, out, h, w, 0,
                       pp_gauss_weights(nullptr, 0));
    return check_launch("map_gauss(copy)");
  }
  const float* res;
  float* const t[2] = {both ? ww.g[0] : out, out};
  return pp_gauss_launches(in, B, h, w, wy, ry, wx, rx, t, s, "map_gauss(gauss_y)", "map_gauss(gauss_x)", &res);
}

extern "C" size_t diffsal_map_resize_aa_ws_bytes(int B, int h, int w, int order, int clip) {
  if (B <= 0 || h <= 0 || w <= 0 || (order != 1 && order != 3)) return 0;
  return pp_layout(nullptr, B, static_cast<long>(h) * w, clip != 0, order == 3, 2).bytes;
}

extern "C" int diffsal_map_resize_aa(const float* in, int B, int h, int w, int H, int W, int order, int clip, int out_f64, const double* wy,
                                     int ry, const double* wx, int rx, void* out, void* ws, size_t ws_bytes, diffsal_stream_t stream) {
  DS_REQUIRE(order == 1 || order == 3, DIFFSAL_E_ARG, "map_resize_aa: order %d (1 or 3)", order);
  DS_REQUIRE((clip == 0 || clip == 1) && (out_f64 == 0 || out_f64 == 1), DIFFSAL_E_ARG, "map_resize_aa: clip and out_f64 are 0 or 1");
  int rc = pp_gauss_args("map_resize_aa", B, h, w, wy, ry, wx, rx);
  if (rc) return rc;
  DS_REQUIRE(H >= 1 && W >= 1 && H <= PP_MAX_DIM && W <= PP_MAX_DIM, DIFFSAL_E_SHAPE, "map_resize_aa: target %d x %d (1..%d per axis)", H, W,
             PP_MAX_DIM);
  const bool cubic = order == 3;
  DS_REQUIRE(in && out && ws, DIFFSAL_E_ARG, "map_resize_aa: null argument");
  const PpWs ww = pp_layout(ws, B, static_cast<long>(h) * w, clip != 0, cubic, 2);
  DS_REQUIRE(ws_bytes >= ww.bytes && aligned16(ws), DIFFSAL_E_ARG, "map_resize_aa: workspace too small or misaligned");
  hipStream_t s = static_cast<hipStream_t>(stream);
  const float* filtered;
  if ((rc = pp_gauss_launches(in, B, h, w, wy, ry, wx, rx, ww.g, s, "map_resize_aa(gauss_y)", "map_resize_aa(gauss_x)", &filtered))) return rc;
  return pp_resize_launches(in, filtered, B, h, w, H, W, cubic, clip, out_f64, out, ww, s);
}
