// One output sample of the anti-aliasing Gaussian in front of a downscale (include/diffsal.h, "benchmark post-processing":
// scipy.ndimage.gaussian_filter's correlate1d for a symmetric kernel) and the mirror fold it reads through, callable from the host
// and from the device: csrc/postprocess.hip runs them in pp_gauss_x_kernel / pp_gauss_y_kernel, tools/postprocess_gauss_host_check.cpp
// runs the same functions serially on the host, where a sanitizer can watch every index.
// Every float64 operation is rounded on its own, in scipy's order: gs_mul / gs_add are single operations compiled with contraction
// off, so no product is fused into the sum that follows it wherever they are inlined (__dmul_rn / __dadd_rn do not pin that: the
// toolchain's headers define them as the plain operators; csrc/audio_resample.h tells the story).  A host compiler that is not clang
// needs -ffp-contract=off.
#pragma once

#if defined(__HIPCC__)
#define GS_HD __host__ __device__ __forceinline__
#else
#define GS_HD inline
#endif
#if defined(__clang__)
#define GS_NO_CONTRACT _Pragma("clang fp contract(off)")
#else
#define GS_NO_CONTRACT
#endif

namespace diffsal {
namespace gauss {

constexpr int kMaxRadius = 64;      // sigma < 16: a downscale factor below 33
constexpr int kSeg = 128;           // samples per workgroup of the pass along x: kSeg + 2 r floats of a row in LDS
constexpr int kTX = 64;             // tile of the pass along y: 64 columns x 32 rows of output, 32 + 2 r rows of input in LDS
constexpr int kTY = 32;

GS_HD double gs_mul(double a, double b) { GS_NO_CONTRACT return a * b; }
GS_HD double gs_add(double a, double b) { GS_NO_CONTRACT return a + b; }

// whole-sample mirror extension: period 2(n - 1), n >= 2; any integer j (a radius above n - 1 folds several times)
GS_HD int mirror(int j, int n) {
  const int p = 2 * (n - 1);
  j %= p;
  if (j < 0) j += p;
  return j > n - 1 ? p - j : j;
}

// e points at the centre sample of a line extended by r mirrored samples on both sides, `stride` elements apart; g[0..r] are the
// normalised weights, centre first.  acc = x[i] g[0]; for k = r .. 1: acc += (x[i - k] + x[i + k]) g[k]; one rounding to float32
GS_HD float sample(const float* e, int stride, int r, const double* g) {
  double acc = gs_mul(static_cast<double>(e[0]), g[0]);
  for (int k = r; k >= 1; --k)
    acc = gs_add(acc, gs_mul(gs_add(static_cast<double>(e[-k * stride]), static_cast<double>(e[k * stride])), g[k]));
  return static_cast<float>(acc);
}

}  // namespace gauss
}  // namespace diffsal
