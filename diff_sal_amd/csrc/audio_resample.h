// The arithmetic and the index arithmetic of the audio front end's resampling stage (include/diffsal.h, "audio front end":
// resampy 0.4.2's resample and _resample_loop), callable from the host and from the device: csrc/audio_input.hip runs it in a
// kernel, tools/resample_host_check.cpp runs the same functions serially on the host, where a sanitizer can watch every buffer.
// Every float64 operation of an output sample is rounded on its own, in the library's order: rs_mul / rs_add / rs_sub are single
// operations compiled with contraction off, so no product is fused into the sum that follows it wherever they are inlined.
// (__dmul_rn / __dadd_rn do not pin that here: the toolchain's headers define them as the plain operators, which carry the
// translation unit's permission to contract, and a first form of the kernel written with them came out as v_fmac_f64.  The
// kernel's code holds no fused fp64 instruction; DESIGN.md, "Audio front end", says how that is looked at.)  A host compiler
// that is not clang needs -ffp-contract=off.
#pragma once

#if defined(__HIPCC__)
#define RS_HD __host__ __device__ __forceinline__
#else
#define RS_HD inline
#endif
#if defined(__clang__)
#define RS_NO_CONTRACT _Pragma("clang fp contract(off)")
#else
#define RS_NO_CONTRACT
#endif

namespace diffsal {
namespace resample {

RS_HD double rs_mul(double a, double b) { RS_NO_CONTRACT return a * b; }
RS_HD double rs_add(double a, double b) { RS_NO_CONTRACT return a + b; }
RS_HD double rs_sub(double a, double b) { RS_NO_CONTRACT return a - b; }

constexpr int kTile = 256;             // outputs per workgroup, one thread each
constexpr int kMaxSpan = 8192;         // input samples a tile may stage: 64 KB of fp64 LDS

// the excerpt wav[start : end + 1] of a video of n valid samples as numpy slices it, centred in the window (diffsal_logmel's rule)
struct Excerpt {
  long lo;       // first sample read, an index into the video's waveform
  long v;        // samples in the excerpt; lo + v <= n
  long off;      // window position of the excerpt's first sample; negative for an unchecked v > window (centre crop)
};

RS_HD Excerpt excerpt(long start, long end, long n, long Lmax, long window) {
  n = n < 0 ? 0 : (n > Lmax ? Lmax : n);
  const long st = start < 0 ? 0 : start, en = end < 0 ? 0 : end;
  const long lo = st < n ? st : n, hi = en + 1 < n ? en + 1 : n;
  Excerpt e;
  e.lo = lo;
  e.v = hi > lo ? hi - lo : 0;
  e.off = window / 2 - e.v / 2;
  return e;
}

// index into the waveform of window position p, or -1 where the padded buffer holds a zero
RS_HD long source_index(const Excerpt& e, long p, long window) {
  const long j = p - e.off;
  return (p >= 0 && p < window && j >= 0 && j < e.v) ? e.lo + j : -1;
}

// int(n * sr_new / sr_orig): the product is exact in integers, the quotient one float64 division, truncated
RS_HD long out_len(long n, int sr_orig, int sr_new) {
  return static_cast<long>(static_cast<double>(n * static_cast<long>(sr_new)) / static_cast<double>(sr_orig));
}

struct Plan {
  double scale;      // min(1, ratio)
  double inc;        // 1 / ratio: input samples per output sample
  int step;          // int(scale * num_table), truncated
  int wing;          // nwin / step: the most taps one wing can have
  int max_span;      // the most input samples a tile of kTile outputs reads
};

inline Plan plan(int sr_orig, int sr_new, int nwin, int num_table) {
  const double ratio = static_cast<double>(sr_new) / static_cast<double>(sr_orig);
  Plan p;
  p.scale = ratio < 1.0 ? ratio : 1.0;
  p.inc = 1.0 / ratio;
  p.step = static_cast<int>(p.scale * static_cast<double>(num_table));
  p.wing = p.step >= 1 ? nwin / p.step : 0;
  const double reach = static_cast<double>(kTile - 1) * p.inc + 2.0 + 2.0 * p.wing;
  p.max_span = reach < 1e9 ? static_cast<int>(reach) : 1000000000;
  return p;
}

// m = int(t * inc): the input sample at or before output t (t and m are below 2^25: the window is at most 2^24 samples and a
// tile reaches at most kMaxSpan past it).  Monotone in t, so a tile's first and last output bound the rest
RS_HD int input_index(int t, double inc) { return static_cast<int>(rs_mul(static_cast<double>(t), inc)); }

// the inputs outputs t0 .. t1 (one tile) can read: window positions base .. base + span - 1
RS_HD void tile_span(int t0, int t1, double inc, int wing, int& base, int& span) {
  const int m0 = input_index(t0, inc), m1 = input_index(t1, inc);
  base = m0 - (wing - 1);
  span = m1 - m0 + 2 * wing;
}

// Output sample t.  xs holds window positions base .. (zeros where the padded buffer is zero), tab the interleaved
// (win, delta)[nwin], n the padded buffer's length.  Left wing in ascending i, then right wing in ascending k; every tap is
// product, sum, product, sum.  Reads xs[m - (wing - 1) - base .. m + wing - base] at most and tab[0 .. nwin - 1].
template <typename Tab>
RS_HD double output(int t, const double* xs, int base, const Tab* tab, int nwin, int num_table, double scale, double inc, int step, int n) {
  const double time = rs_mul(static_cast<double>(t), inc);
  const int m = static_cast<int>(time);
  double frac = rs_mul(scale, rs_sub(time, static_cast<double>(m)));
  double f = rs_mul(frac, static_cast<double>(num_table));
  int off = static_cast<int>(f);
  double eta = rs_sub(f, static_cast<double>(off));
  double y = 0.0;
  int cnt = off <= nwin ? (nwin - off) / step : 0;
  cnt = m + 1 < cnt ? m + 1 : cnt;
  const double* x = xs + (m - base);
  for (int i = 0; i < cnt; ++i) {
    const Tab w = tab[off + i * step];
    y = rs_add(y, rs_mul(rs_add(w.x, rs_mul(eta, w.y)), x[-i]));
  }
  frac = rs_sub(scale, frac);
  f = rs_mul(frac, static_cast<double>(num_table));
  off = static_cast<int>(f);
  eta = rs_sub(f, static_cast<double>(off));
  cnt = off <= nwin ? (nwin - off) / step : 0;
  cnt = n - m - 1 < cnt ? n - m - 1 : cnt;
  for (int k = 0; k < cnt; ++k) {
    const Tab w = tab[off + k * step];
    y = rs_add(y, rs_mul(rs_add(w.x, rs_mul(eta, w.y)), x[k + 1]));
  }
  return y;
}

}  // namespace resample
}  // namespace diffsal
