// The resampling stage's index arithmetic (diff_sal_amd/csrc/audio_resample.h) run serially on the host, one loop iteration per
// device thread, on heap buffers of exactly the sizes the library works with: the waveform [V][Lmax], a tile's staged span of
// Plan::max_span samples (the launch's LDS), the table [nwin][2], the output [B][n_samples].  Built with a sanitizer, an access
// outside them stops the program.  No GPU and no HIP needed.
//   c++ -std=c++17 -O1 -g -ffp-contract=off -fsanitize=address,undefined -fno-sanitize-recover=all tools/resample_host_check.cpp -o resample_host_check
//   resample_host_check        every rate pair below x excerpts that fill the window, have an odd and an even length, are empty,
//                              are clamped at the end of the audio, start below zero, and are longer than the window (the
//                              unchecked case the kernel centre-crops); each output is also computed from a materialised padded
//                              buffer with the loop of include/diffsal.h as written, and must agree bit for bit
// No test runs this.  The table holds arbitrary values: the index arithmetic does not depend on the filter's design.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../diff_sal_amd/csrc/audio_resample.h"

using namespace diffsal::resample;

struct Tap { double x, y; };

static void fail(const char* what, long a, long b) {
  std::fprintf(stderr, "resample_host_check: %s (%ld, %ld)\n", what, a, b);
  std::exit(2);
}

// the loop of include/diffsal.h on a padded buffer that exists in memory
static double direct(long t, const std::vector<double>& x, const std::vector<Tap>& tab, int num_table, const Plan& p) {
  const long n = static_cast<long>(x.size()), nwin = static_cast<long>(tab.size());
  const double time = rs_mul(static_cast<double>(t), p.inc);
  const long m = static_cast<long>(time);
  double frac = rs_mul(p.scale, rs_sub(time, static_cast<double>(m)));
  double f = rs_mul(frac, num_table);
  long off = static_cast<long>(f);
  double eta = rs_sub(f, static_cast<double>(off));
  double y = 0.0;
  long cnt = (nwin - off) / p.step;
  if (m + 1 < cnt) cnt = m + 1;
  for (long i = 0; i < cnt; ++i)
    y = rs_add(y, rs_mul(rs_add(tab.at(off + i * p.step).x, rs_mul(eta, tab.at(off + i * p.step).y)), x.at(m - i)));
  frac = rs_sub(p.scale, frac);
  f = rs_mul(frac, num_table);
  off = static_cast<long>(f);
  eta = rs_sub(f, static_cast<double>(off));
  cnt = (nwin - off) / p.step;
  if (n - m - 1 < cnt) cnt = n - m - 1;
  for (long k = 0; k < cnt; ++k)
    y = rs_add(y, rs_mul(rs_add(tab.at(off + k * p.step).x, rs_mul(eta, tab.at(off + k * p.step).y)), x.at(m + k + 1)));
  return y;
}

static unsigned long long bits(double d) {
  unsigned long long u;
  static_assert(sizeof(u) == sizeof(d), "fp64");
  __builtin_memcpy(&u, &d, sizeof(u));
  return u;
}

static long run(int sr_orig, int sr_new, int nwin, int num_table, int window) {
  const Plan p = plan(sr_orig, sr_new, nwin, num_table);
  if (p.step < 1 || p.wing < 1 || p.max_span > kMaxSpan) fail("a plan the library refuses", p.step, p.max_span);
  std::vector<Tap> tab(nwin);
  unsigned s = 12345u + static_cast<unsigned>(sr_orig);
  for (auto& w : tab) {
    s = s * 1664525u + 1013904223u;
    w.x = static_cast<double>(s >> 8) / 16777216.0 - 0.5;
    s = s * 1664525u + 1013904223u;
    w.y = (static_cast<double>(s >> 8) / 16777216.0 - 0.5) / 64.0;
  }
  const int V = 2;
  const long Lmax = 3L * window + 11;
  const long wav_len[V] = {Lmax, 2L * window + 5};
  std::vector<short> wav(static_cast<size_t>(V) * Lmax);
  for (auto& v : wav) {
    s = s * 1664525u + 1013904223u;
    v = static_cast<short>(s >> 16);
  }
  struct Clip { int video; long start, end; };
  const Clip clips[] = {{0, 7, 7 + window - 1},                                  // fills the window
                        {1, 100, 100 + window / 2},                              // v = window / 2 + 1
                        {1, 101, 101 + window / 2},
                        {0, 50, 50 + window / 2 + 1},                            // the other parity
                        {1, wav_len[1] + 5, wav_len[1] + 900},                   // v = 0
                        {1, wav_len[1] - window / 3, wav_len[1] + 40},           // clamped at the end of the audio
                        {0, -20, window / 4},                                    // a start below zero
                        {0, 3, 3 + 2L * window},                                 // unchecked v > window: centre-cropped
                        {0, 4, 4 + 2L * window + 1}};
  const long n_out = out_len(window, sr_orig, sr_new);
  long done = 0;
  for (const long n_samples : {n_out, n_out > 300 ? n_out - 257 : n_out, 1L}) {
    const size_t B = sizeof(clips) / sizeof(clips[0]);
    std::vector<double> out(B * static_cast<size_t>(n_samples));
    for (size_t b = 0; b < B; ++b) {
      const Clip& c = clips[b];
      const Excerpt e = excerpt(c.start, c.end, wav_len[c.video], Lmax, window);
      if (e.lo < 0 || e.v < 0 || e.lo + e.v > wav_len[c.video]) fail("excerpt outside the audio", e.lo, e.v);
      std::vector<double> padded(window, 0.0);      // what the reference materialises (the centre crop for v > window)
      for (long q = 0; q < window; ++q) {
        const long j = source_index(e, q, window);
        if (j >= 0) padded.at(q) = static_cast<double>(wav.at(static_cast<size_t>(c.video) * Lmax + j)) / 32768.0;
      }
      if (e.v <= window)
        for (long q = 0; q < e.v; ++q)
          if (bits(padded.at(window / 2 - e.v / 2 + q)) != bits(static_cast<double>(wav.at(static_cast<size_t>(c.video) * Lmax + e.lo + q)) / 32768.0))
            fail("centring", static_cast<long>(b), q);
      for (long t0 = 0; t0 < n_samples; t0 += kTile) {                     // workgroup
        const long t1 = t0 + kTile - 1 < n_samples - 1 ? t0 + kTile - 1 : n_samples - 1;
        int base, span;
        tile_span(static_cast<int>(t0), static_cast<int>(t1), p.inc, p.wing, base, span);
        if (span > p.max_span || span < 1) fail("a tile's span against the launch's LDS", span, p.max_span);
        std::vector<double> xs(static_cast<size_t>(p.max_span));           // the launch's LDS
        for (int i = 0; i < span; ++i) {                                    // staging
          const long j = source_index(e, static_cast<long>(base) + i, window);
          xs.at(i) = j >= 0 ? static_cast<double>(wav.at(static_cast<size_t>(c.video) * Lmax + j)) / 32768.0 : 0.0;
        }
        xs.resize(static_cast<size_t>(span));      // what was not staged must not be read: shrink, so that the sanitizer watches it
        xs.shrink_to_fit();
        for (long t = t0; t <= t1; ++t) {                                   // thread
          const double y = output(static_cast<int>(t), xs.data(), base, tab.data(), nwin, num_table, p.scale, p.inc, p.step, window);
          out.at(b * static_cast<size_t>(n_samples) + static_cast<size_t>(t)) = y;
          if (bits(y) != bits(direct(t, padded, tab, num_table, p)))
            fail("an output differs from the loop on the padded buffer", static_cast<long>(b), t);
          ++done;
        }
      }
    }
  }
  std::printf("%6d -> %6d, nwin %5d, window %6d: step %3d, wing %3d, span at most %4d, %ld outputs agree\n", sr_orig, sr_new, nwin, window,
              p.step, p.wing, p.max_span, done);
  return done;
}

int main() {
  long done = 0;
  for (const int window : {1500, 1501, 4097}) {
    done += run(22050, 16000, 32769, 512, window);
    done += run(44100, 16000, 32769, 512, window);
    done += run(48000, 16000, 32769, 512, window);
    done += run(11025, 16000, 32769, 512, window);
    done += run(8000, 16000, 32769, 512, window);
    done += run(22050, 16000, 8193, 512, window);
    done += run(96000, 16000, 32769, 512, window);      // inc = 6: 1530 + 2 + 2 x 385 inputs a tile
    done += run(16000, 44100, 8193, 512, window);
  }
  done += run(22050, 16000, 32769, 512, 35280);
  done += run(8000, 16000, 2, 1, 700);                  // the smallest table the library takes: step 1, wing 2
  std::printf("%ld outputs\n", done);
  return 0;
}
