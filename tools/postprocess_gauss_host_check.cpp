// The anti-aliasing Gaussian's arithmetic and index arithmetic (diff_sal_amd/csrc/postprocess_gauss.h) run serially on the host, one
// loop trip per device thread, with the kernels' workgroup shapes and heap buffers of exactly the sizes of their LDS arrays: built
// with a sanitizer, an access outside them stops the program.  No GPU and no HIP needed.
//   c++ -std=c++17 -O1 -g -ffp-contract=off -fsanitize=address,undefined -fno-sanitize-recover=all tools/postprocess_gauss_host_check.cpp -o postprocess_gauss_host_check
//   postprocess_gauss_host_check in.f32 h w wy.f64 wx.f64 out.f32     one h x w float32 map -> its filtered map; a weight file holds
//                                                                      r + 1 float64, centre first; an empty file means no pass
//   postprocess_gauss_host_check                                       self test: edge shapes (2 samples, one more and one fewer than
//                                                                      a tile, radius 64 on 2 samples) against a plain loop
// No test runs this.  Its maps are scipy's bit for bit (tools/gen_postprocess_aa_golden.py --host-check compares).
#include <cstdio>
#include <cstdlib>
#include <memory>
#include <vector>

#include "../diff_sal_amd/csrc/postprocess_gauss.h"

using namespace diffsal::gauss;

[[noreturn]] static void fail(const char* what, long a = 0, long b = 0) {
  std::fprintf(stderr, "postprocess_gauss_host_check: %s (%ld, %ld)\n", what, a, b);
  std::exit(2);
}

// pp_gauss_x_kernel: grid (ceil(w / kSeg), h), kSeg threads
static void pass_x(const float* in, float* out, int h, int w, int r, const double* wt) {
  std::unique_ptr<float[]> ext(new float[kSeg + 2 * kMaxRadius]);
  std::unique_ptr<double[]> g(new double[kMaxRadius + 1]);
  for (int y = 0; y < h; ++y)
    for (int x0 = 0; x0 < w; x0 += kSeg) {
      const float* row = in + static_cast<long>(y) * w;
      for (int t = 0; t < kSeg; ++t) {
        for (int j = t; j < kSeg + 2 * r; j += kSeg) ext[j] = row[mirror(x0 - r + j, w)];
        if (t <= r) g[t] = wt[t];
      }
      for (int t = 0; t < kSeg; ++t) {
        const int x = x0 + t;
        if (x >= w) continue;
        out[static_cast<long>(y) * w + x] = sample(ext.get() + t + r, 1, r, g.get());
      }
    }
}

// pp_gauss_y_kernel: grid (ceil(w / kTX), ceil(h / kTY)), 256 threads = 64 columns x 4 row groups
static void pass_y(const float* in, float* out, int h, int w, int r, const double* wt) {
  std::unique_ptr<float[]> tile(new float[(kTY + 2 * kMaxRadius) * kTX]);
  std::unique_ptr<double[]> g(new double[kMaxRadius + 1]);
  for (int y0 = 0; y0 < h; y0 += kTY)
    for (int bx = 0; bx * kTX < w; ++bx) {
      for (int t = 0; t < 256; ++t) {
        const int tx = t & 63, tg = t >> 6, x = bx * kTX + tx;
        for (int rr = tg; rr < kTY + 2 * r; rr += 4) {
          const int yy = mirror(y0 - r + rr, h);
          tile[rr * kTX + tx] = x < w ? in[static_cast<long>(yy) * w + x] : 0.0f;
        }
        if (t <= r) g[t] = wt[t];
      }
      for (int t = 0; t < 256; ++t) {
        const int tx = t & 63, tg = t >> 6, x = bx * kTX + tx;
        if (x >= w) continue;
        for (int ly = tg; ly < kTY; ly += 4) {
          const int y = y0 + ly;
          if (y >= h) break;
          out[static_cast<long>(y) * w + x] = sample(&tile[(ly + r) * kTX + tx], kTX, r, g.get());
        }
      }
    }
}

// the library's sequence: rows first, the second pass reads the float32 result of the first; buffers of exactly h * w floats
static std::vector<float> filter(const std::vector<float>& in, int h, int w, const std::vector<double>& wy, const std::vector<double>& wx) {
  const int ry = wy.empty() ? 0 : static_cast<int>(wy.size()) - 1, rx = wx.empty() ? 0 : static_cast<int>(wx.size()) - 1;
  if (h < 2 || w < 2 || ry > kMaxRadius || rx > kMaxRadius) fail("shape or radius outside what the library takes", h, w);
  std::vector<float> cur(in);
  if (ry > 0) { std::vector<float> o(in.size()); pass_y(cur.data(), o.data(), h, w, ry, wy.data()); cur.swap(o); }
  if (rx > 0) { std::vector<float> o(in.size()); pass_x(cur.data(), o.data(), h, w, rx, wx.data()); cur.swap(o); }
  return cur;
}

// the definition, without tiles: one line at a time, the mirror per tap
static std::vector<float> plain(const std::vector<float>& in, int h, int w, const std::vector<double>& wy, const std::vector<double>& wx) {
  std::vector<float> a(in), b(in.size());
  for (int axis = 0; axis < 2; ++axis) {
    const std::vector<double>& g = axis == 0 ? wy : wx;
    const int r = g.empty() ? 0 : static_cast<int>(g.size()) - 1;
    if (r == 0) continue;
    const int n = axis == 0 ? h : w, stride = axis == 0 ? w : 1;
    for (int y = 0; y < h; ++y)
      for (int x = 0; x < w; ++x) {
        const int i = axis == 0 ? y : x;
        const float* line = a.data() + (axis == 0 ? x : static_cast<long>(y) * w);
        double acc = gs_mul(static_cast<double>(line[static_cast<long>(i) * stride]), g[0]);
        for (int k = r; k >= 1; --k)
          acc = gs_add(acc, gs_mul(gs_add(static_cast<double>(line[static_cast<long>(mirror(i - k, n)) * stride]),
                                          static_cast<double>(line[static_cast<long>(mirror(i + k, n)) * stride])), g[k]));
        b[static_cast<long>(y) * w + x] = static_cast<float>(acc);
      }
    a.swap(b);
  }
  return a;
}

template <typename T>
static std::vector<T> read_file(const char* path) {
  std::FILE* f = std::fopen(path, "rb");
  if (!f) fail("cannot open an input file");
  std::vector<T> v;
  T x;
  while (std::fread(&x, sizeof(T), 1, f) == 1) v.push_back(x);
  std::fclose(f);
  return v;
}

static std::vector<double> table(int r) {      // a normalised table of radius r, centre first (any symmetric one serves the check)
  std::vector<double> g(r + 1);
  double sum = 0.0;
  for (int k = 0; k <= r; ++k) { g[k] = 1.0 / (1.0 + 0.37 * k * k); sum += (k ? 2.0 : 1.0) * g[k]; }
  for (double& v : g) v /= sum;
  return g;
}

int main(int argc, char** argv) {
  if (argc == 7) {
    const int h = std::atoi(argv[2]), w = std::atoi(argv[3]);
    const std::vector<float> in = read_file<float>(argv[1]);
    if (h < 2 || w < 2 || static_cast<long>(in.size()) != static_cast<long>(h) * w) fail("the input is not h * w floats", h, w);
    const std::vector<float> out = filter(in, h, w, read_file<double>(argv[4]), read_file<double>(argv[5]));
    std::FILE* f = std::fopen(argv[6], "wb");
    if (!f || std::fwrite(out.data(), sizeof(float), out.size(), f) != out.size()) fail("cannot write the output file");
    std::fclose(f);
    return 0;
  }
  if (argc != 1) fail("usage: postprocess_gauss_host_check [in.f32 h w wy.f64 wx.f64 out.f32]");
  const int shapes[][4] = {{2, 2, 64, 64}, {2, 300, 64, 1}, {6, 7, 10, 5}, {5, 200, 0, 18}, {70, 33, 5, 0}, {31, 127, 3, 64}, {32, 128, 64, 3},
                           {33, 129, 1, 1}, {65, 257, 17, 33}, {97, 64, 64, 0}, {3, 65, 0, 64}};
  unsigned s = 12345u;
  for (const auto& c : shapes) {
    const int h = c[0], w = c[1];
    std::vector<float> in(static_cast<size_t>(h) * w);
    for (float& v : in) { s = s * 1664525u + 1013904223u; v = static_cast<float>(s >> 24) / 255.0f; }
    const std::vector<double> wy = c[2] ? table(c[2]) : std::vector<double>(), wx = c[3] ? table(c[3]) : std::vector<double>();
    const std::vector<float> got = filter(in, h, w, wy, wx), want = plain(in, h, w, wy, wx);
    for (size_t i = 0; i < got.size(); ++i)
      if (got[i] != want[i]) fail("the tiled pass differs from the plain loop at element", static_cast<long>(i), h * 100000L + w);
    std::printf("%d x %d, radius (%d, %d): %zu samples equal the plain loop\n", h, w, c[2], c[3], got.size());
  }
  return 0;
}
