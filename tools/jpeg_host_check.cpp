// The JPEG export's arithmetic and buffer index arithmetic (diff_sal_amd/csrc/jpeg_core.h) run serially on the host, one loop
// iteration per device thread, into heap buffers of exactly the sizes the library's own layout and capacity functions return: built
// with a sanitizer, an access outside them stops the program.  No GPU and no HIP needed.
//   c++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all tools/jpeg_host_check.cpp -o jpeg_host_check
//   jpeg_host_check in.raw h w quality out.jpg out.raw      one image of h * w bytes -> the file and the read-back pixels
//   jpeg_host_check                                        self test: noise at several shapes and qualities, then forced
//                                                          coefficients that make every block's code as long as the tables allow
// No test runs this.  Its files for given inputs are Pillow's byte for byte where tests/_jpeg_ref.py's are (same arithmetic).
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <initializer_list>
#include <vector>

#include "../diff_sal_amd/csrc/jpeg_core.h"

using namespace diffsal::jpeg;

static constexpr HuffEnc kHuff = make_huff();

// `force`: skip the transform and code these 64 zig-zag coefficients for every block instead (to reach the longest codes)
static long encode(const unsigned char* in, int h, int w, int quality, unsigned char* out, long cap, unsigned char* recon, char* ws,
                   const short* force) {
  const Layout l = layout(1, h, w);
  const QTab q = quant_table(quality);
  const int bw = (w + 7) / 8;
  short* coef = reinterpret_cast<short*>(ws + l.coef);
  uint32_t* acbits = reinterpret_cast<uint32_t*>(ws + l.acbits);
  unsigned long long* bitoff = reinterpret_cast<unsigned long long*>(ws + l.bitoff);
  unsigned long long* total = reinterpret_cast<unsigned long long*>(ws + l.total);
  uint32_t* stream = reinterpret_cast<uint32_t*>(ws + l.stream);
  uint32_t* ffcount = reinterpret_cast<uint32_t*>(ws + l.ffcount);
  uint32_t* ffoff = reinterpret_cast<uint32_t*>(ws + l.ffoff);
  std::memset(stream, 0, static_cast<size_t>(l.words) * 4);
  for (long blk = 0; blk < l.nblk; ++blk) {      // block
    const int x0 = static_cast<int>(blk % bw) * 8, y0 = static_cast<int>(blk / bw) * 8;
    int d[64];
    for (int r = 0; r < 8; ++r) {
      const int y = y0 + r < h ? y0 + r : h - 1;
      for (int c = 0; c < 8; ++c) d[8 * r + c] = in[static_cast<long>(y) * w + (x0 + c < w ? x0 + c : w - 1)] - 128;
    }
    fdct_quantise(d, q);
    for (int k = 0; k < 64; ++k) coef[static_cast<long>(k) * l.nblk + blk] = force ? force[k] : static_cast<short>(d[kZigzag[k]]);
    uint32_t bits = 0;
    auto count = [&](uint32_t, int n) { bits += static_cast<uint32_t>(n); };
    put_ac([&](int k) { return static_cast<int>(coef[static_cast<long>(k) * l.nblk + blk]); }, kHuff.ac, count);
    acbits[blk] = bits;
    if (recon) {
      dequantise_idct(d, q);
      for (int r = 0; r < 8 && y0 + r < h; ++r)
        for (int c = 0; c < 8 && x0 + c < w; ++c) recon[static_cast<long>(y0 + r) * w + x0 + c] = static_cast<unsigned char>(d[8 * r + c]);
    }
  }
  unsigned long long carry = 0;      // offsets
  for (long blk = 0; blk < l.nblk; ++blk) {
    uint32_t bits = acbits[blk];
    auto count = [&](uint32_t, int n) { bits += static_cast<uint32_t>(n); };
    put_dc(coef[blk] - (blk ? coef[blk - 1] : 0), kHuff.dc, count);
    if (bits > static_cast<uint32_t>(kMaxBlockBits)) { std::fprintf(stderr, "block of %u bits\n", bits); std::exit(2); }
    bitoff[blk] = carry;
    carry += bits;
  }
  total[0] = carry;
  for (long blk = 0; blk < l.nblk; ++blk) {      // pack
    auto store = [&](long wi, uint32_t word) {
      if (word) stream[wi] |= word;      // no `wi < words` here: the sanitizer is the check
    };
    BitWriter<decltype(store)> bwr(store, bitoff[blk]);
    put_dc(coef[blk] - (blk ? coef[blk - 1] : 0), kHuff.dc, bwr);
    put_ac([&](int k) { return static_cast<int>(coef[static_cast<long>(k) * l.nblk + blk]); }, kHuff.ac, bwr);
    bwr.finish();
  }
  const long nbytes = static_cast<long>((total[0] + 7) >> 3);
  const long used = (nbytes + kStuffChunk - 1) / kStuffChunk;
  auto load = [&](long first, uint32_t* by, int& n) {      // stuff_load of the kernels
    n = 0;
    uint32_t ff = 0;
    if (first >= nbytes) return ff;
    const uint32_t w0 = stream[first >> 2], w1 = first + 4 < nbytes ? stream[(first >> 2) + 1] : 0u;
    for (int j = 0; j < kStuffBytes; ++j) {
      const long i = first + j;
      if (i < nbytes) { by[j] = scan_byte(j < 4 ? w0 : w1, i, nbytes, total[0]); ff += by[j] == 255u; n = j + 1; }
    }
    return ff;
  };
  uint32_t by[kStuffBytes];
  int n;
  for (long c = 0; c < used; ++c) {      // count
    uint32_t sum = 0;
    for (int t = 0; t < kThreads; ++t) sum += load(c * kStuffChunk + static_cast<long>(t) * kStuffBytes, by, n);
    ffcount[c] = sum;
  }
  uint32_t nff = 0;      // frame
  for (long c = 0; c < used; ++c) { ffoff[c] = nff; nff += ffcount[c]; }
  const Header hd = make_header(h, w, q);
  for (int k = 0; k < kHeaderBytes; ++k) out[k] = static_cast<unsigned char>((hd.w[k >> 2] >> (8 * (k & 3))) & 255u);
  const long end = kHeaderBytes + nbytes + nff;
  out[end] = 0xFF;
  out[end + 1] = 0xD9;
  for (long c = 0; c < used; ++c) {      // stuff
    uint32_t before = 0;
    for (int t = 0; t < kThreads; ++t) {
      const long first = c * kStuffChunk + static_cast<long>(t) * kStuffBytes;
      const uint32_t ff = load(first, by, n);
      unsigned char* o = out + kHeaderBytes + first + ffoff[c] + before;
      for (int j = 0; j < n; ++j) {
        *o++ = static_cast<unsigned char>(by[j]);
        if (by[j] == 255u) *o++ = 0;
      }
      before += ff;
    }
  }
  if (end + 2 > cap) { std::fprintf(stderr, "file of %ld bytes above cap %ld\n", end + 2, cap); std::exit(2); }
  return end + 2;
}

static long run(const unsigned char* in, int h, int w, int quality, std::vector<unsigned char>* file, std::vector<unsigned char>* rec,
                const short* force = nullptr) {
  const long cap = capacity(h, w);
  const Layout l = layout(1, h, w);
  unsigned char* out = static_cast<unsigned char*>(std::malloc(static_cast<size_t>(cap)));      // exact sizes: red zones behind them
  unsigned char* recon = static_cast<unsigned char*>(std::malloc(static_cast<size_t>(h) * w));
  char* ws = static_cast<char*>(std::malloc(l.bytes));
  const long len = encode(in, h, w, quality, out, cap, recon, ws, force);
  if (file) file->assign(out, out + len);
  if (rec) rec->assign(recon, recon + static_cast<size_t>(h) * w);
  std::free(out); std::free(recon); std::free(ws);
  return len;
}

int main(int argc, char** argv) {
  if (argc == 7) {
    const int h = std::atoi(argv[2]), w = std::atoi(argv[3]), quality = std::atoi(argv[4]);
    std::vector<unsigned char> in(static_cast<size_t>(h) * w), file, rec;
    FILE* f = std::fopen(argv[1], "rb");
    if (!f || std::fread(in.data(), 1, in.size(), f) != in.size()) { std::fprintf(stderr, "cannot read %s\n", argv[1]); return 1; }
    std::fclose(f);
    run(in.data(), h, w, quality, &file, &rec);
    f = std::fopen(argv[5], "wb"); std::fwrite(file.data(), 1, file.size(), f); std::fclose(f);
    f = std::fopen(argv[6], "wb"); std::fwrite(rec.data(), 1, rec.size(), f); std::fclose(f);
    return 0;
  }
  // self test: noise at several shapes and qualities, then every AC coefficient forced to category 10 (16-bit codes; 1023 has
  // all-ones value bits, so the scan is full of FF bytes to stuff): 63 * 26 + 2 of the 1658 bits a block may take
  unsigned s = 12345u;
  auto rnd = [&] { s = s * 1664525u + 1013904223u; return static_cast<unsigned char>(s >> 24); };
  const int shapes[][2] = {{1, 1}, {3, 17}, {8, 8}, {13, 21}, {64, 72}, {1, 4097}, {181, 183}, {224, 384}};
  for (auto& hw : shapes)
    for (int quality : {1, 30, 75, 95, 100}) {
      std::vector<unsigned char> in(static_cast<size_t>(hw[0]) * hw[1]);
      for (auto& v : in) v = quality == 30 ? (rnd() & 1 ? 255 : 0) : rnd();
      const long len = run(in.data(), hw[0], hw[1], quality, nullptr, nullptr);
      std::printf("%d x %d q %d: %ld of %ld bytes\n", hw[0], hw[1], quality, len, capacity(hw[0], hw[1]));
    }
  for (auto& hw : shapes) {
    std::vector<unsigned char> in(static_cast<size_t>(hw[0]) * hw[1], 0);
    for (short ac : {static_cast<short>(1023), static_cast<short>(-1023), static_cast<short>(-512)}) {
      short force[64];
      for (int k = 1; k < 64; ++k) force[k] = ac;
      force[0] = 0;
      const long len = run(in.data(), hw[0], hw[1], 95, nullptr, nullptr, force);
      std::printf("%d x %d forced %d: %ld of %ld bytes\n", hw[0], hw[1], ac, len, capacity(hw[0], hw[1]));
    }
  }
  std::printf("ok\n");
  return 0;
}
