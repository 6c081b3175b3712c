// The PNG decode's arithmetic and buffer index arithmetic (diff_sal_amd/csrc/png_decode_core.h) run serially on the host, one loop
// iteration per device lane, with buffers of exactly the sizes diffsal_png_decode_ws_bytes reports, so that a sanitizer sees every
// access the kernels of csrc/png_decode.hip would make:
//   c++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all tools/png_decode_host_check.cpp -o png_decode_host_check
//   png_decode_host_check RGB|L out.raw a.png [b.png ...]     files of one size, colour type and depth -> the pixels, [N][H][W][3] or
//                                                            [N][H][W]; prints "file i status s" per file
//   png_decode_host_check                                   self test: the embedded files (tools/png_decode_host_check_files.h)
//                                                            decode to Pillow's pixels (FNV-1a), then several thousand seeded damaged
//                                                            copies of them: truncation at every length, byte flips, zeroed ranges, a
//                                                            forged far distance, block type 3.  Every damaged copy must decode without
//                                                            a sanitizer report, and no loop may exceed its stated bound
// The chunk walk below is the host parser's (diff_sal_amd/png.py) in small: it refuses what that one refuses.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../diff_sal_amd/csrc/png_decode_core.h"
#include "png_decode_host_check_files.h"

using namespace diffsal::png;

struct Parsed {
  int H = 0, W = 0, ctype = 0, depth = 0;
  std::vector<uint8_t> stream;
  uint8_t pal[768] = {};
};
static uint32_t be32(const uint8_t* p) { return (uint32_t(p[0]) << 24) | (uint32_t(p[1]) << 16) | (uint32_t(p[2]) << 8) | p[3]; }

static bool parse(const std::vector<uint8_t>& a, Parsed& out) {
  static const uint8_t sig[8] = {0x89, 'P', 'N', 'G', '\r', '\n', 0x1a, '\n'};
  if (a.size() < 8 || memcmp(a.data(), sig, 8)) return false;
  bool head = false, plte = false;
  size_t at = 8;
  while (at < a.size()) {
    if (at + 8 > a.size()) return false;
    const size_t n = be32(&a[at]);
    if (at + 12 + n > a.size()) return false;
    const uint8_t* p = &a[at + 8];
    if (!memcmp(&a[at + 4], "IHDR", 4)) {
      if (head || n < 13) return false;
      head = true;
      const uint32_t W = be32(p), H = be32(p + 4);
      if (W < 1 || W > uint32_t(kMaxW) || H < 1 || H > uint32_t(kMaxH) || p[10] || p[11] || p[12]) return false;
      out.W = int(W); out.H = int(H); out.depth = p[8]; out.ctype = p[9];
    } else if (!head) {
      return false;
    } else if (!memcmp(&a[at + 4], "PLTE", 4)) {
      plte = true;
      memset(out.pal, 0, 768);
      memcpy(out.pal, p, (n < 768 ? n : 768) / 3 * 3);
    } else if (!memcmp(&a[at + 4], "IDAT", 4)) {
      out.stream.insert(out.stream.end(), p, p + n);
    } else if (!memcmp(&a[at + 4], "IEND", 4)) {
      break;
    }
    at += 12 + n;
  }
  if (!head || !geom_ok(1, out.H, out.W, out.ctype, out.depth) || (out.ctype == 3 && !plte) || out.stream.size() < 2) return false;
  const unsigned cmf = out.stream[0], flg = out.stream[1];
  return (cmf & 15) == 8 && (cmf >> 4) <= 7 && ((cmf << 8) | flg) % 31 == 0 && !(flg & 0x20);
}

static long g_max_ratio_num = 0;      // the worst (loop trips - 64) / stream bits seen, in thousandths: must stay at or below 1000

// What diffsal_png_decode launches, lane by lane.  Buffers are exact: the packed streams, the records, ws_bytes of workspace, out.
static bool decode(const std::vector<Parsed>& files, int mode_l, std::vector<uint8_t>& out, std::vector<int>& status) {
  const int N = int(files.size());
  const Parsed& f0 = files[0];
  for (const Parsed& f : files)
    if (f.H != f0.H || f.W != f0.W || f.ctype != f0.ctype || f.depth != f0.depth) return false;
  const Geom g = geom(N, f0.H, f0.W, f0.ctype, f0.depth);
  std::vector<FileDesc> desc(N);
  size_t nbytes = 0;
  for (int i = 0; i < N; ++i) {
    desc[i] = FileDesc{};
    desc[i].off = uint32_t(nbytes);
    desc[i].len = uint32_t(files[i].stream.size());
    memcpy(desc[i].pal, files[i].pal, 768);
    nbytes += (files[i].stream.size() + 15) & ~size_t(15);
  }
  uint32_t* words = static_cast<uint32_t*>(aligned_alloc(16, nbytes));      // exactly nbytes
  memset(words, 0, nbytes);
  for (int i = 0; i < N; ++i) memcpy(reinterpret_cast<uint8_t*>(words) + desc[i].off, files[i].stream.data(), files[i].stream.size());
  uint8_t* ws = static_cast<uint8_t*>(aligned_alloc(16, g.bytes));         // exactly ws_bytes, dirty
  memset(ws, 0xA5, g.bytes);
  const int C = mode_l ? 1 : 3;
  out.assign(size_t(N) * g.H * g.W * C, 0x5A);
  status.assign(N, -1);
  FileState* state = reinterpret_cast<FileState*>(ws + g.state);
  uint8_t* data = ws + g.data;
  bool ok = true;
  // launch 1: inflate, a wave per file
  InflateShared* s = new InflateShared;
  for (int f = 0; f < N; ++f) {
    memset(s, 0xEE, sizeof(*s));      // LDS is never clean
    Counters ctr{};
    inflate_file(*s, words, long(nbytes), desc[f].off, desc[f].len, g, data + long(f) * g.region, state + f, &ctr);
    // the stated bounds: a trip per symbol or stored byte, each consuming at least one of the stream's bits (the last may run past the
    // end and stops the decode); a copy per trip at most; the flushes from the geometry
    const long bits = 8L * long(files[f].stream.size());
    if (ctr.iterations > bits + 64 || ctr.copies > ctr.iterations || ctr.flushes > g.region / kFlush + 2) {
      fprintf(stderr, "file %d: %ld trips, %ld copies, %ld flushes for %ld bits and a region of %ld bytes\n", f, ctr.iterations, ctr.copies,
              ctr.flushes, bits, g.region);
      ok = false;
    }
    if (bits > 0 && (ctr.iterations - 64) * 1000 / bits > g_max_ratio_num) g_max_ratio_num = (ctr.iterations - 64) * 1000 / bits;
  }
  delete s;
  // launch 2: Adler-32, then the bands on the diagonal: the kernel's own body, a loop trip per lane
  UnfilterShared* u = new UnfilterShared;
  for (int f = 0; f < N; ++f) {
    memset(u, 0xEE, sizeof(*u));
    Counters ctr{};
    status[f] = unfilter_file(*u, g, desc[f].pal, data + long(f) * g.region, state[f], mode_l, out.data() + size_t(f) * g.H * g.W * C, &ctr);
    // the stated bounds: an Adler tile per 1024 bytes of the region, band_steps per band of 64 rows
    if (ctr.iterations > g.region / 1024 + 1 || ctr.copies != long((g.H + kLanes - 1) / kLanes) * band_steps(g)) {
      fprintf(stderr, "file %d: %ld Adler tiles, %ld band steps for %d rows of %d groups\n", f, ctr.iterations, ctr.copies, g.H, g.groups);
      ok = false;
    }
  }
  delete u;
  free(words);
  free(ws);
  return ok;
}

static uint32_t fnv(const uint8_t* p, size_t n) {
  uint32_t h = 0x811C9DC5u;
  for (size_t i = 0; i < n; ++i) h = (h ^ p[i]) * 0x01000193u;
  return h;
}
static std::vector<uint8_t> read_file(const char* path) {
  std::vector<uint8_t> a;
  FILE* f = fopen(path, "rb");
  if (!f) { fprintf(stderr, "cannot open %s\n", path); exit(2); }
  uint8_t buf[65536];
  size_t n;
  while ((n = fread(buf, 1, sizeof buf, f)) > 0) a.insert(a.end(), buf, buf + n);
  fclose(f);
  return a;
}
static int self_test() {
  int failures = 0;
  long damaged = 0, flagged = 0;
  uint64_t seed = 0x9E3779B97F4A7C15ull;
  auto rnd = [&]() { seed ^= seed << 13; seed ^= seed >> 7; seed ^= seed << 17; return seed; };
  for (const Embedded& e : kEmbedded) {
    const std::vector<uint8_t> file(e.data, e.data + e.size);
    Parsed p;
    if (!parse(file, p)) { fprintf(stderr, "%s: refused\n", e.name); ++failures; continue; }
    for (int mode_l = 0; mode_l < 2; ++mode_l) {
      std::vector<uint8_t> out;
      std::vector<int> status;
      // alone and as the second of three: the same pixels
      if (!decode({p}, mode_l, out, status) || status[0] != 0 || fnv(out.data(), out.size()) != (mode_l ? e.l : e.rgb)) {
        fprintf(stderr, "%s mode %d: status %d or other pixels than Pillow's\n", e.name, mode_l, status.empty() ? -1 : status[0]);
        ++failures;
      }
      std::vector<uint8_t> three;
      if (!decode({p, p, p}, mode_l, three, status) || memcmp(three.data() + out.size(), out.data(), out.size())) ++failures;
    }
    // damaged copies of the stream: every one must decode without a report; the status says what was seen
    auto run = [&](const std::vector<uint8_t>& stream) {
      Parsed q = p;
      q.stream = stream;
      if (q.stream.size() < 2) return;
      std::vector<uint8_t> out;
      std::vector<int> status;
      if (!decode({p, q}, 0, out, status)) ++failures;
      if (status[0] != 0) { fprintf(stderr, "%s: the intact neighbour of a damaged file has status %d\n", e.name, status[0]); ++failures; }
      ++damaged;
      if (status[1]) ++flagged;
    };
    const std::vector<uint8_t>& s = p.stream;
    for (size_t n = 2; n < s.size(); ++n) run(std::vector<uint8_t>(s.begin(), s.begin() + long(n)));      // truncation at every length
    const int flips = s.size() > 2000 ? 150 : 400;
    for (int k = 0; k < flips; ++k) {      // byte flips
      std::vector<uint8_t> d = s;
      d[2 + rnd() % (d.size() - 2)] ^= uint8_t(1u << (rnd() % 8));
      if (k % 3 == 0) d[2 + rnd() % (d.size() - 2)] = uint8_t(rnd());
      run(d);
    }
    for (int k = 0; k < 100; ++k) {      // zeroed ranges
      std::vector<uint8_t> d = s;
      const size_t lo = 2 + rnd() % (d.size() - 2), n = 1 + rnd() % 64;
      for (size_t i = lo; i < d.size() && i < lo + n; ++i) d[i] = 0;
      run(d);
    }
    for (int k = 0; k < 32; ++k) {      // a forged far distance / block type 3 at the stream's start, in front of random bytes
      std::vector<uint8_t> d = {s[0], s[1]};
      // fixed block: BFINAL 1, BTYPE 01, then k literals 0 (code 00110000) and a match of length 3 (0000001) at distance code 29
      // (11101, 13 extra bits all ones): distance 32768 with at most k bytes written
      std::vector<int> bits = {1, 1, 0};
      for (int i = 0; i < k; ++i) for (int b : {0, 0, 1, 1, 0, 0, 0, 0}) bits.push_back(b);
      for (int b : {0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 0, 1}) bits.push_back(b);
      for (int i = 0; i < 13; ++i) bits.push_back(1);
      while (bits.size() % 8) bits.push_back(0);
      for (size_t i = 0; i < bits.size(); i += 8) {
        uint8_t v = 0;
        for (int b = 0; b < 8; ++b) v |= uint8_t(bits[i + b] << b);
        d.push_back(v);
      }
      for (int i = 0; i < 40; ++i) d.push_back(uint8_t(rnd()));
      run(d);
      std::vector<uint8_t> t = {s[0], s[1], uint8_t(0x06 | (k << 3))};      // BFINAL 0, BTYPE 11
      for (int i = 0; i < 20; ++i) t.push_back(uint8_t(rnd()));
      run(t);
    }
  }
  printf("self test: %zu embedded files, %ld damaged copies (%ld flagged), worst trips per stream bit %ld / 1000, %d failures\n",
         sizeof(kEmbedded) / sizeof(kEmbedded[0]), damaged, flagged, g_max_ratio_num, failures);
  return failures ? 1 : 0;
}

int main(int argc, char** argv) {
  if (argc == 1) return self_test();
  if (argc < 4 || (strcmp(argv[1], "RGB") && strcmp(argv[1], "L"))) {
    fprintf(stderr, "usage: %s RGB|L out.raw a.png [b.png ...]   |   %s   (self test)\n", argv[0], argv[0]);
    return 2;
  }
  std::vector<Parsed> files;
  for (int i = 3; i < argc; ++i) {
    Parsed p;
    if (!parse(read_file(argv[i]), p)) { fprintf(stderr, "%s: refused by the parser\n", argv[i]); return 3; }
    files.push_back(p);
  }
  std::vector<uint8_t> out;
  std::vector<int> status;
  if (!decode(files, strcmp(argv[1], "L") == 0, out, status)) { fprintf(stderr, "files differ in geometry, or a loop exceeded its bound\n"); return 4; }
  for (size_t i = 0; i < status.size(); ++i) printf("file %zu status %d\n", i, status[i]);
  FILE* f = fopen(argv[2], "wb");
  if (!f || fwrite(out.data(), 1, out.size(), f) != out.size()) { fprintf(stderr, "cannot write %s\n", argv[2]); return 2; }
  fclose(f);
  return 0;
}
