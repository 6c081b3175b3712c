// The JPEG decode's arithmetic and buffer index arithmetic (diff_sal_amd/csrc/jpeg_decode_core.h) run serially on the host, one
// loop iteration per device lane, into heap buffers of exactly the sizes the library's own layout reports: built with a sanitizer,
// an access outside them, or an operation the language leaves undefined, stops the program.  No GPU and no HIP needed.
//   c++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all tools/jpeg_decode_host_check.cpp -o jpeg_decode_host_check
//   jpeg_decode_host_check RGB|L out.raw a.jpg [b.jpg ...]      files of one size and sampling -> the pixels, [N][H][W][3] or [N][H][W];
//                                                             prints each file's status
//   jpeg_decode_host_check                                    self test: the embedded files (written by Pillow) decode to Pillow's pixels
//                                                             (by hash), alone and in one batch; then several thousand damaged copies
// The damage comes from a seeded generator: truncation at every length, byte flips anywhere in the file, zeroed ranges inside the
// scan, a scan of FF only.  A copy the marker walk refuses counts as rejected (the Python parser refuses before any launch); every
// other copy is decoded next to an intact file, which must keep its pixels.  Where a truncated or FF-filled copy decodes to other
// pixels its status must be non-zero.  A flipped or zeroed byte can leave a stream every decoder accepts (a changed value bit, a
// changed table entry): those copies are counted and printed, and must only leave every buffer alone.
// No test runs this.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../diff_sal_amd/csrc/jpeg_decode_core.h"

using namespace diffsal::jpeg;
typedef std::vector<unsigned char> Bytes;

struct Parsed {
  FileDesc d;
  std::vector<Segment> segs;
  int H, W, ncomp, hs, vs;
};

// the marker walk of diff_sal_amd/jpeg.py, as far as the tool needs it; `base`: where the file starts in the packed buffer
static bool parse(const Bytes& f, long base, Parsed& p, std::string& why) {
  std::memset(&p.d, 0, sizeof(p.d));
  p.segs.clear();
  const long n = static_cast<long>(f.size());
  bool have_q[4] = {}, have_h[4] = {}, sof = false;
  auto fail = [&](const char* w) { why = w; return false; };
  if (n < 4 || f[0] != 0xFF || f[1] != 0xD8) return fail("no SOI");
  long i = 2;
  for (;;) {
    if (i + 4 > n) return fail("ends inside a marker segment");
    if (f[i] != 0xFF) return fail("no marker");
    while (i + 1 < n && f[i + 1] == 0xFF) ++i;
    if (i + 4 > n) return fail("ends inside a marker segment");
    const int m = f[i + 1];
    const long len = (f[i + 2] << 8) | f[i + 3], at = i + 4, stop = i + 2 + len;
    if (len < 2 || stop > n) return fail("ends inside a marker segment");
    if (m == 0xDB) {
      for (long k = at; k < stop;) {
        if (f[k] >> 4) return fail("16-bit DQT");
        const int id = f[k] & 15;
        if (id > 3 || k + 65 > stop) return fail("bad DQT");
        for (int z = 0; z < 64; ++z) p.d.qt[id][kZigzag[z]] = f[k + 1 + z];
        have_q[id] = true;
        k += 65;
      }
    } else if (m == 0xC4) {
      for (long k = at; k < stop;) {
        const int cls = f[k] >> 4, id = f[k] & 15;
        if (cls > 1 || id > 1 || k + 17 > stop) return fail("bad DHT");
        int total = 0;
        for (int z = 0; z < 16; ++z) total += f[k + 1 + z];
        if (total > 256 || k + 17 + total > stop) return fail("bad DHT");
        std::memcpy(p.d.hbits[2 * cls + id], &f[k + 1], 16);
        std::memset(p.d.hvals[2 * cls + id], 0, 256);
        std::memcpy(p.d.hvals[2 * cls + id], &f[k + 17], static_cast<size_t>(total));
        have_h[2 * cls + id] = true;
        k += 17 + total;
      }
    } else if (m == 0xC0) {
      if (sof || len < 8) return fail("bad SOF");
      if (f[at] != 8) return fail("precision");
      p.H = (f[at + 1] << 8) | f[at + 2];
      p.W = (f[at + 3] << 8) | f[at + 4];
      p.ncomp = f[at + 5];
      if ((p.ncomp != 1 && p.ncomp != 3) || len != 8 + 3 * p.ncomp || p.H == 0 || p.W == 0) return fail("components or size");
      for (int c = 0; c < p.ncomp; ++c) {
        const int hv = f[at + 7 + 3 * c], tq = f[at + 8 + 3 * c];
        if (tq > 3) return fail("table selector");
        p.d.comp[c][0] = static_cast<uint8_t>(tq);
        if (c == 0) { p.hs = hv >> 4; p.vs = hv & 15; } else if (hv != 0x11) return fail("sampling");
      }
      if (p.ncomp == 1) p.hs = p.vs = 1;      // a single component is not interleaved: its factors do not matter
      if (!geom_ok(1, p.H, p.W, p.ncomp, p.hs, p.vs)) return fail("sampling");
      sof = true;
    } else if ((m >= 0xC1 && m <= 0xCF && m != 0xC4 && m != 0xC8) || m == 0xDC) {
      return fail("not baseline");
    } else if (m == 0xDD) {
      if (len != 4) return fail("bad DRI");
      p.d.restart = static_cast<uint32_t>((f[at] << 8) | f[at + 1]);
    } else if (m == 0xDA) {
      if (!sof || len != 6 + 2 * p.ncomp || f[at] != p.ncomp) return fail("scan");
      for (int c = 0; c < p.ncomp; ++c) {
        const int t = f[at + 2 + 2 * c];
        if ((t >> 4) > 1 || (t & 15) > 1) return fail("table selector");
        p.d.comp[c][1] = static_cast<uint8_t>(t >> 4);
        p.d.comp[c][2] = static_cast<uint8_t>(t & 15);
        if (!have_q[p.d.comp[c][0]] || !have_h[t >> 4] || !have_h[2 + (t & 15)]) return fail("missing table");
      }
      i = stop;
      break;
    }
    i = stop;
  }
  // the scan: up to the first marker that is no RSTn; a segment per restart interval
  const Geom g = geom(1, p.H, p.W, p.ncomp, p.hs, p.vs);
  long seg = i, k = i, end = n;
  int first = 0;
  auto close = [&](long stop) {
    long e = stop;
    while (e > seg && f[e - 1] == 0xFF) --e;      // fill bytes in front of the marker
    p.segs.push_back(Segment{0, static_cast<int32_t>(base + seg), static_cast<int32_t>(base + e), first});
  };
  for (; k + 1 < n; ++k) {
    if (f[k] != 0xFF || f[k + 1] == 0 || f[k + 1] == 0xFF) continue;
    if (f[k + 1] >= 0xD0 && f[k + 1] <= 0xD7) {
      close(k);
      first += static_cast<int>(p.d.restart);
      seg = k + 2;
      ++k;
      continue;
    }
    end = k;
    break;
  }
  close(end);
  const long want = p.d.restart ? (g.mcus + p.d.restart - 1) / p.d.restart : 1;
  if (static_cast<long>(p.segs.size()) != want) return fail("segment count");
  p.d.scan_off = static_cast<uint32_t>(base + i);
  p.d.scan_len = static_cast<uint32_t>(end - i);
  return true;
}

// files of one geometry -> pixels and status; false: a file was refused (why) or differs from the first in geometry
static bool decode(const std::vector<Bytes>& files, bool mode_l, Bytes& pixels, std::vector<int>& status, std::string& why) {
  const int N = static_cast<int>(files.size());
  std::vector<Parsed> ps(N);
  std::vector<Segment> segs;
  long total = 0;
  for (int f = 0; f < N; ++f) {
    if (!parse(files[f], total, ps[f], why)) return false;
    if (ps[f].H != ps[0].H || ps[f].W != ps[0].W || ps[f].ncomp != ps[0].ncomp || ps[f].hs != ps[0].hs || ps[f].vs != ps[0].vs) {
      why = "files differ in size or sampling";
      return false;
    }
    ps[f].d.seg0 = static_cast<uint32_t>(segs.size());
    ps[f].d.nseg = static_cast<uint32_t>(ps[f].segs.size());
    for (Segment s : ps[f].segs) { s.file = f; segs.push_back(s); }
    total += static_cast<long>(files[f].size());
  }
  const long nbytes = (total + 15) & ~15L;
  const Geom g = geom(N, ps[0].H, ps[0].W, ps[0].ncomp, ps[0].hs, ps[0].vs);
  const int C = mode_l ? 1 : 3, nseg = static_cast<int>(segs.size());
  // exact sizes: red zones behind them
  unsigned char* packed = static_cast<unsigned char*>(std::calloc(static_cast<size_t>(nbytes), 1));
  char* ws = static_cast<char*>(std::malloc(g.bytes));
  unsigned char* out = static_cast<unsigned char*>(std::malloc(static_cast<size_t>(N) * g.H * g.W * C));
  FileDesc* desc = static_cast<FileDesc*>(std::malloc(sizeof(FileDesc) * N));
  Segment* seg = static_cast<Segment*>(std::malloc(sizeof(Segment) * nseg));
  long at = 0;
  for (int f = 0; f < N; ++f) {
    std::memcpy(packed + at, files[f].data(), files[f].size());
    at += static_cast<long>(files[f].size());
    desc[f] = ps[f].d;
  }
  std::memcpy(seg, segs.data(), sizeof(Segment) * nseg);
  std::memset(ws + g.planes, 0xCD, g.bytes - g.planes);
  std::memset(ws, 0, g.clear);      // the call's hipMemsetAsync
  int* st = reinterpret_cast<int*>(ws + g.status);
  int16_t* coef = reinterpret_cast<int16_t*>(ws + g.coef);
  unsigned char* planes = reinterpret_cast<unsigned char*>(ws + g.planes);
  HuffDec* tabs = static_cast<HuffDec*>(std::malloc(sizeof(HuffDec) * 4));
  for (int f = 0; f < N; ++f) {      // entropy: a workgroup per file builds the tables, a lane per segment
    for (int t = 0; t < 4; ++t) build_huff(tabs[t], desc[f].hbits[t], desc[f].hvals[t]);
    int lo, n;
    file_segments(desc[f], nseg, lo, n);
    for (int s = lo; s < lo + n; ++s) {
      long begin, end;
      int first, n_mcu;
      if (!segment_work(g, seg[s], desc[f].restart, nbytes, begin, end, first, n_mcu)) continue;
      BitReader br(reinterpret_cast<const uint32_t*>(packed), begin, end);
      int16_t* cf = coef + static_cast<long>(f) * g.nblk * 64;
      auto store = [&](long blk, int k, int16_t v) { cf[blk * 64 + k] = v; };
      st[f] |= decode_segment(g, tabs, desc[f].comp, kZigzag, br, first, n_mcu, store);
    }
  }
  for (int f = 0; f < N; ++f)      // transform: a lane per block
    for (long blk = 0; blk < g.nblk; ++blk) {
      const int c = g.ncomp == 3 && blk >= g.boff[2] ? 2 : g.ncomp == 3 && blk >= g.boff[1] ? 1 : 0;
      QTab q;
      for (int k = 0; k < 64; ++k) q.t[k] = desc[f].qt[desc[f].comp[c][0] & 3][k];
      uint32_t d[64];
      block_samples(coef + (static_cast<long>(f) * g.nblk + blk) * 64, q, d);
      const long b = blk - g.boff[c], stride = 8L * g.bw[c];
      unsigned char* o = planes + static_cast<long>(f) * g.plane + g.poff[c] + (b / g.bw[c]) * 8 * stride + (b % g.bw[c]) * 8;
      for (int r = 0; r < 8; ++r)
        for (int x = 0; x < 8; ++x) o[r * stride + x] = static_cast<unsigned char>(d[8 * r + x]);
    }
  const int groups = (g.W + kRowPixels - 1) / kRowPixels;
  for (int f = 0; f < N; ++f)      // colour: a lane per 16 pixels of a row
    for (long t = 0; t < static_cast<long>(groups) * g.H; ++t) {
      const int y = static_cast<int>(t / groups), x0 = static_cast<int>(t % groups) * kRowPixels;
      for (int x = x0; x < x0 + kRowPixels && x < g.W; ++x) {
        int rgb[3];
        pixel_rgb(g, planes + static_cast<long>(f) * g.plane, x, y, rgb);
        unsigned char* o = out + ((static_cast<long>(f) * g.H + y) * g.W + x) * C;
        if (mode_l) o[0] = static_cast<unsigned char>(g.ncomp == 1 ? rgb[0] : rgb_l(rgb[0], rgb[1], rgb[2]));
        else for (int k = 0; k < 3; ++k) o[k] = static_cast<unsigned char>(rgb[k]);
      }
    }
  pixels.assign(out, out + static_cast<size_t>(N) * g.H * g.W * C);
  status.assign(st, st + N);
  std::free(packed); std::free(ws); std::free(out); std::free(desc); std::free(seg); std::free(tabs);
  return true;
}

static const unsigned char kFileA[] = {      // 13 x 17, 4:2:0, quality 75, optimised tables
    255,216,255,224,0,16,74,70,73,70,0,1,1,0,0,1,0,1,0,0,255,219,0,67,0,8,6,6,7,6,5,8,
    7,7,7,9,9,8,10,12,20,13,12,11,11,12,25,18,19,15,20,29,26,31,30,29,26,28,28,32,36,46,39,32,
    34,44,35,28,28,40,55,41,44,48,49,52,52,52,31,39,57,61,56,50,60,46,51,52,50,255,219,0,67,1,9,9,
    9,12,11,12,24,13,13,24,50,33,28,33,50,50,50,50,50,50,50,50,50,50,50,50,50,50,50,50,50,50,50,50,
    50,50,50,50,50,50,50,50,50,50,50,50,50,50,50,50,50,50,50,50,50,50,50,50,50,50,50,50,50,50,255,192,
    0,17,8,0,13,0,17,3,1,34,0,2,17,1,3,17,1,255,196,0,23,0,0,3,1,0,0,0,0,0,0,0,
    0,0,0,0,0,0,0,4,5,6,255,196,0,39,16,0,1,4,1,2,3,9,0,0,0,0,0,0,0,0,0,1,
    0,2,3,4,17,6,20,5,18,33,19,21,49,82,97,98,193,209,240,255,196,0,21,1,1,1,0,0,0,0,0,0,
    0,0,0,0,0,0,0,0,1,3,255,196,0,32,17,0,0,4,6,3,0,0,0,0,0,0,0,0,0,0,0,0,
    1,2,4,3,17,18,20,33,65,21,81,82,255,218,0,12,3,1,0,2,17,3,17,0,63,0,71,134,234,171,18,90,
    21,109,130,3,186,14,101,161,183,166,42,92,169,184,141,205,115,128,36,128,51,213,45,197,244,237,56,33,221,70,11,100,
    13,207,135,169,80,168,234,43,140,155,176,46,46,102,113,140,251,115,242,131,141,51,180,107,130,217,133,21,62,58,149,136,
    105,208,107,185,164,242,192,133,119,117,39,231,31,180,43,112,139,246,41,38,29,15,255,217,};
static const unsigned char kFileB[] = {      // 5 x 9, one component, quality 90, optimised tables
    255,216,255,224,0,16,74,70,73,70,0,1,1,0,0,1,0,1,0,0,255,219,0,67,0,3,2,2,3,2,2,3,
    3,3,3,4,3,3,4,5,8,5,5,4,4,5,10,7,7,6,8,12,10,12,12,11,10,11,11,13,14,18,16,13,
    14,17,14,11,11,16,22,16,17,19,20,21,21,21,12,15,23,24,22,20,24,18,20,21,20,255,192,0,11,8,0,5,
    0,9,1,1,17,0,255,196,0,20,0,1,0,0,0,0,0,0,0,0,0,0,0,0,0,0,0,6,255,196,0,33,
    16,0,2,1,3,3,5,0,0,0,0,0,0,0,0,0,0,1,2,3,5,17,33,0,4,6,7,22,34,83,145,255,
    218,0,8,1,1,0,0,63,0,123,64,235,149,87,141,108,98,163,109,224,47,19,132,133,100,105,200,40,24,70,48,0,
    24,242,205,173,123,12,232,191,119,212,189,139,243,95,255,217,};
static const unsigned char kFileC[] = {      // 10 x 24, 4:2:2, quality 50, optimised tables, a restart marker behind every MCU
    255,216,255,224,0,16,74,70,73,70,0,1,1,0,0,1,0,1,0,0,255,219,0,67,0,16,11,12,14,12,10,16,
    14,13,14,18,17,16,19,24,40,26,24,22,22,24,49,35,37,29,40,58,51,61,60,57,51,56,55,64,72,92,78,64,
    68,87,69,55,56,80,109,81,87,95,98,103,104,103,62,77,113,121,112,100,120,92,101,103,99,255,219,0,67,1,17,18,
    18,24,21,24,47,26,26,47,99,66,56,66,99,99,99,99,99,99,99,99,99,99,99,99,99,99,99,99,99,99,99,99,
    99,99,99,99,99,99,99,99,99,99,99,99,99,99,99,99,99,99,99,99,99,99,99,99,99,99,99,99,99,99,255,192,
    0,17,8,0,10,0,24,3,1,33,0,2,17,1,3,17,1,255,196,0,24,0,0,3,1,1,0,0,0,0,0,0,
    0,0,0,0,0,0,0,4,5,2,3,255,196,0,33,16,0,1,3,3,4,3,0,0,0,0,0,0,0,0,0,0,
    1,0,2,3,4,17,33,5,19,49,65,18,113,145,255,196,0,24,1,0,2,3,0,0,0,0,0,0,0,0,0,0,
    0,0,0,2,4,0,1,3,255,196,0,29,17,0,2,2,2,3,1,0,0,0,0,0,0,0,0,0,0,1,2,0,
    3,4,51,17,18,65,33,255,221,0,4,0,1,255,218,0,12,3,1,0,2,17,3,17,0,63,0,225,73,170,200,231,
    152,165,192,225,81,151,75,138,104,183,153,107,145,218,38,34,138,186,250,100,200,110,236,42,73,255,208,76,215,207,67,40,
    96,242,13,225,8,169,199,5,57,111,102,229,210,128,16,207,255,209,74,118,180,84,224,1,147,210,169,64,231,22,184,18,
    72,199,106,178,54,136,56,219,76,255,210,206,162,214,238,94,195,231,164,38,108,249,196,79,43,97,159,255,217,};
// FNV-1a of the pixels Pillow 12.2 (libjpeg-turbo) reads from them: convert("RGB"), convert("L")
struct Embedded { const char* name; const unsigned char* data; size_t size; uint32_t rgb, l; };
static const Embedded kEmbedded[] = {{"a 13x17 4:2:0", kFileA, sizeof(kFileA), 0xd7048512u, 0x9619c484u},
                                     {"b 5x9 grey", kFileB, sizeof(kFileB), 0xf987260bu, 0x89bc0443u},
                                     {"c 10x24 4:2:2 restarts", kFileC, sizeof(kFileC), 0x81d827e4u, 0xb2010a86u}};

static uint32_t fnv(const Bytes& b) {
  uint32_t h = 0x811c9dc5u;
  for (unsigned char x : b) h = (h ^ x) * 0x01000193u;
  return h;
}

static long scan_start(const Bytes& f) {      // behind the SOS header
  for (size_t i = 2; i + 3 < f.size(); ++i)
    if (f[i] == 0xFF && f[i + 1] == 0xDA) return static_cast<long>(i) + 2 + ((f[i + 2] << 8) | f[i + 3]);
  return static_cast<long>(f.size());
}

int main(int argc, char** argv) {
  std::string why;
  if (argc >= 4) {
    const bool mode_l = std::strcmp(argv[1], "L") == 0;
    std::vector<Bytes> files;
    for (int a = 3; a < argc; ++a) {
      FILE* f = std::fopen(argv[a], "rb");
      if (!f) { std::fprintf(stderr, "cannot read %s\n", argv[a]); return 1; }
      Bytes b;
      unsigned char buf[4096];
      for (size_t n; (n = std::fread(buf, 1, sizeof(buf), f)) > 0;) b.insert(b.end(), buf, buf + n);
      std::fclose(f);
      files.push_back(b);
    }
    Bytes px;
    std::vector<int> st;
    if (!decode(files, mode_l, px, st, why)) { std::fprintf(stderr, "refused: %s\n", why.c_str()); return 1; }
    for (size_t f = 0; f < st.size(); ++f) std::printf("%s status %d\n", argv[3 + f], st[f]);
    FILE* o = std::fopen(argv[2], "wb");
    if (!o || std::fwrite(px.data(), 1, px.size(), o) != px.size()) { std::fprintf(stderr, "cannot write %s\n", argv[2]); return 1; }
    std::fclose(o);
    return 0;
  }
  unsigned s = 20240901u;
  auto rnd = [&] { s = s * 1664525u + 1013904223u; return s >> 8; };
  long copies = 0, rejected = 0, flagged = 0, same = 0, silent = 0;
  for (const Embedded& e : kEmbedded) {
    const Bytes good(e.data, e.data + e.size);
    Bytes want[2];
    std::vector<int> st;
    for (int l = 0; l < 2; ++l) {
      if (!decode({good}, l == 1, want[l], st, why) || st[0] != 0) { std::fprintf(stderr, "%s: refused or status: %s\n", e.name, why.c_str()); return 2; }
      if (fnv(want[l]) != (l ? e.l : e.rgb)) { std::fprintf(stderr, "%s: pixels are not Pillow's (mode %s)\n", e.name, l ? "L" : "RGB"); return 2; }
    }
    std::printf("%s: %zu bytes, Pillow's pixels in both modes\n", e.name, e.size);
    const long scan = scan_start(good);
    // bad: one damaged copy next to the intact file.  strict: other pixels need a non-zero status
    auto trial = [&](const Bytes& bad, bool strict, const char* what) {
      ++copies;
      Bytes px;
      std::vector<int> st2;
      const bool mode_l = (copies & 1) != 0;
      if (!decode({good, bad, good}, mode_l, px, st2, why)) { ++rejected; return; }
      const Bytes& w = want[mode_l ? 1 : 0];
      const size_t n = w.size();
      if (st2[0] != 0 || st2[2] != 0 || std::memcmp(px.data(), w.data(), n) != 0 || std::memcmp(px.data() + 2 * n, w.data(), n) != 0) {
        std::fprintf(stderr, "%s: %s: the intact files of the batch changed\n", e.name, what);
        std::exit(2);
      }
      const bool differs = std::memcmp(px.data() + n, w.data(), n) != 0;
      if (st2[1]) ++flagged;
      else if (!differs) ++same;
      else if (strict) { std::fprintf(stderr, "%s: %s: other pixels with status 0\n", e.name, what); std::exit(2); }
      else ++silent;
    };
    for (size_t cut = 0; cut < good.size(); ++cut) trial(Bytes(good.begin(), good.begin() + static_cast<long>(cut)), true, "truncation");
    {
      Bytes bad(good);
      for (size_t i = static_cast<size_t>(scan); i < bad.size(); ++i) bad[i] = 0xFF;
      trial(bad, true, "FF fill");
      bad.assign(good.begin(), good.end());
      for (size_t i = static_cast<size_t>(scan); i + 2 < bad.size(); ++i) bad[i] = 0xFF;      // the EOI kept
      trial(bad, true, "FF fill in front of EOI");
    }
    for (int t = 0; t < 1500; ++t) {      // flips anywhere: tables, sizes, selectors, scan
      Bytes bad(good);
      const int n = 1 + static_cast<int>(rnd() % 3);
      for (int k = 0; k < n; ++k) bad[rnd() % bad.size()] ^= static_cast<unsigned char>(1u << (rnd() % 8));
      trial(bad, false, "flip");
    }
    for (int t = 0; t < 500; ++t) {      // whole bytes replaced inside the scan
      Bytes bad(good);
      bad[static_cast<size_t>(scan) + rnd() % (bad.size() - static_cast<size_t>(scan))] = static_cast<unsigned char>(rnd());
      trial(bad, false, "byte");
    }
    for (int t = 0; t < 500; ++t) {      // zeroed ranges inside the scan
      Bytes bad(good);
      const size_t span = bad.size() - 2 - static_cast<size_t>(scan), a = rnd() % span, len = 1 + rnd() % (span - a);
      std::memset(&bad[static_cast<size_t>(scan) + a], 0, len);
      trial(bad, false, "zeroed range");
    }
  }
  std::printf("%ld damaged copies: %ld refused by the marker walk, %ld decoded with a non-zero status, %ld to the same pixels, "
              "%ld to other pixels with status 0 (flips, bytes and zeroed ranges only)\nok\n", copies, rejected, flagged, same, silent);
  return 0;
}
