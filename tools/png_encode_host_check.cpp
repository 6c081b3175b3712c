// The PNG export's arithmetic and buffer index arithmetic (diff_sal_amd/csrc/png_encode_core.h) run serially on the host, one loop
// trip per device thread, into heap buffers of exactly the sizes the library's own capacity and layout functions return (filled
// with A5 first): built with a sanitizer, an access outside them stops the program.  No GPU and no HIP needed.
//   c++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all tools/png_encode_host_check.cpp -o png_encode_host_check
//   png_encode_host_check in.raw H W out.png      one map of H * W bytes -> its file
//   png_encode_host_check                         self test: edge shapes and contents, then a forced worst case per shape (every
//                                                 code 15 bits long, every header 4092 bits) that fills the capacity bound to
//                                                 the bit.  Checked without an inflate: chunk layout and CRC-32s, Adler-32
//                                                 against a plain loop, the length, no write past a bound
// No test runs this.  Its files are tests/_png_encode_ref.py's byte for byte (tools/gen_png_encode_golden.py --host-check compares).
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../diff_sal_amd/csrc/png_encode_core.h"

using namespace diffsal::pnge;

static constexpr CrcTables kCrc = make_crc_tables();

[[noreturn]] static void fail(const char* what, long a = 0, long b = 0) {
  std::fprintf(stderr, "png_encode_host_check: %s (%ld, %ld)\n", what, a, b);
  std::exit(2);
}

// `force`: every stream byte a literal, every literal/length code 15 bits long and the header 4092 bits of ones: not a decodable
// block, the longest one
static long encode(const uint8_t* in, int H, int W, uint8_t* out, long cap, char* ws, bool force) {
  const Layout l = layout(1, H, W);
  uint8_t* filt = reinterpret_cast<uint8_t*>(ws + l.filt);
  uint16_t* tok = reinterpret_cast<uint16_t*>(ws + l.tok);
  uint32_t* chunkoff = reinterpret_cast<uint32_t*>(ws + l.chunkoff);
  uint32_t* code = reinterpret_cast<uint32_t*>(ws + l.code);
  uint32_t* header = reinterpret_cast<uint32_t*>(ws + l.header);
  SegInfo* info = reinterpret_cast<SegInfo*>(ws + l.info);
  unsigned long long* segoff = reinterpret_cast<unsigned long long*>(ws + l.segoff);
  unsigned long long* bits = reinterpret_cast<unsigned long long*>(ws + l.bits);
  std::memset(out, 0, static_cast<size_t>(cap));      // clear
  for (int row = 0; row < H; ++row) {                 // filter
    const uint8_t* rp = in + static_cast<long>(row) * W;
    const uint8_t* up = row ? rp - W : nullptr;
    uint32_t cost[5] = {0, 0, 0, 0, 0};
    for (int lane = 0; lane < kRowLanes; ++lane)
      for (int x = lane; x < W; x += kRowLanes) {
        int v, a, b, c;
        neighbours(rp, up, x, v, a, b, c);
        for (int f = 0; f < 5; ++f) cost[f] += filter_cost(filter_byte(f, v, a, b, c));
      }
    const int f = choose_filter(cost);
    uint8_t* o = filt + static_cast<long>(row) * (W + 1);
    o[0] = static_cast<uint8_t>(f);
    for (int lane = 0; lane < kRowLanes; ++lane)
      for (int x = lane; x < W; x += kRowLanes) {
        int v, a, b, c;
        neighbours(rp, up, x, v, a, b, c);
        o[1 + x] = static_cast<uint8_t>(filter_byte(f, v, a, b, c));
      }
  }
  std::vector<BlockShared> shared(1);
  std::vector<ChunkRegs> regs(kThreads);
  BlockShared& s = shared[0];
  for (long seg = 0; seg < l.nseg; ++seg) {      // segment
    const long at = seg * kSegment;
    const int n = static_cast<int>(l.S - at < kSegment ? l.S - at : kSegment);
    for (int t = 0; t < kThreads; ++t) load_chunk(filt + at, at, n, t, regs[t]);
    for (int i = 0; i < 288; ++i) s.hist[i] = i == 256 ? 1u : 0u;
    s.nonzero = 0; s.m = 0; s.adler_a = 0; s.adler_b = 0;
    for (int t = 0; t < kThreads; ++t) s.ne_last[t] = t && s.ne_last[t - 1] > regs[t].last_ne ? s.ne_last[t - 1] : regs[t].last_ne;
    for (int t = kThreads - 1; t >= 0; --t)
      s.ne_first[t] = t + 1 < kThreads && s.ne_first[t + 1] < regs[t].first_ne ? s.ne_first[t + 1] : regs[t].first_ne;
    for (int t = 0; t < kThreads; ++t) {
      const ChunkRegs& r = regs[t];
      const int before = t ? s.ne_last[t - 1] : -1, after = t + 1 < kThreads ? s.ne_first[t + 1] : n;
      uint32_t* tk = reinterpret_cast<uint32_t*>(tok + at) + t * (kChunk / 2);
      if (!r.nv) continue;
      for (int j = 0; j < kChunk; j += 2) {
        uint32_t pair = 0;
        for (int k = 0; k < 2; ++k) {
          uint32_t tv = j + k < r.nv ? token_at(r, j + k, before, after) : kNone;
          if (force && j + k < r.nv) tv = (r.w[(j + k) >> 2] >> (8 * ((j + k) & 3))) & 255u;
          if (tv != kNone) {
            int eb, ev;
            ++s.hist[token_symbol(tv, eb, ev)];
          }
          pair |= tv << (16 * k);
        }
        tk[j >> 1] = pair;
      }
      s.adler_a += r.s1;
      s.adler_b += r.s2 % kAdlerMod;
    }
    for (int i = 0; i < kLit; ++i) s.nonzero += s.hist[i] > 0;
    for (int i = 0; i < kLit; ++i)
      if (takes_part(s.hist, static_cast<int>(s.nonzero), i)) {
        s.cs.order[rank_of(s.hist, kLit, static_cast<int>(s.nonzero), i)] = static_cast<uint16_t>(i);
        ++s.m;
      }
    build_block(s, seg == l.nseg - 1);
    if (s.header_bits > static_cast<uint32_t>(kMaxHeaderBits)) fail("a header above its bound", s.header_bits);
    uint32_t kraft = 0;
    for (int i = 0; i < kLit; ++i) {
      if ((s.hist[i] > 0) != (s.lens[i] > 0) || s.lens[i] > 15) fail("a literal/length code length", i, s.lens[i]);
      if (s.lens[i]) kraft += 1u << (15 - s.lens[i]);
    }
    if (kraft != 1u << 15) fail("the literal/length code is not complete", kraft);
    kraft = 0;
    for (int i = 0; i < kClen; ++i) {
      if (s.clens[i] > 7) fail("a code-length code length", i, s.clens[i]);
      if (s.clens[i]) kraft += 1u << (7 - s.clens[i]);
    }
    if (kraft != 1u << 7) fail("the code-length code is not complete", kraft);
    if (force) {
      for (int i = 0; i < kLit; ++i) s.code[i] = (0x7FFFu << 4) | 15u;
      for (int i = 0; i < kHeaderWords; ++i) s.header[i] = 0xFFFFFFFFu;
      s.header[kHeaderWords - 1] = 0x0FFFFFFFu;
      s.header_bits = kMaxHeaderBits;
    }
    for (int i = 0; i < 288; ++i) code[seg * 288 + i] = i < kLit ? s.code[i] : 0u;
    for (int t = 0; t < kHeaderWords; ++t) header[seg * kHeaderWords + t] = s.header[t];
    uint32_t sum = 0;
    for (int t = 0; t < kThreads; ++t) {
      const uint32_t* tk = reinterpret_cast<const uint32_t*>(tok + at) + t * (kChunk / 2);
      uint32_t mine = 0;
      for (int j = 0; j < regs[t].nv; ++j) {
        const uint32_t tv = (tk[j >> 1] >> (16 * (j & 1))) & 0xFFFFu;
        if (tv != kNone) mine += token_bits(tv, s.code);
      }
      chunkoff[seg * kThreads + t] = s.header_bits + sum;
      sum += mine;
    }
    info[seg] = SegInfo{s.header_bits, s.header_bits + sum + (s.code[256] & 15u), s.adler_a % kAdlerMod, s.adler_b % kAdlerMod};
  }
  unsigned long long carry = 0;      // frame
  uint32_t a_carry = 1, b_sum = 0;
  for (long sg = 0; sg < l.nseg; ++sg) {
    const long left = l.S - sg * kSegment;
    const uint32_t n = static_cast<uint32_t>(left < kSegment ? left : kSegment);
    segoff[sg] = carry;
    carry += info[sg].total_bits;
    b_sum = static_cast<uint32_t>((b_sum + info[sg].adler_b + static_cast<unsigned long long>(n) * a_carry) % kAdlerMod);
    a_carry = (a_carry + info[sg].adler_a) % kAdlerMod;
  }
  bits[0] = carry;
  if (static_cast<long>((carry + 7) >> 3) > max_deflate_bytes(H, W)) fail("a stream above its bound", static_cast<long>(carry));
  if (force && static_cast<long>((carry + 7) >> 3) != max_deflate_bytes(H, W)) fail("the forced case does not reach the bound", static_cast<long>(carry));
  const uint32_t adler = (b_sum << 16) | a_carry;
  const int length = write_frame(out, make_front(H, W), carry, adler);
  uint32_t* rowp = reinterpret_cast<uint32_t*>(out);
  auto store = [&](long wi, uint32_t word) {
    if (word) rowp[wi] |= word;      // no `wi < words` here: the sanitizer is the check
  };
  for (long seg = 0; seg < l.nseg; ++seg) {      // pack
    const long at = seg * kSegment;
    const SegInfo si = info[seg];
    const uint32_t* sc = code + seg * 288;
    const unsigned long long base = 8ull * kFront + segoff[seg];
    const int n = static_cast<int>(l.S - at < kSegment ? l.S - at : kSegment);
    for (int t = 0; t < kThreads; ++t) {
      for (uint32_t hw = t; hw < kHeaderWords && 32u * hw < si.header_bits; hw += kThreads) {
        const uint32_t left = si.header_bits - 32u * hw;
        BitWriter<decltype(store)> w(store, base + 32u * hw);
        w.put(header[seg * kHeaderWords + hw], static_cast<int>(left < 32u ? left : 32u));
        w.finish();
      }
      const int nv = n - t * kChunk < 0 ? 0 : n - t * kChunk > kChunk ? kChunk : n - t * kChunk;
      if (nv) {
        const uint32_t* tk = reinterpret_cast<const uint32_t*>(tok + at) + t * (kChunk / 2);
        BitWriter<decltype(store)> w(store, base + chunkoff[seg * kThreads + t]);
        for (int j = 0; j < nv; ++j) {
          const uint32_t tv = (tk[j >> 1] >> (16 * (j & 1))) & 0xFFFFu;
          if (tv != kNone && tv < 256u + 259u) put_token(w, tv, sc);
        }
        w.finish();
      }
      if (t == 0) {
        const uint32_t len = sc[256] & 15u;
        BitWriter<decltype(store)> w(store, base + si.total_bits - len);
        w.put(sc[256] >> 4, static_cast<int>(len));
        w.finish();
      }
    }
  }
  const long nb = static_cast<long>((carry + 7) >> 3), total = 4 + 2 + nb + 4;      // crc
  uint8_t* p = out + 37;
  uint32_t acc = 0;
  for (int t = 0; t < kThreads; ++t)
    for (long b0 = 0; b0 < total; b0 += static_cast<long>(kThreads) * kChunk) {
      const long first = b0 + static_cast<long>(t) * kChunk;
      if (first < total) {
        const int len = static_cast<int>(total - first < kChunk ? total - first : kChunk);
        acc ^= crc_shift(kCrc.x2n, crc_bytes(kCrc.byte, p + first, len), static_cast<unsigned long long>(total - first - len));
      }
    }
  put_be32(p + total, acc);
  // ---- checks from the outside: chunk layout, CRC-32s with one plain loop per chunk, Adler-32 with a plain loop, the length ----
  if (length != 57 + 6 + nb || length > cap) fail("the file's length", length, cap);
  auto be32 = [&](long at) { return (uint32_t(out[at]) << 24) | (uint32_t(out[at + 1]) << 16) | (uint32_t(out[at + 2]) << 8) | out[at + 3]; };
  auto plain_crc = [&](long at, long n) {
    uint32_t c = 0xFFFFFFFFu;
    for (long i = 0; i < n; ++i) c = kCrc.byte[(c ^ out[at + i]) & 255u] ^ (c >> 8);
    return c ^ 0xFFFFFFFFu;
  };
  static const uint8_t sig[8] = {0x89, 'P', 'N', 'G', 13, 10, 26, 10};
  if (std::memcmp(out, sig, 8)) fail("the signature");
  long at = 8;
  const char* kinds[3] = {"IHDR", "IDAT", "IEND"};
  for (int k = 0; k < 3; ++k) {
    const long n = be32(at);
    if (at + 12 + n > length || std::memcmp(out + at + 4, kinds[k], 4)) fail("the chunk order", k, at);
    if (plain_crc(at + 4, 4 + n) != be32(at + 8 + n)) fail("a chunk CRC-32", k);
    if (k == 0 && (n != 13 || be32(at + 8) != uint32_t(W) || be32(at + 12) != uint32_t(H) || out[at + 16] != 8 || out[at + 17] || out[at + 18] ||
                   out[at + 19] || out[at + 20]))
      fail("IHDR");
    if (k == 1) {
      if (n != nb + 6 || out[at + 8] != 0x78 || out[at + 9] != 0x01) fail("the zlib header or IDAT's length", n);
      uint32_t a = 1, b = 0;
      for (long i = 0; i < l.S; ++i) { a = (a + filt[i]) % kAdlerMod; b = (b + a) % kAdlerMod; }
      if (be32(at + 8 + n - 4) != ((b << 16) | a)) fail("the Adler-32");
      if ((carry & 7) && (out[at + 8 + 2 + nb - 1] >> (carry & 7))) fail("the last byte's padding");
    }
    at += 12 + n;
  }
  if (at != length) fail("bytes behind IEND", at, length);
  for (long i = length; i < cap; ++i)
    if (out[i]) fail("a byte behind the file", i);
  return length;
}

static long run(const uint8_t* in, int H, int W, std::vector<uint8_t>* file, bool force = false) {
  const long cap = capacity(H, W);
  const Layout l = layout(1, H, W);
  uint8_t* out = static_cast<uint8_t*>(std::malloc(static_cast<size_t>(cap)));      // exact sizes: red zones behind them
  char* ws = static_cast<char*>(std::aligned_alloc(16, l.bytes));
  std::memset(out, 0xA5, static_cast<size_t>(cap));
  std::memset(ws, 0xA5, l.bytes);
  const long len = encode(in, H, W, out, cap, ws, force);
  if (file) file->assign(out, out + len);
  std::free(out); std::free(ws);
  return len;
}

int main(int argc, char** argv) {
  if (argc == 5) {
    const int H = std::atoi(argv[2]), W = std::atoi(argv[3]);
    if (!shape_ok(1, H, W)) fail("the shape", H, W);
    std::vector<uint8_t> in(static_cast<size_t>(H) * W), file;
    FILE* f = std::fopen(argv[1], "rb");
    if (!f || std::fread(in.data(), 1, in.size(), f) != in.size()) { std::fprintf(stderr, "cannot read %s\n", argv[1]); return 1; }
    std::fclose(f);
    run(in.data(), H, W, &file);
    f = std::fopen(argv[4], "wb");
    if (!f || std::fwrite(file.data(), 1, file.size(), f) != file.size()) { std::fprintf(stderr, "cannot write %s\n", argv[4]); return 1; }
    std::fclose(f);
    return 0;
  }
  unsigned sd = 12345u;
  auto rnd = [&] { sd = sd * 1664525u + 1013904223u; return static_cast<uint8_t>(sd >> 24); };
  const int shapes[][2] = {{1, 1}, {1, 5}, {300, 1}, {7, 13}, {17, 33}, {2, 8192}, {16, 16}, {33, 48}, {120, 160}, {128, 127}, {113, 144}, {130, 130}, {224, 384}};
  for (auto& hw : shapes) {
    const int H = hw[0], W = hw[1];
    std::vector<uint8_t> in(static_cast<size_t>(H) * W);
    // contents: zeros; noise; large noise (the Adler sums); a smooth ramp with flat parts; rows of runs
    for (int kind = 0; kind < 5; ++kind) {
      for (int y = 0; y < H; ++y)
        for (int x = 0; x < W; ++x) {
          uint8_t& v = in[static_cast<size_t>(y) * W + x];
          v = kind == 0 ? 0 : kind == 1 ? rnd() : kind == 2 ? static_cast<uint8_t>(200 + rnd() % 56) : kind == 3 ? static_cast<uint8_t>((x / 7 + y / 5) % 40 < 20 ? 0 : (x + y) / 3)
                                                                                                                  : static_cast<uint8_t>((x % 523 < 261 + y % 7) ? 9 : rnd());
        }
      const long len = run(in.data(), H, W, nullptr);
      std::printf("%d x %d kind %d: %ld of %ld bytes\n", H, W, kind, len, capacity(H, W));
    }
    // forced worst case: every stream byte a literal of 15 bits behind headers of 4092 bits
    const long len = run(in.data(), H, W, nullptr, true);
    std::printf("%d x %d forced: %ld of %ld bytes\n", H, W, len, capacity(H, W));
  }
  std::printf("ok\n");
  return 0;
}
