// The arithmetic, the tables and the buffer layout of the PNG decode (include/diffsal.h, "PNG decode"), callable from the host and
// from the device: csrc/png_decode.hip runs it in kernels, tools/png_decode_host_check.cpp runs the same functions and the same
// index arithmetic serially on the host, one loop iteration per device lane, where a sanitizer can watch every buffer.  Integer
// work only.
//
// A wave works on one file.  Code that the 64 lanes run in step is written once: what is the same for all lanes (the bit reader,
// the symbol decode) is plain code, run redundantly by every lane on the device and once on the host; what the lanes share out is
// a PNG_LANES(l) loop, one trip with l = the lane on the device and 64 trips on the host; PNG_SYNC() separates a phase that
// writes the shared arrays from one that reads them.
// PNG_FROM_LANE_BELOW(a, l, u) is a[u] of lane l - 1 (lane 0: its own), a shuffle on the device; on the host the per-lane arrays
// have a slot per lane and the read is an index, so it stands in a PNG_LANES loop of its own, in front of the one that writes a.
// PNG_UNIFORM(x) marks a value every lane reads from the same address: on the device it is taken from the first lane, which keeps
// the decoder's state in scalar registers and its branches scalar.
//
// Nothing here trusts the file's bytes or the descriptor's numbers: every read of the stream is clamped to its range, every write
// to the file's region, and every loop has a bound from the geometry or from the remaining input bits.
#pragma once
#include <cstddef>
#include <cstdint>

#if defined(__HIPCC__)
#define PNG_HD __host__ __device__ __forceinline__
// forced: left to the inliner, one build_table (the dynamic blocks' distance table) stayed an out-of-line call in the inflate kernel,
// and in that build the match copies lost the stores of lanes 0-31 on the device, also in files of fixed blocks that never reach
// the call; the host run of the same source was right.  The kernel must hold no call (tests/test_gpu_png_decode.py names the files)
#define PNG_DEV __device__ __forceinline__
#define PNG_UNROLL _Pragma("unroll")
#else
#define PNG_UNROLL
#define PNG_HD inline
#define PNG_DEV inline
#endif
#if defined(__HIP_DEVICE_COMPILE__)
#define PNG_LANES(l) for (int l = static_cast<int>(threadIdx.x), l##_once = 1; l##_once; l##_once = 0)
#define PNG_SLOT(l) 0
#define PNG_SLOTS 1
#define PNG_SYNC() __syncthreads()
#define PNG_LANE0 (threadIdx.x == 0)
#define PNG_UNIFORM(x) static_cast<uint32_t>(__builtin_amdgcn_readfirstlane(static_cast<int>(x)))
#define PNG_FROM_LANE_BELOW(a, l, u) static_cast<uint32_t>(__shfl_up(static_cast<int>((a)[0][u]), 1, 64))
#define PNG_OR(flag, v) atomicOr(&(flag), (v))
#else
#define PNG_LANES(l) for (int l = 0; l < 64; ++l)
#define PNG_SLOT(l) (l)
#define PNG_SLOTS 64
#define PNG_SYNC() ((void)0)
#define PNG_LANE0 true
#define PNG_UNIFORM(x) static_cast<uint32_t>(x)
#define PNG_FROM_LANE_BELOW(a, l, u) ((a)[(l) ? (l) - 1 : 0][u])
#define PNG_OR(flag, v) ((flag) |= (v))
#endif

namespace diffsal {
namespace png {

constexpr int kLanes = 64;            // one wave per file, in both kernels
constexpr int kMaxN = 65535, kMaxH = 65535;
constexpr int kMaxW = 8192;           // the row above a band of 64 rows is kept in LDS, four bytes per filter unit
constexpr int kWindow = 32768;        // deflate's history: a ring in LDS, every match reads it there
constexpr int kInBytes = 4096;        // the staged part of the stream, refilled by halves
constexpr int kFlush = 1024;          // bytes of the ring written out per flush: 16 per lane

// status bits (include/diffsal.h DIFFSAL_PNG_*)
constexpr int kBadBlock = 1;          // block type 3
constexpr int kBadStored = 2;         // a stored block whose LEN and NLEN disagree
constexpr int kBadLengths = 4;        // an invalid or over-subscribed set of code lengths
constexpr int kBadSymbol = 8;         // an invalid literal/length or distance symbol
constexpr int kBadDistance = 16;      // a distance that reaches before the start of the output
constexpr int kNoInput = 32;          // the stream's bits ran out
constexpr int kShort = 64;            // the stream ended with fewer bytes than the image needs
constexpr int kLong = 128;            // the stream carries more bytes than the image needs (the pixels are delivered)
constexpr int kBadFilter = 256;       // a filter type above 4
constexpr int kBadAdler = 512;        // Adler-32 of the inflated bytes is not the stream's

// what the host uploads per file (784 bytes; the same layout as the NumPy record of diff_sal_amd/png.py)
struct FileDesc {
  uint32_t off, len;      // the file's zlib stream (its IDAT payloads end to end) in the packed buffer; off is a multiple of 16
  uint32_t pad[2];
  uint8_t pal[768];       // PLTE, zero-padded
};
static_assert(sizeof(FileDesc) == 784, "FileDesc layout");
// what the inflate launch leaves per file for the unfilter launch
struct FileState { int32_t status; uint32_t produced, adler, adler_valid; };

struct Geom {
  int N, H, W, ctype, depth;
  int bpp;             // the filters' unit: bytes per pixel, 1 below 8 bits
  int units, groups;   // units per row; groups of four units per row
  long row_bytes, stride, total, region;      // stride = 1 + row_bytes; total = H * stride; region: total padded to 16
  size_t state, data, bytes;                  // byte offsets into the workspace; its size
};
PNG_HD int channels(int ctype) { return ctype == 2 ? 3 : ctype == 4 ? 2 : ctype == 6 ? 4 : 1; }
inline bool geom_ok(int N, int H, int W, int ctype, int depth) {
  if (!(N >= 1 && N <= kMaxN && H >= 1 && H <= kMaxH && W >= 1 && W <= kMaxW)) return false;
  const bool t8 = ctype == 0 || ctype == 2 || ctype == 3 || ctype == 4 || ctype == 6;
  if (!((depth == 8 && t8) || ((depth == 1 || depth == 2 || depth == 4) && (ctype == 0 || ctype == 3)))) return false;
  const long row = (static_cast<long>(W) * channels(ctype) * depth + 7) / 8;
  return static_cast<long>(H) * (1 + row) <= 0x7FFFFFF0L;
}
inline Geom geom(int N, int H, int W, int ctype, int depth) {
  Geom g{};
  g.N = N; g.H = H; g.W = W; g.ctype = ctype; g.depth = depth;
  g.row_bytes = (static_cast<long>(W) * channels(ctype) * depth + 7) / 8;
  g.bpp = depth == 8 ? channels(ctype) : 1;
  g.units = static_cast<int>(g.row_bytes / g.bpp);
  g.groups = (g.units + 3) / 4;
  g.stride = 1 + g.row_bytes;
  g.total = static_cast<long>(H) * g.stride;
  g.region = (g.total + 15) & ~15L;
  g.state = 0;
  g.data = (static_cast<size_t>(N) * sizeof(FileState) + 15) & ~static_cast<size_t>(15);
  g.bytes = g.data + static_cast<size_t>(N) * g.region;
  return g;
}

// ---- inflate (RFC 1951) ---------------------------------------------------------------------------------------------------------
// canonical codes: counts per length and the symbols in code order for the long-code path, a look-up on the next 9 bits in front
struct CodeTable {
  uint16_t look[512];      // (length << 9) | symbol for codes of at most 9 bits, 0: none
  uint16_t count[16];
  uint16_t symbol[288];
};
struct InflateShared {      // LDS on the device
  alignas(16) uint8_t ring[kWindow];
  alignas(16) uint32_t in[kInBytes / 4];
  CodeTable lit, dist, clen;
  uint8_t lens[320];
};
struct Bits {
  uint64_t buf;
  int cnt;                  // bits in buf
  long pos, staged;         // bytes taken into buf; bytes staged (the ring holds [staged - kInBytes, staged))
  long used, total;         // bits consumed; bits the stream holds
};
struct Counters { long iterations, copies, flushes; };      // the host check's loop counts

// bytes [from, from + n) of the stream into the input ring, zeros behind the stream's end; n and from are multiples of 4
PNG_DEV void stage(InflateShared& s, const uint32_t* words, long off, long len, long from, int n) {
  PNG_SYNC();
  PNG_LANES(l) {
    for (int i = l; i < n / 4; i += kLanes) {
      const long b = from + 4L * i;
      uint32_t w = 0;
      if (b < len) {
        w = words[(off + b) >> 2];      // off + len <= nbytes, both multiples of 4 or the tail masked below
        if (len - b < 4) w &= (1u << (8 * static_cast<int>(len - b))) - 1u;
      }
      s.in[(b >> 2) & (kInBytes / 4 - 1)] = w;
    }
  }
  PNG_SYNC();
}
PNG_DEV void refill(Bits& b, InflateShared& s, const uint32_t* words, long off, long len) {
  if (b.cnt > 32) return;
  if (b.pos >= b.staged - kInBytes / 2) {
    stage(s, words, off, len, b.staged, kInBytes / 2);
    b.staged += kInBytes / 2;
  }
  b.buf |= static_cast<uint64_t>(PNG_UNIFORM(s.in[(b.pos >> 2) & (kInBytes / 4 - 1)])) << b.cnt;
  b.cnt += 32;
  b.pos += 4;
}
// n <= 16; n = 0 takes nothing
#define PNG_GETBITS(n) get_bits(b, s, words, off, len, (n))
PNG_DEV uint32_t get_bits(Bits& b, InflateShared& s, const uint32_t* words, long off, long len, int n) {
  refill(b, s, words, off, len);
  const uint32_t v = static_cast<uint32_t>(b.buf) & ((1u << n) - 1u);
  b.buf >>= n;
  b.cnt -= n;
  b.used += n;
  return v;
}

// Builds t from n code lengths (each 0..15).  0: usable.  zlib's rules: an over-subscribed set is an error, an incomplete one too
// unless it is a single code of length 1 (or no code at all for `allow_empty`); the code-length code (`complete_only`) must be
// complete whatever its longest code
PNG_DEV int build_table(CodeTable& t, const uint8_t* lens, int n, bool allow_empty, bool complete_only = false) {
  PNG_SYNC();
  PNG_LANES(l) for (int i = l; i < 512; i += kLanes) t.look[i] = 0;
  if (PNG_LANE0) {
    uint16_t offs[16];
    for (int i = 0; i < 16; ++i) t.count[i] = 0;
    for (int i = 0; i < n; ++i) ++t.count[lens[i] & 15];
    offs[1] = 0;
    for (int i = 1; i < 15; ++i) offs[i + 1] = static_cast<uint16_t>(offs[i] + t.count[i]);
    for (int i = 0; i < n; ++i)
      if (lens[i] & 15) t.symbol[offs[lens[i] & 15]++] = static_cast<uint16_t>(i);      // the offsets sum to at most n <= 288
  }
  PNG_SYNC();
  int left = 1, maxlen = 0, used = 0;
  for (int i = 1; i <= 15; ++i) {
    const int n_i = static_cast<int>(PNG_UNIFORM(t.count[i]));
    left = (left << 1) - n_i;
    if (left < 0) return kBadLengths;
    if (n_i) maxlen = i;
    used += n_i;
  }
  if (used == 0) {
    if (!allow_empty) return kBadLengths;
  } else if (left > 0 && (complete_only || maxlen != 1)) {
    return kBadLengths;
  }
  // a lane per code of at most 9 bits: its entries of the look-up
  PNG_LANES(l) {
    for (int i = l; i < used; i += kLanes) {
      int first = 0, index = 0, len = 1;
      for (; len <= 15; ++len) {
        if (i < index + t.count[len]) break;
        index += t.count[len];
        first = (first + t.count[len]) << 1;
      }
      if (len > 9) continue;
      const uint32_t code = static_cast<uint32_t>(first + (i - index));
      uint32_t rev = 0;
      for (int k = 0; k < len; ++k) rev |= ((code >> k) & 1u) << (len - 1 - k);
      const uint16_t e = static_cast<uint16_t>((len << 9) | t.symbol[i]);
      for (uint32_t m = rev; m < 512u; m += 1u << len) t.look[m] = e;
    }
  }
  PNG_SYNC();
  return 0;
}
// the next symbol of table t, -1 if no code matches.  Consumes the code's bits: at least one, or returns -1
PNG_DEV int decode_symbol(Bits& b, InflateShared& s, const uint32_t* words, long off, long len, const CodeTable& t) {
  refill(b, s, words, off, len);      // more than 32 bits in buf
  const uint32_t e = PNG_UNIFORM(t.look[static_cast<uint32_t>(b.buf) & 511u]);
  if (e) {
    const int n = static_cast<int>(e >> 9);
    b.buf >>= n; b.cnt -= n; b.used += n;
    return static_cast<int>(e & 511u);
  }
  int code = 0, first = 0, index = 0;
  for (int n = 1; n <= 15; ++n) {
    code |= static_cast<int>((b.buf >> (n - 1)) & 1u);
    const int count = static_cast<int>(PNG_UNIFORM(t.count[n]));
    if (code - count < first) {
      b.buf >>= n; b.cnt -= n; b.used += n;
      return static_cast<int>(PNG_UNIFORM(t.symbol[index + (code - first)]));      // index + count <= the symbols built
    }
    index += count;
    first = (first + count) << 1;
    code <<= 1;
  }
  return -1;
}

// ring[flushed, flushed + kFlush) -> the file's region, 16 bytes per lane, zeros from `valid` on; nothing at or behind g.region
PNG_DEV void flush(const InflateShared& s, const Geom& g, uint8_t* region, long flushed, long valid) {
  PNG_SYNC();
  PNG_LANES(l) {
    const long c = flushed + 16L * l;
    if (c < g.region) {
      uint32_t w[4];
      __builtin_memcpy(w, __builtin_assume_aligned(s.ring + (c & (kWindow - 1)), 16), 16);
      for (int k = 0; k < 4; ++k) {
        const long at = c + 4 * k;
        if (at >= valid) w[k] = 0;
        else if (valid - at < 4) w[k] &= (1u << (8 * static_cast<int>(valid - at))) - 1u;
      }
      __builtin_memcpy(__builtin_assume_aligned(region + c, 16), w, 16);
    }
  }
}

// The zlib stream bytes [off, off + len) of the packed buffer (`words`, nbytes long) -> the file's filtered scanlines in `region`
// (g.region bytes, 16-byte aligned; every byte is written: zeros behind what the stream gave) and the file's state
PNG_DEV void inflate_file(InflateShared& s, const uint32_t* words, long nbytes, long off, long len, const Geom& g, uint8_t* region,
                          FileState* state, Counters* ctr) {
  if ((off & 3) || off > nbytes) len = 0;
  if (len > nbytes - off) len = nbytes - off;
  if (len < 0) len = 0;
  Bits b{0, 0, 0, kInBytes, 0, 8 * len};
  stage(s, words, off, len, 0, kInBytes);
  int status = 0;
  long outpos = 0, flushed = 0;      // outpos <= g.total + 258
  uint32_t adler = 0, adler_valid = 0;
  bool fixed_built = false, done = false;
  (void)PNG_GETBITS(16);      // CMF, FLG: checked by the host parser
  // every trip of every loop below consumes at least one bit or ends the decode: at most b.total + 64 trips in all
  while (!done && !status) {
    const uint32_t last = PNG_GETBITS(1), type = PNG_GETBITS(2);
    if (b.used > b.total) { status |= kNoInput; break; }
    if (type == 3) { status |= kBadBlock; break; }
    if (type == 0) {
      (void)PNG_GETBITS(static_cast<int>((8 - (b.used & 7)) & 7));
      const uint32_t n = PNG_GETBITS(16), nn = PNG_GETBITS(16);
      if (b.used > b.total) { status |= kNoInput; break; }
      if ((n ^ 0xFFFFu) != nn) { status |= kBadStored; break; }
      for (uint32_t i = 0; i < n && !status; ++i) {
        const uint32_t v = PNG_GETBITS(8);
        if (ctr) ++ctr->iterations;
        if (b.used > b.total) { status |= kNoInput; break; }
        if (outpos >= g.total) { status |= kLong; break; }
        if (PNG_LANE0) s.ring[outpos & (kWindow - 1)] = static_cast<uint8_t>(v);
        ++outpos;
        if (flushed + kFlush <= outpos) {
          flush(s, g, region, flushed, outpos);
          flushed += kFlush;
          if (ctr) ++ctr->flushes;
        }
      }
    } else {
      if (type == 1) {
        if (!fixed_built) {
          PNG_SYNC();
          PNG_LANES(l) for (int i = l; i < 320; i += kLanes) s.lens[i] = i < 144 ? 8 : i < 256 ? 9 : i < 280 ? 7 : i < 288 ? 8 : 5;
          (void)build_table(s.lit, s.lens, 288, false);
          (void)build_table(s.dist, s.lens + 288, 32, false);
          fixed_built = true;
        }
      } else {
        fixed_built = false;
        const int nlen = static_cast<int>(PNG_GETBITS(5)) + 257, ndist = static_cast<int>(PNG_GETBITS(5)) + 1;
        const int ncode = static_cast<int>(PNG_GETBITS(4)) + 4;
        if (nlen > 286 || ndist > 30) { status |= kBadLengths; break; }
        PNG_SYNC();
        PNG_LANES(l) if (l < 19) s.lens[l] = 0;
        PNG_SYNC();
        for (int i = 0; i < ncode; ++i) {
          const uint32_t v = PNG_GETBITS(3);
          const int order = i < 3 ? 16 + i : i == 3 ? 0 : (i & 1) ? 7 - (i - 5) / 2 : 8 + (i - 4) / 2;      // 16 17 18 0 8 7 9 6 10 5 11 4 12 3 13 2 14 1 15
          if (PNG_LANE0) s.lens[order] = static_cast<uint8_t>(v);
        }
        if (build_table(s.clen, s.lens, 19, false, true)) { status |= kBadLengths; break; }
        int at = 0, prev = 0;
        while (at < nlen + ndist) {      // a symbol per trip
          if (ctr) ++ctr->iterations;
          const int sym = decode_symbol(b, s, words, off, len, s.clen);
          if (sym < 0 || b.used > b.total) { status |= sym < 0 ? kBadLengths : kNoInput; break; }
          int rep = 1, val = sym;
          if (sym == 16) {
            if (at == 0) { status |= kBadLengths; break; }
            val = prev; rep = 3 + static_cast<int>(PNG_GETBITS(2));
          } else if (sym == 17) {
            val = 0; rep = 3 + static_cast<int>(PNG_GETBITS(3));
          } else if (sym == 18) {
            val = 0; rep = 11 + static_cast<int>(PNG_GETBITS(7));
          }
          if (at + rep > nlen + ndist) { status |= kBadLengths; break; }
          if (PNG_LANE0) for (int k = 0; k < rep; ++k) s.lens[at + k] = static_cast<uint8_t>(val);      // at + rep <= 316
          at += rep;
          prev = val;
        }
        if (status) break;
        if (b.used > b.total) { status |= kNoInput; break; }
        PNG_SYNC();
        if (PNG_UNIFORM(s.lens[256]) == 0) { status |= kBadLengths; break; }      // no end-of-block code
        // the distance lengths behind the literal/length ones, moved to a fixed place first
        uint8_t dl[PNG_SLOTS];
        PNG_LANES(l) dl[PNG_SLOT(l)] = l < ndist ? s.lens[nlen + l] : 0;
        PNG_SYNC();
        PNG_LANES(l) if (l < 32) s.lens[288 + l] = dl[PNG_SLOT(l)];
        if (build_table(s.lit, s.lens, nlen, false) || build_table(s.dist, s.lens + 288, ndist, true)) { status |= kBadLengths; break; }
      }
      for (;;) {      // a symbol per trip
        if (ctr) ++ctr->iterations;
        int sym = decode_symbol(b, s, words, off, len, s.lit);
        if (sym < 0) { status |= kBadSymbol; break; }
        if (b.used > b.total) { status |= kNoInput; break; }
        if (sym == 256) break;
        if (sym < 256) {
          if (outpos >= g.total) { status |= kLong; break; }
          if (PNG_LANE0) s.ring[outpos & (kWindow - 1)] = static_cast<uint8_t>(sym);
          ++outpos;
        } else {
          sym -= 257;
          if (sym >= 29) { status |= kBadSymbol; break; }
          const int le = sym < 8 || sym == 28 ? 0 : (sym >> 2) - 1;
          const int length = (sym < 8 ? 3 + sym : sym == 28 ? 258 : 3 + ((4 + (sym & 3)) << le)) + static_cast<int>(PNG_GETBITS(le));
          const int ds = decode_symbol(b, s, words, off, len, s.dist);
          if (ds < 0 || ds >= 30) { status |= kBadSymbol; break; }
          const int de = ds < 4 ? 0 : (ds >> 1) - 1;
          int dist = ds < 4 ? 1 + ds : 1 + ((2 + (ds & 1)) << de);
          dist += static_cast<int>(PNG_GETBITS(de));      // de <= 13
          if (b.used > b.total) { status |= kNoInput; break; }
          if (dist > outpos) { status |= kBadDistance; break; }
          const int take = static_cast<int>(g.total - outpos < length ? g.total - outpos : length);      // the image's bytes only
          // the lanes copy together: byte j comes from the `dist` bytes in front of the match, repeated with period dist when
          // dist < length.  All sources lie in front of outpos, so every lane reads all its bytes, then every lane writes
          if (ctr) ++ctr->copies;
          uint8_t v[PNG_SLOTS][5];
          PNG_SYNC();
          PNG_LANES(l) {
            for (int r = 0; r < 5; ++r) {
              const int j = l + kLanes * r;
              if (j < take) v[PNG_SLOT(l)][r] = s.ring[(outpos - dist + (dist >= length ? j : j % dist)) & (kWindow - 1)];
            }
          }
          PNG_SYNC();      // in the ring a source slot can be another lane's destination once dist + length > 32768
          PNG_LANES(l) {
            for (int r = 0; r < 5; ++r) {
              const int j = l + kLanes * r;
              if (j < take) s.ring[(outpos + j) & (kWindow - 1)] = v[PNG_SLOT(l)][r];
            }
          }
          outpos += take;
          if (take < length) { status |= kLong; break; }
        }
        if (flushed + kFlush <= outpos) {      // a symbol adds at most 258 bytes: one flush keeps up
          flush(s, g, region, flushed, outpos);
          flushed += kFlush;
          if (ctr) ++ctr->flushes;
        }
      }
    }
    if (last && !status) done = true;
  }
  if (done) {
    (void)PNG_GETBITS(static_cast<int>((8 - (b.used & 7)) & 7));
    for (int i = 0; i < 4; ++i) adler = (adler << 8) | PNG_GETBITS(8);
    if (b.used > b.total) status |= kNoInput;
    else adler_valid = 1;
  }
  if (outpos > g.total) outpos = g.total;
  if (outpos < g.total && !(status & kLong)) status |= kShort;
  // the rest of the region: what the ring still holds, then zeros.  (g.region - flushed) / kFlush + 1 trips
  for (; flushed < g.region; flushed += kFlush) {
    flush(s, g, region, flushed, outpos);
    if (ctr) ++ctr->flushes;
  }
  if (PNG_LANE0) {
    state->status = status;
    state->produced = static_cast<uint32_t>(outpos);
    state->adler = adler;
    state->adler_valid = adler_valid;
  }
}

// ---- Adler-32 (RFC 1950) of region[0, n): lane l takes bytes [16 l, 16 l + 16) of every tile of 1024 -----------------------------
constexpr uint32_t kAdlerMod = 65521;
// one lane's share of the tile at `t0`, m = min(1024, n - t0) bytes long: s1 = the sum of its bytes, s2 = the sum of
// (m - index in the tile) * byte.  region + t0 + 16 l is 16-byte aligned and inside the region (padded to 16)
PNG_HD void adler_lane_tile(const uint8_t* region, long t0, int m, int l, uint32_t& s1, uint32_t& s2) {
  s1 = 0; s2 = 0;
  if (16 * l >= m) return;
  uint32_t w[4];
  __builtin_memcpy(w, __builtin_assume_aligned(region + t0 + 16 * l, 16), 16);
  for (int k = 0; k < 16; ++k) {
    const int j = 16 * l + k;
    if (j < m) {
      const uint32_t v = (w[k >> 2] >> (8 * (k & 3))) & 255u;
      s1 += v;
      s2 += static_cast<uint32_t>(m - j) * v;      // <= 1024 * 255 * 16
    }
  }
}
// per lane over all tiles: run1 = the sum of its s1 so far, acc2 += m * run1 (before this tile) + s2; both mod 65521
PNG_HD void adler_lane_step(uint32_t& run1, uint32_t& acc2, int m, uint32_t s1, uint32_t s2) {
  acc2 = static_cast<uint32_t>((static_cast<uint64_t>(acc2) + static_cast<uint64_t>(m) * run1 + s2) % kAdlerMod);
  run1 = (run1 + s1) % kAdlerMod;
}
// the lanes' sums -> the checksum of n bytes (the initial 1 of the low half adds n to the high half)
PNG_HD uint32_t adler_combine(const uint32_t* run1, const uint32_t* acc2, long n) {
  uint64_t a = 1, b = static_cast<uint64_t>(n % kAdlerMod);
  for (int l = 0; l < kLanes; ++l) { a += run1[l]; b += acc2[l]; }
  return static_cast<uint32_t>(((b % kAdlerMod) << 16) | (a % kAdlerMod));
}

// ---- filters (PNG 9.2), four bytes of a unit side by side in a word; bytes a unit does not have stay zero --------------------------
PNG_HD uint32_t paeth(int a, int b, int c) {
  const int p = a + b - c;
  const int pa = p > a ? p - a : a - p, pb = p > b ? p - b : b - p, pc = p > c ? p - c : c - p;
  return static_cast<uint32_t>(pa <= pb && pa <= pc ? a : pb <= pc ? b : c);
}
PNG_HD uint32_t unfilter_unit(int filter, uint32_t raw, uint32_t left, uint32_t up, uint32_t upleft) {
  uint32_t out = 0;
PNG_UNROLL
  for (int k = 0; k < 4; ++k) {
    const int x = (raw >> (8 * k)) & 255, a = (left >> (8 * k)) & 255, b = (up >> (8 * k)) & 255, c = (upleft >> (8 * k)) & 255;
    const uint32_t pred = filter == 1 ? a : filter == 2 ? b : filter == 3 ? static_cast<uint32_t>((a + b) >> 1) : filter == 4 ? paeth(a, b, c) : 0u;
    out |= ((static_cast<uint32_t>(x) + pred) & 255u) << (8 * k);
  }
  return out;
}
// the diagonal: at step t lane k works on group t - k of its row, one group behind lane k - 1, whose result of the step before
// is this lane's row above.  A band of 64 rows takes g.groups + 63 steps
PNG_HD int band_steps(const Geom& g) { return g.groups + kLanes - 1; }
// the raw bytes of group G of `row`, a unit per word; zeros for units the row does not have.  row < g.H, 0 <= G < g.groups
PNG_HD void load_group(const Geom& g, const uint8_t* region, int row, int G, uint32_t raw[4]) {
  const uint8_t* p = region + static_cast<long>(row) * g.stride + 1;
PNG_UNROLL
  for (int u = 0; u < 4; ++u) {
    raw[u] = 0;
    const long at = (4L * G + u) * g.bpp;
    if (4 * G + u < g.units)
      for (int k = 0; k < g.bpp; ++k) raw[u] |= static_cast<uint32_t>(p[at + k]) << (8 * k);      // at + k < g.row_bytes
  }
}
// one lane's step: raw -> recon (left: the lane's last unit of the group before; up: the group above; upleft: the last unit of
// the group above and before)
PNG_HD void unfilter_group(int filter, const uint32_t raw[4], uint32_t left, const uint32_t up[4], uint32_t upleft, uint32_t recon[4]) {
PNG_UNROLL
  for (int u = 0; u < 4; ++u) {
    recon[u] = unfilter_unit(filter, raw[u], left, up[u], upleft);
    left = recon[u];
    upleft = up[u];
  }
}

// ---- samples -> Pillow's RGB / L -------------------------------------------------------------------------------------------------
PNG_HD uint32_t rgb_l(uint32_t r, uint32_t g, uint32_t b) { return (19595u * r + 38470u * g + 7471u * b + 0x8000u) >> 16; }
// palette entry i as r | g << 8 | b << 16 | L << 24
PNG_HD uint32_t palette_word(const uint8_t* pal, int i) {
  const uint32_t r = pal[3 * i], g = pal[3 * i + 1], b = pal[3 * i + 2];
  return r | (g << 8) | (b << 16) | (rgb_l(r, g, b) << 24);
}
// an 8-bit pixel (a unit) as r | g << 8 | b << 16 | L << 24
PNG_HD uint32_t pixel_word(const Geom& g, const uint32_t* pal, uint32_t unit) {
  if (g.ctype == 3) return pal[unit & 255u];
  if (g.ctype == 0 || g.ctype == 4) { const uint32_t v = unit & 255u; return v * 0x01010101u; }      // alpha dropped
  const uint32_t r = unit & 255u, gg = (unit >> 8) & 255u, b = (unit >> 16) & 255u;
  return (unit & 0xFFFFFFu) | (rgb_l(r, gg, b) << 24);
}
// a sample of 1, 2 or 4 bits (index j of byte `unit`, most significant first) likewise
PNG_HD uint32_t sample_word(const Geom& g, const uint32_t* pal, uint32_t unit, int j) {
  const uint32_t v = (unit >> (8 - g.depth * (j + 1))) & ((1u << g.depth) - 1u);
  if (g.ctype == 3) return pal[v];
  return v * (g.depth == 1 ? 255u : g.depth == 2 ? 85u : 17u) * 0x01010101u;
}
// group G of `row` -> the file's frame `out` ([H][W][3] or [H][W] bytes, `out_base` its address for the alignment of wide stores).
// Writes pixels x < g.W of row < g.H only
PNG_HD void emit_group(const Geom& g, const uint32_t* pal, int mode_l, int row, int G, const uint32_t recon[4], uint8_t* out) {
  const int C = mode_l ? 1 : 3;
  if (g.depth == 8) {
    const int x0 = 4 * G;
    uint8_t* o = out + (static_cast<long>(row) * g.W + x0) * C;
    uint32_t p[4];
PNG_UNROLL
    for (int u = 0; u < 4; ++u) p[u] = pixel_word(g, pal, recon[u]);
    if (x0 + 4 <= g.W && (reinterpret_cast<uintptr_t>(o) & 3u) == 0) {
      uint32_t* o32 = reinterpret_cast<uint32_t*>(o);
      if (mode_l) {
        o32[0] = (p[0] >> 24) | ((p[1] >> 24) << 8) | ((p[2] >> 24) << 16) | ((p[3] >> 24) << 24);
      } else {
        o32[0] = (p[0] & 0xFFFFFFu) | (p[1] << 24);
        o32[1] = ((p[1] >> 8) & 0xFFFFu) | (p[2] << 16);
        o32[2] = ((p[2] >> 16) & 0xFFu) | (p[3] << 8);
      }
    } else {
PNG_UNROLL
      for (int u = 0; u < 4; ++u) {
        if (x0 + u >= g.W) continue;
        if (mode_l) o[u] = static_cast<uint8_t>(p[u] >> 24);
        else
          for (int k = 0; k < 3; ++k) o[3 * u + k] = static_cast<uint8_t>(p[u] >> (8 * k));
      }
    }
  } else {
    const int ppb = 8 / g.depth;
    for (int u = 0; u < 4; ++u) {
      if (4 * G + u >= g.units) continue;
      for (int j = 0; j < ppb; ++j) {
        const long x = (4L * G + u) * ppb + j;
        if (x >= g.W) break;
        const uint32_t p = sample_word(g, pal, recon[u], j);
        uint8_t* o = out + (static_cast<long>(row) * g.W + x) * C;
        if (mode_l) o[0] = static_cast<uint8_t>(p >> 24);
        else
          for (int k = 0; k < 3; ++k) o[k] = static_cast<uint8_t>(p >> (8 * k));
      }
    }
  }
}

// ---- the unfilter launch for one file: Adler-32 of the scanlines, then bands of 64 rows on the diagonal --------------------------------
struct UnfilterShared {      // LDS on the device
  uint32_t above[kMaxW];     // the row above the band, a unit per word; lane 63 leaves its row here for the next band's lane 0
  uint32_t pal[256];         // palette_word per entry
  uint32_t sum1[kLanes], sum2[kLanes];
  int bad_filter;
};
// region: the file's filtered scanlines (g.region bytes, 16-byte aligned); frame: its [H][W][3] or [H][W] bytes.  Returns the file's
// status (in every lane on the device).  Steps: ceil(n / 1024) Adler tiles, then ceil(H / 64) bands of band_steps(g) steps
PNG_DEV int unfilter_file(UnfilterShared& s, const Geom& g, const uint8_t* pal768, const uint8_t* region, const FileState& st, int mode_l,
                          uint8_t* frame, Counters* ctr) {
  PNG_LANES(l) {
    for (int i = l; i < 256; i += kLanes) s.pal[i] = palette_word(pal768, i);
    for (int i = l; i < 4 * g.groups; i += kLanes) s.above[i] = 0;      // 4 * groups <= units + 3 <= kMaxW (a multiple of 4)
  }
  if (PNG_LANE0) s.bad_filter = 0;
  const long n = st.produced <= g.total ? st.produced : g.total;      // what the stream gave
  PNG_LANES(l) {
    uint32_t run1 = 0, acc2 = 0;
    for (long t0 = 0; t0 < n; t0 += 1024) {
      const int m = static_cast<int>(n - t0 < 1024 ? n - t0 : 1024);
      uint32_t s1, s2;
      adler_lane_tile(region, t0, m, l, s1, s2);
      adler_lane_step(run1, acc2, m, s1, s2);
      if (ctr && l == 0) ++ctr->iterations;
    }
    s.sum1[l] = run1;
    s.sum2[l] = acc2;
  }
  PNG_SYNC();
  const int steps = band_steps(g);
  for (int r0 = 0; r0 < g.H; r0 += kLanes) {
    uint32_t recon[PNG_SLOTS][4], next[PNG_SLOTS][4], up[PNG_SLOTS][4], left[PNG_SLOTS], upleft[PNG_SLOTS];
    int filter[PNG_SLOTS];
    PNG_LANES(l) {
      const int k = PNG_SLOT(l), row = r0 + l;
      filter[k] = row < g.H ? region[static_cast<long>(row) * g.stride] : 0;
      if (filter[k] > 4) { PNG_OR(s.bad_filter, 1); filter[k] = 0; }
      left[k] = 0; upleft[k] = 0;
      for (int u = 0; u < 4; ++u) { recon[k][u] = 0; next[k][u] = 0; }
      if (l == 0) load_group(g, region, row, 0, next[k]);      // r0 < g.H
    }
    for (int t = 0; t < steps; ++t) {
      if (ctr) ++ctr->copies;
      PNG_LANES(l) {
        PNG_UNROLL
        for (int u = 0; u < 4; ++u) up[PNG_SLOT(l)][u] = PNG_FROM_LANE_BELOW(recon, l, u);      // its group of the step before
      }
      PNG_LANES(l) {
        const int k = PNG_SLOT(l), row = r0 + l, G = t - l;
        const bool live = row < g.H, work = live && G >= 0 && G < g.groups;
        uint32_t raw[4];
        PNG_UNROLL
        for (int u = 0; u < 4; ++u) raw[u] = next[k][u];
        if (l == 0 && work) {
          PNG_UNROLL
          for (int u = 0; u < 4; ++u) up[k][u] = s.above[4 * G + u];
        }
        if (live && G + 1 >= 0 && G + 1 < g.groups) load_group(g, region, row, G + 1, next[k]);      // a step ahead
        if (work) {
          if (G == 0) { left[k] = 0; upleft[k] = 0; }
          unfilter_group(filter[k], raw, left[k], up[k], upleft[k], recon[k]);
          left[k] = recon[k][3];
          upleft[k] = up[k][3];
          emit_group(g, s.pal, mode_l, row, G, recon[k], frame);
          if (l == kLanes - 1) {
            PNG_UNROLL
            for (int u = 0; u < 4; ++u) s.above[4 * G + u] = recon[k][u];
          }
        }
      }
    }
    PNG_SYNC();      // lane 63's row is the next band's row above
  }
  int status = st.status;
  if (s.bad_filter) status |= kBadFilter;
  if (st.adler_valid && adler_combine(s.sum1, s.sum2, n) != st.adler) status |= kBadAdler;
  return status;
}

}  // namespace png
}  // namespace diffsal
