// The arithmetic, the tables and the buffer layout of the PNG export (include/diffsal.h, "PNG export"), callable from the host and
// from the device: csrc/png_encode.hip runs it in kernels, tools/png_encode_host_check.cpp runs the same functions and the same
// index arithmetic serially on the host, one loop trip per device thread, where a sanitizer can watch every buffer.
// tests/_png_encode_ref.py restates the file in NumPy.  Integer work only: the file's bytes are a function of the pixels.
#pragma once
#include <cstddef>
#include <cstdint>

#if defined(__HIPCC__)
// forced for the reason csrc/png_decode_core.h records at PNG_DEV: the kernels must hold no call
#define PNGE_HD __host__ __device__ __forceinline__
#else
#define PNGE_HD inline
#endif

namespace diffsal {
namespace pnge {

constexpr int kThreads = 256;                   // workgroup of the segment, frame, pack and crc kernels
constexpr int kRowLanes = 64;                   // the filter kernel: a wave per row
constexpr int kSegment = 16384;                 // stream bytes per deflate block
constexpr int kChunk = kSegment / kThreads;     // 64 stream positions per thread of a segment
constexpr int kMaxB = 65535, kMaxH = 65535, kMaxW = 8192;
constexpr int kLit = 286, kClen = 19, kLens = 287;      // literal/length symbols; code-length symbols; lengths sent at most (286 + 1)
// BFINAL, BTYPE; HLIT, HDIST, HCLEN; 19 code-length lengths; at most 287 code-length symbols of at most 7 + 7 bits
constexpr int kMaxHeaderBits = 3 + 14 + 3 * kClen + 14 * kLens;      // 4092
constexpr int kHeaderWords = 128;               // 4096 bits
constexpr int kFront = 43;                      // signature 8, IHDR 25, IDAT length and type 8, zlib header 2
constexpr int kFraming = kFront + 4 + 4 + 12;   // + Adler-32, IDAT's CRC, IEND = 63 = 57 + the six bytes of zlib's framing
constexpr uint32_t kAdlerMod = 65521;
constexpr uint32_t kNone = 0xFFFFu;             // token record: 0..255 a literal, 256 + length a match, kNone inside a match

// ---- sizes: every kernel's accesses stay inside these for any pixels -------------------------------------------------------------
inline bool shape_ok(int B, int H, int W) { return B >= 1 && B <= kMaxB && H >= 1 && H <= kMaxH && W >= 1 && W <= kMaxW; }
inline long stream_bytes(int H, int W) { return static_cast<long>(H) * (W + 1); }
inline long segments_of(int H, int W) { return (stream_bytes(H, W) + kSegment - 1) / kSegment; }
// a token covers at least one stream byte per 15 bits (a literal: 15; a match: 15 + 5 + 1 for three bytes or more); a block adds
// its header and an end symbol of at most 15 bits
inline long max_deflate_bytes(int H, int W) { return (15 * stream_bytes(H, W) + (kMaxHeaderBits + 15) * segments_of(H, W) + 7) / 8; }
inline long capacity(int H, int W) { return (kFraming + max_deflate_bytes(H, W) + 15) & ~15L; }      // below 2^31 for every shape taken

struct SegInfo { uint32_t header_bits, total_bits, adler_a, adler_b; };
struct Layout {
  long S, nseg, region;      // per image: stream bytes, segments, stream bytes padded to whole chunks
  size_t filt, tok, chunkoff, code, header, info, segoff, bits, bytes;      // byte offsets into the workspace, and its size
};
inline Layout layout(int B, int H, int W) {
  Layout l{};
  l.S = stream_bytes(H, W);
  l.nseg = segments_of(H, W);
  l.region = (l.S + kChunk - 1) / kChunk * kChunk;
  size_t off = 0;
  auto take = [&](size_t bytes) { const size_t r = off; off += (bytes + 15) & ~static_cast<size_t>(15); return r; };
  const size_t nb = static_cast<size_t>(B), ns = nb * static_cast<size_t>(l.nseg);
  l.filt = take(nb * l.region);                  // uint8 [B][region]: the filtered scanlines
  l.tok = take(nb * l.region * 2);               // uint16 [B][region]: the token that starts at a position
  l.chunkoff = take(ns * kThreads * 4);          // uint32 [B][nseg][256]: bit offset of a chunk's tokens in its block
  l.code = take(ns * 288 * 4);                   // uint32 [B][nseg][288]: literal/length symbol -> (reversed code << 4) | length
  l.header = take(ns * kHeaderWords * 4);        // uint32 [B][nseg][128]: the block header's bits
  l.info = take(ns * sizeof(SegInfo));
  l.segoff = take(ns * 8);                       // uint64 [B][nseg]: where a block starts in the deflate stream
  l.bits = take(nb * 8);                         // uint64 [B]: bits of the deflate stream
  l.bytes = off;
  return l;
}

// ---- filters (PNG 9.2) on raw neighbours ----------------------------------------------------------------------------------------
PNGE_HD int paeth(int a, int b, int c) {
  const int p = a + b - c;
  const int pa = p > a ? p - a : a - p, pb = p > b ? p - b : b - p, pc = p > c ? p - c : c - p;
  return pa <= pb && pa <= pc ? a : pb <= pc ? b : c;
}
PNGE_HD uint32_t filter_byte(int f, int x, int a, int b, int c) {
  const int pred = f == 1 ? a : f == 2 ? b : f == 3 ? (a + b) >> 1 : f == 4 ? paeth(a, b, c) : 0;
  return static_cast<uint32_t>(x - pred) & 255u;
}
PNGE_HD uint32_t filter_cost(uint32_t v) { return v < 128u ? v : 256u - v; }
// pixel x of `row` and its neighbours; up: the row above or nullptr
PNGE_HD void neighbours(const uint8_t* row, const uint8_t* up, int x, int& v, int& a, int& b, int& c) {
  v = row[x];
  a = x ? row[x - 1] : 0;
  b = up ? up[x] : 0;
  c = up && x ? up[x - 1] : 0;
}
// the least of five costs, a tie to the lowest filter
PNGE_HD int choose_filter(const uint32_t cost[5]) {
  int f = 0;
  for (int k = 1; k < 5; ++k)
    if (cost[k] < cost[f]) f = k;
  return f;
}

// ---- tokens: distance 1 only.  A thread holds kChunk positions of its segment --------------------------------------------------------
struct ChunkRegs {
  uint32_t w[kChunk / 4];      // the bytes, four to a word
  uint64_t eq, valid;          // bit j: position base + j equals the stream byte in front of it; the position exists
  int base, nv;                // first position in the segment; positions held
  int last_ne, first_ne;       // the last / first position of the chunk that differs from the byte in front of it; -1 / n if none
  uint32_t s1, s2;             // Adler partials: sum of bytes; sum of (n - position) * byte, below 2^32
};
// chunk t of the segment at `seg` (n bytes; at: its first byte's position in the stream; seg is 16-byte aligned, whole chunks readable)
PNGE_HD void load_chunk(const uint8_t* seg, long at, int n, int t, ChunkRegs& r) {
  r.base = t * kChunk;
  r.nv = n - r.base < 0 ? 0 : n - r.base > kChunk ? kChunk : n - r.base;
  r.eq = 0;
  r.valid = r.nv == kChunk ? ~0ull : (1ull << r.nv) - 1ull;
  r.last_ne = -1; r.first_ne = n; r.s1 = 0; r.s2 = 0;
  if (!r.nv) return;
  __builtin_memcpy(r.w, __builtin_assume_aligned(seg + r.base, 16), kChunk);
  uint32_t prev = at + r.base > 0 ? seg[r.base - 1] : 256u;      // nothing stands in front of the stream's first byte
  for (int j = 0; j < kChunk; ++j) {
    const uint32_t v = (r.w[j >> 2] >> (8 * (j & 3))) & 255u;
    if (j < r.nv) {
      if (v == prev) r.eq |= 1ull << j;
      r.s1 += v;
      r.s2 += static_cast<uint32_t>(n - r.base - j) * v;
    }
    prev = v;
  }
  const uint64_t ne = ~r.eq & r.valid;
  if (ne) {
    r.last_ne = r.base + 63 - __builtin_clzll(ne);
    r.first_ne = r.base + __builtin_ctzll(ne);
  }
}
// the token record of position base + j (j < nv).  before: the last differing position in front of the chunk (-1: none);
// after: the first one behind it (n: none)
PNGE_HD uint32_t token_at(const ChunkRegs& r, int j, int before, int after) {
  const uint32_t v = (r.w[j >> 2] >> (8 * (j & 3))) & 255u;
  if (!((r.eq >> j) & 1ull)) return v;
  const uint64_t ne = ~r.eq & r.valid;
  const uint64_t lo = ne & ((2ull << j) - 1ull), hi = ne >> j;      // j = 63: 2 << 63 wraps to 0, the mask to all ones
  const int s = (lo ? r.base + 63 - __builtin_clzll(lo) : before) + 1;      // the run's first position
  const int e = hi ? r.base + j + __builtin_ctzll(hi) : after;              // behind its last
  const int L = e - s, o = r.base + j - s, k = o / 258;
  const int rem = L - 258 * k;      // what is left of the run where this piece starts
  if (L < 3 || rem < 3) return v;
  return o - 258 * k ? kNone : 256u + static_cast<uint32_t>(rem < 258 ? rem : 258);
}
// match length 3..258 -> symbol, extra bits and their value
PNGE_HD int length_symbol(int length, int& eb, int& ev) {
  eb = 0; ev = 0;
  if (length == 258) return 285;
  if (length < 11) return 254 + length;
  const int v = length - 3;
  eb = 29 - __builtin_clz(static_cast<unsigned>(v));
  ev = v & ((1 << eb) - 1);
  return 257 + 4 * eb + (v >> eb);
}
// token record -> its symbol
PNGE_HD int token_symbol(uint32_t tok, int& eb, int& ev) {
  eb = 0; ev = 0;
  return tok < 256u ? static_cast<int>(tok) : length_symbol(static_cast<int>(tok) - 256, eb, ev);
}
// bits of the token under `code`: its code, its extra bits, and for a match the distance code (symbol 0: one bit)
PNGE_HD uint32_t token_bits(uint32_t tok, const uint32_t* code) {
  int eb, ev;
  const int sym = token_symbol(tok, eb, ev);
  return (code[sym] & 15u) + static_cast<uint32_t>(eb) + (tok >= 256u ? 1u : 0u);
}

// ---- length-limited canonical codes -------------------------------------------------------------------------------------------------
// Symbols with a count take part, and symbols 0 and 1 as well if fewer than two have one.  Order: ascending (count, symbol).
PNGE_HD bool takes_part(const uint32_t* count, int nonzero, int i) { return count[i] > 0 || (nonzero < 2 && i < 2); }
PNGE_HD int rank_of(const uint32_t* count, int n, int nonzero, int i) {
  int r = 0;
  for (int j = 0; j < n; ++j)
    if (takes_part(count, nonzero, j) && (count[j] < count[i] || (count[j] == count[i] && j < i))) ++r;
  return r;
}
struct CodeScratch {
  uint32_t w[2 * 288];
  uint16_t parent[2 * 288], depth[2 * 288], order[288], num[290];
};
// order[0, m): the symbols that take part, ascending.  Huffman's tree by the two-queue method, a leaf before an internal node of
// equal weight; the count of codes per length; lengths above `limit` folded into it and the Kraft sum repaired by moving the
// deepest code that can move one level down (miniz's rule: each round takes exactly one unit of 2^-limit off the sum, and a code
// above the limit's level exists while the sum is too large, since m <= 2^limit); then the lengths go out along the order, the
// longest to the rarest.  The result is complete: Kraft sum exactly 1.  Returns whether the limit changed anything
PNGE_HD bool build_lengths(const uint32_t* count, int n, int m, int limit, CodeScratch& s, uint8_t* lens) {
  for (int k = 0; k < m; ++k) s.w[k] = count[s.order[k]];
  int leaf = 0, inner = m;
  for (int node = m; node < 2 * m - 1; ++node) {
    s.w[node] = 0;
    for (int t = 0; t < 2; ++t) {
      int k;
      if (leaf < m && (inner >= node || s.w[leaf] <= s.w[inner])) k = leaf++;
      else k = inner++;
      s.w[node] += s.w[k];
      s.parent[k] = static_cast<uint16_t>(node);
    }
  }
  for (int i = 0; i < 290; ++i) s.num[i] = 0;
  s.depth[2 * m - 2] = 0;
  int deepest = 0;
  for (int node = 2 * m - 3; node >= 0; --node) {
    s.depth[node] = static_cast<uint16_t>(s.depth[s.parent[node]] + 1);
    if (node < m) {
      ++s.num[s.depth[node]];      // at most m - 1 <= 285
      if (s.depth[node] > deepest) deepest = s.depth[node];
    }
  }
  const bool limited = deepest > limit;
  if (limited) {
    for (int i = limit + 1; i < 290; ++i) { s.num[limit] = static_cast<uint16_t>(s.num[limit] + s.num[i]); s.num[i] = 0; }
    uint32_t total = 0;
    for (int i = 1; i <= limit; ++i) total += static_cast<uint32_t>(s.num[i]) << (limit - i);
    while (total != (1u << limit)) {      // at most m rounds
      --s.num[limit];
      for (int i = limit - 1; i > 0; --i)
        if (s.num[i]) { --s.num[i]; s.num[i + 1] = static_cast<uint16_t>(s.num[i + 1] + 2); break; }
      --total;
    }
  }
  for (int i = 0; i < n; ++i) lens[i] = 0;
  int r = 0;
  for (int length = limit; length > 0; --length)
    for (int c = 0; c < s.num[length] && r < m; ++c) lens[s.order[r++]] = static_cast<uint8_t>(length);
  return limited;
}
// RFC 1951 3.2.2: symbol -> (its code, bit-reversed: the stream takes a code's first bit first) << 4 | its length
PNGE_HD void canonical(const uint8_t* lens, int n, uint32_t* code) {
  uint32_t count[16], next[16];
  for (int b = 0; b < 16; ++b) count[b] = 0;
  for (int i = 0; i < n; ++i) ++count[lens[i]];
  count[0] = 0;
  uint32_t c = 0;
  next[0] = 0;
  for (int b = 1; b < 16; ++b) { c = (c + count[b - 1]) << 1; next[b] = c; }
  for (int i = 0; i < n; ++i) {
    const int len = lens[i];
    uint32_t rev = 0;
    if (len) {
      uint32_t v = next[len]++;      // below 2^15: reversed as 16 bits, then the low len bits of that
      v = ((v >> 1) & 0x5555u) | ((v & 0x5555u) << 1);
      v = ((v >> 2) & 0x3333u) | ((v & 0x3333u) << 2);
      v = ((v >> 4) & 0x0F0Fu) | ((v & 0x0F0Fu) << 4);
      v = ((v >> 8) & 0x00FFu) | ((v & 0x00FFu) << 8);
      rev = v >> (16 - len);
    }
    code[i] = (rev << 4) | static_cast<uint32_t>(len);
  }
}
// The code lengths seq[0, n) as code-length symbols: a run of zeros in pieces of 138 (symbol 18) while 11 or more are left, then 17
// for 3..10, else zeros; another value once, then 16 in pieces of 6 while 3 or more are left, then the value.  Returns how many
// symbols (at most n); ext: the value of a symbol's extra bits
PNGE_HD int run_lengths(const uint8_t* seq, int n, uint8_t* sym, uint8_t* ext) {
  int out = 0, i = 0;
  while (i < n) {
    const uint8_t v = seq[i];
    int j = i;
    while (j < n && seq[j] == v) ++j;
    int L = j - i;
    i = j;
    if (v == 0) {
      while (L >= 11) { const int c = L < 138 ? L : 138; sym[out] = 18; ext[out++] = static_cast<uint8_t>(c - 11); L -= c; }
      if (L >= 3) { sym[out] = 17; ext[out++] = static_cast<uint8_t>(L - 3); L = 0; }
    } else {
      sym[out] = v; ext[out++] = 0;
      --L;
      while (L >= 3) { const int c = L < 6 ? L : 6; sym[out] = 16; ext[out++] = static_cast<uint8_t>(c - 3); L -= c; }
    }
    for (; L > 0; --L) { sym[out] = v; ext[out++] = 0; }
  }
  return out;
}
PNGE_HD int clen_order(int i) { return i < 3 ? 16 + i : i == 3 ? 0 : (i & 1) ? 7 - (i - 5) / 2 : 8 + (i - 4) / 2; }      // 16 17 18 0 8 7 9 6 10 5 11 4 12 3 13 2 14 1 15
// nb <= 14 bits of v at bit `pos` of words (zeroed before), least significant first
PNGE_HD void put_bits(uint32_t* words, uint32_t& pos, uint32_t v, int nb) {
  const uint32_t i = pos >> 5, sh = pos & 31u;
  words[i] |= v << sh;
  if (sh + static_cast<uint32_t>(nb) > 32u) words[i + 1] |= v >> (32u - sh);      // pos + nb <= 4092: i + 1 <= 127
  pos += static_cast<uint32_t>(nb);
}

// what a segment's workgroup shares (LDS on the device)
struct BlockShared {
  uint32_t hist[288];      // symbol counts
  uint32_t code[288];      // (reversed code << 4) | length
  uint32_t header[kHeaderWords];
  uint32_t chist[kClen], ccode[kClen];
  CodeScratch cs;
  uint8_t lens[288], clens[kClen], rsym[288], rext[288];
  uint32_t header_bits, nonzero, m, adler_a, adler_b;
  uint32_t scan[kThreads];
  int ne_last[kThreads], ne_first[kThreads];
};
// One thread's serial part of a block, after hist is complete and cs.order[0, m) holds the symbols that take part: the
// literal/length code, the lengths' run-length form, the code-length code, the header's bits.  ~3000 steps
PNGE_HD void build_block(BlockShared& s, bool final) {
  build_lengths(s.hist, kLit, static_cast<int>(s.m), 15, s.cs, s.lens);
  canonical(s.lens, kLit, s.code);
  int nlen = kLit;
  while (nlen > 257 && !s.lens[nlen - 1]) --nlen;
  s.lens[nlen] = 1;      // the distance code: symbol 0 alone, one bit; sent behind the literal/length lengths as one sequence
  const int nr = run_lengths(s.lens, nlen + 1, s.rsym, s.rext);
  s.lens[nlen] = 0;
  for (int i = 0; i < kClen; ++i) s.chist[i] = 0;
  for (int i = 0; i < nr; ++i) ++s.chist[s.rsym[i]];
  int nonzero = 0, m = 0;
  for (int i = 0; i < kClen; ++i) nonzero += s.chist[i] > 0;
  for (int i = 0; i < kClen; ++i)
    if (takes_part(s.chist, nonzero, i)) { s.cs.order[rank_of(s.chist, kClen, nonzero, i)] = static_cast<uint16_t>(i); ++m; }
  build_lengths(s.chist, kClen, m, 7, s.cs, s.clens);
  canonical(s.clens, kClen, s.ccode);
  int ncl = kClen;
  while (ncl > 4 && !s.clens[clen_order(ncl - 1)]) --ncl;
  for (int i = 0; i < kHeaderWords; ++i) s.header[i] = 0;
  uint32_t pos = 0;
  put_bits(s.header, pos, final ? 1u : 0u, 1);
  put_bits(s.header, pos, 2u, 2);
  put_bits(s.header, pos, static_cast<uint32_t>(nlen - 257), 5);
  put_bits(s.header, pos, 0u, 5);
  put_bits(s.header, pos, static_cast<uint32_t>(ncl - 4), 4);
  for (int i = 0; i < ncl; ++i) put_bits(s.header, pos, s.clens[clen_order(i)], 3);
  for (int i = 0; i < nr; ++i) {
    const int sy = s.rsym[i], len = static_cast<int>(s.ccode[sy] & 15u), eb = sy == 16 ? 2 : sy == 17 ? 3 : sy == 18 ? 7 : 0;
    put_bits(s.header, pos, (s.ccode[sy] >> 4) | (static_cast<uint32_t>(s.rext[i]) << len), len + eb);
  }
  s.header_bits = pos;
}

// ---- the bit stream: least significant bit first, 32-bit little-endian words; store(word index, bits) ORs ----------------------------
template <class Store>
struct BitWriter {
  Store& store;
  long word;
  uint64_t buf;
  int cnt;
  PNGE_HD BitWriter(Store& st, unsigned long long bit) : store(st), word(static_cast<long>(bit >> 5)), buf(0), cnt(static_cast<int>(bit & 31u)) {}
  PNGE_HD void put(uint32_t v, int nb) {      // nb <= 32
    buf |= static_cast<uint64_t>(v) << cnt;
    cnt += nb;
    if (cnt >= 32) { store(word++, static_cast<uint32_t>(buf)); buf >>= 32; cnt -= 32; }
  }
  PNGE_HD void finish() { if (cnt) store(word, static_cast<uint32_t>(buf)); }
};
template <class Store>
PNGE_HD void put_token(BitWriter<Store>& out, uint32_t tok, const uint32_t* code) {
  int eb, ev;
  const int sym = token_symbol(tok, eb, ev);
  const int len = static_cast<int>(code[sym] & 15u);
  out.put((code[sym] >> 4) | (static_cast<uint32_t>(ev) << len), len + eb);
  if (tok >= 256u) out.put(0u, 1);      // distance 1
}

// ---- CRC-32 (PNG annex D), reflected, polynomial EDB88320 ---------------------------------------------------------------------------
constexpr uint32_t kCrcPoly = 0xEDB88320u;
struct CrcTables {
  uint32_t byte[256];      // the usual table
  uint32_t x2n[32];        // x^(2^k) mod P
};
constexpr uint32_t crc_mul(uint32_t a, uint32_t b) {      // a * b mod P, x^0 = bit 31
  uint32_t p = 0;
  for (int i = 0; i < 32; ++i) {
    if (a & (0x80000000u >> i)) p ^= b;
    b = (b & 1u) ? (b >> 1) ^ kCrcPoly : b >> 1;
  }
  return p;
}
constexpr CrcTables make_crc_tables() {
  CrcTables t{};
  for (uint32_t n = 0; n < 256; ++n) {
    uint32_t c = n;
    for (int k = 0; k < 8; ++k) c = (c & 1u) ? kCrcPoly ^ (c >> 1) : c >> 1;
    t.byte[n] = c;
  }
  uint32_t p = 0x40000000u;      // x^1
  for (int k = 0; k < 32; ++k) { t.x2n[k] = p; p = crc_mul(p, p); }
  return t;
}
// x^(8 n) mod P
PNGE_HD uint32_t crc_x8n(const uint32_t* x2n, unsigned long long n) {
  uint32_t p = 0x80000000u;
  for (int k = 3; n; n >>= 1, ++k)
    if (n & 1ull) p = crc_mul(x2n[k & 31], p);
  return p;
}
// the CRC of bytes [p, p + n), as a file carries it
PNGE_HD uint32_t crc_bytes(const uint32_t* table, const uint8_t* p, int n) {
  uint32_t c = 0xFFFFFFFFu;
  for (int i = 0; i < n; ++i) c = table[(c ^ p[i]) & 255u] ^ (c >> 8);
  return c ^ 0xFFFFFFFFu;
}
// crc(A B) = crc(A) * x^(8 |B|) + crc(B): the contribution of a piece that `after` bytes follow
PNGE_HD uint32_t crc_shift(const uint32_t* x2n, uint32_t crc, unsigned long long after) { return crc_mul(crc_x8n(x2n, after), crc); }

// ---- framing ------------------------------------------------------------------------------------------------------------------------
struct Front { uint8_t b[33]; };      // the signature and IHDR with its CRC: the same for every image of a call
inline Front make_front(int H, int W) {
  constexpr CrcTables t = make_crc_tables();
  Front f{{0x89, 'P', 'N', 'G', 13, 10, 26, 10, 0, 0, 0, 13, 'I', 'H', 'D', 'R'}};
  for (int k = 0; k < 4; ++k) {
    f.b[16 + k] = static_cast<uint8_t>(static_cast<uint32_t>(W) >> (24 - 8 * k));
    f.b[20 + k] = static_cast<uint8_t>(static_cast<uint32_t>(H) >> (24 - 8 * k));
  }
  f.b[24] = 8;      // depth 8, colour type 0, compression 0, filter 0, interlace 0
  for (int k = 25; k < 29; ++k) f.b[k] = 0;
  const uint32_t c = crc_bytes(t.byte, f.b + 12, 17);
  for (int k = 0; k < 4; ++k) f.b[29 + k] = static_cast<uint8_t>(c >> (24 - 8 * k));
  return f;
}
PNGE_HD void put_be32(uint8_t* p, uint32_t v) {
  p[0] = static_cast<uint8_t>(v >> 24); p[1] = static_cast<uint8_t>(v >> 16); p[2] = static_cast<uint8_t>(v >> 8); p[3] = static_cast<uint8_t>(v);
}
// Everything of image row `out` but the deflate stream and IDAT's CRC, once the stream has `bits` bits; returns the file's length
PNGE_HD int write_frame(uint8_t* out, const Front& f, unsigned long long bits, uint32_t adler) {
  const long nb = static_cast<long>((bits + 7) >> 3);
  for (int k = 0; k < 33; ++k) out[k] = f.b[k];
  put_be32(out + 33, static_cast<uint32_t>(nb + 6));
  out[37] = 'I'; out[38] = 'D'; out[39] = 'A'; out[40] = 'T';
  out[41] = 0x78; out[42] = 0x01;
  uint8_t* p = out + kFront + nb;
  put_be32(p, adler);
  put_be32(p + 8, 0);
  p[12] = 'I'; p[13] = 'E'; p[14] = 'N'; p[15] = 'D';
  put_be32(p + 16, 0xAE426082u);
  return static_cast<int>(kFraming + nb);
}

}  // namespace pnge
}  // namespace diffsal
