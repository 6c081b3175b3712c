// The arithmetic, the tables and the buffer layout of the JPEG export (include/diffsal.h, "JPEG export"), callable from the host and
// from the device: csrc/jpeg_export.hip runs it in kernels, tools/jpeg_host_check.cpp runs the same functions and the same index
// arithmetic serially on the host, where a sanitizer can watch every buffer.  Integer work only.
#pragma once
#include <cstddef>
#include <cstdint>

#if defined(__HIPCC__)
#define JPEG_HD __host__ __device__ __forceinline__
#else
#define JPEG_HD inline
#endif

namespace diffsal {
namespace jpeg {

constexpr int kHeaderBytes = 328;             // SOI, APP0, DQT, SOF0, two DHT, SOS
constexpr int kMaxDcBits = 9 + 11;            // longest DC code + category 11
constexpr int kMaxAcBits = 16 + 10;           // longest AC code + category 10
constexpr int kMaxBlockBits = kMaxDcBits + 63 * kMaxAcBits;      // 1658: no block's code is longer
constexpr int kThreads = 256;                 // workgroup of every kernel; blocks per chunk of the offset scan
constexpr int kStuffBytes = 8;                // scan bytes per thread of the stuffing passes (two stream words)
constexpr int kStuffChunk = kThreads * kStuffBytes;
constexpr int kMaxDim = 65535;

struct QTab { uint16_t t[64]; };              // quantisation table, natural order
struct Header { uint32_t w[kHeaderBytes / 4]; };      // byte k = (w[k / 4] >> 8 (k % 4)) & 255

// ITU-T T.81: zig-zag order (Figure 5), Annex K.1 luminance table, Annex K.3 luminance DC and AC code lengths and symbols
constexpr uint8_t kZigzag[64] = {0,  1,  8,  16, 9,  2,  3,  10, 17, 24, 32, 25, 18, 11, 4,  5,  12, 19, 26, 33, 40, 48,
                                 41, 34, 27, 20, 13, 6,  7,  14, 21, 28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23,
                                 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63};
constexpr uint8_t kBaseQ[64] = {16, 11, 10, 16, 24,  40,  51,  61,  12, 12, 14, 19, 26,  58,  60,  55,  14, 13, 16, 24, 40,  57,
                                69, 56, 14, 17, 22,  29,  51,  87,  80, 62, 18, 22, 37,  56,  68,  109, 103, 77, 24, 35, 55,  64,
                                81, 104, 113, 92, 49, 64,  78,  87,  103, 121, 120, 101, 72, 92,  95,  98,  112, 100, 103, 99};
constexpr uint8_t kDcBits[16] = {0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0};
constexpr uint8_t kDcVals[12] = {0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11};
constexpr uint8_t kAcBits[16] = {0, 2, 1, 3, 3, 2, 4, 3, 5, 5, 4, 4, 0, 0, 1, 0x7D};
constexpr uint8_t kAcVals[162] = {
    0x01, 0x02, 0x03, 0x00, 0x04, 0x11, 0x05, 0x12, 0x21, 0x31, 0x41, 0x06, 0x13, 0x51, 0x61, 0x07, 0x22, 0x71, 0x14, 0x32, 0x81,
    0x91, 0xA1, 0x08, 0x23, 0x42, 0xB1, 0xC1, 0x15, 0x52, 0xD1, 0xF0, 0x24, 0x33, 0x62, 0x72, 0x82, 0x09, 0x0A, 0x16, 0x17, 0x18,
    0x19, 0x1A, 0x25, 0x26, 0x27, 0x28, 0x29, 0x2A, 0x34, 0x35, 0x36, 0x37, 0x38, 0x39, 0x3A, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48,
    0x49, 0x4A, 0x53, 0x54, 0x55, 0x56, 0x57, 0x58, 0x59, 0x5A, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6A, 0x73, 0x74, 0x75,
    0x76, 0x77, 0x78, 0x79, 0x7A, 0x83, 0x84, 0x85, 0x86, 0x87, 0x88, 0x89, 0x8A, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99,
    0x9A, 0xA2, 0xA3, 0xA4, 0xA5, 0xA6, 0xA7, 0xA8, 0xA9, 0xAA, 0xB2, 0xB3, 0xB4, 0xB5, 0xB6, 0xB7, 0xB8, 0xB9, 0xBA, 0xC2, 0xC3,
    0xC4, 0xC5, 0xC6, 0xC7, 0xC8, 0xC9, 0xCA, 0xD2, 0xD3, 0xD4, 0xD5, 0xD6, 0xD7, 0xD8, 0xD9, 0xDA, 0xE1, 0xE2, 0xE3, 0xE4, 0xE5,
    0xE6, 0xE7, 0xE8, 0xE9, 0xEA, 0xF1, 0xF2, 0xF3, 0xF4, 0xF5, 0xF6, 0xF7, 0xF8, 0xF9, 0xFA};

// symbol -> (code << 5) | length, codes handed out in order of length (Annex C); 0: the symbol has no code
struct HuffEnc {
  uint32_t ac[256];
  uint32_t dc[16];
};
constexpr HuffEnc make_huff() {
  HuffEnc e{};
  uint32_t code = 0;
  int k = 0;
  for (int len = 1; len <= 16; ++len) {
    for (int i = 0; i < kDcBits[len - 1]; ++i) e.dc[kDcVals[k++]] = (code++ << 5) | static_cast<uint32_t>(len);
    code <<= 1;
  }
  code = 0;
  k = 0;
  for (int len = 1; len <= 16; ++len) {
    for (int i = 0; i < kAcBits[len - 1]; ++i) e.ac[kAcVals[k++]] = (code++ << 5) | static_cast<uint32_t>(len);
    code <<= 1;
  }
  return e;
}

// ---- buffer sizes: every kernel's accesses stay inside these for any input ------------------------------------------------------
inline long blocks_of(int h, int w) { return static_cast<long>((h + 7) / 8) * ((w + 7) / 8); }
inline long max_scan_bytes(long nblk) { return (nblk * kMaxBlockBits + 7) / 8; }      // before stuffing
inline long capacity(int h, int w) { return kHeaderBytes + 2 * max_scan_bytes(blocks_of(h, w)) + 2 + 2; }

struct Layout {
  long nblk, words, chunks;      // per image: blocks, 32-bit words of the bit stream, chunks of the stuffing passes
  size_t coef, acbits, bitoff, total, stream, ffcount, ffoff, bytes;      // byte offsets into the workspace, and its size
};
inline Layout layout(int B, int h, int w) {
  Layout l{};
  l.nblk = blocks_of(h, w);
  const long mb = max_scan_bytes(l.nblk);
  l.words = (mb + 3) / 4;
  l.chunks = (mb + kStuffChunk - 1) / kStuffChunk;
  size_t off = 0;
  auto take = [&](size_t bytes) { const size_t r = off; off += (bytes + 15) & ~static_cast<size_t>(15); return r; };
  const size_t nb = static_cast<size_t>(B);
  l.coef = take(nb * 64 * l.nblk * 2);      // int16 [B][64][nblk]: coefficient k of every block side by side
  l.acbits = take(nb * l.nblk * 4);         // uint32 [B][nblk]: bits of a block's AC symbols
  l.bitoff = take(nb * l.nblk * 8);         // uint64 [B][nblk]: where a block's code starts
  l.total = take(nb * 8);                   // uint64 [B]: bits of the image's scan
  l.stream = take(nb * l.words * 4);        // uint32 [B][words]: the bit stream, MSB first
  l.ffcount = take(nb * l.chunks * 4);      // uint32 [B][chunks]: FF bytes of a chunk
  l.ffoff = take(nb * l.chunks * 4);        // uint32 [B][chunks]: FF bytes in front of a chunk
  l.bytes = off;
  return l;
}

// ---- tables and header (host) ---------------------------------------------------------------------------------------------------
inline QTab quant_table(int quality) {
  QTab q{};
  const int s = quality < 50 ? 5000 / quality : 200 - 2 * quality;
  for (int i = 0; i < 64; ++i) {
    const int t = (kBaseQ[i] * s + 50) / 100;
    q.t[i] = static_cast<uint16_t>(t < 1 ? 1 : t > 255 ? 255 : t);
  }
  return q;
}

inline Header make_header(int h, int w, const QTab& q) {
  uint8_t b[kHeaderBytes];
  int n = 0;
  auto put = [&](std::initializer_list<int> v) { for (int x : v) b[n++] = static_cast<uint8_t>(x); };
  put({0xFF, 0xD8, 0xFF, 0xE0, 0, 16, 'J', 'F', 'I', 'F', 0, 1, 1, 0, 0, 1, 0, 1, 0, 0});
  put({0xFF, 0xDB, 0, 67, 0});
  for (int k = 0; k < 64; ++k) b[n++] = static_cast<uint8_t>(q.t[kZigzag[k]]);
  put({0xFF, 0xC0, 0, 11, 8, h >> 8, h & 255, w >> 8, w & 255, 1, 1, 0x11, 0});
  put({0xFF, 0xC4, 0, 19 + 12, 0x00});
  for (int i = 0; i < 16; ++i) b[n++] = kDcBits[i];
  for (int i = 0; i < 12; ++i) b[n++] = kDcVals[i];
  put({0xFF, 0xC4, 0, 19 + 162, 0x10});
  for (int i = 0; i < 16; ++i) b[n++] = kAcBits[i];
  for (int i = 0; i < 162; ++i) b[n++] = kAcVals[i];
  put({0xFF, 0xDA, 0, 8, 1, 1, 0, 0, 0x3F, 0});
  Header hd{};
  for (int k = 0; k < kHeaderBytes && k < n; ++k) hd.w[k >> 2] |= static_cast<uint32_t>(b[k]) << (8 * (k & 3));
  return hd;
}

// ---- transforms: libjpeg's jfdctint / jidctint (CONST_BITS 13, PASS1_BITS 2) ---------------------------------------------------------
constexpr int kC0298 = 2446, kC0390 = 3196, kC0541 = 4433, kC0765 = 6270, kC0899 = 7373, kC1175 = 9633, kC1501 = 12299,
              kC1847 = 15137, kC1961 = 16069, kC2053 = 16819, kC2562 = 20995, kC3072 = 25172;

JPEG_HD int descale(int x, int n) { return (x + (1 << (n - 1))) >> n; }
// the same bits in wrap-around arithmetic: for the decoder, whose coefficients come from a file (jpeg_decode_core.h)
JPEG_HD uint32_t descale(uint32_t x, int n) { return static_cast<uint32_t>(static_cast<int>(x + (1u << (n - 1))) >> n); }

// one forward pass over eight values d[0], d[S], ..., d[7 S]
template <int S, bool FIRST>
JPEG_HD void fdct_pass(int* d) {
  constexpr int N = FIRST ? 11 : 15;
  const int t0 = d[0] + d[7 * S], t7 = d[0] - d[7 * S], t1 = d[S] + d[6 * S], t6 = d[S] - d[6 * S];
  const int t2 = d[2 * S] + d[5 * S], t5 = d[2 * S] - d[5 * S], t3 = d[3 * S] + d[4 * S], t4 = d[3 * S] - d[4 * S];
  const int t10 = t0 + t3, t13 = t0 - t3, t11 = t1 + t2, t12 = t1 - t2;
  d[0] = FIRST ? (t10 + t11) * 4 : descale(t10 + t11, 2);
  d[4 * S] = FIRST ? (t10 - t11) * 4 : descale(t10 - t11, 2);
  int z1 = (t12 + t13) * kC0541;
  d[2 * S] = descale(z1 + t13 * kC0765, N);
  d[6 * S] = descale(z1 - t12 * kC1847, N);
  z1 = t4 + t7;
  int z2 = t5 + t6, z3 = t4 + t6, z4 = t5 + t7;
  const int z5 = (z3 + z4) * kC1175;
  const int u4 = t4 * kC0298, u5 = t5 * kC2053, u6 = t6 * kC3072, u7 = t7 * kC1501;
  z1 *= -kC0899; z2 *= -kC2562;
  z3 = z3 * -kC1961 + z5; z4 = z4 * -kC0390 + z5;
  d[7 * S] = descale(u4 + z1 + z3, N);
  d[5 * S] = descale(u5 + z2 + z4, N);
  d[3 * S] = descale(u6 + z2 + z3, N);
  d[S] = descale(u7 + z1 + z4, N);
}

// d: 64 samples - 128 in raster order -> the quantised coefficients in natural order
JPEG_HD void fdct_quantise(int (&d)[64], const QTab& q) {
#pragma unroll
  for (int r = 0; r < 8; ++r) fdct_pass<1, true>(d + 8 * r);
#pragma unroll
  for (int c = 0; c < 8; ++c) fdct_pass<8, false>(d + c);
#pragma unroll
  for (int i = 0; i < 64; ++i) {
    const int div = 8 * q.t[i];      // the transform's output carries a factor 8
    const int v = d[i], a = ((v < 0 ? -v : v) + (div >> 1)) / div;
    d[i] = v < 0 ? -a : a;
  }
}

// T: int (the export: its own coefficients, no overflow) or uint32_t (the decoder: any coefficients, defined by wrap-around)
template <int S, int N, class T>
JPEG_HD void idct_pass(T* d) {
  T z2 = d[2 * S], z3 = d[6 * S];
  T z1 = (z2 + z3) * kC0541;
  T t2 = z1 - z3 * kC1847, t3 = z1 + z2 * kC0765;
  T t0 = (d[0] + d[4 * S]) * 8192, t1 = (d[0] - d[4 * S]) * 8192;
  const T t10 = t0 + t3, t13 = t0 - t3, t11 = t1 + t2, t12 = t1 - t2;
  t0 = d[7 * S]; t1 = d[5 * S]; t2 = d[3 * S]; t3 = d[S];
  z1 = t0 + t3; z2 = t1 + t2; z3 = t0 + t2;
  T z4 = t1 + t3;
  const T z5 = (z3 + z4) * kC1175;
  t0 *= kC0298; t1 *= kC2053; t2 *= kC3072; t3 *= kC1501;
  z1 *= -kC0899; z2 *= -kC2562;
  z3 = z3 * -kC1961 + z5; z4 = z4 * -kC0390 + z5;
  t0 += z1 + z3; t1 += z2 + z4; t2 += z2 + z3; t3 += z1 + z4;
  d[0] = descale(t10 + t3, N); d[7 * S] = descale(t10 - t3, N);
  d[S] = descale(t11 + t2, N); d[6 * S] = descale(t11 - t2, N);
  d[2 * S] = descale(t12 + t1, N); d[5 * S] = descale(t12 - t1, N);
  d[3 * S] = descale(t13 + t0, N); d[4 * S] = descale(t13 - t0, N);
}

// libjpeg's range limit after the inverse transform: x + 128 clamped to 0..255, read from a table indexed by the low 10 bits of x
JPEG_HD int range_limit(int x) {
  const int v = x & 1023;
  return v < 128 ? v + 128 : v < 512 ? 255 : v < 896 ? 0 : v - 896;
}

// d: the quantised coefficients in natural order -> the 64 pixels a libjpeg decoder returns, in raster order
template <class T>
JPEG_HD void dequantise_idct(T (&d)[64], const QTab& q) {
#pragma unroll
  for (int i = 0; i < 64; ++i) d[i] *= q.t[i];
#pragma unroll
  for (int c = 0; c < 8; ++c) idct_pass<8, 11>(d + c);
#pragma unroll
  for (int r = 0; r < 8; ++r) idct_pass<1, 18>(d + 8 * r);
#pragma unroll
  for (int i = 0; i < 64; ++i) d[i] = range_limit(static_cast<int>(d[i]));
}

// ---- entropy coding ------------------------------------------------------------------------------------------------------------------
// the category of v, capped at `cap`.  An 8-bit image never reaches the cap (DC differences have at most 11 bits, AC coefficients
// 10); the cap makes kMaxBlockBits hold for any bytes, so no buffer size rests on a property of the input
JPEG_HD int category(int v, int cap) {
  const unsigned a = static_cast<unsigned>(v < 0 ? -v : v);
  const int n = a ? 32 - __builtin_clz(a) : 0;
  return n < cap ? n : cap;
}
// Huffman code of `sym` followed by the low n bits of v (v - 1 for a negative v): emit(bits, count), count <= 26
template <class Emit>
JPEG_HD void put_symbol(uint32_t entry, int v, int n, Emit& emit) {
  const uint32_t val = static_cast<uint32_t>(v < 0 ? v - 1 : v) & ((1u << n) - 1u);
  emit(((entry >> 5) << n) | val, static_cast<int>(entry & 31u) + n);
}
template <class Emit>
JPEG_HD void put_dc(int diff, const uint32_t* dc, Emit& emit) {
  const int n = category(diff, 11);
  put_symbol(dc[n], diff, n, emit);
}
// the AC symbols of one block: get(k) = coefficient k of the zig-zag order, k = 1..63
template <class Get, class Emit>
JPEG_HD void put_ac(Get get, const uint32_t* ac, Emit& emit) {
  int run = 0;
  for (int k = 1; k < 64; ++k) {
    const int v = get(k);
    if (v == 0) { ++run; continue; }
    for (; run > 15; run -= 16) emit(ac[0xF0] >> 5, static_cast<int>(ac[0xF0] & 31u));      // ZRL
    const int n = category(v, 10);
    put_symbol(ac[(run << 4) | n], v, n, emit);
    run = 0;
  }
  if (run) emit(ac[0] >> 5, static_cast<int>(ac[0] & 31u));      // EOB
}

// The bit stream is an array of 32-bit words, bit p of the stream in word p / 32 at bit 31 - p % 32.  A block's code is written
// through a 64-bit window over words wi and wi + 1; `store(wi, word)` ORs a finished word into the stream.
template <class Store>
struct BitWriter {
  Store& store;
  uint64_t win;
  long wi;
  int fill;
  JPEG_HD BitWriter(Store& s, uint64_t bit_offset) : store(s), win(0), wi(static_cast<long>(bit_offset >> 5)), fill(static_cast<int>(bit_offset & 31u)) {}
  JPEG_HD void operator()(uint32_t bits, int n) {      // n <= 26, fill <= 31: the window holds them
    if (n == 0) return;
    win |= static_cast<uint64_t>(bits) << (64 - fill - n);
    fill += n;
    if (fill >= 32) {
      store(wi, static_cast<uint32_t>(win >> 32));
      win <<= 32;
      fill -= 32;
      ++wi;
    }
  }
  JPEG_HD void finish() {
    if (fill > 0) store(wi, static_cast<uint32_t>(win >> 32));
  }
};

// byte i of an image's scan before stuffing: from the stream, the last byte filled with 1-bits
JPEG_HD uint32_t scan_byte(uint32_t word, long i, long nbytes, uint64_t total_bits) {
  uint32_t v = (word >> (24 - 8 * static_cast<int>(i & 3))) & 255u;
  if (i == nbytes - 1) v |= (1u << static_cast<int>(8 * static_cast<uint64_t>(nbytes) - total_bits)) - 1u;
  return v;
}

}  // namespace jpeg
}  // namespace diffsal
