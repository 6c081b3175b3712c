// The arithmetic, the tables and the buffer layout of the JPEG decode (include/diffsal.h, "JPEG decode"), callable from the host
// and from the device: csrc/jpeg_decode.hip runs it in kernels, tools/jpeg_decode_host_check.cpp runs the same functions and the
// same index arithmetic serially on the host, where a sanitizer can watch every buffer.  Integer work only.  The inverse DCT and
// the range limit are jpeg_core.h's, instantiated for uint32_t: the coefficients come from a file, so every overflow must be
// defined, and wrap-around gives the bits of the int version wherever that one does not overflow.
//
// Nothing here trusts the file's bytes or the descriptor's numbers: selectors are masked, byte ranges and MCU counts are clamped
// to the buffers by the callers, every loop has a bound that is a constant or comes from the geometry.
#pragma once
#include "jpeg_core.h"

namespace diffsal {
namespace jpeg {

constexpr int kStatusBadCode = 1;       // a bit pattern no Huffman code of the table matches, or a DC category above 15
constexpr int kStatusBadIndex = 2;      // a run that carries the coefficient index past 63
constexpr int kStatusNoBits = 4;        // the segment ended before its MCUs did
constexpr int kSegThreads = 64;         // workgroup of the entropy kernel: one wave, a lane per restart segment
constexpr int kRowPixels = 16;          // output pixels of a lane of the colour kernel

// what the host parser uploads per file (1392 bytes; the same layout as the NumPy record of diff_sal_amd/jpeg.py)
struct FileDesc {
  uint32_t scan_off, scan_len;      // the entropy-coded bytes in the packed buffer (the kernels read the segments, not these)
  uint32_t restart;                 // MCUs per restart interval, 0: none
  uint32_t seg0, nseg;              // the file's rows of the segment table
  uint32_t pad[3];
  uint8_t comp[4][4];               // per component: quantisation table, DC table, AC table, 0
  uint8_t qt[4][64];                // quantisation tables 0..3, natural order
  uint8_t hbits[4][16];             // Huffman tables DC 0, DC 1, AC 0, AC 1: codes per length 1..16
  uint8_t hvals[4][256];            //                                        the symbols in code order
};
static_assert(sizeof(FileDesc) == 1392, "FileDesc layout");
struct Segment { int32_t file, begin, end, first_mcu; };      // bytes [begin, end) of the packed buffer, without the RSTn marker

struct Geom {
  int N, H, W, ncomp, hs, vs;      // hs x vs: the luma sampling factors (chroma is 1 x 1)
  int mcux, mcuy, mcus;
  int bw[3], bh[3];                // blocks per row and per column of a component, MCU padding included
  int cw, ch;                      // a chroma plane's real size: ceil(W / hs), ceil(H / vs)
  long boff[3], nblk;              // first block of a component among a file's blocks; blocks per file
  long poff[3], plane;             // byte offset of a component's plane among a file's planes; their bytes per file
  size_t status, coef, planes, clear, bytes;      // byte offsets into the workspace; [0, clear) is zeroed per call; its size
};
inline bool geom_ok(int N, int H, int W, int ncomp, int hs, int vs) {
  return N >= 1 && N <= 65535 && H >= 1 && H <= kMaxDim && W >= 1 && W <= kMaxDim && (ncomp == 1 || ncomp == 3) &&
         ((hs == 1 && vs == 1) || (ncomp == 3 && hs == 2 && (vs == 1 || vs == 2)));
}
inline Geom geom(int N, int H, int W, int ncomp, int hs, int vs) {
  Geom g{};
  g.N = N; g.H = H; g.W = W; g.ncomp = ncomp; g.hs = hs; g.vs = vs;
  g.mcux = (W + 8 * hs - 1) / (8 * hs);
  g.mcuy = (H + 8 * vs - 1) / (8 * vs);
  g.mcus = g.mcux * g.mcuy;      // <= 8192 * 8192
  g.cw = (W + hs - 1) / hs;
  g.ch = (H + vs - 1) / vs;
  for (int c = 0; c < ncomp; ++c) {
    g.bw[c] = g.mcux * (c ? 1 : hs);
    g.bh[c] = g.mcuy * (c ? 1 : vs);
    g.boff[c] = g.nblk;
    g.poff[c] = g.plane;
    g.nblk += static_cast<long>(g.bw[c]) * g.bh[c];
    g.plane += static_cast<long>(g.bw[c]) * g.bh[c] * 64;
  }
  size_t off = 0;
  auto take = [&](size_t bytes) { const size_t r = off; off += (bytes + 15) & ~static_cast<size_t>(15); return r; };
  g.status = take(static_cast<size_t>(N) * 4);                    // int32 [N]
  g.coef = take(static_cast<size_t>(N) * g.nblk * 64 * 2);        // int16 [N][nblk][64], natural order
  g.clear = off;
  g.planes = take(static_cast<size_t>(N) * g.plane);              // uint8 [N][component][8 bh][8 bw]
  g.bytes = off;
  return g;
}

// ---- Huffman tables: a first-level look-up on the next 9 bits, maxcode / valptr for the longer codes (T.81 F.2.2.3) ------------------
struct HuffDec {
  uint16_t look[512];      // (length << 8) | symbol, 0: no code of at most 9 bits
  int32_t maxcode[17];     // the largest code of a length, -1: none
  int32_t valoff[17];      // symbol index of code c of a length: valoff + c
  uint8_t vals[256];
};
// codes are handed out in order of length (Annex C).  Counts that no valid table has (more than 256 symbols, more codes than a length
// holds) are clamped where they would leave the arrays
JPEG_HD void build_huff(HuffDec& h, const uint8_t* bits, const uint8_t* vals) {
  for (int i = 0; i < 512; ++i) h.look[i] = 0;
  for (int i = 0; i < 256; ++i) h.vals[i] = vals[i];
  uint32_t code = 0;      // at most 256 increments and 16 doublings: below 2^25
  int k = 0;
  h.maxcode[0] = -1;
  h.valoff[0] = 0;
  for (int len = 1; len <= 16; ++len) {
    h.valoff[len] = k - static_cast<int>(code);
    const int n = bits[len - 1];
    for (int i = 0; i < n && k < 256; ++i, ++k, ++code) {
      if (len <= 9) {
        const uint32_t base = code << (9 - len);
        for (uint32_t j = 0; j < (1u << (9 - len)); ++j)
          if (base + j < 512u) h.look[base + j] = static_cast<uint16_t>((len << 8) | vals[k]);
      }
    }
    h.maxcode[len] = n ? static_cast<int>(code) - 1 : -1;
    code <<= 1;
  }
}

// ---- the bits of one segment ---------------------------------------------------------------------------------------------------------
// The packed buffer is read as aligned 32-bit words (its size is a multiple of 4), one load per four bytes.  FF 00 is the byte FF;
// FF in front of anything else, or as the last byte, ends the segment's data.  Behind the end the reader yields zero bits and
// records in `status` when one of them is consumed.
struct BitReader {
  const uint32_t* words;
  long pos, end, curw;
  uint64_t acc;
  uint32_t cur;
  int nbits, real, status;
  JPEG_HD BitReader(const uint32_t* w, long begin, long stop) : words(w), pos(begin), end(stop), curw(-1), acc(0), cur(0), nbits(0), real(0), status(0) {}
  JPEG_HD uint32_t byte_at(long p) {
    const long w = p >> 2;
    if (w != curw) { cur = words[w]; curw = w; }
    return (cur >> (8 * static_cast<int>(p & 3))) & 255u;
  }
  // at least 57 bits in the window: one symbol's code (<= 16) and value (<= 15) never need another
  JPEG_HD void fill() {
    for (int i = 0; i < 8 && nbits <= 56; ++i) {
      uint32_t b = 0;
      if (pos < end) {
        b = byte_at(pos);
        if (b != 255u) {
          ++pos;
          real += 8;
        } else if (pos + 1 < end && byte_at(pos + 1) == 0u) {
          pos += 2;
          real += 8;
        } else {
          end = pos;
          b = 0;
        }
      }
      acc |= static_cast<uint64_t>(b) << (56 - nbits);
      nbits += 8;
    }
  }
  JPEG_HD uint32_t peek(int n) const { return static_cast<uint32_t>(acc >> (64 - n)); }      // 1 <= n <= 32
  JPEG_HD void skip(int n) {
    acc <<= n;
    nbits -= n;
    real -= n;
    if (real < 0) { real = 0; status |= kStatusNoBits; }
  }
  JPEG_HD uint32_t take(int n) {      // 1 <= n <= 16
    const uint32_t v = peek(n);
    skip(n);
    return v;
  }
  // the next symbol of table h, -1: no code matches
  JPEG_HD int symbol(const HuffDec& h) {
    const uint32_t e = h.look[peek(9)];
    if (e) { skip(static_cast<int>(e >> 8)); return static_cast<int>(e & 255u); }
    for (int len = 10; len <= 16; ++len) {
      const uint32_t c = peek(len);
      if (static_cast<int>(c) <= h.maxcode[len]) {
        skip(len);
        return h.vals[static_cast<uint32_t>(h.valoff[len] + static_cast<int>(c)) & 255u];
      }
    }
    status |= kStatusBadCode;
    return -1;
  }
};

// what a row of the segment table asks for, clamped to the packed buffer and to the file's MCUs; false: nothing to decode
JPEG_HD bool segment_work(const Geom& g, const Segment& s, uint32_t restart, long nbytes, long& begin, long& end, int& first, int& n_mcu) {
  begin = s.begin < 0 ? 0 : s.begin > nbytes ? nbytes : s.begin;
  end = s.end < begin ? begin : s.end > nbytes ? nbytes : s.end;
  first = s.first_mcu;
  if (first < 0 || first >= g.mcus) return false;
  const int left = g.mcus - first;
  n_mcu = restart && restart < static_cast<uint32_t>(left) ? static_cast<int>(restart) : left;
  return true;
}
// a file's rows [lo, lo + n) of a segment table of `total` rows
JPEG_HD void file_segments(const FileDesc& d, int total, int& lo, int& n) {
  lo = d.seg0 < static_cast<uint32_t>(total) ? static_cast<int>(d.seg0) : total;
  n = d.nseg < static_cast<uint32_t>(total - lo) ? static_cast<int>(d.nseg) : total - lo;
}

JPEG_HD int extend(uint32_t v, int n) { return v < (1u << (n - 1)) ? static_cast<int>(v) - (1 << n) + 1 : static_cast<int>(v); }      // 1 <= n <= 15

// MCUs first_mcu .. first_mcu + n_mcu - 1 (the caller keeps them below g.mcus) out of `br`; store(block, k, v): coefficient k
// (natural order) of a file's block.  Only non-zero coefficients are stored.  zigzag: kZigzag, or a copy of it where a look-up per
// coefficient is cheaper (LDS on the device).  Returns the segment's status
template <class Store>
JPEG_HD int decode_segment(const Geom& g, const HuffDec* tabs, const uint8_t (*comp)[4], const uint8_t* zigzag, BitReader& br, int first_mcu,
                           int n_mcu, Store& store) {
  uint32_t pred[3] = {0u, 0u, 0u};      // wrap-around: a file may make the sum as large as it likes
  for (int m = first_mcu; m < first_mcu + n_mcu; ++m) {
    const int my = m / g.mcux, mx = m % g.mcux;
    for (int c = 0; c < g.ncomp; ++c) {
      const int hc = c ? 1 : g.hs, vc = c ? 1 : g.vs;
      const HuffDec& dc = tabs[comp[c][1] & 1];
      const HuffDec& ac = tabs[2 + (comp[c][2] & 1)];
      for (int b = 0; b < hc * vc; ++b) {
        const long blk = g.boff[c] + static_cast<long>(my * vc + b / hc) * g.bw[c] + (mx * hc + b % hc);
        br.fill();
        const int t = br.symbol(dc);
        if (t < 0) return br.status;
        if (t > 15) return br.status | kStatusBadCode;
        if (t) pred[c] += static_cast<uint32_t>(extend(br.take(t), t));
        const int16_t d0 = static_cast<int16_t>(static_cast<uint16_t>(pred[c] & 0xFFFFu));
        if (d0) store(blk, 0, d0);
        for (int k = 1; k < 64; ++k) {
          br.fill();
          const int rs = br.symbol(ac);
          if (rs < 0) return br.status;
          const int r = rs >> 4, s = rs & 15;
          if (s == 0) {
            if (r != 15) break;      // EOB
            k += 15;                 // ZRL
            continue;
          }
          k += r;
          if (k > 63) return br.status | kStatusBadIndex;
          store(blk, zigzag[k], static_cast<int16_t>(extend(br.take(s), s)));
        }
      }
    }
  }
  return br.status;
}

// ---- transform: one block's coefficients -> its 64 samples (jpeg_core.h's dequantise_idct in wrap-around arithmetic) ---------------------
JPEG_HD void block_samples(const int16_t* coef, const QTab& q, uint32_t (&d)[64]) {
#pragma unroll
  for (int i = 0; i < 64; ++i) d[i] = static_cast<uint32_t>(static_cast<int>(coef[i]));
  dequantise_idct(d, q);
}

// ---- chroma up-sampling, colour, L -----------------------------------------------------------------------------------------------------
// the sample of a chroma plane (real size cw x ch, rows `stride` apart) that libjpeg puts under output pixel (x, y): "fancy"
// triangle filters when cw > 2, plain replication otherwise; samples outside the real size are never read
JPEG_HD int chroma_at(const uint8_t* p, long stride, int cw, int ch, int hs, int vs, int x, int y) {
  if (hs == 1) return p[y * stride + x];
  const int i = x >> 1;
  if (cw <= 2) return p[(vs == 2 ? y >> 1 : y) * stride + i];
  if (vs == 1) {
    const uint8_t* r = p + y * stride;
    if (x & 1) return i == cw - 1 ? r[i] : (3 * r[i] + r[i + 1] + 2) >> 2;
    return i == 0 ? r[0] : (3 * r[i] + r[i - 1] + 1) >> 2;
  }
  const int j = y >> 1;
  int jn = (y & 1) ? j + 1 : j - 1;
  jn = jn < 0 ? 0 : jn > ch - 1 ? ch - 1 : jn;
  const uint8_t *a = p + j * stride, *b = p + jn * stride;
  const int ri = 3 * a[i] + b[i];
  if (x & 1) return i == cw - 1 ? (4 * ri + 7) >> 4 : (3 * ri + 3 * a[i + 1] + b[i + 1] + 7) >> 4;
  return i == 0 ? (4 * ri + 8) >> 4 : (3 * ri + 3 * a[i - 1] + b[i - 1] + 8) >> 4;
}

JPEG_HD int clamp8(int v) { return v < 0 ? 0 : v > 255 ? 255 : v; }
// libjpeg's jdcolor tables as arithmetic (SCALEBITS 16), cb and cr as stored
JPEG_HD void ycc_rgb(int y, int cb, int cr, int& r, int& g, int& b) {
  cb -= 128;
  cr -= 128;
  r = clamp8(y + ((91881 * cr + 32768) >> 16));
  g = clamp8(y + ((-22554 * cb - 46802 * cr + 32768) >> 16));
  b = clamp8(y + ((116130 * cb + 32768) >> 16));
}
// Pillow's convert("L") of an RGB pixel
JPEG_HD int rgb_l(int r, int g, int b) { return (19595 * r + 38470 * g + 7471 * b + 32768) >> 16; }

// output pixel (x, y) of a file whose planes start at `planes`: ch[0..2] = R, G, B (the same value for one component)
JPEG_HD void pixel_rgb(const Geom& g, const uint8_t* planes, int x, int y, int (&rgb)[3]) {
  const int yy = planes[g.poff[0] + static_cast<long>(y) * (8 * g.bw[0]) + x];
  if (g.ncomp == 1) {
    rgb[0] = rgb[1] = rgb[2] = yy;
    return;
  }
  const long stride = 8 * g.bw[1];
  const int cb = chroma_at(planes + g.poff[1], stride, g.cw, g.ch, g.hs, g.vs, x, y);
  const int cr = chroma_at(planes + g.poff[2], stride, g.cw, g.ch, g.hs, g.vs, x, y);
  ycc_rgb(yy, cb, cr, rgb[0], rgb[1], rgb[2]);
}

}  // namespace jpeg
}  // namespace diffsal
