// The reference's export for the audio-visual sets (R/diffusion_trainer.py:898-935, save_img(av_data=True): cv2.imwrite of
// pred_sal_%06d.jpg) on the device: uint8 maps -> the complete baseline JPEG files and the pixels a libjpeg decoder reads back from
// them.  include/diffsal.h ("JPEG export") states the arithmetic, csrc/jpeg_core.h holds it; the launches, all on the caller's stream:
//   jpeg_roundtrip  block   a thread per 8 x 8 block: forward DCT, quantise, dequantise, inverse DCT, range limit
//   jpeg_encode     clear   hipMemsetAsync of the bit stream (the pack ORs into it)
//                   block   as above (the read-back pixels only when asked for); the quantised coefficients in zig-zag order and
//                           the bit count of the block's AC symbols go to the workspace
//                   offsets a workgroup per image: bit count of every block (its AC bits + its DC symbol, from the DC of the block
//                           before it), exclusive scan in chunks of 256 blocks with a running carry
//                   pack    a thread per block: its code, ORed into the 32-bit words of the bit stream at its bit offset.
//                           Neighbouring blocks share words: integer atomicOr, which commutes, so the words do not depend on the order
//                   count   FF bytes per chunk of 2048 scan bytes
//                   frame   a workgroup per image: exclusive scan of the chunk counts; header, EOI and the file length
//                   stuff   a thread per 8 scan bytes: each byte to its place behind the header, a 00 behind every FF
// A thread owns a whole block (64 integers in registers): the transforms are libjpeg's, statement for statement, and no lane waits
// for another.  Coefficient k of all blocks of an image lies side by side ([64][nblk] int16), so the stores of a wave and the
// entropy coder's loads are contiguous; the coder walks its block's 63 coefficients out of LDS ([k][thread]: no bank conflict).
// Integer work only: two calls give the same bits and an image's bytes do not depend on the batch it is in.  No allocation, no
// synchronisation, no host copy.  Every size comes from jpeg::layout / jpeg::capacity, which bound what any input can produce.
#include <initializer_list>

#include "common.h"
#include "jpeg_core.h"

namespace diffsal {
namespace jpeg {

__constant__ HuffEnc kHuffDev = make_huff();

__device__ __forceinline__ void load_huff(uint32_t* ac, uint32_t* dc) {
  ac[threadIdx.x] = kHuffDev.ac[threadIdx.x];      // kThreads == 256 entries
  if (threadIdx.x < 16) dc[threadIdx.x] = kHuffDev.dc[threadIdx.x];
  __syncthreads();
}

// ENC: coefficients and AC bit counts to the workspace; REC: the read-back pixels to recon.  vec: w % 8 == 0 and 8-byte aligned bases
template <bool ENC, bool REC>
__global__ __launch_bounds__(kThreads) void jpeg_block_kernel(const unsigned char* __restrict__ in, int h, int w, int bw, long nblk, QTab q,
                                                              short* __restrict__ coef, uint32_t* __restrict__ acbits,
                                                              unsigned char* __restrict__ recon, int vec) {
  __shared__ uint32_t ac[256], dc[16];
  __shared__ short zz[ENC ? 64 * kThreads : 1];
  if (ENC) load_huff(ac, dc);
  const long blk = static_cast<long>(blockIdx.x) * kThreads + threadIdx.x;
  const int b = blockIdx.y;
  if (blk >= nblk) return;
  const int x0 = static_cast<int>(blk % bw) * 8, y0 = static_cast<int>(blk / bw) * 8;
  const long io = static_cast<long>(b) * h * w;
  const bool whole = vec && x0 + 8 <= w;
  int d[64];
#pragma unroll
  for (int r = 0; r < 8; ++r) {
    const int y = y0 + r < h ? y0 + r : h - 1;      // the last row again
    const unsigned char* row = in + io + static_cast<long>(y) * w;
    if (whole) {
      const uint2 v = *reinterpret_cast<const uint2*>(row + x0);
#pragma unroll
      for (int c = 0; c < 4; ++c) {
        d[8 * r + c] = static_cast<int>((v.x >> (8 * c)) & 255u) - 128;
        d[8 * r + 4 + c] = static_cast<int>((v.y >> (8 * c)) & 255u) - 128;
      }
    } else {
#pragma unroll
      for (int c = 0; c < 8; ++c) d[8 * r + c] = static_cast<int>(row[x0 + c < w ? x0 + c : w - 1]) - 128;      // the last column again
    }
  }
  fdct_quantise(d, q);
  if (ENC) {
    short* cb = coef + static_cast<long>(b) * 64 * nblk + blk;
#pragma unroll
    for (int k = 0; k < 64; ++k) {
      const short v = static_cast<short>(d[kZigzag[k]]);
      cb[static_cast<long>(k) * nblk] = v;
      zz[k * kThreads + threadIdx.x] = v;
    }
    uint32_t bits = 0;
    auto count = [&](uint32_t, int n) { bits += static_cast<uint32_t>(n); };
    put_ac([&](int k) { return static_cast<int>(zz[k * kThreads + threadIdx.x]); }, ac, count);      // its own column: no barrier
    acbits[static_cast<long>(b) * nblk + blk] = bits;
  }
  if (REC) {
    dequantise_idct(d, q);
    unsigned char* ob = recon + io;
#pragma unroll
    for (int r = 0; r < 8; ++r) {
      if (y0 + r >= h) break;
      unsigned char* row = ob + static_cast<long>(y0 + r) * w;
      if (whole) {
        uint2 v;
        v.x = d[8 * r] | (d[8 * r + 1] << 8) | (d[8 * r + 2] << 16) | (d[8 * r + 3] << 24);
        v.y = d[8 * r + 4] | (d[8 * r + 5] << 8) | (d[8 * r + 6] << 16) | (d[8 * r + 7] << 24);
        *reinterpret_cast<uint2*>(row + x0) = v;
      } else {
#pragma unroll
        for (int c = 0; c < 8; ++c)
          if (x0 + c < w) row[x0 + c] = static_cast<unsigned char>(d[8 * r + c]);
      }
    }
  }
}

// workgroup = image: bit offset of every block, the image's bit count
__global__ __launch_bounds__(kThreads) void jpeg_offsets_kernel(const short* __restrict__ coef, const uint32_t* __restrict__ acbits, long nblk,
                                                                unsigned long long* __restrict__ bitoff, unsigned long long* __restrict__ total) {
  __shared__ uint32_t ac[256], dc[16];
  __shared__ uint32_t sh[kThreads];
  load_huff(ac, dc);
  const int b = blockIdx.x;
  const short* dcs = coef + static_cast<long>(b) * 64 * nblk;      // plane 0: the quantised DC of every block
  unsigned long long carry = 0;
  for (long base = 0; base < nblk; base += kThreads) {      // uniform trip count: every thread reaches the barriers
    const long blk = base + threadIdx.x;
    uint32_t bits = 0;
    if (blk < nblk) {
      auto count = [&](uint32_t, int n) { bits += static_cast<uint32_t>(n); };
      put_dc(static_cast<int>(dcs[blk]) - (blk ? static_cast<int>(dcs[blk - 1]) : 0), dc, count);
      bits += acbits[static_cast<long>(b) * nblk + blk];
    }
    uint32_t sum;
    const uint32_t before = block_exclusive_scan<kThreads>(bits, sh, sum);
    if (blk < nblk) bitoff[static_cast<long>(b) * nblk + blk] = carry + before;
    carry += sum;
  }
  if (threadIdx.x == 0) total[b] = carry;
}

__global__ __launch_bounds__(kThreads) void jpeg_pack_kernel(const short* __restrict__ coef, const unsigned long long* __restrict__ bitoff,
                                                             long nblk, uint32_t* __restrict__ stream, long words) {
  __shared__ uint32_t ac[256], dc[16];
  __shared__ short zz[64 * kThreads];
  load_huff(ac, dc);
  const long blk = static_cast<long>(blockIdx.x) * kThreads + threadIdx.x;
  const int b = blockIdx.y;
  if (blk >= nblk) return;
  const short* cb = coef + static_cast<long>(b) * 64 * nblk + blk;
#pragma unroll 8
  for (int k = 0; k < 64; ++k) zz[k * kThreads + threadIdx.x] = cb[static_cast<long>(k) * nblk];
  uint32_t* ws = stream + static_cast<long>(b) * words;
  auto store = [&](long wi, uint32_t word) {
    if (word && wi < words) atomicOr(ws + wi, word);      // wi < words always (a block's code has at most kMaxBlockBits bits)
  };
  BitWriter<decltype(store)> out(store, bitoff[static_cast<long>(b) * nblk + blk]);
  put_dc(static_cast<int>(zz[threadIdx.x]) - (blk ? static_cast<int>(cb[-1]) : 0), dc, out);
  put_ac([&](int k) { return static_cast<int>(zz[k * kThreads + threadIdx.x]); }, ac, out);
  out.finish();
}

// FF bytes among this thread's kStuffBytes scan bytes, which it leaves in by[]; n = how many of them exist
__device__ __forceinline__ uint32_t stuff_load(const uint32_t* __restrict__ ws, long first, long nbytes, unsigned long long total_bits,
                                               uint32_t (&by)[kStuffBytes], int& n) {
  n = 0;
  uint32_t ff = 0;
  if (first >= nbytes) return 0;
  const uint32_t w0 = ws[first >> 2], w1 = first + 4 < nbytes ? ws[(first >> 2) + 1] : 0u;
#pragma unroll
  for (int j = 0; j < kStuffBytes; ++j) {
    const long i = first + j;
    if (i < nbytes) {
      by[j] = scan_byte(j < 4 ? w0 : w1, i, nbytes, total_bits);
      ff += by[j] == 255u;
      n = j + 1;
    }
  }
  return ff;
}

__global__ __launch_bounds__(kThreads) void jpeg_count_kernel(const uint32_t* __restrict__ stream, long words, const unsigned long long* __restrict__ total,
                                                              uint32_t* __restrict__ ffcount, long chunks) {
  __shared__ uint32_t sh[kThreads];
  const int b = blockIdx.y;
  const long chunk = blockIdx.x;
  const unsigned long long tb = total[b];
  const long nbytes = static_cast<long>((tb + 7) >> 3);
  if (chunk * kStuffChunk >= nbytes) return;      // uniform
  uint32_t by[kStuffBytes];
  int n;
  const uint32_t ff = stuff_load(stream + static_cast<long>(b) * words, chunk * kStuffChunk + static_cast<long>(threadIdx.x) * kStuffBytes, nbytes, tb, by, n);
  uint32_t sum;
  block_exclusive_scan<kThreads>(ff, sh, sum);
  if (threadIdx.x == 0) ffcount[static_cast<long>(b) * chunks + chunk] = sum;
}

// workgroup = image: FF bytes in front of every chunk; the header, EOI and the file's length
__global__ __launch_bounds__(kThreads) void jpeg_frame_kernel(const uint32_t* __restrict__ ffcount, long chunks, const unsigned long long* __restrict__ total,
                                                              uint32_t* __restrict__ ffoff, Header hd, unsigned char* __restrict__ out, long cap,
                                                              int* __restrict__ lengths) {
  __shared__ uint32_t sh[kThreads];
  const int b = blockIdx.x;
  const long nbytes = static_cast<long>((total[b] + 7) >> 3);
  const long used = (nbytes + kStuffChunk - 1) / kStuffChunk;      // <= chunks
  uint32_t carry = 0;
  for (long base = 0; base < used; base += kThreads) {
    const long c = base + threadIdx.x;
    const uint32_t v = c < used ? ffcount[static_cast<long>(b) * chunks + c] : 0u;
    uint32_t sum;
    const uint32_t before = block_exclusive_scan<kThreads>(v, sh, sum);
    if (c < used) ffoff[static_cast<long>(b) * chunks + c] = carry + before;
    carry += sum;
  }
  unsigned char* ob = out + static_cast<long>(b) * cap;
  for (int k = threadIdx.x; k < kHeaderBytes; k += kThreads) ob[k] = static_cast<unsigned char>((hd.w[k >> 2] >> (8 * (k & 3))) & 255u);
  if (threadIdx.x == 0) {
    const long end = kHeaderBytes + nbytes + carry;      // <= cap - 4
    ob[end] = 0xFF;
    ob[end + 1] = 0xD9;
    lengths[b] = static_cast<int>(end + 2);
  }
}

__global__ __launch_bounds__(kThreads) void jpeg_stuff_kernel(const uint32_t* __restrict__ stream, long words, const unsigned long long* __restrict__ total,
                                                              const uint32_t* __restrict__ ffoff, long chunks, unsigned char* __restrict__ out, long cap) {
  __shared__ uint32_t sh[kThreads];
  const int b = blockIdx.y;
  const long chunk = blockIdx.x;
  const unsigned long long tb = total[b];
  const long nbytes = static_cast<long>((tb + 7) >> 3);
  if (chunk * kStuffChunk >= nbytes) return;      // uniform
  uint32_t by[kStuffBytes];
  int n;
  const long first = chunk * kStuffChunk + static_cast<long>(threadIdx.x) * kStuffBytes;
  const uint32_t ff = stuff_load(stream + static_cast<long>(b) * words, first, nbytes, tb, by, n);
  uint32_t sum;
  const uint32_t before = block_exclusive_scan<kThreads>(ff, sh, sum);
  // byte i lands at header + i + (FF bytes in front of it) <= header + 2 nbytes - 1, its 00 one further: inside cap
  unsigned char* o = out + static_cast<long>(b) * cap + kHeaderBytes + first + ffoff[static_cast<long>(b) * chunks + chunk] + before;
#pragma unroll
  for (int j = 0; j < kStuffBytes; ++j) {
    if (j < n) {
      *o++ = static_cast<unsigned char>(by[j]);
      if (by[j] == 255u) *o++ = 0;
    }
  }
}

static int jpeg_args(const char* what, const void* u8, int B, int h, int w, int quality) {
  DS_REQUIRE(u8, DIFFSAL_E_ARG, "%s: null argument", what);
  DS_REQUIRE(B >= 1 && B <= 65535, DIFFSAL_E_SHAPE, "%s: B=%d (1..65535)", what, B);
  DS_REQUIRE(h >= 1 && h <= kMaxDim && w >= 1 && w <= kMaxDim, DIFFSAL_E_SHAPE, "%s: %d x %d (1..%d per axis)", what, h, w, kMaxDim);
  DS_REQUIRE(quality >= 1 && quality <= 100, DIFFSAL_E_ARG, "%s: quality %d (1..100)", what, quality);
  return DIFFSAL_OK;
}

static inline bool aligned8(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 7u) == 0; }

}  // namespace jpeg
}  // namespace diffsal

using namespace diffsal;
using namespace diffsal::jpeg;

extern "C" long diffsal_jpeg_capacity(int h, int w) {
  if (h < 1 || h > kMaxDim || w < 1 || w > kMaxDim) return 0;
  return capacity(h, w);
}

extern "C" size_t diffsal_jpeg_encode_ws_bytes(int B, int h, int w) {
  if (B < 1 || h < 1 || h > kMaxDim || w < 1 || w > kMaxDim) return 0;
  return layout(B, h, w).bytes;
}

extern "C" int diffsal_jpeg_roundtrip(const unsigned char* u8, int B, int h, int w, int quality, unsigned char* recon,
                                      diffsal_stream_t stream) {
  int rc = jpeg_args("jpeg_roundtrip", u8, B, h, w, quality);
  if (rc) return rc;
  DS_REQUIRE(recon, DIFFSAL_E_ARG, "jpeg_roundtrip: null argument");
  const long nblk = blocks_of(h, w);
  const int vec = (w % 8 == 0 && aligned8(u8) && aligned8(recon)) ? 1 : 0;
  const dim3 grid(static_cast<unsigned>((nblk + kThreads - 1) / kThreads), B);
  hipLaunchKernelGGL((jpeg_block_kernel<false, true>), grid, dim3(kThreads), 0, static_cast<hipStream_t>(stream), u8, h, w, (w + 7) / 8, nblk,
                     quant_table(quality), nullptr, nullptr, recon, vec);
  return check_launch("jpeg_roundtrip(block)");
}

extern "C" int diffsal_jpeg_encode(const unsigned char* u8, int B, int h, int w, int quality, unsigned char* out, long cap, int* lengths,
                                   unsigned char* recon, void* ws, size_t ws_bytes, diffsal_stream_t stream) {
  int rc = jpeg_args("jpeg_encode", u8, B, h, w, quality);
  if (rc) return rc;
  DS_REQUIRE(out && lengths && ws, DIFFSAL_E_ARG, "jpeg_encode: null argument");
  const long need = capacity(h, w);
  DS_REQUIRE(need <= 0x7FFFFFFFL, DIFFSAL_E_SHAPE, "jpeg_encode: %d x %d: a file may reach %ld bytes, above the int32 lengths", h, w, need);
  DS_REQUIRE(cap >= need, DIFFSAL_E_ARG, "jpeg_encode: cap %ld below diffsal_jpeg_capacity(%d, %d) = %ld", cap, h, w, need);
  const Layout l = layout(B, h, w);
  DS_REQUIRE(ws_bytes >= l.bytes && aligned16(ws), DIFFSAL_E_ARG, "jpeg_encode: workspace too small (%zu of %zu bytes) or misaligned", ws_bytes,
             l.bytes);
  DS_REQUIRE((reinterpret_cast<uintptr_t>(lengths) & 3u) == 0, DIFFSAL_E_ARG, "jpeg_encode: lengths misaligned");
  char* base = static_cast<char*>(ws);
  short* coef = reinterpret_cast<short*>(base + l.coef);
  uint32_t* acbits = reinterpret_cast<uint32_t*>(base + l.acbits);
  unsigned long long* bitoff = reinterpret_cast<unsigned long long*>(base + l.bitoff);
  unsigned long long* total = reinterpret_cast<unsigned long long*>(base + l.total);
  uint32_t* words = reinterpret_cast<uint32_t*>(base + l.stream);
  uint32_t* ffcount = reinterpret_cast<uint32_t*>(base + l.ffcount);
  uint32_t* ffoff = reinterpret_cast<uint32_t*>(base + l.ffoff);
  hipStream_t s = static_cast<hipStream_t>(stream);
  const QTab q = quant_table(quality);
  const int vec = (w % 8 == 0 && aligned8(u8) && (!recon || aligned8(recon))) ? 1 : 0;
  const dim3 per_block(static_cast<unsigned>((l.nblk + kThreads - 1) / kThreads), B), per_chunk(static_cast<unsigned>(l.chunks), B);
  if (hipMemsetAsync(words, 0, static_cast<size_t>(B) * l.words * 4, s) != hipSuccess) {
    (void)hipGetLastError();
    set_error("jpeg_encode: clearing the bit stream failed");
    return DIFFSAL_E_LAUNCH;
  }
  if (recon)
    hipLaunchKernelGGL((jpeg_block_kernel<true, true>), per_block, dim3(kThreads), 0, s, u8, h, w, (w + 7) / 8, l.nblk, q, coef, acbits, recon, vec);
  else
    hipLaunchKernelGGL((jpeg_block_kernel<true, false>), per_block, dim3(kThreads), 0, s, u8, h, w, (w + 7) / 8, l.nblk, q, coef, acbits, nullptr, vec);
  if ((rc = check_launch("jpeg_encode(block)"))) return rc;
  hipLaunchKernelGGL(jpeg_offsets_kernel, dim3(B), dim3(kThreads), 0, s, coef, acbits, l.nblk, bitoff, total);
  if ((rc = check_launch("jpeg_encode(offsets)"))) return rc;
  hipLaunchKernelGGL(jpeg_pack_kernel, per_block, dim3(kThreads), 0, s, coef, bitoff, l.nblk, words, l.words);
  if ((rc = check_launch("jpeg_encode(pack)"))) return rc;
  hipLaunchKernelGGL(jpeg_count_kernel, per_chunk, dim3(kThreads), 0, s, words, l.words, total, ffcount, l.chunks);
  if ((rc = check_launch("jpeg_encode(count)"))) return rc;
  hipLaunchKernelGGL(jpeg_frame_kernel, dim3(B), dim3(kThreads), 0, s, ffcount, l.chunks, total, ffoff, make_header(h, w, q), out, cap, lengths);
  if ((rc = check_launch("jpeg_encode(frame)"))) return rc;
  hipLaunchKernelGGL(jpeg_stuff_kernel, per_chunk, dim3(kThreads), 0, s, words, l.words, total, ffoff, l.chunks, out, cap);
  return check_launch("jpeg_encode(stuff)");
}
