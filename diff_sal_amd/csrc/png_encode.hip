// The reference's export for the visual sets (R/diffusion_trainer.py:898-935, save_img: '<video>/<frame>.png') on the device: uint8
// maps -> the complete 8-bit greyscale PNG file of each map.  include/diffsal.h ("PNG export") states the file, csrc/png_encode_core.h
// holds the arithmetic; the launches, all on the caller's stream:
//   clear     hipMemsetAsync of `data` (the pack ORs into it)
//   filter    a wave per row: the five filters' costs from the raw neighbours, a wave reduction, the choice, the filtered row
//   segment   a workgroup per 16384 stream bytes = one deflate block.  A thread holds 64 positions in registers: equality with the
//             byte in front as a 64-bit mask, the run a position lies in from the mask (clz / ctz) and, across threads, from a prefix
//             maximum and a suffix minimum of the differing positions in LDS; token records to the workspace; the symbol histogram
//             with integer LDS atomics; the symbols' order by a rank per thread; then one thread builds the two length-limited
//             codes, the run-length form and the header's bits (a few thousand steps); bit count per thread, exclusive scan;
//             Adler-32 partial sums of the segment
//   frame     a workgroup per image: exclusive scan of the blocks' bit counts, the Adler-32 of the stream from the segments' sums,
//             signature, IHDR, IDAT's length and type, the zlib header, Adler-32, IEND, the file's length
//   pack      a workgroup per segment: header words, then a thread per 64 positions puts its tokens at its bit offset.  Neighbours
//             share words: integer atomicOr, which commutes, so the bytes do not depend on the order
//   crc       a workgroup per image: the CRC of 64 bytes per thread, shifted by x^(8 * bytes behind it) mod P, XORed together
// Integer work only: two calls give the same bytes and an image's bytes do not depend on the batch it is in.  No allocation, no
// synchronisation, no host copy.  Every size comes from pnge::layout / pnge::capacity, which bound what any pixels can produce.
#include "common.h"
#include "png_encode_core.h"

namespace diffsal {
namespace pnge {

__constant__ CrcTables kCrcDev = make_crc_tables();

__global__ __launch_bounds__(kRowLanes) void png_filter_kernel(const uint8_t* __restrict__ in, int H, int W, long region, uint8_t* __restrict__ filt) {
  const int row = blockIdx.x, b = blockIdx.y, lane = threadIdx.x;
  const uint8_t* rp = in + (static_cast<long>(b) * H + row) * W;
  const uint8_t* up = row ? rp - W : nullptr;
  uint32_t cost[5] = {0, 0, 0, 0, 0};
  for (int x = lane; x < W; x += kRowLanes) {
    int v, a, bb, c;
    neighbours(rp, up, x, v, a, bb, c);
#pragma unroll
    for (int f = 0; f < 5; ++f) cost[f] += filter_cost(filter_byte(f, v, a, bb, c));      // at most 8192 * 128 in all
  }
#pragma unroll
  for (int f = 0; f < 5; ++f)
    for (int o = kRowLanes / 2; o; o >>= 1) cost[f] += __shfl_xor(cost[f], o, kRowLanes);
  const int f = choose_filter(cost);
  uint8_t* o = filt + static_cast<long>(b) * region + static_cast<long>(row) * (W + 1);      // row * (W + 1) + W < S <= region
  if (lane == 0) o[0] = static_cast<uint8_t>(f);
  for (int x = lane; x < W; x += kRowLanes) {
    int v, a, bb, c;
    neighbours(rp, up, x, v, a, bb, c);
    o[1 + x] = static_cast<uint8_t>(filter_byte(f, v, a, bb, c));
  }
}

__global__ __launch_bounds__(kThreads) void png_segment_kernel(const uint8_t* __restrict__ filt, Layout l, uint16_t* __restrict__ tok,
                                                               uint32_t* __restrict__ chunkoff, uint32_t* __restrict__ code,
                                                               uint32_t* __restrict__ header, SegInfo* __restrict__ info) {
  __shared__ BlockShared s;
  const int t = threadIdx.x, seg = blockIdx.x, b = blockIdx.y;
  const long at = static_cast<long>(seg) * kSegment, sidx = static_cast<long>(b) * l.nseg + seg;
  const int n = static_cast<int>(l.S - at < kSegment ? l.S - at : kSegment);
  ChunkRegs r;
  load_chunk(filt + static_cast<long>(b) * l.region + at, at, n, t, r);
  for (int i = t; i < 288; i += kThreads) s.hist[i] = i == 256 ? 1u : 0u;      // the end-of-block symbol, once
  if (t == 0) { s.nonzero = 0; s.m = 0; s.adler_a = 0; s.adler_b = 0; }
  s.ne_last[t] = r.last_ne;
  s.ne_first[t] = r.first_ne;
  __syncthreads();
  for (int o = 1; o < kThreads; o <<= 1) {      // prefix maximum, suffix minimum
    const int a = t >= o ? s.ne_last[t - o] : -1, f = t + o < kThreads ? s.ne_first[t + o] : n;
    __syncthreads();
    s.ne_last[t] = s.ne_last[t] > a ? s.ne_last[t] : a;
    s.ne_first[t] = s.ne_first[t] < f ? s.ne_first[t] : f;
    __syncthreads();
  }
  const int before = t ? s.ne_last[t - 1] : -1, after = t + 1 < kThreads ? s.ne_first[t + 1] : n;
  uint32_t* tk = reinterpret_cast<uint32_t*>(tok + static_cast<long>(b) * l.region + at) + t * (kChunk / 2);      // its chunk lies inside region when nv > 0
  if (r.nv) {
    for (int j = 0; j < kChunk; j += 2) {
      uint32_t pair = 0;
      for (int k = 0; k < 2; ++k) {
        const uint32_t tv = j + k < r.nv ? token_at(r, j + k, before, after) : kNone;
        if (tv != kNone) {
          int eb, ev;
          atomicAdd(&s.hist[token_symbol(tv, eb, ev)], 1u);
        }
        pair |= tv << (16 * k);
      }
      tk[j >> 1] = pair;
    }
    atomicAdd(&s.adler_a, r.s1);                  // at most 16384 * 255
    atomicAdd(&s.adler_b, r.s2 % kAdlerMod);      // at most 256 * 65520
  }
  __syncthreads();
  for (int i = t; i < kLit; i += kThreads)
    if (s.hist[i]) atomicAdd(&s.nonzero, 1u);
  __syncthreads();
  const int nonzero = static_cast<int>(s.nonzero);
  for (int i = t; i < kLit; i += kThreads)
    if (takes_part(s.hist, nonzero, i)) {
      s.cs.order[rank_of(s.hist, kLit, nonzero, i)] = static_cast<uint16_t>(i);
      atomicAdd(&s.m, 1u);
    }
  __syncthreads();
  if (t == 0) build_block(s, seg == l.nseg - 1);
  __syncthreads();
  for (int i = t; i < 288; i += kThreads) code[sidx * 288 + i] = i < kLit ? s.code[i] : 0u;
  if (t < kHeaderWords) header[sidx * kHeaderWords + t] = s.header[t];
  uint32_t mine = 0;
  for (int j = 0; j < r.nv; ++j) {
    const uint32_t tv = (tk[j >> 1] >> (16 * (j & 1))) & 0xFFFFu;      // its own stores
    if (tv != kNone) mine += token_bits(tv, s.code);
  }
  uint32_t sum;
  const uint32_t in_front = block_exclusive_scan<kThreads>(mine, s.scan, sum);      // at most 16384 * 21
  chunkoff[sidx * kThreads + t] = s.header_bits + in_front;
  if (t == 0) info[sidx] = SegInfo{s.header_bits, s.header_bits + sum + (s.code[256] & 15u), s.adler_a % kAdlerMod, s.adler_b % kAdlerMod};
}

// workgroup = image
__global__ __launch_bounds__(kThreads) void png_frame_kernel(const SegInfo* __restrict__ info, Layout l, Front front, unsigned long long* __restrict__ segoff,
                                                             unsigned long long* __restrict__ bits, uint8_t* __restrict__ out, long cap,
                                                             int* __restrict__ lengths) {
  __shared__ uint32_t sh[kThreads];
  const int t = threadIdx.x, b = blockIdx.x;
  unsigned long long carry = 0;
  uint32_t a_carry = 1, b_sum = 0;      // Adler-32: a starts at 1
  for (long base = 0; base < l.nseg; base += kThreads) {      // uniform trip count: every thread reaches the barriers
    const long sg = base + t;
    const bool have = sg < l.nseg;
    const SegInfo si = have ? info[static_cast<long>(b) * l.nseg + sg] : SegInfo{0, 0, 0, 0};
    const long left = l.S - sg * kSegment;
    const uint32_t n = have ? static_cast<uint32_t>(left < kSegment ? left : kSegment) : 0u;
    uint32_t sum, a_sum, c_sum;
    const uint32_t in_front = block_exclusive_scan<kThreads>(si.total_bits, sh, sum);      // a block has below 2^18.3 bits: the sum fits
    if (have) segoff[static_cast<long>(b) * l.nseg + sg] = carry + in_front;
    carry += sum;
    const uint32_t a_front = block_exclusive_scan<kThreads>(si.adler_a, sh, a_sum);
    const uint32_t a_here = (a_carry + a_front) % kAdlerMod;      // a where the segment starts
    const uint32_t c = static_cast<uint32_t>((si.adler_b + static_cast<unsigned long long>(n) * a_here) % kAdlerMod);
    (void)block_exclusive_scan<kThreads>(c, sh, c_sum);
    b_sum = (b_sum + c_sum) % kAdlerMod;
    a_carry = (a_carry + a_sum) % kAdlerMod;
  }
  if (t == 0) {
    bits[b] = carry;      // (carry + 7) / 8 <= max_deflate_bytes: the frame stays inside cap
    lengths[b] = write_frame(out + static_cast<long>(b) * cap, front, carry, (b_sum << 16) | a_carry);
  }
}

__global__ __launch_bounds__(kThreads) void png_pack_kernel(const uint16_t* __restrict__ tok, Layout l, const uint32_t* __restrict__ chunkoff,
                                                            const uint32_t* __restrict__ code, const uint32_t* __restrict__ header,
                                                            const SegInfo* __restrict__ info, const unsigned long long* __restrict__ segoff,
                                                            uint8_t* __restrict__ out, long cap) {
  __shared__ uint32_t sc[288];
  const int t = threadIdx.x, seg = blockIdx.x, b = blockIdx.y;
  const long at = static_cast<long>(seg) * kSegment, sidx = static_cast<long>(b) * l.nseg + seg;
  for (int i = t; i < 288; i += kThreads) sc[i] = code[sidx * 288 + i];
  __syncthreads();
  const SegInfo si = info[sidx];
  const unsigned long long base = 8ull * kFront + segoff[sidx];
  uint32_t* row = reinterpret_cast<uint32_t*>(out + static_cast<long>(b) * cap);
  const long words = cap / 4;
  auto store = [&](long wi, uint32_t word) {
    if (word && wi < words) atomicOr(row + wi, word);      // wi < words always: the stream ends inside max_deflate_bytes
  };
  for (uint32_t hw = t; hw < kHeaderWords && 32u * hw < si.header_bits; hw += kThreads) {
    const uint32_t left = si.header_bits - 32u * hw;
    BitWriter<decltype(store)> w(store, base + 32u * hw);
    w.put(header[sidx * kHeaderWords + hw], static_cast<int>(left < 32u ? left : 32u));
    w.finish();
  }
  const int n = static_cast<int>(l.S - at < kSegment ? l.S - at : kSegment);
  const int nv = n - t * kChunk < 0 ? 0 : n - t * kChunk > kChunk ? kChunk : n - t * kChunk;
  if (nv) {
    const uint32_t* tk = reinterpret_cast<const uint32_t*>(tok + static_cast<long>(b) * l.region + at) + t * (kChunk / 2);
    BitWriter<decltype(store)> w(store, base + chunkoff[sidx * kThreads + t]);
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

// workgroup = image: CRC-32 of IDAT's type and payload
__global__ __launch_bounds__(kThreads) void png_crc_kernel(const unsigned long long* __restrict__ bits, uint8_t* __restrict__ out, long cap) {
  __shared__ uint32_t table[256], x2n[32], acc;
  const int t = threadIdx.x, b = blockIdx.x;
  table[t] = kCrcDev.byte[t];      // kThreads == 256
  if (t < 32) x2n[t] = kCrcDev.x2n[t];
  if (t == 0) acc = 0;
  __syncthreads();
  long nb = static_cast<long>((bits[b] + 7) >> 3);
  if (nb > cap - kFraming) nb = cap - kFraming;      // never: the frame kernel's bound
  const long total = 4 + 2 + nb + 4;                 // type, zlib header, deflate stream, Adler-32
  uint8_t* p = out + static_cast<long>(b) * cap + 37;
  uint32_t mine = 0;
  for (long base = 0; base < total; base += static_cast<long>(kThreads) * kChunk) {
    const long first = base + static_cast<long>(t) * kChunk;
    if (first < total) {
      const int len = static_cast<int>(total - first < kChunk ? total - first : kChunk);
      mine ^= crc_shift(x2n, crc_bytes(table, p + first, len), static_cast<unsigned long long>(total - first - len));
    }
  }
  atomicXor(&acc, mine);
  __syncthreads();
  if (t == 0) put_be32(p + total, acc);
}

}  // namespace pnge
}  // namespace diffsal

using namespace diffsal;
using namespace diffsal::pnge;

extern "C" long diffsal_png_encode_capacity(int H, int W) {
  if (!shape_ok(1, H, W)) return 0;
  return capacity(H, W);
}

extern "C" size_t diffsal_png_encode_ws_bytes(int B, int H, int W) {
  if (!shape_ok(B, H, W)) return 0;
  return layout(B, H, W).bytes;
}

extern "C" int diffsal_png_encode(const void* u8, int B, int H, int W, void* data, long cap, void* lengths, void* ws, size_t ws_bytes,
                                  diffsal_stream_t stream) {
  DS_REQUIRE(u8 && data && lengths && ws, DIFFSAL_E_ARG, "png_encode: null argument");
  DS_REQUIRE(shape_ok(B, H, W), DIFFSAL_E_SHAPE, "png_encode: B=%d (1..%d), %d x %d (H 1..%d, W 1..%d)", B, kMaxB, H, W, kMaxH, kMaxW);
  const long need = capacity(H, W);
  DS_REQUIRE(cap >= need && cap % 16 == 0, DIFFSAL_E_ARG, "png_encode: cap %ld below diffsal_png_encode_capacity(%d, %d) = %ld or no multiple of 16", cap,
             H, W, need);
  const Layout l = layout(B, H, W);
  DS_REQUIRE(ws_bytes >= l.bytes && aligned16(ws), DIFFSAL_E_ARG, "png_encode: workspace too small (%zu of %zu bytes) or misaligned", ws_bytes, l.bytes);
  DS_REQUIRE(aligned16(data) && (reinterpret_cast<uintptr_t>(lengths) & 3u) == 0, DIFFSAL_E_ARG, "png_encode: data (16 bytes) or lengths (4) misaligned");
  char* base = static_cast<char*>(ws);
  uint8_t* filt = reinterpret_cast<uint8_t*>(base + l.filt);
  uint16_t* tok = reinterpret_cast<uint16_t*>(base + l.tok);
  uint32_t* chunkoff = reinterpret_cast<uint32_t*>(base + l.chunkoff);
  uint32_t* code = reinterpret_cast<uint32_t*>(base + l.code);
  uint32_t* header = reinterpret_cast<uint32_t*>(base + l.header);
  SegInfo* info = reinterpret_cast<SegInfo*>(base + l.info);
  unsigned long long* segoff = reinterpret_cast<unsigned long long*>(base + l.segoff);
  unsigned long long* bits = reinterpret_cast<unsigned long long*>(base + l.bits);
  uint8_t* out = static_cast<uint8_t*>(data);
  hipStream_t s = static_cast<hipStream_t>(stream);
  const dim3 per_segment(static_cast<unsigned>(l.nseg), B);
  int rc;
  if (hipMemsetAsync(out, 0, static_cast<size_t>(B) * cap, s) != hipSuccess) {
    (void)hipGetLastError();
    set_error("png_encode: clearing data failed");
    return DIFFSAL_E_LAUNCH;
  }
  hipLaunchKernelGGL(png_filter_kernel, dim3(H, B), dim3(kRowLanes), 0, s, static_cast<const uint8_t*>(u8), H, W, l.region, filt);
  if ((rc = check_launch("png_encode(filter)"))) return rc;
  hipLaunchKernelGGL(png_segment_kernel, per_segment, dim3(kThreads), 0, s, filt, l, tok, chunkoff, code, header, info);
  if ((rc = check_launch("png_encode(segment)"))) return rc;
  hipLaunchKernelGGL(png_frame_kernel, dim3(B), dim3(kThreads), 0, s, info, l, make_front(H, W), segoff, bits, out, cap, static_cast<int*>(lengths));
  if ((rc = check_launch("png_encode(frame)"))) return rc;
  hipLaunchKernelGGL(png_pack_kernel, per_segment, dim3(kThreads), 0, s, tok, l, chunkoff, code, header, info, segoff, out, cap);
  if ((rc = check_launch("png_encode(pack)"))) return rc;
  hipLaunchKernelGGL(png_crc_kernel, dim3(B), dim3(kThreads), 0, s, bits, out, cap);
  return check_launch("png_encode(crc)");
}
