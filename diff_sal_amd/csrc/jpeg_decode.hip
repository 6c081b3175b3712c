// The reference's frame loader (R/datasets/saliency_db.py:29-44: pil_loader = Image.open(f).convert('RGB'), pil_loader_sal =
// .convert('L') of img_%05d.jpg / eyeMap_%05d.jpg) on the device: the bytes of baseline JPEG files -> the uint8 frames Pillow
// returns, bit for bit.  include/diffsal.h ("JPEG decode") states the arithmetic, csrc/jpeg_decode_core.h holds it; the launches,
// all on the caller's stream:
//   clear      hipMemsetAsync of the status words and the coefficients (the entropy pass writes non-zero coefficients only)
//   entropy    grid (segment chunks, files), a wave per workgroup.  The workgroup builds the file's four Huffman tables in LDS from
//              the DHT counts and symbols (a lane per table), then each lane decodes one restart segment serially: bits through a
//              64-bit window refilled from aligned 32-bit loads, a 9-bit first-level look-up, maxcode / valoff for longer codes.
//              A file without restart markers is one lane's work: the parallelism is across files and restart intervals
//   transform  a lane per 8 x 8 block, 64 values in registers: dequantise, jpeg_core.h's inverse DCT and range limit, eight 8-byte
//              stores into the component's plane (component resolution, MCU padding included)
//   colour     a lane per 16 output pixels of a row: chroma up-sampling (libjpeg's fancy filters), YCbCr -> RGB, Pillow's L where
//              asked; 16-byte stores when the rows allow it.  Lane 0 of a file copies its status word out
// Hostile bytes: the byte ranges and MCU counts of the segment table are clamped to the packed buffer and the file's MCUs
// (segment_work), selectors are masked, every loop bound is a constant or comes from the geometry, the reader yields zero bits
// behind a segment's end, the coefficient index is checked before the store.  tools/jpeg_decode_host_check.cpp runs the same
// functions under a sanitizer.  Integer work only: two calls give the same bits and a file's pixels do not depend on the batch it
// is in.  No allocation, no synchronisation, no host copy.
#include "common.h"
#include "jpeg_decode_core.h"

namespace diffsal {
namespace jpeg {

__global__ __launch_bounds__(kSegThreads) void jpeg_entropy_kernel(const uint32_t* __restrict__ words, long nbytes, const FileDesc* __restrict__ files,
                                                                   const Segment* __restrict__ segs, int nseg, Geom g, short* __restrict__ coef,
                                                                   int* __restrict__ status) {
  __shared__ HuffDec tabs[4];
  __shared__ uint8_t comp[4][4];
  __shared__ uint8_t zigzag[64];      // a look-up per coefficient: out of LDS, not out of constant memory
  zigzag[threadIdx.x] = kZigzag[threadIdx.x];      // kSegThreads == 64
  const int f = blockIdx.y;
  const FileDesc& d = files[f];
  if (threadIdx.x < 4) build_huff(tabs[threadIdx.x], d.hbits[threadIdx.x], d.hvals[threadIdx.x]);
  if (threadIdx.x < 16) comp[threadIdx.x >> 2][threadIdx.x & 3] = d.comp[threadIdx.x >> 2][threadIdx.x & 3];
  __syncthreads();
  int lo, n;
  file_segments(d, nseg, lo, n);
  const long i = static_cast<long>(blockIdx.x) * kSegThreads + threadIdx.x;
  if (i >= n) return;
  long begin, end;
  int first, n_mcu;
  if (!segment_work(g, segs[lo + i], d.restart, nbytes, begin, end, first, n_mcu)) return;
  BitReader br(words, begin, end);
  short* cf = coef + static_cast<long>(f) * g.nblk * 64;
  auto store = [&](long blk, int k, int16_t v) { cf[blk * 64 + k] = v; };      // blk < g.nblk (m < g.mcus), k <= 63
  const int st = decode_segment(g, tabs, comp, zigzag, br, first, n_mcu, store);
  if (st) atomicOr(status + f, st);
}

__global__ __launch_bounds__(kThreads) void jpeg_transform_kernel(const FileDesc* __restrict__ files, Geom g, const short* __restrict__ coef,
                                                                  unsigned char* __restrict__ planes) {
  __shared__ QTab q[3];
  const int f = blockIdx.y;
  if (threadIdx.x < 64 * g.ncomp) {
    const int c = threadIdx.x >> 6, k = threadIdx.x & 63;
    q[c].t[k] = files[f].qt[files[f].comp[c][0] & 3][k];
  }
  __syncthreads();
  const long blk = static_cast<long>(blockIdx.x) * kThreads + threadIdx.x;
  if (blk >= g.nblk) return;
  const int c = g.ncomp == 3 && blk >= g.boff[2] ? 2 : g.ncomp == 3 && blk >= g.boff[1] ? 1 : 0;
  const uint4* src = reinterpret_cast<const uint4*>(coef + (static_cast<long>(f) * g.nblk + blk) * 64);      // 128 bytes, 16-byte aligned
  uint32_t d[64];
#pragma unroll
  for (int v = 0; v < 8; ++v) {
    const uint4 w = src[v];
    const uint32_t ws[4] = {w.x, w.y, w.z, w.w};
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      d[8 * v + 2 * j] = static_cast<uint32_t>(static_cast<int>(static_cast<int16_t>(ws[j] & 0xFFFFu)));
      d[8 * v + 2 * j + 1] = static_cast<uint32_t>(static_cast<int>(static_cast<int16_t>(ws[j] >> 16)));
    }
  }
  dequantise_idct(d, q[c]);
  const long b = blk - g.boff[c], stride = 8L * g.bw[c];
  unsigned char* o = planes + static_cast<long>(f) * g.plane + g.poff[c] + (b / g.bw[c]) * 8 * stride + (b % g.bw[c]) * 8;
#pragma unroll
  for (int r = 0; r < 8; ++r) {
    uint2 v;
    v.x = d[8 * r] | (d[8 * r + 1] << 8) | (d[8 * r + 2] << 16) | (d[8 * r + 3] << 24);
    v.y = d[8 * r + 4] | (d[8 * r + 5] << 8) | (d[8 * r + 6] << 16) | (d[8 * r + 7] << 24);
    *reinterpret_cast<uint2*>(o + r * stride) = v;      // the planes are 16-byte aligned and a multiple of 8 wide
  }
}

// L: one byte per pixel, else three.  vec: W % 16 == 0 and a 16-byte aligned output
template <bool L>
__global__ __launch_bounds__(kThreads) void jpeg_colour_kernel(Geom g, const unsigned char* __restrict__ planes, int groups, unsigned char* __restrict__ out,
                                                               const int* __restrict__ ws_status, int* __restrict__ status, int vec) {
  constexpr int C = L ? 1 : 3;
  const int f = blockIdx.y;
  const long t = static_cast<long>(blockIdx.x) * kThreads + threadIdx.x;
  if (t == 0) status[f] = ws_status[f];
  if (t >= static_cast<long>(groups) * g.H) return;
  const int y = static_cast<int>(t / groups), x0 = static_cast<int>(t % groups) * kRowPixels;
  const unsigned char* p = planes + static_cast<long>(f) * g.plane;
  unsigned char* o = out + ((static_cast<long>(f) * g.H + y) * g.W + x0) * C;
  uint32_t w[4 * C] = {};
#pragma unroll
  for (int i = 0; i < kRowPixels; ++i) {
    if (x0 + i >= g.W) continue;
    int rgb[3];
    pixel_rgb(g, p, x0 + i, y, rgb);
    if (L) {
      const int v = g.ncomp == 1 ? rgb[0] : rgb_l(rgb[0], rgb[1], rgb[2]);
      if (vec) w[i >> 2] |= static_cast<uint32_t>(v) << (8 * (i & 3));
      else o[i] = static_cast<unsigned char>(v);
    } else {
#pragma unroll
      for (int k = 0; k < 3; ++k) {
        if (vec) w[(3 * i + k) >> 2] |= static_cast<uint32_t>(rgb[k]) << (8 * ((3 * i + k) & 3));
        else o[3 * i + k] = static_cast<unsigned char>(rgb[k]);
      }
    }
  }
  if (vec) {
#pragma unroll
    for (int v = 0; v < C; ++v) reinterpret_cast<uint4*>(o)[v] = make_uint4(w[4 * v], w[4 * v + 1], w[4 * v + 2], w[4 * v + 3]);
  }
}

}  // namespace jpeg
}  // namespace diffsal

using namespace diffsal;
using namespace diffsal::jpeg;

extern "C" size_t diffsal_jpeg_decode_ws_bytes(int N, int H, int W, int ncomp, int hs, int vs) {
  if (!geom_ok(N, H, W, ncomp, hs, vs)) return 0;
  return geom(N, H, W, ncomp, hs, vs).bytes;
}

extern "C" int diffsal_jpeg_decode(const unsigned char* bytes, long nbytes, const void* files, const int* segments, int nseg, int max_file_seg,
                                   int N, int H, int W, int ncomp, int hs, int vs, int mode_l, unsigned char* out, int* status, void* ws,
                                   size_t ws_bytes, diffsal_stream_t stream) {
  DS_REQUIRE(bytes && files && segments && out && status && ws, DIFFSAL_E_ARG, "jpeg_decode: null argument");
  DS_REQUIRE(geom_ok(N, H, W, ncomp, hs, vs), DIFFSAL_E_SHAPE,
             "jpeg_decode: N=%d (1..65535), %d x %d (1..%d per axis), %d components (1 or 3), luma sampling %d x %d (1x1, 2x1, 2x2)", N, H, W,
             kMaxDim, ncomp, hs, vs);
  DS_REQUIRE(nbytes >= 4 && nbytes % 4 == 0 && nbytes <= 0x7FFFFFFFL && (reinterpret_cast<uintptr_t>(bytes) & 3u) == 0, DIFFSAL_E_ARG,
             "jpeg_decode: the packed files must be 4-byte aligned and a multiple of 4 bytes below 2^31 (padded), got %ld", nbytes);
  DS_REQUIRE(nseg >= 1 && max_file_seg >= 1 && max_file_seg <= nseg, DIFFSAL_E_ARG, "jpeg_decode: %d segments, at most %d per file", nseg, max_file_seg);
  DS_REQUIRE(mode_l == 0 || mode_l == 1, DIFFSAL_E_ARG, "jpeg_decode: mode_l %d (0: RGB, 1: L)", mode_l);
  const Geom g = geom(N, H, W, ncomp, hs, vs);
  DS_REQUIRE(ws_bytes >= g.bytes && aligned16(ws), DIFFSAL_E_ARG, "jpeg_decode: workspace too small (%zu of %zu bytes) or misaligned", ws_bytes, g.bytes);
  DS_REQUIRE((reinterpret_cast<uintptr_t>(status) & 3u) == 0 && (reinterpret_cast<uintptr_t>(segments) & 3u) == 0 &&
                 (reinterpret_cast<uintptr_t>(files) & 3u) == 0,
             DIFFSAL_E_ARG, "jpeg_decode: status, segments or files misaligned");
  const long groups = (W + kRowPixels - 1) / kRowPixels;
  const long tgrid = (g.nblk + kThreads - 1) / kThreads, cgrid = (groups * H + kThreads - 1) / kThreads;
  DS_REQUIRE(tgrid <= 0x7FFFFFFFL && cgrid <= 0x7FFFFFFFL, DIFFSAL_E_SHAPE, "jpeg_decode: %d x %d exceeds the grid", H, W);
  char* base = static_cast<char*>(ws);
  int* st = reinterpret_cast<int*>(base + g.status);
  short* coef = reinterpret_cast<short*>(base + g.coef);
  unsigned char* planes = reinterpret_cast<unsigned char*>(base + g.planes);
  hipStream_t s = static_cast<hipStream_t>(stream);
  int rc;
  if (hipMemsetAsync(base, 0, g.clear, s) != hipSuccess) {
    (void)hipGetLastError();
    set_error("jpeg_decode: clearing the coefficients failed");
    return DIFFSAL_E_LAUNCH;
  }
  const FileDesc* fd = static_cast<const FileDesc*>(files);
  hipLaunchKernelGGL(jpeg_entropy_kernel, dim3(static_cast<unsigned>((max_file_seg + kSegThreads - 1) / kSegThreads), N), dim3(kSegThreads), 0, s,
                     reinterpret_cast<const uint32_t*>(bytes), nbytes, fd, reinterpret_cast<const Segment*>(segments), nseg, g, coef, st);
  if ((rc = check_launch("jpeg_decode(entropy)"))) return rc;
  hipLaunchKernelGGL(jpeg_transform_kernel, dim3(static_cast<unsigned>(tgrid), N), dim3(kThreads), 0, s, fd, g, coef, planes);
  if ((rc = check_launch("jpeg_decode(transform)"))) return rc;
  const int vec = (W % kRowPixels == 0 && aligned16(out)) ? 1 : 0;
  const dim3 grid(static_cast<unsigned>(cgrid), N);
  if (mode_l)
    hipLaunchKernelGGL((jpeg_colour_kernel<true>), grid, dim3(kThreads), 0, s, g, planes, static_cast<int>(groups), out, st, status, vec);
  else
    hipLaunchKernelGGL((jpeg_colour_kernel<false>), grid, dim3(kThreads), 0, s, g, planes, static_cast<int>(groups), out, st, status, vec);
  return check_launch("jpeg_decode(colour)");
}
