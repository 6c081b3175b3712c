// The frame and map loaders of the visual sets (R/datasets/dhf1k_data.py:78, ucf_dataset.py:68, holly2wood_dataset.py:72:
// Image.open('%d.png').convert('RGB'); R/datasets/meta_data.py:49-57: .convert('L') of '%04d.png') on the device: the zlib
// streams of PNG files -> the uint8 frames Pillow returns, bit for bit.  include/diffsal.h ("PNG decode") states the arithmetic,
// csrc/png_decode_core.h holds it; two launches on the caller's stream, a wave per file in both (a deflate stream has no restart
// points and a row needs the row above: the parallelism is across files, and inside a file across the lanes of its wave):
//   inflate    all lanes walk the stream in step.  The stream is staged in LDS by halves of 4 KB with aligned 32-bit loads; the
//              code tables are built in LDS (counts and code order by one lane, the 9-bit look-up by a lane per code); deflate's
//              32 K history is a ring in LDS, so a match never waits for global memory: the lanes copy a match together, byte j
//              from (j mod distance) of the bytes in front of it, all reads before all writes; every 1024 bytes the ring goes out
//              to the file's filtered scanlines in the workspace with a 16-byte store per lane.  Every byte of the region is
//              written (zeros behind a short stream), so a dirty workspace changes nothing
//   unfilter   Adler-32 of the region (16 bytes per lane per tile of 1024, combined at the end), then bands of 64 rows on the
//              diagonal: at step t lane k reconstructs group t - k (four filter units) of row r0 + k; the group above is what
//              lane k - 1 made one step earlier and comes through __shfl_up, lane 0's from the band's LDS copy of the row above,
//              which lane 63 writes.  The raw bytes are loaded a step ahead.  Each group goes straight through sample unpacking,
//              the palette and Pillow's L into `out`, in 32-bit stores where the address allows
// Hostile bytes: stream reads are clamped to [off, off + len) of the packed buffer, region writes to the region, frame writes to
// x < W of row < H, and every loop is bounded by the geometry or the stream's bits (png_decode_core.h).
// tools/png_decode_host_check.cpp runs the same functions under a sanitizer.  Integer work only; no allocation, no
// synchronisation, no host copy.
#include "common.h"
#include "png_decode_core.h"

namespace diffsal {
namespace png {

__global__ __launch_bounds__(kLanes) void png_inflate_kernel(const uint32_t* __restrict__ words, long nbytes, const FileDesc* __restrict__ files, Geom g,
                                                             uint8_t* __restrict__ data, FileState* __restrict__ state) {
  __shared__ InflateShared s;
  const int f = blockIdx.x;
  inflate_file(s, words, nbytes, files[f].off, files[f].len, g, data + static_cast<long>(f) * g.region, state + f, nullptr);
}

__global__ __launch_bounds__(kLanes) void png_unfilter_kernel(const FileDesc* __restrict__ files, Geom g, const uint8_t* __restrict__ data,
                                                              const FileState* __restrict__ state, int mode_l, uint8_t* __restrict__ out,
                                                              int* __restrict__ status) {
  __shared__ UnfilterShared s;
  const int f = blockIdx.x;
  const int st = unfilter_file(s, g, files[f].pal, data + static_cast<long>(f) * g.region, state[f], mode_l,
                               out + static_cast<long>(f) * g.H * g.W * (mode_l ? 1 : 3), nullptr);
  if (threadIdx.x == 0) status[f] = st;
}

}  // namespace png
}  // namespace diffsal

using namespace diffsal;
using namespace diffsal::png;

extern "C" size_t diffsal_png_decode_ws_bytes(int N, int H, int W, int color_type, int bit_depth) {
  if (!geom_ok(N, H, W, color_type, bit_depth)) return 0;
  return geom(N, H, W, color_type, bit_depth).bytes;
}

extern "C" int diffsal_png_decode(const void* bytes, long nbytes, const void* files, int N, int H, int W, int color_type, int bit_depth,
                                  int mode_l, void* out, void* status, void* ws, size_t ws_bytes, diffsal_stream_t stream) {
  DS_REQUIRE(bytes && files && out && status && ws, DIFFSAL_E_ARG, "png_decode: null argument");
  DS_REQUIRE(geom_ok(N, H, W, color_type, bit_depth), DIFFSAL_E_SHAPE,
             "png_decode: N=%d (1..%d), %d x %d (H 1..%d, W 1..%d, below 2^31 filtered bytes), colour type %d at %d bits (8 bits: 0, 2, 3, 4, 6; "
             "1, 2, 4 bits: 0, 3)", N, kMaxN, H, W, kMaxH, kMaxW, color_type, bit_depth);
  DS_REQUIRE(nbytes >= 16 && nbytes % 16 == 0 && nbytes <= 0x7FFFFFF0L && aligned16(bytes), DIFFSAL_E_ARG,
             "png_decode: the packed streams must be 16-byte aligned and a multiple of 16 bytes below 2^31 (padded), got %ld", nbytes);
  DS_REQUIRE(mode_l == 0 || mode_l == 1, DIFFSAL_E_ARG, "png_decode: mode_l %d (0: RGB, 1: L)", mode_l);
  const Geom g = geom(N, H, W, color_type, bit_depth);
  DS_REQUIRE(ws_bytes >= g.bytes && aligned16(ws), DIFFSAL_E_ARG, "png_decode: workspace too small (%zu of %zu bytes) or misaligned", ws_bytes, g.bytes);
  DS_REQUIRE((reinterpret_cast<uintptr_t>(status) & 3u) == 0 && (reinterpret_cast<uintptr_t>(files) & 3u) == 0, DIFFSAL_E_ARG,
             "png_decode: status or files misaligned");
  char* base = static_cast<char*>(ws);
  FileState* st = reinterpret_cast<FileState*>(base + g.state);
  uint8_t* data = reinterpret_cast<uint8_t*>(base + g.data);
  const FileDesc* fd = static_cast<const FileDesc*>(files);
  hipStream_t s = static_cast<hipStream_t>(stream);
  int rc;
  hipLaunchKernelGGL(png_inflate_kernel, dim3(N), dim3(kLanes), 0, s, static_cast<const uint32_t*>(bytes), nbytes, fd, g, data, st);
  if ((rc = check_launch("png_decode(inflate)"))) return rc;
  hipLaunchKernelGGL(png_unfilter_kernel, dim3(N), dim3(kLanes), 0, s, fd, g, data, st, mode_l, static_cast<uint8_t*>(out), static_cast<int*>(status));
  return check_launch("png_decode(unfilter)");
}
