// From PCM samples to the audio tensor forward_vggish reads: the host pipeline of R/datasets/saliency_db.py:449-497 (get_mel_feature),
// R/datasets/torchvggish/vggish_input.py:30-82 (waveform_to_examples), R/datasets/torchvggish/mel_features.py:71-223 (log-mel) and
// R/datasets/saliency_db.py:303-305,351-354 (resize and stack).  include/diffsal.h ("audio front end") states the arithmetic; two
// launches, three for input at another rate than 16 kHz, all on the caller's stream:
//   logmel           per (clip, 8 frames): the 1520 samples the frames span, read straight from the video's waveform (the centring
//                    and the zero padding of the excerpt are index arithmetic) and kept in LDS as fp64; re / im of the 235 bins that
//                    carry mel weight as a direct DFT of length 400 against the host-built basis hann[n] (cos, sin)(2 pi n k / 512);
//                    magnitudes to LDS; 64 banded mel sums of at most 17 terms; log(x + 0.01); one rounding to fp32
//   examples_resize  per output pixel: the example index map, then the bilinear resize in torch's fp32 arithmetic
//   resample_excerpts (opt-in, in front of logmel for input at another rate) per (clip, 256 outputs): resampy's band-limited sinc
//                    interpolation of the zero-padded, centred excerpt (csrc/audio_resample.h holds the arithmetic, shared with
//                    tools/resample_host_check.cpp).  The span of the padded buffer the tile reads (at 22050 -> 16000: 353 + 2 x 88
//                    samples) goes to LDS once, as fp64, zeros by index; a thread owns one output and walks its left wing, then its
//                    right wing, one 16-byte (win, delta) load from the L2-resident table and one LDS read per tap, every
//                    operation rounded on its own.  A tile whose span misses the excerpt writes zeros without reading the table.
// Transform form: a direct DFT in plain fp64 FMA, not an FFT.  K is 400 (the window, not the padded 512), 235 of 257 bins are
// needed and no bit reversal or twiddle bookkeeping exists; a thread owns 2 bins x 8 frames (32 accumulators) and walks n in
// ascending order, so each sum has one fixed order whatever the batch.  Per n a thread reads 2 basis pairs (16 bytes each,
// coalesced over bins, 1.6 MB in all: L2-resident) and 8 samples that every lane of the workgroup shares (LDS broadcasts).
// No atomics, no allocation, no synchronisation: two calls give the same bits and a call can be captured in a graph.
#include "common.h"
#include "audio_resample.h"

namespace diffsal {

constexpr int AI_WIN = 400;          // STFT window
constexpr int AI_HOP = 160;          // STFT hop
constexpr int AI_BINS = 235;         // rfft bins 5 .. 239
constexpr int AI_PITCH = 256;        // bins per basis row (235 .. 255 zero)
constexpr int AI_MEL = 64;
constexpr int AI_TAPS = 17;          // widest band
constexpr int AI_FT = 8;             // frames per workgroup
constexpr int AI_SPAN = (AI_FT - 1) * AI_HOP + AI_WIN;      // 1520 samples
constexpr int AI_THREADS = 128;      // thread t owns bins t and t + 128
constexpr int AI_EX_FRAMES = 64, AI_EX_HOP = 11, AI_EX = 9;
constexpr long AI_TABLE_DOUBLES = 2L * AI_WIN * AI_PITCH + AI_MEL * AI_TAPS + AI_MEL;
static_assert(AI_PITCH == 2 * AI_THREADS && AI_BINS <= AI_PITCH, "a thread owns columns t and t + AI_THREADS of a basis row");

template <typename T> __device__ __forceinline__ double ai_sample(const T* p, long i);
template <> __device__ __forceinline__ double ai_sample<short>(const short* p, long i) { return static_cast<double>(p[i]) / 32768.0; }
template <> __device__ __forceinline__ double ai_sample<float>(const float* p, long i) { return static_cast<double>(p[i]); }
template <> __device__ __forceinline__ double ai_sample<double>(const double* p, long i) { return p[i]; }

template <typename T, typename OUT>
__global__ __launch_bounds__(AI_THREADS) void ai_logmel_kernel(const T* __restrict__ wav, long Lmax, int V, const long* __restrict__ wav_len,
                                                               const int* __restrict__ video, const int* __restrict__ starts,
                                                               const int* __restrict__ ends, int window, int n_frames,
                                                               const double* __restrict__ tables, OUT* __restrict__ out) {
  __shared__ double xs[AI_SPAN];
  __shared__ double mag[AI_FT][AI_PITCH];
  __shared__ double melw[AI_MEL * AI_TAPS];
  __shared__ int mel0[AI_MEL];
  const int t = threadIdx.x, b = blockIdx.y, f0 = blockIdx.x * AI_FT;

  // the excerpt wav[start : end + 1] as numpy slices it (both ends clamped to the video's length), centred in the window
  int vid = video ? video[b] : 0;
  vid = vid < 0 ? 0 : (vid >= V ? V - 1 : vid);
  long n = wav_len ? wav_len[vid] : Lmax;
  n = n < 0 ? 0 : (n > Lmax ? Lmax : n);
  const long st = starts[b] < 0 ? 0 : starts[b], en = ends[b] < 0 ? 0 : ends[b];
  const long lo = st < n ? st : n, hi = en + 1 < n ? en + 1 : n;
  const long v = hi > lo ? hi - lo : 0;
  const long off = window / 2 - v / 2;      // may be negative for an unchecked v > window: the excerpt is then centre-cropped
  const T* src = wav + static_cast<long>(vid) * Lmax + lo;
  for (int i = t; i < AI_SPAN; i += AI_THREADS) {
    const long p = static_cast<long>(f0) * AI_HOP + i;      // position in the padded window
    const long j = p - off;
    xs[i] = (p < window && j >= 0 && j < v) ? ai_sample<T>(src, j) : 0.0;
  }
  const double* mt = tables + 2L * AI_WIN * AI_PITCH;
  for (int i = t; i < AI_MEL * AI_TAPS; i += AI_THREADS) melw[i] = mt[i];
  if (t < AI_MEL) {
    const int c = static_cast<int>(mt[AI_MEL * AI_TAPS + t]);
    mel0[t] = c < 0 ? 0 : (c > AI_PITCH - AI_TAPS ? AI_PITCH - AI_TAPS : c);      // a band's 17 taps stay inside a row of mag
  }
  __syncthreads();

  double re0[AI_FT], im0[AI_FT], re1[AI_FT], im1[AI_FT];
#pragma unroll
  for (int f = 0; f < AI_FT; ++f) { re0[f] = im0[f] = re1[f] = im1[f] = 0.0; }
  const double2* basis = reinterpret_cast<const double2*>(tables);
#pragma unroll 2
  for (int i = 0; i < AI_WIN; ++i) {
    const double2 c0 = basis[i * AI_PITCH + t], c1 = basis[i * AI_PITCH + t + AI_THREADS];
#pragma unroll
    for (int f = 0; f < AI_FT; ++f) {
      const double x = xs[f * AI_HOP + i];
      re0[f] = fma(x, c0.x, re0[f]); im0[f] = fma(x, c0.y, im0[f]);
      re1[f] = fma(x, c1.x, re1[f]); im1[f] = fma(x, c1.y, im1[f]);
    }
  }
#pragma unroll
  for (int f = 0; f < AI_FT; ++f) {
    mag[f][t] = hypot(re0[f], im0[f]);
    mag[f][t + AI_THREADS] = hypot(re1[f], im1[f]);
  }
  __syncthreads();

  for (int o = t; o < AI_FT * AI_MEL; o += AI_THREADS) {
    const int f = o >> 6, m = o & 63;
    if (f0 + f >= n_frames) break;
    const double* mg = &mag[f][mel0[m]];
    const double* w = &melw[m * AI_TAPS];
    double acc = 0.0;
#pragma unroll
    for (int k = 0; k < AI_TAPS; ++k) acc = fma(mg[k], w[k], acc);
    out[(static_cast<long>(b) * n_frames + f0 + f) * AI_MEL + m] = static_cast<OUT>(log(acc + 0.01));
  }
}

// One axis of torch's upsample_bilinear2d (align_corners=False) in fp32: the source position is ONE fused multiply-add,
// scale * (dst + 0.5) - 0.5, clamped at 0; index 0 is its truncation, weight 1 the remainder, weight 0 = 1 - weight 1.
__device__ __forceinline__ void ai_axis(int dst, float scale, int n_in, int& i0, int& i1, float& w0, float& w1) {
  float s = __fmaf_rn(scale, __fadd_rn(static_cast<float>(dst), 0.5f), -0.5f);
  s = s < 0.0f ? 0.0f : s;
  i0 = static_cast<int>(s);
  i0 = i0 < n_in - 1 ? i0 : n_in - 1;
  w1 = fminf(fmaxf(__fsub_rn(s, static_cast<float>(i0)), 0.0f), 1.0f);
  w0 = __fsub_rn(1.0f, w1);
  i1 = i0 + (i0 < n_in - 1 ? 1 : 0);
}

// w0 * a + w1 * b as torch's vectorised kernel rounds it: the second product rounded, the first fused into the sum
__device__ __forceinline__ float ai_lerp(float w0, float a, float w1, float b) { return __fmaf_rn(w0, a, __fmul_rn(w1, b)); }

__global__ __launch_bounds__(256) void ai_examples_resize_kernel(const float* __restrict__ lm, const unsigned char* __restrict__ exists,
                                                                 int n_frames, int E, int h, int w, float sy, float sx, long total,
                                                                 float* __restrict__ out) {
  const long idx = static_cast<long>(blockIdx.x) * 256 + threadIdx.x;
  if (idx >= total) return;
  const int x = static_cast<int>(idx % w);
  long r = idx / w;
  const int y = static_cast<int>(r % h);
  r /= h;
  const int j = static_cast<int>(r % AI_EX), b = static_cast<int>(r / AI_EX);
  if (exists && !exists[b]) { out[idx] = 0.0f; return; }
  int e = j;
  if (E < AI_EX) { const int rep = AI_EX / E; e = j < E * rep ? j / rep : (j - E * rep) / rep; }
  int y0, y1, x0, x1;
  float wy0, wy1, wx0, wx1;
  ai_axis(y, sy, AI_EX_FRAMES, y0, y1, wy0, wy1);
  ai_axis(x, sx, AI_MEL, x0, x1, wx0, wx1);
  const float* p = lm + (static_cast<long>(b) * n_frames + e * AI_EX_HOP) * AI_MEL;
  const float t0 = ai_lerp(wx0, p[y0 * AI_MEL + x0], wx1, p[y0 * AI_MEL + x1]);
  const float t1 = ai_lerp(wx0, p[y1 * AI_MEL + x0], wx1, p[y1 * AI_MEL + x1]);
  out[idx] = ai_lerp(wy0, t0, wy1, t1);
}

template <typename T>
__global__ __launch_bounds__(resample::kTile) void ai_resample_kernel(const T* __restrict__ wav, long Lmax, int V, const long* __restrict__ wav_len,
                                                                      const int* __restrict__ video, const int* __restrict__ starts,
                                                                      const int* __restrict__ ends, int window, resample::Plan plan,
                                                                      const double2* __restrict__ table, int nwin, int num_table,
                                                                      int n_samples, double* __restrict__ out) {
  extern __shared__ double rs_xs[];      // plan.max_span samples
  const int b = blockIdx.y;
  const int t0 = blockIdx.x * resample::kTile, t = t0 + threadIdx.x;
  const int t1 = t0 + resample::kTile - 1 < n_samples - 1 ? t0 + resample::kTile - 1 : n_samples - 1;
  int vid = video ? video[b] : 0;
  vid = vid < 0 ? 0 : (vid >= V ? V - 1 : vid);
  const resample::Excerpt e = resample::excerpt(starts[b], ends[b], wav_len ? wav_len[vid] : Lmax, Lmax, window);
  int base, span;
  resample::tile_span(t0, t1, plan.inc, plan.wing, base, span);
  span = span < plan.max_span ? span : plan.max_span;      // the launch's LDS; max_span bounds every tile (tools/resample_host_check.cpp walks them)
  double* o = out + static_cast<long>(b) * n_samples;
  // the part of the excerpt inside the window is positions max(off, 0) .. min(off + v, window) - 1
  const long first = e.off > 0 ? e.off : 0, last = (e.off + e.v < window ? e.off + e.v : window) - 1;
  if (last < base || first >= base + span || last < first) {      // every sample the tile reads is a zero of the padding
    if (t < n_samples) o[t] = 0.0;
    return;
  }
  const T* src = wav + static_cast<long>(vid) * Lmax;
  for (int i = threadIdx.x; i < span; i += resample::kTile) {
    const long j = resample::source_index(e, base + i, window);
    rs_xs[i] = j >= 0 ? ai_sample<T>(src, j) : 0.0;
  }
  __syncthreads();
  if (t < n_samples) o[t] = resample::output(t, rs_xs, base, table, nwin, num_table, plan.scale, plan.inc, plan.step, window);
}

static inline int ai_frames(long window) { return window >= AI_WIN ? static_cast<int>(1 + (window - AI_WIN) / AI_HOP) : 0; }
static inline int ai_examples(long window) { const int F = ai_frames(window); return F >= AI_EX_FRAMES ? 1 + (F - AI_EX_FRAMES) / AI_EX_HOP : 0; }

template <typename T>
static void ai_logmel_launch(dim3 grid, hipStream_t s, const void* wav, long Lmax, int V, const long* wav_len, const int* video,
                             const int* starts, const int* ends, int window, int n_frames, const double* tables, void* out, int out_f64) {
  if (out_f64)
    hipLaunchKernelGGL((ai_logmel_kernel<T, double>), grid, dim3(AI_THREADS), 0, s, static_cast<const T*>(wav), Lmax, V, wav_len, video, starts,
                       ends, window, n_frames, tables, static_cast<double*>(out));
  else
    hipLaunchKernelGGL((ai_logmel_kernel<T, float>), grid, dim3(AI_THREADS), 0, s, static_cast<const T*>(wav), Lmax, V, wav_len, video, starts,
                       ends, window, n_frames, tables, static_cast<float*>(out));
}

}  // namespace diffsal

using namespace diffsal;

extern "C" long diffsal_logmel_table_doubles(void) { return AI_TABLE_DOUBLES; }

extern "C" int diffsal_logmel(const void* wav, int wav_dtype, int V, long Lmax, const long* wav_len, const int* video, const int* starts,
                              const int* ends, int B, int sample_rate, int window, int n_frames, const double* tables, int out_f64,
                              void* out, diffsal_stream_t stream) {
  DS_REQUIRE(sample_rate == 16000, DIFFSAL_E_ARG,
             "logmel: sample_rate %d: the front end takes 16000 Hz input only (resampling is not built: resample on load)", sample_rate);
  DS_REQUIRE(wav_dtype == DIFFSAL_WAV_I16 || wav_dtype == DIFFSAL_WAV_F32 || wav_dtype == DIFFSAL_WAV_F64, DIFFSAL_E_ARG,
             "logmel: wav_dtype %d (DIFFSAL_WAV_I16, DIFFSAL_WAV_F32 or DIFFSAL_WAV_F64)", wav_dtype);
  DS_REQUIRE(out_f64 == 0 || out_f64 == 1, DIFFSAL_E_ARG, "logmel: out_f64 is 0 or 1");
  DS_REQUIRE(B > 0 && B <= 65535 && V > 0 && Lmax > 0 && Lmax < (1L << 31), DIFFSAL_E_SHAPE,
             "logmel: bad shape B=%d (1..65535) V=%d Lmax=%ld (1..2^31-1)", B, V, Lmax);
  DS_REQUIRE(window >= AI_WIN && window <= (1 << 24), DIFFSAL_E_SHAPE, "logmel: window of %d samples (one frame needs %d; at most 2^24)",
             window, AI_WIN);
  DS_REQUIRE(n_frames >= 1 && n_frames <= ai_frames(window), DIFFSAL_E_SHAPE, "logmel: %d frames asked of a window that holds %d", n_frames,
             ai_frames(window));
  DS_REQUIRE(wav && starts && ends && tables && out, DIFFSAL_E_ARG, "logmel: null argument");
  DS_REQUIRE(aligned16(tables), DIFFSAL_E_ARG, "logmel: tables must be 16-byte aligned");
  const dim3 grid((n_frames + AI_FT - 1) / AI_FT, B);
  hipStream_t s = static_cast<hipStream_t>(stream);
  if (wav_dtype == DIFFSAL_WAV_I16) ai_logmel_launch<short>(grid, s, wav, Lmax, V, wav_len, video, starts, ends, window, n_frames, tables, out, out_f64);
  else if (wav_dtype == DIFFSAL_WAV_F32) ai_logmel_launch<float>(grid, s, wav, Lmax, V, wav_len, video, starts, ends, window, n_frames, tables, out, out_f64);
  else ai_logmel_launch<double>(grid, s, wav, Lmax, V, wav_len, video, starts, ends, window, n_frames, tables, out, out_f64);
  return check_launch("logmel");
}

extern "C" long diffsal_resample_length(long n, int sr_orig, int sr_new) {
  if (n < 0 || n > (1L << 31) || sr_orig < 1 || sr_new < 1) return -1;
  return resample::out_len(n, sr_orig, sr_new);
}

extern "C" int diffsal_resample_excerpts(const void* wav, int wav_dtype, int V, long Lmax, const long* wav_len, const int* video,
                                         const int* starts, const int* ends, int B, int window, int sr_orig, int sr_new, const double* table,
                                         int nwin, int num_table, int n_samples, double* out, diffsal_stream_t stream) {
  DS_REQUIRE(sr_orig > 0 && sr_new > 0, DIFFSAL_E_ARG, "resample_excerpts: rates %d -> %d must be positive", sr_orig, sr_new);
  DS_REQUIRE(sr_orig != sr_new, DIFFSAL_E_ARG, "resample_excerpts: rates %d -> %d are equal (the reference does not resample there)", sr_orig,
             sr_new);
  DS_REQUIRE(wav_dtype == DIFFSAL_WAV_I16 || wav_dtype == DIFFSAL_WAV_F32 || wav_dtype == DIFFSAL_WAV_F64, DIFFSAL_E_ARG,
             "resample_excerpts: wav_dtype %d (DIFFSAL_WAV_I16, DIFFSAL_WAV_F32 or DIFFSAL_WAV_F64)", wav_dtype);
  DS_REQUIRE(B > 0 && B <= 65535 && V > 0 && Lmax > 0 && Lmax < (1L << 31), DIFFSAL_E_SHAPE,
             "resample_excerpts: bad shape B=%d (1..65535) V=%d Lmax=%ld (1..2^31-1)", B, V, Lmax);
  DS_REQUIRE(window >= 1 && window <= (1 << 24), DIFFSAL_E_SHAPE, "resample_excerpts: window of %d samples (1..2^24)", window);
  DS_REQUIRE(nwin >= 2 && nwin <= (1 << 24) && num_table >= 1 && num_table <= (1 << 20), DIFFSAL_E_SHAPE,
             "resample_excerpts: table of %d entries (2..2^24), %d per zero crossing (1..2^20)", nwin, num_table);
  const resample::Plan plan = resample::plan(sr_orig, sr_new, nwin, num_table);
  DS_REQUIRE(plan.step >= 1 && plan.wing >= 1, DIFFSAL_E_SHAPE,
             "resample_excerpts: %d -> %d with %d table entries per zero crossing steps %d entries per tap through a table of %d", sr_orig, sr_new,
             num_table, plan.step, nwin);
  DS_REQUIRE(plan.max_span <= resample::kMaxSpan, DIFFSAL_E_SHAPE,
             "resample_excerpts: %d -> %d with this table reads %d input samples per %d outputs, more than the %d a workgroup stages", sr_orig,
             sr_new, plan.max_span, resample::kTile, resample::kMaxSpan);
  const long n_out = resample::out_len(window, sr_orig, sr_new);
  DS_REQUIRE(n_samples >= 1 && n_samples <= n_out, DIFFSAL_E_SHAPE, "resample_excerpts: %d samples asked of a window that gives %ld", n_samples,
             n_out);
  DS_REQUIRE(wav && starts && ends && table && out, DIFFSAL_E_ARG, "resample_excerpts: null argument");
  DS_REQUIRE(aligned16(table), DIFFSAL_E_ARG, "resample_excerpts: table must be 16-byte aligned");
  const dim3 grid((n_samples + resample::kTile - 1) / resample::kTile, B), block(resample::kTile);
  const size_t lds = static_cast<size_t>(plan.max_span) * sizeof(double);
  hipStream_t s = static_cast<hipStream_t>(stream);
  const double2* tab = reinterpret_cast<const double2*>(table);
  if (wav_dtype == DIFFSAL_WAV_I16)
    hipLaunchKernelGGL(ai_resample_kernel<short>, grid, block, lds, s, static_cast<const short*>(wav), Lmax, V, wav_len, video, starts, ends, window,
                       plan, tab, nwin, num_table, n_samples, out);
  else if (wav_dtype == DIFFSAL_WAV_F32)
    hipLaunchKernelGGL(ai_resample_kernel<float>, grid, block, lds, s, static_cast<const float*>(wav), Lmax, V, wav_len, video, starts, ends, window,
                       plan, tab, nwin, num_table, n_samples, out);
  else
    hipLaunchKernelGGL(ai_resample_kernel<double>, grid, block, lds, s, static_cast<const double*>(wav), Lmax, V, wav_len, video, starts, ends,
                       window, plan, tab, nwin, num_table, n_samples, out);
  return check_launch("resample_excerpts");
}

extern "C" int diffsal_audio_examples(const float* logmel, const unsigned char* exists, int B, int n_frames, int n_examples, int h, int w,
                                      float* out, diffsal_stream_t stream) {
  DS_REQUIRE(n_examples >= 1, DIFFSAL_E_SHAPE, "audio_examples: %d examples: the window is too short for one example of %d frames", n_examples,
             AI_EX_FRAMES);
  const int used = n_examples < AI_EX ? n_examples : AI_EX;
  DS_REQUIRE(n_frames >= AI_EX_FRAMES + AI_EX_HOP * (used - 1), DIFFSAL_E_SHAPE, "audio_examples: %d log-mel frames, %d examples read %d",
             n_frames, used, AI_EX_FRAMES + AI_EX_HOP * (used - 1));
  DS_REQUIRE(B > 0 && B <= 65535 && h > 0 && w > 0 && h <= 4096 && w <= 4096, DIFFSAL_E_SHAPE,
             "audio_examples: bad shape B=%d (1..65535) h=%d w=%d (1..4096)", B, h, w);
  DS_REQUIRE(logmel && out, DIFFSAL_E_ARG, "audio_examples: null argument");
  const long total = static_cast<long>(B) * AI_EX * h * w;
  DS_REQUIRE((total + 255) / 256 < (1L << 31), DIFFSAL_E_SHAPE, "audio_examples: %ld outputs", total);
  const float sy = static_cast<float>(AI_EX_FRAMES) / static_cast<float>(h), sx = static_cast<float>(AI_MEL) / static_cast<float>(w);
  hipLaunchKernelGGL(ai_examples_resize_kernel, dim3(static_cast<unsigned>((total + 255) / 256)), dim3(256), 0, static_cast<hipStream_t>(stream),
                     logmel, exists, n_frames, n_examples, h, w, sy, sx, total, out);
  return check_launch("audio_examples");
}
