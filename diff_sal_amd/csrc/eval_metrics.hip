// Benchmark-protocol saliency metrics on the device: AUC-Judd, AUC-Borji, shuffled AUC against the binary fixation map and the
// benchmark forms of CC, NSS, SIM (R/metrics/metrics.py, driven by R/compute_metrics.py through PNG files and a numpy pool).
// include/diffsal.h ("benchmark metrics") states the arithmetic; the launches of one call, all on the caller's stream:
//   stats   per (image, chunk): min / max of the (optionally jittered) map, fp64 sums of pred and gt, fixation counts
//   image   per image: the chunk partials combined in chunk order, the chunks' offsets into the fixation lists
//   prep    per (image, chunk): S = (s - min) / (max - min) in fp32 (numpy's float32 arithmetic, bit for bit), the fixated
//           values / pixel indices compacted in pixel order, centred fp64 sums for CC / NSS, the SIM sum
//   count   AUC-Judd: above_i = #{j : S_j >= S_i} for every fixation i.  One wave per (image, chunk) keeps its 4096 pixels in
//           LDS and holds two fixation values per lane; a 16-byte LDS read feeds eight compares; the per-lane integer counts
//           go to above_i by integer atomic adds, so the result does not depend on the order of accumulation
//   rank    AUC-Judd: position k of every fixation in the descending order of the fixation values (ties in list order),
//           above_i scattered to slot k
//   sweep   AUC-Borji / sAUC: one workgroup per (image, repetition): integer histograms of the fixation values and of the
//           repetition's sampled values over the thresholds k * step, the repetition's trapezoid
//   final   per image: the Judd trapezoid in k order, the mean over repetitions in index order, CC / NSS / SIM, NaN rules
// Cost: count is O(n_fix n) compares per image and rank O(n_fix^2) on at most 64 workgroups per image.  Both are sized for eye-tracking
// maps, n_fix from a few to a few thousand (DHF1K frames: ~300; rank is then < 1 % of count).  A dense map (n_fix ~ n) is
// computed correctly by the same launches but at O(n^2) per image: seconds at 360 x 640.  Callers with such maps should not use Judd.
// Every count is an integer and every fp64 sum has a fixed order: two calls give the same bits.  No floating-point atomics,
// no allocation, no synchronisation; what a launch reads from an earlier one it reads behind a kernel boundary.
#include "common.h"

namespace diffsal {

constexpr int EM_CHUNK = 4096;     // pixels per workgroup of the streaming passes = pixels one wave of the count pass keeps in LDS
constexpr int EM_TILE = 128;       // fixations per tile of the count pass: two per lane
constexpr int EM_MAX_T = 1024;     // most thresholds of a Borji sweep (step >= 1 / 1024: the map's maximum is 1)
constexpr int P1 = 8;              // doubles per chunk partial of `stats`
constexpr int P3 = 5;              // doubles per chunk partial of `prep`
constexpr int IM = 12;             // doubles per image record
constexpr uint32_t EM_DRAW = 0x40000000u;   // | purpose: 0 jitter, 1 Borji locations, 2 sAUC keys

enum { T_JUDD = 1, T_BORJI = 2, T_SAUC = 4, T_CC = 8, T_NSS = 16, T_SIM = 32, T_JITTER = 64 };
// image record (doubles): 0 sum s, 1 sum g, 2 min s', 3 max s', 4 min g, 5 max g, 6 min s, 7 max s, 8 mean s, 9 mean g
// image record (ints):    0 n_fix, 1 n_other, 2 degenerate (no fixation, every pixel fixated or a flat map)

// The [B][n] arrays exist only for the terms that read them (null otherwise: `prep` skips a null list); n_fix may be n - 1, so a
// list has n slots per image.  All six metrics at B = 64, 360 x 640: 6 x 59 MB = 354 MB; CC / NSS / SIM alone: a few KB.
struct EmWs {
  float* S;            // [B][n] range-normalised map                                   judd, borji, sauc
  float* fix_val;      // [B][n] S at the fixated pixels, pixel order (n_fix used)      judd, borji, sauc
  int* fix_idx;        // [B][n] their linear pixel indices                             borji
  int* oth_idx;        // [B][n] fixated pixels of `other`                              sauc
  unsigned* above;     // [B][n] Judd counts per fixation                               judd
  unsigned* sorted;    // [B][n] the same in descending order of value                  judd
  double* p1;          // [B][C][P1]
  double* p3;          // [B][C][P3]
  double* img;         // [B][IM]
  double* rep;         // [2][B][n_rep] per-repetition areas (Borji, sAUC)
  int* pc;             // [B][C][2] fixation counts per chunk, then their exclusive prefix
  int* imgi;           // [B][4]
  size_t bytes;
};

static inline long em_chunks(long n) { return (n + EM_CHUNK - 1) / EM_CHUNK; }

static EmWs em_layout(void* base, int B, long n, unsigned terms, int n_rep) {
  EmWs w;
  char* p = static_cast<char*>(base);
  size_t off = 0;
  auto take = [&](size_t bytes) { char* r = p + off; off += (bytes + 15) & ~static_cast<size_t>(15); return r; };
  const size_t bn = static_cast<size_t>(B) * n, bc = static_cast<size_t>(B) * em_chunks(n);
  w.p1 = reinterpret_cast<double*>(take(bc * P1 * 8));
  w.p3 = reinterpret_cast<double*>(take(bc * P3 * 8));
  w.img = reinterpret_cast<double*>(take(static_cast<size_t>(B) * IM * 8));
  w.rep = reinterpret_cast<double*>(take(static_cast<size_t>(2) * B * (n_rep > 0 ? n_rep : 1) * 8));
  auto list = [&](unsigned users) -> char* { return (terms & users) ? take(bn * 4) : nullptr; };
  w.S = reinterpret_cast<float*>(list(T_JUDD | T_BORJI | T_SAUC));
  w.fix_val = reinterpret_cast<float*>(list(T_JUDD | T_BORJI | T_SAUC));
  w.fix_idx = reinterpret_cast<int*>(list(T_BORJI));
  w.oth_idx = reinterpret_cast<int*>(list(T_SAUC));
  w.above = reinterpret_cast<unsigned*>(list(T_JUDD));
  w.sorted = reinterpret_cast<unsigned*>(list(T_JUDD));
  w.pc = reinterpret_cast<int*>(take(bc * 2 * 4));
  w.imgi = reinterpret_cast<int*>(take(static_cast<size_t>(B) * 4 * 4));
  w.bytes = off;
  return w;
}

// ---- block-wide reductions of 256 threads in a fixed order: lanes by xor butterfly, then the four waves in index order ----
template <typename T, typename Op>
__device__ __forceinline__ T block_all(T v, Op op, T* sh) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = op(v, __shfl_xor(v, o, kWave));
  const int nw = blockDim.x >> 6;
  __syncthreads();      // sh may still be read from the previous reduction
  if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = v;
  __syncthreads();
  T r = sh[0];
  for (int w = 1; w < nw; ++w) r = op(r, sh[w]);
  return r;
}
struct OpAdd { template <typename T> __device__ T operator()(T a, T b) const { return a + b; } };
struct OpMin { __device__ double operator()(double a, double b) const { return fmin(a, b); } };
struct OpMax { __device__ double operator()(double a, double b) const { return fmax(a, b); } };

// pixel i of image b with the jitter of R/metrics/metrics.py:44-45 from the evaluation stream (purpose 0, element i)
__device__ __forceinline__ float em_value(const float* __restrict__ pb, long i, bool jitter, const long long* __restrict__ ids,
                                          const unsigned long long* __restrict__ seed, int b) {
  float s = pb[i];
  if (jitter) {
    uint32_t r[4];
    philox_quad(ids, seed, b, static_cast<uint32_t>(i >> 2), EM_DRAW, r);
    const int e = static_cast<int>(i & 3);
    const uint32_t w = e == 0 ? r[0] : (e == 1 ? r[1] : (e == 2 ? r[2] : r[3]));
    const double u = static_cast<double>(w >> 8) * 0x1p-24;
    s = static_cast<float>(__dadd_rn(static_cast<double>(s), __dmul_rn(u, 1e-7)));      // no fma: numpy rounds the product
  }
  return s;
}

__global__ __launch_bounds__(256) void em_stats_kernel(const float* __restrict__ pred, const unsigned char* __restrict__ fix,
                                                       const float* __restrict__ gt, const unsigned char* __restrict__ other,
                                                       double* __restrict__ p1, int* __restrict__ pc, long n, int jitter,
                                                       const long long* __restrict__ ids, const unsigned long long* __restrict__ seed) {
  __shared__ double shd[4];
  __shared__ int shi[4];
  const int b = blockIdx.y;
  const long C = gridDim.x, chunk = blockIdx.x;
  const long lo = chunk * EM_CHUNK, hi = lo + EM_CHUNK < n ? lo + EM_CHUNK : n;
  const float* pb = pred + static_cast<long>(b) * n;
  const float* gb = gt ? gt + static_cast<long>(b) * n : nullptr;
  const unsigned char* fb = fix ? fix + static_cast<long>(b) * n : nullptr;
  const unsigned char* ob = other ? other + static_cast<long>(b) * n : nullptr;
  double ss = 0, sg = 0, mnj = 1e300, mxj = -1e300, mng = 1e300, mxg = -1e300, mns = 1e300, mxs = -1e300;
  int nf = 0, no = 0;
  for (long i = lo + threadIdx.x; i < hi; i += 256) {
    const double s = pb[i];
    ss += s; mns = fmin(mns, s); mxs = fmax(mxs, s);
    const double sj = jitter ? static_cast<double>(em_value(pb, i, true, ids, seed, b)) : s;
    mnj = fmin(mnj, sj); mxj = fmax(mxj, sj);
    if (gb) { const double g = gb[i]; sg += g; mng = fmin(mng, g); mxg = fmax(mxg, g); }
    if (fb) nf += fb[i] != 0;
    if (ob) no += ob[i] != 0;
  }
  double v[8];
  v[0] = block_all(ss, OpAdd(), shd); v[1] = block_all(sg, OpAdd(), shd);
  v[2] = block_all(mnj, OpMin(), shd); v[3] = block_all(mxj, OpMax(), shd);
  v[4] = block_all(mng, OpMin(), shd); v[5] = block_all(mxg, OpMax(), shd);
  v[6] = block_all(mns, OpMin(), shd); v[7] = block_all(mxs, OpMax(), shd);
  nf = block_all(nf, OpAdd(), shi); no = block_all(no, OpAdd(), shi);
  if (threadIdx.x == 0) {
    double* o = p1 + (static_cast<long>(b) * C + chunk) * P1;
    for (int i = 0; i < 8; ++i) o[i] = v[i];
    pc[(static_cast<long>(b) * C + chunk) * 2] = nf;
    pc[(static_cast<long>(b) * C + chunk) * 2 + 1] = no;
  }
}

__global__ __launch_bounds__(256) void em_image_kernel(const double* __restrict__ p1, int* __restrict__ pc, double* __restrict__ img,
                                                       int* __restrict__ imgi, long n, long C) {
  __shared__ double shd[4];
  const int b = blockIdx.x;
  double ss = 0, sg = 0, mnj = 1e300, mxj = -1e300, mng = 1e300, mxg = -1e300, mns = 1e300, mxs = -1e300;
  for (long c = threadIdx.x; c < C; c += 256) {
    const double* p = p1 + (static_cast<long>(b) * C + c) * P1;
    ss += p[0]; sg += p[1];
    mnj = fmin(mnj, p[2]); mxj = fmax(mxj, p[3]); mng = fmin(mng, p[4]); mxg = fmax(mxg, p[5]);
    mns = fmin(mns, p[6]); mxs = fmax(mxs, p[7]);
  }
  ss = block_all(ss, OpAdd(), shd); sg = block_all(sg, OpAdd(), shd);
  mnj = block_all(mnj, OpMin(), shd); mxj = block_all(mxj, OpMax(), shd);
  mng = block_all(mng, OpMin(), shd); mxg = block_all(mxg, OpMax(), shd);
  mns = block_all(mns, OpMin(), shd); mxs = block_all(mxs, OpMax(), shd);
  if (threadIdx.x == 0) {
    int nf = 0, no = 0;
    for (long c = 0; c < C; ++c) {      // counts -> exclusive prefix, in place
      int* q = pc + (static_cast<long>(b) * C + c) * 2;
      const int a = q[0], o = q[1];
      q[0] = nf; q[1] = no;
      nf += a; no += o;
    }
    double* o = img + static_cast<long>(b) * IM;
    o[0] = ss; o[1] = sg; o[2] = mnj; o[3] = mxj; o[4] = mng; o[5] = mxg; o[6] = mns; o[7] = mxs;
    o[8] = ss / static_cast<double>(n); o[9] = sg / static_cast<double>(n);
    int* oi = imgi + b * 4;
    oi[0] = nf; oi[1] = no;
    oi[2] = (nf == 0 || nf == n || !(mxj > mnj)) ? 1 : 0;
  }
}

__global__ __launch_bounds__(256) void em_prep_kernel(const float* __restrict__ pred, const unsigned char* __restrict__ fix,
                                                      const float* __restrict__ gt, const unsigned char* __restrict__ other,
                                                      const double* __restrict__ img, const int* __restrict__ pc,
                                                      float* __restrict__ S, float* __restrict__ fix_val, int* __restrict__ fix_idx,
                                                      int* __restrict__ oth_idx, unsigned* __restrict__ above,
                                                      double* __restrict__ p3, long n, int jitter,
                                                      const long long* __restrict__ ids, const unsigned long long* __restrict__ seed) {
  __shared__ double shd[4];
  __shared__ int wf[4], wo[4];
  const int b = blockIdx.y, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const long C = gridDim.x, chunk = blockIdx.x;
  const long lo = chunk * EM_CHUNK, hi = lo + EM_CHUNK < n ? lo + EM_CHUNK : n;
  const long bo = static_cast<long>(b) * n;
  const float* pb = pred + bo;
  const float* gb = gt ? gt + bo : nullptr;
  const unsigned char* fb = fix ? fix + bo : nullptr;
  const unsigned char* ob = other ? other + bo : nullptr;
  const double* m = img + static_cast<long>(b) * IM;
  const float mn = static_cast<float>(m[2]), mx = static_cast<float>(m[3]);      // exact: both are float values
  const float range = mx - mn;
  const double nn = static_cast<double>(n), mean_s = m[8], mean_g = m[9];
  // SIM: range normalisation, then sum normalisation, on the fp64 copies of the raw maps (metrics.py:246-249)
  const double rs = m[7] - m[6], rg = m[5] - m[4];
  const double sum_sn = (m[0] - nn * m[6]) / rs, sum_gn = (m[1] - nn * m[4]) / rg;
  int basef = pc[(static_cast<long>(b) * C + chunk) * 2], baseo = pc[(static_cast<long>(b) * C + chunk) * 2 + 1];
  double css = 0, cgg = 0, csg = 0, fs = 0, sim = 0;
  for (long i0 = lo; i0 < hi; i0 += 256) {      // uniform trip count: the barriers below are reached by every thread
    const long i = i0 + threadIdx.x;
    const bool in = i < hi;
    bool f = false, o = false;
    float sn = 0.f;
    if (in) {
      const float sj = em_value(pb, i, jitter != 0, ids, seed, b);
      sn = (sj - mn) / range;      // one fp32 subtraction, one IEEE fp32 division: R/metrics/utils.py:47 on a float32 map
      if (S) S[bo + i] = sn;
      f = fb && fb[i] != 0;
      o = ob && ob[i] != 0;
      const double s = pb[i], ds = s - mean_s;
      css += ds * ds;
      if (f) fs += ds;
      if (gb) {
        const double g = gb[i], dg = g - mean_g;
        cgg += dg * dg; csg += ds * dg;
        sim += fmin((s - m[6]) / rs / sum_sn, (g - m[4]) / rg / sum_gn);
      }
    }
    // ordered compaction: lanes by ballot, waves by a four-entry table, iterations by the running bases
    const unsigned long long bf = __ballot(f), bo_ = __ballot(o);
    const unsigned long long below = (1ull << lane) - 1ull;
    if (lane == 0) { wf[wave] = __popcll(bf); wo[wave] = __popcll(bo_); }
    __syncthreads();
    int pf = basef, po = baseo, tf = 0, to = 0;
    for (int w = 0; w < 4; ++w) {
      if (w < wave) { pf += wf[w]; po += wo[w]; }
      tf += wf[w]; to += wo[w];
    }
    if (f) {
      const long slot = bo + pf + __popcll(bf & below);
      if (fix_val) fix_val[slot] = sn;
      if (fix_idx) fix_idx[slot] = static_cast<int>(i);
      if (above) above[slot] = 0u;
    }
    if (o && oth_idx) oth_idx[bo + po + __popcll(bo_ & below)] = static_cast<int>(i);
    basef += tf; baseo += to;
    __syncthreads();
  }
  css = block_all(css, OpAdd(), shd); cgg = block_all(cgg, OpAdd(), shd); csg = block_all(csg, OpAdd(), shd);
  fs = block_all(fs, OpAdd(), shd); sim = block_all(sim, OpAdd(), shd);
  if (threadIdx.x == 0) {
    double* q = p3 + (static_cast<long>(b) * C + chunk) * P3;
    q[0] = css; q[1] = cgg; q[2] = csg; q[3] = fs; q[4] = sim;
  }
}

// AUC-Judd counts.  One wave per (chunk, image): the chunk's normalised pixels sit in LDS (tail padded with NaN, which no compare
// passes), lane l holds fixations t0 + l and t0 + 64 + l of the current tile (NaN past n_fix) and reads the pixels four at a time:
// every lane reads the same 16 bytes (a broadcast, no bank conflict) and makes eight compares on them.
__global__ __launch_bounds__(64) void em_judd_count_kernel(const float* __restrict__ S, const float* __restrict__ fix_val,
                                                           const int* __restrict__ imgi, unsigned* __restrict__ above, long n) {
  __shared__ float4 px[EM_CHUNK / 4];
  const int b = blockIdx.y, lane = threadIdx.x;
  const int nf = imgi[b * 4];
  if (imgi[b * 4 + 2]) return;      // degenerate image: the result is NaN by definition (uniform exit, before the barrier)
  const long bo = static_cast<long>(b) * n, lo = static_cast<long>(blockIdx.x) * EM_CHUNK;
  const long left = n - lo < EM_CHUNK ? n - lo : EM_CHUNK;
  const float* sb = S + bo + lo;
  const float nanv = __builtin_nanf("");
  const bool vec = (reinterpret_cast<uintptr_t>(sb) & 15u) == 0;
  for (int q = lane; q < EM_CHUNK / 4; q += 64) {
    const long e = static_cast<long>(q) * 4;
    float4 v;
    if (vec && e + 3 < left) {
      v = *reinterpret_cast<const float4*>(sb + e);
    } else {
      v.x = e < left ? sb[e] : nanv; v.y = e + 1 < left ? sb[e + 1] : nanv;
      v.z = e + 2 < left ? sb[e + 2] : nanv; v.w = e + 3 < left ? sb[e + 3] : nanv;
    }
    px[q] = v;
  }
  __syncthreads();
  const int nq = static_cast<int>((left + 3) / 4);
  const float* fv = fix_val + bo;
  unsigned* ab = above + bo;
  for (int t0 = 0; t0 < nf; t0 += EM_TILE) {
    const int i0 = t0 + lane, i1 = t0 + 64 + lane;
    const float v0 = i0 < nf ? fv[i0] : nanv, v1 = i1 < nf ? fv[i1] : nanv;
    unsigned c0 = 0, c1 = 0;
#pragma unroll 4
    for (int q = 0; q < nq; ++q) {
      const float4 p = px[q];
      c0 += (p.x >= v0) + (p.y >= v0) + (p.z >= v0) + (p.w >= v0);
      c1 += (p.x >= v1) + (p.y >= v1) + (p.z >= v1) + (p.w >= v1);
    }
    if (i0 < nf && c0) atomicAdd(ab + i0, c0);
    if (i1 < nf && c1) atomicAdd(ab + i1, c1);
  }
}

// position k of fixation i in the descending order of the values; equal values take consecutive positions in list order
__global__ __launch_bounds__(256) void em_judd_rank_kernel(const float* __restrict__ fix_val, const unsigned* __restrict__ above,
                                                           const int* __restrict__ imgi, unsigned* __restrict__ sorted, long n) {
  const int b = blockIdx.y;
  const int nf = imgi[b * 4];
  if (imgi[b * 4 + 2]) return;
  const long bo = static_cast<long>(b) * n;
  const float* fv = fix_val + bo;
  for (int i = blockIdx.x * 256 + threadIdx.x; i < nf; i += gridDim.x * 256) {
    const float v = fv[i];
    int k = 0;
    for (int j = 0; j < nf; ++j) {
      const float u = fv[j];
      k += (u > v) || (u == v && j < i);
    }
    sorted[bo + k] = above[bo + i];
  }
}

// number of thresholds k * step (k < ntmax) that are <= v, compared in fp64 as numpy compares a float32 value with arange's doubles
__device__ __forceinline__ int em_nthr(float v, double step, int ntmax) {
  const double x = v;
  int c = static_cast<int>(floor(x / step)) + 1;
  c = c < 0 ? 0 : (c > ntmax ? ntmax : c);
  while (c > 0 && __dmul_rn(static_cast<double>(c - 1), step) > x) --c;
  while (c < ntmax && __dmul_rn(static_cast<double>(c), step) <= x) ++c;
  return c;
}

__device__ __forceinline__ uint32_t em_word(const long long* __restrict__ ids, const unsigned long long* __restrict__ seed, int b,
                                            unsigned long long e, uint32_t draw) {
  uint32_t r[4];
  philox_quad(ids, seed, b, static_cast<uint32_t>(e >> 2), draw, r);
  const int k = static_cast<int>(e & 3);
  return k == 0 ? r[0] : (k == 1 ? r[1] : (k == 2 ? r[2] : r[3]));
}

// One workgroup per (repetition, image).  mode 0: locations from rand_index [B][n_rep][cap] (-1 = unused slot); 1: Borji device
// generator (a location per fixated pixel); 2: sAUC device generator (the m = min(n_fix, n_other) pixels of `other` with the
// smallest (word, pixel) keys, found by an 8-pass radix select on the 64-bit key word << 32 | pixel: the keys are distinct).
__global__ __launch_bounds__(256) void em_sweep_kernel(const float* __restrict__ S, const float* __restrict__ fix_val,
                                                       const int* __restrict__ fix_idx, const int* __restrict__ oth_idx,
                                                       const int* __restrict__ imgi, const int* __restrict__ rand_index, int cap,
                                                       int mode, long n, int n_rep, double step, int ntmax,
                                                       const long long* __restrict__ ids, const unsigned long long* __restrict__ seed,
                                                       double* __restrict__ rep_out) {
  __shared__ unsigned hf[EM_MAX_T + 1], hr[EM_MAX_T + 1];
  __shared__ unsigned radix[256];
  __shared__ unsigned mxbits;
  __shared__ unsigned long long sel_prefix;
  __shared__ int sel_left;
  const int rep = blockIdx.x, b = blockIdx.y;
  const int nf = imgi[b * 4], no = imgi[b * 4 + 1];
  if (imgi[b * 4 + 2] || (mode == 2 && no == 0)) return;      // NaN by definition: `final` writes it
  const long bo = static_cast<long>(b) * n;
  const float* sb = S + bo;
  for (int i = threadIdx.x; i <= ntmax; i += 256) { hf[i] = 0u; hr[i] = 0u; }
  if (threadIdx.x == 0) mxbits = 0u;
  __syncthreads();
  // S >= 0 on a non-degenerate image: the bit patterns of the values order as the values do
  for (int i = threadIdx.x; i < nf; i += 256) {
    const float v = fix_val[bo + i];
    atomicAdd(&hf[em_nthr(v, step, ntmax)], 1u);
    atomicMax(&mxbits, __builtin_bit_cast(unsigned, v));
  }
  if (mode == 0) {
    const int* ri = rand_index + (static_cast<long>(b) * n_rep + rep) * cap;
    for (int i = threadIdx.x; i < cap; i += 256) {
      const int loc = ri[i];
      if (loc >= 0 && loc < n) {
        const float v = sb[loc];
        atomicAdd(&hr[em_nthr(v, step, ntmax)], 1u);
        atomicMax(&mxbits, __builtin_bit_cast(unsigned, v));
      }
    }
  } else if (mode == 1) {
    for (int i = threadIdx.x; i < nf; i += 256) {
      const unsigned long long e = static_cast<unsigned long long>(fix_idx[bo + i]) * n_rep + rep;
      const uint32_t w = em_word(ids, seed, b, e, EM_DRAW | 1u);
      const long loc = static_cast<long>((static_cast<unsigned long long>(w) * static_cast<unsigned long long>(n)) >> 32);
      const float v = sb[loc];      // loc < n because w < 2^32
      atomicAdd(&hr[em_nthr(v, step, ntmax)], 1u);
      atomicMax(&mxbits, __builtin_bit_cast(unsigned, v));
    }
  } else {
    const int m = nf < no ? nf : no;      // >= 1 here
    if (threadIdx.x == 0) { sel_prefix = 0ull; sel_left = m; }
    for (int pass = 0; pass < 8; ++pass) {
      const int shift = 56 - 8 * pass;
      radix[threadIdx.x] = 0u;
      __syncthreads();
      const unsigned long long prefix = sel_prefix;
      for (int i = threadIdx.x; i < no; i += 256) {
        const int p = oth_idx[bo + i];
        const unsigned long long e = static_cast<unsigned long long>(p) * n_rep + rep;
        const unsigned long long key = (static_cast<unsigned long long>(em_word(ids, seed, b, e, EM_DRAW | 2u)) << 32) | static_cast<unsigned>(p);
        if (pass == 0 || (key >> (shift + 8)) == (prefix >> (shift + 8))) atomicAdd(&radix[(key >> shift) & 255u], 1u);
      }
      __syncthreads();
      if (threadIdx.x == 0) {      // the bin that holds the sel_left-th smallest key among those that share the prefix
        int left = sel_left, d = 0;
        while (d < 255 && static_cast<int>(radix[d]) < left) { left -= radix[d]; ++d; }
        sel_left = left;
        sel_prefix = prefix | (static_cast<unsigned long long>(d) << shift);
      }
      __syncthreads();
    }
    const unsigned long long kth = sel_prefix;      // the m-th smallest key
    for (int i = threadIdx.x; i < no; i += 256) {
      const int p = oth_idx[bo + i];
      const unsigned long long e = static_cast<unsigned long long>(p) * n_rep + rep;
      const unsigned long long key = (static_cast<unsigned long long>(em_word(ids, seed, b, e, EM_DRAW | 2u)) << 32) | static_cast<unsigned>(p);
      if (key <= kth) {
        const float v = sb[p];
        atomicAdd(&hr[em_nthr(v, step, ntmax)], 1u);
        atomicMax(&mxbits, __builtin_bit_cast(unsigned, v));
      }
    }
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    const double mxv = __builtin_bit_cast(float, mxbits);
    double ntd = ceil(mxv / step);      // numpy's arange length rule for np.r_[0:max:step]
    const int nt = ntd > ntmax ? ntmax : static_cast<int>(ntd);
    const double dn = static_cast<double>(nf);
    // thresholds in descending order; cf / cr = fixation / sampled values >= k * step
    double area = 0, x0 = 0, y0 = 0;
    unsigned cf = 0, cr = 0;
    for (int c = ntmax; c >= 1; --c) {
      cf += hf[c]; cr += hr[c];
      if (c - 1 < nt) {
        const double x1 = static_cast<double>(cr) / dn, y1 = static_cast<double>(cf) / dn;
        area += (x1 - x0) * (y1 + y0) / 2.0;
        x0 = x1; y0 = y1;
      }
    }
    area += (1.0 - x0) * (1.0 + y0) / 2.0;
    rep_out[static_cast<long>(b) * n_rep + rep] = area;
  }
}

__global__ __launch_bounds__(256) void em_final_kernel(const double* __restrict__ img, const int* __restrict__ imgi,
                                                       const double* __restrict__ p3, const unsigned* __restrict__ sorted,
                                                       const double* __restrict__ rep, double* __restrict__ out, int B, long n,
                                                       long C, int n_rep, unsigned terms) {
  __shared__ double shd[4];
  const int b = blockIdx.x;
  const int nf = imgi[b * 4], no = imgi[b * 4 + 1];
  const bool degen = imgi[b * 4 + 2] != 0;
  const double nanv = __builtin_nan("");
  if (terms & T_JUDD) {
    double a = 0;
    if (!degen) {
      const unsigned* so = sorted + static_cast<long>(b) * n;
      const double dnf = static_cast<double>(nf), dneg = static_cast<double>(n - nf);
      for (int j = threadIdx.x; j <= nf; j += 256) {      // trapezoid j joins ROC points j and j + 1; point 0 = (0,0), last = (1,1)
        const double x0 = j == 0 ? 0.0 : static_cast<double>(static_cast<long>(so[j - 1]) - j) / dneg;
        const double y0 = j == 0 ? 0.0 : static_cast<double>(j) / dnf;
        const double x1 = j == nf ? 1.0 : static_cast<double>(static_cast<long>(so[j]) - j - 1) / dneg;
        const double y1 = j == nf ? 1.0 : static_cast<double>(j + 1) / dnf;
        a += (x1 - x0) * (y1 + y0) / 2.0;
      }
    }
    a = block_all(a, OpAdd(), shd);
    if (threadIdx.x == 0) out[0 * B + b] = degen ? nanv : a;
  }
  if (threadIdx.x != 0) return;
  for (int which = 0; which < 2; ++which) {
    if (!(terms & (which ? T_SAUC : T_BORJI))) continue;
    double a = nanv;
    if (!degen && !(which && no == 0)) {
      a = 0;
      const double* r = rep + (static_cast<long>(which) * B + b) * n_rep;
      for (int i = 0; i < n_rep; ++i) a += r[i];
      a /= static_cast<double>(n_rep);
    }
    out[(1 + which) * B + b] = a;
  }
  if (terms & (T_CC | T_NSS | T_SIM)) {
    double css = 0, cgg = 0, csg = 0, fs = 0, sim = 0;
    for (long c = 0; c < C; ++c) {
      const double* q = p3 + (static_cast<long>(b) * C + c) * P3;
      css += q[0]; cgg += q[1]; csg += q[2]; fs += q[3]; sim += q[4];
    }
    // a flat map: 0 / 0 in the reference's normalisations (fmin in `prep` would drop the NaN that numpy's minimum keeps)
    const double* m = img + static_cast<long>(b) * IM;
    const bool flat_s = !(m[7] > m[6]), flat_g = !(m[5] > m[4]);
    if (terms & T_CC) out[3 * B + b] = (flat_s || flat_g) ? nanv : csg / sqrt(css * cgg);
    // mean over the fixated pixels of (s - mean) / std, population std (numpy's default)
    if (terms & T_NSS)
      out[4 * B + b] = (nf == 0 || nf == n || flat_s) ? nanv : fs / static_cast<double>(nf) / sqrt(css / static_cast<double>(n));
    if (terms & T_SIM) out[5 * B + b] = (flat_s || flat_g) ? nanv : sim;
  }
}

}  // namespace diffsal

using namespace diffsal;

extern "C" size_t diffsal_eval_metrics_ws_bytes(int B, long n, unsigned int terms, int n_rep) {
  if (B <= 0 || n <= 0 || n_rep < 0) return 0;
  return em_layout(nullptr, B, n, terms, (terms & (T_BORJI | T_SAUC)) ? n_rep : 0).bytes;
}

extern "C" int diffsal_eval_metrics(const float* pred, const unsigned char* fix, const float* gt, const unsigned char* other, int B,
                                    long n, unsigned int terms, int n_rep, double step, const int* rand_borji, const int* rand_sauc,
                                    int cap, const long long* ids, const unsigned long long* seed, void* ws, size_t ws_bytes,
                                    double* out, diffsal_stream_t stream) {
  DS_REQUIRE(pred && ws && out, DIFFSAL_E_ARG, "eval_metrics: null argument");
  DS_REQUIRE(B > 0 && B <= 65535 && n > 1 && n < (1L << 31), DIFFSAL_E_SHAPE, "eval_metrics: bad shape B=%d (1..65535) n=%ld (2..2^31-1)", B, n);
  const unsigned fix_terms = T_JUDD | T_BORJI | T_SAUC | T_NSS;
  DS_REQUIRE(terms != 0 && (terms & ~127u) == 0 && (terms & 63u) != 0, DIFFSAL_E_ARG, "eval_metrics: terms %u names no metric", terms);
  DS_REQUIRE(!(terms & fix_terms) || fix, DIFFSAL_E_ARG, "eval_metrics: a fixation-based term needs the fixation map");
  DS_REQUIRE(!(terms & (T_CC | T_SIM)) || gt, DIFFSAL_E_ARG, "eval_metrics: CC and SIM need the ground-truth map");
  DS_REQUIRE(!(terms & T_SAUC) || other, DIFFSAL_E_ARG, "eval_metrics: sAUC needs the other-image fixation map");
  const bool jitter = (terms & T_JITTER) != 0, sweeps = (terms & (T_BORJI | T_SAUC)) != 0;
  DS_REQUIRE(!jitter || ((terms & T_JUDD) && !sweeps), DIFFSAL_E_ARG,
             "eval_metrics: jitter belongs to AUC-Judd; ask for the Borji sweeps in a call without it");
  const bool gen = jitter || ((terms & T_BORJI) && !rand_borji) || ((terms & T_SAUC) && !rand_sauc);
  DS_REQUIRE(!gen || (ids && seed), DIFFSAL_E_ARG, "eval_metrics: the device generator needs image ids and a seed");
  int ntmax = 0;
  if (sweeps) {
    DS_REQUIRE(n_rep > 0 && n_rep <= 65535, DIFFSAL_E_SHAPE, "eval_metrics: n_rep=%d (1..65535)", n_rep);
    DS_REQUIRE(step > 0.0 && step <= 1.0 && ceil(1.0 / step) <= EM_MAX_T, DIFFSAL_E_ARG, "eval_metrics: step %g (1/%d..1)", step, EM_MAX_T);
    ntmax = static_cast<int>(ceil(1.0 / step));
    DS_REQUIRE(!(rand_borji || rand_sauc) || cap > 0, DIFFSAL_E_SHAPE, "eval_metrics: rand_index with cap=%d", cap);
    // element p * n_rep + rep of the generator's stream: its quad index is a 32-bit counter word
    DS_REQUIRE(static_cast<unsigned long long>(n) * n_rep <= (1ull << 34), DIFFSAL_E_SHAPE, "eval_metrics: n * n_rep above 2^34");
  }
  const EmWs w = em_layout(ws, B, n, terms, sweeps ? n_rep : 0);
  DS_REQUIRE(ws_bytes >= w.bytes && aligned16(ws), DIFFSAL_E_ARG, "eval_metrics: workspace too small or misaligned");
  hipStream_t s = static_cast<hipStream_t>(stream);
  const long C = em_chunks(n);
  const dim3 grid(static_cast<unsigned>(C), B);
  hipLaunchKernelGGL(em_stats_kernel, grid, dim3(256), 0, s, pred, fix, gt, other, w.p1, w.pc, n, jitter ? 1 : 0, ids, seed);
  int rc = check_launch("eval_metrics(stats)");
  if (rc) return rc;
  hipLaunchKernelGGL(em_image_kernel, dim3(B), dim3(256), 0, s, w.p1, w.pc, w.img, w.imgi, n, C);
  if ((rc = check_launch("eval_metrics(image)"))) return rc;
  hipLaunchKernelGGL(em_prep_kernel, grid, dim3(256), 0, s, pred, fix, gt, other, w.img, w.pc, w.S, w.fix_val, w.fix_idx, w.oth_idx,
                     w.above, w.p3, n, jitter ? 1 : 0, ids, seed);
  if ((rc = check_launch("eval_metrics(prep)"))) return rc;
  if (terms & T_JUDD) {
    hipLaunchKernelGGL(em_judd_count_kernel, grid, dim3(64), 0, s, w.S, w.fix_val, w.imgi, w.above, n);
    if ((rc = check_launch("eval_metrics(count)"))) return rc;
    const unsigned rb = static_cast<unsigned>(C < 64 ? C : 64);
    hipLaunchKernelGGL(em_judd_rank_kernel, dim3(rb, B), dim3(256), 0, s, w.fix_val, w.above, w.imgi, w.sorted, n);
    if ((rc = check_launch("eval_metrics(rank)"))) return rc;
  }
  for (int which = 0; which < 2; ++which) {
    if (!(terms & (which ? T_SAUC : T_BORJI))) continue;
    const int* ri = which ? rand_sauc : rand_borji;
    hipLaunchKernelGGL(em_sweep_kernel, dim3(n_rep, B), dim3(256), 0, s, w.S, w.fix_val, w.fix_idx, w.oth_idx, w.imgi, ri, cap,
                       ri ? 0 : 1 + which, n, n_rep, step, ntmax, ids, seed, w.rep + static_cast<long>(which) * B * n_rep);
    if ((rc = check_launch("eval_metrics(sweep)"))) return rc;
  }
  hipLaunchKernelGGL(em_final_kernel, dim3(B), dim3(256), 0, s, w.img, w.imgi, w.p3, w.sorted, w.rep, out, B, n, C, n_rep, terms);
  return check_launch("eval_metrics(final)");
}
