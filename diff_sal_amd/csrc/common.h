// Shared helpers for the gfx950 kernels of libdiffsal_hip.so.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdarg>
#include <cstdint>
#include <cstdio>

#include "../../include/diffsal.h"

namespace diffsal {

void set_error(const char* fmt, ...);
// which kernel (and tile plan) the GEMM-family entry points launched last on this thread: diffsal_last_gemm_kernel()
void note_kernel(const char* fmt, ...);

inline bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0; }

inline int check_launch(const char* what) {
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) {
    set_error("%s: launch failed: %s", what, hipGetErrorString(e));
    return DIFFSAL_E_LAUNCH;
  }
  return DIFFSAL_OK;
}

#define DS_REQUIRE(cond, code, ...)  \
  do {                               \
    if (!(cond)) {                   \
      diffsal::set_error(__VA_ARGS__); \
      return (code);                 \
    }                                \
  } while (0)

constexpr int kWave = 64;  // CDNA wavefront

// Test / tuning switches ("Environment switches").  The environment is read ONCE, when the library is loaded; afterwards
// a switch changes only through diffsal_set_tuning() -- no getenv on a launch path, and no way for an inherited variable to
// reach a kernel argument.  tune(key) < 0 means "unset".  The one list of switches: X(NAME) is the key TUNE_NAME here and the
// variable / diffsal_set_tuning name "DIFFSAL_NAME" in misc.hip; append new ones at the end.
#define DIFFSAL_TUNE_KEYS(X) \
  X(NO_PERSIST) X(NO_XCD_ORDER) X(NO_HALO) X(FORCE_HALO) X(IGEMM_CFG) X(IGEMM16_CFG) X(PLAN_DEBUG) \
  X(WGRAD_CFG) X(WGRAD_SPLITS) X(WGRAD_VERBOSE) X(NO_FUSED_BLOCK) X(NO_WINOGRAD) X(FORCE_WINOGRAD) X(GN_CHUNKS) \
  X(GN_APPLY_WGS) X(GEMM_DMA) X(CONV_DMA) X(GROUP_GRID) X(GEMM_DMA16) X(WGRAD_DMA) X(NO_GN_SLAB) X(BATCH_TILE) \
  X(BATCH_XCD) X(NO_TAPSUM_ROWS) X(TAPSUM_ROWS_FORM) X(NO_ATTN_BWD_DS) X(NO_POOL_RUNS) X(NO_ATTN_SLOTS) X(NO_STREAM16) \
  X(CONV16_TILE) X(BLOCK16_WAVES) X(NO_ATTN16_MFMA) X(CONV16_HALF) X(FRONT_FOLD_WGS)
#define DIFFSAL_TUNE_ENUM(name) TUNE_##name,
enum TuneKey { DIFFSAL_TUNE_KEYS(DIFFSAL_TUNE_ENUM) TUNE_COUNT };
#undef DIFFSAL_TUNE_ENUM
int tune(int key);

// Butterfly all-reduce over `width` (power of two <= 64) consecutive lanes, entirely on the VALU: quad permutes for the
// strides 1 and 2, row_half_mirror / row_mirror for 4 and 8 (every quad / 8-lane group already holds its own total, so the
// mirrored partner carries the same value the xor partner would), v_permlane16_swap / v_permlane32_swap for 16 and 32.
// `__shfl_xor` compiles to ds_bpermute_b32 -- an LDS round trip of ~100 cycles per step on the critical path of every
// LayerNorm-style reduction.  Bit-identical to the xor butterfly (each step adds the same two operands).
template <int CTRL>
__device__ __forceinline__ float dpp_move(float v) {
  return __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), CTRL, 0xF, 0xF, false));
}
__device__ __forceinline__ float lane_xor16(float v) {   // value of lane ^ 16
  const unsigned u = __builtin_bit_cast(unsigned, v);
  const auto r = __builtin_amdgcn_permlane16_swap(u, u, false, false);   // odd rows of r[0] <-> even rows of r[1]
  return __builtin_bit_cast(float, (__lane_id() & 16) ? r[0] : r[1]);
}
__device__ __forceinline__ float lane_xor32(float v) {   // value of lane ^ 32
  const unsigned u = __builtin_bit_cast(unsigned, v);
  const auto r = __builtin_amdgcn_permlane32_swap(u, u, false, false);   // lanes 32-63 of r[0] <-> lanes 0-31 of r[1]
  return __builtin_bit_cast(float, (__lane_id() & 32) ? r[0] : r[1]);
}
template <int WIDTH, typename OP>
__device__ __forceinline__ float group_reduce(float v, OP op) {
  static_assert(WIDTH >= 1 && WIDTH <= 64 && (WIDTH & (WIDTH - 1)) == 0, "power of two <= 64");
  if constexpr (WIDTH >= 2) v = op(v, dpp_move<0xB1>(v));     // quad_perm [1,0,3,2]
  if constexpr (WIDTH >= 4) v = op(v, dpp_move<0x4E>(v));     // quad_perm [2,3,0,1]
  if constexpr (WIDTH >= 8) v = op(v, dpp_move<0x141>(v));    // row_half_mirror
  if constexpr (WIDTH >= 16) v = op(v, dpp_move<0x140>(v));   // row_mirror
  if constexpr (WIDTH >= 32) v = op(v, lane_xor16(v));
  if constexpr (WIDTH >= 64) v = op(v, lane_xor32(v));
  return v;
}
template <int WIDTH>
__device__ __forceinline__ float group_sum(float v) {
  return group_reduce<WIDTH>(v, [](float a, float b) { return a + b; });
}
template <int WIDTH>
__device__ __forceinline__ float group_max(float v) {
  return group_reduce<WIDTH>(v, [](float a, float b) { return fmaxf(a, b); });
}

// exclusive scan of one value per thread over a workgroup of THREADS; the workgroup's total through `total`.  sh: THREADS words
template <int THREADS>
__device__ __forceinline__ uint32_t block_exclusive_scan(uint32_t v, uint32_t* sh, uint32_t& total) {
  const int t = threadIdx.x;
  __syncthreads();      // sh may still be read from the round before
  sh[t] = v;
  __syncthreads();
  for (int o = 1; o < THREADS; o <<= 1) {
    const uint32_t add = t >= o ? sh[t - o] : 0u;
    __syncthreads();
    sh[t] += add;
    __syncthreads();
  }
  total = sh[THREADS - 1];
  return sh[t] - v;
}

// x sigmoid(x) with e = exp(-|x|) <= 1: x / (1 + e) for x >= 0 (the plain form, bit for bit), x e / (1 + e) below.  The plain form
// x / (1 + exp(-x)) overflows its exponential below x = -88.7 and returns 0 where the value, down to 2e-37, is still a normal float.
__device__ __forceinline__ float swishf(float x) {
  const float e = expf(-fabsf(x));
  return (x < 0.f ? x * e : x) / (1.0f + e);
}
__device__ __forceinline__ float sigmoidf_(float x) { return 1.0f / (1.0f + expf(-x)); }
// x sigmoid(x) on the hardware transcendentals (v_exp_f32, v_rcp_f32: ~1 ulp each, five instructions instead of the ~30 of
// libm's expf + an IEEE division): for kernels that evaluate it per LOADED element (the F(4x4) input transform reads every
// pixel 2.25 times).  exp2 of a large positive argument overflows to +inf, rcp(+inf) = 0: the limit x -> -inf is exact.
// Below x = -88.72 (exp2 argument above 128) that overflow comes early: the result is -0 where x sigmoid(x), between -2.6e-37 and
// the smallest subnormal, is still representable -- an absolute error below 2.6e-37, which swishf's exp(-|x|) form avoids and this
// one accepts (its consumer, the Winograd input transform, carries 1e-5 of the map's maximum).  NaN stays NaN; +inf gives +inf.
__device__ __forceinline__ float swishf_fast(float x) {
  return x * __builtin_amdgcn_rcpf(1.0f + __builtin_amdgcn_exp2f(-1.4426950408889634f * x));
}
// erf with |error| <= 1.5e-7 (Abramowitz & Stegun 7.1.26): one v_exp, one v_rcp, six FMAs -- a third of the
// instructions of libm's erff; the difference is far below the fp32 noise of the surrounding GEMMs.
__device__ __forceinline__ float erf_as(float x) {
  const float ax = fabsf(x);
  const float t = __builtin_amdgcn_rcpf(fmaf(0.3275911f, ax, 1.0f));
  float p = fmaf(1.061405429f, t, -1.453152027f);
  p = fmaf(p, t, 1.421413741f);
  p = fmaf(p, t, -0.284496736f);
  p = fmaf(p, t, 0.254829592f);
  const float r = 1.0f - p * t * __expf(-ax * ax);
  return copysignf(r, x);
}
__device__ __forceinline__ float gelu_erf(float x) { return 0.5f * x * (1.0f + erf_as(x * 0.70710678118654752440f)); }
// d/dx of erf-GELU: Phi(x) + x * phi(x), with erf_as's polynomial; its exp(-x^2 / 2) is the one phi needs (one v_exp, one v_rcp
// and ten FMAs per element -- cheap enough for a GEMM epilogue).  act_bwd_kernel (mode 2) uses the same function.
__device__ __forceinline__ float gelu_erf_grad(float x) {
  const float ax = fabsf(x) * 0.70710678118654752440f;
  const float t = __builtin_amdgcn_rcpf(fmaf(0.3275911f, ax, 1.0f));
  float p = fmaf(1.061405429f, t, -1.453152027f);
  p = fmaf(p, t, 1.421413741f);
  p = fmaf(p, t, -0.284496736f);
  p = fmaf(p, t, 0.254829592f);
  const float e = __expf(-ax * ax);
  const float erf_x = copysignf(1.0f - p * t * e, x);
  return fmaf(x * 0.3989422804014327f, e, 0.5f * (1.0f + erf_x));
}

__device__ __forceinline__ float4 ld4(const float* p) { return *reinterpret_cast<const float4*>(p); }
__device__ __forceinline__ void st4(float* p, float4 v) { *reinterpret_cast<float4*>(p) = v; }

// N groups of MFMAs whose A fragment is one 16-byte LDS read: the read of group i + 1 is issued BEFORE the MFMAs of group i
// (pinned with sched_barrier: left alone, hipcc reads a fragment, waits for it, then issues its four dependent MFMAs, and a
// quarter of the matrix time is LDS latency).  addr(i) -> const float*, body(i, fragment).
template <int N, typename AddrF, typename BodyF>
__device__ __forceinline__ void mfma_groups_f32(AddrF addr, BodyF body) {
  float4 a = ld4(addr(0));
#pragma unroll
  for (int i = 0; i < N; ++i) {
    float4 an = a;
    if (i + 1 < N) an = ld4(addr(i + 1));
    __builtin_amdgcn_sched_barrier(0);
    body(i, a);
    __builtin_amdgcn_sched_barrier(0);
    a = an;
  }
}
// The same for products whose A operand is ONE scalar LDS read per MFMA (the LDS tile is stored [contraction row][feature], the
// operand wants a feature column): group i = the PER scalars of PER MFMAs, read before the MFMAs of group i - 1.
// addr(i, j) -> const float* of scalar j of group i; body(i, fragment array).
template <int N, int PER, typename AddrF, typename BodyF>
__device__ __forceinline__ void mfma_groups_scalar_f32(AddrF addr, BodyF body) {
  float a[2][PER];
#pragma unroll
  for (int j = 0; j < PER; ++j) a[0][j] = *addr(0, j);
#pragma unroll
  for (int i = 0; i < N; ++i) {
    if (i + 1 < N) {
#pragma unroll
      for (int j = 0; j < PER; ++j) a[(i + 1) & 1][j] = *addr(i + 1, j);
    }
    __builtin_amdgcn_sched_barrier(0);
    body(i, a[i & 1]);
    __builtin_amdgcn_sched_barrier(0);
  }
}
#define DS_MFMA4(ACC, A, B0, B1, B2, B3)                                         \
  do {                                                                           \
    ACC = __builtin_amdgcn_mfma_f32_32x32x2f32((A).x, (B0), ACC, 0, 0, 0);       \
    ACC = __builtin_amdgcn_mfma_f32_32x32x2f32((A).y, (B1), ACC, 0, 0, 0);       \
    ACC = __builtin_amdgcn_mfma_f32_32x32x2f32((A).z, (B2), ACC, 0, 0, 0);       \
    ACC = __builtin_amdgcn_mfma_f32_32x32x2f32((A).w, (B3), ACC, 0, 0, 0);       \
  } while (0)

// 16-bit storage (DIFFSAL_BF16 / DIFFSAL_F16): the same 4-channel accessors on 8-byte runs; arithmetic stays fp32,
// one round-to-nearest-even on the way out.
typedef __bf16 bf16_t;
typedef _Float16 f16_t;
typedef float f32x4_t __attribute__((ext_vector_type(4)));
typedef __bf16 bf16x4_t __attribute__((ext_vector_type(4)));
typedef _Float16 f16x4_t __attribute__((ext_vector_type(4)));
__device__ __forceinline__ float4 ld4(const bf16_t* p) {
  const uint2 u = *reinterpret_cast<const uint2*>(p);
  return make_float4(__builtin_bit_cast(float, u.x << 16), __builtin_bit_cast(float, u.x & 0xFFFF0000u),
                     __builtin_bit_cast(float, u.y << 16), __builtin_bit_cast(float, u.y & 0xFFFF0000u));
}
__device__ __forceinline__ void st4(bf16_t* p, float4 v) {
  const f32x4_t f = {v.x, v.y, v.z, v.w};
  *reinterpret_cast<bf16x4_t*>(p) = __builtin_convertvector(f, bf16x4_t);
}
__device__ __forceinline__ float4 ld4(const f16_t* p) {
  const f16x4_t h = *reinterpret_cast<const f16x4_t*>(p);
  const f32x4_t f = __builtin_convertvector(h, f32x4_t);
  return make_float4(f.x, f.y, f.z, f.w);
}
__device__ __forceinline__ void st4(f16_t* p, float4 v) {
  const f32x4_t f = {v.x, v.y, v.z, v.w};
  *reinterpret_cast<f16x4_t*>(p) = __builtin_convertvector(f, f16x4_t);
}
// 8 elements = one 16-byte access of 16-bit storage: what the HBM-bound kernels on 16-bit storage move per lane (the 4-element
// accessors above are 8-byte accesses: half the bytes in flight per instruction, and a 32-channel slab is only half a 128-byte line)
struct f8v { float v[8]; };
typedef __bf16 bf16x8_t __attribute__((ext_vector_type(8)));
typedef _Float16 f16x8_t __attribute__((ext_vector_type(8)));
typedef float f32x8_t __attribute__((ext_vector_type(8)));
__device__ __forceinline__ f8v ld8(const bf16_t* p) {
  const uint4 u = *reinterpret_cast<const uint4*>(p);
  f8v r;
  r.v[0] = __builtin_bit_cast(float, u.x << 16); r.v[1] = __builtin_bit_cast(float, u.x & 0xFFFF0000u);
  r.v[2] = __builtin_bit_cast(float, u.y << 16); r.v[3] = __builtin_bit_cast(float, u.y & 0xFFFF0000u);
  r.v[4] = __builtin_bit_cast(float, u.z << 16); r.v[5] = __builtin_bit_cast(float, u.z & 0xFFFF0000u);
  r.v[6] = __builtin_bit_cast(float, u.w << 16); r.v[7] = __builtin_bit_cast(float, u.w & 0xFFFF0000u);
  return r;
}
__device__ __forceinline__ f8v ld8(const f16_t* p) {
  const f16x8_t h = *reinterpret_cast<const f16x8_t*>(p);
  const f32x8_t f = __builtin_convertvector(h, f32x8_t);
  f8v r;
#pragma unroll
  for (int e = 0; e < 8; ++e) r.v[e] = f[e];
  return r;
}
__device__ __forceinline__ void st8(bf16_t* p, const f8v& x) {
  const f32x8_t f = {x.v[0], x.v[1], x.v[2], x.v[3], x.v[4], x.v[5], x.v[6], x.v[7]};
  *reinterpret_cast<bf16x8_t*>(p) = __builtin_convertvector(f, bf16x8_t);
}
__device__ __forceinline__ void st8(f16_t* p, const f8v& x) {
  const f32x8_t f = {x.v[0], x.v[1], x.v[2], x.v[3], x.v[4], x.v[5], x.v[6], x.v[7]};
  *reinterpret_cast<f16x8_t*>(p) = __builtin_convertvector(f, f16x8_t);
}
__device__ __forceinline__ float to_f32(bf16_t x) { return static_cast<float>(x); }
__device__ __forceinline__ float to_f32(f16_t x) { return static_cast<float>(x); }
// 4-element accesses of T need 4 * sizeof(T) alignment
template <typename T> inline bool aligned_vec4(const T* p) { return (reinterpret_cast<uintptr_t>(p) & (4 * sizeof(T) - 1)) == 0; }

// Opt a kernel in to more than 64 KiB of dynamic LDS once PER DEVICE (the attribute is per device; a process that drives
// several GPUs must not rely on a per-process flag).  A benign race at worst sets the attribute twice.
#define DS_RAISE_DYNAMIC_LDS(fn, bytes)                                                                       \
  do {                                                                                                        \
    static unsigned long long ds_raised_mask_ = 0;                                                            \
    int ds_dev_ = 0;                                                                                          \
    (void)hipGetDevice(&ds_dev_);                                                                             \
    const unsigned long long ds_bit_ = 1ull << (ds_dev_ & 63);                                                \
    if (!(ds_raised_mask_ & ds_bit_)) {                                                                       \
      (void)hipFuncSetAttribute(reinterpret_cast<const void*>(fn), hipFuncAttributeMaxDynamicSharedMemorySize, bytes); \
      ds_raised_mask_ |= ds_bit_;                                                                             \
    }                                                                                                         \
  } while (0)

// Run `CALL(T)` with T = the storage type named by a DIFFSAL_F32 / BF16 / F16 code.
#define DS_DTYPE_DISPATCH(dtype, what, CALL)                                                      \
  do {                                                                                            \
    if ((dtype) == DIFFSAL_F32) { CALL(float); }                                                  \
    else if ((dtype) == DIFFSAL_BF16) { CALL(diffsal::bf16_t); }                                  \
    else if ((dtype) == DIFFSAL_F16) { CALL(diffsal::f16_t); }                                    \
    else { diffsal::set_error("%s: dtype %d (DIFFSAL_F32, DIFFSAL_BF16 or DIFFSAL_F16)", what, (dtype)); return DIFFSAL_E_ARG; } \
  } while (0)

// Source coordinate of a bilinear resize with align_corners=False (PyTorch area_pixel_compute_source_index).
__device__ __forceinline__ void bilin_coord(int dst, float scale, int in_size, int& i0, int& i1, float& l1) {
  float s = (static_cast<float>(dst) + 0.5f) * scale - 0.5f;
  s = s < 0.f ? 0.f : s;
  i0 = static_cast<int>(s);
  i0 = i0 > in_size - 1 ? in_size - 1 : i0;
  i1 = i0 + (i0 < in_size - 1 ? 1 : 0);
  l1 = s - static_cast<float>(i0);
}

// ---------------------------------------------------------------------------------------------------------------------------
// Building blocks of the matrix-core and LDS-DMA kernels: one copy of each, for every kernel.
// ---------------------------------------------------------------------------------------------------------------------------
typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef int i32x4 __attribute__((ext_vector_type(4)));
typedef __attribute__((address_space(3))) void* lds_ptr_t;   // (lds_ptr_t)p: a __shared__ object's LDS pointer (its value: the byte address)

// v_mfma_f32_32x32x16 on 16-bit storage type T: vec = one 8-element operand fragment, run(a, b, c) = c + a x b in fp32
template <typename T> struct Mfma32x16;
template <> struct Mfma32x16<__bf16> {
  typedef bf16x8_t vec;
  static __device__ __forceinline__ f32x16 run(vec a, vec b, f32x16 c) { return __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, b, c, 0, 0, 0); }
};
template <> struct Mfma32x16<_Float16> {
  typedef f16x8_t vec;
  static __device__ __forceinline__ f32x16 run(vec a, vec b, f32x16 c) { return __builtin_amdgcn_mfma_f32_32x32x16_f16(a, b, c, 0, 0, 0); }
};

// Word 3 of every buffer descriptor: 32-bit data format, no swizzle, no stride -- raw byte offsets, range-checked against the
// descriptor's byte count (an access past it reads zeros and touches no memory).
constexpr int kRsrcWord3 = 0x00020000;
// `records` bytes from byte address `base`, in the form the inline-assembly DMA below takes
__device__ __forceinline__ i32x4 dma_rsrc(unsigned long base, int records) {
  return i32x4{static_cast<int>(base), static_cast<int>(base >> 32) & 0xFFFF, records, kRsrcWord3};
}
// the same for __builtin_amdgcn_raw_buffer_load_*
__device__ __forceinline__ __amdgpu_buffer_rsrc_t buffer_rsrc(const void* base, int records) {
  return __builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(base), 0, records, kRsrcWord3);
}

// One LDS-DMA piece: 64 lanes x 16 bytes from the buffer `rsrc` at voff + soff into LDS at lds_addr + 16 lane.  Inline assembly on
// purpose: hipcc orders every later LDS read behind a DMA it knows about (s_waitcnt vmcnt(0) in front of the fragment reads at a
// loop header, whatever object they read), which serialises the ring.  Here the compiler sees neither the LDS write nor the
// vmcnt event; the kernel places its own counted waits.  (Its counted waits for ordinary loads stay safe: vmcnt retires in
// order, so DMAs it does not know about only make such a wait stricter.)
__device__ __forceinline__ void dma_piece(unsigned lds_addr, unsigned voff, i32x4 rsrc, unsigned soff) {
  asm volatile("s_mov_b32 m0, %0\n\ts_nop 0\n\tbuffer_load_dwordx4 %1, %2, %3 offen lds"
               :
               : "s"(lds_addr), "v"(voff), "s"(rsrc), "s"(soff)
               : "memory", "m0");
}
// soff = 0 as an inline constant (no scalar register for it)
__device__ __forceinline__ void dma_piece(unsigned lds_addr, unsigned voff, i32x4 rsrc) {
  asm volatile("s_mov_b32 m0, %0\n\ts_nop 0\n\tbuffer_load_dwordx4 %1, %2, 0 offen lds" : : "s"(lds_addr), "v"(voff), "s"(rsrc) : "memory", "m0");
}

// Counted waits: at most VM vector-memory operations (DMA pieces included) and LGKM LDS / scalar-memory operations of this
// wavefront still outstanding.  gfx950's s_waitcnt holds vmcnt in 6 bits and lgkmcnt in 4.
template <int VM>
__device__ __forceinline__ void wait_vmcnt() {
  static_assert(VM >= 0 && VM < 64, "vmcnt: 6 bits");
  asm volatile("s_waitcnt vmcnt(%0)" ::"n"(VM) : "memory");
}
template <int VM, int LGKM>
__device__ __forceinline__ void wait_vm_lgkm() {
  static_assert(VM >= 0 && VM < 64, "vmcnt: 6 bits");
  static_assert(LGKM >= 0 && LGKM < 16, "lgkmcnt: 4 bits");
  asm volatile("s_waitcnt vmcnt(%0) lgkmcnt(%1)" ::"n"(VM), "n"(LGKM) : "memory");
}

// Workgroups are dealt round-robin over the 8 XCDs, each with its own L2.  xcd_contiguous<I>(nwg): the virtual index of workgroup
// b = blockIdx.x among the first nwg -- the (b / 8)-th item of the contiguous run of the virtual order that belongs to XCD b % 8 -- so
// that neighbouring items (tiles that share operand rows, patches that share halo rows) are read through one L2.  A bijection of
// [0, nwg) for any nwg.  I: the index arithmetic, int or unsigned, as the kernel had it (signed and unsigned shifts and compares
// are different instructions).
template <typename I>
__device__ __forceinline__ I xcd_contiguous(unsigned nwg) {
  const I n = nwg, b = blockIdx.x;
  const I xcd = b & 7, slot = b >> 3;
  const I q = n >> 3, r = n & 7;
  return (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + slot;
}

// a wave-uniform value -> a scalar register
__device__ __forceinline__ int uniform_i(int v) { return __builtin_amdgcn_readfirstlane(v); }
__device__ __forceinline__ float uniform_f(float v) {
  return __builtin_bit_cast(float, __builtin_amdgcn_readfirstlane(__builtin_bit_cast(int, v)));
}

// The epilogue of the matrix kernels, on N (1, 4 or 8) consecutive output channels n .. n + N - 1 of one output row, in fp32:
//   v += bias[n];  v = v * scale[n] + shift[n];  v += rowvec[image of the row][n];  v = act(v);
//   v += residual   (act == DIFFSAL_ACT_GELU_GRAD:  v *= gelu_erf'(residual));   one rounding at the store.
// A term whose operand is absent is skipped (skipped, not "added as zero": -0.0 + 0.0 is +0.0).  scale and shift come together:
// every entry point refuses one without the other, so `scale` alone decides and `shift` is read untested.  Only fp32
// diffsal_conv_igemm accepts DIFFSAL_ACT_GELU_GRAD (and then requires `residual`): its kernels choose between epi_gelu_grad and
// epi_add, every other kernel has epi_add alone.  Loads of the residual, bounds tests, LDS staging and stores stay with the kernels.
template <int N>
__device__ __forceinline__ void epi_act(float (&v)[N], int act) {
  if (act == DIFFSAL_ACT_RELU) {
#pragma unroll
    for (int e = 0; e < N; ++e) v[e] = v[e] < 0.f ? 0.f : v[e];   // not fmaxf: max(NaN, 0) is 0, and a NaN must stay one
  } else if (act == DIFFSAL_ACT_GELU_ERF) {
#pragma unroll
    for (int e = 0; e < N; ++e) v[e] = gelu_erf(v[e]);
  } else if (act == DIFFSAL_ACT_SIGMOID) {
#pragma unroll
    for (int e = 0; e < N; ++e) v[e] = sigmoidf_(v[e]);
  }
}

// t = p[0 .. N - 1], as 16-byte loads when N is 4 or 8
template <int N>
__device__ __forceinline__ void epi_ld(float (&t)[N], const float* p) {
  static_assert(N == 1 || N % 4 == 0, "one channel or whole quads");
  if constexpr (N == 1) {
    t[0] = *p;
  } else {
#pragma unroll
    for (int q = 0; q < N; q += 4) {
      const float4 x = ld4(p + q);
      t[q] = x.x; t[q + 1] = x.y; t[q + 2] = x.z; t[q + 3] = x.w;
    }
  }
}
template <int N>
__device__ __forceinline__ void epi_add(float (&v)[N], const float (&t)[N]) {
#pragma unroll
  for (int e = 0; e < N; ++e) v[e] += t[e];
}
__device__ __forceinline__ void epi_add(float (&v)[4], float4 t) { v[0] += t.x; v[1] += t.y; v[2] += t.z; v[3] += t.w; }
// bias, scale / shift and rowvec from memory: the vectors' base pointers (null: absent) and n.  rowvec's row starts at
// rowvec + row_off(), which is evaluated only when rowvec is set (an image index usually costs a division).
template <int N, typename RowOff>
__device__ __forceinline__ void epi_channels(float (&v)[N], const float* bias, const float* scale, const float* shift, const float* rowvec,
                                             RowOff row_off, int n) {
  float t[N], h[N];
  if (bias) { epi_ld(t, bias + n); epi_add(v, t); }
  if (scale) {
    epi_ld(t, scale + n);
    epi_ld(h, shift + n);
#pragma unroll
    for (int e = 0; e < N; ++e) v[e] = v[e] * t[e] + h[e];
  }
  if (rowvec) { epi_ld(t, rowvec + row_off() + n); epi_add(v, t); }
}
// the same with the row's address in hand: rowvec_row = rowvec + the row's offset, or null
template <int N>
__device__ __forceinline__ void epi_channels(float (&v)[N], const float* bias, const float* scale, const float* shift, const float* rowvec_row,
                                             int n) {
  epi_channels(v, bias, scale, shift, rowvec_row, [] { return 0; }, n);
}

// DIFFSAL_ACT_GELU_GRAD's residual term, v *= gelu_erf'(r), on a residual the caller has loaded (the plain term is epi_add)
__device__ __forceinline__ void epi_gelu_grad(float (&v)[4], float4 r) {
  v[0] *= gelu_erf_grad(r.x); v[1] *= gelu_erf_grad(r.y); v[2] *= gelu_erf_grad(r.z); v[3] *= gelu_erf_grad(r.w);
}


// Philox4x32-10 of include/diffsal.h ("sampler noise"): key = the seed's two halves, counter = (quad, draw, id lo, id hi).  The
// seed and the ids are read from device memory so that a captured graph can be replayed for other clips.
__device__ __forceinline__ void philox4x32_10(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0, uint32_t k1,
                                              uint32_t (&r)[4]) {
#pragma unroll
  for (int i = 0; i < 10; ++i) {
    const uint32_t hi0 = __umulhi(0xD2511F53u, c0), lo0 = 0xD2511F53u * c0;
    const uint32_t hi1 = __umulhi(0xCD9E8D57u, c2), lo1 = 0xCD9E8D57u * c2;
    const uint32_t n0 = hi1 ^ c1 ^ k0, n2 = hi0 ^ c3 ^ k1;
    c0 = n0; c1 = lo1; c2 = n2; c3 = lo0;
    k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
  }
  r[0] = c0; r[1] = c1; r[2] = c2; r[3] = c3;
}

__device__ __forceinline__ void philox_quad(const long long* __restrict__ ids, const unsigned long long* __restrict__ seed,
                                            long n, uint32_t q, uint32_t draw, uint32_t (&r)[4]) {
  const unsigned long long sd = seed[0], id = static_cast<unsigned long long>(ids[n]);
  philox4x32_10(q, draw, static_cast<uint32_t>(id), static_cast<uint32_t>(id >> 32), static_cast<uint32_t>(sd),
                static_cast<uint32_t>(sd >> 32), r);
}

}  // namespace diffsal
