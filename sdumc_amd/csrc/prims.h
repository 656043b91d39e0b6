// prims.h — the device primitives every kernel source shares, one definition each (gfx950 only).  Included by common.h at global
// scope, so a file that includes common.h (or p3_loop.h / chain_common.h, which do) sees them from inside any namespace.
// What belongs to ONE kernel's LDS layout (its swizzle functions, its tile constants) stays with that kernel.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef float f32x16 __attribute__((ext_vector_type(16)));

typedef __attribute__((address_space(3))) void lds_void_t;      // the LDS side of an LDS-DMA load

// The immediate of s_waitcnt that waits for all but the youngest n vector-memory operations (lgkmcnt and expcnt left open).
// vmcnt is a 6-bit counter, split over bits 3:0 and 15:14: a count beyond 63 is waited for as 63 -- stricter, so still correct
// (unclamped, bit 6 and up of n would land in bit 16 and up of the immediate, which are other fields).
constexpr int waitcnt_vm(int n) { return ((n > 63 ? 63 : n) & 0xF) | (((n > 63 ? 63 : n) >> 4) << 14) | (0x7 << 4) | (0xF << 8); }
constexpr int waitcnt_vm_unclamped(int n) { return (n & 0xF) | ((n >> 4) << 14) | (0x7 << 4) | (0xF << 8); }      // (the checks below only)
static_assert(waitcnt_vm(0) == waitcnt_vm_unclamped(0) && waitcnt_vm(1) == waitcnt_vm_unclamped(1) && waitcnt_vm(15) == waitcnt_vm_unclamped(15) &&
                  waitcnt_vm(16) == waitcnt_vm_unclamped(16) && waitcnt_vm(36) == waitcnt_vm_unclamped(36) && waitcnt_vm(63) == waitcnt_vm_unclamped(63),
              "within the counter's range the clamped form is the plain encoding");
static_assert(waitcnt_vm(64) == waitcnt_vm(63) && waitcnt_vm(68) == waitcnt_vm(63), "beyond the counter's range: waited for as 63");

__device__ __forceinline__ float fast_tanh(float x) {
  // 1 - 2 / (1 + e^{2x}): v_exp_f32 + v_rcp_f32, absolute error ~1e-7 (saturates correctly at +-1, NaN propagates)
  return 1.f - 2.f * __frcp_rn(1.f + __expf(2.f * x));
}

// ---- bf16 <-> fp32 ----
__device__ __forceinline__ float bf2f(unsigned short h) { return __uint_as_float((unsigned)h << 16); }
__device__ __forceinline__ unsigned short f2bf(float f) {
  __bf16 h = (__bf16)f;      // v_cvt_pk_bf16_f32: round to nearest even, NaN stays NaN
  return *reinterpret_cast<unsigned short*>(&h);
}
// two fp32 -> one dword of two bf16 (v_cvt_pk_bf16_f32, round to nearest even), low half = lo.  A name of its own, not an overload
// of f2bf / bf2f: with one, an int argument would be ambiguous.
__device__ __forceinline__ uint32_t pack_bf16x2(float lo, float hi) {
  typedef __bf16 bf16x2_t __attribute__((ext_vector_type(2)));
  typedef float f32x2_t __attribute__((ext_vector_type(2)));
  const f32x2_t v = {lo, hi};
  return __builtin_bit_cast(uint32_t, __builtin_convertvector(v, bf16x2_t));
}

// ---- fp32 products on the bf16 matrix pipe (gemm_group.hip derives the arithmetic) ----
typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
// two fp32 values -> their three bf16 parts, one dword per plane (low half = x): x == p0.x + p1.x + p2.x exactly.
// tests/test_split_arithmetic.py restates this on the CPU.
__device__ __forceinline__ void split_bf16x3(float x, float y, uint32_t& p0, uint32_t& p1, uint32_t& p2) {
  p0 = pack_bf16x2(x, y);
  const float x1 = x - __uint_as_float(p0 << 16), y1 = y - __uint_as_float(p0 & 0xFFFF0000u);       // exact
  p1 = pack_bf16x2(x1, y1);
  const float x2 = x1 - __uint_as_float(p1 << 16), y2 = y1 - __uint_as_float(p1 & 0xFFFF0000u);     // exact
  p2 = pack_bf16x2(x2, y2);
}
// the six largest of the nine part products, smallest terms first: (a2 b0), (a0 b2), (a1 b1), (a1 b0), (a0 b1), (a0 b0)
constexpr int BF16X3_TA[6] = {2, 0, 1, 1, 0, 0}, BF16X3_TB[6] = {0, 2, 1, 0, 1, 0};
// one accumulator tile += a b, a and b as three planes of eight k each
__device__ __forceinline__ void mfma_bf16x3(f32x16& acc, const u32x4 (&a)[3], const u32x4 (&b)[3]) {
#pragma unroll
  for (int t = 0; t < 6; ++t)
    acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8, a[BF16X3_TA[t]]), __builtin_bit_cast(bf16x8, b[BF16X3_TB[t]]), acc, 0, 0, 0);
}

// ---- 16-byte accesses ----
__device__ __forceinline__ f32x4 ld4(const float* p) { return *reinterpret_cast<const f32x4*>(p); }
__device__ __forceinline__ void st4(float* p, f32x4 v) { *reinterpret_cast<f32x4*>(p) = v; }
__device__ __forceinline__ float dot4(f32x4 a, f32x4 b) { return a[0] * b[0] + a[1] * b[1] + a[2] * b[2] + a[3] * b[3]; }
// agent-scope (write-through / L2-bypassing) accesses for data that another workgroup of the SAME launch reads after a hand-shake
// (attn_pool.hip's tickets, chain_cluster.hip's arrival counters): the workgroups may run on different XCDs, whose L2s are not coherent
__device__ __forceinline__ void stf_dev(float* p, float v) { __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ float ldf_dev(const float* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ void st4_dev(float* p, f32x4 v) {
#pragma unroll
  for (int j = 0; j < 4; ++j) stf_dev(p + j, v[j]);
}
__device__ __forceinline__ f32x4 ld4_dev(const float* p) {
  f32x4 v;
#pragma unroll
  for (int j = 0; j < 4; ++j) v[j] = ldf_dev(p + j);
  return v;
}

// one element of a norm-and-guard reduction: acc += x^2 in fp64, bad += (x is NaN or +-Inf)
__device__ __forceinline__ void sumsq_count_nonfinite(float x, double& acc, uint32_t& bad) {
  acc = fma((double)x, (double)x, acc);
  bad += (__float_as_uint(x) & 0x7f800000u) == 0x7f800000u;
}
