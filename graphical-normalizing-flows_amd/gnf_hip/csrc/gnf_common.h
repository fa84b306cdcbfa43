// Shared helpers for the gfx950 kernels of libgnf_hip.so.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "gnf_hip.h"

#define GNF_WAVE 64

#define GNF_LAUNCH_CHECK()                         \
  do {                                             \
    hipError_t e__ = hipGetLastError();            \
    if (e__ != hipSuccess) return (int)e__;        \
  } while (0)

// Launch `kernel` with `lds` bytes of dynamic LDS: raises the kernel's dynamic-LDS limit to that size (above the 64 KB
// default a launch fails without it; set on every call), launches, returns the launch status.
template <typename... P, typename... A>
static inline hipError_t gnf_launch_lds(void (*kernel)(P...), dim3 grid, dim3 block, size_t lds, hipStream_t s,
                                        const A&... args) {
  (void)hipFuncSetAttribute(reinterpret_cast<const void*>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
  hipLaunchKernelGGL(kernel, grid, block, lds, s, args...);
  return hipGetLastError();
}

// ---------------------------------------------------------------------------------------------------------------------
// Device support shared by every translation unit: vector types, buffer descriptors, MFMA wrappers, the bf16 split.
// All at global scope like the rest of this header; the units keep their kernels in their own (anonymous) namespaces.
// ---------------------------------------------------------------------------------------------------------------------
typedef float f32x2 __attribute__((ext_vector_type(2)));
typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef float f32x16 __attribute__((ext_vector_type(16)));
// the same with dword alignment: a dwordx2 / dwordx4 at ANY dword address (rows of K = 630 floats).  Never interchangeable
// with the 16-byte aligned types above.
typedef float f32x2u __attribute__((ext_vector_type(2), aligned(4)));
typedef float f32x4u __attribute__((ext_vector_type(4), aligned(4)));
typedef unsigned u32x2 __attribute__((ext_vector_type(2)));
typedef unsigned u32x4 __attribute__((ext_vector_type(4)));
typedef __bf16 bf16x2 __attribute__((ext_vector_type(2)));
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef short s16x4 __attribute__((ext_vector_type(4)));

typedef __amdgpu_buffer_rsrc_t rsrc_t;
// raw buffer descriptor over [base, base + bytes): loads past the end return zeros, stores past it are dropped
__device__ __forceinline__ rsrc_t make_rsrc(const void* base, int bytes) {
  return __builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(base), 0, bytes, 0x00020000);   // word 3: DATA_FORMAT = 32 bit
}

__device__ __forceinline__ f32x4 ld4(const float* p) { return *reinterpret_cast<const f32x4*>(p); }
// v_mfma_f32_16x16x4_f32
__device__ __forceinline__ f32x4 mfma(float a, float b, f32x4 c) {
  return __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, c, 0, 0, 0);
}
// v_mfma_f32_16x16x32_bf16 on operands held as four packed bf16 pairs
__device__ __forceinline__ f32x4 mfma_bf16(const u32x4& a, const u32x4& b, f32x4 c) {
  return __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, a), __builtin_bit_cast(bf16x8, b), c, 0, 0, 0);
}
// max(x, 0) as ONE v_max_f32: fmaxf() is compiled into a canonicalising v_max(x, x) plus the maximum (NaN quieting the
// kernels do not need: a NaN pre-activation stays a NaN either way)
__device__ __forceinline__ float relu1(float x) { float y; asm("v_max_f32 %0, 0, %1" : "=v"(y) : "v"(x)); return y; }
// Values the compiler must not recognise as loop-invariant: everything derived from them (fragment offsets, the small
// vectors w1x / wL / b_l in LDS) would otherwise be hoisted out of the node loop and held in registers -- 80 VGPRs of
// hoisted LDS reads and 200 SGPR offsets in the first build of mono_bwd_wide_k, spilled in turn.
__device__ __forceinline__ int opaque_v(int x) { asm volatile("" : "+v"(x)); return x; }
__device__ __forceinline__ int opaque_s(int x) { asm volatile("" : "+s"(x)); return x; }

// Exact 3 x bf16 split x = hi + mid + lo (hi = rne_bf16(x), mid = rne_bf16(x - hi), lo = x - hi - mid; the method:
// gnf_gemm_split.hip).  cvt_pk_bf16: packed pair of RNE bf16, lo half = bf16(a), hi half = bf16(b).
// (v_cvt_pk_bf16_f32 through the conversion builtin, NOT inline asm: the results feed MFMAs a few instructions later, and the
// compiler's hazard recognizer inserts the VALU-write -> MFMA-read wait states only for instructions it can see.  With the asm
// form mono_fwd_x_k<split> read stale operands: errors of 1e-2 .. 1 that moved with every rebuild)
__device__ __forceinline__ unsigned cvt_pk_bf16(float a, float b) {
  return __builtin_bit_cast(unsigned, __builtin_convertvector(f32x2{a, b}, bf16x2));
}
// x0, x1 -> packed (hi, mid, lo) pairs; the two remainders of a level as ONE packed subtraction (v_pk_add_f32): 9 VALU
// instructions per two elements.  The subtractions are exact (Sterbenz-like: hi is x rounded to 8 significant bits, so
// x - hi has at most 16, and x - hi - mid at most 8)
__device__ __forceinline__ void split3_pair(float x0, float x1, unsigned& h, unsigned& m, unsigned& l) {
  h = cvt_pk_bf16(x0, x1);
  const f32x2 r = f32x2{x0, x1} - f32x2{__uint_as_float(h << 16), __uint_as_float(h & 0xffff0000u)};   // exact
  m = cvt_pk_bf16(r[0], r[1]);
  const f32x2 q = r - f32x2{__uint_as_float(m << 16), __uint_as_float(m & 0xffff0000u)};                // exact
  l = cvt_pk_bf16(q[0], q[1]);
}
// The same split with the conversions as inline asm, for ONE caller: store_split of mono_fwd_wide_split_k, which writes the
// planes to LDS -- no result reaches an MFMA from registers, so the hazard above cannot occur there.  Kept because that
// kernel is 1 .. 5 % slower with the builtin form (the same instructions in another schedule, 41 instead of 117 s_nop:
// profiles/device_header_ab.txt).  NEVER where a result feeds an MFMA.
__device__ __forceinline__ unsigned cvt_pk_bf16_asm(float a, float b) {
  unsigned r;
  asm("v_cvt_pk_bf16_f32 %0, %1, %2" : "=v"(r) : "v"(a), "v"(b));
  return r;
}
__device__ __forceinline__ void split3_pair_asm(float x0, float x1, unsigned& h, unsigned& m, unsigned& l) {
  h = cvt_pk_bf16_asm(x0, x1);
  const f32x2 r = f32x2{x0, x1} - f32x2{__uint_as_float(h << 16), __uint_as_float(h & 0xffff0000u)};   // exact
  m = cvt_pk_bf16_asm(r[0], r[1]);
  const f32x2 q = r - f32x2{__uint_as_float(m << 16), __uint_as_float(m & 0xffff0000u)};                // exact
  l = cvt_pk_bf16_asm(q[0], q[1]);
}
// one value: x -> (hi, mid, lo) as bf16 bit patterns (gemm_split_k, element by element on the way into LDS)
__device__ __forceinline__ void split3(float x, unsigned short& h, unsigned short& m, unsigned short& l) {
  const unsigned ph = cvt_pk_bf16(x, 0.f) & 0xffffu;
  const float r1 = x - __uint_as_float(ph << 16);
  const unsigned pm = cvt_pk_bf16(r1, 0.f) & 0xffffu;
  const float r2 = r1 - __uint_as_float(pm << 16);
  const unsigned pl = cvt_pk_bf16(r2, 0.f) & 0xffffu;
  h = (unsigned short)ph; m = (unsigned short)pm; l = (unsigned short)pl;
}

static inline int gnf_pow2_ge(int64_t v, int cap) {
  int g = 1;
  while (g < v && g < cap) g <<= 1;
  return g;
}

// Sum over the G (power of two <= 64) consecutive lanes of an aligned lane group.
template <int G>
__device__ __forceinline__ float group_sum(float v) {
#pragma unroll
  for (int off = G / 2; off > 0; off >>= 1) v += __shfl_xor(v, off, GNF_WAVE);
  return v;
}

// Philox4x32-10 (Salmon et al. 2011): counter-based, so forward and backward of the DAG
// gate regenerate identical noise from (seed, offset, element index).
__device__ __forceinline__ void philox4x32_10(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3,
                                              uint32_t k0, uint32_t k1, uint32_t out[4]) {
#pragma unroll
  for (int r = 0; r < 10; ++r) {
    // one 32 x 32 -> 64 multiply per product (v_mad_u64_u32) instead of a high and a low one: the quarter-rate integer
    // multiplies are the dominant cost of a call
    const uint64_t p0 = (uint64_t)0xD2511F53u * c0, p1 = (uint64_t)0xCD9E8D57u * c2;
    const uint32_t hi0 = (uint32_t)(p0 >> 32), lo0 = (uint32_t)p0, hi1 = (uint32_t)(p1 >> 32), lo1 = (uint32_t)p1;
    const uint32_t n0 = hi1 ^ c1 ^ k0, n2 = hi0 ^ c3 ^ k1;
    c0 = n0; c1 = lo1; c2 = n2; c3 = lo0;
    k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
  }
  out[0] = c0; out[1] = c1; out[2] = c2; out[3] = c3;
}

// 23-bit uniform centred in its cell: never exactly 0 or 1.  (With 24 bits the + .5f is a rounding tie for words >= 2^23 and
// rounds to even: 16777215.5 -> 16777216, i.e. V = 1.0f about four times per cfg4 step and V / (1 - V) = inf in the
// single-uniform Gumbel ratio.  With 23 bits k + .5 is exactly representable for every k < 2^23.)
__device__ __forceinline__ float u01_open(uint32_t w) {
  return ((float)(w >> 9) + .5f) * (1.0f / 8388608.0f);
}

// 24-bit uniform in [0,1), the resolution torch.rand has for fp32.
__device__ __forceinline__ float u01_24(uint32_t r) { return (float)(r >> 8) * (1.0f / 16777216.0f); }

// out[n] (+)= sum_{p<P} src[p*N + n]   (gnf_rowwise.hip; deterministic order)
int gnf_rowsum_launch(const float* src, float* out, int64_t P, int64_t N, int accumulate, hipStream_t s);
// two independent row sums in one launch
int gnf_rowsum2_launch(const float* src_a, float* out_a, int64_t Pa, int64_t Na, int acc_a, const float* src_b, float* out_b,
                       int64_t Pb, int64_t Nb, int acc_b, hipStream_t s);
// same for tall inputs: two-level, ws >= kRowsumChunks*N floats
constexpr int kRowsumChunks = 1024;
int gnf_rowsum_tall_launch(const float* src, float* out, int64_t P, int64_t N, int accumulate, float* ws,
                           hipStream_t s);
