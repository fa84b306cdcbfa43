// Interventional likelihood: the row reductions of a flow step's tail under do(x_S), i.e. the truncated factorisation
//   log p(x | do(x_S)) = sum over i NOT in S of [ log jac_i + log N(z_i) ]
// as the masked siblings of gnf_nll_reduce_* and of the fused Affine pair (gnf_rowwise.hip, which is not touched).
//
// The mask is a table pin [R, d] of bytes (non-zero: variable i is an intervention target in regime r) and, optionally, a
// regime id per sample; a few KB that stay in cache.  Bytes are read one by one, so the table may sit at any address.
//
// SELECT, NEVER MULTIPLY.  A pinned variable's z overflows and its jac underflows as a matter of course (do(x = 10) on a
// standardised variable), so an excluded term is never formed into a sum or a cotangent: every use below is `free ? term : 0`
// on the ADDEND, or a branch around the load.  0 * inf would be NaN.
//
// A regime id outside [0, R) never indexes the table: the row's logdet / logn -- and in the backward its row of every output
// cotangent -- are NaN.
//
// Kernel forms (as in gnf_rowwise.hip): d <= 64 a row per 16-lane group with one dwordx4 per lane and array at ANY dword
// address and a DPP row sum; few long rows (d >= 256, B <= 4096) a workgroup per row; everything else a row per lane group.
// The backward has no reduction: beyond d = 64 a workgroup takes 256 consecutive columns of one row.  Fixed summation order, no
// atomics, one writer per element, rows never interact.
#include "gnf_common.h"

namespace {

constexpr int kBlock = 256;
constexpr float kLog2Pi = 1.8378770664093453f;     // log(2 pi): summed per element with z^2, as the unmasked kernels do

__device__ __forceinline__ float clampf(float v, float lo, float hi) { return fminf(fmaxf(v, lo), hi); }
__device__ __forceinline__ float qnan() { return __builtin_nanf(""); }

// sum over the hardware's 16-lane row: four DPP adds, VALU only (the row16_sum of gnf_rowwise.hip)
__device__ __forceinline__ float row16_sum(float v) {
  v += __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0xB1, 0xf, 0xf, true));   // quad_perm [1,0,3,2]
  v += __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0x4E, 0xf, 0xf, true));   // quad_perm [2,3,0,1]
  v += __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0x141, 0xf, 0xf, true));  // row_half_mirror
  v += __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0x140, 0xf, 0xf, true));  // row_mirror
  return v;
}

// the row of the pin table sample b reads; -1: its regime id is outside [0, R) and the table must not be indexed
__device__ __forceinline__ int64_t pin_row(const int* __restrict__ regime, int64_t R, int64_t b) {
  if (regime) {
    const int r = regime[b];
    return (r >= 0 && r < R) ? (int64_t)r : (int64_t)-1;
  }
  return R == 1 ? 0 : b;
}

// bit c set: element 4 g + c of the row exists and is FREE (its byte of the table is zero).  prow < 0: nothing is free
__device__ __forceinline__ int free_mask4(const uint8_t* __restrict__ pin, int64_t prow, int d, int g4, int nel) {
  int m = 0;
  if (prow >= 0) {
    const uint8_t* p = pin + prow * d + g4;
#pragma unroll
    for (int c = 0; c < 4; ++c)
      if (c < nel && p[c] == 0) m |= 1 << c;
  }
  return m;
}

// ------------------------------------------------------------------------------------------------ (z, jac) -> row sums
// d <= 64: one row per 16-lane group, lane g holds elements 4 g .. 4 g + 3 (a dwordx4 at any dword address; it may run into
// the next rows, whose elements are not part of nel, and is split up where it would pass the end of the array)
__global__ __launch_bounds__(kBlock) void nll_do_g16_k(const float* __restrict__ z, const float* __restrict__ jac,
                                                       const uint8_t* __restrict__ pin, const int* __restrict__ regime,
                                                       int64_t R, float* __restrict__ logdet, float* __restrict__ logn,
                                                       int64_t B, int d) {
  const int lane = threadIdx.x & 63, g = lane & 15, grp = lane >> 4;
  const int64_t gw = (int64_t)blockIdx.x * (kBlock / 64) + (threadIdx.x >> 6), nw = (int64_t)gridDim.x * (kBlock / 64);
  const int nel = d - 4 * g;
  for (int64_t r0 = gw * 4; r0 < B; r0 += nw * 4) {
    const int64_t row = r0 + grp;
    const bool live = row < B;
    const int64_t prow = live ? pin_row(regime, R, row) : -1;
    const int fm = free_mask4(pin, prow, d, 4 * g, nel);
    const int64_t base = row * d + 4 * g;
    f32x4u zv = f32x4u{0.f, 0.f, 0.f, 0.f}, jv = f32x4u{1.f, 1.f, 1.f, 1.f};
    const bool full = live && nel > 0 && base + 4 <= B * d;
    if (full) {
      zv = __builtin_nontemporal_load(reinterpret_cast<const f32x4u*>(z + base));
      jv = __builtin_nontemporal_load(reinterpret_cast<const f32x4u*>(jac + base));
    } else if (live && nel > 0) {
#pragma unroll
      for (int c = 0; c < 4; ++c)
        if (c < nel) { zv[c] = z[base + c]; jv[c] = jac[base + c]; }
    }
    float sl = 0.f, sn = 0.f;
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      const bool f = (fm >> c) & 1;
      sl += f ? logf(jv[c]) : 0.f;
      sn += f ? kLog2Pi + zv[c] * zv[c] : 0.f;
    }
    sl = row16_sum(sl);
    sn = row16_sum(sn);
    if (g == 0 && live) {
      logdet[row] = prow < 0 ? qnan() : sl;
      logn[row] = prow < 0 ? qnan() : -0.5f * sn;
    }
  }
}

// any d: a row per wavefront, lanes stride over the columns; a pinned element is not loaded
__global__ __launch_bounds__(kBlock) void nll_do_rows_k(const float* __restrict__ z, const float* __restrict__ jac,
                                                        const uint8_t* __restrict__ pin, const int* __restrict__ regime,
                                                        int64_t R, float* __restrict__ logdet, float* __restrict__ logn,
                                                        int64_t B, int64_t d) {
  const int64_t row = (int64_t)blockIdx.x * (kBlock / 64) + (threadIdx.x >> 6);
  const int g = threadIdx.x & 63;
  const bool live = row < B;
  const int64_t prow = live ? pin_row(regime, R, row) : -1;
  float sl = 0.f, sn = 0.f;
  if (prow >= 0) {
    const uint8_t* p = pin + prow * d;
#pragma unroll 4
    for (int64_t i = g; i < d; i += 64) {
      if (p[i] != 0) continue;
      const int64_t e = row * d + i;
      const float v = z[e];
      sl += logf(jac[e]);
      sn += kLog2Pi + v * v;
    }
  }
  sl = group_sum<64>(sl);
  sn = group_sum<64>(sn);
  if (g == 0 && live) {
    logdet[row] = prow < 0 ? qnan() : sl;
    logn[row] = prow < 0 ? qnan() : -0.5f * sn;
  }
}

// few long rows: a workgroup per row, the two sums meet in LDS in wave order
__global__ __launch_bounds__(kBlock) void nll_do_rowblock_k(const float* __restrict__ z, const float* __restrict__ jac,
                                                            const uint8_t* __restrict__ pin, const int* __restrict__ regime,
                                                            int64_t R, float* __restrict__ logdet, float* __restrict__ logn,
                                                            int d) {
  __shared__ float red[2][kBlock / 64];
  const int row = blockIdx.x, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int64_t prow = pin_row(regime, R, row);
  float sl = 0.f, sn = 0.f;
  if (prow >= 0) {
    const uint8_t* p = pin + prow * d;
#pragma unroll 4
    for (int i = threadIdx.x; i < d; i += kBlock) {
      if (p[i] != 0) continue;
      const int64_t e = (int64_t)row * d + i;
      const float v = z[e];
      sl += logf(jac[e]);
      sn += kLog2Pi + v * v;
    }
  }
  sl = group_sum<64>(sl);
  sn = group_sum<64>(sn);
  if (lane == 0) { red[0][wave] = sl; red[1][wave] = sn; }
  __syncthreads();
  if (threadIdx.x == 0) {
    float a = 0.f, b = 0.f;
#pragma unroll
    for (int w = 0; w < kBlock / 64; ++w) { a += red[0][w]; b += red[1][w]; }
    logdet[row] = prow < 0 ? qnan() : a;
    logn[row] = prow < 0 ? qnan() : -0.5f * b;
  }
}

// backward: gz = gz_in - z glogn[b], gjac = glogdet[b] / jac at FREE elements; gz = gz_in (or 0), gjac = +0 at pinned ones
__global__ __launch_bounds__(kBlock) void nll_do_bwd_g16_k(const float* __restrict__ z, const float* __restrict__ jac,
                                                           const uint8_t* __restrict__ pin, const int* __restrict__ regime,
                                                           int64_t R, const float* __restrict__ glogdet,
                                                           const float* __restrict__ glogn, const float* __restrict__ gz_in,
                                                           float* __restrict__ gz, float* __restrict__ gjac, int64_t B, int d) {
  const int lane = threadIdx.x & 63, g = lane & 15, grp = lane >> 4;
  const int64_t gw = (int64_t)blockIdx.x * (kBlock / 64) + (threadIdx.x >> 6), nw = (int64_t)gridDim.x * (kBlock / 64);
  const int nel = d - 4 * g;
  if (nel <= 0) return;
  for (int64_t r0 = gw * 4; r0 < B; r0 += nw * 4) {
    const int64_t row = r0 + grp;
    if (row >= B) continue;
    const int64_t prow = pin_row(regime, R, row);
    const int fm = free_mask4(pin, prow, d, 4 * g, nel);
    const int64_t base = row * d + 4 * g;
    const float gl = glogdet ? glogdet[row] : 0.f, gn = glogn ? glogn[row] : 0.f;
    f32x4u zv = f32x4u{0.f, 0.f, 0.f, 0.f}, jv = f32x4u{1.f, 1.f, 1.f, 1.f}, gv = zv;
    if (base + 4 <= B * d) {
      zv = __builtin_nontemporal_load(reinterpret_cast<const f32x4u*>(z + base));
      jv = __builtin_nontemporal_load(reinterpret_cast<const f32x4u*>(jac + base));
      if (gz_in) gv = __builtin_nontemporal_load(reinterpret_cast<const f32x4u*>(gz_in + base));
    } else {
#pragma unroll
      for (int c = 0; c < 4; ++c)
        if (c < nel) { zv[c] = z[base + c]; jv[c] = jac[base + c]; if (gz_in) gv[c] = gz_in[base + c]; }
    }
    f32x4u oz, oj;
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      const bool f = (fm >> c) & 1;
      oz[c] = prow < 0 ? qnan() : (f ? fmaf(-zv[c], gn, gv[c]) : gv[c]);
      oj[c] = prow < 0 ? qnan() : (f ? gl / jv[c] : 0.f);
    }
    if (nel >= 4) {
      __builtin_nontemporal_store(oz, reinterpret_cast<f32x4u*>(gz + base));
      __builtin_nontemporal_store(oj, reinterpret_cast<f32x4u*>(gjac + base));
    } else {
#pragma unroll
      for (int c = 0; c < 4; ++c)
        if (c < nel) { gz[base + c] = oz[c]; gjac[base + c] = oj[c]; }
    }
  }
}

// d > 64: workgroup (row, chunk) takes columns 256 chunk .. 256 chunk + 255 of its row
__global__ __launch_bounds__(kBlock) void nll_do_bwd_chunk_k(const float* __restrict__ z, const float* __restrict__ jac,
                                                             const uint8_t* __restrict__ pin, const int* __restrict__ regime,
                                                             int64_t R, const float* __restrict__ glogdet,
                                                             const float* __restrict__ glogn, const float* __restrict__ gz_in,
                                                             float* __restrict__ gz, float* __restrict__ gjac, int nchunk,
                                                             int64_t d) {
  const int64_t row = blockIdx.x / nchunk;
  const int64_t i = (int64_t)(blockIdx.x % nchunk) * kBlock + threadIdx.x;
  if (i >= d) return;
  const int64_t prow = pin_row(regime, R, row), e = row * d + i;
  const float gin = gz_in ? gz_in[e] : 0.f;
  if (prow < 0) { gz[e] = qnan(); gjac[e] = qnan(); return; }
  if (pin[prow * d + i] != 0) { gz[e] = gin; gjac[e] = 0.f; return; }
  gz[e] = fmaf(-z[e], glogn ? glogn[row] : 0.f, gin);
  gjac[e] = (glogdet ? glogdet[row] : 0.f) / jac[e];
}

// ------------------------------------------------------------------------------------------------ fused Affine normalizer
// z = x exp(clamp(h1, -5, 2)) + clamp(h0, -5, 5) for EVERY column (a pinned column's z is defined and unused), jac optional,
// logdet / logn reduced over the free columns in the same pass.  Contiguous [B, d, 2] conditioner output, d <= 64:
__global__ __launch_bounds__(kBlock) void affine_do_fwd_g16_k(const float* __restrict__ x, const float* __restrict__ h,
                                                              const uint8_t* __restrict__ pin, const int* __restrict__ regime,
                                                              int64_t R, float* __restrict__ z, float* __restrict__ jac,
                                                              float* __restrict__ logdet, float* __restrict__ logn,
                                                              int64_t B, int d) {
  const int lane = threadIdx.x & 63, g = lane & 15, grp = lane >> 4;
  const int64_t gw = (int64_t)blockIdx.x * (kBlock / 64) + (threadIdx.x >> 6), nw = (int64_t)gridDim.x * (kBlock / 64);
  const int nel = d - 4 * g;
  for (int64_t r0 = gw * 4; r0 < B; r0 += nw * 4) {
    const int64_t row = r0 + grp;
    const bool live = row < B;
    const int64_t prow = live ? pin_row(regime, R, row) : -1;
    const int fm = free_mask4(pin, prow, d, 4 * g, nel);
    const int64_t base = row * d + 4 * g;
    f32x4u xv = f32x4u{0.f, 0.f, 0.f, 0.f}, ha = xv, hb = xv;
    const bool full = live && nel > 0 && base + 4 <= B * d;
    if (full) {
      xv = __builtin_nontemporal_load(reinterpret_cast<const f32x4u*>(x + base));
      ha = __builtin_nontemporal_load(reinterpret_cast<const f32x4u*>(h + 2 * base));
      hb = __builtin_nontemporal_load(reinterpret_cast<const f32x4u*>(h + 2 * base + 4));
    } else if (live && nel > 0) {
#pragma unroll
      for (int c = 0; c < 4; ++c)
        if (c < nel) {
          xv[c] = x[base + c];
          const float a0 = h[2 * (base + c)], a1 = h[2 * (base + c) + 1];
          if (c < 2) { ha[2 * c] = a0; ha[2 * c + 1] = a1; } else { hb[2 * c - 4] = a0; hb[2 * c - 3] = a1; }
        }
    }
    const float h0[4] = {ha[0], ha[2], hb[0], hb[2]}, h1[4] = {ha[1], ha[3], hb[1], hb[3]};
    f32x4u zv, jv;
    float sl = 0.f, sn = 0.f;
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      const float mu = clampf(h0[c], -5.f, 5.f), ls = clampf(h1[c], -5.f, 2.f);
      const float sg = expf(ls);
      zv[c] = fmaf(xv[c], sg, mu);
      jv[c] = sg;
      const bool f = (fm >> c) & 1;
      sl += f ? ls : 0.f;
      sn += f ? kLog2Pi + zv[c] * zv[c] : 0.f;
    }
    if (live && nel >= 4) {
      __builtin_nontemporal_store(zv, reinterpret_cast<f32x4u*>(z + base));
      if (jac) __builtin_nontemporal_store(jv, reinterpret_cast<f32x4u*>(jac + base));
    } else if (live) {
#pragma unroll
      for (int c = 0; c < 4; ++c)
        if (c < nel) { z[base + c] = zv[c]; if (jac) jac[base + c] = jv[c]; }
    }
    sl = row16_sum(sl);
    if (logdet && g == 0 && live) logdet[row] = prow < 0 ? qnan() : sl;
    if (logn) { sn = row16_sum(sn); if (g == 0 && live) logn[row] = prow < 0 ? qnan() : -0.5f * sn; }
  }
}

// any strides of h (MADE's permuted view): a row per G-lane group, lanes stride over the columns
template <int G>
__global__ __launch_bounds__(kBlock) void affine_do_fwd_k(const float* __restrict__ x, const float* __restrict__ h, int64_t h_sb,
                                                          int64_t h_sd, int64_t h_sc, const uint8_t* __restrict__ pin,
                                                          const int* __restrict__ regime, int64_t R, float* __restrict__ z,
                                                          float* __restrict__ jac, float* __restrict__ logdet,
                                                          float* __restrict__ logn, int64_t B, int64_t d) {
  const int64_t row = (int64_t)blockIdx.x * (kBlock / G) + threadIdx.x / G;
  const int g = threadIdx.x % G;
  const bool live = row < B;
  const int64_t prow = live ? pin_row(regime, R, row) : -1;
  float sl = 0.f, sn = 0.f;
  if (live) {
#pragma unroll 4
    for (int64_t i = g; i < d; i += G) {
      const int64_t hi = row * h_sb + i * h_sd, e = row * d + i;
      const float mu = clampf(h[hi], -5.f, 5.f), ls = clampf(h[hi + h_sc], -5.f, 2.f);
      const float sg = expf(ls), zv = fmaf(x[e], sg, mu);
      z[e] = zv;
      if (jac) jac[e] = sg;
      const bool f = prow >= 0 && pin[prow * d + i] == 0;
      sl += f ? ls : 0.f;
      sn += f ? kLog2Pi + zv * zv : 0.f;
    }
  }
  sl = group_sum<G>(sl);
  sn = group_sum<G>(sn);
  if (g == 0 && live) {
    if (logdet) logdet[row] = prow < 0 ? qnan() : sl;
    if (logn) logn[row] = prow < 0 ? qnan() : -0.5f * sn;
  }
}

// few long rows: a workgroup per row
__global__ __launch_bounds__(kBlock) void affine_do_fwd_rowblock_k(const float* __restrict__ x, const float* __restrict__ h,
                                                                   int64_t h_sb, int64_t h_sd, int64_t h_sc,
                                                                   const uint8_t* __restrict__ pin, const int* __restrict__ regime,
                                                                   int64_t R, float* __restrict__ z, float* __restrict__ jac,
                                                                   float* __restrict__ logdet, float* __restrict__ logn, int d) {
  __shared__ float red[2][kBlock / 64];
  const int row = blockIdx.x, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int64_t prow = pin_row(regime, R, row);
  float sl = 0.f, sn = 0.f;
#pragma unroll 4
  for (int i = threadIdx.x; i < d; i += kBlock) {
    const int64_t hi = row * h_sb + i * h_sd, e = (int64_t)row * d + i;
    const float mu = clampf(h[hi], -5.f, 5.f), ls = clampf(h[hi + h_sc], -5.f, 2.f);
    const float sg = expf(ls), zv = fmaf(x[e], sg, mu);
    z[e] = zv;
    if (jac) jac[e] = sg;
    const bool f = prow >= 0 && pin[prow * d + i] == 0;
    sl += f ? ls : 0.f;
    sn += f ? kLog2Pi + zv * zv : 0.f;
  }
  sl = group_sum<64>(sl);
  sn = group_sum<64>(sn);
  if (lane == 0) { red[0][wave] = sl; red[1][wave] = sn; }
  __syncthreads();
  if (threadIdx.x == 0) {
    float a = 0.f, b = 0.f;
#pragma unroll
    for (int w = 0; w < kBlock / 64; ++w) { a += red[0][w]; b += red[1][w]; }
    if (logdet) logdet[row] = prow < 0 ? qnan() : a;
    if (logn) logn[row] = prow < 0 ? qnan() : -0.5f * b;
  }
}

// One element of the Affine backward.  gz / gjac act on every element as in gnf_affine_bwd; the ROW cotangents glogdet / glogn
// (gl, gn) enter only where the element is free.  bad: the sample's regime id is out of range, its outputs are NaN.
__device__ __forceinline__ void affine_do_bwd_elem(float xv, float h0, float h1, float gzv, float gjv, float gl, float gn,
                                                   bool free, bool bad, float& ox, float& o0, float& o1) {
  // torch clamp backward passes the gradient where min <= v <= max (boundaries included)
  const float m0 = (h0 >= -5.f && h0 <= 5.f) ? 1.f : 0.f;
  const float m1 = (h1 >= -5.f && h1 <= 2.f) ? 1.f : 0.f;
  const float sg = expf(clampf(h1, -5.f, 2.f));
  const float gze = free ? fmaf(-fmaf(xv, sg, clampf(h0, -5.f, 5.f)), gn, gzv) : gzv;   // + d logN / dz = -z, free only
  const float gle = free ? gl : 0.f;
  ox = bad ? qnan() : gze * sg;
  o0 = bad ? qnan() : gze * m0;
  o1 = bad ? qnan() : (fmaf(gze * xv, sg, gjv * sg) + gle) * m1;
}

// contiguous [B, d, 2] h and gh, d <= 64
__global__ __launch_bounds__(kBlock) void affine_do_bwd_g16_k(const float* __restrict__ x, const float* __restrict__ h,
                                                              const uint8_t* __restrict__ pin, const int* __restrict__ regime,
                                                              int64_t R, const float* __restrict__ gz,
                                                              const float* __restrict__ gjac, const float* __restrict__ glogdet,
                                                              const float* __restrict__ glogn, float* __restrict__ gx,
                                                              float* __restrict__ gh, int64_t B, int d) {
  const int lane = threadIdx.x & 63, g = lane & 15, grp = lane >> 4;
  const int64_t gw = (int64_t)blockIdx.x * (kBlock / 64) + (threadIdx.x >> 6), nw = (int64_t)gridDim.x * (kBlock / 64);
  const int nel = d - 4 * g;
  if (nel <= 0) return;
  for (int64_t r0 = gw * 4; r0 < B; r0 += nw * 4) {
    const int64_t row = r0 + grp;
    if (row >= B) continue;
    const int64_t prow = pin_row(regime, R, row);
    const int fm = free_mask4(pin, prow, d, 4 * g, nel);
    const int64_t base = row * d + 4 * g;
    const float gl = glogdet ? glogdet[row] : 0.f, gn = glogn ? glogn[row] : 0.f;
    f32x4u xv = f32x4u{0.f, 0.f, 0.f, 0.f}, ha = xv, hb = xv, gv = xv, jv = xv;
    if (base + 4 <= B * d) {
      xv = __builtin_nontemporal_load(reinterpret_cast<const f32x4u*>(x + base));
      ha = __builtin_nontemporal_load(reinterpret_cast<const f32x4u*>(h + 2 * base));
      hb = __builtin_nontemporal_load(reinterpret_cast<const f32x4u*>(h + 2 * base + 4));
      if (gz) gv = __builtin_nontemporal_load(reinterpret_cast<const f32x4u*>(gz + base));
      if (gjac) jv = __builtin_nontemporal_load(reinterpret_cast<const f32x4u*>(gjac + base));
    } else {
#pragma unroll
      for (int c = 0; c < 4; ++c)
        if (c < nel) {
          xv[c] = x[base + c];
          const float a0 = h[2 * (base + c)], a1 = h[2 * (base + c) + 1];
          if (c < 2) { ha[2 * c] = a0; ha[2 * c + 1] = a1; } else { hb[2 * c - 4] = a0; hb[2 * c - 3] = a1; }
          if (gz) gv[c] = gz[base + c];
          if (gjac) jv[c] = gjac[base + c];
        }
    }
    const float h0[4] = {ha[0], ha[2], hb[0], hb[2]}, h1[4] = {ha[1], ha[3], hb[1], hb[3]};
    f32x4u ox, oa, ob;
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      float a, o0, o1;
      affine_do_bwd_elem(xv[c], h0[c], h1[c], gv[c], jv[c], gl, gn, (fm >> c) & 1, prow < 0, a, o0, o1);
      ox[c] = a;
      if (c < 2) { oa[2 * c] = o0; oa[2 * c + 1] = o1; } else { ob[2 * c - 4] = o0; ob[2 * c - 3] = o1; }
    }
    if (nel >= 4) {
      if (gx) __builtin_nontemporal_store(ox, reinterpret_cast<f32x4u*>(gx + base));
      __builtin_nontemporal_store(oa, reinterpret_cast<f32x4u*>(gh + 2 * base));
      __builtin_nontemporal_store(ob, reinterpret_cast<f32x4u*>(gh + 2 * base + 4));
    } else {
#pragma unroll
      for (int c = 0; c < 4; ++c)
        if (c < nel) {
          if (gx) gx[base + c] = ox[c];
          gh[2 * (base + c)] = c < 2 ? oa[2 * c] : ob[2 * c - 4];
          gh[2 * (base + c) + 1] = c < 2 ? oa[2 * c + 1] : ob[2 * c - 3];
        }
    }
  }
}

// any strides, d <= 64: a row per G-lane group
template <int G>
__global__ __launch_bounds__(kBlock) void affine_do_bwd_k(const float* __restrict__ x, const float* __restrict__ h, int64_t h_sb,
                                                          int64_t h_sd, int64_t h_sc, const uint8_t* __restrict__ pin,
                                                          const int* __restrict__ regime, int64_t R, const float* __restrict__ gz,
                                                          const float* __restrict__ gjac, const float* __restrict__ glogdet,
                                                          const float* __restrict__ glogn, float* __restrict__ gx,
                                                          float* __restrict__ gh, int64_t g_sb, int64_t g_sd, int64_t g_sc,
                                                          int64_t B, int64_t d) {
  const int64_t row = (int64_t)blockIdx.x * (kBlock / G) + threadIdx.x / G;
  const int g = threadIdx.x % G;
  if (row >= B) return;
  const int64_t prow = pin_row(regime, R, row);
  const float gl = glogdet ? glogdet[row] : 0.f, gn = glogn ? glogn[row] : 0.f;
#pragma unroll 2
  for (int64_t i = g; i < d; i += G) {
    const int64_t hi = row * h_sb + i * h_sd, e = row * d + i, gi = row * g_sb + i * g_sd;
    const bool f = prow >= 0 && pin[prow * d + i] == 0;
    float ox, o0, o1;
    affine_do_bwd_elem(x[e], h[hi], h[hi + h_sc], gz ? gz[e] : 0.f, gjac ? gjac[e] : 0.f, gl, gn, f, prow < 0, ox, o0, o1);
    if (gx) gx[e] = ox;
    gh[gi] = o0;
    gh[gi + g_sc] = o1;
  }
}

// any strides, d > 64: workgroup (row, chunk) takes 256 consecutive columns of its row
__global__ __launch_bounds__(kBlock) void affine_do_bwd_chunk_k(const float* __restrict__ x, const float* __restrict__ h,
                                                                int64_t h_sb, int64_t h_sd, int64_t h_sc,
                                                                const uint8_t* __restrict__ pin, const int* __restrict__ regime,
                                                                int64_t R, const float* __restrict__ gz,
                                                                const float* __restrict__ gjac, const float* __restrict__ glogdet,
                                                                const float* __restrict__ glogn, float* __restrict__ gx,
                                                                float* __restrict__ gh, int64_t g_sb, int64_t g_sd, int64_t g_sc,
                                                                int nchunk, int64_t d) {
  const int64_t row = blockIdx.x / nchunk;
  const int64_t i = (int64_t)(blockIdx.x % nchunk) * kBlock + threadIdx.x;
  if (i >= d) return;
  const int64_t prow = pin_row(regime, R, row);
  const int64_t hi = row * h_sb + i * h_sd, e = row * d + i, gi = row * g_sb + i * g_sd;
  const bool f = prow >= 0 && pin[prow * d + i] == 0;
  float ox, o0, o1;
  affine_do_bwd_elem(x[e], h[hi], h[hi + h_sc], gz ? gz[e] : 0.f, gjac ? gjac[e] : 0.f, glogdet ? glogdet[row] : 0.f,
                     glogn ? glogn[row] : 0.f, f, prow < 0, ox, o0, o1);
  if (gx) gx[e] = ox;
  gh[gi] = o0;
  gh[gi + g_sc] = o1;
}

// ------------------------------------------------------------------------------------------------------------- host side
// grid of the 16-lane-group kernels: 16 rows per workgroup and trip, grid-stride beyond 4096 workgroups
inline unsigned g16_grid(int64_t B) {
  int64_t grid = (B + 15) / 16;
  if (grid > 256 * 16) grid = 256 * 16;
  return (unsigned)grid;
}

// the common operand checks after B == 0 has been answered; 0 = go on
inline int do_args(const void* pin, const void* regime, int64_t R, int64_t B) {
  if (!pin || R <= 0) return GNF_EINVAL;
  if (!regime && R != 1 && R != B) return GNF_EINVAL;
  return 0;
}

// lane-group width of the strided Affine kernels: 8, 32 or 64 lanes per row
inline int affine_do_group(int64_t d) { return d <= 8 ? 8 : (d <= 32 ? 32 : 64); }

}  // namespace

extern "C" {

int gnf_nll_do_fwd(const float* z, const float* jac, const uint8_t* pin, const int32_t* regime, int64_t R, float* logdet,
                   float* logn, int64_t B, int64_t d, gnf_stream_t stream) {
  if (B < 0 || d <= 0) return GNF_EINVAL;
  if (B == 0) return 0;
  if (const int rc = do_args(pin, regime, R, B)) return rc;
  if (!z || !jac || !logdet || !logn) return GNF_EINVAL;
  hipStream_t s = (hipStream_t)stream;
  if (d <= 64) {
    hipLaunchKernelGGL(nll_do_g16_k, dim3(g16_grid(B)), dim3(kBlock), 0, s, z, jac, pin, regime, R, logdet, logn, B, (int)d);
  } else if (d >= 256 && B <= 4096) {
    if (d > INT32_MAX) return GNF_ESHAPE;
    hipLaunchKernelGGL(nll_do_rowblock_k, dim3((unsigned)B), dim3(kBlock), 0, s, z, jac, pin, regime, R, logdet, logn, (int)d);
  } else {
    const int64_t grid = (B + kBlock / 64 - 1) / (kBlock / 64);
    if (grid > INT32_MAX) return GNF_ESHAPE;
    hipLaunchKernelGGL(nll_do_rows_k, dim3((unsigned)grid), dim3(kBlock), 0, s, z, jac, pin, regime, R, logdet, logn, B, d);
  }
  GNF_LAUNCH_CHECK();
  return 0;
}

int gnf_nll_do_bwd(const float* z, const float* jac, const uint8_t* pin, const int32_t* regime, int64_t R,
                   const float* glogdet, const float* glogn, const float* gz_in, float* gz, float* gjac, int64_t B, int64_t d,
                   gnf_stream_t stream) {
  if (B < 0 || d <= 0) return GNF_EINVAL;
  if (B == 0) return 0;
  if (const int rc = do_args(pin, regime, R, B)) return rc;
  if (!z || !jac || !gz || !gjac) return GNF_EINVAL;
  hipStream_t s = (hipStream_t)stream;
  if (d <= 64) {
    hipLaunchKernelGGL(nll_do_bwd_g16_k, dim3(g16_grid(B)), dim3(kBlock), 0, s, z, jac, pin, regime, R, glogdet, glogn, gz_in, gz,
                       gjac, B, (int)d);
  } else {
    const int64_t nchunk = (d + kBlock - 1) / kBlock;
    if (nchunk > INT32_MAX || B * nchunk > INT32_MAX) return GNF_ESHAPE;
    hipLaunchKernelGGL(nll_do_bwd_chunk_k, dim3((unsigned)(B * nchunk)), dim3(kBlock), 0, s, z, jac, pin, regime, R, glogdet,
                       glogn, gz_in, gz, gjac, (int)nchunk, d);
  }
  GNF_LAUNCH_CHECK();
  return 0;
}

int gnf_affine_do_fwd(const float* x, const float* h, int64_t h_sb, int64_t h_sd, int64_t h_sc, const uint8_t* pin,
                      const int32_t* regime, int64_t R, float* z, float* jac, float* logdet, float* logn, int64_t B,
                      int64_t d, gnf_stream_t stream) {
  if (B < 0 || d <= 0) return GNF_EINVAL;
  if (B == 0) return 0;
  if (const int rc = do_args(pin, regime, R, B)) return rc;
  if (!x || !h || !z) return GNF_EINVAL;
  hipStream_t s = (hipStream_t)stream;
  if (d <= 64 && h_sc == 1 && h_sd == 2 && h_sb == 2 * d) {
    hipLaunchKernelGGL(affine_do_fwd_g16_k, dim3(g16_grid(B)), dim3(kBlock), 0, s, x, h, pin, regime, R, z, jac, logdet, logn, B,
                       (int)d);
  } else if (d >= 256 && B <= 4096) {
    if (d > INT32_MAX) return GNF_ESHAPE;
    hipLaunchKernelGGL(affine_do_fwd_rowblock_k, dim3((unsigned)B), dim3(kBlock), 0, s, x, h, h_sb, h_sd, h_sc, pin, regime, R, z,
                       jac, logdet, logn, (int)d);
  } else {
    const int G = affine_do_group(d);
    const int64_t grid = (B + kBlock / G - 1) / (kBlock / G);
    if (grid > INT32_MAX) return GNF_ESHAPE;
    const dim3 gr((unsigned)grid), bl(kBlock);
    if (G == 8) hipLaunchKernelGGL((affine_do_fwd_k<8>), gr, bl, 0, s, x, h, h_sb, h_sd, h_sc, pin, regime, R, z, jac, logdet, logn, B, d);
    else if (G == 32) hipLaunchKernelGGL((affine_do_fwd_k<32>), gr, bl, 0, s, x, h, h_sb, h_sd, h_sc, pin, regime, R, z, jac, logdet, logn, B, d);
    else hipLaunchKernelGGL((affine_do_fwd_k<64>), gr, bl, 0, s, x, h, h_sb, h_sd, h_sc, pin, regime, R, z, jac, logdet, logn, B, d);
  }
  GNF_LAUNCH_CHECK();
  return 0;
}

int gnf_affine_do_bwd(const float* x, const float* h, int64_t h_sb, int64_t h_sd, int64_t h_sc, const uint8_t* pin,
                      const int32_t* regime, int64_t R, const float* gz, const float* gjac, const float* glogdet,
                      const float* glogn, float* gx, float* gh, int64_t g_sb, int64_t g_sd, int64_t g_sc, int64_t B, int64_t d,
                      gnf_stream_t stream) {
  if (B < 0 || d <= 0) return GNF_EINVAL;
  if (B == 0) return 0;
  if (const int rc = do_args(pin, regime, R, B)) return rc;
  if (!x || !h || !gh) return GNF_EINVAL;
  hipStream_t s = (hipStream_t)stream;
  if (d <= 64 && h_sc == 1 && h_sd == 2 && h_sb == 2 * d && g_sc == 1 && g_sd == 2 && g_sb == 2 * d) {
    hipLaunchKernelGGL(affine_do_bwd_g16_k, dim3(g16_grid(B)), dim3(kBlock), 0, s, x, h, pin, regime, R, gz, gjac, glogdet, glogn,
                       gx, gh, B, (int)d);
  } else if (d > 64) {
    const int64_t nchunk = (d + kBlock - 1) / kBlock;
    if (nchunk > INT32_MAX || B * nchunk > INT32_MAX) return GNF_ESHAPE;
    hipLaunchKernelGGL(affine_do_bwd_chunk_k, dim3((unsigned)(B * nchunk)), dim3(kBlock), 0, s, x, h, h_sb, h_sd, h_sc, pin, regime,
                       R, gz, gjac, glogdet, glogn, gx, gh, g_sb, g_sd, g_sc, (int)nchunk, d);
  } else {
    const int G = affine_do_group(d);
    const int64_t grid = (B + kBlock / G - 1) / (kBlock / G);
    if (grid > INT32_MAX) return GNF_ESHAPE;
    const dim3 gr((unsigned)grid), bl(kBlock);
    if (G == 8) hipLaunchKernelGGL((affine_do_bwd_k<8>), gr, bl, 0, s, x, h, h_sb, h_sd, h_sc, pin, regime, R, gz, gjac, glogdet, glogn, gx, gh, g_sb, g_sd, g_sc, B, d);
    else if (G == 32) hipLaunchKernelGGL((affine_do_bwd_k<32>), gr, bl, 0, s, x, h, h_sb, h_sd, h_sc, pin, regime, R, gz, gjac, glogdet, glogn, gx, gh, g_sb, g_sd, g_sc, B, d);
    else hipLaunchKernelGGL((affine_do_bwd_k<64>), gr, bl, 0, s, x, h, h_sb, h_sd, h_sc, pin, regime, R, gz, gjac, glogdet, glogn, gx, gh, g_sb, g_sd, g_sc, B, d);
  }
  GNF_LAUNCH_CHECK();
  return 0;
}

}  // extern "C"
