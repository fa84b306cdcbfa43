// Batch preparation of the image driver (train_image.py) in ONE launch: gather rows of the uint8 data set, optional
// horizontal flip, uniform dequantisation noise, the squeeze into [alpha, 1 - alpha], the logit, and the per-row term
// sum_j log2 y + log2 (1 - y) of the bits-per-pixel formula (reference lib/transform.py:5-21, ImageExperiments.py:33-37, :97).
//
// HBM-bound by construction: 1 byte read and 4 bytes written per element (+ 4 read with injected uniforms), no float
// temporaries.  One workgroup per output row; a lane owns the element quads q = tid, tid + 256, ... of the row.
//
// TWO forms, bit-identical: image_prep_k<true> reads a quad as ONE dword and writes ONE float4 (d % 4 == 0, data dword-
// aligned, x / u 16-byte aligned, W % 4 == 0 when a row may be flipped -- the mirrored quad is then an aligned quad read
// backwards); image_prep_k<false> moves the same quad byte by byte and float by float, at any address and any d.  Both call
// prep_elem() per element, add the row term in element order inside a lane and reduce the lanes in one fixed tree, so the
// path taken changes no bit of x or of bpp_term.
//
// 1 - y is NOT formed by subtraction: yc = alpha + (1 - 2 alpha) (256 - pixel - u) / 256 is the same number with the
// rounding of a small quantity (256 - pixel is exact, and so is (256 - pixel) - u for every 24-bit uniform), where 1 - y
// loses everything below 6e-8 -- 3 % of 1 - y for a white pixel at alpha = 1e-6.
#include "gnf_common.h"

namespace {

constexpr int kPrepBlock = 256;

struct PrepElem { float x, t; };     // the logit, and log2 y + log2 (1 - y)

// v_log_f32 (base 2, 1 ulp) twice: arguments in [alpha, 1), never subnormal for alpha >= 2^-126
__device__ __forceinline__ PrepElem prep_elem(float pix, float u, float alpha, float scale) {
#pragma clang fp contract(off)
  const float y = fmaf(scale, (pix + u) * (1.f / 256.f), alpha);
  const float yc = fmaf(scale, ((256.f - pix) - u) * (1.f / 256.f), alpha);
  const float ly = __builtin_amdgcn_logf(y), lc = __builtin_amdgcn_logf(yc);
  PrepElem r;
  r.x = (ly - lc) * 0.6931471805599453f;
  r.t = ly + lc;
  return r;
}

// Philox words of the element quad e >> 2: counter (e >> 2, offset), key seed.  e < 2^63, so bit 31 of the second counter
// word is never set by an element -- the row coin below sets it.
__device__ __forceinline__ void elem_words(uint64_t quad, uint64_t seed, uint64_t offset, uint32_t r[4]) {
  philox4x32_10((uint32_t)quad, (uint32_t)(quad >> 32), (uint32_t)offset, (uint32_t)(offset >> 32), (uint32_t)seed,
                (uint32_t)(seed >> 32), r);
}

template <bool VEC>
__global__ __launch_bounds__(kPrepBlock) void image_prep_k(const uint8_t* __restrict__ data, int64_t n_rows,
                                                           const int32_t* __restrict__ rows, int flip_mode,
                                                           const uint8_t* __restrict__ flip, int W, int64_t d,
                                                           const float* __restrict__ u, uint64_t seed, uint64_t offset,
                                                           float alpha, float scale, float* __restrict__ x,
                                                           float* __restrict__ bpp_term) {
  const int64_t b = blockIdx.x;
  int64_t row = rows ? (int64_t)rows[b] : b;
  row = row < 0 ? 0 : (row >= n_rows ? n_rows - 1 : row);          // clamped: never a read outside the data set
  bool flipped = false;
  if (flip_mode == 1) {
    flipped = flip[b] != 0;
  } else if (flip_mode == 2) {
    uint32_t c[4];
    philox4x32_10((uint32_t)b, (uint32_t)((uint64_t)b >> 32) | 0x80000000u, (uint32_t)offset, (uint32_t)(offset >> 32),
                  (uint32_t)seed, (uint32_t)(seed >> 32), c);
    flipped = (c[0] >> 31) != 0;
  }
  const uint8_t* __restrict__ src = data + row * d;
  const int64_t nq = (d + 3) >> 2;
  float acc = 0.f;
  for (int64_t q = threadIdx.x; q < nq; q += kPrepBlock) {
    const int64_t j0 = 4 * q, e0 = b * d + j0;
    float pix[4], un[4];
    int nv = 4;
    if (VEC) {
      int64_t s0 = j0;
      if (flipped) {
        const int64_t w0 = j0 % W;
        s0 = j0 - w0 + (W - 4 - w0);                                 // the mirrored quad, read backwards
      }
      uint32_t pk = *reinterpret_cast<const uint32_t*>(src + s0);
      if (flipped) pk = __builtin_bswap32(pk);
#pragma unroll
      for (int h = 0; h < 4; ++h) pix[h] = (float)((pk >> (8 * h)) & 0xffu);
      if (u) {
        const float4 t = *reinterpret_cast<const float4*>(u + e0);
        un[0] = t.x; un[1] = t.y; un[2] = t.z; un[3] = t.w;
      } else {
        uint32_t r[4];
        elem_words((uint64_t)e0 >> 2, seed, offset, r);              // e0 % 4 == 0: the quad is one Philox call
#pragma unroll
        for (int h = 0; h < 4; ++h) un[h] = u01_open(r[h]);
      }
    } else {
      nv = d - j0 < 4 ? (int)(d - j0) : 4;
      uint32_t r[4] = {0u, 0u, 0u, 0u};
      uint64_t have = ~(uint64_t)0;                                  // no element quad: e >> 2 < 2^62
#pragma unroll
      for (int h = 0; h < 4; ++h) {
        pix[h] = 0.f; un[h] = .5f;
        if (h < nv) {
          const int64_t j = j0 + h, w = j % W;
          pix[h] = (float)src[flipped ? j - w + (W - 1 - w) : j];
          const uint64_t e = (uint64_t)(e0 + h);
          if (u) {
            un[h] = u[e];
          } else {
            if ((e >> 2) != have) { have = e >> 2; elem_words(have, seed, offset, r); }
            const uint32_t k = (uint32_t)e & 3u;                     // selects, not a runtime index (no scratch)
            un[h] = u01_open(k == 0 ? r[0] : k == 1 ? r[1] : k == 2 ? r[2] : r[3]);
          }
        }
      }
    }
    PrepElem o[4];
#pragma unroll
    for (int h = 0; h < 4; ++h) o[h] = prep_elem(pix[h], un[h], alpha, scale);
    if (VEC) {
      *reinterpret_cast<float4*>(x + e0) = make_float4(o[0].x, o[1].x, o[2].x, o[3].x);
    } else {
#pragma unroll
      for (int h = 0; h < 4; ++h)
        if (h < nv) x[e0 + h] = o[h].x;
    }
#pragma unroll
    for (int h = 0; h < 4; ++h)
      if (h < nv) acc += o[h].t;
  }
  if (bpp_term) {                                                    // fixed tree: lanes of a wave, then the four waves in order
    __shared__ float part[kPrepBlock / GNF_WAVE];
    acc = group_sum<GNF_WAVE>(acc);
    if ((threadIdx.x & (GNF_WAVE - 1)) == 0) part[threadIdx.x / GNF_WAVE] = acc;
    __syncthreads();
    if (threadIdx.x == 0) {
      float s = part[0];
#pragma unroll
      for (int k = 1; k < kPrepBlock / GNF_WAVE; ++k) s += part[k];
      bpp_term[b] = s;
    }
  }
}

inline bool aligned_to(const void* p, uintptr_t a) { return (reinterpret_cast<uintptr_t>(p) & (a - 1)) == 0; }

}  // namespace

extern "C" int gnf_image_prep(const unsigned char* data, int64_t n_rows, const int32_t* rows, int flip_mode,
                              const unsigned char* flip, int C, int H, int W, const float* u, uint64_t seed, uint64_t offset,
                              float alpha, float* x, float* bpp_term, int64_t B, gnf_stream_t stream) {
  if (B < 0 || C < 1 || H < 1 || W < 1 || flip_mode < 0 || flip_mode > 2) return GNF_EINVAL;
  if (!(alpha >= 0.f && alpha < .5f)) return GNF_EINVAL;
  if (B == 0) return 0;
  if (!data || !x || n_rows < 1 || (flip_mode == 1 && !flip)) return GNF_EINVAL;
  if (!rows && B > n_rows) return GNF_EINVAL;
  if (!aligned_to(x, 4) || !aligned_to(u, 4) || !aligned_to(bpp_term, 4) || !aligned_to(rows, 4)) return GNF_EINVAL;
  if (B > 0x7fffffff) return GNF_ESHAPE;
  const int64_t d = (int64_t)C * H * W;
  const float scale = 1.f - 2.f * alpha;
  const bool vec = d % 4 == 0 && aligned_to(data, 4) && aligned_to(x, 16) && aligned_to(u, 16) &&
                   (flip_mode == 0 || W % 4 == 0);
  hipStream_t s = static_cast<hipStream_t>(stream);
  if (vec)
    hipLaunchKernelGGL(image_prep_k<true>, dim3((unsigned)B), dim3(kPrepBlock), 0, s, data, n_rows, rows, flip_mode, flip, W,
                       d, u, seed, offset, alpha, scale, x, bpp_term);
  else
    hipLaunchKernelGGL(image_prep_k<false>, dim3((unsigned)B), dim3(kPrepBlock), 0, s, data, n_rows, rows, flip_mode, flip,
                       W, d, u, seed, offset, alpha, scale, x, bpp_term);
  GNF_LAUNCH_CHECK();
  return 0;
}
