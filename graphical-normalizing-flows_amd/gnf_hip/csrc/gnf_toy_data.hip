// Training batches of the toy driver (train_toy.py) in ONE launch: the fourteen 2-D base problems of the reference's
// lib/toy_data.py:62-224, drawn on the device from Philox4x32-10 -- no generator state, no host loop, no host-to-device copy.
// A batch row holds P blocks of two columns (the composites of :16-59 are block lists chosen by the host); block p of sample
// b is one draw of the base problem kinds[p], optionally multiplied by col_scale[2p], col_scale[2p + 1].
//
// One thread per (sample, block).  A WAVE holds one block of 64 consecutive samples, so the problem is a scalar of the wave
// and a composite pays for no divergence: with lane = (sample, block) pairs in row order every wave of 8-MIX ran all eight
// problems one after the other (9.8 us a batch of 100 against 4.0 us in this form, 15.9 against 6.2 us at B = 65 536:
// profiles/toy_data_ab.txt, parts 2 and 4).  The four waves of a workgroup take neighbouring blocks of the same samples, so the 8-byte stores
// of a row meet in the same lines of L2.  No LDS, no scratch: the block list travels as eight 4-bit fields of one kernel
// argument, the scales as a by-value struct read from the kernel-argument segment with a scalar index, and the uniforms are
// picked by name, never by a runtime index.
//
// UNIFORMS.  u_0 .. u_7 of (b, p): u_{4q + w} = u01_open(r_q[w]), r_q = philox4x32_10(counter (lo32(b), (p << 8) | q,
// lo32(offset), hi32(offset)), key (lo32(seed), hi32(seed))), q = 0, 1 (q = 1 is drawn by 2spirals only); or the eight floats
// u[b, p, 0..7] of the caller.  N(a, c) below is the Box-Muller pair  r = sqrt(-2 ln u_a):  n0 = r cos(2 pi u_c),
// n1 = r sin(2 pi u_c).  A coin is u >= .5; a class index among K is the number of thresholds j/K (rounded to fp32) that u
// reaches -- comparisons, so that the fp32 kernel and an fp64 evaluation of the same uniforms never disagree on a class.
//
//   kind             variates                         columns
//   0 2igaussians    N(0,1), class u_2 of 2           .75 n + centre, centres (+-2, 0)
//   1 2gaussians     N(0,1), class u_2 of 2           .75 n + centre, centres (2,-2), (-2,2)
//   2 4gaussians     N(0,1), class u_2 of 4           .75 n + centre, centres (2,-2), (-2,2), (2,2), (-2,-2)
//   3 8gaussians     N(0,1), class u_2 of 8           (.5 n + centre) / 1.414, centres 4 (+-1, 0), 4 (0, +-1), 4 (+-1, +-1) / sqrt 2
//   4 swissroll      t from u_0, N(1,2)               t = 1.5 pi (1 + 2 u_0):  (t cos t + n0) / 5, (t sin t + n1) / 5
//   5 circles        ring coin u_0, angle u_1, N(2,3) f = u_0 >= .5 ? .5 : 1, a = 2 pi u_1:  3 (f cos a + .08 n0), 3 (f sin a + .08 n1)
//   6 moons          moon coin u_0, angle u_1, N(2,3) a = pi u_1; outer (cos a, sin a), inner (1 - cos a, 1 - sin a - .5); + .1 n;
//                                                     x 2 + (-1, -.2)
//   7 pinwheel       N(0,1), class u_2 of 5           f = (1 + .3 n0, .1 n1), a = 2 pi k / 5 + .25 exp f0:
//                                                     2 (f0 cos a + f1 sin a), 2 (f1 cos a - f0 sin a)
//   8 2spirals       u_0, u_1, u_2, arm coin u_3,     m = 3 pi sqrt u_0, d = (-m cos m + .5 u_1, m sin m + .5 u_2),
//                    N(4,5)                           s = u_3 >= .5 ? -1 : 1:  s d / 3 + .1 n
//   9 checkerboard   u_0, u_1, coin u_2               x1 = 4 u_0 - 2, x2 = u_1 - 2 [u_2 >= .5] + (floor x1 mod 2):  2 x1, 2 x2
//                                                     (the parity as [.25 <= u_0 < .5 or u_0 >= .75])
//  10 line           u_0                              x = 5 u_0 - 2.5:  x, x
//  11 line-noisy     u_0, N(1,2)                      x, x + n0
//  12 cos            u_0, N(1,2)                      x = 6 u_0 - 3:  x, 2.5 sin 5x + .3 n0
//  13 joint_gaussian N(0,1)                           x2 = 4 n0:  n1 + x2^2 / 4, x2
//
// Where the reference fixes counts per batch (the arms of 2spirals, the rings, the moons, the five pinwheel classes) the
// device draws a fair coin or class per sample, and circles / moons draw the angle uniformly instead of linspace + shuffle:
// every sample has the law of one reference sample and the batch is i.i.d..
//
// TWO forms, bit-identical: toy_sample_k<true> stores a block's pair as one float2 (x 8-byte aligned, ldx even),
// toy_sample_k<false> as two floats.  logf / sinf / cosf / expf are the library's (about 1 ulp), the division and the square
// root IEEE, contraction off: the kernel is train_toy.toy_reference in fp32, operation by operation.
#include "gnf_common.h"

namespace {

constexpr int kToyBlock = 256;
constexpr int kToyMaxBlocks = 8;
constexpr int kToyKinds = 14;

struct ToyScale { float v[2 * kToyMaxBlocks]; };

struct Pair { float a, b; };

__device__ __forceinline__ Pair box_muller(float ua, float ub) {
#pragma clang fp contract(off)
  const float r = sqrtf(-2.f * logf(ua)), th = 6.283185307179586f * ub;
  return Pair{r * cosf(th), r * sinf(th)};
}

__device__ __forceinline__ Pair toy_draw(int kind, float u0, float u1, float u2, float u3, float u4, float u5) {
#pragma clang fp contract(off)
  Pair o{0.f, 0.f};
  if (kind <= 3) {                                                   // the Gaussian mixtures
    const Pair n = box_muller(u0, u1);
    float cx, cy, std = .75f;
    if (kind == 0) {
      cx = u2 >= .5f ? -2.f : 2.f; cy = 0.f;
    } else if (kind == 1) {
      cx = u2 >= .5f ? -2.f : 2.f; cy = -cx;
    } else if (kind == 2) {
      const int k = (u2 >= .25f) + (u2 >= .5f) + (u2 >= .75f);
      cx = (k & 1) ? -2.f : 2.f;                                     // (2,-2) (-2,2) (2,2) (-2,-2)
      cy = (k == 1 || k == 2) ? 2.f : -2.f;
    } else {
      const int k = (u2 >= .125f) + (u2 >= .25f) + (u2 >= .375f) + (u2 >= .5f) + (u2 >= .625f) + (u2 >= .75f) + (u2 >= .875f);
      const float d = 2.8284271247461903f;                           // 4 / sqrt 2
      cx = k == 0 ? 4.f : k == 1 ? -4.f : k < 4 ? 0.f : k < 6 ? d : -d;
      cy = k < 2 ? 0.f : k == 2 ? 4.f : k == 3 ? -4.f : (k & 1) ? -d : d;
      std = .5f;
    }
    o.a = n.a * std + cx; o.b = n.b * std + cy;
    if (kind == 3) { o.a = o.a / 1.414f; o.b = o.b / 1.414f; }
  } else if (kind == 4) {                                            // swissroll
    const float t = (1.f + 2.f * u0) * 4.71238898038469f;
    const Pair n = box_muller(u1, u2);
    o.a = (t * cosf(t) + n.a) / 5.f; o.b = (t * sinf(t) + n.b) / 5.f;
  } else if (kind == 5) {                                            // circles
    const float f = u0 >= .5f ? .5f : 1.f, a = 6.283185307179586f * u1;
    const Pair n = box_muller(u2, u3);
    o.a = (f * cosf(a) + .08f * n.a) * 3.f; o.b = (f * sinf(a) + .08f * n.b) * 3.f;
  } else if (kind == 6) {                                            // moons
    const float a = 3.141592653589793f * u1, c = cosf(a), s = sinf(a);
    const bool inner = u0 >= .5f;
    const Pair n = box_muller(u2, u3);
    const float mx = inner ? 1.f - c : c, my = inner ? (1.f - s) - .5f : s;
    o.a = (mx + .1f * n.a) * 2.f - 1.f; o.b = (my + .1f * n.b) * 2.f - .2f;
  } else if (kind == 7) {                                            // pinwheel
    const Pair n = box_muller(u0, u1);
    const float f0 = n.a * .3f + 1.f, f1 = n.b * .1f;
    const int k = (u2 >= .2f) + (u2 >= .4f) + (u2 >= .6f) + (u2 >= .8f);
    const float a = (float)k * 1.2566370614359172f + .25f * expf(f0), c = cosf(a), s = sinf(a);
    o.a = 2.f * (f0 * c + f1 * s); o.b = 2.f * (f1 * c - f0 * s);
  } else if (kind == 8) {                                            // 2spirals
    const float m = sqrtf(u0) * 9.42477796076938f, sg = u3 >= .5f ? -1.f : 1.f;
    const float dx = -cosf(m) * m + u1 * .5f, dy = sinf(m) * m + u2 * .5f;
    const Pair n = box_muller(u4, u5);
    o.a = sg * dx / 3.f + .1f * n.a; o.b = sg * dy / 3.f + .1f * n.b;
  } else if (kind == 9) {                                            // checkerboard
    const float x1 = u0 * 4.f - 2.f;
    const float par = ((u0 >= .25f && u0 < .5f) || u0 >= .75f) ? 1.f : 0.f, coin = u2 >= .5f ? 2.f : 0.f;
    o.a = x1 * 2.f; o.b = ((u1 - coin) + par) * 2.f;
  } else if (kind == 10) {                                           // line
    o.a = u0 * 5.f - 2.5f; o.b = o.a;
  } else if (kind == 11) {                                           // line-noisy
    const Pair n = box_muller(u1, u2);
    o.a = u0 * 5.f - 2.5f; o.b = o.a + n.a;
  } else if (kind == 12) {                                           // cos
    const Pair n = box_muller(u1, u2);
    o.a = u0 * 6.f - 3.f; o.b = sinf(o.a * 5.f) * 2.5f + n.a * .3f;
  } else {                                                           // joint_gaussian
    const Pair n = box_muller(u0, u1);
    o.b = 4.f * n.a; o.a = n.b + o.b * o.b / 4.f;
  }
  return o;
}

template <bool VEC>
__global__ __launch_bounds__(kToyBlock) void toy_sample_k(uint32_t kinds, int P, ToyScale scale, int scaled,
                                                          const float* __restrict__ u, uint64_t seed, uint64_t offset,
                                                          float* __restrict__ x, int64_t ldx, int64_t B) {
#pragma clang fp contract(off)
  // wave w of the grid: block p = w % P of the 64 samples 64 (w / P) ..., so p and the kind are scalars
  const int64_t w = (int64_t)blockIdx.x * (kToyBlock / GNF_WAVE) + __builtin_amdgcn_readfirstlane(threadIdx.x / GNF_WAVE);
  const int64_t chunk = w / P;
  const int p = (int)(w - chunk * P);
  const int64_t b = chunk * GNF_WAVE + (threadIdx.x & (GNF_WAVE - 1));
  if (b >= B) return;                                                // the last chunk's tail, and the waves past the last chunk
  const int64_t t = b * P + p;
  const int kind = (int)((kinds >> (4 * p)) & 15u);
  float u0, u1, u2, u3, u4 = .5f, u5 = .5f;
  if (u) {
    const f32x4u q0 = *reinterpret_cast<const f32x4u*>(u + 8 * t);
    u0 = q0[0]; u1 = q0[1]; u2 = q0[2]; u3 = q0[3];
    if (kind == 8) {
      const f32x2u q1 = *reinterpret_cast<const f32x2u*>(u + 8 * t + 4);
      u4 = q1[0]; u5 = q1[1];
    }
  } else {
    uint32_t r[4];
    philox4x32_10((uint32_t)b, (uint32_t)p << 8, (uint32_t)offset, (uint32_t)(offset >> 32), (uint32_t)seed,
                  (uint32_t)(seed >> 32), r);
    u0 = u01_open(r[0]); u1 = u01_open(r[1]); u2 = u01_open(r[2]); u3 = u01_open(r[3]);
    if (kind == 8) {
      philox4x32_10((uint32_t)b, ((uint32_t)p << 8) | 1u, (uint32_t)offset, (uint32_t)(offset >> 32), (uint32_t)seed,
                    (uint32_t)(seed >> 32), r);
      u4 = u01_open(r[0]); u5 = u01_open(r[1]);
    }
  }
  Pair o = toy_draw(kind, u0, u1, u2, u3, u4, u5);
  if (scaled) { o.a *= scale.v[2 * p]; o.b *= scale.v[2 * p + 1]; }
  float* dst = x + b * ldx + 2 * p;
  if (VEC) {
    *reinterpret_cast<float2*>(dst) = make_float2(o.a, o.b);
  } else {
    dst[0] = o.a; dst[1] = o.b;
  }
}

inline bool aligned_to(const void* p, uintptr_t a) { return (reinterpret_cast<uintptr_t>(p) & (a - 1)) == 0; }

}  // namespace

extern "C" int gnf_toy_sample(const int32_t* kinds, int P, const float* col_scale, const float* u, uint64_t seed,
                              uint64_t offset, float* x, int64_t ldx, int64_t B, gnf_stream_t stream) {
  if (P < 1 || P > kToyMaxBlocks || !kinds || B < 0 || B > ((int64_t)1 << 32) || ldx < 2 * (int64_t)P) return GNF_EINVAL;
  uint32_t packed = 0;
  ToyScale scale;
  for (int p = 0; p < kToyMaxBlocks; ++p) {
    if (p < P) {
      if (kinds[p] < 0 || kinds[p] >= kToyKinds) return GNF_EINVAL;
      packed |= (uint32_t)kinds[p] << (4 * p);
    }
    scale.v[2 * p] = col_scale && p < P ? col_scale[2 * p] : 1.f;
    scale.v[2 * p + 1] = col_scale && p < P ? col_scale[2 * p + 1] : 1.f;
  }
  if (B == 0) return 0;
  if (!x || !aligned_to(x, 4) || !aligned_to(u, 4)) return GNF_EINVAL;
  constexpr int kWaves = kToyBlock / GNF_WAVE;
  const int64_t waves = (B + GNF_WAVE - 1) / GNF_WAVE * P;                     // <= 2^29
  const unsigned grid = (unsigned)((waves + kWaves - 1) / kWaves);
  hipStream_t s = static_cast<hipStream_t>(stream);
  if (aligned_to(x, 8) && ldx % 2 == 0)
    hipLaunchKernelGGL(toy_sample_k<true>, dim3(grid), dim3(kToyBlock), 0, s, packed, P, scale, col_scale ? 1 : 0, u, seed,
                       offset, x, ldx, B);
  else
    hipLaunchKernelGGL(toy_sample_k<false>, dim3(grid), dim3(kToyBlock), 0, s, packed, P, scale, col_scale ? 1 : 0, u, seed,
                       offset, x, ldx, B);
  GNF_LAUNCH_CHECK();
  return 0;
}
