// A bias per GROUP of G consecutive rows, behind the first layer of a DAGMLP that takes a context: the d masked copies of a
// sample share one context row, so the context half of the layer is one [B, cond_in] x [cond_in, H] product whose result cb
// enters the [B*d, H] pre-activation as a bias per sample (G = d).
//
//   fwd:  out[r, n]  = act(y[r, n] + cb[r / G, n])                     act = ReLU or the identity
//   bwd:  g_pre[r, n] = g[r, n] * [a[r, n] > 0]   (a = the saved forward output; NULL for the identity: g_pre = g)
//         g_cb[b, n]  = sum_{i < G} g_pre[b G + i, n]                   fp32, ascending i
//
// Both are HBM-streaming (fwd: 4 B read + 4 B written per element and the L2-resident cb; bwd: 8 read + 4 written), no LDS, no
// workspace, no atomics.  A thread owns four consecutive columns (one column in the dword form):
//   fwd  one (row, column quad) unit per thread, grid-strided over the M * H / 4 units;
//   bwd  one (sample, column quad) unit per thread: it walks the G rows of its sample IN ORDER, so every element of g_pre and
//        of g_cb has exactly one writer and the sum is the plain ascending chain whatever the grid -- two calls, or another
//        deal of the units to wavefronts, give the same bits.  The chain of adds is short (G <= a few dozen) and cheap; what
//        would serialise is the LOADS, so a thread requests kRowsAhead rows (g and a: 16 independent 16-byte loads) before it
//        consumes the first: G = 63 is 8 rounds of latency, not 63.  Neighbouring lanes hold neighbouring quads of the same
//        row, so every wave-instruction is a contiguous row segment.  B * H / 4 threads: 2 500 at B = 100, H = 100.
//
// TWO forms, bit-identical (each output element is one add and one select, or the same chain of adds, in both): 16-byte
// accesses when H % 4 == 0 and every array is 16-byte aligned, single dwords at any dword address and any H otherwise.
#include "gnf_common.h"

namespace {

constexpr int kGbBlock = 256;
constexpr int kGbMaxGrid = 2048;          // 8 workgroups per CU; the rest of the units by grid stride
constexpr int kRowsAhead = 8;

template <int V> struct Pack;
template <> struct Pack<4> { typedef f32x4 T; };
template <> struct Pack<1> { typedef float T; };

template <int V> __device__ __forceinline__ typename Pack<V>::T gb_load(const float* p) {
  return *reinterpret_cast<const typename Pack<V>::T*>(p);
}
template <int V> __device__ __forceinline__ void gb_store(float* p, typename Pack<V>::T v) {
  *reinterpret_cast<typename Pack<V>::T*>(p) = v;
}
__device__ __forceinline__ float gb_lane(float v, int) { return v; }
__device__ __forceinline__ float gb_lane(const f32x4& v, int k) { return v[k]; }
__device__ __forceinline__ void gb_set(float& v, int, float s) { v = s; }
__device__ __forceinline__ void gb_set(f32x4& v, int k, float s) { v[k] = s; }

// y and out may be the same array: a thread reads its unit before it writes it, and nobody else touches that unit
template <int V>
__global__ __launch_bounds__(kGbBlock) void group_bias_fwd_k(const float* y, const float* __restrict__ cb, float* out,
                                                             int64_t M, int64_t H, int64_t G, int relu) {
  typedef typename Pack<V>::T T;
  const int64_t hq = H / V, units = M * hq;
  for (int64_t u = (int64_t)blockIdx.x * kGbBlock + threadIdx.x; u < units; u += (int64_t)gridDim.x * kGbBlock) {
    const int64_t r = u / hq, n = (u - r * hq) * V;
    const T a = gb_load<V>(y + r * H + n), c = gb_load<V>(cb + (r / G) * H + n);
    T o;
#pragma unroll
    for (int k = 0; k < V; ++k) {
      const float s = gb_lane(a, k) + gb_lane(c, k);
      gb_set(o, k, (relu && s < 0.f) ? 0.f : s);           // a NaN stays a NaN
    }
    gb_store<V>(out + r * H + n, o);
  }
}

// g and g_pre may be the same array (as above); g_pre may be NULL when a is (g_pre would be g itself)
template <int V>
__global__ __launch_bounds__(kGbBlock) void group_bias_bwd_k(const float* g, const float* __restrict__ a, float* g_pre,
                                                             float* __restrict__ g_cb, int64_t B, int64_t H, int64_t G) {
  typedef typename Pack<V>::T T;
  const int64_t hq = H / V, units = B * hq;
  for (int64_t u = (int64_t)blockIdx.x * kGbBlock + threadIdx.x; u < units; u += (int64_t)gridDim.x * kGbBlock) {
    const int64_t b = u / hq, n = (u - b * hq) * V;
    const int64_t base = b * G * H + n;
    T acc;
#pragma unroll
    for (int k = 0; k < V; ++k) gb_set(acc, k, 0.f);
    for (int64_t i0 = 0; i0 < G; i0 += kRowsAhead) {
      T gv[kRowsAhead], av[kRowsAhead];
#pragma unroll
      for (int j = 0; j < kRowsAhead; ++j) {                 // every load of the round before the first use
        if (i0 + j < G) {
          gv[j] = gb_load<V>(g + base + (i0 + j) * H);
          if (a) av[j] = gb_load<V>(a + base + (i0 + j) * H);
        }
      }
#pragma unroll
      for (int j = 0; j < kRowsAhead; ++j) {                 // consumed in ascending i
        if (i0 + j < G) {
          T p = gv[j];
          if (a) {
#pragma unroll
            for (int k = 0; k < V; ++k) gb_set(p, k, gb_lane(av[j], k) > 0.f ? gb_lane(gv[j], k) : 0.f);
          }
          if (g_pre) gb_store<V>(g_pre + base + (i0 + j) * H, p);
#pragma unroll
          for (int k = 0; k < V; ++k) gb_set(acc, k, gb_lane(acc, k) + gb_lane(p, k));
        }
      }
    }
    gb_store<V>(g_cb + b * H + n, acc);
  }
}

inline bool aligned_to(const void* p, uintptr_t a) { return (reinterpret_cast<uintptr_t>(p) & (a - 1)) == 0; }

inline unsigned gb_grid(int64_t units) {
  const int64_t blocks = (units + kGbBlock - 1) / kGbBlock;
  return (unsigned)(blocks < kGbMaxGrid ? blocks : kGbMaxGrid);
}

}  // namespace

extern "C" int gnf_group_bias_fwd(const float* y, const float* cb, float* out, int relu, int64_t M, int64_t H, int64_t G,
                                  gnf_stream_t stream) {
  if (M < 0 || H < 1 || G < 1) return GNF_EINVAL;
  if (M % G != 0) return GNF_ESHAPE;
  if (M == 0) return 0;
  if (!y || !cb || !out) return GNF_EINVAL;
  if (!aligned_to(y, 4) || !aligned_to(cb, 4) || !aligned_to(out, 4)) return GNF_EINVAL;
  if (M > INT64_MAX / H) return GNF_ESHAPE;
  hipStream_t s = static_cast<hipStream_t>(stream);
  if (H % 4 == 0 && aligned_to(y, 16) && aligned_to(cb, 16) && aligned_to(out, 16))
    hipLaunchKernelGGL(group_bias_fwd_k<4>, dim3(gb_grid(M * (H / 4))), dim3(kGbBlock), 0, s, y, cb, out, M, H, G, relu);
  else
    hipLaunchKernelGGL(group_bias_fwd_k<1>, dim3(gb_grid(M * H)), dim3(kGbBlock), 0, s, y, cb, out, M, H, G, relu);
  GNF_LAUNCH_CHECK();
  return 0;
}

extern "C" int gnf_group_bias_bwd(const float* g, const float* a, float* g_pre, float* g_cb, int64_t M, int64_t H, int64_t G,
                                  gnf_stream_t stream) {
  if (M < 0 || H < 1 || G < 1) return GNF_EINVAL;
  if (M % G != 0) return GNF_ESHAPE;
  if (M == 0) return 0;
  if (!g || !g_cb || (a && !g_pre)) return GNF_EINVAL;
  if (!aligned_to(g, 4) || !aligned_to(a, 4) || !aligned_to(g_pre, 4) || !aligned_to(g_cb, 4)) return GNF_EINVAL;
  if (M > INT64_MAX / H) return GNF_ESHAPE;
  const int64_t B = M / G;
  hipStream_t s = static_cast<hipStream_t>(stream);
  if (H % 4 == 0 && aligned_to(g, 16) && aligned_to(a, 16) && aligned_to(g_pre, 16) && aligned_to(g_cb, 16))
    hipLaunchKernelGGL(group_bias_bwd_k<4>, dim3(gb_grid(B * (H / 4))), dim3(kGbBlock), 0, s, g, a, g_pre, g_cb, B, H, G);
  else
    hipLaunchKernelGGL(group_bias_bwd_k<1>, dim3(gb_grid(B * H)), dim3(kGbBlock), 0, s, g, a, g_pre, g_cb, B, H, G);
  GNF_LAUNCH_CHECK();
  return 0;
}
