// Rational-quadratic spline normalizer (gnf_spline.h holds the law): forward with the two row reductions fused, backward
// that recomputes the forward, inverse in the plain and the variable-major scatter form.  HBM-bound streaming kernels: an
// element reads its 3K-1 conditioner outputs once and writes 1-2 floats (forward) or 3K floats (backward).
//
// A workgroup of kTile lanes owns kTile consecutive elements e = b d + i, one per lane.  Their conditioner outputs are
// staged through LDS as rows of an ODD pitch (lane t reads row t: conflict-free), because a lane-per-element load of the
// contiguous [B, d, C] layout strides 4 C bytes:
//   h_sc = 1, h_sb = d h_sd (DAG / Coupling): the tile's outputs are ONE contiguous span of n h_sd floats, loaded with
//     consecutive lanes on consecutive addresses -- 16-byte loads when the span starts on a 16-byte address, dwords else;
//   any other strides (MADE's permuted view, h_sd = 1, h_sc = d): lane t loads its own row, component by component; lanes
//     along i are then coalesced per component.
// The backward sends the gradient rows back the same way.  The forward's tiles are whole rows of the batch (kTile / d of
// them, or a row in chunks of kTile columns when d > kTile), so that log|det J| and the Normal log-density of a row are
// reduced inside the workgroup in a fixed order: no atomics, deterministic.
#include <stdio.h>
#include "gnf_spline.h"

namespace {

constexpr int kTile = 128;
constexpr double kLog2Pi = 1.8378770664093453;

__host__ __device__ inline int round_up4(int v) { return (v + 3) & ~3; }

// sum over an aligned group of eight lanes (fp64: two dword shuffles per step)
__device__ __forceinline__ double group_sum8(double v) {
#pragma unroll
  for (int off = 4; off > 0; off >>= 1) v += __shfl_xor(v, off, GNF_WAVE);
  return v;
}

// floats per staged row: the WIDE layout of gnf_spline.h (a double over each of the 2K softmax logits), made odd
__host__ __device__ inline int spl_pitch(int K) { return spl_row_floats<true>(K) | 1; }

struct HLay {                               // h[b, i, c] at b sb + i sd + c sc
  int64_t sb, sd, sc;
  int flat;                                 // 1: sc = 1 and sb = d sd, the span form; 2: ... on a 16-byte address grid
};

inline HLay make_lay(const float* p, int64_t sb, int64_t sd, int64_t sc, int64_t d, int C) {
  HLay l{sb, sd, sc, 0};
  if (sc == 1 && sd >= C && sd <= 4096 && sb == d * sd) {
    // a tile whose span starts on a 16-byte address (decided per tile) moves it in 16-byte pieces
    l.flat = ((uintptr_t)p & 15) == 0 ? 2 : 1;
  }
  return l;
}

// rows[t][0 .. C) <- h of element e0 + t, t < n.  Ends in a barrier.
__device__ __forceinline__ void stage_in(const float* __restrict__ h, const HLay& l, int64_t e0, int n, int64_t d, int K,
                                         float* rows) {
  const int tid = threadIdx.x, pitch = spl_pitch(K), C = 3 * K - 1;
  if (l.flat) {
    const int sd = (int)l.sd, total = n * sd;
    const float* src = h + e0 * l.sd;
    if (l.flat == 2 && (e0 * l.sd) % 4 == 0) {
      int el = 4 * tid / sd, c = 4 * tid % sd;
      const int de = 4 * kTile / sd, dc = 4 * kTile % sd, tq = total & ~3;
      if (tid < total - tq) {                                          // the span's last 1-3 floats
        const int idx = tq + tid, ee = idx / sd, cc = idx - ee * sd;
        if (cc < C) rows[ee * pitch + spl_pos<true>(cc, K)] = src[idx];
      }
#pragma unroll 2
      for (int idx = 4 * tid; idx < tq; idx += 4 * kTile) {
        const f32x4 v = *reinterpret_cast<const f32x4*>(src + idx);
        int ee = el, cc = c;
#pragma unroll
        for (int u = 0; u < 4; ++u) {
          if (cc < C) rows[ee * pitch + spl_pos<true>(cc, K)] = v[u];
          if (++cc == sd) { cc = 0; ++ee; }
        }
        el += de; c += dc;
        if (c >= sd) { c -= sd; ++el; }
      }
    } else {
      int el = tid / sd, c = tid % sd;
      const int de = kTile / sd, dc = kTile % sd;
#pragma unroll 4
      for (int idx = tid; idx < total; idx += kTile) {
        if (c < C) rows[el * pitch + spl_pos<true>(c, K)] = src[idx];
        el += de; c += dc;
        if (c >= sd) { c -= sd; ++el; }
      }
    }
  } else if (tid < n) {
    const int64_t e = e0 + tid, b = e / d, i = e - b * d;
    const float* src = h + b * l.sb + i * l.sd;
    float* r = rows + tid * pitch;
#pragma unroll 4
    for (int c = 0; c < C; ++c) r[spl_pos<true>(c, K)] = src[c * l.sc];
  }
  __syncthreads();
}

// the reverse route for the gradient rows (components >= C of gh are the caller's).  Begins with a barrier.
__device__ __forceinline__ void stage_out(float* __restrict__ gh, const HLay& l, int64_t e0, int n, int64_t d, int K,
                                          const float* rows) {
  const int tid = threadIdx.x, pitch = spl_pitch(K), C = 3 * K - 1;
  __syncthreads();
  if (l.flat) {
    const int sd = (int)l.sd, total = n * sd;
    float* dst = gh + e0 * l.sd;
    if (l.flat == 2 && sd == C && (e0 * l.sd) % 4 == 0) {
      int el = 4 * tid / sd, c = 4 * tid % sd;
      const int de = 4 * kTile / sd, dc = 4 * kTile % sd, tq = total & ~3;
      if (tid < total - tq) {
        const int idx = tq + tid, ee = idx / sd;
        dst[idx] = rows[ee * pitch + spl_pos<true>(idx - ee * sd, K)];
      }
      for (int idx = 4 * tid; idx < tq; idx += 4 * kTile) {
        f32x4 v;
        int ee = el, cc = c;
#pragma unroll
        for (int u = 0; u < 4; ++u) {
          v[u] = rows[ee * pitch + spl_pos<true>(cc, K)];
          if (++cc == sd) { cc = 0; ++ee; }
        }
        *reinterpret_cast<f32x4*>(dst + idx) = v;
        el += de; c += dc;
        if (c >= sd) { c -= sd; ++el; }
      }
    } else {
      int el = tid / sd, c = tid % sd;
      const int de = kTile / sd, dc = kTile % sd;
#pragma unroll 4
      for (int idx = tid; idx < total; idx += kTile) {
        if (c < C) dst[idx] = rows[el * pitch + spl_pos<true>(c, K)];
        el += de; c += dc;
        if (c >= sd) { c -= sd; ++el; }
      }
    }
  } else if (tid < n) {
    const int64_t e = e0 + tid, b = e / d, i = e - b * d;
    float* dst = gh + b * l.sb + i * l.sd;
    const float* r = rows + tid * pitch;
#pragma unroll 4
    for (int c = 0; c < C; ++c) dst[c * l.sc] = r[spl_pos<true>(c, K)];
  }
}

// RT = max(1, kTile / d) whole rows per workgroup; a row longer than kTile goes through in chunks
__global__ __launch_bounds__(kTile) void spline_fwd_k(const float* __restrict__ x, const float* __restrict__ h, HLay l, int K,
                                                      double T, float* __restrict__ z, float* __restrict__ jac,
                                                      float* __restrict__ logdet, float* __restrict__ logn, int64_t B,
                                                      int64_t d, int RT) {
  extern __shared__ __attribute__((aligned(16))) float smem[];
  const int pitch = spl_pitch(K), tid = threadIdx.x;
  float* rows = smem;
  double* red = reinterpret_cast<double*>(smem + round_up4(kTile * pitch));   // [2][kTile], 16-byte aligned
  const int64_t row0 = (int64_t)blockIdx.x * RT;
  const int nr = (int)(B - row0 < RT ? B - row0 : RT);
  const int nchunk = RT == 1 ? (int)((d + kTile - 1) / kTile) : 1;
  double lj = 0., lq = 0.;
  for (int ch = 0; ch < nchunk; ++ch) {
    const int64_t e0 = row0 * d + (int64_t)ch * kTile;
    const int n = RT == 1 ? (int)(d - (int64_t)ch * kTile < kTile ? d - (int64_t)ch * kTile : kTile) : nr * (int)d;
    stage_in(h, l, e0, n, d, K, rows);
    if (tid < n) {
      double zv, jv;
      spl_forward(rows + tid * pitch, K, T, x[e0 + tid], zv, jv);
      z[e0 + tid] = (float)zv;
      if (jac) jac[e0 + tid] = (float)jv;
      if (logdet) lj += log(jv);
      lq += kLog2Pi + zv * zv;
    }
    if (ch + 1 < nchunk) __syncthreads();                              // the next chunk's staging overwrites the rows
  }
  if (!logdet && !logn) return;
  red[tid] = lj;
  red[kTile + tid] = lq;
  __syncthreads();
  // eight lanes per row, then a butterfly inside the aligned group of eight
  const int seg = RT == 1 ? kTile : (int)d;
  for (int t0 = 0; t0 < nr * 8; t0 += kTile) {
    const int t = t0 + tid, r = t >> 3, g = t & 7;
    double a = 0., b = 0.;
    if (r < nr)
      for (int i = g; i < seg; i += 8) { a += red[r * seg + i]; b += red[kTile + r * seg + i]; }
    a = group_sum8(a);
    b = group_sum8(b);
    if (r < nr && g == 0) {
      if (logdet) logdet[row0 + r] = (float)a;
      if (logn) logn[row0 + r] = (float)(-0.5 * b);
    }
  }
}

__global__ __launch_bounds__(kTile) void spline_bwd_k(const float* __restrict__ x, const float* __restrict__ h, HLay l, int K,
                                                      double T, const float* __restrict__ gz, const float* __restrict__ gjac,
                                                      const float* __restrict__ glogdet, const float* __restrict__ glogn,
                                                      float* __restrict__ gx, float* __restrict__ gh, HLay gl, int64_t N,
                                                      int64_t d) {
  extern __shared__ __attribute__((aligned(16))) float smem[];
  const int pitch = spl_pitch(K), tid = threadIdx.x;
  const int64_t e0 = (int64_t)blockIdx.x * kTile;
  const int n = (int)(N - e0 < kTile ? N - e0 : kTile);
  // the cotangents are asked for before the staging, which hides their latency
  float xv = 0.f, a = 0.f, bj = 0.f, cl = 0.f, cn = 0.f;
  if (tid < n) {
    const int64_t e = e0 + tid, b = e / d;
    xv = x[e];
    if (gz) a = gz[e];
    if (gjac) bj = gjac[e];
    if (glogdet) cl = glogdet[b];
    if (glogn) cn = glogn[b];
  }
  stage_in(h, l, e0, n, d, K, smem);
  if (tid < n) {
    const float g = spl_backward(smem + tid * pitch, K, T, xv, a, bj, cl, cn);
    if (gx) gx[e0 + tid] = g;
  }
  stage_out(gh, gl, e0, n, d, K, smem);
}

// element (b, i) of the [B, d] problem -> x[b d + i], or out[i width + cols[b]] (the variable-major form: b a variable)
__global__ __launch_bounds__(kTile) void spline_inv_k(const float* __restrict__ z, const float* __restrict__ h, HLay l, int K,
                                                      double T, float* __restrict__ x, const int32_t* __restrict__ cols,
                                                      int64_t width, int64_t N, int64_t d) {
  extern __shared__ __attribute__((aligned(16))) float smem[];
  const int pitch = spl_pitch(K), tid = threadIdx.x;
  const int64_t e0 = (int64_t)blockIdx.x * kTile;
  const int n = (int)(N - e0 < kTile ? N - e0 : kTile);
  const float zv = tid < n ? z[e0 + tid] : 0.f;
  stage_in(h, l, e0, n, d, K, smem);
  if (tid < n) {
    const float xv = spl_inverse<true>(smem + tid * pitch, K, T, zv);
    if (cols) {
      const int64_t e = e0 + tid, b = e / d, i = e - b * d;
      x[i * width + cols[b]] = xv;
    } else {
      x[e0 + tid] = xv;
    }
  }
}

size_t lds_bytes(int K, bool red) { return 4 * (size_t)round_up4(kTile * spl_pitch(K)) + (red ? 16 * kTile : 0); }

// ---- the host's decisions, made ONCE: the three entry points launch from a SplPlan and gnf_spline_route prints one ----
enum { kSplFwd = 0, kSplBwd = 1, kSplInv = 2 };

struct SplPlan {
  int RT, nchunk;                           // forward: whole rows per workgroup, chunks of a row; 0 and 1 for the element tiles
  int64_t grid, tiles16, gtiles16;          // workgroups (0: an empty batch); staged tiles on the 16-byte path, of h and of gh
  size_t lds;
  HLay l, gl;                               // gl: the backward's gh
  bool g16;                                 // gh is as wide as the rows: stage_out may take the 16-byte path
};

// tiles i < count starting at element i step: how many have (e0 sd) % 4 == 0 (the condition of stage_in / stage_out)
int64_t tiles_on_16(int64_t count, int64_t step, int64_t sd) {
  int64_t n = 0;
  for (int r = 0; r < 4 && r < count; ++r)
    if ((r * (step & 3) * (sd & 3)) % 4 == 0) n += (count - r + 3) / 4;
  return n;
}

// the checks the entry points share (T apart, which the query is not given), in their order, then the launch's numbers.
// others_ok: the entry point's remaining arguments, which it needs only where something is launched
int spline_plan(int which, const void* h, int64_t h_sb, int64_t h_sd, int64_t h_sc, int64_t h_c, int K, int64_t B, int64_t d,
                const void* gh, int64_t g_sb, int64_t g_sd, int64_t g_sc, bool others_ok, SplPlan& p) {
  p = SplPlan{};
  if (K < kSplMinBins || K > kSplMaxBins) return GNF_EINVAL;
  if (B < 0 || d <= 0) return GNF_EINVAL;
  if (h_c < 3 * K - 1) return GNF_ESHAPE;
  if (B == 0) return 0;
  if (!h || (which == kSplBwd && !gh) || !others_ok) return GNF_EINVAL;
  const int C = 3 * K - 1;
  if (which == kSplFwd) {
    p.RT = d >= kTile ? 1 : (int)(kTile / d);
    p.nchunk = p.RT == 1 ? (int)((d + kTile - 1) / kTile) : 1;
    p.grid = (B + p.RT - 1) / p.RT;
  } else {
    if (B > INT64_MAX / d) return GNF_ESHAPE;
    p.RT = 0;
    p.nchunk = 1;
    p.grid = (B * d + kTile - 1) / kTile;
  }
  if (p.grid > 0x7fffffff) return GNF_ESHAPE;
  p.lds = lds_bytes(K, which == kSplFwd);
  p.l = make_lay((const float*)h, h_sb, h_sd, h_sc, d, C);
  // a chunk of a row starts a multiple of kTile past the row, which leaves (e0 sd) % 4 alone
  const int64_t step = which == kSplFwd ? p.RT * d : kTile;
  if (p.l.flat == 2) p.tiles16 = tiles_on_16(p.grid, step, h_sd) * p.nchunk;
  if (which == kSplBwd) {
    p.gl = make_lay((const float*)gh, g_sb, g_sd, g_sc, d, C);
    p.g16 = g_sd == C;
    if (p.gl.flat == 2 && p.g16) p.gtiles16 = tiles_on_16(p.grid, step, g_sd);
  }
  return 0;
}

bool bad_tail(double T) { return !(T > 0.) || !(T < 3.0e38); }

const char* lay_name(const HLay& l, bool can16) { return l.flat == 2 && can16 ? "span16" : l.flat ? "span4" : "rows"; }

}  // namespace

extern "C" {

int gnf_spline_fwd(const float* x, const float* h, int64_t h_sb, int64_t h_sd, int64_t h_sc, int64_t h_c, int K, double T,
                   float* z, float* jac, float* logdet, float* logn, int64_t B, int64_t d, gnf_stream_t stream) {
  if (bad_tail(T)) return GNF_EINVAL;
  SplPlan p;
  if (const int rc = spline_plan(kSplFwd, h, h_sb, h_sd, h_sc, h_c, K, B, d, nullptr, 0, 0, 0, x && z, p)) return rc;
  if (B == 0) return 0;
  const hipError_t e = gnf_launch_lds(spline_fwd_k, dim3((unsigned)p.grid), dim3(kTile), p.lds, (hipStream_t)stream,
                                      x, h, p.l, K, T, z, jac, logdet, logn, B, d, p.RT);
  return e == hipSuccess ? 0 : (int)e;
}

int gnf_spline_bwd(const float* x, const float* h, int64_t h_sb, int64_t h_sd, int64_t h_sc, int64_t h_c, int K, double T,
                   const float* gz, const float* gjac, const float* glogdet, const float* glogn, float* gx, float* gh,
                   int64_t g_sb, int64_t g_sd, int64_t g_sc, int64_t B, int64_t d, gnf_stream_t stream) {
  if (bad_tail(T)) return GNF_EINVAL;
  SplPlan p;
  if (const int rc = spline_plan(kSplBwd, h, h_sb, h_sd, h_sc, h_c, K, B, d, gh, g_sb, g_sd, g_sc, x != nullptr, p)) return rc;
  if (B == 0) return 0;
  const hipError_t e = gnf_launch_lds(spline_bwd_k, dim3((unsigned)p.grid), dim3(kTile), p.lds, (hipStream_t)stream,
                                      x, h, p.l, K, T, gz, gjac, glogdet, glogn, gx, gh, p.gl, B * d, d);
  return e == hipSuccess ? 0 : (int)e;
}

int gnf_spline_inv(const float* z, const float* h, int64_t h_sb, int64_t h_sd, int64_t h_sc, int64_t h_c, int K, double T,
                   float* x, const int32_t* out_cols, int64_t out_width, int64_t B, int64_t d, gnf_stream_t stream) {
  if (bad_tail(T)) return GNF_EINVAL;
  const bool no_width = out_cols && out_width <= 0;
  SplPlan p;
  if (const int rc = spline_plan(kSplInv, h, h_sb, h_sd, h_sc, h_c, K, B, d, nullptr, 0, 0, 0, z && x && !no_width, p))
    return rc;
  if (no_width) return GNF_EINVAL;                                      // refused for an empty batch too
  if (B == 0) return 0;
  const hipError_t e = gnf_launch_lds(spline_inv_k, dim3((unsigned)p.grid), dim3(kTile), p.lds, (hipStream_t)stream,
                                      z, h, p.l, K, T, x, out_cols, out_width, B * d, d);
  return e == hipSuccess ? 0 : (int)e;
}

int gnf_spline_route(int which, const void* h, int64_t h_sb, int64_t h_sd, int64_t h_sc, int64_t h_c, int K, int64_t B,
                     int64_t d, const void* gh, int64_t g_sb, int64_t g_sd, int64_t g_sc, int scatter, char* buf, int len) {
  if (which < kSplFwd || which > kSplInv || !buf || len < 1) return GNF_EINVAL;
  SplPlan p;
  if (const int rc = spline_plan(which, h, h_sb, h_sd, h_sc, h_c, K, B, d, gh, g_sb, g_sd, g_sc, true, p)) return rc;
  buf[0] = 0;
  if (p.grid == 0) return 0;                                            // an empty batch launches nothing
  static const char* const kName[] = {"spline_fwd_k", "spline_bwd_k", "spline_inv_k"};
  int o = snprintf(buf, len, "%s rows_per_wg=%d chunks=%d grid=%lld lds=%zu h=%s tiles16=%lld", kName[which], p.RT, p.nchunk,
                   (long long)p.grid, p.lds, lay_name(p.l, true), (long long)p.tiles16);
  if (which == kSplBwd && o >= 0 && o < len)
    o += snprintf(buf + o, len - o, " gh=%s gtiles16=%lld", lay_name(p.gl, p.g16), (long long)p.gtiles16);
  if (which == kSplInv && o >= 0 && o < len) o += snprintf(buf + o, len - o, " out=%s", scatter ? "cols" : "plain");
  if (o < 0 || o >= len) { buf[0] = 0; return GNF_EINVAL; }
  return 0;
}

}  // extern "C"
