// What the two MADE kernels share (gnf_made_prefix.hip: the forward column sweep of an inversion; gnf_made_adjoint.hip: the
// transposed sweep of its adjoint): the layout host and device agree on, the degree-ordered weight image, and the inner
// product of one (layer, step) -- layer_step over a prefix, suffix_step over a suffix of a transposed image.  The two StrADE
// kernels (gnf_strade.h) run the same steps on level tables.  Everything sits in an anonymous namespace, as the kernels of
// every unit do.
#pragma once
#include "gnf_common.h"

namespace {

constexpr int kThreads = 256;
constexpr int kMaxH = GNF_MADE_MAX_HIDDEN;
constexpr int kLdsBytes = 160 * 1024;
constexpr int kRedFloats = 4 * 256;          // the four wavefronts' partial 16 x 16 tiles

__host__ __device__ inline int round_up(int v, int m) { return (v + m - 1) / m * m; }

// what host and device agree on: the activation row and the packed parameter image
struct MadeLayout {
  int nh, d, out;
  int c;                        // context columns (input degree -1) in front of the variables
  int A;                        // floats per activation row: [context | x in degree order | hidden layer 0 | ... ], made odd
  int width[kMaxH];
  int act_off[kMaxH];           // first column of hidden layer l in the activation row (context and inputs start at 0)
  int K[kMaxH + 1];             // in_features of layer l (l = nh: the output layer)
  int ldw[kMaxH + 1];           // K rounded up to 16: row pitch of the packed weights, the tail zero-filled
  int rows[kMaxH + 1];          // out_features
  int64_t w_off[kMaxH + 1];     // float offsets into the pack
  int64_t b_off[kMaxH + 1];
  int64_t pack_floats;
};

inline int make_layout(const gnf_made_net* net, int cond_in, MadeLayout* lay) {
  if (!net || net->nh < 0 || net->nh > kMaxH || net->d <= 0 || net->out <= 0 || cond_in < 0) return GNF_EINVAL;
  if (cond_in > (1 << 26)) return GNF_ESHAPE;          // the kernel indexes a tile's context, up to 16 * cond_in floats, with an int
  lay->nh = net->nh; lay->d = net->d; lay->out = net->out; lay->c = cond_in;
  const int64_t A0 = (int64_t)cond_in + net->d;
  if (A0 > (1 << 30)) return GNF_ESHAPE;
  int64_t A = A0, off = 0;
  for (int l = 0; l <= net->nh; ++l) {
    if (l < net->nh) {
      if (net->width[l] <= 0) return GNF_EINVAL;
      lay->width[l] = net->width[l];
      lay->act_off[l] = (int)A;
      A += net->width[l];
    }
    lay->K[l] = l == 0 ? (int)A0 : net->width[l - 1];
    lay->rows[l] = l < net->nh ? net->width[l] : net->d * net->out;
    if ((int64_t)net->d * net->out > (1 << 30) || A > (1 << 30)) return GNF_ESHAPE;
    lay->ldw[l] = round_up(lay->K[l], 16);
    lay->w_off[l] = off;
    off += (int64_t)lay->rows[l] * lay->ldw[l];
    lay->b_off[l] = off;
    off += round_up(lay->rows[l], 4);
  }
  lay->A = (int)A | 1;          // an odd pitch spreads the 16 rows of an MFMA operand read over the LDS banks
  lay->pack_floats = off;
  return 0;
}

// ------------------------------------------------------------------------------------------------ the weight image
struct PackArgs {
  MadeLayout lay;
  const float* W[kMaxH + 1];
  const float* b[kMaxH + 1];
  const int32_t* order[kMaxH];
  const int32_t* var_of_step;
};

// the parameter row that row r of layer l of the image holds: hidden unit order_l[r]; output row t * out + c is output
// neuron c * d + var_of_step[t]
__device__ __forceinline__ int pack_src_row(const PackArgs& a, int l, int r) {
  const MadeLayout& L = a.lay;
  return l < L.nh ? a.order[l][r] : (r % L.out) * L.d + a.var_of_step[r / L.out];
}

// ... and the parameter column of its column k: the first layer's columns are [context | variables] (column k < c is
// column k, column c + j is column c + var_of_step[j]), a later layer's are the units below in degree order
__device__ __forceinline__ int pack_src_col(const PackArgs& a, int l, int k) {
  const MadeLayout& L = a.lay;
  return l > 0 ? a.order[l - 1][k] : k < L.c ? k : L.c + a.var_of_step[k - L.c];
}

// element e of the image: hidden layer l: Wp[u'][k'] = W[order_l[u']][order_{l-1}[k']], columns K .. ldw-1 zeros, then the
// layer's biases in the same row order
__device__ __forceinline__ float pack_elem(const PackArgs& a, int64_t e) {
  const MadeLayout& L = a.lay;
  int l = 0;
  while (l < L.nh && e >= L.w_off[l + 1]) ++l;
  float v = 0.f;
  if (e < L.b_off[l]) {
    const int64_t i = e - L.w_off[l];
    const int r = (int)(i / L.ldw[l]), k = (int)(i - (int64_t)r * L.ldw[l]);
    if (k < L.K[l]) v = a.W[l][(int64_t)pack_src_row(a, l, r) * L.K[l] + pack_src_col(a, l, k)];
  } else {
    const int r = (int)(e - L.b_off[l]);
    if (r < L.rows[l]) v = a.b[l][pack_src_row(a, l, r)];
  }
  return v;
}

inline int fill_pack_args(const gnf_made_net* net, PackArgs* a) {
  if (!net->var_of_step) return GNF_EINVAL;
  for (int l = 0; l <= net->nh; ++l) {
    if (!net->W[l] || !net->b[l] || (l < net->nh && !net->order[l])) return GNF_EINVAL;
    a->W[l] = net->W[l];
    a->b[l] = net->b[l];
    if (l < net->nh) a->order[l] = net->order[l];
  }
  a->var_of_step = net->var_of_step;
  return 0;
}

// ------------------------------------------------------------------------------------------------ one (layer, step)
struct StepArgs {
  MadeLayout lay;
  const int32_t* off[kMaxH];
  const int32_t* var_of_step;
  int spl_K = 0;                // GNF_MADE_NORM_SPLINE: bins and tail bound of the step's normalizer
  double spl_T = 0.;
};

__device__ __forceinline__ float relu_keep_nan(float v) { return v < 0.f ? 0.f : v; }

// dst[r][u] = act(bias[u] + sum_{k < K} W[u][k] in[r][k]) for the n units u of this step and the tile's rows r < nrows.
// W points at the first of those units' packed rows (rows_avail of them follow in the image).  Ends in a barrier.
template <int TB>
__device__ __forceinline__ void layer_step(const float* __restrict__ W, int ldw, int rows_avail,
                                           const float* __restrict__ bias, int n, int K, const float* in, int A,
                                           float* dst, int dstride, bool relu, int nrows, float* red) {
  const int tid = threadIdx.x;
  if (TB == 16 && n >= 8) {
    const int wave = tid >> 6, lane = tid & 63, m = lane & 15, q = lane >> 4;
    const float* a = in + (size_t)(m < nrows ? m : nrows - 1) * A;
    const int nchunks = (K + 15) >> 4;
    for (int nt = 0; nt * 16 < n; ++nt) {
      // B operand: lane (m, q) holds column m of the tile = unit nt * 16 + m (a padding column reads a row that exists)
      const int urow = nt * 16 + m < rows_avail ? nt * 16 + m : rows_avail - 1;
      const float* w = W + (size_t)urow * ldw + 4 * q;
      f32x4 c0 = {0.f, 0.f, 0.f, 0.f}, c1 = {0.f, 0.f, 0.f, 0.f};
#pragma unroll 2
      for (int ch = wave; ch < nchunks; ch += 4) {
        // MFMA i of a chunk contracts k = 16 ch + 4 q + i over q = 0..3: both operands use that same order
        const int kb = ch * 16 + 4 * q;
        const f32x4 wv = ld4(w + ch * 16);
        const float a0 = kb < K ? a[kb] : 0.f;
        const float a1 = kb + 1 < K ? a[kb + 1] : 0.f;
        const float a2 = kb + 2 < K ? a[kb + 2] : 0.f;
        const float a3 = kb + 3 < K ? a[kb + 3] : 0.f;
        c0 = mfma(a0, wv[0], c0);
        c1 = mfma(a1, wv[1], c1);
        c0 = mfma(a2, wv[2], c0);
        c1 = mfma(a3, wv[3], c1);
      }
      c0 += c1;
#pragma unroll
      for (int r = 0; r < 4; ++r) red[wave * 256 + (q * 4 + r) * 16 + m] = c0[r];     // D: row 4 q + r, column m
      __syncthreads();
      {
        const int rm = tid >> 4, u = nt * 16 + (tid & 15);
        if (u < n && rm < nrows) {
          const float v = ((red[tid] + red[256 + tid]) + red[512 + tid]) + red[768 + tid] + bias[u];
          dst[(size_t)rm * dstride + u] = relu ? relu_keep_nan(v) : v;
        }
      }
      __syncthreads();
    }
    return;
  }
  constexpr int G = kThreads / TB;             // lanes per batch row: 16 / 32 / 64, an aligned part of one wavefront
  const int r = tid / G, j = tid % G;
  const float* a = in + (size_t)(r < nrows ? r : nrows - 1) * A;
  for (int u = 0; u < n; ++u) {
    const float* w = W + (size_t)u * ldw;
    float s0 = 0.f, s1 = 0.f, s2 = 0.f, s3 = 0.f;
    int k = j;
    for (; k + 3 * G < K; k += 4 * G) {          // four weight loads in flight: the row comes from L2, the step is latency
      const float w0 = w[k], w1 = w[k + G], w2 = w[k + 2 * G], w3 = w[k + 3 * G];
      s0 = fmaf(w0, a[k], s0);
      s1 = fmaf(w1, a[k + G], s1);
      s2 = fmaf(w2, a[k + 2 * G], s2);
      s3 = fmaf(w3, a[k + 3 * G], s3);
    }
    for (; k < K; k += G) s0 = fmaf(w[k], a[k], s0);
    const float v = group_sum<G>((s0 + s1) + (s2 + s3)) + bias[u];
    if (j == 0 && r < nrows) dst[(size_t)r * dstride + u] = relu ? relu_keep_nan(v) : v;
  }
  __syncthreads();
}

// dst[r][u] = sum_{k0 <= k < K} W[u][k] in[r][k] for the n units u of this step and the tile's rows r < nrows, times the
// unit's ReLU decision (gate: dst holds its activation).  W points at the first of those units' rows of a transposed
// image (rows_avail of them follow).  layer_step's two inner products on a range.  Ends in a barrier.
template <int TB>
__device__ __forceinline__ void suffix_step(const float* __restrict__ W, int ldw, int rows_avail, int n, int k0, int K,
                                            const float* in, int istride, float* dst, int dstride, bool gate, int nrows,
                                            float* red) {
  const int tid = threadIdx.x;
  if (TB == 16 && n >= 8) {
    const int wave = tid >> 6, lane = tid & 63, m = lane & 15, q = lane >> 4;
    const float* a = in + (size_t)(m < nrows ? m : nrows - 1) * istride;
    const int nchunks = (K + 15) >> 4;
    for (int nt = 0; nt * 16 < n; ++nt) {
      const int urow = nt * 16 + m < rows_avail ? nt * 16 + m : rows_avail - 1;
      const float* w = W + (size_t)urow * ldw + 4 * q;
      f32x4 c0 = {0.f, 0.f, 0.f, 0.f}, c1 = {0.f, 0.f, 0.f, 0.f};
#pragma unroll 2
      for (int ch = (k0 >> 4) + wave; ch < nchunks; ch += 4) {
        const int kb = ch * 16 + 4 * q;
        const f32x4 wv = ld4(w + ch * 16);
        const float a0 = kb >= k0 && kb < K ? a[kb] : 0.f;
        const float a1 = kb + 1 >= k0 && kb + 1 < K ? a[kb + 1] : 0.f;
        const float a2 = kb + 2 >= k0 && kb + 2 < K ? a[kb + 2] : 0.f;
        const float a3 = kb + 3 >= k0 && kb + 3 < K ? a[kb + 3] : 0.f;
        c0 = mfma(a0, wv[0], c0);
        c1 = mfma(a1, wv[1], c1);
        c0 = mfma(a2, wv[2], c0);
        c1 = mfma(a3, wv[3], c1);
      }
      c0 += c1;
#pragma unroll
      for (int r = 0; r < 4; ++r) red[wave * 256 + (q * 4 + r) * 16 + m] = c0[r];     // D: row 4 q + r, column m
      __syncthreads();
      {
        const int rm = tid >> 4, u = nt * 16 + (tid & 15);
        if (u < n && rm < nrows) {
          const float v = ((red[tid] + red[256 + tid]) + red[512 + tid]) + red[768 + tid];
          float* o = dst + (size_t)rm * dstride + u;
          *o = !gate || *o > 0.f ? v : 0.f;
        }
      }
      __syncthreads();
    }
    return;
  }
  constexpr int G = kThreads / TB;
  const int r = tid / G, j = tid % G;
  const float* a = in + (size_t)(r < nrows ? r : nrows - 1) * istride;
  for (int u = 0; u < n; ++u) {
    const float* w = W + (size_t)u * ldw;
    float s0 = 0.f, s1 = 0.f, s2 = 0.f, s3 = 0.f;
    int k = k0 + j;
    for (; k + 3 * G < K; k += 4 * G) {
      const float w0 = w[k], w1 = w[k + G], w2 = w[k + 2 * G], w3 = w[k + 3 * G];
      s0 = fmaf(w0, a[k], s0);
      s1 = fmaf(w1, a[k + G], s1);
      s2 = fmaf(w2, a[k + 2 * G], s2);
      s3 = fmaf(w3, a[k + 3 * G], s3);
    }
    for (; k < K; k += G) s0 = fmaf(w[k], a[k], s0);
    const float v = group_sum<G>((s0 + s1) + (s2 + s3));
    if (j == 0 && r < nrows) {
      float* o = dst + (size_t)r * dstride + u;
      *o = !gate || *o > 0.f ? v : 0.f;
    }
  }
  __syncthreads();
}

// batch rows per workgroup: what decides a row's summation order, so both kernels ask here
inline int tile_rows(const gnf_made_net* net, int64_t B) {
  if (net->max_new >= 8 || net->out >= 8) return 16;                  // the MFMA tile
  if ((B + 3) / 4 <= 1024) return 4;                                  // few rows: short steps on many CUs
  if ((B + 7) / 8 <= 1024) return 8;
  return 16;
}

}  // namespace
