// Prefix evaluation of a MADE (models/Conditionners/AutoregressiveConditioner.py): the conditioner side of inverting an
// autoregressive flow step column by column instead of by d fixed-point passes (reference NormalizingFlow.py:98-107).
//
// A hidden unit of degree m reads inputs of degree <= m only, so it is FINAL once the variables of degree 0..m are known.
// Step t (the variable of degree t is inverted in it) therefore computes, layer by layer, just the hidden units of degree
// t-1 from the already-final units below them, then the `out` outputs of that one variable.  Units and inputs are kept in
// DEGREE order (the plan's stable sort), which makes "every unit of degree < t" a contiguous K range [0, off[t]) of the
// activation row and of the packed weight rows: no mask is read, the prefix length IS the mask.
//
// One workgroup owns TB batch rows and walks the steps [t0, t1) for them; rows never interact, so nothing is synchronised
// across workgroups.  The rows' activations live in LDS when one launch runs the whole inversion (Affine normalizer:
// x[b, v] = (z - mu) / sigma is formed right here and is the next step's input), otherwise in the caller's workspace,
// which carries them from one single-step launch to the next (any other normalizer inverts the column in between).
//
// Two inner products, chosen per (layer, step) by the number of new units n:
//   n >= 8 (and TB = 16): v_mfma_f32_16x16x4_f32, batch rows on M, the new units padded to 16 on N, K split over the four
//           wavefronts in chunks of 16 and reduced through LDS in a fixed order;
//   n <  8: plain dot products, 256 / TB lanes per batch row over K, reduced inside the lane group.
// fp32 throughout, fp32 accumulation, a fixed summation order for a given (net, cond_in, B).
//
// A conditional MADE (ConditionnalMADE, cond_in = c > 0) puts c context columns of input degree -1 in FRONT of the variables
// in its first layer.  Degree -1 is known before step 0, so the context simply heads the activation row,
// [context | x in degree order | hidden 0 | ...], and the first layer's prefix at step t is K = c + t.  Without hidden
// layers the output layer is that first layer (K = c at step 0: the outputs of the degree-0 variable move with the
// context); with hidden layers those outputs read no hidden unit and stay the output bias.  c = 0 is the unconditional
// kernel, instruction for instruction on the arithmetic path.
//
// An intervention do(x_P = v) (gnf_made_prefix_do, NormalizingFlowStep.intervene) hands a pin table over, one byte per
// VARIABLE.  A pinned step keeps the hidden units of degree t - 1 -- later columns read them -- and replaces the rest by a
// load: the caller's x[b, v] becomes the activation row's input c + t; no output-layer product, no epilogue, no store to x.
// The table is the same for every lane, so the branch is uniform and both sides meet the same two barriers.  The kernel
// is instantiated with and without pins: pin == NULL launches the kernel of the entry points above, untouched.
#include <vector>

#include "gnf_made.h"
#include "gnf_spline.h"

namespace {

// the weight image (gnf_made.h: pack_elem): rows in degree order, K .. ldw-1 zeros, biases behind each layer
__global__ void made_prefix_pack_k(PackArgs a, float* __restrict__ pack) {
  for (int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; e < a.lay.pack_floats; e += (int64_t)gridDim.x * blockDim.x)
    pack[e] = pack_elem(a, e);
}

// the spline epilogue of a row, kept OUT of line: inlined, its fp64 exponentials take made_prefix_k from 78 - 85 VGPRs to
// 117 - 129 (a wavefront or two per SIMD less) and to nine dwords of scratch, on the Affine and NONE paths as well
__device__ __noinline__ float spline_row_inverse(float* r, int K, double T, float z) { return spl_inverse<false>(r, K, T, z); }

// ------------------------------------------------------------------------------------------------ the step kernel
template <int TB, bool kLds, bool kPin>
__global__ __launch_bounds__(kThreads) void made_prefix_k(StepArgs s, const float* __restrict__ pack,
                                                          const float* __restrict__ context, const float* __restrict__ z,
                                                          float* x, float* __restrict__ h_out, int t0, int t1, int mode,
                                                          float* ws, int64_t B, const uint8_t* __restrict__ pin) {
  extern __shared__ __attribute__((aligned(16))) float smem[];
  const MadeLayout& L = s.lay;
  float* red = smem;
  float* hbuf = smem + kRedFloats;                                   // [TB][out]: the step's conditioner outputs
  const int tid = threadIdx.x;
  const int64_t row0 = (int64_t)blockIdx.x * TB;
  const int nrows = (int)(B - row0 < TB ? B - row0 : TB);
  const int A = L.A, d = L.d, out = L.out, nh = L.nh, c = L.c;
  float* act = kLds ? hbuf + round_up(TB * out, 4) : ws + (size_t)row0 * A;

  if (c > 0 && (kLds || t0 == 0)) {
    // the context heads the tile's activation rows, once per inversion: later step launches find it in the workspace.
    // One float per load: the caller's rows are dword-aligned, no more
    for (int i = tid; i < nrows * c; i += kThreads) act[(size_t)(i / c) * A + i % c] = context[row0 * c + i];
    __syncthreads();
  }
  if (!kLds && t0 >= 1) {
    // the column the caller inverted (or pinned: x holds it either way) since the previous launch: the newest input of
    // this one
    if (tid < nrows) act[(size_t)tid * A + c + t0 - 1] = x[(row0 + tid) * d + s.var_of_step[t0 - 1]];
    __syncthreads();
  }
  for (int t = t0; t < t1; ++t) {
    const int v = s.var_of_step[t];
    // the step's z is asked for before the layers, which hide its latency
    const bool pinned = kPin && pin[v] != 0;                           // one byte per variable: uniform over the workgroup
    const float zv = mode != GNF_MADE_NORM_NONE && !pinned && tid < nrows ? z[(row0 + tid) * d + v] : 0.f;
    if (t >= 1)
      for (int l = 0; l < nh; ++l) {
        const int n0 = s.off[l][t - 1], n1 = s.off[l][t];             // the units of degree t - 1
        const int K = l == 0 ? c + t : s.off[l - 1][t];                // context, inputs / units below of degree <= t - 1
        layer_step<TB>(pack + L.w_off[l] + (size_t)n0 * L.ldw[l], L.ldw[l], L.rows[l] - n0, pack + L.b_off[l] + n0,
                       n1 - n0, K, act + (l == 0 ? 0 : L.act_off[l - 1]), A, act + L.act_off[l] + n0, A, true, nrows, red);
      }
    if (pinned) {
      // do(x_v): the caller's value is what the later steps read; the step's outputs and its z have no reader.  The barrier
      // stands where the output layer's would (the last step's readers of hbuf are past the one that ended it)
      if (tid < nrows) act[(size_t)tid * A + c + t] = x[(row0 + tid) * d + v];
      __syncthreads();
    } else {
      const int K = nh == 0 ? c + t : s.off[nh - 1][t];                // strict rule: degree < t (the context's is -1)
      const int n0 = t * out;
      layer_step<TB>(pack + L.w_off[nh] + (size_t)n0 * L.ldw[nh], L.ldw[nh], L.rows[nh] - n0, pack + L.b_off[nh] + n0,
                     out, K, act + (nh == 0 ? 0 : L.act_off[nh - 1]), A, hbuf, out, false, nrows, red);
    }
    if (pinned) {
      // nothing: h_out and x[b, v] stay the caller's
    } else if (mode == GNF_MADE_NORM_NONE) {
      for (int i = tid; i < nrows * out; i += kThreads) h_out[row0 * out + i] = hbuf[i];
    } else if (tid < nrows) {
      float xv;
      if (mode == GNF_MADE_NORM_SPLINE) {
        // the arithmetic of gnf_spline_inv on the row's 3K - 1 outputs (hbuf is rewritten by the next step)
        xv = spline_row_inverse(hbuf + tid * out, s.spl_K, s.spl_T, zv);
      } else {
        // AffineNormalizer.py:14-17, the arithmetic of gnf_affine_inv
        const float mu = fminf(fmaxf(hbuf[tid * out], -5.f), 5.f);
        const float sg = expf(fminf(fmaxf(hbuf[tid * out + 1], -5.f), 2.f));
        xv = (zv - mu) / sg;
      }
      x[(row0 + tid) * d + v] = xv;
      act[(size_t)tid * A + c + t] = xv;
    }
    __syncthreads();
  }
}

int64_t lds_bytes(const MadeLayout& lay, int TB, bool with_act) {
  return 4 * ((int64_t)kRedFloats + round_up(TB * lay.out, 4) + (with_act ? (int64_t)TB * lay.A : 0));
}

template <int TB>
int launch(const StepArgs& s, bool lds, size_t smem, int64_t grid, hipStream_t st, const float* pack, const float* context,
           const float* z, float* x, float* h_out, int t0, int t1, int mode, float* ws, int64_t B, const uint8_t* pin) {
  const dim3 g((unsigned)grid), b(kThreads);
  hipError_t e;
  if (pin)
    e = lds ? gnf_launch_lds(made_prefix_k<TB, true, true>, g, b, smem, st, s, pack, context, z, x, h_out, t0, t1, mode, ws, B,
                             pin)
            : gnf_launch_lds(made_prefix_k<TB, false, true>, g, b, smem, st, s, pack, context, z, x, h_out, t0, t1, mode, ws,
                             B, pin);
  else
    e = lds ? gnf_launch_lds(made_prefix_k<TB, true, false>, g, b, smem, st, s, pack, context, z, x, h_out, t0, t1, mode, ws,
                             B, pin)
            : gnf_launch_lds(made_prefix_k<TB, false, false>, g, b, smem, st, s, pack, context, z, x, h_out, t0, t1, mode, ws,
                             B, pin);
  return e == hipSuccess ? 0 : (int)e;
}

// GNF_MADE_NORM_NONE over more than one step: every step but the last must be pinned (its outputs would have no caller to
// invert them).  The table lives on the device, so this one form of the call reads it back -- d bytes and the steps'
// variables -- and waits for the stream; every other form is checked from the host arguments alone.
int check_pinned_run(const gnf_made_net* net, const uint8_t* pin, int t0, int t1, hipStream_t st) {
  std::vector<uint8_t> tab((size_t)net->d);
  std::vector<int32_t> var((size_t)(t1 - 1 - t0));
  hipError_t e = hipMemcpyAsync(tab.data(), pin, tab.size(), hipMemcpyDeviceToHost, st);
  if (e == hipSuccess) e = hipMemcpyAsync(var.data(), net->var_of_step + t0, 4 * var.size(), hipMemcpyDeviceToHost, st);
  if (e == hipSuccess) e = hipStreamSynchronize(st);
  if (e != hipSuccess) return (int)e;
  for (int32_t v : var)
    if (v < 0 || v >= net->d || !tab[(size_t)v]) return GNF_EINVAL;
  return 0;
}

int prefix_run(const gnf_made_net* net, int cond_in, const float* context, const float* pack, const float* z, float* x,
               float* h_out, int t0, int t1, int normalizer_mode, int spline_bins, double spline_tail, const uint8_t* pin,
               int64_t B, void* ws, int64_t ws_bytes, gnf_stream_t stream) {
  StepArgs s;
  const int rc = make_layout(net, cond_in, &s.lay);
  if (rc) return rc;
  if (B < 0 || t0 < 0 || t1 < t0 || t1 > net->d) return GNF_EINVAL;
  if (normalizer_mode != GNF_MADE_NORM_NONE && normalizer_mode != GNF_MADE_NORM_AFFINE &&
      normalizer_mode != GNF_MADE_NORM_SPLINE)
    return GNF_EINVAL;
  // NONE hands ONE variable's outputs back; more steps only behind a run of pinned ones (checked below, on the table)
  const bool run = normalizer_mode == GNF_MADE_NORM_NONE && t1 > t0 + 1;
  if (run && !pin) return GNF_EINVAL;
  if (normalizer_mode == GNF_MADE_NORM_AFFINE && net->out < 2) return GNF_ESHAPE;
  if (normalizer_mode == GNF_MADE_NORM_SPLINE) {
    if (spline_bins < kSplMinBins || spline_bins > kSplMaxBins || !(spline_tail > 0.) || !(spline_tail < 3.0e38))
      return GNF_EINVAL;
    if (net->out < 3 * spline_bins - 1) return GNF_ESHAPE;
    s.spl_K = spline_bins;
    s.spl_T = spline_tail;
  }
  if (B == 0 || t1 == t0) return 0;
  if (!pack || !x || !net->var_of_step || (cond_in > 0 && !context)) return GNF_EINVAL;
  if ((uintptr_t)pack & 15) return GNF_EINVAL;          // rows of the weight image are read as 16-byte quads (ld4)
  if (normalizer_mode == GNF_MADE_NORM_NONE ? !h_out : !z) return GNF_EINVAL;
  for (int l = 0; l < net->nh; ++l) {
    if (!net->off[l]) return GNF_EINVAL;
    s.off[l] = net->off[l];
  }
  s.var_of_step = net->var_of_step;
  const int TB = tile_rows(net, B);
  const int64_t grid = (B + TB - 1) / TB;
  if (grid > 0x7fffffff) return GNF_ESHAPE;
  hipStream_t st = (hipStream_t)stream;
  if (run) {
    const int bad = check_pinned_run(net, pin, t0, t1, st);
    if (bad) return bad;
  }
  // the whole inversion in one launch keeps the tile's activations in LDS; step launches hand them on through ws
  const bool lds = t0 == 0 && t1 == net->d && lds_bytes(s.lay, TB, true) <= kLdsBytes;
  if (lds_bytes(s.lay, TB, false) > kLdsBytes) return GNF_ESHAPE;
  if (!lds && (!ws || ws_bytes < 4 * B * s.lay.A)) return GNF_EWS;
  const size_t smem = (size_t)lds_bytes(s.lay, TB, lds);
  float* w = (float*)ws;
  switch (TB) {
    case 4: return launch<4>(s, lds, smem, grid, st, pack, context, z, x, h_out, t0, t1, normalizer_mode, w, B, pin);
    case 8: return launch<8>(s, lds, smem, grid, st, pack, context, z, x, h_out, t0, t1, normalizer_mode, w, B, pin);
    default: return launch<16>(s, lds, smem, grid, st, pack, context, z, x, h_out, t0, t1, normalizer_mode, w, B, pin);
  }
}

}  // namespace

extern "C" {

int64_t gnf_made_prefix_ctx_pack_floats(const gnf_made_net* net, int cond_in) {
  MadeLayout lay;
  const int rc = make_layout(net, cond_in, &lay);
  return rc ? rc : lay.pack_floats;
}

int gnf_made_prefix_ctx_pack(const gnf_made_net* net, int cond_in, float* pack, gnf_stream_t stream) {
  PackArgs a;
  const int rc = make_layout(net, cond_in, &a.lay);
  if (rc) return rc;
  if (!pack) return GNF_EINVAL;
  if ((uintptr_t)pack & 15) return GNF_EINVAL;          // the step kernel reads the image's rows as 16-byte quads
  if (fill_pack_args(net, &a)) return GNF_EINVAL;
  const int64_t blocks = (a.lay.pack_floats + 255) / 256;
  hipLaunchKernelGGL(made_prefix_pack_k, dim3((unsigned)(blocks < 4096 ? blocks : 4096)), dim3(256), 0, (hipStream_t)stream,
                     a, pack);
  GNF_LAUNCH_CHECK();
  return 0;
}

int64_t gnf_made_prefix_ctx_ws_bytes(const gnf_made_net* net, int cond_in, int64_t B) {
  MadeLayout lay;
  const int rc = make_layout(net, cond_in, &lay);
  if (rc) return rc;
  if (B < 0) return GNF_EINVAL;
  return 4 * B * lay.A;
}

int gnf_made_prefix_ctx_spline(const gnf_made_net* net, int cond_in, const float* context, const float* pack, const float* z,
                               float* x, float* h_out, int t0, int t1, int normalizer_mode, int spline_bins, double spline_tail,
                               int64_t B, void* ws, int64_t ws_bytes, gnf_stream_t stream) {
  return prefix_run(net, cond_in, context, pack, z, x, h_out, t0, t1, normalizer_mode, spline_bins, spline_tail, nullptr, B,
                    ws, ws_bytes, stream);
}

// ... and with a pin table (do(x_P = v)): pin == NULL is the call above
int gnf_made_prefix_do(const gnf_made_net* net, int cond_in, const float* context, const float* pack, const float* z, float* x,
                       float* h_out, int t0, int t1, int normalizer_mode, int spline_bins, double spline_tail,
                       const uint8_t* pin, int64_t B, void* ws, int64_t ws_bytes, gnf_stream_t stream) {
  return prefix_run(net, cond_in, context, pack, z, x, h_out, t0, t1, normalizer_mode, spline_bins, spline_tail, pin, B, ws,
                    ws_bytes, stream);
}

// the entry points from before the spline: the same code, any mode but NONE / AFFINE refused as ever
int gnf_made_prefix_ctx(const gnf_made_net* net, int cond_in, const float* context, const float* pack, const float* z,
                        float* x, float* h_out, int t0, int t1, int normalizer_mode, int64_t B, void* ws, int64_t ws_bytes,
                        gnf_stream_t stream) {
  if (normalizer_mode == GNF_MADE_NORM_SPLINE) return GNF_EINVAL;
  return gnf_made_prefix_ctx_spline(net, cond_in, context, pack, z, x, h_out, t0, t1, normalizer_mode, 0, 0., B, ws, ws_bytes,
                                    stream);
}

int gnf_made_prefix_spline(const gnf_made_net* net, const float* pack, const float* z, float* x, float* h_out, int t0, int t1,
                           int normalizer_mode, int spline_bins, double spline_tail, int64_t B, void* ws, int64_t ws_bytes,
                           gnf_stream_t stream) {
  return gnf_made_prefix_ctx_spline(net, 0, nullptr, pack, z, x, h_out, t0, t1, normalizer_mode, spline_bins, spline_tail, B,
                                    ws, ws_bytes, stream);
}

// the unconditional entry points: cond_in = 0 of the same code
int64_t gnf_made_prefix_pack_floats(const gnf_made_net* net) { return gnf_made_prefix_ctx_pack_floats(net, 0); }

int gnf_made_prefix_pack(const gnf_made_net* net, float* pack, gnf_stream_t stream) {
  return gnf_made_prefix_ctx_pack(net, 0, pack, stream);
}

int64_t gnf_made_prefix_ws_bytes(const gnf_made_net* net, int64_t B) { return gnf_made_prefix_ctx_ws_bytes(net, 0, B); }

int gnf_made_prefix(const gnf_made_net* net, const float* pack, const float* z, float* x, float* h_out, int t0, int t1,
                    int normalizer_mode, int64_t B, void* ws, int64_t ws_bytes, gnf_stream_t stream) {
  return gnf_made_prefix_ctx(net, 0, nullptr, pack, z, x, h_out, t0, t1, normalizer_mode, B, ws, ws_bytes, stream);
}

}  // extern "C"
