// Level sweep of a StrADE net (models/Conditionners/StrADEConditioner.py): the conditioner side of inverting a flow step
// whose masked net encodes a GIVEN DAG, in ONE launch instead of depth + 1 fixed-point passes.  It is the prefix kernel
// (gnf_made_prefix.hip) with "degree" replaced by "topological level" and several variables per step.
//
// Every hidden unit is assigned a parent set S_u (strade_masks); its level is the largest level of a variable in S_u, -1
// for the empty set.  A unit reads variables of S_u only, and units below whose set is a subset of its own, so it is FINAL
// once the variables of the levels <= its own are known.  Level t of the sweep (the variables of level t are inverted in
// it) computes, layer by layer, the hidden units of level t - 1 from the already-final units below them, then the `out`
// outputs of every variable of level t.  Units and variables are kept in LEVEL order (the plan's stable sorts), which
// makes "every unit of level < t" a contiguous K range [0, off[t]) of the activation row and of the packed weight rows.
// Unlike the degree rule, the prefix is not the mask: a unit of level 3 need not read every unit of level <= 3 below it.
// The entries inside the prefix that the mask forbids are exact ZEROS of the weight image -- the pack kernel writes
// mask ? W : 0 -- so the product over the prefix is the masked product, in the same fp32 arithmetic as the dense net.
//
// One workgroup owns TB batch rows and walks the levels t = 0 .. nlev - 1 for them; rows never interact, nothing is
// synchronised across workgroups, no atomics.  The rows' activations [context | x in level order | hidden 0 | ...] live in
// LDS only: there is no workspace, and a net whose tile does not fit at TB = 4 is refused with GNF_ESHAPE (the caller
// inverts by passes).  The inner products are layer_step<TB> of gnf_made.h: MFMA for n >= 8 new units at TB = 16, lane-group
// dot products otherwise; fp32 throughout, a fixed summation order for a given (net, cond_in, B).
//
// The outputs of a level are produced in chunks of kChunkVars variables, so that hbuf ([TB][kChunkVars * out]) stays a
// small, level-independent part of the LDS budget; the normalizer's inverse then runs per (row, variable) of the chunk with
// the arithmetic of gnf_affine_inv / spl_inverse<false>, exactly as made_prefix_k's epilogues, and the result goes to x and
// to the activation row at the variable's level-order position.
//
// An intervention do(x_P = v) hands a pin table over, one byte per VARIABLE (as gnf_made_prefix_do).  A pinned variable
// keeps its level; the caller's x[b, v] takes the place of outputs and inverse.  Two decisions, both said here once:
//   - a chunk whose variables are ALL pinned skips the output product: the table is the same for every lane, the branch
//     is uniform per (level, chunk) and both sides meet the same barriers (layer_step's, or none, then the epilogue's);
//   - in a mixed chunk the product is computed for the whole chunk and the per-variable choice is made AFTER it, in the
//     epilogue, where it is a per-thread select with no barrier inside.
// The hidden units are computed as ever: later levels read them.  pin == NULL instantiates a kernel without the branch.
#include "gnf_strade.h"
#include "gnf_spline.h"

namespace {

struct LevelArgs {
  StepArgs s;
  const int32_t* var_off;
  int nlev;
  int hstride;                  // floats per row of hbuf: min(widest, kChunkVars) * out
};

// the level-ordered image of mask o W (strade_pack_elem), biases behind each layer
__global__ void strade_pack_k(StradePackArgs a, float* __restrict__ pack) {
  const MadeLayout& L = a.p.lay;
  for (int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; e < L.pack_floats; e += (int64_t)gridDim.x * blockDim.x)
    pack[e] = strade_pack_elem(a, e);
}

// (out of line for the reason given at made_prefix_k's: the fp64 exponentials would cost every path its registers)
__device__ __noinline__ float strade_spline_inverse(float* r, int K, double T, float z) { return spl_inverse<false>(r, K, T, z); }

// ------------------------------------------------------------------------------------------------ the sweep kernel
template <int TB, bool kPin>
__global__ __launch_bounds__(kThreads) void strade_levels_k(LevelArgs a, const float* __restrict__ pack,
                                                            const float* __restrict__ context, const float* __restrict__ z,
                                                            float* x, int mode, int64_t B, const uint8_t* __restrict__ pin) {
  extern __shared__ __attribute__((aligned(16))) float smem[];
  const StepArgs& s = a.s;
  const MadeLayout& L = s.lay;
  float* red = smem;
  float* hbuf = smem + kRedFloats;                                   // [TB][hstride]: a chunk's conditioner outputs
  float* act = hbuf + round_up(TB * a.hstride, 4);
  const int tid = threadIdx.x;
  const int64_t row0 = (int64_t)blockIdx.x * TB;
  const int nrows = (int)(B - row0 < TB ? B - row0 : TB);
  const int A = L.A, d = L.d, out = L.out, nh = L.nh, c = L.c;

  if (c > 0) {
    // the context heads the tile's activation rows; one float per load: the caller's rows are dword-aligned, no more
    for (int i = tid; i < nrows * c; i += kThreads) act[(size_t)(i / c) * A + i % c] = context[row0 * c + i];
    __syncthreads();
  }
  for (int t = 0; t < a.nlev; ++t) {
    const int p0 = a.var_off[t], p1 = a.var_off[t + 1];               // the level's variables, positions in level order
    for (int l = 0; l < nh; ++l) {
      const int n0 = t >= 1 ? s.off[l][t - 1] : 0, n1 = s.off[l][t];  // the units of level t - 1 (t = 0: the empty-set units)
      if (n1 == n0) continue;                                         // (uniform: the tables are the same for every lane)
      const int K = l == 0 ? c + p0 : s.off[l - 1][t];                // context, variables / units below of level < t
      layer_step<TB>(pack + L.w_off[l] + (size_t)n0 * L.ldw[l], L.ldw[l], L.rows[l] - n0, pack + L.b_off[l] + n0,
                     n1 - n0, K, act + (l == 0 ? 0 : L.act_off[l - 1]), A, act + L.act_off[l] + n0, A, true, nrows, red);
    }
    const int K = nh == 0 ? c + p0 : s.off[nh - 1][t];                // what the outputs of a variable of level t may read
    for (int q0 = p0; q0 < p1; q0 += kChunkVars) {
      const int nv = p1 - q0 < kChunkVars ? p1 - q0 : kChunkVars;
      // this thread's (row, variable) of the chunk: nrows * nv <= 16 * 8 threads have one
      const bool mine = tid < nrows * nv;
      const int r = mine ? tid / nv : 0, j = mine ? tid % nv : 0;
      const int v = s.var_of_step[q0 + j];
      const bool pinned = kPin && pin[v] != 0;
      bool all_pinned = kPin;
      if (kPin)
        for (int i = 0; i < nv; ++i) all_pinned = all_pinned && pin[s.var_of_step[q0 + i]] != 0;   // uniform
      // z (or the pinned value) is asked for before the product, which hides its latency
      const float zv = !mine ? 0.f : pinned ? x[(row0 + r) * d + v] : z[(row0 + r) * d + v];
      if (!all_pinned) {
        const int n0 = q0 * out;
        layer_step<TB>(pack + L.w_off[nh] + (size_t)n0 * L.ldw[nh], L.ldw[nh], L.rows[nh] - n0, pack + L.b_off[nh] + n0,
                       nv * out, K, act + (nh == 0 ? 0 : L.act_off[nh - 1]), A, hbuf, a.hstride, false, nrows, red);
      }
      if (mine) {
        float xv = zv;                                                // do(x_v): the caller's value, bit for bit
        if (!pinned) {
          float* h = hbuf + r * a.hstride + j * out;
          if (mode == GNF_MADE_NORM_SPLINE) {
            // the arithmetic of gnf_spline_inv on the variable's 3K - 1 outputs (hbuf is rewritten by the next chunk)
            xv = strade_spline_inverse(h, s.spl_K, s.spl_T, zv);
          } else {
            // AffineNormalizer.py:14-17, the arithmetic of gnf_affine_inv
            const float mu = fminf(fmaxf(h[0], -5.f), 5.f);
            const float sg = expf(fminf(fmaxf(h[1], -5.f), 2.f));
            xv = (zv - mu) / sg;
          }
          x[(row0 + r) * d + v] = xv;
        }
        act[(size_t)r * A + c + q0 + j] = xv;
      }
      __syncthreads();          // the chunk's readers of hbuf are done before the next product writes it; act is complete
    }
  }
}

template <int TB>
int launch(const LevelArgs& a, size_t smem, int64_t grid, hipStream_t st, const float* pack, const float* context,
           const float* z, float* x, int mode, int64_t B, const uint8_t* pin) {
  const dim3 g((unsigned)grid), b(kThreads);
  const hipError_t e = pin ? gnf_launch_lds(strade_levels_k<TB, true>, g, b, smem, st, a, pack, context, z, x, mode, B, pin)
                           : gnf_launch_lds(strade_levels_k<TB, false>, g, b, smem, st, a, pack, context, z, x, mode, B, pin);
  return e == hipSuccess ? 0 : (int)e;
}

}  // namespace

extern "C" {

int64_t gnf_strade_pack_floats(const gnf_strade_net* net, int cond_in) {
  MadeLayout lay;
  const int rc = strade_layout(net, cond_in, &lay);
  return rc ? rc : lay.pack_floats;
}

int gnf_strade_pack(const gnf_strade_net* net, int cond_in, float* pack, gnf_stream_t stream) {
  StradePackArgs a;
  const int rc = strade_layout(net, cond_in, &a.p.lay);
  if (rc) return rc;
  if (!pack) return GNF_EINVAL;
  if ((uintptr_t)pack & 15) return GNF_EINVAL;          // the sweep kernel reads the image's rows as 16-byte quads
  if (strade_fill_pack_args(net, &a)) return GNF_EINVAL;
  const int64_t blocks = (a.p.lay.pack_floats + 255) / 256;
  hipLaunchKernelGGL(strade_pack_k, dim3((unsigned)(blocks < 4096 ? blocks : 4096)), dim3(256), 0, (hipStream_t)stream, a,
                     pack);
  GNF_LAUNCH_CHECK();
  return 0;
}

int gnf_strade_levels(const gnf_strade_net* net, int cond_in, const float* context, const float* pack, const float* z,
                      float* x, int normalizer_mode, int spline_bins, double spline_tail, const uint8_t* pin, int64_t B,
                      gnf_stream_t stream) {
  LevelArgs a;
  const int rc = strade_layout(net, cond_in, &a.s.lay);
  if (rc) return rc;
  const gnf_made_net& m = net->made;
  if (B < 0) return GNF_EINVAL;
  if (normalizer_mode != GNF_MADE_NORM_AFFINE && normalizer_mode != GNF_MADE_NORM_SPLINE) return GNF_EINVAL;
  if (normalizer_mode == GNF_MADE_NORM_AFFINE && m.out < 2) return GNF_ESHAPE;
  if (normalizer_mode == GNF_MADE_NORM_SPLINE) {
    if (spline_bins < kSplMinBins || spline_bins > kSplMaxBins || !(spline_tail > 0.) || !(spline_tail < 3.0e38))
      return GNF_EINVAL;
    if (m.out < 3 * spline_bins - 1) return GNF_ESHAPE;
    a.s.spl_K = spline_bins;
    a.s.spl_T = spline_tail;
  }
  // batch rows per workgroup: strade_tile_rows (gnf_strade.h), which the adjoint sweep asks as well
  const int TB = strade_tile_rows(net, a.s.lay, B, &a.hstride);
  if (!TB) return GNF_ESHAPE;
  if (B == 0) return 0;
  if (!pack || !z || !x || !m.var_of_step || !net->var_off || (cond_in > 0 && !context)) return GNF_EINVAL;
  if ((uintptr_t)pack & 15) return GNF_EINVAL;          // rows of the weight image are read as 16-byte quads (ld4)
  for (int l = 0; l < m.nh; ++l) {
    if (!m.off[l]) return GNF_EINVAL;
    a.s.off[l] = m.off[l];
  }
  a.s.var_of_step = m.var_of_step;
  a.var_off = net->var_off;
  a.nlev = net->nlev;
  const int64_t grid = (B + TB - 1) / TB;
  if (grid > 0x7fffffff) return GNF_ESHAPE;
  hipStream_t st = (hipStream_t)stream;
  const size_t smem = (size_t)strade_levels_lds_bytes(a.s.lay, TB, a.hstride);
  switch (TB) {
    case 4: return launch<4>(a, smem, grid, st, pack, context, z, x, normalizer_mode, B, pin);
    case 8: return launch<8>(a, smem, grid, st, pack, context, z, x, normalizer_mode, B, pin);
    default: return launch<16>(a, smem, grid, st, pack, context, z, x, normalizer_mode, B, pin);
  }
}

}  // extern "C"
