// The adjoint of the column sweep of gnf_made_prefix.hip: lambda with J^T lambda = g for one MADE step z = S(x), the hot
// path of NormalizingFlowStep.rsample's backward (implicit function theorem: dL/dz = lambda, and the parameter / context
// gradients are ONE ordinary vjp of the step with cotangent -lambda).
//
// In degree order J = dz/dx is lower triangular, J = D + N: D = diag(jac) is the normalizer's own derivative, and
// N[t'][t] = sum_k dzdh[t'][k] dh[t'][k]/dx[t] is non-zero for t' > t only.  So the transposed system is solved from the
// LAST degree down:  lambda_t = (g_t - u_t) / jac_t,  u_t = sum_{t' > t} N[t'][t] lambda_t' = the input cotangent of
// variable t when the outputs of every later variable t' carry the cotangent lambda_t' dzdh[t'][:].  That backpropagation
// is incremental exactly as the forward sweep is: a hidden unit of degree m feeds outputs of degree > m only (units of
// degree >= m in the layer above), so its cotangent is FINAL once lambda_{m+1} .. lambda_{d-1} are known.  Step t therefore
// finalises, from the last hidden layer down, just the units of degree t -- each a contraction over a SUFFIX of the layer
// above, [off[l+1][t], width) (output rows [(t+1) out, d out) for the last hidden layer: the strict rule) -- times the ReLU
// decision, and then u_t from the suffix [off[0][t], width) of the first layer.  Units are in degree order, so the suffix
// start IS the mask, and in the TRANSPOSED weight image (rows = the units of the layer below) every such contraction is a
// contiguous range of one row.
//
// One workgroup owns TB batch rows; rows never interact.  Phase 1 replays the hidden units from the known x with the
// prefix kernel's own layer_step, step by step and with the prefix kernel's tile height, so the ReLU decisions kept are
// those of the sweep that produced x.  Phase 2 walks t = d-1 .. 0 and overwrites each activation by its unit's cotangent
// (the activation is read once, for act > 0).  The rows [context | x | hidden ...] and the output cotangents [d out] live
// in LDS when they fit, in the caller's workspace otherwise: the same code on another pointer, the same bits.
//
// The two inner products of layer_step over a range [k0, K): n >= 8 new units (and TB = 16) on v_mfma_f32_16x16x4_f32,
// the 16-chunks of the range split over the four wavefronts and reduced through LDS in a fixed order; lane-group dot
// products otherwise.  fp32 throughout, a fixed summation order for a given (net, cond_in, B).
//
// An intervention do(x_P = v) (gnf_made_adjoint_do, NormalizingFlowStep.rsample_do's backward) hands a pin table over, one
// byte per VARIABLE.  The equation of a pinned variable is x_t = v_t, so lambda_t := 0 and the cotangent row of its outputs
// is exact zeros -- both by SELECTION: jac and dzdh of a pinned element are never read, whatever they hold -- and
// gdo_t = g_t - u_t is dL/dv.  What the table makes dead is skipped: with t_last the last free step, the steps above it
// have u = 0 exactly (nothing that reads them carries a cotangent), so they run no contraction at all and phase 1 replays
// the hidden units up to degree t_last - 1 only -- the units of degree >= t_last stay 0, a closed gate in front of a
// cotangent that is zero anyway; and a pinned step whose caller takes no gdo skips the first-layer contraction behind
// u_t.  Every such branch depends on the table and the gdo pointer alone: all 256 threads reach every barrier.  The kernel
// is instantiated with and without pins: pin == NULL launches the kernel of gnf_made_adjoint, untouched.
#include "gnf_made.h"

namespace {

constexpr int kSmallFloats = 32;             // u_t and lambda_t of the tile's rows

// the transposed images behind the forward image: layer l as [K[l]][ldt[l]], element [k][r] = the forward image's [r][k]
struct AdjLayout {
  MadeLayout lay;
  int ldt[kMaxH + 1];           // rows[l] rounded up to 16, the tail zero-filled
  int64_t t_off[kMaxH + 1];     // float offsets into the pack
  int64_t pack_floats;          // forward image + transposed images
  int gos;                      // floats per row of output cotangents, made odd like A
};

int make_adj_layout(const gnf_made_net* net, int cond_in, AdjLayout* a) {
  const int rc = make_layout(net, cond_in, &a->lay);
  if (rc) return rc;
  int64_t off = a->lay.pack_floats;          // a multiple of 4 floats: every image row stays 16-byte aligned
  for (int l = 0; l <= a->lay.nh; ++l) {
    a->ldt[l] = round_up(a->lay.rows[l], 16);
    a->t_off[l] = off;
    off += (int64_t)a->lay.K[l] * a->ldt[l];
  }
  a->pack_floats = off;
  a->gos = (a->lay.d * a->lay.out) | 1;
  return 0;
}

struct AdjPackArgs {
  PackArgs p;
  int ldt[kMaxH + 1];
  int64_t t_off[kMaxH + 1];
  int64_t pack_floats;
};

__global__ void made_adjoint_pack_k(AdjPackArgs a, float* __restrict__ pack) {
  const MadeLayout& L = a.p.lay;
  for (int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; e < a.pack_floats; e += (int64_t)gridDim.x * blockDim.x) {
    float v = 0.f;
    if (e < L.pack_floats) {
      v = pack_elem(a.p, e);
    } else {
      int l = 0;
      while (l < L.nh && e >= a.t_off[l + 1]) ++l;
      const int64_t i = e - a.t_off[l];
      const int k = (int)(i / a.ldt[l]), r = (int)(i - (int64_t)k * a.ldt[l]);
      if (r < L.rows[l]) v = a.p.W[l][(int64_t)pack_src_row(a.p, l, r) * L.K[l] + pack_src_col(a.p, l, k)];
    }
    pack[e] = v;
  }
}

struct AdjArgs {
  StepArgs s;
  int ldt[kMaxH + 1];
  int64_t t_off[kMaxH + 1];
  int gos;
};

template <int TB, bool kLds, bool kPin>
__global__ __launch_bounds__(kThreads) void made_adjoint_k(AdjArgs p, const float* __restrict__ pack,
                                                           const float* __restrict__ context, const float* __restrict__ x,
                                                           const float* __restrict__ g, const float* __restrict__ jac,
                                                           const float* __restrict__ dzdh, float* __restrict__ lam,
                                                           float* ws, int64_t B, const uint8_t* __restrict__ pin,
                                                           float* __restrict__ gdo) {
  extern __shared__ __attribute__((aligned(16))) float smem[];
  const StepArgs& s = p.s;
  const MadeLayout& L = s.lay;
  float* red = smem;
  float* ubuf = smem + kRedFloats;                                   // [TB] u_t
  float* lbuf = ubuf + 16;                                           // [TB] lambda_t
  const int tid = threadIdx.x;
  const int64_t row0 = (int64_t)blockIdx.x * TB;
  const int nrows = (int)(B - row0 < TB ? B - row0 : TB);
  const int A = L.A, d = L.d, out = L.out, nh = L.nh, c = L.c, gos = p.gos;
  // [TB][A] activations, then cotangents | [TB][gos] output cotangents
  float* act = kLds ? smem + kRedFloats + kSmallFloats : ws + (size_t)row0 * (A + gos);
  float* go = act + (size_t)TB * A;
  // the last free step, -1 when every variable is pinned (one byte per variable: uniform over the workgroup)
  int t_last = d - 1;
  if (kPin)
    while (t_last >= 0 && pin[s.var_of_step[t_last]] != 0) --t_last;
  const int t_end = kPin ? t_last + 1 : d;     // phase 1 replays the units of degree < t_end - 1

  // ---- phase 1: the hidden units of the pass that produced x.  Units of degree d - 1 are never evaluated (no output reads
  // them): they stay 0, a closed gate in front of a cotangent that is zero anyway
  for (int i = tid; i < TB * A; i += kThreads) act[i] = 0.f;
  __syncthreads();
  // one float per load: the caller's rows are dword-aligned, no more
  for (int i = tid; i < nrows * c; i += kThreads) act[(size_t)(i / c) * A + i % c] = context[row0 * c + i];
  for (int i = tid; i < nrows * d; i += kThreads) act[(size_t)(i / d) * A + c + i % d] = x[(row0 + i / d) * d + s.var_of_step[i % d]];
  __syncthreads();
  for (int t = 1; t < t_end; ++t)
    for (int l = 0; l < nh; ++l) {
      const int n0 = s.off[l][t - 1], n1 = s.off[l][t];
      const int K = l == 0 ? c + t : s.off[l - 1][t];
      layer_step<TB>(pack + L.w_off[l] + (size_t)n0 * L.ldw[l], L.ldw[l], L.rows[l] - n0, pack + L.b_off[l] + n0,
                     n1 - n0, K, act + (l == 0 ? 0 : L.act_off[l - 1]), A, act + L.act_off[l] + n0, A, true, nrows, red);
    }

  // ---- phase 2: the sweep
  const int KO = d * out;
  for (int t = d - 1; t >= 0; --t) {
    const int v = s.var_of_step[t];
    const bool pinned = kPin && pin[v] != 0;
    const bool live = !kPin || t <= t_last;                           // a step of the trailing pinned run contracts nothing
    // asked for before the layers, which hide the latency (jac of a pinned element is not read: it may hold anything)
    const float gv = tid < nrows ? g[(row0 + tid) * d + v] : 0.f;
    const float jv = tid < nrows && !pinned ? jac[(row0 + tid) * d + v] : 1.f;
    if (live)
      for (int l = nh - 1; l >= 0; --l) {
        const int n0 = s.off[l][t], n1 = s.off[l][t + 1];             // the units of degree t
        const bool last = l == nh - 1;
        suffix_step<TB>(pack + p.t_off[l + 1] + (size_t)n0 * p.ldt[l + 1], p.ldt[l + 1], L.rows[l] - n0, n1 - n0,
                        last ? (t + 1) * out : s.off[l + 1][t], last ? KO : L.rows[l + 1],
                        last ? go : act + L.act_off[l + 1], last ? gos : A, act + L.act_off[l] + n0, A, true, nrows, red);
      }
    // u_t: column c + t of the first layer against the cotangents of everything that reads variable t (a pinned step
    // needs it for gdo alone)
    const bool with_u = live && (!pinned || gdo != nullptr);
    if (with_u)
      suffix_step<TB>(pack + p.t_off[0] + (size_t)(c + t) * p.ldt[0], p.ldt[0], d - t, 1,
                      nh == 0 ? (t + 1) * out : s.off[0][t], nh == 0 ? KO : L.rows[0],
                      nh == 0 ? go : act + L.act_off[0], nh == 0 ? gos : A, ubuf, 1, false, nrows, red);
    if (tid < nrows) {
      if (pinned) {
        lam[(row0 + tid) * d + v] = 0.f;
        if (gdo) gdo[(row0 + tid) * d + v] = live ? gv - ubuf[tid] : gv;
      } else {
        const float lv = (gv - ubuf[tid]) / jv;
        lam[(row0 + tid) * d + v] = lv;
        lbuf[tid] = lv;
        if (kPin && gdo) gdo[(row0 + tid) * d + v] = 0.f;
      }
    }
    __syncthreads();
    // the cotangent of this variable's outputs, read by the steps below: exact zeros for a pinned one (dzdh is not read)
    if (t > 0)
      for (int i = tid; i < nrows * out; i += kThreads)
        go[(size_t)(i / out) * gos + t * out + i % out] =
            pinned ? 0.f : lbuf[i / out] * dzdh[((row0 + i / out) * d + v) * out + i % out];
    __syncthreads();
  }
}

int64_t lds_bytes(const AdjLayout& a, int TB, bool with_rows) {
  return 4 * ((int64_t)kRedFloats + kSmallFloats + (with_rows ? (int64_t)TB * (a.lay.A + a.gos) : 0));
}

int64_t ws_floats(const AdjLayout& a, int64_t B) { return (B + 15) / 16 * 16 * ((int64_t)a.lay.A + a.gos); }

template <int TB>
int launch(const AdjArgs& p, bool lds, size_t smem, int64_t grid, hipStream_t st, const float* pack, const float* context,
           const float* x, const float* g, const float* jac, const float* dzdh, float* lam, float* ws, int64_t B,
           const uint8_t* pin, float* gdo) {
  const dim3 gr((unsigned)grid), bl(kThreads);
  hipError_t e;
  if (pin)
    e = lds ? gnf_launch_lds(made_adjoint_k<TB, true, true>, gr, bl, smem, st, p, pack, context, x, g, jac, dzdh, lam, ws, B,
                             pin, gdo)
            : gnf_launch_lds(made_adjoint_k<TB, false, true>, gr, bl, smem, st, p, pack, context, x, g, jac, dzdh, lam, ws, B,
                             pin, gdo);
  else
    e = lds ? gnf_launch_lds(made_adjoint_k<TB, true, false>, gr, bl, smem, st, p, pack, context, x, g, jac, dzdh, lam, ws,
                             B, pin, gdo)
            : gnf_launch_lds(made_adjoint_k<TB, false, false>, gr, bl, smem, st, p, pack, context, x, g, jac, dzdh, lam, ws,
                             B, pin, gdo);
  return e == hipSuccess ? 0 : (int)e;
}

int adjoint_run(const gnf_made_net* net, int cond_in, const float* context, const float* pack, const float* x, const float* g,
                const float* jac, const float* dzdh, float* lambda, const uint8_t* pin, float* gdo, int64_t B, int force_ws,
                void* ws, int64_t ws_bytes, gnf_stream_t stream) {
  AdjLayout lay;
  const int rc = make_adj_layout(net, cond_in, &lay);
  if (rc) return rc;
  if (B < 0) return GNF_EINVAL;
  if (gdo && !pin) return GNF_EINVAL;                                // dL/dv of no intervention
  if (B == 0) return 0;
  if (!pack || !x || !g || !jac || !dzdh || !lambda || !net->var_of_step || (cond_in > 0 && !context)) return GNF_EINVAL;
  if ((uintptr_t)pack & 15) return GNF_EINVAL;
  AdjArgs p;
  p.s.lay = lay.lay;
  for (int l = 0; l < net->nh; ++l) {
    if (!net->off[l]) return GNF_EINVAL;
    p.s.off[l] = net->off[l];
  }
  p.s.var_of_step = net->var_of_step;
  for (int l = 0; l <= net->nh; ++l) {
    p.ldt[l] = lay.ldt[l];
    p.t_off[l] = lay.t_off[l];
  }
  p.gos = lay.gos;
  const int TB = tile_rows(net, B);                                  // the prefix kernel's: the replay repeats its sums
  const int64_t grid = (B + TB - 1) / TB;
  if (grid > 0x7fffffff) return GNF_ESHAPE;
  const bool lds = !force_ws && lds_bytes(lay, TB, true) <= kLdsBytes;
  if (!lds && (!ws || ws_bytes < 4 * ws_floats(lay, B))) return GNF_EWS;
  const size_t smem = (size_t)lds_bytes(lay, TB, lds);
  hipStream_t st = (hipStream_t)stream;
  float* w = (float*)ws;
  switch (TB) {
    case 4: return launch<4>(p, lds, smem, grid, st, pack, context, x, g, jac, dzdh, lambda, w, B, pin, gdo);
    case 8: return launch<8>(p, lds, smem, grid, st, pack, context, x, g, jac, dzdh, lambda, w, B, pin, gdo);
    default: return launch<16>(p, lds, smem, grid, st, pack, context, x, g, jac, dzdh, lambda, w, B, pin, gdo);
  }
}

}  // namespace

extern "C" {

int64_t gnf_made_adjoint_pack_floats(const gnf_made_net* net, int cond_in) {
  AdjLayout a;
  const int rc = make_adj_layout(net, cond_in, &a);
  return rc ? rc : a.pack_floats;
}

int gnf_made_adjoint_pack(const gnf_made_net* net, int cond_in, float* pack, gnf_stream_t stream) {
  AdjLayout lay;
  const int rc = make_adj_layout(net, cond_in, &lay);
  if (rc) return rc;
  if (!pack || ((uintptr_t)pack & 15)) return GNF_EINVAL;            // image rows are read as 16-byte quads
  AdjPackArgs a;
  a.p.lay = lay.lay;
  if (fill_pack_args(net, &a.p)) return GNF_EINVAL;
  for (int l = 0; l <= net->nh; ++l) {
    a.ldt[l] = lay.ldt[l];
    a.t_off[l] = lay.t_off[l];
  }
  a.pack_floats = lay.pack_floats;
  const int64_t blocks = (a.pack_floats + 255) / 256;
  hipLaunchKernelGGL(made_adjoint_pack_k, dim3((unsigned)(blocks < 4096 ? blocks : 4096)), dim3(256), 0, (hipStream_t)stream,
                     a, pack);
  GNF_LAUNCH_CHECK();
  return 0;
}

int64_t gnf_made_adjoint_ws_bytes(const gnf_made_net* net, int cond_in, int64_t B) {
  AdjLayout a;
  const int rc = make_adj_layout(net, cond_in, &a);
  if (rc) return rc;
  if (B < 0) return GNF_EINVAL;
  return 4 * ws_floats(a, B);
}

int gnf_made_adjoint(const gnf_made_net* net, int cond_in, const float* context, const float* pack, const float* x,
                     const float* g, const float* jac, const float* dzdh, float* lambda, int64_t B, int force_ws, void* ws,
                     int64_t ws_bytes, gnf_stream_t stream) {
  return adjoint_run(net, cond_in, context, pack, x, g, jac, dzdh, lambda, nullptr, nullptr, B, force_ws, ws, ws_bytes,
                     stream);
}

// ... and with a pin table (do(x_P = v)): pin == NULL is the call above
int gnf_made_adjoint_do(const gnf_made_net* net, int cond_in, const float* context, const float* pack, const float* x,
                        const float* g, const float* jac, const float* dzdh, float* lambda, const uint8_t* pin, float* gdo,
                        int64_t B, int force_ws, void* ws, int64_t ws_bytes, gnf_stream_t stream) {
  return adjoint_run(net, cond_in, context, pack, x, g, jac, dzdh, lambda, pin, gdo, B, force_ws, ws, ws_bytes, stream);
}

}  // extern "C"
