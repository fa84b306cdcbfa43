// The adjoint of the level sweep of gnf_strade_levels.hip: lambda with J^T lambda = g for one StrADE step z = S(x), the
// backward of NormalizingFlowStep.rsample for a StrADEConditioner with adjoint_levels on.  It is the adjoint MADE sweep
// (gnf_made_adjoint.hip) with "degree" replaced by "topological level": nlev dependent steps where MADE has d.
//
// In level order J = dz/dx = D + N: D = diag(jac) the normalizer's own derivative, N[p'][p] non-zero only when the level of
// p' is ABOVE the level of p.  So the transposed system is solved from the last level down, a whole level at once (variables
// of one level never read each other):  lambda_p = (g_p - u_p) / jac_p,  u_p = the input cotangent of variable p when the
// outputs of every variable p' of a later level carry the cotangent lambda_p' dzdh[p'][:].  A hidden unit of level m feeds
// units of level >= m above it and outputs of variables of level > m, so its cotangent is FINAL once the levels above m are
// solved.  Level t therefore finalises, from the last hidden layer down, just the units of level t -- each a contraction
// over a SUFFIX of the layer above, [off[l+1][t], width) (output rows [var_off[t+1] out, d out) for the last hidden layer)
// -- times the ReLU decision, and then u_p for the level's variables from the suffix [off[0][t], width) of the first layer.
// Unlike the degree rule the suffix start is NOT the mask: a unit of level 3 need not feed every unit of level >= 3 above
// it.  The entries inside the suffix that the mask forbids are the exact zeros of the weight image, as in the forward sweep.
// The empty-set units (level -1) reach no variable and are never finalised; the units of the last level are never
// evaluated by the replay (no output reads them): they stay 0, a closed gate in front of a cotangent that is zero anyway.
//
// One workgroup owns TB batch rows; rows never interact, nothing crosses workgroups, no atomics.  Phase 1 replays the hidden
// units from the known x exactly as strade_levels_k computes them -- the same layer_step calls, the same tile height
// (strade_tile_rows; 4 where that sweep declines the net) -- so the ReLU decisions kept are those of the sweep that
// produced x.  Phase 2 walks t = nlev-1 .. 0 and overwrites each activation by its unit's cotangent.  u of a level is
// produced in chunks of kChunkVars variables (one suffix_step: n = the chunk's variables, W = rows c + q0 .. of the
// transposed first-layer image), so the small buffers are [TB][kChunkVars] whatever the widest level.  The rows
// [context | x in level order | hidden ...] and the output cotangents [d out] live in LDS when they fit, in the caller's
// workspace otherwise: the same code on another pointer, the same bits.  jac and dzdh are operands: any normalizer.
//
// Every __syncthreads() is reached by all 256 threads: the branches around suffix_step / layer_step depend on the tables
// alone, which are the same for every lane.
//
// An intervention do(x_P = v) (gnf_strade_adjoint_do, rsample_do's backward) hands a pin table over, one byte per VARIABLE.
// A pinned variable keeps its level; its lambda := 0 and the cotangent row of its outputs is exact zeros, both by SELECTION
// (jac and dzdh of a pinned element are never read), and gdo = g - u is dL/dv.  What the table makes dead is skipped: the
// levels above t_last, the last level that holds a free variable, have u = 0 exactly and contract nothing, phase 1 replays
// the units up to level t_last - 1 only (no layer step at all when every variable is pinned), and a chunk whose variables
// are all pinned skips its first-layer contraction when the caller takes no gdo.  Those branches depend on the tables and
// the gdo pointer alone.  Instantiated with and without pins: pin == NULL launches the kernel of gnf_strade_adjoint.
#include "gnf_strade.h"

namespace {

constexpr int kSmallFloats = 2 * 16 * kChunkVars;      // u and lambda of a chunk, [TB][kChunkVars] each

// the transposed images behind the forward image: layer l as [K[l]][ldt[l]], element [k][r] = the forward image's [r][k]
struct AdjLayout {
  MadeLayout lay;
  int ldt[kMaxH + 1];           // rows[l] rounded up to 16, the tail zero-filled
  int64_t t_off[kMaxH + 1];     // float offsets into the pack
  int64_t pack_floats;          // forward image + transposed images
  int gos;                      // floats per row of output cotangents, made odd like A
};

int make_adj_layout(const gnf_strade_net* net, int cond_in, AdjLayout* a) {
  const int rc = strade_layout(net, cond_in, &a->lay);
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
  StradePackArgs p;
  int ldt[kMaxH + 1];
  int64_t t_off[kMaxH + 1];
  int64_t pack_floats;
};

__global__ void strade_adjoint_pack_k(AdjPackArgs a, float* __restrict__ pack) {
  const MadeLayout& L = a.p.p.lay;
  for (int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; e < a.pack_floats; e += (int64_t)gridDim.x * blockDim.x) {
    float v = 0.f;
    if (e < L.pack_floats) {
      v = strade_pack_elem(a.p, e);            // the forward sweep's image, bit for bit: the replay reads what it read
    } else {
      int l = 0;
      while (l < L.nh && e >= a.t_off[l + 1]) ++l;
      const int64_t i = e - a.t_off[l];
      const int k = (int)(i / a.ldt[l]), r = (int)(i - (int64_t)k * a.ldt[l]);
      if (r < L.rows[l]) {
        const int64_t src = (int64_t)pack_src_row(a.p.p, l, r) * L.K[l] + pack_src_col(a.p.p, l, k);
        v = a.p.M[l][src] != 0.f ? a.p.p.W[l][src] : 0.f;
      }
    }
    pack[e] = v;
  }
}

struct AdjArgs {
  StepArgs s;
  const int32_t* var_off;
  int nlev;
  int ldt[kMaxH + 1];
  int64_t t_off[kMaxH + 1];
  int gos;
};

template <int TB, bool kLds, bool kPin>
__global__ __launch_bounds__(kThreads) void strade_adjoint_k(AdjArgs p, const float* __restrict__ pack,
                                                             const float* __restrict__ context, const float* __restrict__ x,
                                                             const float* __restrict__ g, const float* __restrict__ jac,
                                                             const float* __restrict__ dzdh, float* __restrict__ lam,
                                                             float* ws, int64_t B, const uint8_t* __restrict__ pin,
                                                             float* __restrict__ gdo) {
  extern __shared__ __attribute__((aligned(16))) float smem[];
  const StepArgs& s = p.s;
  const MadeLayout& L = s.lay;
  float* red = smem;
  float* ubuf = smem + kRedFloats;                                   // [TB][kChunkVars] u of the chunk
  float* lbuf = ubuf + 16 * kChunkVars;                              // [TB][kChunkVars] lambda of the chunk
  const int tid = threadIdx.x;
  const int64_t row0 = (int64_t)blockIdx.x * TB;
  const int nrows = (int)(B - row0 < TB ? B - row0 : TB);
  const int A = L.A, d = L.d, out = L.out, nh = L.nh, c = L.c, gos = p.gos, nlev = p.nlev;
  // [TB][A] activations, then cotangents | [TB][gos] output cotangents
  float* act = kLds ? smem + kRedFloats + kSmallFloats : ws + (size_t)row0 * (A + gos);
  float* go = act + (size_t)TB * A;
  // the last level that holds a free variable, -1 when every variable is pinned (the tables: uniform over the workgroup)
  int t_last = nlev - 1;
  if (kPin)
    for (; t_last >= 0; --t_last) {
      bool any_free = false;
      for (int q = p.var_off[t_last]; q < p.var_off[t_last + 1]; ++q) any_free |= pin[s.var_of_step[q]] == 0;
      if (any_free) break;
    }
  const int t_end = kPin ? t_last + 1 : nlev;  // phase 1 replays the units of level < t_end - 1

  // ---- phase 1: the hidden units of the sweep that produced x (strade_levels_k's loop without outputs and inverse)
  for (int i = tid; i < TB * A; i += kThreads) act[i] = 0.f;
  __syncthreads();
  // one float per load: the caller's rows are dword-aligned, no more
  for (int i = tid; i < nrows * c; i += kThreads) act[(size_t)(i / c) * A + i % c] = context[row0 * c + i];
  for (int i = tid; i < nrows * d; i += kThreads) act[(size_t)(i / d) * A + c + i % d] = x[(row0 + i / d) * d + s.var_of_step[i % d]];
  __syncthreads();
  for (int t = 0; t < t_end; ++t)
    for (int l = 0; l < nh; ++l) {
      const int n0 = t >= 1 ? s.off[l][t - 1] : 0, n1 = s.off[l][t];  // the units of level t - 1 (t = 0: the empty-set units)
      if (n1 == n0) continue;                                         // (uniform: the tables are the same for every lane)
      const int K = l == 0 ? c + p.var_off[t] : s.off[l - 1][t];
      layer_step<TB>(pack + L.w_off[l] + (size_t)n0 * L.ldw[l], L.ldw[l], L.rows[l] - n0, pack + L.b_off[l] + n0,
                     n1 - n0, K, act + (l == 0 ? 0 : L.act_off[l - 1]), A, act + L.act_off[l] + n0, A, true, nrows, red);
    }

  // ---- phase 2: the sweep
  const int KO = d * out;
  for (int t = nlev - 1; t >= 0; --t) {
    const int p0 = p.var_off[t], p1 = p.var_off[t + 1];               // the level's variables, positions in level order
    const bool live = !kPin || t <= t_last;                           // a level above the last free one contracts nothing
    for (int l = nh - 1; l >= 0; --l) {
      const int n0 = s.off[l][t], n1 = s.off[l][t + 1];               // the units of level t
      if (n1 == n0 || !live) continue;                                // (uniform)
      const bool last = l == nh - 1;
      suffix_step<TB>(pack + p.t_off[l + 1] + (size_t)n0 * p.ldt[l + 1], p.ldt[l + 1], L.rows[l] - n0, n1 - n0,
                      last ? p1 * out : s.off[l + 1][t], last ? KO : L.rows[l + 1],
                      last ? go : act + L.act_off[l + 1], last ? gos : A, act + L.act_off[l] + n0, A, true, nrows, red);
    }
    // u of the level's variables: columns c + p of the first layer against the cotangents of everything of level >= t
    const int k0 = nh == 0 ? p1 * out : s.off[0][t], K = nh == 0 ? KO : L.rows[0];
    for (int q0 = p0; q0 < p1; q0 += kChunkVars) {
      const int nv = p1 - q0 < kChunkVars ? p1 - q0 : kChunkVars;
      // this thread's (row, variable) of the chunk: nrows * nv <= 16 * 8 threads have one
      const bool mine = tid < nrows * nv;
      const int r = mine ? tid / nv : 0, j = mine ? tid % nv : 0;
      const int v = s.var_of_step[q0 + j];
      const bool pinned = kPin && pin[v] != 0;
      // a chunk of pinned variables needs its u for gdo alone (uniform: the table and the pointer)
      bool with_u = live;
      if (kPin && live && !gdo) {
        with_u = false;
        for (int jj = 0; jj < nv; ++jj) with_u |= pin[s.var_of_step[q0 + jj]] == 0;
      }
      // asked for before the product, which hides the latency (jac of a pinned element is not read: it may hold anything)
      const float gv = mine ? g[(row0 + r) * d + v] : 0.f;
      const float jv = mine && !pinned ? jac[(row0 + r) * d + v] : 1.f;
      if (with_u)
        suffix_step<TB>(pack + p.t_off[0] + (size_t)(c + q0) * p.ldt[0], p.ldt[0], d - q0, nv, k0, K,
                        nh == 0 ? go : act + L.act_off[0], nh == 0 ? gos : A, ubuf, kChunkVars, false, nrows, red);
      if (mine) {
        if (pinned) {
          lam[(row0 + r) * d + v] = 0.f;
          if (gdo) gdo[(row0 + r) * d + v] = live ? gv - ubuf[r * kChunkVars + j] : gv;
        } else {
          const float lv = (gv - ubuf[r * kChunkVars + j]) / jv;
          lam[(row0 + r) * d + v] = lv;
          lbuf[r * kChunkVars + j] = lv;
          if (kPin && gdo) gdo[(row0 + r) * d + v] = 0.f;
        }
      }
      __syncthreads();
      // the cotangents of these variables' outputs, read by the levels below (never by this level: its suffixes start at p1)
      if (t > 0) {
        const int64_t per_row = (int64_t)nv * out;
        for (int64_t i = tid; i < nrows * per_row; i += kThreads) {
          const int rr = (int)(i / per_row);
          const int64_t rem = i - rr * per_row;
          const int jj = (int)(rem / out), kk = (int)(rem - (int64_t)jj * out);
          const int vv = s.var_of_step[q0 + jj];
          // exact zeros for a pinned variable: its dzdh is not read
          go[(size_t)rr * gos + (size_t)(q0 + jj) * out + kk] =
              kPin && pin[vv] != 0 ? 0.f : lbuf[rr * kChunkVars + jj] * dzdh[((row0 + rr) * d + vv) * out + kk];
        }
      }
      __syncthreads();          // lbuf and ubuf are free for the next chunk; go is complete for the level below
    }
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
    e = lds ? gnf_launch_lds(strade_adjoint_k<TB, true, true>, gr, bl, smem, st, p, pack, context, x, g, jac, dzdh, lam, ws,
                             B, pin, gdo)
            : gnf_launch_lds(strade_adjoint_k<TB, false, true>, gr, bl, smem, st, p, pack, context, x, g, jac, dzdh, lam, ws,
                             B, pin, gdo);
  else
    e = lds ? gnf_launch_lds(strade_adjoint_k<TB, true, false>, gr, bl, smem, st, p, pack, context, x, g, jac, dzdh, lam, ws,
                             B, pin, gdo)
            : gnf_launch_lds(strade_adjoint_k<TB, false, false>, gr, bl, smem, st, p, pack, context, x, g, jac, dzdh, lam, ws,
                             B, pin, gdo);
  return e == hipSuccess ? 0 : (int)e;
}

}  // namespace

extern "C" {

int64_t gnf_strade_adjoint_pack_floats(const gnf_strade_net* net, int cond_in) {
  AdjLayout a;
  const int rc = make_adj_layout(net, cond_in, &a);
  return rc ? rc : a.pack_floats;
}

int gnf_strade_adjoint_pack(const gnf_strade_net* net, int cond_in, float* pack, gnf_stream_t stream) {
  AdjLayout lay;
  const int rc = make_adj_layout(net, cond_in, &lay);
  if (rc) return rc;
  if (!pack || ((uintptr_t)pack & 15)) return GNF_EINVAL;            // image rows are read as 16-byte quads
  AdjPackArgs a;
  a.p.p.lay = lay.lay;
  if (strade_fill_pack_args(net, &a.p)) return GNF_EINVAL;
  for (int l = 0; l <= net->made.nh; ++l) {
    a.ldt[l] = lay.ldt[l];
    a.t_off[l] = lay.t_off[l];
  }
  a.pack_floats = lay.pack_floats;
  const int64_t blocks = (a.pack_floats + 255) / 256;
  hipLaunchKernelGGL(strade_adjoint_pack_k, dim3((unsigned)(blocks < 4096 ? blocks : 4096)), dim3(256), 0,
                     (hipStream_t)stream, a, pack);
  GNF_LAUNCH_CHECK();
  return 0;
}

int64_t gnf_strade_adjoint_workspace_bytes(const gnf_strade_net* net, int cond_in, int64_t B) {
  AdjLayout a;
  const int rc = make_adj_layout(net, cond_in, &a);
  if (rc) return rc;
  if (B < 0) return GNF_EINVAL;
  return 4 * ws_floats(a, B);
}

}  // extern "C"

namespace {

int adjoint_run(const gnf_strade_net* net, int cond_in, const float* context, const float* pack, const float* x,
                const float* g, const float* jac, const float* dzdh, float* lambda, const uint8_t* pin, float* gdo, int64_t B,
                int force_ws, void* ws, int64_t ws_bytes, gnf_stream_t stream) {
  AdjLayout lay;
  const int rc = make_adj_layout(net, cond_in, &lay);
  if (rc) return rc;
  const gnf_made_net& m = net->made;
  if (B < 0) return GNF_EINVAL;
  if (gdo && !pin) return GNF_EINVAL;                                // dL/dv of no intervention
  if (B == 0) return 0;
  if (!pack || !x || !g || !jac || !dzdh || !lambda || !m.var_of_step || !net->var_off || (cond_in > 0 && !context))
    return GNF_EINVAL;
  if ((uintptr_t)pack & 15) return GNF_EINVAL;
  AdjArgs p;
  p.s.lay = lay.lay;
  for (int l = 0; l < m.nh; ++l) {
    if (!m.off[l]) return GNF_EINVAL;
    p.s.off[l] = m.off[l];
  }
  p.s.var_of_step = m.var_of_step;
  p.var_off = net->var_off;
  p.nlev = net->nlev;
  for (int l = 0; l <= m.nh; ++l) {
    p.ldt[l] = lay.ldt[l];
    p.t_off[l] = lay.t_off[l];
  }
  p.gos = lay.gos;
  // the forward sweep's tile height: the replay repeats its sums.  A net that sweep declines was inverted by passes, whose
  // summation order is none of this kernel's: 4 rows, the least LDS
  int hstride;
  int TB = strade_tile_rows(net, lay.lay, B, &hstride);
  if (!TB) TB = 4;
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

int gnf_strade_adjoint(const gnf_strade_net* net, int cond_in, const float* context, const float* pack, const float* x,
                       const float* g, const float* jac, const float* dzdh, float* lambda, int64_t B, int force_ws, void* ws,
                       int64_t ws_bytes, gnf_stream_t stream) {
  return adjoint_run(net, cond_in, context, pack, x, g, jac, dzdh, lambda, nullptr, nullptr, B, force_ws, ws, ws_bytes,
                     stream);
}

// ... and with a pin table (do(x_P = v)): pin == NULL is the call above
int gnf_strade_adjoint_do(const gnf_strade_net* net, int cond_in, const float* context, const float* pack, const float* x,
                          const float* g, const float* jac, const float* dzdh, float* lambda, const uint8_t* pin, float* gdo,
                          int64_t B, int force_ws, void* ws, int64_t ws_bytes, gnf_stream_t stream) {
  return adjoint_run(net, cond_in, context, pack, x, g, jac, dzdh, lambda, pin, gdo, B, force_ws, ws, ws_bytes, stream);
}

}  // extern "C"
