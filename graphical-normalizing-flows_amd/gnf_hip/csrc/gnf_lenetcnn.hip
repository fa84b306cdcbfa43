// LeNet convolutional front of CIFAR10CNN (models/MLP.py, reference :66-68) as the embedding net of a DAG conditioner:
//     feat = flatten(pool2(relu(conv_k(6 -> 16)(pool2(relu(conv_k(C -> 6)(e)))))))      on rows e [n, C*H*W]
// for the four geometries buildCIFAR10NormalizingFlow constructs, (C, H, W, k) = (3,32,32,5), (1,32,32,3), (1,16,16,3),
// (1,8,8,2): feature widths 400 / 576 / 64 / 16.  Pooling is floor pooling (13 -> 6, 7 -> 3, 5 -> 2 drop the last row and
// column; those conv outputs are never computed).  Everything between e and feat lives in LDS: no im2col, no map in HBM.
//
// gfx950 mapping.  One 256-thread workgroup walks over groups of IPB = 256 / P1^2 images (1 / 1 / 5 / 28): input, pooled
// conv1 map (and the backward's gradient maps) of a group sit in LDS, 17 KB forward and 56 KB backward at (3,32,32,5), so
// several workgroups share a CU and hide each other's barriers.
//   conv1 + ReLU + pool: a thread owns ONE pooled position, its 2 x 2 window for all 6 channels = 24 accumulators, and reads
//           the (k+1) x (k+1) patch of each input channel row by row from LDS;
//   conv2 + ReLU + pool: a wavefront owns 4 (8 at (1,32,32,3)) output channels, a lane one ROW of one 2 x 2 pool window
//           (2 positions), and the two rows of a window meet through one lane exchange;
//   the weights are read through wave-uniform addresses, i.e. scalar loads into SGPRs: they cost no LDS and no VGPR.
//
// Why plain VALU FMAs and not v_mfma_f32_16x16x4_f32.  The fp32 matrix pipe has the rate of the fp32 vector pipe on gfx950
// (64 FLOP / clk / SIMD, MI355X_MICROARCH), so MFMA can only save ISSUE slots and LDS traffic, not time per FLOP; with
// N = 6 output channels 10 of the 16 columns of a tile are padding (conv1 would run at 37 % of the pipe), and the im2col
// operand of a 16 x 16 x 4 step is 64 single LDS dwords per 1024 MACs.  The register-blocked direct form at (3,32,32,5):
//     conv1: 1800 v_fmac per thread (24 accumulators x 75 taps) against 108 LDS dwords (3 channels x 6 x 6 patch)  = 17 : 1
//     conv2: 1200 v_fmac per lane (2 positions x 4 channels x 150 taps) against 180 LDS dwords                     =  7 : 1
// and a CU retires 2 wave-FMAs per clock against one ds_read_b32 per 2 clocks, i.e. it needs >= 4 : 1 to stay on the ALU.
// 0.59 MMAC per image forward; lane utilisation 196 / 256 (conv1) and 50 / 64 (conv2).
//
// Decisions follow torch: the ReLU gate is `pre-activation > 0`, a pool window takes its FIRST maximum in row-major scan
// order (strict > when a later entry replaces an earlier one), always.
//
// Backward.  conv1 is recomputed (its pooled activations are the operand of dW2 and are needed in any case, and the
// recompute yields pool 1's argmax for free), conv2's pool decision (one byte per feature: 0..3 = window entry that carries
// the gradient, 4 = gated off) is either read from the plane the forward saved or recomputed when the caller passes NULL.
// A pooled gradient has ONE non-zero per 2 x 2 window, so the two weight gradients run over (value, offset) lists -- a quarter
// of the dense work -- while the two data gradients (da1, de) gather from the dense maps, bounds checked.  Weight gradients
// are accumulated in registers over all images of a workgroup, written once per workgroup to the caller's workspace and
// summed over workgroups in a fixed order by a second kernel: no float atomics, the same bits on every call.
//
// Gated variants (gnf_lenet_gated_*).  As the embedding net of a DAG conditioner the front receives the B*d masked copies
// e[b*d + i, :] = x[b, :] * gate(b, i, :): at d = 3072 that is 37.7 MB per sample written by the gate kernel, read here, kept
// for the backward, and the same again for its cotangent.  lenet_gated_fwd_k / lenet_gated_bwd_k build each copy in LDS
// from x [B, d], the gate's (i, j) table and the noise (the arithmetic of gnf_dag_gate.h, hence the same bits), and the
// backward multiplies dL/de by de/dp and sums over the samples in registers: neither e nor its cotangent exists in HBM.
// lenet_rows_fwd_k is the no-grad sibling for a deterministic gate: the rows i of a level of the inversion (or all d of them)
// as x[b, :] * P[i, :], the [B, R, d] broadcast product of DAGConditioner.forward_rows built in LDS.
// lenet_rows_fwd_arg_k / lenet_rows_bwd_k are its training form for a FROZEN gate (P a constant): the forward also keeps the
// second pool's decisions, the backward rebuilds each copy in LDS, skips dL/de altogether when x is data and otherwise
// sums dL/dx over the rows in registers (DetRowsSrc).
#include "gnf_dag_gate.h"

namespace {

constexpr int kThreads = 256;
constexpr int kFwdGridMax = 1024;     // 4 workgroups per CU
constexpr int kBwdGridMax = 512;      // 2 workgroups per CU (56 KB of LDS each at the largest geometry)

template <int C_, int H_, int K_>
struct Geo {
  static constexpr int C = C_, H = H_, W = H_, K = K_;
  static constexpr int HW = H * W, IMG = C * HW;
  static constexpr int H1 = H - K + 1;          // conv1 output side
  static constexpr int P1 = H1 / 2;             // pooled (floor)
  static constexpr int NP1 = P1 * P1;
  static constexpr int U1 = 2 * P1;             // conv1 outputs a pool window covers
  static constexpr int H2 = P1 - K + 1;         // conv2 output side
  static constexpr int P2 = H2 / 2;
  static constexpr int NP2 = P2 * P2;
  static constexpr int U2 = 2 * P2;
  static constexpr int F = 16 * NP2;            // feature width
  static constexpr int T1 = C * K * K;          // taps of one conv1 output channel
  static constexpr int T2 = 6 * K * K;
  static constexpr int IPB = kThreads / NP1;    // images of one group
  static constexpr int S2 = IPB * NP2 * 2;      // conv2 lanes: (image, window, window row)
  static constexpr int WPG = (S2 + 63) / 64;    // wavefronts that share a channel group
  static constexpr int CG = 4 * WPG;            // channels of a wavefront
  static constexpr int R2 = (T2 + 63) / 64;     // dW2: rounds of 64 taps
  static constexpr int J1 = (6 * T1 + kThreads - 1) / kThreads;   // dW1: entries per thread
  static constexpr int PW = 6 * T1 + 6 + 16 * T2 + 16;            // floats of one workgroup's partial gradients
  static_assert(IPB >= 1 && (WPG == 1 || WPG == 2) && P2 >= 1, "geometry");
};

struct float2i { float v; int off; };   // a gradient and the offset of the window entry it belongs to

// The weights reach the FMAs as SGPR operands through scalar loads.  Left alone, instruction selection emits every invariant
// load of a 3000-FMA block first: several hundred SGPRs, spilled into VGPR lanes and on to scratch.  So the weights are
// walked in memory order in STAGES of GS groups of KK contiguous floats, double buffered by hand: the loads of stage st + 1
// are issued, then -- between two scheduling barriers -- stage st is consumed.  body(g, w, z) applies group g's KK weights
// and ties every accumulator it has updated to `z` with an empty volatile asm (tie()); z is the zero the loads of stage st + 2
// add to their address, which is what keeps them BEHIND the arithmetic of stage st -- and the arithmetic in its stage.
__device__ __forceinline__ void tie(int& z, float& a) { asm volatile("" : "+s"(z), "+v"(a)); }
__device__ __forceinline__ void tie(int& z, float& a, float& b) { asm volatile("" : "+s"(z), "+v"(a), "+v"(b)); }
__device__ __forceinline__ void tie(int& z, float& a, float& b, float& c, float& d) {
  asm volatile("" : "+s"(z), "+v"(a), "+v"(b), "+v"(c), "+v"(d));
}

template <int K>
struct Stage { static constexpr int GS = K >= 5 ? 1 : (K == 3 ? 3 : 6); };

template <int NG, int KK, int GS_, class Addr, class Body>
__device__ __forceinline__ void staged_weights(Addr addr, Body body) {
  constexpr int GS = GS_ < NG ? GS_ : NG;
  constexpr int NS = (NG + GS - 1) / GS;
  float w[2][GS * KK];
  int z = opaque_s(0);
  auto load = [&](int st, float* dst) {
#pragma unroll
    for (int q = 0; q < GS; ++q)
      if (st * GS + q < NG) {
        const float* p = addr(st * GS + q) + z;
#pragma unroll
        for (int t = 0; t < KK; ++t) dst[q * KK + t] = p[t];
      }
  };
  load(0, w[0]);
#pragma unroll
  for (int st = 0; st < NS; ++st) {
    if (st + 1 < NS) load(st + 1, w[(st + 1) & 1]);
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int q = 0; q < GS; ++q)
      if (st * GS + q < NG) {
        body(st * GS + q, &w[st & 1][q * KK], z);
      }
    __builtin_amdgcn_sched_barrier(0);
  }
}

// ---------------------------------------------------------------------------------------------------------- forward phases
// conv1 + bias + ReLU + pool of the group's images in xs -> a1s [IPB][6][P1][P1]; arg1s (LDS, may be null): 0..3 = the window
// entry that carries the gradient, 4 = the pooled value is 0 (every entry gated off)
template <class G>
__device__ __forceinline__ void conv1_phase(const float* xs, float* a1s, unsigned char* arg1s, const float* __restrict__ W1,
                                            const float* __restrict__ b1, int tid) {
  const int s = tid / G::NP1, p = tid % G::NP1;
  if (s >= G::IPB) return;
  const int py = p / G::P1, px = p % G::P1;
  const float* xb = xs + s * G::IMG + 2 * py * G::W + 2 * px;
  float acc[2][2][6];
#pragma unroll
  for (int o = 0; o < 6; ++o) acc[0][0][o] = acc[0][1][o] = acc[1][0][o] = acc[1][1][o] = b1[o];
  float v[G::K + 1][G::K + 1];
  staged_weights<6 * G::C, G::K * G::K, Stage<G::K>::GS>(
      [&](int g) { return W1 + ((g % 6) * G::C + g / 6) * G::K * G::K; },     // group g = (c, o), c outer
      [&](int g, const float* w, int& z) {
        const int c = g / 6, o = g % 6;
        if (o == 0) {
#pragma unroll
          for (int r = 0; r <= G::K; ++r)
#pragma unroll
            for (int j = 0; j <= G::K; ++j) v[r][j] = xb[c * G::HW + r * G::W + j];
        }
#pragma unroll
        for (int ky = 0; ky < G::K; ++ky)
#pragma unroll
          for (int kx = 0; kx < G::K; ++kx) {
            const float wk = w[ky * G::K + kx];
            acc[0][0][o] = fmaf(v[ky][kx], wk, acc[0][0][o]);
            acc[0][1][o] = fmaf(v[ky][kx + 1], wk, acc[0][1][o]);
            acc[1][0][o] = fmaf(v[ky + 1][kx], wk, acc[1][0][o]);
            acc[1][1][o] = fmaf(v[ky + 1][kx + 1], wk, acc[1][1][o]);
          }
        tie(z, acc[0][0][o], acc[0][1][o], acc[1][0][o], acc[1][1][o]);
      });
#pragma unroll
  for (int o = 0; o < 6; ++o) {
    float m = fmaxf(acc[0][0][o], 0.f);
    int idx = 0;
    float t = fmaxf(acc[0][1][o], 0.f);
    if (t > m) { m = t; idx = 1; }
    t = fmaxf(acc[1][0][o], 0.f);
    if (t > m) { m = t; idx = 2; }
    t = fmaxf(acc[1][1][o], 0.f);
    if (t > m) { m = t; idx = 3; }
    a1s[(s * 6 + o) * G::NP1 + p] = m;
    if (arg1s) arg1s[(s * 6 + o) * G::NP1 + p] = (unsigned char)(m > 0.f ? idx : 4);
  }
}

// conv2 + bias + ReLU + pool of a1s; emit(s, channel, window, pooled value, code) once per feature.  No barrier inside;
// every lane runs the exchange (an idle lane works on slot 0 and emits nothing).
template <class G, class Emit>
__device__ __forceinline__ void conv2_phase(const float* a1s, const float* __restrict__ W2, const float* __restrict__ b2,
                                            int tid, Emit emit) {
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6), lane = tid & 63;
  const int g = wave / G::WPG;                                   // wave-uniform: the weights go through scalar loads
  const int q = (wave % G::WPG) * 64 + lane;
  const bool active = q < G::S2;
  const int qq = active ? q : 0;
  const int s = qq / (2 * G::NP2), rem = qq % (2 * G::NP2), cell = rem >> 1, dy = rem & 1;
  const int cy = cell / G::P2, cx = cell % G::P2;
  const float* ab = a1s + s * 6 * G::NP1 + (2 * cy + dy) * G::P1 + 2 * cx;
  const float* wg = W2 + g * G::CG * G::T2;
  float acc[2][G::CG];
#pragma unroll
  for (int j = 0; j < G::CG; ++j) acc[0][j] = acc[1][j] = b2[g * G::CG + j];
  float v[G::K][G::K + 1];
  staged_weights<6 * G::CG, G::K * G::K, Stage<G::K>::GS>(
      [&](int gq) { return wg + ((gq % G::CG) * 6 + gq / G::CG) * G::K * G::K; },   // group = (ci, j), ci outer
      [&](int gq, const float* w, int& z) {
        const int ci = gq / G::CG, j = gq % G::CG;
        if (j == 0) {
#pragma unroll
          for (int ky = 0; ky < G::K; ++ky)
#pragma unroll
            for (int i = 0; i <= G::K; ++i) v[ky][i] = ab[ci * G::NP1 + ky * G::P1 + i];
        }
#pragma unroll
        for (int ky = 0; ky < G::K; ++ky)
#pragma unroll
          for (int kx = 0; kx < G::K; ++kx) {
            const float wk = w[ky * G::K + kx];
            acc[0][j] = fmaf(v[ky][kx], wk, acc[0][j]);
            acc[1][j] = fmaf(v[ky][kx + 1], wk, acc[1][j]);
          }
        tie(z, acc[0][j], acc[1][j]);
      });
#pragma unroll
  for (int j = 0; j < G::CG; ++j) {
    float m = fmaxf(acc[0][j], 0.f);
    int idx = 2 * dy;
    const float t = fmaxf(acc[1][j], 0.f);
    if (t > m) { m = t; idx = 2 * dy + 1; }
    const float mo = __shfl_xor(m, 1, GNF_WAVE);                 // the window's other row: lanes 2i (row 0) and 2i + 1
    const int io = __shfl_xor(idx, 1, GNF_WAVE);
    if (active && dy == 0) {
      if (mo > m) { m = mo; idx = io; }                          // row 0 keeps a tie: first maximum in scan order
      emit(s, g * G::CG + j, cell, m, m > 0.f ? idx : 4);
    }
  }
}

// the group's inputs -> xs (zeros for the images past the end)
template <class G>
__device__ __forceinline__ void stage_inputs(float* xs, const float* __restrict__ e, int64_t ld_e, int64_t i0, int64_t n,
                                             int tid) {
  for (int i = tid; i < G::IPB * G::IMG; i += kThreads) {
    const int s = i / G::IMG, r = i % G::IMG;
    const int64_t im = i0 + s;
    xs[i] = im < n ? e[im * ld_e + r] : 0.f;
  }
}

template <class G>
__global__ __launch_bounds__(kThreads, 4) void lenet_fwd_k(const float* __restrict__ e, int64_t ld_e,
                                                        const float* __restrict__ W1, const float* __restrict__ b1,
                                                        const float* __restrict__ W2, const float* __restrict__ b2,
                                                        float* __restrict__ feat, unsigned char* __restrict__ arg2,
                                                        int64_t n) {
  __shared__ float xs[G::IPB * G::IMG];
  __shared__ float a1s[G::IPB * 6 * G::NP1];
  const int tid = threadIdx.x;
  for (int64_t i0 = (int64_t)blockIdx.x * G::IPB; i0 < n; i0 += (int64_t)gridDim.x * G::IPB) {
    stage_inputs<G>(xs, e, ld_e, i0, n, tid);
    __syncthreads();
    conv1_phase<G>(xs, a1s, nullptr, W1, b1, tid);
    __syncthreads();
    conv2_phase<G>(a1s, W2, b2, tid, [&](int s, int ch, int cell, float m, int code) {
      const int64_t im = i0 + s;
      if (im < n) {
        feat[im * G::F + ch * G::NP2 + cell] = m;
        if (arg2) arg2[im * G::F + ch * G::NP2 + cell] = (unsigned char)code;
      }
    });
    __syncthreads();
  }
}

// ------------------------------------------------------------------------------------------- masked copies built in LDS
// The gate of a DAG conditioner fused into the front: image (b, i) of the batch is the masked copy
// x[b, :] * gate(b, i, :) (gnf_dag_gate.h), built where stage_inputs would have loaded it.  d = G::IMG.
struct GatedArgs {
  const float* x; const float* tab; const float* u1; const float* u2;
  uint64_t seed, offset; int gate_mode; float T; int64_t B;
  float* dp; int64_t gpc, nchunk;          // backward: [nchunk, d, d] sums of dL/dP, groups per chunk of samples
};

// xs[s] = the masked copy (b0 + s, i), zeros for the samples past the end; fs (may be null) = its derivative de/dp.
// One thread per column quad, as in dag_gate_fwd_k: one Philox call serves four pixels.
template <class G>
__device__ __forceinline__ void stage_gated(float* xs, float* fs, const GatedArgs& a, int64_t i, int64_t b0, int tid) {
  constexpr int64_t d = G::IMG, dd = d * d;
  constexpr int DQ = G::IMG / 4;
  static_assert(G::IMG % 4 == 0, "whole column quads");
  const bool vt = quad_aligned(a.tab, d), vx = quad_aligned(a.x, d);
  for (int q = tid; q < G::IPB * DQ; q += kThreads) {
    const int s = q / DQ, jq = q % DQ;
    const int64_t b = b0 + s;
    float out[4] = {0.f, 0.f, 0.f, 0.f}, f[4] = {0.f, 0.f, 0.f, 0.f};
    if (b < a.B) {
      float p4[4], et4[4] = {0.f, 0.f, 0.f, 0.f}, q4[4] = {0.f, 0.f, 0.f, 0.f}, x4[4];
      load4(a.tab + i * d + 4 * jq, 4, vt, p4);
      if (a.gate_mode == 1) load4(a.tab + 2 * dd + i * d + 4 * jq, 4, vt, et4);
      if (a.gate_mode == 1 && fs) load4(a.tab + 3 * dd + i * d + 4 * jq, 4, vt, q4);
      const Draw4 n = draw4(a.gate_mode, a.u1, a.u2, a.seed, a.offset, b * d + i, jq, d);
      load4(a.x + b * d + 4 * jq, 4, vx, x4);
#pragma unroll
      for (int h = 0; h < 4; ++h) {
        out[h] = gate_copy(a.gate_mode, x4[h], p4[h], et4[h], n.v[h], n.w[h], a.T);
        if (fs) f[h] = gate_dp_add(a.gate_mode, 1.f, x4[h], p4[h], et4[h], q4[h], n.v[h], n.w[h], a.T, 0.f);
      }
    }
    *reinterpret_cast<float4*>(xs + s * G::IMG + 4 * jq) = make_float4(out[0], out[1], out[2], out[3]);
    if (fs) *reinterpret_cast<float4*>(fs + s * G::IMG + 4 * jq) = make_float4(f[0], f[1], f[2], f[3]);
  }
}

// feature rows stay in the order b*d + i; a unit of work is (row i, group of IPB samples)
template <class G>
__global__ __launch_bounds__(kThreads, 4) void lenet_gated_fwd_k(GatedArgs a, const float* __restrict__ W1,
                                                              const float* __restrict__ b1, const float* __restrict__ W2,
                                                              const float* __restrict__ b2, float* __restrict__ feat,
                                                              unsigned char* __restrict__ arg2) {
  __shared__ __attribute__((aligned(16))) float xs[G::IPB * G::IMG];
  __shared__ float a1s[G::IPB * 6 * G::NP1];
  const int tid = threadIdx.x;
  const int64_t ngb = (a.B + G::IPB - 1) / G::IPB;
  for (int64_t u = blockIdx.x; u < G::IMG * ngb; u += gridDim.x) {
    const int64_t i = u / ngb, b0 = (u % ngb) * G::IPB;
    stage_gated<G>(xs, nullptr, a, i, b0, tid);
    __syncthreads();
    conv1_phase<G>(xs, a1s, nullptr, W1, b1, tid);
    __syncthreads();
    conv2_phase<G>(a1s, W2, b2, tid, [&](int s, int ch, int cell, float m, int code) {
      if (b0 + s < a.B) {
        const int64_t im = (b0 + s) * G::IMG + i;
        feat[im * G::F + ch * G::NP2 + cell] = m;
        if (arg2) arg2[im * G::F + ch * G::NP2 + cell] = (unsigned char)code;
      }
    });
    __syncthreads();
  }
}

// ------------------------------------------------------------------------- a subset of the deterministic gate's rows
// Inversion and deterministic evaluation ask for the rows i of an importance matrix P [d, d] (pitch ld_p): image (b, r) is
// x[b, :] * P[i, :], i = rows ? rows[r] : r -- the [B, R, d] tensor torch would broadcast, built in LDS instead.
// xs[s] = that copy of sample b0 + s, zeros for the samples past the end.  One thread per column quad, as stage_gated.
template <class G>
__device__ __forceinline__ void stage_rows(float* xs, const float* __restrict__ x, const float* __restrict__ P, int64_t ld_p,
                                           int64_t i, int64_t b0, int64_t B, int tid) {
  constexpr int64_t d = G::IMG;
  constexpr int DQ = G::IMG / 4;
  static_assert(G::IMG % 4 == 0, "whole column quads");
  const bool vp = quad_aligned(P, ld_p), vx = quad_aligned(x, d);
  for (int q = tid; q < G::IPB * DQ; q += kThreads) {
    const int s = q / DQ, jq = q % DQ;
    const int64_t b = b0 + s;
    float out[4] = {0.f, 0.f, 0.f, 0.f};
    if (b < B) {
      float p4[4], x4[4];
      load4(P + i * ld_p + 4 * jq, 4, vp, p4);
      load4(x + b * d + 4 * jq, 4, vx, x4);
#pragma unroll
      for (int h = 0; h < 4; ++h) out[h] = gate_copy(0, x4[h], p4[h], 0.f, 0.f, 1.f, 1.f);   // one fp32 product
    }
    *reinterpret_cast<float4*>(xs + s * G::IMG + 4 * jq) = make_float4(out[0], out[1], out[2], out[3]);
  }
}

// a unit of work is (row slot r, group of IPB samples), r-major: consecutive units reuse one row of P.  Feature row of
// (b, r): b*R + r, or r*B + b when variable_major.  SAVE: the training form, which also writes the second pool's decisions
// to arg2 (same row order as feat) for lenet_rows_bwd_k
template <class G, bool SAVE>
__device__ __forceinline__ void rows_fwd_body(const float* __restrict__ x, const float* __restrict__ P, int64_t ld_p,
                                              const int32_t* __restrict__ rows, int64_t R, int64_t B,
                                              const float* __restrict__ W1, const float* __restrict__ b1,
                                              const float* __restrict__ W2, const float* __restrict__ b2,
                                              float* __restrict__ feat, unsigned char* __restrict__ arg2,
                                              int variable_major) {
  __shared__ __attribute__((aligned(16))) float xs[G::IPB * G::IMG];
  __shared__ float a1s[G::IPB * 6 * G::NP1];
  const int tid = threadIdx.x;
  const int64_t ngb = (B + G::IPB - 1) / G::IPB;
  for (int64_t u = blockIdx.x; u < R * ngb; u += gridDim.x) {
    const int64_t r = u / ngb, b0 = (u % ngb) * G::IPB;
    const int64_t i = rows ? (int64_t)rows[r] : r;
    stage_rows<G>(xs, x, P, ld_p, i, b0, B, tid);
    __syncthreads();
    conv1_phase<G>(xs, a1s, nullptr, W1, b1, tid);
    __syncthreads();
    conv2_phase<G>(a1s, W2, b2, tid, [&](int s, int ch, int cell, float m, int code) {
      const int64_t b = b0 + s;
      if (b < B) {
        const int64_t im = variable_major ? r * B + b : b * R + r;
        feat[im * G::F + ch * G::NP2 + cell] = m;
        if (SAVE) arg2[im * G::F + ch * G::NP2 + cell] = (unsigned char)code;
      }
    });
    __syncthreads();
  }
}

template <class G>
__global__ __launch_bounds__(kThreads, 4) void lenet_rows_fwd_k(const float* __restrict__ x, const float* __restrict__ P,
                                                             int64_t ld_p, const int32_t* __restrict__ rows, int64_t R,
                                                             int64_t B, const float* __restrict__ W1,
                                                             const float* __restrict__ b1, const float* __restrict__ W2,
                                                             const float* __restrict__ b2, float* __restrict__ feat,
                                                             int variable_major) {
  rows_fwd_body<G, false>(x, P, ld_p, rows, R, B, W1, b1, W2, b2, feat, nullptr, variable_major);
}

template <class G>
__global__ __launch_bounds__(kThreads, 4) void lenet_rows_fwd_arg_k(const float* __restrict__ x, const float* __restrict__ P,
                                                                 int64_t ld_p, const int32_t* __restrict__ rows, int64_t R,
                                                                 int64_t B, const float* __restrict__ W1,
                                                                 const float* __restrict__ b1, const float* __restrict__ W2,
                                                                 const float* __restrict__ b2, float* __restrict__ feat,
                                                                 unsigned char* __restrict__ arg2, int variable_major) {
  rows_fwd_body<G, true>(x, P, ld_p, rows, R, B, W1, b1, W2, b2, feat, arg2, variable_major);
}

// --------------------------------------------------------------------------------------------------------------- backward
// de[c][Y][X] = sum_{o, ky, kx} dpre1[o][Y - ky][X - kx] W1[o][c][ky][kx] of one image (db = its dense dpre1 maps)
template <class G>
__device__ __forceinline__ void de_pixel(const float* db, const float* __restrict__ W1, int Y, int X, float (&acc)[G::C]) {
#pragma unroll
  for (int c = 0; c < G::C; ++c) acc[c] = 0.f;
#pragma unroll 1
  for (int o = 0; o < 6; ++o) {
    const float* wo = W1 + o * G::T1;
    const float* dd = db + o * G::U1 * G::U1;
    float d[G::K * G::K];
#pragma unroll
    for (int ky = 0; ky < G::K; ++ky)
#pragma unroll
      for (int kx = 0; kx < G::K; ++kx) {
        const int yy = Y - ky, xx = X - kx;
        const bool valid = (unsigned)yy < (unsigned)G::U1 && (unsigned)xx < (unsigned)G::U1;
        d[ky * G::K + kx] = valid ? dd[valid ? yy * G::U1 + xx : 0] : 0.f;
      }
    staged_weights<G::C, G::K * G::K, Stage<G::K>::GS>([&](int c) { return wo + c * G::K * G::K; },
                                                       [&](int c, const float* w, int& z) {
#pragma unroll
                                                         for (int t = 0; t < G::K * G::K; ++t)
                                                           acc[c] = fmaf(d[t], w[t], acc[c]);
                                                         tie(z, acc[c]);
                                                       });
  }
}

// Where the images of the backward come from and where dL/de goes.  A source has
//   for_each_group(f): f(g) for every group of IPB images of this workgroup;   stage(xs, g, tid): the group's images -> xs;
//   row(g, s): the feature row of image s of group g, -1 past the end;   de_phase(d1, W1, g, tid): consumes dL/de.
// RowsSrc: rows of e in HBM, dL/de written to ge (when not null).
template <class G>
struct RowsSrc {
  const float* __restrict__ e; int64_t ld_e; float* __restrict__ ge; int64_t ld_ge; int64_t n;
  template <class F>
  __device__ __forceinline__ void for_each_group(F f) {
    for (int64_t i0 = (int64_t)blockIdx.x * G::IPB; i0 < n; i0 += (int64_t)gridDim.x * G::IPB) f(i0);
  }
  __device__ __forceinline__ void stage(float* xs, int64_t i0, int tid) { stage_inputs<G>(xs, e, ld_e, i0, n, tid); }
  __device__ __forceinline__ int64_t row(int64_t i0, int s) const { return i0 + s < n ? i0 + s : -1; }
  __device__ __forceinline__ void de_phase(const float* d1, const float* __restrict__ W1, int64_t i0, int tid) {
    if (!ge) return;
    for (int i = tid; i < G::IPB * G::HW; i += kThreads) {
      const int s = i / G::HW, r = i % G::HW;
      float acc[G::C];
      de_pixel<G>(d1 + s * 6 * G::U1 * G::U1, W1, r / G::W, r % G::W, acc);
      const int64_t im = i0 + s;
      if (im < n)
#pragma unroll
        for (int c = 0; c < G::C; ++c) ge[im * ld_ge + c * G::HW + r] = acc[c];
    }
  }
};

// GatedSrc: masked copies built in LDS; dL/de is never stored.  A unit of work is (row i of A, chunk of samples) walked
// in groups of IPB samples of that row; every dL/de[b,i,j] is multiplied by de/dp[b,i,j] (fs, staged with the copy)
// and summed over the unit's samples in registers, a thread owning the same pixels in every group; the unit writes row i
// of chunk ch of a.dp.  When HW < 256 the SPI = 256 / HW threads that share a pixel meet through LDS in a fixed order.
template <class G>
struct GatedSrc {
  static constexpr int NPT = G::HW >= kThreads ? G::HW / kThreads : 1;     // pixels of a thread
  static constexpr int SPI = G::HW >= kThreads ? 1 : kThreads / G::HW;     // samples of one pass over the threads
  static_assert(G::HW >= kThreads ? G::HW % kThreads == 0
                                    : (kThreads % G::HW == 0 && G::IPB % SPI == 0 && G::IPB * G::IMG >= kThreads),
                "pixel ownership");
  struct Group { int64_t i, b0; };
  GatedArgs a;
  float* fs;                                                               // LDS [IPB][IMG]
  float acc_dp[NPT][G::C];

  template <class F>
  __device__ __forceinline__ void for_each_group(F f) {
    const int64_t ngb = (a.B + G::IPB - 1) / G::IPB;
    for (int64_t u = blockIdx.x; u < G::IMG * a.nchunk; u += gridDim.x) {
      const int64_t i = u / a.nchunk, ch = u % a.nchunk;
#pragma unroll
      for (int t = 0; t < NPT; ++t)
#pragma unroll
        for (int c = 0; c < G::C; ++c) acc_dp[t][c] = 0.f;
      const int64_t g1 = (ch + 1) * a.gpc < ngb ? (ch + 1) * a.gpc : ngb;
      for (int64_t gb = ch * a.gpc; gb < g1; ++gb) f(Group{i, gb * G::IPB});
      if (a.dp) flush(a.dp + (ch * G::IMG + i) * G::IMG, threadIdx.x);
    }
  }
  __device__ __forceinline__ void stage(float* xs, Group g, int tid) {
    stage_gated<G>(xs, a.dp ? fs : nullptr, a, g.i, g.b0, tid);
  }
  __device__ __forceinline__ int64_t row(Group g, int s) const {
    return g.b0 + s < a.B ? (g.b0 + s) * G::IMG + g.i : -1;
  }
  __device__ __forceinline__ void de_phase(const float* d1, const float* __restrict__ W1, Group, int tid) {
    if (!a.dp) return;
#pragma unroll 1
    for (int sb = 0; sb < G::IPB; sb += SPI)
#pragma unroll
      for (int t = 0; t < NPT; ++t) {
        const int s = SPI == 1 ? sb : sb + tid / G::HW, r = SPI == 1 ? t * kThreads + tid : tid % G::HW;
        float acc[G::C];
        de_pixel<G>(d1 + s * 6 * G::U1 * G::U1, W1, r / G::W, r % G::W, acc);
#pragma unroll
        for (int c = 0; c < G::C; ++c) acc_dp[t][c] = fmaf(acc[c], fs[s * G::IMG + c * G::HW + r], acc_dp[t][c]);
      }
  }
  // the unit's sums -> out[d]; called after the barrier that ends the unit's last group, so fs is free
  __device__ __forceinline__ void flush(float* out, int tid) {
    if (SPI == 1) {
#pragma unroll
      for (int t = 0; t < NPT; ++t)
#pragma unroll
        for (int c = 0; c < G::C; ++c) out[c * G::HW + t * kThreads + tid] = acc_dp[t][c];
    } else {
#pragma unroll
      for (int c = 0; c < G::C; ++c) {
        fs[tid] = acc_dp[0][c];
        __syncthreads();
        if (tid < G::HW) {
          float v = fs[tid];
#pragma unroll
          for (int k = 1; k < SPI; ++k) v += fs[tid + k * G::HW];
          out[c * G::HW + tid] = v;
        }
        __syncthreads();
      }
    }
  }
};

// DetRowsSrc: the copies x[b] * P[rows[r]] of a FROZEN deterministic gate built in LDS (stage_rows): no noise, no de/dp
// plane, no dL/dP.  A unit of work is (chunk ch of a.rpc whole rows, group of IPB samples), chunk-major so that the
// workgroups of one wave of the grid read the same rows of P.
//   WANT_DX = false (x is data): the host sets rpc = 1, i.e. the r-major units of lenet_rows_fwd_k; de_phase is empty.
//   WANT_DX = true: dL/dx[b, j] = sum_r P[rows[r], j] dL/de[b, r, j].  A thread owns the same (sample slot, pixel) set in
//     every row of the chunk -- NPASS x NPT x C accumulators, 12 at (3,32,32,5), 7 at (1,8,8,2) -- and adds dL/de * P in
//     registers; P[i, pixel] is read again from L2 (one row, 12 KB at d = 3072: no second LDS plane), and a pixel whose P
//     entries are all zero -- most of them once post_process() has left a 0/1 DAG -- skips its W1^T dpre1 gather.  The unit
//     writes its sums to plane ch of a.dxp [nchunk][B][d]; every (ch, b, j) has exactly one writer, and lenet_rows_dx_k
//     adds the planes in chunk order.
struct RowsArgs {
  const float* x; const float* P; int64_t ld_p; const int32_t* rows; int64_t R, B; int variable_major;
  float* dxp; int64_t rpc, nchunk;         // backward: [nchunk, B, d] sums of dL/dx, rows per chunk
};

template <class G, bool WANT_DX>
struct DetRowsSrc {
  static constexpr int NPT = GatedSrc<G>::NPT, SPI = GatedSrc<G>::SPI;     // the pixel ownership of GatedSrc
  static constexpr int NPASS = G::IPB / SPI;                               // passes over the group's samples
  struct Group { int64_t r, i, b0; };
  RowsArgs a;
  float acc_dx[WANT_DX ? NPASS : 1][NPT][G::C];

  template <class F>
  __device__ __forceinline__ void for_each_group(F f) {
    const int64_t ngb = (a.B + G::IPB - 1) / G::IPB;
    for (int64_t u = blockIdx.x; u < a.nchunk * ngb; u += gridDim.x) {
      const int64_t ch = u / ngb, b0 = (u % ngb) * G::IPB;
      if (WANT_DX) {
#pragma unroll
        for (int ps = 0; ps < NPASS; ++ps)
#pragma unroll
          for (int t = 0; t < NPT; ++t)
#pragma unroll
            for (int c = 0; c < G::C; ++c) acc_dx[ps][t][c] = 0.f;
      }
      const int64_t r1 = (ch + 1) * a.rpc < a.R ? (ch + 1) * a.rpc : a.R;
      for (int64_t r = ch * a.rpc; r < r1; ++r) f(Group{r, a.rows ? (int64_t)a.rows[r] : r, b0});
      if (WANT_DX) flush(a.dxp + ch * a.B * G::IMG, b0, threadIdx.x);
    }
  }
  __device__ __forceinline__ void stage(float* xs, Group g, int tid) {
    stage_rows<G>(xs, a.x, a.P, a.ld_p, g.i, g.b0, a.B, tid);
  }
  __device__ __forceinline__ int64_t row(Group g, int s) const {
    const int64_t b = g.b0 + s;
    return b < a.B ? (a.variable_major ? g.r * a.B + b : b * a.R + g.r) : -1;
  }
  __device__ __forceinline__ void de_phase(const float* d1, const float* __restrict__ W1, Group g, int tid) {
    if (!WANT_DX) return;
    const float* __restrict__ pr = a.P + g.i * a.ld_p;
#pragma unroll
    for (int ps = 0; ps < NPASS; ++ps)
#pragma unroll
      for (int t = 0; t < NPT; ++t) {
        const int s = SPI == 1 ? ps : ps * SPI + tid / G::HW, r = SPI == 1 ? t * kThreads + tid : tid % G::HW;
        float p[G::C];
        bool any = false;
#pragma unroll
        for (int c = 0; c < G::C; ++c) {
          p[c] = pr[c * G::HW + r];
          any = any || p[c] != 0.f;
        }
        if (any && g.b0 + s < a.B) {
          float acc[G::C];
          de_pixel<G>(d1 + s * 6 * G::U1 * G::U1, W1, r / G::W, r % G::W, acc);
#pragma unroll
          for (int c = 0; c < G::C; ++c) acc_dx[ps][t][c] = fmaf(acc[c], p[c], acc_dx[ps][t][c]);
        }
      }
  }
  // the unit's sums -> rows b0 .. b0 + IPB - 1 of one chunk's plane out [B][d]
  __device__ __forceinline__ void flush(float* out, int64_t b0, int tid) {
#pragma unroll
    for (int ps = 0; ps < NPASS; ++ps)
#pragma unroll
      for (int t = 0; t < NPT; ++t) {
        const int s = SPI == 1 ? ps : ps * SPI + tid / G::HW, r = SPI == 1 ? t * kThreads + tid : tid % G::HW;
        if (b0 + s < a.B)
#pragma unroll
          for (int c = 0; c < G::C; ++c) out[(b0 + s) * G::IMG + c * G::HW + r] = acc_dx[ps][t][c];
      }
  }
};

template <class G, bool RECOMPUTE, class Src>
__device__ __forceinline__ void lenet_bwd_body(Src& src, float* xs, const float* __restrict__ W1,
                                               const float* __restrict__ b1, const float* __restrict__ W2,
                                               const float* __restrict__ b2, const unsigned char* __restrict__ arg2,
                                               const float* __restrict__ g_feat, float* __restrict__ part) {
  __shared__ float a1s[G::IPB * 6 * G::NP1];
  __shared__ float d2[G::IPB * 16 * G::U2 * G::U2];      // dL/d(conv2 pre-activation), dense
  __shared__ float2i l2[G::IPB * G::F];                  // ... as one (value, a1 offset of the entry) per window
  __shared__ float d1[G::IPB * 6 * G::U1 * G::U1];       // dL/d(conv1 pre-activation), dense
  __shared__ float2i l1[G::IPB * 6 * G::NP1];            // ... as one (value, input offset of the entry) per window
  __shared__ unsigned char arg1s[G::IPB * 6 * G::NP1];
  __shared__ unsigned char arg2s[RECOMPUTE ? G::IPB * G::F : 1];
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);

  // dW2 / db2: wavefront `wave` owns the channels 4 wave .. 4 wave + 3, a lane the taps lane + 64 rr
  float accW2[4][G::R2], accb2[4];
  int abase[G::R2];
#pragma unroll
  for (int rr = 0; rr < G::R2; ++rr) {
    const int tap = lane + 64 * rr < G::T2 ? lane + 64 * rr : 0;
    const int ci = tap / (G::K * G::K), kk = tap % (G::K * G::K);
    abase[rr] = ci * G::NP1 + (kk / G::K) * G::P1 + kk % G::K;
  }
#pragma unroll
  for (int jj = 0; jj < 4; ++jj) {
    accb2[jj] = 0.f;
#pragma unroll
    for (int rr = 0; rr < G::R2; ++rr) accW2[jj][rr] = 0.f;
  }
  // dW1 / db1: thread owns the entries tid + 256 j of [6][C][k][k]
  float accW1[G::J1], accb1[G::J1];
  int xbase[G::J1], o1[G::J1];
#pragma unroll
  for (int j = 0; j < G::J1; ++j) {
    const int en = tid + kThreads * j < 6 * G::T1 ? tid + kThreads * j : 0;
    const int tap = en % G::T1, c = tap / (G::K * G::K), kk = tap % (G::K * G::K);
    o1[j] = en / G::T1;
    xbase[j] = c * G::HW + (kk / G::K) * G::W + kk % G::K;
    accW1[j] = accb1[j] = 0.f;
  }

  src.for_each_group([&](auto grp) {
    src.stage(xs, grp, tid);
    __syncthreads();
    conv1_phase<G>(xs, a1s, arg1s, W1, b1, tid);
    __syncthreads();
    if (RECOMPUTE) {
      conv2_phase<G>(a1s, W2, b2, tid, [&](int s, int ch, int cell, float, int code) {
        arg2s[s * G::F + ch * G::NP2 + cell] = (unsigned char)code;
      });
      __syncthreads();
    }
    // the cotangent of the features through pool 2 and ReLU: dense map and list
    for (int i = tid; i < G::IPB * G::F; i += kThreads) {
      const int s = i / G::F, r = i % G::F, ch = r / G::NP2, cell = r % G::NP2;
      const int cy = cell / G::P2, cx = cell % G::P2;
      const int64_t im = src.row(grp, s);
      int code = 4;
      if (im >= 0) code = RECOMPUTE ? arg2s[i] : arg2[im * G::F + r];
      const float g = code < 4 ? g_feat[im * G::F + r] : 0.f;
      float* dd = d2 + (s * 16 + ch) * G::U2 * G::U2 + 2 * cy * G::U2 + 2 * cx;
      dd[0] = code == 0 ? g : 0.f;
      dd[1] = code == 1 ? g : 0.f;
      dd[G::U2] = code == 2 ? g : 0.f;
      dd[G::U2 + 1] = code == 3 ? g : 0.f;
      l2[i] = float2i{g, (2 * cy + ((code >> 1) & 1)) * G::P1 + 2 * cx + (code & 1)};
    }
    __syncthreads();
    // dW2[o][ci][ky][kx] += g * a1[ci][y + ky][x + kx] over the windows' entries
#pragma unroll 1
    for (int s = 0; s < G::IPB; ++s)
#pragma unroll 1
      for (int cell = 0; cell < G::NP2; ++cell)
#pragma unroll
        for (int jj = 0; jj < 4; ++jj) {
          const float2i q = l2[(s * 16 + wave * 4 + jj) * G::NP2 + cell];
          accb2[jj] += q.v;
#pragma unroll
          for (int rr = 0; rr < G::R2; ++rr)
            accW2[jj][rr] = fmaf(q.v, a1s[s * 6 * G::NP1 + abase[rr] + q.off], accW2[jj][rr]);
        }
    // da1[ci][y][x] = sum_{o, ky, kx} dpre2[o][y - ky][x - kx] W2[o][ci][ky][kx], then through pool 1 and ReLU
    {
      const int s = tid / G::NP1, p = tid % G::NP1;
      if (s < G::IPB) {
        const int py = p / G::P1, px = p % G::P1;
        float acc[6] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
        const float* db = d2 + s * 16 * G::U2 * G::U2;
#pragma unroll 1
        for (int o = 0; o < 16; ++o) {                 // a rolled loop: the 6 k^2 weights of one o are contiguous scalar loads
          const float* wo = W2 + o * G::T2;
          const float* dd = db + o * G::U2 * G::U2;
          float d[G::K * G::K];
#pragma unroll
          for (int ky = 0; ky < G::K; ++ky)
#pragma unroll
            for (int kx = 0; kx < G::K; ++kx) {
              const int yy = py - ky, xx = px - kx;
              const bool valid = (unsigned)yy < (unsigned)G::U2 && (unsigned)xx < (unsigned)G::U2;
              d[ky * G::K + kx] = valid ? dd[valid ? yy * G::U2 + xx : 0] : 0.f;
            }
          staged_weights<6, G::K * G::K, Stage<G::K>::GS>([&](int ci) { return wo + ci * G::K * G::K; },
                                                          [&](int ci, const float* w, int& z) {
#pragma unroll
                                                            for (int t = 0; t < G::K * G::K; ++t)
                                                              acc[ci] = fmaf(d[t], w[t], acc[ci]);
                                                            tie(z, acc[ci]);
                                                          });
        }
#pragma unroll
        for (int ci = 0; ci < 6; ++ci) {
          const int code = arg1s[(s * 6 + ci) * G::NP1 + p];
          const float g = code < 4 ? acc[ci] : 0.f;
          float* dd = d1 + (s * 6 + ci) * G::U1 * G::U1 + 2 * py * G::U1 + 2 * px;
          dd[0] = code == 0 ? g : 0.f;
          dd[1] = code == 1 ? g : 0.f;
          dd[G::U1] = code == 2 ? g : 0.f;
          dd[G::U1 + 1] = code == 3 ? g : 0.f;
          l1[(s * 6 + ci) * G::NP1 + p] = float2i{g, (2 * py + ((code >> 1) & 1)) * G::W + 2 * px + (code & 1)};
        }
      }
    }
    __syncthreads();
    // dW1[o][c][ky][kx] += g * e[c][y + ky][x + kx] over the windows' entries
#pragma unroll 1
    for (int s = 0; s < G::IPB; ++s)
#pragma unroll 4
      for (int p = 0; p < G::NP1; ++p)
#pragma unroll
        for (int j = 0; j < G::J1; ++j) {
          const float2i q = l1[(s * 6 + o1[j]) * G::NP1 + p];
          accb1[j] += q.v;
          accW1[j] = fmaf(q.v, xs[s * G::IMG + xbase[j] + q.off], accW1[j]);
        }
    src.de_phase(d1, W1, grp, tid);
    __syncthreads();
  });

  // this workgroup's partial gradients: [dW1 6*T1][db1 6][dW2 16*T2][db2 16]
  float* prow = part + (int64_t)blockIdx.x * G::PW;
#pragma unroll
  for (int j = 0; j < G::J1; ++j) {
    const int en = tid + kThreads * j;
    if (en < 6 * G::T1) {
      prow[en] = accW1[j];
      if (en % G::T1 == 0) prow[6 * G::T1 + en / G::T1] = accb1[j];
    }
  }
#pragma unroll
  for (int jj = 0; jj < 4; ++jj) {
#pragma unroll
    for (int rr = 0; rr < G::R2; ++rr)
      if (lane + 64 * rr < G::T2) prow[6 * G::T1 + 6 + (wave * 4 + jj) * G::T2 + lane + 64 * rr] = accW2[jj][rr];
    if (lane == 0) prow[6 * G::T1 + 6 + 16 * G::T2 + wave * 4 + jj] = accb2[jj];
  }
}

template <class G, bool RECOMPUTE>
__global__ __launch_bounds__(kThreads, 2) void lenet_bwd_k(const float* __restrict__ e, int64_t ld_e,
                                                        const float* __restrict__ W1, const float* __restrict__ b1,
                                                        const float* __restrict__ W2, const float* __restrict__ b2,
                                                        const unsigned char* __restrict__ arg2,
                                                        const float* __restrict__ g_feat, float* __restrict__ ge,
                                                        int64_t ld_ge, float* __restrict__ part, int64_t n) {
  __shared__ float xs[G::IPB * G::IMG];
  RowsSrc<G> src{e, ld_e, ge, ld_ge, n};
  lenet_bwd_body<G, RECOMPUTE>(src, xs, W1, b1, W2, b2, arg2, g_feat, part);
}

template <class G, bool RECOMPUTE>
__global__ __launch_bounds__(kThreads, 2) void lenet_gated_bwd_k(GatedArgs a, const float* __restrict__ W1,
                                                              const float* __restrict__ b1, const float* __restrict__ W2,
                                                              const float* __restrict__ b2,
                                                              const unsigned char* __restrict__ arg2,
                                                              const float* __restrict__ g_feat, float* __restrict__ part) {
  __shared__ __attribute__((aligned(16))) float xs[G::IPB * G::IMG];
  __shared__ __attribute__((aligned(16))) float fs[G::IPB * G::IMG];
  GatedSrc<G> src;
  src.a = a;
  src.fs = fs;
  lenet_bwd_body<G, RECOMPUTE>(src, xs, W1, b1, W2, b2, arg2, g_feat, part);
}

template <class G, bool RECOMPUTE, bool WANT_DX>
__global__ __launch_bounds__(kThreads, 2) void lenet_rows_bwd_k(RowsArgs a, const float* __restrict__ W1,
                                                             const float* __restrict__ b1, const float* __restrict__ W2,
                                                             const float* __restrict__ b2,
                                                             const unsigned char* __restrict__ arg2,
                                                             const float* __restrict__ g_feat, float* __restrict__ part) {
  __shared__ __attribute__((aligned(16))) float xs[G::IPB * G::IMG];
  DetRowsSrc<G, WANT_DX> src;
  src.a = a;
  lenet_bwd_body<G, RECOMPUTE>(src, xs, W1, b1, W2, b2, arg2, g_feat, part);
}

// gx = sum over the nc chunks of rows, in chunk order;  nc = 0 (no rows): zeros
__global__ __launch_bounds__(kThreads) void lenet_rows_dx_k(const float* __restrict__ dxp, int nc, float* __restrict__ gx,
                                                            int64_t n) {
  const int64_t ij = (int64_t)blockIdx.x * kThreads + threadIdx.x;
  if (ij >= n) return;
  float s = 0.f;
  if (nc > 0) s = dxp[ij];
  for (int c = 1; c < nc; ++c) s += dxp[(int64_t)c * n + ij];
  gx[ij] = s;
}

// gA (+)= (sum over the nc chunks of samples, in chunk order) * dP/dA;  nc = 0 (empty batch): zeros, or gA left alone
__global__ __launch_bounds__(kThreads) void lenet_gated_dA_k(const float* __restrict__ tab, const float* __restrict__ dp,
                                                             int nc, float* __restrict__ gA, int accumulate, int64_t dd) {
  const int64_t ij = (int64_t)blockIdx.x * kThreads + threadIdx.x;
  if (ij >= dd) return;
  if (nc == 0) {
    if (!accumulate) gA[ij] = 0.f;
    return;
  }
  float s = dp[ij];
  for (int c = 1; c < nc; ++c) s += dp[(int64_t)c * dd + ij];
  gA[ij] = accumulate ? fmaf(s, tab[dd + ij], gA[ij]) : s * tab[dd + ij];
}

// out[en] = sum over the workgroups' partial rows, four interleaved chains in a fixed order (nb = 0: zeros)
__global__ __launch_bounds__(kThreads) void lenet_reduce_k(const float* __restrict__ part, int nb, int pw, int n1, int n2,
                                                           float* __restrict__ gW1, float* __restrict__ gb1,
                                                           float* __restrict__ gW2, float* __restrict__ gb2) {
  const int en = blockIdx.x * kThreads + threadIdx.x;
  if (en >= pw) return;
  float s0 = 0.f, s1 = 0.f, s2 = 0.f, s3 = 0.f;
  int b = 0;
  for (; b + 4 <= nb; b += 4) {
    s0 += part[(int64_t)b * pw + en];
    s1 += part[(int64_t)(b + 1) * pw + en];
    s2 += part[(int64_t)(b + 2) * pw + en];
    s3 += part[(int64_t)(b + 3) * pw + en];
  }
  for (; b < nb; ++b) s0 += part[(int64_t)b * pw + en];
  const float v = (s0 + s1) + (s2 + s3);
  if (en < n1) gW1[en] = v;
  else if (en < n1 + 6) gb1[en - n1] = v;
  else if (en < n1 + 6 + n2) gW2[en - n1 - 6] = v;
  else gb2[en - n1 - 6 - n2] = v;
}

// ------------------------------------------------------------------------------------------------------------------- host
typedef Geo<3, 32, 5> G0;
typedef Geo<1, 32, 3> G1;
typedef Geo<1, 16, 3> G2;
typedef Geo<1, 8, 2> G3;
static_assert(G0::F == 400 && G1::F == 576 && G2::F == 64 && G3::F == 16, "feature widths of the factory's geometries");

// f(G{}) with the Geo of (C, H, W, k); GNF_ESHAPE for a geometry that has none
template <class F>
auto with_geo(int C, int H, int W, int k, F f) -> decltype(f(G0{})) {
  if (C == 3 && H == 32 && W == 32 && k == 5) return f(G0{});
  if (C == 1 && H == 32 && W == 32 && k == 3) return f(G1{});
  if (C == 1 && H == 16 && W == 16 && k == 3) return f(G2{});
  if (C == 1 && H == 8 && W == 8 && k == 2) return f(G3{});
  return GNF_ESHAPE;
}

template <class... P>
bool any_null(P... p) { return (... || (p == nullptr)); }
template <class... P>
bool any_misaligned(P... p) { return (... || (((uintptr_t)p & 3) != 0)); }      // below dword alignment; null passes

inline bool bad_gate(int imp_mode, int gate_mode, const float* u1, const float* u2) {
  return imp_mode < 0 || imp_mode > 3 || gate_mode < 0 || gate_mode > 2 || (gate_mode == 1 && u1 && !u2);
}

inline GatedArgs gated_args(const float* x, const float* tab, int imp_mode, int gate_mode, float T, const float* u1,
                            const float* u2, uint64_t seed, uint64_t offset, int64_t B) {
  if (imp_mode == 0) gate_mode = 0;   // DAG:151-153: raw A, no gate
  GatedArgs a{};                      // dp, gpc, nchunk: the backward's, filled in by it
  a.x = x; a.tab = tab; a.u1 = u1; a.u2 = u2; a.seed = seed; a.offset = offset; a.gate_mode = gate_mode; a.T = T; a.B = B;
  return a;
}

template <class G>
int64_t groups_of(int64_t n) { return (n + G::IPB - 1) / G::IPB; }

inline int grid_of(int64_t units, int cap) { return (int)(units < cap ? units : cap); }

// the backward's chunks (of samples when gated, of rows behind a frozen gate) and its grid
struct Chunks { int64_t per, n; int grid; };

// whole groups of IPB samples, enough units (row, chunk) to fill the grid
template <class G>
Chunks gated_chunks(int64_t B) {
  const int64_t ngb = groups_of<G>(B);
  int64_t nchunk = (kBwdGridMax + G::IMG - 1) / G::IMG;
  if (nchunk > ngb) nchunk = ngb;
  const int64_t gpc = nchunk > 0 ? (ngb + nchunk - 1) / nchunk : 1;
  nchunk = (ngb + gpc - 1) / gpc;
  return Chunks{gpc, nchunk, grid_of(G::IMG * nchunk, kBwdGridMax)};
}

// with dL/dx: whole rows, enough units (chunk, group of samples) to fill the grid, nchunk <= R.  Without it a chunk is one
// row (the units of the forward)
template <class G>
Chunks rows_chunks(int64_t R, int64_t B, bool want_gx) {
  const int64_t ngb = groups_of<G>(B);
  int64_t rpc = 1, nchunk = (B == 0) ? 0 : R;
  if (want_gx && R > 0 && B > 0) {
    nchunk = (kBwdGridMax + ngb - 1) / ngb;
    if (nchunk > R) nchunk = R;
    rpc = (R + nchunk - 1) / nchunk;
    nchunk = (R + rpc - 1) / rpc;
  }
  return Chunks{rpc, nchunk, grid_of(nchunk * ngb, kBwdGridMax)};
}

// floats of the partial weight gradients [grid][PW] at the head of a backward's workspace
template <class G>
int64_t part_floats(int grid) { return (int64_t)(grid > 0 ? grid : 1) * G::PW; }

template <class G>
int64_t ws_bytes_of(int64_t n) { return part_floats<G>(grid_of(groups_of<G>(n), kBwdGridMax)) * (int64_t)sizeof(float); }

// ... | sums of dL/dP [nchunk][d][d]
template <class G>
int64_t gated_ws_bytes_of(int64_t B) {
  const Chunks c = gated_chunks<G>(B);
  return (part_floats<G>(c.grid) + c.n * G::IMG * G::IMG) * (int64_t)sizeof(float);
}

// ... | sums of dL/dx [nchunk][B][d] (want_gx)
template <class G>
int64_t rows_ws_bytes_of(int64_t R, int64_t B, bool want_gx) {
  const Chunks c = rows_chunks<G>(R, B, want_gx);
  return (part_floats<G>(c.grid) + (want_gx ? c.n * B * G::IMG : 0)) * (int64_t)sizeof(float);
}

// the nb workgroups' partial gradients -> gW1, gb1, gW2, gb2
template <class G>
int reduce_launch(const float* part, int nb, float* gW1, float* gb1, float* gW2, float* gb2, hipStream_t s) {
  hipLaunchKernelGGL(lenet_reduce_k, dim3((G::PW + kThreads - 1) / kThreads), dim3(kThreads), 0, s, part, nb, G::PW,
                     6 * G::T1, 16 * G::T2, gW1, gb1, gW2, gb2);
  GNF_LAUNCH_CHECK();
  return 0;
}

}  // namespace

extern "C" {

int gnf_lenet_conv_supported(int C, int H, int W, int k) {
  return with_geo(C, H, W, k, [](auto) { return 0; }) == 0;
}

int64_t gnf_lenet_conv_feat(int C, int H, int W, int k) {
  return with_geo(C, H, W, k, [](auto g) -> int64_t { return decltype(g)::F; });
}

int gnf_lenet_conv_fwd(const float* e, int64_t ld_e, int C, int H, int W, int k, const float* W1, const float* b1,
                       const float* W2, const float* b2, float* feat, unsigned char* argmax2, int64_t n_img,
                       gnf_stream_t stream) {
  return with_geo(C, H, W, k, [&](auto g) -> int {
    using G = decltype(g);
    if (n_img < 0 || any_null(W1, b1, W2, b2) || (any_null(e, feat) && n_img > 0)) return GNF_EINVAL;
    if (any_misaligned(e, W1, b1, W2, b2, feat)) return GNF_EINVAL;
    if (n_img == 0) return 0;
    if (ld_e < G::IMG) return GNF_EINVAL;
    hipLaunchKernelGGL(lenet_fwd_k<G>, dim3(grid_of(groups_of<G>(n_img), kFwdGridMax)), dim3(kThreads), 0,
                       (hipStream_t)stream, e, ld_e, W1, b1, W2, b2, feat, argmax2, n_img);
    GNF_LAUNCH_CHECK();
    return 0;
  });
}

int64_t gnf_lenet_conv_bwd_ws_bytes(int C, int H, int W, int k, int64_t n_img) {
  if (n_img < 0) return GNF_EINVAL;
  return with_geo(C, H, W, k, [&](auto g) { return ws_bytes_of<decltype(g)>(n_img); });
}

int gnf_lenet_conv_bwd(const float* e, int64_t ld_e, int C, int H, int W, int k, const float* W1, const float* b1,
                       const float* W2, const float* b2, const unsigned char* argmax2, const float* g_feat, float* ge,
                       int64_t ld_ge, float* gW1, float* gb1, float* gW2, float* gb2, void* ws, int64_t ws_bytes,
                       int64_t n_img, gnf_stream_t stream) {
  return with_geo(C, H, W, k, [&](auto g) -> int {
    using G = decltype(g);
    if (n_img < 0 || any_null(W1, b1, W2, b2, gW1, gb1, gW2, gb2, ws) || (any_null(e, g_feat) && n_img > 0))
      return GNF_EINVAL;
    if (any_misaligned(e, W1, b1, W2, b2, g_feat, ge, gW1, gb1, gW2, gb2, ws)) return GNF_EINVAL;
    if (ws_bytes < ws_bytes_of<G>(n_img)) return GNF_EWS;
    if (n_img > 0 && (ld_e < G::IMG || (ge && ld_ge < G::IMG))) return GNF_EINVAL;
    hipStream_t s = (hipStream_t)stream;
    float* part = static_cast<float*>(ws);
    const int nb = grid_of(groups_of<G>(n_img), kBwdGridMax);
    if (nb > 0) {
      const auto kern = argmax2 ? lenet_bwd_k<G, false> : lenet_bwd_k<G, true>;       // no saved decisions: recompute
      hipLaunchKernelGGL(kern, dim3(nb), dim3(kThreads), 0, s, e, ld_e, W1, b1, W2, b2, argmax2, g_feat, ge, ld_ge, part,
                         n_img);
      GNF_LAUNCH_CHECK();
    }
    return reduce_launch<G>(part, nb, gW1, gb1, gW2, gb2, s);
  });
}

int gnf_lenet_gated_fwd(const float* x, const float* A, float* tab, int C, int H, int W, int k, int imp_mode, int gate_mode,
                        float h_thresh, float temperature, const float* u1, const float* u2, uint64_t seed,
                        uint64_t offset, const float* W1, const float* b1, const float* W2, const float* b2, float* feat,
                        unsigned char* argmax2, int64_t B, gnf_stream_t stream) {
  return with_geo(C, H, W, k, [&](auto g) -> int {
    using G = decltype(g);
    if (B < 0 || any_null(A, tab, W1, b1, W2, b2) || (any_null(x, feat) && B > 0) || bad_gate(imp_mode, gate_mode, u1, u2))
      return GNF_EINVAL;
    if (any_misaligned(x, A, tab, u1, u2, W1, b1, W2, b2, feat)) return GNF_EINVAL;
    if (B == 0) return 0;
    hipStream_t s = (hipStream_t)stream;
    if (const int rc = launch_tab(A, tab, imp_mode, h_thresh, temperature, (int64_t)G::IMG, s)) return rc;
    const GatedArgs a = gated_args(x, tab, imp_mode, gate_mode, temperature, u1, u2, seed, offset, B);
    hipLaunchKernelGGL(lenet_gated_fwd_k<G>, dim3(grid_of(G::IMG * groups_of<G>(B), kFwdGridMax)), dim3(kThreads), 0, s, a,
                       W1, b1, W2, b2, feat, argmax2);
    GNF_LAUNCH_CHECK();
    return 0;
  });
}

int gnf_lenet_rows_fwd_arg(const float* x, const float* P, int64_t ld_p, const int32_t* rows, int64_t R, int C, int H, int W,
                           int k, const float* W1, const float* b1, const float* W2, const float* b2, float* feat,
                           unsigned char* argmax2, int variable_major, int64_t B, gnf_stream_t stream) {
  return with_geo(C, H, W, k, [&](auto g) -> int {
    using G = decltype(g);
    if (B < 0 || R < 0 || any_null(P, W1, b1, W2, b2) || (any_null(x, feat) && B > 0 && R > 0)) return GNF_EINVAL;
    if (any_misaligned(x, P, rows, W1, b1, W2, b2, feat)) return GNF_EINVAL;
    if (ld_p < G::IMG || (!rows && R > G::IMG)) return GNF_EINVAL;
    if (B == 0 || R == 0) return 0;
    const dim3 grid(grid_of(R * groups_of<G>(B), kFwdGridMax));
    hipStream_t s = (hipStream_t)stream;
    if (argmax2)
      hipLaunchKernelGGL(lenet_rows_fwd_arg_k<G>, grid, dim3(kThreads), 0, s, x, P, ld_p, rows, R, B, W1, b1, W2, b2, feat,
                         argmax2, variable_major);
    else
      hipLaunchKernelGGL(lenet_rows_fwd_k<G>, grid, dim3(kThreads), 0, s, x, P, ld_p, rows, R, B, W1, b1, W2, b2, feat,
                         variable_major);
    GNF_LAUNCH_CHECK();
    return 0;
  });
}

int gnf_lenet_rows_fwd(const float* x, const float* P, int64_t ld_p, const int32_t* rows, int64_t R, int C, int H, int W,
                       int k, const float* W1, const float* b1, const float* W2, const float* b2, float* feat,
                       int variable_major, int64_t B, gnf_stream_t stream) {
  return gnf_lenet_rows_fwd_arg(x, P, ld_p, rows, R, C, H, W, k, W1, b1, W2, b2, feat, nullptr, variable_major, B, stream);
}

int64_t gnf_lenet_rows_bwd_ws_bytes(int C, int H, int W, int k, int64_t R, int64_t B, int want_gx) {
  if (R < 0 || B < 0) return GNF_EINVAL;
  return with_geo(C, H, W, k, [&](auto g) { return rows_ws_bytes_of<decltype(g)>(R, B, want_gx != 0); });
}

int gnf_lenet_rows_bwd(const float* x, const float* P, int64_t ld_p, const int32_t* rows, int64_t R, int C, int H, int W,
                       int k, const float* W1, const float* b1, const float* W2, const float* b2,
                       const unsigned char* argmax2, const float* g_feat, int variable_major, float* gx, float* gW1,
                       float* gb1, float* gW2, float* gb2, void* ws, int64_t ws_bytes, int64_t B, gnf_stream_t stream) {
  return with_geo(C, H, W, k, [&](auto g) -> int {
    using G = decltype(g);
    if (B < 0 || R < 0 || any_null(P, W1, b1, W2, b2, gW1, gb1, gW2, gb2, ws) || (any_null(x, g_feat) && B > 0 && R > 0))
      return GNF_EINVAL;
    if (any_misaligned(x, P, rows, W1, b1, W2, b2, g_feat, gx, gW1, gb1, gW2, gb2, ws)) return GNF_EINVAL;
    if (ld_p < G::IMG || (!rows && R > G::IMG)) return GNF_EINVAL;
    if (ws_bytes < rows_ws_bytes_of<G>(R, B, gx != nullptr)) return GNF_EWS;
    hipStream_t s = (hipStream_t)stream;
    float* part = static_cast<float*>(ws);
    const Chunks c = rows_chunks<G>(R, B, gx != nullptr);
    RowsArgs a{};
    a.x = x; a.P = P; a.ld_p = ld_p; a.rows = rows; a.R = R; a.B = B; a.variable_major = variable_major;
    a.dxp = gx ? part + part_floats<G>(c.grid) : nullptr; a.rpc = c.per; a.nchunk = c.n;
    if (c.grid > 0) {
      const auto kern = argmax2 ? (gx ? lenet_rows_bwd_k<G, false, true> : lenet_rows_bwd_k<G, false, false>)
                                : (gx ? lenet_rows_bwd_k<G, true, true> : lenet_rows_bwd_k<G, true, false>);
      hipLaunchKernelGGL(kern, dim3(c.grid), dim3(kThreads), 0, s, a, W1, b1, W2, b2, argmax2, g_feat, part);
      GNF_LAUNCH_CHECK();
    }
    if (const int rc = reduce_launch<G>(part, c.grid, gW1, gb1, gW2, gb2, s)) return rc;
    const int64_t n = B * G::IMG;
    if (gx && n > 0) {
      hipLaunchKernelGGL(lenet_rows_dx_k, dim3((unsigned)((n + kThreads - 1) / kThreads)), dim3(kThreads), 0, s, a.dxp,
                         c.grid > 0 ? (int)c.n : 0, gx, n);
      GNF_LAUNCH_CHECK();
    }
    return 0;
  });
}

int64_t gnf_lenet_gated_bwd_ws_bytes(int C, int H, int W, int k, int64_t B) {
  if (B < 0) return GNF_EINVAL;
  return with_geo(C, H, W, k, [&](auto g) { return gated_ws_bytes_of<decltype(g)>(B); });
}

int gnf_lenet_gated_bwd(const float* x, const float* tab, int C, int H, int W, int k, int imp_mode, int gate_mode,
                        float temperature, const float* u1, const float* u2, uint64_t seed, uint64_t offset,
                        const float* W1, const float* b1, const float* W2, const float* b2, const unsigned char* argmax2,
                        const float* g_feat, float* gA, int accumulate, float* gW1, float* gb1, float* gW2, float* gb2,
                        void* ws, int64_t ws_bytes, int64_t B, gnf_stream_t stream) {
  return with_geo(C, H, W, k, [&](auto g) -> int {
    using G = decltype(g);
    if (B < 0 || any_null(W1, b1, W2, b2, gW1, gb1, gW2, gb2, ws) || (any_null(x, tab, g_feat) && B > 0) ||
        bad_gate(imp_mode, gate_mode, u1, u2))
      return GNF_EINVAL;
    if (any_misaligned(x, tab, u1, u2, W1, b1, W2, b2, g_feat, gA, gW1, gb1, gW2, gb2, ws)) return GNF_EINVAL;
    if (ws_bytes < gated_ws_bytes_of<G>(B)) return GNF_EWS;
    hipStream_t s = (hipStream_t)stream;
    float* part = static_cast<float*>(ws);
    const Chunks c = gated_chunks<G>(B);
    float* dp = part + part_floats<G>(c.grid);
    GatedArgs a = gated_args(x, tab, imp_mode, gate_mode, temperature, u1, u2, seed, offset, B);
    a.dp = gA ? dp : nullptr;
    a.gpc = c.per;
    a.nchunk = c.n;
    if (c.grid > 0) {
      const auto kern = argmax2 ? lenet_gated_bwd_k<G, false> : lenet_gated_bwd_k<G, true>;
      hipLaunchKernelGGL(kern, dim3(c.grid), dim3(kThreads), 0, s, a, W1, b1, W2, b2, argmax2, g_feat, part);
      GNF_LAUNCH_CHECK();
    }
    if (const int rc = reduce_launch<G>(part, c.grid, gW1, gb1, gW2, gb2, s)) return rc;
    if (gA) {
      const int64_t dd = (int64_t)G::IMG * G::IMG;
      hipLaunchKernelGGL(lenet_gated_dA_k, dim3((unsigned)((dd + kThreads - 1) / kThreads)), dim3(kThreads), 0, s, tab, dp,
                         (int)c.n, gA, accumulate, dd);
      GNF_LAUNCH_CHECK();
    }
    return 0;
  });
}

}  // extern "C"
