// First layer of a DAGMLP behind a DAG conditioner, with the gate fused in (models/Conditionners/DAGConditioner.py:7-20,
// 94-169): the masked copies e[b*d+i, :] = x[b, :] * gate(b, i, :) are built in LDS and contracted at once,
//   a1[b*d+i, n] = act( b1[n] + [hot] W1[n, d+i] + sum_{j<d} W1[n, j] * e[b*d+i, j] ),
// so neither e (with its one-hot half: d-1 exact zeros and a one per row) nor its cotangent ever exists in memory.  The
// one-hot half of the layer is column d+i of W1, a per-variable bias of the epilogue.  Gate arithmetic: gnf_dag_gate.h only,
// with the Philox counter of gnf_dag_gate_fwd, so a copy built here has the bits that kernel writes.
//
// Tiles are WHOLE samples: s = floor(64 / d) samples = s*d <= 64 consecutive rows, in 16-row MFMA tiles.  The contraction
// runs on v_mfma_f32_16x16x4_f32 with W1 as the A operand and the copies as the B operand, so a lane ends up with four
// CONSECUTIVE n of one row (one 16-byte store).  Each lane fetches 16 bytes of its operand row per four MFMAs
// (k = 16 kb + 4 (lane >> 4) + t in step t: the same k for both operands, a fixed summation order that does not depend on the
// alignment of W1).  LDS pitch of the copies: 72 floats = 8 (mod 64), for which the four 16-lane groups of ds_read_b128
// ({0-3, 12-15, 20-27}, ...) hit 16 distinct 16-byte slots (rows r at 8 r, the other k quad at 8 r + 4).
#include "gnf_dag_gate.h"

namespace {

constexpr int kT = 256;           // threads per workgroup (4 wavefronts)
constexpr int kRows = 64;         // rows of a tile
constexpr int kPE = 72;           // LDS pitch of the copies (forward, data gradient)
constexpr int kSlab = 16;         // n tiles (of 16) per workgroup of the forward
constexpr int kMaxD = 64;
constexpr int kCT = 9;            // column tiles of the weight-gradient role: 2 d + 1 <= 129 columns
constexpr int kPW = 144;          // LDS pitch of its copies (e | one-hot | ones) = 16 (mod 32): the two k rows of a
constexpr int kPG = 80;           //   ds_read_b32 half-wave sit on opposite halves of the banks; same for the cotangent

__device__ __forceinline__ bool al16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

struct Src {
  const float* x;
  // gated form
  const float* tab; int gate_mode; float T; const float* u1; const float* u2; uint64_t seed, offset;
  // rows form (tab == nullptr)
  const float* P; int64_t ld_p; const int32_t* rows; int64_t R; int vm;
  int64_t B, d, M;                // M = number of copies (B*d, or B*R)
  int rpt;                        // rows per tile
};

// copy (m, column quad jq) of the source: four values, exact zeros behind column d
__device__ __forceinline__ void copy_quad(const Src& s, int64_t m, int jq, float (&out)[4]) {
  const int64_t d = s.d, j0 = 4 * jq;
  const int nv = d - j0 < 4 ? (int)(d - j0) : 4;
  float x4[4], p4[4];
  if (s.tab) {
    const int64_t b = m / d, i = m - b * d, dd = d * d;
    float et4[4] = {0.f, 0.f, 0.f, 0.f};
    const bool vt = quad_aligned(s.tab, d), vx = quad_aligned(s.x, d);
    load4(s.tab + i * d + j0, nv, vt, p4);
    if (s.gate_mode == 1) load4(s.tab + 2 * dd + i * d + j0, nv, vt, et4);
    const Draw4 n = draw4(s.gate_mode, s.u1, s.u2, s.seed, s.offset, m, jq, d);
    load4(s.x + b * d + j0, nv, vx, x4);
#pragma unroll
    for (int h = 0; h < 4; ++h) out[h] = h < nv ? gate_copy(s.gate_mode, x4[h], p4[h], et4[h], n.v[h], n.w[h], s.T) : 0.f;
  } else {
    const int64_t b = m / s.R, r = m - b * s.R;
    const int64_t i = s.rows ? (int64_t)s.rows[r] : r;
    load4(s.P + i * s.ld_p + j0, nv, quad_aligned(s.P, s.ld_p), p4);
    load4(s.x + b * d + j0, nv, quad_aligned(s.x, d), x4);
#pragma unroll
    for (int h = 0; h < 4; ++h) out[h] = h < nv ? x4[h] * p4[h] : 0.f;
  }
}

// variable index (the one-hot column) and output row of copy m
__device__ __forceinline__ void copy_row(const Src& s, int64_t m, int* var, int64_t* orow) {
  if (s.tab) { *var = (int)(m % s.d); *orow = m; return; }
  const int64_t b = m / s.R, r = m - b * s.R;
  *var = s.rows ? s.rows[r] : (int)r;
  *orow = s.vm ? r * s.B + b : m;
}

struct FwdArgs {
  Src s; const float* W1; int64_t ld_w; const float* b1; int hot, relu; float* a1; int64_t H, ntiles;
};

__global__ __launch_bounds__(kT) void dagmlp_fwd_k(FwdArgs a) {
  __shared__ __attribute__((aligned(16))) float es[kRows * kPE];
  __shared__ int64_t orow_s[kRows];
  __shared__ int var_s[kRows];
  const Src& s = a.s;
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, lr = lane & 15, q = lane >> 4;
  const int d = (int)s.d, KP = (d + 15) & ~15, KQ = KP >> 2, rpt = s.rpt, RT = (rpt + 15) >> 4;
  const int64_t H = a.H;
  const int NT = (int)((H + 15) >> 4);
  const int nt0 = blockIdx.y * kSlab, nt1 = nt0 + kSlab < NT ? nt0 + kSlab : NT;
  const bool vw = al16(a.W1) && (a.ld_w & 3) == 0, vo = al16(a.a1) && (H & 3) == 0;
  for (int64_t t = blockIdx.x; t < a.ntiles; t += gridDim.x) {
    const int64_t m0 = t * rpt;
    __syncthreads();                                         // the previous tile's readers are done
    for (int u = tid; u < RT * 16 * KQ; u += kT) {
      const int rl = u / KQ, jq = u - rl * KQ;
      float o[4] = {0.f, 0.f, 0.f, 0.f};
      if (rl < rpt && m0 + rl < s.M && 4 * jq < d) copy_quad(s, m0 + rl, jq, o);
      *reinterpret_cast<float4*>(&es[rl * kPE + 4 * jq]) = make_float4(o[0], o[1], o[2], o[3]);
    }
    if (tid < kRows) {
      int var = 0; int64_t orow = -1;
      if (tid < rpt && m0 + tid < s.M) copy_row(s, m0 + tid, &var, &orow);
      var_s[tid] = var; orow_s[tid] = orow;
    }
    __syncthreads();
    for (int nt = nt0 + w; nt < nt1; nt += 4) {
      const int64_t n = (int64_t)nt * 16 + lr;
      f32x4 acc[4];
#pragma unroll
      for (int rt = 0; rt < 4; ++rt) acc[rt] = f32x4{0.f, 0.f, 0.f, 0.f};
      for (int kb = 0; kb < KP; kb += 16) {
        const int k0 = kb + 4 * q;
        float wv[4] = {0.f, 0.f, 0.f, 0.f};
        if (n < H) {
          const float* wp = a.W1 + n * a.ld_w + k0;
          if (vw && k0 + 3 < d) {
            const float4 v = *reinterpret_cast<const float4*>(wp);
            wv[0] = v.x; wv[1] = v.y; wv[2] = v.z; wv[3] = v.w;
          } else {
#pragma unroll
            for (int h = 0; h < 4; ++h) wv[h] = k0 + h < d ? wp[h] : 0.f;
          }
        }
#pragma unroll
        for (int rt = 0; rt < 4; ++rt) {
          if (rt < RT) {
            const f32x4 ev = *reinterpret_cast<const f32x4*>(&es[(rt * 16 + lr) * kPE + k0]);
#pragma unroll
            for (int h = 0; h < 4; ++h) acc[rt] = mfma(wv[h], ev[h], acc[rt]);
          }
        }
      }
      // lane: D[n = 16 nt + 4 q + r][row = 16 rt + lr]
      const int64_t n0 = (int64_t)nt * 16 + 4 * q;
      float bias[4];
#pragma unroll
      for (int r = 0; r < 4; ++r) bias[r] = n0 + r < H ? a.b1[n0 + r] : 0.f;
#pragma unroll
      for (int rt = 0; rt < 4; ++rt) {
        if (rt < RT) {
          const int rl = rt * 16 + lr;
          const int64_t orow = orow_s[rl];
          if (orow >= 0) {
            float o[4];
#pragma unroll
            for (int r = 0; r < 4; ++r) {
              float v = acc[rt][r] + bias[r];
              if (a.hot && n0 + r < H) v += a.W1[(n0 + r) * a.ld_w + d + var_s[rl]];
              o[r] = a.relu ? relu1(v) : v;
            }
            float* op = a.a1 + orow * H + n0;
            if (vo && n0 + 3 < H) {
              *reinterpret_cast<float4*>(op) = make_float4(o[0], o[1], o[2], o[3]);
            } else {
#pragma unroll
              for (int r = 0; r < 4; ++r)
                if (n0 + r < H) op[r] = o[r];
            }
          }
        }
      }
    }
  }
}

// ------------------------------------------------------------------------------------------------------------------
// Backward.  g [B*d, H]: the cotangent of a1, already multiplied by [a1 > 0].  One launch, two roles, both rebuild the
// copies (and the noise) of their tiles; nothing was kept by the forward:
//   data role (workgroups 0 .. nwg_d):  de = g W1[:, :d] of a tile on MFMA (K = H) into LDS;  gP[i, j] += through
//     gate_dp_add, held in registers across the workgroup's tiles (one thread per (i, column quad) unit, up to four units),
//     one [d, d] partial per workgroup;  gx[b, j] = sum_i de * d e / d x in ascending i: a sample's d copies sit in one tile,
//     so gx has one writer per element.
//   weight role (workgroup (wx, slab of 64 n)):  g^T [e | one-hot | 1] of a tile on MFMA (K = the tile's rows), accumulated
//     in registers across the tiles wx, wx + nwg_w, ...: columns [0, d) are gW1, [d, 2 d) its one-hot half, the last gb1.
// dagmlp_reduce_k adds the partials in workgroup order.  No float atomics; the same call gives the same bits.
struct BwdArgs {
  Src s; const float* W1; int64_t ld_w; int hot; const float* g; float* gx; float* partP; float* partW;
  int64_t H, ntiles; int nwg_d, nwg_w, ncols, want_p;
};

__device__ __forceinline__ void bwd_data_role(const BwdArgs& a, float* des, int wg) {
  const Src& s = a.s;
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, lr = lane & 15, q = lane >> 4;
  const int d = (int)s.d, KP = (d + 15) & ~15, JT = KP >> 4, dq = (d + 3) >> 2, rpt = s.rpt, RT = (rpt + 15) >> 4;
  const int64_t H = a.H, dd = (int64_t)d * d;
  const int spt = rpt / d;                                    // samples per tile
  const bool vg = al16(a.g) && (H & 3) == 0;
  const bool vt = quad_aligned(s.tab, d), vx = quad_aligned(s.x, d);
  float accP[4][4];
#pragma unroll
  for (int uu = 0; uu < 4; ++uu)
#pragma unroll
    for (int h = 0; h < 4; ++h) accP[uu][h] = 0.f;
  for (int64_t t = wg; t < a.ntiles; t += a.nwg_d) {
    const int64_t m0 = t * rpt;
    __syncthreads();
    if (w < RT) {                                             // wavefront w: row tile w, every column tile
      const int64_t m = m0 + w * 16 + lr;
      const bool rok = w * 16 + lr < rpt && m < s.M;
      f32x4 acc[4];
#pragma unroll
      for (int jt = 0; jt < 4; ++jt) acc[jt] = f32x4{0.f, 0.f, 0.f, 0.f};
      for (int64_t nb = 0; nb < H; nb += 16) {
        const int64_t n0 = nb + 4 * q;
        float gv[4] = {0.f, 0.f, 0.f, 0.f};
        if (rok && n0 < H) {
          const float* gp = a.g + m * H + n0;
          if (vg && n0 + 3 < H) {
            const float4 v = *reinterpret_cast<const float4*>(gp);
            gv[0] = v.x; gv[1] = v.y; gv[2] = v.z; gv[3] = v.w;
          } else {
#pragma unroll
            for (int h = 0; h < 4; ++h) gv[h] = n0 + h < H ? gp[h] : 0.f;
          }
        }
#pragma unroll
        for (int jt = 0; jt < 4; ++jt) {
          if (jt < JT) {
            const int j = jt * 16 + lr;
#pragma unroll
            for (int h = 0; h < 4; ++h) {
              const float wv = (n0 + h < H && j < d) ? a.W1[(n0 + h) * a.ld_w + j] : 0.f;
              acc[jt] = mfma(gv[h], wv, acc[jt]);
            }
          }
        }
      }
      // lane: D[row = 16 w + 4 q + r][j = 16 jt + lr]
#pragma unroll
      for (int jt = 0; jt < 4; ++jt)
        if (jt < JT)
#pragma unroll
          for (int r = 0; r < 4; ++r) des[(w * 16 + 4 * q + r) * kPE + jt * 16 + lr] = acc[jt][r];
    }
    __syncthreads();
#pragma unroll
    for (int uu = 0; uu < 4; ++uu) {
      const int u = tid + uu * kT;
      if (u < d * dq) {
        const int i = u / dq, jq = u - i * dq, j0 = 4 * jq;
        const int nv = d - j0 < 4 ? d - j0 : 4;
        float p4[4], et4[4] = {0.f, 0.f, 0.f, 0.f}, q4[4] = {0.f, 0.f, 0.f, 0.f};
        load4(s.tab + (int64_t)i * d + j0, nv, vt, p4);
        if (s.gate_mode == 1) {
          load4(s.tab + 2 * dd + (int64_t)i * d + j0, nv, vt, et4);
          load4(s.tab + 3 * dd + (int64_t)i * d + j0, nv, vt, q4);
        }
        for (int sl = 0; sl < spt; ++sl) {
          const int rl = sl * d + i;
          const int64_t m = m0 + rl;
          if (m >= s.M) break;
          const int64_t b = m / d;
          const Draw4 n = draw4(s.gate_mode, s.u1, s.u2, s.seed, s.offset, m, jq, d);
          float x4[4];
          load4(s.x + b * d + j0, nv, vx, x4);
#pragma unroll
          for (int h = 0; h < 4; ++h) {
            if (h < nv) {
              float* dp = &des[rl * kPE + j0 + h];
              const float gde = *dp;
              if (a.want_p)
                accP[uu][h] = gate_dp_add(s.gate_mode, gde, x4[h], p4[h], et4[h], q4[h], n.v[h], n.w[h], s.T, accP[uu][h]);
              const float f = s.gate_mode == 1 ? gumbel_gate(et4[h], n.v[h], n.w[h], s.T) : p4[h];
              *dp = gde * f;
            }
          }
        }
      }
    }
    if (a.gx) {
      __syncthreads();
      if (tid < spt * d) {
        const int sl = tid / d, j = tid - sl * d;
        const int64_t b = t * spt + sl;
        if (b < s.B) {
          float sum = 0.f;
          for (int i = 0; i < d; ++i) sum += des[(sl * d + i) * kPE + j];
          a.gx[b * d + j] = sum;
        }
      }
    }
  }
  if (a.want_p) {
#pragma unroll
    for (int uu = 0; uu < 4; ++uu) {
      const int u = tid + uu * kT;
      if (u < d * dq) {
        const int i = u / dq, jq = u - i * dq;
#pragma unroll
        for (int h = 0; h < 4; ++h)
          if (4 * jq + h < d) a.partP[(int64_t)wg * dd + (int64_t)i * d + 4 * jq + h] = accP[uu][h];
      }
    }
  }
}

__device__ __forceinline__ void bwd_weight_role(const BwdArgs& a, float* ew, float* gs, int wx, int slab) {
  const Src& s = a.s;
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, lr = lane & 15, q = lane >> 4;
  const int d = (int)s.d, dq = (d + 3) >> 2, rpt = s.rpt, ncols = a.ncols, CT = (ncols + 15) >> 4, CW = CT * 16;
  const int KS = (rpt + 3) >> 2;
  const int64_t H = a.H, nslab0 = (int64_t)slab * 64;
  const bool vg = al16(a.g) && (H & 3) == 0;
  f32x4 acc[kCT];
#pragma unroll
  for (int ct = 0; ct < kCT; ++ct) acc[ct] = f32x4{0.f, 0.f, 0.f, 0.f};
  for (int64_t t = wx; t < a.ntiles; t += a.nwg_w) {
    const int64_t m0 = t * rpt;
    __syncthreads();
    for (int u = tid; u < KS * 4 * dq; u += kT) {             // the copies
      const int rl = u / dq, jq = u - rl * dq;
      float o[4] = {0.f, 0.f, 0.f, 0.f};
      if (rl < rpt && m0 + rl < s.M) copy_quad(s, m0 + rl, jq, o);
#pragma unroll
      for (int h = 0; h < 4; ++h)
        if (4 * jq + h < d) ew[rl * kPW + 4 * jq + h] = o[h];
    }
    for (int u = tid; u < KS * 4 * (CW - d); u += kT) {       // one-hot half, the column of ones, zero padding
      const int rl = u / (CW - d), c = d + (u - rl * (CW - d));
      float v = 0.f;
      if (rl < rpt && m0 + rl < s.M) {
        if (c == ncols - 1) v = 1.f;
        else if (a.hot && c < 2 * d) v = (c - d == (int)((m0 + rl) % d)) ? 1.f : 0.f;
      }
      ew[rl * kPW + c] = v;
    }
    for (int u = tid; u < KS * 4 * 16; u += kT) {             // the cotangent slab [rows][64 n]
      const int rl = u >> 4, c0 = (u & 15) * 4;
      const int64_t m = m0 + rl, n0 = nslab0 + c0;
      float gv[4] = {0.f, 0.f, 0.f, 0.f};
      if (rl < rpt && m < s.M && n0 < H) {
        const float* gp = a.g + m * H + n0;
        if (vg && n0 + 3 < H) {
          const float4 v = *reinterpret_cast<const float4*>(gp);
          gv[0] = v.x; gv[1] = v.y; gv[2] = v.z; gv[3] = v.w;
        } else {
#pragma unroll
          for (int h = 0; h < 4; ++h) gv[h] = n0 + h < H ? gp[h] : 0.f;
        }
      }
      *reinterpret_cast<float4*>(&gs[rl * kPG + c0]) = make_float4(gv[0], gv[1], gv[2], gv[3]);
    }
    __syncthreads();
    for (int ks = 0; ks < KS; ++ks) {
      const int r = 4 * ks + q;
      const float av = gs[r * kPG + w * 16 + lr];
#pragma unroll
      for (int ct = 0; ct < kCT; ++ct)
        if (ct < CT) acc[ct] = mfma(av, ew[r * kPW + ct * 16 + lr], acc[ct]);
    }
  }
  // lane: D[n = 64 slab + 16 w + 4 q + r][c = 16 ct + lr]
  float* out = a.partW + (int64_t)wx * H * ncols;
#pragma unroll
  for (int ct = 0; ct < kCT; ++ct) {
    if (ct < CT) {
      const int c = ct * 16 + lr;
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int64_t n = nslab0 + w * 16 + 4 * q + r;
        if (n < H && c < ncols) out[n * ncols + c] = acc[ct][r];
      }
    }
  }
}

__global__ __launch_bounds__(kT) void dagmlp_gated_bwd_k(BwdArgs a) {
  __shared__ __attribute__((aligned(16))) float lds[kRows * kPW + kRows * kPG];
  const int wg = blockIdx.x;
  if (wg < a.nwg_d) {
    bwd_data_role(a, lds, wg);
  } else {
    const int u = wg - a.nwg_d;
    bwd_weight_role(a, lds, lds + kRows * kPW, u % a.nwg_w, u / a.nwg_w);
  }
}

// gW1[n, c] (c < ncols - 1), gb1[n] (c = ncols - 1) and gA[i, j] = dP/dA * (...) from the per-workgroup partials, summed
// in workgroup order; nw / np = 0 (empty batch, or the role did not run) gives zeros
__global__ void dagmlp_reduce_k(const float* __restrict__ partW, int nw, const float* __restrict__ partP, int np,
                                const float* __restrict__ tab, float* __restrict__ gW1, int64_t ld_gw,
                                float* __restrict__ gb1, float* __restrict__ gA, int accumulate, int64_t H, int ncols,
                                int64_t dd, int do_w) {
  const int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x, nW = do_w ? H * ncols : 0;
  if (idx < nW) {
    const int64_t n = idx / ncols;
    const int c = (int)(idx - n * ncols);
    float sum = 0.f;
    for (int p = 0; p < nw; ++p) sum += partW[(int64_t)p * nW + idx];
    if (c == ncols - 1) { if (gb1) gb1[n] = sum; }
    else if (gW1) gW1[n * ld_gw + c] = sum;
    return;
  }
  const int64_t ij = idx - nW;
  if (!gA || ij >= dd) return;
  float sum = 0.f;
  for (int p = 0; p < np; ++p) sum += partP[(int64_t)p * dd + ij];
  if (accumulate) { if (np > 0) gA[ij] = fmaf(sum, tab[dd + ij], gA[ij]); }
  else gA[ij] = np > 0 ? sum * tab[dd + ij] : 0.f;
}

inline bool supported(int64_t d, int64_t H) { return d >= 1 && d <= kMaxD && H >= 1 && H <= (int64_t)1 << 20; }
inline int rows_per_tile(int64_t d) { return (int)((kRows / d) * d); }

struct BwdPlan { int64_t ntiles; int nwg_d, nwg_w, nslab, ncols; };
inline BwdPlan bwd_plan(int64_t B, int64_t d, int64_t H, int hot) {
  BwdPlan p;
  const int64_t spt = kRows / d;
  p.ntiles = (B + spt - 1) / spt;
  p.ncols = (int)((hot ? 2 * d : d) + 1);
  p.nslab = (int)((H + 63) / 64);
  int64_t nw = ((int64_t)1 << 20) / (H * p.ncols);          // <= 4 MB of weight partials
  if (nw > 256) nw = 256;
  if (nw > p.ntiles) nw = p.ntiles;
  if (nw < 1) nw = 1;
  int64_t nd = p.ntiles < 256 ? p.ntiles : 256;
  if (nd < 1) nd = 1;
  p.nwg_w = (int)nw; p.nwg_d = (int)nd;
  return p;
}

inline bool dword(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 3) == 0; }

int launch_fwd(FwdArgs& a, hipStream_t st) {
  const int64_t NT = (a.H + 15) / 16, ny = (NT + kSlab - 1) / kSlab;
  if (ny > 65535) return GNF_ESHAPE;
  const int64_t gx = a.ntiles < 8192 ? a.ntiles : 8192;
  hipLaunchKernelGGL(dagmlp_fwd_k, dim3((unsigned)gx, (unsigned)ny), dim3(kT), 0, st, a);
  GNF_LAUNCH_CHECK();
  return 0;
}

}  // namespace

extern "C" {

int gnf_dagmlp_supported(int64_t d, int64_t H) { return supported(d, H) ? 1 : 0; }

int gnf_dagmlp_gated_fwd(const float* x, const float* A, float* tab, int imp_mode, int gate_mode, float h_thresh,
                         float temperature, const float* u1, const float* u2, uint64_t seed, uint64_t offset,
                         const float* W1, int64_t ld_w, const float* b1, int hot, int relu, float* a1, int64_t B, int64_t d,
                         int64_t H, gnf_stream_t stream) {
  if (d <= 0 || H <= 0 || B < 0) return GNF_EINVAL;
  if (!supported(d, H)) return GNF_ESHAPE;
  if (((!x || !a1) && B > 0) || !A || !tab || !W1 || !b1 || imp_mode < 0 || imp_mode > 3 || gate_mode < 0 || gate_mode > 2 ||
      ld_w < (hot ? 2 * d : d))
    return GNF_EINVAL;
  if (gate_mode == 1 && u1 && !u2) return GNF_EINVAL;
  if (!dword(x) || !dword(A) || !dword(tab) || !dword(u1) || !dword(u2) || !dword(W1) || !dword(b1) || !dword(a1))
    return GNF_EINVAL;
  if (imp_mode == 0) gate_mode = 0;
  hipStream_t st = (hipStream_t)stream;
  int rc = launch_tab(A, tab, imp_mode, h_thresh, temperature, d, st);      // (also for B == 0: the backward reads dP/dA)
  if (rc || B == 0) return rc;
  FwdArgs a{};
  a.s.x = x; a.s.tab = tab; a.s.gate_mode = gate_mode; a.s.T = temperature; a.s.u1 = u1; a.s.u2 = u2; a.s.seed = seed;
  a.s.offset = offset; a.s.B = B; a.s.d = d; a.s.M = B * d; a.s.rpt = rows_per_tile(d);
  a.W1 = W1; a.ld_w = ld_w; a.b1 = b1; a.hot = hot ? 1 : 0; a.relu = relu ? 1 : 0; a.a1 = a1; a.H = H;
  a.ntiles = (a.s.M + a.s.rpt - 1) / a.s.rpt;
  return launch_fwd(a, st);
}

int gnf_dagmlp_rows_fwd(const float* x, const float* P, int64_t ld_p, const int32_t* rows, int64_t R, const float* W1,
                        int64_t ld_w, const float* b1, int hot, int relu, float* a1, int variable_major, int64_t B,
                        int64_t d, int64_t H, gnf_stream_t stream) {
  if (d <= 0 || H <= 0 || B < 0 || R < 0) return GNF_EINVAL;
  if (!supported(d, H)) return GNF_ESHAPE;
  if (((!x || !a1) && B > 0 && R > 0) || !P || !W1 || !b1 || ld_p < d || ld_w < (hot ? 2 * d : d) || (!rows && R > d))
    return GNF_EINVAL;
  if (!dword(x) || !dword(P) || !dword(rows) || !dword(W1) || !dword(b1) || !dword(a1)) return GNF_EINVAL;
  if (B == 0 || R == 0) return 0;
  FwdArgs a{};
  a.s.x = x; a.s.P = P; a.s.ld_p = ld_p; a.s.rows = rows; a.s.R = R; a.s.vm = variable_major ? 1 : 0;
  a.s.B = B; a.s.d = d; a.s.M = B * R; a.s.rpt = kRows;
  a.W1 = W1; a.ld_w = ld_w; a.b1 = b1; a.hot = hot ? 1 : 0; a.relu = relu ? 1 : 0; a.a1 = a1; a.H = H;
  a.ntiles = (a.s.M + kRows - 1) / kRows;
  return launch_fwd(a, (hipStream_t)stream);
}

int64_t gnf_dagmlp_gated_bwd_ws_bytes(int64_t B, int64_t d, int64_t H) {
  if (!supported(d, H) || B < 0) return GNF_ESHAPE;
  const BwdPlan p = bwd_plan(B, d, H, 1), q = bwd_plan(B, d, H, 0);          // with and without the one-hot half
  const int64_t wp = (int64_t)p.nwg_w * H * p.ncols, wq = (int64_t)q.nwg_w * H * q.ncols;
  return ((wp > wq ? wp : wq) + (int64_t)p.nwg_d * d * d + 4) * (int64_t)sizeof(float);
}

int gnf_dagmlp_gated_bwd(const float* x, const float* tab, int imp_mode, int gate_mode, float temperature, const float* u1,
                         const float* u2, uint64_t seed, uint64_t offset, const float* W1, int64_t ld_w, int hot,
                         const float* g, float* gx, float* gA, int accumulate, float* gW1, int64_t ld_gw, float* gb1,
                         void* ws, int64_t ws_bytes, int64_t B, int64_t d, int64_t H, gnf_stream_t stream) {
  if (d <= 0 || H <= 0 || B < 0) return GNF_EINVAL;
  if (!supported(d, H)) return GNF_ESHAPE;
  const int64_t kw = hot ? 2 * d : d;
  if (((!x || !g) && B > 0) || !tab || !W1 || !ws || imp_mode < 0 || imp_mode > 3 || gate_mode < 0 || gate_mode > 2 ||
      ld_w < kw || (gW1 && ld_gw < kw))
    return GNF_EINVAL;
  if (gate_mode == 1 && u1 && !u2) return GNF_EINVAL;
  if (!dword(x) || !dword(tab) || !dword(u1) || !dword(u2) || !dword(W1) || !dword(g) || !dword(gx) || !dword(gA) ||
      !dword(gW1) || !dword(gb1) || !dword(ws))
    return GNF_EINVAL;
  if (ws_bytes < gnf_dagmlp_gated_bwd_ws_bytes(B, d, H)) return GNF_EWS;
  if (imp_mode == 0) gate_mode = 0;
  hipStream_t st = (hipStream_t)stream;
  const BwdPlan p = bwd_plan(B, d, H, hot ? 1 : 0);
  const bool do_w = gW1 || gb1, do_d = gx || gA;
  float* partW = static_cast<float*>(ws);
  float* partP = partW + (int64_t)p.nwg_w * H * p.ncols;
  const int nwg_d = do_d ? p.nwg_d : 0;
  if (B > 0 && (do_w || do_d)) {
    BwdArgs a{};
    a.s.x = x; a.s.tab = tab; a.s.gate_mode = gate_mode; a.s.T = temperature; a.s.u1 = u1; a.s.u2 = u2; a.s.seed = seed;
    a.s.offset = offset; a.s.B = B; a.s.d = d; a.s.M = B * d; a.s.rpt = rows_per_tile(d);
    a.W1 = W1; a.ld_w = ld_w; a.hot = hot ? 1 : 0; a.g = g; a.gx = gx; a.partP = partP; a.partW = partW; a.H = H;
    a.ntiles = p.ntiles; a.nwg_d = nwg_d; a.nwg_w = p.nwg_w; a.ncols = p.ncols; a.want_p = gA ? 1 : 0;
    const int64_t grid = nwg_d + (do_w ? (int64_t)p.nwg_w * p.nslab : 0);
    hipLaunchKernelGGL(dagmlp_gated_bwd_k, dim3((unsigned)grid), dim3(kT), 0, st, a);
    GNF_LAUNCH_CHECK();
  }
  if (do_w || gA) {
    const int64_t total = (do_w ? H * p.ncols : 0) + (gA ? d * d : 0);
    hipLaunchKernelGGL(dagmlp_reduce_k, dim3((unsigned)((total + kT - 1) / kT)), dim3(kT), 0, st, (const float*)partW,
                       B > 0 ? p.nwg_w : 0, (const float*)partP, B > 0 ? nwg_d : 0, tab, gW1, ld_gw, gb1, gA, accumulate,
                       H, p.ncols, d * d, do_w ? 1 : 0);
    GNF_LAUNCH_CHECK();
  }
  return 0;
}

}  // extern "C"
