// Gate arithmetic of the DAG conditioner (models/Conditionners/DAGConditioner.py:94-166) shared by the gate kernels
// (gnf_dag_gate.hip) and the kernels that build the masked copies themselves (gnf_lenetcnn.hip): importance, the (i, j)
// table, the noise of a column quad, the gate, one element of a masked copy and its derivative.  ONE definition of each,
// so a masked copy built in LDS has the bits gnf_dag_gate_fwd writes to HBM.
#pragma once
#include "gnf_common.h"

namespace {

constexpr int kGateBlock = 256;

__device__ __forceinline__ float sigmoidf(float v) { return 1.f / (1.f + expf(-v)); }

// importance p(A) and dp/dA   (DAG:118-124, :151-153)
__device__ __forceinline__ float importance(float a, int mode, float h_thresh, float* dp_da) {
  if (mode == 0) { *dp_da = 1.f; return a; }
  if (mode == 3) {
    const float a2 = a * a;
    const bool on = a2 > h_thresh;
    *dp_da = on ? 2.f * a : 0.f;
    return on ? a2 : 0.f;
  }
  const float s = sigmoidf(2.f * a * a);
  const float G = 2.f * (s - .5f);
  const float dG = 8.f * a * s * (1.f - s);
  if (mode == 2) {
    const bool on = G > h_thresh;
    *dp_da = on ? dG : 0.f;
    return on ? G : 0.f;
  }
  *dp_da = dG;
  return G;
}

// Per-(i,j) table, built once per call (d*d entries, negligible next to the B*d*d gate work):
//   P  = importance p,   dP = dp/dA,
//   ET = ((1-p+eps)/(p+eps))^(1/T)         Gumbel gate:  z1/(z1+z2) = 1/(1 + ET * (ln u1/ln u2)^(1/T))
//   Q  = (1/(p+eps) + 1/(1-p+eps))/T       d gate/dp = gate (1-gate) Q
// so the per-element work is the noise plus two logarithms (the reference's four logs, two exps and the
// sigmoid collapse algebraically; same value to fp32 rounding, no overflow for large Gumbel draws).
// Entry ij of the four planes tab[0 .. 4 dd); returns dP/dA.
__device__ __forceinline__ float gate_tab_entry(const float* A, float* tab, int imp_mode, float h_thresh, float T,
                                                int64_t ij, int64_t dd) {
  float dpda;
  const float p = importance(A[ij], imp_mode, h_thresh, &dpda);
  const float eps = 1e-6f;
  const float pa = p + eps, pb = 1.f - p + eps;
  tab[ij] = p;
  tab[dd + ij] = dpda;
  tab[2 * dd + ij] = expf((logf(pb) - logf(pa)) / T);
  tab[3 * dd + ij] = (1.f / pa + 1.f / pb) / T;
  return dpda;
}

__global__ void dag_gate_tab_k(const float* __restrict__ A, float* __restrict__ tab, int imp_mode, float h_thresh,
                               float T, int64_t dd) {
  const int64_t ij = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (ij >= dd) return;
  gate_tab_entry(A, tab, imp_mode, h_thresh, T, ij, dd);
}

inline int launch_tab(const float* A, float* tab, int imp_mode, float h_thresh, float T, int64_t d, hipStream_t s) {
  hipLaunchKernelGGL(dag_gate_tab_k, dim3((unsigned)((d * d + kGateBlock - 1) / kGateBlock)), dim3(kGateBlock), 0, s, A,
                     tab, imp_mode, h_thresh, T, d * d);
  GNF_LAUNCH_CHECK();
  return 0;
}

// Noise of the FOUR adjacent columns 4 jq .. 4 jq + 3 of row (b*d + i), one value per column:
//   gate_mode 1 (Gumbel-softmax): v = exp(g2 - g1) = E1 / E2, the ratio of two independent Exp(1) variates.
//     * injected uniforms (parity tests, the reference's draw order u1 then u2):  v = ln u1 / ln u2;
//     * Philox:  E1 / (E1 + E2) is EXACTLY uniform on (0,1), so v = V / (1 - V) with ONE uniform V has exactly the law of
//       the reference's ratio -- one 32-bit word and one division per element instead of two words and two logarithms.
//       One Philox4x32-10 call (the dominant VALU cost of these kernels: 40 quarter-rate integer multiplies) then serves
//       four columns: the counter is the column QUAD (row * ceil(d/4) + jq).
//   gate_mode 2 (noise gate): one standard normal per column; Philox: both Box-Muller outputs of each uniform pair.
// Forward and backward use the same mapping, so the backward regenerates the forward's noise.
// gate_mode 1: the ratio is handed on as numerator v / denominator w (the gate then needs ONE division, see gumbel_gate)
struct Draw4 { float v[4]; float w[4]; };

// (u01_open, the uniform of a Philox word: gnf_common.h, shared with gnf_image_prep.hip)
__device__ __forceinline__ Draw4 draw4(int gate_mode, const float* u1, const float* u2, uint64_t seed, uint64_t offset,
                                       int64_t row, int64_t jq, int64_t d) {
  Draw4 n;
#pragma unroll
  for (int h = 0; h < 4; ++h) { n.v[h] = 0.f; n.w[h] = 1.f; }
  if (gate_mode == 0) return n;
  const int64_t j0 = 4 * jq;
  if (u1) {
#pragma unroll
    for (int h = 0; h < 4; ++h)
      if (j0 + h < d) {
        const float a = u1[row * d + j0 + h];
        if (gate_mode == 1) { n.v[h] = log2f(a); n.w[h] = log2f(u2[row * d + j0 + h]); }      // ln u1 / ln u2 = exp(g2 - g1)
        else n.v[h] = a;
      }
    return n;
  }
  const uint64_t idx = (uint64_t)(row * ((d + 3) / 4) + jq);
  uint32_t r[4];
  philox4x32_10((uint32_t)idx, (uint32_t)(idx >> 32), (uint32_t)offset, (uint32_t)(offset >> 32),
                (uint32_t)seed, (uint32_t)(seed >> 32), r);
  if (gate_mode == 1) {
#pragma unroll
    for (int h = 0; h < 4; ++h) {
      const float V = u01_open(r[h]);
      n.v[h] = V;
      n.w[h] = 1.f - V;
    }
  } else {
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      const float rad = sqrtf(-2.f * logf(u01_open(r[2 * h]))), ang = 6.283185307179586f * u01_open(r[2 * h + 1]);
      n.v[2 * h] = rad * cosf(ang);
      n.v[2 * h + 1] = rad * sinf(ang);
    }
  }
  return n;
}

// four consecutive floats: one 16-B load when the quad is whole and 16-B aligned (vec), scalar loads otherwise
__device__ __forceinline__ void load4(const float* __restrict__ p, int nv, bool vec, float (&o)[4]) {
  if (vec && nv == 4) {
    const float4 t = *reinterpret_cast<const float4*>(p);
    o[0] = t.x; o[1] = t.y; o[2] = t.z; o[3] = t.w;
  } else {
#pragma unroll
    for (int h = 0; h < 4; ++h) o[h] = h < nv ? p[h] : 0.f;
  }
}
__device__ __forceinline__ bool quad_aligned(const float* base, int64_t ld) {
  return ((ld | (int64_t)(reinterpret_cast<uintptr_t>(base) >> 2)) & 3) == 0;
}

// Gumbel-softmax gate z1/(z1+z2) = 1/(1 + ET * v^(1/T)) from the table entry ET and the ratio v = num / den.  For the two
// temperatures the drivers use the ratio is never formed: 1/(1 + ET num/den) = den / (den + ET num) -- ONE IEEE division per
// gate instead of two (a division is ~10 VALU instructions, the two of them cost as much as the gate's share of the Philox
// call: 0.094 -> 0.08 ms forward, 0.111 -> 0.09 ms backward at cfg4).  num, den have the same sign (both logs <= 0, or V and
// 1 - V in (0, 1)); num = 0 -> 1, den = 0 -> 0, as the two-division form.
// Round 5: the one division is v_rcp_f32 (1 ulp) + a multiply instead of the IEEE sequence (~10 VALU instructions with its
// scaling and fix-up): the gate is a random draw compared at 1e-5 relative in the injected-noise parity tests, ~2 ulp is far
// inside that.  Same limits: denominator inf -> gate 0; num = den = 0 -> NaN either way.
__device__ __forceinline__ float gumbel_gate(float ET, float num, float den, float T) {
  if (T == 1.f) return den * __builtin_amdgcn_rcpf(fmaf(ET, num, den));
  if (T == .5f) { const float n2 = num * num, d2 = den * den; return d2 * __builtin_amdgcn_rcpf(fmaf(ET, n2, d2)); }
  const float vT = exp2f(log2f(num / den) / T);
  return 1.f / (1.f + ET * vT);                       // u1 -> 0: gate 0;  u2 -> 0: gate 1 (as the reference)
}

// One element of a masked copy, e[b,i,j] = x[b,j] * gate(b,i,j): xv = x[b,j], (p, et) = the table's P and ET at (i,j),
// (nv, nw) = element j & 3 of the quad's Draw4
__device__ __forceinline__ float gate_copy(int gate_mode, float xv, float p, float et, float nv, float nw, float T) {
  float e;
  if (gate_mode == 0) e = xv * p;
  else e = gate_mode == 1 ? xv * gumbel_gate(et, nv, nw, T) : p * (xv + nv * fabsf(1.f - p));
  return e;
}

// acc + g * de/dp[b,i,j]: one term of dL/dP[i,j] = sum_b dL/de[b,i,j] * de/dp[b,i,j]  (Q = the table's Q at (i,j))
__device__ __forceinline__ float gate_dp_add(int gate_mode, float g, float xv, float p, float ET, float Q, float nv, float nw,
                                             float T, float acc) {
  if (gate_mode == 0) return fmaf(g, xv, acc);
  if (gate_mode == 1) {
    const float s = gumbel_gate(ET, nv, nw, T);
    return fmaf(g * xv, s * (1.f - s) * Q, acc);
  }
  const float om = 1.f - p;
  const float sgn = om > 0.f ? 1.f : (om < 0.f ? -1.f : 0.f);
  return fmaf(g, xv + nv * fabsf(om) - p * nv * sgn, acc);
}

}  // namespace
