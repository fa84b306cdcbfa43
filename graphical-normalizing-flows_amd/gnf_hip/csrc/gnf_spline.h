// The monotone rational-quadratic spline transformer (Durkan et al., Neural Spline Flows, 2019) of ONE element, on a row of
// conditioner outputs that the caller holds in LDS: shared by the streaming kernels of gnf_spline.hip and the per-row
// epilogue of made_prefix_k.
//
//   h[0:K] width logits, h[K:2K] height logits, h[2K:3K-1] derivative logits of the K-1 interior knots
//   w = MIN + (1 - MIN K) softmax,  X_0 = -T, X_k = -T + 2T sum_{j<k} w_j, X_K = T (forced); Y likewise
//   D_0 = D_K = 1, D_k = MIN + softplus(h[2K + k - 1])
//
// ARITHMETIC.  Inputs and outputs are fp32, everything between is fp64.  The map is ill-conditioned where a bin is narrow
// and steep (s = H/W up to 1e3, W down to 2e-3 T): an error of 1e-7 in a knot -- one fp32 rounding of the softmax or of its
// running sum -- moves z by 1e-4 and dz/dh by more, and which of two fp32 evaluations is the worse one is a coin flip per
// element.  In fp64 the only roundings left are those of the outputs.  The kernels stay bound by HBM (gfx950 issues an fp64
// FMA per lane and clock, as it does an unpacked fp32 one): profiles/spline_ab.txt.
//
// No per-thread array anywhere: the K bins are WALKED (running sums, the numbers of the hit bin kept in scalars), so nothing
// is indexed at run time but the row itself and nothing goes to scratch.
//
// Two row layouts (floats):
//   WIDE   (gnf_spline.hip)  component c < 2K at 2c, with 2c + 1 free; c >= 2K at c + 2K: spl_exp_row() writes
//          exp(logit - max) as a DOUBLE over each of the 2K pairs, and the walks read those;
//   NARROW (made_prefix_k)   component c at c, read-only: the walk computes the exponentials again.
#pragma once
#include "gnf_common.h"

constexpr double kSplMin = 1e-3;            // MIN_W = MIN_H = MIN_D
constexpr int kSplMinBins = 2, kSplMaxBins = 32;

template <bool WIDE> __host__ __device__ inline int spl_pos(int c, int K) { return WIDE ? (c < 2 * K ? 2 * c : c + 2 * K) : c; }
template <bool WIDE> __host__ __device__ inline int spl_row_floats(int K) { return WIDE ? 5 * K - 1 : 3 * K - 1; }

struct SplBin {
  int k;
  double X, W, Y, H, D0, D1;                // left knot, width, left height knot, height, derivatives at both ends
  double Pw, pw, Ph, ph;                    // softmax mass in front of the bin and of the bin itself (widths, heights)
};

struct SplRow {                             // what spl_exp_row leaves behind
  double mw, mh, iw, ih;                    // the two maxima, the reciprocals of the two sums of exp(logit - max)
};

__device__ __forceinline__ double spl_ldd(const float* p) { double v; __builtin_memcpy(&v, p, 8); return v; }
__device__ __forceinline__ void spl_std(float* p, double v) { __builtin_memcpy(p, &v, 8); }
__device__ __forceinline__ double spl_softplus(double u) { return u > 30. ? u : log1p(exp(u)); }
__device__ __forceinline__ double spl_sigmoid(double u) { return 1. / (1. + exp(-u)); }
__device__ __forceinline__ bool spl_inside(double v, double T) { return v >= -T && v <= T; }      // false for NaN

// exp(logit j - max of its group), j < 2K
template <bool WIDE>
__device__ __forceinline__ double spl_e(const float* r, int j, int K, const SplRow& a) {
  return WIDE ? spl_ldd(r + 2 * j) : exp((double)r[j] - (j < K ? a.mw : a.mh));
}

template <bool WIDE>
__device__ __forceinline__ SplRow spl_exp_row(float* r, int K) {
  SplRow a;
  float mw = r[spl_pos<WIDE>(0, K)], mh = r[spl_pos<WIDE>(K, K)];
  for (int j = 1; j < K; ++j) { mw = fmaxf(mw, r[spl_pos<WIDE>(j, K)]); mh = fmaxf(mh, r[spl_pos<WIDE>(K + j, K)]); }
  a.mw = mw; a.mh = mh;
  double sw = 0., sh = 0.;
  for (int j = 0; j < K; ++j) {
    const double ew = exp((double)r[spl_pos<WIDE>(j, K)] - a.mw), eh = exp((double)r[spl_pos<WIDE>(K + j, K)] - a.mh);
    if (WIDE) { spl_std(r + 2 * j, ew); spl_std(r + 2 * (K + j), eh); }
    sw += ew; sh += eh;
  }
  a.iw = 1. / sw; a.ih = 1. / sh;
  return a;
}

// the bin of v: by the X knots (forward) or the Y knots (INV): k = #{j in 1..K-1 : v >= knot_j}.  r: after spl_exp_row
template <bool WIDE, bool INV>
__device__ __forceinline__ void spl_find(const float* r, int K, double T, const SplRow& a, double v, SplBin& o) {
  const double cs = 1. - kSplMin * K, T2 = 2. * T;
  double cw = 0., ch = 0., Pw = 0., Ph = 0., Xlo = -T, Ylo = -T;
  for (int j = 0; j < K; ++j) {
    const double pw = spl_e<WIDE>(r, j, K, a) * a.iw, ph = spl_e<WIDE>(r, K + j, K, a) * a.ih;
    cw += kSplMin + cs * pw;
    ch += kSplMin + cs * ph;
    const bool last = j == K - 1;
    const double Xhi = last ? T : T2 * cw - T, Yhi = last ? T : T2 * ch - T;
    if (last || v < (INV ? Yhi : Xhi)) {
      o.k = j; o.X = Xlo; o.W = Xhi - Xlo; o.Y = Ylo; o.H = Yhi - Ylo;
      o.Pw = Pw; o.pw = pw; o.Ph = Ph; o.ph = ph;
      break;
    }
    Xlo = Xhi; Ylo = Yhi; Pw += pw; Ph += ph;
  }
  o.D0 = o.k == 0 ? 1. : kSplMin + spl_softplus((double)r[spl_pos<WIDE>(2 * K + o.k - 1, K)]);
  o.D1 = o.k == K - 1 ? 1. : kSplMin + spl_softplus((double)r[spl_pos<WIDE>(2 * K + o.k, K)]);
}

// z and jac = dz/dx of one element (fp64: the caller rounds); the WIDE row is consumed
__device__ __forceinline__ void spl_forward(float* r, int K, double T, float xf, double& z, double& jac) {
  const double x = xf;
  z = x; jac = 1.;
  if (!spl_inside(x, T)) return;
  const SplRow a = spl_exp_row<true>(r, K);
  SplBin b;
  spl_find<true, false>(r, K, T, a, x, b);
  // true divisions: x = T gives xi = 1 and jac = D_K = 1 exactly, as the tail beyond it
  const double xi = (x - b.X) / b.W, s = b.H / b.W, e = b.D1 + b.D0 - 2. * s;
  const double q = xi * (1. - xi), id = 1. / (s + e * q), om = 1. - xi;
  z = b.Y + b.H * (s * xi * xi + b.D0 * q) * id;
  jac = s * s * (b.D1 * xi * xi + 2. * s * q + b.D0 * om * om) * (id * id);
}

// x of one element
template <bool WIDE>
__device__ __forceinline__ float spl_inverse(float* r, int K, double T, float zf) {
  const double z = zf;
  if (!spl_inside(z, T)) return zf;
  const SplRow a = spl_exp_row<WIDE>(r, K);
  SplBin b;
  spl_find<WIDE, true>(r, K, T, a, z, b);
  const double s = b.H / b.W, e = b.D1 + b.D0 - 2. * s, dl = z - b.Y;
  const double qa = b.H * (s - b.D0) + dl * e, qb = b.H * b.D0 - dl * e, qc = -s * dl;
  const double disc = fmax(qb * qb - 4. * qa * qc, 0.);
  const double xi = 2. * qc / (-qb - sqrt(disc));
  return (float)(xi * b.W + b.X);
}

// Backward of one element: returns dL/dx and leaves dL/dh[c] (fp32) at spl_pos<WIDE>(c) of the WIDE row, c < 3K-1.
// Cotangents: gz on z, gj on jac, gld on log jac (the row's log|det J|), gln on the row's Normal log-density (z gains
// -z gln).  The forward is recomputed.
//   softmax part, c = 2T (1 - MIN K):  gh[j] = p_j (c (g_X [j < k] + g_W [j = k]) - S),  S = c (g_X P_{<k} + g_W p_k)
//   (X_K = T is forced, so the last bin's width is T - X_{K-1} rather than 2T w_{K-1}: the two differ by a constant over
//   j in g_p, which the softmax Jacobian annihilates); heights alike; of the derivative logits only D_k, D_{k+1} get one.
__device__ __forceinline__ float spl_backward(float* r, int K, double T, float xf, float gzf, float gjf, float gldf,
                                              float glnf) {
  const int C = 3 * K - 1;
  const double x = xf, gz = gzf, gj = gjf, gld = gldf, gln = glnf;
  if (!spl_inside(x, T)) {
    for (int j = 0; j < C; ++j) r[spl_pos<true>(j, K)] = 0.f;
    return (float)(gz - x * gln);
  }
  const SplRow a = spl_exp_row<true>(r, K);
  SplBin b;
  spl_find<true, false>(r, K, T, a, x, b);
  const int k = b.k;
  const double W = b.W, H = b.H, D0 = b.D0, D1 = b.D1, iW = 1. / W;
  const double xi = (x - b.X) / W, s = H / W, e = D1 + D0 - 2. * s;
  const double om = 1. - xi, q = xi * om, t12 = 1. - 2. * xi, den = s + e * q;
  const double N = s * xi * xi + D0 * q, M = D1 * xi * xi + 2. * s * q + D0 * om * om;
  const double id = 1. / den, id2 = id * id, id3 = id2 * id;
  const double z = b.Y + H * N * id, jac = s * s * M * id2;
  const double gzt = gz - z * gln, gJ = gj + gld / jac;
  const double den_xi = e * t12, den_s = 1. - 2. * q;
  // partials of z and jac in (xi, s, H, D0, D1); dz/dxi = jac W
  const double dz_ds = H * (xi * xi * den - N * den_s) * id2;
  const double dz_dD0 = H * q * (den - N) * id2, dz_dD1 = -H * N * q * id2;
  const double M_xi = 2. * (D1 * xi + s * t12 - D0 * om);
  const double dJ_dxi = s * s * (M_xi * den - 2. * M * den_xi) * id3;
  const double dJ_ds = (2. * s * M + 2. * s * s * q) * id2 - 2. * s * s * M * den_s * id3;
  const double dJ_dD0 = s * s * (om * om * den - 2. * M * q) * id3, dJ_dD1 = s * s * (xi * xi * den - 2. * M * q) * id3;
  const double gxi = gzt * jac * W + gJ * dJ_dxi;
  const double gs = gzt * dz_ds + gJ * dJ_ds;
  const double gD0 = gzt * dz_dD0 + gJ * dJ_dD0, gD1 = gzt * dz_dD1 + gJ * dJ_dD1;
  const double gx = gxi * iW;
  const double gX = -gx, gW = -(gxi * xi + gs * s) * iW;
  const double gY = gzt, gH = gzt * N * id + gs * iW;
  const double c = 2. * T * (1. - kSplMin * K);
  const double Sw = c * (gX * b.Pw + gW * b.pw), Sh = c * (gY * b.Ph + gH * b.ph);
  for (int j = 0; j < K; ++j) {
    const double pw = spl_ldd(r + 2 * j) * a.iw, ph = spl_ldd(r + 2 * (K + j)) * a.ih;
    r[2 * j] = (float)(pw * (c * (j < k ? gX : (j == k ? gW : 0.)) - Sw));
    r[2 * (K + j)] = (float)(ph * (c * (j < k ? gY : (j == k ? gH : 0.)) - Sh));
  }
  const double u0 = k > 0 ? (double)r[4 * K + k - 1] : 0., u1 = k < K - 1 ? (double)r[4 * K + k] : 0.;
  for (int j = 0; j < K - 1; ++j) r[4 * K + j] = 0.f;
  if (k > 0) r[4 * K + k - 1] = (float)(gD0 * spl_sigmoid(u0));
  if (k < K - 1) r[4 * K + k] = (float)(gD1 * spl_sigmoid(u1));
  return (float)gx;
}
