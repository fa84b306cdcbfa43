// What the two StrADE kernels share (gnf_strade_levels.hip: the forward level sweep of an inversion; gnf_strade_adjoint.hip:
// the transposed sweep of its adjoint): the checked layout, one element of the level-ordered image of mask o W, and the
// tile height -- the adjoint replays the hidden units with the summation order of the sweep that produced x, so both ask
// here.  Everything sits in an anonymous namespace, as the kernels of every unit do.
#pragma once
#include "gnf_made.h"

namespace {

constexpr int kChunkVars = GNF_STRADE_CHUNK_VARS;      // variables whose outputs one output product computes

struct StradePackArgs {
  PackArgs p;
  const float* M[kMaxH + 1];
};

inline int strade_layout(const gnf_strade_net* net, int cond_in, MadeLayout* lay) {
  if (!net) return GNF_EINVAL;
  const int rc = make_layout(&net->made, cond_in, lay);
  if (rc) return rc;
  if (net->nlev < 1 || net->nlev > net->made.d || net->widest < 1 || net->widest > net->made.d) return GNF_EINVAL;
  return 0;
}

inline int strade_fill_pack_args(const gnf_strade_net* net, StradePackArgs* a) {
  if (fill_pack_args(&net->made, &a->p)) return GNF_EINVAL;
  for (int l = 0; l <= net->made.nh; ++l) {
    if (!net->mask[l]) return GNF_EINVAL;
    a->M[l] = net->mask[l];
  }
  return 0;
}

// element e of the level-ordered image of mask o W: rows and columns permuted as pack_elem permutes them (the plan's tables
// stand where the degree tables stand), a masked entry an exact zero whatever the weight holds; biases behind each layer
__device__ __forceinline__ float strade_pack_elem(const StradePackArgs& a, int64_t e) {
  const MadeLayout& L = a.p.lay;
  int l = 0;
  while (l < L.nh && e >= L.w_off[l + 1]) ++l;
  float v = 0.f;
  if (e < L.b_off[l]) {
    const int64_t i = e - L.w_off[l];
    const int r = (int)(i / L.ldw[l]), k = (int)(i - (int64_t)r * L.ldw[l]);
    if (k < L.K[l]) {
      const int64_t src = (int64_t)pack_src_row(a.p, l, r) * L.K[l] + pack_src_col(a.p, l, k);
      v = a.M[l][src] != 0.f ? a.p.W[l][src] : 0.f;
    }
  } else {
    const int r = (int)(e - L.b_off[l]);
    if (r < L.rows[l]) v = a.p.b[l][pack_src_row(a.p, l, r)];
  }
  return v;
}

// LDS of the forward sweep: the partial tiles, a chunk's conditioner outputs [TB][hstride], the activation rows
inline int64_t strade_levels_lds_bytes(const MadeLayout& lay, int TB, int hstride) {
  return 4 * ((int64_t)kRedFloats + round_up(TB * hstride, 4) + (int64_t)TB * lay.A);
}

// batch rows per workgroup of the forward sweep, and *hstride = floats per row of its output buffer: tile_rows on what one
// product computes at most (hidden units of a level, outputs of a chunk), then halved until the tile's rows fit in LDS.
// Decided from (net, cond_in, B) alone: a fixed summation order.  0 where the sweep answers GNF_ESHAPE (a chunk's outputs
// beyond 2^24 floats, or a tile of 4 rows beyond LDS)
inline int strade_tile_rows(const gnf_strade_net* net, const MadeLayout& lay, int64_t B, int* hstride) {
  const gnf_made_net& m = net->made;
  const int nv = net->widest < kChunkVars ? net->widest : kChunkVars;
  *hstride = 0;
  if ((int64_t)nv * m.out > (1 << 24)) return 0;
  const int hs = nv * m.out;
  *hstride = hs;
  gnf_made_net probe = m;
  if (hs > probe.max_new) probe.max_new = hs;
  int TB = tile_rows(&probe, B);
  while (TB > 4 && strade_levels_lds_bytes(lay, TB, hs) > kLdsBytes) TB /= 2;
  if (strade_levels_lds_bytes(lay, TB, hs) > kLdsBytes) return 0;
  return TB;
}

}  // namespace
