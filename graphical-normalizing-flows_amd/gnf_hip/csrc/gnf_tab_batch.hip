// Training batches of the tabular driver (train_uci.py) from device memory: the keys whose sort is an epoch's permutation,
// and the gather of one minibatch out of the data set through that permutation.
//
// gnf_shuffle_keys: keys[i] = ((r[i & 3] >> 1) << 32) | i, r the Philox words of counter (i >> 2, 0, offset) under key seed.
// The high word is 31 random bits (keys stay non-negative), the low word is the row: sorting the keys sorts the random words
// and breaks their ties by row, so the low words of the sorted keys are a permutation of 0 .. n-1 whatever the draws.  One
// thread per Philox call: four keys, 32 contiguous bytes.
//
// gnf_tab_batch: output row r is row perm[pos + r*stride] of X, pos = first (+ cursor[0] read from device memory, so that a
// captured launch walks through the epoch as a separate launch advances the cursor between replays).  HBM-bound: 4 B read and
// 4 B written per element, plus ONE 4-byte perm entry per row -- a row is copied by an aligned group of G lanes (G = the
// power of two >= the row's units, at most 64: 4 lanes for POWER's six floats -- a quad and two floats --, 32 for BSDS300's
// 63, 16 for a row of 64 floats as float4), the group's first lane reads the entry and the others take it by a lane shuffle.  Lanes of a group read and
// write consecutive units of one row, groups of a wave consecutive output rows.  (Four rows per group, their entries and
// units loaded before the first store, was slower at [50 000, 64]: profiles/uci_device_batches_ab.txt.)  Position and row index are clamped: a wrong
// cursor prepares a wrong row, never a read outside perm or X.
//
// TWO forms with identical bits (they only move floats): tab_batch_k<true> moves float4 units (d % 4 == 0, ldx % 4 == 0, X
// and x 16-byte aligned); tab_batch_k<false> takes any dword address and any d: the row's d / 4 quads as dwordx4 accesses at
// dword alignment (f32x4u), then its d % 4 last floats singly.  (Single floats throughout: 10.7 us against 9.2 us for
// torch.index_select at [50 000, 63], one wave per row; profiles/uci_device_batches_ab.txt.)
#include "gnf_common.h"

namespace {

constexpr int kTabBlock = 256;

__global__ __launch_bounds__(kTabBlock) void shuffle_keys_k(uint64_t seed, uint64_t offset, int64_t n,
                                                            int64_t* __restrict__ keys) {
  const int64_t q = (int64_t)blockIdx.x * kTabBlock + threadIdx.x;
  const int64_t i0 = 4 * q;
  if (i0 >= n) return;
  uint32_t r[4];
  philox4x32_10((uint32_t)q, 0u, (uint32_t)offset, (uint32_t)(offset >> 32), (uint32_t)seed, (uint32_t)(seed >> 32), r);
#pragma unroll
  for (int h = 0; h < 4; ++h)
    if (i0 + h < n) keys[i0 + h] = (int64_t)(((uint64_t)(r[h] >> 1) << 32) | (uint64_t)(i0 + h));
}

template <bool VEC>
__global__ __launch_bounds__(kTabBlock) void tab_batch_k(const float* __restrict__ X, int64_t n_rows, int units, int64_t ldx,
                                                         const int32_t* __restrict__ perm, int64_t n_perm, int64_t first,
                                                         int64_t stride, const int32_t* __restrict__ cursor,
                                                         float* __restrict__ x, int64_t B, int group_log2) {
  const int G = 1 << group_log2;
  const int64_t t = (int64_t)blockIdx.x * kTabBlock + threadIdx.x;
  const int64_t r = t >> group_log2;                   // whole groups only: kTabBlock is a multiple of every G
  const int lane = (int)(threadIdx.x & (G - 1));
  const bool live = r < B;                             // every lane reaches the shuffle; dead groups move nothing
  int32_t row32 = 0;
  if (lane == 0 && live) {
    // (unsigned: a wild stride next to a cursor wraps into some position instead of overflowing)
    int64_t pos = (int64_t)((uint64_t)first + (uint64_t)r * (uint64_t)stride + (uint64_t)(cursor ? (int64_t)cursor[0] : 0));
    pos = pos < 0 ? 0 : (pos >= n_perm ? n_perm - 1 : pos);       // clamped: never a read outside perm
    row32 = perm ? perm[pos] : (int32_t)pos;
  }
  int64_t row = __shfl(row32, (int)(threadIdx.x & (GNF_WAVE - 1)) & ~(G - 1), GNF_WAVE);
  if (!live) return;
  row = row < 0 ? 0 : (row >= n_rows ? n_rows - 1 : row);         // clamped: never a read outside the data set
  if (VEC) {
    const f32x4* __restrict__ src = reinterpret_cast<const f32x4*>(X + row * ldx);
    f32x4* __restrict__ dst = reinterpret_cast<f32x4*>(x + r * (4 * (int64_t)units));
    for (int j = lane; j < units; j += G) dst[j] = src[j];
  } else {                                             // units = d: d / 4 quads at dword alignment, then d % 4 single floats
    const float* __restrict__ src = X + row * ldx;
    float* __restrict__ dst = x + r * (int64_t)units;
    const int quads = units >> 2, work = quads + (units & 3);
    for (int j = lane; j < work; j += G) {
      if (j < quads) {
        reinterpret_cast<f32x4u*>(dst)[j] = reinterpret_cast<const f32x4u*>(src)[j];
      } else {
        const int e = 4 * quads + (j - quads);
        dst[e] = src[e];
      }
    }
  }
}

inline bool aligned_to(const void* p, uintptr_t a) { return (reinterpret_cast<uintptr_t>(p) & (a - 1)) == 0; }

}  // namespace

extern "C" int gnf_shuffle_keys(uint64_t seed, uint64_t offset, int64_t n, int64_t* keys, gnf_stream_t stream) {
  if (n < 0) return GNF_EINVAL;
  if (n > 0x7fffffffLL) return GNF_ESHAPE;
  if (n == 0) return 0;
  if (!keys || !aligned_to(keys, 8)) return GNF_EINVAL;
  const int64_t quads = (n + 3) >> 2;
  hipLaunchKernelGGL(shuffle_keys_k, dim3((unsigned)((quads + kTabBlock - 1) / kTabBlock)), dim3(kTabBlock), 0,
                     static_cast<hipStream_t>(stream), seed, offset, n, keys);
  GNF_LAUNCH_CHECK();
  return 0;
}

extern "C" int gnf_tab_batch(const float* X, int64_t n_rows, int64_t d, int64_t ldx, const int32_t* perm, int64_t n_perm,
                             int64_t first, int64_t stride, const int32_t* cursor, float* x, int64_t B,
                             gnf_stream_t stream) {
  if (B < 0 || d < 1 || ldx < d || stride < 1 || first < 0) return GNF_EINVAL;
  if (B == 0) return 0;
  if (!X || !x || n_rows < 1 || (perm && n_perm < 1)) return GNF_EINVAL;
  if (!aligned_to(X, 4) || !aligned_to(x, 4) || !aligned_to(perm, 4) || !aligned_to(cursor, 4)) return GNF_EINVAL;
  if (B > 0x7fffffffLL / d) return GNF_ESHAPE;                     // B*d >= 2^31 (B*d == 2^31 - 1 passes)
  const int64_t n_pos = perm ? n_perm : n_rows;                    // the identity runs over the rows
  // without a cursor the last position is known here: first + (B-1)*stride < n_pos, stated without an overflow
  if (!cursor && (first >= n_pos || (B > 1 && stride > (n_pos - 1 - first) / (B - 1)))) return GNF_EINVAL;
  const bool vec = d % 4 == 0 && ldx % 4 == 0 && aligned_to(X, 16) && aligned_to(x, 16);
  const int units = (int)(vec ? d / 4 : d);
  const int work = (int)(vec ? d / 4 : d / 4 + d % 4);             // lanes a row can keep busy at once
  int group_log2 = 0;
  while ((1 << group_log2) < work && group_log2 < 6) ++group_log2;
  const int64_t threads = B << group_log2;                         // < 2^32: G < 2 * units <= 2 d
  const dim3 grid((unsigned)((threads + kTabBlock - 1) / kTabBlock));
  hipStream_t s = static_cast<hipStream_t>(stream);
  if (vec)
    hipLaunchKernelGGL(tab_batch_k<true>, grid, dim3(kTabBlock), 0, s, X, n_rows, units, ldx, perm, n_pos, first, stride,
                       cursor, x, B, group_log2);
  else
    hipLaunchKernelGGL(tab_batch_k<false>, grid, dim3(kTabBlock), 0, s, X, n_rows, units, ldx, perm, n_pos, first, stride,
                       cursor, x, B, group_log2);
  GNF_LAUNCH_CHECK();
  return 0;
}
