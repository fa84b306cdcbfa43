// Structural queries on the dependency graph of a DAG conditioner, on the device: topological levels (the length of the
// longest parent chain of every node), the depth and acyclicity of G graphs on d nodes each, in two launches.
//
// Node j is a parent of node i in graph g when pred_g(M[g, i, j]) holds (include/gnf_hip.h: m != 0, or m > thresholds[g]
// compared in fp32).  The question is integer: the only float operation is the predicate.
//
//   dag_pack_k   many workgroups, one wavefront per (graph, row).  A wavefront turns 64 columns of its row into one 64-bit
//                word with __ballot; lane w keeps word w (d <= 4096: at most 64 words per row), and at the end of the row
//                the lanes 0 .. W-1 store theirs with ordinary stores.  Layout: words[g][w][i] (transposed), so that the
//                peel's thread-per-row reads are coalesced.  The padding bits of the last word are zero.  One more word per
//                row, nz[g][i]: bit w is set when word w of the row is not zero (a second __ballot, stored by lane 0).
//   dag_peel_k   exactly ONE workgroup per graph (blockIdx.x = g): nothing is communicated between workgroups, there is no
//                grid barrier and no wait on memory.  Round k gives level k to every unlevelled row whose words are covered
//                by the mask of the rows levelled in EARLIER rounds.  The mask lives in LDS twice: round k reads
//                mask[k & 1] (levels < k) and ORs into mask[(k + 1) & 1], which holds the levels < k - 1 -- a row levelled
//                in round k sets its bit there at once and in the other copy one round later, so no round reads a bit set
//                in the same round (the result does not depend on the order of the threads) and one barrier per round is
//                enough.  Integer LDS atomicOr / atomicAdd only.
//                The mask only grows, so a word that was covered stays covered: a row keeps a cursor at its first blocking
//                word, holds that word in a register and walks the NONZERO words only (nz): the chain 0 -> 1 -> ... at
//                d = 3072 takes 3.0 ms instead of 12.8, a density-.1 graph 5.7 instead of 5.1.  (Loading the next nonzero
//                word ahead of the cursor as well was measured and dropped: 7.0 ms on that graph.)  The traffic is at most
//                d (W + 1) words, once.  Levels stay in registers until the end: no global store inside the round loop.
//                The round loop is a counted `for` over at most d + 1 rounds (a round that levels nothing ends it; every
//                earlier one levels at least one of the d rows), the cursor loop a counted `for` over at most W + 1 steps:
//                the kernel ends for every input.
#include "gnf_common.h"

namespace {

constexpr int kDagMaxD = 4096;
constexpr int kDagMaxWords = kDagMaxD / 64;
constexpr int kPackBlock = 256;
constexpr int kPeelMaxBlock = 1024;
constexpr int kPeelRows = kDagMaxD / kPeelMaxBlock;      // rows per thread at the largest d

template <typename T, bool THRESH>
__global__ __launch_bounds__(kPackBlock) void dag_pack_k(const T* __restrict__ M, int64_t stride_g, int64_t ld,
                                                         const float* __restrict__ thresholds,
                                                         unsigned long long* __restrict__ words,
                                                         unsigned long long* __restrict__ nz, int d, int W, int row_blocks) {
  const int g = blockIdx.x / row_blocks;
  const int i = (blockIdx.x - g * row_blocks) * (kPackBlock / GNF_WAVE) + (int)(threadIdx.x / GNF_WAVE);
  if (i >= d) return;                                   // whole wavefronts leave: __ballot below sees complete ones
  const int lane = threadIdx.x & (GNF_WAVE - 1);
  const T* __restrict__ row = M + (int64_t)g * stride_g + (int64_t)i * ld;
  float th = 0.f;
  if (THRESH) th = thresholds[g];
  unsigned long long mine = 0ull;
#pragma unroll 4
  for (int w = 0; w < W; ++w) {
    const int j = w * GNF_WAVE + lane;
    bool edge = false;
    if (j < d) {
      const T m = row[j];
      edge = THRESH ? ((float)m > th) : (m != (T)0);    // NaN: no edge above a threshold, an edge for != 0
    }
    const unsigned long long b = __ballot(edge);
    if (lane == w) mine = b;
  }
  const unsigned long long some = __ballot(mine != 0ull);   // lanes >= W hold 0
  if (lane < W) words[((int64_t)g * W + lane) * d + i] = mine;
  if (lane == 0) nz[(int64_t)g * d + i] = some;
}

// index of the first set bit of `nz` above position c (c = -1: from the start), W when there is none
__device__ __forceinline__ int next_word(unsigned long long nz, int c, int W) {
  const unsigned long long m = c >= 63 ? 0ull : nz & (~0ull << (c + 1));
  return m ? __ffsll((long long)m) - 1 : W;
}

__global__ __launch_bounds__(kPeelMaxBlock) void dag_peel_k(const unsigned long long* __restrict__ words,
                                                            const unsigned long long* __restrict__ nz,
                                                            int32_t* __restrict__ level, int32_t* __restrict__ info, int d,
                                                            int W) {
  __shared__ unsigned long long mask[2][kDagMaxWords];
  __shared__ int added[3];
  const int g = blockIdx.x, tid = threadIdx.x, nt = blockDim.x;
  const unsigned long long* __restrict__ wg = words + (int64_t)g * W * d;
  const unsigned long long* __restrict__ nzg = nz + (int64_t)g * d;
  int32_t* __restrict__ lv = level + (int64_t)g * d;
  if (tid < kDagMaxWords) { mask[0][tid] = 0ull; mask[1][tid] = 0ull; }
  if (tid < 3) added[tid] = 0;
  int cur[kPeelRows], lvl[kPeelRows];                   // index of the word under the cursor (W: none left), level
  unsigned long long wd[kPeelRows], nzr[kPeelRows];     // that word, the mask of the row's nonzero words
  unsigned open = 0u, pend = 0u;                        // bit r: row r unlevelled / levelled in the last round
#pragma unroll
  for (int r = 0; r < kPeelRows; ++r) {
    const int i = tid + r * nt;
    cur[r] = W;
    lvl[r] = -1;                                        // stays: on or behind a cycle
    wd[r] = nzr[r] = 0ull;
    if (i < d) {
      open |= 1u << r;
      nzr[r] = nzg[i];
      cur[r] = next_word(nzr[r], -1, W);
      if (cur[r] < W) wd[r] = wg[(int64_t)cur[r] * d + i];
    }
  }
  __syncthreads();
  int n_levelled = 0, n_levels = 0;
  for (int k = 0; k <= d; ++k) {
    const unsigned long long* rd = mask[k & 1];
    unsigned long long* wr = mask[(k + 1) & 1];
    int mine = 0;
#pragma unroll
    for (int r = 0; r < kPeelRows; ++r) {
      const int i = tid + r * nt;
      const unsigned long long bit = 1ull << (i & 63);
      if (pend & (1u << r)) {
        atomicOr(&wr[i >> 6], bit);                     // levelled in round k - 1: the second copy of the mask
        pend &= ~(1u << r);
      } else if (open & (1u << r)) {
        int c = cur[r];
        unsigned long long w = wd[r];
        for (int step = 0; step <= W && c < W; ++step) {
          if (w & ~rd[c]) break;
          c = next_word(nzr[r], c, W);                  // covered for good: on to the next nonzero word
          if (c < W) w = wg[(int64_t)c * d + i];
        }
        cur[r] = c;
        wd[r] = w;
        if (c >= W) {
          lvl[r] = k;
          atomicOr(&wr[i >> 6], bit);
          open &= ~(1u << r);
          pend |= 1u << r;
          ++mine;
        }
      }
    }
    if (mine) atomicAdd(&added[k % 3], mine);
    if (tid == 0) added[(k + 1) % 3] = 0;               // last read after the barrier of round k - 2, next written in k + 1
    __syncthreads();
    const int n = added[k % 3];                         // the same value in every thread: the loop ends for all or none
    if (n == 0) break;
    n_levelled += n;
    ++n_levels;
  }
#pragma unroll
  for (int r = 0; r < kPeelRows; ++r) {
    const int i = tid + r * nt;
    if (i < d) lv[i] = lvl[r];
  }
  if (tid == 0) { info[2 * g] = n_levelled; info[2 * g + 1] = n_levels; }
}

inline bool aligned_to(const void* p, uintptr_t a) { return (reinterpret_cast<uintptr_t>(p) & (a - 1)) == 0; }
inline int words_of(int64_t d) { return (int)((d + 63) / 64); }

template <typename T>
void launch_pack(const void* M, int64_t stride_g, int64_t ld, const float* thresholds, unsigned long long* words,
                 unsigned long long* nz, int64_t G, int d, hipStream_t s) {
  const int W = words_of(d), row_blocks = (d + kPackBlock / GNF_WAVE - 1) / (kPackBlock / GNF_WAVE);
  const dim3 grid((unsigned)(G * row_blocks)), block(kPackBlock);
  if (thresholds)
    hipLaunchKernelGGL((dag_pack_k<T, true>), grid, block, 0, s, static_cast<const T*>(M), stride_g, ld, thresholds, words, nz,
                       d, W, row_blocks);
  else
    hipLaunchKernelGGL((dag_pack_k<T, false>), grid, block, 0, s, static_cast<const T*>(M), stride_g, ld, thresholds, words, nz,
                       d, W, row_blocks);
}

}  // namespace

extern "C" int gnf_dag_levels_supported(int64_t d) { return d >= 1 && d <= kDagMaxD; }

extern "C" int64_t gnf_dag_levels_ws_bytes(int64_t G, int64_t d) {
  if (!gnf_dag_levels_supported(d)) return GNF_ESHAPE;
  if (G < 0) return GNF_EINVAL;
  return G * (words_of(d) + 1) * d * 8;                 // the words of every row, and the mask of its nonzero words
}

extern "C" int gnf_dag_levels(const void* M, int elem_type, int64_t stride_g, int64_t ld, const float* thresholds,
                              int32_t* level, int32_t* info, void* ws, int64_t ws_bytes, int64_t G, int64_t d,
                              gnf_stream_t stream) {
  if (!gnf_dag_levels_supported(d)) return GNF_ESHAPE;
  if (G < 0 || (elem_type != GNF_DAG_ELEM_F32 && elem_type != GNF_DAG_ELEM_U8)) return GNF_EINVAL;
  if (G == 0) return 0;
  if (!M || !level || !info || !ws || ld < d || stride_g < 0) return GNF_EINVAL;
  if (elem_type == GNF_DAG_ELEM_U8 && thresholds) return GNF_EINVAL;
  if ((elem_type == GNF_DAG_ELEM_F32 && !aligned_to(M, 4)) || !aligned_to(thresholds, 4) || !aligned_to(level, 4) ||
      !aligned_to(info, 4) || !aligned_to(ws, 8))
    return GNF_EINVAL;
  const int row_blocks = ((int)d + kPackBlock / GNF_WAVE - 1) / (kPackBlock / GNF_WAVE);
  if (G > 0x7fffffff / row_blocks) return GNF_ESHAPE;
  if (ws_bytes < gnf_dag_levels_ws_bytes(G, d)) return GNF_EWS;
  hipStream_t s = static_cast<hipStream_t>(stream);
  unsigned long long* words = static_cast<unsigned long long*>(ws);
  unsigned long long* nz = words + G * words_of(d) * d;
  if (elem_type == GNF_DAG_ELEM_F32)
    launch_pack<float>(M, stride_g, ld, thresholds, words, nz, G, (int)d, s);
  else
    launch_pack<uint8_t>(M, stride_g, ld, thresholds, words, nz, G, (int)d, s);
  GNF_LAUNCH_CHECK();
  int block = (((int)d + GNF_WAVE - 1) / GNF_WAVE) * GNF_WAVE;
  block = block > kPeelMaxBlock ? kPeelMaxBlock : block;
  hipLaunchKernelGGL(dag_peel_k, dim3((unsigned)G), dim3(block), 0, s, words, nz, level, info, (int)d, words_of(d));
  GNF_LAUNCH_CHECK();
  return 0;
}
