// The split merge of the nearest-neighbour searches (aw_knn: knn.hip, aw_dtw_knn: dtw.hip).  A sweep kernel leaves one
// sorted partial list of k (distance, database index) candidates per (database split, query) in the workspace --
// ws_d / ws_i, element ((split * nq + query) * k + slot), index -1 in an empty slot -- and knn_merge_kernel picks the
// k smallest of a query's splits * k candidates in the lexicographic (distance as computed, index) order, so the result
// does not depend on the split count.  Each including file gets its own copy of the kernel (internal linkage).
#pragma once
#include "common.h"

namespace {

constexpr int KNN_MERGE_THREADS = 256;

// f32 bits -> u32 with the same order as the floats (negatives reversed below the positives)
__device__ __forceinline__ uint32_t knn_ord(float d) {
  const uint32_t u = __float_as_uint(d);
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float knn_unord(uint32_t o) {
  return __uint_as_float((o & 0x80000000u) ? (o & 0x7FFFFFFFu) : ~o);
}

// one wave per query: k selection passes on 64-bit keys (order-preserving distance bits above j).  It also clamps the
// stored distance at 0 and widens idx.
__global__ __launch_bounds__(KNN_MERGE_THREADS) void knn_merge_kernel(const float* __restrict__ ws_d,
                                                                      const int* __restrict__ ws_i, int64_t nq, int k,
                                                                      int splits, int64_t* __restrict__ idx,
                                                                      float* __restrict__ dist) {
  const int lane = threadIdx.x & 63;
  const int64_t qi = (int64_t)blockIdx.x * (KNN_MERGE_THREADS / 64) + (threadIdx.x >> 6);
  if (qi >= nq) return;   // wave-uniform
  const int n = splits * k;
  unsigned long long last = 0;
  bool first = true;
  for (int s = 0; s < k; ++s) {
    unsigned long long best = ~0ull;
    for (int c = lane; c < n; c += 64) {
      const int sp = c / k, e = c - sp * k;
      const int64_t o = ((int64_t)sp * nq + qi) * k + e;
      const int j = ws_i[o];
      if (j >= 0) {
        const unsigned long long key = ((unsigned long long)knn_ord(ws_d[o]) << 32) | (uint32_t)j;
        if ((first || key > last) && key < best) best = key;
      }
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
      const uint32_t lo = __shfl_xor((uint32_t)best, off, 64), hi = __shfl_xor((uint32_t)(best >> 32), off, 64);
      const unsigned long long other = ((unsigned long long)hi << 32) | lo;
      best = other < best ? other : best;
    }
    if (best == ~0ull) {   // fewer than s + 1 eligible rows: the tail is (-1, +inf)
      if (lane == 0)
        for (int r = s; r < k; ++r) {
          idx[qi * k + r] = -1;
          dist[qi * k + r] = __builtin_huge_valf();
        }
      return;
    }
    last = best;
    first = false;
    if (lane == 0) {
      const float d = knn_unord((uint32_t)(best >> 32));
      idx[qi * k + s] = (int64_t)(uint32_t)best;
      dist[qi * k + s] = d > 0.f ? d : 0.f;   // the clamp is on the stored value only, never on the ranking
    }
  }
}

// blocks of knn_merge_kernel for nq queries
inline int64_t knn_merge_blocks(int64_t nq) { return (nq + KNN_MERGE_THREADS / 64 - 1) / (KNN_MERGE_THREADS / 64); }

}  // namespace
