// Device functions shared by the row kernels that hold their row in LDS as order-preserving keys: the token pick of
// sample.hip and the beam step of beam.hip.  One workgroup of SMP_THREADS threads per row.
#pragma once
#include "common.h"

#define SMP_THREADS 256
#define SMP_WAVES (SMP_THREADS / 64)

// key(a) < key(b) iff a < b, -0 folded into +0
__device__ __forceinline__ uint32_t smp_key(float x) {
  uint32_t b = __float_as_uint(x);
  if ((b << 1) == 0u) b = 0u;                                   // -0 == +0
  return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}
__device__ __forceinline__ float smp_val(uint32_t k) {
  return __uint_as_float((k & 0x80000000u) ? (k & 0x7FFFFFFFu) : ~k);
}

// block reductions over 4 waves; every thread gets the result.  red: SMP_WAVES words of LDS scratch.
template <typename T, typename F> __device__ __forceinline__ T smp_reduce(T v, T* red, F f) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = f(v, __shfl_xor(v, o, 64));
  __syncthreads();                                              // the previous use of red is over
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  T r = red[0];
#pragma unroll
  for (int w = 1; w < SMP_WAVES; ++w) r = f(r, red[w]);
  return r;
}

// The block sum of the nucleus search: 32 of them in a row, so the wave step runs on DPP (row shifts inside the rows of
// 16 lanes, then lane 15 / 31 broadcast into the rows above: the wave's sum arrives in lane 63) rather than through
// the six dependent LDS-crossbar shuffles of smp_reduce.  A fixed tree like smp_reduce's; every thread gets the sum.
__device__ __forceinline__ float smp_block_sum(float v, float* red) {
#define SMP_DPP(ctrl, rows) \
  __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), ctrl, rows, 0xf, false))
  v += SMP_DPP(0x111, 0xf);                      // row_shr:1 (a lane without a source adds the old value, +0)
  v += SMP_DPP(0x112, 0xf);                      // row_shr:2
  v += SMP_DPP(0x114, 0xf);                      // row_shr:4
  v += SMP_DPP(0x118, 0xf);                      // row_shr:8: lane 15 of a row holds the row's sum
  v += SMP_DPP(0x142, 0xa);                      // row_bcast:15 into rows 1 and 3
  v += SMP_DPP(0x143, 0xc);                      // row_bcast:31 into rows 2 and 3
#undef SMP_DPP
  __syncthreads();                               // the previous use of red is over
  if ((threadIdx.x & 63) == 63) red[threadIdx.x >> 6] = v;
  __syncthreads();
  return (red[0] + red[1]) + (red[2] + red[3]);
}

// The top_k-th largest of keys[0 .. n) (1 <= top_k <= n) by radix select over four 8-bit digits, most significant
// first; every thread gets it.  hist: 256 ints, red_i: SMP_WAVES ints, sel: 2 ints of LDS scratch.
__device__ __forceinline__ uint32_t smp_kth_largest(const uint32_t* keys, int n, int top_k, int* hist, int* red_i,
                                                    int* sel) {
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  uint32_t prefix = 0u;
  int kk = top_k;                                // the rank still wanted among the keys that match the prefix
  for (int shift = 24; shift >= 0; shift -= 8) {
    hist[tid] = 0;
    __syncthreads();
    const uint32_t himask = shift == 24 ? 0u : (0xFFFFFFFFu << (shift + 8));
    for (int j = tid; j < n; j += SMP_THREADS) {
      const uint32_t k = keys[j];
      if ((k & himask) == prefix) atomicAdd(&hist[(k >> shift) & 255u], 1);
    }
    __syncthreads();
    const int h = hist[tid];
    int s = h;                                   // suffix sum over the digits >= tid
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
      const int t = __shfl_down(s, o, 64);
      if (lane + o < 64) s += t;
    }
    if (lane == 0) red_i[wave] = s;
    __syncthreads();
    for (int w = wave + 1; w < SMP_WAVES; ++w) s += red_i[w];
    if (s >= kk && s - h < kk) {                 // exactly one digit holds rank kk
      sel[0] = tid;
      sel[1] = kk - (s - h);
    }
    __syncthreads();
    prefix |= (uint32_t)sel[0] << shift;
    kk = sel[1];
  }
  return prefix;
}
