// Next-token choice of the generation loop in one launch (MyTransformerDecoder.generate_ids): column mask,
// temperature, top-k filter, softmax and the greedy / multinomial pick, written straight into the id buffer.
// The reference's loop (model/transformer_decoder.py:203-224) spends topk + masked_fill + softmax + multinomial + cat
// per token on it.
//
// One workgroup of 256 threads per row.  The row lives in LDS as order-preserving 32-bit keys (key(a) < key(b) iff
// a < b, -0 folded into +0), so the k-th largest value is a radix select over four 8-bit digits -- no sort -- and
// "everything strictly below the k-th largest goes" is one unsigned compare that keeps ties, as
// logits[logits < v[:, [-1]]] = -inf does.  The sampling pass then overwrites each key with exp(x - max) and walks the
// row in index order: thread t owns the contiguous chunk t (an odd number of columns, so the 64 lanes of a wave hit
// different LDS banks), a block scan of the chunk sums gives each chunk its offset, and the first column whose
// inclusive prefix exceeds u * total wins.
#include "common.h"

#define SMP_THREADS 256
#define SMP_WAVES (SMP_THREADS / 64)

__device__ __forceinline__ uint32_t smp_key(float x) {
  uint32_t b = __float_as_uint(x);
  if ((b << 1) == 0u) b = 0u;                                   // -0 == +0
  return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}
__device__ __forceinline__ float smp_val(uint32_t k) {
  return __uint_as_float((k & 0x80000000u) ? (k & 0x7FFFFFFFu) : ~k);
}

// The 24-bit draw of counter c = step * B + row under `seed` (include/arcweld_amd.h): the low 24 bits of c go through a
// keyed permutation of [0, 2^24) -- a 4-round Feistel network on two 12-bit halves whose round function is the counter
// hash of the dropout masks -- so the 2^24 counters of one block (c >> 24, which only re-keys the permutation) draw
// 2^24 different values: a seed never repeats a draw within a generation.  The plain top 24 bits of the hash do
// (4096 of them collide somewhere with probability 0.39).
__device__ __forceinline__ uint32_t smp_draw24(uint64_t seed, uint64_t c) {
  const uint64_t key = aw_hash_group(seed, c >> 24);
  uint32_t l = (uint32_t)(c >> 12) & 0xFFFu, r = (uint32_t)c & 0xFFFu;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const uint32_t f = (uint32_t)(aw_hash_group(key + (uint64_t)i, (uint64_t)r) >> 52);
    const uint32_t t = l ^ f;
    l = r;
    r = t;
  }
  return (l << 12) | r;
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

template <int VMAX>
__global__ __launch_bounds__(SMP_THREADS) void sample_next_kernel(
    const float* __restrict__ logits, int B, int V, int n_valid, int top_k, float inv_t, int do_sample, uint64_t seed,
    uint64_t step, int64_t* __restrict__ ids_out, int64_t ld_ids, int64_t col, float* __restrict__ u_out,
    int* __restrict__ bad_count) {
  __shared__ uint32_t keys[VMAX];
  __shared__ int hist[256];
  __shared__ uint32_t red_u[SMP_WAVES];
  __shared__ int red_i[SMP_WAVES];
  __shared__ float red_f[SMP_WAVES];
  __shared__ int s_digit, s_kk;

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int row = blockIdx.x;
  const float* lr = logits + (int64_t)row * V;
  auto imax = [](int a, int b) { return a > b ? a : b; };
  auto imin = [](int a, int b) { return a < b ? a : b; };
  auto umax = [](uint32_t a, uint32_t b) { return a > b ? a : b; };

  const float u = (float)smp_draw24(seed, step * (uint64_t)B + (uint64_t)row) * 0x1p-24f;   // in [0, 1)
  if (tid == 0 && u_out) u_out[row] = u;

  // ---- the allowed columns as keys; NaN and the maximum
  int nan = 0;
  uint32_t kmax = 0u;
  for (int j = tid; j < n_valid; j += SMP_THREADS) {
    const float x = lr[j] * inv_t;
    nan |= (x != x) ? 1 : 0;
    const uint32_t k = smp_key(x);
    keys[j] = k;
    kmax = umax(kmax, k);
  }
  nan = smp_reduce(nan, red_i, imax);
  kmax = smp_reduce(kmax, red_u, umax);          // (its barriers also publish keys[])
  const float xmax = smp_val(kmax);
  if (nan || !(fabsf(xmax) < INFINITY)) {        // block-uniform: a NaN, or no finite maximum to subtract
    if (tid == 0) {
      ids_out[(int64_t)row * ld_ids + col] = -1;
      atomicAdd(bad_count, 1);
    }
    return;
  }

  // ---- top-k: the k-th largest key by radix select, most significant digit first (the greedy pick needs none: the
  //      maximum survives every filter)
  uint32_t thr = 0u;                             // keys >= thr stay
  if (do_sample && top_k > 0 && top_k < n_valid) {
    uint32_t prefix = 0u;
    int kk = top_k;                              // the rank still wanted among the keys that match the prefix
    for (int shift = 24; shift >= 0; shift -= 8) {
      hist[tid] = 0;
      __syncthreads();
      const uint32_t himask = shift == 24 ? 0u : (0xFFFFFFFFu << (shift + 8));
      for (int j = tid; j < n_valid; j += SMP_THREADS) {
        const uint32_t k = keys[j];
        if ((k & himask) == prefix) atomicAdd(&hist[(k >> shift) & 255u], 1);
      }
      __syncthreads();
      const int h = hist[tid];
      int s = h;                                 // suffix sum over the digits >= tid
#pragma unroll
      for (int o = 1; o < 64; o <<= 1) {
        const int t = __shfl_down(s, o, 64);
        if (lane + o < 64) s += t;
      }
      if (lane == 0) red_i[wave] = s;
      __syncthreads();
      for (int w = wave + 1; w < SMP_WAVES; ++w) s += red_i[w];
      if (s >= kk && s - h < kk) {               // exactly one digit holds rank kk
        s_digit = tid;
        s_kk = kk - (s - h);
      }
      __syncthreads();
      prefix |= (uint32_t)s_digit << shift;
      kk = s_kk;
    }
    thr = prefix;
  }

  int id;
  if (!do_sample) {
    // ---- greedy: the first index of the maximum (always above the threshold)
    int first = 0x7FFFFFFF;
    for (int j = tid; j < n_valid; j += SMP_THREADS)
      if (keys[j] == kmax) first = imin(first, j);
    id = smp_reduce(first, red_i, imin);
  } else {
    // ---- multinomial: keys -> exp(x - max) (0 when filtered), chunk sums, offsets, first prefix above u * total
    const int chunk = ((n_valid + SMP_THREADS - 1) / SMP_THREADS) | 1;
    const int j0 = imin(tid * chunk, n_valid), j1 = imin(j0 + chunk, n_valid);
    __syncthreads();                             // the strided readers of keys[] are done
    float part = 0.f;
    int last = -1;                               // last column that is kept and finite
    for (int j = j0; j < j1; ++j) {
      const uint32_t k = keys[j];
      float e = 0.f;
      if (k >= thr) {
        const float x = smp_val(k);
        e = expf(x - xmax);
        if (x > -INFINITY) last = j;
      }
      keys[j] = __float_as_uint(e);
      part += e;
    }
    float incl = part;                           // inclusive scan over the threads, in thread (= index) order
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
      const float t = __shfl_up(incl, o, 64);
      if (lane >= o) incl += t;
    }
    __syncthreads();
    if (lane == 63) red_f[wave] = incl;
    __syncthreads();
    float off = incl - part, total = 0.f;
#pragma unroll
    for (int w = 0; w < SMP_WAVES; ++w) {
      if (w < wave) off += red_f[w];
      total += red_f[w];
    }
    const float target = u * total;
    int found = 0x7FFFFFFF;
    float run = off;
    for (int j = j0; j < j1; ++j) {
      const float e = __uint_as_float(keys[j]);
      run += e;
      if (e > 0.f && run > target) {             // never a filtered column, whatever the offsets' rounding
        found = j;
        break;
      }
    }
    found = smp_reduce(found, red_i, imin);
    last = smp_reduce(last, red_i, imax);
    id = found != 0x7FFFFFFF ? found : last;     // rounding left no prefix above the target: the last allowed one
  }
  if (tid == 0) ids_out[(int64_t)row * ld_ids + col] = (int64_t)id;
}

extern "C" int aw_sample_next(const float* logits, int B, int V, int n_valid, int top_k, float inv_temperature,
                              int do_sample, uint64_t seed, int64_t step, int64_t* ids_out, int64_t ld_ids,
                              int64_t col, float* u_out, int* bad_count, void* stream) {
  AW_REQUIRE(logits && ids_out && bad_count && B >= 0 && V >= 1, "aw_sample_next: bad args");
  AW_REQUIRE(V <= AW_SAMPLE_MAX_V, "aw_sample_next: V = %d exceeds the %d columns a workgroup holds in LDS", V,
             AW_SAMPLE_MAX_V);
  AW_REQUIRE(n_valid >= 1 && n_valid <= V, "aw_sample_next: n_valid = %d outside 1..V = %d", n_valid, V);
  AW_REQUIRE(top_k >= 0 && top_k <= n_valid, "aw_sample_next: top_k = %d outside 0..n_valid = %d", top_k, n_valid);
  AW_REQUIRE(inv_temperature > 0.f && inv_temperature < INFINITY, "aw_sample_next: inv_temperature must be positive");
  AW_REQUIRE(step >= 0 && ld_ids >= 1 && col >= 0 && col < ld_ids, "aw_sample_next: bad step / ld_ids / col");
  if (B == 0) return AW_OK;
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
#define SMP_LAUNCH(VMAX)                                                                                            \
  hipLaunchKernelGGL(sample_next_kernel<VMAX>, dim3(B), dim3(SMP_THREADS), 0, s, logits, B, V, n_valid, top_k,     \
                     inv_temperature, do_sample ? 1 : 0, seed, (uint64_t)step, ids_out, ld_ids, col, u_out, bad_count)
  if (n_valid <= 1024)
    SMP_LAUNCH(1024);
  else if (n_valid <= 4096)
    SMP_LAUNCH(4096);
  else
    SMP_LAUNCH(AW_SAMPLE_MAX_V);
#undef SMP_LAUNCH
  return aw::check_launch("aw_sample_next");
}
