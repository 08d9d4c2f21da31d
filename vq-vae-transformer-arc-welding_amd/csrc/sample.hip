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
#include "sample_common.h"

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

// greedy: the first index of the maximum (always above every threshold)
__device__ __forceinline__ int smp_first_of(const uint32_t* keys, int n, uint32_t kmax, int* red_i) {
  auto imin = [](int a, int b) { return a < b ? a : b; };
  int first = 0x7FFFFFFF;
  for (int j = threadIdx.x; j < n; j += SMP_THREADS)
    if (keys[j] == kmax) first = imin(first, j);
  return smp_reduce(first, red_i, imin);
}

// multinomial: keys -> exp(x - max) (0 below thr), chunk sums, offsets, first prefix above u * total.  Leaves
// e_j in keys[j] (as float bits) and the sum of e over the kept columns in *total_out.
__device__ __forceinline__ int smp_walk(uint32_t* keys, int n_valid, uint32_t thr, float xmax, float u, float* red_f,
                                        int* red_i, float* total_out) {
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  auto imax = [](int a, int b) { return a > b ? a : b; };
  auto imin = [](int a, int b) { return a < b ? a : b; };
  const int chunk = ((n_valid + SMP_THREADS - 1) / SMP_THREADS) | 1;
  const int j0 = imin(tid * chunk, n_valid), j1 = imin(j0 + chunk, n_valid);
  __syncthreads();                               // the strided readers of keys[] are done
  float part = 0.f;
  int last = -1;                                 // last column that is kept and finite
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
  float incl = part;                             // inclusive scan over the threads, in thread (= index) order
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
    if (e > 0.f && run > target) {               // never a filtered column, whatever the offsets' rounding
      found = j;
      break;
    }
  }
  found = smp_reduce(found, red_i, imin);
  last = smp_reduce(last, red_i, imax);
  *total_out = total;
  return found != 0x7FFFFFFF ? found : last;     // rounding left no prefix above the target: the last allowed one
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
  __shared__ int sel[2];

  const int tid = threadIdx.x;
  const int row = blockIdx.x;
  const float* lr = logits + (int64_t)row * V;
  auto imax = [](int a, int b) { return a > b ? a : b; };
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

  // ---- top-k (the greedy pick needs none: the maximum survives every filter)
  uint32_t thr = 0u;                             // keys >= thr stay
  if (do_sample && top_k > 0 && top_k < n_valid) thr = smp_kth_largest(keys, n_valid, top_k, hist, red_i, sel);

  float total;
  const int id = do_sample ? smp_walk(keys, n_valid, thr, xmax, u, red_f, red_i, &total)
                           : smp_first_of(keys, n_valid, kmax, red_i);
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

// ---------------------------------------------------------------- aw_sample_next_ex: + min-p, top-p, logp / logq
// The same launch with two more filters and the likelihood of the pick (semantics: include/arcweld_amd.h).  Every
// filter ends in one key threshold `thr` (keys >= thr stay), so the pick is aw_sample_next's own code.  The nucleus
// threshold is the largest key t with M(t) >= top_p * total, M(t) = the sum of e over the keys >= t: thread i adds its
// strided columns in order (+0 for a key below t), smp_block_sum adds the threads in its fixed tree.  Adding +0 leaves
// a partial sum as it is and f32 addition is monotone in each operand, so M(smallest surviving key) is `total` itself,
// M never grows with t, and a bisection over the key's bits below the common prefix of the smallest and the largest
// surviving key finds t in at most 32 block sums -- no sort, no float atomic, the same bits every launch.  A thread
// keeps key and e of its VMAX / 256 strided columns in registers between the sums (2 x 64 at the largest VMAX, no
// scratch), so a block sum is compare, select, add per column: a second 64 KB LDS array would need dynamic LDS, and
// recomputing expf from the LDS keys in every sum cost 124 us per launch at V 8194.
template <int VMAX>
__global__ __launch_bounds__(SMP_THREADS) void sample_next_ex_kernel(const aw_sample_args a) {
  __shared__ uint32_t keys[VMAX];
  __shared__ int hist[256];
  __shared__ uint32_t red_u[SMP_WAVES];
  __shared__ int red_i[SMP_WAVES];
  __shared__ float red_f[SMP_WAVES];
  __shared__ int sel[2];
  constexpr int EPT = VMAX / SMP_THREADS;        // strided columns per thread at most

  const int tid = threadIdx.x;
  const int row = blockIdx.x;
  const int n_valid = a.n_valid;
  const float* lr = a.logits + (int64_t)row * a.V;
  auto imax = [](int x, int y) { return x > y ? x : y; };
  auto iadd = [](int x, int y) { return x + y; };
  auto umax = [](uint32_t x, uint32_t y) { return x > y ? x : y; };
  auto umin = [](uint32_t x, uint32_t y) { return x < y ? x : y; };
  auto fadd = [](float x, float y) { return x + y; };
  auto fmx = [](float x, float y) { return fmaxf(x, y); };

  const float u = (float)smp_draw24(a.seed, (uint64_t)a.step * (uint64_t)a.B + (uint64_t)row) * 0x1p-24f;
  if (tid == 0 && a.u_out) a.u_out[row] = u;

  // ---- the allowed columns as keys; NaN, the maximum, and the maximum of the raw logits for logp
  int nan = 0;
  uint32_t kmax = 0u;
  float lmax = -INFINITY;
  for (int j = tid; j < n_valid; j += SMP_THREADS) {
    const float l = lr[j], x = l * a.inv_temperature;
    nan |= (x != x) ? 1 : 0;
    const uint32_t k = smp_key(x);
    keys[j] = k;
    kmax = umax(kmax, k);
    lmax = fmaxf(lmax, l);
  }
  nan = smp_reduce(nan, red_i, imax);
  kmax = smp_reduce(kmax, red_u, umax);          // (its barriers also publish keys[])
  const float xmax = smp_val(kmax);
  const int64_t lp_at = (int64_t)row * a.ld_lp + a.col_lp;
  if (nan || !(fabsf(xmax) < INFINITY)) {        // block-uniform: a NaN, or no finite maximum to subtract
    if (tid == 0) {
      const float qnan = __uint_as_float(0x7FC00000u);
      a.ids_out[(int64_t)row * a.ld_ids + a.col] = -1;
      if (a.logp_out) a.logp_out[lp_at] = qnan;
      if (a.logq_out) a.logq_out[lp_at] = qnan;
      if (a.thr_out) a.thr_out[row] = qnan;
      if (a.n_kept_out) a.n_kept_out[row] = 0;
      atomicAdd(a.bad_count, 1);
    }
    return;
  }

  // ---- lse of the raw row (a good row has no NaN and a finite raw maximum: x = l * inv_t with 0 < inv_t < inf)
  float lse = 0.f;
  if (a.logp_out) {
    lmax = smp_reduce(lmax, red_f, fmx);
    float sm = 0.f;
    for (int j = tid; j < n_valid; j += SMP_THREADS) sm += __expf(lr[j] - lmax);
    lse = lmax + logf(smp_reduce(sm, red_f, fadd));
  }

  // ---- the filters, each a cut on the keys (greedy needs none unless their result is asked for)
  uint32_t thr = 0u;                             // keys >= thr stay
  if (a.do_sample || a.n_kept_out || a.thr_out) {
    bool tight = false;                          // thr is the smallest kept key itself, not only a bound below it
    if (a.top_k > 0 && a.top_k < n_valid) {
      thr = smp_kth_largest(keys, n_valid, a.top_k, hist, red_i, sel);
      tight = true;
    }
    if (a.min_p > 0.f) {                         // the maximum has e = 1 > min_p: never empty
      uint32_t lo = 0xFFFFFFFFu;
      for (int j = tid; j < n_valid; j += SMP_THREADS) {
        const uint32_t k = keys[j];
        if (k >= thr && expf(smp_val(k) - xmax) >= a.min_p) lo = umin(lo, k);
      }
      thr = smp_reduce(lo, red_u, umin);
      tight = true;
    }
    if (!tight && (a.top_p < 1.f || a.thr_out)) {
      uint32_t lo = 0xFFFFFFFFu;
      for (int j = tid; j < n_valid; j += SMP_THREADS) lo = umin(lo, keys[j]);
      thr = smp_reduce(lo, red_u, umin);
    }
    if (a.top_p < 1.f && thr != kmax) {
      const int ne = (n_valid + SMP_THREADS - 1) / SMP_THREADS;   // block-uniform: strided columns per thread in use
      uint32_t kv[EPT];                          // this thread's strided columns: key and e, computed once
      float ev[EPT];
#pragma unroll
      for (int i = 0; i < EPT; ++i) {
        const int j = tid + i * SMP_THREADS;
        kv[i] = j < n_valid ? keys[j] : 0u;
        ev[i] = j < n_valid ? expf(smp_val(kv[i]) - xmax) : 0.f;
      }
      auto mass = [&](uint32_t t) {              // M(t), t >= thr; every call adds in the same order
        float s = 0.f;
#pragma unroll
        for (int i = 0; i < EPT; ++i)
          if (i < ne) s += kv[i] >= t ? ev[i] : 0.f;             // (a column past n_valid adds +0 as well)
        return smp_block_sum(s, red_f);
      };
      const float target = a.top_p * mass(thr);  // top_p * total
      const int hb = 31 - __clz(thr ^ kmax);     // the highest bit in which the surviving keys differ
      uint32_t t = hb == 31 ? 0u : kmax & (0xFFFFFFFFu << (hb + 1));
      for (int b = hb; b >= 0; --b) {            // t stays the largest value so far with M(t) >= target
        const uint32_t cand = t | (1u << b);
        if (cand <= thr || (cand <= kmax && mass(cand) >= target)) t = cand;   // block-uniform
      }
      thr = t;                                   // M steps only at keys, so t is one
    }
    if (a.n_kept_out) {
      int n = 0;
      for (int j = tid; j < n_valid; j += SMP_THREADS) n += keys[j] >= thr ? 1 : 0;
      n = smp_reduce(n, red_i, iadd);
      if (tid == 0) a.n_kept_out[row] = n;
    }
    if (tid == 0 && a.thr_out) a.thr_out[row] = smp_val(thr);
  }

  float total = 0.f;
  const int id = a.do_sample ? smp_walk(keys, n_valid, thr, xmax, u, red_f, red_i, &total)
                             : smp_first_of(keys, n_valid, kmax, red_i);
  if (tid == 0) {
    a.ids_out[(int64_t)row * a.ld_ids + a.col] = (int64_t)id;
    if (a.logp_out) a.logp_out[lp_at] = lr[id] - lse;
    if (a.logq_out) a.logq_out[lp_at] = a.do_sample ? logf(__uint_as_float(keys[id]) / total) : 0.f;
  }
}

extern "C" int aw_sample_next_ex(const aw_sample_args* args, void* stream) {
  AW_REQUIRE(args, "aw_sample_next_ex: null args");
  const aw_sample_args& a = *args;
  AW_REQUIRE(a.logits && a.ids_out && a.bad_count && a.B >= 0 && a.V >= 1, "aw_sample_next_ex: bad args");
  AW_REQUIRE(a.V <= AW_SAMPLE_MAX_V, "aw_sample_next_ex: V = %d exceeds the %d columns a workgroup holds in LDS", a.V,
             AW_SAMPLE_MAX_V);
  AW_REQUIRE(a.n_valid >= 1 && a.n_valid <= a.V, "aw_sample_next_ex: n_valid = %d outside 1..V = %d", a.n_valid, a.V);
  AW_REQUIRE(a.top_k >= 0 && a.top_k <= a.n_valid, "aw_sample_next_ex: top_k = %d outside 0..n_valid = %d", a.top_k,
             a.n_valid);
  AW_REQUIRE(a.top_p > 0.f && a.top_p <= 1.f, "aw_sample_next_ex: top_p = %g outside (0, 1]", (double)a.top_p);
  AW_REQUIRE(a.min_p >= 0.f && a.min_p < 1.f, "aw_sample_next_ex: min_p = %g outside [0, 1)", (double)a.min_p);
  AW_REQUIRE(a.inv_temperature > 0.f && a.inv_temperature < INFINITY,
             "aw_sample_next_ex: inv_temperature must be positive");
  AW_REQUIRE(a.step >= 0 && a.ld_ids >= 1 && a.col >= 0 && a.col < a.ld_ids,
             "aw_sample_next_ex: bad step / ld_ids / col");
  AW_REQUIRE(!(a.logp_out || a.logq_out) || (a.ld_lp >= 1 && a.col_lp >= 0 && a.col_lp < a.ld_lp),
             "aw_sample_next_ex: logp_out / logq_out need ld_lp >= 1 and 0 <= col_lp < ld_lp");
  if (a.B == 0) return AW_OK;
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  aw_sample_args k = a;
  k.do_sample = a.do_sample ? 1 : 0;
  if (!(a.logp_out || a.logq_out)) k.ld_lp = k.col_lp = 0;
#define SMP_LAUNCH(VMAX) hipLaunchKernelGGL(sample_next_ex_kernel<VMAX>, dim3(a.B), dim3(SMP_THREADS), 0, s, k)
  if (a.n_valid <= 1024)
    SMP_LAUNCH(1024);
  else if (a.n_valid <= 4096)
    SMP_LAUNCH(4096);
  else
    SMP_LAUNCH(AW_SAMPLE_MAX_V);
#undef SMP_LAUNCH
  return aw::check_launch("aw_sample_next_ex");
}
