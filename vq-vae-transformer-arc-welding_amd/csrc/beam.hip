// Beam search on the device (MyTransformerDecoder.beam_search_ids): the step that ranks a sequence's W_in * n_valid
// one-token extensions and keeps the best W_out, the reorder of every block's KV cache by the survivors' parents, and
// the walk back through the per-step slabs at the end.  Semantics: include/arcweld_amd.h.
//
// aw_beam_step: one workgroup of 256 threads per sequence.  Each beam row passes through LDS once as raw logits (NaN
// check, maximum, sum of exp: one wave per row, four rows at a time, no barrier) and is overwritten in place by the
// order-preserving keys of its candidates, so the sequence ends up as ONE virtual row of W_in * n_valid keys.  The W_out-th largest key
// comes from sample.hip's radix select; the keys above it are compacted with an integer LDS counter (their order is
// settled afterwards), the keys equal to it are taken in flat-index order through a block scan of per-thread counts
// over contiguous chunks, and one wave ranks the <= 32 winners under (key descending, flat index ascending).  No sort,
// no float atomic: the same inputs give the same bits on every launch.
#include "sample_common.h"

template <int NMAX>
__global__ __launch_bounds__(SMP_THREADS) void beam_step_kernel(const aw_beam_args a) {
  __shared__ uint32_t keys[NMAX];
  __shared__ int hist[256];
  __shared__ int red_i[SMP_WAVES];
  __shared__ int sel[2];
  __shared__ float lse_s[AW_BEAM_MAX_W];
  __shared__ uint32_t win_key[AW_BEAM_MAX_W];
  __shared__ int win_idx[AW_BEAM_MAX_W];
  __shared__ int n_above;

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int b = blockIdx.x;
  const int n_valid = a.n_valid, W_in = a.W_in, W_out = a.W_out;
  const int N = W_in * n_valid;                  // <= NMAX (the launcher picks NMAX)
  auto imax = [](int x, int y) { return x > y ? x : y; };

  if (tid == 0) n_above = 0;                     // (published by the reduction's barriers below)

  // ---- every beam row, one wave each (wave q takes rows q, q + 4, ...): raw logits -> LDS, lse, candidates as keys
  // in place.  A lane only re-reads the columns it wrote itself, and the butterflies leave the same bits in all lanes.
  int bad = 0;
  for (int w = wave; w < W_in; w += SMP_WAVES) { // wave-uniform
    const float* lr = a.logits + (int64_t)(b * W_in + w) * a.ldl;
    const float s = a.scores_in[b * W_in + w];
    uint32_t* row = keys + w * n_valid;
    int nan = (s != s) ? 1 : 0;
    float mx = -INFINITY;
    for (int j = lane; j < n_valid; j += 64) {
      const float l = lr[j];
      nan |= (l != l) ? 1 : 0;
      mx = fmaxf(mx, l);
      row[j] = __float_as_uint(l);
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) mx = fmaxf(mx, __shfl_xor(mx, o, 64));
    if (__any(nan) || !(fabsf(mx) < INFINITY)) { // wave-uniform: a NaN, or no finite maximum to subtract
      bad = 1;
      continue;
    }
    float sm = 0.f;
    for (int j = lane; j < n_valid; j += 64) sm += expf(__uint_as_float(row[j]) - mx);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) sm += __shfl_xor(sm, o, 64);
    const float lse = mx + logf(sm);
    if (lane == 0) lse_s[w] = lse;
    for (int j = lane; j < n_valid; j += 64) row[j] = smp_key(s + (__uint_as_float(row[j]) - lse));
  }
  bad = smp_reduce(bad, red_i, imax);            // (its barriers publish keys[], lse_s[] and n_above)

  float* sc_out = a.scores_out + (int64_t)b * W_out;
  float* lp_out = a.logp_out + (int64_t)b * W_out;
  int* pa_out = a.parent_out + (int64_t)b * W_out;
  int64_t* tk_out = a.token_out + (int64_t)b * W_out;
  if (bad) {
    if (tid < W_out) {
      const float qnan = __uint_as_float(0x7FC00000u);
      sc_out[tid] = qnan;
      lp_out[tid] = qnan;
      pa_out[tid] = tid < W_in ? tid : W_in - 1;
      tk_out[tid] = 0;
    }
    if (tid == 0) atomicAdd(a.bad_count, 1);
    return;
  }

  // ---- the K-th largest candidate
  const int K = W_out < N ? W_out : N;
  const uint32_t thr = smp_kth_largest(keys, N, K, hist, red_i, sel);

  // ---- compaction over contiguous chunks (an odd length: the lanes of a wave start in different LDS banks)
  const int chunk = ((N + SMP_THREADS - 1) / SMP_THREADS) | 1;
  const int j0 = tid * chunk < N ? tid * chunk : N, j1 = j0 + chunk < N ? j0 + chunk : N;
  int n_eq = 0;
  for (int j = j0; j < j1; ++j) {
    const uint32_t k = keys[j];
    if (k > thr) {                               // fewer than K of them in all
      const int slot = atomicAdd(&n_above, 1);
      win_key[slot] = k;
      win_idx[slot] = j;
    }
    n_eq += (k == thr) ? 1 : 0;
  }
  int incl = n_eq;                               // inclusive scan over the threads, in thread (= flat index) order
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const int t = __shfl_up(incl, o, 64);
    if (lane >= o) incl += t;
  }
  __syncthreads();                               // red_i's last readers are done; n_above is final
  if (lane == 63) red_i[wave] = incl;
  __syncthreads();
  int rank_eq = incl - n_eq;                     // the keys == thr before this thread's chunk
  for (int w = 0; w < wave; ++w) rank_eq += red_i[w];
  const int above = n_above;
  const int need = K - above;                    // >= 1: the K-th largest itself equals thr
  if (n_eq > 0 && rank_eq < need) {
    for (int j = j0; j < j1; ++j) {
      if (keys[j] == thr) {
        if (rank_eq < need) {
          win_key[above + rank_eq] = thr;
          win_idx[above + rank_eq] = j;
        }
        ++rank_eq;
      }
    }
  }
  __syncthreads();

  // ---- rank the K winners and store them in order; the slots past them are dead beams
  if (tid < K) {
    const uint32_t k = win_key[tid];
    const int idx = win_idx[tid];
    int r = 0;
    for (int m = 0; m < K; ++m) {
      const uint32_t km = win_key[m];
      r += (km > k || (km == k && win_idx[m] < idx)) ? 1 : 0;
    }
    const int w = idx / n_valid, v = idx - w * n_valid;
    sc_out[r] = smp_val(k);
    lp_out[r] = a.logits[(int64_t)(b * W_in + w) * a.ldl + v] - lse_s[w];     // the logp that went into cand
    pa_out[r] = w;
    tk_out[r] = (int64_t)v;
  } else if (tid < W_out) {
    sc_out[tid] = -INFINITY;
    lp_out[tid] = -INFINITY;
    pa_out[tid] = 0;
    tk_out[tid] = 0;
  }
}

extern "C" int aw_beam_step(const aw_beam_args* args, void* stream) {
  AW_REQUIRE(args, "aw_beam_step: null args");
  const aw_beam_args& a = *args;
  AW_REQUIRE(a.logits && a.scores_in && a.scores_out && a.parent_out && a.token_out && a.logp_out && a.bad_count &&
                 a.B >= 0 && a.V >= 1, "aw_beam_step: bad args");
  AW_REQUIRE(a.W_in >= 1 && a.W_in <= AW_BEAM_MAX_W, "aw_beam_step: W_in = %d outside 1..%d", a.W_in, AW_BEAM_MAX_W);
  AW_REQUIRE(a.W_out >= 1 && a.W_out <= AW_BEAM_MAX_W, "aw_beam_step: W_out = %d outside 1..%d", a.W_out,
             AW_BEAM_MAX_W);
  AW_REQUIRE(a.n_valid >= 1 && a.n_valid <= a.V, "aw_beam_step: n_valid = %d outside 1..V = %d", a.n_valid, a.V);
  AW_REQUIRE(a.ldl >= a.V, "aw_beam_step: ldl = %lld below V = %d", (long long)a.ldl, a.V);
  AW_REQUIRE((int64_t)a.W_in * a.n_valid <= AW_SAMPLE_MAX_V,
             "aw_beam_step: W_in * n_valid = %lld exceeds the %d candidates a workgroup holds in LDS",
             (long long)a.W_in * a.n_valid, AW_SAMPLE_MAX_V);
  AW_REQUIRE((int64_t)a.B * a.W_in < (1ll << 31), "aw_beam_step: B * W_in overflows int");
  if (a.B == 0) return AW_OK;
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  const int N = a.W_in * a.n_valid;
#define BEAM_LAUNCH(NMAX) hipLaunchKernelGGL(beam_step_kernel<NMAX>, dim3(a.B), dim3(SMP_THREADS), 0, s, a)
  if (N <= 1024)
    BEAM_LAUNCH(1024);
  else if (N <= 4096)
    BEAM_LAUNCH(4096);
  else
    BEAM_LAUNCH(AW_SAMPLE_MAX_V);
#undef BEAM_LAUNCH
  return aw::check_launch("aw_beam_step");
}

// ---------------------------------------------------------------- aw_beam_gather
// grid (pieces * rows, n_blocks): a workgroup copies one piece of GATHER_PER_WG units of one destination row's chunk in
// one block's cache.  Pure copy, bound by bytes: every thread keeps GATHER_UNROLL loads in flight before it stores.
#define GATHER_THREADS 256
#define GATHER_UNROLL 4
#define GATHER_PER_WG (GATHER_THREADS * GATHER_UNROLL)

// units [piece * GATHER_PER_WG ..) of a chunk of n units, then every `pieces`-th piece after it (one round when the grid
// was sized for this unit)
template <typename T>
__device__ __forceinline__ void beam_copy_pieces(const T* __restrict__ src, T* __restrict__ dst, int64_t n, int piece,
                                                 int pieces, bool zero) {
  for (int64_t i0 = (int64_t)piece * GATHER_PER_WG + threadIdx.x; i0 - threadIdx.x < n;
       i0 += (int64_t)pieces * GATHER_PER_WG) {
    T v[GATHER_UNROLL];
#pragma unroll
    for (int u = 0; u < GATHER_UNROLL; ++u) {
      const int64_t i = i0 + (int64_t)u * GATHER_THREADS;
      v[u] = T{};
      if (!zero && i < n) v[u] = src[i];
    }
#pragma unroll
    for (int u = 0; u < GATHER_UNROLL; ++u) {
      const int64_t i = i0 + (int64_t)u * GATHER_THREADS;
      if (i < n) dst[i] = v[u];
    }
  }
}

template <typename E>                            // E: the element type by size (uint32_t: f32, uint16_t: bf16)
__global__ __launch_bounds__(GATHER_THREADS) void beam_gather_kernel(
    const void* const* __restrict__ src_tab, void* const* __restrict__ dst_tab, int W_in, int W_out,
    const int* __restrict__ parent, int64_t pitch, int64_t chunk, int pieces, int* __restrict__ bad_count) {
  const int r = blockIdx.x / pieces, piece = blockIdx.x - r * pieces;          // destination row, piece of its chunk
  const int blk = blockIdx.y;
  const int p = parent[r];
  const bool zero = p < 0 || p >= W_in;
  if (zero && piece == 0 && blk == 0 && threadIdx.x == 0) atomicAdd(bad_count, 1);
  const int64_t src_row = zero ? 0 : (int64_t)(r / W_out) * W_in + p;
  const E* s = reinterpret_cast<const E*>(src_tab[blk]) + src_row * pitch;
  E* d = reinterpret_cast<E*>(dst_tab[blk]) + (int64_t)r * pitch;
  constexpr int PER16 = 16 / sizeof(E);
  const bool wide = ((reinterpret_cast<uintptr_t>(src_tab[blk]) | reinterpret_cast<uintptr_t>(dst_tab[blk])) & 15) == 0 &&
                    pitch % PER16 == 0 && chunk % PER16 == 0;                  // block-uniform
  if (wide)
    beam_copy_pieces(reinterpret_cast<const uint4*>(s), reinterpret_cast<uint4*>(d), chunk / PER16, piece, pieces, zero);
  else                                           // several rounds when only a base is misaligned: the grid counts uint4s
    beam_copy_pieces(s, d, chunk, piece, pieces, zero);
}

extern "C" int aw_beam_gather(const void* const* src, void* const* dst, int n_blocks, int B, int W_in, int W_out,
                              const int* parent, int Tmax, int n_pos, int width, int dtype, int* bad_count,
                              void* stream) {
  AW_REQUIRE(src && dst && parent && bad_count && n_blocks >= 1 && n_blocks <= 65535 && B >= 0,
             "aw_beam_gather: bad args");
  AW_REQUIRE(W_in >= 1 && W_in <= AW_BEAM_MAX_W && W_out >= 1 && W_out <= AW_BEAM_MAX_W,
             "aw_beam_gather: W_in = %d, W_out = %d outside 1..%d", W_in, W_out, AW_BEAM_MAX_W);
  AW_REQUIRE(Tmax >= 1 && n_pos >= 0 && n_pos <= Tmax && width >= 1,
             "aw_beam_gather: n_pos = %d outside 0..Tmax = %d, or width = %d < 1", n_pos, Tmax, width);
  AW_REQUIRE(dtype == AW_F32 || dtype == AW_BF16, "aw_beam_gather: dtype must be AW_F32 or AW_BF16");
  if (B == 0 || n_pos == 0) return AW_OK;
  const int64_t pitch = (int64_t)Tmax * width, chunk = (int64_t)n_pos * width;   // in elements
  const int esize = dtype == AW_F32 ? 4 : 2;
  // the grid counts 16-byte units when the pitch and the chunk allow them (the bases are looked at on the device)
  const int per16 = 16 / esize;
  const int64_t units = (pitch % per16 == 0 && chunk % per16 == 0) ? chunk / per16 : chunk;
  const int64_t pieces = (units + GATHER_PER_WG - 1) / GATHER_PER_WG;
  const int64_t rows = (int64_t)B * W_out;
  AW_REQUIRE(pieces * rows < (1ll << 31), "aw_beam_gather: %lld workgroups exceed the grid", (long long)(pieces * rows));
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  const dim3 grid((unsigned)(pieces * rows), (unsigned)n_blocks);
  if (dtype == AW_F32)
    hipLaunchKernelGGL(beam_gather_kernel<uint32_t>, grid, dim3(GATHER_THREADS), 0, s, src, dst, W_in, W_out, parent,
                       pitch, chunk, (int)pieces, bad_count);
  else
    hipLaunchKernelGGL(beam_gather_kernel<uint16_t>, grid, dim3(GATHER_THREADS), 0, s, src, dst, W_in, W_out, parent,
                       pitch, chunk, (int)pieces, bad_count);
  return aw::check_launch("aw_beam_gather");
}

// ---------------------------------------------------------------- aw_beam_backtrack
__global__ __launch_bounds__(64) void beam_backtrack_kernel(const int* __restrict__ parent,
                                                            const int64_t* __restrict__ token,
                                                            const float* __restrict__ logp, int n_new, int B, int W,
                                                            int R, int64_t* __restrict__ ids_out, int64_t ld_ids,
                                                            int64_t col0, float* __restrict__ logp_out,
                                                            int* __restrict__ bad_count) {
  const int h = blockIdx.x * 64 + threadIdx.x;   // hypothesis b * R + j
  if (h >= B * R) return;
  const int b = h / R;
  int cur = h - b * R;
  int64_t* ids = ids_out + (int64_t)h * ld_ids + col0;
  float* lp = logp_out + (int64_t)h * n_new;
  for (int i = n_new - 1; i >= 0; --i) {
    if (cur < 0 || cur >= W) {                   // never an index: the rest of this walk is void
      atomicAdd(bad_count, 1);
      for (; i >= 0; --i) {
        ids[i] = 0;
        lp[i] = __uint_as_float(0x7FC00000u);
      }
      return;
    }
    const int64_t at = ((int64_t)i * B + b) * W + cur;
    ids[i] = token[at];
    lp[i] = logp[at];
    cur = parent[at];
  }
}

extern "C" int aw_beam_backtrack(const int* parent, const int64_t* token, const float* logp, int n_new, int B, int W,
                                 int R, int64_t* ids_out, int64_t ld_ids, int64_t col0, float* logp_out,
                                 int* bad_count, void* stream) {
  AW_REQUIRE(n_new >= 0 && B >= 0 && W >= 1 && W <= AW_BEAM_MAX_W && R >= 1 && R <= W,
             "aw_beam_backtrack: n_new = %d, B = %d, W = %d, R = %d: need n_new, B >= 0 and 1 <= R <= W <= %d", n_new, B,
             W, R, AW_BEAM_MAX_W);
  if (n_new == 0 || B == 0) return AW_OK;
  AW_REQUIRE(parent && token && logp && ids_out && logp_out && bad_count, "aw_beam_backtrack: null pointer");
  AW_REQUIRE(col0 >= 0 && ld_ids >= col0 + n_new, "aw_beam_backtrack: ld_ids = %lld below col0 + n_new = %lld",
             (long long)ld_ids, (long long)(col0 + n_new));
  AW_REQUIRE((int64_t)B * R < (1ll << 31), "aw_beam_backtrack: B * R overflows int");
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  hipLaunchKernelGGL(beam_backtrack_kernel, dim3((B * R + 63) / 64), dim3(64), 0, s, parent, token, logp, n_new, B, W,
                     R, ids_out, ld_ids, col0, logp_out, bad_count);
  return aw::check_launch("aw_beam_backtrack");
}
