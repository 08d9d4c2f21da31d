// Scoring of measured cycles (arcweld.generate.score_cycles, MyTransformerDecoder.score_ids): what the trained models
// say about ids and windows that were measured, not generated.
//
// aw_score_rows: teacher-forced scoring of the lm-head logits in one launch -- per row the target's log-probability,
// its rank and the entropy of the row's softmax over the allowed columns, per group of rows (one cycle) the summed
// negative log-likelihood.  torch spends log_softmax + gather + a comparison count + an entropy + the reshaped sums on
// it: five or more launches and three (R, V) temporaries for one pass over each row.
//
// One workgroup per (sequence, group), one wave per row, the waves striding over the group's rows.  Rows of up to
// 64 * NC allowed columns live in registers with all loads issued at once and the wave's next row in flight while this
// one reduces (ce_fwd_rows_kernel's form, csrc/transformer.hip); wider rows are walked twice from global memory (max,
// then sums: the second walk hits the cache).  A wave sums the log-probabilities of its own rows in row order, lane 0
// leaves the sum in the wave's LDS slot and thread 0 adds the slots in wave order: no floating-point atomics, the
// same bits every launch.  LDS use: one float and one int per wave, whatever V.
//
// aw_window_sqerr: mean squared difference per window, the second operand optionally gathered by row ids (the
// quantisation error of a cycle: encoder rows against their codebook rows).  One workgroup per window.
#include <algorithm>

#include "common.h"

#define SCR_WAVES 16

__device__ __forceinline__ float scr_nan() { return __uint_as_float(0x7FC00000u); }

// the group's sum and bad-row count from the per-wave partials; one integer atomic per workgroup at most
__device__ __forceinline__ void scr_finish(float acc, int nb, float* part, int* nbad, float* __restrict__ group_nll,
                                           int* __restrict__ bad) {
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6, nw = blockDim.x >> 6;
  if (lane == 0) {
    part[wv] = acc;
    nbad[wv] = nb;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    float s = 0.f;
    int n = 0;
    for (int w = 0; w < nw; ++w) {
      s += part[w];
      n += nbad[w];
    }
    group_nll[blockIdx.x] = -s;
    if (n) atomicAdd(bad, n);
  }
}

// rows of n_valid <= 64 * NC allowed columns
template <int NC>
__global__ __launch_bounds__(64 * SCR_WAVES) void score_rows_kernel(
    const float* __restrict__ logits, int64_t ldl, int n_valid, const int64_t* __restrict__ targets, int seq_rows,
    int groups, int group_rows, float* __restrict__ logp, int* __restrict__ rank, float* __restrict__ entropy,
    float* __restrict__ group_nll, int* __restrict__ bad) {
  __shared__ float part[SCR_WAVES];
  __shared__ int nbad[SCR_WAVES];
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6, nw = blockDim.x >> 6;
  const int64_t b = blockIdx.x / groups;
  const int c = (int)(blockIdx.x - b * groups);
  const int64_t row0 = b * seq_rows + (int64_t)c * group_rows;   // the group's first logits row
  const int64_t out0 = (int64_t)blockIdx.x * group_rows;         // ... and its first target / output
  const float ninf = -__builtin_huge_valf();
  float acc = 0.f;
  int nb = 0;
  float nv[NC];
  int64_t ny = -1;
  auto load = [&](int i) {   // row i of the group: its allowed columns and its target, one row ahead of their use
#pragma unroll
    for (int k = 0; k < NC; ++k) {
      const int j = lane + 64 * k;
      nv[k] = (i < group_rows && j < n_valid) ? logits[(row0 + i) * ldl + j] : ninf;
    }
    ny = i < group_rows ? targets[out0 + i] : -1;
  };
  int i = wv;
  load(i);
  for (; i < group_rows; i += nw) {
    float v[NC];
#pragma unroll
    for (int k = 0; k < NC; ++k) v[k] = nv[k];
    const int64_t t = ny;
    load(i + nw);
    float mx = ninf;
    bool nan = false;
#pragma unroll
    for (int k = 0; k < NC; ++k) {
      mx = fmaxf(mx, v[k]);
      nan |= v[k] != v[k];
    }
    mx = wave_max(mx);
    const bool y_ok = t >= 0 && t < (int64_t)n_valid;            // checked before it selects anything
    if (__ballot(nan) != 0ull || !(fabsf(mx) < INFINITY) || !y_ok) {   // wave-uniform
      if (lane == 0) {
        logp[out0 + i] = scr_nan();
        rank[out0 + i] = -1;
        entropy[out0 + i] = scr_nan();
      }
      acc = scr_nan();
      ++nb;
      continue;
    }
    // sum of e = exp(l - mx) and of e (l - mx): entropy = lse - sum p l = log(sum e) - sum e (l - mx) / sum e
    float sm = 0.f, tw = 0.f;
#pragma unroll
    for (int k = 0; k < NC; ++k) {
      const float d = v[k] - mx, e = __expf(d);                  // -inf (excluded, or a -inf logit) -> 0
      sm += e;
      tw += e > 0.f ? e * d : 0.f;
    }
    sm = wave_sum(sm);
    tw = wave_sum(tw);
    const float lsm = logf(sm);
    // the target's logit from the registers of the lane that holds it
    const int ys = (int)t, tk = ys >> 6;
    float tv = v[0];
#pragma unroll
    for (int k = 1; k < NC; ++k) tv = k == tk ? v[k] : tv;
    const float ly = __shfl(tv, ys & 63, 64);
    int above = 0;                                               // columns that greedy decoding prefers to the target
#pragma unroll
    for (int k = 0; k < NC; ++k) {
      const int j = lane + 64 * k;
      above += __popcll(__ballot(v[k] > ly || (v[k] == ly && j < ys)));
    }
    const float lp = ly - (mx + lsm);
    if (lane == 0) {
      logp[out0 + i] = lp;
      rank[out0 + i] = above;
      entropy[out0 + i] = lsm - tw / sm;
    }
    acc += lp;
  }
  scr_finish(acc, nb, part, nbad, group_nll, bad);
}

// rows of any width, read from global memory twice
__global__ __launch_bounds__(64 * SCR_WAVES) void score_rows_wide_kernel(
    const float* __restrict__ logits, int64_t ldl, int n_valid, const int64_t* __restrict__ targets, int seq_rows,
    int groups, int group_rows, float* __restrict__ logp, int* __restrict__ rank, float* __restrict__ entropy,
    float* __restrict__ group_nll, int* __restrict__ bad) {
  __shared__ float part[SCR_WAVES];
  __shared__ int nbad[SCR_WAVES];
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6, nw = blockDim.x >> 6;
  const int64_t b = blockIdx.x / groups;
  const int c = (int)(blockIdx.x - b * groups);
  const int64_t row0 = b * seq_rows + (int64_t)c * group_rows;
  const int64_t out0 = (int64_t)blockIdx.x * group_rows;
  const float ninf = -__builtin_huge_valf();
  float acc = 0.f;
  int nb = 0;
  for (int i = wv; i < group_rows; i += nw) {
    const float* lr = logits + (row0 + i) * ldl;
    const int64_t t = targets[out0 + i];
    float mx = ninf;
    bool nan = false;
#pragma unroll 4
    for (int j = lane; j < n_valid; j += 64) {
      const float x = lr[j];
      mx = fmaxf(mx, x);
      nan |= x != x;
    }
    mx = wave_max(mx);
    const bool y_ok = t >= 0 && t < (int64_t)n_valid;
    if (__ballot(nan) != 0ull || !(fabsf(mx) < INFINITY) || !y_ok) {
      if (lane == 0) {
        logp[out0 + i] = scr_nan();
        rank[out0 + i] = -1;
        entropy[out0 + i] = scr_nan();
      }
      acc = scr_nan();
      ++nb;
      continue;
    }
    const int ys = (int)t;
    const float ly = lr[ys];
    float sm = 0.f, tw = 0.f;
    int above = 0;
#pragma unroll 4
    for (int j = lane; j < n_valid; j += 64) {
      const float x = lr[j], d = x - mx, e = __expf(d);
      sm += e;
      tw += e > 0.f ? e * d : 0.f;
      above += (x > ly || (x == ly && j < ys)) ? 1 : 0;
    }
    sm = wave_sum(sm);
    tw = wave_sum(tw);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) above += __shfl_xor(above, o, 64);
    const float lsm = logf(sm);
    const float lp = ly - (mx + lsm);
    if (lane == 0) {
      logp[out0 + i] = lp;
      rank[out0 + i] = above;
      entropy[out0 + i] = lsm - tw / sm;
    }
    acc += lp;
  }
  scr_finish(acc, nb, part, nbad, group_nll, bad);
}

extern "C" int aw_score_rows(const float* logits, int64_t ldl, int V, int n_valid, const int64_t* targets,
                             int64_t n_seq, int seq_rows, int groups, int group_rows, float* logp, int* rank,
                             float* entropy, float* group_nll, int* bad_count, void* stream) {
  AW_REQUIRE(logits && targets && logp && rank && entropy && group_nll && bad_count && n_seq >= 0,
             "aw_score_rows: bad args");
  AW_REQUIRE(V >= 1 && ldl >= V, "aw_score_rows: V = %d, ldl = %lld: need 1 <= V <= ldl", V, (long long)ldl);
  AW_REQUIRE(n_valid >= 1 && n_valid <= V, "aw_score_rows: n_valid = %d outside 1..V = %d", n_valid, V);
  AW_REQUIRE(groups >= 1 && group_rows >= 1 && (int64_t)groups * group_rows <= (int64_t)seq_rows,
             "aw_score_rows: groups %d x group_rows %d must lie within the %d rows of a sequence", groups, group_rows,
             seq_rows);
  AW_REQUIRE(n_seq * groups <= 0x7FFFFFFFll, "aw_score_rows: n_seq * groups too large");
  if (n_seq == 0) return AW_OK;
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  const dim3 gr((unsigned)(n_seq * groups)), bl(64 * (unsigned)std::min(group_rows, SCR_WAVES));
#define SCR_ARGS logits, ldl, n_valid, targets, seq_rows, groups, group_rows, logp, rank, entropy, group_nll, bad_count
#define SCR_LAUNCH(NC)                                                               \
  {                                                                                  \
    hipLaunchKernelGGL(score_rows_kernel<NC>, gr, bl, 0, s, SCR_ARGS);               \
    return aw::check_launch("aw_score_rows");                                        \
  }
  if (n_valid <= 64) SCR_LAUNCH(1)
  if (n_valid <= 256) SCR_LAUNCH(4)
  if (n_valid <= 512) SCR_LAUNCH(8)
  if (n_valid <= 576) SCR_LAUNCH(9)
  if (n_valid <= 1024) SCR_LAUNCH(16)
#undef SCR_LAUNCH
  hipLaunchKernelGGL(score_rows_wide_kernel, gr, bl, 0, s, SCR_ARGS);
#undef SCR_ARGS
  return aw::check_launch("aw_score_rows");
}

// ---------------------------------------------------------------- per-window mean squared error
#define WSE_THREADS 256

// VEC 4: width % 4 == 0 and every row 16-byte aligned (a float4 never straddles two rows); VEC 1: anything
template <int VEC>
__global__ __launch_bounds__(WSE_THREADS) void window_sqerr_kernel(
    const float* __restrict__ a, const float* __restrict__ b, const int64_t* __restrict__ idx, int64_t n_idx_rows,
    int rows, int width, float* __restrict__ out, int* __restrict__ bad) {
  __shared__ float part[WSE_THREADS / 64];
  __shared__ int nbad[WSE_THREADS / 64];
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int64_t w = blockIdx.x, r0 = w * rows;
  const int64_t n = (int64_t)rows * width;
  float acc = 0.f;
  int nb = 0;
  for (int64_t e = (int64_t)threadIdx.x * VEC; e < n; e += WSE_THREADS * VEC) {
    const int64_t rr = e / width;
    const int cc = (int)(e - rr * width);
    int64_t br = r0 + rr;
    if (idx) {
      const int64_t id = idx[r0 + rr];
      if (id < 0 || id >= n_idx_rows) {              // never used as an index; counted by the row's first column
        nb += cc == 0 ? 1 : 0;
        continue;
      }
      br = id;
    }
    const float* pa = a + (r0 + rr) * width + cc;
    const float* pb = b + br * width + cc;
    if (VEC == 4) {
      const f32x4 x = *(const f32x4*)pa, y = *(const f32x4*)pb;
      const f32x4 d = x - y;
      acc += (d.x * d.x + d.y * d.y) + (d.z * d.z + d.w * d.w);
    } else {
      const float d = *pa - *pb;
      acc += d * d;
    }
  }
  acc = wave_sum(acc);
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) nb += __shfl_xor(nb, o, 64);
  if (lane == 0) {
    part[wv] = acc;
    nbad[wv] = nb;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    const float s = (part[0] + part[1]) + (part[2] + part[3]);
    const int k = (nbad[0] + nbad[1]) + (nbad[2] + nbad[3]);
    out[w] = k ? scr_nan() : s / (float)n;
    if (k) atomicAdd(bad, k);
  }
}

extern "C" int aw_window_sqerr(const float* a, const float* b, const int64_t* idx, int64_t n_idx_rows,
                               int64_t windows, int rows_per_window, int width, float* out, int* bad_count,
                               void* stream) {
  AW_REQUIRE(a && b && out && bad_count && windows >= 0 && rows_per_window >= 1 && width >= 1,
             "aw_window_sqerr: bad args");
  AW_REQUIRE(!idx || n_idx_rows >= 1, "aw_window_sqerr: idx needs the row count of b (n_idx_rows >= 1)");
  AW_REQUIRE(windows <= 0x7FFFFFFFll, "aw_window_sqerr: too many windows");
  if (windows == 0) return AW_OK;
  int rows = rows_per_window;
  if (!idx && (int64_t)rows * width <= 0x7FFFFFFFll) {   // no gather: a window is one contiguous row of both
    width *= rows;
    rows = 1;
  }
  const bool vec = width % 4 == 0 && (((uintptr_t)a | (uintptr_t)b) & 15u) == 0;
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  if (vec)
    hipLaunchKernelGGL(window_sqerr_kernel<4>, dim3((unsigned)windows), dim3(WSE_THREADS), 0, s, a, b, idx,
                       n_idx_rows, rows, width, out, bad_count);
  else
    hipLaunchKernelGGL(window_sqerr_kernel<1>, dim3((unsigned)windows), dim3(WSE_THREADS), 0, s, a, b, idx,
                       n_idx_rows, rows, width, out, bad_count);
  return aw::check_launch("aw_window_sqerr");
}
