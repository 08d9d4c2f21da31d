// Ensemble forecasts (arcweld.generate.forecast_cycles): N sampled continuations of one prompt reduced on the device
// to pointwise bands and, against the cycles that were really measured, to a score per cycle.
//
// aw_ensemble_stats: per point (g, m) of x (G, N, M) the mean, the unbiased standard deviation and Q linear quantiles
// over the N samples; with a truth y (G, M) also the ensemble CRPS of every point, averaged per segment of `seg` points
// (one cycle), and the share of the segment's points whose truth lies between the outermost quantiles.
//
// One 256-thread workgroup per (group, segment); thread t owns the points t, t + 256, ... of the segment.  M is the
// contiguous axis, so sample i of 64 neighbouring points is one coalesced 256-byte read.  The N samples of a thread's
// point sit in the thread's own LDS column, sample i at float index i * 256 + t: a wave's 64 lanes touch 64 consecutive
// dwords on every access (no bank conflict whatever N), and N * 1 KiB <= 64 KiB bounds N at 64.  The column is filled in
// index order (the f64 sum and the f64 sum of |x - y| are taken on the way), read once more for the squared deviations,
// then insertion-sorted in place: order statistics, interpolated quantiles and the CRPS' pair term
//   sum_{i<j} (x_(j) - x_(i)) = sum_i (2 i - N - 1) x_(i)
// all come from the sorted column.  A thread adds its points' CRPS in index order into an f64 partial; the partials go
// through a fixed xor tree per wave and the four wave sums are added in wave order by thread 0 (through the first bytes
// of the column area, free by then): no floating-point atomic, the same bits on every launch.
#include "common.h"

#define ENS_THREADS 256

struct ens_quantiles {
  float q[AW_ENSEMBLE_MAX_Q];
};

__device__ __forceinline__ float ens_nan() { return __uint_as_float(0x7FC00000u); }
__device__ __forceinline__ int ens_wave_sum_i(int v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

__global__ __launch_bounds__(ENS_THREADS) void ensemble_stats_kernel(
    const float* __restrict__ x, int N, int64_t M, ens_quantiles qs, int Q, float* __restrict__ mean,
    float* __restrict__ sdev, float* __restrict__ quant, const float* __restrict__ y, int64_t seg, int64_t n_seg,
    float* __restrict__ crps, float* __restrict__ cover, int* __restrict__ bad) {
  extern __shared__ __align__(16) float ens_col[];   // N rows of ENS_THREADS floats
  const int tid = threadIdx.x;
  const int64_t g = (int64_t)blockIdx.x / n_seg, s = (int64_t)blockIdx.x - g * n_seg;
  const float* xg = x + g * N * M;
  float* col = ens_col + tid;
  const double n_d = (double)N;
  double acc = 0.0;   // this thread's points' CRPS, in index order
  int hit = 0, nb = 0;
  for (int64_t p = tid; p < seg; p += ENS_THREADS) {
    const int64_t m = s * seg + p;
    const float yv = y ? y[g * M + m] : 0.f;
    bool ok = fabsf(yv) < INFINITY;
    double sum = 0.0, sab = 0.0;
#pragma unroll 4
    for (int i = 0; i < N; ++i) {
      const float v = xg[(int64_t)i * M + m];
      col[i * ENS_THREADS] = v;
      ok &= fabsf(v) < INFINITY;
      sum += (double)v;
      sab += fabs((double)v - (double)yv);
    }
    if (!ok) {
      if (mean) mean[g * M + m] = ens_nan();
      if (sdev) sdev[g * M + m] = ens_nan();
      for (int k = 0; k < Q; ++k) quant[(g * Q + k) * M + m] = ens_nan();
      ++nb;
      continue;
    }
    const double mu = sum / n_d;
    if (mean) mean[g * M + m] = (float)mu;
    if (sdev) {
      double ss = 0.0;
      for (int i = 0; i < N; ++i) {
        const double d = (double)col[i * ENS_THREADS] - mu;
        ss += d * d;
      }
      sdev[g * M + m] = N > 1 ? (float)sqrt(ss / (double)(N - 1)) : 0.f;
    }
    if (Q == 0 && !crps) continue;
    for (int i = 1; i < N; ++i) {   // insertion sort of the column, ascending; values move, no bit changes
      const float v = col[i * ENS_THREADS];
      int j = i - 1;
      while (j >= 0) {
        const float w = col[j * ENS_THREADS];
        if (!(w > v)) break;
        col[(j + 1) * ENS_THREADS] = w;
        --j;
      }
      col[(j + 1) * ENS_THREADS] = v;
    }
    float q_lo = 0.f, q_hi = 0.f;
#pragma unroll
    for (int k = 0; k < AW_ENSEMBLE_MAX_Q; ++k) {
      if (k < Q) {
        const double h = (double)(N - 1) * (double)qs.q[k];
        const int lo = (int)floor(h), hi = lo + 1 < N ? lo + 1 : N - 1;
        const float fr = (float)(h - (double)lo);
        const float a = col[lo * ENS_THREADS], b = col[hi * ENS_THREADS];
        const float v = fr == 0.f ? a : fmaf(fr, b - a, a);   // an integral h: the order statistic itself
        quant[(g * Q + k) * M + m] = v;
        if (k == 0) q_lo = v;
        if (k == Q - 1) q_hi = v;
      }
    }
    if (cover) hit += (q_lo <= yv && yv <= q_hi) ? 1 : 0;
    if (crps) {
      double pair = 0.0;
      for (int i = 0; i < N; ++i) pair += (double)(2 * i + 1 - N) * (double)col[i * ENS_THREADS];
      acc += sab / n_d - pair / (n_d * n_d);
    }
  }
  // segment sums: a fixed tree per wave, the waves in order; the column area is free once every thread is here
  acc = wave_sum_d(acc);
  hit = ens_wave_sum_i(hit);
  nb = ens_wave_sum_i(nb);
  __syncthreads();
  double* part = reinterpret_cast<double*>(ens_col);       // 4 doubles, then 2 x 4 ints: 64 of the >= 1024 bytes
  int* ipart = reinterpret_cast<int*>(ens_col) + 8;
  const int lane = tid & 63, wv = tid >> 6;
  if (lane == 0) {
    part[wv] = acc;
    ipart[wv] = hit;
    ipart[4 + wv] = nb;
  }
  __syncthreads();
  if (tid == 0) {
    const double tot = (part[0] + part[1]) + (part[2] + part[3]);
    const int hits = (ipart[0] + ipart[1]) + (ipart[2] + ipart[3]);
    const int k = (ipart[4] + ipart[5]) + (ipart[6] + ipart[7]);
    if (crps) crps[blockIdx.x] = k ? ens_nan() : (float)(tot / (double)seg);
    if (cover) cover[blockIdx.x] = k ? ens_nan() : (float)((double)hits / (double)seg);
    if (k) atomicAdd(bad, k);
  }
}

extern "C" int aw_ensemble_stats(const aw_ensemble_args* a, void* stream) {
  AW_REQUIRE(a && a->bad_count && a->G >= 0 && a->M >= 0, "aw_ensemble_stats: bad args");
  AW_REQUIRE(a->N >= 1 && a->N <= AW_ENSEMBLE_MAX_N, "aw_ensemble_stats: N = %d outside 1..%d", a->N,
             AW_ENSEMBLE_MAX_N);
  AW_REQUIRE(a->Q >= 0 && a->Q <= AW_ENSEMBLE_MAX_Q, "aw_ensemble_stats: Q = %d outside 0..%d", a->Q,
             AW_ENSEMBLE_MAX_Q);
  AW_REQUIRE(a->Q == 0 || (a->q && a->quant), "aw_ensemble_stats: Q = %d needs q and quant", a->Q);
  ens_quantiles qs;
  memset(&qs, 0, sizeof(qs));
  for (int k = 0; k < a->Q; ++k) {
    AW_REQUIRE(a->q[k] >= 0.f && a->q[k] <= 1.f, "aw_ensemble_stats: q[%d] = %g outside [0, 1]", k, (double)a->q[k]);
    qs.q[k] = a->q[k];
  }
  AW_REQUIRE(a->seg >= 1, "aw_ensemble_stats: seg = %lld, need seg >= 1", (long long)a->seg);
  AW_REQUIRE(a->M % a->seg == 0, "aw_ensemble_stats: M = %lld is no multiple of seg = %lld", (long long)a->M,
             (long long)a->seg);
  AW_REQUIRE(a->y || (!a->crps && !a->cover), "aw_ensemble_stats: crps and cover need the truth y");
  AW_REQUIRE(!a->cover || a->Q >= 2, "aw_ensemble_stats: cover needs Q >= 2 (the outermost quantiles), got %d", a->Q);
  if (a->G == 0 || a->M == 0) return AW_OK;
  AW_REQUIRE(a->x, "aw_ensemble_stats: x is NULL");
  const int64_t n_seg = a->M / a->seg;
  AW_REQUIRE(n_seg <= 0x7FFFFFFFll / a->G, "aw_ensemble_stats: G * M / seg too large");
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  hipLaunchKernelGGL(ensemble_stats_kernel, dim3((unsigned)(a->G * n_seg)), dim3(ENS_THREADS),
                     (size_t)a->N * ENS_THREADS * sizeof(float), s, a->x, a->N, a->M, qs, a->Q, a->mean, a->std,
                     a->quant, a->y, a->seg, n_seg, a->crps, a->cover, a->bad_count);
  return aw::check_launch("aw_ensemble_stats");
}
