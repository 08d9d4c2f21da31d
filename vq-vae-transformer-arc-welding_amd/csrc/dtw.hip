// Brute-force exact k-nearest-neighbour search under banded dynamic time warping (aw_dtw_knn, include/arcweld_amd.h):
// the raw-cycle baseline of the latent-space probe (arcweld/retrieve.py dtw_search).  f32 throughout; a min-plus
// dynamic program on the VALU and the LDS, no MFMA.
//
//   dtw_sweep_kernel   grid (query tiles, database splits), ONE wave per workgroup.  A workgroup owns DQ = 4 queries
//                      and sweeps its split's database tiles of DX = 64 rows: lane l evaluates the pair (query, row
//                      l of the tile), one query after the other.  The dynamic program runs row by row over the
//                      database samples a = 0 .. len - 1 (whose c channels the lane holds in registers, the next
//                      sample's loads in flight under the current row) and inside a row over the band's query samples
//                      b = a - r .. a + r, band position p = b - a + r.  The lane keeps ONE line of the band in LDS
//                      ([position][lane]: a wave's accesses fall on consecutive banks): before cell p is written
//                      line[p] is D(a-1, b-1) and line[p+1] is D(a-1, b), and D(a, b-1) is carried in a register, so a
//                      cell costs one ds_read_b32 and one ds_write_b32 of the line.  Position 2r + 1 stays +inf (the
//                      absent cell above the band's upper edge) and position r starts as 0, which makes the origin
//                      cost(0, 0) + 0.  The query samples the band needs sit in a ring of DRING = 512 samples in LDS,
//                      refilled DCHUNK = 64 samples at a time, and are read as broadcasts (one address per wave).
//                      All D values are >= +0, +inf or NaN, for which the order of the f32 values is the order of
//                      their bit patterns as unsigned integers (a NaN above +inf): the minimum is one v_min3_u32,
//                      exact, without the canonicalisation an f32 minimum drags in.
//                      After a pair the lanes whose distance beats the query's current k-th one (a ballot) are taken
//                      in ascending lane = ascending database index and inserted into the query's sorted list in LDS
//                      with a strict <: the lexicographic (d, j) order inside a split, as in knn.hip.
//   knn_merge_kernel   knn_merge.h, shared with knn.hip: the (d, j) selection over the splits' partial lists.
//
//                      The inner loop runs in groups of DU = 4 cells and issues the next group's LDS reads before the
//                      current group's dependent min / add chain (every read of a row lies above the row's writes).
//
// LDS: the line is dynamic, (2r + 2 + DU) * 64 words; the ring and the lists are static.  At the widest band
// (AW_DTW_MAX_WINDOW = 449) and 8 channels that is 116,224 + 16,384 + 1,024 B.  The ring bounds the window: refilling
// samples [f, f + 64) when the band first needs sample f = a + r overwrites samples up to f + 63 - 512, which must lie
// below the band's lower edge a - r = f - 2r: 2r + 1 + 63 <= 512.
//
// Every cell is one fixed expression (the header's) of the two samples and its three predecessors, and min is exact:
// the bits of a distance depend on neither the traversal, the grid, nor the run.  No float atomics anywhere.
#include "common.h"
#include "knn_merge.h"

#include <math.h>

namespace {

constexpr int DQ = 4;         // queries per workgroup, one after the other
constexpr int DX = 64;        // database rows per tile: one per lane
constexpr int DRING = 512;    // query samples in the LDS ring (a power of two)
constexpr int DCHUNK = 64;    // samples per refill: one per lane
constexpr int DU = 4;         // band cells per group of the inner loop; the line has DU spare positions
constexpr uint32_t DINF = 0x7F800000u;
static_assert(AW_DTW_MAX_WINDOW + DCHUNK - 1 <= DRING, "the ring must hold the band and the chunk being refilled");
static_assert((AW_DTW_MAX_WINDOW + 1 + DU) * DX * 4 + DRING * AW_DTW_MAX_C * 4 + DQ * AW_KNN_MAX_K * 8 <= 160 * 1024,
              "dtw LDS");

// dtw(query row qr, this lane's database row xr) as f32 bits.  line: (2r + 2 + DU) * DX words, ring: DRING * C floats.
template <int C>
__device__ __forceinline__ uint32_t dtw_pair(const float* __restrict__ qr, const float* __restrict__ xr, int L, int r,
                                             uint32_t* __restrict__ line, float* __restrict__ ring, int lane) {
  const int W = 2 * r + 1;
  for (int p = 0; p <= W; ++p) line[p * DX + lane] = DINF;
  line[r * DX + lane] = 0u;   // the origin's "predecessor": D(0, 0) = cost(0, 0) + 0
  __syncthreads();            // the previous pair is done with the ring
  int frontier = 0;           // query samples [0, frontier) have been staged
  float xc[C], xn[C];
#pragma unroll
  for (int ch = 0; ch < C; ++ch) xn[ch] = xr[ch];
  for (int a = 0; a < L; ++a) {
#pragma unroll
    for (int ch = 0; ch < C; ++ch) xc[ch] = xn[ch];
    if (a + 1 < L) {
#pragma unroll
      for (int ch = 0; ch < C; ++ch) xn[ch] = xr[(a + 1) * C + ch];
    }
    const int need = a + r < L - 1 ? a + r : L - 1;   // the band's last query sample
    while (frontier <= need) {                         // wave-uniform; several chunks only at a = 0
      __syncthreads();
      const int s = frontier + lane;
      if (s < L) {
#pragma unroll
        for (int ch = 0; ch < C; ++ch) ring[(s & (DRING - 1)) * C + ch] = qr[s * C + ch];
      }
      frontier += DCHUNK;
      __syncthreads();
    }
    const int p_lo = r - a > 0 ? r - a : 0;
    const int p_hi = L - 1 - a + r < 2 * r ? L - 1 - a + r : 2 * r;
    uint32_t left = DINF;                              // D(a, b - 1)
    uint32_t diag = line[p_lo * DX + lane];            // D(a - 1, b - 1)
    int p = p_lo, b = a - r + p_lo;
    // one cell: `up` is D(a - 1, b), qs the query sample b
    auto cell = [&](uint32_t up, const float* qs, int pp) {
      float acc = 0.f;
#pragma unroll
      for (int ch = 0; ch < C; ++ch) {
        const float d = __fsub_rn(qs[ch], xc[ch]);
        acc = __builtin_fmaf(d, d, acc);
      }
      uint32_t m = diag < up ? diag : up;
      m = m < left ? m : left;
      left = __float_as_uint(__fadd_rn(acc, __uint_as_float(m)));
      line[pp * DX + lane] = left;
      diag = up;
    };
    // Groups of DU cells, the next group's LDS reads issued before the current group's dependent chain: every read
    // of a row is of a position above everything the row has written so far, so reading ahead is reading the old
    // line.  A read-ahead past p_hi stays inside the line's DU spare positions and is never used.
    struct Group {
      uint32_t up[DU];
      float q[DU][C];
    };
    auto fetch = [&](Group& g, int pp, int bb) {
#pragma unroll
      for (int u = 0; u < DU; ++u) {
        g.up[u] = line[(pp + 1 + u) * DX + lane];
#pragma unroll
        for (int ch = 0; ch < C; ++ch) g.q[u][ch] = ring[((bb + u) & (DRING - 1)) * C + ch];
      }
    };
    auto run = [&](const Group& g, int pp) {
#pragma unroll
      for (int u = 0; u < DU; ++u) cell(g.up[u], g.q[u], pp + u);
    };
    int groups = (p_hi - p_lo + 1) / DU;
    if (groups > 0) {
      Group g0, g1;
      fetch(g0, p, b);
      for (; groups >= 2; groups -= 2, p += 2 * DU, b += 2 * DU) {
        fetch(g1, p + DU, b + DU);
        run(g0, p);
        fetch(g0, p + 2 * DU, b + 2 * DU);
        run(g1, p + DU);
      }
      if (groups) {
        run(g0, p);
        p += DU, b += DU;
      }
    }
    for (; p <= p_hi; ++p, ++b) cell(line[(p + 1) * DX + lane], ring + (b & (DRING - 1)) * C, p);
  }
  return line[r * DX + lane];   // D(len - 1, len - 1), this lane's own last write to the position
}

template <int C>
__global__ __launch_bounds__(DX) void dtw_sweep_kernel(const float* __restrict__ q, int64_t nq, int64_t ldq,
                                                       const float* __restrict__ x, int64_t nx, int64_t ldx, int L,
                                                       int r, int k, const int* __restrict__ qg,
                                                       const int* __restrict__ xg, int64_t tiles_per_split,
                                                       float* __restrict__ ws_d, int* __restrict__ ws_i) {
  extern __shared__ uint32_t dtw_line[];            // (2r + 2 + DU) * DX: [band position][lane]
  __shared__ float ring[DRING * C];                 // [sample & (DRING - 1)][channel]
  __shared__ float lst_d[DQ * AW_KNN_MAX_K];        // [query][slot], ascending (d, j)
  __shared__ int lst_i[DQ * AW_KNN_MAX_K];
  const int lane = threadIdx.x;
  const int64_t q0 = (int64_t)blockIdx.x * DQ;
  const int nqt = nq - q0 < DQ ? (int)(nq - q0) : DQ;
  const int64_t xtiles = (nx + DX - 1) / DX;
  const int64_t t0 = (int64_t)blockIdx.y * tiles_per_split;
  const int64_t t1 = t0 + tiles_per_split < xtiles ? t0 + tiles_per_split : xtiles;
  const bool use_g = qg != nullptr && xg != nullptr;

  for (int s = lane; s < DQ * AW_KNN_MAX_K; s += DX) {
    lst_d[s] = __builtin_huge_valf();
    lst_i[s] = -1;
  }
  __syncthreads();

  for (int64_t tile = t0; tile < t1; ++tile) {
    const int64_t row = tile * DX + lane;
    const bool valid = row < nx;
    const int64_t rowc = valid ? row : nx - 1;      // a lane past the end reads the last row and is never taken
    const float* xr = x + rowc * ldx;
    const int myg = use_g ? xg[rowc] : 0;
    for (int qq = 0; qq < nqt; ++qq) {
      const float d = __uint_as_float(dtw_pair<C>(q + (q0 + qq) * ldq, xr, L, r, dtw_line, ring, lane));
      float* ld = lst_d + qq * AW_KNN_MAX_K;
      int* li = lst_i + qq * AW_KNN_MAX_K;
      // d < thr is false for a NaN and for +inf (thr <= +inf): only finite distances are ever taken
      bool ok = valid && d < ld[k - 1];
      if (use_g) ok = ok && qg[q0 + qq] != myg;
      unsigned long long cand = __ballot(ok);
      while (cand) {                                 // ascending lane = ascending database index
        const int j = __ffsll((long long)cand) - 1;
        cand &= cand - 1;
        const float dj = __shfl(d, j, 64);
        if (dj < ld[k - 1]) {                        // wave-uniform; an equal distance never displaces a lower j
          if (lane == 0) {
            int pos = k - 1;
            while (pos > 0 && ld[pos - 1] > dj) {
              ld[pos] = ld[pos - 1];
              li[pos] = li[pos - 1];
              --pos;
            }
            ld[pos] = dj;
            li[pos] = (int)(tile * DX + j);
          }
          __syncthreads();
        }
      }
    }
  }

  __syncthreads();
  for (int s = lane; s < nqt * k; s += DX) {
    const int qq = s / k, e = s - qq * k;
    const int64_t o = ((int64_t)blockIdx.y * nq + q0 + qq) * k + e;
    ws_d[o] = lst_d[qq * AW_KNN_MAX_K + e];
    ws_i[o] = lst_i[qq * AW_KNN_MAX_K + e];
  }
}

// The database is split so that a launch with few query tiles still fills the 256 CUs with several one-wave
// workgroups each.
int dtw_auto_splits(int64_t nq, int64_t nx) {
  const int64_t qtiles = (nq + DQ - 1) / DQ, xtiles = (nx + DX - 1) / DX;
  if (qtiles >= 2048 || xtiles <= 1) return 1;
  int64_t s = (2048 + qtiles - 1) / qtiles;
  if (s > xtiles) s = xtiles;
  if (s > AW_KNN_MAX_SPLITS) s = AW_KNN_MAX_SPLITS;
  return (int)(s < 1 ? 1 : s);
}

int dtw_check(const char* who, int64_t nq, int64_t nx, int len, int c, int radius, int k, int splits) {
  AW_REQUIRE(nq >= 0 && nq <= ((int64_t)1 << 40), "%s: nq = %lld outside 0..2^40", who, (long long)nq);
  AW_REQUIRE(nx >= 0 && nx < ((int64_t)1 << 31), "%s: nx = %lld outside 0..2^31 - 1", who, (long long)nx);
  AW_REQUIRE(len >= 1 && len <= AW_DTW_MAX_LEN, "%s: len = %d outside 1..%d", who, len, AW_DTW_MAX_LEN);
  AW_REQUIRE(c >= 1 && c <= AW_DTW_MAX_C, "%s: c = %d outside 1..%d", who, c, AW_DTW_MAX_C);
  AW_REQUIRE(radius >= 0 && radius <= len - 1, "%s: radius = %d outside 0..len - 1 = %d", who, radius, len - 1);
  AW_REQUIRE(2 * radius + 1 <= AW_DTW_MAX_WINDOW, "%s: radius = %d gives a band of %d samples, at most %d", who,
             radius, 2 * radius + 1, AW_DTW_MAX_WINDOW);
  AW_REQUIRE(k >= 1 && k <= AW_KNN_MAX_K, "%s: k = %d outside 1..%d", who, k, AW_KNN_MAX_K);
  AW_REQUIRE(splits >= 0 && splits <= AW_KNN_MAX_SPLITS, "%s: splits = %d outside 0..%d (0 = auto)", who, splits,
             AW_KNN_MAX_SPLITS);
  return AW_OK;
}

template <int C>
int dtw_launch(dim3 grid, size_t lds, hipStream_t s, const float* q, int64_t nq, int64_t ldq, const float* x,
               int64_t nx, int64_t ldx, int len, int radius, int k, const int* qg, const int* xg, int64_t tps,
               float* ws_d, int* ws_i) {
  if (lds > 48 * 1024) {   // a dynamic LDS size above the default limit has to be announced per kernel
    const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(&dtw_sweep_kernel<C>),
                                             hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    AW_REQUIRE(e == hipSuccess, "aw_dtw_knn: cannot reserve %lld bytes of LDS: %s", (long long)lds,
               hipGetErrorString(e));
  }
  hipLaunchKernelGGL((dtw_sweep_kernel<C>), grid, dim3(DX), lds, s, q, nq, ldq, x, nx, ldx, len, radius, k, qg, xg, tps,
                     ws_d, ws_i);
  return aw::check_launch("aw_dtw_knn (sweep)");
}

}  // namespace

extern "C" int64_t aw_dtw_knn_workspace(int64_t nq, int64_t nx, int len, int c, int radius, int k, int splits) {
  if (dtw_check("aw_dtw_knn_workspace", nq, nx, len, c, radius, k, splits) != AW_OK) return AW_ERR_ARG;
  const int64_t sp = splits > 0 ? splits : dtw_auto_splits(nq, nx);
  return sp * nq * k * (int64_t)(sizeof(float) + sizeof(int));
}

extern "C" int aw_dtw_knn_describe(int* tile_q, int* tile_x) {
  if (tile_q) *tile_q = DQ;
  if (tile_x) *tile_x = DX;
  return AW_OK;
}

extern "C" int aw_dtw_knn(const float* q, int64_t nq, int64_t ldq, const float* x, int64_t nx, int64_t ldx, int len,
                          int c, int radius, int k, const int* q_group, const int* x_group, int splits, void* ws,
                          int64_t ws_bytes, int64_t* idx, float* dist, void* stream) {
  const int st = dtw_check("aw_dtw_knn", nq, nx, len, c, radius, k, splits);
  if (st != AW_OK) return st;
  const int64_t d = (int64_t)len * c;
  AW_REQUIRE(ldq >= d && ldx >= d && ldq < (1 << 22) && ldx < (1 << 22),
             "aw_dtw_knn: row strides ldq = %lld, ldx = %lld must lie in len * c = %lld .. 2^22 - 1", (long long)ldq,
             (long long)ldx, (long long)d);
  if (nq == 0) return AW_OK;
  AW_REQUIRE(q && idx && dist, "aw_dtw_knn: q, idx and dist must not be NULL");
  AW_REQUIRE(x || nx == 0, "aw_dtw_knn: x is NULL with nx = %lld", (long long)nx);
  AW_REQUIRE(((uintptr_t)q & 3) == 0 && ((uintptr_t)x & 3) == 0, "aw_dtw_knn: q and x must be 4-byte aligned");
  const int sp = splits > 0 ? splits : dtw_auto_splits(nq, nx);
  const int64_t need = (int64_t)sp * nq * k * (int64_t)(sizeof(float) + sizeof(int));
  AW_REQUIRE(ws && ws_bytes >= need, "aw_dtw_knn: workspace of %lld bytes, need %lld (aw_dtw_knn_workspace)",
             (long long)ws_bytes, (long long)need);
  AW_REQUIRE(((uintptr_t)ws & 3) == 0, "aw_dtw_knn: the workspace must be 4-byte aligned");
  const int64_t qtiles = (nq + DQ - 1) / DQ, xtiles = (nx + DX - 1) / DX;
  AW_REQUIRE(qtiles <= 0x7FFFFFFFll, "aw_dtw_knn: nq = %lld needs too many query tiles", (long long)nq);
  const int64_t mblocks = knn_merge_blocks(nq);
  AW_REQUIRE(mblocks <= 0x7FFFFFFFll, "aw_dtw_knn: nq = %lld needs too many merge blocks", (long long)nq);
  const int64_t tps = xtiles > 0 ? (xtiles + sp - 1) / sp : 1;
  float* ws_d = static_cast<float*>(ws);
  int* ws_i = reinterpret_cast<int*>(ws_d + (int64_t)sp * nq * k);
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  const dim3 grid((unsigned)qtiles, (unsigned)sp);
  const size_t lds = (size_t)(2 * radius + 2 + DU) * DX * sizeof(uint32_t);
  int st2 = AW_ERR_ARG;
#define DTW_SWEEP(CH)                                                                                              \
  case CH:                                                                                                         \
    st2 = dtw_launch<CH>(grid, lds, s, q, nq, ldq, x, nx, ldx, len, radius, k, q_group, x_group, tps, ws_d, ws_i); \
    break
  switch (c) {
    DTW_SWEEP(1);
    DTW_SWEEP(2);
    DTW_SWEEP(3);
    DTW_SWEEP(4);
    DTW_SWEEP(5);
    DTW_SWEEP(6);
    DTW_SWEEP(7);
    DTW_SWEEP(8);
  }
#undef DTW_SWEEP
  if (st2 != AW_OK) return st2;
  hipLaunchKernelGGL(knn_merge_kernel, dim3((unsigned)mblocks), dim3(KNN_MERGE_THREADS), 0, s, ws_d, ws_i, nq, k, sp,
                     idx, dist);
  return aw::check_launch("aw_dtw_knn (merge)");
}
