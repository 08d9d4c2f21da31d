// Brute-force exact k-nearest-neighbour search in squared Euclidean distance (aw_knn, include/arcweld_amd.h): the
// latent-space probe's hot path (arcweld/retrieve.py).  f32 throughout; the (nq x nx) distance matrix never reaches
// memory.
//
//   knn_sweep_kernel   grid (query tiles, database splits).  A 256-thread workgroup owns KQ = 128 queries and sweeps
//                      its split's database tiles of KX = 128 rows.  Per tile the distances come from the shared
//                      all-pairs tile (pair_tile.h: staging through LDS, dots on the f32-input MFMA, norms beside
//                      them) with the queries as its b rows and the database as its a rows (the MFMA's A operand); the
//                      first chunk of the next tile is fetched under the last chunk's MFMAs.  With k <= 6 two
//                      workgroups share a CU and cover each other's stores and barriers.  Wave w owns the 64 x 64
//                      block (database half w >> 1) x (query half w & 1) as 2 x 2 tiles of 32 x 32, so a lane ends with
//                      ONE query per tile column and 16 database rows in its accumulator registers.
//                      At the end of a tile the distances d = fma(-2, dot, fl(|q|^2 + |x|^2)) go to LDS as [x][q]
//                      (over the now idle stages) and thread i < 128 scans query i's 128 candidates in ascending j
//                      against its current k-th distance (a register); the rare winner is inserted into the query's
//                      sorted list in LDS ([slot][query]: conflict-free).  Ascending j with a strict < is the
//                      lexicographic (d, j) order inside a split.
//   knn_merge_kernel   (knn_merge.h, shared with dtw.hip) one wave per query: k selection passes over the splits'
//                      partial lists (splits * k candidates) on 64-bit keys (order-preserving distance bits above j):
//                      the same (d, j) order, so the result does not depend on the split count.  It also clamps the
//                      stored distance at 0 and widens idx.
//
// One (i, j) distance is always accumulated over all of D by one wave in one fixed order (pair_tile.h): its bits
// depend on neither the grid nor the run.  No float atomics anywhere.
#include "common.h"
#include "knn_merge.h"
#include "pair_tile.h"

#include <math.h>

namespace {

namespace pt = aw::pt;
constexpr int KQ = pt::TB;          // queries per workgroup
constexpr int KX = pt::TA;          // database rows per tile
constexpr int KD = pt::TD;          // dims per chunk
constexpr int KTHREADS = pt::THREADS;
constexpr int KDT = pt::OT;         // distance tile row stride
constexpr int KNN_KCAP_SMALL = 6;   // list capacity up to which two workgroups fit a CU's 160 KiB of LDS
static_assert((2 * pt::STAGE + 2 * AW_KNN_MAX_K * KQ + KQ + KX) * 4 <= 160 * 1024, "knn LDS");
static_assert((2 * pt::STAGE + 2 * KNN_KCAP_SMALL * KQ + KQ + KX) * 4 <= 80 * 1024, "knn LDS, two workgroups per CU");

// KCAP: the capacity of the per-query lists.  k <= KNN_KCAP_SMALL leaves the workgroup under half of a CU's LDS, so
// two workgroups share a CU (two waves per SIMD): one's MFMAs cover the other's LDS stores and barriers.
template <bool QVEC, bool XVEC, int KCAP>
__global__ __launch_bounds__(KTHREADS, KCAP <= KNN_KCAP_SMALL ? 2 : 1) void knn_sweep_kernel(
    const float* __restrict__ q, int64_t nq, int64_t ldq, const float* __restrict__ x, int64_t nx, int64_t ldx, int D,
    int k, const int* __restrict__ qg, const int* __restrict__ xg, int64_t tiles_per_split, float* __restrict__ ws_d,
    int* __restrict__ ws_i) {
  __shared__ __attribute__((aligned(16))) float stage[2 * pt::STAGE];
  __shared__ float lst_d[KCAP * KQ];   // [slot][query], ascending (d, j)
  __shared__ int lst_i[KCAP * KQ];
  __shared__ float nrm_s[KQ + KX];             // |q|^2 of the tile's queries, then |x|^2 of the tile's rows
  const int tid = threadIdx.x;
  const int64_t q0 = (int64_t)blockIdx.x * KQ;
  const int64_t xtiles = (nx + KX - 1) / KX;
  const int64_t t0 = (int64_t)blockIdx.y * tiles_per_split;
  const int64_t t1 = t0 + tiles_per_split < xtiles ? t0 + tiles_per_split : xtiles;
  const int nch = (D + KD - 1) / KD;
  const bool use_g = qg != nullptr && xg != nullptr;

  if (tid < KQ)
    for (int s = 0; s < k; ++s) {
      lst_d[s * KQ + tid] = __builtin_huge_valf();
      lst_i[s * KQ + tid] = -1;
    }
  float thr = __builtin_huge_valf();   // this thread's query's current k-th distance
  const int myg = (use_g && tid < KQ && q0 + tid < nq) ? qg[q0 + tid] : 0;

  float4 pre[pt::F4];
  const pt::Operand qo = pt::operand(q, q0, nq, ldq, D, KQ);
  auto fetch = [&](int64_t tile, int ch) {
    pt::fetch<QVEC, XVEC>(pre, qo, pt::operand(x, tile * KX, nx, ldx, D, KX), ch, D, tid);
  };
  if (t0 < t1) fetch(t0, 0);
  int buf = 0;
  for (int64_t tile = t0; tile < t1; ++tile) {
    pt::f32x16 acc[2][2];   // [database tile mi][query tile ni]
    pt::zero(acc);
    float nrm = 0.f;        // the squared norm of staged row `tid`, an in-order fmaf chain over D
    for (int ch = 0; ch < nch; ++ch) {
      float* sb = stage + buf * pt::STAGE;
      pt::stage_put(sb, pre, tid);
      __syncthreads();
      // the next chunk's loads fly under this chunk's MFMAs (the stage written next was last read before this barrier)
      if (ch + 1 < nch)
        fetch(tile, ch + 1);
      else if (tile + 1 < t1)
        fetch(tile + 1, 0);
      pt::dots(sb, tid, acc, nrm);
      buf ^= 1;
    }

    // ---- the tile's distances to LDS as [database row][query]
    float* dt = stage;
    pt::dist_tile(dt, nrm_s, nrm, tid, acc, [](float d) { return d; });

    // ---- thread i scans query i's candidates in ascending j.  d < thr is false for a NaN and for +inf (thr <= +inf),
    //      so only finite distances are ever taken; an equal distance never displaces an earlier (lower) j.
    if (tid < KQ) {
      const int64_t x0 = tile * KX;
      const int cnt = nx - x0 < KX ? (int)(nx - x0) : KX;
      for (int jj = 0; jj < cnt; ++jj) {
        const float d = dt[jj * KDT + tid];
        bool ok = d < thr;
        if (use_g) ok = ok && xg[x0 + jj] != myg;
        if (ok) {
          int pos = k - 1;
          while (pos > 0 && lst_d[(pos - 1) * KQ + tid] > d) {
            lst_d[pos * KQ + tid] = lst_d[(pos - 1) * KQ + tid];
            lst_i[pos * KQ + tid] = lst_i[(pos - 1) * KQ + tid];
            --pos;
          }
          lst_d[pos * KQ + tid] = d;
          lst_i[pos * KQ + tid] = (int)(x0 + jj);
          thr = lst_d[(k - 1) * KQ + tid];
        }
      }
    }
    __syncthreads();   // the scan is done with the distance tile before the next chunk is staged over it
  }

  if (tid < KQ && q0 + tid < nq) {
    const int64_t o = ((int64_t)blockIdx.y * nq + q0 + tid) * k;
    for (int s = 0; s < k; ++s) {
      ws_d[o + s] = lst_d[s * KQ + tid];
      ws_i[o + s] = lst_i[s * KQ + tid];
    }
  }
}

// The database is split so that a launch with few query tiles still fills the 256 CUs (about two workgroups each).
int knn_auto_splits(int64_t nq, int64_t nx) {
  const int64_t qtiles = (nq + KQ - 1) / KQ, xtiles = (nx + KX - 1) / KX;
  if (qtiles >= 256 || xtiles <= 1) return 1;
  int64_t s = (512 + qtiles - 1) / qtiles;
  if (s > xtiles) s = xtiles;
  if (s > AW_KNN_MAX_SPLITS) s = AW_KNN_MAX_SPLITS;
  return (int)(s < 1 ? 1 : s);
}

int knn_check(const char* who, int64_t nq, int64_t nx, int d, int k, int splits) {
  AW_REQUIRE(nq >= 0 && nq <= ((int64_t)1 << 40), "%s: nq = %lld outside 0..2^40", who, (long long)nq);
  AW_REQUIRE(nx >= 0 && nx < ((int64_t)1 << 31), "%s: nx = %lld outside 0..2^31 - 1", who, (long long)nx);
  AW_REQUIRE(d >= 1, "%s: d = %d, need d >= 1", who, d);
  AW_REQUIRE(k >= 1 && k <= AW_KNN_MAX_K, "%s: k = %d outside 1..%d", who, k, AW_KNN_MAX_K);
  AW_REQUIRE(splits >= 0 && splits <= AW_KNN_MAX_SPLITS, "%s: splits = %d outside 0..%d (0 = auto)", who, splits,
             AW_KNN_MAX_SPLITS);
  return AW_OK;
}

}  // namespace

extern "C" int64_t aw_knn_workspace(int64_t nq, int64_t nx, int d, int k, int splits) {
  if (knn_check("aw_knn_workspace", nq, nx, d, k, splits) != AW_OK) return AW_ERR_ARG;
  const int64_t sp = splits > 0 ? splits : knn_auto_splits(nq, nx);
  return sp * nq * k * (int64_t)(sizeof(float) + sizeof(int));
}

extern "C" int aw_knn_describe(int* tile_q, int* tile_x, int* chunk_d, int* max_k) {
  if (tile_q) *tile_q = KQ;
  if (tile_x) *tile_x = KX;
  if (chunk_d) *chunk_d = KD;
  if (max_k) *max_k = AW_KNN_MAX_K;
  return AW_OK;
}

extern "C" int aw_knn(const float* q, int64_t nq, int64_t ldq, const float* x, int64_t nx, int64_t ldx, int d, int k,
                      const int* q_group, const int* x_group, int splits, void* ws, int64_t ws_bytes, int64_t* idx,
                      float* dist, void* stream) {
  const int st = knn_check("aw_knn", nq, nx, d, k, splits);
  if (st != AW_OK) return st;
  AW_REQUIRE(ldq >= d && ldx >= d && ldq < (1 << 22) && ldx < (1 << 22),
             "aw_knn: row strides ldq = %lld, ldx = %lld must lie in d = %d .. 2^22 - 1", (long long)ldq,
             (long long)ldx, d);
  if (nq == 0) return AW_OK;
  AW_REQUIRE(q && idx && dist, "aw_knn: q, idx and dist must not be NULL");
  AW_REQUIRE(x || nx == 0, "aw_knn: x is NULL with nx = %lld", (long long)nx);
  AW_REQUIRE(((uintptr_t)q & 3) == 0 && ((uintptr_t)x & 3) == 0, "aw_knn: q and x must be 4-byte aligned");
  const int sp = splits > 0 ? splits : knn_auto_splits(nq, nx);
  const int64_t need = (int64_t)sp * nq * k * (int64_t)(sizeof(float) + sizeof(int));
  AW_REQUIRE(ws && ws_bytes >= need, "aw_knn: workspace of %lld bytes, need %lld (aw_knn_workspace)",
             (long long)ws_bytes, (long long)need);
  AW_REQUIRE(((uintptr_t)ws & 3) == 0, "aw_knn: the workspace must be 4-byte aligned");
  const int64_t qtiles = (nq + KQ - 1) / KQ, xtiles = (nx + KX - 1) / KX;
  AW_REQUIRE(qtiles <= 0x7FFFFFFFll, "aw_knn: nq = %lld needs too many query tiles", (long long)nq);
  const int64_t tps = xtiles > 0 ? (xtiles + sp - 1) / sp : 1;
  float* ws_d = static_cast<float*>(ws);
  int* ws_i = reinterpret_cast<int*>(ws_d + (int64_t)sp * nq * k);
  const bool qvec = ((uintptr_t)q & 15) == 0 && (ldq & 3) == 0;   // 16-B loads: aligned base and stride
  const bool xvec = ((uintptr_t)x & 15) == 0 && (ldx & 3) == 0;
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  const dim3 grid((unsigned)qtiles, (unsigned)sp), block(KTHREADS);
#define KNN_SWEEP(QV, XV)                                                                                         \
  do {                                                                                                            \
    if (k <= KNN_KCAP_SMALL)                                                                                      \
      hipLaunchKernelGGL((knn_sweep_kernel<QV, XV, KNN_KCAP_SMALL>), grid, block, 0, s, q, nq, ldq, x, nx, ldx, d, \
                         k, q_group, x_group, tps, ws_d, ws_i);                                                   \
    else                                                                                                          \
      hipLaunchKernelGGL((knn_sweep_kernel<QV, XV, AW_KNN_MAX_K>), grid, block, 0, s, q, nq, ldq, x, nx, ldx, d,   \
                         k, q_group, x_group, tps, ws_d, ws_i);                                                   \
  } while (0)
  if (qvec && xvec)
    KNN_SWEEP(true, true);
  else if (qvec)
    KNN_SWEEP(true, false);
  else if (xvec)
    KNN_SWEEP(false, true);
  else
    KNN_SWEEP(false, false);
#undef KNN_SWEEP
  const int st2 = aw::check_launch("aw_knn (sweep)");
  if (st2 != AW_OK) return st2;
  const int64_t mblocks = knn_merge_blocks(nq);
  AW_REQUIRE(mblocks <= 0x7FFFFFFFll, "aw_knn: nq = %lld needs too many merge blocks", (long long)nq);
  hipLaunchKernelGGL(knn_merge_kernel, dim3((unsigned)mblocks), dim3(KNN_MERGE_THREADS), 0, s, ws_d, ws_i, nq, k, sp,
                     idx, dist);
  return aw::check_launch("aw_knn (merge)");
}
