// Brute-force exact k-nearest-neighbour search in squared Euclidean distance (aw_knn, include/arcweld_amd.h): the
// latent-space probe's hot path (arcweld/retrieve.py).  f32 throughout; the (nq x nx) distance matrix never reaches
// memory.
//
//   knn_sweep_kernel   grid (query tiles, database splits).  A 256-thread workgroup owns KQ = 128 queries and sweeps
//                      its split's database tiles of KX = 128 rows.  Per tile it streams both operands through LDS in
//                      KD = 32-dim chunks (range-checked buffer loads -> registers -> LDS, the next chunk's loads in
//                      flight under the current chunk's MFMAs, two LDS stages, one barrier per chunk; with k <= 6 two
//                      workgroups share a CU and cover each other's stores and barriers) and runs the dot products on the
//                      f32-input MFMA (v_mfma_f32_32x32x2_f32: bit for bit an fmaf chain, cdna_hip_programming.md
//                      'FP32-input MFMA').  Wave w owns the 64 x 64 block (database half w >> 1) x (query half w & 1)
//                      as 2 x 2 tiles of 32 x 32; the database is the A operand, so a lane ends with ONE query per
//                      tile column and 16 database rows in its accumulator registers.  The squared norms accumulate
//                      beside the MFMAs as in-order fmaf chains, one staged row per thread.
//                      At the end of a tile the distances d = fma(-2, dot, fl(|q|^2 + |x|^2)) go to LDS as [x][q]
//                      (over the now idle stages) and thread i < 128 scans query i's 128 candidates in ascending j
//                      against its current k-th distance (a register); the rare winner is inserted into the query's
//                      sorted list in LDS ([slot][query]: conflict-free).  Ascending j with a strict < is the
//                      lexicographic (d, j) order inside a split.
//   knn_merge_kernel   one wave per query: k selection passes over the splits' partial lists (splits * k candidates)
//                      on 64-bit keys (order-preserving distance bits above j): the same (d, j) order, so the result
//                      does not depend on the split count.  It also clamps the stored distance at 0 and widens idx.
//
// One (i, j) distance is always accumulated over all of D by one wave in one fixed order (chunks ascending; in a
// chunk, MFMA step 4 g + t multiplies dims 8 g + t (lanes 0..31) and 8 g + 4 + t (lanes 32..63)): its bits depend on
// neither the grid nor the run.  No float atomics anywhere.
#include "common.h"

#include <math.h>

#include <type_traits>

namespace {

constexpr int KQ = 128;             // queries per workgroup
constexpr int KX = 128;             // database rows per tile
constexpr int KD = 32;              // dims per chunk
constexpr int KLD = KD + 4;         // staged row stride (floats): 16 rows of a ds_read_b128 cover all 64 banks
constexpr int KTHREADS = 256;
constexpr int KDT = KQ + 8;         // distance tile row stride: the two lane halves (4 rows apart) land 32 banks apart
constexpr int K_STAGE = (KQ + KX) * KLD;            // floats per stage: q rows 0..127, then x rows
constexpr int K_F4 = (KQ + KX) * (KD / 4) / KTHREADS;   // float4 per thread per chunk
static_assert(KX * KDT <= 2 * K_STAGE, "the distance tile overlays the two stages");
static_assert(KQ + KX == KTHREADS, "one staged row per thread for the norms");
constexpr int KNN_KCAP_SMALL = 6;   // list capacity up to which two workgroups fit a CU's 160 KiB of LDS
static_assert((2 * K_STAGE + 2 * AW_KNN_MAX_K * KQ + KQ + KX) * 4 <= 160 * 1024, "knn LDS");
static_assert((2 * K_STAGE + 2 * KNN_KCAP_SMALL * KQ + KQ + KX) * 4 <= 80 * 1024, "knn LDS, two workgroups per CU");

typedef __attribute__((ext_vector_type(16))) float f32x16;

// Operand loads go through raw buffer descriptors (one per tile of rows: base = the tile's first row, range = up to the
// last value of its last row): an offset past the range returns zeros, so a masked quad -- a row past the end, dims
// past D -- is a load at KNN_BAD_OFF instead of a branch or a select after the load.  The loads are straight-line code
// with nothing consuming them until the next chunk's LDS store, so they stay in flight under the MFMAs (with guarded
// global loads the compiler waited for each before the matrix work began: 45 TFLOP/s instead of the figures in
// DESIGN.md section 4.15).  Neither rows past the end nor the row padding are ever read.
constexpr uint32_t KNN_BAD_OFF = 0x80000000u;   // >= every range (a tile of rows spans < 2^31 bytes: ld < 2^22)
typedef unsigned int knn_u32x4 __attribute__((ext_vector_type(4)));

__device__ __forceinline__ __amdgpu_buffer_rsrc_t knn_rsrc(const float* base, int64_t row0, int64_t nrows, int64_t ld,
                                                           int D, int tile_rows, int& rows) {
  const int64_t left = nrows - row0;
  rows = (int)(left < tile_rows ? left : tile_rows);
  const uint32_t bytes = rows > 0 ? (uint32_t)(((int64_t)(rows - 1) * ld + D) * 4) : 0u;
  return __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(base + row0 * ld), (short)0, (int)bytes, 0x00020000);
}

// dims d0 .. d0 + 3 of tile row `row` (zeros for row >= rows and dims >= D).  VEC: base and stride are 16-byte
// aligned and the caller knows that no quad of this chunk straddles D, so a quad is one 16-B load; !VEC: four 4-byte
// loads, each masked on its own.
template <bool VEC>
__device__ __forceinline__ float4 knn_ld4(__amdgpu_buffer_rsrc_t r, int row, int rows, uint32_t ld_bytes, int d0,
                                          int D) {
  const bool rok = row < rows;
  const uint32_t off = (uint32_t)row * ld_bytes + 4u * (uint32_t)d0;
  if constexpr (VEC) {
    const knn_u32x4 u = __builtin_amdgcn_raw_buffer_load_b128(r, rok && d0 + 4 <= D ? off : KNN_BAD_OFF, 0, 0);
    return make_float4(__uint_as_float(u.x), __uint_as_float(u.y), __uint_as_float(u.z), __uint_as_float(u.w));
  } else {
    auto one = [&](int i) {
      return __uint_as_float(
          __builtin_amdgcn_raw_buffer_load_b32(r, rok && d0 + i < D ? off + 4u * i : KNN_BAD_OFF, 0, 0));
    };
    return make_float4(one(0), one(1), one(2), one(3));
  }
}

// KCAP: the capacity of the per-query lists.  k <= KNN_KCAP_SMALL leaves the workgroup under half of a CU's LDS, so
// two workgroups share a CU (two waves per SIMD): one's MFMAs cover the other's LDS stores and barriers.
template <bool QVEC, bool XVEC, int KCAP>
__global__ __launch_bounds__(KTHREADS, KCAP <= KNN_KCAP_SMALL ? 2 : 1) void knn_sweep_kernel(
    const float* __restrict__ q, int64_t nq, int64_t ldq, const float* __restrict__ x, int64_t nx, int64_t ldx, int D,
    int k, const int* __restrict__ qg, const int* __restrict__ xg, int64_t tiles_per_split, float* __restrict__ ws_d,
    int* __restrict__ ws_i) {
  __shared__ __attribute__((aligned(16))) float stage[2 * K_STAGE];
  __shared__ float lst_d[KCAP * KQ];   // [slot][query], ascending (d, j)
  __shared__ int lst_i[KCAP * KQ];
  __shared__ float nrm_s[KQ + KX];             // |q|^2 of the tile's queries, then |x|^2 of the tile's rows
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int h = lane >> 5, jr = lane & 31, wq = w & 1, wx = w >> 1;
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

  float4 pre[K_F4];
  // float4 i of thread tid is quad (tid & 7) of staged row (tid >> 3) + 32 i: queries for i < K_F4 / 2, database
  // rows after (known at compile time: no divergence between the two operands)
  int q_rows;
  const __amdgpu_buffer_rsrc_t q_rsrc = knn_rsrc(q, q0, nq, ldq, D, KQ, q_rows);
  const uint32_t ldq_b = (uint32_t)ldq * 4u, ldx_b = (uint32_t)ldx * 4u;
  auto fetch_as = [&](int64_t tile, int ch, auto qv, auto xv) {
    int x_rows;
    const __amdgpu_buffer_rsrc_t x_rsrc = knn_rsrc(x, tile * KX, nx, ldx, D, KX, x_rows);
    const int d0 = ch * KD + (tid & 7) * 4;
#pragma unroll
    for (int i = 0; i < K_F4; ++i) {
      const int row = (tid >> 3) + 32 * i;
      if (i < K_F4 / 2)
        pre[i] = knn_ld4<decltype(qv)::value>(q_rsrc, row, q_rows, ldq_b, d0, D);
      else
        pre[i] = knn_ld4<decltype(xv)::value>(x_rsrc, row - KQ, x_rows, ldx_b, d0, D);
    }
  };
  // only the last chunk of a D % 4 != 0 has a quad that straddles D: it alone takes the 4-byte loads (a uniform branch
  // between two straight-line blocks)
  auto fetch = [&](int64_t tile, int ch) {
    if ((D & 3) != 0 && ch == nch - 1)
      fetch_as(tile, ch, std::false_type{}, std::false_type{});
    else
      fetch_as(tile, ch, std::integral_constant<bool, QVEC>{}, std::integral_constant<bool, XVEC>{});
  };
  if (t0 < t1) fetch(t0, 0);
  int buf = 0;
  for (int64_t tile = t0; tile < t1; ++tile) {
    f32x16 acc[2][2];   // [database tile mi][query tile ni]
#pragma unroll
    for (int mi = 0; mi < 2; ++mi)
#pragma unroll
      for (int ni = 0; ni < 2; ++ni)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[mi][ni][r] = 0.f;
    float nrm = 0.f;    // the squared norm of staged row `tid`, an in-order fmaf chain over D
    for (int ch = 0; ch < nch; ++ch) {
      float* sb = stage + buf * K_STAGE;
#pragma unroll
      for (int i = 0; i < K_F4; ++i) {
        const int f = tid + i * KTHREADS;
        *reinterpret_cast<float4*>(sb + (f >> 3) * KLD + (f & 7) * 4) = pre[i];
      }
      __syncthreads();
      // the next chunk's loads fly under this chunk's MFMAs (the stage written next was last read before this barrier)
      if (ch + 1 < nch)
        fetch(tile, ch + 1);
      else if (tile + 1 < t1)
        fetch(tile + 1, 0);
#pragma unroll
      for (int c = 0; c < KD / 4; ++c) {
        const float4 v = *reinterpret_cast<const float4*>(sb + tid * KLD + 4 * c);
        nrm = __builtin_fmaf(v.x, v.x, nrm);
        nrm = __builtin_fmaf(v.y, v.y, nrm);
        nrm = __builtin_fmaf(v.z, v.z, nrm);
        nrm = __builtin_fmaf(v.w, v.w, nrm);
      }
      const float* sa = sb + (KQ + 64 * wx + jr) * KLD + 4 * h;   // A: database rows
      const float* sq = sb + (64 * wq + jr) * KLD + 4 * h;        // B: queries
#pragma unroll
      for (int g = 0; g < KD / 8; ++g) {
        float4 a4[2], b4[2];
#pragma unroll
        for (int t = 0; t < 2; ++t) {
          a4[t] = *reinterpret_cast<const float4*>(sa + 32 * t * KLD + 8 * g);
          b4[t] = *reinterpret_cast<const float4*>(sq + 32 * t * KLD + 8 * g);
        }
        const float av[2][4] = {{a4[0].x, a4[0].y, a4[0].z, a4[0].w}, {a4[1].x, a4[1].y, a4[1].z, a4[1].w}};
        const float bv[2][4] = {{b4[0].x, b4[0].y, b4[0].z, b4[0].w}, {b4[1].x, b4[1].y, b4[1].z, b4[1].w}};
#pragma unroll
        for (int s4 = 0; s4 < 4; ++s4)
#pragma unroll
          for (int mi = 0; mi < 2; ++mi)
#pragma unroll
            for (int ni = 0; ni < 2; ++ni)
              acc[mi][ni] = __builtin_amdgcn_mfma_f32_32x32x2f32(av[mi][s4], bv[ni][s4], acc[mi][ni], 0, 0, 0);
      }
      buf ^= 1;
    }

    // ---- the tile's distances to LDS: register r of acc[mi][ni] is database row 64 wx + 32 mi + 8 (r >> 2) + 4 h +
    //      (r & 3) against query 64 wq + 32 ni + jr.  2 dot is exact, so the fma's one rounding is that of
    //      fl(fl(|q|^2 + |x|^2) - 2 dot).
    nrm_s[tid] = nrm;
    __syncthreads();   // norms visible; every wave is done reading the stages
    float* dt = stage;
#pragma unroll
    for (int ni = 0; ni < 2; ++ni) {
      const int ql = 64 * wq + 32 * ni + jr;
      const float qq = nrm_s[ql];
#pragma unroll
      for (int mi = 0; mi < 2; ++mi)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const int xl = 64 * wx + 32 * mi + 8 * (r >> 2) + 4 * h + (r & 3);
          const float s = __fadd_rn(qq, nrm_s[KQ + xl]);
          dt[xl * KDT + ql] = __builtin_fmaf(-2.f, acc[mi][ni][r], s);
        }
    }
    __syncthreads();

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

// f32 bits -> u32 with the same order as the floats (negatives reversed below the positives)
__device__ __forceinline__ uint32_t knn_ord(float d) {
  const uint32_t u = __float_as_uint(d);
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float knn_unord(uint32_t o) {
  return __uint_as_float((o & 0x80000000u) ? (o & 0x7FFFFFFFu) : ~o);
}

__global__ __launch_bounds__(KTHREADS) void knn_merge_kernel(const float* __restrict__ ws_d,
                                                             const int* __restrict__ ws_i, int64_t nq, int k,
                                                             int splits, int64_t* __restrict__ idx,
                                                             float* __restrict__ dist) {
  const int lane = threadIdx.x & 63;
  const int64_t qi = (int64_t)blockIdx.x * (KTHREADS / 64) + (threadIdx.x >> 6);
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
  const int64_t mblocks = (nq + KTHREADS / 64 - 1) / (KTHREADS / 64);
  AW_REQUIRE(mblocks <= 0x7FFFFFFFll, "aw_knn: nq = %lld needs too many merge blocks", (long long)nq);
  hipLaunchKernelGGL(knn_merge_kernel, dim3((unsigned)mblocks), dim3(KTHREADS), 0, s, ws_d, ws_i, nq, k, sp, idx, dist);
  return aw::check_launch("aw_knn (merge)");
}
