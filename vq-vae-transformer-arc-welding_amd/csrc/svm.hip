// RBF support-vector probe (aw_rbf_gram, aw_svm_smo; include/arcweld_amd.h): the kernel matrix of two row sets and
// the C-SVC dual solver on a precomputed kernel matrix -- the hot path of arcweld.retrieve.svm_fit / svm_decision.
//
//   rbf_gram_kernel   grid (tiles of a, tiles of b); a 256-thread workgroup owns one GA x GB = 128 x 128 tile of k.
//                     The distances come from the all-pairs tile that knn_sweep_kernel uses (pair_tile.h: staging
//                     through LDS, dots on the f32-input MFMA with the rows of a as the A operand, norms beside them),
//                     two workgroups per CU.  The epilogue forms dist = fma(-2, dot, fl(|a|^2 + |b|^2)) -- the
//                     value aw_knn ranks by, from the same code -- and k = expf(fl(-gamma max(dist, 0))) into LDS as
//                     [a row][b row] (over the idle stages), then stores the tile row by row: a wave writes 64
//                     consecutive floats (or 16-byte quads when base and stride allow).
//                     One element is always accumulated over all of d by one wave in one fixed order, and every
//                     product and the sum of the norms commute (pair_tile.h): the bits of an element depend on
//                     neither the grid nor the run, and k(x, x) is bit-symmetric.  So when a and b are the same rows
//                     only the tiles on or above the diagonal are computed, and each writes its mirror image too.
//   svm_smo_kernel    one 1024-thread workgroup per problem, no synchronisation between workgroups.  Thread r owns
//                     rows r, r + 1024, ...: v_t = -y_t G_t (f64) and four bit masks (in I_up, in I_low, y > 0,
//                     y < 0) live in registers for the whole launch, the kernel diagonal and the current row i of k
//                     in LDS slots only their owner touches; alpha stays in global memory (an iteration touches two
//                     elements, written one barrier after every thread has read them).  An iteration is two block
//                     reductions -- a wave butterfly on (value, row), the winning lane posts what the block needs of
//                     its row, one barrier, a 16-lane butterfly over the waves' posts -- and two coalesced reads of a
//                     row of k through a range-checked buffer descriptor (rows past n read zeros).  Every comparison
//                     is a total order (value, then the lower row), so no result depends on the order of evaluation;
//                     all f64 arithmetic is uncontracted, libsvm's operations in libsvm's order.  RPT (rows per
//                     thread) only sizes the arrays: the thread that owns a row and every operation on it are the
//                     same in every instantiation.  128 VGPRs and no scratch at RPT = 20.
#include "common.h"
#include "pair_tile.h"

#include <math.h>

#pragma clang fp contract(off)

namespace {

// ------------------------------------------------------------------------------------------------ Gram matrix
namespace pt = aw::pt;
constexpr int GA = pt::TA;          // rows of a per workgroup (the MFMA's A operand)
constexpr int GB = pt::TB;          // rows of b per workgroup
constexpr int GD = pt::TD;          // dims per chunk
constexpr int GTHREADS = pt::THREADS;
constexpr int GKT = pt::OT;         // k tile row stride
static_assert(GA == GB, "the mirrored tile of a set against itself");
static_assert((2 * pt::STAGE + GA + GB) * 4 <= 80 * 1024, "gram LDS, two workgroups per CU");

template <bool AVEC, bool BVEC>
__global__ __launch_bounds__(GTHREADS, 2) void rbf_gram_kernel(const float* __restrict__ a, int64_t na, int64_t lda,
                                                               const float* __restrict__ b, int64_t nb, int64_t ldb,
                                                               int D, float gamma, float* __restrict__ k, int64_t ldk,
                                                               int kvec, int self) {
  // a set against itself: the tiles below the diagonal are the mirror images, bit for bit, of those above it (the sum
  // of the norms and every product commute), so the workgroup of tile (y, x) writes them and tile (x, y) has no work
  if (self && blockIdx.x > blockIdx.y) return;
  __shared__ __attribute__((aligned(16))) float stage[2 * pt::STAGE];
  __shared__ float nrm_s[GB + GA];             // |b|^2 of the tile's b rows, then |a|^2 of its a rows
  const int tid = threadIdx.x;
  const int64_t a0 = (int64_t)blockIdx.x * GA, b0 = (int64_t)blockIdx.y * GB;
  const int nch = (D + GD - 1) / GD;

  float4 pre[pt::F4];
  const pt::Operand ao = pt::operand(a, a0, na, lda, D, GA), bo = pt::operand(b, b0, nb, ldb, D, GB);
  pt::fetch<BVEC, AVEC>(pre, bo, ao, 0, D, tid);
  pt::f32x16 acc[2][2];   // [a tile mi][b tile ni]
  pt::zero(acc);
  float nrm = 0.f;        // the squared norm of staged row `tid`, an in-order fmaf chain over D
  int buf = 0;
  for (int ch = 0; ch < nch; ++ch) {
    float* sb = stage + buf * pt::STAGE;
    pt::stage_put(sb, pre, tid);
    __syncthreads();
    // the next chunk's loads fly under this chunk's MFMAs (the stage written next was last read before this barrier)
    if (ch + 1 < nch) pt::fetch<BVEC, AVEC>(pre, bo, ao, ch + 1, D, tid);
    pt::dots(sb, tid, acc, nrm);
    buf ^= 1;
  }

  // ---- the tile to LDS as [a row][b row]: k = expf(fl(-gamma max(dist, 0))) of the distance aw_knn ranks by
  float* kt = stage;
  const float ng = -gamma;
  pt::dist_tile(kt, nrm_s, nrm, tid, acc, [ng](float dist) {
    return expf(__fmul_rn(ng, dist < 0.f ? 0.f : dist));   // a NaN distance stays a NaN
  });

  // ---- the store: row al of the tile is GB consecutive floats of k's row a0 + al
  if (kvec) {
    for (int f = tid; f < GA * (GB / 4); f += GTHREADS) {
      const int al = f / (GB / 4), c = (f % (GB / 4)) * 4;
      if (a0 + al >= na || b0 + c >= nb) continue;
      float* dst = k + (a0 + al) * ldk + b0 + c;
      const float4 v = *reinterpret_cast<const float4*>(kt + al * GKT + c);
      if (b0 + c + 4 <= nb) {
        *reinterpret_cast<float4*>(dst) = v;
      } else {
        const float e[4] = {v.x, v.y, v.z, v.w};
        for (int i = 0; i < 4 && b0 + c + i < nb; ++i) dst[i] = e[i];
      }
    }
  } else {
    for (int f = tid; f < GA * GB; f += GTHREADS) {
      const int al = f / GB, c = f % GB;
      if (a0 + al < na && b0 + c < nb) k[(a0 + al) * ldk + b0 + c] = kt[al * GKT + c];
    }
  }
  if (self && blockIdx.x < blockIdx.y) {   // the mirror tile: row b0 + c of k, GA consecutive floats from column a0
    for (int f = tid; f < GA * GB; f += GTHREADS) {
      const int c = f / GA, al = f % GA;
      if (a0 + al < na && b0 + c < nb) k[(b0 + c) * ldk + a0 + al] = kt[al * GKT + c];
    }
  }
}

// ------------------------------------------------------------------------------------------------ SMO
constexpr int ST = 1024;                     // threads of the one workgroup a problem gets
constexpr int SW = ST / 64;                  // its waves
constexpr int S_RPT = AW_SVM_MAX_N / ST;     // rows per thread at full size
static_assert(S_RPT * ST == AW_SVM_MAX_N && S_RPT <= 32, "the row masks are 32-bit words");
constexpr int S_NONE = 0x7FFFFFFF;           // "no row": above every row index
constexpr double S_TAU = 1e-12;

struct svm_params {
  double C[AW_SVM_MAX_P];
};

// what the winning lane of a wave posts for the block: the first reduction uses (val, idx, y, kd) = (m, i, y_i, k_ii)
// and low = the wave's min of v over I_low; the second (val, idx, y, v, quad) = (-b^2 / a, j, y_j, v_j, a).
struct svm_post {
  double val, v, quad, low;
  int idx, y;
  float kd;
};

__device__ __forceinline__ __amdgpu_buffer_rsrc_t svm_rsrc(const void* base, uint32_t bytes) {
  return __builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(base), (short)0, (int)bytes, 0x00020000);
}
typedef unsigned int svm_u32x2 __attribute__((ext_vector_type(2)));
__device__ __forceinline__ double svm_ld_f64(__amdgpu_buffer_rsrc_t r, int voff, int soff) {
  const svm_u32x2 u = __builtin_amdgcn_raw_buffer_load_b64(r, voff, soff, 0);
  return __hiloint2double((int)u.y, (int)u.x);
}

struct svm_pending {
  double ai, aj;
  int i, j;
};

// max of val, the lower idx on a tie, over the wave (every lane ends with the same pair)
__device__ __forceinline__ void svm_wave_argmax(double& val, int& idx) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const double ov = __shfl_xor(val, o, 64);
    const int oi = __shfl_xor(idx, o, 64);
    const bool take = (ov > val) | ((ov == val) & (oi < idx));
    val = take ? ov : val;
    idx = take ? oi : idx;
  }
}
__device__ __forceinline__ double svm_wave_min(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const double ov = __shfl_xor(v, o, 64);
    v = ov < v ? ov : v;
  }
  return v;
}

// the block's result from the waves' posts: lane l folds post l & 15 with a butterfly over 16 lanes (the same total
// order, so the same pair in every thread); the payload is then read from the post of the wave that owns row idx
__device__ __forceinline__ void svm_block_argmax(const svm_post* post, int lane, double& val, int& idx, double* low) {
  const svm_post& p = post[lane & (SW - 1)];
  val = p.val, idx = p.idx;
  double lo = low ? p.low : 0.0;
#pragma unroll
  for (int o = SW / 2; o > 0; o >>= 1) {
    const double ov = __shfl_xor(val, o, 64);
    const int oi = __shfl_xor(idx, o, 64);
    const bool take = (ov > val) | ((ov == val) & (oi < idx));
    val = take ? ov : val;
    idx = take ? oi : idx;
    if (low) {
      const double ol = __shfl_xor(lo, o, 64);
      lo = ol < lo ? ol : lo;
    }
  }
  if (low) *low = lo;
}

template <int RPT>
__global__ __launch_bounds__(ST) void svm_smo_kernel(const float* __restrict__ k, int n, int64_t ldk,
                                                     const int* __restrict__ y, svm_params prm, double tol,
                                                     int max_iter, double* alpha, double* grad,
                                                     int64_t* __restrict__ n_iter, double* __restrict__ gap_out) {
  __shared__ svm_post post[2][SW];
  // Per-thread parking in LDS, [slot][thread] (a thread only ever reads what it wrote): row i of k between the j
  // selection and the gradient update, and the kernel diagonal -- 2 x 20 registers at full size, which together with
  // the 40 of v and a row in flight would not fit the 128 a 1024-thread workgroup has.  At full size the two arrays
  // alone would fill the 160 KiB, so the last slot's diagonal stays in a register.
  constexpr int KD_LDS = RPT == S_RPT ? RPT - 1 : RPT;
  __shared__ float ki_s[RPT * ST];
  __shared__ float kd_s[KD_LDS * ST];
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const int c = blockIdx.x;
  const double C = prm.C[c];
  const int* yc = y + (int64_t)c * n;
  double* ac = alpha + (int64_t)c * n;
  double* gc = grad + (int64_t)c * n;
  const double inf = __builtin_huge_val();

  // Every per-row read goes through a raw buffer descriptor over exactly the n values of its array: a slot past the
  // end reads zeros (y = 0: the row takes no part), with one thread offset and a scalar slot offset for all slots.
  const __amdgpu_buffer_rsrc_t y_rs = svm_rsrc(yc, (uint32_t)n * 4u), a_rs = svm_rsrc(ac, (uint32_t)n * 8u),
                               g_rs = svm_rsrc(gc, (uint32_t)n * 8u);
  double V[RPT];   // v_t = -y_t G_t: what both selections compare.  G_t += y_t d is v_t -= d for either sign, exactly
  float kd_last = 0.f;
  uint32_t up = 0, low = 0, pos = 0, neg = 0;   // bit s: row tid + ST s is in I_up / in I_low / has y > 0 / y < 0
#pragma unroll
  for (int s = 0; s < RPT; ++s) {
    const int yt = (int)__builtin_amdgcn_raw_buffer_load_b32(y_rs, tid * 4, s * ST * 4, 0);
    const double at = svm_ld_f64(a_rs, tid * 8, s * ST * 8);
    const double gt = svm_ld_f64(g_rs, tid * 8, s * ST * 8);
    V[s] = yt > 0 ? -gt : gt;
    const int t = tid + ST * s;
    const float ktt = n > 0 ? k[yt != 0 ? (int64_t)t * (ldk + 1) : 0] : 0.f;   // yt != 0 implies t < n
    if (s < KD_LDS)
      kd_s[s * ST + tid] = ktt;
    else
      kd_last = ktt;
    const bool lo = at <= 0.0, hi = at >= C;
    pos |= (uint32_t)(yt > 0) << s;
    neg |= (uint32_t)(yt < 0) << s;
    up |= (uint32_t)(yt > 0 ? !hi : yt < 0 ? !lo : false) << s;
    low |= (uint32_t)(yt > 0 ? !lo : yt < 0 ? !hi : false) << s;
  }

  asm volatile("" : "+v"(up), "+v"(low), "+v"(pos), "+v"(neg));   // four words from here on, not their partial ORs

  auto slot_v = [&](int sl) {
    double r = 0.0;
#pragma unroll
    for (int s = 0; s < RPT; ++s) r = s == sl ? V[s] : r;
    return r;
  };
  auto slot_kd = [&](int sl) { return sl < KD_LDS ? kd_s[sl * ST + tid] : kd_last; };

  int it = 0;
  double gap;
  __shared__ svm_pending pend;    // thread 0's alone: the pair whose new alpha is still to be written
  if (tid == 0) pend.i = S_NONE;
  for (;;) {
    // ---- i = argmax of v = -y G over I_up (value m), M = min of v over I_low.  The loops carry (value, row) only:
    //      what else the block needs of the winning row, its one owner looks up afterwards (slot_v / slot_kd).
    double bm = -inf, bM = inf;
    int bi = S_NONE;
#pragma unroll
    for (int s = 0; s < RPT; ++s) {
      const double v = V[s];
      const bool cu = (up >> s & 1) & (v > bm), cl = (low >> s & 1) & (v < bM);
      bm = cu ? v : bm;
      bi = cu ? tid + ST * s : bi;
      bM = cl ? v : bM;
    }
    {
      double wm = bm;
      int wi = bi;
      svm_wave_argmax(wm, wi);
      const double wM = svm_wave_min(bM);
      if (wi == S_NONE ? lane == 0 : wi == bi) {
        svm_post& p = post[0][wv];
        const int sl = (wi == S_NONE ? 0 : wi) / ST;
        p.val = wm, p.idx = wi, p.y = (pos >> sl & 1) ? 1 : -1, p.kd = slot_kd(sl);
      }
      if (lane == 0) post[0][wv].low = wM;
    }
    __syncthreads();
    // the previous iteration's alpha: every thread read the old values before this barrier, none reads before the next
    if (tid == 0 && pend.i != S_NONE) {
      ac[pend.i] = pend.ai, ac[pend.j] = pend.aj;
      pend.i = S_NONE;
    }
    double m, M;
    int i;
    svm_block_argmax(post[0], lane, m, i, &M);
    const int yi = i == S_NONE ? 0 : post[0][(i & (ST - 1)) >> 6].y;
    const float kii = i == S_NONE ? 0.f : post[0][(i & (ST - 1)) >> 6].kd;
    gap = m - M;
    if (!(gap > tol) || it >= max_iter || i == S_NONE) break;

    // ---- row i of k, then j = argmin of -b^2 / a over I_low with v < m
    const __amdgpu_buffer_rsrc_t ki_rs =
        svm_rsrc(k + (int64_t)__builtin_amdgcn_readfirstlane(i) * ldk, (uint32_t)n * 4u);
    {
      float Ki[RPT];   // all of the row's loads in flight at once, then out of the registers
#pragma unroll
      for (int s = 0; s < RPT; ++s)
        Ki[s] = __uint_as_float(__builtin_amdgcn_raw_buffer_load_b32(ki_rs, tid * 4, s * ST * 4, 0));
#pragma unroll
      for (int s = 0; s < RPT; ++s) ki_s[s * ST + tid] = Ki[s];
      asm volatile("" ::: "memory");   // the values are read back from LDS below, not kept
    }
    // b^2 / a of row slot s against row i (the reduction maximises it), with v and a for the update
    auto pair_gain = [&](int s, double v, float ktt, double& a) {
      const double bd = m - v;
      a = ((double)kii + (double)ktt) - 2.0 * (double)ki_s[s * ST + tid];
      if (a <= 0.0) a = S_TAU;
      return (bd * bd) / a;
    };
    double bo = -inf;
    int bj = S_NONE;
#pragma unroll
    for (int s = 0; s < RPT; ++s) {
      double a;
      const double v = V[s];
      const double o = pair_gain(s, v, slot_kd(s), a);
      const bool cj = (low >> s & 1) & (v < m) & (o > bo);
      bo = cj ? o : bo;
      bj = cj ? tid + ST * s : bj;
      // one division chain at a time: the SIMD's other three waves fill its latencies, and RPT chains interleaved
      // would hold their temporaries RPT times over
      __builtin_amdgcn_sched_barrier(0);
    }
    {
      double wo = bo;
      int wj = bj;
      svm_wave_argmax(wo, wj);
      if (wj == S_NONE ? lane == 0 : wj == bj) {
        svm_post& p = post[1][wv];
        const int sl = (wj == S_NONE ? 0 : wj) / ST;
        double a;
        const double v = slot_v(sl);
        pair_gain(sl, v, slot_kd(sl), a);   // the same operations on the same values: the same bits
        p.val = wo, p.idx = wj, p.y = (pos >> sl & 1) ? 1 : -1, p.v = v, p.quad = a;
      }
    }
    __syncthreads();
    double o;
    int j;
    svm_block_argmax(post[1], lane, o, j, nullptr);
    if (j == S_NONE) break;   // no candidate (only a NaN gradient gets here)

    // ---- row j's read is in flight under the two-variable update (libsvm's, with its clipping to the box)
    const svm_post& pw = post[1][(j & (ST - 1)) >> 6];
    const int yj = pw.y;
    const double vj = pw.v, quad = pw.quad;
    const __amdgpu_buffer_rsrc_t kj_rs =
        svm_rsrc(k + (int64_t)__builtin_amdgcn_readfirstlane(j) * ldk, (uint32_t)n * 4u);
    float Kj[RPT];
#pragma unroll
    for (int s = 0; s < RPT; ++s)
      Kj[s] = __uint_as_float(__builtin_amdgcn_raw_buffer_load_b32(kj_rs, tid * 4, s * ST * 4, 0));
    const double Gi = yi > 0 ? -m : m, Gj = yj > 0 ? -vj : vj;
    const double oai = ac[i], oaj = ac[j];
    double ai = oai, aj = oaj;
    if (yi != yj) {
      const double delta = (-Gi - Gj) / quad, diff = ai - aj;
      ai += delta, aj += delta;
      if (diff > 0) {
        if (aj < 0) aj = 0, ai = diff;
      } else {
        if (ai < 0) ai = 0, aj = -diff;
      }
      if (diff > 0) {
        if (ai > C) ai = C, aj = C - diff;
      } else {
        if (aj > C) aj = C, ai = C + diff;
      }
    } else {
      const double delta = (Gi - Gj) / quad, sum = ai + aj;
      ai -= delta, aj += delta;
      if (sum > C) {
        if (ai > C) ai = C, aj = sum - C;
      } else {
        if (aj < 0) aj = 0, ai = sum;
      }
      if (sum > C) {
        if (aj > C) aj = C, ai = sum - C;
      } else {
        if (ai < 0) ai = 0, aj = sum;
      }
    }
    if (tid == 0) pend.i = i, pend.j = j, pend.ai = ai, pend.aj = aj;
    // G_t += Q_ti dalpha_i + Q_tj dalpha_j, Q_ts = y_t y_s k_ts: the signs move out of the products exactly
    const double ci = yi > 0 ? ai - oai : -(ai - oai), cj = yj > 0 ? aj - oaj : -(aj - oaj);
#pragma unroll
    for (int s = 0; s < RPT; ++s) {
      const double d = (double)ki_s[s * ST + tid] * ci + (double)Kj[s] * cj;
      V[s] = ((pos | neg) >> s & 1) ? V[s] - d : V[s];
      if (s % 2 == 1) __builtin_amdgcn_sched_barrier(0);   // two rows' temporaries at a time, not RPT
    }
    // the two rows' membership of I_up / I_low, by their owners
#pragma unroll
    for (int e = 0; e < 2; ++e) {
      const int t = e ? j : i, yt = e ? yj : yi;
      const double at = e ? aj : ai;
      if ((t & (ST - 1)) == tid) {
        const uint32_t bit = 1u << (t / ST);
        const bool lo = at <= 0.0, hi = at >= C;
        const bool u = yt > 0 ? !hi : !lo, l = yt > 0 ? !lo : !hi;
        up = u ? up | bit : up & ~bit;
        low = l ? low | bit : low & ~bit;
      }
    }
    ++it;
  }

  if (it > 0) {
    int t0 = tid;
    asm volatile("" : "+v"(t0));   // the store addresses are formed here, not carried through the loop
#pragma unroll
    for (int s = 0; s < RPT; ++s)
      if ((pos | neg) >> s & 1) gc[t0 + ST * s] = (pos >> s & 1) ? -V[s] : V[s];
  }
  if (tid == 0) {
    n_iter[c] += it;
    gap_out[c] = gap;
  }
}

int gram_check(int64_t na, int64_t nb, int d, int64_t lda, int64_t ldb, int64_t ldk, float gamma) {
  AW_REQUIRE(na >= 0 && na < ((int64_t)1 << 31), "aw_rbf_gram: na = %lld outside 0..2^31 - 1", (long long)na);
  AW_REQUIRE(nb >= 0 && nb <= (int64_t)65535 * GB, "aw_rbf_gram: nb = %lld outside 0..%lld", (long long)nb,
             (long long)65535 * GB);
  AW_REQUIRE(d >= 1, "aw_rbf_gram: d = %d, need d >= 1", d);
  AW_REQUIRE(lda >= d && ldb >= d && lda < (1 << 22) && ldb < (1 << 22),
             "aw_rbf_gram: row strides lda = %lld, ldb = %lld must lie in d = %d .. 2^22 - 1", (long long)lda,
             (long long)ldb, d);
  AW_REQUIRE(ldk >= nb, "aw_rbf_gram: ldk = %lld below nb = %lld", (long long)ldk, (long long)nb);
  AW_REQUIRE(gamma > 0.f && gamma <= 3.402823466e38f, "aw_rbf_gram: gamma = %g must be finite and positive",
             (double)gamma);
  return AW_OK;
}

}  // namespace

extern "C" int aw_rbf_gram_describe(int* tile_a, int* tile_b, int* chunk_d) {
  if (tile_a) *tile_a = GA;
  if (tile_b) *tile_b = GB;
  if (chunk_d) *chunk_d = GD;
  return AW_OK;
}

extern "C" int aw_rbf_gram(const float* a, int64_t na, int64_t lda, const float* b, int64_t nb, int64_t ldb, int d,
                           float gamma, float* k, int64_t ldk, void* stream) {
  const int st = gram_check(na, nb, d, lda, ldb, ldk, gamma);
  if (st != AW_OK) return st;
  if (na == 0 || nb == 0) return AW_OK;
  AW_REQUIRE(a && b && k, "aw_rbf_gram: a, b and k must not be NULL");
  AW_REQUIRE(((uintptr_t)a & 3) == 0 && ((uintptr_t)b & 3) == 0 && ((uintptr_t)k & 3) == 0,
             "aw_rbf_gram: a, b and k must be 4-byte aligned");
  const bool avec = ((uintptr_t)a & 15) == 0 && (lda & 3) == 0;   // 16-B loads: aligned base and stride
  const bool bvec = ((uintptr_t)b & 15) == 0 && (ldb & 3) == 0;
  const int kvec = ((uintptr_t)k & 15) == 0 && (ldk & 3) == 0;
  const int self = a == b && lda == ldb && na == nb;   // only the tiles on or above the diagonal are computed
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  const dim3 grid((unsigned)((na + GA - 1) / GA), (unsigned)((nb + GB - 1) / GB)), block(GTHREADS);
#define GRAM_LAUNCH(AV, BV) \
  hipLaunchKernelGGL((rbf_gram_kernel<AV, BV>), grid, block, 0, s, a, na, lda, b, nb, ldb, d, gamma, k, ldk, kvec, \
                     self)
  if (avec && bvec)
    GRAM_LAUNCH(true, true);
  else if (avec)
    GRAM_LAUNCH(true, false);
  else if (bvec)
    GRAM_LAUNCH(false, true);
  else
    GRAM_LAUNCH(false, false);
#undef GRAM_LAUNCH
  return aw::check_launch("aw_rbf_gram");
}

extern "C" int aw_svm_describe(int* threads, int* rows_per_thread, int* max_n, int* max_p) {
  if (threads) *threads = ST;
  if (rows_per_thread) *rows_per_thread = S_RPT;
  if (max_n) *max_n = AW_SVM_MAX_N;
  if (max_p) *max_p = AW_SVM_MAX_P;
  return AW_OK;
}

extern "C" int aw_svm_smo(const float* k, int n, int64_t ldk, const int* y, const double* C, int p, double tol,
                          int max_iter, double* alpha, double* grad, int64_t* n_iter, double* gap, void* stream) {
  AW_REQUIRE(n >= 0 && n <= AW_SVM_MAX_N, "aw_svm_smo: n = %d outside 0..%d", n, AW_SVM_MAX_N);
  AW_REQUIRE(p >= 1 && p <= AW_SVM_MAX_P, "aw_svm_smo: p = %d outside 1..%d", p, AW_SVM_MAX_P);
  AW_REQUIRE(ldk >= n, "aw_svm_smo: ldk = %lld below n = %d", (long long)ldk, n);
  AW_REQUIRE(tol > 0.0, "aw_svm_smo: tol = %g must be positive", tol);
  AW_REQUIRE(max_iter >= 0, "aw_svm_smo: max_iter = %d is negative", max_iter);
  AW_REQUIRE(C && n_iter && gap, "aw_svm_smo: C, n_iter and gap must not be NULL");
  AW_REQUIRE(n == 0 || (k && y && alpha && grad), "aw_svm_smo: k, y, alpha and grad must not be NULL with n = %d", n);
  svm_params prm;
  for (int c = 0; c < AW_SVM_MAX_P; ++c) prm.C[c] = 1.0;
  for (int c = 0; c < p; ++c) {
    AW_REQUIRE(C[c] > 0.0 && C[c] <= 1.7976931348623157e308, "aw_svm_smo: C[%d] = %g must be finite and positive", c,
               C[c]);
    prm.C[c] = C[c];
  }
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  const dim3 grid((unsigned)p), block(ST);
  // the instantiations differ in the length of the register arrays only: the same bits from each
#define SMO_LAUNCH(R) \
  hipLaunchKernelGGL((svm_smo_kernel<R>), grid, block, 0, s, k, n, ldk, y, prm, tol, max_iter, alpha, grad, n_iter, gap)
  if (n <= 2 * ST)
    SMO_LAUNCH(2);
  else if (n <= 8 * ST)
    SMO_LAUNCH(8);
  else
    SMO_LAUNCH(S_RPT);
#undef SMO_LAUNCH
  return aw::check_launch("aw_svm_smo");
}
