// The TS2Vec hierarchical contrastive loss (aw_nce_rows_fwd / aw_nce_rows_bwd, aw_ts_pool2_fwd / aw_ts_pool2_bwd;
// include/arcweld_amd.h): the hot path of arcweld.ts2vec.hierarchical_contrastive_loss.  Both of the reference's terms
// (model/ts2vec/losses.py) are one operation, the paired InfoNCE over groups: a group is 2 n rows of c floats, rows
// 0..n-1 from z1 and n..2n-1 from z2, S = Z Z^T within the group, lse_i = log sum_{j != i} exp S_ij,
// row_loss_i = lse_i - S_{i, p(i)} with p(i) = (i + n) mod 2n.  No similarity is ever written to memory.
//
//   nce_fwd_kernel    grid (row tiles, groups).  The 2 n rows of a group are tiled per half: tiles 0..nt-1 are rows of
//                     z1, nt..2nt-1 rows of z2 (nt = ceil(n / 128)), so one tile is one buffer descriptor.  A 256-thread
//                     workgroup owns one tile as the B operand of pair_tile.h and sweeps all 2 nt tiles as the A
//                     operand: per column tile the K loop over c (fetch / stage_put / mfma_dots: buffer loads that
//                     return zeros out of range, two LDS stages, one barrier per chunk; the next tile's first chunk is
//                     fetched under the last chunk's MFMAs), then, in registers, a running maximum and sum of
//                     exponentials per (own row, lane): a lane holds 32 columns of each of its two own rows.  The
//                     diagonal and the columns past n never enter; the lane that meets S_{i, p(i)} posts it.  The four
//                     partial (max, sum) of a row -- two lane halves, two waves -- are merged in one fixed order.
//                     One row's lse is therefore accumulated in one order, whatever the grid: its bits depend on
//                     neither the number of groups nor the group's position, nor the run.  No atomics.
//   nce_bwd_kernel    grid (row tiles, groups, slabs of 128 output columns).  Same ownership and K loop; per column
//                     tile S is recomputed (bit for bit the forward's), Q = exp(S - lse_i) + exp(S - lse_j) (both
//                     exponents <= 0: lse >= every S it covers) with the diagonal and the padding at 0, and
//                     dZ_i += Q . Z_j runs as a second GEMM on the same MFMA core with the pair index j as the dims:
//                     Q and the transposed slab of Z_j go to LDS over the idle stages, 64 pairs at a time.  The
//                     epilogue subtracts 2 Z_{p(i)}, scales, and stores or adds into dz: every element has one owner.
//   packed kernels    groups of 2 n <= 128 rows (the instance term at any batch up to 64, the deep temporal levels):
//                     128 / S whole groups per workgroup in slots of S = 32, 64 or 128 rows, one tile pair, the same
//                     epilogues with the other slots masked; see "packed small groups" below.
//   pool2 kernels     the hierarchy's max-pool over time (kernel 2, stride 2, an odd last step dropped) and its
//                     backward, which recomputes the argmax from the input (the first step on a tie, as torch does) and
//                     adds into the shallower level's gradient.
#include "common.h"
#include "pair_tile.h"

#include <math.h>

namespace {

namespace pt = aw::pt;
constexpr int NT = pt::TB;            // rows per tile, own (B operand) and column (A operand)
constexpr int NTHREADS = pt::THREADS;
constexpr int SLAB = 128;             // output columns of one backward workgroup
constexpr int PH = 64;                // pairs per step of the second GEMM
constexpr int PLD = PH + 4;           // row stride of Q and of the transposed Z slab in LDS
constexpr float NEG_BIG = -3.0e38f;   // "no value yet": below every similarity, and finite (no inf - inf)
static_assert(NT == pt::TA && SLAB == pt::TA, "mfma_dots' 128 x 128 block");
static_assert((NT + SLAB) * PLD <= 2 * pt::STAGE, "Q and the Z slab overlay the two stages");
static_assert((2 * pt::STAGE + 6 * NT) * 4 <= 80 * 1024, "two workgroups per CU");

struct nce_geom {
  int n, c, nt;                       // rows per half, dims, tiles per half
  int64_t gs, rs;                     // group and row stride (floats)
};

__device__ __forceinline__ pt::Operand tile_operand(const float* z1, const float* z2, const nce_geom& q, int g,
                                                    int tile) {
  const float* z = (tile >= q.nt ? z2 : z1) + (int64_t)g * q.gs;
  return pt::operand(z, (int64_t)(tile % q.nt) * NT, q.n, q.rs, q.c, NT);
}

// S of own tile `bo` against column tile ct into acc.  CARRY: `pre` holds chunk 0 of that pair on entry and chunk 0
// of the next pair on exit (fetched under the last chunk's MFMAs); otherwise chunk 0 is fetched here and `pre` is dead
// between tiles.  The stages alternate across tiles: the one written next was last read before the last barrier.
template <bool CARRY>
__device__ __forceinline__ void s_tile(float* stage, int& buf, float4 (&pre)[pt::F4], const pt::Operand& bo,
                                       const float* z1, const float* z2, const nce_geom& q, int g, int ct, int tid,
                                       pt::f32x16 (&acc)[2][2]) {
  __builtin_assume((q.c & 15) == 0);   // the host's check: fetch's path for a quad that straddles the width is dead
  const int nch = (q.c + pt::TD - 1) / pt::TD;
  const pt::Operand ao = tile_operand(z1, z2, q, g, ct);
  pt::zero(acc);
  if (!CARRY) pt::fetch<true, true>(pre, bo, ao, 0, q.c, tid);
  for (int ch = 0; ch < nch; ++ch) {
    float* sb = stage + buf * pt::STAGE;
    pt::stage_put(sb, pre, tid);
    __syncthreads();
    if (ch + 1 < nch) {
      pt::fetch<true, true>(pre, bo, ao, ch + 1, q.c, tid);
    } else if (CARRY && ct + 1 < 2 * q.nt) {
      const pt::Operand an = tile_operand(z1, z2, q, g, ct + 1);
      pt::fetch<true, true>(pre, bo, an, 0, q.c, tid);
    }
    if (CARRY) {
      pt::mfma_dots<pt::LD, pt::LD, pt::TD>(sb + pt::TB * pt::LD, sb, tid, acc);
    } else {   // beside the backward's second accumulator set: half a chunk's operands in registers at a time
      pt::mfma_dots<pt::LD, pt::LD, pt::TD / 2>(sb + pt::TB * pt::LD, sb, tid, acc);
      __builtin_amdgcn_sched_barrier(0);
      pt::mfma_dots<pt::LD, pt::LD, pt::TD / 2>(sb + pt::TB * pt::LD + pt::TD / 2, sb + pt::TD / 2, tid, acc);
    }
    buf ^= 1;
  }
}

__global__ __launch_bounds__(NTHREADS, 2) void nce_fwd_kernel(const float* __restrict__ z1,
                                                              const float* __restrict__ z2, nce_geom q,
                                                              float* __restrict__ lse, float* __restrict__ row_loss) {
  __shared__ __attribute__((aligned(16))) float stage[2 * pt::STAGE];
  __shared__ float part_m[2][NT], part_s[2][NT], partner_s[NT];
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, h = lane >> 5, jr = lane & 31;
  const int g = blockIdx.y, tile = blockIdx.x;
  const int hb = tile >= q.nt, r0 = (tile % q.nt) * NT;
  const pt::Operand bo = tile_operand(z1, z2, q, g, tile);

  float m[2] = {NEG_BIG, NEG_BIG}, s[2] = {0.f, 0.f};
  float4 pre[pt::F4];
  __builtin_assume((q.c & 15) == 0);
  pt::fetch<true, true>(pre, bo, tile_operand(z1, z2, q, g, 0), 0, q.c, tid);
  pt::f32x16 acc[2][2];
  int buf = 0;
  for (int ct = 0; ct < 2 * q.nt; ++ct) {
    s_tile<true>(stage, buf, pre, bo, z1, z2, q, g, ct, tid, acc);
    const int hc = ct >= q.nt, c0 = (ct % q.nt) * NT;
    const bool same = hc == hb;
    const int cbase = c0 + 64 * (w >> 1) + 4 * h;   // the lane's first column, in-half index
#pragma unroll
    for (int ni = 0; ni < 2; ++ni) {
      // register (mi, r) is column `lim` past the lane's first: the tests below compare tile-relative values with
      // literals (nothing for the compiler to precompute per register and keep across the sweep)
      const int bl = 64 * (w & 1) + 32 * ni + jr;
      int lim = q.n - cbase, own = r0 + bl - cbase;   // columns left in the half; the own row's in-half index
      asm volatile("" : "+v"(lim), "+v"(own));
      float tmax = NEG_BIG;
#pragma unroll
      for (int mi = 0; mi < 2; ++mi)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const int jl = 32 * mi + 8 * (r >> 2) + (r & 3);
          const float v = acc[mi][ni][r];
          const bool ok = jl < lim && !(same && jl == own);
          tmax = ok ? fmaxf(tmax, v) : tmax;
          if (!same && jl == own && jl < lim) partner_s[bl] = v;
        }
      const float mn = fmaxf(m[ni], tmax);
      float sum = s[ni] * expf(m[ni] - mn);
#pragma unroll
      for (int mi = 0; mi < 2; ++mi)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const int jl = 32 * mi + 8 * (r >> 2) + (r & 3);
          const bool ok = jl < lim && !(same && jl == own);
          const float e = expf(acc[mi][ni][r] - mn);
          sum += ok ? e : 0.f;
        }
      m[ni] = mn, s[ni] = sum;
    }
  }

  // the row's four partials: lane half 0 then 1, then column half (wave pair) 0 then 1
#pragma unroll
  for (int ni = 0; ni < 2; ++ni) {
    const float om = __shfl_xor(m[ni], 32, 64), os = __shfl_xor(s[ni], 32, 64);
    const float m0 = h ? om : m[ni], s0 = h ? os : s[ni], m1 = h ? m[ni] : om, s1 = h ? s[ni] : os;
    const float mm = fmaxf(m0, m1);
    const float ss = s0 * expf(m0 - mm) + s1 * expf(m1 - mm);
    if (h == 0) {
      const int bl = 64 * (w & 1) + 32 * ni + jr;
      part_m[w >> 1][bl] = mm, part_s[w >> 1][bl] = ss;
    }
  }
  __syncthreads();
  if (tid < NT && r0 + tid < q.n) {
    const float m0 = part_m[0][tid], m1 = part_m[1][tid];
    const float mm = fmaxf(m0, m1);
    const float ss = part_s[0][tid] * expf(m0 - mm) + part_s[1][tid] * expf(m1 - mm);
    const float l = mm + logf(ss);
    const int64_t o = (int64_t)g * 2 * q.n + (int64_t)hb * q.n + r0 + tid;
    lse[o] = l;
    row_loss[o] = l - partner_s[tid];
  }
}

__global__ __launch_bounds__(NTHREADS, 2) void nce_bwd_kernel(const float* __restrict__ z1,
                                                              const float* __restrict__ z2, nce_geom q,
                                                              const float* __restrict__ lse, float scale,
                                                              float* dz1, float* dz2, int accumulate) {
  __shared__ __attribute__((aligned(16))) float stage[2 * pt::STAGE];
  __shared__ float lse_col[NT];
  float* qs = stage;                  // [own row][pair], PH pairs, row stride PLD
  float* zt = stage + NT * PLD;       // [slab column][pair]
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, h = lane >> 5, jr = lane & 31;
  const int g = blockIdx.y, tile = blockIdx.x, cs0 = blockIdx.z * SLAB;
  const int hb = tile >= q.nt, r0 = (tile % q.nt) * NT;
  const pt::Operand bo = tile_operand(z1, z2, q, g, tile);
  const float* lse_g = lse + (int64_t)g * 2 * q.n;

  float lse_own[2];
#pragma unroll
  for (int ni = 0; ni < 2; ++ni) {
    const int ib = r0 + 64 * (w & 1) + 32 * ni + jr;
    lse_own[ni] = ib < q.n ? lse_g[(int64_t)hb * q.n + ib] : 0.f;
  }

  float4 pre[pt::F4];
  pt::f32x16 acc[2][2], dacc[2][2];   // dacc[slab column tile mi][own row tile ni]
  pt::zero(dacc);
  int buf = 0;
  for (int ct = 0; ct < 2 * q.nt; ++ct) {
    const int hc = ct >= q.nt, c0 = (ct % q.nt) * NT;
    const bool same = hc == hb;
    if (tid < NT) lse_col[tid] = c0 + tid < q.n ? lse_g[(int64_t)hc * q.n + c0 + tid] : 0.f;   // read after a barrier
    s_tile<false>(stage, buf, pre, bo, z1, z2, q, g, ct, tid, acc);
    const pt::Operand ao = tile_operand(z1, z2, q, g, ct);
#pragma unroll
    for (int h2 = 0; h2 < 2; ++h2) {
      // the slab of Z_j, pairs 64 h2 .. + 63: thread (jl, qd) of wave w takes 4 columns of one pair per step, so a
      // wave's transposing LDS stores of one component hit 64 different banks (16 qd + jl + 4 k)
      __syncthreads();                // the stages (or the previous step's Q and Z) have been read
      if ((w >> 1) == h2) {
#pragma unroll
        for (int ni = 0; ni < 2; ++ni) {
          // tile-relative tests against literals, as in the forward
          const int bl = 64 * (w & 1) + 32 * ni + jr;
          int lim = q.n - (c0 + 64 * h2 + 4 * h), own = r0 + bl - (c0 + 64 * h2 + 4 * h);
          asm volatile("" : "+v"(lim), "+v"(own));
          const float* lc = lse_col + 64 * h2 + 4 * h;
          float* qrow = qs + bl * PLD + 4 * h;
#pragma unroll
          for (int mi = 0; mi < 2; ++mi)
#pragma unroll
            for (int r4 = 0; r4 < 4; ++r4) {
              float e[4];
#pragma unroll
              for (int k = 0; k < 4; ++k) {
                const int jl = 32 * mi + 8 * r4 + k;
                const float v = acc[mi][ni][4 * r4 + k];
                const bool ok = jl < lim && !(same && jl == own);
                const float qv = expf(v - lse_own[ni]) + expf(v - lc[jl]);
                e[k] = ok ? qv : 0.f;
              }
              *reinterpret_cast<float4*>(qrow + 32 * mi + 8 * r4) = make_float4(e[0], e[1], e[2], e[3]);
              __builtin_amdgcn_sched_barrier(0);   // four values' exponentials at a time, not all 64 interleaved
            }
        }
      }
      float4 zl[8];                   // loaded after Q is formed: Q's exponentials and these never share registers
#pragma unroll
      for (int it = 0; it < 8; ++it) {
        const int u = it * 4 + w, jb = u & 3, cb = u >> 2;
        zl[it] = pt::ld4<true>(ao.rsrc, PH * h2 + 16 * jb + (lane >> 2), ao.rows, ao.ld_bytes,
                               cs0 + 16 * cb + 4 * (lane & 3), q.c);
      }
#pragma unroll
      for (int it = 0; it < 8; ++it) {
        const int u = it * 4 + w, jb = u & 3, cb = u >> 2;
        float* d = zt + (16 * cb + 4 * (lane & 3)) * PLD + 16 * jb + (lane >> 2);
        d[0] = zl[it].x, d[PLD] = zl[it].y, d[2 * PLD] = zl[it].z, d[3 * PLD] = zl[it].w;
      }
      __syncthreads();
      // 32 pairs at a time: the operands of all 64 read up front would not fit beside the two accumulator sets
      pt::mfma_dots<PLD, PLD, PH / 2>(zt, qs, tid, dacc);
      __builtin_amdgcn_sched_barrier(0);
      pt::mfma_dots<PLD, PLD, PH / 2>(zt + PH / 2, qs + PH / 2, tid, dacc);
    }
    __syncthreads();                  // Q and Z have been read: the next tile stages over them
  }

  // dz[i, col] (+)= scale (sum_j Q_ij Z_j[col] - 2 Z_p(i)[col]); four consecutive registers are four columns
  float* dz = (hb ? dz2 : dz1) + (int64_t)g * q.gs;
  const float* zp = (hb ? z1 : z2) + (int64_t)g * q.gs;
#pragma unroll
  for (int ni = 0; ni < 2; ++ni) {
    const int ib = r0 + 64 * (w & 1) + 32 * ni + jr;
    if (ib >= q.n) continue;
#pragma unroll
    for (int mi = 0; mi < 2; ++mi)
#pragma unroll
      for (int r4 = 0; r4 < 4; ++r4) {
        const int col = cs0 + 64 * (w >> 1) + 32 * mi + 8 * r4 + 4 * h;
        if (col >= q.c) continue;
        const int64_t o = (int64_t)ib * q.rs + col;
        const float4 p = *reinterpret_cast<const float4*>(zp + o);
        float4 v;
        v.x = scale * fmaf(-2.f, p.x, dacc[mi][ni][4 * r4 + 0]);
        v.y = scale * fmaf(-2.f, p.y, dacc[mi][ni][4 * r4 + 1]);
        v.z = scale * fmaf(-2.f, p.z, dacc[mi][ni][4 * r4 + 2]);
        v.w = scale * fmaf(-2.f, p.w, dacc[mi][ni][4 * r4 + 3]);
        if (accumulate) {
          const float4 old = *reinterpret_cast<const float4*>(dz + o);
          v.x = __fadd_rn(old.x, v.x), v.y = __fadd_rn(old.y, v.y), v.z = __fadd_rn(old.z, v.z),
          v.w = __fadd_rn(old.w, v.w);
        }
        *reinterpret_cast<float4*>(dz + o) = v;
      }
  }
}

// ------------------------------------------------------------------------------------------------ packed small groups
// Groups of 2 n <= 128 rows (the instance term: 2 B rows per time step; the deep levels of the temporal term): one
// workgroup holds 128 / S whole groups, each in a slot of S = 32, 64 or 128 tile rows (rows 0..n-1 of a slot from z1,
// n..2n-1 from z2, the rest zeros), as BOTH operands of one tile pair, and columns of another slot are masked like
// the padding.  Slots are multiples of 32 rows: moving a group to another slot changes which accumulator holds its
// similarities, not the order within a lane (MFMA step and register order repeat every 32 rows), and what it leaves
// behind are exact zeros in every sum, so a row's bits still do not depend on the group's position.
struct nce_pack {
  int n, c, groups, slot_log2;
  int64_t gs, rs;
};

struct pack_src {
  __amdgpu_buffer_rsrc_t r1, r2;      // z1 / z2 from the workgroup's first group to the end of its last
  int pv;                             // groups of this workgroup that exist
  uint32_t gs_bytes, rs_bytes;
};

__device__ __forceinline__ pack_src pack_source(const float* z1, const float* z2, const nce_pack& q, int g0) {
  pack_src s;
  const int per = NT >> q.slot_log2;
  s.pv = q.groups - g0 < per ? q.groups - g0 : per;
  const uint32_t bytes = (uint32_t)(((int64_t)(s.pv - 1) * q.gs + (int64_t)(q.n - 1) * q.rs + q.c) * 4);
  s.r1 = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(z1 + (int64_t)g0 * q.gs), (short)0, (int)bytes, 0x00020000);
  s.r2 = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(z2 + (int64_t)g0 * q.gs), (short)0, (int)bytes, 0x00020000);
  s.gs_bytes = (uint32_t)q.gs * 4u, s.rs_bytes = (uint32_t)q.rs * 4u;
  return s;
}

// dims d0 .. d0 + 3 of tile row l: one of the two loads is masked and returns zeros
__device__ __forceinline__ float4 pack_ld4(const pack_src& s, const nce_pack& q, int l, int d0) {
  const int p = l >> q.slot_log2, r = l & ((1 << q.slot_log2) - 1);
  const bool live = p < s.pv && d0 + 4 <= q.c;
  const bool in1 = live && r < q.n, in2 = live && r >= q.n && r < 2 * q.n;
  const uint32_t base = (uint32_t)p * s.gs_bytes + 4u * (uint32_t)d0;
  const pt::u32x4 a = __builtin_amdgcn_raw_buffer_load_b128(s.r1, in1 ? base + (uint32_t)r * s.rs_bytes : pt::BAD_OFF, 0, 0);
  const pt::u32x4 b =
      __builtin_amdgcn_raw_buffer_load_b128(s.r2, in2 ? base + (uint32_t)(r - q.n) * s.rs_bytes : pt::BAD_OFF, 0, 0);
  const pt::u32x4 u = a | b;
  return make_float4(__uint_as_float(u.x), __uint_as_float(u.y), __uint_as_float(u.z), __uint_as_float(u.w));
}

// chunk ch of the tile, staged as both operands
__device__ __forceinline__ void pack_fetch(float4 (&pre)[pt::F4], const pack_src& s, const nce_pack& q, int ch,
                                           int tid) {
#pragma unroll
  for (int i = 0; i < pt::F4 / 2; ++i)
    pre[i] = pre[i + pt::F4 / 2] = pack_ld4(s, q, (tid >> 3) + 32 * i, ch * pt::TD + (tid & 7) * 4);
}

template <bool HALVES>
__device__ __forceinline__ void pack_s_tile(float* stage, float4 (&pre)[pt::F4], const pack_src& s, const nce_pack& q,
                                            int tid, pt::f32x16 (&acc)[2][2]) {
  const int nch = (q.c + pt::TD - 1) / pt::TD;
  pt::zero(acc);
  pack_fetch(pre, s, q, 0, tid);
  for (int ch = 0; ch < nch; ++ch) {
    float* sb = stage + (ch & 1) * pt::STAGE;
    pt::stage_put(sb, pre, tid);
    __syncthreads();
    if (ch + 1 < nch) pack_fetch(pre, s, q, ch + 1, tid);
    if (!HALVES) {
      pt::mfma_dots<pt::LD, pt::LD, pt::TD>(sb + pt::TB * pt::LD, sb, tid, acc);
    } else {
      pt::mfma_dots<pt::LD, pt::LD, pt::TD / 2>(sb + pt::TB * pt::LD, sb, tid, acc);
      __builtin_amdgcn_sched_barrier(0);
      pt::mfma_dots<pt::LD, pt::LD, pt::TD / 2>(sb + pt::TB * pt::LD + pt::TD / 2, sb + pt::TD / 2, tid, acc);
    }
  }
}

// For own tile row bl and a lane whose first column is cb: the lane's registers hold columns cb + jl, jl a literal;
// those of the row's group are lo <= jl < hi, the row itself is jl == own and its partner jl == part.
struct pack_mask {
  int lo, hi, own, part;
};
__device__ __forceinline__ pack_mask pack_masks(const nce_pack& q, int bl, int cb) {
  const int S = 1 << q.slot_log2, rb = bl & (S - 1);
  pack_mask m;
  m.lo = (bl - rb) - cb;
  m.hi = m.lo + 2 * q.n;
  m.own = m.lo + rb;
  m.part = m.lo + (rb < q.n ? rb + q.n : rb - q.n);
  asm volatile("" : "+v"(m.lo), "+v"(m.hi), "+v"(m.own), "+v"(m.part));
  return m;
}

__global__ __launch_bounds__(NTHREADS, 2) void nce_fwd_packed_kernel(const float* __restrict__ z1,
                                                                     const float* __restrict__ z2, nce_pack q,
                                                                     float* __restrict__ lse,
                                                                     float* __restrict__ row_loss) {
  __shared__ __attribute__((aligned(16))) float stage[2 * pt::STAGE];
  __shared__ float part_m[2][NT], part_s[2][NT], partner_s[NT];
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, h = lane >> 5, jr = lane & 31;
  const int g0 = blockIdx.x * (NT >> q.slot_log2);
  __builtin_assume((q.c & 15) == 0);
  const pack_src src = pack_source(z1, z2, q, g0);
  float4 pre[pt::F4];
  pt::f32x16 acc[2][2];
  pack_s_tile<false>(stage, pre, src, q, tid, acc);

#pragma unroll
  for (int ni = 0; ni < 2; ++ni) {
    const int bl = 64 * (w & 1) + 32 * ni + jr;
    const pack_mask k = pack_masks(q, bl, 64 * (w >> 1) + 4 * h);
    float mx = NEG_BIG;
#pragma unroll
    for (int mi = 0; mi < 2; ++mi)
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int jl = 32 * mi + 8 * (r >> 2) + (r & 3);
        const float v = acc[mi][ni][r];
        const bool ok = jl >= k.lo && jl < k.hi && jl != k.own;
        mx = ok ? fmaxf(mx, v) : mx;
        if (jl == k.part && jl >= k.lo && jl < k.hi) partner_s[bl] = v;
      }
    float sum = 0.f;
#pragma unroll
    for (int mi = 0; mi < 2; ++mi)
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int jl = 32 * mi + 8 * (r >> 2) + (r & 3);
        const bool ok = jl >= k.lo && jl < k.hi && jl != k.own;
        const float e = expf(acc[mi][ni][r] - mx);
        sum += ok ? e : 0.f;
      }
    // the row's four partials, merged as in nce_fwd_kernel
    const float om = __shfl_xor(mx, 32, 64), os = __shfl_xor(sum, 32, 64);
    const float m0 = h ? om : mx, s0 = h ? os : sum, m1 = h ? mx : om, s1 = h ? sum : os;
    const float mm = fmaxf(m0, m1);
    const float ss = s0 * expf(m0 - mm) + s1 * expf(m1 - mm);
    if (h == 0) part_m[w >> 1][bl] = mm, part_s[w >> 1][bl] = ss;
  }
  __syncthreads();
  const int p = tid >> q.slot_log2, r = tid & ((1 << q.slot_log2) - 1);
  if (tid < NT && p < src.pv && r < 2 * q.n) {
    const float m0 = part_m[0][tid], m1 = part_m[1][tid];
    const float mm = fmaxf(m0, m1);
    const float ss = part_s[0][tid] * expf(m0 - mm) + part_s[1][tid] * expf(m1 - mm);
    const float l = mm + logf(ss);
    const int64_t o = (int64_t)(g0 + p) * 2 * q.n + r;
    lse[o] = l;
    row_loss[o] = l - partner_s[tid];
  }
}

__global__ __launch_bounds__(NTHREADS, 2) void nce_bwd_packed_kernel(const float* __restrict__ z1,
                                                                     const float* __restrict__ z2, nce_pack q,
                                                                     const float* __restrict__ lse, float scale,
                                                                     float* dz1, float* dz2, int accumulate) {
  __shared__ __attribute__((aligned(16))) float stage[2 * pt::STAGE];
  __shared__ float lse_s[NT];
  float* qs = stage;
  float* zt = stage + NT * PLD;
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, h = lane >> 5, jr = lane & 31;
  const int S = 1 << q.slot_log2;
  const int g0 = blockIdx.x * (NT >> q.slot_log2), cs0 = blockIdx.y * SLAB;
  __builtin_assume((q.c & 15) == 0);
  const pack_src src = pack_source(z1, z2, q, g0);
  if (tid < NT) {                     // lse of tile row tid: read after the K loop's barriers
    const int p = tid >> q.slot_log2, r = tid & (S - 1);
    lse_s[tid] = p < src.pv && r < 2 * q.n ? lse[(int64_t)(g0 + p) * 2 * q.n + r] : 0.f;
  }
  float4 pre[pt::F4];
  pt::f32x16 acc[2][2], dacc[2][2];
  pt::zero(dacc);
  pack_s_tile<true>(stage, pre, src, q, tid, acc);
#pragma unroll
  for (int h2 = 0; h2 < 2; ++h2) {
    __syncthreads();
    if ((w >> 1) == h2) {
#pragma unroll
      for (int ni = 0; ni < 2; ++ni) {
        const int bl = 64 * (w & 1) + 32 * ni + jr;
        const pack_mask k = pack_masks(q, bl, 64 * h2 + 4 * h);
        const float lown = lse_s[bl];
        const float* lc = lse_s + 64 * h2 + 4 * h;
        float* qrow = qs + bl * PLD + 4 * h;
#pragma unroll
        for (int mi = 0; mi < 2; ++mi)
#pragma unroll
          for (int r4 = 0; r4 < 4; ++r4) {
            float e[4];
#pragma unroll
            for (int kk = 0; kk < 4; ++kk) {
              const int jl = 32 * mi + 8 * r4 + kk;
              const float v = acc[mi][ni][4 * r4 + kk];
              const bool ok = jl >= k.lo && jl < k.hi && jl != k.own;
              const float qv = expf(v - lown) + expf(v - lc[jl]);
              e[kk] = ok ? qv : 0.f;
            }
            *reinterpret_cast<float4*>(qrow + 32 * mi + 8 * r4) = make_float4(e[0], e[1], e[2], e[3]);
            __builtin_amdgcn_sched_barrier(0);
          }
      }
    }
    float4 zl[8];
#pragma unroll
    for (int it = 0; it < 8; ++it) {
      const int u = it * 4 + w, jb = u & 3, cb = u >> 2;
      zl[it] = pack_ld4(src, q, PH * h2 + 16 * jb + (lane >> 2), cs0 + 16 * cb + 4 * (lane & 3));
    }
#pragma unroll
    for (int it = 0; it < 8; ++it) {
      const int u = it * 4 + w, jb = u & 3, cb = u >> 2;
      float* d = zt + (16 * cb + 4 * (lane & 3)) * PLD + 16 * jb + (lane >> 2);
      d[0] = zl[it].x, d[PLD] = zl[it].y, d[2 * PLD] = zl[it].z, d[3 * PLD] = zl[it].w;
    }
    __syncthreads();
    pt::mfma_dots<PLD, PLD, PH / 2>(zt, qs, tid, dacc);
    __builtin_amdgcn_sched_barrier(0);
    pt::mfma_dots<PLD, PLD, PH / 2>(zt + PH / 2, qs + PH / 2, tid, dacc);
  }

#pragma unroll
  for (int ni = 0; ni < 2; ++ni) {
    const int bl = 64 * (w & 1) + 32 * ni + jr, p = bl >> q.slot_log2, r = bl & (S - 1);
    if (p >= src.pv || r >= 2 * q.n) continue;
    const bool first = r < q.n;
    const int64_t row = (int64_t)(g0 + p) * q.gs + (int64_t)(first ? r : r - q.n) * q.rs;
    float* dz = (first ? dz1 : dz2) + row;
    const float* zp = (first ? z2 : z1) + row;
#pragma unroll
    for (int mi = 0; mi < 2; ++mi)
#pragma unroll
      for (int r4 = 0; r4 < 4; ++r4) {
        const int col = cs0 + 64 * (w >> 1) + 32 * mi + 8 * r4 + 4 * h;
        if (col >= q.c) continue;
        const float4 pv = *reinterpret_cast<const float4*>(zp + col);
        float4 v;
        v.x = scale * fmaf(-2.f, pv.x, dacc[mi][ni][4 * r4 + 0]);
        v.y = scale * fmaf(-2.f, pv.y, dacc[mi][ni][4 * r4 + 1]);
        v.z = scale * fmaf(-2.f, pv.z, dacc[mi][ni][4 * r4 + 2]);
        v.w = scale * fmaf(-2.f, pv.w, dacc[mi][ni][4 * r4 + 3]);
        if (accumulate) {
          const float4 old = *reinterpret_cast<const float4*>(dz + col);
          v.x = __fadd_rn(old.x, v.x), v.y = __fadd_rn(old.y, v.y), v.z = __fadd_rn(old.z, v.z),
          v.w = __fadd_rn(old.w, v.w);
        }
        *reinterpret_cast<float4*>(dz + col) = v;
      }
  }
}

// ------------------------------------------------------------------------------------------------ max-pool over time
// torch's max_pool1d: the later step wins only when it is greater (or a NaN)
__device__ __forceinline__ bool second_wins(float a, float b) { return b > a || b != b; }

__global__ __launch_bounds__(256) void pool2_fwd_kernel(const float* __restrict__ in, int64_t quads, int T, int To,
                                                        int c4, float* __restrict__ out) {
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < quads; i += (int64_t)gridDim.x * 256) {
    const int64_t row = i / c4;       // b * To + t
    const int64_t src = ((row / To) * T + 2 * (row % To)) * c4 + i % c4;
    const float4 a = reinterpret_cast<const float4*>(in)[src], b = reinterpret_cast<const float4*>(in)[src + c4];
    reinterpret_cast<float4*>(out)[i] = make_float4(second_wins(a.x, b.x) ? b.x : a.x, second_wins(a.y, b.y) ? b.y : a.y,
                                                    second_wins(a.z, b.z) ? b.z : a.z, second_wins(a.w, b.w) ? b.w : a.w);
  }
}

__global__ __launch_bounds__(256) void pool2_bwd_kernel(const float* __restrict__ in, const float* __restrict__ dout,
                                                        int64_t quads, int T, int To, int c4, float* din) {
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < quads; i += (int64_t)gridDim.x * 256) {
    const int64_t row = i / c4;
    const int64_t src = ((row / To) * T + 2 * (row % To)) * c4 + i % c4;
    const float4 a = reinterpret_cast<const float4*>(in)[src], b = reinterpret_cast<const float4*>(in)[src + c4];
    const float4 gd = reinterpret_cast<const float4*>(dout)[i];
    float4 da = reinterpret_cast<float4*>(din)[src], db = reinterpret_cast<float4*>(din)[src + c4];
    const bool sx = second_wins(a.x, b.x), sy = second_wins(a.y, b.y), sz = second_wins(a.z, b.z),
               sw = second_wins(a.w, b.w);
    da.x += sx ? 0.f : gd.x, db.x += sx ? gd.x : 0.f;
    da.y += sy ? 0.f : gd.y, db.y += sy ? gd.y : 0.f;
    da.z += sz ? 0.f : gd.z, db.z += sz ? gd.z : 0.f;
    da.w += sw ? 0.f : gd.w, db.w += sw ? gd.w : 0.f;
    reinterpret_cast<float4*>(din)[src] = da;
    reinterpret_cast<float4*>(din)[src + c4] = db;
  }
}

int nce_check(const char* who, const void* z1, const void* z2, int groups, int n, int c, int64_t gs, int64_t rs) {
  AW_REQUIRE(groups >= 0 && groups <= AW_NCE_MAX_GROUPS, "%s: groups = %d outside 0..%d", who, groups,
             AW_NCE_MAX_GROUPS);
  AW_REQUIRE(n >= 1 && 2 * (int64_t)n <= AW_NCE_MAX_ROWS, "%s: n = %d, need 1 <= n and 2 n <= %d", who, n,
             AW_NCE_MAX_ROWS);
  AW_REQUIRE(c % 16 == 0 && c >= 16 && c <= AW_NCE_MAX_WIDTH, "%s: c = %d is not a multiple of 16 in 16..%d", who, c,
             AW_NCE_MAX_WIDTH);
  AW_REQUIRE(rs >= c && rs < (1 << 22) && (rs & 3) == 0,
             "%s: row stride %lld must be a multiple of 4 in c = %d .. 2^22 - 1", who, (long long)rs, c);
  AW_REQUIRE(gs >= 0 && (gs & 3) == 0, "%s: group stride %lld must be a non-negative multiple of 4", who,
             (long long)gs);
  if (groups == 0) return AW_OK;
  AW_REQUIRE(z1 && z2 && ((uintptr_t)z1 & 15) == 0 && ((uintptr_t)z2 & 15) == 0,
             "%s: z1 and z2 must be 16-byte aligned and not NULL", who);
  return AW_OK;
}

// the slot of a packed group: 32, 64 or 128 tile rows
int slot_log2(int n) { return 2 * n <= 32 ? 5 : 2 * n <= 64 ? 6 : 7; }

int pool_check(const char* who, int batch, int T, int c) {
  AW_REQUIRE(batch >= 0 && batch <= AW_TS_MAX_BATCH, "%s: batch = %d outside 0..%d", who, batch, AW_TS_MAX_BATCH);
  AW_REQUIRE(T >= 2 && T <= AW_TS_MAX_T, "%s: T = %d outside 2..%d", who, T, AW_TS_MAX_T);
  AW_REQUIRE(c % 16 == 0 && c >= 16 && c <= AW_NCE_MAX_WIDTH, "%s: c = %d is not a multiple of 16 in 16..%d", who, c,
             AW_NCE_MAX_WIDTH);
  return AW_OK;
}

}  // namespace

extern "C" int aw_nce_describe(int* tile_rows, int* chunk_c, int* slab_c) {
  if (tile_rows) *tile_rows = NT;
  if (chunk_c) *chunk_c = pt::TD;
  if (slab_c) *slab_c = SLAB;
  return AW_OK;
}

extern "C" int aw_nce_rows_fwd(const float* z1, const float* z2, int groups, int n, int c, int64_t group_stride,
                               int64_t row_stride, float* lse, float* row_loss, void* stream) {
  const int st = nce_check("aw_nce_rows_fwd", z1, z2, groups, n, c, group_stride, row_stride);
  if (st != AW_OK) return st;
  if (groups == 0) return AW_OK;
  AW_REQUIRE(lse && row_loss, "aw_nce_rows_fwd: lse and row_loss must not be NULL");
  hipStream_t hs = reinterpret_cast<hipStream_t>(stream);
  if (2 * n <= NT) {   // whole groups packed into one tile
    const nce_pack pk{n, c, groups, slot_log2(n), group_stride, row_stride};
    const int per = NT >> pk.slot_log2;
    hipLaunchKernelGGL(nce_fwd_packed_kernel, dim3((groups + per - 1) / per), dim3(NTHREADS), 0, hs, z1, z2, pk, lse,
                       row_loss);
    return aw::check_launch("aw_nce_rows_fwd");
  }
  const nce_geom q{n, c, (n + NT - 1) / NT, group_stride, row_stride};
  hipLaunchKernelGGL(nce_fwd_kernel, dim3(2 * q.nt, groups), dim3(NTHREADS), 0, reinterpret_cast<hipStream_t>(stream),
                     z1, z2, q, lse, row_loss);
  return aw::check_launch("aw_nce_rows_fwd");
}

extern "C" int aw_nce_rows_bwd(const float* z1, const float* z2, int groups, int n, int c, int64_t group_stride,
                               int64_t row_stride, const float* lse, float scale, float* dz1, float* dz2,
                               int accumulate, void* stream) {
  const int st = nce_check("aw_nce_rows_bwd", z1, z2, groups, n, c, group_stride, row_stride);
  if (st != AW_OK) return st;
  if (groups == 0) return AW_OK;
  AW_REQUIRE(lse && dz1 && dz2 && ((uintptr_t)dz1 & 15) == 0 && ((uintptr_t)dz2 & 15) == 0,
             "aw_nce_rows_bwd: lse, dz1 and dz2 must not be NULL, dz1 and dz2 16-byte aligned");
  hipStream_t hs = reinterpret_cast<hipStream_t>(stream);
  if (2 * n <= NT) {
    const nce_pack pk{n, c, groups, slot_log2(n), group_stride, row_stride};
    const int per = NT >> pk.slot_log2;
    hipLaunchKernelGGL(nce_bwd_packed_kernel, dim3((groups + per - 1) / per, (c + SLAB - 1) / SLAB), dim3(NTHREADS), 0,
                       hs, z1, z2, pk, lse, scale, dz1, dz2, accumulate);
    return aw::check_launch("aw_nce_rows_bwd");
  }
  const nce_geom q{n, c, (n + NT - 1) / NT, group_stride, row_stride};
  hipLaunchKernelGGL(nce_bwd_kernel, dim3(2 * q.nt, groups, (c + SLAB - 1) / SLAB), dim3(NTHREADS), 0,
                     reinterpret_cast<hipStream_t>(stream), z1, z2, q, lse, scale, dz1, dz2, accumulate);
  return aw::check_launch("aw_nce_rows_bwd");
}

extern "C" int aw_ts_pool2_fwd(const float* in, int batch, int T, int c, float* out, void* stream) {
  const int st = pool_check("aw_ts_pool2_fwd", batch, T, c);
  if (st != AW_OK) return st;
  if (batch == 0) return AW_OK;
  AW_REQUIRE(in && out && ((uintptr_t)in & 15) == 0 && ((uintptr_t)out & 15) == 0,
             "aw_ts_pool2_fwd: in and out must be 16-byte aligned and not NULL");
  const int To = T / 2, c4 = c / 4;
  const int64_t quads = (int64_t)batch * To * c4;
  const int64_t blocks = (quads + 255) / 256;
  hipLaunchKernelGGL(pool2_fwd_kernel, dim3((unsigned)(blocks < 65535 ? blocks : 65535)), dim3(256), 0,
                     reinterpret_cast<hipStream_t>(stream), in, quads, T, To, c4, out);
  return aw::check_launch("aw_ts_pool2_fwd");
}

extern "C" int aw_ts_pool2_bwd(const float* in, const float* dout, int batch, int T, int c, float* din,
                               void* stream) {
  const int st = pool_check("aw_ts_pool2_bwd", batch, T, c);
  if (st != AW_OK) return st;
  if (batch == 0) return AW_OK;
  AW_REQUIRE(in && dout && din && ((uintptr_t)in & 15) == 0 && ((uintptr_t)dout & 15) == 0 &&
                 ((uintptr_t)din & 15) == 0,
             "aw_ts_pool2_bwd: in, dout and din must be 16-byte aligned and not NULL");
  const int To = T / 2, c4 = c / 4;
  const int64_t quads = (int64_t)batch * To * c4;
  const int64_t blocks = (quads + 255) / 256;
  hipLaunchKernelGGL(pool2_bwd_kernel, dim3((unsigned)(blocks < 65535 ? blocks : 65535)), dim3(256), 0,
                     reinterpret_cast<hipStream_t>(stream), in, dout, quads, T, To, c4, din);
  return aw::check_launch("aw_ts_pool2_bwd");
}
