// The 128 x 128 all-pairs tile on the f32-input MFMA: every squared distance between TB rows of b and TA rows of a,
// shared by the k-NN sweep (knn.hip: b = the queries, a = the database) and the RBF Gram matrix (svm.hip).  The
// masked loaders also serve logreg.hip.
//
// A 256-thread workgroup streams both operands through LDS in TD = 32-dim chunks: range-checked buffer loads ->
// registers (fetch) -> LDS (stage_put), the next chunk's loads in flight under the current chunk's MFMAs (dots), two
// LDS stages, one barrier per chunk.  A kernel's chunk loop is
//     stage_put(sb, pre, tid);  __syncthreads();  <fetch the next chunk, if any>;  dots(sb, tid, acc, nrm);
// alternating sb between the two stages: the stage written next was last read before this barrier.  Which chunk comes
// next (the same tile's, or the first of the next tile) is the caller's business.
//
// The dots run on v_mfma_f32_32x32x2_f32 (bit for bit an fmaf chain, cdna_hip_programming.md 'FP32-input MFMA') with
// the rows of a as the A operand.  Wave w owns the 64 x 64 block (a half w >> 1) x (b half w & 1) as 2 x 2 tiles of
// 32 x 32, so a lane ends with ONE b row per tile column and 16 a rows in its accumulator registers: register r of
// acc[mi][ni] is a row 64 (w >> 1) + 32 mi + 8 (r >> 2) + 4 h + (r & 3) against b row 64 (w & 1) + 32 ni + jr
// (h = lane >> 5, jr = lane & 31).  The squared norms accumulate beside the MFMAs as in-order fmaf chains, one staged
// row per thread.
//
// One (a row, b row) distance is always accumulated over all of D by one wave in one fixed order (chunks ascending; in
// a chunk, MFMA step 4 g + t multiplies dims 8 g + t (lanes 0..31) and 8 g + 4 + t (lanes 32..63)), and every product
// and the sum of the norms commute: its bits depend on neither the grid nor the run nor on which operand a row came
// in as.
#pragma once
#include "common.h"

#include <type_traits>

namespace aw::pt {

constexpr int TB = 128;             // rows of b per workgroup (the MFMA's B operand)
constexpr int TA = 128;             // rows of a per tile (the MFMA's A operand)
constexpr int TD = 32;              // dims per chunk
constexpr int LD = TD + 4;          // staged row stride (floats): 16 rows of a ds_read_b128 cover all 64 banks
constexpr int THREADS = 256;
constexpr int OT = TB + 8;          // result tile row stride: the two lane halves (4 rows apart) land 32 banks apart
constexpr int STAGE = (TB + TA) * LD;                 // floats per stage: b rows 0..127, then a rows
constexpr int F4 = (TB + TA) * (TD / 4) / THREADS;    // float4 per thread per chunk
static_assert(TA * OT <= 2 * STAGE, "the result tile overlays the two stages");
static_assert(TB + TA == THREADS, "one staged row per thread for the norms");

typedef __attribute__((ext_vector_type(16))) float f32x16;
typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));

// Operand loads go through raw buffer descriptors (one per tile of rows: base = the tile's first row, range = up to the
// last value of its last row): an offset past the range returns zeros, so a masked element -- a row past the end, dims
// past D -- is a load at BAD_OFF instead of a branch or a select after the load.  The loads are straight-line code
// with nothing consuming them until the next chunk's LDS store, so they stay in flight under the MFMAs (with guarded
// global loads the compiler waited for each before the matrix work began: 45 TFLOP/s instead of the figures in
// DESIGN.md section 4.15).  Neither rows past the end nor the row padding are ever read.
constexpr uint32_t BAD_OFF = 0x80000000u;   // >= every range (a tile of rows spans < 2^31 bytes: ld < 2^22)

__device__ __forceinline__ __amdgpu_buffer_rsrc_t rsrc(const float* base, int64_t row0, int64_t nrows, int64_t ld,
                                                       int D, int tile_rows, int& rows) {
  const int64_t left = nrows - row0;
  rows = (int)(left < tile_rows ? left : tile_rows);
  const uint32_t bytes = rows > 0 ? (uint32_t)(((int64_t)(rows - 1) * ld + D) * 4) : 0u;
  return __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(base + row0 * ld), (short)0, (int)bytes, 0x00020000);
}

__device__ __forceinline__ float ld1(__amdgpu_buffer_rsrc_t r, bool ok, uint32_t off) {
  return __uint_as_float(__builtin_amdgcn_raw_buffer_load_b32(r, ok ? off : BAD_OFF, 0, 0));
}

// dims d0 .. d0 + 3 of tile row `row` (zeros for row >= rows and dims >= D).  VEC: base and stride are 16-byte
// aligned and the caller knows that no quad of this chunk straddles D, so a quad is one 16-B load; !VEC: four 4-byte
// loads, each masked on its own.
template <bool VEC>
__device__ __forceinline__ float4 ld4(__amdgpu_buffer_rsrc_t r, int row, int rows, uint32_t ld_bytes, int d0, int D) {
  const bool rok = row < rows;
  const uint32_t off = (uint32_t)row * ld_bytes + 4u * (uint32_t)d0;
  if constexpr (VEC) {
    const u32x4 u = __builtin_amdgcn_raw_buffer_load_b128(r, rok && d0 + 4 <= D ? off : BAD_OFF, 0, 0);
    return make_float4(__uint_as_float(u.x), __uint_as_float(u.y), __uint_as_float(u.z), __uint_as_float(u.w));
  } else {
    auto one = [&](int i) { return ld1(r, rok && d0 + i < D, off + 4u * i); };
    return make_float4(one(0), one(1), one(2), one(3));
  }
}

// one tile of rows of one operand
struct Operand {
  __amdgpu_buffer_rsrc_t rsrc;
  int rows;            // of the tile that exist
  uint32_t ld_bytes;
};
__device__ __forceinline__ Operand operand(const float* base, int64_t row0, int64_t nrows, int64_t ld, int D,
                                           int tile_rows) {
  Operand o;
  o.rsrc = rsrc(base, row0, nrows, ld, D, tile_rows, o.rows);
  o.ld_bytes = (uint32_t)ld * 4u;
  return o;
}

// Chunk ch of both tiles into registers: float4 i of thread tid is quad (tid & 7) of staged row (tid >> 3) + 32 i, rows
// of b for i < F4 / 2, rows of a after (known at compile time: no divergence between the two operands).  Only the
// last chunk of a D % 4 != 0 has a quad that straddles D: it alone takes the 4-byte loads (a uniform branch between
// two straight-line blocks).
template <bool BVEC, bool AVEC>
__device__ __forceinline__ void fetch(float4 (&pre)[F4], const Operand& b, const Operand& a, int ch, int D, int tid) {
  auto as = [&](auto bv, auto av) {
    const int d0 = ch * TD + (tid & 7) * 4;
#pragma unroll
    for (int i = 0; i < F4; ++i) {
      const int row = (tid >> 3) + 32 * i;
      if (i < F4 / 2)
        pre[i] = ld4<decltype(bv)::value>(b.rsrc, row, b.rows, b.ld_bytes, d0, D);
      else
        pre[i] = ld4<decltype(av)::value>(a.rsrc, row - TB, a.rows, a.ld_bytes, d0, D);
    }
  };
  if ((D & 3) != 0 && ch == (D + TD - 1) / TD - 1)
    as(std::false_type{}, std::false_type{});
  else
    as(std::integral_constant<bool, BVEC>{}, std::integral_constant<bool, AVEC>{});
}

// the fetched chunk to stage sb; the caller's barrier follows
__device__ __forceinline__ void stage_put(float* sb, const float4 (&pre)[F4], int tid) {
#pragma unroll
  for (int i = 0; i < F4; ++i) {
    const int f = tid + i * THREADS;
    *reinterpret_cast<float4*>(sb + (f >> 3) * LD + (f & 7) * 4) = pre[i];
  }
}

__device__ __forceinline__ void zero(f32x16 (&acc)[2][2]) {
#pragma unroll
  for (int mi = 0; mi < 2; ++mi)
#pragma unroll
    for (int ni = 0; ni < 2; ++ni)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[mi][ni][r] = 0.f;
}

// One staged chunk: nrm, the squared norm of staged row `tid`, goes on by TD terms and acc[a tile mi][b tile ni] by
// the chunk's 64 MFMAs.
__device__ __forceinline__ void dots(const float* sb, int tid, f32x16 (&acc)[2][2], float& nrm) {
  const int lane = tid & 63, w = tid >> 6, h = lane >> 5, jr = lane & 31;
#pragma unroll
  for (int c = 0; c < TD / 4; ++c) {
    const float4 v = *reinterpret_cast<const float4*>(sb + tid * LD + 4 * c);
    nrm = __builtin_fmaf(v.x, v.x, nrm);
    nrm = __builtin_fmaf(v.y, v.y, nrm);
    nrm = __builtin_fmaf(v.z, v.z, nrm);
    nrm = __builtin_fmaf(v.w, v.w, nrm);
  }
  const float* sa = sb + (TB + 64 * (w >> 1) + jr) * LD + 4 * h;   // A: rows of a
  const float* sq = sb + (64 * (w & 1) + jr) * LD + 4 * h;         // B: rows of b
#pragma unroll
  for (int g = 0; g < TD / 8; ++g) {
    float4 a4[2], b4[2];
#pragma unroll
    for (int t = 0; t < 2; ++t) {
      a4[t] = *reinterpret_cast<const float4*>(sa + 32 * t * LD + 8 * g);
      b4[t] = *reinterpret_cast<const float4*>(sq + 32 * t * LD + 8 * g);
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
}

// The MFMAs of `dots` alone, on any two staged row sets: acc[mi][ni] += rows 64 (w >> 1) + 32 mi + .. of sa (row
// stride LDA floats) against rows 64 (w & 1) + 32 ni + .. of sq (row stride LDQ) over K dims, in the order of `dots`
// (step 4 g + t multiplies dims 8 g + t and 8 g + 4 + t).  mfma_dots<LD, LD, TD>(sb + TB * LD, sb, ..) is `dots`
// without the norms (ts2vec_loss.hip, whose second GEMM also runs on it with the pair index as the dims).
template <int LDA, int LDQ, int K>
__device__ __forceinline__ void mfma_dots(const float* sa_rows, const float* sq_rows, int tid, f32x16 (&acc)[2][2]) {
  static_assert(K % 8 == 0 && LDA % 4 == 0 && LDQ % 4 == 0, "16-byte LDS reads");
  const int lane = tid & 63, w = tid >> 6, h = lane >> 5, jr = lane & 31;
  const float* sa = sa_rows + (64 * (w >> 1) + jr) * LDA + 4 * h;
  const float* sq = sq_rows + (64 * (w & 1) + jr) * LDQ + 4 * h;
#pragma unroll
  for (int g = 0; g < K / 8; ++g) {
    float4 a4[2], b4[2];
#pragma unroll
    for (int t = 0; t < 2; ++t) {
      a4[t] = *reinterpret_cast<const float4*>(sa + 32 * t * LDA + 8 * g);
      b4[t] = *reinterpret_cast<const float4*>(sq + 32 * t * LDQ + 8 * g);
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
}

// The finished tile to LDS: out[al * OT + bl] = f(fma(-2, dot, fl(|b|^2 + |a|^2))) for a row al against b row bl.
// 2 dot is exact, so the fma's one rounding is that of fl(fl(|b|^2 + |a|^2) - 2 dot).  nrm_s has TB + TA floats; out
// may overlay the stages: the first barrier publishes the norms and ends every wave's reading of the stages, the
// second publishes the tile.
template <class F>
__device__ __forceinline__ void dist_tile(float* out, float* nrm_s, float nrm, int tid, const f32x16 (&acc)[2][2],
                                          F f) {
  const int lane = tid & 63, w = tid >> 6, h = lane >> 5, jr = lane & 31;
  nrm_s[tid] = nrm;
  __syncthreads();
#pragma unroll
  for (int ni = 0; ni < 2; ++ni) {
    const int bl = 64 * (w & 1) + 32 * ni + jr;
    const float bb = nrm_s[bl];
#pragma unroll
    for (int mi = 0; mi < 2; ++mi)
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int al = 64 * (w >> 1) + 32 * mi + 8 * (r >> 2) + 4 * h + (r & 3);
        const float s = __fadd_rn(bb, nrm_s[TB + al]);
        out[al * OT + bl] = f(__builtin_fmaf(-2.f, acc[mi][ni][r], s));
      }
  }
  __syncthreads();
}

}  // namespace aw::pt
