// Batched binary logistic regression over one feature matrix (aw_logreg_forward / aw_logreg_grad,
// include/arcweld_amd.h): the linear latent-space probe's hot path (arcweld/retrieve.py).  P <= 32 independent
// problems -- a (positive class, regularisation strength) pair each -- share every read of X; the skinny products run
// on the f32-input MFMA (v_mfma_f32_32x32x2_f32: bit for bit an fmaf chain, cdna_hip_programming.md 'FP32-input
// MFMA'), whose 32 columns are the problems.  f32 operands, f64 sums.
//
//   logreg_fwd_kernel    grid (row tiles).  A 256-thread workgroup owns LM = 128 rows; wave w the 32 x 32 block
//                        (rows 32 w ..) x (problems).  X and W stream through LDS in LK = 32-dim chunks the way
//                        pair_tile.h stages its operands (its range-checked buffer loads -> registers -> LDS, the next
//                        chunk's loads in flight under the current chunk's MFMAs, two stages, one barrier per chunk);
//                        W is staged transposed ([problem][dim]) so that both operands are read as float4 along the
//                        dims.
//                        Epilogue: z = acc + b; with labels r = sigma(z) - t, and per lane the f64 sums of the loss and
//                        of r over its 16 rows (ascending), the two lane halves added, the four waves added in wave
//                        order: one (loss, gb) partial per workgroup and problem.
//   logreg_sum_kernel    one workgroup per (problem, loss | gb): thread t adds partials t, t + 256, ... in ascending
//                        order, then a fixed tree over the threads.
//   logreg_grad_kernel   grid (dim tiles of GD = 512) x (row splits).  No LDS: the reduction runs over the rows, so
//                        X's rows are the MFMA's k index and a lane's A operands are four consecutive dims of one row:
//                        one 16-byte buffer load (a wave reads 2 x 512 contiguous bytes per load; four guarded 4-byte
//                        loads when base, stride or d are not 16-byte multiples) feeds four MFMAs, accumulator m
//                        holding the dims 4 j + m of the wave's 128; the B operand r[row][problem of the lane] is a
//                        4-byte load.  A wave walks its split's rows in chunks of GR = 16, the next chunk's 16 loads in
//                        flight under the current chunk's 32 MFMAs.  The f32 partial of a split goes to the workspace.
//   logreg_gsum_kernel   g[dim][problem] = the splits' partials added in f64 in split order.
//
// Every sum has one fixed order for given inputs and a given split count: no float atomics anywhere.
#include "common.h"
#include "pair_tile.h"

#include <math.h>

#include <type_traits>

namespace {

constexpr int LM = 128;             // rows per forward workgroup
constexpr int LK = 32;              // dims per forward chunk
constexpr int LLD = LK + 4;         // staged row stride (floats): 16 rows of a ds_read_b128 cover all 64 banks
constexpr int LP = AW_LOGREG_MAX_P; // problems = the MFMA's 32 columns
constexpr int LTHREADS = 256;
constexpr int L_STAGE = (LM + LP) * LLD;              // floats per stage: x rows 0..127, then W^T rows (problems)
constexpr int L_XF4 = LM * (LK / 4) / LTHREADS;       // X float4 per thread per chunk
constexpr int GD = 512;             // dims per gradient workgroup (128 per wave)
constexpr int GR = 16;              // rows per gradient chunk
static_assert(LP == 32, "the problems are the 32 columns of v_mfma_f32_32x32x2_f32");
static_assert(LP * (LK / 4) == LTHREADS, "one W quad per thread per chunk");
static_assert(2 * L_STAGE * 4 <= 80 * 1024, "forward LDS, two workgroups per CU");

namespace pt = aw::pt;
using pt::f32x16;

// Raw buffer descriptors and the masked loads of pair_tile.h: a masked element -- a row past the end, a dim past d, a
// problem past p -- reads zeros.  Neither the row padding nor rows past the end are ever read.  A descriptor spans at
// most 128 rows of stride < 2^22 floats: < 2^31 bytes.
__device__ __forceinline__ __amdgpu_buffer_rsrc_t lr_rsrc(const float* base, int64_t floats) {
  return __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(base), (short)0, (int)(uint32_t)(floats * 4), 0x00020000);
}

template <bool XVEC>
__global__ __launch_bounds__(LTHREADS, 2) void logreg_fwd_kernel(const float* __restrict__ x, int64_t n, int64_t ldx,
                                                                 int d, const float* __restrict__ w,
                                                                 const float* __restrict__ b, int p,
                                                                 const int* __restrict__ y,
                                                                 const int* __restrict__ cls, float* __restrict__ z,
                                                                 float* __restrict__ r, double* __restrict__ part) {
  __shared__ __attribute__((aligned(16))) float stage[2 * L_STAGE];
  __shared__ double red[2][LTHREADS / 64][LP];
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, h = lane >> 5, jr = lane & 31;
  const int64_t row0 = (int64_t)blockIdx.x * LM;
  const int nch = (d + LK - 1) / LK;
  const int64_t left = n - row0;
  const int rows = (int)(left < LM ? left : LM);
  const __amdgpu_buffer_rsrc_t x_rsrc = lr_rsrc(x + row0 * ldx, (int64_t)(rows - 1) * ldx + d);
  const __amdgpu_buffer_rsrc_t w_rsrc = lr_rsrc(w, (int64_t)d * p);
  const uint32_t ldx_b = (uint32_t)ldx * 4u;

  float4 pre[L_XF4 + 1];
  // float4 i < L_XF4 of thread tid is quad (tid & 7) of x row (tid >> 3) + 32 i; the last one is dims 4 (tid >> 5) ..
  // + 3 of problem tid & 31 (a wave reads 128 contiguous bytes of two rows of W per load)
  auto fetch_as = [&](int ch, auto xv) {
    const int d0 = ch * LK + (tid & 7) * 4;
#pragma unroll
    for (int i = 0; i < L_XF4; ++i)
      pre[i] = pt::ld4<decltype(xv)::value>(x_rsrc, (tid >> 3) + 32 * i, rows, ldx_b, d0, d);
    const int col = tid & 31, k0 = ch * LK + 4 * (tid >> 5);
    const bool cok = col < p;
    auto wl = [&](int j) { return pt::ld1(w_rsrc, cok && k0 + j < d, 4u * ((uint32_t)(k0 + j) * (uint32_t)p + col)); };
    pre[L_XF4] = make_float4(wl(0), wl(1), wl(2), wl(3));
  };
  // only the last chunk of a d % 4 != 0 has a quad that straddles d: it alone takes the 4-byte loads
  auto fetch = [&](int ch) {
    if ((d & 3) != 0 && ch == nch - 1)
      fetch_as(ch, std::false_type{});
    else
      fetch_as(ch, std::integral_constant<bool, XVEC>{});
  };

  f32x16 acc;
#pragma unroll
  for (int i = 0; i < 16; ++i) acc[i] = 0.f;
  fetch(0);
  int buf = 0;
  for (int ch = 0; ch < nch; ++ch) {
    float* sb = stage + buf * L_STAGE;
#pragma unroll
    for (int i = 0; i < L_XF4; ++i) {
      const int f = tid + i * LTHREADS;
      *reinterpret_cast<float4*>(sb + (f >> 3) * LLD + (f & 7) * 4) = pre[i];
    }
    *reinterpret_cast<float4*>(sb + (LM + (tid & 31)) * LLD + 4 * (tid >> 5)) = pre[L_XF4];
    __syncthreads();
    // the next chunk's loads fly under this chunk's MFMAs (the stage written next was last read before this barrier)
    if (ch + 1 < nch) fetch(ch + 1);
    const float* sa = sb + (32 * wv + jr) * LLD + 4 * h;   // A: x rows
    const float* sw = sb + (LM + jr) * LLD + 4 * h;        // B: problems
#pragma unroll
    for (int g = 0; g < LK / 8; ++g) {
      const float4 a4 = *reinterpret_cast<const float4*>(sa + 8 * g);
      const float4 b4 = *reinterpret_cast<const float4*>(sw + 8 * g);
      acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a4.x, b4.x, acc, 0, 0, 0);
      acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a4.y, b4.y, acc, 0, 0, 0);
      acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a4.z, b4.z, acc, 0, 0, 0);
      acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a4.w, b4.w, acc, 0, 0, 0);
    }
    buf ^= 1;
  }

  // ---- register i of acc is row 32 wv + 8 (i >> 2) + 4 h + (i & 3) against problem jr
  const bool cok = jr < p;
  const float bias = cok ? b[jr] : 0.f;
  const bool labelled = cls != nullptr;
  const int c = (labelled && cok) ? cls[jr] : 0;
  double loss = 0.0, gb = 0.0;
#pragma unroll
  for (int i = 0; i < 16; ++i) {
    const int rl = 32 * wv + 8 * (i >> 2) + 4 * h + (i & 3);
    if (rl < rows && cok) {
      const int64_t o = (row0 + rl) * p + jr;
      const float zz = __fadd_rn(acc[i], bias);
      z[o] = zz;
      if (labelled) {
        const int yi = y[row0 + rl];
        const float e = expf(-fabsf(zz));                                   // in (0, 1]
        const float sig = __fdiv_rn(zz >= 0.f ? 1.f : e, __fadd_rn(1.f, e));
        const float sp = __fadd_rn(fmaxf(zz, 0.f), log1pf(e));              // the stable softplus
        const bool t = yi == c;
        const float rr = yi >= 0 ? __fsub_rn(sig, t ? 1.f : 0.f) : 0.f;
        r[o] = rr;
        if (yi >= 0) {
          loss += (double)sp - (t ? (double)zz : 0.0);
          gb += (double)rr;
        }
      }
    }
  }
  if (labelled) {
    loss += __shfl_xor(loss, 32, 64);   // a + b on both halves: the same bits
    gb += __shfl_xor(gb, 32, 64);
    if (h == 0) {
      red[0][wv][jr] = loss;
      red[1][wv][jr] = gb;
    }
    __syncthreads();
    if (tid < 2 * LP) {
      const int which = tid >> 5, col = tid & 31;
      double s = red[which][0][col];
      for (int k = 1; k < LTHREADS / 64; ++k) s += red[which][k][col];
      part[((int64_t)blockIdx.x * 2 + which) * LP + col] = s;
    }
  }
}

// out[which][col] = sum over the workgroups' partials: thread t takes blocks t, t + 256, ... in ascending order, then
// a fixed tree.  nblocks == 0 writes zeros.
__global__ __launch_bounds__(LTHREADS) void logreg_sum_kernel(const double* __restrict__ part, int64_t nblocks,
                                                              double* __restrict__ loss, double* __restrict__ gb) {
  __shared__ double s[LTHREADS];
  const int col = blockIdx.x, which = blockIdx.y, tid = threadIdx.x;
  double v = 0.0;
  for (int64_t k = tid; k < nblocks; k += LTHREADS) v += part[(k * 2 + which) * LP + col];
  s[tid] = v;
  __syncthreads();
  for (int o = LTHREADS / 2; o > 0; o >>= 1) {
    if (tid < o) s[tid] += s[tid + o];
    __syncthreads();
  }
  if (tid == 0) (which ? gb : loss)[col] = s[0];
}

// XVEC: base and stride are 16-byte aligned and d % 4 == 0, so a lane's four dims are one 16-B load; !XVEC: four 4-byte
// loads, each masked on its own.
template <bool XVEC>
__global__ __launch_bounds__(LTHREADS, 2) void logreg_grad_kernel(const float* __restrict__ x, int64_t n, int64_t ldx,
                                                                  int d, const float* __restrict__ r, int p,
                                                                  int64_t rows_per_split, float* __restrict__ ws) {
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, h = lane >> 5, jr = lane & 31;
  const int dl = blockIdx.x * GD + (GD / 4) * wv + 4 * jr;   // this lane's first dim
  const int64_t i0 = (int64_t)blockIdx.y * rows_per_split;
  const int64_t i1 = i0 + rows_per_split < n ? i0 + rows_per_split : n;
  const uint32_t ldx_b = (uint32_t)ldx * 4u;
  const bool cok = jr < p;

  float4 xa[GR / 2];
  float rb[GR / 2];
  // MFMA step s of a chunk multiplies rows 2 s (lanes 0..31) and 2 s + 1 (lanes 32..63) of the chunk
  auto fetch = [&](int64_t i) {
    const int64_t left = i1 - i;
    const int rows = (int)(left < GR ? left : GR);
    const __amdgpu_buffer_rsrc_t x_rsrc = lr_rsrc(x + i * ldx, (int64_t)(rows - 1) * ldx + d);
    const __amdgpu_buffer_rsrc_t r_rsrc = lr_rsrc(r + i * p, (int64_t)rows * p);
#pragma unroll
    for (int s = 0; s < GR / 2; ++s) {
      const int row = 2 * s + h;
      xa[s] = pt::ld4<XVEC>(x_rsrc, row, rows, ldx_b, dl, d);
      rb[s] = pt::ld1(r_rsrc, row < rows && cok, 4u * ((uint32_t)row * (uint32_t)p + jr));
    }
  };

  f32x16 acc[4];   // acc[m]: the dims 4 j + m of the wave's 128, j = the MFMA's row index
#pragma unroll
  for (int m = 0; m < 4; ++m)
#pragma unroll
    for (int i = 0; i < 16; ++i) acc[m][i] = 0.f;
  if (i0 < i1) fetch(i0);
  for (int64_t i = i0; i < i1; i += GR) {
    float4 ca[GR / 2];
    float cb[GR / 2];
#pragma unroll
    for (int s = 0; s < GR / 2; ++s) ca[s] = xa[s], cb[s] = rb[s];
    if (i + GR < i1) fetch(i + GR);   // in flight under the MFMAs below
#pragma unroll
    for (int s = 0; s < GR / 2; ++s) {
      acc[0] = __builtin_amdgcn_mfma_f32_32x32x2f32(ca[s].x, cb[s], acc[0], 0, 0, 0);
      acc[1] = __builtin_amdgcn_mfma_f32_32x32x2f32(ca[s].y, cb[s], acc[1], 0, 0, 0);
      acc[2] = __builtin_amdgcn_mfma_f32_32x32x2f32(ca[s].z, cb[s], acc[2], 0, 0, 0);
      acc[3] = __builtin_amdgcn_mfma_f32_32x32x2f32(ca[s].w, cb[s], acc[3], 0, 0, 0);
    }
  }
  // register i of acc[m] is MFMA row j = 8 (i >> 2) + 4 h + (i & 3), i.e. dim (wave's first) + 4 j + m, against
  // problem jr
  float* out = ws + (int64_t)blockIdx.y * d * p;
  const int dw = blockIdx.x * GD + (GD / 4) * wv;
#pragma unroll
  for (int m = 0; m < 4; ++m)
#pragma unroll
    for (int i = 0; i < 16; ++i) {
      const int dim = dw + 4 * (8 * (i >> 2) + 4 * h + (i & 3)) + m;
      if (dim < d && cok) out[(int64_t)dim * p + jr] = acc[m][i];
    }
}

__global__ __launch_bounds__(LTHREADS) void logreg_gsum_kernel(const float* __restrict__ ws, int64_t dp, int splits,
                                                               double* __restrict__ g) {
  for (int64_t e = (int64_t)blockIdx.x * LTHREADS + threadIdx.x; e < dp; e += (int64_t)gridDim.x * LTHREADS) {
    double s = 0.0;
    for (int k = 0; k < splits; ++k) s += (double)ws[(int64_t)k * dp + e];
    g[e] = s;
  }
}

// Workgroups of the gradient kernel that the device holds at once (CUs x workgroups per CU by the kernel's registers):
// asked of the runtime once.
int logreg_grad_slots() {
  static int slots = 0;
  if (slots == 0) {
    int dev = 0, cus = 0, per = 0;
    if (hipGetDevice(&dev) == hipSuccess &&
        hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) == hipSuccess &&
        hipOccupancyMaxActiveBlocksPerMultiprocessor(&per, logreg_grad_kernel<true>, LTHREADS, 0) == hipSuccess &&
        cus > 0 && per > 0) {
      slots = cus * per;
    } else {
      (void)hipGetLastError();
      slots = 512;
    }
  }
  return slots;
}

// The rows are split so that a launch is whole rounds of the workgroups the device holds at once and never a few
// more: with 1040 workgroups on 512 slots the third, nearly empty round cost 5 %, with 1024 on 768 the second, a third
// full, 20 %.  One round where a CU holds three or more workgroups, two otherwise; every split's partial is written
// and read once, so more rounds than that cost more traffic than they hide.  A split is a whole number of GR-row
// chunks.
int logreg_auto_splits(int64_t n, int d) {
  const int64_t dtiles = (d + GD - 1) / GD, chunks = (n + GR - 1) / GR;
  const int slots = logreg_grad_slots();
  int64_t s = (slots >= 768 ? slots : 2 * slots) / dtiles;
  if (s > chunks) s = chunks;
  if (s > AW_LOGREG_MAX_SPLITS) s = AW_LOGREG_MAX_SPLITS;
  return (int)(s < 1 ? 1 : s);
}

int logreg_check(const char* who, int64_t n, int d, int p, int splits) {
  AW_REQUIRE(n >= 0 && n <= ((int64_t)1 << 36), "%s: n = %lld outside 0..2^36", who, (long long)n);
  AW_REQUIRE(d >= 1 && d < (1 << 22), "%s: d = %d outside 1..2^22 - 1", who, d);
  AW_REQUIRE(p >= 1 && p <= AW_LOGREG_MAX_P, "%s: p = %d outside 1..%d", who, p, AW_LOGREG_MAX_P);
  AW_REQUIRE(splits >= 0 && splits <= AW_LOGREG_MAX_SPLITS, "%s: splits = %d outside 0..%d (0 = auto)", who, splits,
             AW_LOGREG_MAX_SPLITS);
  return AW_OK;
}

int64_t logreg_fwd_bytes(int64_t n) { return ((n + LM - 1) / LM) * 2 * LP * (int64_t)sizeof(double); }
int64_t logreg_grad_bytes(int64_t n, int d, int p, int sp) {
  return n > 0 ? (int64_t)sp * d * p * (int64_t)sizeof(float) : 0;
}

}  // namespace

extern "C" int64_t aw_logreg_workspace(int64_t n, int d, int p, int splits) {
  if (logreg_check("aw_logreg_workspace", n, d, p, splits) != AW_OK) return AW_ERR_ARG;
  const int sp = splits > 0 ? splits : logreg_auto_splits(n, d);
  const int64_t f = logreg_fwd_bytes(n), g = logreg_grad_bytes(n, d, p, sp);
  return f > g ? f : g;
}

extern "C" int aw_logreg_describe(int* tile_n, int* chunk_d, int* tile_d, int* max_p) {
  if (tile_n) *tile_n = LM;
  if (chunk_d) *chunk_d = LK;
  if (tile_d) *tile_d = GD;
  if (max_p) *max_p = AW_LOGREG_MAX_P;
  return AW_OK;
}

extern "C" int aw_logreg_forward(const float* x, int64_t n, int64_t ldx, int d, const float* w, const float* b, int p,
                                 const int* y, const int* cls, float* z, float* r, double* loss, double* gb, void* ws,
                                 int64_t ws_bytes, void* stream) {
  const int st = logreg_check("aw_logreg_forward", n, d, p, 0);
  if (st != AW_OK) return st;
  AW_REQUIRE(ldx >= d && ldx < (1 << 22), "aw_logreg_forward: row stride ldx = %lld must lie in d = %d .. 2^22 - 1",
             (long long)ldx, d);
  AW_REQUIRE(w && b, "aw_logreg_forward: w and b must not be NULL");
  AW_REQUIRE((x && z) || n == 0, "aw_logreg_forward: x and z must not be NULL with n = %lld", (long long)n);
  AW_REQUIRE(((uintptr_t)x & 3) == 0, "aw_logreg_forward: x must be 4-byte aligned");
  const bool labelled = cls != nullptr;   // cls has p >= 1 elements; y may be NULL when n == 0
  AW_REQUIRE(labelled || !y, "aw_logreg_forward: labels need cls, loss and gb");
  const int64_t blocks = (n + LM - 1) / LM;
  AW_REQUIRE(blocks <= 0x7FFFFFFFll, "aw_logreg_forward: n = %lld needs too many row tiles", (long long)n);
  if (labelled) {
    AW_REQUIRE(loss && gb, "aw_logreg_forward: labels need cls, loss and gb");
    AW_REQUIRE((y && r) || n == 0, "aw_logreg_forward: cls needs y and r with n = %lld", (long long)n);
    AW_REQUIRE(n == 0 || (ws && ws_bytes >= logreg_fwd_bytes(n)),
               "aw_logreg_forward: workspace of %lld bytes, need %lld (aw_logreg_workspace)", (long long)ws_bytes,
               (long long)logreg_fwd_bytes(n));
    AW_REQUIRE(((uintptr_t)ws & 7) == 0, "aw_logreg_forward: the workspace must be 8-byte aligned");
  }
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  double* part = static_cast<double*>(ws);
  if (n > 0) {
    const bool xvec = ((uintptr_t)x & 15) == 0 && (ldx & 3) == 0;   // 16-B loads: aligned base and stride
    const dim3 grid((unsigned)blocks), block(LTHREADS);
    if (xvec)
      hipLaunchKernelGGL(logreg_fwd_kernel<true>, grid, block, 0, s, x, n, ldx, d, w, b, p, y, cls, z, r, part);
    else
      hipLaunchKernelGGL(logreg_fwd_kernel<false>, grid, block, 0, s, x, n, ldx, d, w, b, p, y, cls, z, r, part);
    const int st2 = aw::check_launch("aw_logreg_forward");
    if (st2 != AW_OK) return st2;
  }
  if (labelled) {
    hipLaunchKernelGGL(logreg_sum_kernel, dim3((unsigned)p, 2), dim3(LTHREADS), 0, s, part, blocks, loss, gb);
    return aw::check_launch("aw_logreg_forward (sum)");
  }
  return AW_OK;
}

extern "C" int aw_logreg_grad(const float* x, int64_t n, int64_t ldx, int d, const float* r, int p, int splits,
                              void* ws, int64_t ws_bytes, double* g, void* stream) {
  const int st = logreg_check("aw_logreg_grad", n, d, p, splits);
  if (st != AW_OK) return st;
  AW_REQUIRE(ldx >= d && ldx < (1 << 22), "aw_logreg_grad: row stride ldx = %lld must lie in d = %d .. 2^22 - 1",
             (long long)ldx, d);
  AW_REQUIRE(g, "aw_logreg_grad: g must not be NULL");
  AW_REQUIRE((x && r) || n == 0, "aw_logreg_grad: x and r must not be NULL with n = %lld", (long long)n);
  AW_REQUIRE(((uintptr_t)x & 3) == 0, "aw_logreg_grad: x must be 4-byte aligned");
  const int sp = n > 0 ? (splits > 0 ? splits : logreg_auto_splits(n, d)) : 0;
  const int64_t need = logreg_grad_bytes(n, d, p, sp);
  AW_REQUIRE(n == 0 || (ws && ws_bytes >= need), "aw_logreg_grad: workspace of %lld bytes, need %lld (aw_logreg_workspace)",
             (long long)ws_bytes, (long long)need);
  AW_REQUIRE(((uintptr_t)ws & 3) == 0, "aw_logreg_grad: the workspace must be 4-byte aligned");
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  float* part = static_cast<float*>(ws);
  const int64_t dp = (int64_t)d * p;
  if (n > 0) {
    const int64_t chunks = (n + GR - 1) / GR;
    const int64_t rps = ((chunks + sp - 1) / sp) * GR;
    const bool xvec = ((uintptr_t)x & 15) == 0 && (ldx & 3) == 0 && (d & 3) == 0;   // 16-B loads
    const dim3 grid((unsigned)((d + GD - 1) / GD), (unsigned)sp), block(LTHREADS);
    if (xvec)
      hipLaunchKernelGGL(logreg_grad_kernel<true>, grid, block, 0, s, x, n, ldx, d, r, p, rps, part);
    else
      hipLaunchKernelGGL(logreg_grad_kernel<false>, grid, block, 0, s, x, n, ldx, d, r, p, rps, part);
    const int st2 = aw::check_launch("aw_logreg_grad");
    if (st2 != AW_OK) return st2;
  }
  int64_t gblocks = (dp + LTHREADS - 1) / LTHREADS;
  if (gblocks > 2048) gblocks = 2048;
  hipLaunchKernelGGL(logreg_gsum_kernel, dim3((unsigned)gblocks), dim3(LTHREADS), 0, s, part, dp, sp, g);
  return aw::check_launch("aw_logreg_grad (sum)");
}
