// TS2Vec baseline encoder, eval forward (aw_ts_input_fc, aw_ts_conv; include/arcweld_amd.h): the hot path of
// arcweld.ts2vec.TSEncoder.encode.  Exact f32 throughout.
//
//   ts_input_fc_kernel  one thread per (row, 4 hidden channels): the C_in <= 8 input projection as an in-order fmaf
//                       chain, the NaN / mask zeroing, and both of the first block's inputs (x and gelu(x)).
//   ts_conv_kernel      a dilated 3-tap (or pointwise) convolution as a GEMM on the f32-input MFMA.  Grid (time tiles,
//                       channel tiles, sequences): a 256-thread workgroup owns CT = 128 time steps x CN = 64 output
//                       channels of ONE sequence, so a tile never spans two sequences.  The K loop runs over (live tap,
//                       chunk of CD = 32 input channels): the tile's 128 activation rows, shifted by the tap's offset,
//                       and 64 weight rows go through LDS as in pair_tile.h -- range-checked 16-byte buffer loads ->
//                       registers -> LDS, the next step's loads in flight under this step's MFMAs, two stages, one
//                       barrier per step.  The activation descriptor spans exactly this sequence's T rows and a row
//                       whose source step is outside [0, T) is loaded at pt::BAD_OFF (zeros), so neither a
//                       neighbouring sequence nor anything past the tensor is ever read.  A tap that is dead for every
//                       row of the tile (source steps all outside the sequence) is skipped, not multiplied as zeros:
//                       with dilation >= T that leaves the centre tap.
//                       Wave w owns time rows 32 w .. 32 w + 31 against all 64 channels: two 32 x 32 accumulators, the
//                       weight rows as the MFMA's A operand (pair_tile.h's orientation), so a lane ends with one time
//                       step and runs of 4 consecutive channels.  The finished tile goes to LDS (over the idle stages)
//                       and is stored row by row in 16-byte quads: bias, residual, v and gelu(v) -- GELU once per
//                       element here, never on operand load.  With pool the workgroup reduces its tile over time and
//                       writes one partial row; ts_pool_kernel takes the maximum over the time tiles.
//                       One output element is accumulated by one wave in one fixed order that depends only on
//                       (t, T, dilation, widths): its bits depend on neither the batch, the sequence's place in it,
//                       nor the run.
#include "common.h"
#include "pair_tile.h"

#include <math.h>

#pragma clang fp contract(off)

namespace {

namespace pt = aw::pt;
constexpr int CT = 128;             // time steps per workgroup (the MFMA's B operand)
constexpr int CN = 64;              // output channels per workgroup (the MFMA's A operand)
constexpr int CD = 32;              // input channels per chunk
constexpr int CLD = CD + 4;         // staged row stride (floats), pair_tile.h's
constexpr int CTHREADS = 256;
constexpr int COT = CN + 4;         // result tile row stride
constexpr int CSTAGE = (CT + CN) * CLD;                  // floats per stage: time rows 0..127, then weight rows
constexpr int CF4 = (CT + CN) * (CD / 4) / CTHREADS;     // float4 per thread per step
constexpr int CF4_X = CT * (CD / 4) / CTHREADS;          // of which activation rows
static_assert(CT * COT <= 2 * CSTAGE, "the result tile overlays the two stages");
static_assert(2 * CSTAGE * 4 <= 80 * 1024, "conv LDS, two workgroups per CU");
static_assert(CT == 32 * (CTHREADS / 64), "one 32-row MFMA tile of time steps per wave");

struct conv_params {
  const float* in;
  const float* w;
  const float* bias;
  const float* resid;
  float* out;
  float* out_gelu;
  float* pool_ws;
  int T, cin, cout, taps, dil;
};

// Step (tap, ch) of the tile into registers: float4 i of thread tid is quad (tid & 7) of staged row (tid >> 3) + 32 i,
// activation rows for i < CF4_X, weight rows after.  Widths are multiples of 16: no quad straddles cin.
__device__ __forceinline__ void conv_fetch(float4 (&pre)[CF4], __amdgpu_buffer_rsrc_t xr, __amdgpu_buffer_rsrc_t wr,
                                           const conv_params& p, int t0, int n0, int tap, int ch, int tid) {
  const int d0 = ch * CD + (tid & 7) * 4;
  const bool dok = d0 + 4 <= p.cin;
  const int shift = p.taps == 3 ? (tap - 1) * p.dil : 0;
  const uint32_t ldb = (uint32_t)p.cin * 4u;
#pragma unroll
  for (int i = 0; i < CF4; ++i) {
    const int row = (tid >> 3) + 32 * i;
    uint32_t off;
    __amdgpu_buffer_rsrc_t r;
    if (i < CF4_X) {
      const int t = t0 + row, ts = t + shift;
      const bool ok = dok && t < p.T && ts >= 0 && ts < p.T;
      off = ok ? (uint32_t)ts * ldb + 4u * (uint32_t)d0 : pt::BAD_OFF;
      r = xr;
    } else {
      const int co = n0 + row - CT;
      const bool ok = dok && co < p.cout;
      off = ok ? (uint32_t)(tap * p.cout + co) * ldb + 4u * (uint32_t)d0 : pt::BAD_OFF;
      r = wr;
    }
    const pt::u32x4 u = __builtin_amdgcn_raw_buffer_load_b128(r, off, 0, 0);
    pre[i] = make_float4(__uint_as_float(u.x), __uint_as_float(u.y), __uint_as_float(u.z), __uint_as_float(u.w));
  }
}

__device__ __forceinline__ void conv_stage_put(float* sb, const float4 (&pre)[CF4], int tid) {
#pragma unroll
  for (int i = 0; i < CF4; ++i) {
    const int f = tid + i * CTHREADS;
    *reinterpret_cast<float4*>(sb + (f >> 3) * CLD + (f & 7) * 4) = pre[i];
  }
}

// One staged step: 32 MFMAs per wave.  Register r of acc[mi] is channel 32 mi + 8 (r >> 2) + 4 h + (r & 3) of the
// tile against time row 32 w + jr (h = lane >> 5, jr = lane & 31).
__device__ __forceinline__ void conv_dots(const float* sb, int tid, pt::f32x16 (&acc)[2]) {
  const int lane = tid & 63, w = tid >> 6, h = lane >> 5, jr = lane & 31;
  const float* sw = sb + (CT + jr) * CLD + 4 * h;        // A: weight rows
  const float* sx = sb + (32 * w + jr) * CLD + 4 * h;    // B: time rows
#pragma unroll
  for (int g = 0; g < CD / 8; ++g) {
    const float4 b4 = *reinterpret_cast<const float4*>(sx + 8 * g);
    const float4 a0 = *reinterpret_cast<const float4*>(sw + 8 * g);
    const float4 a1 = *reinterpret_cast<const float4*>(sw + 32 * CLD + 8 * g);
    const float av[2][4] = {{a0.x, a0.y, a0.z, a0.w}, {a1.x, a1.y, a1.z, a1.w}};
    const float bv[4] = {b4.x, b4.y, b4.z, b4.w};
#pragma unroll
    for (int s4 = 0; s4 < 4; ++s4)
#pragma unroll
      for (int mi = 0; mi < 2; ++mi)
        acc[mi] = __builtin_amdgcn_mfma_f32_32x32x2f32(av[mi][s4], bv[s4], acc[mi], 0, 0, 0);
  }
}

__global__ __launch_bounds__(CTHREADS, 2) void ts_conv_kernel(conv_params p) {
  __shared__ __attribute__((aligned(16))) float stage[2 * CSTAGE];
  const int tid = threadIdx.x;
  const int t0 = blockIdx.x * CT, n0 = blockIdx.y * CN;
  const int64_t b = blockIdx.z;
  const int rows = p.T - t0 < CT ? p.T - t0 : CT;        // time steps of this tile that exist (>= 1)
  const int nch = (p.cin + CD - 1) / CD;

  // the taps with a source step inside the sequence for at least one row of the tile
  int live = 1;                                          // taps == 1: the one tap
  if (p.taps == 3) {
    live = 2;                                            // the centre tap
    if (t0 + rows - 1 - p.dil >= 0) live |= 1;           // tap 0 reads step t - dil
    if (t0 + p.dil < p.T) live |= 4;                     // tap 2 reads step t + dil
  }
  const __amdgpu_buffer_rsrc_t xr = __builtin_amdgcn_make_buffer_rsrc(
      const_cast<float*>(p.in + b * p.T * p.cin), (short)0, (int)((uint32_t)p.T * (uint32_t)p.cin * 4u), 0x00020000);
  const __amdgpu_buffer_rsrc_t wr = __builtin_amdgcn_make_buffer_rsrc(
      const_cast<float*>(p.w), (short)0, (int)((uint32_t)p.taps * (uint32_t)p.cout * (uint32_t)p.cin * 4u),
      0x00020000);

  int tap = 0;
  while (!((live >> tap) & 1)) ++tap;
  int ch = 0;
  float4 pre[CF4];
  conv_fetch(pre, xr, wr, p, t0, n0, tap, ch, tid);
  pt::f32x16 acc[2];
#pragma unroll
  for (int mi = 0; mi < 2; ++mi)
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[mi][r] = 0.f;
  int buf = 0;
  while (tap < p.taps) {
    float* sb = stage + buf * CSTAGE;
    conv_stage_put(sb, pre, tid);
    __syncthreads();
    // the next step: the next chunk of this tap, else the first chunk of the next live tap
    if (++ch == nch) {
      ch = 0;
      do ++tap;
      while (tap < p.taps && !((live >> tap) & 1));
    }
    if (tap < p.taps) conv_fetch(pre, xr, wr, p, t0, n0, tap, ch, tid);
    conv_dots(sb, tid, acc);
    buf ^= 1;
  }

  // ---- the tile to LDS as [time row][channel], over the stages every wave has finished reading
  __syncthreads();
  float* ot = stage;
  {
    const int lane = tid & 63, w = tid >> 6, h = lane >> 5, jr = lane & 31;
#pragma unroll
    for (int mi = 0; mi < 2; ++mi)
#pragma unroll
      for (int q = 0; q < 4; ++q)
        *reinterpret_cast<float4*>(ot + (32 * w + jr) * COT + 32 * mi + 8 * q + 4 * h) =
            make_float4(acc[mi][4 * q], acc[mi][4 * q + 1], acc[mi][4 * q + 2], acc[mi][4 * q + 3]);
  }
  __syncthreads();

  // ---- the epilogue: row `row` of the tile is 64 consecutive channels of step t0 + row
  for (int f = tid; f < CT * (CN / 4); f += CTHREADS) {
    const int row = f / (CN / 4), c = (f % (CN / 4)) * 4;
    if (row >= rows || n0 + c >= p.cout) continue;
    const int64_t o = ((b * p.T + t0 + row) * p.cout) + n0 + c;
    const float4 a = *reinterpret_cast<const float4*>(ot + row * COT + c);
    const float4 bi = *reinterpret_cast<const float4*>(p.bias + n0 + c);
    float4 v = make_float4(__fadd_rn(a.x, bi.x), __fadd_rn(a.y, bi.y), __fadd_rn(a.z, bi.z), __fadd_rn(a.w, bi.w));
    if (p.resid) {
      const float4 r = *reinterpret_cast<const float4*>(p.resid + o);
      v = make_float4(__fadd_rn(v.x, r.x), __fadd_rn(v.y, r.y), __fadd_rn(v.z, r.z), __fadd_rn(v.w, r.w));
    }
    if (p.out) *reinterpret_cast<float4*>(p.out + o) = v;
    if (p.out_gelu)
      *reinterpret_cast<float4*>(p.out_gelu + o) = make_float4(gelu_erf(v.x), gelu_erf(v.y), gelu_erf(v.z), gelu_erf(v.w));
    if (p.pool_ws) *reinterpret_cast<float4*>(ot + row * COT + c) = v;    // this thread's own quad
  }
  if (p.pool_ws) {                                       // uniform: a kernel argument
    __syncthreads();
    if (tid < CN && n0 + tid < p.cout) {
      float m = ot[tid];
      for (int row = 1; row < rows; ++row) m = fmaxf(m, ot[row * COT + tid]);
      p.pool_ws[(b * gridDim.x + blockIdx.x) * p.cout + n0 + tid] = m;
    }
  }
}

// pool[b, c] = max over the time tiles of pool_ws[b, tile, c]
__global__ void ts_pool_kernel(const float* __restrict__ ws, float* __restrict__ pool, int64_t n, int tiles, int cout) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const int64_t b = i / cout;
  const int c = (int)(i % cout);
  float m = ws[b * tiles * cout + c];
  for (int t = 1; t < tiles; ++t) m = fmaxf(m, ws[(b * tiles + t) * cout + c]);
  pool[i] = m;
}

__global__ void ts_input_fc_kernel(const float* __restrict__ x, const unsigned char* __restrict__ mask,
                                   const float* __restrict__ w, const float* __restrict__ bias, int64_t rows, int cin,
                                   int hidden, float* __restrict__ out, float* __restrict__ out_gelu) {
  const int hq = hidden / 4;
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= rows * hq) return;
  const int64_t r = i / hq;
  const int h0 = (int)(i % hq) * 4;
  float xv[AW_TS_MAX_CIN];
  bool keep = mask == nullptr || mask[r] != 0;
#pragma unroll
  for (int c = 0; c < AW_TS_MAX_CIN; ++c) {
    xv[c] = c < cin ? x[r * cin + c] : 0.f;
    keep = keep && !(xv[c] != xv[c]);
  }
  float v[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    float s = bias[h0 + j];
#pragma unroll
    for (int c = 0; c < AW_TS_MAX_CIN; ++c)
      if (c < cin) s = __builtin_fmaf(xv[c], w[(h0 + j) * cin + c], s);
    v[j] = keep ? s : 0.f;
  }
  const int64_t o = r * hidden + h0;
  if (out) *reinterpret_cast<float4*>(out + o) = make_float4(v[0], v[1], v[2], v[3]);
  if (out_gelu)
    *reinterpret_cast<float4*>(out_gelu + o) = make_float4(gelu_erf(v[0]), gelu_erf(v[1]), gelu_erf(v[2]), gelu_erf(v[3]));
}

bool width_ok(int c) { return c >= 16 && c <= AW_TS_MAX_WIDTH && c % 16 == 0; }
bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }

}  // namespace

extern "C" int aw_ts_describe(int* tile_t, int* tile_c, int* chunk_c) {
  if (tile_t) *tile_t = CT;
  if (tile_c) *tile_c = CN;
  if (chunk_c) *chunk_c = CD;
  return AW_OK;
}

extern "C" int aw_ts_input_fc(const float* x, const void* mask, const float* w, const float* bias, int64_t rows,
                              int cin, int hidden, float* out, float* out_gelu, void* stream) {
  AW_REQUIRE(rows >= 0 && rows <= 0x7FFFFFFFll, "aw_ts_input_fc: rows = %lld outside 0..2^31 - 1", (long long)rows);
  AW_REQUIRE(cin >= 1 && cin <= AW_TS_MAX_CIN, "aw_ts_input_fc: cin = %d outside 1..%d", cin, AW_TS_MAX_CIN);
  AW_REQUIRE(width_ok(hidden), "aw_ts_input_fc: hidden = %d is not a multiple of 16 in 16..%d", hidden,
             AW_TS_MAX_WIDTH);
  AW_REQUIRE(out || out_gelu, "aw_ts_input_fc: no output");
  if (rows == 0) return AW_OK;
  AW_REQUIRE(x && w && bias, "aw_ts_input_fc: x, w and bias must not be NULL");
  AW_REQUIRE(((uintptr_t)x & 3) == 0 && ((uintptr_t)w & 3) == 0 && ((uintptr_t)bias & 3) == 0,
             "aw_ts_input_fc: x, w and bias must be 4-byte aligned");
  AW_REQUIRE(aligned16(out) && aligned16(out_gelu), "aw_ts_input_fc: out and out_gelu must be 16-byte aligned");
  const int64_t n = rows * (hidden / 4);
  hipLaunchKernelGGL(ts_input_fc_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0,
                     reinterpret_cast<hipStream_t>(stream), x, static_cast<const unsigned char*>(mask), w, bias, rows,
                     cin, hidden, out, out_gelu);
  return aw::check_launch("aw_ts_input_fc");
}

static int ts_conv_check(const char* who, int batch, int T, int cout) {
  AW_REQUIRE(batch >= 0 && batch <= AW_TS_MAX_BATCH, "%s: batch = %d outside 0..%d", who, batch, AW_TS_MAX_BATCH);
  AW_REQUIRE(T >= 1 && T <= AW_TS_MAX_T, "%s: T = %d outside 1..%d", who, T, AW_TS_MAX_T);
  AW_REQUIRE(width_ok(cout), "%s: cout = %d is not a multiple of 16 in 16..%d", who, cout, AW_TS_MAX_WIDTH);
  return AW_OK;
}

extern "C" int64_t aw_ts_pool_workspace(int batch, int T, int cout) {
  const int st = ts_conv_check("aw_ts_pool_workspace", batch, T, cout);
  if (st != AW_OK) return st;
  return (int64_t)batch * ((T + CT - 1) / CT) * cout * 4;
}

extern "C" int aw_ts_conv(const float* in, const float* w, const float* bias, const float* resid, int batch, int T,
                          int cin, int cout, int taps, int dilation, float* out, float* out_gelu, float* pool,
                          float* pool_ws, void* stream) {
  const int st = ts_conv_check("aw_ts_conv", batch, T, cout);
  if (st != AW_OK) return st;
  AW_REQUIRE(width_ok(cin), "aw_ts_conv: cin = %d is not a multiple of 16 in 16..%d", cin, AW_TS_MAX_WIDTH);
  AW_REQUIRE(taps == 1 || taps == 3, "aw_ts_conv: taps = %d, expected 1 or 3", taps);
  AW_REQUIRE(dilation >= 1 && dilation <= AW_TS_MAX_DILATION, "aw_ts_conv: dilation = %d outside 1..%d", dilation,
             AW_TS_MAX_DILATION);
  AW_REQUIRE(out || out_gelu || pool, "aw_ts_conv: no output");
  AW_REQUIRE(!pool || pool_ws, "aw_ts_conv: pool needs pool_ws (aw_ts_pool_workspace bytes)");
  if (batch == 0) return AW_OK;
  AW_REQUIRE(in && w && bias, "aw_ts_conv: in, w and bias must not be NULL");
  AW_REQUIRE(aligned16(in) && aligned16(w) && aligned16(bias) && aligned16(resid) && aligned16(out) &&
                 aligned16(out_gelu) && aligned16(pool) && aligned16(pool_ws),
             "aw_ts_conv: every operand must be 16-byte aligned");
  conv_params p;
  p.in = in, p.w = w, p.bias = bias, p.resid = resid, p.out = out, p.out_gelu = out_gelu;
  p.pool_ws = pool ? pool_ws : nullptr;
  p.T = T, p.cin = cin, p.cout = cout, p.taps = taps, p.dil = dilation;
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  const int tiles = (T + CT - 1) / CT;
  hipLaunchKernelGGL(ts_conv_kernel, dim3((unsigned)tiles, (unsigned)((cout + CN - 1) / CN), (unsigned)batch),
                     dim3(CTHREADS), 0, s, p);
  if (pool) {
    const int st2 = aw::check_launch("aw_ts_conv");
    if (st2 != AW_OK) return st2;
    const int64_t n = (int64_t)batch * cout;
    hipLaunchKernelGGL(ts_pool_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, pool_ws, pool, n, tiles,
                       cout);
  }
  return aw::check_launch("aw_ts_conv");
}
