// GRU recurrence for gfx950 (model/gru.py:25,47 -- nn.GRU(in_dim, H, L, batch_first) of the weld-quality classifier).
//
// Everything that is not recurrent (input projection, input gradient, weight gradients) is an aw_gemm over all B*T
// rows; the bias gradients are f32 column sums of the gate gradients (gru_bias_grad_kernel below).  This file holds the recurrence: one launch per time step, forward and backward, each an MFMA GEMM
// against W_hh whose epilogue finishes the cell.  No workgroup waits on another, no atomics, plain vector stores:
// the same inputs give the same bits.
//
// Padded layout (the kernels' own): Hp = H rounded up to 32.  Every activation row is Hp wide (3*Hp / 4*Hp for the
// gate-blocked ones, gate g at columns [g*Hp, g*Hp + H)), columns >= H are exact zeros, written by the kernels
// themselves.  The packed W_hh copies are zero-padded the same way (aw_gru_pack_weights), so the GEMMs see whole
// 16 x 16 x (64 B of K) fragments and the padding contributes exact zeros.
//
// Tile: one wave owns 16 hidden units x 16 batch rows; the weights are the MFMA A operand and the batch rows the B
// operand, so a lane ends up with 4 consecutive hidden units of one batch row (C/D: row = 4*(lane >> 4) + reg is the
// unit, col = lane & 15 the batch row) and every epilogue load / store is one 16-B vector.  In the forward the wave's
// "column tile" is gate-interleaved: the same 16 units j in all three gate blocks (rows j, H + j, 2H + j of W_hh), three
// accumulators, so r, z and n of element (b, j) meet in one lane's registers.  A workgroup is 4 waves = 64 batch rows
// of one unit tile (the W fragments are shared through L1 / L2).  Fragments come straight from global memory, 16 B per
// lane (both operands are K-contiguous and L2-resident: W_hh is 3.5 MB in bf16, h is B x Hp); at ~1.8 GFLOP per step
// the launch is latency-bound, not MFMA-bound, and the K loop keeps 4 sub-steps of loads in flight.
#include "common.h"
#include "gemm_core.h"

namespace {

constexpr int GRU_THREADS = 256;   // 4 waves: 64 batch rows of one 16-unit tile
constexpr int GRU_UNROLL = 4;      // K sub-steps (64 B of K each) in flight per wave

__host__ __device__ inline int gru_hp(int H) { return (H + 31) / 32 * 32; }

// 16 B of row `row`: K sub-step u (64 B), lane group g
template <typename T>
__device__ __forceinline__ uint4 gfrag(const T* base, int64_t ld, int row, int u, int g) {
  return *reinterpret_cast<const uint4*>(reinterpret_cast<const char*>(base + (int64_t)row * ld) + 64 * u + 16 * g);
}

__device__ __forceinline__ float sigmoidf_(float x) { return 1.0f / (1.0f + expf(-x)); }

__device__ __forceinline__ f32x4 ld4(const float* p) { return *reinterpret_cast<const f32x4*>(p); }
__device__ __forceinline__ void st4(float* p, f32x4 v) { *reinterpret_cast<f32x4*>(p) = v; }
__device__ __forceinline__ void st4_bf16(bf16* p, f32x4 v) {
  bf16 h[4] = {(bf16)v[0], (bf16)v[1], (bf16)v[2], (bf16)v[3]};   // round to nearest even
  u32x2 u;
  memcpy(&u, h, 8);
  *reinterpret_cast<u32x2*>(p) = u;
}

// W_hh (3H, H) f32 -> forward image [3][Hp][Hp] (gate, unit j, k) and backward image [Hp][3*Hp] (k, gate*Hp + j),
// zero-padded, as T.
template <typename T>
__global__ void gru_pack_kernel(const float* __restrict__ w, int H, int Hp, T* __restrict__ wf, T* __restrict__ wb) {
  const int64_t n = (int64_t)3 * Hp * Hp;
  for (int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; e < n; e += (int64_t)gridDim.x * blockDim.x) {
    const int k = (int)(e % Hp), j = (int)((e / Hp) % Hp), g = (int)(e / ((int64_t)Hp * Hp));
    const float v = (j < H && k < H) ? w[((int64_t)g * H + j) * H + k] : 0.f;
    if (wf) wf[e] = from_f32<T>(v);
    if (wb) wb[(int64_t)k * 3 * Hp + g * Hp + j] = from_f32<T>(v);
  }
}

// ------------------------------------------------------------------------------------------------ forward step
// GH = h_prev . W_hh^T (skipped when h_prev == NULL), then per element (b, j):
//   r = s(gi_r + gh_r + b_hr)  z = s(gi_z + gh_z + b_hz)  hn = gh_n + b_hn  n = tanh(gi_n + r hn)  h = (1 - z) n + z h_prev
template <typename T>
__global__ void __launch_bounds__(GRU_THREADS)
gru_step_fwd_kernel(int B, int H, int Hp, const T* __restrict__ hp_op, const float* __restrict__ hp,
                    const T* __restrict__ wf, const float* __restrict__ gi, const float* __restrict__ bhh,
                    float* __restrict__ h, bf16* __restrict__ h_op, float* __restrict__ saved) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int j0 = blockIdx.x * 16, b0 = blockIdx.y * 64 + wave * 16;
  if (b0 >= B) return;
  const int i = lane & 15, g = lane >> 4;
  f32x4 acc[3] = {{0.f, 0.f, 0.f, 0.f}, {0.f, 0.f, 0.f, 0.f}, {0.f, 0.f, 0.f, 0.f}};
  if (hp_op) {
    const int brow = min(b0 + i, B - 1);          // tail rows read the last row; their results are not stored
    const int nsub = Hp * (int)sizeof(T) / 64;    // Hp % 32 == 0: whole sub-steps; past the last one the loads
                                                  // repeat it and the MFMAs are skipped
    const T* w0 = wf + (int64_t)(j0 + i) * Hp;
    const int64_t gate = (int64_t)Hp * Hp;
    for (int u0 = 0; u0 < nsub; u0 += GRU_UNROLL) {
      uint4 fb[GRU_UNROLL], fw[GRU_UNROLL][3];
#pragma unroll
      for (int s = 0; s < GRU_UNROLL; ++s) {
        const int u = min(u0 + s, nsub - 1);
        fb[s] = gfrag(hp_op, Hp, brow, u, g);
#pragma unroll
        for (int q = 0; q < 3; ++q) fw[s][q] = gfrag(w0 + q * gate, 0, 0, u, g);
      }
#pragma unroll
      for (int s = 0; s < GRU_UNROLL; ++s) {
        if (u0 + s < nsub) {
#pragma unroll
          for (int q = 0; q < 3; ++q) awg::Mfma<T>::run(acc[q], fw[s][q], fb[s]);
        }
      }
    }
  }
  // epilogue: lane holds units j0 + 4g .. + 3 of batch row b0 + i
  const int b = b0 + i, j = j0 + 4 * g;
  if (b >= B) return;
  f32x4 r, z, n, hn, hv;
  const f32x4 gr = ld4(gi + (int64_t)b * 3 * Hp + j), gz = ld4(gi + (int64_t)b * 3 * Hp + Hp + j),
              gn = ld4(gi + (int64_t)b * 3 * Hp + 2 * Hp + j);
  f32x4 hpv = {0.f, 0.f, 0.f, 0.f};
  if (hp) hpv = ld4(hp + (int64_t)b * Hp + j);
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    if (j + e < H) {
      r[e] = sigmoidf_(gr[e] + (acc[0][e] + bhh[j + e]));
      z[e] = sigmoidf_(gz[e] + (acc[1][e] + bhh[H + j + e]));
      hn[e] = acc[2][e] + bhh[2 * H + j + e];
      n[e] = tanhf(fmaf(r[e], hn[e], gn[e]));
      hv[e] = fmaf(z[e], hpv[e] - n[e], n[e]);       // (1 - z) n + z h_prev
    } else {
      r[e] = z[e] = hn[e] = n[e] = hv[e] = 0.f;      // padding columns stay exact zeros
    }
  }
  st4(h + (int64_t)b * Hp + j, hv);
  if (h_op) st4_bf16(h_op + (int64_t)b * Hp + j, hv);
  float* sv = saved + (int64_t)b * 4 * Hp + j;
  st4(sv, r);
  st4(sv + Hp, z);
  st4(sv + 2 * Hp, n);
  st4(sv + 3 * Hp, hn);
}

// ------------------------------------------------------------------------------------------------ backward step
// dh = dGH_next . W_hh (skipped when dgh_next == NULL) + dh_next * z_next + dy, then this step's gate gradients:
//   dn = dh (1 - z)(1 - n^2)   dz = dh (h_prev - n) z (1 - z)   dr = dn hn r (1 - r)
//   dGI = [dr, dz, dn]   dGH = [dr, dz, dn r]
template <typename T>
__global__ void __launch_bounds__(GRU_THREADS)
gru_step_bwd_kernel(int B, int H, int Hp, const T* __restrict__ dgh_next, const float* __restrict__ dh_next,
                    const float* __restrict__ saved_next, const T* __restrict__ wb, const float* __restrict__ dy,
                    const float* __restrict__ saved, const float* __restrict__ hp, float* __restrict__ dh,
                    float* __restrict__ dgi, float* __restrict__ dgh, bf16* __restrict__ dgi_op,
                    bf16* __restrict__ dgh_op) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int j0 = blockIdx.x * 16, b0 = blockIdx.y * 64 + wave * 16;
  if (b0 >= B) return;
  const int i = lane & 15, g = lane >> 4;
  f32x4 acc = {0.f, 0.f, 0.f, 0.f};
  if (dgh_next) {
    const int brow = min(b0 + i, B - 1);
    const int64_t K = (int64_t)3 * Hp;
    const int nsub = (int)(K * sizeof(T) / 64);
    for (int u0 = 0; u0 < nsub; u0 += GRU_UNROLL) {
      uint4 fb[GRU_UNROLL], fw[GRU_UNROLL];
#pragma unroll
      for (int s = 0; s < GRU_UNROLL; ++s) {
        const int u = min(u0 + s, nsub - 1);
        fb[s] = gfrag(dgh_next, K, brow, u, g);
        fw[s] = gfrag(wb, K, j0 + i, u, g);
      }
#pragma unroll
      for (int s = 0; s < GRU_UNROLL; ++s)
        if (u0 + s < nsub) awg::Mfma<T>::run(acc, fw[s], fb[s]);
    }
  }
  const int b = b0 + i, j = j0 + 4 * g;
  if (b >= B) return;
  f32x4 d = acc;
  if (dh_next) {
    const f32x4 c = ld4(dh_next + (int64_t)b * Hp + j), zn = ld4(saved_next + (int64_t)b * 4 * Hp + Hp + j);
#pragma unroll
    for (int e = 0; e < 4; ++e) d[e] = fmaf(c[e], zn[e], d[e]);
  }
  if (dy) {
    const f32x4 y = ld4(dy + (int64_t)b * Hp + j);
#pragma unroll
    for (int e = 0; e < 4; ++e) d[e] += y[e];
  }
  const float* sv = saved + (int64_t)b * 4 * Hp + j;
  const f32x4 r = ld4(sv), z = ld4(sv + Hp), n = ld4(sv + 2 * Hp), hn = ld4(sv + 3 * Hp);
  f32x4 hpv = {0.f, 0.f, 0.f, 0.f};
  if (hp) hpv = ld4(hp + (int64_t)b * Hp + j);
  f32x4 dr, dz, dn, dnr;
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    if (j + e < H) {
      dn[e] = d[e] * (1.f - z[e]) * (1.f - n[e] * n[e]);
      dz[e] = d[e] * (hpv[e] - n[e]) * (z[e] * (1.f - z[e]));
      dr[e] = dn[e] * hn[e] * (r[e] * (1.f - r[e]));
      dnr[e] = dn[e] * r[e];
    } else {
      d[e] = dn[e] = dz[e] = dr[e] = dnr[e] = 0.f;
    }
  }
  st4(dh + (int64_t)b * Hp + j, d);
  const int64_t o = (int64_t)b * 3 * Hp + j;
  st4(dgi + o, dr);
  st4(dgi + o + Hp, dz);
  st4(dgi + o + 2 * Hp, dn);
  st4(dgh + o, dr);
  st4(dgh + o + Hp, dz);
  st4(dgh + o + 2 * Hp, dnr);
  if (dgi_op) {
    st4_bf16(dgi_op + o, dr);
    st4_bf16(dgi_op + o + Hp, dz);
    st4_bf16(dgi_op + o + 2 * Hp, dn);
  }
  if (dgh_op) {
    st4_bf16(dgh_op + o, dr);
    st4_bf16(dgh_op + o + Hp, dz);
    st4_bf16(dgh_op + o + 2 * Hp, dnr);
  }
}

// db[g*H + j] += sum over rows of dg[row][g*Hp + j] (f32, rows x 3*Hp): the bias gradients.  One owner per column and
// a fixed summation order: 4 waves take every 4th row (two running sums each), LDS adds the four.
__global__ void __launch_bounds__(256)
gru_bias_grad_kernel(const float* __restrict__ dg, int64_t rows, int H, int Hp, float* __restrict__ db) {
  __shared__ float part[4][64];
  const int lane = threadIdx.x & 63, q = threadIdx.x >> 6;
  const int c = blockIdx.x * 64 + lane;
  const int64_t ld = (int64_t)3 * Hp;
  float s0 = 0.f, s1 = 0.f;
  if (c < ld) {
    int64_t r = q;
    for (; r + 4 < rows; r += 8) {
      s0 += dg[r * ld + c];
      s1 += dg[(r + 4) * ld + c];
    }
    if (r < rows) s0 += dg[r * ld + c];
  }
  part[q][lane] = s0 + s1;
  __syncthreads();
  if (q == 0 && c < ld) {
    const int g = c / Hp, j = c % Hp;
    if (j < H) db[g * H + j] += (part[0][lane] + part[1][lane]) + (part[2][lane] + part[3][lane]);
  }
}

inline bool al16(const void* p) { return ((uintptr_t)p % 16) == 0; }

}  // namespace

extern "C" int aw_gru_pack_weights(const float* w_hh, int H, int op_dtype, void* w_fwd, void* w_bwd, void* stream) {
  AW_REQUIRE(w_hh && H > 0 && (w_fwd || w_bwd), "aw_gru_pack_weights: bad args");
  AW_REQUIRE(op_dtype == AW_F32 || op_dtype == AW_BF16, "aw_gru_pack_weights: op_dtype must be AW_F32 or AW_BF16");
  AW_REQUIRE(al16(w_fwd) && al16(w_bwd), "aw_gru_pack_weights: packed images must be 16-B aligned");
  const int Hp = gru_hp(H);
  const int64_t n = (int64_t)3 * Hp * Hp;
  const int grid = (int)((n + 255) / 256 < 4096 ? (n + 255) / 256 : 4096);
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  if (op_dtype == AW_BF16)
    hipLaunchKernelGGL(gru_pack_kernel<bf16>, dim3(grid), dim3(256), 0, s, w_hh, H, Hp, (bf16*)w_fwd, (bf16*)w_bwd);
  else
    hipLaunchKernelGGL(gru_pack_kernel<float>, dim3(grid), dim3(256), 0, s, w_hh, H, Hp, (float*)w_fwd, (float*)w_bwd);
  return aw::check_launch("aw_gru_pack_weights");
}

extern "C" int aw_gru_step_fwd(int B, int H, int op_dtype, const void* h_prev_op, const float* h_prev,
                               const void* w_fwd, const float* gi, const float* b_hh, float* h, void* h_op,
                               float* saved, void* stream) {
  AW_REQUIRE(B > 0 && H > 0 && gi && b_hh && h && saved, "aw_gru_step_fwd: bad args");
  AW_REQUIRE(op_dtype == AW_F32 || op_dtype == AW_BF16, "aw_gru_step_fwd: op_dtype must be AW_F32 or AW_BF16");
  AW_REQUIRE((h_prev_op == nullptr) == (h_prev == nullptr), "aw_gru_step_fwd: h_prev_op and h_prev go together");
  AW_REQUIRE(!h_prev_op || w_fwd, "aw_gru_step_fwd: w_fwd is needed with a previous state");
  AW_REQUIRE(op_dtype == AW_F32 ? h_op == nullptr : h_op != nullptr,
             "aw_gru_step_fwd: h_op is the bf16 copy (bf16 mode only; f32 mode reads h itself)");
  AW_REQUIRE(al16(h_prev_op) && al16(h_prev) && al16(w_fwd) && al16(gi) && al16(h) && al16(h_op) && al16(saved),
             "aw_gru_step_fwd: buffers must be 16-B aligned");
  const int Hp = gru_hp(H);
  const dim3 grid(Hp / 16, (B + 63) / 64);
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  if (op_dtype == AW_BF16)
    hipLaunchKernelGGL(gru_step_fwd_kernel<bf16>, grid, dim3(GRU_THREADS), 0, s, B, H, Hp, (const bf16*)h_prev_op,
                       h_prev, (const bf16*)w_fwd, gi, b_hh, h, (bf16*)h_op, saved);
  else
    hipLaunchKernelGGL(gru_step_fwd_kernel<float>, grid, dim3(GRU_THREADS), 0, s, B, H, Hp, (const float*)h_prev_op,
                       h_prev, (const float*)w_fwd, gi, b_hh, h, (bf16*)nullptr, saved);
  return aw::check_launch("aw_gru_step_fwd");
}

extern "C" int aw_gru_step_bwd(int B, int H, int op_dtype, const void* dgh_next_op, const float* dh_next,
                               const float* saved_next, const void* w_bwd, const float* dy, const float* saved,
                               const float* h_prev, float* dh, float* dgi, float* dgh, void* dgi_op, void* dgh_op,
                               void* stream) {
  AW_REQUIRE(B > 0 && H > 0 && saved && dh && dgi && dgh, "aw_gru_step_bwd: bad args");
  AW_REQUIRE(op_dtype == AW_F32 || op_dtype == AW_BF16, "aw_gru_step_bwd: op_dtype must be AW_F32 or AW_BF16");
  AW_REQUIRE((dgh_next_op == nullptr) == (dh_next == nullptr) && (dh_next == nullptr) == (saved_next == nullptr),
             "aw_gru_step_bwd: dgh_next_op, dh_next and saved_next go together (all NULL at the last time step)");
  AW_REQUIRE(!dgh_next_op || w_bwd, "aw_gru_step_bwd: w_bwd is needed with an incoming recurrent gradient");
  AW_REQUIRE(dh_next || dy, "aw_gru_step_bwd: no incoming gradient at all");
  AW_REQUIRE(op_dtype == AW_F32 ? (!dgi_op && !dgh_op) : (dgi_op && dgh_op),
             "aw_gru_step_bwd: dgi_op / dgh_op are the bf16 copies (bf16 mode only)");
  AW_REQUIRE(al16(dgh_next_op) && al16(dh_next) && al16(saved_next) && al16(w_bwd) && al16(dy) && al16(saved) &&
                 al16(h_prev) && al16(dh) && al16(dgi) && al16(dgh) && al16(dgi_op) && al16(dgh_op),
             "aw_gru_step_bwd: buffers must be 16-B aligned");
  const int Hp = gru_hp(H);
  const dim3 grid(Hp / 16, (B + 63) / 64);
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  if (op_dtype == AW_BF16)
    hipLaunchKernelGGL(gru_step_bwd_kernel<bf16>, grid, dim3(GRU_THREADS), 0, s, B, H, Hp, (const bf16*)dgh_next_op,
                       dh_next, saved_next, (const bf16*)w_bwd, dy, saved, h_prev, dh, dgi, dgh, (bf16*)dgi_op,
                       (bf16*)dgh_op);
  else
    hipLaunchKernelGGL(gru_step_bwd_kernel<float>, grid, dim3(GRU_THREADS), 0, s, B, H, Hp,
                       (const float*)dgh_next_op, dh_next, saved_next, (const float*)w_bwd, dy, saved, h_prev, dh, dgi,
                       dgh, (bf16*)nullptr, (bf16*)nullptr);
  return aw::check_launch("aw_gru_step_bwd");
}

extern "C" int aw_gru_bias_grad(const float* dg, int64_t rows, int H, float* db, void* stream) {
  AW_REQUIRE(dg && db && rows >= 0 && H > 0, "aw_gru_bias_grad: bad args");
  if (rows == 0) return AW_OK;
  const int Hp = gru_hp(H);
  hipLaunchKernelGGL(gru_bias_grad_kernel, dim3((3 * Hp + 63) / 64), dim3(256), 0,
                     reinterpret_cast<hipStream_t>(stream), dg, rows, H, Hp, db);
  return aw::check_launch("aw_gru_bias_grad");
}
