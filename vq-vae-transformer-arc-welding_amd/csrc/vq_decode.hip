// Ids back to the decoder's input (arcweld.vqvae.decode): a row gather with the range check in the kernel.
//
// In eval the decoder's first layer depends on the id alone: y0[n] = E[idx[n]] . Wd0^T + b and ya0[n] = GELU(y0[n]).
// aw_gemm computes the two tables over the K codebook rows once; this kernel copies row idx[n] of each to row n of the
// outputs.  One wave per output row, 16 bytes per lane and access; the tables (1.5 MB at K = H = 512) stay in L2, so
// the launch is bound by the 6 bytes per element it writes (bf16 operands: 2 + 2, f32 streams: 4 + 2 ... 4 + 4).
#include "common.h"

typedef __attribute__((ext_vector_type(4))) uint32_t aw_u32x4;

#define VQD_WAVES 4

// bx / ba: bytes per row of table_x / table_a (multiples of 16; ba = 0: no second table)
__global__ __launch_bounds__(64 * VQD_WAVES) void vq_decode_gather_kernel(
    const int64_t* __restrict__ idx, int64_t N, const char* __restrict__ table_x, const char* __restrict__ table_a,
    int K, int bx, int ba, char* __restrict__ y0, char* __restrict__ ya0, int* __restrict__ bad_count) {
  const int lane = threadIdx.x & 63;
  const int64_t n = (int64_t)blockIdx.x * VQD_WAVES + (threadIdx.x >> 6);
  if (n >= N) return;
  const int64_t id = idx[n];                       // wave-uniform
  const bool ok = id >= 0 && id < (int64_t)K;      // an id outside [0, K) reads nothing: a zero row and one count
  if (!ok && lane == 0) atomicAdd(bad_count, 1);
  const aw_u32x4 zero = {0u, 0u, 0u, 0u};
  const char* sx = table_x + (ok ? id : 0) * (int64_t)bx;
  char* dx = y0 + n * (int64_t)bx;
  for (int c = lane * 16; c < bx; c += 64 * 16)
    *(aw_u32x4*)(dx + c) = ok ? *(const aw_u32x4*)(sx + c) : zero;
  if (ba > 0) {
    const char* sa = table_a + (ok ? id : 0) * (int64_t)ba;
    char* da = ya0 + n * (int64_t)ba;
    for (int c = lane * 16; c < ba; c += 64 * 16)
      *(aw_u32x4*)(da + c) = ok ? *(const aw_u32x4*)(sa + c) : zero;
  }
}

static inline int vqd_elem(int dtype) { return dtype == AW_BF16 ? 2 : 4; }
static inline bool vqd_al16(const void* p) { return ((uintptr_t)p & 15u) == 0; }

extern "C" int aw_vq_decode_gather(const int64_t* idx, int64_t N, const void* table_x, const void* table_a, int K,
                                   int H, int x_dtype, int a_dtype, void* y0, void* ya0, int* bad_count,
                                   void* stream) {
  AW_REQUIRE(idx && table_x && y0 && bad_count && N >= 0 && K > 0 && H > 0, "aw_vq_decode_gather: bad args");
  AW_REQUIRE((table_a == nullptr) == (ya0 == nullptr), "aw_vq_decode_gather: table_a and ya0 go together");
  AW_REQUIRE((x_dtype == AW_F32 || x_dtype == AW_BF16) && (a_dtype == AW_F32 || a_dtype == AW_BF16),
             "aw_vq_decode_gather: dtypes are AW_F32 or AW_BF16");
  const int64_t bx = (int64_t)H * vqd_elem(x_dtype), ba = table_a ? (int64_t)H * vqd_elem(a_dtype) : 0;
  AW_REQUIRE(bx % 16 == 0 && ba % 16 == 0 && bx < (1 << 30),
             "aw_vq_decode_gather: rows must be whole 16-byte pieces (H = %d)", H);
  AW_REQUIRE(vqd_al16(table_x) && vqd_al16(table_a) && vqd_al16(y0) && vqd_al16(ya0),
             "aw_vq_decode_gather: tables and outputs must be 16-byte aligned");
  if (N == 0) return AW_OK;
  AW_REQUIRE((N + VQD_WAVES - 1) / VQD_WAVES <= 0x7FFFFFFFll, "aw_vq_decode_gather: N too large");
  hipLaunchKernelGGL(vq_decode_gather_kernel, dim3((unsigned)((N + VQD_WAVES - 1) / VQD_WAVES)), dim3(64 * VQD_WAVES),
                     0, reinterpret_cast<hipStream_t>(stream), idx, N, (const char*)table_x, (const char*)table_a, K,
                     (int)bx, (int)ba, (char*)y0, (char*)ya0, bad_count);
  return aw::check_launch("aw_vq_decode_gather");
}
