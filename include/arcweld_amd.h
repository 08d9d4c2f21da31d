/* arcweld_amd.h -- C ABI of the MI355X (gfx950) HIP kernels behind the VQ-VAE + Transformer training path.
 *
 * The reference (tmdt-buw/VQ-VAE-Transformer-Arc-Welding) is pure Python on stock PyTorch ops; it has no FFI.
 * Its drop-in boundary is the nn.Module surface.  This library sits BELOW that
 * surface: each entry point replaces the ATen work of one reference call site, cited per function.
 *
 * Conventions (all entry points):
 *   - plain device pointers + sizes/leading dimensions (in elements); caller owns every buffer;
 *   - `stream` is a hipStream_t passed as void*; nothing synchronises the host;
 *   - return 0 (AW_OK) or a negative status; aw_last_error() returns a thread-local message;
 *   - no allocation inside (graph-capture safe); accumulators that must start at zero are documented.
 *
 * One entry point per operation: when an operation gains a parameter, its prototype changes and AW_ABI_VERSION goes
 * up; no forwarder keeps the old list alive.  The only consumer is the in-tree Python host, whose binding
 * (arcweld/_native.py) is read from this file: integer constants are `enum { NAME = n }` or `#define AW_NAME n`,
 * argument structs are `typedef struct { ... } aw_x;` of int / int64_t / uint64_t / uint32_t / float / double,
 * pointers and arrays sized by those constants, and every prototype is written out in full.  Keep to that dialect;
 * the binding refuses what it cannot read.
 * Pairs that stay apart on purpose, because they are different kernels or algorithms and not forwarders:
 * aw_sample_next / aw_sample_next_ex, aw_mse_finalize / _add, the aw_embed_bwd* family, aw_bn_finalize /
 * aw_bn_group_finalize, aw_gemm / aw_gemm_ws / aw_gemm_grouped, aw_weight_relayout / _batch.
 */
#ifndef ARCWELD_AMD_H
#define ARCWELD_AMD_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

enum { AW_OK = 0, AW_ERR_ARG = -1, AW_ERR_LAUNCH = -2 };
enum { AW_F32 = 0, AW_BF16 = 1 };
/* act: the activation of C2 modes 1 / 4 and of the epilogue's act'; AW_ACT_DERIV (with pre): pre already holds the
 * activation's derivative (saved by a c2_mode 4 forward), the epilogue multiplies by it as it is */
enum { AW_ACT_GELU_ERF = 0, AW_ACT_GELU_TANH = 1, AW_ACT_DERIV = 2 };

const char* aw_last_error(void);
/* aw_version() returns the AW_ABI_VERSION the library was built from; the host refuses a library that reports another
 * (names outlive their parameter lists, so a stale build would be called with the wrong arguments). */
#define AW_ABI_VERSION 2
int aw_version(void);

/* ------------------------------------------------------------------------------------------------ GEMM
 * C[M,N] = epilogue( alpha * op(A)[M,K] . op(B)[K,N] )  on MFMA (bf16 16x16x32 or exact-f32 16x16x4).
 * Replaces every conv1d / conv_transpose1d / addmm / mm of the hot path (SURVEY.md section 2 ATen table):
 *   model/vq_vae_patch_embedd.py:11,27,30,65,68,81,87,143 and model/transformer_block.py:30,32,78-79,
 *   model/transformer_decoder.py:29 -- forward, input-gradient and weight-gradient forms.
 * Operand storage (dtype = a_dtype for A and B; AW_F32 or AW_BF16):
 *   a_trans = 0: A[m*lda + k]        a_trans = 1: A[k*lda + m]
 *   b_trans = 0: B[n*ldb + k]        b_trans = 1: B[k*ldb + n]      (weights [out][in] are b_trans = 0)
 *   A transposed operand whose width (M or N) is not a multiple of 16 bytes but whose leading dimension is at
 *   least that width rounded up is read in whole 16-B chunks: every row, the last included, must be readable up
 *   to the rounded width (the padding values are never used).
 * Implicit k=3/pad=1 convolution along windows of `conv_seg` rows (conv_cin > 0):
 *   conv_operand = 0 (A, a_trans = 0): K = 3*conv_cin, A[m][j*cin+i] = src[(m + conv_dir*(j-1))*lda + i],
 *                  zero where the shifted row leaves its window;
 *   conv_operand = 1 (B, b_trans = 1): N = 3*conv_cin, B[k][j*cin+i] = src[(k + (j-1))*ldb + i], same mask.
 * Epilogue, per element (row r, col c), in this order:
 *   v = alpha*acc;  v += bias[c] (bias[c % bias_mod] if bias_mod > 0);  v *= act'(pre[r*ld_pre + c]) (pre f32/bf16);  v *= dropout(drop_seed, r*N+c, drop_p);
 *   v += resid[r*ld_resid + c] (resid f32/bf16);  v += beta * C_old (C must be f32 when beta != 0);  C[r*ldc + c] = v (c_dtype)
 *   C2 (c2_mode): 1 = act(v), 2 = v, 3 = v * dropout(drop2_seed, r*N+c, drop2_p); stored as c2_dtype;
 *   c2_mode 4: C = act(v) and C2 = act'(v) instead (from one exponential: the backward multiplies by the saved
 *   derivative, act = AW_ACT_DERIV, rather than evaluating act' of a saved pre-activation)
 *   colstats (f64, 2*stats_mod): += v and v*v into slot (c % stats_mod)      (BatchNorm batch statistics; the
 *   specialised bias + bias_mod + colstats epilogues sum the f32 v in f64 throughout -- no f32 summation order, so any
 *   row grouping gives the same sums to f64 rounding --, the generic kernel sums f32 partials of a tile's rows)
 *   a_rowsum (f32, M): += sum_k A[m][k]                                      (bias gradients, fused)
 */
typedef struct {
  int M, N, K;
  int a_dtype;
  const void* A; int64_t lda; int a_trans;
  const void* B; int64_t ldb; int b_trans;
  int conv_cin, conv_seg, conv_dir, conv_operand;
  float alpha, beta;
  const float* bias;
  int act;                       /* AW_ACT_GELU_ERF / _TANH (act' and C2 modes 1, 4) or AW_ACT_DERIV (pre = act') */
  const float* pre; int64_t ld_pre;
  const float* resid; int64_t ld_resid;
  float drop_p; uint64_t drop_seed;
  void* C; int64_t ldc; int c_dtype;
  void* C2; int64_t ldc2; int c2_mode; int c2_dtype;
  float drop2_p; uint64_t drop2_seed;
  double* colstats; int stats_mod;
  float* a_rowsum;
  int bias_mod;                  /* > 0: bias index is c % bias_mod (ConvT bias shared by the k taps) */
  /* accumulate = 1: C[r*ldc + colmap(c)] += alpha*acc with f32 atomics (split-K allowed; no other epilogue
   * field may be set).  colmap(c) = (c % col_mod)*col_mul + c/col_mod + col_off  (col_mod > 0)
   *                              =  c*col_mul + col_off                          (col_mod == 0)
   * so weight gradients land directly in the reference layouts (conv (O,I,3) taps, ConvT (I,O,k)). */
  int accumulate, col_mod, col_mul, col_off;
  /* seed_ptr != NULL: the dropout seeds become mix(drop_seed, *seed_ptr) and mix(drop2_seed, *seed_ptr), with
   * *seed_ptr read on the device (a per-step counter, so one captured HIP graph replays with fresh masks). */
  const uint64_t* seed_ptr;
  /* dtype of `pre` (AW_F32 or AW_BF16): bf16-mode forwards keep the GELU pre-activations in the operand dtype */
  int pre_dtype;
  /* epilogue store policy for C / C2: AW_STORE_NT (0, non-temporal; the lines stay in the XCD's L2 until the
   * end-of-kernel release writes them back) or AW_STORE_WT (1, write-through: the lines leave L2 at once, so the
   * next dependent launch does not wait for that write-back; the VQ-VAE step's GEMM chain, +3 % per step). */
  int store_policy;
  /* dtype of `resid` (AW_F32 or AW_BF16): the bf16-mode VQ-VAE keeps its ResBlock residual streams (activations and
   * their gradients) in bf16, as autocast would (model/vq_vae_patch_embedd.py:73-74 under bf16 autocast) */
  int resid_dtype;
} aw_gemm_args;
#define AW_STORE_NT 0
#define AW_STORE_WT 1

int aw_gemm(const aw_gemm_args* args, void* stream);
/* Same, with a caller-provided f32 workspace: when the shape is split over K (small M*N, long K: the weight
 * gradients), partial products go to plain-store slabs in `ws` and one reduce pass writes C (no atomics).
 * aw_gemm_workspace returns the number of f32 elements needed (0: no split). */
int64_t aw_gemm_workspace(const aw_gemm_args* args);
int aw_gemm_ws(const aw_gemm_args* args, float* ws, int64_t ws_elems, void* stream);
/* Grouped launch of n <= AW_GEMM_MAX_GROUPS accumulate-mode problems (weight gradients) that share every field
 * except A, B, C and a_rowsum: one kernel over all groups' tiles.  The backward defers the weight gradients of
 * the ResBlock stack and issues them as one launch per layer kind (model/vq_vae_patch_embedd.py:60-74 grads;
 * model/transformer_block.py:30,32,78-79 grads), so each tile runs the full token reduction without split-K. */
#define AW_GEMM_MAX_GROUPS 16
int aw_gemm_grouped(const aw_gemm_args* args, int n, void* stream);
/* Tile policy knob: 0 = automatic (256x128 tiles for bf16 launches that fill the chip, else 128x128), 128 or 256 =
 * force that tile for every eligible launch (bf16, non-ragged) -- used by the tests to cover both pipelines. */
int aw_gemm_set_tile(int bm);
/* Which instantiation aw_gemm would launch for these args: no launch, no device call (the operand pointers are only
 * tested for NULL and alignment).  layout: 0 NN, 1 NN + implicit conv, 2 NT, 3 NT + implicit conv, 4 TN, 5 TT,
 * 6 TT + implicit conv on B (N = a_trans b_trans); epi: the epilogue code of the launch (the EpiBits of
 * csrc/gemm_core.h; 1 << 31 = the generic body that reads every field at run time, 1 << 14 = accumulate / split-K);
 * tile_rows: 128 or 256 (aw_gemm_set_tile applies); specialised: 1 when a compiled specialisation exists for
 * (dtype, layout, tile, epi), 0 when the launch takes the generic body; ragged: an operand extent that is not whole
 * 16-B chunks (register staging); splits: split-K slices.  Any output pointer may be NULL.  M == 0 or N == 0 (no
 * launch) reports tile_rows = 0, splits = 0, the generic code.  Returns AW_OK or the status aw_gemm would return. */
int aw_gemm_describe(const aw_gemm_args* args, int* layout, uint32_t* epi, int* tile_rows, int* specialised,
                     int* ragged, int* splits);
/* Weight-gradient kernel policy for the grouped decoder k = 3 launches (model/vq_vae_patch_embedd.py:60-74 grads):
 * 0 = automatic (the 8-wave ping-pong kernel when the shape qualifies and fills the chip), 1 = force it whenever the
 * shape qualifies, -1 = always the generic grouped GEMM (tests, A/B). */
int aw_gemm_set_wgrad_policy(int mode);
/* Batched weight gradients of plain (1-tap) layers: n <= AW_WGRAD_BATCH_MAX accumulate-mode problems
 *   C_i[m*ldc + colmap(n)] += alpha * sum_k A_i[k*lda + m] * B_i[k*ldb + n],  a_rowsum_i[m] += alpha * sum_k A_i[k*lda + m]
 * with bf16 operands (a_trans = b_trans = 1), f32 C, any M_i / N_i that are multiples of 256, one K (any K: ragged
 * token counts) and one alpha for all problems.  Replaces the weight / bias gradients of the transformer's Linear
 * layers, one launch for the four kinds of all 8 blocks (half of them per launch when a data-parallel step reduces
 * the later half's gradients early) (model/transformer_block.py:28-30,76-77), and of the
 * VQ-VAE encoder's per-token convs (model/vq_vae_patch_embedd.py:65,68 via :108-110).  One stream-K launch (one
 * workgroup per CU, equal work per CU whatever the tile count); tiles split between workgroups are summed through
 * `ws` (aw_wgrad_batch_workspace bytes, 16-B aligned, no initial contents).  One batch at a time per device (the
 * per-tile arrival counters are the library's).  Each tile adds into C with one plain read-modify-write (not
 * atomics, unlike aw_gemm's accumulate mode): the problems' C ranges [C, C + M*ldc) must not overlap (rejected).
 * aw_wgrad_batch_workspace returns -1 when the batch is not eligible. */
#define AW_WGRAD_BATCH_MAX 32
int64_t aw_wgrad_batch_workspace(const aw_gemm_args* args, int n);
int aw_wgrad_batch(const aw_gemm_args* args, int n, void* ws, int64_t ws_bytes, void* stream);
/* Bound of the fix-up's poll for its sibling pieces (default 2^26 polls; a piece that runs out of it poisons its tile
 * with NaN instead of summing unpublished partials).  0 forces that path on every split tile: a test hook, after
 * which the per-tile hand-off counters of this process are stale (tests/test_gpu_kernels.py runs it in a child
 * process). */
int aw_wgrad_set_spin_limit(int polls);

/* Fused ResBlock chain, bf16 operands, H = 512, no BatchNorm: the whole ResBlock stack of the encoder or of the
 * decoder (model/vq_vae_patch_embedd.py:60-74 ResBlock, :103-110 CNNBlock) as ONE persistent launch of N / 64
 * workgroups, each walking a 64-token row block through the 2R convs with its activations resident in LDS; it
 * replaces the 2R aw_gemm launches of either direction.  The forward's operands a1 / a and keep bits are theirs bit for
 * bit; in place of their saved pre-activations h / x it saves GELU'(h) / GELU'(x) (f32 values rounded to bf16), and
 * the backward multiplies by those: its gh / gxo_out track the unfused backward to bf16 rounding.
 *   taps = 1: the encoder (CNNBlock(seperate=True)): every conv sees a length-1 token slice, so it is its centre tap,
 *             a [H][H] contraction per token; weights are [H][H] (packed).
 *   taps = 3: the decoder (CNNBlock(seperate=False)): k = 3, padding 1 convs along windows of seg = 16 consecutive
 *             rows (the rows of one welding window; rows outside the window read as zero, aw_gemm's implicit conv
 *             with conv_seg = 16); weights are [H][3H] with column j*H + i = tap j, input channel i (packed).
 * Forward, per block r (x_0 = x0, a_0 = a0 = GELU(x_0)), conv(W, v)[t] = sum_j W_j v[t + j - 1] (taps = 3) or W v[t]:
 *   h_r = conv(W1_r, a_r) + b1_r,  a1_r = GELU(h_r),  x_{r+1} = x_r + Dropout(conv(W2_r, a1_r) + b2_r; drop_seed[r],
 *   group row*H + c as aw_gemm's epilogue),  a_{r+1} = GELU(x_{r+1}) for r < R-1 and x_R for r = R-1.
 *   Stored: dgelu_h[r] = GELU'(h_r), a1[r] = a1_r, dgelu_x[r] = GELU'(x_{r+1}) (r < R-1), a[r] = a_{r+1} (GELU' of
 *   the f32 values, rounded to bf16: the backward's multipliers, in place of the unfused path's saved h_r / x_{r+1});
 *   dgelu_h / a1 / dgelu_x may be NULL (not stored: eval forwards).  Weights w1 / w2 are the forward copies of aw_res_pack_weights, biases f32.  With drop_p > 0
 *   and drop_masks != NULL the launch also writes the keep bits of every block there (aw_res_dropout_masks_bytes;
 *   the masks aw_res_dropout_masks makes), for the backward.
 * Backward, per block r = R-1 .. 0, from gx = dL/dx_R (bf16) and gxo = gx * mask_{R-1} (bf16), with
 * convT(W, v)[t] = sum_j W_j^T v[t - j + 1] (taps = 3) or W^T v[t]:
 *   gh_r = convT(W2_r, go_r) * GELU'(h_r),  gx_r = gx_{r+1} + convT(W1_r, gh_r) * GELU'(x_r),
 *   gxo_out[r] = gx_r * mask_{r-1} (r > 0: block r-1's conv2 operand) or gx_0 (r = 0); gh[r] = gh_r.
 *   w1t / w2t are the backward copies of aw_res_pack_weights; dgelu_h[r] = the forward's dgelu_h[r], dgelu_x[r] =
 *   the forward's dgelu_x[r-1] (r >= 1; dgelu_x[0] unused), x0 = x_0 (block 0's GELU'(x_0) is evaluated here, the
 *   erf form of aw_gemm's bf16 epilogues); drop_masks (drop_p > 0) = what the forward wrote.
 * All activations are [N][H] bf16 with row stride H, 16-B aligned; N * H * 2 < 2^31; 1 <= R <= AW_RES_CHAIN_MAX;
 * taps = 3 needs seg = 16 and N % 16 == 0.  drop_seed / seed_ptr select the masks (forward); store_policy AW_STORE_WT
 * (sc1) or AW_STORE_NT for every global store.
 * Forward tail (taps = 3 only, tail_k1 = 1 .. AW_RES_TAIL_MAX; all-zero tail fields = no tail): the un-patch
 * ConvTranspose1d(H -> H, kernel = stride = tail_k1) that follows the decoder stack, run on x_R while it is still in
 * LDS: for tap j < tail_k1
 *   tail_y[row][j * H + c] = bf16(x_R[row] . W_j[c] + tail_bias[c])          (tail_y: [N][tail_k1 * H] bf16)
 * with tail_w[j] the forward copy of the [out][in] matrix W_j packed as a taps = 1 matrix (aw_res_pack_weights, job_taps),
 * and tail_colstats (f64, 2 * H, may be NULL) += the column sums of v and v * v over the rows < N and the tail_k1
 * taps, from the f32 values before the bf16 rounding -- what aw_gemm with bias_mod = stats_mod = H computes on
 * a[R-1] and the [tail_k1 * H][H] operand copy, without the launch and without reading x_R back.  a[R-1] is still
 * stored.  (N + 64) * tail_k1 * H * 2 < 2^31; tail_y 16-B aligned.
 * Forward sep tail (taps = 1 only, sep_d = 64; all-zero sep fields = none): the SepCNNBlock conv (H -> sep_d, one tap
 * per token) that follows the encoder stack, run on x_R while it is still in LDS:
 *   sep_z[row][c] = x_R[row] . sep_w[c] + sep_bias[c]                        (sep_z: [N][sep_d] f32, rows < N only)
 * with sep_w the [sep_d][H] bf16 operand copy ([out][in], not packed) and sep_bias f32 -- what aw_gemm computes from
 * a[R-1] with that operand and bias, bit for bit, without the launch and without reading x_R back.  a[R-1] is still
 * stored.  sep_w and sep_z 16-B aligned.
 * Forward head (head_k = 64 with taps = 3, 32 with taps = 1; all-zero head fields = none): the conv that makes x_0 runs
 * in the launch, and x0 / a0 become outputs (either may be NULL: not stored):
 *   x0[row][c] = bf16(v),  a0[row][c] = bf16(GELU(v)),  v = in[row] . head_w[c] + head_bias[c]
 * -- what aw_gemm with c2_mode = 1 writes from the same operands, bit for bit.  head_w: the [H][head_k] bf16 operand
 * copy ([out][in], not packed), head_bias f32.
 *   taps = 3: the decoder's 1x1 conv; in = head_in, the [N][64] bf16 quantized rows.
 *   taps = 1: patchify + the patch embed; head_in = the f32 windows [N / S][head_L][head_C], S = head_L head_C /
 *             head_P tokens per window, in[row] = the row aw_patchify makes (head_P <= 32 elements, zero-padded to
 *             32), also stored to head_patches ([N][32] bf16, 8-B aligned, may be NULL).
 * head_w and (taps = 3) head_in 16-B aligned. */
#define AW_RES_CHAIN_MAX 16
#define AW_RES_TAIL_MAX 8
typedef struct {
  int64_t N;
  int H, R;
  int taps, seg;
  const void* a0;
  const void* x0;
  const void* w1[AW_RES_CHAIN_MAX];
  const void* w2[AW_RES_CHAIN_MAX];
  const float* b1[AW_RES_CHAIN_MAX];
  const float* b2[AW_RES_CHAIN_MAX];
  void* dgelu_h[AW_RES_CHAIN_MAX];
  void* a1[AW_RES_CHAIN_MAX];
  void* dgelu_x[AW_RES_CHAIN_MAX];
  void* a[AW_RES_CHAIN_MAX];
  float drop_p;
  uint64_t drop_seed[AW_RES_CHAIN_MAX];
  const uint64_t* seed_ptr;
  int store_policy;
  uint64_t* drop_masks;
  int tail_k1;
  const void* tail_w[AW_RES_TAIL_MAX];
  const float* tail_bias;
  void* tail_y;
  double* tail_colstats;
  int sep_d;
  const void* sep_w;
  const float* sep_bias;
  float* sep_z;
  int head_k;
  const void* head_in;
  const void* head_w;
  const float* head_bias;
  void* head_patches;
  int head_L, head_C, head_P;
} aw_res_chain_fwd_args;
typedef struct {
  int64_t N;
  int H, R;
  int taps, seg;
  const void* gx;
  const void* gxo;
  const void* x0;
  const void* w1t[AW_RES_CHAIN_MAX];
  const void* w2t[AW_RES_CHAIN_MAX];
  const void* dgelu_h[AW_RES_CHAIN_MAX];
  const void* dgelu_x[AW_RES_CHAIN_MAX];
  void* gh[AW_RES_CHAIN_MAX];
  void* gxo_out[AW_RES_CHAIN_MAX];
  float drop_p;
  int store_policy;
  const uint64_t* drop_masks;
} aw_res_chain_bwd_args;
int aw_res_chain_fwd(const aw_res_chain_fwd_args* args, void* stream);
int aw_res_chain_bwd(const aw_res_chain_bwd_args* args, void* stream);
/* The chain's dropout keep bits for R blocks at N tokens: aw_res_dropout_masks_bytes(N, R) bytes (16-B aligned), one
 * 64-bit word per chain thread and block (block r's mask: the keep decision of aw_gemm's dropout epilogue with seed
 * drop_seed[r] mixed with *seed_ptr, on element row * 512 + c).  aw_res_chain_fwd writes the same words itself;
 * this standalone form serves a backward without a chain forward (and the tests). */
int64_t aw_res_dropout_masks_bytes(int64_t N, int R);
int aw_res_dropout_masks(int64_t N, int R, float drop_p, const uint64_t* drop_seed, const uint64_t* seed_ptr,
                         void* masks, void* stream);
/* Fragment-packed weight copies of the chain: n <= AW_RES_PACK_MAX bf16 matrices src[i] = W of shape
 * [512][taps * 512] ([out][(tap, in)], the forward operand layout; taps 1 or 3).  fwd[i] packs A = W, bwd[i] packs
 * the backward operand A[i][(j, o)] = W[o][j * 512 + i] (W^T for taps = 1); either may be NULL.  Packed layout of a
 * [512][K] A (row m, column k): the 1-KB block (m / 16, k / 32) at byte ((m / 16) * (K / 32) + k / 32) * 1024 holds
 * lane l = (m % 16) + 16 ((k % 32) / 8) at 16 l, element k % 8 within -- one MFMA A-fragment, so a wave reads each
 * fragment as one contiguous KB.
 * job_taps (NULL: every job has `taps`) gives a tap count per job, `taps` or 1.  A 1-tap job packs a [512][512] matrix,
 * forward copy only, beside the launch's [512][taps * 512] ones -- the chain tail's matrices ride in the decoder's
 * forward pack launch. */
#define AW_RES_PACK_MAX 32
int aw_res_pack_weights(const void* const* src, void* const* fwd, void* const* bwd, const int* job_taps, int n,
                        int taps, void* stream);

/* -------------------------------------------------------------------------------- vector quantizer
 * VectorQuantizer.forward (model/vector_quantizer.py:76-119), fp32, codebook staged in LDS, no MFMA:
 *   dist = fl(fl(|z|^2 + |e_k|^2) - 2 * (k-ordered fmaf chain z.e_k)), argmin with first-index ties,
 *   z_q_ste = z + (e_idx - z), idx (int64), counts[k] += 1, sqerr[0] += sum (e_idx - z)^2 (f64).
 * sqerr (1 double) must be zero on entry.  D in {16,32,64,128,256}.
 * counts: count_groups (1..AW_VQ_COUNT_GROUPS_MAX) partial histograms of K floats each, zero on entry; workgroup b adds
 * into partial b % count_groups, so the adds into any one address are count_groups times fewer (they serialise at the
 * memory-side atomic units).  The partials sum to the counts; aw_vq_finalize takes them as they are.
 * zq_copy (NULL = none; 16-B aligned, copy_dtype AW_BF16 or AW_F32) also receives z_q_ste: the GEMM operand of the
 * decoder's first conv, without a separate cast launch.
 */
#define AW_VQ_COUNT_GROUPS_MAX 64
int aw_vq_forward(const float* z, const float* E, int64_t N, int K, int D, float* zq, int64_t* idx, float* counts,
                  int count_groups, double* sqerr, void* zq_copy, int copy_dtype, void* stream);
/* loss = m + beta*m with m = sqerr/(N*D) (vector_quantizer.py:107-108); perplexity = exp(-sum p log(p+1e-10)),
 * p = counts/N (:114-115), counts = the count_groups partial histograms of aw_vq_forward summed per code in a fixed
 * order.  Each output is one f32 device scalar. */
int aw_vq_finalize(const float* counts, int count_groups, const double* sqerr, int64_t N, int K, int D, float beta,
                   float* loss, float* perplexity, void* stream);
/* Backward of the STE + loss: dz = g_zq + g_loss*2(z - z_q)/(N*D);  dE[idx] += g_loss*2*beta*(z_q - z)/(N*D).
 * g_zq may be NULL (treated as 0); g_loss is a device scalar.  dE is accumulated (not overwritten).
 * dz_copy (NULL = none; copy_dtype AW_BF16 or AW_F32) also receives dz: the operand of the SepCNN backward GEMMs. */
int aw_vq_backward(const float* z, const float* E, const int64_t* idx, const float* g_zq, const float* g_loss,
                   int64_t N, int K, int D, float beta, float* dz, float* dE, void* dz_copy, int copy_dtype,
                   void* stream);
/* ------------------------------------------------------------------ residual VQ with EMA codebooks (csrc/rvq.hip)
 * ResidualVQLightning (model/vector_quantizer.py:9-56) wraps vector-quantize-pytorch's ResidualVQ (third-party, not
 * installed here: its published algorithm is restated, parity unpinned).  Per layer i: aw_vq_forward on residual r_i
 * (counts = the EMA's bins, sqerr -> commitment loss via aw_vq_finalize with beta 0), then these:
 * sums[idx[n]][:] += z[n][:] (accumulated; zero on entry), f32, D % 4 == 0 (vector_quantizer.py:20-21 ema update). */
int aw_vq_cluster_sums(const float* z, const int64_t* idx, int64_t N, int K, int D, float* sums, void* stream);
/* One Lloyd step of the k-means init: means[k] = sums[k] / counts[k] where counts[k] > 0 (else unchanged);
 * avg (may be NULL) = the new means * counts (the init's embed_avg, written on the last step). */
int aw_kmeans_update(float* means, const float* sums, const float* counts, int K, int D, float* avg, void* stream);
/* EMA codebook update + dead-code replacement, in place (EuclideanCodebook training branch):
 *   cs = decay cs + (1-decay) counts;  avg = decay avg + (1-decay) sums;
 *   embed = avg / ((cs + eps) / (sum cs + K eps) * sum cs);
 *   codes with cs < threshold (threshold > 0) take a batch row z[r]: embed = z[r], avg = threshold z[r], cs = threshold.
 * Rows: the expired code of rank j (of n) draws uniformly from the j-th of n equal strata of the N rows (distinct rows),
 * hash seed mix(salt, *seed_ptr) (seed_ptr may be NULL).  ws: 2K floats of scratch. */
int aw_rvq_ema_update(float* embed, float* embed_avg, float* cluster_size, const float* counts, const float* sums,
                      const float* z, int64_t N, int K, int D, float decay, float eps, float threshold, uint64_t salt,
                      const uint64_t* seed_ptr, float* ws, void* stream);
/* out = (first ? 0 : out) + zq;  r_next = r - zq (r_next may be NULL).  n elements. */
int aw_rvq_residual(const float* r, const float* zq, int64_t n, float* out, int first, float* r_next, void* stream);
/* Backward of the stack: dz = nq * g_zq + sum_i g_loss[i] * commitment * 2 (res_i - q_i) / (N D);
 * res, q: (nq, N, D) -- each layer's input residual and its straight-through output; g_zq may be NULL. */
int aw_rvq_backward(const float* res, const float* q, const float* g_zq, const float* g_loss, int nq, int64_t N,
                    int D, float commitment, float* dz, void* stream);

/* min_encodings one-hot (N,K) f32 (vector_quantizer.py:98-100). */
int aw_vq_onehot(const int64_t* idx, int64_t N, int K, float* onehot, void* stream);
/* Gather E[idx] -> out (N, D) (get_embedding_from_one_hot, vector_quantizer.py:121-131). */
int aw_vq_gather(const float* E, const int64_t* idx, int64_t N, int D, float* out, void* stream);

/* --------------------------------------------------------------------------- VQ-VAE layout kernels
 * Patchify (model/vq_vae_patch_embedd.py:13-17): x (B, L, C) -> patches (B*S, ldp) with token t covering the
 * channel-major flat window [t*P, (t+1)*P); columns P..ldp-1 are zero.  S = L*C/P. */
int aw_patchify(const float* x, int64_t B, int L, int C, int P, void* patches, int64_t ldp, int dtype,
                void* stream);
/* Weight relayouts (+cast) for the GEMM operand forms; out dtype = `dtype`.
 * mode 0: conv (O,I,k) tap t -> [O][I]                        (centre tap of the per-token encoder convs)
 * mode 1: conv (O,I,3)     -> [O][3*I], col j*I+i              (decoder conv forward, b_trans=0)
 * mode 2: conv (O,I,3)     -> [3*O][I], row j*O+o = W[o][:,j]  (decoder conv input-gradient, b_trans=1)
 * mode 3: convT (I,O,k)    -> [k*O][I], row j*O+o              (un-patch ConvT forward b_trans=0 / dgrad b_trans=1)
 * mode 4: conv (O,I,k)     -> [O][ldo] zero padded, col i*k+j  (patch embed, 1 input channel)
 * `ldo` is the output row length (ignored except for mode 4).  Batched form only:
 * mode 5: plain cast of O*I elements;
 * (mode 6 is retired: it fed the round-2 fused encoder chain, deleted in round 3);
 * mode 7: conv stored tap-major (O,3,I) -> [3*O][I], row j*O+o (decoder conv input-gradient when the optimizer keeps
 *         the weight tap-major; the forward copy [O][3*I] of such a weight is mode 5 over O x 3I). */
int aw_weight_relayout(const float* W, int O, int I, int k, int tap, int mode, void* out, int64_t ldo,
                       int dtype, void* stream);
/* Batched form: up to AW_RELAYOUT_MAX_JOBS relayouts (modes 0-7 above; mode 5 casts e.g. the Linear weights of
 * model/transformer_block.py) into one output dtype, one launch per call. */
#define AW_RELAYOUT_MAX_JOBS 40
typedef struct {
  const float* W;
  void* out;
  int O, I, k, tap, mode;
  int64_t ldo;
} aw_relayout_job;
int aw_weight_relayout_batch(const aw_relayout_job* jobs, int n, int dtype, void* stream);
/* Inverse relayout of weight GRADIENTS, accumulated (+=) into the reference-layout gradient:
 * mode 0: g[O][I] -> G[o][i][tap];  mode 1: g[O][3I] -> G[o][i][j];  mode 3: g[kO][I] -> G[i][o][j];
 * mode 4: g[O][ldo] -> G[o][0][j]. */
int aw_weight_grad_scatter(const float* g, int O, int I, int k, int tap, int mode, int64_t ldg, float* G,
                           void* stream);
/* Elementwise cast/copy: out[i] = in[i] (f32 -> dtype). */
int aw_cast(const float* in, int64_t n, void* out, int dtype, void* stream);

/* Un-patch head forward (vq_vae_patch_embedd.py:27-30,52-57):
 * y (R = B*Q rows of H, y_dtype, BN input) -> BN(stats) -> GELU(erf) -> ConvT(H->1, k5, s5) -> x_hat (B, 200, 2)
 * interleaved (flat position 5q+j of window b).  stats (f32 4*H): mean, invstd, gamma, beta (aw_bn_finalize).
 * y_dtype, here and in the two backward passes: AW_F32, or AW_BF16 when H is a power of two in 64..2048 -- the bf16
 * operand mode stores the ConvT output in bf16, halving the head's three HBM passes over it; the BN statistics still
 * come from the f32 values in the ConvT epilogue. */
int aw_unpatch_head_fwd(const void* y, int y_dtype, int64_t R, int H, int Q, const float* stats, const float* w2,
                        const float* b2, float* x_hat, void* stream);
/* BatchNorm finalize: colstats (f64 sum, sumsq over n rows) -> stats {mean, invstd, gamma, beta};
 * training: running_mean/var momentum update (unbiased var), *nbt += 1.  eval (training == 0): uses running. */
int aw_bn_finalize(const double* colstats, int64_t n, int H, const float* gamma, const float* beta,
                   float* running_mean, float* running_var, int64_t* nbt, float eps, float momentum,
                   int training, float* stats, void* stream);
/* Un-patch head backward from g_xhat (same layout as x_hat).
 * pass 1: per-channel sums sum_g, sum_g*xhat (f64 2H, zero on entry); grads of w2 (H*5), b2 (1), gamma, beta
 *         accumulated (+=).
 * pass 2: g_y (R x H, gy_dtype) = BatchNorm backward (batch stats if training, else running) of g*gelu'(.),
 *         db_y (H f32, +=) = channel sums of g_y (gradient of the ConvT bias feeding the BN). */
int aw_unpatch_head_bwd1(const void* y, int y_dtype, int64_t R, int H, int Q, const float* stats, const float* w2,
                         const float* g_xhat, double* gsums, float* gw2, float* gb2, float* ggamma, float* gbeta,
                         void* stream);
int aw_unpatch_head_bwd2(const void* y, int y_dtype, int64_t R, int H, int Q, const float* stats, const float* w2,
                         const float* g_xhat, const double* gsums, int training, void* g_y, int gy_dtype, float* db_y,
                         void* stream);
/* Fused training-step form of the head forward and pass 1 (train_reconstruction_embedding.py's step: loss =
 * mse(x_hat, x) + embedding loss, autencoder_lightning_base.py:80-97; vq_vae_patch_embedd.py:27-30,52-57), H == 512:
 * one read of y computes x_hat (as aw_unpatch_head_fwd), g_xhat = (2 / (R*5)) * gscale[0] * (x_hat - x) (as
 * aw_mse_bwd), sqerr (f64, +=) = sum (x_hat - x)^2 (as aw_mse_fwd), and pass 1 of the backward from that g_xhat
 * (as aw_unpatch_head_bwd1: gsums, gw2, gb2, ggamma, gbeta).  x: the input windows, same layout as x_hat. */
int aw_unpatch_head_fwd_bwd1(const void* y, int y_dtype, int64_t R, int H, int Q, const float* stats, const float* w2,
                             const float* b2, const float* x, const float* gscale, float* x_hat, float* g_xhat,
                             double* sqerr, double* gsums, float* gw2, float* gb2, float* ggamma, float* gbeta,
                             void* stream);
/* BatchNorm1d of the `--batchnorm 1` ResBlocks (model/vq_vae_patch_embedd.py:60-74).  Activations h are
 * [N rows][H channels] f32; statistics are per (group, channel), group = row % G (decoder G = 1; encoder G = S
 * token positions, each its own batch of B rows: CNNBlock(seperate=True) runs the blocks per token slice).
 * stats sums: double [2][G][H] (sum, sum of squares), zero on entry.
 * finalize: stats f32 [4][G][H] = mean, invstd, gamma, beta; training: batch statistics (biased variance) and
 *   the running statistics moved once per group in group order (unbiased variance, momentum), *nbt += G;
 *   eval: the running statistics for every group.
 * apply: mode 0: out = BN(h), op = GELU(out); mode 1: out = resid + dropout(BN(h)) (mask of element r*H + c
 *   from aw_seed_mix(drop_seed, seed_ptr), as the GEMM epilogues), op = GELU(out) or NULL; mode 2: as mode 1
 *   with op = out (no GELU).  op in op_dtype.
 * bwd_reduce: t = g_in * dropout mask; sums [2][G][H] += (sum t, sum t * xhat), zero on entry.
 * bwd_apply: dh (dh_dtype) = gamma*invstd*(t - S1/n - xhat*S2/n) (training) or gamma*invstd*t (eval);
 *   dgamma += sum_g S2, dbeta += sum_g S1 (either may be NULL).  n = rows per group. */
int aw_bn_group_stats(const float* h, int64_t N, int H, int G, double* sums, void* stream);
int aw_bn_group_finalize(const double* sums, int64_t n, int H, int G, const float* gamma, const float* beta,
                         float* running_mean, float* running_var, int64_t* nbt, float eps, float momentum,
                         int training, float* stats, void* stream);
int aw_bn_apply(const float* h, int64_t N, int H, int G, const float* stats, int mode, const float* resid,
                float drop_p, uint64_t drop_seed, const uint64_t* seed_ptr, float* out, void* op, int op_dtype,
                void* stream);
int aw_bn_bwd_reduce(const float* h, int64_t N, int H, int G, const float* stats, const float* g_in, float drop_p,
                     uint64_t drop_seed, const uint64_t* seed_ptr, double* sums, void* stream);
int aw_bn_bwd_apply(const float* h, int64_t N, int H, int G, const float* stats, const float* g_in, float drop_p,
                    uint64_t drop_seed, const uint64_t* seed_ptr, const double* sums, int64_t n, int training,
                    void* dh, int dh_dtype, float* dgamma, float* dbeta, void* stream);
/* Mean-squared error (F.mse_loss, autencoder_lightning_base.py:82): sqerr[0] (f64, zero on entry) += sum (a-b)^2;
 * backward: ga = 2(a-b)/n * g (device scalar g). */
int aw_mse_fwd(const float* a, const float* b, int64_t n, double* sqerr, void* stream);
int aw_mse_bwd(const float* a, const float* b, int64_t n, const float* g, float* ga, void* stream);

/* loss = a[0] + b[0] (both device scalars) -> out[0]; also used for the autograd scalar plumbing. */
int aw_scalar_add(const float* a, const float* b, float* out, void* stream);
/* recon = sqerr/numel as f32 -> out */
int aw_mse_finalize(const double* sqerr, int64_t numel, float* out, void* stream);
/* out = sqerr / numel and sum = out + addend in one launch (the training step's recon error and total loss,
 * autencoder_lightning_base.py:80-97: loss = recon_error + embedding_loss). */
int aw_mse_finalize_add(const double* sqerr, int64_t numel, const float* addend, float* out, float* sum, void* stream);

/* ------------------------------------------------------------------------------------- optimizer
 * Multi-tensor RAdam over one flat parameter buffer (torch.optim.RAdam semantics, L2 weight decay):
 * segments [seg_off[s], seg_off[s]+seg_len[s]) (sorted, within [0,total)) with weight decay seg_wd[s]; seg_active[s]==0
 * are skipped (grad None: model/transformer_decoder.py heads under find_unused_parameters).  The buffers are 16-B
 * aligned, total % 4 == 0 and every segment starts 16-B aligned; the padding after a segment (up to the next
 * multiple of 4 elements) must be zero in all four buffers and stays zero (same for aw_grad_norm_clip's grad).
 * Nothing outside those float4s is read or written: the elements before the first segment, the gaps between
 * segments and inactive segments may hold anything.
 * scalars come from host (step count, lr, betas, eps); `gscale` is a device scalar multiplying the gradient
 * first (clip coefficient; NULL = 1).  With step_ptr != NULL the step number is read from the device (the host `step`
 * is ignored) and the bias corrections and rectification are derived there, in double precision like torch's
 * python-float scalars.
 * zero_grad != 0: the gradient of every updated element is zeroed after use (optimizer.zero_grad() fused into the
 * update; inactive segments are left as they are).
 * ops != NULL (total < 2^31): the update also writes the operand copies of the updated weights (what
 * aw_weight_relayout_batch would produce from the new values), so the training step needs no relayout launch.  ops:
 * device array of AW_OPS_PER_SEG descriptors per segment (ops[AW_OPS_PER_SEG*s + j]; mode -1 = none): flat element l
 * of segment s (the parameter in its storage order: (O, I, k) contiguous; a declare_centre_tap segment is its [O][I]
 * centre, described as k = 1, tap = 0) goes to `out` at the index of relayout mode `mode` (0-7), cast to `dtype`. */
#define AW_OPS_PER_SEG 2
typedef struct {
  void* out;
  int O, I, k, tap, mode, dtype;
  int64_t ldo;
} aw_operand_desc;
int aw_radam_step(float* param, float* grad, float* exp_avg, float* exp_avg_sq, const int64_t* seg_off,
                  const int64_t* seg_len, const float* seg_wd, const int* seg_active, int nseg, int64_t total, int64_t step,
                  float lr, float beta1, float beta2, float eps, const float* gscale, const int64_t* step_ptr,
                  const aw_operand_desc* ops, int zero_grad, void* stream);
/* Device step counter / RNG counter: *counter += v (graph-capture safe).  snapshot (may be NULL) also receives the new
 * value (the per-forward dropout seed the backward re-reads).  zero (may be NULL; needs snapshot) names a block
 * zero[0 .. nzero) of f64 accumulators that the same launch zeroes (a forward's accumulator block). */
int aw_counter_add(int64_t* counter, int64_t v, int64_t* snapshot, double* zero, int64_t nzero, void* stream);
/* Global L2 norm of the active segments of `grad` -> out_norm (f32 device scalar) and the clip coefficient
 * min(max_norm/(norm+1e-6), 1) -> out_coef (Lightning gradient_clip_val -> clip_grad_norm_).
 * ws: f64[AW_NORM_WS] scratch (per-workgroup partial sums, reduced in a fixed order: the norm is deterministic). */
#define AW_NORM_WS 1024
int aw_grad_norm_clip(const float* grad, const int64_t* seg_off, const int64_t* seg_len, const int* seg_active,
                      int nseg, int64_t total, float max_norm, double* ws, float* out_norm, float* out_coef,
                      void* stream);
/* x[i] *= s (device scalar), over n elements. */
int aw_scale(float* x, int64_t n, const float* s, void* stream);

/* ------------------------------------------------------------------------------------ transformer
 * LayerNorm (model/transformer_block.py:71,73; transformer_decoder.py:28), eps, over the last dim D.
 * y = (x-mean)*rstd*w + b (y_dtype); mean/rstd saved (f32, R each). */
int aw_layernorm_fwd(const float* x, int64_t R, int D, const float* w, const float* b, float eps, void* y,
                     int y_dtype, float* mean, float* rstd, void* stream);
/* dx (+= if accumulate) and dw/db (accumulated, f32).  Optional second output dx2 (dx2_dtype) = the final dx
 * times the dropout mask (drop_seed, r*D + c, drop_p) of the residual branch that produced x -- the operand of
 * the preceding block's output-projection gradients (mask regenerated, never stored). */
int aw_layernorm_bwd(const float* x, const float* dy, int64_t R, int D, const float* w, const float* mean,
                     const float* rstd, float* dx, int accumulate, float* dw, float* db, void* dx2, int dx2_dtype,
                     float drop_p, uint64_t drop_seed, const uint64_t* seed_ptr, void* stream);
/* Classification head (transformer_decoder.py:126-129): s[r] = xf[r].w1 (+b1), g = GELU_erf(s),
 * out[b][c] = sum_t g[b*T+t] W2[c][t] (+b2[c]).  b1/b2 may be NULL (class_h_bias=False). */
int aw_class_head_fwd(const float* xf, int64_t B, int T, int D, const float* w1, const float* b1, const float* W2,
                      const float* b2, float* s, float* out, void* stream);
/* Backward: dxf (R x D, written), dw1 (D), db1 (1), dW2 (2 x T), db2 (2) accumulated (+=); NULL grads skipped. */
int aw_class_head_bwd(const float* xf, const float* s, const float* dout, int64_t B, int T, int D, const float* w1,
                      const float* W2, float* dxf, float* dw1, float* db1, float* dW2, float* db2, void* stream);
/* Token embedding + sinusoidal PE (model/embedding.py:57-59): x[b,t,:] = Wtok[ids[b,t]] + pe[t] */
int aw_embed_fwd(const int64_t* ids, int64_t B, int T, int D, const float* wtok, const float* pe, float* x,
                 void* stream);
/* aw_embed_fwd followed by aw_layernorm_fwd(x, B*T, D, w, b, eps, y, y_dtype, mean, rstd) in one launch, bit-identical
   to the pair (the first block's ln_1, model/transformer_block.py:84); D = 256, 512, 768 or 1024, 16-B aligned rows */
int aw_embed_ln_fwd(const int64_t* ids, int64_t B, int T, int D, const float* wtok, const float* pe, float* x,
                    const float* w, const float* b, float eps, void* y, int y_dtype, float* mean, float* rstd,
                    void* stream);
int aw_embed_bwd(const int64_t* ids, int64_t B, int T, int D, const float* dx, float* dwtok, void* stream);
/* aw_embed_bwd for a table of V rows without global atomics: a counting sort of the rows by id, then one owner per
   table element (ids outside [0, V) are skipped).  work: V + 1 + B*T ints of device scratch.  Falls back to
   aw_embed_bwd when V > 15360, D is not 256 / 512 / 768 / 1024 or dx / dwtok are not 16-B aligned. */
int aw_embed_bwd_sorted(const int64_t* ids, int64_t B, int T, int D, int V, const float* dx, float* dwtok, int* work,
                        void* stream);
/* Its two halves, for a caller that sorts early (the ids are known at the forward): aw_embed_sort fills work (V + 1 + R ints; V <= 15360) from the R ids,
   aw_embed_bwd_segsum adds the rows of dx (R x D, D = 256/512/768/1024, 16-B aligned) into dwtok from it. */
int aw_embed_sort(const int64_t* ids, int64_t R, int V, int* work, void* stream);
int aw_embed_bwd_segsum(const int* work, int V, int D, const float* dx, float* dwtok, void* stream);
/* Causal self-attention core (model/transformer_block.py:44-60) on the packed qkv projection
 * (B*T, 3*d, dtype), heads of hs = d/n_head: y (B*T, d, dtype) = softmax(q k^T / sqrt(hs), causal) v;
 * lse (B*n_head*T f32) saved for the backward (flash-style, T x T never materialised).
 * Attention-probability dropout (CausalSelfAttention.attn_dropout, transformer_block.py:44-57; the reference default
 * is 0.0): P_ij kept with probability 1 - drop_p and scaled by 1/(1 - drop_p); the mask of element
 * ((b*n_head + h)*T + i)*T + j comes from the counter hash of (drop_seed mixed with *seed_ptr when given), so the
 * backward regenerates the forward's mask.  drop_p = 0: no dropout, drop_seed and seed_ptr are not used. */
int aw_attn_fwd(const void* qkv, int64_t B, int T, int n_head, int d, int dtype, void* y, float* lse, float drop_p,
                uint64_t drop_seed, const uint64_t* seed_ptr, void* stream);
/* dqkv (B*T, 3d, dtype) from dy (B*T, d, dtype), recomputing P from lse; ws: f32 B*n_head*T (delta). */
int aw_attn_bwd(const void* qkv, const void* y, const void* dy, const float* lse, int64_t B, int T, int n_head,
                int d, int dtype, void* dqkv, float* ws, float drop_p, uint64_t drop_seed, const uint64_t* seed_ptr,
                void* stream);
/* KV-cache decode attention (MyTransformerDecoder.generate, model/transformer_decoder.py:203-224):
 * n_new query rows per sequence at absolute positions pos0 .. pos0+n_new-1 (qkv_new (B*n_new, 3d, dtype), row
 * b*n_new + i).  Their K and V are appended to kv_cache (B, Tmax, 2d, dtype; row b*Tmax + t = [K | V]) and
 * y (B*n_new, d, dtype) = softmax(q k^T / sqrt(hs)) v over the cached positions 0 .. pos0+i (causal). */
int aw_attn_decode(const void* qkv_new, int64_t B, int n_new, int pos0, int n_head, int d, int dtype,
                   void* kv_cache, int Tmax, void* y, void* stream);
/* Cross entropy with ignore_index (transformer_decoder.py:226-230): logits (R, V) f32 with row stride ldl;
 * loss_sum (f64, zero on entry) += sum over kept rows of (lse - logit[y]); count (f64) += kept rows.
 * The backward writes dlogits = (softmax - onehot) * g / count (g device scalar) into dlogits (dtype) and zeros
 * into its padding columns V..ldd-1. */
int aw_ce_fwd(const float* logits, int64_t R, int V, int64_t ldl, const int64_t* y, int ignore_index,
              double* loss_sum, double* count, float* lse, void* stream);
int aw_ce_bwd(const float* logits, int64_t R, int V, int64_t ldl, const int64_t* y, int ignore_index,
              const float* lse, const double* count, const float* g, void* dlogits, int64_t ldd, int dtype,
              void* stream);
int aw_ce_finalize(const double* loss_sum, const double* count, float* out, void* stream);

/* ------------------------------------------------------------------------------------------------ GRU recurrence
 * One nn.GRU layer (model/gru.py:25,47; torch gate order r, z, n; W_hh (3H, H), b_hh (3H)):
 *   r = s(gi_r + W_hr h + b_hr)   z = s(gi_z + W_hz h + b_hz)   hn = W_hn h + b_hn
 *   n = tanh(gi_n + r hn)         h' = (1 - z) n + z h                    (gi = W_ih x + b_ih, from aw_gemm)
 * Everything that is not recurrent runs through aw_gemm over all B*T rows (input projection, input gradient, weight
 * gradients).  These entry points are the recurrence: ONE launch per time step, an MFMA GEMM against W_hh
 * whose epilogue finishes the cell.  No workgroup waits on another and nothing is atomic: same inputs, same bits.
 * op_dtype selects the GEMM operands: AW_F32 (exact-f32 MFMA; the f32 buffers themselves are the operands) or
 * AW_BF16 (v_mfma_f32_16x16x32_bf16, f32 accumulation; the kernels write a bf16 copy of what the next GEMM reads).
 * State, saved gates and gradients are f32 in both modes.
 * Padded layout (the kernels' own): Hp = H rounded up to a multiple of 32.  Every row below is Hp wide, or 3*Hp /
 * 4*Hp with gate g at columns [g*Hp, g*Hp + H); rows are contiguous (leading dimension = the row width); columns
 * >= H of every output are written as exact zeros, and inputs must hold zeros there (they do when they come from
 * these kernels, or from an aw_gemm against zero-padded weights and bias).  Every buffer is 16-B aligned.  B is
 * arbitrary (tail rows are guarded).
 * aw_gru_pack_weights: the operand images of W_hh (f32 (3H, H)) as op_dtype, zero-padded:
 *   w_fwd [3][Hp][Hp]: w_fwd[g][j][k] = W_hh[g*H + j][k]        (read by aw_gru_step_fwd)
 *   w_bwd [Hp][3*Hp]:  w_bwd[k][g*Hp + j] = W_hh[g*H + j][k]    (read by aw_gru_step_bwd); either may be NULL. */
int aw_gru_pack_weights(const float* w_hh, int H, int op_dtype, void* w_fwd, void* w_bwd, void* stream);
/* One forward step.  h_prev_op (B, Hp, op_dtype) / h_prev (B, Hp, f32): the previous state as GEMM operand and in
 * f32 (the same buffer in f32 mode); both NULL = zero initial state (GRU.init_hidden, model/gru.py:29-32): no K loop.
 * gi (B, 3*Hp) f32; b_hh (3H, unpadded).  Writes h (B, Hp) f32, h_op (B, Hp) bf16 = h rounded to nearest even (bf16
 * mode; NULL in f32 mode), and saved (B, 4*Hp) f32 = [r | z | n | hn] for the backward. */
int aw_gru_step_fwd(int B, int H, int op_dtype, const void* h_prev_op, const float* h_prev, const void* w_fwd,
                    const float* gi, const float* b_hh, float* h, void* h_op, float* saved, void* stream);
/* One backward step, for time step t:
 *   dh = dgh_next . W_hh + dh_next * z_next + dy        (dgh_next_op (B, 3*Hp, op_dtype), dh_next (B, Hp) and
 *        saved_next (B, 4*Hp) belong to step t+1: all three NULL at the last step, where the GEMM is skipped;
 *        dy (B, Hp) f32 is the gradient from the layer above or the head, NULL = none)
 *   dn = dh (1 - z)(1 - n^2)    dz = dh (h_prev - n) z (1 - z)    dr = dn hn r (1 - r)       (saved = step t's,
 *        h_prev (B, Hp) f32 = h_{t-1}, NULL = zero state)
 * Writes dh (B, Hp), dgi = [dr | dz | dn] and dgh = [dr | dz | dn r] (B, 3*Hp) f32, and their bf16 copies dgi_op /
 * dgh_op (bf16 mode; NULL in f32 mode).  dh may alias dh_next. */
int aw_gru_step_bwd(int B, int H, int op_dtype, const void* dgh_next_op, const float* dh_next,
                    const float* saved_next, const void* w_bwd, const float* dy, const float* saved,
                    const float* h_prev, float* dh, float* dgi, float* dgh, void* dgi_op, void* dgh_op, void* stream);
/* Bias gradients: db[g*H + j] += sum over the rows of dg (rows, 3*Hp) f32 of column g*Hp + j (db_ih from all steps'
 * dgi, db_hh from dgh).  From the f32 gate gradients in both operand modes (aw_gemm's fused a_rowsum would sum the
 * bf16-rounded operand copy); one owner per column and a fixed summation order, so it is deterministic. */
int aw_gru_bias_grad(const float* dg, int64_t rows, int H, float* db, void* stream);

/* ------------------------------------------------------------------------------------------------ generation
 * Ids back to the decoder's input (arcweld.vqvae.decode).  In eval the decoder's 1x1 conv depends on the id alone, so
 * aw_gemm computes y0 = E . Wd0^T + b and GELU(y0) once over the K codebook rows (table_x (K, H, x_dtype), table_a
 * (K, H, a_dtype)) and this launch copies row idx[n] of each table to row n of y0 (N, H, x_dtype) / ya0 (N, H, a_dtype);
 * one wave per row, 16 bytes per access (rows must be whole 16-byte pieces, every buffer 16-B aligned).
 * Every id is range-checked in the kernel: an id outside [0, K) reads nothing, writes a zero row and adds 1 to
 * *bad_count (a device int the caller zeroed).  table_a = ya0 = NULL gathers one table only (H = D over the codebook
 * itself: the K > N route, where the GEMM runs over the N gathered rows instead). */
int aw_vq_decode_gather(const int64_t* idx, int64_t N, const void* table_x, const void* table_a, int K, int H,
                        int x_dtype, int a_dtype, void* y0, void* ya0, int* bad_count, void* stream);
/* The next token of each of B sequences from logits (B, V) f32 (contiguous rows), one workgroup per row with the row
 * in LDS; V <= AW_SAMPLE_MAX_V (a larger V returns AW_ERR_ARG and launches nothing).  Per row, following the
 * reference's loop (model/transformer_decoder.py:203-224) with a column mask and a temperature added:
 *   - only columns < n_valid take part (n_valid = V: all), x = logit * inv_temperature;
 *   - top_k > 0: every x strictly below the top_k-th largest is dropped; ties at the threshold stay (top_k <= n_valid);
 *   - do_sample = 0: the first index of the maximum;
 *   - do_sample = 1: p = softmax of what is left (max-subtracted, f32); the first index whose inclusive prefix sum in
 *     index order exceeds u * total, or the last finite kept column when rounding leaves none, with
 *       u = draw24(seed, c = step * B + row) * 2^-24   in [0, 1),
 *       draw24: key = aw_hash_group(seed, c >> 24); l = (c >> 12) & 0xFFF; r = c & 0xFFF;
 *               4 times, i = 0..3: (l, r) = (r, l ^ (aw_hash_group(key + i, r) >> 52)); return l << 12 | r
 *       aw_hash_group(s, g): z = s + (g + 1) * 0x9E3779B97F4A7C15; z = (z ^ z >> 30) * 0xBF58476D1CE4E5B9;
 *                            z = (z ^ z >> 27) * 0x94D049BB133111EB; return z ^ z >> 31      (64-bit, wrapping)
 *     -- a keyed permutation (4-round Feistel) of the counter's low 24 bits, its round function the counter hash of
 *     the dropout masks: the 2^24 counters that share c >> 24 draw 2^24 different values, so one seed never repeats
 *     a draw within a generation (the hash's plain top 24 bits would: 4096 of them collide with probability 0.39).
 *     u_out (B f32, or NULL) receives u;
 *   - the id goes to ids_out[row * ld_ids + col] (int64);
 *   - a row with a NaN among its columns < n_valid, or whose maximum there is not finite, stores -1 and adds 1 to
 *     *bad_count (a device int the caller zeroed). */
#define AW_SAMPLE_MAX_V 16384
int aw_sample_next(const float* logits, int B, int V, int n_valid, int top_k, float inv_temperature, int do_sample,
                   uint64_t seed, int64_t step, int64_t* ids_out, int64_t ld_ids, int64_t col, float* u_out,
                   int* bad_count, void* stream);
/* aw_sample_next with a nucleus (top-p) and a min-p filter beside top-k, and with the likelihood of the chosen id.
 * The same launch shape (one workgroup per row, the row in LDS, V <= AW_SAMPLE_MAX_V), the same u, and with top_p = 1
 * and min_p = 0 the same ids bit for bit.  Per row, x_j = logit_j * inv_temperature over the columns j < n_valid,
 * xmax their maximum, e_j = expf(x_j - xmax) in f32; the filters run in this order and each sees only the survivors
 * of the one before:
 *   - top_k > 0: as aw_sample_next (ties at the threshold stay);
 *   - min_p in [0, 1), 0 = off: a column survives iff e_j >= min_p, that is p_j >= min_p * p_max whatever the
 *     normalisation (the cut is taken at the smallest x whose e passes, so the survivors are all columns from that x up);
 *   - top_p in (0, 1], 1 = off (no search runs): with total = the sum of e over the survivors and M(t) = the sum of e
 *     over the survivors whose x >= t, the kept set is the survivors with x >= t*, t* the largest x of the row with
 *     M(t*) >= top_p * total (f32 product): the smallest set of most probable columns that reaches the mass, plus every
 *     column tied with its last member (the tie rule of top_k).  total and every M(t) are summed in one fixed order --
 *     thread i adds its columns i, i + 256, ... in that order, a column outside the set adding +0, then a fixed tree
 *     over the 256 threads -- so M(smallest surviving x) == total bit for bit, M is monotone in t, and t* is found by
 *     bisection over the bits of the order-preserving 32-bit key of x below the common prefix of the smallest and the
 *     largest surviving key: at most 32 block sums, no sort, no floating-point atomic, the same t* on every launch;
 *   - do_sample = 0: the first index of the maximum (no filter can remove it); the filters are then evaluated only when
 *     n_kept_out or thr_out asks for their result;
 *   - do_sample = 1: aw_sample_next's walk in index order over the kept columns with the same u.
 * Outputs; u_out, logp_out, logq_out, n_kept_out, thr_out may each be NULL (skipped):
 *   - ids_out[row * ld_ids + col], u_out[row]: as aw_sample_next;
 *   - logp_out[row * ld_lp + col_lp] = l[id] - lse,  lse = mx + log sum_j exp(l[j] - mx) over the RAW logits of the
 *     columns j < n_valid: no temperature, no filter -- aw_score_rows' logp of that id, so generated and measured ids
 *     sit on one scale;
 *   - logq_out[row * ld_lp + col_lp] = log(e_id / sum of e over the kept set), the log-probability of the id under the
 *     distribution it was drawn from; 0 when do_sample = 0;
 *   - n_kept_out[row] (int): the number of columns < n_valid that passed all filters;
 *   - thr_out[row]: the smallest kept x, so the kept set is exactly { j < n_valid : x_j >= thr_out[row] };
 *   - a bad row (aw_sample_next's definition) stores id -1, logp = logq = thr = NaN, n_kept = 0 and adds 1 to *bad_count.
 * AW_ERR_ARG and no launch for aw_sample_next's argument errors, for top_p outside (0, 1] or NaN, min_p outside [0, 1)
 * or NaN, and for ld_lp < 1 or col_lp outside [0, ld_lp) when logp_out or logq_out is given. */
typedef struct {
  const float* logits; int B, V, n_valid;
  int top_k; float top_p, min_p, inv_temperature;
  int do_sample; uint64_t seed; int64_t step;
  int64_t* ids_out; int64_t ld_ids, col;
  float* u_out;
  float* logp_out; float* logq_out; int64_t ld_lp, col_lp;
  int* n_kept_out; float* thr_out;
  int* bad_count;
} aw_sample_args;
int aw_sample_next_ex(const aw_sample_args* args, void* stream);

/* ------------------------------------------------------------------------------------------------ beam search
 * One step of a fixed-length beam search (MyTransformerDecoder.beam_search_ids): B sequences, each with W_in live beams,
 * keep the W_out best of their W_in * n_valid one-token extensions.  One workgroup per sequence, the sequence's whole
 * candidate set in LDS as the order-preserving keys of aw_sample_next.
 *   logits: f32, B * W_in rows of V columns, ldl >= V floats apart; beam w of sequence b is row b * W_in + w.  Only the
 *   columns v < n_valid are candidates (aw_sample_next's restriction).  scores_in: (B, W_in) f32, the beams' running
 *   log-probabilities.  For every candidate (w, v), in f32:
 *     logp = l[w][v] - lse_w,  lse_w = mx_w + logf(sum_{j < n_valid} expf(l[w][j] - mx_w))     (the RAW logits: the
 *            logp of aw_score_rows and of aw_sample_next_ex), the sum in one fixed order;
 *     cand = scores_in[b][w] + logp.
 *   The kept set is the W_out best candidates under ONE total order -- cand descending, ties by the lower flat index
 *   w * n_valid + v -- and slot j of the outputs is the j-th of them:
 *     scores_out[b][j] = cand    parent_out[b][j] = w (int32, in [0, W_in))    token_out[b * W_out + j] = v (int64: the
 *     next step's ids_new as it stands)    logp_out[b][j] = the candidate's own logp.
 *   There is no special case for a dead beam: a score of -inf gives -inf candidates, which sort behind every finite one
 *   and fill the tail by the same tie rule (so does a -inf logit).  When W_out exceeds the W_in * n_valid candidates
 *   that exist, the slots past them hold score = logp = -inf, parent 0, token 0: dead beams for the next step.
 *   The same inputs give the same bits on every launch (no floating-point atomic, fixed summation order).
 * A sequence is bad when the allowed columns of any of its rows hold a NaN or have no finite maximum (aw_sample_next's
 * definition), or when one of its input scores is NaN: all its slots store score = logp = NaN, parent min(j, W_in - 1),
 * token 0, and 1 is added to *bad_count (a device int the caller zeroed).  No id outside [0, n_valid) and no parent
 * outside [0, W_in) is ever stored: the next decode step and aw_beam_gather index with them.
 * AW_ERR_ARG and no launch unless 1 <= W_in <= AW_BEAM_MAX_W, 1 <= W_out <= AW_BEAM_MAX_W, 1 <= n_valid <= V <= ldl and
 * W_in * n_valid <= AW_SAMPLE_MAX_V (the largest LDS image: 32 beams at a 512-code codebook). */
#define AW_BEAM_MAX_W 32
typedef struct {
  const float* logits; int64_t ldl; int B, W_in, W_out, V, n_valid;
  const float* scores_in;
  float* scores_out; int* parent_out; int64_t* token_out; float* logp_out;
  int* bad_count;
} aw_beam_args;
int aw_beam_step(const aw_beam_args* args, void* stream);
/* The key/value caches of all decoder blocks reordered by the surviving beams' parents, in one launch: for every block
 * k < n_blocks, destination row r = b * W_out + j (b < B, j < W_out) and position t < n_pos
 *     dst[k][r, t, :] = src[k][b * W_in + parent[b * W_out + j], t, :]
 * A cache is (rows, Tmax, width) in `dtype` (AW_F32 / AW_BF16), rows [K | V] of width = 2 * d_model: the layout
 * aw_attn_decode defines, so a row's n_pos * width elements are one contiguous chunk.  Positions >= n_pos of dst are
 * not written.  src / dst: DEVICE arrays of n_blocks pointers (built once per search); src[k] and dst[k] are different
 * buffers.  W_in = 1 spreads a prefill cache of B rows over B * W_out rows.  16-byte accesses when a block's two bases,
 * the row pitch and the chunk are all multiples of 16 bytes (decided per block in the kernel), element copies
 * otherwise: any width >= 1.  A parent outside [0, W_in) is never used as an index: its destination chunk is
 * zero-filled and 1 is added to *bad_count (a device int the caller zeroed), once per such parent.
 * AW_ERR_ARG unless 1 <= n_blocks <= 65535, B >= 0, 1 <= W_in, W_out <= AW_BEAM_MAX_W, 0 <= n_pos <= Tmax, width >= 1. */
int aw_beam_gather(const void* const* src, void* const* dst, int n_blocks, int B, int W_in, int W_out,
                   const int* parent, int Tmax, int n_pos, int width, int dtype, int* bad_count, void* stream);
/* The hypotheses of a finished search from its per-step slabs parent (int32), token (int64), logp (f32), each
 * (n_new, B, W) as aw_beam_step wrote them: for b < B, j < R <= W, walking back from final beam j (cur = j; for i =
 * n_new - 1 .. 0: at = (i * B + b) * W + cur, emit, cur = parent[at]):
 *     ids_out[(b * R + j) * ld_ids + col0 + i] = token[at]      logp_out[(b * R + j) * n_new + i] = logp[at]
 * One thread per hypothesis.  A parent outside [0, W) met on the way ends that walk: the steps before it store id 0 and
 * logp NaN, and 1 is added to *bad_count.  n_new >= 0, ld_ids >= col0 + n_new, col0 >= 0. */
int aw_beam_backtrack(const int* parent, const int64_t* token, const float* logp, int n_new, int B, int W, int R,
                      int64_t* ids_out, int64_t ld_ids, int64_t col0, float* logp_out, int* bad_count, void* stream);

/* ------------------------------------------------------------------------------------------------ scoring
 * Teacher-forced scoring of lm-head logits in one launch (MyTransformerDecoder.score_ids, arcweld.generate.score_cycles).
 * logits: f32 rows of V columns, ldl >= V floats apart; the row of position t of sequence b is b * seq_rows + t.
 * Sequence b has `groups` groups of `group_rows` consecutive rows, group c = rows t in [c * group_rows, (c + 1) *
 * group_rows); groups * group_rows <= seq_rows, and the rows past them (the position that predicts the end token) and
 * the columns >= V of a padded row are never read.  targets, logp, rank, entropy: (n_seq, groups * group_rows)
 * compact; group_nll: (n_seq, groups).  For a row with target y, over the allowed columns j < n_valid only (the
 * softmax renormalised over them, the restriction aw_sample_next applies), all in f32:
 *   - logp    = l[y] - lse,  lse = mx + log sum_j exp(l[j] - mx)   (a -inf target logit in a finite row gives -inf);
 *   - rank    = the number of j with l[j] > l[y], or l[j] == l[y] and j < y: 0 means the greedy aw_sample_next picks y;
 *   - entropy = lse - sum_j p_j l[j], evaluated as log(sum e) - sum e (l - mx) / sum e; columns with p_j == 0 add 0;
 *   - group_nll[b, c] = -(sum of the group's logp), summed per wave in row order and then over the waves in order
 *     inside the workgroup that scored the rows: no floating-point atomics, the same bits on every launch.
 * A row is bad when its allowed columns hold a NaN, a +inf or no finite value (as in aw_sample_next: no finite maximum
 * to subtract), or when its target lies outside [0, n_valid) -- checked before it selects anything.  A bad row stores
 * logp = NaN, rank = -1, entropy = NaN, makes its group's group_nll NaN and adds 1 to *bad_count (a device int the
 * caller zeroed; one integer atomic per workgroup at most).
 * One workgroup per (b, c), one wave per row; rows of n_valid <= 1024 are held in registers, wider ones are read
 * twice.  Any V >= 1, 1 <= n_valid <= V, groups >= 1, group_rows >= 1; n_seq * groups < 2^31. */
int aw_score_rows(const float* logits, int64_t ldl, int V, int n_valid, const int64_t* targets, int64_t n_seq,
                  int seq_rows, int groups, int group_rows, float* logp, int* rank, float* entropy, float* group_nll,
                  int* bad_count, void* stream);
/* out[w] = the mean over window w's rows_per_window x width elements of (a[r, c] - b'[r, c])^2, r = w *
 * rows_per_window ..; a: (windows * rows_per_window, width) f32 contiguous.  idx == NULL: b' = b, the same shape.
 * idx (windows * rows_per_window int64): b'[r] = b[idx[r]], b: (n_idx_rows, width) -- the quantisation error of a
 * cycle, encoder rows against their codebook rows.  An idx[r] outside [0, n_idx_rows) is never used as an index: it
 * adds 1 to *bad_count (a device int the caller zeroed) and its window becomes NaN.  One workgroup per window, 16-byte
 * loads when width is a multiple of 4 and a, b are 16-byte aligned, a fixed summation order (no float atomics). */
int aw_window_sqerr(const float* a, const float* b, const int64_t* idx, int64_t n_idx_rows, int64_t windows,
                    int rows_per_window, int width, float* out, int* bad_count, void* stream);

/* ------------------------------------------------------------------------------------------------ ensemble forecasts
 * Pointwise statistics over an ensemble in one launch (arcweld.generate.forecast_cycles), and with a truth the forecast's
 * score against it.  x: (G, N, M) f32 contiguous -- G groups (prompts), N samples, M points each.  Per point (g, m) over
 * its samples x_1..x_N, with x_(1) <= ... <= x_(N) the same values sorted ascending (values move, no bit changes):
 *   - mean[g, m]     = (sum_i x_i) / N, the sum in f64 in index order, rounded once to f32;
 *   - std[g, m]      = sqrt(sum_i (x_i - mean64)^2 / (N - 1)) in f64, rounded once (torch.std's default); 0 for N = 1;
 *   - quant[g, k, m] = numpy's default "linear" quantile of q[k]: h = (N - 1) * q[k] in f64, lo = floor(h), hi =
 *     min(lo + 1, N - 1), value = x_(lo+1) + (float)(h - lo) * (x_(hi+1) - x_(lo+1)) in f32 (one subtract, one fused
 *     multiply-add); an integral h gives the order statistic itself bit for bit (q = 0, q = 1, N = 1 included);
 *   - with y (G, M), the ensemble CRPS of the point, in f64 from the f32 values:
 *       c = (1/N) sum_i |x_i - y| - (1/N^2) sum_{i=1..N} (2 i - N - 1) x_(i)
 *     (= mean |x - y| - 0.5 * mean_{i,j} |x_i - x_j|, the pair term from the sorted samples in O(N));
 *   - crps[g, s]  = the mean of c over the `seg` points of segment s (points [s * seg, (s + 1) * seg): one cycle),
 *     rounded once to f32;
 *   - cover[g, s] = the number of the segment's points with quant[g, 0, m] <= y <= quant[g, Q-1, m] -- the f32
 *     quantiles exactly as stored --, divided by seg.
 * Segment sums run in one fixed order: a thread adds its points in index order into an f64 partial, then a fixed tree
 * over the workgroup; no floating-point atomic, the same bits on every launch.
 * A point is bad when one of its samples is non-finite, or when y is given and non-finite there: it stores NaN in mean,
 * std and every quant, makes its segment's crps and cover NaN and adds 1 to *bad_count (a device int the caller zeroed;
 * one integer atomic per workgroup at most).
 * q is a HOST array of Q probabilities (they travel in the kernel arguments).  mean, std may each be NULL (skipped);
 * quant is required when Q > 0; y NULL: crps and cover must be NULL; crps, cover may each be NULL.
 * One 256-thread workgroup per (g, s); a thread's N samples are sorted in its own LDS column, sample i at float index
 * i * 256 + thread (N KiB of LDS per workgroup, conflict-free).
 * AW_ERR_ARG and no launch: N outside 1..AW_ENSEMBLE_MAX_N, Q outside 0..AW_ENSEMBLE_MAX_Q, a q outside [0, 1] or NaN,
 * seg < 1, M % seg != 0, cover with Q < 2, crps or cover without y, quant NULL with Q > 0, G * M / seg >= 2^31.
 * G == 0 or M == 0: AW_OK, nothing launched. */
#define AW_ENSEMBLE_MAX_N 64
#define AW_ENSEMBLE_MAX_Q 8
typedef struct {
  const float* x;  int G, N; int64_t M;
  const float* q;  int Q;
  float* mean; float* std;
  float* quant;
  const float* y;
  int64_t seg;
  float* crps;
  float* cover;
  int* bad_count;
} aw_ensemble_args;
int aw_ensemble_stats(const aw_ensemble_args* args, void* stream);

/* ------------------------------------------------------------------------------------------------ k-NN search
 * Brute-force exact k-nearest-neighbour search in squared Euclidean distance, f32 throughout (arcweld.retrieve): the
 * (nq x nx) distance matrix is never written to memory.
 * q: (nq, d) f32 queries, rows ldq >= d floats apart; x: (nx, d) f32 database, rows ldx >= d apart; any 4-byte aligned
 * base (16-byte loads when base and stride are 16-byte aligned, guarded 4-byte loads otherwise); the row padding and
 * the rows past the end are never read.  idx (nq, k) int64 and dist (nq, k) f32, compact, nearest first.
 *   - d(i, j) = fl(fl(|q_i|^2 + |x_j|^2) - 2 dot(q_i, x_j)); the norms are in-order fmaf chains over the dims, the dot
 *     products run on the f32-input MFMA (exact f32) in one fixed order over d, always inside one workgroup: the bits
 *     of a distance depend on neither the launch geometry nor the run.  No bf16 operand mode exists.
 *   - candidates are ranked lexicographically by (d as computed, j): the lower database index wins a tie.  Only a
 *     finite d is ever taken: a NaN or +inf distance (NaN / inf rows, f32 overflow) never appears as a neighbour.
 *   - the stored distance is max(d, 0); the clamp never touches the ranking.
 *   - q_group (nq) / x_group (nx) int32, each optional: row j is skipped for query i when q_group[i] == x_group[j];
 *     a NULL on either side means no exclusion (leave-one-out of a set against itself: group = row index).
 *   - with fewer than k eligible rows the remaining slots hold idx = -1 and dist = +inf.
 * Grid: (query tiles) x (database splits); every split writes its partial lists to the workspace and a second kernel
 * merges splits * k candidates per query in the same (d, j) order, so the result is bit-identical for every split
 * count.  splits = 0 picks the count that fills the device; ws needs aw_knn_workspace(nq, nx, d, k, splits) bytes
 * (4-byte aligned).  aw_knn_describe reports the tile sizes (queries per workgroup, database rows per tile, dims per
 * chunk) and AW_KNN_MAX_K.
 * AW_ERR_ARG and no launch (aw_knn_workspace returns AW_ERR_ARG): nq < 0, nx outside 0..2^31 - 1, d < 1, k outside
 * 1..AW_KNN_MAX_K, splits outside 0..AW_KNN_MAX_SPLITS, a stride below d or above 2^22 - 1, a NULL q / idx / dist, a
 * workspace that is too small.  nq == 0: AW_OK, nothing launched; nx == 0: every slot is (-1, +inf). */
#define AW_KNN_MAX_K 32
#define AW_KNN_MAX_SPLITS 1024
int64_t aw_knn_workspace(int64_t nq, int64_t nx, int d, int k, int splits);
int aw_knn(const float* q, int64_t nq, int64_t ldq, const float* x, int64_t nx, int64_t ldx, int d, int k,
           const int* q_group, const int* x_group, int splits /* 0 = auto */, void* ws, int64_t ws_bytes, int64_t* idx,
           float* dist, void* stream);
int aw_knn_describe(int* tile_q, int* tile_x, int* chunk_d, int* max_k);

/* ------------------------------------------------------------------------------------------------ DTW k-NN search
 * Brute-force exact k-nearest-neighbour search under banded dynamic time warping, f32 throughout
 * (arcweld.retrieve.dtw_search): the strong raw-signal baseline of the latent-space probe.  Neither the (nq x nx)
 * distance matrix nor any warping matrix is written to memory.
 * q: (nq, len, c) f32 queries and x: (nx, len, c) f32 database, time-major (the c channels of one sample contiguous),
 * rows ldq / ldx >= len * c floats apart; any 4-byte aligned base; the row padding and the rows past the end are never
 * read.  idx (nq, k) int64 and dist (nq, k) f32, compact, nearest first.
 *   - the band is Sakoe-Chiba with radius r: cell (i, j) -- sample i of the query, sample j of the database row --
 *     exists iff |i - j| <= r.  r = 0 is the squared Euclidean distance, r = len - 1 is unconstrained.
 *   - cost(i, j): acc = 0; for ch = 0 .. c - 1 in order: d = q[i][ch] - x[j][ch] (one f32 subtraction),
 *     acc = fmaf(d, d, acc).
 *   - D(0, 0) = cost(0, 0); otherwise D(i, j) = cost(i, j) + min(D(i-1, j-1), D(i-1, j), D(i, j-1)), one f32 addition,
 *     an absent cell counting as +inf.  dtw(q, x) = D(len - 1, len - 1): the squared-cost "dependent" multichannel
 *     DTW; no square root is taken.
 *   - min is exact and every cell has ONE fixed expression, so the bits of dtw(q, x) depend on neither the order the
 *     cells are evaluated in (rows, columns, anti-diagonals), the launch geometry, nor the run; dtw(q, x) and
 *     dtw(x, q) are the same bits.  A NaN cell never wins a minimum and everything behind it on every path is
 *     non-finite, so a row holding a NaN or an inf sample has a non-finite distance to everything.
 *   - candidates are ranked lexicographically by (dtw as computed, j): the lower database index wins a tie.  Only a
 *     finite distance is ever taken: NaN / inf rows and f32 overflow never appear as neighbours.
 *   - q_group (nq) / x_group (nx) int32, each optional: row j is skipped for query i when q_group[i] == x_group[j];
 *     a NULL on either side means no exclusion.  With fewer than k eligible rows the remaining slots hold idx = -1
 *     and dist = +inf.
 * Grid: (query tiles) x (database splits), one lane per (query, database row) pair; every split writes its partial
 * lists to the workspace and aw_knn's merge kernel picks from splits * k candidates per query in the same (d, j)
 * order, so the result is bit-identical for every split count.  splits = 0 picks the count that fills the device; ws
 * needs aw_dtw_knn_workspace(nq, nx, len, c, radius, k, splits) bytes (4-byte aligned).  aw_dtw_knn_describe reports
 * the tile sizes (queries per workgroup, database rows per tile).
 * AW_DTW_MAX_WINDOW is the largest band width 2 r + 1: a lane keeps one line of the band in LDS and the workgroup a
 * ring of 512 query samples that is refilled 64 samples at a time, so 2 r + 1 + 63 <= 512 (csrc/dtw.hip; about
 * 131 KiB of the CU's 160 KiB at the widest band with 8 channels).
 * AW_ERR_ARG and no launch (aw_dtw_knn_workspace returns AW_ERR_ARG): nq < 0, nx outside 0..2^31 - 1, len outside
 * 1..AW_DTW_MAX_LEN, c outside 1..AW_DTW_MAX_C, radius outside 0..len - 1, 2 radius + 1 > AW_DTW_MAX_WINDOW, k outside
 * 1..AW_KNN_MAX_K, splits outside 0..AW_KNN_MAX_SPLITS, a stride below len * c or above 2^22 - 1, a NULL q / idx /
 * dist, a workspace that is too small.  nq == 0: AW_OK, nothing launched; nx == 0: every slot is (-1, +inf). */
#define AW_DTW_MAX_LEN 2000
#define AW_DTW_MAX_WINDOW 449
#define AW_DTW_MAX_C 8
int64_t aw_dtw_knn_workspace(int64_t nq, int64_t nx, int len, int c, int radius, int k, int splits);
int aw_dtw_knn(const float* q, int64_t nq, int64_t ldq, const float* x, int64_t nx, int64_t ldx, int len, int c,
               int radius, int k, const int* q_group, const int* x_group, int splits /* 0 = auto */, void* ws,
               int64_t ws_bytes, int64_t* idx, float* dist, void* stream);
int aw_dtw_knn_describe(int* tile_q, int* tile_x);

/* ------------------------------------------------------------------------------------------------ logistic regression
 * One loss + gradient evaluation of p <= AW_LOGREG_MAX_P independent binary logistic regressions over one feature
 * matrix (arcweld.retrieve.logreg_fit): problem c is "class cls[c] against the rest" under its own parameters, so a
 * one-vs-rest fit and a sweep over regularisation strengths share every read of x.  f32 operands on the f32-input
 * MFMA (exact f32), f64 sums.  The kernels return raw sums: the regulariser and the 1/N scaling are the caller's.
 * x: (n, d) f32, rows ldx >= d floats apart, any 4-byte aligned base (16-byte loads in the forward when base and stride
 * are 16-byte aligned); the row padding and the rows past the end are never read.
 *
 * aw_logreg_forward.  w (d, p) f32 and b (p) f32, compact.  Always written: z (n, p) f32 compact, z = x w + b (one
 * fixed order over d, inside one workgroup; the bias is added last).  With labels -- y (n) int32 class ids and
 * cls (p) int32 -- also:
 *   r (n, p) f32 = sigma(z) - t, t_ic = (y_i == cls_c); sigma(z) = (z >= 0 ? 1 : e) / (1 + e), e = expf(-|z|);
 *   loss (p) f64, loss_c = sum_i softplus(z_ic) - t_ic z_ic, softplus(z) = fl(max(z, 0) + log1pf(e)) in f32, the
 *     difference and the sum in f64;
 *   gb (p) f64, gb_c = sum_i r_ic.
 *   A row with y_i < 0 takes no part: r = 0, and it counts in neither loss nor gb (z is still written).  A class
 *   that no row has gives t = 0 everywhere.  Each workgroup (aw_logreg_describe's tile_n rows) writes one partial
 *   per problem to ws; a second kernel adds them in a fixed order.  Labels are given when cls is not NULL (y may
 *   be NULL with n == 0).  y == NULL and cls == NULL: z only (the decision function of queries); r, loss, gb and ws
 *   are then ignored.
 * aw_logreg_grad.  g (d, p) f64 compact, g_kc = sum_i x_ik r_ic, r (n, p) f32 compact.  Grid: (tiles of tile_d dims)
 * x (row splits); a workgroup accumulates its rows in ascending order on the f32 MFMA and writes an f32 partial to
 * ws; a second kernel adds the splits' partials in f64 in split order.  splits = 0 picks the count that fills the
 * device.  The same inputs and the same split count give the same bits on every launch (no float atomics); the
 * bits may differ between split counts.
 * ws: aw_logreg_workspace(n, d, p, splits) bytes serve both calls (8-byte aligned).  aw_logreg_describe reports the
 * forward's rows per workgroup and dims per chunk, the gradient's dims per workgroup and AW_LOGREG_MAX_P.
 * n == 0: AW_OK; loss, gb (with labels) and g are written as zeros.  Neither call allocates or synchronises.
 * AW_ERR_ARG and no launch (aw_logreg_workspace returns AW_ERR_ARG): n < 0, d outside 1..2^22 - 1, p outside
 * 1..AW_LOGREG_MAX_P, splits outside 0..AW_LOGREG_MAX_SPLITS, a stride below d or above 2^22 - 1, a NULL w / b / g,
 * a NULL x / z with n > 0, y without cls, cls without loss / gb or (n > 0) y / r, a workspace that is missing or too small. */
#define AW_LOGREG_MAX_P 32
#define AW_LOGREG_MAX_SPLITS 1024
int64_t aw_logreg_workspace(int64_t n, int d, int p, int splits);
int aw_logreg_describe(int* tile_n, int* chunk_d, int* tile_d, int* max_p);
int aw_logreg_forward(const float* x, int64_t n, int64_t ldx, int d, const float* w, const float* b, int p,
                      const int* y, const int* cls, float* z, float* r, double* loss, double* gb, void* ws,
                      int64_t ws_bytes, void* stream);
int aw_logreg_grad(const float* x, int64_t n, int64_t ldx, int d, const float* r, int p, int splits /* 0 = auto */,
                   void* ws, int64_t ws_bytes, double* g, void* stream);

/* ------------------------------------------------------------------------------------------------ RBF-SVM probe
 * The two device steps of an RBF support-vector classifier on a frozen feature space (arcweld.retrieve.svm_fit /
 * svm_decision): the kernel matrix of two row sets, and the C-SVC dual solved by SMO on a precomputed kernel matrix.
 *
 * aw_rbf_gram.  a: (na, d) f32, rows lda >= d floats apart; b: (nb, d) f32, rows ldb >= d apart; any 4-byte aligned
 * base (16-byte loads when base and stride are 16-byte aligned, guarded 4-byte loads otherwise); the row padding and
 * the rows past the end are never read.  k: (na, nb) f32, rows ldk >= nb floats apart, any 4-byte aligned base; its
 * row padding is never written.
 *   - k[i][j] = expf(fl(-gamma * max(dist(i, j), 0))), dist(i, j) = fl(fl(|a_i|^2 + |b_j|^2) - 2 dot(a_i, b_j)): the
 *     norms are in-order fmaf chains over the dims, the dot products run on the f32-input MFMA (exact f32) in one fixed
 *     order over d, always inside one workgroup -- dist is bit for bit the distance aw_knn ranks by.
 *   - the bits of an element depend on neither the launch geometry nor the run, and since the sum of the norms and
 *     every product commute, the matrix of a set against itself is bit-symmetric: k[i][j] == k[j][i].  Its diagonal is
 *     what the formula gives: 1, or a hair below where the rounded dist is positive.
 *   - a distance that overflows to +inf gives 0.  A NaN distance (a NaN or inf feature, or inf - inf when the norms
 *     and the dot product both overflow) gives NaN: the caller keeps the features finite and their squares in range.
 *   - a == b with the same stride and row count: only the tiles on or above the diagonal are computed, each writes its
 *     mirror image as well -- the same bits as the general path, in about half the time.
 * Grid: (tiles of a) x (tiles of b), one tile per workgroup; aw_rbf_gram_describe reports the tile sizes (rows of a
 * and rows of b per workgroup, dims per chunk).
 * AW_ERR_ARG and no launch: na outside 0..2^31 - 1, nb outside 0..65535 * tile_b, d < 1, lda or ldb below d or above
 * 2^22 - 1, ldk < nb, a gamma that is not finite and positive, a NULL or misaligned a / b / k (with na, nb > 0).
 * na == 0 or nb == 0: AW_OK, nothing launched.
 *
 * aw_svm_smo.  p <= AW_SVM_MAX_P independent problems over one symmetric kernel matrix k (n, n) f32, rows ldk >= n
 * floats apart, n <= AW_SVM_MAX_N.  Problem c:  minimise  1/2 alpha' Q alpha - e' alpha  subject to
 * 0 <= alpha_t <= C[c] and sum_t y_ct alpha_t = 0,  Q_st = y_cs y_ct k_st,  y (p, n) int32 in {-1, 0, +1}, compact.
 * A row with y = 0 takes no part: its alpha is never written (the caller keeps it 0), it is never selected and its
 * grad entry is left alone -- the mask by which one-vs-one pairs and folds share one matrix.  Only rows of k
 * and its diagonal are read, which is where aw_rbf_gram's bit-symmetry matters.
 *   - C: p doubles in HOST memory, read before the call returns.
 *   - alpha, grad (p, n) f64, compact, in/out: a solve starts from alpha = 0, grad = -1; the kernel resumes from the
 *     state it is given and runs at most max_iter further iterations per problem, so a launch always ends.
 *     n_iter (p) int64 is incremented by the iterations run; gap (p) f64 receives m - M of the state that is left
 *     (-inf when either candidate set is empty).  A problem with gap <= tol on entry runs no iteration and leaves
 *     alpha, grad and n_iter as they are, bit for bit.
 *   - one iteration is libsvm's: with v_t = -y_t G_t, I_up = {y = +1, alpha < C} u {y = -1, alpha > 0} and
 *     I_low = {y = +1, alpha > 0} u {y = -1, alpha < C}:  i = argmax_{I_up} v (value m);  M = min_{I_low} v;  stop when
 *     m - M <= tol;  j = argmin over t in I_low with v_t < m of -b^2 / a, b = m - v_t, a = k_ii + k_tt - 2 k_it
 *     (a <= 0 is replaced by 1e-12);  libsvm's update of (alpha_i, alpha_j) with its clipping to the box;
 *     G_t += Q_ti dalpha_i + Q_tj dalpha_j for every row of the problem.  All of it in f64 without contraction.
 *   - every tie goes to the lowest row index and every reduction is a total order, so there are no float atomics and
 *     the bits are the same on every launch; a solve cut into several launches gives the bits of one launch.
 * One 1024-thread workgroup per problem, nothing shared between workgroups; the gradient and the rows' status live in
 * registers, the kernel diagonal and the current row i in LDS.  aw_svm_describe reports the threads per workgroup, the
 * rows per thread at AW_SVM_MAX_N, AW_SVM_MAX_N and AW_SVM_MAX_P; smaller n run shorter arrays with the same bits.
 * AW_ERR_ARG and no launch: n outside 0..AW_SVM_MAX_N, p outside 1..AW_SVM_MAX_P, ldk < n, a C that is not finite and
 * positive, a tol that is not positive, max_iter < 0, a NULL C / n_iter / gap, a NULL k / y / alpha / grad with n > 0.
 * n == 0: AW_OK, gap = -inf.  Neither call allocates or synchronises. */
#define AW_SVM_MAX_N 20480
#define AW_SVM_MAX_P 32
int aw_rbf_gram(const float* a, int64_t na, int64_t lda, const float* b, int64_t nb, int64_t ldb, int d, float gamma,
                float* k, int64_t ldk, void* stream);
int aw_rbf_gram_describe(int* tile_a, int* tile_b, int* chunk_d);
int aw_svm_smo(const float* k, int n, int64_t ldk, const int* y, const double* C, int p, double tol, int max_iter,
               double* alpha, double* grad, int64_t* n_iter, double* gap, void* stream);
int aw_svm_describe(int* threads, int* rows_per_thread, int* max_n, int* max_p);

/* ------------------------------------------------------------------------------------------------ TS2Vec encoder
 * The eval forward of the TS2Vec baseline's dilated-convolution encoder (arcweld.ts2vec.TSEncoder.encode; the
 * reference's model/ts2vec/encoder.py and dilated_conv.py), exact f32.  Activations are row-major (batch * T, C) f32:
 * row b * T + t holds the C channels of time step t of sequence b, rows C floats apart, 16-byte aligned bases.
 *
 * aw_ts_input_fc: out[r, h] = bias[h] + sum_c x[r, c] * w[h, c] (an in-order fmaf chain from the bias; w is
 *   (hidden, cin) as nn.Linear stores it) and out_gelu = gelu(out), the exact erf GELU.  A row of x with a NaN in any
 *   channel, and a row whose mask byte is 0 (mask: rows bytes, optional), is all zeros in both outputs: the zeroing
 *   before and after the reference's input_fc, bias included.  x is only read.
 * aw_ts_conv: one dilated convolution of `taps` = 3 taps (or the pointwise projection, taps = 1) as a GEMM on
 *   v_mfma_f32_32x32x2_f32 (bit for bit an fmaf chain):
 *       acc[b, t, :] = sum_{k < taps} W_k . in[b, t + (k - taps / 2) * dilation, :],
 *   w is (taps, cout, cin): tap k of torch's (cout, cin, taps) weight, re-laid-out once by the host.  A tap whose
 *   source step lies outside [0, T) of ITS OWN sequence contributes nothing: every operand load goes through a buffer
 *   descriptor that spans one sequence, so no row of a neighbouring sequence is ever read.  A workgroup owns
 *   128 time steps x 64 output channels of one sequence and skips a tap that is dead for all of its rows (all but the
 *   centre tap once dilation >= T): dead taps are not multiplied as zeros.
 *   Epilogue: v = fl(fl(acc + bias) + resid) (resid (batch * T, cout), optional); out = v and out_gelu = gelu(v), each
 *   optional.  pool (batch, cout), optional: pool[b, :] = max over t of v[b, t, :] -- a maximum per workgroup into
 *   pool_ws, then a second small pass over the time tiles; max does not round, so the result has the bits of the
 *   maximum of `out` whatever the order.  pool_ws needs aw_ts_pool_workspace(batch, T, cout) bytes.
 *   A sequence's values depend only on its own rows, T and the weights: not on batch, its position in it, or the run.
 * The order of one output element's sum: taps ascending (dead ones skipped), channels in chunks of 32 ascending, in a
 * chunk MFMA step 4 g + s multiplies channels 8 g + s (lanes 0..31) and 8 g + 4 + s (lanes 32..63).
 * Limits (AW_ERR_ARG and no launch beyond them): T in 1..AW_TS_MAX_T, cin (of aw_ts_input_fc) in 1..AW_TS_MAX_CIN,
 * every width (hidden, cin / cout of aw_ts_conv) a multiple of 16 in 16..AW_TS_MAX_WIDTH, taps 1 or 3, dilation in
 * 1..AW_TS_MAX_DILATION, batch in 0..AW_TS_MAX_BATCH per call, rows in 0..2^31 - 1; a NULL or misaligned operand; no
 * output at all.  batch == 0 / rows == 0: AW_OK, nothing launched.  Neither call allocates or synchronises.
 * Working set: beside the result the host keeps 5 hidden-wide and 2 output-wide activation buffers per row,
 * 4 T (5 hidden + 2 cout) bytes per sequence, and cuts the batch into chunks so that they stay within
 * AW_TS_WORKSPACE_BYTES (256 MiB; one sequence at the limits needs 56 MiB). */
#define AW_TS_MAX_T 4096
#define AW_TS_MAX_CIN 8
#define AW_TS_MAX_WIDTH 512
#define AW_TS_MAX_DILATION 1073741824
#define AW_TS_MAX_BATCH 65535
#define AW_TS_WORKSPACE_BYTES 268435456
int aw_ts_input_fc(const float* x, const void* mask, const float* w, const float* bias, int64_t rows, int cin,
                   int hidden, float* out, float* out_gelu, void* stream);
int64_t aw_ts_pool_workspace(int batch, int T, int cout);
int aw_ts_conv(const float* in, const float* w, const float* bias, const float* resid, int batch, int T, int cin,
               int cout, int taps, int dilation, float* out, float* out_gelu, float* pool, float* pool_ws,
               void* stream);
int aw_ts_describe(int* tile_t, int* tile_c, int* chunk_c);

/* ------------------------------------------------------------------------------------------------ TS2Vec loss
 * The hierarchical contrastive loss of TS2Vec training (arcweld.ts2vec.hierarchical_contrastive_loss; the reference's
 * model/ts2vec/losses.py), f32.  Both of its terms are the paired InfoNCE over groups: a group is 2 n rows of c
 * floats, rows 0..n-1 from z1 and rows n..2n-1 from z2; row r of group g of either tensor starts at
 * g * group_stride + r * row_stride floats.  With S = Z Z^T within a group and p(i) = (i + n) mod 2n,
 *     lse[g, i] = log sum_{j != i} exp S_ij,      row_loss[g, i] = lse[g, i] - S_{i, p(i)}
 * (lse and row_loss: (groups, 2 n) f32, contiguous).  The temporal term of (B, T, C) inputs is groups = B, n = T,
 * group_stride = T C, row_stride = C; the instance term is groups = T, n = B, group_stride = C, row_stride = T C.
 * No similarity is written to memory: the working set is the inputs and two floats per row.
 *
 * aw_nce_rows_fwd: lse and row_loss.  One row's value is accumulated in one fixed order over the group's rows (tiles
 *   of 128 rows of z1, then of z2; within a tile per lane, then a fixed merge): its bits depend on neither the number
 *   of groups, the group's position, nor the run.  n == 1 gives row_loss == 0 exactly.  No atomics.  Groups of
 *   2 n <= 128 rows are packed, 4, 2 or 1 to a workgroup in slots of 32, 64 or 128 rows; the slot a group lands in
 *   does not change its bits either.
 * aw_nce_rows_bwd: with the forward's lse,
 *     dz_i (+)= scale * [ sum_{j != i} (exp(S_ij - lse_i) + exp(S_ij - lse_j)) z_j  -  2 z_p(i) ],
 *   the gradient of scale * sum of row_loss; dz1 / dz2 are addressed as z1 / z2.  accumulate != 0 adds to what dz
 *   holds, 0 overwrites it.  Every element has one owning thread: no atomics, the same bits every run.
 * aw_ts_pool2_fwd: out[b, t, :] = max(in[b, 2 t, :], in[b, 2 t + 1, :]) for t < T / 2 (in (batch, T, c), out
 *   (batch, T / 2, c), contiguous): torch's max_pool1d(kernel 2, stride 2); an odd last step is dropped.
 * aw_ts_pool2_bwd: din[b, 2 t + k, :] += dout[b, t, :] at the k the forward took (recomputed from `in`; the first
 *   step on a tie, as torch does); the other step and an odd last step keep what they hold.
 * Limits (AW_ERR_ARG and no launch beyond them): c a multiple of 16 in 16..AW_NCE_MAX_WIDTH, n >= 1 with
 * 2 n <= AW_NCE_MAX_ROWS, groups in 0..AW_NCE_MAX_GROUPS per call, row_stride a multiple of 4 in c..2^22 - 1,
 * group_stride a non-negative multiple of 4; the pools: T in 2..AW_TS_MAX_T, batch in 0..AW_TS_MAX_BATCH; a NULL or
 * a not 16-byte aligned operand.  groups == 0 / batch == 0: AW_OK, nothing launched.  No call allocates or
 * synchronises. */
#define AW_NCE_MAX_ROWS 8192
#define AW_NCE_MAX_GROUPS 65535
#define AW_NCE_MAX_WIDTH 512
int aw_nce_rows_fwd(const float* z1, const float* z2, int groups, int n, int c, int64_t group_stride,
                    int64_t row_stride, float* lse, float* row_loss, void* stream);
int aw_nce_rows_bwd(const float* z1, const float* z2, int groups, int n, int c, int64_t group_stride,
                    int64_t row_stride, const float* lse, float scale, float* dz1, float* dz2, int accumulate,
                    void* stream);
int aw_nce_describe(int* tile_rows, int* chunk_c, int* slab_c);
int aw_ts_pool2_fwd(const float* in, int batch, int T, int c, float* out, void* stream);
int aw_ts_pool2_bwd(const float* in, const float* dout, int batch, int T, int c, float* din, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* ARCWELD_AMD_H */
