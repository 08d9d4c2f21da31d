"""Fused VQ-VAE-Patch training path on the HIP kernels (model/vq_vae_patch_embedd.py:117-167).

Activations are TOKEN-MAJOR: a batch of B windows is N = B*S token rows of H channels, row = b*S + t, with the
reference's channel-major patch order (tokens 0..S/2-1 voltage, S/2..S-1 current).  Every dense contraction is
one ``aw_gemm`` launch:

  patch embed   (N x ldp) . Wp^T            -> x0 (f32) + gelu(x0) (operand dtype)
  enc ResBlock  a0 . W1c^T -> h, gelu(h);  a1 . W2c^T + b, dropout, + x  -> x', gelu(x')   (centre taps only)
  sep conv      x_R . Ws^T                  -> z (f32)
  VQ            aw_vq_forward (fp32, bit-exact argmin)
  dec 1x1       zq . Wd0^T                  -> y0, gelu(y0)
  dec ResBlock  implicit k=3 conv GEMMs (K = 3H, rows shifted within each window)
  ConvT(H->H)   y_R . Wt1r^T (N = k1*H)     -> Y (f32) + BatchNorm column statistics in the epilogue
  head          BN -> GELU -> ConvT(H->1) -> x_hat, one wave per position

The backward mirrors it (input-gradient GEMMs with the GELU' and dropout masks fused in the epilogues,
weight-gradient GEMMs with the bias gradient fused as an A-row-sum).  Operands are exact fp32 MFMA by default
(the reference's numerics on MI355X); bf16 MFMA with fp32 accumulation is an explicit opt-in (arcweld.precision).
"""
from __future__ import annotations

import os
import types
import weakref

import torch

from . import _native as nat
from . import boundary
from . import kernels as K
from . import operands
from . import resstack
from .precision import operand_dtype  # noqa: F401  (re-exported: model/ and arcweld.decoder import it from here)

F32 = torch.float32


def rng_snapshot(m, dev, p_drop, zero=None):
    """Advance the module's device-side dropout counter and return a device copy of it for this forward (None
    when no dropout is active).  The kernels mix it into the host seeds (aw_gemm_args.seed_ptr), so a captured
    HIP graph draws fresh masks on every replay and the backward regenerates exactly the forward's masks.
    `zero` (a float64 block, the forward's accumulators) is zeroed by the same launch."""
    if p_drop <= 0.0:
        if zero is not None:
            zero.zero_()
        return None
    ctr = getattr(m, "_rng_counter", None)
    if ctr is None or ctr.device != dev:
        ctr = torch.zeros(1, dtype=torch.int64, device=dev)
        m._rng_counter = ctr
    snap = torch.empty(1, dtype=torch.int64, device=dev)
    K.counter_add_snapshot(ctr, snap, zero=zero)      # advance, snapshot (and zero) in one launch
    return snap


# partial code histograms of the VQ forward (aw_vq_forward, count_groups): workgroup b adds into partial b % 8, so no more
# than N / (64 * 8) workgroups add into one address (at 1, every workgroup's adds into the same 2 KB serialised at
# the memory-side atomic units: 2.5 us of the configs[1] kernel)
VQ_COUNT_GROUPS = 8


def accumulators(m, dev, K, H, zero=True):
    """Device accumulators of one forward, carved from one persistent f64 block (zeroed by ONE launch: here, or by
    rng_snapshot's when zero=False and the caller passes it the "block"): VQ sqerr (f64), MSE sqerr (f64,
    fused_train_step), BN column statistics (2H f64) and the VQ code counts (VQ_COUNT_GROUPS partial histograms of K
    f32, summed by aw_vq_finalize).  Each is consumed inside the call that filled it (never across a
    forward/backward boundary)."""
    key = (dev, K, H)
    st = m.__dict__.get("_acc_block")
    if st is None or st[0] != key:
        st = (key, torch.empty(2 + 4 * H + (VQ_COUNT_GROUPS * K + 1) // 2, dtype=torch.float64, device=dev))
        m.__dict__["_acc_block"] = st
    buf = st[1]
    if zero:
        buf.zero_()
    return dict(block=buf, vq_sq=buf[0:1], mse_sq=buf[1:2], colstats=buf[2:2 + 2 * H], head_gsums=buf[2 + 2 * H:2 + 4 * H],
                counts=buf[2 + 4 * H:].view(torch.float32)[:VQ_COUNT_GROUPS * K])


def resid_dtype(m, T):
    """dtype of the ResBlock residual streams (the activations x, y and their gradients) of the fused step.

    Exact-fp32 operands keep them in fp32 (the reference's numerics).  In the bf16 operand mode they are bf16, which
    is what the reference under bf16 autocast holds: its conv outputs are bf16, so x + block(x) and its gradient are
    bf16 tensors (model/vq_vae_patch_embedd.py:73-74) -- half the epilogue bytes of the 32 residual launches per step.
    ``--batchnorm 1`` keeps fp32 streams (its BatchNorm kernels read f32), as does ARCWELD_RESID_F32=1 (A/B)."""
    if T == F32 or m.batch_norm or os.environ.get("ARCWELD_RESID_F32", "0") == "1":
        return F32
    return T


class VQVAEShapes:
    def __init__(self, m, B):
        self.B = B
        self.H, self.D, self.K = m.hidden_dim, m.embedding_dim, m.num_embeddings
        self.R = m.n_resblocks
        self.P, self.L, self.C = m.patch_size, m.seq_len, m.input_dim
        self.S = self.L * self.C // self.P
        self.N = B * self.S
        self.k1 = m.reverse_patch_embed.k1
        self.Q = self.S * self.k1
        self.ldp = (self.P + 7) // 8 * 8


def _params(m):
    """Reference-layout parameter tensors of a VQVAEPatch, by role."""
    enc = [(blk.block[1], blk.block[4]) for blk in m.encoder[0].shared_conv]
    dec = [(blk.block[1], blk.block[4]) for blk in m.decoder[1].shared_conv]
    # --batchnorm 1: per block the BatchNorm1d after each ResBlock conv (block[2], block[5]); None with Identity
    enc_bn = [(blk.block[2], blk.block[5]) for blk in m.encoder[0].shared_conv] if m.batch_norm else None
    dec_bn = [(blk.block[2], blk.block[5]) for blk in m.decoder[1].shared_conv] if m.batch_norm else None
    rp = m.reverse_patch_embed.proj
    # the residual VQ (--use-improved-vq) keeps EMA codebook buffers, no codebook parameter
    E = None if getattr(m, "use_improved_vq", False) else m.vector_quantization.embedding.weight
    return dict(pe=m.patch_embed.proj, enc=enc, sep=m.encoder[1].shared_conv, E=E,
                dec0=m.decoder[0], dec=dec, t1=rp[0], bn=rp[1], t2=rp[3], enc_bn=enc_bn, dec_bn=dec_bn)


def routes(m, sh, T):
    """The launch routes of a pass over `m` with operand dtype T: ``forward`` reads all, ``decode`` the decoder's."""
    H, D, R, k1 = sh.H, sh.D, sh.R, sh.k1
    rt = types.SimpleNamespace(RT=resid_dtype(m, T))
    # bf16: a whole ResBlock stack as ONE persistent launch (csrc/reschain.hip), the same tensors bit for bit
    rt.enc_chain = K.res_chain_ok(H, R, T, rt.RT) and not m.batch_norm
    rt.dec_chain = K.res_chain_ok(H, R, T, rt.RT, 3, sh.S, "DEC") and not m.batch_norm
    # With the encoder chain and the reference's patch 25 (32 padded columns) patchify and the patch-embed GEMM run as
    # the head of the chain launch, which writes patches, x0 and a0 itself (ARCWELD_CHAIN_HEAD=0: two launches)
    rt.enc_head = rt.enc_chain and sh.ldp == 32 and K.chain_head_ok()
    # The sep conv (D = 64) rides as the tail of the encoder chain launch when that runs: x_R is still in LDS there,
    # so z costs 16 more K steps on a quarter of the fragments and no launch of its own (ARCWELD_SEP_TAIL=0: a GEMM)
    rt.sep_tail = rt.enc_chain and D == 64 and K.sep_tail_ok()
    # In the bf16 operand mode the ConvT output Y is bf16 (what autocast keeps for a ConvTranspose1d output; the BN
    # statistics still come from the f32 values in the epilogue): half the bytes of the GEMM's output and of the head's
    # passes over Y.  Round 3 measured it even over the step (the head passes are VALU-bound); on the round-4 step it
    # measured 3.162 / 3.155 / 3.157 vs 3.170 / 3.170 / 3.193 ms for an f32 Y (alternating, same box).
    # ARCWELD_HEAD_BF16=0 keeps Y in f32.
    rt.bf_y = T != F32 and K.head_bf16_ok(H) and os.environ.get("ARCWELD_HEAD_BF16", "1") == "1"
    # The un-patch ConvT rides as the tail of the decoder chain launch when that runs and Y is bf16: x_R is still in
    # LDS there, so the ConvT is k1 more 1-tap convs and no launch of its own (ARCWELD_CONVT_TAIL=0: a GEMM)
    rt.convt_tail = rt.dec_chain and rt.bf_y and k1 <= nat.AW_RES_TAIL_MAX and K.convt_tail_ok()
    # ... and the 1x1 conv (D = 64) as its head: the launch loads its rows of zq_T and writes y0 / ya0 itself
    # (ARCWELD_CHAIN_HEAD=0: a GEMM)
    rt.dec_head = rt.dec_chain and D == 64 and K.chain_head_ok()
    return rt


def _decoder_walk(m, pr, ops, rt, T, y0, ya0, x_hat, stack, **unpatch):
    """Decoder ResBlocks from y0 / ya0 = GELU(y0), the un-patch ConvT, the BatchNorm statistics and the fused head
    into x_hat, on the routes rt.  stack: resstack.forward's keywords, unpatch: boundary.unpatch_fwd's.  Returns
    (the ConvT's input operand, Y as (N k1, H), the BatchNorm stats, the saved stack)."""
    sh = VQVAEShapes(m, 1)
    H, R, k1, N = sh.H, sh.R, sh.k1, ya0.shape[0]
    Wt1, t1 = ops["Wt1"], pr["t1"]
    Y = torch.empty(N, k1 * H, device=ya0.device, dtype=T if rt.bf_y else F32)
    _, yR_T, rec = resstack.forward(resstack.Geometry(3, H, sh.S), y0, ya0,
                                    [(ops[f"dec{r}_1"], ops[f"dec{r}_2"]) for r in range(R)],
                                    resstack.biases(pr["dec"]), pr["dec_bn"], T=T, RT=rt.RT, chain=rt.dec_chain,
                                    tail=(Wt1, t1.bias, Y, unpatch.get("colstats")) if rt.convt_tail else None,
                                    **stack)
    if R == 0:
        yR_T = boundary.operand(y0, T)
    stats = boundary.unpatch_fwd(yR_T, Wt1, t1, pr["bn"], pr["t2"], Y, sh.Q, x_hat, convt=not rt.convt_tail, **unpatch)
    return yR_T, Y.view(N * k1, H), stats, rec


class Saved:
    pass


def _operand_jobs(m, T):
    """Every weight operand of the training step (forward and backward): arcweld.operands.OperandJob list."""
    from .operands import OperandJob as J
    sh = VQVAEShapes(m, 1)
    H, D, R, P, k1 = sh.H, sh.D, sh.R, sh.P, sh.k1
    pr = _params(m)
    dev = pr["pe"].weight.device
    e = lambda *s: torch.empty(*s, device=dev, dtype=T)  # noqa: E731
    jobs = [J("Wp", pr["pe"].weight, H, 1, P, 0, 4, torch.zeros(H, sh.ldp, device=dev, dtype=T),
              sh.ldp)]
    centre = lambda w: resstack._centre_job(w, None)[:6]  # noqa: E731  (the centre tap of the CURRENT storage)
    for r, (c1, c2) in enumerate(pr["enc"]):
        for nm, c in (("1", c1), ("2", c2)):
            jobs.append(J(f"enc{r}_{nm}", c.weight, H, H, 1, 0, 0, e(H, H), derive=centre))
    jobs.append(J("Ws", pr["sep"].weight, D, H, 1, 0, 0, e(D, H)))
    jobs.append(J("Wd0", pr["dec0"].weight, H, D, 1, 0, 0, e(H, D)))
    for r, (c1, c2) in enumerate(pr["dec"]):
        for nm, c in (("1", c1), ("2", c2)):
            jobs.append(J(f"dec{r}_{nm}", c.weight, H, H, 3, 0, 1, e(H, 3 * H)))     # forward [O][3I]
            jobs.append(J(f"dgw{r}_{nm}", c.weight, H, H, 3, 0, 2, e(3 * H, H)))     # dgrad [3O][I]
    jobs.append(J("Wt1", pr["t1"].weight, H, H, k1, 0, 3, e(k1 * H, H)))
    return jobs


def operand_set(m, T=None):
    """The OperandSet the training step of `m` reads (for arcweld.optim.RAdam.attach_operands)."""
    T = operand_dtype(T)
    return operands.peek(m, ("vqvae", T), lambda: _operand_jobs(m, T))


# The step's GEMM chain stores its epilogue outputs write-through (aw_gemm_args.store_policy): with 64 dependent
# class-A launches per step, each launch otherwise waits for the previous one's end-of-kernel L2 write-back of up to
# 32 MB of dirty output lines (same-box A/B: +3 % windows/s)
@K.store_policy(nat.AW_STORE_WT)
def forward(m, x, training: bool, need_backward: bool, dtype=None, seed: int = 0, head=True):
    """Returns (emb_loss (), x_hat (B, L, C), perplexity (), indices (N,), saved-or-None).

    ``head=False`` (the fused training step, need_backward only) stops after the BN statistics of the ConvT output:
    x_hat is returned unwritten, and the caller runs the head forward fused with the loss gradient and the first
    head-backward pass (``head_train``)."""
    T = operand_dtype(dtype)
    if x.dtype != F32 or x.dim() != 3:
        raise ValueError("VQVAEPatch expects float32 windows of shape (B, seq_len, input_dim)")
    x = x.contiguous()
    sh = VQVAEShapes(m, x.shape[0])
    H, D, N, S, R, P, k1 = sh.H, sh.D, sh.N, sh.S, sh.R, sh.P, sh.k1
    if x.shape[1] != sh.L or x.shape[2] != sh.C:
        raise ValueError(f"expected windows (B, {sh.L}, {sh.C}), got {tuple(x.shape)}")
    pr = _params(m)
    dev = x.device
    p_drop = float(m.dropout_p) if training else 0.0
    e = lambda *s, dt=F32: torch.empty(*s, device=dev, dtype=dt)  # noqa: E731
    sv = Saved()
    sv.sh, sv.T, sv.p_drop, sv.training = sh, T, p_drop, training
    rt = routes(m, sh, T)
    RT = sv.RT = rt.RT
    acc = sv.acc = accumulators(m, dev, sh.K, H, zero=False)
    sv.ctr = rng_snapshot(m, dev, p_drop, zero=acc["block"])
    # the head-backward sums of the block belong to one saved forward at a time: the owner is held by a weak
    # reference, released by its backward -- or by its collection when it is never backpropagated
    owner = m.__dict__.get("_acc_owner")
    owned = owner is not None and owner() is not None
    sv.head_gsums = acc["head_gsums"] if not owned else torch.zeros(2 * H, device=dev, dtype=torch.float64)
    if need_backward and not owned:
        m.__dict__["_acc_owner"] = weakref.ref(sv)

    # ---- operand copies of the weights (relayout + cast): persistent, refreshed by one batched relayout only when
    #      a weight changed outside the optimizer (the flat RAdam rewrites them in its update kernel)
    ops = sv.ops = operands.get(m, ("vqvae", T), lambda: _operand_jobs(m, T))
    Wp, Ws, Wd0 = ops["Wp"], ops["Ws"], ops["Wd0"]

    # ---- patch embed (unless it runs as the head of the encoder chain launch)
    patches = e(N, sh.ldp, dt=T)
    x0, a0 = e(N, H, dt=RT), e(N, H, dt=T)
    if not rt.enc_head:
        K.patchify(x, P, patches)
        boundary.conv_fwd(patches, Wp, pr["pe"].bias, x0, C2=a0, c2_mode=1, flops=2 * N * H * P)

    # ---- encoder ResBlocks (per-token: centre taps); the last block writes only the operand copy of x_R (all the
    #      sep conv consumes)
    stack = dict(p_drop=p_drop, ctr=sv.ctr, training=training, save=need_backward)
    z = e(N, D)
    _, xR_T, sv.enc = resstack.forward(resstack.Geometry(1, H, S), x0, a0,
                                       [(ops[f"enc{r}_1"], ops[f"enc{r}_2"]) for r in range(R)],
                                       resstack.biases(pr["enc"]), pr["enc_bn"], T=T, RT=RT,
                                       seeds=[boundary.mix(seed, 100 + r) for r in range(R)], chain=rt.enc_chain,
                                       sep=(Ws, pr["sep"].bias, z) if rt.sep_tail else None,
                                       head=(x, Wp, pr["pe"].bias, patches, P) if rt.enc_head else None, **stack)
    if R == 0:
        xR_T = boundary.operand(x0, T)

    # ---- SepCNNBlock -> z (B, S, D) (unless it ran as the tail of the encoder chain launch)
    if not rt.sep_tail:
        boundary.conv_fwd(xR_T, Ws, pr["sep"].bias, z)

    # ---- vector quantizer
    Kc = sh.K
    if pr["E"] is None:
        # residual VQ with EMA codebooks (vector_quantizer.py:9-56): commitment loss, no perplexity (:39)
        rvq = m.vector_quantization.vq
        zq, idx2, losses, sv.rvq = rvq.quantize_rows(z, training, save=need_backward)
        idx = idx2[:, 0] if rvq.num_quantizers == 1 else idx2
        emb_loss = losses.view(()) if rvq.num_quantizers == 1 else losses.sum()
        perplexity = None
    else:
        zq = e(N, D)
        idx = e(N, dt=torch.int64)
        counts, sq = acc["counts"], acc["vq_sq"]
        zq_T = None if T == F32 else e(N, D, dt=T)    # the operand copy comes out of the VQ kernel itself
        K.vq_forward(z, pr["E"], zq, idx, counts, sq, zq_copy=zq_T, count_groups=VQ_COUNT_GROUPS)
        emb_loss, perplexity = e(()), e(())
        K.vq_finalize(counts, sq, N, Kc, D, m.vector_quantization.beta, emb_loss, perplexity,
                      count_groups=VQ_COUNT_GROUPS)
    if pr["E"] is None or T == F32:
        zq_T = zq if T == F32 else boundary.cast(zq, T)

    # ---- decoder: 1x1 conv (unless it runs as the head of the decoder chain launch), ResBlocks with k=3 convs along
    #      the window, un-patch ConvT(H->H, k1) with BN statistics in the epilogue, then the fused head
    y0, ya0 = e(N, H, dt=RT), e(N, H, dt=T)
    if not rt.dec_head:
        boundary.conv_fwd(zq_T, Wd0, pr["dec0"].bias, y0, C2=ya0, c2_mode=1)
    x_hat = e(sh.B, sh.L, sh.C)
    sv.head_fused = not head and need_backward and fused_head_ok(H)
    stack.update(seeds=[boundary.mix(seed, 200 + r) for r in range(R)],
                 head=(zq_T, Wd0, pr["dec0"].bias) if rt.dec_head else None)
    yR_T, Y2, stats, sv.dec = _decoder_walk(m, pr, ops, rt, T, y0, ya0, x_hat, stack, training=training,
                                            colstats=acc["colstats"] if training else None, stats_mod=H,
                                            head=not sv.head_fused)

    if not need_backward:
        return emb_loss, x_hat, perplexity, idx, None
    sv.patches, sv.xR_T, sv.z, sv.idx, sv.zq_T = patches, xR_T, z, idx, zq_T
    sv.yR_T, sv.Y2, sv.stats = yR_T, Y2, stats
    return emb_loss, x_hat, perplexity, idx, sv


def fused_head_ok(H):
    """aw_unpatch_head_fwd_bwd1 serves H == 512 (the reference's hidden size)."""
    return H == 512


def head_train(m, sv, x, gscale, x_hat, sqerr, slot):
    """Head forward + MSE value and gradient + head-backward pass 1 in one read of the ConvT output (the fused
    training step; ``forward(..., head=False)`` left x_hat for it).  Returns g_xhat; ``backward`` then skips pass 1."""
    sh, H = sv.sh, sv.sh.H
    pr = _params(m)
    bn = pr["bn"]
    g_xhat = torch.empty_like(x_hat)
    K.unpatch_head_fwd_bwd1(sv.Y2, sh.Q, sv.stats, pr["t2"].weight.view(H, 5), pr["t2"].bias, x, gscale, x_hat,
                            g_xhat, sqerr, sv.head_gsums, slot(pr["t2"].weight).view(H, 5), slot(pr["t2"].bias),
                            slot(bn.weight), slot(bn.bias))
    sv.head_pass1_done = True
    return g_xhat


@torch.no_grad()
def encode(m, x, dtype=F32):
    """Frozen-encoder tokenization: windows (W, L, C) f32 -> (codebook indices (W*S,) int64, z (W*S, D) f32).

    patch embed -> encoder ResBlocks (eval: no dropout) -> sep conv -> VQ argmin; the decoder is never run
    (latentspace_dataloader.py:154-161 calls only patch_embed/encoder/vector_quantization).  Operands are exact
    fp32 unless ``dtype`` says otherwise, so the indices are the reference's bit for bit; ``dtype=torch.bfloat16``
    trades that for speed.
    """
    T = F32 if dtype is None else operand_dtype(dtype)
    if x.dtype != F32 or x.dim() != 3:
        raise ValueError("expected float32 windows of shape (W, seq_len, input_dim)")
    x = x.contiguous()
    sh = VQVAEShapes(m, x.shape[0])
    H, D, N, R, P = sh.H, sh.D, sh.N, sh.R, sh.P
    if x.shape[1] != sh.L or x.shape[2] != sh.C:
        raise ValueError(f"expected windows (W, {sh.L}, {sh.C}), got {tuple(x.shape)}")
    pr = _params(m)
    e = lambda *s, dt=F32: torch.empty(*s, device=x.device, dtype=dt)  # noqa: E731
    Wp = e(H, sh.ldp, dt=T)
    K.weight_relayout(pr["pe"].weight, H, 1, P, 0, 4, Wp, ldo=sh.ldp)
    patches = e(N, sh.ldp, dt=T)
    K.patchify(x, P, patches)
    xr, a = e(N, H), e(N, H, dt=T)
    boundary.conv_fwd(patches, Wp, pr["pe"].bias, xr, C2=a, c2_mode=1, flops=2 * N * H * P)
    ew = [(e(H, H, dt=T), e(H, H, dt=T)) for _ in range(R)]
    Ws = e(D, H, dt=T)
    geo = resstack.Geometry(1, H, sh.S)
    K.weight_relayout_batch([geo.fwd_job(c.weight, w) for cs, ws in zip(pr["enc"], ew) for c, w in zip(cs, ws)]
                            + [(pr["sep"].weight, D, H, 1, 0, 0, Ws)])
    # x <- x + conv2(gelu(h)) in place (row-local epilogue), a <- gelu(x); the sep conv consumes x_R itself (no GELU),
    # written in the operand dtype.  BatchNorm ResBlocks: the module mode decides batch vs running statistics
    _, xR_T, _ = resstack.forward(geo, xr, a, ew, resstack.biases(pr["enc"]), pr["enc_bn"], T=T, RT=F32,
                                  training=m.training, in_place=True, save=False)
    if R == 0:
        xR_T = boundary.operand(xr, T)
    z = e(N, D)
    boundary.conv_fwd(xR_T, Ws, pr["sep"].bias, z)
    if pr["E"] is None:   # residual VQ: eval-mode assignment (no EMA), one token per position needs nq == 1
        rvq = m.vector_quantization.vq
        if rvq.num_quantizers != 1:
            raise ValueError("tokenization needs a single quantizer (ResidualVQ num_quantizers == 1)")
        _, idx2, _, _ = rvq.quantize_rows(z, False)
        return idx2[:, 0].contiguous(), z
    zq, idx = e(N, D), e(N, dt=torch.int64)
    counts = torch.zeros(sh.K, device=x.device)
    sq = torch.zeros(1, device=x.device, dtype=torch.float64)
    K.vq_forward(z, pr["E"], zq, idx, counts, sq)
    return idx, z


@torch.no_grad()
@K.store_policy(nat.AW_STORE_WT)      # as forward(): the same GEMM chain
def decode(m, idx, dtype=None):
    """Ids back to signals: codebook indices (W*S,) int64 -> x_hat (W, L, C) f32 -- the mirror of ``encode``, the
    second half of ``forward`` with eval semantics: no dropout, the un-patch BatchNorm on its running statistics
    (which it leaves alone) whatever the module mode; BatchNorm ResBlocks follow the module mode, as in ``encode``.
    ``dtype=None`` is the process operand setting (arcweld.precision).

    In eval the decoder's 1x1 conv depends on the id alone, so it runs once over the K codebook rows (y0 and GELU(y0)
    tables, one aw_gemm) and aw_vq_decode_gather copies row idx[n] of each to token n; with more codes than tokens the
    codebook rows are gathered first and the GEMM runs over the N tokens.  Either gather checks every id in the
    kernel: an id outside [0, K) reads nothing, and the call raises ValueError once its launches are queued."""
    if getattr(m, "use_improved_vq", False):
        raise NotImplementedError("decode: ids -> signals is not implemented for use_improved_vq=True (the EMA "
                                  "residual quantizer keeps no codebook parameter to look the ids up in)")
    T = operand_dtype(dtype)
    if idx.dtype != torch.int64 or idx.dim() != 1:
        raise ValueError("decode expects a flat int64 tensor of W*S codebook indices")
    sh = VQVAEShapes(m, 1)
    H, D, S, Kc = sh.H, sh.D, sh.S, sh.K
    N = idx.numel()
    if N == 0 or N % S:
        raise ValueError(f"decode: {N} ids are not a positive multiple of the {S} ids of one window")
    W = N // S
    idx = idx.contiguous()
    pr = _params(m)
    dev = idx.device
    e = lambda *s, dt=F32: torch.empty(*s, device=dev, dtype=dt)  # noqa: E731
    rt = routes(m, sh, T)
    ops = operands.get(m, ("vqvae", T), lambda: _operand_jobs(m, T))
    Wd0, b0 = ops["Wd0"], pr["dec0"].bias

    # ---- decoder 1x1 conv: over the codebook + a two-table gather, or (K > N) a codebook gather + the GEMM
    bad = torch.zeros(1, device=dev, dtype=torch.int32)
    y0, ya0 = e(N, H, dt=rt.RT), e(N, H, dt=T)
    E = pr["E"]
    if Kc <= N:
        table_x, table_a = e(Kc, H, dt=rt.RT), e(Kc, H, dt=T)
        boundary.conv_fwd(boundary.operand(E, T), Wd0, b0, table_x, C2=table_a, c2_mode=1)
        K.vq_decode_gather(idx, table_x, table_a, y0, ya0, bad)
    else:
        zq = e(N, D)
        K.vq_decode_gather(idx, E, None, zq, None, bad)
        boundary.conv_fwd(boundary.operand(zq, T), Wd0, b0, y0, C2=ya0, c2_mode=1)

    # ---- decoder ResBlocks, un-patch ConvT and the head on the running statistics: forward()'s walk and routes
    x_hat = e(W, sh.L, sh.C)
    _decoder_walk(m, pr, ops, rt, T, y0, ya0, x_hat, dict(training=m.training, save=False), training=False)
    nbad = int(bad.item())
    if nbad:
        raise ValueError(f"decode: {nbad} of {N} ids lie outside the codebook [0, {Kc})")
    return x_hat


@K.store_policy(nat.AW_STORE_WT)
def backward(m, sv, g_emb, g_xhat, slot, mid_hook=None):
    """Accumulate parameter gradients into ``slot(param)`` (f32 tensors shaped like the parameter).

    ``mid_hook()`` runs once the decoder side is done (head, ConvT, decoder ResBlocks, decoder 1x1, codebook): those
    gradients are final there, which lets a data-parallel step reduce them while the encoder backward runs."""
    sh, T, RT, p_drop, ops = sv.sh, sv.T, sv.RT, sv.p_drop, sv.ops
    H, D, N, R, P = sh.H, sh.D, sh.N, sh.R, sh.P
    pr = _params(m)
    dev = g_xhat.device
    e = lambda *s, dt=F32: torch.empty(*s, device=dev, dtype=dt)  # noqa: E731
    g_xhat = g_xhat.contiguous()
    bnm = m.batch_norm and R > 0    # BatchNorm ResBlocks: each block applies its own dropout mask to the gradient

    def into_stack(rec, copy):    # epilogue of the GEMM in front of a stack's backward: + the masked operand copy
        return dict(C2=None if bnm else copy, c2_mode=0 if bnm else (3 if R > 0 else 2),
                    drop2=(p_drop, rec.seeds[-1] if R > 0 else 0), seed_ptr=sv.ctr)

    # ---- head + BN backward, ConvT1 weight gradient and input gradient -> grad of the decoder output
    owner = m.__dict__.get("_acc_owner")
    if owner is not None and owner() is sv:
        m.__dict__["_acc_owner"] = None
    gy, go = e(N, H, dt=RT), e(N, H, dt=T)
    boundary.unpatch_bwd(sv.yR_T, ops["Wt1"], pr["t1"], pr["bn"], pr["t2"], sv.Y2, sh.Q, sv.stats, g_xhat, sv.head_gsums,
                         slot, T, training=sv.training, pass1=not getattr(sv, "head_pass1_done", False), gx=gy,
                         **into_stack(sv.dec, go))

    # ---- decoder ResBlocks (reverse; bf16: the input-gradient chain of all R blocks in one launch).  The weight
    #      gradients of the whole stack are deferred and issued as ONE grouped launch (every tile runs the full token
    #      reduction: no split-K, no slab reduce); their operands stay alive until then
    dgw = [(ops[f"dgw{r}_1"], ops[f"dgw{r}_2"]) for r in range(R)]
    gy, go, wgrads = resstack.backward(sv.dec, gy, go, dgw, resstack.grads(pr["dec"], slot), pr["dec_bn"], slot)
    K.gemm_grouped(wgrads)

    # ---- decoder 1x1 conv (weight (H, D, 1) is a contiguous [H][D] matrix)
    boundary.conv_wgrad(go, sv.zq_T, slot(pr["dec0"].weight).view(H, D), slot(pr["dec0"].bias))
    gzq = e(N, D)
    boundary.conv_dgrad(go, ops["Wd0"], gzq)

    # ---- vector quantizer (straight-through + codebook/commitment loss)
    dz = e(N, D)
    dz_T = dz if T == F32 else None
    if pr["E"] is None:   # residual VQ: straight-through + commitment terms, codebooks are EMA buffers
        res, qs = sv.rvq
        nq = res.shape[0]
        K.rvq_backward(res, qs, gzq, g_emb if nq == 1 else g_emb.expand(nq).contiguous(), dz)
    else:
        dz_T = dz if T == F32 else e(N, D, dt=T)    # operand copy written by the VQ backward kernel
        K.vq_backward(sv.z, pr["E"], sv.idx, gzq, g_emb, m.vector_quantization.beta, dz, slot(pr["E"]),
                      dz_copy=None if T == F32 else dz_T)
    if mid_hook is not None:
        with K.store_policy(nat.AW_STORE_NT):     # the hook's own launches (e.g. collectives) keep the default policy
            mid_hook()
    if dz_T is None:
        dz_T = boundary.cast(dz, T)

    # ---- SepCNNBlock
    boundary.conv_wgrad(dz_T, sv.xR_T, slot(pr["sep"].weight).view(D, H), slot(pr["sep"].bias))
    gx, gxo = e(N, H, dt=RT), e(N, H, dt=T)
    boundary.conv_dgrad(dz_T, ops["Ws"], gx, **into_stack(sv.enc, gxo))

    # ---- encoder ResBlocks (reverse), on the forward's operand copies; weight gradients deferred as in the decoder
    gx, gxo, wgrads = resstack.backward(sv.enc, gx, gxo, sv.enc.ws, resstack.grads(pr["enc"], slot), pr["enc_bn"],
                                        slot)
    K.wgrad_issue(wgrads)      # the 16 per-token conv weight gradients: one stream-K batch (bf16) or one grouped launch

    # ---- patch embed weight/bias
    boundary.conv_wgrad(gxo, sv.patches, slot(pr["pe"].weight).view(H, P), slot(pr["pe"].bias))


class VQVAEPatchFunction(torch.autograd.Function):
    """autograd boundary of the fused path: inputs (x, *params) -> (emb_loss, x_hat, perplexity)."""

    @staticmethod
    def forward(ctx, m, x, seed, *params):
        training = m.training
        need = torch.is_grad_enabled() or any(p.requires_grad for p in params)
        emb, x_hat, perp, idx, sv = forward(m, x, training, need_backward=True, seed=seed)
        ctx.m, ctx.sv, ctx.params = m, sv, params
        if perp is not None:          # None for the residual VQ (vector_quantizer.py:39)
            ctx.mark_non_differentiable(perp)
        m._last_indices = idx
        return emb, x_hat, perp

    @staticmethod
    def backward(ctx, g_emb, g_xhat, g_perp):
        m, sv = ctx.m, ctx.sv
        sink = getattr(m, "_grad_sink", None)
        grads = {}

        def slot(p):
            if sink is not None and p in sink:
                return sink[p]
            g = grads.get(p)
            if g is None:
                g = torch.zeros_like(p, dtype=F32)
                grads[p] = g
            return g

        if g_emb is None:
            g_emb = torch.zeros(1, device=g_xhat.device)
        if g_xhat is None:
            g_xhat = torch.zeros(sv.sh.B, sv.sh.L, sv.sh.C, device=g_emb.device)
        backward(m, sv, g_emb.reshape(1).contiguous(), g_xhat, slot)
        ctx.sv = None
        return (None, None, None) + tuple(grads.get(p) for p in ctx.params)
