"""Typed wrappers over the C ABI (one function per entry point of include/arcweld_amd.h).

Every wrapper takes torch DEVICE tensors, derives sizes/leading dimensions from their strides, launches on the
current torch stream and raises on a non-zero status.  No wrapper has a CPU path.
"""
from __future__ import annotations

import contextvars
import ctypes

import torch

from . import _native as nat
from ._native import AW_ACT_DERIV, AW_ACT_GELU_ERF, AW_ACT_GELU_TANH, AW_BF16, AW_F32, GemmArgs, call, dtype_code, ptr, stream_ptr

__all__ = ["gemm", "AW_ACT_DERIV", "AW_ACT_GELU_ERF", "AW_ACT_GELU_TANH", "AW_BF16", "AW_F32"]


def _ld(t):
    if t is None:
        return 0
    if t.dim() == 1:
        return t.shape[0]
    if t.stride(-1) != 1:
        raise nat.NativeError("operand rows must be contiguous (stride(-1) == 1)")
    return t.stride(0)


# Epilogue store policy of the GEMMs issued inside a `store_policy(...)` block (aw_gemm_args.store_policy):
# nat.AW_STORE_NT (default) or nat.AW_STORE_WT (write-through: the VQ-VAE step, see arcweld/vqvae.py).
# The policy is context-local (a ContextVar): GEMMs issued from another thread, or from a callback that resets it
# (the VQ-VAE backward's mid_hook), keep their own.
_STORE_POLICY = contextvars.ContextVar("arcweld_store_policy", default=0)


class store_policy:
    """Context manager / decorator: GEMM launches issued inside use `policy` for their epilogue stores."""

    def __init__(self, policy):
        self.policy = int(policy)

    def __enter__(self):
        self._tok = _STORE_POLICY.set(self.policy)

    def __exit__(self, *exc):
        _STORE_POLICY.reset(self._tok)
        return False

    def __call__(self, fn):
        import functools

        @functools.wraps(fn)
        def wrapped(*a, **k):
            with store_policy(self.policy):
                return fn(*a, **k)
        return wrapped


# Optional live profiler: when set to a list, every gemm() appends (start_event, end_event, algorithmic_flops)
# recorded on the launch stream (bench.py uses it for the roofline of the GEMM kernel over the timed region).
PROFILE = None


def _algorithmic_flops(M, N, Kd, conv, flops):
    """2*M*N*K counting only taps that touch real input: the implicit k=3 conv loses one tap at each window
    edge (K_eff = cin*(3 - 2/seg)); callers with zero-padded operands (patch embed) pass `flops` explicitly."""
    if flops is not None:
        return float(flops)
    if conv is not None:
        seg = conv[1]
        return 2.0 * M * N * (Kd / 3.0) * (3.0 - 2.0 / seg)
    return 2.0 * M * N * Kd


def _gemm_args(A, B, M, N, K, *, a_trans=False, b_trans=False, conv=None, alpha=1.0, beta=0.0, bias=None,
               act=AW_ACT_GELU_ERF, pre=None, resid=None, drop=(0.0, 0), C=None, C2=None, c2_mode=0, drop2=(0.0, 0),
               colstats=None, stats_mod=0, a_rowsum=None, bias_mod=0, accumulate=False, col_map=(0, 1, 0),
               seed_ptr=None):
    if A.dtype != B.dtype:
        raise nat.NativeError(f"gemm operands must share a dtype ({A.dtype} vs {B.dtype})")
    a = GemmArgs()
    a.M, a.N, a.K = int(M), int(N), int(K)
    a.a_dtype = dtype_code(A.dtype)
    a.A, a.lda, a.a_trans = ptr(A), _ld(A), int(bool(a_trans))
    a.B, a.ldb, a.b_trans = ptr(B), _ld(B), int(bool(b_trans))
    if conv is not None:
        a.conv_cin, a.conv_seg, a.conv_dir, a.conv_operand = (int(v) for v in conv)
    a.alpha, a.beta = float(alpha), float(beta)
    a.bias = ptr(bias)
    a.act = int(act)
    a.store_policy = _STORE_POLICY.get()
    a.pre, a.ld_pre = ptr(pre), _ld(pre)
    if pre is not None:
        if pre.dtype not in (torch.float32, torch.bfloat16):
            raise nat.NativeError("pre must be float32 or bfloat16")
        a.pre_dtype = dtype_code(pre.dtype)
    a.resid, a.ld_resid = ptr(resid), _ld(resid)
    if resid is not None:
        if resid.dtype not in (torch.float32, torch.bfloat16):
            raise nat.NativeError("resid must be float32 or bfloat16")
        a.resid_dtype = dtype_code(resid.dtype)
    a.drop_p, a.drop_seed = float(drop[0]), int(drop[1]) & 0xFFFFFFFFFFFFFFFF
    if C is not None:
        a.C, a.ldc, a.c_dtype = ptr(C), _ld(C), dtype_code(C.dtype)
    if C2 is not None:
        a.C2, a.ldc2, a.c2_dtype = ptr(C2), _ld(C2), dtype_code(C2.dtype)
    a.c2_mode = int(c2_mode)
    a.drop2_p, a.drop2_seed = float(drop2[0]), int(drop2[1]) & 0xFFFFFFFFFFFFFFFF
    if colstats is not None:
        if colstats.dtype != torch.float64:
            raise nat.NativeError("colstats must be float64")
        a.colstats, a.stats_mod = ptr(colstats), int(stats_mod)
    a.a_rowsum = ptr(a_rowsum)
    a.bias_mod = int(bias_mod)
    a.accumulate = int(bool(accumulate))
    a.col_mod, a.col_mul, a.col_off = (int(v) for v in col_map)
    a.seed_ptr = ptr(seed_ptr)
    return a


def _timed(s, fn, flops, tag, name=None, nbytes=None):
    """Bench profiling (PROFILE is a list): HIP events around one launch on its stream, with the launch's
    algorithmic FLOPs, a kernel-family tag ("gemm_bf16", "gemm_f32", "attn_fwd", "attn_bwd", "vq_fwd"), the name of
    the kernel it runs (the rocprofv3 kernel name's stem, for the per-kernel roofline) and its algorithmic HBM bytes
    (None where not stated)."""
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(s)
    fn(s.cuda_stream)
    e1.record(s)
    PROFILE.append((e0, e1, flops, tag, name or tag, nbytes))


def _gemm_tag(A):
    return "gemm_bf16" if A.dtype == torch.bfloat16 else "gemm_f32"


def gemm(A, B, M, N, K, *, stream=None, flops=None, **kw):
    """C = epilogue(alpha * op(A) @ op(B)); see aw_gemm in include/arcweld_amd.h for the exact semantics.

    conv = (cin, seg, dir, operand) selects the implicit k=3 convolution form."""
    a = _gemm_args(A, B, M, N, K, **kw)
    lib = nat.load()
    wsn = lib.aw_gemm_workspace(ctypes.byref(a))
    ws = torch.empty(wsn, device=A.device, dtype=torch.float32) if wsn > 0 else None
    if PROFILE is None:
        call("aw_gemm_ws", ctypes.byref(a), ptr(ws), wsn, stream_ptr(stream))
        return kw.get("C")
    s = stream if stream is not None else torch.cuda.current_stream()
    _timed(s, lambda sp: call("aw_gemm_ws", ctypes.byref(a), ptr(ws), wsn, sp),
           _algorithmic_flops(M, N, K, kw.get("conv"), flops), _gemm_tag(A), "gemm_kernel")
    return kw.get("C")


MAX_GROUPS = nat.AW_GEMM_MAX_GROUPS


def gemm_grouped(problems, stream=None):
    """One aw_gemm_grouped launch per chunk of <= 16 accumulate-mode problems that share everything except
    (A, B, C, a_rowsum).  ``problems`` is a list of (A, B, M, N, K, kwargs) tuples as for ``gemm``."""
    for c0 in range(0, len(problems), MAX_GROUPS):
        chunk = problems[c0:c0 + MAX_GROUPS]
        arr = (GemmArgs * len(chunk))(*[_gemm_args(A, B, M, N, K, **kw) for (A, B, M, N, K, kw) in chunk])
        if PROFILE is None:
            call("aw_gemm_grouped", arr, len(chunk), stream_ptr(stream))
            continue
        s = stream if stream is not None else torch.cuda.current_stream()
        fl = sum(_algorithmic_flops(M, N, K, kw.get("conv"), None) for (_, _, M, N, K, kw) in chunk)
        c0_ = chunk[0]
        # the grouped decoder k = 3 weight gradients run wgrad_conv3_kernel (csrc/wgrad.hip wgrad_conv3_try)
        nm = "wgrad_conv3_kernel" if (c0_[5].get("conv") is not None and c0_[0].dtype == torch.bfloat16) \
            else "gemm_kernel (grouped)"
        _timed(s, lambda sp: call("aw_gemm_grouped", arr, len(chunk), sp), fl, _gemm_tag(chunk[0][0]), nm)


WGRAD_BATCH_MAX = nat.AW_WGRAD_BATCH_MAX     # aw_wgrad_batch problems per launch


def wgrad_batch_ok(problems):
    """True when aw_wgrad_batch takes these problems (bf16 operands, M / N multiples of 256, one K) and pays: at least
    128 of its 256 x 256 tiles (the transformer's half-step batch of four Linear kinds, 192 tiles: 656 -> 532 us per
    launch in tools/probe/wgrad_tt_probe.py, the decoder step 5.58 -> 5.44 ms same box).  Below that its split-K
    fix-up costs more than it saves (the VQ-VAE encoder's 64 tiles: 214 vs 184 us for the grouped launch), and the
    per-shape grouped launches run instead.  ARCWELD_WGRAD_BATCH=0 / 1 forces them off / on (A/B, tests)."""
    import os
    mode = os.environ.get("ARCWELD_WGRAD_BATCH", "auto")
    if mode == "0" or not problems or len(problems) > WGRAD_BATCH_MAX:
        return False
    arr = (GemmArgs * len(problems))(*[_gemm_args(A, B, M, N, K, **kw) for (A, B, M, N, K, kw) in problems])
    if nat.load().aw_wgrad_batch_workspace(arr, len(problems)) <= 0:
        return False
    tiles = sum((M // 256) * (N // 256) for (_, _, M, N, _, _) in problems)
    return mode == "1" or tiles >= 128


def wgrad_batch(problems, stream=None):
    """One aw_wgrad_batch launch over <= 32 weight-gradient problems (A, B, M, N, K, kwargs) as for ``gemm`` (M and
    N may differ between problems; K, alpha and the dtype may not); the stream-K workspace comes from the caching
    allocator."""
    arr = (GemmArgs * len(problems))(*[_gemm_args(A, B, M, N, K, **kw) for (A, B, M, N, K, kw) in problems])
    lib = nat.load()
    wsb = lib.aw_wgrad_batch_workspace(arr, len(problems))
    if wsb < 0:
        raise nat.NativeError(f"aw_wgrad_batch: batch not eligible ({lib.aw_last_error().decode(errors='replace')})")
    ws = torch.empty((wsb + 3) // 4, device=problems[0][0].device, dtype=torch.float32)
    if PROFILE is None:
        call("aw_wgrad_batch", arr, len(problems), ptr(ws), wsb, stream_ptr(stream))
        return
    s = stream if stream is not None else torch.cuda.current_stream()
    fl = sum(_algorithmic_flops(M, N, K, None, None) for (_, _, M, N, K, _) in problems)
    _timed(s, lambda sp: call("aw_wgrad_batch", arr, len(problems), ptr(ws), wsb, sp), fl, _gemm_tag(problems[0][0]),
           "wgrad_tt_kernel")


def wgrad_issue(problems, stream=None):
    """Weight-gradient problems of one backward region that share K: in aw_wgrad_batch launches of <= 32 problems
    when eligible (bf16, M / N multiples of 256), else one aw_gemm_grouped launch per shape."""
    if not problems:
        return
    nch = (len(problems) + WGRAD_BATCH_MAX - 1) // WGRAD_BATCH_MAX
    per = (len(problems) + nch - 1) // nch
    chunks = [problems[i:i + per] for i in range(0, len(problems), per)]
    if all(wgrad_batch_ok(c) for c in chunks):
        for c in chunks:
            wgrad_batch(c, stream)
        return
    by_shape = {}
    for pb in problems:
        by_shape.setdefault((pb[2], pb[3]), []).append(pb)
    for grp in by_shape.values():
        gemm_grouped(grp, stream)


# ------------------------------------------------------------------------------------------------ encoder chain
RES_CHAIN_MAX = nat.AW_RES_CHAIN_MAX


def res_chain_ok(H, R, T, RT, taps=1, seg=16, which="ENC"):
    """aw_res_chain_fwd / _bwd serve the bf16 operand mode with bf16 residual streams, H == 512 and 1 <= R <= 16
    (ResBlocks without BatchNorm): the encoder's per-token stack (taps 1) and the decoder's k = 3 stack over 16-token
    windows (taps 3, seg 16).  ARCWELD_ENC_CHAIN=0 / ARCWELD_DEC_CHAIN=0 keep the per-conv GEMM launches of that
    stack (A/B runs, and the tests that compare the two)."""
    import os
    if os.environ.get(f"ARCWELD_{which}_CHAIN", "1") == "0":
        return False
    return (H == 512 and 1 <= R <= RES_CHAIN_MAX and T == torch.bfloat16 and RT == torch.bfloat16
            and (taps == 1 or (taps == 3 and seg == 16)))


def _chain_store_policy():
    """The chain's store policy: non-temporal (ARCWELD_CHAIN_STORE=wt: write-through, for A/B runs).  Same-box
    A/B of the VQ-VAE step: 2.932 / 2.914 ms nt vs 2.971 / 2.959 ms wt (the GEMM launches it replaces use wt)."""
    import os
    return nat.AW_STORE_WT if os.environ.get("ARCWELD_CHAIN_STORE", "nt") == "wt" else nat.AW_STORE_NT


def _chk_rows(ts, N, H, who):
    for t in ts:
        if t is None:
            continue
        if t.dtype != torch.bfloat16 or t.dim() != 2 or tuple(t.shape) != (N, H) or not t.is_contiguous():
            raise nat.NativeError(f"{who}: activations must be contiguous ({N}, {H}) bfloat16 tensors")


def res_dropout_masks_empty(N, R, device):
    """An uninitialised buffer for the chain's dropout keep bits of R blocks at N tokens (res_chain_fwd fills it)."""
    nb = nat.load().aw_res_dropout_masks_bytes(int(N), int(R))
    if nb <= 0:
        raise nat.NativeError("res_dropout_masks: bad N / R")
    return torch.empty(nb, device=device, dtype=torch.uint8)


def res_dropout_masks(N, drop, seed_ptr=None, stream=None):
    """The chain's dropout keep bits for drop = (p, R seeds) at N tokens (aw_res_dropout_masks, the standalone form of
    what res_chain_fwd writes): a uint8 device tensor, or None when p == 0."""
    p, seeds = float(drop[0]), list(drop[1] or [])
    if p <= 0.0:
        return None
    R = len(seeds)
    out = res_dropout_masks_empty(N, R, torch.cuda.current_device() if seed_ptr is None else seed_ptr.device)
    sd = (ctypes.c_uint64 * R)(*[int(v) & 0xFFFFFFFFFFFFFFFF for v in seeds])
    call("aw_res_dropout_masks", int(N), R, p, sd, ptr(seed_ptr), ptr(out), stream_ptr(stream))
    return out


def _nbytes(ts):
    """Algorithmic HBM bytes of a launch: every operand read once and every output written once (distinct tensors;
    None entries are absent operands)."""
    seen, n = set(), 0
    for t in ts:
        if t is not None and t.data_ptr() not in seen:
            seen.add(t.data_ptr())
            n += t.numel() * t.element_size()
    return n


def _chain_flops(R, N, H, taps, seg):
    """Algorithmic flops of one chain launch: 2R convs of 2 N H (taps H) -- for taps 3 only the taps that touch a
    real row (the window edges lose one tap each, as _algorithmic_flops counts the implicit conv GEMMs)."""
    if taps == 1:
        return 4.0 * R * N * H * H
    return 4.0 * R * N * H * H * (3 - 2.0 / seg)


def convt_tail_ok():
    """The decoder chain may run the un-patch ConvT as its tail (res_chain_fwd(tail=...)).  ARCWELD_CONVT_TAIL=0 keeps
    the ConvT's own GEMM launch (A/B runs, and the tests that compare the two)."""
    import os
    return os.environ.get("ARCWELD_CONVT_TAIL", "1") != "0"


def sep_tail_ok():
    """The encoder chain may run the sep conv as its tail (res_chain_fwd(sep=...)).  ARCWELD_SEP_TAIL=0 keeps the sep
    conv's own GEMM launch (A/B runs, and the tests that compare the two)."""
    import os
    return os.environ.get("ARCWELD_SEP_TAIL", "1") != "0"


def chain_head_ok():
    """The chains may run the conv that makes their x_0 as their head (res_chain_fwd(head=...)): the decoder's 1x1
    conv, and patchify + the patch embed.  ARCWELD_CHAIN_HEAD=0 keeps those launches (A/B runs, and the tests that
    compare the two)."""
    import os
    return os.environ.get("ARCWELD_CHAIN_HEAD", "1") != "0"


def res_chain_fwd(a0, x0, w1, w2, b1, b2, dh, a1, dx, a, drop=(0.0, None), seed_ptr=None, masks=None, taps=1, seg=16,
                  stream=None, tail=None, sep=None, head=None):
    """One aw_res_chain_fwd launch over the R = len(w1) ResBlocks (see include/arcweld_amd.h).

    a0 / x0: (N, H) bf16; w1 / w2: R packed weight copies (res_pack_weights); b1 / b2: R f32 biases; dh / a1 / dx / a:
    R output tensors each -- dh[r] = GELU'(h_r), a1[r], dx[r] = GELU'(x_{r+1}) (the backward's multipliers), a[r]
    (dh, a1, dx entries may be None: not stored; dx[R-1] is never stored); drop = (p, R seeds); masks: None or a
    res_dropout_masks_empty(N, R) buffer the launch fills with the keep bits (for res_chain_bwd).

    tail (taps 3 only) = (wt, bias, Y, colstats): the un-patch ConvT on x_R inside the launch -- wt: its k1 matrices
    [out][in], each packed as a 1-tap forward copy (res_pack_weights(..., job_taps=)), bias: (H,) f32, Y: (N, k1 H)
    bf16, colstats: (2 H,) f64 accumulators or None.

    sep (taps 1 only) = (ws, bias, z): the sep conv on x_R inside the launch -- ws: its (64, H) bf16 operand copy
    [out][in] (not packed), bias: (64,) f32, z: (N, 64) f32 (may be the first N rows of a longer tensor).

    head: the conv that makes x_0 inside the launch; a0 / x0 are then outputs (either may be None: not stored).
    taps 3: (zq, w, bias) -- zq: (N, 64) bf16, w: the (H, 64) bf16 operand copy [out][in], bias: (H,) f32 (the
    decoder's 1x1 conv); taps 1: (x, w, bias, patches, P) -- x: the (B, L, C) f32 windows, w: the (H, 32) bf16 operand
    copy, patches: (N, 32) bf16 output or None, P <= 32 the patch size (patchify + the patch embed)."""
    N, H = a[-1].shape
    R = len(w1)
    if not (1 <= R <= RES_CHAIN_MAX) or not all(len(v) == R for v in (w2, b1, b2, dh, a1, dx, a)):
        raise nat.NativeError("res_chain_fwd: need R (1..16) entries in every per-block list")
    _chk_rows([a0, x0] + list(dh) + list(a1) + list(dx) + list(a), N, H, "res_chain_fwd")
    g = nat.ResChainFwdArgs()
    g.N, g.H, g.R, g.taps, g.seg = N, H, R, int(taps), int(seg)
    g.a0, g.x0 = ptr(a0), ptr(x0)
    for r in range(R):
        g.w1[r], g.w2[r], g.b1[r], g.b2[r] = ptr(w1[r]), ptr(w2[r]), ptr(b1[r]), ptr(b2[r])
        g.dgelu_h[r], g.a1[r], g.dgelu_x[r], g.a[r] = ptr(dh[r]), ptr(a1[r]), ptr(dx[r]), ptr(a[r])
        g.drop_seed[r] = int(drop[1][r]) & 0xFFFFFFFFFFFFFFFF if drop[0] > 0 else 0
    g.drop_p = float(drop[0])
    g.seed_ptr = ptr(seed_ptr)
    g.store_policy = _chain_store_policy()
    g.drop_masks = ptr(masks)
    flops, extra = _chain_flops(R, N, H, taps, seg), []
    if tail is not None:
        wt, tb, Y, cst = tail
        k1 = len(wt)
        if taps != 3 or not (1 <= k1 <= nat.AW_RES_TAIL_MAX):
            raise nat.NativeError(f"res_chain_fwd: the tail needs taps == 3 and 1..{nat.AW_RES_TAIL_MAX} matrices")
        if Y.dtype != torch.bfloat16 or tuple(Y.shape) != (N, k1 * H) or not Y.is_contiguous():
            raise nat.NativeError(f"res_chain_fwd: tail Y must be a contiguous ({N}, {k1 * H}) bfloat16 tensor")
        if tb.dtype != torch.float32 or tb.numel() != H or not tb.is_contiguous():
            raise nat.NativeError("res_chain_fwd: tail bias must be (H,) float32")
        if cst is not None and (cst.dtype != torch.float64 or cst.numel() < 2 * H or not cst.is_contiguous()):
            raise nat.NativeError("res_chain_fwd: tail colstats must be (2 H,) float64")
        for w in wt:
            if w.dtype != torch.bfloat16 or w.numel() != H * H or not w.is_contiguous():
                raise nat.NativeError("res_chain_fwd: tail matrices must be packed (H, H) bfloat16 copies")
        g.tail_k1 = k1
        for j in range(k1):
            g.tail_w[j] = ptr(wt[j])
        g.tail_bias, g.tail_y, g.tail_colstats = ptr(tb), ptr(Y), ptr(cst)
        # the launch's record carries the ConvT it absorbed: its algorithmic flops, and Y and the matrices as bytes
        flops += 2.0 * N * k1 * H * H
        extra = [Y, tb] + list(wt)
    if sep is not None:
        ws, sb, z = sep
        D = 64
        if taps != 1:
            raise nat.NativeError("res_chain_fwd: the sep tail needs taps == 1")
        if ws.dtype != torch.bfloat16 or tuple(ws.shape) != (D, H) or not ws.is_contiguous():
            raise nat.NativeError(f"res_chain_fwd: sep weights must be a contiguous ({D}, {H}) bfloat16 operand copy")
        if sb.dtype != torch.float32 or sb.numel() != D or not sb.is_contiguous():
            raise nat.NativeError(f"res_chain_fwd: sep bias must be ({D},) float32")
        if z.dtype != torch.float32 or tuple(z.shape) != (N, D) or not z.is_contiguous():
            raise nat.NativeError(f"res_chain_fwd: sep z must be a contiguous ({N}, {D}) float32 tensor")
        g.sep_d, g.sep_w, g.sep_bias, g.sep_z = D, ptr(ws), ptr(sb), ptr(z)
        # the launch's record carries the sep conv it absorbed, as the ConvT tail's does
        flops += 2.0 * N * D * H
        extra += [z, sb, ws]
    if head is not None:
        hin, hw, hb = head[:3]
        hk = 64 if taps == 3 else 32
        if hw.dtype != torch.bfloat16 or tuple(hw.shape) != (H, hk) or not hw.is_contiguous():
            raise nat.NativeError(f"res_chain_fwd: head weights must be a contiguous ({H}, {hk}) bfloat16 operand copy")
        if hb.dtype != torch.float32 or hb.numel() != H or not hb.is_contiguous():
            raise nat.NativeError("res_chain_fwd: head bias must be (H,) float32")
        if taps == 3:
            if len(head) != 3 or hin.dtype != torch.bfloat16 or tuple(hin.shape) != (N, hk) or not hin.is_contiguous():
                raise nat.NativeError(f"res_chain_fwd: the decoder head's input must be a contiguous ({N}, {hk}) "
                                      "bfloat16 tensor")
            hp = None
        else:
            hp, P = head[3], int(head[4])
            if hin.dtype != torch.float32 or hin.dim() != 3 or not hin.is_contiguous():
                raise nat.NativeError("res_chain_fwd: the encoder head's input must be contiguous (B, L, C) float32 windows")
            Bw, Lw, Cw = hin.shape
            if not (1 <= P <= hk) or (Lw * Cw) % P or Bw * (Lw * Cw // P) != N:
                raise nat.NativeError(f"res_chain_fwd: windows {tuple(hin.shape)} do not make {N} patches of {P}")
            if hp is not None and (hp.dtype != torch.bfloat16 or tuple(hp.shape) != (N, hk) or not hp.is_contiguous()):
                raise nat.NativeError(f"res_chain_fwd: patches must be a contiguous ({N}, {hk}) bfloat16 tensor")
            g.head_patches, g.head_L, g.head_C, g.head_P = ptr(hp), Lw, Cw, P
        g.head_k, g.head_in, g.head_w, g.head_bias = hk, ptr(hin), ptr(hw), ptr(hb)
        # the launch's record carries the conv it absorbed (the patch embed as its GEMM counted it: P real columns)
        flops += 2.0 * N * H * (hk if taps == 3 else P)
        extra += [hin, hw, hb, hp]
    elif a0 is None or x0 is None:
        raise nat.NativeError("res_chain_fwd: a0 / x0 missing")
    _maybe_timed(stream, "gemm_bf16", flops,
                 lambda sp: call("aw_res_chain_fwd", ctypes.byref(g), sp),
                 lambda: (f"res_chain_fwd_kernel<{int(taps)}>",
                          _nbytes([a0, x0, masks] + list(w1) + list(w2) + list(b1) + list(b2) + list(dh) + list(a1) +
                                  list(dx)[:-1] + list(a) + extra)))


def res_chain_bwd(gx, gxo, w1t, w2t, dh, x0, dx, gh, gxo_out, drop_p=0.0, masks=None, taps=1, seg=16, stream=None):
    """One aw_res_chain_bwd launch (see include/arcweld_amd.h): w1t / w2t are the packed backward copies, dh the
    forward's saved GELU'(h_r), x0 the stack input x_0 and dx[r] (r >= 1) the forward's GELU'(x_r) (dx[0] is not read:
    GELU'(x_0) is evaluated in the launch), gh / gxo_out the R outputs each; masks (drop_p > 0, R > 1): the keep bits
    res_chain_fwd wrote (or res_dropout_masks made)."""
    N, H = gx.shape
    R = len(w1t)
    if not (1 <= R <= RES_CHAIN_MAX) or not all(len(v) == R for v in (w2t, dh, dx, gh, gxo_out)):
        raise nat.NativeError("res_chain_bwd: need R (1..16) entries in every per-block list")
    _chk_rows([gx, gxo, x0] + list(dh) + list(dx[1:]) + list(gh) + list(gxo_out), N, H, "res_chain_bwd")
    g = nat.ResChainBwdArgs()
    g.N, g.H, g.R, g.taps, g.seg = N, H, R, int(taps), int(seg)
    g.gx, g.gxo, g.x0 = ptr(gx), ptr(gxo), ptr(x0)
    for r in range(R):
        g.w1t[r], g.w2t[r], g.dgelu_h[r] = ptr(w1t[r]), ptr(w2t[r]), ptr(dh[r])
        g.dgelu_x[r] = ptr(dx[r]) if r > 0 else None
        g.gh[r], g.gxo_out[r] = ptr(gh[r]), ptr(gxo_out[r])
    g.drop_p = float(drop_p)
    g.store_policy = _chain_store_policy()
    g.drop_masks = ptr(masks)
    _maybe_timed(stream, "gemm_bf16", _chain_flops(R, N, H, taps, seg),
                 lambda sp: call("aw_res_chain_bwd", ctypes.byref(g), sp),
                 lambda: (f"res_chain_bwd_kernel<{int(taps)}>",
                          _nbytes([gx, gxo, x0, masks] + list(w1t) + list(w2t) + list(dh) + list(dx[1:]) + list(gh) +
                                  list(gxo_out))))


def res_pack_weights(src, fwd=None, bwd=None, taps=1, stream=None, job_taps=None):
    """Fragment-packed copies of [512][taps*512] bf16 [out][(tap, in)] weights for the chain (aw_res_pack_weights):
    fwd[i] <- W packed (aw_res_chain_fwd's w1 / w2), bwd[i] <- the backward operand packed (aw_res_chain_bwd's w1t /
    w2t); either list may be None.  One launch per 32 matrices.  job_taps[i] (default taps) may be 1 in a taps = 3
    launch: a [512][512] matrix, forward copy only (the chain tail's matrices)."""
    n = len(src)
    fwd = fwd if fwd is not None else [None] * n
    bwd = bwd if bwd is not None else [None] * n
    jt = [int(taps)] * n if job_taps is None else [int(v) for v in job_taps]
    if len(fwd) != n or len(bwd) != n or len(jt) != n:
        raise nat.NativeError("res_pack_weights: list lengths differ")
    for i in range(n):
        for t in (src[i], fwd[i], bwd[i]):
            if t is not None and (t.dtype != torch.bfloat16 or t.numel() != 512 * 512 * jt[i] or not t.is_contiguous()):
                raise nat.NativeError(f"res_pack_weights: need contiguous 512 x {512 * jt[i]} bfloat16 tensors")
    for c0 in range(0, n, nat.AW_RES_PACK_MAX):
        sl = slice(c0, c0 + nat.AW_RES_PACK_MAX)
        m = len(src[sl])
        arr = lambda ts: (ctypes.c_void_p * m)(*[ptr(t) for t in ts])  # noqa: E731
        call("aw_res_pack_weights", arr(src[sl]), arr(fwd[sl]), arr(bwd[sl]),
             (ctypes.c_int * m)(*jt[sl]) if job_taps is not None else None, m, int(taps), stream_ptr(stream))


# ------------------------------------------------------------------------------------------------ VQ
def _chk_vq(who, name, t, shape, dtypes=(torch.float32,)):
    """The VQ entry points take raw pointers and sizes: a transposed, sliced or wrongly typed tensor would be read or
    written as garbage in silence."""
    if t.dtype not in dtypes or tuple(t.shape) != tuple(shape) or not t.is_contiguous():
        want = " or ".join(str(d).replace("torch.", "") for d in dtypes)
        raise nat.NativeError(f"{who}: {name} must be a contiguous {want} tensor of shape {tuple(shape)} (got "
                              f"{str(t.dtype).replace('torch.', '')} {tuple(t.shape)}, strides {tuple(t.stride())})")


def vq_forward(z2d, E, zq, idx, counts, sqerr, stream=None, zq_copy=None, count_groups=1):
    """zq_copy: optional bf16/f32 tensor that also receives z_q.  count_groups > 1: counts holds that many partial
    histograms of K floats (vq_finalize sums them)."""
    if z2d.dim() != 2 or E.dim() != 2:
        raise nat.NativeError(f"vq_forward: z must be (N, D) and E (K, D) (got {tuple(z2d.shape)}, {tuple(E.shape)})")
    N, D = z2d.shape
    Kc = E.shape[0]
    _chk_vq("vq_forward", "z", z2d, (N, D))
    _chk_vq("vq_forward", "E", E, (Kc, D))
    _chk_vq("vq_forward", "zq", zq, (N, D))
    _chk_vq("vq_forward", "idx", idx, (N,), (torch.int64,))
    _chk_vq("vq_forward", "sqerr", sqerr, (1,), (torch.float64,))
    if zq_copy is not None:
        _chk_vq("vq_forward", "zq_copy", zq_copy, (N, D), (torch.float32, torch.bfloat16))
    if counts.dtype != torch.float32 or not counts.is_contiguous() or counts.numel() < count_groups * Kc:
        raise nat.NativeError(f"vq_forward: counts must hold count_groups x K = {count_groups} x {Kc} contiguous "
                              f"float32 values (got {str(counts.dtype).replace('torch.', '')} {tuple(counts.shape)})")
    _maybe_timed(stream, "vq_fwd", 2.0 * N * Kc * D, lambda sp: call(
        "aw_vq_forward", ptr(z2d), ptr(E), N, Kc, D, ptr(zq), ptr(idx), ptr(counts), int(count_groups),
        ptr(sqerr), ptr(zq_copy), dtype_code(zq_copy.dtype) if zq_copy is not None else 0, sp),
        # the pinned kernel (codebook in LDS, f32-input MFMA) serves K <= 512, D in {16, 32, 64} (csrc/vq.hip)
        lambda: ("vq_fwd_pinned_kernel" if Kc <= 512 and D in (16, 32, 64) else "vq_fwd_kernel",
                 _nbytes([z2d, E, zq, idx, zq_copy]) + 4 * Kc * count_groups))


def vq_finalize(counts, sqerr, N, K, D, beta, loss, perplexity, stream=None, count_groups=1):
    call("aw_vq_finalize", ptr(counts), int(count_groups), ptr(sqerr), N, K, D, float(beta), ptr(loss),
         ptr(perplexity), stream_ptr(stream))


def vq_backward(z2d, E, idx, g_zq, g_loss, beta, dz, dE, stream=None, dz_copy=None):
    """dz_copy: optional bf16/f32 tensor that also receives dz."""
    if z2d.dim() != 2 or E.dim() != 2:
        raise nat.NativeError(f"vq_backward: z must be (N, D) and E (K, D) (got {tuple(z2d.shape)}, {tuple(E.shape)})")
    N, D = z2d.shape
    _chk_vq("vq_backward", "z", z2d, (N, D))
    _chk_vq("vq_backward", "E", E, (E.shape[0], D))
    _chk_vq("vq_backward", "idx", idx, (N,), (torch.int64,))
    if g_zq is not None:
        _chk_vq("vq_backward", "g_zq", g_zq, (N, D))
    if g_loss is not None and (g_loss.dtype != torch.float32 or g_loss.numel() != 1):
        raise nat.NativeError("vq_backward: g_loss must be one float32 on the device")
    _chk_vq("vq_backward", "dz", dz, (N, D))
    _chk_vq("vq_backward", "dE", dE, (E.shape[0], D))
    if dz_copy is not None:
        _chk_vq("vq_backward", "dz_copy", dz_copy, (N, D), (torch.float32, torch.bfloat16))
    call("aw_vq_backward", ptr(z2d), ptr(E), ptr(idx), ptr(g_zq), ptr(g_loss), N, E.shape[0], D, float(beta),
         ptr(dz), ptr(dE), ptr(dz_copy), dtype_code(dz_copy.dtype) if dz_copy is not None else AW_F32,
         stream_ptr(stream))


# ------------------------------------------------------------------------ residual VQ (EMA codebooks)
def vq_cluster_sums(z2d, idx, K, sums, stream=None):
    """sums[idx[n]] += z[n] (sums zeroed by the caller)."""
    _dense(z2d, "vq_cluster_sums")
    call("aw_vq_cluster_sums", ptr(z2d), ptr(idx), z2d.shape[0], K, z2d.shape[1], ptr(sums), stream_ptr(stream))


def kmeans_update(means, sums, counts, avg=None, stream=None):
    call("aw_kmeans_update", ptr(means), ptr(sums), ptr(counts), means.shape[0], means.shape[1], ptr(avg),
         stream_ptr(stream))


def rvq_ema_update(embed, embed_avg, cluster_size, counts, sums, z2d, decay, eps, threshold, salt, seed_ptr, ws,
                   stream=None):
    K, D = embed.shape
    call("aw_rvq_ema_update", ptr(embed), ptr(embed_avg), ptr(cluster_size), ptr(counts), ptr(sums), ptr(z2d),
         z2d.shape[0], K, D, float(decay), float(eps), float(threshold), int(salt) & 0xFFFFFFFFFFFFFFFF,
         ptr(seed_ptr), ptr(ws), stream_ptr(stream))


def rvq_residual(r, zq, out, first, r_next=None, stream=None):
    call("aw_rvq_residual", ptr(r), ptr(zq), zq.numel(), ptr(out), int(bool(first)), ptr(r_next), stream_ptr(stream))


def rvq_backward(res, q, g_zq, g_loss, dz, commitment=1.0, stream=None):
    """res, q: (nq, N, D); dz (N, D)."""
    nq, N, D = res.shape
    call("aw_rvq_backward", ptr(res), ptr(q), ptr(g_zq), ptr(g_loss), nq, N, D, float(commitment), ptr(dz),
         stream_ptr(stream))


def vq_onehot(idx, K, out, stream=None):
    call("aw_vq_onehot", ptr(idx), idx.numel(), K, ptr(out), stream_ptr(stream))


def vq_gather(E, idx, out, stream=None):
    call("aw_vq_gather", ptr(E), ptr(idx), idx.numel(), E.shape[1], ptr(out), stream_ptr(stream))


def _chk_i32_counter(t, who):
    if t.dtype != torch.int32 or t.numel() != 1:
        raise nat.NativeError(f"{who}: bad_count must be one int32 on the device")


def vq_decode_gather(idx, table_x, table_a, y0, ya0, bad_count, stream=None):
    """aw_vq_decode_gather: y0[n] = table_x[idx[n]] (and ya0[n] = table_a[idx[n]] unless both are None), range-checked
    in the kernel: an id outside [0, K) leaves a zero row and adds 1 to bad_count (an int32 the caller zeroed)."""
    Kc, H = table_x.shape
    N = idx.numel()
    if idx.dtype != torch.int64 or not idx.is_contiguous():
        raise nat.NativeError("vq_decode_gather: idx must be a contiguous int64 tensor")
    if (table_a is None) != (ya0 is None):
        raise nat.NativeError("vq_decode_gather: table_a and ya0 go together")
    for nm, tab, out in (("x", table_x, y0), ("a", table_a, ya0)):
        if tab is None:
            continue
        if (tuple(tab.shape) != (Kc, H) or tuple(out.shape) != (N, H) or out.dtype != tab.dtype
                or not tab.is_contiguous() or not out.is_contiguous()):
            raise nat.NativeError(f"vq_decode_gather: table_{nm} must be a contiguous ({Kc}, {H}) tensor and its output "
                                  f"a contiguous ({N}, {H}) tensor of the same dtype")
    _chk_i32_counter(bad_count, "vq_decode_gather")
    call("aw_vq_decode_gather", ptr(idx), N, ptr(table_x), ptr(table_a), Kc, H, dtype_code(table_x.dtype),
         dtype_code(table_a.dtype) if table_a is not None else AW_F32, ptr(y0), ptr(ya0), ptr(bad_count),
         stream_ptr(stream))


def sample_next(logits, ids_out, col, bad_count, n_valid=None, top_k=0, inv_temperature=1.0, do_sample=False, seed=0,
                step=0, u_out=None, stream=None):
    """aw_sample_next: the next token of each row of logits (B, V) f32 into ids_out[:, col] ((B, >= col + 1) int64);
    see include/arcweld_amd.h for the semantics.  u_out (B,) f32 receives the uniform draws when given."""
    B, V = logits.shape
    if logits.dtype != torch.float32 or not logits.is_contiguous():
        raise nat.NativeError("sample_next: logits must be a contiguous (B, V) float32 tensor")
    if (ids_out.dtype != torch.int64 or ids_out.dim() != 2 or ids_out.shape[0] != B or ids_out.stride(1) != 1
            or not 0 <= col < ids_out.shape[1]):
        raise nat.NativeError(f"sample_next: ids_out must be a (B, > {col}) int64 tensor with contiguous rows")
    if u_out is not None and (u_out.dtype != torch.float32 or u_out.numel() != B or not u_out.is_contiguous()):
        raise nat.NativeError("sample_next: u_out must be a contiguous (B,) float32 tensor")
    _chk_i32_counter(bad_count, "sample_next")
    call("aw_sample_next", ptr(logits), B, V, V if n_valid is None else int(n_valid), int(top_k or 0),
         float(inv_temperature), int(bool(do_sample)), int(seed) & 0xFFFFFFFFFFFFFFFF, int(step), ptr(ids_out),
         ids_out.stride(0), int(col), ptr(u_out), ptr(bad_count), stream_ptr(stream))


def sample_next_ex(logits, ids_out, col, bad_count, n_valid=None, top_k=0, top_p=1.0, min_p=0.0, inv_temperature=1.0,
                   do_sample=False, seed=0, step=0, u_out=None, logp_out=None, logq_out=None, col_lp=0,
                   n_kept_out=None, thr_out=None, stream=None):
    """aw_sample_next_ex: sample_next with a min-p and a nucleus (top-p) filter after top-k, and the likelihood of the
    chosen id; see include/arcweld_amd.h for the semantics.  logp_out / logq_out: (B, > col_lp) f32 with contiguous
    rows (the same shape and strides when both are given), written at [:, col_lp]; n_kept_out (B,) int32 and thr_out
    (B,) f32 receive the size of the kept set and its smallest scaled logit."""
    B, V = logits.shape
    if logits.dtype != torch.float32 or not logits.is_contiguous():
        raise nat.NativeError("sample_next_ex: logits must be a contiguous (B, V) float32 tensor")
    if (ids_out.dtype != torch.int64 or ids_out.dim() != 2 or ids_out.shape[0] != B or ids_out.stride(1) != 1
            or not 0 <= col < ids_out.shape[1]):
        raise nat.NativeError(f"sample_next_ex: ids_out must be a (B, > {col}) int64 tensor with contiguous rows")
    for nm, t, dt in (("u_out", u_out, torch.float32), ("n_kept_out", n_kept_out, torch.int32),
                      ("thr_out", thr_out, torch.float32)):
        if t is not None and (t.dtype != dt or t.numel() != B or not t.is_contiguous()):
            raise nat.NativeError(f"sample_next_ex: {nm} must be a contiguous (B,) {dt} tensor")
    lp = [t for t in (logp_out, logq_out) if t is not None]
    for t in lp:
        if (t.dtype != torch.float32 or t.dim() != 2 or t.shape[0] != B or t.stride(1) != 1
                or not 0 <= col_lp < t.shape[1] or (B > 1 and t.stride(0) < t.shape[1])):
            raise nat.NativeError(f"sample_next_ex: logp_out / logq_out must be (B, > {col_lp}) float32 tensors with "
                                  "contiguous rows")
    if len(lp) == 2 and (lp[0].shape != lp[1].shape or lp[0].stride() != lp[1].stride()):
        raise nat.NativeError("sample_next_ex: logp_out and logq_out must share shape and strides (one ld_lp)")
    _chk_i32_counter(bad_count, "sample_next_ex")
    a = nat.SampleArgs()
    a.logits, a.B, a.V, a.n_valid = ptr(logits), B, V, V if n_valid is None else int(n_valid)
    a.top_k, a.top_p, a.min_p, a.inv_temperature = int(top_k or 0), float(top_p), float(min_p), float(inv_temperature)
    a.do_sample, a.seed, a.step = int(bool(do_sample)), int(seed) & 0xFFFFFFFFFFFFFFFF, int(step)
    a.ids_out, a.ld_ids, a.col = ptr(ids_out), ids_out.stride(0), int(col)
    a.u_out, a.logp_out, a.logq_out = ptr(u_out), ptr(logp_out), ptr(logq_out)
    a.ld_lp, a.col_lp = (max(lp[0].stride(0), lp[0].shape[1]) if lp else 0), int(col_lp)
    a.n_kept_out, a.thr_out, a.bad_count = ptr(n_kept_out), ptr(thr_out), ptr(bad_count)
    call("aw_sample_next_ex", ctypes.byref(a), stream_ptr(stream))


def beam_step(logits, scores_in, scores_out, parent_out, token_out, logp_out, bad_count, n_valid=None, stream=None):
    """aw_beam_step: the W_out best one-token extensions of each sequence's W_in beams; see include/arcweld_amd.h for
    the semantics.  logits (B * W_in, V) f32 with contiguous rows (stride(0) is ldl), scores_in (B, W_in) f32; the
    outputs are contiguous with B * W_out elements each -- scores_out, logp_out f32, parent_out int32, token_out int64
    -- typically one step's slice of the search's (n_new, B, W_out) slabs.  The ranges of W_in, W_out, n_valid and
    W_in * n_valid are the library's to refuse (NativeError, nothing launched)."""
    if logits.dim() != 2 or logits.dtype != torch.float32 or logits.stride(1) != 1:
        raise nat.NativeError("beam_step: logits must be a (B * W_in, V) float32 tensor with contiguous rows")
    rows, V = logits.shape
    if scores_in.dim() != 2 or scores_in.dtype != torch.float32 or not scores_in.is_contiguous():
        raise nat.NativeError("beam_step: scores_in must be a contiguous (B, W_in) float32 tensor")
    B, W_in = scores_in.shape
    if B * W_in != rows or (rows > 1 and logits.stride(0) < V):
        raise nat.NativeError(f"beam_step: {rows} logits rows (stride {logits.stride(0)}) do not match scores_in "
                              f"{tuple(scores_in.shape)}")
    n_out = scores_out.numel()
    if B == 0 or n_out % B:
        raise nat.NativeError(f"beam_step: scores_out holds {n_out} elements, no multiple of B = {B}")
    for nm, t, dt in (("scores_out", scores_out, torch.float32), ("parent_out", parent_out, torch.int32),
                      ("token_out", token_out, torch.int64), ("logp_out", logp_out, torch.float32)):
        if t.dtype != dt or t.numel() != n_out or not t.is_contiguous():
            raise nat.NativeError(f"beam_step: {nm} must be a contiguous {dt} tensor of B * W_out = {n_out} elements")
    _chk_i32_counter(bad_count, "beam_step")
    a = nat.BeamArgs()
    a.logits, a.ldl, a.B, a.W_in, a.W_out = ptr(logits), max(logits.stride(0), V), B, W_in, n_out // B
    a.V, a.n_valid, a.scores_in = V, V if n_valid is None else int(n_valid), ptr(scores_in)
    a.scores_out, a.parent_out, a.token_out, a.logp_out = ptr(scores_out), ptr(parent_out), ptr(token_out), ptr(logp_out)
    a.bad_count = ptr(bad_count)
    call("aw_beam_step", ctypes.byref(a), stream_ptr(stream))


def beam_cache_table(cache_sets):
    """The device pointer tables aw_beam_gather reads: row i holds the base pointers of cache_sets[i], a list of one
    (rows, Tmax, width) tensor per decoder block.  Built once per search; the sets must outlive its use."""
    first = cache_sets[0][0]
    for kv in cache_sets:
        if len(kv) != len(cache_sets[0]):
            raise nat.NativeError("beam_cache_table: every cache set needs one tensor per block")
        for t in kv:
            if t.dim() != 3 or t.dtype != first.dtype or t.shape[1:] != first.shape[1:] or not t.is_contiguous():
                raise nat.NativeError("beam_cache_table: caches must be contiguous (rows, Tmax, width) tensors of one "
                                      "dtype, Tmax and width")
    return torch.tensor([[ptr(t) for t in kv] for kv in cache_sets], dtype=torch.int64, device=first.device)


def beam_gather(src_tab, dst_tab, B, W_in, parent, Tmax, n_pos, width, dtype, bad_count, stream=None):
    """aw_beam_gather: dst[k][b * W_out + j, :n_pos] = src[k][b * W_in + parent[b, j], :n_pos] for every block k in one
    launch; see include/arcweld_amd.h.  src_tab / dst_tab: rows of ``beam_cache_table`` (int64 device tensors of one
    pointer per block) whose caches hold B * W_in and B * W_out rows of (Tmax, width) ``dtype`` elements; parent (B,
    W_out) int32.  A parent outside [0, W_in) zero-fills its row and adds 1 to bad_count."""
    for nm, t in (("src_tab", src_tab), ("dst_tab", dst_tab)):
        if t.dtype != torch.int64 or t.dim() != 1 or not t.is_contiguous() or t.numel() != src_tab.numel():
            raise nat.NativeError(f"beam_gather: {nm} must be a contiguous 1-d int64 tensor, one pointer per block")
    if parent.dtype != torch.int32 or parent.dim() != 2 or parent.shape[0] != B or not parent.is_contiguous():
        raise nat.NativeError(f"beam_gather: parent must be a contiguous ({B}, W_out) int32 tensor")
    _chk_i32_counter(bad_count, "beam_gather")
    call("aw_beam_gather", ptr(src_tab), ptr(dst_tab), src_tab.numel(), int(B), int(W_in), parent.shape[1], ptr(parent),
         int(Tmax), int(n_pos), int(width), dtype_code(dtype), ptr(bad_count), stream_ptr(stream))


def beam_backtrack(parent, token, logp, ids_out, col0, logp_out, bad_count, stream=None):
    """aw_beam_backtrack: the slabs parent (int32), token (int64), logp (f32), each (n_new, B, W), walked back into
    ids_out[:, :, col0:col0 + n_new] ((B, R, >= col0 + n_new) int64) and logp_out ((B, R, n_new) f32) for the final
    beams j < R; see include/arcweld_amd.h."""
    if parent.dim() != 3:
        raise nat.NativeError("beam_backtrack: the slabs must be (n_new, B, W)")
    n_new, B, W = parent.shape
    for nm, t, dt in (("parent", parent, torch.int32), ("token", token, torch.int64), ("logp", logp, torch.float32)):
        if t.dtype != dt or tuple(t.shape) != (n_new, B, W) or not t.is_contiguous():
            raise nat.NativeError(f"beam_backtrack: {nm} must be a contiguous {dt} tensor of shape {(n_new, B, W)}")
    if (ids_out.dtype != torch.int64 or ids_out.dim() != 3 or ids_out.shape[0] != B or not ids_out.is_contiguous()
            or not 0 <= col0 <= ids_out.shape[2] - n_new):
        raise nat.NativeError(f"beam_backtrack: ids_out must be a contiguous (B, R, >= {col0} + {n_new}) int64 tensor")
    R = ids_out.shape[1]
    if logp_out.dtype != torch.float32 or tuple(logp_out.shape) != (B, R, n_new) or not logp_out.is_contiguous():
        raise nat.NativeError(f"beam_backtrack: logp_out must be a contiguous float32 tensor of shape {(B, R, n_new)}")
    _chk_i32_counter(bad_count, "beam_backtrack")
    call("aw_beam_backtrack", ptr(parent), ptr(token), ptr(logp), n_new, B, W, R, ptr(ids_out), ids_out.shape[2],
         int(col0), ptr(logp_out), ptr(bad_count), stream_ptr(stream))


def score_rows(logits, targets, seq_rows, groups, group_rows, logp, rank, entropy, group_nll, bad_count, n_valid=None,
               stream=None):
    """aw_score_rows: teacher-forced scores of logits (n_seq * seq_rows, V) f32 (rows may be padded: stride(0) >= V)
    against targets (n_seq, groups * group_rows) int64; see include/arcweld_amd.h for the semantics.  logp, entropy
    (f32) and rank (int32) take the targets' shape, group_nll (n_seq, groups) f32."""
    if logits.dim() != 2 or logits.dtype != torch.float32 or logits.stride(1) != 1:
        raise nat.NativeError("score_rows: logits must be a (rows, V) float32 tensor with contiguous rows")
    V = logits.shape[1]
    seq_rows, groups, group_rows = int(seq_rows), int(groups), int(group_rows)
    if seq_rows < 1 or groups < 1 or group_rows < 1 or groups * group_rows > seq_rows or logits.shape[0] % seq_rows:
        raise nat.NativeError(f"score_rows: {groups} groups of {group_rows} rows do not fit sequences of {seq_rows} "
                              f"rows, or the {logits.shape[0]} logits rows are not whole sequences")
    n_seq = logits.shape[0] // seq_rows
    if logits.shape[0] > 1 and logits.stride(0) < V:
        raise nat.NativeError("score_rows: logits rows overlap (stride(0) < V)")
    shape = (n_seq, groups * group_rows)
    for nm, t, dt, sh in (("targets", targets, torch.int64, shape), ("logp", logp, torch.float32, shape),
                          ("rank", rank, torch.int32, shape), ("entropy", entropy, torch.float32, shape),
                          ("group_nll", group_nll, torch.float32, (n_seq, groups))):
        if t.dtype != dt or tuple(t.shape) != sh or not t.is_contiguous():
            raise nat.NativeError(f"score_rows: {nm} must be a contiguous {dt} tensor of shape {sh}, got {t.dtype} "
                                  f"{tuple(t.shape)}")
    _chk_i32_counter(bad_count, "score_rows")
    call("aw_score_rows", ptr(logits), max(logits.stride(0), V), V, V if n_valid is None else int(n_valid),
         ptr(targets), n_seq, seq_rows, groups, group_rows, ptr(logp), ptr(rank), ptr(entropy), ptr(group_nll),
         ptr(bad_count), stream_ptr(stream))


def window_sqerr(a, b, out, bad_count, idx=None, stream=None):
    """aw_window_sqerr: out[w] = mean((a[w] - b'[w])^2) over a's windows a (windows, rows, width) f32.  idx None:
    b' = b, the same shape; idx (windows, rows) int64: b'[w, r] = b[idx[w, r]] with b (n, width), each id range-checked
    in the kernel (one outside [0, n) makes its window NaN and adds 1 to bad_count)."""
    if a.dim() != 3 or a.dtype != torch.float32 or not a.is_contiguous():
        raise nat.NativeError("window_sqerr: a must be a contiguous (windows, rows, width) float32 tensor")
    W, rows, width = a.shape
    want_b = (W, rows, width) if idx is None else (b.shape[0], width)
    if b.dtype != torch.float32 or tuple(b.shape) != want_b or not b.is_contiguous() or b.shape[0] < 1:
        raise nat.NativeError(f"window_sqerr: b must be a contiguous float32 tensor of shape {want_b}")
    if idx is not None and (idx.dtype != torch.int64 or tuple(idx.shape) != (W, rows) or not idx.is_contiguous()):
        raise nat.NativeError(f"window_sqerr: idx must be a contiguous ({W}, {rows}) int64 tensor")
    if out.dtype != torch.float32 or out.numel() != W or not out.is_contiguous():
        raise nat.NativeError(f"window_sqerr: out must be a contiguous float32 tensor of {W} elements")
    _chk_i32_counter(bad_count, "window_sqerr")
    call("aw_window_sqerr", ptr(a), ptr(b), ptr(idx), b.shape[0] if idx is not None else 0, W, rows, width, ptr(out),
         ptr(bad_count), stream_ptr(stream))


def ensemble_stats(x, q, mean=None, std=None, quant=None, y=None, seg=None, crps=None, cover=None, bad_count=None,
                   stream=None):
    """aw_ensemble_stats: pointwise statistics of x (G, N, M) f32 over its N samples, and with a truth y (G, M) the
    forecast's score per segment of ``seg`` points (None: one segment, seg = M); see include/arcweld_amd.h for the
    semantics.  q: a sequence of Q probabilities on the host.  mean, std (G, M), quant (G, Q, M), crps, cover
    (G, M // seg): contiguous f32, each optional except quant when Q > 0.  The ranges of N, Q, q and seg, and which
    outputs need which inputs, are the library's to refuse (NativeError, nothing launched)."""
    if x.dim() != 3 or x.dtype != torch.float32 or not x.is_contiguous():
        raise nat.NativeError("ensemble_stats: x must be a contiguous (G, N, M) float32 tensor")
    G, N, M = x.shape
    qs = [float(v) for v in q]
    Q = len(qs)
    seg = M if seg is None else int(seg)
    n_seg = M // seg if seg >= 1 else 0        # seg < 1 or M % seg != 0: refused by the library
    for nm, t, sh in (("mean", mean, (G, M)), ("std", std, (G, M)), ("quant", quant, (G, Q, M)), ("y", y, (G, M)),
                      ("crps", crps, (G, n_seg)), ("cover", cover, (G, n_seg))):
        if t is not None and (t.dtype != torch.float32 or tuple(t.shape) != sh or not t.is_contiguous()
                              or t.device != x.device):
            raise nat.NativeError(f"ensemble_stats: {nm} must be a contiguous float32 tensor of shape {sh} on x's "
                                  f"device, got {t.dtype} {tuple(t.shape)}")
    if bad_count is None:
        raise nat.NativeError("ensemble_stats: bad_count must be one int32 on the device")
    _chk_i32_counter(bad_count, "ensemble_stats")
    a = nat.EnsembleArgs()
    qa = (ctypes.c_float * max(Q, 1))(*qs)        # a host array: it outlives the call below
    a.x, a.G, a.N, a.M = ptr(x), G, N, M
    a.q, a.Q = ctypes.cast(qa, ctypes.c_void_p), Q
    a.mean, a.std, a.quant, a.y = ptr(mean), ptr(std), ptr(quant), ptr(y)
    a.seg, a.crps, a.cover, a.bad_count = seg, ptr(crps), ptr(cover), ptr(bad_count)
    call("aw_ensemble_stats", ctypes.byref(a), stream_ptr(stream))


def knn_describe():
    """aw_knn_describe: (tile_q, tile_x, chunk_d, max_k) of the k-NN kernel (the tests aim at the tile edges)."""
    v = [ctypes.c_int(0) for _ in range(4)]
    call("aw_knn_describe", *[ctypes.byref(c) for c in v])
    return tuple(int(c.value) for c in v)


def knn(q, x, k, q_group=None, x_group=None, splits=None, idx=None, dist=None, stream=None):
    """aw_knn: the k nearest rows of x (nx, D) for every row of q (nq, D) in squared Euclidean distance, f32, ranked by
    (distance, index); see include/arcweld_amd.h.  q, x: f32 device tensors with contiguous rows (any row stride >= D,
    any 4-byte aligned base).  q_group (nq) / x_group (nx): optional int32, equal groups are skipped.  splits None or
    0: the library picks the database split count.  Returns (idx (nq, k) int64, dist (nq, k) f32); slots past the
    eligible rows hold (-1, +inf).  The ranges of k and splits are the library's to refuse."""
    for nm, t in (("q", q), ("x", x)):
        if t.dim() != 2 or t.dtype != torch.float32 or (t.shape[1] > 1 and t.stride(1) != 1) or not t.is_cuda:
            raise nat.NativeError(f"knn: {nm} must be a 2-d float32 device tensor with contiguous rows, got "
                                  f"{t.dtype} {tuple(t.shape)} strides {tuple(t.stride())}")
    nq, D = q.shape
    nx = x.shape[0]
    if x.shape[1] != D or D < 1:
        raise nat.NativeError(f"knn: q has {D} features, x has {x.shape[1]}; need the same D >= 1")
    k = int(k)
    ldq = max(q.stride(0), D) if nq > 1 else D
    ldx = max(x.stride(0), D) if nx > 1 else D
    for nm, g, n in (("q_group", q_group, nq), ("x_group", x_group, nx)):
        if g is not None and (g.dtype != torch.int32 or tuple(g.shape) != (n,) or not g.is_contiguous()
                              or g.device != q.device):
            raise nat.NativeError(f"knn: {nm} must be a contiguous int32 tensor of {n} elements on q's device")
    sp = 0 if splits is None else int(splits)
    if idx is None:
        idx = torch.empty((nq, max(k, 0)), dtype=torch.int64, device=q.device)
    if dist is None:
        dist = torch.empty((nq, max(k, 0)), dtype=torch.float32, device=q.device)
    for nm, t, dt in (("idx", idx, torch.int64), ("dist", dist, torch.float32)):
        if t.dtype != dt or tuple(t.shape) != (nq, k) or not t.is_contiguous() or t.device != q.device:
            raise nat.NativeError(f"knn: {nm} must be a contiguous {dt} tensor of shape {(nq, k)} on q's device")
    lib = nat.load()
    ws_bytes = lib.aw_knn_workspace(nq, nx, D, k, sp)
    if ws_bytes < 0:
        raise nat.NativeError(f"aw_knn_workspace failed ({ws_bytes}): {lib.aw_last_error().decode(errors='replace')}")
    ws = torch.empty(max(ws_bytes, 16), dtype=torch.uint8, device=q.device)
    _maybe_timed(stream, "knn", 2.0 * nq * nx * D, lambda s: call(
        "aw_knn", ptr(q), nq, ldq, ptr(x) if nx else None, nx, ldx, D, k, ptr(q_group), ptr(x_group), sp, ptr(ws),
        ws.numel(), ptr(idx), ptr(dist), s),
        info=lambda: (f"knn_sweep_kernel k={k} D={D}", 4.0 * (nq + nx) * D + 12.0 * nq * k))
    return idx, dist


def dtw_knn_describe():
    """aw_dtw_knn_describe: (tile_q, tile_x) of the DTW search: queries per workgroup and database rows per tile (the
    tests aim at the tile edges)."""
    v = [ctypes.c_int(0) for _ in range(2)]
    call("aw_dtw_knn_describe", *[ctypes.byref(c) for c in v])
    return tuple(int(c.value) for c in v)


def dtw_knn(q, x, length, channels, radius, k, q_group=None, x_group=None, splits=None, idx=None, dist=None,
            stream=None):
    """aw_dtw_knn: the k nearest rows of x for every row of q under dynamic time warping inside a Sakoe-Chiba band of
    `radius` samples (squared sample costs, no square root), f32, ranked by (distance, index); see
    include/arcweld_amd.h.  q (nq, length * channels), x (nx, length * channels): f32 device tensors whose rows are
    time-major sequences -- an (n, length, channels) tensor flattened per row -- with contiguous rows (any row stride
    >= length * channels, any 4-byte aligned base).  q_group (nq) / x_group (nx): optional int32, equal groups are
    skipped.  splits None or 0: the library picks the database split count.  Returns (idx (nq, k) int64, dist (nq, k)
    f32); slots past the eligible rows hold (-1, +inf).  The ranges of length, channels, radius, k and splits are the
    library's to refuse."""
    for nm, t in (("q", q), ("x", x)):
        if t.dim() != 2 or t.dtype != torch.float32 or (t.shape[1] > 1 and t.stride(1) != 1) or not t.is_cuda:
            raise nat.NativeError(f"dtw_knn: {nm} must be a 2-d float32 device tensor with contiguous rows, got "
                                  f"{t.dtype} {tuple(t.shape)} strides {tuple(t.stride())}")
    length, channels, radius, k = int(length), int(channels), int(radius), int(k)
    nq, D = q.shape
    nx = x.shape[0]
    if x.shape[1] != D or D < 1 or D != length * channels:
        raise nat.NativeError(f"dtw_knn: q has {D} values per row, x has {x.shape[1]}; need length * channels = "
                              f"{length} * {channels} on both")
    ldq = max(q.stride(0), D) if nq > 1 else D
    ldx = max(x.stride(0), D) if nx > 1 else D
    for nm, g, n in (("q_group", q_group, nq), ("x_group", x_group, nx)):
        if g is not None and (g.dtype != torch.int32 or tuple(g.shape) != (n,) or not g.is_contiguous()
                              or g.device != q.device):
            raise nat.NativeError(f"dtw_knn: {nm} must be a contiguous int32 tensor of {n} elements on q's device")
    sp = 0 if splits is None else int(splits)
    if idx is None:
        idx = torch.empty((nq, max(k, 0)), dtype=torch.int64, device=q.device)
    if dist is None:
        dist = torch.empty((nq, max(k, 0)), dtype=torch.float32, device=q.device)
    for nm, t, dt in (("idx", idx, torch.int64), ("dist", dist, torch.float32)):
        if t.dtype != dt or tuple(t.shape) != (nq, k) or not t.is_contiguous() or t.device != q.device:
            raise nat.NativeError(f"dtw_knn: {nm} must be a contiguous {dt} tensor of shape {(nq, k)} on q's device")
    lib = nat.load()
    ws_bytes = lib.aw_dtw_knn_workspace(nq, nx, length, channels, radius, k, sp)
    if ws_bytes < 0:
        raise nat.NativeError(f"aw_dtw_knn_workspace failed ({ws_bytes}): "
                              f"{lib.aw_last_error().decode(errors='replace')}")
    ws = torch.empty(max(ws_bytes, 16), dtype=torch.uint8, device=q.device)
    cells = float(length * (2 * radius + 1) - radius * (radius + 1))      # cells of the band, 0 <= radius < length
    _maybe_timed(stream, "dtw_knn", float(nq) * nx * cells, lambda s: call(
        "aw_dtw_knn", ptr(q), nq, ldq, ptr(x) if nx else None, nx, ldx, length, channels, radius, k, ptr(q_group),
        ptr(x_group), sp, ptr(ws), ws.numel(), ptr(idx), ptr(dist), s),
        info=lambda: (f"dtw_sweep_kernel k={k} L={length} C={channels} r={radius}",
                      4.0 * (nq + nx) * D + 12.0 * nq * k))
    return idx, dist


def logreg_describe():
    """aw_logreg_describe: (tile_n, chunk_d, tile_d, max_p) of the logistic-regression kernels: the forward's rows per
    workgroup and dims per chunk, the gradient's dims per workgroup, the problem limit (the tests aim at the edges)."""
    v = [ctypes.c_int(0) for _ in range(4)]
    call("aw_logreg_describe", *[ctypes.byref(c) for c in v])
    return tuple(int(c.value) for c in v)


def _logreg_x(x, who):
    if x.dim() != 2 or x.dtype != torch.float32 or (x.shape[1] > 1 and x.stride(1) != 1) or not x.is_cuda:
        raise nat.NativeError(f"{who}: x must be a 2-d float32 device tensor with contiguous rows, got "
                              f"{x.dtype} {tuple(x.shape)} strides {tuple(x.stride())}")
    n, D = x.shape
    return n, D, (max(x.stride(0), D) if n > 1 else D)


def logreg_workspace(n, D, P, splits=None, device=None):
    """A uint8 workspace of aw_logreg_workspace(n, D, P, splits) bytes: it serves logreg_forward and logreg_grad at
    these sizes, so a fit allocates it once."""
    lib = nat.load()
    ws_bytes = lib.aw_logreg_workspace(n, D, P, 0 if splits is None else int(splits))
    if ws_bytes < 0:
        raise nat.NativeError(f"aw_logreg_workspace failed ({ws_bytes}): "
                              f"{lib.aw_last_error().decode(errors='replace')}")
    return torch.empty(max(ws_bytes, 16), dtype=torch.uint8, device=device)


def _logreg_ws(n, D, P, sp, ws, dev):
    return logreg_workspace(n, D, P, sp, dev) if ws is None else ws


def _logreg_out(t, nm, shape, dt, dev, who):
    if t is None:
        return torch.empty(shape, dtype=dt, device=dev)
    if t.dtype != dt or tuple(t.shape) != tuple(shape) or not t.is_contiguous() or t.device != dev:
        raise nat.NativeError(f"{who}: {nm} must be a contiguous {dt} tensor of shape {tuple(shape)} on x's device")
    return t


def logreg_forward(x, w, b, y=None, cls=None, z=None, r=None, loss=None, gb=None, ws=None, stream=None):
    """aw_logreg_forward: z (n, P) = x (n, D) @ w (D, P) + b (P) in f32 for P <= 32 binary problems; with labels y (n)
    int32 and cls (P) int32 also r = sigmoid(z) - (y == cls) (n, P) f32 and the f64 sums loss (P) = sum softplus(z) -
    t z and gb (P) = sum r over the rows with y >= 0; see include/arcweld_amd.h.  x: f32 device tensor with contiguous
    rows (any row stride >= D, any 4-byte aligned base).  Returns z without labels, (z, r, loss, gb) with them.  ws: an
    optional uint8 workspace of aw_logreg_workspace bytes to reuse across calls."""
    who = "logreg_forward"
    n, D, ldx = _logreg_x(x, who)
    dev = x.device
    if w.dim() != 2 or w.dtype != torch.float32 or not w.is_contiguous() or w.device != dev or w.shape[0] != D:
        raise nat.NativeError(f"{who}: w must be a contiguous float32 tensor of shape ({D}, P) on x's device, got "
                              f"{w.dtype} {tuple(w.shape)}")
    P = w.shape[1]
    if b.dtype != torch.float32 or tuple(b.shape) != (P,) or not b.is_contiguous() or b.device != dev:
        raise nat.NativeError(f"{who}: b must be a contiguous float32 tensor of {P} elements on x's device")
    if (y is None) != (cls is None):
        raise nat.NativeError(f"{who}: y and cls go together")
    for nm, t, m in (("y", y, n), ("cls", cls, P)):
        if t is not None and (t.dtype != torch.int32 or tuple(t.shape) != (m,) or not t.is_contiguous()
                              or t.device != dev):
            raise nat.NativeError(f"{who}: {nm} must be a contiguous int32 tensor of {m} elements on x's device")
    z = _logreg_out(z, "z", (n, P), torch.float32, dev, who)
    if y is not None:
        r = _logreg_out(r, "r", (n, P), torch.float32, dev, who)
        loss = _logreg_out(loss, "loss", (P,), torch.float64, dev, who)
        gb = _logreg_out(gb, "gb", (P,), torch.float64, dev, who)
        ws = _logreg_ws(n, D, P, 0, ws, dev)
    _maybe_timed(stream, "logreg_forward", 2.0 * n * D * P, lambda s: call(
        "aw_logreg_forward", ptr(x) if n else None, n, ldx, D, ptr(w), ptr(b), P, ptr(y), ptr(cls),
        ptr(z) if n else None, ptr(r) if (n and y is not None) else None, ptr(loss) if y is not None else None,
        ptr(gb) if y is not None else None, ptr(ws) if y is not None else None,
        ws.numel() if y is not None else 0, s),
        info=lambda: (f"logreg_fwd_kernel P={P} D={D}", 4.0 * n * D + 4.0 * D * P + 8.0 * n * P))
    return z if y is None else (z, r, loss, gb)


def logreg_grad(x, r, splits=None, g=None, ws=None, stream=None):
    """aw_logreg_grad: g (D, P) f64 = x.T @ r summed over the rows, x (n, D) f32 (contiguous rows, any stride >= D),
    r (n, P) f32 contiguous.  splits None or 0: the library picks the row split count; the same count gives the same
    bits on every launch."""
    who = "logreg_grad"
    n, D, ldx = _logreg_x(x, who)
    dev = x.device
    if r.dim() != 2 or r.dtype != torch.float32 or not r.is_contiguous() or r.device != dev or r.shape[0] != n:
        raise nat.NativeError(f"{who}: r must be a contiguous float32 tensor of shape ({n}, P) on x's device, got "
                              f"{r.dtype} {tuple(r.shape)}")
    P = r.shape[1]
    sp = 0 if splits is None else int(splits)
    g = _logreg_out(g, "g", (D, P), torch.float64, dev, who)
    ws = _logreg_ws(n, D, P, sp, ws, dev)
    _maybe_timed(stream, "logreg_grad", 2.0 * n * D * P, lambda s: call(
        "aw_logreg_grad", ptr(x) if n else None, n, ldx, D, ptr(r) if n else None, P, sp, ptr(ws), ws.numel(),
        ptr(g), s), info=lambda: (f"logreg_grad_kernel P={P} D={D}", 4.0 * n * D + 4.0 * n * P + 8.0 * D * P))
    return g


def rbf_gram_describe():
    """aw_rbf_gram_describe: (tile_a, tile_b, chunk_d) of the Gram kernel: rows of a and of b per workgroup, dims per
    chunk (the tests aim at the tile edges)."""
    v = [ctypes.c_int(0) for _ in range(3)]
    call("aw_rbf_gram_describe", *[ctypes.byref(c) for c in v])
    return tuple(int(c.value) for c in v)


def _rows(t, nm, who):
    if t.dim() != 2 or t.dtype != torch.float32 or (t.shape[1] > 1 and t.stride(1) != 1) or not t.is_cuda:
        raise nat.NativeError(f"{who}: {nm} must be a 2-d float32 device tensor with contiguous rows, got "
                              f"{t.dtype} {tuple(t.shape)} strides {tuple(t.stride())}")
    n, D = t.shape
    return n, D, (max(t.stride(0), D) if n > 1 else D)


def rbf_gram(a, b, gamma, k=None, stream=None):
    """aw_rbf_gram: k (na, nb) f32 = exp(-gamma |a_i - b_j|^2) with the squared distance as aw_knn forms it (f32 norms
    and dots, the dots on the f32-input MFMA); see include/arcweld_amd.h.  a (na, D), b (nb, D): f32 device tensors
    with contiguous rows (any row stride >= D, any 4-byte aligned base); gamma: a float, passed as f32.  k: an optional
    f32 output with contiguous rows (row stride >= nb; its padding is not written).  The matrix of a set against itself
    is bit-symmetric.  The range of gamma is the library's to refuse."""
    who = "rbf_gram"
    na, D, lda = _rows(a, "a", who)
    nb, Db, ldb = _rows(b, "b", who)
    if Db != D or D < 1 or b.device != a.device:
        raise nat.NativeError(f"{who}: a has {D} features, b has {Db}; need the same D >= 1 on one device")
    if k is None:
        k = torch.empty((na, nb), dtype=torch.float32, device=a.device)
    if k.dim() != 2 or k.dtype != torch.float32 or tuple(k.shape) != (na, nb) or (nb > 1 and k.stride(1) != 1) \
            or k.device != a.device:
        raise nat.NativeError(f"{who}: k must be a float32 tensor of shape {(na, nb)} with contiguous rows on a's "
                              f"device, got {k.dtype} {tuple(k.shape)} strides {tuple(k.stride())}")
    ldk = max(k.stride(0), nb) if na > 1 else nb
    _maybe_timed(stream, "rbf_gram", 2.0 * na * nb * D, lambda s: call(
        "aw_rbf_gram", ptr(a) if na else None, na, lda, ptr(b) if nb else None, nb, ldb, D, float(gamma),
        ptr(k) if na and nb else None, ldk, s),
        info=lambda: (f"rbf_gram_kernel D={D}", 4.0 * (na + nb) * D + 4.0 * na * nb))
    return k


def svm_describe():
    """aw_svm_describe: (threads, rows_per_thread, max_n, max_p) of the SMO kernel: the threads of the one workgroup a
    problem gets, the rows each owns at max_n, the row and problem limits."""
    v = [ctypes.c_int(0) for _ in range(4)]
    call("aw_svm_describe", *[ctypes.byref(c) for c in v])
    return tuple(int(c.value) for c in v)


def svm_smo(k, y, C, tol, max_iter, alpha=None, grad=None, n_iter=None, gap=None, stream=None):
    """aw_svm_smo: at most max_iter further SMO iterations on each of P <= 32 C-SVC duals over one kernel matrix; see
    include/arcweld_amd.h.  k (n, n): symmetric f32 device tensor with contiguous rows (row stride >= n); y (P, n)
    int32 in {-1, 0, +1} (0: the row takes no part); C: P positive floats (a number or a sequence; read on the host).
    alpha, grad (P, n) f64 are the state, updated in place; None starts a solve (alpha = 0, grad = -1).  n_iter (P)
    int64 is incremented (None: zeros), gap (P) f64 receives m - M.  Returns (alpha, grad, n_iter, gap).  A launch
    neither allocates nor synchronises; the ranges of C, tol and max_iter are the library's to refuse."""
    who = "svm_smo"
    if k.dim() != 2 or k.dtype != torch.float32 or k.shape[0] != k.shape[1] or not k.is_cuda \
            or (k.shape[1] > 1 and k.stride(1) != 1):
        raise nat.NativeError(f"{who}: k must be a square 2-d float32 device tensor with contiguous rows, got "
                              f"{k.dtype} {tuple(k.shape)} strides {tuple(k.stride())}")
    n, dev = k.shape[0], k.device
    ldk = max(k.stride(0), n) if n > 1 else n
    if y.dim() != 2 or y.dtype != torch.int32 or y.shape[1] != n or not y.is_contiguous() or y.device != dev:
        raise nat.NativeError(f"{who}: y must be a contiguous int32 tensor of shape (P, {n}) on k's device, got "
                              f"{y.dtype} {tuple(y.shape)}")
    P = y.shape[0]
    Cs = [float(C)] * P if isinstance(C, (int, float)) else [float(c) for c in C]
    if len(Cs) != P:
        raise nat.NativeError(f"{who}: C has {len(Cs)} values for {P} problems")
    if alpha is None:
        alpha = torch.zeros((P, n), dtype=torch.float64, device=dev)
    if grad is None:
        grad = torch.full((P, n), -1.0, dtype=torch.float64, device=dev)
    if n_iter is None:
        n_iter = torch.zeros(P, dtype=torch.int64, device=dev)
    if gap is None:
        gap = torch.empty(P, dtype=torch.float64, device=dev)
    for nm, t, shape, dt in (("alpha", alpha, (P, n), torch.float64), ("grad", grad, (P, n), torch.float64),
                             ("n_iter", n_iter, (P,), torch.int64), ("gap", gap, (P,), torch.float64)):
        if t.dtype != dt or tuple(t.shape) != shape or not t.is_contiguous() or t.device != dev:
            raise nat.NativeError(f"{who}: {nm} must be a contiguous {dt} tensor of shape {shape} on k's device")
    Ca = (ctypes.c_double * max(P, 1))(*Cs)        # a host array: read before the call returns
    _maybe_timed(stream, "svm_smo", 0.0, lambda s: call(
        "aw_svm_smo", ptr(k) if n else None, n, ldk, ptr(y) if n else None, ctypes.cast(Ca, ctypes.c_void_p), P,
        float(tol), int(max_iter), ptr(alpha) if n else None, ptr(grad) if n else None, ptr(n_iter), ptr(gap), s),
        info=lambda: (f"svm_smo_kernel n={n} P={P}", 0.0))
    return alpha, grad, n_iter, gap


def ts_describe():
    """aw_ts_describe: (tile_t, tile_c, chunk_c) of the TS2Vec convolution kernel: time steps and output channels per
    workgroup, input channels per chunk (the tests aim at the tile edges)."""
    v = [ctypes.c_int(0) for _ in range(3)]
    call("aw_ts_describe", *[ctypes.byref(c) for c in v])
    return tuple(int(c.value) for c in v)


def _ts_act(t, nm, rows, width, who, dev):
    if t is not None and (t.dtype != torch.float32 or tuple(t.shape) != (rows, width) or not t.is_contiguous()
                          or t.device != dev):
        raise nat.NativeError(f"{who}: {nm} must be a contiguous float32 tensor of shape {(rows, width)} on the "
                              f"input's device, got {t.dtype} {tuple(t.shape)}")


def ts_input_fc(x, w, bias, mask=None, out=None, out_gelu=None, stream=None):
    """aw_ts_input_fc: the TS2Vec encoder's input projection with its NaN / mask zeroing.  x (rows, cin) f32 (NaN =
    missing), w (hidden, cin), bias (hidden,), mask (rows,) uint8 or bool (0 = zero the row), all contiguous on one
    device.  Writes out and out_gelu (rows, hidden) f32 -- the projected rows and their exact-erf GELU -- and returns
    them; x is not modified.  The ranges of cin and hidden are the library's to refuse."""
    who = "ts_input_fc"
    if x.dim() != 2 or x.dtype != torch.float32 or not x.is_contiguous() or not x.is_cuda:
        raise nat.NativeError(f"{who}: x must be a contiguous (rows, cin) float32 device tensor")
    rows, cin = x.shape
    dev = x.device
    if w.dim() != 2 or w.shape[1] != cin or w.dtype != torch.float32 or not w.is_contiguous() or w.device != dev:
        raise nat.NativeError(f"{who}: w must be a contiguous (hidden, {cin}) float32 tensor on x's device")
    hidden = w.shape[0]
    if bias.dtype != torch.float32 or tuple(bias.shape) != (hidden,) or not bias.is_contiguous() or bias.device != dev:
        raise nat.NativeError(f"{who}: bias must be a contiguous float32 tensor of {hidden} elements on x's device")
    if mask is not None:
        if (mask.dtype not in (torch.uint8, torch.bool) or tuple(mask.shape) != (rows,) or not mask.is_contiguous()
                or mask.device != dev):
            raise nat.NativeError(f"{who}: mask must be a contiguous uint8 / bool tensor of {rows} elements on x's "
                                  f"device")
    if out is None:
        out = torch.empty((rows, hidden), dtype=torch.float32, device=dev)
    if out_gelu is None:
        out_gelu = torch.empty((rows, hidden), dtype=torch.float32, device=dev)
    _ts_act(out, "out", rows, hidden, who, dev)
    _ts_act(out_gelu, "out_gelu", rows, hidden, who, dev)
    call("aw_ts_input_fc", ptr(x), ptr(mask), ptr(w), ptr(bias), rows, cin, hidden, ptr(out), ptr(out_gelu),
         stream_ptr(stream))
    return out, out_gelu


def ts_conv(x, w, bias, batch, T, dilation, resid=None, out=None, out_gelu=None, pool=None, stream=None):
    """aw_ts_conv: one dilated convolution of the TS2Vec encoder over (batch * T, cin) f32 activations (row b * T + t
    = step t of sequence b).  w (taps, cout, cin) f32, taps 3 or 1 (the pointwise projection), bias (cout,).
    v = conv + bias (+ resid (batch * T, cout)); out = v, out_gelu = gelu(v), pool (batch, cout) = max over t of v: the
    caller passes the tensors it wants written, at least one.  No tap reads another sequence's rows.  The ranges of
    T, the widths, taps, dilation and batch are the library's to refuse (NativeError, nothing launched)."""
    who = "ts_conv"
    batch, T, dilation = int(batch), int(T), int(dilation)
    if x.dim() != 2 or x.dtype != torch.float32 or not x.is_contiguous() or not x.is_cuda or x.shape[0] != batch * T:
        raise nat.NativeError(f"{who}: the input must be a contiguous (batch * T = {batch * T}, cin) float32 device "
                              f"tensor, got {x.dtype} {tuple(x.shape)}")
    rows, cin = x.shape
    dev = x.device
    if w.dim() != 3 or w.shape[2] != cin or w.dtype != torch.float32 or not w.is_contiguous() or w.device != dev:
        raise nat.NativeError(f"{who}: w must be a contiguous (taps, cout, {cin}) float32 tensor on the input's device")
    taps, cout = w.shape[0], w.shape[1]
    if bias.dtype != torch.float32 or tuple(bias.shape) != (cout,) or not bias.is_contiguous() or bias.device != dev:
        raise nat.NativeError(f"{who}: bias must be a contiguous float32 tensor of {cout} elements on the input's "
                              f"device")
    _ts_act(resid, "resid", rows, cout, who, dev)
    _ts_act(out, "out", rows, cout, who, dev)
    _ts_act(out_gelu, "out_gelu", rows, cout, who, dev)
    _ts_act(pool, "pool", batch, cout, who, dev)
    ws = None
    if pool is not None:
        lib = nat.load()
        ws_bytes = lib.aw_ts_pool_workspace(batch, T, cout)
        if ws_bytes < 0:
            raise nat.NativeError(f"aw_ts_pool_workspace failed ({ws_bytes}): "
                                  f"{lib.aw_last_error().decode(errors='replace')}")
        ws = torch.empty(max(ws_bytes // 4, 4), dtype=torch.float32, device=dev)
    live = sum(1 for k in range(taps) if taps == 1 or abs(k - 1) * dilation < T)
    _maybe_timed(stream, "ts_conv", 2.0 * rows * cout * cin * live, lambda s: call(
        "aw_ts_conv", ptr(x), ptr(w), ptr(bias), ptr(resid), batch, T, cin, cout, taps, dilation, ptr(out),
        ptr(out_gelu), ptr(pool), ptr(ws), s),
        info=lambda: (f"ts_conv_kernel taps={taps} cin={cin} cout={cout} d={dilation}",
                      4.0 * rows * (cin + cout * sum(t is not None for t in (resid, out, out_gelu)))))
    return out, out_gelu, pool


# ------------------------------------------------------------------------------------------ TS2Vec loss
NCE_MAX_ROWS, NCE_MAX_GROUPS, NCE_MAX_WIDTH = nat.AW_NCE_MAX_ROWS, nat.AW_NCE_MAX_GROUPS, nat.AW_NCE_MAX_WIDTH
NCE_LAYOUTS = ("temporal", "instance")


def nce_describe():
    """aw_nce_describe: (rows per tile, dims per chunk, output columns per backward slab) of the loss kernels."""
    v = [ctypes.c_int(0) for _ in range(3)]
    call("aw_nce_describe", *[ctypes.byref(c) for c in v])
    return tuple(int(c.value) for c in v)


def _nce_geometry(z1, z2, layout, who):
    """(groups, n, c, group stride, row stride) of the paired InfoNCE over (B, T, C) inputs; what the library would
    refuse is a ValueError here, before any launch (and before the device is looked at)."""
    if layout not in NCE_LAYOUTS:
        raise ValueError(f"{who}: layout must be one of {NCE_LAYOUTS}, got {layout!r}")
    for nm, z in (("z1", z1), ("z2", z2)):
        if not isinstance(z, torch.Tensor) or z.dim() != 3 or z.dtype != torch.float32:
            raise ValueError(f"{who}: {nm} must be a (B, T, C) float32 tensor, got "
                             f"{(z.dtype, tuple(z.shape)) if isinstance(z, torch.Tensor) else type(z).__name__}")
    if z1.shape != z2.shape:
        raise ValueError(f"{who}: z1 {tuple(z1.shape)} and z2 {tuple(z2.shape)} differ in shape")
    B, T, C = z1.shape
    if C % 16 or not 16 <= C <= NCE_MAX_WIDTH:
        raise ValueError(f"{who}: C = {C} is not a multiple of 16 in 16..{NCE_MAX_WIDTH}")
    if B < 1 or T < 1:
        raise ValueError(f"{who}: empty input {tuple(z1.shape)}")
    groups, n = (B, T) if layout == "temporal" else (T, B)
    if 2 * n > NCE_MAX_ROWS:
        raise ValueError(f"{who}: a {layout} group has 2 * {n} rows, above {NCE_MAX_ROWS}")
    if T * C >= 1 << 22:
        raise ValueError(f"{who}: T * C = {T * C} must stay below 2^22")
    if not z1.is_contiguous() or not z2.is_contiguous():
        raise ValueError(f"{who}: z1 and z2 must be contiguous")
    if z1.is_cuda and z1.device != z2.device:
        raise ValueError(f"{who}: z1 and z2 are on different devices")
    return (groups, n, C, T * C, C) if layout == "temporal" else (groups, n, C, C, T * C)


def _nce_chunks(groups, layout):
    """(first group, count) per launch: only the temporal layout (groups = B) can exceed the per-launch bound, and
    its groups are contiguous slabs."""
    return [(o, min(NCE_MAX_GROUPS, groups - o)) for o in range(0, groups, NCE_MAX_GROUPS)]


def nce_rows_fwd(z1, z2, layout, lse=None, row_loss=None, stream=None):
    """aw_nce_rows_fwd: the paired InfoNCE of contiguous (B, T, C) f32 device tensors, per row.  layout 'temporal':
    groups = B sequences of 2 T rows; 'instance': groups = T steps of 2 B rows.  Returns (lse, row_loss), each
    (groups, 2 n) f32: rows 0..n-1 of a group are z1's, n..2n-1 z2's."""
    who = "nce_rows_fwd"
    groups, n, c, gs, rs = _nce_geometry(z1, z2, layout, who)
    p1, p2 = ptr(z1), ptr(z2)
    dev = z1.device
    if lse is None:
        lse = torch.empty((groups, 2 * n), dtype=torch.float32, device=dev)
    if row_loss is None:
        row_loss = torch.empty((groups, 2 * n), dtype=torch.float32, device=dev)
    _ts_act(lse, "lse", groups, 2 * n, who, dev)
    _ts_act(row_loss, "row_loss", groups, 2 * n, who, dev)
    for o, m in _nce_chunks(groups, layout):
        _maybe_timed(stream, "nce_rows_fwd", 2.0 * m * (2 * n) ** 2 * c, lambda s: call(
            "aw_nce_rows_fwd", p1 + 4 * o * gs, p2 + 4 * o * gs, m, n, c, gs, rs, ptr(lse[o:o + m]),
            ptr(row_loss[o:o + m]), s),
            info=lambda: (f"nce_fwd_kernel {layout} n={n} c={c}", 4.0 * m * 2 * n * (c + 2)))
    return lse, row_loss


def nce_rows_bwd(z1, z2, layout, lse, scale, dz1, dz2, accumulate=False, stream=None):
    """aw_nce_rows_bwd: dz (+)= scale * d(sum of row_loss)/dz with the forward's lse; dz1 / dz2 are contiguous f32
    tensors of z1's shape, overwritten, or added to with accumulate."""
    who = "nce_rows_bwd"
    groups, n, c, gs, rs = _nce_geometry(z1, z2, layout, who)
    p1, p2 = ptr(z1), ptr(z2)
    dev = z1.device
    _ts_act(lse, "lse", groups, 2 * n, who, dev)
    for nm, t in (("dz1", dz1), ("dz2", dz2)):
        if (t is None or t.dtype != torch.float32 or t.shape != z1.shape or not t.is_contiguous()
                or t.device != dev):
            raise nat.NativeError(f"{who}: {nm} must be a contiguous float32 tensor of shape {tuple(z1.shape)} on the "
                                  f"inputs' device")
    d1, d2 = ptr(dz1), ptr(dz2)
    for o, m in _nce_chunks(groups, layout):
        _maybe_timed(stream, "nce_rows_bwd", 2.0 * m * (2 * n) ** 2 * c * (1 + -(-c // 128)), lambda s: call(
            "aw_nce_rows_bwd", p1 + 4 * o * gs, p2 + 4 * o * gs, m, n, c, gs, rs, ptr(lse[o:o + m]), float(scale),
            d1 + 4 * o * gs, d2 + 4 * o * gs, int(bool(accumulate)), s),
            info=lambda: (f"nce_bwd_kernel {layout} n={n} c={c}", 4.0 * m * 2 * n * (2 * c + 1)))
    return dz1, dz2


def _pool2_check(x, who):
    if not isinstance(x, torch.Tensor) or x.dim() != 3 or x.dtype != torch.float32 or not x.is_contiguous():
        raise ValueError(f"{who}: the input must be a contiguous (B, T, C) float32 tensor")
    B, T, C = x.shape
    if C % 16 or not 16 <= C <= NCE_MAX_WIDTH:
        raise ValueError(f"{who}: C = {C} is not a multiple of 16 in 16..{NCE_MAX_WIDTH}")
    if not 2 <= T <= nat.AW_TS_MAX_T:
        raise ValueError(f"{who}: T = {T} outside 2..{nat.AW_TS_MAX_T}")
    return B, T, C


def ts_pool2_fwd(x, out=None, stream=None):
    """aw_ts_pool2_fwd: max over pairs of time steps, (B, T, C) -> (B, T // 2, C) (an odd last step is dropped)."""
    who = "ts_pool2_fwd"
    B, T, C = _pool2_check(x, who)
    px = ptr(x)
    if out is None:
        out = torch.empty((B, T // 2, C), dtype=torch.float32, device=x.device)
    if out.dtype != torch.float32 or tuple(out.shape) != (B, T // 2, C) or not out.is_contiguous() \
            or out.device != x.device:
        raise nat.NativeError(f"{who}: out must be a contiguous float32 tensor of shape {(B, T // 2, C)}")
    for o in range(0, B, nat.AW_TS_MAX_BATCH):
        m = min(nat.AW_TS_MAX_BATCH, B - o)
        call("aw_ts_pool2_fwd", px + 4 * o * T * C, m, T, C, ptr(out[o:o + m]), stream_ptr(stream))
    return out


def ts_pool2_bwd(x, dout, din, stream=None):
    """aw_ts_pool2_bwd: din[b, 2 t + k] += dout[b, t] at the step k the forward took from x (the first on a tie)."""
    who = "ts_pool2_bwd"
    B, T, C = _pool2_check(x, who)
    px = ptr(x)
    if dout.dtype != torch.float32 or tuple(dout.shape) != (B, T // 2, C) or not dout.is_contiguous() \
            or dout.device != x.device:
        raise nat.NativeError(f"{who}: dout must be a contiguous float32 tensor of shape {(B, T // 2, C)}")
    if din.dtype != torch.float32 or din.shape != x.shape or not din.is_contiguous() or din.device != x.device:
        raise nat.NativeError(f"{who}: din must be a contiguous float32 tensor of shape {tuple(x.shape)}")
    pd = ptr(din)
    for o in range(0, B, nat.AW_TS_MAX_BATCH):
        m = min(nat.AW_TS_MAX_BATCH, B - o)
        call("aw_ts_pool2_bwd", px + 4 * o * T * C, ptr(dout[o:o + m]), m, T, C, pd + 4 * o * T * C,
             stream_ptr(stream))
    return din


# ------------------------------------------------------------------------------------------ layouts
def patchify(x, P, out, stream=None):
    B, L, C = x.shape
    call("aw_patchify", ptr(x), B, L, C, P, ptr(out), out.stride(0), dtype_code(out.dtype), stream_ptr(stream))


def weight_relayout(W, O, I, k, tap, mode, out, ldo=0, stream=None):
    _dense(W, "weight_relayout")
    call("aw_weight_relayout", ptr(W), O, I, k, tap, mode, ptr(out), ldo, dtype_code(out.dtype), stream_ptr(stream))


RELAYOUT_MAX_JOBS = nat.AW_RELAYOUT_MAX_JOBS


def _dense(W, who):
    if not W.is_contiguous():
        raise nat.NativeError(f"{who}: the source weight must be contiguous (got strides {tuple(W.stride())})")


def weight_relayout_batch(jobs, stream=None):
    """Many weight_relayout calls in one launch per output dtype.  jobs: (W, O, I, k, tap, mode, out[, ldo]);
    mode 5 is a plain cast of O*I elements."""
    by_dtype = {}
    for jb in jobs:
        by_dtype.setdefault(jb[6].dtype, []).append(jb)
    for dt, js in by_dtype.items():
        for c0 in range(0, len(js), RELAYOUT_MAX_JOBS):
            chunk = js[c0:c0 + RELAYOUT_MAX_JOBS]
            arr = (nat.RelayoutJob * len(chunk))()
            for r, jb in zip(arr, chunk):
                W, O, I, k, tap, mode, out = jb[:7]
                _dense(W, "weight_relayout_batch")
                r.W, r.out = ptr(W), ptr(out)
                r.O, r.I, r.k, r.tap, r.mode = int(O), int(I), int(k), int(tap), int(mode)
                r.ldo = int(jb[7]) if len(jb) > 7 else 0
            call("aw_weight_relayout_batch", arr, len(chunk), dtype_code(dt), stream_ptr(stream))


def weight_grad_scatter(g, O, I, k, tap, mode, G, stream=None):
    call("aw_weight_grad_scatter", ptr(g), O, I, k, tap, mode, g.stride(0), ptr(G), stream_ptr(stream))


def cast(x, out, stream=None):
    call("aw_cast", ptr(x), x.numel(), ptr(out), dtype_code(out.dtype), stream_ptr(stream))


def bn_finalize(colstats, n, H, gamma, beta, rm, rv, nbt, eps, momentum, training, stats, stream=None):
    call("aw_bn_finalize", ptr(colstats), n, H, ptr(gamma), ptr(beta), ptr(rm), ptr(rv), ptr(nbt), float(eps),
         float(momentum), int(training), ptr(stats), stream_ptr(stream))


def unpatch_head_fwd(y, Q, stats, w2, b2, x_hat, stream=None):
    """y (R, H) f32 or bf16 (the ConvT output in the bf16 operand mode)."""
    R, H = y.shape
    call("aw_unpatch_head_fwd", ptr(y), dtype_code(y.dtype), R, H, Q, ptr(stats), ptr(w2), ptr(b2), ptr(x_hat),
         stream_ptr(stream))


def unpatch_head_bwd1(y, Q, stats, w2, g_xhat, gsums, gw2, gb2, ggamma, gbeta, stream=None):
    R, H = y.shape
    call("aw_unpatch_head_bwd1", ptr(y), dtype_code(y.dtype), R, H, Q, ptr(stats), ptr(w2), ptr(g_xhat), ptr(gsums),
         ptr(gw2), ptr(gb2), ptr(ggamma), ptr(gbeta), stream_ptr(stream))


def unpatch_head_bwd2(y, Q, stats, w2, g_xhat, gsums, training, g_y, db_y, stream=None):
    R, H = y.shape
    call("aw_unpatch_head_bwd2", ptr(y), dtype_code(y.dtype), R, H, Q, ptr(stats), ptr(w2), ptr(g_xhat),
         ptr(gsums), int(training), ptr(g_y), dtype_code(g_y.dtype), ptr(db_y), stream_ptr(stream))


def unpatch_head_fwd_bwd1(y, Q, stats, w2, b2, x, gscale, x_hat, g_xhat, sqerr, gsums, gw2, gb2, ggamma, gbeta,
                          stream=None):
    """Fused training-step head: forward + MSE value / gradient + backward pass 1 in one read of y (H == 512).
    The kernel reads x, x_hat and g_xhat as R*5 contiguous f32 values (its buffer range check would silently
    return zeros for a shorter x), so their sizes are checked here."""
    R, H = y.shape
    for nm, t in (("x", x), ("x_hat", x_hat), ("g_xhat", g_xhat)):
        if t.dtype != torch.float32 or not t.is_contiguous() or t.numel() != R * 5:
            raise nat.NativeError(f"unpatch_head_fwd_bwd1: {nm} must be a contiguous float32 tensor of R*5 = {R * 5} "
                                  f"elements (got {tuple(t.shape)} {t.dtype}, contiguous={t.is_contiguous()})")
    call("aw_unpatch_head_fwd_bwd1", ptr(y), dtype_code(y.dtype), R, H, Q, ptr(stats), ptr(w2), ptr(b2), ptr(x),
         ptr(gscale), ptr(x_hat), ptr(g_xhat), ptr(sqerr), ptr(gsums), ptr(gw2), ptr(gb2), ptr(ggamma), ptr(gbeta),
         stream_ptr(stream))


def head_bf16_ok(H):
    """The head passes take a bf16 ConvT output when H is a power of two in 64..2048 (aw_unpatch_head_*)."""
    return 64 <= H <= 2048 and H & (H - 1) == 0


def mse_fwd(a, b, sqerr, stream=None):
    call("aw_mse_fwd", ptr(a), ptr(b), a.numel(), ptr(sqerr), stream_ptr(stream))


def mse_bwd(a, b, g, ga, stream=None):
    call("aw_mse_bwd", ptr(a), ptr(b), a.numel(), ptr(g), ptr(ga), stream_ptr(stream))


def scalar_add(a, b, out, stream=None):
    call("aw_scalar_add", ptr(a), ptr(b), ptr(out), stream_ptr(stream))


def mse_finalize(sqerr, numel, out, stream=None):
    call("aw_mse_finalize", ptr(sqerr), int(numel), ptr(out), stream_ptr(stream))


def mse_finalize_add(sqerr, numel, addend, out, total, stream=None):
    """out = sqerr / numel and total = out + addend (device scalars), in one launch."""
    call("aw_mse_finalize_add", ptr(sqerr), int(numel), ptr(addend), ptr(out), ptr(total), stream_ptr(stream))


# ------------------------------------------------------------------------------------------ optimizer
def radam_step(param, grad, m, v, seg_off, seg_len, seg_wd, seg_active, nseg, total, step, lr, beta1, beta2, eps,
               gscale=None, stream=None, step_ptr=None, ops=None, zero_grad=False):
    """aw_radam_step; with `ops` (device table of aw_operand_desc, AW_OPS_PER_SEG per segment) the update also
    writes the operand copies of the updated weights.  zero_grad: the updated elements' gradients are zeroed in the
    same pass."""
    call("aw_radam_step", ptr(param), ptr(grad), ptr(m), ptr(v), ptr(seg_off), ptr(seg_len), ptr(seg_wd),
         ptr(seg_active), int(nseg), int(total), int(step), float(lr), float(beta1), float(beta2), float(eps),
         ptr(gscale), ptr(step_ptr), ctypes.cast(ptr(ops), ctypes.POINTER(nat.OperandDesc)), int(bool(zero_grad)),
         stream_ptr(stream))


def counter_add_snapshot(counter, snapshot, v=1, stream=None, zero=None):
    """counter += v and snapshot = the new value, in one launch; `zero` (a contiguous float64 tensor) is zeroed by
    the same launch."""
    if zero is not None and (zero.dtype != torch.float64 or not zero.is_contiguous()):
        raise nat.NativeError("counter_add_snapshot: zero must be a contiguous float64 tensor")
    call("aw_counter_add", ptr(counter), int(v), ptr(snapshot), ptr(zero), zero.numel() if zero is not None else 0,
         stream_ptr(stream))


def counter_add(counter, v=1, stream=None):
    """counter (int64 device tensor) += v on the stream (per-step RNG / optimizer-step counters)."""
    call("aw_counter_add", ptr(counter), int(v), None, None, 0, stream_ptr(stream))


NORM_WS = nat.AW_NORM_WS


def grad_norm_clip(grad, seg_off, seg_len, seg_active, nseg, max_norm, ws, out_norm, out_coef, stream=None):
    if ws.numel() < NORM_WS or ws.dtype != torch.float64:
        raise nat.NativeError(f"grad_norm_clip: ws must hold {NORM_WS} float64")
    call("aw_grad_norm_clip", ptr(grad), ptr(seg_off), ptr(seg_len), ptr(seg_active), int(nseg), grad.numel(),
         float(max_norm), ptr(ws), ptr(out_norm), ptr(out_coef), stream_ptr(stream))


def scale_(x, s, stream=None):
    call("aw_scale", ptr(x), x.numel(), ptr(s), stream_ptr(stream))


# ---------------------------------------------------------------------------------------- transformer
def layernorm_fwd(x, w, b, eps, y, mean, rstd, stream=None):
    R, D = x.shape
    call("aw_layernorm_fwd", ptr(x), R, D, ptr(w), ptr(b), float(eps), ptr(y), dtype_code(y.dtype), ptr(mean),
         ptr(rstd), stream_ptr(stream))


def layernorm_bwd(x, dy, w, mean, rstd, dx, accumulate, dw, db, dx2=None, drop=(0.0, 0), stream=None,
                  seed_ptr=None):
    R, D = x.shape
    call("aw_layernorm_bwd", ptr(x), ptr(dy), R, D, ptr(w), ptr(mean), ptr(rstd), ptr(dx), int(accumulate), ptr(dw),
         ptr(db), ptr(dx2), dtype_code(dx2.dtype) if dx2 is not None else AW_F32, float(drop[0]),
         int(drop[1]) & 0xFFFFFFFFFFFFFFFF, ptr(seed_ptr), stream_ptr(stream))


def class_head_fwd(xf, B, T, w1, b1, W2, b2, s, out, stream=None):
    call("aw_class_head_fwd", ptr(xf), B, T, xf.shape[-1], ptr(w1), ptr(b1), ptr(W2), ptr(b2), ptr(s), ptr(out),
         stream_ptr(stream))


def class_head_bwd(xf, s, dout, B, T, w1, W2, dxf, dw1, db1, dW2, db2, stream=None):
    call("aw_class_head_bwd", ptr(xf), ptr(s), ptr(dout), B, T, xf.shape[-1], ptr(w1), ptr(W2), ptr(dxf), ptr(dw1),
         ptr(db1), ptr(dW2), ptr(db2), stream_ptr(stream))


def embed_fwd(ids, wtok, pe, x, stream=None):
    B, T = ids.shape
    call("aw_embed_fwd", ptr(ids), B, T, wtok.shape[1], ptr(wtok), ptr(pe), ptr(x), stream_ptr(stream))


def embed_ln_fwd(ids, wtok, pe, x, w, b, eps, y, mean, rstd, stream=None):
    """embed_fwd followed by layernorm_fwd(x, ...) in one launch (d_model 256/512/768/1024), bit-identical to the pair."""
    B, T = ids.shape
    call("aw_embed_ln_fwd", ptr(ids), B, T, wtok.shape[1], ptr(wtok), ptr(pe), ptr(x), ptr(w), ptr(b), float(eps),
         ptr(y), dtype_code(y.dtype), ptr(mean), ptr(rstd), stream_ptr(stream))


def embed_bwd(ids, dx, dwtok, stream=None, sort=True):
    """dwtok[ids[r]] += dx[r].  sort: the counting-sort form (aw_embed_bwd_sorted; scratch allocated here), else the
    atomic form."""
    B, T = ids.shape
    if not sort:
        call("aw_embed_bwd", ptr(ids), B, T, dwtok.shape[1], ptr(dx), ptr(dwtok), stream_ptr(stream))
        return
    V = dwtok.shape[0]
    work = torch.empty(V + 1 + B * T, device=dx.device, dtype=torch.int32)
    call("aw_embed_bwd_sorted", ptr(ids), B, T, dwtok.shape[1], V, ptr(dx), ptr(dwtok), ptr(work),
         stream_ptr(stream))


EMBED_SORT_MAX_V = 15360


def embed_sort(ids, V, work, stream=None):
    """The counting sort half of embed_bwd (work: V + 1 + ids.numel() int32)."""
    call("aw_embed_sort", ptr(ids), ids.numel(), V, ptr(work), stream_ptr(stream))


def embed_bwd_segsum(work, dx, dwtok, stream=None):
    """The table-row sums half of embed_bwd, from embed_sort's work."""
    call("aw_embed_bwd_segsum", ptr(work), dwtok.shape[0], dwtok.shape[1], ptr(dx), ptr(dwtok), stream_ptr(stream))


def attn_flops(B, T, n_head, d):
    """Algorithmic FLOPs of the causal attention forward: QK^T and PV over the T(T+1)/2 causal pairs per head."""
    return 4.0 * B * n_head * (T * (T + 1) / 2) * (d // n_head)


def _maybe_timed(stream, tag, flops, fn, info=None):
    """Launch fn(stream pointer); when profiling, under _timed with info() = (kernel name, algorithmic HBM bytes),
    evaluated only then (the byte count walks every tensor of the launch)."""
    if PROFILE is None:
        fn(stream_ptr(stream))
        return
    s = stream if stream is not None else torch.cuda.current_stream()
    _timed(s, fn, flops, tag, *(info() if info is not None else ()))


def _attn_drop(drop, seed_ptr):
    """(drop_p, drop_seed, seed_ptr) of the attention entry points; no dropout passes neither seed."""
    if drop[0] > 0:
        return float(drop[0]), int(drop[1]) & 0xFFFFFFFFFFFFFFFF, ptr(seed_ptr)
    return 0.0, 0, None


def attn_fwd(qkv, B, T, n_head, d, y, lse, drop=(0.0, 0), seed_ptr=None, stream=None):
    """drop = (p, seed): attention-probability dropout; p = 0 is none."""
    _maybe_timed(stream, "attn_fwd", attn_flops(B, T, n_head, d), lambda sp: call(
        "aw_attn_fwd", ptr(qkv), B, T, n_head, d, dtype_code(qkv.dtype), ptr(y), ptr(lse), *_attn_drop(drop, seed_ptr),
        sp))


def attn_bwd(qkv, y, dy, lse, B, T, n_head, d, dqkv, ws, drop=(0.0, 0), seed_ptr=None, stream=None):
    """Algorithmic FLOPs: twice the forward (dQ, dK, dV, dP; the recomputed S is not counted)."""
    _maybe_timed(stream, "attn_bwd", 2.0 * attn_flops(B, T, n_head, d), lambda sp: call(
        "aw_attn_bwd", ptr(qkv), ptr(y), ptr(dy), ptr(lse), B, T, n_head, d, dtype_code(qkv.dtype), ptr(dqkv),
        ptr(ws), *_attn_drop(drop, seed_ptr), sp))


# ------------------------------------------------------------------------------ ResBlock BatchNorm
def bn_group_stats(h, G, sums, stream=None):
    N, H = h.shape
    call("aw_bn_group_stats", ptr(h), N, H, int(G), ptr(sums), stream_ptr(stream))


def bn_group_finalize(sums, n, H, G, bn, training, stats, stream=None):
    """stats [4][G][H] from the sums (training) or the running statistics (eval) of nn.BatchNorm1d ``bn``."""
    mom = bn.momentum if bn.momentum is not None else 0.1
    call("aw_bn_group_finalize", ptr(sums) if training else None, int(n), int(H), int(G), ptr(bn.weight),
         ptr(bn.bias), ptr(bn.running_mean), ptr(bn.running_var), ptr(bn.num_batches_tracked) if training else None,
         float(bn.eps), float(mom), int(bool(training)), ptr(stats), stream_ptr(stream))


def bn_apply(h, G, stats, mode, out, op=None, resid=None, drop=(0.0, 0), seed_ptr=None, stream=None):
    N, H = h.shape
    call("aw_bn_apply", ptr(h), N, H, int(G), ptr(stats), int(mode), ptr(resid), float(drop[0]), int(drop[1]),
         ptr(seed_ptr), ptr(out), ptr(op), dtype_code(op.dtype) if op is not None else AW_F32, stream_ptr(stream))


def bn_bwd_reduce(h, G, stats, g_in, sums, drop=(0.0, 0), seed_ptr=None, stream=None):
    N, H = h.shape
    call("aw_bn_bwd_reduce", ptr(h), N, H, int(G), ptr(stats), ptr(g_in), float(drop[0]), int(drop[1]),
         ptr(seed_ptr), ptr(sums), stream_ptr(stream))


def bn_bwd_apply(h, G, stats, g_in, sums, n, training, dh, dgamma=None, dbeta=None, drop=(0.0, 0), seed_ptr=None,
                 stream=None):
    N, H = h.shape
    call("aw_bn_bwd_apply", ptr(h), N, H, int(G), ptr(stats), ptr(g_in), float(drop[0]), int(drop[1]),
         ptr(seed_ptr), ptr(sums), int(n), int(bool(training)), ptr(dh), dtype_code(dh.dtype), ptr(dgamma),
         ptr(dbeta), stream_ptr(stream))


def attn_decode(qkv_new, B, n_new, pos0, n_head, d, kv_cache, y, stream=None):
    """KV-cache attention for n_new rows per sequence at positions pos0..; kv_cache (B, Tmax, 2d)."""
    if kv_cache.dtype != qkv_new.dtype or y.dtype != qkv_new.dtype or kv_cache.shape[-1] != 2 * d:
        raise nat.NativeError("attn_decode: qkv, cache and y share a dtype; cache rows are [K | V] (2d)")
    call("aw_attn_decode", ptr(qkv_new), B, n_new, pos0, n_head, d, dtype_code(qkv_new.dtype), ptr(kv_cache),
         kv_cache.shape[1], ptr(y), stream_ptr(stream))


def ce_fwd(logits, V, y, ignore_index, loss_sum, count, lse, stream=None):
    R = y.numel()
    call("aw_ce_fwd", ptr(logits), R, V, logits.stride(0), ptr(y), int(ignore_index), ptr(loss_sum), ptr(count),
         ptr(lse), stream_ptr(stream))


def ce_bwd(logits, V, y, ignore_index, lse, count, g, dlogits, stream=None):
    R = y.numel()
    call("aw_ce_bwd", ptr(logits), R, V, logits.stride(0), ptr(y), int(ignore_index), ptr(lse), ptr(count), ptr(g),
         ptr(dlogits), dlogits.stride(0), dtype_code(dlogits.dtype), stream_ptr(stream))


def ce_finalize(loss_sum, count, out, stream=None):
    call("aw_ce_finalize", ptr(loss_sum), ptr(count), ptr(out), stream_ptr(stream))


# ------------------------------------------------------------------------------ GRU recurrence
def gru_padded(H):
    """Hp of the GRU kernels' padded layout (include/arcweld_amd.h): H rounded up to a multiple of 32."""
    return (int(H) + 31) // 32 * 32


def _chk_gru(name, t, shape, dtype):
    if t is None:
        return
    if t.dtype != dtype or tuple(t.shape) != tuple(shape) or not t.is_contiguous():
        raise nat.NativeError(f"gru: {name} must be a contiguous {dtype} tensor of shape {tuple(shape)}, got "
                              f"{t.dtype} {tuple(t.shape)}")


def gru_pack_weights(w_hh, H, w_fwd=None, w_bwd=None, stream=None):
    """Zero-padded operand images of W_hh (3H, H): w_fwd [3][Hp][Hp], w_bwd [Hp][3*Hp] (either may be None)."""
    Hp = gru_padded(H)
    T = (w_fwd if w_fwd is not None else w_bwd).dtype
    _chk_gru("w_hh", w_hh, (3 * H, H), torch.float32)
    _chk_gru("w_fwd", w_fwd, (3, Hp, Hp), T)
    _chk_gru("w_bwd", w_bwd, (Hp, 3 * Hp), T)
    call("aw_gru_pack_weights", ptr(w_hh), int(H), dtype_code(T), ptr(w_fwd), ptr(w_bwd), stream_ptr(stream))


def gru_step_fwd(H, T, gi, b_hh, h, saved, w_fwd=None, h_prev_op=None, h_prev=None, h_op=None, stream=None):
    """aw_gru_step_fwd: one time step of one layer (T = the operand dtype; h_prev_op = h_prev = None: zero state)."""
    B, Hp = gi.shape[0], gru_padded(H)
    _chk_gru("gi", gi, (B, 3 * Hp), torch.float32)
    _chk_gru("b_hh", b_hh, (3 * H,), torch.float32)
    _chk_gru("h", h, (B, Hp), torch.float32)
    _chk_gru("saved", saved, (B, 4 * Hp), torch.float32)
    _chk_gru("h_prev_op", h_prev_op, (B, Hp), T)
    _chk_gru("h_prev", h_prev, (B, Hp), torch.float32)
    _chk_gru("h_op", h_op, (B, Hp), torch.bfloat16)
    _chk_gru("w_fwd", w_fwd, (3, Hp, Hp), T)
    call("aw_gru_step_fwd", B, int(H), dtype_code(T), ptr(h_prev_op), ptr(h_prev), ptr(w_fwd), ptr(gi), ptr(b_hh),
         ptr(h), ptr(h_op), ptr(saved), stream_ptr(stream))


def gru_step_bwd(H, T, saved, dh, dgi, dgh, w_bwd=None, dgh_next_op=None, dh_next=None, saved_next=None, dy=None,
                 h_prev=None, dgi_op=None, dgh_op=None, stream=None):
    """aw_gru_step_bwd: one time step of one layer's backward (the *_next arguments are step t+1's: all None at the
    last step)."""
    B, Hp = saved.shape[0], gru_padded(H)
    f32 = torch.float32
    _chk_gru("saved", saved, (B, 4 * Hp), f32)
    _chk_gru("saved_next", saved_next, (B, 4 * Hp), f32)
    for name, t in (("dh", dh), ("dh_next", dh_next), ("dy", dy), ("h_prev", h_prev)):
        _chk_gru(name, t, (B, Hp), f32)
    for name, t in (("dgi", dgi), ("dgh", dgh)):
        _chk_gru(name, t, (B, 3 * Hp), f32)
    for name, t in (("dgi_op", dgi_op), ("dgh_op", dgh_op)):
        _chk_gru(name, t, (B, 3 * Hp), torch.bfloat16)
    _chk_gru("dgh_next_op", dgh_next_op, (B, 3 * Hp), T)
    _chk_gru("w_bwd", w_bwd, (Hp, 3 * Hp), T)
    call("aw_gru_step_bwd", B, int(H), dtype_code(T), ptr(dgh_next_op), ptr(dh_next), ptr(saved_next), ptr(w_bwd),
         ptr(dy), ptr(saved), ptr(h_prev), ptr(dh), ptr(dgi), ptr(dgh), ptr(dgi_op), ptr(dgh_op), stream_ptr(stream))


def gru_bias_grad(dg, H, db, stream=None):
    """aw_gru_bias_grad: db (3H) += the column sums of the f32 gate gradients dg (rows, 3*Hp)."""
    rows = dg.shape[0]
    _chk_gru("dg", dg, (rows, 3 * gru_padded(H)), torch.float32)
    _chk_gru("db", db, (3 * H,), torch.float32)
    call("aw_gru_bias_grad", ptr(dg), rows, int(H), ptr(db), stream_ptr(stream))
