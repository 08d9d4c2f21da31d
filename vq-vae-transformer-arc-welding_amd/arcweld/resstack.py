"""The launches of a ResBlock stack (model/vq_vae_patch_embedd.py:60-74 inside CNNBlock :93-114), in one place.

A stack is R blocks x' = x + Drop(BN?(Conv2(GELU(BN?(Conv1(GELU x)))))) on token-major activations [N][H].  The
encoder's stack runs every token on its own (taps 1: only the centre tap of its k = 3 convs contributes), the decoder's
convolves along each window of S tokens (taps 3: the implicit conv GEMM, K = 3H).  ``Geometry`` holds everything that
differs between the two.  ``forward`` takes one of three routes -- the chain (the whole stack as one persistent launch,
csrc/reschain.hip), one GEMM per conv, or the BatchNorm blocks -- and returns a ``Saved`` record; ``backward`` takes
that record and returns the input gradient and the weight-gradient problems, which the caller issues.

Everything here works on plain tensors.  Where the weight operands come from is the caller's business: ``weights[r]``
(forward) and ``dweights[r]`` (backward) are looked up right before block r's launches, so a caller that builds them
per block (arcweld.modules) passes an object whose ``__getitem__`` launches the relayout.
"""
from __future__ import annotations

import torch

from . import kernels as K

F32 = torch.float32


def _centre_job(w, out):
    """Relayout job: the centre tap of a per-token encoder conv weight (O, I, 3) -> [O][I].  The weight is either
    the reference's contiguous layout or the optimizer's tap-major view (arcweld.optim.RAdam.declare_centre_tap),
    whose centre tap is already a contiguous [O][I] matrix."""
    O, I = w.shape[0], w.shape[1]
    c = w[:, :, 1]
    if w.is_contiguous():
        return (w, O, I, 3, 1, 0, out)
    if not c.is_contiguous():
        raise ValueError("encoder conv weight: unsupported layout")
    return (c, O, I, 1, 0, 0, out)


def _centre_grad(g):
    """Where the encoder conv weight-gradient GEMM writes: (C [O][ldc], col_map) for either weight layout."""
    O, I = g.shape[0], g.shape[1]
    if g.is_contiguous():
        return g.view(O, 3 * I), (0, 3, 1)
    c = g[:, :, 1]
    if not c.is_contiguous():
        raise ValueError("encoder conv gradient: unsupported layout")
    return c, (0, 1, 0)


def _conv3_job(w, mode, out):
    """Relayout job of a decoder k = 3 conv weight (mode 1: [O][3I] forward, mode 2: [3O][I] input gradient) for
    either storage order of the weight (contiguous (O, I, 3), or the optimizer's tap-major (O, 3, I))."""
    from .operands import OperandJob
    return OperandJob("", w, w.shape[0], w.shape[1], 3, 0, mode, out).relayout_job()


def _conv3_grad(g):
    """Where a decoder k = 3 conv weight-gradient GEMM (columns j*I + i) writes: (C [O][3I], col_map).  The
    reference's contiguous (O, I, 3) layout takes the columns through the (I, 3) column map; the optimizer's tap-major
    storage (arcweld.optim.RAdam.declare_tap_major, (O, 3, I)) is [O][3I] itself, written by contiguous atomics."""
    O, I = g.shape[0], g.shape[1]
    if g.is_contiguous():
        return g.view(O, 3 * I), (I, 3, 0)
    st = g.permute(0, 2, 1)
    if not st.is_contiguous():
        raise ValueError("decoder conv gradient: unsupported layout")
    return st.reshape(O, 3 * I), (0, 1, 0)


class Geometry:
    """What differs between the per-token stack (taps 1) and the k = 3 stack over windows of S tokens (taps 3)."""

    def __init__(self, taps, H, S):
        self.taps, self.H, self.S, self.Kd = taps, H, S, taps * H
        conv = lambda d, operand: dict(conv=(H, S, d, operand)) if taps == 3 else {}  # noqa: E731
        self.fwd, self.dgrad, self.wgrad = conv(1, 0), conv(-1, 0), conv(1, 1)    # aw_gemm's implicit conv forms
        self.G = S if taps == 1 else 1     # BatchNorm groups: per-token statistics, or over all B*S positions
        self.grad_target = _centre_grad if taps == 1 else _conv3_grad

    def fwd_job(self, w, out):
        """Relayout job of a conv weight into its forward operand [O][Kd]."""
        return _centre_job(w, out) if self.taps == 1 else _conv3_job(w, 1, out)

    def dgrad_job(self, w, out):
        """Relayout job of a k = 3 conv weight into its input-gradient operand [3O][I] (taps 1: the forward copy)."""
        return _conv3_job(w, 2, out)

    def wgrad_problem(self, A, B, gw, gb):
        """The weight-gradient GEMM of one conv (A: output gradient, B: input operand) accumulating into the
        parameter-shaped gw, with the bias gradient gb as its A-row-sum: a (A, B, M, N, K, kwargs) problem."""
        Cw, cm = self.grad_target(gw)
        return (A, B, self.H, self.Kd, A.shape[0], dict(a_trans=True, b_trans=True, C=Cw, accumulate=True, col_map=cm,
                                                        a_rowsum=gb, **self.wgrad))


def biases(convs):
    """``forward``'s biases of a stack given as its (conv1, conv2) module pairs."""
    return [(c1.bias, c2.bias) for c1, c2 in convs]


def grads(convs, slot):
    """``backward``'s grads(r, i) of the same pairs: the accumulators of block r's conv i (weight, then bias)."""
    return lambda r, i: (slot(convs[r][i].weight), slot(convs[r][i].bias))


class Saved:
    """What one stack forward leaves for its backward.  geo: the stack's Geometry; route: "chain", "conv" or "bn".
    xs[r] / a0s[r]: block r's input and its GELU operand copy, hs[r] / a1s[r]: conv1's pre-activation and its GELU --
    on the chain route xs[1:] and hs hold GELU'(x_r) and GELU'(h_r) instead (the chain's backward multiplies by
    them).  bs: the BatchNorm blocks' saved tensors; ws: the forward weight operands (none on the chain route);
    masks / pk_bwd: the chain's dropout keep bits and the sources of its backward's packed weights."""

    def __init__(self, geo, route, T, p_drop, seeds, ctr, training, x0, a0):
        self.geo = geo
        self.route, self.T, self.p_drop, self.seeds, self.ctr, self.training = route, T, p_drop, seeds, ctr, training
        self.xs, self.a0s, self.hs, self.a1s, self.bs, self.ws = [x0], [a0], [], [], [], []
        self.masks = self.pk_bwd = None


def _bn_stats(h, G, bn, training):
    """BatchNorm statistics [4][G][H] of h [N][H] (rows grouped by row % G); training moves the running stats."""
    N, H = h.shape
    sums = None
    if training and N // G <= 1:
        # torch BatchNorm1d refuses it too (a ragged last batch of one window under --batchnorm 1)
        raise ValueError(f"Expected more than 1 value per channel when training, got input size "
                         f"torch.Size([{N // G}, {H}])")
    if training:
        sums = torch.zeros(2, G, H, device=h.device, dtype=torch.float64)
        K.bn_group_stats(h, G, sums)
    st = torch.empty(4, G, H, device=h.device)
    K.bn_group_finalize(sums, N // G, H, G, bn, training, st)
    return st


def _bn_block_fwd(geo, a0, x, w1, w2, b1, b2, bns, training, p_drop, seed, ctr, T, last):
    """One `--batchnorm 1` ResBlock: x + Drop(BN2(Conv2(GELU(BN1(Conv1(GELU x)))))) (vq_vae_patch_embedd.py:60-74).
    a0 = GELU(x) in the operand dtype.  Returns (y f32, operand copy of GELU(y) -- of y itself when `last`: the
    output feeds the next conv directly --, saved)."""
    N, H = x.shape
    G = geo.G
    bn1, bn2 = bns
    e = lambda *s, dt=F32: torch.empty(*s, device=x.device, dtype=dt)  # noqa: E731
    h1 = e(N, H)
    K.gemm(a0, w1, N, H, geo.Kd, bias=b1, C=h1, **geo.fwd)
    st1 = _bn_stats(h1, G, bn1, training)
    hn1, a1 = e(N, H), e(N, H, dt=T)
    K.bn_apply(h1, G, st1, 0, hn1, op=a1)
    h2 = e(N, H)
    K.gemm(a1, w2, N, H, geo.Kd, bias=b2, C=h2, **geo.fwd)
    st2 = _bn_stats(h2, G, bn2, training)
    y, an = e(N, H), e(N, H, dt=T)
    K.bn_apply(h2, G, st2, 2 if last else 1, y, op=an, resid=x, drop=(p_drop, seed), seed_ptr=ctr)
    return y, an, dict(h1=h1, hn1=hn1, a1=a1, h2=h2, st1=st1, st2=st2)


def _bn_block_bwd(sv, r, gy, w1d, w2d, grads, bns, slot, wgrads, need_copy):
    """Backward of block r of a BatchNorm stack from gy (f32 gradient of its output).  Appends the two
    weight-gradient problems to ``wgrads`` and returns (gx f32, operand-dtype copy of gx or None)."""
    N, H = gy.shape
    geo = sv.geo
    G, T, training = geo.G, sv.T, sv.training
    bs, drop = sv.bs[r], dict(drop=(sv.p_drop, sv.seeds[r]), seed_ptr=sv.ctr)
    bn1, bn2 = bns
    dev = gy.device
    e = lambda *s, dt=F32: torch.empty(*s, device=dev, dtype=dt)  # noqa: E731
    n = N // G
    sums2 = torch.zeros(2, G, H, device=dev, dtype=torch.float64)
    K.bn_bwd_reduce(bs["h2"], G, bs["st2"], gy, sums2, **drop)
    dh2 = e(N, H, dt=T)
    K.bn_bwd_apply(bs["h2"], G, bs["st2"], gy, sums2, n, training, dh2, slot(bn2.weight), slot(bn2.bias), **drop)
    t1 = e(N, H)   # gradient of BN1's output: (dh2 . W2) * GELU'(BN1(h1))
    K.gemm(dh2, w2d, N, H, geo.Kd, b_trans=True, pre=bs["hn1"], C=t1, **geo.dgrad)
    wgrads.append(geo.wgrad_problem(dh2, bs["a1"], *grads(r, 1)))
    sums1 = torch.zeros(2, G, H, device=dev, dtype=torch.float64)
    K.bn_bwd_reduce(bs["h1"], G, bs["st1"], t1, sums1)
    dh1 = e(N, H, dt=T)
    K.bn_bwd_apply(bs["h1"], G, bs["st1"], t1, sums1, n, training, dh1, slot(bn1.weight), slot(bn1.bias))
    gx = e(N, H)
    gxo = e(N, H, dt=T) if need_copy else None
    K.gemm(dh1, w1d, N, H, geo.Kd, b_trans=True, pre=sv.xs[r], resid=gy, C=gx, C2=gxo, c2_mode=2 if need_copy else 0,
           **geo.dgrad)
    wgrads.append(geo.wgrad_problem(dh1, sv.a0s[r], *grads(r, 0)))
    return gx, gxo


def _chain_fwd(sv, weights, biases, RT, save, tail=None, sep=None, head=None):
    """Forward of the whole stack through aw_res_chain_fwd, from sv.xs[0] / sv.a0s[0].  Fills sv with GELU'(h), a1,
    GELU'(x), a per block -- a1 and a as the per-conv route makes them, the saved derivatives in place of its h and x
    (None without `save`) --, the operand copies the backward packs its weights from and the dropout keep bits.
    tail / sep / head: see ``forward``; the tail's matrices are packed in the same launch as the stack's, the sep
    conv's and the head's operand copies are read as they are."""
    geo = sv.geo
    R, H, taps, T = len(biases), geo.H, geo.taps, sv.T
    x0, a0 = sv.xs[0], sv.a0s[0]
    N, dev = a0.shape[0], a0.device
    e = lambda dt: torch.empty(N, H, device=dev, dtype=dt)  # noqa: E731
    sv.hs = [e(T) if save else None for _ in range(R)]
    sv.a1s = [e(T) if save else None for _ in range(R)]
    sv.xs += [e(RT) if save and r < R - 1 else None for r in range(R)]
    sv.a0s += [e(T) for _ in range(R)]
    # fragment-packed weight copies, from the operand copies, packed right before the chain that streams them (the
    # backward's by _chain_bwd, right before the backward chain): the pack's writes are still in the caches when the
    # chain starts reading
    wsrc = [w for r in range(R) for w in weights[r]]
    pk = [torch.empty(H, geo.Kd, device=dev, dtype=T) for _ in wsrc]
    ktail = None
    if tail is not None:
        Wt, tb, Y, cst = tail
        k1 = Wt.shape[0] // H
        tsrc = [Wt[j * H:(j + 1) * H] for j in range(k1)]      # k1 contiguous [out][in] matrices
        tpk = [torch.empty(H, H, device=dev, dtype=T) for _ in tsrc]
        K.res_pack_weights(wsrc + tsrc, pk + tpk, None, taps=taps, job_taps=[taps] * len(wsrc) + [1] * k1)
        ktail = (tpk, tb, Y, cst)
    else:
        K.res_pack_weights(wsrc, pk, None, taps=taps)
    if save:
        sv.pk_bwd = wsrc               # the sources of the backward's packed copies
        if sv.p_drop > 0 and R > 1:
            sv.masks = K.res_dropout_masks_empty(N, R, dev)
    K.res_chain_fwd(a0, x0, pk[0::2], pk[1::2], [b1 for b1, _ in biases], [b2 for _, b2 in biases], sv.hs, sv.a1s,
                    sv.xs[1:], sv.a0s[1:], drop=(sv.p_drop, sv.seeds), seed_ptr=sv.ctr, masks=sv.masks, taps=taps,
                    seg=geo.S, tail=ktail, sep=sep, head=head)


def _chain_bwd(sv, gx, gxo, grads):
    """Backward of the whole stack through aw_res_chain_bwd; returns (the stack input's operand gradient gxo_out[0],
    the weight-gradient problems in the per-conv route's order)."""
    N, H = gx.shape
    geo = sv.geo
    R, taps, dev, T = len(sv.hs), geo.taps, gx.device, gxo.dtype
    gh = [torch.empty(N, H, device=dev, dtype=T) for _ in range(R)]
    go = [torch.empty(N, H, device=dev, dtype=T) for _ in range(R)]
    pk_bwd = [torch.empty(H, geo.Kd, device=dev, dtype=T) for _ in sv.pk_bwd]
    K.res_pack_weights(sv.pk_bwd, None, pk_bwd, taps=taps)
    # hs / xs[1:]: the forward chain's saved GELU'(h_r) / GELU'(x_r); xs[0] = x_0, the stack input
    K.res_chain_bwd(gx, gxo, pk_bwd[0::2], pk_bwd[1::2], sv.hs, sv.xs[0], [None] + list(sv.xs[1:R]), gh, go,
                    drop_p=sv.p_drop, masks=sv.masks, taps=taps, seg=geo.S)
    sv.pk_bwd = sv.masks = None
    wgrads = []
    for r in reversed(range(R)):
        gin = gxo if r == R - 1 else go[r + 1]
        wgrads.append(geo.wgrad_problem(gin, sv.a1s[r], *grads(r, 1)))
        wgrads.append(geo.wgrad_problem(gh[r], sv.a0s[r], *grads(r, 0)))
    return go[0], wgrads


def forward(geo, x0, a0, weights, biases, bns=None, *, T, RT, p_drop=0.0, seeds=None, ctr=None, training=False,
            chain=False, last_operand_only=True, in_place=False, save=True, tail=None, sep=None, head=None):
    """R = len(biases) ResBlocks from x0 [N][H] (dtype RT) and a0 = GELU(x0) (operand dtype T).

    weights[r]: block r's (conv1, conv2) forward operands [H][Kd]; biases[r]: its (b1, b2); bns: per block the
    (BatchNorm1d, BatchNorm1d) pair of a BatchNorm stack, else None.  p_drop / seeds[r] / ctr: the dropout of block r
    (ctr: the device counter aw_gemm_args.seed_ptr mixes in, or None).  chain: take the one-launch route (the caller
    asked K.res_chain_ok; never with BatchNorm).  last_operand_only: the last block writes only the operand copy of
    x_R itself (what the next conv consumes: no f32 x_R, no GELU); otherwise it is a block like any other.  in_place
    (nothing saved): x and a are updated in place and h / a1 reused across blocks.  save=False keeps no per-block
    tensor (and the chain stores none of its derivatives).  tail = (Wt [k1 H][H] operand copy, bias (H,) f32,
    Y (N, k1 H) bf16, colstats (2 H,) f64 or None): only on the chain route of a taps = 3 stack -- the chain launch
    also runs the un-patch ConvT on x_R (Y and the BatchNorm column statistics of K.gemm(x_R, Wt, bias_mod=H,
    stats_mod=H)).  sep = (Ws [64][H] operand copy, bias (64,) f32, z (N, 64) f32): only on the chain route of a
    taps = 1 stack -- the chain launch also runs the sep conv on x_R (z of K.gemm(x_R, Ws, N, 64, H, bias=bias)).
    head (chain route only; K.res_chain_fwd's): the launch also runs the conv that makes x_0, and x0 / a0 are outputs
    the launch fills (what K.gemm(..., C=x0, C2=a0, c2_mode=1) writes).

    Returns (x_R or None when only its operand copy was written, the operand copy -- GELU(x_R), or x_R itself under
    last_operand_only --, Saved)."""
    R, H, Kd = len(biases), geo.H, geo.Kd
    N, dev = a0.shape[0], a0.device
    seeds = [0] * R if seeds is None else seeds
    route = "bn" if bns is not None else "chain" if chain else "conv"
    sv = Saved(geo, route, T, p_drop, seeds, ctr, training, x0, a0)
    e = lambda dt: torch.empty(N, H, device=dev, dtype=dt)  # noqa: E731
    if tail is not None and (route != "chain" or geo.taps != 3):
        raise ValueError("resstack.forward: the ConvT tail runs only inside the decoder chain")
    if sep is not None and (route != "chain" or geo.taps != 1):
        raise ValueError("resstack.forward: the sep tail runs only inside the encoder chain")
    if head is not None and route != "chain":
        raise ValueError("resstack.forward: a head runs only inside a chain launch")
    if route == "chain":
        _chain_fwd(sv, weights, biases, RT, save, tail, sep, head)
        return sv.xs[R], sv.a0s[R], sv
    x, a, h, a1 = x0, a0, None, None
    for r in range(R):
        (w1, w2), (b1, b2) = weights[r], biases[r]
        last = last_operand_only and r == R - 1
        if route == "bn":
            xn, an, bs = _bn_block_fwd(geo, a, x, w1, w2, b1, b2, bns[r], training, p_drop, seeds[r], ctr, T, last)
        else:
            if h is None or not in_place:
                h, a1 = e(T), e(T)         # pre-activation kept in the operand dtype
            K.gemm(a, w1, N, H, Kd, bias=b1, C=h, C2=a1, c2_mode=1, **geo.fwd)
            xn = None if last else x if in_place else e(RT)
            an = a if in_place else e(T)
            out = dict(C=an) if last else dict(C=xn, C2=an, c2_mode=1)
            K.gemm(a1, w2, N, H, Kd, bias=b2, drop=(p_drop, seeds[r]), seed_ptr=ctr, resid=x, **out, **geo.fwd)
            bs = None
        if save:
            sv.xs.append(xn)
            sv.a0s.append(an)
            sv.hs.append(h)
            sv.a1s.append(a1)
            sv.bs.append(bs)
            sv.ws.append((w1, w2))
        x, a = xn, an
    return x, a, sv


def backward(sv, gy, go, dweights, grads, bns=None, slot=None, r0_copy=True):
    """Backward of a stack from gy (the gradient of x_R) and go (its operand copy under block R-1's dropout mask; not
    read by a BatchNorm stack, whose blocks mask gy themselves).

    dweights[r]: block r's (conv1, conv2) input-gradient operands; grads(r, i) -> (weight gradient, bias gradient) of
    block r's conv i, parameter-shaped f32 accumulators; bns / slot: the BatchNorm modules per block and the
    accumulator of a parameter (BatchNorm stacks).  r0_copy: block 0 also writes the operand copy of the stack's
    input gradient (c2_mode 2); every other block writes the copy under the previous block's mask (c2_mode 3).

    Returns (gx, its operand copy or None, the 2R weight-gradient problems: blocks reversed, conv2 before conv1)."""
    if sv.route == "chain":
        gxo, wgrads = _chain_bwd(sv, gy, go, grads)
        return gxo, gxo, wgrads        # RT == T on the chain route: one tensor is both
    N, H = gy.shape
    geo, RT, T, p = sv.geo, gy.dtype, sv.T, sv.p_drop
    e = lambda dt: torch.empty(N, H, device=gy.device, dtype=dt)  # noqa: E731
    wgrads = []
    for r in reversed(range(len(sv.hs))):
        W1d, W2d = dweights[r]
        if sv.route == "bn":
            gy, go = _bn_block_bwd(sv, r, gy, W1d, W2d, grads, bns[r], slot, wgrads, r0_copy and r == 0)
            continue
        gh = e(T)
        K.gemm(go, W2d, N, H, geo.Kd, b_trans=True, pre=sv.hs[r], C=gh, **geo.dgrad)
        wgrads.append(geo.wgrad_problem(go, sv.a1s[r], *grads(r, 1)))
        gyn = e(RT)
        gon = e(T) if r > 0 or r0_copy else None
        K.gemm(gh, W1d, N, H, geo.Kd, b_trans=True, pre=sv.xs[r], resid=gy, C=gyn, C2=gon,
               c2_mode=3 if r > 0 else 2 if r0_copy else 0, drop2=(p, sv.seeds[r - 1] if r > 0 else 0),
               seed_ptr=sv.ctr, **geo.dgrad)
        wgrads.append(geo.wgrad_problem(gh, sv.a0s[r], *grads(r, 0)))
        gy, go = gyn, gon
    return gy, go, wgrads
