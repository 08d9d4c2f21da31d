"""The launches of the layers around the ResBlock stacks (arcweld.resstack), in one place: the pointwise convs (patch
embed, sep conv, decoder 1x1 conv: one GEMM each way) and the un-patch layer (model/vq_vae_patch_embedd.py:19-57:
ConvT(H, H, k1) -> BatchNorm1d -> GELU -> ConvT(H, 1, 5, 5)).

As in resstack everything works on plain token-major tensors, where the operands come from is the caller's business
(arcweld.vqvae: the persistent copies; arcweld.modules: built per call) and the weight-gradient accumulators are
``slot(param)`` results.  No helper sets a store policy: the caller's holds.
"""
import torch

from . import kernels as K


def mix(seed: int, salt: int) -> int:
    """Host seed of one dropout site (salt) of a call (seed)."""
    z = (seed * 0x9E3779B97F4A7C15 + salt * 0xBF58476D1CE4E5B9 + 0x94D049BB133111EB) & 0xFFFFFFFFFFFFFFFF
    z ^= z >> 31
    z = (z * 0xD6E8FEB86659FD93) & 0xFFFFFFFFFFFFFFFF
    return z ^ (z >> 32)


def cast(t, T):
    """t as a contiguous tensor of dtype T: t itself when it already is one, else a copy (aw_cast across dtypes)."""
    if t.dtype == T:
        return t.contiguous()
    out = torch.empty(t.shape, device=t.device, dtype=T)
    K.cast(t.contiguous(), out)
    return out


def operand(x, T):
    """x in the operand dtype T, no copy if it already is (what a stack of no blocks hands to the next conv)."""
    return x if x.dtype == T else cast(x, T)


def conv_fwd(x, W, bias, C, **epilogue):
    """C [N][O] = x [N][I] . W [O][I]^T + bias, with the caller's epilogue (C2 / c2_mode, flops)."""
    K.gemm(x, W, x.shape[0], W.shape[0], W.shape[1], bias=bias, C=C, **epilogue)


def conv_wgrad(g, x, gw, gb):
    """gw [O][I] += g [N][O]^T . x [N][I..]; gb (O,) += the column sums of g."""
    K.gemm(g, x, gw.shape[0], gw.shape[1], g.shape[0], a_trans=True, b_trans=True, C=gw, accumulate=True, a_rowsum=gb)


def conv_dgrad(g, W, C, **epilogue):
    """C [N][I] = g [N][O] . W [O][I], with the caller's epilogue (C2 / c2_mode / drop2 / seed_ptr)."""
    K.gemm(g, W, g.shape[0], W.shape[1], W.shape[0], b_trans=True, C=C, **epilogue)


def unpatch_fwd(xt, Wt, t1, bn, t2, Y, Q, x_hat, *, training, colstats=None, stats_mod=0, convt=True, head=True):
    """xt [N][H] -> Y (N, k1 H) by ConvT1 (Wt [k1 H][H]: its operand copy) -> BatchNorm stats [4 H] (returned) ->
    x_hat by the fused head (Q = S k1 positions per window).  colstats (2 H f64, zeroed) / stats_mod: the ConvT
    GEMM's batch-statistics epilogue; colstats None: the running statistics, which only `training` moves.
    convt=False: a chain tail already wrote Y (and colstats); head=False: the caller runs the head itself."""
    N, H = xt.shape
    k1 = Wt.shape[0] // H
    if convt:
        K.gemm(xt, Wt, N, k1 * H, H, bias=t1.bias, bias_mod=H, C=Y, colstats=colstats, stats_mod=stats_mod)
    stats = torch.empty(4 * H, device=Y.device)
    K.bn_finalize(colstats, N * k1, H, bn.weight, bn.bias, bn.running_mean, bn.running_var,
                  bn.num_batches_tracked if training else None, bn.eps,
                  bn.momentum if bn.momentum is not None else 0.1, training, stats)
    if head:
        K.unpatch_head_fwd(Y.view(N * k1, H), Q, stats, t2.weight.view(H, 5), t2.bias, x_hat)
    return stats


def unpatch_bwd(xt, Wt, t1, bn, t2, Y2, Q, stats, g, gsums, slot, T, *, training, pass1=True, gx=None, **epilogue):
    """Backward of ``unpatch_fwd`` from g (the gradient of x_hat): Y2 = Y as (N k1, H), gsums 2 H f64 (zeroed, or
    filled by a pass 1 the caller ran fused: pass1=False).  The input gradient goes to gx [N][H] (None: not wanted)
    with the caller's epilogue."""
    N, H = xt.shape
    k1 = Wt.shape[0] // H
    w2 = t2.weight.view(H, 5)
    if pass1:
        K.unpatch_head_bwd1(Y2, Q, stats, w2, g, gsums, slot(t2.weight).view(H, 5), slot(t2.bias), slot(bn.weight),
                            slot(bn.bias))
    gY = torch.empty(N * k1, H, device=g.device, dtype=T)
    K.unpatch_head_bwd2(Y2, Q, stats, w2, g, gsums, training, gY, slot(t1.bias))
    gY2 = gY.view(N, k1 * H)
    # ConvT1 weight gradient, computed as [i][(j,o)] and accumulated straight into the (H_in, H_out, k1) layout
    K.gemm(xt, gY2, H, k1 * H, N, a_trans=True, b_trans=True, C=slot(t1.weight).view(H, H * k1), accumulate=True,
           col_map=(H, k1, 0))
    if gx is not None:
        conv_dgrad(gY2, Wt, gx, **epilogue)
