"""A stack of GRU layers (torch ``nn.GRU(in_dim, H, L, batch_first=True)``, model/gru.py:25,47) as ONE autograd node.

Work split ("GRU recurrence"): per layer, everything that is not recurrent is an ``aw_gemm`` over all T*B
rows -- the input projection GI = X W_ih^T + b_ih, the input gradient dX = dGI W_ih, and the weight gradients
(accumulate mode, one grouped launch of the three gate blocks per weight) -- and the recurrence is one
``aw_gru_step_fwd`` / ``aw_gru_step_bwd`` launch per time step.  The bias gradients are column sums of the f32 gate
gradients (``aw_gru_bias_grad``), not the GEMM's fused a_rowsum: that would sum the bf16-rounded operand copy in bf16
mode, and only GEMM operands may be rounded.

Buffers are time-major ([T][B][...], row t*B + b) in the kernels' padded layout (Hp = H rounded up to 32, gate g at
columns [g*Hp, g*Hp + H), zeros beyond H; the input width is padded to a multiple of 32 the same way).  A layer's
states live in one [T+1][B][Hp] buffer whose slot 0 is the zero initial state, so ``buf[:T]`` is h_{t-1} for every t
(the reduction operand of dW_hh) and ``buf[1:]`` is the layer's output (the next layer's input projection operand).
In bf16 mode the f32 states have a bf16 twin written by the step kernel; in f32 mode the f32 buffer is the operand.

The operand copies of the weights are built per call (as arcweld/modules.py does for the other stand-alone nodes).
Parameter gradients accumulate into ``owner._grad_sink[p]`` when a Trainer installed one (the flat optimizer views).
"""
from __future__ import annotations

import torch

from . import kernels as K
from .precision import operand_dtype

F32 = torch.float32
BF16 = torch.bfloat16


def pad32(n):
    return (int(n) + 31) // 32 * 32


class _Layer:
    """Per-call operand copies of one layer's weights, zero-padded: wih [3*Hp][Ip], bih [3*Hp], the two W_hh images."""

    def __init__(self, w_ih, w_hh, b_ih, b_hh, H, T, need_bwd):
        dev = w_ih.device
        self.H, self.I = H, w_ih.shape[1]
        self.Hp, self.Ip = K.gru_padded(H), pad32(w_ih.shape[1])
        self.p = (w_ih, w_hh, b_ih, b_hh)
        self.wih = torch.zeros(3, self.Hp, self.Ip, device=dev, dtype=T)
        self.wih[:, :H, :self.I].copy_(w_ih.detach().view(3, H, self.I))
        self.wih = self.wih.view(3 * self.Hp, self.Ip)
        self.bih = torch.zeros(3, self.Hp, device=dev, dtype=F32)
        self.bih[:, :H].copy_(b_ih.detach().view(3, H))
        self.bih = self.bih.view(-1)
        self.bhh = b_hh.detach().contiguous()
        self.w_fwd = torch.empty(3, self.Hp, self.Hp, device=dev, dtype=T)
        self.w_bwd = torch.empty(self.Hp, 3 * self.Hp, device=dev, dtype=T) if need_bwd else None
        K.gru_pack_weights(w_hh.detach().contiguous(), H, self.w_fwd, self.w_bwd)


def forward(x, params, H, T=None, save=True):
    """x (B, T, I) f32; params = [(w_ih, w_hh, b_ih, b_hh)] per layer.  Returns (out (B, T, H) f32 of the top layer,
    saved state for ``backward`` or None)."""
    T_op = operand_dtype(T)
    B, S, I = x.shape
    dev = x.device
    Hp = K.gru_padded(H)
    bf = T_op == BF16
    layers = [_Layer(*p, H, T_op, save) for p in params]
    xop = torch.zeros(S, B, layers[0].Ip, device=dev, dtype=T_op)
    xop[:, :, :I].copy_(x.detach().transpose(0, 1))
    recs = []
    cur = xop.view(S * B, -1)
    for ly in layers:
        gi = torch.empty(S * B, 3 * Hp, device=dev, dtype=F32)
        K.gemm(cur, ly.wih, S * B, 3 * Hp, ly.Ip, bias=ly.bih, C=gi)
        hf = torch.empty(S + 1, B, Hp, device=dev, dtype=F32)
        hf[0].zero_()
        hb = None
        if bf:
            hb = torch.empty(S + 1, B, Hp, device=dev, dtype=BF16)
            hb[0].zero_()
        hop = hb if bf else hf
        saved = torch.empty(S, B, 4 * Hp, device=dev, dtype=F32)
        gi3 = gi.view(S, B, 3 * Hp)
        for t in range(S):
            K.gru_step_fwd(H, T_op, gi3[t], ly.bhh, hf[t + 1], saved[t], w_fwd=ly.w_fwd if t > 0 else None,
                           h_prev_op=hop[t] if t > 0 else None, h_prev=hf[t] if t > 0 else None,
                           h_op=hb[t + 1] if bf else None)
        recs.append((ly, cur, hf, hop, saved))
        cur = hop[1:].view(S * B, Hp)
    out = hf[1:, :, :H].transpose(0, 1).contiguous()
    return out, ((B, S, I, H, T_op, recs) if save else None)


def backward(sv, g, slot, need_x):
    """g (B, T, H): gradient of the top layer's outputs.  Parameter gradients accumulate into slot(p).  Returns dx
    (B, T, I) or None."""
    B, S, I, H, T_op, recs = sv
    dev = g.device
    Hp = K.gru_padded(H)
    bf = T_op == BF16
    dy = torch.zeros(S, B, Hp, device=dev, dtype=F32)
    dy[:, :, :H].copy_(g.transpose(0, 1))
    dx = None
    for li in range(len(recs) - 1, -1, -1):
        ly, xin, hf, hop, saved = recs[li]
        dgi = torch.empty(S, B, 3 * Hp, device=dev, dtype=F32)
        dgh = torch.empty(S, B, 3 * Hp, device=dev, dtype=F32)
        dgi_b = torch.empty(S, B, 3 * Hp, device=dev, dtype=BF16) if bf else None
        dgh_b = torch.empty(S, B, 3 * Hp, device=dev, dtype=BF16) if bf else None
        dgh_op = dgh_b if bf else dgh
        dh = torch.empty(2, B, Hp, device=dev, dtype=F32)
        for t in range(S - 1, -1, -1):
            nxt = t + 1 < S
            K.gru_step_bwd(H, T_op, saved[t], dh[t & 1], dgi[t], dgh[t], w_bwd=ly.w_bwd if nxt else None,
                           dgh_next_op=dgh_op[t + 1] if nxt else None, dh_next=dh[(t + 1) & 1] if nxt else None,
                           saved_next=saved[t + 1] if nxt else None, dy=dy[t], h_prev=hf[t] if t > 0 else None,
                           dgi_op=dgi_b[t] if bf else None, dgh_op=dgh_b[t] if bf else None)
        w_ih, w_hh, b_ih, b_hh = ly.p
        gi_op = (dgi_b if bf else dgi).view(S * B, 3 * Hp)
        gh_op = dgh_op.view(S * B, 3 * Hp)
        hprev = hop[:S].view(S * B, Hp)
        g_wih, g_whh, g_bih, g_bhh = slot(w_ih), slot(w_hh), slot(b_ih), slot(b_hh)
        kw = dict(a_trans=True, b_trans=True, accumulate=True)
        # the three gate blocks of each weight: rows [g*H, (g+1)*H) of the (3H, .) gradient, columns [g*Hp, ..) of dG
        K.gemm_grouped([(gi_op[:, q * Hp:(q + 1) * Hp], xin, H, ly.I, S * B, dict(kw, C=g_wih[q * H:(q + 1) * H]))
                        for q in range(3)])
        K.gemm_grouped([(gh_op[:, q * Hp:(q + 1) * Hp], hprev, H, H, S * B, dict(kw, C=g_whh[q * H:(q + 1) * H]))
                        for q in range(3)])
        # the bias gradients from the f32 gate gradients in both modes (a_rowsum would sum the rounded bf16 copies)
        K.gru_bias_grad(dgi.view(S * B, 3 * Hp), H, g_bih)
        K.gru_bias_grad(dgh.view(S * B, 3 * Hp), H, g_bhh)
        if li > 0 or need_x:
            dxl = torch.empty(S * B, ly.Ip, device=dev, dtype=F32)
            K.gemm(gi_op, ly.wih, S * B, ly.Ip, 3 * Hp, b_trans=True, C=dxl)
            if li > 0:
                dy = dxl.view(S, B, Hp)
            else:
                dx = dxl.view(S, B, ly.Ip)[:, :, :I].transpose(0, 1).contiguous()
    return dx


class GRUFunction(torch.autograd.Function):
    """(owner, x, H, *params) -> top-layer outputs (B, T, H); params in torch's order per layer
    (weight_ih, weight_hh, bias_ih, bias_hh).  ``owner`` is the module whose ``_grad_sink`` is honoured."""

    @staticmethod
    def forward(ctx, owner, x, H, *params):
        per_layer = [tuple(params[i:i + 4]) for i in range(0, len(params), 4)]
        out, sv = forward(x.contiguous().float(), per_layer, H, save=True)
        ctx.owner, ctx.sv, ctx.params = owner, sv, params
        return out

    @staticmethod
    def backward(ctx, g):
        sink = getattr(ctx.owner, "_grad_sink", None)
        grads = {}

        def slot(p):
            if sink is not None and p in sink:
                return sink[p]
            t = grads.get(p)
            if t is None:
                t = torch.zeros_like(p, dtype=F32)
                grads[p] = t
            return t

        dx = backward(ctx.sv, g.contiguous(), slot, ctx.needs_input_grad[1])
        ctx.sv = None
        return (None, dx, None) + tuple(grads.get(p) for p in ctx.params)


def gru_stack(owner, x, H, params):
    """The stack from a zero initial state: an autograd node when grad mode is on and anything requires grad, else
    the plain kernel forward."""
    flat = [p for layer in params for p in layer]
    if not x.is_cuda:
        raise K.nat.NativeError("the GRU runs on HIP kernels only (got a CPU input); there is no CPU fallback")
    if torch.is_grad_enabled() and (x.requires_grad or any(p.requires_grad for p in flat)):
        return GRUFunction.apply(owner, x, H, *flat)
    with torch.no_grad():
        return forward(x.contiguous().float(), params, H, save=False)[0]
