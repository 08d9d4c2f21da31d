"""A restatement of TS2Vec training's arithmetic in torch CPU ops, parameterised by dtype: what the kernels of
csrc/ts2vec_loss.hip and ``TS2Vec.fit`` are held to (float64), and the yardstick of the reference arithmetic's own
rounding (float32 against float64).  Written from the definitions, not from the kernels:

  paired InfoNCE over groups: a group is 2 N rows, rows 0..N-1 from z1 and N..2N-1 from z2; S = Z Z^T;
      lse_i = log sum_{j != i} exp S_ij;   row_loss_i = lse_i - S_{i, (i + N) mod 2N};   the term is the mean row_loss
  temporal term of (B, T, C): groups = sequences, rows = steps;   instance term: groups = steps, rows = sequences
  hierarchy: at every level alpha * instance (+ (1 - alpha) * temporal from level temporal_unit on), then a max-pool
      over time (kernel 2, stride 2, an odd last step dropped; torch sends the gradient to the first step on a tie);
      at length 1 one more alpha * instance; the sum over the number of levels.  Zero-weight terms are skipped.
  the encoder's forward as in tests/ts2vec_refs.py, but differentiable and over a dict of parameter tensors.
"""
from __future__ import annotations

import numpy as np
import torch
import torch.nn.functional as F


def groups_of(z1, z2, layout):
    """(G, 2N, C): the rows of every group, z1's first."""
    if layout == "temporal":
        return torch.cat([z1, z2], dim=1)
    if layout == "instance":
        return torch.cat([z1, z2], dim=0).transpose(0, 1)
    raise ValueError(layout)


def nce_rows(z1, z2, layout):
    """(lse, row_loss), each (G, 2N)."""
    Z = groups_of(z1, z2, layout)
    n2 = Z.shape[1]
    S = Z @ Z.transpose(1, 2)
    eye = torch.eye(n2, dtype=torch.bool)
    lse = torch.logsumexp(S.masked_fill(eye, float("-inf")), dim=-1)
    i = torch.arange(n2)
    return lse, lse - S[:, i, (i + n2 // 2) % n2]


def nce_term(z1, z2, layout):
    return nce_rows(z1, z2, layout)[1].mean()


def pool2(z):
    return F.max_pool1d(z.transpose(1, 2), kernel_size=2).transpose(1, 2)


def hierarchical(z1, z2, alpha=0.5, temporal_unit=0):
    total, d = z1.new_zeros(()), 0
    while z1.shape[1] > 1:
        if alpha != 0:
            total = total + alpha * nce_term(z1, z2, "instance")
        if d >= temporal_unit and 1 - alpha != 0:
            total = total + (1 - alpha) * nce_term(z1, z2, "temporal")
        d += 1
        z1, z2 = pool2(z1), pool2(z2)
    if z1.shape[1] == 1:
        if alpha != 0:
            total = total + alpha * nce_term(z1, z2, "instance")
        d += 1
    return total / d


def loss_and_grads(fn, z1, z2, dtype, *args, **kw):
    """(loss, dz1, dz2) of fn(z1, z2, ...) evaluated in dtype."""
    a = torch.as_tensor(np.asarray(z1)).to(dtype).clone().requires_grad_(True)
    b = torch.as_tensor(np.asarray(z2)).to(dtype).clone().requires_grad_(True)
    loss = fn(a, b, *args, **kw)
    if loss.requires_grad:
        loss.backward()
    zero = torch.zeros_like(a)
    return loss.detach(), a.grad if a.grad is not None else zero, b.grad if b.grad is not None else zero


def rows_grads(z1, z2, layout, dtype, scale=1.0):
    """(lse, row_loss, dz1, dz2) with dz the gradient of scale * sum(row_loss)."""
    a = torch.as_tensor(np.asarray(z1)).to(dtype).clone().requires_grad_(True)
    b = torch.as_tensor(np.asarray(z2)).to(dtype).clone().requires_grad_(True)
    lse, rl = nce_rows(a, b, layout)
    (scale * rl.sum()).backward()
    return lse.detach(), rl.detach(), a.grad, b.grad


# ------------------------------------------------------------------------------------------------ encoder
def n_blocks(p):
    return 1 + max(int(k.split(".")[2]) for k in p if k.startswith("feature_extractor.net."))


def encoder_forward(p, x, keep=None):
    """p: {name: tensor} under the reference's key names, in the dtype to compute in (requires_grad as the caller
    wishes); x (B, T, C_in) with NaN for missing; keep: (B, T) bool or None.  No dropout.  (B, T, C_out)."""
    dtype = p["input_fc.weight"].dtype
    x = torch.as_tensor(np.asarray(x)).to(dtype)
    ok = ~torch.isnan(x).any(-1)
    if keep is not None:
        ok = ok & torch.as_tensor(np.asarray(keep)).bool()
    ok = ok.unsqueeze(-1)
    zero = torch.zeros((), dtype=dtype)
    h = torch.where(ok, x, zero) @ p["input_fc.weight"].t() + p["input_fc.bias"]
    h = torch.where(ok, h, zero).transpose(1, 2)
    for i in range(n_blocks(p)):
        pre, d = f"feature_extractor.net.{i}.", 2 ** i
        res = h
        if pre + "projector.weight" in p:
            res = F.conv1d(h, p[pre + "projector.weight"], p[pre + "projector.bias"])
        u = F.conv1d(F.gelu(h), p[pre + "conv1.conv.weight"], p[pre + "conv1.conv.bias"], padding=d, dilation=d)
        u = F.conv1d(F.gelu(u), p[pre + "conv2.conv.weight"], p[pre + "conv2.conv.bias"], padding=d, dilation=d)
        h = u + res
    return h.transpose(1, 2)


def error_ratio(got, r64, r32):
    """(err, e_ref): max |got - r64| and max |r32 - r64|."""
    got = torch.as_tensor(np.asarray(got)).double()
    return float((got - r64.double()).abs().max()), float((r32.double() - r64.double()).abs().max())
