"""fp64 restatements of the small HIP kernels (csrc/bn.hip, csrc/transformer.hip), shared by the direct kernel tests.

Everything here is plain torch/numpy in double precision, evaluated on the inputs the kernels saw (already rounded to
their storage type).  tests/test_kernel_refs_cpu.py checks these helpers against torch's own modules without a GPU, so
the GPU tests compare the kernels with something that was itself validated.
"""
from __future__ import annotations

import math

import numpy as np
import torch
import torch.nn.functional as F

from oracle import residual_vq as orv

M64 = orv.M64
BF16_REL = 2.0 ** -8          # one bf16 rounding of the reference value, as a relative bound


# ------------------------------------------------------------------------------------------ dropout mask
def effective_seed(seed, ctr=None):
    """aw_seed_mix: the salt itself, or aw_seed_mix_value(salt, *seed_ptr) when a device counter is passed."""
    return orv._seed_mix(int(seed) & M64, int(ctr)) if ctr is not None else int(seed) & M64


def drop_threshold(p):
    """aw_drop_threshold: (uint32)(p * 65536.f + 0.5f), in f32 like the kernel."""
    return int(np.float32(p) * np.float32(65536.0) + np.float32(0.5))


def dropout_keep(seed, idx, p, ctr=None):
    """Keep-mask (numpy bool) of aw_dropout_scale for the flat element indices ``idx``: element e is dropped iff the
    16-bit slice ``e & 3`` of aw_hash_group(seed, e >> 2) is below round(p * 65536).  The hash is the oracle's
    (oracle.residual_vq._hash_group), evaluated on uint64 arrays."""
    e = np.asarray(idx, dtype=np.uint64)
    if p <= 0:
        return np.ones(e.shape, dtype=bool)
    with np.errstate(over="ignore"):
        h = orv._hash_group(np.uint64(effective_seed(seed, ctr)), e >> np.uint64(2))
    u = (h >> (np.uint64(16) * (e & np.uint64(3)))) & np.uint64(0xFFFF)
    return u >= np.uint64(drop_threshold(p))


def dropout_keep_scalar(seed, e, p, ctr=None):
    """The same rule for one index, on Python integers (the form the oracle uses)."""
    if p <= 0:
        return True
    h = orv._hash_group(effective_seed(seed, ctr), int(e) >> 2)
    return ((h >> (16 * (int(e) & 3))) & 0xFFFF) >= drop_threshold(p)


def dropout_scale(seed, shape, p, ctr=None, device="cpu"):
    """fp64 tensor of the given shape: 0 where dropped, 1 / (1 - p) where kept (flat row-major element index)."""
    n = int(np.prod(shape))
    keep = dropout_keep(seed, np.arange(n, dtype=np.uint64), p, ctr).reshape(shape)
    return torch.from_numpy(keep).to(device=device, dtype=torch.float64) / (1.0 - p)


# ------------------------------------------------------------------------------------------ grouped BatchNorm
def gelu(x):
    return F.gelu(x)          # erf form


def bn_group_batch_stats(h, G):
    """h (N, H) double, group = row % G: per-group mean and biased variance, each (G, H)."""
    N, H = h.shape
    hg = h.view(N // G, G, H)
    return hg.mean(0), hg.var(0, unbiased=False)


def bn_group_forward(h, G, gamma, beta, eps, training, running_mean=None, running_var=None):
    """Normalised rows y (N, H) and the statistics used (mean, invstd; each (G, H)).  Training: batch statistics of
    each group; eval: the running statistics for every group.  Differentiable (fp64 autograd)."""
    N, H = h.shape
    if training:
        mean, var = bn_group_batch_stats(h, G)
    else:
        mean, var = running_mean.expand(G, H), running_var.expand(G, H)
    invstd = (var + eps).rsqrt()
    g = gamma if gamma is not None else 1.0
    b = beta if beta is not None else 0.0
    y = ((h.view(N // G, G, H) - mean) * invstd * g + b).reshape(N, H)
    return y, mean, invstd


def bn_running_update(running_mean, running_var, mean, var, n, momentum):
    """The G updates of torch.nn.BatchNorm1d's running statistics, in group order, with the unbiased variance."""
    rm, rv = running_mean.clone(), running_var.clone()
    for g in range(mean.shape[0]):
        rm = (1 - momentum) * rm + momentum * mean[g]
        rv = (1 - momentum) * rv + momentum * var[g] * (n / max(n - 1, 1))
    return rm, rv


def bn_apply_ref(y, mode, resid=None, scale=None):
    """aw_bn_apply on the normalised rows: mode 0 out = y; modes 1, 2 out = resid + y * scale (scale: the dropout
    keep-mask / (1 - p), or None).  op = out (mode 2) or GELU(out)."""
    out = y if mode == 0 else resid + (y * scale if scale is not None else y)
    return out, (out if mode == 2 else gelu(out))


# ------------------------------------------------------------------------------------------ cross entropy
def ce_ref(logits, y, ignore_index):
    """logits (R, V) double, y (R,) int64 -> lse (R,), loss_sum, count and d(loss_sum / count)/dlogits (zero rows
    where ignored).  count == 0 leaves dlogits all zero (and loss_sum / count NaN, as torch)."""
    lse = torch.logsumexp(logits, dim=1)
    valid = y != ignore_index
    t = torch.where(valid, y, torch.zeros_like(y))
    picked = logits.gather(1, t[:, None])[:, 0]
    loss_sum = torch.where(valid, lse - picked, torch.zeros_like(lse)).sum()
    count = valid.sum().to(torch.float64)
    p = (logits - lse[:, None]).exp()
    onehot = F.one_hot(t, logits.shape[1]).to(torch.float64)
    d = (p - onehot) * valid[:, None].to(torch.float64)
    d = d / count if count > 0 else torch.zeros_like(d)
    return lse, loss_sum, count, d


# ------------------------------------------------------------------------------------------ class head
def class_head_ref(xf, B, T, w1, b1, W2, b2):
    """out (B, 2) = GELU_erf(xf . w1 + b1).view(B, T) @ W2^T + b2; also returns s = xf . w1 + b1 (B*T,)."""
    s = xf @ w1
    if b1 is not None:
        s = s + b1
    out = gelu(s).view(B, T) @ W2.t()
    if b2 is not None:
        out = out + b2
    return out, s


# ------------------------------------------------------------------------------------------ KV-cache attention
def attn_cached_ref(q_new, k_all, v_all, pos0):
    """q_new (B, n_new, nh, hs), k_all / v_all (B, pos0 + n_new, nh, hs), all double: new row i attends to keys
    0 .. pos0 + i.  Returns (B, n_new, nh * hs)."""
    B, n_new, nh, hs = q_new.shape
    Tk = k_all.shape[1]
    att = torch.einsum("bihe,bjhe->bhij", q_new, k_all) / math.sqrt(hs)
    j = torch.arange(Tk, device=q_new.device)[None, :]
    i = torch.arange(n_new, device=q_new.device)[:, None]
    att = att.masked_fill(j > pos0 + i, float("-inf")).softmax(-1)
    return torch.einsum("bhij,bjhe->bihe", att, v_all).reshape(B, n_new, nh * hs)


# ------------------------------------------------------------------------------------------ comparison bars
def close(got, ref, name, rtol=1e-3, extra_rel=0.0):
    """Gradients and statistics: the bar of tests/test_submodules.py::_close (atol scaled by max|ref|);
    ``extra_rel`` adds a storage rounding of the reference value (bf16 outputs)."""
    got = got.detach().double().cpu().numpy() if torch.is_tensor(got) else np.asarray(got, dtype=np.float64)
    ref = ref.detach().double().cpu().numpy() if torch.is_tensor(ref) else np.asarray(ref, dtype=np.float64)
    scale = np.abs(ref).max() + 1e-12 if ref.size else 0.0
    np.testing.assert_allclose(got, ref, rtol=rtol + extra_rel, atol=2e-4 * scale + 1e-7, err_msg=name)


def close_out(got, ref, name, extra_rel=0.0):
    """Outputs: rtol = atol = 1e-4 (tests/test_submodules.py::_close_out)."""
    got = got.detach().double().cpu().numpy() if torch.is_tensor(got) else np.asarray(got, dtype=np.float64)
    ref = ref.detach().double().cpu().numpy() if torch.is_tensor(ref) else np.asarray(ref, dtype=np.float64)
    np.testing.assert_allclose(got, ref, rtol=1e-4 + extra_rel, atol=1e-4, err_msg=name)


def max_err(got, ref):
    return float((got.detach().double().cpu() - ref.detach().double().cpu()).abs().max()) if ref.numel() else 0.0
