"""fp64 restatements of the small HIP kernels (csrc/bn.hip, csrc/transformer.hip) and of the causal-attention training
kernels (csrc/attention.hip and the VALU kernels of csrc/transformer.hip), shared by the direct kernel tests.

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


# ------------------------------------------------------------------------------------------ causal attention, training
LOG2E = 1.4426950408889634
ATTN_RESCALE_STEP = 8.0 / LOG2E      # growth of a row's running max (scaled score) that makes the MFMA forward rescale


def _bf16(x):
    return x.to(torch.bfloat16).to(torch.float64)


def _same(x):
    return x


def _attn_heads(x, B, T, nh, hs):
    """(B*T, nh*hs) -> (B, nh, T, hs) double."""
    return x.double().reshape(B, T, nh, hs).transpose(1, 2)


def _attn_rows(x, B, T, nh, hs):
    """(B, nh, T, hs) -> (B*T, nh*hs)."""
    return x.transpose(1, 2).reshape(B * T, nh * hs)


def _attn_scores(qkv, B, T, nh, d):
    """q, k, v (B, nh, T, hs) double and the masked scaled scores (B, nh, T, T)."""
    hs = d // nh
    q, k, v = (_attn_heads(t, B, T, nh, hs) for t in qkv.view(B * T, 3, d).unbind(1))
    s = (q @ k.transpose(-2, -1)) / math.sqrt(hs)
    causal = torch.ones(T, T, dtype=torch.bool, device=qkv.device).tril()
    return q, k, v, s.masked_fill(~causal, float("-inf"))


def _attn_train(qkv, dy, B, T, nh, d, keep, p, rnd_p, rnd_y, rnd_ds, rnd_out):
    """Forward and backward of causal attention written out in double precision; the four ``rnd_*`` callables are the
    identity (attn_train_ref) or a bf16 rounding (attn_bf16_model) at the places named there."""
    hs = d // nh
    scale = 1.0 / math.sqrt(hs)
    q, k, v, s = _attn_scores(qkv, B, T, nh, d)
    g = _attn_heads(dy, B, T, nh, hs)
    lse = torch.logsumexp(s, dim=-1)
    P = (s - lse[..., None]).exp()                       # softmax; exactly 0 above the diagonal
    ms = None if keep is None else keep.to(device=qkv.device, dtype=torch.float64) / (1.0 - p)
    Pv = rnd_p(P if ms is None else P * ms)              # the (dropped) probabilities as P.V and P^T.dO take them
    y = rnd_y(Pv @ v)                                    # y as stored: delta is taken from the stored y
    delta = (g * y).sum(-1)
    dP = g @ v.transpose(-2, -1)
    if ms is not None:
        dP = dP * ms
    dS = rnd_ds(P * (dP - delta[..., None]))
    dq = rnd_out((dS @ k) * scale)
    dk = rnd_out((dS.transpose(-2, -1) @ q) * scale)
    dv = rnd_out(Pv.transpose(-2, -1) @ g)
    dqkv = torch.cat([_attn_rows(t, B, T, nh, hs) for t in (dq, dk, dv)], dim=1)
    return _attn_rows(y, B, T, nh, hs), lse.reshape(-1), dqkv, delta.reshape(-1)


def attn_train_ref(qkv, dy, B, T, nh, d, keep=None, p=0.0):
    """Causal self-attention (model/transformer_block.py:37-63) and its input gradients in double precision on the
    inputs as the kernels saw them: qkv (B*T, 3d), dy (B*T, d) -> y (B*T, d), lse (B*nh*T,), dqkv (B*T, 3d) and
    delta = rowsum(dy . y) (B*nh*T,).  ``keep`` (B, nh, T, T) bool with ``p``: attention-probability dropout, the
    mask applied after the softmax with the 1 / (1 - p) scaling (lse is that of the undropped row).  The backward
    formulas are written out (P, dP, dS), no autograd."""
    return _attn_train(qkv, dy, B, T, nh, d, keep, p, _same, _same, _same, _same)


def attn_bf16_model(qkv, dy, B, T, nh, d, keep=None, p=0.0, round_p=True, round_y=True, round_ds=True,
                    round_out=True):
    """attn_train_ref with a bf16 rounding at exactly the places the MFMA kernels (csrc/attention.hip) round: P
    before P.V and before P^T.dO, y before delta = dO.y (the stored y), dS before dS.K and dS^T.Q, and the four
    outputs.  Everything else stays fp64, so its distance from attn_train_ref is the error a correct bf16 kernel
    cannot avoid.  The VALU kernels (csrc/transformer.hip) keep P and dS in f32: round_p = round_ds = False is
    their model.  All four switches off gives attn_train_ref bit for bit."""
    rnd = [_bf16 if on else _same for on in (round_p, round_y, round_ds, round_out)]
    return _attn_train(qkv, dy, B, T, nh, d, keep, p, *rnd)


ATTN_REGIMES = ("flat", "big", "spike", "ramp")


def attn_regime(name, B, nh, T, hs, dtype, seed):
    """qkv (B*T, 3*nh*hs) and dy (B*T, nh*hs) of ``dtype`` on the CPU from a seeded generator (e0 = first head
    dimension, j = position):
      flat   randn (the control: scaled logits ~ N(0, 1))
      big    q and k x 3
      spike  q x 1.5 and every key at j = 40 (mod 64) x 6
      ramp   k = 0.5 randn + 0.25 j e0, q = 0.5 randn + 0.4 sqrt(hs) e0: the scaled score rises by 0.1 per key."""
    g = torch.Generator().manual_seed(seed)
    q, k, v, dy = (torch.randn(B, nh, T, hs, generator=g, dtype=torch.float64) for _ in range(4))
    e0 = torch.zeros(hs, dtype=torch.float64)
    e0[0] = 1.0
    if name == "big":
        q, k = q * 3, k * 3
    elif name == "spike":
        q = q * 1.5
        k = k.clone()
        k[..., 40::64, :] *= 6
    elif name == "ramp":
        k = k * 0.5 + 0.25 * torch.arange(T, dtype=torch.float64)[:, None] * e0
        q = q * 0.5 + 0.4 * math.sqrt(hs) * e0
    elif name != "flat":
        raise ValueError(name)
    qkv = torch.cat([_attn_rows(t, B, T, nh, hs) for t in (q, k, v)], dim=1)
    return qkv.to(dtype).contiguous(), _attn_rows(dy, B, T, nh, hs).to(dtype).contiguous()


def attn_rescale_events(qkv, B, T, nh, d, tile, step=ATTN_RESCALE_STEP):
    """(rescale, stale) summed over all rows: the key tiles after a row's first where its running max of the scaled
    score grows by more than ``step``, and those where it grows by an amount in (0, step].  At the default step and
    tile 64 ``rescale`` counts the firings of the MFMA forward's lazy rescale and ``stale`` the tiles it processes
    with a stale max; the VALU kernels (tile 32) rescale on every tile, by exp(-growth)."""
    _, _, _, s = _attn_scores(qkv, B, T, nh, d)
    tmax = torch.stack([s[..., t0:t0 + tile].max(-1).values for t0 in range(0, T, tile)], dim=-1)
    run = torch.cummax(tmax, dim=-1).values              # tile 0 holds key 0: finite for every row
    grow = run[..., 1:] - run[..., :-1]
    return int((grow > step).sum()), int(((grow > 0) & (grow <= step)).sum())


def attn_keep(seed, B, nh, T, p):
    """The attention kernels' dropout keep-mask (B, nh, T, T) bool: element ((b*nh + h)*T + i)*T + j."""
    keep = dropout_keep(seed, np.arange(B * nh * T * T, dtype=np.uint64), p)
    return torch.from_numpy(keep.reshape(B, nh, T, T))


def rel_fro(got, ref):
    """|got - ref|_F / |ref|_F in double (0 when both vanish)."""
    got, ref = got.detach().double().cpu(), ref.detach().double().cpu()
    n = float(ref.norm())
    e = float((got - ref).norm())
    return e / n if n > 0 else e


# The cases of tests/test_attn_train_gpu.py; tests/test_kernel_refs_cpu.py checks on the CPU that each reaches the
# rescale path (or, for ``flat``, does not) and is well enough conditioned.  (regime, B, nh, T, hs, dtype)
ATTN_MFMA_CASES = [(r, 2, nh, T, 64, torch.bfloat16) for nh in (2, 3) for T in (129, 200, 257) for r in ATTN_REGIMES]
# ramp at hs 16 runs at T = 130 only: at T = 70 it has too few tiles with a large step of the running max
ATTN_VALU_CASES = [(r, 2, 2, T, hs, dt)
                   for hs, dt in ((16, torch.float32), (64, torch.float32), (12, torch.float32), (32, torch.bfloat16))
                   for T in (70, 130) for r in ATTN_REGIMES if not (r == "ramp" and hs == 16 and T == 70)]
ATTN_DROP_CASES = [("big", 2, 2, 130, 64, torch.bfloat16), ("big", 2, 2, 70, 32, torch.bfloat16),
                   ("big", 2, 2, 130, 12, torch.float32)]
ATTN_DROP_P, ATTN_DROP_SEED = 0.2, 12345


def attn_case_seed(B, nh, T, hs):
    """Seed of a case's inputs.  The offsets at hs 12 and hs 32 move on from draws whose T = 70 case missed an event
    count that tests/test_kernel_refs_cpu.py requires (flat: 47 and 41 stale tiles; big at hs 32: 13 rescales)."""
    return 1000 + T + hs + 17 * (nh - 2) + {12: 2, 32: 1}.get(hs, 0)


def attn_case_id(c):
    return f"{c[0]}-nh{c[2]}-T{c[3]}-hs{c[4]}-{'bf16' if c[5] == torch.bfloat16 else 'f32'}"


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
