"""The fp64 references of tests/kernel_refs.py against torch's own modules (no GPU): the direct kernel tests compare
the HIP kernels with these helpers, so the helpers are pinned first."""
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import kernel_refs as kr
from oracle import residual_vq as orv


def _bn(H, seed):
    g = torch.Generator().manual_seed(seed)
    bn = torch.nn.BatchNorm1d(H).double()
    with torch.no_grad():
        bn.weight.copy_(torch.randn(H, generator=g).double() * 0.5 + 1.0)
        bn.bias.copy_(torch.randn(H, generator=g).double() * 0.3)
        bn.running_mean.copy_(torch.randn(H, generator=g).double() * 0.2)
        bn.running_var.copy_(torch.rand(H, generator=g).double() + 0.5)
        bn.num_batches_tracked.fill_(5)
    return bn


@pytest.mark.parametrize("N,H,G", [(6, 8, 3), (130, 40, 1), (84, 16, 12)])
@pytest.mark.parametrize("training", [True, False])
def test_grouped_bn_is_batchnorm1d_per_slice(N, H, G, training):
    g = torch.Generator().manual_seed(N + H)
    h = (torch.randn(N, H, generator=g).double() * 1.5 + 0.5)
    gin = torch.randn(N, H, generator=g).double()
    bn = _bn(H, 3).train(training)
    rm0, rv0 = bn.running_mean.clone(), bn.running_var.clone()

    h_t = h.clone().requires_grad_(True)
    outs = [bn(h_t[k::G]) for k in range(G)]            # S separate calls, in token order
    ref = torch.empty(N, H, dtype=torch.float64)
    for k in range(G):
        ref[k::G] = outs[k].detach()
    sum((o * gin[k::G]).sum() for k, o in enumerate(outs)).backward()

    h_r = h.clone().requires_grad_(True)
    gamma = bn.weight.detach().clone().requires_grad_(True)
    beta = bn.bias.detach().clone().requires_grad_(True)
    y, mean, invstd = kr.bn_group_forward(h_r, G, gamma, beta, bn.eps, training, rm0, rv0)
    (y * gin).sum().backward()

    torch.testing.assert_close(y.detach(), ref, rtol=1e-12, atol=1e-12)
    torch.testing.assert_close(h_r.grad, h_t.grad, rtol=1e-11, atol=1e-12)
    torch.testing.assert_close(gamma.grad, bn.weight.grad, rtol=1e-11, atol=1e-12)
    torch.testing.assert_close(beta.grad, bn.bias.grad, rtol=1e-11, atol=1e-12)
    if training:
        m, v = kr.bn_group_batch_stats(h, G)
        rm, rv = kr.bn_running_update(rm0, rv0, m, v, N // G, bn.momentum)
        torch.testing.assert_close(rm, bn.running_mean, rtol=1e-12, atol=1e-12)
        torch.testing.assert_close(rv, bn.running_var, rtol=1e-12, atol=1e-12)
        assert int(bn.num_batches_tracked) == 5 + G
    else:
        assert torch.equal(bn.running_mean, rm0) and torch.equal(bn.running_var, rv0)
        assert int(bn.num_batches_tracked) == 5
        torch.testing.assert_close(mean, rm0.expand(G, H))
        torch.testing.assert_close(invstd, (rv0 + bn.eps).rsqrt().expand(G, H))


def test_bn_apply_modes_follow_the_module_order():
    """mode 0: BN then GELU; modes 1, 2: residual + dropout(BN), with GELU (1) or without (2) for the operand."""
    g = torch.Generator().manual_seed(0)
    y = torch.randn(5, 8, generator=g).double()
    resid = torch.randn(5, 8, generator=g).double()
    scale = kr.dropout_scale(9, (5, 8), 0.25)
    out, op = kr.bn_apply_ref(y, 0)
    assert torch.equal(out, y) and torch.equal(op, F.gelu(y))
    out, op = kr.bn_apply_ref(y, 1, resid, scale)
    assert torch.equal(out, resid + y * scale) and torch.equal(op, F.gelu(out))
    out, op = kr.bn_apply_ref(y, 2, resid, None)
    assert torch.equal(out, resid + y) and op is out
    assert set(scale.unique().tolist()) == {0.0, 1.0 / 0.75}


@pytest.mark.parametrize("ignore", [-1, -100, 3])
@pytest.mark.parametrize("frac", [0.0, 0.3, 1.0])
def test_ce_is_torch_cross_entropy(ignore, frac):
    g = torch.Generator().manual_seed(7)
    R, V = 50, 9
    logits = (3 * torch.randn(R, V, generator=g)).double()
    logits[::7, 1] = float("-inf")
    y = torch.randint(0, V, (R,), generator=g)
    y[y == 1] = 2                                                   # no target on a -inf logit
    if ignore >= 0:
        y[y == ignore] = ignore + 1
    y[torch.rand(R, generator=g) < frac] = ignore
    lt = logits.clone().requires_grad_(True)
    loss = F.cross_entropy(lt, y, ignore_index=ignore)
    lse, loss_sum, count, d = kr.ce_ref(logits, y, ignore)
    assert count.item() == (y != ignore).sum().item()
    torch.testing.assert_close(lse, torch.logsumexp(logits, 1))
    if count > 0:
        loss.backward()
        torch.testing.assert_close(loss_sum / count, loss.detach(), rtol=1e-12, atol=1e-12)
        torch.testing.assert_close(d, lt.grad, rtol=1e-12, atol=1e-14)
    else:
        assert math.isnan(loss.item()) and math.isnan((loss_sum / count).item())
        assert torch.count_nonzero(d) == 0


@pytest.mark.parametrize("ctr", [None, 7])
def test_vectorised_mask_is_the_scalar_oracle_hash(ctr):
    seed, p = 0x1234_5678_9ABC_DEF1, 0.25
    rng = np.random.default_rng(0)
    idx = np.concatenate([np.arange(500), rng.integers(0, 1 << 40, 500)]).astype(np.uint64)
    keep = kr.dropout_keep(seed, idx, p, ctr)
    s = orv._seed_mix(seed, ctr) if ctr is not None else seed
    thr = round(p * 65536)
    want = np.array([((orv._hash_group(s, int(e) >> 2) >> (16 * (int(e) & 3))) & 0xFFFF) >= thr for e in idx])
    assert np.array_equal(keep, want)
    assert np.array_equal(keep, [kr.dropout_keep_scalar(seed, e, p, ctr) for e in idx])
    assert 0.65 < keep.mean() < 0.85
    assert kr.dropout_keep(seed, idx, 0.0, ctr).all()
    if ctr is not None:
        assert not np.array_equal(keep, kr.dropout_keep(seed, idx, p, None))


def test_class_head_is_linear_gelu_linear():
    g = torch.Generator().manual_seed(1)
    B, T, D = 3, 5, 6
    l1, l2 = torch.nn.Linear(D, 1).double(), torch.nn.Linear(T, 2).double()
    xf = torch.randn(B * T, D, generator=g).double()
    ref = l2(F.gelu(l1(xf)).view(B, T))
    out, s = kr.class_head_ref(xf, B, T, l1.weight[0], l1.bias, l2.weight, l2.bias)
    torch.testing.assert_close(out, ref, rtol=1e-12, atol=1e-12)
    torch.testing.assert_close(s, l1(xf)[:, 0], rtol=1e-12, atol=1e-12)
    out, _ = kr.class_head_ref(xf, B, T, l1.weight[0], None, l2.weight, None)
    torch.testing.assert_close(out, F.gelu(xf @ l1.weight[0]).view(B, T) @ l2.weight.t(), rtol=1e-12, atol=1e-12)


@pytest.mark.parametrize("pos0,n_new", [(0, 6), (4, 1), (3, 3)])
def test_cached_attention_is_causal_sdpa(pos0, n_new):
    g = torch.Generator().manual_seed(2)
    B, nh, hs, T = 2, 3, 4, pos0 + n_new
    q, k, v = (torch.randn(B, T, nh, hs, generator=g).double() for _ in range(3))
    full = F.scaled_dot_product_attention(q.transpose(1, 2), k.transpose(1, 2), v.transpose(1, 2), is_causal=True)
    full = full.transpose(1, 2).reshape(B, T, nh * hs)
    got = kr.attn_cached_ref(q[:, pos0:], k, v, pos0)
    torch.testing.assert_close(got, full[:, pos0:], rtol=1e-12, atol=1e-12)


# ------------------------------------------------------------------------------------------ causal attention, training
def _attn_autograd(qkv, dy, B, T, nh, d, keep=None, p=0.0):
    """fp64 autograd through masked_fill + softmax (the module's own formulation)."""
    hs = d // nh
    x = qkv.double().clone().requires_grad_(True)
    q, k, v = (t.reshape(B, T, nh, hs).transpose(1, 2) for t in x.view(B, T, 3 * d).split(d, dim=2))
    att = (q @ k.transpose(-2, -1)) / math.sqrt(hs)
    att = att.masked_fill(~torch.ones(T, T, dtype=torch.bool).tril(), float("-inf"))
    lse = torch.logsumexp(att.detach(), dim=-1).reshape(-1)
    att = att.softmax(-1)
    if keep is not None:
        att = att * keep.double() / (1 - p)
    y = (att @ v).transpose(1, 2).reshape(B * T, d)
    y.backward(dy.double())
    return y.detach(), lse, x.grad


@pytest.mark.parametrize("regime", kr.ATTN_REGIMES)
@pytest.mark.parametrize("B,nh,T,hs,drop", [(2, 3, 70, 12, False), (1, 2, 130, 64, False), (2, 2, 45, 16, True),
                                            (3, 1, 1, 8, False)])
def test_attn_train_ref_is_autograd_softmax(regime, B, nh, T, hs, drop):
    d = nh * hs
    qkv, dy = kr.attn_regime(regime, B, nh, T, hs, torch.float32, 5 + T)
    keep, p = (kr.attn_keep(77, B, nh, T, 0.2), 0.2) if drop else (None, 0.0)
    y, lse, dqkv, delta = kr.attn_train_ref(qkv, dy, B, T, nh, d, keep, p)
    ay, alse, ag = _attn_autograd(qkv, dy, B, T, nh, d, keep, p)
    torch.testing.assert_close(y, ay, rtol=1e-12, atol=1e-12)
    torch.testing.assert_close(lse, alse, rtol=1e-12, atol=1e-12)
    torch.testing.assert_close(dqkv, ag, rtol=1e-12, atol=1e-12 * max(1.0, float(ag.abs().max())))
    want = (dy.double() * y).view(B, T, nh, hs).sum(-1).transpose(1, 2).reshape(-1)
    torch.testing.assert_close(delta, want, rtol=1e-12, atol=1e-12)
    if drop:
        assert not torch.equal(y, kr.attn_train_ref(qkv, dy, B, T, nh, d)[0])


@pytest.mark.parametrize("drop", [False, True])
def test_attn_bf16_model_without_roundings_is_the_reference(drop):
    B, nh, T, hs = 2, 2, 70, 16
    qkv, dy = kr.attn_regime("spike", B, nh, T, hs, torch.bfloat16, 3)
    keep, p = (kr.attn_keep(5, B, nh, T, 0.2), 0.2) if drop else (None, 0.0)
    ref = kr.attn_train_ref(qkv, dy, B, T, nh, nh * hs, keep, p)
    off = kr.attn_bf16_model(qkv, dy, B, T, nh, nh * hs, keep, p, round_p=False, round_y=False, round_ds=False,
                             round_out=False)
    assert all(torch.equal(a, b) for a, b in zip(off, ref))
    on = kr.attn_bf16_model(qkv, dy, B, T, nh, nh * hs, keep, p)
    assert torch.equal(on[1], ref[1])                                   # lse takes no rounding
    for a, b in zip((on[0], on[2]), (ref[0], ref[2])):
        assert torch.equal(a, a.to(torch.bfloat16).double()) and not torch.equal(a, b)
    # the VALU model rounds less, so it lies nearer the reference
    valu = kr.attn_bf16_model(qkv, dy, B, T, nh, nh * hs, keep, p, round_p=False, round_ds=False)
    assert kr.rel_fro(valu[2], ref[2]) < kr.rel_fro(on[2], ref[2])


def test_attn_regimes_are_seeded_and_shaped():
    B, nh, T, hs = 2, 3, 130, 16
    d = nh * hs
    flat, dy = kr.attn_regime("flat", B, nh, T, hs, torch.float64, 9)
    again, dy2 = kr.attn_regime("flat", B, nh, T, hs, torch.float64, 9)
    assert torch.equal(flat, again) and torch.equal(dy, dy2)
    assert flat.shape == (B * T, 3 * d) and dy.shape == (B * T, d) and flat.dtype == torch.float64
    big, _ = kr.attn_regime("big", B, nh, T, hs, torch.float64, 9)
    assert torch.equal(big[:, :2 * d], flat[:, :2 * d] * 3) and torch.equal(big[:, 2 * d:], flat[:, 2 * d:])
    spike, _ = kr.attn_regime("spike", B, nh, T, hs, torch.float64, 9)
    k, fk = spike.view(B, T, 3 * d)[:, :, d:2 * d], flat.view(B, T, 3 * d)[:, :, d:2 * d]
    assert torch.equal(k[:, 40::64], fk[:, 40::64] * 6) and torch.equal(k[:, :40], fk[:, :40])
    ramp, _ = kr.attn_regime("ramp", B, nh, T, hs, torch.float64, 9)
    _, _, _, s = kr._attn_scores(ramp, B, T, nh, d)
    slope = (s[..., -1, 1:] - s[..., -1, :-1]).mean().item()             # last row sees every key
    assert abs(slope - 0.1) < 0.01, slope
    assert kr.attn_regime("flat", B, nh, T, hs, torch.bfloat16, 9)[0].dtype == torch.bfloat16
    with pytest.raises(ValueError):
        kr.attn_regime("nope", B, nh, T, hs, torch.float64, 9)


def test_attn_rescale_events_counts_tile_steps():
    """One head, hs 1, q = 1: the scaled score of key j is k_j.  Keys step by 6 at j = 4 and by 1 at j = 8 (tile 4):
    rows >= 4 rescale once, rows >= 8 also take one stale tile."""
    T = 12
    k = torch.zeros(T, dtype=torch.float64)
    k[4:] = 6.0
    k[8:] = 7.0
    qkv = torch.stack([torch.ones(T, dtype=torch.float64), k, torch.zeros(T, dtype=torch.float64)], dim=1)
    assert kr.attn_rescale_events(qkv, 1, T, 1, 1, 4) == (8, 4)
    assert kr.attn_rescale_events(qkv, 1, T, 1, 1, 4, step=0.5) == (12, 0)
    assert kr.attn_rescale_events(qkv, 1, T, 1, 1, 12) == (0, 0)
    assert abs(kr.ATTN_RESCALE_STEP - 5.545) < 1e-3


_ATTN_CASES = ([("mfma",) + c for c in kr.ATTN_MFMA_CASES] + [("valu",) + c for c in kr.ATTN_VALU_CASES]
               + [("drop",) + c for c in kr.ATTN_DROP_CASES])


def test_attn_case_lists_are_the_issue_sets():
    assert len(kr.ATTN_MFMA_CASES) == 24 and len(kr.ATTN_VALU_CASES) == 31 and len(kr.ATTN_DROP_CASES) == 3
    assert {c[2:5] for c in kr.ATTN_MFMA_CASES} == {(nh, T, 64) for nh in (2, 3) for T in (129, 200, 257)}
    assert {(c[3], c[4], c[5]) for c in kr.ATTN_VALU_CASES} == {
        (T, hs, dt) for T in (70, 130)
        for hs, dt in ((16, torch.float32), (64, torch.float32), (12, torch.float32), (32, torch.bfloat16))}
    assert ("ramp", 2, 2, 130, 16, torch.float32) in kr.ATTN_VALU_CASES


@pytest.mark.parametrize("case", _ATTN_CASES, ids=lambda c: c[0] + "-" + kr.attn_case_id(c[1:]))
def test_attn_gpu_cases_reach_the_rescale_path_and_are_conditioned(case):
    """Every case of tests/test_attn_train_gpu.py: the peaked regimes make the running max jump past the lazy-rescale
    threshold (flat never does, but runs tiles on a stale max), and the bf16 rounding model stays within 5e-2
    (relative Frobenius) of the fp64 reference, so a 2 x model bar still means something.

    ``ramp`` rises by 0.1 per key by construction: 6.4 per 64-key MFMA tile, but 3.2 per 32-key VALU tile, below
    the 5.55 step.  The VALU kernels rescale on every tile whatever the step (corr = exp(m - mn)), so for them ramp
    is held to >= 14 tiles whose max grows by more than 2.5 (corr < 0.09) instead."""
    path, regime, B, nh, T, hs, dtype = case
    d = nh * hs
    qkv, dy = kr.attn_regime(regime, B, nh, T, hs, dtype, kr.attn_case_seed(B, nh, T, hs))
    assert qkv.dtype == dtype and not qkv.is_cuda
    tile = 64 if path == "mfma" else 32
    resc, stale = kr.attn_rescale_events(qkv, B, T, nh, d, tile)
    if regime == "flat":
        assert resc == 0 and stale >= 50, (resc, stale)
    elif path == "mfma":
        assert resc >= 8, resc
    elif regime == "ramp":
        assert kr.attn_rescale_events(qkv, B, T, nh, d, tile, step=2.5)[0] >= 14
    else:
        assert resc >= 14, resc
    keep, p = (kr.attn_keep(kr.ATTN_DROP_SEED, B, nh, T, kr.ATTN_DROP_P), kr.ATTN_DROP_P) if path == "drop" \
        else (None, 0.0)
    if keep is not None:
        assert 0.7 <= keep.float().mean().item() <= 0.9
        causal = torch.ones(T, T, dtype=torch.bool).tril()
        assert 0.7 <= keep[..., causal].float().mean().item() <= 0.9       # the elements the kernels look at
    ref = kr.attn_train_ref(qkv, dy, B, T, nh, d, keep, p)
    mod = kr.attn_bf16_model(qkv, dy, B, T, nh, d, keep, p)
    assert kr.rel_fro(mod[0], ref[0]) <= 5e-2
    for j in range(3):
        assert kr.rel_fro(mod[2][:, j * d:(j + 1) * d], ref[2][:, j * d:(j + 1) * d]) <= 5e-2, j
