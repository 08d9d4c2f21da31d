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
