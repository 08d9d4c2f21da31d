"""The one-line kernels behind arcweld.kernels that no test called directly, each against its torch fp64 equivalent."""
import pytest
import torch

import kernel_refs as kr

pytestmark = pytest.mark.gpu


def _K():
    from arcweld import kernels
    return kernels


def test_vq_gather():
    g = torch.Generator().manual_seed(0)
    E = torch.randn(70, 12, generator=g).cuda()
    idx = torch.randint(0, 70, (333,), generator=g).cuda()
    idx[:2] = torch.tensor([0, 69])
    out = torch.full((333, 12), float("nan"), device="cuda")
    _K().vq_gather(E, idx, out)
    torch.cuda.synchronize()
    assert torch.equal(out, E[idx])


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
@pytest.mark.parametrize("pad", [0, 7])
def test_patchify(dtype, pad):
    """Channel-major flattening of each (L, C) window cut into patches of P; padding columns of the output are zero."""
    g = torch.Generator().manual_seed(1)
    B, L, C, P = 3, 50, 2, 25
    S = L * C // P
    x = torch.randn(B, L, C, generator=g).cuda()
    buf = torch.full((B * S + 1, P + pad), float("nan"), device="cuda", dtype=dtype)
    out = buf[:B * S]
    _K().patchify(x, P, out)
    torch.cuda.synchronize()
    ref = x.double().transpose(1, 2).reshape(B * S, P)
    assert torch.equal(out[:, :P], ref.to(dtype))
    assert torch.count_nonzero(out[:, P:]) == 0 and not torch.isnan(out[:, P:]).any()
    assert torch.isnan(buf[B * S]).all()


@pytest.mark.parametrize("training", [True, False])
def test_bn_finalize(training):
    g = torch.Generator().manual_seed(2)
    n, H, eps, mom = 37, 300, 1e-5, 0.1
    h = (torch.randn(n, H, generator=g) * 2 + 1).double()
    colstats = torch.stack([h.sum(0), (h * h).sum(0)]).cuda()
    gamma, beta = torch.randn(H, generator=g).cuda(), torch.randn(H, generator=g).cuda()
    rm0, rv0 = torch.randn(H, generator=g).cuda(), (torch.rand(H, generator=g) + 0.5).cuda()
    rm, rv = rm0.clone(), rv0.clone()
    nbt = torch.tensor([4], device="cuda", dtype=torch.int64)
    stats = torch.full((4, H), float("nan"), device="cuda")
    _K().bn_finalize(colstats, n, H, gamma, beta, rm, rv, nbt, eps, mom, training, stats)
    torch.cuda.synchronize()
    assert torch.equal(stats[2], gamma) and torch.equal(stats[3], beta)
    if training:
        mean, var = h.mean(0), h.var(0, unbiased=False)
        kr.close(stats[0], mean, "mean")
        kr.close(stats[1], (var + eps).rsqrt(), "invstd")
        kr.close(rm, (1 - mom) * rm0.double().cpu() + mom * mean, "running_mean")
        kr.close(rv, (1 - mom) * rv0.double().cpu() + mom * var * n / (n - 1), "running_var")
        assert nbt.item() == 5
    else:
        assert torch.equal(stats[0], rm0)
        kr.close(stats[1], (rv0.double() + eps).rsqrt(), "invstd")
        assert torch.equal(rm, rm0) and torch.equal(rv, rv0) and nbt.item() == 4


def test_mse_finalize():
    sqerr = torch.tensor([1234.56789], device="cuda", dtype=torch.float64)
    out = torch.full((1,), float("nan"), device="cuda")
    _K().mse_finalize(sqerr, 1000, out)
    torch.cuda.synchronize()
    assert out.item() == (sqerr / 1000).float().item()


def test_scalar_add():
    a, b = torch.tensor([1.25], device="cuda"), torch.tensor([-3.7], device="cuda")
    out = torch.full((1,), float("nan"), device="cuda")
    _K().scalar_add(a, b, out)
    torch.cuda.synchronize()
    assert out.item() == (a.double() + b.double()).float().item()


def test_scale_():
    """x *= s[0] over more elements than one pass of the grid (4096 blocks of 256)."""
    g = torch.Generator().manual_seed(3)
    n = 4096 * 256 + 1000
    x0 = torch.randn(n, generator=g).cuda()
    s = torch.tensor([0.37], device="cuda")
    x = x0.clone()
    _K().scale_(x, s)
    torch.cuda.synchronize()
    assert torch.equal(x, (x0.double() * s.double()).float())      # one rounding of the exact product


def test_counter_add():
    c = torch.tensor([41], device="cuda", dtype=torch.int64)
    _K().counter_add(c)
    _K().counter_add(c, 1 << 40)
    torch.cuda.synchronize()
    assert c.item() == 42 + (1 << 40)
