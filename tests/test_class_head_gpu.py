"""aw_class_head_fwd / aw_class_head_bwd called directly: out = GELU_erf(xf . w1 + b1).view(B, T) @ W2^T + b2 and its
gradients against fp64 autograd -- the += accumulation into dw1 / db1 / dW2 / db2, the missing-bias and dw1 = None
variants, T > 64 (the lane loop) and more rows than the 1024 waves of the backward grid (the row loop)."""
import pytest
import torch

import kernel_refs as kr

pytestmark = pytest.mark.gpu

# (B, T, D); the last has 1605 rows > 1024 waves
SHAPES = [(1, 1, 4), (3, 63, 40), (2, 65, 64), (70, 7, 100), (5, 321, 512)]
VARIANTS = ["all", "no_bias", "no_dw1"]


def _K():
    from arcweld import kernels
    return kernels


@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("B,T,D", SHAPES)
def test_class_head_forward_backward(B, T, D, variant):
    K = _K()
    g = torch.Generator().manual_seed(B * 10007 + T * 101 + D)
    R = B * T
    rnd = lambda *s: torch.randn(*s, generator=g).cuda()  # noqa: E731
    xf, w1, W2, dout = rnd(R, D), rnd(D) / D ** 0.5, rnd(2, T) / T ** 0.5, rnd(B, 2)
    bias = variant != "no_bias"
    b1, b2 = (rnd(1), rnd(2)) if bias else (None, None)

    s = torch.full((R,), float("nan"), device="cuda")
    out = torch.full((B, 2), float("nan"), device="cuda")
    K.class_head_fwd(xf, B, T, w1, b1, W2, b2, s, out)

    priors = dict(dw1=rnd(D), db1=rnd(1), dW2=rnd(2, T), db2=rnd(2))
    acc = {k: v.clone() for k, v in priors.items()}
    if not bias:
        acc["db1"] = acc["db2"] = None
    if variant == "no_dw1":
        acc["dw1"] = None
    dxf = torch.full((R, D), float("nan"), device="cuda")
    K.class_head_bwd(xf, s, dout, B, T, w1, W2, dxf, acc["dw1"], acc["db1"], acc["dW2"], acc["db2"])
    torch.cuda.synchronize()

    leaf = lambda t: None if t is None else t.double().requires_grad_(True)  # noqa: E731
    xr, w1r, b1r, W2r, b2r = leaf(xf), leaf(w1), leaf(b1), leaf(W2), leaf(b2)
    ref_out, ref_s = kr.class_head_ref(xr, B, T, w1r, b1r, W2r, b2r)
    (ref_out * dout.double()).sum().backward()

    kr.close_out(s, ref_s.detach(), "s")
    kr.close_out(out, ref_out.detach(), "out")
    kr.close(dxf, xr.grad, "dxf")
    grads = dict(dw1=w1r.grad, db1=b1r.grad if bias else None, dW2=W2r.grad, db2=b2r.grad if bias else None)
    for name, got in acc.items():
        if got is None:
            continue
        # result = prior + gradient; compared as (result - prior) at the gradient's own bar
        kr.close(got.double() - priors[name].double(), grads[name], name + " - prior")
        assert not torch.equal(got, priors[name])
