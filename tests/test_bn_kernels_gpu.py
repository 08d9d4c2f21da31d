"""csrc/bn.hip called directly through arcweld.kernels, against the fp64 restatement of tests/kernel_refs.py.

The module-parity tests reach these kernels at dropout 0, in training mode, with fp32 operands and two small shapes;
here every kernel runs at the shapes where its loops change (H > 256, groups of more than BN_ROWS = 64 rows with a short
tail, N*H above the 8192*256 grid cap), with the regenerated dropout masks compared elementwise, bf16 outputs, the eval
backward, accumulating / absent parameter gradients, and badly conditioned inputs (|mean| >> std)."""
import functools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import kernel_refs as kr

pytestmark = pytest.mark.gpu

# (N, H, G), N % G == 0: n = 2 (the minimum); 3 row blocks with a 2-row tail; H > 256 and 65 = 64 + 1 rows per group;
# the encoder-like G = S; 2,101,248 elements (> 2,097,152 = the grid cap of the elementwise kernels)
SHAPES = [(6, 8, 3), (130, 40, 1), (325, 300, 5), (84, 64, 12), (4104, 512, 8)]
SEED = 0xC0FFEE12345678AB
DROPS = [(0.0, None), (0.25, None), (0.25, 7)]        # (p, value of the device counter behind seed_ptr)
NBT0 = 5


def _K():
    from arcweld import kernels
    return kernels


@functools.lru_cache(maxsize=None)
def _data(N, H, G):
    g = torch.Generator().manual_seed(1000 * N + H + G)
    h = torch.randn(N, H, generator=g) * (0.5 + torch.rand(H, generator=g)) + torch.randn(H, generator=g) * 0.7
    resid = torch.randn(N, H, generator=g)
    gin = torch.randn(N, H, generator=g)
    return tuple(t.cuda() for t in (h, resid, gin))


@functools.lru_cache(maxsize=None)
def _scale(N, H, p, ctr):
    return kr.dropout_scale(SEED, (N, H), p, ctr, device="cuda") if p > 0 else None


def _bn(H):
    g = torch.Generator().manual_seed(H)
    bn = torch.nn.BatchNorm1d(H)
    with torch.no_grad():
        bn.weight.copy_(torch.randn(H, generator=g) * 0.5 + 1.0)
        bn.bias.copy_(torch.randn(H, generator=g) * 0.3)
        bn.running_mean.copy_(torch.randn(H, generator=g) * 0.2)
        bn.running_var.copy_(torch.rand(H, generator=g) + 0.5)
        bn.num_batches_tracked.fill_(NBT0)
    return bn.cuda()


def _stats(h, G, bn, training):
    """stats [4][G][H] by the kernels, as arcweld.resstack._bn_stats does."""
    K = _K()
    N, H = h.shape
    sums = None
    if training:
        sums = torch.zeros(2, G, H, device="cuda", dtype=torch.float64)
        K.bn_group_stats(h, G, sums)
    st = torch.full((4, G, H), float("nan"), device="cuda")
    K.bn_group_finalize(sums, N // G, H, G, bn, training, st)
    return st


def _ctr(v):
    return None if v is None else torch.tensor([v], device="cuda", dtype=torch.int64)


@pytest.mark.parametrize("N,H,G", SHAPES)
def test_training_statistics_and_running_updates(N, H, G):
    h, _, _ = _data(N, H, G)
    bn = _bn(H)
    rm0, rv0 = bn.running_mean.double().clone(), bn.running_var.double().clone()
    st = _stats(h, G, bn, True)
    torch.cuda.synchronize()
    mean, var = kr.bn_group_batch_stats(h.double(), G)
    kr.close(st[0], mean, "mean")
    kr.close(st[1], (var + bn.eps).rsqrt(), "invstd")
    assert torch.equal(st[2], bn.weight.detach().expand(G, H)) and torch.equal(st[3], bn.bias.detach().expand(G, H))
    rm, rv = kr.bn_running_update(rm0, rv0, mean, var, N // G, bn.momentum)
    kr.close(bn.running_mean, rm, "running_mean after G ordered updates")
    kr.close(bn.running_var, rv, "running_var after G ordered updates")
    assert int(bn.num_batches_tracked) == NBT0 + G


@pytest.mark.parametrize("N,H,G", SHAPES)
def test_eval_statistics_come_from_the_running_buffers(N, H, G):
    h, _, _ = _data(N, H, G)
    bn = _bn(H).eval()
    rm0, rv0 = bn.running_mean.clone(), bn.running_var.clone()
    st = _stats(h, G, bn, False)
    torch.cuda.synchronize()
    assert torch.equal(bn.running_mean, rm0) and torch.equal(bn.running_var, rv0)
    assert int(bn.num_batches_tracked) == NBT0
    assert torch.equal(st[0], rm0.expand(G, H))
    kr.close(st[1], (rv0.double() + bn.eps).rsqrt().expand(G, H), "invstd")
    assert torch.equal(st[2], bn.weight.detach().expand(G, H)) and torch.equal(st[3], bn.bias.detach().expand(G, H))


def _apply_cases():
    for mode in (0, 1, 2):
        for p, ctr in (DROPS if mode else DROPS[:1]):
            for op_dtype in (torch.float32, torch.bfloat16):
                yield mode, p, ctr, op_dtype


@pytest.mark.parametrize("mode,p,ctr,op_dtype", list(_apply_cases()))
@pytest.mark.parametrize("N,H,G", SHAPES)
def test_bn_apply_elementwise(N, H, G, mode, p, ctr, op_dtype):
    K = _K()
    h, resid, _ = _data(N, H, G)
    bn = _bn(H)
    st = _stats(h, G, bn, True)
    out = torch.full((N, H), float("nan"), device="cuda")
    op = torch.full((N, H), float("nan"), device="cuda", dtype=op_dtype)
    K.bn_apply(h, G, st, mode, out, op=op, resid=resid if mode else None, drop=(p, SEED), seed_ptr=_ctr(ctr))
    torch.cuda.synchronize()
    y, _, _ = kr.bn_group_forward(h.double(), G, bn.weight.detach().double(), bn.bias.detach().double(), bn.eps, True)
    ref_out, ref_op = kr.bn_apply_ref(y, mode, resid.double(), _scale(N, H, p, ctr))
    if p > 0:   # the mask itself, exactly: a dropped element is the residual bit for bit, a kept one is not
        dropped = _scale(N, H, p, ctr) == 0
        assert torch.equal(out[dropped], resid[dropped])
        assert 0.2 < dropped.double().mean().item() < 0.3 or N * H < 1000
    kr.close_out(out, ref_out, "out")
    kr.close_out(op, ref_op, "op", extra_rel=kr.BF16_REL if op_dtype == torch.bfloat16 else 0.0)


def test_bn_apply_without_operand_output():
    K = _K()
    N, H, G = SHAPES[1]
    h, resid, _ = _data(N, H, G)
    bn = _bn(H)
    st = _stats(h, G, bn, True)
    out = torch.full((N, H), float("nan"), device="cuda")
    K.bn_apply(h, G, st, 1, out, op=None, resid=resid, drop=(0.25, SEED), seed_ptr=_ctr(7))
    torch.cuda.synchronize()
    y, _, _ = kr.bn_group_forward(h.double(), G, bn.weight.detach().double(), bn.bias.detach().double(), bn.eps, True)
    kr.close_out(out, kr.bn_apply_ref(y, 1, resid.double(), _scale(N, H, 0.25, 7))[0], "out")


def _bwd_cases():
    for training in (True, False):
        for dh_dtype in (torch.float32, torch.bfloat16):
            for p, ctr in DROPS:
                yield training, dh_dtype, p, ctr, True
            yield training, dh_dtype, 0.0, None, False          # dgamma = dbeta = None


@pytest.mark.parametrize("training,dh_dtype,p,ctr,pgrads", list(_bwd_cases()))
@pytest.mark.parametrize("N,H,G", SHAPES)
def test_bn_backward(N, H, G, training, dh_dtype, p, ctr, pgrads):
    K = _K()
    h, resid, gin = _data(N, H, G)
    bn = _bn(H).train(training)
    rm0, rv0 = bn.running_mean.double().clone(), bn.running_var.double().clone()
    st = _stats(h, G, bn, training)
    sums = torch.zeros(2, G, H, device="cuda", dtype=torch.float64)
    K.bn_bwd_reduce(h, G, st, gin, sums, drop=(p, SEED), seed_ptr=_ctr(ctr))
    dh = torch.full((N, H), float("nan"), device="cuda", dtype=dh_dtype)
    g = torch.Generator().manual_seed(3)
    prior_g, prior_b = torch.randn(H, generator=g).cuda(), torch.randn(H, generator=g).cuda()
    dgamma, dbeta = (prior_g.clone(), prior_b.clone()) if pgrads else (None, None)
    K.bn_bwd_apply(h, G, st, gin, sums, N // G, training, dh, dgamma, dbeta, drop=(p, SEED), seed_ptr=_ctr(ctr))
    torch.cuda.synchronize()

    h64 = h.double().requires_grad_(True)
    gamma = bn.weight.detach().double().requires_grad_(True)
    beta = bn.bias.detach().double().requires_grad_(True)
    y, _, _ = kr.bn_group_forward(h64, G, gamma, beta, bn.eps, training, rm0, rv0)
    out, _ = kr.bn_apply_ref(y, 1, resid.double(), _scale(N, H, p, ctr))
    (out * gin.double()).sum().backward()
    kr.close(dh, h64.grad, "dh", extra_rel=kr.BF16_REL if dh_dtype == torch.bfloat16 else 0.0)
    if pgrads:
        # accumulated onto the prior: the bar is that of the gradient itself, the prior adds one f32 rounding
        kr.close(dgamma.double() - prior_g.double(), gamma.grad, "dgamma - prior")
        kr.close(dbeta.double() - prior_b.double(), beta.grad, "dbeta - prior")
        assert not torch.equal(dgamma, prior_g) and not torch.equal(dbeta, prior_b)


# |mean| / std of the pre-BN activations: E[h^2] - mean^2 loses (mean/std)^2 of its leading digits
CONDITIONING = [(0.0, 1.0), (3.0, 1.0), (30.0, 1.0), (30.0, 0.1)]


@pytest.mark.parametrize("mean,std", CONDITIONING)
@pytest.mark.parametrize("N,H", [(512, 8), (130, 40)])
def test_normalised_output_is_as_well_conditioned_as_torch(N, H, mean, std):
    """Normalised output (gamma = 1, beta = 0, mode 0) within 8 * E_ref + 1e-6 * max|ref| of the fp64 reference, E_ref
    being the error of torch's own fp32 batch_norm (CPU) on the same input.  The margin of 8 covers the few f32
    roundings by which the operation order may differ; a cancellation error is orders of magnitude larger.
    Measured on an MI355X as E_ref / kernels with 64-row f32 partial sums (before) / with f64 sums (now):
      N=512 H=8   (0,1)    2.39e-7 / 2.88e-7 / 2.50e-7      N=130 H=40  (0,1)    3.27e-7 / 3.73e-7 / 3.21e-7
                  (3,1)    3.46e-7 / 3.96e-6 / 2.79e-7                  (3,1)    4.56e-7 / 7.14e-6 / 3.39e-7
                  (30,1)   3.19e-6 / 2.45e-4 / 7.82e-7                  (30,1)   2.36e-6 / 4.07e-4 / 1.18e-6
                  (30,0.1) 2.01e-5 / 2.33e-2 / 8.95e-6                  (30,0.1) 2.28e-5 / 5.06e-2 / 9.87e-6
    The f32 partial sums missed the bound at (30,1) and (30,0.1) for both shapes and at (3,1) for N=130."""
    K = _K()
    g = torch.Generator().manual_seed(N + int(mean * 10) + int(std * 100))
    x = (mean + std * torch.randn(N, H, generator=g)).float()
    x64 = x.double()
    eps = 1e-5
    ref = (x64 - x64.mean(0)) / (x64.var(0, unbiased=False) + eps).sqrt()
    e_ref = float((F.batch_norm(x, None, None, training=True, eps=eps).double() - ref).abs().max())
    xd = x.cuda()
    bn = torch.nn.BatchNorm1d(H, eps=eps).cuda()
    st = _stats(xd, 1, bn, True)
    out = torch.empty(N, H, device="cuda")
    K.bn_apply(xd, 1, st, 0, out)
    torch.cuda.synchronize()
    err = float((out.double().cpu() - ref).abs().max())
    bound = 8 * e_ref + 1e-6 * float(ref.abs().max())
    print(f"conditioning N={N} H={H} mean={mean} std={std}: E_ref={e_ref:.3e} kernel={err:.3e} bound={bound:.3e}")
    assert err <= bound, f"mean={mean} std={std} N={N} H={H}: kernel error {err:.3e} > bound {bound:.3e} " \
                         f"(E_ref {e_ref:.3e})"
