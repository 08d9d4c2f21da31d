"""The fused TS2Vec loss kernels (csrc/ts2vec_loss.hip; arcweld.kernels.nce_rows_fwd / nce_rows_bwd / ts_pool2_*,
arcweld.ts2vec.hierarchical_contrastive_loss) against the restatement of tests/ts2vec_loss_refs.py.

The tolerance is the rule of tests/test_ts2vec_gpu.py: e_ref = max |restatement_f32 - restatement_f64| on the same
input is the reference arithmetic's own rounding, and the kernels must satisfy max |gpu - restatement_f64| <= 4 e_ref.
The scalar loss is itself rounded to f32 and its e_ref can be 0 by chance, so one f32 ulp of the loss is added there.
What the design makes exact -- a pair alone in its group, group isolation, run-to-run, accumulation -- is compared
bit for bit.  Every ratio is printed.
"""
import numpy as np
import pytest
import torch

import ts2vec_loss_refs as L
from conftest import golden

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
FACTOR = 4.0


def _hold(what, got, r64, r32, extra=0.0):
    err, e_ref = L.error_ratio(got.detach().cpu(), r64, r32)
    print(f"{what}: err {err:.3e} e_ref {e_ref:.3e} ratio {err / e_ref if e_ref else float('inf') if err else 0:.2f}")
    assert err <= FACTOR * e_ref + extra, (what, err, e_ref)
    return err / e_ref if e_ref else 0.0


def _views(seed, B, T, C, scale=0.5):
    g = torch.Generator().manual_seed(seed)
    z1 = torch.randn((B, T, C), generator=g) * scale
    return z1, 0.5 * z1 + torch.randn((B, T, C), generator=g) * scale


def _ulp(v):
    return float(np.spacing(np.float32(abs(float(v)))))


# ------------------------------------------------------------------------------------------------ row kernels
_ref_cache = {}


def _rows_ref(key, z1, z2, layout, scale):
    """The restatement in both precisions, computed once per case and shared (never modified)."""
    if key not in _ref_cache:
        _ref_cache[key] = (L.rows_grads(z1, z2, layout, torch.float64, scale),
                           L.rows_grads(z1, z2, layout, torch.float32, scale))
    return _ref_cache[key]


ROW_CASES = [  # (layout, B, T, C, input scale): temporal G = B, N = T; instance G = T, N = B
    ("temporal", 2, 5, 16, 0.5),
    ("temporal", 3, 16, 32, 0.5),        # 2N = 32: four groups per workgroup, the last workgroup not full
    ("temporal", 5, 17, 16, 0.5),        # 2N = 34: the first size in slots of 64, two groups per workgroup
    ("temporal", 2, 32, 16, 0.5),        # 2N = 64
    ("temporal", 3, 64, 32, 0.5),        # 2N = 128: the last packed size, one group per workgroup
    ("temporal", 2, 65, 16, 0.5),        # 2N = 130: the first size swept tile by tile
    ("temporal", 2, 70, 48, 0.5),        # ragged tiles, C not a multiple of the 32-dim chunk
    ("temporal", 1, 129, 16, 0.5),       # two tiles per half, the second of one row
    ("temporal", 2, 128, 320, 0.15),     # the default width: three backward slabs, the last of 64 columns
    ("instance", 3, 9, 16, 0.5),         # G = 9, N = 3
    ("instance", 16, 130, 32, 0.5),      # G = 130, N = 16
    ("temporal", 2, 70, 64, 6.0),        # peaked: similarities in the thousands
    ("instance", 5, 3, 64, 6.0),
]


@pytest.mark.parametrize("layout, B, T, C, zs", ROW_CASES)
def test_row_kernels(layout, B, T, C, zs):
    from arcweld import kernels as k
    z1, z2 = _views(6000 + B * 1000 + T, B, T, C, zs)
    scale = 0.37
    (lse64, rl64, a64, b64), (lse32, rl32, a32, b32) = _rows_ref((layout, B, T, C, zs), z1, z2, layout, scale)
    d1, d2 = z1.to(DEV), z2.to(DEV)
    lse, rl = k.nce_rows_fwd(d1, d2, layout)
    G, N = (B, T) if layout == "temporal" else (T, B)
    assert lse.shape == rl.shape == (G, 2 * N)
    tag = f"{layout} G={G} N={N} C={C} x{zs}"
    _hold(f"{tag} lse", lse, lse64, lse32)
    _hold(f"{tag} row_loss", rl, rl64, rl32)
    g1, g2 = torch.full_like(d1, float("nan")), torch.full_like(d2, float("nan"))
    k.nce_rows_bwd(d1, d2, layout, lse, scale, g1, g2)
    _hold(f"{tag} dz1", g1, a64, a32)
    _hold(f"{tag} dz2", g2, b64, b32)
    assert torch.isfinite(g1).all() and torch.isfinite(g2).all()       # every element was written


@pytest.mark.parametrize("layout, shape", [("temporal", (1, 1, 16)), ("instance", (1, 4, 16)), ("temporal", (3, 1, 32))])
def test_a_pair_alone_in_its_group_is_exactly_zero(layout, shape):
    from arcweld import kernels as k
    z1, z2 = (t.to(DEV) for t in _views(61, *shape, scale=3.0))
    lse, rl = k.nce_rows_fwd(z1, z2, layout)
    assert torch.count_nonzero(rl) == 0
    r64 = L.nce_rows(z1.cpu().double(), z2.cpu().double(), layout)[0]
    r32 = L.nce_rows(z1.cpu(), z2.cpu(), layout)[0]
    _hold(f"{layout} {shape} lse", lse, r64, r32, extra=_ulp(r64.abs().max()))
    g1, g2 = torch.full_like(z1, 7.0), torch.full_like(z2, 7.0)
    k.nce_rows_bwd(z1, z2, layout, lse, 0.5, g1, g2)
    assert torch.count_nonzero(g1) == 0 and torch.count_nonzero(g2) == 0
    from arcweld.ts2vec import hierarchical_contrastive_loss
    if shape == (1, 1, 16):
        a, b = z1.clone().requires_grad_(True), z2.clone().requires_grad_(True)
        loss = hierarchical_contrastive_loss(a, b)
        loss.backward()
        assert float(loss) == 0.0 and torch.count_nonzero(a.grad) == 0 and torch.count_nonzero(b.grad) == 0


def _fwd_bwd(z1, z2, layout, scale=0.37):
    from arcweld import kernels as k
    lse, rl = k.nce_rows_fwd(z1, z2, layout)
    g1, g2 = torch.empty_like(z1), torch.empty_like(z2)
    k.nce_rows_bwd(z1, z2, layout, lse, scale, g1, g2)
    return lse, rl, g1, g2


def test_a_group_does_not_depend_on_its_batch():
    z1, z2 = (t.to(DEV) for t in _views(62, 3, 70, 48))
    lse, rl, g1, g2 = _fwd_bwd(z1, z2, "temporal")
    a, b = z1[1:2].contiguous(), z2[1:2].contiguous()
    lse1, rl1, h1, h2 = _fwd_bwd(a, b, "temporal")
    assert torch.equal(lse[1:2], lse1) and torch.equal(rl[1:2], rl1)
    assert torch.equal(g1[1:2], h1) and torch.equal(g2[1:2], h2)
    # packed groups (2N = 40: slots of 64, two per workgroup): a group has the same bits in either slot and alone
    y1, y2 = (t.to(DEV) for t in _views(162, 5, 20, 32))
    lse, rl, g1, g2 = _fwd_bwd(y1, y2, "temporal")
    for b in (1, 4):
        lse1, rl1, h1, h2 = _fwd_bwd(y1[b:b + 1].contiguous(), y2[b:b + 1].contiguous(), "temporal")
        assert torch.equal(lse[b:b + 1], lse1) and torch.equal(rl[b:b + 1], rl1)
        assert torch.equal(g1[b:b + 1], h1) and torch.equal(g2[b:b + 1], h2)
    # the instance layout: a group is a time step
    lse, rl, g1, g2 = _fwd_bwd(z1, z2, "instance")
    a, b = z1[:, 5:6].contiguous(), z2[:, 5:6].contiguous()
    lse1, rl1, h1, h2 = _fwd_bwd(a, b, "instance")
    assert torch.equal(lse[5:6], lse1) and torch.equal(rl[5:6], rl1)
    assert torch.equal(g1[:, 5:6], h1) and torch.equal(g2[:, 5:6], h2)


def test_two_runs_give_the_same_bits():
    from arcweld.ts2vec import hierarchical_contrastive_loss
    z1, z2 = (t.to(DEV) for t in _views(63, 2, 150, 80))
    first = _fwd_bwd(z1, z2, "temporal")
    second = _fwd_bwd(z1, z2, "temporal")
    assert all(torch.equal(a, b) for a, b in zip(first, second))
    outs = []
    for _ in range(2):
        a, b = z1.clone().requires_grad_(True), z2.clone().requires_grad_(True)
        loss = hierarchical_contrastive_loss(a, b)
        loss.backward()
        outs.append((loss.detach(), a.grad, b.grad))
    assert all(torch.equal(a, b) for a, b in zip(*outs))


def test_accumulate_adds_to_what_is_there():
    from arcweld import kernels as k
    z1, z2 = (t.to(DEV) for t in _views(64, 3, 40, 32))
    lse_t, _ = k.nce_rows_fwd(z1, z2, "temporal")
    lse_i, _ = k.nce_rows_fwd(z1, z2, "instance")
    parts = []
    for layout, lse, s in (("temporal", lse_t, 0.25), ("instance", lse_i, 0.5)):
        g1, g2 = torch.empty_like(z1), torch.empty_like(z2)
        k.nce_rows_bwd(z1, z2, layout, lse, s, g1, g2)
        parts.append((g1, g2))
    a1, a2 = torch.empty_like(z1), torch.empty_like(z2)
    k.nce_rows_bwd(z1, z2, "temporal", lse_t, 0.25, a1, a2, accumulate=False)
    k.nce_rows_bwd(z1, z2, "instance", lse_i, 0.5, a1, a2, accumulate=True)
    assert torch.equal(a1, parts[0][0] + parts[1][0]) and torch.equal(a2, parts[0][1] + parts[1][1])


def test_pool2_kernels():
    from arcweld import kernels as k
    g = torch.Generator().manual_seed(65)
    x = torch.randn((3, 9, 48), generator=g)
    x[:, 3] = x[:, 2]                                                    # a tie: the first step takes the gradient
    x[0, 5, :8] = x[0, 4, :8]
    xd = x.to(DEV)
    y = k.ts_pool2_fwd(xd)
    xr = x.clone().requires_grad_(True)
    yr = L.pool2(xr)
    assert torch.equal(y.cpu(), yr.detach())
    dy = torch.randn((3, 4, 48), generator=g)
    yr.backward(dy)
    din = torch.full_like(xd, 2.0)
    k.ts_pool2_bwd(xd, dy.to(DEV), din)
    assert torch.equal(din.cpu(), xr.grad + 2.0)                          # adds; the odd last step keeps its 2.0
    assert torch.count_nonzero(xr.grad[:, 3]) == 0 and torch.equal(din[:, 8].cpu(), torch.full((3, 48), 2.0))


# ------------------------------------------------------------------------------------------------ hierarchy
def _hier_check(tag, z1, z2, alpha=0.5, tu=0, d1=None, d2=None):
    """d1 / d2: the device views to pass (default: contiguous copies of z1 / z2)."""
    from arcweld.ts2vec import hierarchical_contrastive_loss
    l64, a64, b64 = L.loss_and_grads(L.hierarchical, z1, z2, torch.float64, alpha, tu)
    l32, a32, b32 = L.loss_and_grads(L.hierarchical, z1, z2, torch.float32, alpha, tu)
    a = (torch.as_tensor(z1).to(DEV) if d1 is None else d1).requires_grad_(True)
    b = (torch.as_tensor(z2).to(DEV) if d2 is None else d2).requires_grad_(True)
    loss = hierarchical_contrastive_loss(a, b, alpha=alpha, temporal_unit=tu)
    assert loss.dtype == torch.float32 and loss.dim() == 0
    loss.backward()
    ga = a.grad if a.grad is not None else torch.zeros_like(a)
    gb = b.grad if b.grad is not None else torch.zeros_like(b)
    _hold(f"{tag} loss", loss, l64, l32, extra=_ulp(l64))
    _hold(f"{tag} dz1", ga, a64, a32)
    _hold(f"{tag} dz2", gb, b64, b32)
    return loss, ga, gb


@pytest.mark.parametrize("i", range(7))
def test_hierarchy_on_the_fixture_cases(i):
    fx = golden("ts2vec_loss.npz")
    alpha, tu = fx[f"L{i}/cfg"]
    loss, _, _ = _hier_check(f"fixture {i}", fx[f"L{i}/z1"], fx[f"L{i}/z2"], float(alpha), int(tu))
    # the reference's own f32 value: the bound of tests/test_ts2vec_loss_refs_cpu.py, plus the kernel's rounding
    smax = max(float((torch.tensor(fx[f"L{i}/{z}"]) ** 2).sum(-1).max()) for z in ("z1", "z2"))
    assert abs(float(loss) - float(fx[f"L{i}/loss"])) <= 16 * float(np.finfo(np.float32).eps) * max(1.0, smax)


def test_hierarchy_with_odd_drops():
    _hier_check("4x200x64", *_views(66, 4, 200, 64, 0.3))               # 200 100 50 25 12 6 3 1


def test_hierarchy_of_one_sequence_and_of_one_step():
    _hier_check("B=1", *_views(67, 1, 37, 16))
    _hier_check("T=1", *_views(68, 5, 1, 32))
    _hier_check("temporal_unit=2", *_views(69, 2, 40, 16), alpha=0.3, tu=2)


def test_hierarchy_sends_a_tied_gradient_to_the_first_step():
    z1, z2 = _views(70, 2, 16, 16)
    z1[:, 1::2] = z1[:, 0::2]                                            # every pair the first pooling sees is a tie
    z2[:, 1::2] = z2[:, 0::2]
    _, ga, gb = _hier_check("ties", z1, z2)
    # level 0's own terms treat the equal steps alike; what comes up from the pooled levels lands on the even steps
    l0 = L.loss_and_grads(lambda a, b: (0.5 * L.nce_term(a, b, "instance") + 0.5 * L.nce_term(a, b, "temporal")) / 5,
                          z1, z2, torch.float64)
    up_even = (ga.cpu().double() - l0[1])[:, 0::2].abs().max()
    up_odd = (ga.cpu().double() - l0[1])[:, 1::2].abs().max()
    print(f"ties: pooled-level gradient on even steps {float(up_even):.3e}, on odd steps {float(up_odd):.3e}")
    assert up_odd <= 1e-3 * up_even


def test_non_contiguous_views_are_accepted():
    z1, z2 = _views(71, 3, 30, 32)
    wide1, wide2 = torch.zeros((3, 41, 32)), torch.zeros((3, 41, 32))
    wide1[:, -30:] = z1
    wide2[:, :30] = z2
    d1, d2 = wide1.to(DEV)[:, -30:], wide2.to(DEV)[:, :30]
    assert not d1.is_contiguous() and not d2.is_contiguous()
    d1, d2 = d1.detach(), d2.detach()
    loss, ga, gb = _hier_check("slices", z1, z2, d1=d1, d2=d2)
    dense = _hier_check("dense", z1, z2)
    assert torch.equal(loss, dense[0]) and torch.equal(ga, dense[1]) and torch.equal(gb, dense[2])


def test_single_terms():
    from arcweld.ts2vec import instance_contrastive_loss, temporal_contrastive_loss
    z1, z2 = _views(72, 4, 20, 32)
    for fn, layout in ((instance_contrastive_loss, "instance"), (temporal_contrastive_loss, "temporal")):
        ref = lambda a, b: L.nce_term(a, b, layout)                      # noqa: E731
        l64, a64, b64 = L.loss_and_grads(ref, z1, z2, torch.float64)
        l32, a32, b32 = L.loss_and_grads(ref, z1, z2, torch.float32)
        a, b = z1.to(DEV).requires_grad_(True), z2.to(DEV).requires_grad_(True)
        loss = fn(a, b)
        (2.0 * loss).backward()                                          # an upstream gradient other than 1
        _hold(f"{layout} term", loss, l64, l32, extra=_ulp(l64))
        _hold(f"{layout} term dz1", a.grad, 2 * a64, 2 * a32)
        _hold(f"{layout} term dz2", b.grad, 2 * b64, 2 * b32)


def test_memory_stays_linear_in_the_rows():
    """B = 2, T = 2048, C = 64: pooled levels < 2x the inputs' bytes, level gradients < 2x, the outputs 1x, the row
    statistics negligible -- 8x is the bound; one (2T)^2 f32 similarity per sequence alone would be 32x."""
    from arcweld.ts2vec import hierarchical_contrastive_loss
    z1, z2 = (t.to(DEV).requires_grad_(True) for t in _views(73, 2, 2048, 64, 0.2))
    hierarchical_contrastive_loss(z1[:, :64], z2[:, :64]).backward()     # the library is loaded, caches are warm
    z1.grad = z2.grad = None
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    loss = hierarchical_contrastive_loss(z1, z2)
    loss.backward()
    torch.cuda.synchronize()
    rise = torch.cuda.max_memory_allocated() - base
    inputs = 2 * z1.numel() * 4
    print(f"memory: peak rise {rise} bytes = {rise / inputs:.2f} x the inputs ({inputs} bytes)")
    assert rise <= 8 * inputs and torch.isfinite(loss) and torch.isfinite(z1.grad).all()
