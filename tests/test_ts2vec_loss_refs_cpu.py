"""CPU-side checks of TS2Vec training: the restatement of tests/ts2vec_loss_refs.py against the fixture written by the
reference's losses.py / utils.py (tests/golden/ts2vec_loss.npz), the helpers ``fit`` is made of, and the argument
errors of the loss -- none of which needs a GPU."""
import numpy as np
import pytest
import torch

import ts2vec_loss_refs as L
import ts2vec_refs as R
from conftest import golden

N_CASES = 7
EPS32 = float(np.finfo(np.float32).eps)


@pytest.fixture(scope="module")
def fx():
    return golden("ts2vec_loss.npz")


def _case(fx, i):
    alpha, tu = fx[f"L{i}/cfg"]
    return fx[f"L{i}/z1"], fx[f"L{i}/z2"], float(alpha), int(tu)


@pytest.mark.parametrize("i", range(N_CASES))
def test_restatement_agrees_with_the_reference(fx, i):
    """The reference accumulates in f32: its loss carries a few roundings of the largest similarity (lse and the
    partner's S are each rounded at that magnitude, 8 eps covers their sum, the log and the f32 accumulation); the
    gradients must agree to 1e-6 of their maximum."""
    z1, z2, alpha, tu = _case(fx, i)
    loss, d1, d2 = L.loss_and_grads(L.hierarchical, z1, z2, torch.float64, alpha, tu)
    smax = max(float((torch.tensor(z) ** 2).sum(-1).max()) for z in (z1, z2))
    tol = 8 * EPS32 * max(1.0, smax)
    print(f"case {i}: loss {float(loss):.7f} reference {float(fx[f'L{i}/loss']):.7f} tol {tol:.2e}")
    assert abs(float(loss) - float(fx[f"L{i}/loss"])) <= tol
    for got, want in ((d1, fx[f"L{i}/dz1"]), (d2, fx[f"L{i}/dz2"])):
        gmax = max(float(np.abs(want).max()), float(got.abs().max()))
        assert float((got - torch.tensor(want).double()).abs().max()) <= 1e-6 * gmax


def test_single_terms_are_the_hierarchys_parts(fx):
    z1, z2, _, _ = _case(fx, 0)
    a, b = torch.tensor(z1).double(), torch.tensor(z2).double()
    one_level = 0.5 * L.nce_term(a[:, :1], b[:, :1], "instance")       # T = 1: the hierarchy is that one term
    assert float(L.hierarchical(a[:, :1], b[:, :1])) == float(one_level)


@pytest.mark.parametrize("layout, shape", [("instance", (1, 5, 16)), ("temporal", (3, 1, 16))])
def test_a_pair_alone_in_its_group_costs_exactly_zero(layout, shape):
    g = torch.Generator().manual_seed(11)
    z1, z2 = torch.randn(shape, generator=g) * 3, torch.randn(shape, generator=g) * 3
    for dtype in (torch.float32, torch.float64):
        lse, rl = L.nce_rows(z1.to(dtype), z2.to(dtype), layout)
        assert torch.count_nonzero(rl) == 0


# ------------------------------------------------------------------------------------------------ helpers
def test_helpers_equal_the_reference(fx):
    from arcweld.ts2vec import centerize_vary_length_series, split_with_nan, take_per_row
    got = take_per_row(torch.tensor(fx["take/A"]), fx["take/idx"], int(fx["take/n"]))
    assert np.array_equal(got.numpy(), fx["take/out"])
    parts = split_with_nan(fx["split/x"], int(fx["split/sections"]), axis=1)
    assert len(parts) == 3
    for j, part in enumerate(parts):
        assert np.array_equal(part, fx[f"split/out{j}"], equal_nan=True)
    assert np.array_equal(centerize_vary_length_series(fx["center/x"]), fx["center/out"], equal_nan=True)
    with pytest.raises(ValueError):
        split_with_nan(np.zeros((2, 4, 1), dtype=np.int64), 2, axis=1)


def test_the_crop_draw_replays_the_reference_order():
    from arcweld.ts2vec import draw_crops
    ts_l, B, tu = 37, 5, 1
    np.random.seed(77)
    c = draw_crops(ts_l, B, tu)
    np.random.seed(77)
    crop_l = np.random.randint(low=2 ** (tu + 1), high=ts_l + 1)
    left = np.random.randint(ts_l - crop_l + 1)
    eleft = np.random.randint(left + 1)
    eright = np.random.randint(low=left + crop_l, high=ts_l + 1)
    offset = np.random.randint(low=-eleft, high=ts_l - eright + 1, size=B)
    assert (c["crop_l"], c["left"], c["right"], c["eleft"], c["eright"]) == (crop_l, left, left + crop_l, eleft, eright)
    assert np.array_equal(c["offset"], offset)
    assert 2 ** (tu + 1) <= crop_l <= ts_l and 0 <= eleft <= left and left + crop_l <= eright <= ts_l


@pytest.mark.parametrize("seed", range(5))
def test_the_two_views_overlap_on_the_same_steps(seed):
    from arcweld.ts2vec import draw_crops, take_per_row
    np.random.seed(seed)
    x = torch.arange(6 * 40 * 2, dtype=torch.float32).reshape(6, 40, 2)
    c = draw_crops(40, 6)
    v1 = take_per_row(x, c["offset"] + c["eleft"], c["right"] - c["eleft"])[:, -c["crop_l"]:]
    v2 = take_per_row(x, c["offset"] + c["left"], c["eright"] - c["left"])[:, :c["crop_l"]]
    assert v1.shape == (6, c["crop_l"], 2) and torch.equal(v1, v2)


def test_masks_draw_from_numpy():
    from arcweld.ts2vec import binomial_mask, continuous_mask
    np.random.seed(3)
    m = binomial_mask(4, 9)
    np.random.seed(3)
    assert np.array_equal(m.numpy(), np.random.binomial(1, 0.5, size=(4, 9)).astype(bool))
    np.random.seed(4)
    c = continuous_mask(3, 50)
    assert c.shape == (3, 50) and c.dtype == torch.bool
    hidden = (~c).sum(1)
    assert ((hidden >= 5) & (hidden <= 25)).all()               # 5 runs of 5 steps, overlapping or not


def test_swa_mean_equals_torchs_averaged_model():
    """avg += (p - avg) / (n + 1) against torch.optim.swa_utils.AveragedModel, which may evaluate the same mean as a
    lerp: two f32 roundings of the largest parameter apart at the most."""
    from arcweld.ts2vec import TSEncoder, swa_update
    torch.manual_seed(5)
    net = TSEncoder(2, 16, hidden_dims=16, depth=1)
    ref = torch.optim.swa_utils.AveragedModel(net)
    ref.update_parameters(net)
    import copy
    avg, n = copy.deepcopy(net), 1
    for _ in range(3):
        with torch.no_grad():
            for p in net.parameters():
                p.add_(torch.randn_like(p) * 0.1)
        ref.update_parameters(net)
        n = swa_update(avg, net, n)
    assert n == 4 == int(ref.n_averaged)
    for (name, a), b in zip(avg.named_parameters(), ref.module.parameters()):
        assert float((a - b).detach().abs().max()) <= 2 * EPS32 * float(b.detach().abs().max()), name
        assert not torch.equal(a, dict(net.named_parameters())[name])
    fresh = copy.deepcopy(net)
    assert swa_update(fresh, avg, 0) == 1 and all(torch.equal(a, b) for a, b in zip(fresh.parameters(),
                                                                                    avg.parameters()))


# ------------------------------------------------------------------------------------------------ train_forward
def _cpu_encoder(seed=4301, p=0.0):
    from arcweld.ts2vec import TSEncoder
    sd = R.seeded_state(2, 32, 16, 2, seed=seed)
    enc = TSEncoder(2, 32, hidden_dims=16, depth=2)
    enc.load_state_dict(sd)
    enc.repr_dropout.p = p
    return sd, enc


def test_train_forward_equals_the_eval_restatement_without_randomness():
    sd, enc = _cpu_encoder()
    g = torch.Generator().manual_seed(9)
    x = torch.randn((3, 21, 2), generator=g)
    x[0, 4, :] = float("nan")
    x[2, 20, 1] = float("nan")
    before = x.clone()
    got = enc.train_forward(x, mask="all_true")
    assert torch.equal(torch.nan_to_num(x, nan=7.0), torch.nan_to_num(before, nan=7.0))      # the input is only read
    want64 = R.encode_ref(sd, x, None, torch.float64)
    want32 = R.encode_ref(sd, x, None, torch.float32)
    err, e_ref = L.error_ratio(got.detach(), want64, want32)
    assert err <= 4 * e_ref + 1e-7 and got.requires_grad
    # the differentiable restatement of this file's refs is the same function
    p32 = {k: v.float() for k, v in R.plain(sd).items()}
    assert float((L.encoder_forward(p32, x) - want32).abs().max()) <= 4 * e_ref + 1e-7


def test_train_forward_masks_and_dropout():
    sd, enc = _cpu_encoder()
    g = torch.Generator().manual_seed(10)
    x = torch.randn((2, 12, 2), generator=g)
    keep = torch.rand((2, 12), generator=g) > 0.4
    got = enc.train_forward(x, mask=keep)
    want = R.encode_ref(sd, x, keep, torch.float32)
    assert float((got.detach() - want).abs().max()) <= 1e-5
    np.random.seed(21)
    a = enc.train_forward(x)                                           # None / 'binomial': from np.random
    np.random.seed(21)
    m = torch.from_numpy(np.random.binomial(1, 0.5, size=(2, 12))).bool()
    assert torch.equal(a, enc.train_forward(x, mask=m))
    for name in ("continuous", "all_false", "mask_last"):
        assert enc.train_forward(x, mask=name).shape == (2, 12, 32)
    with pytest.raises(ValueError, match="mask"):
        enc.train_forward(x, mask="nope")
    with pytest.raises(ValueError, match="mask"):
        enc.train_forward(x, mask=torch.ones((2, 11), dtype=torch.bool))
    enc.repr_dropout.p = 0.5
    torch.manual_seed(1)
    dropped = enc.train_forward(x, mask="all_true")
    assert 0.3 < float((dropped == 0).float().mean()) < 0.7
    # encode keeps refusing the random masks
    with pytest.raises(ValueError, match="random masks"):
        enc.encode(x, mask="binomial")


def test_train_forward_gradients_reach_every_parameter():
    _, enc = _cpu_encoder()
    x = torch.randn((2, 9, 2), generator=torch.Generator().manual_seed(12))
    enc.train_forward(x, mask="all_true").square().sum().backward()
    assert all(p.grad is not None and torch.isfinite(p.grad).all() and p.grad.abs().max() > 0
               for p in enc.parameters())


# ------------------------------------------------------------------------------------------------ binding, arguments
def test_the_binding_has_the_loss_entry_points():
    from arcweld import _native as nat
    assert {"aw_nce_rows_fwd", "aw_nce_rows_bwd", "aw_nce_describe", "aw_ts_pool2_fwd",
            "aw_ts_pool2_bwd"} <= set(nat.SIGNATURES)
    assert (nat.AW_NCE_MAX_ROWS, nat.AW_NCE_MAX_GROUPS, nat.AW_NCE_MAX_WIDTH) == (8192, 65535, 512)
    assert len(nat.SIGNATURES["aw_nce_rows_fwd"]) == 10 and len(nat.SIGNATURES["aw_nce_rows_bwd"]) == 13


def test_the_drop_in_module_has_the_reference_names():
    import inspect
    from model.ts2vec import losses
    assert list(inspect.signature(losses.hierarchical_contrastive_loss).parameters) == ["z1", "z2", "alpha",
                                                                                        "temporal_unit"]
    for nm in ("instance_contrastive_loss", "temporal_contrastive_loss"):
        assert list(inspect.signature(getattr(losses, nm)).parameters) == ["z1", "z2"]


def test_loss_argument_errors():
    from arcweld import _native as nat
    from arcweld import kernels as k
    from arcweld.ts2vec import (hierarchical_contrastive_loss, instance_contrastive_loss,
                                temporal_contrastive_loss)
    z = torch.zeros((2, 8, 16))
    with pytest.raises(ValueError, match="multiple of 16"):
        hierarchical_contrastive_loss(torch.zeros((2, 8, 24)), torch.zeros((2, 8, 24)))
    with pytest.raises(ValueError, match="multiple of 16"):
        k.nce_rows_fwd(torch.zeros((2, 8, 24)), torch.zeros((2, 8, 24)), "temporal")
    with pytest.raises(ValueError, match="8192"):
        temporal_contrastive_loss(torch.zeros((1, 4097, 16)), torch.zeros((1, 4097, 16)))
    with pytest.raises(ValueError, match="8192"):
        instance_contrastive_loss(torch.zeros((4097, 1, 16)), torch.zeros((4097, 1, 16)))
    with pytest.raises(ValueError, match="8192"):
        k.nce_rows_fwd(torch.zeros((1, 4097, 16)), torch.zeros((1, 4097, 16)), "temporal")
    # temporal_unit moves the first temporal level below the bound; the instance term never sees T
    with pytest.raises(nat.NativeError):
        hierarchical_contrastive_loss(torch.zeros((1, 4100, 16)), torch.zeros((1, 4100, 16)), temporal_unit=1)
    with pytest.raises(ValueError, match="differ in shape"):
        hierarchical_contrastive_loss(z, torch.zeros((2, 7, 16)))
    with pytest.raises(ValueError, match="float32"):
        hierarchical_contrastive_loss(z.double(), z.double())
    with pytest.raises(ValueError, match="temporal_unit"):
        hierarchical_contrastive_loss(z, z, temporal_unit=-1)
    with pytest.raises(ValueError, match="layout"):
        k.nce_rows_fwd(z, z, "spatial")
    for fn in (hierarchical_contrastive_loss, instance_contrastive_loss, temporal_contrastive_loss):
        with pytest.raises(nat.NativeError, match="no CPU path"):
            fn(z, z)
    with pytest.raises(nat.NativeError):
        k.nce_rows_fwd(z, z, "instance")
    with pytest.raises(ValueError, match="T = 1"):
        k.ts_pool2_fwd(torch.zeros((2, 1, 16)))


def test_fit_bookkeeping_is_set_up_without_a_gpu():
    from model.ts2vec import TS2Vec
    m = TS2Vec(2, output_dims=16, hidden_dims=16, depth=1, device="cpu")
    assert m._net is m.net and m.n_averaged == 1 and m.n_epochs == 0 and m.n_iters == 0
    with pytest.raises(NotImplementedError, match="no CPU path"):
        m.fit(np.zeros((2, 8, 2)), n_iters=1)
