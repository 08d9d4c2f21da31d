"""The TS2Vec encoder's HIP forward (csrc/ts2vec.hip, arcweld.ts2vec.TSEncoder.encode) against the restatement of
tests/ts2vec_refs.py.

The tolerance rule (every comparison of values here): e_ref = max |restatement_f32 - restatement_f64| on the same
input is the reference arithmetic's own rounding; the kernels must satisfy max |gpu - restatement_f64| <= 4 e_ref
(the factor covers another summation order: the MFMA's k-ordered fmaf chain against the CPU's blocked sums, both
O(sqrt(K) eps) walks), and the project's standing 1e-4 fp32 bar on top.  Everything that the design makes exact --
sequence isolation, batch invariance, pooling -- is compared bit for bit.
"""
import itertools

import numpy as np
import pytest
import torch

import ts2vec_refs as R
from conftest import golden

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
FACTOR, CAP = 4.0, 1e-4


def _encoder(sd):
    from arcweld.ts2vec import encoder_from_state_dict
    return encoder_from_state_dict(sd, device=DEV)


def _hold(got, sd, x, mask, pooled, what):
    err, e_ref = R.error_ratio(got.cpu(), sd, x, mask, pooled)
    print(f"{what}: err {err:.3e} e_ref {e_ref:.3e} ratio {err / e_ref if e_ref else float('inf'):.2f}")
    assert err <= FACTOR * e_ref and err <= CAP, (what, err, e_ref)


def _inputs(seed, B, T, C, nan=True):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn((B, T, C), generator=g)
    if nan and T > 1:
        x[0, T // 2, :] = float("nan")
        x[B - 1, T - 1, C - 1] = float("nan")
    return x, torch.rand((B, T), generator=g) > 0.3


# ------------------------------------------------------------------------------------------------ fixtures
@pytest.fixture(scope="module")
def fixtures():
    out = {}
    for name in "abc":
        f = golden(f"ts2vec_{name}.npz")
        sd = {k[2:]: f[k] for k in f.files if k.startswith("w/")}
        out[name] = (f, sd, _encoder(sd))
    return out


@pytest.mark.parametrize("pooled", [False, True])
@pytest.mark.parametrize("mask", R.MASKS)
@pytest.mark.parametrize("name", "abc")
def test_fixture_parity(fixtures, name, mask, pooled):
    f, sd, enc = fixtures[name]
    j = 0
    while f"x{j}" in f.files:
        x = torch.tensor(f[f"x{j}"])
        explicit = torch.tensor(f[f"mask{j}"])
        arg = explicit if mask == "explicit" else mask
        got = enc.encode(x, mask=arg, encoding_window="full_series" if pooled else None)
        want = f[f"pool{j}/{mask}" if pooled else f"y{j}/{mask}"]
        assert tuple(got.shape) == want.shape
        _hold(got, sd, x, R.mask_of(mask, *x.shape[:2], explicit), pooled, f"fixture {name} x{j} {mask} pooled={pooled}")
        # the reference's own fp32 output is within its rounding of the same f64 values
        assert np.abs(got.cpu().numpy() - want).max() <= CAP
        j += 1


# ------------------------------------------------------------------------------------------------ default widths
@pytest.fixture(scope="module")
def default_net():
    sd = R.seeded_state(2, 320, 64, 10, seed=4201)
    return sd, _encoder(sd)


@pytest.mark.parametrize("B, T", [(2, 200), (1, 1000)])
def test_default_widths(default_net, B, T):
    """hidden 64, output 320, depth 10: the dilations 256, 512 and 1024 straddle T."""
    sd, enc = default_net
    x, _ = _inputs(4202 + T, B, T, 2)
    _hold(enc.encode(x), sd, x, None, False, f"default B={B} T={T}")
    _hold(enc.encode(x, encoding_window="full_series"), sd, x, None, True, f"default pooled B={B} T={T}")


# ------------------------------------------------------------------------------------------------ shape sweep
_FACTORS = dict(T=(1, 2, 31, 32, 33, 63, 65, 129), B=(1, 5), C=(1, 2, 8), hidden=(16, 48), out=(16, 80),
                depth=(1, 4, 8))


def _pairwise(factors):
    """A deterministic greedy pairwise-covering set of the factors' product: every pair of values of every two
    factors occurs in at least one case."""
    names = list(factors)
    pairs = {((a, va), (b, vb)) for a, b in itertools.combinations(names, 2) for va in factors[a] for vb in factors[b]}
    cases = []
    product = [dict(zip(names, vs)) for vs in itertools.product(*factors.values())]
    while pairs:
        def gain(c):
            return sum(((a, c[a]), (b, c[b])) in pairs for a, b in itertools.combinations(names, 2))
        best = max(product, key=gain)
        cases.append(best)
        pairs -= {((a, best[a]), (b, best[b])) for a, b in itertools.combinations(names, 2)}
    return cases


SWEEP = _pairwise(_FACTORS)


def test_sweep_covers_every_pair():
    assert len(SWEEP) < 40
    for a, b in itertools.combinations(_FACTORS, 2):
        assert {(c[a], c[b]) for c in SWEEP} == set(itertools.product(_FACTORS[a], _FACTORS[b]))


@pytest.mark.parametrize("i", range(len(SWEEP)))
def test_shape_sweep(i):
    c = SWEEP[i]
    sd = R.seeded_state(c["C"], c["out"], c["hidden"], c["depth"], seed=4300 + i)
    enc = _encoder(sd)
    x, explicit = _inputs(4400 + i, c["B"], c["T"], c["C"])
    mask = explicit if i % 2 else None
    pooled = bool(i % 3 == 0)
    got = enc.encode(x, mask=mask, encoding_window="full_series" if pooled else None)
    _hold(got, sd, x, mask, pooled, f"sweep {c}")


# ------------------------------------------------------------------------------------------------ exact properties
@pytest.fixture(scope="module")
def small_net():
    sd = R.seeded_state(2, 80, 48, 8, seed=4501)       # dilations 1..256 against T = 150: live and dead taps
    return sd, _encoder(sd)


def test_sequence_isolation(small_net):
    """No tap reads a neighbouring sequence: s1's output has the same bits whatever s0 and s2 hold."""
    _, enc = small_net
    x, _ = _inputs(4502, 3, 150, 2, nan=False)
    base = enc.encode(x)[1]
    for fill in (1e30, float("nan")):
        y = x.clone()
        y[0], y[2] = fill, fill
        out = enc.encode(y)
        assert torch.equal(out[1], base)
        assert torch.equal(enc.encode(y, encoding_window="full_series")[1],
                           enc.encode(x, encoding_window="full_series")[1])


def test_batch_invariance(small_net):
    """Alone, at any batch position, under any chunking -- the host's workspace split included: the same bits."""
    _, enc = small_net
    x, _ = _inputs(4503, 7, 150, 2)
    whole = enc.encode(x)
    pooled = enc.encode(x, encoding_window="full_series")
    for b in (0, 3, 6):
        assert torch.equal(enc.encode(x[b:b + 1])[0], whole[b])
    perm = torch.tensor([4, 0, 6, 2, 1, 5, 3])
    assert torch.equal(enc.encode(x[perm]), whole[perm])
    for bs in (1, 2, 3, 7, 100):
        assert torch.equal(enc.encode(x, batch_size=bs), whole)
        assert torch.equal(enc.encode(x, encoding_window="full_series", batch_size=bs), pooled)
    bound = enc.workspace_bytes
    try:
        enc.workspace_bytes = 2 * enc._bytes_per_sequence(150) + 8     # the host must split 7 sequences into 2 + 2 + 2 + 1
        assert torch.equal(enc.encode(x), whole)
        assert torch.equal(enc.encode(x, encoding_window="full_series"), pooled)
        enc.workspace_bytes = enc._bytes_per_sequence(150) - 4
        with pytest.raises(ValueError, match="workspace"):
            enc.encode(x)
    finally:
        enc.workspace_bytes = bound


@pytest.mark.parametrize("T", [1, 127, 128, 129, 300])
def test_pooling_is_the_max_over_time(small_net, T):
    """full_series == the max over time of the per-step output of the same call, bit for bit (max does not round)."""
    _, enc = small_net
    x, explicit = _inputs(4504 + T, 3, T, 2)
    for mask in (None, "mask_last", explicit):
        assert torch.equal(enc.encode(x, mask=mask, encoding_window="full_series"),
                           enc.encode(x, mask=mask).amax(1))


def test_missing_data(small_net):
    sd, enc = small_net
    x, _ = _inputs(4505, 2, 40, 2, nan=False)
    x[1] = float("nan")
    keep = x.clone()
    xd = x.to(DEV)
    for data in (x, xd, x.numpy()):
        got = enc.encode(data)
        assert torch.isfinite(got).all()
        _hold(got, sd, x, None, False, "all-NaN sequence")
    assert torch.equal(torch.isnan(x), torch.isnan(keep)) and torch.isnan(xd[1]).all() and torch.isnan(xd.cpu()[1]).all()
    # an all-NaN sequence is the all-masked one
    assert torch.equal(enc.encode(x)[1], enc.encode(torch.zeros_like(x), mask="all_false")[1])


def test_weights_are_relaid_out_once_per_load(small_net):
    sd, enc = small_net
    x, _ = _inputs(4506, 1, 20, 2)
    enc.encode(x)
    n = enc.n_relayouts
    enc.encode(x)
    enc.encode(x, encoding_window="full_series")
    assert enc.n_relayouts == n
    enc.load_state_dict({k: torch.as_tensor(v) for k, v in R.seeded_state(2, 80, 48, 8, seed=4507).items()})
    other = enc.encode(x)
    assert enc.n_relayouts == n + 1
    enc.load_state_dict({k: torch.as_tensor(v) for k, v in sd.items()})
    assert not torch.equal(other, enc.encode(x))


# ------------------------------------------------------------------------------------------------ limits
def test_largest_length():
    from arcweld.ts2vec import MAX_T
    sd = R.seeded_state(1, 16, 16, 1, seed=4601)
    enc = _encoder(sd)
    x, _ = _inputs(4602, 1, MAX_T, 1)
    _hold(enc.encode(x), sd, x, None, False, f"T = {MAX_T}")
    with pytest.raises(ValueError, match="data: sequence length"):
        enc.encode(torch.zeros(1, MAX_T + 1, 1))


def test_largest_widths():
    from arcweld.ts2vec import MAX_INPUT_DIMS, MAX_WIDTH
    sd = R.seeded_state(MAX_INPUT_DIMS, MAX_WIDTH, MAX_WIDTH, 1, seed=4603)
    enc = _encoder(sd)
    x, _ = _inputs(4604, 1, 33, MAX_INPUT_DIMS)
    _hold(enc.encode(x), sd, x, None, False, f"widths {MAX_WIDTH}")
    _hold(enc.encode(x, encoding_window="full_series"), sd, x, None, True, f"widths {MAX_WIDTH} pooled")


@pytest.mark.parametrize("kw, name", [(dict(input_dims=9, output_dims=16, hidden_dims=16), "input_dims"),
                                      (dict(input_dims=2, output_dims=528, hidden_dims=16), "output_dims"),
                                      (dict(input_dims=2, output_dims=16, hidden_dims=528), "hidden_dims"),
                                      (dict(input_dims=2, output_dims=24, hidden_dims=16), "output_dims"),
                                      (dict(input_dims=2, output_dims=16, hidden_dims=40), "hidden_dims")])
def test_encoder_refuses_widths_beyond_the_limits(kw, name):
    from arcweld.ts2vec import TSEncoder
    enc = TSEncoder(depth=1, **kw).to(DEV)
    with pytest.raises(ValueError, match=name):
        enc.encode(torch.zeros(1, 8, kw["input_dims"]))


def test_library_refuses_beyond_the_limits_without_a_launch():
    from arcweld import _native as nat
    from arcweld import kernels as k
    assert k.ts_describe() == (128, 64, 32)

    def conv(T=8, cin=16, cout=16, taps=3, dilation=1, batch=1):
        x = torch.zeros((batch * T, cin), device=DEV)
        out = torch.full((batch * T, cout), 7.0, device=DEV)
        w, b = torch.zeros((taps, cout, cin), device=DEV), torch.zeros(cout, device=DEV)
        try:
            k.ts_conv(x, w, b, batch, T, dilation, out=out)
        finally:
            torch.cuda.synchronize()
        return out

    assert float(conv().abs().max()) == 0.0                       # the call itself works
    for kw in (dict(T=nat.AW_TS_MAX_T + 1), dict(cin=nat.AW_TS_MAX_WIDTH + 16), dict(cout=nat.AW_TS_MAX_WIDTH + 16),
               dict(cin=24), dict(cout=40), dict(taps=2), dict(dilation=0), dict(dilation=nat.AW_TS_MAX_DILATION + 1)):
        with pytest.raises(nat.NativeError):
            conv(**kw)
    x = torch.zeros((8, 16), device=DEV)
    w, b = torch.zeros((3, 16, 16), device=DEV), torch.zeros(16, device=DEV)
    with pytest.raises(nat.NativeError, match="no output"):
        k.ts_conv(x, w, b, 1, 8, 1)
    out = torch.full((4, 24), 7.0, device=DEV)
    with pytest.raises(nat.NativeError):
        k.ts_input_fc(torch.zeros((4, 2), device=DEV), torch.zeros((24, 2), device=DEV), torch.zeros(24, device=DEV),
                      out=out, out_gelu=torch.empty_like(out))
    with pytest.raises(nat.NativeError):
        k.ts_input_fc(torch.zeros((4, 9), device=DEV), torch.zeros((16, 9), device=DEV), torch.zeros(16, device=DEV))
    torch.cuda.synchronize()
    assert float(out.min()) == 7.0 == float(out.max())            # refused before any launch


# ------------------------------------------------------------------------------------------------ end to end
def shapes_task(seed, n, T=64):
    """Two classes of (n, T, 2) sequences: a localised shape at a random position on noise -- class 1 a smooth bump,
    class 0 a one-sample-period zigzag of the same extent and energy."""
    g = torch.Generator().manual_seed(seed)
    y = torch.arange(n) % 2
    x = 0.1 * torch.randn((n, T, 2), generator=g)
    pos = torch.randint(0, T - 12, (n,), generator=g)
    bump = torch.hann_window(12, periodic=False)
    zig = bump * torch.tensor([1.0, -1.0]).repeat(6)
    for i in range(n):
        x[i, pos[i]:pos[i] + 12, 0] += 2.0 * (bump if y[i] else zig)
        x[i, pos[i]:pos[i] + 12, 1] -= 1.0 * (bump if y[i] else zig)
    return x, y


TASK = dict(sd=dict(input_dims=2, output_dims=32, hidden_dims=16, depth=4, seed=4701), sizes=(96, 32, 32), T=64)


def task_splits():
    return [shapes_task(4710 + i, n, TASK["T"]) for i, n in enumerate(TASK["sizes"])]


def decided_queries(feats_train, feats_q, tol):
    """Queries whose top-2 gap in standardised squared distance exceeds what a feature error of `tol` (the tolerance
    rule's bound on these features) can move: both rows of a pair may move by tol per feature."""
    f0, fq = feats_train.double(), feats_q.double()
    mean, var = f0.mean(0), f0.var(0, unbiased=False)
    scale = torch.where(var > 0, var.sqrt(), torch.ones_like(var))
    d = torch.cdist((fq - mean) / scale, (f0 - mean) / scale) ** 2
    top = d.topk(2, largest=False).values
    delta = float(((2 * tol / scale) ** 2).sum().sqrt())
    moved = 2 * top[:, 1].sqrt() * delta + delta ** 2
    return (top[:, 1] - top[:, 0]) > 2 * moved


def feature_tolerance(sd, splits, feats):
    e_ref = max(float((R.encode_ref(sd, x, dtype=torch.float32, pooled=True).double() - f).abs().max())
                for (x, _), f in zip(splits, feats))
    return min(FACTOR * e_ref, CAP)


def test_probe_on_ts2vec_features_end_to_end():
    """latent_knn_probe(dataset='ts2vec') predicts what the same protocol predicts on the restatement's features."""
    from arcweld.retrieve import latent_knn_probe
    sd = R.seeded_state(**TASK["sd"])
    enc = _encoder(sd)
    splits = task_splits()
    res = latent_knn_probe(splits, 1, k=1, dataset="ts2vec", ts2vec=enc, window=TASK["T"])
    feats = [R.encode_ref(sd, x, pooled=True) for x, _ in splits]
    Co = feats[0].shape[1]
    ref = latent_knn_probe([(f.float().reshape(-1, Co, 1), y) for f, (_, y) in zip(feats, splits)], 1, k=1,
                           dataset="asimow", window=Co)
    tol = feature_tolerance(sd, splits, feats)
    for i, nm in ((1, "val"), (2, "test")):
        sure = decided_queries(feats[0], feats[i], tol)
        assert float(sure.double().mean()) >= 0.95
        assert torch.equal(res[nm]["pred"].cpu()[sure], ref[nm]["pred"].cpu()[sure])
        print(f"{nm}: acc {res[nm]['acc']:.3f} (restatement {ref[nm]['acc']:.3f}), decided {int(sure.sum())}/{len(sure)}")
    from model.ts2vec import TS2Vec
    m = TS2Vec(2, output_dims=32, hidden_dims=16, depth=4, device=DEV)
    m.net.load_state_dict({k: torch.as_tensor(v) for k, v in sd.items()})
    out = m.encode(splits[1][0].numpy(), encoding_window="full_series")
    assert isinstance(out, np.ndarray) and np.array_equal(out, enc.encode(splits[1][0],
                                                                         encoding_window="full_series").cpu().numpy())
