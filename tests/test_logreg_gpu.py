"""aw_logreg_forward / aw_logreg_grad (csrc/logreg.hip), the fit built on them (arcweld.retrieve.logreg_fit) and the
linear probe (latent_linear_probe, probe_latent_space.py --protocol linear) against the fp64 restatements of
tests/logreg_refs.py.  Sizes come from aw_logreg_describe: below, at and above a row tile, a dim chunk and a dim tile.
Buffers are placed as in tests/test_knn_gpu.py: the inputs inside NaN-filled allocations with NaN row padding and odd
base offsets (a read outside a row's d values would surface as a NaN), the outputs between canaries.

Exact block: integer features in -4..4 with w = 0, b = 0 give z = 0 and r = 1/2 - t exactly, every gradient sum is a
sum of half-integers far below 2^24: z, r, g and gb must equal the fp64 values bit for bit, the loss must be
(rows taking part) * ln 2 within its bound.  Random block: every element within the bounds derived in logreg_refs
(checked against an f32 evaluation on the CPU in tests/test_logreg_refs_cpu.py); no case is left out.

Fit: the three conditions of logreg_refs.fit_conditions, on the inputs and tolerances tests/test_logreg_refs_cpu.py
checks with an f32 evaluation under scipy's L-BFGS-B."""
import itertools
import json

import numpy as np
import pytest
import torch

import knn_refs as KR
import logreg_refs as R
from oracle import gen
from oracle import vqvae as ov

pytestmark = pytest.mark.gpu

PAD = 64
CANARY = -1234.5


@pytest.fixture(scope="module")
def tiles():
    from arcweld import kernels as K
    tn, cd, td, mp = K.logreg_describe()
    assert mp == 32 and tn >= 4 and cd >= 4 and td >= cd
    return tn, cd, td


def _place(a, pad=0, off=0):
    """(n, D) array on the device inside a NaN-filled buffer: rows D + pad floats apart, the first ``off`` floats into
    the allocation; the padding and both margins are NaN."""
    a = np.ascontiguousarray(a, dtype=np.float32)
    n, D = a.shape
    ld = D + pad
    buf = torch.full((off + n * ld + PAD,), float("nan"), device="cuda")
    view = buf.as_strided((n, D), (ld, 1), off)
    if n:
        view.copy_(torch.as_tensor(a))
    return view


def _compact(a, dtype=np.float32):
    """A compact array on the device with NaN margins on both sides (float) or as it is (int)."""
    a = np.ascontiguousarray(a, dtype=dtype)
    if dtype != np.float32:
        return torch.as_tensor(a, device="cuda")
    buf = torch.full((a.size + 2 * PAD,), float("nan"), device="cuda")
    view = buf[PAD:PAD + a.size].view(a.shape)
    view.copy_(torch.as_tensor(a))
    return view


class _Out:
    """An output between canaries."""

    def __init__(self, shape, dtype):
        self.n = int(np.prod(shape))
        self.buf = torch.full((self.n + 2 * PAD,), CANARY, dtype=dtype, device="cuda")
        self.view = self.buf[PAD:PAD + self.n].view(shape)

    def check(self, untouched=False):
        assert bool((self.buf[:PAD] == CANARY).all() and (self.buf[PAD + self.n:] == CANARY).all()), \
            "an output canary was written"
        if untouched:
            assert bool((self.buf == CANARY).all()), "an output was written by a refused call"
        return self.view.cpu().numpy()


def _run(x, w, b, y=None, cls=None, splits=None, pad=0, off=0, xd=None):
    """One forward (+ gradient with labels); dict of numpy outputs after checking the canaries."""
    from arcweld import kernels as K
    n, d = x.shape
    p = w.shape[1]
    xd = _place(x, pad, off) if xd is None else xd
    wd, bd = _compact(w), _compact(b)
    z = _Out((n, p), torch.float32)
    if y is None:
        K.logreg_forward(xd, wd, bd, z=z.view)
        torch.cuda.synchronize()
        return {"z": z.check()}
    r, loss, gb, g = _Out((n, p), torch.float32), _Out((p,), torch.float64), _Out((p,), torch.float64), \
        _Out((d, p), torch.float64)
    K.logreg_forward(xd, wd, bd, _compact(y, np.int32), _compact(cls, np.int32), z=z.view, r=r.view, loss=loss.view,
                     gb=gb.view)
    K.logreg_grad(xd, r.view, splits=splits, g=g.view)
    torch.cuda.synchronize()
    return {"z": z.check(), "r": r.check(), "loss": loss.check(), "gb": gb.check(), "g": g.check()}


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32 if a.dtype == np.float32 else np.uint64)


def _ints(seed, n, d):
    return gen.randint(seed, (n, d), -4, 5).astype(np.float32)


def _labels(seed, n, p):
    """Class ids -1 (the row takes no part) .. 3, and the problems' classes: 0..3 in turn, with class 7 -- which no
    row has -- at position 1."""
    y = gen.randint(seed, (n,), -1, 4)
    cls = np.arange(p) % 4
    if p >= 2:
        cls[1] = 7
    return y, cls


# ------------------------------------------------------------------------------------------------ the selection
# A pairwise-covering selection of the 5 x 6 x 4 x 2 x 2 grid (positions in the value lists of _case: n, d, p, row
# padding, base offset), built greedily in a fixed order: every pair of values of every two parameters meets in some
# case.  test_the_selection_covers_every_pair checks it.
GRID = (5, 6, 4, 2, 2)


def _greedy_pairwise(grid):
    cells = list(itertools.product(*(range(g) for g in grid)))
    axes = list(itertools.combinations(range(len(grid)), 2))
    todo = {(a, b, va, vb) for a, b in axes for va in range(grid[a]) for vb in range(grid[b])}
    picked = []
    while todo:
        best = max(cells, key=lambda c: sum((a, b, c[a], c[b]) in todo for a, b in axes))
        picked.append(best)
        todo -= {(a, b, best[a], best[b]) for a, b in axes}
    return tuple(picked)


SELECTION = _greedy_pairwise(GRID)
N_CASES = len(SELECTION)


def _case(i, tiles):
    tn, cd, td = tiles
    a, b, c, e, f = SELECTION[i]
    n = (1, tn - 1, tn, tn + 1, 2 * tn + 3)[a]
    d = (1, cd - 1, cd, cd + 1, 2 * cd + 5, td + 1)[b]
    p = (1, 2, 31, 32)[c]
    return n, d, p, (0, 3)[e], (0, 1)[f]


def test_the_selection_covers_every_pair():
    assert 30 <= N_CASES <= 48
    for a in range(5):
        for b in range(a + 1, 5):
            assert len({(c[a], c[b]) for c in SELECTION}) == GRID[a] * GRID[b], (a, b)


# ------------------------------------------------------------------------------------------------ exact block
def _assert_exact(got, x, y, cls, label):
    n, d = x.shape
    p = len(cls)
    want = R.bounds(x, np.zeros((d, p)), np.zeros(p), y, cls)
    assert np.array_equal(_bits(got["z"]), _bits(np.zeros((n, p), np.float32))), f"{label}: z"
    assert np.array_equal(_bits(got["r"]), _bits(want["r"].astype(np.float32))), f"{label}: r"
    assert np.array_equal(want["r"].astype(np.float32).astype(np.float64), want["r"])      # r is exact in f32
    assert np.array_equal(_bits(got["g"]), _bits(want["g"] + 0.0)), f"{label}: g"
    assert np.array_equal(_bits(got["gb"]), _bits(want["gb"] + 0.0)), f"{label}: gb"
    active = int((y >= 0).sum())
    assert np.allclose(want["loss"], active * np.log(2.0), rtol=1e-12, atol=0)
    err = np.abs(got["loss"] - want["loss"])
    print(f"{label}: max |loss - n ln 2| / eps = {(err / np.maximum(want['eps_loss'], 1e-300)).max():.3g}")
    assert (err <= want["eps_loss"]).all(), f"{label}: loss"


@pytest.mark.parametrize("i", range(N_CASES))
def test_exact_on_integer_features(tiles, i):
    n, d, p, pad, off = _case(i, tiles)
    x = _ints(1000 + i, n, d)
    y, cls = _labels(2000 + i, n, p)
    got = _run(x, np.zeros((d, p)), np.zeros(p), y, cls, pad=pad, off=off)
    _assert_exact(got, x, y, cls, f"n={n} d={d} p={p} pad={pad} off={off}")


def test_exact_when_all_rows_share_a_class(tiles):
    tn, cd, td = tiles
    n, d, p = 2 * tn + 3, cd + 1, 3
    x = _ints(31, n, d)
    y, cls = np.full(n, 2), np.array([2, 0, 7])
    got = _run(x, np.zeros((d, p)), np.zeros(p), y, cls, pad=1)
    _assert_exact(got, x, y, cls, "one class")
    assert (got["r"][:, 0] == -0.5).all() and (got["r"][:, 1:] == 0.5).all()
    none = _run(x, np.zeros((d, p)), np.zeros(p), np.full(n, -1), cls)         # no row takes part
    assert (none["r"] == 0).all() and (none["loss"] == 0).all() and (none["gb"] == 0).all() and (none["g"] == 0).all()


def test_no_rows(tiles):
    d, p = 5, 3
    got = _run(np.zeros((0, d), np.float32), gen.normal(1, (d, p)), gen.normal(2, (p,)), np.zeros(0, np.int64),
               np.arange(p))
    assert got["z"].shape == (0, p)
    for k in ("loss", "gb", "g"):
        assert (got[k] == 0).all(), k


# ------------------------------------------------------------------------------------------------ random block
def _assert_within(got, x, w, b, y, cls, label):
    bd = R.bounds(x, w, b, y, cls)
    for name in ("z", "r", "loss", "gb", "g"):
        assert np.isfinite(got[name]).all(), f"{label}: {name} is not finite"
        err, eps = np.abs(got[name].astype(np.float64) - bd[name]), bd["eps_" + name]
        print(f"{label}: max |{name} - fp64| / eps = {(err / np.maximum(eps, 1e-300)).max():.3g}")
        assert (err <= eps).all(), f"{label}: {name} is off by more than its bound"
    assert (got["r"][np.asarray(y) < 0] == 0).all()
    return bd


def _random(seed, n, d, p, scale=1.0):
    x = gen.normal(seed, (n, d))
    w = gen.normal(seed + 1, (d, p), std=scale / np.sqrt(d))
    b = gen.normal(seed + 2, (p,), std=0.5)
    return x, w, b


@pytest.mark.parametrize("i", range(N_CASES))
def test_random_features_within_the_derived_bounds(tiles, i):
    n, d, p, pad, off = _case(i, tiles)
    x, w, b = _random(3000 + 3 * i, n, d, p)
    y, cls = _labels(4000 + i, n, p)
    label = f"n={n} d={d} p={p} pad={pad} off={off}"
    got = _run(x, w, b, y, cls, pad=pad, off=off)
    _assert_within(got, x, w, b, y, cls, label)
    only_z = _run(x, w, b, pad=pad, off=off)                  # without labels: the same decision values
    assert np.array_equal(_bits(only_z["z"]), _bits(got["z"])), label


def test_both_tails_of_softplus_and_sigma(tiles):
    tn, cd, td = tiles
    n, d, p = 2 * tn + 3, 2 * cd + 5, 32
    x, w, b = _random(51, n, d, p, scale=16.0)
    y, cls = _labels(52, n, p)
    got = _run(x, w, b, y, cls, pad=3, off=1)
    bd = _assert_within(got, x, w, b, y, cls, "tails")
    assert bd["z"].max() > 45 and bd["z"].min() < -45 and np.abs(bd["z"]).max() < 100


def test_launches_and_split_counts(tiles):
    tn, cd, td = tiles
    n, d, p = 2 * tn + 3, td + 1, 31
    x, w, b = _random(61, n, d, p)
    y, cls = _labels(62, n, p)
    xd = _place(x, 3, 1)
    ref = _run(x, w, b, y, cls, xd=xd)
    for sp in (None, 1, 2, 7):
        a, c = _run(x, w, b, y, cls, splits=sp, xd=xd), _run(x, w, b, y, cls, splits=sp, xd=xd)
        for name in ("z", "r", "loss", "gb", "g"):
            assert np.array_equal(_bits(a[name]), _bits(c[name])), f"splits={sp}: {name} differs between launches"
        for name in ("z", "r", "loss", "gb"):                 # the forward does not depend on the gradient's splits
            assert np.array_equal(_bits(a[name]), _bits(ref[name])), f"splits={sp}: {name}"
        _assert_within(a, x, w, b, y, cls, f"splits={sp}")


def test_refused_calls_launch_nothing(tiles):
    from arcweld import _native as nat
    from arcweld import kernels as K
    lib = nat.load()
    n, d, p = 9, 7, 3
    xd = _place(gen.normal(71, (n, d)), 1, 0)
    ldx = xd.stride(0)
    wd, bd = _compact(gen.normal(72, (d, p))), _compact(gen.normal(73, (p,)))
    y, cls = _compact(np.zeros(n), np.int32), _compact(np.arange(p), np.int32)
    ws = K.logreg_workspace(n, d, p, device="cuda")
    outs = {k: _Out(s, t) for k, (s, t) in {"z": ((n, 32), torch.float32), "r": ((n, 32), torch.float32),
                                            "loss": ((32,), torch.float64), "gb": ((32,), torch.float64),
                                            "g": ((d, 32), torch.float64)}.items()}
    P = lambda t: None if t is None else t.data_ptr()  # noqa: E731
    o = {k: v.view for k, v in outs.items()}

    def fwd(x=xd, n=n, ldx=ldx, d=d, w=wd, b=bd, p=p, y=y, cls=cls, z=o["z"], r=o["r"], loss=o["loss"], gb=o["gb"],
            ws=ws, ws_bytes=None):
        return lib.aw_logreg_forward(P(x), n, ldx, d, P(w), P(b), p, P(y), P(cls), P(z), P(r), P(loss), P(gb), P(ws),
                                     ws.numel() if ws_bytes is None and ws is not None else (ws_bytes or 0), 0)

    def grad(x=xd, n=n, ldx=ldx, d=d, r=o["r"], p=p, splits=0, ws=ws, ws_bytes=None, g=o["g"]):
        return lib.aw_logreg_grad(P(x), n, ldx, d, P(r), p, splits, P(ws),
                                  ws.numel() if ws_bytes is None and ws is not None else (ws_bytes or 0), P(g), 0)

    refused = [fwd(p=0), fwd(p=33), fwd(d=0), fwd(ldx=d - 1), fwd(w=None), fwd(b=None), fwd(x=None), fwd(z=None),
               fwd(n=-1), fwd(r=None), fwd(cls=None), fwd(loss=None), fwd(gb=None), fwd(ws=None), fwd(ws_bytes=8),
               grad(p=0), grad(p=33), grad(d=0), grad(ldx=d - 1), grad(x=None), grad(r=None), grad(g=None),
               grad(splits=-1), grad(splits=nat.AW_LOGREG_MAX_SPLITS + 1), grad(ws=None), grad(ws_bytes=8),
               grad(n=-1)]
    torch.cuda.synchronize()
    assert all(st == nat.AW_ERR_ARG for st in refused), refused
    for v in outs.values():
        v.check(untouched=True)
    assert lib.aw_logreg_workspace(n, d, 33, 0) == nat.AW_ERR_ARG and lib.aw_logreg_workspace(n, 0, p, 0) == nat.AW_ERR_ARG
    with pytest.raises(nat.NativeError, match="p = 33"):
        K.logreg_forward(xd, torch.zeros((d, 33), device="cuda"), torch.zeros(33, device="cuda"))
    with pytest.raises(nat.NativeError, match="contiguous rows"):
        K.logreg_forward(xd.t(), wd, bd)


# ------------------------------------------------------------------------------------------------ the fit
FITS = [(300, 20, 0.1, 1e-6), (300, 20, 1.0, 1e-6), (517, 33, 1.0, 1e-6), (300, 20, 1.0, 1e-4)]


def _theta(fit, ci, k):
    return np.concatenate([fit["coef"][ci, k].cpu().numpy(), fit["intercept"][ci, k:k + 1].cpu().numpy()])


def _assert_fit(fit, ci, k, x, y, pos, C, tol, label):
    """The three conditions (logreg_refs.fit_conditions) on problem (ci, k) of a fit; returns the figures."""
    theta = _theta(fit, ci, k)
    assert bool(fit["converged"][ci, k]), f"{label}: not converged after {int(fit['n_iter'][ci, k])} iterations"
    t = (np.asarray(y) == pos).astype(np.int64)
    c = R.fit_conditions(theta, x, t, C, tol, R.grad_bound(theta, x, y, pos))
    print(f"{label}: {int(fit['n_iter'][ci, k])} iterations, max|grad F64| = {c['gmax']:.3g} (max over elements of "
          f"|grad| - eps = {c['grad_excess']:.3g}, tol {tol:g}), dist / bound = {c['dist'] / c['bound']:.3g}, "
          f"under = {c['under']:.4f}, agree = {c['agree']:.4f}")
    assert c["grad_ok"], f"{label}: the fp64 gradient exceeds tol + eps_g / N"
    assert c["dist_ok"], f"{label}: |theta - theta*| = {c['dist']:.3g} > {c['bound']:.3g}"
    assert c["pred_ok"] and c["under"] <= 0.02, f"{label}: predictions"
    eps_f = R.bounds(x, theta[:-1, None], theta[-1:], y, np.array([pos]))["eps_loss"][0] / len(x)
    assert abs(float(fit["objective"][ci, k]) - R.objective(theta, x, t, C)) <= eps_f
    return c


@pytest.mark.parametrize("n, d, C, tol", FITS)
def test_fit_meets_the_three_conditions(n, d, C, tol):
    from arcweld.retrieve import logreg_decision, logreg_fit, logreg_predict
    x, y = R.problem_data(1, n, d)
    fit = logreg_fit(torch.tensor(x), torch.tensor(y), C=C, standardize=False, tol=tol)
    assert tuple(fit["coef"].shape) == (1, 1, d) and tuple(fit["intercept"].shape) == (1, 1)
    assert bool((fit["mean"] == 0).all() and (fit["scale"] == 1).all()) and fit["C"].tolist() == [C]
    c = _assert_fit(fit, 0, 0, x, y, 1, C, tol, f"n={n} d={d} C={C} tol={tol}")
    # the decision values and the predictions on the training rows
    z = logreg_decision(fit, torch.tensor(x)).cpu().numpy()
    theta = _theta(fit, 0, 0)
    assert z.shape == (1, n, 1)
    assert (np.abs(z[0, :, 0] - (x.astype(np.float64) @ theta[:-1] + theta[-1]))
            <= R.eps_z(x, theta[:-1, None], theta[-1:])[:, 0]).all()
    pred = logreg_predict(fit, torch.tensor(x)).cpu().numpy()
    assert pred.shape == (1, n) and np.array_equal(pred[0], (z[0, :, 0] > 0).astype(np.int64))
    star = c["theta_star"]
    zs = x.astype(np.float64) @ star[:-1] + star[-1]
    safe = np.abs(zs) >= np.linalg.norm(np.c_[x, np.ones(n)], axis=1) * c["bound"] \
        + R.eps_z(x, theta[:-1, None], theta[-1:])[:, 0]
    assert np.array_equal(pred[0][safe], R.predict(zs[:, None], 2)[safe])


def _three_class(seed, n, d):
    x = gen.normal(seed, (n, d))
    w = gen.normal(seed + 1, (d, 3)).astype(np.float64)
    u = gen.uniform(seed + 2, (n, 3), 1e-6, 1 - 1e-6).astype(np.float64)
    return x, (x.astype(np.float64) @ w / np.sqrt(d) * 2 - np.log(-np.log(u))).argmax(1)


def test_three_classes_one_vs_rest():
    from arcweld.retrieve import logreg_decision, logreg_fit, logreg_predict
    n, d, C, tol = 240, 9, 1.0, 1e-6
    x, y = _three_class(81, n, d)
    assert set(y) == {0, 1, 2}
    fit = logreg_fit(torch.tensor(x), torch.tensor(y), C=C, standardize=False, tol=tol)
    assert tuple(fit["coef"].shape) == (1, 3, d) and fit["n_classes"] == 3
    for k in range(3):
        _assert_fit(fit, 0, k, x, y, k, C, tol, f"class {k}")
    z = logreg_decision(fit, torch.tensor(x)).cpu().numpy()
    pred = logreg_predict(fit, torch.tensor(x)).cpu().numpy()
    assert z.shape == (1, n, 3) and np.array_equal(pred[0], R.predict(z[0], 3))
    want = R.decision(fit["coef"].cpu().numpy(), fit["intercept"].cpu().numpy(), x)
    coef, icpt = fit["coef"].cpu().numpy(), fit["intercept"].cpu().numpy()
    assert (np.abs(z[0] - want[0]) <= R.eps_z(x, coef[0].T, icpt[0])).all() and (pred[0] == y).mean() > 0.5


def test_two_C_values_at_once_match_two_single_fits():
    from arcweld.retrieve import logreg_fit
    n, d, tol = 300, 20, 1e-6
    x, y = R.problem_data(1, n, d)
    xt, yt = torch.tensor(x), torch.tensor(y)
    both = logreg_fit(xt, yt, C=[0.1, 1.0], standardize=False, tol=tol)
    assert tuple(both["coef"].shape) == (2, 1, d) and both["C"].tolist() == [0.1, 1.0]
    for ci, C in enumerate((0.1, 1.0)):
        one = logreg_fit(xt, yt, C=C, standardize=False, tol=tol)
        cb = _assert_fit(both, ci, 0, x, y, 1, C, tol, f"both, C={C}")
        co = _assert_fit(one, 0, 0, x, y, 1, C, tol, f"alone, C={C}")
        assert np.linalg.norm(_theta(both, ci, 0) - _theta(one, 0, 0)) <= cb["bound"] + co["bound"]


def test_more_than_32_problems():
    from arcweld.retrieve import MAX_PROBLEMS, logreg_fit
    n, d, tol = 150, 6, 1e-5
    x, y = _three_class(91, n, d)
    Cs = [0.05 * 1.6 ** i for i in range(11)]
    assert 3 * len(Cs) > MAX_PROBLEMS == 32
    fit = logreg_fit(torch.tensor(x), torch.tensor(y), C=Cs, standardize=False, tol=tol)
    assert tuple(fit["coef"].shape) == (11, 3, d) and bool(fit["converged"].all())
    for ci in (0, 5, 10):                                     # problems 0..2 and 15..17 of the first group, 30, 31 and
        for k in range(3):                                    # the second group's only problem, 32
            _assert_fit(fit, ci, k, x, y, k, Cs[ci], tol, f"C={Cs[ci]:.3g} class {k}")


def test_standardized_fit_uses_the_probes_scaler():
    from arcweld.retrieve import logreg_fit
    n, d, C, tol = 300, 20, 1.0, 1e-6
    x, y = R.problem_data(1, n, d)
    x = (x * gen.uniform(5, (d,), 0.5, 30.0) + gen.normal(6, (d,), std=10.0)).astype(np.float32)
    x[:, 3] = 2.5                                             # a constant feature: scale 1
    fit = logreg_fit(torch.tensor(x), torch.tensor(y), C=C, tol=tol)
    mean, scale = KR.scaler(x)
    assert np.allclose(fit["mean"].cpu().numpy(), mean, rtol=1e-12, atol=1e-12)
    assert np.allclose(fit["scale"].cpu().numpy(), scale, rtol=1e-12) and scale[3] == 1.0
    _assert_fit(fit, 0, 0, KR.standardize(x, mean, scale), y, 1, C, tol, "standardised")


def test_argument_errors_name_the_argument():
    from arcweld.retrieve import latent_linear_probe, logreg_decision, logreg_fit
    x, y = torch.zeros(6, 3), torch.tensor([0, 1, 0, 1, 0, 1])
    for kw, name in ((dict(C=0.0), "C"), (dict(C=[]), "C"), (dict(C=[1.0, -1.0]), "C"), (dict(C="1"), "C"),
                     (dict(standardize=1), "standardize"), (dict(tol=0.0), "tol"), (dict(max_iter=0), "max_iter"),
                     (dict(max_iter=1.5), "max_iter"), (dict(n_classes=1), "n_classes")):
        with pytest.raises(ValueError, match=f"^{name}:"):
            logreg_fit(x, y, **kw)
    for bad_y in (y.float(), y[:5], torch.tensor([0, 1, 0, 1, 0, 2])):
        with pytest.raises(ValueError, match="^labels:"):
            logreg_fit(x, bad_y, n_classes=2)
    with pytest.raises(ValueError, match="^labels:"):
        logreg_fit(x, torch.tensor([0, 1, 0, 1, 0, -1]))
    with pytest.raises(ValueError, match="^features:"):
        logreg_fit(torch.zeros(6), y)
    with pytest.raises(ValueError, match="^features:"):
        logreg_fit(torch.zeros(0, 3), y[:0])
    with pytest.raises(ValueError, match="^fit:"):
        logreg_decision({}, x)
    sp = [(torch.zeros(4, 400, 2), torch.zeros(4, dtype=torch.long))] * 3
    for kw, name in ((dict(dataset="x"), "dataset"), (dict(dataset="latent_vq_vae"), "vqvae"), (dict(C=()), "C"),
                     (dict(max_samples=0), "max_samples"), (dict(tol=-1.0), "tol")):
        with pytest.raises(ValueError, match=f"^{name}:"):
            latent_linear_probe(sp, 2, **{"dataset": "asimow", **kw})
    with pytest.raises(ValueError, match="^splits:"):
        latent_linear_probe(sp[:2], 2, dataset="asimow")
    with pytest.raises(ValueError, match="^n_cycles:"):
        latent_linear_probe(sp, 0, dataset="asimow")


# ------------------------------------------------------------------------------------------------ probe and script
KW = dict(hidden_dim=64, num_embeddings=32, embedding_dim=16, n_resblocks=2, patch_size=25)
N_CYCLES, SIZES = 2, (40, 9, 7)
METRICS = {"acc", "acc_good", "acc_bad", "f1"}


@pytest.fixture(scope="module")
def vqvae():
    from model.vq_vae_patch_embedd import VQVAEPatch
    v = VQVAEPatch(input_dim=2, learning_rate=1e-3, dropout_p=0.0, batch_norm=False, **KW)
    v.load_state_dict({k: torch.tensor(a) for k, a in ov.det_state_dict(ov.VQVAEConfig(**KW), 2501).items()})
    return v.cuda().eval()


@pytest.fixture(scope="module")
def splits():
    return [(torch.tensor(gen.windows(300 + i, n * N_CYCLES).reshape(n, N_CYCLES * 200, 2), device="cuda"),
             torch.tensor(gen.randint(310 + i, (n,), 0, 2), device="cuda")) for i, n in enumerate(SIZES)]


@pytest.fixture
def fp32():
    from arcweld.precision import operands
    with operands(torch.float32):
        yield


@pytest.mark.parametrize("dataset", ["latent_vq_vae", "asimow"])
def test_probe_metrics_and_selection(vqvae, splits, fp32, dataset):
    from arcweld.data import latent_vectors
    from arcweld.retrieve import latent_linear_probe
    Cs, tol = (1.0, 0.01), 1e-5
    res = latent_linear_probe(splits, N_CYCLES, C=Cs, dataset=dataset, vqvae=vqvae, tol=tol)
    assert set(res) == {"val", "test", "per_C", "C_selected", "fit", "converged", "n_iter"}
    assert res["converged"] == [True, True] and len(res["n_iter"]) == 2
    feats = [(latent_vectors(vqvae, x, N_CYCLES) if dataset == "latent_vq_vae" else x).reshape(len(x), -1).cpu().numpy()
             for x, _ in splits]
    labels = [y.cpu().numpy() for _, y in splits]
    fit = res["fit"]
    mean, scale = KR.scaler(feats[0])
    assert np.allclose(fit["mean"].cpu().numpy(), mean, rtol=1e-9, atol=1e-9)
    zx = KR.standardize(feats[0], mean, scale)
    for ci, C in enumerate(Cs):                               # condition 1 on the train split, per C
        theta = _theta(fit, ci, 0)
        g = R.gradient(theta, zx, labels[0], C)
        assert (np.abs(g) <= tol + R.grad_bound(theta, zx, labels[0], 1)).all(), (dataset, C)
    coef, icpt = fit["coef"].cpu().numpy(), fit["intercept"].cpu().numpy()
    best, wants = None, {}
    for ci in sorted(range(len(Cs)), key=lambda i: Cs[i]):
        entry = res["per_C"][ci]
        assert entry["C"] == Cs[ci] and set(entry) == {"C", "val", "test"}
        for qi, name in ((1, "val"), (2, "test")):
            zq = KR.standardize(feats[qi], mean, scale)
            want = R.decision(coef, icpt, zq)[ci, :, 0]
            wants[ci, name] = (want, R.eps_z(zq, coef[ci].T, icpt[ci])[:, 0])
            sure = np.abs(want) > 2 * wants[ci, name][1]
            assert set(entry[name]) == METRICS
            if sure.all():
                for m, v in KR.metrics((want > 0).astype(np.int64), labels[qi]).items():
                    assert abs(entry[name][m] - v) <= 1e-6, (dataset, C, name, m)
        if best is None or entry["val"]["f1"] > res["per_C"][best]["val"]["f1"]:
            best = ci
    assert res["C_selected"] == Cs[best]
    for qi, name in ((1, "val"), (2, "test")):
        r = res[name]
        assert set(r) == METRICS | {"pred", "decision"}
        pred, dec = r["pred"].cpu().numpy(), r["decision"].cpu().numpy()
        assert dec.shape == (SIZES[qi], 1) and np.array_equal(pred, (dec[:, 0] > 0).astype(np.int64))
        assert (np.abs(dec[:, 0] - wants[best, name][0]) <= wants[best, name][1]).all(), (dataset, name)
        for m, v in KR.metrics(pred, labels[qi]).items():
            assert abs(r[m] - v) <= 1e-6 and r[m] == res["per_C"][best][name][m]


def test_probe_subsamples_the_train_split(splits, fp32):
    from arcweld.retrieve import latent_linear_probe, logreg_fit, stratified_subsample
    y = splits[0][1].cpu().numpy()
    rows = R.stratified_subsample(y, 21, seed=4)
    assert np.array_equal(stratified_subsample(splits[0][1], 21, seed=4), rows) and len(rows) == 21
    assert np.array_equal(stratified_subsample(y, 40), np.arange(40))
    res = latent_linear_probe(splits, N_CYCLES, C=(1.0,), dataset="asimow", max_samples=21, seed=4)
    sub = torch.as_tensor(rows, device="cuda")
    direct = logreg_fit(splits[0][0][sub].reshape(21, -1), splits[0][1][sub], C=1.0)
    assert torch.equal(res["fit"]["coef"], direct["coef"]) and torch.equal(res["fit"]["mean"], direct["mean"])


def test_script_linear_protocol(vqvae, fp32, tmp_path):
    import probe_latent_space as pls
    ckpt, out, model = tmp_path / "v.ckpt", tmp_path / "probe.json", tmp_path / "model.npz"
    vqvae.save_checkpoint(str(ckpt))
    common = ["--vqvae-model", str(ckpt), "--n-cycles", str(N_CYCLES), "--n-train", "24", "--n-val", "5", "--n-test",
              "6", "--seed", "3", "--out", str(out)]
    pls.main(pls.parser().parse_args(common + ["--protocol", "linear", "--C", "0.1", "1.0", "10", "--tol", "1e-5",
                                               "--max-iter", "500", "--model-out", str(model)]))
    summary = json.loads(out.read_text())
    assert set(summary) == {"val", "test", "per_C", "C_selected", "protocol", "dataset", "standardize", "n_cycles",
                            "converged", "n_iter"}
    assert summary["protocol"] == "linear" and summary["dataset"] == "latent_vq_vae" and summary["standardize"] is True
    assert summary["C_selected"] in (0.1, 1.0, 10.0) and summary["converged"] == [True] * 3
    assert [e["C"] for e in summary["per_C"]] == [0.1, 1.0, 10.0]
    for name in ("val", "test"):
        assert set(summary[name]) == METRICS and all(0.0 <= v <= 1.0 for v in summary[name].values())
        assert summary[name] == summary["per_C"][[0.1, 1.0, 10.0].index(summary["C_selected"])][name]
    with np.load(model, allow_pickle=False) as f:
        assert set(f.files) == {"coef", "intercept", "mean", "scale", "C"}
        D = f["mean"].shape[0]
        assert f["coef"].shape == (3, 1, D) and f["intercept"].shape == (3, 1) and f["scale"].shape == (D,)
        assert f["C"].tolist() == [0.1, 1.0, 10.0] and np.isfinite(f["coef"]).all()
    with pytest.raises(SystemExit, match="neighbours-out"):
        pls.main(pls.parser().parse_args(common + ["--protocol", "linear", "--neighbours-out",
                                                   str(tmp_path / "nb.npz")]))
    # the k-NN protocol is the default and keeps its key set
    assert pls.parser().parse_args(common).protocol == "knn"
    pls.main(pls.parser().parse_args(common + ["--k", "3"]))
    assert set(json.loads(out.read_text())) == {"val", "test", "k", "weights", "dataset", "standardize", "n_cycles"}
    with pytest.raises(SystemExit, match="model-out"):
        pls.main(pls.parser().parse_args(common + ["--model-out", str(model)]))
