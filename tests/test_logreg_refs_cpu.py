"""tests/logreg_refs.py against itself and against scikit-learn, on the CPU: the derived bounds hold for an f32
evaluation in two summation orders, the Newton solver reaches a zero gradient, the objective is scikit-learn's, and the
three fit conditions the GPU test asks of arcweld.retrieve.logreg_fit hold for an f32 evaluation minimised by scipy's
L-BFGS-B at the same tolerances."""
import numpy as np
import pytest

import logreg_refs as R
from oracle import gen

FITS = [(300, 20, 0.1, 1e-6), (300, 20, 1.0, 1e-6), (517, 33, 1.0, 1e-6), (300, 20, 1.0, 1e-4)]


def _labelled(seed, n, d, p, scale=1.0):
    x = gen.normal(seed, (n, d))
    w = gen.normal(seed + 1, (d, p), std=scale / np.sqrt(d))
    b = gen.normal(seed + 2, (p,), std=0.5)
    y = gen.randint(seed + 3, (n,), -1, 4)                  # class ids -1 (no part) .. 3
    cls = gen.randint(seed + 4, (p,), 0, 5)                 # class 4 is absent from y
    return x, w, b, y, cls


@pytest.mark.parametrize("scale", [1.0, 20.0])
@pytest.mark.parametrize("shuffled", [False, True])
def test_bounds_hold_for_an_f32_evaluation(scale, shuffled):
    n, d, p = 131, 37, 5
    x, w, b, y, cls = _labelled(11, n, d, p, scale)
    order = rows = None
    if shuffled:
        order = np.random.RandomState(0).permutation(d)
        rows = np.random.RandomState(1).permutation(n)
    z, r, loss, gb, g = R.eval32(x, w, b, y, cls, order, rows)
    bd = R.bounds(x, w, b, y, cls)
    for name, got in (("z", z), ("r", r), ("loss", loss), ("gb", gb), ("g", g)):
        err, eps = np.abs(got.astype(np.float64) - bd[name]), bd["eps_" + name]
        print(f"{name}: max err / eps = {(err / np.maximum(eps, 1e-300)).max():.3g}")
        assert (err <= eps).all(), name
    assert (r[y < 0] == 0).all() and (bd["eps_r"][y < 0] == 0).all()
    if scale > 1:
        assert np.abs(bd["z"]).max() > 30                   # both tails of softplus and sigma


def test_softplus_and_sigmoid_are_stable_in_both_tails():
    z = np.array([-800.0, -60.0, -1e-20, 0.0, 1e-20, 60.0, 800.0])
    with np.errstate(over="raise", invalid="raise", divide="raise"):      # exp(-800) underflows to 0: intended
        sp, sg = R.softplus(z), R.sigmoid(z)
    assert np.isfinite(sp).all() and sp[0] == 0 and sp[-1] == 800 and sp[3] == np.log(2.0)
    assert sg[0] == 0 and sg[-1] == 1 and sg[3] == 0.5 and (np.diff(sg) >= 0).all()


@pytest.mark.parametrize("n, d, C", [(300, 20, 0.1), (517, 33, 1.0), (60, 5, 100.0)])
def test_newton_reaches_a_zero_gradient(n, d, C):
    x, y = R.problem_data(1, n, d)
    theta = R.newton(x, y, C)
    assert np.abs(R.gradient(theta, x, y, C)).max() <= 1e-12
    # the gradient and the Hessian are the derivatives of the objective (central differences)
    h = 1e-5
    for j in (0, d // 2, d):
        e = np.zeros(d + 1)
        e[j] = h
        num = (R.objective(theta + e, x, y, C) - R.objective(theta - e, x, y, C)) / (2 * h)
        assert abs(num - R.gradient(theta, x, y, C)[j]) <= 1e-9
        numh = (R.gradient(theta + e, x, y, C) - R.gradient(theta - e, x, y, C)) / (2 * h)
        assert np.abs(numh - R.hessian(theta, x, C)[:, j]).max() <= 1e-8


@pytest.mark.parametrize("C", [0.1, 1.0])
def test_the_objective_is_scikit_learns(C):
    linear_model = pytest.importorskip("sklearn.linear_model")
    x, y = R.problem_data(1, 300, 20)
    x = x.astype(np.float64)
    xs = (x - x.mean(0)) / x.std(0)
    m = linear_model.LogisticRegression(C=C, tol=1e-10, max_iter=10000).fit(xs, y)
    theirs = np.concatenate([m.coef_[0], m.intercept_])
    f_sk, f_nt = R.objective(theirs, xs, y, C), R.objective(R.newton(xs, y, C), xs, y, C)
    print(f"C={C}: F(sklearn) = {f_sk:.15g}, F(newton) = {f_nt:.15g}")
    assert abs(f_sk - f_nt) <= 1e-9 * abs(f_nt)
    assert f_nt <= f_sk + 1e-9 * abs(f_nt)


@pytest.mark.parametrize("n, d, C, tol", FITS)
def test_fit_conditions_hold_for_an_f32_lbfgs(n, d, C, tol):
    optimize = pytest.importorskip("scipy.optimize")
    x, y = R.problem_data(1, n, d)
    x32 = x.astype(np.float32)
    t32 = y.astype(np.float32)

    def fun(theta):
        th = theta.astype(np.float32)
        z = (x32 @ th[:-1] + th[-1]).astype(np.float32)
        e = np.exp(-np.abs(z)).astype(np.float32)
        sig = np.where(z >= 0, np.float32(1), e) / (np.float32(1) + e)
        sp = np.maximum(z, np.float32(0)) + np.log1p(e)
        r = (sig - t32).astype(np.float32)
        th64 = th.astype(np.float64)
        f = (sp.astype(np.float64) - y * z.astype(np.float64)).sum() / n + (th64[:-1] ** 2).sum() / (2 * C * n)
        g = np.concatenate([(x32.T @ r).astype(np.float64), [r.astype(np.float64).sum()]]) / n
        g[:-1] += th64[:-1] / (C * n)
        return f, g

    res = optimize.minimize(fun, np.zeros(d + 1), jac=True, method="L-BFGS-B",
                            options={"gtol": tol, "ftol": 0.0, "maxiter": 1000, "maxcor": 10})
    theta = res.x.astype(np.float32).astype(np.float64)
    c = R.fit_conditions(theta, x, y, C, tol, R.grad_bound(theta, x, y, 1))
    print(f"n={n} d={d} C={C} tol={tol}: max|grad F64| = {c['gmax']:.3g}, dist / bound = {c['dist'] / c['bound']:.3g}, "
          f"under = {c['under']:.4f}, agree = {c['agree']:.4f}")
    assert c["grad_ok"] and c["dist_ok"] and c["pred_ok"] and c["under"] <= 0.02


def test_stratified_subsample():
    y = np.array([0] * 70 + [1] * 25 + [2] * 5)
    y = y[np.random.RandomState(3).permutation(len(y))]
    rows = R.stratified_subsample(y, 20, seed=0)
    assert len(rows) == 20 and len(set(rows)) == 20 and (np.diff(rows) > 0).all()
    assert [int((y[rows] == c).sum()) for c in range(3)] == [14, 5, 1]
    assert np.array_equal(rows, R.stratified_subsample(y, 20, seed=0))
    assert not np.array_equal(rows, R.stratified_subsample(y, 20, seed=1))
    assert np.array_equal(R.stratified_subsample(y, 100), np.arange(100))
    odd = R.stratified_subsample(np.array([0, 0, 0, 1, 1, 1, 2]), 3)        # 9/7, 9/7, 3/7: one each
    assert len(odd) == 3 and sorted(np.array([0, 0, 0, 1, 1, 1, 2])[odd]) == [0, 1, 2]
