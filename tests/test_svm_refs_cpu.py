"""CPU checks of tests/svm_refs.py -- the yardstick of tests/test_svm_gpu.py -- and of every argument error of the
RBF-SVM probe's host side, raised on CPU tensors before any device is looked for.

The reference SMO against scikit-learn's SVC (libsvm) on the same f64 kernel: both stop at m - M <= tol, so by
f(alpha) - f* <= gap sum |alpha - alpha*| <= tol C n each objective is within tol C n of the optimum and the two
within 2 tol C n of each other; the decision values of two solutions that stop on opposite sides of the optimum are
compared at 2 tol (measured: 0.9 tol at these shapes), the predictions must be identical.  libsvm breaks ties towards
the last row and shrinks, so iteration counts differ slightly (144 / 140, 447 / 430, 1190 / 1189 here).

The Gram bound against an f32 evaluation of the kernel's expression in natural and in shuffled order, and the band
condition of the decision test on the data the GPU tests use: at most 2 % of the query rows within 3 e of 0, for the
reference alone."""
import numpy as np
import pytest
import torch

import svm_refs as R
from oracle import gen


# ------------------------------------------------------------------------------------------------ the reference solver
@pytest.mark.parametrize("n, D, C", [(300, 20, 0.1), (300, 20, 10.0), (2000, 64, 1.0)])
def test_reference_smo_against_libsvm(n, D, C):
    svm = pytest.importorskip("sklearn.svm")
    x, lab = R.blobs(5, n, D, sep=3.0)
    gamma, tol = float(np.float32(R.rbf_gamma(x))), 1e-3
    k = R.gram64(x, x, gamma)
    y = 2 * lab - 1
    f = R.fit(k, y, C, tol)
    m = svm.SVC(kernel="rbf", gamma=gamma, C=C, tol=tol).fit(x.astype(np.float64), lab)
    alpha = np.zeros(n)
    alpha[m.support_] = np.abs(m.dual_coef_[0])
    obj_sk = R.objective(alpha, R.grad64(k, y, alpha), y)
    dec, dec_sk = R.decision(k, f["coef"], f["rho"]), m.decision_function(x.astype(np.float64))
    print(f"n={n} C={C}: iterations {f['n_iter']} / {int(m.n_iter_[0])}, objective {f['objective']:.9f} / {obj_sk:.9f}, "
          f"max decision difference {np.abs(dec - dec_sk).max():.2e}")
    assert f["gap"] <= tol and R.kkt_gap(k, y, C, f["alpha"]) <= tol + 1e-9
    assert abs(f["objective"] - obj_sk) <= 2 * tol * C * n
    assert np.abs(dec - dec_sk).max() <= 2 * tol
    assert np.array_equal(dec > 0, dec_sk > 0)
    assert abs(f["n_iter"] - int(m.n_iter_[0])) <= 0.1 * f["n_iter"]


def test_reference_smo_resumes_and_masks():
    x, lab = R.blobs(7, 120, 6, sep=2.0)
    k = R.gram64(x, x, 0.2)
    y = 2 * lab - 1
    y[::5] = 0
    whole = R.smo(k, y, 1.0)
    a, g, it, _ = R.smo(k, y, 1.0, max_iter=11)
    rest = R.smo(k, y, 1.0, alpha=a, grad=g)
    assert it == 11 and np.array_equal(whole[0], rest[0]) and whole[2] == 11 + rest[2]
    assert (whole[0][::5] == 0).all() and (whole[1][::5] == -1).all()
    sub = R.smo(k[y != 0][:, y != 0], y[y != 0], 1.0)           # masking equals leaving the rows out
    assert np.array_equal(sub[0], whole[0][y != 0]) and sub[2] == whole[2]
    assert R.gap_of(-np.ones(3), np.array([1, 1, 1]), np.zeros(3), 1.0)[0] == -np.inf


def test_rho_and_vote_rules():
    y, C = np.array([1, 1, -1, -1, 0]), 1.0
    G = np.array([-0.5, -0.25, 0.75, 0.5, 9.0])
    assert R.rho(np.array([0.5, 0.0, 0.5, 0.0, 0.0]), G, y, C) == (-0.5 - 0.75) / 2        # the free rows' mean of y G
    # nothing free: ub from (upper, y = -1) and (lower, y = +1), lb from the other two
    assert R.rho(np.array([1.0, 0.0, 1.0, 0.0, 0.0]), G, y, C) == (min(-0.75, -0.25) + max(-0.5, -0.5)) / 2
    assert R.rho(np.zeros(5), G, np.array([1, 1, 1, 0, 0]), C) == -0.5                      # one class: the one bound
    pairs = R.pairs_of(3)
    dec = np.array([[1.0, 1.0, 1.0], [-1.0, 1.0, -1.0], [1.0, -1.0, 1.0], [-1.0, -1.0, 1.0]])
    assert R.vote(dec, pairs, 3).tolist() == [0, 0, 0, 1]      # rows 1 and 2: a three-way tie goes to the lowest class
    assert R.pairs_of(2) == [(1, 0)] and R.pair_labels([0, 1, 2], pairs).tolist() == [[1, -1, 0], [1, 0, -1], [0, 1, -1]]


# ------------------------------------------------------------------------------------------------ the Gram bound
@pytest.mark.parametrize("na, nb, d, gamma", [(40, 50, 1, 1.0), (40, 50, 33, 0.03), (30, 20, 513, 1.0 / 513),
                                              (20, 20, 69, 2.0)])
def test_gram_bound_holds_for_an_f32_evaluation(na, nb, d, gamma):
    a, b = gen.normal(11, (na, d)), gen.normal(12, (nb, d), 1.0, 0.25)
    want, bound = R.gram64(a, b, gamma), R.eps_gram(a, b, gamma)
    for order in (None, np.argsort(gen.uniform(13, (d,)), kind="stable")):
        err = np.abs(R.gram32(a, b, gamma, order).astype(np.float64) - want)
        assert (err <= bound).all(), float((err / bound).max())
    assert (bound <= 1e-3).all()                                # a bound, not a licence


def test_rbf_gamma_is_sklearns_scale():
    x = gen.normal(3, (50, 7), 2.5, 1.0)
    assert R.rbf_gamma(x) == 1.0 / (7 * x.astype(np.float64).var())
    assert R.rbf_gamma(np.ones((4, 3), np.float32)) == 1.0
    from arcweld.retrieve import rbf_gamma
    assert abs(rbf_gamma(torch.tensor(x)) - R.rbf_gamma(x)) <= 1e-12 * R.rbf_gamma(x)
    assert rbf_gamma(torch.ones(4, 3)) == 1.0
    assert rbf_gamma(torch.tensor(x).reshape(50, 7, 1)) == rbf_gamma(torch.tensor(x))


# ------------------------------------------------------------------------------------------------ the decision band
def _inside(x, y, q, C, tol=1e-3):
    gamma = float(np.float32(R.rbf_gamma(x)))
    k, kq = R.gram64(x, x, gamma), R.gram64(q, x, gamma)
    f1, f2 = R.fit(k, y, C, tol), R.fit(k, y, C, tol / 100)
    d1, d2 = R.decision(kq, f1["coef"], f1["rho"]), R.decision(kq, f2["coef"], f2["rho"])
    e = np.abs(d1 - d2).max()
    return float((np.abs(d2) <= 3 * e).mean()), float(e)


def test_the_gpu_tests_data_meets_the_band_condition():
    x, lab = R.blobs(1234, 1000, 20, sep=3.0)                  # tests/test_svm_gpu.py fit_data
    for C in (0.1, 10.0):
        inside, e = _inside(x[:600], 2 * lab[:600] - 1, x[600:], C)
        assert inside <= 0.02 and e <= 5e-3, (C, inside, e)
    x, lab = R.blobs(321, 450, 12, sep=4.0, n_classes=3)       # its three-class test
    q, _ = R.blobs(322, 200, 12, sep=4.0, n_classes=3)
    sure = 1.0
    for yp in R.pair_labels(lab, R.pairs_of(3)):
        inside, e = _inside(x, yp, q, 1.0)
        sure -= inside
    assert sure > 0.9


# ------------------------------------------------------------------------------------------------ argument errors
X, Y = torch.zeros(8, 3), torch.tensor([0, 1] * 4)


@pytest.mark.parametrize("args, kw, name", [
    ((torch.zeros(8), Y), {}, "features"),
    ((X.numpy(), Y), {}, "features"),
    ((torch.zeros(0, 3), Y[:0]), {}, "features"),
    ((X, Y[:5]), {}, "labels"),
    ((X, Y.float()), {}, "labels"),
    ((X, Y + 3), dict(n_classes=2), "labels"),
    ((X, Y), dict(C=0.0), "C"),
    ((X, Y), dict(C=[]), "C"),
    ((X, Y), dict(C=float("inf")), "C"),
    ((X, Y), dict(gamma="auto"), "gamma"),
    ((X, Y), dict(gamma=0.0), "gamma"),
    ((X, Y), dict(gamma=True), "gamma"),
    ((X, Y), dict(standardize=1), "standardize"),
    ((X, Y), dict(tol=0.0), "tol"),
    ((X, Y), dict(max_iter=0), "max_iter"),
    ((X, Y), dict(max_iter=1.5), "max_iter"),
    ((X, Y), dict(n_classes=1), "n_classes"),
    ((torch.zeros(20481, 1), torch.zeros(20481, dtype=torch.long)), {}, "max_samples"),
])
def test_svm_fit_argument_errors(args, kw, name):
    from arcweld.retrieve import svm_fit
    with pytest.raises(ValueError, match=name):
        svm_fit(*args, **kw)


def test_svm_decision_argument_errors():
    from arcweld.retrieve import rbf_gamma, svm_decision, svm_predict
    with pytest.raises(ValueError, match="fit"):
        svm_decision({"dual_coef": X}, X)
    with pytest.raises(ValueError, match="fit"):
        svm_predict(None, X)
    fit = {"dual_coef": torch.zeros(1, 1, 8), "rho": torch.zeros(1, 1), "support": torch.zeros(0, dtype=torch.long),
           "support_vectors": torch.zeros(0, 3), "gamma": 1.0, "mean": torch.zeros(3), "scale": torch.ones(3),
           "pairs": [(1, 0)], "n_classes": 2, "standardize": False}
    with pytest.raises(ValueError, match="queries"):
        svm_decision(fit, torch.zeros(4, 5))
    with pytest.raises(ValueError, match="queries"):
        svm_decision(fit, torch.zeros(4))
    with pytest.raises(ValueError, match="features"):
        rbf_gamma(torch.zeros(0, 3))


def _splits(n_cycles=2, n=(60, 3, 3)):
    return [(torch.zeros(m, n_cycles * 200, 2), torch.arange(m) % 2) for m in n]


@pytest.mark.parametrize("kw, name", [
    (dict(dataset="mnist"), "dataset"),
    (dict(dataset="latent_vq_vae", vqvae=None), "vqvae"),
    (dict(n_cycles=0), "n_cycles"),
    (dict(C=(1.0, -1.0)), "C"),
    (dict(gamma="auto"), "gamma"),
    (dict(standardize=None), "standardize"),
    (dict(tol=-1.0), "tol"),
    (dict(max_iter=0), "max_iter"),
    (dict(max_samples=0), "max_samples"),
    (dict(max_samples=20481), "max_samples"),
    (dict(splits=_splits()[:2]), "splits"),
    (dict(splits=_splits(n_cycles=3)), "splits"),
    (dict(splits=[(x, y.float()) for x, y in _splits()]), "splits"),
    (dict(splits=_splits(n=(0, 3, 3))), "splits"),
    (dict(splits=_splits(n=(49, 3, 3))), "C = inf"),                              # fewer than 50 rows
    (dict(splits=[(x, torch.arange(len(y)) % 13) for x, y in _splits()]), "C = inf"),   # 60 // 13 < 5 per class
])
def test_latent_svm_probe_argument_errors(kw, name):
    from arcweld.retrieve import latent_svm_probe
    args = dict(splits=_splits(), n_cycles=2, dataset="asimow")
    args.update(kw)
    with pytest.raises(ValueError, match=name):
        latent_svm_probe(**args)


def test_script_refusals_and_per_protocol_defaults(tmp_path):
    import probe_latent_space as pls
    base = ["--dataset", "asimow", "--out", str(tmp_path / "o.json")]
    hp = pls.parser().parse_args(base)
    assert hp.C is None and hp.tol is None and hp.max_iter is None and hp.gamma == "scale" and not hp.standardize
    for proto, want in (("linear", ([1.0], 1e-4, 1000)), ("svm", ([0.1], 1e-3, 20000))):
        assert pls.resolve_fit_args(pls.parser().parse_args(base + ["--protocol", proto])) == want
    hp = pls.parser().parse_args(base + ["--protocol", "svm", "--C", "2", "3", "--tol", "0.01", "--max-iter", "7",
                                         "--gamma", "0.25"])
    assert pls.resolve_fit_args(hp) == ([2.0, 3.0], 0.01, 7) and hp.gamma == 0.25
    with pytest.raises(SystemExit):
        pls.parser().parse_args(base + ["--gamma", "auto"])
    for extra, what in ((["--protocol", "svm", "--neighbours-out", "nb.npz"], "neighbours-out"),
                        (["--protocol", "svm", "--loo"], "loo"),
                        (["--protocol", "svm", "--no-standardize"], "no-standardize"),
                        (["--protocol", "svm", "--gamma", "-1"], "gamma"),
                        (["--protocol", "svm", "--C", "0"], "--C"),
                        (["--protocol", "svm", "--tol", "0"], "--tol"),
                        (["--protocol", "svm", "--max-iter", "0"], "--max-iter"),
                        (["--protocol", "linear", "--standardize"], "--standardize"),
                        (["--protocol", "linear", "--gamma", "0.5"], "--gamma"),
                        (["--protocol", "linear", "--C", "-1"], "--C"),
                        (["--standardize"], "--standardize"),
                        (["--gamma", "0.5"], "--gamma"),
                        (["--model-out", "m.npz"], "model-out")):
        with pytest.raises(SystemExit, match=what):
            pls.main(pls.parser().parse_args(base + extra))
    assert not (tmp_path / "o.json").exists()


def test_abi_constants_match_the_header():
    import os
    import re
    from conftest import REPO
    from arcweld import _native, retrieve
    src = open(os.path.join(REPO, "include", "arcweld_amd.h")).read()
    assert int(re.search(r"#define AW_SVM_MAX_N (\d+)", src).group(1)) == _native.AW_SVM_MAX_N == 20480
    assert int(re.search(r"#define AW_SVM_MAX_P (\d+)", src).group(1)) == _native.AW_SVM_MAX_P == 32
    assert retrieve.MAX_SVM_ROWS == 20480 and retrieve.MAX_PROBLEMS == _native.AW_SVM_MAX_P
    lib = _native.load()
    import ctypes
    v = [ctypes.c_int(0) for _ in range(4)]
    assert lib.aw_svm_describe(*[ctypes.byref(c) for c in v]) == 0
    assert v[0].value * v[1].value == v[2].value == 20480 and v[3].value == 32
    assert _native.SIGNATURES["aw_rbf_gram"][7] is ctypes.c_float and _native.SIGNATURES["aw_svm_smo"][6] is ctypes.c_double
