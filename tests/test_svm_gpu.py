"""aw_rbf_gram / aw_svm_smo (csrc/svm.hip), the fit built on them (arcweld.retrieve.svm_fit / svm_decision /
svm_predict) and the RBF-SVM probe (latent_svm_probe, probe_latent_space.py --protocol svm) against the fp64
restatements of tests/svm_refs.py.  Sizes come from the describe calls: below, at and above a tile, a dim chunk, the
solver's thread count and the sizes at which it switches to longer register arrays.  Buffers are placed as in
tests/test_knn_gpu.py: inputs inside NaN-filled allocations with NaN row padding and odd base offsets, outputs between
canaries (the Gram matrix's row padding included).

Gram: every element within svm_refs.eps_gram (derived there, checked against an f32 evaluation on the CPU in
tests/test_svm_refs_cpu.py); integer features with a power-of-two gamma, whose arguments are exact, within 2 ulp of
expf; bit-symmetry, run-to-run bits, overflow to 0.

Solver: the conditions of the issue on the returned state, with G64 = Q alpha - e recomputed in f64 from the f32 matrix
the kernel was given, drift = 8 n_iter 2^-53 C max|k|:
  (a) 0 <= alpha <= C exactly, alpha = 0 where y = 0;       (b) |sum y alpha| <= 4 n_iter 2^-53 C;
  (c) the recomputed gap <= tol + drift;                      (d) |grad - G64| <= drift;
  (e) the objective within tol C n_c of the reference SMO's at the same tol (n_c rows take part).
The drift counts the roundings of an update's terms, each of size <= C max|k|.  The running gradient's own rounding,
2^-53 |G| per update with |G| about 1, is not among them: it lies inside the drift only while C max|k| is not far
below |G|.  The cases whose C is left to this file therefore keep C >= 0.25; at C = 0.01 (n = 700, 203 iterations)
the fp64 reference solver itself is 1.11 drifts away from its own recomputed gradient, and the kernel, which stopped
at the same iteration with the same drift (1.108), with it.
Decision values have no derived bound (the dual need not be strongly convex): with e = max |dec_ref(tol) -
dec_ref(tol / 100)| measured on the reference alone, the device's decisions must lie within 3 e of dec_ref(tol / 100),
the predictions must agree wherever |dec_ref(tol / 100)| > 3 e, and at most 2 % of the query rows may lie inside that
band (tests/test_svm_refs_cpu.py checks that the reference alone meets it on this data)."""
import itertools
import json

import numpy as np
import pytest
import torch

import knn_refs as KR
import svm_refs as R
from oracle import gen
from oracle import vqvae as ov

pytestmark = pytest.mark.gpu

PAD = 64
CANARY = -1234.5
U53 = 2.0 ** -53


@pytest.fixture(scope="module")
def tiles():
    from arcweld import kernels as K
    ta, tb, cd = K.rbf_gram_describe()
    assert ta >= 4 and tb >= 4 and cd >= 4
    return ta, tb, cd


@pytest.fixture(scope="module")
def smo_dims():
    from arcweld import kernels as K
    T, rpt, max_n, max_p = K.svm_describe()
    assert max_n == 20480 and max_p == 32 and T * rpt == max_n
    return T, rpt, max_n, max_p


def _place(a, pad=0, off=0):
    """(n, D) array on the device inside a NaN-filled buffer: rows D + pad floats apart, `off` floats in."""
    a = np.ascontiguousarray(a, dtype=np.float32)
    n, D = a.shape
    ld = D + pad
    buf = torch.full((off + n * ld + PAD,), float("nan"), device="cuda")
    view = buf.as_strided((n, D), (ld, 1), off)
    if n:
        view.copy_(torch.as_tensor(a))
    return view


class _Out:
    """An output between canaries; rows `pad` elements apart, `off` elements after the front canary."""

    def __init__(self, shape, dtype, pad=0, off=0):
        shape = tuple(shape)
        rows, cols = (shape if len(shape) == 2 else (1, int(np.prod(shape))))
        self.ld = cols + pad
        self.canary = CANARY if dtype.is_floating_point else int(CANARY)
        self.buf = torch.full((2 * PAD + off + rows * self.ld,), self.canary, dtype=dtype, device="cuda")
        self.view = self.buf.as_strided((rows, cols), (self.ld, 1), PAD + off)
        self.mask = torch.ones_like(self.buf, dtype=torch.bool)
        self.mask.as_strided((rows, cols), (self.ld, 1), PAD + off).fill_(False)
        if len(shape) != 2:
            self.view = self.view[0]

    def set(self, a):
        self.view.copy_(torch.as_tensor(np.asarray(a)).to(self.view.dtype))
        return self

    def check(self, untouched=False):
        assert bool((self.buf[self.mask] == self.canary).all()), "a canary or a row padding was written"
        if untouched:
            assert bool((self.buf == self.canary).all()), "an output was written by a refused call"
        return self.view.cpu().numpy()


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view({4: np.uint32, 8: np.uint64}[a.dtype.itemsize])


def _gram(a, b, gamma, pads=(0, 0, 0), offs=(0, 0, 0)):
    from arcweld import kernels as K
    ad, bd = _place(a, pads[0], offs[0]), _place(b, pads[1], offs[1])
    out = _Out((len(a), len(b)), torch.float32, pads[2], offs[2])
    K.rbf_gram(ad, bd, gamma, k=out.view)
    torch.cuda.synchronize()
    return out.check()


# ------------------------------------------------------------------------------------------------ Gram matrix
def _pairwise_cases():
    """A greedy pairwise covering of (na, nb, d) choices (indices into the size lists): every pair of values of any two
    of the three appears in some case."""
    levels = (5, 5, 6)
    need = {(i, a, j, b) for i, j in ((0, 1), (0, 2), (1, 2)) for a in range(levels[i]) for b in range(levels[j])}
    cases = []
    while need:
        best = max(itertools.product(*(range(m) for m in levels)),
                   key=lambda c: sum((i, c[i], j, c[j]) in need for i, j in ((0, 1), (0, 2), (1, 2))))
        cases.append(best)
        need -= {(i, best[i], j, best[j]) for i, j in ((0, 1), (0, 2), (1, 2))}
    return cases


GRAM_CASES = _pairwise_cases()
DIMS = (1, 31, 32, 33, 69, 513)


def test_the_covering_is_pairwise():
    for i, j in ((0, 1), (0, 2), (1, 2)):
        assert len({(c[i], c[j]) for c in GRAM_CASES}) == (5, 5, 6)[i] * (5, 5, 6)[j]
    assert len(GRAM_CASES) <= 40


@pytest.mark.parametrize("case", range(len(GRAM_CASES)))
def test_gram_within_the_derived_bound(tiles, case):
    ta, tb, _ = tiles
    ia, ib, idd = GRAM_CASES[case]
    na = (1, ta - 1, ta, ta + 1, 2 * ta + 3)[ia]
    nb = (1, tb - 1, tb, tb + 1, 2 * tb + 3)[ib]
    d = DIMS[idd]
    a, b = gen.normal(9000 + case, (na, d)), gen.normal(9100 + case, (nb, d), 1.0, 0.25)
    gamma = 1.0 / d
    pads = ((0, 0, 0), (3, 1, 5), (4, 8, 4), (1, 0, 3))[case % 4]
    offs = ((0, 0, 0), (1, 3, 1), (4, 4, 4), (0, 2, 3))[case % 4]
    k = _gram(a, b, gamma, pads, offs)
    err = np.abs(k.astype(np.float64) - R.gram64(a, b, gamma))
    bound = R.eps_gram(a, b, gamma)
    worst = float((err / bound).max())
    print(f"gram na={na} nb={nb} d={d}: max err / bound = {worst:.3f}")
    assert (err <= bound).all(), worst


def test_gram_of_exact_distances_is_expf_within_2_ulp(tiles):
    ta, tb, _ = tiles
    a = gen.randint(41, (ta + 5, 33), -4, 5).astype(np.float32)
    b = gen.randint(42, (2 * tb + 3, 33), -4, 5).astype(np.float32)
    b[:3] = a[:3]
    gamma = 2.0 ** -6                                          # dist <= 33 * 64: integers, exact in f32, as gamma dist is
    k = _gram(a, b, gamma, (3, 0, 1), (1, 0, 1))
    want = np.exp(-gamma * R.sqdist64(a, b))
    ulp = np.spacing(want.astype(np.float32)).astype(np.float64)
    assert (np.abs(k.astype(np.float64) - want) <= 2 * ulp).all()
    assert (k[np.arange(3), np.arange(3)] == 1.0).all()        # distance 0 gives exactly 1


def test_gram_of_a_set_against_itself_is_bit_symmetric_and_repeatable(tiles):
    ta, _, _ = tiles
    x = gen.normal(77, (2 * ta + 3, 69), 2.0)
    k1 = _gram(x, x, 0.01, (1, 1, 3), (1, 1, 1))
    k2 = _gram(x, x, 0.01, (1, 1, 3), (1, 1, 1))
    assert np.array_equal(_bits(k1), _bits(k1.T.copy()))
    assert np.array_equal(_bits(k1), _bits(k2))
    k3 = _gram(x, x, 0.01)                                     # another alignment: 16-byte loads and stores
    assert np.array_equal(_bits(k1), _bits(k3))
    d = np.diag(k1)
    assert (d <= 1.0).all() and (d >= 1.0 - 1e-3).all()       # 1, or a hair below


@pytest.mark.parametrize("d, pad, off", [(33, 0, 0), (69, 3, 1)])
def test_gram_of_one_buffer_against_itself_mirrors_the_upper_tiles_bit_for_bit(tiles, d, pad, off):
    """a and b the same rows in memory: only the tiles on or above the diagonal are computed and mirrored; the bits
    are those of the general path (two buffers), with and without 16-byte stores."""
    from arcweld import kernels as K
    ta = tiles[0]
    for n in (1, ta - 1, ta + 1, 2 * ta + 3, 3 * ta):
        x = gen.normal(880 + n, (n, d), 1.5)
        xd = _place(x, pad, off)
        out = _Out((n, n), torch.float32, pad, off)
        K.rbf_gram(xd, xd, 0.02, k=out.view)
        torch.cuda.synchronize()
        k = out.check()
        assert np.array_equal(_bits(k), _bits(_gram(x, x, 0.02, (pad, pad, pad), (off, off, off)))), n
        assert np.array_equal(_bits(k), _bits(k.T.copy()))


def test_gram_huge_distances_give_zero_without_nan():
    a = np.array([[1e18, 1e18], [3e19, 0.0], [1.0, 2.0]], np.float32)
    b = np.array([[-1e18, -1e18], [-3e19, 0.0]], np.float32)
    k = _gram(a, b, 1.0)
    assert np.isfinite(k).all() and (k == 0.0).all()


def test_gram_refused_calls_leave_the_output_untouched():
    from arcweld import _native as nat
    from arcweld import kernels as K
    a, b = _place(gen.normal(1, (5, 7))), _place(gen.normal(2, (6, 7)))
    out = _Out((5, 6), torch.float32)
    for gamma in (0.0, -1.0, float("inf"), float("nan")):
        with pytest.raises(nat.NativeError, match="gamma"):
            K.rbf_gram(a, b, gamma, k=out.view)
    s = nat.stream_ptr()
    bad = [(nat.ptr(a), 5, 6, nat.ptr(b), 6, 7, 7, 1.0, nat.ptr(out.view), 6),      # lda < d
           (nat.ptr(a), 5, 7, nat.ptr(b), 6, 7, 7, 1.0, nat.ptr(out.view), 5),      # ldk < nb
           (nat.ptr(a), 5, 7, nat.ptr(b), 6, 7, 0, 1.0, nat.ptr(out.view), 6),      # d < 1
           (nat.ptr(a), -1, 7, nat.ptr(b), 6, 7, 7, 1.0, nat.ptr(out.view), 6),     # na < 0
           (None, 5, 7, nat.ptr(b), 6, 7, 7, 1.0, nat.ptr(out.view), 6),            # NULL a
           (nat.ptr(a), 5, 7, nat.ptr(b), 6, 7, 7, 1.0, None, 6)]                   # NULL k
    for args in bad:
        with pytest.raises(nat.NativeError, match="aw_rbf_gram"):
            nat.call("aw_rbf_gram", *args, s)
    nat.call("aw_rbf_gram", None, 0, 7, nat.ptr(b), 6, 7, 7, 1.0, None, 6, s)       # na = 0: fine, nothing launched
    torch.cuda.synchronize()
    out.check(untouched=True)


# ------------------------------------------------------------------------------------------------ solver
def _problem(seed, n, d=8, sep=2.0, share=None):
    """x, labels and the f32 kernel matrix at gamma = 'scale' (computed in fp64, rounded: symmetric by construction)."""
    x, lab = R.blobs(seed, n, d, sep=sep, share=share)
    k = R.gram64(x, x, R.rbf_gamma(x)).astype(np.float32)
    return x, lab, k


class _State:
    """The solver's in/out arrays between canaries, for P problems of n rows."""

    def __init__(self, P, n, alpha=None, grad=None):
        self.alpha = _Out((P, n), torch.float64).set(np.zeros((P, n)) if alpha is None else alpha)
        self.grad = _Out((P, n), torch.float64).set(-np.ones((P, n)) if grad is None else grad)
        self.n_iter = _Out((P,), torch.int64).set(np.zeros(P, np.int64))
        self.gap = _Out((P,), torch.float64)

    def read(self, untouched=False):
        torch.cuda.synchronize()
        return (self.alpha.check(), self.grad.check(), self.n_iter.check(), self.gap.check(untouched))


def _solve(k, y, C, tol=1e-3, max_iter=10 ** 6, chunk=None, pad=0, state=None, kd=None):
    """Solve on the device from scratch (or from `state`); chunk: iterations per launch.  Returns alpha, grad,
    n_iter, gap as numpy after checking the canaries."""
    from arcweld import kernels as K
    y = np.atleast_2d(np.asarray(y, np.int32))
    P, n = y.shape
    kd = _place(k, pad, 4 if pad else 0) if kd is None else kd
    yd = torch.as_tensor(y, device="cuda")
    st = _State(P, n) if state is None else state
    Cs = [float(C)] * P if np.isscalar(C) else list(C)
    done = 0
    while True:
        step = max_iter - done if chunk is None else min(chunk, max_iter - done)
        K.svm_smo(kd, yd, Cs, tol, step, alpha=st.alpha.view, grad=st.grad.view, n_iter=st.n_iter.view,
                  gap=st.gap.view)
        done += step
        out = st.read()
        if done >= max_iter or (out[3] <= tol).all():
            return out


def _conditions(k, y, C, tol, alpha, grad, n_iter, gap, ref=True):
    """(a) - (e) for one problem; returns the measured fractions of the bounds."""
    y = np.asarray(y)
    act = y != 0
    k64 = np.asarray(k, np.float64)
    drift = 8 * max(int(n_iter), 1) * U53 * C * np.abs(k64).max()
    assert (alpha >= 0).all() and (alpha <= C).all() and (alpha[~act] == 0).all()                      # (a)
    b = abs(float((y * alpha).sum()))
    assert b <= 4 * int(n_iter) * U53 * C, (b, 4 * int(n_iter) * U53 * C)                               # (b)
    G64 = R.grad64(k64, y, alpha)
    g64 = R.gap_of(G64, y, alpha, C)[0]
    assert g64 <= tol + drift, (g64, tol, drift)                                                        # (c)
    dg = float(np.abs(grad - G64)[act].max()) if act.any() else 0.0
    assert dg <= drift, (dg, drift)                                                                     # (d)
    assert gap <= tol and abs(gap - R.gap_of(grad, y, alpha, C)[0]) == 0.0
    out = {"sum_y_alpha": b / (4 * max(int(n_iter), 1) * U53 * C), "grad_drift": dg / drift}
    if ref:
        f = R.fit(k64, y, C, tol)
        obj = R.objective(alpha, grad, y)
        assert abs(obj - f["objective"]) <= tol * C * int(act.sum()), (obj, f["objective"])            # (e)
        out["objective"] = abs(obj - f["objective"]) / (tol * C * int(act.sum()))
        out["n_iter"] = (int(n_iter), f["n_iter"])
    return out


def test_smo_two_rows_analytically():
    for k12, C, want in ((0.5, 10.0, 2.0), (0.5, 0.5, 0.5), (0.25, 10.0, 1.0 / 0.75)):
        k = np.array([[1.0, k12], [k12, 1.0]], np.float32)
        alpha, grad, n_iter, gap = _solve(k, [1, -1], C)
        assert np.allclose(alpha[0], [want, want], rtol=1e-15, atol=0) and n_iter[0] == 1 and gap[0] <= 1e-3


def test_smo_degenerate_problems_run_no_iteration():
    _, _, k = _problem(3, 6)
    ys = np.array([[1, 1, 1, 1, 1, 1], [0, 0, 0, 0, 0, 0], [-1, 0, -1, 0, 0, -1]], np.int32)
    alpha, grad, n_iter, gap = _solve(k, ys, 1.0, max_iter=50)
    assert (gap == -np.inf).all() and (n_iter == 0).all() and (alpha == 0).all() and (grad == -1).all()
    alpha, grad, n_iter, gap = _solve(k[:1, :1], [[1]], 1.0, max_iter=50)
    assert gap[0] == -np.inf and n_iter[0] == 0 and alpha[0, 0] == 0
    from arcweld import kernels as K
    st = _State(2, 0)
    K.svm_smo(torch.empty((0, 0), device="cuda"), torch.empty((2, 0), dtype=torch.int32, device="cuda"), 1.0, 1e-3, 5,
              alpha=st.alpha.view, grad=st.grad.view, n_iter=st.n_iter.view, gap=st.gap.view)
    assert (st.read()[3] == -np.inf).all()


@pytest.mark.parametrize("which", ["T-1", "T", "T+1", "2T+3"])
def test_smo_conditions_around_the_thread_count(smo_dims, which):
    T = smo_dims[0]
    n = {"T-1": T - 1, "T": T, "T+1": T + 1, "2T+3": 2 * T + 3}[which]
    _, lab, k = _problem(500 + n, n)
    y = 2 * lab - 1
    out = _solve(k, y, 1.0, pad=5)
    print(f"smo n={n}:", _conditions(k, y, 1.0, 1e-3, out[0][0], out[1][0], out[2][0], out[3][0]))


@pytest.mark.parametrize("C, share", [(0.25, 0.1), (10.0, 0.5)])
def test_smo_conditions_at_the_bound_and_free(C, share):
    n = 700
    _, lab, k = _problem(61, n, sep=3.0 if C > 1 else 1.0, share=share)
    y = 2 * lab - 1
    alpha, grad, n_iter, gap = _solve(k, y, C)
    print(f"smo C={C}:", _conditions(k, y, C, 1e-3, alpha[0], grad[0], n_iter[0], gap[0]))
    minority = y == (1 if lab.sum() * 2 < n else -1)
    free = (alpha[0] > 0) & (alpha[0] < C)
    if C < 1:
        assert (alpha[0][minority] == C).all()                 # every minority row ends at the bound
    else:
        assert free.sum() > 0.5 * (alpha[0] > 0).sum()         # mostly free rows (the reference: 103 of 155)


def _masked_problems(seed, P, n):
    lab3 = gen.randint(seed, (P, n), 0, 4)                     # a quarter of the rows of every problem masked
    sign = 2 * gen.randint(seed + 1, (P, n), 0, 2) - 1
    return np.where(lab3 == 0, 0, sign).astype(np.int32)


def test_smo_three_problems_equal_three_single_solves_bit_for_bit():
    n = 300
    _, _, k = _problem(71, n)
    ys, Cs = _masked_problems(72, 3, n), [0.25, 1.0, 7.0]
    both = _solve(k, ys, Cs)
    for c in range(3):
        one = _solve(k, ys[c], Cs[c])
        for a, b in zip(both, one):
            assert np.array_equal(_bits(a[c]), _bits(b[0]))
        _conditions(k, ys[c], Cs[c], 1e-3, both[0][c], both[1][c], both[2][c], both[3][c])


def test_smo_thirty_two_problems(smo_dims):
    P, n = smo_dims[3], 257
    _, _, k = _problem(81, n)
    ys = _masked_problems(82, P, n)
    Cs = [float(c) for c in 10.0 ** gen.uniform(83, (P,), -0.6, 1.0)]
    alpha, grad, n_iter, gap = _solve(k, ys, Cs)
    for c in range(P):
        _conditions(k, ys[c], Cs[c], 1e-3, alpha[c], grad[c], n_iter[c], gap[c], ref=c % 11 == 0)


def test_smo_masked_rows_and_longer_register_arrays_change_no_bit(smo_dims):
    """n = 2 T rows run the shortest instantiation; the same rows inside a matrix of 2 T + 100, the rest masked, run
    the next one: alpha, grad, n_iter and gap of the rows that take part must agree bit for bit, the masked rows'
    alpha and grad must be left alone."""
    T = smo_dims[0]
    n, big = 2 * T, 2 * T + 100
    _, lab, k = _problem(91, big)
    y = 2 * lab - 1
    small = _solve(k[:n, :n], y[:n], 1.0)
    yb = y.copy()
    yb[n:] = 0
    st = _State(1, big, grad=np.where(yb != 0, -1.0, 5.0)[None])
    large = _solve(k, yb, 1.0, state=st)
    assert np.array_equal(_bits(small[0][0]), _bits(large[0][0, :n])) and (large[0][0, n:] == 0).all()
    assert np.array_equal(_bits(small[1][0]), _bits(large[1][0, :n])) and (large[1][0, n:] == 5.0).all()
    assert small[2][0] == large[2][0] and _bits(small[3])[0] == _bits(large[3])[0]


def test_smo_resumption():
    n = 400
    _, lab, k = _problem(95, n)
    y = 2 * lab - 1
    whole = _solve(k, y, 2.0)
    again = _solve(k, y, 2.0)
    pieces = _solve(k, y, 2.0, chunk=7)
    for a, b, c in zip(whole, again, pieces):
        assert np.array_equal(_bits(a), _bits(b)) and np.array_equal(_bits(a), _bits(c))
    assert whole[2][0] > 14
    # a further launch on the converged state changes nothing
    st = _State(1, n, alpha=whole[0], grad=whole[1])
    st.n_iter.set(whole[2])
    more = _solve(k, y, 2.0, state=st, max_iter=100)
    for a, b in zip(whole, more):
        assert np.array_equal(_bits(a), _bits(b))
    # max_iter = 0 only writes the gap
    st = _State(1, n)
    alpha, grad, n_iter, gap = _solve(k, y, 2.0, state=st, max_iter=0)
    assert (alpha == 0).all() and (grad == -1).all() and n_iter[0] == 0 and gap[0] == 2.0      # m - M = 1 - (-1)
    # stopped by the cap: the state is the same as the first iterations of the whole solve
    capped = _solve(k, y, 2.0, max_iter=9)
    assert capped[2][0] == 9 and capped[3][0] > 1e-3


def test_smo_refused_calls_leave_every_output_untouched():
    from arcweld import _native as nat
    from arcweld import kernels as K
    n = 5
    _, _, k = _problem(97, n)
    kd, yd = _place(k), torch.ones((2, n), dtype=torch.int32, device="cuda")
    st = _State(2, n)
    before = [t.buf.clone() for t in (st.alpha, st.grad, st.n_iter, st.gap)]
    for C, tol, mi, what in (([1.0, 0.0], 1e-3, 5, "C"), ([1.0, float("inf")], 1e-3, 5, "C"),
                             ([float("nan"), 1.0], 1e-3, 5, "C"), ([1.0, 1.0], 0.0, 5, "tol"),
                             ([1.0, 1.0], float("nan"), 5, "tol"), ([1.0, 1.0], 1e-3, -1, "max_iter")):
        with pytest.raises(nat.NativeError, match=what):
            K.svm_smo(kd, yd, C, tol, mi, alpha=st.alpha.view, grad=st.grad.view, n_iter=st.n_iter.view,
                      gap=st.gap.view)
    import ctypes
    Ca = (ctypes.c_double * 2)(1.0, 1.0)
    Cp = ctypes.cast(Ca, ctypes.c_void_p)
    ptrs = [nat.ptr(kd), nat.ptr(yd), nat.ptr(st.alpha.view), nat.ptr(st.grad.view), nat.ptr(st.n_iter.view),
            nat.ptr(st.gap.view)]
    s = nat.stream_ptr()

    def raw(n_=n, ldk=n, p=2, C=Cp, null=None):
        q = [None if i == null else v for i, v in enumerate(ptrs)]
        nat.call("aw_svm_smo", q[0], n_, ldk, q[1], C, p, 1e-3, 5, q[2], q[3], q[4], q[5], s)

    for kw in (dict(n_=-1), dict(n_=20481, ldk=20481), dict(ldk=n - 1), dict(p=0), dict(p=33), dict(C=None),
               *(dict(null=i) for i in range(6))):
        with pytest.raises(nat.NativeError, match="aw_svm_smo"):
            raw(**kw)
    torch.cuda.synchronize()
    for t, b in zip((st.alpha, st.grad, st.n_iter, st.gap), before):
        assert torch.equal(t.buf, b)
    st.gap.check(untouched=True)


def _device_conditions(k, y, C, tol, alpha, grad, n_iter, gap):
    """(a) - (d) with chunked f64 torch on the device, for sizes whose f64 matrix does not belong on the host."""
    n = y.numel()
    yf = y.double()
    coef = yf * alpha
    G64 = torch.empty(n, dtype=torch.float64, device="cuda")
    kmax = 0.0
    for o in range(0, n, 2048):
        rows = k[o:o + 2048].double()
        G64[o:o + 2048] = rows @ coef
        kmax = max(kmax, float(rows.abs().max()))
    G64 = yf * G64 - 1.0
    it = int(n_iter)
    drift = 8 * max(it, 1) * U53 * C * kmax
    assert bool(((alpha >= 0) & (alpha <= C)).all())
    b = abs(float((yf * alpha).sum()))
    assert b <= 4 * it * U53 * C, (b, 4 * it * U53 * C)
    v = -yf * G64
    up = ((y > 0) & (alpha < C)) | ((y < 0) & (alpha > 0))
    low = ((y > 0) & (alpha > 0)) | ((y < 0) & (alpha < C))
    g64 = float(v[up].max() - v[low].min())
    assert g64 <= tol + drift, (g64, tol, drift)
    dg = float((grad - G64).abs().max())
    assert dg <= drift, (dg, drift)
    assert float(gap) <= tol
    return {"n_iter": it, "sum_y_alpha": b / (4 * max(it, 1) * U53 * C), "grad_drift": dg / drift, "gap64": g64}


@pytest.mark.parametrize("which", ["8T+1", "MAX_N"])
def test_smo_longest_register_arrays_on_a_device_gram(smo_dims, which):
    """n just above the middle instantiation's limit, and AW_SVM_MAX_N (the last register slot) with 512 positive
    rows, d = 8, C = 0.1, on the Gram matrix aw_rbf_gram leaves on the device (1.7 GB at full size)."""
    from arcweld import kernels as K
    T, _, max_n, _ = smo_dims
    n = 8 * T + 1 if which == "8T+1" else max_n
    x = gen.normal(4242, (n, 8)).astype(np.float64)
    lab = np.zeros(n, np.int64)
    lab[np.argsort(gen.uniform(4243, (n,)), kind="stable")[:512]] = 1
    x[:, 0] += 2.0 * lab
    xd = torch.as_tensor(x.astype(np.float32), device="cuda")
    k = K.rbf_gram(xd, xd, float(np.float32(R.rbf_gamma(x.astype(np.float32)))))
    assert bool((k == k.t()).all())
    y = torch.as_tensor((2 * lab - 1).astype(np.int32), device="cuda")[None].contiguous()
    alpha, grad, n_iter, gap = K.svm_smo(k, y, 0.1, 1e-3, 20000)
    torch.cuda.synchronize()
    out = _device_conditions(k, y[0], 0.1, 1e-3, alpha[0], grad[0], n_iter[0], gap[0])
    print(f"smo n={n}:", out)
    assert 100 < out["n_iter"] < 20000


# ------------------------------------------------------------------------------------------------ fit and decisions
FIT_N, FIT_D, FIT_Q = 600, 20, 400


@pytest.fixture(scope="module")
def fit_data():
    x, lab = R.blobs(1234, FIT_N + FIT_Q, FIT_D, sep=3.0)
    return x[:FIT_N], lab[:FIT_N], x[FIT_N:], lab[FIT_N:]


def _dev(a, dtype=None):
    return torch.as_tensor(np.asarray(a), device="cuda") if dtype is None else \
        torch.as_tensor(np.asarray(a), device="cuda").to(dtype)


def _band(kq, k, y, C, tol):
    """dec_ref(tol / 100) and e = max |dec_ref(tol) - dec_ref(tol / 100)| on the query rows (reference only)."""
    f1, f2 = R.fit(k, y, C, tol), R.fit(k, y, C, tol / 100)
    d1, d2 = R.decision(kq, f1["coef"], f1["rho"]), R.decision(kq, f2["coef"], f2["rho"])
    return d2, float(np.abs(d1 - d2).max())


def test_fit_decisions_within_three_e_of_the_reference(fit_data):
    from arcweld import kernels as K
    from arcweld.retrieve import svm_decision, svm_fit, svm_predict
    x, lab, q, _ = fit_data
    tol = 1e-3
    fit = svm_fit(_dev(x), _dev(lab), C=(0.1, 10.0), tol=tol)
    assert fit["pairs"] == [(1, 0)] and bool(fit["converged"].all()) and fit["standardize"] is False
    g = fit["gamma"]
    assert g == float(np.float32(g)) and abs(g - R.rbf_gamma(x)) <= 1e-6 * g
    k = K.rbf_gram(_dev(x), _dev(x), g).cpu().numpy()
    kq = K.rbf_gram(_dev(q), _dev(x), g).cpu().numpy()
    dec = svm_decision(fit, _dev(q)).cpu().numpy()
    pred = svm_predict(fit, _dev(q)).cpu().numpy()
    y = 2 * lab - 1
    for ci, C in enumerate((0.1, 10.0)):
        want, e = _band(kq, k, y, C, tol)
        ratio = float(np.abs(dec[ci, :, 0] - want).max() / e)
        inside = float((np.abs(want) <= 3 * e).mean())
        print(f"decision C={C}: max |dec - dec_ref(tol/100)| / e = {ratio:.3f}, rows inside the band {inside:.4f}")
        assert ratio <= 3.0 and inside <= 0.02
        sure = np.abs(want) > 3 * e
        assert np.array_equal(pred[ci][sure], (want > 0).astype(np.int64)[sure])
        assert np.array_equal(pred[ci], (dec[ci, :, 0] > 0).astype(np.int64))
        alpha = np.abs(fit["dual_coef"][ci, 0].cpu().numpy())
        assert abs(float(fit["objective"][ci, 0]) - R.fit(k, y, C, tol)["objective"]) <= tol * C * FIT_N
        assert int(fit["n_support"][ci, 0]) == int((alpha > 0).sum())
        G = R.grad64(k, y, alpha)
        assert abs(float(fit["rho"][ci, 0]) - R.rho(alpha, G, y, C)) <= 1e-9
    sup = fit["support"].cpu().numpy()
    assert np.array_equal(sup, np.flatnonzero((fit["dual_coef"].cpu().numpy() != 0).any((0, 1))))
    assert np.array_equal(fit["support_vectors"].cpu().numpy(), x[sup])


def test_fit_two_C_at_once_equals_two_single_fits(fit_data):
    from arcweld.retrieve import svm_fit
    x, lab = _dev(fit_data[0]), _dev(fit_data[1])
    both = svm_fit(x, lab, C=(0.1, 10.0))
    for ci, C in enumerate((0.1, 10.0)):
        one = svm_fit(x, lab, C=C)
        for key in ("dual_coef", "rho", "n_iter", "gap", "objective"):
            assert torch.equal(both[key][ci], one[key][0]), key


def test_fit_three_classes_one_vs_one_against_the_reference_vote():
    from arcweld import kernels as K
    from arcweld.retrieve import svm_decision, svm_fit, svm_predict
    x, lab = R.blobs(321, 450, 12, sep=4.0, n_classes=3)
    q, _ = R.blobs(322, 200, 12, sep=4.0, n_classes=3)
    fit = svm_fit(_dev(x), _dev(lab), C=1.0)
    pairs = R.pairs_of(3)
    assert fit["pairs"] == pairs == [(0, 1), (0, 2), (1, 2)] and fit["n_classes"] == 3
    g = fit["gamma"]
    k = K.rbf_gram(_dev(x), _dev(x), g).cpu().numpy()
    kq = K.rbf_gram(_dev(q), _dev(x), g).cpu().numpy()
    ys = R.pair_labels(lab, pairs)
    coef = fit["dual_coef"].cpu().numpy()
    for p, (a, b) in enumerate(pairs):
        assert (coef[0, p][(lab != a) & (lab != b)] == 0).all() and (np.sign(coef[0, p]) * ys[p] >= 0).all()
    dec = svm_decision(fit, _dev(q)).cpu().numpy()[0]
    want, sure = np.empty_like(dec), np.ones(len(q), bool)
    for p in range(3):
        want[:, p], e = _band(kq, k, ys[p], 1.0, 1e-3)
        assert (np.abs(dec[:, p] - want[:, p]) <= 3 * e).all()
        sure &= np.abs(want[:, p]) > 3 * e
    pred = svm_predict(fit, _dev(q)).cpu().numpy()[0]
    assert np.array_equal(pred, R.vote(dec, pairs, 3))
    assert np.array_equal(pred[sure], R.vote(want, pairs, 3)[sure]) and sure.mean() > 0.9


def test_fit_thirty_three_problems_run_in_two_groups():
    from arcweld.retrieve import svm_fit
    x, lab = R.blobs(555, 240, 10, sep=3.0, n_classes=3)
    Cs = [float(c) for c in np.linspace(0.05, 2.0, 11)]
    fit = svm_fit(_dev(x), _dev(lab), C=Cs)
    assert tuple(fit["dual_coef"].shape) == (11, 3, 240) and bool(fit["converged"].all())
    last = svm_fit(_dev(x), _dev(lab), C=Cs[10])
    for key in ("dual_coef", "rho", "n_iter", "objective"):
        assert torch.equal(fit[key][10], last[key][0]), key


def test_fit_standardised_and_gamma_given(fit_data):
    from arcweld import kernels as K
    from arcweld.retrieve import svm_decision, svm_fit
    x, lab, q, _ = fit_data
    x = (x * np.linspace(0.1, 30.0, FIT_D)[None, :] + 5.0).astype(np.float32)
    x[3, 4] = np.nan                                            # nan_to_num: 0 before the scaler
    xz = np.nan_to_num(x)
    mean, scale = KR.scaler(xz)
    zx = KR.standardize(xz, mean, scale)
    fit = svm_fit(_dev(x), _dev(lab), C=1.0, standardize=True)
    assert np.allclose(fit["mean"].cpu().numpy(), mean, rtol=1e-9, atol=1e-9)
    assert np.allclose(fit["scale"].cpu().numpy(), scale, rtol=1e-9)
    assert abs(fit["gamma"] - R.rbf_gamma(zx)) <= 1e-5 * fit["gamma"] and bool(fit["converged"].all())
    fit2 = svm_fit(_dev(x), _dev(lab), C=1.0, gamma=0.03, standardize=True)
    assert fit2["gamma"] == float(np.float32(0.03))
    qz = KR.standardize(np.nan_to_num(q), mean, scale)
    sv = fit2["support_vectors"].cpu().numpy()
    assert np.abs(sv - zx[fit2["support"].cpu().numpy()]).max() <= 1e-6
    kq = K.rbf_gram(_dev(qz), _dev(sv), fit2["gamma"]).cpu().numpy().astype(np.float64)
    coef = fit2["dual_coef"][0, 0][fit2["support"]].cpu().numpy()
    want = kq @ coef - float(fit2["rho"][0, 0])
    got = svm_decision(fit2, _dev(q)).cpu().numpy()[0, :, 0]
    assert np.abs(got - want).max() <= 1e-4 * max(1.0, np.abs(coef).sum())   # the queries' f32 standardisation


def test_fit_refuses_too_many_rows_before_any_device_work():
    from arcweld.retrieve import svm_fit
    with pytest.raises(ValueError, match="max_samples"):
        svm_fit(torch.zeros(20481, 2), torch.zeros(20481, dtype=torch.long))


# ------------------------------------------------------------------------------------------------ probe and script
KW = dict(hidden_dim=64, num_embeddings=32, embedding_dim=16, n_resblocks=2, patch_size=25)
N_CYCLES, SIZES = 2, (64, 9, 7)
METRICS = {"acc", "acc_good", "acc_bad", "f1"}


@pytest.fixture(scope="module")
def vqvae():
    from model.vq_vae_patch_embedd import VQVAEPatch
    v = VQVAEPatch(input_dim=2, learning_rate=1e-3, dropout_p=0.0, batch_norm=False, **KW)
    v.load_state_dict({k: torch.tensor(a) for k, a in ov.det_state_dict(ov.VQVAEConfig(**KW), 2501).items()})
    return v.cuda().eval()


@pytest.fixture(scope="module")
def splits():
    out = []
    for i, n in enumerate(SIZES):
        lab = gen.randint(410 + i, (n,), 0, 2)
        x = gen.windows(400 + i, n * N_CYCLES).reshape(n, N_CYCLES * 200, 2) + 0.15 * lab[:, None, None]
        out.append((torch.tensor(x.astype(np.float32), device="cuda"), torch.tensor(lab, device="cuda")))
    return out


@pytest.fixture
def fp32():
    from arcweld.precision import operands
    with operands(torch.float32):
        yield


@pytest.mark.parametrize("dataset", ["latent_vq_vae", "asimow"])
def test_probe_metrics_and_selection(vqvae, splits, fp32, dataset):
    from arcweld.retrieve import latent_svm_probe, svm_fit
    Cs = (10.0, 0.5)
    res = latent_svm_probe(splits, N_CYCLES, C=Cs, dataset=dataset, vqvae=vqvae)
    assert set(res) == {"val", "test", "per_C", "C_selected", "fit", "gamma", "n_support", "converged", "n_iter"}
    assert res["converged"] == [True, True] and len(res["n_iter"]) == 2 and res["gamma"] == res["fit"]["gamma"]
    labels = [y.cpu().numpy() for _, y in splits]
    best = None
    for ci in sorted(range(2), key=lambda i: Cs[i]):
        entry = res["per_C"][ci]
        assert entry["C"] == Cs[ci] and set(entry) == {"C", "val", "test", "n_support"}
        assert entry["n_support"] == res["n_support"][ci] == int(res["fit"]["n_support"][ci, 0]) > 0
        if best is None or entry["val"]["f1"] > res["per_C"][best]["val"]["f1"]:
            best = ci
    assert res["C_selected"] == Cs[best]
    for qi, name in ((1, "val"), (2, "test")):
        r = res[name]
        assert set(r) == METRICS | {"pred", "decision"}
        pred, dec = r["pred"].cpu().numpy(), r["decision"].cpu().numpy()
        assert dec.shape == (SIZES[qi], 1) and np.array_equal(pred, (dec[:, 0] > 0).astype(np.int64))
        for m, v in KR.metrics(pred, labels[qi]).items():
            assert abs(r[m] - v) <= 1e-6 and r[m] == res["per_C"][best][name][m]
    if dataset == "asimow":                                     # the probe is svm_fit on the flattened windows
        direct = svm_fit(splits[0][0].reshape(SIZES[0], -1), splits[0][1], C=Cs)
        assert torch.equal(res["fit"]["dual_coef"], direct["dual_coef"])
    with pytest.raises(ValueError, match="^splits:.*C = inf"):
        latent_svm_probe([(x[:40], y[:40]) for x, y in splits], N_CYCLES, dataset="asimow")


def test_probe_subsamples_the_train_split(splits, fp32):
    from arcweld.retrieve import latent_svm_probe, svm_fit
    import logreg_refs as LR
    rows = LR.stratified_subsample(splits[0][1].cpu().numpy(), 55, seed=42)
    res = latent_svm_probe(splits, N_CYCLES, C=(1.0,), dataset="asimow", max_samples=55)
    sub = torch.as_tensor(rows, device="cuda")
    direct = svm_fit(splits[0][0][sub].reshape(55, -1), splits[0][1][sub], C=1.0)
    assert torch.equal(res["fit"]["dual_coef"], direct["dual_coef"])


def test_script_svm_protocol(vqvae, fp32, tmp_path):
    import probe_latent_space as pls
    ckpt, out, model = tmp_path / "v.ckpt", tmp_path / "probe.json", tmp_path / "model.npz"
    vqvae.save_checkpoint(str(ckpt))
    common = ["--vqvae-model", str(ckpt), "--n-cycles", str(N_CYCLES), "--n-train", "60", "--n-val", "5", "--n-test",
              "6", "--seed", "3", "--out", str(out)]
    pls.main(pls.parser().parse_args(common + ["--protocol", "svm", "--C", "0.1", "1.0", "--model-out", str(model)]))
    summary = json.loads(out.read_text())
    assert set(summary) == {"val", "test", "per_C", "C_selected", "protocol", "dataset", "standardize", "n_cycles",
                            "converged", "n_iter", "gamma", "n_support"}
    assert summary["protocol"] == "svm" and summary["standardize"] is False and summary["converged"] == [True, True]
    assert [e["C"] for e in summary["per_C"]] == [0.1, 1.0] and summary["gamma"] > 0
    assert summary["n_support"] == [e["n_support"] for e in summary["per_C"]]
    for name in ("val", "test"):
        assert set(summary[name]) == METRICS and all(0.0 <= v <= 1.0 for v in summary[name].values())
    with np.load(model, allow_pickle=False) as f:
        assert set(f.files) == {"support", "support_vectors", "dual_coef", "rho", "gamma", "C", "mean", "scale"}
        nsv, D = f["support_vectors"].shape
        assert f["support"].shape == (nsv,) and f["dual_coef"].shape == (2, 1, nsv) and f["rho"].shape == (2, 1)
        assert f["mean"].shape == f["scale"].shape == (D,) and float(f["gamma"]) == summary["gamma"]
        assert f["C"].tolist() == [0.1, 1.0] and np.isfinite(f["dual_coef"]).all()
        assert (f["mean"] == 0).all() and (f["scale"] == 1).all()
    # the defaults resolve per protocol: fit_svm's C = 0.1 here, C = 1.0 under linear exactly as before
    pls.main(pls.parser().parse_args(common + ["--protocol", "svm", "--gamma", "0.001", "--standardize"]))
    summary = json.loads(out.read_text())
    assert [e["C"] for e in summary["per_C"]] == [0.1] and summary["standardize"] is True
    assert summary["gamma"] == float(np.float32(0.001))
    pls.main(pls.parser().parse_args(common + ["--protocol", "linear"]))
    summary = json.loads(out.read_text())
    assert [e["C"] for e in summary["per_C"]] == [1.0] and summary["protocol"] == "linear"
    assert set(summary) == {"val", "test", "per_C", "C_selected", "protocol", "dataset", "standardize", "n_cycles",
                            "converged", "n_iter"}
    with pytest.raises(SystemExit, match="neighbours-out"):
        pls.main(pls.parser().parse_args(common + ["--protocol", "svm", "--neighbours-out", str(tmp_path / "nb.npz")]))
    with pytest.raises(SystemExit, match="C = inf"):
        pls.main(pls.parser().parse_args(common[:4] + ["--n-train", "30"] + common[6:] + ["--protocol", "svm"]))
