"""aw_sample_next_ex (aw_sample_next with a min-p and a nucleus filter and the likelihood of the pick) against numpy
f64 restatements on x = f32(logit * f32(inv_t)), using the kernel's own draws u: the old path bit for bit, the kept set
as an upper set of x, the nucleus property and the minimal nucleus, min-p, the filtered CDF, logp / logq, and
hand-built rows (ties across the mass boundary, bad rows, refused arguments, bit-identical relaunches)."""
import numpy as np
import pytest
import torch

from oracle import gen

pytestmark = pytest.mark.gpu

VS, BS = (34, 514, 1030, 8194), (1, 5)     # 1030 and 8194: the 4096- and 16384-column LDS instantiations
TOL = 1e-4                                 # tests/test_score_rows_gpu.py's bar for a logit minus a log-sum-exp


def _slack(V):
    """tests/test_sample_next_gpu.py's bound for f32 partial sums <= 1 over V columns."""
    return V * 2.0 ** -24 + 2.0 ** -20


def _logits(seed, B, V):
    return gen.normal(seed, (B, V), std=3.0)


def _run(logits, greedy_filters=True, **kw):
    """One launch with every optional output: dict of numpy arrays (ids, u, logp, logq, n_kept, thr) and bad."""
    from arcweld import kernels as K
    lg = torch.as_tensor(np.ascontiguousarray(logits), device="cuda")
    B = lg.shape[0]
    ids = torch.full((B, 3), -7, dtype=torch.int64, device="cuda")
    u = torch.full((B,), -1.0, device="cuda")
    lp = torch.full((2, B, 4), 7.0, device="cuda")
    nk = torch.full((B,), -7, dtype=torch.int32, device="cuda")
    thr = torch.full((B,), 7.0, device="cuda")
    bad = torch.zeros(1, dtype=torch.int32, device="cuda")
    K.sample_next_ex(lg, ids, 1, bad, u_out=u, logp_out=lp[0], logq_out=lp[1], col_lp=2,
                     n_kept_out=nk if greedy_filters else None, thr_out=thr if greedy_filters else None, **kw)
    assert (ids[:, [0, 2]] == -7).all() and (lp[:, :, [0, 1, 3]] == 7.0).all()      # only the asked columns
    return dict(ids=ids[:, 1].cpu().numpy(), u=u.cpu().numpy(), logp=lp[0, :, 2].cpu().numpy(),
                logq=lp[1, :, 2].cpu().numpy(), n_kept=nk.cpu().numpy(), thr=thr.cpu().numpy(), bad=int(bad.item()))


def _x(logits, n_valid, inv_t=1.0):
    return (np.asarray(logits, dtype=np.float32)[:, :n_valid] * np.float32(inv_t)).astype(np.float32)


def _top_k_keep(x, top_k):
    if not top_k:
        return np.ones_like(x, dtype=bool)
    return x >= np.sort(x, axis=1)[:, ::-1][:, top_k - 1:top_k]      # ties at the threshold stay


def _e64(x):
    x = x.astype(np.float64)
    return np.exp(x - x.max(axis=1, keepdims=True))


def _mass(x, keep):
    """f64 probabilities over the columns of `keep`, 0 elsewhere."""
    e = np.where(keep, _e64(x), 0.0)
    return e / e.sum(axis=1, keepdims=True)


def _minimal_nucleus(xr, pr, top_p):
    """For one row (x, f64 masses over the survivors, 0 elsewhere): the smallest x of the minimal set of most probable
    columns whose mass reaches top_p (ties of its last member included), and the cumulative mass just before and just
    after that last group of ties."""
    vals = np.unique(xr[pr > 0])[::-1]
    cum = 0.0
    for v in vals:
        before = cum
        cum += pr[xr == v].sum()
        if cum >= top_p:
            return v, before, cum
    return vals[-1], before, cum


@pytest.mark.parametrize("B", BS)
@pytest.mark.parametrize("V", VS)
def test_with_the_new_filters_off_ids_and_u_are_those_of_sample_next(V, B):
    from arcweld import kernels as K
    lg = _logits(3200 + V + B, B, V)
    lgd = torch.as_tensor(lg, device="cuda")
    for n_valid in (V, V - 2):
        for do_sample in (False, True):
            for top_k in (None, 7):
                for step in range(8):
                    kw = dict(n_valid=n_valid, top_k=top_k, do_sample=do_sample, seed=V + B, step=step)
                    out = torch.full((B, 1), -7, dtype=torch.int64, device="cuda")
                    u = torch.full((B,), -1.0, device="cuda")
                    bad = torch.zeros(1, dtype=torch.int32, device="cuda")
                    K.sample_next(lgd, out, 0, bad, u_out=u, **kw)
                    for gf in (False, True):       # with and without the filters' own outputs
                        got = _run(lg, greedy_filters=gf, top_p=1.0, min_p=0.0, **kw)
                        assert got["bad"] == 0 and int(bad.item()) == 0
                        assert np.array_equal(got["ids"], out[:, 0].cpu().numpy()), (n_valid, do_sample, top_k, step)
                        assert np.array_equal(got["u"], u.cpu().numpy())


@pytest.mark.parametrize("B", BS)
@pytest.mark.parametrize("V", VS)
def test_the_kept_set_is_an_upper_set_of_x(V, B):
    """n_kept == count(x >= thr_out) exactly, and thr_out is a value of the row, for every combination of filters."""
    lg = _logits(3250 + V + B, B, V)
    for n_valid in (V, V - 2):
        x = _x(lg, n_valid)
        for top_k in (None, 7):
            for min_p in (0.0, 0.05):
                for top_p in (0.5, 0.9, 0.99, 1.0):
                    for do_sample in (True, False):
                        got = _run(lg, n_valid=n_valid, top_k=top_k, min_p=min_p, top_p=top_p, do_sample=do_sample,
                                   seed=1)
                        what = (n_valid, top_k, min_p, top_p, do_sample)
                        assert got["bad"] == 0
                        assert np.array_equal(got["n_kept"], (x >= got["thr"][:, None]).sum(1)), what
                        assert (x == got["thr"][:, None]).any(1).all(), what
                        assert (got["n_kept"] >= 1).all() and (x.max(1) >= got["thr"]).all(), what
                        if top_k:
                            assert (got["n_kept"] <= _top_k_keep(x, top_k).sum(1)).all(), what


def _nucleus_rows(V, B, n_valids, top_ks, top_ps):
    """Runs the launches; yields (what, x row, masses over the top-k survivors, top_p, kernel thr)."""
    lg = _logits(3300 + V + B, B, V)
    for n_valid in n_valids:
        x = _x(lg, n_valid)
        for top_k in top_ks:
            p = _mass(x, _top_k_keep(x, top_k))
            for top_p in top_ps:
                got = _run(lg, n_valid=n_valid, top_k=top_k, top_p=top_p, do_sample=True, seed=2)
                assert got["bad"] == 0
                for r in range(B):
                    yield (V, B, n_valid, top_k, top_p, r), x[r], p[r], top_p, got["thr"][r]


@pytest.mark.parametrize("B", BS)
@pytest.mark.parametrize("V", VS)
def test_the_kept_set_reaches_the_mass_and_is_minimal_in_f64(V, B):
    """mass(kept) >= top_p - d and mass(kept without the columns equal to thr_out) < top_p + d, masses in f64 over the
    survivors of top-k, d = V 2^-24 + 2^-20; the compare is made on the f32 product top_p * total."""
    d = _slack(V)
    for what, xr, pr, top_p, thr in _nucleus_rows(V, B, (V, V - 2), (None, 7), (0.5, 0.9, 0.99)):
        kept = pr[xr >= thr].sum()
        assert (pr[xr >= thr] > 0).all(), what                     # inside the survivors
        assert kept >= top_p - d, (what, kept)
        assert pr[xr > thr].sum() < top_p + d, (what, pr[xr > thr].sum())


def test_clear_rows_keep_exactly_the_f64_minimal_nucleus():
    """A row is clear when the f64 cumulative mass on both sides of its boundary is more than d from top_p; there the
    kept set must be the f64 minimal nucleus.  All 48 rows of these shapes are clear (checked in f64 on the host: the
    count of exempted rows is asserted to be 0)."""
    rows = exempt = 0
    for V in (34, 514):
        d = _slack(V)
        for B in BS:
            for what, xr, pr, top_p, thr in _nucleus_rows(V, B, (V,), (None, 7), (0.5, 0.9)):
                v, before, after = _minimal_nucleus(xr, pr, top_p)
                rows += 1
                if top_p - before > d and after - top_p > d:
                    assert thr == v, (what, thr, v, before, after)
                else:
                    exempt += 1
    assert rows == 48 and exempt == 0


MINP_SEED = 3400


def _minp_cases():
    for V in VS:
        for B in BS:
            lg = _logits(MINP_SEED + V + B, B, V)
            for n_valid in (V, V - 2):
                for top_k in (None, 7):
                    yield V, B, n_valid, top_k, lg


def test_min_p_keeps_the_columns_with_e_at_least_min_p():
    """Kept == top-k survivors with e64 >= min_p, for rows where no column has |e64 - min_p| <= 1e-5 min_p; with
    MINP_SEED no row is exempt (asserted)."""
    min_p = 0.05
    rows = 0
    for V, B, n_valid, top_k, lg in _minp_cases():
        x = _x(lg, n_valid)
        e = _e64(x)
        assert not (np.abs(e - min_p) <= 1e-5 * min_p).any(), (V, B, n_valid)      # no row exempt
        want = _top_k_keep(x, top_k) & (e >= min_p)
        got = _run(lg, n_valid=n_valid, top_k=top_k, min_p=min_p, do_sample=True, seed=3)
        assert got["bad"] == 0
        assert np.array_equal(x >= got["thr"][:, None], want), (V, B, n_valid, top_k)
        assert np.array_equal(got["n_kept"], want.sum(1))
        assert (np.take_along_axis(want, got["ids"][:, None], 1)).all()
        rows += B
    assert rows == 8 * 2 * 6


def test_min_p_keeps_ties_and_the_maximum():
    V = 34
    lg = np.full((2, V), -3.0, dtype=np.float32)
    lg[0, [4, 21]] = 2.0                      # a tied maximum; everything else has e = exp(-5) < 0.05
    lg[1, 7] = 2.0
    lg[1, [2, 30]] = 2.0 + np.log(0.5)        # two tied columns at e = 0.5 (to rounding): both in at 0.05, out at 0.7
    got = _run(lg, min_p=0.05, do_sample=True, seed=4)
    assert list(got["n_kept"]) == [2, 3] and got["ids"][0] in (4, 21) and got["ids"][1] in (2, 7, 30)
    got = _run(lg, min_p=0.7, do_sample=True, seed=4)
    assert list(got["n_kept"]) == [2, 1] and got["ids"][1] == 7
    got = _run(lg, min_p=0.999, do_sample=False)
    assert list(got["n_kept"]) == [2, 1] and list(got["ids"]) == [4, 7] and list(got["thr"]) == [2.0, 2.0]


FILTERS = ((None, 0.0, 0.9), (7, 0.0, 0.5), (None, 0.05, 1.0), (7, 0.05, 0.99), (None, 0.0, 0.5))


def test_sampling_follows_the_f64_cdf_of_the_kept_set_with_the_kernels_own_draws():
    """Returned id j: kept, and c[j-1] - d <= u < c[j] + d on the f64 inclusive CDF c over the kernel's reported kept
    set; at most 1 % of all rows may need the slack.  logq against the same f64 probabilities within 1e-4 + d."""
    rows = loose = 0
    for V in VS:
        d = _slack(V)
        for B in BS:
            lg = _logits(3500 + V + B, B, V)
            for n_valid in (V, V - 2):
                x = _x(lg, n_valid)
                for top_k, min_p, top_p in FILTERS:
                    for step in range(8):
                        got = _run(lg, n_valid=n_valid, top_k=top_k, min_p=min_p, top_p=top_p, do_sample=True,
                                   seed=V + B, step=step)
                        assert got["bad"] == 0
                        keep = x >= got["thr"][:, None]
                        p = _mass(x, keep)
                        c = np.cumsum(p, axis=1)
                        for r in range(B):
                            j, ur = int(got["ids"][r]), float(got["u"][r])
                            what = (V, B, n_valid, top_k, min_p, top_p, step, r, j)
                            assert 0 <= j < n_valid and keep[r, j], what
                            lo = c[r, j - 1] if j > 0 else 0.0
                            assert lo - d <= ur < c[r, j] + d, (what, ur, lo, c[r, j])
                            assert abs(got["logq"][r] - np.log(p[r, j])) <= TOL + d, (what, got["logq"][r], p[r, j])
                            rows += 1
                            loose += not (lo <= ur < c[r, j])
    print(f"{loose} of {rows} rows needed the slack")
    assert loose <= 0.01 * rows


def _logp64(lg, n_valid, ids):
    z = np.asarray(lg, dtype=np.float64)[:, :n_valid]
    m = z.max(axis=1)
    lse = m + np.log(np.exp(z - m[:, None]).sum(axis=1))
    return z[np.arange(len(ids)), ids] - lse


@pytest.mark.parametrize("B", BS)
@pytest.mark.parametrize("V", VS)
def test_logp_is_the_models_own_log_probability(V, B):
    """logp = l[id] - logsumexp(l[:n_valid]) on the raw logits within 1e-4, whatever the temperature and the filters;
    logq == 0 for greedy; for one id, logp has the same bits under any temperature and filters."""
    lg = _logits(3600 + V + B, B, V)
    worst = 0.0
    for n_valid in (V, V - 2):
        for kw in (dict(do_sample=False), dict(do_sample=True, seed=5),
                   dict(do_sample=True, seed=6, inv_temperature=1.7, top_k=7, min_p=0.05, top_p=0.9),
                   dict(do_sample=True, seed=7, inv_temperature=0.5, top_p=0.5)):
            got = _run(lg, n_valid=n_valid, **kw)
            assert got["bad"] == 0
            err = np.abs(got["logp"] - _logp64(lg, n_valid, got["ids"])).max()
            worst = max(worst, err)
            assert err <= TOL, (n_valid, kw, err)
            if not kw["do_sample"]:
                assert (got["logq"] == 0.0).all()
        a = _run(lg, n_valid=n_valid, do_sample=False)
        b = _run(lg, n_valid=n_valid, do_sample=False, inv_temperature=2.0, top_k=7, min_p=0.05, top_p=0.5)
        c = _run(lg, n_valid=n_valid, do_sample=False, greedy_filters=False, top_p=0.9)
        assert np.array_equal(a["ids"], b["ids"]) and np.array_equal(a["ids"], c["ids"])      # x2 keeps the order
        assert np.array_equal(a["logp"], b["logp"]) and np.array_equal(a["logp"], c["logp"])
    print(f"V {V} B {B}: max |logp - f64| = {worst:.2e}")


def test_a_tie_across_the_mass_boundary_keeps_both_columns():
    V = 34
    lg = np.full((1, V), -20.0, dtype=np.float32)
    lg[0, 3] = 5.0
    lg[0, [10, 20]] = 4.0                     # masses 0.576, 0.212, 0.212: 0.7 is reached inside the tie
    got = _run(lg, top_p=0.7, do_sample=True, seed=8)
    assert got["n_kept"][0] == 3 and got["thr"][0] == 4.0 and got["ids"][0] in (3, 10, 20)
    seen = {int(_run(lg, top_p=0.7, do_sample=True, seed=s)["ids"][0]) for s in range(32)}
    assert seen <= {3, 10, 20} and 20 in seen
    got = _run(lg, top_p=0.5, do_sample=True, seed=8)          # the maximum alone reaches 0.5
    assert got["n_kept"][0] == 1 and got["thr"][0] == 5.0 and got["ids"][0] == 3 and got["logq"][0] == 0.0
    got = _run(lg, top_p=0.99, do_sample=True, seed=8, top_k=2)      # top-k keeps the tie as well
    assert got["n_kept"][0] == 3


def test_a_tiny_top_p_keeps_exactly_the_ties_of_the_maximum():
    for V in (34, 1030, 8194):
        lg = _logits(3700 + V, 2, V)
        lg[0, [5, V - 3]] = lg.max() + 1.0
        for top_p in (1e-6, 1e-30):
            got = _run(lg, top_p=top_p, do_sample=True, seed=9)
            x = _x(lg, V)
            assert np.array_equal(got["n_kept"], (x == x.max(1, keepdims=True)).sum(1)) and got["n_kept"][0] == 2
            assert np.array_equal(got["thr"], x.max(1))
            assert got["ids"][0] in (5, V - 3) and got["ids"][1] == x[1].argmax()


@pytest.mark.parametrize("do_sample", [False, True])
def test_a_bad_row_gives_minus_one_nan_nan_zero_and_one_count(do_sample):
    V = 514
    lg = _logits(3710, 5, V)
    lg[1, 100] = np.nan
    lg[3, :V - 2] = -np.inf
    lg[4, V - 1] = np.nan                     # an excluded column is not looked at
    got = _run(lg, n_valid=V - 2, top_p=0.9, min_p=0.01, do_sample=do_sample, seed=2)
    assert got["bad"] == 2
    for r in (1, 3):
        assert got["ids"][r] == -1 and got["n_kept"][r] == 0
        assert np.isnan(got["logp"][r]) and np.isnan(got["logq"][r]) and np.isnan(got["thr"][r])
    clean = _run(_logits(3710, 5, V), n_valid=V - 2, top_p=0.9, min_p=0.01, do_sample=do_sample, seed=2)
    for k in ("ids", "logp", "logq", "n_kept", "thr"):
        assert np.array_equal(got[k][[0, 2, 4]], clean[k][[0, 2, 4]]), k


def test_refused_arguments_launch_nothing():
    from arcweld import _native
    from arcweld import kernels as K

    def attempt(V, match, **kw):
        lg = torch.zeros(2, V, device="cuda")
        out = torch.full((2, 1), -7, dtype=torch.int64, device="cuda")
        lp = torch.full((2, 1), 7.0, device="cuda")
        bad = torch.zeros(1, dtype=torch.int32, device="cuda")
        with pytest.raises(_native.NativeError, match=match):
            K.sample_next_ex(lg, out, 0, bad, logp_out=lp, **kw)
        torch.cuda.synchronize()
        assert (out == -7).all() and (lp == 7.0).all() and int(bad.item()) == 0

    attempt(16385, "16384")
    for top_p in (0.0, -0.5, 1.5, float("nan")):
        attempt(34, "top_p", top_p=top_p)
    for min_p in (-0.1, 1.0, 2.0, float("nan")):
        attempt(34, "min_p", min_p=min_p)
    ok = _run(np.eye(2, 16384, 3, dtype=np.float32), top_p=0.9, do_sample=True)      # the largest V that is served
    assert ok["bad"] == 0 and (ok["ids"] >= 0).all()
    with pytest.raises(_native.NativeError, match="n_kept_out"):
        K.sample_next_ex(torch.zeros(2, 34, device="cuda"), torch.zeros(2, 1, dtype=torch.int64, device="cuda"), 0,
                         torch.zeros(1, dtype=torch.int32, device="cuda"), n_kept_out=torch.zeros(2, device="cuda"))


@pytest.mark.parametrize("V", VS)
def test_two_launches_of_the_same_inputs_give_the_same_bits(V):
    lg = _logits(3800 + V, 5, V)
    kw = dict(n_valid=V - 2, top_k=50 if V > 50 else 7, min_p=0.001, top_p=0.95, inv_temperature=1.3, do_sample=True,
              seed=10, step=3)
    a, b = _run(lg, **kw), _run(lg, **kw)
    for k in ("ids", "u", "logp", "logq", "n_kept", "thr"):
        assert a[k].tobytes() == b[k].tobytes(), k
