"""CPU checks of tests/vq_refs.py, the instrument of tests/test_vq_kernels_gpu.py: the derived bounds against an f32
evaluation of the reference expression (torch, oracle.vqvae.vq_quantize), the exactness of the integer block, and
mutation checks -- every checker must reject the wrong answers a subtly broken kernel would give."""
import numpy as np
import pytest
import torch

import vq_refs as R
from oracle import vqvae as ov

# the exact cases the CPU looks at: one per kernel regime of the GPU test (pinned ragged, pinned full, one code in the
# second tile, three tiles, D = 256 over 17 tiles) and the smallest codebooks
EXACT = ((3, 32, 63), (7, 128, 5), (100, 16, 65), (512, 64, 64), (513, 32, 33), (1030, 64, 100), (8197, 256, 20))


def _d32(z, E):
    """The reference's distance expression (model/vector_quantizer.py, oracle.vqvae.vq_quantize) in torch f32."""
    zf, Et = torch.tensor(z), torch.tensor(E)
    return ((zf ** 2).sum(1, keepdim=True) + (Et ** 2).sum(1) - 2 * zf @ Et.t()).numpy()


@pytest.fixture(scope="module")
def regimes():
    return [(r, R.random_case(400 + 10 * i, *r)) for i, r in enumerate(R.REGIMES)]


def test_f32_reference_stays_inside_eps_and_passes_the_checker(regimes):
    for r, (z, E) in regimes:
        err = np.abs(_d32(z, E).astype(np.float64) - R.dist64(z, E))
        ratio = float((err / R.eps(z, E)).max())
        print(f"{r}: max |d32 - d64| / eps = {ratio:.3g}")
        assert ratio < 1.0
        _, _, _, idx, _ = ov.vq_quantize(torch.tensor(z), torch.tensor(E), 0.25)
        R.check_indices(z, E, idx.numpy(), label=str(r))


def test_checker_rejects_the_runner_up_and_a_lost_last_code(regimes):
    for r, (z, E) in regimes:
        N, K = len(z), len(E)
        frac = R.index_violations(z, E, R.second_best(z, E)).size / N
        print(f"{r}: the runner-up is rejected on {100 * frac:.1f} % of the rows")
        assert frac >= 0.90
        best = R.dist64(z, E).argmin(1)
        assert best[N - 1] == K - 1 and best[0] == 0                 # the planted rows
        lost = R.dist64(z, E[:K - 1]).argmin(1)                      # a search that never sees code K - 1
        assert (N - 1) in R.index_violations(z, E, lost)
        shifted = R.dist64(z, E[1:]).argmin(1) + 1                   # ... or code 0
        assert 0 in R.index_violations(z, E, shifted)
        for wrong in (-1, K):                                        # an unwritten or out-of-range index
            idx = best.copy()
            idx[N // 2] = wrong
            assert list(R.index_violations(z, E, idx)) == [N // 2]


@pytest.mark.parametrize("K, D, N", EXACT)
def test_exact_block_is_exact_and_tied_everywhere(K, D, N):
    c = R.exact_case(7, K, D, N)
    d64 = R.dist64(c.z, c.E)
    assert np.array_equal(_d32(c.z, c.E).astype(np.float64), d64)     # bitwise: every f32 distance is the integer
    assert d64.max() < 2 ** 24 and np.array_equal(d64, np.rint(d64))
    ties = (d64 == d64.min(1, keepdims=True)).sum(1)
    lone = c.last is not None and N >= 4           # z row 1: the unique winner at the last code, by design
    assert (np.delete(ties, 1 if lone else []) >= 2).all(), f"rows without a tie: {np.flatnonzero(ties < 2)[:8]}"
    assert (c.last is not None) == (K >= 8)
    if lone:
        assert ties[1] == 1 and c.idx[1] == K - 1 and d64[1, K - 1] == 0
    # the hand-placed rows: z row 0 is at distance 0 from every copy of s, the first wins; the zero row likewise
    assert c.idx[0] == c.base and d64[0, c.idx[0]] == 0
    assert set(np.flatnonzero(d64[0] == 0)) >= set(c.copies)           # (K = 3: the one free code holds s as well)
    assert {k - c.base for k in c.copies} == {0} | {o for o in R.OFFSETS if c.base + o < K}
    if c.zeros:
        assert c.idx[N - 1] == c.zeros[0] and set(np.flatnonzero(d64[N - 1] == 0)) == set(c.zeros)
    # ties sit at many index distances, not only the hand-placed ones
    if K >= 64:
        gaps = {int(b - a) for row in (d64 == d64.min(1, keepdims=True)) for a, b in
                zip(np.flatnonzero(row)[:-1], np.flatnonzero(row)[1:])}
        assert len(gaps) >= 8
    R.check_exact(c, c.idx, c.zq, c.counts, c.sqerr)
    R.check_indices(c.z, c.E, c.idx)


def test_offsets_all_occur_at_the_sizes_of_the_gpu_block():
    for K, want in ((1, ()), (3, (1,)), (7, (1, 4)), (64, (1, 4, 8, 32)), (100, (1, 4, 8, 32, 64)), (513, R.OFFSETS[:5]),
                    (1030, R.OFFSETS)):
        c = R.exact_case(3, K, 16, 4)
        assert tuple(k - c.base for k in c.copies[1:]) == tuple(want), K
        assert bool(c.zeros) == (K >= 8) == (c.last is not None)


def test_exact_checker_rejects_wrong_answers():
    c = R.exact_case(11, 520, 16, 70)
    d64 = R.dist64(c.z, c.E)
    R.check_exact(c, c.idx, c.zq, c.counts, c.sqerr)
    R.check_exact(c, c.idx, c.zq, np.concatenate([c.counts * 0, c.counts, c.counts * 0]), c.sqerr)   # partial histograms

    def rejected(**kw):
        out = dict(idx=c.idx, zq=c.zq, counts=c.counts, sqerr=c.sqerr)
        out.update(kw)
        with pytest.raises(AssertionError):
            R.check_exact(c, **out)

    last = d64.shape[1] - 1 - (d64 == d64.min(1, keepdims=True))[:, ::-1].argmax(1)      # last index of the minimum
    assert (np.delete(last != c.idx, 1)).all() and last[0] == c.copies[-1]      # (row 1 has the one unique winner)
    rejected(idx=last)                                                # last index wins: same z_q, counts differ too
    rejected(idx=last, counts=np.bincount(last, minlength=c.K).astype(np.float32))
    assert c.idx[1] == c.K - 1
    rejected(idx=R.dist64(c.z, c.E[:-1]).argmin(1))                   # the last code (its whole code tile) dropped
    one = c.idx.copy()
    one[0] = c.copies[1]                                              # a single tie broken the wrong way
    rejected(idx=one)
    off = c.counts.copy()
    off[c.idx[3]] += 1                                                # counts off by one
    rejected(counts=off)
    # the last row dropped: never written (the buffers' fill shows), never counted
    idx, zq, counts = c.idx.copy(), c.zq.copy(), c.counts.copy()
    idx[-1], zq[-1] = -77, -1024.0
    counts[c.idx[-1]] -= 1
    rejected(idx=idx)
    rejected(zq=zq)
    rejected(counts=counts)
    rejected(sqerr=c.sqerr - d64[-2, c.idx[-2]])                       # (row N - 1 is the zero row: row N - 2's share)
    # the last row duplicated: row N - 1 counted twice (the write to row N lands in the canary margin)
    counts = c.counts.copy()
    counts[c.idx[-1]] += 1
    rejected(counts=counts)
    rejected(sqerr=c.sqerr + d64[-2, c.idx[-2]])
    bad = c.zq.copy()
    bad[5, 3] = -bad[5, 3] if bad[5, 3] else -0.0                      # one sign bit
    rejected(zq=bad)


# ------------------------------------------------------------------------------------------------ finalize
def test_perplexity_allowance_holds_for_the_f32_restatement():
    worst = 0.0
    for kind, K, N, groups in R.FINALIZE:
        c = R.finalize_counts(kind, K, N, groups)
        _, want = R.finalize_ref(c, 0.0, N, K, 16, 0.25)
        got = R.perplexity32(c, N, K, groups)
        ratio = abs(got - want) / R.perplexity_tol(c, N, K)
        print(f"{kind} K={K} N={N} groups={groups}: perplexity {want:.6g}, |f32 - f64| / allowance = {ratio:.3g}")
        worst = max(worst, ratio)
        assert ratio < 1.0
        if kind == "one code":
            assert abs(want - 1.0) < 1e-6
        if kind == "all equal":
            assert abs(want - K) < 1e-5 * K
    # torch's f32 evaluation of the reference expression is inside the same allowance
    c = R.finalize_counts("random", 520, 1000, 1)
    p = torch.tensor(c) / 1000
    ref = float(torch.exp(-torch.sum(p * torch.log(p + 1e-10))))
    assert abs(ref - R.finalize_ref(c, 0.0, 1000, 520, 16, 0.25)[1]) <= R.perplexity_tol(c, 1000, 520)
    print(f"worst ratio {worst:.3g}")


def test_finalize_ref_matches_the_oracle():
    z, E = R.random_case(77, 100, 32, 300, 1.0, 1.0)
    loss, _, perp, idx, counts = ov.vq_quantize(torch.tensor(z, dtype=torch.float64), torch.tensor(E, dtype=torch.float64),
                                                0.25)
    want = R.finalize_ref(counts.numpy(), R.sqerr64(z, E, idx.numpy()), 300, 100, 32, 0.25)
    assert abs(want[0] - float(loss)) <= 1e-12 * float(loss) and abs(want[1] - float(perp)) <= 1e-12 * float(perp)


# ------------------------------------------------------------------------------------------------ backward, one-hot
def _backward32(z, E, idx, g_zq, g_loss, beta, prior):
    """The kernel's expressions in f32 numpy, the code sums taken row by row."""
    f = np.float32
    N, D = z.shape
    g = f(0.0) if g_loss is None else f(g_loss)
    scale = f(2.0) / f(float(N) * float(D))
    diff = (E[idx] - z).astype(f)
    dz = ((f(0.0) if g_zq is None else g_zq) - (f(g * scale) * diff).astype(f)).astype(f)
    dE = prior.copy()
    if g != 0:
        t = (f(f(g * f(beta)) * scale) * diff).astype(f)
        for n in range(N):
            dE[idx[n]] = (dE[idx[n]] + t[n]).astype(f)
    return dz, dE


@pytest.mark.parametrize("K, D, N, one_code", [(3, 5, 7, False), (64, 16, 1000, False), (64, 16, 1000, True)])
def test_backward_allowances_hold_and_reject_an_overwritten_prior(K, D, N, one_code):
    from oracle import gen
    z, E = gen.normal(31, (N, D), 0.5), gen.uniform(32, (K, D), -0.5, 0.5)
    idx = np.full(N, K - 1) if one_code else gen.randint(33, (N,), 0, K)
    g_zq, prior = gen.normal(34, (N, D), 1.0), gen.normal(35, (K, D), 0.01)
    for gz, gl in ((g_zq, -0.5), (None, 2.0), (g_zq, None)):
        dz, dE = _backward32(z, E, idx, gz, gl, 0.25, prior)
        R.check_backward(z, E, idx, gz, gl, 0.25, prior, dz, dE, label=f"K={K} N={N} g_loss={gl}")
    dz, dE = _backward32(z, E, idx, g_zq, 2.0, 0.25, prior)
    for wrong_dz, wrong_dE in ((dz, _backward32(z, E, idx, g_zq, 2.0, 0.25, np.zeros_like(prior))[1]),   # overwrote
                               (dz, prior), (g_zq, dE), (dz, dE + np.float32(1e-5) * (np.arange(K)[:, None] == idx[0]))):
        with pytest.raises(AssertionError):
            R.check_backward(z, E, idx, g_zq, 2.0, 0.25, prior, wrong_dz, wrong_dE)
    with pytest.raises(AssertionError):                               # no loss gradient: dE must stay the prior's bits
        R.check_backward(z, E, idx, g_zq, None, 0.25, prior, _backward32(z, E, idx, g_zq, None, 0.25, prior)[0],
                         prior + np.float32(1e-9))


def test_onehot_ref():
    oh = R.onehot_ref(np.array([2, 0, 2]), 3)
    assert oh.dtype == np.float32 and oh.tolist() == [[0, 0, 1], [1, 0, 0], [0, 0, 1]]
