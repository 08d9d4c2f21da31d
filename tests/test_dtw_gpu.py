"""aw_dtw_knn (banded dynamic-time-warping k-NN search, csrc/dtw.hip) and what arcweld.retrieve and
probe_latent_space.py build on it, against the fp64 restatements of tests/dtw_refs.py.  Sizes come from
aw_dtw_knn_describe: below, at and above a query tile and a database tile.  The buffer discipline is test_knn_gpu.py's:
the inputs sit inside NaN-filled buffers with NaN row padding (a read outside a row's L * C values would surface as a
non-finite distance, which is never taken -- a wrong neighbour), the outputs between canaries.

Bit-exact block: integer features in -4..4 keep every value of the dynamic program an integer below 2^24, so the f32
result is exact in any evaluation order: idx must equal the fp64 (d, j) ranking and dist its bits (dtw_refs).
Random block: the same cases on Gaussian features against the derived bound eps of dtw_refs; no case is left out."""
import json

import numpy as np
import pytest
import torch

import dtw_refs as R
import knn_refs as KR
from oracle import gen

pytestmark = pytest.mark.gpu

PAD = 64
CANARY_F, CANARY_I = -1234.5, -77


@pytest.fixture(scope="module")
def tiles():
    from arcweld import kernels as K
    tq, tx = K.dtw_knn_describe()
    assert tq >= 2 and tx >= 34
    return tq, tx


def _place(a, pad=0, off=0):
    """(n, L, C) array on the device as (n, L * C) rows inside a NaN-filled buffer: rows L * C + pad floats apart, the
    first ``off`` floats (4 * off bytes) into the allocation; the padding and both margins are NaN."""
    a = np.ascontiguousarray(a, dtype=np.float32)
    n, D = a.shape[0], a.shape[1] * a.shape[2]
    ld = D + pad
    buf = torch.full((off + n * ld + PAD,), float("nan"), device="cuda")
    view = buf.as_strided((n, D), (ld, 1), off)
    if n:
        view.copy_(torch.as_tensor(a.reshape(n, D)))
    return view


def _run(q, x, radius, k, qg=None, xg=None, splits=None, q_pad=0, x_pad=0, q_off=0, x_off=0, q_dev=None, x_dev=None,
         length=None, channels=None):
    """One search; (idx, dist) as numpy after checking the output canaries."""
    from arcweld import kernels as K
    nq = len(q)
    L, C = q.shape[1:] if length is None else (length, channels)
    ibuf = torch.full((nq * k + 2 * PAD,), CANARY_I, dtype=torch.int64, device="cuda")
    dbuf = torch.full((nq * k + 2 * PAD,), CANARY_F, device="cuda")
    idx, dist = ibuf[PAD:PAD + nq * k].view(nq, k), dbuf[PAD:PAD + nq * k].view(nq, k)
    g = lambda a: None if a is None else torch.as_tensor(np.asarray(a, np.int32), device="cuda")  # noqa: E731
    qd = _place(q, q_pad, q_off) if q_dev is None else q_dev
    xd = _place(x, x_pad, x_off) if x_dev is None else x_dev
    try:
        K.dtw_knn(qd, xd, L, C, radius, k, q_group=g(qg), x_group=g(xg), splits=splits, idx=idx, dist=dist)
    finally:
        torch.cuda.synchronize()
        for buf, c in ((ibuf, CANARY_I), (dbuf, CANARY_F)):
            assert bool((buf[:PAD] == c).all() and (buf[PAD + nq * k:] == c).all()), "an output canary was written"
    return idx.cpu().numpy(), dist.cpu().numpy()


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _ints(seed, n, L, C):
    return gen.randint(seed, (n, L, C), -4, 5).astype(np.float32)


def _assert_exact(got, q, x, radius, k, qg=None, xg=None, label=""):
    idx, dist = got
    want_i, want_d = R.knn(q, x, radius, k, qg, xg)
    assert np.array_equal(idx, want_i), f"{label}: idx differs from the fp64 (d, j) ranking"
    assert np.array_equal(_bits(dist), _bits(want_d)), f"{label}: dist bits"


def _check_bounds(idx, dist, q, x, radius, k, qg=None, xg=None, label=""):
    """The conditions of a correct f32 search on arbitrary data, per query, for every pair (test_knn_gpu.py's
    _check_bounds with the DTW bound; rows with fewer than k eligible neighbours end in (-1, +inf))."""
    nq, nx = len(q), len(x)
    L, C = q.shape[1:]
    d64 = R.dtw64(q, x, radius) if nx else np.empty((nq, 0))
    e = R.eps(d64, L, C)
    ok = KR.eligible(nq, nx, qg, xg, d64)
    assert idx.shape == (nq, k) and (idx >= -1).all() and (idx < nx).all()
    worst = 0.0
    for i in range(nq):
        n = min(k, int(ok[i].sum()))
        assert (idx[i, :n] >= 0).all() and (idx[i, n:] == -1).all() and np.isposinf(dist[i, n:]).all(), \
            f"{label}: query {i} should have {n} neighbours"
        js = idx[i, :n]
        assert len(set(js)) == n, f"{label}: repeated neighbours"
        assert ok[i, js].all(), f"{label}: an ineligible neighbour"
        assert (np.diff(dist[i, :n]) >= 0).all() and (dist[i, :n] >= 0).all(), f"{label}: dist not ascending"
        err = np.abs(dist[i, :n].astype(np.float64) - d64[i, js])
        assert (err <= e[i, js]).all(), f"{label}: a stored distance is off by more than eps"
        if n:
            worst = max(worst, float((err / np.maximum(e[i, js], 1e-300)).max()))
        if n == k:
            # a row left out lost to the k-th in f32, so d64 + eps >= d64(k-th) - eps(k-th): one eps per pair
            rest = ok[i].copy()
            rest[js] = False
            nearer = rest & (d64[i] < d64[i, js[-1]] - e[i, js[-1]] - e[i])
            assert not nearer.any(), f"{label}: a nearer row was left out"
    print(f"{label}: max |dist - dtw64| / eps = {worst:.3g}")


# ------------------------------------------------------------------------------------------------ the cases
# A pairwise-covering selection of the 5 x 7 x 6 x 4 x 4 x 4 x 2 x 2 grid (positions in the value lists of _case: nq,
# nx, L, radius, C, k, row padding, base offset), built greedily: every pair of values of every two parameters meets
# in some case -- the 42 (nx, L) pairs need at least 42 cases.  test_the_selection_covers_every_pair checks it.
SELECTION = (
    (4, 2, 5, 2, 0, 3, 0, 0), (0, 4, 1, 0, 0, 2, 1, 1), (3, 1, 2, 1, 1, 1, 1, 0), (1, 5, 3, 1, 3, 0, 0, 1),
    (2, 0, 0, 3, 2, 0, 1, 0), (2, 1, 4, 0, 1, 2, 0, 1), (4, 3, 2, 0, 2, 1, 0, 1), (1, 6, 4, 2, 3, 1, 1, 0),
    (3, 6, 5, 3, 0, 0, 0, 1), (0, 2, 3, 3, 1, 3, 1, 0), (3, 2, 0, 0, 3, 3, 0, 1), (4, 4, 5, 3, 3, 2, 1, 0),
    (2, 3, 1, 2, 1, 0, 0, 0), (3, 0, 4, 2, 2, 2, 0, 1), (0, 5, 5, 1, 2, 1, 1, 1), (1, 2, 1, 1, 2, 3, 0, 1),
    (1, 3, 0, 3, 0, 1, 1, 1), (4, 5, 4, 1, 0, 2, 0, 0), (4, 0, 3, 0, 0, 0, 1, 0), (0, 1, 2, 2, 3, 0, 1, 0),
    (2, 6, 2, 3, 0, 3, 1, 1), (2, 4, 3, 2, 2, 1, 1, 1), (0, 6, 0, 1, 2, 2, 0, 0), (4, 4, 0, 2, 1, 0, 0, 0),
    (2, 0, 5, 1, 1, 1, 0, 1), (1, 6, 3, 0, 1, 2, 1, 1), (2, 5, 1, 3, 3, 1, 0, 0), (0, 3, 4, 1, 2, 3, 0, 1),
    (3, 1, 3, 3, 2, 3, 1, 1), (2, 2, 4, 3, 0, 0, 1, 1), (1, 1, 5, 0, 0, 2, 1, 0), (3, 5, 2, 2, 1, 3, 1, 0),
    (1, 4, 2, 1, 2, 3, 0, 1), (3, 3, 5, 3, 3, 2, 1, 0), (1, 0, 2, 1, 3, 3, 1, 1), (2, 2, 2, 2, 2, 2, 1, 1),
    (4, 1, 1, 1, 2, 3, 1, 0), (3, 0, 1, 0, 1, 0, 0, 1), (4, 6, 1, 1, 0, 1, 0, 1), (3, 4, 4, 3, 1, 0, 1, 1),
    (4, 5, 0, 0, 3, 0, 1, 0), (0, 0, 1, 1, 3, 1, 1, 0), (3, 2, 2, 1, 2, 1, 0, 0), (0, 1, 0, 3, 3, 1, 0, 1),
    (3, 3, 3, 0, 3, 3, 0, 0))
N_CASES = len(SELECTION)
GRID = (5, 7, 6, 4, 4, 4, 2, 2)


def _case(i, tiles):
    tq, tx = tiles
    a, b, c, d, e, f, g, h = SELECTION[i]
    k = (1, 2, 5, 32)[f]
    nq = (1, tq - 1, tq, tq + 1, 2 * tq + 2)[a]
    nx = (1, k - 1, k, tx - 1, tx, tx + 1, 2 * tx + 5)[b]
    L = (1, 2, 3, 17, 64, 65)[c]
    radius = min((0, 1, 3, L - 1)[d], L - 1)
    C = (1, 2, 3, 8)[e]
    return nq, nx, L, radius, C, k, (0, 3)[g], (0, 1)[h]


def test_the_selection_covers_every_pair():
    for a in range(8):
        for b in range(a + 1, 8):
            assert len({(c[a], c[b]) for c in SELECTION}) == GRID[a] * GRID[b], (a, b)


@pytest.mark.parametrize("i", range(N_CASES))
def test_exact_on_integer_features(tiles, i):
    nq, nx, L, radius, C, k, pad, off = _case(i, tiles)
    q, x = _ints(1000 + i, nq, L, C), _ints(2000 + i, nx, L, C)
    if nx >= 4:                                   # ties on purpose: duplicated database rows, the lower index first
        x[nx - 1] = x[0]
        x[nx // 2] = x[1]
    if nq >= 2 and nx >= 1:
        q[1] = x[0]                               # distance exactly 0
    got = _run(q, x, radius, k, q_pad=pad, x_pad=pad, q_off=off, x_off=(off + i // 8) % 2)
    _assert_exact(got, q, x, radius, k, label=f"nq={nq} nx={nx} L={L} r={radius} C={C} k={k} pad={pad} off={off}")
    if nx < k:
        assert (got[0][:, nx:] == -1).all() and np.isposinf(got[1][:, nx:]).all()


@pytest.mark.parametrize("i", range(N_CASES))
def test_random_features_within_the_derived_bound(tiles, i):
    nq, nx, L, radius, C, k, pad, off = _case(i, tiles)
    q, x = gen.normal(3000 + i, (nq, L, C)), gen.normal(4000 + i, (nx, L, C))
    idx, dist = _run(q, x, radius, k, q_pad=pad, x_pad=pad, q_off=off, x_off=(off + i // 8) % 2)
    _check_bounds(idx, dist, q, x, radius, k, label=f"nq={nq} nx={nx} L={L} r={radius} C={C} k={k}")


@pytest.mark.parametrize("k", [1, 32])
def test_every_candidate_inserts(tiles, k):
    """Distances that fall strictly with j: each database row displaces the whole current list."""
    tq, tx = tiles
    nq, nx, L, C = tq + 1, 2 * tx + 5, 5, 2
    q, x = np.zeros((nq, L, C), np.float32), np.zeros((nx, L, C), np.float32)
    x[:, 2, 1] = nx - np.arange(nx)               # a lone spike no band of radius 1 can match with anything but zeros
    got = _run(q, x, 1, k)
    _assert_exact(got, q, x, 1, k)
    assert (got[0] == np.arange(nx - 1, nx - 1 - k, -1)[None, :]).all()


# ------------------------------------------------------------------------------------------------ the limits
def test_widest_band_and_most_channels(tiles):
    """2 radius + 1 = AW_DTW_MAX_WINDOW with 8 channels: the largest LDS footprint."""
    from arcweld import _native
    radius = (_native.AW_DTW_MAX_WINDOW - 1) // 2
    L, C = radius + 1, 8
    assert (2 * L - 1) * 64 * C < 2 ** 24
    q, x = _ints(11, 2, L, C), _ints(12, 70, L, C)
    _assert_exact(_run(q, x, radius, 5, x_pad=1), q, x, radius, 5)


def test_sequences_longer_than_the_query_ring(tiles):
    """L > 512 samples: the staged query samples wrap around, under the widest band and under a narrow one."""
    from arcweld import _native
    radius = (_native.AW_DTW_MAX_WINDOW - 1) // 2
    L, C = 531, 2
    q, x = _ints(21, 1, L, C), _ints(22, 3, L, C)
    _assert_exact(_run(q, x, radius, 3), q, x, radius, 3, label="wide")
    L = _native.AW_DTW_MAX_LEN
    assert (2 * L - 1) * 64 * 3 < 2 ** 24
    q, x = _ints(23, 3, L, 3), _ints(24, 5, L, 3)
    x[3] = np.roll(q[1], 2, axis=0)               # a shifted copy: the band of radius 2 absorbs most of it
    _assert_exact(_run(q, x, 2, 2, q_pad=3, x_off=1), q, x, 2, 2, label="longest")


# ------------------------------------------------------------------------------------------------ eligibility
def test_leave_one_out_never_returns_the_row_itself(tiles):
    tq, tx = tiles
    n, L, C, radius, k = 2 * tx + 5, 9, 2, 2, 5
    x = _ints(51, n, L, C)
    xd = _place(x, 3, 0)
    g = np.arange(n)
    idx, dist = got = _run(x, x, radius, k, g, g, q_dev=xd, x_dev=xd)
    assert not (idx == g[:, None]).any() and (idx >= 0).all()
    _assert_exact(got, x, x, radius, k, g, g)
    plain = _run(x, x, radius, 1, q_dev=xd, x_dev=xd)
    assert (plain[1] == 0).all()                              # without groups every row finds itself or a duplicate
    assert (plain[0][:, 0] <= g).all()


@pytest.mark.parametrize("block", [3, 50])
def test_block_groups(tiles, block):
    tq, tx = tiles
    nq, nx, L, C, radius, k = tq + 1, 2 * tx + 5, 7, 3, 2, 5
    q, x = _ints(61, nq, L, C), _ints(62, nx, L, C)
    qg, xg = np.arange(nq) // block, np.arange(nx) // block
    idx, dist = got = _run(q, x, radius, k, qg, xg, x_pad=1)
    assert (xg[idx] != qg[:, None]).all()
    _assert_exact(got, q, x, radius, k, qg, xg)
    # a NULL on either side: no exclusion
    _assert_exact(_run(q, x, radius, k, qg, None), q, x, radius, k)
    _assert_exact(_run(q, x, radius, k, None, xg), q, x, radius, k)


def test_exclusion_leaves_fewer_than_k_rows(tiles):
    tq, tx = tiles
    nq, nx, L, C, radius, k = 5, tx + 9, 4, 1, 1, 5
    q, x = _ints(71, nq, L, C), _ints(72, nx, L, C)
    xg = np.zeros(nx, np.int64)
    xg[[7, tx + 2]] = 1                                       # two rows outside group 0
    qg = np.array([0, 0, 1, 0, 2])
    idx, dist = got = _run(q, x, radius, k, qg, xg)
    _assert_exact(got, q, x, radius, k, qg, xg)
    for i in (0, 1, 3):
        assert sorted(idx[i, :2]) == [7, tx + 2] and (idx[i, 2:] == -1).all() and np.isposinf(dist[i, 2:]).all()
    assert (idx[[2, 4]] >= 0).all()
    none = _run(q, x, radius, k, np.zeros(nq, np.int64), np.zeros(nx, np.int64))
    assert (none[0] == -1).all() and np.isposinf(none[1]).all()


def test_empty_sides(tiles):
    q = _ints(75, 3, 6, 2)
    idx, dist = _run(q, np.zeros((0, 6, 2), np.float32), 2, 4)          # nx == 0: every slot (-1, +inf)
    assert (idx == -1).all() and np.isposinf(dist).all()
    idx, dist = _run(np.zeros((0, 6, 2), np.float32), q, 2, 4)          # nq == 0: nothing to write
    assert idx.shape == (0, 4) and dist.shape == (0, 4)


def test_nan_and_inf_rows_are_never_neighbours(tiles):
    tq, tx = tiles
    nq, nx, L, C, radius, k = 9, tx + 40, 12, 2, 3, 32
    q, x = _ints(81, nq, L, C), _ints(82, nx, L, C)
    bad = {0: np.nan, 5: np.inf, 6: -np.inf, tx - 1: np.nan, tx: np.inf, nx - 1: -np.inf}
    for j, v in bad.items():
        x[j, (3 * j) % L, j % C] = v                          # anywhere in the row, the first and last samples too
    x[5, 0, 0] = np.inf
    x[6, L - 1, 1] = np.nan
    idx, dist = got = _run(q, x, radius, k)
    assert not np.isin(idx, list(bad)).any() and np.isfinite(dist).all()
    _assert_exact(got, q, x, radius, k)
    few = _run(q, x[:8], radius, k)                           # 5 finite rows only: the tail
    assert (few[0][:, 5:] == -1).all() and not np.isin(few[0], [0, 5, 6]).any()
    qn = q.copy()
    qn[2, 4, 1] = np.nan                                      # a NaN or inf query has no neighbour
    qn[3, L - 1, 0] = np.inf
    i2, d2 = _run(qn, x, radius, 3)
    assert (i2[[2, 3]] == -1).all() and np.isposinf(d2[[2, 3]]).all() and (i2[[0, 1, 4]] >= 0).all()


def test_argument_errors_launch_nothing(tiles):
    """Every AW_ERR_ARG case: a NativeError naming the argument, the outputs (between canaries, checked by _run and
    here) untouched."""
    from arcweld import _native
    from arcweld import kernels as K
    nat = _native
    L, C = 10, 2
    q, x = _ints(85, 3, L, C), _ints(86, 6, L, C)
    wide = (nat.AW_DTW_MAX_WINDOW + 1) // 2
    for match, kw in (("radius = -1", dict(radius=-1)), ("radius = 10", dict(radius=L)), ("k = 0", dict(k=0)),
                      ("k = 33", dict(k=nat.AW_KNN_MAX_K + 1)), ("splits", dict(splits=nat.AW_KNN_MAX_SPLITS + 1)),
                      ("splits", dict(splits=-1))):
        args = dict(radius=2, k=2)
        args.update(kw)
        with pytest.raises(nat.NativeError, match=match):
            _run(q, x, **args)
    big = np.zeros((1, 2 * wide, 1), np.float32)
    with pytest.raises(nat.NativeError, match="band"):
        _run(big, big, wide, 1)
    long = np.zeros((1, nat.AW_DTW_MAX_LEN + 1, 1), np.float32)
    with pytest.raises(nat.NativeError, match="len = 2001"):
        _run(long, long, 1, 1)
    nine = np.zeros((1, 4, nat.AW_DTW_MAX_C + 1), np.float32)
    with pytest.raises(nat.NativeError, match="c = 9"):
        _run(nine, nine, 1, 1)
    with pytest.raises(nat.NativeError, match="length \\* channels"):
        _run(q, x, 2, 2, length=L + 1, channels=C)
    assert nat.load().aw_dtw_knn_workspace(3, 6, 0, C, 0, 1, 0) == nat.AW_ERR_ARG        # len < 1
    assert nat.load().aw_dtw_knn_workspace(3, 6, L, 0, 0, 1, 0) == nat.AW_ERR_ARG        # c < 1
    assert nat.load().aw_dtw_knn_workspace(-1, 6, L, C, 0, 1, 0) == nat.AW_ERR_ARG
    assert nat.load().aw_dtw_knn_workspace(3, 2 ** 31, L, C, 0, 1, 0) == nat.AW_ERR_ARG

    # the raw entry point: strides, NULL operands, the workspace
    qd, xd = _place(q), _place(x)
    k = 2
    ibuf = torch.full((3 * k + 2 * PAD,), CANARY_I, dtype=torch.int64, device="cuda")
    dbuf = torch.full((3 * k + 2 * PAD,), CANARY_F, device="cuda")
    idx, dist = ibuf[PAD:PAD + 3 * k], dbuf[PAD:PAD + 3 * k]
    ws = torch.empty(nat.load().aw_dtw_knn_workspace(3, 6, L, C, 2, k, 1), dtype=torch.uint8, device="cuda")
    s = nat.stream_ptr()
    good = dict(q=K.ptr(qd), nq=3, ldq=L * C, x=K.ptr(xd), nx=6, ldx=L * C, len=L, c=C, radius=2, k=k, qg=None, xg=None,
                splits=1, ws=K.ptr(ws), ws_bytes=ws.numel(), idx=K.ptr(idx), dist=K.ptr(dist), stream=s)
    for match, kw in (("strides", dict(ldq=L * C - 1)), ("strides", dict(ldx=L * C - 1)),
                      ("strides", dict(ldx=1 << 22)), ("NULL", dict(q=None)), ("NULL", dict(idx=None)),
                      ("NULL", dict(dist=None)), ("x is NULL", dict(x=None)), ("workspace", dict(ws=None)),
                      ("workspace", dict(ws_bytes=ws.numel() - 1)), ("aligned", dict(q=K.ptr(qd) + 2))):
        with pytest.raises(nat.NativeError, match=match):
            nat.call("aw_dtw_knn", *{**good, **kw}.values())
    nat.call("aw_dtw_knn", *{**good, "nq": 0, "q": None, "idx": None, "dist": None}.values())     # nq == 0: AW_OK
    torch.cuda.synchronize()
    assert bool((ibuf == CANARY_I).all() and (dbuf == CANARY_F).all()), "a refused call wrote its outputs"
    nat.call("aw_dtw_knn", *good.values())                                                         # and the good call
    torch.cuda.synchronize()
    want_i, want_d = R.knn(q, x, 2, k)
    assert np.array_equal(idx.view(3, k).cpu().numpy(), want_i)
    assert np.array_equal(_bits(dist.view(3, k).cpu().numpy()), _bits(want_d))


# ------------------------------------------------------------------------------------------------ geometry
def test_split_counts_and_launches_give_identical_bits(tiles):
    tq, tx = tiles
    nq, nx, L, C, radius, k = tq + 1, 7 * tx + 9, 21, 2, 4, 5
    q, x = gen.normal(91, (nq, L, C)), gen.normal(92, (nx, L, C))
    x[nx - 1] = x[3]                                          # a tie across splits
    x[tx] = x[3]
    q[0] = x[3]
    ref = _run(q, x, radius, k, splits=1)
    assert list(ref[0][0, :3]) == [3, tx, nx - 1]             # equal distances: ascending index, across tiles
    assert len(set(_bits(ref[1][0, :3]))) == 1
    for sp in (2, 7, None, 1):
        got = _run(q, x, radius, k, splits=sp)
        assert np.array_equal(got[0], ref[0]) and np.array_equal(_bits(got[1]), _bits(ref[1])), f"splits={sp}"
    _check_bounds(ref[0], ref[1], q, x, radius, k, label="splits")


# ------------------------------------------------------------------------------------------------ what it is for
def _shifted_copies(seed=711, nx=48, nq=24, L=64, C=2):
    """A database of smooth sequences in sibling pairs (a row and a slightly perturbed copy) and queries that are
    copies of one row delayed by 1..3 samples, the first sample held, plus small noise.  The seed was chosen on the
    CPU with the restatements: under DTW of radius 4 every query's source row is its nearest (by a relative margin of
    0.38 at the least), under the Euclidean distance 6 of the 24 queries prefer another row."""
    t = np.arange(L, dtype=np.float64)[None, :, None, None]
    amp = gen.uniform(seed, (nx // 2, 1, C, 3), 0.5, 1.5).astype(np.float64)
    frq = gen.uniform(seed + 1, (nx // 2, 1, C, 3), 1.0, 4.0).astype(np.float64)
    phs = gen.uniform(seed + 2, (nx // 2, 1, C, 3), 0.0, 2 * np.pi).astype(np.float64)
    base = (amp * np.sin(2 * np.pi * frq * t / L + phs)).sum(-1)
    pa = gen.uniform(seed + 3, (nx // 2, 1, C), 0.1, 0.2).astype(np.float64)
    pf = gen.uniform(seed + 4, (nx // 2, 1, C), 1.0, 3.0).astype(np.float64)
    x = np.empty((nx, L, C), np.float32)
    x[0::2], x[1::2] = base, base + pa * np.sin(2 * np.pi * pf * t[..., 0] / L)
    src = gen.randint(seed + 5, (nq,), 0, nx)
    shift = gen.randint(seed + 6, (nq,), 1, 4)
    q = np.stack([x[s][np.maximum(np.arange(L) - d, 0)] for s, d in zip(src, shift)])
    return q + gen.normal(seed + 7, (nq, L, C), 0.01), x, src


def test_warping_finds_the_shifted_source_where_euclid_does_not():
    from arcweld.retrieve import dtw_search, knn_search
    q, x, src = _shifted_copies()
    ref_dtw, _ = R.knn(q, x, 4, 1)
    ref_euc, _ = KR.knn(q.reshape(len(q), -1), x.reshape(len(x), -1), 1)
    assert (ref_dtw[:, 0] == src).all() and (ref_euc[:, 0] != src).sum() >= 3           # the reference itself
    qt, xt = torch.tensor(q), torch.tensor(x)
    idx, dist = dtw_search(qt, xt, k=1, radius=4)
    assert np.array_equal(idx.cpu().numpy()[:, 0], src)
    _check_bounds(idx.cpu().numpy(), dist.cpu().numpy(), q, x, 4, 1, label="shifted copies")
    euc, _ = knn_search(qt, xt, k=1, standardize=False)
    assert np.array_equal(euc.cpu().numpy(), ref_euc) and (euc.cpu().numpy()[:, 0] != src).any()
    # radius 0 is the Euclidean search; None is the unconstrained one
    idx0, dist0 = dtw_search(qt, xt, k=3, radius=0)
    want_i, want_d = KR.knn(q.reshape(len(q), -1), x.reshape(len(x), -1), 3)
    assert np.array_equal(idx0.cpu().numpy(), want_i)
    assert np.allclose(dist0.cpu().numpy(), want_d, rtol=1e-5, atol=0)
    full, dfull = dtw_search(qt, xt, k=2, sqrt=True)
    _check_bounds(full.cpu().numpy(), dfull.cpu().numpy() ** 2, q, x, 63, 2, label="unconstrained")
    _, plain = dtw_search(qt, xt, k=2)
    assert torch.equal(dfull, plain.sqrt())


def test_search_standardizes_per_channel():
    from arcweld.retrieve import dtw_search
    q = gen.normal(95, (7, 30, 3), 2.0, 1.0) * np.array([1.0, 10.0, 0.1], np.float32)
    x = gen.normal(96, (40, 30, 3), 2.0, 1.0) * np.array([1.0, 10.0, 0.1], np.float32)
    mean, scale = R.channel_scaler(x)
    zq, zx = R.standardize(q, mean, scale), R.standardize(x, mean, scale)
    g = np.arange(7) % 3, np.arange(40) % 3
    idx, dist = dtw_search(torch.tensor(q), torch.tensor(x), k=4, radius=5, standardize=True,
                           q_group=torch.tensor(g[0]), x_group=torch.tensor(g[1]))
    _check_bounds(idx.cpu().numpy(), dist.cpu().numpy(), zq, zx, 5, 4, g[0], g[1], label="standardised")


# ------------------------------------------------------------------------------------------------ end to end
N_CYCLES, SIZES = 2, (40, 9, 11)


@pytest.fixture(scope="module")
def splits():
    return [(torch.tensor(gen.windows(500 + i, n * N_CYCLES).reshape(n, N_CYCLES * 200, 2), device="cuda"),
             torch.tensor(gen.randint(510 + i, (n,), 0, 2), device="cuda")) for i, n in enumerate(SIZES)]


def _check_result(r, feats_q, feats_x, labels_q, labels_x, radius, k, weights, qg=None, xg=None, label=""):
    idx, dist, pred = (r[n].cpu().numpy() for n in ("idx", "dist", "pred"))
    _check_bounds(idx, dist, feats_q, feats_x, radius, k, qg, xg, label=label)
    want_p, _ = KR.vote(idx, dist.astype(np.float64), labels_x, 2, weights)
    assert np.array_equal(pred, want_p)
    for name, v in KR.metrics(pred, labels_q).items():
        assert abs(r[name] - v) <= 1e-6, (label, name, r[name], v)


def test_probe_neighbours_and_metrics(splits):
    from arcweld.retrieve import latent_knn_probe
    k, radius = 3, 6
    groups = {"train": torch.arange(SIZES[0]) // 4, "val": torch.arange(SIZES[1]) // 4}
    res = latent_knn_probe(splits, N_CYCLES, k=k, dataset="asimow", weights="distance", standardize=False, loo=True,
                           groups=groups, metric="dtw", radius=radius)
    assert set(res) == {"val", "test", "train_loo"}
    feats = [x.cpu().numpy() for x, _ in splits]
    labels = [y.cpu().numpy() for _, y in splits]
    tg, vg = groups["train"].numpy(), groups["val"].numpy()
    for qi, name, qg, xg in ((1, "val", vg, tg), (2, "test", None, None), (0, "train_loo", tg, tg)):
        assert set(res[name]) == {"acc", "acc_good", "acc_bad", "f1", "idx", "dist", "pred"}
        _check_result(res[name], feats[qi], feats[0], labels[qi], labels[0], radius, k, "distance", qg, xg,
                      label=f"dtw {name}")
    assert (tg[res["train_loo"]["idx"].cpu().numpy()] != tg[:, None]).all()           # leave-one-group-out
    assert (tg[res["val"]["idx"].cpu().numpy()] != vg[:, None]).all()
    # without groups, loo leaves out the row itself
    res = latent_knn_probe(splits, N_CYCLES, k=1, dataset="asimow", standardize=False, loo=True, metric="dtw",
                           radius=radius)
    own = np.arange(SIZES[0])
    assert not (res["train_loo"]["idx"].cpu().numpy() == own[:, None]).any()
    _check_result(res["train_loo"], feats[0], feats[0], labels[0], labels[0], radius, 1, "uniform", own, own,
                  label="dtw loo")


def test_probe_standardizes_per_channel(splits):
    from arcweld.retrieve import latent_knn_probe
    radius = 6
    scaled = [(x * torch.tensor([3.0, 0.2], device=x.device) + 1.5, y) for x, y in splits]
    res = latent_knn_probe(scaled, N_CYCLES, k=1, dataset="asimow", metric="dtw", radius=radius)
    feats = [x.cpu().numpy() for x, _ in scaled]
    labels = [y.cpu().numpy() for _, y in scaled]
    mean, scale = R.channel_scaler(feats[0])
    assert mean.shape == (2,)
    z = [R.standardize(f, mean, scale) for f in feats]
    for qi, name in ((1, "val"), (2, "test")):
        _check_result(res[name], z[qi], z[0], labels[qi], labels[0], radius, 1, "uniform", label=f"scaled {name}")


def test_script_writes_both_files(tmp_path):
    import probe_latent_space as pls
    out, nb = tmp_path / "probe.json", tmp_path / "nb.npz"
    common = ["--vqvae-model", str(tmp_path / "none.ckpt"), "--dataset", "asimow", "--n-cycles", str(N_CYCLES), "--k",
              "3", "--loo", "--n-train", "24", "--n-val", "5", "--n-test", "6", "--seed", "3", "--out", str(out)]
    pls.main(pls.parser().parse_args(common + ["--metric", "dtw", "--band", "0.05", "--neighbours-out", str(nb)]))
    summary = json.loads(out.read_text())
    base = {"val", "test", "train_loo", "k", "weights", "dataset", "standardize", "n_cycles"}
    assert set(summary) == base | {"metric", "band", "radius"}
    assert summary["metric"] == "dtw" and summary["band"] == 0.05 and summary["radius"] == 20
    assert summary["k"] == 3 and summary["dataset"] == "asimow" and summary["standardize"] is True
    for name in ("val", "test", "train_loo"):
        assert set(summary[name]) == {"acc", "acc_good", "acc_bad", "f1"}
        assert all(0.0 <= v <= 1.0 for v in summary[name].values())
    with np.load(nb, allow_pickle=False) as f:
        assert set(f.files) == {f"{s}_{key}" for s in ("val", "test", "train_loo") for key in ("idx", "dist", "pred")}
        for s, n in (("val", 5), ("test", 6), ("train_loo", 24)):
            assert f[f"{s}_idx"].shape == (n, 3) and f[f"{s}_idx"].dtype == np.int64
            assert f[f"{s}_dist"].shape == (n, 3) and f[f"{s}_dist"].dtype == np.float32
            assert np.isfinite(f[f"{s}_dist"]).all() and (f[f"{s}_idx"] >= 0).all()
            assert f[f"{s}_pred"].shape == (n,) and set(np.unique(f[f"{s}_pred"])) <= {0, 1}
        assert not (f["train_loo_idx"] == np.arange(24)[:, None]).any()
    # the default metric: the key set is what it was
    pls.main(pls.parser().parse_args(common))
    assert set(json.loads(out.read_text())) == base
