"""CPU checks of the DTW restatements (tests/dtw_refs.py) that the GPU tests of aw_dtw_knn lean on, of the argument
errors of arcweld.retrieve.dtw_search / latent_knn_probe(metric="dtw") -- raised before any device work, so CPU tensors
trigger them -- and of probe_latent_space.py's --metric / --band handling."""
import numpy as np
import pytest
import torch

import dtw_refs as R
import knn_refs as KR
from oracle import gen


def _ints(seed, n, L, C):
    return gen.randint(seed, (n, L, C), -4, 5).astype(np.float32)


# ------------------------------------------------------------------------------------------------ the restatements
def test_radius_zero_is_the_squared_euclidean_distance():
    q, x = gen.normal(1, (5, 17, 3)), gen.normal(2, (7, 17, 3))
    want = KR.sqdist64(q.reshape(5, -1), x.reshape(7, -1))
    assert np.allclose(R.dtw64(q, x, 0), want, rtol=1e-13, atol=0)


def test_hand_computed_example():
    """q = (0, 1, 3), x = (1, 1, 0), one channel.  cost[i][j] = (q_i - x_j)^2:
         1 1 0        unconstrained D:  1 2 2        radius 1 (cells (0, 2) and (2, 0) absent):  1 2 .
         0 0 1                          1 1 2                                                    1 1 2
         4 4 9                          5 5 10                                                   . 5 10
    and radius 0 is the diagonal: 1 + 0 + 9."""
    q = np.array([[[0.0], [1.0], [3.0]]], np.float32)
    x = np.array([[[1.0], [1.0], [0.0]]], np.float32)
    for radius, want in ((2, 10.0), (1, 10.0), (0, 10.0)):
        assert R.dtw64(q, x, radius)[0, 0] == want
        for order in R.ORDERS:
            assert R.dtw32(q, x, radius, order)[0, 0] == want
    # a pair on which the band matters: a spike two samples late costs nothing once the band reaches it
    a = np.array([[[0.0], [5.0], [0.0], [0.0], [0.0]]], np.float32)
    b = np.array([[[0.0], [0.0], [0.0], [5.0], [0.0]]], np.float32)
    # (radius 1: each spike still meets only zeros, 25 each)
    assert [R.dtw64(a, b, r)[0, 0] for r in (0, 1, 2, 4)] == [50.0, 50.0, 0.0, 0.0]


def test_symmetry_and_band_monotonicity():
    q, x = gen.normal(3, (6, 19, 2)), gen.normal(4, (6, 19, 2))
    prev = None
    for radius in (0, 1, 2, 5, 18):
        d = R.dtw64(q, x, radius)
        assert np.array_equal(d, R.dtw64(x, q, radius).T)
        self_d = R.dtw64(q, q, radius)
        assert np.array_equal(self_d, self_d.T) and (np.diag(self_d) == 0).all()
        if prev is not None:
            assert (d <= prev).all()                   # a wider band only adds paths
        prev = d
    assert (prev >= 0).all()


@pytest.mark.parametrize("L, C, radius", [(1, 1, 0), (2, 8, 1), (3, 2, 1), (17, 3, 3), (33, 1, 32), (40, 8, 7)])
def test_f32_evaluations_in_three_orders_stay_within_the_bound(L, C, radius):
    q, x = gen.normal(10 + L, (9, L, C)), gen.normal(20 + L, (11, L, C))
    d64 = R.dtw64(q, x, radius)
    e = R.eps(d64, L, C)
    worst = 0.0
    for order in R.ORDERS:
        err = np.abs(R.dtw32(q, x, radius, order).astype(np.float64) - d64)
        assert (err <= e).all(), order
        worst = max(worst, float((err / e).max()))
    print(f"L={L} C={C} r={radius}: worst |dtw32 - dtw64| / eps = {worst:.3g}")


@pytest.mark.parametrize("L, C, radius", [(1, 8, 0), (17, 3, 3), (65, 8, 64), (64, 2, 1)])
def test_integer_features_are_exact_in_every_order(L, C, radius):
    assert (2 * L - 1) * 64 * C < 2 ** 24
    q, x = _ints(30 + L, 4, L, C), _ints(40 + L, 6, L, C)
    d64 = R.dtw64(q, x, radius)
    assert (d64 == np.round(d64)).all()
    for order in R.ORDERS:
        assert np.array_equal(R.dtw32(q, x, radius, order).astype(np.float64), d64), order


def test_ranking_reuses_the_knn_rules():
    q, x = _ints(51, 3, 5, 2), _ints(52, 9, 5, 2)
    x[7] = x[2]                                        # a tie: the lower index first
    idx, dist = R.knn(q, x, 1, 4)
    d = R.dtw64(q, x, 1)
    for i in range(3):
        order = sorted(range(9), key=lambda j: (d[i, j], j))[:4]
        assert list(idx[i]) == order and list(dist[i]) == [d[i, j] for j in order]
    idx, dist = R.knn(q, x, 1, 4, np.zeros(3, int), (np.arange(9) > 1).astype(int))
    assert (idx[:, :2] >= 2).all() and (idx[:, 2:] >= 2).all()
    idx, dist = R.knn(q, x[:2], 0, 4)
    assert (idx[:, 2:] == -1).all() and np.isposinf(dist[:, 2:]).all()


def test_channel_scaler():
    x = gen.normal(61, (7, 11, 3), 2.0, 1.5)
    mean, scale = R.channel_scaler(x)
    assert mean.shape == (3,) and np.allclose(mean, x.reshape(-1, 3).astype(np.float64).mean(0))
    z = R.standardize(x, mean, scale)
    assert z.shape == x.shape and z.dtype == np.float32
    assert np.allclose(z.reshape(-1, 3).mean(0), 0, atol=1e-6) and np.allclose(z.reshape(-1, 3).std(0), 1, atol=1e-6)


# ------------------------------------------------------------------------------------------------ argument errors
def test_dtw_search_argument_errors_need_no_device():
    from arcweld.retrieve import MAX_DTW_CHANNELS, MAX_DTW_LEN, MAX_DTW_WINDOW, MAX_K, dtw_search
    assert MAX_DTW_LEN >= 2000 and MAX_DTW_WINDOW >= 401 and MAX_DTW_CHANNELS == 8
    q, x = torch.zeros(3, 10, 2), torch.zeros(5, 10, 2)
    wide = (MAX_DTW_WINDOW + 1) // 2                   # the first radius whose band is too wide
    cases = [
        ("queries", dict(queries=[[1.0]])),
        ("queries", dict(queries=torch.zeros(3, 20))),
        ("queries", dict(queries=torch.zeros(3, 10, 2, dtype=torch.int64))),
        ("database", dict(database=torch.zeros(5, 10, 2, 1))),
        ("database", dict(database=torch.zeros(5, 9, 2))),
        ("database", dict(database=torch.zeros(5, 10, 3))),
        ("queries", dict(queries=torch.zeros(1, MAX_DTW_LEN + 1, 1), database=torch.zeros(1, MAX_DTW_LEN + 1, 1))),
        ("queries", dict(queries=torch.zeros(1, 0, 1), database=torch.zeros(1, 0, 1))),
        ("queries", dict(queries=torch.zeros(1, 4, 9), database=torch.zeros(1, 4, 9))),
        ("queries", dict(queries=torch.zeros(1, 4, 0), database=torch.zeros(1, 4, 0))),
        ("k", dict(k=0)), ("k", dict(k=MAX_K + 1)), ("k", dict(k=True)), ("k", dict(k=1.0)),
        ("radius", dict(radius=-1)), ("radius", dict(radius=10)), ("radius", dict(radius=1.0)),
        ("radius", dict(radius=True)),
        ("radius", dict(queries=torch.zeros(1, 2 * wide, 1), database=torch.zeros(1, 2 * wide, 1), radius=wide)),
        ("radius", dict(queries=torch.zeros(1, 2 * wide, 1), database=torch.zeros(1, 2 * wide, 1))),   # None: L - 1
        ("standardize", dict(standardize=1)), ("sqrt", dict(sqrt="yes")),
        ("q_group", dict(q_group=torch.zeros(4, dtype=torch.long), x_group=torch.zeros(5, dtype=torch.long))),
        ("x_group", dict(q_group=torch.zeros(3, dtype=torch.long), x_group=torch.zeros(5))),
    ]
    for name, kw in cases:
        args = dict(queries=q, database=x)
        args.update(kw)
        with pytest.raises(ValueError, match=name):
            dtw_search(**args)


def test_probe_argument_errors_need_no_device():
    from arcweld.retrieve import MAX_DTW_WINDOW, latent_knn_probe
    y = lambda n: torch.zeros(n, dtype=torch.long)  # noqa: E731
    splits = [(torch.zeros(n, 400, 2), y(n)) for n in (6, 2, 2)]
    with pytest.raises(ValueError, match="latent_vq_vae.*not time series"):
        latent_knn_probe(splits, 2, metric="dtw", dataset="latent_vq_vae", vqvae=object())
    with pytest.raises(ValueError, match="latent_vq_vae"):
        latent_knn_probe(splits, 2, metric="dtw")                          # the default dataset
    with pytest.raises(ValueError, match="metric"):
        latent_knn_probe(splits, 2, metric="cosine", dataset="asimow")
    with pytest.raises(ValueError, match="radius"):
        latent_knn_probe(splits, 2, dataset="asimow", radius=3)            # radius without the dtw metric
    for radius in (-1, 400, 2.0, (MAX_DTW_WINDOW + 1) // 2):
        with pytest.raises(ValueError, match="radius"):
            latent_knn_probe(splits, 2, metric="dtw", dataset="asimow", radius=radius)
    with pytest.raises(ValueError, match="radius"):                        # None is L - 1 = 399: too wide a band
        latent_knn_probe(splits, 2, metric="dtw", dataset="asimow")
    nine = [(torch.zeros(n, 400, 9), y(n)) for n in (6, 2, 2)]
    with pytest.raises(ValueError, match="channels"):
        latent_knn_probe(nine, 2, metric="dtw", dataset="asimow", radius=3)
    long = [(torch.zeros(n, 2200, 2), y(n)) for n in (6, 2, 2)]
    with pytest.raises(ValueError, match="length"):
        latent_knn_probe(long, 11, metric="dtw", dataset="asimow", radius=3)


# ------------------------------------------------------------------------------------------------ the script
def _args(*extra):
    import probe_latent_space as pls
    return pls, pls.parser().parse_args(["--vqvae-model", "/nonexistent/v.ckpt", *extra])


def test_script_defaults():
    pls, a = _args()
    assert a.metric == "euclidean" and a.band is None and pls.DEFAULT_BAND == 0.1
    assert pls.resolve_dtw(a) == {}
    _, a = _args("--metric", "dtw", "--dataset", "asimow")
    assert pls.resolve_dtw(a) == {"metric": "dtw", "band": 0.1, "radius": 100}         # n_cycles 5: L = 1000
    _, a = _args("--metric", "dtw", "--dataset", "asimow", "--band", "0.05", "--n-cycles", "2")
    assert pls.resolve_dtw(a) == {"metric": "dtw", "band": 0.05, "radius": 20}
    _, a = _args("--metric", "dtw", "--dataset", "asimow", "--band", "1", "--n-cycles", "1")
    assert pls.resolve_dtw(a)["radius"] == 199                                         # min(L - 1, floor(F L))
    _, a = _args("--metric", "dtw", "--dataset", "asimow", "--band", "0", "--n-cycles", "1")
    assert pls.resolve_dtw(a)["radius"] == 0


@pytest.mark.parametrize("extra, message", [
    (("--protocol", "linear", "--metric", "dtw", "--dataset", "asimow"), "--protocol knn"),
    (("--protocol", "svm", "--band", "0.2", "--dataset", "asimow"), "--protocol knn"),
    (("--protocol", "linear", "--band", "0.1"), "--protocol knn"),
    (("--metric", "dtw"), "--dataset asimow"),                                         # the default dataset
    (("--metric", "dtw", "--dataset", "latent_vq_vae"), "--dataset asimow"),
    (("--band", "0.2", "--dataset", "asimow"), "--metric dtw"),
    (("--metric", "dtw", "--dataset", "asimow", "--band", "1.5"), "--band must lie in 0..1"),
    (("--metric", "dtw", "--dataset", "asimow", "--band", "-0.1"), "--band must lie in 0..1"),
    (("--metric", "dtw", "--dataset", "asimow", "--band", "nan"), "--band must lie in 0..1"),
    (("--metric", "dtw", "--dataset", "asimow", "--n-cycles", "11"), "at most 2000 samples"),
    (("--metric", "dtw", "--dataset", "asimow", "--band", "0.5"), "radius of 500"),
])
def test_script_refuses(extra, message):
    pls, a = _args(*extra)
    with pytest.raises(SystemExit) as e:
        pls.main(a)
    assert message in str(e.value), str(e.value)


def test_script_rejects_an_unknown_metric():
    import probe_latent_space as pls
    with pytest.raises(SystemExit):
        pls.parser().parse_args(["--metric", "cosine"])
