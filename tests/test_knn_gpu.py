"""aw_knn (fused squared-distance + top-k search, csrc/knn.hip) and the probe built on it (arcweld.retrieve,
probe_latent_space.py) against the fp64 restatements of tests/knn_refs.py.  Sizes come from aw_knn_describe: below, at
and above a query tile, a database tile and a D chunk.  Every buffer the kernel touches sits between canary margins:
the inputs inside NaN-filled buffers with NaN row padding (a read outside a row's D values would surface as a NaN
distance, which is never taken -- a wrong neighbour), the outputs between canaries.

Bit-exact block: integer features in -4..4 at D <= 512 make every product and partial sum an integer below 2^24, so
the f32 distance is exact under any summation order: idx must equal the fp64 (d, j) ranking and dist its bits.
Random block: the bound eps of knn_refs (derived there, checked against an f32 evaluation on the CPU in
tests/test_knn_refs_cpu.py) on every pair; no case is left out."""
import json

import numpy as np
import pytest
import torch

import knn_refs as R
from oracle import gen
from oracle import vqvae as ov

pytestmark = pytest.mark.gpu

PAD = 64
CANARY_F, CANARY_I = -1234.5, -77


@pytest.fixture(scope="module")
def tiles():
    from arcweld import kernels as K
    tq, tx, cd, mk = K.knn_describe()
    assert mk == 32 and tq >= 2 and tx >= 34 and cd >= 2
    return tq, tx, cd


def _place(a, pad=0, off=0):
    """(n, D) array on the device inside a NaN-filled buffer: rows D + pad floats apart, the first ``off`` floats
    (4 * off bytes) into the allocation; the padding and both margins are NaN."""
    a = np.ascontiguousarray(a, dtype=np.float32)
    n, D = a.shape
    ld = D + pad
    buf = torch.full((off + n * ld + PAD,), float("nan"), device="cuda")
    view = buf.as_strided((n, D), (ld, 1), off)
    if n:
        view.copy_(torch.as_tensor(a))
    assert view.data_ptr() % 16 == (4 * off) % 16
    return view


def _run(q, x, k, qg=None, xg=None, splits=None, q_pad=0, x_pad=0, q_off=0, x_off=0, q_dev=None, x_dev=None):
    """One search; (idx, dist) as numpy after checking the output canaries."""
    from arcweld import kernels as K
    nq = len(q)
    ibuf = torch.full((nq * k + 2 * PAD,), CANARY_I, dtype=torch.int64, device="cuda")
    dbuf = torch.full((nq * k + 2 * PAD,), CANARY_F, device="cuda")
    idx, dist = ibuf[PAD:PAD + nq * k].view(nq, k), dbuf[PAD:PAD + nq * k].view(nq, k)
    g = lambda a: None if a is None else torch.as_tensor(np.asarray(a, np.int32), device="cuda")  # noqa: E731
    qd = _place(q, q_pad, q_off) if q_dev is None else q_dev
    xd = _place(x, x_pad, x_off) if x_dev is None else x_dev
    K.knn(qd, xd, k, q_group=g(qg), x_group=g(xg), splits=splits, idx=idx, dist=dist)
    torch.cuda.synchronize()
    for buf, c in ((ibuf, CANARY_I), (dbuf, CANARY_F)):
        assert bool((buf[:PAD] == c).all() and (buf[PAD + nq * k:] == c).all()), "an output canary was written"
    return idx.cpu().numpy(), dist.cpu().numpy()


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _ints(seed, n, D):
    return gen.randint(seed, (n, D), -4, 5).astype(np.float32)


def _assert_exact(got, q, x, k, qg=None, xg=None, label=""):
    idx, dist = got
    want_i, want_d = R.knn(q, x, k, qg, xg)
    assert np.array_equal(idx, want_i), f"{label}: idx differs from the fp64 (d, j) ranking"
    assert np.array_equal(_bits(dist), _bits(want_d)), f"{label}: dist bits"


# ------------------------------------------------------------------------------------------------ bit-exact block
# A pairwise-covering selection of the 5 x 7 x 7 x 4 x 2 x 2 grid (positions in the value lists of _case: nq, nx, D,
# k, row padding, base offset), built greedily: every pair of values of every two parameters meets in some case -- the
# 49 (nx, D) pairs need at least 49 cases.  test_the_selection_covers_every_pair checks it.
SELECTION = (
    (0, 0, 0, 0, 0, 0), (0, 1, 1, 1, 1, 1), (1, 2, 2, 2, 0, 1), (1, 3, 3, 3, 1, 0), (2, 4, 4, 0, 1, 1),
    (2, 5, 5, 1, 0, 0), (3, 6, 6, 2, 1, 0), (4, 0, 5, 3, 1, 1), (3, 1, 4, 3, 0, 0), (4, 4, 1, 2, 0, 0),
    (3, 2, 0, 1, 1, 1), (4, 3, 6, 0, 0, 1), (4, 6, 3, 1, 0, 1), (0, 5, 2, 3, 1, 0), (1, 5, 1, 0, 0, 1),
    (2, 2, 1, 3, 0, 0), (0, 3, 4, 2, 0, 0), (1, 0, 4, 1, 0, 0), (2, 0, 3, 2, 0, 0), (0, 2, 3, 0, 0, 0),
    (0, 4, 6, 1, 0, 0), (0, 6, 5, 0, 0, 0), (1, 1, 0, 2, 0, 0), (2, 1, 2, 0, 0, 0), (2, 6, 0, 3, 0, 0),
    (3, 3, 2, 1, 0, 0), (1, 4, 5, 2, 0, 0), (3, 0, 1, 0, 0, 0), (3, 4, 3, 3, 0, 0), (4, 5, 0, 2, 0, 0),
    (1, 0, 6, 3, 0, 0), (4, 2, 4, 0, 0, 0), (1, 6, 1, 0, 0, 0), (2, 1, 6, 1, 0, 1), (2, 3, 0, 2, 1, 1),
    (3, 1, 5, 3, 1, 1), (3, 5, 3, 0, 0, 0), (4, 0, 2, 1, 0, 0), (4, 1, 3, 2, 1, 0), (4, 2, 5, 3, 1, 1),
    (0, 2, 6, 0, 0, 1), (1, 3, 1, 1, 0, 1), (2, 3, 5, 2, 1, 0), (3, 4, 0, 3, 1, 0), (4, 4, 2, 0, 0, 0),
    (0, 5, 4, 1, 0, 1), (1, 5, 6, 2, 1, 1), (2, 6, 2, 3, 1, 1), (3, 6, 4, 0, 0, 0))
N_CASES = len(SELECTION)
GRID = (5, 7, 7, 4, 2, 2)


def _case(i, tiles):
    tq, tx, cd = tiles
    a, b, c, d, e, f = SELECTION[i]
    k = (1, 2, 5, 32)[d]
    nq = (1, tq - 1, tq, tq + 1, 2 * tq + 2)[a]
    nx = (1, k - 1, k, tx - 1, tx, tx + 1, 2 * tx + 76)[b]
    D = (1, 3, 4, cd - 1, cd, cd + 1, 257)[c]
    return nq, nx, D, k, (0, 3)[e], (0, 1)[f]


def test_the_selection_covers_every_pair():
    for a in range(6):
        for b in range(a + 1, 6):
            assert len({(c[a], c[b]) for c in SELECTION}) == GRID[a] * GRID[b], (a, b)


@pytest.mark.parametrize("i", range(N_CASES))
def test_exact_on_integer_features(tiles, i):
    nq, nx, D, k, pad, off = _case(i, tiles)
    q, x = _ints(1000 + i, nq, D), _ints(2000 + i, nx, D)
    if nx >= 4:                                   # ties on purpose: duplicated database rows, the lower index first
        x[nx - 1] = x[0]
        x[nx // 2] = x[1]
    if nq >= 2 and nx >= 1:
        q[1] = x[0]                               # distance exactly 0
    got = _run(q, x, k, q_pad=pad, x_pad=pad, q_off=off, x_off=(off + i // 8) % 2)
    _assert_exact(got, q, x, k, label=f"nq={nq} nx={nx} D={D} k={k} pad={pad} off={off}")
    if nx < k:
        assert (got[0][:, nx:] == -1).all() and np.isposinf(got[1][:, nx:]).all()


@pytest.mark.parametrize("k", [6, 7, 32])
def test_every_candidate_inserts(tiles, k):
    """Distances that fall strictly with j: each database row displaces the whole current list.  k = 6 and 7 sit on
    either side of the list capacity up to which the kernel runs two workgroups per CU (csrc/knn.hip)."""
    tq, tx, _ = tiles
    nq, nx, D = tq + 1, 2 * tx + 76, 4
    q, x = _ints(31, nq, D), np.zeros((nx, D), np.float32)
    q[:, 0] = 0
    x[:, 0] = nx - np.arange(nx)
    got = _run(q, x, k)
    _assert_exact(got, q, x, k)
    assert (got[0] == np.arange(nx - 1, nx - 1 - k, -1)[None, :]).all()


def test_widest_exact_width(tiles):
    tq, tx, _ = tiles
    q, x = _ints(41, tq + 1, 512), _ints(42, tx + 1, 512)
    _assert_exact(_run(q, x, 5, q_pad=4, x_pad=8), q, x, 5)


# ------------------------------------------------------------------------------------------------ eligibility
def test_leave_one_out_never_returns_the_row_itself(tiles):
    tq, tx, _ = tiles
    n, D, k = 2 * tx + 76, 5, 5
    x = _ints(51, n, D)
    xd = _place(x, 3, 0)
    g = np.arange(n)
    idx, dist = got = _run(x, x, k, g, g, q_dev=xd, x_dev=xd)
    assert not (idx == g[:, None]).any() and (idx >= 0).all()
    _assert_exact(got, x, x, k, g, g)
    plain = _run(x, x, 1, q_dev=xd, x_dev=xd)
    assert (plain[1] == 0).all()                              # without groups every row finds itself or a duplicate
    assert (plain[0][:, 0] <= g).all()


@pytest.mark.parametrize("block", [3, 50])
def test_block_groups(tiles, block):
    tq, tx, _ = tiles
    nq, nx, D, k = tq + 1, 2 * tx + 76, 7, 5
    q, x = _ints(61, nq, D), _ints(62, nx, D)
    qg, xg = np.arange(nq) // block, np.arange(nx) // block
    idx, dist = got = _run(q, x, k, qg, xg, x_pad=1)
    assert (xg[idx] != qg[:, None]).all()
    _assert_exact(got, q, x, k, qg, xg)
    # a NULL on either side: no exclusion
    _assert_exact(_run(q, x, k, qg, None), q, x, k)
    _assert_exact(_run(q, x, k, None, xg), q, x, k)


def test_exclusion_leaves_fewer_than_k_rows(tiles):
    tq, tx, _ = tiles
    nq, nx, D, k = 5, tx + 9, 3, 5
    q, x = _ints(71, nq, D), _ints(72, nx, D)
    xg = np.zeros(nx, np.int64)
    xg[[7, tx + 2]] = 1                                       # two rows outside group 0
    qg = np.array([0, 0, 1, 0, 2])
    idx, dist = got = _run(q, x, k, qg, xg)
    _assert_exact(got, q, x, k, qg, xg)
    for i in (0, 1, 3):
        assert sorted(idx[i, :2]) == [7, tx + 2] and (idx[i, 2:] == -1).all() and np.isposinf(dist[i, 2:]).all()
    assert (idx[[2, 4]] >= 0).all()
    none = _run(q, x, k, np.zeros(nq, np.int64), np.zeros(nx, np.int64))
    assert (none[0] == -1).all() and np.isposinf(none[1]).all()


def test_nan_and_inf_rows_are_never_neighbours(tiles):
    tq, tx, cd = tiles
    nq, nx, D, k = 9, tx + 40, cd + 1, 32
    q, x = _ints(81, nq, D), _ints(82, nx, D)
    q[:, 3] = 0                                               # 0 * inf on some pairs as well
    bad = {0: np.nan, 5: np.inf, 6: -np.inf, tx - 1: np.nan, tx: np.inf, nx - 1: -np.inf}
    for j, v in bad.items():
        x[j, (3 * j) % D] = v
    x[5, 3] = np.inf
    idx, dist = got = _run(q, x, k)
    assert not np.isin(idx, list(bad)).any() and np.isfinite(dist).all()
    _assert_exact(got, q, x, k)
    few = _run(q, x[:8], k)                                   # 5 finite rows only: the tail
    assert (few[0][:, 5:] == -1).all() and not np.isin(few[0], [0, 5, 6]).any()
    qn = q.copy()
    qn[2, 1] = np.nan                                         # a NaN query has no neighbour
    i2, d2 = _run(qn, x, 3)
    assert (i2[2] == -1).all() and np.isposinf(d2[2]).all() and (i2[[0, 1, 3]] >= 0).all()


# ------------------------------------------------------------------------------------------------ geometry
def test_split_counts_and_launches_give_identical_bits(tiles):
    tq, tx, _ = tiles
    nq, nx, D, k = tq + 1, 2 * tx + 76, 33, 5
    q, x = gen.normal(91, (nq, D)), gen.normal(92, (nx, D))
    x[nx - 1] = x[3]                                          # a tie across splits
    x[tx] = x[3]
    q[0] = x[3]
    ref = _run(q, x, k, splits=1)
    assert list(ref[0][0, :3]) == [3, tx, nx - 1]             # equal distances: ascending index, across tiles
    assert len(set(_bits(ref[1][0, :3]))) == 1
    for sp in (2, 7, None, 1):
        got = _run(q, x, k, splits=sp)
        assert np.array_equal(got[0], ref[0]) and np.array_equal(_bits(got[1]), _bits(ref[1])), f"splits={sp}"
    from arcweld import _native
    with pytest.raises(_native.NativeError, match="splits"):
        _run(q, x, k, splits=_native.KNN_MAX_SPLITS + 1)
    with pytest.raises(_native.NativeError, match="k = 33"):
        _run(q, x, 33)


# ------------------------------------------------------------------------------------------------ random block
def _check_bounds(idx, dist, q, x, k, qg=None, xg=None, label=""):
    """The four conditions of a correct f32 search on arbitrary data, per query, for every pair."""
    nq, nx = len(q), len(x)
    D = q.shape[1]
    d64, e = R.sqdist64(q, x), R.eps(q, x, D)
    ok = R.eligible(nq, nx, qg, xg, d64)
    assert idx.shape == (nq, k) and (idx >= 0).all() and (idx < nx).all()
    rows = np.arange(nq)[:, None]
    assert all(len(set(r)) == k for r in idx), f"{label}: repeated neighbours"
    assert ok[rows, idx].all(), f"{label}: an ineligible neighbour"
    assert (np.diff(dist, axis=1) >= 0).all() and (dist >= 0).all(), f"{label}: dist not ascending"
    err = np.abs(dist.astype(np.float64) - d64[rows, idx])
    print(f"{label}: max |dist - d64| / eps = {(err / e[rows, idx]).max():.3g}")
    assert (err <= e[rows, idx]).all(), f"{label}: a stored distance is off by more than eps"
    # a row left out lost to the k-th in f32, so d64 + eps >= d64(k-th) - eps(k-th): "2 eps", one eps per pair
    kth, e_kth = d64[rows, idx][:, -1:], e[rows, idx][:, -1:]
    rest = ok.copy()
    rest[rows, idx] = False
    assert not (rest & (d64 < kth - e_kth - e)).any(), f"{label}: a nearer row was left out"


@pytest.mark.parametrize("D", [33, 1024])
def test_random_features_within_the_derived_bound(tiles, D):
    tq, tx, _ = tiles
    nq, nx, k = tq + 1, 2 * tx + 76, 5
    q, x = gen.normal(101 + D, (nq, D)), gen.normal(102 + D, (nx, D))
    idx, dist = _run(q, x, k, q_pad=3, x_off=1)
    _check_bounds(idx, dist, q, x, k, label=f"D={D}")
    qg, xg = np.arange(nq) // 3, np.arange(nx) // 3
    idx, dist = _run(q, x, k, qg, xg)
    _check_bounds(idx, dist, q, x, k, qg, xg, label=f"D={D} groups")


# ------------------------------------------------------------------------------------------------ end to end
KW = dict(hidden_dim=64, num_embeddings=32, embedding_dim=16, n_resblocks=2, patch_size=25)
N_CYCLES, SIZES = 2, (40, 9, 7)


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


def _check_result(r, feats_q, feats_x, labels_q, labels_x, k, weights, qg=None, xg=None, label=""):
    idx, dist, pred = (r[n].cpu().numpy() for n in ("idx", "dist", "pred"))
    if feats_q is not None:
        _check_bounds(idx, dist, feats_q, feats_x, k, qg, xg, label=label)
    want_p, _ = R.vote(idx, dist.astype(np.float64), labels_x, 2, weights)
    assert np.array_equal(pred, want_p)
    for name, v in R.metrics(pred, labels_q).items():
        assert abs(r[name] - v) <= 1e-6, (label, name, r[name], v)


@pytest.mark.parametrize("dataset, weights", [("latent_vq_vae", "uniform"), ("asimow", "distance")])
def test_probe_neighbours_and_metrics(vqvae, splits, fp32, dataset, weights):
    from arcweld.data import latent_vectors
    from arcweld.retrieve import latent_knn_probe
    k = 3
    res = latent_knn_probe(splits, N_CYCLES, k=k, dataset=dataset, vqvae=vqvae, weights=weights, standardize=False,
                           loo=True)
    assert set(res) == {"val", "test", "train_loo"}
    feats = [(latent_vectors(vqvae, x, N_CYCLES) if dataset == "latent_vq_vae" else x).reshape(len(x), -1).cpu().numpy()
             for x, _ in splits]
    labels = [y.cpu().numpy() for _, y in splits]
    for qi, name in ((1, "val"), (2, "test")):
        assert set(res[name]) == {"acc", "acc_good", "acc_bad", "f1", "idx", "dist", "pred"}
        _check_result(res[name], feats[qi], feats[0], labels[qi], labels[0], k, weights, label=f"{dataset} {name}")
    own = np.arange(SIZES[0])
    loo = res["train_loo"]["idx"].cpu().numpy()
    assert not (loo == own[:, None]).any()
    _check_result(res["train_loo"], feats[0], feats[0], labels[0], labels[0], k, weights, own, own,
                  label=f"{dataset} loo")


def test_probe_standardized_and_grouped(vqvae, splits, fp32):
    from arcweld.retrieve import knn_search, latent_knn_probe
    groups = {"train": torch.arange(SIZES[0]) // 4, "val": torch.arange(SIZES[1]) // 4}
    res = latent_knn_probe(splits, N_CYCLES, k=1, dataset="asimow", loo=True, groups=groups)
    labels = [y.cpu().numpy() for _, y in splits]
    for qi, name in ((1, "val"), (2, "test"), (0, "train_loo")):
        _check_result(res[name], None, None, labels[qi], labels[0], 1, "uniform", label=name)
    tg, vg = groups["train"].numpy(), groups["val"].numpy()
    assert (tg[res["train_loo"]["idx"].cpu().numpy()[:, 0]] != tg).all()       # leave-one-group-out
    assert (tg[res["val"]["idx"].cpu().numpy()[:, 0]] != vg).all()
    # the scaler: the probe's standardised search equals a search of features standardised by the restatement
    x_tr, x_te = (splits[i][0].reshape(SIZES[i], -1) for i in (0, 2))
    mean, scale = R.scaler(x_tr.cpu().numpy())
    zq, zx = R.standardize(x_te.cpu().numpy(), mean, scale), R.standardize(x_tr.cpu().numpy(), mean, scale)
    idx, dist = knn_search(x_te, x_tr, k=1)
    _check_bounds(idx.cpu().numpy(), dist.cpu().numpy(), zq, zx, 1, label="standardised")
    assert np.array_equal(idx.cpu().numpy(), res["test"]["idx"].cpu().numpy())
    _, root = knn_search(x_te, x_tr, k=1, sqrt=True)
    assert torch.equal(root, dist.sqrt())


def test_script_writes_both_files(vqvae, fp32, tmp_path):
    import probe_latent_space as pls
    ckpt, out, nb = tmp_path / "v.ckpt", tmp_path / "probe.json", tmp_path / "nb.npz"
    vqvae.save_checkpoint(str(ckpt))
    pls.main(pls.parser().parse_args(["--vqvae-model", str(ckpt), "--n-cycles", str(N_CYCLES), "--k", "3", "--loo",
                                      "--n-train", "24", "--n-val", "5", "--n-test", "6", "--seed", "3",
                                      "--out", str(out), "--neighbours-out", str(nb)]))
    summary = json.loads(out.read_text())
    assert set(summary) == {"val", "test", "train_loo", "k", "weights", "dataset", "standardize", "n_cycles"}
    assert summary["k"] == 3 and summary["dataset"] == "latent_vq_vae" and summary["standardize"] is True
    for name in ("val", "test", "train_loo"):
        assert set(summary[name]) == {"acc", "acc_good", "acc_bad", "f1"}
        assert all(0.0 <= v <= 1.0 for v in summary[name].values())
    with np.load(nb, allow_pickle=False) as f:
        assert set(f.files) == {f"{s}_{key}" for s in ("val", "test", "train_loo") for key in ("idx", "dist", "pred")}
        for s, n in (("val", 5), ("test", 6), ("train_loo", 24)):
            assert f[f"{s}_idx"].shape == (n, 3) and f[f"{s}_idx"].dtype == np.int64
            assert f[f"{s}_dist"].shape == (n, 3) and f[f"{s}_dist"].dtype == np.float32
            assert f[f"{s}_pred"].shape == (n,) and set(np.unique(f[f"{s}_pred"])) <= {0, 1}
        assert not (f["train_loo_idx"] == np.arange(24)[:, None]).any()
