"""CPU checks around the k-NN probe: the fp64 restatements of tests/knn_refs.py against a literal double loop, the
derived bound eps against an f32 evaluation, arcweld.retrieve.knn_vote on hand-written neighbours, and every argument
error of knn_search / latent_knn_probe / probe_latent_space.py -- raised on CPU tensors, before any device is looked
at."""
import numpy as np
import pytest
import torch

import knn_refs as R
from oracle import gen


# ------------------------------------------------------------------------------------------------ the restatements
def _literal(q, x, k, qg=None, xg=None):
    nq, nx, D = len(q), len(x), q.shape[1]
    idx = np.full((nq, k), -1, np.int64)
    dist = np.full((nq, k), np.inf)
    for i in range(nq):
        cands = []
        for j in range(nx):
            if qg is not None and xg is not None and qg[i] == xg[j]:
                continue
            d = 0.0
            for c in range(D):
                d += (float(q[i, c]) - float(x[j, c])) ** 2
            if np.isfinite(d):
                cands.append((d, j))
        cands.sort()
        for s, (d, j) in enumerate(cands[:k]):
            idx[i, s], dist[i, s] = j, d
    return idx, dist


@pytest.mark.parametrize("k", [1, 3, 9])
def test_restatement_matches_a_literal_double_loop(k):
    q = gen.randint(71, (5, 3), -4, 5).astype(np.float32)
    x = gen.randint(72, (7, 3), -4, 5).astype(np.float32)
    x[4] = x[1]                                   # a tie: the lower index first
    x[6, 1] = np.nan                              # never a neighbour
    qg, xg = np.array([0, 1, 2, 0, 1]), np.array([0, 0, 1, 1, 2, 2, 3])
    for groups in ((None, None), (qg, xg), (qg, None)):
        want_i, want_d = _literal(q, x, k, *groups)
        got_i, got_d = R.knn(q, x, k, *groups)
        assert np.array_equal(got_i, want_i)
        assert np.allclose(got_d, want_d, rtol=1e-15, atol=0)
    i, _ = R.knn(q, x, 7)
    assert not (i == 6).any() and (i[:, -1] == -1).all()          # 6 eligible rows only
    for r in i:
        r = list(r)
        assert r.index(1) < r.index(4)


def test_eps_bounds_an_f32_evaluation():
    """The bound the GPU test relies on, checked where it can be: an in-order f32 numpy evaluation of the kernel's
    expression stays within eps of fp64 for every pair, at both widths of the GPU test's random block."""
    for D, seed in ((33, 81), (1024, 83)):
        q, x = gen.normal(seed, (6, D)), gen.normal(seed + 1, (40, D))
        err = np.abs(R.d32(q, x).astype(np.float64) - R.sqdist64(q, x))
        bound = R.eps(q, x, D)
        print(f"D={D}: max err / eps = {(err / bound).max():.3g}")
        assert (err <= bound).all()


def test_scaler_restatement():
    x = gen.normal(91, (11, 4)).astype(np.float64)
    x[:, 2] = 3.0                                 # zero variance: scale 1
    mean, scale = R.scaler(x)
    assert np.allclose(mean, x.mean(0)) and scale[2] == 1.0
    assert np.allclose(scale[[0, 1, 3]], x[:, [0, 1, 3]].std(0))
    z = R.standardize(x, mean, scale)
    assert z.dtype == np.float32 and np.allclose(z[:, 2], 0) and np.allclose(z[:, 0].std(), 1, atol=1e-6)


# ------------------------------------------------------------------------------------------------ knn_vote
IDX = torch.tensor([[0, 1, 2], [3, 4, -1], [-1, -1, -1], [5, 0, 1], [2, 5, 3]])
DIST = torch.tensor([[1.0, 2.0, 4.0], [0.5, 0.5, float("inf")], [float("inf")] * 3, [0.0, 0.1, 0.2], [1.0, 4.0, 4.0]])
LABELS = torch.tensor([1, 1, 0, 0, 1, 0])


@pytest.mark.parametrize("weights", ["uniform", "distance"])
def test_vote_matches_the_restatement(weights):
    from arcweld.retrieve import knn_vote
    pred, votes = knn_vote(IDX, DIST, LABELS, n_classes=2, weights=weights)
    want_p, want_v = R.vote(IDX.numpy(), DIST.numpy().astype(np.float64), LABELS.numpy(), 2, weights)
    assert pred.dtype == torch.int64 and votes.shape == (5, 2)
    assert np.array_equal(pred.numpy(), want_p)
    assert np.allclose(votes.numpy(), want_v, rtol=1e-12)


def test_vote_rules_by_hand():
    from arcweld.retrieve import knn_vote
    pred, votes = knn_vote(IDX, DIST, LABELS)
    assert pred.tolist() == [1, 0, -1, 1, 0]      # row 1: a 1-1 tie goes to class 0; row 2: no neighbour
    assert votes[1].tolist() == [1.0, 1.0] and votes[2].tolist() == [0.0, 0.0]
    pred, votes = knn_vote(IDX, DIST, LABELS, weights="distance")
    # row 3: the exact-zero neighbour (label 0) outweighs the two class-1 neighbours at 0.1 and 0.2
    assert pred.tolist() == [1, 0, -1, 0, 0] and votes[3].tolist() == [1.0, 0.0]
    assert votes[0].tolist() == [0.25, 1.5] and votes[4].tolist() == [1.5, 0.0]
    pred3, _ = knn_vote(torch.tensor([[0, 1, 2]]), torch.ones(1, 3), torch.tensor([2, 1, 0]), n_classes=3)
    assert pred3.tolist() == [0]                  # a three-way tie: the lowest class id


def test_vote_argument_errors():
    from arcweld.retrieve import knn_vote
    for kw, name in ((dict(weights="rank"), "weights"), (dict(n_classes=0), "n_classes")):
        with pytest.raises(ValueError, match=name):
            knn_vote(IDX, DIST, LABELS, **kw)
    with pytest.raises(ValueError, match="dist"):
        knn_vote(IDX, DIST[:, :2], LABELS)
    with pytest.raises(ValueError, match="labels"):
        knn_vote(IDX, DIST, LABELS + 1)
    with pytest.raises(ValueError, match="idx"):
        knn_vote(IDX + 1, DIST, LABELS)


# ------------------------------------------------------------------------------------------------ argument errors
Q, X = torch.zeros(4, 6), torch.zeros(9, 6)


@pytest.mark.parametrize("args, kw, name", [
    ((Q, torch.zeros(9, 5)), {}, "database"),
    ((torch.zeros(4), X), {}, "queries"),
    ((Q, torch.zeros(9, 6, dtype=torch.int64)), {}, "database"),
    ((Q.numpy(), X), {}, "queries"),
    ((Q, X), dict(k=0), "k"),
    ((Q, X), dict(k=33), "k"),
    ((Q, X), dict(k=2.0), "k"),
    ((Q, X), dict(standardize=1), "standardize"),
    ((Q, X), dict(sqrt="yes"), "sqrt"),
    ((Q, X), dict(q_group=torch.zeros(3, dtype=torch.int64)), "q_group"),
    ((Q, X), dict(x_group=torch.zeros(9)), "x_group"),
])
def test_knn_search_argument_errors(args, kw, name):
    from arcweld.retrieve import knn_search
    with pytest.raises(ValueError, match=name):
        knn_search(*args, **kw)


def _splits(n_cycles=2, n=(6, 3, 3)):
    return [(torch.zeros(m, n_cycles * 200, 2), torch.zeros(m, dtype=torch.long)) for m in n]


@pytest.mark.parametrize("kw, name", [
    (dict(dataset="mnist"), "dataset"),
    (dict(dataset="latent_vq_vae", vqvae=None), "vqvae"),
    (dict(n_cycles=0), "n_cycles"),
    (dict(k=40), "k"),
    (dict(weights="rank"), "weights"),
    (dict(standardize=None), "standardize"),
    (dict(splits=_splits()[:2]), "splits"),
    (dict(splits=_splits(n_cycles=3)), "splits"),
    (dict(splits=[(x, y.float()) for x, y in _splits()]), "splits"),
    (dict(splits=_splits(n=(0, 3, 3))), "splits"),
    (dict(groups={"dev": torch.zeros(3, dtype=torch.long)}), "groups"),
    (dict(groups={"train": torch.zeros(5, dtype=torch.long)}), "groups"),
])
def test_latent_knn_probe_argument_errors(kw, name):
    from arcweld.retrieve import latent_knn_probe
    args = dict(splits=_splits(), n_cycles=2, dataset="asimow")
    args.update(kw)
    with pytest.raises(ValueError, match=name):
        latent_knn_probe(**args)


def test_script_refuses_a_missing_checkpoint(tmp_path):
    import probe_latent_space as pls
    hp = pls.parser().parse_args(["--vqvae-model", str(tmp_path / "none.ckpt"), "--out", str(tmp_path / "o.json")])
    with pytest.raises(SystemExit, match="--vqvae-model: checkpoint .* not found"):
        pls.main(hp)
    assert not (tmp_path / "o.json").exists()
    with pytest.raises(SystemExit):
        pls.parser().parse_args(["--dataset", "mnist"])
    with pytest.raises(SystemExit):
        pls.parser().parse_args(["--precision", "bf16"])       # no operand mode is offered for the neighbour order


def test_abi_constants_match_the_header():
    import os
    import re
    from conftest import REPO
    from arcweld import _native
    src = open(os.path.join(REPO, "include", "arcweld_amd.h")).read()
    assert int(re.search(r"#define AW_KNN_MAX_K (\d+)", src).group(1)) == _native.KNN_MAX_K == 32
    assert int(re.search(r"#define AW_KNN_MAX_SPLITS (\d+)", src).group(1)) == _native.KNN_MAX_SPLITS
    lib = _native.load()
    assert lib.aw_knn_workspace(100, 1000, 8, 5, 3) == 3 * 100 * 5 * 8
    assert lib.aw_knn_workspace(100, 1000, 8, 33, 3) < 0 and b"k = 33" in lib.aw_last_error()
    assert lib.aw_knn_workspace(100, 2 ** 31, 8, 1, 0) < 0 and lib.aw_knn_workspace(100, 10, 0, 1, 0) < 0
    one, many = lib.aw_knn_workspace(100000, 1 << 20, 8, 1, 0), lib.aw_knn_workspace(128, 1 << 20, 8, 1, 0)
    assert one == 100000 * 8 and many > 128 * 8              # many query tiles: one split; one tile: the database splits
