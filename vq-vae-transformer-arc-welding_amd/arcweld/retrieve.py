"""Retrieval in a feature space: exact k-nearest-neighbour search on the device (arcweld.kernels.knn, csrc/knn.hip)
and the training-free k-NN probe of a latent space built on it.

The reference's tree carries the protocol for learned representations (model/ts2vec/_eval_protocols.py::fit_knn: a
StandardScaler followed by a 1-nearest-neighbour classifier); here it scores the frozen VQ-VAE's latent vectors -- the
features train_classification_model.py --dataset latent_vq_vae fits a GRU on -- in seconds instead of a training run,
and answers "which training welds does this sequence look like".

  knn_search        (idx, dist) of the k nearest database rows per query, optionally standardised
  knn_vote          class votes of the neighbours' labels -> (pred, votes); plain torch on the inputs' device
  latent_knn_probe  train split = database, val / test = queries: accuracy, per-class accuracy, F1 and the neighbours

The search itself is the HIP kernel; the scaler and the vote are torch plumbing around it.  There is no CPU search.
"""
from __future__ import annotations

import torch

from . import _native as nat

__all__ = ["knn_search", "knn_vote", "latent_knn_probe", "standard_scaler", "MAX_K"]

MAX_K = nat.AW_KNN_MAX_K
_ROWS_PER_CHUNK = 8192


def _as_rows(t, name):
    if not isinstance(t, torch.Tensor):
        raise ValueError(f"{name}: expected a torch tensor, got {type(t).__name__}")
    if t.dim() < 2:
        raise ValueError(f"{name}: expected (n, ...) with at least 2 dimensions, got shape {tuple(t.shape)}")
    if not t.is_floating_point():
        raise ValueError(f"{name}: expected a floating-point tensor, got {t.dtype}")
    rows = t.reshape(t.shape[0], -1)
    if rows.shape[1] < 1:
        raise ValueError(f"{name}: rows have no features (shape {tuple(t.shape)})")
    return rows


def _check_k(k):
    if isinstance(k, bool) or not isinstance(k, int) or not 1 <= k <= MAX_K:
        raise ValueError(f"k: expected an int in 1..{MAX_K}, got {k!r}")
    return k


def _as_group(g, n, name):
    if g is None:
        return None
    g = torch.as_tensor(g)
    if g.dim() != 1 or g.shape[0] != n or g.is_floating_point() or g.dtype == torch.bool:
        raise ValueError(f"{name}: expected {n} integer group ids, got {g.dtype} of shape {tuple(g.shape)}")
    return g


def _device_of(*tensors):
    for t in tensors:
        if t.is_cuda:
            return t.device
    return torch.device("cuda", torch.cuda.current_device())


@torch.no_grad()
def standard_scaler(database):
    """(mean, scale) of the database's features as f64 tensors: sklearn's StandardScaler -- the per-feature mean and
    the square root of the population variance, both accumulated in f64 over row chunks; scale 1 where the variance is
    0 (the rule of asimow.ChannelScaler)."""
    n, D = database.shape
    mean = torch.zeros(D, dtype=torch.float64, device=database.device)
    for o in range(0, n, _ROWS_PER_CHUNK):
        mean += database[o:o + _ROWS_PER_CHUNK].double().sum(0)
    mean /= max(n, 1)
    var = torch.zeros_like(mean)
    for o in range(0, n, _ROWS_PER_CHUNK):
        var += ((database[o:o + _ROWS_PER_CHUNK].double() - mean) ** 2).sum(0)
    var /= max(n, 1)
    scale = torch.where(var > 0, var.sqrt(), torch.ones_like(var))
    return mean, scale


@torch.no_grad()
def _standardize(rows, mean, scale):
    out = torch.empty(rows.shape, dtype=torch.float32, device=rows.device)
    for o in range(0, rows.shape[0], _ROWS_PER_CHUNK):
        out[o:o + _ROWS_PER_CHUNK] = ((rows[o:o + _ROWS_PER_CHUNK].double() - mean) / scale).float()
    return out


@torch.no_grad()
def knn_search(queries, database, k=1, standardize=True, q_group=None, x_group=None, sqrt=False):
    """The k nearest database rows of every query in Euclidean distance.

    queries (nq, ...) and database (nx, ...) are flattened to (n, D).  standardize: fit_knn's StandardScaler, fitted on
    the database (standard_scaler) and applied to both sides.  q_group (nq) / x_group (nx): integer ids; a database
    row is skipped for a query of the same id (leave-one-out of a set against itself: both arange(n); leave-one-run-
    out: run ids); either None: no exclusion.  Returns idx (nq, k) int64 and dist (nq, k) f32 on the device, nearest
    first, ties to the lower database index; dist is the squared distance, or the distance with sqrt=True.  Slots
    past the eligible rows hold (-1, +inf).  Argument errors are ValueErrors naming the argument, raised before any
    device work."""
    q, x = _as_rows(queries, "queries"), _as_rows(database, "database")
    if q.shape[1] != x.shape[1]:
        raise ValueError(f"database: {x.shape[1]} features per row, queries have {q.shape[1]}")
    k = _check_k(k)
    if x.shape[0] >= 2 ** 31:
        raise ValueError(f"database: {x.shape[0]} rows, the search indexes at most 2^31 - 1")
    if not isinstance(standardize, bool):
        raise ValueError(f"standardize: expected a bool, got {standardize!r}")
    if not isinstance(sqrt, bool):
        raise ValueError(f"sqrt: expected a bool, got {sqrt!r}")
    qg, xg = _as_group(q_group, q.shape[0], "q_group"), _as_group(x_group, x.shape[0], "x_group")

    from . import kernels
    dev = _device_of(q, x)
    q, x = q.to(dev), x.to(dev)
    if standardize:
        mean, scale = standard_scaler(x)
        q, x = _standardize(q, mean, scale), _standardize(x, mean, scale)
    else:
        q, x = q.float(), x.float()
        q = q if q.stride(-1) == 1 else q.contiguous()
        x = x if x.stride(-1) == 1 else x.contiguous()
    if qg is not None and xg is not None:
        qg, xg = qg.to(dev, torch.int32).contiguous(), xg.to(dev, torch.int32).contiguous()
    else:
        qg = xg = None
    idx, dist = kernels.knn(q, x, k, q_group=qg, x_group=xg)
    return idx, (dist.sqrt() if sqrt else dist)


@torch.no_grad()
def knn_vote(idx, dist, labels, n_classes=2, weights="uniform"):
    """Class votes of the neighbours: pred (n,) int64 and votes (n, n_classes) f64, on idx's device.

    idx, dist: (n, k) from knn_search; labels: (nx,) class ids of the database rows.  Slots with idx = -1 are ignored.
    weights "uniform": one vote per neighbour; "distance": 1 / dist, and where a query has neighbours at distance
    exactly 0 only those vote, with weight 1 (scikit-learn's rule).  Ties go to the lowest class id; a query without
    any neighbour gets pred = -1."""
    if weights not in ("uniform", "distance"):
        raise ValueError(f"weights: expected 'uniform' or 'distance', got {weights!r}")
    if idx.dim() != 2 or idx.is_floating_point():
        raise ValueError(f"idx: expected (n, k) integers, got {idx.dtype} of shape {tuple(idx.shape)}")
    if tuple(dist.shape) != tuple(idx.shape):
        raise ValueError(f"dist: shape {tuple(dist.shape)} differs from idx's {tuple(idx.shape)}")
    if isinstance(n_classes, bool) or not isinstance(n_classes, int) or n_classes < 1:
        raise ValueError(f"n_classes: expected a positive int, got {n_classes!r}")
    labels = torch.as_tensor(labels)
    if labels.dim() != 1 or labels.is_floating_point():
        raise ValueError(f"labels: expected (nx,) integer class ids, got {labels.dtype} of shape {tuple(labels.shape)}")
    dev = idx.device
    labels, dist = labels.to(dev).long(), dist.to(dev)
    if labels.numel() and (int(labels.min()) < 0 or int(labels.max()) >= n_classes):
        raise ValueError(f"labels: class ids must lie in 0..{n_classes - 1}")
    if idx.numel() and int(idx.max()) >= labels.shape[0]:
        raise ValueError(f"idx: neighbour {int(idx.max())} is outside the {labels.shape[0]} labelled rows")
    valid = idx >= 0
    if weights == "uniform":
        w = valid.double()
    else:
        zero = valid & (dist == 0)
        has_zero = zero.any(1, keepdim=True)
        inv = torch.where(valid & (dist > 0), 1.0 / dist.double().clamp(min=1e-300), torch.zeros((), dtype=torch.float64,
                                                                                                  device=dev))
        w = torch.where(has_zero, zero.double(), inv)
    votes = torch.zeros((idx.shape[0], n_classes), dtype=torch.float64, device=dev)
    if labels.numel() and idx.numel():
        votes.scatter_add_(1, labels[idx.clamp(min=0)], w)
    # the lowest class id among the maximal votes
    classes = torch.arange(n_classes, device=dev).expand_as(votes)
    top = votes.max(1, keepdim=True).values
    pred = torch.where(votes == top, classes, torch.full_like(classes, n_classes)).min(1).values
    pred = torch.where(valid.any(1), pred, torch.full_like(pred, -1))
    return pred, votes


def _metrics(pred, target):
    from model.classification_model import binary_f1, class_accuracy, multiclass_accuracy
    return {"acc": float(multiclass_accuracy(pred, target)), "acc_good": float(class_accuracy(pred, target, 1)),
            "acc_bad": float(class_accuracy(pred, target, 0)), "f1": float(binary_f1(pred, target))}


@torch.no_grad()
def latent_knn_probe(splits, n_cycles, k=1, dataset="latent_vq_vae", vqvae=None, weights="uniform", standardize=True,
                     loo=False, groups=None, window=200):
    """k-NN probe of a feature space: the train split is the database, val and test are the queries.

    splits: [(x (n, n_cycles*window, C), labels (n,))] for train / val / test, as ClassificationDataModule takes them.
    The features are what that module would feed the GRU, flattened per sequence: the windows themselves ("asimow") or
    the frozen VQ-VAE's latent vectors (arcweld.data.latent_vectors, "latent_vq_vae").  Returns {"val": r, "test": r},
    r = {acc, acc_good, acc_bad, f1: floats on the GRU path's scale (model.classification_model's metric functions),
    idx, dist (n, k), pred (n,): device tensors}.  loo=True adds "train_loo": the train split against itself, each row
    excluded from its own neighbours -- or, with groups["train"], everything of its own group (leave-one-run-out).
    groups: optional {"train" / "val" / "test": (n,) integer ids}; a val / test split with ids is searched with its
    rows' own groups excluded from the database as well."""
    if dataset not in ("asimow", "latent_vq_vae"):
        raise ValueError(f"dataset: expected 'asimow' or 'latent_vq_vae', got {dataset!r}")
    if dataset == "latent_vq_vae" and vqvae is None:
        raise ValueError("vqvae: dataset latent_vq_vae needs the frozen VQ-VAE")
    if isinstance(n_cycles, bool) or not isinstance(n_cycles, int) or n_cycles < 1:
        raise ValueError(f"n_cycles: expected a positive int, got {n_cycles!r}")
    k = _check_k(k)
    if weights not in ("uniform", "distance"):
        raise ValueError(f"weights: expected 'uniform' or 'distance', got {weights!r}")
    if not isinstance(standardize, bool):
        raise ValueError(f"standardize: expected a bool, got {standardize!r}")
    try:
        splits = [(x, y) for x, y in splits]
    except (TypeError, ValueError):
        raise ValueError("splits: expected three (x, labels) pairs: train, val, test") from None
    if len(splits) != 3:
        raise ValueError(f"splits: expected three (x, labels) pairs: train, val, test; got {len(splits)}")
    names = ("train", "val", "test")
    for nm, (x, y) in zip(names, splits):
        if not isinstance(x, torch.Tensor) or x.dim() != 3 or x.shape[1] != n_cycles * window:
            raise ValueError(f"splits: {nm} x must be (n, n_cycles * window = {n_cycles * window}, C), got "
                             f"{tuple(x.shape) if isinstance(x, torch.Tensor) else type(x).__name__}")
        if not isinstance(y, torch.Tensor) or y.dim() != 1 or y.shape[0] != x.shape[0] or y.is_floating_point():
            raise ValueError(f"splits: {nm} labels must be ({x.shape[0]},) integers")
    if splits[0][0].shape[0] < 1:
        raise ValueError("splits: the train split (the database) is empty")
    groups = dict(groups) if groups is not None else {}
    for key in groups:
        if key not in names:
            raise ValueError(f"groups: unknown split {key!r} (expected train / val / test)")
    g = {nm: _as_group(groups.get(nm), splits[i][0].shape[0], f"groups[{nm!r}]") for i, nm in enumerate(names)}

    dev = _device_of(*(x for x, _ in splits))
    feats, labels = [], []
    for x, y in splits:
        x = x.to(dev).float()
        if dataset == "latent_vq_vae":
            from .data import latent_vectors
            x = latent_vectors(vqvae, x, n_cycles, window)
        feats.append(x.reshape(x.shape[0], -1))
        labels.append(y.to(dev).long())
    if standardize:
        mean, scale = standard_scaler(feats[0])
        feats = [_standardize(f, mean, scale) for f in feats]
    n_classes = max(2, max(int(y.max()) + 1 if y.numel() else 0 for y in labels))

    def run(qi, q_group, x_group):
        idx, dist = knn_search(feats[qi], feats[0], k, standardize=False, q_group=q_group, x_group=x_group)
        pred, _ = knn_vote(idx, dist, labels[0], n_classes=n_classes, weights=weights)
        return {**_metrics(pred, labels[qi]), "idx": idx, "dist": dist, "pred": pred}

    out = {}
    for qi in (1, 2):
        nm = names[qi]
        both = g[nm] is not None and g["train"] is not None
        out[nm] = run(qi, g[nm] if both else None, g["train"] if both else None)
    if loo:
        own = g["train"] if g["train"] is not None else torch.arange(feats[0].shape[0])
        out["train_loo"] = run(0, own, own)
    return out
