"""Retrieval in a feature space: exact k-nearest-neighbour search on the device (arcweld.kernels.knn, csrc/knn.hip)
and the training-free k-NN probe of a latent space built on it.

The reference's tree carries the protocol for learned representations (model/ts2vec/_eval_protocols.py::fit_knn: a
StandardScaler followed by a 1-nearest-neighbour classifier); here it scores the frozen VQ-VAE's latent vectors -- the
features train_classification_model.py --dataset latent_vq_vae fits a GRU on -- in seconds instead of a training run,
and answers "which training welds does this sequence look like".

  knn_search        (idx, dist) of the k nearest database rows per query, optionally standardised
  knn_vote          class votes of the neighbours' labels -> (pred, votes); plain torch on the inputs' device
  latent_knn_probe  train split = database, val / test = queries: accuracy, per-class accuracy, F1 and the neighbours
                    (dataset "ts2vec": of the TS2Vec baseline's pooled representations, arcweld.ts2vec)

  dtw_search        the same under banded dynamic time warping of (n, L, C) sequences (arcweld.kernels.dtw_knn,
                    csrc/dtw.hip): the strong baseline for raw weld cycles, which differ in phase and duration

The search itself is the HIP kernel; the scaler and the vote are torch plumbing around it.  There is no CPU search.

The same tree's default protocol is the linear one (fit_lr: a StandardScaler, then an L2-regularised one-vs-rest
logistic regression); its loss + gradient evaluation over the feature matrix is the HIP kernel pair of
csrc/logreg.hip (arcweld.kernels.logreg_forward / logreg_grad), the optimiser a small batched L-BFGS around it:

  logreg_fit           coefficients of one problem per (class, C), all sharing every pass over the features
  logreg_decision      decision values of the queries; logreg_predict: the class ids
  latent_linear_probe  fit on train, {acc, acc_good, acc_bad, f1} on val / test per C, the C with the best val F1

The third protocol of that tree is an RBF support-vector classifier (fit_svm: no scaler, SVC(kernel='rbf',
gamma='scale', C=0.1)); its kernel matrix and its SMO solver are the HIP kernels of csrc/svm.hip
(arcweld.kernels.rbf_gram / svm_smo), the host side the problem set-up, rho and the vote:

  svm_fit              dual coefficients of one problem per (class pair, C), all on one Gram matrix; rbf_gamma: 'scale'
  svm_decision         decision values of the queries against the support rows; svm_predict: the class ids
  latent_svm_probe     the linear probe's report for the SVM, plus gamma and the support-vector counts
"""
from __future__ import annotations

import torch

from . import _native as nat

__all__ = ["knn_search", "knn_vote", "latent_knn_probe", "standard_scaler", "MAX_K", "logreg_fit", "logreg_decision",
           "logreg_predict", "latent_linear_probe", "stratified_subsample", "MAX_PROBLEMS", "rbf_gamma", "svm_pairs",
           "svm_fit", "svm_decision", "svm_predict", "latent_svm_probe", "MAX_SVM_ROWS", "dtw_search", "MAX_DTW_LEN",
           "MAX_DTW_WINDOW", "MAX_DTW_CHANNELS"]

MAX_K = nat.AW_KNN_MAX_K
MAX_DTW_LEN, MAX_DTW_WINDOW, MAX_DTW_CHANNELS = nat.AW_DTW_MAX_LEN, nat.AW_DTW_MAX_WINDOW, nat.AW_DTW_MAX_C
MAX_PROBLEMS = nat.AW_LOGREG_MAX_P
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


_DATASETS = ("asimow", "latent_vq_vae", "ts2vec")


def _check_ts2vec(dataset, ts2vec):
    if dataset == "ts2vec" and (ts2vec is None or not callable(getattr(ts2vec, "encode", None))):
        raise ValueError("ts2vec: dataset ts2vec needs the TS2Vec encoder (arcweld.ts2vec.TSEncoder or "
                         "model.ts2vec.TS2Vec)")
    if dataset != "ts2vec" and ts2vec is not None:
        raise ValueError(f"ts2vec: belongs to dataset 'ts2vec', got an encoder with dataset {dataset!r}")


def _ts2vec_features(ts2vec, x):
    """The reference's eval_classification features: encode(x, encoding_window='full_series') of the (n, n_cycles *
    window, C) split, (n, output_dims) f32 on x's device (model.ts2vec.TS2Vec returns an array, TSEncoder a tensor)."""
    f = ts2vec.encode(x, encoding_window="full_series")
    f = torch.as_tensor(f).to(x.device, torch.float32)
    if f.dim() != 2 or f.shape[0] != x.shape[0]:
        raise ValueError(f"ts2vec: encode returned shape {tuple(f.shape)} for {x.shape[0]} sequences")
    return f


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


def _check_radius(radius, L):
    """The band radius in samples: None is L - 1 (unconstrained); limits from the header (MAX_DTW_WINDOW)."""
    if radius is None:
        radius = L - 1
    if isinstance(radius, bool) or not isinstance(radius, int) or not 0 <= radius <= L - 1:
        raise ValueError(f"radius: expected None or an int in 0..L - 1 = {L - 1}, got {radius!r}")
    if 2 * radius + 1 > MAX_DTW_WINDOW:
        raise ValueError(f"radius: {radius} gives a band of {2 * radius + 1} samples, the search holds at most "
                         f"{MAX_DTW_WINDOW} (radius <= {(MAX_DTW_WINDOW - 1) // 2})")
    return radius


def _as_sequences(t, name):
    if not isinstance(t, torch.Tensor):
        raise ValueError(f"{name}: expected a torch tensor, got {type(t).__name__}")
    if t.dim() != 3:
        raise ValueError(f"{name}: expected (n, L, C) sequences, got shape {tuple(t.shape)}")
    if not t.is_floating_point():
        raise ValueError(f"{name}: expected a floating-point tensor, got {t.dtype}")
    if not 1 <= t.shape[1] <= MAX_DTW_LEN:
        raise ValueError(f"{name}: sequence length {t.shape[1]} outside 1..{MAX_DTW_LEN}")
    if not 1 <= t.shape[2] <= MAX_DTW_CHANNELS:
        raise ValueError(f"{name}: {t.shape[2]} channels outside 1..{MAX_DTW_CHANNELS}")
    return t


@torch.no_grad()
def dtw_search(queries, database, k=1, radius=None, standardize=False, q_group=None, x_group=None, sqrt=False):
    """The k nearest database sequences of every query under dynamic time warping (csrc/dtw.hip).

    queries (nq, L, C) and database (nx, L, C) share L <= 2000 and C <= 8.  The distance is the squared-cost
    "dependent" multichannel DTW inside a Sakoe-Chiba band: sample i of the query may be matched with sample j of the
    database row iff |i - j| <= radius; radius None means L - 1 (no constraint), radius 0 is the squared Euclidean
    distance; 2 radius + 1 <= 449.  standardize: a PER-CHANNEL scaler fitted on the database,
    standard_scaler(database.reshape(-1, C)), applied to both sides (a per-position scaler would erase the axis DTW
    warps, so it is not offered).  q_group / x_group, the ranking, ties and the (-1, +inf) slots are knn_search's.
    Returns idx (nq, k) int64 and dist (nq, k) f32 on the device: the DTW cost, or its square root with sqrt=True.
    Argument errors are ValueErrors naming the argument, raised before any device work."""
    q, x = _as_sequences(queries, "queries"), _as_sequences(database, "database")
    if q.shape[1:] != x.shape[1:]:
        raise ValueError(f"database: sequences of shape {tuple(x.shape[1:])}, queries have {tuple(q.shape[1:])}")
    L, C = x.shape[1], x.shape[2]
    k = _check_k(k)
    radius = _check_radius(radius, L)
    if x.shape[0] >= 2 ** 31:
        raise ValueError(f"database: {x.shape[0]} rows, the search indexes at most 2^31 - 1")
    if not isinstance(standardize, bool):
        raise ValueError(f"standardize: expected a bool, got {standardize!r}")
    if not isinstance(sqrt, bool):
        raise ValueError(f"sqrt: expected a bool, got {sqrt!r}")
    qg, xg = _as_group(q_group, q.shape[0], "q_group"), _as_group(x_group, x.shape[0], "x_group")

    from . import kernels
    dev = _device_of(q, x)
    q, x = q.to(dev).reshape(q.shape[0], L * C), x.to(dev).reshape(x.shape[0], L * C)
    if standardize:
        mean, scale = standard_scaler(x.reshape(-1, C))
        q = _standardize(q.reshape(-1, C), mean, scale).reshape(-1, L * C)
        x = _standardize(x.reshape(-1, C), mean, scale).reshape(-1, L * C)
    else:
        q, x = q.float(), x.float()
        q = q if q.stride(-1) == 1 else q.contiguous()
        x = x if x.stride(-1) == 1 else x.contiguous()
    if qg is not None and xg is not None:
        qg, xg = qg.to(dev, torch.int32).contiguous(), xg.to(dev, torch.int32).contiguous()
    else:
        qg = xg = None
    idx, dist = kernels.dtw_knn(q, x, L, C, radius, k, q_group=qg, x_group=xg)
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
                     loo=False, groups=None, window=200, metric="euclidean", radius=None, ts2vec=None):
    """k-NN probe of a feature space: the train split is the database, val and test are the queries.

    splits: [(x (n, n_cycles*window, C), labels (n,))] for train / val / test, as ClassificationDataModule takes them.
    The features are what that module would feed the GRU, flattened per sequence: the windows themselves ("asimow") or
    the frozen VQ-VAE's latent vectors (arcweld.data.latent_vectors, "latent_vq_vae"), or -- dataset "ts2vec" with
    ts2vec= an arcweld.ts2vec.TSEncoder or a model.ts2vec.TS2Vec -- the learned baseline's pooled representations,
    encode(x, encoding_window='full_series') of each split: the reference's eval_classification.  The linear and the
    SVM probe take the same two arguments.  Returns {"val": r, "test": r},
    r = {acc, acc_good, acc_bad, f1: floats on the GRU path's scale (model.classification_model's metric functions),
    idx, dist (n, k), pred (n,): device tensors}.  loo=True adds "train_loo": the train split against itself, each row
    excluded from its own neighbours -- or, with groups["train"], everything of its own group (leave-one-run-out).
    groups: optional {"train" / "val" / "test": (n,) integer ids}; a val / test split with ids is searched with its
    rows' own groups excluded from the database as well.
    metric "dtw" (dataset "asimow" only: latent rows are (n_cycles, 1024)-shaped vectors, not time series) searches
    the raw (n, n_cycles * window, C) sequences under dynamic time warping (dtw_search) in a band of `radius` samples
    (None: unconstrained); standardize is then dtw_search's per-channel scaler, fitted on the train split; dist is
    the DTW cost.  Voting, metrics, loo and groups are the same.  radius belongs to metric "dtw"."""
    if dataset not in _DATASETS:
        raise ValueError(f"dataset: expected 'asimow' or 'latent_vq_vae', got {dataset!r}")
    if metric not in ("euclidean", "dtw"):
        raise ValueError(f"metric: expected 'euclidean' or 'dtw', got {metric!r}")
    if metric == "dtw" and dataset == "ts2vec":
        raise ValueError("metric: 'dtw' warps the time axis of the raw cycles and needs dataset 'asimow'; the rows of "
                         "dataset 'ts2vec' are pooled representations, not time series")
    if metric == "dtw" and dataset != "asimow":
        raise ValueError("metric: 'dtw' warps the time axis of the raw cycles and needs dataset 'asimow'; the rows of "
                         "dataset 'latent_vq_vae' are (n_cycles, 1024)-shaped latent vectors, not time series")
    if metric != "dtw" and radius is not None:
        raise ValueError(f"radius: belongs to metric 'dtw', got {radius!r} with metric {metric!r}")
    if dataset == "latent_vq_vae" and vqvae is None:
        raise ValueError("vqvae: dataset latent_vq_vae needs the frozen VQ-VAE")
    _check_ts2vec(dataset, ts2vec)
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
    if metric == "dtw":
        for nm, (x, _) in zip(names, splits):
            _as_sequences(x, f"splits: {nm} x")
            if x.shape[2] != splits[0][0].shape[2]:
                raise ValueError(f"splits: {nm} x has {x.shape[2]} channels, train has {splits[0][0].shape[2]}")
        radius = _check_radius(radius, n_cycles * window)

    dev = _device_of(*(x for x, _ in splits))
    feats, labels = [], []
    for x, y in splits:
        x = x.to(dev).float()
        if dataset == "latent_vq_vae":
            from .data import latent_vectors
            x = latent_vectors(vqvae, x, n_cycles, window)
        elif dataset == "ts2vec":
            x = _ts2vec_features(ts2vec, x)
        feats.append(x if metric == "dtw" else x.reshape(x.shape[0], -1))
        labels.append(y.to(dev).long())
    if standardize and metric == "dtw":
        C = feats[0].shape[2]
        mean, scale = standard_scaler(feats[0].reshape(-1, C))
        feats = [_standardize(f.reshape(-1, C), mean, scale).reshape(f.shape) for f in feats]
    elif standardize:
        mean, scale = standard_scaler(feats[0])
        feats = [_standardize(f, mean, scale) for f in feats]
    n_classes = max(2, max(int(y.max()) + 1 if y.numel() else 0 for y in labels))

    def run(qi, q_group, x_group):
        if metric == "dtw":
            idx, dist = dtw_search(feats[qi], feats[0], k, radius=radius, standardize=False, q_group=q_group,
                                   x_group=x_group)
        else:
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


# ------------------------------------------------------------------------------------------------ linear probe
_LBFGS_HISTORY = 10
_LS_C1, _LS_C2, _LS_SHRINK, _LS_MAX = 1e-4, 0.9, 0.5, 30
_LS_FLAT = 1e-6     # relative agreement of two objective values below which their f32 evaluation noise decides


def _check_C(C):
    seq = [C] if isinstance(C, (int, float)) and not isinstance(C, bool) else C
    try:
        vals = [v for v in seq]
    except TypeError:
        raise ValueError(f"C: expected a positive float or a sequence of them, got {C!r}") from None
    if not vals or any(isinstance(v, bool) or not isinstance(v, (int, float)) or not 0 < float(v) < float("inf")
                       for v in vals):
        raise ValueError(f"C: expected a positive float or a non-empty sequence of them, got {C!r}")
    return [float(v) for v in vals]


def _check_fit_args(standardize, tol, max_iter):
    if not isinstance(standardize, bool):
        raise ValueError(f"standardize: expected a bool, got {standardize!r}")
    if isinstance(tol, bool) or not isinstance(tol, (int, float)) or not 0 < float(tol) < float("inf"):
        raise ValueError(f"tol: expected a positive float, got {tol!r}")
    if isinstance(max_iter, bool) or not isinstance(max_iter, int) or max_iter < 1:
        raise ValueError(f"max_iter: expected a positive int, got {max_iter!r}")


def _logreg_minimize(x, y, cls, Cp, tol, max_iter):
    """Batched L-BFGS over P <= 32 problems that share x (n, D) f32: theta (P, D + 1) f64 [w | b], n_iter, converged
    and the objective F (logreg_fit's docstring).  Every trial point is rounded to f32 before it is
    evaluated and kept rounded, so the state is exactly what the kernels saw and what the caller gets back."""
    from . import kernels
    n, D = x.shape
    P, dev = cls.numel(), x.device
    lam = 1.0 / (Cp * n)
    ws = kernels.logreg_workspace(n, D, P, device=dev)
    z = torch.empty((n, P), dtype=torch.float32, device=dev)
    r = torch.empty_like(z)
    loss, gb = (torch.empty(P, dtype=torch.float64, device=dev) for _ in range(2))
    g = torch.empty((D, P), dtype=torch.float64, device=dev)

    def evaluate(theta):
        w = theta[:, :D]
        kernels.logreg_forward(x, w.t().float().contiguous(), theta[:, D].float().contiguous(), y, cls, z=z, r=r,
                               loss=loss, gb=gb, ws=ws)
        kernels.logreg_grad(x, r, g=g, ws=ws)
        return (loss / n + 0.5 * lam * (w * w).sum(1),
                torch.cat([g.t() / n + lam[:, None] * w, (gb / n)[:, None]], 1))

    theta = torch.zeros((P, D + 1), dtype=torch.float64, device=dev)
    F, G = evaluate(theta)
    done = G.abs().amax(1) <= tol
    stalled = torch.zeros_like(done)
    has_hist = torch.zeros_like(done)
    n_iter = torch.zeros(P, dtype=torch.int64, device=dev)
    gamma = torch.ones(P, dtype=torch.float64, device=dev)
    hist = []                                      # (s, y, rho), oldest first; a problem's invalid pair is all zeros
    for _ in range(max_iter):
        active = ~(done | stalled)
        if not bool(active.any()):
            break
        q, al = G.clone(), []
        for s_, y_, rho_ in reversed(hist):
            a = rho_ * (s_ * q).sum(1)
            q -= a[:, None] * y_
            al.append(a)
        q *= gamma[:, None]
        for (s_, y_, rho_), a in zip(hist, reversed(al)):
            q += (a - rho_ * (y_ * q).sum(1))[:, None] * s_
        d = -q
        gd = (G * d).sum(1)
        uphill = ~(gd < 0)
        d = torch.where(uphill[:, None], -G, d)
        gd = torch.where(uphill, -(G * G).sum(1), gd)
        alpha = torch.where(has_hist & ~uphill, torch.ones_like(gamma), (1.0 / G.abs().sum(1)).clamp(max=1.0))
        accepted = ~active                          # a finished problem is frozen at its point
        theta_new, F_new, G_new = theta, F, G
        for _ in range(_LS_MAX):
            trial = torch.where(accepted[:, None], theta_new, (theta + alpha[:, None] * d).float().double())
            Ft, Gt = evaluate(trial)
            gtd = (Gt * d).sum(1)
            # sufficient decrease: Armijo's form, or -- where the two values agree to within their f32 evaluation
            # noise -- Hager and Zhang's derivative form of it together with the curvature condition (a step that
            # rounds to nothing fails the latter)
            ok = (Ft <= F + _LS_C1 * alpha * gd) | ((Ft <= F + _LS_FLAT * F.abs()) & (gtd <= (2 * _LS_C1 - 1) * gd)
                                                    & (gtd >= _LS_C2 * gd))
            ok &= ~accepted
            theta_new = torch.where(ok[:, None], trial, theta_new)
            F_new, G_new = torch.where(ok, Ft, F_new), torch.where(ok[:, None], Gt, G_new)
            accepted = accepted | ok
            if bool(accepted.all()):
                break
            alpha = torch.where(accepted, alpha, alpha * _LS_SHRINK)
        moved = active & accepted
        s_, y_ = theta_new - theta, G_new - G
        sy, yy = (s_ * y_).sum(1), (y_ * y_).sum(1)
        valid = moved & (yy > 0) & (sy > 1e-10 * yy)
        zero = torch.zeros((), dtype=torch.float64, device=dev)
        hist.append((torch.where(valid[:, None], s_, zero), torch.where(valid[:, None], y_, zero),
                     torch.where(valid, 1.0 / sy.clamp(min=1e-300), zero)))
        hist = hist[-_LBFGS_HISTORY:]
        gamma = torch.where(valid, sy / yy.clamp(min=1e-300), gamma)
        # a failed search drops the problem's history and retries along the gradient; failing there too ends it
        failed = active & ~accepted
        stalled = stalled | (failed & ~has_hist)
        keep = (~failed).double()
        hist = [(a * keep[:, None], b * keep[:, None], c * keep) for a, b, c in hist]
        gamma = torch.where(failed, torch.ones_like(gamma), gamma)
        has_hist = (has_hist & ~failed) | valid
        n_iter += moved.long()
        theta, F, G = theta_new, F_new, G_new
        done = done | (G.abs().amax(1) <= tol)
    return theta, n_iter, done, F


@torch.no_grad()
def logreg_fit(features, labels, C=1.0, standardize=True, tol=1e-4, max_iter=1000, n_classes=None):
    """L2-regularised logistic regression of labels on features: the reference's fit_lr (a StandardScaler, then
    scikit-learn's LogisticRegression, one-vs-rest), fitted on the device (csrc/logreg.hip).

    features (n, ...) are flattened to (n, D); labels (n,) integer class ids.  C: the inverse regularisation strength,
    one value or a sequence.  Per problem it minimises scikit-learn's objective
        F(w, b) = (1 / n) sum_i [softplus(z_i) - t_i z_i] + |w|^2 / (2 C n),   z_i = x_i . w + b,
    with an unpenalised intercept, and stops a problem when max |grad F| <= tol.  Two classes: one problem per C with
    positive class 1; more: one per (class, C), one-vs-rest.  All problems share every pass over the features, 32 at a
    time.  The optimiser is a batched L-BFGS (history 10, backtracking line search on sufficient decrease, f64 state
    on the device, a finished problem frozen); the kernels see the parameters as f32 and return f64 sums.
    Returns a dict: coef (n_C, n_problems_per_C, D) and intercept (n_C, n_problems_per_C) f64 in the standardised
    space, mean and scale (D,) f64 (0 and 1 without standardize), C (n_C,) f64, n_iter, converged, objective (n_C,
    n_problems_per_C), n_classes, standardize.  Argument errors are ValueErrors naming the argument, raised before any
    device work."""
    if isinstance(features, torch.Tensor) and features.dim() >= 2 and features.shape[0] < 1:
        raise ValueError("features: no rows to fit on")
    x = _as_rows(features, "features")
    Cs = _check_C(C)
    _check_fit_args(standardize, tol, max_iter)
    if n_classes is not None and (isinstance(n_classes, bool) or not isinstance(n_classes, int) or n_classes < 2):
        raise ValueError(f"n_classes: expected None or an int >= 2, got {n_classes!r}")
    labels = torch.as_tensor(labels)
    if labels.dim() != 1 or labels.shape[0] != x.shape[0] or labels.is_floating_point() or labels.dtype == torch.bool:
        raise ValueError(f"labels: expected ({x.shape[0]},) integer class ids, got {labels.dtype} of shape "
                         f"{tuple(labels.shape)}")
    if x.shape[0] < 1:
        raise ValueError("features: no rows to fit on")
    lo, hi = int(labels.min()), int(labels.max())
    if n_classes is None:
        n_classes = max(2, hi + 1)
    if lo < 0 or hi >= n_classes:
        raise ValueError(f"labels: class ids must lie in 0..{n_classes - 1}, got {lo}..{hi}")

    dev = _device_of(x)
    x = x.to(dev)
    D = x.shape[1]
    if standardize:
        mean, scale = standard_scaler(x)
        x = _standardize(x, mean, scale)
    else:
        mean = torch.zeros(D, dtype=torch.float64, device=dev)
        scale = torch.ones(D, dtype=torch.float64, device=dev)
        x = x.float()
        x = x if x.stride(-1) == 1 else x.contiguous()
    y = labels.to(dev, torch.int32).contiguous()
    classes = [1] if n_classes == 2 else list(range(n_classes))
    K = len(classes)
    cls = torch.tensor(classes * len(Cs), dtype=torch.int32, device=dev)
    Cp = torch.tensor([c for c in Cs for _ in classes], dtype=torch.float64, device=dev)
    parts = [_logreg_minimize(x, y, cls[o:o + MAX_PROBLEMS].contiguous(), Cp[o:o + MAX_PROBLEMS], float(tol), max_iter)
             for o in range(0, cls.numel(), MAX_PROBLEMS)]
    theta, n_iter, conv, obj = (torch.cat([p[i] for p in parts]) for i in range(4))
    shape = (len(Cs), K)
    return {"coef": theta[:, :D].reshape(*shape, D), "intercept": theta[:, D].reshape(shape), "mean": mean,
            "scale": scale, "C": torch.tensor(Cs, dtype=torch.float64, device=dev), "n_iter": n_iter.reshape(shape),
            "converged": conv.reshape(shape), "objective": obj.reshape(shape), "n_classes": n_classes,
            "standardize": standardize}


def _check_fit(fit):
    if not isinstance(fit, dict) or not {"coef", "intercept", "mean", "scale", "n_classes", "standardize"} <= set(fit):
        raise ValueError("fit: expected the dict logreg_fit returns")
    return fit


@torch.no_grad()
def logreg_decision(fit, queries):
    """z (n_C, n, n_problems_per_C) f32: the decision function of every fitted problem on the queries (scaled with the
    fit's mean and scale), 32 problems per pass over the queries (aw_logreg_forward without labels)."""
    fit = _check_fit(fit)
    q = _as_rows(queries, "queries")
    coef, icpt = fit["coef"], fit["intercept"]
    nC, K, D = coef.shape
    if q.shape[1] != D:
        raise ValueError(f"queries: {q.shape[1]} features per row, the fit has {D}")
    from . import kernels
    dev = coef.device
    q = q.to(dev)
    if fit["standardize"]:
        q = _standardize(q, fit["mean"], fit["scale"])
    else:
        q = q.float()
        q = q if q.stride(-1) == 1 else q.contiguous()
    w, b = coef.reshape(nC * K, D).t().float(), icpt.reshape(nC * K).float()
    z = torch.cat([kernels.logreg_forward(q, w[:, o:o + MAX_PROBLEMS].contiguous(), b[o:o + MAX_PROBLEMS].contiguous())
                   for o in range(0, nC * K, MAX_PROBLEMS)], 1)
    return z.reshape(q.shape[0], nC, K).permute(1, 0, 2).contiguous()


@torch.no_grad()
def logreg_predict(fit, queries, decision=None):
    """Class ids (n_C, n) int64: z > 0 for two classes, else the class of the largest decision value (one-vs-rest;
    ties to the lowest class).  decision: logreg_decision's output, when the caller has it already."""
    z = logreg_decision(fit, queries) if decision is None else decision
    if fit["n_classes"] == 2:
        return (z[..., 0] > 0).long()
    return z.argmax(-1)


def stratified_subsample(labels, max_samples, seed=0):
    """Sorted row indices (numpy int64) of a stratified subsample of at most max_samples rows, every row when there
    are no more than that.  Class c keeps floor(max_samples * n_c / n) rows plus one for the largest remainders (ties
    to the lower class id); which rows: the first of numpy.random.RandomState(seed).permutation(n_c), classes drawn in
    ascending order."""
    import numpy as np
    y = np.asarray(labels.cpu() if isinstance(labels, torch.Tensor) else labels)
    n = len(y)
    if n <= max_samples:
        return np.arange(n, dtype=np.int64)
    classes, counts = np.unique(y, return_counts=True)
    share = max_samples * counts.astype(np.int64)
    take, rem = share // n, share % n
    for i in np.argsort(-rem, kind="stable")[:max_samples - int(take.sum())]:
        take[i] += 1
    rng = np.random.RandomState(seed)
    rows = [np.flatnonzero(y == c)[np.sort(rng.permutation(int(m))[:int(t)])] for c, m, t in zip(classes, counts, take)]
    return np.sort(np.concatenate(rows)).astype(np.int64)


@torch.no_grad()
def latent_linear_probe(splits, n_cycles, C=(1.0,), dataset="latent_vq_vae", vqvae=None, standardize=True, tol=1e-4,
                        max_iter=1000, max_samples=100000, window=200, seed=0, ts2vec=None):
    """Linear probe of a feature space: the reference's eval_protocol='linear' (fit_lr) on the features of
    latent_knn_probe.  A logistic regression per C is fitted on the train split (logreg_fit; above max_samples rows on
    a seeded stratified subsample, as fit_lr does) and scored on val and test.

    Returns {"per_C": [{"C", "val": m, "test": m}], "C_selected": the C with the best val F1 (the selection rule of
    the GRU path's val/f1_score_mean; ties to the smaller C), "val" / "test": m at that C plus "pred" (n,) int64 and
    "decision" (n, n_problems_per_C) f32 device tensors, "fit": logreg_fit's dict, "converged", "n_iter" (per C, over
    its problems)}, m = {acc, acc_good, acc_bad, f1} as latent_knn_probe reports them."""
    if dataset not in _DATASETS:
        raise ValueError(f"dataset: expected 'asimow' or 'latent_vq_vae', got {dataset!r}")
    if dataset == "latent_vq_vae" and vqvae is None:
        raise ValueError("vqvae: dataset latent_vq_vae needs the frozen VQ-VAE")
    _check_ts2vec(dataset, ts2vec)
    if isinstance(n_cycles, bool) or not isinstance(n_cycles, int) or n_cycles < 1:
        raise ValueError(f"n_cycles: expected a positive int, got {n_cycles!r}")
    Cs = _check_C(C)
    _check_fit_args(standardize, tol, max_iter)
    if isinstance(max_samples, bool) or not isinstance(max_samples, int) or max_samples < 1:
        raise ValueError(f"max_samples: expected a positive int, got {max_samples!r}")
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
        raise ValueError("splits: the train split is empty")

    dev = _device_of(*(x for x, _ in splits))
    keep = stratified_subsample(splits[0][1], max_samples, seed)
    if len(keep) < splits[0][0].shape[0]:
        rows = torch.as_tensor(keep, device=splits[0][0].device)
        splits[0] = (splits[0][0][rows], splits[0][1][rows.to(splits[0][1].device)])
    feats, labels = [], []
    for x, y in splits:
        x = x.to(dev).float()
        if dataset == "latent_vq_vae":
            from .data import latent_vectors
            x = latent_vectors(vqvae, x, n_cycles, window)
        elif dataset == "ts2vec":
            x = _ts2vec_features(ts2vec, x)
        feats.append(x.reshape(x.shape[0], -1))
        labels.append(y.to(dev).long())
    n_classes = max(2, max(int(y.max()) + 1 if y.numel() else 0 for y in labels))
    fit = logreg_fit(feats[0], labels[0], C=Cs, standardize=standardize, tol=tol, max_iter=max_iter,
                     n_classes=n_classes)
    dec = {nm: logreg_decision(fit, feats[i]) for i, nm in ((1, "val"), (2, "test"))}
    pred = {nm: logreg_predict(fit, None, decision=z) for nm, z in dec.items()}
    per_C = [{"C": c, **{nm: _metrics(pred[nm][ci], labels[i]) for i, nm in ((1, "val"), (2, "test"))}}
             for ci, c in enumerate(Cs)]
    best = None
    for ci in sorted(range(len(Cs)), key=lambda i: Cs[i]):
        if best is None or per_C[ci]["val"]["f1"] > per_C[best]["val"]["f1"]:
            best = ci
    out = {"per_C": per_C, "C_selected": Cs[best], "fit": fit,
           "converged": [bool(v) for v in fit["converged"].all(1).cpu()],
           "n_iter": [int(v) for v in fit["n_iter"].amax(1).cpu()]}
    for nm in ("val", "test"):
        out[nm] = {**per_C[best][nm], "pred": pred[nm][best], "decision": dec[nm][best]}
    return out


# ------------------------------------------------------------------------------------------------ RBF-SVM probe
MAX_SVM_ROWS = nat.AW_SVM_MAX_N
_SMO_CHUNK = 1024               # iterations per aw_svm_smo launch; the gaps are read once per launch
_SVM_MAX_ITER = 20000           # fit_svm's cap (SVC(max_iter=20_000)), per problem


def _check_gamma(gamma):
    if isinstance(gamma, str):
        if gamma != "scale":
            raise ValueError(f"gamma: expected 'scale' or a positive float, got {gamma!r}")
        return gamma
    if isinstance(gamma, bool) or not isinstance(gamma, (int, float)) or not 0 < float(gamma) < float("inf"):
        raise ValueError(f"gamma: expected 'scale' or a positive float, got {gamma!r}")
    return float(gamma)


@torch.no_grad()
def rbf_gamma(features):
    """scikit-learn's gamma='scale' of the features (n, ...): 1 / (D var), var the population variance over all
    elements, accumulated in f64 over row chunks on the features' device; 1.0 where the variance is 0.  A float."""
    if isinstance(features, torch.Tensor) and features.dim() >= 2 and features.shape[0] < 1:
        raise ValueError("features: no rows")
    x = _as_rows(features, "features")
    n, D = x.shape
    total = torch.zeros((), dtype=torch.float64, device=x.device)
    for o in range(0, n, _ROWS_PER_CHUNK):
        total += x[o:o + _ROWS_PER_CHUNK].double().sum()
    mean = total / (n * D)
    ss = torch.zeros_like(total)
    for o in range(0, n, _ROWS_PER_CHUNK):
        ss += ((x[o:o + _ROWS_PER_CHUNK].double() - mean) ** 2).sum()
    var = float(ss / (n * D))
    return 1.0 / (D * var) if var > 0 else 1.0


def svm_pairs(n_classes):
    """(positive class, negative class) of every problem: [(1, 0)] for two classes, else one-vs-one, every a < b as
    (a, b) in libsvm's order."""
    return [(1, 0)] if n_classes == 2 else [(a, b) for a in range(n_classes) for b in range(a + 1, n_classes)]


def _svm_rho(alpha, grad, y, C):
    """libsvm's calculate_rho per problem (rows of the (P, n) arguments; C (P,)): the mean of y G over the free rows,
    else the midpoint of the bounds the rows at the box give (a side without a bound takes the other's; neither: 0)."""
    yf = y.double()
    yG = yf * grad
    act = y != 0
    at_lo, at_up = act & (alpha <= 0), act & (alpha >= C[:, None])
    free = act & ~at_lo & ~at_up
    inf = torch.full_like(yG, float("inf"))
    ub = torch.where((at_up & (y < 0)) | (at_lo & (y > 0)), yG, inf).amin(1)
    lb = torch.where((at_up & (y > 0)) | (at_lo & (y < 0)), yG, -inf).amax(1)
    has_ub, has_lb = torch.isfinite(ub), torch.isfinite(lb)
    zero = torch.zeros_like(ub)
    mid = torch.where(has_ub & has_lb, (ub + lb) / 2, torch.where(has_ub, ub, torch.where(has_lb, lb, zero)))
    n_free = free.sum(1)
    mean_free = torch.where(free, yG, torch.zeros_like(yG)).sum(1) / n_free.clamp(min=1)
    return torch.where(n_free > 0, mean_free, mid)


@torch.no_grad()
def svm_fit(features, labels, C=0.1, gamma="scale", standardize=False, tol=1e-3, max_iter=_SVM_MAX_ITER,
            n_classes=None):
    """RBF support-vector classifier of labels on features: the reference's fit_svm (np.nan_to_num, NO scaler, then
    scikit-learn's SVC(kernel='rbf', gamma='scale', C=0.1, tol=1e-3, max_iter=20000)), fitted on the device
    (csrc/svm.hip): one Gram matrix (aw_rbf_gram), then libsvm's SMO on it (aw_svm_smo).

    features (n, ...) are flattened to (n, D), n <= 20480; labels (n,) integer class ids.  C: one value or a sequence;
    gamma: 'scale' (rbf_gamma of the features as fitted) or a positive float; the kernel uses its f32 value, which is
    what the fit reports.  standardize: the scaler of the other two probes, off by default as in fit_svm.  One problem
    per (class pair, C): two classes give the pair (1, 0) -- y = +1 for class 1 --, more classes every a < b
    (one-vs-one; rows of other classes are masked out of the pair's problem).  All problems share the Gram matrix and
    run 32 to a launch, in launches of a fixed iteration chunk, until every problem has gap = m - M <= tol or has run
    max_iter iterations; the gaps are read once per launch.
    Returns a dict: dual_coef (n_C, n_pairs, n) f64 = alpha y, rho (n_C, n_pairs) f64 (libsvm's rule), support (n_sv,)
    int64 -- the rows with any alpha > 0 -- and support_vectors (n_sv, D) f32, their features as the kernel saw them,
    gamma (float), mean and scale (D,) f64 (0 and 1 without standardize), C (n_C,) f64, pairs [(pos, neg)], n_iter,
    converged, gap, objective = 1/2 sum alpha (G - 1) and n_support, each (n_C, n_pairs), n_classes, standardize.
    Argument errors are ValueErrors naming the argument, raised before any device work; more than 20480 rows is one of
    them (subsample: latent_svm_probe's max_samples).
    Not offered: fit_svm's small-set branch (C = inf) and its 5-fold cross-validation over a one-point grid."""
    if isinstance(features, torch.Tensor) and features.dim() >= 2 and features.shape[0] < 1:
        raise ValueError("features: no rows to fit on")
    x = _as_rows(features, "features")
    Cs = _check_C(C)
    gamma = _check_gamma(gamma)
    _check_fit_args(standardize, tol, max_iter)
    if n_classes is not None and (isinstance(n_classes, bool) or not isinstance(n_classes, int) or n_classes < 2):
        raise ValueError(f"n_classes: expected None or an int >= 2, got {n_classes!r}")
    labels = torch.as_tensor(labels)
    if labels.dim() != 1 or labels.shape[0] != x.shape[0] or labels.is_floating_point() or labels.dtype == torch.bool:
        raise ValueError(f"labels: expected ({x.shape[0]},) integer class ids, got {labels.dtype} of shape "
                         f"{tuple(labels.shape)}")
    if x.shape[0] > MAX_SVM_ROWS:
        raise ValueError(f"features: {x.shape[0]} rows, the solver holds at most {MAX_SVM_ROWS}; fit on a subsample "
                         f"(latent_svm_probe's max_samples, stratified_subsample)")
    lo, hi = int(labels.min()), int(labels.max())
    if n_classes is None:
        n_classes = max(2, hi + 1)
    if lo < 0 or hi >= n_classes:
        raise ValueError(f"labels: class ids must lie in 0..{n_classes - 1}, got {lo}..{hi}")

    from . import kernels
    dev = _device_of(x)
    x = torch.nan_to_num(x.to(dev))
    n, D = x.shape
    if standardize:
        mean, scale = standard_scaler(x)
        x = _standardize(x, mean, scale)
    else:
        mean = torch.zeros(D, dtype=torch.float64, device=dev)
        scale = torch.ones(D, dtype=torch.float64, device=dev)
        x = x.float()
        x = x if x.stride(-1) == 1 else x.contiguous()
    g = rbf_gamma(x) if gamma == "scale" else gamma
    g = float(torch.tensor(g, dtype=torch.float32))            # the value the kernel receives
    if not 0 < g < float("inf"):
        raise ValueError(f"gamma: {gamma!r} is not a positive finite f32 value on these features")
    K = kernels.rbf_gram(x, x, g)

    pairs = svm_pairs(n_classes)
    lab = labels.to(dev)
    y_pairs = torch.stack([(lab == a).to(torch.int32) - (lab == b).to(torch.int32) for a, b in pairs])
    y = y_pairs.repeat(len(Cs), 1).contiguous()                # problem c * n_pairs + p
    Cp = [c for c in Cs for _ in pairs]
    P = len(Cp)
    alpha = torch.zeros((P, n), dtype=torch.float64, device=dev)
    grad = torch.full((P, n), -1.0, dtype=torch.float64, device=dev)
    n_iter = torch.zeros(P, dtype=torch.int64, device=dev)
    gap = torch.empty(P, dtype=torch.float64, device=dev)
    for o in range(0, P, MAX_PROBLEMS):
        sl = slice(o, o + MAX_PROBLEMS)
        ys, a_, g_, it_, gp_ = y[sl].contiguous(), alpha[sl], grad[sl], n_iter[sl], gap[sl]
        done = 0
        while True:
            step = min(_SMO_CHUNK, max_iter - done)
            kernels.svm_smo(K, ys, Cp[sl], tol, step, alpha=a_, grad=g_, n_iter=it_, gap=gp_)
            done += step
            if done >= max_iter or bool((gp_ <= tol).all()):    # the one read of the gaps per launch
                break
    Ct = torch.tensor(Cp, dtype=torch.float64, device=dev)
    act = y != 0
    shape = (len(Cs), len(pairs))
    support = torch.nonzero((alpha > 0).any(0)).flatten()
    return {"dual_coef": (alpha * y.double()).reshape(*shape, n), "rho": _svm_rho(alpha, grad, y, Ct).reshape(shape),
            "support": support, "support_vectors": x[support].contiguous(), "gamma": g, "mean": mean, "scale": scale,
            "C": torch.tensor(Cs, dtype=torch.float64, device=dev), "pairs": pairs,
            "n_iter": n_iter.reshape(shape), "converged": (gap <= tol).reshape(shape), "gap": gap.reshape(shape),
            "objective": (0.5 * torch.where(act, alpha * (grad - 1.0), torch.zeros_like(alpha)).sum(1)).reshape(shape),
            "n_support": (alpha > 0).sum(1).reshape(shape), "n_classes": n_classes, "standardize": standardize}


def _check_svm_fit(fit):
    need = {"dual_coef", "rho", "support", "support_vectors", "gamma", "mean", "scale", "pairs", "n_classes",
            "standardize"}
    if not isinstance(fit, dict) or not need <= set(fit):
        raise ValueError("fit: expected the dict svm_fit returns")
    return fit


@torch.no_grad()
def svm_decision(fit, queries):
    """Decision values (n_C, n, n_pairs) f64 of every fitted problem on the queries: aw_rbf_gram of query chunks
    against the support rows only, an f64 matmul with their dual coefficients, minus rho.  The queries go through
    nan_to_num and the fit's scaler as the training features did."""
    fit = _check_svm_fit(fit)
    q = _as_rows(queries, "queries")
    sv = fit["support_vectors"]
    if q.shape[1] != sv.shape[1]:
        raise ValueError(f"queries: {q.shape[1]} features per row, the fit has {sv.shape[1]}")
    from . import kernels
    dev = sv.device
    q = torch.nan_to_num(q.to(dev))
    if fit["standardize"]:
        q = _standardize(q, fit["mean"], fit["scale"])
    else:
        q = q.float()
        q = q if q.stride(-1) == 1 else q.contiguous()
    coef = fit["dual_coef"][:, :, fit["support"]]                               # (n_C, n_pairs, n_sv)
    nC, nP, nsv = coef.shape
    out = torch.empty((nC, q.shape[0], nP), dtype=torch.float64, device=dev)
    w = coef.reshape(nC * nP, nsv).t().contiguous()
    for o in range(0, q.shape[0], _ROWS_PER_CHUNK):
        rows = q[o:o + _ROWS_PER_CHUNK]
        if nsv:
            z = kernels.rbf_gram(rows, sv, fit["gamma"]).double() @ w           # (rows, n_C * n_pairs)
        else:
            z = torch.zeros((rows.shape[0], nC * nP), dtype=torch.float64, device=dev)
        out[:, o:o + _ROWS_PER_CHUNK] = z.reshape(rows.shape[0], nC, nP).permute(1, 0, 2)
    return out - fit["rho"][:, None, :]


@torch.no_grad()
def svm_predict(fit, queries, decision=None):
    """Class ids (n_C, n) int64.  Two classes: class 1 where the decision > 0.  More: the one-vs-one vote -- a pair
    votes for its positive class where its decision > 0, else for its negative one --, ties to the lowest class id.
    decision: svm_decision's output, when the caller has it already."""
    fit = _check_svm_fit(fit)
    z = svm_decision(fit, queries) if decision is None else decision
    K = fit["n_classes"]
    votes = torch.zeros((*z.shape[:2], K), dtype=torch.int64, device=z.device)
    for p, (a, b) in enumerate(fit["pairs"]):
        win = torch.where(z[..., p] > 0, a, b)
        votes.scatter_add_(2, win[..., None], torch.ones_like(win)[..., None])
    return votes.argmax(-1) if K > 2 else (votes[..., 1] > votes[..., 0]).long()


@torch.no_grad()
def latent_svm_probe(splits, n_cycles, C=(0.1,), gamma="scale", dataset="latent_vq_vae", vqvae=None,
                     standardize=False, tol=1e-3, max_iter=_SVM_MAX_ITER, max_samples=20000, window=200, seed=42,
                     ts2vec=None):
    """RBF-SVM probe of a feature space: the reference's eval_protocol='svm' (fit_svm) on the features of
    latent_knn_probe.  A support-vector classifier per C is fitted on the train split (svm_fit; above max_samples rows
    on a seeded stratified subsample, as fit_svm does above 20 000) and scored on val and test.

    Returns {"per_C": [{"C", "val": m, "test": m, "n_support"}], "C_selected": the C with the best val F1 (ties to the
    smaller C), "val" / "test": m at that C plus "pred" (n,) int64 and "decision" (n, n_pairs) f64 device tensors,
    "fit": svm_fit's dict, "gamma", "n_support", "converged", "n_iter" (per C, over its problems)}, m = {acc, acc_good,
    acc_bad, f1} as latent_knn_probe reports them.
    Not offered, and refused or left out on purpose: fit_svm's small-set branch (a train split of fewer than 50 rows,
    or fewer than 5 per class, which it fits with C = inf) is a ValueError; its 5-fold cross-validation is skipped, the
    grid having one point; the subsample is stratified_subsample's, not scikit-learn's rows."""
    if dataset not in _DATASETS:
        raise ValueError(f"dataset: expected 'asimow' or 'latent_vq_vae', got {dataset!r}")
    if dataset == "latent_vq_vae" and vqvae is None:
        raise ValueError("vqvae: dataset latent_vq_vae needs the frozen VQ-VAE")
    _check_ts2vec(dataset, ts2vec)
    if isinstance(n_cycles, bool) or not isinstance(n_cycles, int) or n_cycles < 1:
        raise ValueError(f"n_cycles: expected a positive int, got {n_cycles!r}")
    Cs = _check_C(C)
    gamma = _check_gamma(gamma)
    _check_fit_args(standardize, tol, max_iter)
    if isinstance(max_samples, bool) or not isinstance(max_samples, int) or not 1 <= max_samples <= MAX_SVM_ROWS:
        raise ValueError(f"max_samples: expected an int in 1..{MAX_SVM_ROWS}, got {max_samples!r}")
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
    n_train = splits[0][0].shape[0]
    if n_train < 1:
        raise ValueError("splits: the train split is empty")
    n_distinct = int(torch.unique(splits[0][1]).numel())
    if n_train < 50 or n_train // n_distinct < 5:
        raise ValueError(f"splits: a train split of {n_train} rows in {n_distinct} classes is the small set fit_svm "
                         f"fits with C = inf (fewer than 50 rows, or fewer than 5 per class): not offered")

    dev = _device_of(*(x for x, _ in splits))
    keep = stratified_subsample(splits[0][1], max_samples, seed)
    if len(keep) < n_train:
        rows = torch.as_tensor(keep, device=splits[0][0].device)
        splits[0] = (splits[0][0][rows], splits[0][1][rows.to(splits[0][1].device)])
    feats, labels = [], []
    for x, y in splits:
        x = x.to(dev).float()
        if dataset == "latent_vq_vae":
            from .data import latent_vectors
            x = latent_vectors(vqvae, x, n_cycles, window)
        elif dataset == "ts2vec":
            x = _ts2vec_features(ts2vec, x)
        feats.append(x.reshape(x.shape[0], -1))
        labels.append(y.to(dev).long())
    n_classes = max(2, max(int(y.max()) + 1 if y.numel() else 0 for y in labels))
    fit = svm_fit(feats[0], labels[0], C=Cs, gamma=gamma, standardize=standardize, tol=tol, max_iter=max_iter,
                  n_classes=n_classes)
    dec = {nm: svm_decision(fit, feats[i]) for i, nm in ((1, "val"), (2, "test"))}
    pred = {nm: svm_predict(fit, None, decision=z) for nm, z in dec.items()}
    n_sv = [int(v) for v in (fit["dual_coef"] != 0).any(1).sum(1).cpu()]
    per_C = [{"C": c, "n_support": n_sv[ci],
              **{nm: _metrics(pred[nm][ci], labels[i]) for i, nm in ((1, "val"), (2, "test"))}}
             for ci, c in enumerate(Cs)]
    best = None
    for ci in sorted(range(len(Cs)), key=lambda i: Cs[i]):
        if best is None or per_C[ci]["val"]["f1"] > per_C[best]["val"]["f1"]:
            best = ci
    out = {"per_C": per_C, "C_selected": Cs[best], "fit": fit, "gamma": fit["gamma"], "n_support": n_sv,
           "converged": [bool(v) for v in fit["converged"].all(1).cpu()],
           "n_iter": [int(v) for v in fit["n_iter"].amax(1).cpu()]}
    for nm in ("val", "test"):
        out[nm] = {**per_C[best][nm], "pred": pred[nm][best], "decision": dec[nm][best]}
    return out
