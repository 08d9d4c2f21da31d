"""fp64 numpy restatements of the k-NN search and of the probe's host side (arcweld.retrieve), for the CPU and the GPU
tests: all-pairs squared distances, eligibility, the (d, j) ranking, the class vote and the scaler.  Nothing here is
tuned to the code under test.

The bound eps(q, x, D).  The kernel evaluates d = fl(fl(|q|^2 + |x|^2) - 2 dot(q, x)) in f32: three sums of D products
each (two norms and the dot product; the f32-input MFMA is bit for bit an fmaf chain, one rounding per term), then two
more roundings.  With u = 2^-24 a sum of D terms accumulated in ANY order has error <= D u sum |terms| (to first
order; (1 + u)^D - 1 <= 1.01 D u for D u < 0.01), so |err(|q|^2)| <= D u |q|^2, |err(|x|^2)| <= D u |x|^2 and
|err(2 dot)| <= 2 D u sum |q_i x_i| <= D u (|q|^2 + |x|^2) (2 |a b| <= a^2 + b^2).  The two final roundings add at
most u (|q|^2 + |x|^2)(1 + ...) and u |d| <= 2 u (|q|^2 + |x|^2).  Together <= (2 D + 3 + slack) u (|q|^2 + |x|^2),
stated as eps = 2 (D + 4) u (|q|^2 + |x|^2): derived, not measured, and valid for every summation order.
"""
import numpy as np

U = 2.0 ** -24


def sqdist64(q, x):
    """(nq, nx) sum((q_i - x_j)^2) in f64 from the f32 values."""
    q, x = np.asarray(q, np.float64), np.asarray(x, np.float64)
    out = np.empty((len(q), len(x)))
    step = max(1, (1 << 22) // max(1, x.size))          # about 32 MB of differences at a time
    with np.errstate(all="ignore"):                     # NaN / inf rows are part of the tests
        for o in range(0, len(q), step):
            out[o:o + step] = ((q[o:o + step, None, :] - x[None, :, :]) ** 2).sum(-1)
    return out


def eps(q, x, D):
    """(nq, nx) bound on |d_f32(i, j) - d64(i, j)| (module docstring)."""
    q, x = np.asarray(q, np.float64), np.asarray(x, np.float64)
    return 2.0 * (D + 4) * U * ((q * q).sum(-1)[:, None] + (x * x).sum(-1)[None, :])


def eligible(nq, nx, q_group=None, x_group=None, d=None):
    """(nq, nx) bool: row j may be a neighbour of query i.  Equal groups are excluded when BOTH sides give groups; with
    distances d, only a finite distance is eligible (NaN / inf rows never are)."""
    ok = np.ones((nq, nx), bool)
    if q_group is not None and x_group is not None:
        ok &= np.asarray(q_group)[:, None] != np.asarray(x_group)[None, :]
    if d is not None:
        ok &= np.isfinite(d)
    return ok


def rank(d, ok, k):
    """idx (nq, k) int64 and dist (nq, k) f64: the eligible rows by ascending (d, j), (-1, +inf) past them."""
    nq, nx = d.shape
    idx = np.full((nq, k), -1, np.int64)
    dist = np.full((nq, k), np.inf)
    for i in range(nq):
        js = np.flatnonzero(ok[i])
        order = js[np.lexsort((js, d[i, js]))][:k]     # primary key d, then j
        idx[i, :len(order)] = order
        dist[i, :len(order)] = d[i, order]
    return idx, dist


def knn(q, x, k, q_group=None, x_group=None):
    d = sqdist64(q, x)
    return rank(d, eligible(len(q), len(x), q_group, x_group, d), k)


def vote(idx, dist, labels, n_classes=2, weights="uniform"):
    """pred (n,) and votes (n, n_classes) f64: scikit-learn's KNeighborsClassifier rule on given neighbours (-1 slots
    ignored; 'distance': 1 / dist, and a query with zero-distance neighbours lets only those vote, weight 1; ties to
    the lowest class; no neighbour at all: -1)."""
    n, k = idx.shape
    votes = np.zeros((n, n_classes))
    pred = np.full(n, -1, np.int64)
    for i in range(n):
        js = [(int(j), float(dd)) for j, dd in zip(idx[i], dist[i]) if j >= 0]
        if not js:
            continue
        if weights == "uniform":
            w = [1.0] * len(js)
        elif any(dd == 0 for _, dd in js):
            w = [1.0 if dd == 0 else 0.0 for _, dd in js]
        else:
            w = [1.0 / dd for _, dd in js]
        for (j, _), wi in zip(js, w):
            votes[i, int(labels[j])] += wi
        pred[i] = int(np.flatnonzero(votes[i] == votes[i].max())[0])
    return pred, votes


def scaler(x):
    """(mean, scale) f64 per feature: population standard deviation, 1 where the variance is 0."""
    x = np.asarray(x, np.float64)
    mean = x.mean(0)
    var = ((x - mean) ** 2).mean(0)
    return mean, np.where(var > 0, np.sqrt(var), 1.0)


def standardize(a, mean, scale):
    return ((np.asarray(a, np.float64) - mean) / scale).astype(np.float32)


def metrics(pred, target):
    """acc, acc_good (class 1), acc_bad (class 0), f1 (class 1) as model.classification_model defines them."""
    pred, target = np.asarray(pred), np.asarray(target)
    acc = float((pred == target).mean()) if len(target) else 0.0
    good, bad = target == 1, target == 0
    tp = float(((pred == 1) & good).sum())
    fp = float(((pred == 1) & ~good).sum())
    fn = float(((pred != 1) & good).sum())
    den = 2 * tp + fp + fn
    return {"acc": acc, "acc_good": float((pred[good] == 1).mean()) if good.any() else 0.0,
            "acc_bad": float((pred[bad] == 0).mean()) if bad.any() else 0.0, "f1": 2 * tp / den if den > 0 else 0.0}


def d32(q, x):
    """The kernel's distance expression restated in f32 numpy with in-order sums (one valid summation order): used on
    the CPU to check that eps really bounds an f32 evaluation."""
    q, x = np.asarray(q, np.float32), np.asarray(x, np.float32)
    D = q.shape[1]
    qq = np.zeros(len(q), np.float32)
    xx = np.zeros(len(x), np.float32)
    dot = np.zeros((len(q), len(x)), np.float32)
    for c in range(D):
        qq = (qq + q[:, c] * q[:, c]).astype(np.float32)
        xx = (xx + x[:, c] * x[:, c]).astype(np.float32)
        dot = (dot + q[:, c, None] * x[None, :, c]).astype(np.float32)
    s = (qq[:, None] + xx[None, :]).astype(np.float32)
    return (s - np.float32(2.0) * dot).astype(np.float32)
