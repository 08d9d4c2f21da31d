"""fp64 numpy restatements of aw_ensemble_stats' statistics (include/arcweld_amd.h), written independently of the
kernel's forms: numpy's own linear quantile, the CRPS as the pairwise double sum (the kernel takes the pair term from
the sorted samples), the coverage from whichever quantile arrays it is given.  x is (G, N, M): the samples on axis 1."""
import numpy as np


def mean_std(x):
    """(mean, unbiased std) over the samples, both (G, M) f64; the std of a single sample is 0."""
    x = np.asarray(x, dtype=np.float64)
    if x.shape[1] == 1:
        return x[:, 0].copy(), np.zeros_like(x[:, 0])
    return x.mean(axis=1), x.std(axis=1, ddof=1)


def quantiles(x, q):
    """(G, Q, M) f64: np.quantile(method="linear") at the probabilities q AS THE KERNEL SEES THEM (f32 values)."""
    x = np.asarray(x, dtype=np.float64)
    q64 = np.asarray(q, dtype=np.float32).astype(np.float64)
    if q64.size == 0:
        return np.empty((x.shape[0], 0, x.shape[2]))
    return np.moveaxis(np.quantile(x, q64, axis=1, method="linear"), 0, 1)


def quantile_is_order_statistic(N, q):
    """Per probability: is (N - 1) * q integral in f64, so that the quantile is one of the samples bit for bit?"""
    h = (N - 1) * np.asarray(q, dtype=np.float32).astype(np.float64)
    return h == np.floor(h)


def quantile_neighbours(x, q):
    """(lo, hi), each (G, Q, M) f64: the two order statistics an interpolated quantile lies between."""
    xs = np.sort(np.asarray(x, dtype=np.float64), axis=1)
    N = xs.shape[1]
    h = (N - 1) * np.asarray(q, dtype=np.float32).astype(np.float64)
    lo = np.floor(h).astype(np.int64)
    hi = np.minimum(lo + 1, N - 1)
    return xs[:, lo], xs[:, hi]


def crps_pairwise(x, y):
    """The ensemble CRPS of every point, (G, M) f64: mean_i |x_i - y| - 0.5 * mean_{i,j} |x_i - x_j|."""
    x, y = np.asarray(x, dtype=np.float64), np.asarray(y, dtype=np.float64)
    pair = np.stack([np.abs(xg[:, None, :] - xg[None, :, :]).mean(axis=(0, 1)) for xg in x])   # group by group
    return np.abs(x - y[:, None, :]).mean(axis=1) - 0.5 * pair


def crps_sorted(x, y):
    """The same value from the sorted samples, the form the kernel evaluates:
    mean_i |x_i - y| - (1 / N^2) sum_{i=1..N} (2 i - N - 1) x_(i)."""
    x, y = np.asarray(x, dtype=np.float64), np.asarray(y, dtype=np.float64)
    N = x.shape[1]
    w = 2.0 * np.arange(1, N + 1) - N - 1
    return np.abs(x - y[:, None, :]).mean(axis=1) - (w[None, :, None] * np.sort(x, axis=1)).sum(axis=1) / N ** 2


def segment_mean(c, seg):
    """(G, M) -> (G, M // seg): the mean over each run of seg points."""
    G, M = c.shape
    return c.reshape(G, M // seg, seg).mean(axis=2)


def coverage(q_lo, q_hi, y, seg):
    """(G, M // seg) f64: the share of each segment's points with q_lo <= y <= q_hi (arrays of shape (G, M))."""
    inside = (np.asarray(q_lo) <= np.asarray(y)) & (np.asarray(y) <= np.asarray(q_hi))
    G, M = inside.shape
    return inside.reshape(G, M // seg, seg).sum(axis=2) / float(seg)
