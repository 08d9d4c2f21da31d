"""fp64 numpy restatements of the DTW k-NN search (aw_dtw_knn, csrc/dtw.hip) and of what arcweld.retrieve builds on it,
for the CPU and the GPU tests.  Ranking, vote, scaler and metrics are knn_refs'.  Nothing here is tuned to the code
under test.

The distance (include/arcweld_amd.h).  Sequences q, x of shape (L, C); the band is Sakoe-Chiba with radius r: cell
(i, j) exists iff |i - j| <= r.  cost(i, j) = sum over the channels of (q[i][ch] - x[j][ch])^2; D(0, 0) = cost(0, 0),
otherwise D(i, j) = cost(i, j) + min(D(i-1, j-1), D(i-1, j), D(i, j-1)) with absent cells +inf; dtw = D(L-1, L-1).
Everything is vectorised over the (query, database row) pairs, one numpy step per cell.

The bound eps = 1.01 (2 L + C + 3) u dtw64, u = 2^-24, on |dtw_f32 - dtw64| for ANY evaluation order of the cells.
dtw64 is the minimum over the band's warping paths P of S(P) = sum of cost(i, j) over the cells of P; a path has at most
2 L - 1 cells.  The f32 program computes, for every cell, cost_f32 + min(...): unrolled along a path P it is the sum of
the path's f32 costs, accumulated from the path's first cell to its last with one rounding per addition.  Every term
is non-negative, so no cancellation occurs and each rounding multiplies the running sum by (1 + d), |d| <= u:
  - a cost passes through at most C + 3 roundings of relative size u before it enters the sum -- per channel one for
    the subtraction, whose relative error the square doubles, and one for the fmaf; the fmaf chain over the channels
    is again a sum of non-negative terms, so channel ch's term sees at most C - ch + 1 further factors.  Counting
    generously, every term of cost_f32 is its exact value times a product of at most C + 3 factors (1 + d): 2 for
    the squared difference, 1 for its own fmaf, at most C for the later fmafs of the chain;
  - a term then passes through at most 2 L - 1 additions of the path.
So S_f32(P) = sum of terms, each its exact value times at most 2 L + C + 2 factors: |S_f32(P) - S(P)| <=
((1 + u)^(2 L + C + 2) - 1) S(P) <= 1.01 (2 L + C + 3) u S(P) while (2 L + C + 3) u < 0.01.  The program takes the
minimum over predecessors of ROUNDED values, i.e. the minimum over paths of S_f32(P); a common relative factor
survives a minimum on both sides: min_P S_f32(P) <= S_f32(P*) <= (1 + e) S(P*) = (1 + e) dtw64 for the optimal P*,
and min_P S_f32(P) >= (1 - e) min_P S(P).  Hence |dtw_f32 - dtw64| <= e dtw64.  Derived, not measured; the CPU tests
check it against f32 evaluations in three orders.

Exactness on integers: with integer features in -4..4 every difference is an integer of magnitude <= 8, a cost at
most 64 C, a path sum at most (2 L - 1) 64 C; below 2^24 every f32 operation is exact in any order, so dtw_f32 equals
dtw64 bit for bit.
"""
import numpy as np

import knn_refs as K

U = 2.0 ** -24
ORDERS = ("row", "column", "antidiagonal")
_BYTES = 192 << 20          # the band arrays of one chunk of queries


def _cells(L, r, order):
    """The band's cells (i, j) in an order in which every cell comes after its three predecessors."""
    if order == "row":
        return [(i, j) for i in range(L) for j in range(max(0, i - r), min(L - 1, i + r) + 1)]
    if order == "column":
        return [(i, j) for j in range(L) for i in range(max(0, j - r), min(L - 1, j + r) + 1)]
    if order == "antidiagonal":
        return [(i, t - i) for t in range(2 * L - 1) for i in range(max(0, t - L + 1), min(L - 1, t) + 1)
                if abs(2 * i - t) <= r]
    raise ValueError(order)


def _dtw(q, x, radius, dtype, order):
    q, x = np.asarray(q, dtype), np.asarray(x, dtype)
    assert q.ndim == 3 and x.ndim == 3 and q.shape[1:] == x.shape[1:], (q.shape, x.shape)
    nq, L, C = q.shape
    nx = len(x)
    r = int(radius)
    assert 0 <= r <= L - 1
    W = 2 * r + 1
    out = np.empty((nq, nx), dtype)
    cells = _cells(L, r, order)
    step = max(1, _BYTES // max(1, 2 * L * W * max(nx, 1) * np.dtype(dtype).itemsize))
    inf = np.array(np.inf, dtype)
    with np.errstate(all="ignore"):                     # NaN / inf rows are part of the tests
        for o in range(0, nq, step):
            qc = q[o:o + step]
            n = len(qc)
            # cost[i, p] of cell (i, j = i - r + p), (n, nx) each: the fmaf chain over the channels.  numpy has no
            # fmaf; in f32 it is emulated as f32(f64(d) * f64(d) + f64(acc)) -- the product is exact in f64, the
            # sum carries one extra rounding at 2^-53, immaterial to the bound and absent on integers.
            cost = np.full((L, W, n, nx), np.inf, dtype)
            for i in range(L):
                lo, hi = max(0, i - r), min(L - 1, i + r)
                acc = np.zeros((hi - lo + 1, n, nx), dtype)
                for ch in range(C):
                    d = (qc[:, i, ch][None, :, None] - x[:, lo:hi + 1, ch].T[:, None, :]).astype(dtype)
                    if dtype == np.float32:
                        acc = (d.astype(np.float64) * d.astype(np.float64) + acc.astype(np.float64)).astype(dtype)
                    else:
                        acc = d * d + acc
                cost[i, lo - i + r:hi - i + r + 1] = acc
            D = np.full((L, W, n, nx), np.inf, dtype)

            def at(i, j):
                return D[i, j - i + r] if i >= 0 and j >= 0 and abs(i - j) <= r else inf

            for i, j in cells:
                if i == 0 and j == 0:
                    D[0, r] = cost[0, r]
                else:
                    m = np.minimum(np.minimum(at(i - 1, j - 1), at(i - 1, j)), at(i, j - 1))
                    D[i, j - i + r] = (cost[i, j - i + r] + m).astype(dtype)
            out[o:o + n] = D[L - 1, r]
    return out


def dtw64(q, x, radius):
    """(nq, nx) banded DTW of q (nq, L, C) against x (nx, L, C) in f64 from the f32 values (module docstring).  A NaN
    propagates through the minimum here; the kernel's distance for such a pair is non-finite as well."""
    return _dtw(np.asarray(q, np.float32), np.asarray(x, np.float32), radius, np.float64, "row")


def dtw32(q, x, radius, order="row"):
    """The same in f32 -- one rounding per subtraction, fmaf and addition -- with the cells evaluated in `order`."""
    return _dtw(np.asarray(q, np.float32), np.asarray(x, np.float32), radius, np.float32, order)


def eps(d64, L, C):
    """Bound on |dtw_f32 - dtw64| given dtw64 (module docstring)."""
    return 1.01 * (2 * L + C + 3) * U * np.asarray(d64, np.float64)


def knn(q, x, radius, k, q_group=None, x_group=None):
    """idx (nq, k) int64 and dist (nq, k) f64: the eligible rows by ascending (dtw64, j), (-1, +inf) past them."""
    if len(x) == 0:
        d = np.empty((len(q), 0))
    else:
        d = dtw64(q, x, radius)
    return K.rank(d, K.eligible(len(q), len(x), q_group, x_group, d), k)


def channel_scaler(x):
    """(mean, scale) f64 per channel of sequences x (n, L, C): knn_refs.scaler over all samples of all rows."""
    x = np.asarray(x)
    return K.scaler(x.reshape(-1, x.shape[-1]))


def standardize(a, mean, scale):
    """(n, L, C) f32: the per-channel scaler applied."""
    a = np.asarray(a)
    return K.standardize(a.reshape(-1, a.shape[-1]), mean, scale).reshape(a.shape)
