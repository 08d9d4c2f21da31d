"""aw_window_sqerr (mean squared error per window, the second operand optionally gathered by row ids) against fp64:
planted differences land in their own window, equal windows give exactly 0, a bad id spoils only its window."""
import numpy as np
import pytest
import torch

from oracle import gen

pytestmark = pytest.mark.gpu

SHAPES = [(1, 1, 1), (5, 16, 16), (3, 200, 2), (4, 7, 33)]
TABLE = 32


def _run(a, b, idx=None):
    from arcweld import kernels as K
    W = a.shape[0]
    out = torch.full((W,), 7.0, device="cuda")
    bad = torch.zeros(1, dtype=torch.int32, device="cuda")
    K.window_sqerr(torch.as_tensor(a, device="cuda"), torch.as_tensor(b, device="cuda"), out, bad,
                   idx=None if idx is None else torch.as_tensor(idx, device="cuda"))
    return out.cpu().numpy(), int(bad.item())


def _inputs(shape, gather, seed):
    W, rows, width = shape
    a = gen.normal(seed, shape)
    if gather:
        b = gen.normal(seed + 1, (TABLE, width))
        idx = gen.randint(seed + 2, (W, rows), 0, TABLE)
        return a, b, idx, b[idx]
    b = gen.normal(seed + 1, shape)
    return a, b, None, b


@pytest.mark.parametrize("gather", [False, True], ids=["plain", "idx"])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_window_means_match_fp64(shape, gather):
    a, b, idx, bsel = _inputs(shape, gather, 6100 + sum(shape))
    got, bad = _run(a, b, idx)
    want = ((a.astype(np.float64) - bsel.astype(np.float64)) ** 2).mean(axis=(1, 2))
    assert bad == 0
    np.testing.assert_allclose(got, want, rtol=1e-4, atol=0)


@pytest.mark.parametrize("gather", [False, True], ids=["plain", "idx"])
@pytest.mark.parametrize("shape", SHAPES[1:], ids=lambda s: "x".join(map(str, s)))
def test_a_planted_difference_lands_in_its_own_window(shape, gather):
    W, rows, width = shape
    _, b, idx, bsel = _inputs(shape, gather, 6200 + sum(shape))
    a = bsel.copy()
    w, r, c = W - 2, rows - 1, width - 1                   # the last element of the last-but-one window
    a[w, r, c] += 2.0
    got, bad = _run(a, b, idx)
    d = float(np.float32(a[w, r, c]) - np.float32(bsel[w, r, c]))
    want = np.zeros(W)
    want[w] = d * d / (rows * width)
    assert bad == 0
    assert (np.delete(got, w) == 0.0).all()                # a == b gives exactly 0
    np.testing.assert_allclose(got[w], want[w], rtol=1e-4)


@pytest.mark.parametrize("shape", SHAPES[1:], ids=lambda s: "x".join(map(str, s)))
def test_an_id_outside_the_table_is_counted_and_spoils_only_its_window(shape):
    W, rows, width = shape
    a, b, idx, _ = _inputs(shape, True, 6300 + sum(shape))
    idx[1, rows // 2] = TABLE                              # one past the table
    idx[1, 0] = -1
    got, bad = _run(a, b, idx)
    assert bad == 2 and np.isnan(got[1])
    ok = idx.copy()
    ok[1] = 0
    want = ((a.astype(np.float64) - b[ok].astype(np.float64)) ** 2).mean(axis=(1, 2))
    keep = np.arange(W) != 1
    np.testing.assert_allclose(got[keep], want[keep], rtol=1e-4)
