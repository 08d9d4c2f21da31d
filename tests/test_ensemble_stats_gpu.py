"""aw_ensemble_stats (pointwise mean / std / quantiles over an ensemble, CRPS and band coverage per segment, one launch)
against the fp64 restatements of tests/ensemble_refs.py at the smallest shapes where it can still go wrong: sample
counts around the sort's and the LDS limit's edges, segments below, at and above one workgroup's stride of 256 points,
several segments and groups, every quantile count.  Every buffer the kernel touches sits between canary margins (the
inputs between NaNs: a read outside them would surface as a bad point).

Tolerances.  Order statistics (an integral (N - 1) q) are bit-exact.  An interpolated quantile is one f32 subtract and
one fused multiply-add on exact operands: within 2 f32 ulps of max(|x_lo|, |x_hi|).  mean, std and crps are f64 sums of
f32 data rounded once to f32 (6e-8 relative) plus f64 reordering: rtol 1e-6, atol 1e-7, about 16 f32 ulps -- a wrong
divisor or a dropped sample misses that by orders of magnitude.  cover is a count divided by seg: exact, against the
restatement applied to the kernel's own stored quantiles."""
import numpy as np
import pytest
import torch

import ensemble_refs as R
from oracle import gen

pytestmark = pytest.mark.gpu

PAD = 64
CANARY = -1234.5
RTOL, ATOL = 1e-6, 1e-7

QS = {0: (), 1: (0.5,), 3: (0.05, 0.5, 0.95), 8: (0.0, 0.05, 0.25, 0.5, 0.5, 0.75, 0.95, 1.0)}


class _Out:
    """A float32 output of ``shape`` inside a canary-filled buffer."""

    def __init__(self, *shape):
        self.n = int(np.prod(shape))
        self.buf = torch.full((self.n + 2 * PAD,), CANARY, device="cuda")
        self.t = self.buf[PAD:PAD + self.n].view(*shape)

    def margins_intact(self):
        return bool((self.buf[:PAD] == CANARY).all() and (self.buf[PAD + self.n:] == CANARY).all())

    def untouched(self):
        return bool((self.buf == CANARY).all())

    def numpy(self):
        return self.t.cpu().numpy()


def _inside_nans(a, off):
    """The array on the device inside a NaN-filled buffer, starting ``off`` floats (4 * off bytes) into it."""
    a = np.ascontiguousarray(a, dtype=np.float32)
    buf = torch.full((a.size + off + PAD,), float("nan"), device="cuda")
    view = buf[off:off + a.size].view(*a.shape)
    view.copy_(torch.as_tensor(a))
    assert view.is_contiguous() and view.data_ptr() % 16 == (4 * off) % 16
    return view


def _run(x, q, y=None, seg=None, x_off=4, want_mean=True, want_std=True):
    """One launch; returns a dict of numpy outputs (None where not asked for) and the bad count, after checking that no
    canary margin changed."""
    from arcweld import kernels as K
    G, N, M = x.shape
    Q = len(q)
    seg = M if seg is None else seg
    o = {"mean": _Out(G, M) if want_mean else None, "std": _Out(G, M) if want_std else None,
         "quant": _Out(G, Q, M) if Q else None,
         "crps": _Out(G, M // seg) if y is not None else None,
         "cover": _Out(G, M // seg) if y is not None and Q >= 2 else None}
    bad = torch.zeros(1, dtype=torch.int32, device="cuda")
    t = lambda k: None if o[k] is None else o[k].t  # noqa: E731
    K.ensemble_stats(_inside_nans(x, x_off), q, mean=t("mean"), std=t("std"), quant=t("quant"),
                     y=None if y is None else _inside_nans(y, 1), seg=seg, crps=t("crps"), cover=t("cover"),
                     bad_count=bad)
    torch.cuda.synchronize()
    for k, v in o.items():
        assert v is None or v.margins_intact(), f"{k}: a canary margin was written"
    return {k: None if v is None else v.numpy() for k, v in o.items()}, int(bad.item())


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _close(got, want):
    return bool((np.abs(got.astype(np.float64) - want) <= ATOL + RTOL * np.abs(want)).all())


def _check(out, x, q, y, seg, label=""):
    """Every output of one launch against the restatements (the tolerances of the module docstring)."""
    G, N, M = x.shape
    mean, std = R.mean_std(x)
    print(f"{label} max |mean - fp64| {np.abs(out['mean'] - mean).max():.3g}, |std - fp64| "
          f"{np.abs(out['std'] - std).max():.3g}")
    assert _close(out["mean"], mean) and _close(out["std"], std)
    if len(q):
        got, want = out["quant"], R.quantiles(x, q)
        exact = R.quantile_is_order_statistic(N, q)
        lo, hi = R.quantile_neighbours(x, q)
        ulp = np.spacing(np.maximum(np.abs(lo), np.abs(hi)).astype(np.float32)).astype(np.float64)
        err = np.abs(got.astype(np.float64) - want) / ulp
        print(f"{label} interpolated quantiles: max error {err[:, ~exact].max() if (~exact).any() else 0.0:.3g} ulp")
        assert np.array_equal(_bits(got[:, exact]), _bits(want[:, exact].astype(np.float32)))
        assert (err[:, ~exact] <= 2.0).all()
    if y is not None:
        crps = R.segment_mean(R.crps_pairwise(x, y), seg)
        print(f"{label} max |crps - fp64| {np.abs(out['crps'] - crps).max():.3g}")
        assert _close(out["crps"], crps)
        if len(q) >= 2:
            cover = R.coverage(out["quant"][:, 0], out["quant"][:, -1], y, seg).astype(np.float32)
            assert np.array_equal(_bits(out["cover"]), _bits(cover))


def _cases():
    """N x seg, the other axes cycled so that every value of G, M / seg and Q meets several N and seg."""
    cases = []
    for i, N in enumerate((1, 2, 3, 31, 32, 33, 64)):
        for j, seg in enumerate((1, 7, 400, 1000)):
            G, n_seg, Q = (1, 3)[(i // 2 + j) % 2], (3, 1)[(i + j // 2) % 2], (0, 1, 3, 8)[(i + j) % 4]
            cases.append(pytest.param(N, seg, n_seg, G, Q, id=f"N{N}-seg{seg}x{n_seg}-G{G}-Q{Q}"))
    return cases


@pytest.mark.parametrize("N,seg,n_seg,G,Q", _cases())
def test_statistics_match_fp64_and_are_the_same_bits_every_launch(N, seg, n_seg, G, Q):
    M = seg * n_seg
    x = gen.normal(7200 + 131 * N + seg, (G, N, M), std=2.0, mean=0.5)
    y = gen.normal(7201 + 131 * N + seg, (G, M), std=2.5, mean=0.5)
    out, bad = _run(x, QS[Q], y, seg)
    assert bad == 0
    _check(out, x, QS[Q], y, seg, label=f"N {N} seg {seg} x {n_seg} G {G} Q {Q}:")
    again, _ = _run(x, QS[Q], y, seg)
    for k, v in out.items():
        assert v is None or np.array_equal(_bits(v), _bits(again[k])), k       # no float atomics: the same bits


@pytest.mark.parametrize("Q", [0, 3])
def test_without_a_truth_only_the_pointwise_statistics_are_written(Q):
    x = gen.normal(7300 + Q, (2, 5, 21), std=2.0)
    out, bad = _run(x, QS[Q], None, 7)
    assert bad == 0 and out["crps"] is None and out["cover"] is None
    _check(out, x, QS[Q], None, 7)
    only_q, bad = _run(x, QS[3], None, 7, want_mean=False, want_std=False)      # mean and std are optional
    assert bad == 0 and np.array_equal(_bits(only_q["quant"]), _bits(_run(x, QS[3], None, 7)[0]["quant"]))


def test_a_misaligned_x_and_a_row_length_that_is_no_multiple_of_4():
    """M = 7; x starts 4 bytes off a 16-byte boundary, its neighbours are NaN: nothing outside x is read."""
    x = gen.normal(7400, (3, 3, 7), std=2.0)
    y = gen.normal(7401, (3, 7), std=2.0)
    out, bad = _run(x, QS[8], y, 7, x_off=1)
    assert bad == 0
    _check(out, x, QS[8], y, 7)
    aligned, _ = _run(x, QS[8], y, 7, x_off=4)
    for k, v in out.items():
        assert np.array_equal(_bits(v), _bits(aligned[k])), k


@pytest.mark.parametrize("N", [2, 5, 32])
def test_ties(N):
    G, M, seg, q = 2, 14, 7, QS[8]
    y = gen.normal(7500 + N, (G, M), std=2.0)
    point = gen.normal(7501 + N, (G, 1, M), std=2.0)
    x = np.repeat(point, N, axis=1)                       # every sample equal
    out, bad = _run(x, q, y, seg)
    assert bad == 0 and not out["std"].any()
    assert np.array_equal(_bits(out["mean"]), _bits(point[:, 0]))
    for k in range(len(q)):
        assert np.array_equal(_bits(out["quant"][:, k]), _bits(point[:, 0])), k
    assert _close(out["crps"], R.segment_mean(np.abs(point[:, 0].astype(np.float64) - y), seg))
    x = gen.normal(7502 + N, (G, N, M), std=2.0)          # duplicated pairs among distinct values
    x[:, N - 1] = x[:, 0]
    x[:, N // 2] = x[:, 0]
    out, bad = _run(x, q, y, seg)
    assert bad == 0
    _check(out, x, q, y, seg)


def test_bad_points_are_marked_and_counted_and_leave_the_rest_alone():
    G, N, seg, n_seg, q = 2, 5, 7, 3, QS[3]
    M = seg * n_seg
    x = gen.normal(7600, (G, N, M), std=2.0)
    y = gen.normal(7601, (G, M), std=2.0)
    clean, bad = _run(x, q, y, seg)
    assert bad == 0
    xb, yb = x.copy(), y.copy()
    xb[0, 2, 3] = np.nan              # point (0, 3)  -> segment (0, 0)
    xb[1, 0, 15] = np.inf             # point (1, 15) -> segment (1, 2)
    yb[1, 8] = np.nan                 # point (1, 8)  -> segment (1, 1)
    out, bad = _run(xb, q, yb, seg)
    assert bad == 3
    pts = np.zeros((G, M), dtype=bool)
    pts[0, 3] = pts[1, 15] = pts[1, 8] = True
    segs = np.zeros((G, n_seg), dtype=bool)
    segs[0, 0] = segs[1, 2] = segs[1, 1] = True
    for k in ("mean", "std"):
        assert np.isnan(out[k][pts]).all(), k
        assert np.array_equal(_bits(out[k][~pts]), _bits(clean[k][~pts])), k
    for j in range(len(q)):
        assert np.isnan(out["quant"][:, j][pts]).all()
        assert np.array_equal(_bits(out["quant"][:, j][~pts]), _bits(clean["quant"][:, j][~pts]))
    for k in ("crps", "cover"):
        assert np.isnan(out[k][segs]).all(), k
        assert np.array_equal(_bits(out[k][~segs]), _bits(clean[k][~segs])), k
    # without a truth the NaN in y does not exist: two bad points
    out, bad = _run(xb, q, None, seg)
    assert bad == 2 and np.isnan(out["mean"]).sum() == 2


def test_argument_errors_launch_nothing():
    from arcweld import _native, kernels as K
    bad = torch.zeros(1, dtype=torch.int32, device="cuda")
    x = lambda *s: torch.zeros(*s, device="cuda")  # noqa: E731

    def refused(xs, q, seg=None, y=False, crps=False, cover=False, quant=True, n_seg=None):
        G, N, M = xs
        outs = {"mean": _Out(G, M), "std": _Out(G, M), "quant": _Out(G, len(q), M) if quant and len(q) else None,
                "crps": _Out(G, n_seg) if crps else None, "cover": _Out(G, n_seg) if cover else None}
        t = {k: None if v is None else v.t for k, v in outs.items()}
        with pytest.raises(_native.NativeError, match="aw_ensemble_stats"):
            K.ensemble_stats(x(*xs), q, y=x(G, M) if y else None, seg=seg, bad_count=bad, **t)
        torch.cuda.synchronize()
        for k, v in outs.items():
            assert v is None or v.untouched(), k

    refused((1, 0, 4), (0.5,))                                        # N outside 1..64
    refused((1, 65, 4), (0.5,))
    refused((1, 3, 4), tuple(i / 10 for i in range(9)))               # Q outside 0..8
    for q in (1.5, -0.1, float("nan")):                               # a q outside [0, 1] or NaN
        refused((1, 3, 4), (0.5, q))
    refused((1, 3, 10), (0.1, 0.9), seg=4, y=True, crps=True, n_seg=2)        # M % seg != 0
    refused((1, 3, 4), (0.5,), seg=0)                                 # seg < 1
    refused((1, 3, 4), (0.5,), seg=-2)
    refused((1, 3, 4), (0.5,), seg=2, y=True, cover=True, n_seg=2)    # cover with Q < 2
    refused((1, 3, 4), (0.1, 0.9), seg=2, crps=True, n_seg=2)         # crps without y
    refused((1, 3, 4), (0.1, 0.9), seg=2, cover=True, n_seg=2)        # cover without y
    refused((1, 3, 4), (0.1, 0.9), quant=False)                       # quant NULL with Q > 0
    with pytest.raises(_native.NativeError, match="float32"):         # the binding's own checks
        K.ensemble_stats(x(1, 3, 4).double(), (), bad_count=bad)
    with pytest.raises(_native.NativeError, match="shape"):
        K.ensemble_stats(x(1, 3, 4), (), mean=x(1, 5), bad_count=bad)
    with pytest.raises(_native.NativeError, match="bad_count"):
        K.ensemble_stats(x(1, 3, 4), ())
    # empty input: fine, nothing launched
    m = _Out(2, 4)
    K.ensemble_stats(x(0, 3, 4), (), mean=x(0, 4), seg=2, bad_count=bad)
    K.ensemble_stats(x(2, 3, 0), (), mean=x(2, 0), seg=1, bad_count=bad)
    torch.cuda.synchronize()
    assert m.untouched() and int(bad.item()) == 0
