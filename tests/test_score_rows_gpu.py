"""aw_score_rows (teacher-forced scoring of lm-head logits in one launch) against an fp64 numpy restatement: the
target's log-probability, its rank (exact, on the same f32 logits), the entropy and the per-group sums, over row widths
on both sides of the register-row form; the rows and columns that must not be read, excluded columns, ties, bad rows."""
import numpy as np
import pytest
import torch

from oracle import gen

pytestmark = pytest.mark.gpu

TOL = 1e-4      # the project's fp32 parity bar (absolute)


def _pad8(v):
    return (v + 7) // 8 * 8


def _run(lg, tg, n_seq, seq_rows, groups, group_rows, n_valid=None, ldl=None, pad=float("nan")):
    """One launch on logits lg (n_seq * seq_rows, V) f32 laid out with row stride ldl (the padding filled with ``pad``):
    (logp, rank, entropy (n_seq, G), group_nll (n_seq, groups), bad count)."""
    from arcweld import kernels as K
    R, V = lg.shape
    buf = torch.full((R, ldl or V), pad, device="cuda")
    buf[:, :V] = torch.as_tensor(lg, device="cuda")
    G = groups * group_rows
    tgt = torch.as_tensor(tg, device="cuda").reshape(n_seq, G).contiguous()
    logp, ent = torch.full((n_seq, G), 7.0, device="cuda"), torch.full((n_seq, G), 7.0, device="cuda")
    rank = torch.full((n_seq, G), 7, device="cuda", dtype=torch.int32)
    nll = torch.full((n_seq, groups), 7.0, device="cuda")
    bad = torch.zeros(1, dtype=torch.int32, device="cuda")
    K.score_rows(buf[:, :V], tgt, seq_rows, groups, group_rows, logp, rank, ent, nll, bad, n_valid=n_valid)
    return logp.cpu().numpy(), rank.cpu().numpy(), ent.cpu().numpy(), nll.cpu().numpy(), int(bad.item())


def _ref(lg, tg, n_seq, seq_rows, groups, group_rows, n_valid):
    """fp64 scores of the scored rows over the allowed columns; the rank by comparison of the f32 logits themselves."""
    G = groups * group_rows
    l32 = np.asarray(lg, dtype=np.float32).reshape(n_seq, seq_rows, -1)[:, :G, :n_valid]
    tg = np.asarray(tg).reshape(n_seq, G)
    l = l32.astype(np.float64)
    with np.errstate(invalid="ignore", divide="ignore"):
        mx = l.max(-1, keepdims=True)
        lse = mx[..., 0] + np.log(np.exp(l - mx).sum(-1))
        logp = np.take_along_axis(l, tg[..., None], -1)[..., 0] - lse
        p = np.exp(l - lse[..., None])
        ent = lse - np.where(p > 0, p * l, 0.0).sum(-1)
    ly = np.take_along_axis(l32, tg[..., None], -1)
    rank = ((l32 > ly) | ((l32 == ly) & (np.arange(n_valid) < tg[..., None]))).sum(-1)
    return logp, rank, ent, -logp.reshape(n_seq, groups, group_rows).sum(-1)


SHAPES = [(1, 1, 1), (3, 3, 5), (2, 2, 16)]


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("padded", [False, True], ids=["ldl=V", "ldl=pad8"])
@pytest.mark.parametrize("drop", [0, 2], ids=["n_valid=V", "n_valid=V-2"])
@pytest.mark.parametrize("V", [34, 514, 8194])
def test_scores_match_fp64_and_the_rank_is_exact(V, drop, padded, shape):
    n_seq, groups, group_rows = shape
    seq_rows, n_valid = groups * group_rows + 1, V - drop
    lg = gen.normal(5100 + V + 7 * n_seq, (n_seq * seq_rows, V), std=3.0)
    tg = gen.randint(5101 + V + n_seq, (n_seq, groups * group_rows), 0, n_valid)
    args = (lg, tg, n_seq, seq_rows, groups, group_rows)
    logp, rank, ent, nll, bad = _run(*args, n_valid=n_valid, ldl=_pad8(V) if padded else V)
    wl, wr, we, wn = _ref(*args, n_valid)
    print(f"V {V} n_valid {n_valid} {shape}: max |logp - fp64| {np.abs(logp - wl).max():.3g}, |entropy - fp64| "
          f"{np.abs(ent - we).max():.3g}, |group_nll - fp64| {np.abs(nll - wn).max():.3g}")
    assert bad == 0
    assert rank.dtype == np.int32 and np.array_equal(rank, wr)
    assert np.abs(logp - wl).max() <= TOL
    assert np.abs(ent - we).max() <= TOL
    assert np.abs(nll - wn).max() <= group_rows * TOL
    again = _run(*args, n_valid=n_valid, ldl=_pad8(V) if padded else V)
    assert np.array_equal(nll.view(np.uint32), again[3].view(np.uint32))      # no float atomics: the same bits
    assert np.array_equal(logp.view(np.uint32), again[0].view(np.uint32))


@pytest.mark.parametrize("V", [34, 514, 8194])
def test_the_unscored_row_and_the_padding_columns_are_never_read(V):
    n_seq, groups, group_rows = 3, 2, 4
    seq_rows = groups * group_rows + 1
    lg = gen.normal(5200 + V, (n_seq * seq_rows, V), std=3.0)
    tg = gen.randint(5201 + V, (n_seq, groups * group_rows), 0, V)
    want = _ref(lg, tg, n_seq, seq_rows, groups, group_rows, V)
    lg.reshape(n_seq, seq_rows, V)[:, -1] = np.nan           # the position that predicts the end token
    logp, rank, ent, nll, bad = _run(lg, tg, n_seq, seq_rows, groups, group_rows, ldl=_pad8(V), pad=float("nan"))
    assert bad == 0
    assert np.isfinite(logp).all() and np.isfinite(ent).all() and np.isfinite(nll).all() and (rank >= 0).all()
    assert np.array_equal(rank, want[1]) and np.abs(logp - want[0]).max() <= TOL


@pytest.mark.parametrize("V", [34, 514, 8194])
def test_excluded_columns_do_not_change_ranks_or_logp(V):
    n_seq, groups, group_rows = 2, 1, 5
    seq_rows, n_valid = 6, V - 2
    lg = gen.normal(5300 + V, (n_seq * seq_rows, V), std=3.0)
    lg[:, V - 2] = lg.max() + 5.0            # the two largest logits of every row sit in the excluded columns
    lg[:, V - 1] = lg.max() + 1.0
    tg = gen.randint(5301 + V, (n_seq, groups * group_rows), 0, n_valid)
    logp, rank, ent, nll, bad = _run(lg, tg, n_seq, seq_rows, groups, group_rows, n_valid=n_valid)
    wl, wr, we, wn = _ref(lg[:, :n_valid], tg, n_seq, seq_rows, groups, group_rows, n_valid)
    assert bad == 0 and np.array_equal(rank, wr)
    assert np.abs(logp - wl).max() <= TOL and np.abs(ent - we).max() <= TOL
    assert np.abs(nll - wn).max() <= group_rows * TOL


@pytest.mark.parametrize("V", [34, 514, 8194])
def test_ties_break_low_as_the_greedy_pick_does(V):
    lg = gen.normal(5400 + V, (3, V), std=3.0)       # one sequence of 3 scored rows + none unscored: seq_rows = 3
    y, lo, hi = 17, 5, V - 3
    lg[0, lo] = lg[0, hi] = lg[0, y]                 # an exact tie with a lower and a higher column
    lg[1, y] = lg[1, hi] = lg[1].max() + 1.0         # the target ties the row maximum with a higher column: rank 0
    lg[2, lo] = lg[2, y] = lg[2].max() + 1.0         # ... and here with a lower one: rank 1
    tg = np.full((1, 3), y, dtype=np.int64)
    _, rank, _, _, bad = _run(lg, tg, 1, 3, 1, 3)
    strictly_above = int((lg[0] > lg[0, y]).sum())
    assert bad == 0 and rank.tolist() == [[strictly_above + 1, 0, 1]]
    assert np.array_equal(rank, _ref(lg, tg, 1, 3, 1, 3, V)[1])


@pytest.mark.parametrize("V", [34, 514, 8194])
def test_bad_rows_are_counted_and_marked_and_leave_the_rest_alone(V):
    n_seq, groups, group_rows = 2, 3, 4
    G = groups * group_rows
    seq_rows, n_valid = G + 1, V - 2
    lg = gen.normal(5500 + V, (n_seq * seq_rows, V), std=3.0)
    tg = gen.randint(5501 + V, (n_seq, G), 0, n_valid)
    l3 = lg.reshape(n_seq, seq_rows, V)
    l3[0, 1, n_valid - 1] = np.nan           # (0, 1): a NaN in an allowed column           -> group (0, 0)
    l3[0, 9, :] = -np.inf                    # (0, 9): no finite value                      -> group (0, 2)
    tg[1, 2] = n_valid                       # (1, 2): target one past the allowed ids      -> group (1, 0)
    tg[1, 6] = -1                            # (1, 6): negative target                      -> group (1, 1)
    l3[1, 8, tg[1, 8]] = -np.inf             # (1, 8): a -inf TARGET logit in a finite row: logp -inf, not bad
    l3[1, 9, V - 1] = np.nan                 # a NaN in an EXCLUDED column is not seen
    logp, rank, ent, nll, bad = _run(lg, tg, n_seq, seq_rows, groups, group_rows, n_valid=n_valid)
    assert bad == 4
    bad_rows = np.zeros((n_seq, G), dtype=bool)
    for b, t in ((0, 1), (0, 9), (1, 2), (1, 6)):
        bad_rows[b, t] = True
    assert np.isnan(logp[bad_rows]).all() and np.isnan(ent[bad_rows]).all() and (rank[bad_rows] == -1).all()
    bad_groups = np.array([[True, False, True], [True, True, False]])
    assert np.isnan(nll[bad_groups]).all() and not np.isnan(nll[~bad_groups]).any()
    # every other row against the reference (on inputs whose bad rows are made harmless first)
    lg_ok, tg_ok = lg.copy(), tg.copy()
    lg_ok.reshape(n_seq, seq_rows, V)[0, 1, n_valid - 1] = 0.0
    lg_ok.reshape(n_seq, seq_rows, V)[0, 9, :] = 0.0
    tg_ok[1, 2] = tg_ok[1, 6] = 0
    wl, wr, we, wn = _ref(lg_ok, tg_ok, n_seq, seq_rows, groups, group_rows, n_valid)
    ok = ~bad_rows
    assert logp[1, 8] == -np.inf and wl[1, 8] == -np.inf and nll[1, 2] == np.inf
    ok[1, 8] = False
    assert np.array_equal(rank[~bad_rows], wr[~bad_rows])
    assert np.abs(logp[ok] - wl[ok]).max() <= TOL and np.abs(ent[~bad_rows] - we[~bad_rows]).max() <= TOL
    assert np.abs(nll[0, 1] - wn[0, 1]) <= group_rows * TOL


def test_argument_errors_launch_nothing():
    from arcweld import _native, kernels as K
    lg = torch.zeros(6, 10, device="cuda")
    tg = torch.zeros(2, 2, dtype=torch.int64, device="cuda")
    f = lambda *s: torch.empty(*s, device="cuda")  # noqa: E731
    rank, bad = torch.empty(2, 2, dtype=torch.int32, device="cuda"), torch.zeros(1, dtype=torch.int32, device="cuda")
    with pytest.raises(_native.NativeError):
        K.score_rows(lg, tg, 3, 1, 2, f(2, 2), rank, f(2, 2), f(2, 1), bad, n_valid=11)     # n_valid > V
    with pytest.raises(_native.NativeError):
        K.score_rows(lg, tg, 3, 2, 2, f(2, 4), rank, f(2, 4), f(2, 2), bad)                 # 4 rows of a 3-row sequence
    assert int(bad.item()) == 0
