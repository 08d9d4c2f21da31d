"""The three beam-search launches alone: aw_beam_step against an f64 numpy restatement (log-softmax, add the beam
score, stable sort by (-cand, flat index)), aw_beam_gather against index_select, aw_beam_backtrack against a Python
walk."""
import numpy as np
import pytest
import torch

from oracle import gen

pytestmark = pytest.mark.gpu

NEG = -np.inf


def ref_beam_step(logits, scores, n_valid, W_out):
    """logits (B, W_in, V), scores (B, W_in) -> cand (B, W_in * n_valid) f64, and per kept slot (B, W_out): order
    (flat index), score, logp.  Slots past the candidates that exist: index -1, score and logp -inf."""
    l = logits[:, :, :n_valid].astype(np.float64)
    mx = l.max(-1, keepdims=True)
    with np.errstate(divide="ignore", invalid="ignore"):
        logp = l - (mx + np.log(np.exp(l - mx).sum(-1, keepdims=True)))
        cand = (scores.astype(np.float64)[:, :, None] + logp).reshape(len(l), -1)
    order = np.argsort(-cand, axis=1, kind="stable")
    B, N = cand.shape
    idx = np.full((B, W_out), -1, dtype=np.int64)
    sc = np.full((B, W_out), NEG)
    lp = np.full((B, W_out), NEG)
    k = min(W_out, N)
    idx[:, :k] = order[:, :k]
    sc[:, :k] = np.take_along_axis(cand, order[:, :k], 1)
    lp[:, :k] = np.take_along_axis(logp.reshape(B, -1), order[:, :k], 1)
    return cand, idx, sc, lp


def top_gap(cand, W_out):
    """The smallest distance between two of the candidates ranked 1 .. W_out + 1 (sorted: neighbours suffice)."""
    top = -np.sort(-cand, axis=1)[:, :W_out + 1]
    return np.abs(np.diff(top, axis=1)).min()


def run_step(logits, scores, n_valid, W_out, ldl=None):
    """logits (B, W_in, V) / scores (B, W_in) numpy -> scores, parent, token, logp (B, W_out) numpy and bad_count."""
    from arcweld import kernels as K
    B, W_in, V = logits.shape
    ldl = V if ldl is None else ldl
    buf = torch.full((B * W_in, ldl), float("nan"), device="cuda")       # the padding columns must never be read
    buf[:, :V] = torch.tensor(logits.reshape(B * W_in, V))
    sc = torch.empty(B, W_out, device="cuda")
    lp = torch.empty(B, W_out, device="cuda")
    pa = torch.full((B, W_out), -7, dtype=torch.int32, device="cuda")
    tk = torch.full((B * W_out,), -7, dtype=torch.int64, device="cuda")
    bad = torch.zeros(1, dtype=torch.int32, device="cuda")
    K.beam_step(buf[:, :V], torch.tensor(scores, device="cuda"), sc, pa, tk, lp, bad, n_valid=n_valid)
    return (sc.cpu().numpy(), pa.cpu().numpy(), tk.view(B, W_out).cpu().numpy(), lp.cpu().numpy(), int(bad.item()))


# seed, B, W_in, W_out, V, n_valid, ldl: the issue's case, the largest LDS image (32 beams x 512 codes), W_in = 1 (the
# first step of a search), and the middle image (N = 4 * 514 in 1025..4096)
RANDOM_CASES = {
    "small": (4101, 3, 4, 4, 37, 33, 40),
    "largest": (4102, 3, 32, 32, 514, 512, 514),
    "first_step": (4103, 3, 1, 4, 37, 33, 40),
    "middle": (4104, 2, 4, 8, 514, 514, 520),
}


@pytest.mark.parametrize("case", list(RANDOM_CASES))
def test_random_candidates_match_the_f64_ranking(case):
    """|cand| < 64 has an f32 ulp of 7.6e-6 and the kernel a handful of roundings, so candidates more than 1e-4 apart in
    f64 cannot swap places: the ranking must be exact, the values within the project's 1e-4 kernel bar.  Measured on
    an MI355X: 5.9e-7 at most for scores and logp, the smallest gap 7.4e-4 (the largest image)."""
    seed, B, W_in, W_out, V, n_valid, ldl = RANDOM_CASES[case]
    logits = gen.normal(seed, (B, W_in, V), 3.0)
    scores = gen.normal(seed + 50, (B, W_in), 1.0)
    cand, idx, want_sc, want_lp = ref_beam_step(logits, scores, n_valid, W_out)
    gap = top_gap(cand, W_out)
    print(f"{case}: smallest gap among the ranks 1..{W_out + 1}: {gap:.3e}, max |cand| {np.abs(cand).max():.1f}")
    assert gap > 1e-4 and np.abs(want_sc).max() < 64
    sc, pa, tk, lp, bad = run_step(logits, scores, n_valid, W_out, ldl)
    assert bad == 0
    assert np.array_equal(pa, idx // n_valid) and np.array_equal(tk, idx % n_valid)
    print(f"{case}: max score error {np.abs(sc - want_sc).max():.2e}, max logp error {np.abs(lp - want_lp).max():.2e}")
    assert np.abs(sc - want_sc).max() <= 1e-4 and np.abs(lp - want_lp).max() <= 1e-4
    again = run_step(logits, scores, n_valid, W_out, ldl)
    for x, y in zip((sc, pa, tk, lp), again):                      # the same bits on every launch
        assert np.array_equal(x.view(np.int32) if x.dtype == np.float32 else x,
                              y.view(np.int32) if y.dtype == np.float32 else y)


def test_exact_ties_break_by_the_lower_flat_index():
    logits = gen.normal(4111, (2, 3, 20), 3.0)
    logits[:, 1] = logits[:, 0]                                     # beams 0 and 1: identical rows, equal scores
    scores = np.array([[0.5, 0.5, -30.0], [-1.0, -1.0, -40.0]], dtype=np.float32)
    sc, pa, tk, lp, bad = run_step(logits, scores, 17, 4)
    assert bad == 0
    for b in range(2):
        v = np.argsort(-logits[b, 0, :17].astype(np.float64), kind="stable")[:2]
        assert pa[b].tolist() == [0, 1, 0, 1] and tk[b].tolist() == [v[0], v[0], v[1], v[1]]
        assert sc[b, 0] == sc[b, 1] and sc[b, 2] == sc[b, 3] and sc[b, 1] > sc[b, 2]
    _, idx, want_sc, _ = ref_beam_step(logits, scores, 17, 4)
    assert np.array_equal(pa * 17 + tk, idx) and np.abs(sc - want_sc).max() <= 1e-4


def test_dead_beams_fill_the_tail_by_the_same_tie_rule():
    logits = gen.normal(4112, (2, 4, 5), 3.0)
    scores = np.array([[0.0, NEG, NEG, NEG]] * 2, dtype=np.float32)
    sc, pa, tk, lp, bad = run_step(logits, scores, 3, 4)
    assert bad == 0
    for b in range(2):
        order = np.argsort(-logits[b, 0, :3].astype(np.float64), kind="stable")
        assert pa[b].tolist() == [0, 0, 0, 1] and tk[b].tolist() == order.tolist() + [0]
        assert np.isfinite(sc[b, :3]).all() and sc[b, 0] >= sc[b, 1] >= sc[b, 2] and sc[b, 3] == NEG
    _, _, want_sc, want_lp = ref_beam_step(logits, scores, 3, 4)
    assert np.abs(sc[:, :3] - want_sc[:, :3]).max() <= 1e-4 and np.abs(lp - want_lp).max() <= 1e-4


def test_more_slots_than_candidates_leaves_dead_beams():
    """W_in * n_valid = 3 candidates for 5 slots (the first step of a search wider than the vocabulary)."""
    logits = gen.normal(4113, (2, 1, 6), 3.0)
    sc, pa, tk, lp, bad = run_step(logits, np.zeros((2, 1), dtype=np.float32), 3, 5)
    assert bad == 0
    for b in range(2):
        order = np.argsort(-logits[b, 0, :3].astype(np.float64), kind="stable")
        assert tk[b].tolist() == order.tolist() + [0, 0] and pa[b].tolist() == [0] * 5
        assert (sc[b, 3:] == NEG).all() and (lp[b, 3:] == NEG).all() and np.isfinite(sc[b, :3]).all()


def test_a_minus_inf_column_is_never_chosen_while_finite_ones_remain():
    logits = gen.normal(4114, (2, 2, 12), 3.0)
    logits[:, :, [1, 4, 7]] = NEG
    scores = gen.normal(4115, (2, 2), 1.0)
    sc, pa, tk, lp, bad = run_step(logits, scores, 10, 8)           # 2 * 7 = 14 finite candidates for 8 slots
    assert bad == 0 and np.isfinite(sc).all() and not np.isin(tk, [1, 4, 7]).any()
    _, idx, want_sc, _ = ref_beam_step(logits, scores, 10, 8)
    assert np.array_equal(pa * 10 + tk, idx) and np.abs(sc - want_sc).max() <= 1e-4
    # all 16 slots: the 14 finite ones first, then -inf candidates in flat-index order
    sc, pa, tk, lp, bad = run_step(logits, scores, 10, 16)
    assert np.isfinite(sc[:, :14]).all() and (sc[:, 14:] == NEG).all()
    assert pa[:, 14:].tolist() == [[0, 0]] * 2 and tk[:, 14:].tolist() == [[1, 4]] * 2


@pytest.mark.parametrize("what", ["nan_logit", "nan_score", "no_finite", "nan_outside"])
def test_a_bad_sequence_is_counted_and_stores_token_zero(what):
    logits = gen.normal(4116, (3, 4, 12), 3.0)
    scores = gen.normal(4117, (3, 4), 1.0)
    want = ref_beam_step(logits, scores, 10, 4)
    if what == "nan_logit":
        logits[1, 2, 9] = np.nan
    elif what == "nan_score":
        scores[1, 3] = np.nan
    elif what == "no_finite":
        logits[1, 0, :10] = NEG
    else:
        logits[1, 2, 10] = np.nan                                   # a column >= n_valid: not a candidate, not read
    sc, pa, tk, lp, bad = run_step(logits, scores, 10, 4)
    good = [0, 1, 2] if what == "nan_outside" else [0, 2]
    assert bad == (0 if what == "nan_outside" else 1)
    if what != "nan_outside":
        assert np.isnan(sc[1]).all() and np.isnan(lp[1]).all() and (tk[1] == 0).all() and pa[1].tolist() == [0, 1, 2, 3]
    assert np.array_equal((pa * 10 + tk)[good], want[1][good]) and np.abs(sc[good] - want[2][good]).max() <= 1e-4
    assert ((tk >= 0) & (tk < 10)).all() and ((pa >= 0) & (pa < 4)).all()


@pytest.mark.parametrize("W_in, W_out, V, n_valid", [(33, 4, 8, 8), (4, 33, 8, 8), (4, 0, 8, 8), (4, 4, 8, 9),
                                                     (4, 4, 8, 0), (32, 4, 514, 513), (17, 4, 1024, 1024)])
def test_each_limit_is_an_argument_error_without_a_launch(W_in, W_out, V, n_valid):
    from arcweld import _native
    from arcweld import kernels as K
    B = 2
    logits = torch.zeros(B * W_in, V, device="cuda")
    outs = [torch.full((B * max(W_out, 1),), -7, dtype=dt, device="cuda")
            for dt in (torch.float32, torch.int32, torch.int64, torch.float32)]
    if W_out == 0:                                                  # the wrapper derives W_out from the outputs' size
        a = _native.BeamArgs()
        a.logits, a.ldl, a.B, a.W_in, a.W_out, a.V, a.n_valid = logits.data_ptr(), V, B, W_in, 0, V, n_valid
        a.scores_in = torch.zeros(B, W_in, device="cuda").data_ptr()
        a.scores_out, a.parent_out, a.token_out, a.logp_out = (t.data_ptr() for t in outs)
        a.bad_count = torch.zeros(1, dtype=torch.int32, device="cuda").data_ptr()
        import ctypes
        with pytest.raises(_native.NativeError, match="W_out"):
            _native.call("aw_beam_step", ctypes.byref(a), _native.stream_ptr())
    else:
        bad = torch.zeros(1, dtype=torch.int32, device="cuda")
        with pytest.raises(_native.NativeError, match="aw_beam_step"):
            K.beam_step(logits, torch.zeros(B, W_in, device="cuda"), *outs, bad, n_valid=n_valid)
    torch.cuda.synchronize()
    assert all((t == -7).all() for t in outs)                       # nothing ran


# ---------------------------------------------------------------------------------------------- aw_beam_gather
SENTINEL = 7.0


def _gather_case(dtype, d, Tmax, n_pos, B, W_in, W_out, parents=None, n_blocks=3):
    from arcweld import kernels as K
    seed = 4200 + d + Tmax + W_in
    src = [torch.tensor(gen.normal(seed + k, (B * W_in, Tmax, 2 * d), 1.0), device="cuda").to(dtype)
           for k in range(n_blocks)]
    dst = [torch.full((B * W_out, Tmax, 2 * d), SENTINEL, device="cuda", dtype=dtype) for _ in range(n_blocks)]
    if parents is None:
        parents = gen.randint(seed + 9, (B, W_out), 0, W_in)
    par = torch.tensor(parents, dtype=torch.int32, device="cuda")
    bad = torch.zeros(1, dtype=torch.int32, device="cuda")
    tab = K.beam_cache_table([src, dst])
    K.beam_gather(tab[0], tab[1], B, W_in, par, Tmax, n_pos, 2 * d, dtype, bad)
    rows = (torch.arange(B, device="cuda")[:, None] * W_in + par.long().clamp(0, W_in - 1)).view(-1)
    return src, dst, rows, int(bad.item())


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("d, Tmax, n_pos, B, W_in, W_out", [
    (64, 33, 20, 3, 4, 4),      # aligned: 16-byte accesses
    (3, 5, 3, 3, 4, 4),         # d 3, Tmax 5: neither the pitch nor the chunk is a multiple of 16 bytes
    (3, 5, 5, 2, 5, 3),         # the whole cache, W_in != W_out
    (64, 33, 9, 3, 1, 4),       # W_in = 1: the prefill cache spread over the beams
    (1024, 6, 5, 2, 2, 3),      # a chunk of several pieces per row (5 * 2048 elements)
])
def test_gather_reorders_every_block_and_leaves_the_tail_alone(dtype, d, Tmax, n_pos, B, W_in, W_out):
    src, dst, rows, bad = _gather_case(dtype, d, Tmax, n_pos, B, W_in, W_out)
    assert bad == 0
    for s, t in zip(src, dst):
        assert torch.equal(t[:, :n_pos], s.index_select(0, rows)[:, :n_pos])
        assert (t[:, n_pos:] == SENTINEL).all()


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("d", [64, 3])
def test_gather_counts_and_zero_fills_an_out_of_range_parent(dtype, d):
    parents = np.array([[0, 3, 4, 1], [2, -1, 0, 3], [1, 1, 2, 0]])          # 4 and -1 lie outside [0, 4)
    src, dst, rows, bad = _gather_case(dtype, d, 5, 3, 3, 4, 4, parents=parents)
    assert bad == 2
    for s, t in zip(src, dst):
        want = s.index_select(0, rows)[:, :3].clone()
        want[2] = 0
        want[5] = 0
        assert torch.equal(t[:, :3], want) and (t[:, 3:] == SENTINEL).all()


def test_gather_of_no_positions_writes_nothing():
    _, dst, _, bad = _gather_case(torch.float32, 3, 5, 0, 2, 2, 2)
    assert bad == 0 and all((t == SENTINEL).all() for t in dst)


# ---------------------------------------------------------------------------------------------- aw_beam_backtrack
@pytest.mark.parametrize("n_new, B, W, R, col0, extra", [(7, 3, 4, 4, 5, 0), (16, 5, 32, 3, 1, 2), (1, 2, 2, 2, 0, 0)])
def test_backtrack_matches_a_python_walk(n_new, B, W, R, col0, extra):
    from arcweld import kernels as K
    parent = gen.randint(4301, (n_new, B, W), 0, W)
    token = gen.randint(4302, (n_new, B, W), 0, 1000)
    logp = gen.normal(4303, (n_new, B, W), 1.0)
    ids = torch.full((B, R, col0 + n_new + extra), -5, dtype=torch.int64, device="cuda")
    lp = torch.empty(B, R, n_new, device="cuda")
    bad = torch.zeros(1, dtype=torch.int32, device="cuda")
    K.beam_backtrack(torch.tensor(parent, dtype=torch.int32, device="cuda"), torch.tensor(token, device="cuda"),
                     torch.tensor(logp, device="cuda"), ids, col0, lp, bad)
    want_ids = np.full((B, R, col0 + n_new + extra), -5, dtype=np.int64)
    want_lp = np.zeros((B, R, n_new), dtype=np.float32)
    for b in range(B):
        for j in range(R):
            cur = j
            for i in range(n_new - 1, -1, -1):
                want_ids[b, j, col0 + i] = token[i, b, cur]
                want_lp[b, j, i] = logp[i, b, cur]
                cur = parent[i, b, cur]
    assert int(bad.item()) == 0
    assert np.array_equal(ids.cpu().numpy(), want_ids) and np.array_equal(lp.cpu().numpy(), want_lp)


def test_backtrack_counts_a_parent_outside_the_beams():
    from arcweld import kernels as K
    n_new, B, W = 4, 2, 3
    parent = np.zeros((n_new, B, W), dtype=np.int32)
    parent[2, 1, 0] = 3                                             # met by every hypothesis of sequence 1 at step 2
    token = gen.randint(4304, (n_new, B, W), 1, 50)
    ids = torch.full((B, W, n_new), -5, dtype=torch.int64, device="cuda")
    lp = torch.empty(B, W, n_new, device="cuda")
    bad = torch.zeros(1, dtype=torch.int32, device="cuda")
    K.beam_backtrack(torch.tensor(parent, device="cuda"), torch.tensor(token, device="cuda"),
                     torch.zeros(n_new, B, W, device="cuda"), ids, 0, lp, bad)
    assert int(bad.item()) == W
    ids = ids.cpu().numpy()
    assert (ids[1, :, :2] == 0).all() and (ids[1, :, 2] == token[2, 1, 0]).all() and (ids[0] > 0).all()
    assert torch.isnan(lp[1, :, :2]).all() and (lp[0] == 0).all()
