"""CPU checks of tests/optim_refs.py, the instrument of tests/test_optim_kernels_gpu.py: the fp64 RAdam / clip
restatement against torch.optim.RAdam and clip_grad_norm_ in float64 and against the committed golden trajectory, an
honest f32 restatement of radam_one (both contractions) under the derived allowance, the permute-built index maps
against the formulas written in include/arcweld_amd.h, and the kernels' element selection emulated on the layouts the
GPU tests use and on the layouts arcweld.optim plans for centre-tap parameters."""
import itertools

import numpy as np
import pytest
import torch

import optim_refs as R
from conftest import golden
from oracle import gen

SHAPES = [(33, 7), (7,), (5, 3, 2)]
STEPS_32 = (1, 5, 6, 7, R.BIG_STEP)


def _flat_layout(shapes, wd_of):
    L = R.make_layout([int(np.prod(s)) for s in shapes], align=64)
    L.wd = np.asarray(wd_of, np.float32)
    return L


def _scatter(L, arrays, dtype=np.float64):
    flat = np.zeros(L.total, dtype)
    for o, a in zip(L.off, arrays):
        flat[o:o + a.size] = np.asarray(a, dtype).reshape(-1)
    return flat


# ------------------------------------------------------------------------------------------ reference vs torch
@pytest.mark.parametrize("tag", sorted(R.BETAS))
def test_reference_matches_torch_in_float64(tag):
    betas, lr, eps, max_norm, nsteps = R.BETAS[tag], 1e-3, 1e-8, 0.7, 14
    wd_of = [0.1, 0.37, 0.1]
    params = [torch.nn.Parameter(torch.tensor(gen.normal(500 + i, s, 0.3), dtype=torch.float64))
              for i, s in enumerate(SHAPES)]
    opt = torch.optim.RAdam([{"params": [params[0], params[2]], "weight_decay": 0.1},
                             {"params": [params[1]], "weight_decay": 0.37}], lr=lr, betas=betas, eps=eps, foreach=False)
    L = _flat_layout(SHAPES, wd_of)
    L.wd = np.asarray(wd_of, np.float64)            # torch takes the python floats: no f32 rounding on this side
    sg = [(int(o), int(n), w, 1) for o, n, w in zip(L.off, L.len, wd_of)]
    p = _scatter(L, [q.detach().numpy() for q in params])
    m, v = np.zeros(L.total), np.zeros(L.total)
    torch_rectified = []
    for step in range(1, nsteps + 1):
        grads = [gen.normal(600 + 17 * step + i, s, 1.0).astype(np.float64) for i, s in enumerate(SHAPES)]
        for q, gr in zip(params, grads):
            q.grad = torch.tensor(gr)
        g = _scatter(L, grads)
        want_norm = float(torch.nn.utils.clip_grad_norm_(params, max_norm))
        norm, coef = R.clip64(g, sg, max_norm)
        assert abs(norm - want_norm) <= 1e-12 * want_norm
        before = [q.detach().clone() for q in params]
        opt.step()
        p, m, v = R.radam_step64(p, g, m, v, sg, step, lr, *betas, eps, gscale=coef, abi32=False)
        S = R.radam_scalars(step, *betas)
        unrect = []
        for i, q in enumerate(params):
            st = opt.state[q]
            o, n = int(L.off[i]), int(L.len[i])
            for got, want in ((p, q.detach()), (m, st["exp_avg"]), (v, st["exp_avg_sq"])):
                np.testing.assert_allclose(got[o:o + n], want.numpy().reshape(-1), rtol=1e-12, atol=0,
                                           err_msg=f"{tag} step {step} param {i}")
            # torch's own behaviour: below the threshold its update is lr * exp_avg / bias_correction1 and nothing else
            unrect.append(torch.allclose(before[i] - q.detach(), lr * st["exp_avg"] / S.bc1, rtol=1e-9, atol=0))
        assert all(unrect) or not any(unrect)
        torch_rectified.append(not unrect[0])
    first = 1 + torch_rectified.index(True)
    assert torch_rectified == [t >= first for t in range(1, nsteps + 1)]
    assert first == R.first_rectified(*betas) == 6 and 1 < first < nsteps          # the run crosses the threshold
    assert [R.radam_scalars(t, *betas).rectified for t in range(1, nsteps + 1)] == torch_rectified


@pytest.mark.parametrize("tag,betas,groups", [
    ("vqvae", (0.9, 0.999), [(0.0, [0, 1, 2])]),
    ("decoder", (0.9, 0.95), [(0.1, [0, 2]), (0.0, [1])]),
])
def test_reference_follows_the_golden_trajectory(tag, betas, groups):
    """tests/golden/radam.npz (f32 torch.optim.RAdam of the reference project) at test_gpu_optim.py's tolerances."""
    gold = golden("radam.npz")
    wd_of = [0.0] * len(SHAPES)
    for wd, idx in groups:
        for i in idx:
            wd_of[i] = wd
    L = _flat_layout(SHAPES, wd_of)
    sg = R.segs(L)
    p = _scatter(L, [gen.normal(500 + i, s, 0.3) for i, s in enumerate(SHAPES)])
    m, v = np.zeros(L.total), np.zeros(L.total)
    for step in range(8):
        g = _scatter(L, [gen.normal(600 + 17 * step + i, s, 1.0) for i, s in enumerate(SHAPES)])
        norm, coef = R.clip64(g, sg, 0.7)
        np.testing.assert_allclose(norm, gold[f"{tag}/prenorm_{step}"], rtol=2e-6)
        p, m, v = R.radam_step64(p, g, m, v, sg, step + 1, 1e-3, *betas, 1e-8, gscale=coef)
        for i, s in enumerate(SHAPES):
            o, n = int(L.off[i]), int(L.len[i])
            np.testing.assert_allclose(p[o:o + n].reshape(s), gold[f"{tag}/p{i}_step{step}"], rtol=2e-6, atol=2e-7,
                                       err_msg=f"step {step} param {i}")


def test_scalars_at_a_step_where_beta2_pow_t_underflows():
    for betas in R.BETAS.values():
        S = R.radam_scalars(R.BIG_STEP, R.r32(betas[0]), R.r32(betas[1]))
        assert R.r32(betas[1]) ** float(R.BIG_STEP) == 0.0
        assert S.rectified and S.rect == 1.0 and S.bc1 == 1.0 and S.bc2 == 1.0 and S.rho_t == S.rho_inf


def test_untouched_outside_live_elements():
    L = R.with_active(R.lead_layout(4), R.active_patterns(12)["two-off"])
    st = R.fill(L, 11, "normal", sentinel=R.SENTINEL)
    live, cover, pad = R.masks(L)
    out = R.radam_step64(st.p, st.g, st.m, st.v, R.segs(L), 6, R.LR, 0.9, 0.999, R.EPS, 0.37)
    for new, old in zip(out, (st.p, st.m, st.v)):
        assert np.array_equal(R.bits(new[~live]), R.bits(old[~live].astype(np.float64)))
        assert not np.array_equal(new[live], old[live].astype(np.float64))
    assert np.isnan(st.p[~cover]).any() and (st.p[~cover] == R.SENTINEL).any() and (st.p[pad] == 0).all()


# ------------------------------------------------------------------------------------------ honest f32 vs allowance
def _worst_ratio(L, kind, step, betas, gs, fused):
    st = R.fill(L, 40, kind)
    sg = R.segs(L)
    args = (sg, step, R.LR, *betas, R.EPS, gs)
    ref = R.radam_step64(st.p, st.g, st.m, st.v, *args)
    tol = R.allowance(st.p, st.g, st.m, st.v, *args)
    got = R.radam_step32(st.p, st.g, st.m, st.v, *args, fused=fused)
    live = R.masks(L)[0]
    worst = 0.0
    for x, r, a, old in zip(got, ref, tol, (st.p, st.m, st.v)):
        assert np.array_equal(R.bits(x[~live]), R.bits(old[~live]))
        err = np.abs(x[live].astype(np.float64) - r[live])
        assert np.isfinite(r[live]).all() and (err[a[live] == 0] == 0).all()
        pos = a[live] > 0
        if pos.any():
            worst = max(worst, float((err[pos] / a[live][pos]).max()))
    return worst


@pytest.mark.parametrize("kind", ["normal", "small", "zero"])
def test_honest_f32_stays_under_the_allowance(kind):
    L = R.make_layout(R.RAGGED, align=4)
    worst = 0.0
    for step, betas, gs, fused in itertools.product(STEPS_32, R.BETAS.values(), (1.0, 0.37), (False, True)):
        ratio = _worst_ratio(L, kind, step, betas, gs, fused)
        assert ratio < 1.0, (kind, step, betas, gs, fused, ratio)
        worst = max(worst, ratio)
    print(f"{kind}: worst |f32 - f64| / allowance = {worst:.3f}")


def test_zero_state_without_decay_leaves_p_bit_unchanged():
    L = R.make_layout(R.RAGGED, align=4, wds=(0.0,))
    st = R.fill(L, 41, "zero")
    for step in (5, 6):
        p, m, v = R.radam_step64(st.p, st.g, st.m, st.v, R.segs(L), step, R.LR, 0.9, 0.999, R.EPS)
        assert np.array_equal(p, st.p.astype(np.float64)) and not m.any() and not v.any()
        ap, am, av = R.allowance(st.p, st.g, st.m, st.v, R.segs(L), step, R.LR, 0.9, 0.999, R.EPS)
        assert not am.any() and not av.any()            # m and v must be exact; p may round its own subtraction only
        assert (ap <= R.U * np.abs(st.p)).all()


def test_allowance_separates_the_wrong_formulas():
    """The mutants the GPU test must catch sit far outside the allowance: eps inside the root (small gradients), the
    first segment's weight decay for all, the step of the wrong phase."""
    L = R.make_layout(R.RAGGED, align=4)
    sg = R.segs(L)
    live = R.masks(L)[0]
    st = R.fill(L, 40, "small")
    args = (sg, 6, R.LR, 0.9, 0.999, R.EPS)
    ref = R.radam_step64(st.p, st.g, st.m, st.v, *args)[0]
    ap = R.allowance(st.p, st.g, st.m, st.v, *args)[0]
    p, g, m, v = (x.astype(np.float64) for x in (st.p, st.g, st.m, st.v))
    S = R.radam_scalars(6, R.r32(0.9), R.r32(0.999))
    wd = R._per_element(L.total, sg)[1]
    t = R._trace64(p, g, m, v, wd, S, R.r32(R.LR), R.r32(0.9), R.r32(0.999), R.r32(R.EPS), 1.0)
    inside = p - t.x1 * (np.sqrt(S.bc2) / np.sqrt(t.v2 + R.r32(R.EPS))) * S.rect
    assert (np.abs(inside - ref)[live] > ap[live]).mean() > 0.5           # every element must pass on the GPU
    st = R.fill(L, 40, "normal")
    ref, ref_m, _ = R.radam_step64(st.p, st.g, st.m, st.v, *args)
    ap, am, _ = R.allowance(st.p, st.g, st.m, st.v, *args)
    wd0_m = R.radam_step64(st.p, st.g, st.m, st.v, [(o, n, sg[0][2], a) for o, n, _, a in sg], *args[1:])[1]
    decayed = live & (wd != 0)
    assert (np.abs(wd0_m - ref_m)[decayed] > 100 * am[decayed]).mean() > 0.9     # the first moment shows it
    other = R.radam_step64(st.p, st.g, st.m, st.v, sg, 1, *args[2:])[0]
    assert (np.abs(other - ref)[live] > 100 * ap[live]).mean() > 0.9


def test_norm_constants():
    assert R.norm_k(268) == 1 and R.norm_k(4 * 512 * 1024) == 1 and R.norm_k(4 * 512 * 1024 + 4) == 2
    assert R.norm_k(4 * 256 * 1024 + 4, nt=256) == 2
    T = R.strided_total()
    assert T % 4 == 0 and T // 4 > R.RADAM_GRID_CAP * R.RADAM_THREADS and T // 4 > 4 * R.NORM_WS * 512
    assert R.norm_k(T) == 5                                      # one full unrolled trip and the start of a second
    L = R.strided_layout()
    assert L.nseg == 300 and L.total == T and (L.off % 4 == 0).all() and L.off[-1] + L.len[-1] <= T
    assert (np.diff(L.off) >= L.len[:-1]).all() and 0 < (L.active == 0).sum() < 300
    M = R.many_layout()
    assert M.nseg == 1024 and (M.off % 4 == 0).all() and set(M.len.tolist()) == set(range(1, 8))


# ------------------------------------------------------------------------------------------ index maps
MAPS = [(0, 5, 7, 3, 0, 0), (0, 5, 7, 3, 1, 0), (0, 5, 7, 3, 2, 0), (0, 4, 8, 1, 0, 0), (0, 5, 7, 1, 0, 0),
        (1, 5, 7, 3, 0, 0), (1, 4, 8, 3, 0, 0), (2, 5, 7, 3, 0, 0), (2, 4, 8, 3, 0, 0), (3, 5, 6, 5, 0, 0),
        (4, 7, 1, 25, 0, 32), (4, 3, 1, 25, 0, 25), (5, 7, 9, 1, 0, 0), (5, 8, 8, 1, 0, 0),
        (7, 5, 8, 3, 0, 0), (7, 5, 4, 3, 0, 0), (7, 5, 6, 3, 0, 0)]


@pytest.mark.parametrize("mode,O,I,k,tap,ldo", MAPS)
def test_operand_dst_is_injective_with_the_stated_image(mode, O, I, k, tap, ldo):
    dst = R.operand_dst(mode, O, I, k, tap, ldo)
    assert len(dst) == int(np.prod(R.storage_shape(mode, O, I, k)))
    hit = dst[dst >= 0]
    assert len(hit) == R.image_size(mode, O, I, k) and len(np.unique(hit)) == len(hit)
    out_n = R.relayout_ref(np.zeros(len(dst)), mode, O, I, k, tap, ldo).size
    assert hit.min() == 0 and hit.max() < out_n
    if mode != 4:
        assert len(hit) == out_n                       # every operand element is written; mode 4 leaves its padding
    W = gen.normal(3, (len(dst),), 1.0)
    out = R.relayout_ref(W, mode, O, I, k, tap, ldo, pad=-5.0).reshape(-1)
    assert np.array_equal(out[hit], W[dst >= 0]) and (np.delete(out, hit) == -5.0).all()


def _header_formula(mode, O, I, k, tap, ldo):
    """dst by the sentences of include/arcweld_amd.h, as loops over the named indices."""
    dst = {}
    if mode in (0, 1, 2, 4):                     # conv (O, I, k)
        for o, i, j in itertools.product(range(O), range(I), range(k)):
            l = (o * I + i) * k + j
            if mode == 0 and j == tap:
                dst[l] = o * I + i                                # tap t -> [O][I]
            if mode == 1:
                dst[l] = o * (3 * I) + (j * I + i)                # [O][3 I], col j I + i
            if mode == 2:
                dst[l] = (j * O + o) * I + i                      # [3 O][I], row j O + o = W[o][:, j]
            if mode == 4:
                dst[l] = o * ldo + (i * k + j)                    # [O][ldo], col i k + j
    elif mode == 3:                              # convT (I, O, k) -> [k O][I], row j O + o
        for i, o, j in itertools.product(range(I), range(O), range(k)):
            dst[(i * O + o) * k + j] = (j * O + o) * I + i
    elif mode == 5:
        dst = {l: l for l in range(O * I)}
    elif mode == 7:                              # stored (O, 3, I) -> [3 O][I], row j O + o
        for o, j, i in itertools.product(range(O), range(3), range(I)):
            dst[(o * 3 + j) * I + i] = (j * O + o) * I + i
    return dst


@pytest.mark.parametrize("mode,O,I,k,tap,ldo", [(0, 2, 3, 3, 1, 0), (1, 2, 3, 3, 0, 0), (2, 2, 3, 3, 0, 0),
                                                (3, 2, 3, 4, 0, 0), (4, 3, 1, 5, 0, 7), (5, 2, 3, 1, 0, 0),
                                                (7, 2, 3, 3, 0, 0)])
def test_operand_dst_against_the_header_formula(mode, O, I, k, tap, ldo):
    want = _header_formula(mode, O, I, k, tap, ldo)
    dst = R.operand_dst(mode, O, I, k, tap, ldo)
    assert {l: int(d) for l, d in enumerate(dst) if d >= 0} == want


@pytest.mark.parametrize("mode,O,I,k,tap,rows,row", [(0, 2, 3, 3, 1, 2, 3), (1, 2, 3, 3, 0, 2, 9), (3, 2, 3, 4, 0, 8, 3),
                                                     (4, 3, 1, 5, 0, 3, 5)])
def test_scatter_ref_inverts_the_relayout(mode, O, I, k, tap, rows, row):
    n = int(np.prod(R.storage_shape(mode, O, I, k)))
    W = np.arange(1, n + 1, dtype=np.float64)
    op = R.relayout_ref(W, mode, O, I, k, tap, ldo=row)
    g = np.full((rows, row + 3), np.nan)
    g[:, :row] = op.reshape(rows, row)
    S = R.scatter_ref(g, mode, O, I, k, tap)
    assert S.shape == R.storage_shape(mode, O, I, k)
    mapped = R.operand_dst(mode, O, I, k, tap, ldo=row) >= 0
    assert np.array_equal(S.reshape(-1)[mapped], W[mapped]) and not S.reshape(-1)[~mapped].any()


# ------------------------------------------------------------------------------------------ element selection
@pytest.mark.parametrize("align", [4, 64])
def test_selection_on_contract_layouts_is_the_cover_of_the_active_segments(align):
    base = R.make_layout(R.RAGGED, align=align)
    for name, act in R.active_patterns(base.nseg).items():
        L = R.with_active(base, act)
        live, cover, _ = R.masks(L)
        for threads in (1, 8, 257):                       # 257: one stride skips several short segments at once
            for lb in (False, True):
                taken, seg = R.emulate_selection(L, threads, lower_bound=lb)
                assert np.array_equal(taken, cover), (name, threads, lb)
                for s, (o, n, _, a) in enumerate(R.segs(L)):
                    assert not a or (seg[o:o + n] == s).all()


def test_selection_before_the_first_segment_needs_the_lower_bound():
    """Finding 2: without a lower bound the elements before off[0] are taken as segment 0 -- even when segment 0 is
    inactive, for the kernels whose table folds the flag into the end -- and with it exactly the cover is taken."""
    L = R.lead_layout(4)
    _, cover, _ = R.masks(L)
    taken, seg = R.emulate_selection(L, 8, lower_bound=False)
    assert taken[:64].all() and (seg[:64] == 0).all() and np.array_equal(taken[64:], cover[64:])
    taken, _ = R.emulate_selection(L, 8, lower_bound=True)
    assert np.array_equal(taken, cover)
    M = R.many_layout()
    assert np.array_equal(R.emulate_selection(M, 300)[0], R.masks(M)[1])


CENTRE_ORDERS = [([(6, 5, 3), (6,), (6, 5, 3), (4, 7), (6, 5, 3)], [0, 2, 4]),
                 ([(6,), (6, 5, 3), (6, 5, 3), (4, 7), (6, 5, 3)], [1, 2, 4]),
                 ([(6,), (6, 6, 3), (6, 6, 3), (4, 7), (6, 6, 3)], [1, 2, 4])]


def _planned(shapes, centre):
    from arcweld.optim import RAdam
    params = [torch.nn.Parameter(torch.zeros(s)) for s in shapes]
    opt = RAdam(params, lr=1e-2)
    opt.declare_centre_tap([params[i] for i in centre])
    _, kept, _, _, sg, _, total, blk, slot = opt._plan()
    return params, kept, sg, total, blk, slot


@pytest.mark.parametrize("shapes,centre", CENTRE_ORDERS)
def test_planned_centre_tap_layouts_start_every_segment_on_a_float4(shapes, centre):
    params, kept, sg, total, blk, slot = _planned(shapes, centre)
    assert len(kept) == 3 and slot % 4 == 0 and slot >= shapes[centre[0]][0] * shapes[centre[0]][1]
    offs, lens = [s[1] for s in sg], [s[2] for s in sg]
    assert all(o % 4 == 0 for o in offs) and offs == sorted(offs) and total % 64 == 0
    assert all(a + n <= b for a, n, b in zip(offs, lens, offs[1:] + [total]))
    L = R.plan_layout(offs, lens, total)
    live, cover, _ = R.masks(L)
    taken, seg = R.emulate_selection(L, 8, lower_bound=True)
    assert np.array_equal(taken, cover)
    for s, (o, n) in enumerate(zip(offs, lens)):
        assert (seg[o:o + n] == s).all()
    # the dead side-tap slots (taps 0 and 2 of the block) are outside every segment
    assert not cover[blk:blk + 3 * slot].any() and not cover[blk + 6 * slot:blk + 9 * slot].any()
    assert live.sum() == sum(lens)


def test_unpadded_centre_block_drops_elements():
    """Finding 1, on the layout the packing produced before its slots were padded: [(6,), 3 x (6, 5, 3), (4, 7)] with
    the centre block after the (6,) vector puts the first centre segment at 154; the float4 at 152 resolves to the
    segment before it and is skipped as past its end, so elements 0 and 1 of that segment are never taken."""
    offs, lens = [0, 64 + 90, 64 + 120, 64 + 150, 384], [6, 30, 30, 30, 28]
    L = R.plan_layout(offs, lens, 448)
    for lb in (False, True):
        taken, _ = R.emulate_selection(L, 8, lower_bound=lb)
        assert not taken[154:156].any() and taken[156:184].all()
    # with the block first, only the missing lower bound kept every element (the float4 at 88 ran as segment 0)
    offs, lens = [90, 120, 150, 320, 384], [30, 30, 30, 6, 28]
    L = R.plan_layout(offs, lens, 448)
    assert R.emulate_selection(L, 8, lower_bound=False)[0][90:180].all()
    assert not R.emulate_selection(L, 8, lower_bound=True)[0][90:92].any()
