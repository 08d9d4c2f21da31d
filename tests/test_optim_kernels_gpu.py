"""csrc/optim.hip (aw_radam_step with and without ops, aw_grad_norm_clip, aw_scale) and the weight-relayout family of
csrc/vqvae.hip (aw_weight_relayout, aw_weight_relayout_batch, aw_weight_grad_scatter, aw_cast) against the fp64
restatements and the permute-built index maps of tests/optim_refs.py.  The kernels are called directly through
arcweld.kernels.  Every buffer a kernel may write sits between canary margins that are checked after every launch; the
weights of the relayout family sit inside NaN-filled margins; inactive segments hold NaN and 1e30 and the regions no
segment owns hold a sentinel, so a read from them shows in a result and a write to them shows bit for bit.

The bounds are derived in optim_refs.py (allowance, norm_rtol) and measured against an honest f32 restatement on the
CPU in tests/test_optim_refs_cpu.py; no number here was taken from the kernels.

Which layout reaches which path:
  ragged-a64 / ragged-a4   one workgroup per 256 float4s, several workgroups; segments shorter than a float4, tails of
                           1..3 elements, back-to-back segments (a4); every active pattern
  lead-a64 / lead-a4       off[0] = 64: the region before the first segment and interior gaps hold a sentinel
  many                     1024 segments of 1..7 elements: both LDS table loaders loop (4 x 256, 2 x 512 threads) and one
                           stride of next_seg skips whole runs of segments
  strided                  total just above one trip of radam's capped grid (4096 x 256 float4s) and of sumsq's 4x
                           unrolled loop (1024 x 512 x 4 float4s): grid cap, grid-stride loops, the q < n4 guard partly
                           false in the last trip, k = 5 float4s per thread in the norm
  operand copies           op_store4's vector path (mode 5, mode 0 with k = 1, mode 7 with I % 4 == 0), its element
                           path (every other mode, mode 7 with I = 6, an `out` that is not 16-B aligned) and the segment
                           tail path (segment lengths that are no multiple of 4)"""
import ctypes
import functools
import itertools
import os
import subprocess
import sys
import types

import numpy as np
import pytest
import torch

import optim_refs as R
from oracle import gen

pytestmark = pytest.mark.gpu

PAD = 64
CANARY = -1024.0
SENT = -3.0                 # prefill of the operand copies: exact in bf16, never a weight
FIRST = {tag: R.first_rectified(*b) for tag, b in R.BETAS.items()}


class _Buf:
    """A device tensor holding `a` (or `fill`) between two PAD-long canary margins; .t is 16-byte aligned."""

    def __init__(self, a=None, shape=None, dtype=torch.float32, fill=None, canary=CANARY):
        if a is not None:
            a = np.ascontiguousarray(a)
            shape, dtype = a.shape, torch.from_numpy(a[:0].copy()).dtype
        self.n, self.canary = int(np.prod(shape)), canary
        self.buf = torch.full((self.n + 2 * PAD,), canary, dtype=dtype, device="cuda")
        self.t = self.buf[PAD:PAD + self.n].view(shape)
        if a is not None:
            if self.n:
                self.t.copy_(torch.from_numpy(a))
        elif fill is not None:
            self.t.fill_(fill)
        self.fill = fill
        assert self.t.data_ptr() % 16 == 0

    def check(self):
        lo, hi = self.buf[:PAD], self.buf[PAD + self.n:]
        if self.canary != self.canary:
            ok = torch.isnan(lo).all() and torch.isnan(hi).all()
        else:
            ok = (lo == self.canary).all() and (hi == self.canary).all()
        assert bool(ok), "a margin next to a buffer was written"

    def np(self):
        self.check()
        return (self.t.float() if self.t.dtype == torch.bfloat16 else self.t).cpu().numpy()

    def tbits(self):
        self.check()
        t = self.t.contiguous().cpu()
        return t.view(torch.int16 if t.dtype == torch.bfloat16 else torch.int32).numpy()


def _place(a):
    """f32 on the device inside a NaN-filled allocation (an input the kernel must not read outside of)."""
    return _Buf(np.asarray(a, np.float32), canary=float("nan"))


class _Table:
    """The segment table on the device: offsets and lengths between -77 margins, weight decay between NaN ones."""

    def __init__(self, L):
        self.off, self.len = _Buf(L.off, canary=-77), _Buf(L.len, canary=-77)
        self.act, self.wd = _Buf(L.active, canary=-77), _Buf(L.wd, canary=float("nan"))

    def check(self, L):
        for b, a in ((self.off, L.off), (self.len, L.len), (self.act, L.active), (self.wd, L.wd)):
            assert np.array_equal(b.np(), a)


@functools.lru_cache(maxsize=None)
def _layout(name):
    if name.startswith("ragged"):
        _, al, pat = name.split("/")
        base = R.make_layout(R.RAGGED, align=int(al[1:]))
        return R.with_active(base, R.active_patterns(base.nseg)[pat])
    if name.startswith("lead"):
        return R.lead_layout(int(name.split("/")[1][1:]))
    return {"many": R.many_layout, "strided": R.strided_layout}[name]()


@functools.lru_cache(maxsize=8)
def _state(name, kind):
    L = _layout(name)
    return R.fill(L, 4000 + len(name), kind, sentinel=R.SENTINEL if name.startswith("lead") else None)


def _launch(L, st, step, betas, src, gs, zero_grad=False, ops=None, host_step=None, T=None):
    """One aw_radam_step launch (with ops when given) from the state `st`; the four buffers afterwards (numpy)."""
    from arcweld import kernels as K
    T = T or _Table(L)
    b = types.SimpleNamespace(p=_Buf(st.p), g=_Buf(st.g), m=_Buf(st.m), v=_Buf(st.v))
    gsd = None if gs is None else _place([gs])
    sp = torch.tensor([step], dtype=torch.int64, device="cuda") if src == "ptr" else None
    host = (step if host_step is None else host_step) if src == "ptr" else step
    K.radam_step(b.p.t, b.g.t, b.m.t, b.v.t, T.off.t, T.len.t, T.wd.t, T.act.t, L.nseg, L.total, host, R.LR, *betas, R.EPS,
                 gscale=None if gsd is None else gsd.t, step_ptr=sp, ops=ops, zero_grad=zero_grad)
    torch.cuda.synchronize()
    T.check(L)
    return types.SimpleNamespace(p=b.p.np(), g=b.g.np(), m=b.m.np(), v=b.v.np())


@functools.lru_cache(maxsize=64)
def _ref(name, kind, step, tag, gs):
    L, st = _layout(name), _state(name, kind)
    args = (R.segs(L), step, R.LR, *R.BETAS[tag], R.EPS, 1.0 if gs is None else R.r32(gs))
    return R.radam_step64(st.p, st.g, st.m, st.v, *args), R.allowance(st.p, st.g, st.m, st.v, *args)


def _check_step(name, kind, got, step, tag, gs, zero_grad, label):
    L, st = _layout(name), _state(name, kind)
    ref, tol = (_ref.__wrapped__ if name == "strided" else _ref)(name, kind, step, tag, gs)   # too large to keep
    live, cover, pad = R.masks(L)
    worst = 0.0
    for nm, x, r, a, old in zip("pmv", (got.p, got.m, got.v), ref, tol, (st.p, st.m, st.v)):
        assert np.array_equal(R.bits(x[~cover]), R.bits(old[~cover])), f"{label}: {nm} written outside the segments"
        assert not x[pad].any(), f"{label}: {nm} padding is no longer zero"
        err = np.abs(x[live].astype(np.float64) - r[live])
        assert np.isfinite(x[live]).all(), f"{label}: {nm} not finite"
        bad = np.flatnonzero(err > a[live])
        if a[live].any():
            worst = max(worst, float((err[a[live] > 0] / a[live][a[live] > 0]).max()))
        assert bad.size == 0, (f"{label}: {nm} outside the allowance at {bad.size} elements, first live index {bad[0]}: "
                               f"err {err[bad[0]]:.3g} allowance {a[live][bad[0]]:.3g}")
    if zero_grad:
        assert not got.g[cover].any(), f"{label}: g not zeroed on the updated float4s"
    else:
        assert np.array_equal(R.bits(got.g[cover]), R.bits(st.g[cover])), f"{label}: g changed"
    assert np.array_equal(R.bits(got.g[~cover]), R.bits(st.g[~cover])), f"{label}: g written outside the segments"
    return worst


def _one_ops_table(L, seg=0, dtype=torch.float32):
    """An operand table as RAdam.attach_operands builds it with one plain-cast copy (mode 5) of segment `seg`."""
    from arcweld import _native as nat
    from arcweld import kernels as K
    out = _Buf(shape=(int(L.len[seg]),), dtype=dtype, fill=SENT)
    table = (nat.OperandDesc * (nat.OPS_PER_SEG * L.nseg))()
    for d in table:
        d.mode = -1
    d = table[nat.OPS_PER_SEG * seg]
    d.out, d.O, d.I, d.k, d.tap, d.mode, d.ldo = out.t.data_ptr(), 1, int(L.len[seg]), 1, 0, 5, 0
    d.dtype = K.dtype_code(dtype)
    return torch.frombuffer(bytearray(bytes(table)), dtype=torch.uint8).to("cuda"), out


def _combos(tag_steps, srcs=("host", "ptr"), scales=(None, 1.0, 0.37)):
    return list(itertools.product(tag_steps, srcs, scales))


def _tag_steps():
    out = []
    for tag in sorted(R.BETAS):
        out += [(tag, FIRST[tag] - 1), (tag, FIRST[tag]), (tag, FIRST[tag] + 1)]
    return out + [("vqvae", R.BIG_STEP), ("decoder", R.BIG_STEP)]


SMALL_LAYOUTS = [f"ragged/a{a}/{p}" for a in (64, 4) for p in ("all", "first-off", "last-off", "two-off", "none")] + \
    ["lead/a64", "lead/a4", "many"]


# ------------------------------------------------------------------------------------------------ RAdam
@pytest.mark.parametrize("kind", ["normal", "small", "zero"])
@pytest.mark.parametrize("name", SMALL_LAYOUTS)
def test_radam_step_within_the_allowance(name, kind):
    """Every (betas, step) x step source x gradient scale on one layout and input kind; the operand-writing kernel
    on the same inputs must store the same bits and copy segment 0 (and nothing from before it)."""
    L, st = _layout(name), _state(name, kind)
    T = _Table(L)
    ops, out = _one_ops_table(L)
    worst = 0.0
    for i, ((tag, step), src, gs) in enumerate(_combos(_tag_steps())):
        zg = bool(i % 2)
        label = f"{name} {kind} {tag} step {step} {src} gscale {gs} zero_grad {zg}"
        got = _launch(L, st, step, R.BETAS[tag], src, gs, zero_grad=zg, T=T)
        worst = max(worst, _check_step(name, kind, got, step, tag, gs, zg, label))
        if step == R.BIG_STEP:
            S = R.radam_scalars(step, *map(R.r32, R.BETAS[tag]))
            assert S.rectified and S.rect == 1.0
        out.t.fill_(SENT)
        got2 = _launch(L, st, step, R.BETAS[tag], src, gs, zero_grad=zg, ops=ops, T=T)
        for nm in "pgmv":
            assert np.array_equal(R.bits(getattr(got2, nm)), R.bits(getattr(got, nm))), f"{label}: ops kernel {nm}"
        o, n = int(L.off[0]), int(L.len[0])
        want = got.p[o:o + n] if L.active[0] else np.full(n, SENT, np.float32)
        assert np.array_equal(R.bits(out.np()), R.bits(want)), f"{label}: operand copy of segment 0"
    print(f"{name} {kind}: worst |kernel - fp64| / allowance = {worst:.3f}")
    if kind == "zero":
        live = R.masks(L)[0]
        wd0 = np.zeros(L.total, bool)
        for o, n, w, a in R.segs(L):
            wd0[o:o + n] = a and w == 0
        for tag in R.BETAS:
            for step in (FIRST[tag] - 1, FIRST[tag]):
                got = _launch(L, st, step, R.BETAS[tag], "host", None, T=T)
                assert np.array_equal(R.bits(got.p[wd0]), R.bits(st.p[wd0])), "zero state, no decay: p moved"
                assert (got.p[live & ~wd0] != st.p[live & ~wd0]).any() or not (live & ~wd0).any()


@pytest.mark.parametrize("tag,step,src,gs", [("vqvae", 5, "host", None), ("decoder", 6, "ptr", 0.37)])
def test_radam_step_strided(tag, step, src, gs):
    name = "strided"
    L, st = _layout(name), _state(name, "normal")
    assert L.total // 4 > R.RADAM_GRID_CAP * R.RADAM_THREADS
    got = _launch(L, st, step, R.BETAS[tag], src, gs, zero_grad=True)
    worst = _check_step(name, "normal", got, step, tag, gs, True, f"strided {tag} step {step}")
    print(f"strided {tag} step {step}: worst |kernel - fp64| / allowance = {worst:.3f}")
    ops, out = _one_ops_table(L, seg=L.nseg - 1, dtype=torch.bfloat16)
    got2 = _launch(L, st, step, R.BETAS[tag], src, gs, zero_grad=True, ops=ops)
    for nm in "pgmv":
        assert np.array_equal(R.bits(getattr(got2, nm)), R.bits(getattr(got, nm))), f"ops kernel {nm}"
    o, n = int(L.off[-1]), int(L.len[-1])
    assert torch.equal(out.t.cpu(), torch.from_numpy(got.p[o:o + n]).to(torch.bfloat16))
    out.check()


def test_step_ptr_overrides_a_contradicting_host_step():
    name, tag = "ragged/a4/all", "vqvae"
    L, st = _layout(name), _state(name, "normal")
    got = _launch(L, st, FIRST[tag], R.BETAS[tag], "ptr", 0.37, host_step=1)
    _check_step(name, "normal", got, FIRST[tag], tag, 0.37, False, "device step 6, host step 1")
    ref1 = _ref(name, "normal", 1, tag, 0.37)[0][0]
    live = R.masks(L)[0]
    assert (np.abs(got.p[live] - ref1[live]) > 1e-5).mean() > 0.5            # and not the host's step


def test_trajectory_on_its_own_state():
    """12 steps with a clip every step, one segment inactive: the kernels on their own f32 state against the fp64
    reference on its own state, at test_gpu_optim.py's trajectory tolerances."""
    from arcweld import kernels as K
    L = _layout("ragged/a4/two-off")
    L = R.with_active(L, [0 if i == 5 else 1 for i in range(L.nseg)])
    st = R.fill(L, 77, "normal")
    sg, T = R.segs(L), _Table(L)
    live = R.masks(L)[0]
    b = types.SimpleNamespace(p=_Buf(st.p), g=_Buf(st.g), m=_Buf(np.zeros_like(st.m)), v=_Buf(np.zeros_like(st.v)))
    ws = _Buf(shape=(K.NORM_WS,), dtype=torch.float64, fill=0.0)
    norm, coef = _Buf(shape=(1,), fill=0.0), _Buf(shape=(1,), fill=0.0)
    p, m, v = st.p.astype(np.float64), np.zeros(L.total), np.zeros(L.total)
    stepd = torch.zeros(1, dtype=torch.int64, device="cuda")
    for step in range(1, 13):
        g = R.fill(L, 100 + step, "normal").g
        b.g.t.copy_(torch.from_numpy(g))
        K.grad_norm_clip(b.g.t, T.off.t, T.len.t, T.act.t, L.nseg, 0.7, ws.t, norm.t, coef.t)
        K.counter_add(stepd, 1)
        K.radam_step(b.p.t, b.g.t, b.m.t, b.v.t, T.off.t, T.len.t, T.wd.t, T.act.t, L.nseg, L.total, step, R.LR, 0.9, 0.95,
                     R.EPS, gscale=coef.t, step_ptr=stepd)
        torch.cuda.synchronize()
        want_norm, want_coef = R.clip64(g, sg, 0.7)
        np.testing.assert_allclose(norm.np()[0], want_norm, rtol=2e-6)
        p, m, v = R.radam_step64(p, g, m, v, sg, step, R.LR, 0.9, 0.95, R.EPS, gscale=want_coef)
        got = b.p.np()
        np.testing.assert_allclose(got[live], p[live], rtol=2e-6, atol=2e-7, err_msg=f"step {step}")
        assert np.array_equal(R.bits(got[~live]), R.bits(st.p[~live]))
    assert int(stepd.item()) == 12
    ws.check()


def _refusal_args(L, st):
    T = _Table(L)
    b = types.SimpleNamespace(p=_Buf(st.p), g=_Buf(st.g), m=_Buf(st.m), v=_Buf(st.v))
    return T, b, dict(param=b.p.t, grad=b.g.t, m=b.m.t, v=b.v.t, seg_off=T.off.t, seg_len=T.len.t, seg_wd=T.wd.t,
                      seg_active=T.act.t, nseg=L.nseg, total=L.total, step=3, lr=R.LR, beta1=0.9, beta2=0.999, eps=R.EPS)


REFUSALS = {
    "total % 4 != 0": lambda a: a.update(total=a["total"] - 2),
    "misaligned p": lambda a: a.update(param=a["param"][1:]),
    "misaligned v": lambda a: a.update(v=a["v"][1:]),
    "nseg 0": lambda a: a.update(nseg=0),
    "nseg 1025": None,
    "step 0 without step_ptr": lambda a: a.update(step=0),
}


@pytest.mark.parametrize("with_ops", [False, True])
@pytest.mark.parametrize("case", sorted(REFUSALS))
def test_radam_refusals_write_nothing(case, with_ops):
    from arcweld import _native as nat
    from arcweld import kernels as K
    L = R.many_layout(1025) if case == "nseg 1025" else _layout("ragged/a4/all")
    st = R.fill(L, 5, "normal")
    T, b, args = _refusal_args(L, st)
    if REFUSALS[case]:
        REFUSALS[case](args)
    out = None
    if with_ops:
        args["ops"], out = _one_ops_table(L)
    with pytest.raises(nat.NativeError):
        K.radam_step(**args)
    torch.cuda.synchronize()
    for nm in "pgmv":
        assert np.array_equal(R.bits(getattr(b, nm).np()), R.bits(getattr(st, nm))), f"{case}: {nm} was written"
    if out is not None:
        assert (out.np() == SENT).all()
    if case == "nseg 1025":             # the norm refuses it too
        ws, o = _Buf(shape=(K.NORM_WS,), dtype=torch.float64, fill=0.0), _Buf(shape=(2,), fill=5.0)
        with pytest.raises(nat.NativeError):
            K.grad_norm_clip(b.g.t, T.off.t, T.len.t, T.act.t, L.nseg, 1.0, ws.t, o.t[0:1], o.t[1:2])
        torch.cuda.synchronize()
        assert (o.np() == 5.0).all() and not ws.np().any()


def test_ops_form_refuses_2_31_elements():
    """Only the count says 2^31: nothing of that size exists, and the refusal comes before any launch."""
    from arcweld import _native as nat
    from arcweld import kernels as K
    L = _layout("ragged/a4/all")
    st = R.fill(L, 5, "normal")
    T, b, args = _refusal_args(L, st)
    args["ops"], out = _one_ops_table(L)
    args["total"] = 2 ** 31
    with pytest.raises(nat.NativeError, match="2\\^31"):
        K.radam_step(**args)
    torch.cuda.synchronize()
    for nm in "pgmv":
        assert np.array_equal(R.bits(getattr(b, nm).np()), R.bits(getattr(st, nm)))
    assert (out.np() == SENT).all()


# ------------------------------------------------------------------------------------------------ clip norm
def _clip(L, g, max_norm, T=None):
    from arcweld import kernels as K
    T = T or _Table(L)
    gb = _Buf(g)
    ws, o = _Buf(shape=(K.NORM_WS,), dtype=torch.float64, fill=0.0), _Buf(shape=(2,), fill=-5.0)
    K.grad_norm_clip(gb.t, T.off.t, T.len.t, T.act.t, L.nseg, max_norm, ws.t, o.t[0:1], o.t[1:2])
    torch.cuda.synchronize()
    ws.check()
    assert np.array_equal(R.bits(gb.np()), R.bits(g)), "the gradient was written"
    n, c = o.np()
    return np.float32(n), np.float32(c)


def _check_clip(L, g, max_norm, label, nt=512, got=None):
    norm, coef = got or _clip(L, g, max_norm)
    want, _ = R.clip64(g, R.segs(L), max_norm)
    rtol = R.norm_rtol(L.total, nt)
    print(f"{label}: norm {norm:.9g} (fp64 {want:.9g}), |diff| / allowance = "
          f"{abs(float(norm) - want) / (rtol * want) if want else 0.0:.3f}, coef {coef:.9g}")
    assert np.isfinite(norm) and abs(float(norm) - want) <= rtol * want, f"{label}: norm"
    c32 = R.coef32(norm, max_norm)
    assert abs(float(coef) - float(c32)) <= float(np.spacing(c32)), \
        f"{label}: coef is not min(1, max_norm / (norm + 1e-6))"
    return norm, coef


@pytest.mark.parametrize("name", SMALL_LAYOUTS + ["strided"])
def test_clip_norm_against_fp64(name):
    L = _layout(name)
    g = _state(name, "normal").g
    want, _ = R.clip64(g, R.segs(L), 1.0)
    if not L.active.any():
        norm, coef = _check_clip(L, g, 0.7, f"{name} no active segment")
        assert norm == 0.0 and coef == 1.0
        return
    norm, coef = _check_clip(L, g, 2 * want, f"{name} below max_norm")
    assert coef == 1.0
    norm, coef = _check_clip(L, g, 0.1 * want, f"{name} above max_norm")
    assert coef < 1.0
    if name != "strided":
        zero = np.where(R.masks(L)[1], np.float32(0), g).astype(np.float32)      # NaN / 1e30 stay where nobody reads
        norm, coef = _check_clip(L, zero, 0.7, f"{name} zero gradients")
        assert norm == 0.0 and coef == 1.0
        spread = g.copy()
        for s, (o, n, _, a) in enumerate(R.segs(L)):
            if a:
                spread[o:o + n] *= np.float32(1e4 if s == 8 else 1e-4)
        _check_clip(L, spread, 0.7, f"{name} magnitude spread")


_CHILD = """
import sys
sys.path[:0] = {paths!r}
import numpy as np, torch
import optim_refs as R
from arcweld import kernels as K
L = R.make_layout(R.RAGGED, align=4, active=R.active_patterns(12)["two-off"])
L2 = R.strided_layout()
for L in (L, L2):
    g = R.fill(L, 4321, "normal").g
    d = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    ws, out = torch.zeros(K.NORM_WS, dtype=torch.float64, device="cuda"), torch.zeros(2, device="cuda")
    K.grad_norm_clip(d(g), d(L.off), d(L.len), d(L.active), L.nseg, 0.7, ws, out[0:1], out[1:2])
    torch.cuda.synchronize()
    print("NORM", repr(float(out[0])), repr(float(out[1])), int((ws != 0).sum()))
"""


def test_clip_norm_with_256_thread_workgroups_in_a_child_process():
    """AW_NORM_THREADS=256 is read once per process: a fresh child runs sumsq_kernel<256> on the ragged and the strided
    layout and prints what it got."""
    here = os.path.dirname(os.path.abspath(__file__))
    paths = [here, os.path.dirname(here), os.path.join(os.path.dirname(here), "vq-vae-transformer-arc-welding_amd")]
    env = dict(os.environ, AW_NORM_THREADS="256")
    r = subprocess.run([sys.executable, "-c", _CHILD.format(paths=paths)], env=env, capture_output=True, text=True,
                       timeout=240)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [ln.split() for ln in r.stdout.splitlines() if ln.startswith("NORM")]
    assert len(lines) == 2
    layouts = (R.make_layout(R.RAGGED, align=4, active=R.active_patterns(12)["two-off"]), R.strided_layout())
    for (_, n, c, nws), L in zip(lines, layouts):
        g = R.fill(L, 4321, "normal").g
        _check_clip(L, g, 0.7, f"256 threads, total {L.total}", nt=256, got=(np.float32(float(n)), np.float32(float(c))))
        assert int(nws) == min((L.total // 4 + 255) // 256, R.NORM_WS)       # one partial per 256-thread workgroup


@pytest.mark.parametrize("n", [1, 3, 255, 257, 4099, 4096 * 256 + 13])
def test_scale_is_one_f32_multiply(n):
    from arcweld import kernels as K
    x = np.resize(gen.normal(9, (min(n, 65521),), 3.0), n)
    s = np.float32(0.37)
    b, sd = _Buf(x), _place([s])
    K.scale_(b.t, sd.t)
    torch.cuda.synchronize()
    assert np.array_equal(R.bits(b.np()), R.bits(x * s))


# ------------------------------------------------------------------------------------------------ operand copies
# (mode, (O, I, k), tap, ldo): the segment stores the weight in the mode's storage order
OPS_CASES = [[(0, (5, 7, 3), 0, 0)], [(0, (5, 7, 3), 1, 0)], [(0, (5, 7, 3), 2, 0)],
             [(0, (4, 8, 1), 0, 0)], [(0, (5, 7, 1), 0, 0)],
             [(1, (5, 7, 3), 0, 0)], [(1, (4, 8, 3), 0, 0)], [(2, (5, 7, 3), 0, 0)], [(2, (4, 8, 3), 0, 0)],
             [(3, (5, 6, 5), 0, 0)],                                  # convT (I_in, O, k) = (6, 5, 5)
             [(4, (7, 1, 25), 0, 32)],
             [(5, (7, 9, 1), 0, 0)], [(5, (8, 8, 1), 0, 0)],
             [(7, (5, 8, 3), 0, 0)], [(7, (5, 4, 3), 0, 0)], [(7, (5, 6, 3), 0, 0)],
             [(1, (5, 7, 3), 0, 0), (2, (5, 7, 3), 0, 0)],            # two operands on one segment
             [(5, (5, 24, 1), 0, 0), (7, (5, 8, 3), 0, 0)],
             [(5, (8, 8, 1), 0, 0, "unaligned")],
             [(1, (4, 8, 3), 0, 0), (5, (4, 24, 1), 0, 0)]]           # the last segment is inactive
OPS_INACTIVE = len(OPS_CASES) - 1


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32])
@pytest.mark.parametrize("step,src", [(5, "host"), (6, "ptr")])
def test_operand_copies_are_the_relayout_of_the_stored_weights(dtype, step, src):
    from arcweld import _native as nat
    from arcweld import kernels as K
    lens = [int(np.prod(R.storage_shape(c[0][0], *c[0][1]))) for c in OPS_CASES]
    for c, n in zip(OPS_CASES, lens):
        assert all(int(np.prod(R.storage_shape(d[0], *d[1]))) == n for d in c)
    L = R.make_layout(lens, align=64, active=[0 if i == OPS_INACTIVE else 1 for i in range(len(lens))])
    st = R.fill(L, 900, "normal")
    table = (nat.OperandDesc * (nat.OPS_PER_SEG * L.nseg))()
    outs = []
    for s, case in enumerate(OPS_CASES):
        for j in range(nat.OPS_PER_SEG):
            d = table[nat.OPS_PER_SEG * s + j]
            if j >= len(case):
                d.mode = -1
                continue
            mode, (O, I, k), tap, ldo = case[j][:4]
            n_out = R.relayout_ref(np.zeros(lens[s]), mode, O, I, k, tap, ldo).size
            shift = 1 if len(case[j]) > 4 else 0
            ob = _Buf(shape=(n_out + shift,), dtype=dtype, fill=SENT)
            view = ob.t[shift:]
            assert (view.data_ptr() % 16 != 0) == bool(shift)
            d.out, d.O, d.I, d.k, d.tap, d.mode, d.ldo = view.data_ptr(), O, I, k, tap, mode, ldo
            d.dtype = K.dtype_code(dtype)
            outs.append((s, case[j], ob, shift))
    ops = torch.frombuffer(bytearray(bytes(table)), dtype=torch.uint8).to("cuda")
    tag = "decoder"
    plain = _launch(L, st, step, R.BETAS[tag], src, 0.37, zero_grad=True)
    got = _launch(L, st, step, R.BETAS[tag], src, 0.37, zero_grad=True, ops=ops)
    for nm in "pgmv":
        assert np.array_equal(R.bits(getattr(got, nm)), R.bits(getattr(plain, nm))), f"{nm} differs from aw_radam_step"
    live = R.masks(L)[0]
    assert (got.p[live] != st.p[live]).mean() > 0.9
    sent_bits = torch.tensor([SENT]).to(dtype).view(torch.int16 if dtype == torch.bfloat16 else torch.int32).item()
    for s, (mode, (O, I, k), tap, ldo, *_), ob, shift in outs:
        o, n = int(L.off[s]), lens[s]
        label = f"segment {s} mode {mode} (O, I, k) = {(O, I, k)} tap {tap} {dtype}"
        out_bits = ob.tbits()
        if shift:
            assert out_bits[0] == sent_bits, f"{label}: the element before an unaligned out was written"
            out_bits = out_bits[1:]
        if s == OPS_INACTIVE:
            assert (out_bits == sent_bits).all(), f"{label}: an inactive segment's operand was written"
            continue
        cast = torch.from_numpy(got.p[o:o + n].copy()).to(dtype)                 # torch's RNE cast of the stored p
        p_bits = cast.view(torch.int16 if dtype == torch.bfloat16 else torch.int32).numpy()
        want = R.relayout_ref(p_bits, mode, O, I, k, tap, ldo, pad=sent_bits).reshape(-1)
        assert np.array_equal(out_bits, want), f"{label}: {int((out_bits != want).sum())} of {want.size} elements"


# ------------------------------------------------------------------------------------------------ relayout family
def _as_bits(t):
    return t.contiguous().cpu().view(torch.int16 if t.dtype == torch.bfloat16 else torch.int32).numpy()


def _want_relayout(W, dtype, mode, O, I, k, tap, ldo):
    ref = R.relayout_ref(W, mode, O, I, k, tap, ldo, pad=0.0)
    return _as_bits(torch.from_numpy(np.ascontiguousarray(ref, np.float32)).to(dtype)).reshape(-1)


RELAYOUTS = [(0, (5, 7, 3), 0, 0), (0, (5, 7, 3), 1, 0), (0, (5, 7, 3), 2, 0), (1, (5, 7, 3), 0, 0), (2, (5, 7, 3), 0, 0),
             (3, (5, 6, 5), 0, 0), (4, (3, 1, 25), 0, 25), (4, (3, 1, 25), 0, 33)]
BATCH_ONLY = [(5, (5, 7, 1), 0, 0), (7, (5, 7, 3), 0, 0), (7, (5, 8, 3), 0, 0)]
BIG_JOB = (1, (150, 151, 3), 0, 0)                 # 67950 elements: the batch's 256 x 256 threads stride


def _job(case, seed, dtype):
    mode, (O, I, k), tap, ldo = case
    W = gen.normal(seed, R.storage_shape(mode, O, I, k), 1.0)
    Wd = _place(W)
    n_out = R.relayout_ref(W, mode, O, I, k, tap, ldo).size
    return W, Wd, _Buf(shape=(n_out,), dtype=dtype, fill=SENT)


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32])
def test_weight_relayout_against_permutes(dtype):
    from arcweld import kernels as K
    for i, case in enumerate(RELAYOUTS):
        mode, (O, I, k), tap, ldo = case
        W, Wd, out = _job(case, 50 + i, dtype)
        K.weight_relayout(Wd.t, O, I, k, tap, mode, out.t, ldo=ldo)
        torch.cuda.synchronize()
        Wd.check()
        assert np.array_equal(out.tbits(), _want_relayout(W, dtype, mode, O, I, k, tap, ldo)), f"{case} {dtype}"


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32])
def test_weight_relayout_batch_against_permutes(dtype):
    from arcweld import kernels as K
    cases = (RELAYOUTS + BATCH_ONLY) * 4
    cases = cases[:K.RELAYOUT_MAX_JOBS - 1] + [BIG_JOB]
    assert len(cases) == K.RELAYOUT_MAX_JOBS == 40 and BIG_JOB[1][0] * BIG_JOB[1][1] * 3 > 256 * 256
    made = [_job(c, 70 + i, dtype) for i, c in enumerate(cases)]
    K.weight_relayout_batch([(Wd.t, c[1][0], c[1][1], c[1][2], c[2], c[0], out.t, c[3])
                             for c, (_, Wd, out) in zip(cases, made)])
    torch.cuda.synchronize()
    for c, (W, Wd, out) in zip(cases, made):
        mode, (O, I, k), tap, ldo = c
        Wd.check()
        assert np.array_equal(out.tbits(), _want_relayout(W, dtype, mode, O, I, k, tap, ldo)), f"{c} {dtype}"
    for one in (RELAYOUTS + BATCH_ONLY):                              # and each on its own (a one-job batch)
        mode, (O, I, k), tap, ldo = one
        W, Wd, out = _job(one, 7, dtype)
        K.weight_relayout_batch([(Wd.t, O, I, k, tap, mode, out.t, ldo)])
        torch.cuda.synchronize()
        assert np.array_equal(out.tbits(), _want_relayout(W, dtype, mode, O, I, k, tap, ldo)), f"single {one} {dtype}"


@pytest.mark.parametrize("what", ["41 jobs", "mode 6", "single-call mode 5"])
def test_relayout_refusals_write_nothing(what):
    from arcweld import _native as nat
    from arcweld import kernels as K
    n = 41 if what == "41 jobs" else 3
    made = [_job((5, (5, 7, 1), 0, 0), 90 + i, torch.float32) for i in range(n)]
    with pytest.raises(nat.NativeError):
        if what == "single-call mode 5":
            K.weight_relayout(made[0][1].t, 5, 7, 1, 0, 5, made[0][2].t)
        else:
            arr = (nat.RelayoutJob * n)()
            for i, (r, (_, Wd, out)) in enumerate(zip(arr, made)):
                r.W, r.out, r.O, r.I, r.k, r.tap, r.ldo = Wd.t.data_ptr(), out.t.data_ptr(), 5, 7, 1, 0, 0
                r.mode = 6 if (what == "mode 6" and i == 1) else 5
            nat.call("aw_weight_relayout_batch", arr, n, nat.AW_F32, nat.stream_ptr())
    torch.cuda.synchronize()
    for _, _, out in made:
        assert (out.np() == SENT).all()


@pytest.mark.parametrize("mode,O,I,k,tap,rows,row", [(0, 5, 7, 3, 0, 5, 7), (0, 5, 7, 3, 2, 5, 7), (1, 5, 7, 3, 0, 5, 21),
                                                     (3, 5, 6, 5, 0, 25, 6), (4, 3, 1, 25, 0, 3, 25),
                                                     (1, 90, 91, 3, 0, 90, 273)])
def test_weight_grad_scatter_is_one_add_per_element(mode, O, I, k, tap, rows, row):
    from arcweld import kernels as K
    ldg = row + 5
    g = np.full((rows, ldg), np.nan, np.float32)
    g[:, :row] = gen.normal(21 + mode, (rows, row), 1.0)
    G0 = gen.normal(22 + mode, R.storage_shape(mode, O, I, k), 1.0)
    gd, Gb = _place(g), _Buf(G0)
    K.weight_grad_scatter(gd.t, O, I, k, tap, mode, Gb.t)
    torch.cuda.synchronize()
    gd.check()
    S = R.scatter_ref(g, mode, O, I, k, tap).astype(np.float32)
    got = Gb.np()
    assert np.array_equal(R.bits(got), R.bits(G0 + S))
    if mode == 0:
        other = [j for j in range(k) if j != tap]
        assert np.array_equal(R.bits(got[:, :, other]), R.bits(G0[:, :, other]))
        assert (got[:, :, tap] != G0[:, :, tap]).all()


def _cast_inputs(n):
    special = np.array([0x3F808000, 0x3F818000, 0x3F80FFFF, 0x3F807FFF, 0x3F808001,       # ties to even, both sides
                        0x3FFFFFFF, 0x3FFF8000, 0xBFFFC000,                               # up into the next exponent
                        0x7F7F0000, 0x7F7F7FFF, 0x7F7F8000, 0x7F7FFFFF, 0xFF7FFFFF,       # around the largest finite bf16
                        0x7F800000, 0xFF800000, 0x7FC00000, 0x7F800001, 0xFFC12345,       # inf, NaN
                        0x00000000, 0x80000000, 0x00000001, 0x00008000, 0x00018000, 0x807FFFFF], np.uint32)
    x = R.bits(np.resize(gen.normal(31, (min(n, 65521),), 10.0), n)).copy()
    x[:min(n, special.size)] = special[:n]
    if n > 100:
        x[-special.size:] = special
    return x.view(np.float32)


@pytest.mark.parametrize("n", [1, 24, 63, 257, 4099, 8192 * 256 + 77])      # the last: past the grid cap
def test_cast_is_round_to_nearest_even(n):
    from arcweld import kernels as K
    x = _cast_inputs(n)
    xd = _place(x)
    for dtype in (torch.bfloat16, torch.float32):
        out = _Buf(shape=(n,), dtype=dtype, fill=SENT)
        K.cast(xd.t, out.t)
        torch.cuda.synchronize()
        got, want = out.tbits(), _as_bits(torch.from_numpy(x.copy()).to(dtype))
        nan = np.isnan(x)
        assert np.array_equal(got[~nan], want[~nan]), f"n = {n} {dtype}"
        back = out.np()
        assert np.isnan(back[nan]).all() and not np.isnan(back[~nan]).any()
    xd.check()
