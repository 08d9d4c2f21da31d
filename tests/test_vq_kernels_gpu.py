"""csrc/vq.hip -- the nearest-code search behind aw_vq_forward (both kernels), vq_finalize, vq_backward and
vq_onehot -- against the fp64 restatements of tests/vq_refs.py, at ragged K and N, every reachable instantiation and
both count paths.  Every buffer sits between margins: z and E inside NaN-filled allocations (a read outside them
surfaces as a NaN distance, which is never taken -- a wrong code), every output between canaries that are checked
after every launch (a write to row N, code K or element N D shows).

Exact block: integer inputs (vq_refs.exact_case) make every f32 distance exact, with ties on every row at lane, lane
half, MFMA tile, wave and code tile distances: idx, z_q, counts, sqerr and the operand copies are compared bit for bit.
Random block: the derived bound of vq_refs.eps on every row; the two kernels are NOT compared with each other (their
norm chains round differently).  The allowances are derived in vq_refs.py and measured on the CPU in
tests/test_vq_refs_cpu.py.

Which exact case reaches which kernel (aw_vq_forward's dispatch: pinned when K <= 512 and D in 16 / 32 / 64, else
streaming with 32-row workgroups (RPL 4) when N < 32768 and D <= 64, 64-row ones (RPL 8) otherwise):
  pinned<16>       (1, 16, 1) (65, 16, 65) (509, 16, 63)         pinned<32>   (3, 32, 63) (100, 32, 200) (512, 32, 64)
  pinned<64>       (64, 64, 64) (509, 64, 65) (512, 64, 200) (100, 64, 1)
  streaming<16,4>  (513, 16, 1) (1030, 16, 100) (520, 16, 33) (15700, 16, 65) (16001, 16, 65)
  streaming<32,4>  (520, 32, 31) (513, 32, 100)                  streaming<64,4>  (1030, 64, 33) (513, 64, 100)
  streaming<16,8>  (513, 16, 32805)    streaming<32,8>  (513, 32, 32805)    streaming<64,8>  (520, 64, 32805)
  streaming<128,8> (7, 128, 1) (513, 128, 70) (8197, 128, 70) (15700, 128, 64)
  streaming<256,8> (513, 256, 63) (7, 256, 70) (8197, 256, 63) (16001, 256, 64)
streaming<128,4> and <256,4> are compiled but the dispatch never selects them (only ARCWELD_VQ_ROWS=32 does, a
process-wide A/B switch read once).  Counts: the LDS histogram serves every case up to its capacity (15488 codes at 64
rows, 16000 at 32: (15700, 16, 65) is the largest), global atomics (16001, 16, 65), (16001, 256, 64) and
(15700, 128, 64)."""
import types

import numpy as np
import pytest
import torch

import vq_refs as R
from oracle import gen

pytestmark = pytest.mark.gpu

PAD = 64
CANARY_F, CANARY_I = -1024.0, -77
BETA = 0.25


class _Out:
    """A device tensor of `shape` between two PAD-long canary margins, itself filled with `fill` (the canary unless
    given).  .t is the view the kernel gets: 16-byte aligned (PAD elements of any dtype here are a multiple of it)."""

    def __init__(self, shape, dtype=torch.float32, fill=None):
        self.n = int(np.prod(shape))
        self.canary = CANARY_I if dtype == torch.int64 else CANARY_F
        self.fill = self.canary if fill is None else fill
        self.buf = torch.full((self.n + 2 * PAD,), self.canary, dtype=dtype, device="cuda")
        self.t = self.buf[PAD:PAD + self.n].view(shape)
        self.t.fill_(self.fill)
        assert self.t.data_ptr() % 16 == 0

    def check(self):
        ok = (self.buf[:PAD] == self.canary).all() and (self.buf[PAD + self.n:] == self.canary).all()
        assert bool(ok), "a canary next to an output was written"

    def untouched(self):
        self.check()
        assert bool((self.t == self.fill).all()), "an output was written by a refused call"

    def np(self):
        return (self.t.float() if self.t.dtype == torch.bfloat16 else self.t).cpu().numpy()


def _place(a):
    """(n, D) f32 on the device inside a NaN-filled allocation, PAD NaN floats on either side, 16-byte aligned."""
    a = np.ascontiguousarray(a, dtype=np.float32)
    buf = torch.full((a.size + 2 * PAD,), float("nan"), device="cuda")
    view = buf[PAD:PAD + a.size].view(a.shape)
    if a.size:
        view.copy_(torch.as_tensor(a))
    assert view.data_ptr() % 16 == 0
    return view


def _forward(z, E, groups=1, copy=None, zd=None, Ed=None):
    """One aw_vq_forward launch; the outputs (as _Out) after the canary checks."""
    from arcweld import kernels as K
    (N, D), Kc = z.shape, len(E)
    o = types.SimpleNamespace(zq=_Out((N, D)), idx=_Out((N,), torch.int64), counts=_Out((groups * Kc,), fill=0.0),
                              sq=_Out((1,), torch.float64, fill=0.0), zc=_Out((N, D), copy) if copy else None)
    K.vq_forward(_place(z) if zd is None else zd, _place(E) if Ed is None else Ed, o.zq.t, o.idx.t, o.counts.t, o.sq.t,
                 zq_copy=o.zc.t if copy else None, count_groups=groups)
    torch.cuda.synchronize()
    for b in (o.zq, o.idx, o.counts, o.sq) + ((o.zc,) if copy else ()):
        b.check()
    return o


def _finalize(counts, sqerr, N, Kc, D, groups):
    """(loss, perplexity) of aw_vq_finalize over host counts (groups * K,) and an f64 sqerr."""
    from arcweld import kernels as K
    c = _Out((groups * Kc,))
    c.t.copy_(torch.as_tensor(np.asarray(counts, np.float32)))
    sq = torch.tensor([sqerr], dtype=torch.float64, device="cuda")
    out = _Out((2,))
    K.vq_finalize(c.t, sq, N, Kc, D, BETA, out.t[0:1], out.t[1:2], count_groups=groups)
    torch.cuda.synchronize()
    out.check()
    c.check()
    assert np.array_equal(c.np(), np.asarray(counts, np.float32))
    return out.np().astype(np.float64)


def _check_finalize(got, counts, sqerr, N, Kc, D, label):
    want_loss, want_perp = R.finalize_ref(counts, sqerr, N, Kc, D, BETA)
    tol = R.perplexity_tol(counts, N, Kc)
    print(f"{label}: loss {got[0]:.8g} (want {want_loss:.8g}), perplexity {got[1]:.8g} (want {want_perp:.8g}, "
          f"|diff| / allowance = {abs(got[1] - want_perp) / tol:.3g})")
    assert abs(got[0] - want_loss) <= R.LOSS_RTOL * abs(want_loss), f"{label}: loss"
    assert abs(got[1] - want_perp) <= tol, f"{label}: perplexity"


# ------------------------------------------------------------------------------------------------ exact block
# (K, D, N, count_groups): see the module docstring for the kernel each one reaches
EXACT = (
    (1, 16, 1, 1), (3, 32, 63, 1), (64, 64, 64, 1), (65, 16, 65, 3), (100, 32, 200, 3), (509, 64, 65, 3),
    (512, 32, 64, 1), (512, 64, 200, 1), (509, 16, 63, 1), (100, 64, 1, 1),
    (513, 16, 1, 1), (520, 32, 31, 1), (1030, 64, 33, 3), (513, 64, 100, 1), (1030, 16, 100, 1), (520, 16, 33, 1),
    (513, 32, 100, 3),
    (513, 16, 32805, 8), (520, 64, 32805, 1), (513, 32, 32805, 1),
    (7, 128, 1, 1), (513, 256, 63, 1), (8197, 128, 70, 3), (7, 256, 70, 1), (8197, 256, 63, 1), (513, 128, 70, 1),
    (16001, 16, 65, 3), (16001, 256, 64, 1), (15700, 16, 65, 1), (15700, 128, 64, 1))


@pytest.mark.parametrize("Kc, D, N, groups", EXACT)
def test_exact_on_integer_inputs(Kc, D, N, groups):
    c = R.exact_case(1000 + Kc + D + N, Kc, D, N)
    zd, Ed = _place(c.z), _place(c.E)
    label = f"K={Kc} D={D} N={N} groups={groups}"
    for copy in (torch.float32, torch.bfloat16):
        o = _forward(c.z, c.E, groups, copy, zd, Ed)
        R.check_exact(c, o.idx.np(), o.zq.np(), o.counts.np(), o.sq.np()[0], label=label)
        assert torch.equal(o.zc.t, o.zq.t.to(copy)), f"{label}: the {copy} operand copy is not the cast of z_q"
        assert np.array_equal(R.bits(o.zc.np()), R.bits(c.zq)), f"{label}: {copy} operand copy"   # -3..3: exact in bf16
    counts = o.counts.np()
    assert (counts >= 0).all() and np.array_equal(counts, np.rint(counts))
    _check_finalize(_finalize(counts, o.sq.np()[0], N, Kc, D, groups), c.counts, c.sqerr, N, Kc, D, label)


# ------------------------------------------------------------------------------------------------ random block
# vq_refs.REGIMES, their pinned counterparts (e_std None: the untrained codebook U(+-1/K)) and the streaming D = 32
RANDOM = R.REGIMES + ((509, 64, 999, .08, .08), (100, 16, 65, .08, .08), (512, 32, 130, .08, None),
                      (513, 32, 100, .08, .08))


@pytest.mark.parametrize("Kc, D, N, z_std, e_std", RANDOM)
def test_random_within_the_derived_bound(Kc, D, N, z_std, e_std):
    z, E = R.random_case(500 + Kc + D + N, Kc, D, N, z_std, e_std)
    label = f"K={Kc} D={D} N={N} std={z_std}/{e_std}"
    o = _forward(z, E, groups=2)
    idx = o.idx.np()
    R.check_indices(z, E, idx, label=label)
    print(f"{label}: {int((idx != R.dist64(z, E).argmin(1)).sum())} of {N} rows differ from the fp64 argmin")
    assert np.array_equal(R.bits(o.zq.np()), R.bits(R.zq_ste32(z, E, idx))), f"{label}: z_q is not z + (E[idx] - z)"
    assert np.array_equal(o.counts.np().reshape(2, Kc).sum(0), np.bincount(idx, minlength=Kc)), f"{label}: counts"
    want = R.sqerr64(z, E, idx)
    err = abs(o.sq.np()[0] - want)
    print(f"{label}: |sqerr - sqerr64| / allowance = {err / (R.SQERR_RTOL * want):.3g}")
    assert err <= R.SQERR_RTOL * want, f"{label}: sqerr"


@pytest.mark.parametrize("Kc, D, N", [(100, 32, 130), (520, 64, 100)])
def test_nan_row_gets_code_zero_and_disturbs_no_other_row(Kc, D, N):
    """One z row with a NaN in the middle of a tile (pinned and streaming kernel): the documented guard gives it
    idx 0; every other row keeps its idx and z_q bits."""
    z, E = R.random_case(600 + Kc, Kc, D, N, .08, .08)
    ref = _forward(z, E)
    row = 37
    zn = z.copy()
    zn[row, D // 2 + 1] = np.nan
    got = _forward(zn, E)
    idx, keep = got.idx.np(), np.arange(N) != row
    assert idx[row] == 0
    assert np.array_equal(idx[keep], ref.idx.np()[keep])
    assert np.array_equal(R.bits(got.zq.np()[keep]), R.bits(ref.zq.np()[keep]))
    assert np.array_equal(got.counts.np(), np.bincount(idx, minlength=Kc))


# ------------------------------------------------------------------------------------------------ backward
@pytest.mark.parametrize("Kc, D, N, one_code", [(3, 5, 7, False), (64, 16, 1000, False), (520, 64, 333, False),
                                                (64, 16, 1000, True)])
def test_backward_against_fp64(Kc, D, N, one_code):
    """vq_bwd_kernel: N D not a multiple of its 256-thread blocks, a non-zero dE to accumulate into, no upstream
    gradient, no loss gradient (dE must keep its bits), every row on one code (N atomics per dE element), and the
    operand copy of dz in both types.  g_loss is a power of two: vq_refs.backward_tols' count of roundings."""
    from arcweld import kernels as K
    z, E = gen.normal(31, (N, D), 0.5), gen.uniform(32, (Kc, D), -0.5, 0.5)
    idx = np.full(N, Kc - 1) if one_code else gen.randint(33, (N,), 0, Kc)
    g_zq, prior = gen.normal(34, (N, D), 1.0), gen.normal(35, (Kc, D), 0.01)
    zd, Ed, gd = _place(z), _place(E), _place(g_zq)
    idxd = torch.as_tensor(idx, device="cuda")
    for gz, gl in ((g_zq, -0.5), (None, 2.0), (g_zq, None)):
        for cdt in (torch.float32, torch.bfloat16, None):
            dz, dE, dc = _Out((N, D)), _Out((Kc, D)), _Out((N, D), cdt) if cdt else None
            dE.t.copy_(torch.as_tensor(prior))
            K.vq_backward(zd, Ed, idxd, None if gz is None else gd,
                          None if gl is None else torch.tensor([gl], device="cuda"), BETA, dz.t, dE.t,
                          dz_copy=dc.t if cdt else None)
            torch.cuda.synchronize()
            for b in (dz, dE) + ((dc,) if cdt else ()):
                b.check()
            label = f"K={Kc} D={D} N={N} one_code={one_code} g_zq={'yes' if gz is not None else 'None'} g_loss={gl}"
            R.check_backward(z, E, idx, gz, gl, BETA, prior, dz.np(), dE.np(), label=label)
            if cdt:
                assert torch.equal(dc.t, dz.t.to(cdt)), f"{label}: the {cdt} operand copy is not the cast of dz"


# ------------------------------------------------------------------------------------------------ finalize, one-hot
@pytest.mark.parametrize("kind, Kc, N, groups", R.FINALIZE)
def test_finalize_against_fp64(kind, Kc, N, groups):
    counts = R.finalize_counts(kind, Kc, N, groups)
    sqerr, D = 12345.678 * N, 16
    got = _finalize(counts, sqerr, N, Kc, D, groups)
    _check_finalize(got, counts, sqerr, N, Kc, D, f"{kind} K={Kc} N={N} groups={groups}")


@pytest.mark.parametrize("N, Kc", [(7, 3), (1000, 65)])
def test_onehot(N, Kc):
    from arcweld import kernels as K
    idx = gen.randint(41, (N,), 0, Kc)
    out = _Out((N, Kc))
    K.vq_onehot(torch.as_tensor(idx, device="cuda"), Kc, out.t)
    torch.cuda.synchronize()
    out.check()
    assert np.array_equal(R.bits(out.np()), R.bits(R.onehot_ref(idx, Kc)))


# ------------------------------------------------------------------------------------------------ refusals
def _forward_args(N=10, Kc=64, D=16, groups=1):
    return dict(z2d=_place(np.zeros((N, D))), E=_place(np.ones((Kc, D))), zq=_Out((N, D)).t,
                idx=_Out((N,), torch.int64).t, counts=_Out((groups * Kc,), fill=0.0).t,
                sqerr=_Out((1,), torch.float64, fill=0.0).t, zq_copy=_Out((N, D), torch.bfloat16).t)


def _refused(fn, args, match):
    """fn(**args) raises NativeError matching `match` and leaves every tensor argument as it was."""
    from arcweld import _native
    before = {k: v.clone() for k, v in args.items() if torch.is_tensor(v)}
    with pytest.raises(_native.NativeError, match=match):
        fn(**args)
    torch.cuda.synchronize()
    for k, v in before.items():
        assert torch.equal(torch.nan_to_num(args[k].float()), torch.nan_to_num(v.float())), f"{k} was written"


@pytest.mark.parametrize("Kc, D, match", [(64, 48, "unsupported embedding dim 48"), (0, 16, "bad N/K|null pointer")])
def test_unsupported_sizes_raise_and_write_nothing(Kc, D, match):
    from arcweld import _native, kernels as K
    N = 10
    o = types.SimpleNamespace(zq=_Out((N, D)), idx=_Out((N,), torch.int64), counts=_Out((max(Kc, 1),), fill=0.0),
                              sq=_Out((1,), torch.float64, fill=0.0), zc=_Out((N, D), torch.bfloat16))
    with pytest.raises(_native.NativeError, match=match):
        K.vq_forward(_place(np.zeros((N, D))), _place(np.ones((Kc, D))), o.zq.t, o.idx.t, o.counts.t, o.sq.t,
                     zq_copy=o.zc.t)
    torch.cuda.synchronize()
    for b in (o.zq, o.idx, o.counts, o.sq, o.zc):
        b.untouched()


FORWARD_REFUSALS = {
    "z transposed": (lambda a: a.update(z2d=_place(np.zeros((16, 10))).t()), "z must be a contiguous"),
    "z sliced": (lambda a: a.update(z2d=_place(np.zeros((10, 32)))[:, :16]), "z must be a contiguous"),
    "z float64": (lambda a: a.update(z2d=a["z2d"].double()), "z must be a contiguous float32"),
    "z 3-d": (lambda a: a.update(z2d=a["z2d"].view(2, 5, 16)), r"z must be \(N, D\)"),
    "E of another width": (lambda a: a.update(E=_place(np.ones((64, 32)))), "E must be a contiguous"),
    "E sliced": (lambda a: a.update(E=_place(np.ones((128, 16)))[::2]), "E must be a contiguous"),
    "zq of another shape": (lambda a: a.update(zq=_Out((11, 16)).t), "zq must be a contiguous"),
    "zq bf16": (lambda a: a.update(zq=_Out((10, 16), torch.bfloat16).t), "zq must be a contiguous float32"),
    "idx int32": (lambda a: a.update(idx=torch.zeros(10, dtype=torch.int32, device="cuda")), "idx must be a contiguous"),
    "idx too short": (lambda a: a.update(idx=_Out((9,), torch.int64).t), "idx must be a contiguous int64"),
    "idx strided": (lambda a: a.update(idx=_Out((20,), torch.int64).t[::2]), "idx must be a contiguous"),
    "idx (N, 1)": (lambda a: a.update(idx=a["idx"].view(10, 1)), "idx must be a contiguous"),
    "sqerr float32": (lambda a: a.update(sqerr=torch.zeros(1, device="cuda")), "sqerr must be a contiguous float64"),
    "sqerr of two": (lambda a: a.update(sqerr=_Out((2,), torch.float64, fill=0.0).t), "sqerr must be"),
    "counts too short": (lambda a: a.update(counts=_Out((63,), fill=0.0).t), "counts must hold"),
    "counts for one group of two": (lambda a: a.update(count_groups=2), "counts must hold"),
    "zq_copy of another shape": (lambda a: a.update(zq_copy=_Out((10, 8), torch.bfloat16).t), "zq_copy must be"),
}


@pytest.mark.parametrize("name", sorted(FORWARD_REFUSALS))
def test_forward_wrapper_refuses(name):
    from arcweld import kernels as K
    args = _forward_args()
    mutate, match = FORWARD_REFUSALS[name]
    mutate(args)
    _refused(K.vq_forward, args, match)


def _backward_args(N=10, Kc=64, D=16):
    return dict(z2d=_place(np.zeros((N, D))), E=_place(np.ones((Kc, D))), idx=torch.zeros(N, dtype=torch.int64, device="cuda"),
                g_zq=_place(np.ones((N, D))), g_loss=torch.ones(1, device="cuda"), beta=BETA, dz=_Out((N, D)).t,
                dE=_Out((Kc, D), fill=0.0).t, dz_copy=_Out((N, D), torch.bfloat16).t)


BACKWARD_REFUSALS = {
    "z transposed": (lambda a: a.update(z2d=_place(np.zeros((16, 10))).t()), "z must be a contiguous"),
    "E of another width": (lambda a: a.update(E=_place(np.ones((64, 32)))), "E must be a contiguous"),
    "idx int32": (lambda a: a.update(idx=a["idx"].int()), "idx must be a contiguous int64"),
    "idx too short": (lambda a: a.update(idx=a["idx"][:9]), "idx must be a contiguous int64"),
    "g_zq of another shape": (lambda a: a.update(g_zq=_place(np.ones((10, 8)))), "g_zq must be a contiguous"),
    "g_zq transposed": (lambda a: a.update(g_zq=_place(np.ones((16, 10))).t()), "g_zq must be a contiguous"),
    "g_loss float64": (lambda a: a.update(g_loss=a["g_loss"].double()), "g_loss must be one float32"),
    "g_loss of two": (lambda a: a.update(g_loss=torch.ones(2, device="cuda")), "g_loss must be one float32"),
    "dz of another shape": (lambda a: a.update(dz=_Out((9, 16)).t), "dz must be a contiguous"),
    "dE of another shape": (lambda a: a.update(dE=_Out((63, 16), fill=0.0).t), "dE must be a contiguous"),
    "dE sliced": (lambda a: a.update(dE=_Out((128, 16), fill=0.0).t[::2]), "dE must be a contiguous"),
    "dz_copy float64": (lambda a: a.update(dz_copy=_Out((10, 16), torch.float64).t), "dz_copy must be a contiguous"),
}


@pytest.mark.parametrize("name", sorted(BACKWARD_REFUSALS))
def test_backward_wrapper_refuses(name):
    from arcweld import kernels as K
    args = _backward_args()
    mutate, match = BACKWARD_REFUSALS[name]
    mutate(args)
    _refused(K.vq_backward, args, match)


def test_wrappers_accept_what_the_model_passes():
    """The checks refuse nothing the callers pass: a 0-d g_loss, counts longer than needed, no copies."""
    from arcweld import kernels as K
    a = _forward_args()
    a["counts"] = _Out((200,), fill=0.0).t
    a["zq_copy"] = None
    K.vq_forward(**a)
    b = _backward_args()
    b["g_loss"], b["dz_copy"], b["g_zq"] = torch.ones((), device="cuda"), None, None
    K.vq_backward(**b)
    torch.cuda.synchronize()
    assert bool((a["idx"] == 0).all()) and float(a["counts"].sum()) == 10
