"""The causal-attention training kernels (aw_attn_fwd / aw_attn_bwd: the MFMA kernels of csrc/attention.hip for bf16 at
head size 64, the VALU kernels of csrc/transformer.hip otherwise) against the fp64 reference of tests/kernel_refs.py on
peaked inputs.

tests/test_gpu_attention.py feeds randn, whose scaled logits are ~ N(0, 1): the MFMA forward's lazy rescale (alpha, the
o / l rescale, the max that lse is taken from) never fires there after the first tile, and the backward's
exp2(s c2 - lse log2 e) never sees an lse above ~6.  The regimes of kernel_refs.attn_regime do reach them;
tests/test_kernel_refs_cpu.py counts the rescale events of every case used here on the CPU.  Inputs are built on the
CPU from a seeded generator, so those counts are about the very numbers the kernels get.

bf16 bars: the error of kernel_refs.attn_bf16_model (fp64 arithmetic, bf16 roundings where the kernel rounds) against
the reference is what a correct kernel cannot avoid; the kernel gets twice that plus the floors of
tests/test_gpu_attention.py (2e-2 absolute, 1e-4 on the relative Frobenius error).  The factor 2 covers what the model
leaves out (f32 accumulation order, exp2 / log approximations: ~1e-5 relative against bf16 steps of 2e-3) and a
different side taken at a rounding tie.  f32 bars: kernel_refs.close_out / close, the project's own.  Each test prints
its figures before it asserts (pytest -s shows them; DESIGN.md holds the measured tables).
"""
import functools

import pytest
import torch

import kernel_refs as kr

pytestmark = pytest.mark.gpu

GUARD = 64          # elements on either side of a guarded view
NAMES = ("y", "dq", "dk", "dv")


def run(qkv, dy, B, T, nh, d, drop=None, bufs=None):
    """Forward + backward on device tensors -> (y, lse, dqkv, ws).  ``bufs``: the four outputs to write into."""
    from arcweld import kernels as K
    kw = {"drop": drop} if drop else {}
    if bufs is None:
        bufs = (torch.empty(B * T, d, device="cuda", dtype=qkv.dtype), torch.empty(B * nh * T, device="cuda"),
                torch.empty(B * T, 3 * d, device="cuda", dtype=qkv.dtype), torch.empty(B * nh * T, device="cuda"))
    y, lse, dqkv, ws = bufs
    K.attn_fwd(qkv, B, T, nh, d, y, lse, **kw)
    K.attn_bwd(qkv, y, dy, lse, B, T, nh, d, dqkv, ws, **kw)
    torch.cuda.synchronize()
    return y, lse, dqkv, ws


def _parts(y, dqkv, d):
    return (y,) + tuple(dqkv[:, j * d:(j + 1) * d] for j in range(3))


@functools.lru_cache(maxsize=None)
def _cpu_side(path, case):
    """Inputs, fp64 reference and rounding model of one case, computed once on the CPU and shared (read-only)."""
    regime, B, nh, T, hs, dtype = case
    d = nh * hs
    qkv, dy = kr.attn_regime(regime, B, nh, T, hs, dtype, kr.attn_case_seed(B, nh, T, hs))
    keep, p = (kr.attn_keep(kr.ATTN_DROP_SEED, B, nh, T, kr.ATTN_DROP_P), kr.ATTN_DROP_P) if path == "drop" \
        else (None, 0.0)
    ref = kr.attn_train_ref(qkv, dy, B, T, nh, d, keep, p)
    model = None
    if dtype == torch.bfloat16:
        mfma = path == "mfma"       # the VALU kernels (dropout always runs on them) keep P and dS in f32
        model = kr.attn_bf16_model(qkv, dy, B, T, nh, d, keep, p, round_p=mfma, round_ds=mfma)
    return qkv, dy, ref, model


@functools.lru_cache(maxsize=None)
def _gpu_side(path, case):
    """The kernels' (y, lse, dqkv, ws) of one case, on the CPU."""
    regime, B, nh, T, hs, dtype = case
    qkv, dy, _, _ = _cpu_side(path, case)
    drop = (kr.ATTN_DROP_P, kr.ATTN_DROP_SEED) if path == "drop" else None
    return tuple(t.cpu() for t in run(qkv.cuda(), dy.cuda(), B, T, nh, nh * hs, drop))


def figures(path, case):
    """Per output: the model's and the kernel's max-abs and relative Frobenius error against the fp64 reference."""
    d = case[2] * case[4]
    _, _, ref, model = _cpu_side(path, case)
    y, lse, dqkv, _ = _gpu_side(path, case)
    out = {"lse_err": kr.max_err(lse, ref[1]), "lse_max": float(ref[1].max())}
    for i, name in enumerate(NAMES):
        r = _parts(ref[0], ref[2], d)[i]
        g = _parts(y, dqkv, d)[i]
        f = {"k_max": kr.max_err(g, r), "k_fro": kr.rel_fro(g, r), "ref_max": float(r.abs().max())}
        if model is not None:
            m = _parts(model[0], model[2], d)[i]
            f.update(m_max=kr.max_err(m, r), m_fro=kr.rel_fro(m, r))
        out[name] = f
    return out


def check_case(path, case):
    regime, B, nh, T, hs, dtype = case
    d = nh * hs
    _, _, ref, model = _cpu_side(path, case)
    y, lse, dqkv, _ = _gpu_side(path, case)
    fig = figures(path, case)
    tag = f"{path} {kr.attn_case_id(case)}"
    print(f"\n{tag}: lse max {fig['lse_max']:.1f} err {fig['lse_err']:.2e}")
    for name in NAMES:
        print(f"  {name}: " + " ".join(f"{k} {v:.3e}" for k, v in fig[name].items()))
    for t in (y, lse, dqkv):
        assert torch.isfinite(t.float()).all(), tag
    kr.close_out(lse, ref[1], f"{tag} lse")
    if dtype == torch.float32:
        kr.close_out(y, ref[0], f"{tag} y")
        for name, g, r in zip(NAMES[1:], _parts(y, dqkv, d)[1:], _parts(ref[0], ref[2], d)[1:]):
            kr.close(g, r, f"{tag} {name}")
        return
    for name in NAMES:
        f = fig[name]
        assert f["k_max"] <= 2 * f["m_max"] + 2e-2, (tag, name, f)
        assert f["k_fro"] <= 2 * f["m_fro"] + 1e-4, (tag, name, f)


@pytest.mark.parametrize("case", kr.ATTN_MFMA_CASES, ids=kr.attn_case_id)
def test_mfma_kernels_on_peaked_inputs(case):
    """attn_fwd_mfma_kernel, attn_dq_ring_kernel, attn_dkv_ring_kernel.  T = 129: one row in a second query block and
    a third key tile; 200: four tiles (the 3-deep ring wraps) and a partial last one; 257: three query blocks.  The
    lse bar (1e-4) is the one that sees a stale max in lse = m scale + log l."""
    check_case("mfma", case)


@pytest.mark.parametrize("case", kr.ATTN_VALU_CASES, ids=kr.attn_case_id)
def test_valu_kernels_on_peaked_inputs(case):
    """attn_fwd_kernel, attn_delta_kernel, attn_bwd_dq_kernel, attn_bwd_dkv_kernel: the compiled head sizes 16 / 64,
    the runtime-size kernel (hs 12) and bf16 operands (hs 32), at two and three row blocks."""
    check_case("valu", case)


@pytest.mark.parametrize("case", kr.ATTN_DROP_CASES, ids=kr.attn_case_id)
def test_probability_dropout_across_row_blocks(case):
    """p = 0.2 on more than one 64-row block, the mask regenerated from the counter hash and applied inside the
    reference and the model (bf16 at head size 64 leaves the MFMA path when p > 0)."""
    check_case("drop", case)


@pytest.mark.parametrize("path,case", [("mfma", c) for c in kr.ATTN_MFMA_CASES]
                         + [("valu", c) for c in kr.ATTN_VALU_CASES] + [("drop", c) for c in kr.ATTN_DROP_CASES],
                         ids=lambda v: v if isinstance(v, str) else kr.attn_case_id(v))
def test_delta_workspace_is_rowsum_dy_y(path, case):
    """ws after attn_bwd is delta_i = dy_i . y_i of the kernel's own y: the MFMA dQ kernel writes it for the dK/dV
    kernel's DMA, attn_delta_kernel for both VALU kernels.  An f32 fma chain of <= 128 exact products."""
    regime, B, nh, T, hs, dtype = case
    _, dy, _, _ = _cpu_side(path, case)
    y, _, _, ws = _gpu_side(path, case)
    want = (dy.double() * y.double()).view(B, T, nh, hs).sum(-1).transpose(1, 2).reshape(-1)
    scale = float(want.abs().max())
    print(f"\n{path} {kr.attn_case_id(case)}: delta max err {kr.max_err(ws, want):.3e} of max {scale:.3e}")
    torch.testing.assert_close(ws.double(), want, rtol=1e-5, atol=1e-5 * scale)


def _guarded(shape, dtype, guard_fill, body):
    """A view of ``shape`` GUARD elements into a larger buffer: guards filled with ``guard_fill``, the view with
    ``body`` (a tensor to copy, or a fill value).  The tail guard of a matrix spans 32 further rows on top of GUARD:
    the reach of a 32-row wave store that ignores its row count stays inside the buffer and is seen."""
    n = 1
    for s in shape:
        n *= s
    tail = GUARD + (32 * shape[1] if len(shape) == 2 else 0)
    buf = torch.full((GUARD + n + tail,), guard_fill, device="cuda", dtype=dtype)
    view = buf[GUARD:GUARD + n].view(shape)
    if torch.is_tensor(body):
        view.copy_(body)
    else:
        view.fill_(body)
    return buf, view, (slice(0, GUARD), slice(GUARD + n, None))


def _bits(t):
    return t.view(torch.int16 if t.dtype == torch.bfloat16 else torch.int32)


def _shape_ids(shapes):
    return [f"{'bf16' if dt == torch.bfloat16 else 'f32'}-hs{hs}-T{T}" for hs, dt, T in shapes]


GUARDED_SHAPES = [(64, torch.bfloat16, T) for T in (1, 33, 129, 200)] \
    + [(hs, torch.float32, T) for hs in (16, 12) for T in (1, 33, 70)]
INDEPENDENCE_SHAPES = [(64, torch.bfloat16, 129), (16, torch.float32, 70)]


@pytest.mark.parametrize("hs,dtype,T", GUARDED_SHAPES, ids=_shape_ids(GUARDED_SHAPES))
def test_no_access_outside_the_buffers_and_every_output_written(hs, dtype, T):
    """Every operand is a view 64 elements into a larger buffer: NaN around the inputs, a sentinel around the outputs,
    the outputs themselves NaN before the call.  Afterwards every output element is finite (written, and from
    in-bounds data), the guards are untouched, and the results are those of the plain call bit for bit (made last:
    it has no guards to catch a stray store)."""
    B, nh = 2, 2
    d = nh * hs
    qkv, dy = (t.cuda() for t in kr.attn_regime("spike", B, nh, T, hs, dtype, 300 + T + hs))
    nan = float("nan")
    gq = _guarded(qkv.shape, dtype, nan, qkv)[1]
    gdy = _guarded(dy.shape, dtype, nan, dy)[1]
    outs = [_guarded(s, dt, 1234.0, nan) for s, dt in (((B * T, d), dtype), ((B * nh * T,), torch.float32),
                                                      ((B * T, 3 * d), dtype), ((B * nh * T,), torch.float32))]
    before = [buf.clone() for buf, _, _ in outs]
    got = run(gq, gdy, B, T, nh, d, bufs=tuple(v for _, v, _ in outs))
    names = ("y", "lse", "dqkv", "ws")
    for name, (buf, view, guards), b4 in zip(names, outs, before):
        for sl in guards:
            assert torch.equal(_bits(buf[sl]), _bits(b4[sl])), f"{name}: a guard was written"
        assert torch.isfinite(view.float()).all(), f"{name}: an element is unwritten or not finite"
    assert torch.equal(_bits(gq), _bits(qkv)) and torch.equal(_bits(gdy), _bits(dy))     # inputs untouched
    plain = run(qkv, dy, B, T, nh, d)
    for name, g, p in zip(names, got, plain):
        assert torch.equal(_bits(g), _bits(p)), f"{name}: differs from the unguarded call"


@pytest.mark.parametrize("hs,dtype,T", INDEPENDENCE_SHAPES, ids=_shape_ids(INDEPENDENCE_SHAPES))
def test_batches_and_heads_are_independent_and_runs_repeat(hs, dtype, T):
    """B = 3, nh = 3 (BlockId's bh % nh, bh / nh at an nh that is no power of two): new inputs for batch 1 leave
    batches 0 and 2 bit-identical, new q, k, v columns for head 1 leave heads 0 and 2 bit-identical, and the same
    call twice gives the same bits (no atomics anywhere in attention)."""
    B, nh = 3, 3
    d = nh * hs
    qkv, dy = (t.cuda() for t in kr.attn_regime("spike", B, nh, T, hs, dtype, 500 + T))
    oq, ody = (t.cuda() for t in kr.attn_regime("big", B, nh, T, hs, dtype, 600 + T))
    base = run(qkv, dy, B, T, nh, d)
    again = run(qkv, dy, B, T, nh, d)
    for name, a, b in zip(("y", "lse", "dqkv", "ws"), base, again):
        assert torch.equal(_bits(a), _bits(b)), f"{name}: two identical calls differ"

    q2, dy2 = qkv.clone(), dy.clone()
    q2[T:2 * T], dy2[T:2 * T] = oq[T:2 * T], ody[T:2 * T]
    other = run(q2, dy2, B, T, nh, d)
    for name, a, b in zip(("y", "lse", "dqkv", "ws"), base, other):
        a3, b3 = a.view(B, -1), b.view(B, -1)            # rows (y, dqkv) and (b, h, t) vectors are both batch-major
        assert torch.equal(_bits(a3[[0, 2]]), _bits(b3[[0, 2]])), f"{name}: batch 1 leaked into batch 0 or 2"
        assert not torch.equal(_bits(a3[1]), _bits(b3[1])), name

    q3 = qkv.clone()
    for j in range(3):
        q3[:, j * d + hs:j * d + 2 * hs] = oq[:, j * d + hs:j * d + 2 * hs]
    other = run(q3, dy, B, T, nh, d)
    keep_heads = [0, 2]
    for name, a, b in zip(("y", "lse", "dqkv", "ws"), base, other):
        if name in ("lse", "ws"):
            a4, b4 = a.view(B, nh, T), b.view(B, nh, T)
            same = torch.equal(_bits(a4[:, keep_heads]), _bits(b4[:, keep_heads]))
            changed = not torch.equal(_bits(a4[:, 1]), _bits(b4[:, 1]))
        else:
            a4, b4 = a.view(B * T, -1, nh, hs), b.view(B * T, -1, nh, hs)
            same = torch.equal(_bits(a4[:, :, keep_heads]), _bits(b4[:, :, keep_heads]))
            changed = not torch.equal(_bits(a4[:, :, 1]), _bits(b4[:, :, 1]))
        assert same, f"{name}: head 1 leaked into head 0 or 2"
        assert changed, name
