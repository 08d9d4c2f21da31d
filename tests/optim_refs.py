"""fp64 restatements of csrc/optim.hip (RAdam over a flat segmented buffer, global-norm clip) and permute-built index
maps of the weight-relayout family of csrc/vqvae.hip: the instrument of tests/test_optim_kernels_gpu.py, checked on
the CPU by tests/test_optim_refs_cpu.py.  Plain numpy, no GPU.

Segments are (off, len, wd, active) tuples over flat arrays; a Layout carries them as arrays the kernels take.  The
ABI's contract (include/arcweld_amd.h): every segment starts on a multiple of 4 elements, the padding up to the next
multiple of 4 after a segment is zero in p, g, m and v, and nothing outside the float4s of active segments is read or
written.

The allowance.  radam_one (csrc/optim.hip) is a fixed sequence of f32 operations; each rounds its exact result by at
most u = 2^-24 relative.  allowance() follows the sequence on the fp64 reference's own intermediates and adds, to
first order, every rounding scaled by the magnitude of the term it rounds, carried through the later operations by
their derivatives.  A sum or difference is charged u (|a| + |b|), its operands and not its result, so the
cancellations in gr - m and p - update cannot shrink the bound below what the operands' roundings put in.  Count per
element (r = roundings):
    gr   = g gs                  1 r  (none when gs == 1: the kernel skips the multiply)
    gr   = gr + wd p             2 r  (none when wd == 0)
    d    = gr - m                1 r
    m'   = m + (1 - b1) d        2 r   (1 - b1 is exact in f32 for b1 in [0.5, 1])          m': 6 r
    gg   = gr gr                 1 r
    t1   = (1 - b2) gg           1 r
    t2   = v b2                  1 r
    v'   = t2 + t1               1 r                                                        v': 3 + 4 = 7 r
    mhat = m' / bc1              2 r   (bc1 itself is rounded to f32 once)
    unrectified:  x = mhat lr    1 r;   p' = p - x   1 r                                    p': 6 + 2 + 2 = 10 r
    rectified:    s = sqrt(v')   1 r;   den = s + eps   1 r
                  a = sqrt_bc2 / den   2 r   (sqrt_bc2 is rounded to f32 once)
                  x1 = mhat lr   1 r;   x2 = x1 a   1 r;   x3 = x2 rect   2 r   (rect is rounded to f32 once)
                  p' = p - x3    1 r                                      p': 6 + 2 + 7 (v') + 4 + 4 + 1 = 24 r
A contraction of a b + c into one fma drops a rounding and never adds one, so the bound covers either code
generation.  Terms of order u^2 are left out: they are 2^-24 of a sum of at least six terms of order u.  lr, the
betas and eps are taken at their f32 values (the C ABI takes float), so the bound covers the kernel's arithmetic only.

The norm.  sumsq_kernel squares and adds in f32 per thread (4 squares and 3 adds per float4, one add into the
accumulator per float4: at most k + 3 roundings on any path into a thread's sum of k float4s, all terms positive, so
relative (k + 3) u on the sum of squares), reduces in f64, takes the root (halving the relative error) and rounds the
norm to f32 once: within (k + 4) u of the exact norm, as norm_rtol() returns for the launch constants.
"""
import math
import types

import numpy as np

from oracle import gen

U = 2.0 ** -24
F32 = np.float32
BETAS = {"vqvae": (0.9, 0.999), "decoder": (0.9, 0.95)}       # the two setups the project trains with
LR, EPS = 1e-3, 1e-8
BIG_STEP = 10 ** 6                                            # beta2 ** t underflows for both setups
NORM_WS = 1024                                                # AW_NORM_WS
RADAM_GRID_CAP, RADAM_THREADS = 4096, 256
MAXSEG = 1024


def r32(x):
    """The value a python float has after crossing the C ABI as `float`."""
    return float(np.float32(x))


# ----------------------------------------------------------------------------------------------- scalars
def radam_scalars(step, beta1, beta2):
    """bc1, bc2, rho_inf, rho_t, rectified, rect in python floats, as torch.optim.RAdam (_single_tensor_radam)."""
    step = float(step)
    bc1 = 1 - beta1 ** step
    bc2 = 1 - beta2 ** step
    rho_inf = 2 / (1 - beta2) - 1
    rho_t = rho_inf - 2 * step * (beta2 ** step) / bc2
    rectified = rho_t > 5.0
    rect = ((rho_t - 4) * (rho_t - 2) * rho_inf / ((rho_inf - 4) * (rho_inf - 2) * rho_t)) ** 0.5 if rectified else 1.0
    return types.SimpleNamespace(bc1=bc1, bc2=bc2, rho_inf=rho_inf, rho_t=rho_t, rectified=rectified, rect=rect)


def first_rectified(beta1, beta2):
    t = 1
    while not radam_scalars(t, beta1, beta2).rectified:
        t += 1
    return t


# ----------------------------------------------------------------------------------------------- layouts
def _up(n, a):
    return (n + a - 1) // a * a


RAGGED = (1, 2, 3, 4, 5, 63, 64, 65, 255, 257, 1023, 4097)
WDS = (0.0, 0.1, 0.37)


def make_layout(lens, align=4, wds=WDS, active=None, lead=0, gaps=None):
    """Segments of `lens` elements, each start rounded up to `align` elements (4: the ABI's contract, segments back to
    back; 64: what arcweld.optim produces), weight decay cycling through `wds`, `lead` elements before the first
    segment and gaps[i] further elements before segment i."""
    off, pos = [], lead
    for i, n in enumerate(lens):
        pos = _up(pos + (gaps or {}).get(i, 0), align)
        off.append(pos)
        pos += n
    act = np.ones(len(lens), np.int32) if active is None else np.asarray(active, np.int32)
    return types.SimpleNamespace(off=np.asarray(off, np.int64), len=np.asarray(lens, np.int64),
                                 wd=np.asarray([wds[i % len(wds)] for i in range(len(lens))], np.float32),
                                 active=act, total=_up(pos, max(align, 4)), nseg=len(lens), align=align)


def with_active(L, active):
    return types.SimpleNamespace(**dict(vars(L), active=np.asarray(active, np.int32)))


def active_patterns(n):
    one = np.ones(n, np.int32)
    pats = {"all": one, "first-off": one.copy(), "last-off": one.copy(), "two-off": one.copy(),
            "none": np.zeros(n, np.int32)}
    pats["first-off"][0] = 0
    pats["last-off"][-1] = 0
    pats["two-off"][n // 2:n // 2 + 2] = 0
    return pats


def segs(L):
    return [(int(o), int(n), float(w), int(a)) for o, n, w, a in zip(L.off, L.len, L.wd, L.active)]


def masks(L):
    """(live, cover, padding): elements of active segments; those plus the rest of their last float4 (what the kernels
    may read and write); the difference (must stay zero)."""
    live, cover = np.zeros(L.total, bool), np.zeros(L.total, bool)
    for o, n, _, a in segs(L):
        if a:
            live[o:o + n] = True
            cover[o:o + _up(n, 4)] = True
    return live, cover, cover & ~live


def strided_total():
    """Just above what one trip of radam's capped grid covers and what one trip of sumsq_kernel's 4x unrolled loop
    covers (512-thread workgroups), whichever is larger -- computed from the launch constants."""
    return max(RADAM_GRID_CAP * RADAM_THREADS * 4, NORM_WS * 512 * 4 * 4) + 4 * 1000 + 12


def strided_layout():
    """About 300 ragged segments filling strided_total() elements, every 7th inactive, 4-element alignment."""
    total, n = strided_total(), 300
    base = total // n
    lens = [base - 37 + int(x) for x in gen.randint(77, (n,), 0, 23)]
    L = make_layout(lens, align=4, active=[0 if i % 7 == 3 else 1 for i in range(n)])
    assert L.total <= total
    L.total = total
    return L


def many_layout(nseg=MAXSEG):
    return make_layout([1 + i % 7 for i in range(nseg)], align=4, active=[0 if i % 5 == 2 else 1 for i in range(nseg)])


def lead_layout(align):
    """RAGGED behind a 64-element region no segment owns, with interior gaps larger than any alignment padding."""
    return make_layout(RAGGED, align=align, lead=64, gaps={3: 8, 7: 72, 11: 132}, active=active_patterns(12)["two-off"])


SENTINEL = 7.5         # in the regions no segment owns (lead, gaps): must be neither read into a result nor written


def fill(L, seed, kind, sentinel=None):
    """f32 p, g, m, v over the layout: zero padding, live values by `kind`, inactive segments NaN / 1e30, and
    `sentinel` (if given) everywhere outside the float4 cover of every segment.
    normal: unit g, non-zero m and v.  small: |g| log-uniform in [1e-9, 1e-5] with v of its order, so eps = 1e-8 is a
    visible part of sqrt(v) + eps.  zero: g = m = v = 0 (p moves by the weight decay only)."""
    T = L.total
    B = (min(T, 65521),)                   # one generated block, repeated over a longer buffer (65521 is prime)
    p = gen.normal(seed, B, 0.3)
    if kind == "normal":
        g, m, v = gen.normal(seed + 1, B, 1.0), gen.normal(seed + 2, B, 0.1), gen.uniform(seed + 3, B, 1e-3, 1.0)
    elif kind == "small":
        mag = np.exp(gen.uniform(seed + 1, B, math.log(1e-9), math.log(1e-5)).astype(np.float64))
        sign = np.where(gen.uniform(seed + 4, B) < 0.5, -1.0, 1.0)
        g = (sign * mag).astype(F32)
        m = (0.5 * sign * mag * gen.uniform(seed + 2, B, 0.5, 1.5)).astype(F32)
        v = (mag * mag * gen.uniform(seed + 3, B, 0.5, 2.0)).astype(F32)
    elif kind == "zero":
        g, m, v = (np.zeros(B, F32) for _ in range(3))
    else:
        raise ValueError(kind)
    p, g, m, v = (np.resize(x, T) for x in (p, g, m, v))
    owned = np.zeros(T, bool)
    keep = np.zeros(T, bool)
    for o, n, _, a in segs(L):
        owned[o:o + _up(n, 4)] = True
        keep[o:o + n] = True
    out = []
    for i, x in enumerate((p, g, m, v)):
        x = np.where(keep, x, F32(0)).astype(F32)
        for j, (o, n, _, a) in enumerate(segs(L)):
            if not a:
                x[o:o + n] = F32(np.nan) if (i + j) % 2 else F32(1e30)
        if sentinel is not None:
            x[~owned] = F32(sentinel)
        out.append(x)
    return types.SimpleNamespace(p=out[0], g=out[1], m=out[2], v=out[3])


# ----------------------------------------------------------------------------------------------- RAdam
def _per_element(total, sg, abi32=True):
    live, wd = np.zeros(total, bool), np.zeros(total)
    for o, n, w, a in sg:
        if a:
            live[o:o + n] = True
            wd[o:o + n] = r32(w) if abi32 else w
    return live, wd


def _trace64(p, g, m, v, wd, S, lr, b1, b2, eps, gs):
    """Every intermediate of radam_one, in fp64, in the order the head of csrc/optim.hip states."""
    t = types.SimpleNamespace()
    t.gr0 = g * gs
    t.wp = wd * p
    t.gr = t.gr0 + t.wp
    t.d = t.gr - m
    t.cd = (1 - b1) * t.d
    t.m2 = m + t.cd
    t.gg = t.gr * t.gr
    t.t1 = (1 - b2) * t.gg
    t.t2 = v * b2
    t.v2 = t.t2 + t.t1
    t.mhat = t.m2 / S.bc1
    t.x1 = t.mhat * lr
    if S.rectified:
        t.s = np.sqrt(t.v2)
        t.den = t.s + eps
        t.a = math.sqrt(S.bc2) / t.den
        t.x2 = t.x1 * t.a
        t.x3 = t.x2 * S.rect
    else:
        t.x3 = t.x1
    t.p2 = p - t.x3
    return t


def _setup(p, g, m, v, sg, step, lr, beta1, beta2, eps, gscale, abi32):
    p, g, m, v = (np.asarray(a, np.float64) for a in (p, g, m, v))
    if abi32:
        lr, beta1, beta2, eps = r32(lr), r32(beta1), r32(beta2), r32(eps)
    S = radam_scalars(step, beta1, beta2)
    live, wd = _per_element(len(p), sg, abi32)
    with np.errstate(all="ignore"):                 # inactive segments hold NaN and 1e30; they are masked out below
        t = _trace64(p, g, m, v, wd, S, lr, beta1, beta2, eps, float(gscale))
    return p, g, m, v, S, live, wd, t, (lr, beta1, beta2, eps)


def radam_step64(p, g, m, v, sg, step, lr, beta1, beta2, eps, gscale=1.0, abi32=True):
    """One RAdam step over flat arrays in fp64 -> (p, m, v).  Everything outside the live elements of active segments
    is returned unchanged.  abi32: lr, betas and eps at their f32 values (what the kernels receive); False: as given
    (the comparison with torch.optim.RAdam)."""
    p, g, m, v, S, live, wd, t, _ = _setup(p, g, m, v, sg, step, lr, beta1, beta2, eps, gscale, abi32)
    return np.where(live, t.p2, p), np.where(live, t.m2, m), np.where(live, t.v2, v)


def allowance(p, g, m, v, sg, step, lr, beta1, beta2, eps, gscale=1.0):
    """Per-element bounds (ap, am, av) on |f32 kernel - radam_step64| for f32 inputs: the module docstring's count,
    evaluated on the reference's intermediates.  Zero outside the live elements of active segments."""
    p, g, m, v, S, live, wd, t, (lr, b1, b2, eps) = _setup(p, g, m, v, sg, step, lr, beta1, beta2, eps, gscale, True)
    A = np.abs
    with np.errstate(all="ignore"):
        e_gr = np.where(wd != 0, U * A(t.wp) + U * (A(t.gr0) + A(t.wp)), 0.0)
        if float(gscale) != 1.0:
            e_gr = e_gr + U * A(t.gr0)
        e_d = e_gr + U * (A(t.gr) + A(m))
        e_m = (1 - b1) * e_d + U * A(t.cd) + U * (A(m) + A(t.cd))
        e_gg = 2 * A(t.gr) * e_gr + U * t.gg
        e_t1 = (1 - b2) * e_gg + U * t.t1
        e_v = e_t1 + U * A(t.t2) + U * (A(t.t2) + t.t1)
        e_mhat = e_m / S.bc1 + 2 * U * A(t.mhat)
        e_x1 = lr * e_mhat + U * A(t.x1)
        if S.rectified:
            e_s = np.where(t.s > 0, e_v / (2 * np.where(t.s > 0, t.s, 1.0)), 0.0) + U * t.s
            e_den = e_s + U * (t.s + eps)
            e_a = t.a * (e_den / t.den + 2 * U)
            e_x2 = t.a * e_x1 + A(t.x1) * e_a + U * A(t.x2)
            e_x = S.rect * e_x2 + 2 * U * A(t.x3)
        else:
            e_x = e_x1
        e_p = e_x + U * (A(p) + A(t.x3))
    z = np.zeros(len(p))
    return np.where(live, e_p, z), np.where(live, e_m, z), np.where(live, e_v, z)


def radam_step32(p, g, m, v, sg, step, lr, beta1, beta2, eps, gscale=1.0, fused=False):
    """radam_one restated in numpy f32, operation by operation as written in csrc/optim.hip.  fused: every a b + c is
    one fma (computed in f64, where an f32 product is exact, and rounded once).  Only here to measure, on the CPU, how
    far honest f32 arithmetic sits from radam_step64."""
    p, g, m, v = (np.asarray(a, F32) for a in (p, g, m, v))
    lr, b1, b2, eps, gs = F32(lr), F32(beta1), F32(beta2), F32(eps), F32(gscale)
    S = radam_scalars(step, float(b1), float(b2))
    bc1, sb, rect = F32(S.bc1), F32(math.sqrt(S.bc2)), F32(S.rect)
    c1, c2 = F32(1) - b1, F32(1) - b2
    live, wd64 = _per_element(len(p), sg)
    wd = wd64.astype(F32)
    D = lambda x: np.asarray(x, np.float64)                              # noqa: E731
    fma = (lambda a, b, c: (D(a) * D(b) + D(c)).astype(F32)) if fused else (lambda a, b, c: (a * b).astype(F32) + c)
    with np.errstate(all="ignore"):
        gr = g if float(gs) == 1.0 else g * gs
        gr = np.where(wd != 0, fma(wd, p, gr), gr)
        d = gr - m
        m2 = fma(np.full_like(d, c1), d, m)
        t1 = c2 * (gr * gr)
        v2 = fma(v, np.full_like(v, b2), t1)
        mhat = m2 / bc1
        if S.rectified:
            a = sb / (np.sqrt(v2) + eps)
            x = (mhat * lr) * a
            p2 = fma(-x, np.full_like(x, rect), p)
        else:
            p2 = fma(-mhat, np.full_like(mhat, lr), p)
    out = [np.where(live, n, o).astype(F32) for n, o in ((p2, p), (m2, m), (v2, v))]
    assert all(o.dtype == F32 for o in out)
    return tuple(out)


# ----------------------------------------------------------------------------------------------- clip norm
def clip64(g, sg, max_norm):
    """(norm, coef): L2 norm of the live gradients of active segments and torch's clip_grad_norm_ coefficient."""
    g = np.asarray(g, np.float64)
    ss = 0.0
    for o, n, _, a in sg:
        if a:
            ss += float(np.dot(g[o:o + n], g[o:o + n]))
    norm = math.sqrt(ss)
    return norm, min(1.0, max_norm / (norm + 1e-6))


def coef32(norm32, max_norm):
    """The kernel's f32 evaluation of the coefficient from the norm it returned."""
    c = F32(max_norm) / (F32(norm32) + F32(1e-6))
    return c if c < F32(1) else F32(1)


def norm_k(total, nt=512):
    """float4s one thread of sumsq_kernel<nt> accumulates in f32 for a buffer of `total` elements."""
    n4 = total // 4
    blocks = min(max((n4 + nt - 1) // nt, 1), NORM_WS)
    stride = blocks * nt
    return (n4 + stride - 1) // stride


def norm_rtol(total, nt=512):
    return (norm_k(total, nt) + 4) * U


# ----------------------------------------------------------------------------------------------- selection
def next_seg(off, nseg, s, e):
    while s + 1 < nseg and off[s + 1] <= e:
        s += 1
    return s


def emulate_selection(L, threads=8, lower_bound=True):
    """Which elements the update / norm kernels take, by their own rule: `threads` threads stride over the float4s,
    each advancing its segment with next_seg from its last one; a float4 at e is taken when e < end[s] (the segment's
    start when inactive); with lower_bound (what this suite made the kernels gain) the threads start at the first
    segment's float4 instead of 0.  Returns
    (taken, seg): a bool per element and the segment each taken element was processed as (-1 = not taken)."""
    off = [int(x) for x in L.off]
    end = [int(o + n) if a else int(o) for o, n, a in zip(L.off, L.len, L.active)]
    taken, seg = np.zeros(L.total, bool), np.full(L.total, -1)
    n4 = L.total // 4
    q_first = (off[0] + 3) // 4 if lower_bound else 0
    for t in range(threads):
        s = 0
        for q in range(q_first + t, n4, threads):
            e = 4 * q
            s = next_seg(off, L.nseg, s, e)
            if e >= end[s]:
                continue
            taken[e:e + 4] = True
            seg[e:e + 4] = s
    return taken, seg


def plan_layout(offs, lens, total):
    """The layout arcweld.optim.RAdam planned (its segment table), as a Layout for emulate_selection."""
    o = np.asarray(offs, np.int64)
    return types.SimpleNamespace(off=o, len=np.asarray(lens, np.int64), wd=np.zeros(len(o), F32),
                                 active=np.ones(len(o), np.int32), total=int(total), nseg=len(o), align=4)


# ----------------------------------------------------------------------------------------------- index maps
def storage_shape(mode, O, I, k):
    """Shape of the source weight in its storage order, per relayout mode (include/arcweld_amd.h)."""
    return {0: (O, I, k), 1: (O, I, 3), 2: (O, I, 3), 3: (I, O, k), 4: (O, 1, k), 5: (O * I,), 7: (O, 3, I)}[mode]


def image_size(mode, O, I, k):
    """How many operand elements a weight maps to, as the header states each mode."""
    return {0: O * I, 1: 3 * O * I, 2: 3 * O * I, 3: k * O * I, 4: O * k, 5: O * I, 7: 3 * O * I}[mode]


def relayout_ref(W, mode, O, I, k=3, tap=0, ldo=0, pad=0):
    """The operand of relayout mode `mode` from the weight W (any dtype, flat or shaped), by transposes, reshapes and
    slices only.  Mode 4's padding columns hold `pad`."""
    W = np.asarray(W).reshape(storage_shape(mode, O, I, k))
    if mode == 0:
        return np.ascontiguousarray(W[:, :, tap])
    if mode == 1:
        return W.transpose(0, 2, 1).reshape(O, 3 * I)
    if mode == 2:
        return W.transpose(2, 0, 1).reshape(3 * O, I)
    if mode == 3:
        return W.transpose(2, 1, 0).reshape(k * O, I)
    if mode == 4:
        out = np.full((O, ldo), pad, W.dtype)
        out[:, :k] = W[:, 0, :]
        return out
    if mode == 5:
        return W.reshape(-1).copy()
    if mode == 7:
        return W.transpose(1, 0, 2).reshape(3 * O, I)
    raise ValueError(mode)


def operand_dst(mode, O, I, k=3, tap=0, ldo=0):
    """For each storage element of the weight, its flat index in the operand, or -1: relayout_ref of an arange."""
    n = int(np.prod(storage_shape(mode, O, I, k)))
    src = relayout_ref(np.arange(n, dtype=np.int64), mode, O, I, k, tap, ldo, pad=-1).reshape(-1)
    dst = np.full(n, -1, np.int64)
    at = np.flatnonzero(src >= 0)
    dst[src[at]] = at
    return dst


def scatter_ref(g, mode, O, I, k=3, tap=0):
    """What aw_weight_grad_scatter adds to the reference-layout gradient G, from the operand-layout gradient g (2-D,
    rows of ldg >= the row length: the columns past the row are ignored)."""
    g = np.asarray(g)
    if mode == 0:
        S = np.zeros((O, I, k), g.dtype)
        S[:, :, tap] = g[:O, :I]
        return S
    if mode == 1:
        return g[:O, :3 * I].reshape(O, 3, I).transpose(0, 2, 1).copy()
    if mode == 3:
        return g[:k * O, :I].reshape(k, O, I).transpose(2, 1, 0).copy()
    if mode == 4:
        return g[:O, :k].reshape(O, 1, k).copy()
    raise ValueError(mode)


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view({2: np.uint16, 4: np.uint32, 8: np.uint64}[a.dtype.itemsize])
