"""Every specialised GEMM epilogue (csrc/gemm_fast_*.hip) and the generic body with a real epilogue against an fp64
restatement of the documented epilogue order (include/arcweld_amd.h, aw_gemm).

CPU part (no marker): the kernels are enumerated from the sources (the EpiBits enum, the five AW_*_CODES lists, the
switch bodies that instantiate them), `args_for` synthesises the one launch epi_code() maps to each code, and
aw_gemm_describe (host only, no device call) must report that layout, code, tile and a specialised kernel for every one
of them, and the generic body for every fallback trigger.

GPU part: each of those kernels is launched once on the smallest shape that has every tile edge (M = 336: full tiles
and an 80-row tail at 128 and 256 rows; N = 192: a 64-column tail; K = 192: three K steps) and every output is
compared with `ref_epilogue` on the device operands upcast to float64: closed-form erf- / tanh-GELU and derivatives,
the dropout masks from the counter hash restated in numpy, BatchNorm column sums.  Bars: f32 outputs rtol
2e-5 sqrt(K / 64), atol 1e-4 (the kernel-level bar of tests/test_gpu_kernels.py); bf16 outputs within one bf16 step
(2^-7 |ref| + 1e-4) AND at most 3 % of the elements different from the reference rounded to bf16 -- an f32 evaluation
of the same epilogue differs on at most 1.2 % at these inputs (1.3 % with the one-exponential erf of the bf16
epilogues), a swapped activation on 17 - 31 %.  A second test runs the generic body with four real epilogues under each
condition that selects it (alpha != 1, N % 4 != 0, misaligned C / pre / resid, ragged K).
"""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from conftest import PKG
from oracle import gen

DEV = "cuda:0"
F32, BF, F64 = torch.float32, torch.bfloat16, torch.float64
CSRC = os.path.join(PKG, "csrc")

M_, N_ = 336, 192
K_OF = {BF: 192, F32: 96}
MOD = 64                     # bias_mod / stats_mod = N / 3
P_DROP = 0.25
SEED1, SEED2 = 0x5EED0001, 0x5EED0002
CTR = 0x1234567              # value of the device step counter in the seed_ptr runs
ATOL = 1e-4                  # _tol's atol x 10, as test_gemm_epilogue_chain uses it
ACT_ERF, ACT_TANH, ACT_DERIV = 0, 1, 2


# ------------------------------------------------------------------ the kernels, read from the sources
def _src(name):
    with open(os.path.join(CSRC, name)) as f:
        return f.read()


def _enum(text, name):
    body = re.search(r"enum\s+%s\b[^{]*\{(.*?)\}" % name, text, re.S).group(1)
    return body


def _parse_bits():
    body = _enum(_src("gemm_core.h"), "EpiBits")
    bits = {n: 1 << int(s) for n, s in re.findall(r"(EP_\w+)\s*=\s*1u\s*<<\s*(\d+)", body)}
    assert len(bits) == len(re.findall(r"EP_\w+\s*=", body)), "an EpiBits entry is not of the form 1u << n"
    return bits


def _parse_layouts():
    body = _enum(_src("gemm_core.h"), "Layout")
    return {n: int(v) for n, v in re.findall(r"(L_\w+)\s*=\s*(\d+)", body)}


EP = _parse_bits()
LY = _parse_layouts()


def _parse_code_lists():
    text = _src("gemm_fast_codes.h").replace("\\\n", " ")
    lists = {}
    for name, body in re.findall(r"^#define\s+(AW_\w+_CODES)\(X, T, LY\)(.*)$", text, re.M):
        codes = []
        for expr in re.findall(r"X\(T, LY,([^)]*)\)", body):
            names = [t.strip() for t in expr.split("|")]
            assert all(n in EP for n in names), (name, expr)
            codes.append(sum(EP[n] for n in set(names)))
        lists[name] = codes
    return lists


CODE_LISTS = _parse_code_lists()


def _parse_instantiations():
    """[(dtype, layout name, tile, list name)] from the switch bodies of the three gemm_fast_*.hip files; every macro
    invocation must sit under the guard (dtype, layout) it instantiates."""
    out = []
    for fname in ("gemm_fast_fwd.hip", "gemm_fast_bwd.hip", "gemm_fast_256.hip"):
        text = _src(fname)
        for m in re.finditer(r"(AW_\w+_CODES)\(AW_FAST_CASE(128|256), (bf16|float), (L_\w+)\)", text):
            lst, tile, ty, ly = m.group(1), int(m.group(2)), m.group(3), m.group(4)
            before = text[:m.start()]
            guard = re.findall(r"(?:ly == |case )(L_\w+)", before)[-1]
            assert guard == ly, f"{fname}: {lst} instantiated for {ly} under the guard {guard}"
            if tile == 128:
                neg = re.findall(r"\((!?)is_bf16 && ly ==", before)[-1]
                assert (neg == "!") == (ty == "float"), f"{fname}: {lst} dtype {ty} under the wrong dtype guard"
            else:
                assert ty == "bf16" and fname == "gemm_fast_256.hip"
            out.append((BF if ty == "bf16" else F32, ly, tile, lst))
    return out


INSTANTIATIONS = _parse_instantiations()


def _bit_names(code):
    return "+".join(n[3:] for n, b in EP.items() if code & b)


class Case:
    def __init__(self, dtype, layout, tile, code, seg=16, seedptr=False):
        self.dtype, self.layout, self.tile, self.code, self.seg, self.seedptr = dtype, layout, tile, code, seg, seedptr
        self.K = K_OF[dtype]

    @property
    def id(self):
        return "%s-%s-t%d-%s%s" % ("bf16" if self.dtype == BF else "f32", self.layout[2:], self.tile,
                                   _bit_names(self.code), "-seg%d" % self.seg if self.seg != 16 else "")


def _kernel_cases():
    cases, seen_drop = [], set()
    for dtype, ly, tile, lst in INSTANTIATIONS:
        for code in CODE_LISTS[lst]:
            # one EP_DROP and one EP_C2DROP kernel per layout (and tile) also run with a device seed counter
            sp = False
            for bit in ("EP_DROP", "EP_C2DROP"):
                if code & EP[bit] and (ly, tile, bit) not in seen_drop:
                    seen_drop.add((ly, tile, bit))
                    sp = True
            cases.append(Case(dtype, ly, tile, code, seedptr=sp))
    return cases


KERNELS = _kernel_cases()
# a window of 24 rows straddles the 128- and the 256-row tile edge: first code of the forward / input-gradient conv lists
SEG24 = [Case(BF, ly, tile, CODE_LISTS[lst][0], seg=24)
         for ly, lst in (("L_NN_CONV", "AW_FWD_CODES"), ("L_NT_CONV", "AW_BWD_CONV_CODES")) for tile in (128, 256)]


# ------------------------------------------------------------------ operands and the launch of a code
class _Dummy:
    """Stands in for a device tensor where only the address, dtype and strides are read (aw_gemm_describe)."""
    is_cuda = True
    _next = [1 << 20]

    def __init__(self, shape, dtype, offset=0, ld=None):
        self.shape, self.dtype, self._ld = tuple(shape), dtype, ld
        self._addr = _Dummy._next[0] + offset * torch.empty(0, dtype=dtype).element_size()
        _Dummy._next[0] += 1 << 20

    def data_ptr(self):
        return self._addr

    def dim(self):
        return len(self.shape)

    def stride(self, i):
        i %= len(self.shape)
        if i == 0 and self._ld is not None:
            return self._ld
        return int(np.prod(self.shape[i + 1:], dtype=np.int64))


def _dummy_alloc(name, shape, dtype, offset=0, ld=None, **_):
    return _Dummy(shape, dtype, offset, ld)


_HOST = {}


def _host(seed, shape, scale=1.0):
    key = (seed, tuple(shape), scale)
    if key not in _HOST:
        _HOST[key] = torch.tensor(gen.normal(seed, shape, scale))
    return _HOST[key]


def _gelu(x, act):
    if act == ACT_TANH:
        u = np.sqrt(2 / np.pi) * (x + 0.044715 * x ** 3)
        return 0.5 * x * (1 + torch.tanh(u))
    return 0.5 * x * (1 + torch.erf(x / np.sqrt(2)))


def _gelu_grad(x, act):
    if act == ACT_TANH:
        u = np.sqrt(2 / np.pi) * (x + 0.044715 * x ** 3)
        t = torch.tanh(u)
        return 0.5 * (1 + t) + 0.5 * x * (1 - t * t) * np.sqrt(2 / np.pi) * (1 + 3 * 0.044715 * x * x)
    return 0.5 * (1 + torch.erf(x / np.sqrt(2))) + x * torch.exp(-0.5 * x * x) / np.sqrt(2 * np.pi)


SEEDS = {"A": 701, "B": 702, "bias": 703, "pre": 704, "resid": 705, "C_old": 706}
# A and pre N(0, 1), the weight-like B N(0, 0.1).  bias and resid N(0, 0.5): the 3 % cap below needs inputs at which
# evaluation precision alone stays well under it.  ref_epilogue run in float32 against float64 (CPU, these inputs)
# differs on at most 1.2 % of a bf16 output (GELU of the dropout-scaled sum; 0.25 % without dropout); with bias and
# resid at scale 1 the wider negative tail of v, where 1 + erf cancels, took that to 2.9 %.
SCALES = {"B": 0.1, "bias": 0.5, "resid": 0.5}


def _make_alloc(device):
    """name -> tensor on `device`: operands from oracle.gen.normal (scale 1; 0.1 for the weight-like B), outputs
    NaN-filled so an element the kernel does not write fails its comparison."""
    def alloc(name, shape, dtype, deriv_of=None, offset=0, ld=None):
        rows = shape[0]
        if name in ("C", "C2"):
            n = int(np.prod(shape))
            buf = torch.full((n + 8,), float("nan"), dtype=dtype, device=device)
            return buf[offset:offset + n].view(shape)
        if name == "colstats":
            return torch.full(shape, 0.5, dtype=F64, device=device)
        if name == "a_rowsum":
            return torch.full(shape, 0.25, dtype=F32, device=device)
        v = _host(SEEDS[name], shape, SCALES.get(name, 1.0))
        if deriv_of is not None:
            v = _gelu_grad(v.double(), deriv_of).float()
        if ld is not None:      # rows padded to ld elements (ragged K with 16-B aligned rows)
            buf = torch.zeros(rows, ld, dtype=dtype, device=device)
            buf[:, :shape[1]] = v.to(dtype)
            return buf[:, :shape[1]]
        if offset:
            buf = torch.zeros(v.numel() + 8, dtype=dtype, device=device)
            buf[offset:offset + v.numel()] = v.reshape(-1).to(dtype)
            return buf[offset:offset + v.numel()].view(shape)
        return v.to(device=device, dtype=dtype)
    return alloc


def launch_for(code, layout, dtype, M, N, K, alloc, seg=16):
    """(A, B, kwargs of arcweld.kernels.gemm): the one launch epi_code() (csrc/gemm.hip) maps to `code`."""
    has = lambda n: bool(code & EP[n])  # noqa: E731
    conv = layout.endswith("_CONV")
    b_trans = layout.startswith("L_NT")
    cin = K // 3
    A = alloc("A", (M, cin if conv else K), dtype)
    B = alloc("B", (K, N) if b_trans else (N, K), dtype)
    kw = dict(b_trans=b_trans)
    if conv:
        kw["conv"] = (cin, seg, -1 if b_trans else 1, 0)
    if has("EP_BIAS"):
        kw["bias"] = alloc("bias", (N,), F32)
    if has("EP_BIASMOD"):
        kw["bias_mod"] = N // 3
    kw["act"] = ACT_DERIV if has("EP_DERIV") else ACT_TANH if has("EP_TANH") else ACT_ERF
    if has("EP_PRE"):
        kw["pre"] = alloc("pre", (M, N), BF if has("EP_PREBF") else F32,
                          deriv_of=ACT_TANH if has("EP_DERIV") else None)
    if has("EP_DROP"):
        kw["drop"] = (P_DROP, SEED1)
    if has("EP_RESID"):
        kw["resid"] = alloc("resid", (M, N), BF if has("EP_RESIDBF") else F32)
    if has("EP_C"):
        kw["C"] = alloc("C", (M, N), BF if has("EP_CBF") else F32)
    mode = 1 if has("EP_C2ACT") else 2 if has("EP_C2COPY") else 3 if has("EP_C2DROP") else 4 if has("EP_C2DACT") else 0
    if mode:
        kw["c2_mode"] = mode
        kw["C2"] = alloc("C2", (M, N), BF if has("EP_C2BF") else F32)
        if mode == 3:
            kw["drop2"] = (P_DROP, SEED2)
    if has("EP_STATS"):
        kw["stats_mod"] = N // 3
        kw["colstats"] = alloc("colstats", (2 * (N // 3),), F64)
    return A, B, kw


def _kernels():
    from arcweld import kernels
    return kernels


def args_for(code, layout, dtype, M, N, K, seg=16):
    """aw_gemm_args of that launch on dummy (non-null, 16-B aligned) addresses: for the host-only query."""
    A, B, kw = launch_for(code, layout, dtype, M, N, K, _dummy_alloc, seg)
    return _kernels()._gemm_args(A, B, M, N, K, **kw)


def describe(a):
    from arcweld import _native as nat
    ly, tile, spec, rag, spl = (ctypes.c_int(-1) for _ in range(5))
    epi = ctypes.c_uint32(0)
    nat.call("aw_gemm_describe", ctypes.byref(a), ctypes.byref(ly), ctypes.byref(epi), ctypes.byref(tile),
             ctypes.byref(spec), ctypes.byref(rag), ctypes.byref(spl))
    return dict(layout=ly.value, epi=epi.value, tile=tile.value, specialised=spec.value, ragged=rag.value,
                splits=spl.value)


class _forced_tile:
    def __init__(self, bm):
        self.bm = bm

    def __enter__(self):
        from arcweld import _native as nat
        nat.call("aw_gemm_set_tile", self.bm)

    def __exit__(self, *exc):
        from arcweld import _native as nat
        nat.call("aw_gemm_set_tile", 0)
        return False


def _expect(case):
    return dict(layout=LY[case.layout], epi=case.code, tile=case.tile, specialised=1, ragged=0, splits=1)


# ------------------------------------------------------------------ CPU: enumeration and dispatch
def test_kernel_enumeration_totals():
    assert sorted(CODE_LISTS) == ["AW_BWD_CONV_CODES", "AW_BWD_PLAIN_CODES", "AW_FWD_CODES", "AW_FWD_F32_CODES",
                                  "AW_FWD_PLAIN_CODES"]
    assert sum(len(v) for v in CODE_LISTS.values()) == 42
    per = {}
    for c in KERNELS:
        per[(c.dtype, c.layout, c.tile)] = per.get((c.dtype, c.layout, c.tile), 0) + 1
    assert per == {(BF, "L_NN", 128): 23, (BF, "L_NN_CONV", 128): 10, (F32, "L_NN", 128): 4, (BF, "L_NT", 128): 15,
                   (BF, "L_NT_CONV", 128): 6, (BF, "L_NN", 256): 23, (BF, "L_NN_CONV", 256): 10,
                   (BF, "L_NT", 256): 15, (BF, "L_NT_CONV", 256): 6}
    assert sum(1 for c in KERNELS if c.tile == 128) == 58 and sum(1 for c in KERNELS if c.tile == 256) == 54
    keys = [(c.dtype, c.layout, c.tile, c.code) for c in KERNELS]
    assert len(set(keys)) == len(keys) == 112
    generic, accum = EP["EP_GENERIC"], EP["EP_ACCUM"]
    assert not any(c.code & (generic | accum | EP["EP_BETA"]) for c in KERNELS)
    # the seed_ptr runs: one EP_DROP kernel per forward layout, one EP_C2DROP kernel per input-gradient layout
    sp = {(c.layout, c.tile) for c in KERNELS if c.seedptr}
    assert sp == {(ly, t) for ly in ("L_NN", "L_NN_CONV", "L_NT", "L_NT_CONV") for t in (128, 256)}


@pytest.mark.parametrize("case", KERNELS + SEG24, ids=lambda c: c.id)
def test_dispatch_reports_the_specialised_kernel(case):
    with _forced_tile(case.tile):
        got = describe(args_for(case.code, case.layout, case.dtype, M_, N_, case.K, case.seg))
    assert got == _expect(case), (got, _bit_names(got["epi"]))


def test_f32_kernels_ignore_the_256_row_tile():
    """The exact-f32 forms exist on the 128-row tile only: forcing 256 rows leaves them where they are."""
    for c in KERNELS:
        if c.dtype == F32:
            with _forced_tile(256):
                assert describe(args_for(c.code, c.layout, c.dtype, M_, N_, c.K)) == _expect(c)


# the generic triggers of the GPU part: name -> (alpha, N, misaligned C / pre / resid, ragged K)
TRIGGERS = {"alpha": dict(alpha=0.5), "n190": dict(N=190), "misaligned": dict(offset=1), "ragged_k": dict(K=100)}
EPILOGUES = ("a", "b", "c", "d")


def generic_launch(epi, trig, dtype, act, alloc):
    """(A, B, M, N, K, kwargs) of epilogue (a) - (d) under one generic trigger.
    (a) bias + pre + drop + resid + C + c2_mode 3     (b) bias + c2_mode 4
    (c) pre with AW_ACT_DERIV (= act' of a normal tensor) + resid
    (d) bias + resid + beta = 1 on a non-zero C + colstats + a_rowsum"""
    t = TRIGGERS[trig]
    N, K, off = t.get("N", N_), t.get("K", K_OF[dtype]), t.get("offset", 0)
    ld = (K + 7) // 8 * 8 if K % 8 else None
    A = alloc("A", (M_, K), dtype, ld=ld)
    B = alloc("B", (N, K), dtype, ld=ld)
    kw = dict(alpha=t.get("alpha", 1.0), act=act)
    odt = dtype                               # outputs / streams follow the operand dtype where the ABI allows
    if epi in "abd":
        kw["bias"] = alloc("bias", (N,), F32)
    if epi == "a":
        kw.update(pre=alloc("pre", (M_, N), odt, offset=off), drop=(P_DROP, SEED1),
                  resid=alloc("resid", (M_, N), odt, offset=off), C=alloc("C", (M_, N), odt, offset=off),
                  C2=alloc("C2", (M_, N), odt), c2_mode=3, drop2=(P_DROP, SEED2))
    elif epi == "b":
        kw.update(C=alloc("C", (M_, N), odt, offset=off), C2=alloc("C2", (M_, N), odt), c2_mode=4)
    elif epi == "c":
        kw.update(pre=alloc("pre", (M_, N), F32, deriv_of=act, offset=off), act=ACT_DERIV,
                  resid=alloc("resid", (M_, N), odt, offset=off), C=alloc("C", (M_, N), F32, offset=off))
    else:
        C = alloc("C", (M_, N), F32, offset=off)
        if not isinstance(C, _Dummy):
            C.copy_(_host(SEEDS["C_old"], (M_, N)))
        kw.update(resid=alloc("resid", (M_, N), odt, offset=off), beta=1.0, C=C,
                  colstats=alloc("colstats", (2 * MOD,), F64), stats_mod=MOD, a_rowsum=alloc("a_rowsum", (M_,), F32))
    return A, B, M_, N, K, kw


def _generic_cases():
    out = []
    for dtype in (F32, BF):
        for trig in TRIGGERS:
            if trig == "ragged_k" and dtype == F32:
                continue       # K = 100 is whole 16-B chunks of f32: not a trigger there
            for tile in ((128, 256) if dtype == BF and trig != "ragged_k" else (128,)):
                for epi in EPILOGUES:
                    for act in (ACT_ERF, ACT_TANH):
                        out.append((dtype, trig, tile, epi, act))
    return out


GENERIC = _generic_cases()


def _gid(c):
    dtype, trig, tile, epi, act = c
    return "%s-%s-t%d-%s-%s" % ("bf16" if dtype == BF else "f32", trig, tile, epi, "tanh" if act else "erf")


@pytest.mark.parametrize("case", GENERIC, ids=_gid)
def test_fallback_triggers_report_the_generic_body(case):
    dtype, trig, tile, epi, act = case
    A, B, M, N, K, kw = generic_launch(epi, trig, dtype, act, _dummy_alloc)
    with _forced_tile(tile):
        got = describe(_kernels()._gemm_args(A, B, M, N, K, **kw))
    want_tile = 256 if tile == 256 and dtype == BF else 128
    assert got == dict(layout=LY["L_NN"], epi=EP["EP_GENERIC"], tile=want_tile, specialised=0,
                       ragged=int(trig == "ragged_k"), splits=1), got


def test_a_rowsum_takes_the_generic_body():
    """The specialised kernels do not compile the fused A-row sums: a launch that asks for them must not reach one."""
    code = EP["EP_BIAS"] | EP["EP_C"]
    for dtype in (F32, BF):
        A, B, kw = launch_for(code, "L_NN", dtype, M_, N_, K_OF[dtype], _dummy_alloc)
        K = _kernels()
        assert describe(K._gemm_args(A, B, M_, N_, K_OF[dtype], **kw))["specialised"] == 1
        got = describe(K._gemm_args(A, B, M_, N_, K_OF[dtype], a_rowsum=_Dummy((M_,), F32), **kw))
        assert got["specialised"] == 0 and got["epi"] == EP["EP_GENERIC"], got


def test_describe_validates_like_the_launch():
    from arcweld import _native as nat
    a = args_for(EP["EP_C"], "L_NN", BF, M_, N_, 192)
    a.c2_mode = 1          # c2_mode without C2: rejected by aw_gemm's argument checks
    with pytest.raises(nat.NativeError, match="c2_mode without C2"):
        describe(a)
    a = args_for(EP["EP_C"], "L_NN", BF, 0, N_, 192)
    assert describe(a) == dict(layout=LY["L_NN"], epi=EP["EP_GENERIC"], tile=0, specialised=0, ragged=0, splits=0)


# ------------------------------------------------------------------ the fp64 reference
def _seed_mix(salt, ctr):
    """aw_seed_mix_value (csrc/common.h), as tests/test_res_chain.py restates it."""
    m = (1 << 64) - 1
    z = (salt ^ ((ctr * 0xD1B54A32D192ED03 + 0x8CB92BA72F3D8DD7) & m)) & m
    z = ((z ^ (z >> 32)) * 0xD6E8FEB86659FD93) & m
    return z ^ (z >> 32)


def keep_mask(M, N, seed, ctr, p):
    """Keep bits of element (r, c) = r * N + c (logical N) under the epilogue's counter hash (common.h
    aw_dropout_scale: splitmix64 of the seed on group e >> 2, 16-bit slice e & 3, dropped iff < round(p * 65536))."""
    s = _seed_mix(seed, ctr) if ctr is not None else seed
    e = np.arange(M * N, dtype=np.uint64)
    with np.errstate(over="ignore"):
        z = np.uint64(s) + (e // np.uint64(4) + np.uint64(1)) * np.uint64(0x9E3779B97F4A7C15)
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        z = z ^ (z >> np.uint64(31))
    u = (z >> (np.uint64(16) * (e & np.uint64(3)))) & np.uint64(0xFFFF)
    return torch.tensor((u >= np.uint64(int(p * 65536 + 0.5))).reshape(M, N))


def _shift_taps(x, S, d):
    """[rows][cin] -> [rows][3 cin]: tap j holds x[r + d (j - 1)] inside each window of S rows (zero across)."""
    n, c = x.shape
    w = x.view(n // S, S, c)
    z = torch.zeros_like(w[:, :1])
    prev = torch.cat([z, w[:, :-1]], 1)
    nxt = torch.cat([w[:, 1:], z], 1)
    return torch.cat([prev, w, nxt] if d > 0 else [nxt, w, prev], 2).view(n, 3 * c)


_ACC = {}


def product(A, B, kw, key=None, dt=F64):
    """op(A) . op(B) in `dt` of the operand values as the device holds them (computed once per operand pair)."""
    if key is not None and (key, dt) in _ACC:
        return _ACC[(key, dt)]
    a, b = A.to("cpu", dt), B.to("cpu", dt)
    if kw.get("conv"):
        a = _shift_taps(a, kw["conv"][1], kw["conv"][2])
    acc = a @ (b if kw.get("b_trans") else b.t())
    if key is not None:
        _ACC[(key, dt)] = acc
    return acc


def ref_epilogue(acc, kw, ctr=None, C_old=None, dt=F64, flip_masks=False):
    """The documented order of include/arcweld_amd.h (aw_gemm): returns dict(C, C2, colstats, v) in `dt` (float64; a
    float32 run of the same code measures what evaluation precision alone does to the bf16 mismatch share)."""
    M, N = acc.shape
    up = lambda t: t.to("cpu", dt)  # noqa: E731
    act = kw.get("act", ACT_ERF)
    v = kw.get("alpha", 1.0) * acc
    if kw.get("bias") is not None:
        c = torch.arange(N)
        v = v + up(kw["bias"])[c % kw["bias_mod"] if kw.get("bias_mod", 0) > 0 else c]
    if kw.get("pre") is not None:
        pre = up(kw["pre"])
        v = v * (pre if act == ACT_DERIV else _gelu_grad(pre, act))
    p, seed = kw.get("drop", (0.0, 0))
    if p > 0:
        keep = keep_mask(M, N, seed, ctr, p) ^ flip_masks
        v = v * keep.to(dt) / (1.0 - p)
    if kw.get("resid") is not None:
        v = v + up(kw["resid"])
    if kw.get("beta", 0.0) != 0.0:
        v = v + kw["beta"] * up(C_old)
    out = dict(v=v, C=v)
    mode = kw.get("c2_mode", 0)
    if mode == 1:
        out["C2"] = _gelu(v, act)
    elif mode == 2:
        out["C2"] = v
    elif mode == 3:
        p2, seed2 = kw.get("drop2", (0.0, 0))
        out["C2"] = v * (keep_mask(M, N, seed2, ctr, p2) ^ flip_masks).to(dt) / (1.0 - p2) if p2 > 0 else v
    elif mode == 4:
        out["C"], out["C2"] = _gelu(v, act), _gelu_grad(v, act)
    sm = kw.get("stats_mod", 0)
    if kw.get("colstats") is not None:
        s = torch.zeros(2 * sm, dtype=dt)
        s[:sm].index_add_(0, torch.arange(N) % sm, v.sum(0))
        s[sm:].index_add_(0, torch.arange(N) % sm, (v * v).sum(0))
        out["colstats"] = s
    return out


# ------------------------------------------------------------------ the bars
SEEN = {}   # bar name -> largest fraction of the bar (or share) any case used, for the next tightening


def _note(name, value):
    SEEN[name] = max(SEEN.get(name, 0.0), float(value))


def check_output(got, ref64, Kd, what, tag):
    got = got.detach().to("cpu")
    assert torch.isfinite(got.float()).all(), f"{what}: non-finite / unwritten elements"
    if got.dtype == F32:
        rtol = 2e-5 * np.sqrt(Kd / 64)
        err = (got.double() - ref64).abs()
        frac = (err / (rtol * ref64.abs() + ATOL)).max().item()
        print(f"{what}: f32 max |err| {err.max().item():.3e}, {frac:.3f} of the bar")
        _note(f"{tag} f32 output, fraction of rtol {rtol:.2e} / atol {ATOL:g}", frac)
        _note(f"{tag} f32 output, max abs error", err.max().item())
        assert frac <= 1.0, f"{what}: {frac:.2f} x the f32 bar"
    else:
        err = (got.double() - ref64).abs()
        frac = (err / (2.0 ** -7 * ref64.abs() + ATOL)).max().item()
        share = (got != ref64.to(BF)).float().mean().item()
        print(f"{what}: bf16 {frac:.3f} of the neighbour bar, {100 * share:.3f} % differ from the rounded reference")
        _note(f"{tag} bf16 output, fraction of 2^-7 |ref| + {ATOL:g}", frac)
        _note(f"{tag} bf16 output, share != round(ref)", share)
        assert frac <= 1.0, f"{what}: {frac:.2f} x the bf16-neighbour bar"
        assert share <= 0.03, f"{what}: {100 * share:.2f} % of the elements are not the rounded reference"


def check_masks(got, kept_ref, flipped_ref, keep, resid, what):
    """The dropped positions are the reference mask's, exactly.  Without a residual a dropped element is a zero; with
    one it is the residual itself, so each element is assigned to the nearer of the reference and the reference under
    the complementary mask, wherever those two are further apart than 8 x the element's bar."""
    got = got.detach().to("cpu").double()
    tol = 2.0 ** -7 * torch.maximum(kept_ref.abs(), flipped_ref.abs()) + ATOL   # the wider (bf16) bar for both dtypes
    if not resid:
        sel = torch.maximum(kept_ref.abs(), flipped_ref.abs()) > ATOL
        assert torch.equal((got == 0)[sel], ~keep[sel]), \
            f"{what}: {int(((got == 0) != ~keep)[sel].sum())} dropped positions differ from the counter hash"
    sel = (kept_ref - flipped_ref).abs() > 8 * tol
    nearer_flipped = (got - flipped_ref).abs() < (got - kept_ref).abs()
    assert sel.float().mean() > 0.25, f"{what}: too few elements tell the two masks apart"
    assert not nearer_flipped[sel].any(), f"{what}: {int(nearer_flipped[sel].sum())} elements carry the wrong mask bit"


def run_and_check(K, A, B, M, N, Kd, kw, what, tag, acc_key=None, ctr=None):
    """One launch of K.gemm and every output against ref_epilogue; returns the outputs."""
    C_old = kw["C"].detach().to("cpu", copy=True) if kw.get("beta", 0.0) != 0.0 else None
    stats0 = kw["colstats"].detach().to("cpu", copy=True) if kw.get("colstats") is not None else None
    rows0 = kw["a_rowsum"].detach().to("cpu", copy=True) if kw.get("a_rowsum") is not None else None
    extra = {}
    if ctr is not None:
        extra["seed_ptr"] = torch.tensor([ctr], dtype=torch.int64, device=DEV)
    K.gemm(A, B, M, N, Kd, **kw, **extra)
    torch.cuda.synchronize()
    acc = product(A, B, kw, acc_key)
    ref = ref_epilogue(acc, kw, ctr=ctr, C_old=C_old)
    for name in ("C", "C2"):
        if kw.get(name) is not None:
            check_output(kw[name], ref[name], Kd, f"{what} {name}", tag)
    p, seed = kw.get("drop", (0.0, 0))
    p2, seed2 = kw.get("drop2", (0.0, 0))
    if p > 0 or (kw.get("c2_mode") == 3 and p2 > 0):
        flipped = ref_epilogue(acc, kw, ctr=ctr, C_old=C_old, flip_masks=True)
        if p > 0 and kw.get("C") is not None:
            check_masks(kw["C"], ref["C"], flipped["C"], keep_mask(M, N, seed, ctr, p),
                        kw.get("resid") is not None or kw.get("beta", 0.0) != 0.0, f"{what} C")
        if kw.get("c2_mode") == 3 and p2 > 0 and p <= 0:
            check_masks(kw["C2"], ref["C2"], flipped["C2"], keep_mask(M, N, seed2, ctr, p2), False, f"{what} C2")
        elif kw.get("c2_mode") == 3 and p2 > 0:
            # C2 = v * mask2 with v already masked: its zeros are exactly the elements mask2 drops or v is zero at
            k2 = keep_mask(M, N, seed2, ctr, p2)
            sel = ref["v"].abs() > ATOL
            assert torch.equal((kw["C2"].detach().to("cpu").float() == 0)[sel], ~k2[sel]), f"{what} C2: mask"
    if stats0 is not None:
        got = kw["colstats"].detach().to("cpu")
        want = stats0 + ref["colstats"]
        err = (got - want).abs()
        frac = (err / (2e-5 * want.abs() + 1e-3)).max().item()
        print(f"{what} colstats: {frac:.3f} of the bar")
        _note(f"{tag} colstats, fraction of rtol 2e-5 / atol 1e-3", frac)
        assert frac <= 1.0, f"{what} colstats: {frac:.2f} x the bar"
    if rows0 is not None:
        got = kw["a_rowsum"].detach().to("cpu").double()
        want = rows0.double() + A.detach().to("cpu", F64).sum(1)
        err = (got - want).abs()
        frac = (err / (1e-5 * want.abs() + 1e-4)).max().item()
        print(f"{what} a_rowsum: {frac:.3f} of the bar")
        _note(f"{tag} a_rowsum, fraction of rtol 1e-5 / atol 1e-4", frac)
        assert frac <= 1.0, f"{what} a_rowsum: {frac:.2f} x the bar"
    return ref


# ------------------------------------------------------------------ GPU
@pytest.fixture(scope="module")
def K():
    yield _kernels()
    for name in sorted(SEEN):
        print(f"[gemm epilogue bars] {name}: {SEEN[name]:.4g}")


_DEV = {}


def _dev_alloc(name, shape, dtype, **kw):
    """Device operands, the inputs made once per (name, shape, dtype, form) and shared by the cases (read-only)."""
    if name in ("C", "C2", "colstats", "a_rowsum"):
        return _make_alloc(DEV)(name, shape, dtype, **kw)
    key = (name, tuple(shape), dtype, tuple(sorted(kw.items())))
    if key not in _DEV:
        _DEV[key] = _make_alloc(DEV)(name, shape, dtype, **kw)
    return _DEV[key]


@pytest.mark.gpu
@pytest.mark.parametrize("case", KERNELS + SEG24, ids=lambda c: c.id)
def test_specialised_epilogue_vs_fp64(K, case):
    M, N, Kd = M_, N_, case.K
    A, B, kw = launch_for(case.code, case.layout, case.dtype, M, N, Kd, _dev_alloc, case.seg)
    tag = "bf16 operands" if case.dtype == BF else "f32 operands"
    key = (case.dtype, case.layout, case.seg)
    with _forced_tile(case.tile):
        got = describe(K._gemm_args(A, B, M, N, Kd, **kw))
        assert got == _expect(case), (got, _bit_names(got["epi"]))
        run_and_check(K, A, B, M, N, Kd, kw, case.id, tag, acc_key=key)
        if case.seedptr:
            _, _, kw2 = launch_for(case.code, case.layout, case.dtype, M, N, Kd, _dev_alloc, case.seg)
            run_and_check(K, A, B, M, N, Kd, kw2, case.id + " seed_ptr", tag, acc_key=key, ctr=CTR)


@pytest.mark.gpu
@pytest.mark.parametrize("case", GENERIC, ids=_gid)
def test_generic_body_with_a_real_epilogue_vs_fp64(K, case):
    dtype, trig, tile, epi, act = case
    A, B, M, N, Kd, kw = generic_launch(epi, trig, dtype, act, _dev_alloc)
    tag = ("bf16" if dtype == BF else "f32") + " operands, generic body"
    with _forced_tile(tile):
        got = describe(K._gemm_args(A, B, M, N, Kd, **kw))
        assert got["specialised"] == 0 and got["epi"] == EP["EP_GENERIC"], got
        assert got["tile"] == (256 if tile == 256 else 128) and got["ragged"] == int(trig == "ragged_k")
        key = (dtype, trig) if trig in ("n190", "ragged_k") else (dtype, "L_NN", 16)   # the main test's operands
        run_and_check(K, A, B, M, N, Kd, kw, _gid(case), tag, acc_key=key)
        if epi == "c":
            # the same product through act' of the saved pre-activation: AW_ACT_DERIV with pre = GELU'(h) against
            # act = GELU with pre = h must agree within the f32 bar (h f32; GELU'(h) rounded to f32 once)
            off = TRIGGERS[trig].get("offset", 0)
            kw2 = dict(kw, act=act, pre=_dev_alloc("pre", (M, N), F32, offset=off),
                       C=_dev_alloc("C", (M, N), F32, offset=off))
            assert describe(K._gemm_args(A, B, M, N, Kd, **kw2))["specialised"] == 0
            K.gemm(A, B, M, N, Kd, **kw2)
            rtol = 2e-5 * np.sqrt(Kd / 64)
            torch.testing.assert_close(kw2["C"], kw["C"], rtol=rtol, atol=ATOL)


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", [F32, BF], ids=["f32", "bf16"])
def test_a_rowsum_beside_a_specialisable_epilogue(K, dtype):
    """bias + C is a specialised code; with a_rowsum the launch must still produce the row sums (generic body)."""
    Kd = K_OF[dtype]
    A, B, kw = launch_for(EP["EP_BIAS"] | EP["EP_C"], "L_NN", dtype, M_, N_, Kd, _dev_alloc)
    kw["a_rowsum"] = _dev_alloc("a_rowsum", (M_,), F32)
    run_and_check(K, A, B, M_, N_, Kd, kw, "bias + C + a_rowsum", "a_rowsum", acc_key=(dtype, "L_NN", 16))
