"""The forward boundaries of the chain launches (csrc/reschain.hip res_chain_fwd_kernel<.., TAIL, HEAD>) against the
launches they replace:
  * the sep conv (H -> D = 64, one tap per token) as the tail of the encoder chain (aw_res_chain_fwd_args.sep_*;
    model/vq_vae_patch_embedd.py SepCNNBlock) against K.gemm(x_R, Ws, N, D, H, bias=...);
  * the decoder's 1x1 conv (64 -> H) as the head of the decoder chain, and patchify + the patch embed (32 -> H) as the
    head of the encoder chain (aw_res_chain_fwd_args.head_*) against K.patchify / K.gemm(..., c2_mode=1).

Shapes: the smallest at which they can go wrong -- one full 64-token workgroup (N = 64), a ragged lone one (N = 16: 48
zero rows in the image, whose z / patches must not be written), a full one plus a ragged one (N = 80); R = 1 and 2
(both image parities: the tail's image is the one the last conv2 epilogue staged x_R in); dropout 0.1 and 0 (two
kernel instantiations).  The decoder head cases run with the ConvT tail (k1 = 5), the encoder head cases with the sep
tail.  Outputs are pre-filled with NaN; z and patches have guard rows past N, which must stay NaN.

Bars.  x_0, a_0 = GELU(x_0) against the fp64 reference on the same bf16 operands: 2^-7 |ref| + 1e-4 (one bf16 step, the
bar of tests/test_chain_convt.py), and at most 1 % of the elements off the bf16-rounded reference (a CPU emulation of
32-deep f32 accumulation flips 0 / 2.4e-5 / 1.5e-4 of them); against the launches: bit-equal, patches included.  z
against the fp64 reference on the chain's own stored x_R: 2^-15 (sum_k |x_k||w_k| + |b|), the forward bound of summing
K = 512 exact bf16 products in f32, (K - 1) 2^-24 <= 2^-15; against the GEMM launch: bit-equal (one flipped z would
move a codebook index).  Whole step, switches on against off: loss, x_hat, indices and perplexity equal; every
parameter gradient within 1e-5 relative Frobenius -- the forward's saved tensors are bit-equal, so only the order of
the backward's f32 atomic adds differs, sqrt(16384) 2^-24 ~ 8e-6 per element; the off-against-off figure of the same
run is printed beside it.

Figures measured on an MI355X (one run of this file; the printed lines give them again):
  x_0 / a_0 / patches / z and every chain output: bit-equal to the launches in all cases; x_0 and a_0 at most 0.491 of
  one bf16 step from the fp64 reference, at most 0.0049 % / 0.0122 % of the elements off the rounded reference; z at
  most 0.0023 of its bar; whole step on / off: loss, x_hat, indices, perplexity equal, largest gradient relative
  Frobenius difference 9.1e-8 (off against off: 8.8e-8).
"""
import itertools

import pytest
import torch

pytestmark = pytest.mark.gpu

H, D = 512, 64
GUARD = 8
BF = torch.bfloat16
F64 = torch.float64
CASES = list(itertools.product([64, 16, 80], [1, 2], [0.1, 0.0]))
# The un-patch ConvT's bias feeds a train-mode BatchNorm: its gradient is analytically zero, what is stored is the
# rounding noise of sums that cancel, and a difference relative to it says nothing (two runs of the same launches
# differ by 4e-4 of it).  It is held to an absolute bar instead, as tests/test_chain_convt.py holds it.
ZERO_GRAD = "reverse_patch_embed.proj.0.bias"


def _rand(shape, seed, scale=1.0, dtype=BF, shift=0.0):
    g = torch.Generator(device="cpu").manual_seed(seed)
    return (torch.randn(*shape, generator=g) * scale + shift).to(dtype).cuda()


def _run(K, N, R, p, sep):
    """One encoder chain launch on seeded bf16 operands, with or without the sep tail.  Returns every output."""
    x0, a0 = _rand((N, H), 11), _rand((N, H), 12)
    w = [_rand((H, H), 100 + r, H ** -0.5) for r in range(2 * R)]
    b = [_rand((H,), 200 + r, 0.1, torch.float32) for r in range(2 * R)]
    Ws = _rand((D, H), 300, H ** -0.5)
    sb = _rand((D,), 301, 0.5, torch.float32, shift=1.0)
    seeds = [0x4321 + 77 * r for r in range(R)]
    ctr = torch.tensor([5], device="cuda", dtype=torch.int64)
    e = lambda: torch.full((N, H), float("nan"), device="cuda", dtype=BF)  # noqa: E731
    dh, a1, a = [e() for _ in range(R)], [e() for _ in range(R)], [e() for _ in range(R)]
    dx = [e() if r < R - 1 else None for r in range(R)]
    pk = [torch.empty(H, H, device="cuda", dtype=BF) for _ in w]
    out = dict(Ws=Ws, sb=sb, dh=dh, a1=a1, dx=dx, a=a)
    masks = K.res_dropout_masks_empty(N, R, "cuda") if p > 0 else None
    K.res_pack_weights(w, pk, None, taps=1)
    ks = None
    if sep:
        out["zbuf"] = torch.full((N + GUARD, D), float("nan"), device="cuda", dtype=torch.float32)
        ks = (Ws, sb, out["zbuf"][:N])
    K.res_chain_fwd(a0, x0, pk[0::2], pk[1::2], b[0::2], b[1::2], dh, a1, dx, a, drop=(p, seeds), seed_ptr=ctr,
                    masks=masks, taps=1, sep=ks)
    torch.cuda.synchronize()
    out["masks"] = masks
    return out


_cache = {}


def _runs(N, R, p):
    """The two launches of a case, run once and shared by the tests (never modified)."""
    from arcweld import kernels as K
    key = (N, R, p)
    if key not in _cache:
        _cache.clear()         # the tests of one case run back to back: keep one case alive
        _cache[key] = (_run(K, N, R, p, False), _run(K, N, R, p, True))
    return _cache[key]


@pytest.mark.parametrize("N,R,p", CASES)
def test_chain_outputs_unchanged_by_the_sep_tail(N, R, p):
    plain, sep = _runs(N, R, p)
    for name in ("a1", "a", "dh", "dx"):
        for r, (g, w) in enumerate(zip(sep[name], plain[name])):
            if w is not None:
                assert not bool(torch.isnan(w.float()).any()), f"{name}[{r}] not fully written"
                assert torch.equal(g.view(torch.int16), w.view(torch.int16)), f"{name}[{r}]"
    if p > 0:
        assert torch.equal(sep["masks"], plain["masks"])


@pytest.mark.parametrize("N,R,p", CASES)
def test_sep_z_matches_gemm_and_fp64_reference(N, R, p):
    from arcweld import kernels as K
    _, t = _runs(N, R, p)
    z, xR = t["zbuf"][:N], t["a"][-1]
    assert bool(torch.isnan(t["zbuf"][N:]).all()), "rows at or past N were written"
    assert not bool(torch.isnan(z).any()), "z not fully written"
    zg = torch.full((N, D), float("nan"), device="cuda", dtype=torch.float32)
    K.gemm(xR, t["Ws"], N, D, H, bias=t["sb"], C=zg)
    torch.cuda.synchronize()
    ndiff = int((z.view(torch.int32) != zg.view(torch.int32)).sum())
    x64, w64, b64 = xR.to(F64), t["Ws"].to(F64), t["sb"].to(F64)
    ref = x64 @ w64.t() + b64
    bar = 2.0 ** -15 * (x64.abs() @ w64.abs().t() + b64.abs())
    frac = float(((z.to(F64) - ref).abs() / bar).max())
    print(f"N {N} R {R} p {p}: z {frac:.4f} of the bar, {ndiff} of {z.numel()} elements differ from the GEMM launch")
    assert ndiff == 0, f"z: {ndiff} elements differ from the GEMM launch"
    assert frac <= 1.0, f"z: {frac:.3f} x the bar"


def test_sep_argument_checks():
    from arcweld import _native
    from arcweld import kernels as K
    N, R = 16, 1
    z = lambda *s, dt=BF: torch.zeros(*s, device="cuda", dtype=dt)  # noqa: E731
    args = lambda taps: ([z(N, H), z(N, H)] + [[z(H, taps * H)] for _ in range(2)]             # noqa: E731
                         + [[z(H, dt=torch.float32)] for _ in range(2)] + [[z(N, H)] for _ in range(4)])
    sep = (z(D, H), z(D, dt=torch.float32), z(N, D, dt=torch.float32))
    with pytest.raises(_native.NativeError):      # the decoder chain has no sep tail
        K.res_chain_fwd(*args(3), taps=3, sep=sep)
    with pytest.raises(_native.NativeError):      # z of the wrong width
        K.res_chain_fwd(*args(1), taps=1, sep=(sep[0], sep[1], z(N, 2 * D, dt=torch.float32)))
    with pytest.raises(_native.NativeError):      # a 256-wide codebook keeps its launch
        K.res_chain_fwd(*args(1), taps=1, sep=(z(256, H), z(256, dt=torch.float32), z(N, 256, dt=torch.float32)))


def _run_head(K, kind, N, R, p, head):
    """One chain launch whose x_0 comes from a conv on seeded operands -- kind "dec": the 1x1 conv (64 -> H) on zq, ahead
    of the decoder chain with the ConvT tail (k1 = 5); kind "enc": patchify + the patch embed (32 -> H) on f32 windows
    of 200 x 2, ahead of the encoder chain with the sep tail.  head False: the conv as its launches (K.patchify,
    K.gemm with c2_mode 1), head True: inside the chain launch.  Returns every output."""
    taps, k1 = (3, 5) if kind == "dec" else (1, 0)
    w = [_rand((H, taps * H), 100 + r, (taps * H) ** -0.5) for r in range(2 * R)]
    b = [_rand((H,), 200 + r, 0.1, torch.float32) for r in range(2 * R)]
    hb = _rand((H,), 401, 0.3, torch.float32)
    seeds = [0x2468 + 77 * r for r in range(R)]
    ctr = torch.tensor([5], device="cuda", dtype=torch.int64)
    e = lambda *s, dt=BF: torch.full(s or (N, H), float("nan"), device="cuda", dtype=dt)  # noqa: E731
    dh, a1, a = [e() for _ in range(R)], [e() for _ in range(R)], [e() for _ in range(R)]
    dx = [e() if r < R - 1 else None for r in range(R)]
    x0, a0 = e(), e()
    pk = [torch.empty(H, taps * H, device="cuda", dtype=BF) for _ in w]
    masks = K.res_dropout_masks_empty(N, R, "cuda") if p > 0 else None
    out = dict(dh=dh, a1=a1, dx=dx, a=a, x0=x0, a0=a0, masks=masks, hb=hb)
    kw = {}
    if kind == "dec":
        hin, hw = _rand((N, 64), 402), _rand((H, 64), 403, 0.125)
        Wt, tb = _rand((k1 * H, H), 300, 0.04), _rand((H,), 301, 0.5, torch.float32, shift=1.0)
        tpk = [torch.empty(H, H, device="cuda", dtype=BF) for _ in range(k1)]
        K.res_pack_weights(w + [Wt[j * H:(j + 1) * H] for j in range(k1)], pk + tpk, None, taps=3,
                           job_taps=[3] * len(w) + [1] * k1)
        out["Y"], out["stats"] = e(N, k1 * H), torch.zeros(2 * H, device="cuda", dtype=F64)
        kw["tail"] = (tpk, tb, out["Y"], out["stats"])
        hd = (hin, hw, hb)
        out["in64"] = hin.to(F64)
    else:
        g = torch.Generator(device="cpu").manual_seed(402)
        hin, hw = torch.randn(N // 16, 200, 2, generator=g).cuda(), _rand((H, 32), 403, 0.2)
        K.res_pack_weights(w, pk, None, taps=1)
        out["zbuf"] = e(N + GUARD, D, dt=torch.float32)
        kw["sep"] = (_rand((D, H), 300, H ** -0.5), _rand((D,), 301, 0.5, torch.float32, shift=1.0), out["zbuf"][:N])
        out["pbuf"] = e(N + GUARD, 32)
        hd = (hin, hw, hb, out["pbuf"][:N], 25)
        # token t of window b, element j < 25: the window's channel-major flat element 25 t + j
        out["in64"] = torch.zeros(N, 32, dtype=F64, device="cuda")
        out["in64"][:, :25] = hin.permute(0, 2, 1).reshape(N // 16, 16, 25).reshape(N, 25).to(BF).to(F64)
    out["hw"] = hw
    if not head:
        if kind == "enc":
            K.patchify(hin, 25, out["pbuf"][:N])
        K.gemm(out["pbuf"][:N] if kind == "enc" else hin, hw, N, H, hw.shape[1], bias=hb, C=x0, C2=a0, c2_mode=1)
    K.res_chain_fwd(a0, x0, pk[0::2], pk[1::2], b[0::2], b[1::2], dh, a1, dx, a, drop=(p, seeds), seed_ptr=ctr,
                    masks=masks, taps=taps, head=hd if head else None, **kw)
    torch.cuda.synchronize()
    return out


def _head_runs(kind, N, R, p):
    from arcweld import kernels as K
    key = (kind, N, R, p)
    if key not in _cache:
        _cache.clear()
        _cache[key] = (_run_head(K, kind, N, R, p, False), _run_head(K, kind, N, R, p, True))
    return _cache[key]


def _bits(t):
    return t.view(torch.int16 if t.dtype == BF else torch.int32 if t.dtype == torch.float32 else torch.int64)


@pytest.mark.parametrize("N,R,p", CASES)
@pytest.mark.parametrize("kind", ["dec", "enc"])
def test_chain_outputs_unchanged_by_the_head(kind, N, R, p):
    plain, head = _head_runs(kind, N, R, p)
    names = ("a1", "a", "dh", "dx") + (("Y", "stats") if kind == "dec" else ("zbuf",))
    for name in names:
        gs, ws = (head[name], plain[name]) if isinstance(head[name], list) else ([head[name]], [plain[name]])
        for r, (g, w) in enumerate(zip(gs, ws)):
            if w is not None:
                assert torch.equal(_bits(g), _bits(w)), f"{name}[{r}]"
    assert not bool(torch.isnan(head["a"][-1].float()).any())
    if p > 0:
        assert torch.equal(head["masks"], plain["masks"])


@pytest.mark.parametrize("N,R,p", CASES)
@pytest.mark.parametrize("kind", ["dec", "enc"])
def test_head_outputs_match_gemm_and_fp64_reference(kind, N, R, p):
    plain, head = _head_runs(kind, N, R, p)
    if kind == "enc":
        assert torch.equal(_bits(head["pbuf"][:N]), _bits(plain["pbuf"][:N])), "patches differ from K.patchify"
        assert bool(torch.isnan(head["pbuf"][N:].float()).all()), "patches rows at or past N were written"
        assert torch.equal(head["pbuf"][:N].to(F64), head["in64"]), "patches differ from the windows' elements"
    v = head["in64"] @ head["hw"].to(F64).t() + head["hb"].to(F64)
    refs = dict(x0=v, a0=0.5 * v * (1.0 + torch.erf(v * 0.5 ** 0.5)))
    line = []
    for name, ref in refs.items():
        got = head[name]
        ndiff = int((_bits(got) != _bits(plain[name])).sum())
        frac = float(((got.to(F64) - ref).abs() / (2.0 ** -7 * ref.abs() + 1e-4)).max())
        flips = float((_bits(got) != _bits(ref.to(torch.float32).to(BF))).float().mean())
        line.append(f"{name} {frac:.3f} of one bf16 step, {100 * flips:.4f} % off bf16(ref), {ndiff} differ from the GEMM")
        assert ndiff == 0, f"{name}: {ndiff} elements differ from the GEMM launch"
        assert frac <= 1.0, f"{name}: {frac:.2f} x one bf16 step"
        assert flips <= 0.01, f"{name}: {100 * flips:.2f} % of the elements differ from the rounded reference"
    print(f"{kind} N {N} R {R} p {p}: " + "; ".join(line))


def test_head_argument_checks():
    from arcweld import _native
    from arcweld import kernels as K
    N, R = 16, 1
    z = lambda *s, dt=BF: torch.zeros(*s, device="cuda", dtype=dt)  # noqa: E731
    args = lambda taps: ([z(N, H), z(N, H)] + [[z(H, taps * H)] for _ in range(2)]             # noqa: E731
                         + [[z(H, dt=torch.float32)] for _ in range(2)] + [[z(N, H)] for _ in range(4)])
    with pytest.raises(_native.NativeError):      # the decoder head's weights are (H, 64)
        K.res_chain_fwd(*args(3), taps=3, head=(z(N, 64), z(H, 32), z(H, dt=torch.float32)))
    with pytest.raises(_native.NativeError):      # a 256-wide code keeps its launch
        K.res_chain_fwd(*args(3), taps=3, head=(z(N, 256), z(H, 256), z(H, dt=torch.float32)))
    with pytest.raises(_native.NativeError):      # windows that do not make N patches
        K.res_chain_fwd(*args(1), taps=1, head=(z(2, 200, 2, dt=torch.float32), z(H, 32), z(H, dt=torch.float32), None, 25))
    with pytest.raises(_native.NativeError):      # a patch wider than the 32 padded columns
        K.res_chain_fwd(*args(1), taps=1, head=(z(1, 320, 2, dt=torch.float32), z(H, 32), z(H, dt=torch.float32), None, 40))
    with pytest.raises(_native.NativeError):      # no head: a0 / x0 are inputs
        K.res_chain_fwd(None, None, *args(1)[2:], taps=1)


def _step(monkeypatch, sd, x, kw, mode):
    """One fused_train_step from the seeded state with both switches set to `mode`; returns (loss, x_hat, indices,
    perplexity, gradients, the sep= / head= arguments the chain launches saw)."""
    import model.vq_vae_patch_embedd as mod

    from arcweld import kernels as K
    from arcweld.precision import operands

    monkeypatch.setenv("ARCWELD_SEP_TAIL", mode)
    monkeypatch.setenv("ARCWELD_CHAIN_HEAD", mode)
    seen, fw = [], []
    real, real_fw = K.res_chain_fwd, mod.engine.forward
    monkeypatch.setattr(K, "res_chain_fwd", lambda *a, **k: (seen.append((k.get("sep") is not None, k.get("head") is not None)), real(*a, **k))[1])
    monkeypatch.setattr(mod.engine, "forward", lambda *a, **k: (fw.append(real_fw(*a, **k)), fw[-1])[1])
    m = mod.VQVAEPatch(input_dim=2, learning_rate=1e-3, dropout_p=0.1, batch_norm=False, **kw)
    m.load_state_dict({k: torch.tensor(v) for k, v in sd.items()})
    m = m.cuda().train()
    with operands(torch.bfloat16):
        loss = m.fused_train_step(x, 1.0)
    torch.cuda.synchronize()
    monkeypatch.setattr(K, "res_chain_fwd", real)
    monkeypatch.setattr(mod.engine, "forward", real_fw)
    _, x_hat, perp, idx, _ = fw[0]
    return (loss.clone(), x_hat.clone(), idx.clone(), perp.clone(),
            {n: p.grad.detach().clone() for n, p in m.named_parameters()}, seen)


def test_whole_step_with_and_without_the_fused_boundaries(monkeypatch):
    """fused_train_step at B = 8 windows (N = 128), bf16, R = 2, dropout 0.1, from the same seeded state with
    ARCWELD_SEP_TAIL / ARCWELD_CHAIN_HEAD on and off."""
    from oracle import gen
    from oracle import vqvae as ov

    kw = dict(hidden_dim=512, num_embeddings=512, embedding_dim=64, n_resblocks=2, patch_size=25)
    sd = ov.det_state_dict(ov.VQVAEConfig(**kw), 41)
    x = torch.tensor(gen.windows(42, 8), device="cuda")
    off, off2, on = (_step(monkeypatch, sd, x, kw, mode) for mode in ("0", "0", "1"))
    # (sep tail, head) of the encoder chain and of the decoder chain
    assert off[5] == [(False, False), (False, False)] and on[5] == [(True, True), (False, True)]
    for name, a, b in zip(("loss", "x_hat", "indices", "perplexity"), on, off):
        assert torch.equal(a, b), name

    def worst(g0, g1):
        w, who = 0.0, ""
        for n, a in g0.items():
            if n == ZERO_GRAD:      # analytically zero: both runs hold summation noise only
                assert a.abs().max().item() < 1e-5 and g1[n].abs().max().item() < 1e-5, n
                continue
            if a.norm() == 0:
                assert g1[n].norm() == 0, n
                continue
            rel = float((a - g1[n]).norm() / a.norm())
            if rel > w:
                w, who = rel, n
        return w, who

    (w_on, n_on), (w_off, n_off) = worst(off[4], on[4]), worst(off[4], off2[4])
    print(f"whole step switches on / off: loss {on[0].item():.9g} / {off[0].item():.9g}, largest gradient relative "
          f"Frobenius difference {w_on:.3g} ({n_on}; off against off: {w_off:.3g}, {n_off})")
    assert w_on <= 1e-5, f"gradients: {w_on:.3g} ({n_on})"
