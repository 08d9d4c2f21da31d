"""The un-patch ConvTranspose1d(H -> H, kernel = stride = k1) as the tail of the decoder chain launch
(csrc/reschain.hip res_chain_fwd_kernel<3, .., TAIL>, aw_res_chain_fwd_args.tail_*; model/vq_vae_patch_embedd.py:
reverse_patch_embed.proj[0]) against the launch it replaces, K.gemm(x_R, Wt1, bias_mod=H, colstats, stats_mod=H).

Shapes: the smallest at which the tail can go wrong -- one full 64-token workgroup (N = 64), a ragged lone one
(N = 16: 48 zero rows in the image, whose v = bias must enter neither Y nor the sums), a full one plus a ragged one
(N = 80); R = 1 and 2 (the tail's image is the one the last conv2 epilogue staged x_R in, either parity of the slice
counters); k1 = 5 (patch 25) and 2 (patch 10); dropout 0.1 and 0 (two kernel instantiations); colstats given and NULL.

Figures measured on an MI355X (one run of this file; the printed lines give them again):
  Y vs the GEMM launch: bit-equal in all 24 cases; Y vs the fp64 reference: at most 0.496 of one bf16 step, at most
  0.0092 % of the elements differ from the rounded reference (the cap is 1 %); colstats at most 0.0067 of the bar;
  whole step tail on / off: loss relative difference 0, largest gradient relative Frobenius difference 1.1e-7 (Y
  bit-equal; both launches sum the statistics in f64, so they differ in f64 rounding only).
"""
import itertools

import pytest
import torch

pytestmark = pytest.mark.gpu

H = 512
BF = torch.bfloat16
F64 = torch.float64
CASES = list(itertools.product([64, 16, 80], [1, 2], [5, 2], [0.1, 0.0]))


def _rand(shape, seed, scale=1.0, dtype=BF, shift=0.0):
    g = torch.Generator(device="cpu").manual_seed(seed)
    return (torch.randn(*shape, generator=g) * scale + shift).to(dtype).cuda()


def _run(K, N, R, k1, p, tail, stats):
    """One chain launch on seeded bf16 operands; tail: with the ConvT tail (stats: onto a non-zero colstats start
    value, else NULL).  Returns every output."""
    x0, a0 = _rand((N, H), 11), _rand((N, H), 12)
    sc = (3 * H) ** -0.5
    w = [_rand((H, 3 * H), 100 + r, sc) for r in range(2 * R)]
    b = [_rand((H,), 200 + r, 0.1, torch.float32) for r in range(2 * R)]
    Wt = _rand((k1 * H, H), 300, 0.04)
    tb = _rand((H,), 301, 0.5, torch.float32, shift=1.0)     # order 1: counted padded rows would show in the sums
    seeds = [0x1234 + 77 * r for r in range(R)]
    ctr = torch.tensor([5], device="cuda", dtype=torch.int64)
    e = lambda: torch.full((N, H), float("nan"), device="cuda", dtype=BF)  # noqa: E731
    dh, a1, a = [e() for _ in range(R)], [e() for _ in range(R)], [e() for _ in range(R)]
    dx = [e() if r < R - 1 else None for r in range(R)]
    pk = [torch.empty(H, 3 * H, device="cuda", dtype=BF) for _ in w]
    out = dict(Wt=Wt, tb=tb, dh=dh, a1=a1, dx=dx, a=a)
    masks = K.res_dropout_masks_empty(N, R, "cuda") if p > 0 else None
    kt = None
    if tail:
        tpk = [torch.empty(H, H, device="cuda", dtype=BF) for _ in range(k1)]
        K.res_pack_weights(w + [Wt[j * H:(j + 1) * H] for j in range(k1)], pk + tpk, None, taps=3,
                           job_taps=[3] * len(w) + [1] * k1)
        out["Y"] = torch.full((N, k1 * H), float("nan"), device="cuda", dtype=BF)
        out["stats0"] = _rand((2 * H,), 302, 3.0, F64)
        out["stats"] = out["stats0"].clone() if stats else None
        kt = (tpk, tb, out["Y"], out["stats"])
    else:
        K.res_pack_weights(w, pk, None, taps=3)
    K.res_chain_fwd(a0, x0, pk[0::2], pk[1::2], b[0::2], b[1::2], dh, a1, dx, a, drop=(p, seeds), seed_ptr=ctr,
                    masks=masks, taps=3, tail=kt)
    torch.cuda.synchronize()
    out["masks"] = masks
    return out


_cache = {}


def _runs(N, R, k1, p):
    """The three launches of a case, run once and shared by the tests (never modified)."""
    from arcweld import kernels as K
    key = (N, R, k1, p)
    if key not in _cache:
        _cache.clear()         # the tests of one case run back to back: keep one case alive
        _cache[key] = (_run(K, N, R, k1, p, False, False), _run(K, N, R, k1, p, True, True),
                       _run(K, N, R, k1, p, True, False))
    return _cache[key]


def _ref64(t):
    """fp64 x_R W_j^T + b on the chain's own stored x_R and the bf16 matrices: (N, k1 H)."""
    return t["a"][-1].to(F64) @ t["Wt"].to(F64).t() + t["tb"].to(F64).repeat(t["Wt"].shape[0] // H)


@pytest.mark.parametrize("N,R,k1,p", CASES)
def test_chain_outputs_unchanged_by_the_tail(N, R, k1, p):
    plain, tail, tail_ns = _runs(N, R, k1, p)
    for other in (tail, tail_ns):
        for name in ("a1", "a", "dh", "dx"):
            for r, (g, w) in enumerate(zip(other[name], plain[name])):
                if w is not None:
                    assert torch.equal(g.view(torch.int16), w.view(torch.int16)), f"{name}[{r}]"
        if p > 0:
            assert torch.equal(other["masks"], plain["masks"])


@pytest.mark.parametrize("N,R,k1,p", CASES)
def test_tail_y_matches_fp64_reference_and_gemm(N, R, k1, p):
    from arcweld import kernels as K
    _, tail, tail_ns = _runs(N, R, k1, p)
    Y = tail["Y"]
    assert torch.equal(Y.view(torch.int16), tail_ns["Y"].view(torch.int16)), "Y depends on colstats being given"
    ref = _ref64(tail)
    err = (Y.to(F64) - ref).abs()
    frac = float((err / (2.0 ** -7 * ref.abs() + 1e-4)).max())
    flips = float((Y.view(torch.int16) != ref.to(torch.float32).to(BF).view(torch.int16)).float().mean())
    Yg = torch.full_like(Y, float("nan"))
    K.gemm(tail["a"][-1], tail["Wt"], N, k1 * H, H, bias=tail["tb"], bias_mod=H, C=Yg)
    torch.cuda.synchronize()
    ndiff = int((Y.view(torch.int16) != Yg.view(torch.int16)).sum())
    print(f"N {N} R {R} k1 {k1} p {p}: Y {frac:.3f} of one bf16 step, {100 * flips:.4f} % off bf16(ref), "
          f"{ndiff} of {Y.numel()} elements differ from the GEMM launch")
    assert frac <= 1.0, f"Y: {frac:.2f} x one bf16 step"
    assert flips <= 0.01, f"Y: {100 * flips:.2f} % of the elements differ from the rounded reference"
    gerr = (Y.to(F64) - Yg.to(F64)).abs()
    assert bool((gerr <= 2.0 ** -7 * ref.abs() + 1e-4).all()), "Y: more than one bf16 step from the GEMM launch"


@pytest.mark.parametrize("N,R,k1,p", CASES)
def test_tail_colstats_match_fp64_sums(N, R, k1, p):
    _, tail, _ = _runs(N, R, k1, p)
    v = _ref64(tail).to(torch.float32).to(F64).view(N * k1, H)      # the f32 values, rows < N only
    want = tail["stats0"] + torch.cat([v.sum(0), (v * v).sum(0)])
    err = (tail["stats"] - want).abs()
    frac = float((err / (2e-5 * want.abs() + 1e-3)).max())
    print(f"N {N} R {R} k1 {k1} p {p}: colstats {frac:.4f} of the bar")
    assert frac <= 1.0, f"colstats: {frac:.2f} x the bar"


def test_tail_argument_checks():
    from arcweld import _native
    from arcweld import kernels as K
    N, R = 16, 1
    z = lambda *s, dt=BF: torch.zeros(*s, device="cuda", dtype=dt)  # noqa: E731
    args = lambda taps: ([z(N, H), z(N, H)] + [[z(H, taps * H)] for _ in range(2)]             # noqa: E731
                         + [[z(H, dt=torch.float32)] for _ in range(2)] + [[z(N, H)] for _ in range(4)])
    tail = ([z(H, H)] * 2, z(H, dt=torch.float32), z(N, 2 * H), None)
    with pytest.raises(_native.NativeError):      # the encoder chain has no tail
        K.res_chain_fwd(*args(1), taps=1, tail=tail)
    with pytest.raises(_native.NativeError):      # Y of the wrong width
        K.res_chain_fwd(*args(3), taps=3, tail=(tail[0], tail[1], z(N, 3 * H), None))
    with pytest.raises(_native.NativeError):      # a 3-tap backward copy cannot be a 1-tap job
        K.res_pack_weights([z(H, H)], None, [z(H, H)], taps=3, job_taps=[1])


def test_whole_step_with_and_without_the_tail(monkeypatch):
    """fused_train_step at B = 8 windows (N = 128), bf16, R = 2, from the same seeded state with ARCWELD_CONVT_TAIL on
    and off: the loss to 1e-3 relative, every parameter gradient within 1 % relative Frobenius."""
    from model.vq_vae_patch_embedd import VQVAEPatch

    from arcweld import kernels as K
    from arcweld.precision import operands
    from oracle import gen
    from oracle import vqvae as ov

    kw = dict(hidden_dim=512, num_embeddings=512, embedding_dim=64, n_resblocks=2, patch_size=25)
    sd = ov.det_state_dict(ov.VQVAEConfig(**kw), 41)
    x = torch.tensor(gen.windows(42, 8), device="cuda")
    out, launches = {}, {}
    real = K.res_chain_fwd
    for mode in ("0", "1"):
        monkeypatch.setenv("ARCWELD_CONVT_TAIL", mode)
        seen = []
        monkeypatch.setattr(K, "res_chain_fwd", lambda *a, _s=seen, **k: (_s.append(k.get("tail") is not None),
                                                                          real(*a, **k))[1])
        m = VQVAEPatch(input_dim=2, learning_rate=1e-3, dropout_p=0.1, batch_norm=False, **kw)
        m.load_state_dict({k: torch.tensor(v) for k, v in sd.items()})
        m = m.cuda().train()
        with operands(torch.bfloat16):
            loss = m.fused_train_step(x, 1.0)
        torch.cuda.synchronize()
        out[mode] = (loss.item(), {n: p.grad.detach().clone() for n, p in m.named_parameters()})
        launches[mode] = seen
    assert launches["0"] == [False, False] and launches["1"] == [False, True]   # encoder chain, decoder chain
    l0, l1 = out["0"][0], out["1"][0]
    worst = 0.0
    for n, g0 in out["0"][1].items():
        g1 = out["1"][1][n]
        if n == "reverse_patch_embed.proj.0.bias":   # feeds a train-mode BatchNorm: analytically zero, noise only
            assert g0.abs().max().item() < 1e-5 and g1.abs().max().item() < 1e-5
            continue
        if g0.norm() == 0:
            assert g1.norm() == 0, n
            continue
        rel = float((g0 - g1).norm() / g0.norm())
        worst = max(worst, rel)
        assert rel <= 1e-2, f"{n}: {rel:.3g}"
    print(f"whole step tail on / off: loss {l1:.9g} / {l0:.9g} (relative {abs(l1 - l0) / abs(l0):.3g}), "
          f"largest gradient relative Frobenius difference {worst:.3g}")
    assert abs(l1 - l0) <= 1e-3 * abs(l0)
