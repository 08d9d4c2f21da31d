"""Ids back to signals (VQVAEPatch.decode_ids / arcweld.vqvae.decode / aw_vq_decode_gather): against the reference's
recorded eval outputs, against the module's own eval forward (fp32 within the standing 1e-4; bf16 through an f64
restatement on the same ids), the gather kernel bit for bit, and its range check."""
import os

import numpy as np
import pytest
import torch

from conftest import GOLDEN, golden
from oracle import gen
from oracle import vqvae as ov

pytestmark = pytest.mark.gpu

# (constructor arguments, windows, weight seed) of the fixtures tests/test_vqvae_module.py pins
FIXTURES = {
    "vqvae_small.npz": (dict(hidden_dim=64, num_embeddings=64, embedding_dim=16, n_resblocks=2, patch_size=25), 8, 301),
    "vqvae_small_p10.npz": (dict(hidden_dim=64, num_embeddings=64, embedding_dim=16, n_resblocks=1, patch_size=10), 4,
                            305),
}


def _model(kw, wseed):
    from model.vq_vae_patch_embedd import VQVAEPatch
    m = VQVAEPatch(input_dim=2, learning_rate=1e-3, dropout_p=0.0, batch_norm=False, **kw)
    sd = ov.det_state_dict(ov.VQVAEConfig(**kw), wseed)
    m.load_state_dict({k: torch.tensor(v) for k, v in sd.items()})
    return m.cuda(), sd


def _S(m):
    return m.seq_len * m.input_dim // m.patch_size


def test_reference_checkpoint_ids_decode_to_the_reference_reconstruction():
    from arcweld.precision import operands
    from model.vq_vae_patch_embedd import VQVAEPatch
    g = golden("ref_ckpt_outputs.npz")
    with operands(torch.float32):
        m = VQVAEPatch.load_from_checkpoint(os.path.join(GOLDEN, "ref_vqvae_small.ckpt")).cuda().eval()
        ids = torch.tensor(g["vq_idx"], device="cuda").view(4, 16)
        x_hat = m.decode_ids(ids)
    assert x_hat.shape == (4, 200, 2) and x_hat.dtype == torch.float32
    np.testing.assert_allclose(x_hat.cpu().numpy(), g["vq_x_hat"], rtol=1e-4, atol=1e-4)


@pytest.mark.parametrize("fname", list(FIXTURES))
def test_fixture_ids_decode_to_the_reference_eval_output(fname):
    """The encoder of these fixtures has no BatchNorm and dropout 0, so the recorded train-step ids are the eval ids;
    eval_x_hat was taken after that step, on the running statistics the fixture records."""
    from arcweld.precision import operands
    kw, B, wseed = FIXTURES[fname]
    g = golden(fname)
    m, _ = _model(kw, wseed)
    sd = m.state_dict()
    for k in g.files:
        if k.startswith("state/") and "running" in k:
            sd[k[6:]].copy_(torch.tensor(g[k]))
    m.eval()
    with operands(torch.float32):
        x_hat = m.decode_ids(torch.tensor(g["idx"], device="cuda").view(B, -1))
    assert x_hat.shape[1:] == (200, 2) and g["idx"].size == B * _S(m)
    np.testing.assert_allclose(x_hat.cpu().numpy(), g["eval_x_hat"], rtol=1e-4, atol=1e-4)


def _oracle_eval_on_ids(sd, x, cfg, ids):
    """oracle.vqvae.vqvae_forward(train=False) in f64 with the quantizer replaced by a lookup of the given ids."""
    sd64 = {k: torch.tensor(v).double() if np.issubdtype(v.dtype, np.floating) else torch.tensor(v)
            for k, v in sd.items()}
    E = sd64["vector_quantization.embedding.weight"]
    idc = torch.tensor(ids)
    quant = lambda z: (torch.zeros(()), E[idc].view(z.shape), torch.zeros(()), idc)  # noqa: E731
    _, x_hat, _ = ov.vqvae_forward(sd64, torch.tensor(x).double(), cfg, train=False, quantizer=quant)
    return x_hat.numpy()


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
@pytest.mark.parametrize("Kc", [32, 512])
@pytest.mark.parametrize("W", [3, 8])
@pytest.mark.parametrize("H", [64, 512])
def test_decode_ids_matches_the_modules_own_eval_forward(H, W, Kc, dtype):
    """N = 48 (W = 3) is no multiple of a GEMM row tile; K = 32 takes the codebook-table route, K = 512 > N the
    gather-then-GEMM route; H = 512 in bf16 runs the chain launch with the ConvT tail, as forward does."""
    from arcweld.precision import operands
    kw = dict(hidden_dim=H, num_embeddings=Kc, embedding_dim=16 if H == 64 else 64, n_resblocks=2, patch_size=25)
    m, sd = _model(kw, 2301)
    m.eval()
    xn = gen.windows(2302 + W, W)
    x = torch.tensor(xn, device="cuda")
    with operands(dtype), torch.no_grad():
        _, fwd, _ = m(x)
        ids = m._last_indices.clone()
        dec = m.decode_ids(ids.view(W, -1))
    assert dec.shape == fwd.shape == (W, 200, 2)
    fwd, dec = fwd.cpu().numpy(), dec.cpu().numpy()
    if dtype == torch.float32:
        np.testing.assert_allclose(dec, fwd, rtol=1e-4, atol=1e-4)
        return
    ref = _oracle_eval_on_ids(sd, xn, ov.VQVAEConfig(**kw), ids.cpu().numpy())
    err_f, err_d = np.abs(fwd - ref).max(), np.abs(dec - ref).max()
    print(f"bf16 H={H} W={W} K={Kc}: err(forward) {err_f:.3e}  err(decode_ids) {err_d:.3e}")
    # same operand dtype and the same launches after the first layer, whose operand route differs (a GEMM over the
    # codebook + gather against a GEMM over the tokens): twice the forward's own error, plus the fp32 floor
    assert err_d <= 2 * err_f + 1e-4, (err_d, err_f)


def _gather_case(N, H, dt, Kc=37, seed=0, ids=None):
    from arcweld import kernels as K
    tx = torch.tensor(gen.normal(2400 + seed, (Kc, H)), device="cuda").to(dt)
    ta = torch.tensor(gen.normal(2401 + seed, (Kc, H)), device="cuda").to(dt)
    if ids is None:
        ids = gen.randint(2402 + seed + N, (N,), 0, Kc)
        ids[0], ids[-1] = Kc - 1, 0
    idx = torch.tensor(ids, device="cuda")
    y0 = torch.full((N, H), 7.0, device="cuda", dtype=dt)
    ya0 = torch.full((N, H), 7.0, device="cuda", dtype=dt)
    bad = torch.zeros(1, device="cuda", dtype=torch.int32)
    K.vq_decode_gather(idx, tx, ta, y0, ya0, bad)
    return tx, ta, idx, y0, ya0, int(bad.item())


@pytest.mark.parametrize("dt", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
@pytest.mark.parametrize("H", [64, 512])
@pytest.mark.parametrize("N", [1, 48, 4097])
def test_gather_kernel_copies_rows_bit_for_bit(N, H, dt):
    tx, ta, idx, y0, ya0, bad = _gather_case(N, H, dt)
    assert bad == 0
    assert torch.equal(y0.view(torch.uint8), tx[idx].view(torch.uint8))
    assert torch.equal(ya0.view(torch.uint8), ta[idx].view(torch.uint8))


def test_gather_kernel_single_table_form():
    """table_a = ya0 = None: the codebook gather of the K > N route (H = D)."""
    from arcweld import kernels as K
    E = torch.tensor(gen.normal(2410, (300, 16)), device="cuda")
    idx = torch.tensor(gen.randint(2411, (48,), 0, 300), device="cuda")
    out = torch.empty(48, 16, device="cuda")
    bad = torch.zeros(1, device="cuda", dtype=torch.int32)
    K.vq_decode_gather(idx, E, None, out, None, bad)
    assert int(bad.item()) == 0 and torch.equal(out, E[idx])


def test_ids_outside_the_codebook_are_refused_and_read_nothing():
    """The kernel guards every id by construction: K, K + 1 and -1 leave exact zero rows and a count of 3, the valid
    rows are untouched by their neighbours, and decode_ids raises ValueError naming the count and K (both routes)."""
    Kc = 37
    ids = gen.randint(2420, (48,), 0, Kc)
    ids[5], ids[17], ids[40] = Kc, Kc + 1, -1
    tx, ta, idx, y0, ya0, bad = _gather_case(48, 64, torch.float32, Kc=Kc, ids=ids)
    ok = torch.tensor((ids >= 0) & (ids < Kc), device="cuda")
    assert bad == 3
    assert torch.equal(y0[ok], tx[idx[ok]]) and torch.equal(ya0[ok], ta[idx[ok]])
    assert not y0[~ok].any() and not ya0[~ok].any() and (~ok).sum() == 3
    for Kc in (32, 512):                       # the table route (K <= N) and the gather-then-GEMM route (K > N)
        m, _ = _model(dict(hidden_dim=64, num_embeddings=Kc, embedding_dim=16, n_resblocks=1, patch_size=25), 2421)
        m.eval()
        good = gen.randint(2422, (3, 16), 0, Kc)
        assert torch.isfinite(m.decode_ids(torch.tensor(good, device="cuda"))).all()
        for v in (Kc, Kc + 1, -1):
            wrong = good.copy()
            wrong[1, 7] = v
            with pytest.raises(ValueError, match=rf"1 of 48 ids .*\[0, {Kc}\)"):
                m.decode_ids(torch.tensor(wrong, device="cuda"))


def test_tokenize_round_trip_keeps_the_window_order():
    from arcweld import tokenize
    from arcweld.precision import operands
    m, _ = _model(dict(hidden_dim=64, num_embeddings=32, embedding_dim=16, n_resblocks=2, patch_size=25), 2430)
    m.eval()
    n_cycles, B = 3, 2
    x = torch.tensor(gen.windows(2431, B * n_cycles).reshape(B, n_cycles * 200, 2), device="cuda")
    with operands(torch.float32):
        ids = tokenize.encode_ids(m, x)
        S = _S(m)
        assert ids.shape == (B, n_cycles * S)
        whole = tokenize.decode_ids(m, ids)
        parts = [m.decode_ids(ids[:, i * S:(i + 1) * S].contiguous()) for i in range(n_cycles)]
    assert whole.shape == (B, n_cycles * 200, 2)
    assert torch.equal(whole, torch.cat(parts, dim=1))


def test_train_mode_still_decodes_on_the_running_statistics():
    from arcweld.precision import operands
    m, _ = _model(dict(hidden_dim=64, num_embeddings=32, embedding_dim=16, n_resblocks=2, patch_size=25), 2440)
    ids = torch.tensor(gen.randint(2441, (5, 16), 0, 32), device="cuda")
    with operands(torch.float32):
        ref = m.eval().decode_ids(ids)
        before = {k: v.clone() for k, v in m.state_dict().items() if "running" in k or "num_batches" in k}
        assert before
        got = m.train().decode_ids(ids)
    assert torch.equal(got, ref)
    after = m.state_dict()
    for k, v in before.items():
        assert torch.equal(after[k], v), k
