"""Generation end to end on tiny random models: MyTransformerDecoder.generate_ids against the existing cached
``generate``, and arcweld.generate.continue_cycles (prompt ids kept, generated ids inside the codebook, both halves of
x_hat, seeding, and the shape checks)."""
import numpy as np
import pytest
import torch

from oracle import gen
from oracle import vqvae as ov

pytestmark = pytest.mark.gpu

KW = dict(hidden_dim=64, num_embeddings=32, embedding_dim=16, n_resblocks=2, patch_size=25)
S, L, KC, N_CYCLES, C_PROMPT, B = 16, 200, 32, 2, 1, 3


@pytest.fixture(scope="module")
def models():
    from model.transformer_decoder import MyTransformerDecoder
    from model.vq_vae_patch_embedd import VQVAEPatch
    v = VQVAEPatch(input_dim=2, learning_rate=1e-3, dropout_p=0.0, batch_norm=False, **KW)
    v.load_state_dict({k: torch.tensor(a) for k, a in ov.det_state_dict(ov.VQVAEConfig(**KW), 2501).items()})
    torch.manual_seed(2502)
    d = MyTransformerDecoder(d_model=64, n_classes=KC + 2, seq_len=N_CYCLES * S + 1, n_blocks=2, n_head=4)
    with torch.no_grad():                       # the 0.02 initialisation leaves near-flat logits: spread them out
        d.lm_head.weight.mul_(10.0)
    return v.cuda().eval(), d.cuda().eval()


@pytest.fixture
def fp32():
    from arcweld.precision import operands
    with operands(torch.float32):
        yield


def _prompt():
    return torch.tensor(gen.windows(2503, B * C_PROMPT).reshape(B, C_PROMPT * L, 2), device="cuda")


def test_generate_ids_greedy_equals_the_cached_generate(models, fp32):
    _, d = models
    x = torch.tensor(gen.randint(2504, (B, 1 + C_PROMPT * S), 0, KC), device="cuda")
    x[:, 0] = KC
    n_new = (N_CYCLES - C_PROMPT) * S
    got = d.generate_ids(x, n_new)
    assert got.shape == (B, x.shape[1] + n_new) and got.dtype == torch.int64
    want = d.generate(x, use_cache=True)[:, :x.shape[1] + n_new]
    # precondition: no step's choice hangs on a tie (logits recomputed by the full forward)
    with torch.no_grad():
        lg = d(want)[:, x.shape[1] - 1:-1]
    top2 = torch.topk(lg, 2, dim=-1).values
    assert ((top2[..., 0] - top2[..., 1]) > 0).all()
    assert torch.equal(got, want)
    assert torch.equal(got[:, :x.shape[1]], x)


def test_continue_cycles_end_to_end(models, fp32):
    from arcweld.generate import continue_cycles
    v, d = models
    xp = _prompt()
    out = continue_cycles(v, d, xp, N_CYCLES)
    ids, x_hat = out["ids"], out["x_hat"]
    assert ids.shape == (B, N_CYCLES * S) and ids.dtype == torch.int64
    assert x_hat.shape == (B, N_CYCLES * L, 2) and x_hat.dtype == torch.float32
    assert torch.equal(ids[:, :C_PROMPT * S], v.encode_ids(xp))
    assert (ids >= 0).all() and (ids < KC).all()
    with torch.no_grad():
        _, recon, _ = v(xp)
    np.testing.assert_allclose(x_hat[:, :C_PROMPT * L].cpu().numpy(), recon.cpu().numpy(), rtol=1e-4, atol=1e-4)
    assert torch.equal(x_hat[:, C_PROMPT * L:], v.decode_ids(ids[:, C_PROMPT * S:].contiguous()))
    # sampling: inside the codebook, reproducible per seed, different across seeds
    s0 = continue_cycles(v, d, xp, N_CYCLES, do_sample=True, top_k=5, seed=0)["ids"]
    s0b = continue_cycles(v, d, xp, N_CYCLES, do_sample=True, top_k=5, seed=0)["ids"]
    s1 = continue_cycles(v, d, xp, N_CYCLES, do_sample=True, top_k=5, seed=1)["ids"]
    assert (s0 >= 0).all() and (s0 < KC).all() and (s1 < KC).all()
    assert torch.equal(s0, s0b) and not torch.equal(s0, s1)
    assert torch.equal(s0[:, :C_PROMPT * S], ids[:, :C_PROMPT * S])
    t = continue_cycles(v, d, xp, N_CYCLES, do_sample=True, seed=0, temperature=0.7)["ids"]
    assert (t >= 0).all() and (t < KC).all()


def test_script_generates_from_two_checkpoints(models, fp32, tmp_path):
    """generate_welding_cycles.py end to end: both models through load_from_checkpoint, synthetic prompts, the .npz."""
    import generate_welding_cycles as gwc
    from arcweld.generate import continue_cycles
    v, d = models
    v.save_checkpoint(str(tmp_path / "v.ckpt"))
    d.save_checkpoint(str(tmp_path / "d.ckpt"))
    out = tmp_path / "cycles.npz"
    gwc.main(gwc.parser().parse_args(["--vqvae-model", str(tmp_path / "v.ckpt"), "--transformer-model",
                                      str(tmp_path / "d.ckpt"), "--n-cycles", str(N_CYCLES), "--prompt-cycles",
                                      str(C_PROMPT), "--n-seqs", str(B), "--seed", "4", "--out", str(out)]))
    with np.load(out, allow_pickle=False) as f:
        prompt, ids, x_hat = f["prompt"], f["ids"], f["x_hat"]
    assert prompt.shape == (B, C_PROMPT * L, 2) and ids.shape == (B, N_CYCLES * S)
    assert x_hat.shape == (B, N_CYCLES * L, 2) and ids.dtype == np.int64 and (ids >= 0).all() and (ids < KC).all()
    want = continue_cycles(v, d, torch.tensor(prompt, device="cuda"), N_CYCLES)
    assert np.array_equal(ids, want["ids"].cpu().numpy())
    np.testing.assert_allclose(x_hat, want["x_hat"].cpu().numpy(), rtol=1e-4, atol=1e-4)


def test_generate_ids_refuses_to_run_past_seq_len(models):
    _, d = models
    x = torch.zeros(B, 17, dtype=torch.int64, device="cuda")
    with pytest.raises(ValueError, match="seq_len"):
        d.generate_ids(x, 17)
    with pytest.raises(ValueError, match="top_k"):
        d.generate_ids(x, 4, top_k=33, valid_ids=KC)        # more than the allowed columns, as torch.topk refuses
    assert d.generate_ids(x, 0).shape == (B, 17)


def test_continue_cycles_checks_that_the_two_models_fit(models):
    from arcweld.generate import continue_cycles
    from model.transformer_decoder import MyTransformerDecoder
    v, d = models
    xp = _prompt()
    wrong_v = MyTransformerDecoder(d_model=64, n_classes=KC + 3, seq_len=N_CYCLES * S + 1, n_blocks=1, n_head=4).cuda()
    with pytest.raises(ValueError, match=rf"n_classes {KC + 3}.*{KC + 2}"):
        continue_cycles(v, wrong_v, xp, N_CYCLES)
    wrong_t = MyTransformerDecoder(d_model=64, n_classes=KC + 2, seq_len=N_CYCLES * S, n_blocks=1, n_head=4).cuda()
    with pytest.raises(ValueError, match=rf"seq_len {N_CYCLES * S}.*{N_CYCLES * S + 1}"):
        continue_cycles(v, wrong_t, xp, N_CYCLES)
    with pytest.raises(ValueError, match="prompt"):
        continue_cycles(v, d, torch.cat([xp, xp], dim=1), N_CYCLES)      # c == n_cycles: nothing left to generate
