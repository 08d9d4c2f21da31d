"""Generation with the nucleus / min-p filters and per-token log-probabilities, on the tiny random models of
tests/test_generate_cycles_gpu.py: ``generate_ids(return_logp=True)`` against ``score_ids`` of what it generated,
seeding under top_p, the id range, the per-cycle sums of ``continue_cycles`` and the script's extra arrays."""
import numpy as np
import pytest
import torch

from oracle import gen
from oracle import vqvae as ov

pytestmark = pytest.mark.gpu

KW = dict(hidden_dim=64, num_embeddings=32, embedding_dim=16, n_resblocks=2, patch_size=25)
S, L, KC, N_CYCLES, C_PROMPT, B = 16, 200, 32, 2, 1, 3
N_NEW = (N_CYCLES - C_PROMPT) * S


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


def _start_ids():
    x = torch.tensor(gen.randint(2504, (B, 1 + C_PROMPT * S), 0, KC), device="cuda")
    x[:, 0] = KC
    return x


def _prompt():
    return torch.tensor(gen.windows(2503, B * C_PROMPT).reshape(B, C_PROMPT * L, 2), device="cuda")


@pytest.mark.parametrize("valid", [None, KC])
def test_generated_logp_agrees_with_scoring_the_generated_ids(models, fp32, valid):
    """Both sides are a logit minus a log-sum-exp of logits; cached-decode and full-forward logits agree within 1e-4
    (test_kv_cache_prefill_and_decode_match_full_forward), so the two differ by at most 2e-4 plus the 1e-4 kernel bar
    of each side: 4e-4.  Measured on an MI355X: 9.5e-7 greedy and 7.2e-7 sampled at most."""
    _, d = models
    x = _start_ids()
    L0 = x.shape[1]
    plain = d.generate_ids(x, N_NEW, valid_ids=valid)
    ids, lp = d.generate_ids(x, N_NEW, valid_ids=valid, return_logp=True)
    assert torch.equal(ids, plain)
    assert set(lp) == {"logp", "logq"} and all(t.shape == (B, N_NEW) and t.dtype == torch.float32 for t in lp.values())
    assert (lp["logq"] == 0).all()                                  # greedy: nothing was drawn
    want = d.score_ids(ids, valid_ids=valid)["logp"][:, L0 - 1:]
    err = (lp["logp"] - want).abs().max().item()
    print(f"valid_ids {valid}: max |generated logp - scored logp| = {err:.2e}")
    assert err <= 4e-4
    # sampled with every filter on: logp is still the model's own distribution, logq the narrower one
    sid, slp = d.generate_ids(x, N_NEW, valid_ids=valid, do_sample=True, top_k=12, min_p=0.01, top_p=0.9,
                              temperature=0.8, seed=3, return_logp=True)
    want = d.score_ids(sid, valid_ids=valid)["logp"][:, L0 - 1:]
    err = (slp["logp"] - want).abs().max().item()
    print(f"valid_ids {valid}, sampled: max |generated logp - scored logp| = {err:.2e}")
    assert err <= 4e-4
    assert (slp["logq"] <= 0).all() and torch.isfinite(slp["logq"]).all() and torch.isfinite(slp["logp"]).all()


def test_nucleus_sampling_is_seeded_and_stays_inside_the_allowed_ids(models, fp32):
    _, d = models
    x = _start_ids()
    a = d.generate_ids(x, N_NEW, do_sample=True, top_p=0.9, valid_ids=KC, seed=0)
    b = d.generate_ids(x, N_NEW, do_sample=True, top_p=0.9, valid_ids=KC, seed=0)
    c = d.generate_ids(x, N_NEW, do_sample=True, top_p=0.9, valid_ids=KC, seed=1)
    assert torch.equal(a, b) and not torch.equal(a, c)
    for t in (a, c, d.generate_ids(x, N_NEW, do_sample=True, min_p=0.1, valid_ids=KC, seed=2)):
        assert t.shape == (B, x.shape[1] + N_NEW) and torch.equal(t[:, :x.shape[1]], x)
        assert (t[:, x.shape[1]:] >= 0).all() and (t[:, x.shape[1]:] < KC).all()
    # a nucleus so small that only the mode is left is greedy decoding
    assert torch.equal(d.generate_ids(x, N_NEW, do_sample=True, top_p=1e-6, valid_ids=KC, seed=5),
                       d.generate_ids(x, N_NEW, valid_ids=KC))
    ids, lp = d.generate_ids(x, 0, return_logp=True)
    assert ids.shape == x.shape and lp["logp"].shape == (B, 0)


def test_continue_cycles_returns_the_generated_cycles_likelihood(models, fp32):
    from arcweld.generate import continue_cycles
    v, d = models
    xp = _prompt()
    plain = continue_cycles(v, d, xp, N_CYCLES)
    assert set(plain) == {"ids", "x_hat"}
    out = continue_cycles(v, d, xp, N_CYCLES, return_logp=True)
    assert torch.equal(out["ids"], plain["ids"]) and torch.equal(out["x_hat"], plain["x_hat"])
    n_gen = N_CYCLES - C_PROMPT
    assert out["gen_logp"].shape == (B, n_gen * S) and out["gen_logq"].shape == (B, n_gen * S)
    assert out["gen_cycle_nll"].shape == (B, n_gen)
    np.testing.assert_allclose(out["gen_cycle_nll"].cpu().numpy(),
                               -out["gen_logp"].view(B, -1, S).sum(-1).cpu().numpy(), rtol=1e-6)
    s = continue_cycles(v, d, xp, N_CYCLES, do_sample=True, top_p=0.9, min_p=0.01, seed=4, return_logp=True)
    assert (s["ids"] >= 0).all() and (s["ids"] < KC).all()
    np.testing.assert_allclose(s["gen_cycle_nll"].cpu().numpy(),
                               -s["gen_logp"].view(B, -1, S).sum(-1).cpu().numpy(), rtol=1e-6)
    # the scale of score_cycles: the same ids scored by a full forward, per id within the 4e-4 of the test above, so
    # within 4e-4 * S per cycle
    sc = d.score_groups(torch.cat([torch.full_like(s["ids"][:, :1], KC), s["ids"]], 1), N_CYCLES, S, valid_ids=KC)
    assert (sc["group_nll"][:, C_PROMPT:] - s["gen_cycle_nll"]).abs().max().item() <= 4e-4 * S


def test_script_writes_the_three_extra_arrays(models, fp32, tmp_path):
    import generate_welding_cycles as gwc
    v, d = models
    v.save_checkpoint(str(tmp_path / "v.ckpt"))
    d.save_checkpoint(str(tmp_path / "d.ckpt"))
    out = tmp_path / "cycles.npz"
    gwc.main(gwc.parser().parse_args(["--vqvae-model", str(tmp_path / "v.ckpt"), "--transformer-model",
                                      str(tmp_path / "d.ckpt"), "--n-cycles", str(N_CYCLES), "--prompt-cycles",
                                      str(C_PROMPT), "--n-seqs", str(B), "--seed", "4", "--top-p", "0.9",
                                      "--do-sample", "--logp", "--out", str(out)]))
    n_gen = N_CYCLES - C_PROMPT
    with np.load(out, allow_pickle=False) as f:
        assert set(f.files) == {"prompt", "ids", "x_hat", "gen_logp", "gen_logq", "gen_cycle_nll"}
        assert f["ids"].shape == (B, N_CYCLES * S) and (f["ids"] >= 0).all() and (f["ids"] < KC).all()
        assert f["gen_logp"].shape == (B, n_gen * S) and f["gen_logp"].dtype == np.float32
        assert f["gen_logq"].shape == (B, n_gen * S) and f["gen_cycle_nll"].shape == (B, n_gen)
        assert (f["gen_logp"] <= 0).all() and (f["gen_logq"] <= 0).all()
        np.testing.assert_allclose(f["gen_cycle_nll"], -f["gen_logp"].reshape(B, n_gen, S).sum(-1), rtol=1e-6)
