"""Beam search end to end on the tiny random models of tests/test_generate_logp_gpu.py: one beam against greedy
``generate_ids``, every hypothesis against ``score_ids`` of its own ids (which a wrong KV-cache reorder misses by orders
of magnitude), an exhaustive search over a 3-id vocabulary against brute force, ``continue_cycles`` and the script."""
import itertools

import numpy as np
import pytest
import torch

from oracle import gen
from oracle import vqvae as ov

pytestmark = pytest.mark.gpu

KW = dict(hidden_dim=64, num_embeddings=32, embedding_dim=16, n_resblocks=2, patch_size=25)
S, L, KC, N_CYCLES, C_PROMPT, B = 16, 200, 32, 2, 1, 3
N_NEW = (N_CYCLES - C_PROMPT) * S
TOL = 4e-4          # cached-decode against full-forward logp: the bound tests/test_generate_logp_gpu.py derives


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


def _start_ids(hi=KC):
    x = torch.tensor(gen.randint(2504, (B, 1 + C_PROMPT * S), 0, hi), device="cuda")
    x[:, 0] = KC
    return x


def _prompt():
    return torch.tensor(gen.windows(2503, B * C_PROMPT).reshape(B, C_PROMPT * L, 2), device="cuda")


@pytest.mark.parametrize("valid", [None, KC])
def test_one_beam_is_greedy_decoding(models, fp32, valid):
    _, d = models
    x = _start_ids()
    ids, lp = d.generate_ids(x, N_NEW, valid_ids=valid, return_logp=True)
    bs = d.beam_search_ids(x, N_NEW, 1, valid_ids=valid)
    assert set(bs) == {"ids", "scores", "logp"}
    assert bs["ids"].shape == (B, 1, x.shape[1] + N_NEW) and bs["ids"].dtype == torch.int64
    assert bs["scores"].shape == (B, 1) and bs["logp"].shape == (B, 1, N_NEW) and bs["logp"].dtype == torch.float32
    assert torch.equal(bs["ids"][:, 0], ids)
    err = (bs["scores"][:, 0].double() - lp["logp"].double().sum(-1)).abs().max().item()
    print(f"valid_ids {valid}: max |beam score - sum of greedy logp| = {err:.2e}")
    assert err <= TOL * N_NEW
    assert (bs["logp"][:, 0] - lp["logp"]).abs().max().item() <= TOL


def test_every_hypothesis_carries_the_models_own_likelihood(models, fp32):
    """B 3, 4 beams, 16 new ids: each hypothesis' logp against ``score_ids`` of its own ids, within the 4e-4 that
    tests/test_generate_logp_gpu.py derives for cached-decode against full-forward logits; a cache row gathered from a
    wrong parent misses it by orders of magnitude.  Measured on an MI355X: 9.5e-7 (logp), 4.1e-6 (score against the sum
    of 16 logp)."""
    _, d = models
    x = _start_ids()
    L0, W = x.shape[1], 4
    bs = d.beam_search_ids(x, N_NEW, W, valid_ids=KC, num_return=W)
    ids, scores, logp = bs["ids"], bs["scores"], bs["logp"]
    assert ids.shape == (B, W, L0 + N_NEW) and scores.shape == (B, W) and logp.shape == (B, W, N_NEW)
    want = d.score_ids(ids.view(B * W, -1), valid_ids=KC)["logp"][:, L0 - 1:].view(B, W, N_NEW)
    err = (logp - want).abs().max().item()
    serr = (scores.double() - logp.double().sum(-1)).abs().max().item()
    print(f"max |beam logp - scored logp| = {err:.2e}, max |score - sum of logp| = {serr:.2e}")
    assert err <= TOL and serr <= TOL * N_NEW
    assert torch.isfinite(scores).all() and (scores[:, :-1] >= scores[:, 1:]).all()
    for b in range(B):
        assert len({tuple(h) for h in ids[b].tolist()}) == W           # pairwise distinct
    assert (ids[:, :, L0:] >= 0).all() and (ids[:, :, L0:] < KC).all()
    assert (ids[:, :, :L0] == x[:, None]).all()
    again = d.beam_search_ids(x, N_NEW, W, valid_ids=KC, num_return=W)
    assert all(torch.equal(bs[k], again[k]) for k in bs)
    best = d.beam_search_ids(x, N_NEW, W, valid_ids=KC)                 # num_return = 1: the head of the same list
    assert torch.equal(best["ids"], ids[:, :1]) and torch.equal(best["scores"], scores[:, :1])


def test_a_beam_wider_than_the_search_space_finds_every_sequence(models, fp32):
    """valid_ids 3, n_new 3, 32 beams >= 3 ** 3: the search is exhaustive, so its finite hypotheses are all 27
    sequences, scored as brute force scores them (27 full forwards per prompt through ``score_ids``), and the best is
    the brute-force argmax.  That last claim needs the two best sequences to lie further apart than the two
    computations can differ, 3 * 4e-4 each: the test asserts a gap of 10 * 3 * 4e-4 = 1.2e-2 before it compares.
    oracle/decoder.py in f64 on the CPU gives top-two gaps of 0.9726, 1.2019 and 1.2019 for the three prompts of this
    model seed (2502)."""
    _, d = models
    x = _start_ids(hi=3)                                                # score_ids wants every target below valid_ids
    L0, n_new, W = x.shape[1], 3, 32
    all_seq = torch.tensor(list(itertools.product(range(3), repeat=n_new)), device="cuda")          # (27, 3)
    full = torch.cat([x[:, None].expand(B, 27, L0), all_seq[None].expand(B, 27, n_new)], dim=2)
    brute = d.score_ids(full.reshape(B * 27, -1), valid_ids=3)["logp"][:, L0 - 1:].double().sum(-1).view(B, 27)
    top2 = brute.topk(2, dim=1).values
    gaps = (top2[:, 0] - top2[:, 1]).tolist()
    print("brute-force top-two gaps:", ["%.4f" % g for g in gaps])
    assert min(gaps) > 10 * n_new * TOL
    bs = d.beam_search_ids(x, n_new, W, valid_ids=3, num_return=W)
    ids, scores = bs["ids"], bs["scores"]
    assert torch.isfinite(scores[:, :27]).all() and (scores[:, 27:] == -float("inf")).all()
    assert (scores[:, :-1] >= scores[:, 1:]).all()
    for b in range(B):
        found = [tuple(h) for h in ids[b, :27, L0:].tolist()]
        assert set(found) == set(itertools.product(range(3), repeat=n_new)) and len(set(found)) == 27
        at = [t[0] * 9 + t[1] * 3 + t[2] for t in found]               # the row of `brute` each hypothesis is
        err = (scores[b, :27].double() - brute[b, at]).abs().max().item()
        assert err <= n_new * TOL, err
        assert at[0] == int(brute[b].argmax())
    assert (ids[:, :, :L0] == x[:, None]).all() and (ids[:, :, L0:] >= 0).all() and (ids[:, :, L0:] < 3).all()


def test_short_searches(models, fp32):
    _, d = models
    x = _start_ids()
    L0 = x.shape[1]
    z = d.beam_search_ids(x, 0, 4, valid_ids=KC, num_return=2)
    assert torch.equal(z["ids"], x[:, None].expand(B, 2, L0)) and z["ids"].is_contiguous()
    assert z["scores"].shape == (B, 2) and (z["scores"] == 0).all() and z["logp"].shape == (B, 2, 0)
    one = d.beam_search_ids(x, 1, 4, valid_ids=KC, num_return=4)       # one step: the four most likely next ids
    assert torch.equal(one["ids"][:, 0], d.generate_ids(x, 1, valid_ids=KC))
    want = d.score_ids(one["ids"].view(B * 4, -1), valid_ids=KC)["logp"][:, L0 - 1:].view(B, 4)
    assert (one["scores"] - want).abs().max().item() <= TOL and torch.equal(one["scores"], one["logp"][:, :, 0])
    assert (one["scores"][:, :-1] >= one["scores"][:, 1:]).all()
    assert all(len(set(r)) == 4 for r in one["ids"][:, :, L0].tolist())


def test_bf16_operands_search_deterministically(models):
    from arcweld.precision import operands
    _, d = models
    x = _start_ids()
    with operands(torch.bfloat16):
        assert torch.equal(d.beam_search_ids(x, N_NEW, 1, valid_ids=KC)["ids"][:, 0],
                           d.generate_ids(x, N_NEW, valid_ids=KC))
        a = d.beam_search_ids(x, N_NEW, 4, valid_ids=KC, num_return=4)
        b = d.beam_search_ids(x, N_NEW, 4, valid_ids=KC, num_return=4)
    assert all(torch.equal(a[k], b[k]) for k in a)
    assert (a["scores"][:, :-1] >= a["scores"][:, 1:]).all()
    assert (a["scores"].double() - a["logp"].double().sum(-1)).abs().max().item() <= TOL * N_NEW


def test_continue_cycles_returns_ranked_hypotheses(models, fp32):
    from arcweld.generate import continue_cycles
    v, d = models
    xp = _prompt()
    R = 3
    assert set(continue_cycles(v, d, xp, N_CYCLES)) == {"ids", "x_hat"}
    out = continue_cycles(v, d, xp, N_CYCLES, num_beams=4, num_return=R, return_logp=True)
    assert set(out) == {"ids", "x_hat", "beam_ids", "beam_scores", "beam_x_hat", "gen_logp", "gen_logq",
                        "gen_cycle_nll"}
    assert out["ids"].shape == (B, N_CYCLES * S) and out["x_hat"].shape == (B, N_CYCLES * L, 2)
    assert out["beam_ids"].shape == (B, R, N_CYCLES * S) and out["beam_ids"].dtype == torch.int64
    assert out["beam_scores"].shape == (B, R) and out["beam_x_hat"].shape == (B, R, N_CYCLES * L, 2)
    assert torch.equal(out["beam_ids"][:, 0], out["ids"]) and torch.equal(out["beam_x_hat"][:, 0], out["x_hat"])
    n_gen = N_CYCLES - C_PROMPT
    assert out["gen_logp"].shape == (B, n_gen * S) and out["gen_cycle_nll"].shape == (B, n_gen)
    assert (out["gen_logq"] == 0).all() and out["gen_logq"].shape == (B, n_gen * S)
    sc = d.score_groups(torch.cat([torch.full_like(out["ids"][:, :1], KC), out["ids"]], 1), N_CYCLES, S, valid_ids=KC)
    assert (sc["group_nll"][:, C_PROMPT:] - out["gen_cycle_nll"]).abs().max().item() <= TOL * S
    assert (out["beam_scores"][:, 0] + out["gen_cycle_nll"].sum(-1)).abs().max().item() <= TOL * N_NEW
    # the prompt's ids are the encoder's, whatever decodes them afterwards
    plain = continue_cycles(v, d, xp, N_CYCLES)
    assert torch.equal(out["beam_ids"][:, :, :C_PROMPT * S], plain["ids"][:, None, :C_PROMPT * S].expand(B, R, -1))
    without = continue_cycles(v, d, xp, N_CYCLES, num_beams=4)
    assert set(without) == {"ids", "x_hat", "beam_ids", "beam_scores", "beam_x_hat"}
    assert without["beam_ids"].shape == (B, 1, N_CYCLES * S) and torch.equal(without["ids"], out["ids"])
    for kw in (dict(do_sample=True), dict(top_k=3), dict(top_p=0.9), dict(min_p=0.1), dict(temperature=0.5)):
        with pytest.raises(ValueError, match="num_beams"):
            continue_cycles(v, d, xp, N_CYCLES, num_beams=4, **kw)
    for kw in (dict(num_beams=0), dict(num_beams=33), dict(num_beams=4, num_return=5)):
        with pytest.raises(ValueError):
            continue_cycles(v, d, xp, N_CYCLES, **kw)


def test_script_writes_the_beam_arrays_only_with_the_flags(models, fp32, tmp_path):
    import generate_welding_cycles as gwc
    v, d = models
    v.save_checkpoint(str(tmp_path / "v.ckpt"))
    d.save_checkpoint(str(tmp_path / "d.ckpt"))
    base = ["--vqvae-model", str(tmp_path / "v.ckpt"), "--transformer-model", str(tmp_path / "d.ckpt"), "--n-cycles",
            str(N_CYCLES), "--prompt-cycles", str(C_PROMPT), "--n-seqs", str(B), "--seed", "4"]
    out = tmp_path / "beam.npz"
    gwc.main(gwc.parser().parse_args(base + ["--num-beams", "4", "--num-return", "2", "--out", str(out)]))
    with np.load(out, allow_pickle=False) as f:
        assert set(f.files) == {"prompt", "ids", "x_hat", "beam_ids", "beam_scores", "beam_x_hat"}
        assert f["beam_ids"].shape == (B, 2, N_CYCLES * S) and f["beam_ids"].dtype == np.int64
        assert f["beam_scores"].shape == (B, 2) and f["beam_scores"].dtype == np.float32
        assert f["beam_x_hat"].shape == (B, 2, N_CYCLES * L, 2)
        assert np.array_equal(f["beam_ids"][:, 0], f["ids"]) and np.array_equal(f["beam_x_hat"][:, 0], f["x_hat"])
        assert (f["beam_scores"][:, 0] >= f["beam_scores"][:, 1]).all() and (f["beam_scores"] <= 0).all()
        beam_ids = f["ids"]
    plain = tmp_path / "plain.npz"
    gwc.main(gwc.parser().parse_args(base + ["--out", str(plain)]))
    with np.load(plain, allow_pickle=False) as f:
        assert set(f.files) == {"prompt", "ids", "x_hat"}
        assert f["ids"].shape == beam_ids.shape
