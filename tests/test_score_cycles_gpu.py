"""Scoring end to end on the tiny random models of the generation tests: MyTransformerDecoder.score_ids against the same
run's logits, the fp64 oracle, the training loss and the greedy generator; arcweld.generate.score_cycles (ids, per-cycle
sums, reconstruction and quantisation errors, fewer cycles, bf16 operands); score_welding_cycles.py from two
checkpoints."""
import numpy as np
import pytest
import torch

from oracle import decoder as od
from oracle import gen
from oracle import vqvae as ov

pytestmark = pytest.mark.gpu

KW = dict(hidden_dim=64, num_embeddings=32, embedding_dim=16, n_resblocks=2, patch_size=25)
S, L, KC, N_CYCLES, B = 16, 200, 32, 2, 3
T = N_CYCLES * S + 1
TOL = 1e-4


@pytest.fixture(scope="module")
def models():
    from model.transformer_decoder import MyTransformerDecoder
    from model.vq_vae_patch_embedd import VQVAEPatch
    v = VQVAEPatch(input_dim=2, learning_rate=1e-3, dropout_p=0.0, batch_norm=False, **KW)
    v.load_state_dict({k: torch.tensor(a) for k, a in ov.det_state_dict(ov.VQVAEConfig(**KW), 2501).items()})
    torch.manual_seed(2502)
    d = MyTransformerDecoder(d_model=64, n_classes=KC + 2, seq_len=T, n_blocks=2, n_head=4)
    with torch.no_grad():                       # the 0.02 initialisation leaves near-flat logits: spread them out
        d.lm_head.weight.mul_(10.0)
    return v.cuda().eval(), d.cuda().eval()


@pytest.fixture
def fp32():
    from arcweld.precision import operands
    with operands(torch.float32):
        yield


def _ids(seed=2604):
    x = torch.tensor(gen.randint(seed, (B, T), 0, KC), device="cuda")
    x[:, 0] = KC
    return x


def _cycles(n=N_CYCLES):
    return torch.tensor(gen.windows(2603, B * n).reshape(B, n * L, 2), device="cuda")


def _scores64(logits, targets, n_valid):
    """fp64 (logp, entropy) and the exact rank of ``targets`` under logits (B, T', V) over the columns < n_valid."""
    l32 = logits[..., :n_valid].cpu()
    lsm = torch.log_softmax(l32.double(), dim=-1)
    tg = targets.cpu()[..., None]
    logp = lsm.gather(-1, tg)[..., 0]
    ent = -(lsm.exp() * lsm).sum(-1)
    ly = l32.gather(-1, tg)
    rank = ((l32 > ly) | ((l32 == ly) & (torch.arange(n_valid) < tg))).sum(-1)
    return logp.numpy(), ent.numpy(), rank.numpy()


@pytest.mark.parametrize("valid", [None, KC])
def test_score_ids_against_the_same_runs_logits(models, fp32, valid):
    _, d = models
    x = _ids()
    got = d.score_ids(x, valid_ids=valid)
    assert set(got) == {"logp", "rank", "entropy"}
    assert all(got[k].shape == (B, T - 1) for k in got)
    assert got["logp"].dtype == torch.float32 and got["entropy"].dtype == torch.float32
    assert got["rank"].dtype == torch.int32
    with torch.no_grad():
        lg = d(x)[:, :-1]
    logp, ent, rank = _scores64(lg, x[:, 1:], KC + 2 if valid is None else valid)
    print(f"score_ids vs the run's logits: max |logp| err {np.abs(got['logp'].cpu().numpy() - logp).max():.3g}, "
          f"|entropy| err {np.abs(got['entropy'].cpu().numpy() - ent).max():.3g}")
    assert np.array_equal(got["rank"].cpu().numpy(), rank)
    assert np.abs(got["logp"].cpu().numpy() - logp).max() <= TOL
    assert np.abs(got["entropy"].cpu().numpy() - ent).max() <= TOL


def test_score_ids_against_the_fp64_oracle(models, fp32):
    _, d = models
    x = _ids(2605)
    sd = {k: (t.detach().cpu().double() if t.is_floating_point() else t.detach().cpu())
          for k, t in d.state_dict().items()}
    lg = od.decoder_forward(sd, x.cpu(), 4)[:, :-1, :KC]
    want = torch.log_softmax(lg, dim=-1).gather(-1, x.cpu()[:, 1:, None])[..., 0].numpy()
    got = d.score_ids(x, valid_ids=KC)["logp"].cpu().numpy()
    print(f"score_ids vs the fp64 oracle: max |logp| err {np.abs(got - want).max():.3g}")
    assert np.abs(got - want).max() <= 2e-4      # logits within the project's 1e-4, the log-sum-exp as much again


def test_whole_vocabulary_scores_are_the_training_loss(models, fp32):
    _, d = models
    ids = _ids(2606)[:, :T - 1]                                       # [start, T - 2 ids]
    y = torch.cat([ids[:, 1:], torch.full_like(ids[:, :1], KC + 1)], dim=1)      # the targets, end token appended
    got = d.score_ids(torch.cat([ids, y[:, -1:]], dim=1))             # valid_ids=None: the softmax of the loss
    with torch.no_grad():
        loss = d.loss_gen(d(ids), y).item()
    assert abs(-got["logp"].double().mean().item() - loss) <= 1e-5 * abs(loss)


def test_greedy_generation_scores_rank_zero(models, fp32):
    _, d = models
    L0 = 1 + S
    x = _ids(2504)[:, :L0]
    out = d.generate_ids(x, T - L0, valid_ids=KC)
    with torch.no_grad():                       # precondition: no step's choice hangs on a tie
        lg = d(out)[:, L0 - 1:-1, :KC]
    top2 = torch.topk(lg, 2, dim=-1).values
    assert ((top2[..., 0] - top2[..., 1]) > 0).all()
    rank = d.score_ids(out, valid_ids=KC)["rank"]
    assert (rank[:, L0 - 1:] == 0).all()


def test_score_ids_reports_ids_outside_the_allowed_columns(models, fp32):
    _, d = models
    x = _ids()
    x[1, 5] = KC + 1                            # the end token as a target, with only the codebook ids allowed
    with pytest.raises(RuntimeError, match="1 positions"):
        d.score_ids(x, valid_ids=KC)
    assert d.score_ids(x)["rank"].min() >= 0    # the whole vocabulary takes it


@pytest.fixture(scope="module")
def full_run(models):
    """score_cycles of N_CYCLES cycles in exact fp32, computed once: (x, scores)."""
    from arcweld.generate import score_cycles
    from arcweld.precision import operands
    v, d = models
    x = _cycles()
    with operands(torch.float32):
        return x, score_cycles(v, d, x)


def test_score_cycles_shapes_ids_and_cycle_sums(models, fp32, full_run):
    v, d = models
    x, sc = full_run
    n = N_CYCLES
    want = dict(ids=((B, n * S), torch.int64), logp=((B, n * S), torch.float32), entropy=((B, n * S), torch.float32),
                rank=((B, n * S), torch.int32), cycle_nll=((B, n), torch.float32), recon_mse=((B, n), torch.float32),
                vq_mse=((B, n), torch.float32))
    assert set(sc) == set(want)
    for k, (shape, dt) in want.items():
        assert sc[k].shape == shape and sc[k].dtype == dt, k
    assert torch.equal(sc["ids"], v.encode_ids(x))
    sums = -sc["logp"].double().view(B, n, S).sum(-1)
    assert (sc["cycle_nll"].double() - sums).abs().max().item() <= S * TOL
    # the token scores are score_ids' of [start, ids] restricted to the codebook
    seq = torch.cat([torch.full_like(sc["ids"][:, :1], KC), sc["ids"]], dim=1)
    tok = d.score_ids(seq, valid_ids=KC)
    for k in ("logp", "rank", "entropy"):
        assert torch.equal(tok[k], sc[k]), k
    assert torch.isfinite(sc["logp"]).all() and (sc["rank"] >= 0).all() and (sc["rank"] < KC).all()


def test_score_cycles_reconstruction_and_quantisation_errors(models, fp32, full_run):
    from arcweld import vqvae as engine
    v, _ = models
    x, sc = full_run
    n = N_CYCLES
    x_hat = v.decode_ids(sc["ids"])
    want = ((x.double() - x_hat.double()) ** 2).view(B, n, L * 2).mean(-1)
    np.testing.assert_allclose(sc["recon_mse"].cpu().numpy(), want.cpu().numpy(), rtol=1e-4)
    idx, z = engine.encode(v, x.view(B * n, L, 2))
    E = v.vector_quantization.embedding.weight.detach().double()
    want = ((z.double() - E[idx]) ** 2).view(B, n, S * KW["embedding_dim"]).mean(-1)
    np.testing.assert_allclose(sc["vq_mse"].cpu().numpy(), want.cpu().numpy(), rtol=1e-4)
    assert (sc["vq_mse"] > 0).all() and (sc["recon_mse"] > 0).all()


def test_scoring_fewer_cycles_gives_the_first_cycles_of_the_full_run(models, fp32, full_run):
    from arcweld.generate import score_cycles
    v, d = models
    x, sc = full_run
    part = score_cycles(v, d, x[:, :L].contiguous())
    assert part["ids"].shape == (B, S) and part["cycle_nll"].shape == (B, 1)
    assert torch.equal(part["ids"], sc["ids"][:, :S]) and torch.equal(part["rank"], sc["rank"][:, :S])
    for k, m in (("logp", S), ("entropy", S), ("cycle_nll", 1), ("recon_mse", 1), ("vq_mse", 1)):
        tol = S * TOL if k == "cycle_nll" else TOL
        assert (part[k] - sc[k][:, :m]).abs().max().item() <= tol, k


def test_score_cycles_with_bf16_operands(models):
    from arcweld.generate import score_cycles
    from arcweld.precision import operands
    v, d = models
    x = _cycles()
    with operands(torch.bfloat16):
        sc = score_cycles(v, d, x)
        seq = torch.cat([torch.full_like(sc["ids"][:, :1], KC), sc["ids"]], dim=1)
        with torch.no_grad():
            lg = d(seq)[:, :-1]
    for k in ("logp", "entropy", "cycle_nll", "recon_mse", "vq_mse"):
        assert torch.isfinite(sc[k]).all(), k
    _, _, rank = _scores64(lg, sc["ids"], KC)
    assert np.array_equal(sc["rank"].cpu().numpy(), rank)


def test_script_scores_from_two_checkpoints(models, fp32, tmp_path):
    """score_welding_cycles.py end to end: both models through load_from_checkpoint, synthetic cycles, the .npz."""
    import score_welding_cycles as swc
    from arcweld.generate import score_cycles
    v, d = models
    v.save_checkpoint(str(tmp_path / "v.ckpt"))
    d.save_checkpoint(str(tmp_path / "d.ckpt"))
    out = tmp_path / "scores.npz"
    swc.main(swc.parser().parse_args(["--vqvae-model", str(tmp_path / "v.ckpt"), "--transformer-model",
                                      str(tmp_path / "d.ckpt"), "--n-cycles", str(N_CYCLES), "--n-seqs", str(B),
                                      "--seed", "4", "--out", str(out)]))
    with np.load(out, allow_pickle=False) as f:
        got = {k: f[k] for k in f.files}
    assert set(got) == {"x", "ids", "logp", "rank", "entropy", "cycle_nll", "recon_mse", "vq_mse"}
    assert got["x"].shape == (B, N_CYCLES * L, 2) and got["ids"].shape == (B, N_CYCLES * S)
    assert got["ids"].dtype == np.int64 and got["rank"].dtype == np.int32 and got["cycle_nll"].shape == (B, N_CYCLES)
    want = score_cycles(v, d, torch.tensor(got["x"], device="cuda"))
    assert np.array_equal(got["ids"], want["ids"].cpu().numpy())
    assert np.array_equal(got["rank"], want["rank"].cpu().numpy())
    for k in ("logp", "entropy", "cycle_nll", "recon_mse", "vq_mse"):
        np.testing.assert_allclose(got[k], want[k].cpu().numpy(), rtol=1e-4, atol=1e-4, err_msg=k)
