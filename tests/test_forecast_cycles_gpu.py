"""Ensemble forecasts end to end on the tiny random models of tests/test_generate_cycles_gpu.py (one prompt cycle, two
forecast cycles): MyTransformerDecoder.sample_ids against generate_ids on the repeated prompt -- the test of the cache
fan-out and of the row numbering --, arcweld.generate.forecast_cycles' likelihoods against score_ids, its statistics
against tests/ensemble_refs.py applied to its own x_hat (the tolerances of tests/test_ensemble_stats_gpu.py), the
single-sample case against continue_cycles, bf16 shapes, and forecast_welding_cycles.py's .npz."""
import numpy as np
import pytest
import torch

import ensemble_refs as R
from oracle import gen
from oracle import vqvae as ov

pytestmark = pytest.mark.gpu

KW = dict(hidden_dim=64, num_embeddings=32, embedding_dim=16, n_resblocks=2, patch_size=25)
S, L, C, KC, N_CYCLES, C_PROMPT, B = 16, 200, 2, 32, 3, 1, 2
F = N_CYCLES - C_PROMPT
N_NEW = F * S
LOGP_TOL = 4e-4        # generated against scored log-probabilities: tests/test_generate_logp_gpu.py's bound per id
RTOL, ATOL = 1e-6, 1e-7


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
    x = torch.tensor(gen.randint(2604, (B, 1 + C_PROMPT * S), 0, KC), device="cuda")
    x[:, 0] = KC
    return x


def _prompt():
    return torch.tensor(gen.windows(2603, B * C_PROMPT).reshape(B, C_PROMPT * L, C), device="cuda")


def _truth():
    return torch.tensor(gen.windows(2605, B * F).reshape(B, F * L, C), device="cuda")


@pytest.fixture(scope="module")
def forecast(models):
    """One forecast with a truth, shared (and left unchanged) by the tests that read it."""
    from arcweld.generate import forecast_cycles
    from arcweld.precision import operands
    v, d = models
    with operands(torch.float32):
        return forecast_cycles(v, d, _prompt(), N_CYCLES, 6, quantiles=(0.0, 0.05, 0.5, 0.95, 1.0), x_true=_truth(),
                               seed=11)


def test_sample_ids_is_generate_ids_on_the_repeated_prompt(models, fp32):
    _, d = models
    x = _start_ids()
    N, kw = 5, dict(top_k=12, top_p=0.9, temperature=0.8, valid_ids=KC, seed=3)
    got = d.sample_ids(x, N_NEW, N, **kw)
    assert got.shape == (B, N, x.shape[1] + N_NEW) and got.dtype == torch.int64
    want = d.generate_ids(x.repeat_interleave(N, 0), N_NEW, do_sample=True, **kw)
    assert torch.equal(got.view(B * N, -1), want)
    assert torch.equal(got[:, :, :x.shape[1]], x[:, None, :].expand(B, N, -1))
    ids, lp = d.sample_ids(x, N_NEW, N, return_logp=True, **kw)
    wids, wlp = d.generate_ids(x.repeat_interleave(N, 0), N_NEW, do_sample=True, return_logp=True, **kw)
    assert torch.equal(ids, got) and torch.equal(wids, want)
    for k in ("logp", "logq"):
        assert lp[k].shape == (B, N, N_NEW) and lp[k].dtype == torch.float32
        err = (lp[k].view(B * N, N_NEW) - wlp[k]).abs().max().item()
        print(f"{k}: max |sample_ids - generate_ids| = {err:.2e}")
        assert err <= LOGP_TOL
    # the plain launch (no nucleus, no logp) and the edges of the call
    assert torch.equal(d.sample_ids(x, N_NEW, 3, valid_ids=KC, seed=9).view(B * 3, -1),
                       d.generate_ids(x.repeat_interleave(3, 0), N_NEW, do_sample=True, valid_ids=KC, seed=9))
    assert d.sample_ids(x, 0, 4).shape == (B, 4, x.shape[1])
    one, lp1 = d.sample_ids(x, 1, 4, valid_ids=KC, return_logp=True)          # a single token: no fan-out of the cache
    assert one.shape == (B, 4, x.shape[1] + 1) and lp1["logp"].shape == (B, 4, 1)
    assert torch.equal(one.view(B * 4, -1), d.generate_ids(x.repeat_interleave(4, 0), 1, do_sample=True, valid_ids=KC))


def test_samples_of_one_prompt_differ(models, fp32):
    """A condition on the inputs, checked first: seed 5 is one at which generate_ids on the prompt repeated 8 times
    already gives at least two distinct rows (temperature 1, no filter, 32 draws per row)."""
    _, d = models
    x = _start_ids()[:1]
    rep = d.generate_ids(x.repeat_interleave(8, 0), N_NEW, do_sample=True, valid_ids=KC, seed=5)
    assert len({tuple(r.tolist()) for r in rep}) >= 2                         # the precondition
    got = d.sample_ids(x, N_NEW, 8, valid_ids=KC, seed=5)
    assert len({tuple(r.tolist()) for r in got[0]}) >= 2
    assert torch.equal(got[0], rep)


def test_forecast_shapes_and_dtypes(forecast):
    N, Q = 6, 5
    want = {"ids": ((B, N, N_CYCLES * S), torch.int64), "x_prompt_hat": ((B, C_PROMPT * L, C), torch.float32),
            "x_hat": ((B, N, F * L, C), torch.float32), "sample_cycle_nll": ((B, N, F), torch.float32),
            "mean": ((B, F * L, C), torch.float32), "std": ((B, F * L, C), torch.float32),
            "quantiles": ((B, Q, F * L, C), torch.float32), "crps": ((B, F), torch.float32),
            "coverage": ((B, F), torch.float32)}
    assert set(forecast) == set(want)
    for k, (shape, dt) in want.items():
        assert tuple(forecast[k].shape) == shape and forecast[k].dtype == dt, k
    ids = forecast["ids"]
    assert (ids >= 0).all() and (ids < KC).all()
    assert torch.isfinite(forecast["crps"]).all() and (forecast["crps"] > 0).all()
    cov = forecast["coverage"]
    assert ((cov >= 0) & (cov <= 1)).all()


def test_sample_cycle_nll_is_on_score_ids_scale(models, fp32, forecast):
    _, d = models
    ids = forecast["ids"]
    N = ids.shape[1]
    seq = torch.cat([torch.full_like(ids.view(B * N, -1)[:, :1], KC), ids.view(B * N, -1)], dim=1)
    logp = d.score_ids(seq, valid_ids=KC)["logp"][:, C_PROMPT * S:]
    want = -logp.reshape(B, N, F, S).sum(-1)
    err = (forecast["sample_cycle_nll"] - want).abs().max().item()
    print(f"max |sample_cycle_nll - scored| = {err:.2e}")
    assert err <= LOGP_TOL * S


def test_forecast_statistics_are_those_of_its_own_samples(forecast):
    q = (0.0, 0.05, 0.5, 0.95, 1.0)
    N = forecast["x_hat"].shape[1]
    M, seg = F * L * C, L * C
    x = forecast["x_hat"].cpu().numpy().reshape(B, N, M)
    y = _truth().cpu().numpy().reshape(B, M)
    close = lambda got, want: bool((np.abs(got.astype(np.float64) - want) <= ATOL + RTOL * np.abs(want)).all())  # noqa: E731
    mean, std = R.mean_std(x)
    assert close(forecast["mean"].cpu().numpy().reshape(B, M), mean)
    assert close(forecast["std"].cpu().numpy().reshape(B, M), std)
    got = forecast["quantiles"].cpu().numpy().reshape(B, len(q), M)
    want = R.quantiles(x, q)
    exact = R.quantile_is_order_statistic(N, q)
    assert exact.tolist() == [True, False, False, False, True]
    assert np.array_equal(got[:, exact].view(np.uint32), want[:, exact].astype(np.float32).view(np.uint32))
    lo, hi = R.quantile_neighbours(x, q)
    ulp = np.spacing(np.maximum(np.abs(lo), np.abs(hi)).astype(np.float32)).astype(np.float64)
    assert (np.abs(got.astype(np.float64) - want)[:, ~exact] <= 2.0 * ulp[:, ~exact]).all()
    assert close(forecast["crps"].cpu().numpy(), R.segment_mean(R.crps_pairwise(x, y), seg))
    cover = R.coverage(got[:, 0], got[:, -1], y, seg).astype(np.float32)
    assert np.array_equal(forecast["coverage"].cpu().numpy(), cover)
    # q = 0 and q = 1 are the pointwise extremes of the samples: nothing lies outside them
    assert np.array_equal(got[:, 0], x.min(axis=1)) and np.array_equal(got[:, -1], x.max(axis=1))


def test_prompt_reconstruction_and_prompt_ids(models, fp32, forecast):
    v, _ = models
    xp = _prompt()
    pid = v.encode_ids(xp)
    assert torch.equal(forecast["x_prompt_hat"], v.decode_ids(pid))
    N = forecast["ids"].shape[1]
    assert torch.equal(forecast["ids"][:, :, :C_PROMPT * S], pid[:, None, :].expand(B, N, -1))


def test_one_sample_is_continue_cycles_sampled(models, fp32):
    from arcweld.generate import continue_cycles, forecast_cycles
    v, d = models
    xp = _prompt()
    kw = dict(top_k=10, temperature=0.9, seed=21)
    one = forecast_cycles(v, d, xp, N_CYCLES, 1, quantiles=(0.5,), **kw)
    want = continue_cycles(v, d, xp, N_CYCLES, do_sample=True, **kw)
    assert torch.equal(one["ids"][:, 0], want["ids"])
    assert torch.equal(one["x_hat"][:, 0], want["x_hat"][:, C_PROMPT * L:])
    assert torch.equal(one["x_prompt_hat"], want["x_hat"][:, :C_PROMPT * L])
    # one sample: the mean and every quantile are that sample, the spread is zero
    assert torch.equal(one["mean"], one["x_hat"][:, 0]) and torch.equal(one["quantiles"][:, 0], one["x_hat"][:, 0])
    assert not one["std"].any() and "crps" not in one and "coverage" not in one


def test_bf16_runs_and_keeps_the_shapes(models):
    from arcweld.generate import forecast_cycles
    v, d = models
    out = forecast_cycles(v, d, _prompt(), N_CYCLES, 3, x_true=_truth(), dtype=torch.bfloat16, seed=2)
    assert out["ids"].shape == (B, 3, N_CYCLES * S) and out["ids"].dtype == torch.int64
    assert out["x_hat"].shape == (B, 3, F * L, C) and out["x_hat"].dtype == torch.float32
    assert out["x_prompt_hat"].shape == (B, C_PROMPT * L, C) and out["x_prompt_hat"].dtype == torch.float32
    assert out["quantiles"].shape == (B, 3, F * L, C) and out["mean"].shape == out["std"].shape == (B, F * L, C)
    assert out["crps"].shape == out["coverage"].shape == (B, F) and out["sample_cycle_nll"].shape == (B, 3, F)
    assert all(t.dtype == torch.float32 for k, t in out.items() if k != "ids")


def test_script_writes_the_forecast(models, fp32, tmp_path):
    """forecast_welding_cycles.py end to end, in this process as the sibling scripts' tests run theirs: both models
    through load_from_checkpoint, synthetic cycles, --truth, the .npz."""
    import forecast_welding_cycles as fwc
    v, d = models
    v.save_checkpoint(str(tmp_path / "v.ckpt"))
    d.save_checkpoint(str(tmp_path / "d.ckpt"))
    out = tmp_path / "forecast.npz"
    N, n = 4, 2
    fwc.main(fwc.parser().parse_args(["--vqvae-model", str(tmp_path / "v.ckpt"), "--transformer-model",
                                      str(tmp_path / "d.ckpt"), "--n-cycles", str(N_CYCLES), "--prompt-cycles",
                                      str(C_PROMPT), "--n-seqs", str(n), "--seed", "4", "--num-samples", str(N),
                                      "--quantiles", "0.1,0.9", "--truth", "--top-p", "0.95", "--out", str(out)]))
    want = {"prompt": (n, C_PROMPT * L, C), "x_true": (n, F * L, C), "q": (2,), "ids": (n, N, N_CYCLES * S),
            "x_prompt_hat": (n, C_PROMPT * L, C), "x_hat": (n, N, F * L, C), "sample_cycle_nll": (n, N, F),
            "mean": (n, F * L, C), "std": (n, F * L, C), "quantiles": (n, 2, F * L, C), "crps": (n, F),
            "coverage": (n, F)}
    with np.load(out, allow_pickle=False) as f:
        assert set(f.files) == set(want)
        for k, shape in want.items():
            assert f[k].shape == shape, k
            assert f[k].dtype == (np.int64 if k == "ids" else np.float32), k
        assert (f["ids"] >= 0).all() and (f["ids"] < KC).all() and np.isfinite(f["crps"]).all()
        assert (f["quantiles"][:, 0] <= f["quantiles"][:, 1]).all()
    # without --truth: no score, no truth
    fwc.main(fwc.parser().parse_args(["--vqvae-model", str(tmp_path / "v.ckpt"), "--transformer-model",
                                      str(tmp_path / "d.ckpt"), "--n-cycles", str(N_CYCLES), "--prompt-cycles",
                                      str(C_PROMPT), "--n-seqs", str(n), "--seed", "4", "--num-samples", str(N),
                                      "--out", str(out)]))
    with np.load(out, allow_pickle=False) as f:
        assert set(f.files) == set(want) - {"x_true", "crps", "coverage"} and f["quantiles"].shape[1] == 3
