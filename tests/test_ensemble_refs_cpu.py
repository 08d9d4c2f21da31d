"""The ensemble-forecast surface without a GPU: the fp64 restatements the GPU tests lean on (the pairwise CRPS against
the sorted form the kernel evaluates), forecast_welding_cycles.py's flags, and the argument checks of sample_ids /
forecast_cycles that come before any device work (CPU tensors throughout: any launch would raise NativeError)."""
import numpy as np
import pytest
import torch

import ensemble_refs as R


@pytest.mark.parametrize("N", [1, 2, 3, 7, 32, 64])
def test_pairwise_crps_equals_the_sorted_form(N):
    rng = np.random.default_rng(7100 + N)
    x = rng.normal(size=(3, N, 41)).astype(np.float32)
    y = rng.normal(size=(3, 41)).astype(np.float32)
    assert np.abs(R.crps_pairwise(x, y) - R.crps_sorted(x, y)).max() <= 1e-12
    if N >= 2:                                   # ties: duplicated pairs, then every sample equal
        x[:, 1] = x[:, 0]
        x[:, N - 1] = x[:, N // 2]
        assert np.abs(R.crps_pairwise(x, y) - R.crps_sorted(x, y)).max() <= 1e-12
    x[:] = x[:, :1]
    c = R.crps_pairwise(x, y)
    assert np.abs(c - R.crps_sorted(x, y)).max() <= 1e-12
    assert np.abs(c - np.abs(x[:, 0].astype(np.float64) - y)).max() <= 1e-12      # no spread: the absolute error


def test_single_sample_statistics():
    x = np.array([[[1.5, -2.0, 0.25]]], dtype=np.float32)
    mean, std = R.mean_std(x)
    assert np.array_equal(mean, x[:, 0]) and not std.any()
    q = R.quantiles(x, [0.0, 0.3, 1.0])
    assert q.shape == (1, 3, 3) and all(np.array_equal(q[:, k], x[:, 0]) for k in range(3))
    assert R.quantile_is_order_statistic(1, [0.0, 0.3, 1.0]).all()
    assert R.quantile_is_order_statistic(3, [0.0, 0.5, 1.0]).all()
    assert not R.quantile_is_order_statistic(32, [0.05, 0.5, 0.95]).any()


def test_coverage_counts_the_closed_band():
    lo, hi = np.zeros((1, 6)), np.ones((1, 6))
    y = np.array([[0.0, 1.0, 0.5, -0.1, 1.1, 0.2]])
    assert R.coverage(lo, hi, y, 3).tolist() == [[1.0, 1 / 3]]


def test_forecast_flags_parse_with_their_defaults():
    import forecast_welding_cycles as fwc
    a = fwc.parser().parse_args([])
    assert (a.n_cycles, a.prompt_cycles, a.n_seqs, a.data_npz, a.seed, a.precision) == (20, 10, 16, "", 0, "fp32")
    assert (a.num_samples, a.quantiles, a.truth, a.out) == (16, (0.05, 0.5, 0.95), False, "forecast_cycles.npz")
    assert (a.top_k, a.top_p, a.min_p, a.temperature) == (None, None, None, 1.0)
    assert a.vqvae_model.endswith(".ckpt") and a.transformer_model == ""
    b = fwc.parser().parse_args(["--num-samples", "4", "--quantiles", "0.1,0.9", "--truth", "--top-k", "5",
                                 "--precision", "bf16"])
    assert (b.num_samples, b.quantiles, b.truth, b.top_k, b.precision) == (4, (0.1, 0.9), True, 5, "bf16")
    with pytest.raises(SystemExit):
        fwc.parser().parse_args(["--quantiles", "0.1,x"])
    with pytest.raises(SystemExit):
        fwc.parser().parse_args(["--do-sample"])                 # a forecast always samples: no such flag
    assert callable(fwc.main)


def _decoder(**kw):
    from model.transformer_decoder import MyTransformerDecoder
    args = dict(d_model=16, n_classes=6, seq_len=33, n_blocks=1, n_head=2)
    args.update(kw)
    return MyTransformerDecoder(**args)


def _vqvae():
    from model.vq_vae_patch_embedd import VQVAEPatch
    return VQVAEPatch(hidden_dim=8, input_dim=2, num_embeddings=4, embedding_dim=4, n_resblocks=1, learning_rate=1e-3,
                      batch_norm=False)                           # S = 16 ids per window of 200 x 2


def test_sample_ids_checks_its_arguments_before_touching_the_device():
    d = _decoder()
    x = torch.zeros(2, 17, dtype=torch.int64)
    for n in (0, 33, -1):
        with pytest.raises(ValueError, match="num_samples"):
            d.sample_ids(x, 4, n)
    with pytest.raises(ValueError, match="int64 ids of shape"):
        d.sample_ids(x.int(), 4, 2)
    with pytest.raises(ValueError, match="seq_len"):
        d.sample_ids(x, 17, 2)
    with pytest.raises(ValueError, match="top_k"):
        d.sample_ids(x, 4, 2, top_k=5, valid_ids=4)
    with pytest.raises(ValueError, match="top_p"):
        d.sample_ids(x, 4, 2, top_p=0.0)
    with pytest.raises(ValueError, match="min_p"):
        d.sample_ids(x, 4, 2, min_p=1.0)
    with pytest.raises(ValueError, match="temperature"):
        d.sample_ids(x, 4, 2, temperature=0.0)
    with pytest.raises(ValueError, match="valid_ids"):
        d.sample_ids(x, 4, 2, valid_ids=7)


def test_forecast_cycles_checks_its_arguments_before_touching_the_device():
    from arcweld.generate import forecast_cycles
    v, d = _vqvae(), _decoder()                                   # two cycles of 16 ids + the start token
    xp = torch.zeros(2, 200, 2)
    for n in (0, 33):
        with pytest.raises(ValueError, match="num_samples"):
            forecast_cycles(v, d, xp, 2, n)
    with pytest.raises(ValueError, match="quantiles"):
        forecast_cycles(v, d, xp, 2, 4, quantiles=(0.9, 0.5, 0.1))                    # descending
    with pytest.raises(ValueError, match="quantiles"):
        forecast_cycles(v, d, xp, 2, 4, quantiles=tuple(i / 10 for i in range(9)))    # nine
    with pytest.raises(ValueError, match="quantiles"):
        forecast_cycles(v, d, xp, 2, 4, quantiles=(0.5, 1.5))
    with pytest.raises(ValueError, match="quantiles"):
        forecast_cycles(v, d, xp, 2, 4, quantiles=(float("nan"),))
    for bad in (torch.zeros(2, 400, 2), torch.zeros(3, 200, 2), torch.zeros(2, 200, 3), torch.zeros(2, 200, 2).double(),
                torch.zeros(2, 200)):
        with pytest.raises(ValueError, match="x_true must be"):
            forecast_cycles(v, d, xp, 2, 4, x_true=bad)
    with pytest.raises(ValueError, match="at least two quantiles"):
        forecast_cycles(v, d, xp, 2, 4, quantiles=(0.5,), x_true=torch.zeros(2, 200, 2))
    with pytest.raises(ValueError, match=r"n_classes 7.*= 6"):
        forecast_cycles(v, _decoder(n_classes=7), xp, 2, 4)
    with pytest.raises(ValueError, match="prompt"):
        forecast_cycles(v, d, torch.zeros(2, 400, 2), 2, 4)       # c == n_cycles: nothing left to forecast
