"""CPU-side checks of the weld-quality classifier (train_classification_model.py, model/gru.py,
model/classification_model.py, the classification data module): flags, state-dict layout, checkpoint round trip,
the torch restatements of the torchmetrics calls, the sampler weights and the latent flattening order."""
import numpy as np
import pytest
import torch

from conftest import golden


def test_reference_flags_and_defaults():
    import train_classification_model as tcm
    a = tcm.parser().parse_args([])
    assert (a.epochs, a.batch_size, a.hidden_dim, a.learning_rate, a.clipping_value, a.dropout_p, a.n_hidden_layer,
            a.model_name, a.dataset, a.n_cycles) == (30, 512, 758, 0.001, 0.42, 0.032015121309774644, 6, "GRU",
                                                     "asimow", 5)
    assert a.vqvae_model == "model_checkpoints/VQ-VAE-Patch/vq_vae_patch_best_02.ckpt"
    assert a.use_wandb is None and a.use_mlflow is None and a.mlflow_url is None
    assert a.logging_entity is None and a.logging_project is None and a.logging_tag is None
    assert (a.data_npz, a.seed, a.precision) == ("", 0, "fp32")
    assert callable(tcm.main)


def test_mlp_is_refused_with_a_clear_message():
    import train_classification_model as tcm
    with pytest.raises(SystemExit, match="not built yet"):
        tcm.main(tcm.parser().parse_args(["--model-name", "MLP"]))
    with pytest.raises(SystemExit, match="W&B / MLflow"):
        tcm.main(tcm.parser().parse_args(["--use-wandb"]))


def test_state_dict_matches_fixture_and_torch_gru():
    from model.gru import GRU
    m = GRU(input_size=3, in_dim=12, hidden_sizes=20, n_hidden_layers=2, output_size=2, dropout_p=0.0)
    sd = m.state_dict()
    g = golden("gru_small.npz")
    keys = [str(k) for k in g["state_keys"]]
    assert sorted(sd) == keys
    for k, shp in zip(keys, g["state_shapes"]):
        assert tuple(sd[k].shape) == tuple(int(v) for v in shp[:sd[k].dim()]), k
    ref = {"gru." + k: v for k, v in torch.nn.GRU(12, 20, 2, batch_first=True).state_dict().items()}
    ref.update({"output_layer." + k: v for k, v in torch.nn.Linear(20, 2).state_dict().items()})
    assert list(sd) == list(ref)                       # same names in the same registration order
    assert all(sd[k].shape == ref[k].shape and sd[k].dtype == ref[k].dtype for k in ref)
    m.load_state_dict(ref, strict=True)


def test_initialisation_is_torchs():
    """Same seed, same draws as nn.GRU followed by nn.Linear (U(-1/sqrt(H), 1/sqrt(H)) per tensor, in order)."""
    from model.gru import GRU
    torch.manual_seed(7)
    m = GRU(input_size=3, in_dim=12, hidden_sizes=20, n_hidden_layers=2, output_size=2)
    torch.manual_seed(7)
    g, lin = torch.nn.GRU(12, 20, 2, batch_first=True), torch.nn.Linear(20, 2)
    for k, v in g.state_dict().items():
        assert torch.equal(m.state_dict()["gru." + k], v), k
    assert torch.equal(m.output_layer.weight, lin.weight) and torch.equal(m.output_layer.bias, lin.bias)


def test_checkpoint_round_trip(tmp_path):
    from model.gru import GRU
    torch.manual_seed(3)
    m = GRU(input_size=4, in_dim=10, hidden_sizes=12, n_hidden_layers=3, output_size=2, dropout_p=0.25,
            learning_rate=0.5, model_id="abc")
    assert m.model_id == "abc/"
    hp = dict(m.hparams)
    assert hp == dict(input_size=4, in_dim=10, output_size=2, hidden_sizes=12, n_hidden_layers=3, dropout_p=0.25,
                      learning_rate=0.5, model_id="abc", warmup=150, max_iters=10_000)
    path = str(tmp_path / "gru.ckpt")
    m.save_checkpoint(path)
    r = GRU.load_from_checkpoint(path)
    assert dict(r.hparams) == hp and r.model_id == "abc/" and r.dropout.p == 0.25
    assert list(r.state_dict()) == list(m.state_dict())
    for k, v in m.state_dict().items():
        assert torch.equal(r.state_dict()[k], v), k


def _metrics(preds, target):
    from model.classification_model import binary_f1, class_accuracy, multiclass_accuracy
    p, t = torch.tensor(preds), torch.tensor(target)
    return (float(multiclass_accuracy(p, t)), float(class_accuracy(p, t, 1)), float(class_accuracy(p, t, 0)),
            float(binary_f1(p, t)))


def test_metric_restatements():
    assert _metrics([0, 1, 1, 0], [0, 1, 1, 0]) == (1.0, 1.0, 1.0, 1.0)            # all correct
    assert _metrics([1, 0, 0, 1], [0, 1, 1, 0]) == (0.0, 0.0, 0.0, 0.0)            # all wrong
    # no positive labels: F1's denominator is FP only (or 0): F1 = 0, acc_good of the empty class = 0
    assert _metrics([0, 0, 0], [0, 0, 0]) == (1.0, 0.0, 1.0, 0.0)
    acc, good, bad, f1 = _metrics([0, 1, 0], [0, 0, 0])
    assert (good, f1) == (0.0, 0.0) and acc == pytest.approx(2 / 3) and bad == pytest.approx(2 / 3)
    # by hand: target 1 1 1 0 0 0 1 0, preds 1 0 1 1 0 0 1 1 -> TP 3, FP 2, FN 1, TN 2
    acc, good, bad, f1 = _metrics([1, 0, 1, 1, 0, 0, 1, 1], [1, 1, 1, 0, 0, 0, 1, 0])
    assert acc == pytest.approx(5 / 8) and good == pytest.approx(3 / 4) and bad == pytest.approx(2 / 4)
    assert f1 == pytest.approx(2 * 3 / (2 * 3 + 2 + 1))


def test_epoch_end_hooks_and_log_keys():
    """The step methods log the reference's keys; the hooks keep the four summary attributes."""
    from model.classification_model import ClassificationLightningModule

    class Fixed(ClassificationLightningModule):
        def __init__(self):
            super().__init__(input_size=1, output_size=2, in_dim=2, hidden_sizes=4, model_id="m")
            self.w = torch.nn.Parameter(torch.zeros(1))

        def forward(self, x):
            return x + self.w

    m = Fixed()
    x = torch.tensor([[2.0, 0.0], [0.0, 2.0], [2.0, 0.0], [0.0, 2.0]])       # predictions 0 1 0 1
    y = torch.tensor([0, 1, 1, 1])
    m.training_step((x, y), 0)
    assert sorted(m.logged) == [f"m/train/{k}" for k in ("acc", "acc_bad", "acc_good", "f1_score", "loss")]
    m._logged = {}
    m.validation_step((x, y), 0)
    assert sorted(m.logged) == [f"m/val/{k}" for k in ("acc", "acc_bad", "acc_good", "f1_score", "loss")]
    assert m.logged["m/val/acc"] == pytest.approx(0.75) and m.logged["m/val/f1_score"] == pytest.approx(0.8)
    m.validation_step((x, torch.tensor([0, 1, 0, 1])), 1)
    m._logged = {}
    m.on_validation_epoch_end()
    assert sorted(m.logged) == ["m/val/acc_mean", "m/val/f1_score_mean"]
    assert m.hyper_search_value == pytest.approx(0.9) and m.val_acc_score == pytest.approx(0.875)
    assert m.val_f1_scores == [] and m.val_acc_scores == []
    m._logged = {}
    m.test_step((x, y), 0)
    assert sorted(m.logged) == [f"m/test/{k}" for k in ("acc", "acc_bad", "acc_good", "f1_score", "loss")]
    m._logged = {}
    m.on_test_epoch_end()
    assert list(m.logged) == ["m/test/f1_score_mean"]
    assert m.test_f1_score == pytest.approx(0.8) and m.test_acc_score == pytest.approx(0.75)
    from arcweld.optim import RAdam
    assert RAdam.__name__ == "RAdam" and ClassificationLightningModule.configure_optimizers is not None


def test_trainer_folds_epoch_end_metrics():
    """Trainer.evaluate calls the epoch-end hook and returns what it logged beside the per-batch means."""
    from arcweld.lightning import LightningModule
    from arcweld.trainer import Trainer

    class M(LightningModule):
        def __init__(self):
            super().__init__()
            self.w = torch.nn.Parameter(torch.zeros(1))
            self.seen = []

        def validation_step(self, batch, i):
            self.seen.append(float(batch[0].sum()))
            self.log("val/loss", float(batch[0].sum()))

        def on_validation_epoch_end(self):
            self.log("val/f1_score_mean", sum(self.seen) / len(self.seen))

        def test_step(self, batch, i):
            self.log("test/loss", 1.0)

    m = M()
    batches = [(torch.ones(2, 1), torch.zeros(2)), (3 * torch.ones(2, 1), torch.zeros(2))]
    out = Trainer(devices=1).evaluate(m, batches, "val")
    assert out == {"val/loss": pytest.approx(4.0), "val/f1_score_mean": pytest.approx(4.0)}
    assert Trainer(devices=1).evaluate(m, batches, "test") == {"test/loss": pytest.approx(1.0)}     # no test hook


def test_sampler_weights_and_weighted_batches():
    from arcweld.data import WeightedBatches, class_sampling_weights
    y = torch.tensor([0, 0, 0, 1, 0, 1, 0, 0])
    w = class_sampling_weights(y)
    ratio = 6 / 8
    assert torch.allclose(w, torch.where(y == 0, torch.tensor(1 - ratio), torch.tensor(ratio)).float())
    x = torch.arange(8).float().view(8, 1)
    ld = WeightedBatches((x, y), w, batch_size=3, seed=1)
    assert len(ld) == 3
    got = list(ld)
    assert [len(b[0]) for b in got] == [3, 3, 2]
    idx = torch.cat([b[0].view(-1) for b in got]).long()
    assert torch.equal(torch.cat([b[1] for b in got]), y[idx])           # samples and labels stay paired
    assert torch.equal(idx, ld.indices())                                # one epoch = n draws with replacement
    ld.set_epoch(1)
    assert not torch.equal(ld.indices(), idx)
    # weight 0 is never drawn; both classes carry the same total weight (2 * 0.75 = 6 * 0.25)
    only1 = WeightedBatches((x, y), torch.where(y == 1, 1.0, 0.0), batch_size=8)
    assert set(next(iter(only1))[1].tolist()) == {1}
    assert float(w[y == 0].sum()) == pytest.approx(float(w[y == 1].sum()))


class _FakeVQVAE:
    """Identity-like stages: z_q[b, d, s] = x[b, s, d] (the permute of the non-patch reference path), D = 2."""
    embedding_dim, enc_out_len = 2, 3

    def patch_embed(self, x):
        return x.permute(0, 2, 1)

    def encoder(self, x):
        return x

    def vector_quantization(self, z):
        return None, z, None, None, None


def test_latent_flattening_order():
    from arcweld.data import ClassificationDataModule, latent_vectors
    n, nc, L, C = 4, 2, 3, 2
    x = torch.arange(n * nc * L * C).float().view(n, nc * L, C)
    z = latent_vectors(_FakeVQVAE(), x, nc, window=L)
    assert z.shape == (n, nc, 6)
    for b in range(n):
        for i in range(nc):
            win = x[b, i * L:(i + 1) * L]                     # (L, C) -> z_q (D = C, S = L) -> reshape(-1): d-major
            assert torch.equal(z[b, i], win.t().reshape(-1))
    y = torch.tensor([0, 1, 0, 0])
    dm = ClassificationDataModule([(x, y)] * 3, batch_size=3, n_cycles=nc, dataset="latent_vq_vae", vqvae=_FakeVQVAE(),
                                  window=L)
    assert dm.in_dim == 6
    dm.setup("fit")
    xb, yb = next(iter(dm.val_dataloader()))
    assert torch.equal(xb, z[:3]) and torch.equal(yb, y[:3])               # sequential, (B, n_cycles, in_dim)
    assert [len(b[0]) for b in dm.test_dataloader()] == [3, 1]
    raw = ClassificationDataModule([(x, y)] * 3, batch_size=4, n_cycles=nc, dataset="asimow", window=L)
    raw.setup("fit")
    assert raw.in_dim == 2 * L and torch.equal(next(iter(raw.val_dataloader()))[0], x)
    assert len(raw.train_dataloader()) == 1
    with pytest.raises(ValueError):
        ClassificationDataModule([(x, y)] * 3, dataset="ts2vec")


def test_fixture_is_small_and_complete():
    g = golden("gru_small.npz")
    assert g["logits"].shape == (6, 2) and np.isfinite(g["loss"])
    assert all("grad/" + str(k) in g.files for k in g["state_keys"])
