"""Weld-quality classifier training -- drop-in for the reference's train_classification_model.py.

Same flags, defaults and flow: fit the GRU with ModelCheckpoint + EarlyStopping on ``val/f1_score_mean`` (max,
min_delta 0.001, patience 5), gradient_clip_val = ``--clipping-value``, reload the best checkpoint, test, and log
val/mean_f1_score, val/mean_acc, test/mean_f1_score, test/mean_acc.  ``--dataset asimow`` trains on the raw
current / voltage cycles ((B, n_cycles, 400) per batch), ``--dataset latent_vq_vae`` on the latent vectors of the frozen
VQ-VAE given by ``--vqvae-model`` -- the reference's measure of how good a trained VQ-VAE's latent space is.

Data: synthetic welding sequences of n_cycles 200x2 windows with random labels, or ``--data-npz`` with real windows
('train'/'val'/'test' of shape (n, n_cycles*200, 2) and '<split>_labels').  W&B / MLflow are not available (CSVLogger
only).  ``--precision`` picks the MFMA operand dtype (fp32 default, bf16 opt-in; arcweld.precision).  The MLP
classifier (``--model-name MLP``) is not built yet.
"""
import argparse
import logging as log
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import torch  # noqa: E402

from arcweld.data import ClassificationDataModule  # noqa: E402
from arcweld.launch import CSVLogger  # noqa: E402
from arcweld.precision import set_operand_dtype  # noqa: E402
from arcweld.trainer import EarlyStopping, ModelCheckpoint, Trainer  # noqa: E402
from model.gru import GRU  # noqa: E402
from train_transformer_mtasks import load_splits, load_vqvae  # noqa: E402


def main(hparams):
    if hparams.use_wandb or hparams.use_mlflow:
        raise SystemExit("W&B / MLflow are not available in this build (no network); use the CSV logger")
    model_name, dataset = hparams.model_name, hparams.dataset
    classification_model = model_name.split("-")[0]
    if classification_model == "MLP":
        raise SystemExit("--model-name MLP: the MLP classifier is not built yet in this build; use GRU")
    if classification_model != "GRU":
        raise ValueError(f"Classification model name: {classification_model} not supported")
    if dataset not in ("asimow", "latent_vq_vae"):
        raise ValueError(f"Invalid dataset name. {dataset} not supported")
    set_operand_dtype(hparams.precision)
    dev = torch.device("cuda", torch.cuda.current_device())
    logger = CSVLogger("logs", name="vq-vae-transformer")
    logger.log_hyperparams(vars(hparams))

    vqvae = load_vqvae(hparams.vqvae_model, dev) if dataset == "latent_vq_vae" else None
    data_module = ClassificationDataModule(load_splits(hparams, dev), batch_size=hparams.batch_size,
                                           n_cycles=hparams.n_cycles, dataset=dataset, vqvae=vqvae, seed=hparams.seed)
    seq_len, input_dim = hparams.n_cycles, data_module.in_dim
    log.info(f"{seq_len=} - {input_dim=} - {dataset=}")

    torch.manual_seed(hparams.seed)
    model = GRU(input_size=seq_len, in_dim=input_dim, hidden_sizes=hparams.hidden_dim, dropout_p=hparams.dropout_p,
                n_hidden_layers=hparams.n_hidden_layer, output_size=2, learning_rate=hparams.learning_rate).to(dev)

    checkpoint_callback = ModelCheckpoint(dirpath="model_checkpoints", monitor="val/f1_score_mean", mode="max",
                                          filename=f"{model_name}-{dataset}-best")
    early_stop_callback = EarlyStopping(monitor="val/f1_score_mean", min_delta=0.001, patience=5, verbose=False,
                                        mode="max")
    trainer = Trainer(max_epochs=hparams.epochs, logger=logger, callbacks=[checkpoint_callback, early_stop_callback],
                      devices=1, num_nodes=1, gradient_clip_val=hparams.clipping_value)
    trainer.fit(model=model, datamodule=data_module)

    best_score = model.hyper_search_value
    best_acc_score = model.val_acc_score
    print(f"best score: {best_score}")
    print("------ Testing ------")

    trainer = Trainer(devices=1, num_nodes=1, logger=logger)
    model = GRU.load_from_checkpoint(checkpoint_callback.best_model_path, map_location=dev)
    res = trainer.test(model=model, datamodule=data_module)
    logdict = {"val/mean_f1_score": float(best_score), "val/mean_acc": float(best_acc_score),
               "test/mean_f1_score": float(model.test_f1_score), "test/mean_acc": float(model.test_acc_score)}
    logger.log_metrics(logdict, step=trainer.global_step)
    print("test:", res)
    return res[0]


def parser():
    p = argparse.ArgumentParser(description='Train Classification Model')
    p.add_argument('--epochs', type=int, help='Number of epochs to train', default=30)
    p.add_argument('--batch-size', type=int, help='Batch size', default=512)
    p.add_argument('--hidden-dim', type=int, help='Hidden dimension', default=758)
    p.add_argument('--learning-rate', type=float, help='Learning rate', default=0.001)
    p.add_argument('--clipping-value', type=float, help='Gradient Clipping', default=0.42)
    p.add_argument('--dropout-p', type=float, help='Dropout propability', default=0.032015121309774644)
    p.add_argument('--n-hidden-layer', type=int, help='Number of hidden layers', default=6)
    p.add_argument('--model-name', type=str, help='Model name', default="GRU")
    p.add_argument('--dataset', type=str, help='Dataset', default="asimow")
    p.add_argument('--n-cycles', type=int, help='Number of cycles', default=5)
    p.add_argument('--use-wandb', action=argparse.BooleanOptionalAction)
    p.add_argument('--use-mlflow', action=argparse.BooleanOptionalAction)
    p.add_argument('--mlflow-url', type=str, help='URL of the MLflow server')
    p.add_argument('--logging-entity', type=str, help='Weights and Bias or MLflow entity')
    p.add_argument('--logging-project', type=str, help='Weights and Bias or MLflow project')
    p.add_argument('--logging-tag', type=str, help='Logging Tag')
    p.add_argument('--vqvae-model', type=str, help='Model URL for wandb or Path',
                   default="model_checkpoints/VQ-VAE-Patch/vq_vae_patch_best_02.ckpt")
    # this build: synthetic data sizes, real-data .npz, seed, MFMA operand dtype
    p.add_argument('--n-train', type=int, default=1024)
    p.add_argument('--n-val', type=int, default=128)
    p.add_argument('--n-test', type=int, default=128)
    p.add_argument('--data-npz', type=str, default="")
    p.add_argument('--seed', type=int, default=0)
    p.add_argument('--precision', choices=["fp32", "bf16"], default="fp32",
                   help="MFMA operand dtype (bf16: opt-in, fp32 accumulation and master weights)")
    return p


if __name__ == '__main__':
    args = parser().parse_args()
    log.basicConfig(level=log.INFO, format='%(asctime)s - %(levelname)s - %(message)s')
    torch.set_float32_matmul_precision('medium')
    main(args)
