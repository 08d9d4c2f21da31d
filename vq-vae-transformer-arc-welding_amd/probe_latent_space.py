"""k-NN, linear or RBF-SVM probe of a latent space: how well can weld quality be read off the features, without training anything.

The train split is the database, val and test are the queries (arcweld.retrieve.latent_knn_probe): every query
sequence takes the label its ``--k`` nearest training sequences vote for, after the StandardScaler of the reference's
fit_knn protocol (``--no-standardize`` switches it off).  ``--dataset latent_vq_vae`` probes the latent vectors of the
frozen VQ-VAE given by ``--vqvae-model`` -- the features train_classification_model.py fits its GRU on --,
``--dataset asimow`` the raw current / voltage cycles.  The search runs on the device (csrc/knn.hip) and takes seconds.

Data: synthetic welding sequences of n_cycles 200x2 windows with random labels, or ``--data-npz`` in the layout
train_classification_model.py reads ('train' / 'val' / 'test' of shape (n, n_cycles*200, 2) and '<split>_labels'),
with optional '<split>_groups' (integer ids, e.g. the welding run): a query never takes a neighbour of its own group.
``--loo`` adds the train split against itself, each sequence (or, with 'train_groups', each group) left out of its own
neighbours.

``--dataset ts2vec --ts2vec-model PATH`` probes the learned baseline the protocols were written for: PATH is a checkpoint
written by the reference's ``TS2Vec.save`` (widths and depth are read from its shapes), the features are its pooled
representations ``encode(x, encoding_window='full_series')`` of every sequence (arcweld.ts2vec, csrc/ts2vec.hip): the
reference's eval_classification.  All three protocols take it; ``--out`` keeps its keys, "dataset" reads "ts2vec".

``--out`` receives the metrics as JSON: {"val" / "test" / "train_loo": {"acc", "acc_good", "acc_bad", "f1"}, "k",
"weights", "dataset", "standardize", "n_cycles"}.  ``--neighbours-out`` (optional) receives an .npz with
'<split>_idx' (n, k) int64, '<split>_dist' (n, k) f32 (squared distances; -1 / +inf past the eligible rows) and
'<split>_pred' (n,) int64 per split.

``--metric dtw`` (k-NN protocol, ``--dataset asimow`` only) replaces the sample-by-sample Euclidean distance of the raw
cycles by dynamic time warping (arcweld.retrieve.dtw_search, csrc/dtw.hip): weld cycles differ in phase and duration,
and 1-NN under DTW is the baseline a representation of time series has to beat.  ``--band F`` (0 <= F <= 1, default
0.1) is the Sakoe-Chiba band as a fraction of the sequence length L = n_cycles * 200: radius = min(L - 1,
floor(F * L)) samples, at most 224.  The scaler is then one mean and scale per channel.  ``--out`` gains "metric",
"band" and "radius"; the distances of ``--neighbours-out`` are DTW costs.

``--protocol linear`` is the reference's other protocol, fit_lr: the same StandardScaler, then an L2-regularised
logistic regression fitted on the train split (arcweld.retrieve.latent_linear_probe, csrc/logreg.hip), one per value
of ``--C``, all in the same passes over the features; ``--tol`` and ``--max-iter`` bound the fit.  ``--out`` then
receives {"val" / "test": the metrics at the selected C, "per_C": [{"C", "val", "test"}], "C_selected": the C with the
best val F1 (ties to the smaller C), "protocol", "dataset", "standardize", "n_cycles", "converged", "n_iter" (per C)}.
``--model-out`` (optional) receives an .npz with 'coef' (n_C, n_problems, D), 'intercept' (n_C, n_problems), 'mean',
'scale' (D,) and 'C' (n_C,); the coefficients live in the standardised space.  ``--neighbours-out``, ``--loo``, ``--k``
and ``--weights`` belong to the k-NN protocol.

``--protocol svm`` is the third, fit_svm: np.nan_to_num, NO scaler (``--standardize`` switches one on), then an RBF
support-vector classifier per value of ``--C`` (arcweld.retrieve.latent_svm_probe, csrc/svm.hip: one Gram matrix on
the f32 MFMA, libsvm's SMO on it), ``--gamma`` a float or ``scale`` (1 / (D var), scikit-learn's default).  ``--C``,
``--tol`` and ``--max-iter`` resolve per protocol when not given: 1.0 / 1e-4 / 1000 for linear, 0.1 / 1e-3 / 20000
(fit_svm's values) for svm.  ``--out`` then receives the linear protocol's keys plus "gamma" (the f32 value used) and
"n_support" (per C; also in every per_C entry).  ``--model-out`` receives an .npz with 'support' (n_sv,) row indices
into the fitted train rows, 'support_vectors' (n_sv, D), 'dual_coef' (n_C, n_pairs, n_sv), 'rho' (n_C, n_pairs),
'gamma', 'C' (n_C,), 'mean' and 'scale' (D,).  A train split of fewer than 50 rows, or fewer than 5 per class, is
refused (fit_svm fits those with C = inf).
"""
import argparse
import json
import logging as log
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import numpy as np  # noqa: E402
import torch  # noqa: E402

from generate_welding_cycles import require_checkpoint  # noqa: E402

METRICS = ("acc", "acc_good", "acc_bad", "f1")


def parser():
    p = argparse.ArgumentParser(description='Probe-Latent-Space')
    p.add_argument('--vqvae-model', type=str, help='Path of the VQ-VAE checkpoint',
                   default="model_checkpoints/VQ-VAE-Patch/vq_vae_patch_best_02.ckpt")
    p.add_argument('--dataset', choices=["latent_vq_vae", "asimow", "ts2vec"], default="latent_vq_vae")
    p.add_argument('--ts2vec-model', type=str, default="",
                   help="--dataset ts2vec: a checkpoint written by the reference's TS2Vec.save")
    p.add_argument('--n-cycles', type=int, help='Number of cycles', default=5)
    p.add_argument('--k', type=int, help='Neighbours per query', default=1)
    p.add_argument('--weights', choices=["uniform", "distance"], default="uniform")
    p.add_argument('--no-standardize', action='store_true', help="knn, linear: use the features as they are")
    p.add_argument('--standardize', action='store_true', help="svm: apply the scaler fit_svm does not have")
    p.add_argument('--loo', action='store_true', help="also: the train split against itself, leave-one-out")
    p.add_argument('--data-npz', type=str, default="")
    p.add_argument('--n-train', type=int, default=1024)
    p.add_argument('--n-val', type=int, default=128)
    p.add_argument('--n-test', type=int, default=128)
    p.add_argument('--seed', type=int, default=0)
    p.add_argument('--out', type=str, default="latent_probe.json")
    p.add_argument('--neighbours-out', type=str, default="")
    p.add_argument('--protocol', choices=["knn", "linear", "svm"], default="knn")
    p.add_argument('--C', type=float, nargs='+', default=None,
                   help="linear: inverse regularisation strength(s), default 1.0; svm: box constraint(s), default 0.1")
    p.add_argument('--tol', type=float, default=None,
                   help="linear: stop at max |grad F| <= tol, default 1e-4; svm: stop at m - M <= tol, default 1e-3")
    p.add_argument('--max-iter', type=int, default=None,
                   help="linear: L-BFGS iterations at most, default 1000; svm: SMO iterations per problem at most, "
                        "default 20000")
    p.add_argument('--gamma', type=gamma_arg, default="scale", help="svm: RBF width, a positive float or 'scale'")
    p.add_argument('--model-out', type=str, default="", help="linear, svm: .npz of the fitted model")
    p.add_argument('--metric', choices=["euclidean", "dtw"], default="euclidean",
                   help="knn: the distance; dtw (dynamic time warping) needs --dataset asimow")
    p.add_argument('--band', type=float, default=None,
                   help="knn, --metric dtw: the warping band as a fraction of the sequence length, 0..1, default 0.1")
    return p


DEFAULT_BAND = 0.1


def resolve_dtw(hparams):
    """{} for the Euclidean metric, {"metric": "dtw", "band", "radius"} for --metric dtw; refuses --metric and --band
    where they do not belong and values outside their ranges, before any file is read."""
    if hparams.protocol != "knn":
        if hparams.metric != "euclidean" or hparams.band is not None:
            raise SystemExit("--metric and --band belong to --protocol knn")
        return {}
    if hparams.metric != "dtw":
        if hparams.band is not None:
            raise SystemExit("--band belongs to --metric dtw")
        return {}
    if hparams.dataset == "ts2vec":
        raise SystemExit("--metric dtw warps the raw cycles and needs --dataset asimow: the pooled representations of "
                         "--dataset ts2vec are not time series")
    if hparams.dataset != "asimow":
        raise SystemExit("--metric dtw warps the raw cycles and needs --dataset asimow: the latent vectors of "
                         "--dataset latent_vq_vae are not time series")
    band = DEFAULT_BAND if hparams.band is None else hparams.band
    if not 0 <= band <= 1:
        raise SystemExit("--band must lie in 0..1 (a fraction of the sequence length)")
    if hparams.n_cycles < 1:
        raise SystemExit("--n-cycles must be at least 1")
    from arcweld.retrieve import MAX_DTW_LEN, MAX_DTW_WINDOW
    L = hparams.n_cycles * 200
    radius = min(L - 1, int(band * L))
    if L > MAX_DTW_LEN:
        raise SystemExit(f"--metric dtw holds sequences of at most {MAX_DTW_LEN} samples, --n-cycles "
                         f"{hparams.n_cycles} gives {L}")
    if 2 * radius + 1 > MAX_DTW_WINDOW:
        raise SystemExit(f"--band {band:g} of {L} samples is a radius of {radius}, --metric dtw holds at most "
                         f"{(MAX_DTW_WINDOW - 1) // 2}")
    return dict(metric="dtw", band=band, radius=radius)


PROTOCOL_DEFAULTS = {"linear": dict(C=[1.0], tol=1e-4, max_iter=1000), "svm": dict(C=[0.1], tol=1e-3, max_iter=20000)}


def gamma_arg(text):
    if text == "scale":
        return text
    try:
        return float(text)
    except ValueError:
        raise argparse.ArgumentTypeError(f"expected a float or 'scale', got {text!r}") from None


def resolve_fit_args(hparams):
    """--C, --tol and --max-iter where given, else the protocol's defaults; refuses values outside their ranges."""
    d = PROTOCOL_DEFAULTS[hparams.protocol]
    C = list(hparams.C) if hparams.C is not None else d["C"]
    tol = hparams.tol if hparams.tol is not None else d["tol"]
    max_iter = hparams.max_iter if hparams.max_iter is not None else d["max_iter"]
    if any(not 0 < c < float("inf") for c in C):
        raise SystemExit("--C must be positive")
    if not 0 < tol < float("inf") or max_iter < 1:
        raise SystemExit("--tol must be positive and --max-iter at least 1")
    return C, tol, max_iter


def load_ts2vec(hparams, dev):
    """The TS2Vec encoder of --ts2vec-model on the device for --dataset ts2vec (widths and depth from the
    checkpoint's shapes), else None."""
    if hparams.dataset != "ts2vec":
        return None
    from arcweld.ts2vec import load_checkpoint
    try:
        return load_checkpoint(hparams.ts2vec_model, dev)
    except (ValueError, RuntimeError, KeyError) as e:
        raise SystemExit(f"--ts2vec-model: {hparams.ts2vec_model!r} is not a TS2Vec checkpoint ({e})") from None


def load_groups(path):
    """{'train' / 'val' / 'test': ids} for the '<split>_groups' arrays the .npz holds (none: {})."""
    if not path:
        return {}
    with np.load(path, allow_pickle=False) as f:
        return {k: torch.tensor(f[k + "_groups"], dtype=torch.long) for k in ("train", "val", "test")
                if k + "_groups" in f.files}


def main_linear(hparams):
    if hparams.neighbours_out or hparams.loo:
        raise SystemExit("--neighbours-out and --loo belong to --protocol knn: a linear probe has no neighbours "
                         "(--model-out writes the fitted coefficients)")
    if hparams.standardize:
        raise SystemExit("--standardize belongs to --protocol svm: the linear probe scales unless --no-standardize")
    if hparams.gamma != "scale":
        raise SystemExit("--gamma belongs to --protocol svm")
    C, tol, max_iter = resolve_fit_args(hparams)
    from arcweld.retrieve import latent_linear_probe
    from train_transformer_mtasks import load_splits, load_vqvae
    dev = torch.device("cuda", torch.cuda.current_device())
    vqvae = load_vqvae(hparams.vqvae_model, dev) if hparams.dataset == "latent_vq_vae" else None
    ts2vec = load_ts2vec(hparams, dev)
    res = latent_linear_probe(load_splits(hparams, dev), hparams.n_cycles, C=C, dataset=hparams.dataset,
                              vqvae=vqvae, standardize=not hparams.no_standardize, tol=tol, max_iter=max_iter,
                              ts2vec=ts2vec)
    summary = {name: {m: res[name][m] for m in METRICS} for name in ("val", "test")}
    summary.update(per_C=res["per_C"], C_selected=res["C_selected"], protocol="linear", dataset=hparams.dataset,
                   standardize=not hparams.no_standardize, n_cycles=hparams.n_cycles, converged=res["converged"],
                   n_iter=res["n_iter"])
    with open(hparams.out, "w") as f:
        json.dump(summary, f, indent=1, sort_keys=True)
    if hparams.model_out:
        np.savez(hparams.model_out, **{k: res["fit"][k].cpu().numpy() for k in ("coef", "intercept", "mean", "scale",
                                                                                "C")})
    for name in ("val", "test"):
        log.info(f"{name} (C = {res['C_selected']:g}): " + ", ".join(f"{m} {res[name][m]:.4f}" for m in METRICS))
    return res


def main_svm(hparams):
    if hparams.neighbours_out or hparams.loo:
        raise SystemExit("--neighbours-out and --loo belong to --protocol knn: an SVM probe has no neighbours "
                         "(--model-out writes the support vectors)")
    if hparams.no_standardize:
        raise SystemExit("--no-standardize belongs to the knn and linear protocols: the SVM probe does not scale "
                         "unless --standardize")
    if hparams.gamma != "scale" and not 0 < hparams.gamma < float("inf"):
        raise SystemExit("--gamma must be positive or 'scale'")
    C, tol, max_iter = resolve_fit_args(hparams)
    from arcweld.retrieve import latent_svm_probe
    from train_transformer_mtasks import load_splits, load_vqvae
    dev = torch.device("cuda", torch.cuda.current_device())
    vqvae = load_vqvae(hparams.vqvae_model, dev) if hparams.dataset == "latent_vq_vae" else None
    ts2vec = load_ts2vec(hparams, dev)
    try:
        res = latent_svm_probe(load_splits(hparams, dev), hparams.n_cycles, C=C, gamma=hparams.gamma,
                               dataset=hparams.dataset, vqvae=vqvae, standardize=hparams.standardize, tol=tol,
                               max_iter=max_iter, ts2vec=ts2vec)
    except ValueError as e:
        raise SystemExit(f"--protocol svm: {e}") from None
    summary = {name: {m: res[name][m] for m in METRICS} for name in ("val", "test")}
    summary.update(per_C=res["per_C"], C_selected=res["C_selected"], protocol="svm", dataset=hparams.dataset,
                   standardize=hparams.standardize, n_cycles=hparams.n_cycles, converged=res["converged"],
                   n_iter=res["n_iter"], gamma=res["gamma"], n_support=res["n_support"])
    with open(hparams.out, "w") as f:
        json.dump(summary, f, indent=1, sort_keys=True)
    if hparams.model_out:
        fit = res["fit"]
        np.savez(hparams.model_out, support=fit["support"].cpu().numpy(),
                 support_vectors=fit["support_vectors"].cpu().numpy(),
                 dual_coef=fit["dual_coef"][:, :, fit["support"]].cpu().numpy(), rho=fit["rho"].cpu().numpy(),
                 gamma=np.float64(fit["gamma"]), C=fit["C"].cpu().numpy(), mean=fit["mean"].cpu().numpy(),
                 scale=fit["scale"].cpu().numpy())
    for name in ("val", "test"):
        log.info(f"{name} (C = {res['C_selected']:g}, gamma = {res['gamma']:g}): "
                 + ", ".join(f"{m} {res[name][m]:.4f}" for m in METRICS))
    return res


def main(hparams):
    dtw = resolve_dtw(hparams)
    if hparams.dataset == "latent_vq_vae":
        require_checkpoint(hparams.vqvae_model, "--vqvae-model")
    if hparams.dataset == "ts2vec":
        if not hparams.ts2vec_model or not os.path.exists(hparams.ts2vec_model):
            raise SystemExit(f"--ts2vec-model: checkpoint {hparams.ts2vec_model!r} not found -- --dataset ts2vec "
                             "probes a trained TS2Vec encoder (the file the reference's TS2Vec.save writes)")
    elif hparams.ts2vec_model:
        raise SystemExit("--ts2vec-model belongs to --dataset ts2vec")
    if hparams.n_cycles < 1:
        raise SystemExit("--n-cycles must be at least 1")
    if hparams.protocol == "linear":
        return main_linear(hparams)
    if hparams.protocol == "svm":
        return main_svm(hparams)
    if hparams.model_out:
        raise SystemExit("--model-out belongs to --protocol linear or svm")
    if hparams.standardize or hparams.gamma != "scale":
        raise SystemExit("--standardize and --gamma belong to --protocol svm")
    from arcweld.retrieve import MAX_K, latent_knn_probe
    if not 1 <= hparams.k <= MAX_K:
        raise SystemExit(f"--k must lie in 1..{MAX_K}")
    from train_transformer_mtasks import load_splits, load_vqvae
    dev = torch.device("cuda", torch.cuda.current_device())
    vqvae = load_vqvae(hparams.vqvae_model, dev) if hparams.dataset == "latent_vq_vae" else None
    ts2vec = load_ts2vec(hparams, dev)
    res = latent_knn_probe(load_splits(hparams, dev), hparams.n_cycles, k=hparams.k, dataset=hparams.dataset,
                           vqvae=vqvae, weights=hparams.weights, standardize=not hparams.no_standardize,
                           loo=hparams.loo, groups=load_groups(hparams.data_npz), ts2vec=ts2vec,
                           **({"metric": "dtw", "radius": dtw["radius"]} if dtw else {}))
    summary = {name: {m: r[m] for m in METRICS} for name, r in res.items()}
    summary.update(k=hparams.k, weights=hparams.weights, dataset=hparams.dataset,
                   standardize=not hparams.no_standardize, n_cycles=hparams.n_cycles, **dtw)
    with open(hparams.out, "w") as f:
        json.dump(summary, f, indent=1, sort_keys=True)
    if hparams.neighbours_out:
        np.savez(hparams.neighbours_out, **{f"{name}_{key}": r[key].cpu().numpy() for name, r in res.items()
                                            for key in ("idx", "dist", "pred")})
    for name, r in res.items():
        log.info(f"{name}: " + ", ".join(f"{m} {r[m]:.4f}" for m in METRICS))
    return res


if __name__ == '__main__':
    args = parser().parse_args()
    log.basicConfig(level=log.INFO, format='%(asctime)s - %(levelname)s - %(message)s')
    main(args)
