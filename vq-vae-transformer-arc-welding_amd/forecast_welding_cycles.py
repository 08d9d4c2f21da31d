"""Forecast weld cycles with the two trained models: measured cycles in, an ensemble of the following ones out.

``--vqvae-model`` and ``--transformer-model`` are the two checkpoints of generate_welding_cycles.py (trained with the
same ``--n-cycles``); both must exist.  The first ``--prompt-cycles`` cycles of each sequence are the prompt: synthetic
windows (arcweld.data.synthetic_windows), or the 'test' split of ``--data-npz`` ((n, >= prompt_cycles*200, 2)).  For
every prompt ``--num-samples`` N continuations are drawn on the device (arcweld.generate.forecast_cycles: one prefill per
prompt, ``--top-k`` / ``--min-p`` / ``--top-p`` filtered, ``--temperature`` scaled, ``--seed``) and reduced there to
bands; with c = prompt_cycles, f = n_cycles - c and Q = the number of ``--quantiles``, ``--out`` receives an .npz with

  prompt (n, c*200, 2) f32            ids (n, N, n_cycles*S) int64        x_prompt_hat (n, c*200, 2) f32
  x_hat (n, N, f*200, 2) f32          sample_cycle_nll (n, N, f) f32      mean, std (n, f*200, 2) f32
  quantiles (n, Q, f*200, 2) f32      q (Q,) f32

``--truth``: the measured cycles that follow the prompt in the input are the forecast's truth -- the input must then
hold n_cycles cycles -- and the file also gets x_true (n, f*200, 2), crps (n, f), the ensemble CRPS per cycle in signal
units, and coverage (n, f), the share of each cycle's points between the first and the last quantile.
"""
import argparse
import logging as log
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import numpy as np  # noqa: E402
import torch  # noqa: E402

from generate_welding_cycles import require_checkpoint  # noqa: E402


def quantile_list(text):
    try:
        return tuple(float(t) for t in text.split(",") if t.strip())
    except ValueError:
        raise argparse.ArgumentTypeError(f"expected comma-separated probabilities, got {text!r}")


def parser():
    p = argparse.ArgumentParser(description='Forecast-Welding-Cycles')
    p.add_argument('--vqvae-model', type=str, default="model_checkpoints/VQ-VAE-Patch/vq_vae_patch_best_01.ckpt")
    p.add_argument('--transformer-model', type=str, default="",
                   help="MyTransformerDecoder checkpoint (model.save_checkpoint)")
    p.add_argument('--n-cycles', type=int, help='Cycles per sequence (prompt + forecast)', default=20)
    p.add_argument('--prompt-cycles', type=int, help='Measured cycles given as the prompt', default=10)
    p.add_argument('--n-seqs', type=int, help='Number of sequences to forecast', default=16)
    p.add_argument('--data-npz', type=str, default="", help="real windows: its 'test' split provides the prompts")
    p.add_argument('--num-samples', type=int, default=16, help="continuations drawn per prompt (1..32)")
    p.add_argument('--quantiles', type=quantile_list, default=(0.05, 0.5, 0.95),
                   help="ascending probabilities of the bands, comma-separated (at most 8)")
    p.add_argument('--truth', action=argparse.BooleanOptionalAction, default=False,
                   help="score the forecast against the measured cycles that follow the prompt in the input")
    p.add_argument('--top-k', type=int, default=None)
    p.add_argument('--top-p', type=float, default=None, help="nucleus: keep the fewest ids reaching this mass")
    p.add_argument('--min-p', type=float, default=None, help="keep ids with >= this share of the mode's probability")
    p.add_argument('--temperature', type=float, default=1.0)
    p.add_argument('--seed', type=int, default=0)
    p.add_argument('--precision', choices=["fp32", "bf16"], default="fp32",
                   help="MFMA operand dtype (bf16: opt-in, fp32 accumulation)")
    p.add_argument('--out', type=str, default="forecast_cycles.npz")
    return p


def load_cycles(hparams, window, dev):
    """(prompt, truth or None): the first prompt_cycles cycles of every sequence and, with --truth, the rest."""
    from arcweld.data import synthetic_windows
    n_prompt, n_all = hparams.prompt_cycles * window, hparams.n_cycles * window
    if hparams.data_npz:
        with np.load(hparams.data_npz, allow_pickle=False) as f:
            x = torch.tensor(f["test"][:hparams.n_seqs], dtype=torch.float32, device=dev)
        need = n_all if hparams.truth else n_prompt
        if x.dim() != 3 or x.shape[1] < need:
            raise SystemExit(f"--data-npz: 'test' must hold (n, >= {need}, C) windows"
                             f"{' (--truth needs all n_cycles cycles)' if hparams.truth else ''}, "
                             f"got {tuple(x.shape)}")
    else:
        x = synthetic_windows(hparams.n_seqs, hparams.n_cycles, hparams.seed, dev, window=window)
    return x[:, :n_prompt].contiguous(), (x[:, n_prompt:n_all].contiguous() if hparams.truth else None)


def main(hparams):
    require_checkpoint(hparams.vqvae_model, "--vqvae-model")
    require_checkpoint(hparams.transformer_model, "--transformer-model")
    if not 1 <= hparams.prompt_cycles < hparams.n_cycles:
        raise SystemExit(f"--prompt-cycles must lie in 1..n_cycles - 1 = {hparams.n_cycles - 1}")
    from arcweld.generate import forecast_cycles
    from arcweld.precision import set_operand_dtype
    from model.transformer_decoder import MyTransformerDecoder
    from model.vq_vae_patch_embedd import VQVAEPatch
    set_operand_dtype(hparams.precision)
    dev = torch.device("cuda", torch.cuda.current_device())
    vqvae = VQVAEPatch.load_from_checkpoint(hparams.vqvae_model).to(dev).eval()
    decoder = MyTransformerDecoder.load_from_checkpoint(hparams.transformer_model).to(dev).eval()
    prompt, truth = load_cycles(hparams, vqvae.seq_len, dev)
    out = forecast_cycles(vqvae, decoder, prompt, hparams.n_cycles, hparams.num_samples, quantiles=hparams.quantiles,
                          x_true=truth, top_k=hparams.top_k, top_p=hparams.top_p, min_p=hparams.min_p,
                          temperature=hparams.temperature, seed=hparams.seed)
    extra = {} if truth is None else {"x_true": truth.cpu().numpy()}
    np.savez(hparams.out, prompt=prompt.cpu().numpy(), q=np.asarray(hparams.quantiles, dtype=np.float32), **extra,
             **{k: v.cpu().numpy() for k, v in out.items()})
    msg = f"wrote {hparams.out}: {tuple(out['x_hat'].shape)} sampled signals, mean spread {out['std'].mean().item():.4f}"
    if truth is not None:
        msg += f", mean CRPS {out['crps'].mean().item():.4f}, mean coverage {out['coverage'].mean().item():.3f}"
    log.info(msg)
    return out


if __name__ == '__main__':
    args = parser().parse_args()
    log.basicConfig(level=log.INFO, format='%(asctime)s - %(levelname)s - %(message)s')
    main(args)
