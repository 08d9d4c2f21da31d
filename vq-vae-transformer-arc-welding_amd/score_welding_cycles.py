"""Score measured weld cycles under the two trained models: which run, which cycle and which tokens are unusual.

``--vqvae-model`` and ``--transformer-model`` are the checkpoints generate_welding_cycles.py takes (trained with the
same ``--n-cycles``); both must exist.  ``--n-seqs`` sequences of ``--n-cycles`` measured cycles are scored on the
device (arcweld.generate.score_cycles): synthetic windows (arcweld.data.synthetic_windows), or the 'test' split of
``--data-npz`` ((n, >= n_cycles*200, 2), the layout train_transformer_mtasks.py reads).  ``--out`` receives an .npz with

  x (n, n_cycles*200, 2) f32       ids (n, n_cycles*S) int64
  logp, entropy (n, n_cycles*S) f32    rank (n, n_cycles*S) int32
  cycle_nll, recon_mse, vq_mse (n, n_cycles) f32

logp / rank / entropy: each id under the Transformer given the ids before it (rank 0: the greedy generator would have
produced it); cycle_nll: -logp summed over a cycle (cycle 0 has only the start token as context); recon_mse / vq_mse:
the VQ-VAE's reconstruction and quantisation error per cycle.
"""
import argparse
import logging as log
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import numpy as np  # noqa: E402
import torch  # noqa: E402

from generate_welding_cycles import require_checkpoint  # noqa: E402


def parser():
    p = argparse.ArgumentParser(description='Score-Welding-Cycles')
    p.add_argument('--vqvae-model', type=str, default="model_checkpoints/VQ-VAE-Patch/vq_vae_patch_best_01.ckpt")
    p.add_argument('--transformer-model', type=str, default="",
                   help="MyTransformerDecoder checkpoint (model.save_checkpoint)")
    p.add_argument('--n-cycles', type=int, help='Measured cycles per sequence', default=20)
    p.add_argument('--n-seqs', type=int, help='Number of sequences to score', default=16)
    p.add_argument('--data-npz', type=str, default="", help="real windows: its 'test' split is scored")
    p.add_argument('--seed', type=int, default=0)
    p.add_argument('--precision', choices=["fp32", "bf16"], default="fp32",
                   help="MFMA operand dtype (bf16: opt-in, fp32 accumulation)")
    p.add_argument('--out', type=str, default="cycle_scores.npz")
    return p


def load_cycles(hparams, window, dev):
    from arcweld.data import synthetic_windows
    n = hparams.n_cycles * window
    if hparams.data_npz:
        with np.load(hparams.data_npz, allow_pickle=False) as f:
            x = torch.tensor(f["test"][:hparams.n_seqs], dtype=torch.float32, device=dev)
        if x.dim() != 3 or x.shape[1] < n:
            raise SystemExit(f"--data-npz: 'test' must hold (n, >= {n}, C) windows, got {tuple(x.shape)}")
        return x[:, :n].contiguous()
    return synthetic_windows(hparams.n_seqs, hparams.n_cycles, hparams.seed, dev, window=window)


def main(hparams):
    require_checkpoint(hparams.vqvae_model, "--vqvae-model")
    require_checkpoint(hparams.transformer_model, "--transformer-model")
    if hparams.n_cycles < 1:
        raise SystemExit("--n-cycles must be at least 1")
    from arcweld.generate import score_cycles
    from arcweld.precision import set_operand_dtype
    from model.transformer_decoder import MyTransformerDecoder
    from model.vq_vae_patch_embedd import VQVAEPatch
    set_operand_dtype(hparams.precision)
    dev = torch.device("cuda", torch.cuda.current_device())
    vqvae = VQVAEPatch.load_from_checkpoint(hparams.vqvae_model).to(dev).eval()
    decoder = MyTransformerDecoder.load_from_checkpoint(hparams.transformer_model).to(dev).eval()
    x = load_cycles(hparams, vqvae.seq_len, dev)
    out = score_cycles(vqvae, decoder, x)
    np.savez(hparams.out, x=x.cpu().numpy(), **{k: v.cpu().numpy() for k, v in out.items()})
    log.info(f"wrote {hparams.out}: {tuple(out['ids'].shape)} ids, mean NLL per token "
             f"{-out['logp'].mean().item():.4f}, rank-0 share {(out['rank'] == 0).float().mean().item():.3f}")
    return out


if __name__ == '__main__':
    args = parser().parse_args()
    log.basicConfig(level=log.INFO, format='%(asctime)s - %(levelname)s - %(message)s')
    main(args)
