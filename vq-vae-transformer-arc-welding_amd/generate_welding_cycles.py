"""Generate weld cycles with the two trained models: measured cycles in, the following ones out as signals.

``--vqvae-model`` (a checkpoint of train_reconstruction_embedding.py) and ``--transformer-model`` (one of
train_transformer_mtasks.py, trained with the same ``--n-cycles``) are loaded through their ``load_from_checkpoint``;
both must exist -- a randomly initialised generator is of no use to anyone.  The first ``--prompt-cycles`` cycles of
each sequence are the prompt: synthetic windows (arcweld.data.synthetic_windows, as the training scripts use), or the
'test' split of ``--data-npz`` ((n, n_cycles*200, 2), the layout train_transformer_mtasks.py reads).  The remaining
cycles are generated on the device (arcweld.generate.continue_cycles) and ``--out`` receives an .npz with

  prompt (n, prompt_cycles*200, 2) f32    ids (n, n_cycles*S) int64    x_hat (n, n_cycles*200, 2) f32

where x_hat[:, :prompt_cycles*200] is the VQ-VAE's reconstruction of the prompt.  ``--do-sample`` draws from the
(``--top-k`` / ``--min-p`` / ``--top-p`` filtered, ``--temperature`` scaled) distribution with ``--seed``; the default
is greedy.  ``--logp`` adds gen_logp, gen_logq (n, (n_cycles - prompt_cycles)*S) and gen_cycle_nll (n, n_cycles -
prompt_cycles): the generated ids' log-probabilities on the scale of score_welding_cycles.py (continue_cycles).
``--num-beams W`` searches for the most probable continuation with a beam of width W instead (it excludes the sampling
flags); ids / x_hat are then the best hypothesis, and the ``--num-return`` R best ones are added as beam_ids
(n, R, n_cycles*S), beam_scores (n, R) -- their log-probabilities, best first -- and beam_x_hat (n, R, n_cycles*200, 2).
"""
import argparse
import logging as log
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import numpy as np  # noqa: E402
import torch  # noqa: E402


def parser():
    p = argparse.ArgumentParser(description='Generate-Welding-Cycles')
    p.add_argument('--vqvae-model', type=str, default="model_checkpoints/VQ-VAE-Patch/vq_vae_patch_best_01.ckpt")
    p.add_argument('--transformer-model', type=str, default="",
                   help="MyTransformerDecoder checkpoint (model.save_checkpoint)")
    p.add_argument('--n-cycles', type=int, help='Cycles per sequence (prompt + generated)', default=20)
    p.add_argument('--prompt-cycles', type=int, help='Measured cycles given as the prompt', default=10)
    p.add_argument('--n-seqs', type=int, help='Number of sequences to continue', default=16)
    p.add_argument('--data-npz', type=str, default="", help="real windows: its 'test' split provides the prompts")
    p.add_argument('--do-sample', action=argparse.BooleanOptionalAction, default=False)
    p.add_argument('--top-k', type=int, default=None)
    p.add_argument('--top-p', type=float, default=None, help="nucleus: keep the fewest ids reaching this mass")
    p.add_argument('--min-p', type=float, default=None, help="keep ids with >= this share of the mode's probability")
    p.add_argument('--temperature', type=float, default=1.0)
    p.add_argument('--seed', type=int, default=0)
    p.add_argument('--logp', action=argparse.BooleanOptionalAction, default=False,
                   help="also store the generated ids' log-probabilities")
    p.add_argument('--num-beams', type=int, default=None,
                   help="beam search of this width (1..32) instead of greedy decoding or sampling")
    p.add_argument('--num-return', type=int, default=1, help="hypotheses stored per sequence (1..num_beams)")
    p.add_argument('--precision', choices=["fp32", "bf16"], default="fp32",
                   help="MFMA operand dtype (bf16: opt-in, fp32 accumulation)")
    p.add_argument('--out', type=str, default="generated_cycles.npz")
    return p


def require_checkpoint(path, flag):
    if not path or not os.path.exists(path):
        raise SystemExit(f"{flag}: checkpoint {path!r} not found -- generation needs both trained models "
                         "(train_reconstruction_embedding.py and train_transformer_mtasks.py write them)")
    return path


def load_prompts(hparams, window, dev):
    from arcweld.data import synthetic_windows
    n = hparams.prompt_cycles * window
    if hparams.data_npz:
        with np.load(hparams.data_npz, allow_pickle=False) as f:
            x = torch.tensor(f["test"][:hparams.n_seqs], dtype=torch.float32, device=dev)
        if x.dim() != 3 or x.shape[1] < n:
            raise SystemExit(f"--data-npz: 'test' must hold (n, >= {n}, C) windows, got {tuple(x.shape)}")
        return x[:, :n].contiguous()
    return synthetic_windows(hparams.n_seqs, hparams.prompt_cycles, hparams.seed, dev, window=window)


def main(hparams):
    require_checkpoint(hparams.vqvae_model, "--vqvae-model")
    require_checkpoint(hparams.transformer_model, "--transformer-model")
    if not 1 <= hparams.prompt_cycles < hparams.n_cycles:
        raise SystemExit(f"--prompt-cycles must lie in 1..n_cycles - 1 = {hparams.n_cycles - 1}")
    from arcweld.generate import continue_cycles
    from arcweld.precision import set_operand_dtype
    from model.transformer_decoder import MyTransformerDecoder
    from model.vq_vae_patch_embedd import VQVAEPatch
    set_operand_dtype(hparams.precision)
    dev = torch.device("cuda", torch.cuda.current_device())
    vqvae = VQVAEPatch.load_from_checkpoint(hparams.vqvae_model).to(dev).eval()
    decoder = MyTransformerDecoder.load_from_checkpoint(hparams.transformer_model).to(dev).eval()
    prompt = load_prompts(hparams, vqvae.seq_len, dev)
    out = continue_cycles(vqvae, decoder, prompt, hparams.n_cycles, do_sample=bool(hparams.do_sample),
                          top_k=hparams.top_k, temperature=hparams.temperature, seed=hparams.seed,
                          top_p=hparams.top_p, min_p=hparams.min_p, return_logp=bool(hparams.logp),
                          **({} if hparams.num_beams is None else
                             dict(num_beams=hparams.num_beams, num_return=hparams.num_return)))
    extra = {k: out[k].cpu().numpy() for k in ("gen_logp", "gen_logq", "gen_cycle_nll", "beam_ids", "beam_scores",
                                               "beam_x_hat") if k in out}
    np.savez(hparams.out, prompt=prompt.cpu().numpy(), ids=out["ids"].cpu().numpy(),
             x_hat=out["x_hat"].cpu().numpy(), **extra)
    log.info(f"wrote {hparams.out}: {tuple(out['ids'].shape)} ids, {tuple(out['x_hat'].shape)} signals")
    return out


if __name__ == '__main__':
    args = parser().parse_args()
    log.basicConfig(level=log.INFO, format='%(asctime)s - %(levelname)s - %(message)s')
    main(args)
