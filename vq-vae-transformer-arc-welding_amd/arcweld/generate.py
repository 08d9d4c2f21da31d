"""Generate weld cycles: measured cycles in, the next ones out as current / voltage signals.

The three trained pieces end to end, all on the device: the frozen VQ-VAE encoder turns the prompt cycles into ids
(arcweld.tokenize.encode_ids), the Transformer continues the id sequence (MyTransformerDecoder.generate_ids: one cached
decode step and one aw_sample_next launch per token, restricted to the codebook ids), and the VQ-VAE decoder half
turns every id back into a window (arcweld.tokenize.decode_ids, aw_vq_decode_gather).
"""
from __future__ import annotations

import torch

from . import tokenize


@torch.no_grad()
def continue_cycles(vqvae, decoder, x_prompt, n_cycles, do_sample=False, top_k=None, temperature=1.0, seed=0,
                    dtype=None):
    """x_prompt (B, c*L, C) f32, 1 <= c < n_cycles measured cycles -> {"ids": (B, n_cycles*S) int64, "x_hat":
    (B, n_cycles*L, C) f32}: the prompt's ids followed by (n_cycles - c)*S generated ones, and all of them decoded
    (the first c*L rows of x_hat are the VQ-VAE's reconstruction of the prompt).

    The Transformer must have been trained on [start, ids of n_cycles cycles] (tokenize.autoregressive_pairs):
    seq_len = n_cycles*S + 1 and n_classes = K + 2 with start = K, end = K + 1; generation is restricted to ids < K.
    ``dtype``: the VQ-VAE's operand dtype on both ways (None: the process setting, arcweld.precision)."""
    S = tokenize.ids_per_window(vqvae)
    L, Kc = vqvae.seq_len, vqvae.num_embeddings
    n_cycles = int(n_cycles)
    if decoder.seq_len != n_cycles * S + 1 or decoder.n_classes != Kc + 2:
        raise ValueError(f"continue_cycles: the Transformer (seq_len {decoder.seq_len}, n_classes {decoder.n_classes}) "
                         f"does not fit {n_cycles} cycles of this VQ-VAE: it needs seq_len = n_cycles*S + 1 = "
                         f"{n_cycles * S + 1} and n_classes = num_embeddings + 2 = {Kc + 2}")
    if x_prompt.dim() != 3 or x_prompt.shape[1] % L or not L <= x_prompt.shape[1] < n_cycles * L:
        raise ValueError(f"continue_cycles: the prompt must be (B, c*{L}, C) with 1 <= c < n_cycles = {n_cycles}, "
                         f"got {tuple(x_prompt.shape)}")
    c = x_prompt.shape[1] // L
    start = decoder.n_classes - 2
    kw = {} if dtype is None else dict(dtype=dtype)          # encode_ids' own default is exact fp32
    prompt_ids = tokenize.encode_ids(vqvae, x_prompt, **kw)
    x = torch.cat([torch.full_like(prompt_ids[:, :1], start), prompt_ids], dim=1)
    out = decoder.generate_ids(x, (n_cycles - c) * S, do_sample=do_sample, top_k=top_k, temperature=temperature,
                               valid_ids=start, seed=seed)
    ids = out[:, 1:].contiguous()
    return {"ids": ids, "x_hat": tokenize.decode_ids(vqvae, ids, dtype=dtype)}
