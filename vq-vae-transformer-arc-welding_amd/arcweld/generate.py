"""Generate weld cycles: measured cycles in, the next ones out as current / voltage signals.

The three trained pieces end to end, all on the device: the frozen VQ-VAE encoder turns the prompt cycles into ids
(arcweld.tokenize.encode_ids), the Transformer continues the id sequence (MyTransformerDecoder.generate_ids: one cached
decode step and one aw_sample_next / aw_sample_next_ex launch per token, restricted to the codebook ids), and the VQ-VAE decoder half
turns every id back into a window (arcweld.tokenize.decode_ids, aw_vq_decode_gather).  With ``num_beams`` the
continuation is searched for instead (MyTransformerDecoder.beam_search_ids: aw_beam_step and aw_beam_gather per token)
and the ranked hypotheses come back beside the best one.

``score_cycles`` is the mirror for cycles that were measured: the same two models, the same id layout and the same
restriction to the codebook ids, but the ids come from the encoder and the Transformer only says how likely each one
was (aw_score_rows), beside the VQ-VAE's own reconstruction and quantisation errors per cycle (aw_window_sqerr).

``forecast_cycles`` draws many continuations of one prompt at once (MyTransformerDecoder.sample_ids: one prefill, the
cache fanned out by aw_beam_gather) and reduces their decoded signals on the device to a mean, a spread, quantile bands
and -- against the cycles that were measured afterwards -- a CRPS and a band coverage per cycle (aw_ensemble_stats).
"""
from __future__ import annotations

import torch

from . import tokenize


@torch.no_grad()
def continue_cycles(vqvae, decoder, x_prompt, n_cycles, do_sample=False, top_k=None, temperature=1.0, seed=0,
                    dtype=None, top_p=None, min_p=None, return_logp=False, num_beams=None, num_return=1):
    """x_prompt (B, c*L, C) f32, 1 <= c < n_cycles measured cycles -> {"ids": (B, n_cycles*S) int64, "x_hat":
    (B, n_cycles*L, C) f32}: the prompt's ids followed by (n_cycles - c)*S generated ones, and all of them decoded
    (the first c*L rows of x_hat are the VQ-VAE's reconstruction of the prompt).

    The Transformer must have been trained on [start, ids of n_cycles cycles] (tokenize.autoregressive_pairs):
    seq_len = n_cycles*S + 1 and n_classes = K + 2 with start = K, end = K + 1; generation is restricted to ids < K.
    ``dtype``: the VQ-VAE's operand dtype on both ways (None: the process setting, arcweld.precision).

    top_p / min_p: the nucleus and min-p cuts of ``generate_ids``.  return_logp adds, for the generated ids only,
    "gen_logp" and "gen_logq" (B, (n_cycles - c)*S) f32 and "gen_cycle_nll" (B, n_cycles - c) f32 = -gen_logp summed
    per cycle: gen_logp / gen_cycle_nll are on the scale of ``score_cycles``' logp / cycle_nll (the model's own
    distribution over the codebook ids), gen_logq is the log-probability under the filtered, tempered distribution the
    id was drawn from.  They come out of the launches that picked the ids: no second forward.

    num_beams (1..32): the continuation is searched for instead of drawn (MyTransformerDecoder.beam_search_ids: the
    most probable continuations a beam of that width finds).  "ids" and "x_hat" are then the best hypothesis, and the
    R = num_return (1..num_beams) best ones, best first, are added as "beam_ids" (B, R, n_cycles*S) int64, "beam_scores"
    (B, R) f32 -- the log-probability of each hypothesis' generated ids, on the scale of -cycle_nll summed -- and
    "beam_x_hat" (B, R, n_cycles*L, C) f32, all decoded in one ``decode_ids`` pass.  return_logp then gives gen_logp and
    gen_cycle_nll of the best hypothesis and gen_logq = 0, as for greedy.  The search is deterministic: combining it with
    do_sample, top_k, top_p, min_p or a temperature other than 1 raises ValueError."""
    if num_beams is not None and (do_sample or top_k is not None or top_p is not None or min_p is not None
                                  or temperature != 1):
        raise ValueError("continue_cycles: num_beams searches the model's own distribution: it cannot be combined "
                         "with do_sample, top_k, top_p, min_p or temperature != 1")
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
    if num_beams is not None:
        bs = decoder.beam_search_ids(x, (n_cycles - c) * S, num_beams, valid_ids=start, num_return=num_return)
        B, R = bs["scores"].shape
        beam_ids = bs["ids"][:, :, 1:].contiguous()
        x_hat = tokenize.decode_ids(vqvae, beam_ids.view(B * R, n_cycles * S), dtype=dtype)
        x_hat = x_hat.view(B, R, *x_hat.shape[1:])
        res = {"ids": beam_ids[:, 0].contiguous(), "x_hat": x_hat[:, 0].contiguous(), "beam_ids": beam_ids,
               "beam_scores": bs["scores"], "beam_x_hat": x_hat}
        if return_logp:
            lp = bs["logp"][:, 0].contiguous()
            res.update(gen_logp=lp, gen_logq=torch.zeros_like(lp), gen_cycle_nll=-lp.view(B, n_cycles - c, S).sum(-1))
        return res
    out = decoder.generate_ids(x, (n_cycles - c) * S, do_sample=do_sample, top_k=top_k, temperature=temperature,
                               valid_ids=start, seed=seed, top_p=top_p, min_p=min_p, return_logp=return_logp)
    lp = None
    if return_logp:
        out, lp = out
    ids = out[:, 1:].contiguous()
    res = {"ids": ids, "x_hat": tokenize.decode_ids(vqvae, ids, dtype=dtype)}
    if lp is not None:
        res.update(gen_logp=lp["logp"], gen_logq=lp["logq"],
                   gen_cycle_nll=-lp["logp"].view(ids.shape[0], n_cycles - c, S).sum(-1))
    return res


@torch.no_grad()
def forecast_cycles(vqvae, decoder, x_prompt, n_cycles, num_samples, quantiles=(0.05, 0.5, 0.95), x_true=None,
                    top_k=None, top_p=None, min_p=None, temperature=1.0, seed=0, dtype=None):
    """An ensemble forecast: N = num_samples (1..32) sampled continuations of every prompt, the pointwise spread of
    their signals, and -- when the cycles that followed were measured -- the forecast's score against them.  With
    x_prompt (B, c*L, C) f32, 1 <= c < n_cycles, f = n_cycles - c forecast cycles and Q quantiles:

      ids (B, N, n_cycles*S) int64          x_prompt_hat (B, c*L, C)          x_hat (B, N, f*L, C)
      sample_cycle_nll (B, N, f)            mean, std (B, f*L, C)             quantiles (B, Q, f*L, C)
      with x_true (B, f*L, C) f32:          crps (B, f)                       coverage (B, f)   (needs Q >= 2)

    ids: the prompt's ids followed by each sample's f*S drawn ones (MyTransformerDecoder.sample_ids: one prefill per
    prompt, the cache fanned out to B*N rows; top_k / top_p / min_p / temperature / seed as in ``continue_cycles``
    with do_sample).  x_prompt_hat is the VQ-VAE's reconstruction of the prompt, decoded once; x_hat the generated
    cycles of all samples, one ``decode_ids`` pass.  sample_cycle_nll is -logp summed per cycle, on ``score_cycles``'
    cycle_nll scale, from the launches that drew the ids.  mean / std (unbiased) / quantiles (numpy's "linear"
    rule; ``quantiles`` ascending in [0, 1], at most 8) are taken over the N samples at every point; crps is the
    ensemble CRPS against x_true averaged over each cycle's L*C points (in signal units: 0 is a perfect, sharp
    forecast), coverage the share of a cycle's points whose truth lies between the first and the last quantile.  All
    of them come from ONE aw_ensemble_stats launch (G = B, M = f*L*C, seg = L*C): no sample leaves the device.

    The model-fit and prompt rules are ``continue_cycles``'; num_samples = 1 gives its sampled continuation."""
    S = tokenize.ids_per_window(vqvae)
    L, Kc = vqvae.seq_len, vqvae.num_embeddings
    n_cycles = int(n_cycles)
    if decoder.seq_len != n_cycles * S + 1 or decoder.n_classes != Kc + 2:
        raise ValueError(f"forecast_cycles: the Transformer (seq_len {decoder.seq_len}, n_classes {decoder.n_classes}) "
                         f"does not fit {n_cycles} cycles of this VQ-VAE: it needs seq_len = n_cycles*S + 1 = "
                         f"{n_cycles * S + 1} and n_classes = num_embeddings + 2 = {Kc + 2}")
    if (not isinstance(x_prompt, torch.Tensor) or x_prompt.dim() != 3 or x_prompt.shape[1] % L
            or not L <= x_prompt.shape[1] < n_cycles * L):
        raise ValueError(f"forecast_cycles: the prompt must be (B, c*{L}, C) with 1 <= c < n_cycles = {n_cycles}, "
                         f"got {tuple(getattr(x_prompt, 'shape', ()))}")
    from . import kernels as K
    N = int(num_samples)
    if not 1 <= N <= K.nat.AW_BEAM_MAX_W:
        raise ValueError(f"forecast_cycles: num_samples = {num_samples} outside 1..{K.nat.AW_BEAM_MAX_W}")
    qs = [float(q) for q in quantiles]
    Q = len(qs)
    if Q > K.nat.AW_ENSEMBLE_MAX_Q or any(not 0.0 <= q <= 1.0 for q in qs) or any(a > b for a, b in zip(qs, qs[1:])):
        raise ValueError(f"forecast_cycles: quantiles must be at most {K.nat.AW_ENSEMBLE_MAX_Q} ascending probabilities "
                         f"in [0, 1], got {tuple(quantiles)}")
    B, C = x_prompt.shape[0], x_prompt.shape[2]
    c = x_prompt.shape[1] // L
    f = n_cycles - c
    if x_true is not None:
        if (not isinstance(x_true, torch.Tensor) or x_true.dtype != torch.float32
                or tuple(x_true.shape) != (B, f * L, C)):
            raise ValueError(f"forecast_cycles: x_true must be float32 {(B, f * L, C)}, the {f} cycles after the "
                             f"prompt, got {getattr(x_true, 'dtype', type(x_true))} "
                             f"{tuple(getattr(x_true, 'shape', ()))}")
        if Q < 2:
            raise ValueError("forecast_cycles: the coverage of x_true needs at least two quantiles (the band's edges), "
                             f"got {Q}")
    start = decoder.n_classes - 2
    kw = {} if dtype is None else dict(dtype=dtype)          # encode_ids' own default is exact fp32
    prompt_ids = tokenize.encode_ids(vqvae, x_prompt, **kw)
    x = torch.cat([torch.full_like(prompt_ids[:, :1], start), prompt_ids], dim=1)
    out, lp = decoder.sample_ids(x, f * S, N, top_k=top_k, temperature=temperature, valid_ids=start, seed=seed,
                                 top_p=top_p, min_p=min_p, return_logp=True)
    ids = out[:, :, 1:].contiguous()
    x_prompt_hat = tokenize.decode_ids(vqvae, prompt_ids, dtype=dtype)
    x_hat = tokenize.decode_ids(vqvae, ids[:, :, c * S:].reshape(B * N, f * S), dtype=dtype).view(B, N, f * L, C)
    dev = x_hat.device
    M = f * L * C
    mean, std = torch.empty(B, f * L, C, device=dev), torch.empty(B, f * L, C, device=dev)
    quant = torch.empty(B, Q, f * L, C, device=dev)
    res = {"ids": ids, "x_prompt_hat": x_prompt_hat, "x_hat": x_hat,
           "sample_cycle_nll": -lp["logp"].view(B, N, f, S).sum(-1), "mean": mean, "std": std, "quantiles": quant}
    y = crps = cover = None
    if x_true is not None:
        y = x_true.contiguous().view(B, M)
        crps, cover = torch.empty(B, f, device=dev), torch.empty(B, f, device=dev)
        res.update(crps=crps, coverage=cover)
    bad = torch.zeros(1, dtype=torch.int32, device=dev)
    K.ensemble_stats(x_hat.view(B, N, M), qs, mean=mean.view(B, M), std=std.view(B, M),
                     quant=quant.view(B, Q, M) if Q else None, y=y, seg=L * C, crps=crps, cover=cover, bad_count=bad)
    nbad = int(bad.item())
    if nbad:
        raise RuntimeError(f"forecast_cycles: {nbad} points hold a non-finite sample or a non-finite x_true value")
    return res


@torch.no_grad()
def score_cycles(vqvae, decoder, x, dtype=None):
    """How well the two trained models explain measured cycles: x (B, n*L, C) f32, n >= 1 whole cycles ->

      ids (B, n*S) int64      logp, entropy (B, n*S) f32      rank (B, n*S) int32
      cycle_nll (B, n) f32    recon_mse (B, n) f32            vq_mse (B, n) f32

    ids are the cycles' codebook ids (``encode_ids``).  logp / rank / entropy score every id under the Transformer
    given the ids before it (MyTransformerDecoder.score_ids, restricted to the codebook ids as ``continue_cycles``
    generates), cycle_nll is -logp summed over a cycle's S ids.  Cycle 0 is scored with only the start token as
    context, so its figures say less than those of the cycles after it.  recon_mse is the mean squared error of the
    VQ-VAE's reconstruction of each cycle (``decode_ids`` of its ids), vq_mse that between the encoder output and the
    codebook rows it was quantised to -- for the plain VectorQuantizer what ``forward_ood``'s loss_OOD is for the
    residual one.

    The Transformer must fit the VQ-VAE as in ``continue_cycles`` (seq_len = n_cycles*S + 1, n_classes = K + 2) with
    n <= n_cycles; scoring fewer cycles gives the first cycles' scores of the full run.  ``dtype``: the VQ-VAE's
    operand dtype on both ways (None: exact fp32 ids, the process setting for the way back).  One encoder pass, one
    Transformer forward, one aw_score_rows launch, one decoder pass and two aw_window_sqerr launches."""
    if getattr(vqvae, "use_improved_vq", False):
        raise ValueError("score_cycles: use_improved_vq=True is not supported (the EMA residual quantizer keeps no "
                         "codebook parameter to decode the ids with or to measure the quantisation error against)")
    S = tokenize.ids_per_window(vqvae)
    L, Kc, D = vqvae.seq_len, vqvae.num_embeddings, vqvae.embedding_dim
    if (decoder.seq_len - 1) % S or decoder.seq_len <= S or decoder.n_classes != Kc + 2:
        raise ValueError(f"score_cycles: the Transformer (seq_len {decoder.seq_len}, n_classes {decoder.n_classes}) "
                         f"does not fit this VQ-VAE: it needs seq_len = n_cycles*S + 1 with S = {S} and n_classes = "
                         f"num_embeddings + 2 = {Kc + 2}")
    n_model = (decoder.seq_len - 1) // S
    if (not isinstance(x, torch.Tensor) or x.dtype != torch.float32 or x.dim() != 3 or x.shape[2] != vqvae.input_dim
            or x.shape[1] % L or not L <= x.shape[1] <= n_model * L):
        raise ValueError(f"score_cycles: x must be float32 (B, n*{L}, {vqvae.input_dim}) with 1 <= n <= n_cycles = "
                         f"{n_model}, got {getattr(x, 'dtype', type(x))} {tuple(getattr(x, 'shape', ()))}")
    from . import kernels as K
    from . import vqvae as engine
    B, n = x.shape[0], x.shape[1] // L
    x = x.contiguous()
    kw = {} if dtype is None else dict(dtype=dtype)          # encode's own default is exact fp32
    idx, z = engine.encode(vqvae, x.view(B * n, L, x.shape[2]), **kw)
    ids = idx.view(B, n * S)
    start = decoder.n_classes - 2
    seq = torch.cat([torch.full_like(ids[:, :1], start), ids], dim=1)
    sc = decoder.score_groups(seq, n, S, valid_ids=start, who="score_cycles")
    x_hat = tokenize.decode_ids(vqvae, ids, dtype=dtype)
    recon, vq = torch.empty(B, n, device=x.device), torch.empty(B, n, device=x.device)
    bad = torch.zeros(1, dtype=torch.int32, device=x.device)
    K.window_sqerr(x.view(B * n, L, x.shape[2]), x_hat.view(B * n, L, x.shape[2]), recon, bad)
    K.window_sqerr(z.view(B * n, S, D), vqvae.vector_quantization.embedding.weight.detach(), vq, bad,
                   idx=idx.view(B * n, S))
    nbad = int(bad.item())
    if nbad:        # not reachable from ids the encoder made: score_groups and decode_ids have checked them already
        raise RuntimeError(f"score_cycles: {nbad} ids lie outside the codebook [0, {Kc})")
    return {"ids": ids, "logp": sc["logp"], "rank": sc["rank"], "entropy": sc["entropy"], "cycle_nll": sc["group_nll"],
            "recon_mse": recon, "vq_mse": vq}
