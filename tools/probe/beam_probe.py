"""Beam search at the reference defaults (Transformer d 512, 8 blocks, 8 heads, T = 321, V = 514, bf16 operands):
us per token of greedy ``generate_ids`` at 16 and at 128 rows, of ``beam_search_ids`` at B 16 with 4 and 8 beams (64 and
128 decode rows), of aw_beam_step alone and of aw_beam_gather alone at n_pos 160 (with the bytes it moves), and one
cached decode step at position 160 on the same rows to set the two launches against.  HIP events, 3 warm-up calls.

The prompt is the start token alone (L0 = 1) and every loop generates T - 1 tokens, so the gather's n_pos averages
T / 2.  The comparison that matters is beam search at B * W rows against greedy at the same number of rows: the
difference is what the two new launches (and the wider token slabs) cost.
usage: python tools/probe/beam_probe.py [iters]"""
import sys

import torch

sys.path.insert(0, "vq-vae-transformer-arc-welding_amd")
from arcweld import decoder as engine  # noqa: E402
from arcweld import kernels as K  # noqa: E402
from arcweld.precision import operands  # noqa: E402
from model.transformer_decoder import MyTransformerDecoder  # noqa: E402

B, T, V, D_MODEL, BLOCKS, HEADS = 16, 321, 514, 512, 8, 8
N_POS = 160


def timed(fn, iters, warm=3):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    for _ in range(iters):
        fn()
    t1.record()
    torch.cuda.synchronize()
    return t0.elapsed_time(t1) / iters * 1e3


def main(iters=5):
    dev = "cuda"
    torch.manual_seed(0)
    dec = MyTransformerDecoder(d_model=D_MODEL, n_classes=V, seq_len=T, n_blocks=BLOCKS, n_head=HEADS).to(dev).eval()
    with torch.no_grad():
        dec.lm_head.weight.mul_(10.0)           # spread the logits: flat ones would make every candidate a near tie
    n_valid, n_new = V - 2, T - 1
    print(f"{torch.cuda.get_device_name(0)}  T {T}  V {V}  d {D_MODEL}  blocks {BLOCKS}  bf16 operands "
          f"({iters} iterations, {n_new} tokens per call)", flush=True)
    with operands(torch.bfloat16):
        greedy = {}
        for rows in (16, 64, 128):
            start = torch.full((rows, 1), V - 2, dtype=torch.int64, device=dev)
            greedy[rows] = timed(lambda: dec.generate_ids(start, n_new, valid_ids=n_valid), iters) / n_new
            print(f"generate_ids, greedy, ids < K, {rows} rows: {greedy[rows]:.1f} us per token", flush=True)
        start = torch.full((B, 1), V - 2, dtype=torch.int64, device=dev)
        for W in (4, 8):
            t = timed(lambda: dec.beam_search_ids(start, n_new, W, valid_ids=n_valid, num_return=W), iters) / n_new
            print(f"beam_search_ids, B {B}, {W} beams ({B * W} rows): {t:.1f} us per token, "
                  f"{t - greedy[B * W]:+.1f} against greedy at {B * W} rows", flush=True)

        for W in (4, 8, 32):
            lg = torch.randn(B * W, V, device=dev) * 3
            sc_in = torch.randn(B, W, device=dev)
            sc, lp = torch.empty(B, W, device=dev), torch.empty(B, W, device=dev)
            pa = torch.empty(B, W, dtype=torch.int32, device=dev)
            tk = torch.empty(B * W, dtype=torch.int64, device=dev)
            bad = torch.zeros(1, dtype=torch.int32, device=dev)
            t = timed(lambda: K.beam_step(lg, sc_in, sc, pa, tk, lp, bad, n_valid=n_valid), 500)
            print(f"aw_beam_step B {B}, W {W}, n_valid {n_valid}: {t:.1f} us per launch, back to back on one stream",
                  flush=True)

        for W in (4, 8):
            rows = B * W
            caches = [[torch.randn(rows, T, 2 * D_MODEL, device=dev).bfloat16() for _ in range(BLOCKS)]
                      for _ in range(2)]
            tab = list(K.beam_cache_table(caches))
            par = torch.randint(0, W, (B, W), dtype=torch.int32, device=dev)
            bad = torch.zeros(1, dtype=torch.int32, device=dev)
            flip = [0]

            def gather():
                s = flip[0]
                flip[0] ^= 1
                K.beam_gather(tab[s], tab[s ^ 1], B, W, par, T, N_POS, 2 * D_MODEL, torch.bfloat16, bad)

            t = timed(gather, 200)
            gb = 2 * rows * N_POS * 2 * D_MODEL * 2 * BLOCKS / 1e9
            print(f"aw_beam_gather {rows} rows, n_pos {N_POS}, {BLOCKS} blocks, bf16: {t:.1f} us per launch, "
                  f"{gb:.3f} GB read + written, {gb / t * 1e3:.2f} TB/s", flush=True)
            assert int(bad.item()) == 0
            del caches, tab

            cache = engine.KVCache(dec, rows, T)
            ids = torch.randint(0, n_valid, (rows, 1), device=dev)
            t_dec = timed(lambda: engine.forward_cached(dec, ids, cache, N_POS), 50)
            print(f"forward_cached, one token at position {N_POS}, {rows} rows: {t_dec:.1f} us; the gather is "
                  f"{100 * t / t_dec:.1f} % of it", flush=True)
            del cache


if __name__ == "__main__":
    main(int(sys.argv[1]) if len(sys.argv) > 1 else 5)
