"""Generation path at the reference defaults (Transformer d 512, 8 blocks, 8 heads, T = 321, V = 514, B = 16; VQ-VAE
H 512, 8 ResBlocks, codebook 512 x 64; bf16 operands): us per token of the existing ``generate(use_cache=True)`` greedy
loop and of ``generate_ids``, aw_sample_next alone at V = 514 and 8194, and ``decode_ids`` of 1024 windows beside the
eval ``forward`` of the same windows.  HIP events, 3 warm-up calls.

The prompt is the start token alone (L0 = 1), so none of ``generate``'s seq_len steps runs on a cropped context: every
step of both loops is one cached decode step plus the token choice.
usage: python tools/probe/generate_probe.py [iters]"""
import sys

import torch

sys.path.insert(0, "vq-vae-transformer-arc-welding_amd")
from arcweld import kernels as K  # noqa: E402
from arcweld.precision import operands  # noqa: E402
from model.transformer_decoder import MyTransformerDecoder  # noqa: E402
from model.vq_vae_patch_embedd import VQVAEPatch  # noqa: E402

B, T, V, D_MODEL, BLOCKS, HEADS = 16, 321, 514, 512, 8, 8
WINDOWS = 1024


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
    vq = VQVAEPatch(hidden_dim=512, input_dim=2, num_embeddings=512, embedding_dim=64, n_resblocks=8,
                    learning_rate=1e-3, dropout_p=0.1, patch_size=25, batch_norm=False).to(dev).eval()
    start = torch.full((B, 1), V - 2, dtype=torch.int64, device=dev)
    print(f"{torch.cuda.get_device_name(0)}  B {B}  T {T}  V {V}  d {D_MODEL}  blocks {BLOCKS}  bf16 operands "
          f"({iters} iterations)", flush=True)
    with operands(torch.bfloat16):
        t_gen = timed(lambda: dec.generate(start, use_cache=True), iters)
        print(f"generate(use_cache=True), greedy, {T} uncropped steps: {t_gen / T:.1f} us per token", flush=True)
        for kw, tag in ((dict(), "greedy"), (dict(valid_ids=V - 2), "greedy, ids < K"),
                        (dict(do_sample=True, top_k=50, valid_ids=V - 2), "sampled, top_k 50, ids < K")):
            t_ids = timed(lambda: dec.generate_ids(start, T - 1, **kw), iters)
            print(f"generate_ids, {tag}, {T - 1} steps: {t_ids / (T - 1):.1f} us per token", flush=True)

        for v in (514, 8194):
            lg = torch.randn(B, v, device=dev) * 3
            out = torch.empty(B, 1, dtype=torch.int64, device=dev)
            bad = torch.zeros(1, dtype=torch.int32, device=dev)
            for kw, tag in ((dict(), "greedy"), (dict(do_sample=True), "sampled"),
                            (dict(do_sample=True, top_k=50), "sampled, top_k 50")):
                t = timed(lambda: K.sample_next(lg, out, 0, bad, n_valid=v - 2, **kw), 200)
                print(f"aw_sample_next V {v} B {B}, {tag}: {t:.1f} us per launch, back to back on one stream",
                      flush=True)

        x = torch.randn(WINDOWS, 200, 2, device=dev)
        with torch.no_grad():
            ids = vq.encode_ids(x)
            t_fwd = timed(lambda: vq(x), 4 * iters)
        t_dec = timed(lambda: vq.decode_ids(ids), 4 * iters)
        print(f"{WINDOWS} windows: decode_ids {t_dec:.0f} us, eval forward {t_fwd:.0f} us", flush=True)


if __name__ == "__main__":
    main(int(sys.argv[1]) if len(sys.argv) > 1 else 5)
