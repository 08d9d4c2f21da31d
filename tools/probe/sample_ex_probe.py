"""What the nucleus / min-p / log-probability launch costs beside the plain one and beside the decode step it follows
(B = 16, V = 514, n_valid = 512, logits N(0, 3)): us per launch of
  (a) aw_sample_next, sampling, no top_k;
  (b) aw_sample_next_ex with nothing new switched on (top_p = 1, min_p = 0, no logp / logq);
  (c) aw_sample_next_ex with top_p = 0.9 and logp + logq;
  (c+) the same with top_k = 50 and min_p = 0.01 as well;
and of one cached decode step (arcweld.decoder.forward_cached, one new token at position 160, the workload decoder:
d 512, 8 blocks, 8 heads, T = 321, bf16 operands).  (c) is also timed at V = 8194 (the 16384-column instantiation,
33 columns per thread).  HIP events around back-to-back launches on one stream after a warm-up, the candidates
alternating over several rounds in one process; min / median / max over the rounds give the run-to-run spread.  The
first line checks (b) against (a) bit for bit.  A third argument is a regular expression that selects candidates by
name: under ``rocprofv3 --kernel-trace --stats`` (a run of its own) the kernel durations can then be told apart, since
(b), (c) and (c+) are one kernel.
usage: python tools/probe/sample_ex_probe.py [launches per round] [rounds] [name regex]"""
import re
import sys

import torch

sys.path.insert(0, "vq-vae-transformer-arc-welding_amd")
from arcweld import decoder as engine  # noqa: E402
from arcweld import kernels as K  # noqa: E402
from arcweld.precision import operands  # noqa: E402
from model.transformer_decoder import MyTransformerDecoder  # noqa: E402

B, T, V, D_MODEL, BLOCKS, HEADS, POS = 16, 321, 514, 512, 8, 8, 160


def timed(fn, iters, warm=20):
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


def main(iters=2000, rounds=5, only=""):
    dev = "cuda"
    torch.manual_seed(0)
    bad = torch.zeros(1, dtype=torch.int32, device=dev)
    out = torch.empty(B, 2, dtype=torch.int64, device=dev)
    lp = torch.empty(2, B, 1, device=dev)

    def plain(lg):
        return lambda: K.sample_next(lg, out, 0, bad, n_valid=lg.shape[1] - 2, do_sample=True, seed=1, step=3)

    def ex(lg, full, col=0, **kw):
        extra = dict(logp_out=lp[0], logq_out=lp[1]) if full else {}
        return lambda: K.sample_next_ex(lg, out, col, bad, n_valid=lg.shape[1] - 2, do_sample=True, seed=1, step=3,
                                        **extra, **kw)

    lg = torch.randn(B, V, device=dev) * 3
    wide = torch.randn(B, 8194, device=dev) * 3
    plain(lg)()
    ex(lg, False, col=1)()
    print(f"{torch.cuda.get_device_name(0)}  B {B}  V {V}  n_valid {V - 2}  ({iters} launches x {rounds} rounds)",
          flush=True)
    print(f"(b) ids equal (a) ids: {torch.equal(out[:, 0], out[:, 1])}, bad {int(bad.item())}", flush=True)

    dec = MyTransformerDecoder(d_model=D_MODEL, n_classes=V, seq_len=T, n_blocks=BLOCKS, n_head=HEADS).to(dev).eval()
    ids = torch.randint(0, V - 2, (B, POS + 1), device=dev)
    with operands(torch.bfloat16), torch.no_grad():
        cache = engine.KVCache(dec, B, T)
        engine.forward_cached(dec, ids[:, :POS], cache, 0)

        def decode():
            engine.forward_cached(dec, ids[:, POS:POS + 1], cache, POS)

        cands = (("(a) aw_sample_next", plain(lg), iters),
                 ("(b) _ex, nothing new on", ex(lg, False), iters),
                 ("(c) _ex top_p 0.9 + logp/logq", ex(lg, True, top_p=0.9), iters),
                 ("(c+) .. + top_k 50, min_p 0.01", ex(lg, True, top_p=0.9, top_k=50, min_p=0.01), iters),
                 ("(a) at V 8194", plain(wide), iters),
                 ("(c) at V 8194", ex(wide, True, top_p=0.9), iters),
                 ("cached decode step", decode, max(iters // 10, 20)))
        cands = [c for c in cands if re.search(only, c[0])]
        res = {name: [] for name, _, _ in cands}
        for _ in range(rounds):
            for name, fn, n in cands:
                res[name].append(timed(fn, n))
    for name, ts in res.items():
        ts = sorted(ts)
        print(f"{name:32s} median {ts[len(ts) // 2]:8.1f} us   min {ts[0]:8.1f}   max {ts[-1]:8.1f}", flush=True)


if __name__ == "__main__":
    main(*(int(a) for a in sys.argv[1:3]), *sys.argv[3:4])
