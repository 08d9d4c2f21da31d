"""Ensemble forecast at the workload shape.  Part 1: us per launch of aw_ensemble_stats at G = 8 prompts, N = 32 samples,
M = 19 * 400 points (19 forecast cycles of 200 x 2) with three quantiles and a truth, next to the torch composition it
replaces on the device (mean, std, quantile, a sort for the CRPS pair term, the per-cycle sums) and to one read of x
(x.sum(): the bandwidth yardstick); the first line checks the kernel against the composition.  Part 2: ms per call of
MyTransformerDecoder.sample_ids (one prefill on 8 rows, the cache fanned out to 256) against generate_ids on the prompt
repeated 32 times (the prefill on 256 rows), one prompt cycle and 19 generated ones at the full-size decoder, and
whether the two return the same ids.  HIP events around back-to-back calls on one stream after a warm-up, the candidates
alternating over several rounds in one process.
usage: python tools/probe/ensemble_probe.py [launches per round] [rounds] [generation calls per round]"""
import sys

import torch

sys.path.insert(0, "vq-vae-transformer-arc-welding_amd")
from arcweld import kernels as K  # noqa: E402

G, N, CYC, SEG, S, KC = 8, 32, 19, 400, 16, 512
M = CYC * SEG
QS = (0.05, 0.5, 0.95)


def timed(fn, iters, warm):
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


def report(res, unit, scale):
    for name, ts in res.items():
        ts = sorted(t * scale for t in ts)
        print(f"{name:34s} median {ts[len(ts) // 2]:9.1f} {unit}   min {ts[0]:9.1f}   max {ts[-1]:9.1f}", flush=True)


def stats_part(iters, rounds):
    dev = "cuda"
    torch.manual_seed(0)
    x = torch.randn(G, N, M, device=dev)
    y = torch.randn(G, M, device=dev)
    mean, std = torch.empty(G, M, device=dev), torch.empty(G, M, device=dev)
    quant = torch.empty(G, len(QS), M, device=dev)
    crps, cover = torch.empty(G, CYC, device=dev), torch.empty(G, CYC, device=dev)
    bad = torch.zeros(1, dtype=torch.int32, device=dev)
    qt = torch.tensor(QS, device=dev)
    w = (2.0 * torch.arange(1, N + 1, device=dev) - N - 1).view(1, N, 1)

    def kernel():
        K.ensemble_stats(x, QS, mean=mean, std=std, quant=quant, y=y, seg=SEG, crps=crps, cover=cover, bad_count=bad)

    def composed():
        q = torch.quantile(x, qt, dim=1).movedim(0, 1)
        c = (x - y[:, None]).abs().mean(1) - (w * x.sort(dim=1).values).sum(1) / N ** 2
        inside = ((q[:, 0] <= y) & (y <= q[:, -1])).float()
        return x.mean(1), x.std(1), q, c.view(G, CYC, SEG).mean(-1), inside.view(G, CYC, SEG).mean(-1)

    kernel()
    mu, sd, q, c, cv = composed()
    print(f"aw_ensemble_stats  G {G}  N {N}  M {M} = {CYC} x {SEG}  Q {len(QS)}  ({iters} launches x {rounds} rounds); "
          f"x is {x.numel() * 4 / 2 ** 20:.1f} MiB", flush=True)
    print(f"kernel vs composition: max |mean| diff {(mu - mean).abs().max().item():.2e}, |std| "
          f"{(sd - std).abs().max().item():.2e}, |quant| {(q - quant).abs().max().item():.2e}, |crps| "
          f"{(c - crps).abs().max().item():.2e}, |cover| {(cv - cover).abs().max().item():.2e}, bad {int(bad.item())}",
          flush=True)
    cands = (("aw_ensemble_stats", kernel, iters), ("x.sum() (one read of x)", lambda: x.sum(), iters),
             ("torch composition", composed, max(iters // 10, 20)))
    res = {name: [] for name, _, _ in cands}
    for _ in range(rounds):
        for name, fn, n in cands:
            res[name].append(timed(fn, n, 20))
    report(res, "us", 1.0)


def generation_part(calls, rounds):
    from model.transformer_decoder import MyTransformerDecoder
    from arcweld.precision import operands
    torch.manual_seed(1)
    n_cycles = CYC + 1
    d = MyTransformerDecoder(d_model=512, n_classes=KC + 2, seq_len=n_cycles * S + 1, n_blocks=6, n_head=8)
    with torch.no_grad():
        d.lm_head.weight.mul_(10.0)
    d = d.cuda().eval()
    x = torch.randint(0, KC, (G, 1 + S), device="cuda")
    x[:, 0] = KC
    n_new = CYC * S
    kw = dict(top_k=50, valid_ids=KC, seed=3)
    with operands(torch.float32):
        a = d.sample_ids(x, n_new, N, **kw)
        b = d.generate_ids(x.repeat_interleave(N, 0), n_new, do_sample=True, **kw)
        print(f"sample_ids vs generate_ids on the repeated prompt: B {G}  N {N}  L0 {1 + S}  n_new {n_new}  d_model 512, "
              f"6 blocks; same ids: {torch.equal(a.view(G * N, -1), b)}  ({calls} calls x {rounds} rounds)", flush=True)
        cands = (("sample_ids (prefill on 8 rows)", lambda: d.sample_ids(x, n_new, N, **kw)),
                 ("generate_ids (prompt x 32)", lambda: d.generate_ids(x.repeat_interleave(N, 0), n_new, do_sample=True,
                                                                      **kw)))
        res = {name: [] for name, _ in cands}
        for _ in range(rounds):
            for name, fn in cands:
                res[name].append(timed(fn, calls, 1))
    report(res, "ms", 1e-3)


def main(iters=1000, rounds=5, calls=3):
    print(torch.cuda.get_device_name(0), flush=True)
    stats_part(iters, rounds)
    generation_part(calls, rounds)


if __name__ == "__main__":
    main(*(int(a) for a in sys.argv[1:4]))
