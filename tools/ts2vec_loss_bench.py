#!/usr/bin/env python
"""Time the fused TS2Vec hierarchical contrastive loss (arcweld.ts2vec.hierarchical_contrastive_loss,
csrc/ts2vec_loss.hip), forward + backward, at the reference's training sizes: B = 16 views of T x 320 at T = 1000 and
T = 200, N(0, 0.05) inputs generated on the device (similarities of order 1).  The same loss restated in torch ops
(cat, matmul, masked_fill, logsumexp, max_pool1d; f32, 'highest' matmul precision, autograd) on the same GPU is timed
beside it -- the code under test is never compared against itself -- and the peak memory of both is recorded.

Each case is warmed up with a forward + backward of the same shape, then timed with device events over whole
forward + backward passes until at least ``--min-seconds`` have passed (at least ``--repeats`` passes); the median is
reported, the spread beside it.  ``--fit`` adds one training iteration's split at the reference's defaults (hidden 64,
output 320, depth 10, 2 input channels, both views the full length): the encoder's forward and backward on torch ops
against the loss.  Prints ONE JSON line:

  {"bench": "ts2vec_loss", "peak_tflops": 157.3, "results": [{"B", "T", "C", "flop", "flop_issued", "ms",
   "ms_minmax", "passes", "tflops", "frac_of_f32_mfma_peak", "peak_bytes", "peak_over_inputs", "torch_ms",
   "torch_ms_minmax", "torch_peak_bytes", "torch_over_hip", "loss_abs_diff", "grad_max_abs_diff"}, ...],
   "fit_split": {...}}

flop counts the dot products the algorithm needs: per term 2 G (2N)^2 C for S in the forward, and in the backward S
again (it is recomputed, never stored) plus Q . Z, three times the forward's in all.  flop_issued adds what the
backward's slabs of 128 output columns recompute: S once per slab, and Q . Z over whole slabs.  tflops is flop over
the median time of forward + backward: an end-to-end rate of the loss, launches and the max-pools included, not one
kernel's share of peak.  Needs the GPU; there is no CPU path.
"""
import argparse
import json
import os
import statistics
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "vq-vae-transformer-arc-welding_amd"))

import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

PEAK_TFLOPS = 157.3        # f32-input MFMA, MI355X
SLAB = 128


def terms(B, T, alpha=0.5, temporal_unit=0):
    """(G, N) of every term of the hierarchy that is computed (a pair alone in its group is skipped)."""
    out, d = [], 0
    while T > 1:
        if alpha != 0 and B > 1:
            out.append((T, B))
        if d >= temporal_unit and 1 - alpha != 0:
            out.append((B, T))
        d, T = d + 1, T // 2
    if alpha != 0 and B > 1:
        out.append((1, B))
    return out


def flops(B, T, C):
    s = sum(2.0 * G * (2 * N) ** 2 * C for G, N in terms(B, T))
    slabs = -(-C // SLAB)
    return 3.0 * s, s * (1 + slabs + slabs * SLAB / C)


def torch_nce(z1, z2, layout):
    Z = torch.cat([z1, z2], dim=1) if layout == "temporal" else torch.cat([z1, z2], dim=0).transpose(0, 1)
    n2 = Z.shape[1]
    S = Z @ Z.transpose(1, 2)
    lse = torch.logsumexp(S.masked_fill(torch.eye(n2, dtype=torch.bool, device=Z.device), float("-inf")), dim=-1)
    i = torch.arange(n2, device=Z.device)
    return (lse - S[:, i, (i + n2 // 2) % n2]).mean()


def torch_loss(z1, z2, alpha=0.5, temporal_unit=0):
    total, d = z1.new_zeros(()), 0
    while z1.shape[1] > 1:
        if alpha != 0 and z1.shape[0] > 1:
            total = total + alpha * torch_nce(z1, z2, "instance")
        if d >= temporal_unit and 1 - alpha != 0:
            total = total + (1 - alpha) * torch_nce(z1, z2, "temporal")
        d += 1
        z1 = F.max_pool1d(z1.transpose(1, 2), kernel_size=2).transpose(1, 2)
        z2 = F.max_pool1d(z2.transpose(1, 2), kernel_size=2).transpose(1, 2)
    if alpha != 0 and z1.shape[0] > 1:
        total = total + alpha * torch_nce(z1, z2, "instance")
    return total / (d + 1)


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    out = fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1), out


def measure(fn, repeats, min_seconds):
    """(times in ms, last result, peak bytes above what was allocated before)."""
    fn()
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    ts, total, out = [], 0.0, None
    while len(ts) < repeats or total < min_seconds * 1e3:
        out = None
        ms, out = timed(fn)
        ts.append(ms)
        total += ms
    torch.cuda.synchronize()
    return ts, out, torch.cuda.max_memory_allocated() - base


def fwd_bwd(loss_fn, z1, z2):
    def run():
        z1.grad = z2.grad = None
        loss = loss_fn(z1, z2)
        loss.backward()
        return loss.detach(), z1.grad, z2.grad
    return run


def fit_split(dev, B, T, repeats, seed):
    """One iteration at the reference's defaults, stage by stage (device events; medians over `repeats`)."""
    from arcweld.ts2vec import TSEncoder, hierarchical_contrastive_loss
    torch.manual_seed(seed)
    net = TSEncoder(2, 320, hidden_dims=64, depth=10).to(dev).train()
    opt = torch.optim.AdamW(net.parameters(), lr=1e-3)
    x = torch.randn(B, T, 2, device=dev)
    stages = {k: [] for k in ("encoder_forward", "loss_forward", "loss_backward", "encoder_backward", "optimizer")}
    for it in range(repeats + 1):
        opt.zero_grad()
        t_ef, (o1, o2) = timed(lambda: (net.train_forward(x), net.train_forward(x)))
        t_lf, loss = timed(lambda: hierarchical_contrastive_loss(o1, o2))
        t_lb, (g1, g2) = timed(lambda: torch.autograd.grad(loss, (o1, o2)))
        t_eb, _ = timed(lambda: torch.autograd.backward((o1, o2), (g1, g2)))
        t_op, _ = timed(opt.step)
        if it:                                   # the first iteration warms up
            for k, v in zip(stages, (t_ef, t_lf, t_lb, t_eb, t_op)):
                stages[k].append(v)
    med = {k: round(statistics.median(v), 3) for k, v in stages.items()}
    total = sum(med.values())
    return {"B": B, "T": T, "iterations": repeats, "ms": med, "ms_total": round(total, 3),
            "loss_share": round((med["loss_forward"] + med["loss_backward"]) / total, 4),
            "encoder_backward_share": round(med["encoder_backward"] / total, 4)}


def main():
    p = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    p.add_argument("--batch", type=int, default=16)
    p.add_argument("--lengths", type=int, nargs="+", default=[1000, 200])
    p.add_argument("--width", type=int, default=320)
    p.add_argument("--repeats", type=int, default=5)
    p.add_argument("--min-seconds", type=float, default=0.5)
    p.add_argument("--seed", type=int, default=0)
    p.add_argument("--fit", action="store_true", help="also time one training iteration's stages")
    p.add_argument("--out", type=str, default="", help="also write the JSON line to this file")
    a = p.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("ts2vec_loss_bench needs the GPU: a CPU run says nothing about the kernels")
    from arcweld.ts2vec import hierarchical_contrastive_loss
    torch.set_float32_matmul_precision("highest")
    dev = torch.device("cuda", torch.cuda.current_device())
    results = []
    for T in a.lengths:
        g = torch.Generator(device=dev).manual_seed(a.seed + T)
        B, C = a.batch, a.width
        z1 = (torch.randn(B, T, C, device=dev, generator=g) * 0.05).requires_grad_(True)
        z2 = (0.5 * z1.detach() + torch.randn(B, T, C, device=dev, generator=g) * 0.05).requires_grad_(True)
        ts, got, peak = measure(fwd_bwd(hierarchical_contrastive_loss, z1, z2), a.repeats, a.min_seconds)
        got = tuple(t.clone() for t in got)
        tt, want, tpeak = measure(fwd_bwd(torch_loss, z1, z2), a.repeats, a.min_seconds)
        flop, issued = flops(B, T, C)
        med, tmed = statistics.median(ts), statistics.median(tt)
        tflops = flop / (med * 1e-3) / 1e12
        inputs = 2 * z1.numel() * 4
        results.append({"B": B, "T": T, "C": C, "flop": flop, "flop_issued": issued, "ms": round(med, 3),
                        "ms_minmax": [round(min(ts), 3), round(max(ts), 3)], "passes": len(ts),
                        "tflops": round(tflops, 2), "frac_of_f32_mfma_peak": round(tflops / PEAK_TFLOPS, 4),
                        "peak_bytes": peak, "peak_over_inputs": round(peak / inputs, 2),
                        "torch_ms": round(tmed, 3), "torch_ms_minmax": [round(min(tt), 3), round(max(tt), 3)],
                        "torch_peak_bytes": tpeak, "torch_over_hip": round(tmed / med, 3),
                        "loss_abs_diff": abs(float(got[0]) - float(want[0])),
                        "grad_max_abs_diff": max(float((got[i] - want[i]).abs().max()) for i in (1, 2))})
        del z1, z2, got, want
    out = {"bench": "ts2vec_loss", "peak_tflops": PEAK_TFLOPS, "results": results}
    if a.fit:
        out["fit_split"] = fit_split(dev, a.batch, a.lengths[0], a.repeats, a.seed)
    line = json.dumps(out)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
