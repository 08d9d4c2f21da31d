#!/usr/bin/env python
"""Time the TS2Vec encoder's eval forward (arcweld.ts2vec.TSEncoder.encode, csrc/ts2vec.hip) at the probe's own
sizes: n = 16384 sequences of T x 2 at T = 1000 (n_cycles = 5) and T = 200, the reference's default widths (hidden 64,
output 320, depth 10), encoding_window='full_series'; N(0, 1) inputs and nn.Conv1d-like seeded weights, generated on
the device.  The same forward restated in torch ops (F.linear, F.gelu, F.conv1d; f32, 'highest' matmul precision) on
the same GPU is timed beside it, on ``--torch-sequences`` sequences in chunks of ``--torch-chunk`` (the (B, C, T)
intermediates of the op-by-op forward bound its batch), and compared per sequence.

Each case is warmed up with an encode of the same shape, then timed with device events over whole encodes until at
least ``--min-seconds`` have passed (at least ``--repeats`` encodes); the median is reported, the spread beside it.
Prints ONE JSON line:

  {"bench": "ts2vec_encode", "peak_tflops": 157.3, "results": [{"T", "n", "flop", "ms", "ms_minmax", "encodes",
   "tflops", "frac_of_f32_mfma_peak", "us_per_sequence", "torch_n", "torch_ms", "torch_us_per_sequence",
   "torch_over_hip", "max_abs_diff"}, ...]}

flop counts the multiply-adds that touch real input: per convolution 2 cout cin (T + 2 max(T - d, 0)) per sequence (a
tap loses d steps at its edge and vanishes at d >= T), the projector and input_fc at 2 cout cin T.  torch_over_hip is
the torch time per sequence over the kernels' time per sequence (above 1: the kernels are faster); max_abs_diff
compares the two outputs on the torch run's sequences.  Needs the GPU; there is no CPU path.
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


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    out = fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1), out


def measure(fn, repeats, min_seconds):
    fn()
    torch.cuda.synchronize()
    ts, total, out = [], 0.0, None
    while len(ts) < repeats or total < min_seconds * 1e3:
        ms, out = timed(fn)
        ts.append(ms)
        total += ms
    return ts, out


def flop_per_sequence(enc, T):
    H, Co, Ci = enc.hidden_dims, enc.output_dims, enc.input_dims
    total = 2.0 * H * Ci * T
    for i in range(enc.depth + 1):
        d = 2 ** i
        live = T + 2 * max(T - d, 0)
        cout = Co if i == enc.depth else H
        total += 2.0 * cout * H * live + 2.0 * cout * cout * live
        if i == enc.depth:
            total += 2.0 * Co * H * T
    return total


@torch.no_grad()
def torch_forward(enc, x, chunk):
    """The eval forward op by op, pooled over time: (n, T, C) -> (n, C_out)."""
    out = []
    for o in range(0, x.shape[0], chunk):
        xb = x[o:o + chunk]
        keep = ~torch.isnan(xb).any(-1, keepdim=True)
        h = F.linear(torch.where(keep, xb, torch.zeros_like(xb)), enc.input_fc.weight, enc.input_fc.bias)
        h = torch.where(keep, h, torch.zeros_like(h)).transpose(1, 2)
        for i, blk in enumerate(enc.feature_extractor.net):
            d = 2 ** i
            res = h if blk.projector is None else F.conv1d(h, blk.projector.weight, blk.projector.bias)
            u = F.conv1d(F.gelu(h), blk.conv1.conv.weight, blk.conv1.conv.bias, padding=d, dilation=d)
            u = F.conv1d(F.gelu(u), blk.conv2.conv.weight, blk.conv2.conv.bias, padding=d, dilation=d)
            h = u + res
        out.append(h.amax(2))
    return torch.cat(out)


def main():
    p = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    p.add_argument("--n", type=int, default=16384)
    p.add_argument("--lengths", type=int, nargs="+", default=[1000, 200])
    p.add_argument("--channels", type=int, default=2)
    p.add_argument("--hidden", type=int, default=64)
    p.add_argument("--output", type=int, default=320)
    p.add_argument("--depth", type=int, default=10)
    p.add_argument("--torch-sequences", type=int, default=2048)
    p.add_argument("--torch-chunk", type=int, default=128)
    p.add_argument("--repeats", type=int, default=3)
    p.add_argument("--min-seconds", type=float, default=0.5)
    p.add_argument("--seed", type=int, default=0)
    p.add_argument("--out", type=str, default="", help="also write the JSON line to this file")
    a = p.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("ts2vec_bench needs the GPU: a CPU run says nothing about the kernels")
    from arcweld.ts2vec import TSEncoder
    torch.set_float32_matmul_precision("highest")
    dev = torch.device("cuda", torch.cuda.current_device())
    torch.manual_seed(a.seed)
    enc = TSEncoder(a.channels, a.output, hidden_dims=a.hidden, depth=a.depth).to(dev).eval()
    results = []
    for T in a.lengths:
        g = torch.Generator(device=dev).manual_seed(a.seed + T)
        x = torch.randn(a.n, T, a.channels, device=dev, generator=g)
        ts, got = measure(lambda: enc.encode(x, encoding_window="full_series"), a.repeats, a.min_seconds)
        nt = min(a.torch_sequences, a.n)
        tt, want = measure(lambda: torch_forward(enc, x[:nt], a.torch_chunk), a.repeats, a.min_seconds)
        flop = flop_per_sequence(enc, T) * a.n
        med, tmed = statistics.median(ts), statistics.median(tt)
        tflops = flop / (med * 1e-3) / 1e12
        us, tus = med * 1e3 / a.n, tmed * 1e3 / nt
        results.append({"T": T, "n": a.n, "flop": flop, "ms": round(med, 3),
                        "ms_minmax": [round(min(ts), 3), round(max(ts), 3)], "encodes": len(ts),
                        "tflops": round(tflops, 2), "frac_of_f32_mfma_peak": round(tflops / PEAK_TFLOPS, 4),
                        "us_per_sequence": round(us, 3), "torch_n": nt, "torch_ms": round(tmed, 3),
                        "torch_us_per_sequence": round(tus, 3), "torch_over_hip": round(tus / us, 3),
                        "max_abs_diff": float((got[:nt] - want).abs().max())})
        del x, got, want
    line = json.dumps({"bench": "ts2vec_encode", "peak_tflops": PEAK_TFLOPS, "hidden": a.hidden, "output": a.output,
                       "depth": a.depth, "results": results})
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
