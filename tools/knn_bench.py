#!/usr/bin/env python
"""Time the fused k-NN search (arcweld.kernels.knn, csrc/knn.hip) against the three-line alternative in torch.

Shape: the latent probe's own -- nq = 8192 queries against nx = 131072 database rows, k = 1 and k = 5, at D = 5120
(latent_vq_vae: 5 cycles x 16 x 64) and D = 2000 (raw cycles); N(0, 1) features from a seed, generated on the device.
Baseline, same process and device: chunked ``torch.cdist(q, x) ** 2`` + ``torch.topk(largest=False)`` in f32, the
query chunk sized to 1 GiB of distances.  Both sides are warmed up, then timed alternately with device events
(``--repeats`` times each; the median is reported, the spread beside it).  Prints ONE JSON line:

  {"bench": "knn", "peak_tflops": 157.3, "results": [{"D", "k", "nq", "nx", "knn_ms", "knn_ms_minmax", "torch_ms",
   "torch_ms_minmax", "ratio_torch_over_knn", "knn_tflops", "knn_frac_of_f32_matrix_peak", "idx_agree"}, ...]}

knn_tflops counts the 2 nq nx D operations of the dot products over the whole call (sweep + merge kernels);
idx_agree is the share of (query, slot) pairs where both sides name the same neighbour (they round differently, so
near-ties may swap).  Needs the GPU; there is no CPU path.
"""
import argparse
import json
import os
import statistics
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "vq-vae-transformer-arc-welding_amd"))

import torch  # noqa: E402

PEAK_F32_MATRIX_TFLOPS = 157.3


def torch_knn(q, x, k, chunk):
    idx, dist = [], []
    for o in range(0, q.shape[0], chunk):
        d = torch.cdist(q[o:o + chunk], x) ** 2
        v, i = torch.topk(d, k, dim=1, largest=False)
        idx.append(i)
        dist.append(v)
    return torch.cat(idx), torch.cat(dist)


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    out = fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1), out


def main():
    p = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    p.add_argument("--nq", type=int, default=8192)
    p.add_argument("--nx", type=int, default=131072)
    p.add_argument("--dims", type=int, nargs="+", default=[5120, 2000])
    p.add_argument("--ks", type=int, nargs="+", default=[1, 5])
    p.add_argument("--warmup", type=int, default=1)
    p.add_argument("--repeats", type=int, default=5)
    p.add_argument("--seed", type=int, default=0)
    p.add_argument("--out", type=str, default="", help="also write the JSON line to this file")
    a = p.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("knn_bench needs the GPU: a CPU run says nothing about the kernel")
    from arcweld import kernels as K
    torch.backends.cuda.matmul.allow_tf32 = False
    torch.set_float32_matmul_precision("highest")
    dev = torch.device("cuda", torch.cuda.current_device())
    chunk = max(1, (1 << 30) // (4 * a.nx))
    results = []
    for D in a.dims:
        g = torch.Generator(device=dev).manual_seed(a.seed + D)
        q = torch.randn(a.nq, D, device=dev, generator=g)
        x = torch.randn(a.nx, D, device=dev, generator=g)
        for k in a.ks:
            ours = lambda: K.knn(q, x, k)               # noqa: E731
            theirs = lambda: torch_knn(q, x, k, chunk)  # noqa: E731
            for _ in range(a.warmup):
                ours(), theirs()
            torch.cuda.synchronize()
            t_o, t_t = [], []
            for _ in range(a.repeats):
                ms, (idx, _) = timed(ours)
                t_o.append(ms)
                ms, (tidx, _) = timed(theirs)
                t_t.append(ms)
            mo, mt = statistics.median(t_o), statistics.median(t_t)
            tf = 2.0 * a.nq * a.nx * D / (mo * 1e-3) / 1e12
            results.append({"D": D, "k": k, "nq": a.nq, "nx": a.nx, "knn_ms": round(mo, 3),
                            "knn_ms_minmax": [round(min(t_o), 3), round(max(t_o), 3)], "torch_ms": round(mt, 3),
                            "torch_ms_minmax": [round(min(t_t), 3), round(max(t_t), 3)],
                            "ratio_torch_over_knn": round(mt / mo, 4), "knn_tflops": round(tf, 2),
                            "knn_frac_of_f32_matrix_peak": round(tf / PEAK_F32_MATRIX_TFLOPS, 4),
                            "idx_agree": round(float((idx == tidx).float().mean()), 6)})
        del q, x
    line = json.dumps({"bench": "knn", "peak_tflops": PEAK_F32_MATRIX_TFLOPS, "warmup": a.warmup,
                       "repeats": a.repeats, "baseline_chunk_rows": chunk, "results": results})
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
