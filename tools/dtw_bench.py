#!/usr/bin/env python
"""Time the DTW k-NN search (arcweld.kernels.dtw_knn, csrc/dtw.hip) at the probe's own sizes for the raw-cycle
baseline: nq = 2048 queries against nx = 16384 database rows of C = 2 channels, k = 1, at L = 1000 with radius 100
(n_cycles = 5, --band 0.1) and at L = 200 with radius 20; N(0, 1) features from a seed, generated on the device.

Each case is warmed up with a search of the same shape, then timed with device events over whole searches (sweep +
merge kernels) until at least ``--min-seconds`` have passed (at least ``--repeats`` searches); the median is reported,
the spread beside it.  Prints ONE JSON line:

  {"bench": "dtw_knn", "valu_per_cell": 7.5, "results": [{"L", "radius", "C", "k", "nq", "nx", "cells", "ms",
   "ms_minmax", "searches", "cells_per_s", "frac_of_valu_bound", "frac_of_lds_bound"}, ...]}

cells counts the band's cells of every (query, row) pair: nq nx (L (2 r + 1) - r (r + 1)).  The two bounds (DESIGN.md
4.19): the VALU bound is cells x ``--valu-per-cell`` vector instructions (counted in the kernel's ISA, C = 2: 7.5)
over the chip's issue rate, 256 CUs x 4 SIMDs x one wave64 instruction per 2 cycles at 2.4 GHz; the LDS bound is
cells x ``--lds-cycles-per-cell`` LDS cycles per wave-instruction-cell (8: a broadcast ds_read_b64, half a
ds_read2st64_b32 and half a ds_write2st64_b32, whose stores pay 4 cycles per dword) at one LDS pipe per CU.
Needs the GPU; there is no CPU path.
"""
import argparse
import json
import os
import statistics
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "vq-vae-transformer-arc-welding_amd"))

import torch  # noqa: E402

CUS, GHZ = 256, 2.4


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    out = fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1), out


def main():
    p = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    p.add_argument("--nq", type=int, default=2048)
    p.add_argument("--nx", type=int, default=16384)
    p.add_argument("--channels", type=int, default=2)
    p.add_argument("--k", type=int, default=1)
    p.add_argument("--cases", type=str, nargs="+", default=["1000:100", "200:20"], help="L:radius")
    p.add_argument("--repeats", type=int, default=3)
    p.add_argument("--min-seconds", type=float, default=0.5)
    p.add_argument("--valu-per-cell", type=float, default=7.5)
    p.add_argument("--lds-cycles-per-cell", type=float, default=8.0)
    p.add_argument("--seed", type=int, default=0)
    p.add_argument("--out", type=str, default="", help="also write the JSON line to this file")
    a = p.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("dtw_bench needs the GPU: a CPU run says nothing about the kernel")
    from arcweld import kernels as K
    dev = torch.device("cuda", torch.cuda.current_device())
    valu_rate = CUS * 4 * 64 / 2 * GHZ * 1e9 / a.valu_per_cell            # cells per second
    lds_rate = CUS * 64 / a.lds_cycles_per_cell * GHZ * 1e9
    results = []
    for case in a.cases:
        L, r = (int(v) for v in case.split(":"))
        C = a.channels
        g = torch.Generator(device=dev).manual_seed(a.seed + L)
        q = torch.randn(a.nq, L * C, device=dev, generator=g)
        x = torch.randn(a.nx, L * C, device=dev, generator=g)
        run = lambda: K.dtw_knn(q, x, L, C, r, a.k)       # noqa: E731
        run()
        torch.cuda.synchronize()
        ts, total = [], 0.0
        while len(ts) < a.repeats or total < a.min_seconds * 1e3:
            ms, _ = timed(run)
            ts.append(ms)
            total += ms
        cells = float(a.nq) * a.nx * (L * (2 * r + 1) - r * (r + 1))
        med = statistics.median(ts)
        rate = cells / (med * 1e-3)
        results.append({"L": L, "radius": r, "C": C, "k": a.k, "nq": a.nq, "nx": a.nx, "cells": cells,
                        "ms": round(med, 3), "ms_minmax": [round(min(ts), 3), round(max(ts), 3)], "searches": len(ts),
                        "cells_per_s": float(f"{rate:.4g}"), "frac_of_valu_bound": round(rate / valu_rate, 4),
                        "frac_of_lds_bound": round(rate / lds_rate, 4)})
        del q, x
    line = json.dumps({"bench": "dtw_knn", "valu_per_cell": a.valu_per_cell,
                       "lds_cycles_per_cell": a.lds_cycles_per_cell, "results": results})
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
