#!/usr/bin/env python
"""Time one loss + gradient evaluation of the batched logistic regression (arcweld.kernels.logreg_forward +
logreg_grad, csrc/logreg.hip) against its restatement in torch.

Shape: the latent probe's own -- n = 131072 rows at D = 5120 (latent_vq_vae: 5 cycles x 16 x 64) and D = 2000 (raw
cycles), P = 1, 8 and 32 problems; N(0, 1) features from a seed, generated on the device, w ~ N(0, 1 / D), labels 0 / 1.
Baseline, same process and device, f32: ``z = x @ w + b``, ``r = sigmoid(z) - t``, ``loss = sum softplus(z) - t z``,
``gb = r.sum(0)``, ``g = x.T @ r``.  Both sides are warmed up, then timed alternately with device events
(``--repeats`` times each; the median is reported, the spread beside it).  Prints ONE JSON line:

  {"bench": "logreg", "peak_tflops": 157.3, "results": [{"D", "P", "n", "ours_ms", "ours_ms_minmax", "fwd_ms",
   "grad_ms", "torch_ms", "torch_ms_minmax", "ratio_torch_over_ours", "gbps_two_reads_of_x", "tflops",
   "frac_of_f32_matrix_peak", "max_rel_diff_g"}, ...], "fit": {...}}

gbps_two_reads_of_x counts 2 * 4 n D bytes (the two-pass form reads X twice per evaluation), tflops the 4 n D P
operations of the two products.  ``--fit`` adds the wall time and the iteration counts of a whole
arcweld.retrieve.logreg_fit (StandardScaler included) at the probe's training shape: ``--fit-n`` rows (the probe's
max_samples) of D = 5120 features with labels from a random linear score plus logistic noise, C = 0.1, 1, 10.
Needs the GPU; there is no CPU path.
"""
import argparse
import json
import os
import statistics
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "vq-vae-transformer-arc-welding_amd"))

import torch  # noqa: E402

PEAK_F32_MATRIX_TFLOPS = 157.3


def torch_eval(x, w, b, t):
    z = x @ w + b
    r = torch.sigmoid(z) - t
    loss = (torch.nn.functional.softplus(z) - t * z).sum(0)
    return loss, r.sum(0), x.t() @ r


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    out = fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1), out


def main():
    p = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    p.add_argument("--n", type=int, default=131072)
    p.add_argument("--dims", type=int, nargs="+", default=[5120, 2000])
    p.add_argument("--ps", type=int, nargs="+", default=[1, 8, 32])
    p.add_argument("--warmup", type=int, default=2)
    p.add_argument("--repeats", type=int, default=7)
    p.add_argument("--seed", type=int, default=0)
    p.add_argument("--fit", action="store_true", help="also time a whole logreg_fit at D = 5120")
    p.add_argument("--fit-n", type=int, default=100000)
    p.add_argument("--out", type=str, default="", help="also write the JSON line to this file")
    a = p.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("logreg_bench needs the GPU: a CPU run says nothing about the kernels")
    from arcweld import kernels as K
    torch.backends.cuda.matmul.allow_tf32 = False
    torch.set_float32_matmul_precision("highest")
    dev = torch.device("cuda", torch.cuda.current_device())
    results = []
    for D in a.dims:
        g = torch.Generator(device=dev).manual_seed(a.seed + D)
        x = torch.randn(a.n, D, device=dev, generator=g)
        y = (torch.rand(a.n, device=dev, generator=g) < 0.5).to(torch.int32)
        for P in a.ps:
            w = torch.randn(D, P, device=dev, generator=g) / D ** 0.5
            b = torch.randn(P, device=dev, generator=g)
            cls = torch.ones(P, dtype=torch.int32, device=dev)
            t = (y[:, None] == cls[None, :]).float()
            ws = K.logreg_workspace(a.n, D, P, device=dev)
            bufs = dict(z=torch.empty(a.n, P, device=dev), r=torch.empty(a.n, P, device=dev),
                        loss=torch.empty(P, dtype=torch.float64, device=dev),
                        gb=torch.empty(P, dtype=torch.float64, device=dev))
            gbuf = torch.empty(D, P, dtype=torch.float64, device=dev)
            fwd = lambda: K.logreg_forward(x, w, b, y, cls, ws=ws, **bufs)      # noqa: E731
            grd = lambda: K.logreg_grad(x, bufs["r"], g=gbuf, ws=ws)            # noqa: E731
            ours = lambda: (fwd(), grd())[1]                                   # noqa: E731
            theirs = lambda: torch_eval(x, w, b, t)                            # noqa: E731
            for _ in range(a.warmup):
                ours(), theirs()
            torch.cuda.synchronize()
            t_o, t_t, t_f, t_g = [], [], [], []
            for _ in range(a.repeats):
                ms, gg = timed(ours)
                t_o.append(ms)
                ms, (_, _, tg) = timed(theirs)
                t_t.append(ms)
                t_f.append(timed(fwd)[0])
                t_g.append(timed(grd)[0])
            mo, mt = statistics.median(t_o), statistics.median(t_t)
            tf = 4.0 * a.n * D * P / (mo * 1e-3) / 1e12
            results.append({"D": D, "P": P, "n": a.n, "ours_ms": round(mo, 3),
                            "ours_ms_minmax": [round(min(t_o), 3), round(max(t_o), 3)],
                            "fwd_ms": round(statistics.median(t_f), 3), "grad_ms": round(statistics.median(t_g), 3),
                            "torch_ms": round(mt, 3), "torch_ms_minmax": [round(min(t_t), 3), round(max(t_t), 3)],
                            "ratio_torch_over_ours": round(mt / mo, 4),
                            "gbps_two_reads_of_x": round(8.0 * a.n * D / (mo * 1e-3) / 1e9, 1),
                            "tflops": round(tf, 2), "frac_of_f32_matrix_peak": round(tf / PEAK_F32_MATRIX_TFLOPS, 4),
                            "max_rel_diff_g": float(((gg - tg.double()).abs().max() / tg.abs().max()).item())})
            del t, bufs, gbuf, ws
        del x
    line = {"bench": "logreg", "peak_tflops": PEAK_F32_MATRIX_TFLOPS, "warmup": a.warmup, "repeats": a.repeats,
            "results": results}
    if a.fit:
        from arcweld.retrieve import logreg_fit
        D, Cs = 5120, [0.1, 1.0, 10.0]
        g = torch.Generator(device=dev).manual_seed(a.seed + 1)
        x = torch.randn(a.fit_n, D, device=dev, generator=g)
        u = torch.rand(a.fit_n, device=dev, generator=g).clamp(1e-6, 1 - 1e-6)
        score = x @ (torch.randn(D, device=dev, generator=g) / D ** 0.5) * 2.0
        y = (score + torch.log(u / (1 - u)) > 0).long()
        del score, u
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fit = logreg_fit(x, y, C=Cs)
        torch.cuda.synchronize()
        line["fit"] = {"n": a.fit_n, "D": D, "C": Cs, "tol": 1e-4, "wall_s": round(time.perf_counter() - t0, 3),
                       "n_iter": [int(v) for v in fit["n_iter"].flatten().cpu()],
                       "converged": [bool(v) for v in fit["converged"].flatten().cpu()]}
    line = json.dumps(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
