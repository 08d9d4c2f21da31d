#!/usr/bin/env python
"""Time the two kernels of the RBF-SVM probe (arcweld.kernels.rbf_gram / svm_smo, csrc/svm.hip) against their
restatements in torch, and one whole arcweld.retrieve.svm_fit.

Gram: n = 20000 rows against themselves at D = 2000 and D = 5120 (the probe's raw and latent widths), N(0, 1) features
from a seed, gamma = 1 / D.  Baseline, same process and device, f32:
``exp(-gamma * clamp(|a|^2 + |b|^2 - 2 a b', 0))``.  Also timed: aw_knn's sweep (k = 1) at the same shape, the kernel
whose staging the Gram kernel shares.  "ours" is the call the fit makes, one buffer against itself, which computes the
tiles on or above the diagonal and mirrors them; "two_buffers" is the same rows in two buffers, where every tile is
computed: tflops counts the 2 n^2 D operations of its dot products.
Solver: microseconds per iteration at n = 20000 (512 positive rows, d = 8, gamma = 'scale', C = 0.1 (1 + c)) for
p = 1 and p = 8 problems: ``--smo-iters`` iterations from alpha = 0 in one launch (no problem converges that early).
Baseline: one iteration -- both selections, libsvm's update, the gradient update -- restated in torch ops on the same
state without a host synchronisation, ``--torch-iters`` of them.
Both sides are warmed up, then timed alternately with device events (``--repeats`` times each; the median is reported,
the spread beside it).  ``--fit`` adds the wall time of a whole svm_fit at 20000 x 5120, C = 0.1.  Prints ONE JSON line:

  {"bench": "svm", "peak_tflops": 157.3, "gram": [{"D", "n", "ours_ms", "ours_ms_minmax", "torch_ms",
   "torch_ms_minmax", "ratio_torch_over_ours", "tflops", "frac_of_f32_matrix_peak", "knn_ms", "ratio_knn_over_ours",
   "max_abs_diff", "two_buffers_ms", "ratio_torch_over_two_buffers",
   "ratio_knn_over_two_buffers"}], "smo": [{"p", "n", "iters", "ours_us_per_iter", "ours_us_minmax", "torch_us_per_iter",
   "torch_us_minmax", "ratio_torch_over_ours"}], "fit": {...}}

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
TAU = 1e-12


def torch_gram(a, b, gamma):
    d = (a * a).sum(1)[:, None] + (b * b).sum(1)[None, :] - 2.0 * (a @ b.t())
    return torch.exp(-gamma * d.clamp_(min=0))


def torch_smo_iteration(K, Kd, yf, C, alpha, G):
    """One SMO iteration of include/arcweld_amd.h's rule in torch ops, in place, without a host synchronisation."""
    inf = torch.full((), float("inf"), dtype=torch.float64, device=K.device)
    zero = torch.zeros((), dtype=torch.float64, device=K.device)
    v = -yf * G
    up = ((yf > 0) & (alpha < C)) | ((yf < 0) & (alpha > 0))
    low = ((yf > 0) & (alpha > 0)) | ((yf < 0) & (alpha < C))
    i = torch.where(up, v, -inf).argmax()
    m = v[i]
    Ki = K[i].double()
    b = m - v
    a = Kd[i] + Kd - 2.0 * Ki
    a = torch.where(a <= 0, torch.full_like(a, TAU), a)
    j = torch.where(low & (v < m), -(b * b) / a, inf).argmin()
    Kj = K[j].double()
    yi, yj, ai, aj, quad = yf[i], yf[j], alpha[i], alpha[j], a[j]
    same = yi == yj
    delta = torch.where(same, G[i] - G[j], -G[i] - G[j]) / quad
    diff, s = ai - aj, ai + aj
    # y_i != y_j
    di, dj = ai + delta, aj + delta
    c = (diff > 0) & (dj < 0)
    di, dj = torch.where(c, diff, di), torch.where(c, zero, dj)
    c = (diff <= 0) & (di < 0)
    di, dj = torch.where(c, zero, di), torch.where(c, -diff, dj)
    c = (diff > 0) & (di > C)
    di, dj = torch.where(c, C, di), torch.where(c, C - diff, dj)
    c = (diff <= 0) & (dj > C)
    di, dj = torch.where(c, C + diff, di), torch.where(c, C, dj)
    # y_i == y_j
    si, sj = ai - delta, aj + delta
    c = (s > C) & (si > C)
    si, sj = torch.where(c, C, si), torch.where(c, s - C, sj)
    c = (s <= C) & (sj < 0)
    si, sj = torch.where(c, s, si), torch.where(c, zero, sj)
    c = (s > C) & (sj > C)
    si, sj = torch.where(c, s - C, si), torch.where(c, C, sj)
    c = (s <= C) & (si < 0)
    si, sj = torch.where(c, zero, si), torch.where(c, s, sj)
    ni, nj = torch.where(same, si, di), torch.where(same, sj, dj)
    G += yf * ((yi * (ni - ai)) * Ki + (yj * (nj - aj)) * Kj)
    alpha[i] = ni
    alpha[j] = nj


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    out = fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1), out


def alternate(ours, theirs, warmup, repeats):
    for _ in range(warmup):
        ours(), theirs()
    torch.cuda.synchronize()
    t_o, t_t = [], []
    for _ in range(repeats):
        t_o.append(timed(ours)[0])
        t_t.append(timed(theirs)[0])
    return t_o, t_t


def main():
    p = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    p.add_argument("--n", type=int, default=20000)
    p.add_argument("--dims", type=int, nargs="+", default=[2000, 5120])
    p.add_argument("--ps", type=int, nargs="+", default=[1, 8])
    p.add_argument("--smo-iters", type=int, default=512)
    p.add_argument("--torch-iters", type=int, default=32)
    p.add_argument("--warmup", type=int, default=2)
    p.add_argument("--repeats", type=int, default=7)
    p.add_argument("--seed", type=int, default=0)
    p.add_argument("--fit", action="store_true", help="also time a whole svm_fit at n x 5120, C = 0.1")
    p.add_argument("--out", type=str, default="", help="also write the JSON line to this file")
    a = p.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("svm_bench needs the GPU: a CPU run says nothing about the kernels")
    from arcweld import kernels as K
    from arcweld.retrieve import rbf_gamma
    torch.backends.cuda.matmul.allow_tf32 = False
    torch.set_float32_matmul_precision("highest")
    dev = torch.device("cuda", torch.cuda.current_device())
    n = a.n
    gram = []
    for D in a.dims:
        g = torch.Generator(device=dev).manual_seed(a.seed + D)
        x = torch.randn(n, D, device=dev, generator=g)
        gamma = 1.0 / D
        out = torch.empty(n, n, device=dev)
        ours = lambda: K.rbf_gram(x, x, gamma, k=out)                      # noqa: E731
        theirs = lambda: torch_gram(x, x, gamma)                           # noqa: E731
        diff = float((ours() - theirs()).abs().max())
        t_o, t_t = alternate(ours, theirs, a.warmup, a.repeats)
        knn = lambda: K.knn(x, x, 1)                                       # noqa: E731
        knn()
        t_k = [timed(knn)[0] for _ in range(a.repeats)]
        x2 = x.clone()                                                     # two buffers: every tile is computed
        full = lambda: K.rbf_gram(x, x2, gamma, k=out)                     # noqa: E731
        full()
        t_f = [timed(full)[0] for _ in range(a.repeats)]
        mf = statistics.median(t_f)
        mo, mt, mk = statistics.median(t_o), statistics.median(t_t), statistics.median(t_k)
        tf = 2.0 * n * n * D / (mf * 1e-3) / 1e12                          # of the run that computes every tile
        gram.append({"D": D, "n": n, "ours_ms": round(mo, 3), "ours_ms_minmax": [round(min(t_o), 3), round(max(t_o), 3)],
                     "torch_ms": round(mt, 3), "torch_ms_minmax": [round(min(t_t), 3), round(max(t_t), 3)],
                     "ratio_torch_over_ours": round(mt / mo, 4), "tflops": round(tf, 2),
                     "frac_of_f32_matrix_peak": round(tf / PEAK_F32_MATRIX_TFLOPS, 4), "knn_ms": round(mk, 3),
                     "ratio_knn_over_ours": round(mk / mo, 4), "max_abs_diff": diff,
                     "two_buffers_ms": round(mf, 3),
                     "ratio_torch_over_two_buffers": round(mt / mf, 4),
                     "ratio_knn_over_two_buffers": round(mk / mf, 4)})
        del x, x2, out
    # the solver on a Gram matrix of its own
    g = torch.Generator(device=dev).manual_seed(a.seed + 1)
    x = torch.randn(n, 8, device=dev, generator=g)
    lab = torch.zeros(n, dtype=torch.int64, device=dev)
    lab[torch.randperm(n, device=dev, generator=g)[:512]] = 1
    x[:, 0] += 2.0 * lab
    k = K.rbf_gram(x, x, rbf_gamma(x))
    y1 = (2 * lab - 1).to(torch.int32)
    smo = []
    for P in a.ps:
        y = y1[None].repeat(P, 1).contiguous()
        Cs = [0.1 * (1 + c) for c in range(P)]
        st = [torch.empty((P, n), dtype=torch.float64, device=dev) for _ in range(2)]
        n_iter = torch.zeros(P, dtype=torch.int64, device=dev)
        gap = torch.empty(P, dtype=torch.float64, device=dev)

        def ours():
            st[0].zero_(), st[1].fill_(-1.0), n_iter.zero_()
            K.svm_smo(k, y, Cs, 1e-3, a.smo_iters, alpha=st[0], grad=st[1], n_iter=n_iter, gap=gap)

        yf, Kd = y1.double(), k.diagonal().double().contiguous()
        ta, tg = torch.empty(n, dtype=torch.float64, device=dev), torch.empty(n, dtype=torch.float64, device=dev)

        def theirs():
            ta.zero_(), tg.fill_(-1.0)
            for _ in range(a.torch_iters):
                torch_smo_iteration(k, Kd, yf, Cs[0], ta, tg)

        t_o, t_t = alternate(ours, theirs, a.warmup, a.repeats)
        assert int(n_iter.min()) == a.smo_iters, "a problem converged before --smo-iters iterations"
        uo = [1e3 * t / a.smo_iters for t in t_o]
        ut = [1e3 * t / a.torch_iters for t in t_t]
        smo.append({"p": P, "n": n, "iters": a.smo_iters, "ours_us_per_iter": round(statistics.median(uo), 3),
                    "ours_us_minmax": [round(min(uo), 3), round(max(uo), 3)],
                    "torch_us_per_iter": round(statistics.median(ut), 2),
                    "torch_us_minmax": [round(min(ut), 2), round(max(ut), 2)],
                    "ratio_torch_over_ours": round(statistics.median(ut) / statistics.median(uo), 2)})
    del k, x
    line = {"bench": "svm", "peak_tflops": PEAK_F32_MATRIX_TFLOPS, "warmup": a.warmup, "repeats": a.repeats,
            "gram": gram, "smo": smo}
    if a.fit:
        from arcweld.retrieve import svm_fit
        D = 5120
        g = torch.Generator(device=dev).manual_seed(a.seed + 2)
        x = torch.randn(n, D, device=dev, generator=g)
        lab = (torch.rand(n, device=dev, generator=g) < 0.5).long()
        w = torch.randn(D, device=dev, generator=g)
        x += 3.0 * lab[:, None] * (w / w.norm())[None, :]
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fit = svm_fit(x, lab, C=0.1)
        torch.cuda.synchronize()
        line["fit"] = {"n": n, "D": D, "C": 0.1, "tol": 1e-3, "wall_s": round(time.perf_counter() - t0, 3),
                       "gamma": fit["gamma"], "n_iter": int(fit["n_iter"][0, 0]),
                       "converged": bool(fit["converged"][0, 0]), "n_support": int(fit["n_support"][0, 0])}
    line = json.dumps(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
