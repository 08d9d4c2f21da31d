"""Benchmark: welding windows/sec of the VQ-VAE-Patch reconstruction TRAIN step (BASELINE.json configs[1]:
batch 1024 windows of 200x2 per GPU, codebook 512x64, H=512, 8 ResBlocks, patch 25, dropout 0.1, bf16 MFMA
operands with fp32 accumulation / fp32 master weights).

One step = forward + backward of loss = mse(x_hat, x) + vq_loss, global-norm clip 0.7 and the RAdam update
(train_reconstruction_embedding.py:190-199) over one batch of synthetic standardised windows that is resident
in HBM before the timed region.  Multi-GPU: one process per GPU (torch.distributed.run), RCCL all-reduce of the
flat gradient buffer every step, per-rank batch fixed (weak scaling).

A plain run sets up, warms up, times `--steps` steps and prints ONE JSON line (rank 0) with the headline figure;
`--dump-outputs DIR` also writes what the last timed step computed.  `--full` adds everything else to the line: the
roofline of the dominant kernel (the MFMA GEMM family, timed live with HIP events on its launch stream in eager
steps after the timed region), the VQ kernel alone, the fp32 / stress / Transformer sub-lines, a CPU baseline (the
oracle port on the host cores, bounded sample, rank 0 at N=1 only) and the detail file.
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

REPO = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(REPO, "vq-vae-transformer-arc-welding_amd"))
sys.path.insert(0, REPO)

import torch  # noqa: E402
import torch.distributed as dist  # noqa: E402

METRIC = "welding windows/sec (train) VQ-VAE+8-blk Transformer at 1/2/4/8 MI355X"
BF16_PEAK_TFLOPS = 2500.0     # MI355X dense bf16 MFMA (MI355X_MICROARCH.md: ~2.5 PF dense)
FP32_PEAK_TFLOPS = 157.3      # f32-input MFMA = the fp32 vector rate (MI355X_MICROARCH.md)
HBM_PEAK_GBS = 8000.0


def parse():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--batch", type=int, default=1024, help="windows per GPU")
    ap.add_argument("--full", action="store_true",
                    help="also measure everything beside the headline figure: the per-GEMM roofline pass, the VQ kernel "
                         "alone, the fp32, stress and Transformer sub-lines and the CPU baseline, and write --detail "
                         "(the --no-* switches below trim this set; without --full none of it runs)")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="after the timed steps write what the last one computed (the loss it returned, the updated "
                         "parameters) as DIR/<name>.npy in float32; that step starts from the seeded initial state, "
                         "reset with the clock stopped")
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--cpu-seconds", type=float, default=15.0)
    ap.add_argument("--no-profile", action="store_true", help="skip the live per-GEMM event timing")
    ap.add_argument("--no-graph", action="store_true", help="eager launches instead of the captured step graph")
    ap.add_argument("--no-transformer", action="store_true",
                    help="skip the secondary configs[2]/[3] line items (tokenize + 8-block Transformer train step)")
    ap.add_argument("--no-fp32", action="store_true", help="skip the exact-fp32 operand line of configs[1]")
    ap.add_argument("--no-stress", action="store_true",
                    help="skip the configs[4] line (codebook 8192x256, T 1025, 16-block Transformer)")
    ap.add_argument("--seqs", type=int, default=51, help="Transformer sequences per GPU per step (configs[2])")
    ap.add_argument("--n-cycles", type=int, default=20)
    ap.add_argument("--only", default="all", choices=["all", "transformer_pretokenized", "transformer_b16_acc5"],
                    help="profiling aid: run one sub-line alone (the PMC passes of tools/prof_transformer.sh)")
    ap.add_argument("--detail", default="gpurun_out/bench_detail.json",
                    help="where the full record (every sub-line with its per-kernel objects) is written; the printed "
                         "line keeps the compact form (empty: no file)")
    ap.add_argument("--gemm-tile", type=int, default=0, choices=[0, 128, 256],
                    help="GEMM tile policy (aw_gemm_set_tile): 0 = automatic")
    return ap.parse_args()


def build_model(dev, K=512, D=64):
    from model.vq_vae_patch_embedd import VQVAEPatch
    torch.manual_seed(1)
    m = VQVAEPatch(hidden_dim=512, input_dim=2, num_embeddings=K, embedding_dim=D, n_resblocks=8,
                   learning_rate=1e-3, dropout_p=0.1, patch_size=25, seq_len=200, batch_norm=False)
    return m.to(dev).train()


def _timed_steps(step, warmup, steps, world, before_last=None):
    """warmup untimed steps, then `steps` timed ones between barrier + synchronize; max over ranks (seconds).
    `before_last` (--dump-outputs: the reset of the training state) runs before the last timed step with the clock
    stopped: the steps before it and the last one are timed as two stretches, each between synchronizes."""
    for i in range(warmup):
        step(i)
    torch.cuda.synchronize()
    if world > 1:
        dist.barrier()
    torch.cuda.synchronize()
    el = 0.0
    t0 = time.perf_counter()
    for i in range(steps):
        if before_last is not None and i == steps - 1:
            torch.cuda.synchronize()
            el += time.perf_counter() - t0
            before_last()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
        step(i)
    torch.cuda.synchronize()
    if world > 1:
        dist.barrier()
    torch.cuda.synchronize()
    t = torch.tensor([el + time.perf_counter() - t0], device="cuda", dtype=torch.float64)
    if world > 1:
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
    return float(t.item())


def transformer_flops_per_seq(T, n_blocks=8, d=512, V=514):
    """3 x forward; linear 24 d^2 T per block, causal attention 2 d T (T+1), lm_head 2 d V T."""
    return 3 * (n_blocks * (24 * d * d * T + 2 * d * T * (T + 1)) + 2 * d * V * T)


def transformer_workload(dev, rank, world, args, seqs, n_cycles, accumulate=1, label="configs[2]", K=512, D=64,
                         n_blocks=8, pretokenized=False):
    """Per optimizer step the frozen VQ-VAE encoder tokenizes seqs x n_cycles windows per micro-batch (fused
    encoder + VQ, exact fp32 operands), then the 8-block/8-head d512 decoder trains on the generation task
    (T = 16*n_cycles + 1, V = 514, clip 0.8, RAdam betas (0.9, 0.95) wd 0.1 on Linear weights) over `accumulate`
    micro-batches (train_transformer_mtasks.py:23-33).  bf16 operands (opt-in).  Returns windows/s over all ranks.
    pretokenized: the reference's own regime -- the frozen encoder tokenizes the dataset once at setup
    (dataloader/latentspace_dataloader.py:205-263, create_latent_space_dataset_VQ_VAE_IDs) and the training steps
    read the ids; here the two synthetic batches are tokenized before the timed region (ids resident in HBM) and a
    step is the decoder train step alone."""
    from arcweld import tokenize
    from arcweld.trainer import Trainer
    from model.transformer_decoder import MyTransformerDecoder
    vq = build_model(dev, K, D).eval()
    nc = n_cycles
    T = 16 * nc + 1
    V = K + 2
    torch.manual_seed(2)
    dec = MyTransformerDecoder(d_model=512, n_classes=V, seq_len=T, n_blocks=n_blocks, n_head=8, res_dropout=0.1,
                               pe_len=max(512, T)).to(dev).train()
    tr = Trainer(gradient_clip_val=0.8, accumulate_grad_batches=accumulate)
    tr.setup_optimizer(dec)
    g = torch.Generator(device=dev)
    g.manual_seed(2000 + rank)
    wins = [torch.randn(seqs, 200 * nc, 2, device=dev, generator=g) for _ in range(2)]
    cond = torch.zeros(seqs, dtype=torch.long, device=dev)
    use_graph = not args.no_graph

    assert dec.task == "generate"   # the synthetic condition is unread by the generation loss

    def train(w):
        # w: one micro-batch of windows, or the captured group's micro-batches side by side (arcweld/graphs.py): the
        # condition rows follow the windows (each micro-batch's synthetic condition is zeros)
        ids = tokenize.encode_ids(vq, w)
        x, y, _ = tokenize.autoregressive_pairs(ids, start_token=K)
        c = cond if w.shape[0] == seqs else torch.cat([cond] * (w.shape[0] // seqs))
        return (x, c, y)

    batches = [train(w) for w in wins] if pretokenized else None

    def group(src, i):   # the micro-batches of optimizer step i (one, or an accumulation group)
        g = [src[(i + j) % 2] for j in range(accumulate)]
        return g if accumulate > 1 else g[0]

    def step(i):
        if pretokenized:
            if use_graph:
                tr.graphed_step(dec, group(batches, i), 1.0 / (accumulate * world))
            else:
                for j in range(accumulate):
                    tr.micro_step(dec, batches[(i + j) % 2], j, 1.0 / (accumulate * world))
                tr.optimizer_step(dec)
        elif use_graph:
            # tokenization is captured with the step: the static window buffer feeds the encoder inside g1, once
            # per micro-batch of the group
            tr.graphed_step(dec, group(wins, i), 1.0 / (accumulate * world))
        else:
            for j in range(accumulate):
                tr.micro_step(dec, train(wins[(i + j) % 2]), j, 1.0 / (accumulate * world))
            tr.optimizer_step(dec)

    if use_graph and not pretokenized:
        # the captured step tokenizes its static window buffer itself (warm-up calls: training_step; captured
        # replays: the fused step with the mid-backward all-reduce split)
        orig, orig_fused = dec.training_step, dec.fused_train_step
        dec.training_step = lambda w, i: orig(train(w), i)
        dec.fused_train_step = lambda w, scale, mid_hook=None, **kw: orig_fused(train(w), scale, mid_hook=mid_hook, **kw)
    el = _timed_steps(step, max(args.warmup, 3 if use_graph else 0), args.steps, world)
    windows = world * seqs * accumulate * nc * args.steps
    flops = transformer_flops_per_seq(T, n_blocks, 512, V) * seqs * accumulate * world * args.steps
    roof, attn = None, None
    if not args.no_profile:
        # per-launch HIP events cannot sit inside the captured graph: a profiled eager pass of the same step follows
        from arcweld import kernels
        n_prof = min(args.steps, 5)
        kernels.PROFILE = []
        t1 = time.perf_counter()
        for i in range(n_prof):
            for j in range(accumulate):
                k = (i + j) % 2      # graphed runs patched training_step to tokenize its window batch itself
                b = batches[k] if pretokenized else (wins[k] if use_graph else train(wins[k]))
                tr.micro_step(dec, b, j, 1.0 / (accumulate * world))
            tr.optimizer_step(dec)
        torch.cuda.synchronize()
        pel = (time.perf_counter() - t1) / n_prof
        prof = (kernels.PROFILE, n_prof)
        kernels.PROFILE = None
        pmc, tsrc = pmc_traffic("pmc_traffic_transformer.json")
        roof = gemm_roofline(prof, pel, el, args.steps, BF16_PEAK_TFLOPS, "bf16",
                             pmc if pretokenized else None, tsrc if pretokenized else None)
        if not pretokenized and any(e[3] == "gemm_f32" for e in prof[0]):
            r32 = gemm_roofline(prof, pel, el, args.steps, FP32_PEAK_TFLOPS, "f32")
            roof["tokenize_gemm_f32"] = {"peak": FP32_PEAK_TFLOPS, **r32["family"]}
        attn = attn_roofline(prof)
    return {"value": round(windows / el, 2), "unit": "windows/s", "ms_per_step": round(el * 1e3 / args.steps, 3),
            "steps": args.steps, "roofline": roof, "attention": attn,
            "config": {"workload": (f"Transformer train step on ids tokenized once at setup ({label})" if pretokenized
                                    else f"tokenize (frozen VQ-VAE encoder, fp32 exact) + Transformer train step ({label})"),
                       "seqs_per_gpu_per_micro_batch": seqs, "accumulate_grad_batches": accumulate,
                       "n_cycles": nc, "T": T, "d_model": 512, "n_blocks": n_blocks, "n_head": 8, "V": V,
                       "codebook": f"{K}x{D}",
                       "global_batch_windows": windows // args.steps, "operands": "bf16"},
            "transformer_tflops": round(flops / el / 1e12, 2),
            "launch": "hip-graph" if use_graph else "eager"}


def _newest_profile(name):
    """The newest committed profiles/r<round>/<session>*/<name>, by round then session number (s14 after s9)."""
    import glob
    import re

    def key(path):
        parts = os.path.relpath(path, REPO).split(os.sep)
        nums = [int(m.group(1)) if (m := re.match(r"[rs](\d+)", q)) else -1 for q in parts[1:3]]
        return nums, path
    files = sorted(glob.glob(os.path.join(REPO, "profiles", "r0*", "*", name)), key=key)
    return files[-1] if files else None


def pmc_traffic(name):
    """The newest committed pmc_traffic.py record `name` (profiles/r<round>/<session>/): HBM bytes per launch of
    every traced kernel of this same workload, FETCH_SIZE (doubled on gfx950) and WRITE_SIZE from separate rocprofv3
    passes (tools/prof_round.sh, tools/prof_transformer.sh): counters cannot be read from inside the timed run."""
    newest = _newest_profile(name)
    if newest is None:
        return None, None
    with open(newest) as f:
        return json.load(f), os.path.relpath(newest, REPO)


REFERENCE_CPU = {"value": 85.0, "unit": "windows/s", "cores": 8, "kind": "reference",
                 "sample": "the reference's own model modules (model/vq_vae_patch_embedd.py, autencoder_lightning_base.py) "
                           "imported through the oracle shim, B=1024 fp32 train step (fwd+bwd+clip 0.7+RAdam), "
                           "torch CPU, 8-vCPU Intel Xeon (AVX-512/AMX); measured in the build container "
                           "(BASELINE.md): the reference's Python does not travel to the GPU box"}


def _cpu_model():
    try:
        with open("/proc/cpuinfo") as f:
            for line in f:
                if line.startswith("model name"):
                    return line.split(":", 1)[1].strip()
    except OSError:
        pass
    return "unknown"


def _cgroup_cpus():
    """CPUs granted by the cgroup CPU quota (cgroup v2 cpu.max / v1 cfs quota), None when unlimited or unknown."""
    try:
        with open("/sys/fs/cgroup/cpu.max") as f:
            q, per = f.read().split()[:2]
        return None if q == "max" else max(1, int(int(q) / int(per)))
    except (OSError, ValueError):
        pass
    try:
        with open("/sys/fs/cgroup/cpu/cpu.cfs_quota_us") as f:
            q = int(f.read())
        with open("/sys/fs/cgroup/cpu/cpu.cfs_period_us") as f:
            per = int(f.read())
        return None if q <= 0 else max(1, q // per)
    except (OSError, ValueError):
        return None


def cpu_baseline(seconds):
    """Oracle port (oracle/vqvae.py, torch CPU fp32) on a bounded sample of the same workload: full-size model,
    B=32 windows per step, fwd+bwd+clip+RAdam; windows/s.  Threads: the CPUs this process may use -- on the GPU box
    that is its CPU share (OMP_NUM_THREADS, 16 per GPU; nproc there reports the whole host)."""
    from oracle import gen
    from oracle import optim as oo
    from oracle import vqvae as ov
    nproc = os.cpu_count() or 1
    try:
        avail = len(os.sched_getaffinity(0))
    except AttributeError:
        avail = nproc
    quota = _cgroup_cpus()
    share = int(os.environ.get("OMP_NUM_THREADS", "0") or 0)
    # all the CPUs this process may actually run on: the affinity set, capped by the cgroup CPU quota (the GPU box
    # grants each GPU's job a share of a larger host; its affinity mask lists every host CPU) and OMP_NUM_THREADS
    threads = max(1, min(x for x in (avail, quota or avail, share or avail)))
    torch.set_num_threads(threads)
    cfg = ov.VQVAEConfig(dropout_p=0.0)
    sd = ov.det_state_dict(cfg, 1)
    names = [k for k in sd if not (k.endswith("running_mean") or k.endswith("running_var") or
                                   k.endswith("num_batches_tracked"))]
    st = oo.RAdamState([sd[k].shape for k in names])
    B = 32
    x = gen.windows(0, B)
    steps, t0 = 0, None
    while True:
        out, grads, state = ov.vqvae_train_step_grads(sd, x, cfg)
        gl = [grads[k].copy() for k in names]
        oo.clip_grad_norm(gl, 0.7)
        ps = [sd[k] for k in names]
        oo.radam_step(ps, gl, st, 1e-3, (0.9, 0.999), 1e-8, [0.0] * len(ps))
        if t0 is None:            # first step is warm-up
            t0 = time.time()
            continue
        steps += 1
        if time.time() - t0 > seconds:
            break
    el = time.time() - t0
    return {"value": round(B * steps / el, 2), "unit": "windows/s", "cores": threads, "kind": "port",
            "nproc": nproc, "affinity_cpus": avail, "cgroup_cpu_quota": quota, "omp_num_threads": share or None,
            "cpu_model": _cpu_model(),
            "sample": f"oracle/vqvae.py full-size VQ-VAE (H512 R8 K512xD64) fp32 train step, B={B} windows, "
                      f"{steps} timed steps ({el:.1f} s) after 1 warm-up, torch CPU {threads} threads "
                      f"(= min of the affinity set, the cgroup quota and OMP_NUM_THREADS on a {nproc}-CPU host)",
            "reference": REFERENCE_CPU}


DUMP_MAX_BYTES = 32 << 20     # all of --dump-outputs (the float32 payload) stays under this


def dump_outputs(out_dir, model, loss):
    """What a caller of the timed step holds after its last call, as out_dir/<name>.npy (float32): `loss`, the
    tensor the step returned, and `params`, every parameter as the update left it, flattened and joined in
    named_parameters() order.  An array over its share
    of DUMP_MAX_BYTES is written as a fixed sample of its elements (flat indices drawn once from a seeded generator,
    sorted: the same ones in every run and every build)."""
    import numpy as np
    arrays = {"loss": loss.detach().reshape(1),
              "params": torch.cat([p.detach().to(torch.float32).reshape(-1) for p in model.parameters()])}
    cap = DUMP_MAX_BYTES // 4 // len(arrays)
    os.makedirs(out_dir, exist_ok=True)
    for name, t in arrays.items():
        if t.numel() > cap:
            keep = np.sort(np.random.default_rng(0).choice(t.numel(), cap, replace=False))
            t = t[torch.from_numpy(keep).to(t.device)]
        np.save(os.path.join(out_dir, name + ".npy"), t.to(torch.float32).cpu().numpy())


def reset_training_state(model, opt, params0):
    """Put the model and its optimizer back where setup left them: the initial parameters (`params0`, a copy of the
    optimizer's flat buffer), zero RAdam moments and step count, the dropout counter at zero, and the GEMM operand
    copies relaid from those parameters into their own buffers (a captured step graph keeps reading them).  The
    gradients are zero already (the update zeroes them)."""
    F = opt._flat
    F["p"].copy_(params0)
    F["m"].zero_()
    F["v"].zero_()
    F["step"].zero_()
    opt._step_count = 0
    if getattr(model, "_rng_counter", None) is not None:
        model._rng_counter.zero_()
    for st in model.__dict__.get("_operand_sets", {}).values():
        st.refresh(force=True)


def vqvae_workload(dev, rank, world, args, dtype, steps, warmup, profile=True, K=512, D=64, dump=None):
    """configs[1]: one step = fwd + bwd (mse + VQ loss) + clip 0.7 + RAdam over B windows per GPU, inputs resident
    in HBM, captured as HIP graphs; operands `dtype` (bf16 opt-in or exact fp32).  `dump`: the directory
    dump_outputs writes to right after the timed steps (None: no dump, False: a rank that only takes part).  The last
    timed step then starts from the state setup left (reset_training_state), not from where the steps before it got
    to: the f32 atomic adds of the backward land in another order every run, with bf16 operands such a last-bit
    difference flips bf16 roundings, and after a few steps two runs of one build are 1e-4 apart; one step from the
    seeded state is the same in every run down to those last bits.  Returns (elapsed seconds, per-GEMM profile list
    or None, eager seconds/step of the profiled pass)."""
    from arcweld import kernels
    from arcweld.precision import operands
    from arcweld.trainer import Trainer
    with operands(dtype):
        model = build_model(dev, K, D)
        trainer = Trainer(gradient_clip_val=0.7)
        opt = trainer.setup_optimizer(model)
        params0 = opt.flatten()[0].clone() if dump is not None else None
        scale = 1.0 / world
        gen_ = torch.Generator(device=dev)
        gen_.manual_seed(1000 + rank)
        batches = [torch.randn(args.batch, 200, 2, device=dev, generator=gen_) for _ in range(4)]
        use_graph = not args.no_graph

        last = {}

        def eager_step(i):
            last["loss"] = trainer.micro_step(model, batches[i % len(batches)], i, scale)
            trainer.optimizer_step(model)

        def step(i):
            if use_graph:
                last["loss"] = trainer.graphed_step(model, batches[i % len(batches)], scale)
            else:
                eager_step(i)

        # graphed_step runs 2 eager warm-up calls and captures on the 3rd: >= 3 untimed calls keep the capture out
        elapsed = _timed_steps(step, max(warmup, 3 if use_graph else 0), steps, world,
                               (lambda: reset_training_state(model, opt, params0)) if dump is not None else None)
        if dump:
            dump_outputs(dump, model, last["loss"])
        # per-GEMM HIP events cannot sit inside a captured graph: the kernel durations for the roofline come from a
        # profiled eager pass over the same workload right after the timed region (GPU-side durations are the
        # same; rocprofv3 in profiles/ cross-checks them against the graph replays)
        prof, prof_el = None, None
        if profile:
            n_prof = min(steps, 10)
            kernels.PROFILE = []
            t1 = time.perf_counter()
            for i in range(n_prof):
                eager_step(i)
            torch.cuda.synchronize()
            prof_el = (time.perf_counter() - t1) / n_prof
            prof = (kernels.PROFILE, n_prof)
            kernels.PROFILE = None
    return elapsed, prof, prof_el


def _ev_ms(e):
    return e[0].elapsed_time(e[1])


def _pmc_bytes(pmc, name, exclude=None):
    """HBM bytes per launch of the kernel `name` (the profile name: "res_chain_bwd_kernel<3>", "wgrad_conv3_kernel",
    ...) from a pmc_traffic.py record: every traced kernel whose rocprofv3 name holds the stem (template arguments
    after the first dropped), the f32 instantiations left out of a bf16 family."""
    if not pmc:
        return None
    stem = name.split(" ")[0]
    stem = stem[:-1] if stem.endswith(">") else stem
    tot, n = 0.0, 0
    for k, v in pmc.get("kernels", {}).items():
        if stem in k and not (exclude and exclude in k):
            tot += v["bytes_per_launch"] * v["launches"]
            n += v["launches"]
    return round(tot / n) if n else None


def kernel_table(prof, tag, peak, pmc=None, exclude=None):
    """Per kernel of one family (the profile's kernel names): launches per step, average launch duration (HIP events
    on the launch stream), algorithmic GFLOP per launch, achieved TFLOP/s and fraction of `peak`, algorithmic HBM
    bytes per launch where the call states them, and the PMC-counted bytes per launch with their ratio to it."""
    lst, n_prof = prof
    by = {}
    for e in lst:
        if e[3] == tag:
            by.setdefault(e[4], []).append(e)
    out = {}
    for name, ev in by.items():
        ms = sum(_ev_ms(e) for e in ev)
        fl = sum(e[2] for e in ev)
        tf = fl / (ms * 1e-3) / 1e12
        row = {"launches_per_step": len(ev) // n_prof, "avg_launch_us": round(ms * 1e3 / len(ev), 2),
               "ms_per_step": round(ms / n_prof, 3), "gflop_per_launch": round(fl / len(ev) / 1e9, 4),
               "achieved": round(tf, 2), "frac": round(tf / peak, 4)}
        if all(e[5] is not None for e in ev):
            row["algorithmic_bytes_per_launch"] = round(sum(e[5] for e in ev) / len(ev))
        t = _pmc_bytes(pmc, name, exclude)
        if t is not None:
            row["traffic_bytes_per_launch"] = t
            if row.get("algorithmic_bytes_per_launch"):
                row["traffic_over_algorithmic"] = round(t / row["algorithmic_bytes_per_launch"], 3)
        out[name] = row
    return dict(sorted(out.items(), key=lambda kv: -kv[1]["ms_per_step"]))


def gemm_roofline(prof, prof_el, elapsed, steps, peak, dtype_name, pmc=None, traffic_src=None):
    """The roofline of the DOMINANT kernel of the MFMA family of one operand dtype (the kernel with the most time
    per step over the profiled eager steps, HIP events per launch on its launch stream): its algorithmic FLOPs per
    launch / its average launch duration, and its PMC-counted HBM bytes per launch (`pmc`: the pmc_traffic.py
    record of the same workload, committed under profiles/).  `kernels` holds the same figures for every kernel of
    the family, `family` the aggregate over all of them."""
    lst, n_prof = prof
    tag = f"gemm_{dtype_name}"
    fam = [e for e in lst if e[3] == tag]
    ms = sum(_ev_ms(e) for e in fam)
    flops = sum(e[2] for e in fam)
    n = len(fam)
    fam_tf = flops / (ms * 1e-3) / 1e12
    excl = "<float" if dtype_name == "bf16" else None
    table = kernel_table(prof, tag, peak, pmc, excl)
    dom_name, dom = next(iter(table.items()))
    return {"bound": "mfma", "achieved": dom["achieved"], "peak": peak, "unit": "TFLOP/s", "frac": dom["frac"],
            "traffic": dom.get("traffic_bytes_per_launch"), "traffic_unit": "bytes/launch",
            "traffic_source": traffic_src, "kernel": dom_name,
            "avg_launch_us": dom["avg_launch_us"], "algorithmic_gflop_per_launch": dom["gflop_per_launch"],
            "algorithmic_bytes_per_launch": dom.get("algorithmic_bytes_per_launch"),
            "traffic_over_algorithmic": dom.get("traffic_over_algorithmic"),
            "family": {"achieved": round(fam_tf, 2), "frac": round(fam_tf / peak, 4), "launches_per_step": n // n_prof,
                       "ms_per_step": round(ms / n_prof, 3),
                       "share_of_step": round(ms / n_prof / (elapsed * 1e3 / steps), 4),
                       "kernels": f"every {tag} MFMA launch: " + ", ".join(table)},
            "kernels": table,
            "measured_over": f"{n_prof} eager steps after the timed region (HIP events per launch, on the launch "
                             "stream)",
            "eager_ms_per_step_with_events": round(prof_el * 1e3, 3)}


def vq_in_step(prof):
    """The VQ forward as the training step runs it (profiled eager steps: its codebook cold behind the encoder)."""
    lst, n_prof = prof
    ev = [e for e in lst if e[3] == "vq_fwd"]
    if not ev:
        return None
    us = sum(_ev_ms(e) for e in ev) * 1e3 / len(ev)
    tf = sum(e[2] for e in ev) / len(ev) / (us * 1e-6) / 1e12
    return {"kernel": ev[0][4], "avg_launch_us": round(us, 2), "frac": round(tf / FP32_PEAK_TFLOPS, 4),
            "launches_per_step": len(ev) // n_prof}


def attn_roofline(prof):
    """The flash-attention kernels of the profiled steps (HIP events per launch; algorithmic FLOPs: the causal QK^T
    and PV of the forward, twice that for the backward) against the bf16 dense MFMA peak."""
    lst, n_prof = prof
    out = {}
    for tag in ("attn_fwd", "attn_bwd"):
        ev = [e for e in lst if e[3] == tag]
        if not ev:
            continue
        us = sum(_ev_ms(e) for e in ev) * 1e3 / len(ev)
        tf = sum(e[2] for e in ev) / len(ev) / (us * 1e-6) / 1e12
        out[tag] = {"avg_launch_us": round(us, 2), "achieved": round(tf, 2), "peak": BF16_PEAK_TFLOPS,
                    "unit": "TFLOP/s", "frac": round(tf / BF16_PEAK_TFLOPS, 4),
                    "gflop_per_launch": round(sum(e[2] for e in ev) / len(ev) / 1e9, 4),
                    "launches_per_step": len(ev) // n_prof}
    return out


def vq_kernel_roofline(dev, N, K, D, iters=10):
    """aw_vq_forward_ex2 alone at (N, K, D), called as the training step calls it (the bf16 operand copy of z_q and
    the grouped code counts, arcweld/vqvae.py): HIP events around each launch on its stream; 2*N*K*D FP32 FLOPs
    against the 157.3 TF fp32 peak (the f32-input MFMA's = the vector peak: the pinned kernel runs the dot products
    on the MFMA, the streaming one on the VALU), plus its algorithmic HBM bytes (z + E + idx + z_q + counts)."""
    from arcweld import kernels
    from arcweld.vqvae import VQ_COUNT_GROUPS
    g = torch.Generator(device=dev).manual_seed(5)
    z = torch.randn(N, D, device=dev, generator=g) * 0.08
    E = torch.randn(K, D, device=dev, generator=g) * 0.08
    zq, idx = torch.empty_like(z), torch.empty(N, dtype=torch.int64, device=dev)
    zq2 = torch.empty(N, D, device=dev, dtype=torch.bfloat16)
    counts, sq = torch.zeros(VQ_COUNT_GROUPS * K, device=dev), torch.zeros(1, device=dev, dtype=torch.float64)
    s = torch.cuda.current_stream()

    def launch():
        kernels.vq_forward(z, E, zq, idx, counts, sq, zq_copy=zq2, count_groups=VQ_COUNT_GROUPS)
    launch()
    # the average launch duration over back-to-back launches (HIP events around the run, on the launches' stream):
    # the per-kernel average rocprofv3's kernel trace reports for the same run; an event pair around every launch
    # adds ~2.5 us of event and dispatch latency to each (21.5 vs 19.0 us measured for this kernel)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(s)
    for _ in range(iters):
        launch()
    e1.record(s)
    torch.cuda.synchronize()
    us = e0.elapsed_time(e1) * 1e3 / iters
    tf = 2.0 * N * K * D / (us * 1e-6) / 1e12
    byts = N * D * 4 * 2 + N * D * 2 + K * D * 4 + N * 8 + K * 4
    pinned = K <= 512 and D in (16, 32, 64)
    return {"kernel": "vq_fwd_pinned_kernel<D> (f32 MFMA)" if pinned else "vq_fwd_kernel<D> (f32 VALU)",
            "bound": "fp32-mfma" if pinned else "fp32-valu", "N": N, "K": K, "D": D,
            "avg_launch_us": round(us, 2), "achieved": round(tf, 2), "peak": FP32_PEAK_TFLOPS, "unit": "TFLOP/s",
            "frac": round(tf / FP32_PEAK_TFLOPS, 4), "algorithmic_bytes": byts,
            "hbm_gbs": round(byts / (us * 1e-6) / 1e9, 1)}


def stress_workload(dev, rank, world, args):
    """configs[4]: the VQ-VAE with the 8192 x 256 codebook (B = 1024 windows per GPU, bf16 operands, graphed step)
    and the 16-block Transformer at T = 1025 (n_cycles 64, V 8194; 16 sequences = 1024 windows per GPU, tokenized
    by that VQ-VAE), each reported as windows/s with its roofline."""
    from arcweld.precision import operands
    n = max(20, args.steps)                 # steady state: >= 20 timed replays after the capture (warm-up >= 3)
    el, prof, pel = vqvae_workload(dev, rank, world, args, torch.bfloat16, n, max(5, args.warmup),
                                   profile=not args.no_profile, K=8192, D=256)
    out = {"vqvae": {"value": round(world * args.batch * n / el, 2), "unit": "windows/s",
                     "ms_per_step": round(el * 1e3 / n, 3), "steps": n,
                     "config": {"workload": "VQ-VAE-Patch train step, stress codebook (configs[4])",
                                "per_gpu_batch": args.batch, "codebook": "8192x256", "operands": "bf16"},
                     "roofline": gemm_roofline(prof, pel, el, n, BF16_PEAK_TFLOPS, "bf16") if prof else None,
                     "vq_kernel": vq_kernel_roofline(dev, args.batch * 16, 8192, 256)}}
    sargs = argparse.Namespace(**vars(args))
    sargs.steps = n
    sargs.warmup = max(5, args.warmup)
    with operands(torch.bfloat16):
        out["transformer"] = transformer_workload(dev, rank, world, sargs, 16, 64, K=8192, D=256, n_blocks=16,
                                                  label="configs[4] stress: 16 blocks, T 1025, codebook 8192x256")
    return out


def _transformer_lines(extra, dev, rank, world, args):
    """configs[2] at 51 sequences per step (1020 windows), configs[2] at the reference's own batch (16 sequences x
    accumulate_grad_batches 5, train_transformer_mtasks.py:32) and the configs[3](ii) shape (n_cycles 16, T = 257,
    64 sequences = 1024 windows per rank)."""
    extra["transformer"] = transformer_workload(dev, rank, world, args, args.seqs, args.n_cycles)
    extra["transformer_b16_acc5"] = transformer_workload(dev, rank, world, args, 16, args.n_cycles, accumulate=5,
                                                         label="configs[2], reference batch 16 x accumulate 5")
    extra["transformer_t257"] = transformer_workload(dev, rank, world, args, 64, 16,
                                                     label="configs[3](ii) shape, 64 seq x 16 cycles per rank")
    extra["transformer_pretokenized"] = transformer_workload(dev, rank, world, args, args.seqs, args.n_cycles,
                                                             pretokenized=True,
                                                             label="configs[2], the reference's regime")


_ROOF_KEYS = ("bound", "achieved", "peak", "unit", "frac", "traffic", "traffic_unit", "traffic_source", "kernel",
              "avg_launch_us", "algorithmic_gflop_per_launch", "algorithmic_bytes_per_launch",
              "traffic_over_algorithmic")


def _compact_roof(r, keys=_ROOF_KEYS):
    """The dominant kernel's roofline, the family aggregate, and per kernel of the family its launch time, fraction
    of the peak and counted / algorithmic HBM bytes."""
    if r is None:
        return None
    out = {k: r[k] for k in keys if k in r}
    out["family"] = {k: r["family"][k] for k in ("achieved", "frac", "launches_per_step", "ms_per_step")}
    out["per_kernel"] = {n: {k: v[k] for k in ("avg_launch_us", "launches_per_step", "frac", "traffic_over_algorithmic")
                             if k in v} for n, v in r["kernels"].items()}
    return out


def _sub(d):
    """One secondary line as {value, unit, ms_per_step, frac[, attention fracs]}."""
    out = {"value": d["value"], "unit": d["unit"], "ms_per_step": d["ms_per_step"]}
    r = d.get("roofline")
    if r:
        out["gemm_frac"] = r["family"]["frac"]
        if "tokenize_gemm_f32" in r:
            out["tokenize_gemm_f32_frac"] = r["tokenize_gemm_f32"]["frac"]
    for tag, a in (d.get("attention") or {}).items():
        out[f"{tag}_us"] = a["avg_launch_us"]
        out[f"{tag}_frac"] = a["frac"]
    return out


def compact_line(line, detail):
    """The printed JSON line: the contract keys, the headline roofline and CPU baseline, and one short summary per
    secondary line LAST (the driver keeps the tail of stdout); the full record goes to `detail`."""
    out = {k: v for k, v in line.items() if k not in ("vq_kernel", "fp32", "stress", "transformer",
                                                      "transformer_b16_acc5", "transformer_t257",
                                                      "transformer_pretokenized", "roofline", "cpu_baseline")}
    out["roofline"] = _compact_roof(line.get("roofline"))
    cpu = line.get("cpu_baseline")
    if cpu:
        out["cpu_baseline"] = {k: cpu[k] for k in ("value", "unit", "cores", "kind", "sample", "cpu_model")}
        out["cpu_baseline"]["reference"] = {k: REFERENCE_CPU[k] for k in ("value", "unit", "cores", "kind")}
    out["detail_file"] = detail or None
    lines = {}
    if "vq_kernel" in line:
        v = line["vq_kernel"]
        lines["vq_kernel"] = {"us": v["avg_launch_us"], "frac": v["frac"], "bound": v["bound"]}
        if v.get("in_step"):
            lines["vq_kernel"]["in_step_us"] = v["in_step"]["avg_launch_us"]
            lines["vq_kernel"]["in_step_frac"] = v["in_step"]["frac"]
    if "fp32" in line:
        f = line["fp32"]
        lines["fp32"] = {"value": f["value"], "unit": f["unit"], "ms_per_step": f["ms_per_step"],
                         "gemm_frac_of_fp32_peak": f["roofline"]["family"]["frac"] if f.get("roofline") else None}
    st = line.get("stress")
    if st:
        lines["stress_vqvae"] = {"value": st["vqvae"]["value"], "unit": "windows/s",
                                 "ms_per_step": st["vqvae"]["ms_per_step"],
                                 "gemm_frac": st["vqvae"]["roofline"]["family"]["frac"] if st["vqvae"].get("roofline")
                                 else None,
                                 "vq_kernel_frac": st["vqvae"]["vq_kernel"]["frac"]}
        lines["stress_transformer"] = _sub(st["transformer"])
    for k in ("transformer", "transformer_b16_acc5", "transformer_t257", "transformer_pretokenized"):
        if k in line:
            lines[k] = _sub(line[k])
    out["lines"] = lines
    return out


def main():
    args = parse()
    distributed = int(os.environ.get("WORLD_SIZE", "1")) > 1
    if distributed:
        # ARCWELD_DIST_BACKEND=gloo rehearses N ranks on one GPU (RCCL refuses two ranks per device); the
        # measured multi-GPU path is "nccl" (= RCCL over xGMI)
        dist.init_process_group(os.environ.get("ARCWELD_DIST_BACKEND", "nccl"))
        rank, world = dist.get_rank(), dist.get_world_size()
        local = int(os.environ.get("LOCAL_RANK", "0")) % max(1, torch.cuda.device_count())
    else:
        rank, world, local = 0, 1, 0
    torch.cuda.set_device(local)
    dev = torch.device("cuda", local)

    from arcweld import _native
    _native.call("aw_gemm_set_tile", args.gemm_tile)

    if args.only != "all":
        from arcweld.precision import operands
        with operands(torch.bfloat16):
            if args.only == "transformer_pretokenized":
                line = transformer_workload(dev, rank, world, args, args.seqs, args.n_cycles, pretokenized=True,
                                            label="configs[2], the reference's regime")
            else:
                line = transformer_workload(dev, rank, world, args, 16, args.n_cycles, accumulate=5,
                                            label="configs[2], reference batch 16 x accumulate 5")
        if rank == 0:
            print(json.dumps({"only": args.only, **line}), flush=True)
        if distributed:
            dist.destroy_process_group()
        return

    # headline: configs[1] in bf16 (BASELINE.json names bf16 for it; an explicit opt-in, arcweld.precision)
    full = args.full
    elapsed, prof, prof_el = vqvae_workload(dev, rank, world, args, torch.bfloat16, args.steps, args.warmup,
                                            profile=full and not args.no_profile,
                                            dump=args.dump_outputs and (args.dump_outputs if rank == 0 else False))
    value = world * args.batch * args.steps / elapsed
    roofline = None
    if prof:
        pmc, traffic_src = pmc_traffic("pmc_traffic_vqvae.json")
        roofline = gemm_roofline(prof, prof_el, elapsed, args.steps, BF16_PEAK_TFLOPS, "bf16", pmc, traffic_src)

    extra = {}
    if full:
        extra["vq_kernel"] = vq_kernel_roofline(dev, args.batch * 16, 512, 64)
    if prof:
        extra["vq_kernel"]["in_step"] = vq_in_step(prof)
    if full and not args.no_fp32:
        # the same step with exact-fp32 operands (the default numerics, the reference's): priced against the
        # 157.3 TF fp32 MFMA roof
        n32 = max(20, args.steps)           # steady state: >= 20 timed replays after the capture (warm-up >= 3)
        el32, prof32, pel32 = vqvae_workload(dev, rank, world, args, torch.float32, n32, max(5, args.warmup),
                                             profile=not args.no_profile)
        extra["fp32"] = {"value": round(world * args.batch * n32 / el32, 2), "unit": "windows/s",
                         "ms_per_step": round(el32 * 1e3 / n32, 3), "steps": n32, "dtype": "f32",
                         "roofline": gemm_roofline(prof32, pel32, el32, n32, FP32_PEAK_TFLOPS, "f32") if prof32 else None}
    if full and not args.no_stress:
        extra["stress"] = stress_workload(dev, rank, world, args)
    if full and not args.no_transformer:
        from arcweld.precision import operands
        with operands(torch.bfloat16):
            _transformer_lines(extra, dev, rank, world, args)

    if rank == 0:
        cpu = None
        if full and world == 1 and not args.no_cpu_baseline:
            cpu = cpu_baseline(args.cpu_seconds)
        line = {"metric": METRIC, "value": round(value, 2), "unit": "windows/s", "n_gpus": world,
                "steps": args.steps, "warmup": args.warmup, "ms_per_step": round(elapsed * 1e3 / args.steps, 3),
                "higher_is_better": True, "scaling": "weak",
                # BASELINE.md has no published number; the basis is the reference's own CPU path measured on this
                # exact workload (configs[1] shape, B=1024) in BASELINE.md -- the target there is >= 10x it
                "vs_baseline": round(value / REFERENCE_CPU["value"], 1),
                "vs_baseline_basis": "reference CPU path, 85.0 windows/s at B=1024 (BASELINE.md, measured)",
                "dtype": "bf16",
                "data": "synthetic N(0,1) standardised 200x2 welding windows, random-init weights",
                "config": {"workload": "VQ-VAE-Patch reconstruction train step (configs[1])",
                           "global_batch": world * args.batch, "per_gpu_batch": args.batch, "seq_len": 200,
                           "codebook": "512x64", "hidden": 512, "n_resblocks": 8, "patch": 25,
                           "parallelism": f"dp{world}", "clip": 0.7, "optimizer": "RAdam(lr 1e-3)",
                           "operands": "bf16 (opt-in), fp32 accumulation and master weights"},
                "roofline": roofline, "cpu_baseline": cpu, **extra,
                "launch": "eager" if args.no_graph else "hip-graph"}
        detail = args.detail if full else None
        if detail:
            path = os.path.join(REPO, detail)
            os.makedirs(os.path.dirname(path), exist_ok=True)
            with open(path, "w") as f:
                json.dump(line, f, indent=1)
        print(json.dumps(compact_line(line, detail)), flush=True)
    if distributed:
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
