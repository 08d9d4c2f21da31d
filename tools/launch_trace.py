"""The kernel-launch sequence of the VQ-VAE paths of a tree, recorded on the CPU: no library is loaded, no device touched.

Every launching wrapper of ``arcweld.kernels`` is replaced by a recorder and the model runs on CPU tensors.  One record
per call: the wrapper's name, its arguments bound to the wrapper's own signature (defaults filled in, so a call that
spells a default out and one that omits it are the same record) and the store policy in force.  A tensor argument --
also inside lists, the problem tuples of ``gemm_grouped`` and a BatchNorm module -- is recorded as (ordinal, shape,
dtype, strides); the ordinal is given at first appearance, keyed by storage pointer and offset, and the recorder keeps
every tensor it has seen alive, so that no storage is reused: two same-shaped tensors swapped between roles change the
trace.  A host-side refactor of the drivers must leave every digest as it was:

    python tools/launch_trace.py --tree <parent checkout> --digests parent.json
    python tools/launch_trace.py --digests new.json          # this tree; --json FILE keeps the full records

``--digests FILE`` writes {case: {path: digest}}; tests/golden/launch_trace.json is that file, and
tests/test_launch_trace_cpu.py compares a few cases (``--cases NAME ...``) against it.
"""
import argparse
import hashlib
import inspect
import json
import os
import sys

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REAL = {"res_chain_ok", "convt_tail_ok", "sep_tail_ok", "chain_head_ok", "head_bf16_ok", "wgrad_issue", "wgrad_batch_ok", "attn_flops"}
PATHS = ("fused_train_step", "autograd", "eval", "encode", "encoder[0]", "decoder[1]", "resblock", "decode",
         "decode_small", "patch_embed", "encoder[1]", "reverse_patch_embed", "reverse_patch_embed_eval")
# the route switches of the boundary layers, one at a time and the first three together (bf16 bn=0, R in (1, 3))
ROUTES_OFF = ("ARCWELD_CONVT_TAIL", "ARCWELD_SEP_TAIL", "ARCWELD_CHAIN_HEAD")
ROUTE_ENVS = [{k: "0"} for k in ROUTES_OFF + ("ARCWELD_HEAD_BF16",)] + [{k: "0" for k in ROUTES_OFF}]
ENV = ("ARCWELD_ENC_CHAIN", "ARCWELD_DEC_CHAIN", "ARCWELD_RESID_F32", "ARCWELD_HEAD_BF16", "ARCWELD_CHAIN_STORE",
       "ARCWELD_WGRAD_BATCH", "ARCWELD_OPERANDS", "ARCWELD_CONVT_TAIL", "ARCWELD_SEP_TAIL",
       "ARCWELD_CHAIN_HEAD")


class Recorder:
    def __init__(self, K, torch):
        self.K, self.torch = K, torch
        self.log, self.ids, self.hold = [], {}, []
        self.gemm_defaults = {n: p.default for n, p in inspect.signature(K._gemm_args).parameters.items()
                              if p.kind is p.KEYWORD_ONLY}
        for name, fn in list(vars(K).items()):
            if inspect.isfunction(fn) and fn.__module__ == K.__name__ and not name.startswith("_") and name not in REAL:
                setattr(K, name, self.stub(name, inspect.signature(fn)))

    def reset(self):
        self.log, self.ids, self.hold = [], {}, []

    def desc(self, v):
        torch = self.torch
        if isinstance(v, torch.Tensor):
            key = (v.untyped_storage().data_ptr(), v.storage_offset())
            if key not in self.ids:
                self.ids[key] = len(self.ids)
                self.hold.append(v)
            return ["T", self.ids[key], list(v.shape), str(v.dtype), list(v.stride())]
        if isinstance(v, torch.nn.Module):
            return [type(v).__name__, {n: self.desc(t) for n, t in list(v.named_parameters()) + list(v.named_buffers())}]
        if isinstance(v, (list, tuple)):
            return [self.desc(x) for x in v]
        if isinstance(v, dict):
            return {k: self.desc(v[k]) for k in sorted(v)}
        if isinstance(v, (int, float, bool, str)) or v is None:
            return v
        return type(v).__name__

    def gemm_kw(self, kw):
        return self.desc({**self.gemm_defaults, **kw})

    def stub(self, name, sig):
        def record(*a, **k):
            b = sig.bind(*a, **k)
            b.apply_defaults()
            args = dict(b.arguments)
            if name == "gemm":
                args["kw"] = self.gemm_kw(args["kw"])
            elif name in ("gemm_grouped", "wgrad_batch"):
                args["problems"] = [[self.desc(list(pb[:5])), self.gemm_kw(pb[5])] for pb in args["problems"]]
            self.log.append([name, self.K._STORE_POLICY.get(),
                             {n: v if n in ("kw", "problems") else self.desc(v) for n, v in sorted(args.items())}])
            if name == "res_dropout_masks_empty":
                return self.torch.empty(8, dtype=self.torch.uint8)
            return k.get("C")
        return record

    def take(self):
        out = self.log
        self.reset()
        return out


def cases():
    for T in ("f32", "bf16"):
        for bn in (False, True):
            variants = [{}]
            if T == "bf16" and not bn:
                variants += [{"ARCWELD_ENC_CHAIN": "0", "ARCWELD_DEC_CHAIN": "0"}, {"ARCWELD_RESID_F32": "1"}]
            for env in variants:
                for R in (0, 1, 3):
                    for p in (0.1, 0.0):
                        yield dict(T=T, bn=bn, R=R, p=p, env=env, batch=False)
            if T == "bf16" and not bn:
                for env in ROUTE_ENVS:
                    for R in (1, 3):
                        for p in (0.1, 0.0):
                            yield dict(T=T, bn=bn, R=R, p=p, env=env, batch=False)
    yield dict(T="bf16", bn=False, R=3, p=0.1, env={}, batch=True)


def case_name(c):
    env = ",".join(f"{k[8:]}={v}" for k, v in sorted(c["env"].items()))
    return f"{c['T']} bn={int(c['bn'])} R={c['R']} p={c['p']}" + (f" {env}" if env else "") + \
        (" wgrad_batch" if c["batch"] else "")


def run_case(c, rec, torch):
    from arcweld import modules, precision
    from arcweld import vqvae as engine
    from model.vq_vae_patch_embedd import ResBlock, VQVAEPatch
    T = torch.bfloat16 if c["T"] == "bf16" else torch.float32
    rec.K.wgrad_batch_ok = lambda problems: c["batch"]
    modules._seed = lambda p: 0x5EED if p > 0 else 0
    for k in ENV:
        os.environ.pop(k, None)
    os.environ.update(c["env"])
    torch.manual_seed(0)
    m = VQVAEPatch(hidden_dim=512, input_dim=2, num_embeddings=512, embedding_dim=64, n_resblocks=c["R"],
                   learning_rate=1e-3, dropout_p=c["p"], batch_norm=c["bn"])
    blk = ResBlock(512, dropout_p=c["p"], batch_norm=c["bn"])
    x = torch.randn(4, 200, 2)
    out = {}
    with precision.operands(T):
        rec.reset()
        m.train()
        m.fused_train_step(x, 1.0)
        out["fused_train_step"] = rec.take()
        emb, x_hat, _ = m(x)
        (emb + x_hat.sum()).backward()
        out["autograd"] = rec.take()
        m.eval()
        with torch.no_grad():
            m(x)
        out["eval"] = rec.take()
        engine.encode(m, x, T)
        out["encode"] = rec.take()
        m.train()
        for name, mod, L in (("encoder[0]", m.encoder[0], 16), ("decoder[1]", m.decoder[1], 16), ("resblock", blk, 7)):
            xx = torch.randn(4, 512, L, requires_grad=True)
            mod(xx).sum().backward()
            out[name] = rec.take()
        # ids -> signals: S = 16, K = 512, so 64 ids take the codebook-table branch and 16 the gather-then-GEMM one
        for name, n in (("decode", 64), ("decode_small", 16)):
            engine.decode(m, torch.arange(n) * 7 % 512, T)
            out[name] = rec.take()
        for name, mod, shape, train in (("patch_embed", m.patch_embed, (4, 200, 2), True),
                                        ("encoder[1]", m.encoder[1], (4, 512, 16), True),
                                        ("reverse_patch_embed", m.reverse_patch_embed, (4, 512, 16), True),
                                        ("reverse_patch_embed_eval", m.reverse_patch_embed, (4, 512, 16), False)):
            m.train(train)
            xx = torch.randn(*shape, requires_grad=True)
            mod(xx).sum().backward()
            out[name] = rec.take()
    for k in c["env"]:
        os.environ.pop(k)
    return out


def digest(v):
    return hashlib.sha1(json.dumps(v).encode()).hexdigest()[:12]


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--tree", default=HERE, help="the checkout to import arcweld / model from (default: this one)")
    ap.add_argument("--json", help="write the full records of every case to this file")
    ap.add_argument("--digests", help="write {case: {path: digest}} of every case to this file")
    ap.add_argument("--cases", nargs="+", metavar="NAME", help="run only the cases of these names (as printed)")
    a = ap.parse_args()
    tree = os.path.abspath(a.tree)
    sys.path[:0] = [tree, os.path.join(tree, "vq-vae-transformer-arc-welding_amd")]
    import torch
    from arcweld import kernels as K
    rec = Recorder(K, torch)
    full = {}
    print(f"{'case':44s} " + " ".join(f"{p[:10]:>10s}" for p in PATHS) + "  digest")
    todo = [c for c in cases() if a.cases is None or case_name(c) in a.cases]
    if a.cases is not None and len(todo) != len(set(a.cases)):
        ap.error(f"unknown case among {a.cases}")
    for c in todo:
        out = run_case(c, rec, torch)
        full[case_name(c)] = out
        print(f"{case_name(c):44s} " + " ".join(f"{len(out[p]):10d}" for p in PATHS) + f"  {digest(out)}")
    print(f"all cases: {digest(full)}")
    if a.json:
        with open(a.json, "w") as f:
            json.dump(full, f, indent=0)
    if a.digests:
        with open(a.digests, "w") as f:
            json.dump({name: {p: digest(v) for p, v in out.items()} for name, out in full.items()}, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
