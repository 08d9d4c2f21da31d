"""GRU classifier stack at the reference default (B = 512, T = 5, in_dim = 400, H = 758, 6 layers): time per call of
the forward, of forward + backward, and per launch of the two recurrent step kernels (aw_gru_step_fwd / _bwd), in both
operand modes; torch's own nn.GRU (fp32) on the same device beside them for context.  HIP events, warm-up first.
usage: python tools/probe/gru_probe.py [iters]"""
import sys

import torch

sys.path.insert(0, "vq-vae-transformer-arc-welding_amd")
from arcweld import gru as G  # noqa: E402
from arcweld import kernels as K  # noqa: E402
from arcweld.precision import operands  # noqa: E402

B, T, I, H, L = 512, 5, 400, 758, 6


def timed(fn, iters, warm=3):
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


def main(iters=20):
    dev = "cuda"
    torch.manual_seed(0)
    ref = torch.nn.GRU(I, H, L, batch_first=True).to(dev)
    names = [f"{n}_l{k}" for k in range(L) for n in ("weight_ih", "weight_hh", "bias_ih", "bias_hh")]
    ps = [getattr(ref, n).detach().clone().requires_grad_() for n in names]
    layers = [tuple(ps[4 * k:4 * k + 4]) for k in range(L)]
    x = torch.randn(B, T, I, device=dev)
    gout = torch.randn(B, T, H, device=dev)

    def ours_fwd():
        with torch.no_grad():
            return G.gru_stack(None, x, H, layers)

    def ours_fb():
        out = G.gru_stack(None, x, H, layers)
        torch.autograd.grad(out, ps, gout)

    def torch_fwd():
        with torch.no_grad():
            return ref(x)[0]

    def torch_fb():
        out = ref(x)[0]
        torch.autograd.grad(out, list(ref.parameters()), gout)

    print(f"B {B}  T {T}  in_dim {I}  H {H}  layers {L}   ({iters} iterations)", flush=True)
    print(f"torch nn.GRU fp32: forward {timed(torch_fwd, iters):.0f} us, forward + backward "
          f"{timed(torch_fb, iters):.0f} us", flush=True)
    Hp = K.gru_padded(H)
    for dt in (torch.float32, torch.bfloat16):
        tag = str(dt)[6:]
        with operands(dt):
            print(f"arcweld {tag} operands: forward {timed(ours_fwd, iters):.0f} us, forward + backward "
                  f"{timed(ours_fb, iters):.0f} us", flush=True)
        bf = dt == torch.bfloat16
        e = lambda *s, d=torch.float32: torch.randn(*s, device=dev).to(d)  # noqa: E731
        w_fwd, w_bwd = torch.empty(3, Hp, Hp, device=dev, dtype=dt), torch.empty(Hp, 3 * Hp, device=dev, dtype=dt)
        K.gru_pack_weights(ps[1].detach(), H, w_fwd, w_bwd)
        gi, bhh, hp = e(B, 3 * Hp), e(3 * H), e(B, Hp)
        h, saved = e(B, Hp), torch.rand(B, 4 * Hp, device=dev)
        hb = torch.empty(B, Hp, device=dev, dtype=torch.bfloat16) if bf else None
        hp_op = hp.to(dt)
        dgh_n, dh_n, dy = e(B, 3 * Hp, d=dt), e(B, Hp), e(B, Hp)
        dh, dgi, dgh = e(B, Hp), e(B, 3 * Hp), e(B, 3 * Hp)
        dgi_b = torch.empty(B, 3 * Hp, device=dev, dtype=torch.bfloat16) if bf else None
        dgh_b = torch.empty(B, 3 * Hp, device=dev, dtype=torch.bfloat16) if bf else None
        n = 10 * iters
        t_f = timed(lambda: K.gru_step_fwd(H, dt, gi, bhh, h, saved, w_fwd=w_fwd, h_prev_op=hp_op, h_prev=hp, h_op=hb),
                    n)
        t_f0 = timed(lambda: K.gru_step_fwd(H, dt, gi, bhh, h, saved, h_op=hb), n)
        t_b = timed(lambda: K.gru_step_bwd(H, dt, saved, dh, dgi, dgh, w_bwd=w_bwd, dgh_next_op=dgh_n, dh_next=dh_n,
                                           saved_next=saved, dy=dy, h_prev=hp, dgi_op=dgi_b, dgh_op=dgh_b), n)
        t_b0 = timed(lambda: K.gru_step_bwd(H, dt, saved, dh, dgi, dgh, dy=dy, h_prev=hp, dgi_op=dgi_b, dgh_op=dgh_b), n)
        print(f"  step kernels, {tag}: fwd {t_f:.1f} us (zero state, no GEMM: {t_f0:.1f} us), bwd {t_b:.1f} us "
              f"(last step, no GEMM: {t_b0:.1f} us) per launch, back to back on one stream", flush=True)


if __name__ == "__main__":
    main(int(sys.argv[1]) if len(sys.argv) > 1 else 20)
