"""aw_attn_decode called directly: KV-cache append + causal attention of the new rows, against fp64 attention over the
cached history and the new rows.  Head sizes above 64 (the strided output loop) and odd ones, n_new > 1 at pos0 > 0,
key counts crossing 64, and pos0 + n_new == Tmax; every cache position at or past pos0 holds NaN beforehand, so a read
past the causal limit shows in y and a write outside [pos0, pos0 + n_new) shows in the cache."""
import pytest
import torch

import kernel_refs as kr

pytestmark = pytest.mark.gpu

# (B, n_head, hs, Tmax, pos0, n_new)
CASES = [(2, 2, 16, 40, 0, 1), (2, 3, 6, 70, 0, 33), (3, 2, 64, 130, 63, 1), (3, 2, 64, 130, 64, 1),
         (3, 2, 64, 130, 65, 2), (1, 1, 128, 70, 10, 5), (2, 8, 64, 321, 300, 21)]


def _run(B, nh, hs, Tmax, pos0, n_new, dtype):
    from arcweld import kernels as K
    g = torch.Generator().manual_seed(hs * 1000 + pos0 * 10 + n_new)
    d = nh * hs
    qkv = torch.randn(B * n_new, 3 * d, generator=g).to(dtype).cuda()
    hist = torch.randn(B, pos0, 2 * d, generator=g).to(dtype).cuda()
    cache = torch.full((B, Tmax, 2 * d), float("nan"), device="cuda", dtype=dtype)
    cache[:, :pos0] = hist
    y = torch.full((B * n_new, d), float("nan"), device="cuda", dtype=dtype)
    K.attn_decode(qkv, B, n_new, pos0, nh, d, cache, y)
    torch.cuda.synchronize()

    new_kv = qkv.view(B, n_new, 3 * d)[:, :, d:]
    assert torch.equal(cache[:, :pos0], hist)
    assert torch.equal(cache[:, pos0:pos0 + n_new], new_kv)
    assert torch.isnan(cache[:, pos0 + n_new:]).all()
    assert torch.isfinite(y).all()

    kv_all = torch.cat([hist, new_kv], dim=1).double()
    q = qkv.view(B, n_new, 3 * d)[:, :, :d].double().view(B, n_new, nh, hs)
    k_all = kv_all[:, :, :d].reshape(B, pos0 + n_new, nh, hs)
    v_all = kv_all[:, :, d:].reshape(B, pos0 + n_new, nh, hs)
    ref = kr.attn_cached_ref(q, k_all, v_all, pos0).reshape(B * n_new, d)
    extra = kr.BF16_REL if dtype == torch.bfloat16 else 0.0
    print(f"attn_decode {(B, nh, hs, Tmax, pos0, n_new)} {dtype}: max err {kr.max_err(y, ref):.3e}")
    torch.testing.assert_close(y.double(), ref, rtol=1e-4 + extra, atol=1e-4)
    return qkv, y


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
@pytest.mark.parametrize("B,nh,hs,Tmax,pos0,n_new", CASES)
def test_attn_decode(B, nh, hs, Tmax, pos0, n_new, dtype):
    _run(B, nh, hs, Tmax, pos0, n_new, dtype)


def test_attn_decode_prefill_matches_attn_fwd():
    """pos0 = 0 with n_new = T is a whole causal forward: the same rows as aw_attn_fwd on the same qkv."""
    from arcweld import kernels as K
    B, nh, hs, Tmax, pos0, T = CASES[1]
    qkv, y = _run(B, nh, hs, Tmax, pos0, T, torch.float32)
    d = nh * hs
    y_fwd = torch.empty(B * T, d, device="cuda")
    lse = torch.empty(B * nh * T, device="cuda")
    K.attn_fwd(qkv, B, T, nh, d, y_fwd, lse)
    torch.cuda.synchronize()
    torch.testing.assert_close(y, y_fwd, rtol=1e-4, atol=1e-4)
