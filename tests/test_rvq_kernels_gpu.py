"""csrc/rvq.hip called directly: per-code sums, the k-means mean update, the residual step and the EMA codebook update
with dead-code replacement.  The EMA update's expired-code ranks come from a scan over chunks of 1024 codes; K = 1025
and 2500 place expired codes in every chunk (every other test of the suite uses K = 64)."""
import numpy as np
import pytest
import torch

from oracle import residual_vq as orv

pytestmark = pytest.mark.gpu


def _K():
    from arcweld import kernels
    return kernels


@pytest.mark.parametrize("N,D,K", [(7, 4, 3), (1000, 16, 64), (5000, 64, 1500)])
def test_vq_cluster_sums(N, D, K):
    g = torch.Generator().manual_seed(N)
    z = torch.randn(N, D, generator=g)
    idx = torch.randint(1, K, (N,), generator=g)             # code 0 stays empty ...
    idx[idx == K - 1] = 1                                     # ... and so does the last one
    idx[torch.arange(N) % 3 == 0] = K // 2                    # one code takes a third of the rows
    sums = torch.zeros(K, D, device="cuda")
    _K().vq_cluster_sums(z.cuda(), idx.cuda(), K, sums)
    torch.cuda.synchronize()
    ref = torch.zeros(K, D, dtype=torch.float64).index_add_(0, idx, z.double())
    mag = torch.zeros(K, D, dtype=torch.float64).index_add_(0, idx, z.double().abs())
    n_k = torch.bincount(idx, minlength=K).double()
    assert n_k[0] == 0 and n_k[K - 1] == 0 and n_k[K // 2] >= N // 3
    # order-independent bound of n_k - 1 f32 additions: (n_k - 1) * 2^-24 * sum|z|
    tol = (n_k - 1).clamp(min=0)[:, None] * 2.0 ** -24 * mag
    err = (sums.double().cpu() - ref).abs()
    assert (err <= tol).all(), f"max excess {(err - tol).max().item():.3e}"
    assert torch.count_nonzero(sums[0]) == 0


def _within_one_ulp(got, ref):
    got, ref = got.numpy(), ref.numpy()
    return bool((np.abs(got.astype(np.float64) - ref) <= np.spacing(np.abs(ref))).all())


@pytest.mark.parametrize("with_avg", [True, False])
@pytest.mark.parametrize("K,D", [(3, 4), (1500, 64)])
def test_kmeans_update(K, D, with_avg):
    g = torch.Generator().manual_seed(K)
    means0, sums = torch.randn(K, D, generator=g), torch.randn(K, D, generator=g) * 5
    counts = torch.randint(0, 4, (K,), generator=g).float()
    counts[0], counts[K - 1] = 0.0, 7.0
    means = means0.clone().cuda()
    avg = torch.full((K, D), float("nan"), device="cuda") if with_avg else None
    _K().kmeans_update(means, sums.cuda(), counts.cuda(), avg)
    torch.cuda.synchronize()
    ref = torch.where(counts[:, None] > 0, sums / counts[:, None].clamp(min=1), means0)
    empty = counts == 0
    assert torch.equal(means.cpu()[empty], means0[empty])                       # empty clusters keep their mean
    assert _within_one_ulp(means.cpu(), ref)
    if with_avg:
        assert _within_one_ulp(avg.cpu(), means.cpu() * counts[:, None])        # avg = mean * count


@pytest.mark.parametrize("first", [True, False])
@pytest.mark.parametrize("with_next", [True, False])
def test_rvq_residual(first, with_next):
    g = torch.Generator().manual_seed(5)
    N, D = 5000, 64
    r, zq, out0 = (torch.randn(N, D, generator=g).cuda() for _ in range(3))
    out = out0.clone()
    r_next = torch.full((N, D), float("nan"), device="cuda") if with_next else None
    _K().rvq_residual(r, zq, out, first, r_next)
    torch.cuda.synchronize()
    assert torch.equal(out, zq if first else out0 + zq)
    if with_next:
        assert torch.equal(r_next, r - zq)


def _ema_cases():
    for K in (64, 1024, 1025, 2500):
        yield K, "none", None
        for ctr in (None, 11):
            yield K, "few", ctr           # n_exp <= N: one row of each of n_exp strata
            yield K, "many", ctr          # n_exp > N (N = 5, 40 expired): rows drawn with replacement


@pytest.mark.parametrize("K,expiry,ctr", list(_ema_cases()))
def test_rvq_ema_update(K, expiry, ctr):
    g = torch.Generator().manual_seed(K + len(expiry))
    D = 8
    N = 5 if expiry == "many" else 50
    decay, eps = float(np.float32(0.8)), float(np.float32(1e-5))
    threshold = 0.0 if expiry == "none" else 2.0
    salt = 0xA5A5_0123_4567_89AB
    # dying codes: the first and last code of every chunk of 1024 and one in the middle of it
    if expiry == "many":
        dying = np.unique(np.linspace(0, K - 1, 40).astype(np.int64))
        assert len(dying) == 40
    else:
        dying = np.unique([c for k0 in range(0, K, 1024) for c in (k0, min(k0 + 1023, K - 1), min(k0 + 500, K - 1))])
    dying_t = torch.zeros(K, dtype=torch.bool)
    dying_t[torch.from_numpy(dying)] = True
    cs0 = torch.where(dying_t, 0.5 + 0.5 * torch.rand(K, generator=g), 10 + 10 * torch.rand(K, generator=g))
    counts = torch.where(dying_t, torch.zeros(K), torch.randint(5, 30, (K,), generator=g).float())
    embed0, eavg0, sums = (torch.randn(K, D, generator=g) for _ in range(3))
    z = torch.randn(N, D, generator=g)

    embed, eavg, cs = embed0.clone().cuda(), eavg0.clone().cuda(), cs0.clone().cuda()
    ws = torch.empty(2 * K, device="cuda")
    seed_ptr = None if ctr is None else torch.tensor([ctr], device="cuda", dtype=torch.int64)
    _K().rvq_ema_update(embed, eavg, cs, counts.cuda(), sums.cuda(), z.cuda(), decay, eps, threshold, salt, seed_ptr, ws)
    torch.cuda.synchronize()

    c = cs0.double() * decay + counts.double() * (1 - decay)
    if threshold > 0:   # no EMA'd size within a factor 2 of the threshold: f32 rounding cannot flip an expiry
        assert ((c >= 2 * threshold) | (c <= threshold / 2)).all()
    expired = (c < threshold) if threshold > 0 else torch.zeros(K, dtype=torch.bool)
    assert torch.equal(expired, dying_t if threshold > 0 else torch.zeros(K, dtype=torch.bool))
    total = c.sum()
    smooth = (c + eps) / (total + K * eps) * total
    eavg_ref = eavg0.double() * decay + sums.double() * (1 - decay)
    embed_ref = eavg_ref / smooth[:, None]
    cs_ref = torch.where(expired, torch.full_like(c, threshold), c)
    rows = orv.dead_code_rows(expired.numpy(), N, salt, ctr)
    ex = expired.numpy()
    if ex.any():
        zr = z[torch.from_numpy(rows[ex])]
        assert torch.equal(embed.cpu()[expired], zr), "replacement rows differ from oracle.dead_code_rows"
        embed_ref[expired] = zr.double()
        eavg_ref[expired] = zr.double() * threshold
        if expiry == "few":
            assert len(set(rows[ex].tolist())) == int(ex.sum())       # distinct rows, one per stratum
    # relative 1e-5.  The sizes are sums of positive terms; embed_avg is a signed two-term sum, so its bar is relative
    # to the magnitude of its terms (a rounding of either term is not relative to a cancelled result)
    torch.testing.assert_close(cs.double().cpu(), cs_ref, rtol=1e-5, atol=0.0)
    mag = eavg0.double().abs() * decay + sums.double().abs() * (1 - decay)
    mag[expired] = eavg_ref[expired].abs()
    assert ((eavg.double().cpu() - eavg_ref).abs() <= 1e-5 * mag).all()
    live = ~expired
    assert ((embed.double().cpu() - embed_ref).abs()[live] <= (1e-5 * mag / smooth[:, None])[live]).all()
