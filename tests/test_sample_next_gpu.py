"""aw_sample_next (the generation loop's token choice in one launch): greedy against torch.argmax over the allowed,
filtered columns; sampling against an f64 restatement of the filtered softmax CDF, using the kernel's own draws u; the
draws themselves; the sampled distribution; temperature, bad rows and the vocabulary limit."""
import numpy as np
import pytest
import torch

from oracle import gen

pytestmark = pytest.mark.gpu

VS, BS = (34, 514, 8194), (1, 5)


def _logits(seed, B, V):
    return gen.normal(seed, (B, V), std=3.0)


def _run(logits, col=0, ld=1, **kw):
    """One launch: returns (ids (B,), u (B,), bad count)."""
    from arcweld import kernels as K
    lg = torch.as_tensor(logits, device="cuda")
    B = lg.shape[0]
    out = torch.full((B, ld), -7, dtype=torch.int64, device="cuda")
    u = torch.full((B,), -1.0, device="cuda")
    bad = torch.zeros(1, dtype=torch.int32, device="cuda")
    K.sample_next(lg, out, col, bad, u_out=u, **kw)
    return out[:, col].cpu().numpy(), u.cpu().numpy(), int(bad.item())


def _filtered(logits, n_valid, top_k, inv_t=1.0):
    """The reference's filter on the allowed columns, in f32 as the kernel sees them: (x (B, n_valid) f32, keep)."""
    x = (np.asarray(logits, dtype=np.float32)[:, :n_valid] * np.float32(inv_t)).astype(np.float32)
    keep = np.ones_like(x, dtype=bool)
    if top_k:
        kth = np.sort(x, axis=1)[:, ::-1][:, top_k - 1:top_k]
        keep = x >= kth                      # logits[logits < v[:, [-1]]] = -inf: ties at the threshold stay
    return x, keep


def _cdf64(x, keep):
    z = np.where(keep, x.astype(np.float64), -np.inf)
    p = np.exp(z - z.max(axis=1, keepdims=True))
    p /= p.sum(axis=1, keepdims=True)
    return p, np.cumsum(p, axis=1)


@pytest.mark.parametrize("B", BS)
@pytest.mark.parametrize("V", VS)
def test_greedy_is_argmax_over_the_allowed_filtered_columns(V, B):
    lg = _logits(3100 + V + B, B, V)
    for n_valid in (V, V - 2):
        for top_k in (None, 1, 7):
            ids, _, bad = _run(lg, n_valid=n_valid, top_k=top_k, do_sample=False)
            x, keep = _filtered(lg, n_valid, top_k)
            want = torch.argmax(torch.tensor(np.where(keep, x, -np.inf)), dim=1).numpy()
            assert bad == 0 and np.array_equal(ids, want), (n_valid, top_k)


def test_greedy_never_returns_an_excluded_column_and_breaks_ties_low():
    V = 514
    lg = _logits(3110, 5, V)
    lg[:, V - 2] = lg.max() + 5.0            # the two largest logits of every row sit in the excluded columns
    lg[:, V - 1] = lg.max() + 1.0
    ids, _, _ = _run(lg, n_valid=V - 2)
    assert (ids < V - 2).all() and np.array_equal(ids, lg[:, :V - 2].argmax(1))
    sids, _, _ = _run(lg, n_valid=V - 2, do_sample=True, seed=3)
    assert (sids < V - 2).all() and (sids >= 0).all()
    tie = _logits(3111, 2, V)
    tie[:, 400] = tie[:, 77] = tie.max() + 1.0          # an exact tie of the maximum: the lower index wins
    ids, _, _ = _run(tie)
    assert (ids == 77).all()
    ids, _, _ = _run(tie, top_k=1)
    assert (ids == 77).all()


_M64 = (1 << 64) - 1


def _hash_group(s, g):
    """aw_hash_group as include/arcweld_amd.h states it (64-bit, wrapping)."""
    z = (s + (g + 1) * 0x9E3779B97F4A7C15) & _M64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & _M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & _M64
    return z ^ (z >> 31)


def _host_u(seed, step, B, row):
    """The documented draw (include/arcweld_amd.h): the keyed 24-bit permutation of the counter step*B + row."""
    c = step * B + row
    key = _hash_group(seed & _M64, c >> 24)
    left, right = (c >> 12) & 0xFFF, c & 0xFFF
    for i in range(4):
        left, right = right, left ^ (_hash_group((key + i) & _M64, right) >> 52)
    return float(left << 12 | right) * 2.0 ** -24


def test_top_k_keeps_ties_at_the_threshold():
    """k = 2 with the 2nd and 3rd largest equal: both stay.  The seed is chosen on the host so that u lands well
    inside the second tied column, which a filter that cut at exactly k columns would have dropped."""
    V, k = 34, 2
    lg = _logits(3120, 1, V)
    lg[0, 9] = 9.0
    lg[0, 4] = lg[0, 21] = 8.5
    x, keep = _filtered(lg, V, k)
    assert keep.sum() == 3
    p, c = _cdf64(x, keep)
    seed = next(s for s in range(256) if c[0, 20] + 1e-3 < _host_u(s, 0, 1, 0) < c[0, 21] - 1e-3)
    ids, u, bad = _run(lg, top_k=k, do_sample=True, seed=seed, step=0)
    assert bad == 0 and u[0] == np.float32(_host_u(seed, 0, 1, 0))
    assert ids[0] == 21
    for s in range(32):                      # and nothing outside the three kept columns, whatever u
        ids, _, _ = _run(lg, top_k=k, do_sample=True, seed=1000 + s)
        assert ids[0] in (4, 9, 21)


def test_sampling_follows_the_f64_cdf_with_the_kernels_own_draws():
    """Returned id j: c[j-1] - d <= u < c[j] + d on the f64 inclusive CDF c of the filtered softmax, d = V 2^-24 +
    2^-20 (one f32 rounding per add on partial sums <= 1, a few ulp for exp and the scale); at most 1 % of all rows
    may need the slack."""
    rows = loose = 0
    for V in VS:
        d = V * 2.0 ** -24 + 2.0 ** -20
        for B in BS:
            lg = _logits(3130 + V + B, B, V)
            for n_valid in (V, V - 2):
                for top_k in (None, 7):
                    x, keep = _filtered(lg, n_valid, top_k)
                    p, c = _cdf64(x, keep)
                    for step in range(8):
                        ids, u, bad = _run(lg, n_valid=n_valid, top_k=top_k, do_sample=True, seed=V + B, step=step)
                        assert bad == 0
                        for r in range(B):
                            j, ur = int(ids[r]), float(u[r])
                            assert 0 <= j < n_valid and keep[r, j], (V, B, n_valid, top_k, step, r, j)
                            lo = c[r, j - 1] if j > 0 else 0.0
                            assert lo - d <= ur < c[r, j] + d, (V, B, n_valid, top_k, step, r, j, ur, lo, c[r, j])
                            rows += 1
                            loose += not (lo <= ur < c[r, j])
    print(f"{loose} of {rows} rows needed the slack")
    assert loose <= 0.01 * rows


@pytest.fixture(scope="module")
def draw_streams():
    """The kernel's u for seed 0 and 1, step 0..15, B = 256: 4096 draws per seed, computed once."""
    lg = _logits(3140, 256, 34)
    return [np.concatenate([_run(lg, do_sample=True, seed=seed, step=step)[1] for step in range(16)])
            for seed in (0, 1)]


def test_the_draws_are_uniform_and_seeded(draw_streams):
    for us in draw_streams:
        assert us.shape == (4096,) and (us >= 0).all() and (us < 1).all()
        assert abs(us.mean() - 0.5) <= 0.02          # 4.4 sigma of a uniform mean over 4096 draws; deterministic
    assert not np.array_equal(draw_streams[0], draw_streams[1])
    # the documented formula, on a few (seed, step, row)
    for seed, step, row in ((0, 0, 0), (1, 15, 255), (0, 7, 100)):
        assert draw_streams[seed][step * 256 + row] == np.float32(_host_u(seed, step, 256, row))


@pytest.mark.parametrize("seed", [0, 1])
def test_the_draws_of_one_seed_are_all_distinct(draw_streams, seed):
    """All 4096 draws of a seed are distinct.  The draw is a keyed permutation of the counter's low 24 bits, so this
    holds by construction for any seed; the plain top 24 bits of the counter hash gave 4094 distinct values for
    seed 1 (4096 values of 24 bits collide somewhere with probability 1 - exp(-4096^2 / 2^25) = 0.39 per seed)."""
    us = draw_streams[seed]
    print(f"seed {seed}: {np.unique(us).size} distinct of {us.size}")
    assert np.unique(us).size == 4096


def test_sampled_distribution_matches_the_softmax():
    B, V = 4096, 6
    row = np.array([1.0, 0.0, -1.0, 2.0, 0.5, -3.0], dtype=np.float32)
    lg = np.tile(row, (B, 1))
    ids, _, bad = _run(lg, do_sample=True, seed=11)
    assert bad == 0
    p = np.exp(row.astype(np.float64) - row.max())
    p /= p.sum()
    counts = np.bincount(ids, minlength=V)
    sigma = np.sqrt(B * p * (1 - p))
    assert (np.abs(counts - B * p) <= 5 * sigma).all(), (counts, B * p, sigma)


def test_temperature_scales_the_logits():
    lg = _logits(3150, 5, 514)
    for kw in (dict(do_sample=True, seed=5, step=3), dict(do_sample=True, top_k=7, seed=6), dict(do_sample=False)):
        a, _, _ = _run(lg, inv_temperature=2.0, **kw)
        b, _, _ = _run(lg * np.float32(2.0), inv_temperature=1.0, **kw)
        assert np.array_equal(a, b), kw


@pytest.mark.parametrize("do_sample", [False, True])
def test_bad_rows_store_minus_one_and_are_counted(do_sample):
    V = 514
    lg = _logits(3160, 5, V)
    lg[1, 100] = np.nan                       # a NaN among the allowed columns
    lg[3, :V - 2] = -np.inf                   # no finite allowed logit (the excluded columns do not count)
    lg[4, V - 1] = np.nan                     # a NaN in an excluded column is not looked at
    ids, _, bad = _run(lg, n_valid=V - 2, do_sample=do_sample, seed=2)
    assert bad == 2 and ids[1] == -1 and ids[3] == -1
    clean = _logits(3160, 5, V)
    want, _, _ = _run(clean, n_valid=V - 2, do_sample=do_sample, seed=2)
    assert np.array_equal(ids[[0, 2, 4]], want[[0, 2, 4]])


def test_ids_land_in_the_asked_column_only():
    lg = _logits(3170, 5, 34)
    from arcweld import kernels as K
    out = torch.full((5, 9), -7, dtype=torch.int64, device="cuda")
    bad = torch.zeros(1, dtype=torch.int32, device="cuda")
    K.sample_next(torch.tensor(lg, device="cuda"), out, 4, bad)
    out = out.cpu().numpy()
    assert np.array_equal(out[:, 4], lg.argmax(1))
    assert (np.delete(out, 4, axis=1) == -7).all()


def test_oversized_vocabulary_is_refused_before_any_launch():
    from arcweld import _native
    lg = np.zeros((2, 16385), dtype=np.float32)
    lg[:, 3] = 1.0
    from arcweld import kernels as K
    out = torch.full((2, 1), -7, dtype=torch.int64, device="cuda")
    bad = torch.zeros(1, dtype=torch.int32, device="cuda")
    with pytest.raises(_native.NativeError, match="16384"):
        K.sample_next(torch.tensor(lg, device="cuda"), out, 0, bad)
    torch.cuda.synchronize()
    assert (out == -7).all() and int(bad.item()) == 0
    ok, _, _ = _run(np.ascontiguousarray(lg[:, :16384]))           # the largest vocabulary that is served
    assert (ok == 3).all()
