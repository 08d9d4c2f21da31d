"""fp64 numpy restatements of the vector quantizer (csrc/vq.hip: the nearest-code search, finalize, backward, one-hot)
for the CPU and the GPU tests, with the bounds the tests assert.  Nothing here is tuned to the code under test: every
allowance is derived below from the number of f32 roundings of the operation, and tests/test_vq_refs_cpu.py checks each
against an f32 evaluation on the CPU and prints the measured ratio.

u = 2^-24 is the unit roundoff of f32.  A chain s_d = fl(s_{d-1} + x_d) over n terms that starts at 0 rounds each term
at most n times (the first addition, 0 + x, is exact), so its error is at most n u sum |x_d| to first order; the same
holds for a fused chain s_d = fma(a_d, b_d, s_{d-1}) and, counting the product's own rounding, for the mul-then-add
chain s_d = fl(s_{d-1} + fl(a_d b_d)).  A sum of n terms in ANY order (atomics, trees) has n - 1 additions and the same
bound with n - 1.
"""
import types

import numpy as np

U = 2.0 ** -24


# ------------------------------------------------------------------------------------------------ the search
def dist64(z, E):
    """(N, K) |z|^2 + |e|^2 - 2 z.e in f64 from the f32 values (exact for the integer block: every term is an integer
    far below 2^53)."""
    z, E = np.asarray(z, np.float64), np.asarray(E, np.float64)
    with np.errstate(all="ignore"):                     # a NaN row is part of the tests
        return (z * z).sum(1)[:, None] + (E * E).sum(1)[None, :] - 2.0 * (z @ E.T)


def eps(z, E):
    """(N, K) bound on |d_f32(n, k) - dist64(n, k)| that holds for both kernels' rounding orders:

        eps[n, k] = (D + 2) u (|z_n|^2 + |e_k|^2 + 2 sum_d |z_nd| |e_kd|).

    Both kernels evaluate d = fl(fl(|z|^2 + |e|^2) - 2 dot).  The pinned kernel (K <= 512, D <= 64) sums |z|^2, |e|^2
    and the dot product as fma chains over the D embedding values (the f32-input MFMA is such a chain) and ends with
    s = fl(|z|^2 + |e|^2), d = fma(-2, dot, s): one rounding each.  The streaming kernel sums the dot product as an fma
    chain, the norms as mul-then-add chains, and ends with fsub(fadd(|z|^2, |e|^2), fmul(2, dot)); 2 dot is exact.
    By the module docstring every D-long chain is off by at most D u times the sum of its absolute terms:
    D u |z|^2, D u |e|^2 and 2 D u sum |z_d e_d| for 2 dot.  The two final roundings add u (|z|^2 + |e|^2) and
    u |d| <= u (|z|^2 + |e|^2 + 2 sum |z_d e_d|).  The sum is at most (D + 2) u (|z|^2 + |e|^2 + 2 sum |z_d e_d|), to
    first order in u (the second-order remainder is below (D + 2) u = 1.6e-5 of eps itself at D = 256).

    Measured on the CPU (test_vq_refs_cpu.py): the f32 reference expression (torch, oracle.vqvae.vq_quantize's) stays
    below 0.19 eps on every pair of the random regimes of REGIMES (max |d32 - d64| / eps: 0.041, 0.174, 0.012, 0.083,
    0.021, 0.066 in their order), and the fp64 runner-up is rejected on 100, 100, 99.6, 100, 100 and 95.4 % of the
    rows."""
    z, E = np.asarray(z, np.float64), np.asarray(E, np.float64)
    D = z.shape[1]
    with np.errstate(all="ignore"):
        mag = (z * z).sum(1)[:, None] + (E * E).sum(1)[None, :] + 2.0 * (np.abs(z) @ np.abs(E).T)
    return (D + 2) * U * mag


def index_violations(z, E, idx):
    """Rows whose idx no correct f32 search could return: idx outside [0, K), or
    dist64[n, idx] - min_k dist64[n, k] > eps[n, idx] + eps[n, kmin].  An f32 search takes idx over kmin only if
    d32(idx) <= d32(kmin), and each side is within its own eps of dist64.  No row is excluded; wherever the top-2 gap
    exceeds the allowance this forces idx == argmin64."""
    idx = np.asarray(idx)
    N, K = len(z), len(E)
    assert idx.shape == (N,), f"idx shape {idx.shape}, want ({N},)"
    d, e = dist64(z, E), eps(z, E)
    rows = np.arange(N)
    inside = (idx >= 0) & (idx < K)
    safe = np.where(inside, idx, 0)
    kmin = d.argmin(1)
    with np.errstate(all="ignore"):
        excess = d[rows, safe] - d[rows, kmin]
        bad = ~inside | ~(excess <= e[rows, safe] + e[rows, kmin])
    return np.flatnonzero(bad)


def check_indices(z, E, idx, label=""):
    bad = index_violations(z, E, idx)
    assert bad.size == 0, (f"{label}: {bad.size} of {len(z)} rows hold an index outside the fp64 bound, first rows "
                           f"{bad[:8].tolist()} -> idx {np.asarray(idx)[bad[:8]].tolist()}")


def second_best(z, E):
    """(N,) the fp64 runner-up of every row by (distance, index): what a search that loses the winner returns."""
    d = dist64(z, E)
    rows = np.arange(len(z))
    d[rows, d.argmin(1)] = np.inf
    return d.argmin(1)


def sqerr64(z, E, idx):
    z, E = np.asarray(z, np.float64), np.asarray(E, np.float64)
    return float(((E[np.asarray(idx)] - z) ** 2).sum())


# sqerr: per float4 of a row the kernel takes d_i = fl(e_i - z_i) (u: 2 u on d_i^2), squares and sums the four in f32
# (one rounding per product and per addition, fused or not: at most 4 u on the sum of non-negative terms), then adds
# in f64 (N D 2^-53: nothing).  6 u to first order; 7 u with the second-order remainder and the f64 tail.  (Measured
# on the MI355X: at most 0.018 of it on the random block; the per-element errors average out over N D terms.)
SQERR_RTOL = 7 * U


def zq_ste32(z, E, idx):
    """The straight-through value the kernels write, in f32: z + (e_idx - z), one rounding per operation."""
    z, E = np.asarray(z, np.float32), np.asarray(E, np.float32)
    with np.errstate(all="ignore"):
        return (z + (E[np.asarray(idx)] - z).astype(np.float32)).astype(np.float32)


# (K, D, N, z std, E std): the regimes the bound and the checker are measured on (CPU) and the kernels run at (GPU).
# K 513 = one code in the second code tile; 8197 = 16 tiles and 5 codes; 100 x 32 is served by the pinned kernel.
REGIMES = ((520, 64, 1000, .08, .08), (513, 16, 999, .08, .08), (8197, 256, 257, .08, .05), (100, 32, 777, 1., 1.),
           (1030, 128, 300, .08, .08), (520, 64, 1000, 5., .01))


def random_case(seed, K, D, N, z_std, e_std):
    """z (N, D), E (K, D) f32: normal rows (e_std None: the untrained codebook U(+-1/K)).  Two rows are planted so that
    the clamped edges decide an answer whatever the seed: row N - 1 next to the last code and row 0 next to code 0
    (a tenth of the codebook's spread away: a search that loses code K - 1, code 0 or row N - 1 is off by far more
    than the bound)."""
    from oracle import gen
    z = gen.normal(seed, (N, D), z_std)
    E = gen.uniform(seed + 1, (K, D), -1.0 / K, 1.0 / K) if e_std is None else gen.normal(seed + 1, (K, D), e_std)
    spread = float(np.abs(E).mean())
    noise = gen.normal(seed + 2, (2, D), 0.1 * spread)
    z[N - 1] = E[K - 1] + noise[0]
    z[0] = E[0] + noise[1]
    return z, E


# ------------------------------------------------------------------------------------------------ the integer block
OFFSETS = (1, 4, 8, 32, 64, 512)     # lane, lane half, MFMA tile, wave (both kernels: 64 codes) and code tile apart


def exact_case(seed, K, D, N, m=3):
    """Integer-valued z and E in -m..m (m <= 3, D <= 256): every product, partial sum and distance is an integer below
    2^24, so an f32 evaluation is exact in any summation order and the kernel must return the fp64 answer bit for bit.

    E is drawn from a pool of about K / 8 distinct rows, each used at least twice, and every z row is a code of E
    with about one value in six moved by +-1: its nearest pool row wins at every copy, so every row has exact ties at many
    index distances (K = 1 has none to offer).  Hand-placed on top:
      * the row s = (m, -m, m, ...) sits at code `base` and at base + OFFSETS (where K allows), and z rows 0 and N // 2
        equal s: distance 0 at every copy, the first must win;
      * two all-zero codes, k = 5 and k = 300 (K - 2 when K <= 301), and an all-zero z row N - 1;
      * the row t = -s sits at the last code K - 1 and nowhere else (K >= 8), and z row 1 equals it (N >= 4): the one
        row WITHOUT a tie, because only a unique winner shows a search that loses the last code or the last code tile
        (a tied last code never wins under the first-index rule).
    Neither s, t nor the zero row is in the pool.  Returns z, E and the exact idx (first index of the minimum), zq,
    counts and sqerr, plus base, the copies of s, the zero codes and `last` (K - 1 where t was placed, else None)."""
    assert 1 <= m <= 3 and D <= 256 and K >= 1 and N >= 1
    rng = np.random.default_rng(seed)
    s = np.where(np.arange(D) % 2 == 0, m, -m).astype(np.float32)
    E = np.empty((K, D), np.float32)
    base = 10 if K >= 12 else 0
    copies = [base + o for o in (0,) + OFFSETS if base + o < K]
    last = K - 1 if K >= 8 and K - 1 not in copies else None
    zeros = [5, 300 if K > 301 else K - 2] if K >= 8 else []
    if zeros and (zeros[1] in copies or zeros[0] in copies):
        zeros = []
    E[np.asarray(copies, np.intp)] = s
    E[np.asarray(zeros, np.intp)] = 0.0
    if last is not None:
        E[last] = -s
    free = np.setdiff1d(np.arange(K), copies + zeros + ([] if last is None else [last]))
    if free.size >= 2:
        P = max(1, free.size // 8)
        pool = np.empty((0, D), np.float32)
        while len(pool) < P:
            cand = rng.integers(-m, m + 1, size=(2 * P + 8, D)).astype(np.float32)
            cand = cand[(cand != 0).any(1) & (cand != s).any(1) & (cand != -s).any(1)]
            pool = np.unique(np.concatenate([pool, cand]), axis=0)
        pool = pool[rng.permutation(len(pool))[:P]]
        ids = np.concatenate([np.arange(P), np.arange(P), rng.integers(P, size=free.size - 2 * P)])
        E[free] = pool[rng.permutation(ids)]
    else:
        E[free] = s
    moved = rng.integers(-1, 2, size=(N, D)) * (rng.integers(0, 4, size=(N, D)) == 0)
    z = np.clip(E[rng.integers(K if last is None else K - 1, size=N)] + moved, -m, m).astype(np.float32)
    z[0] = s
    z[N // 2] = s
    if N >= 2:
        z[N - 1] = 0.0
    if N >= 4 and last is not None:
        z[1] = -s
    d = dist64(z, E)
    idx = d.argmin(1)                       # numpy: the first index of the minimum
    best = d[np.arange(N), idx]
    assert best.max() < 2 ** 24 and np.array_equal(best, np.rint(best))
    return types.SimpleNamespace(z=z, E=E, K=K, D=D, N=N, idx=idx.astype(np.int64), zq=E[idx],
                                 counts=np.bincount(idx, minlength=K).astype(np.float32), sqerr=float(best.sum()),
                                 base=base, copies=copies, zeros=zeros, last=last)


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def check_exact(c, idx, zq, counts, sqerr, label=""):
    """The outputs of one forward over the exact case c, bit for bit.  counts: (groups * K,) partial histograms."""
    idx, zq = np.asarray(idx), np.asarray(zq)
    assert idx.shape == (c.N,) and zq.shape == (c.N, c.D), f"{label}: output shapes"
    bad = np.flatnonzero(idx != c.idx)
    assert bad.size == 0, (f"{label}: idx differs from the fp64 first-index argmin on {bad.size} rows, first "
                           f"{bad[:6].tolist()}: got {idx[bad[:6]].tolist()}, want {c.idx[bad[:6]].tolist()}")
    assert np.array_equal(bits(zq), bits(c.zq)), f"{label}: z_q is not E[idx] bit for bit"
    total = np.asarray(counts, np.float64).reshape(-1, c.K).sum(0)
    assert np.array_equal(total, c.counts), f"{label}: counts differ from bincount(idx)"
    assert float(sqerr) == c.sqerr, f"{label}: sqerr {float(sqerr)!r}, want the integer {c.sqerr!r}"


# ------------------------------------------------------------------------------------------------ finalize
LIBM_ULPS = 4     # logf / expf allowance in units in the last place: numpy's vectorised f32 log / exp document up to
                  # 3.83 / 2.52 ulp, the device library 1 ulp each; the restatement below needs this much against fp64


def finalize_ref(counts, sqerr, N, K, D, beta):
    """(loss, perplexity) in f64: m = sqerr / (N D), loss = m + beta m; p = counts / N,
    perplexity = exp(-sum p log(p + 1e-10)).  counts: (groups * K,) or (K,)."""
    c = np.asarray(counts, np.float64).reshape(-1, K).sum(0)
    m = float(sqerr) / (float(N) * float(D))
    p = c / float(N)
    return m + float(np.float32(beta)) * m, float(np.exp(-(p * np.log(p + 1e-10)).sum()))


# loss: m is one cast of an f64 quotient (u), beta m one product (u), the sum one more (u): 3 u of the result at most
# (one rounding when the two fuse), 4 u with the second-order terms.
LOSS_RTOL = 4 * U


# (kind, K, N, groups): the finalize cases of the CPU and the GPU test
FINALIZE = (("one code", 300, 1000, 1), ("all equal", 8197, 8197 * 3, 8), ("all equal", 257, 257, 1),
            ("empty codes", 255, 100, 8), ("random", 8197, 1000, 1), ("random", 520, 32805, 8), ("one code", 1, 7, 1),
            ("random", 100, 1, 1))


def finalize_counts(kind, K, N, groups, seed=5):
    """(groups * K,) f32 partial histograms of N rows."""
    rng = np.random.default_rng(seed)
    if kind == "one code":
        idx = np.full(N, K // 2)
    elif kind == "all equal":
        idx = np.arange(N) % K
    elif kind == "empty codes":
        idx = rng.integers(0, max(1, K // 10), size=N) * 7 % K
    else:
        idx = rng.integers(0, K, size=N)
    c = np.zeros((groups, K), np.float32)
    np.add.at(c, (rng.integers(0, groups, size=N), idx), 1.0)
    return c.reshape(-1)


def perplexity32(counts, N, K, groups=1):
    """The kernel's own order in f32 numpy: the partial histograms summed group by group, p = c fl(1 / N),
    t = p logf(p + 1e-10f), 256 strided partial sums of ceil(K / 256) terms each (k = t, t + 256, ...), the 8-level
    tree 128, 64, .. 1, then expf(-s)."""
    f = np.float32
    c = np.asarray(counts, f).reshape(groups, K)
    tot = c[0].copy()
    for g in range(1, groups):
        tot = (tot + c[g]).astype(f)
    p = (tot * (f(1.0) / f(N))).astype(f)
    t = (p * np.log((p + f(1e-10)).astype(f)).astype(f)).astype(f)
    rows = np.zeros(-(-K // 256) * 256, f)
    rows[:K] = t
    part = np.zeros(256, f)
    for r in rows.reshape(-1, 256):
        part = (part + r).astype(f)
    o = 128
    while o:
        part[:o] = (part[:o] + part[o:2 * o]).astype(f)
        o >>= 1
    return float(np.exp(f(-part[0])).astype(f))


def perplexity_tol(counts, N, K):
    """Absolute allowance on the f32 perplexity against finalize_ref.  With H = sum |p log(p + 1e-10)| (<= log K):
      * p = fl(c fl(1 / N)) is off by 2 u, p + 1e-10f by one more: 3 u relative on logf's argument = 3 u absolute on
        the logarithm, p times that summed over k (sum p = 1): 3 u;
      * each term p logf(.) carries p's 2 u, logf's LIBM_ULPS ulp (2 u each) and the product's u relative to itself;
      * the sum is 256 strided chains of n = ceil(K / 256) terms and an 8-level tree: (n + 8) u H;
    so |s - s64| <= (n + 11 + 2 LIBM_ULPS) u H + 3 u.  perplexity = expf(-s): its relative error is that of s
    (absolute) plus expf's LIBM_ULPS ulp.
    Measured: perplexity32 on the CPU stays below 0.036 of this allowance on the cases of FINALIZE (empty codes at
    K = 255 the largest; test_vq_refs_cpu.py prints each), the kernel on the MI355X below 0.07 (test_vq_kernels_gpu.py
    prints each).  The worst-case summation bound is that much wider than a typical sum; it is not narrowed."""
    c = np.asarray(counts, np.float64).reshape(-1, K).sum(0)
    p = c / float(N)
    H = float(np.abs(p * np.log(p + 1e-10)).sum())
    n = -(-K // 256)
    ds = (n + 11 + 2 * LIBM_ULPS) * U * H + 3 * U
    return float(np.exp(-(p * np.log(p + 1e-10)).sum())) * (ds + 2 * LIBM_ULPS * U)


# ------------------------------------------------------------------------------------------------ backward / one-hot
def backward_ref(z, E, idx, g_zq, g_loss, beta, dE_prior):
    """(dz, dE) in f64: dz = g_zq - g scale (e_idx - z), dE[k] = prior[k] + sum_{n: idx[n] = k} g beta scale
    (e_k - z_n), scale = 2 / (N D).  g_zq None: no upstream term; g_loss None: g = 0 and dE is the prior, untouched."""
    z, E = np.asarray(z, np.float64), np.asarray(E, np.float64)
    idx = np.asarray(idx)
    N, D = z.shape
    g = 0.0 if g_loss is None else float(g_loss)
    scale = 2.0 / (float(N) * float(D))
    diff = E[idx] - z
    dz = (0.0 if g_zq is None else np.asarray(g_zq, np.float64)) - g * scale * diff
    dE = np.array(dE_prior, np.float64)
    if g != 0.0:
        np.add.at(dE, idx, g * float(np.float32(beta)) * scale * diff)
    return dz, dE


def backward_tols(z, E, idx, g_zq, g_loss, beta, dE_prior):
    """(tol_dz (N, D), tol_dE (K, D)).

    dz: scale = fl(2 / (N D)), diff = fl(e - z), fl(g scale), fl(. diff) and the subtraction: five roundings, the
    first four relative to |g scale diff|, the last to |dz| <= |g_zq| + |g scale diff|: 5 u (|g_zq| + |g scale diff|).

    dE[k]: every term g beta scale diff carries scale's and diff's rounding and the product chain's: fl(g beta),
    fl(. scale), fl(. diff).  The tests take beta = 0.25 and g_loss a power of two, which makes the first two products
    exact: three roundings per term.  The n_k terms of a code are added to the prior by f32 atomics in any order:
    n_k additions.  (n_k + 3) u (|prior| + sum |terms|).
    Measured (f32 numpy restatement on the CPU and the kernel on the MI355X alike): dz at most 0.55 of its allowance,
    dE 0.44; with every row on one code (n_k = 1000) dE stays below 0.02."""
    z, E = np.asarray(z, np.float64), np.asarray(E, np.float64)
    idx = np.asarray(idx)
    N, D = z.shape
    g = 0.0 if g_loss is None else float(g_loss)
    b = float(np.float32(beta))
    assert g == 0.0 or (np.frexp(g)[0] in (0.5, -0.5) and np.frexp(b)[0] == 0.5), "the dE bound wants powers of two"
    scale = 2.0 / (float(N) * float(D))
    term = np.abs(g * scale * (E[idx] - z))
    tol_dz = 5 * U * ((0.0 if g_zq is None else np.abs(np.asarray(g_zq, np.float64))) + term)
    mag = np.abs(np.asarray(dE_prior, np.float64)).copy()
    np.add.at(mag, idx, b * term)
    n_k = np.bincount(idx, minlength=len(E)).astype(np.float64)
    return tol_dz, (n_k[:, None] + 3) * U * mag


def check_backward(z, E, idx, g_zq, g_loss, beta, dE_prior, dz, dE, label=""):
    want_dz, want_dE = backward_ref(z, E, idx, g_zq, g_loss, beta, dE_prior)
    tol_dz, tol_dE = backward_tols(z, E, idx, g_zq, g_loss, beta, dE_prior)
    err_dz, err_dE = np.abs(np.asarray(dz, np.float64) - want_dz), np.abs(np.asarray(dE, np.float64) - want_dE)
    with np.errstate(all="ignore"):
        r_dz = np.nanmax(np.where(tol_dz > 0, err_dz / tol_dz, 0.0)) if err_dz.size else 0.0
        r_dE = np.nanmax(np.where(tol_dE > 0, err_dE / tol_dE, 0.0))
    print(f"{label}: max |dz - dz64| / tol = {r_dz:.3g}, max |dE - dE64| / tol = {r_dE:.3g}")
    assert (err_dz <= tol_dz).all(), f"{label}: dz off by {r_dz:.3g} of its allowance"
    if g_loss is None:
        assert np.array_equal(bits(dE), bits(dE_prior)), f"{label}: dE changed without a loss gradient"
    assert (err_dE <= tol_dE).all(), f"{label}: dE off by {r_dE:.3g} of its allowance"


def onehot_ref(idx, K):
    return (np.asarray(idx)[:, None] == np.arange(K)[None, :]).astype(np.float32)
