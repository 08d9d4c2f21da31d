"""fp64 numpy restatements of the batched logistic regression (csrc/logreg.hip) and of the linear probe's host side
(arcweld.retrieve), for the CPU and the GPU tests: the kernels' outputs, the objective with its gradient and Hessian, a
Newton solver, the decision and prediction rules and the stratified subsample.  Nothing here is tuned to the code under
test.

The objective (scikit-learn's LogisticRegression, L2 penalty, unpenalised intercept), per problem:
    F(w, b) = (1 / N) sum_i [softplus(z_i) - t_i z_i] + |w|^2 / (2 C N),   z_i = x_i . w + b,   t_i in {0, 1}.

The bounds.  u = 2^-24 is the unit roundoff of f32; a sum of n terms accumulated in f32 in ANY order has error
<= n u sum |terms| to first order ((1 + u)^n - 1 <= 1.01 n u for n u < 0.01); none of the bounds is measured.
  z     z = fl(dot + b): the dot product of d products (the f32-input MFMA is bit for bit an fmaf chain: one rounding
        per term, so d roundings on the running sum), then one more rounding for the bias:
            |dz_ip| <= (d + 2) u (sum_k |x_ik w_kp| + |b_p|)                                              eps_z
  r     r = fl(sigma(z) - t) with sigma(z) = (z >= 0 ? 1 : e) / fl(1 + e), e = expf(-|z|).  sigma is 1/4-Lipschitz, so
        the error of z contributes |dz| / 4.  The evaluation itself: expf is documented at 1 ulp = 2 u relative; e
        enters 1 / (1 + e) and e / (1 + e) with a relative sensitivity below 1, the add and the correctly rounded
        divide (__fdiv_rn) add u each: 4 u relative on sigma <= 1, and the final subtraction at most u more:
        5 u absolute, stated with C_U = 8:
            |dr_ip| <= |dz_ip| / 4 + C_U u                                                                eps_r
        (a row with y_i < 0 has r = 0 exactly).
  loss  one term is softplus(z) - t z, whose derivative sigma - t lies in [-1, 1]: the error of z contributes at most
        |dz|.  softplus(z) = fl(max(z, 0) + log1pf(e)): log1pf is documented at 1 ulp = 2 u, the 2 u of e pass into
        log1p(e) with sensitivity e / ((1 + e) log1p(e)) <= 1, the add rounds once: 5 u softplus(z), again stated with
        C_U.  The difference and the sum over the rows are f64 (n 2^-53 relative, added for completeness):
            |dloss_p| <= sum_i (|dz_ip| + C_U u softplus(z_ip)) + n 2^-53 sum_i |term_ip|               eps_loss
  gb    the f64 sum of the f32 r: |dgb_p| <= sum_i |dr_ip|                                                 eps_gb
  g     g_kp = sum_i x_ik r_ip: the products of the stored (already rounded) r, accumulated in f32 in some order over
        n rows (the splits' partials are then added in f64):
            |dg_kp| <= sum_i |x_ik| |dr_ip| + (n + 2) u sum_i |x_ik r_ip|                                 eps_g
The device functions the kernel calls are expf, log1pf (HIP math API: maximum error 1 ulp each), __fdiv_rn, __fadd_rn,
__fsub_rn (correctly rounded) and fmaxf / fabsf (exact).
"""
import numpy as np

U = 2.0 ** -24
C_U = 8.0


# ------------------------------------------------------------------------------------------------ the kernels
def softplus(z):
    z = np.asarray(z, np.float64)
    return np.maximum(z, 0.0) + np.log1p(np.exp(-np.abs(z)))


def sigmoid(z):
    z = np.asarray(z, np.float64)
    e = np.exp(-np.abs(z))
    return np.where(z >= 0, 1.0, e) / (1.0 + e)


def targets(y, cls):
    """t (n, p) in {0, 1} and active (n,) bool: rows with y < 0 take no part."""
    y, cls = np.asarray(y), np.asarray(cls)
    return (y[:, None] == cls[None, :]).astype(np.float64), y >= 0


def forward64(x, w, b, y=None, cls=None):
    """z (n, p); with labels also r (n, p), loss (p,), gb (p,), all f64 from the f32 values."""
    x, w, b = (np.asarray(a, np.float64) for a in (x, w, b))
    z = x @ w + b[None, :]
    if y is None:
        return z
    t, act = targets(y, cls)
    r = np.where(act[:, None], sigmoid(z) - t, 0.0)
    loss = np.where(act[:, None], softplus(z) - t * z, 0.0).sum(0)
    return z, r, loss, r.sum(0)


def grad64(x, r):
    return np.asarray(x, np.float64).T @ np.asarray(r, np.float64)


def eps_z(x, w, b):
    x, w, b = (np.asarray(a, np.float64) for a in (x, w, b))
    return (x.shape[1] + 2) * U * (np.abs(x) @ np.abs(w) + np.abs(b)[None, :])


def eps_r(ez, y=None):
    e = ez / 4.0 + C_U * U
    return e if y is None else np.where((np.asarray(y) >= 0)[:, None], e, 0.0)


def eps_loss(ez, z64, y, cls):
    t, act = targets(y, cls)
    term = np.abs(softplus(z64) - t * z64)
    per_row = ez + C_U * U * softplus(z64) + len(z64) * 2.0 ** -53 * term
    return np.where(act[:, None], per_row, 0.0).sum(0)


def eps_gb(er):
    return er.sum(0)


def eps_g(x, r64, er):
    ax = np.abs(np.asarray(x, np.float64))
    return ax.T @ er + (len(ax) + 2) * U * (ax.T @ np.abs(r64))


def bounds(x, w, b, y, cls):
    """Everything at once: dict of the fp64 values and their bounds for one labelled evaluation."""
    z, r, loss, gb = forward64(x, w, b, y, cls)
    ez = eps_z(x, w, b)
    er = eps_r(ez, y)
    return {"z": z, "r": r, "loss": loss, "gb": gb, "g": grad64(x, r), "eps_z": ez, "eps_r": er,
            "eps_loss": eps_loss(ez, z, y, cls), "eps_gb": eps_gb(er), "eps_g": eps_g(x, r, er)}


def eval32(x, w, b, y, cls, order=None, rows=None):
    """The kernels' expressions restated in f32 numpy, the dims accumulated in `order` and the rows in `rows` (default:
    ascending): one valid evaluation order each.  Returns z, r (f32), loss, gb (f64), g (f32 accumulation, as f64)."""
    x, w, b = (np.asarray(a, np.float32) for a in (x, w, b))
    n, d = x.shape
    z = np.zeros((n, w.shape[1]), np.float32)
    for k in (range(d) if order is None else order):
        z = (z + x[:, k, None] * w[None, k, :]).astype(np.float32)
    z = (z + b[None, :]).astype(np.float32)
    e = np.exp(-np.abs(z)).astype(np.float32)
    sig = (np.where(z >= 0, np.float32(1), e) / (np.float32(1) + e)).astype(np.float32)
    sp = (np.maximum(z, np.float32(0)) + np.log1p(e).astype(np.float32)).astype(np.float32)
    t, act = targets(y, cls)
    r = np.where(act[:, None], (sig - t.astype(np.float32)).astype(np.float32), np.float32(0)).astype(np.float32)
    loss = np.where(act[:, None], sp.astype(np.float64) - t * z.astype(np.float64), 0.0).sum(0)
    g = np.zeros((d, w.shape[1]), np.float32)
    for i in (range(n) if rows is None else rows):
        g = (g + x[i, :, None] * r[i, None, :]).astype(np.float32)
    return z, r, loss, r.astype(np.float64).sum(0), g.astype(np.float64)


# ------------------------------------------------------------------------------------------------ the objective
def _aug(x):
    x = np.asarray(x, np.float64)
    return np.concatenate([x, np.ones((len(x), 1))], 1)


def objective(theta, x, t, C):
    """F at theta = [w | b] (d + 1,) for one problem with 0/1 targets t."""
    xa, t = _aug(x), np.asarray(t, np.float64)
    z = xa @ theta
    return float((softplus(z) - t * z).sum() / len(xa) + (theta[:-1] ** 2).sum() / (2.0 * C * len(xa)))


def gradient(theta, x, t, C):
    xa, t = _aug(x), np.asarray(t, np.float64)
    g = xa.T @ (sigmoid(xa @ theta) - t) / len(xa)
    g[:-1] += theta[:-1] / (C * len(xa))
    return g


def hessian(theta, x, C):
    xa = _aug(x)
    s = sigmoid(xa @ theta)
    h = (xa * (s * (1.0 - s))[:, None]).T @ xa / len(xa)
    h[np.arange(len(theta) - 1), np.arange(len(theta) - 1)] += 1.0 / (C * len(xa))
    return h


def newton(x, t, C, gtol=1e-12, max_iter=200):
    """The minimiser of F by damped Newton steps from 0, iterated to max |grad F| <= gtol (asserted)."""
    theta = np.zeros(np.asarray(x).shape[1] + 1)
    for _ in range(max_iter):
        g = gradient(theta, x, t, C)
        if np.abs(g).max() <= gtol:
            return theta
        step = np.linalg.solve(hessian(theta, x, C), g)
        f0, a = objective(theta, x, t, C), 1.0
        # damped only far from the solution: within the last steps F no longer resolves the decrease in f64
        while np.abs(step).max() > 1e-3 and a > 1e-8 and objective(theta - a * step, x, t, C) > f0:
            a *= 0.5
        theta = theta - a * step
    g = gradient(theta, x, t, C)
    assert np.abs(g).max() <= gtol, f"Newton stopped at max |grad F| = {np.abs(g).max():.3g}"
    return theta


def decision(coef, intercept, x):
    """z (n_C, n, K) f64 for coef (n_C, K, d), intercept (n_C, K)."""
    return np.einsum("nd,ckd->cnk", np.asarray(x, np.float64), np.asarray(coef, np.float64)) \
        + np.asarray(intercept, np.float64)[:, None, :]


def predict(z, n_classes):
    """z > 0 for two classes, else the argmax over the classes (ties to the lowest)."""
    return (z[..., 0] > 0).astype(np.int64) if n_classes == 2 else z.argmax(-1)


def fit_conditions(theta, x, t, C, tol, eps_grad):
    """The three conditions of a fit stopped at max |grad F| <= tol by an f32 evaluation whose gradient (of F, i.e.
    already divided by N) is within eps_grad (d + 1,) of the fp64 one.  Returns a dict of figures and the verdicts:
    1. |grad F64(theta)| <= tol + eps_grad, elementwise;
    2. |theta - theta*|_2 <= 2 |grad F64(theta)|_2 / mu*, theta* the Newton solution, mu* the least eigenvalue of the
       Hessian there (strong convexity; the 2 covers the Hessian's variation between the two points);
    3. the predictions equal the reference's on every row with |z*_i| >= |(x_i, 1)|_2 * that bound (Cauchy-Schwarz:
       such a row cannot change sign), and at most 2 % of the rows fall under the threshold."""
    theta = np.asarray(theta, np.float64)
    star = newton(x, t, C)
    g = gradient(theta, x, t, C)
    mu = float(np.linalg.eigvalsh(hessian(star, x, C)).min())
    dist, bound = float(np.linalg.norm(theta - star)), 2.0 * float(np.linalg.norm(g)) / mu
    xa = _aug(x)
    zs, zt = xa @ star, xa @ theta
    safe = np.abs(zs) >= np.linalg.norm(xa, axis=1) * bound
    return {"gmax": float(np.abs(g).max()), "grad_ok": bool((np.abs(g) <= tol + eps_grad).all()),
            "grad_excess": float((np.abs(g) - eps_grad).max()), "dist": dist, "bound": bound,
            "dist_ok": dist <= bound, "under": float((~safe).mean()),
            "pred_ok": bool(((zs > 0) == (zt > 0))[safe].all()), "agree": float(((zs > 0) == (zt > 0)).mean()),
            "theta_star": star}


def grad_bound(theta, x, y, pos, n_rows=None):
    """eps of the f32 gradient OF F (divided by N) at theta = [w | b] for the problem 'class pos against the rest':
    (d + 1,) -- eps_g / N for w, eps_gb / N for b.  The regulariser is evaluated in f64 and adds nothing."""
    theta = np.asarray(theta, np.float64)
    bd = bounds(x, theta[:-1, None], theta[-1:], y, np.array([pos]))
    n = len(np.asarray(x)) if n_rows is None else n_rows
    return np.concatenate([bd["eps_g"][:, 0], bd["eps_gb"]]) / n


# ------------------------------------------------------------------------------------------------ the probe's host side
def stratified_subsample(labels, max_samples, seed=0):
    """Sorted row indices of the subsample: per class floor(max_samples n_c / n) rows plus one for the largest
    remainders (ties to the lower class), the rows being the first of RandomState(seed).permutation(n_c), classes in
    ascending order; everything when n <= max_samples."""
    y = np.asarray(labels)
    n = len(y)
    if n <= max_samples:
        return np.arange(n, dtype=np.int64)
    classes = sorted(set(int(v) for v in y))
    counts = [int((y == c).sum()) for c in classes]
    take = [max_samples * m // n for m in counts]
    rem = [max_samples * m % n for m in counts]
    for i in sorted(range(len(classes)), key=lambda i: (-rem[i], i))[:max_samples - sum(take)]:
        take[i] += 1
    rng = np.random.RandomState(seed)
    rows = []
    for c, m, k in zip(classes, counts, take):
        rows.extend(np.flatnonzero(y == c)[rng.permutation(m)[:k]])
    return np.array(sorted(rows), np.int64)


def problem_data(seed, n, d):
    """N(0, 1) features (f32) with labels from a random linear score plus logistic noise."""
    from oracle import gen
    x = gen.normal(seed, (n, d))
    w = gen.normal(seed + 7919, (d,)).astype(np.float64) / np.sqrt(d)
    u = gen.uniform(seed + 104729, (n,), 1e-6, 1.0 - 1e-6).astype(np.float64)
    y = (x.astype(np.float64) @ w * 2.0 + np.log(u / (1.0 - u)) > 0).astype(np.int64)
    return x, y
