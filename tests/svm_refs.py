"""fp64 numpy restatements of the RBF-SVM probe (csrc/svm.hip, arcweld.retrieve.svm_*), for the CPU and the GPU tests:
the kernel matrix with its error bound, a dense SMO solver with the selection rule of include/arcweld_amd.h, rho, the
objective, the decision function, the one-vs-one vote, the KKT gap of a given alpha and scikit-learn's gamma='scale'.
Nothing here is tuned to the code under test.

The bound of a Gram element.  The kernel evaluates, in f32 with u = 2^-24,
    k = expf(fl(-gamma * max(dist, 0))),   dist = fl(fl(|a|^2 + |b|^2) - 2 dot(a, b)).
A sum of d terms accumulated in ANY order has error <= d u sum |terms| to first order ((1 + u)^d - 1 <= 1.01 d u for
d u < 0.01; the f32-input MFMA is bit for bit an fmaf chain, one rounding per term); none of the bounds is measured.
  norms    d roundings on the running sum, stated with one to spare:   |d|a|^2| <= (d + 1) u |a|^2, the same for b;
  dot      |d dot| <= d u sum_i |a_i b_i|, and it enters twice;
  the sum  fl(|a|^2 + |b|^2) rounds once: u (|a|^2 + |b|^2);
  dist     fl(s - 2 dot) rounds once: u |dist| <= 2 u (|a|^2 + |b|^2)   (|s - 2 dot| <= 2 (|a|^2 + |b|^2));
           together, with S = |a|^2 + |b|^2:
               eps_dist = 1.01 u ((d + 4) S + 2 d sum_i |a_i b_i|)
           the clamp at 0 moves dist towards the true value (which is >= 0) and adds nothing;
  product  fl(gamma * dist) rounds once: the argument x = gamma dist has
               eps_x = gamma eps_dist + u gamma (dist64 + eps_dist)
  expf     the derivative of exp(-x) is the element itself: an argument error e changes k by at most
           k64 (exp(e) - 1) in either direction; expf is documented at 1 ulp = 2 u relative (HIP math API), on a
           value of at most k64 exp(eps_x):
               eps_k = k64 expm1(eps_x) + 2 u k64 exp(eps_x) + 2^-126
           the last term covers results in the subnormal range, where an absolute spacing replaces the relative one
           and expf may flush to zero.
gamma is the f32 value the kernel receives.
"""
import numpy as np

U = 2.0 ** -24
TAU = 1e-12


# ------------------------------------------------------------------------------------------------ the Gram matrix
def sqdist64(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    out = np.empty((len(a), len(b)))
    step = max(1, (1 << 22) // max(1, b.size))
    for o in range(0, len(a), step):
        out[o:o + step] = ((a[o:o + step, None, :] - b[None, :, :]) ** 2).sum(-1)
    return out


def gram64(a, b, gamma):
    """(na, nb) exp(-gamma |a_i - b_j|^2) in f64 from the f32 values; gamma as the kernel receives it (f32)."""
    return np.exp(-float(np.float32(gamma)) * sqdist64(a, b))


def eps_dist(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    d = a.shape[1]
    S = (a * a).sum(-1)[:, None] + (b * b).sum(-1)[None, :]
    return 1.01 * U * ((d + 4) * S + 2 * d * (np.abs(a) @ np.abs(b).T))


def eps_gram(a, b, gamma):
    """(na, nb) bound on |k_f32(i, j) - gram64(i, j)| (module docstring)."""
    g = float(np.float32(gamma))
    ed = eps_dist(a, b)
    ex = g * ed + U * g * (sqdist64(a, b) + ed)
    k = gram64(a, b, gamma)
    return k * np.expm1(ex) + 2 * U * k * np.exp(ex) + 2.0 ** -126


def gram32(a, b, gamma, order=None):
    """The kernel's expression restated in f32 numpy, the dims accumulated in `order` (default ascending): one valid
    evaluation order, to check on the CPU that eps_gram bounds an f32 evaluation."""
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    aa, bb = np.zeros(len(a), np.float32), np.zeros(len(b), np.float32)
    dot = np.zeros((len(a), len(b)), np.float32)
    for c in (range(a.shape[1]) if order is None else order):
        aa = (aa + a[:, c] * a[:, c]).astype(np.float32)
        bb = (bb + b[:, c] * b[:, c]).astype(np.float32)
        dot = (dot + a[:, c, None] * b[None, :, c]).astype(np.float32)
    s = (aa[:, None] + bb[None, :]).astype(np.float32)
    dist = np.maximum((s - np.float32(2.0) * dot).astype(np.float32), np.float32(0))
    return np.exp((np.float32(-gamma) * dist).astype(np.float32)).astype(np.float32)


def rbf_gamma(x):
    """scikit-learn's gamma='scale': 1 / (D var), var the population variance over all elements; 1.0 at zero variance."""
    x = np.asarray(x, np.float64)
    var = x.var()
    return 1.0 / (x.shape[1] * var) if var > 0 else 1.0


# ------------------------------------------------------------------------------------------------ the solver
def masks(y, alpha, C):
    y, alpha = np.asarray(y), np.asarray(alpha)
    up = ((y > 0) & (alpha < C)) | ((y < 0) & (alpha > 0))
    low = ((y > 0) & (alpha > 0)) | ((y < 0) & (alpha < C))
    return up, low


def gap_of(G, y, alpha, C):
    """(m - M, m, M) of a state; -inf when either candidate set is empty."""
    v = -np.asarray(y, np.float64) * G
    up, low = masks(y, alpha, C)
    m = v[up].max() if up.any() else -np.inf
    M = v[low].min() if low.any() else np.inf
    return m - M, m, M


def smo(K, y, C, tol=1e-3, max_iter=10 ** 7, alpha=None, grad=None):
    """The C-SVC dual on the kernel matrix K (n, n) by SMO: libsvm's second-order working-set selection and its
    two-variable update, every tie to the lowest row; y in {-1, 0, +1}, rows with y = 0 take no part.  Dense f64.
    Starts from alpha = 0, grad = -1, or resumes from the state given.  Returns alpha, grad, n_iter, gap."""
    K = np.asarray(K, np.float64)
    y = np.asarray(y, np.float64)
    n = len(y)
    alpha = np.zeros(n) if alpha is None else np.array(alpha, np.float64)
    G = -np.ones(n) if grad is None else np.array(grad, np.float64)
    act = y != 0
    Kd = np.diag(K).copy() if n else np.zeros(0)
    it = 0
    while True:
        gap, m, M = gap_of(G, y, alpha, C)
        if not gap > tol or it >= max_iter:
            return alpha, G, it, gap
        v = -y * G
        up, low = masks(y, alpha, C)
        i = int(np.argmax(np.where(up, v, -np.inf)))                  # the first of the maxima
        b = m - v
        a = Kd[i] + Kd - 2.0 * K[i]
        a = np.where(a <= 0, TAU, a)
        cand = low & (v < m)
        j = int(np.argmin(np.where(cand, -(b * b) / a, np.inf)))      # the first of the minima
        ai, aj, yi, yj = alpha[i], alpha[j], y[i], y[j]
        quad = a[j]
        if yi != yj:
            delta = (-G[i] - G[j]) / quad
            diff = ai - aj
            ai, aj = ai + delta, aj + delta
            if diff > 0:
                if aj < 0:
                    aj, ai = 0.0, diff
            elif ai < 0:
                ai, aj = 0.0, -diff
            if diff > 0:
                if ai > C:
                    ai, aj = C, C - diff
            elif aj > C:
                aj, ai = C, C + diff
        else:
            delta = (G[i] - G[j]) / quad
            s = ai + aj
            ai, aj = ai - delta, aj + delta
            if s > C:
                if ai > C:
                    ai, aj = C, s - C
            elif aj < 0:
                aj, ai = 0.0, s
            if s > C:
                if aj > C:
                    aj, ai = C, s - C
            elif ai < 0:
                ai, aj = 0.0, s
        dai, daj = ai - alpha[i], aj - alpha[j]
        alpha[i], alpha[j] = ai, aj
        G[act] += ((y * yi * K[i]) * dai + (y * yj * K[j]) * daj)[act]
        it += 1


def grad64(K, y, alpha):
    """G = Q alpha - e recomputed in f64, Q_st = y_s y_t K_st; 0 on rows with y = 0."""
    y = np.asarray(y, np.float64)
    return np.where(y != 0, y * (np.asarray(K, np.float64) @ (y * np.asarray(alpha, np.float64))) - 1.0, 0.0)


def kkt_gap(K, y, C, alpha):
    """m - M of alpha with the gradient recomputed from scratch."""
    return gap_of(grad64(K, y, alpha), y, alpha, C)[0]


def objective(alpha, G, y):
    act = np.asarray(y) != 0
    return 0.5 * float((np.asarray(alpha)[act] * (np.asarray(G)[act] - 1.0)).sum())


def rho(alpha, G, y, C):
    """libsvm's rule: the mean of y G over the free rows, else the midpoint of the bounds the rows at the box give (a
    side without a bound takes the other's; neither: 0)."""
    y = np.asarray(y, np.float64)
    alpha, yG = np.asarray(alpha), y * np.asarray(G)
    act = y != 0
    free = act & (alpha > 0) & (alpha < C)
    if free.any():
        return float(yG[free].mean())
    at_up, at_lo = act & (alpha >= C), act & (alpha <= 0)
    ub_set = (at_up & (y < 0)) | (at_lo & (y > 0))
    lb_set = (at_up & (y > 0)) | (at_lo & (y < 0))
    ub = yG[ub_set].min() if ub_set.any() else None
    lb = yG[lb_set].max() if lb_set.any() else None
    if ub is None and lb is None:
        return 0.0
    if ub is None or lb is None:
        return float(lb if ub is None else ub)
    return float((ub + lb) / 2.0)


def fit(K, y, C, tol=1e-3, max_iter=10 ** 7):
    """One problem solved from scratch: dict of alpha, grad, n_iter, gap, rho, objective, coef = alpha y."""
    alpha, G, it, gap = smo(K, y, C, tol, max_iter)
    return {"alpha": alpha, "grad": G, "n_iter": it, "gap": gap, "rho": rho(alpha, G, y, C),
            "objective": objective(alpha, G, y), "coef": alpha * np.asarray(y, np.float64)}


def decision(Kq, coef, rho_):
    """(nq,) decision values for the kernel rows Kq (nq, n) of the queries against the training rows."""
    return np.asarray(Kq, np.float64) @ np.asarray(coef, np.float64) - rho_


def pairs_of(n_classes):
    """(positive class, negative class) per problem: (1, 0) for two classes, else every a < b as (a, b)."""
    return [(1, 0)] if n_classes == 2 else [(a, b) for a in range(n_classes) for b in range(a + 1, n_classes)]


def pair_labels(labels, pairs):
    """y (n_pairs, n) in {-1, 0, +1}."""
    labels = np.asarray(labels)
    return np.stack([(labels == a).astype(np.int32) - (labels == b).astype(np.int32) for a, b in pairs])


def vote(dec, pairs, n_classes):
    """Class ids (n,) from the decisions (n, n_pairs): a problem votes for its positive class where dec > 0, else for
    its negative one; the most votes win, ties to the lowest class id."""
    dec = np.asarray(dec)
    votes = np.zeros((dec.shape[0], n_classes), np.int64)
    for p, (a, b) in enumerate(pairs):
        votes[np.arange(dec.shape[0]), np.where(dec[:, p] > 0, a, b)] += 1
    return votes.argmax(1)


# ------------------------------------------------------------------------------------------------ data
def blobs(seed, n, d, sep=1.0, n_classes=2, share=None):
    """n rows of N(0, 1) features (f32) whose class c is shifted by sep * c along a seeded unit direction; labels from
    a seeded draw (share: the probability of class 1 for two classes, default 1/2)."""
    from oracle import gen
    x = gen.normal(seed, (n, d)).astype(np.float64)
    w = gen.normal(seed + 7919, (d,)).astype(np.float64)
    w /= np.linalg.norm(w)
    if n_classes == 2 and share is not None:
        y = (gen.uniform(seed + 104729, (n,)) < share).astype(np.int64)
    else:
        y = gen.randint(seed + 104729, (n,), 0, n_classes)
    return (x + sep * y[:, None] * w[None, :]).astype(np.float32), y
