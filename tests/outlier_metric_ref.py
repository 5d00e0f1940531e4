"""Float64 numpy restatements of the metrics of the neighbour search (vgan_amd.outlier.SubspaceEnsemble, metric= / p=) and the
row-wise checks of the lists the kernels return, on top of outlier_checks.py.  Every check covers every row.

The generalised sandwich.  Let the selection rank the reference rows by g' with |g' - g| <= rho g, g the exact ranking value
(Manhattan: the sum of |x_f - y_f|; Chebyshev: their maximum; Minkowski: the sum of |x_f - y_f|^p, no root).  The argument of
outlier_checks.py then gives, for position t of a correct list, g_(t) <= g <= g_(t) (1 + rho) / (1 - rho), and in distances
d_(t) <= D <= d_(t) ((1 + rho) / (1 - rho))^(1/p) (p = 1 for Manhattan and Chebyshev).  The cosine selection ranks by the Gram
engine's d2 = 2 - 2 cos = 2 (cosine distance) with an absolute error of at most tau, so d_(t) <= D <= d_(t) + tau there.

rho, in units of eps32 = 2^-24, from the arithmetic of csrc/outlier_metric.hpp (never from device output):
  Manhattan   w_s + 2: one rounding of x_f - y_f (the operands are the raw values), |.| is exact, at most w_s - 1 float32
              additions of non-negative terms.
  Chebyshev   2: one rounding of x_f - y_f; the maximum is exact.
  Minkowski   w_s + 2 + U_p.  A term is exp2f(p log2f(a)), a = fl(|x_f - y_f|):
                a carries the relative error eps32 of the subtraction, a^p therefore p eps32;
                log2f is within 1 ulp, L' = L (1 + 2 eps32); the product p L' is rounded once: the exponent is off by at most
                3 eps32 |p L| absolutely, the term by ln 2 times that, relatively: 2.08 eps32 |p log2 a|;
                exp2f is within 1 ulp: 2 eps32.
              U_p = p + 2 + 2.08 M, M the largest |p log2 |x_f - y_f|| over the non-zero differences of the case's data (a
              zero difference gives log2f(0) = -inf and exp2f(-inf) = 0, an exact term).  All terms are non-negative, so the
              sum inherits the largest relative error of a term, plus the w_s - 1 additions.
  cosine      tau = 64 eps32 sqrt(d_s) (|u_q|^2 + max_r |u_r|^2): outlier_checks.d2_tolerance("gram", ...) evaluated on the unit
              rows u about the origin (|u|^2 = 1, or 0 for a zero row), as an error of d2; the cosine distance is d2 / 2 and the
              sandwich spends 2 tau of d2, that is tau of distance.
"""
import numpy as np

from outlier_checks import EPS32
from test_outlier_cpu import restate_knn_score

FAMILY = ("manhattan", "chebyshev", "minkowski")


# ---- the distances ---------------------------------------------------------------------------------------------------------
def metric_dists(Xq, Xr, feats, metric, p=None):
    """float64 [nq, nr]: the distance of every pair over the features feats, from the data taken as float64, features
    ascending.  cosine: 1 - <x, y> / (|x| |y|) clipped to [0, 2], exactly 1 where a norm is exactly 0 (scipy: NaN)."""
    A = np.asarray(Xq, np.float64)[:, feats]
    B = np.asarray(Xr, np.float64)[:, feats]
    D = np.zeros((A.shape[0], B.shape[0]))
    if metric == "cosine":
        for f in range(A.shape[1]):
            D += A[:, f, None] * B[None, :, f]
        na, nb = np.sqrt((A * A).sum(axis=1)), np.sqrt((B * B).sum(axis=1))
        den = na[:, None] * nb[None, :]
        with np.errstate(divide="ignore", invalid="ignore"):
            out = np.clip(1.0 - D / den, 0.0, 2.0)
        return np.where(den > 0, out, 1.0)
    for f in range(A.shape[1]):
        e = np.abs(A[:, f, None] - B[None, :, f])
        if metric == "euclidean":
            D += e * e
        elif metric == "manhattan":
            D += e
        elif metric == "chebyshev":
            np.maximum(D, e, out=D)
        elif metric == "minkowski":
            D += e ** p
        else:
            raise ValueError(metric)
    if metric == "euclidean":
        return np.sqrt(D)
    return D ** (1.0 / p) if metric == "minkowski" else D


def sorted_lists(D, k, exclude_self):
    """(dist [nq, k + 1], idx [nq, k + 1]) in (distance, index) order from a distance matrix; inf / -1 where there is no row."""
    D = D.copy()
    if exclude_self:
        np.fill_diagonal(D, np.inf)
    order = np.argsort(D, axis=1, kind="stable")[:, :k + 1]
    dist = np.take_along_axis(D, order, axis=1)
    if order.shape[1] < k + 1:
        pad = k + 1 - order.shape[1]
        order = np.pad(order, ((0, 0), (0, pad)), constant_values=-1)
        dist = np.pad(dist, ((0, 0), (0, pad)), constant_values=np.inf)
    return dist, order


def metric_neighbors(Xq, Xr, feats, k, exclude_self, metric, p=None):
    return sorted_lists(metric_dists(Xq, Xr, feats, metric, p), k, exclude_self)


def refine_metric_lists(sel, D):
    """What the refine step makes of a selected index set sel [nq, k]: float32 roundings of the float64 distances D of its
    pairs, sorted by (float32 distance, index)."""
    sel = np.asarray(sel, np.int64)
    dist = np.take_along_axis(D, sel, axis=1).astype(np.float32)
    order = np.lexsort((sel, dist), axis=1)
    return np.take_along_axis(dist, order, axis=1), np.take_along_axis(sel, order, axis=1).astype(np.int32)


# ---- the bounds --------------------------------------------------------------------------------------------------------------
def power_term_bound(Xq, Xr, feats, p):
    """U_p of the module docstring from the data range of the case."""
    A = np.asarray(Xq, np.float64)[:, feats]
    B = np.asarray(Xr, np.float64)[:, feats]
    M = 0.0
    for f in range(A.shape[1]):
        e = np.abs(A[:, f, None] - B[None, :, f])
        e = e[e > 0]
        if e.size:
            M = max(M, float(np.abs(p * np.log2(e)).max()))
    return p + 2.0 + 2.08 * M


def metric_rho(metric, Xq, Xr, feats, p=None):
    w = (len(feats) + 3) // 4 * 4
    if metric == "manhattan":
        return (w + 2) * EPS32
    if metric == "chebyshev":
        return 2 * EPS32
    if metric == "minkowski":
        return (w + 2 + power_term_bound(Xq, Xr, feats, p)) * EPS32
    raise ValueError(metric)


def cosine_tau(Xq, Xr, feats):
    """[nq, 1]: the Gram engine's bound on d2 of the unit rows about the origin (see the module docstring)."""
    def unit_sq(X):
        A = np.asarray(X, np.float64)[:, feats]
        n = np.sqrt((A * A).sum(axis=1, keepdims=True))
        U = np.divide(A, n, out=np.zeros_like(A), where=n > 0)
        return (U * U).sum(axis=1)
    return (64 * EPS32 * np.sqrt(len(feats)) * (unit_sq(Xq) + unit_sq(Xr).max()))[:, None]


def metric_upper_envelope(true, Xq, Xr, feats, metric, p=None):
    """[nq, k]: the largest distance position t of a correct list may hold, from the true sorted distances."""
    if metric == "cosine":
        return true + cosine_tau(Xq, Xr, feats)
    rho = metric_rho(metric, Xq, Xr, feats, p)
    return true * ((1.0 + rho) / (1.0 - rho)) ** (1.0 / (p if metric == "minkowski" else 1.0))


def metric_sandwich_use(I, D_all, true, Xq, Xr, feats, metric, p=None):
    """max over rows and positions of (D - d_(t)) / (envelope - d_(t)), D from the returned indices in float64: 0 for the true
    neighbours, <= 1 for a list the bound allows."""
    k = np.asarray(I).shape[1]
    got = np.sort(np.take_along_axis(D_all, np.asarray(I, np.int64), axis=1), axis=1)
    room = metric_upper_envelope(true[:, :k], Xq, Xr, feats, metric, p) - true[:, :k]
    err = got - true[:, :k]
    err = np.where(err > 4e-16 * np.maximum(true[:, :k], 1e-300), err, 0.0)
    with np.errstate(divide="ignore", invalid="ignore"):
        use = np.where(err > 0, err / room, 0.0)
    return float(use.max())


# ---- the checks --------------------------------------------------------------------------------------------------------------
def check_metric_lists(D, I, Xq, Xr, feats, k, exclude_self, metric, p=None, D_all=None):
    """outlier_checks.check_neighbor_lists under another metric, every row: valid distinct indices (not the row's own when
    exclude_self), D the float32 rounding of the float64 distance of its index, (distance, index) order, the sandwich.
    Returns the share of the sandwich the lists use."""
    D, I = np.asarray(D), np.asarray(I)
    nq, nr = np.asarray(Xq).shape[0], np.asarray(Xr).shape[0]
    assert D.shape == (nq, k) and I.shape == (nq, k), (D.shape, I.shape, nq, k)
    D_all = metric_dists(Xq, Xr, feats, metric, p) if D_all is None else D_all
    true = sorted_lists(D_all, k, exclude_self)[0][:, :k]
    assert ((I >= 0) & (I < nr)).all(), "index outside [0, nr)"
    srt = np.sort(I, axis=1)
    dup = (srt[:, 1:] == srt[:, :-1]).any(axis=1)
    assert not dup.any(), ("repeated index in rows", np.flatnonzero(dup)[:8])
    if exclude_self:
        own = (I == np.arange(nq)[:, None]).any(axis=1)
        assert not own.any(), ("own index in rows", np.flatnonzero(own)[:8])
    pair = np.take_along_axis(D_all, I.astype(np.int64), axis=1)
    # cosine: 1 - cos cancels; the float64 error of the difference is absolute, of the order of 1e-16
    np.testing.assert_allclose(D, pair, rtol=1e-6, atol=1e-12 if metric == "cosine" else 1e-30,
                               err_msg="distance of the returned index")
    Df = D.astype(np.float64)
    ordered = (Df[:, 1:] > Df[:, :-1]) | ((Df[:, 1:] == Df[:, :-1]) & (I[:, 1:] > I[:, :-1]))
    assert ordered.all(), ("not in (distance, index) order in rows", np.flatnonzero(~ordered.all(axis=1))[:8])
    slack = 1e-12 if metric == "cosine" else 0.0
    low = Df >= true * (1.0 - 1e-6) - slack
    assert low.all(), ("below the true t-th distance in rows", np.flatnonzero(~low.all(axis=1))[:8])
    upper = metric_upper_envelope(true, Xq, Xr, feats, metric, p)
    high = Df <= upper * (1.0 + 1e-6) + slack  # 1e-6: float32 rounding of D
    bad = np.flatnonzero(~high.all(axis=1))
    assert high.all(), ("above the sandwich in rows", bad[:8], Df[bad[:1]], true[bad[:1]], upper[bad[:1]])
    return metric_sandwich_use(I, D_all, true, Xq, Xr, feats, metric, p)


def check_metric_knn_scores(per_row_scores, Xq, Xr, feats, k, knn_method, exclude_self, metric, p=None):
    """outlier_checks.check_knn_scores under another metric: want (1 - 1e-5) <= got <= score of the envelope + 1e-5 want."""
    got = np.asarray(per_row_scores, np.float64)
    true = metric_neighbors(Xq, Xr, feats, k, exclude_self, metric, p)[0][:, :k]
    want = restate_knn_score(true, k, knn_method)
    assert got.shape == want.shape, (got.shape, want.shape)
    assert np.isfinite(got).all()
    top = restate_knn_score(metric_upper_envelope(true, Xq, Xr, feats, metric, p), k, knn_method)
    low, high = got >= want * (1.0 - 1e-5) - 1e-12, got <= top + 1e-5 * want + 1e-12
    bad = np.flatnonzero(~(low & high))
    assert (low & high).all(), (knn_method, "rows", bad[:8], got[bad[:4]], want[bad[:4]], top[bad[:4]])


def roc_auc(scores, n_outliers):
    """ROC AUC of scores whose first n_outliers rows are the outliers (rank statistic, ties counted half)."""
    s = np.asarray(scores, np.float64)
    pos, neg = s[:n_outliers], s[n_outliers:]
    return float(((pos[:, None] > neg[None, :]).sum() + 0.5 * (pos[:, None] == neg[None, :]).sum()) / (len(pos) * len(neg)))
