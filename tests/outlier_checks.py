"""Checks of the outlier kernels' outputs that hold for every row, in float64 numpy on top of the restatements of
test_outlier_cpu.py and test_outlier_kde_cpu.py.  No row is filtered out: where a float32 distance engine may
legitimately choose another neighbour at a near-tie, the check is a two-sided bound (the "sandwich") derived from the
engine's error bound, not a comparison on the rows without near-ties.

The sandwich.  Let d_(1) <= d_(2) <= ... be the true sorted distances of a query row and let the engine rank the reference
rows by d2' with |d2' - d2| <= tau.  The t truly nearest rows have d2' <= d_(t)^2 + tau, so the selected k >= t rows
include t rows with d2' <= d_(t)^2 + tau, whose true d2 is at most d_(t)^2 + 2 tau.  The refined list is the selected set
sorted by true distance, and no subset's t-th smallest lies below the global t-th smallest, hence

    d_(t)^2 <= D[q, t - 1]^2 <= d_(t)^2 + 2 tau.

For a relative bound |d2' - d2| <= rho d2 the same argument gives D^2 <= d_(t)^2 (1 + rho) / (1 - rho), that is
tau = rho d_(t)^2 / (1 - rho).
"""
import numpy as np

from test_outlier_cpu import restate_knn_score, restate_lof, restate_neighbors
from test_outlier_kde_cpu import restate_sq_dists

EPS32 = 2.0 ** -24
ENGINES = ("exact", "gram")
ADVERSARIAL = ["normal", "offset100", "scales", "lowrank", "shifted_query"]


# ---- data ------------------------------------------------------------------------------------------------------------
def adversarial(name, n, d, seed):
    """float32 [n, d].  Every restatement takes this float32 data cast to float64.  "shifted_query" is the query side of
    its case (the reference side is "normal" with another seed): see adversarial_pair."""
    rng = np.random.default_rng(seed)
    base = rng.normal(size=(n, d))
    # the per-feature draws come from a generator of their own, so that reference and query sets built with different
    # seeds share the feature scales, offsets and the low-rank map
    frng = np.random.default_rng(977)
    if name == "normal":
        data = base
    elif name == "offset100":
        data = base + 100.0
    elif name == "scales":  # feature scales over six decades, offsets of a few sigma (adversarial_case of test_hip_parity.py)
        sc = 10.0 ** frng.uniform(-3, 3, size=(1, d))
        data = (base + frng.uniform(-3, 3, size=(1, d))) * sc
    elif name == "lowrank":  # 4 latent factors: distances vary widely while the norms (offset 30) stay alike
        data = rng.normal(size=(n, 4)) @ frng.normal(size=(4, d)) + 0.05 * base + 30.0
    elif name == "shifted_query":
        data = base + 5.0
    else:
        raise ValueError(name)
    return np.ascontiguousarray(data, dtype=np.float32)


def adversarial_pair(name, nr, nq, d, seed):
    """(reference rows [nr, d], query rows [nq, d]) of a case; the queries of "shifted_query" lie 5 sigma per feature away
    from an N(0, 1) reference cloud."""
    ref = adversarial("normal" if name == "shifted_query" else name, nr, d, seed)
    return ref, adversarial(name, nq, d, seed + 1)


# ---- sorted true distances ---------------------------------------------------------------------------------------------
def sorted_sq_dists(D2, k, exclude_self):
    """restate_neighbors from a squared-distance matrix of restate_sq_dists (the same sums): (dist [nq, k + 1], idx
    [nq, k + 1]) sorted by (distance, index), padded with inf / -1."""
    D = np.sqrt(D2)
    if exclude_self:
        np.fill_diagonal(D, np.inf)
    order = None
    if D.shape[1] > 4 * (k + 1):  # partition first; exact only if no tie straddles the (k + 1)-th value
        cand = np.sort(np.argpartition(D, k, axis=1)[:, :k + 1], axis=1)
        vals = np.take_along_axis(D, cand, axis=1)
        if ((D <= vals.max(axis=1, keepdims=True)).sum(axis=1) == k + 1).all():
            order = np.take_along_axis(cand, np.argsort(vals, axis=1, kind="stable"), axis=1)
    if order is None:
        order = np.argsort(D, axis=1, kind="stable")[:, :k + 1]
    dist = np.take_along_axis(D, order, axis=1)
    if order.shape[1] < k + 1:
        pad = k + 1 - order.shape[1]
        order = np.pad(order, ((0, 0), (0, pad)), constant_values=-1)
        dist = np.pad(dist, ((0, 0), (0, pad)), constant_values=np.inf)
    return dist, order


def refine_lists(sel, D2):
    """What the refine step makes of a selected index set sel [nq, k]: the float64 distances of its pairs rounded to
    float32, each row sorted by (float32 distance, index).  Returns (D float32 [nq, k], I int32 [nq, k])."""
    sel = np.asarray(sel, np.int64)
    dist = np.sqrt(np.take_along_axis(D2, sel, axis=1)).astype(np.float32)
    order = np.lexsort((sel, dist), axis=1)
    return np.take_along_axis(dist, order, axis=1), np.take_along_axis(sel, order, axis=1).astype(np.int32)


def _true_lists(Xq, Xr, feats, k, exclude_self, D2):
    if D2 is None:
        return restate_neighbors(Xq, Xr, feats, k, exclude_self)[0], restate_sq_dists(Xq, Xr, feats)
    return sorted_sq_dists(D2, k, exclude_self)[0], D2


# ---- the engines' error bounds -----------------------------------------------------------------------------------------
def d2_tolerance(engine, Xq, Xr, feats, d2=None):
    """Bound on the engine's error in a squared distance, per query row.
    gram:  64 eps32 sqrt(d_s) (qn + rmax), [nq, 1]: the cancellation bound of test_outlier_gpu.py, qn the query row's and
           rmax the largest reference row's squared norm about the float64 column mean of the reference rows.
    exact: (w_s + 2) eps32 d2, w_s = round4(d_s): the bound of kde_tolerance, relative to each pair's own d2 (an array
           [nq, ...], required)."""
    feats = np.asarray(feats)
    ds = len(feats)
    if engine == "gram":
        A = np.asarray(Xr, np.float64)[:, feats]
        c = A.mean(axis=0)
        rmax = ((A - c) ** 2).sum(axis=1).max()
        qn = ((np.asarray(Xq, np.float64)[:, feats] - c) ** 2).sum(axis=1)
        return (64 * EPS32 * np.sqrt(ds) * (qn + rmax))[:, None]
    if engine == "exact":
        return ((ds + 3) // 4 * 4 + 2) * EPS32 * np.asarray(d2, np.float64)
    raise ValueError(engine)


def sandwich_tau(engine, Xq, Xr, feats, d2_sorted):
    """tau [nq, k] of the sandwich at every list position: d2_sorted [nq, k] holds d_(t+1)^2 at position t."""
    if engine == "gram":
        return np.broadcast_to(d2_tolerance(engine, Xq, Xr, feats), d2_sorted.shape)
    rho = ((len(feats) + 3) // 4 * 4 + 2) * EPS32
    return d2_tolerance(engine, Xq, Xr, feats, d2_sorted) / (1.0 - rho)


def upper_envelope(engine, Xq, Xr, feats, true_dist):
    """sqrt(d_(t+1)^2 + 2 tau) [nq, k]: the largest distance position t of a correct list may hold."""
    d2 = true_dist ** 2
    return np.sqrt(d2 + 2.0 * sandwich_tau(engine, Xq, Xr, feats, d2))


def sandwich_use(I, Xq, Xr, feats, k, exclude_self, engine, D2=None, true=None):
    """max over rows and positions of (D[q, t]^2 - d_(t+1)^2) / (2 tau), D recomputed in float64 from the returned
    indices I [nq, k]: the share of the sandwich a list uses (0 when it holds the true neighbours, <= 1 for a list the
    engine's bound allows).  true: the sorted true distances [nq, >= k] if the caller has them."""
    if true is None or D2 is None:
        true, D2 = _true_lists(Xq, Xr, feats, k, exclude_self, D2)
    d2 = true[:, :k] ** 2
    tau = sandwich_tau(engine, Xq, Xr, feats, d2)
    got = np.sort(np.take_along_axis(D2, np.asarray(I, np.int64), axis=1), axis=1)
    err = got - d2
    err = np.where(err > 4e-16 * d2, err, 0.0)  # d2 went through a square root and back
    with np.errstate(divide="ignore", invalid="ignore"):
        use = np.where(err > 0, err / (2.0 * tau), 0.0)
    return float(use.max())


# ---- the checks --------------------------------------------------------------------------------------------------------
def check_neighbor_lists(D, I, Xq, Xr, feats, k, exclude_self, engine, D2=None):
    """Asserts for every row of the lists (D float32 [nq, k], I int [nq, k]) of Xq among Xr in the subspace feats: valid
    distinct indices (not the row's own when exclude_self), D the float32 rounding of the float64 distance of its index,
    (distance, index) order, and the sandwich against the true sorted distances.  D2: restate_sq_dists(Xq, Xr, feats) if
    the caller has it.  Returns sandwich_use."""
    D, I = np.asarray(D), np.asarray(I)
    nq, nr = np.asarray(Xq).shape[0], np.asarray(Xr).shape[0]
    assert D.shape == (nq, k) and I.shape == (nq, k), (D.shape, I.shape, nq, k)
    true, D2 = _true_lists(Xq, Xr, feats, k, exclude_self, D2)
    true = true[:, :k]
    assert ((I >= 0) & (I < nr)).all(), "index outside [0, nr)"
    srt = np.sort(I, axis=1)
    dup = (srt[:, 1:] == srt[:, :-1]).any(axis=1)
    assert not dup.any(), ("repeated index in rows", np.flatnonzero(dup)[:8])
    if exclude_self:
        own = (I == np.arange(nq)[:, None]).any(axis=1)
        assert not own.any(), ("own index in rows", np.flatnonzero(own)[:8])
    # the refine step computes in float64: only the rounding to float32 may differ
    pair = np.sqrt(np.take_along_axis(D2, I.astype(np.int64), axis=1))
    np.testing.assert_allclose(D, pair, rtol=1e-6, atol=1e-30, err_msg="distance of the returned index")
    Df = D.astype(np.float64)
    ordered = (Df[:, 1:] > Df[:, :-1]) | ((Df[:, 1:] == Df[:, :-1]) & (I[:, 1:] > I[:, :-1]))
    assert ordered.all(), ("not in (distance, index) order in rows", np.flatnonzero(~ordered.all(axis=1))[:8])
    low = Df >= true * (1.0 - 1e-6)
    assert low.all(), ("below the true t-th distance in rows", np.flatnonzero(~low.all(axis=1))[:8])
    upper = upper_envelope(engine, Xq, Xr, feats, true)
    high = Df <= upper * (1.0 + 1e-6)  # 1e-6: float32 rounding of D
    bad = np.flatnonzero(~high.all(axis=1))
    assert high.all(), ("above the sandwich in rows", bad[:8], Df[bad[:1]], true[bad[:1]], upper[bad[:1]])
    return sandwich_use(I, Xq, Xr, feats, k, exclude_self, engine, D2=D2, true=true)


def check_knn_scores(per_row_scores, Xq, Xr, feats, k, knn_method, exclude_self, engine, D2=None):
    """The sandwich through restate_knn_score (largest, mean and median are monotone in every distance):
    want (1 - 1e-5) <= got <= score of the upper envelope + 1e-5 want, every row."""
    got = np.asarray(per_row_scores, np.float64)
    true, _ = _true_lists(Xq, Xr, feats, k, exclude_self, D2)
    true = true[:, :k]
    want = restate_knn_score(true, k, knn_method)
    assert got.shape == want.shape, (got.shape, want.shape)
    assert np.isfinite(got).all()
    top = restate_knn_score(upper_envelope(engine, Xq, Xr, feats, true), k, knn_method)
    low, high = got >= want * (1.0 - 1e-5), got <= top + 1e-5 * want
    bad = np.flatnonzero(~(low & high))
    assert (low & high).all(), (knn_method, "rows", bad[:8], got[bad[:4]], want[bad[:4]], top[bad[:4]])


def check_lof_scores(per, D_fit, I_fit, D_q, I_q, k):
    """LOF restated in float64 from the lists the kernels read (float32 distances as float64), rtol 1e-5 on every row.
    The lists themselves must have passed check_neighbor_lists first: that is the half which ties them to the data."""
    got = np.asarray(per, np.float64)
    want = restate_lof(np.asarray(D_fit, np.float64), np.asarray(I_fit, np.int64), np.asarray(D_q, np.float64),
                       np.asarray(I_q, np.int64), k)
    assert got.shape == want.shape, (got.shape, want.shape)
    assert np.isfinite(got).all()
    np.testing.assert_allclose(got, want, rtol=1e-5, atol=0)


def kde_tolerance(D2, want, ds, h, exclude_self, engine, d2_abs=None):
    """Per-row bound on |score - restatement|: 1e-5 relative, 1e-6 absolute for the float32 sums of the exp2 terms and
    the float32 output, plus the float32 error of the engine's d2 carried through the logsumexp.  A d2 error of at most
    e_r moves -log p by at most max_r e_r / (2 h^2) over the rows that carry weight; the exact engine's sum of w_s
    non-negative squares is within (w_s + 2) eps32 relative, so there the move is at most (w_s + 2) eps32 times the
    softmax-weighted mean of d2 / (2 h^2).  The Gram engine's error is absolute, d2_abs per row (the cancellation bound
    of test_outlier_gpu.py)."""
    L = -D2 / (2.0 * h * h)
    if exclude_self:
        L = L.copy()
        np.fill_diagonal(L, -np.inf)
    w = np.exp(L - L.max(axis=1, keepdims=True))
    w /= w.sum(axis=1, keepdims=True)
    energy = np.nansum(w * np.where(np.isfinite(L), -L, 0.0), axis=1)
    tol = 1e-5 * np.abs(want) + 1e-6 + (ds + 6) * EPS32 * energy
    if engine == "gram":
        tol += d2_abs / (2.0 * h * h)
    return tol


def check_kde_scores(scores, Xq, Xr, feats, h, exclude_self, engine, D2=None):
    """|score - restate_kde_from_sq_dists| <= kde_tolerance on every row (the Gram engine's d2 bound is d2_tolerance)."""
    from test_outlier_kde_cpu import restate_kde_from_sq_dists
    got = np.asarray(scores, np.float64)
    D2 = restate_sq_dists(Xq, Xr, feats) if D2 is None else D2
    want = restate_kde_from_sq_dists(D2, len(feats), h, exclude_self)
    assert got.shape == want.shape, (got.shape, want.shape)
    assert np.isfinite(got).all()
    d2_abs = d2_tolerance("gram", Xq, Xr, feats)[:, 0] if engine == "gram" else None
    tol = kde_tolerance(D2, want, len(feats), h, exclude_self, engine, d2_abs)
    err = np.abs(got - want)
    bad = np.flatnonzero(err > tol)
    assert (err <= tol).all(), ("rows", bad[:8], float((err / tol).max()), got[bad[:4]], want[bad[:4]])
    return float((err / tol).max())
