"""Stochastic outlier selection over the subspaces, CPU tier: the numpy restatement the GPU tests compare against, pinned to the
scalar loops of the definition on a hand-worked case and to sklearn's ``_binary_search_perplexity``; the properties of the
contract; and everything of vgan_amd.SubspaceSOS that runs without a device (argument checks, the host rules, the dispatch
from the model, the C ABI's argument checks).

The definition is SubspaceSOS's docstring, and restate_sos_fit follows it line for line: the float32 matrix widened to float64,
the shift by the row minimum, the degenerate rule, the search with every operation a numpy operation of its own (numpy
contracts nothing into an FMA), log(perplexity) from the C library (math.log).  The updates of beta are exact (doublings and
means), so given the same float32 D the device reaches the same beta bit for bit unless an exp or log that differs in the last
place flips a comparison; that can happen only where |diff| lies within WINDOW of 0 or of tol, and the restatement flags those
rows."""
import ctypes
import math
import os
import re
from collections import namedtuple

import numpy as np
import pytest

from conftest import REPO
from test_outlier_ecod_cpu import _mask
from test_outlier_ocsvm_cpu import planted_data, ranking_rate, restate_sq_dists, shifted_data

WINDOW = 1e-12
SosFit = namedtuple("SosFit", "beta dmin Z n_iter degenerate unconverged flagged")


# ---- the restatement --------------------------------------------------------------------------------------------------------
def off_diagonal(D):
    """[n, n - 1]: row i without its own entry, the others in ascending j."""
    n = D.shape[0]
    return D[~np.eye(n, dtype=bool)].reshape(n, n - 1)


def restate_sos_fit(D, perplexity, tol=1e-5, max_iter=200):
    """SosFit of the float32 matrix D (row i: D[i, j]); flagged marks the rows on which some step's |diff| lay within WINDOW
    of 0 or of tol."""
    D = np.asarray(D)
    assert D.dtype == np.float32 and D.ndim == 2 and D.shape[0] == D.shape[1]
    n = D.shape[0]
    R = off_diagonal(D).astype(np.float64)
    dmin = R.min(axis=1)
    E = R - dmin[:, None]
    m = (E == 0.0).sum(axis=1)
    degenerate = m >= perplexity
    log_perplexity = math.log(perplexity)
    beta = np.where(degenerate, np.inf, 1.0)
    lo, hi = np.zeros(n), np.full(n, np.inf)
    Z = m.astype(np.float64)
    n_iter = np.zeros(n, np.int32)
    unconverged, flagged = np.zeros(n, bool), np.zeros(n, bool)
    active = np.flatnonzero(~degenerate)
    while active.size:
        b, e = beta[active], E[active]
        a = np.exp(-(b[:, None] * e))
        z = a.sum(axis=1)
        s = (e * a).sum(axis=1)
        diff = (np.log(z) + b * (s / z)) - log_perplexity
        Z[active] = z
        size = np.abs(diff)
        flagged[active] |= (size <= WINDOW) | (np.abs(size - tol) <= WINDOW)
        stop = size <= tol
        late = ~stop & (n_iter[active] >= max_iter)
        unconverged[active[late]] = True
        go = ~stop & ~late
        active, b, up = active[go], b[go], diff[go] > 0.0
        lo_old, hi_old = lo[active], hi[active]
        lo[active] = np.where(up, b, lo_old)
        hi[active] = np.where(up, hi_old, b)
        beta[active] = np.where(up, np.where(np.isinf(hi_old), 2.0 * b, (b + hi_old) / 2.0), (b + lo_old) / 2.0)
        n_iter[active] += 1
    return SosFit(beta, dmin, Z, n_iter, degenerate, unconverged, flagged)


def restate_sos_terms(d, beta, dmin, Z, fitting):
    """float64 [nq, n]: min(t_i, 128) for rows at dissimilarity d[q, i] to fitted row i (the diagonal included)."""
    d = np.asarray(d, np.float64)
    deg = np.isinf(beta)
    with np.errstate(over="ignore", divide="ignore", invalid="ignore"):
        a = np.where(deg[None, :], (d <= dmin[None, :]).astype(np.float64),
                     np.exp(-(np.where(deg, 0.0, beta)[None, :] * (d - dmin[None, :]))))
        r = a / Z[None, :]
        t = -np.log1p(-np.minimum(r, 1.0)) if fitting else np.log1p(r)
    return np.minimum(t, 128.0)


def restate_sos_scores(d, beta, dmin, Z, fitting):
    """float64 [nq]: exp(-(sum_i rint(term 2^40)) 2^-40); fitting leaves i = q out (d square) and takes the fit form."""
    fixed = np.rint(restate_sos_terms(d, beta, dmin, Z, fitting) * 2.0 ** 40).astype(np.int64)
    if fitting:
        np.fill_diagonal(fixed, 0)
    return np.exp(-(fixed.sum(axis=1).astype(np.float64) * 2.0 ** -40))


def entropy_gap(D, fit, perplexity):
    """|H - log(perplexity)| per row, recomputed from beta (nan on degenerate rows)."""
    E = off_diagonal(np.asarray(D)).astype(np.float64) - fit.dmin[:, None]
    with np.errstate(invalid="ignore"):
        a = np.exp(-(fit.beta[:, None] * E))
        z = a.sum(axis=1)
        H = np.log(z) + fit.beta * ((E * a).sum(axis=1) / z)
    return np.where(fit.degenerate, np.nan, np.abs(H - math.log(perplexity)))


def binding_matrix(D, fit):
    """float64 [n, n]: B[i, j] = the probability that fitted row i binds to row j (0 on the diagonal)."""
    D64 = np.asarray(D).astype(np.float64)
    E = D64 - fit.dmin[:, None]
    with np.errstate(invalid="ignore"):
        A = np.where(fit.degenerate[:, None], (E <= 0.0).astype(np.float64), np.exp(-(np.where(fit.degenerate, 0.0, fit.beta)[:, None] * E)))
    np.fill_diagonal(A, 0.0)
    return A / fit.Z[:, None]


def host_distance_matrix(Z, metric="euclidean"):
    """float32 [n, n]: the float64 dissimilarities of the rows of Z rounded: a matrix as ``fit`` hands one to the search."""
    d2 = restate_sq_dists(Z, Z)
    return (np.sqrt(d2) if metric == "euclidean" else d2).astype(np.float32)


# ---- the scalar loops of the definition -------------------------------------------------------------------------------------
def scalar_row(values, perplexity, tol=1e-5, max_iter=200):
    """(beta, dmin, Z, n_iter, degenerate, unconverged) of one row's other entries, one Python float operation at a time."""
    values = [float(v) for v in values]
    dmin = min(values)
    e = [v - dmin for v in values]
    m = sum(1 for v in e if v == 0.0)
    if m >= perplexity:
        return math.inf, dmin, float(m), 0, True, False
    beta, lo, hi, n_iter = 1.0, 0.0, math.inf, 0
    while True:
        a = [math.exp(-(beta * v)) for v in e]
        Z = 0.0
        for v in a:
            Z = Z + v
        S = 0.0
        for v, w in zip(e, a):
            S = S + v * w
        diff = (math.log(Z) + beta * (S / Z)) - math.log(perplexity)
        if abs(diff) <= tol:
            return beta, dmin, Z, n_iter, False, False
        if n_iter >= max_iter:
            return beta, dmin, Z, n_iter, False, True
        if diff > 0.0:
            lo = beta
            beta = 2.0 * beta if hi == math.inf else (beta + hi) / 2.0
        else:
            hi = beta
            beta = (beta + lo) / 2.0
        n_iter += 1


def test_restatement_is_the_scalar_definition_on_a_hand_worked_case():
    """Three rows on a line at 0, 1 and 2 with the outer distance stretched to 3, perplexity 1.5.  The middle row sees two rows
    at distance 1: m = 2 >= 1.5, degenerate, Z = 2, each bound with probability 1/2.  An outer row sees e = (0, 2): with p =
    1 / (1 + exp(-2 beta)) the entropy is the binary entropy of p, so beta solves -(p log p + (1 - p) log(1 - p)) = log 1.5.  Scores
    at fit: an outer row is missed by the middle one (1/2) and by the other outer one (p): p / 2; the middle row is missed by
    both outer rows: (1 - p)^2."""
    D = np.array([[0, 1, 3], [1, 0, 1], [3, 1, 0]], np.float32)
    fit = restate_sos_fit(D, 1.5)
    for i, others in enumerate(([1, 3], [1, 1], [3, 1])):
        beta, dmin, Z, n_iter, degenerate, unconverged = scalar_row(others, 1.5)
        assert (fit.beta[i], fit.dmin[i], fit.n_iter[i], fit.degenerate[i], fit.unconverged[i]) == (beta, dmin, n_iter, degenerate, unconverged)
        assert fit.Z[i] == pytest.approx(Z, rel=1e-15)
    assert list(fit.degenerate) == [False, True, False] and fit.beta[1] == np.inf and fit.Z[1] == 2.0 and not fit.flagged.any()
    assert fit.beta[0] == fit.beta[2] and 0 < fit.n_iter[0] < 40
    p = 1.0 / (1.0 + math.exp(-2.0 * fit.beta[0]))
    assert abs(-(p * math.log(p) + (1 - p) * math.log(1 - p)) - math.log(1.5)) <= 1e-5 + 1e-15
    lo, hi = 0.5, 1.0 - 1e-12  # the root of the binary entropy above p = 1/2, by bisection
    for _ in range(200):
        mid = (lo + hi) / 2
        lo, hi = (mid, hi) if -(mid * math.log(mid) + (1 - mid) * math.log(1 - mid)) > math.log(1.5) else (lo, mid)
    assert abs(p - lo) < 1e-4  # tol 1e-5 on the entropy, whose slope at the root is about 1.4
    scores = restate_sos_scores(D.astype(np.float64), fit.beta, fit.dmin, fit.Z, fitting=True)
    np.testing.assert_allclose(scores, [p / 2, (1 - p) ** 2, p / 2], rtol=1e-11)
    # a new row on top of the middle one: bound by the middle row with 1 / (2 + 1) and by an outer row with 1 / (Z + 1)
    new = restate_sos_scores(np.array([[1.0, 0.0, 1.0]]), fit.beta, fit.dmin, fit.Z, fitting=False)
    assert new[0] == pytest.approx((2.0 / 3.0) * (fit.Z[0] / (fit.Z[0] + 1.0)) ** 2, rel=1e-11)


def test_max_iter_cuts_the_search_off():
    D = host_distance_matrix(shifted_data(65, 5, seed=3).astype(np.float64))
    full = restate_sos_fit(D, 4.5)
    cut = restate_sos_fit(D, 4.5, max_iter=3)
    assert full.n_iter.max() > 3 and not full.unconverged.any()
    late = full.n_iter > 3
    assert late.any() and (cut.unconverged == late).all() and (cut.n_iter[late] == 3).all()
    np.testing.assert_array_equal(cut.beta[~late], full.beta[~late])
    for i in np.flatnonzero(late)[:5]:
        beta, _, Z, n_iter, degenerate, unconverged = scalar_row(off_diagonal(D)[i], 4.5, max_iter=3)
        assert (beta, n_iter, degenerate, unconverged) == (cut.beta[i], 3, False, True) and cut.Z[i] == pytest.approx(Z, rel=1e-14)


# ---- pinned to sklearn ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,d,perplexity", [(65, 17, 4.5), (65, 17, 30.0), (257, 5, 4.5), (3, 2, 1.5)])
def test_conditional_probabilities_are_sklearns(n, d, perplexity):
    """sklearn's t-SNE search on the off-diagonal float32 rows (no shift, its own order of operations, tol 1e-5, 100 steps)
    returns the same conditional probabilities a_ij / Z_i.  Measured here: at most 4e-16."""
    from sklearn.manifold._utils import _binary_search_perplexity
    D = host_distance_matrix(shifted_data(n, d, seed=n + d).astype(np.float64))
    fit = restate_sos_fit(D, perplexity)
    assert not fit.degenerate.any() and not fit.unconverged.any() and fit.n_iter.max() < 100
    want = np.asarray(_binary_search_perplexity(np.ascontiguousarray(off_diagonal(D)), perplexity, 0), np.float64)
    got = off_diagonal(binding_matrix(D, fit))
    print(f"n={n} d={d} perplexity={perplexity}: max difference {np.abs(got - want).max():.3g}, steps {fit.n_iter.min()}..{fit.n_iter.max()}")
    assert np.abs(got - want).max() <= 1e-12


# ---- properties -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("metric", ["euclidean", "sqeuclidean"])
@pytest.mark.parametrize("n,d,perplexity", [(65, 1, 4.5), (65, 17, 30.0), (257, 70, 4.5), (257, 5, 30.0)])
def test_search_meets_the_perplexity_and_binding_rows_sum_to_one(n, d, perplexity, metric):
    D = host_distance_matrix(shifted_data(n, d, seed=n, scale=True).astype(np.float64), metric)
    fit = restate_sos_fit(D, perplexity)
    assert not fit.unconverged.any() and not fit.flagged.any()
    gap = entropy_gap(D, fit, perplexity)
    assert (gap[~fit.degenerate] <= 1e-5).all()
    B = binding_matrix(D, fit)
    np.testing.assert_allclose(B.sum(axis=1), 1.0, rtol=1e-13)
    scores = restate_sos_scores(D.astype(np.float64), fit.beta, fit.dmin, fit.Z, fitting=True)
    want = np.exp(np.log1p(-np.minimum(B, 1.0)).sum(axis=0))  # prod_i (1 - b_ij), the paper's outlier probability (D symmetric here)
    np.testing.assert_allclose(scores, want, rtol=n * 2.0 ** -40)
    assert ((scores >= 0.0) & (scores <= 1.0)).all()


def test_duplicated_rows_take_the_degenerate_rule():
    Z = shifted_data(65, 3, seed=4).astype(np.float64)
    Z[:6] = Z[0]  # six copies: each sees five rows at distance 0, m = 5 >= 4.5
    Z[10:13] = Z[10]  # three copies: m = 2 < 4.5, searched like any row
    D = host_distance_matrix(Z)
    fit = restate_sos_fit(D, 4.5)
    assert fit.degenerate[:6].all()
    assert (fit.beta[:6] == np.inf).all() and (fit.Z[:6] == 5.0).all() and (fit.dmin[:6] == 0.0).all() and (fit.n_iter[:6] == 0).all()
    # a row whose nearest row is one of the copies sees all six at its minimum: degenerate too, with Z = 6
    beside = np.flatnonzero(fit.degenerate[6:]) + 6
    assert (np.argmin(D[beside] + 1e30 * np.eye(65, dtype=np.float32)[beside], axis=1) < 6).all() and (fit.Z[beside] == 6.0).all()
    assert (fit.beta[beside] == np.inf).all() and not fit.degenerate[10:13].any()
    rest = ~fit.degenerate
    assert rest.sum() >= 50 and np.isfinite(fit.beta[rest]).all() and (entropy_gap(D, fit, 4.5)[rest] <= 1e-5).all()
    B = binding_matrix(D, fit)
    np.testing.assert_array_equal(B[:6, :6], (1.0 - np.eye(6)) / 5.0)  # uniform over the tied nearest rows
    assert (B[:6, 6:] == 0.0).all() and (B[beside][:, :6] == 1.0 / 6.0).all()
    np.testing.assert_allclose(B.sum(axis=1), 1.0, rtol=1e-13)
    assert restate_sos_fit(D, 5.0).degenerate[:6].all() and not restate_sos_fit(D, 5.5).degenerate[:6].any()


@pytest.mark.parametrize("n", [3, 65, 257])
def test_an_all_zero_matrix_gives_the_constant_score(n):
    from vgan_amd.outlier import sos_constant_score
    perplexity = 1.5 if n == 3 else 4.5
    fit = restate_sos_fit(np.zeros((n, n), np.float32), perplexity)
    assert fit.degenerate.all() and (fit.Z == n - 1).all()
    scores = restate_sos_scores(np.zeros((n, n)), fit.beta, fit.dmin, fit.Z, fitting=True)
    assert (scores == scores[0]).all()
    assert scores[0] == pytest.approx((1.0 - 1.0 / (n - 1)) ** (n - 1), rel=n * 2.0 ** -40)
    assert np.float32(scores[0]) == pytest.approx(sos_constant_score(n), rel=2.0 ** -22)
    # a new row on top of them all: every fitted row binds to it with 1 / n
    new = restate_sos_scores(np.zeros((1, n)), fit.beta, fit.dmin, fit.Z, fitting=False)
    assert new[0] == pytest.approx((1.0 - 1.0 / n) ** n, rel=n * 2.0 ** -40)


def test_a_far_row_scores_near_one_and_a_row_inside_a_cluster_near_zero():
    rng = np.random.default_rng(11)
    Z = rng.normal(size=(129, 16))
    shell = rng.normal(size=(19, 16))
    Z[1:20] = Z[0] + 1e-2 * shell / np.linalg.norm(shell, axis=1, keepdims=True)  # a dense cluster around row 0, every member's nearest row
    Z[128] = 50.0  # far from everything
    D = host_distance_matrix(Z)
    fit = restate_sos_fit(D, 4.5)
    scores = restate_sos_scores(D.astype(np.float64), fit.beta, fit.dmin, fit.Z, fitting=True)
    print(f"far row {scores[128]:.6f}, centre of the cluster {scores[0]:.3g}, its members {scores[1:20].min():.3g}..{scores[1:20].max():.3g}")
    assert scores[128] > 0.99 and scores[0] < 0.01
    # a new row at the far row's place is bound by it (its nearest row now); one much farther out by nobody
    far = np.sqrt(restate_sq_dists(np.array([[50.0] * 16, [500.0] * 16]), Z))
    new = restate_sos_scores(far, fit.beta, fit.dmin, fit.Z, fitting=False)
    assert new[0] < new[1] and new[1] > 0.99


def test_overflowing_affinities_clamp_to_a_zero_score():
    D = host_distance_matrix(shifted_data(65, 5, seed=6).astype(np.float64))
    fit = restate_sos_fit(D, 4.5)
    d = np.full((1, 65), 1e-6)  # on top of every fitted row's nearest distance: a_i = exp(beta_i (dmin_i - d)) large, finite
    assert restate_sos_scores(d, fit.beta, fit.dmin, fit.Z, fitting=False)[0] < 1e-30
    beta = fit.beta.copy()
    beta[0] = 1e300  # exp overflows: log1p(inf) = inf, clamped at 128
    terms = restate_sos_terms(d, beta, fit.dmin, fit.Z, fitting=False)
    assert terms[0, 0] == 128.0 and np.isfinite(terms).all()
    assert restate_sos_terms(np.zeros((1, 65)), fit.beta, np.zeros(65), np.ones(65), fitting=True).max() == 128.0  # b = 1


def test_planted_outliers_rank_on_top():
    X, rows = planted_data(1025, 64, seed=7)
    D = host_distance_matrix(X.astype(np.float64))
    fit = restate_sos_fit(D, 4.5)
    scores = restate_sos_scores(D.astype(np.float64), fit.beta, fit.dmin, fit.Z, fitting=True)
    assert ranking_rate(scores, rows) > 0.9


# ---- the constructor and the host rules, without a device -------------------------------------------------------------------
def test_constructor_validates_without_touching_the_device():
    import vgan_amd
    from vgan_amd import outlier
    m = _mask(4, [[0, 1], [1, 2, 3]])
    ens = vgan_amd.SubspaceSOS(m, [0.5, 0.5])
    assert (ens.perplexity, ens.metric, ens.tol, ens.max_iter, ens.engine, ens.splits, ens.normalize, ens.combination,
            ens.contamination, ens.storage, ens.keep_distance_matrix) == (4.5, "euclidean", 1e-5, 200, "auto", None, None, "sum", 0.1,
                                                                          "auto", False)
    assert isinstance(ens, outlier._SubspaceScorer)
    for bad in (1, 1.0, 0.5, -3.0, float("inf"), float("nan"), "4.5", None, True):
        with pytest.raises(ValueError, match="perplexity must be"):
            vgan_amd.SubspaceSOS(m, [0.5, 0.5], perplexity=bad)
    for bad in ("cosine", "l2", None, 0):
        with pytest.raises(ValueError, match="metric must be"):
            vgan_amd.SubspaceSOS(m, [0.5, 0.5], metric=bad)
    for bad in (0, -1e-3, float("inf"), float("nan"), "1e-3", None, True):
        with pytest.raises(ValueError, match="tol must be"):
            vgan_amd.SubspaceSOS(m, [0.5, 0.5], tol=bad)
    for bad in (0, -1, 2.5, 2 ** 31, "10", None, True):
        with pytest.raises(ValueError, match="max_iter must be"):
            vgan_amd.SubspaceSOS(m, [0.5, 0.5], max_iter=bad)
    for bad in (0, 65536):
        with pytest.raises(ValueError, match="splits"):
            vgan_amd.SubspaceSOS(m, [0.5, 0.5], splits=bad)
    ok = vgan_amd.SubspaceSOS(m, [0.5, 0.5], perplexity=np.float32(30), metric="sqeuclidean", tol=np.float64(1e-9), max_iter=np.int64(7),
                              splits=3, engine="gram")
    assert (ok.perplexity, ok.metric, ok.tol, ok.max_iter, ok.splits, ok.engine) == (30.0, "sqeuclidean", 1e-9, 7, 3, "gram")
    with pytest.raises(ValueError, match="proba has 3 entries for 2 subspaces"):
        vgan_amd.SubspaceSOS(m, [0.5, 0.25, 0.25])
    with pytest.raises(ValueError, match="normalize"):
        vgan_amd.SubspaceSOS(m, [0.5, 0.5], normalize="l2")
    with pytest.raises(ValueError, match="combination"):
        vgan_amd.SubspaceSOS(m, [0.5, 0.5], combination="mean")
    with pytest.raises(ValueError, match="contamination"):
        vgan_amd.SubspaceSOS(m, [0.5, 0.5], contamination=0.7)
    with pytest.raises(ValueError, match="engine"):
        vgan_amd.SubspaceSOS(m, [0.5, 0.5], engine="fast")
    # fit knows n: the row count first, then perplexity against it
    for rows in (1, 2, outlier.SOS_MAX_ROWS + 1):
        with pytest.raises(ValueError, match="between 3 and 32768"):
            ens.fit(np.zeros((rows, 4), np.float32))
    for rows in (3, 5):  # n - 1 <= 4.5 ... and 5.5 rows would be the first to do
        with pytest.raises(ValueError, match="strictly between 1 and n - 1"):
            ens.fit(np.zeros((rows, 4), np.float32))
    with pytest.raises(ValueError, match="strictly between 1 and n - 1 = 30"):
        vgan_amd.SubspaceSOS(m, [0.5, 0.5], perplexity=30.0).fit(np.zeros((31, 4), np.float32))
    with pytest.raises(ValueError, match="features"):
        ens.fit(np.zeros((9, 3), np.float32))
    assert ens.ops is None  # none of this touched the device
    with pytest.raises(RuntimeError, match="not fitted"):
        ens.decision_function(np.zeros((5, 4), np.float32))
    doc = " ".join(vgan_amd.SubspaceSOS.__doc__.split())
    for word in ("_binary_search_perplexity", "divide beta by 10", "m_i >= perplexity", "beta_i = inf", "2^40", "128", "log1p",
                 "never read", "bitwise symmetric", "bit-identical", "(1 - 1/(n-1))^(n-1)", "keep_distance_matrix", "not built"):
        assert word in doc, word


def test_host_rules():
    from vgan_amd import outlier
    outlier.check_sos_rows(3), outlier.check_sos_rows(1 << 15)
    outlier.check_sos_perplexity(1.5, 3), outlier.check_sos_perplexity(4.5, 7), outlier.check_sos_perplexity(30.0, 32)
    for perplexity, n in ((1.5, 2), (2.0, 3), (4.5, 5), (30.0, 31), (1.0, 100)):
        with pytest.raises(ValueError):
            outlier.check_sos_perplexity(perplexity, n)
    assert outlier.check_sos_params(2, "sqeuclidean", 1, 5) == (2.0, "sqeuclidean", 1.0, 5)
    assert outlier.sos_constant_score(3) == np.float32(0.25) and outlier.sos_constant_score(65).dtype == np.float32
    # chunks: those of the one-class SVM, whose matrices have the same size
    plan = outlier.SubspacePlan(_mask(70, [list(range(40)), [0], [1, 2], list(range(33)), [5]]))
    n = 100
    assert outlier.sos_chunks(plan, n, 1 << 30) == [(0, 3, False), (3, 2, True)]
    assert outlier.sos_chunks(plan, n, 1) == [(z, 1, z >= 3) for z in range(5)]
    two = 2 * (n * n * 4 + n * 5 * 4)
    assert outlier.sos_chunks(plan, n, two) == outlier.ocsvm_chunks(plan, n, two) == [(0, 2, False), (2, 1, False), (3, 1, True), (4, 1, True)]


def test_outlier_ensemble_routes_sos_to_the_new_class():
    import vgan_amd
    model = vgan_amd.VGAN_no_kl(epochs=1)
    model.subspaces = _mask(6, [[0, 1], [2, 3, 5], [4]])
    model.proba = np.array([0.5, 0.3, 0.2])
    ens = model.outlier_ensemble(method="sos")
    assert type(ens) is vgan_amd.SubspaceSOS and ens.perplexity == 4.5 and ens.plan.count == 3
    np.testing.assert_array_equal(ens.proba, model.proba)
    ens = model.outlier_ensemble(method="sos", n_neighbors=17, perplexity=30, metric="sqeuclidean", tol=1e-4, max_iter=50, engine="exact",
                                 splits=2, normalize="zscore", combination="max", contamination=0.05, workspace_bytes=1 << 20)
    assert (ens.perplexity, ens.metric, ens.tol, ens.max_iter, ens.engine, ens.splits, ens.normalize, ens.combination, ens.contamination,
            ens.workspace_bytes) == (30.0, "sqeuclidean", 1e-4, 50, "exact", 2, "zscore", "max", 0.05, 1 << 20)
    with pytest.raises(TypeError):
        model.outlier_ensemble(method="sos", nu=0.5)
    doc = vgan_amd.VGAN_no_kl.outlier_ensemble.__doc__
    assert '"sos"' in doc and "perplexity" in doc and "SubspaceSOS" in vgan_amd.__all__
    with pytest.raises(ValueError, match="method must be 'knn', 'lof' or 'kde'"):  # the neighbour ensemble does not know it
        vgan_amd.SubspaceEnsemble(model.subspaces, model.proba, method="sos")


# ---- C ABI: argument checks without a GPU -----------------------------------------------------------------------------------
def test_sos_entries_reject_bad_arguments_without_gpu():
    import vgan_amd
    from vgan_amd import outlier
    lib = vgan_amd.lib.load()
    header = open(os.path.join(REPO, "include", "vgan_hip.h")).read()
    for name, value in (("MIN_ROWS", outlier.SOS_MIN_ROWS), ("MAX_ROWS", outlier.SOS_MAX_ROWS), ("WAVE_ROWS", outlier.SOS_WAVE_ROWS),
                        ("FLAG_DEGENERATE", outlier._SOS_DEGENERATE), ("FLAG_UNCONVERGED", outlier._SOS_UNCONVERGED)):
        assert int(re.search(rf"#define VGAN_SOS_{name} (\d+)", header).group(1)) == value
    for table, prefix in ((outlier.SOS_METRICS, "METRIC"), (outlier.SOS_STORAGE, "STORAGE")):
        for name, value in table.items():
            assert int(re.search(rf"#define VGAN_SOS_{prefix}_{name.upper()} (\d+)", header).group(1)) == value
    null = None
    buf = ctypes.create_string_buffer(256)
    p = ctypes.cast(ctypes.addressof(buf) + (-ctypes.addressof(buf)) % 16, ctypes.c_void_p)  # never read
    odd = ctypes.c_void_p(p.value + 4)

    def rejected(rc):
        msg = lib.vgan_last_error()
        return rc == 1 and b"bad argument" in msg and b"outlier_sos.hip" in msg

    def each(fn, good, pointers, bad_values):
        for pos in pointers:
            assert rejected(fn(*[null if i == pos else v for i, v in enumerate(good)])), pos
        for pos, bad in bad_values:
            assert rejected(fn(*[bad if i == pos else v for i, v in enumerate(good)])), (pos, bad)

    big = outlier.SOS_MAX_ROWS + 1
    # P, sq, n, feat_off, col_off, first, count, metric, engine, splits, D, stream
    each(lib.vgan_sos_distance_matrix, [p, p, 10, p, p, 0, 2, 0, 1, 1, p, null], (0, 1, 3, 4, 10),
         [(0, odd), (2, 2), (2, 0), (2, big), (5, -1), (6, 0), (6, 65536), (7, 2), (7, -1), (8, 2), (8, -1), (9, 0), (9, 65536)])
    assert rejected(lib.vgan_sos_distance_matrix(null, null, 0, null, null, 0, 0, 0, 0, 0, null, null))
    # D, n, count, perplexity, tol, max_iter, storage, beta, dmin, Z, n_iter, flags, stream
    each(lib.vgan_sos_fit, [p, 10, 2, 4.5, 1e-5, 200, 0, p, p, p, p, p, null], (0, 7, 8, 9, 10, 11),
         [(1, 2), (1, big), (2, 0), (2, 65536), (3, 1.0), (3, 9.0), (3, float("nan")), (3, float("inf")), (4, 0.0), (4, -1.0),
          (4, float("nan")), (4, float("inf")), (5, 0), (6, 3), (6, -1)])
    assert rejected(lib.vgan_sos_fit(p, outlier.SOS_WAVE_ROWS + 1, 2, 4.5, 1e-5, 200, outlier.SOS_STORAGE["wave"], p, p, p, p, p, null))
    # D, n, count, beta, dmin, Z, score, score_row, ld_score, stream
    each(lib.vgan_sos_fit_scores, [p, 10, 2, p, p, p, p, null, 10, null], (0, 3, 4, 5, 6), [(1, 2), (1, big), (2, 0), (2, 65536), (8, 9)])
    # Pq, sq_q, nq, Pr, sq_r, nr, feat_off, col_off, first, count, metric, beta, dmin, Z, engine, splits, acc, score, score_row, ld, stream
    each(lib.vgan_sos_scores, [p, p, 7, p, p, 10, p, p, 0, 2, 0, p, p, p, 1, 1, p, p, null, 7, null], (0, 1, 3, 4, 6, 7, 11, 12, 13, 16, 17),
         [(0, odd), (3, odd), (2, 0), (5, 2), (5, big), (8, -1), (9, 0), (9, 65536), (10, 2), (14, 2), (15, 0), (15, 65536), (19, 6)])
    for name, nargs in (("vgan_sos_distance_matrix", 12), ("vgan_sos_fit", 13), ("vgan_sos_fit_scores", 10), ("vgan_sos_scores", 21)):
        assert len(vgan_amd.lib.SIGNATURES[name][1]) == nargs
    text = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    assert sorted(vgan_amd.lib.SIGNATURES) == sorted(set(re.findall(r"\b(vgan_[a-z0-9_]+)\s*\(", text)))
    assert vgan_amd.lib.ABI_VERSION == lib.vgan_abi_version() == 11  # symbols were only added
