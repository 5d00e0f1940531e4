"""The local correlation integral over the subspaces, CPU tier: the numpy restatement the GPU tests compare against, pinned to a
scalar triple loop of the definition on a hand-worked case and to the identities that hold at every radius; the recipe on which
the detector earns its place (a micro-cluster of more than 32 rows, which LOF with k = 32 scores as inliers); the edge
definitions; and everything of vgan_amd.SubspaceLOCI that runs without a device (argument checks, the host rules, the
dispatch from the model, the C ABI's argument checks).

The definition is SubspaceLOCI's docstring and restate_loci follows it line for line: the float32 matrix with the diagonal
taken as 0, r_max its largest off-diagonal entry, the radii formed in float64 and rounded to float32, every comparison in
float32, the counts and sums as int64, num and den as int64, one float64 division and square root per (row, radius).

Measured here with this file's restatement on micro_cluster(seed), n = 1000, d = 6, defaults, the matrix float32(sqrt) of the
float64 squared distances, seeds 0 to 4: LOCI ROC AUC 0.9985 to 1.0000; sklearn LOF with k = 32 0.366 to 0.411; score > 3 flags
all 50 outliers and 4 to 8 of the 950 inliers (0.4 to 0.8 %); near-ties of the best radius (relative gap below 1e-9, not equal)
on no row."""
import ctypes
import math
import os
import re
from collections import namedtuple

import numpy as np
import pytest

from conftest import REPO
from test_outlier_ecod_cpu import _mask
from test_outlier_ocsvm_cpu import restate_sq_dists

LociFit = namedtuple("LociFit", "r a cnt m S1 S2 num den ratio score best")
LociRows = namedtuple("LociRows", "A M T1 T2 num den ratio score best")
TIE_GAP = 1e-9


# ---- the restatement --------------------------------------------------------------------------------------------------------
def zero_diagonal(D):
    D = np.array(D, dtype=np.float32)
    assert D.ndim == 2 and D.shape[0] == D.shape[1]
    np.fill_diagonal(D, 0.0)
    return D


def off_diagonal_max(D):
    """float32: the largest entry of D off the diagonal."""
    D = np.asarray(D)
    assert D.dtype == np.float32
    return D[~np.eye(D.shape[0], dtype=bool)].max()


def restate_radii(r_max, n_radii, radii_per_octave, alpha):
    """(r, a) float32 [R]: r_j = float32(float64(r_max) exp2(-(R - 1 - j) / radii_per_octave)), a_j = float32(alpha float64(r_j))."""
    r = np.array([np.float32(np.float64(r_max) * np.exp2(-(n_radii - 1 - j) / np.float64(radii_per_octave))) for j in range(n_radii)],
                 dtype=np.float32)
    return r, np.array([np.float32(np.float64(alpha) * np.float64(v)) for v in r], dtype=np.float32)


def within(D, thr):
    """bool [n_c, n_q, R]: D[c][q] <= thr_j, compared in float32."""
    D, thr = np.asarray(D), np.asarray(thr)
    assert D.dtype == np.float32 and thr.dtype == np.float32
    return D[:, :, None] <= thr[None, None, :]


def score_rule(cnt, m, S1, S2, n_min):
    """(num, den int64, ratio float64 with -inf at invalid radii, score float32, best int32) of the rows whose integers are
    given as int64 [rows, R]."""
    cnt, m, S1, S2 = (np.asarray(v, np.int64) for v in (cnt, m, S1, S2))
    num = S1 - cnt * m
    den = m * S2 - S1 * S1
    assert (den >= 0).all()
    valid = (m >= n_min) & (den > 0)
    with np.errstate(divide="ignore", invalid="ignore"):
        ratio = np.where(valid, num.astype(np.float64) / np.sqrt(den.astype(np.float64)), -np.inf)
    top = ratio.max(axis=1)
    score = np.maximum(top, 0.0).astype(np.float32)
    best = np.where(top > 0.0, ratio.argmax(axis=1), -1).astype(np.int32)  # argmax: the lowest index of the maximum
    return num, den, ratio, score, best


def restate_loci(D, n_radii=32, radii_per_octave=4.0, alpha=0.5, n_min=20, radii=None):
    """LociFit of the float32 matrix D (D[c][q]: the distance of subject row q to row c; the diagonal counts as 0); radii: a
    given (r, a) pair instead of the grid under r_max."""
    D = zero_diagonal(D)
    n = D.shape[0]
    r, a = restate_radii(off_diagonal_max(D), n_radii, radii_per_octave, alpha) if radii is None else radii
    cnt = within(D, a).sum(axis=0).astype(np.int64)  # [q, j]
    inside = within(D, r)  # [c, p, j]
    m = inside.sum(axis=0).astype(np.int64)
    S1, S2 = np.empty((n, len(r)), np.int64), np.empty((n, len(r)), np.int64)
    for j in range(len(r)):
        sel = inside[:, :, j].T.astype(np.int64)  # [p, c]
        S1[:, j] = sel @ cnt[:, j]
        S2[:, j] = sel @ (cnt[:, j] * cnt[:, j])
    return LociFit(r, a, cnt, m, S1, S2, *score_rule(cnt, m, S1, S2, n_min))


def restate_new_rows(d, fit, n_min=20):
    """LociRows of new rows at float32 distances d [nq, n] to the fitted rows of `fit`, each appended alone to the fitted set."""
    d = np.asarray(d)
    assert d.dtype == np.float32 and d.shape[1] == fit.cnt.shape[0]
    A = (d[:, :, None] <= fit.a[None, None, :]).sum(axis=1).astype(np.int64)
    inside = d[:, :, None] <= fit.r[None, None, :]  # [q, c, j]
    M = inside.sum(axis=1).astype(np.int64)
    T1 = (inside * fit.cnt[None, :, :]).sum(axis=1)
    T2 = (inside * (fit.cnt * fit.cnt)[None, :, :]).sum(axis=1)
    cnt_x = A + 1
    return LociRows(A, M, T1, T2, *score_rule(cnt_x, M + 1, T1 + cnt_x, T2 + cnt_x * cnt_x, n_min))


def best_is_decided(ratio):
    """bool [rows]: the two largest ratios of the row are equal or differ by more than TIE_GAP relative (or nothing is positive):
    a last-place difference in a division or a square root cannot move the best radius of such a row."""
    if ratio.shape[1] == 1:
        return np.ones(ratio.shape[0], bool)
    top2 = np.sort(ratio, axis=1)[:, -2:]
    lo, hi = top2[:, 0], top2[:, 1]
    with np.errstate(invalid="ignore"):
        return (hi <= 0.0) | (lo == hi) | (hi - lo > TIE_GAP * np.abs(hi))


def scalar_loci(D, r, a, n_min):
    """The definition as plain loops over rows, radii and rows again: (cnt, m, S1, S2, score, best) as Python lists."""
    n, R = len(D), len(r)
    d = [[np.float32(0.0) if c == q else np.float32(D[c][q]) for q in range(n)] for c in range(n)]
    cnt = [[sum(1 for c in range(n) if d[c][q] <= a[j]) for j in range(R)] for q in range(n)]
    m = [[0] * R for _ in range(n)]
    S1 = [[0] * R for _ in range(n)]
    S2 = [[0] * R for _ in range(n)]
    score, best = [0.0] * n, [-1] * n
    for p in range(n):
        for j in range(R):
            for c in range(n):
                if d[c][p] <= r[j]:
                    m[p][j] += 1
                    S1[p][j] += cnt[c][j]
                    S2[p][j] += cnt[c][j] ** 2
            num = S1[p][j] - cnt[p][j] * m[p][j]
            den = m[p][j] * S2[p][j] - S1[p][j] ** 2
            if m[p][j] >= n_min and den > 0 and float(num) / math.sqrt(float(den)) > score[p]:
                score[p], best[p] = float(num) / math.sqrt(float(den)), j
    return cnt, m, S1, S2, [np.float32(v) for v in score], best


# ---- data -------------------------------------------------------------------------------------------------------------------
def micro_cluster(seed, n=1000, m=40, d=6):
    """(X float32 [n, d], labels [n]): n - m - 10 standard normal rows, a cluster of m rows of spread 0.15 around 7 e_0, and 10
    isolated rows at distance 5 to 7 from the origin; the last m + 10 rows are the outliers."""
    rng = np.random.default_rng(seed)
    inliers = rng.normal(0, 1, (n - m - 10, d))
    c = np.zeros(d)
    c[0] = 7.0
    cluster = c + rng.normal(0, 0.15, (m, d))
    v = rng.normal(size=(10, d))
    v /= np.linalg.norm(v, axis=1, keepdims=True)
    isolated = v * rng.uniform(5, 7, (10, 1))
    X = np.vstack([inliers, cluster, isolated]).astype(np.float32)
    y = np.zeros(n, int)
    y[n - m - 10:] = 1
    return X, y


def host_matrix(X):
    """float32 [n, n]: float32(sqrt) of the float64 squared distances."""
    return np.sqrt(restate_sq_dists(X, X)).astype(np.float32)


def roc_auc(y, scores):
    """The rank statistic: the share of (outlier, inlier) pairs the scores order rightly, ties counting a half."""
    y = np.asarray(y, bool)
    values, inverse, counts = np.unique(np.asarray(scores, np.float64), return_inverse=True, return_counts=True)
    ranks = (np.cumsum(counts) - (counts - 1) / 2.0)[inverse]  # average ranks from 1
    n1, n0 = y.sum(), (~y).sum()
    return float((ranks[y].sum() - n1 * (n1 + 1) / 2) / (n1 * n0))


_RECIPE = {}


def recipe_fit(seed):
    if seed not in _RECIPE:
        X, y = micro_cluster(seed)
        _RECIPE[seed] = (X, y, restate_loci(host_matrix(X)))
    return _RECIPE[seed]


# ---- 1. the restatement against the definition --------------------------------------------------------------------------------
def test_restatement_is_the_scalar_definition_on_a_hand_worked_case():
    """Six rows on a line at 0, 1, 2, 3, 10, 11: r_max = 11, two radii an octave apart, r = (5.5, 11), a = (2.75, 5.5).  Within 2.75
    the four rows on the left count 3, 4, 4, 3 rows and the pair on the right 2 each; within 5.5 every row counts its own group;
    within 11 every row reaches all six."""
    x = np.array([0, 1, 2, 3, 10, 11], np.float32)
    D = np.abs(x[:, None] - x[None, :])
    fit = restate_loci(D, n_radii=2, radii_per_octave=1.0, alpha=0.5, n_min=2)
    np.testing.assert_array_equal(fit.r, np.array([5.5, 11.0], np.float32))
    np.testing.assert_array_equal(fit.a, np.array([2.75, 5.5], np.float32))
    np.testing.assert_array_equal(fit.cnt, [[3, 4], [4, 4], [4, 4], [3, 4], [2, 2], [2, 2]])
    np.testing.assert_array_equal(fit.m, [[4, 6], [4, 6], [4, 6], [4, 6], [2, 6], [2, 6]])
    np.testing.assert_array_equal(fit.S1, [[14, 20]] * 4 + [[4, 20]] * 2)  # 3 + 4 + 4 + 3; 2 + 2; 4 x 4 + 2 x 2
    np.testing.assert_array_equal(fit.S2, [[50, 72]] * 4 + [[8, 72]] * 2)  # 9 + 16 + 16 + 9; 4 + 4; 4 x 16 + 2 x 4
    np.testing.assert_array_equal(fit.num, [[2, -4], [-2, -4], [-2, -4], [2, -4], [0, 8], [0, 8]])
    np.testing.assert_array_equal(fit.den, [[4, 32]] * 4 + [[0, 32]] * 2)  # 4 x 50 - 14^2; 2 x 8 - 4^2; 6 x 72 - 20^2
    # the ends of the left group are one count short of their neighbourhood's mean at the small radius (2 / sqrt(4)); the pair
    # on the right has no spread at the small radius (den = 0) and is 8 / sqrt(32) short at the large one
    np.testing.assert_array_equal(fit.score, np.array([1, 0, 0, 1, np.sqrt(2.0), np.sqrt(2.0)], np.float32))
    np.testing.assert_array_equal(fit.best, [0, -1, -1, 0, 1, 1])
    for n_min in (1, 2, 5, 6, 7):
        want = scalar_loci(D, fit.r, fit.a, n_min)
        got = restate_loci(D, n_radii=2, radii_per_octave=1.0, alpha=0.5, n_min=n_min)
        for a, b in zip(want, (got.cnt, got.m, got.S1, got.S2, got.score, got.best)):
            np.testing.assert_array_equal(np.asarray(a), b)
    # n_min = 5 leaves only the large radius, 7 none
    np.testing.assert_array_equal(restate_loci(D, 2, 1.0, 0.5, n_min=5).best, [-1, -1, -1, -1, 1, 1])
    assert (restate_loci(D, 2, 1.0, 0.5, n_min=7).score == 0).all()


@pytest.mark.parametrize("n,d,R,per_octave,alpha,n_min", [(9, 1, 5, 2.0, 0.5, 2), (23, 3, 7, 4.0, 1.0, 3), (17, 2, 1, 4.0, 0.25, 1),
                                                          (31, 5, 33, 8.0, 0.5, 20)])
def test_restatement_is_the_scalar_definition_on_random_cases(n, d, R, per_octave, alpha, n_min):
    X = np.random.default_rng(n).normal(size=(n, d)).astype(np.float32)
    X[n // 2] = X[0]  # a duplicate
    D = host_matrix(X)
    D[1, 2] = np.nextafter(D[1, 2], np.float32(9))  # not bitwise symmetric, and a diagonal that must not be read
    np.fill_diagonal(D, 7.0)
    got = restate_loci(D, R, per_octave, alpha, n_min)
    want = scalar_loci(D, got.r, got.a, n_min)
    for a, b in zip(want, (got.cnt, got.m, got.S1, got.S2, got.score, got.best)):
        np.testing.assert_array_equal(np.asarray(a), b)


def test_restatement_meets_the_radius_free_identities():
    for seed, alpha in ((0, 0.5), (1, 1.0), (2, 0.1)):
        X = np.random.default_rng(seed).normal(size=(120, 4)).astype(np.float32)
        fit = restate_loci(host_matrix(X), alpha=alpha, n_min=5)
        n = len(X)
        assert (fit.den >= 0).all()
        assert (fit.m[:, -1] == n).all()  # the last radius is r_max
        assert (np.diff(fit.cnt, axis=1) >= 0).all() and (np.diff(fit.m, axis=1) >= 0).all() and (np.diff(fit.r) > 0).all()
        assert (fit.cnt <= fit.m).all() and (fit.cnt >= 1).all()  # alpha <= 1; the row itself
        if alpha == 1.0:
            np.testing.assert_array_equal(fit.cnt, fit.m)
        assert (fit.S1 >= fit.m).all() and (fit.S2 >= fit.S1).all()
        # at r_max every row sums over the whole set: one S1, one S2
        assert (fit.S1[:, -1] == fit.cnt[:, -1].sum()).all() and (fit.S2[:, -1] == (fit.cnt[:, -1] ** 2).sum()).all()
        assert fit.r[-1] == off_diagonal_max(host_matrix(X)) and fit.score.dtype == np.float32 and fit.best.dtype == np.int32
        assert ((fit.best == -1) == (fit.score == 0)).all()


def test_host_radii_are_the_restatements():
    from vgan_amd import outlier
    for r_max, R, per_octave, alpha in ((np.float32(11.0), 2, 1.0, 0.5), (np.float32(3.1415927), 32, 4.0, 0.5), (np.float32(1e-3), 64, 8.0, 1.0),
                                        (np.float32(17.25), 1, 4.0, 0.3), (np.float32(0.0), 5, 3.0, 0.5), (np.float32(2.5e4), 33, 2.5, 0.7)):
        r, a = outlier.loci_radii(r_max, R, per_octave, alpha)
        want_r, want_a = restate_radii(r_max, R, per_octave, alpha)
        assert r.dtype == np.float32 and a.dtype == np.float32 and r.shape == (R,)
        np.testing.assert_array_equal(r, want_r)
        np.testing.assert_array_equal(a, want_a)
        assert r[-1] == r_max
    r, a = outlier.loci_radii(np.array([1.0, 2.0, 0.0], np.float32), 4, 1.0, 0.5)
    np.testing.assert_array_equal(r, [[0.125, 0.25, 0.5, 1.0], [0.25, 0.5, 1.0, 2.0], [0, 0, 0, 0]])
    np.testing.assert_array_equal(a, r / 2)


# ---- 2. the recipe ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", range(5))
def test_micro_cluster_is_found_by_loci_and_missed_by_lof(seed):
    from sklearn.neighbors import LocalOutlierFactor
    X, y, fit = recipe_fit(seed)
    assert X.dtype == np.float32 and X.shape == (1000, 6) and y.sum() == 50 and y[-50:].all()
    auc = roc_auc(y, fit.score)
    lof = -LocalOutlierFactor(n_neighbors=32).fit(X.astype(np.float64)).negative_outlier_factor_
    lof_auc = roc_auc(y, lof)
    flagged = fit.score > 3.0
    undecided = int((~best_is_decided(fit.ratio)).sum())
    print(f"seed {seed}: LOCI AUC {auc:.4f}, LOF(32) AUC {lof_auc:.3f}, flagged outliers {flagged[y == 1].sum()} / 50, "
          f"inliers {flagged[y == 0].sum()} / 950, rows with a near-tie of the best radius {undecided}")
    assert auc >= 0.99
    assert lof_auc <= 0.6
    assert flagged[y == 1].all() and flagged[y == 0].mean() <= 0.02
    assert undecided <= 0.01 * len(y)
    assert int(np.abs(fit.den).max()).bit_length() <= 60 and int(np.abs(fit.num).max()).bit_length() <= 60


def test_recipe_barely_moves_with_the_grid():
    X, y, _ = recipe_fit(0)
    D = host_matrix(X)
    for R, per_octave in ((16, 2.0), (64, 8.0)):
        assert roc_auc(y, restate_loci(D, R, per_octave).score) >= 0.99


# ---- 3. edge definitions ------------------------------------------------------------------------------------------------------
def test_constant_matrix_scores_zero():
    fit = restate_loci(np.zeros((9, 9), np.float32), n_radii=4, n_min=1)
    assert (fit.r == 0).all() and (fit.a == 0).all()
    assert (fit.cnt == 9).all() and (fit.m == 9).all() and (fit.num == 0).all() and (fit.den == 0).all()
    assert (fit.score == 0).all() and (fit.best == -1).all()
    new = restate_new_rows(np.zeros((3, 9), np.float32), fit, n_min=1)  # a new copy: cnt_x = 10 against nine rows that count 9
    assert (new.A == 9).all() and (new.num[:, 0] == (9 * 9 + 10) - 10 * 10).all() and (new.score == 0).all() and (new.best == -1).all()


def test_duplicates_count_each_other_at_every_radius():
    x = np.array([0, 0, 0, 1, 1, 5], np.float32)
    D = np.abs(x[:, None] - x[None, :])
    fit = restate_loci(D, n_radii=8, radii_per_octave=1.0, alpha=0.5, n_min=1)
    assert fit.r[0] == np.float32(5.0 / 128) and (fit.cnt[:, 0] == [3, 3, 3, 2, 2, 1]).all()  # nothing but the copies
    np.testing.assert_array_equal(fit.m[:, 0], fit.cnt[:, 0])
    np.testing.assert_array_equal(fit.den[:, 0], 0)  # a neighbourhood of copies has no spread
    np.testing.assert_array_equal(fit.score[:3], fit.score[0])  # copies score alike
    assert fit.score[5] == fit.score.max() > 0


def test_n_min_of_all_rows_leaves_the_radii_that_reach_everyone():
    X = np.random.default_rng(3).normal(size=(40, 2)).astype(np.float32)
    D = host_matrix(X)
    fit = restate_loci(D, n_radii=12, radii_per_octave=2.0, n_min=40)
    full = fit.m == 40
    assert full[:, -1].all() and not full[:, 0].any()
    assert np.isinf(fit.ratio[~full]).all()
    with_all = restate_loci(D, n_radii=12, radii_per_octave=2.0, n_min=1)
    np.testing.assert_array_equal(fit.ratio[full], with_all.ratio[full])


def test_a_single_radius_is_r_max():
    X = np.random.default_rng(4).normal(size=(30, 3)).astype(np.float32)
    D = host_matrix(X)
    fit = restate_loci(D, n_radii=1, n_min=1)
    assert fit.r.shape == (1,) and fit.r[0] == off_diagonal_max(D) and (fit.m == 30).all()
    # one S1 and one S2 for all rows: the score orders the rows by how few rows they count within alpha r_max
    order = np.argsort(fit.cnt[:, 0], kind="stable")
    assert (np.diff(fit.score[order]) <= 0).all() and set(fit.best) <= {0, -1}


def test_new_row_rule_against_the_fit_rule():
    """A new row that copies fitted row p meets the distances of column p (a symmetric matrix), so A, M, T1, T2 are that row's
    fitted cnt, m, S1, S2, and the row then joins the set with one more in each: the score differs from the fitted one."""
    X = np.random.default_rng(5).normal(size=(60, 3)).astype(np.float32)
    D = host_matrix(X)
    D = np.maximum(D, D.T)
    fit = restate_loci(D, n_radii=9, radii_per_octave=2.0, n_min=4)
    new = restate_new_rows(np.ascontiguousarray(zero_diagonal(D).T), fit, n_min=4)
    for a, b in ((new.A, fit.cnt), (new.M, fit.m), (new.T1, fit.S1), (new.T2, fit.S2)):
        np.testing.assert_array_equal(a, b)
    cnt_x = fit.cnt + 1
    np.testing.assert_array_equal(new.num, (fit.S1 + cnt_x) - cnt_x * (fit.m + 1))
    np.testing.assert_array_equal(new.den, (fit.m + 1) * (fit.S2 + cnt_x * cnt_x) - (fit.S1 + cnt_x) ** 2)
    assert (new.score != fit.score).any()
    # a row beyond r_max of every fitted row stands alone at every radius: m = 1, den = 0, score 0 even with n_min = 1
    far = restate_new_rows(np.full((2, 60), np.float32(2.0) * fit.r[-1]), fit, n_min=1)
    assert (far.A == 0).all() and (far.M == 0).all() and (far.den == 0).all() and (far.score == 0).all() and (far.best == -1).all()
    # a row within r_max of everyone and within alpha r of no one at the last radius: counts itself alone against the set
    ring = restate_new_rows(np.full((1, 60), fit.r[-1]), fit, n_min=1)
    assert ring.M[0, -1] == 60 and ring.A[0, -1] == 0 and ring.best[0] == 8
    want = (fit.cnt[:, -1].sum() + 1 - 61) / np.sqrt(float(61 * ((fit.cnt[:, -1] ** 2).sum() + 1) - (fit.cnt[:, -1].sum() + 1) ** 2))
    assert ring.score[0] == np.float32(want)


# ---- 4. the class without a device ------------------------------------------------------------------------------------------
def test_constructor_validation_needs_no_device():
    import vgan_amd
    m = _mask(4, [[0, 1], [2, 3]])
    ens = vgan_amd.SubspaceLOCI(m, [0.5, 0.5])
    assert (ens.alpha, ens.n_min, ens.n_radii, ens.radii_per_octave, ens.k_sigma) == (0.5, 20, 32, 4.0, 3.0)
    assert ens.keep_sums is False and ens.keep_distance_matrix is False and ens.splits is None
    for kw in (dict(alpha=0.0), dict(alpha=1.5), dict(alpha=-0.5), dict(alpha=float("nan")), dict(alpha="half"), dict(n_min=0),
               dict(n_min=2.5), dict(n_min=-3), dict(n_radii=0), dict(n_radii=65), dict(n_radii=8.0), dict(radii_per_octave=0.0),
               dict(radii_per_octave=-1.0), dict(radii_per_octave=float("inf")), dict(radii_per_octave=float("nan")),
               dict(k_sigma=0.0), dict(k_sigma=-3.0), dict(k_sigma=float("nan")), dict(splits=0), dict(splits=65536),
               dict(engine="fast"), dict(normalize="rank"), dict(combination="mean"), dict(contamination=0.7)):
        with pytest.raises(ValueError):
            vgan_amd.SubspaceLOCI(m, [0.5, 0.5], **kw)
    vgan_amd.SubspaceLOCI(m, [0.5, 0.5], alpha=1.0, n_min=1, n_radii=64, radii_per_octave=0.5, k_sigma=0.1)
    for rows in (1, (1 << 15) + 1):
        with pytest.raises(ValueError, match="between 2 and 32768"):
            vgan_amd.SubspaceLOCI(m, [0.5, 0.5], n_min=1).fit(np.zeros((rows, 4), np.float32))
    with pytest.raises(ValueError, match="n_min must not exceed the number of fitted rows 19"):
        ens.fit(np.zeros((19, 4), np.float32))
    with pytest.raises(ValueError, match="features"):
        ens.fit(np.zeros((30, 3), np.float32))
    assert ens.ops is None  # none of this touched the device
    for call in (lambda: ens.decision_function(np.zeros((5, 4), np.float32)), lambda: ens.distance_rows(np.zeros((5, 4), np.float32), 0),
                 lambda: ens.row_sums(np.zeros((5, 4), np.float32), 0)):
        with pytest.raises(RuntimeError, match="not fitted"):
            call()
    doc = " ".join(vgan_amd.SubspaceLOCI.__doc__.split())
    for word in ("Papadimitriou", "pyod", "diagonal as 0", "r_max", "exp2(-(R - 1 - j) / radii_per_octave)", "alpha * float64(r_j)",
                 "S1 - cnt[p, j] m", "m S2 - S1^2", "below 2^60", "m >= n_min and den > 0", "lowest j", "-1 where", "constant features",
                 "appended", "cnt_x = A + 1", "is not ``decision_scores_``", "bit-identical", "keep_sums", "keep_distance_matrix",
                 "Not built", "quad-tree", "2^15"):
        assert word in doc, word


def test_host_rules():
    from vgan_amd import outlier
    assert (outlier.LOCI_MIN_ROWS, outlier.LOCI_MAX_ROWS, outlier.LOCI_MAX_RADII) == (2, 1 << 15, 64)
    outlier.check_loci_rows(2, 1), outlier.check_loci_rows(1 << 15, 20), outlier.check_loci_rows(20, 20)
    for n, n_min in ((1, 1), ((1 << 15) + 1, 20), (19, 20)):
        with pytest.raises(ValueError):
            outlier.check_loci_rows(n, n_min)
    assert outlier.check_loci_params(1, 3, 7, 2, 3) == (1.0, 3, 7, 2.0, 3.0)
    # chunks: those of SOS with the counts and sums of every subspace next to its matrix
    plan = outlier.SubspacePlan(_mask(70, [list(range(40)), [0], [1, 2], list(range(33)), [5]]))
    n, R = 100, 32
    assert outlier.loci_chunks(plan, n, R, 1 << 30) == [(0, 3, False), (3, 2, True)]
    assert outlier.loci_chunks(plan, n, R, 1) == [(z, 1, z >= 3) for z in range(5)]
    two = 2 * (n * n * 4 + 24 * n * R + n * 5 * 4)
    assert outlier.loci_chunks(plan, n, R, two) == [(0, 2, False), (2, 1, False), (3, 1, True), (4, 1, True)]
    assert outlier.loci_chunks(plan, n, R, two - 1) == [(0, 1, False), (1, 1, False), (2, 1, False), (3, 1, True), (4, 1, True)]


def test_outlier_ensemble_routes_loci_to_the_new_class():
    import vgan_amd
    model = vgan_amd.VGAN_no_kl(epochs=1)
    model.subspaces = _mask(6, [[0, 1], [2, 3, 5], [4]])
    model.proba = np.array([0.5, 0.3, 0.2])
    ens = model.outlier_ensemble(method="loci")
    assert type(ens) is vgan_amd.SubspaceLOCI and ens.n_radii == 32 and ens.plan.count == 3
    np.testing.assert_array_equal(ens.proba, model.proba)
    ens = model.outlier_ensemble(method="loci", n_neighbors=17, alpha=0.25, n_min=5, n_radii=16, radii_per_octave=2, k_sigma=2.5,
                                 engine="exact", splits=2, normalize="zscore", combination="max", contamination=0.05,
                                 workspace_bytes=1 << 20)
    assert (ens.alpha, ens.n_min, ens.n_radii, ens.radii_per_octave, ens.k_sigma, ens.engine, ens.splits, ens.normalize, ens.combination,
            ens.contamination, ens.workspace_bytes) == (0.25, 5, 16, 2.0, 2.5, "exact", 2, "zscore", "max", 0.05, 1 << 20)
    with pytest.raises(TypeError):
        model.outlier_ensemble(method="loci", perplexity=4.5)
    doc = vgan_amd.VGAN_no_kl.outlier_ensemble.__doc__
    assert '"loci"' in doc and "n_radii" in doc and "SubspaceLOCI" in vgan_amd.__all__
    with pytest.raises(ValueError, match="method must be 'knn', 'lof' or 'kde'"):  # the neighbour ensemble does not know it
        vgan_amd.SubspaceEnsemble(model.subspaces, model.proba, method="loci")


# ---- C ABI: argument checks without a GPU -----------------------------------------------------------------------------------
def test_loci_entries_reject_bad_arguments_without_gpu():
    import vgan_amd
    from vgan_amd import outlier
    lib = vgan_amd.lib.load()
    header = open(os.path.join(REPO, "include", "vgan_hip.h")).read()
    for name, value in (("MIN_ROWS", outlier.LOCI_MIN_ROWS), ("MAX_ROWS", outlier.LOCI_MAX_ROWS), ("MAX_RADII", outlier.LOCI_MAX_RADII)):
        assert int(re.search(rf"#define VGAN_LOCI_{name} (\d+)", header).group(1)) == value
    null = None
    buf = ctypes.create_string_buffer(256)
    p = ctypes.cast(ctypes.addressof(buf) + (-ctypes.addressof(buf)) % 16, ctypes.c_void_p)  # never read
    odd = ctypes.c_void_p(p.value + 4)

    def rejected(rc):
        msg = lib.vgan_last_error()
        return rc == 1 and b"bad argument" in msg and b"outlier_loci.hip" in msg

    def each(fn, good, pointers, bad_values):
        for pos in pointers:
            assert rejected(fn(*[null if i == pos else v for i, v in enumerate(good)])), pos
        for pos, bad in bad_values:
            assert rejected(fn(*[bad if i == pos else v for i, v in enumerate(good)])), (pos, bad)

    big = outlier.LOCI_MAX_ROWS + 1
    # P, sq, n, feat_off, col_off, first, count, engine, splits, D, stream
    each(lib.vgan_loci_distance_matrix, [p, p, 10, p, p, 0, 2, 1, 1, p, null], (0, 1, 3, 4, 9),
         [(0, odd), (2, 1), (2, 0), (2, big), (5, -1), (6, 0), (6, 65536), (7, 2), (7, -1), (8, 0), (8, 65536)])
    # D, n, count, rmax, stream
    each(lib.vgan_loci_rmax, [p, 10, 2, p, null], (0, 3), [(1, 1), (1, big), (2, 0), (2, 65536)])
    # D, n, count, a, R, cnt, stream
    each(lib.vgan_loci_counts, [p, 10, 2, p, 8, p, null], (0, 3, 5), [(1, 1), (1, 0), (1, big), (2, 0), (2, 65536), (4, 0), (4, 65), (4, -1)])
    assert rejected(lib.vgan_loci_counts(null, 0, 0, null, 0, null, null))
    # D, n, count, r, R, cnt, m, S1, S2, stream
    each(lib.vgan_loci_sums, [p, 10, 2, p, 8, p, p, p, p, null], (0, 3, 5, 6, 7, 8),
         [(1, 1), (1, big), (2, 0), (2, 65536), (4, 0), (4, 65)])
    # cnt, m, S1, S2, n, count, R, n_min, score, score_row, ld_score, best, stream
    each(lib.vgan_loci_finish, [p, p, p, p, 10, 2, 8, 3, p, null, 10, null, null], (0, 1, 2, 3, 8),
         [(4, 1), (4, big), (5, 0), (5, 65536), (6, 0), (6, 65), (7, 0), (7, -2), (10, 9)])
    # Pq, sq_q, nq, Pr, sq_r, nr, feat_off, col_off, first, count, r, a, cnt, R, n_min, engine, splits, acc, dist_out, score, score_row,
    # ld_score, best, stream
    good = [p, p, 7, p, p, 10, p, p, 0, 2, p, p, p, 8, 3, 1, 1, p, null, p, null, 7, null, null]
    each(lib.vgan_loci_scores, good, (0, 1, 3, 4, 6, 7, 10, 11, 12, 17, 19),
         [(0, odd), (3, odd), (2, 0), (5, 1), (5, big), (8, -1), (9, 0), (9, 65536), (13, 0), (13, 65), (14, 0), (15, 2), (15, -1), (16, 0),
          (16, 65536), (21, 6), (18, p)])  # the last: the distances of one subspace only
    for name, nargs in (("vgan_loci_distance_matrix", 11), ("vgan_loci_rmax", 5), ("vgan_loci_counts", 7), ("vgan_loci_sums", 10), ("vgan_loci_finish", 13), ("vgan_loci_scores", 24)):
        assert len(vgan_amd.lib.SIGNATURES[name][1]) == nargs
    text = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    assert sorted(vgan_amd.lib.SIGNATURES) == sorted(set(re.findall(r"\b(vgan_[a-z0-9_]+)\s*\(", text)))
    assert vgan_amd.lib.ABI_VERSION == lib.vgan_abi_version() == 11  # symbols were only added
