"""Mahalanobis / MCD scores over the subspaces, CPU tier: the float64 numpy restatement the GPU tests compare against, pinned
to sklearn (ShrunkCovariance, OAS, EmpiricalCovariance and, where it imports, one private concentration step), to cases
worked by hand, and to the robustness the single-start concentration is documented to have; and everything of
vgan_amd.SubspaceMahalanobis that runs without a device (defaults, argument checks, the support-size and range rules, the
dispatch from the model, the C ABI's argument checks).

The definition (SubspaceMahalanobis's docstring): X as float32, arithmetic in float64.  Over the support H (h rows; every
row when not robust): mu = mean, C = (1 / h) sum (x - mu)(x - mu)^T, Sigma = (1 - alpha) C + alpha (tr C / d) I with alpha given
or sklearn's OAS rule, score = ||L^-1 (x - mu)||^2 with L the lower Cholesky factor of Sigma, rounded to float32.  tr C == 0:
every score 0.  A pivot that is not positive and finite: an error.  robust: from the all-rows estimate, the support becomes
the h rows with the smallest (float32 score, row index) and the estimate is renewed, until the support repeats or
max_csteps renewals have run."""
import ctypes
import os
import re
from fractions import Fraction

import numpy as np
import pytest

from conftest import REPO
from test_outlier_ecod_cpu import _mask

TOL_PIN = 1e-12  # pins the formula to sklearn; not a kernel tolerance


# ---- the restatement --------------------------------------------------------------------------------------------------
class SingularCovariance(ValueError):
    pass


def restate_moments(Z, support=None):
    """(mu [d], C [d, d], h): float64 mean and biased covariance of the rows of Z (float32 values) in the support."""
    Z = np.asarray(Z, dtype=np.float32).astype(np.float64)
    H = Z if support is None else Z[np.asarray(support, dtype=bool)]
    h = H.shape[0]
    mu = H.sum(axis=0) / h
    E = H - mu
    return mu, E.T @ E / h, h


def restate_alpha(C, h, shrinkage):
    """alpha: the float given, or sklearn's OAS rule for "oas"."""
    if shrinkage != "oas":
        return float(shrinkage)
    d = C.shape[0]
    m = np.trace(C) / d
    a = np.mean(C ** 2)
    den = (h + 1.0) * (a - m * m / d)
    return 1.0 if den == 0 else min((a + m * m) / den, 1.0)


def restate_shrunk(C, alpha):
    d = C.shape[0]
    S = (1.0 - alpha) * C
    S.flat[::d + 1] += alpha * np.trace(C) / d
    return S


def restate_cholesky(S):
    """The lower factor by columns; SingularCovariance on a pivot that is not positive and finite (the status rule)."""
    d = S.shape[0]
    L = np.zeros_like(S)
    for j in range(d):
        p = S[j, j] - L[j, :j] @ L[j, :j]
        if not (p > 0.0 and np.isfinite(p)):
            raise SingularCovariance(f"pivot {j} is {float(p)!r}")
        L[j, j] = np.sqrt(p)
        L[j + 1:, j] = (S[j + 1:, j] - L[j + 1:, :j] @ L[j, :j]) / L[j, j]
    return L


def restate_estimate(Z, shrinkage, support=None):
    """dict of mu, C, h, alpha, Sigma and L (None for a subspace that is constant on the support: tr C == 0)."""
    mu, C, h = restate_moments(Z, support)
    alpha = restate_alpha(C, h, shrinkage)
    Sigma = restate_shrunk(C, alpha)
    L = None if np.trace(C) == 0.0 else restate_cholesky(Sigma)
    return dict(mu=mu, C=C, h=h, alpha=alpha, Sigma=Sigma, L=L)


def restate_distances(Z, est):
    """float64 [n]: ||L^-1 (z - mu)||^2, exactly 0 for a constant subspace."""
    from scipy.linalg import solve_triangular
    Z = np.asarray(Z, dtype=np.float32).astype(np.float64)
    if est["L"] is None:
        return np.zeros(Z.shape[0])
    Y = solve_triangular(est["L"], (Z - est["mu"]).T, lower=True)
    return (Y * Y).sum(axis=0)


def support_size(n, d, support_fraction=None):
    if support_fraction is None:
        return min(n, int(np.ceil((n + d + 1) / 2)))
    return int(support_fraction * n)


def select_support(scores32, h):
    """bool [n]: the h rows with the smallest (float32 score, row index)."""
    order = np.lexsort((np.arange(scores32.shape[0]), scores32))
    support = np.zeros(scores32.shape[0], dtype=bool)
    support[order[:h]] = True
    return support


def selection_gap(scores32, h):
    """The relative gap between the h-th and the (h + 1)-th smallest score (inf when h == n)."""
    v = np.sort(scores32.astype(np.float64))
    return np.inf if h >= v.shape[0] else (v[h] - v[h - 1]) / v[h]


def restate_fit(Z, shrinkage=0.1, robust=False, support_fraction=None, max_csteps=30):
    """The whole contract for one subspace Z [n, d_s]: dict of est, scores (float32), and when robust support, n_csteps,
    converged and gaps (selection_gap at every selection)."""
    Z = np.asarray(Z, dtype=np.float32)
    n, d = Z.shape
    est = restate_estimate(Z, shrinkage)
    scores = restate_distances(Z, est).astype(np.float32)
    out = dict(est=est, scores=scores)
    if robust:
        h = support_size(n, d, support_fraction)
        support, steps, converged, gaps = np.ones(n, dtype=bool), 0, False, []
        for _ in range(max_csteps):
            gaps.append(selection_gap(scores, h))
            new = select_support(scores, h)
            if (new == support).all():
                converged = True
                break
            support, steps = new, steps + 1
            est = restate_estimate(Z, shrinkage, support)
            scores = restate_distances(Z, est).astype(np.float32)
        out.update(est=est, scores=scores, support=support, n_csteps=steps, converged=converged, gaps=gaps, h=h)
    return out


def raw_data(n, d, seed, constant=None, duplicate=None):
    """float32 [n, d]: correlated rows with a mean of about 100 and unit spread; column `constant` is constant, column
    duplicate[1] repeats column duplicate[0]."""
    rng = np.random.default_rng(seed)
    A = np.eye(d) + 0.3 * rng.normal(size=(d, d)) / np.sqrt(d)
    X = (100.0 + rng.normal(size=d) + rng.normal(size=(n, d)) @ A).astype(np.float32)
    if constant is not None:
        X[:, constant] = np.float32(101.7)
    if duplicate is not None:
        X[:, duplicate[1]] = X[:, duplicate[0]]
    return X


def planted_shift(n, d, share, seed):
    """(X float32 [n, d], outlier bool [n]): unit Gaussian rows about 100, the first share n rows shifted by +6 in every
    feature."""
    rng = np.random.default_rng(seed)
    X = 100.0 + rng.normal(size=(n, d))
    out = np.zeros(n, dtype=bool)
    out[:int(round(share * n))] = True
    X[out] += 6.0
    return X.astype(np.float32), out


PLANTED = {"257x5": dict(n=257, d=5, share=0.10, seed=3), "1000x20": dict(n=1000, d=20, share=0.20, seed=4)}
MIN_GAP = 2.0 ** -18


def separation_ratio(scores, outlier):
    return float(scores[outlier].min() / scores[~outlier].max())


# ---- pinned to sklearn ---------------------------------------------------------------------------------------------------
PIN_SHAPES = [(300, 7), (1000, 67), (200, 130)]  # the last has n < d_s


@pytest.mark.parametrize("n,d", PIN_SHAPES)
@pytest.mark.parametrize("alpha", [0.1, 0.5])
def test_shrunk_distances_are_sklearns(n, d, alpha):
    from sklearn.covariance import ShrunkCovariance
    X = raw_data(n, d, seed=n + d, constant=2)
    sk = ShrunkCovariance(shrinkage=alpha).fit(X.astype(np.float64))
    est = restate_estimate(X, alpha)
    np.testing.assert_allclose(est["mu"], sk.location_, rtol=TOL_PIN)
    np.testing.assert_allclose(est["Sigma"], sk.covariance_, rtol=TOL_PIN, atol=TOL_PIN * np.abs(sk.covariance_).max())
    np.testing.assert_allclose(restate_distances(X, est), sk.mahalanobis(X.astype(np.float64)), rtol=TOL_PIN)


@pytest.mark.parametrize("n,d", PIN_SHAPES)
def test_oas_shrinkage_and_distances_are_sklearns(n, d):
    from sklearn.covariance import OAS
    X = raw_data(n, d, seed=n + d, constant=2)
    sk = OAS().fit(X.astype(np.float64))
    est = restate_estimate(X, "oas")
    assert 0.0 < est["alpha"] < 1.0
    np.testing.assert_allclose(est["alpha"], sk.shrinkage_, rtol=TOL_PIN)
    np.testing.assert_allclose(restate_distances(X, est), sk.mahalanobis(X.astype(np.float64)), rtol=TOL_PIN)


def test_unshrunk_distances_are_the_empirical_covariances():
    from sklearn.covariance import EmpiricalCovariance
    X = raw_data(300, 7, seed=1)
    sk = EmpiricalCovariance().fit(X.astype(np.float64))
    est = restate_estimate(X, 0.0)
    assert est["alpha"] == 0.0
    np.testing.assert_allclose(est["Sigma"], sk.covariance_, rtol=TOL_PIN, atol=TOL_PIN * np.abs(sk.covariance_).max())
    np.testing.assert_allclose(restate_distances(X, est), sk.mahalanobis(X.astype(np.float64)), rtol=TOL_PIN)


def test_one_concentration_step_is_sklearns():
    """From the same initial estimates, on tie-free data without shrinkage, one C-step selects sklearn's support."""
    c_step = pytest.importorskip("sklearn.covariance._robust_covariance")._c_step  # private: skipped if it moves
    X = raw_data(400, 6, seed=9)
    X64 = X.astype(np.float64)
    est = restate_estimate(X, 0.0)
    h = support_size(400, 6)
    scores = restate_distances(X, est).astype(np.float32)
    assert selection_gap(scores, h) > MIN_GAP
    mine = select_support(scores, h)
    _, _, _, theirs, _ = c_step(X64, h, np.random.RandomState(0), remaining_iterations=0, initial_estimates=(est["mu"], est["C"]))
    assert mine.sum() == theirs.sum() == h == 204
    np.testing.assert_array_equal(mine, theirs)


# ---- worked by hand -------------------------------------------------------------------------------------------------------
def test_one_feature_is_the_squared_z_score():
    x = np.array([1.0, 2.0, 4.0, 9.0, 4.0], dtype=np.float32)
    mu, var = 4.0, (9.0 + 4.0 + 0.0 + 25.0 + 0.0) / 5
    for alpha in (0.0, 0.1, 1.0, "oas"):  # a 1 x 1 matrix is its own shrinkage target
        out = restate_fit(x[:, None], shrinkage=alpha)
        np.testing.assert_allclose(out["scores"], ((x - mu) ** 2 / var).astype(np.float32), rtol=2.0 ** -23)
    assert restate_alpha(np.array([[var]]), 5, "oas") == 1.0  # (h + 1)(a - m^2 / d) == 0


def test_two_features_in_exact_rationals():
    rows = [(0, 0), (2, 0), (0, 2), (2, 4), (1, 4)]
    X = np.array(rows, dtype=np.float32)
    F = [[Fraction(v) for v in r] for r in rows]
    h, alpha = len(rows), Fraction(1, 4)
    mu = [sum(r[k] for r in F) / h for k in range(2)]
    C = [[sum((r[a] - mu[a]) * (r[b] - mu[b]) for r in F) / h for b in range(2)] for a in range(2)]
    m = (C[0][0] + C[1][1]) / 2
    S = [[(1 - alpha) * C[a][b] + (alpha * m if a == b else 0) for b in range(2)] for a in range(2)]
    det = S[0][0] * S[1][1] - S[0][1] * S[1][0]
    want = []
    for r in F:
        z = [r[0] - mu[0], r[1] - mu[1]]
        want.append((z[0] * z[0] * S[1][1] - 2 * z[0] * z[1] * S[0][1] + z[1] * z[1] * S[0][0]) / det)
    assert C[0][0] == Fraction(4, 5) and C[0][1] == Fraction(2, 5) and C[1][1] == Fraction(16, 5)
    est = restate_estimate(X, 0.25)
    np.testing.assert_allclose(est["Sigma"], np.array([[float(v) for v in r] for r in S]), rtol=1e-15)
    np.testing.assert_allclose(restate_distances(X, est), [float(v) for v in want], rtol=1e-14)


def test_a_constant_subspace_scores_exactly_zero():
    X = np.full((9, 3), 2.5, dtype=np.float32)
    X[:, 1] = 101.7
    for alpha in (0.0, 0.1, "oas"):
        out = restate_fit(X, shrinkage=alpha)
        assert out["est"]["L"] is None and (out["scores"] == 0).all() and out["scores"].dtype == np.float32
    assert restate_alpha(np.zeros((3, 3)), 9, "oas") == 1.0


def test_a_duplicated_feature_without_shrinkage_raises():
    """The two columns hold 99 and 101 equally often: the mean is 100, C is all ones, every operation is exact and the
    second pivot is exactly 0."""
    x = np.where(np.arange(20) % 2 == 0, 99.0, 101.0).astype(np.float32)
    X = np.stack([x, x], axis=1)
    with pytest.raises(SingularCovariance, match="pivot 1 is 0.0"):
        restate_fit(X, shrinkage=0.0)
    out = restate_fit(X, shrinkage=0.1)  # Sigma = [[1, 0.9], [0.9, 1]]
    np.testing.assert_allclose(out["scores"], np.full(20, 1.0 / 0.95, dtype=np.float32), rtol=2.0 ** -23)


# ---- robustness of the single-start concentration --------------------------------------------------------------------------
@pytest.mark.parametrize("case", sorted(PLANTED))
def test_concentration_separates_planted_outliers_where_the_classical_estimate_does_not(case):
    cfg = PLANTED[case]
    X, outlier = planted_shift(cfg["n"], cfg["d"], cfg["share"], cfg["seed"])
    robust = restate_fit(X, robust=True)
    classical = restate_fit(X)
    print(case, "robust", separation_ratio(robust["scores"], outlier), "classical", separation_ratio(classical["scores"], outlier),
          "steps", robust["n_csteps"], "gaps", robust["gaps"])
    assert robust["converged"] and 1 <= robust["n_csteps"] <= 10
    assert min(robust["gaps"]) > MIN_GAP  # the GPU test relies on it: no selection hinges on the last bit of a score
    assert robust["support"].sum() == robust["h"] == support_size(cfg["n"], cfg["d"])
    assert not (robust["support"] & outlier).any()
    assert separation_ratio(robust["scores"], outlier) > 1.0
    assert separation_ratio(classical["scores"], outlier) < 1.0


def test_the_documented_breakdown_under_heavy_clustered_contamination():
    X, outlier = planted_shift(1000, 67, 0.30, 5)
    robust = restate_fit(X, robust=True)
    assert robust["converged"] and robust["h"] == 534
    assert min(robust["gaps"]) > MIN_GAP  # no selection hinges on the last bits of a score, so the count below is stable
    assert (robust["support"] & outlier).sum() == 124  # the figure of the class docstring
    assert separation_ratio(robust["scores"], outlier) < 1.0


def test_ties_go_to_the_lower_row_and_max_csteps_bounds_the_loop():
    scores = np.array([3, 1, 2, 1, 2, 2, 0], dtype=np.float32)
    np.testing.assert_array_equal(np.flatnonzero(select_support(scores, 4)), [1, 2, 3, 6])
    np.testing.assert_array_equal(np.flatnonzero(select_support(scores, 5)), [1, 2, 3, 4, 6])
    X, _ = planted_shift(257, 5, 0.10, 3)
    full = restate_fit(X, robust=True)
    cut = restate_fit(X, robust=True, max_csteps=1)
    assert full["n_csteps"] > 1 and cut["n_csteps"] == 1 and not cut["converged"]
    np.testing.assert_array_equal(cut["scores"], restate_distances(X, cut["est"]).astype(np.float32))  # under the last estimate
    whole = restate_fit(X, robust=True, support_fraction=1.0)  # h == n: the first selection repeats the start
    assert whole["converged"] and whole["n_csteps"] == 0
    np.testing.assert_array_equal(whole["scores"], restate_fit(X)["scores"])


# ---- host logic of the class -------------------------------------------------------------------------------------------------
def test_constructor_and_argument_errors_touch_no_device():
    import vgan_amd
    from vgan_amd import outlier
    m = _mask(4, [[0, 1], [2, 3]])
    ens = vgan_amd.SubspaceMahalanobis(m, [0.5, 0.5])
    assert (ens.shrinkage, ens.robust, ens.support_fraction, ens.max_csteps) == (0.1, False, None, 30)
    assert ens.ops is None and ens.workspace_bytes == outlier.DEFAULT_WORKSPACE_BYTES
    assert (ens.normalize, ens.combination, ens.contamination) == (None, "sum", 0.1)
    assert list(ens.plan.order) == [0, 1]  # the given order
    for name in ("n_neighbors", "engine", "splits", "bandwidth"):
        assert not hasattr(ens, name)
        with pytest.raises(TypeError):
            vgan_amd.SubspaceMahalanobis(m, [0.5, 0.5], **{name: 1})
    for bad in (-0.1, 1.5, float("nan"), "lw", None, True):
        with pytest.raises(ValueError, match="shrinkage"):
            vgan_amd.SubspaceMahalanobis(m, [0.5, 0.5], shrinkage=bad)
    for bad in (0.0, -0.5, 1.5, float("nan"), "half", True):
        with pytest.raises(ValueError, match="support_fraction"):
            vgan_amd.SubspaceMahalanobis(m, [0.5, 0.5], robust=True, support_fraction=bad)
    for bad in (0, -1, 2.0, None, True):
        with pytest.raises(ValueError, match="max_csteps"):
            vgan_amd.SubspaceMahalanobis(m, [0.5, 0.5], max_csteps=bad)
    ok = vgan_amd.SubspaceMahalanobis(m, [0.5, 0.5], shrinkage="oas", robust=True, support_fraction=0.75, max_csteps=1)
    assert (ok.shrinkage, ok.robust, ok.support_fraction, ok.max_csteps) == ("oas", True, 0.75, 1)
    assert vgan_amd.SubspaceMahalanobis(m, [0.5, 0.5], shrinkage=0).shrinkage == 0.0
    assert vgan_amd.SubspaceMahalanobis(m, [0.5, 0.5], shrinkage=1).shrinkage == 1.0
    with pytest.raises(ValueError, match="proba has 3 entries for 2 subspaces"):
        vgan_amd.SubspaceMahalanobis(m, [0.5, 0.25, 0.25])
    with pytest.raises(ValueError, match="normalize"):
        vgan_amd.SubspaceMahalanobis(m, [0.5, 0.5], normalize="l2")
    with pytest.raises(ValueError, match="combination"):
        vgan_amd.SubspaceMahalanobis(m, [0.5, 0.5], combination="mean")
    with pytest.raises(ValueError, match="contamination"):
        vgan_amd.SubspaceMahalanobis(m, [0.5, 0.5], contamination=0.7)
    with pytest.raises(ValueError, match="at most 1024"):
        vgan_amd.SubspaceMahalanobis(np.ones((1, outlier.MAHA_MAX_DIMS + 1), bool), [1.0])
    vgan_amd.SubspaceMahalanobis(np.ones((1, outlier.MAHA_MAX_DIMS), bool), [1.0])
    with pytest.raises(ValueError, match="between 2 and"):
        ens.fit(np.zeros((1, 4), np.float32))
    with pytest.raises(ValueError, match="features"):
        ens.fit(np.zeros((5, 3), np.float32))

    class Tall:  # only its shape is looked at before the row check raises
        shape = ((1 << 24) + 1, 4)

    with pytest.raises(ValueError, match="between 2 and"):
        ens.fit(Tall())
    few = vgan_amd.SubspaceMahalanobis(m, [0.5, 0.5], robust=True, support_fraction=0.3)
    with pytest.raises(ValueError, match="support_fraction"):
        few.fit(np.zeros((6, 4), np.float32))  # int(0.3 * 6) = 1 row
    assert ens.ops is None and few.ops is None  # none of this touched the device
    for attr in ("location_", "covariance_", "shrinkage_"):
        with pytest.raises(RuntimeError, match="not fitted"):
            getattr(ens, attr)
    with pytest.raises(AttributeError, match="robust=True"):
        ens.support_
    with pytest.raises(RuntimeError, match="not fitted"):
        ens.decision_function(np.zeros((5, 4), np.float32))
    doc = vgan_amd.SubspaceMahalanobis.__doc__
    for word in ("FastMCD", "consistency correction", "reweighting", "Ledoit-Wolf", "max_csteps", "124 outliers", "normalize"):
        assert word in doc, word


def test_support_size_and_ranges_follow_the_documented_rules():
    from vgan_amd.outlier import MAHA_TILE, maha_ranges, maha_tiles, mcd_support_size
    for n, d in ((257, 5), (1000, 20), (10, 3), (4, 7), (2, 1), (200, 130)):
        assert mcd_support_size(n, d) == support_size(n, d) == min(n, (n + d + 2) // 2)
    assert mcd_support_size(257, 5) == 132 and mcd_support_size(4, 7) == 4
    assert mcd_support_size(100, 5, 0.75) == 75 and mcd_support_size(100, 5, 1.0) == 100 and mcd_support_size(7, 5, 0.3) == 2
    with pytest.raises(ValueError, match="at least 2"):
        mcd_support_size(6, 5, 0.3)
    # 8 bytes a feature of a range; never below one subspace or one tile
    assert maha_ranges([3, 5, 2], 1 << 30) == ((1 << 30) // 8, [(0, 3)])
    assert maha_ranges([300, 500, 200], 8 * 800) == (800, [(0, 2), (2, 1)])
    assert maha_ranges([300, 500, 200], 0) == (500, [(0, 1), (1, 1), (2, 1)])
    assert maha_ranges([3, 5, 2], 0) == (MAHA_TILE * MAHA_TILE, [(0, 3)])
    assert maha_ranges([1] * 70000, 1 << 30)[1] == [(0, 65535), (65535, 4465)]
    tiles = maha_tiles([3, 40, 16], 1, 2)
    assert tiles.dtype == np.int32
    np.testing.assert_array_equal(tiles, [[1, 0, 0], [1, 1, 0], [1, 1, 1], [1, 2, 0], [1, 2, 1], [1, 2, 2], [2, 0, 0]])


def test_outlier_ensemble_routes_mahalanobis_and_mcd_to_the_new_class():
    import vgan_amd
    model = vgan_amd.VGAN_no_kl(epochs=1)
    model.subspaces = _mask(6, [[0, 1], [2, 3, 5], [4]])
    model.proba = np.array([0.5, 0.3, 0.2])
    ens = model.outlier_ensemble(method="mahalanobis")
    assert type(ens) is vgan_amd.SubspaceMahalanobis and not ens.robust and ens.shrinkage == 0.1 and ens.plan.count == 3
    np.testing.assert_array_equal(ens.proba, model.proba)
    ens = model.outlier_ensemble(method="mcd", n_neighbors=17, shrinkage="oas", support_fraction=0.8, max_csteps=5, normalize="zscore",
                                 combination="max", contamination=0.05, workspace_bytes=1 << 20)  # n_neighbors is ignored
    assert type(ens) is vgan_amd.SubspaceMahalanobis and ens.robust
    assert (ens.shrinkage, ens.support_fraction, ens.max_csteps, ens.normalize, ens.combination, ens.contamination,
            ens.workspace_bytes) == ("oas", 0.8, 5, "zscore", "max", 0.05, 1 << 20)
    with pytest.raises(TypeError):
        model.outlier_ensemble(method="mahalanobis", engine="exact")  # not a keyword of SubspaceMahalanobis
    with pytest.raises(TypeError):
        model.outlier_ensemble(method="mcd", robust=True)  # "mcd" sets it
    doc = vgan_amd.VGAN_no_kl.outlier_ensemble.__doc__
    assert "mahalanobis" in doc and "mcd" in doc
    assert "SubspaceMahalanobis" in vgan_amd.__all__
    for method in ("mahalanobis", "mcd"):
        with pytest.raises(ValueError, match="method"):  # the neighbour ensemble still does not know them
            vgan_amd.SubspaceEnsemble(model.subspaces, model.proba, method=method)


# ---- C ABI: argument checks without a GPU -----------------------------------------------------------------------------------
def test_maha_entries_reject_bad_arguments_without_gpu():
    import vgan_amd
    from vgan_amd import outlier
    lib = vgan_amd.lib.load()
    header = open(os.path.join(REPO, "include", "vgan_hip.h")).read()
    assert int(re.search(r"#define VGAN_MAHA_MAX_DIMS (\d+)", header).group(1)) == outlier.MAHA_MAX_DIMS >= 1024
    assert int(re.search(r"#define VGAN_MAHA_MAX_ROWS (\d+)", header).group(1)) == outlier.MAHA_MAX_ROWS == 1 << 24
    assert int(re.search(r"#define VGAN_MAHA_SLAB_ROWS (\d+)", header).group(1)) == outlier.MAHA_SLAB_ROWS
    null = None
    buf = ctypes.create_string_buffer(256)
    p = ctypes.cast(ctypes.addressof(buf) + (-ctypes.addressof(buf)) % 16, ctypes.c_void_p)  # never read

    def rejected(rc):
        msg = lib.vgan_last_error()
        return rc == 1 and b"bad argument" in msg and b"outlier_maha.hip" in msg

    def each(fn, good, pointers, bad_values):
        for pos in pointers:
            assert rejected(fn(*[null if i == pos else v for i, v in enumerate(good)])), pos
        for pos, bad in bad_values:
            assert rejected(fn(*[bad if i == pos else v for i, v in enumerate(good)])), (pos, bad)

    big = outlier.MAHA_MAX_DIMS + 1
    # X, ldx, n, d, feat, feat_off, sq_off, first, count, total_dims, max_dims, tiles, n_tiles, support, ld_support, hcount, mean,
    # cov, workspace, workspace_bytes, stream
    each(lib.vgan_maha_moments, [p, 4, 100, 4, p, p, p, 0, 2, 5, 3, p, 2, p, 100, p, p, p, p, 4096, null], (0, 4, 5, 6, 11, 15, 16, 17, 18),
         [(1, 3), (2, 1), (2, (1 << 24) + 1), (3, 0), (7, -1), (8, 0), (8, 65536), (9, 1), (9, 7), (10, 0), (10, big), (12, 1), (14, 99),
          (19, 39), (19, 2047)])
    # cov, sq_off, feat_off, first, count, max_dims, hcount, shrinkage, L, W, alpha, status, stream
    each(lib.vgan_maha_factor, [p, p, p, 0, 2, 3, p, 0.1, p, p, p, p, null], (0, 1, 2, 6, 8, 9, 10, 11),
         [(3, -1), (4, 0), (4, 65536), (5, 0), (5, big), (7, -0.5), (7, 1.5), (7, float("nan"))])
    # Xq, ldq, rows, d, feat, feat_off, sq_off, first, count, max_dims, mean, W, score, ld_score, stream
    each(lib.vgan_maha_scores, [p, 4, 10, 4, p, p, p, 0, 2, 3, p, p, p, 10, null], (0, 4, 5, 6, 10, 11, 12),
         [(1, 3), (2, 0), (2, (1 << 24) + 1), (3, 0), (7, -1), (8, 0), (8, 65536), (9, 0), (9, big), (13, 9)])
    # score, ld_score, n, first, count, hcount, support, ld_support, changed, stream
    each(lib.vgan_maha_select, [p, 10, 10, 0, 2, p, p, 10, p, null], (0, 5, 6, 8),
         [(1, 9), (2, 0), (2, (1 << 24) + 1), (3, -1), (4, 0), (4, 65536), (7, 9)])
    for name, nargs in (("vgan_maha_moments", 21), ("vgan_maha_factor", 13), ("vgan_maha_scores", 15), ("vgan_maha_select", 10)):
        assert len(vgan_amd.lib.SIGNATURES[name][1]) == nargs
    assert vgan_amd.lib.ABI_VERSION == lib.vgan_abi_version() == 11  # symbols were only added
