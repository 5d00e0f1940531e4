"""PCA scores over the subspaces on the MI355X (csrc/outlier_pca.hip through vgan_amd.SubspacePCA), against the float64
restatement of test_outlier_pca_cpu.py (pinned there to sklearn), never a second run of the code under test.

Bars, with u = 2^-53.  Decomposition, against M recomputed on the host: max |V V^T - I| <= 32 d_s u, max |V^T Lambda V - M| <= 16
d_s u ||M||_2, |lambda - eigvalsh(M)| <= 16 d_s u ||M||_2; the constants come from the CPU restatement of the Jacobi order built
(that file's docstring: 3.51, 1.58 and 0.56 observed there; the first is above 2.5, hence 8 x 3.51 rounded up to 32, the other
two keep the 16); scale_ within 2 u relative of the root of the device's own variance (its test says why not of the
host's).  Scores given the device's own eigenpairs: |got - want| <= 2^-23 |want| + 4 d_s u sum_j w_j |y_j| sum_k |v_jk
z_k|, the final rounding plus the summation bound with a factor 4.  End to end against the eigh restatement at q = 1: |got -
want| <= 2^-23 |want| + w_max ||z||^2 E (w_max + 2 / gap) with E = 16 d_s u ||M||_2 and gap = lambda_1 - lambda_2, every case asserting E
(w_max + 2 / gap) < 2^-24 on its input first.  Identity claims are compared bit for bit."""
import numpy as np
import pytest

from test_outlier_maha_cpu import restate_fit as restate_maha_fit
from test_outlier_maha_gpu import assert_one_ulp, assert_well_conditioned
from test_outlier_norm_gpu import _check_scores, _check_stats
from test_outlier_pca_cpu import (CONST, DUP, K_EIGENVALUE, K_ORTHOGONAL, K_RESIDUAL, LDS_DIMS, ROWS, SIZES, U, component_count, edge_data,
                                  edge_mask, planted_plane, planted_ranks, restate_fit, restate_matrix, restate_scores, restate_weights,
                                  sign_rule_holds)

pytestmark = pytest.mark.gpu

MASK = edge_mask()
PROBA = np.arange(1, len(SIZES) + 1) / np.arange(1, len(SIZES) + 1).sum()
# components, n_components, weighted, standardize
SETTINGS = [("all", None, True, True), ("all", None, False, False), ("all", None, True, False), ("major", 1, True, True),
            ("major", 1, False, False), ("minor", 1, True, False), ("minor", 1, False, True), ("major", 0.9, True, True),
            ("minor", 0.9, False, False)]


def features(mask, s):
    return np.flatnonzero(mask[s])


@pytest.fixture(scope="module")
def data():
    return {n: edge_data(n) for n in ROWS}


@pytest.fixture(scope="module")
def fitted(data):
    """(n, components, n_components, weighted, standardize) -> the ensemble over MASK fitted on data[n], once for the module."""
    import vgan_amd
    cache = {}

    def get(n, components="all", n_components=None, weighted=True, standardize=True):
        key = (n, components, n_components, weighted, standardize)
        if key not in cache:
            cache[key] = vgan_amd.SubspacePCA(MASK, PROBA, n_components=n_components, components=components, weighted=weighted,
                                              standardize=standardize).fit(data[n])
        return cache[key]
    return get


def test_the_mask_crosses_the_lds_limit():
    from vgan_amd.outlier import PCA_LDS_DIMS
    assert PCA_LDS_DIMS == LDS_DIMS and LDS_DIMS in SIZES and LDS_DIMS + 1 in SIZES
    assert SIZES[:3] == [1, 2, 3] and MASK[0, CONST] and MASK[2, list(DUP)].all()


# ---- 1. the decomposition -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("standardize", [True, False])
@pytest.mark.parametrize("n", ROWS)
def test_eigenpairs_decompose_the_hosts_matrix(data, fitted, n, standardize):
    X, ens = data[n], fitted(n, standardize=standardize)
    assert (ens.n_sweeps_ >= 1).all() and ens.converged_.all() and ens.converged_.dtype == bool
    np.testing.assert_array_equal(ens.n_components_, SIZES)
    for s, d in enumerate(SIZES):
        Z = X[:, features(MASK, s)]
        _, scale, M = restate_matrix(Z, standardize)
        lam, Vt = ens.explained_variance_[s], ens.components_[s]
        assert lam.shape == (d,) and Vt.shape == (d, d) and lam.dtype == Vt.dtype == np.float64
        norm = np.linalg.norm(M, 2)
        orth = np.abs(Vt @ Vt.T - np.eye(d)).max()
        resid = np.abs(Vt.T @ (lam[:, None] * Vt) - M).max()
        eig = np.abs(lam - np.linalg.eigvalsh(M)[::-1]).max()
        print(f"n={n} std={standardize} d={d}: orth {orth / (d * U):.2f} resid {resid / (d * U * max(norm, 1e-300)):.2f} "
              f"eig {eig / (d * U * max(norm, 1e-300)):.2f} scale {np.abs(ens.scale_[s] - scale).max() / U:.2f} u sweeps {ens.n_sweeps_[s]}")
        assert orth <= K_ORTHOGONAL * d * U, (s, orth / (d * U))
        assert resid <= K_RESIDUAL * d * U * norm, (s, resid)
        assert eig <= K_EIGENVALUE * d * U * norm, (s, eig)
        assert (np.diff(lam) <= 0).all() and sign_rule_holds(Vt), s
        assert (np.abs(ens.scale_[s] - scale) <= (2 * n + 1) * U * scale).all(), s  # the moments' own bar, see below
        np.testing.assert_allclose(ens.location_[s], Z.astype(np.float64).mean(axis=0), rtol=1e-13)
        ratio = ens.explained_variance_ratio_[s]
        assert (ratio >= 0).all() and (norm == 0 or abs(ratio.sum() - 1) < 1e-14)


@pytest.mark.parametrize("n", ROWS)
def test_scale_is_the_root_of_the_devices_own_variance(data, fitted, n):
    """scale_ within 2 u relative of sqrt(C_kk), C as vgan_maha_moments left it on the device (an exact 0 becomes 1), and 1 when
    not standardising.  Against the variance recomputed from X the 2 u cannot hold and is not what is asserted: C_kk is a
    float64 sum of n squares in the moments' fixed order, which the Mahalanobis tests bar at 4 n u C_kk, so scale inherits up
    to 2 n u (asserted in the test above); observed against a long-double variance at n = 65, 257, 2051: up to 2.004 u, two
    ulps of a value just below 1."""
    import vgan_amd
    X = data[n]
    ens = vgan_amd.SubspacePCA(MASK, PROBA)
    Xd = ens._begin_fit(X)
    ens._prepare(n, Xd.device)
    ens._moments(Xd)
    cov, sq, off = ens._cov.cpu().numpy(), ens._sq_off, ens.plan.feat_off
    ens._eigen()
    got = ens._scale.cpu().numpy()
    for s, d in enumerate(SIZES):
        want = np.sqrt(np.diag(cov[sq[s]:sq[s + 1]].reshape(d, d)))
        want[want == 0] = 1.0
        assert (np.abs(got[off[s]:off[s + 1]] - want) <= 2 * U * want).all(), s
        np.testing.assert_array_equal(got[off[s]:off[s + 1]], fitted(n).scale_[s])  # fit publishes the same bits
        assert (fitted(n, standardize=False).scale_[s] == 1).all()
    assert got[off[0]] == 1 and got[off[1]] == 1  # the constant column, alone and in company


# ---- 2. the scores given the device's own eigenpairs ------------------------------------------------------------------------
@pytest.mark.parametrize("setting", SETTINGS, ids=lambda v: "-".join(str(x) for x in v))
@pytest.mark.parametrize("n", ROWS)
def test_scores_follow_from_the_devices_eigenpairs(data, fitted, n, setting):
    components, n_components, weighted, standardize = setting
    X, ens = data[n], fitted(n, *setting)
    batches = [(X, ens.per_subspace_scores_)]
    for rows in (63, 65):
        Y = data[65][:rows] + np.float32(0.25)
        batches.append((Y, ens.decision_function(Y, return_per_subspace=True)[1]))
    assert ens.per_subspace_scores_.shape == (len(SIZES), n) and ens.per_subspace_scores_.dtype == np.float32
    for s, d in enumerate(SIZES):
        lam, Vt = ens.explained_variance_[s], ens.components_[s]
        q = component_count(lam, n_components)
        assert q == ens.n_components_[s]
        wt = restate_weights(lam, q, components, weighted, 0.1)
        for Y, per in batches:
            want, term = restate_scores(Y[:, features(MASK, s)], ens.location_[s], ens.scale_[s], Vt, wt)
            err = np.abs(per[s].astype(np.float64) - want)
            assert (err <= 2.0 ** -23 * np.abs(want) + 4 * d * U * term).all(), (s, float(err.max()))
            assert (per[s][want == 0] == 0).all()
    assert (ens.per_subspace_scores_[0] == 0).all()  # the constant subspace


# ---- 3. end to end ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("standardize", [True, False])
@pytest.mark.parametrize("weighted", [True, False])
@pytest.mark.parametrize("components", ["major", "minor"])
@pytest.mark.parametrize("n", [257, 2051])
def test_scores_at_one_component_meet_the_eigh_restatement(data, fitted, n, components, weighted, standardize):
    X, ens = data[n], fitted(n, components, 1, weighted, standardize)
    worst = 0.0
    for s, d in enumerate(SIZES):
        Z = X[:, features(MASK, s)]
        want = restate_fit(Z, n_components=1, components=components, weighted=weighted, standardize=standardize)
        got = ens.per_subspace_scores_[s].astype(np.float64)
        w_max = want["wt"].max()
        if w_max == 0:
            assert (got == 0).all() and (want["scores"] == 0).all()
            continue
        E = 16 * d * U * np.linalg.norm(want["M"], 2)
        gap = want["lam"][0] - want["lam"][1] if d > 1 else np.inf
        factor = E * (w_max + 2.0 / gap)
        worst = max(worst, factor)
        assert factor < 2.0 ** -24, (s, factor)
        z = (Z.astype(np.float64) - want["mu"]) / want["scale"]
        bound = 2.0 ** -23 * np.abs(want["scores"]) + w_max * (z * z).sum(axis=1) * factor
        err = np.abs(got - want["scores"])
        assert (err <= bound).all(), (s, float((err / np.maximum(bound, 1e-300)).max()))
    print(f"n={n} {components} weighted={weighted} std={standardize}: worst E (w_max + 2 / gap) = 2^{np.log2(worst):.1f}")


@pytest.mark.parametrize("n", [257, 2051])
def test_all_components_unstandardised_is_the_mahalanobis_score(data, fitted, n):
    X, ens = data[n], fitted(n, standardize=False)
    for s in range(len(SIZES)):
        want = restate_maha_fit(X[:, features(MASK, s)])
        assert_well_conditioned(want["est"])
        assert_one_ulp(ens.per_subspace_scores_[s], want["scores"])


# ---- 4. exactness and identity ----------------------------------------------------------------------------------------------
def _same(a, b):
    np.testing.assert_array_equal(a.per_subspace_scores_, b.per_subspace_scores_)
    np.testing.assert_array_equal(a.decision_scores_, b.decision_scores_)
    for name in ("n_sweeps_", "converged_", "n_components_"):
        np.testing.assert_array_equal(getattr(a, name), getattr(b, name))
    for name in ("explained_variance_", "explained_variance_ratio_", "components_", "location_", "scale_"):
        for x, y in zip(getattr(a, name), getattr(b, name)):
            np.testing.assert_array_equal(x, y)


def test_results_do_not_depend_on_the_workspace_the_run_or_the_neighbours(data, fitted):
    import vgan_amd
    from vgan_amd.outlier import maha_ranges
    n = ROWS[-1]
    X, a = data[n], fitted(n)
    small = 1200  # bytes: 256 cells, so several ranges of subspaces, one slab and one tile a launch
    assert len(maha_ranges(MASK.sum(axis=1), small)[1]) > 1
    _same(a, vgan_amd.SubspacePCA(MASK, PROBA, workspace_bytes=small).fit(X))
    _same(a, vgan_amd.SubspacePCA(MASK, PROBA).fit(X))
    got, per = a.decision_function(X, return_per_subspace=True)
    np.testing.assert_array_equal(per, a.per_subspace_scores_)  # nothing is excluded at fit
    np.testing.assert_array_equal(got, a.decision_scores_)
    alone = vgan_amd.SubspacePCA(MASK[6:7], [1.0]).fit(X)
    np.testing.assert_array_equal(alone.per_subspace_scores_[0], a.per_subspace_scores_[6])
    np.testing.assert_array_equal(alone.components_[0], a.components_[6])
    np.testing.assert_array_equal(alone.explained_variance_[0], a.explained_variance_[6])
    for rows in (slice(1000, 1001), slice(1000, 1100)):  # a row's bits do not depend on its position or its company
        np.testing.assert_array_equal(a.decision_function(X[rows], return_per_subspace=True)[1], a.per_subspace_scores_[:, rows])


def test_constant_subspace_and_empty_component_set_score_exactly_zero(data, fitted):
    import vgan_amd
    a = fitted(257)
    status = a._status.cpu().numpy()
    assert status[0] & 1 and not (status[1:] & 1).any() and (a.per_subspace_scores_[0] == 0).all()
    assert (a.explained_variance_[0] == 0).all() and (a.scale_[0] == 1).all() and (a.components_[0] == 1).all()
    assert (a.per_subspace_scores_[1:] > 0).any(axis=1).all()
    empty = vgan_amd.SubspacePCA(MASK, PROBA, components="minor", n_components=200).fit(data[257])
    np.testing.assert_array_equal(empty.n_components_, SIZES)
    assert (empty.per_subspace_scores_ == 0).all() and (empty.decision_scores_ == 0).all()
    assert (empty.decision_function(data[65]) == 0).all()


# ---- 5. edges ---------------------------------------------------------------------------------------------------------------
def test_max_sweeps_bounds_the_solver(data):
    import vgan_amd
    assert SIZES[5] == 17
    ens = vgan_amd.SubspacePCA(MASK[5:6], [1.0], max_sweeps=1).fit(data[257])
    assert not ens.converged_[0] and ens.n_sweeps_[0] == 1
    assert np.isfinite(ens.per_subspace_scores_).all() and np.isfinite(ens.components_[0]).all()


def test_an_unshrunk_weight_on_a_null_direction_raises_and_names_the_subspace(data):
    """Without shrinkage the first subspace with a numerically zero selected eigenvalue is named.  With the mask of this file
    that is subspace 1, not 2: its two features are the constant column and one varying one, so M = diag(0, 1) already has a
    null direction before the duplicated pair of subspace 2 comes into play (the constant subspace 0 has tr M == 0 and scores
    0 by rule).  With two ordinary features in its place, subspace 2, the one with the duplicated pair, is named."""
    import vgan_amd
    X = data[257]
    with pytest.raises(ValueError, match=r"subspace 1\b.*shrinkage > 0"):
        vgan_amd.SubspacePCA(MASK, PROBA, shrinkage=0.0).fit(X)
    mask = MASK.copy()
    mask[1] = False
    mask[1, [20, 21]] = True
    with pytest.raises(ValueError, match=r"subspace 2\b.*shrinkage > 0"):
        vgan_amd.SubspacePCA(mask, PROBA, shrinkage=0.0).fit(X)
    with pytest.raises(ValueError, match=r"subspace 2\b"):
        vgan_amd.SubspacePCA(mask, PROBA, shrinkage=0.0, components="minor", n_components=1, standardize=False).fit(X)
    ok = vgan_amd.SubspacePCA(mask, PROBA, shrinkage=0.0, components="major", n_components=1).fit(X)  # lambda_1 alone is safe
    assert np.isfinite(ok.decision_scores_).all()
    assert np.isfinite(vgan_amd.SubspacePCA(MASK, PROBA, shrinkage=0.0, weighted=False).fit(X).decision_scores_).all()


@pytest.mark.parametrize("normalize,combination", [("zscore", "max"), (None, "sum"), ("zscore", "sum"), (None, "max")])
def test_the_shared_tail_serves_the_new_scores(data, normalize, combination):
    import vgan_amd
    X, Y = data[257], data[65]
    mask = MASK[1:]  # without the constant subspace, whose scores are all equal
    proba = PROBA[1:] / PROBA[1:].sum()
    ens = vgan_amd.SubspacePCA(mask, proba, components="minor", n_components=1, normalize=normalize, combination=combination,
                               contamination=0.05).fit(X)
    per = ens.per_subspace_scores_
    c, w = (None, None) if normalize is None else _check_stats(ens, normalize)
    if normalize == "zscore":
        c, w = ens.score_center_, ens.score_scale_
    _check_scores(ens.decision_scores_, per, proba, c, w, combination)
    got, per_new = ens.decision_function(Y, return_per_subspace=True)
    _check_scores(got, per_new, proba, c, w, combination)
    assert ens.threshold_ == np.percentile(ens.decision_scores_, 95.0)
    np.testing.assert_array_equal(ens.labels_, (ens.decision_scores_ > ens.threshold_).astype(int))
    np.testing.assert_array_equal(ens.predict(Y), (got > ens.threshold_).astype(int))
    proba_out = ens.predict_proba(Y)
    assert proba_out.shape == (65, 2) and np.allclose(proba_out.sum(axis=1), 1.0) and (proba_out >= 0).all()


# ---- 6. a planted case ------------------------------------------------------------------------------------------------------
def test_minor_components_rank_the_rows_off_the_plane_first():
    import vgan_amd
    X, out = planted_plane()
    want_minor = restate_fit(X, components="minor", n_components=3, weighted=False)["scores"]
    want_major = restate_fit(X, components="major", n_components=3)["scores"]
    assert planted_ranks(want_minor, out).max() < 10 and planted_ranks(want_major, out).mean() > 30
    model = vgan_amd.VGAN_no_kl(epochs=1)
    model.subspaces, model.proba = np.ones((1, 20), bool), np.ones(1)
    minor = model.outlier_ensemble(method="pca", components="minor", n_components=3, weighted=False, X=X)
    major = model.outlier_ensemble(method="pca", components="major", n_components=3, X=X)
    assert type(minor) is vgan_amd.SubspacePCA and minor.n_components_[0] == 3
    assert planted_ranks(minor.decision_scores_, out).max() < 10
    assert planted_ranks(major.decision_scores_, out).mean() > 30
    assert minor.explained_variance_ratio_[0][:3].sum() > 0.99
