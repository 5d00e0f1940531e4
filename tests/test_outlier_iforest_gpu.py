"""Isolation forest over the subspaces on the MI355X (csrc/outlier_iforest.hip through vgan_amd.SubspaceIForest), against the
numpy restatement of test_outlier_iforest_cpu.py (pinned there to sklearn and to a hand-worked case).

Trees and path sums are exact: features and sizes integer-equal, thresholds bit-equal (both sides form them by the same
three float64 operations and one rounding to float32), sums int64-equal.  The bar on a per-subspace score is one float32
ulp, |got - want| <= 2^-23 |want| with no absolute term: kernel and restatement share the exactly representable integers sum
and T cq[psi] and their correctly rounded quotient; the two exp2 differ by ulps of float64; so only the final rounding to
float32 can differ, by one ulp where the float64 values straddle a rounding boundary.  A subspace of constant features has
sum == T cq[psi] and must score exactly 0.5."""
import functools

import numpy as np
import pytest

from test_outlier_ecod_cpu import _mask, tied_data
from test_outlier_gpu import _planted
from test_outlier_iforest_cpu import depth_limit, restate_cq, restate_forest, restate_iforest
from test_outlier_norm_cpu import restate_proba
from test_outlier_norm_gpu import _check_scores, _check_stats

pytestmark = pytest.mark.gpu

ULP32 = 2.0 ** -23
D = 310
#: subspaces of 1 (heavy integer ties), 5, 67 and 300 (wider than a workgroup) features, and the constant column alone
FEATS = [[1], [0, 1, 2, 3, 4], list(range(3, 70)), list(range(300)), [3]]
TREE_CASES = [(2, 2), (3, 3), (100, 7), (255, 256), (256, 256), (257, "auto"), (1000, 2), (1500, 1024)]


def _data(n, d, seed):
    """tied_data (heavy integer ties, +-0.0, a constant and a descending column) with a third of the rows duplicated."""
    X = tied_data(n, d, seed)
    X[n - n // 3:] = X[:n // 3]
    return X


def _psi(n, max_samples):
    return min(256 if max_samples == "auto" else max_samples, n)


@functools.lru_cache(maxsize=None)
def _reference(n, max_samples, T, seed):
    """(X, restated forest) of a tree case: computed once, shared by the tests below and left unchanged."""
    X = _data(n, D, seed=1000 + n)
    forest = restate_forest(X, FEATS, T, _psi(n, max_samples), seed)
    for a in forest:
        a.setflags(write=False)
    return X, forest


def _trees(n, max_samples):
    return 2 if _psi(n, max_samples) > 256 else 3


def _fit(X, feats, T, max_samples, seed, **kw):
    import vgan_amd
    proba = np.arange(1, len(feats) + 1, dtype=np.float64)
    proba /= proba.sum()
    return vgan_amd.SubspaceIForest(_mask(X.shape[1], feats), proba, n_estimators=T, max_samples=max_samples, seed=seed, **kw).fit(X), proba


def _check_forest(ens, forest):
    feature, threshold, size = forest
    assert ens.tree_feature_.dtype == np.int32 and ens.tree_size_.dtype == np.int32 and ens.tree_threshold_.dtype == np.float32
    assert ens.tree_feature_.shape == feature.shape
    np.testing.assert_array_equal(ens.tree_feature_, feature)
    np.testing.assert_array_equal(ens.tree_size_, size)
    np.testing.assert_array_equal(np.ascontiguousarray(ens.tree_threshold_).view(np.uint32), np.ascontiguousarray(threshold).view(np.uint32))


def _check_per(got32, want, constant=()):
    got32 = np.asarray(got32)
    assert got32.dtype == np.float32 and got32.shape == want.shape
    want32 = want.astype(np.float32).astype(np.float64)
    np.testing.assert_allclose(got32.astype(np.float64), want32, rtol=ULP32, atol=0)
    assert (got32 > 0).all() and (got32 <= 1).all()
    for s in constant:
        assert (got32[s] == np.float32(0.5)).all()


# ---- 1. the trees ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,max_samples", TREE_CASES)
def test_trees_equal_the_restatement(n, max_samples):
    """n and psi at the smallest sizes, psi off and at the powers of two, n one below, at and one above "auto", psi = 2 on many
    rows and psi = 1 024 (the largest tree, N = 2 048)."""
    T = _trees(n, max_samples)
    X, forest = _reference(n, max_samples, T, 9)
    ens, _ = _fit(X, FEATS, T, max_samples, 9)
    psi = _psi(n, max_samples)
    assert ens.max_samples_ == psi and ens.depth_limit_ == depth_limit(psi)
    assert ens.tree_feature_.shape == (len(FEATS), T, 2 << depth_limit(psi))
    _check_forest(ens, forest)
    # the subspace of the constant column: a root leaf of psi rows and nothing else
    assert (ens.tree_feature_[4, :, 1] == -1).all() and (ens.tree_size_[4, :, 1] == psi).all()
    assert (ens.tree_feature_[4, :, 2:] == -2).all() and (ens.tree_feature_[:, :, 0] == -2).all()
    # fit scored the training rows through those trees
    want, sums = restate_iforest(X, X, FEATS, T, max_samples, 9, forest=forest)
    np.testing.assert_array_equal(ens.path_sums(X), sums)
    _check_per(ens.per_subspace_scores_, want, constant=[4])


# ---- 2. sums and scores ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("T,max_samples,feats", [(1, "auto", [0, 1, 4]), (7, 256, [0, 1, 4]), (17, 100, [0, 1, 2, 4]), (100, 64, [1, 4]),
                                                 (1024, 16, [1])])
def test_sums_and_scores_match_the_restatement(T, max_samples, feats):
    """T below, at no multiple of and across several LDS groups of trees (8 trees a group at N = 512, 16 at 256, 32 at 128, 128
    at 32); query sets of 1, 63, 64, 65 and 257 rows."""
    feats = [FEATS[k] for k in feats]
    X = _data(300, D, seed=50 + T)
    Y = _data(257, D, seed=60 + T)
    Y[:40] = X[:40]
    ens, proba = _fit(X, feats, T, max_samples, 4)
    forest = restate_forest(X, feats, T, _psi(300, max_samples), 4)
    _check_forest(ens, forest)
    constant = [k for k, f in enumerate(feats) if f == [3]]
    want, sums = restate_iforest(X, Y, feats, T, max_samples, 4, forest=forest)
    for nq in (1, 63, 64, 65, 257):
        Q = np.ascontiguousarray(Y[:nq])
        np.testing.assert_array_equal(ens.path_sums(Q), sums[:, :nq])
        got, per = ens.decision_function(Q, return_per_subspace=True)
        _check_per(per, want[:, :nq], constant)
        _check_scores(got, per, proba, None, None, "sum")
        np.testing.assert_allclose(got, proba @ want[:, :nq], rtol=2.4e-7, atol=0)
    fit_want, fit_sums = restate_iforest(X, X, feats, T, max_samples, 4, forest=forest)
    np.testing.assert_array_equal(ens.path_sums(X), fit_sums)
    _check_per(ens.per_subspace_scores_, fit_want, constant)
    _check_scores(ens.decision_scores_, ens.per_subspace_scores_, proba, None, None, "sum")


@pytest.mark.parametrize("nq", [87_000, 90_000])
def test_sums_on_both_sides_of_the_rows_per_thread_switch(nq):
    """Six subspaces: below 512 workgroups of 1 024 rows the walk takes one row a thread (87 000 rows: 85 x 6 = 510), from there
    on four (90 000 rows: 88 x 6 = 528); neither is a multiple of 1 024."""
    feats = [[0], [1, 2], [3], [0, 4, 5], [2, 5], list(range(6))]
    X = _data(500, 6, seed=70)
    Y = np.ascontiguousarray(np.resize(_data(4001, 6, seed=71), (nq, 6)))
    ens, _ = _fit(X, feats, 3, 64, 2)
    want, sums = restate_iforest(X, Y, feats, 3, 64, 2)
    np.testing.assert_array_equal(ens.path_sums(Y), sums)
    _check_per(ens.decision_function(Y, return_per_subspace=True)[1], want, constant=[2])


# ---- 3. bit identity -------------------------------------------------------------------------------------------------------
def test_trees_and_scores_are_bit_identical_for_every_workspace_and_run():
    from vgan_amd.outlier import iforest_chunks
    n, T = 700, 5
    feats = FEATS[:3] + [FEATS[4]]
    X, Y = _data(n, D, seed=81), _data(130, D, seed=82)
    S = len(feats)
    assert iforest_chunks(S, 1 << 30) == (S, (1 << 30) // (12 * S))  # the default: one range, one chunk
    assert iforest_chunks(S, 12) == (1, 1)  # one subspace a build range (and single rows)
    assert iforest_chunks(S, 12 * S) == (S, 1)  # every subspace, chunks of a single row
    runs = []
    for ws in (1 << 30, 1 << 30, 12, 12 * S):
        ens, _ = _fit(X, feats, T, 128, 6, workspace_bytes=ws)
        assert np.array_equal(ens.decision_function(X), ens.decision_scores_)  # nothing is excluded at fit
        got, per = ens.decision_function(X, return_per_subspace=True)
        assert np.array_equal(per, ens.per_subspace_scores_)
        runs.append((ens.tree_feature_, ens.tree_threshold_.view(np.uint32), ens.tree_size_, ens.per_subspace_scores_, ens.decision_scores_,
                     ens.path_sums(Y), *ens.decision_function(Y, return_per_subspace=True)))
    for other in runs[1:]:
        for a, b in zip(runs[0], other):
            assert a.dtype == b.dtype and np.array_equal(a, b)


# ---- 4. the shared tail ----------------------------------------------------------------------------------------------------
def test_normalize_max_predict_and_predict_proba_on_iforest_scores():
    import vgan_amd
    X = _planted()
    Xr, Y = np.ascontiguousarray(X[:1500]), np.ascontiguousarray(X[1400:])
    feats = [[0, 1], [0, 1, 2], [4, 7], list(range(10))]
    proba = np.array([0.4, 0.3, 0.2, 0.1])
    ens = vgan_amd.SubspaceIForest(_mask(10, feats), proba, n_estimators=17, max_samples=128, seed=1, normalize="robust", combination="max",
                                   contamination=0.05).fit(Xr)
    forest = restate_forest(Xr, feats, 17, 128, 1)
    per = ens.per_subspace_scores_
    _check_per(per, restate_iforest(Xr, Xr, feats, 17, 128, 1, forest=forest)[0])
    c, w = _check_stats(ens, "robust")
    _check_scores(ens.decision_scores_, per, proba, c, w, "max")
    assert ens.threshold_ == np.percentile(ens.decision_scores_, 95.0)
    np.testing.assert_array_equal(ens.labels_, (ens.decision_scores_ > ens.threshold_).astype(int))
    assert ens.labels_.shape == (1500,) and 0 < ens.labels_.sum() <= 75
    got, per_new = ens.decision_function(Y, return_per_subspace=True)
    _check_per(per_new, restate_iforest(Xr, Y, feats, 17, 128, 1, forest=forest)[0])
    _check_scores(got, per_new, proba, c, w, "max")  # the statistics of the fit
    np.testing.assert_array_equal(ens.predict(Y), (got > ens.threshold_).astype(int))
    p = ens.predict_proba(Y)
    assert p.shape == (620, 2)
    np.testing.assert_allclose(p, restate_proba(ens.decision_scores_, got, "linear"), rtol=1e-12, atol=1e-15)


# ---- 5. through the model --------------------------------------------------------------------------------------------------
def test_vgan_outlier_ensemble_iforest_end_to_end():
    import vgan_amd
    X = _planted()[:, :10]
    model = vgan_amd.VGAN_no_kl(epochs=2)
    model.fit(X)
    ens = model.outlier_ensemble(method="iforest", n_neighbors=3, n_estimators=5, max_samples=64, X=X)  # n_neighbors is ignored
    assert isinstance(ens, vgan_amd.SubspaceIForest)
    S = model.subspaces.shape[0]
    feats = [np.flatnonzero(model.subspaces[s]) for s in range(S)]
    per = ens.per_subspace_scores_
    assert per.shape == (S, X.shape[0]) and np.isfinite(per).all()
    _check_per(per, restate_iforest(X, X, feats, 5, 64, 0)[0])
    _check_scores(ens.decision_scores_, per, model.proba, None, None, "sum")
    ens = model.outlier_ensemble(method="iforest", n_estimators=5, max_samples=64, normalize="minmax", X=X)
    assert ens.predict_proba(X[:50]).shape == (50, 2)
