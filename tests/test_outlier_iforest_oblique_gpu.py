"""Oblique isolation-forest cuts on the MI355X (vgan_iforest_build_oblique / vgan_iforest_path_sums_oblique through
vgan_amd.SubspaceIForest(n_dims = q >= 2)), against the numpy restatement of test_outlier_iforest_oblique_cpu.py (pinned there
to a hand-worked case, to the position and weight rules and to the structure the definition demands).

Trees, planes and path sums are exact: attempts, sizes and plane columns integer-equal, thresholds and weights bit-equal (both
sides form them by the same exact integer steps, the same float64 operations and one rounding to float32), sums int64-equal.
The bar on a per-subspace score is one float32 ulp, as in test_outlier_iforest_gpu.py: sum and T cq[psi] are shared integers,
so only the final rounding of exp2 to float32 can differ.  A subspace without candidates must score exactly 0.5."""
import functools

import numpy as np
import pytest

from test_outlier_ecod_cpu import _mask, tied_data
from test_outlier_iforest_cpu import auc, depth_limit, restate_cq
from test_outlier_iforest_gpu import _check_per
from test_outlier_iforest_oblique_cpu import OBLIQUE_AUC_BAR, SKLEARN_AUC_BAR, ghost, restate_candidates, restate_oblique_iforest

pytestmark = pytest.mark.gpu

D = 73  # no multiple of 4
#: 1 feature (heavy integer ties; m_s = 1 < q), 2 features that are both constant (c_s = 0), 3 features with a constant one
#: among them (c_s = 2), 17 features, and 70 features with both constant columns among them
FEATS = [[1], [3, 60], [2, 3, 4], list(range(5, 22)), list(range(3, 73))]
CONSTANT_SUBSPACE = 1
TREE_CASES = [(2, 2), (3, "auto"), (65, 7), (300, 64), (300, 256), (1100, 1024)]


def _data(n, seed, d=D):
    """tied_data (heavy integer ties, +-0.0, the constant column 3, a descending column) with a second constant column,
    fifteen columns rounded to integers (a plane over a few of them is often constant on a small node whose rows still
    differ elsewhere: attempts fail and later ones succeed) and a third of the rows duplicated (all four attempts fail)."""
    X = tied_data(n, d, seed)
    X[:, 60] = -1.25
    X[:, 5:20] = np.round(X[:, 5:20])
    X[n - n // 3:] = X[:n // 3]
    return X


def _psi(n, max_samples):
    return min(256 if max_samples == "auto" else max_samples, n)


@functools.lru_cache(maxsize=None)
def _reference(n, max_samples, T, q, seed):
    """(X, candidates, restated forest, float64 scores, sums) of a tree case on its own rows: computed once, left unchanged."""
    X = _data(n, seed=2000 + n)
    want, sums, forest = restate_oblique_iforest(X, X, FEATS, T, max_samples, q, seed)
    for a in forest + (want, sums):
        a.setflags(write=False)
    return X, restate_candidates(X, FEATS), forest, want, sums


def _fit(X, feats, T, max_samples, q, seed, **kw):
    import vgan_amd
    proba = np.arange(1, len(feats) + 1, dtype=np.float64)
    proba /= proba.sum()
    return vgan_amd.SubspaceIForest(_mask(X.shape[1], feats), proba, n_estimators=T, max_samples=max_samples, seed=seed, n_dims=q, **kw).fit(X)


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _check_forest(ens, forest):
    attempt, threshold, size, plane_col, plane_w = forest
    assert ens.tree_attempt_.dtype == ens.tree_size_.dtype == ens.plane_features_.dtype == ens.tree_feature_.dtype == np.int32
    assert ens.tree_threshold_.dtype == ens.plane_weights_.dtype == np.float32
    assert ens.tree_attempt_.shape == attempt.shape and ens.plane_features_.shape == plane_col.shape == ens.plane_weights_.shape
    np.testing.assert_array_equal(ens.tree_attempt_, attempt)
    np.testing.assert_array_equal(ens.tree_size_, size)
    np.testing.assert_array_equal(_bits(ens.tree_threshold_), _bits(threshold))
    np.testing.assert_array_equal(ens.plane_features_, plane_col)
    np.testing.assert_array_equal(_bits(ens.plane_weights_), _bits(plane_w))
    np.testing.assert_array_equal(ens.tree_feature_, np.where(attempt >= 0, plane_col[..., 0], attempt))


def _state(ens):
    return (ens.tree_attempt_, _bits(ens.tree_threshold_), ens.tree_size_, ens.plane_features_, _bits(ens.plane_weights_),
            ens.per_subspace_scores_, ens.decision_scores_)


# ---- 1. trees, planes and sums, exact ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("q", [2, 3, 16])
@pytest.mark.parametrize("T", [1, 5])
@pytest.mark.parametrize("n,max_samples", TREE_CASES)
def test_trees_planes_and_sums_equal_the_restatement(n, max_samples, T, q):
    """n and psi at the smallest sizes, psi off and at the powers of two up to the largest tree (psi = 1 024, N = 2 048), one
    tree and several, q below, at and above the candidates of the narrow subspaces."""
    X, cands, forest, want, sums = _reference(n, max_samples, T, q, 9)
    ens = _fit(X, FEATS, T, max_samples, q, 9)
    psi = _psi(n, max_samples)
    assert ens.max_samples_ == psi and ens.depth_limit_ == depth_limit(psi) and ens.n_dims == q
    assert len(ens.candidate_features_) == len(FEATS)
    for got, c in zip(ens.candidate_features_, cands):
        assert got.dtype == np.int32
        np.testing.assert_array_equal(got, c)
    assert ens.plane_features_.shape == (len(FEATS), T, 2 << depth_limit(psi), q)
    _check_forest(ens, forest)
    if (n, max_samples, T, q) == (300, 256, 5, 2):  # a condition on the inputs: both rarer paths are on the device's way
        attempt, _, size = forest[:3]
        exhausted = ((attempt == -1) & (size > 1))[:, :, :1 << depth_limit(256)]  # leaves of several rows above the depth limit
        exhausted[CONSTANT_SUBSPACE] = False  # those are leaves for want of a candidate
        assert (attempt >= 1).any() and exhausted.any()
    # the subspace without candidates: a root leaf of psi rows and nothing else
    z = CONSTANT_SUBSPACE
    assert (ens.tree_attempt_[z, :, 1] == -1).all() and (ens.tree_size_[z, :, 1] == psi).all() and (ens.tree_attempt_[z, :, 2:] == -2).all()
    assert (ens.tree_attempt_[:, :, 0] == -2).all() and (ens.plane_features_[:, :, 0] == -1).all()
    np.testing.assert_array_equal(ens.path_sums(X), sums)
    assert (sums[z] == T * int(restate_cq(psi)[psi])).all()
    _check_per(ens.per_subspace_scores_, want, constant=[z])


# ---- 2. query-row tiling -----------------------------------------------------------------------------------------------------
def test_query_row_tiles_give_the_same_sums():
    """1, 63, 64, 65, 257 and 1 025 query rows (below, at and past a wave, a workgroup and four workgroups) against one forest."""
    X, _, forest, _, _ = _reference(300, 64, 5, 3, 9)
    ens = _fit(X, FEATS, 5, 64, 3, 9)
    Y = np.ascontiguousarray(np.resize(_data(401, seed=31), (1025, D)))
    Y[:40] = X[:40]
    want, sums, _ = restate_oblique_iforest(X, Y, FEATS, 5, 64, 3, 9, forest=forest)
    whole = ens.path_sums(Y)
    np.testing.assert_array_equal(whole, sums)
    for nq in (1, 63, 64, 65, 257, 1025):
        Q = np.ascontiguousarray(Y[:nq])
        got = ens.path_sums(Q)
        np.testing.assert_array_equal(got, sums[:, :nq])
        np.testing.assert_array_equal(got, whole[:, :nq])
        _check_per(ens.decision_function(Q, return_per_subspace=True)[1], want[:, :nq], constant=[CONSTANT_SUBSPACE])


@pytest.mark.parametrize("nq", [87_000, 90_000])
def test_sums_on_both_sides_of_the_rows_per_thread_switch(nq):
    """Six subspaces: below 512 workgroups of 1 024 rows the walk takes one row a thread (87 000 rows: 85 x 6 = 510), from there
    on four (90 000 rows: 88 x 6 = 528); neither is a multiple of 1 024."""
    feats = [[0], [1, 2], [3], [0, 4, 5], [2, 5], list(range(6))]
    X = _data(500, seed=70, d=61)[:, :6].copy()
    Y = np.ascontiguousarray(np.resize(_data(4001, seed=71, d=61)[:, :6], (nq, 6)))
    ens = _fit(X, feats, 3, 64, 2, 2)
    want, sums, _ = restate_oblique_iforest(X, Y, feats, 3, 64, 2, 2)
    np.testing.assert_array_equal(ens.path_sums(Y), sums)
    _check_per(ens.decision_function(Y, return_per_subspace=True)[1], want, constant=[2])


# ---- 3. chunking and bit equalities ----------------------------------------------------------------------------------------
def test_every_workspace_and_run_gives_the_same_bits():
    from vgan_amd.outlier import iforest_chunks
    S = len(FEATS)
    assert iforest_chunks(S, 0) == (1, 1) and iforest_chunks(S, 59) == (4, 1) and iforest_chunks(S, 120) == (S, 2)
    X, Y = _data(130, seed=81), _data(67, seed=82)
    runs = []
    for ws in (1 << 30, 1 << 30, 0, 59, 120):  # the default twice: two fits give the same bits
        ens = _fit(X, FEATS, 5, 64, 3, 6, workspace_bytes=ws)
        assert np.array_equal(ens.decision_function(X), ens.decision_scores_)  # nothing is excluded at fit
        assert np.array_equal(ens.decision_function(X, return_per_subspace=True)[1], ens.per_subspace_scores_)
        runs.append(_state(ens) + (ens.path_sums(Y),) + tuple(ens.decision_function(Y, return_per_subspace=True)))
    for other in runs[1:]:
        for a, b in zip(runs[0], other):
            assert a.dtype == b.dtype and np.array_equal(a, b)


def test_one_feature_a_cut_is_the_class_without_the_keyword():
    import vgan_amd
    X, Y = _data(300, seed=91), _data(130, seed=92)
    proba = np.full(len(FEATS), 1.0 / len(FEATS))
    plain = vgan_amd.SubspaceIForest(_mask(D, FEATS), proba, n_estimators=5, max_samples=64, seed=4).fit(X)
    keyed = vgan_amd.SubspaceIForest(_mask(D, FEATS), proba, n_estimators=5, max_samples=64, seed=4, n_dims=1).fit(X)
    for a, b in ((plain.tree_feature_, keyed.tree_feature_), (_bits(plain.tree_threshold_), _bits(keyed.tree_threshold_)),
                 (plain.tree_size_, keyed.tree_size_), (plain.path_sums(Y), keyed.path_sums(Y)),
                 (plain.per_subspace_scores_, keyed.per_subspace_scores_), (plain.decision_scores_, keyed.decision_scores_),
                 (plain.decision_function(Y), keyed.decision_function(Y))):
        assert a.dtype == b.dtype and np.array_equal(a, b)
    for attr in ("plane_features_", "plane_weights_", "tree_attempt_", "candidate_features_"):
        with pytest.raises(AttributeError, match="n_dims"):
            getattr(keyed, attr)
    oblique = _fit(X, FEATS, 5, 64, 2, 4)
    assert not np.array_equal(oblique.per_subspace_scores_[3], plain.per_subspace_scores_[3])  # the keyword changes the forest


# ---- 4. layouts at the Python boundary ---------------------------------------------------------------------------------------
def _layouts(A):
    """(name, view) pairs of A that hold its values in other layouts: rows padded to a wider array, a base shifted by three
    floats; each as a numpy array and as a torch tensor."""
    import torch
    n, d = A.shape
    padded = np.full((n, d + 7), np.float32(777.0))
    padded[:, :d] = A
    flat = np.full(3 + n * d, np.float32(-777.0))
    flat[3:] = A.reshape(-1)
    views = [("padded", padded[:, :d]), ("shifted", flat[3:].reshape(n, d))]
    assert not views[0][1].flags["C_CONTIGUOUS"] and all(np.array_equal(v, A) for _, v in views)
    return views + [(name + "-torch", torch.from_numpy(v)) for name, v in views]


def test_padded_and_shifted_inputs_give_the_bits_of_the_contiguous_copy():
    X, Y = _data(130, seed=101), _data(67, seed=102)
    base = _fit(X, FEATS, 5, 64, 3, 1)
    want_state = _state(base)
    want_sums = base.path_sums(Y)
    want_scores, want_per = base.decision_function(Y, return_per_subspace=True)
    for name, view in _layouts(X):
        ens = _fit(view, FEATS, 5, 64, 3, 1)
        for a, b in zip(want_state, _state(ens)):
            assert a.dtype == b.dtype and np.array_equal(a, b), name
    for name, view in _layouts(Y):
        assert np.array_equal(base.path_sums(view), want_sums), name
        got, per = base.decision_function(view, return_per_subspace=True)
        assert np.array_equal(got, want_scores) and np.array_equal(per, want_per), name


# ---- 5. detection ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", [0, 1, 2])
def test_oblique_cuts_find_the_ghost_outliers_on_the_device(seed):
    """The recipe and the bars of test_outlier_iforest_oblique_cpu.py: n_dims = 3 above the restatement's bar, the axis-parallel
    forest of this class below sklearn's."""
    import vgan_amd
    X, y = ghost(seed)
    mask = _mask(6, [list(range(6))])
    oblique = vgan_amd.SubspaceIForest(mask, [1.0], n_estimators=100, max_samples=256, seed=seed, n_dims=3).fit(X)
    axis = vgan_amd.SubspaceIForest(mask, [1.0], n_estimators=100, max_samples=256, seed=seed, n_dims=1).fit(X)
    got, flat = auc(oblique.decision_scores_, y), auc(axis.decision_scores_, y)
    print(f"ghost seed {seed}: n_dims = 3 AUC {got:.4f}, n_dims = 1 AUC {flat:.4f}")
    assert got > OBLIQUE_AUC_BAR
    assert flat < SKLEARN_AUC_BAR
