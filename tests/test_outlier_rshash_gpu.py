"""RS-Hash over the subspaces on the MI355X (csrc/outlier_rshash.hip through vgan_amd.SubspaceRSHash), against the numpy
restatement of test_outlier_rshash_cpu.py (pinned there to a hand-worked case and to an independent count of the cells).

Cells and sums are exact: the numbers of cells, the keys and the counts integer-equal, the sample minima and maxima bit-equal,
the int64 sums equal for the fitted rows and for new rows.  The bar on a per-subspace score is one float32 ulp, |got - want|
<= 2^-23 |want| with no absolute term, the forest's argument: kernel and restatement share the exactly representable
integers sum and T table[s + 1], their correctly rounded quotient and its correctly rounded difference from 1, so only the
final rounding to float32 could differ.  A subspace of constant features has sum == T table[s + 1] and must score exactly
0."""
import functools

import numpy as np
import pytest

from test_outlier_dif_cpu import corr
from test_outlier_ecod_cpu import _mask, tied_data
from test_outlier_gpu import _planted
from test_outlier_iforest_cpu import auc
from test_outlier_norm_cpu import restate_proba
from test_outlier_norm_gpu import _check_scores, _check_stats
from test_outlier_rshash_cpu import restate_fit, restate_rshash, restate_scores, restate_sums

pytestmark = pytest.mark.gpu

ULP32 = 2.0 ** -23
D = 310
#: subspaces of 1 (heavy integer ties), 5, 67 and 300 (wider than a workgroup) features, and the constant column alone
FEATS = [[1], [0, 1, 2, 3, 4], list(range(3, 70)), list(range(300)), [3]]
CASES = [(2, 2), (3, 4), (63, 64), (64, 64), (65, 64), (257, 256), (1000, "auto"), (1500, 1024), (5000, 4096)]


def _data(n, d, seed):
    """tied_data (heavy integer ties, +-0.0, a constant and a descending column) with a third of the rows duplicated."""
    X = tied_data(n, d, seed)
    X[n - n // 3:] = X[:n // 3]
    return X


def _components(n, max_samples):
    return 2 if min(1000 if max_samples == "auto" else max_samples, n) > 1024 else 7


@functools.lru_cache(maxsize=None)
def _reference(n, max_samples):
    """(X, Y, restated model with fit_sums and query_sums, fit scores, query scores) of a case: computed once, shared."""
    X, Y = _data(n, D, seed=1000 + n), _data(97, D, seed=2000 + n)
    Y[:min(20, n)] = X[:min(20, n)]
    m, fit, new = restate_rshash(X, Y, FEATS, _components(n, max_samples), max_samples, 9)
    for a in (X, Y, m.cell_key, m.cell_count, m.n_cells, m.sample_min, m.sample_max, m.fit_sums, m.query_sums, fit, new):
        a.setflags(write=False)
    return X, Y, m, fit, new


def _fit(X, feats, T, max_samples, seed, **kw):
    import vgan_amd
    proba = np.arange(1, len(feats) + 1, dtype=np.float64)
    proba /= proba.sum()
    return vgan_amd.SubspaceRSHash(_mask(X.shape[1], feats), proba, n_estimators=T, max_samples=max_samples, seed=seed, **kw).fit(X), proba


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _check_state(ens, m):
    assert ens.max_samples_ == m.s
    assert ens.cell_key_.dtype == np.uint64 and ens.cell_count_.dtype == np.int32 and ens.n_cells_.dtype == np.int32
    assert ens.sample_min_.dtype == np.float32 and ens.sample_max_.dtype == np.float32
    assert ens.cell_key_.shape == ens.cell_count_.shape == (m.S, m.T, m.s) and ens.sample_min_.shape == (m.S, m.T, 12)
    np.testing.assert_array_equal(ens.n_cells_, m.n_cells)
    np.testing.assert_array_equal(ens.cell_key_, m.cell_key)
    np.testing.assert_array_equal(ens.cell_count_, m.cell_count)
    np.testing.assert_array_equal(_bits(ens.sample_min_), _bits(m.sample_min))
    np.testing.assert_array_equal(_bits(ens.sample_max_), _bits(m.sample_max))
    for z in range(m.S):
        np.testing.assert_array_equal(ens.candidate_features_[z], m.candidates[z])
        for t, comp in enumerate(m.comps[z]):
            r = len(comp[0])
            assert ens.component_dims_[z, t] == r and ens.grid_width_[z, t] == comp[2]
            np.testing.assert_array_equal(ens.component_features_[z, t, :r], comp[0])
            np.testing.assert_array_equal(ens.component_shift_[z, t, :r], comp[1])


def _check_per(got32, want, constant=()):
    got32 = np.asarray(got32)
    assert got32.dtype == np.float32 and got32.shape == want.shape
    want32 = want.astype(np.float32).astype(np.float64)
    np.testing.assert_allclose(got32.astype(np.float64), want32, rtol=ULP32, atol=0)
    assert (got32 >= 0).all() and (got32 <= 1).all()
    for z in constant:
        assert (got32[z] == 0).all()


# ---- 1. cells, sums and scores ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,max_samples", CASES)
def test_cells_sums_and_scores_equal_the_restatement(n, max_samples):
    """n and s at the smallest sizes, s above n, n one below, at and one above s = 64 (the sort's padding, one row outside the
    sample), s = 256 of 257, "auto" = 1 000 = n, s = 1 024 of 1 500 and s = 4 096 (the largest sample: 48 KB of LDS in the build,
    56 KB in the fit's look-up)."""
    X, Y, m, fit, new = _reference(n, max_samples)
    T = _components(n, max_samples)
    ens, proba = _fit(X, FEATS, T, max_samples, 9)
    _check_state(ens, m)
    assert (ens.n_cells_[4] == 0).all() and (ens.component_dims_[4] == 0).all()  # the constant column alone: no component
    np.testing.assert_array_equal(ens.cell_sums_, m.fit_sums)
    _check_per(ens.per_subspace_scores_, fit, constant=[4])
    _check_scores(ens.decision_scores_, ens.per_subspace_scores_, proba, None, None, "sum")
    np.testing.assert_array_equal(ens.cell_sums(Y), m.query_sums)
    got, per = ens.decision_function(Y, return_per_subspace=True)
    _check_per(per, new, constant=[4])
    _check_scores(got, per, proba, None, None, "sum")
    if n <= m.s:  # every row is in every sample: as new rows every count is exactly one more, and the two scores differ
        again = restate_sums(m, X)
        np.testing.assert_array_equal(ens.cell_sums(X), again)
        live = [z for z in range(m.S) if m.comps[z]]
        assert (again[live] > m.fit_sums[live]).all()
        assert (ens.decision_function(X, return_per_subspace=True)[1][live] < ens.per_subspace_scores_[live]).all()


@pytest.mark.parametrize("nq", [87_000, 90_000])
def test_sums_on_both_sides_of_the_rows_per_thread_switch(nq):
    """Six subspaces: below 512 workgroups of 1 024 rows the look-up takes one row a thread (87 000 rows: 85 x 6 = 510), from
    there on four (90 000 rows: 88 x 6 = 528); neither is a multiple of 1 024.  Fitted on the same rows, so that both the
    fit's look-up (with the in-sample test) and the one for new rows take either path."""
    feats = [[0], [1, 2], [3], [0, 4, 5], [2, 5], list(range(6))]
    X = np.ascontiguousarray(np.resize(_data(4001, 6, seed=71), (nq, 6)))
    ens, _ = _fit(X, feats, 3, 64, 2)
    m, fit, new = restate_rshash(X, X, feats, 3, 64, 2)
    _check_state(ens, m)
    np.testing.assert_array_equal(ens.cell_sums_, m.fit_sums)
    np.testing.assert_array_equal(ens.cell_sums(X), m.query_sums)
    _check_per(ens.per_subspace_scores_, fit, constant=[2])
    _check_per(ens.decision_function(X, return_per_subspace=True)[1], new, constant=[2])


# ---- 2. edges --------------------------------------------------------------------------------------------------------------
def test_a_feature_constant_inside_the_samples_but_not_over_the_data():
    """One nonzero entry in 1 000 rows and samples of 4 rows: the feature is a candidate, and in nearly every component w = 0."""
    rng = np.random.default_rng(3)
    X = np.zeros((1000, 3), np.float32)
    X[617, 0] = 1.0
    X[:, 1:] = rng.normal(size=(1000, 2))
    feats = [[0], [0, 1, 2], [1]]
    ens, _ = _fit(X, feats, 7, 4, 1)
    m, fit, new = restate_rshash(X, X, feats, 7, 4, 1)
    assert list(m.candidates[0]) == [0]
    flat = sum(1 for comp in m.comps[0] if comp[5][0] == comp[6][0])
    assert flat >= 6  # mn == mx in (nearly) every component of the first subspace
    _check_state(ens, m)
    np.testing.assert_array_equal(ens.cell_sums_, m.fit_sums)
    np.testing.assert_array_equal(ens.cell_sums(X), m.query_sums)
    _check_per(ens.per_subspace_scores_, fit)


def test_new_rows_on_and_beyond_the_sample_range():
    """New rows at exactly mn_j and at exactly mx_j of a component's chosen features, one float32 step outside either, and at
    +-1e30: the rows far outside take the clamped digits 0 and R - 1, which no sampled row has, so their cells count 0 and c =
    1 in every component: sum 0, score exactly 1."""
    X = _data(300, 6, seed=5)
    feats = [[0, 1, 2, 4, 5], [0, 5]]
    T = 7
    ens, _ = _fit(X, feats, T, 64, 8)
    m = restate_fit(X, feats, T, 64, 8)
    rows = []
    for z in range(2):
        for cols, alpha, f, keys, counts, mn, mx in m.comps[z]:
            for value in (mn, mx, np.nextafter(mn, np.float32(-np.inf)), np.nextafter(mx, np.float32(np.inf))):
                q = X[len(rows) % 300].copy()
                q[cols] = value
                rows.append(q)
    far = np.full((2, 6), 1e30, np.float32)
    far[1] = -1e30
    Q = np.vstack([np.array(rows, np.float32), far])
    want = restate_sums(m, Q)
    assert (want[:, -2:] == 0).all()
    got = ens.cell_sums(Q)
    np.testing.assert_array_equal(got, want)
    per = ens.decision_function(Q, return_per_subspace=True)[1]
    _check_per(per, restate_scores(m, want))
    assert (per[:, -2:] == 1).all()


# ---- 3. bit identity -------------------------------------------------------------------------------------------------------
def test_everything_is_bit_identical_for_every_workspace_split_layout_and_run():
    import vgan_amd
    from vgan_amd.outlier import iforest_chunks
    n, T = 700, 5
    feats = FEATS[:3] + [FEATS[4]]
    X, Y = _data(n, D, seed=81), _data(130, D, seed=82)
    S = len(feats)
    assert iforest_chunks(S, 12) == (1, 1) and iforest_chunks(S, 12 * S) == (S, 1) and iforest_chunks(S, 12 * 3) == (3, 1)
    runs = []
    for ws, column_major in ((1 << 30, False), (1 << 30, False), (12, False), (12 * S, False), (12 * 3, False), (1 << 30, True), (12 * 40, True)):
        ens = vgan_amd.SubspaceRSHash(_mask(D, feats), np.full(S, 1.0 / S), n_estimators=T, max_samples=128, seed=6, workspace_bytes=ws)
        ens._column_major = column_major  # the look-up through a column-major copy of X
        ens.fit(X)
        whole, per = ens.decision_function(Y, return_per_subspace=True)
        parts = [ens.decision_function(Y[a:b], return_per_subspace=True) for a, b in ((0, 1), (1, 32), (32, 65), (65, 130))]
        assert np.array_equal(np.concatenate([p[0] for p in parts]), whole)
        assert np.array_equal(np.concatenate([p[1] for p in parts], axis=1), per)
        assert np.array_equal(np.concatenate([ens.cell_sums(Y[a:b]) for a, b in ((0, 1), (1, 32), (32, 65), (65, 130))], axis=1), ens.cell_sums(Y))
        runs.append((ens.cell_key_, ens.cell_count_, ens.n_cells_, _bits(ens.sample_min_), _bits(ens.sample_max_), ens.cell_sums_,
                     ens.per_subspace_scores_, ens.decision_scores_, ens.cell_sums(Y), whole, per))
    for other in runs[1:]:
        for a, b in zip(runs[0], other):
            assert a.dtype == b.dtype and np.array_equal(a, b)


# ---- 4. the shared tail ----------------------------------------------------------------------------------------------------
def test_normalize_max_predict_and_predict_proba_on_rshash_scores():
    import vgan_amd
    X = _planted()
    Xr, Y = np.ascontiguousarray(X[:1500]), np.ascontiguousarray(X[1400:])
    feats = [[0, 1], [0, 1, 2], [4, 7], list(range(10))]
    proba = np.array([0.4, 0.3, 0.2, 0.1])
    ens = vgan_amd.SubspaceRSHash(_mask(10, feats), proba, n_estimators=17, max_samples=128, seed=1, normalize="robust", combination="max",
                                  contamination=0.05).fit(Xr)
    m, fit, new = restate_rshash(Xr, Y, feats, 17, 128, 1)
    per = ens.per_subspace_scores_
    _check_per(per, fit)
    c, w = _check_stats(ens, "robust")
    _check_scores(ens.decision_scores_, per, proba, c, w, "max")
    assert ens.threshold_ == np.percentile(ens.decision_scores_, 95.0)
    np.testing.assert_array_equal(ens.labels_, (ens.decision_scores_ > ens.threshold_).astype(int))
    assert ens.labels_.shape == (1500,) and 0 < ens.labels_.sum() <= 75
    got, per_new = ens.decision_function(Y, return_per_subspace=True)
    _check_per(per_new, new)
    _check_scores(got, per_new, proba, c, w, "max")  # the statistics of the fit
    np.testing.assert_array_equal(ens.predict(Y), (got > ens.threshold_).astype(int))
    p = ens.predict_proba(Y)
    assert p.shape == (620, 2)
    np.testing.assert_allclose(p, restate_proba(ens.decision_scores_, got, "linear"), rtol=1e-12, atol=1e-15)


# ---- 5. the recipe and the model ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", [0, 1, 2])
def test_recipe_auc_on_the_device_equals_the_restatements(seed):
    import vgan_amd
    X, y = corr(seed=seed)
    every = [list(range(6))]
    ens = vgan_amd.SubspaceRSHash(_mask(6, every), [1.0], seed=seed).fit(X)
    m, fit, _ = restate_rshash(X, None, every, seed=seed)
    np.testing.assert_array_equal(ens.cell_sums_, m.fit_sums)
    got, want = auc(ens.decision_scores_, y), auc(fit[0], y)
    print(f"corr({seed}): ROC AUC device {got:.5f}, restatement {want:.5f}")
    assert abs(got - want) <= 1e-3


def test_vgan_outlier_ensemble_rshash_end_to_end():
    import vgan_amd
    X = _planted()[:, :10]
    model = vgan_amd.VGAN_no_kl(epochs=2)
    model.fit(X)
    ens = model.outlier_ensemble(method="rshash", n_neighbors=3, n_estimators=5, max_samples=64, X=X)  # n_neighbors is ignored
    assert isinstance(ens, vgan_amd.SubspaceRSHash)
    S = model.subspaces.shape[0]
    feats = [np.flatnonzero(model.subspaces[s]) for s in range(S)]
    per = ens.per_subspace_scores_
    assert per.shape == (S, X.shape[0]) and np.isfinite(per).all()
    _check_per(per, restate_rshash(X, None, feats, 5, 64, 0)[1])
    _check_scores(ens.decision_scores_, per, model.proba, None, None, "sum")
    ens = model.outlier_ensemble(method="rshash", n_estimators=5, max_samples=64, normalize="minmax", X=X)
    assert ens.predict_proba(X[:50]).shape == (50, 2)
