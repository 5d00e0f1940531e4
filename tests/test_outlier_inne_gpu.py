"""iNNE over the subspaces on the MI355X (csrc/outlier_inne.hip through vgan_amd.SubspaceINNE), against the numpy restatement
of test_outlier_inne_cpu.py (pinned there to a hand-worked case, to the scalar loops of the definition and to sklearn).

With ratio="squared" nothing has a tolerance: centre rows and nearest positions are integer-equal, radius_sq_ and
isolation_ratio_ bit-equal as uint64, and the per-subspace scores bit-equal to float32 of the restatement: both sides do the
same separately rounded float64 operations in the same order and round once.  With ratio="distance" the two square roots of
a ratio may each differ in the last place between device and numpy, so isolation_ratio_ is within 4 * 2^-53 absolute (two
square roots and three operations on values in [0, 1]) and the scores within rtol 2^-23, atol 2^-40."""
import functools

import numpy as np
import pytest

from test_outlier_ecod_cpu import _mask, tied_data
from test_outlier_gpu import _planted
from test_outlier_inne_cpu import restate_inne_both
from test_outlier_norm_cpu import restate_proba
from test_outlier_norm_gpu import _check_scores, _check_stats

pytestmark = pytest.mark.gpu

D = 310
#: subspaces of 1 (heavy integer ties), 5, 67 (three feature tiles) and 300 features, and the constant column alone
FEATS = [[1], [0, 1, 2, 3, 4], list(range(3, 70)), list(range(300)), [3]]
#: (n, max_samples, T): the smallest sizes, "auto" above n's minimum, psi off the tiles of 16 centres, at and one above
#: a multiple of them, the largest psi (four passes of the build), and T psi = 296 centres: a ragged last tile
CASES = [(2, 2, 3), (3, 3, 3), (9, "auto", 3), (100, 7, 3), (300, 64, 3), (300, 65, 3), (1500, 1024, 2), (100, 8, 37)]
RATIO_BAR = 4 * 2.0 ** -53
SEED = 9


def _data(n, d, seed):
    """tied_data (heavy integer ties, +-0.0, a constant and a descending column) with a third of the rows duplicated."""
    X = tied_data(n, d, seed)
    X[n - n // 3:] = X[:n // 3]
    return X


def _psi(n, max_samples):
    return min(8 if max_samples == "auto" else max_samples, n)


def _queries(X):
    """1 000 new rows: fresh ones, exact copies of fitted rows and rows far outside the data (the constant column kept)."""
    Y = _data(1000, D, seed=77)
    k = min(40, X.shape[0])
    Y[1:1 + k] = X[:k]
    Y[300:320] += np.float32(1.0e4)
    Y[300:320, 3] = 2.5
    return Y


@functools.lru_cache(maxsize=None)
def _reference(n, max_samples, T, with_queries=False):
    """(X, Y or None, {ratio: ([fit scores, query scores], state)}) of a case: computed once, shared by the tests below and
    left unchanged."""
    X = _data(n, D, seed=1000 + n)
    Y = _queries(X) if with_queries else None
    both = restate_inne_both(X, [X] + ([Y] if with_queries else []), FEATS, T, max_samples, SEED)
    for scores, state in both.values():
        for a in list(scores) + list(state):
            a.setflags(write=False)
    return X, Y, both


def _fit(X, feats, T, max_samples, ratio, seed=SEED, **kw):
    import vgan_amd
    proba = np.arange(1, len(feats) + 1, dtype=np.float64)
    proba /= proba.sum()
    ens = vgan_amd.SubspaceINNE(_mask(X.shape[1], feats), proba, n_estimators=T, max_samples=max_samples, ratio=ratio, seed=seed, **kw)
    return ens.fit(X), proba


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint64)


def _check_state(ens, state, ratio):
    rows, r2, nn, rho = state
    assert ens.center_rows_.dtype == np.int32 and ens.center_nn_.dtype == np.int32
    assert ens.radius_sq_.dtype == np.float64 and ens.isolation_ratio_.dtype == np.float64
    assert ens.center_rows_.shape == ens.center_nn_.shape == ens.radius_sq_.shape == ens.isolation_ratio_.shape == rows.shape
    np.testing.assert_array_equal(ens.center_rows_, rows)
    np.testing.assert_array_equal(ens.center_nn_, nn)
    np.testing.assert_array_equal(_bits(ens.radius_sq_), _bits(r2))
    if ratio == "squared":
        np.testing.assert_array_equal(_bits(ens.isolation_ratio_), _bits(rho))
    else:
        np.testing.assert_allclose(ens.isolation_ratio_, rho, rtol=0, atol=RATIO_BAR)
    assert (ens.isolation_ratio_ >= 0).all() and (ens.isolation_ratio_ <= 1).all()


def _check_per(got32, want, ratio):
    got32 = np.asarray(got32)
    assert got32.dtype == np.float32 and got32.shape == want.shape
    if ratio == "squared":
        np.testing.assert_array_equal(got32.view(np.uint32), want.astype(np.float32).view(np.uint32))
    else:
        np.testing.assert_allclose(got32.astype(np.float64), want, rtol=2.0 ** -23, atol=2.0 ** -40)
    assert (got32 >= 0).all() and (got32 <= 1).all()


# ---- 1. the fitted state and the scores of the fitted rows ----------------------------------------------------------------------
@pytest.mark.parametrize("ratio", ["squared", "distance"])
@pytest.mark.parametrize("n,max_samples,T", CASES)
def test_fitted_state_and_scores_equal_the_restatement(n, max_samples, T, ratio):
    X, _, both = _reference(n, max_samples, T)
    (fit_scores,), state = both[ratio]
    ens, proba = _fit(X, FEATS, T, max_samples, ratio)
    psi = _psi(n, max_samples)
    assert ens.max_samples_ == psi and ens.center_rows_.shape == (len(FEATS), T, psi)
    _check_state(ens, state, ratio)
    _check_per(ens.per_subspace_scores_, fit_scores, ratio)
    # the constant column: every radius 0, every ratio 1 - eps / eps = 0, every row covered
    assert (ens.radius_sq_[4] == 0).all() and (ens.isolation_ratio_[4] == 0).all() and (ens.per_subspace_scores_[4] == 0).all()
    _check_scores(ens.decision_scores_, ens.per_subspace_scores_, proba, None, None, "sum")
    # fit excluded nothing
    got, per = ens.decision_function(X, return_per_subspace=True)
    assert np.array_equal(per.view(np.uint32), ens.per_subspace_scores_.view(np.uint32))
    assert np.array_equal(got.view(np.uint64), ens.decision_scores_.view(np.uint64))


# ---- 2. new rows -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ratio", ["squared", "distance"])
def test_decision_function_on_new_rows(ratio):
    """1, 257 and 1 000 query rows (none a multiple of a workgroup's 256), exact copies of fitted rows, rows far outside the
    data, and a query matrix and a fitted matrix whose row strides are not d."""
    import torch
    n, max_samples, T = 300, 64, 3
    X, Y, both = _reference(n, max_samples, T, with_queries=True)
    (fit_scores, want), state = both[ratio]
    ens, proba = _fit(X, FEATS, T, max_samples, ratio)
    _check_state(ens, state, ratio)
    for nq in (1, 257, 1000):
        Q = np.ascontiguousarray(Y[:nq])
        got, per = ens.decision_function(Q, return_per_subspace=True)
        _check_per(per, want[:, :nq], ratio)
        _check_scores(got, per, proba, None, None, "sum")
        wide = np.full((nq, D + 7), np.float32(123.0))
        wide[:, :D] = Q
        got_view = ens.decision_function(wide[:, :D])  # a numpy view with a row stride of d + 7
        assert np.array_equal(got_view.view(np.uint64), got.view(np.uint64))
        Qd = torch.as_tensor(wide, device="cuda")[:, :D]  # the same on the device, as the kernel sees it
        Xd = torch.as_tensor(np.hstack([X, np.zeros((n, 5), np.float32)]), device="cuda")[:, :D]
        assert Qd.stride(0) == D + 7 and Xd.stride(0) == D + 5
        out = torch.full((len(FEATS), nq + 3), -1.0, dtype=torch.float32, device="cuda")
        ens.ops.inne_scores(Qd, Xd, ens._table, 0, len(FEATS), 300, ens._state, out)
        out = out.cpu().numpy()
        assert np.array_equal(out[:, :nq].view(np.uint32), per.view(np.uint32)) and (out[:, nq:] == -1.0).all()
    per = ens.decision_function(Y, return_per_subspace=True)[1]
    assert (per[:4, 300:320] == 1.0).all() and (per[4, 300:320] == 0.0).all()  # far rows: covered by nothing
    assert (want[:4, 300:320] == 1.0).all()
    copies = ens.per_subspace_scores_[:, :40]  # exact copies of fitted rows score what those rows scored
    assert np.array_equal(per[:, 1:41].view(np.uint32), copies.view(np.uint32))


# ---- 3. bit identity -------------------------------------------------------------------------------------------------------
def test_state_and_scores_are_bit_identical_for_every_workspace_and_run():
    n, T = 700, 5
    feats = FEATS[:3] + [FEATS[4]]
    X, Y = _data(n, D, seed=81), _data(130, D, seed=82)
    runs = []
    for ws in (1 << 30, 1 << 30, 1 << 12):
        ens, _ = _fit(X, feats, T, 24, "distance", seed=6, workspace_bytes=ws)
        runs.append((ens.center_rows_, ens.center_nn_, _bits(ens.radius_sq_), _bits(ens.isolation_ratio_), ens.per_subspace_scores_,
                     ens.decision_scores_, *ens.decision_function(Y, return_per_subspace=True)))
    for other in runs[1:]:
        for a, b in zip(runs[0], other):
            assert a.dtype == b.dtype and np.array_equal(a, b)


# ---- 4. the shared tail ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("normalize", ["zscore", "robust", "minmax"])
def test_normalize_max_predict_and_predict_proba_on_inne_scores(normalize):
    import vgan_amd
    X = _planted()
    Xr, Y = np.ascontiguousarray(X[:1500]), np.ascontiguousarray(X[1400:])
    feats = [[0, 1], [0, 1, 2], [4, 7], list(range(10))]
    proba = np.array([0.4, 0.3, 0.2, 0.1])
    ens = vgan_amd.SubspaceINNE(_mask(10, feats), proba, n_estimators=17, max_samples=16, seed=1, normalize=normalize, combination="max",
                                contamination=0.05).fit(Xr)
    per = ens.per_subspace_scores_
    c, w = _check_stats(ens, normalize)
    _check_scores(ens.decision_scores_, per, proba, c, w, "max")
    assert ens.threshold_ == np.percentile(ens.decision_scores_, 95.0)
    np.testing.assert_array_equal(ens.labels_, (ens.decision_scores_ > ens.threshold_).astype(int))
    assert ens.labels_.shape == (1500,) and 0 < ens.labels_.sum() <= 75
    got, per_new = ens.decision_function(Y, return_per_subspace=True)
    assert np.array_equal(per_new[:, :100].view(np.uint32), per[:, 1400:].view(np.uint32))  # fitted rows score as at fit
    _check_scores(got, per_new, proba, c, w, "max")  # the statistics of the fit
    np.testing.assert_array_equal(ens.predict(Y), (got > ens.threshold_).astype(int))
    p = ens.predict_proba(Y)
    assert p.shape == (620, 2)
    np.testing.assert_allclose(p, restate_proba(ens.decision_scores_, got, "linear"), rtol=1e-12, atol=1e-15)


# ---- 5. the detector detects -----------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _planted_reference():
    X = _planted()
    return X, restate_inne_both(X, [X], [[0, 1]], 200, "auto", 0)


@pytest.mark.parametrize("ratio", ["squared", "distance"])
def test_planted_rows_score_above_every_inlier(ratio):
    """The restated margins: 0.974 over 0.793 ("squared"), 0.954 over 0.752 ("distance")."""
    import vgan_amd
    X, both = _planted_reference()
    (want,), state = both[ratio]
    ens = vgan_amd.SubspaceINNE(_mask(10, [[0, 1]]), [1.0], n_estimators=200, max_samples="auto", ratio=ratio, seed=0).fit(X)
    assert ens.max_samples_ == 8
    _check_state(ens, state, ratio)
    per = ens.per_subspace_scores_
    _check_per(per, want, ratio)
    print(f"{ratio}: lowest planted {per[0, 2000:].min():.3f}, highest inlier {per[0, :2000].max():.3f}")
    assert per[0, 2000:].min() > per[0, :2000].max()
    assert ens.decision_scores_[2000:].min() > ens.decision_scores_[:2000].max()


# ---- 6. through the model --------------------------------------------------------------------------------------------------
def test_vgan_outlier_ensemble_inne_end_to_end():
    import vgan_amd
    X = _planted()[:, :10]
    model = vgan_amd.VGAN_no_kl(epochs=2)
    model.fit(X)
    ens = model.outlier_ensemble(method="inne", n_neighbors=3, n_estimators=5, max_samples=16, X=X)  # n_neighbors is ignored
    assert isinstance(ens, vgan_amd.SubspaceINNE)
    S = model.subspaces.shape[0]
    feats = [np.flatnonzero(model.subspaces[s]) for s in range(S)]
    per = ens.per_subspace_scores_
    assert per.shape == (S, X.shape[0])
    (want,), state = restate_inne_both(X, [X], feats, 5, 16, 0)["squared"]
    _check_state(ens, state, "squared")
    _check_per(per, want, "squared")
    _check_scores(ens.decision_scores_, per, model.proba, None, None, "sum")
    ens = model.outlier_ensemble(method="inne", n_estimators=5, max_samples=16, normalize="minmax", X=X)
    assert ens.predict_proba(X[:50]).shape == (50, 2)
