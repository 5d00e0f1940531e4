"""Gaussian-KDE outlier scores on the MI355X (csrc/outlier.hip through vgan_amd.SubspaceEnsemble(method="kde")), against the
float64 restatement in test_outlier_kde_cpu.py."""
import numpy as np
import pytest

from outlier_checks import kde_tolerance as _tolerance
from test_outlier_cpu import restate_neighbors
from test_outlier_gpu import _planted
from test_outlier_kde_cpu import (restate_bandwidth, restate_kde, restate_kde_ensemble, restate_kde_from_sq_dists,
                                  restate_sq_dists)

pytestmark = pytest.mark.gpu

EPS32 = 2.0 ** -24


def _single(d, feats):
    m = np.zeros((1, d), bool)
    m[0, feats] = True
    return m


_D2 = {}


@pytest.fixture(scope="module")
def data():
    rng = np.random.default_rng(11)
    return rng.normal(size=(777, 784)).astype(np.float32), rng.normal(size=(1000, 784)).astype(np.float32)


def _sq_dists(data, ds):
    if ds not in _D2:
        Xr, Xq = data
        feats = np.sort(np.random.default_rng(ds).choice(784, ds, replace=False))
        _D2[ds] = (feats, restate_sq_dists(Xr, Xr, feats), restate_sq_dists(Xq, Xr, feats))
    return _D2[ds]


@pytest.mark.parametrize("engine", ["exact", "gram"])
@pytest.mark.parametrize("ds", [1, 3, 17, 200, 784])
@pytest.mark.parametrize("bandwidth", [1.0, "scott", "silverman", 0.05])
def test_kde_scores_match_the_restatement(data, engine, ds, bandwidth):
    import vgan_amd
    Xr, Xq = data
    feats, D2_fit, D2_new = _sq_dists(data, ds)
    h = restate_bandwidth(bandwidth, 777, ds)
    ens = vgan_amd.SubspaceEnsemble(_single(784, feats), [1.0], method="kde", bandwidth=bandwidth, engine=engine).fit(Xr)
    assert ens.bandwidth_.dtype == np.float64 and ens.bandwidth_.shape == (1,)
    assert ens.bandwidth_[0] == pytest.approx(h, rel=1e-15)
    A = Xr[:, feats].astype(np.float64)
    c = A.mean(axis=0)
    rmax = ((A - c) ** 2).sum(axis=1).max()
    got_new, per_new = ens.decision_function(Xq, return_per_subspace=True)
    for got, Q, D2, excl in [(ens.decision_scores_, Xr, D2_fit, True), (got_new, Xq, D2_new, False)]:
        want = restate_kde_from_sq_dists(D2, ds, h, excl)
        assert got.dtype == np.float64 and got.shape == want.shape
        assert np.isfinite(got).all()  # h = 1 at d_s = 784: every plain exp underflows in float32
        d2_abs = None
        if engine == "gram":
            qn = ((Q[:, feats].astype(np.float64) - c) ** 2).sum(axis=1)
            d2_abs = 64 * EPS32 * np.sqrt(ds) * (qn + rmax)
        tol = _tolerance(D2, want, ds, h, excl, engine, d2_abs)
        err = np.abs(got - want)
        assert (err <= tol).all(), (float((err / tol).max()), float(np.abs(got - want).max()))
    assert per_new.dtype == np.float32 and per_new.shape == (1, 1000)
    np.testing.assert_array_equal(per_new[0], got_new.astype(np.float32))


@pytest.mark.parametrize("engine", ["exact", "gram"])
def test_kde_output_is_bit_identical_for_every_split_and_chunking(engine):
    import vgan_amd
    rng = np.random.default_rng(8)
    X = rng.normal(size=(900, 48)).astype(np.float32)
    Y = rng.normal(size=(130, 48)).astype(np.float32)
    m = rng.random((9, 48)) < 0.4
    m[:, 0] = True
    p = rng.random(9)
    p /= p.sum()
    for bandwidth in [0.3, "scott"]:
        runs = []
        for splits in [1, 3, 7]:
            for ws in [1 << 30, 1, 60_000]:
                ens = vgan_amd.SubspaceEnsemble(m, p, method="kde", bandwidth=bandwidth, engine=engine, splits=splits,
                                                workspace_bytes=ws).fit(X)
                runs.append((ens.decision_scores_, ens.per_subspace_scores_, ens.decision_function(Y),
                             *ens.decision_function(Y, return_per_subspace=True)))
        for other in runs[1:]:
            for a, b in zip(runs[0], other):
                assert np.array_equal(a, b)
        want, want_per, _ = restate_kde_ensemble(m, p, X.astype(np.float64), bandwidth=bandwidth)
        np.testing.assert_allclose(runs[0][0], want, rtol=1e-5)
        np.testing.assert_allclose(runs[0][1], want_per, rtol=1e-5)


@pytest.mark.parametrize("engine", ["exact", "gram"])
def test_kde_duplicates_stay_in_the_sum_and_do_not_depend_on_splits(engine):
    import vgan_amd
    rng = np.random.default_rng(3)
    X = rng.integers(-3, 4, size=(300, 4)).astype(np.float32)  # integer grid: exact ties and duplicates everywhere
    X[[40, 90, 150]] = X[7]
    feats = np.arange(4)
    D2_fit, D2_new = restate_sq_dists(X, X, feats), restate_sq_dists(X[:20], X, feats)
    qn = ((X.astype(np.float64) - X.mean(axis=0, dtype=np.float64)) ** 2).sum(axis=1)
    d2_abs = 64 * EPS32 * 2.0 * (qn + qn.max())  # the Gram engine's cancellation bound: its d2 of a duplicate need not be 0
    for h in [1.0, 0.05]:
        want_fit = restate_kde_from_sq_dists(D2_fit, 4, h, exclude_self=True)
        want_new = restate_kde_from_sq_dists(D2_new, 4, h, exclude_self=False)
        tol_fit = _tolerance(D2_fit, want_fit, 4, h, True, engine, d2_abs)
        tol_new = _tolerance(D2_new, want_new, 4, h, False, engine, d2_abs[:20])
        runs = []
        for splits in [1, 3, 7]:
            ens = vgan_amd.SubspaceEnsemble(np.ones((1, 4), bool), [1.0], method="kde", bandwidth=h, engine=engine,
                                            splits=splits).fit(X)
            runs.append((ens.decision_scores_, ens.decision_function(X[:20])))
            assert (np.abs(runs[-1][0] - want_fit) <= tol_fit).all()
            assert (np.abs(runs[-1][1] - want_new) <= tol_new).all()
        for other in runs[1:]:
            assert np.array_equal(runs[0][0], other[0]) and np.array_equal(runs[0][1], other[1])
        if engine == "exact" and h == 0.05:
            # the exact engine's d2 of a copy is 0: the three copies of row 7 left when row 7 itself is excluded decide
            # its density, the next rows (d2 >= 1) add terms of e^-200
            dup = np.array([7, 40, 90, 150])
            assert (runs[0][0][dup] == runs[0][0][7]).all()
            assert runs[0][0][7] == pytest.approx(-(np.log(3 / 299) - 4 * np.log(h) - 2 * np.log(2 * np.pi)), rel=1e-6)


def test_kde_planted_outliers_rank_above_every_inlier():
    import vgan_amd
    X = _planted()
    m = np.zeros((1, 10), bool)
    m[0, [0, 1]] = True
    ens = vgan_amd.SubspaceEnsemble(m, [1.0], method="kde", bandwidth="scott").fit(X)
    s = ens.decision_scores_
    assert s.dtype == np.float64 and s.shape == (2020,)
    assert s[2000:].min() > s[:2000].max()
    want, _, hs = restate_kde_ensemble(m, [1.0], X.astype(np.float64), bandwidth="scott")
    np.testing.assert_allclose(s, want, rtol=1e-5)
    np.testing.assert_allclose(ens.bandwidth_, hs, rtol=1e-15)


def test_kde_bandwidths_follow_the_given_subspace_order_and_kneighbors_still_works():
    import vgan_amd
    X = _planted()[:600]
    m = np.zeros((3, 10), bool)
    m[0, :] = True  # 10 features
    m[1, [0, 1]] = True
    m[2, :5] = True
    p = np.array([0.2, 0.5, 0.3])
    ens = vgan_amd.SubspaceEnsemble(m, p, method="kde", bandwidth="silverman", engine="exact").fit(X)
    np.testing.assert_allclose(ens.bandwidth_, [restate_bandwidth("silverman", 600, d) for d in [10, 2, 5]], rtol=1e-15)
    want, want_per, _ = restate_kde_ensemble(m, p, X.astype(np.float64), bandwidth="silverman")
    np.testing.assert_allclose(ens.decision_scores_, want, rtol=1e-5)
    np.testing.assert_allclose(ens.per_subspace_scores_, want_per, rtol=1e-5)
    D, I = ens.kneighbors()
    rd, ri = restate_neighbors(X, X, np.flatnonzero(m[1]), 5, exclude_self=True)
    assert D.shape == (3, 600, 5) and not (I[1] == np.arange(600)[:, None]).any()
    np.testing.assert_allclose(D[1], rd[:, :5], rtol=1e-5)


def test_kde_row_count_checks():
    import vgan_amd
    X = np.random.default_rng(1).normal(size=(2, 3)).astype(np.float32)
    with pytest.raises(ValueError, match="at least 2"):
        vgan_amd.SubspaceEnsemble(np.ones((1, 3), bool), [1.0], method="kde").fit(X[:1])
    ens = vgan_amd.SubspaceEnsemble(np.ones((1, 3), bool), [1.0], method="kde", bandwidth=0.5).fit(X)  # N = 1 each
    want = restate_kde(X, X, np.arange(3), 0.5, exclude_self=True)
    np.testing.assert_allclose(ens.decision_scores_, want, rtol=1e-5)


def test_vgan_outlier_ensemble_kde_end_to_end():
    import vgan_amd
    X = _planted()[:, :10]
    model = vgan_amd.VGAN_no_kl(epochs=5)
    model.fit(X)
    ens = model.outlier_ensemble(method="kde", bandwidth="scott", subspace_count=200, X=X)
    assert model.subspaces.shape[1] == 10 and np.isclose(model.proba.sum(), 1.0)
    want, want_per, hs = restate_kde_ensemble(model.subspaces, model.proba, X.astype(np.float64), bandwidth="scott")
    np.testing.assert_allclose(ens.bandwidth_, hs, rtol=1e-15)
    np.testing.assert_allclose(ens.decision_scores_, want, rtol=1e-5)
    np.testing.assert_allclose(ens.per_subspace_scores_, want_per, rtol=1e-5)
