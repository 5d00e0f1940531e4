"""Outlier scoring over subspaces on the MI355X (csrc/outlier.hip through vgan_amd.SubspaceEnsemble), against the float64
restatement in test_outlier_cpu.py."""
import numpy as np
import pytest

from outlier_checks import check_neighbor_lists
from test_outlier_cpu import restate_ensemble, restate_neighbors

pytestmark = pytest.mark.gpu

EPS32 = 2.0 ** -24


def _single(d, feats):
    m = np.zeros((1, d), bool)
    m[0, feats] = True
    return m


def _clear_rows(dist, k, gram_tol=None):
    """Rows whose k-th and (k+1)-th restated distances differ by more than 1e-4 relative (and, for the Gram engine, by more
    than its cancellation bound on squared distances, given per row)."""
    dk, dk1 = dist[:, k - 1], dist[:, k]
    ok = (dk1 - dk) > 1e-4 * dk1
    if gram_tol is not None:
        ok &= (dk1 ** 2 - dk ** 2) > gram_tol
    return ok


@pytest.fixture(scope="module")
def data():
    rng = np.random.default_rng(11)
    return rng.normal(size=(777, 784)).astype(np.float32), rng.normal(size=(1000, 784)).astype(np.float32)


@pytest.mark.parametrize("engine", ["exact", "gram"])
@pytest.mark.parametrize("ds", [1, 3, 17, 200, 784])
def test_neighbor_lists_match_the_restatement(data, engine, ds):
    import vgan_amd
    Xr, Xq = data
    feats = np.sort(np.random.default_rng(ds).choice(784, ds, replace=False))
    A = Xr[:, feats].astype(np.float64)
    c = A.mean(axis=0)
    rmax = ((A - c) ** 2).sum(axis=1).max()
    for k in [1, 5, 20, 32]:
        ens = vgan_amd.SubspaceEnsemble(_single(784, feats), [1.0], n_neighbors=k, engine=engine).fit(Xr)
        for Q, excl in [(None, True), (Xq, False)]:
            D, I = ens.kneighbors(Q)
            assert D.shape == (1, 777 if Q is None else 1000, k) and D.dtype == np.float32 and I.dtype == np.int32
            rd, ri = restate_neighbors(Xr if Q is None else Q, Xr, feats, k, exclude_self=excl)
            tol = None
            if engine == "gram":
                qn = (((Xr if Q is None else Q)[:, feats].astype(np.float64) - c) ** 2).sum(axis=1)
                tol = 64 * EPS32 * np.sqrt(ds) * (qn + rmax)
            ok = _clear_rows(rd, k, tol)
            if engine == "exact":
                assert ok.mean() > 0.5, (k, ok.mean())  # high d_s concentrates distances: fewer clear gaps
            assert (np.sort(I[0][ok], axis=1) == np.sort(ri[ok, :k], axis=1)).all(), (k, excl)
            np.testing.assert_allclose(D[0][ok], rd[ok, :k], rtol=1e-5, atol=1e-30)
            assert (np.diff(D[0], axis=1) >= 0).all()
            if excl:
                assert not (I[0] == np.arange(777)[:, None]).any()
            check_neighbor_lists(D[0], I[0], Xr if Q is None else Q, Xr, feats, k, excl, engine)  # every row, no filter


@pytest.mark.parametrize("engine", ["exact", "gram"])
def test_duplicates_give_zero_distance_and_the_lower_index_first(engine):
    import vgan_amd
    rng = np.random.default_rng(3)
    X = rng.integers(-3, 4, size=(300, 4)).astype(np.float32)  # integer grid: exact ties everywhere
    X[[40, 90, 150]] = X[7]
    ens = vgan_amd.SubspaceEnsemble(np.ones((1, 4), bool), [1.0], n_neighbors=5, engine=engine).fit(X)
    D, I = ens.kneighbors()
    assert D[0, 7, :3].tolist() == [0.0, 0.0, 0.0] and I[0, 7, :3].tolist() == [40, 90, 150]
    assert I[0, 40, :3].tolist() == [7, 90, 150]
    rd, ri = restate_neighbors(X, X, np.arange(4), 5, exclude_self=True)
    np.testing.assert_array_equal(D[0], rd[:, :5].astype(np.float32))
    if engine == "exact":  # the exact engine sees the ties as ties: (distance, index) order throughout
        np.testing.assert_array_equal(I[0], ri[:, :5])
    D, I = ens.kneighbors(X[:20])
    assert D[0, 7, :4].tolist() == [0.0] * 4 and I[0, 7, :4].tolist() == [7, 40, 90, 150]


def test_lof_with_duplicates_matches_the_restatement():
    import vgan_amd
    rng = np.random.default_rng(4)
    X = rng.normal(size=(400, 3)).astype(np.float32)
    X[200:260] = X[0]  # many copies: k-distances of 0, lrd of 1e10
    X[300:303] = X[5]
    Y = np.vstack([X[:10], rng.normal(size=(30, 3)).astype(np.float32)])
    m = np.array([[True, True, False], [False, True, True], [True, True, True]])
    p = np.array([0.5, 0.3, 0.2])
    ens = vgan_amd.SubspaceEnsemble(m, p, method="lof", n_neighbors=8).fit(X)
    want, want_per = restate_ensemble(m, p, X.astype(np.float64), method="lof", k=8)
    np.testing.assert_allclose(ens.decision_scores_, want, rtol=1e-5)
    got, per = ens.decision_function(Y, return_per_subspace=True)
    want, want_per = restate_ensemble(m, p, X.astype(np.float64), Y.astype(np.float64), method="lof", k=8)
    np.testing.assert_allclose(got, want, rtol=1e-5)
    np.testing.assert_allclose(per, want_per, rtol=1e-5)


@pytest.mark.parametrize("engine", ["exact", "gram"])
def test_output_is_bit_identical_for_every_split_and_chunking(engine):
    import vgan_amd
    rng = np.random.default_rng(8)
    X = rng.normal(size=(900, 48)).astype(np.float32)
    Y = rng.normal(size=(130, 48)).astype(np.float32)
    m = rng.random((9, 48)) < 0.4
    m[:, 0] = True
    p = rng.random(9)
    p /= p.sum()
    runs = []
    for splits, ws in [(1, 1 << 30), (3, 1 << 30), (7, 1 << 30), (1, 1), (7, 60_000)]:
        ens = vgan_amd.SubspaceEnsemble(m, p, method="lof", n_neighbors=12, engine=engine, splits=splits, workspace_bytes=ws).fit(X)
        runs.append((ens.decision_scores_, ens.per_subspace_scores_, *ens.decision_function(Y, return_per_subspace=True),
                     *ens.kneighbors(), *ens.kneighbors(Y)))
    for other in runs[1:]:
        for a, b in zip(runs[0], other):
            assert np.array_equal(a, b)


def _planted():
    rng = np.random.default_rng(21)
    x0 = rng.uniform(-2.0, 2.0, size=2000)
    inl = rng.normal(size=(2000, 10))
    inl[:, 0], inl[:, 1] = x0, x0 + 0.05 * rng.normal(size=2000)
    a = rng.uniform(0.7, 1.8, size=20) * rng.choice([-1, 1], size=20)
    out = rng.normal(size=(20, 10))
    out[:, 0], out[:, 1] = a, -a  # marginals look normal, the pair breaks the correlation
    return np.vstack([inl, out]).astype(np.float32)


@pytest.mark.parametrize("method,k", [("knn", 5), ("lof", 20)])
def test_planted_outliers_rank_above_every_inlier(method, k):
    import vgan_amd
    X = _planted()
    m = np.zeros((3, 10), bool)
    m[0, [0, 1]] = True
    m[1, [0, 1, 2]] = True
    m[2, [4, 7]] = True
    p = np.array([0.8, 0.15, 0.05])
    ens = vgan_amd.SubspaceEnsemble(m[:1], [1.0], method=method, n_neighbors=k).fit(X)
    s = ens.decision_scores_
    assert s.dtype == np.float64 and s.shape == (2020,)
    assert s[2000:].min() > s[:2000].max()
    want, _ = restate_ensemble(m[:1], [1.0], X.astype(np.float64), method=method, k=k)
    np.testing.assert_allclose(s, want, rtol=1e-5)
    for knn_method in (["largest", "mean", "median"] if method == "knn" else ["largest"]):
        ens = vgan_amd.SubspaceEnsemble(m, p, method=method, n_neighbors=k, knn_method=knn_method).fit(X[:1500])
        got, per = ens.decision_function(X, return_per_subspace=True)
        want, want_per = restate_ensemble(m, p, X[:1500].astype(np.float64), X.astype(np.float64), method=method, k=k,
                                          knn_method=knn_method)
        np.testing.assert_allclose(got, want, rtol=1e-5)
        np.testing.assert_allclose(per, want_per, rtol=1e-5)
        assert per.dtype == np.float32 and per.shape == (3, 2020)


def test_row_count_checks():
    import vgan_amd
    X = np.random.default_rng(1).normal(size=(6, 3)).astype(np.float32)
    with pytest.raises(ValueError, match="n_neighbors \\+ 1"):
        vgan_amd.SubspaceEnsemble(np.ones((1, 3), bool), [1.0], n_neighbors=6).fit(X)
    with pytest.raises(RuntimeError, match="not fitted"):
        vgan_amd.SubspaceEnsemble(np.ones((1, 3), bool), [1.0]).decision_function(X)


def test_vgan_outlier_ensemble_end_to_end():
    import vgan_amd
    X = _planted()[:, :10]
    model = vgan_amd.VGAN_no_kl(epochs=5)
    model.fit(X)
    ens = model.outlier_ensemble(method="knn", n_neighbors=5, subspace_count=200, X=X)
    assert model.subspaces.shape[1] == 10 and np.isclose(model.proba.sum(), 1.0)
    want, _ = restate_ensemble(model.subspaces, model.proba, X.astype(np.float64), method="knn", k=5)
    np.testing.assert_allclose(ens.decision_scores_, want, rtol=1e-5)
    lof = model.outlier_ensemble(method="lof", n_neighbors=10).fit(X)
    want, _ = restate_ensemble(model.subspaces, model.proba, X.astype(np.float64), method="lof", k=10)
    np.testing.assert_allclose(lof.decision_scores_, want, rtol=1e-5)
