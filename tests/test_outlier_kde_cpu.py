"""Gaussian-KDE outlier scores, CPU tier: a float64 restatement of the KDE contract (vgan_amd/outlier.py module docstring)
pinned against sklearn's KernelDensity, bandwidth resolution and validation, and the argument checks of vgan_outlier_kde."""
import math

import numpy as np
import pytest


# ---- float64 restatement of the contract ------------------------------------------------------------------------------
def restate_sq_dists(Xq, Xr, feats):
    """float64 [nq, nr]: squared distances over the features `feats`, differences first."""
    A = np.asarray(Xq, np.float64)[:, feats]
    B = np.asarray(Xr, np.float64)[:, feats]
    D2 = np.zeros((A.shape[0], B.shape[0]))
    for f in range(A.shape[1]):
        D2 += (A[:, f, None] - B[None, :, f]) ** 2
    return D2


def restate_bandwidth(bandwidth, n, ds):
    """sklearn's KernelDensity rules (sklearn/neighbors/_kde.py) for n rows of d_s features, or the given float."""
    if bandwidth == "scott":
        return n ** (-1.0 / (ds + 4))
    if bandwidth == "silverman":
        return (n * (ds + 2) / 4.0) ** (-1.0 / (ds + 4))
    return float(bandwidth)


def restate_kde_from_sq_dists(D2, ds, h, exclude_self):
    """-log p [nq] from the squared distances: logsumexp over the reference rows, row q's own index left out when
    exclude_self (N = nr - 1)."""
    from scipy.special import logsumexp
    L = -D2 / (2.0 * h * h)
    n = D2.shape[1]
    if exclude_self:
        L = L.copy()
        np.fill_diagonal(L, -np.inf)
        n -= 1
    return -(logsumexp(L, axis=1) - math.log(n) - ds * math.log(h) - 0.5 * ds * math.log(2.0 * math.pi))


def restate_kde(Xq, Xr, feats, h, exclude_self):
    return restate_kde_from_sq_dists(restate_sq_dists(Xq, Xr, feats), len(feats), h, exclude_self)


def restate_kde_ensemble(subspaces, proba, Xtr, Xq=None, bandwidth=1.0):
    """(scores float64 [n], per-subspace scores float64 [S, n], bandwidths [S]) of Xq (None: the training set,
    leave-one-out)."""
    per, hs = [], []
    for s in range(len(subspaces)):
        feats = np.flatnonzero(subspaces[s])
        h = restate_bandwidth(bandwidth, Xtr.shape[0], len(feats))
        hs.append(h)
        per.append(restate_kde(Xtr if Xq is None else Xq, Xtr, feats, h, exclude_self=Xq is None))
    per = np.array(per)
    scores = np.zeros(per.shape[1])
    for s in range(per.shape[0]):
        scores += float(proba[s]) * per[s]
    return scores, per, np.array(hs)


def _data(n, d, seed):
    return np.random.default_rng(seed).normal(size=(n, d))


def _sklearn_kde(neighbors, bandwidth, X):
    """KernelDensity on one tree leaf, so that every kernel term is evaluated: with the default leaf size its node bounds
    prune far nodes even at rtol = 0, which moves outlying rows' log densities by up to ~1e-3."""
    return neighbors.KernelDensity(bandwidth=bandwidth, leaf_size=len(X) + 1).fit(X)


# ---- the restatement against sklearn --------------------------------------------------------------------------------
@pytest.mark.parametrize("bandwidth", [0.7, "scott", "silverman"])
@pytest.mark.parametrize("ds", [1, 3, 12])
def test_restated_kde_matches_sklearn(bandwidth, ds):
    neighbors = pytest.importorskip("sklearn.neighbors")
    X, Y = _data(300, 12, 0), _data(50, 12, 1) * 1.5
    feats = np.sort(np.random.default_rng(ds).choice(12, ds, replace=False))
    kd = _sklearn_kde(neighbors, bandwidth, X[:, feats])
    h = restate_bandwidth(bandwidth, 300, ds)
    assert kd.bandwidth_ == pytest.approx(h, rel=1e-14)
    np.testing.assert_allclose(restate_kde(Y, X, feats, h, exclude_self=False), -kd.score_samples(Y[:, feats]), rtol=1e-10)


def test_restated_kde_survives_a_bandwidth_where_plain_exp_underflows():
    neighbors = pytest.importorskip("sklearn.neighbors")
    X, Y = _data(200, 12, 2), _data(20, 12, 3) * 3.0
    feats, h = np.arange(12), 0.02
    D2 = restate_sq_dists(Y, X, feats)
    with np.errstate(divide="ignore"):
        assert np.isneginf(np.log(np.exp(-D2 / (2 * h * h)).sum(axis=1))).all()  # the plain sum is 0 in float64
    got = restate_kde(Y, X, feats, h, exclude_self=False)
    assert np.isfinite(got).all()
    np.testing.assert_allclose(got, -_sklearn_kde(neighbors, h, X).score_samples(Y), rtol=1e-10)


@pytest.mark.parametrize("bandwidth", [0.5, "scott"])
def test_restated_leave_one_out_matches_sklearn_refits_without_the_row(bandwidth):
    neighbors = pytest.importorskip("sklearn.neighbors")
    X = _data(150, 5, 4)
    X[17] = X[3]  # an exact duplicate stays in the sum
    feats = np.array([0, 2, 3])
    h = restate_bandwidth(bandwidth, 150, 3)  # the numeric bandwidth of the full set, also for the refits
    loo = restate_kde(X, X, feats, h, exclude_self=True)
    for q in [0, 3, 17, 80, 149]:
        rest = np.delete(X, q, axis=0)[:, feats]
        want = -_sklearn_kde(neighbors, h, rest).score_samples(X[q:q + 1, feats])[0]
        assert loo[q] == pytest.approx(want, rel=1e-10)


# ---- bandwidth resolution, validation, row limits -------------------------------------------------------------------
def test_bandwidth_rules_per_subspace():
    from vgan_amd.outlier import resolve_bandwidth
    dims = np.array([1, 3, 12, 784])
    np.testing.assert_allclose(resolve_bandwidth("scott", 1000, dims), 1000.0 ** (-1.0 / (dims + 4)), rtol=1e-15)
    np.testing.assert_allclose(resolve_bandwidth("silverman", 1000, dims), (1000.0 * (dims + 2) / 4) ** (-1.0 / (dims + 4)),
                               rtol=1e-15)
    got = resolve_bandwidth(0.3, 1000, dims)
    assert got.dtype == np.float64 and got.tolist() == [0.3] * 4
    for ds in [1, 3, 12]:
        for rule in ["scott", "silverman"]:
            assert resolve_bandwidth(rule, 1000, [ds])[0] == pytest.approx(restate_bandwidth(rule, 1000, ds), rel=1e-15)


@pytest.mark.parametrize("bad", [0, 0.0, -1, -1.0, float("nan"), float("inf"), "foo", "Scott", None, True, [1.0]])
def test_bad_bandwidths_are_value_errors_before_device_work(bad):
    import vgan_amd
    from vgan_amd.outlier import check_bandwidth
    with pytest.raises(ValueError, match="bandwidth"):
        check_bandwidth(bad)
    with pytest.raises(ValueError, match="bandwidth"):
        vgan_amd.SubspaceEnsemble(np.ones((1, 3), bool), [1.0], method="kde", bandwidth=bad)


def test_good_bandwidths_pass_validation():
    from vgan_amd.outlier import check_bandwidth
    assert check_bandwidth(1) == 1.0 and check_bandwidth(np.float32(0.25)) == 0.25
    assert check_bandwidth("scott") == "scott" and check_bandwidth("silverman") == "silverman"


def test_kde_row_limits():
    from vgan_amd.outlier import KDE_MAX_ROWS, check_kde_rows
    assert KDE_MAX_ROWS == 2 ** 23 - 1
    check_kde_rows(2, exclude_self=True)
    check_kde_rows(1, exclude_self=False)
    check_kde_rows(KDE_MAX_ROWS, exclude_self=True)
    with pytest.raises(ValueError, match="at least 2"):
        check_kde_rows(1, exclude_self=True)
    with pytest.raises(ValueError, match="at least 1"):
        check_kde_rows(0, exclude_self=False)
    with pytest.raises(ValueError, match="at most"):
        check_kde_rows(KDE_MAX_ROWS + 1, exclude_self=False)


def test_unknown_methods_are_still_value_errors():
    import vgan_amd
    for method in ["iforest", "KDE", "density"]:
        with pytest.raises(ValueError, match="'knn', 'lof' or 'kde'"):
            vgan_amd.SubspaceEnsemble(np.ones((1, 3), bool), [1.0], method=method)


# ---- C ABI: argument checks without a GPU ------------------------------------------------------------------------------
def test_kde_entry_rejects_bad_arguments_without_gpu():
    import ctypes
    import vgan_amd
    lib = vgan_amd.lib.load()
    null = None
    buf = ctypes.create_string_buffer(256)
    p = ctypes.cast(ctypes.addressof(buf) + (-ctypes.addressof(buf)) % 16, ctypes.c_void_p)  # 16-byte aligned, never read

    def rejected(rc):
        msg = lib.vgan_last_error()
        return rc == 1 and b"bad argument" in msg and b"outlier.hip" in msg

    def kde(Pq=p, sq_q=p, nq=10, Pr=p, sq_r=p, nr=10, feat_off=p, col_off=p, first=0, count=1, bw=p, excl=0, engine=0, splits=1,
            pivot=p, acc=p, score=p, score_row=null, ld=10):
        return lib.vgan_outlier_kde(Pq, sq_q, nq, Pr, sq_r, nr, feat_off, col_off, first, count, bw, excl, engine, splits, pivot,
                                    acc, score, score_row, ld, null)

    for name in ["Pq", "Pr", "feat_off", "col_off", "bw", "pivot", "acc", "score"]:
        assert rejected(kde(**{name: null})), name
    assert rejected(kde(engine=2))  # unknown engine
    assert rejected(kde(engine=1, sq_q=null))  # gram without norms
    assert rejected(kde(excl=1, nr=5))  # self excluded, nq != nr
    assert rejected(kde(excl=1, nq=1, nr=1, ld=1))  # fit needs 2 reference rows
    assert rejected(kde(nr=2 ** 23))  # over VGAN_OUTLIER_KDE_MAX_ROWS
    assert rejected(kde(ld=9))  # ld_score < nq
    assert rejected(kde(count=0))
    assert rejected(kde(splits=0))
    assert rejected(kde(nq=0))
