"""Score normalisation, combination rules and decisions of the outlier ensemble on the MI355X (csrc/outlier_norm.hip
through vgan_amd.SubspaceEnsemble(normalize=..., combination=..., contamination=...)).

The reference of every comparison is the float64 restatement of test_outlier_norm_cpu.py applied to the raw
per_subspace_scores_ the same ensemble returned (float32: exactly what the kernels read), never a second run of the
code under test.  Bars: order statistics (robust / minmax centres) exact, their scales rtol 1e-14; z-score centre within
1e-12 mean(|x|) and scale rtol 1e-12 (a float64 sum of n <= 1000 terms in any order is within (n - 1) 2^-53 < 1.2e-13
relative of the sum of absolute values); "sum" scores atol 1e-12 sum_s p_s |t_s| per row, "max" scores rtol 1e-14.
The scores of a "zscore" ensemble are restated from the centre / scale it published (held to the restatement by the
statistics test): a 1e-14 bar on (x - c) / w only has a meaning for the same c and w.  Robust and minmax scores are
restated from the restated statistics."""
import numpy as np
import pytest

from test_outlier_norm_cpu import (planted_band, planted_band_subspaces, restate_combine, restate_proba, restate_stats,
                                   restate_threshold, restate_transform, separation)

pytestmark = pytest.mark.gpu

NORMS = ["zscore", "robust", "minmax"]
DETECTORS = {"knn": dict(n_neighbors=5), "lof": dict(n_neighbors=5), "kde": dict(bandwidth="scott")}


def _mask(d, sizes, seed=0):
    rng = np.random.default_rng(seed)
    m = np.zeros((len(sizes), d), bool)
    for s, ds in enumerate(sizes):
        m[s, rng.choice(d, ds, replace=False)] = True
    return m


def _check_stats(ens, how, per=None):
    per = ens.per_subspace_scores_ if per is None else per
    assert per.dtype == np.float32
    c, w = restate_stats(per, how)
    got_c, got_w = ens.score_center_, ens.score_scale_
    assert got_c.dtype == np.float64 and got_w.dtype == np.float64 and got_c.shape == got_w.shape == (per.shape[0],)
    if how == "zscore":
        bar = 1e-12 * np.abs(per.astype(np.float64)).mean(axis=1)
        assert (np.abs(got_c - c) <= bar).all(), (got_c - c, bar)
        np.testing.assert_allclose(got_w, w, rtol=1e-12, atol=0)
    else:
        np.testing.assert_array_equal(got_c, c)
        np.testing.assert_allclose(got_w, w, rtol=1e-14, atol=0)
    return c, w


def _reference_stats(ens, how, per):
    if how is None:
        return None, None
    if how == "zscore":
        return ens.score_center_, ens.score_scale_
    return restate_stats(per, how)


def _check_scores(got, per, proba, c, w, combination):
    want = restate_combine(per, proba, c, w, combination)
    assert got.dtype == np.float64 and got.shape == want.shape
    if combination == "max":
        np.testing.assert_allclose(got, want, rtol=1e-14, atol=0)
    else:
        bar = 1e-12 * (np.asarray(proba)[:, None] * np.abs(restate_transform(per, c, w))).sum(axis=0)
        err = np.abs(got - want)
        assert (err <= bar).all(), float((err / np.maximum(bar, 1e-300)).max())


@pytest.fixture(scope="module")
def wide():
    rng = np.random.default_rng(12)
    return {777: rng.normal(size=(777, 784)).astype(np.float32), 1000: rng.normal(size=(1000, 784)).astype(np.float32),
            "new": rng.normal(size=(130, 784)).astype(np.float32)}


@pytest.mark.parametrize("n", [777, 1000])
@pytest.mark.parametrize("normalize", NORMS)
@pytest.mark.parametrize("method", sorted(DETECTORS))
def test_statistics_and_scores_match_the_restatement(wide, method, normalize, n):
    """Subspaces of 200, 1, 17 and 3 of 784 features in one ensemble: both engines, processing order != given order, several
    chunks."""
    import vgan_amd
    mask = _mask(784, [200, 1, 17, 3], seed=n)
    proba = np.array([0.1, 0.2, 0.3, 0.4])
    X, Y = wide[n], wide["new"]
    for combination in ("sum", "max"):
        ens = vgan_amd.SubspaceEnsemble(mask, proba, method=method, normalize=normalize, combination=combination,
                                        workspace_bytes=60_000, **DETECTORS[method]).fit(X)
        assert list(ens.plan.order) != sorted(ens.plan.order) and len(ens.plan.chunks(n, 60_000)) > 2
        per = ens.per_subspace_scores_
        assert per.shape == (4, n) and np.isfinite(per).all()
        _check_stats(ens, normalize)
        c, w = _reference_stats(ens, normalize, per)
        _check_scores(ens.decision_scores_, per, proba, c, w, combination)
        got, per_new = ens.decision_function(Y, return_per_subspace=True)
        assert per_new.dtype == np.float32 and per_new.shape == (4, 130)
        _check_scores(got, per_new, proba, c, w, combination)  # the statistics of fit, not of the new rows
        np.testing.assert_array_equal(ens.decision_function(Y), got)


@pytest.mark.parametrize("method", sorted(DETECTORS))
def test_defaults_keep_the_raw_weighted_sum(wide, method):
    import vgan_amd
    mask = _mask(784, [200, 1, 17, 3], seed=5)
    proba = np.array([0.1, 0.2, 0.3, 0.4])
    ens = vgan_amd.SubspaceEnsemble(mask, proba, method=method, **DETECTORS[method]).fit(wide[777])
    assert ens.normalize is None and ens.combination == "sum" and ens.contamination == 0.1
    assert ens.score_center_ is None and ens.score_scale_ is None
    want = restate_combine(ens.per_subspace_scores_, proba, None, None, "sum")
    np.testing.assert_allclose(ens.decision_scores_, want, rtol=1e-12)
    assert ens.threshold_ == np.percentile(ens.decision_scores_, 90.0)
    np.testing.assert_array_equal(ens.labels_, (ens.decision_scores_ > ens.threshold_).astype(int))
    assert ens.labels_.shape == (777,) and ens.labels_.dtype.kind == "i" and 0 < ens.labels_.sum() <= 78
    # the raw maximum goes through the new combination entry with the identity transform
    mx = vgan_amd.SubspaceEnsemble(mask, proba, method=method, combination="max", **DETECTORS[method]).fit(wide[777])
    assert mx.score_center_ is None
    np.testing.assert_array_equal(mx.per_subspace_scores_, ens.per_subspace_scores_)
    np.testing.assert_array_equal(mx.decision_scores_, ens.per_subspace_scores_.astype(np.float64).max(axis=0))


@pytest.mark.parametrize("normalize", ["robust", "zscore"])
@pytest.mark.parametrize("engine", ["exact", "gram"])
def test_everything_is_bit_identical_for_every_split_and_chunking(engine, normalize):
    import vgan_amd
    rng = np.random.default_rng(8)
    X = rng.normal(size=(900, 48)).astype(np.float32)
    Y = rng.normal(size=(130, 48)).astype(np.float32)
    mask = _mask(48, [40, 2, 33, 5, 11], seed=2)
    proba = np.array([0.3, 0.1, 0.2, 0.25, 0.15])
    first = None
    for splits in (1, 3, 7):
        for workspace_bytes in (1 << 30, 1, 60_000):
            ens = vgan_amd.SubspaceEnsemble(mask, proba, method="knn", n_neighbors=5, engine=engine, normalize=normalize,
                                            splits=splits, workspace_bytes=workspace_bytes).fit(X)
            out = (ens.score_center_, ens.score_scale_, ens.decision_scores_, ens.decision_function(Y))
            if first is None:
                first = out
                _check_stats(ens, normalize)
                continue
            for a, b in zip(first, out):
                np.testing.assert_array_equal(a, b)


def test_ties_and_a_constant_subspace():
    import vgan_amd
    rng = np.random.default_rng(3)
    X = rng.integers(-3, 4, size=(300, 4)).astype(np.float32)  # integer grid: many equal scores
    X[[40, 90, 150]] = X[7]
    X = np.concatenate([X, np.full((300, 1), 2.5, dtype=np.float32)], axis=1)  # a constant column ...
    mask = np.zeros((3, 5), bool)
    mask[0, :4] = True
    mask[1, [0, 2]] = True
    mask[2, 4] = True  # ... and a subspace that holds only it: every score equal
    proba = np.array([0.5, 0.3, 0.2])
    Y = np.concatenate([rng.integers(-3, 4, size=(130, 4)).astype(np.float32), np.full((130, 1), 2.5, dtype=np.float32)], axis=1)
    for normalize in NORMS:
        for combination in ("sum", "max"):
            ens = vgan_amd.SubspaceEnsemble(mask, proba, method="knn", n_neighbors=5, normalize=normalize,
                                            combination=combination).fit(X)
            per = ens.per_subspace_scores_
            assert len(np.unique(per[0])) < 30 and len(np.unique(per[2])) == 1
            c, w = _check_stats(ens, normalize)
            assert ens.score_scale_[2] == 1.0 and ens.score_center_[2] == per[2, 0]
            assert (restate_transform(per, ens.score_center_, ens.score_scale_)[2] == 0.0).all()
            c, w = _reference_stats(ens, normalize, per)
            assert np.isfinite(ens.decision_scores_).all()
            _check_scores(ens.decision_scores_, per, proba, c, w, combination)
            got, per_new = ens.decision_function(Y, return_per_subspace=True)
            assert np.isfinite(got).all()
            _check_scores(got, per_new, proba, c, w, combination)
            if combination == "sum":  # the constant subspace contributes 0 everywhere
                np.testing.assert_allclose(got, restate_combine(per_new[:2], proba[:2], c[:2], w[:2], "sum"), rtol=1e-12, atol=1e-14)


def test_kde_with_negative_scores():
    """One feature, h = 0.05 on N(0, 0.1^2): most leave-one-out -log p are negative, which exercises the sign handling of
    the select keys."""
    import vgan_amd
    X = (0.1 * np.random.default_rng(11).normal(size=(777, 1))).astype(np.float32)
    for normalize in NORMS:
        ens = vgan_amd.SubspaceEnsemble(np.ones((1, 1), bool), [1.0], method="kde", bandwidth=0.05, normalize=normalize).fit(X)
        per = ens.per_subspace_scores_
        assert (per < 0).mean() > 0.8 and (per > 0).sum() > 10, ((per < 0).mean(), per.min(), per.max())
        c, w = _check_stats(ens, normalize)
        if normalize == "robust":
            assert c[0] < 0
        c, w = _reference_stats(ens, normalize, per)
        _check_scores(ens.decision_scores_, per, [1.0], c, w, "sum")


@pytest.mark.parametrize("n", [2, 3, 4, 5, 64, 65, 4096, 4097, 8192, 8193])
def test_small_even_and_odd_row_counts(n):
    import vgan_amd
    rng = np.random.default_rng(n)
    X = rng.normal(size=(n, 6)).astype(np.float32)
    mask = _mask(6, [1, 4, 2], seed=n)
    proba = np.array([0.2, 0.5, 0.3])
    k = 1 if n < 6 else 5
    for normalize in NORMS:
        ens = vgan_amd.SubspaceEnsemble(mask, proba, method="knn", n_neighbors=k, normalize=normalize).fit(X)
        per = ens.per_subspace_scores_
        assert per.shape == (3, n)
        _check_stats(ens, normalize)
        c, w = _reference_stats(ens, normalize, per)
        _check_scores(ens.decision_scores_, per, proba, c, w, "sum")


def test_planted_band_is_found_once_the_scores_are_normalised():
    """planted_band(seed=6): the restatement on sklearn's distances gives min(planted) / max(inlier) = 0.92 for the raw sum
    and 0.67 for the raw max; z-score / robust 2.34 / 3.06 under "sum" and 3.02 / 3.00 under "max"."""
    import vgan_amd
    X = planted_band(seed=6)
    mask, p = planted_band_subspaces(seed=6)
    Y = np.random.default_rng(60).normal(size=(130, 30)).astype(np.float32)
    Y[:5, 0] = [1.5, -1.5, 2.0, -2.0, 1.0]
    Y[:5, 1] = -Y[:5, 0]  # a few fresh rows further off the band than the planted ones
    raw = vgan_amd.SubspaceEnsemble(mask, p, method="knn", n_neighbors=5).fit(X)
    assert separation(raw.decision_scores_) < 1.0  # at least one inlier outranks a planted row
    assert separation(vgan_amd.SubspaceEnsemble(mask, p, method="knn", n_neighbors=5, combination="max").fit(X).decision_scores_) < 1.0
    for normalize in ("zscore", "robust"):
        for combination in ("sum", "max"):
            ens = vgan_amd.SubspaceEnsemble(mask, p, method="knn", n_neighbors=5, normalize=normalize, combination=combination,
                                            contamination=0.005).fit(X)
            np.testing.assert_array_equal(ens.per_subspace_scores_, raw.per_subspace_scores_)
            assert separation(ens.decision_scores_) > 1.0, (normalize, combination, separation(ens.decision_scores_))
            np.testing.assert_allclose(ens.threshold_, restate_threshold(ens.decision_scores_, 0.005), rtol=1e-13)
            assert ens.labels_.sum() == 11 and ens.labels_[2000:].all() and ens.labels_[:2000].sum() == 1
            scores = ens.decision_function(Y)
            pred = ens.predict(Y)
            assert pred.shape == (130,) and pred.dtype.kind == "i"
            np.testing.assert_array_equal(pred, (scores > ens.threshold_).astype(int))
            assert pred[:5].sum() >= 1 and pred.sum() < 130


@pytest.mark.parametrize("method", ["linear", "unify"])
def test_predict_proba_matches_the_restatement(method):
    import vgan_amd
    X = planted_band(seed=6)
    mask, p = planted_band_subspaces(seed=6)
    Y = np.random.default_rng(61).normal(size=(130, 30)).astype(np.float32)
    ens = vgan_amd.SubspaceEnsemble(mask, p, method="knn", n_neighbors=5, normalize="robust").fit(X)
    got = ens.predict_proba(Y, method=method)
    want = restate_proba(ens.decision_scores_, ens.decision_function(Y), method)
    assert got.dtype == np.float64 and got.shape == (130, 2)
    np.testing.assert_allclose(got, want, rtol=1e-12, atol=1e-15)
    np.testing.assert_allclose(got.sum(axis=1), 1.0, rtol=1e-15)
    assert got.min() >= 0.0 and got.max() <= 1.0
    if method == "linear":
        np.testing.assert_array_equal(ens.predict_proba(Y), got)  # the default method
    with pytest.raises(ValueError, match="method"):
        ens.predict_proba(Y, method="erf")


def test_vgan_outlier_ensemble_normalised_end_to_end():
    import vgan_amd
    from test_outlier_gpu import _planted
    X = _planted()[:, :10]
    model = vgan_amd.VGAN_no_kl(epochs=5)
    model.fit(X)
    ens = model.outlier_ensemble(method="lof", n_neighbors=20, normalize="robust", combination="max", subspace_count=200, X=X)
    assert ens.normalize == "robust" and ens.combination == "max"
    S = model.subspaces.shape[0]
    per = ens.per_subspace_scores_
    assert per.shape == (S, X.shape[0])
    c, w = _check_stats(ens, "robust")
    _check_scores(ens.decision_scores_, per, model.proba, c, w, "max")
    assert ens.labels_.sum() == (ens.decision_scores_ > np.percentile(ens.decision_scores_, 90.0)).sum()
    np.testing.assert_array_equal(ens.predict(X[:50]), (ens.decision_function(X[:50]) > ens.threshold_).astype(int))
