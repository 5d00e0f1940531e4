"""Subspace outlier degree on the MI355X (csrc/outlier_sod.hip through vgan_amd.SubspaceSOD), against the float64
restatement of test_outlier_sod_cpu.py.

The kernel's neighbour lists are held to the data by check_neighbor_lists; everything after them is compared on the kernel's
own lists, so no row is left out.  Reference sets, ``n_unshared_``, ``n_relevant_`` and the relevance masks are integers and
must equal the restatement exactly (the moments are the same float64 operations in the same order, so v_f < T is the same
comparison).  The bar on a score is one float32 ulp, |got - want| <= 2^-23 |want|: the float64 value differs from the
restatement's by the square root at most and the one rounding to float32 adds at most 2^-24.  A row with r = 0 scores 0."""
import numpy as np
import pytest

import outlier_checks as oc
from test_outlier_abod_gpu import _mask, _report
from test_outlier_gpu import _planted
from test_outlier_kde_cpu import restate_sq_dists
from test_outlier_norm_gpu import _check_scores, _check_stats
from test_outlier_sod_cpu import FORMS, restate_refsets, restate_refsets_dense, restate_sod, roc_auc, tight_clusters

pytestmark = pytest.mark.gpu

ULP32 = 2.0 ** -23
SIZES = [3, 24, 45, 33, 2]  # of 64 features: narrow, mid, wide; 45 and 33 are no multiples of 4
KS = [1, 2, 8, 17, 32]
REF_SETS = [1, 2, 10, 31, 64]


@pytest.fixture(autouse=True)
def sod_class():
    import vgan_amd
    return vgan_amd.SubspaceSOD


def _check_rows(got32, want, n_rel):
    """Every row within one float32 ulp of the restatement, a row without a relevant feature exactly 0.  Returns the largest
    error in float32 ulps."""
    got = np.asarray(got32).astype(np.float64)
    assert np.asarray(got32).dtype == np.float32 and got.shape == want.shape and np.isfinite(got).all()
    assert (got[n_rel == 0] == 0).all() and (want[n_rel == 0] == 0).all()
    err = np.abs(got - want)
    bad = np.flatnonzero(err > ULP32 * np.abs(want))
    assert bad.size == 0, ("rows", bad[:8], got[bad[:4]], want[bad[:4]])
    with np.errstate(divide="ignore", invalid="ignore"):
        return float(np.where(want > 0, err / (ULP32 * np.abs(want)), 0.0).max())


def _check_subspace(ens, s, feats, Q, Xr, I_q, I_fit, R_got, per, n_rel_got, fitting, masks=True):
    """One subspace, fit (Q is Xr) or new rows, on the kernel's own lists.  Returns (largest score error in ulps, the
    number of sets that took a row sharing nothing)."""
    R_want, n_unshared = restate_refsets_dense(I_q, I_fit, ens.ref_set, fitting)
    assert R_got.dtype == np.int32 and R_got.shape == R_want.shape
    np.testing.assert_array_equal(R_got, R_want)
    want, n_rel, rel, _, _ = restate_sod(Q, Xr, feats, R_got, ens.alpha, ens.form)
    if n_rel_got is not None:
        assert n_rel_got.dtype == np.int32
        np.testing.assert_array_equal(n_rel_got, n_rel)
    if masks:
        got_mask = ens.relevant_features(s, None if fitting else Q)
        want_mask = np.zeros((Q.shape[0], Xr.shape[1]), bool)
        want_mask[:, np.sort(feats)] = rel
        assert got_mask.dtype == bool
        np.testing.assert_array_equal(got_mask, want_mask)
    return _check_rows(per, want, n_rel), n_unshared


# ---- 1. every row against the restatement on the kernel's own lists -----------------------------------------------------
@pytest.mark.parametrize("engine", oc.ENGINES)
@pytest.mark.parametrize("case", oc.ADVERSARIAL)
def test_every_row_matches_the_restatement_on_the_kernels_own_lists(case, engine, sod_class, capsys):
    """301 fitted and 131 new rows (neither a multiple of the four rows of a scoring workgroup), both engines forced on
    every width, every n_neighbors with every ref_set; form "paper" rides on the pairs (k_i, ref_set_i), "pyod" on the
    rest.  The lists are checked once per n_neighbors (they do not depend on ref_set)."""
    d, nr, nq = 64, 301, 131
    Xr, Xq = oc.adversarial_pair(case, nr, nq, d, seed=13)
    rng = np.random.default_rng(4)
    feature_lists = [np.sort(rng.choice(d, ds, replace=False)) for ds in SIZES]
    D2 = {(s, mode): restate_sq_dists(Q, Xr, f) for s, f in enumerate(feature_lists) for mode, Q in (("fit", Xr), ("new", Xq))}
    worst, zero_rows, unshared = 0.0, 0, 0
    for ki, k in enumerate(KS):
        for ri, ref_set in enumerate(REF_SETS):
            form = FORMS[ki == ri]
            ens = sod_class(_mask(d, feature_lists), np.full(len(SIZES), 0.2), n_neighbors=k, ref_set=ref_set, alpha=0.8,
                            form=form, engine=engine).fit(Xr)
            assert ens.reference_set_.shape == (len(SIZES), nr, ref_set) and ens.n_relevant_.shape == (len(SIZES), nr)
            assert ens.n_unshared_.shape == (len(SIZES),) and ens.n_unshared_.dtype.kind == "i"
            (D_fit, I_fit), (D_new, I_new) = ens.kneighbors(), ens.kneighbors(Xq)
            _, per_new = ens.decision_function(Xq, return_per_subspace=True)
            R_new = ens.reference_set(Xq)
            for s, feats in enumerate(feature_lists):
                if ri == 0:
                    oc.check_neighbor_lists(D_fit[s], I_fit[s], Xr, Xr, feats, k, True, engine, D2=D2[s, "fit"])
                    oc.check_neighbor_lists(D_new[s], I_new[s], Xq, Xr, feats, k, False, engine, D2=D2[s, "new"])
                masks = ri == ki or s == 2
                err, nu = _check_subspace(ens, s, feats, Xr, Xr, I_fit[s], I_fit[s], ens.reference_set_[s],
                                          ens.per_subspace_scores_[s], ens.n_relevant_[s], True, masks)
                assert ens.n_unshared_[s] == nu
                unshared += nu
                worst = max(worst, err)
                err, _ = _check_subspace(ens, s, feats, Xq, Xr, I_new[s], I_fit[s], R_new[s], per_new[s], None, False, masks)
                worst = max(worst, err)
                zero_rows += int((ens.n_relevant_[s] == 0).sum())
    assert unshared > 0 and zero_rows > 0  # k = 1 cannot fill 64 places; ref_set = 1 has no variance: r = 0
    _report(capsys, f"{case:14s} {engine:5s} max |got - want| / (2^-23 |want|) {worst:.3f}, {unshared} sets with a row that "
                    f"shares nothing, {zero_rows} rows with r = 0")


def test_wide_subspaces_in_several_chunks_with_both_engines(sod_class):
    """Sizes [200, 1, 17, 3] of 784 features under workspace_bytes = 60 000: several chunks, the 200-wide subspace on the
    Gram engine and processed last (processing order is not the given order), four trips of the 64 lanes."""
    d, nr, nq = 784, 301, 131
    rng = np.random.default_rng(9)
    Xr = (rng.normal(size=(nr, d)) * rng.uniform(0.05, 2.0, size=d)).astype(np.float32)
    Xq = (rng.normal(size=(nq, d)) * rng.uniform(0.05, 2.0, size=d)).astype(np.float32)
    feature_lists = [np.sort(rng.choice(d, ds, replace=False)) for ds in [200, 1, 17, 3]]
    for k, ref_set, alpha, form in [(17, 31, 0.3, "pyod"), (8, 10, 0.8, "paper")]:
        ens = sod_class(_mask(d, feature_lists), [0.4, 0.3, 0.2, 0.1], n_neighbors=k, ref_set=ref_set, alpha=alpha, form=form,
                        workspace_bytes=60_000).fit(Xr)
        assert len(ens.plan.chunks(nr, 60_000)) >= 2 and ens.plan.order[-1] == 0 and ens.plan.gram.tolist() == [False] * 3 + [True]
        (D_fit, I_fit), (D_new, I_new) = ens.kneighbors(), ens.kneighbors(Xq)
        _, per_new = ens.decision_function(Xq, return_per_subspace=True)
        R_new = ens.reference_set(Xq)
        for s, feats in enumerate(feature_lists):
            engine = "gram" if len(feats) >= 32 else "exact"
            oc.check_neighbor_lists(D_fit[s], I_fit[s], Xr, Xr, feats, k, True, engine)
            oc.check_neighbor_lists(D_new[s], I_new[s], Xq, Xr, feats, k, False, engine)
            _, nu = _check_subspace(ens, s, feats, Xr, Xr, I_fit[s], I_fit[s], ens.reference_set_[s], ens.per_subspace_scores_[s],
                                    ens.n_relevant_[s], True)
            assert ens.n_unshared_[s] == nu
            _check_subspace(ens, s, feats, Xq, Xr, I_new[s], I_fit[s], R_new[s], per_new[s], None, False)
        assert (ens.per_subspace_scores_[1] == 0).all() and (ens.n_relevant_[1] == 0).all()  # one feature: v < alpha v never holds
        assert (ens.relevant_features(0).sum(axis=1) == ens.n_relevant_[0]).all() and ens.n_relevant_[0].max() > 64


# ---- 2. edges ------------------------------------------------------------------------------------------------------------------
def test_smallest_row_counts(sod_class):
    """n = ref_set + 1: every other row is in every set.  n = n_neighbors + 1: every list is all other rows."""
    rng = np.random.default_rng(2)
    feats = [np.array([0, 2, 3]), np.arange(6)]
    for n, k, ref_set in [(65, 8, 64), (33, 32, 10), (2, 1, 1)]:
        X = rng.normal(size=(n, 6)).astype(np.float32)
        ens = sod_class(_mask(6, feats), [0.5, 0.5], n_neighbors=k, ref_set=ref_set).fit(X)
        I = ens.kneighbors()[1]
        for s, f in enumerate(feats):
            _, nu = _check_subspace(ens, s, f, X, X, I[s], I[s], ens.reference_set_[s], ens.per_subspace_scores_[s],
                                    ens.n_relevant_[s], True)
            assert ens.n_unshared_[s] == nu
            if ref_set == n - 1:
                assert (np.sort(ens.reference_set_[s], axis=1) == np.array([np.delete(np.arange(n), q) for q in range(n)])).all()
            if k == n - 1 and n > 2:
                assert ens.n_unshared_[s] == 0 and (np.sort(I[s], axis=1) == np.array([np.delete(np.arange(n), q) for q in range(n)])).all()


@pytest.mark.parametrize("n", [301, 3000])
def test_rows_that_are_all_duplicates(n, sod_class):
    """Every list is the lowest indices, so rows 0 .. k - 1 sit in n - 1 lists each (at n = 3000 a reverse list of 2999
    rows, and every fitted row touched by every query); every reference set has variance 0: r = 0 and every score exactly 0."""
    k, ref_set = 8, 10
    X = np.tile(np.array([[1.5, -2.0, 0.25, 7.0]], np.float32), (n, 1))
    ens = sod_class(_mask(4, [[0, 1, 3], [2]]), [0.5, 0.5], n_neighbors=k, ref_set=ref_set).fit(X)
    I = ens.kneighbors()[1]
    for s in range(2):
        want = np.array([[j for j in range(k + 1) if j != q][:k] for q in range(n)])
        np.testing.assert_array_equal(I[s], want)
        R_want, nu = restate_refsets_dense(I[s], I[s], ref_set, True)
        np.testing.assert_array_equal(ens.reference_set_[s], R_want)
        assert ens.n_unshared_[s] == nu == 0
    assert (ens.per_subspace_scores_ == 0).all() and (ens.n_relevant_ == 0).all() and (ens.decision_scores_ == 0).all()
    assert not ens.relevant_features(0).any()
    Y = np.vstack([X[:3], X[:2] + 1.0]).astype(np.float32)
    got, per_new = ens.decision_function(Y, return_per_subspace=True)
    assert (per_new == 0).all() and (got == 0).all()  # off the point mass too: no feature is relevant
    np.testing.assert_array_equal(ens.reference_set(Y)[0], restate_refsets_dense(ens.kneighbors(Y)[1][0], I[0], ref_set, False)[0])


def test_sets_that_take_rows_sharing_nothing_and_constant_features(sod_class):
    """40 rows, n_neighbors = 1, ref_set = 10: a row shares its one neighbour with a few rows at most, so the sets are filled
    from the rows that share nothing, lowest indices first.  Subspace 1 is two constant features: score 0."""
    rng = np.random.default_rng(3)
    X = rng.normal(size=(40, 5)).astype(np.float32)
    X[:, 3], X[:, 4] = 2.0, -1.0
    feats = [np.array([0, 1, 2]), np.array([3, 4]), np.array([0, 3])]
    ens = sod_class(_mask(5, feats), [0.5, 0.25, 0.25], n_neighbors=1, ref_set=10).fit(X)
    I = ens.kneighbors()[1]
    for s, f in enumerate(feats):
        R_loops, nu_loops = restate_refsets(I[s], I[s], 10, True)
        np.testing.assert_array_equal(ens.reference_set_[s], R_loops)
        _, nu = _check_subspace(ens, s, f, X, X, I[s], I[s], ens.reference_set_[s], ens.per_subspace_scores_[s], ens.n_relevant_[s], True)
        assert ens.n_unshared_[s] == nu == nu_loops
    assert ens.n_unshared_[0] == 40 and (ens.n_unshared_ > 0).all()
    assert (ens.per_subspace_scores_[1] == 0).all() and (ens.n_relevant_[1] == 0).all()
    # subspace 2: the constant feature has variance 0 < T, the other one is never below alpha times the mean of the two
    assert (ens.relevant_features(2)[:, 3]).all() and not ens.relevant_features(2)[:, 0].any()
    assert (ens.per_subspace_scores_[2] == 0).all() and (ens.n_relevant_[2] == 1).all()  # x_3 is the constant: distance 0


@pytest.mark.parametrize("n", [8200, 16400])
def test_every_size_of_the_count_table(n, sod_class):
    """Up to 2^13 rows the 8 KiB table runs (the cases above), up to 2^14 the 16 KiB one and beyond it the 32 KiB one, in which
    a bit of a lane's dirty mask covers two and four words.  The first 600 rows are duplicates of one another (hubs: reverse
    lists of 599 rows).  A sample of the rows against the loop restatement on the kernel's own lists."""
    rng = np.random.default_rng(n)
    X = rng.normal(size=(n, 6)).astype(np.float32)
    X[:600] = X[0]
    feats = np.array([0, 1, 2, 4])
    k, ref_set = 8, 10
    ens = sod_class(_mask(6, [feats]), [1.0], n_neighbors=k, ref_set=ref_set, alpha=0.8).fit(X)
    I = ens.kneighbors()[1][0]
    assert (np.bincount(I.ravel(), minlength=n)[:k] >= 599).all()
    rows = np.concatenate([[0, 1, 5, 599, 600, n - 1], rng.choice(n, 40, replace=False)])
    R_want, _ = restate_refsets(I[rows], I, ref_set, True, self_rows=rows)
    np.testing.assert_array_equal(ens.reference_set_[0][rows], R_want)
    want, n_rel, rel, _, _ = restate_sod(X[rows], X, feats, ens.reference_set_[0][rows], 0.8, "pyod")
    np.testing.assert_array_equal(ens.n_relevant_[0][rows], n_rel)
    _check_rows(ens.per_subspace_scores_[0][rows], want, n_rel)
    Y = np.vstack([X[:2], rng.normal(size=(30, 6)).astype(np.float32)])
    I_new = ens.kneighbors(Y)[1][0]
    R_new = ens.reference_set(Y)[0]
    np.testing.assert_array_equal(R_new, restate_refsets(I_new, I, ref_set, False)[0])
    want, n_rel, _, _, _ = restate_sod(Y, X, feats, R_new, 0.8, "pyod")
    _check_rows(ens.decision_function(Y, return_per_subspace=True)[1][0], want, n_rel)


# ---- 3. determinism ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("engine", oc.ENGINES)
def test_results_are_bit_identical_for_every_split_chunking_and_run(engine, sod_class):
    rng = np.random.default_rng(8)
    X = rng.normal(size=(901, 48)).astype(np.float32)
    X[:, 5] = rng.integers(0, 3, size=901)
    Y = rng.normal(size=(130, 48)).astype(np.float32)
    m = rng.random((9, 48)) < 0.4
    m[:, 0] = True
    m[8] = False
    m[8, 5] = True  # a subspace of point masses rides along
    p = rng.random(9)
    p /= p.sum()

    def run(mask, proba, splits, ws):
        ens = sod_class(mask, proba, n_neighbors=12, ref_set=20, alpha=0.5, engine=engine, splits=splits, workspace_bytes=ws).fit(X)
        return ens, (ens.per_subspace_scores_, ens.decision_scores_, ens.reference_set_, ens.n_relevant_, ens.n_unshared_,
                     ens.relevant_features(min(3, len(proba) - 1)), *ens.decision_function(Y, return_per_subspace=True), ens.reference_set(Y))

    first, base = run(m, p, 1, 1 << 30)
    for splits, ws in [(1, 1 << 30), (3, 1 << 30), (1, 60_000), (3, 60_000), (None, 1)]:
        ens, other = run(m, p, splits, ws)
        assert ws != 1 or len(ens.plan.chunks(901, ws)) == 9  # one chunk per subspace
        for a, b in zip(base, other):
            assert a.dtype == b.dtype and np.array_equal(a, b)
    assert (base[0][8] == 0).all()
    # a subspace fitted alone
    for s in (0, 3, 8):
        _, alone = run(m[s:s + 1], [1.0], None, 1 << 30)
        for i in (0, 2, 3, 4, 7, 8):
            assert np.array_equal(alone[i][0], base[i][s]), (s, i)
        assert np.array_equal(alone[5], base[5]) or s != 3
    # a new row scored alone is the row scored in a batch
    for i in (0, 77, 129):
        got, per = first.decision_function(Y[i:i + 1], return_per_subspace=True)
        assert got[0] == base[6][i] and np.array_equal(per[:, 0], base[7][:, i])
        assert np.array_equal(first.reference_set(Y[i:i + 1])[:, 0], base[8][:, i])


# ---- 4. the ensemble tail ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("normalize", [None, "zscore", "robust"])
@pytest.mark.parametrize("combination", ["sum", "max"])
def test_ensemble_tail_on_the_scores_the_kernels_left(normalize, combination, sod_class):
    X, _ = tight_clusters(1, n=600, m=10)
    Xr, Y = np.ascontiguousarray(X[:500]), np.ascontiguousarray(X[450:])
    rng = np.random.default_rng(0)
    mask = _mask(20, [np.arange(20)] + [np.sort(rng.choice(20, 12, replace=False)) for _ in range(3)])
    proba = np.array([0.4, 0.3, 0.2, 0.1])
    ens = sod_class(mask, proba, n_neighbors=16, ref_set=15, alpha=0.5, normalize=normalize, combination=combination,
                    contamination=0.05).fit(Xr)
    per = ens.per_subspace_scores_
    assert per.dtype == np.float32 and per.shape == (4, 500) and np.isfinite(per).all() and (per >= 0).all()
    assert ens.decision_scores_.dtype == np.float64 and ens.decision_scores_.shape == (500,)
    if normalize is None:
        assert ens.score_center_ is None and ens.score_scale_ is None
        c = w = None
    else:
        c, w = _check_stats(ens, normalize)
    _check_scores(ens.decision_scores_, per, proba, c, w, combination)
    assert ens.threshold_ == np.percentile(ens.decision_scores_, 95.0)
    np.testing.assert_array_equal(ens.labels_, (ens.decision_scores_ > ens.threshold_).astype(int))
    got, per_new = ens.decision_function(Y, return_per_subspace=True)
    assert got.shape == (160,) and per_new.dtype == np.float32 and per_new.shape == (4, 160)
    _check_scores(got, per_new, proba, c, w, combination)  # the statistics of the fit
    np.testing.assert_array_equal(ens.predict(Y), (got > ens.threshold_).astype(int))
    assert ens.predict_proba(Y).shape == (160, 2)
    # decision_function(X_train) is not decision_scores_: a row's list starts with the row itself
    again = ens.decision_function(Xr, return_per_subspace=True)[1]
    assert not np.array_equal(again, per) and (ens.kneighbors(Xr)[1][0][:, 0] == np.arange(500)).all()


# ---- 5. what it detects ----------------------------------------------------------------------------------------------------
def test_quality_bar_on_the_device(sod_class, capsys):
    """The recipe and the two bars of the CPU tier, on the device: one subspace of all 20 features,
    (n_neighbors, ref_set, alpha) = (32, 31, 0.3), mean ROC AUC over seeds 0, 1, 2 at least 0.98 and at least 0.2 above
    sklearn's LOF (k = 20) on the same rows.  A second ensemble adds random 12-feature subspaces and has to run."""
    from sklearn.neighbors import LocalOutlierFactor
    sod, lof, mixed = [], [], []
    rng = np.random.default_rng(0)
    for seed in (0, 1, 2):
        X, y = tight_clusters(seed)
        ens = sod_class(np.ones((1, 20), bool), [1.0], n_neighbors=32, ref_set=31, alpha=0.3).fit(X)
        sod.append(roc_auc(ens.decision_scores_, y))
        lof.append(roc_auc(-LocalOutlierFactor(n_neighbors=20).fit(X).negative_outlier_factor_, y))
        mask = _mask(20, [np.arange(20)] + [np.sort(rng.choice(20, 12, replace=False)) for _ in range(4)])
        more = sod_class(mask, np.full(5, 0.2), n_neighbors=32, ref_set=31, alpha=0.3, combination="max").fit(X)
        assert np.isfinite(more.decision_scores_).all() and np.array_equal(more.per_subspace_scores_[0], ens.per_subspace_scores_[0])
        mixed.append(roc_auc(more.decision_scores_, y))
        # the planted rows are judged in few features, and the feature they were moved along is among them
        assert np.median(ens.n_relevant_[0][y == 1]) <= 6
    _report(capsys, f"ROC AUC seeds 0, 1, 2: SOD {np.round(sod, 4).tolist()}, sklearn LOF {np.round(lof, 4).tolist()}, SOD with "
                    f"four random 12-feature subspaces (max) {np.round(mixed, 4).tolist()}")
    assert np.mean(sod) >= 0.98, sod
    assert np.mean(sod) >= np.mean(lof) + 0.2, (sod, lof)


# ---- 6. through the model --------------------------------------------------------------------------------------------------
def test_vgan_outlier_ensemble_sod_end_to_end(sod_class):
    import vgan_amd
    X = _planted()[:, :10]
    model = vgan_amd.VGAN_no_kl(epochs=2)
    model.fit(X)
    ens = model.outlier_ensemble(method="sod", n_neighbors=16, ref_set=12, alpha=0.5, X=X)
    assert isinstance(ens, sod_class) and (ens.n_neighbors, ens.ref_set, ens.alpha, ens.form) == (16, 12, 0.5, "pyod")
    S = model.subspaces.shape[0]
    per = ens.per_subspace_scores_
    assert per.shape == (S, X.shape[0]) and np.isfinite(per).all() and (per >= 0).all()
    assert ens.reference_set_.shape == (S, X.shape[0], 12) and ens.n_relevant_.shape == (S, X.shape[0]) and ens.n_unshared_.shape == (S,)
    _check_scores(ens.decision_scores_, per, model.proba, None, None, "sum")
    I = ens.kneighbors()[1]
    for s in range(min(S, 4)):
        feats = np.flatnonzero(model.subspaces[s])
        _check_subspace(ens, s, feats, X, X, I[s], I[s], ens.reference_set_[s], per[s], ens.n_relevant_[s], True)
        assert not ens.relevant_features(s)[:, ~model.subspaces[s].astype(bool)].any()
    assert isinstance(model.outlier_ensemble(method="knn", X=X), vgan_amd.SubspaceEnsemble)
