"""Angle-based outlier scores on the MI355X (csrc/outlier_abod.hip through vgan_amd.SubspaceABOD), against the float64
restatement of test_outlier_abod_cpu.py (itself pinned to exact arithmetic there).

The bar on a score is one float32 ulp, |got - want| <= 2^-23 |want|: the float64 arithmetic is within 1e-12 of the exact
value whatever the summation order (measured at 1.2e-14 for one order, asserted at 1e-12 on the CPU tier), and the one
rounding to float32 adds at most 2^-24, which leaves a factor of two.  Where the kernel's own neighbour lists are the
input of the restatement no row is left out; the lists themselves are held to the data by check_neighbor_lists."""
import numpy as np
import pytest

import outlier_checks as oc
from test_outlier_abod_cpu import FLT_MAX, restate_abod_ensemble, restate_abod_from_lists, restate_floor, to_score32
from test_outlier_cpu import restate_neighbors
from test_outlier_gpu import _planted
from test_outlier_kde_cpu import restate_sq_dists
from test_outlier_norm_gpu import _check_scores, _check_stats
from test_outlier_norm_cpu import restate_proba, restate_stats

pytestmark = pytest.mark.gpu

ULP32 = 2.0 ** -23


def _mask(d, feature_lists):
    m = np.zeros((len(feature_lists), d), bool)
    for s, feats in enumerate(feature_lists):
        m[s, feats] = True
    return m


def _report(capsys, line):
    with capsys.disabled():
        print("\n    " + line, end="")


def _check_rows(got32, want, floor):
    """Every row: a non-degenerate one within one float32 ulp of the restatement, a degenerate one (NaN in want) exactly
    the floor.  Returns the largest error in ulps."""
    got = np.asarray(got32).astype(np.float64)
    assert np.asarray(got32).dtype == np.float32 and got.shape == want.shape and np.isfinite(got).all()
    deg = np.isnan(want)
    assert (got[deg] == float(np.float32(floor))).all(), ("degenerate rows off the floor", np.flatnonzero(deg)[:8])
    want32 = to_score32(want).astype(np.float64)  # the clamp at the float32 range is part of the contract
    err = np.abs(got[~deg] - want32[~deg])
    bar = ULP32 * np.abs(want32[~deg])
    bad = np.flatnonzero(err > bar)
    assert (err <= bar).all(), ("rows", np.flatnonzero(~deg)[bad[:8]], got[~deg][bad[:4]], want[~deg][bad[:4]])
    with np.errstate(divide="ignore", invalid="ignore"):
        return float(np.where(bar > 0, err / bar, 0.0).max()) if err.size else 0.0


# ---- 1. every row against the restatement on the kernel's own lists -----------------------------------------------------
SIZES = [3, 24, 45, 33, 2]  # narrow, mid, wide; 45 and 33 are no multiples of 4 or of the kernel's 32-feature block


@pytest.mark.parametrize("engine", oc.ENGINES)
@pytest.mark.parametrize("case", oc.ADVERSARIAL)
def test_every_row_matches_the_restatement_on_the_kernels_own_lists(case, engine, capsys):
    """301 reference and 131 query rows (neither a multiple of the four rows of a workgroup), k at the 8 | 16 | 32 tile
    boundaries and at 2 and 3, fit and decision_function, both engines forced on every width."""
    import vgan_amd
    d, nr, nq = 100, 301, 131
    Xr, Xq = oc.adversarial_pair(case, nr, nq, d, seed=13)
    rng = np.random.default_rng(4)
    feature_lists = [np.sort(rng.choice(d, ds, replace=False)) for ds in SIZES]
    D2 = {(s, mode): restate_sq_dists(Q, Xr, f) for s, f in enumerate(feature_lists) for mode, Q in (("fit", Xr), ("new", Xq))}
    worst = 0.0
    for k in [2, 3, 8, 10, 16, 17, 31, 32]:
        ens = vgan_amd.SubspaceABOD(_mask(d, feature_lists), np.full(len(SIZES), 0.2), n_neighbors=k, engine=engine).fit(Xr)
        assert ens.score_floor_.dtype == np.float64 and ens.score_floor_.shape == (len(SIZES),)
        assert ens.n_degenerate_.shape == (len(SIZES),) and ens.n_degenerate_.dtype.kind == "i"
        _, per_new = ens.decision_function(Xq, return_per_subspace=True)
        for mode, Q, excl, per, lists in [("fit", Xr, True, ens.per_subspace_scores_, ens.kneighbors()),
                                          ("new", Xq, False, per_new, ens.kneighbors(Xq))]:
            D, I = lists
            assert per.shape == (len(SIZES), Q.shape[0]) and I.shape == (len(SIZES), Q.shape[0], k)
            for s, feats in enumerate(feature_lists):
                oc.check_neighbor_lists(D[s], I[s], Q, Xr, feats, k, excl, engine, D2=D2[s, mode])
                want = restate_abod_from_lists(Q, Xr, feats, I[s])
                assert not np.isnan(want).any()  # continuous data: no duplicates
                if k == 2:
                    assert (per[s] == 0).all()
                worst = max(worst, _check_rows(per[s], want, ens.score_floor_[s]))
                if mode == "fit":
                    assert ens.n_degenerate_[s] == 0 and ens.score_floor_[s] == float(per[s].min())
    _report(capsys, f"{case:14s} {engine:5s} max |got - want| / (2^-23 |want|) {worst:.3f}")


def test_hand_checkable_cases_on_the_device():
    """The origin among (1, 0), (0, 2), (-3, 0): -2/81 (test_three_neighbours_at_right_angles).  Distances of 1e-11:
    w of 1e22, a variance beyond the float32 range, stored as the most negative finite float32."""
    import vgan_amd
    X = np.array([[0, 0], [1, 0], [0, 2], [-3, 0]], np.float32)
    ens = vgan_amd.SubspaceABOD(np.ones((1, 2), bool), [1.0], n_neighbors=3).fit(X)
    assert abs(float(ens.per_subspace_scores_[0, 0]) + 2.0 / 81.0) <= ULP32 * 2.0 / 81.0
    assert ens.decision_scores_[0] == float(ens.per_subspace_scores_[0, 0])
    tiny = (1e-11 * np.random.default_rng(0).normal(size=(50, 3))).astype(np.float32)
    ens = vgan_amd.SubspaceABOD(np.ones((1, 3), bool), [1.0], n_neighbors=5).fit(tiny)
    want = restate_abod_from_lists(tiny, tiny, np.arange(3), ens.kneighbors()[1][0])
    assert (want < -FLT_MAX).all()
    assert (ens.per_subspace_scores_ == -np.float32(FLT_MAX)).all() and np.isfinite(ens.decision_scores_).all()
    assert ens.score_floor_[0] == -FLT_MAX and ens.n_degenerate_[0] == 0


# ---- 2. end to end against an independent restatement ----------------------------------------------------------------------
PLANTED_SUBSPACES = [[0, 1], [0, 1, 2], [4, 7]]


@pytest.mark.parametrize("k", [5, 10, 20])
@pytest.mark.parametrize("mode", ["fit", "new"])
def test_end_to_end_against_an_independent_restatement(mode, k, capsys):
    """The restatement finds its own float64 neighbours.  A row may be left out only where the neighbour set is
    legitimately open: its float64 gap d_(k+1)^2 - d_(k)^2 is within 2 tau of the exact engine's bound (sandwich_tau).
    Every other row must carry the restatement's set and its score within one float32 ulp; at most 0.1 % are left out."""
    import vgan_amd
    X = _planted()
    Xr = X if mode == "fit" else np.ascontiguousarray(X[:1500])
    mask = _mask(10, PLANTED_SUBSPACES)
    ens = vgan_amd.SubspaceABOD(mask, [0.5, 0.3, 0.2], n_neighbors=k, engine="exact").fit(Xr)
    if mode == "fit":
        per, (_, I) = ens.per_subspace_scores_, ens.kneighbors()
    else:
        per, (_, I) = ens.decision_function(X, return_per_subspace=True)[1], ens.kneighbors(X)
    left_out = 0
    for s, feats in enumerate(PLANTED_SUBSPACES):
        feats = np.array(feats)
        dist, idx = restate_neighbors(X, Xr, feats, k, exclude_self=mode == "fit")
        d2 = dist ** 2
        tau = oc.sandwich_tau("exact", X, Xr, feats, d2[:, :k])[:, k - 1]
        open_set = (d2[:, k] - d2[:, k - 1]) <= 2.0 * tau
        left_out += int(open_set.sum())
        keep = ~open_set
        assert (np.sort(I[s][keep], axis=1) == np.sort(idx[keep, :k], axis=1)).all(), (s, "another neighbour set")
        want = restate_abod_from_lists(X, Xr, feats, idx[:, :k])
        assert not np.isnan(want).any()
        got = per[s].astype(np.float64)
        assert (np.abs(got[keep] - want[keep]) <= ULP32 * np.abs(want[keep])).all(), (s, "score off the restatement")
    total = 3 * X.shape[0]
    assert left_out <= 1e-3 * total, (left_out, total)
    _report(capsys, f"{mode} k {k:2d}: {left_out} of {total} rows inside the engine's bound")


# ---- 3. the ensemble tail ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("normalize", [None, "robust"])
@pytest.mark.parametrize("combination", ["sum", "max"])
def test_ensemble_matches_the_restated_ensemble(normalize, combination):
    import vgan_amd
    X = _planted()
    Xr, Y = np.ascontiguousarray(X[:1500]), np.ascontiguousarray(X[1400:])
    mask, proba = _mask(10, PLANTED_SUBSPACES), np.array([0.5, 0.3, 0.2])
    ens = vgan_amd.SubspaceABOD(mask, proba, n_neighbors=10, normalize=normalize, combination=combination,
                                contamination=0.05, engine="exact").fit(Xr)
    want = restate_abod_ensemble(mask, proba, Xr, k=10, normalize=normalize, combination=combination)
    per = ens.per_subspace_scores_
    assert per.dtype == np.float32 and per.shape == (3, 1500) and np.isfinite(per).all()
    assert ens.decision_scores_.dtype == np.float64 and ens.decision_scores_.shape == (1500,)
    # the raw scores against the independent restatement: the rows whose neighbour set both agree on, within one ulp
    I = ens.kneighbors()[1]
    same = np.stack([(np.sort(I[s], axis=1) == np.sort(want["lists"][s][1][:, :10], axis=1)).all(axis=1) for s in range(3)])
    assert same.mean() > 0.999
    err = np.abs(per.astype(np.float64) - want["per"].astype(np.float64))
    assert (err[same] <= ULP32 * np.abs(want["per"].astype(np.float64)[same])).all()
    # the tail, at the bars of test_outlier_norm_gpu.py, on the scores the kernels left
    if normalize is None:
        assert ens.score_center_ is None and ens.score_scale_ is None
        c = w = None
    else:
        c, w = _check_stats(ens, normalize)
    _check_scores(ens.decision_scores_, per, proba, c, w, combination)
    if normalize is None:  # raw scores share a sign: the combined score of the independent restatement, to float32 accuracy
        rows = same.all(axis=0)
        np.testing.assert_allclose(ens.decision_scores_[rows], want["scores"][rows], rtol=2 * ULP32)
    assert ens.threshold_ == np.percentile(ens.decision_scores_, 95.0)
    np.testing.assert_array_equal(ens.labels_, (ens.decision_scores_ > ens.threshold_).astype(int))
    assert ens.labels_.shape == (1500,) and ens.labels_.dtype.kind == "i" and 0 < ens.labels_.sum() <= 75
    got, per_new = ens.decision_function(Y, return_per_subspace=True)
    assert got.dtype == np.float64 and got.shape == (620,) and per_new.dtype == np.float32 and per_new.shape == (3, 620)
    _check_scores(got, per_new, proba, c, w, combination)  # the statistics of the fit
    np.testing.assert_array_equal(ens.decision_function(Y), got)
    np.testing.assert_array_equal(ens.predict(Y), (got > ens.threshold_).astype(int))
    proba_new = ens.predict_proba(Y)
    assert proba_new.shape == (620, 2)
    np.testing.assert_allclose(proba_new, restate_proba(ens.decision_scores_, got, "linear"), rtol=1e-12, atol=1e-15)
    # decision_function(X_train) is not decision_scores_: every row is its own, unusable, nearest neighbour there
    again = ens.decision_function(Xr, return_per_subspace=True)[1]
    assert not np.array_equal(again, per)
    want_again = restate_abod_from_lists(Xr, Xr, np.array([0, 1]), ens.kneighbors(Xr)[1][0])
    _check_rows(again[0], want_again, ens.score_floor_[0])


# ---- 4. degenerate rows --------------------------------------------------------------------------------------------------
def _degenerate_data(k, seed):
    """Features 0 and 1 are small integers (many repeated rows), 2 .. 5 continuous.  For every j in 0 .. k a group of
    k - j + 1 copies of one point of its own: at fit each copy has k - j duplicates among its neighbours, m = j."""
    rng = np.random.default_rng(seed)
    X = rng.normal(size=(340, 6))
    X[:, :2] = rng.integers(0, 30, size=(340, 2))
    rows = 300
    for j in range(k + 1):
        X[rows:rows + k - j + 1, :2] = [100 + 10 * j, 200 - 7 * j]
        rows += k - j + 1
    X = X[:rows]
    Y = rng.normal(size=(61, 6))
    Y[:, :2] = rng.integers(0, 30, size=(61, 2))
    Y[:k + 1, :2] = X[300:300 + k + 1, :2]  # queries on the largest group: k + 1 duplicates, nothing excluded
    Y[k + 1:k + 4, :2] = X[rows - 1, :2]     # and on the single point
    return X.astype(np.float32), Y.astype(np.float32)


@pytest.mark.parametrize("engine", oc.ENGINES)
def test_degenerate_rows_take_the_floor_of_the_fit(engine):
    import vgan_amd
    k = 6
    X, Y = _degenerate_data(k, seed=5)
    feature_lists = [[0, 1], [2, 3, 4], [0, 5], [1]]
    ens = vgan_amd.SubspaceABOD(_mask(6, feature_lists), [0.4, 0.3, 0.2, 0.1], n_neighbors=k, engine=engine).fit(X)
    I = ens.kneighbors()[1]
    raw = np.array([restate_abod_from_lists(X, X, np.array(f), I[s]) for s, f in enumerate(feature_lists)])
    usable = (restate_sq_dists(X, X, np.array([0, 1]))[np.arange(len(X))[:, None], I[0]] > 0).sum(axis=1)
    assert sorted(set(usable.tolist())) == list(range(k + 1))  # m takes every value from 0 to k
    deg = np.isnan(raw)
    assert deg[0].sum() >= k + 3 and not deg[1].any() and deg[3].any()
    # the kernel's scores with NaN put back where the restatement has no pair: the floor rule, exactly
    per = ens.per_subspace_scores_
    want_per, want_floor, want_n = restate_floor(np.where(deg, np.float32(np.nan), per))
    np.testing.assert_array_equal(per, want_per)
    np.testing.assert_array_equal(ens.score_floor_, want_floor)
    np.testing.assert_array_equal(ens.n_degenerate_, want_n)
    assert (ens.score_floor_[:3] < 0).all()
    assert (per[0][usable == 2] == 0).all() and (per[0][usable == 2] > ens.score_floor_[0]).all()  # one pair: 0, not the floor
    for s, f in enumerate(feature_lists):
        _check_rows(per[s], raw[s], ens.score_floor_[s])
    assert np.isfinite(ens.decision_scores_).all() and np.isfinite(per).all()
    # new rows take the stored floor, and compute none of their own
    floor_before = ens.score_floor_.copy()
    got, per_new = ens.decision_function(Y, return_per_subspace=True)
    I_new = ens.kneighbors(Y)[1]
    raw_new = np.array([restate_abod_from_lists(Y, X, np.array(f), I_new[s]) for s, f in enumerate(feature_lists)])
    assert np.isnan(raw_new[0][:k + 1]).all() and not np.isnan(raw_new[0][k + 1:k + 4]).any()
    for s in range(len(feature_lists)):
        _check_rows(per_new[s], raw_new[s], floor_before[s])
    assert (per_new[0][:k + 1] == np.float32(floor_before[0])).all()
    assert np.isfinite(got).all() and np.array_equal(ens.score_floor_, floor_before)
    # a subspace in which every row is degenerate: floor 0, all 0
    X1 = X.copy()
    X1[:, 3] = 2.5
    one = vgan_amd.SubspaceABOD(_mask(6, [[3], [2, 4]]), [0.5, 0.5], n_neighbors=k, engine=engine, normalize="zscore").fit(X1)
    assert one.n_degenerate_.tolist() == [len(X1), 0] and one.score_floor_[0] == 0.0
    assert (one.per_subspace_scores_[0] == 0).all() and one.score_scale_[0] == 1.0 and np.isfinite(one.decision_scores_).all()
    assert (one.decision_function(X1[:9], return_per_subspace=True)[1][0] == 0).all()


# ---- 5. determinism ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("engine", oc.ENGINES)
def test_scores_are_bit_identical_for_every_split_chunking_and_run(engine):
    import vgan_amd
    rng = np.random.default_rng(8)
    X = rng.normal(size=(901, 48)).astype(np.float32)
    X[:, 5] = rng.integers(0, 3, size=901)
    Y = rng.normal(size=(130, 48)).astype(np.float32)
    m = rng.random((9, 48)) < 0.4
    m[:, 0] = True
    m[8] = False
    m[8, 5] = True  # a subspace of degenerate rows rides along
    p = rng.random(9)
    p /= p.sum()
    runs = []
    for splits, ws in [(1, 1 << 30), (1, 1 << 30), (3, 1 << 30), (7, 1 << 30), (1, 1), (7, 60_000), (None, 1 << 30)]:
        ens = vgan_amd.SubspaceABOD(m, p, n_neighbors=12, engine=engine, splits=splits, workspace_bytes=ws).fit(X)
        assert ws != 1 or len(ens.plan.chunks(901, ws)) == 9  # one chunk per subspace
        runs.append((ens.per_subspace_scores_, ens.decision_scores_, ens.score_floor_, ens.n_degenerate_,
                     *ens.decision_function(Y, return_per_subspace=True)))
    assert runs[0][3][8] == 901
    for other in runs[1:]:
        for a, b in zip(runs[0], other):
            assert a.dtype == b.dtype and np.array_equal(a, b)


# ---- 6. what it detects ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", [5, 10, 20])
def test_planted_rows_score_above_every_held_out_inlier(k, capsys):
    """The one-class setting V-GAN is used in: fit on normal rows, score new ones.  Not asserted for a fit on all 2020 rows:
    there the 20 planted rows are each other's neighbours."""
    import vgan_amd
    X = _planted()
    ens = vgan_amd.SubspaceABOD(_mask(10, [[0, 1], [0, 1, 2]]), [0.5, 0.5], n_neighbors=k).fit(X[:1500])
    _, per = ens.decision_function(X, return_per_subspace=True)
    for s in range(2):
        planted, inliers = per[s, 2000:].astype(np.float64), per[s, 1500:2000].astype(np.float64)
        assert planted.min() > inliers.max(), (s, k, planted.min(), inliers.max())
        _report(capsys, f"k {k:2d} subspace {s}: smallest planted / largest inlier score {planted.min() / inliers.max():.2e}")


# ---- 7. through the model --------------------------------------------------------------------------------------------------
def test_vgan_outlier_ensemble_abod_end_to_end():
    import vgan_amd
    X = _planted()[:, :10]
    model = vgan_amd.VGAN_no_kl(epochs=2)
    model.fit(X)
    ens = model.outlier_ensemble(method="abod", n_neighbors=10, X=X)
    assert isinstance(ens, vgan_amd.SubspaceABOD) and ens.n_neighbors == 10
    S = model.subspaces.shape[0]
    per = ens.per_subspace_scores_
    assert per.shape == (S, X.shape[0]) and np.isfinite(per).all() and (per <= 0).all() and np.isfinite(ens.decision_scores_).all()
    assert ens.score_floor_.shape == (S,) and ens.n_degenerate_.shape == (S,)
    _check_scores(ens.decision_scores_, per, model.proba, None, None, "sum")
    D, I = ens.kneighbors()
    for s in range(min(S, 4)):
        feats = np.flatnonzero(model.subspaces[s])
        want = restate_abod_from_lists(X, X, feats, I[s])
        _check_rows(per[s], want, ens.score_floor_[s])
    ens = model.outlier_ensemble(method="abod", n_neighbors=5, normalize="robust", combination="max", contamination=0.05, X=X)
    assert ens.n_neighbors == 5 and ens.normalize == "robust" and ens.combination == "max"
    c, w = _check_stats(ens, "robust")
    np.testing.assert_array_equal(c, restate_stats(ens.per_subspace_scores_, "robust")[0])
    _check_scores(ens.decision_scores_, ens.per_subspace_scores_, model.proba, c, w, "max")
    assert ens.threshold_ == np.percentile(ens.decision_scores_, 95.0)
    np.testing.assert_array_equal(ens.predict(X[:50]), (ens.decision_function(X[:50]) > ens.threshold_).astype(int))
    assert ens.predict_proba(X[:50]).shape == (50, 2)
    assert isinstance(model.outlier_ensemble(method="knn", X=X), vgan_amd.SubspaceEnsemble)
