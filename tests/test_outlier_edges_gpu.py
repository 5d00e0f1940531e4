"""The outlier kernels (csrc/outlier.hip through vgan_amd.SubspaceEnsemble) on unstandardised data, wide subspaces and the
edges of the tile machinery, every row held to the float64 restatement by the checks of outlier_checks.py (CPU tier of
those checks: test_outlier_checks_cpu.py).  Nothing is filtered: a list or score the engines' error bounds do not allow
fails on the row that carries it.  Left out on purpose: NaN / inf inputs and timing assertions."""
import functools

import numpy as np
import pytest

import outlier_checks as oc
from test_outlier_kde_cpu import restate_bandwidth, restate_sq_dists

pytestmark = pytest.mark.gpu

NR, NQ, DIM = 777, 300, 784
KNN_HOW = ["largest", "mean", "median"]


def _mask(d, feature_lists):
    m = np.zeros((len(feature_lists), d), bool)
    for s, feats in enumerate(feature_lists):
        m[s, feats] = True
    return m


def _report(capsys, line):
    with capsys.disabled():
        print("\n    " + line, end="")


def _check_detectors(make, Xr, Xq, feature_lists, engines, k, bandwidth, D2=None):
    """Every detector of the ensembles make(method=..., **kw) over the subspaces feature_lists (engine of subspace s:
    engines[s]) at fit on Xr and for the new rows Xq, every row of every subspace.  bandwidth: a float or a rule (None: no
    KDE).  D2: {(s, "fit" | "new"): restate_sq_dists} where the caller has them.  Returns the ensembles' outputs (for
    bit-identity comparisons) and the largest sandwich use of the lists."""
    S = len(feature_lists)
    modes = [("fit", Xr, True), ("new", Xq, False)]
    D2 = dict(D2 or {})
    for s, feats in enumerate(feature_lists):
        for mode, Q, _ in modes:
            if (s, mode) not in D2:
                D2[s, mode] = restate_sq_dists(Q, Xr, feats)
    out, use = [], 0.0
    # neighbour lists, and LOF restated from them
    ens = make(method="lof", n_neighbors=k).fit(Xr)
    lists = {"fit": ens.kneighbors(), "new": ens.kneighbors(Xq)}
    score = {"fit": ens.per_subspace_scores_, "new": ens.decision_function(Xq, return_per_subspace=True)[1]}
    for mode, Q, excl in modes:
        D, I = lists[mode]
        assert D.shape == I.shape == (S, Q.shape[0], k) and D.dtype == np.float32 and I.dtype == np.int32
        for s, feats in enumerate(feature_lists):
            use = max(use, oc.check_neighbor_lists(D[s], I[s], Q, Xr, feats, k, excl, engines[s], D2=D2[s, mode]))
            oc.check_lof_scores(score[mode][s], lists["fit"][0][s], lists["fit"][1][s], D[s], I[s], k)
        out += [D, I, score[mode]]
    for how in KNN_HOW:
        ens = make(method="knn", n_neighbors=k, knn_method=how).fit(Xr)
        per_new = ens.decision_function(Xq, return_per_subspace=True)[1]
        for (mode, Q, excl), per in zip(modes, [ens.per_subspace_scores_, per_new]):
            assert per.shape == (S, Q.shape[0]) and per.dtype == np.float32
            for s, feats in enumerate(feature_lists):
                oc.check_knn_scores(per[s], Q, Xr, feats, k, how, excl, engines[s], D2=D2[s, mode])
            out.append(per)
    if bandwidth is not None:
        ens = make(method="kde", bandwidth=bandwidth).fit(Xr)
        want = [restate_bandwidth(bandwidth, Xr.shape[0], len(feats)) for feats in feature_lists]
        np.testing.assert_allclose(ens.bandwidth_, want, rtol=1e-15)
        per_new = ens.decision_function(Xq, return_per_subspace=True)[1]
        for (mode, Q, excl), per in zip(modes, [ens.per_subspace_scores_, per_new]):
            for s, feats in enumerate(feature_lists):
                oc.check_kde_scores(per[s], Q, Xr, feats, float(ens.bandwidth_[s]), excl, engines[s], D2=D2[s, mode])
            out.append(per)
    return out, use


# ---- unstandardised data -----------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _wide(case, ds):
    Xr, Xq = oc.adversarial_pair(case, NR, NQ, DIM, seed=5)
    feats = np.sort(np.random.default_rng(ds).choice(DIM, ds, replace=False))
    return Xr, Xq, feats, restate_sq_dists(Xr, Xr, feats), restate_sq_dists(Xq, Xr, feats)


@pytest.mark.parametrize("engine", oc.ENGINES)
@pytest.mark.parametrize("ds", [17, 40, 200, 784])
@pytest.mark.parametrize("case", oc.ADVERSARIAL)
def test_unstandardised_data_every_row(case, ds, engine, capsys):
    """Column offsets, feature scales over six decades, low-rank structure and queries away from the reference cloud; both
    engines forced at every width.  kNN (largest, mean, median; k = 20 and 32 are the even-k medians), LOF and the lists
    for k in {5, 20, 32}; KDE at h = 1 and at the median nearest-neighbour distance of the subspace."""
    import vgan_amd
    Xr, Xq, feats, D2_fit, D2_new = _wide(case, ds)
    D2 = {(0, "fit"): D2_fit, (0, "new"): D2_new}

    def make(**kw):
        return vgan_amd.SubspaceEnsemble(_mask(DIM, [feats]), [1.0], engine=engine, **kw)

    use = 0.0
    for k in [5, 20, 32]:
        use = max(use, _check_detectors(make, Xr, Xq, [feats], [engine], k, None, D2=D2)[1])
    h_nn = float(np.median(oc.sorted_sq_dists(D2_fit, 1, True)[0][:, 0]))
    kde = 0.0
    for h in [1.0, h_nn]:
        ens = make(method="kde", bandwidth=h).fit(Xr)
        assert ens.bandwidth_[0] == h
        kde = max(kde, oc.check_kde_scores(ens.decision_scores_, Xr, Xr, feats, h, True, engine, D2=D2_fit))
        got, per = ens.decision_function(Xq, return_per_subspace=True)
        kde = max(kde, oc.check_kde_scores(got, Xq, Xr, feats, h, False, engine, D2=D2_new))
        np.testing.assert_array_equal(per[0], got.astype(np.float32))
    _report(capsys, f"{case:14s} d_s {ds:3d} {engine:5s}  lists max(err / 2 tau) {use:.2e}   kde max(err / tol) {kde:.2e}")


# ---- one mixed ensemble against the truth ------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ["normal", "scales"])
def test_mixed_ensemble_against_the_truth(case, capsys):
    """Subspaces of 200, 1, 33, 3, 64 and 17 features with unequal weights under a 60 kB workspace: several chunks, both
    engines, processing order != given order.  The raw per-subspace scores are held to the data, not taken on trust."""
    import vgan_amd
    n, nq, k = 777, 130, 10
    Xr, Xq = oc.adversarial_pair(case, n, nq, DIM, seed=9)
    rng = np.random.default_rng(3)
    sizes = [200, 1, 33, 3, 64, 17]
    feature_lists = [np.sort(rng.choice(DIM, ds, replace=False)) for ds in sizes]
    engines = ["gram" if ds >= 32 else "exact" for ds in sizes]
    proba = np.array([0.05, 0.3, 0.1, 0.25, 0.12, 0.18])
    made = []

    def make(**kw):
        made.append(vgan_amd.SubspaceEnsemble(_mask(DIM, feature_lists), proba, workspace_bytes=60_000, **kw))
        return made[-1]

    _, use = _check_detectors(make, Xr, Xq, feature_lists, engines, k, "scott")
    plan = made[0].plan
    assert list(plan.order) != sorted(plan.order) and len(plan.chunks(n, 60_000)) > 2
    assert [("gram" if g else "exact") for g in plan.gram[np.argsort(plan.order)]] == engines
    for ens in made:
        per = ens.per_subspace_scores_
        assert per.dtype == np.float32 and np.isfinite(per).all()
        want = np.zeros(n)
        for s in range(len(sizes)):
            want += proba[s] * per[s].astype(np.float64)
        np.testing.assert_allclose(ens.decision_scores_, want, rtol=1e-12, atol=0)
        got, per = ens.decision_function(Xq, return_per_subspace=True)
        want = np.zeros(nq)
        for s in range(len(sizes)):
            want += proba[s] * per[s].astype(np.float64)
        np.testing.assert_allclose(got, want, rtol=1e-12, atol=0)
    _report(capsys, f"mixed {case:8s} lists max(err / 2 tau) {use:.2e}")


# ---- row-count and split edges -----------------------------------------------------------------------------------------
def _same(a, b):
    assert len(a) == len(b)
    for x, y in zip(a, b):
        assert x.dtype == y.dtype and np.array_equal(x, y)


@pytest.mark.parametrize("engine", oc.ENGINES)
@pytest.mark.parametrize("k", [1, 8, 9, 16, 17, 32])
@pytest.mark.parametrize("d", [11, 787])
def test_row_count_and_split_edges(d, k, engine):
    """Odd row strides, k at the TopK<8 | 16 | 32> boundaries, reference sets of k + 1 rows and around one and two tiles,
    query blocks of 1 and 63 to 65 rows, and splits that leave slices with fewer than k candidates or none (the automatic
    choice at 65 rows gives one slice a single row).  Subspaces of 3 and 40 features (d = 11: 3 and all 11).  The run with
    splits = 1 is checked against the truth; every other (splits, workspace_bytes) must reproduce it bit for bit."""
    import vgan_amd
    rng = np.random.default_rng(100 * d + k)
    feature_lists = [np.sort(rng.choice(d, 3, replace=False)), np.sort(rng.choice(d, min(40, d), replace=False))]
    X, Y = rng.normal(size=(129, d)).astype(np.float32), rng.normal(size=(65, d)).astype(np.float32)
    NQS = [1, 63, 64, 65]
    for nr in sorted({k + 1, 63, 64, 65, 128, 129}):
        if nr < k + 1:
            continue
        Xr = np.ascontiguousarray(X[:nr])
        ntiles = -(-nr // 64)
        D2_fit = {(s, "fit"): restate_sq_dists(Xr, Xr, f) for s, f in enumerate(feature_lists)}
        base = None
        for splits, ws in [(1, 1 << 30), (None, 1 << 30), (2, 1 << 30), (ntiles, 1), (ntiles + 3, 1 << 30), (40, 1)]:
            def make(**kw):
                return vgan_amd.SubspaceEnsemble(_mask(d, feature_lists), [0.6, 0.4], engine=engine, splits=splits,
                                                 workspace_bytes=ws, **kw)
            if base is None:  # outputs per nq: lists and LOF at fit and for the new rows, kNN x 3, KDE
                base = {nq: _check_detectors(make, Xr, Y[:nq], feature_lists, [engine] * 2, k, 1.0, D2=D2_fit)[0] for nq in NQS}
                continue
            fitted = [make(method="lof", n_neighbors=k).fit(Xr)]
            fitted += [make(method="knn", n_neighbors=k, knn_method=how).fit(Xr) for how in KNN_HOW]
            fitted.append(make(method="kde", bandwidth=1.0).fit(Xr))
            for nq in NQS:
                out = [*fitted[0].kneighbors(), fitted[0].per_subspace_scores_, *fitted[0].kneighbors(Y[:nq])]
                for ens in fitted:
                    if ens is not fitted[0]:
                        out.append(ens.per_subspace_scores_)
                    out.append(ens.decision_function(Y[:nq], return_per_subspace=True)[1])
                _same(base[nq], out)


def test_the_automatic_split_at_65_rows_leaves_one_slice_a_single_row():
    """The host-side premise of the edge above, so that the edge stays visited if the split rule changes."""
    import vgan_amd
    ens = vgan_amd.SubspaceEnsemble(np.ones((1, 3), bool), [1.0])
    J = ens._splits(65, 65, 1)
    ntiles = 2
    per = -(-ntiles // J)
    assert J == 2 and per == 1 and 65 - 64 * per * (J - 1) == 1


# ---- width edges -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("engine", oc.ENGINES)
@pytest.mark.parametrize("ds", [4, 5, 31, 32, 33, 36, 63, 64, 65])
def test_width_edges(ds, engine):
    """Widths around the float4 padding, the exact engine's resident-query switch (w = 32 | 36) and the Gram K-tile (32,
    64), of d = 100 features: the last d_s features, the first d_s, and a scattered set."""
    import vgan_amd
    d, nr, nq, k = 100, 300, 100, 5
    rng = np.random.default_rng(ds)
    Xr, Xq = oc.adversarial_pair("offset100", nr, nq, d, seed=ds)
    feature_lists = [np.arange(d - ds, d), np.arange(ds), np.sort(rng.choice(d, ds, replace=False))]

    def make(**kw):
        return vgan_amd.SubspaceEnsemble(_mask(d, feature_lists), [0.2, 0.3, 0.5], engine=engine, **kw)

    _check_detectors(make, Xr, Xq, feature_lists, [engine] * 3, k, 2.0)


# ---- KDE regimes -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("engine", oc.ENGINES)
@pytest.mark.parametrize("ds", [3, 40])
def test_kde_regimes(ds, engine):
    import vgan_amd
    d, nr = 48, 500
    rng = np.random.default_rng(40 + ds)
    Xr = rng.normal(size=(nr, d)).astype(np.float32)
    Xn = rng.normal(size=(70, d)).astype(np.float32)
    feats = np.sort(rng.choice(d, ds, replace=False))
    D2_fit, D2_new = restate_sq_dists(Xr, Xr, feats), restate_sq_dists(Xn, Xr, feats)
    nn = np.sqrt(np.sort(D2_new, axis=1)[:, :2])

    def scores(h, Xq):
        ens = vgan_amd.SubspaceEnsemble(_mask(d, [feats]), [1.0], method="kde", bandwidth=h, engine=engine).fit(Xr)
        return ens.decision_scores_, ens.decision_function(Xq)

    # a bandwidth so small that only the pivot row carries weight: the second nearest row's term is below e^-1000
    h = float(np.sqrt((nn[:, 1] ** 2 - nn[:, 0] ** 2).min() / 2000.0))
    fit, new = scores(h, Xn)
    oc.check_kde_scores(fit, Xr, Xr, feats, h, True, engine, D2=D2_fit)
    oc.check_kde_scores(new, Xn, Xr, feats, h, False, engine, D2=D2_new)
    if engine == "exact":
        want = nn[:, 0] ** 2 / (2 * h * h) + np.log(nr) + ds * np.log(h) + 0.5 * ds * np.log(2 * np.pi)
        np.testing.assert_allclose(new, want, rtol=1e-5)
    # a bandwidth so large that every term is 1 to float32: the sum is the row count
    h = 1e5
    fit, new = scores(h, Xn)
    oc.check_kde_scores(fit, Xr, Xr, feats, h, True, engine, D2=D2_fit)
    oc.check_kde_scores(new, Xn, Xr, feats, h, False, engine, D2=D2_new)
    np.testing.assert_allclose(new, ds * np.log(h) + 0.5 * ds * np.log(2 * np.pi), rtol=1e-6)
    np.testing.assert_allclose(fit, ds * np.log(h) + 0.5 * ds * np.log(2 * np.pi), rtol=1e-6)
    # queries that equal reference rows: the pivot is d2 = 0
    for h in [0.5, 0.05]:
        _, new = scores(h, Xr[100:170])
        oc.check_kde_scores(new, Xr[100:170], Xr, feats, h, False, engine, D2=D2_fit[100:170])
        if engine == "exact" and h == 0.05 and ds == 40:  # every other row is e^-(d2 / 0.005) away: the row itself decides
            np.testing.assert_allclose(new, np.log(nr) + ds * np.log(h) + 0.5 * ds * np.log(2 * np.pi), rtol=1e-6)
    # queries 1e3 sigma away from the reference cloud
    far = (Xn + np.float32(1e3)).astype(np.float32)
    D2_far = restate_sq_dists(far, Xr, feats)
    for h in [1.0, 100.0]:
        _, new = scores(h, far)
        oc.check_kde_scores(new, far, Xr, feats, h, False, engine, D2=D2_far)


# ---- many tiles --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ds,engine", [(3, "exact"), (40, "gram")])
def test_many_tiles(ds, engine, capsys):
    """100_000 reference rows, 64 query rows, k = 32: J = 64 slices of 25 tiles each for the queries, and 1563 tiles per
    workgroup at fit.  kNN and KDE of the query rows and their lists against the restatement (64 x 100_000 pairs).  The
    full size is kept: fit plus scoring takes about 0.1 s per detector on an MI355X (reported with the run)."""
    import time
    import vgan_amd
    d, nr, nq, k = 48, 100_000, 64, 32
    rng = np.random.default_rng(77 + ds)
    Xr = rng.normal(size=(nr, d)).astype(np.float32)
    Xq = (1.5 * rng.normal(size=(nq, d))).astype(np.float32)
    feats = np.sort(rng.choice(d, ds, replace=False))
    D2 = restate_sq_dists(Xq, Xr, feats)

    def make(**kw):
        return vgan_amd.SubspaceEnsemble(_mask(d, [feats]), [1.0], engine=engine, **kw)

    t0 = time.perf_counter()
    ens = make(method="knn", n_neighbors=k, knn_method="mean").fit(Xr)
    assert ens._splits(nq, nr, 1) == 64
    assert np.isfinite(ens.decision_scores_).all() and ens.decision_scores_.shape == (nr,)
    got = ens.decision_function(Xq)
    t_knn = time.perf_counter() - t0
    oc.check_knn_scores(got, Xq, Xr, feats, k, "mean", False, engine, D2=D2)
    D, I = ens.kneighbors(Xq)
    use = oc.check_neighbor_lists(D[0], I[0], Xq, Xr, feats, k, False, engine, D2=D2)
    t_kde = 0.0
    for h in [0.2 if ds == 3 else 1.0, 3.0]:
        t0 = time.perf_counter()
        ens = make(method="kde", bandwidth=h).fit(Xr)
        got = ens.decision_function(Xq)
        t_kde = max(t_kde, time.perf_counter() - t0)
        assert np.isfinite(ens.decision_scores_).all()
        oc.check_kde_scores(got, Xq, Xr, feats, h, False, engine, D2=D2)
    _report(capsys, f"many tiles d_s {ds} {engine}: lists max(err / 2 tau) {use:.2e}; fit + scoring {t_knn:.2f} s (knn), "
                    f"{t_kde:.2f} s (kde)")
