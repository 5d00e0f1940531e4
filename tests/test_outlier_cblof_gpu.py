"""CBLOF over subspaces on the MI355X (csrc/cluster.hip through vgan_amd.SubspaceCBLOF), every row of every subspace held
to the float64 restatement of test_outlier_cblof_cpu.py.  Nothing is filtered: where a float32 distance engine may
legitimately give a row another centre at a near-tie, the check is the engine's own bound (tau: the k = 1 sandwich of
outlier_checks.py), not a comparison on the rows without near-ties.

tau.  exact engine: (w_s + 2) eps32 d2 / (1 - rho) at the row's true smallest d2.  Gram engine: d2_tolerance with the
data rows on both sides: every centre is a mean of data rows (or one of them), so its squared norm about the column mean
is at most the largest row's, which is what the bound takes for the reference side.
What the exact bound does not cover: it is the project's bound for the engine's arithmetic on float32 operands that are
exact, as data rows are for kNN.  A centre is a float64 mean, so its float32 image is rounded by up to eps32 |c - mean|
per coordinate (and, because both operands are centred here, a data row by eps32 |x - mean|); that moves d2 by up to
about 2 eps32 sqrt(d2) (|x - mean| + |c - mean|), which exceeds (w_s + 2) eps32 d2 for rows much farther from the mean
than from their centre (blobs at scale 6 in 2 features).  The bound is kept as the issue sets it and not widened by that
term: a row so close to a bisector that only the operand rounding decides it would fail check 1.  None of the inputs
below has such a row (the reports print "max(excess / 2 tau) 0": no assigned centre is farther than the true minimum).
Centres.  A float64 sum of n float32 values in any order is within (n - 1) 2^-53 of the sum of their absolute values,
relative; two such orders differ by at most n 2^-52 max|x| after the division by the count.  That is the bar on every
comparison of centres with numpy means, per feature."""
import functools

import numpy as np
import pytest

import outlier_checks as oc
from test_outlier_cblof_cpu import (SAFE_SEEDS, blobs, engine_bound_use, restate_boundary, restate_cblof, restate_lloyd, safe_case,
                                    sq_dists, subspace_features)

pytestmark = pytest.mark.gpu

N = 600
GROUPS = {24: [2, 4, 8, 24], 48: [40, 48]}  # data width -> widths of the subspaces of one ensemble
HARD = [("blobs", 24), ("blobs", 48), ("offset100", 48), ("scales", 48), ("lowrank", 48)]
HARD_WIDTHS = {24: [2, 4, 8, 24], 48: [2, 4, 8, 24, 40, 48]}


def _mask(d, feature_lists):
    m = np.zeros((len(feature_lists), d), bool)
    for s, feats in enumerate(feature_lists):
        m[s, feats] = True
    return m


def _report(capsys, line):
    with capsys.disabled():
        print("\n    " + line, end="")


def _make(d, feature_lists, engine, **kw):
    import vgan_amd
    S = len(feature_lists)
    return vgan_amd.SubspaceCBLOF(_mask(d, feature_lists), np.full(S, 1.0 / S), engine=engine, **kw)


def _centre_bar(X, feats):
    return X.shape[0] * 2.0 ** -52 * np.abs(X.astype(np.float64)[:, feats]).max(axis=0)


def _tau(engine, X, feats, dmin):
    return oc.sandwich_tau(engine, X, X, feats, dmin[:, None])[:, 0]


@functools.lru_cache(maxsize=None)
def _hard(name, d, seed=2):
    """(X, feature lists, the rows of the random init, the restatement per subspace with tol = 0)."""
    X = blobs(seed, d)[0] if name == "blobs" else oc.adversarial(name, N, d, seed)
    lists = [subspace_features(ds, d) for ds in HARD_WIDTHS[d]]
    rows = np.random.default_rng(seed).choice(N, size=8, replace=False)
    refs = [restate_lloyd(X, f, X.astype(np.float64)[rows][:, f], tol=0.0) for f in lists]
    return X, lists, rows, refs


def _check_step(X, feats, engine, c_in, c_out, labels):
    """One Lloyd step of the code under test from c_in: labels are the E step's, c_out the centres after the M step.
    Returns (largest use of 2 tau by an assigned centre, rows allowed to differ from the restatement)."""
    A = X.astype(np.float64)[:, feats]
    D2 = sq_dists(A, c_in)
    dmin = D2.min(axis=1)
    tau = _tau(engine, X, feats, dmin)
    got = D2[np.arange(len(A)), labels]
    over = got - dmin
    bad = np.flatnonzero(over > 2.0 * tau + 4e-16 * dmin)
    assert bad.size == 0, ("assigned centre beyond the minimum + 2 tau in rows", bad[:8], over[bad[:4]], tau[bad[:4]])
    srt = np.sort(D2, axis=1)
    clear = srt[:, 1] - srt[:, 0] > 2.0 * tau
    want = D2.argmin(axis=1)
    assert (labels[clear] == want[clear]).all(), ("rows away from every bisector", np.flatnonzero(clear & (labels != want))[:8])
    bar = _centre_bar(X, feats)
    for c in range(c_in.shape[0]):
        rows = labels == c
        if rows.any():
            assert (np.abs(c_out[c] - A[rows].mean(axis=0)) <= bar).all(), (c, np.abs(c_out[c] - A[rows].mean(axis=0)).max())
        else:
            np.testing.assert_array_equal(c_out[c], c_in[c])  # an empty cluster keeps its centre
    with np.errstate(divide="ignore", invalid="ignore"):
        use = np.where(over > 0, over / (2.0 * tau), 0.0).max()
    return float(use), int((~clear).sum())


# ---- 1. one Lloyd step from given centres --------------------------------------------------------------------------------
@pytest.mark.parametrize("engine", oc.ENGINES)
@pytest.mark.parametrize("name,d", HARD)
def test_one_lloyd_step_along_the_restatement_trajectory(name, d, engine, capsys):
    """max_iter = 1, tol = 0, float-array init: the centres before every M step of the restatement's run from 8 random
    rows (blobs get split, so rows sit near bisectors).  A subspace whose restatement is shorter repeats its last centres."""
    X, lists, rows, refs = _hard(name, d)
    steps = max(len(r["trajectory"]) for r in refs)
    use, near, emptied = 0.0, 0, 0
    for t in range(steps):
        c_in = [r["trajectory"][min(t, len(r["trajectory"]) - 1)] for r in refs]
        ens = _make(d, lists, engine, n_clusters=8, init=c_in, max_iter=1, tol=0.0)
        ens.keep_iteration_labels = True
        ens.fit(X)
        assert (ens.n_iter_ == 1).all() and not ens.converged_.any()
        for s, feats in enumerate(lists):
            labels = ens.last_iteration_labels_[s]
            assert labels.dtype == np.int32 and labels.min() >= 0 and labels.max() < 8
            u, m = _check_step(X, feats, engine, c_in[s], ens.cluster_centers_[s], labels)
            use, near = max(use, u), near + m
            emptied += int(np.bincount(labels, minlength=8).min() == 0)
    _report(capsys, f"{name:9s} d {d} {engine:5s}  {steps} steps  max(excess / 2 tau) {use:.2e}  rows within 2 tau of a bisector "
                    f"{near}  steps with an empty cluster {emptied}")


def test_empty_cluster_keeps_its_centre():
    """A centre far away from every row receives none: it stays, the others move (not sklearn's relocation)."""
    X, _ = blobs(1)
    feats = [subspace_features(4, 24), subspace_features(24, 24)]
    c0 = [np.concatenate([X.astype(np.float64)[:3][:, f], np.full((1, len(f)), 1e3)]) for f in feats]
    for engine in oc.ENGINES:
        ens = _make(24, feats, engine, n_clusters=4, init=c0, tol=0.0).fit(X)
        for s, f in enumerate(feats):
            ref = restate_lloyd(X, f, c0[s], tol=0.0)
            assert ref["emptied"] and ens.cluster_sizes_[s][3] == 0
            np.testing.assert_array_equal(ens.cluster_centers_[s][3], c0[s][3])
            assert (np.abs(ens.cluster_centers_[s] - ref["centers"]) <= _centre_bar(X, f)).all()


# ---- 2. whole fit, safe inputs -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("engine", oc.ENGINES)
@pytest.mark.parametrize("d", sorted(GROUPS))
@pytest.mark.parametrize("seed", SAFE_SEEDS)
def test_whole_fit_on_safe_inputs(seed, d, engine):
    """blobs(seed), C = 5, init = the first row of each blob.  Precondition, asserted on the restatement: strict
    convergence, no empty cluster, no row within the engines' bound of a bisector at any iteration, t = 3."""
    cases = [safe_case(seed, ds, d) for ds in GROUPS[d]]
    X = cases[0][0]
    lists, c0 = [c[2] for c in cases], [c[3] for c in cases]
    refs = [restate_lloyd(X, f, c) for f, c in zip(lists, c0)]
    for f, r in zip(lists, refs):
        assert r["converged"] and not r["emptied"] and engine_bound_use(X, f, r["trajectory"]) <= 0.5
        assert restate_cblof(X, f, r["centers"])[4] == 3
    Xq = blobs(seed + 100, d)[0][:200]
    try:
        from sklearn.cluster import KMeans
    except ImportError:
        KMeans = None
    per = {}
    for weights in (False, True):
        ens = _make(d, lists, engine, n_clusters=5, init=c0, use_weights=weights).fit(X)
        assert ens.converged_.all() and ens.converged_.dtype == bool
        assert ens.cluster_labels_.dtype == np.int32 and ens.cluster_sizes_.dtype == np.int64
        got_new, per_new = ens.decision_function(Xq, return_per_subspace=True)
        clusters_new = ens.predict_clusters(Xq)
        assert clusters_new.dtype == np.int32 and clusters_new.shape == (len(lists), 200)
        for s, (f, r) in enumerate(zip(lists, refs)):
            np.testing.assert_array_equal(ens.cluster_labels_[s], r["labels"])
            if KMeans is not None:
                km = KMeans(n_clusters=5, init=c0[s], n_init=1, algorithm="lloyd").fit(X.astype(np.float64)[:, f])
                np.testing.assert_array_equal(ens.cluster_labels_[s], km.labels_)
                assert (np.abs(ens.cluster_centers_[s] - km.cluster_centers_) <= _centre_bar(X, f) + 1e-12).all()
            assert ens.cluster_centers_[s].dtype == np.float64
            assert (np.abs(ens.cluster_centers_[s] - r["centers"]) <= _centre_bar(X, f)).all()
            assert ens.n_iter_[s] == r["n_iter"]
            np.testing.assert_array_equal(ens.cluster_sizes_[s], r["sizes"])
            np.testing.assert_allclose(ens.inertia_[s], r["inertia"], rtol=1e-12)
            want, _, _, large, t = restate_cblof(X, f, r["centers"], use_weights=weights)
            assert t == 3 and ens.large_cluster_mask_[s].sum() == 3
            np.testing.assert_array_equal(ens.large_cluster_mask_[s], large)
            np.testing.assert_allclose(ens.per_subspace_scores_[s], want, rtol=1e-6, atol=0)
            want_new, labels_new = restate_cblof(X, f, r["centers"], use_weights=weights, Xq=Xq)[:2]
            np.testing.assert_allclose(per_new[s], want_new, rtol=1e-6, atol=0)
            np.testing.assert_array_equal(clusters_new[s], labels_new)
        assert ens.per_subspace_scores_.dtype == np.float32 and ens.decision_scores_.dtype == np.float64
        np.testing.assert_allclose(ens.decision_scores_, ens.per_subspace_scores_.astype(np.float64).mean(axis=0), rtol=1e-14)
        np.testing.assert_allclose(got_new, per_new.astype(np.float64).mean(axis=0), rtol=1e-14)
        again, per_again = ens.decision_function(X, return_per_subspace=True)
        np.testing.assert_array_equal(again, ens.decision_scores_)  # fit excludes nothing: bit for bit
        np.testing.assert_array_equal(per_again, ens.per_subspace_scores_)
        per[weights] = ens.per_subspace_scores_
    assert (per[True] >= per[False]).all()  # every cluster holds at least one row


# ---- 3. whole fit, hard inputs -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("engine", oc.ENGINES)
@pytest.mark.parametrize("name,d", HARD)
def test_whole_fit_on_hard_inputs(name, d, engine, capsys):
    """C = 8 from random rows, tol = 0: what holds whatever near-tie an engine took."""
    X, lists, rows, refs = _hard(name, d)
    ens = _make(d, lists, engine, n_clusters=8, init=rows, tol=0.0, max_iter=100)
    ens.keep_iteration_labels = True
    ens.fit(X)
    step = _make(d, lists, engine, n_clusters=8, init=ens.cluster_centers_, tol=0.0, max_iter=1).fit(X)
    X64 = X.astype(np.float64)
    for s, feats in enumerate(lists):
        A, cen, labels = X64[:, feats], ens.cluster_centers_[s], ens.cluster_labels_[s]
        D2 = sq_dists(A, cen)
        own = D2[np.arange(N), labels]
        assert (own <= D2.min(axis=1) * (1 + 1e-13)).all()  # the exact float64 arg-min (sums of d_s <= 48 terms)
        np.testing.assert_array_equal(ens.cluster_sizes_[s], np.bincount(labels, minlength=8))
        assert ens.cluster_sizes_[s].sum() == N
        np.testing.assert_allclose(ens.inertia_[s], own.sum(), rtol=1e-12)
        if ens.converged_[s]:
            last, bar = ens.last_iteration_labels_[s], _centre_bar(X, feats)
            for c in range(8):
                if (last == c).any():
                    assert (np.abs(cen[c] - A[last == c].mean(axis=0)) <= bar).all()
            np.testing.assert_array_equal(step.cluster_centers_[s], cen)  # a further step changes nothing
            np.testing.assert_array_equal(step.cluster_labels_[s], labels)
        # exact Lloyd never raises the inertia; an engine's near-tie pick raises one row's d2 by at most 2 tau per
        # iteration, tau at the row's smallest d2 as in (1).  Those d2 change with the centres, but their sum is the
        # inertia of that iteration, which the bound so far bounds: the exact engine's tau is linear in d2 (sum over the
        # rows = tau of the inertia), the Gram engine's does not depend on it.
        bound = sq_dists(A, A[rows]).min(axis=1).sum()
        for _ in range(int(ens.n_iter_[s])):
            bound += 2.0 * _tau(engine, X, feats, np.full(N, bound / N)).sum()
        assert ens.inertia_[s] <= bound, (ens.inertia_[s], bound)
        want, _, sizes, large, t = restate_cblof(X, feats, cen)
        np.testing.assert_array_equal(ens.large_cluster_mask_[s], large)
        np.testing.assert_allclose(ens.per_subspace_scores_[s], want, rtol=1e-6, atol=0)
    _report(capsys, f"{name:9s} d {d} {engine:5s}  n_iter {ens.n_iter_.tolist()} (restatement {[r['n_iter'] for r in refs]})  "
                    f"converged {int(ens.converged_.sum())}/{len(lists)}")


# ---- 4. device-driven loop = host-driven loop ----------------------------------------------------------------------------
@pytest.mark.parametrize("engine", oc.ENGINES)
@pytest.mark.parametrize("name,d", HARD)
def test_device_loop_equals_host_driven_steps(name, d, engine):
    """fit(max_iter=m) against m fits of max_iter = 1 fed with the previous centres, on every hard input: finished and
    unfinished subspaces share the chunk, m is below, at and beyond every subspace's convergence, at multiples of the
    polling stride and between them."""
    X, lists, rows, refs = _hard(name, d)
    S = len(lists)
    centres = [X.astype(np.float64)[rows][:, f] for f in lists]
    host, moved = [], []
    while len(host) < 60:
        ens = _make(d, lists, engine, n_clusters=8, init=centres, tol=0.0, max_iter=1).fit(X)
        moved.append([not np.array_equal(a, b) for a, b in zip(ens.cluster_centers_, centres)])
        host.append(ens)
        centres = ens.cluster_centers_
        if not any(moved[-1]) and len(host) >= 2 and not any(moved[-2]):
            break
    moved = np.array(moved)
    needs = moved.sum(axis=0)  # M steps that moved each subspace
    assert moved[-1].sum() == 0 and needs.max() < 58 and len(set(needs.tolist())) > 1, needs
    for m in sorted({1, 2, int(needs.min()), int(needs.min()) + 1, int(np.median(needs)), int(needs.max()), int(needs.max()) + 1,
                     int(needs.max()) + 2}):
        ens = _make(d, lists, engine, n_clusters=8, init=rows, tol=0.0, max_iter=m).fit(X)
        ref = host[m - 1]
        for s in range(S):
            np.testing.assert_array_equal(ens.cluster_centers_[s], ref.cluster_centers_[s])
        np.testing.assert_array_equal(ens.cluster_labels_, ref.cluster_labels_)
        np.testing.assert_array_equal(ens.per_subspace_scores_, ref.per_subspace_scores_)
        np.testing.assert_array_equal(ens.decision_scores_, ref.decision_scores_)
        np.testing.assert_array_equal(ens.n_iter_, moved[:m].sum(axis=0))
        np.testing.assert_array_equal(ens.converged_, needs < m)


# ---- 5. bit-identity, the tolerance rule, max_iter -----------------------------------------------------------------------
def _outputs(ens):
    return [np.concatenate([c.reshape(-1) for c in ens.cluster_centers_]), ens.cluster_labels_, ens.n_iter_, ens.converged_,
            ens.per_subspace_scores_, ens.decision_scores_, ens.inertia_, ens.cluster_sizes_]


@pytest.mark.parametrize("engine", ["auto"] + list(oc.ENGINES))
def test_bit_identical_across_chunking_and_runs(engine):
    X, lists, rows, _ = _hard("scales", 48)
    lists = lists[::-1]  # processing order != given order under "auto"
    one = _make(48, lists, engine, n_clusters=8, init=rows, max_iter=40).fit(X)
    two = _make(48, lists, engine, n_clusters=8, init=rows, max_iter=40).fit(X)
    per_subspace = _make(48, lists, engine, n_clusters=8, init=rows, max_iter=40, workspace_bytes=1)
    assert len(per_subspace.plan.chunks(N, 1)) == len(lists) and len(one.plan.chunks(N, one.workspace_bytes)) <= 2
    per_subspace.fit(X)
    for a, b, c in zip(_outputs(one), _outputs(two), _outputs(per_subspace)):
        np.testing.assert_array_equal(a, b)
        np.testing.assert_array_equal(a, c)
    rand = _make(48, lists, engine, n_clusters=8, seed=2, max_iter=40).fit(X)  # init="random" draws these very rows
    np.testing.assert_array_equal(rand.cluster_labels_, one.cluster_labels_)


@pytest.mark.parametrize("engine", oc.ENGINES)
@pytest.mark.parametrize("seed", SAFE_SEEDS[:3])
def test_tolerance_rule_against_the_restatement(seed, engine):
    """tol so large that the rule ends the run before the labels settle (where the restatement says so)."""
    stopped = 0
    for d in sorted(GROUPS):
        cases = [safe_case(seed, ds, d) for ds in GROUPS[d]]
        X, lists, c0 = cases[0][0], [c[2] for c in cases], [c[3] for c in cases]
        for tol in (0.3, 1e-2):
            ens = _make(d, lists, engine, n_clusters=5, init=c0, tol=tol).fit(X)
            for s, f in enumerate(lists):
                r = restate_lloyd(X, f, c0[s], tol=tol)
                assert all(abs(v - 1.0) > 1e-6 for v in r["shifts"])  # no shift sits on the threshold
                assert ens.n_iter_[s] == r["n_iter"] and ens.converged_[s] == r["converged"]
                np.testing.assert_array_equal(ens.cluster_labels_[s], r["labels"])
                assert (np.abs(ens.cluster_centers_[s] - r["centers"]) <= _centre_bar(X, f)).all()
                stopped += int(not r["converged"])
    assert stopped > 0


@pytest.mark.parametrize("engine", oc.ENGINES)
def test_max_iter_reached_is_not_converged(engine):
    X, lists, rows, refs = _hard("blobs", 24)
    assert min(r["n_iter"] for r in refs) > 2
    ens = _make(24, lists, engine, n_clusters=8, init=rows, tol=0.0, max_iter=2).fit(X)
    assert (ens.n_iter_ == 2).all() and not ens.converged_.any()


# ---- 6. through the model ------------------------------------------------------------------------------------------------
def test_vgan_outlier_ensemble_cblof_end_to_end():
    import vgan_amd
    from test_outlier_gpu import _planted
    from test_outlier_norm_gpu import _check_scores, _check_stats
    X = _planted()[:, :10]
    model = vgan_amd.VGAN_no_kl(epochs=2)
    model.fit(X)
    ens = model.outlier_ensemble(method="cblof", X=X)
    assert isinstance(ens, vgan_amd.SubspaceCBLOF) and ens.n_clusters == 8
    S = model.subspaces.shape[0]
    assert ens.per_subspace_scores_.shape == (S, X.shape[0]) and np.isfinite(ens.decision_scores_).all()
    _check_scores(ens.decision_scores_, ens.per_subspace_scores_, model.proba, None, None, "sum")
    ens = model.outlier_ensemble(method="cblof", n_clusters=4, normalize="robust", combination="max", contamination=0.05, X=X)
    assert ens.n_clusters == 4 and ens.normalize == "robust" and ens.combination == "max"
    c, w = _check_stats(ens, "robust")
    _check_scores(ens.decision_scores_, ens.per_subspace_scores_, model.proba, c, w, "max")
    assert ens.threshold_ == np.percentile(ens.decision_scores_, 95.0)
    np.testing.assert_array_equal(ens.labels_, (ens.decision_scores_ > ens.threshold_).astype(int))
    np.testing.assert_array_equal(ens.predict(X[:50]), (ens.decision_function(X[:50]) > ens.threshold_).astype(int))
    assert ens.predict_proba(X[:50]).shape == (50, 2)
    assert isinstance(model.outlier_ensemble(method="knn", X=X), vgan_amd.SubspaceEnsemble)


# ---- 7. it detects what it is for ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", SAFE_SEEDS)
def test_small_blobs_rank_above_every_other_row(seed, capsys):
    """The 40 rows of the two small blobs against the 560 others in the 24-, 40- and 48-feature subspaces, default
    settings but C = 5 from the first row of each blob.  kNN (k = 5) on the same rows is reported, not asserted."""
    import vgan_amd
    for ds, d in [(24, 24), (40, 48), (48, 48)]:
        X, blob, feats, c0 = safe_case(seed, ds, d)
        ens = _make(d, [feats], "auto", n_clusters=5, init=[c0]).fit(X)
        small = blob >= 3
        assert ens.decision_scores_[small].min() > ens.decision_scores_[~small].max()
        knn = vgan_amd.SubspaceEnsemble(_mask(d, [feats]), [1.0], method="knn", n_neighbors=5).fit(X).decision_scores_
        top = np.argsort(-knn)[:40]
        _report(capsys, f"blobs({seed}) {ds:2d} features: CBLOF ranks all 40 small-blob rows first; kNN (k = 5) has "
                        f"{int(small[top].sum())} of them in its top 40, the best-ranked large-blob row at rank "
                        f"{int(np.flatnonzero(~small[np.argsort(-knn)])[0]) + 1}")
