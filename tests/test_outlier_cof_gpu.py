"""Connectivity-based outlier scores on the MI355X (csrc/outlier_cof.hip through vgan_amd.SubspaceCOF), against the float64
restatement of test_outlier_cof_cpu.py (its set-based nearest chain pinned to scipy's minimum spanning tree there).

The bar on a chaining distance is relative (d_s + k + 8) 2^-53: every term is positive and every operation rounds once (d_s
additions per d2, half of that after the square root, k weighted additions).  The bar on a score is one float32 ulp,
|got - want| <= 2^-23 |want|: the float64 error is far below 2^-24 and the one rounding to float32 adds at most 2^-24.  Where
the kernel's own neighbour lists and its own ``ac_dist_`` are the input of the restatement no row is left out; the lists
themselves are held to the data by check_neighbor_lists."""
import numpy as np
import pytest

import outlier_checks as oc
from test_outlier_abod_gpu import _mask, _report
from test_outlier_cof_cpu import CHAINS, FLT_MAX, restate_ceiling, restate_cof_chain, restate_cof_from_lists, to_score32
from test_outlier_cpu import restate_neighbors
from test_outlier_gpu import _planted
from test_outlier_kde_cpu import restate_sq_dists
from test_outlier_norm_gpu import _check_scores, _check_stats
from test_outlier_norm_cpu import restate_proba, restate_stats

pytestmark = pytest.mark.gpu

ULP32 = 2.0 ** -23
EPS64 = 2.0 ** -53
MIN_GAP = 1e-9  # below this a disagreement of the chains could be blamed on a near-tie


@pytest.fixture(autouse=True)
def cof_class():
    import vgan_amd
    return vgan_amd.SubspaceCOF


def _check_rows(got32, want, ceiling, bar=ULP32):
    """Every row: a non-degenerate one within `bar` (one float32 ulp) of the restatement, a degenerate one (NaN in want)
    exactly the ceiling.  Returns the largest error in float32 ulps."""
    got = np.asarray(got32).astype(np.float64)
    assert np.asarray(got32).dtype == np.float32 and got.shape == want.shape and np.isfinite(got).all()
    deg = np.isnan(want)
    assert (got[deg] == float(np.float32(ceiling))).all(), ("degenerate rows off the ceiling", np.flatnonzero(deg)[:8])
    want32 = to_score32(want).astype(np.float64)  # the clamp at the float32 range is part of the contract
    err = np.abs(got[~deg] - want32[~deg])
    lim = bar * np.abs(want32[~deg])
    bad = np.flatnonzero(err > lim)
    assert (err <= lim).all(), ("rows", np.flatnonzero(~deg)[bad[:8]], got[~deg][bad[:4]], want[~deg][bad[:4]])
    with np.errstate(divide="ignore", invalid="ignore"):
        return float(np.where(lim > 0, err / (ULP32 * np.abs(want32[~deg])), 0.0).max()) if err.size else 0.0


def _check_ac(got, want, ds, k):
    """The chaining distances within relative (d_s + k + 8) 2^-53; returns the largest error in units of 2^-53 |want|."""
    assert got.dtype == np.float64 and got.shape == want.shape and np.isfinite(got).all()
    err = np.abs(got - want)
    assert (err <= (ds + k + 8) * EPS64 * want).all(), (ds, k, float((err / np.maximum(want, 1e-300)).max() / EPS64))
    return float((err / np.maximum(want, 1e-300)).max() / EPS64)


# ---- 1. every row against the restatement on the kernel's own lists -----------------------------------------------------
SIZES = [3, 24, 45, 33, 2]  # narrow, mid, wide; 45 and 33 are no multiples of 4 or of the kernel's 32-feature block
KS = [1, 2, 8, 9, 16, 17, 31, 32]  # a single edge, the 8 | 16 | 32 tile boundaries, the 33-point case


@pytest.mark.parametrize("chain", CHAINS)
@pytest.mark.parametrize("engine", oc.ENGINES)
@pytest.mark.parametrize("case", oc.ADVERSARIAL)
def test_every_row_matches_the_restatement_on_the_kernels_own_lists(case, engine, chain, cof_class, capsys):
    """301 reference and 131 query rows (neither a multiple of the four rows of a workgroup), fit and decision_function,
    both engines forced on every width.  The restatement takes the kernel's lists and, for the denominators, the kernel's
    ac_dist_ (itself checked against the restated chain), so no row is left out; its smallest chain gap is asserted first,
    so that no disagreement can be blamed on a near-tie.  The lists are checked once (they do not depend on the chain)."""
    d, nr, nq = 100, 301, 131
    Xr, Xq = oc.adversarial_pair(case, nr, nq, d, seed=13)
    rng = np.random.default_rng(4)
    feature_lists = [np.sort(rng.choice(d, ds, replace=False)) for ds in SIZES]
    D2 = {}
    if chain == "sbn":
        D2 = {(s, mode): restate_sq_dists(Q, Xr, f) for s, f in enumerate(feature_lists) for mode, Q in (("fit", Xr), ("new", Xq))}
    worst, worst_ac, min_gap = 0.0, 0.0, np.inf
    for k in KS:
        ens = cof_class(_mask(d, feature_lists), np.full(len(SIZES), 0.2), n_neighbors=k, chain=chain, engine=engine).fit(Xr)
        assert ens.score_ceiling_.dtype == np.float64 and ens.score_ceiling_.shape == (len(SIZES),)
        assert ens.n_degenerate_.shape == (len(SIZES),) and ens.n_degenerate_.dtype.kind == "i"
        assert ens.ac_dist_.dtype == np.float64 and ens.ac_dist_.shape == (len(SIZES), nr)
        _, per_new = ens.decision_function(Xq, return_per_subspace=True)
        for mode, Q, excl, per, lists in [("fit", Xr, True, ens.per_subspace_scores_, ens.kneighbors()),
                                          ("new", Xq, False, per_new, ens.kneighbors(Xq))]:
            D, I = lists
            assert per.shape == (len(SIZES), Q.shape[0]) and I.shape == (len(SIZES), Q.shape[0], k)
            for s, feats in enumerate(feature_lists):
                if chain == "sbn":
                    oc.check_neighbor_lists(D[s], I[s], Q, Xr, feats, k, excl, engine, D2=D2[s, mode])
                ac, gap = restate_cof_chain(Q, Xr, feats, I[s], chain)
                min_gap = min(min_gap, float(gap.min()))
                assert gap.min() >= MIN_GAP, (mode, s, k, float(gap.min()))
                if mode == "fit":
                    worst_ac = max(worst_ac, _check_ac(ens.ac_dist_[s], ac, len(feats), k))
                want = restate_cof_from_lists(ac, ens.ac_dist_[s], I[s])
                assert not np.isnan(want).any()  # continuous data: no duplicates
                worst = max(worst, _check_rows(per[s], want, ens.score_ceiling_[s]))
                if mode == "fit":
                    assert ens.n_degenerate_[s] == 0 and ens.score_ceiling_[s] == float(per[s].max())
    _report(capsys, f"{case:14s} {engine:5s} {chain:4s} max |got - want| / (2^-23 |want|) {worst:.3f}, ac error "
                    f"{worst_ac:.1f} x 2^-53, smallest chain gap {min_gap:.1e}")


def test_hand_checkable_cases_on_the_device(cof_class):
    """Points 0, 1, 3, 7 and 15 on a line, k = 3.  From 0: edges 1, 2, 4, ac 22/12 under either chain; from 15: 8, 4, 2, ac
    68/12.  The list (1, -1.5, 1.2) of the query 0, given to the chain entry in that order: 9.8/12 set-based, 12.4/12 by
    rank.  Data of scale 1e15: the ratio stays near 1 (scale free).  A ratio beyond the float32 range is stored as the
    largest finite float32 (the score entry alone: the float32 neighbour search does not span 1e38)."""
    import torch
    X = np.zeros((5, 2), np.float32)
    X[:, 0] = [0, 1, 3, 7, 15]
    for chain in CHAINS:
        ens = cof_class(np.array([[True, False]]), [1.0], n_neighbors=3, chain=chain).fit(X)
        assert abs(ens.ac_dist_[0, 0] - 22.0 / 12.0) <= 4 * EPS64 * 22.0 / 12.0
        assert abs(ens.ac_dist_[0, 4] - 68.0 / 12.0) <= 4 * EPS64 * 68.0 / 12.0
        want = restate_cof_from_lists(ens.ac_dist_[0], ens.ac_dist_[0], ens.kneighbors()[1][0])
        _check_rows(ens.per_subspace_scores_[0], want, ens.score_ceiling_[0])
        assert ens.decision_scores_[0] == float(ens.per_subspace_scores_[0, 0])
    ops, dev = ens.ops, "cuda"
    Xr = np.array([[1.0], [-1.5], [1.2]], np.float32)
    table = (torch.zeros(1, dtype=torch.int32, device=dev), torch.tensor([0, 1], dtype=torch.int32, device=dev), None)
    idx = torch.tensor([[[0, 1, 2]]], dtype=torch.int32, device=dev)
    ac = torch.empty(2, 1, dtype=torch.float64, device=dev)
    for c, chain in enumerate(CHAINS):
        ops.outlier_cof_chain(torch.zeros(1, 1, device=dev), torch.as_tensor(Xr, device=dev), table, 0, 1, idx, 3, c, ac[c:c + 1])
        want = restate_cof_chain(np.zeros((1, 1), np.float32), Xr, [0], [[0, 1, 2]], chain)[0][0]
        assert abs(float(ac[c, 0]) - want) <= 8 * EPS64 * want
    assert abs(float(ac[0, 0]) - 9.8 / 12.0) < 1e-7 and abs(float(ac[1, 0]) - 12.4 / 12.0) < 1e-7
    huge = (1e15 * np.random.default_rng(0).normal(size=(50, 3))).astype(np.float32)
    ens = cof_class(np.ones((1, 3), bool), [1.0], n_neighbors=5).fit(huge)
    assert np.isfinite(ens.ac_dist_).all() and (ens.ac_dist_ > 1e13).all()
    assert (ens.per_subspace_scores_ > 0.1).all() and (ens.per_subspace_scores_ < 100).all()
    ac_q = torch.tensor([[1e40, 1e300, 3.0, 0.0, 2.0]], dtype=torch.float64, device=dev)
    ac_ref = torch.tensor([[1.0, 1e-300, 0.0, 0.0, 0.5]], dtype=torch.float64, device=dev)
    lists = torch.tensor([[[0, 0], [1, 1], [0, 4], [2, 3], [3, 2]]], dtype=torch.int32, device=dev)
    score = torch.empty(1, 5, dtype=torch.float32, device=dev)
    ops.outlier_cof_score(ac_q, ac_ref, lists, 2, score)
    got = score.cpu().numpy()[0]
    assert got[0] == got[1] == np.float32(FLT_MAX) and got[2] == 4.0 and got[3] == 1.0 and np.isnan(got[4])
    want = restate_cof_from_lists(ac_q.cpu().numpy()[0], ac_ref.cpu().numpy()[0], lists.cpu().numpy()[0])
    np.testing.assert_array_equal(to_score32(want), got)


# ---- 2. end to end against an independent restatement ----------------------------------------------------------------------
PLANTED_SUBSPACES = [[0, 1], [0, 1, 2], [4, 7]]


def _open_sets(Xq, Xr, feats, k, exclude_self):
    """(idx [nq, k + 1], open [nq]): the restatement's own float64 neighbours, and whether the row's neighbour set is
    legitimately open: its float64 gap d_(k+1)^2 - d_(k)^2 is within 2 tau of the exact engine's bound (sandwich_tau)."""
    dist, idx = restate_neighbors(Xq, Xr, feats, k, exclude_self=exclude_self)
    d2 = dist ** 2
    tau = oc.sandwich_tau("exact", Xq, Xr, feats, d2[:, :k])[:, k - 1]
    return idx, (d2[:, k] - d2[:, k - 1]) <= 2.0 * tau


@pytest.mark.parametrize("k", [5, 10, 20])
@pytest.mark.parametrize("mode", ["fit", "new"])
def test_end_to_end_against_an_independent_restatement(mode, k, cof_class, capsys):
    """The restatement finds its own float64 neighbours and its own chaining distances of the fitted rows.  A row may be
    left out only where its own neighbour set, or the fit-time set of one of its k neighbours, is open (the sandwich_tau
    criterion of the ABOD test).  Every other row must carry the restatement's set and its score within 2^-22 |want|: two
    float32-sized roundings, the denominators differing from the restatement's by float64 noise only.  At most 1 % of the
    (subspace, row) pairs are left out (on the CPU the restatement alone leaves out 0, 0, 30 at fit and 0, 0, 52 on new
    rows, for k = 5, 10, 20)."""
    X = _planted()
    Xr = X if mode == "fit" else np.ascontiguousarray(X[:1500])
    mask = _mask(10, PLANTED_SUBSPACES)
    ens = cof_class(mask, [0.5, 0.3, 0.2], n_neighbors=k, engine="exact").fit(Xr)
    if mode == "fit":
        per, (_, I) = ens.per_subspace_scores_, ens.kneighbors()
    else:
        per, (_, I) = ens.decision_function(X, return_per_subspace=True)[1], ens.kneighbors(X)
    left_out = 0
    for s, feats in enumerate(PLANTED_SUBSPACES):
        feats = np.array(feats)
        idx_fit, open_fit = _open_sets(Xr, Xr, feats, k, True)
        idx, open_own = (idx_fit, open_fit) if mode == "fit" else _open_sets(X, Xr, feats, k, False)
        ac_fit = restate_cof_chain(Xr, Xr, feats, idx_fit[:, :k])[0]
        ac_q = ac_fit if mode == "fit" else restate_cof_chain(X, Xr, feats, idx[:, :k])[0]
        want = restate_cof_from_lists(ac_q, ac_fit, idx[:, :k])
        assert not np.isnan(want).any()
        assert (np.sort(I[s][~open_own], axis=1) == np.sort(idx[~open_own, :k], axis=1)).all(), (s, "another neighbour set")
        keep = ~(open_own | open_fit[idx[:, :k]].any(axis=1))
        left_out += int((~keep).sum())
        got = per[s].astype(np.float64)
        assert (np.abs(got[keep] - want[keep]) <= 2 * ULP32 * np.abs(want[keep])).all(), (s, "score off the restatement")
    total = 3 * X.shape[0]
    assert total == 6060 and left_out <= 0.01 * total, (left_out, total)
    _report(capsys, f"{mode} k {k:2d}: {left_out} of {total} rows with an open neighbour set in their chain or denominator")


# ---- 3. the ensemble tail ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("normalize", [None, "robust"])
@pytest.mark.parametrize("combination", ["sum", "max"])
def test_ensemble_tail_on_the_scores_the_kernels_left(normalize, combination, cof_class):
    X = _planted()
    Xr, Y = np.ascontiguousarray(X[:1500]), np.ascontiguousarray(X[1400:])
    mask, proba = _mask(10, PLANTED_SUBSPACES), np.array([0.5, 0.3, 0.2])
    ens = cof_class(mask, proba, n_neighbors=10, normalize=normalize, combination=combination, contamination=0.05,
                    engine="exact").fit(Xr)
    per = ens.per_subspace_scores_
    assert per.dtype == np.float32 and per.shape == (3, 1500) and np.isfinite(per).all() and (per > 0).all()
    assert ens.decision_scores_.dtype == np.float64 and ens.decision_scores_.shape == (1500,)
    assert (np.abs(np.median(per, axis=1) - 1) < 0.25).all()  # scale free: inliers sit around 1
    if normalize is None:
        assert ens.score_center_ is None and ens.score_scale_ is None
        c = w = None
    else:
        c, w = _check_stats(ens, normalize)
    _check_scores(ens.decision_scores_, per, proba, c, w, combination)
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
    # decision_function(X_train) is not decision_scores_: every row is its own nearest neighbour there, the first edge is 0
    again = ens.decision_function(Xr, return_per_subspace=True)[1]
    assert not np.array_equal(again, per)
    I_again = ens.kneighbors(Xr)[1][0]
    assert (I_again[:, 0] == np.arange(1500)).all()
    ac_again = restate_cof_chain(Xr, Xr, np.array([0, 1]), I_again)[0]
    _check_rows(again[0], restate_cof_from_lists(ac_again, ens.ac_dist_[0], I_again), ens.score_ceiling_[0])


# ---- 4. degenerate and discrete data -----------------------------------------------------------------------------------------
def _degenerate_data(k, seed):
    """Features 0 and 1 are small integers (many repeated rows), 2 .. 5 continuous.  For every j in 0 .. k a group of
    k - j + 1 copies of one point of its own (the data of the ABOD test), and one row next to the (k + 1)-fold group: at fit
    its k neighbours are copies of that group, whose chaining distances are 0, while its own is not.  Queries: on the
    (k + 1)-fold group, next to it, and on the single point."""
    rng = np.random.default_rng(seed)
    X = rng.normal(size=(340, 6))
    X[:, :2] = rng.integers(0, 30, size=(340, 2))
    rows = 300
    for j in range(k + 1):
        X[rows:rows + k - j + 1, :2] = [100 + 10 * j, 200 - 7 * j]
        rows += k - j + 1
    X[rows, :2] = [101, 200]
    rows += 1
    X = X[:rows]
    Y = rng.normal(size=(61, 6))
    Y[:, :2] = rng.integers(0, 30, size=(61, 2))
    Y[:3, :2] = X[300, :2]                       # on the largest group: ac 0 over a denominator of 0
    Y[3:6, :2] = [[100, 201], [99, 200], [98, 198]]  # next to it: degenerate
    Y[6:9, :2] = X[rows - 2, :2]                 # on the single point
    return X.astype(np.float32), Y.astype(np.float32)


@pytest.mark.parametrize("engine", oc.ENGINES)
def test_zero_denominators_and_the_ceiling_of_the_fit(engine, cof_class):
    """Integer features: d2 is exact, so ties are decided by the rule alone and every row must match the restatement on the
    kernel's lists within the ulp bar, none left out."""
    k = 6
    X, Y = _degenerate_data(k, seed=5)
    feature_lists = [[0, 1], [2, 3, 4], [0, 5], [1]]
    for chain in CHAINS:
        ens = cof_class(_mask(6, feature_lists), [0.4, 0.3, 0.2, 0.1], n_neighbors=k, chain=chain, engine=engine).fit(X)
        I = ens.kneighbors()[1]
        ac = np.array([restate_cof_chain(X, X, np.array(f), I[s], chain)[0] for s, f in enumerate(feature_lists)])
        for s, f in enumerate(feature_lists):
            _check_ac(ens.ac_dist_[s], ac[s], len(f), k)
        raw = np.array([restate_cof_from_lists(ac[s], ens.ac_dist_[s], I[s]) for s in range(4)])
        deg = np.isnan(raw)
        assert deg[0].sum() >= 1 and deg[0][-1] and not deg[1].any()  # the row next to the (k + 1)-fold group
        assert (ac[0][300:300 + k + 1] == 0).all() and (raw[0][300:300 + k + 1] == 1).all()  # both zero: exactly 1
        # the kernel's scores with NaN put back where the restatement is degenerate: the ceiling rule, exactly
        per = ens.per_subspace_scores_
        want_per, want_ceiling, want_n = restate_ceiling(np.where(deg, np.float32(np.nan), per))
        np.testing.assert_array_equal(per, want_per)
        np.testing.assert_array_equal(ens.score_ceiling_, want_ceiling)
        np.testing.assert_array_equal(ens.n_degenerate_, want_n)
        assert (per[0][300:300 + k + 1] == 1).all() and per[0][-1] == np.float32(ens.score_ceiling_[0]) > 1
        for s in range(4):
            _check_rows(per[s], raw[s], ens.score_ceiling_[s])
        assert np.isfinite(ens.decision_scores_).all() and np.isfinite(per).all()
        # new rows take the stored ceiling, and compute none of their own
        before = ens.score_ceiling_.copy()
        got, per_new = ens.decision_function(Y, return_per_subspace=True)
        I_new = ens.kneighbors(Y)[1]
        raw_new = np.array([restate_cof_from_lists(restate_cof_chain(Y, X, np.array(f), I_new[s], chain)[0], ens.ac_dist_[s], I_new[s])
                            for s, f in enumerate(feature_lists)])
        assert (raw_new[0][:3] == 1).all() and np.isnan(raw_new[0][3:6]).all() and not np.isnan(raw_new[0][6:9]).any()
        for s in range(4):
            _check_rows(per_new[s], raw_new[s], before[s])
        assert (per_new[0][:3] == 1).all() and (per_new[0][3:6] == np.float32(before[0])).all()
        assert np.isfinite(got).all() and np.array_equal(ens.score_ceiling_, before)
    # a subspace in which every row is a duplicate: all exactly 1, nothing degenerate, ceiling 1; zscore scale 1
    X1 = X.copy()
    X1[:, 3] = 2.5
    one = cof_class(_mask(6, [[3], [2, 4]]), [0.5, 0.5], n_neighbors=k, engine=engine, normalize="zscore").fit(X1)
    assert one.n_degenerate_.tolist() == [0, 0] and one.score_ceiling_[0] == 1.0 and (one.ac_dist_[0] == 0).all()
    assert (one.per_subspace_scores_[0] == 1).all() and one.score_scale_[0] == 1.0 and one.score_center_[0] == 1.0
    assert np.isfinite(one.decision_scores_).all()
    assert (one.decision_function(X1[:9], return_per_subspace=True)[1][0] == 1).all()
    # every row degenerate is reachable only for new rows: off the constant, over fitted rows that are all point masses
    off = X1[:5].copy()
    off[:, 3] = 3.5
    got, per_off = one.decision_function(off, return_per_subspace=True)
    assert (per_off[0] == 1).all() and np.isfinite(got).all()  # the ceiling of a subspace without a non-degenerate row


# ---- 5. determinism ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("engine", oc.ENGINES)
def test_scores_are_bit_identical_for_every_split_chunking_and_run(engine, cof_class):
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
    runs = []
    for splits, ws in [(1, 1 << 30), (1, 1 << 30), (3, 1 << 30), (7, 1 << 30), (1, 1), (7, 60_000), (None, 1 << 30)]:
        ens = cof_class(m, p, n_neighbors=12, engine=engine, splits=splits, workspace_bytes=ws).fit(X)
        assert ws != 1 or len(ens.plan.chunks(901, ws)) == 9  # one chunk per subspace
        runs.append((ens.per_subspace_scores_, ens.decision_scores_, ens.ac_dist_, ens.score_ceiling_, ens.n_degenerate_,
                     *ens.decision_function(Y, return_per_subspace=True)))
    assert runs[0][4][8] == 0 and (runs[0][0][8] == 1).all() and (runs[0][2][8] == 0).all()
    for other in runs[1:]:
        for a, b in zip(runs[0], other):
            assert a.dtype == b.dtype and np.array_equal(a, b)


# ---- 6. what it detects ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", [5, 10, 20])
def test_planted_rows_score_above_every_held_out_inlier(k, cof_class, capsys):
    """Fit on normal rows, score new ones.  The planted rows break the correlation of features 0 and 1: they sit off a thin
    band, and their chain starts with one long edge.  The float64 restatement's margins: smallest planted score 9.1 .. 15.6
    against 1.6 .. 3.9 in [0, 1], 2.06 .. 4.6 against 1.7 .. 2.4 in [0, 1, 2] (the thinnest: 2.06 against 1.70 at k = 20)."""
    X = _planted()
    ens = cof_class(_mask(10, [[0, 1], [0, 1, 2]]), [0.5, 0.5], n_neighbors=k).fit(X[:1500])
    _, per = ens.decision_function(X, return_per_subspace=True)
    for s in range(2):
        planted, inliers = per[s, 2000:].astype(np.float64), per[s, 1500:2000].astype(np.float64)
        assert planted.min() > inliers.max(), (s, k, planted.min(), inliers.max())
        _report(capsys, f"k {k:2d} subspace {s}: smallest planted / largest inlier score {planted.min():.2f} / {inliers.max():.2f}"
                        f" = {planted.min() / inliers.max():.2f}")


# ---- 7. through the model --------------------------------------------------------------------------------------------------
def test_vgan_outlier_ensemble_cof_end_to_end(cof_class):
    import vgan_amd
    X = _planted()[:, :10]
    model = vgan_amd.VGAN_no_kl(epochs=2)
    model.fit(X)
    ens = model.outlier_ensemble(method="cof", n_neighbors=10, X=X)
    assert isinstance(ens, cof_class) and ens.n_neighbors == 10 and ens.chain == "sbn"
    S = model.subspaces.shape[0]
    per = ens.per_subspace_scores_
    assert per.shape == (S, X.shape[0]) and np.isfinite(per).all() and (per >= 0).all() and np.isfinite(ens.decision_scores_).all()
    assert (ens.decision_scores_ >= 0).all()
    assert ens.score_ceiling_.shape == (S,) and ens.n_degenerate_.shape == (S,) and ens.ac_dist_.shape == (S, X.shape[0])
    _check_scores(ens.decision_scores_, per, model.proba, None, None, "sum")
    D, I = ens.kneighbors()
    for s in range(min(S, 4)):
        feats = np.flatnonzero(model.subspaces[s])
        ac = restate_cof_chain(X, X, feats, I[s])[0]
        _check_ac(ens.ac_dist_[s], ac, len(feats), 10)
        _check_rows(per[s], restate_cof_from_lists(ac, ens.ac_dist_[s], I[s]), ens.score_ceiling_[s])
    ens = model.outlier_ensemble(method="cof", n_neighbors=5, chain="rank", normalize="robust", combination="max",
                                 contamination=0.05, X=X)
    assert ens.n_neighbors == 5 and ens.chain == "rank" and ens.normalize == "robust" and ens.combination == "max"
    c, w = _check_stats(ens, "robust")
    np.testing.assert_array_equal(c, restate_stats(ens.per_subspace_scores_, "robust")[0])
    _check_scores(ens.decision_scores_, ens.per_subspace_scores_, model.proba, c, w, "max")
    assert ens.threshold_ == np.percentile(ens.decision_scores_, 95.0)
    np.testing.assert_array_equal(ens.predict(X[:50]), (ens.decision_function(X[:50]) > ens.threshold_).astype(int))
    assert ens.predict_proba(X[:50]).shape == (50, 2)
    assert isinstance(model.outlier_ensemble(method="knn", X=X), vgan_amd.SubspaceEnsemble)
