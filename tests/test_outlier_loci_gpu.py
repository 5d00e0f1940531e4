"""The local correlation integral over the subspaces on the MI355X (csrc/outlier_loci.hip through vgan_amd.SubspaceLOCI and the ops
wrappers), against the numpy restatement of test_outlier_loci_cpu.py (pinned there to the scalar definition), never a second
run of the code under test.

Everything up to one division and one square root per (row, radius) is an integer, so the restatement runs on the very
float32 matrix the device used (keep_distance_matrix) and the counts and sums are compared as integers, exactly.  The scores
are compared within one float32 ulp (float64 division and square root are correctly rounded on either side; the ulp allows for
a last-place difference before the rounding to float32).  The best radius is compared wherever the restatement's two largest
ratios are equal or more than 1e-9 apart (relative); at most 1 % of a case's rows may be exempt.

Shapes.  The kernels give a subject row to a thread, 256 a workgroup; the sums sweep stages 64 rows of counts a tile and keeps
16 radii a pass, the counts sweep 32 radii a pass, the new-row sweep 32 radii a launch and 64 new rows a workgroup.  CASES walks
those edges: n = 2 (the smallest), 63 / 64 / 65 (the staged tile), 256 / 257 (a second workgroup), R = 1, 15 / 16 / 17 (the sums
pass), 31 / 32 / 33 (the counts pass and the new-row launch), 64 (the most: four and two passes).  New rows: 1 and 33, and 65
in the split test (a second workgroup of new rows).

The matrix, with eps32 = 2^-24 and d2_err the engine's bound on its squared distance (outlier_checks.d2_tolerance; the query of
entry D[c][q] is row q): |D^2 - d2| <= d2_err + 3 eps32 d2, as in the SOS tests."""
import numpy as np
import pytest

from outlier_checks import d2_tolerance
from test_outlier_gmm_gpu import D, MASK, PROBA, SIZES
from test_outlier_loci_cpu import (best_is_decided, micro_cluster, off_diagonal_max, restate_loci, restate_new_rows, restate_radii,
                                   roc_auc)
from test_outlier_norm_gpu import _check_scores, _check_stats
from test_outlier_ocsvm_cpu import restate_sq_dists, shifted_data

pytestmark = pytest.mark.gpu

# (n, R): see the header
CASES = [(2, 1), (63, 15), (64, 16), (65, 17), (256, 31), (257, 32), (257, 33), (65, 64)]
NEW_ROWS = (1, 33)
GRAM_MIN_DIMS = 32
EPS32 = 2.0 ** -24
PER_OCTAVE, ALPHA = 4.0, 0.5


def n_min_of(n):
    return min(5, n)


def features(s):
    return np.flatnonzero(MASK[s])


def engine_of(s):
    return "gram" if SIZES[s] >= GRAM_MIN_DIMS else "exact"


_DATA, _FIT = {}, {}


def case_data(n):
    """(X float32 [n, 70], Y float32 [65, 70]).  X: raw rows, columns scaled and offset, a twentieth shifted.  Y: fitted rows
    drawn at random and jittered by half a column sigma; the first 3 are exact copies of fitted rows, the next 2 lie 200 away in
    every feature (beyond r_max of everyone: no column spans more than a fifth of that)."""
    if n not in _DATA:
        X = shifted_data(n, D, seed=n, scale=True)
        rng = np.random.default_rng(7000 + n)
        Y = X[rng.integers(0, n, 65)].astype(np.float64)
        Y[3:] += 0.5 * X.std(axis=0) * rng.normal(size=(62, D))
        Y[3:5] += 200.0
        _DATA[n] = (X, np.ascontiguousarray(Y, dtype=np.float32))
    return _DATA[n]


def fitted(n, R):
    """(the fitted detector with its matrices and sums kept, the restatement on the device's own matrix per subspace), made once."""
    import vgan_amd
    if (n, R) not in _FIT:
        X, _ = case_data(n)
        ens = vgan_amd.SubspaceLOCI(MASK, PROBA, alpha=ALPHA, n_min=n_min_of(n), n_radii=R, radii_per_octave=PER_OCTAVE)
        ens.keep_distance_matrix = ens.keep_sums = True
        ens.fit(X)
        want = [restate_loci(ens.distance_matrix_[s], R, PER_OCTAVE, ALPHA, n_min_of(n)) for s in range(len(SIZES))]
        _FIT[n, R] = (ens, want)
    return _FIT[n, R]


def within_one_ulp(got, want):
    got, want = np.asarray(got), np.asarray(want)
    assert got.dtype == np.float32 and want.dtype == np.float32 and got.shape == want.shape
    return np.abs(got.astype(np.float64) - want.astype(np.float64)) <= np.spacing(np.maximum(np.abs(want), np.abs(got))).astype(np.float64)


def check_best(got, want):
    """The best radius of one subspace against the restatement's (a LociFit or LociRows), near-ties exempt (header)."""
    decided = best_is_decided(want.ratio)
    assert (~decided).sum() <= 0.01 * len(decided), int((~decided).sum())
    np.testing.assert_array_equal(got[decided], want.best[decided])


# ---- 1. the fit: integers, scores, best radius, radii -------------------------------------------------------------------------
@pytest.mark.parametrize("n,R", CASES)
def test_fit_is_the_restatement_on_the_devices_matrix(n, R):
    ens, want = fitted(n, R)
    S = len(SIZES)
    assert ens.radii_.dtype == np.float32 and ens.radii_.shape == (S, R)
    assert ens.neighbor_counts_.dtype == np.int32 and ens.neighbor_counts_.shape == (S, n, R)
    assert ens.sampling_counts_.dtype == np.int32 and ens.sum_counts_.dtype == np.int64 and ens.sum_sq_counts_.dtype == np.int64
    assert ens.sampling_counts_.shape == ens.sum_counts_.shape == ens.sum_sq_counts_.shape == (S, n, R)
    assert ens.best_radius_.dtype == np.int32 and ens.best_radius_.shape == (S, n)
    assert ens.per_subspace_scores_.dtype == np.float32 and ens.flagged_.dtype == bool and ens.n_flagged_.dtype == np.int64
    positive = 0
    for s in range(S):
        Dm, w = ens.distance_matrix_[s], want[s]
        assert Dm.dtype == np.float32 and Dm.shape == (n, n)
        # the radii, bit for bit from the device's r_max
        assert ens.radii_[s, -1] == off_diagonal_max(Dm)
        np.testing.assert_array_equal(ens.radii_[s], restate_radii(ens.radii_[s, -1], R, PER_OCTAVE, ALPHA)[0])
        np.testing.assert_array_equal(ens.radii_[s], w.r)
        np.testing.assert_array_equal(ens.neighbor_counts_[s], w.cnt)
        np.testing.assert_array_equal(ens.sampling_counts_[s], w.m)
        np.testing.assert_array_equal(ens.sum_counts_[s], w.S1)
        np.testing.assert_array_equal(ens.sum_sq_counts_[s], w.S2)
        assert within_one_ulp(ens.per_subspace_scores_[s], w.score).all()
        np.testing.assert_array_equal(ens.per_subspace_scores_[s] == 0, w.score == 0)
        check_best(ens.best_radius_[s], w)
        positive += int((w.score > 0).sum())
    assert positive > 0 or n == 2  # the cases are no empty comparison
    np.testing.assert_array_equal(ens.flagged_, ens.per_subspace_scores_.astype(np.float64) > 3.0)
    np.testing.assert_array_equal(ens.n_flagged_, ens.flagged_.sum(axis=1))
    np.testing.assert_allclose(ens.decision_scores_, PROBA @ ens.per_subspace_scores_.astype(np.float64), rtol=1e-12)


def test_kernels_take_the_diagonal_as_zero_and_name_their_row():
    """The ops entries on a host-made matrix that is not symmetric and whose diagonal holds numbers that must not count."""
    import torch
    from vgan_amd.ops import default_ops
    n, R, n_min = 130, 33, 4
    rng = np.random.default_rng(11)
    Dm = np.stack([rng.uniform(0.1, 3.0, (n, n)), np.round(rng.uniform(0, 4, (n, n)))]).astype(np.float32)  # the second: many ties
    for z in range(2):
        np.fill_diagonal(Dm[z], 9.0 if z == 0 else np.inf)
    want = []
    r, a = np.empty((2, R), np.float32), np.empty((2, R), np.float32)
    for z in range(2):
        want.append(restate_loci(Dm[z], R, PER_OCTAVE, ALPHA, n_min))
        r[z], a[z] = want[z].r, want[z].a
    ops = default_ops()
    dev, rd, ad = (torch.as_tensor(v).cuda() for v in (Dm, r, a))
    cnt, m = (torch.full((2, n, R), -1, dtype=torch.int32, device="cuda") for _ in range(2))
    S1, S2 = (torch.full((2, n, R), -1, dtype=torch.int64, device="cuda") for _ in range(2))
    ops.loci_counts(dev, ad, cnt)
    ops.loci_sums(dev, rd, cnt, m, S1, S2)
    score = torch.full((2, n), -1.0, dtype=torch.float32, device="cuda")
    best = torch.full((2, n), -7, dtype=torch.int32, device="cuda")
    ops.loci_finish(cnt, m, S1, S2, n_min, score, None, best)
    for z in range(2):
        for got, w in ((cnt, want[z].cnt), (m, want[z].m), (S1, want[z].S1), (S2, want[z].S2)):
            np.testing.assert_array_equal(got[z].cpu().numpy(), w)
        assert within_one_ulp(score[z].cpu().numpy(), want[z].score).all()
        check_best(best[z].cpu().numpy(), want[z])
    assert (want[1].score > 0).any()


# ---- 2. the matrix ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("engine", ["exact", "gram"])
@pytest.mark.parametrize("n", [2, 65, 257])
def test_distance_matrix_against_float64(n, engine):
    import vgan_amd
    X, _ = case_data(n)
    ens = vgan_amd.SubspaceLOCI(MASK, PROBA, n_min=n_min_of(n), n_radii=4, engine=engine)
    ens.keep_distance_matrix = True
    ens.fit(X)
    for s in range(len(SIZES)):
        Dm = ens.distance_matrix_[s]
        d2 = restate_sq_dists(X[:, features(s)], X[:, features(s)])
        err2 = d2_tolerance(engine, X, X, features(s), d2)
        if engine == "gram":
            err2 = err2.T  # the bound goes with the query row, and the query of D[c][q] is row q
        got = Dm.astype(np.float64)
        ok = np.abs(got * got - d2) <= err2 + 3 * EPS32 * d2
        np.fill_diagonal(ok, True)  # the diagonal is never read
        assert ok.all(), s


def test_distance_matrix_has_the_bits_of_the_sos_matrix():
    """vgan_loci_distance_matrix exists because SOS needs three rows; from there on the two write the same Euclidean entries."""
    import vgan_amd
    n = 65
    X, _ = case_data(n)
    ens, _ = fitted(n, 17)
    sos = vgan_amd.SubspaceSOS(MASK, PROBA, perplexity=4.5)
    sos.keep_distance_matrix = True
    sos.fit(X)
    off = ~np.eye(n, dtype=bool)
    for s in range(len(SIZES)):
        np.testing.assert_array_equal(ens.distance_matrix_[s][off], sos.distance_matrix_[s][off])


# ---- 3. new rows --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nq", NEW_ROWS)
@pytest.mark.parametrize("n,R", [(65, 17), (257, 33), (65, 64), (2, 1)])
def test_new_rows_are_the_restatement_on_the_devices_distances(n, R, nq):
    ens, want = fitted(n, R)
    X, Y = case_data(n)
    Y = Y[:nq] if nq > 1 else Y[5:6]
    scores, per, best = ens.decision_function(Y, return_per_subspace=True, return_best_radius=True)
    assert per.dtype == np.float32 and per.shape == (len(SIZES), nq) and best.dtype == np.int32 and best.shape == per.shape
    for s in range(len(SIZES)):
        d = ens.distance_rows(Y, s)
        assert d.dtype == np.float32 and d.shape == (nq, n)
        d2 = restate_sq_dists(Y[:, features(s)], X[:, features(s)])
        err2 = d2_tolerance(engine_of(s), Y, X, features(s), d2)
        got = d.astype(np.float64)
        assert (np.abs(got * got - d2) <= err2 + 3 * EPS32 * d2).all(), s
        new = restate_new_rows(d, want[s], n_min_of(n))
        sums = ens.row_sums(Y, s)
        for got, w in zip(sums, (new.A, new.M, new.T1, new.T2)):
            assert got.dtype == np.int64 and got.shape == (nq, R)
            np.testing.assert_array_equal(got, w)
        assert within_one_ulp(per[s], new.score).all()
        np.testing.assert_array_equal(per[s] == 0, new.score == 0)
        check_best(best[s], new)
    np.testing.assert_allclose(scores, PROBA @ per.astype(np.float64), rtol=1e-12)
    if nq > 1:
        # the rows beyond everyone's reach stand alone at every radius
        assert (per[:, 3:5] == 0).all() and (best[:, 3:5] == -1).all()
        # a row scored with others is the row scored alone
        alone = ens.decision_function(Y[7:8], return_per_subspace=True)[1]
        np.testing.assert_array_equal(alone[:, 0], per[:, 7])


def test_decision_function_of_the_fitted_rows_is_not_decision_scores():
    ens, _ = fitted(257, 32)
    X, _ = case_data(257)
    again = ens.decision_function(X, return_per_subspace=True)[1]
    assert again.shape == ens.per_subspace_scores_.shape and (again != ens.per_subspace_scores_).any()


# ---- 4. the same bits ---------------------------------------------------------------------------------------------------------
def test_results_are_the_same_bits_for_every_split_chunking_and_company():
    import vgan_amd
    from vgan_amd.outlier import loci_chunks
    n, R = 257, 33
    X, Y = case_data(n)

    def run(mask=MASK, proba=PROBA, **kw):
        ens = vgan_amd.SubspaceLOCI(mask, proba, n_min=5, n_radii=R, **kw)
        ens.keep_sums = True
        ens.fit(X)
        return ens, (ens.decision_scores_, ens.per_subspace_scores_, ens.best_radius_, ens.radii_, ens.neighbor_counts_,
                     ens.sampling_counts_, ens.sum_counts_, ens.sum_sq_counts_, ens.flagged_,
                     *ens.decision_function(Y, return_per_subspace=True, return_best_radius=True),
                     *ens.row_sums(Y, min(5, len(proba) - 1)))

    base_ens, base = run()
    assert len(loci_chunks(base_ens.plan, n, R, base_ens.workspace_bytes)) == 2
    tiny = dict(workspace_bytes=1)  # one subspace per chunk
    assert len(loci_chunks(base_ens.plan, n, R, 1)) == len(SIZES)
    for kw in ({}, dict(splits=1), dict(splits=3), tiny, dict(splits=5, **tiny)):  # {}: from one fit to the next
        for a, b in zip(base, run(**kw)[1]):
            np.testing.assert_array_equal(a, b)
    for s in (0, 5):  # one subspace of either engine, fitted alone
        alone = run(mask=MASK[s:s + 1], proba=[1.0])[1]
        for k in range(1, 9):
            np.testing.assert_array_equal(alone[k][0], base[k][s])
        for k in (10, 11):
            np.testing.assert_array_equal(alone[k][0], base[k][s])
        if s == 5:  # the integers of the new rows in that subspace
            for k in range(12, 16):
                np.testing.assert_array_equal(alone[k], base[k])


# ---- 5. degenerate input ------------------------------------------------------------------------------------------------------
def test_constant_subspaces_score_zero():
    import vgan_amd
    n = 65
    X = case_data(n)[0].copy()
    X[:, :40] = np.float32(2.7)
    mask = np.zeros((3, D), bool)
    mask[0, :3] = mask[1, :40] = mask[2, 38:45] = True  # constant on either engine, and a mixed one
    ens = vgan_amd.SubspaceLOCI(mask, [0.2, 0.3, 0.5], n_min=1).fit(X)
    assert (ens.radii_[:2] == 0).all() and (ens.radii_[2] > 0).all()
    assert (ens.neighbor_counts_[:2] == n).all()
    assert (ens.per_subspace_scores_[:2] == 0).all() and (ens.best_radius_[:2] == -1).all() and (ens.n_flagged_[:2] == 0).all()
    assert (ens.per_subspace_scores_[2] > 0).any()
    per, best = ens.decision_function(X[:7], return_per_subspace=True, return_best_radius=True)[1:]
    assert (per[:2] == 0).all() and (best[:2] == -1).all()


def test_duplicates_in_a_narrow_subspace_of_discrete_features():
    """The d_s = 1 subspace of rounded data: integers, so the exact engine's distances are exact and most radii cut between
    ties; the restatement runs on the distances formed on the host."""
    import vgan_amd
    n, R = 65, 32
    X = np.round(case_data(n)[0])
    ens = vgan_amd.SubspaceLOCI(MASK, PROBA, n_min=5, n_radii=R)
    ens.keep_distance_matrix = ens.keep_sums = True
    ens.fit(X)
    x = X[:, features(0)].astype(np.float64)
    host = np.abs(x - x.T).astype(np.float32)
    np.testing.assert_array_equal(ens.distance_matrix_[0], host)
    assert (host[~np.eye(n, dtype=bool)] == 0).sum() >= 2 * n  # duplicates
    want = restate_loci(host, R, PER_OCTAVE, ALPHA, 5)
    np.testing.assert_array_equal(ens.neighbor_counts_[0], want.cnt)
    np.testing.assert_array_equal(ens.sampling_counts_[0], want.m)
    np.testing.assert_array_equal(ens.sum_counts_[0], want.S1)
    np.testing.assert_array_equal(ens.sum_sq_counts_[0], want.S2)
    assert within_one_ulp(ens.per_subspace_scores_[0], want.score).all()
    check_best(ens.best_radius_[0], want)
    assert (want.den == 0).any() and (want.score > 0).any()


# ---- 6. the shared tail -------------------------------------------------------------------------------------------------------
def test_normalize_max_and_predict_go_through_the_shared_tail():
    import vgan_amd
    X, Y = case_data(257)
    ens = vgan_amd.SubspaceLOCI(MASK, PROBA, n_min=5, normalize="robust", combination="max", contamination=0.05).fit(X)
    per = ens.per_subspace_scores_
    c, w = _check_stats(ens, "robust")
    _check_scores(ens.decision_scores_, per, PROBA, c, w, "max")
    got, per_new = ens.decision_function(Y, return_per_subspace=True)
    _check_scores(got, per_new, PROBA, c, w, "max")
    assert ens.threshold_ == np.percentile(ens.decision_scores_, 95.0)
    np.testing.assert_array_equal(ens.labels_, (ens.decision_scores_ > ens.threshold_).astype(int))
    np.testing.assert_array_equal(ens.predict(Y), (got > ens.threshold_).astype(int))
    assert ens.predict_proba(Y).shape == (len(Y), 2)


def test_vgan_outlier_ensemble_loci_end_to_end():
    import vgan_amd
    from test_outlier_gpu import _planted
    X = _planted()[:, :10]
    model = vgan_amd.VGAN_no_kl(epochs=5)
    model.fit(X)
    X = np.ascontiguousarray(X[-600:])
    ens = model.outlier_ensemble(method="loci", n_radii=16, subspace_count=200, X=X)
    assert type(ens) is vgan_amd.SubspaceLOCI and ens._fitted
    S = model.subspaces.shape[0]
    assert ens.decision_scores_.shape == (600,) and np.isfinite(ens.decision_scores_).all()
    assert (ens.per_subspace_scores_ >= 0).all() and ens.radii_.shape == (S, 16) and ens.neighbor_counts_.shape == (S, 600, 16)
    assert ((ens.best_radius_ >= -1) & (ens.best_radius_ < 16)).all() and ens.flagged_.shape == (S, 600)
    assert ens.decision_function(X[:9]).shape == (9,)


# ---- 7. the recipe ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", range(3))
def test_micro_cluster_is_found_by_loci_and_missed_by_lof_on_the_device(seed):
    import vgan_amd
    X, y = micro_cluster(seed)
    mask = np.ones((1, X.shape[1]), bool)
    ens = vgan_amd.SubspaceLOCI(mask, [1.0]).fit(X)
    lof = vgan_amd.SubspaceEnsemble(mask, [1.0], method="lof", n_neighbors=32).fit(X)
    auc, lof_auc = roc_auc(y, ens.decision_scores_), roc_auc(y, lof.decision_scores_)
    print(f"seed {seed}: device LOCI AUC {auc:.4f}, device LOF(32) AUC {lof_auc:.3f}, flagged outliers {ens.flagged_[0][y == 1].sum()} / 50, "
          f"inliers {ens.flagged_[0][y == 0].sum()} / 950")
    assert auc >= 0.99
    assert lof_auc <= 0.6
    assert ens.flagged_[0][y == 1].all() and ens.n_flagged_[0] == ens.flagged_[0].sum()
