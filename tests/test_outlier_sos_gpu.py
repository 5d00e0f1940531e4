"""Stochastic outlier selection over the subspaces on the MI355X (csrc/outlier_sos.hip through vgan_amd.SubspaceSOS and the ops
wrappers), against the numpy restatement of test_outlier_sos_cpu.py (pinned there to the scalar definition and to sklearn),
never a second run of the code under test.

The search.  Rounding the dissimilarity matrix to float32 moves beta, so every exact comparison runs the restatement on the
very float32 D the device used.  The updates of beta are exact (doublings and means), so beta and the step count are compared
bit for bit; the device's exp and log may differ from numpy's in the last place, which can flip a comparison only where some
step's |diff| lies within 1e-12 of 0 or of tol.  The restatement flags such rows; they are exempt from the bit comparison but,
like every non-degenerate row, must meet |H - log(perplexity)| <= tol + 1e-12 recomputed in numpy from the device's beta.  On
host-made matrices no row may be flagged.  Z is compared with its numpy recomputation at the device's beta at relative n 2^-50
(n terms in (0, 1], each exp within an ulp or two, any order of the sum).

The matrix, with eps32 = 2^-24 and d2_err the engine's bound on its squared distance (outlier_checks.d2_tolerance; the query
of entry D[i, j] is row j): |D - d2| <= d2_err + eps32 d2 for "sqeuclidean" (one float32 rounding), |D^2 - d2| <= d2_err + 3 eps32 d2
for "euclidean" (sqrtf's one rounding doubles on squaring, plus the float32 rounding of d2).

A score is exp(-sum_i t_i).  A dissimilarity that moves by delta moves log a_i by beta_i delta, so a_i and a_i / Z_i by that
relative amount; the term t_i = -log1p(-b), b = a_i / Z_i, has dt / db = 1 / (1 - b), so it moves by kbar_i = beta_i delta b / (1 - b).
For a new row t_i = log1p(a_i / Z_i) and b = a_i / (Z_i + a_i), b / (1 - b) = a_i / Z_i, which bounds the move of that term too.  delta
is the move of d under d2_err: the larger of sqrt(d2 + d2_err) - d and d - sqrt(max(d2 - d2_err, 0)), plus eps32 d for sqrtf; d2_err +
eps32 d2 for "sqeuclidean".  Z enters as recomputed in numpy (relative n 2^-50, far below the grid).  The bar of a row's score:
score (sum_i kbar_i + n 2^-40) + 2^-23 score, the moves, the fixed-point grid of n terms and the float32 result.  A term at the
128 clamp puts the score below float32's smallest subnormal number: such a score, bar included, must come out as exactly 0,
and every other comparison allows for the spacing of those numbers, 2^-149."""
import numpy as np
import pytest

from outlier_checks import d2_tolerance
from test_outlier_gmm_gpu import D, MASK, PROBA, SIZES
from test_outlier_norm_gpu import _check_scores, _check_stats
from test_outlier_ocsvm_cpu import planted_data, ranking_rate, restate_sq_dists, shifted_data
from test_outlier_sos_cpu import entropy_gap, off_diagonal, restate_sos_fit, restate_sos_scores, restate_sos_terms

pytestmark = pytest.mark.gpu

ROWS = [3, 63, 65, 255, 257, 1025]  # the smallest, the 64-row tile edges, the 256-thread edges, several strided passes
CASES = [(3, 1.5)] + [(n, p) for n in ROWS[1:] for p in (4.5, 30.0)]
NEW_ROWS = 130
GRAM_MIN_DIMS = 32
TOL, MAX_ITER = 1e-5, 200
EPS32 = 2.0 ** -24


def features(s):
    return np.flatnonzero(MASK[s])


def engine_of(s):
    return "gram" if SIZES[s] >= GRAM_MIN_DIMS else "exact"


_DATA, _D2, _HOST, _WANT = {}, {}, {}, {}


def case_data(n):
    """(X float32 [n, 70], Y float32 [130, 70]).  X: raw rows, columns scaled by factors in [0.5, 2] and offset, a twentieth
    shifted.  Y: fitted rows drawn at random and jittered by half a column sigma; the first 5 are exact copies of fitted rows
    (dissimilarity 0 to one of them), the next 3 lie 20 away in every feature (bound by nobody)."""
    if n not in _DATA:
        X = shifted_data(n, D, seed=n, scale=True)
        rng = np.random.default_rng(5000 + n)
        Y = X[rng.integers(0, n, NEW_ROWS)].astype(np.float64)
        Y[5:] += 0.5 * X.std(axis=0) * rng.normal(size=(NEW_ROWS - 5, D))
        Y[5:8] += 20.0
        _DATA[n] = (X, np.ascontiguousarray(Y, dtype=np.float32))
    return _DATA[n]


def sq_dists(n, s):
    """(d2 of the fitted rows among themselves, d2 of the new rows against them), float64, made once."""
    if (n, s) not in _D2:
        X, Y = case_data(n)
        _D2[n, s] = (restate_sq_dists(X[:, features(s)], X[:, features(s)]), restate_sq_dists(Y[:, features(s)], X[:, features(s)]))
    return _D2[n, s]


def host_matrices(n):
    """float32 [S, n, n]: float32(sqrt(d2)) per subspace, made on the host."""
    if n not in _HOST:
        _HOST[n] = np.stack([np.sqrt(sq_dists(n, s)[0]).astype(np.float32) for s in range(len(SIZES))])
    return _HOST[n]


def host_fit(n, perplexity, s):
    if (n, perplexity, s) not in _WANT:
        _WANT[n, perplexity, s] = restate_sos_fit(host_matrices(n)[s], perplexity, TOL, MAX_ITER)
    return _WANT[n, perplexity, s]


def search(Dm, perplexity, storage="auto", tol=TOL, max_iter=MAX_ITER):
    """(beta, dmin, Z, n_iter, flags) [S, n] of vgan_sos_fit on the uploaded matrices Dm [S, n, n]."""
    import torch
    from vgan_amd import outlier
    from vgan_amd.ops import default_ops
    S, n = Dm.shape[0], Dm.shape[1]
    dev = torch.as_tensor(np.ascontiguousarray(Dm)).cuda()
    beta, dmin, Z = (torch.full((S, n), -1.0, dtype=torch.float64, device="cuda") for _ in range(3))
    n_iter, flags = (torch.full((S, n), -1, dtype=torch.int32, device="cuda") for _ in range(2))
    default_ops().sos_fit(dev, perplexity, tol, max_iter, beta, dmin, Z, n_iter, flags, outlier.SOS_STORAGE[storage])
    return tuple(v.cpu().numpy() for v in (beta, dmin, Z, n_iter, flags))


def recomputed_Z(Dm, beta, dmin):
    """float64 [n]: sum_j exp(-(beta (D[i, j] - dmin))) over j != i at the given beta (nan where beta is inf)."""
    E = off_diagonal(np.asarray(Dm)).astype(np.float64) - dmin[:, None]
    with np.errstate(invalid="ignore"):
        return np.exp(-(beta[:, None] * E)).sum(axis=1)


def check_search(got, want, Dm, perplexity, exempt_allowed, tol=TOL):
    """One subspace: got = (beta, dmin, Z, n_iter, flags) [n] of the device against the restatement on the same matrix Dm."""
    beta, dmin, Z, n_iter, flags = got
    n = Dm.shape[0]
    np.testing.assert_array_equal(flags == 1, want.degenerate)
    np.testing.assert_array_equal(dmin, want.dmin)
    exempt = want.flagged
    assert exempt.sum() <= (exempt_allowed * n), ("flagged rows", np.flatnonzero(exempt))
    keep = ~exempt
    np.testing.assert_array_equal(beta[keep], want.beta[keep])
    np.testing.assert_array_equal(n_iter[keep], want.n_iter[keep])
    np.testing.assert_array_equal((flags == 2)[keep], want.unconverged[keep])
    searched = ~want.degenerate
    assert (Z[want.degenerate] == want.Z[want.degenerate]).all() and (n_iter[want.degenerate] == 0).all()
    converged = searched & (flags == 0)
    fit = want._replace(beta=beta, dmin=dmin)
    gap = entropy_gap(Dm, fit, perplexity)
    assert (gap[converged] <= tol + 1e-12).all(), float(np.nanmax(gap[converged]))
    Zn = recomputed_Z(Dm, beta, dmin)
    assert (np.abs(Z - Zn)[searched] <= n * 2.0 ** -50 * Zn[searched]).all(), float((np.abs(Z - Zn) / Zn)[searched].max())


# ---- 1. the search on host-made matrices ------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,perplexity", CASES)
def test_search_is_the_restatement_bit_for_bit(n, perplexity):
    Dm = host_matrices(n)
    got = search(Dm, perplexity)
    assert (got[4] != 2).all()  # no unconverged row
    for s in range(len(SIZES)):
        want = host_fit(n, perplexity, s)
        assert not want.unconverged.any() and want.n_iter.max() <= 40
        check_search([v[s] for v in got], want, Dm[s], perplexity, exempt_allowed=0)


# ---- 2. the storage edge ----------------------------------------------------------------------------------------------------
def test_search_bits_do_not_depend_on_who_owns_a_row():
    from vgan_amd import outlier
    from vgan_amd.lib import VganHipError
    # both forms wherever both apply: every subspace of a small case
    n, perplexity = 257, 4.5
    Dm = host_matrices(n)
    wave, block = search(Dm, perplexity, "wave"), search(Dm, perplexity, "block")
    for a, b in zip(wave[:2] + wave[3:], block[:2] + block[3:]):  # beta, dmin, n_iter, flags: the same bits
        np.testing.assert_array_equal(a, b)
    assert (np.abs(wave[2] - block[2]) <= n * 2.0 ** -50 * wave[2]).all()  # Z: the order of the sum is each form's own
    # the edge of "auto": 2048 rows belong to a wave each (and to a workgroup: the same bits), 2049 to a workgroup
    assert outlier.SOS_WAVE_ROWS == 2048
    Zd = shifted_data(2049, 5, seed=5).astype(np.float64)
    big = np.sqrt(restate_sq_dists(Zd, Zd)).astype(np.float32)
    edge = np.ascontiguousarray(big[None, :2048, :2048])
    for perplexity in (4.5, 30.0):
        want = restate_sos_fit(edge[0], perplexity, TOL, MAX_ITER)
        auto, forced = search(edge, perplexity), search(edge, perplexity, "block")
        check_search([v[0] for v in auto], want, edge[0], perplexity, exempt_allowed=0)
        check_search([v[0] for v in forced], want, edge[0], perplexity, exempt_allowed=0)
        np.testing.assert_array_equal(auto[0], search(edge, perplexity, "wave")[0])
        want = restate_sos_fit(big, perplexity, TOL, MAX_ITER)
        check_search([v[0] for v in search(big[None], perplexity)], want, big, perplexity, exempt_allowed=0)
    with pytest.raises(VganHipError, match="bad argument"):
        search(big[None], 4.5, "wave")


def test_max_iter_cuts_the_search_off_on_the_device():
    n, perplexity = 65, 4.5
    Dm = host_matrices(n)
    got = search(Dm, perplexity, max_iter=3)
    for s in range(len(SIZES)):
        want = restate_sos_fit(Dm[s], perplexity, TOL, 3)
        assert want.unconverged.any() and want.n_iter.max() == 3
        check_search([v[s] for v in got], want, Dm[s], perplexity, exempt_allowed=0)


# ---- 3. the matrix ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("metric", ["euclidean", "sqeuclidean"])
@pytest.mark.parametrize("engine", ["exact", "gram"])
@pytest.mark.parametrize("n", [3, 65, 257])
def test_distance_matrix_against_float64(n, engine, metric):
    import vgan_amd
    X, _ = case_data(n)
    ens = vgan_amd.SubspaceSOS(MASK, PROBA, perplexity=1.5 if n == 3 else 4.5, metric=metric, engine=engine)
    ens.keep_distance_matrix = True
    ens.fit(X)
    for s in range(len(SIZES)):
        Dm = ens.distance_matrix_[s]
        assert Dm.dtype == np.float32 and Dm.shape == (n, n)
        d2 = sq_dists(n, s)[0]
        err2 = d2_tolerance(engine, X, X, features(s), d2)
        if engine == "gram":
            err2 = err2.T  # the bound goes with the query row, and the query of D[i, j] is row j
        got = Dm.astype(np.float64)
        if metric == "euclidean":
            err, bar = np.abs(got * got - d2), err2 + 3 * EPS32 * d2
        else:
            err, bar = np.abs(got - d2), err2 + EPS32 * d2
        ok = err <= bar
        np.fill_diagonal(ok, True)  # the diagonal is never read
        assert ok.all(), (s, float((err / np.maximum(bar, 1e-300))[~ok].max()))


# ---- 4. end to end ----------------------------------------------------------------------------------------------------------
def move_of_d(metric, d2, err2):
    """(d, delta): the float64 dissimilarity and the bound on the device's move of it (header)."""
    if metric == "sqeuclidean":
        return d2, err2 + EPS32 * d2
    d = np.sqrt(d2)
    return d, np.maximum(np.sqrt(d2 + err2) - d, d - np.sqrt(np.maximum(d2 - err2, 0.0))) + EPS32 * d


def check_scores(got, beta, dmin, Z, metric, engine, Xq, Xr, s, d2, fitting):
    """The device's float32 scores got [nq] against the restatement from the fitted state and float64 dissimilarities."""
    n = len(beta)
    err2 = d2_tolerance(engine, Xq, Xr, features(s), d2)
    if fitting and engine == "gram":
        err2 = err2.T  # at fit row j reads D[j, i], the engine's value with row i as the query: the bound goes with the column
    d, delta = move_of_d(metric, d2, np.broadcast_to(err2, d2.shape))
    want = restate_sos_scores(d, beta, dmin, Z, fitting)
    t = restate_sos_terms(d, beta, dmin, Z, fitting)
    deg = np.isinf(beta)
    with np.errstate(over="ignore", invalid="ignore"):
        # b / (1 - b) = expm1(t) in either form: t = -log(1 - b) at fit, t = log(1 + a / Z) for a new row
        kbar = np.where(deg[None, :], 0.0, np.where(deg, 0.0, beta)[None, :] * delta * np.expm1(t))
    # a degenerate fitted row's affinity is a step at dmin: a pair within delta of it could fall on either side; none of the
    # cases that come here has one (asserted), so those terms move by nothing
    near_step = (np.abs(d - dmin[None, :]) <= delta) & deg[None, :] & (d != dmin[None, :])
    if fitting:
        np.fill_diagonal(kbar, 0.0)
        np.fill_diagonal(near_step, False)
    assert not near_step.any()
    bar = want * (kbar.sum(axis=1) + n * 2.0 ** -40) + 2.0 ** -23 * want
    got = np.asarray(got, np.float64)
    assert got.shape == want.shape and np.isfinite(bar).all()
    # float32 holds nothing below 2^-149: a score that stays under half of that with its whole bar, a term at the 128 clamp
    # among them, is an exact zero; elsewhere the spacing of float32's subnormal numbers joins the bar
    zero = want + bar < 2.0 ** -150
    assert (got[zero] == 0.0).all()
    err = np.abs(got - want)
    bar = bar + 2.0 ** -149
    assert (err <= bar)[~zero].all(), (s, float((err / bar)[~zero].max()))
    return float((err / bar)[~zero].max()) if (~zero).any() else 0.0


def check_fit_end_to_end(ens, X, Y, n, perplexity, metric="euclidean"):
    per_new = ens.decision_function(Y, return_per_subspace=True)[1]
    assert ens.beta_.dtype == np.float64 and ens.beta_.shape == (len(SIZES), n)
    assert ens.n_iter_.dtype == np.int32 and ens.n_iter_.shape == (len(SIZES), n)
    assert ens.n_degenerate_.dtype == np.int64 and ens.n_unconverged_.dtype == np.int64
    assert ens.per_subspace_scores_.dtype == np.float32 and per_new.shape == (len(SIZES), NEW_ROWS)
    dmin_dev, Z_dev = (v.cpu().numpy()[ens.plan.given] for v in (ens._dmin, ens._Z))
    worst = 0.0
    for s in range(len(SIZES)):
        Dm = ens.distance_matrix_[s]
        want = restate_sos_fit(Dm, perplexity, TOL, MAX_ITER)
        flags = np.where(np.isinf(ens.beta_[s]), 1, 0)  # the class publishes the counts: no row is unconverged (asserted)
        assert ens.n_unconverged_[s] == 0 == want.unconverged.sum() and ens.n_degenerate_[s] == want.degenerate.sum()
        check_search((ens.beta_[s], dmin_dev[s], Z_dev[s], ens.n_iter_[s], flags), want, Dm, perplexity, exempt_allowed=1)
        # the scores from the published beta, the row minima of the device's matrix and Z recomputed in numpy
        beta, dmin = ens.beta_[s], want.dmin
        Z = np.where(want.degenerate, want.Z, recomputed_Z(Dm, beta, dmin))
        d2_fit, d2_new = sq_dists(n, s)
        worst = max(worst, check_scores(ens.per_subspace_scores_[s], beta, dmin, Z, metric, engine_of(s), X, X, s, d2_fit, True))
        worst = max(worst, check_scores(per_new[s], beta, dmin, Z, metric, engine_of(s), Y, X, s, d2_new, False))
    np.testing.assert_allclose(ens.decision_scores_, PROBA @ ens.per_subspace_scores_.astype(np.float64), rtol=1e-12)
    print(f"n={n} perplexity={perplexity} {metric}: largest share of the score bar {worst:.3g}")


@pytest.mark.parametrize("n,perplexity", CASES)
def test_fit_end_to_end(n, perplexity):
    import vgan_amd
    X, Y = case_data(n)
    ens = vgan_amd.SubspaceSOS(MASK, PROBA, perplexity=perplexity)
    ens.keep_distance_matrix = True
    ens.fit(X)
    check_fit_end_to_end(ens, X, Y, n, perplexity)
    # decision_function(X_train) is not decision_scores_: there every row meets itself at dissimilarity 0
    again = ens.decision_function(X, return_per_subspace=True)[1]
    assert (again != ens.per_subspace_scores_).any()


# ---- 5. the same bits -------------------------------------------------------------------------------------------------------
def test_results_are_the_same_bits_for_every_split_chunking_and_company():
    import vgan_amd
    from vgan_amd.outlier import sos_chunks
    n, perplexity = 257, 4.5
    X, Y = case_data(n)

    def run(mask=MASK, proba=PROBA, **kw):
        ens = vgan_amd.SubspaceSOS(mask, proba, perplexity=perplexity, **kw).fit(X)
        return ens, (ens.decision_scores_, ens.per_subspace_scores_, ens.beta_, ens.n_iter_, ens.n_degenerate_,
                     *ens.decision_function(Y, return_per_subspace=True))

    base_ens, base = run()
    assert len(sos_chunks(base_ens.plan, n, base_ens.workspace_bytes)) == 2
    tiny = dict(workspace_bytes=1)  # one subspace per chunk
    assert len(sos_chunks(base_ens.plan, n, 1)) == len(SIZES)
    for kw in ({}, dict(splits=1), dict(splits=3), tiny, dict(splits=3, **tiny)):  # {}: from one fit to the next
        for a, b in zip(base, run(**kw)[1]):
            np.testing.assert_array_equal(a, b)
    for s in (0, 5):  # one subspace of either engine, fitted alone
        alone = run(mask=MASK[s:s + 1], proba=[1.0])[1]
        for k in (1, 2, 3, 6):
            np.testing.assert_array_equal(alone[k][0], base[k][s])


# ---- 6. degenerate input ----------------------------------------------------------------------------------------------------
def test_constant_subspaces_score_the_constant():
    import vgan_amd
    from vgan_amd.outlier import sos_constant_score
    n = 65
    X = case_data(n)[0].copy()
    X[:, :40] = np.float32(2.7)
    mask = np.zeros((3, D), bool)
    mask[0, :3] = mask[1, :40] = mask[2, 38:45] = True  # constant on either engine, and a mixed one
    ens = vgan_amd.SubspaceSOS(mask, [0.2, 0.3, 0.5]).fit(X)
    assert list(ens.n_degenerate_) == [n, n, 0] and (ens.n_unconverged_ == 0).all()
    assert np.isinf(ens.beta_[:2]).all() and (ens.n_iter_[:2] == 0).all() and np.isfinite(ens.beta_[2]).all()
    want = restate_sos_scores(np.zeros((n, n)), np.full(n, np.inf), np.zeros(n), np.full(n, n - 1.0), True)
    np.testing.assert_array_equal(ens.per_subspace_scores_[:2], np.broadcast_to(want.astype(np.float32), (2, n)))
    assert ens.per_subspace_scores_[0, 0] == pytest.approx(sos_constant_score(n), rel=2.0 ** -22)
    new = restate_sos_scores(np.zeros((7, n)), np.full(n, np.inf), np.zeros(n), np.full(n, n - 1.0), False)
    np.testing.assert_array_equal(ens.decision_function(X[:7], return_per_subspace=True)[1][:2], np.broadcast_to(new.astype(np.float32), (2, 7)))


def test_duplicates_in_a_narrow_subspace_take_the_degenerate_rule():
    """The d_s = 1 subspace of rounded data: most rows have at least five others at dissimilarity 0."""
    import vgan_amd
    n, perplexity = 65, 4.5
    X = np.round(case_data(n)[0])
    ens = vgan_amd.SubspaceSOS(MASK, PROBA, perplexity=perplexity)
    ens.keep_distance_matrix = True
    ens.fit(X)
    Dm = ens.distance_matrix_[0]
    want = restate_sos_fit(Dm, perplexity, TOL, MAX_ITER)
    assert want.degenerate.sum() >= 40 and not want.degenerate.all()
    assert ens.n_degenerate_[0] == want.degenerate.sum() and ens.n_unconverged_[0] == 0
    np.testing.assert_array_equal(np.isinf(ens.beta_[0]), want.degenerate)
    keep = ~want.flagged
    np.testing.assert_array_equal(ens.beta_[0][keep], want.beta[keep])
    # integers in float32: the exact engine's d2 and its square root are exact, so the scores follow from the restated state
    x = X[:, features(0)].astype(np.float64)
    d = np.abs(x - x.T)
    np.testing.assert_array_equal(Dm, d.astype(np.float32))
    Z = np.where(want.degenerate, want.Z, recomputed_Z(Dm, ens.beta_[0], want.dmin))
    ref = restate_sos_scores(d, ens.beta_[0], want.dmin, Z, True)
    np.testing.assert_allclose(ens.per_subspace_scores_[0], ref, rtol=n * 2.0 ** -40 + 2.0 ** -23, atol=1e-45)


# ---- 7. the paper's metric --------------------------------------------------------------------------------------------------
def test_fit_end_to_end_sqeuclidean():
    import vgan_amd
    n, perplexity = 257, 4.5
    X, Y = case_data(n)
    ens = vgan_amd.SubspaceSOS(MASK, PROBA, perplexity=perplexity, metric="sqeuclidean")
    ens.keep_distance_matrix = True
    ens.fit(X)
    check_fit_end_to_end(ens, X, Y, n, perplexity, metric="sqeuclidean")


# ---- 8. the shared tail -----------------------------------------------------------------------------------------------------
def test_normalize_max_and_predict_go_through_the_shared_tail():
    import vgan_amd
    X, Y = case_data(257)
    ens = vgan_amd.SubspaceSOS(MASK, PROBA, normalize="robust", combination="max", contamination=0.05).fit(X)
    per = ens.per_subspace_scores_
    c, w = _check_stats(ens, "robust")
    _check_scores(ens.decision_scores_, per, PROBA, c, w, "max")
    got, per_new = ens.decision_function(Y, return_per_subspace=True)
    _check_scores(got, per_new, PROBA, c, w, "max")
    assert ens.threshold_ == np.percentile(ens.decision_scores_, 95.0)
    np.testing.assert_array_equal(ens.labels_, (ens.decision_scores_ > ens.threshold_).astype(int))
    np.testing.assert_array_equal(ens.predict(Y), (got > ens.threshold_).astype(int))
    assert ens.predict_proba(Y).shape == (NEW_ROWS, 2)


def test_vgan_outlier_ensemble_sos_end_to_end():
    import vgan_amd
    from test_outlier_gpu import _planted
    X = _planted()[:, :10]
    model = vgan_amd.VGAN_no_kl(epochs=5)
    model.fit(X)
    X = np.ascontiguousarray(X[-600:])
    ens = model.outlier_ensemble(method="sos", perplexity=10.0, subspace_count=200, X=X)
    assert type(ens) is vgan_amd.SubspaceSOS and ens._fitted
    assert ens.decision_scores_.shape == (600,) and np.isfinite(ens.decision_scores_).all()
    assert ((ens.per_subspace_scores_ >= 0) & (ens.per_subspace_scores_ <= 1)).all()
    assert ens.beta_.shape == (model.subspaces.shape[0], 600) and (ens.n_unconverged_ == 0).all()
    assert ens.decision_function(X[:9]).shape == (9,)


# ---- 9. planted outliers ----------------------------------------------------------------------------------------------------
def test_planted_outliers_rank_on_top_at_the_restatements_rate():
    """The device's rate is compared with the restatement's on the device's own D, never with a fixed number; a row whose
    reference score lies within twice the score bar of the cut may fall on either side of it."""
    import vgan_amd
    n, perplexity = 1025, 4.5
    X, rows = planted_data(n, D, seed=3)
    ens = vgan_amd.SubspaceSOS(MASK, PROBA, perplexity=perplexity)
    ens.keep_distance_matrix = True
    ens.fit(X)
    k = len(rows)
    rates = []
    for s in (0, 2, 5, 7):  # 1, 16, 64 and 70 features: both engines
        Dm = ens.distance_matrix_[s]
        want = restate_sos_fit(Dm, perplexity, TOL, MAX_ITER)
        d2 = restate_sq_dists(X[:, features(s)], X[:, features(s)])
        d, delta = move_of_d("euclidean", d2, np.broadcast_to(d2_tolerance(engine_of(s), X, X, features(s), d2), d2.shape))
        ref = restate_sos_scores(d, want.beta, want.dmin, want.Z, True)
        t = restate_sos_terms(d, want.beta, want.dmin, want.Z, True)
        with np.errstate(over="ignore", invalid="ignore"):
            kbar = np.where(np.isinf(want.beta)[None, :], 0.0, np.where(np.isinf(want.beta), 0.0, want.beta)[None, :] * delta * np.expm1(t))
        np.fill_diagonal(kbar, 0.0)
        bar = ref * (kbar.sum(axis=1) + n * 2.0 ** -40) + 2.0 ** -23 * ref
        cut = np.sort(ref)[-k]
        near = int((np.abs(ref - cut) <= 2 * bar).sum()) - 1  # rows other than the k-th itself that may cross the cut
        got, base = ranking_rate(ens.per_subspace_scores_[s], rows), ranking_rate(ref, rows)
        print(f"d_s={SIZES[s]}: device {got:.3f}, restatement {base:.3f}, rows near the cut {near}")
        assert abs(got - base) <= near / k, (s, got, base, near)
        rates.append(base)
    assert max(rates) > 0.9  # the wide subspaces find them
