"""Mahalanobis / MCD scores over the subspaces on the MI355X (csrc/outlier_maha.hip through vgan_amd.SubspaceMahalanobis),
against the float64 restatement of test_outlier_maha_cpu.py (pinned there to sklearn), never a second run of the code under
test.

Bars, with u = 2^-53.  Moments: |C - want| <= 4 h u (sum_i |z_ia z_ib| / h) per element, the order-independent summation bound
with a factor 4 of slack (the mean likewise on |x|).  Factor: W lower triangular with a positive diagonal and max |W Sigma
W^T - I| <= 8 d_s kappa u, kappa = cond(Sigma) from numpy; shrinkage_ within 1e-12 relative.  Scores: one float32 ulp, |got -
want32| <= 2^-23 |want32|, and exactly 0 where want is 0.  That bar is derived, not measured: the float64 error of moments,
factor and product is of order h d_s kappa u, and every case asserts on its input that h d_s kappa u < 2^-30, so that only
the final rounding to float32 can differ.  Supports, step counts and flags are compared exactly; the planted cases assert
first that no selection of the restatement hinges on a gap below 2^-18 relative."""
import numpy as np
import pytest

from test_outlier_maha_cpu import (MIN_GAP, PLANTED, planted_shift, raw_data, restate_alpha, restate_estimate, restate_fit,
                                   restate_moments, restate_shrunk, select_support, separation_ratio)
from test_outlier_norm_gpu import _check_scores, _check_stats

pytestmark = pytest.mark.gpu

U = 2.0 ** -53
D = 140
SIZES = [1, 3, 4, 15, 16, 17, 33, 67, 130]  # the edges of the 4-deep K and the 16-wide tiles
CONST, DUP = 5, (7, 11)  # a constant column; column 11 repeats column 7
ROWS = [2, 63, 64, 65, 257, 2 * 1024 + 3]  # the last: two moment slabs + 3


def edge_mask():
    """bool [9, 140]: the subspace of one feature is the constant column, the one of three the constant column and both
    copies of the duplicated feature, and every wider one holds those three among its features."""
    rng = np.random.default_rng(0)
    forced = [CONST, DUP[0], DUP[1]]
    rest = np.setdiff1d(np.arange(D), forced)
    m = np.zeros((len(SIZES), D), bool)
    for s, size in enumerate(SIZES):
        m[s, forced[:size]] = True
        if size > 3:
            m[s, rng.choice(rest, size - 3, replace=False)] = True
    assert list(m.sum(axis=1)) == SIZES
    return m


MASK = edge_mask()
PROBA = np.arange(1, len(SIZES) + 1) / np.arange(1, len(SIZES) + 1).sum()


def features(mask, s):
    return np.flatnonzero(mask[s])


def assert_one_ulp(got, want32):
    assert got.dtype == np.float32 and want32.dtype == np.float32 and got.shape == want32.shape
    err = np.abs(got.astype(np.float64) - want32.astype(np.float64))
    assert (err <= 2.0 ** -23 * np.abs(want32.astype(np.float64))).all(), float(err.max())
    assert (got[want32 == 0] == 0).all()


def assert_well_conditioned(est):
    """The condition on the input under which one float32 ulp is the bar: h d kappa u < 2^-30."""
    d = est["Sigma"].shape[0]
    if est["L"] is None:
        return
    kappa = np.linalg.cond(est["Sigma"])
    assert est["h"] * d * kappa * U < 2.0 ** -30, (est["h"], d, kappa)


@pytest.fixture(scope="module")
def data():
    return {n: raw_data(n, D, seed=n, constant=CONST, duplicate=DUP) for n in ROWS}


@pytest.fixture(scope="module")
def fitted(data):
    """n -> the ensemble over MASK fitted on data[n] with the default shrinkage, once for the module."""
    import vgan_amd
    cache = {}

    def get(n):
        if n not in cache:
            cache[n] = vgan_amd.SubspaceMahalanobis(MASK, PROBA).fit(data[n])
        return cache[n]
    return get


def prepared(mask, X, **kw):
    """(ensemble, X on the device) with the tables and buffers of fit in place and nothing estimated yet."""
    import vgan_amd
    ens = vgan_amd.SubspaceMahalanobis(mask, np.full(mask.shape[0], 1.0 / mask.shape[0]), **kw)
    Xd = ens._begin_fit(X)
    ens._prepare(X.shape[0], Xd.device)
    return ens, Xd


def device_moments(ens, Xd, support):
    """Runs the moment kernels; returns (hcount tensor, list of mu, list of C) as the device left them."""
    import torch
    S, n = ens.plan.count, Xd.shape[0]
    sup = None if support is None else torch.as_tensor(support.astype(np.uint8), device=Xd.device)
    h = np.full(S, n) if support is None else support.sum(axis=1)
    hcount = torch.as_tensor(h.astype(np.int32), device=Xd.device)
    ens._moments(Xd, sup, hcount)
    mean, cov = ens._mean.cpu().numpy(), ens._cov.cpu().numpy()
    off, sq, dims = ens.plan.feat_off, ens._sq_off, ens.plan.dims
    return (hcount, [mean[off[s]:off[s + 1]] for s in range(S)],
            [cov[sq[s]:sq[s + 1]].reshape(dims[s], dims[s]) for s in range(S)])


# ---- moments --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("masked", [False, True])
@pytest.mark.parametrize("n", ROWS)
def test_moments_are_within_the_summation_bound(data, n, masked):
    X = data[n]
    support = None
    if masked:
        support = np.random.default_rng(n).random((len(SIZES), n)) < 0.6
        support[:, 0] = True  # no empty support
    ens, Xd = prepared(MASK, X, workspace_bytes=1 << 30 if n != 65 else 1200)  # 1200: two ranges, one slab and one tile a launch
    _, mus, Cs = device_moments(ens, Xd, support)
    for s in range(len(SIZES)):
        Z = X[:, features(MASK, s)]
        mu, C, h = restate_moments(Z, None if support is None else support[s])
        H = Z.astype(np.float64) if support is None else Z.astype(np.float64)[support[s]]
        assert (np.abs(mus[s] - mu) <= 4 * h * U * np.abs(H).mean(axis=0)).all(), s
        E = np.abs(H - mu)
        bound = 4 * h * U * (E.T @ E / h)
        assert (np.abs(Cs[s] - C) <= bound).all(), (s, float(np.abs(Cs[s] - C).max()))
        np.testing.assert_array_equal(Cs[s], Cs[s].T)
        j = list(features(MASK, s)).index(CONST)
        assert (Cs[s][j] == 0).all() and mus[s][j] == np.float32(101.7)  # a constant column is exact


# ---- factor ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shrinkage", [0.1, "oas"])
@pytest.mark.parametrize("n", ROWS)
def test_factor_inverts_the_shrunk_covariance(data, n, shrinkage):
    X = data[n]
    ens, Xd = prepared(MASK, X, shrinkage=shrinkage)
    hcount, _, Cs = device_moments(ens, Xd, None)
    Cs = [C.copy() for C in Cs]
    ens._factor(hcount)
    cov, W, alpha, status = ens._cov.cpu().numpy(), ens._W.cpu().numpy(), ens._alpha.cpu().numpy(), ens._status.cpu().numpy()
    sq, dims = ens._sq_off, ens.plan.dims
    for s, d in enumerate(dims):
        want_alpha = restate_alpha(Cs[s], n, shrinkage)
        np.testing.assert_allclose(alpha[s], want_alpha, rtol=1e-12)
        Sigma = cov[sq[s]:sq[s + 1]].reshape(d, d)
        want_Sigma = restate_shrunk(Cs[s], alpha[s])
        np.testing.assert_allclose(Sigma, want_Sigma, rtol=4 * U, atol=4 * U * np.abs(want_Sigma).max())
        Ws = W[sq[s]:sq[s + 1]].reshape(d, d)
        if np.trace(Cs[s]) == 0:
            assert status[s] == 1 and (Ws == 0).all()
            continue
        assert status[s] == 0
        assert (np.triu(Ws, 1) == 0).all() and (np.diag(Ws) > 0).all()
        kappa = np.linalg.cond(Sigma)
        resid = np.abs(Ws @ Sigma @ Ws.T - np.eye(d)).max()
        assert resid <= 8 * d * kappa * U, (s, resid, kappa)


# ---- per-subspace scores --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", ROWS)
def test_scores_are_within_one_float32_ulp(data, fitted, n):
    X, ens = data[n], fitted(n)
    per = ens.per_subspace_scores_
    assert per.shape == (len(SIZES), n) and per.dtype == np.float32
    for s in range(len(SIZES)):
        want = restate_fit(X[:, features(MASK, s)])
        assert_well_conditioned(want["est"])
        assert_one_ulp(per[s], want["scores"])
        np.testing.assert_allclose(ens.shrinkage_[s], 0.1, rtol=0, atol=0)
        np.testing.assert_allclose(ens.location_[s], want["est"]["mu"], rtol=1e-13)
        np.testing.assert_allclose(ens.covariance_[s], want["est"]["Sigma"], rtol=1e-10, atol=1e-12 * np.abs(want["est"]["Sigma"]).max())
    assert (per[0] == 0).all()  # the constant subspace
    assert (per >= 0).all()


@pytest.mark.parametrize("S", [1, 2, 33])
def test_scores_for_one_two_and_many_subspaces(S):
    import vgan_amd
    rng = np.random.default_rng(S)
    X = raw_data(65, 24, seed=S)
    mask = np.zeros((S, 24), bool)
    for s in range(S):
        mask[s, rng.choice(24, 1 + (5 * s) % 20, replace=False)] = True  # the first has one (varying) feature
    ens = vgan_amd.SubspaceMahalanobis(mask, np.full(S, 1.0 / S), shrinkage="oas").fit(X)
    for s in range(S):
        want = restate_fit(X[:, features(mask, s)], shrinkage="oas")
        assert_well_conditioned(want["est"])
        assert_one_ulp(ens.per_subspace_scores_[s], want["scores"])
        np.testing.assert_allclose(ens.shrinkage_[s], want["est"]["alpha"], rtol=1e-12)


def test_scores_at_the_widest_subspace():
    """d_s = MAHA_MAX_DIMS with n < d_s; shrinkage 0.5 keeps kappa near 10, which the one-ulp bar needs at this width."""
    import vgan_amd
    from vgan_amd.outlier import MAHA_MAX_DIMS
    X = raw_data(300, MAHA_MAX_DIMS + 6, seed=77, constant=CONST, duplicate=DUP)
    mask = np.ones((2, MAHA_MAX_DIMS + 6), bool)
    mask[0, -6:] = False
    mask[1, 3:] = False  # a narrow one behind it: its matrices start past 2^20 elements
    ens = vgan_amd.SubspaceMahalanobis(mask, [0.5, 0.5], shrinkage=0.5).fit(X)
    for s in range(2):
        want = restate_fit(X[:, features(mask, s)], shrinkage=0.5)
        assert_well_conditioned(want["est"])
        assert_one_ulp(ens.per_subspace_scores_[s], want["scores"])
    np.testing.assert_array_equal(ens.decision_function(X[17:90], return_per_subspace=True)[1], ens.per_subspace_scores_[:, 17:90])


def test_unshrunk_scores_on_full_rank_data():
    """alpha = 0: Gaussian rows mixed by a random matrix; the condition number is the data's own and the test computes it."""
    import vgan_amd
    rng = np.random.default_rng(21)
    X = (100.0 + rng.normal(size=(257, 40)) @ (np.eye(40) + 0.2 * rng.normal(size=(40, 40)) / np.sqrt(40))).astype(np.float32)
    mask = np.zeros((3, 40), bool)
    for s, size in enumerate([3, 16, 33]):
        mask[s, rng.choice(40, size, replace=False)] = True
    ens = vgan_amd.SubspaceMahalanobis(mask, [0.2, 0.3, 0.5], shrinkage=0.0).fit(X)
    for s in range(3):
        want = restate_fit(X[:, features(mask, s)], shrinkage=0.0)
        assert_well_conditioned(want["est"])
        assert_one_ulp(ens.per_subspace_scores_[s], want["scores"])
    assert (ens.shrinkage_ == 0).all()


# ---- select ---------------------------------------------------------------------------------------------------------------
def _device_select(per, h, previous=None):
    import torch
    from vgan_amd.ops import default_ops
    S, n = per.shape
    score = torch.as_tensor(per, device="cuda")
    support = torch.ones(S, n, dtype=torch.uint8, device="cuda") if previous is None else torch.as_tensor(previous.astype(np.uint8), device="cuda")
    changed = torch.full((S,), -1, dtype=torch.int32, device="cuda")
    default_ops().maha_select(score, 0, S, torch.as_tensor(np.asarray(h, dtype=np.int32), device="cuda"), support, changed)
    return support.cpu().numpy().astype(bool), changed.cpu().numpy()


@pytest.mark.parametrize("n", [2, 65, 257, 2051])
def test_select_is_lexsort_on_the_devices_own_scores(fitted, n):
    per = fitted(n).per_subspace_scores_  # row 0 is all zeros: every row ties
    h = [1 + (s * 37) % n for s in range(per.shape[0])]
    h[1], h[2] = n, max(1, n - 1)
    got, changed = _device_select(per, h)
    want = np.stack([select_support(per[s], h[s]) for s in range(per.shape[0])])
    np.testing.assert_array_equal(got, want)
    np.testing.assert_array_equal(changed, (~want).any(axis=1).astype(np.int32))  # against the all-ones start
    again, changed = _device_select(per, h, previous=want)
    np.testing.assert_array_equal(again, want)
    assert (changed == 0).all()


def test_select_breaks_heavy_ties_by_the_lower_row():
    rng = np.random.default_rng(8)
    n = 3 * 256 + 17
    per = rng.integers(0, 5, size=(4, n)).astype(np.float32)  # integer-valued scores
    per[3] = 2.0
    per[2, ::7] = -0.0  # counts as +0.0
    h = [n // 2, 1, 300, 513]
    got, _ = _device_select(per, h)
    want = np.stack([select_support(per[s], h[s]) for s in range(4)])
    np.testing.assert_array_equal(got, want)
    np.testing.assert_array_equal(np.flatnonzero(got[3]), np.arange(513))


# ---- robust, end to end ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", sorted(PLANTED))
def test_concentration_follows_the_restatement_and_separates_the_planted_rows(case):
    import vgan_amd
    cfg = PLANTED[case]
    X, outlier = planted_shift(cfg["n"], cfg["d"], cfg["share"], cfg["seed"])
    want = restate_fit(X, robust=True)
    assert min(want["gaps"]) > MIN_GAP and want["converged"]  # no selection hinges on the last bits of a score
    assert_well_conditioned(want["est"])
    mask = np.ones((1, cfg["d"]), bool)
    model = vgan_amd.VGAN_no_kl(epochs=1)
    model.subspaces, model.proba = mask, np.ones(1)
    ens = model.outlier_ensemble(method="mcd", X=X)
    assert type(ens) is vgan_amd.SubspaceMahalanobis and ens.robust
    np.testing.assert_array_equal(ens.support_[0], want["support"])
    assert ens.support_.dtype == bool and ens.support_[0].sum() == want["h"]
    assert int(ens.n_csteps_[0]) == want["n_csteps"] and bool(ens.converged_[0])
    assert_one_ulp(ens.per_subspace_scores_[0], want["scores"])
    np.testing.assert_allclose(ens.location_[0], want["est"]["mu"], rtol=1e-13)
    classical = model.outlier_ensemble(method="mahalanobis", X=X)
    assert_one_ulp(classical.per_subspace_scores_[0], restate_fit(X)["scores"])
    robust_ratio = separation_ratio(ens.per_subspace_scores_[0], outlier)
    classical_ratio = separation_ratio(classical.per_subspace_scores_[0], outlier)
    print(case, "robust", robust_ratio, "classical", classical_ratio, "steps", ens.n_csteps_)
    assert robust_ratio > 1.0 and classical_ratio < 1.0


def test_max_csteps_bounds_the_concentration(data):
    import vgan_amd
    X, _ = planted_shift(257, 5, 0.10, 3)
    mask = np.ones((1, 5), bool)
    want = restate_fit(X, robust=True, max_csteps=1)
    ens = vgan_amd.SubspaceMahalanobis(mask, [1.0], robust=True, max_csteps=1).fit(X)
    assert int(ens.n_csteps_[0]) == 1 and not ens.converged_[0] and not want["converged"]
    np.testing.assert_array_equal(ens.support_[0], want["support"])
    assert_one_ulp(ens.per_subspace_scores_[0], want["scores"])
    whole = vgan_amd.SubspaceMahalanobis(mask, [1.0], robust=True, support_fraction=1.0).fit(X)
    assert int(whole.n_csteps_[0]) == 0 and whole.converged_[0] and whole.support_.all()


# ---- invariants -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("robust", [False, True])
def test_results_do_not_depend_on_the_workspace_or_the_run(data, robust):
    import vgan_amd
    from vgan_amd.outlier import maha_ranges
    n = ROWS[-1]
    X = data[n]
    kw = dict(robust=robust, max_csteps=2)
    small = 1200  # bytes: 256 cells, so two ranges of subspaces, one slab and one tile a launch
    cells, ranges = maha_ranges(MASK.sum(axis=1), small)
    assert len(ranges) > 1 and cells < 2 * max(SIZES) and -(-n // 1024) == 3
    a = vgan_amd.SubspaceMahalanobis(MASK, PROBA, **kw).fit(X)
    b = vgan_amd.SubspaceMahalanobis(MASK, PROBA, workspace_bytes=small, **kw).fit(X)
    c = vgan_amd.SubspaceMahalanobis(MASK, PROBA, **kw).fit(X)
    for other in (b, c):
        np.testing.assert_array_equal(a.per_subspace_scores_, other.per_subspace_scores_)
        np.testing.assert_array_equal(a.decision_scores_, other.decision_scores_)
        np.testing.assert_array_equal(a.shrinkage_, other.shrinkage_)
        for s in range(len(SIZES)):
            np.testing.assert_array_equal(a.location_[s], other.location_[s])
            np.testing.assert_array_equal(a.covariance_[s], other.covariance_[s])
        if robust:
            np.testing.assert_array_equal(a.support_, other.support_)
            np.testing.assert_array_equal(a.n_csteps_, other.n_csteps_)
            np.testing.assert_array_equal(a.converged_, other.converged_)
    got, per = a.decision_function(X, return_per_subspace=True)
    np.testing.assert_array_equal(per, a.per_subspace_scores_)  # nothing is excluded at fit
    np.testing.assert_array_equal(got, a.decision_scores_)
    part = a.decision_function(X[1000:1100], return_per_subspace=True)[1]  # a row's bits do not depend on its position
    np.testing.assert_array_equal(part, a.per_subspace_scores_[:, 1000:1100])


@pytest.mark.parametrize("normalize", [None, "zscore", "robust", "minmax"])
@pytest.mark.parametrize("combination", ["sum", "max"])
def test_the_shared_tail_serves_the_new_scores(data, normalize, combination):
    import vgan_amd
    X, Y = data[257], data[65]
    mask = MASK[1:]  # without the constant subspace, whose scores are all equal
    proba = PROBA[1:] / PROBA[1:].sum()
    ens = vgan_amd.SubspaceMahalanobis(mask, proba, normalize=normalize, combination=combination, contamination=0.05).fit(X)
    per = ens.per_subspace_scores_
    c, w = (None, None) if normalize is None else _check_stats(ens, normalize)
    if normalize == "zscore":
        c, w = ens.score_center_, ens.score_scale_
    _check_scores(ens.decision_scores_, per, proba, c, w, combination)
    got, per_new = ens.decision_function(Y, return_per_subspace=True)
    _check_scores(got, per_new, proba, c, w, combination)
    assert ens.threshold_ == np.percentile(ens.decision_scores_, 95.0)
    np.testing.assert_array_equal(ens.labels_, (ens.decision_scores_ > ens.threshold_).astype(int))
    np.testing.assert_array_equal(ens.predict(Y), (got > ens.threshold_).astype(int))
    proba_out = ens.predict_proba(Y)
    assert proba_out.shape == (65, 2) and np.allclose(proba_out.sum(axis=1), 1.0) and (proba_out >= 0).all()


# ---- errors ----------------------------------------------------------------------------------------------------------------
def test_a_duplicated_feature_without_shrinkage_raises_and_fits_with_it():
    """Columns 2 and 3 hold 99 and 101 equally often: their covariance is exactly all ones, the second pivot exactly 0."""
    import vgan_amd
    X = raw_data(64, 6, seed=2)
    X[:, 2] = np.where(np.arange(64) % 2 == 0, 99.0, 101.0)
    X[:, 3] = X[:, 2]
    mask = np.zeros((3, 6), bool)
    mask[0, [0, 1, 4]] = mask[1, [2, 3]] = mask[2, [0, 5]] = True
    with pytest.raises(ValueError, match=r"subspace 1\b.*shrinkage > 0"):
        vgan_amd.SubspaceMahalanobis(mask, [0.3, 0.3, 0.4], shrinkage=0.0).fit(X)
    ens = vgan_amd.SubspaceMahalanobis(mask, [0.3, 0.3, 0.4]).fit(X)
    assert_one_ulp(ens.per_subspace_scores_[1], np.full(64, 1.0 / 0.95, dtype=np.float32))
    for s in (0, 2):
        assert_one_ulp(ens.per_subspace_scores_[s], restate_fit(X[:, features(mask, s)])["scores"])
