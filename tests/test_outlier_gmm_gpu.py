"""Gaussian-mixture scores over the subspaces on the MI355X (csrc/outlier_gmm.hip through vgan_amd.SubspaceGMM), against the
float64 restatement of test_outlier_gmm_cpu.py (pinned there to sklearn), never a second run of the code under test.

Bars, with u = 2^-53.  The device adds in another order than numpy, so a fit is compared at what the restatement itself
moves by when its rows are put in another order: spread = max |ln - ln'| between two row orders of the same case, with a
floor of 1e-12 times the largest |lp| term.  Scores: |got - want32| <= 2^-23 |want32| + 16 spread (one float32 ulp of the
reference plus the absolute term).  Parameters: 16 (spread / largest |lp|) relative to the largest entry of the array.
Iteration counts and flags are compared exactly, on cases whose restatement passes the tol guard (no |lb - lb_prev| within 1 %
of tol of tol) under both row orders.  Every fitted case asserts first that d_s kappa u < 2^-30 for the condition number kappa of
every covariance of the restatement: the float64 error of the factor and of the triangular product is of that order relative
to d^2, and under the bar it stays 2^-7 of the float32 rounding of a score (the rule of the Mahalanobis tests without their row
count: there it guards the sums over the rows as well, here the spread does, and it grows with kappa by itself).  It turns
away the draws in which a component collapses onto a few rows and leaves the recipe's own kappa of 10^2 to 10^4.  Moments: the order-independent summation
bound with a factor 4 of slack, |S - want| <= 4 n u (sum_i r_i |z_ia z_ib| / nk), the mean and nk likewise.  E step on
host-made parameters: (16e-12 + 8 d_s kappa u) times the largest |lp| term, the floor above plus the bar of the factor.

Rows below 1023 are fewer than the widest subspaces have features; those cases use reg_covar = 0.05 so that the covariances
stay well conditioned, the others sklearn's 1e-6."""
import numpy as np
import pytest

from test_outlier_gmm_cpu import (LOG_2PI, clustered, planted_case, ranking_fraction, restate_e_step,
                                  restate_fit, restate_m_step, single_gaussian_fraction, tol_guard)
from test_outlier_maha_cpu import raw_data
from test_outlier_norm_gpu import _check_scores, _check_stats

pytestmark = pytest.mark.gpu

U = 2.0 ** -53
D = 70
SIZES = [1, 5, 16, 17, 33, 64, 65, 70]  # the edges of the 4-deep K, the 16-wide tiles, the 32-deep K slabs and the 64 columns of Y
ROWS = [3, 63, 65, 1023, 1025, 2051]  # the smallest, the edges of the 64-row workgroups and of the 1024-row slabs, two slabs + 3
COMPONENTS = {3: (1, 2), 63: (1, 3), 65: (2, 5), 1023: (2, 3), 1025: (3, 5), 2051: (1, 2)}
CASES = [(n, C) for n in ROWS for C in COMPONENTS[n]]
# (n, C) -> seed, 0 unless that draw misses the tol guard or the condition bar (both asserted by the reference fixture)
CASE_SEEDS = {(1023, 2): 3, (1023, 3): 9, (1025, 3): 4, (1025, 5): 1, (2051, 2): 3}
STAGGERED = (1025, 3)  # the case whose subspaces stop at different iterations


def edge_mask():
    rng = np.random.default_rng(0)
    m = np.zeros((len(SIZES), D), bool)
    for s, size in enumerate(SIZES):
        m[s, rng.choice(D, size, replace=False)] = True
    assert list(m.sum(axis=1)) == SIZES
    return m


MASK = edge_mask()
PROBA = np.arange(1, len(SIZES) + 1) / np.arange(1, len(SIZES) + 1).sum()


def features(mask, s):
    return np.flatnonzero(mask[s])


def reg_for(n):
    return 1e-6 if n >= 1023 else 0.05


def case_data(n, C):
    """(X float32 [n, 70] with C planted clusters, labels int [S, n]: per subspace the planted cluster of a row, a fifth of the
    rows relabelled at random).  A start near the planted clusters keeps every component on one cluster, which is what keeps
    its covariance well conditioned; the relabelled rows leave EM several iterations of work."""
    seed = CASE_SEEDS.get((n, C), 0)
    X, cluster, _ = clustered(n, D, C, seed=100 * seed + n + C)
    rng = np.random.default_rng(seed)
    labels = np.stack([np.where(rng.random(n) < 0.2, rng.integers(0, C, size=n), cluster) for _ in SIZES]).astype(np.int64)
    return X, labels


def row_order_spread(Z, labels, C, reg_covar, fit, seed=0, **kw):
    """max |ln - ln'| between the restatement on the rows as given and on a permutation of them, floored at 1e-12 times the
    largest |lp| term; the permuted run must pass the tol guard and take the same iterations."""
    perm = np.random.default_rng(seed).permutation(Z.shape[0])
    other = restate_fit(Z[perm], labels[perm], C, reg_covar=reg_covar, **kw)
    assert other["n_iter"] == fit["n_iter"] and other["converged"] == fit["converged"] and tol_guard(other, kw.get("tol", 1e-3)) >= 0.01
    back = np.empty_like(other["ln"])
    back[perm] = other["ln"]
    return max(float(np.abs(back - fit["ln"]).max()), 1e-12 * fit["lp_max"])


def condition_use(fit):
    """max over the covariances of the start and of the end of d kappa u / 2^-30; the cases need it below 1."""
    return max(S.shape[0] * np.linalg.cond(S) * U / 2.0 ** -30 for par in (fit["start"], fit["par"]) for S in par["Sigma"])


def assert_well_conditioned(fit):
    """The condition on the input under which the bars above hold: d kappa u < 2^-30 for every covariance."""
    assert condition_use(fit) < 1.0, condition_use(fit)


@pytest.fixture(scope="module")
def reference():
    """(n, C) -> (X, labels, [restate_fit per subspace], [spread per subspace]), computed once and shared."""
    cache = {}

    def get(n, C):
        if (n, C) not in cache:
            X, labels = case_data(n, C)
            fits, spreads = [], []
            for s in range(len(SIZES)):
                Z = X[:, features(MASK, s)]
                fit = restate_fit(Z, labels[s], C, reg_covar=reg_for(n))
                assert tol_guard(fit) >= 0.01 and fit["converged"], (n, C, s, tol_guard(fit))
                assert_well_conditioned(fit)
                fits.append(fit)
                spreads.append(row_order_spread(Z, labels[s], C, reg_for(n), fit))
            cache[(n, C)] = (X, labels, fits, spreads)
        return cache[(n, C)]
    return get


def assert_scores(got, fit, spread):
    want32 = fit["scores"]
    assert got.dtype == np.float32 and got.shape == want32.shape
    err = np.abs(got.astype(np.float64) - want32.astype(np.float64))
    assert (err <= 2.0 ** -23 * np.abs(want32.astype(np.float64)) + 16.0 * spread).all(), (float(err.max()), spread)


def assert_parameters(ens, s, fit, spread):
    rel = 16.0 * spread / fit["lp_max"]
    for got, want in ((ens.weights_[s], fit["par"]["w"]), (ens.means_[s], fit["par"]["mu"]), (ens.covariances_[s], fit["par"]["Sigma"])):
        assert got.shape == want.shape and got.dtype == np.float64
        assert np.abs(got - want).max() <= rel * np.abs(want).max(), (s, float(np.abs(got - want).max()), rel)


def prepared(mask, X, C, **kw):
    """(detector, X on the device) with the tables and buffers of fit in place and nothing estimated yet."""
    import vgan_amd
    ens = vgan_amd.SubspaceGMM(mask, np.full(mask.shape[0], 1.0 / mask.shape[0]), n_components=C, init=np.zeros(X.shape[0], dtype=np.int64), **kw)
    Xd = ens._begin_fit(X)
    ens._prepare(X.shape[0], Xd.device)
    return ens, Xd


def load_responsibilities(ens, R, i):
    """R float64 [S, C, n] on the host -> the responsibilities of range i."""
    import torch
    first, count = ens._ranges[i]
    block = torch.as_tensor(np.ascontiguousarray(R[first:first + count]).reshape(-1), device="cuda")
    ens._resp[:block.numel()].copy_(block)


def entries(ens, flat, s, shape):
    """The values of subspace s in a per-entry device array (at feat_off or sq_off), as float64 [C, *shape]."""
    C = ens.n_components
    off = ens._efeat_off if len(shape) == 1 else ens._esq_off
    return flat[off[s * C]:off[(s + 1) * C]].reshape((C,) + shape)


# ---- moments ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [64, 65, 1025, 2051])
def test_one_component_moments_are_the_classical_moments_bit_for_bit(n):
    """C = 1, every responsibility 1 and reg_covar = 0 against vgan_maha_moments with no support on the same data: both run
    the core of csrc/outlier_moments.hpp, and the weighted instantiation then does nothing the plain one does not.  1.0 x is
    x; nk = n + 10 eps rounds to n (half an ulp of an n >= 32 is at least 2^-48 = 16 eps); + 0.0 leaves a diagonal element, a
    sum of squares and never -0.0, as it is.  mean and cov are compared bit for bit."""
    import torch
    import vgan_amd
    sizes = [1, 16, 17, 33, 65]
    rng = np.random.default_rng(n)
    mask = np.zeros((len(sizes), D), bool)
    for s, size in enumerate(sizes):
        mask[s, rng.choice(D, size, replace=False)] = True
    X = raw_data(n, D, seed=n)
    gm, Xd = prepared(mask, X, 1, reg_covar=0.0)
    assert len(gm._ranges) == 1
    gm._resp.fill_(1.0)
    gm._moments(Xd, 0)
    maha = vgan_amd.SubspaceMahalanobis(mask, np.full(len(sizes), 1.0 / len(sizes)))
    maha._begin_fit(X)
    maha._prepare(n, Xd.device)
    maha._moments(Xd, None, torch.full((len(sizes),), n, dtype=torch.int32, device=Xd.device))
    assert (gm._nk.cpu().numpy() == float(n)).all()
    for name in ("_mean", "_cov"):
        got, want = getattr(gm, name).cpu().numpy(), getattr(maha, name).cpu().numpy()
        assert got.shape == want.shape and got.dtype == want.dtype == np.float64
        differs = np.flatnonzero(got.view(np.uint64) != want.view(np.uint64))
        assert differs.size == 0, (name, int(differs[0]), got[differs[0]].hex(), want[differs[0]].hex())


@pytest.mark.parametrize("frozen", [None, 3])
@pytest.mark.parametrize("n", ROWS)
def test_moments_are_within_the_summation_bound(n, frozen):
    C = COMPONENTS[n][1]
    X, _ = case_data(n, C)
    R = np.random.default_rng(n).dirichlet(np.full(C, 0.7), size=(len(SIZES), n)).transpose(0, 2, 1)  # [S, C, n], not one-hot
    ens, Xd = prepared(MASK, X, C, reg_covar=0.25, workspace_bytes=1 << 30 if n != 65 else 8 * C * n * 3)  # 65: ranges of three subspaces
    assert (len(ens._ranges) > 1) == (n == 65)
    for t in (ens._nk, ens._weights, ens._logw, ens._mean, ens._cov):
        t.fill_(-7.0)
    if frozen is not None:
        ens._done[frozen] = 1
    for i in range(len(ens._ranges)):
        load_responsibilities(ens, R, i)
        ens._moments(Xd, i)
    nk, w, logw = (t.cpu().numpy().reshape(len(SIZES), C) for t in (ens._nk, ens._weights, ens._logw))
    mean, cov = ens._mean.cpu().numpy(), ens._cov.cpu().numpy()
    for s, d in enumerate(SIZES):
        mu, Sigma = entries(ens, mean, s, (d,)), entries(ens, cov, s, (d, d))
        if s == frozen:  # a frozen subspace is not touched
            assert (nk[s] == -7.0).all() and (w[s] == -7.0).all() and (logw[s] == -7.0).all() and (mu == -7.0).all() and (Sigma == -7.0).all()
            continue
        Z = X[:, features(MASK, s)].astype(np.float64)
        want = restate_m_step(Z, R[s].T, 0.25)
        assert (np.abs(nk[s] - want["nk"]) <= 4 * n * U * want["nk"]).all()
        assert (np.abs(w[s] - want["w"]) <= 8 * n * U * want["w"]).all()
        assert (np.abs(logw[s] - np.log(want["w"])) <= 8 * n * U + 4 * U * np.abs(np.log(want["w"]))).all()
        for c in range(C):
            r = R[s, c]
            assert (np.abs(mu[c] - want["mu"][c]) <= 4 * n * U * (r @ np.abs(Z)) / want["nk"][c]).all(), (s, c)
            E = np.abs(Z - want["mu"][c])
            bound = 4 * n * U * ((r * E.T) @ E / want["nk"][c]) + 4 * U * 0.25
            assert (np.abs(Sigma[c] - want["Sigma"][c]) <= bound).all(), (s, c, float(np.abs(Sigma[c] - want["Sigma"][c]).max()))
            np.testing.assert_array_equal(Sigma[c], Sigma[c].T)


# ---- E step ----------------------------------------------------------------------------------------------------------------
def device_e_step(ens, Xd, par_of, n):
    """Loads host-made parameters (par_of(s) -> dict of w, mu, Sigma), factors them on the device and runs the E step in
    training mode with the scores beside it, then in scoring mode.  Returns (the parameters, resp [S, C, n], partials [S,
    blocks], scores of the training call, scores of the scoring call)."""
    import torch
    S, C = ens.plan.count, ens.n_components
    pars = [par_of(s) for s in range(S)]
    ens._mean.copy_(torch.as_tensor(np.concatenate([p["mu"].reshape(-1) for p in pars]), device="cuda"))
    ens._cov.copy_(torch.as_tensor(np.concatenate([p["Sigma"].reshape(-1) for p in pars]), device="cuda"))
    ens._logw.copy_(torch.as_tensor(np.concatenate([np.log(p["w"]) for p in pars]), device="cuda"))
    blocks = -(-n // 64)
    resp, partial = np.empty((S, C, n)), np.empty((S, blocks))
    both = torch.full((S, n), float("nan"), dtype=torch.float32, device="cuda")
    alone = torch.full((S, n), float("nan"), dtype=torch.float32, device="cuda")
    for i, (first, count) in enumerate(ens._ranges):
        ens._factor(i)
        args = (Xd, ens._etable, C, first, count, int(ens.plan.dims[first:first + count].max()), ens._mean, ens._W, ens._logdet, ens._logw)
        ens.ops.gmm_estep(*args, resp=ens._resp, lb_partial=ens._lbpart, score=both)
        ens.ops.gmm_estep(*args, score=alone)
        resp[first:first + count] = ens._resp[:count * C * n].cpu().numpy().reshape(count, C, n)
        partial[first:first + count] = ens._lbpart[:count * blocks].cpu().numpy().reshape(count, blocks)
    assert (ens._status.cpu().numpy() == 0).all()
    return pars, resp, partial, both.cpu().numpy(), alone.cpu().numpy()


def check_e_step(X, mask, pars, resp, partial, both, alone):
    n = X.shape[0]
    np.testing.assert_array_equal(both, alone)  # scoring mode rounds the same ln
    for s in range(mask.shape[0]):
        Z = X[:, features(mask, s)].astype(np.float64)
        par = dict(pars[s])
        par["L"] = np.linalg.cholesky(par["Sigma"])
        ln, R, lb, lp = restate_e_step(Z, par)
        d = Z.shape[1]
        kappa = max(np.linalg.cond(S) for S in par["Sigma"])
        atol = (16e-12 + 8 * d * kappa * U) * np.abs(lp).max()
        assert np.abs(resp[s].sum(axis=0) - 1.0).max() <= 1e-14
        assert np.abs(resp[s] - R.T).max() <= 2 * atol, (s, float(np.abs(resp[s] - R.T).max()), atol)
        want32 = (-ln).astype(np.float32)
        err = np.abs(alone[s].astype(np.float64) - want32.astype(np.float64))
        assert (err <= 2.0 ** -23 * np.abs(want32.astype(np.float64)) + atol).all(), (s, float(err.max()), atol)
        padded = np.concatenate([ln, np.zeros(-n % 64)]).reshape(-1, 64)
        assert np.abs(partial[s] - padded.sum(axis=1)).max() <= 64 * atol, s


@pytest.mark.parametrize("n", ROWS)
def test_e_step_matches_numpy_on_host_made_parameters(n):
    import torch
    C = COMPONENTS[n][1]
    X, _ = case_data(n, C)
    R = np.random.default_rng(n + 1).dirichlet(np.full(C, 0.7), size=(len(SIZES), n))  # [S, n, C]
    ens, Xd = prepared(MASK, X, C, workspace_bytes=1 << 30 if n != 1025 else 0)  # 0: one subspace a range
    assert (len(ens._ranges) == len(SIZES)) == (n == 1025)

    def par_of(s):
        return restate_m_step(X[:, features(MASK, s)].astype(np.float64), R[s], 0.5)

    pars, resp, partial, both, alone = device_e_step(ens, Xd, par_of, n)
    check_e_step(X, MASK, pars, resp, partial, both, alone)
    # the stop rule on these partial sums: iteration 1 never stops (lb_prev is -inf) and records the lower bound
    for i in range(len(ens._ranges)):
        first, count = ens._ranges[i]
        ens._lbpart[:count * partial.shape[1]].copy_(torch.as_tensor(partial[first:first + count].reshape(-1), device="cuda"))
        ens._converge(i, 1, n)
    lb = ens._lb.cpu().numpy()
    assert (ens._done.cpu().numpy() == 0).all() and (ens._iters.cpu().numpy() == 1).all()
    np.testing.assert_array_equal(ens._lb_prev.cpu().numpy(), lb)
    for s in range(len(SIZES)):  # each slab of 16 workgroups in order, then the slabs in order
        slabs = [float(np.cumsum(partial[s, j:j + 16])[-1]) for j in range(0, partial.shape[1], 16)]
        assert lb[s] == float(np.cumsum(slabs)[-1]) / n


def test_e_step_at_the_widest_subspace():
    """d_s = MAHA_MAX_DIMS, n = 65, C = 2, Sigma = A A^T / d + I made on the host."""
    from vgan_amd.outlier import MAHA_MAX_DIMS
    d, n, C = MAHA_MAX_DIMS, 65, 2
    rng = np.random.default_rng(1024)
    X = rng.normal(size=(n, d)).astype(np.float32)
    mask = np.ones((1, d), bool)
    A = rng.normal(size=(C, d, d))
    par = dict(w=np.array([0.3, 0.7]), mu=0.1 * rng.normal(size=(C, d)), Sigma=np.einsum("cik,cjk->cij", A, A) / d + np.eye(d))
    ens, Xd = prepared(mask, X, C)
    pars, resp, partial, both, alone = device_e_step(ens, Xd, lambda s: par, n)
    check_e_step(X, mask, pars, resp, partial, both, alone)


# ---- fit -------------------------------------------------------------------------------------------------------------------
def fit_on_device(X, labels, C, n, mask=MASK, proba=PROBA, **kw):
    import vgan_amd
    return vgan_amd.SubspaceGMM(mask, proba, n_components=C, init=labels, reg_covar=reg_for(n), **kw).fit(X)


@pytest.mark.parametrize("n,C", CASES)
def test_fit_follows_the_restatement(reference, n, C):
    X, labels, fits, spreads = reference(n, C)
    if (n, C) == STAGGERED:
        assert len({fit["n_iter"] for fit in fits}) > 1, [fit["n_iter"] for fit in fits]  # the subspaces stop at different iterations
    ens = fit_on_device(X, labels, C, n)
    print((n, C), "n_iter", [fit["n_iter"] for fit in fits], "relative spreads", [sp / fit["lp_max"] for sp, fit in zip(spreads, fits)],
          "tol guards", [round(tol_guard(fit), 3) for fit in fits])
    np.testing.assert_array_equal(ens.n_iter_, [fit["n_iter"] for fit in fits])
    np.testing.assert_array_equal(ens.converged_, [fit["converged"] for fit in fits])
    assert ens.per_subspace_scores_.shape == (len(SIZES), n) and ens.weights_.shape == (len(SIZES), C)
    for s, (fit, spread) in enumerate(zip(fits, spreads)):
        assert_scores(ens.per_subspace_scores_[s], fit, spread)
        assert_parameters(ens, s, fit, spread)
        assert abs(ens.lower_bound_[s] - fit["lower_bound"]) <= 16 * spread
    want = (PROBA[:, None] * ens.per_subspace_scores_.astype(np.float64)).sum(axis=0)
    np.testing.assert_allclose(ens.decision_scores_, want, rtol=1e-12)


def test_max_iter_bounds_the_loop_and_tol_zero_never_fires(reference):
    n, C = 1023, 3
    X, labels, fits, _ = reference(n, C)
    ens = fit_on_device(X, labels, C, n, tol=0.0, max_iter=5)
    assert (ens.n_iter_ == 5).all() and not ens.converged_.any()
    for s in (1, 7):
        Z = X[:, features(MASK, s)]
        want = restate_fit(Z, labels[s], C, reg_covar=reg_for(n), tol=0.0, max_iter=5)
        assert want["n_iter"] == 5 and not want["converged"]
        assert_scores(ens.per_subspace_scores_[s], want, row_order_spread(Z, labels[s], C, reg_for(n), want, tol=0.0, max_iter=5))


# ---- freezing and determinism --------------------------------------------------------------------------------------------------
def published(ens):
    out = [ens.per_subspace_scores_, ens.decision_scores_, ens.weights_, ens.n_iter_, ens.converged_, ens.lower_bound_]
    return out + list(ens.means_) + list(ens.covariances_)


def test_results_do_not_depend_on_company_workspace_polling_or_the_run(reference):
    n, C = STAGGERED
    X, labels, fits, _ = reference(n, C)
    a = fit_on_device(X, labels, C, n)
    assert len(set(a.n_iter_)) > 1  # some subspaces froze while others went on
    variants = [fit_on_device(X, labels, C, n), fit_on_device(X, labels, C, n, workspace_bytes=0)]
    for stride in (1, 7):
        import vgan_amd
        other = vgan_amd.SubspaceGMM(MASK, PROBA, n_components=C, init=labels, reg_covar=reg_for(n))
        other.poll_stride = stride
        variants.append(other.fit(X))
    assert len(variants[1]._ranges) == len(SIZES) and len(a._ranges) == 1
    for other in variants:
        for x, y in zip(published(a), published(other)):
            np.testing.assert_array_equal(x, y)
    first = int(np.argmin(a.n_iter_))  # the subspace that stops first, alone and then in company
    for s in (first, int(np.argmax(a.n_iter_))):
        alone = fit_on_device(X, labels[s:s + 1], C, n, mask=MASK[s:s + 1], proba=[1.0])
        np.testing.assert_array_equal(alone.per_subspace_scores_[0], a.per_subspace_scores_[s])
        np.testing.assert_array_equal(alone.means_[0], a.means_[s])
        np.testing.assert_array_equal(alone.covariances_[0], a.covariances_[s])
        np.testing.assert_array_equal(alone.weights_[0], a.weights_[s])
        assert alone.n_iter_[0] == a.n_iter_[s] and alone.lower_bound_[0] == a.lower_bound_[s]
    got, per = a.decision_function(X, return_per_subspace=True)
    np.testing.assert_array_equal(per, a.per_subspace_scores_)  # nothing is left out at fit
    np.testing.assert_array_equal(got, a.decision_scores_)
    part = a.decision_function(X[17:90], return_per_subspace=True)[1]  # a row's bits do not depend on its position
    np.testing.assert_array_equal(part, a.per_subspace_scores_[:, 17:90])


# ---- what the detector is for --------------------------------------------------------------------------------------------------
def test_the_mixture_ranks_the_planted_rows_on_the_device():
    import vgan_amd
    X, labels, mark, C = planted_case("300x5")
    model = vgan_amd.VGAN_no_kl(epochs=1)
    model.subspaces, model.proba = np.ones((1, X.shape[1]), bool), np.ones(1)
    ens = model.outlier_ensemble(method="gmm", n_components=C, init=labels, X=X)
    assert type(ens) is vgan_amd.SubspaceGMM
    want = restate_fit(X, labels, C)
    assert tol_guard(want) >= 0.01 and int(ens.n_iter_[0]) == want["n_iter"] and bool(ens.converged_[0])
    mixture, single = ranking_fraction(ens.per_subspace_scores_[0], mark), single_gaussian_fraction(X, mark)
    print("planted 300x5: mixture", mixture, "one Gaussian", single)
    assert mixture >= 0.99 and single <= 0.05


def test_one_component_is_the_mahalanobis_detector():
    """C = 1, reg_covar = 0 against SubspaceMahalanobis(shrinkage=0) on full-rank data: the covariance is the same to the bit
    (the responsibilities after an E step are exp(0) / 1 = 1.0, and the moments are one code path), and 2 score - d_s log 2pi - 2
    sum log diag L is its d^2.  Both published numbers are float32: the score carries half an ulp of its own size, doubled by the factor 2, d^2
    half an ulp of its own, so the bar is 2 float32 ulps of the larger of |score| and d^2."""
    import vgan_amd
    rng = np.random.default_rng(21)
    X = (100.0 + rng.normal(size=(257, 40)) @ (np.eye(40) + 0.2 * rng.normal(size=(40, 40)) / np.sqrt(40))).astype(np.float32)
    mask = np.zeros((3, 40), bool)
    for s, size in enumerate([3, 16, 33]):
        mask[s, rng.choice(40, size, replace=False)] = True
    maha = vgan_amd.SubspaceMahalanobis(mask, [0.2, 0.3, 0.5], shrinkage=0.0).fit(X)
    gm = vgan_amd.SubspaceGMM(mask, [0.2, 0.3, 0.5], n_components=1, reg_covar=0.0).fit(X)  # init "kmeans" with C = 1: all labels 0
    assert (gm.n_iter_ == 2).all() and gm.converged_.all() and (gm.weights_ == 1.0).all()
    for s in range(3):
        d = int(mask[s].sum())
        np.testing.assert_array_equal(gm.covariances_[s][0], maha.covariance_[s])  # one code path: the same bits
        logdet = np.log(np.diag(np.linalg.cholesky(gm.covariances_[s][0]))).sum()
        score = gm.per_subspace_scores_[s].astype(np.float64)
        d2 = maha.per_subspace_scores_[s].astype(np.float64)
        err = np.abs(2.0 * score - d * LOG_2PI - 2.0 * logdet - d2)
        assert (err <= 2.0 * 2.0 ** -23 * np.maximum(np.abs(score), d2)).all(), (s, float(err.max()))


def test_init_kmeans_takes_the_labels_of_the_cblof_kmeans():
    import vgan_amd
    n, C = 1023, 3
    X, _ = case_data(n, C)
    mask, proba = MASK[1:6], PROBA[1:6] / PROBA[1:6].sum()
    km = vgan_amd.SubspaceCBLOF(mask, proba, n_clusters=C, init="random", seed=3, max_iter=30).fit(X)
    auto = vgan_amd.SubspaceGMM(mask, proba, n_components=C, seed=3).fit(X)
    np.testing.assert_array_equal(auto.kmeans_labels_, km.cluster_labels_)
    given = vgan_amd.SubspaceGMM(mask, proba, n_components=C, init=km.cluster_labels_).fit(X)
    for x, y in zip(published(auto), published(given)):
        np.testing.assert_array_equal(x, y)


def test_a_duplicated_feature_without_reg_covar_raises_and_fits_with_it():
    """Columns 2 and 3 hold 99 and 101 equally often in both components (32 rows each, so nk = 32 + 10 eps rounds to 32): their
    covariance is exactly all ones, the second pivot exactly 0."""
    import vgan_amd
    X = raw_data(64, 6, seed=2)
    X[:, 2] = np.where(np.arange(64) % 2 == 0, 99.0, 101.0)
    X[:, 3] = X[:, 2]
    labels = (np.arange(64) // 2) % 2
    mask = np.zeros((3, 6), bool)
    mask[0, [0, 1, 4]] = mask[1, [2, 3]] = mask[2, [0, 5]] = True
    bad = vgan_amd.SubspaceGMM(mask, [0.3, 0.3, 0.4], n_components=2, init=labels, reg_covar=0.0)
    with pytest.raises(ValueError, match=r"subspace 1, component 0\b.*reg_covar > 0"):
        bad.fit(X)
    assert bad.converged_[0] and bad.converged_[2] and not bad.converged_[1]  # the others were not held up
    for s in (0, 2):
        want = restate_fit(X[:, features(mask, s)], labels, 2, reg_covar=0.0)
        assert tol_guard(want) >= 0.01 and int(bad.n_iter_[s]) == want["n_iter"]
    ens = vgan_amd.SubspaceGMM(mask, [0.3, 0.3, 0.4], n_components=2, init=labels, reg_covar=1e-6).fit(X)
    assert ens.converged_.all() and np.isfinite(ens.per_subspace_scores_).all()
    for s in (0, 2):
        want = restate_fit(X[:, features(mask, s)], labels, 2, reg_covar=1e-6)
        assert_scores(ens.per_subspace_scores_[s], want, 1e-12 * want["lp_max"])


@pytest.mark.parametrize("normalize", [None, "zscore", "robust", "minmax"])
@pytest.mark.parametrize("combination", ["sum", "max"])
def test_the_shared_tail_serves_the_new_scores(reference, normalize, combination):
    X, labels, _, _ = reference(1023, 2)
    Y = case_data(65, 2)[0]
    ens = fit_on_device(X, labels, 2, 1023, normalize=normalize, combination=combination, contamination=0.05)
    per = ens.per_subspace_scores_
    c, w = (None, None) if normalize is None else _check_stats(ens, normalize)
    if normalize == "zscore":
        c, w = ens.score_center_, ens.score_scale_
    _check_scores(ens.decision_scores_, per, PROBA, c, w, combination)
    got, per_new = ens.decision_function(Y, return_per_subspace=True)
    _check_scores(got, per_new, PROBA, c, w, combination)
    assert ens.threshold_ == np.percentile(ens.decision_scores_, 95.0)
    np.testing.assert_array_equal(ens.labels_, (ens.decision_scores_ > ens.threshold_).astype(int))
    np.testing.assert_array_equal(ens.predict(Y), (got > ens.threshold_).astype(int))
    proba_out = ens.predict_proba(Y)
    assert proba_out.shape == (65, 2) and np.allclose(proba_out.sum(axis=1), 1.0) and (proba_out >= 0).all()
