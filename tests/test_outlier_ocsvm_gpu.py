"""One-class SVM scores over the subspaces on the MI355X (csrc/outlier_ocsvm.hip through vgan_amd.SubspaceOCSVM and the ops
wrappers), against the numpy restatement of test_outlier_ocsvm_cpu.py (pinned there to sklearn), never a second run of the
code under test.

Rounding the kernel matrix to float32 moves the pairs the solver picks, so every exact comparison runs the restatement on
the very float32 K the device used: with identical input and the fixed arithmetic of the contract every decision is
identical, and alpha, G and the iteration count are compared bit for bit.  K itself is held to float64 separately.

Bars, with eps32 = 2^-24.  An entry of K: K64 (gamma d2_err + (gamma d2 + 4) 2^-23) + 2^-126, d2_err the engine's bound on its
squared distance (exact: (round4(d_s) + 2) eps32 d2; Gram: 64 eps32 sqrt(d_s) (|q - c|^2 + max |r - c|^2): outlier_checks.d2_tolerance),
the trailing terms the rounding of the argument and of expf and float32's smallest normal number.  rho: n 2^-53 max |G|.  A
score: sum_r a_r Kbar(q, r) + n 2^-45 + 2^-23 |want|, Kbar the bar of that entry, then the fixed-point grid and the float32 result."""
import numpy as np
import pytest

from outlier_checks import d2_tolerance
from test_outlier_gmm_gpu import D, MASK, PROBA, SIZES
from test_outlier_norm_gpu import _check_scores, _check_stats
from test_outlier_ocsvm_cpu import (host_kernel_matrix, planted_data, ranking_rate, restate_gamma, restate_scores, restate_smo,
                                    restate_sq_dists, shifted_data)

pytestmark = pytest.mark.gpu

ROWS = [2, 3, 63, 65, 255, 257, 1025]  # the smallest, the 64-row tile edges, the 256-thread workgroup edges, several strided passes
CASES = [(n, 0.5) for n in ROWS] + [(n, 0.1) for n in ROWS if n >= 63] + [(65, 0.01)]  # nu n < 1 at n = 65
NEW_ROWS = 130
GRAM_MIN_DIMS = 32
STAGGERED = (257, 0.1)  # the d_s = 1 subspace takes about five times the steps of the others


def features(s):
    return np.flatnonzero(MASK[s])


_DATA, _D2, _HOST = {}, {}, {}


def case_data(n):
    """(X float32 [n, 70], Y float32 [130, 70]): raw rows, columns scaled by factors in [0.5, 2] and offset, a twentieth shifted."""
    if n not in _DATA:
        rows = shifted_data(n + NEW_ROWS, D, seed=n, scale=True)
        _DATA[n] = (np.ascontiguousarray(rows[:n]), np.ascontiguousarray(rows[n:]))
    return _DATA[n]


def sq_dists(n, s):
    """(d2 of the fitted rows among themselves, d2 of the new rows against them), float64, made once."""
    if (n, s) not in _D2:
        X, Y = case_data(n)
        _D2[n, s] = (restate_sq_dists(X[:, features(s)], X[:, features(s)]), restate_sq_dists(Y[:, features(s)], X[:, features(s)]))
    return _D2[n, s]


def gamma_of(n, s):
    return restate_gamma(case_data(n)[0][:, features(s)].astype(np.float64), "scale")


def host_matrices(n):
    """float32 [S, n, n]: a kernel matrix per subspace made on the host."""
    if n not in _HOST:
        K = np.exp(-np.stack([gamma_of(n, s) * sq_dists(n, s)[0] for s in range(len(SIZES))])).astype(np.float32)
        K[:, np.arange(n), np.arange(n)] = 1.0
        _HOST[n] = K
    return _HOST[n]


def kernel_bar(engine, Xq, Xr, s, d2, gamma):
    """(K64, the bar of every entry) for the query rows Xq against the fitted rows Xr in subspace s."""
    K64 = np.exp(-gamma * d2)
    d2_err = d2_tolerance(engine, Xq, Xr, features(s), d2)
    return K64, K64 * (gamma * d2_err + (gamma * d2 + 4.0) * 2.0 ** -23) + 2.0 ** -126


def engine_of(s):
    return "gram" if SIZES[s] >= GRAM_MIN_DIMS else "exact"


class Solver:
    """init / smo / rho through the ops wrappers on uploaded matrices."""

    def __init__(self, K, nu, tol=1e-3, max_iter=None, stride=128, storage="auto"):
        import torch
        from vgan_amd import outlier
        from vgan_amd.ops import default_ops
        self.ops, self.torch = default_ops(), torch
        S, n = K.shape[0], K.shape[1]
        self.K = torch.as_tensor(K).cuda()
        self.alpha = torch.empty(S, n, dtype=torch.float64, device="cuda")
        self.G = torch.empty(S, n, dtype=torch.float64, device="cuda")
        self.done = torch.full((S,), -1, dtype=torch.int32, device="cuda")
        self.iters = torch.full((S,), -1, dtype=torch.int32, device="cuda")
        self.tol, self.max_iter, self.stride = tol, 100 * n if max_iter is None else max_iter, stride
        self.storage = outlier.OCSVM_STORAGE[storage]
        self.ops.ocsvm_init(self.K, *outlier.ocsvm_start(nu, n), self.alpha, self.G, self.done, self.iters)
        self.launched = 0

    def launch(self):
        steps = min(self.stride, self.max_iter - self.launched)
        self.ops.ocsvm_smo(self.K, self.tol, self.max_iter, steps, self.alpha, self.G, self.done, self.iters, self.storage)
        self.launched += steps

    def state(self):
        return self.alpha.cpu().numpy(), self.G.cpu().numpy(), self.done.cpu().numpy(), self.iters.cpu().numpy()

    def run(self):
        while self.launched < self.max_iter and not bool((self.done != 0).all()):
            self.launch()
        rho = self.torch.empty(self.K.shape[0], dtype=self.torch.float64, device="cuda")
        self.ops.ocsvm_rho(self.alpha, self.G, rho)
        return (*self.state(), rho.cpu().numpy())


_WANT = {}


def host_fit(n, nu, s, **kw):
    key = (n, nu, s, tuple(sorted(kw.items())))
    if key not in _WANT:
        _WANT[key] = restate_smo(host_matrices(n)[s], nu, **kw)
    return _WANT[key]


def check_state(got, want, n):
    alpha, G, done, iters, rho = got
    np.testing.assert_array_equal(alpha, want.a)
    np.testing.assert_array_equal(G, want.G)
    assert iters == want.n_iter and done == (1 if want.converged else 2)
    assert abs(rho - want.rho) <= n * 2.0 ** -53 * np.abs(want.G).max(), (rho, want.rho)


# ---- the solver on a host-made matrix ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,nu", CASES)
def test_solver_is_the_restatement_bit_for_bit(n, nu):
    got = Solver(host_matrices(n), nu).run()
    assert (got[2] == 1).all()
    for s in range(len(SIZES)):
        check_state([v[s] for v in got], host_fit(n, nu, s), n)


def test_solver_bits_do_not_depend_on_the_launch_stride_or_on_where_a_and_g_live():
    n, nu = STAGGERED
    K = host_matrices(n)
    base = Solver(K, nu).run()
    for stride, storage in ((1, "auto"), (7, "auto"), (7, "global"), (128, "global"), (128, "lds"), (7, "wide"), (128, "wide")):
        other = Solver(K, nu, stride=stride, storage=storage).run()
        for a, b in zip(base, other):
            np.testing.assert_array_equal(a, b)
    # the edge of "auto": 2048 rows fit LDS (and in place: the same bits), 2049 rows run in place with 1024 threads (and with
    # 256: the same bits)
    Z = shifted_data(2049, 5, seed=5).astype(np.float64)
    big = host_kernel_matrix(Z, restate_gamma(Z, "scale"))
    edge = np.ascontiguousarray(big[None, :2048, :2048])
    in_lds, in_place = Solver(edge, 0.1).run(), Solver(edge, 0.1, storage="global").run()
    for a, b in zip(in_lds, in_place):
        np.testing.assert_array_equal(a, b)
    check_state([v[0] for v in in_lds], restate_smo(edge[0], 0.1), 2048)
    wide, narrow = Solver(big[None], 0.1).run(), Solver(big[None], 0.1, storage="global").run()
    for a, b in zip(wide, narrow):
        np.testing.assert_array_equal(a, b)
    check_state([v[0] for v in wide], restate_smo(big, 0.1), 2049)


def test_a_stopped_subspace_is_left_alone_while_the_others_go_on():
    n, nu = STAGGERED
    want = [host_fit(n, nu, s) for s in range(len(SIZES))]
    steps = [w.n_iter for w in want]
    assert steps[0] >= 3 * max(steps[1:])  # d_s = 1 takes several times more
    solver = Solver(host_matrices(n), nu, stride=32)
    frozen = {}
    for _ in range(steps[0] // 32 + 1):
        solver.launch()
        alpha, G, done, iters = solver.state()
        for s in range(len(SIZES)):
            if s in frozen:
                np.testing.assert_array_equal(alpha[s], frozen[s][0])
                np.testing.assert_array_equal(G[s], frozen[s][1])
                assert iters[s] == frozen[s][2]
            elif done[s] != 0:  # the launch that looks at the stop rule after steps[s] updates
                assert solver.launched - 32 <= steps[s] < solver.launched and iters[s] == steps[s]
                frozen[s] = (alpha[s].copy(), G[s].copy(), iters[s])
            else:
                assert iters[s] == solver.launched  # every launch ran its 32 steps
    assert len(frozen) == len(SIZES)
    assert solver.launched > 3 * max(steps[1:])  # the others were done long before
    for s in range(len(SIZES)):
        np.testing.assert_array_equal(frozen[s][0], want[s].a)
        np.testing.assert_array_equal(frozen[s][1], want[s].G)
        assert frozen[s][2] == steps[s]


def test_max_iter_cuts_the_loop_off():
    n, nu = STAGGERED
    got = Solver(host_matrices(n), nu, max_iter=10, stride=4).run()
    for s in range(len(SIZES)):
        want = host_fit(n, nu, s, max_iter=10)
        assert want.n_iter == 10 and not want.converged
        check_state([v[s] for v in got], want, n)


# ---- the kernel matrix ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("engine", ["exact", "gram"])
@pytest.mark.parametrize("n", [2, 65, 257])
def test_kernel_matrix_against_float64(n, engine):
    import vgan_amd
    X, _ = case_data(n)
    ens = vgan_amd.SubspaceOCSVM(MASK, PROBA, engine=engine, max_iter=1)
    ens.keep_kernel_matrix = True
    ens.fit(X)
    for s in range(len(SIZES)):
        K = ens.kernel_matrix_[s]
        assert K.dtype == np.float32 and K.shape == (n, n)
        gamma = gamma_of(n, s)
        assert ens.gamma_[s] == pytest.approx(gamma, rel=1e-12)
        assert (np.diagonal(K) == 1.0).all()
        K64, bar = kernel_bar(engine, X, X, s, sq_dists(n, s)[0], gamma)
        err = np.abs(K.astype(np.float64) - K64)
        np.fill_diagonal(err, 0.0)  # the Gram engine's own d2 of a row with itself need not be 0: the diagonal is set
        assert (err <= bar).all(), (s, float((err / bar).max()))


# ---- end to end -------------------------------------------------------------------------------------------------------------
def check_scores(got, a, rho, engine, Xq, Xr, s, d2, gamma):
    K64, kbar = kernel_bar(engine, Xq, Xr, s, d2, gamma)
    want = restate_scores(a, rho, K64)
    bar = (kbar * a[None, :]).sum(axis=1) + len(a) * 2.0 ** -45 + 2.0 ** -23 * np.abs(want)
    err = np.abs(np.asarray(got, np.float64) - want)
    assert (err <= bar).all(), (s, float((err / bar).max()))


@pytest.mark.parametrize("n,nu", CASES)
def test_fit_end_to_end(n, nu):
    import vgan_amd
    X, Y = case_data(n)
    ens = vgan_amd.SubspaceOCSVM(MASK, PROBA, nu=nu)
    ens.keep_kernel_matrix = True
    ens.fit(X)
    assert ens.dual_coef_.dtype == np.float64 and ens.dual_coef_.shape == (len(SIZES), n)
    assert ens.intercept_.dtype == np.float64 and ens.gamma_.dtype == np.float64 and ens.converged_.all()
    per_new = ens.decision_function(Y, return_per_subspace=True)[1]
    again, per_again = ens.decision_function(X, return_per_subspace=True)
    np.testing.assert_array_equal(again, ens.decision_scores_)
    np.testing.assert_array_equal(per_again, ens.per_subspace_scores_)
    for s in range(len(SIZES)):
        want = restate_smo(ens.kernel_matrix_[s], nu)
        np.testing.assert_array_equal(ens.dual_coef_[s], want.a)
        assert ens.n_iter_[s] == want.n_iter and want.converged
        np.testing.assert_array_equal(ens.support_[s], np.flatnonzero(want.a > 0))
        assert ens.n_support_[s] == (want.a > 0).sum()
        assert abs(-ens.intercept_[s] - want.rho) <= n * 2.0 ** -53 * np.abs(want.G).max()
        gamma = gamma_of(n, s)
        assert ens.gamma_[s] == pytest.approx(gamma, rel=1e-12)
        d2_fit, d2_new = sq_dists(n, s)
        check_scores(ens.per_subspace_scores_[s], want.a, -ens.intercept_[s], engine_of(s), X, X, s, d2_fit, gamma)
        check_scores(per_new[s], want.a, -ens.intercept_[s], engine_of(s), Y, X, s, d2_new, gamma)
    np.testing.assert_allclose(ens.decision_scores_, PROBA @ ens.per_subspace_scores_.astype(np.float64), rtol=1e-12)


def test_scores_are_the_same_bits_for_every_split_chunking_and_company():
    import vgan_amd
    n, nu = 257, 0.5
    X, Y = case_data(n)

    def run(mask=MASK, proba=PROBA, **kw):
        ens = vgan_amd.SubspaceOCSVM(mask, proba, nu=nu, **kw).fit(X)
        return ens, (ens.decision_scores_, ens.per_subspace_scores_, ens.dual_coef_, ens.n_iter_, ens.intercept_,
                     *ens.decision_function(Y, return_per_subspace=True))

    base_ens, base = run()
    assert len(base_ens.plan.chunks(n, base_ens.workspace_bytes)) == 2
    tiny = dict(workspace_bytes=1)  # one subspace per chunk
    from vgan_amd.outlier import ocsvm_chunks
    assert len(ocsvm_chunks(base_ens.plan, n, 1)) == len(SIZES)
    for kw in ({}, dict(splits=1), dict(splits=3), tiny, dict(splits=3, **tiny)):
        for a, b in zip(base, run(**kw)[1]):
            np.testing.assert_array_equal(a, b)
    for s in (0, 5):  # one subspace of either engine, fitted alone
        alone = run(mask=MASK[s:s + 1], proba=[1.0])[1]
        np.testing.assert_array_equal(alone[1][0], base[1][s])
        np.testing.assert_array_equal(alone[2][0], base[2][s])
        np.testing.assert_array_equal(alone[6][0], base[6][s])
        assert alone[3][0] == base[3][s] and alone[4][0] == base[4][s]


def test_a_constant_subspace_scores_exactly_zero():
    import vgan_amd
    n = 65
    X = case_data(n)[0].copy()
    X[:, :40] = np.float32(2.7)
    mask = np.zeros((3, D), bool)
    mask[0, :3] = mask[1, :40] = mask[2, 38:45] = True  # constant on either engine, and a mixed one
    for nu in (0.5, 0.1, 0.37):
        ens = vgan_amd.SubspaceOCSVM(mask, [0.2, 0.3, 0.5], nu=nu).fit(X)
        assert list(ens.n_iter_[:2]) == [0, 0] and ens.n_iter_[2] > 0 and ens.converged_.all()
        np.testing.assert_array_equal(ens.gamma_[:2], [1.0 / 3, 1.0 / 40])
        np.testing.assert_array_equal(ens.intercept_[:2], [-nu * n, -nu * n])
        np.testing.assert_array_equal(ens.per_subspace_scores_[:2], np.zeros((2, n), np.float32))
        np.testing.assert_array_equal(ens.decision_function(X[:7], return_per_subspace=True)[1][:2], np.zeros((2, 7), np.float32))


def test_nu_one_and_two_rows():
    import vgan_amd
    X, Y = case_data(63)
    ens = vgan_amd.SubspaceOCSVM(MASK, PROBA, nu=1.0)
    ens.keep_kernel_matrix = True
    ens.fit(X)
    assert (ens.n_iter_ == 0).all() and ens.converged_.all() and (ens.dual_coef_ == 1.0).all()
    for s in range(len(SIZES)):
        want = restate_smo(ens.kernel_matrix_[s], 1.0)
        assert -ens.intercept_[s] == want.rho == want.G.max()  # this class's rule: the one bound there is
    X2 = X[:2]
    two = vgan_amd.SubspaceOCSVM(MASK, PROBA, nu=1.0).fit(X2)
    assert (two.n_iter_ == 0).all() and two.decision_scores_.shape == (2,) and np.isfinite(two.decision_scores_).all()


# ---- optimality, independent of the path ------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,nu", [(65, 0.5), (257, 0.1), (1025, 0.5)])
def test_published_dual_is_optimal_within_tol(n, nu):
    import vgan_amd
    X, _ = case_data(n)
    ens = vgan_amd.SubspaceOCSVM(MASK, PROBA, nu=nu)
    ens.keep_kernel_matrix = True
    ens.fit(X)
    for s in range(len(SIZES)):
        a = ens.dual_coef_[s]
        assert a.min() >= 0.0 and a.max() <= 1.0 and abs(a.sum() - nu * n) <= n * 2.0 ** -52 * nu * n
        G64 = np.exp(-gamma_of(n, s) * sq_dists(n, s)[0]) @ a
        G_dev = ens.kernel_matrix_[s].astype(np.float64) @ a
        violation = (-G64[a < 1.0]).max() + G64[a > 0.0].max()
        assert violation < ens.tol + 2 * np.abs(G_dev - G64).max(), (s, violation)


# ---- the shared tail --------------------------------------------------------------------------------------------------------
def test_normalize_max_and_predict_go_through_the_shared_tail():
    import vgan_amd
    X, Y = case_data(257)
    ens = vgan_amd.SubspaceOCSVM(MASK, PROBA, nu=0.1, normalize="robust", combination="max", contamination=0.05).fit(X)
    per = ens.per_subspace_scores_
    c, w = _check_stats(ens, "robust")
    _check_scores(ens.decision_scores_, per, PROBA, c, w, "max")
    got, per_new = ens.decision_function(Y, return_per_subspace=True)
    _check_scores(got, per_new, PROBA, c, w, "max")
    assert ens.threshold_ == np.percentile(ens.decision_scores_, 95.0)
    np.testing.assert_array_equal(ens.labels_, (ens.decision_scores_ > ens.threshold_).astype(int))
    np.testing.assert_array_equal(ens.predict(Y), (got > ens.threshold_).astype(int))
    assert ens.predict_proba(Y).shape == (NEW_ROWS, 2)


def test_vgan_outlier_ensemble_ocsvm_end_to_end():
    import vgan_amd
    from test_outlier_gpu import _planted
    X = _planted()[:, :10]
    model = vgan_amd.VGAN_no_kl(epochs=5)
    model.fit(X)
    X = np.ascontiguousarray(X[-600:])
    ens = model.outlier_ensemble(method="ocsvm", nu=0.1, subspace_count=200, X=X)
    assert type(ens) is vgan_amd.SubspaceOCSVM and ens._fitted
    assert ens.decision_scores_.shape == (600,) and np.isfinite(ens.decision_scores_).all()
    assert ens.dual_coef_.shape == (model.subspaces.shape[0], 600) and ens.converged_.all()
    np.testing.assert_array_equal(ens.decision_function(X), ens.decision_scores_)


# ---- planted outliers -------------------------------------------------------------------------------------------------------
def test_planted_outliers_rank_on_top_at_the_restatements_rate():
    """The device's rate is compared with the restatement's on the device's own K, never with a fixed number; a row whose
    reference score lies within twice the score bar of the cut may fall on either side of it."""
    import vgan_amd
    n, nu = 1025, 0.1
    X, rows = planted_data(n, D, seed=3)
    ens = vgan_amd.SubspaceOCSVM(MASK, PROBA, nu=nu)
    ens.keep_kernel_matrix = True
    ens.fit(X)
    k = len(rows)
    rates = []
    for s in (0, 2, 5, 7):  # 1, 16, 64 and 70 features: both engines
        d2 = restate_sq_dists(X[:, features(s)], X[:, features(s)])
        gamma = restate_gamma(X[:, features(s)].astype(np.float64), "scale")
        want = restate_smo(ens.kernel_matrix_[s], nu)
        K64, kbar = kernel_bar(engine_of(s), X, X, s, d2, gamma)
        ref = restate_scores(want.a, want.rho, K64)
        bar = (kbar * want.a[None, :]).sum(axis=1) + n * 2.0 ** -45 + 2.0 ** -23 * np.abs(ref)
        cut = np.sort(ref)[-k]
        near = int((np.abs(ref - cut) <= 2 * bar).sum()) - 1  # rows other than the k-th itself that may cross the cut
        got, base = ranking_rate(ens.per_subspace_scores_[s], rows), ranking_rate(ref, rows)
        assert abs(got - base) <= near / k, (s, got, base, near)
        rates.append(base)
    assert max(rates) > 0.9  # the wide subspaces find them
