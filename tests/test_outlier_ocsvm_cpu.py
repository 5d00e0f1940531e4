"""One-class SVM scores over the subspaces, CPU tier: the numpy restatement the GPU tests compare against, pinned to sklearn's
OneClassSVM(kernel="rbf", shrinking=False); the edge cases of the contract; and everything of vgan_amd.SubspaceOCSVM that
runs without a device (argument checks, the host rules, the dispatch from the model, the C ABI's argument checks).

The definition is SubspaceOCSVM's docstring, and restate_smo follows it line for line: the float32 kernel matrix widened to
float64, libsvm's start, WSS2 with the lowest index on a tie, every operation a numpy operation of its own (numpy
contracts nothing into an FMA), rho with this class's rule where libsvm's is infinite.  Given the same float32 K the
device takes the same decisions, so the GPU tests compare alpha, G and the iteration count exactly."""
import ctypes
import math
import os
import re
from collections import namedtuple

import numpy as np
import pytest

from conftest import REPO
from test_outlier_ecod_cpu import _mask

PIN_CASES = [(65, 5, 0.5), (257, 17, 0.1), (257, 70, 0.5), (1025, 33, 0.1), (1025, 70, 0.5)]  # (n, d_s, nu)
# measured by test_scores_are_sklearns_at_a_tight_tolerance (its docstring): the largest |restatement - sklearn| over
# PIN_CASES at tol 1e-9, relative to the largest |score| of the case
PIN_MEASURED = 1.2e-10
PIN_BAR = 8 * PIN_MEASURED

Fit = namedtuple("Fit", "a G rho path n_iter converged")


# ---- the restatement --------------------------------------------------------------------------------------------------------
def restate_gamma(Z, gamma):
    """gamma_s of the block Z [n, d_s] (float64): "scale" 1 / (d_s var), var over all entries, 1.0 where it is 0; "auto" 1 / d_s."""
    Z = np.asarray(Z, np.float64)
    if gamma == "scale":
        var = Z.var()
        return 1.0 / (Z.shape[1] * (var if var != 0.0 else 1.0))
    if gamma == "auto":
        return 1.0 / Z.shape[1]
    return float(gamma)


def restate_sq_dists(Zq, Zr):
    """float64 [nq, nr]: sum_f (q_f - r_f)^2 from the differences."""
    Zq, Zr = np.asarray(Zq, np.float64), np.asarray(Zr, np.float64)
    out = np.empty((Zq.shape[0], Zr.shape[0]))
    for lo in range(0, Zq.shape[0], 128):
        diff = Zq[lo:lo + 128, None, :] - Zr[None, :, :]
        out[lo:lo + 128] = (diff * diff).sum(axis=2)
    return out


def restate_kernel(Zq, Zr, gamma):
    """float64 [nq, nr]: exp(-gamma d^2)."""
    return np.exp(-gamma * restate_sq_dists(Zq, Zr))


def host_kernel_matrix(Z, gamma):
    """float32 [n, n]: the float64 kernel rounded, the diagonal exactly 1: a matrix as ``fit`` hands one to the solver."""
    K = restate_kernel(Z, Z, gamma).astype(np.float32)
    np.fill_diagonal(K, 1.0)
    return K


def restate_start(nu, n):
    m = int(nu * n)
    a = np.zeros(n)
    a[:m] = 1.0
    if m < n:
        a[m] = nu * n - m
    return a


def restate_rho(a, G):
    """The mean of G over the free rows (exact sum, one division); without one the midpoint of the two bounds, and with one
    bound missing as well the other one."""
    free = (a > 0.0) & (a < 1.0)
    if free.any():
        return math.fsum(G[free]) / int(free.sum())
    upper, lower = G[a >= 1.0], G[a <= 0.0]
    if upper.size and lower.size:
        return (lower.min() + upper.max()) / 2.0
    return upper.max() if upper.size else lower.min()


def restate_smo(K, nu, tol=1e-3, max_iter=None):
    """Fit(a, G, rho, path, n_iter, converged) of the SMO loop on the float32 matrix K (row r: K[r, t]); path is the list of
    pairs (i, j)."""
    K = np.asarray(K)
    assert K.dtype == np.float32 and K.ndim == 2 and K.shape[0] == K.shape[1]
    n = K.shape[0]
    K64 = K.astype(np.float64)
    a = restate_start(nu, n)
    G = np.zeros(n)
    for r in np.flatnonzero(a):
        G = G + K64[r] * a[r]
    max_iter = 100 * n if max_iter is None else max_iter
    path, n_iter, converged = [], 0, False
    while n_iter < max_iter:
        up, low = a < 1.0, a > 0.0
        if not up.any():
            converged = True
            break
        neg = np.where(up, -G, -np.inf)
        i = int(np.argmax(neg))  # the first of the largest: the lowest index
        Gmax, Gmax2 = neg[i], G[low].max()
        if Gmax + Gmax2 < tol:
            converged = True
            break
        b = Gmax + G
        cand = low & (b > 0.0)
        if not cand.any():
            converged = True
            break
        q = 2.0 - 2.0 * K64[i]
        q = np.where(q <= 0.0, 1e-12, q)
        obj = np.where(cand, -(b * b) / q, np.inf)
        j = int(np.argmin(obj))
        delta = (G[i] - G[j]) / q[j]
        s, old_i, old_j = a[i] + a[j], a[i], a[j]
        ai, aj = old_i - delta, old_j + delta
        if s > 1.0:
            if ai > 1.0:
                ai, aj = 1.0, s - 1.0
        elif aj < 0.0:
            aj, ai = 0.0, s
        if s > 1.0:
            if aj > 1.0:
                aj, ai = 1.0, s - 1.0
        elif ai < 0.0:
            ai, aj = 0.0, s
        a[i], a[j] = ai, aj
        G = G + (K64[i] * (ai - old_i) + K64[j] * (aj - old_j))
        n_iter += 1
        path.append((i, j))
    return Fit(a, G, restate_rho(a, G), path, n_iter, converged)


def restate_scores(a, rho, Kqr):
    """float64 [nq]: rho - sum_r a_r K(q, r) for the float64 kernel Kqr [nq, nr]."""
    return rho - (np.asarray(Kqr, np.float64) * a[None, :]).sum(axis=1)


def shifted_rows(n, seed):
    """The twentieth of the rows that shifted_data moves."""
    return np.random.default_rng(1000 + seed).choice(n, max(1, n // 20), replace=False)


def shifted_data(n, d, seed, scale=False):
    """float32 [n, d]: Gaussian rows, a twentieth of them shifted by 4 sigma in every feature; with scale the columns times
    factors in [0.5, 2] plus offsets: raw, unstandardised data."""
    rng = np.random.default_rng(seed)
    X = rng.normal(size=(n, d))
    X[shifted_rows(n, seed)] += 4.0
    if scale:
        X = X * rng.uniform(0.5, 2.0, size=(1, d)) + rng.uniform(-1.0, 1.0, size=(1, d))
    return np.ascontiguousarray(X, dtype=np.float32)


def planted_data(n, d, seed):
    """(float32 [n, d], the planted rows): Gaussian rows, a twentieth of them moved by 4 sigma in every feature, each feature
    of each such row to its own side, so that the planted rows do not form a cluster of their own."""
    rng = np.random.default_rng(seed)
    X = rng.normal(size=(n, d))
    rows = shifted_rows(n, seed)
    X[rows] += 4.0 * rng.choice([-1.0, 1.0], size=(len(rows), d))
    return np.ascontiguousarray(X, dtype=np.float32), rows


def ranking_rate(scores, rows):
    """The share of the planted rows among the len(rows) highest scores."""
    return float(np.isin(np.argsort(-np.asarray(scores), kind="stable")[:len(rows)], rows).mean())


_PIN = {}


def pin_case(n, d, nu):
    """(Z float64, gamma, K float32, restatement at tol 1e-9, restatement at tol 1e-3), made once."""
    key = (n, d, nu)
    if key not in _PIN:
        Z = shifted_data(n, d, seed=n + d).astype(np.float64)
        gamma = restate_gamma(Z, "scale")
        K = host_kernel_matrix(Z, gamma)
        _PIN[key] = (Z, gamma, K, restate_smo(K, nu, tol=1e-9), restate_smo(K, nu, tol=1e-3))
    return _PIN[key]


# ---- pinned to sklearn ------------------------------------------------------------------------------------------------------
@pytest.mark.filterwarnings("ignore:Solver terminated early")
@pytest.mark.parametrize("n,d,nu", PIN_CASES)
def test_gamma_rules_are_sklearns(n, d, nu):
    from sklearn.svm import OneClassSVM
    from vgan_amd.outlier import ocsvm_block_variance, ocsvm_gamma
    Z = pin_case(n, d, nu)[0]
    for rule in ("scale", "auto"):
        want = OneClassSVM(kernel="rbf", gamma=rule, nu=nu, shrinking=False, max_iter=1).fit(Z)._gamma
        assert restate_gamma(Z, rule) == pytest.approx(want, rel=1e-12)
        # the product's host rule, from per-column means and sums of squared deviations
        mean = Z.mean(axis=0)
        var = ocsvm_block_variance(mean, ((Z - mean) ** 2).sum(axis=0), n, np.arange(d))
        assert ocsvm_gamma(rule, [d], [var])[0] == pytest.approx(want, rel=1e-12)
    assert restate_gamma(np.full((5, 3), 2.5), "scale") == 1.0 / 3 == ocsvm_gamma("scale", [3], [0.0])[0]
    assert ocsvm_gamma(0.25, [3, 9])[1] == 0.25


def test_scores_are_sklearns_at_a_tight_tolerance():
    """Both solvers at tol 1e-9: -decision_function agrees within PIN_BAR of the largest |score|.  Measured here over
    PIN_CASES: 1.18e-10 relative at n = 65 (where libsvm's highest-index tie rule takes another path: 50 iterations against
    56) and 1e-14 or less on the four cases whose iteration counts equal sklearn's; the bar is 8 times the largest."""
    from sklearn.svm import OneClassSVM
    worst = 0.0
    for n, d, nu in PIN_CASES:
        Z, gamma, K, fit, _ = pin_case(n, d, nu)
        assert fit.converged
        ref = OneClassSVM(kernel="rbf", gamma="scale", nu=nu, shrinking=False, tol=1e-9).fit(Z)
        want = -ref.decision_function(Z)
        got = restate_scores(fit.a, fit.rho, restate_kernel(Z, Z, gamma))
        rel = np.abs(got - want).max() / np.abs(want).max()
        print(f"n={n} d={d} nu={nu}: n_iter {fit.n_iter} (sklearn {int(np.ravel(ref.n_iter_)[0])}), max |score| {np.abs(want).max():.3g}, "
              f"relative difference {rel:.3g}")
        worst = max(worst, rel)
    assert worst <= PIN_BAR, worst


@pytest.mark.parametrize("n,d,nu", PIN_CASES)
def test_scores_are_sklearns_at_the_default_tolerance(n, d, nu):
    """tol 1e-3 on both sides.  The bar is 4 times the restatement's own distance between its tol 1e-3 and tol 1e-9 scores:
    two solvers may stop on opposite sides of the optimum."""
    from sklearn.svm import OneClassSVM
    Z, gamma, K, tight, loose = pin_case(n, d, nu)
    K64 = restate_kernel(Z, Z, gamma)
    got = restate_scores(loose.a, loose.rho, K64)
    own = np.abs(got - restate_scores(tight.a, tight.rho, K64)).max()
    want = -OneClassSVM(kernel="rbf", gamma="scale", nu=nu, shrinking=False, tol=1e-3).fit(Z).decision_function(Z)
    print(f"n={n} d={d} nu={nu}: own distance {own:.3g}, to sklearn {np.abs(got - want).max():.3g}")
    assert loose.converged and 0 < loose.n_iter < tight.n_iter
    assert np.abs(got - want).max() <= 4 * own


@pytest.mark.parametrize("n,d,nu", PIN_CASES)
def test_dual_coefficients_keep_the_constraints(n, d, nu):
    for fit in pin_case(n, d, nu)[3:]:
        assert fit.a.min() >= 0.0 and fit.a.max() <= 1.0
        assert abs(math.fsum(fit.a) - nu * n) <= n * 2.0 ** -52 * nu * n
        support = fit.a > 0
        assert nu * n <= support.sum() < n  # nu bounds the share of support vectors from below
        # the optimality gap the loop stopped at, from the gradient it carried
        assert (-fit.G[fit.a < 1]).max() + fit.G[support].max() < 1e-3


# ---- edge cases -------------------------------------------------------------------------------------------------------------
def test_nu_one_takes_no_iteration_and_rho_is_the_one_bound():
    Z = shifted_data(33, 4, seed=1).astype(np.float64)
    K = host_kernel_matrix(Z, 0.3)
    fit = restate_smo(K, 1.0)
    assert fit.n_iter == 0 and fit.converged and (fit.a == 1.0).all()
    assert fit.rho == fit.G.max() and np.isfinite(fit.rho)
    scores = restate_scores(fit.a, fit.rho, K.astype(np.float64))
    assert scores.min() == 0.0 and (scores >= 0).all()


def test_fewer_than_one_row_of_mass():
    Z = shifted_data(65, 5, seed=2).astype(np.float64)
    K = host_kernel_matrix(Z, restate_gamma(Z, "scale"))
    nu = 0.01  # nu n = 0.65
    fit = restate_smo(K, nu)
    assert restate_start(nu, 65)[0] == nu * 65 and (restate_start(nu, 65)[1:] == 0).all()
    assert fit.converged and fit.n_iter > 0
    assert abs(math.fsum(fit.a) - nu * 65) <= 65 * 2.0 ** -52 and (fit.a < 1).all()
    free = (fit.a > 0) & (fit.a < 1)
    assert free.sum() >= 1 and fit.rho == math.fsum(fit.G[free]) / free.sum()


def test_two_rows():
    K = np.array([[1.0, 0.25], [0.25, 1.0]], np.float32)
    fit = restate_smo(K, 0.5)  # a = (1, 0): G = (1, 0.25), one step to (0.5, 0.5)
    np.testing.assert_array_equal(fit.a, [0.5, 0.5])
    np.testing.assert_array_equal(fit.G, [0.625, 0.625])
    assert (fit.n_iter, fit.converged, fit.path, fit.rho) == (1, True, [(1, 0)], 0.625)
    fit = restate_smo(K, 1.0)
    assert fit.n_iter == 0 and fit.rho == 1.25
    fit = restate_smo(K, 0.75)  # a = (1, 0.5), G = (1.125, 0.75): row 1 takes mass from row 0 until both hold 0.75
    assert fit.converged and abs(fit.a.sum() - 1.5) < 1e-15 and fit.a[0] == pytest.approx(0.75) and fit.a[1] == pytest.approx(0.75)


@pytest.mark.parametrize("nu", [0.5, 0.1, 0.37])
def test_a_constant_subspace_scores_exactly_zero(nu):
    Z = np.full((65, 3), 2.5)
    gamma = restate_gamma(Z, "scale")
    assert gamma == 1.0 / 3
    K = host_kernel_matrix(Z, gamma)
    assert (K == 1.0).all()
    fit = restate_smo(K, nu)
    assert fit.n_iter == 0 and fit.converged and fit.rho == nu * 65
    np.testing.assert_array_equal(restate_scores(fit.a, fit.rho, K.astype(np.float64)), np.zeros(65))


def test_max_iter_cuts_the_loop_off():
    Z, gamma, K, _, loose = pin_case(257, 17, 0.1)
    cut = restate_smo(K, 0.1, max_iter=10)
    assert cut.n_iter == 10 and not cut.converged and cut.path == loose.path[:10]
    exact = restate_smo(K, 0.1, max_iter=loose.n_iter)  # the budget ends where the stop rule would have been looked at
    assert exact.n_iter == loose.n_iter and not exact.converged
    np.testing.assert_array_equal(exact.a, loose.a)


def test_planted_outliers_rank_on_top():
    X, rows = planted_data(1025, 16, seed=7)
    Z = X.astype(np.float64)
    gamma = restate_gamma(Z, "scale")
    for nu in (0.1, 0.5):
        fit = restate_smo(host_kernel_matrix(Z, gamma), nu)
        assert ranking_rate(restate_scores(fit.a, fit.rho, restate_kernel(Z, Z, gamma)), rows) > 0.9


# ---- the constructor and the host rules, without a device -------------------------------------------------------------------
def test_constructor_validates_without_touching_the_device():
    import vgan_amd
    from vgan_amd import outlier
    m = _mask(4, [[0, 1], [1, 2, 3]])
    ens = vgan_amd.SubspaceOCSVM(m, [0.5, 0.5])
    assert (ens.nu, ens.gamma, ens.tol, ens.max_iter, ens.engine, ens.splits, ens.normalize, ens.combination,
            ens.contamination) == (0.5, "scale", 1e-3, None, "auto", None, None, "sum", 0.1)
    assert isinstance(ens, outlier._SubspaceScorer)
    for bad in (0, 0.0, -0.1, 1.5, float("nan"), "half", None, True):
        with pytest.raises(ValueError, match="nu must be"):
            vgan_amd.SubspaceOCSVM(m, [0.5, 0.5], nu=bad)
    for bad in (0, -1.0, float("inf"), float("nan"), "median", None, True):
        with pytest.raises(ValueError, match="gamma must be"):
            vgan_amd.SubspaceOCSVM(m, [0.5, 0.5], gamma=bad)
    for bad in (0, -1e-3, float("inf"), float("nan"), "1e-3", None, True):
        with pytest.raises(ValueError, match="tol must be"):
            vgan_amd.SubspaceOCSVM(m, [0.5, 0.5], tol=bad)
    for bad in (0, -1, 2.5, 2 ** 31, "10", True):
        with pytest.raises(ValueError, match="max_iter must be"):
            vgan_amd.SubspaceOCSVM(m, [0.5, 0.5], max_iter=bad)
    for bad in (0, 65536):
        with pytest.raises(ValueError, match="splits"):
            vgan_amd.SubspaceOCSVM(m, [0.5, 0.5], splits=bad)
    ok = vgan_amd.SubspaceOCSVM(m, [0.5, 0.5], nu=1, gamma=np.float32(0.5), tol=np.float64(1e-9), max_iter=np.int64(7), splits=3,
                                engine="gram")
    assert (ok.nu, ok.gamma, ok.tol, ok.max_iter, ok.splits, ok.engine) == (1.0, 0.5, 1e-9, 7, 3, "gram")
    assert vgan_amd.SubspaceOCSVM(m, [0.5, 0.5], gamma="auto").gamma == "auto"
    with pytest.raises(ValueError, match="proba has 3 entries for 2 subspaces"):
        vgan_amd.SubspaceOCSVM(m, [0.5, 0.25, 0.25])
    with pytest.raises(ValueError, match="normalize"):
        vgan_amd.SubspaceOCSVM(m, [0.5, 0.5], normalize="l2")
    with pytest.raises(ValueError, match="combination"):
        vgan_amd.SubspaceOCSVM(m, [0.5, 0.5], combination="mean")
    with pytest.raises(ValueError, match="contamination"):
        vgan_amd.SubspaceOCSVM(m, [0.5, 0.5], contamination=0.7)
    with pytest.raises(ValueError, match="engine"):
        vgan_amd.SubspaceOCSVM(m, [0.5, 0.5], engine="fast")
    for rows in (1, outlier.OCSVM_MAX_ROWS + 1):
        with pytest.raises(ValueError, match="between 2 and 32768"):
            ens.fit(np.zeros((rows, 4), np.float32))
    with pytest.raises(ValueError, match="features"):
        ens.fit(np.zeros((5, 3), np.float32))
    assert ens.ops is None  # none of this touched the device
    with pytest.raises(RuntimeError, match="not fitted"):
        ens.decision_function(np.zeros((5, 4), np.float32))
    doc = vgan_amd.SubspaceOCSVM.__doc__
    for word in ("shrinking", "kernel cache", "coef0", "lowest index", "1e-12", "2^44", "this class's own rule", "exactly 0",
                 "bit for bit", "100 n"):
        assert word in doc, word


def test_host_rules():
    from vgan_amd import outlier
    assert outlier.ocsvm_start(0.5, 65) == (32, 0.5) and outlier.ocsvm_start(1.0, 7) == (7, 0.0)
    assert outlier.ocsvm_start(0.01, 65) == (0, 0.01 * 65)
    for nu, n in ((0.1, 65), (0.37, 1025), (0.5, 2)):
        m, a_m = outlier.ocsvm_start(nu, n)
        np.testing.assert_array_equal(restate_start(nu, n), np.r_[np.ones(m), [a_m], np.zeros(n - m - 1)])
    # chunks: the kernel matrices count against the workspace, one engine per chunk, a lone subspace that exceeds it stays
    plan = outlier.SubspacePlan(_mask(70, [list(range(40)), [0], [1, 2], list(range(33)), [5]]))
    n = 100
    assert outlier.ocsvm_chunks(plan, n, 1 << 30) == [(0, 3, False), (3, 2, True)]
    assert outlier.ocsvm_chunks(plan, n, 1) == [(z, 1, z >= 3) for z in range(5)]
    two = 2 * (n * n * 4 + n * 5 * 4)
    assert outlier.ocsvm_chunks(plan, n, two) == [(0, 2, False), (2, 1, False), (3, 1, True), (4, 1, True)]


def test_outlier_ensemble_routes_ocsvm_to_the_new_class():
    import vgan_amd
    model = vgan_amd.VGAN_no_kl(epochs=1)
    model.subspaces = _mask(6, [[0, 1], [2, 3, 5], [4]])
    model.proba = np.array([0.5, 0.3, 0.2])
    ens = model.outlier_ensemble(method="ocsvm")
    assert type(ens) is vgan_amd.SubspaceOCSVM and ens.nu == 0.5 and ens.plan.count == 3
    np.testing.assert_array_equal(ens.proba, model.proba)
    ens = model.outlier_ensemble(method="ocsvm", n_neighbors=17, nu=0.1, gamma="auto", tol=1e-4, max_iter=50, engine="exact", splits=2,
                                 normalize="zscore", combination="max", contamination=0.05, workspace_bytes=1 << 20)
    assert (ens.nu, ens.gamma, ens.tol, ens.max_iter, ens.engine, ens.splits, ens.normalize, ens.combination, ens.contamination,
            ens.workspace_bytes) == (0.1, "auto", 1e-4, 50, "exact", 2, "zscore", "max", 0.05, 1 << 20)
    with pytest.raises(TypeError):
        model.outlier_ensemble(method="ocsvm", kernel="linear")  # only the RBF kernel is built
    assert '"ocsvm"' in vgan_amd.VGAN_no_kl.outlier_ensemble.__doc__ and "SubspaceOCSVM" in vgan_amd.__all__
    with pytest.raises(ValueError, match="method must be 'knn', 'lof' or 'kde'"):  # the neighbour ensemble does not know it
        vgan_amd.SubspaceEnsemble(model.subspaces, model.proba, method="ocsvm")


# ---- C ABI: argument checks without a GPU -----------------------------------------------------------------------------------
def test_ocsvm_entries_reject_bad_arguments_without_gpu():
    import vgan_amd
    from vgan_amd import outlier
    lib = vgan_amd.lib.load()
    header = open(os.path.join(REPO, "include", "vgan_hip.h")).read()
    assert int(re.search(r"#define VGAN_OCSVM_MAX_ROWS (\d+)", header).group(1)) == outlier.OCSVM_MAX_ROWS
    assert int(re.search(r"#define VGAN_OCSVM_LDS_ROWS (\d+)", header).group(1)) == outlier.OCSVM_LDS_ROWS
    for name, value in outlier.OCSVM_STORAGE.items():
        assert int(re.search(rf"#define VGAN_OCSVM_STORAGE_{name.upper()} (\d+)", header).group(1)) == value
    null = None
    buf = ctypes.create_string_buffer(256)
    p = ctypes.cast(ctypes.addressof(buf) + (-ctypes.addressof(buf)) % 16, ctypes.c_void_p)  # never read
    odd = ctypes.c_void_p(p.value + 4)

    def rejected(rc):
        msg = lib.vgan_last_error()
        return rc == 1 and b"bad argument" in msg and b"outlier_ocsvm.hip" in msg

    def each(fn, good, pointers, bad_values):
        for pos in pointers:
            assert rejected(fn(*[null if i == pos else v for i, v in enumerate(good)])), pos
        for pos, bad in bad_values:
            assert rejected(fn(*[bad if i == pos else v for i, v in enumerate(good)])), (pos, bad)

    big = outlier.OCSVM_MAX_ROWS + 1
    # P, sq, n, feat_off, col_off, first, count, gamma, engine, splits, K, stream
    each(lib.vgan_ocsvm_kernel_matrix, [p, p, 10, p, p, 0, 2, p, 1, 1, p, null], (0, 1, 3, 4, 7, 10),
         [(0, odd), (2, 1), (2, 0), (2, big), (5, -1), (6, 0), (6, 65536), (8, 2), (8, -1), (9, 0), (9, 65536)])
    assert rejected(lib.vgan_ocsvm_kernel_matrix(null, null, 0, null, null, 0, 0, null, 0, 0, null, null))
    # K, n, count, m, a_m, alpha, G, done, n_iter, stream
    each(lib.vgan_ocsvm_init, [p, 10, 2, 5, 0.5, p, p, p, p, null], (0, 5, 6, 7, 8),
         [(1, 1), (1, big), (2, 0), (2, 65536), (3, -1), (3, 11), (4, 1.0), (4, -0.5), (4, float("nan"))])
    assert rejected(lib.vgan_ocsvm_init(p, 10, 2, 10, 0.5, p, p, p, p, null))  # m = n leaves no row for a_m
    assert rejected(lib.vgan_ocsvm_init(p, 10, 2, 0, 0.0, p, p, p, p, null))  # no mass at all
    # K, n, count, tol, max_iter, iterations, storage, alpha, G, done, n_iter, stream
    each(lib.vgan_ocsvm_smo, [p, 10, 2, 1e-3, 100, 8, 0, p, p, p, p, null], (0, 7, 8, 9, 10),
         [(1, 1), (1, big), (2, 0), (3, 0.0), (3, -1.0), (3, float("nan")), (4, 0), (5, 0), (6, 4), (6, -1)])
    assert rejected(lib.vgan_ocsvm_smo(p, outlier.OCSVM_LDS_ROWS + 1, 2, 1e-3, 100, 8, outlier.OCSVM_STORAGE["lds"], p, p, p, p, null))
    # alpha, G, n, count, rho, stream
    each(lib.vgan_ocsvm_rho, [p, p, 10, 2, p, null], (0, 1, 4), [(2, 1), (2, big), (3, 0)])
    # Pq, sq_q, nq, Pr, sq_r, nr, feat_off, col_off, first, count, gamma, alpha, rho, engine, splits, acc, score, score_row, ld, stream
    each(lib.vgan_ocsvm_scores, [p, p, 7, p, p, 10, p, p, 0, 2, p, p, p, 1, 1, p, p, null, 7, null], (0, 1, 3, 4, 6, 7, 10, 11, 12, 15, 16),
         [(0, odd), (3, odd), (2, 0), (5, 1), (5, big), (8, -1), (9, 0), (9, 65536), (13, 2), (14, 0), (14, 65536), (18, 6)])
    for name, nargs in (("vgan_ocsvm_kernel_matrix", 12), ("vgan_ocsvm_init", 10), ("vgan_ocsvm_smo", 12), ("vgan_ocsvm_rho", 6),
                        ("vgan_ocsvm_scores", 20)):
        assert len(vgan_amd.lib.SIGNATURES[name][1]) == nargs
    text = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    assert sorted(vgan_amd.lib.SIGNATURES) == sorted(set(re.findall(r"\b(vgan_[a-z0-9_]+)\s*\(", text)))
    assert vgan_amd.lib.ABI_VERSION == lib.vgan_abi_version() == 11  # symbols were only added
