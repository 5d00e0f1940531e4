"""Kernel PCA novelty scores over the subspaces, CPU tier: the float64 numpy restatement the GPU tests compare against,
pinned to sklearn's KernelPCA and KernelCenterer; the Jacobi restatement of test_outlier_pca_cpu.py on centred kernel
matrices; and everything of vgan_amd.SubspaceKPCA that runs without a device (argument checks, the landmark, component and
chunk rules, the dispatch from the model, the C ABI's argument checks).

The definition (SubspaceKPCA's docstring).  K float32 [m, m] over the landmark rows, K' the symmetric matrix of its entries
K[r][c], r <= c; colmean_c = (sum_r K'[r][c], r ascending) / m; tot = (sum_c colmean_c, c ascending) / m; Kc[i][j] = ((K'[i][j] -
colmean_j) - colmean_i) + tot for i <= j, mirrored; Kc = V^T Lambda V descending, rows signed by their entry of largest
magnitude; component j usable iff lambda_j > eig_tol lambda_0; q from n_components over the usable ones; w_j = 1 / lambda_j for
j < q.  A row with kernel values k_c against the landmarks: rowmean = the mean of k_c (64 strided partials, the xor
butterfly, / m), z_c = ((k_c - rowmean) - colmean_c) + tot, y = V z, proj = sum_j w_j y_j^2, pot = (1 - 2 rowmean) + tot, score =
float32(max(pot - proj, 0)).

Against sklearn: the eigenvalues of Kc are KernelPCA.eigenvalues_, |y_j| / sqrt(lambda_j) is |KernelPCA.transform|, and the
score is k(x, x) - 2 mean_c k_c + tot - ||transform(x)||^2 (Hoffmann 2007).  The centring differs from KernelCenterer only in
the order of its sums: both form a mean of m values in [0, 1] (error at most m u each, u = 2^-53, first order) and then
three rounded operations on values of magnitude at most 2, so the two agree within (2 m + 8) u; the test prints what it
sees (a few u)."""
import ctypes
import os
import re

import numpy as np
import pytest

from conftest import REPO
from test_outlier_ecod_cpu import _mask
from test_outlier_ocsvm_cpu import host_kernel_matrix, restate_gamma, restate_kernel, shifted_data
from test_outlier_pca_cpu import (K_EIGENVALUE, TOL_PIN, U, component_count, decomposition_errors, restate_eigh, restate_jacobi,
                                  sign_rule_holds)

MAX_LANDMARKS = 1024  # VGAN_KPCA_MAX_LANDMARKS
EIG_TOL = 1e-6  # the constructor's default


# ---- the restatement ------------------------------------------------------------------------------------------------------
def restate_center(K):
    """(colmean [m], tot, Kc [m, m]) from the upper triangle of K (float32 as the device made it, or float64), in the
    stated order: every operation rounded on its own."""
    K = np.asarray(K, np.float64)
    m = K.shape[0]
    Ks = np.triu(K) + np.triu(K, 1).T
    acc = np.zeros(m)
    for r in range(m):  # r ascending, every column at once
        acc = acc + Ks[r]
    colmean = acc / m
    t = 0.0
    for c in range(m):
        t = t + colmean[c]
    tot = t / m
    Kc = np.triu(((Ks - colmean[None, :]) - colmean[:, None]) + tot)
    return colmean, tot, Kc + np.triu(Kc, 1).T


def restate_row_means(R):
    """float64 [n]: the mean of every row of R [n, m] in the device's order: partial l over the columns l, l + 64, ...
    ascending, the xor butterfly 32, 16, 8, 4, 2, 1 over the 64 partials, the division by m."""
    R = np.asarray(R, np.float64)
    n, m = R.shape
    pad = np.zeros((n, -(-m // 64) * 64))
    pad[:, :m] = R
    p = np.zeros((n, 64))
    for t in range(pad.shape[1] // 64):
        p = p + pad[:, 64 * t:64 * t + 64]
    lanes = np.arange(64)
    for o in (32, 16, 8, 4, 2, 1):
        p = p + p[:, lanes ^ o]
    return p[:, 0] / m


def restate_weights(lam, n_components=None, eig_tol=EIG_TOL):
    """(wt [m], q, n_usable) from the eigenvalues in descending order."""
    lam = np.asarray(lam, np.float64)
    usable = int((lam > eig_tol * lam[0]).sum()) if lam[0] > 0 else 0
    q = component_count(lam[:usable], n_components) if usable else 0
    wt = np.zeros(len(lam))
    wt[:q] = 1.0 / lam[:q]
    return wt, q, usable


def restate_scores(R, rowmean, colmean, tot, Vt, wt):
    """dict: score float64 [n] (before the float32 rounding), pot, proj, y [n, m] and term = sum_j w_j |y_j| sum_c |v_jc z_c|
    (what the GPU test's summation bar multiplies) for the kernel rows R [n, m]."""
    z = ((np.asarray(R, np.float64) - rowmean[:, None]) - colmean[None, :]) + tot
    y = z @ Vt.T
    proj = (wt[None, :] * y * y).sum(axis=1)
    pot = (1.0 - 2.0 * rowmean) + tot
    term = (wt[None, :] * np.abs(y) * (np.abs(z) @ np.abs(Vt).T)).sum(axis=1)
    return dict(score=np.maximum(pot - proj, 0.0), pot=pot, proj=proj, y=y, z=z, term=term)


def restate_fit(K, n_components=None, eig_tol=EIG_TOL, eigen=restate_eigh):
    """The fitted state from a landmark kernel matrix K."""
    colmean, tot, Kc = restate_center(K)
    lam, Vt = eigen(Kc)
    wt, q, usable = restate_weights(lam, n_components, eig_tol)
    return dict(colmean=colmean, tot=tot, Kc=Kc, lam=lam, Vt=Vt, wt=wt, q=q, usable=usable)


def restate_score_rows(fit, R):
    """The scores of the kernel rows R under a restated fit."""
    return restate_scores(R, restate_row_means(R), fit["colmean"], fit["tot"], fit["Vt"], fit["wt"])


def restate_landmarks(n, max_samples="auto", seed=0):
    m = min(n, 256 if max_samples == "auto" else max_samples)
    return np.sort(np.random.default_rng(seed).choice(n, m, replace=False))


def kernel_rows32(Zq, Zl, gamma):
    """float32 [nq, m]: the float64 kernel rounded, as the device's kernel block holds it up to its entry bar."""
    return restate_kernel(Zq, Zl, gamma).astype(np.float32)


def ring(seed, n=2000, n_out=20, d=6):
    """The issue's recipe: a noisy circle of radius 3 in the first two of six features, 20 rows moved to its centre."""
    r = np.random.default_rng(seed)
    t = r.uniform(0, 2 * np.pi, n)
    X = r.normal(0, 0.3, (n, d))
    X[:, 0] = 3 * np.cos(t) + r.normal(0, 0.15, n)
    X[:, 1] = 3 * np.sin(t) + r.normal(0, 0.15, n)
    y = np.zeros(n, int)
    o = r.choice(n, n_out, replace=False)
    y[o] = 1
    X[o, 0] = r.normal(0, 0.5, n_out)
    X[o, 1] = r.normal(0, 0.5, n_out)
    return X.astype(np.float32), y


def ring_gamma(X):
    return 4.0 / (X.shape[1] * X.astype(np.float64).var())


RING_COMPONENTS = 8


def restate_ring_scores(X):
    Z = X.astype(np.float64)
    L = Z[restate_landmarks(len(Z))]
    g = ring_gamma(X)
    fit = restate_fit(host_kernel_matrix(L, g), RING_COMPONENTS)
    return restate_score_rows(fit, kernel_rows32(Z, L, g))["score"]


def duplicated_landmarks(m, d=5, seed=0):
    """float64 [m, d]: Gaussian rows, the last a copy of the first (m > 2) -- a singular kernel matrix."""
    Z = shifted_data(m, d, seed=seed + m).astype(np.float64)
    if m > 2:
        Z[-1] = Z[0]
    return Z


# ---- pinned to sklearn ----------------------------------------------------------------------------------------------------
PIN_CASES = [(200, 13, 60), (130, 5, 8), (65, 33, 20)]  # (m, d_s, q)


@pytest.mark.parametrize("m,d,q", PIN_CASES)
def test_decomposition_transform_and_score_are_sklearns(m, d, q):
    from sklearn.decomposition import KernelPCA
    Z = shifted_data(m + 77, d, seed=m + d, scale=True).astype(np.float64)
    L, Y = Z[:m], Z[m:]
    g = restate_gamma(L, "scale")
    ref = KernelPCA(n_components=q, kernel="rbf", gamma=g, eigen_solver="dense").fit(L)
    K = restate_kernel(L, L, g)  # float64: the pin is of the formula
    fit = restate_fit(K, q)
    assert fit["q"] == q <= fit["usable"]
    err = np.abs(fit["lam"][:q] - ref.eigenvalues_).max() / fit["lam"][0]
    R = restate_kernel(Y, L, g)
    got = restate_score_rows(fit, R)
    T = ref.transform(Y)
    terr = np.abs(np.abs(got["y"][:, :q]) / np.sqrt(fit["lam"][:q]) - np.abs(T)).max()
    want = (1.0 - 2.0 * R.mean(axis=1) + K.mean()) - (T * T).sum(axis=1)
    serr = np.abs(got["score"] - np.maximum(want, 0.0)).max()
    print(f"m={m} q={q}: eigenvalues {err:.1e} transform {terr:.1e} score {serr:.1e}")
    assert err <= TOL_PIN and terr <= TOL_PIN and serr <= TOL_PIN
    assert (got["score"] > 0).any()


@pytest.mark.parametrize("m", [2, 3, 49, 65, 130])
def test_centring_is_symmetric_to_the_bit_and_kernel_centerers_within_a_few_ulps(m):
    from sklearn.preprocessing import KernelCenterer
    L = duplicated_landmarks(m)
    K = host_kernel_matrix(L, restate_gamma(L, "scale"))
    K[np.tril_indices(m, -1)] = K[np.tril_indices(m, -1)] * np.float32(1 + 2.0 ** -20)  # the lower triangle is not read
    colmean, tot, Kc = restate_center(K)
    np.testing.assert_array_equal(Kc, Kc.T)
    Ks = np.triu(K.astype(np.float64)) + np.triu(K.astype(np.float64), 1).T
    want = KernelCenterer().fit_transform(Ks)
    err = np.abs(Kc - want).max() / U
    print(f"m={m}: centring against KernelCenterer {err:.2f} u")
    assert err <= 2 * m + 8
    assert abs(colmean.mean() - Ks.mean()) <= m * U and abs(tot - Ks.mean()) <= 2 * m * U
    assert np.abs(Kc.sum(axis=0)).max() <= 4 * m * m * U  # centred


def test_row_means_in_the_stated_order():
    rng = np.random.default_rng(3)
    for m in (2, 3, 63, 64, 65, 130, 256):
        R = rng.uniform(0, 1, (7, m)).astype(np.float32)
        got = restate_row_means(R)
        assert (np.abs(got - R.astype(np.float64).mean(axis=1)) <= (m // 64 + 8) * U).all()
    np.testing.assert_array_equal(restate_row_means(np.ones((3, 130), np.float32)), np.ones(3))


@pytest.mark.parametrize("m", [2, 3, 49, 65])
def test_jacobi_restatement_converges_on_centred_kernel_matrices(m):
    L = duplicated_landmarks(m)
    _, _, Kc = restate_center(host_kernel_matrix(L, restate_gamma(L, "scale")))
    lam, Vt, sweeps, converged = restate_jacobi(Kc)
    res, ev, orth = decomposition_errors(Kc, lam, Vt)
    print(f"m={m}: sweeps {sweeps} eigenvalue error {ev:.2f} of m u ||M||_2")
    assert converged and 1 <= sweeps <= 30 and ev <= K_EIGENVALUE
    assert (np.diff(lam) <= 0).all() and sign_rule_holds(Vt)
    assert abs(lam[-1]) <= K_EIGENVALUE * m * U * lam[0]  # a centred matrix has a zero eigenvalue


# ---- component selection --------------------------------------------------------------------------------------------------
def test_component_selection_rules():
    from vgan_amd.outlier import kpca_weights
    lam = np.array([4.0, 2.0, 1.0, 0.5, 3e-6, 1e-9, 0.0, -1e-12])
    for nc, q in ((None, 4), (1, 1), (3, 3), (4, 4), (5, 4), (100, 4), (0.5, 1), (0.6, 2), (0.8, 3), (0.99, 4)):
        wt, got_q, usable = kpca_weights(lam, nc, EIG_TOL)
        want = restate_weights(lam, nc)
        assert (got_q, usable) == (q, 4) == want[1:], nc
        np.testing.assert_array_equal(wt, want[0])
        np.testing.assert_array_equal(wt[:q], 1.0 / lam[:q])
        assert (wt[q:] == 0).all()
    assert kpca_weights(lam, None, 1e-7)[1:] == (5, 5) and kpca_weights(lam, None, 0.0)[1:] == (6, 6)  # the eig_tol rule
    for const in (np.zeros(5), np.array([0.0, 0.0, -1e-18])):  # a constant subspace: Kc = 0, no usable component
        wt, q, usable = kpca_weights(const, None, EIG_TOL)
        assert (q, usable) == (0, 0) and (wt == 0).all()


def test_a_constant_subspace_scores_exactly_zero_in_the_restatement():
    m = 65
    fit = restate_fit(np.ones((m, m), np.float32))
    assert fit["tot"] == 1.0 and (fit["colmean"] == 1.0).all() and (fit["Kc"] == 0).all() and fit["usable"] == 0
    got = restate_score_rows(fit, np.ones((9, m), np.float32))
    assert (got["pot"] == 0).all() and (got["score"] == 0).all()


def test_more_components_than_usable_takes_the_usable_ones():
    L = duplicated_landmarks(49)
    K = host_kernel_matrix(L, restate_gamma(L, "scale"))
    every, many = restate_fit(K, None), restate_fit(K, 10 ** 6)
    assert every["q"] == many["q"] == every["usable"] < 49
    np.testing.assert_array_equal(every["wt"], many["wt"])


# ---- the landmark and chunk rules -----------------------------------------------------------------------------------------
def test_landmark_rule():
    from vgan_amd.outlier import check_kpca_landmarks, resolve_kpca_landmarks
    for n, ms, seed in ((10, "auto", 0), (257, "auto", 3), (2000, "auto", 0), (2000, 1024, 1), (5, 64, 2)):
        got = resolve_kpca_landmarks(None, ms, n, seed)
        np.testing.assert_array_equal(got, restate_landmarks(n, ms, seed))
        assert got.dtype == np.int64 and len(got) == min(n, 256 if ms == "auto" else ms)
    given = check_kpca_landmarks([5, 1, 3])
    np.testing.assert_array_equal(resolve_kpca_landmarks(given, "auto", 6, 0), [5, 1, 3])  # the given order
    with pytest.raises(ValueError, match="out of range for 5 rows"):
        resolve_kpca_landmarks(given, "auto", 5, 0)


def test_chunk_rule_fits_the_workspace_and_covers_every_subspace():
    from vgan_amd.outlier import SubspacePlan, kpca_chunks, kpca_fit_chunks
    plan = SubspacePlan(_mask(70, [list(range(1)), list(range(5)), list(range(40)), list(range(70)), list(range(3))]))
    m, rows = 130, 1000
    for limit in (1, 50_000, 400_000, 1 << 30):
        chunks = kpca_chunks(plan, m, rows, limit)
        assert [c[0] for c in chunks] == list(np.cumsum([0] + [c[1] for c in chunks[:-1]])) and sum(c[1] for c in chunks) == plan.count
        for first, count, gram, slab in chunks:
            assert (plan.gram[first:first + count] == gram).all() and 1 <= slab <= rows and (slab == rows or slab % 64 == 0)
            w = (plan.dims[first:first + count] + 3) // 4 * 4
            need = int((m * (w + 1) * 4).sum() + slab * (m * 4 + 8 + (w + 1) * 4).sum())
            assert need <= limit or (count == 1 and slab == 64)  # a piece that alone exceeds it forms its own chunk
        fit = kpca_fit_chunks(plan, m, limit)
        assert sum(c[1] for c in fit) == plan.count and all((plan.gram[f:f + c] == g).all() for f, c, g in fit)
    assert len(kpca_chunks(plan, m, rows, 1)) == plan.count == len(kpca_fit_chunks(plan, m, 1))
    assert kpca_chunks(plan, m, 10, 1)[0][3] == 10  # fewer rows than a slab
    assert len(kpca_chunks(plan, m, rows, 1 << 30)) == 2  # one chunk an engine


# ---- the constructor, without a device ----------------------------------------------------------------------------------------
def test_constructor_validates_without_touching_the_device():
    import vgan_amd
    from vgan_amd import outlier
    m = _mask(4, [[0, 1], [1, 2, 3]])
    p = [0.5, 0.5]
    ens = vgan_amd.SubspaceKPCA(m, p)
    assert (ens.n_components, ens.gamma, ens.max_samples, ens.landmarks, ens.eig_tol, ens.max_sweeps, ens.seed, ens.engine, ens.splits,
            ens.normalize, ens.combination, ens.contamination) == (None, "scale", "auto", None, 1e-6, 30, 0, "auto", None, None, "sum", 0.1)
    assert ens.max_sweeps == vgan_amd.SubspacePCA(m, p).max_sweeps and isinstance(ens, outlier._SubspaceScorer)
    assert ens.keep_kernel_matrix is False
    for bad in (0, -1, 1.0, 1.5, 0.0, float("nan"), "mle", True):
        with pytest.raises(ValueError, match="n_components"):
            vgan_amd.SubspaceKPCA(m, p, n_components=bad)
    for bad in (0, -1.0, float("inf"), float("nan"), "rbf", None):
        with pytest.raises(ValueError, match="gamma"):
            vgan_amd.SubspaceKPCA(m, p, gamma=bad)
    for bad in (1, 0, MAX_LANDMARKS + 1, 2.5, "all", None, True):
        with pytest.raises(ValueError, match="max_samples"):
            vgan_amd.SubspaceKPCA(m, p, max_samples=bad)
    for bad in ([1], [1, 1], [0, -1], [0.5, 1.5], [[0, 1]], "rows", 3, list(range(MAX_LANDMARKS + 1))):
        with pytest.raises(ValueError, match="landmarks"):
            vgan_amd.SubspaceKPCA(m, p, landmarks=bad)
    for bad in (-1e-9, 1.0, float("nan"), None, "tight"):
        with pytest.raises(ValueError, match="eig_tol"):
            vgan_amd.SubspaceKPCA(m, p, eig_tol=bad)
    for bad in (0, -1, 2.0, None, True):
        with pytest.raises(ValueError, match="max_sweeps"):
            vgan_amd.SubspaceKPCA(m, p, max_sweeps=bad)
    for bad in (-1, 1.5, None, 1 << 64):
        with pytest.raises(ValueError, match="seed"):
            vgan_amd.SubspaceKPCA(m, p, seed=bad)
    for bad in (0, 65536):
        with pytest.raises(ValueError, match="splits"):
            vgan_amd.SubspaceKPCA(m, p, splits=bad)
    with pytest.raises(ValueError, match="engine"):
        vgan_amd.SubspaceKPCA(m, p, engine="fast")
    ok = vgan_amd.SubspaceKPCA(m, p, n_components=0.9, gamma="auto", max_samples=MAX_LANDMARKS, landmarks=np.array([3, 0, 2]), eig_tol=0,
                               max_sweeps=1, seed=7, engine="gram", splits=3)
    assert (ok.n_components, ok.gamma, ok.max_samples, ok.eig_tol, ok.max_sweeps, ok.seed, ok.engine, ok.splits) == (
        0.9, "auto", MAX_LANDMARKS, 0.0, 1, 7, "gram", 3)
    assert ok.landmarks.dtype == np.int64 and list(ok.landmarks) == [3, 0, 2]
    assert outlier.check_kpca_params(np.int64(3), 2, np.int32(7), None, 0.5, np.int32(7), np.int64(1)) == (3, 2.0, 7, None, 0.5, 7, 1)
    assert outlier.KPCA_MAX_LANDMARKS == MAX_LANDMARKS == outlier.MAHA_MAX_DIMS and outlier.KPCA_MAX_ROWS == 1 << 24
    with pytest.raises(ValueError, match="proba has 3 entries for 2 subspaces"):
        vgan_amd.SubspaceKPCA(m, [0.5, 0.25, 0.25])
    for name, bad in (("normalize", "l2"), ("combination", "mean"), ("contamination", 0.7)):
        with pytest.raises(ValueError, match=name):
            vgan_amd.SubspaceKPCA(m, p, **{name: bad})
    with pytest.raises(ValueError, match="between 2 and"):
        ens.fit(np.zeros((1, 4), np.float32))
    with pytest.raises(ValueError, match="features"):
        ens.fit(np.zeros((5, 3), np.float32))
    assert ens.ops is None  # none of this touched the device
    for use in (lambda: ens.components_, lambda: ens.decision_function(np.zeros((5, 4), np.float32)),
                lambda: ens.kernel_rows(np.zeros((5, 4), np.float32), 0)):
        with pytest.raises(RuntimeError, match="not fitted"):
            use()
    doc = " ".join(vgan_amd.SubspaceKPCA.__doc__.split())
    for word in ("Hoffmann 2007", "default_rng(seed).choice(n, m, replace=False)", "r <= c", "eig_tol lambda_0", "1 / lambda_j",
                 "(1.0 - 2.0 rowmean) + tot", "exactly 0", "bit for bit", "fit_inverse_transform", "pre-images", "precomputed",
                 "subset_size", "Lanczos", "keep_kernel_matrix", "kernel_rows"):
        assert word in doc, word


def test_outlier_ensemble_routes_kpca_to_the_new_class():
    import vgan_amd
    model = vgan_amd.VGAN_no_kl(epochs=1)
    model.subspaces = _mask(6, [[0, 1], [2, 3, 5], [4]])
    model.proba = np.array([0.5, 0.3, 0.2])
    ens = model.outlier_ensemble(method="kpca")
    assert type(ens) is vgan_amd.SubspaceKPCA and ens.n_components is None and ens.plan.count == 3
    np.testing.assert_array_equal(ens.proba, model.proba)
    ens = model.outlier_ensemble(method="kpca", n_neighbors=17, n_components=8, gamma=0.25, max_samples=64, eig_tol=1e-5, max_sweeps=9,
                                 seed=4, engine="exact", splits=2, normalize="zscore", combination="max", contamination=0.05,
                                 workspace_bytes=1 << 20)  # n_neighbors is ignored
    assert (ens.n_components, ens.gamma, ens.max_samples, ens.eig_tol, ens.max_sweeps, ens.seed, ens.engine, ens.splits, ens.normalize,
            ens.combination, ens.contamination, ens.workspace_bytes) == (8, 0.25, 64, 1e-5, 9, 4, "exact", 2, "zscore", "max", 0.05, 1 << 20)
    with pytest.raises(TypeError):
        model.outlier_ensemble(method="kpca", nu=0.1)  # not a keyword of SubspaceKPCA
    assert '"kpca"' in vgan_amd.VGAN_no_kl.outlier_ensemble.__doc__ and "SubspaceKPCA" in vgan_amd.__all__
    with pytest.raises(ValueError, match="method"):  # the neighbour ensemble does not know it
        vgan_amd.SubspaceEnsemble(model.subspaces, model.proba, method="kpca")


# ---- C ABI: argument checks without a GPU -----------------------------------------------------------------------------------
def test_kpca_entries_reject_bad_arguments_without_gpu():
    import vgan_amd
    from vgan_amd import outlier
    lib = vgan_amd.lib.load()
    header = open(os.path.join(REPO, "include", "vgan_hip.h")).read()
    assert int(re.search(r"#define VGAN_KPCA_MAX_LANDMARKS (\d+)", header).group(1)) == outlier.KPCA_MAX_LANDMARKS
    null = None
    buf = ctypes.create_string_buffer(256)
    p = ctypes.cast(ctypes.addressof(buf) + (-ctypes.addressof(buf)) % 16, ctypes.c_void_p)  # never read
    odd = ctypes.c_void_p(p.value + 4)

    def rejected(rc):
        msg = lib.vgan_last_error()
        return rc == 1 and b"bad argument" in msg and b"outlier_kpca.hip" in msg

    def each(fn, good, pointers, bad_values):
        for pos in pointers:
            assert rejected(fn(*[null if i == pos else v for i, v in enumerate(good)])), pos
        for pos, bad in bad_values:
            assert rejected(fn(*[bad if i == pos else v for i, v in enumerate(good)])), (pos, bad)

    big = MAX_LANDMARKS + 1
    # K, m, count, col_mean, total, Kc, stream
    each(lib.vgan_kpca_center, [p, 5, 2, p, p, p, null], (0, 3, 4, 5), [(1, 1), (1, big), (2, 0), (2, 65536)])
    # Pq, sq_q, nq, Pr, sq_r, m, feat_off, col_off, first, count, gamma, engine, splits, R, stream
    good = [p, p, 10, p, p, 5, p, p, 0, 2, p, 0, 1, p, null]
    each(lib.vgan_kpca_kernel_rows, good, (0, 3, 6, 7, 10, 13),
         [(2, 0), (2, (1 << 24) + 1), (5, 1), (5, big), (8, -1), (9, 0), (9, 65536), (11, 2), (11, -1), (12, 0), (12, 65536), (0, odd),
          (3, odd)])
    gram = list(good)
    gram[11] = 1
    each(lib.vgan_kpca_kernel_rows, gram, (1, 4), [])  # the Gram engine needs both norms
    # R, rows, m, mean, stream
    each(lib.vgan_kpca_row_means, [p, 10, 5, p, null], (0, 3), [(1, 0), (1, -1), (2, 1), (2, big)])
    # R, rows, m, first, count, row_mean, col_mean, total, V, wt, score, score_row, ld_score, stream
    each(lib.vgan_kpca_scores, [p, 10, 5, 0, 2, p, p, p, p, p, p, null, 10, null], (0, 5, 6, 7, 8, 9, 10),
         [(1, 0), (1, (1 << 24) + 1), (2, 1), (2, big), (3, -1), (4, 0), (4, 65536), (12, 9)])
    for name, nargs in (("vgan_kpca_center", 7), ("vgan_kpca_kernel_rows", 15), ("vgan_kpca_row_means", 5), ("vgan_kpca_scores", 14)):
        assert len(vgan_amd.lib.SIGNATURES[name][1]) == nargs
    assert vgan_amd.lib.ABI_VERSION == lib.vgan_abi_version() == 11  # symbols were only added
    assert int(re.search(r"#define VGAN_ABI_VERSION (\d+)", header).group(1)) == 11


# ---- the ring: outliers that sit inside the data ---------------------------------------------------------------------------
@pytest.mark.parametrize("seed", range(5))
def test_kpca_finds_the_centre_of_the_ring_and_mahalanobis_does_not(seed):
    from sklearn.covariance import EmpiricalCovariance
    from sklearn.metrics import roc_auc_score
    X, y = ring(seed)
    auc = roc_auc_score(y, restate_ring_scores(X))
    maha = roc_auc_score(y, EmpiricalCovariance().fit(X.astype(np.float64)).mahalanobis(X.astype(np.float64)))
    print(f"seed {seed}: KPCA AUC {auc:.3f}, Mahalanobis AUC {maha:.3f}")
    assert auc >= 0.99
    assert maha < 0.5
