"""Kernel PCA novelty scores over the subspaces on the MI355X (csrc/outlier_kpca.hip through vgan_amd.SubspaceKPCA and the ops
wrappers), against the float64 restatement of test_outlier_kpca_cpu.py (pinned there to sklearn), never a second run of the
code under test.

Rounding the kernel entries to float32 moves every later number, so the exact comparisons run the restatement on the very
float32 matrices the device made: the centring (column means, total mean, centred matrix) and the row means have one stated
order without a product and are compared bit for bit.  The float32 entries themselves are held to float64 separately.

Bars, with u = 2^-53.  An entry of a kernel block: test_outlier_ocsvm_gpu.py's kernel_bar (K64 (gamma d2_err + (gamma d2 + 4)
2^-23) + 2^-126), restated here for this file's mask.  Decomposition, against the centred matrix recomputed on the host from
the device's K, the three bars of the PCA test with m in place of d_s: max |V V^T - I| <= 32 m u, max |V^T Lambda V - Kc| <= 16 m u
||Kc||_2, |lambda - eigvalsh(Kc)| <= 16 m u ||Kc||_2.  Scores given the device's own eigenpairs, kernel rows and means: |got - want| <=
2^-23 |want| + 4 m u sum_j w_j |y_j| sum_c |v_jc z_c| + 4 u (|pot| + proj): the final rounding, the summation bound of the projection
with a factor 4 (2 m u of it is the first-order bound of the products y_j, the rest covers the sum of the squares, since the
term is at least proj) and the three roundings of pot and of the difference; pot - proj cancels, so the bar is absolute.  End to
end against the eigh restatement on the device's K at q = 1: the same bar plus w_1 ||z||^2 E (w_1 + 2 / gap), E = 16 m u ||Kc||_2, gap =
lambda_1 - lambda_2, w_1 = 1 / lambda_1, every case asserting E (w_1 + 2 / gap) < 2^-24 on its input first.  Identity claims are
compared bit for bit."""
import numpy as np
import pytest

from outlier_checks import d2_tolerance
from test_outlier_kpca_cpu import (EIG_TOL, RING_COMPONENTS, restate_center, restate_fit, restate_landmarks, restate_row_means,
                                   restate_scores, restate_weights, ring, ring_gamma)
from test_outlier_norm_gpu import _check_scores, _check_stats
from test_outlier_ocsvm_cpu import restate_gamma, restate_sq_dists, shifted_data
from test_outlier_pca_cpu import K_EIGENVALUE, K_ORTHOGONAL, K_RESIDUAL, LDS_DIMS, U, sign_rule_holds

pytestmark = pytest.mark.gpu

GRAM_MIN_DIMS = 32
D = 70
SIZES = [1, 2, 3, GRAM_MIN_DIMS - 1, GRAM_MIN_DIMS, 70]  # both engines on either side of the threshold, and a wide one
CONST, DUP = 5, (7, 11)  # a constant column; column 11 repeats column 7
LANDMARKS = [2, 3, LDS_DIMS - 1, LDS_DIMS, LDS_DIMS + 1, 65, 130]  # the solver's LDS limit, the 64-component group, the 32-wide K slab tail
CASES = [(m, n) for m in LANDMARKS for n in (m, 257)]
NEW_ROWS = (1, 63, 65, 130)  # the 64-row workgroup edges
SETTINGS = [None, 3, 0.9]  # n_components


def edge_mask():
    """bool [6, 70]: the subspace of one feature is the constant column, the one of two adds the duplicated feature's
    original, the one of three its copy, and every wider one holds those three among its features."""
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
_DATA, _FIT = {}, {}


def features(s):
    return np.flatnonzero(MASK[s])


def engine_of(s):
    return "gram" if SIZES[s] >= GRAM_MIN_DIMS else "exact"


def case_data(m, n):
    """(X float32 [n, 70], Y float32 [130, 70]): raw rows, columns scaled and offset, a twentieth shifted; a constant and a
    duplicated column."""
    if (m, n) not in _DATA:
        rows = shifted_data(n + max(NEW_ROWS), D, seed=1000 * m + n, scale=True)
        rows[:, CONST] = np.float32(2.7)
        rows[:, DUP[1]] = rows[:, DUP[0]]
        _DATA[m, n] = (np.ascontiguousarray(rows[:n]), np.ascontiguousarray(rows[n:]))
    return _DATA[m, n]


def fitted(m, n, n_components=None):
    """The ensemble over MASK fitted on case_data(m, n)[0] with m landmarks, once for the module."""
    import vgan_amd
    key = (m, n, n_components)
    if key not in _FIT:
        ens = vgan_amd.SubspaceKPCA(MASK, PROBA, n_components=n_components, max_samples=m)
        ens.keep_kernel_matrix = True
        _FIT[key] = ens.fit(case_data(m, n)[0])
    return _FIT[key]


def kernel_bar(engine, Xq, Xr, s, d2, gamma):
    """(K64, the bar of every entry): the entry bar of test_outlier_ocsvm_gpu.py for the features of this file's mask."""
    K64 = np.exp(-gamma * d2)
    d2_err = d2_tolerance(engine, Xq, Xr, features(s), d2)
    return K64, K64 * (gamma * d2_err + (gamma * d2 + 4.0) * 2.0 ** -23) + 2.0 ** -126


def score_bar(want, m):
    return 2.0 ** -23 * np.abs(want["score"]) + 4 * m * U * want["term"] + 4 * U * (np.abs(want["pot"]) + want["proj"])


def batches(ens, X, Y):
    """[(rows, their per-subspace scores)]: the fitted rows and new rows at the workgroup edges."""
    out = [(X, ens.per_subspace_scores_)]
    for rows in NEW_ROWS:
        out.append((Y[:rows], ens.decision_function(Y[:rows], return_per_subspace=True)[1]))
    return out


def test_the_shapes_cross_every_edge():
    from vgan_amd import outlier
    assert outlier.GRAM_MIN_DIMS == GRAM_MIN_DIMS and outlier.PCA_LDS_DIMS == LDS_DIMS
    assert SIZES[:3] == [1, 2, 3] and MASK[0, CONST] and MASK[2, list(DUP)].all()
    assert [engine_of(s) for s in range(len(SIZES))] == ["exact"] * 4 + ["gram"] * 2
    assert {LDS_DIMS - 1, LDS_DIMS, LDS_DIMS + 1, 65, 130} <= set(LANDMARKS)


# ---- 1. the centring and the row means, bit for bit -------------------------------------------------------------------------
@pytest.mark.parametrize("m,n", CASES)
def test_centring_and_row_means_are_the_restatement_bit_for_bit(m, n):
    import torch
    from vgan_amd.ops import default_ops
    X, Y = case_data(m, n)
    ens = fitted(m, n)
    ops = default_ops()
    np.testing.assert_array_equal(ens.landmark_rows_, restate_landmarks(n, m, 0))
    assert ens.column_mean_.shape == (len(SIZES), m) and ens.total_mean_.shape == (len(SIZES),)
    K = np.stack(ens.kernel_matrix_)
    assert K.dtype == np.float32 and K.shape == (len(SIZES), m, m) and (K[:, np.arange(m), np.arange(m)] == 1).all()
    Kd = torch.as_tensor(K).cuda()
    cm = torch.empty(len(SIZES), m, dtype=torch.float64, device="cuda")
    tot = torch.empty(len(SIZES), dtype=torch.float64, device="cuda")
    Kc = torch.empty(len(SIZES), m, m, dtype=torch.float64, device="cuda")
    ops.kpca_center(Kd, cm, tot, Kc.view(-1))
    Kc = Kc.cpu().numpy()
    for s in range(len(SIZES)):
        colmean, total, centred = restate_center(K[s])
        np.testing.assert_array_equal(ens.column_mean_[s], colmean)
        assert ens.total_mean_[s] == total
        np.testing.assert_array_equal(cm[s].cpu().numpy(), colmean)
        np.testing.assert_array_equal(Kc[s], centred)
        np.testing.assert_array_equal(Kc[s], Kc[s].T)
        for rows in (X,) + tuple(Y[:r] for r in NEW_ROWS):
            R = ens.kernel_rows(rows, s)
            assert R.dtype == np.float32 and R.shape == (len(rows), m)
            Rd = torch.as_tensor(R[None]).cuda()
            mean = torch.empty(1, len(rows), dtype=torch.float64, device="cuda")
            ops.kpca_row_means(Rd, mean)
            np.testing.assert_array_equal(mean[0].cpu().numpy(), restate_row_means(R))
    assert (K[0] == 1).all() and (Kc[0] == 0).all() and ens.total_mean_[0] == 1  # the constant subspace


# ---- 2. the kernel entries against float64 ----------------------------------------------------------------------------------
@pytest.mark.parametrize("m,n", CASES)
def test_kernel_rows_meet_float64_within_the_entry_bar(m, n):
    X, Y = case_data(m, n)
    ens = fitted(m, n)
    L = X[ens.landmark_rows_]
    worst = 0.0
    for s in range(len(SIZES)):
        f = features(s)
        gamma = restate_gamma(X[:, f].astype(np.float64), "scale")
        assert abs(ens.gamma_[s] - gamma) <= 1e-12 * gamma
        for rows in (X,) + tuple(Y[:r] for r in NEW_ROWS):
            d2 = restate_sq_dists(rows[:, f], L[:, f])
            K64, bar = kernel_bar(engine_of(s), rows, L, s, d2, ens.gamma_[s])
            err = np.abs(ens.kernel_rows(rows, s).astype(np.float64) - K64)
            worst = max(worst, float((err / bar).max()))
            assert (err <= bar).all(), (s, len(rows), float((err / bar).max()))
        d2 = restate_sq_dists(L[:, f], L[:, f])
        K64, bar = kernel_bar(engine_of(s), L, L, s, d2, ens.gamma_[s])
        assert (np.abs(ens.kernel_matrix_[s].astype(np.float64) - K64) <= bar).all(), s
    print(f"m={m} n={n}: worst kernel entry error {worst:.3f} of its bar")


@pytest.mark.parametrize("splits", [1, 3])
@pytest.mark.parametrize("m", [2, 65, 130])
@pytest.mark.parametrize("width", [3, 40])  # one subspace per engine
def test_the_square_and_the_rectangular_kernel_are_one_kernel(width, m, splits):
    """vgan_ocsvm_kernel_matrix (by reference row, unit diagonal) and vgan_kpca_kernel_rows (by query row) of the same packed
    block on both sides: a pair's d2 does not depend on who asks and both apply rbf_entry, so K[c][q] == R[q][c] bit for bit off
    the diagonal, and K's diagonal is exactly 1."""
    import torch
    import vgan_amd
    from vgan_amd.outlier import ENGINES
    mask = np.zeros((1, D), bool)
    mask[0, :width] = True
    ens = vgan_amd.SubspaceKPCA(mask, [1.0], max_samples=m).fit(case_data(m, m)[0])
    gram = width >= GRAM_MIN_DIMS
    assert bool(ens.plan.gram[0]) == gram and ens._L.shape[0] == m
    P, sq = ens._pack(ens._L, 0, 1, gram)
    K = torch.full((1, m, m), float("nan"), dtype=torch.float32, device="cuda")
    R = torch.full((1, m, m), float("nan"), dtype=torch.float32, device="cuda")
    engine = ENGINES["gram" if gram else "exact"]
    ens.ops.ocsvm_kernel_matrix(P, sq, m, ens._table, 0, 1, ens._gamma, engine, splits, K)
    ens.ops.kpca_kernel_rows(P, sq, m, P, sq, m, ens._table, 0, 1, ens._gamma, engine, splits, R)
    K, R = K[0].cpu().numpy(), R[0].cpu().numpy()
    off = ~np.eye(m, dtype=bool)
    assert not np.isnan(K).any() and not np.isnan(R).any()
    assert np.array_equal(K[off], R.T[off])
    assert (np.diag(K) == 1).all()


# ---- 3. the decomposition ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("m,n", CASES)
def test_eigenpairs_decompose_the_hosts_centred_matrix(m, n):
    ens = fitted(m, n)
    assert (ens.n_sweeps_ >= 1).all() and ens.converged_.all() and ens.converged_.dtype == bool
    for s in range(len(SIZES)):
        _, _, Kc = restate_center(ens.kernel_matrix_[s])
        lam, Vt = ens.eigenvalues_[s], ens.components_[s]
        assert lam.shape == (m,) and Vt.shape == (m, m) and lam.dtype == Vt.dtype == np.float64
        norm = np.linalg.norm(Kc, 2)
        orth = np.abs(Vt @ Vt.T - np.eye(m)).max()
        resid = np.abs(Vt.T @ (lam[:, None] * Vt) - Kc).max()
        eig = np.abs(lam - np.linalg.eigvalsh(Kc)[::-1]).max()
        print(f"m={m} n={n} d={SIZES[s]}: orth {orth / (m * U):.2f} resid {resid / (m * U * max(norm, 1e-300)):.2f} "
              f"eig {eig / (m * U * max(norm, 1e-300)):.2f} sweeps {ens.n_sweeps_[s]} usable {ens.n_usable_[s]}")
        assert orth <= K_ORTHOGONAL * m * U, (s, orth / (m * U))
        assert resid <= K_RESIDUAL * m * U * norm, (s, resid)
        assert eig <= K_EIGENVALUE * m * U * norm, (s, eig)
        assert (np.diff(lam) <= 0).all() and sign_rule_holds(Vt), s
        wt, q, usable = restate_weights(lam, None, EIG_TOL)
        assert ens.n_usable_[s] == usable == ens.n_components_[s] == q < m  # a centred matrix has a zero eigenvalue
    assert ens.n_usable_[0] == 0 and ens.n_sweeps_[0] == 1 and (ens.eigenvalues_[0] == 0).all()  # the constant subspace


# ---- 4. the scores given the device's own eigenpairs, kernel rows and means -------------------------------------------------
@pytest.mark.parametrize("n_components", SETTINGS)
@pytest.mark.parametrize("m,n", CASES)
def test_scores_follow_from_the_devices_eigenpairs(m, n, n_components):
    X, Y = case_data(m, n)
    ens = fitted(m, n, n_components)
    assert ens.per_subspace_scores_.shape == (len(SIZES), n) and ens.per_subspace_scores_.dtype == np.float32
    worst = 0.0
    for s in range(len(SIZES)):
        lam, Vt = ens.eigenvalues_[s], ens.components_[s]
        wt, q, usable = restate_weights(lam, n_components, EIG_TOL)
        assert (q, usable) == (ens.n_components_[s], ens.n_usable_[s])
        for rows, per in batches(ens, X, Y):
            R = ens.kernel_rows(rows, s)
            want = restate_scores(R, restate_row_means(R), ens.column_mean_[s], ens.total_mean_[s], Vt, wt)
            err = np.abs(per[s].astype(np.float64) - want["score"])
            bar = score_bar(want, m)
            worst = max(worst, float((err / np.maximum(bar, 1e-300)).max()))
            assert (err <= bar).all(), (s, len(rows), float((err / np.maximum(bar, 1e-300)).max()))
            assert (per[s] >= 0).all()
    print(f"m={m} n={n} n_components={n_components}: worst score error {worst:.3f} of its bar")
    assert (ens.per_subspace_scores_[0] == 0).all()  # the constant subspace


# ---- 5. end to end ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("m,n", CASES)
def test_scores_at_one_component_meet_the_eigh_restatement(m, n):
    X, Y = case_data(m, n)
    ens = fitted(m, n, 1)
    worst = 0.0
    for s in range(len(SIZES)):
        fit = restate_fit(ens.kernel_matrix_[s], 1)
        if fit["usable"] == 0:
            assert (ens.per_subspace_scores_[s] == 0).all() and ens.n_components_[s] == 0
            continue
        assert ens.n_components_[s] == 1
        w1 = fit["wt"][0]
        E = 16 * m * U * np.linalg.norm(fit["Kc"], 2)
        factor = E * (w1 + 2.0 / (fit["lam"][0] - fit["lam"][1]))
        worst = max(worst, factor)
        assert factor < 2.0 ** -24, (s, factor)
        for rows, per in batches(ens, X, Y):
            R = ens.kernel_rows(rows, s)
            want = restate_scores(R, restate_row_means(R), fit["colmean"], fit["tot"], fit["Vt"], fit["wt"])
            bound = score_bar(want, m) + w1 * (want["z"] ** 2).sum(axis=1) * factor
            err = np.abs(per[s].astype(np.float64) - want["score"])
            assert (err <= bound).all(), (s, len(rows), float((err / np.maximum(bound, 1e-300)).max()))
    print(f"m={m} n={n}: worst E (w_1 + 2 / gap) = 2^{np.log2(max(worst, 1e-300)):.1f}")


# ---- 6. exactness and identity ------------------------------------------------------------------------------------------------
def _published(ens, Y):
    got, per = ens.decision_function(Y, return_per_subspace=True)
    return dict(scores=ens.decision_scores_, per=ens.per_subspace_scores_, new=got, new_per=per, lam=np.stack(ens.eigenvalues_),
                V=np.stack(ens.components_), colmean=ens.column_mean_, tot=ens.total_mean_, gamma=ens.gamma_, q=ens.n_components_,
                usable=ens.n_usable_, sweeps=ens.n_sweeps_, converged=ens.converged_, rows=ens.landmark_rows_)


def _same(a, b):
    for name in a:
        np.testing.assert_array_equal(a[name], b[name], err_msg=name)


@pytest.mark.parametrize("m", [LDS_DIMS - 1, 130])
def test_results_do_not_depend_on_the_workspace_the_splits_the_run_or_the_company(m):
    import vgan_amd
    from vgan_amd.outlier import kpca_chunks, kpca_fit_chunks
    n = 257
    X, Y = case_data(m, n)

    def run(mask=MASK, proba=PROBA, **kw):
        ens = vgan_amd.SubspaceKPCA(mask, proba, n_components=3, max_samples=m, **kw).fit(X)
        return ens, _published(ens, Y)

    base_ens, base = run()
    got, per = base_ens.decision_function(X, return_per_subspace=True)
    np.testing.assert_array_equal(per, base["per"])  # nothing is excluded at fit
    np.testing.assert_array_equal(got, base["scores"])
    small = 64 * (m * 4 + 8 + 73 * 4) * 2 + 2 * m * 73 * 4  # bytes: about two 64-row pieces
    chunks = kpca_chunks(base_ens.plan, m, n, small)
    assert len(chunks) >= 2 and any(c[3] < n for c in chunks) and len(kpca_fit_chunks(base_ens.plan, m, small)) > 2
    for kw in ({}, dict(splits=1), dict(splits=3), dict(workspace_bytes=small), dict(workspace_bytes=1, splits=3)):
        _same(base, run(**kw)[1])
    _same(base, run(landmarks=base["rows"])[1])  # the drawn rows, given
    for s in (1, 3, 4):  # subspaces of either engine, fitted alone
        alone = run(mask=MASK[s:s + 1], proba=[1.0])[1]
        for name in ("per", "new_per", "lam", "V", "colmean", "tot", "gamma", "q", "usable", "sweeps"):
            np.testing.assert_array_equal(alone[name][0], base[name][s], err_msg=name)


def test_a_constant_subspace_scores_exactly_zero():
    import vgan_amd
    n = 65
    X, Y = case_data(65, n)
    X = X.copy()
    X[:, :40] = np.float32(2.7)
    mask = np.zeros((3, D), bool)
    mask[0, :3] = mask[1, :40] = mask[2, 38:45] = True  # constant on either engine, and a mixed one
    ens = vgan_amd.SubspaceKPCA(mask, [0.2, 0.3, 0.5], max_samples=33).fit(X)
    np.testing.assert_array_equal(ens.gamma_[:2], [1.0 / 3, 1.0 / 40])
    np.testing.assert_array_equal(ens.n_usable_[:2], [0, 0])
    assert ens.n_usable_[2] > 0 and (ens.per_subspace_scores_[2] > 0).any()
    np.testing.assert_array_equal(ens.total_mean_[:2], [1.0, 1.0])
    np.testing.assert_array_equal(ens.per_subspace_scores_[:2], np.zeros((2, n), np.float32))
    np.testing.assert_array_equal(ens.decision_function(X[:7], return_per_subspace=True)[1][:2], np.zeros((2, 7), np.float32))


# ---- 7. the shared tail -------------------------------------------------------------------------------------------------------
def test_normalize_max_and_predict_go_through_the_shared_tail():
    import vgan_amd
    from test_outlier_gmm_gpu import MASK as GMM_MASK, PROBA as GMM_PROBA
    rows = shifted_data(257 + 130, GMM_MASK.shape[1], seed=257, scale=True)
    X, Y = np.ascontiguousarray(rows[:257]), np.ascontiguousarray(rows[257:])
    ens = vgan_amd.SubspaceKPCA(GMM_MASK, GMM_PROBA, n_components=4, max_samples=65, normalize="robust", combination="max",
                                contamination=0.05).fit(X)
    per = ens.per_subspace_scores_
    c, w = _check_stats(ens, "robust")
    _check_scores(ens.decision_scores_, per, GMM_PROBA, c, w, "max")
    got, per_new = ens.decision_function(Y, return_per_subspace=True)
    _check_scores(got, per_new, GMM_PROBA, c, w, "max")
    assert ens.threshold_ == np.percentile(ens.decision_scores_, 95.0)
    np.testing.assert_array_equal(ens.labels_, (ens.decision_scores_ > ens.threshold_).astype(int))
    np.testing.assert_array_equal(ens.predict(Y), (got > ens.threshold_).astype(int))
    assert ens.predict_proba(Y).shape == (130, 2)
    plain = vgan_amd.SubspaceKPCA(GMM_MASK, GMM_PROBA, n_components=4, max_samples=65).fit(X)
    np.testing.assert_array_equal(plain.per_subspace_scores_, per)
    np.testing.assert_allclose(plain.decision_scores_, GMM_PROBA @ per.astype(np.float64), rtol=1e-12)


def test_vgan_outlier_ensemble_kpca_end_to_end():
    import vgan_amd
    from test_outlier_gpu import _planted
    X = _planted()[:, :10]
    model = vgan_amd.VGAN_no_kl(epochs=5)
    model.fit(X)
    X = np.ascontiguousarray(X[-600:])
    ens = model.outlier_ensemble(method="kpca", n_components=8, subspace_count=200, X=X)
    assert type(ens) is vgan_amd.SubspaceKPCA and ens._fitted
    assert ens.decision_scores_.shape == (600,) and np.isfinite(ens.decision_scores_).all()
    assert ens.column_mean_.shape == (model.subspaces.shape[0], 256) and ens.converged_.all()
    np.testing.assert_array_equal(ens.decision_function(X), ens.decision_scores_)


# ---- 8. the ring: outliers that sit inside the data ---------------------------------------------------------------------------
@pytest.mark.parametrize("seed", range(5))
def test_kpca_finds_the_centre_of_the_ring_on_the_device(seed):
    import vgan_amd
    from sklearn.metrics import roc_auc_score
    X, y = ring(seed)
    ens = vgan_amd.SubspaceKPCA(np.ones((1, X.shape[1]), bool), [1.0], n_components=RING_COMPONENTS, gamma=ring_gamma(X)).fit(X)
    np.testing.assert_array_equal(ens.landmark_rows_, restate_landmarks(len(X)))
    auc = roc_auc_score(y, ens.decision_scores_)
    print(f"seed {seed}: KPCA AUC on the device {auc:.3f}, {ens.n_sweeps_[0]} sweeps, {ens.n_usable_[0]} usable components")
    assert auc >= 0.99
