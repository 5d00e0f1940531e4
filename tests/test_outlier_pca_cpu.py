"""PCA scores over the subspaces, CPU tier: the float64 numpy restatement the GPU tests compare against, pinned to sklearn
(StandardScaler + PCA) and to the Mahalanobis restatement; a restatement of the Jacobi order that csrc/outlier_pca.hip
builds, from which the constants of the GPU test's decomposition bars are taken; and everything of vgan_amd.SubspacePCA
that runs without a device (argument checks, the component count and weight rules, the dispatch from the model, the C ABI's
argument checks).

The definition (SubspacePCA's docstring): X as float32, arithmetic in float64.  mu = mean, C = (1 / n) sum (x - mu)(x - mu)^T,
scale = sqrt(diag C) with 0 -> 1 (standardize) or 1, M = C / (scale scale^T) = V^T Lambda V with the eigenvalues descending
(ties by the ascending diagonal position) and every row of V signed so that its entry of largest magnitude (lowest index
on a tie) is positive; q from n_components (None, int, or sklearn's cumulative-ratio rule for a float); J = all / the first
q / those after the first q; score = sum_{j in J} w_j y_j^2, y = V ((x - mu) / scale), w = 1 or 1 / ((1 - a) max(lambda, 0) + a tr /
d), rounded to float32.  tr M == 0 or an empty J: every score 0.

The Jacobi order (restate_jacobi; the header's vgan_pca_eigen text): rounds of a round-robin tournament, the rotations
of a round from the matrix as the previous round left it, M <- J^T M J per 2 x 2 block as R_I^T (B R_J).  Observed on the GPU
test's inputs (edge_mask below, raw_data(n, 140, seed=n) with the constant and the duplicated column, n = 2, 65, 257, 2051,
standardised and not), with u = 2^-53, by test_jacobi_restatement_sets_the_constants_of_the_gpu_bars:

    max |V^T Lambda V - M| / (d_s u ||M||_2)     = 1.58   (bar of the GPU test: 16, the issue's constant, since 1.58 <= 2.5)
    max |lambda - eigvalsh(M)| / (d_s u ||M||_2) = 0.56   (bar: 16)
    max |V V^T - I| / (d_s u)                    = 3.51   (above 2.5, so the bar is 8 x 3.51 = 28.1 rounded up to a power of
                                                          two: 32)
    sweeps: at most 17 (n = 65), every subspace converged

The constants are the restatement's, never the device's."""
import ctypes
import os
import re

import numpy as np
import pytest

from conftest import REPO
from test_outlier_ecod_cpu import _mask
from test_outlier_maha_cpu import raw_data, restate_moments
from test_outlier_maha_cpu import restate_fit as restate_maha_fit

U = 2.0 ** -53
TOL_PIN = 1e-12  # pins the formula to sklearn; not a kernel tolerance
LDS_DIMS = 48  # VGAN_PCA_LDS_DIMS

# ---- the inputs of the GPU test (shared, so that the constants above are taken on them) ------------------------------------
D = 140
SIZES = [1, 2, 3, 15, 16, 17, 33, LDS_DIMS, LDS_DIMS + 1, 65, 130]
CONST, DUP = 5, (7, 11)  # a constant column; column 11 repeats column 7
ROWS = [2, 65, 257, 2 * 1024 + 3]
K_RESIDUAL, K_EIGENVALUE, K_ORTHOGONAL = 16, 16, 32  # the docstring says where each comes from
MEASURED = dict(residual=1.58, eigenvalue=0.56, orthogonal=3.51)  # what the docstring records, rounded up


def edge_mask():
    """bool [11, 140]: the subspace of one feature is the constant column, the one of two adds the duplicated feature's
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


def edge_data(n):
    return raw_data(n, D, seed=n, constant=CONST, duplicate=DUP)


# ---- the restatement --------------------------------------------------------------------------------------------------
def restate_matrix(Z, standardize=True):
    """(mu [d], scale [d], M [d, d]) of the rows of Z (float32 values)."""
    mu, C, _ = restate_moments(Z)
    scale = np.ones(C.shape[0])
    if standardize:
        scale = np.sqrt(np.diag(C))
        scale[scale == 0] = 1.0
    return mu, scale, C / (scale[:, None] * scale[None, :])


def order_and_sign(lam, Vt):
    """Eigenvalues descending (ties by the ascending position), rows of Vt signed by their entry of largest magnitude."""
    order = np.lexsort((np.arange(lam.shape[0]), -lam))
    lam, Vt = lam[order], Vt[order].copy()
    at = np.argmax(np.abs(Vt), axis=1)  # the first of equal magnitudes
    Vt[Vt[np.arange(len(at)), at] < 0] *= -1.0
    return lam, Vt


def restate_eigh(M):
    w, Q = np.linalg.eigh(M)
    return order_and_sign(w[::-1].copy(), Q[:, ::-1].T.copy())


def sign_rule_holds(Vt):
    at = np.argmax(np.abs(Vt), axis=1)
    return bool((Vt[np.arange(len(at)), at] > 0).all())


def variance_ratio(lam):
    clipped = np.maximum(lam, 0.0)
    return clipped / clipped.sum() if clipped.sum() > 0 else np.zeros_like(lam)


def component_count(lam, n_components):
    d = lam.shape[0]
    if n_components is None:
        return d
    if isinstance(n_components, (int, np.integer)):
        return min(int(n_components), d)
    return min(int(np.searchsorted(np.cumsum(variance_ratio(lam)), n_components, side="right")) + 1, d)


def restate_weights(lam, q, components="all", weighted=True, shrinkage=0.1):
    d = lam.shape[0]
    chosen = {"all": np.ones(d, bool), "major": np.arange(d) < q, "minor": np.arange(d) >= q}[components]
    tr = lam.sum()
    if tr == 0 or not chosen.any():
        return np.zeros(d)
    if not weighted:
        return chosen.astype(np.float64)
    if shrinkage == 0 and (lam[chosen] <= 16 * d * U * lam[0]).any():
        raise ValueError("a selected eigenvalue is numerically zero")
    w = np.zeros(d)
    w[chosen] = 1.0 / ((1.0 - shrinkage) * np.maximum(lam, 0.0) + shrinkage * tr / d)[chosen]
    return w


def restate_scores(Z, mu, scale, Vt, wt):
    """(float64 [n] scores, float64 [n] the summation term sum_j w_j |y_j| sum_k |v_jk z_k| of the GPU test's bar)."""
    Zs = (np.asarray(Z, dtype=np.float32).astype(np.float64) - mu) * (1.0 / scale)
    Y = Zs @ Vt.T
    return (wt * Y * Y).sum(axis=1), (wt * np.abs(Y) * (np.abs(Zs) @ np.abs(Vt).T)).sum(axis=1)


def restate_fit(Z, n_components=None, components="all", weighted=True, standardize=True, shrinkage=0.1):
    """The whole contract for one subspace Z [n, d_s] with numpy.linalg.eigh as the solver."""
    mu, scale, M = restate_matrix(Z, standardize)
    lam, Vt = restate_eigh(M)
    q = component_count(lam, n_components)
    wt = restate_weights(lam, q, components, weighted, shrinkage)
    scores, _ = restate_scores(Z, mu, scale, Vt, wt)
    return dict(mu=mu, scale=scale, M=M, lam=lam, Vt=Vt, q=q, wt=wt, scores=scores)


# ---- the Jacobi order of csrc/outlier_pca.hip, restated -----------------------------------------------------------------
def round_pairs(d, r):
    """(a, b) int [n / 2]: the pairs of round r among n = d rounded up to even players; a player >= d is the bye."""
    n = d + (d & 1)
    pos = np.arange(n // 2)

    def player(p):
        return np.where(p == 0, n - 1, (p - 1 + r) % (n - 1))
    return player(pos), player(n - 1 - pos)


def folded_blocks(npairs):
    """[(I, J)]: the kernel's enumeration of the blocks I <= J, the triangle folded into ceil(np / 2) x (np + 1) items."""
    half, wid, out = (npairs + 1) // 2, npairs + 1, []
    for e in range(half * wid):
        fa, fb = divmod(e, wid)
        if fb < npairs - fa:
            out.append((fa, fa + fb))
        else:
            i = npairs - 1 - fa
            if i != fa:
                out.append((i, i + fb - (npairs - fa)))
    return out


def restate_jacobi(M, max_sweeps=30):
    """(lam, Vt, sweeps, converged) ordered and signed: every rotation of a round from the matrix as the previous round left
    it; the blocks I < J as R_I^T (B R_J), mirrored; the block I = I set to diag(m_aa - t m_ab, m_bb + t m_ab).  The bye is a
    zero row and column with an identity rotation, which the padding makes literal."""
    d = M.shape[0]
    n = d + (d & 1)
    A = np.zeros((n, n))
    A[:d, :d] = M
    Vt = np.eye(n)
    sweeps, converged = 0, False
    while sweeps < max_sweeps and not converged:
        rotated = False
        for r in range(n - 1):
            a, b = round_pairs(d, r)
            app, aqq, apq = A[a, a], A[b, b], A[a, b]
            rot = (np.abs(apq) > U * np.sqrt(np.abs(app * aqq))) & (a < d) & (b < d)
            if not rot.any():
                continue
            rotated = True
            with np.errstate(over="ignore", divide="ignore", invalid="ignore"):
                zeta = (aqq - app) / (2.0 * apq)
                t = np.where(rot, np.copysign(1.0, zeta) / (np.abs(zeta) + np.sqrt(1.0 + zeta * zeta)), 0.0)
            c = 1.0 / np.sqrt(1.0 + t * t)
            s = c * t
            x11, x12, x21, x22 = A[np.ix_(a, a)], A[np.ix_(a, b)], A[np.ix_(b, a)], A[np.ix_(b, b)]
            c2, s2, c1, s1 = c[None, :], s[None, :], c[:, None], s[:, None]
            y11, y12, y21, y22 = c2 * x11 - s2 * x12, s2 * x11 + c2 * x12, c2 * x21 - s2 * x22, s2 * x21 + c2 * x22
            z11, z12, z21, z22 = c1 * y11 - s1 * y21, c1 * y12 - s1 * y22, s1 * y11 + c1 * y21, s1 * y12 + c1 * y22
            upper = np.triu(np.ones((len(a), len(a)), bool), 1)  # I < J; the mirror image is written with it
            for rows, cols, z in ((a, a, z11), (a, b, z12), (b, a, z21), (b, b, z22)):
                ri, ci = np.broadcast_to(rows[:, None], upper.shape)[upper], np.broadcast_to(cols[None, :], upper.shape)[upper]
                A[ri, ci] = z[upper]
                A[ci, ri] = z[upper]
            ar, br = a[rot], b[rot]
            A[ar, ar], A[br, br] = app[rot] - t[rot] * apq[rot], aqq[rot] + t[rot] * apq[rot]
            A[ar, br] = A[br, ar] = 0.0
            va, vb = Vt[ar].copy(), Vt[br].copy()
            Vt[ar] = c[rot][:, None] * va - s[rot][:, None] * vb
            Vt[br] = s[rot][:, None] * va + c[rot][:, None] * vb
        sweeps += 1
        converged = not rotated
    lam, Vt = order_and_sign(np.diag(A)[:d].copy(), Vt[:d, :d])
    return lam, Vt, sweeps, converged


def decomposition_errors(M, lam, Vt):
    """(residual, eigenvalue, orthogonality) errors in units of d u ||M||_2, d u ||M||_2 and d u."""
    d = M.shape[0]
    norm = np.linalg.norm(M, 2)
    orth = np.abs(Vt @ Vt.T - np.eye(d)).max() / (d * U)
    if norm == 0:
        return float(np.abs(Vt.T @ (lam[:, None] * Vt) - M).max()), float(np.abs(lam).max()), orth
    res = np.abs(Vt.T @ (lam[:, None] * Vt) - M).max() / (d * U * norm)
    ev = np.abs(lam - np.linalg.eigvalsh(M)[::-1]).max() / (d * U * norm)
    return res, ev, orth


def test_the_folded_enumeration_takes_every_block_once():
    for npairs in (1, 2, 3, 4, 7, 8, 24, 25, 65, 512):
        got = folded_blocks(npairs)
        assert len(got) == npairs * (npairs + 1) // 2 == len(set(got))
        assert all(0 <= i <= j < npairs for i, j in got)


def test_a_sweep_meets_every_pair_once():
    for d in (1, 2, 3, 16, 17, 49):
        n = d + (d & 1)
        seen = set()
        for r in range(n - 1):
            a, b = round_pairs(d, r)
            assert sorted(np.concatenate([a, b])) == list(range(n))  # disjoint: a round parallelises
            seen |= {(min(x, y), max(x, y)) for x, y in zip(a, b)}
        assert len(seen) == n * (n - 1) // 2
        if d > 2:
            a, b = round_pairs(d, 3)
            assert (np.diff(a[1:]) % (n - 1) == 1).all() and (np.diff(b[1:]) % (n - 1) == n - 2).all()  # neighbours in memory


@pytest.mark.parametrize("n", ROWS)
def test_jacobi_restatement_sets_the_constants_of_the_gpu_bars(n):
    X, mask = edge_data(n), edge_mask()
    worst = np.zeros(3)
    most = 0
    for standardize in (True, False):
        for s in range(len(SIZES)):
            _, _, M = restate_matrix(X[:, mask[s]], standardize)
            lam, Vt, sweeps, converged = restate_jacobi(M)
            assert converged and 1 <= sweeps <= 30
            assert (np.diff(lam) <= 0).all() and sign_rule_holds(Vt)
            worst = np.maximum(worst, decomposition_errors(M, lam, Vt))
            most = max(most, sweeps)
    print(f"n={n}: residual {worst[0]:.3f} eigenvalue {worst[1]:.3f} orthogonality {worst[2]:.3f} sweeps <= {most}")
    assert worst[0] <= MEASURED["residual"] <= 2.5 and K_RESIDUAL == 16
    assert worst[1] <= MEASURED["eigenvalue"] <= 2.5 and K_EIGENVALUE == 16
    assert worst[2] <= MEASURED["orthogonal"] and K_ORTHOGONAL == 2 ** int(np.ceil(np.log2(8 * MEASURED["orthogonal"])))


def test_jacobi_restatement_agrees_with_eigh_and_honours_max_sweeps():
    X = edge_data(257)
    Z = X[:, edge_mask()[5]]
    for standardize in (True, False):
        _, _, M = restate_matrix(Z, standardize)
        lam, Vt, _, _ = restate_jacobi(M)
        want_lam, want_Vt = restate_eigh(M)
        np.testing.assert_allclose(lam, want_lam, rtol=0, atol=1e-13 * want_lam[0])
        np.testing.assert_allclose(Vt[:4], want_Vt[:4], rtol=0, atol=1e-10)  # separated eigenvalues
    _, Vt, sweeps, converged = restate_jacobi(M, max_sweeps=1)
    assert sweeps == 1 and not converged and np.isfinite(Vt).all()


# ---- pinned to sklearn ---------------------------------------------------------------------------------------------------
PIN_SHAPES = [(300, 13), (1000, 67), (200, 130)]  # the last has n < d_s


def pin_data(n, d):
    return raw_data(n, d, seed=n + d, constant=5, duplicate=(7, 11))


@pytest.mark.parametrize("n,d", PIN_SHAPES)
def test_spectrum_and_components_are_sklearns(n, d):
    from sklearn.decomposition import PCA
    from sklearn.preprocessing import StandardScaler
    Z = pin_data(n, d)
    sk = PCA().fit(StandardScaler().fit_transform(Z.astype(np.float64)))
    got = restate_fit(Z)
    k = min(n, d)
    scale = got["lam"][0]
    np.testing.assert_allclose(got["lam"][:k], sk.explained_variance_ * (n - 1) / n, rtol=0, atol=TOL_PIN * scale)
    assert (np.abs(got["lam"][k:]) <= TOL_PIN * scale).all()
    np.testing.assert_allclose(variance_ratio(got["lam"])[:k], sk.explained_variance_ratio_, rtol=0, atol=TOL_PIN)
    lam = got["lam"]
    gap = np.minimum(np.abs(np.diff(lam, prepend=np.inf)), np.abs(np.diff(lam, append=-np.inf))) / lam[0]
    separated = np.flatnonzero(gap[:k] > 2.0 ** -20)
    assert separated.size >= k // 2
    for j in separated:
        v, w = got["Vt"][j], sk.components_[j]
        np.testing.assert_allclose(v, w if v @ w > 0 else -w, rtol=0, atol=64 * d * U / gap[j])  # the perturbation bound of a vector
    assert sign_rule_holds(got["Vt"]) and (np.diff(lam) <= 0).all()
    sd = Z.astype(np.float64).std(axis=0)
    np.testing.assert_allclose(got["scale"], np.where(sd == 0, 1.0, sd), rtol=TOL_PIN)


@pytest.mark.parametrize("n,d", PIN_SHAPES)
@pytest.mark.parametrize("f", [0.5, 0.9, 0.99])
def test_fractional_component_count_is_sklearns(n, d, f):
    from sklearn.decomposition import PCA
    from sklearn.preprocessing import StandardScaler
    from vgan_amd.outlier import pca_component_count
    Z = pin_data(n, d)
    sk = PCA(n_components=f, svd_solver="full").fit(StandardScaler().fit_transform(Z.astype(np.float64)))
    lam = restate_fit(Z)["lam"]
    cum = np.cumsum(variance_ratio(lam))
    assert np.abs(cum - f).min() > 1e-9  # the count does not hinge on the last bits
    assert component_count(lam, f) == sk.n_components_ == pca_component_count(lam, f)


@pytest.mark.parametrize("n,d", PIN_SHAPES)
@pytest.mark.parametrize("alpha", [0.1, 0.5])
def test_all_weighted_unstandardised_is_the_mahalanobis_score(n, d, alpha):
    Z = pin_data(n, d)
    got = restate_fit(Z, standardize=False, shrinkage=alpha)["scores"]
    want = restate_maha_fit(Z, shrinkage=alpha)
    kappa = np.linalg.cond(want["est"]["Sigma"])
    np.testing.assert_allclose(got.astype(np.float32), want["scores"], rtol=2.0 ** -23)
    from test_outlier_maha_cpu import restate_distances
    np.testing.assert_allclose(got, restate_distances(Z, want["est"]), rtol=64 * d * kappa * U)


def test_component_sets_weights_and_special_cases():
    from vgan_amd.outlier import pca_component_count, pca_variance_ratio, pca_weights
    lam = np.array([4.0, 2.0, 1.0, 1.0, 0.0])
    assert [pca_component_count(lam, q) for q in (None, 1, 5, 9)] == [5, 1, 5, 5]
    assert [pca_component_count(lam, f) for f in (0.4, 0.5, 0.75, 0.99)] == [1, 2, 3, 4]  # cumsum 0.5, 0.75, 0.875, 1, 1
    np.testing.assert_array_equal(pca_variance_ratio(np.array([3.0, 1.0, -1e-17])), [0.75, 0.25, 0.0])
    np.testing.assert_array_equal(pca_variance_ratio(np.zeros(3)), np.zeros(3))
    assert pca_component_count(np.zeros(3), 0.5) == 3
    for components, q, chosen in (("all", 5, [1, 1, 1, 1, 1]), ("major", 2, [1, 1, 0, 0, 0]), ("minor", 2, [0, 0, 1, 1, 1]),
                                  ("minor", 5, [0, 0, 0, 0, 0]), ("major", 5, [1, 1, 1, 1, 1])):
        w, bad = pca_weights(lam, q, components, False, 0.1)
        np.testing.assert_array_equal(w, chosen)
        assert not bad
        w, bad = pca_weights(lam, q, components, True, 0.25)
        np.testing.assert_allclose(w, np.array(chosen) / (0.75 * lam + 0.25 * 8.0 / 5), rtol=1e-15)
        np.testing.assert_array_equal(w, restate_weights(lam, q, components, True, 0.25))
    w, bad = pca_weights(lam, 2, "major", True, 0.0)
    np.testing.assert_array_equal(w, [0.25, 0.5, 0, 0, 0])
    assert not bad
    assert pca_weights(lam, 2, "minor", True, 0.0)[1] and pca_weights(lam, 5, "all", True, 0.0)[1]  # lambda_5 = 0 is selected
    tiny = np.array([1.0, 16 * 2 * U])
    assert pca_weights(tiny, 2, "all", True, 0.0)[1] and not pca_weights(tiny * [1, 1.01], 2, "all", True, 0.0)[1]
    w, bad = pca_weights(np.zeros(4), 4, "all", True, 0.0)  # tr M == 0 comes first: all scores 0
    assert not bad and (w == 0).all()
    # a row of a duplicated pair and a constant: M = [[0, 0, 0], [0, 1, 1], [0, 1, 1]]
    Z = np.array([[3, 1, 1], [3, 2, 2], [3, 4, 4], [3, 5, 5]], dtype=np.float32)
    got = restate_fit(Z, components="minor", n_components=1, weighted=False)
    np.testing.assert_allclose(got["lam"], [2, 0, 0], atol=1e-15)
    np.testing.assert_allclose(got["Vt"][0], [0, np.sqrt(0.5), np.sqrt(0.5)], atol=1e-15)
    np.testing.assert_allclose(got["scores"], 0, atol=1e-28)  # every row lies on the one direction
    assert (restate_fit(np.full((5, 3), 7, np.float32))["scores"] == 0).all()


def planted_plane(seed=6):
    """(X float32 [300, 20], outlier bool [300]): rows on a 3-dimensional plane plus 1e-3 noise; the first ten are moved
    0.05 along a direction orthogonal to the plane, their position inside the plane left as drawn."""
    rng = np.random.default_rng(seed)
    Q, _ = np.linalg.qr(rng.normal(size=(20, 4)))
    X = 100.0 + rng.normal(size=(300, 3)) @ Q[:, :3].T + 1e-3 * rng.normal(size=(300, 20))
    out = np.zeros(300, dtype=bool)
    out[:10] = True
    X[out] += 0.05 * Q[:, 3]
    return X.astype(np.float32), out


def planted_ranks(scores, outlier):
    """The ranks (0 = the highest score) of the planted rows."""
    return np.argsort(np.argsort(-scores, kind="stable"), kind="stable")[outlier]


def test_minor_components_find_the_rows_off_the_plane_and_major_ones_do_not():
    X, out = planted_plane()
    minor = restate_fit(X, components="minor", n_components=3, weighted=False)["scores"]
    major = restate_fit(X, components="major", n_components=3)["scores"]
    assert planted_ranks(minor, out).max() < 10
    assert planted_ranks(major, out).mean() > 30


# ---- the constructor and the host rules, without a device -------------------------------------------------------------------
def test_constructor_validates_without_touching_the_device():
    import vgan_amd
    from vgan_amd import outlier
    m = _mask(4, [[0, 1], [1, 2, 3]])
    ens = vgan_amd.SubspacePCA(m, [0.5, 0.5])
    assert (ens.n_components, ens.components, ens.weighted, ens.standardize, ens.shrinkage, ens.max_sweeps, ens.normalize,
            ens.combination, ens.contamination) == (None, "all", True, True, 0.1, 30, None, "sum", 0.1)
    assert isinstance(ens, outlier._SubspaceScorer)
    for bad in (0, -1, 1.0, 1.5, 0.0, float("nan"), "mle", True):
        with pytest.raises(ValueError, match="n_components"):
            vgan_amd.SubspacePCA(m, [0.5, 0.5], n_components=bad, components="major")
    for bad in ("some", None, 1):
        with pytest.raises(ValueError, match="components must be"):
            vgan_amd.SubspacePCA(m, [0.5, 0.5], components=bad)
    for q in (1, 0.9):
        with pytest.raises(ValueError, match="components='all'.*n_components must be None"):
            vgan_amd.SubspacePCA(m, [0.5, 0.5], n_components=q)
    for name in ("weighted", "standardize"):
        for bad in (1, 0, None, "yes"):
            with pytest.raises(ValueError, match=name):
                vgan_amd.SubspacePCA(m, [0.5, 0.5], **{name: bad})
    for bad in (-0.1, 1.5, "oas", None, float("nan"), True):
        with pytest.raises(ValueError, match="shrinkage"):
            vgan_amd.SubspacePCA(m, [0.5, 0.5], shrinkage=bad)
    for bad in (0, -1, 2.0, None, True):
        with pytest.raises(ValueError, match="max_sweeps"):
            vgan_amd.SubspacePCA(m, [0.5, 0.5], max_sweeps=bad)
    ok = vgan_amd.SubspacePCA(m, [0.5, 0.5], n_components=0.9, components="minor", weighted=False, standardize=False, shrinkage=0,
                              max_sweeps=1)
    assert (ok.n_components, ok.components, ok.weighted, ok.standardize, ok.shrinkage, ok.max_sweeps) == (0.9, "minor", False, False, 0.0, 1)
    assert outlier.check_pca_params(np.int64(3), "major", np.True_, False, 1, np.int32(7)) == (3, "major", True, False, 1.0, 7)
    with pytest.raises(ValueError, match="proba has 3 entries for 2 subspaces"):
        vgan_amd.SubspacePCA(m, [0.5, 0.25, 0.25])
    with pytest.raises(ValueError, match="normalize"):
        vgan_amd.SubspacePCA(m, [0.5, 0.5], normalize="l2")
    with pytest.raises(ValueError, match="combination"):
        vgan_amd.SubspacePCA(m, [0.5, 0.5], combination="mean")
    with pytest.raises(ValueError, match="contamination"):
        vgan_amd.SubspacePCA(m, [0.5, 0.5], contamination=0.7)
    with pytest.raises(ValueError, match="at most 1024"):
        vgan_amd.SubspacePCA(np.ones((1, outlier.MAHA_MAX_DIMS + 1), bool), [1.0])
    vgan_amd.SubspacePCA(np.ones((1, outlier.MAHA_MAX_DIMS), bool), [1.0])
    with pytest.raises(ValueError, match="between 2 and"):
        ens.fit(np.zeros((1, 4), np.float32))
    with pytest.raises(ValueError, match="features"):
        ens.fit(np.zeros((5, 3), np.float32))
    assert ens.ops is None  # none of this touched the device
    with pytest.raises(RuntimeError, match="not fitted"):
        ens.components_
    with pytest.raises(RuntimeError, match="not fitted"):
        ens.decision_function(np.zeros((5, 4), np.float32))
    doc = vgan_amd.SubspacePCA.__doc__
    for word in ("as remembered, not pinned against", "randomized", "whiten", "cdist", "incremental", "ShrunkCovariance", "searchsorted",
                 "max_sweeps", "16 d_s 2^-53"):
        assert word in doc, word


def test_outlier_ensemble_routes_pca_to_the_new_class():
    import vgan_amd
    model = vgan_amd.VGAN_no_kl(epochs=1)
    model.subspaces = _mask(6, [[0, 1], [2, 3, 5], [4]])
    model.proba = np.array([0.5, 0.3, 0.2])
    ens = model.outlier_ensemble(method="pca")
    assert type(ens) is vgan_amd.SubspacePCA and ens.components == "all" and ens.plan.count == 3
    np.testing.assert_array_equal(ens.proba, model.proba)
    ens = model.outlier_ensemble(method="pca", n_neighbors=17, components="minor", n_components=2, weighted=False, standardize=False,
                                 shrinkage=0.3, max_sweeps=9, normalize="zscore", combination="max", contamination=0.05,
                                 workspace_bytes=1 << 20)  # n_neighbors is ignored
    assert (ens.components, ens.n_components, ens.weighted, ens.standardize, ens.shrinkage, ens.max_sweeps, ens.normalize, ens.combination,
            ens.contamination, ens.workspace_bytes) == ("minor", 2, False, False, 0.3, 9, "zscore", "max", 0.05, 1 << 20)
    with pytest.raises(TypeError):
        model.outlier_ensemble(method="pca", engine="exact")  # not a keyword of SubspacePCA
    assert '"pca"' in vgan_amd.VGAN_no_kl.outlier_ensemble.__doc__ and "SubspacePCA" in vgan_amd.__all__
    with pytest.raises(ValueError, match="method"):  # the neighbour ensemble does not know it
        vgan_amd.SubspaceEnsemble(model.subspaces, model.proba, method="pca")


# ---- C ABI: argument checks without a GPU -----------------------------------------------------------------------------------
def test_pca_entries_reject_bad_arguments_without_gpu():
    import vgan_amd
    from vgan_amd import outlier
    lib = vgan_amd.lib.load()
    header = open(os.path.join(REPO, "include", "vgan_hip.h")).read()
    assert int(re.search(r"#define VGAN_PCA_LDS_DIMS (\d+)", header).group(1)) == outlier.PCA_LDS_DIMS == LDS_DIMS
    null = None
    buf = ctypes.create_string_buffer(256)
    p = ctypes.cast(ctypes.addressof(buf) + (-ctypes.addressof(buf)) % 16, ctypes.c_void_p)  # never read

    def rejected(rc):
        msg = lib.vgan_last_error()
        return rc == 1 and b"bad argument" in msg and b"outlier_pca.hip" in msg

    def each(fn, good, pointers, bad_values):
        for pos in pointers:
            assert rejected(fn(*[null if i == pos else v for i, v in enumerate(good)])), pos
        for pos, bad in bad_values:
            assert rejected(fn(*[bad if i == pos else v for i, v in enumerate(good)])), (pos, bad)

    big = outlier.MAHA_MAX_DIMS + 1
    # cov, sq_off, feat_off, first, count, max_dims, standardize, max_sweeps, scale, evals, V, sweeps, status, stream
    each(lib.vgan_pca_eigen, [p, p, p, 0, 2, 3, 1, 30, p, p, p, p, p, null], (0, 1, 2, 8, 9, 10, 11, 12),
         [(3, -1), (4, 0), (4, 65536), (5, 0), (5, big), (6, 2), (6, -1), (7, 0)])
    # Xq, ldq, rows, d, feat, feat_off, sq_off, first, count, max_dims, mean, inv_scale, V, wt, score, ld_score, stream
    each(lib.vgan_pca_scores, [p, 4, 10, 4, p, p, p, 0, 2, 3, p, p, p, p, p, 10, null], (0, 4, 5, 6, 10, 11, 12, 13, 14),
         [(1, 3), (2, 0), (2, (1 << 24) + 1), (3, 0), (7, -1), (8, 0), (8, 65536), (9, 0), (9, big), (15, 9)])
    for name, nargs in (("vgan_pca_eigen", 14), ("vgan_pca_scores", 17)):
        assert len(vgan_amd.lib.SIGNATURES[name][1]) == nargs
    assert vgan_amd.lib.ABI_VERSION == lib.vgan_abi_version() == 11  # symbols were only added
