"""iNNE over the subspaces, CPU tier: the float64 numpy restatement the GPU tests compare against, pinned to a case worked
by hand, to a second restatement written as the scalar loops of the definition, to sklearn's NearestNeighbors where there
are no ties and to the structural rules of the definition; and everything of vgan_amd.SubspaceINNE that runs without a
device (defaults, argument checks, the export, the dispatch from the model, the C ABI's argument checks).

The definition (SubspaceINNE's docstring): X as float32.  Estimator (s, t) has the stream id = s T + t and the centres c_j =
row feistel_perm(j, n, seed, id), j < psi, in that order.  d2 runs over the features in ascending order in float64, per
feature diff = a - b, p = diff * diff, acc = acc + p, each rounded on its own.  nn_j is the position i != j with the smallest
(d2(c_j, c_i), i), r2_j that d2.  rho_j = 1 - (r2[nn_j] + eps) / (r2_j + eps), eps = 2^-52 ("squared"), or the same on the
square roots ("distance").  A row takes from an estimator rho_j of the centre with the smallest (r2_j, j) among those with
d2(x, c_j) <= r2_j, 1.0 where there is none; score = float32(sum_t iso_t / T), the sum in float64 with t ascending."""
import ctypes
import inspect
import os
import re

import numpy as np
import pytest

from conftest import REPO
from small_ops_ref import feistel_perm_ref
from test_outlier_ecod_cpu import _mask, tied_data
from test_outlier_gpu import _planted

EPS = 2.0 ** -52


# ---- the restatement --------------------------------------------------------------------------------------------------
def restate_d2(A, B):
    """float64 [..., a, b]: d2 of the rows of A [..., a, ds] to the rows of B [..., b, ds] (float32 values), vectorised over
    the pairs, with a Python loop over the features so that the sum is sequential: three numpy operations per feature, each
    rounded on its own (numpy fuses nothing; add.reduce is pairwise and is not used)."""
    A, B = np.asarray(A, dtype=np.float64), np.asarray(B, dtype=np.float64)
    acc = np.zeros(A.shape[:-1] + (B.shape[-2],))
    diff = np.empty_like(acc)
    for f in range(A.shape[-1]):
        np.subtract(A[..., :, None, f], B[..., None, :, f], out=diff)
        np.multiply(diff, diff, out=diff)
        np.add(acc, diff, out=acc)
    return acc


def restate_centres(n, psi, seed, stream):
    """int64 [psi]: the centre rows of the estimator with that stream id, in draw order."""
    return feistel_perm_ref(np.arange(psi), n, seed, stream)


def restate_spheres(C, ratio="squared"):
    """(r2 float64 [..., psi], nn int32 [..., psi], rho float64 [..., psi]) of the centres C [..., psi, ds]."""
    D = restate_d2(C, C)
    psi = D.shape[-1]
    D[..., np.arange(psi), np.arange(psi)] = np.inf  # i != j
    nn = np.argmin(D, axis=-1)  # the first minimum: the lowest position among equal d2
    r2 = np.take_along_axis(D, nn[..., None], axis=-1)[..., 0]
    theirs = np.take_along_axis(r2, nn, axis=-1)
    if ratio == "distance":
        rho = 1.0 - (np.sqrt(theirs) + EPS) / (np.sqrt(r2) + EPS)
    else:
        assert ratio == "squared"
        rho = 1.0 - (theirs + EPS) / (r2 + EPS)
    return r2, nn.astype(np.int32), rho


def restate_cover(Q, C, r2):
    """(covered bool [nq], position int64 [nq]): whether a sphere covers each row of Q [nq, ds], and the covering centre with
    the smallest (r2, position)."""
    covered = restate_d2(Q, C) <= r2[None, :]
    at = np.argmin(np.where(covered, r2[None, :], np.inf), axis=1)  # the first minimum: the lowest position among equal r2
    return covered.any(axis=1), at


def restate_inne_build(X, feats_list, T, psi, seed, ratio="squared"):
    """(rows int32, r2 float64, nn int32, rho float64), each [S, T, psi]."""
    X = np.asarray(X, dtype=np.float32)
    n = X.shape[0]
    rows = np.stack([np.stack([restate_centres(n, psi, seed, s * T + t) for t in range(T)]) for s in range(len(feats_list))])
    out = [restate_spheres(X[rows[s]][:, :, feats], ratio) for s, feats in enumerate(feats_list)]
    return (rows.astype(np.int32),) + tuple(np.stack([o[k] for o in out]) for k in range(3))


def restate_inne_scores(X, Xq, feats_list, state):
    """float64 [S, nq]: sum_t iso_t / T before the rounding to float32; state: what restate_inne_build returned for X."""
    X, Xq = np.asarray(X, dtype=np.float32), np.asarray(Xq, dtype=np.float32)
    rows, r2, _, rho = state
    T = rows.shape[1]
    out = np.empty((len(feats_list), Xq.shape[0]))
    for s, feats in enumerate(feats_list):
        Q = Xq[:, feats]
        total = np.zeros(Xq.shape[0])
        for t in range(T):
            covered, at = restate_cover(Q, X[rows[s, t]][:, feats], r2[s, t])
            total = total + np.where(covered, rho[s, t][at], 1.0)
        out[s] = total / float(T)
    return out


def restate_inne(X, Xq, feats_list, T, max_samples, seed, ratio="squared"):
    psi = min(8 if max_samples == "auto" else max_samples, np.asarray(X).shape[0])
    state = restate_inne_build(X, feats_list, T, psi, seed, ratio)
    return restate_inne_scores(X, Xq, feats_list, state), state


def restate_inne_both(X, Xq_list, feats_list, T, max_samples, seed):
    """{ratio: ([scores float64 [S, nq] for every matrix of Xq_list], state)} for both ratios from one sweep over the pairs:
    centres, r2, nn and which sphere a row takes do not depend on the ratio, only rho does."""
    X = np.asarray(X, dtype=np.float32)
    psi = min(8 if max_samples == "auto" else max_samples, X.shape[0])
    states = {"squared": restate_inne_build(X, feats_list, T, psi, seed, "squared")}
    rows, r2, nn, _ = states["squared"]
    theirs = np.take_along_axis(r2, nn.astype(np.int64), axis=-1)
    states["distance"] = (rows, r2, nn, 1.0 - (np.sqrt(theirs) + EPS) / (np.sqrt(r2) + EPS))
    scores = {ratio: [np.empty((len(feats_list), np.asarray(Q).shape[0])) for Q in Xq_list] for ratio in states}
    for k, Q in enumerate(Xq_list):
        Q = np.asarray(Q, dtype=np.float32)
        for s, feats in enumerate(feats_list):
            picks = [restate_cover(Q[:, feats], X[rows[s, t]][:, feats], r2[s, t]) for t in range(T)]
            for ratio, state in states.items():
                total = np.zeros(Q.shape[0])
                for t, (covered, at) in enumerate(picks):
                    total = total + np.where(covered, state[3][s, t][at], 1.0)
                scores[ratio][k][s] = total / float(T)
    return {ratio: (scores[ratio], states[ratio]) for ratio in states}


# ---- the same as the loops of the definition: per row, per estimator, per centre, Python floats ------------------------------
def scalar_d2(a, b):
    acc = 0.0
    for x, y in zip(a, b):
        diff = float(x) - float(y)
        p = diff * diff
        acc = acc + p
    return acc


def scalar_inne(X, Xq, feats_list, T, psi, seed, ratio):
    X, Xq = np.asarray(X, dtype=np.float32), np.asarray(Xq, dtype=np.float32)
    n = X.shape[0]
    S = len(feats_list)
    rows, nn = np.zeros((S, T, psi), np.int32), np.zeros((S, T, psi), np.int32)
    r2, rho = np.zeros((S, T, psi)), np.zeros((S, T, psi))
    score = np.zeros((S, Xq.shape[0]))
    for s, feats in enumerate(feats_list):
        for t in range(T):
            c = [int(v) for v in feistel_perm_ref(np.arange(psi), n, seed, s * T + t)]
            rows[s, t] = c
            for j in range(psi):
                best = None
                for i in range(psi):
                    if i == j:
                        continue
                    key = (scalar_d2(X[c[j], feats], X[c[i], feats]), i)
                    if best is None or key < best:
                        best = key
                r2[s, t, j], nn[s, t, j] = best
            for j in range(psi):
                mine, theirs = float(r2[s, t, j]), float(r2[s, t, nn[s, t, j]])
                if ratio == "distance":
                    mine, theirs = float(np.sqrt(mine)), float(np.sqrt(theirs))
                rho[s, t, j] = 1.0 - (theirs + EPS) / (mine + EPS)
        for q in range(Xq.shape[0]):
            total = 0.0
            for t in range(T):
                best = None
                for j in range(psi):
                    if scalar_d2(Xq[q, feats], X[rows[s, t, j], feats]) <= r2[s, t, j]:
                        key = (float(r2[s, t, j]), j)
                        if best is None or key < best:
                            best = key
                total = total + (1.0 if best is None else float(rho[s, t, best[1]]))
            score[s, q] = total / float(T)
    return score, (rows, r2, nn, rho)


def _same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    assert a.dtype == b.dtype == np.float64 and a.shape == b.shape
    np.testing.assert_array_equal(a.view(np.uint64), b.view(np.uint64))


def _duplicated(n, d, seed):
    """tied_data with a third of the rows duplicated."""
    X = tied_data(n, d, seed)
    X[n - n // 3:] = X[:n // 3]
    return X


# ---- a case worked by hand --------------------------------------------------------------------------------------------------
def test_hand_computed_case():
    """Four centres on a line at 0, 1, 3, 7 (positions 0 .. 3).  d2: (0,1) 1, (0,2) 9, (0,3) 49, (1,2) 4, (1,3) 36, (2,3) 16.
    nn = (1, 0, 1, 2), r2 = (1, 1, 4, 16).  rho squared: (0, 0, 1 - (1 + eps) / (4 + eps), 1 - (4 + eps) / (16 + eps)), both
    0.75 to within an ulp; rho distance: (0, 0, 1 - (1 + eps) / (2 + eps), 1 - (2 + eps) / (4 + eps)), both 0.5.
    Queries: 0.5 is covered by centres 0 and 1 (r2 1 and 1: position 0 wins) -> 0; 2 lies on the sphere of centre 1 (d2 1 <= 1)
    and inside that of centre 2 -> centre 1, 0; 4.5 is covered by centres 2 (r2 4) and 3 (r2 16) -> centre 2, rho 0.75; 10 by
    centre 3 alone -> its rho; 12 (d2 25 > 16) and -2 (d2 4 > 1) by none -> 1."""
    C = np.array([[0.0], [1.0], [3.0], [7.0]], np.float32)
    r2, nn, rho = restate_spheres(C, "squared")
    np.testing.assert_array_equal(nn, [1, 0, 1, 2])
    np.testing.assert_array_equal(r2, [1.0, 1.0, 4.0, 16.0])
    np.testing.assert_array_equal(rho, [0.0, 0.0, 1.0 - (1.0 + EPS) / (4.0 + EPS), 1.0 - (4.0 + EPS) / (16.0 + EPS)])
    np.testing.assert_allclose(rho[2:], 0.75, rtol=0, atol=2.0 ** -52)
    r2d, nnd, rhod = restate_spheres(C, "distance")
    np.testing.assert_array_equal(nnd, nn)
    np.testing.assert_array_equal(r2d, r2)
    np.testing.assert_array_equal(rhod, [0.0, 0.0, 1.0 - (1.0 + EPS) / (2.0 + EPS), 1.0 - (2.0 + EPS) / (4.0 + EPS)])
    np.testing.assert_allclose(rhod[2:], 0.5, rtol=0, atol=2.0 ** -52)
    Q = np.array([[0.5], [2.0], [4.5], [10.0], [12.0], [-2.0]], np.float32)
    covered, at = restate_cover(Q, C, r2)
    np.testing.assert_array_equal(covered, [True, True, True, True, False, False])
    np.testing.assert_array_equal(at[:4], [0, 1, 2, 3])


def test_hand_computed_tie_goes_to_the_lower_position():
    """Centres at 2, 0, 4, 10 (positions 0 .. 3): centre 0 is at d2 4 from positions 1 and 2, the lower position wins.
    nn = (1, 0, 0, 2), r2 = (4, 4, 4, 36); rho squared (0, 0, 0, 1 - (4 + eps) / (36 + eps)) = 8/9, distance 1 - (2 + eps) /
    (6 + eps) = 2/3.  The query 3 is covered by positions 0 and 2 with equal radii: position 0."""
    C = np.array([[2.0], [0.0], [4.0], [10.0]], np.float32)
    r2, nn, rho = restate_spheres(C, "squared")
    np.testing.assert_array_equal(nn, [1, 0, 0, 2])
    np.testing.assert_array_equal(r2, [4.0, 4.0, 4.0, 36.0])
    np.testing.assert_array_equal(rho, [0.0, 0.0, 0.0, 1.0 - (4.0 + EPS) / (36.0 + EPS)])
    assert abs(rho[3] - 8.0 / 9.0) < 1e-15
    rhod = restate_spheres(C, "distance")[2]
    np.testing.assert_array_equal(rhod, [0.0, 0.0, 0.0, 1.0 - (2.0 + EPS) / (6.0 + EPS)])
    assert abs(rhod[3] - 2.0 / 3.0) < 1e-15
    covered, at = restate_cover(np.array([[3.0], [1.0], [6.5]], np.float32), C, r2)
    np.testing.assert_array_equal(covered, [True, True, True])
    np.testing.assert_array_equal(at, [0, 0, 3])  # 3: positions 0 and 2; 1: positions 0 and 1; 6.5: d2 6.25 > 4, position 3 alone
    # through the sampler: n = psi = 4 draws a permutation of the four rows, whatever it is the radii follow the rows
    X = C
    score, (rows, r2s, nns, rhos) = restate_inne(X, X, [[0]], 3, 4, 5)
    for t in range(3):
        assert sorted(rows[0, t].tolist()) == [0, 1, 2, 3]
        np.testing.assert_array_equal(r2s[0, t], r2[rows[0, t]])
        np.testing.assert_array_equal(rows[0, t][nns[0, t]][rows[0, t] == 3], [2])  # row 3 (at 10) has row 2 (at 4) nearest
    np.testing.assert_array_equal(score[0, :3], 0.0)  # rows 0 .. 2 are covered by a sphere of ratio 0 in every estimator
    assert abs(score[0, 3] - 8.0 / 9.0) < 2e-15  # (a + a + a) / 3


# ---- the scalar loops -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ratio", ["squared", "distance"])
def test_vectorised_restatement_equals_the_scalar_loops(ratio):
    X = _duplicated(60, 6, seed=3)
    Q = np.vstack([_duplicated(20, 6, seed=4), X[:10], X[:3] + np.float32(50.0)])
    feats_list = [[0, 1, 2, 3, 4, 5], [3], [1, 2], [1], [0, 5]]
    T, psi, seed = 3, 7, 11
    want, want_state = scalar_inne(X, Q, feats_list, T, psi, seed, ratio)
    got, state = restate_inne(X, Q, feats_list, T, psi, seed, ratio)
    np.testing.assert_array_equal(state[0], want_state[0])
    np.testing.assert_array_equal(state[2], want_state[2])
    _same_bits(state[1], want_state[1])
    _same_bits(state[3], want_state[3])
    _same_bits(got, want)
    assert (state[1] == 0).any() and len(np.unique(state[1][2])) < state[1][2].size  # zero radii and equal radii are in there


def test_the_two_ratio_sweep_is_the_restatement():
    X, Q = _duplicated(90, 6, seed=8), _duplicated(31, 6, seed=9)
    feats_list = [[0, 1, 2, 3, 4, 5], [3], [1, 2]]
    both = restate_inne_both(X, [X, Q], feats_list, 4, "auto", 2)
    for ratio in ("squared", "distance"):
        scores, state = both[ratio]
        for Y, got in zip((X, Q), scores):
            want, want_state = restate_inne(X, Y, feats_list, 4, "auto", 2, ratio)
            _same_bits(got, want)
        for a, b in zip(state, want_state):
            assert a.dtype == b.dtype and np.array_equal(a, b)


# ---- sklearn where there are no ties ------------------------------------------------------------------------------------------
def test_radii_and_nearest_centres_are_sklearns():
    from sklearn.neighbors import NearestNeighbors
    X = np.random.default_rng(2).normal(size=(400, 9)).astype(np.float32)
    feats_list = [[0, 1], [2, 3, 4, 5, 6], list(range(9))]
    T, psi = 4, 33
    rows, r2, nn, _ = restate_inne_build(X, feats_list, T, psi, 1)
    for s, feats in enumerate(feats_list):
        for t in range(T):
            C = X[rows[s, t]][:, feats].astype(np.float64)
            dist, idx = NearestNeighbors(n_neighbors=2, algorithm="brute").fit(C).kneighbors(C)
            np.testing.assert_array_equal(idx[:, 0], np.arange(psi))
            np.testing.assert_array_equal(idx[:, 1], nn[s, t])
            np.testing.assert_allclose(dist[:, 1] ** 2, r2[s, t], rtol=1e-12, atol=0)


# ---- structure ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,psi", [(2, 2), (3, 3), (100, 7), (300, 64), (300, 8)])
@pytest.mark.parametrize("ratio", ["squared", "distance"])
def test_restatement_obeys_the_definition(n, psi, ratio):
    X = _duplicated(n, 6, seed=n + psi)
    feats_list = [[0, 1, 2, 3, 4, 5], [3], [1, 2, 3], [0]]
    T = 3
    rows, r2, nn, rho = restate_inne_build(X, feats_list, T, psi, 7, ratio)
    assert rows.shape == r2.shape == nn.shape == rho.shape == (4, T, psi)
    assert rows.dtype == np.int32 and nn.dtype == np.int32 and r2.dtype == np.float64 and rho.dtype == np.float64
    for s, feats in enumerate(feats_list):
        for t in range(T):
            assert len(set(rows[s, t].tolist())) == psi and rows[s, t].min() >= 0 and rows[s, t].max() < n
            np.testing.assert_array_equal(rows[s, t], feistel_perm_ref(np.arange(psi), n, 7, s * T + t))
            assert (nn[s, t] != np.arange(psi)).all() and nn[s, t].min() >= 0 and nn[s, t].max() < psi
            assert (r2[s, t][nn[s, t]] <= r2[s, t]).all()
            # every centre is covered by a sphere of radius at most its own
            C = X[rows[s, t]][:, feats]
            covered, at = restate_cover(C, C, r2[s, t])
            assert covered.all() and (r2[s, t][at] <= r2[s, t]).all()
    assert (rho >= 0).all() and (rho <= 1).all()
    far = X[:4] + np.float32(1000.0)  # moved in every feature but the constant one
    far[:, 3] = X[:4, 3]
    score = restate_inne_scores(X, np.vstack([X, far]), feats_list, (rows, r2, nn, rho))
    assert (score >= 0).all() and (score <= 1).all()
    assert (r2[1] == 0).all() and (rho[1] == 0).all()  # the constant column: 1 - eps / eps
    assert (score[1] == 0).all()  # ... and every row has that value, so every sphere of radius 0 covers it
    assert (score[[0, 2, 3], n:] == 1).all()  # the far rows are covered by nothing


def test_far_rows_in_the_constant_subspace():
    """A far row in the constant subspace is not on the fitted value: d2 > 0 = r2, so nothing covers it and it scores 1;
    a row that has the fitted value scores exactly 0."""
    X = _duplicated(50, 6, seed=1)
    state = restate_inne_build(X, [[3]], 5, 8, 0)
    Q = X[:3].copy()
    Q[1, 3] += 1.0
    np.testing.assert_array_equal(restate_inne_scores(X, Q, [[3]], state)[0], [0.0, 1.0, 0.0])


def test_restatement_separates_the_planted_rows():
    """tests/test_outlier_gpu.py::_planted over the subspace [0, 1], T = 200, psi = 8, seed 0: every planted row scores above
    every inlier in both ratio modes."""
    X = _planted()
    for ratio in ("squared", "distance"):
        score, _ = restate_inne(X, X, [[0, 1]], 200, "auto", 0, ratio)
        print(f"{ratio}: lowest planted {score[0, 2000:].min():.3f}, highest inlier {score[0, :2000].max():.3f}")
        assert score[0, 2000:].min() > score[0, :2000].max()


# ---- the class, without a device ----------------------------------------------------------------------------------------------
def test_constructor_and_argument_errors_touch_no_device():
    import vgan_amd
    from vgan_amd import outlier
    m = _mask(4, [[0, 1], [2, 3]])
    ens = vgan_amd.SubspaceINNE(m, [0.5, 0.5])
    assert list(inspect.signature(vgan_amd.SubspaceINNE.__init__).parameters) == [
        "self", "subspaces", "proba", "n_estimators", "max_samples", "ratio", "seed", "workspace_bytes", "normalize", "combination",
        "contamination"]
    assert (ens.n_estimators, ens.max_samples, ens.ratio, ens.seed) == (200, "auto", "squared", 0)
    assert outlier.INNE_AUTO_SAMPLES == 8 and outlier.check_inne_samples("auto") == 8
    assert ens.ops is None and ens.workspace_bytes == outlier.DEFAULT_WORKSPACE_BYTES
    assert (ens.normalize, ens.combination, ens.contamination) == (None, "sum", 0.1)
    assert list(ens.plan.order) == [0, 1]  # the given order
    for name in ("n_neighbors", "engine", "splits", "max_features"):
        assert not hasattr(ens, name)
        with pytest.raises(TypeError):
            vgan_amd.SubspaceINNE(m, [0.5, 0.5], **{name: 1})
    for bad in (0, 1025, -1, 2.0, True, None):
        with pytest.raises(ValueError, match="n_estimators must be an integer between 1 and 1024"):
            vgan_amd.SubspaceINNE(m, [0.5, 0.5], n_estimators=bad)
    for bad in (1, 1025, 0.5, 8.0, "all", None, True):
        with pytest.raises(ValueError, match="max_samples must be 'auto' or an integer between 2 and 1024"):
            vgan_amd.SubspaceINNE(m, [0.5, 0.5], max_samples=bad)
    for bad in ("euclidean", 0, None, True):
        with pytest.raises(ValueError, match="ratio must be 'squared' or 'distance'"):
            vgan_amd.SubspaceINNE(m, [0.5, 0.5], ratio=bad)
    for bad in (-1, 1 << 64, 0.0, "0", None):
        with pytest.raises(ValueError, match=r"seed must be an integer in \[0, 2\^64\)"):
            vgan_amd.SubspaceINNE(m, [0.5, 0.5], seed=bad)
    ok = vgan_amd.SubspaceINNE(m, [0.5, 0.5], n_estimators=1024, max_samples=1024, ratio="distance", seed=(1 << 64) - 1)
    assert (ok.n_estimators, ok.max_samples, ok.ratio, ok.seed) == (1024, 1024, "distance", (1 << 64) - 1)
    assert vgan_amd.SubspaceINNE(m, [0.5, 0.5], n_estimators=1, max_samples=2).max_samples == 2
    with pytest.raises(ValueError, match="proba has 3 entries for 2 subspaces"):
        vgan_amd.SubspaceINNE(m, [0.5, 0.25, 0.25])
    with pytest.raises(ValueError, match="normalize"):
        vgan_amd.SubspaceINNE(m, [0.5, 0.5], normalize="l2")
    with pytest.raises(ValueError, match="combination"):
        vgan_amd.SubspaceINNE(m, [0.5, 0.5], combination="mean")
    with pytest.raises(ValueError, match="contamination"):
        vgan_amd.SubspaceINNE(m, [0.5, 0.5], contamination=0.7)
    with pytest.raises(ValueError, match="a subspace has 8193 features, SubspaceINNE takes at most 8192"):
        vgan_amd.SubspaceINNE(np.ones((1, 8193), bool), [1.0])
    with pytest.raises(ValueError, match="SubspaceINNE fit needs between 2 and 2147483647 rows, got 1"):
        ens.fit(np.zeros((1, 4), np.float32))
    with pytest.raises(ValueError, match="features"):
        ens.fit(np.zeros((5, 3), np.float32))

    class Tall:  # only its shape is looked at before the row check raises
        shape = (1 << 31, 4)

    with pytest.raises(ValueError, match="between 2 and"):
        ens.fit(Tall())
    assert ens.ops is None  # none of this touched the device
    for attr in ("center_rows_", "radius_sq_", "center_nn_", "isolation_ratio_"):
        with pytest.raises(RuntimeError, match="not fitted"):
            getattr(ens, attr)
    with pytest.raises(RuntimeError, match="not fitted"):
        ens.decision_function(np.zeros((5, 4), np.float32))
    doc = vgan_amd.SubspaceINNE.__doc__
    assert "pyod" in doc and "not pinned" in doc and "fraction" in doc and "24 T psi bytes" in doc and "workspace_bytes" in doc
    assert "SubspaceINNE" in outlier.__doc__


def test_outlier_ensemble_routes_inne_to_the_new_class():
    import vgan_amd
    model = vgan_amd.VGAN_no_kl(epochs=1)
    model.subspaces = _mask(6, [[0, 1], [2, 3, 5], [4]])
    model.proba = np.array([0.5, 0.3, 0.2])
    ens = model.outlier_ensemble(method="inne")
    assert type(ens) is vgan_amd.SubspaceINNE and ens.n_estimators == 200 and ens.plan.count == 3
    np.testing.assert_array_equal(ens.proba, model.proba)
    ens = model.outlier_ensemble(method="inne", n_neighbors=17, n_estimators=7, max_samples=64, ratio="distance", seed=3,
                                 normalize="robust", combination="max", contamination=0.05, workspace_bytes=1 << 20)
    assert (ens.n_estimators, ens.max_samples, ens.ratio, ens.seed, ens.normalize, ens.combination, ens.contamination,
            ens.workspace_bytes) == (7, 64, "distance", 3, "robust", "max", 0.05, 1 << 20)
    assert not hasattr(ens, "n_neighbors")  # it is ignored
    with pytest.raises(TypeError):
        model.outlier_ensemble(method="inne", engine="exact")  # not a keyword of SubspaceINNE
    assert "inne" in vgan_amd.VGAN_no_kl.outlier_ensemble.__doc__
    assert "SubspaceINNE" in vgan_amd.__all__
    with pytest.raises(ValueError, match="method"):  # the neighbour ensemble still does not know it
        vgan_amd.SubspaceEnsemble(model.subspaces, model.proba, method="inne")


# ---- C ABI: argument checks without a GPU -----------------------------------------------------------------------------------
def test_inne_entries_reject_bad_arguments_without_gpu():
    import vgan_amd
    from vgan_amd import outlier
    lib = vgan_amd.lib.load()
    header = open(os.path.join(REPO, "include", "vgan_hip.h")).read()
    assert int(re.search(r"#define VGAN_INNE_MAX_SAMPLES (\d+)", header).group(1)) == outlier.INNE_MAX_SAMPLES
    assert int(re.search(r"#define VGAN_INNE_MAX_ESTIMATORS (\d+)", header).group(1)) == outlier.INNE_MAX_ESTIMATORS
    assert int(re.search(r"#define VGAN_INNE_MAX_DIMS (\d+)", header).group(1)) == outlier.INNE_MAX_DIMS
    for name, value in outlier.INNE_RATIOS.items():
        assert int(re.search(rf"#define VGAN_INNE_RATIO_{name.upper()} (\d+)", header).group(1)) == value
    null = None
    buf = ctypes.create_string_buffer(256)
    p = ctypes.cast(ctypes.addressof(buf) + (-ctypes.addressof(buf)) % 16, ctypes.c_void_p)  # never read

    def rejected(rc):
        msg = lib.vgan_last_error()
        return rc == 1 and b"bad argument" in msg and b"outlier_inne.hip" in msg

    def each(fn, good, pointers, bad_values):
        for pos in pointers:
            assert rejected(fn(*[null if i == pos else v for i, v in enumerate(good)])), pos
        for pos, bad in bad_values:
            assert rejected(fn(*[bad if i == pos else v for i, v in enumerate(good)])), (pos, bad)

    # X, ldx, n, d, feat, feat_off, first, count, max_dims, T, psi, ratio, seed, rows, r2, nn, rho, stream
    each(lib.vgan_inne_build, [p, 4, 100, 4, p, p, 0, 2, 3, 5, 8, 0, 0, p, p, p, p, null], (0, 4, 5, 13, 14, 15, 16),
         [(1, 3), (2, 1), (2, 1 << 31), (2, 7), (3, 0), (6, -1), (7, 0), (7, 65536), (8, 0), (8, 5), (8, outlier.INNE_MAX_DIMS + 1), (9, 0),
          (9, outlier.INNE_MAX_ESTIMATORS + 1), (10, 1), (10, 101), (10, outlier.INNE_MAX_SAMPLES + 1), (11, 2), (11, -1)])
    # Xq, ldq, nq, d, X, ldx, n, feat, feat_off, first, count, max_dims, T, psi, rows, r2, rho, score, ld_score, stream
    each(lib.vgan_inne_scores, [p, 4, 10, 4, p, 4, 100, p, p, 0, 2, 3, 5, 8, p, p, p, p, 10, null], (0, 4, 7, 8, 14, 15, 16, 17),
         [(1, 3), (2, 0), (3, 0), (5, 3), (6, 1), (6, 1 << 31), (6, 7), (9, -1), (10, 0), (10, 65536), (11, 0), (11, 5), (12, 0), (12, 1025),
          (13, 1), (13, 101), (13, 1025), (18, 9)])
    for name, nargs in (("vgan_inne_build", 18), ("vgan_inne_scores", 20)):
        assert len(vgan_amd.lib.SIGNATURES[name][1]) == nargs
    assert vgan_amd.lib.ABI_VERSION == lib.vgan_abi_version() == 11
