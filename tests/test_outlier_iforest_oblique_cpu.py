"""Oblique (extended) isolation-forest cuts, SubspaceIForest(n_dims = q >= 2), CPU tier: the numpy restatement the GPU tests
compare against, pinned to a case worked by hand, to the position and weight rules, to the structural rules of the
definition and to sklearn's axis-parallel forest on a recipe only joint cuts separate; and everything of the keyword that
runs without a device (defaults, argument checks, the dispatch, the C ABI's argument checks).

The definition is SubspaceIForest's docstring ("Oblique cuts"): the candidates of a subspace are its features that vary over
the fitted rows; attempt a = 0 .. 3 of a node uses the Philox4x32-10 blocks at counter (node, 32 a + b, 0x45494600, 0) under
the tree's key: block 0 gives the threshold word w1, blocks 1 .. 4 the position words, block 5 + i weight i.  Python ints for
the position rule, numpy float64 and float32 for the rest."""
import ctypes
import functools
import os
import re

import numpy as np
import pytest

from conftest import REPO
from small_ops_ref import feistel_perm_ref, philox4x32_10  # noqa: F401  (feistel_perm_ref: through restate_sample)
from test_outlier_ecod_cpu import _mask, tied_data
from test_outlier_iforest_cpu import auc, depth_limit, restate_cq, restate_sample, restate_score

OBLIQUE_TAG = 0x45494600
ATTEMPTS = 4
MAX_PLANE = 16
BLOCKS = 5 + MAX_PLANE  # of one attempt: the threshold word, four of positions, sixteen of weights
WEIGHT_CENTRE = 8589934590.0  # 2 (2^32 - 1): the mean of the sum of four words


# ---- the restatement --------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=256)
def attempt_blocks(seed, stream, L):
    """uint64 [2^L, 4, 21, 4]: the words of block b of attempt a of every node that can be internal (node < 2^L) of the tree
    with that stream id; read-only, shared between the callers."""
    seed, stream = int(seed), int(stream)
    k0 = (seed & 0xFFFFFFFF) ^ (stream & 0xFFFFFFFF)
    k1 = (seed >> 32) ^ (stream >> 32) ^ 0x5bd1e995
    node = np.arange(1 << L, dtype=np.uint64)[:, None, None]
    second = (32 * np.arange(ATTEMPTS, dtype=np.uint64)[:, None] + np.arange(BLOCKS, dtype=np.uint64))[None]
    node, second = np.broadcast_arrays(node, second)
    words = np.stack(philox4x32_10((node, second, np.full(node.shape, OBLIQUE_TAG, np.uint64), np.zeros(node.shape, np.uint64)), k0, k1),
                     axis=-1)
    words.setflags(write=False)
    return words


def restate_plane(blocks, c, m):
    """(positions int [m] ascending, weights float32 [m] in that order, w1): the draws of one attempt from its blocks
    [21, 4] for c candidates and m = min(q, c) of them chosen."""
    chosen = []
    for i in range(m):
        j = (int(blocks[1 + (i >> 2)][i & 3]) * (c - i)) >> 32
        for p in sorted(pos for pos, _ in chosen):
            if p <= j:
                j += 1
        t = sum(int(v) for v in blocks[5 + i])
        chosen.append((j, np.float32((float(t) - WEIGHT_CENTRE) * 2.0 ** -32)))  # exact up to the one rounding
    chosen.sort(key=lambda pw: pw[0])
    return np.array([p for p, _ in chosen], np.int64), np.array([w for _, w in chosen], np.float32), int(blocks[0][1])


def _canonical(X):
    return np.asarray(X, dtype=np.float32) + np.float32(0.0)  # -0.0 + 0.0 is +0.0


def restate_projection(Xc, rows, cols, weights):
    """float32 [len(rows)]: acc = 0.0; acc = acc + double(w) double(x) over the columns as given; float32(acc)."""
    acc = np.zeros(len(rows), np.float64)
    for col, w in zip(cols, weights):
        acc = acc + np.float64(w) * Xc[rows, col].astype(np.float64)  # the product is exact, the sum rounded once
    return acc.astype(np.float32)


def restate_candidates(X, feats_list):
    """[int32 array]: per subspace its features whose float32 column maximum exceeds the minimum (-0.0 as +0.0), ascending."""
    Xc = _canonical(X)
    varying = Xc.max(axis=0) > Xc.min(axis=0)
    return [np.array([f for f in sorted(feats) if varying[f]], np.int32) for feats in feats_list]


def restate_oblique_tree(X, cand, rows, L, q, seed, stream, members=None, tried=None):
    """(attempt int32 [N], threshold float32 [N], size int32 [N], plane_col int32 [N, q], plane_w float32 [N, q]) of one tree
    on the sample `rows` of X with the candidates `cand` (columns of X, ascending).  attempt: the successful attempt of an
    internal node, -1 a leaf, -2 absent.  members receives node -> its rows, tried node -> the attempts made (0 .. 4)."""
    Xc = _canonical(X)
    cand = np.asarray(cand, np.int64)
    c, m = len(cand), min(q, len(cand))
    N = 2 << L
    attempt = np.full(N, -2, np.int32)
    threshold = np.zeros(N, np.float32)
    size = np.zeros(N, np.int32)
    plane_col = np.full((N, q), -1, np.int32)
    plane_w = np.zeros((N, q), np.float32)
    words = attempt_blocks(seed, stream, L)
    todo = [(1, 0, np.asarray(rows))]
    while todo:
        node, e, R = todo.pop()
        size[node], attempt[node] = len(R), -1
        if members is not None:
            members[node] = R
        if len(R) <= 1 or e == L or c == 0:
            continue
        for a in range(ATTEMPTS):
            pos, w, w1 = restate_plane(words[node, a], c, m)
            zf = restate_projection(Xc, R, cand[pos], w)
            lo, hi = zf.min(), zf.max()
            if lo != hi:
                break
        else:
            a = ATTEMPTS
        if tried is not None:
            tried[node] = min(a + 1, ATTEMPTS)
        if a == ATTEMPTS:
            continue  # a leaf: every attempt projected the rows onto one value
        u = (float(w1) + 0.5) * 2.0 ** -32  # exact
        lo64, hi64 = float(lo), float(hi)
        p = np.float32(lo64 + u * (hi64 - lo64))  # Python floats: three separately rounded float64 operations
        if p >= hi:
            p = lo
        attempt[node], threshold[node] = a, p
        plane_col[node, :m], plane_w[node, :m] = cand[pos], w
        left = zf <= p  # float32 against float32
        todo.append((2 * node, e + 1, R[left]))
        todo.append((2 * node + 1, e + 1, R[~left]))
    return attempt, threshold, size, plane_col, plane_w


def restate_oblique_forest(X, cands, T, psi, q, seed):
    """(attempt, threshold, size) [S, T, N] and (plane_col, plane_w) [S, T, N, q]: the trees of every subspace, stream id s T + t."""
    n, L = np.asarray(X).shape[0], depth_limit(psi)
    out = [restate_oblique_tree(X, cand, restate_sample(n, psi, seed, s * T + t), L, q, seed, s * T + t)
           for s, cand in enumerate(cands) for t in range(T)]
    return tuple(np.stack([o[k] for o in out]).reshape((len(cands), T) + out[0][k].shape) for k in range(5))


def restate_oblique_path_sums(attempt, threshold, size, plane_col, plane_w, Xq, cq):
    """int64 [nq]: the total over the trees ([T, N] and [T, N, q] heap arrays) of (depth << 32) + cq[leaf size]."""
    Xc = _canonical(Xq)
    at = np.arange(Xc.shape[0])
    total = np.zeros(Xc.shape[0], np.int64)
    for att, thr, sz, pc, pw in zip(attempt, threshold, size, plane_col, plane_w):
        node = np.ones(Xc.shape[0], np.int64)
        while True:
            inner = att[node] >= 0
            if not inner.any():
                break
            acc = np.zeros(Xc.shape[0], np.float64)
            for k in range(pc.shape[1]):
                col = pc[node, k]
                term = acc + pw[node, k].astype(np.float64) * Xc[at, np.maximum(col, 0)].astype(np.float64)
                acc = np.where(inner & (col >= 0), term, acc)
            right = ~(acc.astype(np.float32) <= thr[node])
            node = np.where(inner, 2 * node + right, node)
        depth = np.frexp(node.astype(np.float64))[1] - 1  # floor(log2 node)
        total += (depth.astype(np.int64) << 32) + cq[sz[node]]
    return total


def restate_oblique_iforest(X_fit, X_query, feats_list, T, max_samples, q, seed, forest=None):
    """(scores float64 [S, nq] before the rounding to float32, sums int64 [S, nq], the forest)."""
    n = np.asarray(X_fit).shape[0]
    psi = min(256 if max_samples == "auto" else max_samples, n)
    cq = restate_cq(psi)
    if forest is None:
        forest = restate_oblique_forest(X_fit, restate_candidates(X_fit, feats_list), T, psi, q, seed)
    sums = np.stack([restate_oblique_path_sums(*(a[s] for a in forest), X_query, cq) for s in range(len(feats_list))])
    return restate_score(sums, T, cq[psi]), sums, forest


def ghost(seed, n=2000, n_out=20, d=6):
    """Two blobs at (0, 10) and (10, 0) in features 0 and 1, the outliers at (0, 0) or (10, 10): inside both marginals."""
    r = np.random.default_rng(seed)
    X = r.standard_normal((n, d)); y = np.zeros(n, bool)
    half = r.random(n) < 0.5
    X[half, 1] += 10; X[~half, 0] += 10
    idx = r.choice(n, n_out, replace=False); y[idx] = True
    g = r.random(n_out) < 0.5
    X[idx, 0] = r.standard_normal(n_out) + np.where(g, 0, 10)
    X[idx, 1] = r.standard_normal(n_out) + np.where(g, 0, 10)
    return X.astype(np.float32), y


#: the bars of test_oblique_cuts_separate_the_ghost_recipe, shared with the GPU module: 0.01 beyond each side's worst seed
OBLIQUE_AUC_BAR = 0.9765  # the restatement's worst seed, 0.9865, less 0.01
SKLEARN_AUC_BAR = 0.9149  # sklearn's best seed, 0.9049, plus 0.01


# ---- a case worked by hand --------------------------------------------------------------------------------------------------
def test_hand_computed_case():
    """n = 4, d = 3, psi = 4, T = 1, q = 2, seed 0: the sample is all four rows, L = 2, N = 8, every feature a candidate (c = 3,
    m = 2); X = (0 0 0), (1 0 3), (0 2 1), (4 4 0).  The words of attempt 0 of the stream 0 (checked below against the Philox
    restatement, itself pinned in test_small_ops_cpu.py):

      node 1: position words 0x33292855, 0x08371EBA: j = (w 3) >> 32 = 0; j = (w 2) >> 32 = 0, and the chosen 0 <= 0 moves it
              to 1.  Positions (0, 1).  The word sums 4960709888 and 7674930474 give the weights (t - 8589934590) / 2^32 =
              -0.8449947, -0.2130410.  zf = -0.8449947 x0 - 0.2130410 x1 = 0, -0.8449947, -0.4260820, -4.2321430.
              w1 = 0x8C810C94, u = 0.5488441: p = float32(-4.2321430 + u 4.2321430) = -1.9093561 -> rows {3} | {0, 1, 2}
      node 3: position words 0x92EF4BE8, 0x3C16B4D2: j = 1; j = 0, and the chosen 1 > 0 leaves it.  Draw 0 is position 1 and
              draw 1 position 0, so the sums 2244214134, 7928984041 give weight -1.4774781 on feature 1 and -0.1538895 on
              feature 0.  zf = -0.1538895 x0 - 1.4774781 x1 = 0, -0.1538895, -2.9549563 on rows 0, 1, 2.
              w1 = 0xD1E13C84, u = 0.8198431: p = float32(-2.9549563 + u 2.9549563) = -0.5323558 -> rows {2} | {0, 1}
      node 7 is at depth 2 = L: a leaf of 2 rows.

    Leaves: node 2 (depth 1, 1 row), node 6 (depth 2, 1 row), node 7 (depth 2, 2 rows).  With c(1) = 0 and c(2) = 1 the path
    lengths of the rows are 3, 3, 2, 1, as in the hand-worked case of the axis-parallel forest."""
    X = np.array([[0, 0, 0], [1, 0, 3], [0, 2, 1], [4, 4, 0]], np.float32)
    words = attempt_blocks(0, 0, 2)
    assert words.shape == (4, ATTEMPTS, BLOCKS, 4)
    assert [int(words[1, 0, 1, i]) for i in (0, 1)] == [0x33292855, 0x08371EBA] and int(words[1, 0, 0, 1]) == 0x8C810C94
    assert [int(words[3, 0, 1, i]) for i in (0, 1)] == [0x92EF4BE8, 0x3C16B4D2] and int(words[3, 0, 0, 1]) == 0xD1E13C84
    assert [sum(int(v) for v in words[1, 0, b]) for b in (5, 6)] == [4960709888, 7674930474]
    assert [sum(int(v) for v in words[3, 0, b]) for b in (5, 6)] == [2244214134, 7928984041]
    # one block by the scalar route: counter (node, 32 a + b, tag, 0) under the key of seed 0, stream 0
    np.testing.assert_array_equal(words[3, 2, 7], [int(v) for v in philox4x32_10((3, 32 * 2 + 7, OBLIQUE_TAG, 0), 0, 0x5bd1e995)])
    np.testing.assert_array_equal(restate_sample(4, 4, 0, 0), [0, 1, 2, 3])
    np.testing.assert_array_equal(restate_candidates(X, [[0, 1, 2]])[0], [0, 1, 2])

    def weight(t):
        return np.float32((t - 8589934590) / 2.0 ** 32)

    pos, w, w1 = restate_plane(words[1, 0], 3, 2)
    assert pos.tolist() == [0, 1] and w.tolist() == [weight(4960709888), weight(7674930474)] and w1 == 0x8C810C94
    pos, w, w1 = restate_plane(words[3, 0], 3, 2)
    assert pos.tolist() == [0, 1] and w.tolist() == [weight(7928984041), weight(2244214134)] and w1 == 0xD1E13C84
    attempt, threshold, size, plane_col, plane_w = restate_oblique_tree(X, [0, 1, 2], np.arange(4), 2, 2, 0, 0)
    np.testing.assert_array_equal(attempt, [-2, 0, -1, 0, -2, -2, -1, -1])
    np.testing.assert_array_equal(size, [0, 4, 1, 3, 0, 0, 1, 2])
    np.testing.assert_array_equal(plane_col[[1, 3]], [[0, 1], [0, 1]])
    assert (plane_col[[0, 2, 4, 5, 6, 7]] == -1).all() and (plane_w[[0, 2, 4, 5, 6, 7]] == 0).all()
    np.testing.assert_allclose(plane_w[[1, 3]], [[-0.8449947, -0.2130410], [-0.1538895, -1.4774781]], rtol=0, atol=5e-8)
    z1 = np.float32(np.float64(weight(4960709888)) * 4.0 + np.float64(weight(7674930474)) * 4.0)  # row 3 at the root
    z3 = np.float32(np.float64(weight(2244214134)) * 2.0)  # row 2 at node 3: x0 = 0
    assert abs(z1 + 4.2321430) < 1e-6 and abs(z3 + 2.9549563) < 1e-6
    assert threshold[1] == np.float32(float(z1) + (0x8C810C94 + 0.5) / 2.0 ** 32 * (0.0 - float(z1)))
    assert threshold[3] == np.float32(float(z3) + (0xD1E13C84 + 0.5) / 2.0 ** 32 * (0.0 - float(z3)))
    assert abs(threshold[1] + 1.9093561) < 1e-6 and abs(threshold[3] + 0.5323558) < 1e-6 and (threshold[[0, 2, 4, 5, 6, 7]] == 0).all()
    cq = restate_cq(4)
    sums = restate_oblique_path_sums(attempt[None], threshold[None], size[None], plane_col[None], plane_w[None], X, cq)
    one = 1 << 32
    np.testing.assert_array_equal(sums, [3 * one, 3 * one, 2 * one, one])
    per, sums2, _ = restate_oblique_iforest(X, X, [[0, 1, 2]], 1, 4, 2, 0)
    np.testing.assert_array_equal(sums2[0], sums)
    c4 = int(cq[4]) / one
    np.testing.assert_allclose(per[0], 2.0 ** (-np.array([3.0, 3.0, 2.0, 1.0]) / c4), rtol=1e-12)


# ---- the position and the weight rule -------------------------------------------------------------------------------------
@pytest.mark.parametrize("c,m", [(1, 1), (2, 2), (5, 3), (17, 16), (8192, 16)])
def test_positions_are_distinct_and_below_c(c, m):
    for stream in range(20):
        words = attempt_blocks(3, stream, 3)
        for node in range(1, 8):
            for a in range(ATTEMPTS):
                pos, w, _ = restate_plane(words[node, a], c, m)
                assert len(pos) == len(w) == m and len(set(pos.tolist())) == m and 0 <= pos.min() and pos.max() < c
                assert (np.diff(pos) > 0).all()
    if c == m:  # every candidate is taken
        assert pos.tolist() == list(range(c))


def test_position_pairs_are_uniform():
    """The root planes of 2 000 streams (seed 11) with c = 5, m = 2: chi-square on the ten pairs below 27.88 (p = 0.001, 9
    degrees of freedom)."""
    counts = {}
    for stream in range(2000):
        pos, _, _ = restate_plane(attempt_blocks(11, stream, 1)[1, 0], 5, 2)
        counts[tuple(pos.tolist())] = counts.get(tuple(pos.tolist()), 0) + 1
    assert len(counts) == 10 and sum(counts.values()) == 2000
    chi2 = sum((v - 200.0) ** 2 / 200.0 for v in counts.values())
    assert chi2 < 27.88, (counts, chi2)


def test_weights_are_irwin_hall_of_four():
    """20 000 weights (1 250 root planes of 16): float32 in (-2, 2); the mean within 4 standard errors of 0 (the standard
    error is sqrt(1 / 3 / 20 000)), the variance within 5 % of 1 / 3."""
    w = np.concatenate([restate_plane(attempt_blocks(5, stream, 1)[1, 0], 16, 16)[1] for stream in range(1250)])
    assert w.dtype == np.float32 and w.shape == (20000,) and (np.abs(w) < 2).all()
    assert abs(w.astype(np.float64).mean()) < 4.0 * np.sqrt(1.0 / 3.0 / 20000.0)
    assert abs(w.astype(np.float64).var() - 1.0 / 3.0) < 0.05 / 3.0
    # the formula at its ends and centre: the sum of four words is 0 .. 4 (2^32 - 1)
    for t, want in ((2 * (2 ** 32 - 1), 0.0), (2 * (2 ** 32 - 1) + 2 ** 32, 1.0), (2 ** 31, -1.5 + 2.0 ** -31)):
        assert np.float32((float(t) - WEIGHT_CENTRE) * 2.0 ** -32) == np.float32(want)


# ---- structure of the restated trees ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,psi,q", [(2, 2, 2), (3, 3, 2), (100, 7, 3), (300, 256, 2), (300, 64, 16)])
def test_restated_trees_obey_the_definition(n, psi, q):
    X = tied_data(n, 6, seed=n + psi)
    X[n // 2:] = X[:n - n // 2]  # duplicated rows
    Xc = _canonical(X)
    psi = min(psi, n)
    L = depth_limit(psi)
    feats_list = [[0, 1, 2, 3, 4, 5], [3], [1, 2, 3], [0]]
    cands = restate_candidates(X, feats_list)
    assert all(3 not in c and (np.ptp(Xc[:, c], axis=0) > 0).all() for c in cands) and len(cands[1]) == 0  # column 3 is constant
    if n >= 100:
        assert [c.tolist() for c in cands] == [[0, 1, 2, 4, 5], [], [1, 2], [0]]
    later, exhausted = 0, 0
    for s, cand in enumerate(cands):
        c, m = len(cand), min(q, len(cand))
        for t in range(3):
            stream = s * 3 + t
            rows = restate_sample(n, psi, 7, stream)
            members, tried = {}, {}
            attempt, threshold, size, plane_col, plane_w = restate_oblique_tree(X, cand, rows, L, q, 7, stream, members, tried)
            assert size[1] == psi and attempt[0] == -2 and size[0] == 0
            for node, R in members.items():
                e = node.bit_length() - 1
                assert e <= L and size[node] == len(R)
                if attempt[node] == -1:  # a leaf, for one of the four reasons
                    assert len(R) <= 1 or e == L or c == 0 or tried[node] == ATTEMPTS
                    if node in tried:  # all four attempts project R onto a single value
                        exhausted += len(R) > 1
                        for a in range(ATTEMPTS):
                            pos, w, _ = restate_plane(attempt_blocks(7, stream, L)[node, a], c, m)
                            assert len(set(restate_projection(Xc, R, cand[pos], w).tolist())) == 1
                    assert threshold[node] == 0 and (plane_col[node] == -1).all() and (plane_w[node] == 0).all()
                    assert e == L or (attempt[2 * node] == -2 and attempt[2 * node + 1] == -2)
                    continue
                a = attempt[node]
                assert 0 <= a < ATTEMPTS and tried[node] == a + 1 and len(R) > 1 and e < L
                later += a >= 1
                cols, w = plane_col[node, :m], plane_w[node, :m]
                assert (np.diff(cols) > 0).all() and set(cols.tolist()) <= set(cand.tolist()) and 3 not in cols
                assert (plane_col[node, m:] == -1).all() and (plane_w[node, m:] == 0).all()
                zf = restate_projection(Xc, R, cols, w)
                assert zf.min() <= threshold[node] < zf.max()
                assert size[2 * node] >= 1 and size[2 * node + 1] >= 1 and size[2 * node] + size[2 * node + 1] == size[node]
                assert set(members[2 * node].tolist()) == set(R[zf <= threshold[node]].tolist())
            absent = np.setdiff1d(np.arange(2 << L), list(members))
            assert (attempt[absent] == -2).all() and (size[absent] == 0).all() and (threshold[absent] == 0).all()
            assert (plane_col[absent] == -1).all() and (plane_w[absent] == 0).all()
            if c == 0:
                assert attempt[1] == -1 and size[1] == psi  # a root leaf: no candidate
    if (n, psi) == (300, 256):  # a condition on the inputs: both rarer paths of the definition are taken
        assert later >= 1, "no internal node needed a second attempt"
        assert exhausted >= 1, "no leaf of more than one row was reached by exhausting the attempts"


# ---- detection ------------------------------------------------------------------------------------------------------------
def test_oblique_cuts_separate_the_ghost_recipe():
    """ghost (two blobs at (0, 10) and (10, 0) in features 0 and 1 of six, 20 outliers of 2 000 rows at (0, 0) or (10, 10)), all
    six features one subspace, T = 100, psi = 256, seeds 0 to 4 for the data and the forest alike.  ROC AUC measured here:

        sklearn IsolationForest(n_estimators=100, random_state=seed)   0.7271, 0.7173, 0.8394, 0.8094, 0.9049
        the restatement, n_dims = 3, real Philox and Feistel draws      0.9865, 0.9933, 0.9905, 0.9958, 0.9921

    The ranges do not overlap; each side is pinned 0.01 beyond its worst seed (OBLIQUE_AUC_BAR, SKLEARN_AUC_BAR)."""
    from sklearn.ensemble import IsolationForest
    theirs, ours = [], []
    for seed in range(5):
        X, y = ghost(seed)
        theirs.append(auc(-IsolationForest(n_estimators=100, random_state=seed).fit(X).score_samples(X), y))
        ours.append(auc(restate_oblique_iforest(X, X, [list(range(6))], 100, 256, 3, seed)[0][0], y))
    print("sklearn AUC " + ", ".join(f"{v:.4f}" for v in theirs) + "; restatement n_dims = 3 AUC " + ", ".join(f"{v:.4f}" for v in ours))
    assert max(theirs) < min(ours)  # the two ranges do not overlap
    assert min(ours) > OBLIQUE_AUC_BAR and max(theirs) < SKLEARN_AUC_BAR


# ---- the class, without a device ----------------------------------------------------------------------------------------------
def test_keyword_and_argument_errors_touch_no_device():
    import vgan_amd
    from vgan_amd import outlier
    m = _mask(4, [[0, 1], [2, 3]])
    assert outlier.IFOREST_MAX_PLANE == MAX_PLANE
    assert vgan_amd.SubspaceIForest(m, [0.5, 0.5]).n_dims == 1
    for good in (1, 2, 16, np.int64(3)):
        ens = vgan_amd.SubspaceIForest(m, [0.5, 0.5], n_dims=good)
        assert ens.n_dims == good and type(ens.n_dims) is int and ens.ops is None
    for bad in (0, 17, 2.0, True, None, "full", -1):
        with pytest.raises(ValueError, match="n_dims"):
            vgan_amd.SubspaceIForest(m, [0.5, 0.5], n_dims=bad)
    ens = vgan_amd.SubspaceIForest(m, [0.5, 0.5], 7, 64, 3, 2)  # the keyword follows seed
    assert (ens.n_estimators, ens.max_samples, ens.seed, ens.n_dims) == (7, 64, 3, 2)
    for attr in ("tree_feature_", "tree_threshold_", "tree_size_", "tree_attempt_", "plane_features_", "plane_weights_",
                 "candidate_features_"):
        with pytest.raises(RuntimeError, match="not fitted"):
            getattr(ens, attr)
    with pytest.raises(RuntimeError, match="not fitted"):
        ens.decision_function(np.zeros((5, 4), np.float32))
    assert ens.ops is None  # none of this touched the device
    doc = vgan_amd.SubspaceIForest.__doc__
    assert "Hariri" in doc and "Not built" in doc and "SCiForest" in doc and "n_dims" in doc and "0x45494600" in doc


def test_keyword_reaches_the_class_through_the_dispatch():
    import vgan_amd
    from vgan_amd.outlier import build_ensemble
    model = vgan_amd.VGAN_no_kl(epochs=1)
    model.subspaces = _mask(6, [[0, 1], [2, 3, 5], [4]])
    model.proba = np.array([0.5, 0.3, 0.2])
    ens = model.outlier_ensemble(method="iforest", n_dims=3)
    assert type(ens) is vgan_amd.SubspaceIForest and ens.n_dims == 3 and ens.n_estimators == 100
    assert model.outlier_ensemble(method="iforest").n_dims == 1
    ens = build_ensemble(model.subspaces, model.proba, method="iforest", n_dims=16, seed=5)
    assert type(ens) is vgan_amd.SubspaceIForest and (ens.n_dims, ens.seed) == (16, 5)
    with pytest.raises(ValueError, match="n_dims"):
        model.outlier_ensemble(method="iforest", n_dims="full")
    hics = vgan_amd.HiCS()
    hics.subspaces, hics.proba = model.subspaces, model.proba
    assert hics.outlier_ensemble(method="iforest", n_dims=2).n_dims == 2
    assert "n_dims" in vgan_amd.VGAN_no_kl.outlier_ensemble.__doc__ and "n_dims" in vgan_amd.HiCS.outlier_ensemble.__doc__


# ---- C ABI: argument checks without a GPU -----------------------------------------------------------------------------------
def test_oblique_entries_reject_bad_arguments_without_gpu():
    import vgan_amd
    from vgan_amd import outlier
    lib = vgan_amd.lib.load()
    header = open(os.path.join(REPO, "include", "vgan_hip.h")).read()
    assert int(re.search(r"#define VGAN_IFOREST_MAX_PLANE (\d+)", header).group(1)) == outlier.IFOREST_MAX_PLANE
    assert "vgan_iforest_*_oblique" in re.search(r"#define VGAN_ABI_VERSION[^\n]*", header).group(0)
    null = None
    buf = ctypes.create_string_buffer(256)
    p = ctypes.cast(ctypes.addressof(buf) + (-ctypes.addressof(buf)) % 16, ctypes.c_void_p)  # never read

    def rejected(rc):
        msg = lib.vgan_last_error()
        return rc == 1 and b"bad argument" in msg and b"outlier_iforest.hip" in msg

    def each(fn, good, pointers, bad_values):
        for pos in pointers:
            assert rejected(fn(*[null if i == pos else v for i, v in enumerate(good)])), pos
        for pos, bad in bad_values:
            assert rejected(fn(*[bad if i == pos else v for i, v in enumerate(good)])), (pos, bad)

    # X, n, d, cand, cand_off, first, count, T, psi, L, q, seed, nodes, plane_col, plane_w, stream
    each(lib.vgan_iforest_build_oblique, [p, 100, 4, p, p, 0, 2, 5, 64, 6, 3, 0, p, p, p, null], (0, 3, 4, 12, 13, 14),
         [(1, 1), (1, 63), (1, 1 << 31), (2, 0), (5, -1), (6, 0), (6, 65536), (7, 0), (7, outlier.IFOREST_MAX_TREES + 1), (8, 1),
          (8, outlier.IFOREST_MAX_SAMPLES + 1), (9, 5), (9, 7), (9, 0), (10, 1), (10, 0), (10, outlier.IFOREST_MAX_PLANE + 1)])
    # Xq, rows, d, nodes, plane_col, plane_w, first, count, T, psi, L, q, cq, sums, ld_sums, stream
    each(lib.vgan_iforest_path_sums_oblique, [p, 10, 4, p, p, p, 0, 2, 5, 64, 6, 3, p, p, 10, null], (0, 3, 4, 5, 12, 13),
         [(1, 0), (2, 0), (6, -1), (7, 0), (7, 65536), (8, 0), (8, 1025), (9, 1), (9, 1025), (10, 5), (10, 7), (11, 1), (11, 17),
          (14, 9)])
    for name, nargs in (("vgan_iforest_build_oblique", 16), ("vgan_iforest_path_sums_oblique", 16)):
        assert len(vgan_amd.lib.SIGNATURES[name][1]) == nargs
    assert callable(vgan_amd.ops.HipOps.iforest_build_oblique) and callable(vgan_amd.ops.HipOps.iforest_path_sums_oblique)
    assert vgan_amd.lib.ABI_VERSION == lib.vgan_abi_version() == 11
