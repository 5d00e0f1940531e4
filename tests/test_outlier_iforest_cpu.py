"""Isolation forest over the subspaces, CPU tier: the float64 / integer numpy restatement the GPU tests compare against,
pinned to sklearn (the average path length, and the scores of sklearn's own trees walked by the restated scorer), to a case
worked by hand and to the structural rules of the definition; and everything of vgan_amd.SubspaceIForest that runs without
a device (defaults, argument checks, the chunk rule, the dispatch from the model, the C ABI's argument checks).

The definition (SubspaceIForest's docstring): X as float32.  Tree (s, t) has the stream id = s T + t and the psi sample rows
feistel_perm(i, n, seed, id), i < psi.  Heap-numbered nodes, depth limit L = ceil(log2 psi).  A node of m rows at depth e is
a leaf if m <= 1, e == L or no feature of the subspace varies on its rows; otherwise the Philox words (w0, w1) of counter
(node, 0, 0x49464F52, 0) choose the j-th varying feature, j = (w0 c) >> 32, and p = float32(lo + u (hi - lo)), u = (w1 + 0.5)
2^-32, p >= hi replaced by lo; a row goes left iff x <= p.  A leaf of depth e and size m contributes (e << 32) + cq[m], cq[m] =
rint(c(m) 2^32); score = float32(exp2(-(sum / (T cq[psi]))))."""
import ctypes
import os
import re
from decimal import Decimal, getcontext

import numpy as np
import pytest

from conftest import REPO
from small_ops_ref import feistel_perm_ref, philox4x32_10
from test_outlier_ecod_cpu import _mask, tied_data

EULER_GAMMA = 0.5772156649015329
PHILOX_TAG = 0x49464F52


# ---- the restatement --------------------------------------------------------------------------------------------------
def restate_c(m):
    """float64: the average path length of an unsuccessful search among m rows; 0 for m <= 1, 1 for m = 2."""
    m = np.asarray(m, dtype=np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        c = 2.0 * (np.log(m - 1.0) + EULER_GAMMA) - 2.0 * (m - 1.0) / m
    return np.where(m <= 1, 0.0, np.where(m == 2, 1.0, c))


def restate_cq(psi):
    """int64 [psi + 1]: rint(c(m) 2^32)."""
    return np.rint(restate_c(np.arange(psi + 1)) * 2.0 ** 32).astype(np.int64)


def depth_limit(psi):
    return int(psi - 1).bit_length()  # ceil(log2 psi)


def restate_sample(n, psi, seed, stream):
    """int64 [psi], ascending: the sample rows of the tree with that stream id (only the set matters)."""
    return np.sort(feistel_perm_ref(np.arange(psi), n, seed, stream))


def node_words(node, seed, stream):
    """(w0, w1): the first two Philox4x32-10 words of a node of the tree with that stream id, as Python ints."""
    seed, stream = int(seed), int(stream)
    k0 = (seed & 0xFFFFFFFF) ^ (stream & 0xFFFFFFFF)
    k1 = (seed >> 32) ^ (stream >> 32) ^ 0x5bd1e995
    w = philox4x32_10((node, 0, PHILOX_TAG, 0), k0, k1)
    return int(w[0]), int(w[1])


def _canonical(X):
    return np.asarray(X, dtype=np.float32) + np.float32(0.0)  # -0.0 + 0.0 is +0.0


def restate_tree(X, feats, rows, L, seed, stream, members=None):
    """(feature int32 [N], threshold float32 [N], size int32 [N]) of one tree on the sample `rows` of X over the features
    `feats` (columns of X, ascending); N = 2^(L + 1).  members: a dict that receives node -> the rows reaching it."""
    Xc = _canonical(X)
    feats = np.asarray(feats)
    N = 2 << L
    feature = np.full(N, -2, np.int32)
    threshold = np.zeros(N, np.float32)
    size = np.zeros(N, np.int32)
    todo = [(1, 0, np.asarray(rows))]
    while todo:
        node, e, R = todo.pop()
        m = len(R)
        size[node], feature[node] = m, -1
        if members is not None:
            members[node] = R
        if m <= 1 or e == L:
            continue
        sub = Xc[np.ix_(R, feats)]
        lo, hi = sub.min(axis=0), sub.max(axis=0)
        varying = np.flatnonzero(lo != hi)
        if len(varying) == 0:
            continue
        w0, w1 = node_words(node, seed, stream)
        j = varying[(w0 * len(varying)) >> 32]
        u = (float(w1) + 0.5) * 2.0 ** -32  # exact
        lo64, hi64 = float(lo[j]), float(hi[j])
        p = np.float32(lo64 + u * (hi64 - lo64))  # Python floats: three separately rounded float64 operations
        if p >= hi[j]:
            p = lo[j]
        feature[node], threshold[node] = feats[j], p
        left = Xc[R, feats[j]] <= p  # float32 against float32
        todo.append((2 * node, e + 1, R[left]))
        todo.append((2 * node + 1, e + 1, R[~left]))
    return feature, threshold, size


def restate_forest(X, feats_list, T, psi, seed):
    """(feature, threshold, size), each [S, T, N]: the trees of every subspace, stream id = s T + t."""
    n, L = np.asarray(X).shape[0], depth_limit(psi)
    out = [restate_tree(X, feats, restate_sample(n, psi, seed, s * T + t), L, seed, s * T + t)
           for s, feats in enumerate(feats_list) for t in range(T)]
    return tuple(np.stack([o[k] for o in out]).reshape(len(feats_list), T, 2 << L) for k in range(3))


def restate_path_sums(feature, threshold, size, Xq, cq):
    """int64 [nq]: the total over the trees (feature, threshold, size: [T, N] heap arrays) of (depth << 32) + cq[leaf size]
    for every row of Xq.  The comparison x <= threshold is numpy's: float32 against a float32 threshold, float64 against a
    float64 one (sklearn's trees)."""
    Xq = np.asarray(Xq, dtype=np.float32)
    at = np.arange(Xq.shape[0])
    total = np.zeros(Xq.shape[0], np.int64)
    for f, thr, sz in zip(feature, threshold, size):
        node = np.ones(Xq.shape[0], np.int64)
        while True:
            inner = f[node] >= 0
            if not inner.any():
                break
            right = ~(Xq[at, np.maximum(f[node], 0)] <= thr[node])
            node = np.where(inner, 2 * node + right, node)
        depth = np.frexp(node.astype(np.float64))[1] - 1  # floor(log2 node)
        total += (depth.astype(np.int64) << 32) + cq[sz[node]]
    return total


def restate_score(sums, T, cq_psi):
    """float64: exp2(-(sum / (T cq[psi]))), before the rounding to float32."""
    return np.exp2(-(np.asarray(sums, dtype=np.float64) / float(T * int(cq_psi))))


def restate_iforest(X_fit, X_query, feats_list, T, max_samples, seed, forest=None):
    """(scores float64 [S, nq] before the rounding to float32, sums int64 [S, nq])."""
    n = np.asarray(X_fit).shape[0]
    psi = min(256 if max_samples == "auto" else max_samples, n)
    cq = restate_cq(psi)
    feature, threshold, size = restate_forest(X_fit, feats_list, T, psi, seed) if forest is None else forest
    sums = np.stack([restate_path_sums(feature[s], threshold[s], size[s], X_query, cq) for s in range(len(feats_list))])
    return restate_score(sums, T, cq[psi]), sums


def auc(scores, positive):
    """ROC AUC by the rank sum (ties share their mean rank)."""
    from scipy.stats import rankdata
    r = rankdata(scores)
    n1 = int(positive.sum())
    n0 = len(scores) - n1
    return (r[positive].sum() - n1 * (n1 + 1) / 2.0) / (n0 * n1)


def shifted_outliers(seed=5, n=2000, m=20, d=10):
    """float32 [n + m, d]: N(0, 1) inliers; the last m rows are moved out by 4 to 6 in three features each (the kind of
    outlier axis-parallel cuts isolate early), and the labels."""
    rng = np.random.default_rng(seed)
    X = rng.normal(size=(n + m, d))
    for i in range(n, n + m):
        f = rng.choice(d, 3, replace=False)
        X[i, f] = rng.uniform(4.0, 6.0, size=3) * rng.choice([-1.0, 1.0], size=3)
    y = np.zeros(n + m, bool)
    y[n:] = True
    return X.astype(np.float32), y


# ---- c(m) and its fixed-point image -----------------------------------------------------------------------------------
def test_average_path_length_is_sklearns():
    from sklearn.ensemble._iforest import _average_path_length
    m = np.arange(1025)
    np.testing.assert_allclose(restate_c(m), _average_path_length(m), rtol=0, atol=1e-12)
    assert restate_c(0) == 0 and restate_c(1) == 0 and restate_c(2) == 1


def test_cq_is_the_correctly_rounded_q32_image():
    """Against 50-digit decimal arithmetic: cq[m] is the integer nearest to c(m) 2^32 with gamma as the float64 constant."""
    getcontext().prec = 50
    cq = restate_cq(1024)
    assert cq.dtype == np.int64 and cq[0] == 0 and cq[1] == 0 and cq[2] == 1 << 32
    gamma, two32 = Decimal(EULER_GAMMA), Decimal(2) ** 32
    for m in range(3, 1025):
        exact = (2 * ((Decimal(m) - 1).ln() + gamma) - 2 * (Decimal(m) - 1) / Decimal(m)) * two32
        assert abs(Decimal(int(cq[m])) - exact) <= Decimal("0.5"), m
    from vgan_amd.outlier import iforest_path_table
    for psi in (2, 3, 256, 1024):
        np.testing.assert_array_equal(iforest_path_table(psi), cq[:psi + 1])


# ---- the restated scorer walks sklearn's own trees to sklearn's scores ---------------------------------------------------
def _heap_of(tree, L):
    """sklearn's tree_ as heap arrays (feature, float64 threshold, n_node_samples) of N = 2^(L + 1) slots."""
    N = 2 << L
    feature, threshold, size = np.full(N, -2, np.int32), np.zeros(N, np.float64), np.zeros(N, np.int32)
    todo = [(0, 1)]
    while todo:
        k, node = todo.pop()
        size[node] = tree.n_node_samples[k]
        if tree.children_left[k] < 0:
            feature[node] = -1
            continue
        feature[node], threshold[node] = tree.feature[k], tree.threshold[k]
        todo.append((tree.children_left[k], 2 * node))
        todo.append((tree.children_right[k], 2 * node + 1))
    return feature, threshold, size


def test_restated_scorer_gives_sklearns_scores_on_sklearns_trees():
    from sklearn.ensemble import IsolationForest
    X = np.random.default_rng(0).normal(size=(300, 6)).astype(np.float32)
    X[:, 5] = np.round(X[:, 5])  # ties
    T, psi = 8, 64
    model = IsolationForest(n_estimators=T, max_samples=psi, random_state=0).fit(X)
    L = depth_limit(psi)
    assert all(est.tree_.max_depth <= L for est in model.estimators_)
    heaps = [_heap_of(est.tree_, L) for est in model.estimators_]
    feature, threshold, size = (np.stack([h[k] for h in heaps]) for k in range(3))
    cq = restate_cq(psi)
    got = restate_score(restate_path_sums(feature, threshold, size, X, cq), T, cq[psi])
    np.testing.assert_allclose(got, -model.score_samples(X), rtol=0, atol=1e-8)
    assert got.min() > 0 and got.max() <= 1


# ---- a case worked by hand --------------------------------------------------------------------------------------------------
def test_hand_computed_case():
    """n = 4, d = 1, psi = 4, T = 1, seed 0: the sample is all four rows, L = 2, N = 8; X = (0, 1, 2, 10).  The words of the
    stream 0 (checked below against the Philox restatement, itself pinned in test_small_ops_cpu.py):

        node 1: w1 = 0xB56A4E5F -> u = 0.70865335...: p = float32(0 + u 10) = 7.0865335 -> rows {0, 1, 2} | {10}
        node 2: w1 = 0xD993D912 -> u = 0.84991223...: p = float32(0 + u 2)  = 1.6998245 -> rows {0, 1} | {2}
        node 4 is at depth 2 = L: a leaf of 2 rows.

    One feature: w0 chooses nothing.  Leaves: node 3 (depth 1, 1 row), node 4 (depth 2, 2 rows), node 5 (depth 2, 1 row).
    With c(1) = 0, c(2) = 1, c(4) = 2 (ln 3 + gamma) - 1.5 = 1.851655...: path lengths 3, 3, 2, 1 and scores 2^(-h / c(4))."""
    X = np.array([[0.0], [1.0], [2.0], [10.0]], np.float32)
    assert node_words(1, 0, 0)[1] == 0xB56A4E5F and node_words(2, 0, 0)[1] == 0xD993D912
    np.testing.assert_array_equal(restate_sample(4, 4, 0, 0), [0, 1, 2, 3])
    feature, threshold, size = restate_tree(X, [0], np.arange(4), 2, 0, 0)
    np.testing.assert_array_equal(feature, [-2, 0, 0, -1, -1, -1, -2, -2])
    np.testing.assert_array_equal(size, [0, 4, 3, 1, 2, 1, 0, 0])
    assert threshold[1] == np.float32((0xB56A4E5F + 0.5) / 2.0 ** 32 * 10.0)
    assert threshold[2] == np.float32((0xD993D912 + 0.5) / 2.0 ** 32 * 2.0)
    assert 7.0865 < threshold[1] < 7.0866 and 1.6998 < threshold[2] < 1.6999 and (threshold[3:] == 0).all()
    cq = restate_cq(4)
    sums = restate_path_sums(feature[None], threshold[None], size[None], X, cq)
    one = 1 << 32
    np.testing.assert_array_equal(sums, [3 * one, 3 * one, 2 * one, one])
    c4 = 2.0 * (np.log(3.0) + EULER_GAMMA) - 1.5
    assert abs(c4 - 1.851656) < 1e-6 and abs(int(cq[4]) - c4 * one) <= 0.5
    want = 2.0 ** (-np.array([3.0, 3.0, 2.0, 1.0]) / c4)
    np.testing.assert_allclose(restate_score(sums, 1, cq[4]), want, rtol=1e-9)
    per, _ = restate_iforest(X, X, [[0]], 1, 4, 0)
    np.testing.assert_allclose(per[0], want, rtol=1e-9)
    assert per[0, 3] > per[0, 2] > per[0, 1] == per[0, 0]  # the far row is the most outlying


# ---- structure of the restated trees ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,psi", [(2, 2), (3, 3), (100, 7), (300, 256), (300, 64)])
def test_restated_trees_obey_the_definition(n, psi):
    X = tied_data(n, 6, seed=n + psi)
    X[n // 2:] = X[:n - n // 2]  # duplicated rows
    Xc = _canonical(X)
    psi = min(psi, n)
    L = depth_limit(psi)
    for s, feats in enumerate([[0, 1, 2, 3, 4, 5], [3], [1, 2, 3], [0]]):
        for t in range(3):
            stream = s * 3 + t
            rows = restate_sample(n, psi, 7, stream)
            assert len(set(rows.tolist())) == psi and rows.min() >= 0 and rows.max() < n
            members = {}
            feature, threshold, size = restate_tree(X, feats, rows, L, 7, stream, members)
            assert size[1] == psi and feature[0] == -2 and size[0] == 0
            for node, R in members.items():
                e = node.bit_length() - 1
                assert e <= L and size[node] == len(R)
                sub = Xc[np.ix_(R, feats)]
                varies = sub.min(axis=0) != sub.max(axis=0) if len(R) else np.zeros(len(feats), bool)
                if feature[node] == -1:
                    assert len(R) <= 1 or e == L or not varies.any()
                    assert threshold[node] == 0 and (e == L or (feature[2 * node] == -2 and feature[2 * node + 1] == -2))
                    continue
                assert len(R) > 1 and e < L and feature[node] in feats and feature[node] != 3  # column 3 is constant
                col = Xc[R, feature[node]]
                assert col.min() <= threshold[node] < col.max()
                assert size[2 * node] >= 1 and size[2 * node + 1] >= 1 and size[2 * node] + size[2 * node + 1] == size[node]
                assert set(members[2 * node].tolist()) == set(R[col <= threshold[node]].tolist())
            absent = np.setdiff1d(np.arange(2 << L), list(members))
            assert (feature[absent] == -2).all() and (size[absent] == 0).all() and (threshold[absent] == 0).all()
            if feats == [3]:
                assert feature[1] == -1 and size[1] == psi  # a root leaf: nothing varies


def test_feature_choice_is_uniform_over_the_varying_features():
    """The root features of 2 000 trees (seed 11) over four varying features and a constant one: chi-square on the four cells
    below 16.27 (p = 0.001, 3 degrees of freedom), and the constant feature never.  (The varying columns are continuous: a
    tied column can be constant on a sample of 8 rows, and is then rightly not a candidate.)"""
    X = np.random.default_rng(1).normal(size=(40, 5)).astype(np.float32)  # continuous: four features vary on every sample
    X[:, 3] = 2.5
    counts = np.zeros(5)
    for stream in range(2000):
        feature, _, _ = restate_tree(X, [0, 1, 2, 3, 4], restate_sample(40, 8, 11, stream), 1, 11, stream)
        assert feature[1] >= 0
        counts[feature[1]] += 1
    assert counts[3] == 0 and counts.sum() == 2000
    cells = counts[[0, 1, 2, 4]]
    chi2 = float(((cells - 500.0) ** 2 / 500.0).sum())
    assert chi2 < 16.27, (cells, chi2)


def test_restatement_detects_what_sklearn_detects():
    """shifted_outliers (2 000 N(0, 1) rows in 10 features and 20 rows moved out by 4 to 6 in three features each), all ten
    features as one subspace, T = 100, psi = 256.  Measured here: sklearn's IsolationForest over random_state 0 .. 19 has
    ROC AUC mean 0.99928 and standard deviation 0.00045 (minimum 0.99833); the restatement with seed 0 has 0.99887.  The bar
    is sklearn's mean - 3 standard deviations, taken in the test."""
    from sklearn.ensemble import IsolationForest
    X, y = shifted_outliers()
    theirs = np.array([auc(-IsolationForest(n_estimators=100, max_samples=256, random_state=r).fit(X).score_samples(X), y)
                       for r in range(20)])
    per, _ = restate_iforest(X, X, [list(range(10))], 100, 256, 0)
    ours = auc(per[0], y)
    print(f"sklearn AUC mean {theirs.mean():.5f} std {theirs.std():.5f} min {theirs.min():.5f}; restatement {ours:.5f}")
    assert theirs.mean() > 0.99  # sklearn itself separates this recipe well
    assert ours >= theirs.mean() - 3.0 * theirs.std()


# ---- the class, without a device ----------------------------------------------------------------------------------------------
def test_constructor_and_argument_errors_touch_no_device():
    import vgan_amd
    from vgan_amd import outlier
    m = _mask(4, [[0, 1], [2, 3]])
    ens = vgan_amd.SubspaceIForest(m, [0.5, 0.5])
    assert (ens.n_estimators, ens.max_samples, ens.seed) == (100, "auto", 0)
    assert ens.ops is None and ens.workspace_bytes == outlier.DEFAULT_WORKSPACE_BYTES
    assert (ens.normalize, ens.combination, ens.contamination) == (None, "sum", 0.1)
    assert list(ens.plan.order) == [0, 1]  # the given order
    for name in ("n_neighbors", "engine", "splits", "max_features", "bootstrap"):
        assert not hasattr(ens, name)
        with pytest.raises(TypeError):
            vgan_amd.SubspaceIForest(m, [0.5, 0.5], **{name: 1})
    for bad in (0, 1025, -1, 2.0, True, None):
        with pytest.raises(ValueError, match="n_estimators"):
            vgan_amd.SubspaceIForest(m, [0.5, 0.5], n_estimators=bad)
    for bad in (1, 1025, 0.5, 256.0, "all", None, True):
        with pytest.raises(ValueError, match="max_samples"):
            vgan_amd.SubspaceIForest(m, [0.5, 0.5], max_samples=bad)
    for bad in (-1, 1 << 64, 0.0, "0", None):
        with pytest.raises(ValueError, match="seed"):
            vgan_amd.SubspaceIForest(m, [0.5, 0.5], seed=bad)
    ok = vgan_amd.SubspaceIForest(m, [0.5, 0.5], n_estimators=1024, max_samples=1024, seed=(1 << 64) - 1)
    assert (ok.n_estimators, ok.max_samples, ok.seed) == (1024, 1024, (1 << 64) - 1)
    assert vgan_amd.SubspaceIForest(m, [0.5, 0.5], n_estimators=1, max_samples=2).max_samples == 2
    with pytest.raises(ValueError, match="proba has 3 entries for 2 subspaces"):
        vgan_amd.SubspaceIForest(m, [0.5, 0.25, 0.25])
    with pytest.raises(ValueError, match="normalize"):
        vgan_amd.SubspaceIForest(m, [0.5, 0.5], normalize="l2")
    with pytest.raises(ValueError, match="combination"):
        vgan_amd.SubspaceIForest(m, [0.5, 0.5], combination="mean")
    with pytest.raises(ValueError, match="contamination"):
        vgan_amd.SubspaceIForest(m, [0.5, 0.5], contamination=0.7)
    with pytest.raises(ValueError, match="between 2 and"):
        ens.fit(np.zeros((1, 4), np.float32))
    with pytest.raises(ValueError, match="features"):
        ens.fit(np.zeros((5, 3), np.float32))

    class Tall:  # only its shape is looked at before the row check raises
        shape = (1 << 31, 4)

    with pytest.raises(ValueError, match="between 2 and"):
        ens.fit(Tall())
    assert ens.ops is None  # none of this touched the device
    for attr in ("tree_feature_", "tree_threshold_", "tree_size_"):
        with pytest.raises(RuntimeError, match="not fitted"):
            getattr(ens, attr)
    with pytest.raises(RuntimeError, match="not fitted"):
        ens.decision_function(np.zeros((5, 4), np.float32))
    doc = vgan_amd.SubspaceIForest.__doc__
    assert "max_features" in doc and "bootstrap" in doc and "pyod" in doc


def test_chunks_follow_the_documented_rule():
    from vgan_amd.outlier import iforest_chunks
    # 12 bytes per (subspace, row): an int64 sum and a float32 score
    assert iforest_chunks(5, 1 << 30) == (5, (1 << 30) // 60)
    assert iforest_chunks(5, 60) == (5, 1)  # single rows, every subspace
    assert iforest_chunks(5, 119) == (5, 1)
    assert iforest_chunks(5, 120) == (5, 2)
    assert iforest_chunks(5, 59) == (4, 1)
    assert iforest_chunks(5, 12) == (1, 1) and iforest_chunks(5, 0) == (1, 1)  # one subspace a range
    assert iforest_chunks(100_000, 1 << 30)[0] == 65535


def test_outlier_ensemble_routes_iforest_to_the_new_class():
    import vgan_amd
    model = vgan_amd.VGAN_no_kl(epochs=1)
    model.subspaces = _mask(6, [[0, 1], [2, 3, 5], [4]])
    model.proba = np.array([0.5, 0.3, 0.2])
    ens = model.outlier_ensemble(method="iforest")
    assert type(ens) is vgan_amd.SubspaceIForest and ens.n_estimators == 100 and ens.plan.count == 3
    np.testing.assert_array_equal(ens.proba, model.proba)
    ens = model.outlier_ensemble(method="iforest", n_neighbors=17, n_estimators=7, max_samples=64, seed=3, normalize="robust",
                                 combination="max", contamination=0.05, workspace_bytes=1 << 20)  # n_neighbors is ignored
    assert (ens.n_estimators, ens.max_samples, ens.seed, ens.normalize, ens.combination, ens.contamination,
            ens.workspace_bytes) == (7, 64, 3, "robust", "max", 0.05, 1 << 20)
    assert not hasattr(ens, "n_neighbors")
    with pytest.raises(TypeError):
        model.outlier_ensemble(method="iforest", engine="exact")  # not a keyword of SubspaceIForest
    with pytest.raises(TypeError):
        model.outlier_ensemble(method="iforest", max_features=0.5)
    assert "iforest" in vgan_amd.VGAN_no_kl.outlier_ensemble.__doc__
    assert "SubspaceIForest" in vgan_amd.__all__
    with pytest.raises(ValueError, match="method"):  # the neighbour ensemble still does not know it
        vgan_amd.SubspaceEnsemble(model.subspaces, model.proba, method="iforest")


# ---- C ABI: argument checks without a GPU -----------------------------------------------------------------------------------
def test_iforest_entries_reject_bad_arguments_without_gpu():
    import vgan_amd
    from vgan_amd import outlier
    lib = vgan_amd.lib.load()
    header = open(os.path.join(REPO, "include", "vgan_hip.h")).read()
    assert int(re.search(r"#define VGAN_IFOREST_MAX_SAMPLES (\d+)", header).group(1)) == outlier.IFOREST_MAX_SAMPLES
    assert int(re.search(r"#define VGAN_IFOREST_MAX_TREES (\d+)", header).group(1)) == outlier.IFOREST_MAX_TREES
    assert int(re.search(r"#define VGAN_IFOREST_MAX_DIMS (\d+)", header).group(1)) == outlier.IFOREST_MAX_DIMS
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

    # X, ldx, n, d, feat, feat_off, first, count, max_dims, T, psi, L, seed, nodes, stream
    each(lib.vgan_iforest_build, [p, 4, 100, 4, p, p, 0, 2, 3, 5, 64, 6, 0, p, null], (0, 4, 5, 13),
         [(1, 3), (2, 1), (2, 1 << 31), (2, 63), (3, 0), (6, -1), (7, 0), (8, 0), (8, 5), (8, outlier.IFOREST_MAX_DIMS + 1), (9, 0),
          (9, outlier.IFOREST_MAX_TREES + 1), (10, 1), (10, outlier.IFOREST_MAX_SAMPLES + 1), (11, 5), (11, 7), (11, 0)])
    # Xq, ldq, rows, d, nodes, first, count, T, psi, L, cq, sums, ld_sums, stream
    each(lib.vgan_iforest_path_sums, [p, 4, 10, 4, p, 0, 2, 5, 64, 6, p, p, 10, null], (0, 4, 10, 11),
         [(1, 3), (2, 0), (3, 0), (5, -1), (6, 0), (6, 65536), (7, 0), (7, 1025), (8, 1), (8, 1025), (9, 5), (9, 7), (12, 9)])
    # sums, ld_sums, count, rows, denom, score, ld_score, stream
    each(lib.vgan_iforest_scores, [p, 10, 2, 10, 1 << 32, p, 10, null], (0, 5),
         [(1, 9), (2, 0), (2, 65536), (3, 0), (4, 0), (4, -1), (6, 9)])
    for name, nargs in (("vgan_iforest_build", 15), ("vgan_iforest_path_sums", 14), ("vgan_iforest_scores", 8)):
        assert len(vgan_amd.lib.SIGNATURES[name][1]) == nargs
    assert vgan_amd.lib.ABI_VERSION == lib.vgan_abi_version() == 11
