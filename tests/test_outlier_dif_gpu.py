"""Deep isolation forest over the subspaces on the MI355X (csrc/outlier_dif.hip and the block entries of
csrc/outlier_iforest.hip through vgan_amd.SubspaceDIF and vgan_amd.ops), against the numpy restatement of
test_outlier_dif_cpu.py.

Weights are bit-equal to the restatement (one float64 product and one rounding on both sides).  The representation is compared
per element with the float64 net within the first-order bound documented in test_outlier_dif_cpu.py, on the case tables whose
teeth that file asserts.  Everything after the representation is exact: trees, path sums and scores are compared bit for bit
with the restated forest grown on the device's OWN representation (same matrix, same decisions), and R itself is bit-equal
across every split of the rows and the blocks over launches."""
import functools

import numpy as np
import pytest

from gemm_ref import worst_ratio
from test_outlier_dif_cpu import (CASE_BLOCKS, CASE_D, CASE_RANGE, CASE_SEED, PHILOX_CASES, STRUCTURED_CASES, case_features, case_matrix, corr,
                                  pack_weights, philox_case, restate_dif, restate_range, restate_weights, structured_case)
from test_outlier_ecod_cpu import _mask
from test_outlier_iforest_cpu import auc, depth_limit, restate_cq, restate_path_sums, restate_sample, restate_score, restate_tree
from test_outlier_norm_gpu import _check_scores

pytestmark = pytest.mark.gpu

R_NETS = 8  # representations per subspace in the op-level tests: blocks 3 and 4 are representations 3 and 4 of subspace 0


def _ops():
    from vgan_amd.ops import default_ops
    return default_ops()


def _dev(a):
    import torch
    return torch.as_tensor(np.ascontiguousarray(a), device="cuda")


def _table(feats_list):
    """(feat, feat_off, None) on the device for the subspaces given as feature lists."""
    feat = np.concatenate([np.asarray(f) for f in feats_list]).astype(np.int32)
    off = np.concatenate([[0], np.cumsum([len(f) for f in feats_list])]).astype(np.int32)
    return _dev(feat), _dev(off), None


def _scale(dims, hidden, q):
    widths = np.asarray(tuple(hidden) + (q,), dtype=np.float64)
    scale = np.empty((len(dims), len(widths)))
    scale[:, 0] = 1.0 / np.sqrt(np.asarray(dims, dtype=np.float64))
    scale[:, 1:] = 1.0 / np.sqrt(widths[:-1])
    return _dev(scale)


def _device_weights(table, d_s, hidden, q, first, count, seed, r=R_NETS):
    """(W, w_off) of vgan_dif_weights for `count` blocks of a one-subspace table."""
    import torch
    from vgan_amd.outlier import dif_block_floats
    size = int(dif_block_floats(d_s, hidden, q))
    W = torch.full((count * size,), float("nan"), dtype=torch.float32, device="cuda")  # the entry zeroes the pad columns itself
    w_off = _dev(np.arange(count, dtype=np.int64) * size)
    _ops().dif_weights(table[1], (r, tuple(hidden), q, 0), first, count, _scale([d_s], hidden, q), seed, W, w_off, count * size)
    return W, w_off


def _represent(X, table, lo, hi, hidden, q, activation, first, count, W, w_off, r=R_NETS):
    import torch
    from vgan_amd.outlier import DIF_ACTIVATIONS
    Xd = _dev(X)
    R = torch.full((count, Xd.shape[0], q), float("nan"), dtype=torch.float32, device="cuda")
    _ops().dif_represent(Xd, table, _dev(lo), _dev(hi), (r, tuple(hidden), q, DIF_ACTIVATIONS[activation]), first, count, W, w_off, R)
    return R.cpu().numpy()


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


# ---- 1. weights --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("hidden", [(), (1,), (3, 2), (65, 33)])
def test_weights_equal_the_restatement_bit_for_bit(hidden):
    """K_0 1, 3, 5 and 33 (no multiple of the 4 weights of a Philox call, rows that straddle calls), q 1, 3 and 20, two blocks
    starting at first = 3, and a seed that crosses the 32-bit halves of the key."""
    for d_s in (1, 3, 5, 33):
        table = _table([np.arange(d_s)])
        for q in (1, 3, 20):
            W, _ = _device_weights(table, d_s, hidden, q, CASE_BLOCKS[0], len(CASE_BLOCKS), CASE_SEED)
            want = np.concatenate([pack_weights(restate_weights(CASE_SEED, b, d_s, hidden, q)) for b in CASE_BLOCKS])
            np.testing.assert_array_equal(_bits(W.cpu().numpy()), _bits(want), err_msg=f"{d_s} {hidden} {q}")


# ---- 2. the representation ----------------------------------------------------------------------------------------------------
def test_representation_with_philox_weights_stays_within_the_bound():
    """Every case of PHILOX_CASES (rows 1 .. 130 across the 32-row tile, d_s 1 .. 65 across the 64-feature staging tile and
    scattered over 70 columns with a constant column and one whose minimum is -0.0, nets of 0 to 3 hidden layers, q 1 .. 64,
    both activations), two blocks in one launch: per element within the first-order bound of the float64 net."""
    worst = 0.0
    for rows, d_s, hidden, q, act in PHILOX_CASES:
        feats = case_features(d_s)
        table = _table([feats])
        W, w_off = _device_weights(table, d_s, hidden, q, CASE_BLOCKS[0], len(CASE_BLOCKS), CASE_SEED)
        got = _represent(case_matrix(rows), table, *CASE_RANGE, hidden, q, act, CASE_BLOCKS[0], len(CASE_BLOCKS), W, w_off)
        assert got.shape == (len(CASE_BLOCKS), rows, q) and np.isfinite(got).all()
        for k, block in enumerate(CASE_BLOCKS):
            _, _, _, want, bound = philox_case(rows, d_s, hidden, q, act, block)
            worst = max(worst, worst_ratio(got[k], want, bound))
    print(f"worst err / bound over {len(PHILOX_CASES)} cases: {worst:.3f}")


@pytest.mark.parametrize("kind,K", STRUCTURED_CASES)
def test_representation_with_structured_weights_at_k_edges(kind, K):
    """Layer-0 contractions of 127, 128, 129 and 784 (hidden = ()) and inner ones of 511 and 512 (relu after an all-positive
    layer), 33 rows, agreeing signs: every element within its bound, which sits below the smallest single term."""
    X, weights, hidden, act, want, bound, _, _ = structured_case(kind, K)
    d_s = X.shape[1]
    table = _table([np.arange(d_s)])
    W, w_off = _dev(pack_weights(weights)), _dev(np.zeros(1, np.int64))
    got = _represent(X, table, np.zeros(d_s, np.float32), np.ones(d_s, np.float32), hidden, want.shape[1], act, 0, 1, W, w_off, r=1)
    print(f"{kind} K = {K}: worst err / bound {worst_ratio(got[0], want, bound):.3f}")


# ---- 3. determinism ---------------------------------------------------------------------------------------------------------------
def test_representation_is_bit_equal_for_every_split_of_rows_and_blocks():
    d_s, hidden, q, act = 33, (65, 33), 20, "tanh"
    feats = case_features(d_s)
    table = _table([feats])
    X = case_matrix(130)
    W, w_off = _device_weights(table, d_s, hidden, q, 3, 2, CASE_SEED)
    whole = _represent(X, table, *CASE_RANGE, hidden, q, act, 3, 2, W, w_off)
    again = _represent(X, table, *CASE_RANGE, hidden, q, act, 3, 2, W, w_off)
    np.testing.assert_array_equal(_bits(whole), _bits(again))
    parts = [_represent(X[a:b], table, *CASE_RANGE, hidden, q, act, 3, 2, W, w_off) for a, b in ((0, 1), (1, 65), (65, 130))]
    np.testing.assert_array_equal(_bits(np.concatenate(parts, axis=1)), _bits(whole))
    for k, block in enumerate((3, 4)):  # one block at a time, with its own weight buffer
        W1, off1 = _device_weights(table, d_s, hidden, q, block, 1, CASE_SEED)
        alone = _represent(X, table, *CASE_RANGE, hidden, q, act, block, 1, W1, off1)
        np.testing.assert_array_equal(_bits(alone[0]), _bits(whole[k]))


# ---- 4. the block entries of the isolation forest -----------------------------------------------------------------------------------
def _split_nodes(nodes, L):
    """(feature, threshold, size) of raw int32 [..., N, 2] nodes, as the restatement states them."""
    feature = np.ascontiguousarray(nodes[..., 0])
    word = np.ascontiguousarray(nodes[..., 1])
    threshold = np.where(feature >= 0, word.view(np.float32), np.float32(0.0))
    size = np.where(feature == -1, word, 0).astype(np.int32)
    for e in range(L - 1, -1, -1):
        at = np.arange(1 << e, 2 << e)
        size[..., at] = np.where(feature[..., at] >= 0, size[..., 2 * at] + size[..., 2 * at + 1], size[..., at])
    return feature, threshold, size


@pytest.mark.parametrize("psi", [2, 100, 130])
def test_block_entries_equal_the_restated_forest_per_block(psi):
    """A given R [3, 130, 5] (ties, a constant column in block 1), first = 2, T = 4: nodes and sums bit-equal to the restated
    trees of each block with the stream ids b T + t; and vgan_iforest_build on a block's matrix alone, as subspace b of a table,
    grows the same trees."""
    import torch
    n, q, T, first, seed = 130, 5, 4, 2, 77
    rng = np.random.default_rng(psi)
    R = rng.normal(size=(3, n, q)).astype(np.float32)
    R[:, :, 2] = np.round(R[:, :, 2])  # ties
    R[1, :, 4] = 0.25
    R[2, :7, 0] = -0.0
    L, cq = depth_limit(psi), restate_cq(psi)
    N = 2 << L
    nodes = torch.full((first + 3, T, N, 2), -7, dtype=torch.int32, device="cuda")
    sums = torch.empty(3 * n, dtype=torch.int64, device="cuda")
    ops, Rd = _ops(), _dev(R)
    ops.iforest_build_blocks(Rd, first, psi, L, seed, nodes)
    ops.iforest_path_sums_blocks(Rd, nodes, first, psi, L, _dev(cq), sums)
    host = nodes.cpu().numpy()
    assert (host[:first] == -7).all()  # the blocks before `first` are not touched
    got_sums = sums.cpu().numpy().reshape(3, n)
    for z in range(3):
        b = first + z
        grown = [restate_tree(R[z], np.arange(q), restate_sample(n, psi, seed, b * T + t), L, seed, b * T + t) for t in range(T)]
        want = tuple(np.stack([g[k] for g in grown]) for k in range(3))
        got = _split_nodes(host[b], L)
        np.testing.assert_array_equal(got[0], want[0])
        np.testing.assert_array_equal(_bits(got[1]), _bits(want[1]))
        np.testing.assert_array_equal(got[2], want[2])
        np.testing.assert_array_equal(got_sums[z], restate_path_sums(*want, R[z], cq))
        # the subspace entry on this block's matrix alone: subspace b of b + 1 identical ones, so that its stream ids match
        table = _table([np.arange(q)] * (b + 1))
        alone = torch.full((b + 1, T, N, 2), -7, dtype=torch.int32, device="cuda")
        ops.iforest_build(_dev(R[z]), table, b, 1, q, psi, L, seed, alone)
        np.testing.assert_array_equal(alone.cpu().numpy()[b], host[b])


# ---- 5. the class, end to end ------------------------------------------------------------------------------------------------------
FEATS = [[0, 1, 2, 3, 4, 5, 6], [7], [2, 5, 8, 9, 10, 11]]  # subspace 1 is the constant column
KW = dict(n_representations=4, n_estimators=5, hidden=(16, 8), representation_dim=6, seed=21)
PROBA = np.array([0.5, 0.2, 0.3])


def _class_data(n, seed):
    X = np.random.default_rng(seed).normal(size=(n, 12)).astype(np.float32) * np.float32(40.0) + np.float32(100.0)  # pixel-like
    X[:, 7] = np.float32(3.0)
    X[:5, 9] = np.float32(-0.0)
    X[5:, 9] = np.abs(X[5:, 9])
    return X


@functools.lru_cache(maxsize=None)
def _fitted():
    import vgan_amd
    X = _class_data(300, 1)
    X.setflags(write=False)
    return X, vgan_amd.SubspaceDIF(_mask(12, FEATS), PROBA, **KW).fit(X)


def test_class_trees_sums_and_scores_equal_the_restated_forest_on_the_device_representation():
    X, ens = _fitted()
    Y = _class_data(70, 2)
    r, T, q = KW["n_representations"], KW["n_estimators"], KW["representation_dim"]
    lo, hi = restate_range(X)
    np.testing.assert_array_equal(_bits(ens.feature_min_), _bits(lo))
    np.testing.assert_array_equal(_bits(ens.feature_max_), _bits(hi))
    assert not np.signbit(ens.feature_min_[9]) and ens.max_samples_ == 256 and ens.depth_limit_ == 8
    assert ens.tree_feature_.shape == ens.tree_threshold_.shape == ens.tree_size_.shape == (3, r, T, 512)
    for s, j in ((0, 0), (2, 3)):  # the weights the class regenerates are the restated ones
        for got, want in zip(ens.layer_weights(s, j), restate_weights(KW["seed"], s * r + j, len(FEATS[s]), KW["hidden"], q)):
            np.testing.assert_array_equal(_bits(got), _bits(want))
    reps = {(which, s, j): ens.representation((X, Y)[which], s, j) for which in (0, 1) for s in range(3) for j in range(r)}
    assert all(v.dtype == np.float32 and v.shape == ((300, 70)[w], q) for (w, _, _), v in reps.items())
    assert not any(reps[0, 1, j].any() for j in range(r))  # constant features: R = 0
    want, pooled, trees = restate_dif(X, Y, FEATS, r, T, "auto", KW["hidden"], q, "tanh", KW["seed"], R_of=lambda w, s, j: reps[w, s, j])
    for s in range(3):
        for j in range(r):
            feature, threshold, size = trees[s * r + j]
            np.testing.assert_array_equal(ens.tree_feature_[s, j], feature)
            np.testing.assert_array_equal(_bits(ens.tree_threshold_[s, j]), _bits(threshold))
            np.testing.assert_array_equal(ens.tree_size_[s, j], size)
    np.testing.assert_array_equal(ens.path_sums(Y), pooled)
    got, per = ens.decision_function(Y, return_per_subspace=True)
    assert per.dtype == np.float32 and per.shape == (3, 70)
    np.testing.assert_array_equal(_bits(per), _bits(want.astype(np.float32)))
    assert (per[1] == np.float32(0.5)).all() and (per > 0).all() and (per <= 1).all()
    _check_scores(got, per, PROBA, None, None, "sum")
    # fit scored the training rows through the same trees
    fit_want, fit_pooled, _ = restate_dif(X, X, FEATS, r, T, "auto", KW["hidden"], q, "tanh", KW["seed"], R_of=lambda w, s, j: reps[0, s, j])
    np.testing.assert_array_equal(ens.path_sums(X), fit_pooled)
    np.testing.assert_array_equal(_bits(ens.per_subspace_scores_), _bits(fit_want.astype(np.float32)))
    cq = restate_cq(256)
    np.testing.assert_array_equal(_bits(ens.per_subspace_scores_), _bits(restate_score(fit_pooled, r * T, cq[256]).astype(np.float32)))
    assert (ens.per_subspace_scores_[1] == np.float32(0.5)).all()


def test_class_representation_stays_within_the_bound_of_the_float64_net():
    from test_outlier_dif_cpu import restate_representation, restate_scaling
    X, ens = _fitted()
    z = restate_scaling(X, *restate_range(X))
    for s, j in ((0, 1), (2, 2)):
        weights = restate_weights(KW["seed"], s * KW["n_representations"] + j, len(FEATS[s]), KW["hidden"], KW["representation_dim"])
        want, bound = restate_representation(z[:, FEATS[s]], weights, "tanh")
        worst_ratio(ens.representation(X, s, j), want, bound)


def test_class_is_bit_identical_for_every_workspace_and_run():
    import vgan_amd
    X, ens = _fitted()
    Y = _class_data(70, 2)
    dec = ens.decision_function(X)
    np.testing.assert_array_equal(dec, ens.decision_scores_)  # decision_function(X_train) == decision_scores_, bit for bit
    again = vgan_amd.SubspaceDIF(_mask(12, FEATS), PROBA, **KW).fit(X)
    # one block per chunk at fit (the workspace holds exactly one block's R), then single-row scoring chunks
    tight = vgan_amd.SubspaceDIF(_mask(12, FEATS), PROBA, workspace_bytes=300 * 6 * 4, **KW).fit(X)
    from vgan_amd.outlier import dif_chunks
    assert dif_chunks(tight._weight_bytes, 6, 300, tight.workspace_bytes, whole_rows=True) == (1, 300)
    for other in (again, tight):
        np.testing.assert_array_equal(other.decision_scores_, ens.decision_scores_)
        np.testing.assert_array_equal(_bits(other.per_subspace_scores_), _bits(ens.per_subspace_scores_))
        np.testing.assert_array_equal(other.tree_feature_, ens.tree_feature_)
        np.testing.assert_array_equal(_bits(other.tree_threshold_), _bits(ens.tree_threshold_))
    want, want_per = ens.decision_function(Y, return_per_subspace=True)
    tight.workspace_bytes = 1
    assert dif_chunks(tight._weight_bytes, 6, 70, 1) == (1, 1)
    got, got_per = tight.decision_function(Y, return_per_subspace=True)
    np.testing.assert_array_equal(got, want)
    np.testing.assert_array_equal(_bits(got_per), _bits(want_per))
    np.testing.assert_array_equal(_bits(tight.representation(Y, 2, 1)), _bits(ens.representation(Y, 2, 1)))
    with pytest.raises(ValueError, match="needs 7200 bytes"):
        vgan_amd.SubspaceDIF(_mask(12, FEATS), PROBA, workspace_bytes=7199, **KW).fit(X)


def test_shared_tail_two_rows_and_position_keyed_nets():
    import vgan_amd
    X, ens = _fitted()
    Y = _class_data(70, 2)
    tail = vgan_amd.SubspaceDIF(_mask(12, FEATS), PROBA, normalize="zscore", combination="max", contamination=0.2, **KW).fit(X)
    np.testing.assert_array_equal(_bits(tail.per_subspace_scores_), _bits(ens.per_subspace_scores_))  # the raw scores are the same
    got, per = tail.decision_function(Y, return_per_subspace=True)
    _check_scores(got, per, PROBA, tail.score_center_, tail.score_scale_, "max")
    assert tail.labels_.sum() == (tail.decision_scores_ > tail.threshold_).sum() and 0 < tail.labels_.sum() <= 0.2 * 300 + 1
    np.testing.assert_array_equal(tail.predict(Y), (got > tail.threshold_).astype(int))
    assert tail.predict_proba(Y).shape == (70, 2)
    # n = 2: psi = 2, L = 1
    two = vgan_amd.SubspaceDIF(_mask(12, FEATS), PROBA, **KW).fit(X[:2])
    assert two.max_samples_ == 2 and two.depth_limit_ == 1 and two.tree_feature_.shape == (3, 4, 5, 4)
    assert np.isfinite(two.decision_scores_).all() and (two.per_subspace_scores_[1] == np.float32(0.5)).all()
    np.testing.assert_array_equal(two.decision_function(X[:2]), two.decision_scores_)
    # the nets are keyed by the subspace's position: subspace 2 fitted alone is another detector
    alone = vgan_amd.SubspaceDIF(_mask(12, [FEATS[2]]), [1.0], **KW).fit(X)
    assert not np.array_equal(alone.per_subspace_scores_[0], ens.per_subspace_scores_[2])
    np.testing.assert_array_equal(_bits(alone.layer_weights(0, 1)[0]), _bits(restate_weights(KW["seed"], 1, 6, KW["hidden"], 6)[0]))
    # relu and a plain random projection run through the same path
    for kw in (dict(activation="relu"), dict(hidden=())):
        other = vgan_amd.SubspaceDIF(_mask(12, FEATS), PROBA, **{**KW, **kw}).fit(X)
        np.testing.assert_array_equal(other.decision_function(X), other.decision_scores_)
        assert (other.per_subspace_scores_[1] == np.float32(0.5)).all()


def test_nan_input_neither_faults_nor_hangs():
    import torch
    X, ens = _fitted()
    Y = _class_data(40, 3)
    Y[3, 2] = np.nan
    Y[7, :] = np.nan
    got = ens.decision_function(Y)
    torch.cuda.synchronize()
    assert got.shape == (40,)
    clean = np.delete(np.arange(40), [3, 7])
    np.testing.assert_array_equal(got[clean], ens.decision_function(Y[clean]))  # a row's score depends on that row alone


# ---- 6. detection on the device ---------------------------------------------------------------------------------------------------
def test_device_detector_finds_broken_correlations_like_the_restatement():
    """corr() (2 020 x 6, one subspace of all features, defaults, seed 0): the device's AUC is at least the restated detector's
    minus 0.005.  The two differ only where a float32 rounding of R flips a comparison in a tree."""
    import vgan_amd
    X, y = corr()
    ens = vgan_amd.SubspaceDIF(np.ones((1, 6), bool), [1.0]).fit(X)
    ours = auc(ens.per_subspace_scores_[0].astype(np.float64), y)
    scores, _, _ = restate_dif(X, X, [list(range(6))], 50, 6, "auto", (500, 100), 20, "tanh", 0)
    theirs = auc(scores[0], y)
    print(f"corr: device DIF AUC {ours:.5f}, restated DIF {theirs:.5f}")
    assert ours >= theirs - 0.005
