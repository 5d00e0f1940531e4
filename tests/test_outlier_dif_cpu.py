"""Deep isolation forest over the subspaces, CPU tier: the numpy restatement the GPU tests compare against (weights, scaling,
a float64 representation with its per-element error bound, and the whole detector: float64 net -> float32 R -> the restated
isolation trees of tests/test_outlier_iforest_cpu.py per block -> pooled score), the case tables of
tests/test_outlier_dif_gpu.py with the conditions that give their tolerances teeth, the detection bars against sklearn's
IsolationForest, and everything of vgan_amd.SubspaceDIF that runs without a device.

The definition (SubspaceDIF's docstring).  z = float32((double(x) - double(lo)) / (double(hi) - double(lo))), 0 for a constant
column.  Block b = s r + j has the layer sizes K_0 = d_s, hidden, q; W_l[o, i], e = o K_l + i, is float32((2 u - 1) c_l) with
u = (w + 0.5) 2^-32, w the word e & 3 of Philox4x32-10 at counter (lo32(e >> 2), hi32(e >> 2), 0x44494600 + l, 0) and key
(lo32(seed) ^ lo32(b), hi32(seed) ^ hi32(b) ^ 0x5bd1e995), c_l = 1 / sqrt(K_l) in float64.  No bias; tanh or relu after every
layer but the last.  T trees per block on R[b] with the stream id b T + t; score[s] = exp2(-(sum over the r blocks and their T
trees) / (r T cq[psi])).

Error bound of the representation (u = 2^-24, the unit roundoff of float32; per element, first order, nothing fitted to a device)
--------------------------------------------------------------------------------------------------------------------------------
The reference is the float64 net on the float32 z and float32 weights, both restated bit for bit, so E_0 = 0.
layer l        E <- E |W_l|^T + K_l 2u (|h| |W_l|^T)
    the error of the input passes through the linear map, and the float32 product of K_l terms in any order adds at most
    K_l u sum |h w| to first order (gemm_ref.py: each term passes through at most K_l roundings); factor 2: the project's margin.
tanh           E <- E + 2u
    tanh is 1-Lipschitz, so the incoming error is not amplified.  The device takes the float64 tanh of the float32
    pre-activation; the float64 tanh of the device library is taken as accurate to a few float64 ulp (not measured here), and
    the rounding to float32 costs at most u since |t| <= 1.  Factor 2 as above.
relu           nothing: 1-Lipschitz and exact.
Conditions asserted for every case of the GPU tables (test_case_tables_have_teeth): cap_ok, max(bound) <= 2e-2 max |want|
(gemm_ref.py's guard against a vacuous bound); and for the Philox-weight cases two mutants of the restatement -- the last term
of a layer dropped, a row taken from its neighbour -- move at least one row of every output column by more than its bound.
The dropped term is that of layer 0 (the staged K tail) in every case and that of each later layer in turn in the tanh cases:
the last unit of a relu layer may be 0 on every row, and dropping it then changes nothing -- the inner contractions under relu
are what the structured cases below are for.  At the pyod widths (500, 100) this worst-case bound is vacuous (cap ratio 0.08 to 0.25), so the long
contractions are checked with STRUCTURED weights fed to vgan_dif_represent: gemm_ref's agreeing signs and magnitudes in
[lo, 1] c, hidden = () for the K edges of layer 0, and relu after an all-positive first layer for the inner K edges (tanh
would saturate and hide a term); there every term is at least lo^2 c in magnitude and teeth() asserts max(bound) below it."""
import ctypes
import os
import re

import numpy as np
import pytest

from conftest import REPO
from gemm_ref import U, alt, cap_ok, draw, product_bound, rng_for, signs, teeth
from small_ops_ref import philox4x32_10
from test_outlier_ecod_cpu import _mask
from test_outlier_iforest_cpu import (auc, depth_limit, restate_cq, restate_path_sums, restate_sample, restate_score, restate_tree,
                                      shifted_outliers)

PHILOX_TAG = 0x44494600
M32 = 0xFFFFFFFF


# ---- the restatement --------------------------------------------------------------------------------------------------
def round8(k):
    return (int(k) + 7) // 8 * 8


def layer_sizes(d_s, hidden, q):
    """[(K_l, K_{l + 1})] of the net of a subspace of d_s features."""
    widths = [int(d_s)] + [int(w) for w in hidden] + [int(q)]
    return list(zip(widths[:-1], widths[1:]))


def weight_words(count, seed, b, layer):
    """uint64 [count]: the Philox words of the weights e = 0 .. count - 1 of a layer of block b."""
    seed, b = int(seed), int(b)
    g = np.arange((count + 3) // 4, dtype=np.uint64)
    k0 = (seed & M32) ^ (b & M32)
    k1 = (seed >> 32) ^ (b >> 32) ^ 0x5bd1e995
    w = philox4x32_10((g & np.uint64(M32), g >> np.uint64(32), PHILOX_TAG + layer, 0), k0, k1)
    return np.stack(w, axis=1).reshape(-1)[:count]


def restate_weights(seed, b, d_s, hidden, q):
    """The float32 [K_{l + 1}, K_l] weights of every layer of block b."""
    out = []
    for layer, (K, N) in enumerate(layer_sizes(d_s, hidden, q)):
        u = (weight_words(N * K, seed, b, layer).astype(np.float64) + 0.5) * 2.0 ** -32  # exact
        c = 1.0 / np.sqrt(np.float64(K))
        out.append(((2.0 * u - 1.0) * c).astype(np.float32).reshape(N, K))
    return out


def pack_weights(weights):
    """float32, flat: a block's layers as the library stores them: quad-major, [K_l rounded up to 8, in quads][K_{l + 1}][4], so
    that W[o, i] sits at ((i >> 2) K_{l + 1} + o) 4 + (i & 3), with zeros in the pad positions."""
    parts = []
    for W in weights:
        padded = np.zeros((W.shape[0], round8(W.shape[1])), np.float32)
        padded[:, :W.shape[1]] = W
        parts.append(padded.reshape(W.shape[0], -1, 4).transpose(1, 0, 2).reshape(-1))
    return np.concatenate(parts)


def restate_range(X):
    """(lo, hi) float32 [d]: the column min and max, -0.0 taken as +0.0."""
    Xc = np.asarray(X, dtype=np.float32) + np.float32(0.0)
    return Xc.min(axis=0), Xc.max(axis=0)


def restate_scaling(X, lo, hi):
    """float32 z: (double(x) - double(lo)) / (double(hi) - double(lo)) rounded once; a constant column gives exactly 0."""
    lo64, hi64 = np.asarray(lo, dtype=np.float64), np.asarray(hi, dtype=np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        z = ((np.asarray(X, dtype=np.float32).astype(np.float64) - lo64) / (hi64 - lo64)).astype(np.float32)
    return np.where(hi64 == lo64, np.float32(0.0), z)


def restate_representation(z, weights, activation, drop_last_of=None):
    """(R float64 [n, q], bound float64 [n, q]): the float64 net on the float32 z and weights, and the per-element error bound
    of the module docstring.  drop_last_of: the mutant that leaves the last term out of the products of that layer."""
    h = np.asarray(z, dtype=np.float32).astype(np.float64)
    err = np.zeros_like(h)
    for layer, W in enumerate(weights):
        w = np.asarray(W, dtype=np.float32).astype(np.float64)
        if drop_last_of == layer:
            w = w.copy()
            w[:, -1] = 0.0
        err = err @ np.abs(w).T + product_bound(np.abs(h), np.abs(w).T, w.shape[1])
        h = h @ w.T
        if layer + 1 < len(weights):
            if activation == "tanh":
                h, err = np.tanh(h), err + 2.0 * U
            else:
                h = np.maximum(h, 0.0)
    return h, err


def restate_dif(X_fit, X_query, feats_list, r, T, max_samples, hidden, q, activation, seed, R_of=None):
    """(scores float64 [S, nq] before the rounding to float32, pooled sums int64 [S, nq], trees): the whole detector.  R_of(which,
    s, j) -> float32 [n, q] replaces the restated representation of the fitted (which = 0) or the query rows (1): the GPU tier
    grows the restated forest on the device's own R."""
    X_fit, X_query = np.asarray(X_fit, dtype=np.float32), np.asarray(X_query, dtype=np.float32)
    n = X_fit.shape[0]
    psi = min(256 if max_samples == "auto" else max_samples, n)
    L, cq = depth_limit(psi), restate_cq(psi)
    lo, hi = restate_range(X_fit)
    z_fit, z_query = restate_scaling(X_fit, lo, hi), restate_scaling(X_query, lo, hi)
    pooled = np.zeros((len(feats_list), X_query.shape[0]), np.int64)
    trees = {}
    for s, feats in enumerate(feats_list):
        for j in range(r):
            b = s * r + j
            weights = restate_weights(seed, b, len(feats), hidden, q)
            if R_of is None:
                R_fit = restate_representation(z_fit[:, feats], weights, activation)[0].astype(np.float32)
                R_query = restate_representation(z_query[:, feats], weights, activation)[0].astype(np.float32)
            else:
                R_fit, R_query = R_of(0, s, j), R_of(1, s, j)
            grown = [restate_tree(R_fit, np.arange(q), restate_sample(n, psi, seed, b * T + t), L, seed, b * T + t) for t in range(T)]
            trees[b] = tuple(np.stack([g[k] for g in grown]) for k in range(3))
            pooled[s] += restate_path_sums(*trees[b], R_query, cq)
    return restate_score(pooled, r * T, cq[psi]), pooled, trees


def corr(seed=7, n=2000, m=20):
    """float32 [n + m, 6] and the labels: features 0 .. 3 are one latent N(0, 1) plus 0.1 noise each, features 4 .. 5 N(0, 1);
    the last m rows carry a latent of magnitude 1 to 2 with the sign flipped in two of the four correlated features, so every
    outlier sits inside every marginal range and breaks only the correlation."""
    rng = np.random.default_rng(seed)
    latent = rng.normal(size=n + m)
    latent[n:] = rng.uniform(1.0, 2.0, size=m) * rng.choice([-1.0, 1.0], size=m)
    X = np.empty((n + m, 6))
    X[:, :4] = latent[:, None] + 0.1 * rng.normal(size=(n + m, 4))
    X[:, 4:] = rng.normal(size=(n + m, 2))
    for i in range(n, n + m):
        X[i, rng.choice(4, 2, replace=False)] *= -1.0
    y = np.zeros(n + m, bool)
    y[n:] = True
    return X.astype(np.float32), y


# ---- the case tables of the GPU tier ----------------------------------------------------------------------------------------
CASE_D = 70
CASE_SEED = (1 << 63) + 5
ROWS = (1, 31, 32, 33, 130)
DIMS = (1, 3, 31, 33, 65)
HIDDENS = ((), (1,), (65, 33), (33, 65, 3))
QS = (1, 20, 64)
ACTIVATIONS = ("tanh", "relu")
PRODUCT = [(rows, d_s, hidden, q, act) for rows in ROWS for d_s in DIMS for hidden in HIDDENS for q in QS for act in ACTIVATIONS]
CASE_BLOCKS = (3, 4)  # two blocks starting at first = 3
STRUCTURED_CASES = [("first", 127), ("first", 128), ("first", 129), ("first", 784), ("inner", 511), ("inner", 512)]
STRUCTURED_ROWS, STRUCTURED_Q = 33, 20


def case_features(d_s):
    """d_s ascending columns of the CASE_D: scattered, with column 0 (constant) and column CASE_D - 1 (its minimum is -0.0)."""
    rng = rng_for(f"dif-features-{d_s}")
    if d_s == 1:
        return np.array([CASE_D - 1])
    inner = rng.choice(np.arange(1, CASE_D - 1), size=d_s - 2, replace=False)
    return np.sort(np.concatenate([[0, CASE_D - 1], inner]))


def case_matrix(rows):
    """float32 [rows, CASE_D] in [-3, 5) per column (a range that would saturate tanh unscaled); column 0 constant, column
    CASE_D - 1 non-negative with -0.0 in row 1 (row 0 is all a one-row case has).  The range used for the scaling is CASE_RANGE, that of the 130-row matrix, so
    that a one-row case is not all constant."""
    rng = rng_for("dif-matrix")
    X = rng.uniform(-3.0, 5.0, size=(max(ROWS), CASE_D)).astype(np.float32)
    X[:, 0] = np.float32(1.5)
    X[:, CASE_D - 1] = np.abs(X[:, CASE_D - 1])
    X[1, CASE_D - 1] = np.float32(-0.0)
    return X[:rows]


CASE_RANGE = restate_range(case_matrix(max(ROWS)))


def philox_case(rows, d_s, hidden, q, activation, block):
    """z restricted to the case's features, the weights of `block`, and want / bound of the representation."""
    feats = case_features(d_s)
    z = restate_scaling(case_matrix(rows), *CASE_RANGE)[:, feats]
    weights = restate_weights(CASE_SEED, block, d_s, hidden, q)
    want, bound = restate_representation(z, weights, activation)
    return feats, z, weights, want, bound


def structured_case(kind, K):
    """(X float32 [33, d_s] to be scaled with lo = 0 and hi = 1, i.e. taken as it is; the weights; hidden; activation; want;
    bound; the smallest magnitude a term of the edge layer can have).  first: hidden = (), d_s = K, gemm_ref's agreeing signs.
    inner: d_s = 1, hidden = (K,), relu; x and W_0 positive in [0.75, 1], so h is positive in [0.56, 1], and W_1 carries the
    sign of its output column."""
    rng = rng_for(f"dif-structured-{kind}-{K}")
    c = np.float32(1.0 / np.sqrt(K))
    lo = 0.5
    while True:
        if kind == "first":
            t = signs(rng, K)
            X = draw(rng, (STRUCTURED_ROWS, K), lo, alt(STRUCTURED_ROWS), t)
            weights = [(draw(rng, (STRUCTURED_Q, K), lo, alt(STRUCTURED_Q), t) * c).astype(np.float32)]
            hidden, activation, floor = (), "tanh", lo * lo * float(c)
        else:
            X = draw(rng, (STRUCTURED_ROWS, 1), 0.75)
            weights = [draw(rng, (K, 1), 0.75), (draw(rng, (STRUCTURED_Q, K), lo, alt(STRUCTURED_Q)) * c).astype(np.float32)]
            hidden, activation, floor = (K,), "relu", 0.75 * 0.75 * lo * float(c)
        want, bound = restate_representation(X, weights, activation)
        if np.max(bound) <= 2e-2 * np.abs(want).max() and np.max(bound) < floor:
            return X, weights, hidden, activation, want, bound, floor, lo
        assert lo == 0.5, "no structured draw meets cap_ok and teeth"
        lo = 0.9  # as gemm_ref.py does for its longest contractions


def moved_everywhere(mutant, want, bound):
    """the least, over the output columns, of the largest |mutant - want| / bound of a column: above 1 when the mutant moves at
    least one row of every column by more than its bound"""
    return float((np.abs(mutant - want) / np.maximum(bound, 1e-300)).max(axis=0).min())


def case_figures(case, block):
    """(cap ratio, least move of the dropped-term mutants, move of the neighbour-row mutant or None) of a Philox case."""
    rows, d_s, hidden, q, act = case
    _, z, weights, want, bound = philox_case(*case, block)
    top = np.abs(want).max()
    cap = float(np.max(bound) / top) if top > 0 else np.inf
    layers = range(len(weights) if act == "tanh" else 1)  # a relu unit may be dead on every row: see the module docstring
    drop = min(moved_everywhere(restate_representation(z, weights, act, drop_last_of=layer)[0], want, bound) for layer in layers)
    return cap, drop, (moved_everywhere(np.roll(want, 1, axis=0), want, bound) if rows > 1 else None)


def has_teeth(case):
    return all(cap <= 2e-2 and drop > 1.0 and (row is None or row > 1.0) for cap, drop, row in (case_figures(case, b) for b in CASE_BLOCKS))


# The GPU tier runs the cases of the product whose tolerance has teeth in the RESTATEMENT (nothing here looks at a device): with
# random weights a relu net of width 1 is dead on every row for some blocks (want = 0: no cap), and a single row, or 64 output
# columns behind a 3-wide layer, leave some column that a dropped term moves by less than its bound.  test_case_tables_have_teeth
# asserts that what is left still holds every value of every list with both activations, and most of the product.
PHILOX_CASES = [case for case in PRODUCT if has_teeth(case)]


# ---- weights --------------------------------------------------------------------------------------------------------------------
def test_weights_follow_the_definition_by_hand():
    seed, b, layer, K = (1 << 63) + 5, 3, 1, 5
    weights = restate_weights(seed, b, 3, (K,), 2)  # layer 1 is [2, 5]: e = 0 .. 9, three Philox calls
    k0 = (seed & M32) ^ b
    k1 = (seed >> 32) ^ 0x5bd1e995
    assert k0 == 5 ^ 3 and k1 == 0x80000000 ^ 0x5bd1e995  # the seed crosses the two halves of the key
    for e in (0, 3, 4, 9):
        words = philox4x32_10((e >> 2, 0, PHILOX_TAG + layer, 0), k0, k1)
        w = int(words[e & 3])
        u = (w + 0.5) / 4294967296.0
        want = np.float32((2.0 * u - 1.0) * (1.0 / np.sqrt(5.0)))
        assert weights[layer][e // K, e % K] == want, e
    # another block, another layer and another seed give other words
    assert not np.array_equal(restate_weights(seed, b + 1, 3, (K,), 2)[1], weights[1])
    assert not np.array_equal(restate_weights(seed + 1, b, 3, (K,), 2)[1], weights[1])
    assert not np.array_equal(restate_weights(seed, b, 5, (K,), 2)[0][:2, :], weights[1])  # layer 0 of [5, 5]: tag + 0
    assert [w.shape for w in restate_weights(0, 0, 7, (4, 3), 2)] == [(4, 7), (3, 4), (2, 3)]
    assert [w.shape for w in restate_weights(0, 0, 7, (), 2)] == [(2, 7)]


def test_weights_are_uniform_in_the_init_range():
    """10^5 weights of one layer, K = 400, so c = 0.05: all inside (-c, c); mean and variance against U(-c, c) within 4.5
    standard errors (two-sided 7e-6 each: mean 0 with standard error c / sqrt(3 n), variance c^2 / 3 with standard error
    c^2 sqrt(4 / (45 n))); and a chi-square over 20 equal cells below 43.82, the 0.999 quantile at 19 degrees of freedom."""
    K, N = 400, 250
    W = restate_weights(11, 17, K, (), N)[0].astype(np.float64).reshape(-1)
    n, c = W.size, 1.0 / np.sqrt(K)
    assert n == 100_000 and np.abs(W).max() < c
    assert abs(W.mean()) < 4.5 * c / np.sqrt(3.0 * n)
    assert abs(W.var() - c * c / 3.0) < 4.5 * c * c * np.sqrt(4.0 / (45.0 * n))
    cells = np.histogram(W, bins=20, range=(-c, c))[0]
    chi2 = float(((cells - n / 20.0) ** 2 / (n / 20.0)).sum())
    assert chi2 < 43.82, (cells, chi2)


def test_packed_layout_is_quad_major_with_zero_pads():
    from vgan_amd.outlier import dif_block_floats
    weights = restate_weights(0, 0, 33, (65, 3), 20)
    flat = pack_weights(weights)
    assert flat.size == 65 * 40 + 3 * 72 + 20 * 8 == int(dif_block_floats(33, (65, 3), 20))
    first = flat[:65 * 40].reshape(10, 65, 4)
    for o, i in ((0, 0), (64, 32), (17, 5), (3, 31)):
        assert first[i >> 2, o, i & 3] == weights[0][o, i] and flat[((i >> 2) * 65 + o) * 4 + (i & 3)] == weights[0][o, i]
    assert not first[8, :, 1:].any() and not first[9].any() and np.count_nonzero(first) == 65 * 33  # i = 33 .. 39 are pads
    np.testing.assert_array_equal(dif_block_floats(np.array([1, 8, 9]), (), 2), [16, 16, 32])


# ---- scaling --------------------------------------------------------------------------------------------------------------------
def test_scaling_follows_the_definition():
    X = np.array([[-0.0, 2.0, 1.0], [3.0, 2.0, -1.0], [1.0, 2.0, 0.5]], np.float32)
    lo, hi = restate_range(X)
    assert not np.signbit(lo[0]) and lo.tolist() == [0.0, 2.0, -1.0] and hi.tolist() == [3.0, 2.0, 1.0]
    z = restate_scaling(X, lo, hi)
    assert z[:, 1].tolist() == [0.0, 0.0, 0.0]  # a constant column gives exactly 0
    assert z[0, 0] == 0.0 and z[1, 0] == 1.0 and z[2, 0] == np.float32(1.0 / 3.0)
    new = restate_scaling(np.array([[6.0, 5.0, -3.0]], np.float32), lo, hi)  # new rows are not clipped
    assert new.tolist() == [[2.0, 0.0, -1.0]]


# ---- the bound and the case tables ------------------------------------------------------------------------------------------------
def test_bound_follows_the_documented_recursion():
    rng = np.random.default_rng(3)
    z = rng.uniform(0, 1, size=(4, 5)).astype(np.float32)
    W0, W1 = rng.uniform(-1, 1, size=(3, 5)).astype(np.float32), rng.uniform(-1, 1, size=(2, 3)).astype(np.float32)
    want, bound = restate_representation(z, [W0, W1], "tanh")
    z64, a0, a1 = z.astype(np.float64), np.abs(W0.astype(np.float64)), np.abs(W1.astype(np.float64))
    e0 = 5 * 2 * U * (np.abs(z64) @ a0.T) + 2 * U
    h = np.tanh(z64 @ W0.astype(np.float64).T)
    np.testing.assert_allclose(bound, e0 @ a1.T + 3 * 2 * U * (np.abs(h) @ a1.T), rtol=1e-14)
    np.testing.assert_allclose(want, h @ W1.astype(np.float64).T, rtol=1e-14)
    _, relu_bound = restate_representation(z, [W0, W1], "relu")
    hr = np.maximum(z64 @ W0.astype(np.float64).T, 0.0)
    np.testing.assert_allclose(relu_bound, (5 * 2 * U * (np.abs(z64) @ a0.T)) @ a1.T + 3 * 2 * U * (hr @ a1.T), rtol=1e-14)


def test_case_tables_have_teeth():
    """Every case of the GPU tables: the bound is not vacuous, and the mutants exceed it in every output column, for both blocks
    the GPU tier runs (first = 3)."""
    for act in ACTIVATIONS:
        kept = [c for c in PHILOX_CASES if c[4] == act]
        assert {c[0] for c in kept} == set(ROWS) and {c[1] for c in kept} == set(DIMS)
        assert {c[2] for c in kept} == set(HIDDENS) and {c[3] for c in kept} == set(QS)
        for hidden in HIDDENS:  # every net meets every row count and, unless a single relu unit is dead for a width, every width
            assert {c[0] for c in kept if c[2] == hidden} == set(ROWS)
            assert {c[1] for c in kept if c[2] == hidden} == set(DIMS) or (act, hidden) == ("relu", (1,))
    assert len(PHILOX_CASES) >= 0.8 * len(PRODUCT)
    figures = [case_figures(case, block) for case in PHILOX_CASES for block in CASE_BLOCKS]
    worst_cap, least_drop = max(f[0] for f in figures), min(f[1] for f in figures)
    least_row = min(f[2] for f in figures if f[2] is not None)
    assert worst_cap <= 2e-2 and least_drop > 1.0 and least_row > 1.0
    for rows, d_s, hidden, q, act in PHILOX_CASES:
        feats = case_features(d_s)
        assert feats[-1] == CASE_D - 1 and (d_s == 1 or feats[0] == 0) and len(set(feats)) == d_s and (np.diff(feats) > 0).all()
    print(f"philox cases: {len(PHILOX_CASES)} of {len(PRODUCT)}; worst cap ratio {worst_cap:.2e}, least dropped-term move "
          f"{least_drop:.1f} bounds, least row move {least_row:.1f}")
    for kind, K in STRUCTURED_CASES:
        X, weights, hidden, act, want, bound, floor, lo = structured_case(kind, K)
        ratio, bite = cap_ok(bound, want), teeth(bound, lo, floor)
        edge = len(weights) - 1
        assert weights[edge].shape[1] == K
        mutant = restate_representation(X, weights, act, drop_last_of=edge)[0]
        assert (np.abs(mutant - want) > bound).all()  # agreeing signs: EVERY element moves by more than its bound
        assert (np.abs(np.roll(want, 1, axis=0) - want) > bound).all()
        print(f"structured {kind} K = {K}: lo {lo}, cap ratio {ratio:.2e}, bound / smallest term {bite:.2e}")


def test_documented_figures_of_the_bound():
    """d_s = 33, hidden (65, 33), q = 20, 130 rows, uniform weights, inputs in [0, 1): the cap ratio is of the order 4e-4 and
    the dropped-term mutant exceeds the bound many times over in every column; at widths (500, 100) the bound is vacuous."""
    rng = np.random.default_rng(0)
    z = rng.uniform(0, 1, size=(130, 33)).astype(np.float32)
    weights = restate_weights(0, 0, 33, (65, 33), 20)
    want, bound = restate_representation(z, weights, "tanh")
    assert cap_ok(bound, want) < 2e-3
    assert moved_everywhere(restate_representation(z, weights, "tanh", drop_last_of=0)[0], want, bound) > 5.0
    zw = rng.uniform(0, 1, size=(64, 784)).astype(np.float32)
    wide = restate_weights(0, 0, 784, (500, 100), 20)
    want, bound = restate_representation(zw, wide, "tanh")
    assert np.max(bound) / np.abs(want).max() > 2e-2  # why the long-K cases use structured weights


# ---- detection --------------------------------------------------------------------------------------------------------------------
def sklearn_aucs(X, y, states=20):
    from sklearn.ensemble import IsolationForest
    return np.array([auc(-IsolationForest(n_estimators=100, max_samples=256, random_state=r).fit(X).score_samples(X), y)
                     for r in range(states)])


def restated_default_auc(X, y):
    scores, _, _ = restate_dif(X, X, [list(range(X.shape[1]))], 50, 6, "auto", (500, 100), 20, "tanh", 0)
    return auc(scores[0], y)


def test_restatement_finds_broken_correlations_before_the_isolation_forest():
    """corr(): 2 000 rows in 6 features, 20 outliers that break the correlation of features 0 .. 3 inside every marginal range.
    The restated DIF at its defaults and seed 0 must reach sklearn IsolationForest's mean + 3 standard deviations over
    random_state 0 .. 19 (100 trees, psi 256); both are computed and printed here."""
    X, y = corr()
    theirs = sklearn_aucs(X, y)
    ours = restated_default_auc(X, y)
    print(f"corr: sklearn IsolationForest AUC mean {theirs.mean():.5f} std {theirs.std():.5f} max {theirs.max():.5f}; restated DIF {ours:.5f}")
    assert ours >= theirs.mean() + 3.0 * theirs.std()


def test_restatement_keeps_what_the_isolation_forest_detects():
    """shifted_outliers() of the isolation forest's tests: at least sklearn's mean - 3 standard deviations."""
    X, y = shifted_outliers()
    theirs = sklearn_aucs(X, y)
    ours = restated_default_auc(X, y)
    print(f"shifted: sklearn IsolationForest AUC mean {theirs.mean():.5f} std {theirs.std():.5f}; restated DIF {ours:.5f}")
    assert ours >= theirs.mean() - 3.0 * theirs.std()


def test_restated_detector_pools_and_degenerates_as_documented():
    rng = np.random.default_rng(1)
    X = rng.normal(size=(40, 5)).astype(np.float32)
    X[:, 3] = 2.0
    scores, pooled, trees = restate_dif(X, X, [[0, 1, 4], [3]], 3, 2, 16, (4,), 3, "tanh", 9)
    assert (scores[1] == 0.5).all()  # constant features: R = 0, one leaf of psi rows per tree
    cq = restate_cq(16)
    assert (pooled[1] == 3 * 2 * cq[16]).all()
    assert all((trees[b][0][:, 1] == -1).all() and (trees[b][2][:, 1] == 16).all() for b in (3, 4, 5))
    assert 0.0 < scores[0].min() and scores[0].max() <= 1.0 and len(set(scores[0])) > 10
    alone, _, _ = restate_dif(X, X, [[3], [0, 1, 4]], 3, 2, 16, (4,), 3, "tanh", 9)
    assert not np.array_equal(alone[1], scores[0])  # the nets are keyed by the subspace's position


# ---- the class, without a device ----------------------------------------------------------------------------------------------
def test_constructor_and_argument_errors_touch_no_device():
    import vgan_amd
    from vgan_amd import outlier
    m = _mask(4, [[0, 1], [2, 3]])
    ens = vgan_amd.SubspaceDIF(m, [0.5, 0.5])
    assert (ens.n_representations, ens.n_estimators, ens.max_samples, ens.hidden, ens.representation_dim, ens.activation,
            ens.seed) == (50, 6, "auto", (500, 100), 20, "tanh", 0)
    assert ens.ops is None and ens.workspace_bytes == outlier.DEFAULT_WORKSPACE_BYTES
    assert (ens.normalize, ens.combination, ens.contamination) == (None, "sum", 0.1)
    assert list(ens.plan.order) == [0, 1]  # the given order
    for name in ("n_neighbors", "engine", "skip_connection", "batch_size", "device"):
        assert not hasattr(ens, name)
        with pytest.raises(TypeError):
            vgan_amd.SubspaceDIF(m, [0.5, 0.5], **{name: 1})
    for bad in (0, 257, -1, 2.0, True, None):
        with pytest.raises(ValueError, match="n_representations"):
            vgan_amd.SubspaceDIF(m, [0.5, 0.5], n_representations=bad)
    for bad in (0, 1025, 2.0, None):
        with pytest.raises(ValueError, match="n_estimators"):
            vgan_amd.SubspaceDIF(m, [0.5, 0.5], n_estimators=bad)
    for bad in (1, 1025, 0.5, "all", None):
        with pytest.raises(ValueError, match="max_samples"):
            vgan_amd.SubspaceDIF(m, [0.5, 0.5], max_samples=bad)
    for bad in ((0,), (513,), (4, 4, 4, 4), (4.0,), (True,), 500, None, ("a",)):
        with pytest.raises(ValueError, match="hidden"):
            vgan_amd.SubspaceDIF(m, [0.5, 0.5], hidden=bad)
    for bad in (0, 65, 2.0, None, True):
        with pytest.raises(ValueError, match="representation_dim"):
            vgan_amd.SubspaceDIF(m, [0.5, 0.5], representation_dim=bad)
    for bad in ("sigmoid", "leaky_relu", None, 0):
        with pytest.raises(ValueError, match="activation"):
            vgan_amd.SubspaceDIF(m, [0.5, 0.5], activation=bad)
    for bad in (-1, 1 << 64, 0.0, None):
        with pytest.raises(ValueError, match="seed"):
            vgan_amd.SubspaceDIF(m, [0.5, 0.5], seed=bad)
    ok = vgan_amd.SubspaceDIF(m, [0.5, 0.5], n_representations=256, n_estimators=1024, max_samples=1024, hidden=[512, 1, 512],
                              representation_dim=64, activation="relu", seed=(1 << 64) - 1)
    assert (ok.n_representations, ok.hidden, ok.representation_dim, ok.activation) == (256, (512, 1, 512), 64, "relu")
    assert vgan_amd.SubspaceDIF(m, [0.5, 0.5], hidden=()).hidden == ()
    with pytest.raises(ValueError, match="proba has 3 entries for 2 subspaces"):
        vgan_amd.SubspaceDIF(m, [0.5, 0.25, 0.25])
    with pytest.raises(ValueError, match="normalize"):
        vgan_amd.SubspaceDIF(m, [0.5, 0.5], normalize="l2")
    with pytest.raises(ValueError, match="combination"):
        vgan_amd.SubspaceDIF(m, [0.5, 0.5], combination="mean")
    with pytest.raises(ValueError, match="contamination"):
        vgan_amd.SubspaceDIF(m, [0.5, 0.5], contamination=0.7)
    with pytest.raises(ValueError, match="between 2 and"):
        ens.fit(np.zeros((1, 4), np.float32))
    with pytest.raises(ValueError, match="features"):
        ens.fit(np.zeros((5, 3), np.float32))

    class Tall:  # only its shape is looked at before the row check raises
        shape = ((1 << 24) + 1, 4)

    with pytest.raises(ValueError, match="between 2 and"):
        ens.fit(Tall())
    small = vgan_amd.SubspaceDIF(m, [0.5, 0.5], representation_dim=6, workspace_bytes=7199)
    with pytest.raises(ValueError, match="needs 7200 bytes"):  # one block's R: 300 rows x 6 columns x 4 bytes
        small.fit(np.zeros((300, 4), np.float32))
    assert ens.ops is None and small.ops is None  # none of this touched the device
    for attr in ("tree_feature_", "tree_threshold_", "tree_size_"):
        with pytest.raises(RuntimeError, match="not fitted"):
            getattr(ens, attr)
    with pytest.raises(RuntimeError, match="not fitted"):
        ens.decision_function(np.zeros((5, 4), np.float32))
    with pytest.raises(RuntimeError, match="not fitted"):
        ens.representation(np.zeros((5, 4), np.float32), 0, 0)
    with pytest.raises(ValueError, match="no representation"):
        ens.layer_weights(2, 0)
    doc = vgan_amd.SubspaceDIF.__doc__
    for word in ("DEAS", "skip_connection", "pyod", "ring", "POSITION", "exactly 0.5", "0x44494600", "not clipped", "NaN"):
        assert word in doc, word


def test_chunks_follow_the_documented_rule():
    from vgan_amd.outlier import dif_chunks
    # per block: its weights, and per row q float32 of R and an int64 sum
    assert dif_chunks(1000, 20, 100, 1 << 22) == ((1 << 22) // (1000 + 100 * 88), 100)
    assert dif_chunks(1000, 20, 100, 2 * 9800) == (2, 100) and dif_chunks(1000, 20, 100, 2 * 9800 - 1) == (1, 100)
    assert dif_chunks(1000, 20, 100, 9799) == (1, 99)  # one block a chunk, the rows chunked
    assert dif_chunks(1000, 20, 100, 1000 + 2 * 88) == (1, 2) and dif_chunks(1000, 20, 100, 1000 + 2 * 88 - 1) == (1, 1)
    assert dif_chunks(1000, 20, 100, 0) == (1, 1)  # single rows
    assert dif_chunks(8, 1, 2, 1 << 40)[0] == 65535  # a grid dimension
    # fit grows a block's trees on its whole R: the rows are never chunked, and R itself must fit
    assert dif_chunks(1000, 20, 100, 8000, whole_rows=True) == (1, 100)
    assert dif_chunks(1000, 20, 100, 3 * 9800, whole_rows=True) == (3, 100)
    with pytest.raises(ValueError, match="needs 8000 bytes"):
        dif_chunks(1000, 20, 100, 7999, whole_rows=True)


def test_outlier_ensemble_routes_dif_to_the_new_class():
    import vgan_amd
    model = vgan_amd.VGAN_no_kl(epochs=1)
    model.subspaces = _mask(6, [[0, 1], [2, 3, 5], [4]])
    model.proba = np.array([0.5, 0.3, 0.2])
    ens = model.outlier_ensemble(method="dif")
    assert type(ens) is vgan_amd.SubspaceDIF and ens.n_representations == 50 and ens.plan.count == 3
    np.testing.assert_array_equal(ens.proba, model.proba)
    ens = model.outlier_ensemble(method="dif", n_neighbors=17, n_representations=4, n_estimators=7, max_samples=64, hidden=(16,),
                                 representation_dim=5, activation="relu", seed=3, normalize="robust", combination="max",
                                 contamination=0.05, workspace_bytes=1 << 20)  # n_neighbors is ignored
    assert (ens.n_representations, ens.n_estimators, ens.max_samples, ens.hidden, ens.representation_dim, ens.activation, ens.seed,
            ens.normalize, ens.combination, ens.contamination, ens.workspace_bytes) == (4, 7, 64, (16,), 5, "relu", 3, "robust", "max",
                                                                                         0.05, 1 << 20)
    assert not hasattr(ens, "n_neighbors")
    with pytest.raises(TypeError):
        model.outlier_ensemble(method="dif", engine="exact")  # not a keyword of SubspaceDIF
    assert '"dif"' in vgan_amd.VGAN_no_kl.outlier_ensemble.__doc__
    assert "SubspaceDIF" in vgan_amd.__all__
    with pytest.raises(ValueError, match="method"):  # the neighbour ensemble still does not know it
        vgan_amd.SubspaceEnsemble(model.subspaces, model.proba, method="dif")


# ---- C ABI: argument checks without a GPU -----------------------------------------------------------------------------------
def test_dif_entries_reject_bad_arguments_without_gpu():
    import vgan_amd
    from vgan_amd import outlier
    lib = vgan_amd.lib.load()
    header = open(os.path.join(REPO, "include", "vgan_hip.h")).read()
    for name, value in (("MAX_NETS", outlier.DIF_MAX_REPRESENTATIONS), ("MAX_HIDDEN", outlier.DIF_MAX_HIDDEN),
                        ("MAX_WIDTH", outlier.DIF_MAX_WIDTH), ("MAX_OUT", outlier.DIF_MAX_DIM), ("MAX_ROWS", outlier.DIF_MAX_ROWS),
                        ("ROW_TILE", outlier.DIF_ROW_TILE), ("K_TILE", outlier.DIF_K_TILE), ("ACT_TANH", outlier.DIF_ACTIVATIONS["tanh"]),
                        ("ACT_RELU", outlier.DIF_ACTIVATIONS["relu"])):
        assert int(re.search(rf"#define VGAN_DIF_{name} (\d+)", header).group(1)) == value, name
    null = None
    buf = ctypes.create_string_buffer(256)
    p = ctypes.cast(ctypes.addressof(buf) + (-ctypes.addressof(buf)) % 16, ctypes.c_void_p)  # never read
    odd = ctypes.c_void_p(p.value + 4)

    def widths(*w):
        return (ctypes.c_int32 * 4)(*w)

    def rejected(rc, source):
        msg = lib.vgan_last_error()
        return rc == 1 and b"bad argument" in msg and source in msg

    def each(fn, source, good, pointers, bad_values):
        for pos in pointers:
            assert rejected(fn(*[null if i == pos else v for i, v in enumerate(good)]), source), pos
        for pos, bad in bad_values:
            assert rejected(fn(*[bad if i == pos else v for i, v in enumerate(good)]), source), (pos, bad)

    hidden_bad = [(5, widths(0, 4)), (5, widths(4, 513)), (5, widths(-1, 4))]
    # feat_off, r, first, count, n_hidden, hidden, q, scale, seed, W, w_off, total, stream
    each(lib.vgan_dif_weights, b"outlier_dif.hip", [p, 2, 0, 2, 2, widths(4, 3), 5, p, 0, p, p, 100, null], (0, 5, 7, 9, 10),
         [(1, 0), (1, 257), (2, -1), (3, 0), (3, 65536), (4, -1), (4, 4), (6, 0), (6, 65), (9, odd), (11, 0)] + hidden_bad)
    # X, ldx, rows, d, feat, feat_off, lo, hi, r, first, count, n_hidden, hidden, q, activation, W, w_off, R, stream
    each(lib.vgan_dif_represent, b"outlier_dif.hip", [p, 4, 10, 4, p, p, p, p, 2, 0, 2, 2, widths(4, 3), 5, 0, p, p, p, null],
         (0, 4, 5, 6, 7, 12, 15, 16, 17),
         [(1, 3), (2, 0), (2, (1 << 24) + 1), (3, 0), (8, 0), (8, 257), (9, -1), (10, 0), (10, 65536), (11, -1), (11, 4), (13, 0), (13, 65),
          (14, 2), (14, -1), (15, odd)] + [(12, w) for _, w in hidden_bad])
    assert lib.vgan_dif_represent(p, 4, 10, 4, p, p, p, p, 2, 0, 2, 0, null, 5, 0, p, p, null, null) == 1  # hidden may be NULL only at 0: R is what is missing
    # R, block_stride, n, q, first, count, T, psi, L, seed, nodes, stream
    each(lib.vgan_iforest_build_blocks, b"outlier_iforest.hip", [p, 500, 100, 5, 0, 2, 4, 64, 6, 0, p, null], (0, 10),
         [(1, 499), (2, 1), (2, 1 << 31), (2, 63), (3, 0), (3, 8193), (4, -1), (5, 0), (6, 0), (6, 1025), (7, 1), (7, 1025), (8, 5), (8, 7),
          (8, 0)])
    # Rq, block_stride, rows, q, nodes, first, count, T, psi, L, cq, sums, ld_sums, stream
    each(lib.vgan_iforest_path_sums_blocks, b"outlier_iforest.hip", [p, 50, 10, 5, p, 0, 2, 4, 64, 6, p, p, 10, null], (0, 4, 10, 11),
         [(1, 49), (2, 0), (3, 0), (3, 8193), (5, -1), (6, 0), (6, 65536), (7, 0), (7, 1025), (8, 1), (8, 1025), (9, 5), (9, 7), (12, 9)])
    for name, nargs in (("vgan_dif_weights", 13), ("vgan_dif_represent", 19), ("vgan_iforest_build_blocks", 12),
                        ("vgan_iforest_path_sums_blocks", 14)):
        assert len(vgan_amd.lib.SIGNATURES[name][1]) == nargs
    assert vgan_amd.lib.ABI_VERSION == lib.vgan_abi_version() == 11
