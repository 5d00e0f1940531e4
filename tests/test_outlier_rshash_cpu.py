"""RS-Hash over the subspaces, CPU tier: the float64 / integer numpy restatement the GPU tests compare against, pinned to a
case worked by hand, to an independent count of the cells (numpy.unique on the digit vectors, so the key packing is not
trusted), to the stated formulas of the host draws and of the log table, and to a detection recipe; and everything of
vgan_amd.SubspaceRSHash that runs without a device (defaults, argument checks, the dispatch, the C ABI's argument checks).

The definition (SubspaceRSHash's docstring): X as float32.  The candidates of a subspace are its features whose maximum
exceeds their minimum over the fitted rows.  Component (z, t) draws f, r, r positions among the candidates and r shifts alpha
(rshash_components), samples the s rows feistel_perm(i, n, seed, z T + t), i < s, takes the float32 min and max of each chosen
feature over the sample (-0.0 as +0.0), and counts the sample's cells: digit = clamp(floor(((x - mn) / w + alpha) / f), -1,
floor(1 / f) + 2) + 1 in float64 ((x - mn) / w is 0 where w = 0), key = sum_j digit_j R^j, R = floor(1 / f) + 4.  A row's c_t
is the count of its cell plus 1 (at fit: not for a row of the sample); sum = sum_t table[c_t], table[c] = rint(log2(c) 2^32);
score = float32(1 - sum / (T table[s + 1]))."""
import ctypes
import math
import os
import re
from types import SimpleNamespace

import numpy as np
import pytest

from conftest import REPO
from small_ops_ref import feistel_perm_ref
from test_outlier_dif_cpu import corr
from test_outlier_ecod_cpu import _mask, tied_data
from test_outlier_hist_cpu import restate_hbos
from test_outlier_iforest_cpu import auc

MAX_DIMS = 12
PAD_KEY = np.uint64(0xFFFFFFFFFFFFFFFF)


# ---- the restatement --------------------------------------------------------------------------------------------------
def _canonical(X):
    return np.asarray(X, dtype=np.float32) + np.float32(0.0)  # -0.0 + 0.0 is +0.0


def restate_log_table(s):
    """int64 [s + 2]: rint(log2(c) 2^32), entry 0 (never used) 0."""
    return np.concatenate([[0], np.rint(np.log2(np.arange(1, s + 2, dtype=np.float64)) * 2.0 ** 32)]).astype(np.int64)


def restate_samples(max_samples, n):
    return min(1000 if max_samples == "auto" else max_samples, n)


def restate_components(candidate_counts, T, s, seed):
    """[[(f, positions int64 [r], alpha float64 [r]) per component] per subspace]: the draws in the stated order from one
    generator; a subspace without candidates draws nothing and has no component."""
    rng = np.random.default_rng(seed)
    lo = 1.0 / np.sqrt(float(s))
    hi = 1.0 - lo
    out = []
    for c in candidate_counts:
        comps = []
        for _ in range(T if c > 0 else 0):
            f = lo + (hi - lo) * rng.random()
            L = np.log(float(s)) / np.log(max(2.0, 1.0 / f))
            r_lo = int(np.floor(1.0 + L / 2.0))
            r_hi = max(r_lo, int(np.floor(L)))
            r = min(int(rng.integers(r_lo, r_hi + 1)), int(c))
            positions = np.sort(rng.choice(int(c), r, replace=False))
            comps.append((f, positions, f * rng.random(r)))
        out.append(comps)
    return out


def restate_candidates(X, feats_list):
    """Per subspace its features (ascending) whose maximum exceeds their minimum over all rows of X."""
    Xc = _canonical(X)
    lo, hi = Xc.min(axis=0), Xc.max(axis=0)
    return [np.asarray([f for f in sorted(feats) if hi[f] > lo[f]], dtype=np.int64) for feats in feats_list]


def restate_digits(x32, mn32, mx32, alpha, f):
    """int64 [m, r]: the digits of the float32 values x32 [m, r]; every operation is one numpy float64 operation."""
    x = np.asarray(x32, dtype=np.float32).astype(np.float64)
    mn = np.asarray(mn32, dtype=np.float32).astype(np.float64)
    w = np.asarray(mx32, dtype=np.float32).astype(np.float64) - mn
    t = np.zeros(x.shape)
    for j in range(x.shape[1]):
        if w[j] > 0:
            t[:, j] = (x[:, j] - mn[j]) / w[j]
    y = np.floor((t + np.asarray(alpha)[None, :]) / f)
    y = np.minimum(np.maximum(y, -1.0), np.floor(1.0 / f) + 2.0)
    return y.astype(np.int64) + 1


def radix(f):
    return int(np.floor(1.0 / f)) + 4


def pack_keys(digits, f):
    """uint64 [m]: sum_j digit_j R^j."""
    R, key = radix(f), np.zeros(digits.shape[0], np.uint64)
    assert R ** digits.shape[1] < 1 << 63
    for j in range(digits.shape[1]):
        key += digits[:, j].astype(np.uint64) * np.uint64(R ** j)
    return key


def restate_component(X, rows, cols, alpha, f):
    """(keys uint64 ascending, counts int64, mn float32 [r], mx float32 [r]) of one component on the sample `rows` of X."""
    sub = _canonical(X)[np.ix_(np.asarray(rows), np.asarray(cols))]
    mn, mx = sub.min(axis=0), sub.max(axis=0)
    keys, counts = np.unique(pack_keys(restate_digits(np.asarray(X, np.float32)[np.ix_(rows, cols)], mn, mx, alpha, f), f), return_counts=True)
    return keys, counts, mn, mx


def component_counts(comp, Q):
    """int64 [nq]: the count of the cell of every row of Q in a component (cols, alpha, f, keys, counts, mn, mx), 0 if absent."""
    cols, alpha, f, keys, counts, mn, mx = comp
    q = pack_keys(restate_digits(np.asarray(Q, np.float32)[:, cols], mn, mx, alpha, f), f)
    at = np.minimum(np.searchsorted(keys, q), len(keys) - 1)
    return np.where(keys[at] == q, counts[at], 0)


def restate_fit(X, feats_list, T, max_samples, seed):
    """The fitted state: s, table, denom, candidates, comps[z][t] = (cols, alpha, f, keys, counts, mn, mx), samples[z][t]
    (ascending rows) and the published arrays cell_key / cell_count / n_cells / sample_min / sample_max."""
    X = np.asarray(X, dtype=np.float32)
    n, S = X.shape[0], len(feats_list)
    s = restate_samples(max_samples, n)
    m = SimpleNamespace(s=s, T=T, S=S, table=restate_log_table(s), candidates=restate_candidates(X, feats_list), comps=[], samples=[])
    m.denom = T * int(m.table[s + 1])
    m.cell_key = np.full((S, T, s), PAD_KEY, np.uint64)
    m.cell_count, m.n_cells = np.zeros((S, T, s), np.int32), np.zeros((S, T), np.int32)
    m.sample_min, m.sample_max = np.zeros((S, T, MAX_DIMS), np.float32), np.zeros((S, T, MAX_DIMS), np.float32)
    for z, draws in enumerate(restate_components([len(c) for c in m.candidates], T, s, seed)):
        comps, samples = [], []
        for t, (f, positions, alpha) in enumerate(draws):
            rows = np.sort(feistel_perm_ref(np.arange(s), n, seed, z * T + t))
            cols = m.candidates[z][positions]
            keys, counts, mn, mx = restate_component(X, rows, cols, alpha, f)
            comps.append((cols, alpha, f, keys, counts, mn, mx))
            samples.append(rows)
            m.cell_key[z, t, :len(keys)], m.cell_count[z, t, :len(keys)], m.n_cells[z, t] = keys, counts, len(keys)
            m.sample_min[z, t, :len(cols)], m.sample_max[z, t, :len(cols)] = mn, mx
        m.comps.append(comps)
        m.samples.append(samples)
    return m


def restate_sums(m, Q, fitted_rows=False):
    """int64 [S, nq]: sum_t table[c_t]; fitted_rows: Q is the fitted X and a sampled row does not get the plus 1.  A subspace
    without components holds T table[s + 1]."""
    Q = np.asarray(Q, dtype=np.float32)
    out = np.zeros((m.S, Q.shape[0]), np.int64)
    for z in range(m.S):
        if not m.comps[z]:
            out[z] = m.denom
        for comp, rows in zip(m.comps[z], m.samples[z]):
            c = component_counts(comp, Q) + 1
            if fitted_rows:
                c[rows] -= 1
            assert c.min() >= 1 and c.max() <= m.s + 1
            out[z] += m.table[c]
    return out


def restate_scores(m, sums):
    """float64: 1 - sum / (T table[s + 1]), before the rounding to float32."""
    return 1.0 - np.asarray(sums, dtype=np.float64) / float(m.denom)


def restate_rshash(X_fit, X_query, feats_list, T=100, max_samples="auto", seed=0):
    """(model, fit scores float64 [S, n], query scores float64 [S, nq] or None)."""
    m = restate_fit(X_fit, feats_list, T, max_samples, seed)
    m.fit_sums = restate_sums(m, X_fit, fitted_rows=True)
    m.query_sums = None if X_query is None else restate_sums(m, X_query)
    return m, restate_scores(m, m.fit_sums), None if X_query is None else restate_scores(m, m.query_sums)


# ---- 1. a case worked by hand -------------------------------------------------------------------------------------------
def test_hand_computed_case():
    """One component, r = 2, f = 0.5, alpha = (0.25, 0.125), six rows which are all sampled (s = 6):

        feature 0: 0, 1, 2, 4, 4, 3: mn = 0, mx = 4, w = 4: x' = 0, .25, .5, 1, 1, .75; (x' + .25) / .5 = .5, 1, 1.5, 2.5, 2.5, 2
                   -> y = 0, 1, 1, 2, 2, 2 (row 1 lies exactly on the edge 1.0 and belongs to the cell above); digits 1, 2, 2, 3, 3, 3
        feature 1: 7 everywhere: w = 0 -> x' = 0; (0 + .125) / .5 = .25 -> y = 0; digit 1

    R = floor(1 / .5) + 4 = 6; keys = digit_0 + 6 digit_1 = 7, 8, 8, 9, 9, 9: three cells with 1, 2 and 3 rows.  At fit every
    row is in the sample: c = 1, 2, 2, 3, 3, 3 and score = 1 - log2(c) / log2(7) = 1, 0.64379, 0.64379, 0.43543 (x 3).  As new
    rows c = 2, 3, 3, 4, 4, 4.  The new row (-10, 7): x' = -2.5, (x' + .25) / .5 = -4.5, floor -5, clamped to -1: digit 0, key 6,
    an absent cell: c = 1, score 1.  The new row (1e30, 8): y clamped to floor(1 / f) + 2 = 4, digit 5 = R - 1; feature 1 has w
    = 0 and so x' = 0 whatever x: key 5 + 6 = 11, absent."""
    X = np.array([[0, 7], [1, 7], [2, 7], [4, 7], [4, 7], [3, 7]], np.float32)
    alpha, f = np.array([0.25, 0.125]), 0.5
    digits = restate_digits(X, [0, 7], [4, 7], alpha, f)
    np.testing.assert_array_equal(digits, [[1, 1], [2, 1], [2, 1], [3, 1], [3, 1], [3, 1]])
    assert radix(f) == 6
    np.testing.assert_array_equal(pack_keys(digits, f), [7, 8, 8, 9, 9, 9])
    keys, counts, mn, mx = restate_component(X, np.arange(6), [0, 1], alpha, f)
    np.testing.assert_array_equal(keys, [7, 8, 9])
    np.testing.assert_array_equal(counts, [1, 2, 3])
    np.testing.assert_array_equal(mn, [0, 7])
    np.testing.assert_array_equal(mx, [4, 7])
    comp = (np.array([0, 1]), alpha, f, keys, counts, mn, mx)
    table = restate_log_table(6)
    m = SimpleNamespace(S=1, T=1, s=6, table=table, denom=int(table[7]), comps=[[comp]], samples=[[np.arange(6)]])
    fit = restate_sums(m, X, fitted_rows=True)
    np.testing.assert_array_equal(fit[0], table[[1, 2, 2, 3, 3, 3]])
    np.testing.assert_allclose(restate_scores(m, fit)[0], 1.0 - np.log2([1, 2, 2, 3, 3, 3]) / np.log2(7.0), rtol=0, atol=1e-9)
    np.testing.assert_allclose(restate_scores(m, fit)[0, [0, 1, 3]], [1.0, 0.64379, 0.43543], rtol=0, atol=1e-5)
    np.testing.assert_array_equal(restate_sums(m, X)[0], table[[2, 3, 3, 4, 4, 4]])
    new = np.array([[-10, 7], [1e30, 8]], np.float32)
    np.testing.assert_array_equal(restate_digits(new, mn, mx, alpha, f), [[0, 1], [5, 1]])
    np.testing.assert_array_equal(restate_sums(m, new)[0], [0, 0])
    np.testing.assert_array_equal(restate_scores(m, restate_sums(m, new))[0], [1.0, 1.0])


# ---- 2. counts against an independent count ---------------------------------------------------------------------------
@pytest.mark.parametrize("n,max_samples", [(2, 2), (65, 64), (300, "auto"), (1500, 1024)])
def test_counts_equal_numpy_unique_on_the_digit_vectors(n, max_samples):
    X = tied_data(n, 8, seed=n)
    X[n - n // 3:] = X[:n // 3]  # duplicated rows
    feats = [[0, 1, 2, 3, 4, 5, 6, 7], [1, 2], [3], [0]]
    T = 4
    m = restate_fit(X, feats, T, max_samples, 5)
    if n >= 65:
        assert [list(c) for c in m.candidates] == [[0, 1, 2, 4, 5, 6, 7], [1, 2], [], [0]]  # column 3 is constant
    assert all(3 not in c for c in m.candidates) and len(m.candidates[0]) >= 5  # two rows can tie in columns 1 and 2
    live = [z for z in range(4) if len(m.candidates[z])]
    assert m.comps[2] == [] and (m.n_cells[2] == 0).all() and (m.cell_key[2] == PAD_KEY).all()
    for z in live:
        for t in range(T):
            cols, alpha, f, keys, counts, mn, mx = m.comps[z][t]
            rows = m.samples[z][t]
            assert len(set(rows.tolist())) == m.s and rows.min() >= 0 and rows.max() < n
            digits = restate_digits(X[np.ix_(rows, cols)], mn, mx, alpha, f)
            assert digits.min() >= 1 and digits.max() <= radix(f) - 2  # sampled rows use neither digit 0 nor digit R - 1
            cells, cell_counts = np.unique(digits, axis=0, return_counts=True)
            assert len(cells) == len(keys) == m.n_cells[z, t] and cell_counts.sum() == m.s
            np.testing.assert_array_equal(np.sort(pack_keys(cells, f)), keys)  # distinct vectors, distinct keys
            np.testing.assert_array_equal(cell_counts[np.argsort(pack_keys(cells, f))], counts)
            every = restate_digits(X[:, cols], mn, mx, alpha, f)  # all rows: a count is the number of equal sampled vectors
            want = (every[:, None, :] == digits[None, :, :]).all(axis=2).sum(axis=1)
            np.testing.assert_array_equal(component_counts(m.comps[z][t], X), want)
    sums = restate_sums(m, X, fitted_rows=True)
    assert (sums[2] == m.denom).all() and (restate_scores(m, sums)[2] == 0).all()
    per = restate_scores(m, sums)
    assert per.min() >= 0 and per.max() <= 1
    if n <= m.s:  # every row is in every sample: as new rows each count grows by exactly one
        for z in live:
            want = sum(m.table[component_counts(c, X) + 1] for c in m.comps[z])
            np.testing.assert_array_equal(restate_sums(m, X)[z], want)
            assert (restate_sums(m, X)[z] > sums[z]).all()


# ---- 3. the host draws and the log table against their formulas ---------------------------------------------------------
@pytest.mark.parametrize("s", [2, 3, 4, 64, 1000, 4096])
def test_components_follow_the_stated_rules(s):
    from vgan_amd.outlier import RSHASH_MAX_DIMS, rshash_components
    counts, T, seed = [40, 0, 1, 3, 12], 60, 11 + s
    width, dims, positions, shifts = rshash_components(counts, T, s, seed)
    assert width.shape == dims.shape == (5, T) and positions.shape == shifts.shape == (5, T, RSHASH_MAX_DIMS) == (5, T, MAX_DIMS)
    assert width.dtype == np.float64 and dims.dtype == np.int32 and positions.dtype == np.int32 and shifts.dtype == np.float64
    want = restate_components(counts, T, s, seed)
    lo = 1.0 / np.sqrt(float(s))
    clipped = 0
    for z, c in enumerate(counts):
        if c == 0:  # nothing drawn: the stream goes on with the next subspace
            assert want[z] == [] and (dims[z] == 0).all() and (width[z] == 0).all() and (positions[z] == -1).all() and (shifts[z] == 0).all()
            continue
        for t, (f, pos, alpha) in enumerate(want[z]):
            r = len(pos)
            assert width[z, t] == f and dims[z, t] == r
            np.testing.assert_array_equal(positions[z, t, :r], pos)
            np.testing.assert_array_equal(shifts[z, t, :r], alpha)
            assert (positions[z, t, r:] == -1).all() and (shifts[z, t, r:] == 0).all()
            # the stated ranges, from f alone
            assert min(lo, 1.0 - lo) <= f <= max(lo, 1.0 - lo)
            L = np.log(float(s)) / np.log(max(2.0, 1.0 / f))
            r_lo = int(np.floor(1.0 + L / 2.0))
            r_hi = max(r_lo, int(np.floor(L)))
            assert 1 <= r <= min(r_hi, c) and (r >= r_lo or r == c) and r <= MAX_DIMS
            clipped += r_lo > c
            assert (np.diff(pos) > 0).all() and pos.min() >= 0 and pos.max() < c
            assert (alpha >= 0).all() and (alpha < f).all()
            assert radix(f) ** r < 1 << 32
    if s >= 64:
        assert clipped > 0  # c_z < r_lo happened (one candidate, r_lo >= 2) and r fell to c_z
    if s == 4096:
        assert dims[0].max() == 12 and dims[4].max() == 12  # r = 12 is reached
    if s < 4:  # the inverted interval is used as written
        assert (width[0] <= lo).all() and (width[0] >= 1.0 - lo).all()


def test_log_table_is_the_correctly_rounded_q32_image():
    from decimal import Decimal, getcontext
    from vgan_amd.outlier import rshash_log_table
    getcontext().prec = 60
    ln2 = Decimal(2).ln()
    for s in (2, 3, 1000, 4096):
        table = rshash_log_table(s)
        assert table.dtype == np.int64 and table.shape == (s + 2,) and table[0] == 0 and table[1] == 0 and table[2] == 1 << 32
        np.testing.assert_array_equal(table, restate_log_table(s))
    table = rshash_log_table(4096)
    assert table[4096] == 12 << 32 and (np.diff(table[1:]) > 0).all()
    for c in list(range(1, 300)) + [1000, 1001, 4095, 4097]:
        exact = Decimal(c).ln() / ln2 * Decimal(2) ** 32
        assert abs(Decimal(int(table[c])) - exact) <= Decimal("0.5") + Decimal("1e-3"), c  # float64 log2 is within an ulp: 2^-17 here


# ---- 4. the recipe ------------------------------------------------------------------------------------------------------
RECIPE_SEEDS = (0, 1, 2, 3, 4)
RSHASH_BAR = 0.9695  # each bar 0.01 beyond the worst seed of its own side (the ranges in the test's docstring)
IFOREST_BAR = 0.9723
HBOS_BAR = 0.8914


def recipe_aucs(seed):
    """(RS-Hash restated at its defaults, sklearn's IsolationForest, HBOS restated at its defaults) on corr(seed)."""
    from sklearn.ensemble import IsolationForest
    X, y = corr(seed=seed)
    every = [list(range(X.shape[1]))]
    ours = auc(restate_rshash(X, None, every, seed=seed)[1][0], y)
    forest = auc(-IsolationForest(random_state=seed).fit(X).score_samples(X), y)
    hbos = auc(restate_hbos(X, None, every, 10, 0.1, 0.5)[0], y)
    return ours, forest, hbos


def test_restatement_finds_broken_correlations_before_the_forest_and_hbos():
    """corr(seed) for seed 0 .. 4 (2 000 rows in 6 features, 20 outliers that break the correlation of features 0 .. 3 inside
    every marginal range), all six features as one subspace, every detector at its defaults and seeded with the same seed.
    Measured with the real sampler (feistel_perm_ref), ROC AUC per seed:

        RS-Hash restated (T = 100, s = 1 000)      0.9795  0.9878  0.9930  0.9870  0.9910   range 0.9795 .. 0.9930
        sklearn IsolationForest(random_state=seed)  0.9486  0.9492  0.9623  0.9420  0.9591   range 0.9420 .. 0.9623
        HBOS restated (10 bins, alpha 0.1)          0.8415  0.8051  0.8605  0.8125  0.8814   range 0.8051 .. 0.8814

    The ranges do not overlap: the worst RS-Hash seed lies 0.017 above the best forest.  The bars are 0.01 beyond the worst
    seed of each side: RS-Hash >= 0.9695, the forest <= 0.9723, HBOS <= 0.8914; and seed by seed RS-Hash is above both."""
    got = np.array([recipe_aucs(seed) for seed in RECIPE_SEEDS])
    print("corr(seed), seeds 0 .. 4: RS-Hash", got[:, 0].round(4), "IsolationForest", got[:, 1].round(4), "HBOS", got[:, 2].round(4))
    assert got[:, 0].min() > got[:, 1].max() > got[:, 2].max()  # the ranges do not overlap
    assert (got[:, 0] >= RSHASH_BAR).all()
    assert (got[:, 1] <= IFOREST_BAR).all()
    assert (got[:, 2] <= HBOS_BAR).all()


# ---- the class, without a device ------------------------------------------------------------------------------------------
def test_constructor_and_argument_errors_touch_no_device():
    import vgan_amd
    from vgan_amd import outlier
    m = _mask(4, [[0, 1], [2, 3]])
    ens = vgan_amd.SubspaceRSHash(m, [0.5, 0.5])
    assert (ens.n_estimators, ens.max_samples, ens.seed) == (100, "auto", 0)
    assert ens.ops is None and ens.workspace_bytes == outlier.DEFAULT_WORKSPACE_BYTES
    assert (ens.normalize, ens.combination, ens.contamination) == (None, "sum", 0.1)
    assert list(ens.plan.order) == [0, 1]  # the given order
    for name in ("n_neighbors", "engine", "splits", "n_bins"):
        assert not hasattr(ens, name)
        with pytest.raises(TypeError):
            vgan_amd.SubspaceRSHash(m, [0.5, 0.5], **{name: 1})
    for bad in (0, 1025, -1, 2.0, True, None):
        with pytest.raises(ValueError, match="n_estimators"):
            vgan_amd.SubspaceRSHash(m, [0.5, 0.5], n_estimators=bad)
    for bad in (1, 4097, 0.5, 256.0, "all", None, True):
        with pytest.raises(ValueError, match="max_samples"):
            vgan_amd.SubspaceRSHash(m, [0.5, 0.5], max_samples=bad)
    for bad in (-1, 1 << 64, 0.0, "0", None):
        with pytest.raises(ValueError, match="seed"):
            vgan_amd.SubspaceRSHash(m, [0.5, 0.5], seed=bad)
    ok = vgan_amd.SubspaceRSHash(m, [0.5, 0.5], n_estimators=1024, max_samples=4096, seed=(1 << 64) - 1)
    assert (ok.n_estimators, ok.max_samples, ok.seed) == (1024, 4096, (1 << 64) - 1)
    assert vgan_amd.SubspaceRSHash(m, [0.5, 0.5], n_estimators=1, max_samples=2).max_samples == 2
    with pytest.raises(ValueError, match="proba has 3 entries for 2 subspaces"):
        vgan_amd.SubspaceRSHash(m, [0.5, 0.25, 0.25])
    with pytest.raises(ValueError, match="normalize"):
        vgan_amd.SubspaceRSHash(m, [0.5, 0.5], normalize="l2")
    with pytest.raises(ValueError, match="combination"):
        vgan_amd.SubspaceRSHash(m, [0.5, 0.5], combination="mean")
    with pytest.raises(ValueError, match="contamination"):
        vgan_amd.SubspaceRSHash(m, [0.5, 0.5], contamination=0.7)
    with pytest.raises(ValueError, match="between 2 and"):
        ens.fit(np.zeros((1, 4), np.float32))
    with pytest.raises(ValueError, match="features"):
        ens.fit(np.zeros((5, 3), np.float32))

    class Tall:  # only its shape is looked at before the row check raises
        shape = ((1 << 24) + 1, 4)

    with pytest.raises(ValueError, match="between 2 and"):
        ens.fit(Tall())
    assert ens.ops is None  # none of this touched the device
    for attr in ("cell_key_", "cell_count_", "n_cells_", "sample_min_", "sample_max_", "cell_sums_"):
        with pytest.raises(RuntimeError, match="not fitted"):
            getattr(ens, attr)
    with pytest.raises(RuntimeError, match="not fitted"):
        ens.decision_function(np.zeros((5, 4), np.float32))
    with pytest.raises(RuntimeError, match="not fitted"):
        ens.cell_sums(np.zeros((5, 4), np.float32))
    doc = vgan_amd.SubspaceRSHash.__doc__
    assert "position" in doc and "decision_function(X_train)" in doc and "Sathe" in doc
    assert outlier.rshash_components.__doc__ and "loda_projections" in outlier.__dict__


def test_outlier_ensemble_routes_rshash_to_the_new_class():
    import vgan_amd
    sub, proba = _mask(6, [[0, 1], [2, 3, 5], [4]]), np.array([0.5, 0.3, 0.2])
    kw = dict(n_estimators=7, max_samples=64, seed=3, normalize="robust", combination="max", contamination=0.05, workspace_bytes=1 << 20)

    def check(make):
        ens = make(method="rshash")
        assert type(ens) is vgan_amd.SubspaceRSHash and ens.n_estimators == 100 and ens.plan.count == 3
        np.testing.assert_array_equal(ens.proba, proba)
        ens = make(method="rshash", n_neighbors=17, **kw)  # n_neighbors is ignored
        assert (ens.n_estimators, ens.max_samples, ens.seed, ens.normalize, ens.combination, ens.contamination,
                ens.workspace_bytes) == (7, 64, 3, "robust", "max", 0.05, 1 << 20)
        assert not hasattr(ens, "n_neighbors")
        with pytest.raises(TypeError):
            make(method="rshash", engine="exact")  # not a keyword of SubspaceRSHash

    check(lambda **k: vgan_amd.build_ensemble(sub, proba, **k))
    for cls in (vgan_amd.VGAN_no_kl, vgan_amd.VGAN):
        model = cls(epochs=1)
        model.subspaces, model.proba = sub, proba
        check(model.outlier_ensemble)
        assert "rshash" in cls.outlier_ensemble.__doc__ and "SubspaceRSHash" in cls.outlier_ensemble.__doc__
    hics = vgan_amd.HiCS()
    with pytest.raises(RuntimeError, match="not fitted"):
        hics.outlier_ensemble(method="rshash")
    hics.subspaces, hics.proba = sub, proba
    check(hics.outlier_ensemble)
    assert "SubspaceRSHash" in vgan_amd.__all__
    with pytest.raises(ValueError, match="method"):  # the neighbour ensemble does not know it
        vgan_amd.SubspaceEnsemble(sub, proba, method="rshash")


# ---- C ABI: argument checks without a GPU -----------------------------------------------------------------------------------
def test_rshash_entries_reject_bad_arguments_without_gpu():
    import vgan_amd
    from vgan_amd import outlier
    lib = vgan_amd.lib.load()
    header = open(os.path.join(REPO, "include", "vgan_hip.h")).read()
    for name, value in (("MAX_SAMPLES", outlier.RSHASH_MAX_SAMPLES), ("MAX_COMPONENTS", outlier.RSHASH_MAX_COMPONENTS),
                        ("MAX_DIMS", outlier.RSHASH_MAX_DIMS), ("MAX_ROWS", outlier.RSHASH_MAX_ROWS)):
        assert int(re.search(rf"#define VGAN_RSHASH_{name} (\d+)", header).group(1)) == value
    null = None
    buf = ctypes.create_string_buffer(256)
    p = ctypes.cast(ctypes.addressof(buf) + (-ctypes.addressof(buf)) % 16, ctypes.c_void_p)  # never read

    def rejected(rc):
        msg = lib.vgan_last_error()
        return rc == 1 and b"bad argument" in msg and b"outlier_rshash.hip" in msg

    def each(fn, good, pointers, bad_values):
        for pos in pointers:
            assert rejected(fn(*[null if i == pos else v for i, v in enumerate(good)])), pos
        for pos, bad in bad_values:
            assert rejected(fn(*[bad if i == pos else v for i, v in enumerate(good)])), (pos, bad)

    # X, ldx, n, d, first, count, T, s, seed, comp x 4, key, count, cells, min, max, sample_rows (may be null), stream
    each(lib.vgan_rshash_build, [p, 4, 100, 4, 0, 2, 5, 64, 0, p, p, p, p, p, p, p, p, p, null, null], (0, 9, 10, 11, 12, 13, 14, 15, 16, 17),
         [(1, 3), (2, 1), (2, (1 << 24) + 1), (2, 63), (3, 0), (4, -1), (5, 0), (6, 0), (6, 1025), (7, 1), (7, 4097), (5, 1 << 30)])
    # Xq, row_stride, col_stride, rows, d, row_base, first, count, T, s, comp x 4, key, count, cells, min, max, sample_rows (may be
    # null), table, sums, ld_sums, stream
    good = [p, 4, 1, 10, 4, 0, 0, 2, 5, 64, p, p, p, p, p, p, p, p, p, null, p, p, 10, null]
    each(lib.vgan_rshash_cell_sums, good, (0, 10, 11, 12, 13, 14, 15, 16, 17, 18, 20, 21),
         [(1, 3), (2, 2), (3, 0), (4, 0), (5, -1), (6, -1), (7, 0), (7, 65536), (8, 0), (8, 1025), (9, 1), (9, 4097), (22, 9)])
    column_major = list(good)
    column_major[1], column_major[2] = 1, 9  # a column pitch below the row count
    assert rejected(lib.vgan_rshash_cell_sums(*column_major))
    # sums, ld_sums, count, rows, denom, score, ld_score, stream
    each(lib.vgan_rshash_scores, [p, 10, 2, 10, 1 << 32, p, 10, null], (0, 5),
         [(1, 9), (2, 0), (2, 65536), (3, 0), (4, 0), (4, -1), (6, 9)])
    for name, nargs in (("vgan_rshash_build", 20), ("vgan_rshash_cell_sums", 24), ("vgan_rshash_scores", 8)):
        assert len(vgan_amd.lib.SIGNATURES[name][1]) == nargs
    assert vgan_amd.lib.ABI_VERSION == lib.vgan_abi_version() == 11
