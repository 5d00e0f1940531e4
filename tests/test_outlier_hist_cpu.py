"""Histogram outlier scores over the subspaces (HBOS, LODA), CPU tier: the float64 numpy restatements the GPU tests compare
against, pinned to numpy.linspace (edges, bit for bit), numpy.histogram (edges and counts) and to a case worked by hand, and
everything of vgan_amd.SubspaceHBOS / SubspaceLODA that runs without a device (argument checks, the chunk rules, the host
term tables, the projections, the dispatch from the model, the C ABI's argument checks).

The definitions (the class docstrings): X as float32, arithmetic in float64, -0.0 as +0.0.  A histogram of a column with B
bins: lo, hi = min, max (lo == hi: lo - 0.5, lo + 0.5); step = (hi - lo) / B; e_j = j * step + lo in two roundings, e_B =
hi; the bin of x is #{j in 1 .. B - 1 : e_j <= x}.  HBOS: term_f[b] = -log2(count_b / (n step_f) + alpha), the term of the
rarest bin beyond tol steps outside the range, summed over the features of a subspace.  LODA: z = (((0 + w_0 x_0) + w_1 x_1) +
...), p[b] = (count_b + 1e-12) / (n + B 1e-12), the score (1 / k) sum_j -log p_j[bin(z_j)]."""
import ctypes
import os
import re

import numpy as np
import pytest

from conftest import REPO
from test_outlier_ecod_cpu import _f32, _mask, tied_data

BINS = [2, 3, 10, 33, 256]


def restate_edges(col, n_bins):
    """float64 [B + 1]: the edges of the float64 column col."""
    lo, hi = col.min(), col.max()
    if lo == hi:
        lo, hi = lo - 0.5, hi + 0.5
    step = (hi - lo) / n_bins
    e = np.arange(n_bins + 1, dtype=np.float64) * step  # the product, rounded
    e = e + lo  # then the sum
    e[n_bins] = hi
    return e


def restate_bins(edges, x):
    """int64 [len(x)]: #{j in 1 .. B - 1 : e_j <= x}."""
    B = len(edges) - 1
    return (edges[1:B][None, :] <= np.asarray(x)[:, None]).sum(axis=1)


def restate_histograms(A, n_bins):
    """(edges float64 [P, B + 1], counts int64 [P, B]) of the columns of the float64 matrix A [n, P]."""
    edges = np.stack([restate_edges(A[:, c], n_bins) for c in range(A.shape[1])])
    counts = np.stack([np.bincount(restate_bins(edges[c], A[:, c]), minlength=n_bins) for c in range(A.shape[1])])
    return edges, counts.astype(np.int64)


def restate_hbos_terms(X_fit, X_query, n_bins, alpha, tol):
    """(T float64 [nq, d], edges, counts): the term of every (query row, feature); X_query None: X_fit itself."""
    A = _f32(X_fit)
    Q = A if X_query is None else _f32(X_query)
    n, d = A.shape
    edges, counts = restate_histograms(A, n_bins)
    T = np.empty(Q.shape)
    for f in range(d):
        lo, hi = edges[f, 0], edges[f, -1]
        step = (hi - lo) / n_bins
        dens = counts[f].astype(np.float64) / (float(n) * step)
        term = -np.log2(dens + alpha)
        rare = -np.log2(dens.min() + alpha)
        x = Q[:, f]
        outside = (x < lo - tol * step) | (x > hi + tol * step)
        T[:, f] = np.where(outside, rare, term[restate_bins(edges[f], x)])
    return T, edges, counts


def restate_hbos(X_fit, X_query, feats_list, n_bins, alpha, tol):
    """float64 [S, nq]: the per-subspace HBOS scores before the rounding to float32."""
    T = restate_hbos_terms(X_fit, X_query, n_bins, alpha, tol)[0]
    return np.stack([T[:, np.asarray(feats)].sum(axis=1) for feats in feats_list])


def restate_projected(A, feats, features, weights):
    """float64 [n, k]: z of the rows of the float64 matrix A for one subspace (feats: its columns of A)."""
    sub = A[:, np.asarray(feats)]
    z = np.zeros((A.shape[0], features.shape[0]))
    for j in range(features.shape[0]):
        acc = np.zeros(A.shape[0])
        for t in range(features.shape[1]):
            acc = acc + weights[j, t] * sub[:, features[j, t]]
        z[:, j] = acc
    return z


def restate_loda_parts(X_fit, X_query, feats_list, features, weights, n_bins):
    """(per float64 [S, nq], edges [S, k, B + 1], counts [S, k, B]); X_query None: X_fit itself."""
    A = _f32(X_fit)
    Q = A if X_query is None else _f32(X_query)
    n = A.shape[0]
    per, all_edges, all_counts = [], [], []
    for s, feats in enumerate(feats_list):
        k = features[s].shape[0]
        edges, counts = restate_histograms(restate_projected(A, feats, features[s], weights[s]), n_bins)
        zq = restate_projected(Q, feats, features[s], weights[s])
        p = (counts.astype(np.float64) + 1e-12) / (float(n) + n_bins * 1e-12)
        total = np.zeros(Q.shape[0])
        for j in range(k):
            total = total + -np.log(p[j][restate_bins(edges[j], zq[:, j])])
        per.append((1.0 / k) * total)
        all_edges.append(edges)
        all_counts.append(counts)
    return np.stack(per), np.stack(all_edges), np.stack(all_counts)


def restate_loda(X_fit, X_query, feats_list, features, weights, n_bins):
    """float64 [S, nq]: the per-subspace LODA scores before the rounding to float32."""
    return restate_loda_parts(X_fit, X_query, feats_list, features, weights, n_bins)[0]


def planted_feature_outliers():
    """(X float32 [2020, 10], y): 2000 standard normal rows, then 20 whose feature 3 is shifted by +-(4.5 .. 6)."""
    rng = np.random.default_rng(5)
    inliers = rng.normal(size=(2000, 10))
    outliers = rng.normal(size=(20, 10))
    signs = rng.choice([-1, 1], size=20)
    outliers[:, 3] += signs * rng.uniform(4.5, 6, size=20)
    return np.vstack([inliers, outliers]).astype(np.float32), np.r_[np.zeros(2000, int), np.ones(20, int)]


def roc_auc(scores, y):
    from scipy.stats import rankdata
    r = rankdata(scores)
    pos = y == 1
    return (r[pos].sum() - pos.sum() * (pos.sum() + 1) / 2.0) / (pos.sum() * (~pos).sum())


# ---- the restatement, pinned ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 2, 7, 300])
def test_edges_are_linspace_and_counts_are_numpy_histogram(n):
    A = _f32(tied_data(n, 6, seed=n))
    for B in BINS:
        edges, counts = restate_histograms(A, B)
        assert edges.shape == (6, B + 1) and counts.shape == (6, B) and (counts.sum(axis=1) == n).all()
        for f in range(6):
            want_counts, want_edges = np.histogram(A[:, f], bins=B)
            np.testing.assert_array_equal(edges[f].view(np.uint64), want_edges.astype(np.float64).view(np.uint64))
            np.testing.assert_array_equal(edges[f].view(np.uint64), np.linspace(want_edges[0], want_edges[-1], B + 1).view(np.uint64))
            np.testing.assert_array_equal(counts[f], want_counts)
        if n > 1:
            np.testing.assert_array_equal(edges[3, [0, -1]], [2.0, 3.0])  # the constant column 2.5


@pytest.mark.parametrize("B", [2, 4, 10, 16])
def test_values_exactly_on_edges_fall_where_numpy_puts_them(B):
    col = np.arange(41, dtype=np.float64) / 4
    edges, counts = restate_histograms(col[:, None], B)
    want_counts, want_edges = np.histogram(col, bins=B)
    np.testing.assert_array_equal(edges[0].view(np.uint64), want_edges.view(np.uint64))
    np.testing.assert_array_equal(counts[0], want_counts)
    # outside the range: the first and the last bin
    np.testing.assert_array_equal(restate_bins(edges[0], np.array([-1e30, -0.25, 10.0, 10.25, 1e30])), [0, 0, B - 1, B - 1, B - 1])


def test_hand_worked_case():
    """Column (0, 1, 3, 3, 4), B = 2: edges (0, 2, 4), bins (0, 0, 1, 1, 1), counts (2, 3), step 2, dens = (2, 3) / 10.
    HBOS, alpha 0.1, tol 0.5: terms -log2(0.3), -log2(0.4); the limits are -1 and 5; beyond them -log2(0.2 + 0.1)."""
    X = np.array([[0.0], [1.0], [3.0], [3.0], [4.0]], np.float32)
    edges, counts = restate_histograms(_f32(X), 2)
    np.testing.assert_array_equal(edges, [[0.0, 2.0, 4.0]])
    np.testing.assert_array_equal(counts, [[2, 3]])
    a, b = -np.log2(0.2 + 0.1), -np.log2(0.3 + 0.1)
    np.testing.assert_allclose(restate_hbos(X, None, [[0]], 2, 0.1, 0.5)[0], [a, a, b, b, b], rtol=1e-15)
    # 4.9 and -0.9 lie outside the range but within tol * step = 1: the last and the first bin; 5.5 and -1.5 lie beyond
    Q = np.array([[4.9], [5.5], [-0.9], [-1.5], [2.0]], np.float32)
    np.testing.assert_allclose(restate_hbos(X, Q, [[0]], 2, 0.1, 0.5)[0], [b, a, a, a, b], rtol=1e-15)
    np.testing.assert_allclose(restate_hbos(X, Q, [[0]], 2, 0.1, 0.0)[0], [a, a, a, a, b], rtol=1e-15)  # tol 0: all four beyond
    assert restate_hbos(X, Q, [[0]], 2, 1.0, 0.5)[0, 1] < 0  # scores may be negative: -log2(0.2 + 1)
    # LODA, two projections of the one feature, weights 2 and -1: z = (0, 2, 6, 6, 8) -> edges (0, 4, 8), counts (2, 3);
    # z = (0, -1, -3, -3, -4) -> edges (-4, -2, 0), bins (1, 1, 0, 0, 0), counts (3, 2)
    features, weights = [np.array([[0], [0]])], [np.array([[2.0], [-1.0]])]
    per, e, c = restate_loda_parts(X, None, [[0]], features, weights, 2)
    np.testing.assert_array_equal(e[0], [[0.0, 4.0, 8.0], [-4.0, -2.0, 0.0]])
    np.testing.assert_array_equal(c[0], [[2, 3], [3, 2]])
    l2, l3 = -np.log(0.4), -np.log(0.6)
    np.testing.assert_allclose(per[0], [l2, l2, l3, l3, l3], rtol=1e-11)
    one = restate_loda(X, np.array([[100.0], [3.5]], np.float32), [[0]], [features[0][:1]], [weights[0][:1]], 2)
    np.testing.assert_allclose(one[0], [l3, l3], rtol=1e-11)  # beyond the range: the last bin, no special rule
    assert (per >= 0).all()


def test_negative_zero_is_zero():
    X = np.array([[-0.0], [0.0], [-1.0], [1.0]], np.float32)
    T, edges, counts = restate_hbos_terms(X, np.array([[-0.0], [0.0]], np.float32), 2, 0.1, 0.5)
    np.testing.assert_array_equal(counts, [[1, 3]])  # both zeros sit on the middle edge: the upper bin
    assert T[0, 0] == T[1, 0]


# ---- the projections --------------------------------------------------------------------------------------------------------
def test_loda_projections():
    from vgan_amd.outlier import loda_projections
    dims = [1, 2, 3, 4, 67]
    features, weights = loda_projections(dims, 9, seed=3)
    assert len(features) == len(weights) == 5
    for d_s, m, f, w in zip(dims, [1, 1, 1, 2, 8], features, weights):
        assert f.shape == w.shape == (9, m) and f.dtype.kind == "i" and w.dtype == np.float64
        assert (f >= 0).all() and (f < d_s).all()
        assert (np.diff(f, axis=1) > 0).all()  # ascending and distinct
    again = loda_projections(dims, 9, seed=3)
    other = loda_projections(dims, 9, seed=4)
    for a, b, c in zip(weights, again[1], other[1]):
        np.testing.assert_array_equal(a, b)
        assert not np.array_equal(a, c)
    for a, b in zip(features, again[0]):
        np.testing.assert_array_equal(a, b)
    assert not all(np.array_equal(a, c) for a, c in zip(features, other[0]))
    # the documented stream, literally
    rng = np.random.default_rng(3)
    for s, d_s in enumerate(dims):
        m = max(1, int(np.floor(np.sqrt(d_s))))
        for j in range(9):
            np.testing.assert_array_equal(features[s][j], np.sort(rng.choice(d_s, m, replace=False)))
            np.testing.assert_array_equal(weights[s][j], rng.standard_normal(m))
    # the first subspace alone draws what it draws among others
    np.testing.assert_array_equal(loda_projections([67, 5], 9, seed=3)[1][0], loda_projections([67], 9, seed=3)[1][0])


# ---- the classes, without a device ------------------------------------------------------------------------------------------
def test_constructors_and_argument_errors_touch_no_device():
    import vgan_amd
    from vgan_amd import outlier
    m = _mask(4, [[0, 1], [2, 3]])
    h = vgan_amd.SubspaceHBOS(m, [0.5, 0.5])
    assert (h.n_bins, h.alpha, h.tol, h.workspace_bytes) == (10, 0.1, 0.5, outlier.DEFAULT_WORKSPACE_BYTES) and h.ops is None
    lo = vgan_amd.SubspaceLODA(m, [0.5, 0.5])
    assert (lo.n_projections, lo.n_bins, lo.seed, lo.workspace_bytes) == (100, 10, 0, outlier.DEFAULT_WORKSPACE_BYTES) and lo.ops is None
    for ens in (h, lo):
        assert (ens.normalize, ens.combination, ens.contamination) == (None, "sum", 0.1) and list(ens.plan.order) == [0, 1]
        assert not hasattr(ens, "engine")
    for cls in (vgan_amd.SubspaceHBOS, vgan_amd.SubspaceLODA):
        for name in ("n_neighbors", "engine", "splits"):
            with pytest.raises(TypeError):
                cls(m, [0.5, 0.5], **{name: 1})
        for good in (2, 256, np.int64(33)):
            assert cls(m, [0.5, 0.5], n_bins=good).n_bins == int(good)
        for bad in (1, 0, -3, 257, 10.0, "auto", None, True):
            with pytest.raises(ValueError, match="n_bins"):
                cls(m, [0.5, 0.5], n_bins=bad)
        with pytest.raises(ValueError, match="proba has 3 entries for 2 subspaces"):
            cls(m, [0.5, 0.25, 0.25])
        with pytest.raises(ValueError, match="normalize"):
            cls(m, [0.5, 0.5], normalize="l2")
        with pytest.raises(ValueError, match="combination"):
            cls(m, [0.5, 0.5], combination="mean")
        with pytest.raises(ValueError, match="contamination"):
            cls(m, [0.5, 0.5], contamination=0.7)
    assert vgan_amd.SubspaceHBOS(m, [0.5, 0.5], alpha=1e-300, tol=0).tol == 0.0
    assert vgan_amd.SubspaceHBOS(m, [0.5, 0.5], alpha=7, tol=3).alpha == 7.0
    for bad in (0, 0.0, -0.1, np.nan, np.inf, "0.1", None):
        with pytest.raises(ValueError, match="alpha"):
            vgan_amd.SubspaceHBOS(m, [0.5, 0.5], alpha=bad)
    for bad in (-1e-9, -1, np.nan, np.inf, "0.5", None):
        with pytest.raises(ValueError, match="tol"):
            vgan_amd.SubspaceHBOS(m, [0.5, 0.5], tol=bad)
    for good in (1, 1024):
        assert vgan_amd.SubspaceLODA(m, [0.5, 0.5], n_projections=good).n_projections == good
    for bad in (0, -1, 1025, 100.0, None, "100"):
        with pytest.raises(ValueError, match="n_projections"):
            vgan_amd.SubspaceLODA(m, [0.5, 0.5], n_projections=bad)
    assert vgan_amd.SubspaceLODA(m, [0.5, 0.5], seed=12345).seed == 12345
    for bad in (-1, 0.5, None, "0"):
        with pytest.raises(ValueError, match="seed"):
            vgan_amd.SubspaceLODA(m, [0.5, 0.5], seed=bad)
    with pytest.raises(ValueError, match="at most"):
        vgan_amd.SubspaceLODA(np.ones((1, outlier.LODA_MAX_DIMS + 1), bool), [1.0])
    assert vgan_amd.SubspaceLODA(np.ones((1, outlier.LODA_MAX_DIMS), bool), [1.0]).plan.count == 1

    class Tall:  # only its shape is looked at before the row check raises
        shape = (outlier.HIST_MAX_ROWS + 1, 4)

    assert outlier.HIST_MAX_ROWS == 1 << 24
    for ens in (h, lo):
        with pytest.raises(ValueError, match="between 1 and"):
            ens.fit(np.empty((0, 4), np.float32))
        with pytest.raises(ValueError, match="between 1 and"):
            ens.fit(Tall())
        with pytest.raises(ValueError, match="features"):
            ens.fit(np.zeros((5, 3), np.float32))
        assert ens.ops is None  # none of this touched the device
        with pytest.raises(RuntimeError, match="not fitted"):
            ens.decision_function(np.zeros((5, 4), np.float32))


def test_chunk_rules():
    from vgan_amd.outlier import hbos_chunk_rows, loda_chunks
    # HBOS, per row: one float64 term per feature, one float32 score per subspace
    assert hbos_chunk_rows(10, 3, 1) == 1
    assert hbos_chunk_rows(10, 3, 92) == 1
    assert hbos_chunk_rows(10, 3, 2 * 92) == 2
    assert hbos_chunk_rows(10, 3, 5 * 92 + 91) == 5
    assert hbos_chunk_rows(784, 500, 1 << 30) == (1 << 30) // (784 * 8 + 2000)
    # LODA: the packed block, float32 [rows, round4(d_s)] per subspace
    dims = [3, 4, 5, 20]  # packed widths 4, 4, 8, 20: 144 bytes a row
    assert loda_chunks(dims, 100, 1 << 30) == (100, [(0, 4)])
    assert loda_chunks(dims, 100, 100 * 144) == (100, [(0, 4)])
    assert loda_chunks(dims, 100, 100 * 144 - 1) == (99, [(0, 4)])
    assert loda_chunks(dims, 100, 50 * 144 + 143) == (50, [(0, 4)])
    assert loda_chunks(dims, 100, 144) == (1, [(0, 4)])
    assert loda_chunks(dims, 100, 143) == (1, [(0, 3), (3, 1)])  # below a row of every subspace: ranges of single rows
    assert loda_chunks(dims, 100, 32) == (1, [(0, 2), (2, 1), (3, 1)])
    assert loda_chunks(dims, 100, 1) == (1, [(0, 1), (1, 1), (2, 1), (3, 1)])
    assert loda_chunks([7], 5, 1 << 20) == (5, [(0, 1)])


@pytest.mark.parametrize("B", [2, 10, 33])
def test_term_tables_equal_the_restatement_bit_for_bit(B):
    from vgan_amd.outlier import hbos_term_table, loda_term_table
    X, Y = tied_data(301, 6, seed=1), tied_data(40, 6, seed=2)
    Y[0], Y[1] = 1e30, -1e30
    alpha, tol = 0.1, 0.5
    T, edges, counts = restate_hbos_terms(X, Y, B, alpha, tol)
    table, limits = hbos_term_table(counts, edges, 301, alpha, tol)
    assert table.shape == (6, B + 1) and limits.shape == (6, 2) and table.dtype == limits.dtype == np.float64
    Q = _f32(Y)
    for f in range(6):
        bins = restate_bins(edges[f], Q[:, f])
        outside = (Q[:, f] < limits[f, 0]) | (Q[:, f] > limits[f, 1])
        assert outside[:2].all()
        np.testing.assert_array_equal(np.where(outside, table[f, B], table[f, bins]).view(np.uint64), T[:, f].view(np.uint64))
    counts3 = np.stack([counts, counts[::-1]])
    want = -np.log((counts3.astype(np.float64) + 1e-12) / (301.0 + B * 1e-12))
    got = loda_term_table(counts3, 301)
    assert got.shape == (2, 6, B) and (got >= 0).all()
    np.testing.assert_array_equal(got.view(np.uint64), want.view(np.uint64))


def test_outlier_ensemble_routes_hbos_and_loda_to_the_new_classes():
    import vgan_amd
    model = vgan_amd.VGAN_no_kl(epochs=1)
    model.subspaces = _mask(6, [[0, 1], [2, 3, 5], [4]])
    model.proba = np.array([0.5, 0.3, 0.2])
    ens = model.outlier_ensemble(method="hbos")
    assert type(ens) is vgan_amd.SubspaceHBOS and ens.n_bins == 10 and ens.plan.count == 3
    np.testing.assert_array_equal(ens.proba, model.proba)
    ens = model.outlier_ensemble(method="hbos", n_neighbors=17, n_bins=33, alpha=0.2, tol=0.25, normalize="robust", combination="max",
                                 contamination=0.05, workspace_bytes=1 << 20)  # n_neighbors is ignored
    assert (ens.n_bins, ens.alpha, ens.tol, ens.normalize, ens.combination, ens.contamination, ens.workspace_bytes) == (
        33, 0.2, 0.25, "robust", "max", 0.05, 1 << 20)
    assert not hasattr(ens, "n_neighbors")
    ens = model.outlier_ensemble(method="loda", n_neighbors=17, n_projections=7, n_bins=5, seed=9, normalize="zscore")
    assert type(ens) is vgan_amd.SubspaceLODA and (ens.n_projections, ens.n_bins, ens.seed, ens.normalize) == (7, 5, 9, "zscore")
    assert not hasattr(ens, "n_neighbors")
    for method in ("hbos", "loda"):
        with pytest.raises(TypeError):
            model.outlier_ensemble(method=method, engine="exact")
        assert method in vgan_amd.VGAN_no_kl.outlier_ensemble.__doc__
    assert "SubspaceHBOS" in vgan_amd.__all__ and "SubspaceLODA" in vgan_amd.__all__


# ---- detection, on the restatement (the GPU scores match it) ----------------------------------------------------------------
def test_a_shifted_feature_is_found_in_its_subspace():
    from vgan_amd.outlier import loda_projections
    X, y = planted_feature_outliers()
    assert roc_auc(restate_hbos(X, None, [[3]], 10, 0.1, 0.5)[0], y) >= 0.99
    features, weights = loda_projections([1], 100, 0)
    assert roc_auc(restate_loda(X, None, [[3]], features, weights, 10)[0], y) >= 0.99


# ---- C ABI: argument checks without a GPU -----------------------------------------------------------------------------------
def test_hist_entries_reject_bad_arguments_without_gpu():
    import vgan_amd
    from vgan_amd import outlier
    lib = vgan_amd.lib.load()
    header = open(os.path.join(REPO, "include", "vgan_hip.h")).read()
    for macro, value in (("VGAN_HIST_MAX_BINS", outlier.HIST_MAX_BINS), ("VGAN_HIST_MAX_ROWS", outlier.HIST_MAX_ROWS),
                         ("VGAN_LODA_MAX_PROJECTIONS", outlier.LODA_MAX_PROJECTIONS), ("VGAN_LODA_MAX_DIMS", outlier.LODA_MAX_DIMS)):
        assert int(re.search(rf"#define {macro} (\d+)", header).group(1)) == value
    null = None
    buf = ctypes.create_string_buffer(256)
    p = ctypes.cast(ctypes.addressof(buf) + (-ctypes.addressof(buf)) % 16, ctypes.c_void_p)  # never read

    def rejected(rc):
        msg = lib.vgan_last_error()
        return rc == 1 and b"bad argument" in msg and b"outlier_hist.hip" in msg

    def each_bad(fn, good, pointers, bad_values):
        for pos in pointers:
            assert rejected(fn(*[null if i == pos else v for i, v in enumerate(good)])), (fn.__name__, pos)
        for pos, bad in bad_values:
            assert rejected(fn(*[bad if i == pos else v for i, v in enumerate(good)])), (fn.__name__, pos, bad)

    rows_max = outlier.HIST_MAX_ROWS
    # X, ldx, n, d, keys, stream
    each_bad(lib.vgan_hist_column_range, [p, 4, 10, 4, p, null], (0, 4), ((1, 3), (2, 0), (2, rows_max + 1), (3, 0)))
    # keys, P, B, edges, stream
    each_bad(lib.vgan_hist_edges, [p, 4, 10, p, null], (0, 3), ((1, 0), (2, 1), (2, 257), (1, 1 << 40)))
    # X, ldx, n, d, edges, B, counts, stream
    each_bad(lib.vgan_hist_column_counts, [p, 4, 10, 4, p, 10, p, null], (0, 4, 6),
             ((1, 3), (2, 0), (2, rows_max + 1), (3, 0), (5, 1), (5, 257)))
    # Xq, ldq, rows, d, edges, B, table, limits, mask, ldm, S, terms, score, ld_score, stream
    each_bad(lib.vgan_hbos_scores, [p, 4, 3, 4, p, 10, p, p, p, 2, 2, p, p, 3, null], (0, 4, 6, 7, 8, 11, 12),
             ((1, 3), (2, 0), (3, 0), (5, 1), (5, 257), (9, 1), (10, 0), (13, 2)))
    # keys, P, counts, cells, stream
    assert rejected(lib.vgan_hist_reset(null, 0, null, 0, null))
    assert rejected(lib.vgan_hist_reset(p, 0, null, 0, null))
    assert rejected(lib.vgan_hist_reset(null, 0, p, 0, null))
    # P, rows, feat_off, col_off, first, count, max_dims, pidx, pw, moff, k, ...
    head = [p, 3, p, p, 0, 2, 8, p, p, p, 7]
    head_bad = ((1, 0), (1, rows_max + 1), (4, -1), (5, 0), (5, 65536), (6, 0), (6, outlier.LODA_MAX_DIMS + 1), (10, 0),
                (10, outlier.LODA_MAX_PROJECTIONS + 1))
    each_bad(lib.vgan_loda_range, head + [p, null], (0, 2, 3, 7, 8, 9, 11), head_bad)
    each_bad(lib.vgan_loda_counts, head + [p, 10, p, null], (0, 2, 3, 7, 8, 9, 11, 13), head_bad + ((12, 1), (12, 257)))
    each_bad(lib.vgan_loda_scores, head + [p, 10, p, p, 3, null], (0, 2, 3, 7, 8, 9, 11, 13, 14), head_bad + ((12, 1), (12, 257), (15, 2)))
    for name, nargs in (("vgan_hist_column_range", 6), ("vgan_hist_edges", 5), ("vgan_hist_column_counts", 8), ("vgan_hbos_scores", 15),
                        ("vgan_hist_reset", 5), ("vgan_loda_range", 13), ("vgan_loda_counts", 15), ("vgan_loda_scores", 17)):
        assert len(vgan_amd.lib.SIGNATURES[name][1]) == nargs
    assert vgan_amd.lib.ABI_VERSION == lib.vgan_abi_version()
