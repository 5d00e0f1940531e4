"""Histogram outlier scores over the subspaces on the MI355X (csrc/outlier_hist.hip through vgan_amd.SubspaceHBOS,
vgan_amd.SubspaceLODA and the ops wrappers), against the float64 restatements of test_outlier_hist_cpu.py (pinned to
numpy.linspace, numpy.histogram and a hand-worked case there).

Range, edges and counts are exact: edges bit-equal (two separately rounded operations, as numpy.linspace takes them), counts
integer-equal.

The HBOS bar on a per-subspace score is |got - want| <= 2^-23 |want| + (d_s + 4) 2^-52 sum_f |T_f|.  The terms come from the
table the host builds from the integer counts, so they are bit-equal to the restatement's; kernel and restatement then differ
in the order of a sum of d_s float64 terms only.  A sum of d_s terms in any order is within (d_s - 1) 2^-53 sum_f |T_f| of the
exact sum (first order), so two orders differ by at most (d_s - 1) 2^-52 sum_f |T_f|; the matrix unit adds the masked-out
features as exact zeros.  HBOS terms change sign (-log2 of a density above 1 - alpha is negative), so the sum can cancel and
this part of the bar is absolute, in units of the terms, not of the result.  The final rounding to float32 adds half an ulp of
the result, and one ulp where the two float64 values straddle a rounding boundary: 2^-23 |want|.

LODA's terms are non-negative (-log of a probability), so every order of their sum is within k 2^-53 relative of the exact
one and the bar is one float32 ulp relative, with no absolute term.  Its projected values must equal the restatement's bit for
bit (every product and every sum rounded on its own): a fused multiply-add would move edges by an ulp, which the bit-equal
comparison of bin_edges_ shows, and values across bin boundaries, which histograms_ shows."""
import numpy as np
import pytest

from test_outlier_ecod_cpu import _f32, _mask, tied_data
from test_outlier_ecod_gpu import _features
from test_outlier_gpu import _planted
from test_outlier_hist_cpu import restate_hbos_terms, restate_histograms, restate_loda, restate_loda_parts
from test_outlier_norm_cpu import restate_proba
from test_outlier_norm_gpu import _check_scores, _check_stats

pytestmark = pytest.mark.gpu

ULP32 = 2.0 ** -23
ALPHA, TOL = 0.1, 0.5


def _proba(S):
    p = np.random.default_rng(S).random(S)
    return p / p.sum()


def _rows(d):
    """301 fitted and 130 new rows: the first 40 new rows are fitted rows again, rows 40 / 41 lie far outside every range,
    rows 42 / 43 outside the range but within tol * step of it."""
    X, Y = tied_data(301, d, seed=11), tied_data(130, d, seed=12)
    Y[:40] = X[:40]
    Y[40], Y[41] = 1e30, -1e30
    return X, Y


def _just_inside(X, Y, n_bins):
    """Y with rows 42 / 43 set to hi + 0.4 step and lo - 0.4 step of every fitted column (tol is 0.5)."""
    edges = restate_histograms(_f32(X), n_bins)[0]
    step = (edges[:, -1] - edges[:, 0]) / n_bins
    Y = Y.copy()
    Y[42], Y[43] = (edges[:, -1] + 0.4 * step).astype(np.float32), (edges[:, 0] - 0.4 * step).astype(np.float32)
    return Y


def _check_hbos(got32, X, Y, feats, n_bins):
    T = restate_hbos_terms(X, Y, n_bins, ALPHA, TOL)[0]
    got32 = np.asarray(got32)
    assert got32.dtype == np.float32 and got32.shape == (len(feats), T.shape[0])
    for s, f in enumerate(feats):
        want = T[:, f].sum(axis=1)
        bar = ULP32 * np.abs(want) + (len(f) + 4) * 2.0 ** -52 * np.abs(T[:, f]).sum(axis=1)
        err = np.abs(got32[s].astype(np.float64) - want)
        assert (err <= bar).all(), (s, float((err / np.maximum(bar, 1e-300)).max()))


def _check_loda(got32, want):
    got32 = np.asarray(got32)
    assert got32.dtype == np.float32 and got32.shape == want.shape
    assert (got32 >= 0).all()
    assert (np.abs(got32.astype(np.float64) - want) <= ULP32 * np.abs(want)).all()


# ---- 1. range, edges and counts --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("d", [1, 5, 67])
@pytest.mark.parametrize("n", [1, 2, 3, 257, 1000, 4099])
def test_edges_and_counts_equal_numpy(n, d):
    """n below, at and above a slab of rows, d off every tile width (d > 3 brings the constant column, d > 4 the descending
    one); the output buffers hold a sentinel first, so that an unwritten entry shows."""
    import torch
    from vgan_amd.ops import default_ops
    ops = default_ops()
    X = tied_data(n, d, seed=400 + n)
    Xd = torch.as_tensor(X, device="cuda")
    for B in (2, 10, 33, 256):
        keys = torch.full((d, 2), 0x5555555555555555, dtype=torch.int64, device="cuda")
        edges = torch.full((d, B + 1), -7.25, dtype=torch.float64, device="cuda")
        counts = torch.full((d, B), -7, dtype=torch.int32, device="cuda")
        ops.hist_column_range(Xd, keys)
        ops.hist_edges(keys, B, edges)
        ops.hist_column_counts(Xd, edges, counts)
        want_edges, want_counts = restate_histograms(_f32(X), B)
        np.testing.assert_array_equal(edges.cpu().numpy().view(np.uint64), want_edges.view(np.uint64))
        np.testing.assert_array_equal(counts.cpu().numpy(), want_counts)
        assert int(counts.sum()) == n * d


# ---- 2. HBOS ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("S", [1, 17, 33])
@pytest.mark.parametrize("d", [1, 5, 67])
def test_hbos_scores_match_the_restatement(d, S):
    """Neither row count is a multiple of the 64-row tile, d is off the multiples of 4, S off the multiples of 16 and 32; the
    full mask, a single-feature mask on the constant column and random masks."""
    import vgan_amd
    X, Y0 = _rows(d)
    feats = _features(d, S, seed=5)
    proba = _proba(S)
    for B in (2, 10, 33):
        Y = _just_inside(X, Y0, B)
        ens = vgan_amd.SubspaceHBOS(_mask(d, feats), proba, n_bins=B, alpha=ALPHA, tol=TOL).fit(X)
        want_edges, want_counts = restate_histograms(_f32(X), B)
        assert ens.bin_edges_.dtype == np.float64 and ens.bin_edges_.shape == (d, B + 1)
        assert ens.histograms_.dtype == np.int64 and ens.histograms_.shape == (d, B)
        np.testing.assert_array_equal(ens.bin_edges_.view(np.uint64), want_edges.view(np.uint64))
        np.testing.assert_array_equal(ens.histograms_, want_counts)
        per = ens.per_subspace_scores_
        _check_hbos(per, X, None, feats, B)
        np.testing.assert_allclose(ens.decision_scores_, proba @ per.astype(np.float64), rtol=1e-12, atol=0)
        got, per_new = ens.decision_function(Y, return_per_subspace=True)
        _check_hbos(per_new, X, Y, feats, B)
        np.testing.assert_allclose(got, proba @ per_new.astype(np.float64), rtol=1e-12, atol=0)
        again, per_again = ens.decision_function(X, return_per_subspace=True)
        np.testing.assert_array_equal(per_again, per)
        np.testing.assert_array_equal(again, ens.decision_scores_)


# ---- 3. LODA ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", [1, 7, 100])
@pytest.mark.parametrize("S", [1, 17, 33])
@pytest.mark.parametrize("d", [1, 5, 67])
def test_loda_scores_match_the_restatement_within_one_float32_ulp(d, S, k):
    """The rows and subspaces of the HBOS test; k below, well below and above the 64 projections a wave takes at a time."""
    import vgan_amd
    from vgan_amd.outlier import loda_projections
    X, Y = _rows(d)
    feats = _features(d, S, seed=5)
    proba = _proba(S)
    for B in (2, 10):
        ens = vgan_amd.SubspaceLODA(_mask(d, feats), proba, n_projections=k, n_bins=B, seed=k).fit(X)
        features, weights = loda_projections([len(f) for f in feats], k, k)
        assert len(ens.projection_features_) == len(ens.projection_weights_) == S
        for a, b, c, e in zip(ens.projection_features_, features, ens.projection_weights_, weights):
            assert a.dtype.kind == "i" and c.dtype == np.float64
            np.testing.assert_array_equal(a, b)
            np.testing.assert_array_equal(c, e)
        want, want_edges, want_counts = restate_loda_parts(X, None, feats, ens.projection_features_, ens.projection_weights_, B)
        assert ens.bin_edges_.dtype == np.float64 and ens.bin_edges_.shape == (S, k, B + 1)
        assert ens.histograms_.dtype == np.int64 and ens.histograms_.shape == (S, k, B)
        np.testing.assert_array_equal(ens.bin_edges_.view(np.uint64), want_edges.view(np.uint64))
        np.testing.assert_array_equal(ens.histograms_, want_counts)
        per = ens.per_subspace_scores_
        _check_loda(per, want)
        np.testing.assert_allclose(ens.decision_scores_, proba @ per.astype(np.float64), rtol=1e-12, atol=0)
        got, per_new = ens.decision_function(Y, return_per_subspace=True)
        _check_loda(per_new, restate_loda(X, Y, feats, ens.projection_features_, ens.projection_weights_, B))
        np.testing.assert_allclose(got, proba @ per_new.astype(np.float64), rtol=1e-12, atol=0)
        again, per_again = ens.decision_function(X, return_per_subspace=True)
        np.testing.assert_array_equal(per_again, per)
        np.testing.assert_array_equal(again, ens.decision_scores_)


# ---- 4. determinism --------------------------------------------------------------------------------------------------------
def test_everything_is_bit_identical_for_every_chunking_and_run():
    import vgan_amd
    from vgan_amd.outlier import hbos_chunk_rows, loda_chunks
    n, d, S = 1000, 20, 7
    X, Y = tied_data(n, d, seed=31), tied_data(333, d, seed=32)
    feats = _features(d, S, seed=2)
    dims = [len(f) for f in feats]
    proba = np.full(S, 1.0 / S)
    hbos, loda = [], []
    for chunks in (1, 1, 2, 5):
        ws = (8 * d + 4 * S) * (n // chunks)
        assert -(-n // hbos_chunk_rows(d, S, ws)) == chunks
        ens = vgan_amd.SubspaceHBOS(_mask(d, feats), proba, n_bins=33, workspace_bytes=ws).fit(X)
        hbos.append((ens.per_subspace_scores_, ens.decision_scores_, ens.bin_edges_, ens.histograms_,
                     *ens.decision_function(Y, return_per_subspace=True)))
        ws = 4 * sum((w + 3) // 4 * 4 for w in dims) * (n // chunks)
        rows, ranges = loda_chunks(dims, n, ws)
        assert len(ranges) == 1 and -(-n // rows) == chunks
        ens = vgan_amd.SubspaceLODA(_mask(d, feats), proba, n_projections=70, n_bins=10, seed=3, workspace_bytes=ws).fit(X)
        loda.append((ens.per_subspace_scores_, ens.decision_scores_, ens.bin_edges_, ens.histograms_,
                     *ens.decision_function(Y, return_per_subspace=True)))
    # single rows and the subspaces split into ranges: below a packed row of every subspace
    ws = 4 * sum((w + 3) // 4 * 4 for w in dims) - 1
    rows, ranges = loda_chunks(dims, 40, ws)
    assert rows == 1 and len(ranges) == 2
    for runs in (hbos, loda):
        for other in runs[1:]:
            for a, b in zip(runs[0], other):
                assert a.dtype == b.dtype and np.array_equal(a, b)
    few = [vgan_amd.SubspaceLODA(_mask(d, feats), proba, n_projections=70, n_bins=10, seed=3, workspace_bytes=w).fit(X[:40]) for w in
           (1 << 30, ws)]
    for name in ("per_subspace_scores_", "decision_scores_", "bin_edges_", "histograms_"):
        assert np.array_equal(getattr(few[0], name), getattr(few[1], name))
    # the first subspace fitted alone: the same projections (the host rule draws them first), the same bits
    alone_h = vgan_amd.SubspaceHBOS(_mask(d, feats[:1]), [1.0], n_bins=33).fit(X)
    assert np.array_equal(alone_h.per_subspace_scores_[0], hbos[0][0][0])
    assert np.array_equal(alone_h.bin_edges_, hbos[0][2]) and np.array_equal(alone_h.histograms_, hbos[0][3])
    alone = vgan_amd.SubspaceLODA(_mask(d, feats[:1]), [1.0], n_projections=70, n_bins=10, seed=3).fit(X)
    assert np.array_equal(alone.per_subspace_scores_[0], loda[0][0][0])
    assert np.array_equal(alone.bin_edges_[0], loda[0][2][0]) and np.array_equal(alone.histograms_[0], loda[0][3][0])
    assert np.array_equal(alone.decision_function(Y, return_per_subspace=True)[1][0], loda[0][5][0])


# ---- 5. the shared tail ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("method", ["hbos", "loda"])
def test_normalize_max_predict_and_predict_proba(method):
    import vgan_amd
    X = _planted()
    Xr, Y = np.ascontiguousarray(X[:1500]), np.ascontiguousarray(X[1400:])
    feats = [[0, 1], [0, 1, 2], [4, 7], list(range(10))]
    proba = np.array([0.4, 0.3, 0.2, 0.1])
    tail = dict(normalize="robust", combination="max", contamination=0.05)
    if method == "hbos":
        ens = vgan_amd.SubspaceHBOS(_mask(10, feats), proba, **tail).fit(Xr)
        _check_hbos(ens.per_subspace_scores_, Xr, None, feats, 10)
    else:
        ens = vgan_amd.SubspaceLODA(_mask(10, feats), proba, n_projections=20, **tail).fit(Xr)
        _check_loda(ens.per_subspace_scores_, restate_loda(Xr, None, feats, ens.projection_features_, ens.projection_weights_, 10))
    per = ens.per_subspace_scores_
    c, w = _check_stats(ens, "robust")
    _check_scores(ens.decision_scores_, per, proba, c, w, "max")
    assert ens.threshold_ == np.percentile(ens.decision_scores_, 95.0)
    np.testing.assert_array_equal(ens.labels_, (ens.decision_scores_ > ens.threshold_).astype(int))
    assert ens.labels_.shape == (1500,) and 0 < ens.labels_.sum() <= 75
    got, per_new = ens.decision_function(Y, return_per_subspace=True)
    _check_scores(got, per_new, proba, c, w, "max")  # the statistics of the fit
    np.testing.assert_array_equal(per_new[:, :100], per[:, 1400:])  # fit excludes nothing
    np.testing.assert_array_equal(ens.predict(Y), (got > ens.threshold_).astype(int))
    p = ens.predict_proba(Y)
    assert p.shape == (620, 2)
    np.testing.assert_allclose(p, restate_proba(ens.decision_scores_, got, "linear"), rtol=1e-12, atol=1e-15)


# ---- 6. NaN input ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("method", ["hbos", "loda"])
def test_nan_input_returns(method):
    import vgan_amd
    X, Y = tied_data(300, 6, seed=41), tied_data(50, 6, seed=42)
    X[17, 2] = np.nan
    Y[3, 0] = np.nan
    m = _mask(6, [[0, 1, 2], [3, 4, 5]])
    ens = (vgan_amd.SubspaceHBOS(m, [0.5, 0.5]) if method == "hbos" else vgan_amd.SubspaceLODA(m, [0.5, 0.5], n_projections=9)).fit(X)
    assert ens.decision_scores_.shape == (300,) and ens.per_subspace_scores_.shape == (2, 300)
    got, per = ens.decision_function(Y, return_per_subspace=True)
    assert got.shape == (50,) and per.shape == (2, 50)


# ---- 7. through the model --------------------------------------------------------------------------------------------------
def test_vgan_outlier_ensemble_hbos_and_loda_end_to_end():
    import vgan_amd
    X = _planted()[:, :10]
    model = vgan_amd.VGAN_no_kl(epochs=2)
    model.fit(X)
    ens = model.outlier_ensemble(method="hbos", n_neighbors=3, X=X)  # n_neighbors is ignored; draws model.subspaces
    assert isinstance(ens, vgan_amd.SubspaceHBOS)
    S = model.subspaces.shape[0]
    feats = [np.flatnonzero(model.subspaces[s]) for s in range(S)]
    per = ens.per_subspace_scores_
    assert per.shape == (S, X.shape[0]) and np.isfinite(per).all()
    _check_hbos(per, X, None, feats, 10)
    _check_scores(ens.decision_scores_, per, model.proba, None, None, "sum")
    assert ens.predict_proba(X[:50]).shape == (50, 2)
    ens = model.outlier_ensemble(method="loda", n_projections=7, X=X)
    assert isinstance(ens, vgan_amd.SubspaceLODA)
    per = ens.per_subspace_scores_
    assert per.shape == (S, X.shape[0]) and np.isfinite(per).all() and (per >= 0).all()
    _check_loda(per, restate_loda(X, None, feats, ens.projection_features_, ens.projection_weights_, 10))
    _check_scores(ens.decision_scores_, per, model.proba, None, None, "sum")
    assert ens.predict_proba(X[:50]).shape == (50, 2)
