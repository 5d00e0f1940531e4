"""ECOD over the subspaces on the MI355X (csrc/outlier_ecod.hip through vgan_amd.SubspaceECOD and the ops wrappers), against
the float64 restatement of test_outlier_ecod_cpu.py (pinned to scipy and to hand-worked cases there).

The sort and the counts are exact: bit-equal to numpy.sort, integer-equal to searchsorted.  The bar on a per-subspace score
is one float32 ulp, |got - want| <= 2^-23 |want| with no absolute term: kernel and restatement share the correctly rounded
quotient c / n; their two logs differ by ulps of float64; a sum of at most 67 non-negative terms in any order is within
67 x 2^-53 relative of the exact sum; so only the final rounding to float32 can differ, by one ulp where the float64
values straddle a rounding boundary.  A row whose terms are all 0 has want == 0 and must be exactly 0."""
import numpy as np
import pytest

from test_outlier_ecod_cpu import _mask, restate_counts, restate_ecod, restate_skew_sign, restate_terms, tied_data
from test_outlier_gpu import _planted
from test_outlier_norm_cpu import restate_proba
from test_outlier_norm_gpu import _check_scores, _check_stats

pytestmark = pytest.mark.gpu

ULP32 = 2.0 ** -23


def _run():
    from vgan_amd.outlier import ECOD_SORT_RUN
    return ECOD_SORT_RUN


def _n_grid():
    run = _run()
    return [1, 2, 3, 257, run - 1, run, run + 1, 2 * run + 3]


def _sorted_on_device(X):
    """(ops, device X, device sorted [d, n_pad]) of float32 X [n, d]."""
    import torch
    from vgan_amd.ops import default_ops
    ops = default_ops()
    n, d = X.shape
    Xd = torch.as_tensor(X, device="cuda")
    out = torch.empty(d, 1 << (n - 1).bit_length(), dtype=torch.float32, device="cuda")
    ops.ecod_sort_columns(Xd, out)
    return ops, Xd, out


def _features(d, S, seed):
    """S feature lists over d features: the full set first, then (S >= 2) a single feature (the constant column when d has
    one), then random subsets."""
    rng = np.random.default_rng(seed)
    lists = [list(range(d))]
    if S >= 2:
        lists.append([3 if d > 3 else 0])
    while len(lists) < S:
        keep = np.flatnonzero(rng.random(d) < 0.4)
        lists.append(sorted(set(keep.tolist()) | {int(rng.integers(d))}))
    return lists


def _check_per(got32, want):
    got32 = np.asarray(got32)
    assert got32.dtype == np.float32 and got32.shape == want.shape
    want32 = want.astype(np.float32).astype(np.float64)
    np.testing.assert_allclose(got32.astype(np.float64), want32, rtol=ULP32, atol=0)
    assert (got32[want == 0] == 0).all()


# ---- 1. the column sort ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("d", [1, 5, 67])
@pytest.mark.parametrize("n", range(8))
def test_sorted_columns_equal_numpy_sort_bit_for_bit(n, d):
    """n at 1, 2, 3, an odd size inside one run, the run length and its neighbours, and two runs and a bit (strided stages);
    columns with heavy integer ties, +-0.0, a constant and a descending column."""
    n = _n_grid()[n]
    X = tied_data(n, d, seed=100 + n)
    _, _, out = _sorted_on_device(X)
    got = out.cpu().numpy()
    want = np.sort(X + np.float32(0.0), axis=0).T  # -0.0 + 0.0 is +0.0
    assert got.shape[1] >= n and got.shape[1] < 2 * n
    np.testing.assert_array_equal(got[:, :n].view(np.uint32), np.ascontiguousarray(want).view(np.uint32))
    assert np.isposinf(got[:, n:]).all()


# ---- 2. the skew signs -----------------------------------------------------------------------------------------------------
def test_skew_signs():
    import torch
    n = 1001
    rng = np.random.default_rng(7)
    sym = np.arange(-500, 501).astype(np.float64) + 3.0  # exactly symmetric about 3
    X = np.concatenate([rng.lognormal(size=(n, 1)), -rng.lognormal(size=(n, 1)), np.full((n, 1), -1.25),
                        rng.permutation(sym)[:, None], rng.normal(size=(n, 24))], axis=1).astype(np.float32)
    ops, _, out = _sorted_on_device(X)
    sign = torch.empty(X.shape[1], dtype=torch.int8, device="cuda")
    ops.ecod_skew_sign(out, n, sign)
    got = sign.cpu().numpy().astype(np.int64)
    assert got[:4].tolist() == [1, -1, 0, 0]
    np.testing.assert_array_equal(got, restate_skew_sign(X))


# ---- 3. the tail counts ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", range(8))
def test_tail_counts_equal_searchsorted(n):
    """Queries: the fitted rows themselves (the fit rule: the row is among the n) and new rows holding fitted values (tied
    runs), values below every minimum and above every maximum (the query rule adds the row itself to both counts)."""
    import torch
    n = _n_grid()[n]
    for d in (5, 67):
        X = tied_data(n, d, seed=200 + n)
        ops, Xd, out = _sorted_on_device(X)
        rng = np.random.default_rng(n)
        for rows in (1, 15, 17, 130):
            Y = tied_data(rows, d, seed=300 + rows)
            take = rng.random(Y.shape) < 0.5
            Y[take] = X[rng.integers(n, size=Y.shape), np.arange(d)[None, :]][take]  # values of the fitted columns
            Y[0, 0] = -1e30
            Y[-1, -1] = 1e30
            for Q in ([X, Y] if rows == 130 else [Y]):
                Qd = Xd if Q is X else torch.as_tensor(Q, device="cuda")
                cl = torch.full((Q.shape[0], d), -7, dtype=torch.int32, device="cuda")
                cr = torch.full((Q.shape[0], d), -7, dtype=torch.int32, device="cuda")
                ops.ecod_tail_counts(Qd, out, n, cl, cr)
                want_l, want_r = restate_counts(X, Q)
                np.testing.assert_array_equal(cl.cpu().numpy(), want_l)
                np.testing.assert_array_equal(cr.cpu().numpy(), want_r)
                if Q is X:  # the fit rule never sees a zero count
                    assert want_l.min() >= 1 and want_r.min() >= 1
        assert want_l[0, 0] == 0 and want_r[0, 0] == n and want_l[-1, -1] == n and want_r[-1, -1] == 0


# ---- 4. the scores ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("aggregate", ["dimension", "tail"])
@pytest.mark.parametrize("S", [1, 17, 33])
@pytest.mark.parametrize("d", [1, 5, 67])
def test_scores_match_the_restatement_within_one_float32_ulp(d, S, aggregate):
    """301 fitted and 130 new rows (neither a multiple of the 64-row tile), d off the multiples of 4, S off the multiples of
    16 and 32; the full mask, a single-feature mask on the constant column (every term 0) and random masks."""
    import vgan_amd
    X, Y = tied_data(301, d, seed=11), tied_data(130, d, seed=12)
    Y[:40] = X[:40]
    feats = _features(d, S, seed=5)
    rng = np.random.default_rng(S)
    proba = rng.random(S)
    proba /= proba.sum()
    ens = vgan_amd.SubspaceECOD(_mask(d, feats), proba, aggregate=aggregate).fit(X)
    np.testing.assert_array_equal(ens.skew_sign_, restate_skew_sign(X))
    assert ens.skew_sign_.shape == (d,) and ens.skew_sign_.dtype.kind == "i"
    assert ens.sorted_columns_.shape == (d, 301) and ens.sorted_columns_.dtype == np.float32
    np.testing.assert_array_equal(ens.sorted_columns_, np.sort(X + np.float32(0.0), axis=0).T)
    per = ens.per_subspace_scores_
    want = restate_ecod(X, None, feats, aggregate)
    _check_per(per, want)
    if d > 3 and S >= 2:
        assert (want[1] == 0).all() and (per[1] == 0).all()  # the constant column
    own = proba @ per.astype(np.float64)
    np.testing.assert_allclose(ens.decision_scores_, own, rtol=1e-12, atol=0)
    np.testing.assert_allclose(ens.decision_scores_, proba @ want, rtol=2.4e-7, atol=0)
    got, per_new = ens.decision_function(Y, return_per_subspace=True)
    want_new = restate_ecod(X, Y, feats, aggregate)
    _check_per(per_new, want_new)
    np.testing.assert_allclose(got, proba @ per_new.astype(np.float64), rtol=1e-12, atol=0)
    np.testing.assert_allclose(got, proba @ want_new, rtol=2.4e-7, atol=0)
    # the training rows scored again follow the append rule, not the fit rule
    assert not np.array_equal(per_new[:, :40], per[:, :40])


def test_ensemble_is_a_weighted_sum_of_the_per_feature_terms():
    """aggregate "dimension", no normalisation, "sum": sum_s p_s sum_{f in F_s} O[i, f] = sum_f w_f O[i, f] with w_f = sum_s p_s
    mask[s, f]."""
    import vgan_amd
    d, S = 67, 33
    X, Y = tied_data(500, d, seed=21), tied_data(77, d, seed=22)
    feats = _features(d, S, seed=9)
    m = _mask(d, feats)
    proba = np.random.default_rng(3).random(S)
    proba /= proba.sum()
    w = proba @ m.astype(np.float64)
    ens = vgan_amd.SubspaceECOD(m, proba).fit(X)
    ul, ur, usk = restate_terms(X)
    np.testing.assert_allclose(ens.decision_scores_, np.maximum(np.maximum(ul, ur), usk) @ w, rtol=2.4e-7, atol=0)
    ul, ur, usk = restate_terms(X, Y)
    np.testing.assert_allclose(ens.decision_function(Y), np.maximum(np.maximum(ul, ur), usk) @ w, rtol=2.4e-7, atol=0)


# ---- 5. determinism --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("aggregate", ["dimension", "tail"])
def test_scores_are_bit_identical_for_every_chunking_and_run(aggregate):
    import vgan_amd
    from vgan_amd.outlier import ecod_chunk_rows
    n, d, S = 1000, 20, 7
    X, Y = tied_data(n, d, seed=31), tied_data(333, d, seed=32)
    feats = _features(d, S, seed=2)
    proba = np.full(S, 1.0 / S)
    row_bytes = d * (8 + 8 * (3 if aggregate == "tail" else 1)) + 4 * S
    runs = []
    for chunks in (1, 1, 2, 5):
        ws = row_bytes * (n // chunks)
        assert -(-n // ecod_chunk_rows(d, S, aggregate, ws)) == chunks
        ens = vgan_amd.SubspaceECOD(_mask(d, feats), proba, aggregate=aggregate, workspace_bytes=ws).fit(X)
        runs.append((ens.per_subspace_scores_, ens.decision_scores_, ens.skew_sign_, ens.sorted_columns_,
                     *ens.decision_function(Y, return_per_subspace=True)))
    for other in runs[1:]:
        for a, b in zip(runs[0], other):
            assert a.dtype == b.dtype and np.array_equal(a, b)


# ---- 6. the shared tail ----------------------------------------------------------------------------------------------------
def test_normalize_max_predict_and_predict_proba_on_ecod_scores():
    import vgan_amd
    X = _planted()
    Xr, Y = np.ascontiguousarray(X[:1500]), np.ascontiguousarray(X[1400:])
    feats = [[0, 1], [0, 1, 2], [4, 7], list(range(10))]
    proba = np.array([0.4, 0.3, 0.2, 0.1])
    ens = vgan_amd.SubspaceECOD(_mask(10, feats), proba, normalize="robust", combination="max", contamination=0.05).fit(Xr)
    per = ens.per_subspace_scores_
    _check_per(per, restate_ecod(Xr, None, feats, "dimension"))
    c, w = _check_stats(ens, "robust")
    _check_scores(ens.decision_scores_, per, proba, c, w, "max")
    assert ens.threshold_ == np.percentile(ens.decision_scores_, 95.0)
    np.testing.assert_array_equal(ens.labels_, (ens.decision_scores_ > ens.threshold_).astype(int))
    assert ens.labels_.shape == (1500,) and 0 < ens.labels_.sum() <= 75
    got, per_new = ens.decision_function(Y, return_per_subspace=True)
    _check_per(per_new, restate_ecod(Xr, Y, feats, "dimension"))
    _check_scores(got, per_new, proba, c, w, "max")  # the statistics of the fit
    np.testing.assert_array_equal(ens.predict(Y), (got > ens.threshold_).astype(int))
    p = ens.predict_proba(Y)
    assert p.shape == (620, 2)
    np.testing.assert_allclose(p, restate_proba(ens.decision_scores_, got, "linear"), rtol=1e-12, atol=1e-15)


# ---- 7. NaN input ----------------------------------------------------------------------------------------------------------
def test_nan_input_returns():
    import vgan_amd
    X, Y = tied_data(300, 6, seed=41), tied_data(50, 6, seed=42)
    X[17, 2] = np.nan
    Y[3, 0] = np.nan
    ens = vgan_amd.SubspaceECOD(_mask(6, [[0, 1, 2], [3, 4, 5]]), [0.5, 0.5]).fit(X)
    assert ens.decision_scores_.shape == (300,) and ens.per_subspace_scores_.shape == (2, 300)
    got, per = ens.decision_function(Y, return_per_subspace=True)
    assert got.shape == (50,) and per.shape == (2, 50)


# ---- 8. through the model --------------------------------------------------------------------------------------------------
def test_vgan_outlier_ensemble_ecod_end_to_end():
    import vgan_amd
    X = _planted()[:, :10]
    model = vgan_amd.VGAN_no_kl(epochs=2)
    model.fit(X)
    ens = model.outlier_ensemble(method="ecod", n_neighbors=3, X=X)  # n_neighbors is ignored
    assert isinstance(ens, vgan_amd.SubspaceECOD)
    S = model.subspaces.shape[0]
    feats = [np.flatnonzero(model.subspaces[s]) for s in range(S)]
    per = ens.per_subspace_scores_
    assert per.shape == (S, X.shape[0]) and np.isfinite(per).all() and (per >= 0).all()
    _check_per(per, restate_ecod(X, None, feats, "dimension"))
    _check_scores(ens.decision_scores_, per, model.proba, None, None, "sum")
    ens = model.outlier_ensemble(method="ecod", aggregate="tail", normalize="minmax", X=X)
    _check_per(ens.per_subspace_scores_, restate_ecod(X, None, feats, "tail"))
    assert ens.predict_proba(X[:50]).shape == (50, 2)
