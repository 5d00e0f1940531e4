"""The every-row checks of outlier_checks.py, CPU tier: they accept what is right (the restatement's own lists and scores,
and a float32 numpy emulation of each distance engine followed by the float64 refinement) and refuse what is subtly
wrong (one mutation per test), on every adversarial data case, d_s in {40, 200, 784} of 784 features, k in {5, 32}, at
fit (777 rows, self excluded) and for 300 new rows."""
import functools

import numpy as np
import pytest

import outlier_checks as oc
from test_outlier_cpu import restate_knn_score, restate_lof, restate_neighbors
from test_outlier_kde_cpu import restate_bandwidth, restate_kde_from_sq_dists, restate_sq_dists

NR, NQ, DIM = 777, 300, 784
WIDTHS = [40, 200, 784]
KS = [5, 32]
MODES = ["fit", "new"]
GRID = [(c, ds) for c in oc.ADVERSARIAL for ds in WIDTHS]
grid = pytest.mark.parametrize("case,ds", GRID)


@functools.lru_cache(maxsize=None)
def _data(case):
    return oc.adversarial_pair(case, NR, NQ, DIM, seed=5)


@functools.lru_cache(maxsize=None)
def _setup(case, ds, mode, seed=0):
    """(Xq, Xr, feats, D2, exclude_self) of a case: D2 the float64 squared distances of the mode's query rows."""
    Xr, Xn = _data(case)
    feats = np.sort(np.random.default_rng(ds + seed).choice(DIM, ds, replace=False))
    Xq = Xr if mode == "fit" else Xn
    D2 = restate_sq_dists(Xq, Xr, feats)
    D2.setflags(write=False)
    return Xq, Xr, feats, D2, mode == "fit"


def _select(d2, k, exclude_self):
    """The k best of every row of the (approximate) squared distances d2 on the order (d2, index)."""
    return oc.sorted_sq_dists(np.asarray(d2, dtype=np.float64), k, exclude_self)[1][:, :k]


def _lists(D2, k, exclude_self, ranked_by=None):
    """Refined lists of the selection that ranks by `ranked_by` (default: the true D2)."""
    return oc.refine_lists(_select(D2 if ranked_by is None else ranked_by, k, exclude_self), D2)


def emulate_gram(Xq, Xr, feats):
    """float32 |q|^2 + |r|^2 - 2 q.r on operands centred with the float32 column mean of the reference rows, clamped at 0."""
    c = Xr[:, feats].astype(np.float64).mean(axis=0).astype(np.float32)
    Q, R = Xq[:, feats] - c, Xr[:, feats] - c
    assert Q.dtype == np.float32 and R.dtype == np.float32
    sq, sr = (Q * Q).sum(axis=1, dtype=np.float32), (R * R).sum(axis=1, dtype=np.float32)
    return np.maximum(sq[:, None] + sr[None, :] - np.float32(2) * (Q @ R.T), np.float32(0))


def emulate_exact(Xq, Xr, feats):
    """float32 running sum of squared float32 differences, features in order."""
    d2 = np.zeros((Xq.shape[0], Xr.shape[0]), np.float32)
    for f in feats:
        e = Xq[:, f, None] - Xr[None, :, f]
        d2 += e * e
    assert d2.dtype == np.float32
    return d2


EMULATE = {"gram": emulate_gram, "exact": emulate_exact}


def _refused(check, *args, **kwargs):
    with pytest.raises(AssertionError):
        check(*args, **kwargs)


# ---- the helpers themselves --------------------------------------------------------------------------------------------
def test_sorted_sq_dists_is_restate_neighbors():
    for mode in MODES:
        Xq, Xr, feats, D2, excl = _setup("scales", 40, mode)
        for k in [1, 32]:
            d, i = oc.sorted_sq_dists(D2, k, excl)
            rd, ri = restate_neighbors(Xq, Xr, feats, k, exclude_self=excl)
            np.testing.assert_array_equal(d, rd)
            np.testing.assert_array_equal(i, ri)
    d, i = oc.sorted_sq_dists(np.arange(6.0).reshape(2, 3), 4, False)  # fewer rows than k + 1: padded
    assert np.isinf(d[:, 3:]).all() and (i[:, 3:] == -1).all()
    G = np.random.default_rng(0).integers(-2, 3, size=(60, 3)).astype(np.float32)  # an integer grid: ties everywhere
    for excl in [True, False]:
        d, i = oc.sorted_sq_dists(restate_sq_dists(G, G, np.arange(3)), 4, excl)
        rd, ri = restate_neighbors(G, G, np.arange(3), 4, exclude_self=excl)
        np.testing.assert_array_equal(d, rd)
        np.testing.assert_array_equal(i, ri)


@pytest.mark.parametrize("case", oc.ADVERSARIAL)
def test_adversarial_data_is_float32_and_has_the_stated_shape_of_trouble(case):
    Xr, Xq = oc.adversarial_pair(case, 400, 100, 64, seed=1)
    assert Xr.dtype == Xq.dtype == np.float32 and Xr.shape == (400, 64) and Xq.shape == (100, 64)
    assert np.isfinite(Xr).all() and np.isfinite(Xq).all()
    mean, std = Xr.astype(np.float64).mean(axis=0), Xr.astype(np.float64).std(axis=0)
    if case == "offset100":
        assert (np.abs(mean - 100) < 1).all() and (np.abs(std - 1) < 0.3).all()
    if case == "scales":
        assert std.max() / std.min() > 1e4
        np.testing.assert_allclose(Xq.astype(np.float64).std(axis=0), std, rtol=0.5)  # the same feature scales
    if case == "lowrank":
        norms = np.sqrt((Xr.astype(np.float64) ** 2).sum(axis=1))
        d = np.sqrt(restate_sq_dists(Xr, Xr, np.arange(64)))[np.triu_indices(400, 1)]
        assert norms.std() / norms.mean() < 0.05 and d.max() / d.min() > 20
    if case == "shifted_query":
        assert (np.abs(mean) < 0.3).all() and (np.abs(Xq.astype(np.float64).mean(axis=0) - 5) < 0.5).all()
    with pytest.raises(ValueError):
        oc.adversarial("nope", 4, 4, 0)


def test_d2_tolerance_is_the_two_bounds_of_the_project():
    Xq, Xr, feats, D2, _ = _setup("offset100", 40, "new")
    A = Xr[:, feats].astype(np.float64)
    c = A.mean(axis=0)
    qn = ((Xq[:, feats].astype(np.float64) - c) ** 2).sum(axis=1)
    want = 64 * oc.EPS32 * np.sqrt(40) * (qn + ((A - c) ** 2).sum(axis=1).max())
    np.testing.assert_allclose(oc.d2_tolerance("gram", Xq, Xr, feats)[:, 0], want, rtol=1e-14)
    np.testing.assert_allclose(oc.d2_tolerance("exact", Xq, Xr, feats[:38], D2), (40 + 2) * oc.EPS32 * D2, rtol=1e-14)
    with pytest.raises(ValueError):
        oc.d2_tolerance("fast", Xq, Xr, feats)


# ---- what must pass ----------------------------------------------------------------------------------------------------
@grid
def test_the_restatements_own_lists_and_scores_pass(case, ds):
    for mode in MODES:
        Xq, Xr, feats, D2, excl = _setup(case, ds, mode)
        for k in KS:
            D, I = _lists(D2, k, excl)
            for engine in oc.ENGINES:
                assert oc.check_neighbor_lists(D, I, Xq, Xr, feats, k, excl, engine, D2=D2) == 0.0
                for how in ["largest", "mean", "median"]:
                    oc.check_knn_scores(restate_knn_score(D.astype(np.float64), k, how), Xq, Xr, feats, k, how, excl, engine,
                                        D2=D2)
            Df, If = _lists(_setup(case, ds, "fit")[3], k, True)
            oc.check_lof_scores(restate_lof(Df.astype(np.float64), If, D.astype(np.float64), I, k), Df, If, D, I, k)
        h = restate_bandwidth("scott", NR, ds)
        for engine in oc.ENGINES:
            assert oc.check_kde_scores(restate_kde_from_sq_dists(D2, ds, h, excl), Xq, Xr, feats, h, excl, engine, D2=D2) == 0.0


@pytest.mark.parametrize("engine", oc.ENGINES)
@grid
def test_a_float32_emulation_of_each_engine_passes(case, ds, engine):
    """The emulated engine's d2 error stays inside d2_tolerance on every pair (the premise of the sandwich), and its refined
    lists and the kNN / LOF scores taken from them pass on every row."""
    lists = {}
    for mode in MODES:
        Xq, Xr, feats, D2, excl = _setup(case, ds, mode)
        d2 = EMULATE[engine](Xq, Xr, feats)
        tol = oc.d2_tolerance(engine, Xq, Xr, feats, D2)
        assert (np.abs(d2.astype(np.float64) - D2) <= tol).all()
        for k in KS:
            D, I = lists[mode, k] = _lists(D2, k, excl, ranked_by=d2)
            assert oc.check_neighbor_lists(D, I, Xq, Xr, feats, k, excl, engine, D2=D2) <= 1.0
            for how in ["largest", "mean", "median"]:
                oc.check_knn_scores(restate_knn_score(D.astype(np.float64), k, how), Xq, Xr, feats, k, how, excl, engine, D2=D2)
    for k in KS:
        Df, If = lists["fit", k]
        for mode in MODES:
            D, I = lists[mode, k]
            oc.check_lof_scores(restate_lof(Df.astype(np.float64), If, D.astype(np.float64), I, k), Df, If, D, I, k)


# ---- mutations: each must be refused -----------------------------------------------------------------------------------
def _each(case, ds):
    for mode in MODES:
        Xq, Xr, feats, D2, excl = _setup(case, ds, mode)
        for k in KS:
            for engine in oc.ENGINES:
                yield Xq, Xr, feats, D2, excl, k, engine


@grid
def test_lists_without_the_last_reference_tile_are_refused(case, ds):
    """Where no row has a neighbour in the last tile the lists are the right ones and pass (the queries of "shifted_query"
    all share a few neighbours at small k); every list the dropped tile changes is refused."""
    first = 64 * ((NR - 1) // 64)
    changed = 0
    for Xq, Xr, feats, D2, excl, k, engine in _each(case, ds):
        seen = np.array(D2)
        seen[:, first:] = np.inf
        D, I = _lists(D2, k, excl, ranked_by=seen)
        if np.array_equal(I, _lists(D2, k, excl)[1]):
            oc.check_neighbor_lists(D, I, Xq, Xr, feats, k, excl, engine, D2=D2)
            continue
        changed += 1
        _refused(oc.check_neighbor_lists, D, I, Xq, Xr, feats, k, excl, engine, D2=D2)
    assert changed >= 4  # at fit, both k and both engines, on every case


@grid
def test_lists_of_one_slice_of_three_are_refused(case, ds):
    ntiles = -(-NR // 64)
    per = -(-ntiles // 3)
    for Xq, Xr, feats, D2, excl, k, engine in _each(case, ds):
        for slice_ in range(3):
            seen = np.full(D2.shape, np.inf)
            lo, hi = 64 * per * slice_, min(NR, 64 * per * (slice_ + 1))
            seen[:, lo:hi] = D2[:, lo:hi]
            D, I = _lists(D2, k, excl, ranked_by=seen)
            _refused(oc.check_neighbor_lists, D, I, Xq, Xr, feats, k, excl, engine, D2=D2)


@grid
def test_the_own_index_kept_at_fit_is_refused(case, ds):
    Xq, Xr, feats, D2, excl = _setup(case, ds, "fit")
    for k in KS:
        D, I = _lists(D2, k, False)
        assert (I[:, 0] == np.arange(NR)).all()
        for engine in oc.ENGINES:
            _refused(oc.check_neighbor_lists, D, I, Xq, Xr, feats, k, True, engine, D2=D2)
        # in one row only, in the last position
        D, I = _lists(D2, k, True)
        D[400, -1], I[400, -1] = 0.0, 400
        D[400], I[400] = np.roll(D[400], 1), np.roll(I[400], 1)
        for engine in oc.ENGINES:
            _refused(oc.check_neighbor_lists, D, I, Xq, Xr, feats, k, True, engine, D2=D2)


@grid
def test_a_repeated_index_is_refused(case, ds):
    for Xq, Xr, feats, D2, excl, k, engine in _each(case, ds):
        D, I = _lists(D2, k, excl)
        D[7, k - 1], I[7, k - 1] = D[7, k - 2], I[7, k - 2]
        _refused(oc.check_neighbor_lists, D, I, Xq, Xr, feats, k, excl, engine, D2=D2)


@grid
def test_two_swapped_positions_are_refused(case, ds):
    for Xq, Xr, feats, D2, excl, k, engine in _each(case, ds):
        D, I = _lists(D2, k, excl)
        a, b = k // 2, k // 2 + 1
        D[11, [a, b]], I[11, [a, b]] = D[11, [b, a]], I[11, [b, a]]
        _refused(oc.check_neighbor_lists, D, I, Xq, Xr, feats, k, excl, engine, D2=D2)
        # the indices alone: every distance still in order, but no longer that of its index
        D, I = _lists(D2, k, excl)
        I[11, [a, b]] = I[11, [b, a]]
        _refused(oc.check_neighbor_lists, D, I, Xq, Xr, feats, k, excl, engine, D2=D2)


@grid
def test_the_nearest_neighbour_replaced_by_a_farther_row_is_refused(case, ds):
    for Xq, Xr, feats, D2, excl, k, engine in _each(case, ds):
        far = oc.sorted_sq_dists(D2, k + 6, excl)[1]
        sel = np.concatenate([far[:, 1:k], far[:, k + 5:k + 6]], axis=1)  # ranks 2 .. k and k + 6
        D, I = oc.refine_lists(sel, D2)
        _refused(oc.check_neighbor_lists, D, I, Xq, Xr, feats, k, excl, engine, D2=D2)
        for how in ["largest", "mean", "median"]:
            _refused(oc.check_knn_scores, restate_knn_score(D.astype(np.float64), k, how), Xq, Xr, feats, k, how, excl, engine,
                     D2=D2)


@grid
def test_distances_scaled_by_one_part_in_ten_thousand_are_refused(case, ds):
    for Xq, Xr, feats, D2, excl, k, engine in _each(case, ds):
        D, I = _lists(D2, k, excl)
        for factor in [1 + 1e-4, 1 - 1e-4]:
            Dm = (D.astype(np.float64) * factor).astype(np.float32)
            _refused(oc.check_neighbor_lists, Dm, I, Xq, Xr, feats, k, excl, engine, D2=D2)
        # scores of the true lists, scaled down: below the true score
        got = restate_knn_score(D.astype(np.float64), k, "mean") * (1 - 1e-4)
        _refused(oc.check_knn_scores, got, Xq, Xr, feats, k, "mean", excl, engine, D2=D2)


def _lof_with_kdist(kdist, D_fit, I_fit, D_q, I_q, k):
    """restate_lof with the k-distances of the reference rows given from outside."""
    lrd_ref = 1.0 / (np.maximum(kdist[I_fit], D_fit).mean(axis=1) + 1e-10)
    lrd_q = 1.0 / (np.maximum(kdist[I_q], D_q).mean(axis=1) + 1e-10)
    return (lrd_ref[I_q] / lrd_q[:, None]).mean(axis=1)


@grid
def test_lof_with_the_k_distances_of_another_subspace_is_refused(case, ds):
    """The processing-order mix-up: kdist row of subspace s' read for subspace s."""
    other_fit = _setup(case, 200, "fit")[3] if ds == DIM else _setup(case, ds, "fit", seed=1)[3]  # another subspace
    for k in KS:
        Df, If = _lists(_setup(case, ds, "fit")[3], k, True)
        Df, If = Df.astype(np.float64), If.astype(np.int64)
        wrong = _lists(other_fit, k, True)[0][:, k - 1].astype(np.float64)
        np.testing.assert_allclose(_lof_with_kdist(Df[:, k - 1], Df, If, Df, If, k), restate_lof(Df, If, Df, If, k), rtol=1e-14)
        for mode in MODES:
            Xq, Xr, feats, D2, excl = _setup(case, ds, mode)
            D, I = _lists(D2, k, excl)
            got = _lof_with_kdist(wrong, Df, If, D.astype(np.float64), I.astype(np.int64), k)
            _refused(oc.check_lof_scores, got, Df, If, D, I, k)


@grid
def test_kde_with_one_reference_row_left_out_of_the_sum_is_refused(case, ds):
    h = restate_bandwidth("scott", NR, ds)
    for mode in MODES:
        Xq, Xr, feats, D2, excl = _setup(case, ds, mode)
        gone = int(oc.sorted_sq_dists(D2, 1, excl)[1][0, 0])  # the nearest row of query 0
        short = np.array(D2)
        short[:, gone] = np.inf  # its term is 0, N stays
        got = restate_kde_from_sq_dists(short, ds, h, excl)
        for engine in oc.ENGINES:
            _refused(oc.check_kde_scores, got, Xq, Xr, feats, h, excl, engine, D2=D2)


@grid
def test_the_upper_middle_taken_as_the_median_of_an_even_k_is_refused(case, ds):
    for Xq, Xr, feats, D2, excl, k, engine in _each(case, ds):
        if k % 2:
            continue
        D, _ = _lists(D2, k, excl)
        _refused(oc.check_knn_scores, D[:, k // 2].astype(np.float64), Xq, Xr, feats, k, "median", excl, engine, D2=D2)
