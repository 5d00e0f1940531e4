"""Manhattan, Chebyshev, Minkowski and cosine metrics of the neighbour search on the device (csrc/outlier_metric.hpp and the
metric entries of csrc/outlier.hip through vgan_amd.SubspaceEnsemble), every row held to the float64 restatements of
outlier_metric_ref.py.  Nothing is filtered: where the float32 selection may choose another neighbour at a near-tie the check
is the sandwich derived there from the kernel's arithmetic."""
import functools

import numpy as np
import pytest

import outlier_checks as oc
import outlier_metric_ref as mr
from test_outlier_metric_cpu import recipe_auc, recipe_bright, recipe_heavy

pytestmark = pytest.mark.gpu

METRICS = [("manhattan", None), ("chebyshev", None), ("minkowski", 0.5), ("minkowski", 3.0), ("cosine", None)]
KS = [1, 8, 9, 16, 17, 32]
LARGEST_USE = {}


def _mask(d, feature_lists):
    m = np.zeros((len(feature_lists), d), bool)
    for s, feats in enumerate(feature_lists):
        m[s, feats] = True
    return m


def _report(capsys, line):
    with capsys.disabled():
        print("\n    " + line, end="")


def _name(metric, p):
    return metric if p is None else f"{metric}(p={p:g})"


def _kw(metric, p):
    return {"metric": metric} if p is None else {"metric": metric, "p": p}


# ---- lists ---------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _case(case, ds):
    nr, nq, d = (200, 70, 784) if ds == 391 else (130, 70, 128)
    Xr, Xq = oc.adversarial_pair(case, nr, nq, d, seed=11)
    feats = np.sort(np.random.default_rng(100 + ds).choice(d, ds, replace=False))
    return Xr, Xq, feats, d


@pytest.mark.parametrize("ds", [1, 3, 4, 5, 31, 32, 33, 37, 100, 391])
@pytest.mark.parametrize("case", oc.ADVERSARIAL)
def test_lists_every_row(case, ds, capsys):
    """nr = 130 is two full reference tiles plus 2 rows, nq = 70 one full query tile plus 6; the widths cover one feature, the
    padding to 4, the 32-feature LDS block and its neighbours, and several blocks; k covers the three K instances at and
    just above their edges."""
    import vgan_amd
    Xr, Xq, feats, d = _case(case, ds)
    lines = []
    for metric, p in METRICS:
        D_fit, D_new = mr.metric_dists(Xr, Xr, feats, metric, p), mr.metric_dists(Xq, Xr, feats, metric, p)
        use = 0.0
        for k in KS:
            ens = vgan_amd.SubspaceEnsemble(_mask(d, [feats]), [1.0], n_neighbors=k, **_kw(metric, p)).fit(Xr)
            for Q, excl, D_all, (D, I) in ((Xr, True, D_fit, ens.kneighbors()), (Xq, False, D_new, ens.kneighbors(Xq))):
                assert D.dtype == np.float32 and I.dtype == np.int32 and D.shape == I.shape == (1, Q.shape[0], k)
                use = max(use, mr.check_metric_lists(D[0], I[0], Q, Xr, feats, k, excl, metric, p, D_all=D_all))
        LARGEST_USE[_name(metric, p)] = max(LARGEST_USE.get(_name(metric, p), 0.0), use)
        lines.append(f"{_name(metric, p)} {use:.2e}")
    _report(capsys, f"{case:14s} d_s {ds:3d}  sandwich use: " + "  ".join(lines))


def test_report_largest_sandwich_use(capsys):
    _report(capsys, "largest sandwich use so far: " + "  ".join(f"{m} {u:.2e}" for m, u in sorted(LARGEST_USE.items())))
    assert all(u <= 1.0 for u in LARGEST_USE.values())


# ---- exact ties ----------------------------------------------------------------------------------------------------------------
def _grid(n, d, seed):
    rng = np.random.default_rng(seed)
    X = rng.integers(-3, 4, size=(n, d)).astype(np.float32)
    if n == 300:
        X[[10, 150, 299]] = X[3]  # planted duplicates of row 3
        X[[64, 65]] = X[63]  # and across a tile edge
    return X


@pytest.mark.parametrize("metric", ["manhattan", "chebyshev"])
@pytest.mark.parametrize("k", [5, 32])
def test_integer_grid_lists_are_the_restatement_bit_for_bit(metric, k):
    """Small integers: every difference, sum and maximum is exact in float32, so the selection has no freedom and the lists
    equal the restatement on every row; duplicates come first at distance 0 in index order."""
    import vgan_amd
    d, feats = 6, np.array([0, 2, 3, 5])
    Xr, Xq = _grid(300, d, 1), _grid(70, d, 2)
    Xq[7] = Xr[3]
    ens = vgan_amd.SubspaceEnsemble(_mask(d, [feats]), [1.0], n_neighbors=k, metric=metric).fit(Xr)
    for Q, excl, (D, I) in ((Xr, True, ens.kneighbors()), (Xq, False, ens.kneighbors(Xq))):
        dist, idx = mr.metric_neighbors(Q, Xr, feats, k, excl, metric)
        np.testing.assert_array_equal(I[0], idx[:, :k])
        np.testing.assert_array_equal(D[0], dist[:, :k].astype(np.float32))
    D, I = ens.kneighbors()
    assert I[0, 3, :3].tolist() == [10, 150, 299] and (D[0, 3, :3] == 0).all()
    assert I[0, 63, :2].tolist() == [64, 65] and I[0, 64, :2].tolist() == [63, 65]
    D, I = ens.kneighbors(Xq)
    assert I[0, 7, :4].tolist() == [3, 10, 150, 299] and (D[0, 7, :4] == 0).all()


def test_cosine_zero_rows_follow_the_zero_row_rule():
    import vgan_amd
    d, feats, k = 8, np.array([1, 2, 5, 6]), 6
    rng = np.random.default_rng(4)
    Xr = rng.normal(size=(300, d)).astype(np.float32)
    Xq = rng.normal(size=(70, d)).astype(np.float32)
    zero = [5, 77, 140]
    Xr[np.ix_(zero, feats)] = 0.0  # zero over F_s, not elsewhere
    Xq[np.ix_([9], feats)] = 0.0
    ens = vgan_amd.SubspaceEnsemble(_mask(d, [feats]), [1.0], n_neighbors=k, metric="cosine").fit(Xr)
    D, I = ens.kneighbors()
    mr.check_metric_lists(D[0], I[0], Xr, Xr, feats, k, True, "cosine")
    for q in zero:  # distance exactly 1 to every row, ties by index, self excluded
        assert (D[0, q] == 1.0).all() and I[0, q].tolist() == [i for i in range(k + 1) if i != q][:k]
    listed = np.isin(I[0], zero)
    assert (D[0][listed] == 1.0).all()
    D, I = ens.kneighbors(Xq)
    mr.check_metric_lists(D[0], I[0], Xq, Xr, feats, k, False, "cosine")
    assert (D[0, 9] == 1.0).all() and I[0, 9].tolist() == list(range(k))
    assert np.isfinite(ens.decision_function(Xq)).all()


# ---- independence of the split, the chunking and the company ------------------------------------------------------------------
@pytest.mark.parametrize("metric,p", METRICS)
def test_lists_do_not_depend_on_splits_chunks_or_company(metric, p):
    import vgan_amd
    d, k = 128, 9
    rng = np.random.default_rng(6)
    lists = [np.sort(rng.choice(d, w, replace=False)) for w in (3, 31, 32, 33, 40, 100)]
    Xr, Xq = oc.adversarial_pair("normal", 300, 70, d, seed=8)
    w = np.full(6, 1 / 6)

    def both(ens):
        ens.fit(Xr)
        return ens.kneighbors() + ens.kneighbors(Xq)

    base = both(vgan_amd.SubspaceEnsemble(_mask(d, lists), w, n_neighbors=k, splits=1, **_kw(metric, p)))
    for kw in (dict(splits=2), dict(splits=3), dict(), dict(splits=1, workspace_bytes=1), dict(splits=3, workspace_bytes=1)):
        got = both(vgan_amd.SubspaceEnsemble(_mask(d, lists), w, n_neighbors=k, **kw, **_kw(metric, p)))
        for a, b in zip(base, got):
            np.testing.assert_array_equal(a, b, err_msg=str(kw))
    for s in (0, 2, 5):
        got = both(vgan_amd.SubspaceEnsemble(_mask(d, [lists[s]]), [1.0], n_neighbors=k, **_kw(metric, p)))
        for a, b in zip(base, got):
            np.testing.assert_array_equal(a[s], b[0])


# ---- existing behaviour ------------------------------------------------------------------------------------------------------------
def _outputs(ens, Xr, Xq):
    ens.fit(Xr)
    return (ens.decision_scores_, ens.per_subspace_scores_) + ens.kneighbors() + ens.kneighbors(Xq) + (ens.decision_function(Xq),)


@pytest.mark.parametrize("engine", ["auto", "exact", "gram"])
@pytest.mark.parametrize("method", ["knn", "lof"])
def test_euclidean_and_minkowski_2_are_the_default_bit_for_bit(method, engine):
    import vgan_amd
    d = 64
    rng = np.random.default_rng(7)
    lists = [np.sort(rng.choice(d, w, replace=False)) for w in (3, 33, 17, 40)]
    Xr, Xq = oc.adversarial_pair("scales", 300, 70, d, seed=3)
    w = [0.1, 0.2, 0.3, 0.4]
    want = _outputs(vgan_amd.SubspaceEnsemble(_mask(d, lists), w, method=method, n_neighbors=7, engine=engine), Xr, Xq)
    for kw in (dict(metric="euclidean"), dict(metric="l2"), dict(metric="minkowski", p=2), dict(metric="minkowski")):
        got = _outputs(vgan_amd.SubspaceEnsemble(_mask(d, lists), w, method=method, n_neighbors=7, engine=engine, **kw), Xr, Xq)
        for a, b in zip(want, got):
            np.testing.assert_array_equal(a, b, err_msg=str(kw))


def test_minkowski_1_is_manhattan_bit_for_bit():
    import vgan_amd
    d = 64
    lists = [np.arange(5), np.arange(10, 50)]
    Xr, Xq = oc.adversarial_pair("lowrank", 300, 70, d, seed=3)
    want = _outputs(vgan_amd.SubspaceEnsemble(_mask(d, lists), [0.5, 0.5], method="lof", metric="manhattan"), Xr, Xq)
    for kw in (dict(metric="minkowski", p=1), dict(metric="l1"), dict(metric="cityblock")):
        got = _outputs(vgan_amd.SubspaceEnsemble(_mask(d, lists), [0.5, 0.5], method="lof", **kw), Xr, Xq)
        for a, b in zip(want, got):
            np.testing.assert_array_equal(a, b)


def test_refine_metric_with_the_euclidean_metric_is_refine_bit_for_bit():
    import torch
    import vgan_amd
    d, k, nq = 64, 9, 70
    lists = [np.arange(5), np.arange(10, 50), np.arange(20, 53)]
    Xr, Xq = oc.adversarial_pair("scales", 300, nq, d, seed=3)
    ens = vgan_amd.SubspaceEnsemble(_mask(d, lists), [0.2, 0.3, 0.5], n_neighbors=k).fit(Xr)
    rng = np.random.default_rng(0)
    nbr = np.stack([np.stack([rng.choice(300, k, replace=False) for _ in range(nq)]) for _ in lists]).astype(np.int32)
    nbr_d = torch.as_tensor(nbr, device="cuda")
    Xq_d = torch.as_tensor(Xq, device="cuda")
    out = []
    for metric in (None, (0, 0.0), (3, 2.0)):
        idx = torch.zeros_like(nbr_d)
        dist = torch.zeros(3, nq, k, dtype=torch.float32, device="cuda")
        kd = torch.zeros(3, nq, dtype=torch.float32, device="cuda")
        if metric is None:
            ens.ops.outlier_refine(Xq_d, ens._X, ens._table, 0, 3, nbr_d, k, idx, dist, kd)
        else:
            ens.ops.outlier_refine_metric(Xq_d, ens._X, ens._table, 0, 3, nbr_d, k, metric[0], metric[1], idx, dist, kd)
        out.append((idx.cpu().numpy(), dist.cpu().numpy(), kd.cpu().numpy()))
    for got in out[1:]:
        for a, b in zip(out[0], got):
            np.testing.assert_array_equal(a, b)
    assert (out[0][1][:, :, -1] == out[0][2]).all() and (out[0][1] > 0).all()


# ---- scores ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("metric,p", METRICS)
def test_lof_and_knn_scores_every_row(metric, p):
    import vgan_amd
    d, k = 128, 10
    rng = np.random.default_rng(9)
    lists = [np.sort(rng.choice(d, w, replace=False)) for w in (5, 40)]
    Xr, Xq = oc.adversarial_pair("lowrank", 300, 70, d, seed=13)
    ens = vgan_amd.SubspaceEnsemble(_mask(d, lists), [0.4, 0.6], method="lof", n_neighbors=k, **_kw(metric, p)).fit(Xr)
    (D_fit, I_fit), (D_new, I_new) = ens.kneighbors(), ens.kneighbors(Xq)
    per_new = ens.decision_function(Xq, return_per_subspace=True)[1]
    for s, feats in enumerate(lists):
        mr.check_metric_lists(D_fit[s], I_fit[s], Xr, Xr, feats, k, True, metric, p)
        mr.check_metric_lists(D_new[s], I_new[s], Xq, Xr, feats, k, False, metric, p)
        oc.check_lof_scores(ens.per_subspace_scores_[s], D_fit[s], I_fit[s], D_fit[s], I_fit[s], k)
        oc.check_lof_scores(per_new[s], D_fit[s], I_fit[s], D_new[s], I_new[s], k)
    for how in ("largest", "mean", "median"):
        ens = vgan_amd.SubspaceEnsemble(_mask(d, lists), [0.4, 0.6], n_neighbors=k, knn_method=how, **_kw(metric, p)).fit(Xr)
        per_new = ens.decision_function(Xq, return_per_subspace=True)[1]
        for s, feats in enumerate(lists):
            mr.check_metric_knn_scores(ens.per_subspace_scores_[s], Xr, Xr, feats, k, how, True, metric, p)
            mr.check_metric_knn_scores(per_new[s], Xq, Xr, feats, k, how, False, metric, p)


def test_the_tail_of_the_ensemble_runs_on_another_metric():
    import vgan_amd
    from vgan_amd.outlier import build_ensemble
    d, k = 64, 8
    lists = [np.arange(5), np.arange(10, 50)]
    Xr, Xq = oc.adversarial_pair("normal", 300, 70, d, seed=13)
    Xr[:6] += 6.0
    ens = vgan_amd.SubspaceEnsemble(_mask(d, lists), [0.4, 0.6], n_neighbors=k, metric="chebyshev", normalize="zscore",
                                    combination="max", contamination=0.05).fit(Xr)
    per = ens.per_subspace_scores_.astype(np.float64)
    t = (per - ens.score_center_[:, None]) / ens.score_scale_[:, None]
    np.testing.assert_allclose(ens.decision_scores_, t.max(axis=0), rtol=1e-12, atol=1e-12)
    assert ens.labels_[:6].all() and ens.labels_.sum() == 15
    got, per_new = ens.decision_function(Xq, return_per_subspace=True)
    t = (per_new.astype(np.float64) - ens.score_center_[:, None]) / ens.score_scale_[:, None]
    np.testing.assert_allclose(got, t.max(axis=0), rtol=1e-12, atol=1e-12)
    np.testing.assert_array_equal(ens.predict(Xq), (got > ens.threshold_).astype(int))
    built = build_ensemble(_mask(d, lists), [0.4, 0.6], method="lof", n_neighbors=k, metric="manhattan").fit(Xr)
    direct = vgan_amd.SubspaceEnsemble(_mask(d, lists), [0.4, 0.6], method="lof", n_neighbors=k, metric="manhattan").fit(Xr)
    np.testing.assert_array_equal(built.decision_scores_, direct.decision_scores_)
    D, I = built.kneighbors()
    for s, feats in enumerate(lists):
        mr.check_metric_lists(D[s], I[s], Xr, Xr, feats, k, True, "manhattan")
        oc.check_lof_scores(built.per_subspace_scores_[s], D[s], I[s], D[s], I[s], k)


# ---- the recipes --------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _restated_auc(recipe, seed, metric, p):
    X, n_out = (recipe_heavy if recipe == "heavy" else recipe_bright)(seed)
    return recipe_auc(X, n_out, metric, p)


@pytest.mark.parametrize("seed", [0, 1])
@pytest.mark.parametrize("recipe,metric,p", [("heavy", "euclidean", None), ("heavy", "manhattan", None), ("heavy", "minkowski", 0.5),
                                             ("bright", "euclidean", None), ("bright", "cosine", None)])
def test_recipe_auc_on_the_device(recipe, metric, p, seed):
    import vgan_amd
    X, n_out = (recipe_heavy if recipe == "heavy" else recipe_bright)(seed)
    ens = vgan_amd.SubspaceEnsemble(np.ones((1, X.shape[1]), bool), [1.0], n_neighbors=10, **_kw(metric, p)).fit(X)
    got, want = mr.roc_auc(ens.decision_scores_, n_out), _restated_auc(recipe, seed, metric, p)
    assert abs(got - want) <= 1e-3, (got, want)
