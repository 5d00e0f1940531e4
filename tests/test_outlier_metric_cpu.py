"""Manhattan, Chebyshev, Minkowski and cosine metrics of the neighbour search, CPU tier: the float64 restatements of
outlier_metric_ref.py pinned to scipy and sklearn, the two recipes that motivate the metrics, the host checks of
SubspaceEnsemble and the argument checks of the new C-ABI entries."""
import numpy as np
import pytest

from outlier_metric_ref import metric_dists, metric_neighbors, roc_auc
from test_outlier_cpu import restate_lof

SCIPY = [("manhattan", None, "cityblock", {}), ("chebyshev", None, "chebyshev", {}), ("minkowski", 0.5, "minkowski", {"p": 0.5}),
         ("minkowski", 3.0, "minkowski", {"p": 3.0}), ("cosine", None, "cosine", {})]


def _data(n, d, seed):
    return np.random.default_rng(seed).normal(size=(n, d))


# ---- the restatements against scipy and sklearn ------------------------------------------------------------------------------
@pytest.mark.parametrize("metric,p,name,kw", SCIPY)
def test_restated_distances_match_scipy(metric, p, name, kw):
    distance = pytest.importorskip("scipy.spatial.distance")
    X, Y = _data(60, 9, 0), _data(25, 9, 1)
    feats = np.array([0, 2, 3, 5, 8])
    want = distance.cdist(Y[:, feats], X[:, feats], name, **kw)
    np.testing.assert_allclose(metric_dists(Y, X, feats, metric, p), want, rtol=1e-12, atol=0)


@pytest.mark.parametrize("metric,p,name,kw", SCIPY)
def test_restated_lists_match_sklearn_brute_force(metric, p, name, kw):
    neighbors = pytest.importorskip("sklearn.neighbors")
    X, Y = _data(200, 6, 2), _data(40, 6, 3)
    feats = np.array([1, 3, 4, 5])
    k = 7
    nn = neighbors.NearestNeighbors(n_neighbors=k, algorithm="brute", metric=name, **kw).fit(X[:, feats])
    d_self, i_self = nn.kneighbors()
    dist, idx = metric_neighbors(X, X, feats, k, True, metric, p)
    np.testing.assert_array_equal(idx[:, :k], i_self)
    np.testing.assert_allclose(dist[:, :k], d_self, rtol=1e-9)
    d_new, i_new = nn.kneighbors(Y[:, feats])
    dist, idx = metric_neighbors(Y, X, feats, k, False, metric, p)
    np.testing.assert_array_equal(idx[:, :k], i_new)
    np.testing.assert_allclose(dist[:, :k], d_new, rtol=1e-9)


@pytest.mark.parametrize("metric,p,name,kw", SCIPY)
def test_restated_lof_matches_sklearn(metric, p, name, kw):
    neighbors = pytest.importorskip("sklearn.neighbors")
    X, Y = _data(300, 5, 4), _data(50, 5, 5) * 1.5
    feats = np.array([0, 2, 4])
    k = 10
    dr, ir = metric_neighbors(X, X, feats, k, True, metric, p)
    lof = neighbors.LocalOutlierFactor(n_neighbors=k, algorithm="brute", metric=name, **kw).fit(X[:, feats])
    np.testing.assert_allclose(restate_lof(dr, ir, dr, ir, k), -lof.negative_outlier_factor_, rtol=1e-9)
    nov = neighbors.LocalOutlierFactor(n_neighbors=k, algorithm="brute", metric=name, novelty=True, **kw).fit(X[:, feats])
    dq, iq = metric_neighbors(Y, X, feats, k, False, metric, p)
    np.testing.assert_allclose(restate_lof(dr, ir, dq, iq, k), -nov.score_samples(Y[:, feats]), rtol=1e-9)


def test_cosine_zero_rows_lie_at_distance_one_from_every_row():
    X = np.array([[0.0, 0.0, 5.0], [1.0, 0.0, 7.0], [0.0, 0.0, -2.0], [2.0, 0.0, 1.0], [-1.0, 0.0, 0.0], [0.0, 3.0, 9.0]])
    feats = np.array([0, 1])  # rows 0 and 2 are zero over these features
    D = metric_dists(X, X, feats, "cosine")
    assert (D[0] == 1.0).all() and (D[2] == 1.0).all() and (D[:, 0] == 1.0).all() and (D[:, 2] == 1.0).all()
    assert D[1, 3] == 0.0 and D[1, 4] == 2.0 and D[1, 5] == 1.0  # parallel, opposite, orthogonal
    dist, idx = metric_neighbors(X, X, feats, 3, True, "cosine")
    assert idx[0, :3].tolist() == [1, 2, 3] and dist[0, :3].tolist() == [1.0, 1.0, 1.0]  # ties by index, self excluded
    assert idx[1, :3].tolist() == [3, 0, 2] and dist[1, :3].tolist() == [0.0, 1.0, 1.0]


def test_minkowski_family_gives_zero_for_duplicates_and_orders_ties_by_index():
    X = np.array([[1.0, 2.0], [3.0, 1.0], [1.0, 2.0], [0.0, 2.0], [1.0, 2.0]])
    for metric, p in (("manhattan", None), ("chebyshev", None), ("minkowski", 0.5), ("minkowski", 3.0)):
        dist, idx = metric_neighbors(X, X, np.array([0, 1]), 3, True, metric, p)
        assert idx[0, :3].tolist() == [2, 4, 3] and dist[0, :2].tolist() == [0.0, 0.0]


# ---- the two recipes ------------------------------------------------------------------------------------------------------------
def recipe_heavy(seed):
    """Heavy tails: 1000 x 100 Student-t(2) features; rows 0..19 are shifted by 2 in 60 features."""
    rng = np.random.default_rng(seed)
    X = rng.standard_t(2, size=(1000, 100))
    X[:20, :60] += 2.0
    return X.astype(np.float32), 20


def recipe_bright(seed):
    """Brightness: every row is one pattern times a log-normal scale; rows 0..19 carry five times the angular noise."""
    rng = np.random.default_rng(seed)
    n, d = 1000, 50
    base = np.abs(rng.normal(size=d)) + 0.5
    s = np.exp(rng.normal(0, 0.7, size=(n, 1)))
    X = s * (base + 0.05 * rng.normal(size=(n, d)))
    X[:20] = s[:20] * (base + 0.05 * rng.normal(size=(20, d)) + 0.25 * rng.normal(size=(20, d)))
    return X.astype(np.float32), 20


def recipe_auc(X, n_out, metric, p=None, k=10):
    dist, _ = metric_neighbors(X, X, np.arange(X.shape[1]), k, True, metric, p)
    return roc_auc(dist[:, k - 1], n_out)


@pytest.mark.parametrize("seed", range(5))
def test_recipe_heavy_tails_favour_small_p(seed):
    X, n_out = recipe_heavy(seed)
    half, l1, l2 = (recipe_auc(X, n_out, *m) for m in (("minkowski", 0.5), ("manhattan",), ("euclidean",)))
    assert half > l1 > l2, (half, l1, l2)
    assert half >= 0.93 and l2 <= 0.80, (half, l2)


@pytest.mark.parametrize("seed", range(5))
def test_recipe_brightness_needs_the_cosine_distance(seed):
    X, n_out = recipe_bright(seed)
    assert recipe_auc(X, n_out, "cosine") >= 0.999
    for m in (("euclidean",), ("manhattan",), ("minkowski", 0.5), ("chebyshev",)):
        assert recipe_auc(X, n_out, *m) <= 0.91, m


# ---- host checks ----------------------------------------------------------------------------------------------------------------
def _mask(widths, d=64):
    m = np.zeros((len(widths), d), bool)
    for s, w in enumerate(widths):
        m[s, :w] = True
    return m


def test_check_metric_names_aliases_and_p():
    from vgan_amd.outlier import check_metric
    assert check_metric("euclidean") == check_metric("l2") == check_metric("minkowski") == check_metric("minkowski", 2) == ("euclidean", None)
    assert check_metric("manhattan") == check_metric("l1") == check_metric("cityblock") == check_metric("minkowski", 1.0) == ("manhattan", None)
    assert check_metric("chebyshev") == ("chebyshev", None) and check_metric("cosine") == ("cosine", None)
    assert check_metric("minkowski", 0.5) == ("minkowski", 0.5) and check_metric("minkowski", 8) == ("minkowski", 8.0)
    for bad in ("mahalanobis", "hamming", None, 2, lambda a, b: 0.0):
        with pytest.raises(ValueError, match="metric must be one of"):
            check_metric(bad)
    for bad in (0, -1.0, 8.5, float("inf"), float("nan"), "2", True):
        with pytest.raises(ValueError, match="p must be a finite float"):
            check_metric("minkowski", bad)
    for metric in ("euclidean", "manhattan", "chebyshev", "cosine", "l1"):
        with pytest.raises(ValueError, match="p is the exponent of metric='minkowski'"):
            check_metric(metric, 2.0)


def test_constructor_metric_keywords_and_value_errors(monkeypatch):
    import vgan_amd
    m, w = _mask([3, 40]), [0.5, 0.5]
    ens = vgan_amd.SubspaceEnsemble(m, w)
    assert (ens.metric, ens.p) == ("euclidean", None)
    ens = vgan_amd.SubspaceEnsemble(m, w, method="lof", metric="minkowski", p=0.5)
    assert (ens.metric, ens.p, ens.engine) == ("minkowski", 0.5, "auto")
    assert vgan_amd.SubspaceEnsemble(m, w, metric="l1").metric == "manhattan"
    assert vgan_amd.SubspaceEnsemble(m, w, metric="minkowski", p=2).metric == "euclidean"
    assert vgan_amd.SubspaceEnsemble(m, w, metric="cosine", engine="gram").metric == "cosine"
    with pytest.raises(ValueError, match="'kde' takes the Euclidean distance only"):
        vgan_amd.SubspaceEnsemble(m, w, method="kde", metric="manhattan")
    vgan_amd.SubspaceEnsemble(m, w, method="kde", metric="l2")
    with pytest.raises(ValueError, match="p is the exponent"):
        vgan_amd.SubspaceEnsemble(m, w, p=3)
    with pytest.raises(ValueError, match="p must be a finite float"):
        vgan_amd.SubspaceEnsemble(m, w, metric="minkowski", p=9)
    with pytest.raises(ValueError, match="metric must be one of"):
        vgan_amd.SubspaceEnsemble(m, w, metric="mahalanobis")
    for metric, p in (("manhattan", None), ("chebyshev", None), ("minkowski", 3)):
        for engine in ("exact", "gram"):
            with pytest.raises(ValueError, match="one distance producer"):
                vgan_amd.SubspaceEnsemble(m, w, metric=metric, p=p, engine=engine)
    with pytest.raises(ValueError, match="'cosine' runs on the Gram engine"):
        vgan_amd.SubspaceEnsemble(m, w, metric="cosine", engine="exact")
    with pytest.raises(ValueError, match="engine must be"):
        vgan_amd.SubspaceEnsemble(m, w, metric="cosine", engine="fast")


def test_metric_and_p_are_keyword_only_arguments_of_the_class_call():
    import inspect
    import vgan_amd
    params = inspect.signature(vgan_amd.SubspaceEnsemble).parameters
    assert list(params)[-2:] == ["metric", "p"] and list(params)[:2] == ["subspaces", "proba"]
    assert params["metric"].kind is params["p"].kind is inspect.Parameter.KEYWORD_ONLY
    assert (params["metric"].default, params["p"].default) == ("euclidean", None)
    assert "metric" not in inspect.signature(vgan_amd.SubspaceEnsemble.__init__).parameters
    ens = vgan_amd.SubspaceEnsemble(_mask([3, 40]), [0.5, 0.5], "lof", 7, metric="chebyshev")
    assert type(ens) is vgan_amd.SubspaceEnsemble and (ens.method, ens.n_neighbors, ens.metric) == ("lof", 7, "chebyshev")
    with pytest.raises(TypeError):
        vgan_amd.SubspaceEnsemble(_mask([3, 40]), [0.5, 0.5], distance="chebyshev")


def test_plan_forms_one_engine_group_for_the_other_metrics(monkeypatch):
    import vgan_amd
    from vgan_amd.outlier import ENGINE_ENV
    m = _mask([3, 40, 31, 32, 33, 5])
    w = np.full(6, 1 / 6)
    assert len(vgan_amd.SubspaceEnsemble(m, w).plan.chunks(100, 1 << 30)) == 2  # Euclidean: the groups split at d_s = 32
    for env in (None, "gram", "exact"):
        if env is None:
            monkeypatch.delenv(ENGINE_ENV, raising=False)
        else:
            monkeypatch.setenv(ENGINE_ENV, env)  # ignored by the Minkowski family, and by cosine
        for metric, p, gram in (("manhattan", None, False), ("chebyshev", None, False), ("minkowski", 0.5, False), ("cosine", None, True)):
            ens = vgan_amd.SubspaceEnsemble(m, w, metric=metric, p=p)
            assert ens.plan.order.tolist() == list(range(6)) and (ens.plan.gram == gram).all()
            assert ens.plan.chunks(100, 1 << 30) == [(0, 6, gram)]


def test_build_ensemble_and_the_models_pass_metric_and_p_through():
    import inspect
    import vgan_amd
    from vgan_amd.hics import HiCS
    from vgan_amd.outlier import build_ensemble
    ens = build_ensemble(_mask([3, 40]), [0.5, 0.5], method="lof", n_neighbors=7, metric="minkowski", p=0.5)
    assert isinstance(ens, vgan_amd.SubspaceEnsemble) and (ens.method, ens.n_neighbors, ens.metric, ens.p) == ("lof", 7, "minkowski", 0.5)
    with pytest.raises(TypeError):
        build_ensemble(_mask([3, 40]), [0.5, 0.5], method="abod", metric="manhattan")  # not built for SubspaceABOD
    for owner in (HiCS, vgan_amd.VGAN if hasattr(vgan_amd, "VGAN") else None):
        if owner is not None:
            assert any(v.kind is inspect.Parameter.VAR_KEYWORD for v in inspect.signature(owner.outlier_ensemble).parameters.values())
    h = HiCS.__new__(HiCS)
    h.subspaces, h.proba = _mask([3, 40]), np.array([0.5, 0.5])
    ens = h.outlier_ensemble(method="knn", metric="cosine")
    assert ens.metric == "cosine" and ens.plan.gram.all()


def test_fit_with_a_metric_rejects_bad_data_before_the_device_is_touched():
    import vgan_amd
    X = np.random.default_rng(0).normal(size=(5, 64)).astype(np.float32)
    with pytest.raises(ValueError, match=r"n_neighbors \+ 1 reference rows \(6\), got 5"):
        vgan_amd.SubspaceEnsemble(_mask([3, 40]), [0.5, 0.5], metric="manhattan").fit(X)


# ---- C ABI: argument checks without a GPU ----------------------------------------------------------------------------------------
def test_metric_entries_reject_bad_arguments_without_gpu():
    import ctypes
    import vgan_amd
    lib = vgan_amd.lib.load()
    null = None
    buf = ctypes.create_string_buffer(256)
    p = ctypes.cast(ctypes.addressof(buf) + (-ctypes.addressof(buf)) % 16, ctypes.c_void_p)  # 16-byte aligned, never read
    odd = ctypes.c_void_p(p.value + 4)

    def rejected(rc):
        msg = lib.vgan_last_error()
        return rc == 1 and b"bad argument" in msg and b"outlier.hip" in msg

    knn = lib.vgan_outlier_knn_metric  # Pq nq Pr nr feat_off col_off first count k exclude_self metric p splits part_d part_i nbr stream
    for metric in (0, 4, 5, -1):  # Euclidean and cosine go through vgan_outlier_knn
        assert rejected(knn(p, 10, p, 10, p, p, 0, 1, 5, 0, metric, 1.0, 1, null, null, p, null)), metric
    for bad_p in (0.0, -1.0, 8.5, float("inf"), float("nan")):
        assert rejected(knn(p, 10, p, 10, p, p, 0, 1, 5, 0, 3, bad_p, 1, null, null, p, null)), bad_p
    assert rejected(knn(p, 10, p, 4, p, p, 0, 1, 5, 0, 1, 0.0, 1, null, null, p, null))  # nr < k
    assert rejected(knn(p, 5, p, 5, p, p, 0, 1, 5, 1, 1, 0.0, 1, null, null, p, null))  # nr < k + 1, self excluded
    assert rejected(knn(p, 10, p, 5, p, p, 0, 1, 5, 1, 1, 0.0, 1, null, null, p, null))  # self excluded, nq != nr
    assert rejected(knn(p, 10, p, 10, p, p, 0, 1, 0, 0, 1, 0.0, 1, null, null, p, null))  # k = 0
    assert rejected(knn(p, 10, p, 10, p, p, 0, 1, 33, 0, 2, 0.0, 1, null, null, p, null))  # k > 32
    assert rejected(knn(odd, 10, p, 10, p, p, 0, 1, 5, 0, 1, 0.0, 1, null, null, p, null))  # unaligned query block
    assert rejected(knn(p, 10, odd, 10, p, p, 0, 1, 5, 0, 2, 0.0, 1, null, null, p, null))  # unaligned reference block
    assert rejected(knn(p, 10, p, 10, p, p, 0, 1, 5, 0, 1, 0.0, 0, null, null, p, null))  # splits = 0
    assert rejected(knn(p, 10, p, 10, p, p, 0, 1, 5, 0, 1, 0.0, 65536, p, p, p, null))  # splits > 65535
    assert rejected(knn(p, 10, p, 10, p, p, 0, 1, 5, 0, 1, 0.0, 3, null, null, p, null))  # split without workspace
    assert rejected(knn(null, 10, p, 10, p, p, 0, 1, 5, 0, 1, 0.0, 1, null, null, p, null))
    pack = lib.vgan_outlier_pack_unit  # X ldx n d feat feat_off col_off first count packed sq stream
    assert rejected(pack(null, 4, 10, 4, p, p, p, 0, 1, p, null, null))
    assert rejected(pack(p, 2, 10, 4, p, p, p, 0, 1, p, null, null))  # ldx < d
    assert rejected(pack(p, 4, 10, 4, p, p, p, 0, 0, p, null, null))  # no subspace
    assert rejected(pack(p, 4, 10, 4, p, p, p, 0, 1, odd, null, null))  # unaligned block
    refine = lib.vgan_outlier_refine_metric  # Xq ldq nq Xr ldr nr d feat feat_off first count nbr k metric p out_idx out_dist kdist stream
    assert rejected(refine(p, 4, 10, p, 4, 10, 4, p, p, 0, 1, p, 5, 5, 0.0, p, p, null, null))  # unknown metric
    assert rejected(refine(p, 4, 10, p, 4, 10, 4, p, p, 0, 1, p, 5, -1, 0.0, p, p, null, null))
    assert rejected(refine(p, 4, 10, p, 4, 10, 4, p, p, 0, 1, p, 5, 3, 0.0, p, p, null, null))  # p = 0
    assert rejected(refine(p, 4, 10, p, 4, 10, 4, p, p, 0, 1, p, 5, 3, float("nan"), p, p, null, null))
    assert rejected(refine(p, 4, 10, p, 4, 3, 4, p, p, 0, 1, p, 5, 1, 0.0, p, p, null, null))  # nr < k
    assert rejected(refine(null, 4, 10, p, 4, 10, 4, p, p, 0, 1, p, 5, 4, 0.0, p, p, null, null))
