"""Outlier scoring over subspaces, CPU tier: a float64 numpy restatement of the scoring contract (pinned against sklearn),
the argument checks of the new C-ABI entries, and the host planner of vgan_amd.outlier."""
import numpy as np
import pytest


# ---- float64 restatement of the contract (vgan_amd/outlier.py module docstring) ----------------------------------------
def restate_neighbors(Xq, Xr, feats, k, exclude_self):
    """Sorted (distance, index) neighbour lists of Xq among Xr in the subspace `feats`: dist [nq, k + 1], idx [nq, k + 1]
    (one extra column for the gap checks; inf / -1 when there is no such row)."""
    A = np.asarray(Xq, np.float64)[:, feats]
    B = np.asarray(Xr, np.float64)[:, feats]
    D2 = np.zeros((A.shape[0], B.shape[0]))
    for f in range(A.shape[1]):
        D2 += (A[:, f, None] - B[None, :, f]) ** 2
    D = np.sqrt(D2)
    if exclude_self:
        np.fill_diagonal(D, np.inf)
    order = np.argsort(D, axis=1, kind="stable")[:, :k + 1]  # stable on index order: ties go to the lower index
    dist = np.take_along_axis(D, order, axis=1)
    if order.shape[1] < k + 1:
        pad = k + 1 - order.shape[1]
        order = np.pad(order, ((0, 0), (0, pad)), constant_values=-1)
        dist = np.pad(dist, ((0, 0), (0, pad)), constant_values=np.inf)
    return dist, order


def restate_knn_score(dist, k, knn_method):
    d = dist[:, :k]
    return {"largest": d[:, k - 1], "mean": d.mean(axis=1), "median": np.median(d, axis=1)}[knn_method]


def restate_lof(dist_ref, idx_ref, dist_q, idx_q, k):
    kdist = dist_ref[:, k - 1]
    lrd_ref = 1.0 / (np.maximum(kdist[idx_ref[:, :k]], dist_ref[:, :k]).mean(axis=1) + 1e-10)
    lrd_q = 1.0 / (np.maximum(kdist[idx_q[:, :k]], dist_q[:, :k]).mean(axis=1) + 1e-10)
    return (lrd_ref[idx_q[:, :k]] / lrd_q[:, None]).mean(axis=1)


def restate_ensemble(subspaces, proba, Xtr, Xq=None, method="knn", k=5, knn_method="largest"):
    """(scores float64 [n], per-subspace scores float64 [S, n]) of Xq (None: the training set, self excluded)."""
    per = []
    for s in range(len(subspaces)):
        feats = np.flatnonzero(subspaces[s])
        dq, iq = restate_neighbors(Xtr if Xq is None else Xq, Xtr, feats, k, exclude_self=Xq is None)
        if method == "knn":
            per.append(restate_knn_score(dq, k, knn_method))
        else:
            dr, ir = (dq, iq) if Xq is None else restate_neighbors(Xtr, Xtr, feats, k, exclude_self=True)
            per.append(restate_lof(dr, ir, dq, iq, k))
    per = np.array(per)
    scores = np.zeros(per.shape[1])
    for s in range(per.shape[0]):
        scores += float(proba[s]) * per[s]
    return scores, per


def _untied(n, d, seed):
    return np.random.default_rng(seed).normal(size=(n, d))


# ---- the restatement against sklearn --------------------------------------------------------------------------------
@pytest.mark.parametrize("k", [1, 5, 20])
def test_restated_neighbors_match_sklearn(k):
    neighbors = pytest.importorskip("sklearn.neighbors")
    X, Y = _untied(300, 6, 0), _untied(50, 6, 1)
    feats = np.array([1, 3, 4])
    nn = neighbors.NearestNeighbors(n_neighbors=k).fit(X[:, feats])
    d_self, i_self = nn.kneighbors()  # X=None: each row's own index excluded
    dist, idx = restate_neighbors(X, X, feats, k, exclude_self=True)
    np.testing.assert_array_equal(idx[:, :k], i_self)
    np.testing.assert_allclose(dist[:, :k], d_self, rtol=1e-12)
    d_new, i_new = nn.kneighbors(Y[:, feats])
    dist, idx = restate_neighbors(Y, X, feats, k, exclude_self=False)
    np.testing.assert_array_equal(idx[:, :k], i_new)
    np.testing.assert_allclose(dist[:, :k], d_new, rtol=1e-12)


@pytest.mark.parametrize("k", [3, 10])
def test_restated_lof_matches_sklearn(k):
    neighbors = pytest.importorskip("sklearn.neighbors")
    X, Y = _untied(400, 5, 2), _untied(60, 5, 3) * 1.5
    feats = np.array([0, 2, 4])
    dr, ir = restate_neighbors(X, X, feats, k, exclude_self=True)
    lof = neighbors.LocalOutlierFactor(n_neighbors=k).fit(X[:, feats])
    np.testing.assert_allclose(restate_lof(dr, ir, dr, ir, k), -lof.negative_outlier_factor_, rtol=1e-10)
    nov = neighbors.LocalOutlierFactor(n_neighbors=k, novelty=True).fit(X[:, feats])
    dq, iq = restate_neighbors(Y, X, feats, k, exclude_self=False)
    np.testing.assert_allclose(restate_lof(dr, ir, dq, iq, k), -nov.score_samples(Y[:, feats]), rtol=1e-10)


def test_restated_knn_scores_match_pyod_definitions():
    X = _untied(200, 4, 4)
    feats = np.array([0, 1, 2, 3])
    dist, _ = restate_neighbors(X, X, feats, 6, exclude_self=True)
    assert np.array_equal(restate_knn_score(dist, 6, "largest"), dist[:, 5])
    np.testing.assert_allclose(restate_knn_score(dist, 6, "mean"), dist[:, :6].mean(1))
    np.testing.assert_allclose(restate_knn_score(dist, 6, "median"), 0.5 * (dist[:, 2] + dist[:, 3]))


def test_restated_ties_go_to_the_lower_index_and_keep_duplicates():
    X = np.array([[0.0], [1.0], [0.0], [2.0], [0.0]])
    dist, idx = restate_neighbors(X, X, np.array([0]), 3, exclude_self=True)
    assert idx[0, :3].tolist() == [2, 4, 1] and dist[0, :2].tolist() == [0.0, 0.0]
    assert idx[2, :3].tolist() == [0, 4, 1]
    dist, idx = restate_neighbors(X[:1], X, np.array([0]), 3, exclude_self=False)
    assert idx[0, :3].tolist() == [0, 2, 4]


# ---- C ABI: argument checks without a GPU ------------------------------------------------------------------------------
def test_outlier_entries_reject_bad_arguments_without_gpu():
    import ctypes
    import vgan_amd
    lib = vgan_amd.lib.load()
    null = None
    buf = ctypes.create_string_buffer(256)
    p = ctypes.cast(ctypes.addressof(buf) + (-ctypes.addressof(buf)) % 16, ctypes.c_void_p)  # 16-byte aligned, never read

    def rejected(rc):
        msg = lib.vgan_last_error()
        return rc == 1 and b"bad argument" in msg and b"outlier.hip" in msg

    assert rejected(lib.vgan_outlier_pack(null, 4, 10, 4, null, p, p, p, 0, 1, p, null, null))
    assert rejected(lib.vgan_outlier_pack(p, 2, 10, 4, null, p, p, p, 0, 1, p, null, null))  # ldx < d
    assert rejected(lib.vgan_outlier_pack(p, 4, 10, 4, null, p, p, p, 0, 0, p, null, null))  # no subspace
    knn = lib.vgan_outlier_knn
    assert rejected(knn(p, p, 10, p, p, 10, p, p, 0, 1, 0, 0, 0, 1, null, null, p, null))  # k = 0
    assert rejected(knn(p, p, 10, p, p, 10, p, p, 0, 1, 33, 0, 0, 1, null, null, p, null))  # k > 32
    assert rejected(knn(p, p, 10, p, p, 5, p, p, 0, 1, 5, 1, 0, 1, null, null, p, null))  # self excluded, nq != nr
    assert rejected(knn(p, p, 5, p, p, 5, p, p, 0, 1, 5, 1, 0, 1, null, null, p, null))  # nr < k + 1
    assert rejected(knn(p, p, 10, p, p, 10, p, p, 0, 1, 5, 0, 2, 1, null, null, p, null))  # unknown engine
    assert rejected(knn(p, null, 10, p, null, 10, p, p, 0, 1, 5, 0, 1, 1, null, null, p, null))  # gram without norms
    assert rejected(knn(p, p, 10, p, p, 10, p, p, 0, 1, 5, 0, 0, 3, null, null, p, null))  # split without workspace
    assert rejected(lib.vgan_outlier_refine(p, 4, 10, p, 4, 3, 4, p, p, 0, 1, p, 5, p, p, null, null))  # nr < k
    assert rejected(lib.vgan_outlier_refine(null, 4, 10, p, 4, 10, 4, p, p, 0, 1, p, 5, p, p, null, null))
    score = lib.vgan_outlier_score
    assert rejected(score(p, p, 10, 5, 1, 5, null, null, 0, p, null, 10, null, null))  # unknown method
    assert rejected(score(p, p, 10, 5, 1, 3, null, null, 10, null, null, 10, p, null))  # lrd without kdist
    assert rejected(score(p, p, 10, 5, 1, 4, p, null, 10, p, null, 10, null, null))  # lof without lrd
    assert rejected(score(p, p, 10, 5, 1, 0, null, null, 0, p, null, 9, null, null))  # ld_score < nq
    assert rejected(lib.vgan_outlier_combine(p, 5, 2, 10, p, p, null))  # ld < n
    assert rejected(lib.vgan_outlier_combine(null, 10, 2, 10, p, p, null))


# ---- host planner --------------------------------------------------------------------------------------------------
def test_planner_feature_lists_and_offsets():
    from vgan_amd.outlier import SubspacePlan
    m = np.zeros((4, 40), bool)
    m[0, [1, 3]] = True
    m[1, :35] = True
    m[2, [0, 5, 9, 39, 38]] = True
    m[3, [7]] = True
    plan = SubspacePlan(m)  # 35 features -> Gram engine, processed after the others
    assert plan.order.tolist() == [0, 2, 3, 1]
    assert plan.gram.tolist() == [False, False, False, True]
    assert plan.feat_off.tolist() == [0, 2, 7, 8, 43]
    assert plan.col_off.tolist() == [0, 4, 12, 16, 52]
    assert plan.feat[:8].tolist() == [1, 3, 0, 5, 9, 38, 39, 7]
    assert plan.feat[8:].tolist() == list(range(35))
    assert plan.feat.dtype == np.int32 and plan.col_off.dtype == np.int64
    assert plan.given.tolist() == [0, 3, 1, 2]  # given subspace index -> processing position
    np.testing.assert_array_equal(plan.order[plan.given], np.arange(plan.count))
    np.testing.assert_array_equal(plan.given[plan.order], np.arange(plan.count))
    forced = SubspacePlan(m, engine="gram")
    assert forced.order.tolist() == [0, 1, 2, 3] and forced.gram.all()
    assert forced.given.tolist() == [0, 1, 2, 3]
    assert not SubspacePlan(m, engine="exact").gram.any()


def test_planner_chunks_respect_the_byte_limit_and_the_engine_boundary():
    from vgan_amd.outlier import SubspacePlan
    rng = np.random.default_rng(5)
    m = rng.random((30, 64)) < 0.3
    m[:, 0] = True
    plan = SubspacePlan(m, gram_min_dims=20)
    rows = 1000
    widths = (plan.dims + 3) // 4 * 4
    for limit in [1, 40_000, 200_000, 10 ** 9]:
        chunks = plan.chunks(rows, limit)
        covered = [i for first, count, _ in chunks for i in range(first, first + count)]
        assert covered == list(range(plan.count))
        for first, count, gram in chunks:
            assert (plan.gram[first:first + count] == gram).all()
            need = rows * (widths[first:first + count] + 1) * 4
            assert count == 1 or need.sum() <= limit
    assert all(count == 1 for _, count, _ in plan.chunks(rows, 1))
    assert len(plan.chunks(rows, 10 ** 9)) == (2 if plan.gram.any() and not plan.gram.all() else 1)


def _greedy_chunks(plan, need, limit, cap):
    """The chunk loop as ocsvm_chunks, kpca_fit_chunks (cap 65535) and SubspacePlan.chunks (no cap) each spelt it out; need(z):
    the bytes of the subspace at processing position z."""
    out, first = [], 0
    while first < plan.count:
        end, used = first, 0
        while end < plan.count and plan.gram[end] == plan.gram[first] and (cap is None or end - first < cap):
            if end > first and used + need(end) > limit:
                break
            used += need(end)
            end += 1
        out.append((first, end - first, bool(plan.gram[first])))
        first = end
    return out


def test_planner_chunks_with_extra_bytes_and_a_cap_are_the_old_kernel_method_loops():
    from vgan_amd.outlier import SubspacePlan, kpca_fit_chunks, ocsvm_chunks, sos_chunks
    mask = np.zeros((5, 256), bool)
    for s, width in enumerate((1, 3, 17, 33, 200)):
        mask[s, :width] = True
    plan = SubspacePlan(mask)
    assert plan.gram.tolist() == [False, False, False, True, True]
    many = SubspacePlan(np.ones((65536 + 1, 1), bool))
    unlimited = 1 << 62
    for rows in (3, 65, 257):
        # bytes an entry of the rows x rows matrices next to a packed block: none (the two-argument form), OCSVM / SOS, KPCA
        for square, entry in ((0, None), (4, ocsvm_chunks), (12, kpca_fit_chunks)):
            def need(p):
                return lambda z: rows * rows * square + rows * (int((p.dims[z] + 3) // 4 * 4) + 1) * 4
            two = need(plan)(0) + need(plan)(1)  # exactly two subspaces' worth
            for p, limit in ((plan, 1), (plan, two), (plan, 1 << 30), (many, unlimited)):
                want = _greedy_chunks(p, need(p), limit, 65535 if square else None)
                if entry is None:
                    assert p.chunks(rows, limit) == p.chunks(rows, limit, extra_bytes=0, max_count=None) == want
                else:
                    assert entry(p, rows, limit) == p.chunks(rows, limit, extra_bytes=square * rows * rows, max_count=65535) == want
                if square == 4:
                    assert sos_chunks(p, rows, limit) == want
            assert _greedy_chunks(plan, need(plan), two, None)[:2] == [(0, 2, False), (2, 1, False)]
            assert _greedy_chunks(plan, need(plan), two - 1, None)[0] == (0, 1, False)
    # the cap: 65535 subspaces a chunk for the kernel methods, none for the two-argument form
    assert ocsvm_chunks(many, 3, unlimited) == kpca_fit_chunks(many, 3, unlimited) == [(0, 65535, False), (65535, 2, False)]
    assert many.chunks(3, unlimited) == [(0, 65537, False)]


def test_planner_rejects_bad_subspaces():
    from vgan_amd.outlier import SubspacePlan
    m = np.ones((3, 5), bool)
    m[1] = False
    with pytest.raises(ValueError, match="subspace 1 selects no feature"):
        SubspacePlan(m)
    with pytest.raises(ValueError, match="engine"):
        SubspacePlan(np.ones((2, 3), bool), engine="fast")
    assert SubspacePlan(np.array([True, False, True])).count == 1


@pytest.mark.parametrize("k", [0, 33, -1, 2.5, True])
def test_n_neighbors_outside_1_to_32_is_a_value_error(k):
    import vgan_amd
    with pytest.raises(ValueError, match="between 1 and 32"):
        vgan_amd.SubspaceEnsemble(np.ones((1, 3), bool), [1.0], n_neighbors=k)


def test_too_few_reference_rows_is_a_value_error():
    from vgan_amd.outlier import check_reference_rows
    check_reference_rows(6, 5, exclude_self=True)
    check_reference_rows(5, 5, exclude_self=False)
    with pytest.raises(ValueError, match="n_neighbors \\+ 1"):
        check_reference_rows(5, 5, exclude_self=True)
    with pytest.raises(ValueError, match="at least n_neighbors"):
        check_reference_rows(4, 5, exclude_self=False)


def test_bad_method_names_are_value_errors():
    import vgan_amd
    with pytest.raises(ValueError, match="method"):
        vgan_amd.SubspaceEnsemble(np.ones((1, 3), bool), [1.0], method="iforest")
    with pytest.raises(ValueError, match="knn_method"):
        vgan_amd.SubspaceEnsemble(np.ones((1, 3), bool), [1.0], knn_method="max")


# ---- the class without a GPU --------------------------------------------------------------------------------------------
def _mask(d, feature_lists):
    m = np.zeros((len(feature_lists), d), bool)
    for s, feats in enumerate(feature_lists):
        m[s, feats] = True
    return m


def test_defaults_and_constructor_keywords_without_a_gpu():
    import inspect
    import vgan_amd
    params = inspect.signature(vgan_amd.SubspaceEnsemble.__init__).parameters
    assert list(params)[1:] == ["subspaces", "proba", "method", "n_neighbors", "knn_method", "bandwidth", "engine", "splits",
                                "workspace_bytes", "normalize", "combination", "contamination"]
    ens = vgan_amd.SubspaceEnsemble(_mask(6, [[0, 1], [2, 3, 5]]), [0.25, 0.75])
    assert (ens.method, ens.n_neighbors, ens.knn_method, ens.bandwidth) == ("knn", 5, "largest", 1.0)
    assert (ens.engine, ens.splits, ens.workspace_bytes) == ("auto", None, 1 << 30)
    assert ens.normalize is None and ens.combination == "sum" and ens.contamination == 0.1
    assert ens.score_center_ is None and ens.score_scale_ is None and ens.plan.count == 2
    assert ens.proba.dtype == np.float64 and ens.proba.tolist() == [0.25, 0.75]
    ens = vgan_amd.SubspaceEnsemble(_mask(6, [[0, 1], [2, 3, 5]]), [0.5, 0.5], method="kde", n_neighbors=np.int64(7),
                                    knn_method="median", bandwidth="scott", engine="gram", splits=3, workspace_bytes=1 << 20,
                                    normalize="robust", combination="max", contamination=0.05)
    assert (ens.method, ens.n_neighbors, ens.knn_method, ens.bandwidth) == ("kde", 7, "median", "scott")
    assert (ens.engine, ens.splits, ens.workspace_bytes) == ("gram", 3, 1 << 20) and ens.plan.gram.all()
    assert (ens.normalize, ens.combination, ens.contamination) == ("robust", "max", 0.05)
    for kw, match in [(dict(splits=0), "splits"), (dict(splits=70000), "splits"), (dict(engine="fast"), "engine"),
                      (dict(normalize="l2"), "normalize"), (dict(combination="mean"), "combination"),
                      (dict(contamination=0.7), "contamination"), (dict(method="kde", bandwidth=-1.0), "bandwidth")]:
        with pytest.raises(ValueError, match=match):
            vgan_amd.SubspaceEnsemble(_mask(6, [[0, 1], [2, 3, 5]]), [0.5, 0.5], **kw)
    with pytest.raises(ValueError, match="proba has 1 entries for 2 subspaces"):
        vgan_amd.SubspaceEnsemble(_mask(6, [[0, 1], [2, 3, 5]]), [1.0])


def test_fit_rejects_bad_data_before_the_device_is_touched():
    """These raise ValueError with or without a GPU: on the CPU tier a call that reached the device would raise
    VganHipError instead."""
    import vgan_amd
    m = _mask(6, [[0, 1], [2, 3, 5]])
    X = np.random.default_rng(0).normal(size=(5, 6)).astype(np.float32)
    with pytest.raises(ValueError, match=r"n_neighbors \+ 1 reference rows \(6\), got 5"):
        vgan_amd.SubspaceEnsemble(m, [0.5, 0.5]).fit(X)
    with pytest.raises(ValueError, match="KDE fit needs at least 2 reference rows, got 1"):
        vgan_amd.SubspaceEnsemble(m, [0.5, 0.5], method="kde").fit(X[:1])
    with pytest.raises(ValueError, match="X has 5 features, the subspaces 6"):
        vgan_amd.SubspaceEnsemble(m, [0.5, 0.5], n_neighbors=3).fit(X[:, :5])
    with pytest.raises(ValueError, match="2-d"):
        vgan_amd.SubspaceEnsemble(m, [0.5, 0.5], n_neighbors=3).fit(X[0])
    for call in ("decision_function", "predict", "kneighbors"):
        with pytest.raises(RuntimeError, match="SubspaceEnsemble is not fitted"):
            getattr(vgan_amd.SubspaceEnsemble(m, [0.5, 0.5]), call)(X)
    with pytest.raises(ValueError, match="method must be 'linear' or 'unify'"):
        vgan_amd.SubspaceEnsemble(m, [0.5, 0.5]).predict_proba(X, method="erf")
