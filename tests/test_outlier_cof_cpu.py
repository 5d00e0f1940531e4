"""Connectivity-based outlier scores (COF) over subspaces, CPU tier: the float64 numpy restatement of the contract of
vgan_amd.SubspaceCOF, its set-based nearest chain pinned to scipy's minimum spanning tree (there is no pyod here to pin it
to; the class docstring says so), hand-checkable cases, the tie rule, the zero-denominator rules and the ceiling, the
restated ensemble, and everything of the class and of the new C-ABI entries that can be checked without a GPU."""
import numpy as np
import pytest

from test_outlier_cpu import restate_neighbors
from test_outlier_norm_cpu import restate_combine, restate_stats

FLT_MAX = float(np.finfo(np.float32).max)
CHAINS = ("sbn", "rank")


@pytest.fixture(autouse=True)
def cof_class():
    """Everything below restates the docstring of this class: without the class there is nothing to restate."""
    import vgan_amd
    return vgan_amd.SubspaceCOF


# ---- float64 restatement of the contract (SubspaceCOF docstring) ---------------------------------------------------------
def restate_pair_sq_dists(Xq, Xr, feats, idx):
    """float64 [nq, k + 1, k + 1]: d2 between the points o_0 = the query row, o_1 .. o_k = the reference rows idx [nq, k], over
    the features `feats` in ascending order, differences first."""
    feats = np.sort(np.asarray(feats))
    A = np.asarray(Xq, np.float64)[:, feats]
    B = np.asarray(Xr, np.float64)[:, feats]
    P = np.concatenate([A[:, None, :], B[np.asarray(idx, np.int64)]], axis=1)
    D2 = np.zeros((P.shape[0], P.shape[1], P.shape[1]))
    for f in range(P.shape[2]):
        D2 += (P[:, :, None, f] - P[:, None, :, f]) ** 2
    return D2


def chain_edges(D2, chain):
    """(e float64 [nq, k], gap float64 [nq]) from the pairwise d2 [nq, k + 1, k + 1] (point 0 is the query): the edges of
    the chain in step order, and the smallest relative gap (runner-up - chosen) / runner-up between the d2 of the chosen
    point and of the runner-up over the steps that had a runner-up (inf for "rank", which selects nothing)."""
    nq, k = D2.shape[0], D2.shape[1] - 1
    rows = np.arange(nq)
    e = np.empty((nq, k))
    gap = np.full(nq, np.inf)
    if chain == "rank":
        for i in range(1, k + 1):
            e[:, i - 1] = np.sqrt(D2[:, i, :i].min(axis=1))
        return e, gap
    assert chain == "sbn"
    dist = D2[:, 0, 1:].copy()  # d2 of every point to the set {o_0}
    rem = np.ones((nq, k), bool)
    for i in range(k):
        masked = np.where(rem, dist, np.inf)
        j = masked.argmin(axis=1)  # the first minimum: a tie goes to the lower list position
        m = masked[rows, j]
        e[:, i] = np.sqrt(m)
        rem[rows, j] = False
        if i < k - 1:
            runner = np.where(rem, dist, np.inf).min(axis=1)
            with np.errstate(invalid="ignore", divide="ignore"):
                gap = np.minimum(gap, np.where(runner > 0, (runner - m) / runner, 0.0))
        dist = np.minimum(dist, D2[rows, j + 1, 1:])
    return e, gap


def restate_cof_chain(Xq, Xr, feats, idx, chain="sbn"):
    """(ac float64 [nq], gap float64 [nq]): the average chaining distance sum_i w_i e_i, w_i = 2 (k + 1 - i) / (k (k + 1)),
    i ascending, of every query row from its list idx [nq, k], and chain_edges' smallest relative gap of the row."""
    e, gap = chain_edges(restate_pair_sq_dists(Xq, Xr, feats, idx), chain)
    k = e.shape[1]
    ac = np.zeros(e.shape[0])
    for i in range(1, k + 1):
        ac += 2.0 * (k + 1 - i) / (k * (k + 1)) * e[:, i - 1]
    return ac, gap


def restate_cof_from_lists(ac_q, ac_ref, idx):
    """float64 [nq]: ac_q k / sum_i ac_ref[idx[:, i]], i ascending; a zero denominator gives exactly 1 where ac_q is 0 too
    and NaN (degenerate) where it is not."""
    idx = np.asarray(idx, np.int64)
    k = idx.shape[1]
    den = np.zeros(idx.shape[0])
    for i in range(k):
        den += np.asarray(ac_ref, np.float64)[idx[:, i]]
    ac_q = np.asarray(ac_q, np.float64)
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        out = ac_q * k / den
    out[(den == 0) & (ac_q == 0)] = 1.0
    out[(den == 0) & (ac_q > 0)] = np.nan
    return out


def to_score32(raw):
    """The float32 the score matrix holds for a float64 score: rounded, a value beyond the float32 range stored as the
    largest finite float32 (never inf); NaN stays."""
    raw = np.asarray(raw, np.float64)
    with np.errstate(over="ignore"):
        out = raw.astype(np.float32)
    out[np.isposinf(out)] = np.float32(FLT_MAX)
    return out


def restate_ceiling(raw32, ceiling=None):
    """The ceiling rule on float32 scores [S, n] with NaN at the degenerate rows: (scores with the ceiling applied, ceiling
    float64 [S], n_degenerate int [S]).  ceiling None: taken from the rows (fit: the largest non-degenerate score, 1 if
    there is none); otherwise the given ceiling is applied (decision_function)."""
    raw32 = np.asarray(raw32, np.float32)
    deg = np.isnan(raw32)
    if ceiling is None:
        ceiling = np.array([raw32[s][~deg[s]].max() if (~deg[s]).any() else 1.0 for s in range(raw32.shape[0])], np.float64)
    out = np.where(deg, np.asarray(ceiling, np.float64).astype(np.float32)[:, None], raw32).astype(np.float32)
    return out, np.asarray(ceiling, np.float64), deg.sum(axis=1)


def restate_cof_ensemble(subspaces, proba, Xtr, Xq=None, k=20, chain="sbn", normalize=None, combination="sum", fitted=None):
    """The whole detector from its own float64 neighbours.  fit (Xq None) returns a dict with scores (float64 [n]), per
    (float32 [S, n], ceiling applied), raw (float64 [S, n], NaN at degenerate rows), ac (float64 [S, n]), ceiling,
    n_degenerate, center, scale (None without normalize) and lists (per subspace, (dist, idx) of restate_neighbors with
    the extra column); scoring new rows takes the dict of the fit as `fitted` and uses its ac, ceiling, centre and scale."""
    subspaces = np.asarray(subspaces, bool)
    raw, acs, lists = [], [], []
    for s in range(subspaces.shape[0]):
        feats = np.flatnonzero(subspaces[s])
        dist, idx = restate_neighbors(Xtr if Xq is None else Xq, Xtr, feats, k, exclude_self=Xq is None)
        lists.append((dist, idx))
        ac = restate_cof_chain(Xtr if Xq is None else Xq, Xtr, feats, idx[:, :k], chain)[0]
        acs.append(ac)
        raw.append(restate_cof_from_lists(ac, ac if fitted is None else fitted["ac"][s], idx[:, :k]))
    raw = np.array(raw)
    per, ceiling, ndeg = restate_ceiling(to_score32(raw), None if fitted is None else fitted["ceiling"])
    if fitted is not None:
        center, scale = fitted["center"], fitted["scale"]
    else:
        center, scale = (None, None) if normalize is None else restate_stats(per, normalize)
    scores = restate_combine(per, proba, center, scale, combination)
    return dict(scores=scores, per=per, raw=raw, ac=np.array(acs), ceiling=ceiling, n_degenerate=ndeg, center=center,
                scale=scale, lists=lists)


def _mask(d, feature_lists):
    m = np.zeros((len(feature_lists), d), bool)
    for s, feats in enumerate(feature_lists):
        m[s, feats] = True
    return m


def _ac(points, chain="sbn"):
    """ac of the first row of `points` with the other rows as its list, in the order given."""
    P = np.atleast_2d(np.asarray(points, np.float32))
    if P.shape[0] == 1:
        P = P.T
    return restate_cof_chain(P[:1], P[1:], np.arange(P.shape[1]), [list(range(P.shape[0] - 1))], chain)[0][0]


# ---- the set-based nearest chain against scipy's minimum spanning tree ---------------------------------------------------
def test_sbn_chain_is_the_minimum_spanning_tree_grown_from_the_query():
    """Another code path: with distinct distances the minimum spanning tree of the k + 1 points is unique, and the set-based
    nearest path is that tree grown from o_0 along the cheapest tree edge that leaves the set (Prim).  200 random point
    sets of 3 .. 33 points and 1 .. 5 features; the edges agree to the bit (both take the square root of the same d2)."""
    from scipy.sparse import csr_matrix
    from scipy.sparse.csgraph import minimum_spanning_tree
    rng = np.random.default_rng(31)
    sizes = set()
    for trial in range(200):
        m, ds = int(rng.integers(3, 34)) if trial >= 2 else (3, 33)[trial], int(rng.integers(1, 6))
        sizes.add(m)
        P = rng.normal(size=(m, ds)).astype(np.float32)
        D2 = restate_pair_sq_dists(P[:1], P[1:], np.arange(ds), [list(range(m - 1))])
        off = D2[0][np.triu_indices(m, 1)]
        assert len(np.unique(off)) == off.size and (off > 0).all()  # distinct distances
        got, gap = chain_edges(D2, "sbn")
        assert gap[0] > 0
        # a sparse graph of the upper triangle: the dense input path of csgraph drops edges below 1e-8
        tree = minimum_spanning_tree(csr_matrix(np.triu(D2[0], 1))).toarray()
        tree = np.maximum(tree, tree.T)
        assert (tree > 0).sum() == 2 * (m - 1)
        inside, want = np.zeros(m, bool), []
        inside[0] = True
        for _ in range(m - 1):
            cand = np.where(inside[:, None] & ~inside[None, :] & (tree > 0), tree, np.inf)
            u, v = np.unravel_index(cand.argmin(), cand.shape)
            want.append(np.sqrt(cand[u, v]))
            inside[v] = True
        np.testing.assert_array_equal(got[0], np.array(want))
    assert {3, 33} <= sizes


# ---- hand-checkable cases -------------------------------------------------------------------------------------------------
def test_hand_checkable_chains():
    """On a line.  Query 0 with neighbours 1, 2, 3: every edge is 1 and the weights sum to 1.  Neighbours 1, 3, 7: edges 1, 2,
    4 under weights 6/12, 4/12, 2/12: 22/12.  Neighbours (1, -1.5, 1.2) in list order: the set-based path takes 1 (edge
    1), then 1.2 (0.2 from 1), then -1.5 (1.5 from 0): (6 + 0.8 + 3) / 12; the rank chain takes them as listed, edges 1,
    1.5 (to 0), 0.2 (to 1): (6 + 6 + 0.4) / 12."""
    for chain in CHAINS:
        assert abs(_ac([0, 1, 2, 3], chain) - 1.0) <= 2e-16  # 6/12 + 4/12 + 2/12 in float64
        assert abs(_ac([0, 1, 3, 7], chain) - 22.0 / 12.0) <= 4e-16
        assert abs(_ac([0, 2.5], chain) - 2.5) == 0.0  # k = 1: ac = d(q, o_1)
        assert abs(_ac([[0, 0], [3, 4]], chain) - 5.0) == 0.0
    sbn, rank = _ac([0, 1, -1.5, 1.2], "sbn"), _ac([0, 1, -1.5, 1.2], "rank")
    assert abs(sbn - 9.8 / 12.0) <= 1e-7 and abs(rank - 12.4 / 12.0) <= 1e-7  # 1.2 is not a float32
    assert abs(sbn - 0.8166666) < 1e-6 and abs(rank - 1.0333333) < 1e-6 and sbn != rank
    # scale free: the chain of c X is c times the chain of X
    assert abs(_ac([0, 2, 6, 14]) - 2 * 22.0 / 12.0) <= 8e-16


def test_a_tie_goes_to_the_lower_list_position():
    """Integer points: d2 is exact.  From (0, 0), (2, 0) and (0, 2) tie at d2 = 4 and (3, 0) is at 9.  Taking (2, 0) first
    brings (3, 0) to 1: edges 2, 1, 2, ac 20/12.  Taking (0, 2) first leaves (2, 0) at 2 and then (3, 0) at 1: edges 2, 2, 1,
    ac 22/12.  Whichever of the two is listed first is taken."""
    a, b, c = [2, 0], [0, 2], [3, 0]
    assert abs(_ac([[0, 0], a, b, c]) - 20.0 / 12.0) <= 4e-16
    assert abs(_ac([[0, 0], b, a, c]) - 22.0 / 12.0) <= 4e-16
    e, gap = chain_edges(restate_pair_sq_dists(np.zeros((1, 2), np.float32), np.array([a, b, c], np.float32), [0, 1], [[0, 1, 2]]), "sbn")
    assert e[0].tolist() == [2.0, 1.0, 2.0] and gap[0] == 0.0  # the tie is reported as a gap of 0
    # duplicates of the query: edges of 0 first, whatever the list order
    assert _ac([[1, 1], [5, 1], [1, 1], [1, 1]]) == (2.0 / 12.0) * 4.0


# ---- zero denominators, the ceiling, the float32 range --------------------------------------------------------------------
def test_zero_denominator_rules():
    """Both zero: exactly 1, not degenerate.  Only the denominator zero: NaN, then the ceiling."""
    ac_ref = np.array([0.0, 0.0, 0.0, 2.0, 4.0])
    idx = np.array([[0, 1, 2], [0, 1, 2], [3, 4, 0], [0, 1, 3]])
    raw = restate_cof_from_lists(np.array([0.0, 0.7, 3.0, 0.0]), ac_ref, idx)
    assert raw[0] == 1.0 and np.isnan(raw[1]) and raw[2] == 3.0 * 3 / 6.0 and raw[3] == 0.0
    per, ceiling, ndeg = restate_ceiling(to_score32(raw[None, :]))
    assert ndeg.tolist() == [1] and ceiling[0] == 1.5 and per[0].tolist() == [1.0, 1.5, 1.5, 0.0]
    # the ceiling of the fit is applied to new rows as stored
    new, ceiling2, ndeg2 = restate_ceiling(np.array([[np.nan, 7.0]], np.float32), ceiling=ceiling)
    assert new[0].tolist() == [1.5, 7.0] and ceiling2[0] == 1.5 and ndeg2.tolist() == [1]
    # a subspace with no non-degenerate row: ceiling 1
    per, ceiling, ndeg = restate_ceiling(np.full((1, 4), np.nan, np.float32))
    assert ceiling[0] == 1.0 and ndeg.tolist() == [4] and (per == 1.0).all()


def test_scores_beyond_the_float32_range_are_stored_as_the_largest_float32():
    got = to_score32([1e39, 3.0, np.nan, FLT_MAX * (1 + 2.0 ** -25), 0.0])
    assert got[0] == np.float32(FLT_MAX) and got[1] == 3.0 and np.isnan(got[2]) and got[3] == np.float32(FLT_MAX)
    assert np.isfinite(got[[0, 1, 3, 4]]).all()


def test_duplicate_groups_through_the_restated_ensemble():
    """k = 3.  Rows 0 .. 3 are one point (each has 3 duplicates: ac 0, denominator 0: exactly 1), row 4 sits next to them
    (its neighbours are three of the four: denominator 0, ac > 0: degenerate), the rest is a cloud.  A subspace on a
    constant feature: every score exactly 1, nothing degenerate."""
    rng = np.random.default_rng(3)
    X = rng.normal(size=(40, 3)).astype(np.float32)
    X[:4, :2] = [10, 10]
    X[4, :2] = [10.5, 10]
    X[:, 2] = 2.5
    res = restate_cof_ensemble(_mask(3, [[0, 1], [2]]), [0.5, 0.5], X, k=3)
    assert (res["ac"][0][:4] == 0).all() and (res["per"][0][:4] == 1).all() and np.isnan(res["raw"][0][4])
    assert res["n_degenerate"].tolist() == [1, 0] and res["ceiling"][0] == res["per"][0].max() == res["per"][0][4]
    assert res["ceiling"][0] == np.nanmax(to_score32(res["raw"][0])) > 1
    assert (res["per"][1] == 1).all() and res["ceiling"][1] == 1.0 and (res["ac"][1] == 0).all()
    assert np.isfinite(res["scores"]).all()


def test_restated_ensemble_on_new_rows_uses_the_state_of_the_fit():
    rng = np.random.default_rng(2)
    X = rng.normal(size=(80, 5)).astype(np.float32)
    X[:, 4] = rng.integers(0, 2, size=80)  # a binary feature: a subspace of point masses at small k
    Y = rng.normal(size=(20, 5)).astype(np.float32)
    Y[:, 4] = rng.integers(0, 2, size=20)
    m, p = _mask(5, [[0, 1], [4], [1, 2, 3]]), [0.2, 0.3, 0.5]
    for chain in CHAINS:
        fit = restate_cof_ensemble(m, p, X, k=6, chain=chain, normalize="robust", combination="max")
        assert fit["n_degenerate"][1] == 0 and (fit["per"][1] == 1).all() and fit["scale"][1] == 1.0
        assert 0.5 < np.median(fit["per"][0]) < 1.5  # inliers sit around 1
        new = restate_cof_ensemble(m, p, X, Y, k=6, chain=chain, combination="max", fitted=fit)
        assert new["center"] is fit["center"] and np.array_equal(new["ceiling"], fit["ceiling"])
        want = ((new["per"].astype(np.float64) - fit["center"][:, None]) / fit["scale"][:, None]).max(axis=0)
        np.testing.assert_array_equal(new["scores"], want)
        # in-sample scoring is not the fit: every row is its own nearest neighbour there and the first edge is 0
        again = restate_cof_ensemble(m, p, X, X, k=6, chain=chain, combination="max", fitted=fit)
        assert not np.array_equal(again["per"][0], fit["per"][0])
    assert not np.array_equal(restate_cof_ensemble(m, p, X, k=6, chain="rank")["ac"][0], restate_cof_ensemble(m, p, X, k=6)["ac"][0])


# ---- the class without a GPU ----------------------------------------------------------------------------------------------
def test_class_is_exported_and_shares_the_pipeline_and_the_tail(cof_class):
    import vgan_amd
    from vgan_amd import outlier
    assert cof_class is outlier.SubspaceCOF and "SubspaceCOF" in vgan_amd.__all__
    assert issubclass(cof_class, outlier._NeighborScorer)
    for name in ["_combine", "predict", "predict_proba", "threshold_", "labels_", "_pack", "decision_function", "_require_fit",
                 "_splits"]:  # the split rule: one copy for every sweep of the module, the kernel methods' too
        assert name in vars(outlier._SubspaceScorer) and name not in vars(cof_class)
    for name in ["_neighbors", "kneighbors", "_chunks"]:  # the neighbour pipeline: one copy
        assert name in vars(outlier._NeighborScorer) and name not in vars(cof_class)
    doc = cof_class.__doc__
    for word in ["pyod", "restatement", "sbn", "rank", "score_ceiling_", "n_degenerate_", "ac_dist_", "decision_function(X_train)"]:
        assert word in doc, word
    with pytest.raises(ValueError, match="method must be 'knn', 'lof' or 'kde', got 'cof'"):
        vgan_amd.SubspaceEnsemble(_mask(4, [[0, 1]]), [1.0], method="cof")


def test_defaults_and_constructor_keywords(cof_class):
    import inspect
    params = inspect.signature(cof_class.__init__).parameters
    assert list(params)[1:] == ["subspaces", "proba", "n_neighbors", "chain", "engine", "splits", "workspace_bytes", "normalize",
                                "combination", "contamination"]
    ens = cof_class(_mask(6, [[0, 1], [2, 3, 5]]), [0.5, 0.5])
    assert ens.n_neighbors == 20 and ens.chain == "sbn" and ens.normalize is None and ens.combination == "sum"
    assert ens.contamination == 0.1 and ens.score_center_ is None and ens.plan.count == 2
    for k in (1, 32, np.int64(7)):
        assert cof_class(_mask(6, [[0, 1]]), [1.0], n_neighbors=k, chain="rank").n_neighbors == int(k)


@pytest.mark.parametrize("kw,match", [
    (dict(n_neighbors=0), "between 1 and 32"), (dict(n_neighbors=33), "between 1 and 32"),
    (dict(n_neighbors=2.5), "between 1 and 32"), (dict(n_neighbors=True), "between 1 and 32"),
    (dict(chain="x"), "chain must be 'sbn' or 'rank', got 'x'"), (dict(chain=0), "chain"), (dict(normalize="l2"), "normalize"),
    (dict(combination="mean"), "combination"), (dict(contamination=0.7), "contamination"), (dict(engine="fast"), "engine"),
    (dict(splits=0), "splits"), (dict(splits=70000), "splits"),
])
def test_constructor_rejects_bad_arguments_without_a_gpu(cof_class, kw, match):
    with pytest.raises(ValueError, match=match):
        cof_class(_mask(6, [[0, 1], [2, 3, 5]]), [0.5, 0.5], **kw)
    with pytest.raises(ValueError, match="proba has 1 entries for 2 subspaces"):
        cof_class(_mask(6, [[0, 1], [2, 3, 5]]), [1.0])


def test_fit_rejects_bad_data_before_the_device_is_touched(cof_class):
    """These raise ValueError with or without a GPU: on the CPU tier a call that reached the device would raise
    VganHipError instead."""
    m = _mask(6, [[0, 1], [2, 3, 5]])
    X = np.random.default_rng(0).normal(size=(20, 6)).astype(np.float32)
    with pytest.raises(ValueError, match=r"n_neighbors \+ 1 reference rows \(21\), got 20"):
        cof_class(m, [0.5, 0.5]).fit(X)
    with pytest.raises(ValueError, match="X has 5 features, the subspaces 6"):
        cof_class(m, [0.5, 0.5], n_neighbors=3).fit(X[:, :5])
    with pytest.raises(ValueError, match="2-d"):
        cof_class(m, [0.5, 0.5], n_neighbors=3).fit(X[0])
    for call in ("decision_function", "predict", "kneighbors"):
        with pytest.raises(RuntimeError, match="SubspaceCOF is not fitted"):
            getattr(cof_class(m, [0.5, 0.5]), call)(X)


def test_outlier_ensemble_routes_cof_to_the_new_class(cof_class):
    import vgan_amd
    model = vgan_amd.VGAN_no_kl(epochs=1)
    model.subspaces = _mask(6, [[0, 1], [2, 3, 5], [4]])
    model.proba = np.array([0.5, 0.3, 0.2])
    ens = model.outlier_ensemble(method="cof", n_neighbors=10)
    assert type(ens) is cof_class and ens.n_neighbors == 10 and ens.chain == "sbn" and ens.plan.count == 3
    np.testing.assert_array_equal(ens.proba, model.proba)
    ens = model.outlier_ensemble(method="cof", n_neighbors=7, chain="rank", normalize="robust", combination="max",
                                 contamination=0.05, engine="exact", splits=3, workspace_bytes=1 << 20)
    assert (ens.n_neighbors, ens.chain, ens.normalize, ens.combination, ens.contamination) == (7, "rank", "robust", "max", 0.05)
    assert (ens.engine, ens.splits, ens.workspace_bytes) == ("exact", 3, 1 << 20)
    with pytest.raises(ValueError, match="between 1 and 32"):
        model.outlier_ensemble(method="cof", n_neighbors=0)
    with pytest.raises(TypeError):
        model.outlier_ensemble(method="cof", knn_method="mean")  # not a keyword of SubspaceCOF
    assert '"cof"' in vgan_amd.VGAN_no_kl.outlier_ensemble.__doc__
    assert type(model.outlier_ensemble(method="abod", n_neighbors=10)) is vgan_amd.SubspaceABOD


# ---- C ABI: argument checks without a GPU -----------------------------------------------------------------------------------
def test_cof_entries_reject_bad_arguments_without_gpu():
    import ctypes
    import vgan_amd
    lib = vgan_amd.lib.load()
    assert vgan_amd.lib.ABI_VERSION == 11 == lib.vgan_abi_version()  # the entries only add symbols
    null = None
    buf = ctypes.create_string_buffer(256)
    p = ctypes.cast(ctypes.addressof(buf) + (-ctypes.addressof(buf)) % 16, ctypes.c_void_p)  # never read

    def rejected(rc):
        msg = lib.vgan_last_error()
        return rc == 1 and b"bad argument" in msg and b"outlier_cof.hip" in msg

    chain = lib.vgan_outlier_cof_chain
    assert rejected(chain(null, 4, 10, p, 4, 10, 4, p, p, 0, 1, p, 5, 0, p, null))  # no query rows
    assert rejected(chain(p, 4, 10, null, 4, 10, 4, p, p, 0, 1, p, 5, 0, p, null))  # no reference rows
    assert rejected(chain(p, 4, 10, p, 4, 10, 4, null, p, 0, 1, p, 5, 0, p, null))  # no feature list
    assert rejected(chain(p, 4, 10, p, 4, 10, 4, p, null, 0, 1, p, 5, 0, p, null))  # no feature offsets
    assert rejected(chain(p, 4, 10, p, 4, 10, 4, p, p, 0, 1, null, 5, 0, p, null))  # no lists
    assert rejected(chain(p, 4, 10, p, 4, 10, 4, p, p, 0, 1, p, 5, 0, null, null))  # no output
    assert rejected(chain(p, 4, 0, p, 4, 10, 4, p, p, 0, 1, p, 5, 0, p, null))  # nq = 0
    assert rejected(chain(p, 3, 10, p, 4, 10, 4, p, p, 0, 1, p, 5, 0, p, null))  # ldq < d
    assert rejected(chain(p, 4, 10, p, 3, 10, 4, p, p, 0, 1, p, 5, 0, p, null))  # ldr < d
    assert rejected(chain(p, 4, 10, p, 4, 10, 4, p, p, 0, 1, p, 0, 0, p, null))  # k = 0
    assert rejected(chain(p, 4, 10, p, 4, 40, 4, p, p, 0, 1, p, 33, 0, p, null))  # k > 32
    assert rejected(chain(p, 4, 10, p, 4, 4, 4, p, p, 0, 1, p, 5, 0, p, null))  # nr < k
    assert rejected(chain(p, 4, 10, p, 4, 10, 4, p, p, 0, 0, p, 5, 0, p, null))  # no subspace
    assert rejected(chain(p, 4, 10, p, 4, 10, 4, p, p, 0, 65536, p, 5, 0, p, null))  # more subspaces than a grid holds
    assert rejected(chain(p, 4, 10, p, 4, 10, 4, p, p, -1, 1, p, 5, 0, p, null))  # first < 0
    assert rejected(chain(p, 4, 10, p, 4, 10, 4, p, p, 0, 1, p, 5, 2, p, null))  # no such chain
    assert rejected(chain(p, 4, 10, p, 4, 10, 4, p, p, 0, 1, p, 5, -1, p, null))
    score = lib.vgan_outlier_cof_score
    assert rejected(score(null, 10, p, 10, p, 5, 1, p, null, 10, null))  # no ac of the query rows
    assert rejected(score(p, 10, null, 10, p, 5, 1, p, null, 10, null))  # no ac of the reference rows
    assert rejected(score(p, 10, p, 10, null, 5, 1, p, null, 10, null))  # no lists
    assert rejected(score(p, 10, p, 10, p, 5, 1, null, null, 10, null))  # no score matrix
    assert rejected(score(p, 10, p, 10, p, 0, 1, p, null, 10, null))  # k = 0
    assert rejected(score(p, 10, p, 40, p, 33, 1, p, null, 10, null))  # k > 32
    assert rejected(score(p, 10, p, 4, p, 5, 1, p, null, 10, null))  # nr < k
    assert rejected(score(p, 10, p, 10, p, 5, 0, p, null, 10, null))  # no subspace
    assert rejected(score(p, 10, p, 10, p, 5, 1, p, null, 9, null))  # ld_score < nq
    ceiling = lib.vgan_outlier_cof_ceiling
    assert rejected(ceiling(null, 10, 2, 10, 1, p, p, null))
    assert rejected(ceiling(p, 10, 2, 10, 1, null, p, null))
    assert rejected(ceiling(p, 10, 2, 10, 1, p, null, null))  # fit without the count
    assert rejected(ceiling(p, 9, 2, 10, 0, p, null, null))  # ld < n
    assert rejected(ceiling(p, 10, 0, 10, 0, p, null, null))
    for name, nargs in (("vgan_outlier_cof_chain", 16), ("vgan_outlier_cof_score", 11), ("vgan_outlier_cof_ceiling", 8)):
        assert len(vgan_amd.lib.SIGNATURES[name][1]) == nargs
    from vgan_amd import outlier
    assert outlier.COF_CHAINS == {"sbn": 0, "rank": 1}  # VGAN_OUTLIER_COF_CHAIN_*
