"""Angle-based outlier scores (FastABOD) over subspaces, CPU tier: the float64 numpy restatement of the contract of
vgan_amd.SubspaceABOD, pinned to exact rational arithmetic (there is no pyod here to pin it to; the class docstring says
so), hand-checkable cases, the floor rule of degenerate rows, the restated ensemble, and everything of the class and of
the new C-ABI entries that can be checked without a GPU."""
from fractions import Fraction

import numpy as np
import pytest

import outlier_checks as oc
from test_outlier_cpu import restate_neighbors
from test_outlier_norm_cpu import restate_combine, restate_stats

FLT_MAX = float(np.finfo(np.float32).max)


# ---- float64 restatement of the contract (SubspaceABOD docstring) -------------------------------------------------------
def restate_abod_from_lists(Xq, Xr, feats, idx):
    """float64 [nq]: -var(w) of every query row from its neighbour list idx [nq, k] (reference row indices), NaN where
    fewer than two neighbours are usable.  Two passes: the mean, then the mean squared deviation."""
    A = np.asarray(Xq, np.float64)[:, feats]
    B = np.asarray(Xr, np.float64)[:, feats]
    idx = np.asarray(idx, np.int64)
    out = np.full(A.shape[0], np.nan)
    for q in range(A.shape[0]):
        V = B[idx[q]] - A[q]
        n2 = (V * V).sum(axis=1)
        V, n2 = V[n2 > 0], n2[n2 > 0]
        m = V.shape[0]
        if m < 2:
            continue
        a, b = np.triu_indices(m, 1)
        w = (V[a] * V[b]).sum(axis=1) / (n2[a] * n2[b])
        mean = w.sum() / w.shape[0]
        out[q] = -(((w - mean) ** 2).sum() / w.shape[0])
    return out


def exact_abod_from_lists(Xq, Xr, feats, idx):
    """The same definition in exact rational arithmetic on the float32 inputs; the result is the exact value rounded once
    to float64 (Fraction.__float__ rounds correctly), NaN where there is no pair.  Every float32 is an integer multiple of
    2^-149, so the vectors are held as integers V = v 2^149; with G = <V_a, V_b> and N_a = |V_a|^2,
    w_ab = G 2^298 / (N_a N_b), brought to the common denominator D = prod_a N_a before the two passes."""
    A = np.asarray(Xq, np.float32)[:, feats]
    B = np.asarray(Xr, np.float32)[:, feats]
    assert np.asarray(Xq).dtype == np.float32 and np.asarray(Xr).dtype == np.float32
    idx = np.asarray(idx, np.int64)

    def ints(row):
        vals = [Fraction(float(x)) * 2 ** 149 for x in row]
        assert all(v.denominator == 1 for v in vals)
        return [v.numerator for v in vals]

    out = np.full(A.shape[0], np.nan)
    for q in range(A.shape[0]):
        qi = ints(A[q])
        V = [[r - c for r, c in zip(ints(B[i]), qi)] for i in idx[q]]
        N = [sum(x * x for x in v) for v in V]
        V = [v for v, n in zip(V, N) if n > 0]
        N = [n for n in N if n > 0]
        m = len(V)
        if m < 2:
            continue
        D = 1
        for n in N:
            D *= n
        P = []  # w_ab = P_ab / D
        for a in range(m):
            for b in range(a + 1, m):
                g = sum(x * y for x, y in zip(V[a], V[b]))
                num = g * 2 ** 298 * D
                assert num % (N[a] * N[b]) == 0
                P.append(num // (N[a] * N[b]))
        c = len(P)
        total = sum(P)  # mean = total / (c D);  w - mean = (c P - total) / (c D)
        dev = sum((c * p - total) ** 2 for p in P)
        out[q] = float(Fraction(-dev, c * c * D * c * D))
    return out


def to_score32(raw):
    """The float32 the score matrix holds for a float64 score: rounded, a value below the float32 range stored as the
    most negative finite float32 (never -inf); NaN stays."""
    raw = np.asarray(raw, np.float64)
    with np.errstate(over="ignore"):
        out = raw.astype(np.float32)
    out[np.isneginf(out)] = -np.float32(FLT_MAX)
    return out


def restate_floor(raw32, floor=None):
    """The floor rule on float32 scores [S, n] with NaN at the degenerate rows: (scores with the floor applied, floor
    float64 [S], n_degenerate int [S]).  floor None: taken from the rows (fit: the smallest non-degenerate score, 0 if
    there is none); otherwise the given floor is applied (decision_function)."""
    raw32 = np.asarray(raw32, np.float32)
    deg = np.isnan(raw32)
    if floor is None:
        floor = np.array([raw32[s][~deg[s]].min() if (~deg[s]).any() else 0.0 for s in range(raw32.shape[0])], np.float64)
    out = np.where(deg, np.asarray(floor, np.float64).astype(np.float32)[:, None], raw32).astype(np.float32)
    return out, np.asarray(floor, np.float64), deg.sum(axis=1)


def restate_abod_ensemble(subspaces, proba, Xtr, Xq=None, k=10, normalize=None, combination="sum", fitted=None):
    """The whole detector from its own float64 neighbours.  fit (Xq None) returns a dict with scores (float64 [n]), per
    (float32 [S, n], floor applied), floor, n_degenerate, center, scale (None without normalize) and lists (per subspace,
    (dist, idx) of restate_neighbors with the extra column); scoring new rows takes the dict of the fit as `fitted` and
    applies its floor, centre and scale."""
    subspaces = np.asarray(subspaces, bool)
    raw, lists = [], []
    for s in range(subspaces.shape[0]):
        feats = np.flatnonzero(subspaces[s])
        dist, idx = restate_neighbors(Xtr if Xq is None else Xq, Xtr, feats, k, exclude_self=Xq is None)
        lists.append((dist, idx))
        raw.append(restate_abod_from_lists(Xtr if Xq is None else Xq, Xtr, feats, idx[:, :k]))
    per, floor, ndeg = restate_floor(to_score32(np.array(raw)), None if fitted is None else fitted["floor"])
    if fitted is not None:
        center, scale = fitted["center"], fitted["scale"]
    else:
        center, scale = (None, None) if normalize is None else restate_stats(per, normalize)
    scores = restate_combine(per, proba, center, scale, combination)
    return dict(scores=scores, per=per, floor=floor, n_degenerate=ndeg, center=center, scale=scale, lists=lists)


def _mask(d, feature_lists):
    m = np.zeros((len(feature_lists), d), bool)
    for s, feats in enumerate(feature_lists):
        m[s, feats] = True
    return m


# ---- the restatement against exact arithmetic -----------------------------------------------------------------------------
@pytest.mark.parametrize("k", [2, 3, 10, 32])
@pytest.mark.parametrize("ds", [3, 48])
@pytest.mark.parametrize("case", oc.ADVERSARIAL)
def test_restatement_is_within_1e12_of_exact_arithmetic(case, ds, k):
    """n = 300, seed 7, the first 40 rows: fit-style lists (self excluded) except for "shifted_query", whose 40 queries
    are scored against the N(0, 1) reference cloud they lie away from."""
    d, n = 64, 300
    feats = np.sort(np.random.default_rng(ds).choice(d, ds, replace=False))
    if case == "shifted_query":
        Xr, Xq = oc.adversarial_pair(case, n, 40, d, seed=7)
        excl = False
    else:
        Xr = oc.adversarial(case, n, d, seed=7)
        Xq, excl = Xr, True
    idx = restate_neighbors(Xq, Xr, feats, k, exclude_self=excl)[1][:40, :k]
    got = restate_abod_from_lists(Xq[:40], Xr, feats, idx)
    want = exact_abod_from_lists(Xq[:40], Xr, feats, idx)
    assert np.isfinite(want).all() and np.isfinite(got).all()
    if k == 2:  # one pair: the variance is exactly 0
        assert (want == 0).all() and (got == 0).all()
        return
    assert (want < 0).all()
    rel = np.abs(got - want) / np.abs(want)
    assert rel.max() <= 1e-12, (case, ds, k, float(rel.max()))


# ---- hand-checkable cases -------------------------------------------------------------------------------------------------
def test_three_neighbours_at_right_angles():
    """q at the origin.  Neighbours (1, 0, 0), (0, 2, 0), (0, 0, 4): every pair at 90 degrees, every w is 0, the score 0.
    Neighbours (1, 0), (0, 2), (-3, 0) at 90, 180 and 90 degrees: w = 0, -3 / (1 x 9) = -1/3, 0; mean -1/9, variance
    ((1/9)^2 + (2/9)^2 + (1/9)^2) / 3 = 2/81."""
    Xr = np.array([[1, 0, 0], [0, 2, 0], [0, 0, 4]], np.float32)
    Xq = np.zeros((1, 3), np.float32)
    got = restate_abod_from_lists(Xq, Xr, np.arange(3), [[0, 1, 2]])
    assert got[0] == 0.0 and exact_abod_from_lists(Xq, Xr, np.arange(3), [[0, 1, 2]])[0] == 0.0
    Xr = np.array([[1, 0], [0, 2], [-3, 0]], np.float32)
    Xq = np.zeros((1, 2), np.float32)
    got = restate_abod_from_lists(Xq, Xr, np.arange(2), [[0, 1, 2]])
    assert abs(got[0] + 2.0 / 81.0) <= 1e-15
    assert exact_abod_from_lists(Xq, Xr, np.arange(2), [[0, 1, 2]])[0] == -2.0 / 81.0
    # the score reads the shape of the neighbourhood, not its radius: scaling by c scales w by 1 / c^2, the score by 1 / c^4
    got2 = restate_abod_from_lists(Xq, 2 * Xr, np.arange(2), [[0, 1, 2]])
    assert abs(got2[0] + 2.0 / 81.0 / 16.0) <= 1e-16


def test_duplicates_are_unusable_and_leave_the_floor():
    """k = 5.  Row 0 with four duplicates among its neighbours (m = 1: degenerate), row 1 with three (m = 2: one pair,
    score 0), row 2 with none (m = 5)."""
    rng = np.random.default_rng(0)
    Xr = rng.normal(size=(12, 3)).astype(np.float32)
    Xq = rng.normal(size=(3, 3)).astype(np.float32)
    Xr[[0, 1, 2, 3]] = Xq[0]
    Xr[[4, 5, 6]] = Xq[1]
    idx = np.array([[0, 1, 2, 3, 8], [4, 5, 6, 9, 10], [7, 8, 9, 10, 11]])
    raw = restate_abod_from_lists(Xq, Xr, np.arange(3), idx)
    assert np.isnan(raw[0]) and raw[1] == 0.0 and raw[2] < 0
    per, floor, ndeg = restate_floor(to_score32(raw[None, :]))
    assert ndeg.tolist() == [1] and floor[0] == float(np.float32(raw[2])) and per[0, 0] == np.float32(raw[2])
    assert per[0].tolist() == [np.float32(raw[2]), 0.0, np.float32(raw[2])]
    # the floor of the fit is applied to new rows as stored
    new, floor2, ndeg2 = restate_floor(np.array([[np.nan, -1.0]], np.float32), floor=floor)
    assert new[0, 0] == np.float32(raw[2]) and new[0, 1] == -1.0 and floor2[0] == floor[0] and ndeg2.tolist() == [1]


def test_a_subspace_of_degenerate_rows_has_floor_zero():
    """Every row equals every other row in the subspace: no usable neighbour anywhere, floor 0, all scores 0."""
    X = np.random.default_rng(1).normal(size=(30, 4)).astype(np.float32)
    X[:, 2] = 1.5
    res = restate_abod_ensemble(_mask(4, [[2], [0, 1, 3]]), [0.5, 0.5], X, k=5)
    assert res["n_degenerate"].tolist() == [30, 0] and res["floor"][0] == 0.0 and (res["per"][0] == 0.0).all()
    assert res["floor"][1] == res["per"][1].min() < 0 and np.isfinite(res["scores"]).all()


def test_scores_below_the_float32_range_are_stored_as_the_most_negative_float32():
    got = to_score32([-1e39, -3.0, np.nan, -FLT_MAX * (1 + 2.0 ** -25), 0.0])
    assert got[0] == -np.float32(FLT_MAX) and got[1] == -3.0 and np.isnan(got[2]) and got[3] == -np.float32(FLT_MAX)
    assert np.isfinite(got[[0, 1, 3, 4]]).all()


def test_restated_ensemble_on_new_rows_uses_the_statistics_of_the_fit():
    rng = np.random.default_rng(2)
    X = rng.normal(size=(80, 5)).astype(np.float32)
    X[:, 4] = rng.integers(0, 2, size=80)  # a binary feature: a subspace of degenerate rows at small k
    Y = rng.normal(size=(20, 5)).astype(np.float32)
    Y[:, 4] = rng.integers(0, 2, size=20)
    m, p = _mask(5, [[0, 1], [4], [1, 2, 3]]), [0.2, 0.3, 0.5]
    fit = restate_abod_ensemble(m, p, X, k=6, normalize="robust", combination="max")
    assert fit["n_degenerate"][1] == 80 and fit["floor"][1] == 0.0 and fit["scale"][1] == 1.0
    new = restate_abod_ensemble(m, p, X, Y, k=6, combination="max", fitted=fit)
    assert new["center"] is fit["center"] and np.array_equal(new["floor"], fit["floor"])
    want = ((new["per"].astype(np.float64) - fit["center"][:, None]) / fit["scale"][:, None]).max(axis=0)
    np.testing.assert_array_equal(new["scores"], want)
    # in-sample scoring is not the fit: every row is its own nearest neighbour and is unusable there
    again = restate_abod_ensemble(m, p, X, X, k=6, combination="max", fitted=fit)
    assert not np.array_equal(again["per"][0], fit["per"][0])


# ---- the class without a GPU ----------------------------------------------------------------------------------------------
def test_class_is_exported_and_shares_the_pipeline_and_the_tail():
    import vgan_amd
    from vgan_amd import outlier
    assert vgan_amd.SubspaceABOD is outlier.SubspaceABOD and "SubspaceABOD" in vgan_amd.__all__
    assert issubclass(vgan_amd.SubspaceABOD, outlier._SubspaceScorer)
    for name in ["_combine", "predict", "predict_proba", "threshold_", "labels_", "_pack"]:  # the tail: on the base only
        assert name in vars(outlier._SubspaceScorer)
        for cls in (vgan_amd.SubspaceABOD, vgan_amd.SubspaceEnsemble, vgan_amd.SubspaceCBLOF):
            assert name not in vars(cls)
    for name in ["_neighbors", "_splits", "kneighbors"]:  # the neighbour pipeline: one copy, shared with SubspaceEnsemble
        owners = [c for c in vgan_amd.SubspaceABOD.__mro__ if name in vars(c)]
        assert len(owners) == 1 and owners[0] not in (vgan_amd.SubspaceABOD, vgan_amd.SubspaceEnsemble)
        assert getattr(vgan_amd.SubspaceABOD, name) is getattr(vgan_amd.SubspaceEnsemble, name)
    for name in ["decision_function", "_require_fit"]:  # one copy for the three detectors, on the base
        assert name in vars(outlier._SubspaceScorer)
        for cls in (vgan_amd.SubspaceABOD, vgan_amd.SubspaceEnsemble, vgan_amd.SubspaceCBLOF, outlier._NeighborScorer):
            assert name not in vars(cls)
    for cls in (vgan_amd.SubspaceABOD, vgan_amd.SubspaceEnsemble, vgan_amd.SubspaceCBLOF):  # one attach rule, no flag of its own
        assert not hasattr(cls, "_attached")
    assert not hasattr(vgan_amd.SubspaceABOD(_mask(4, [[0, 1]]), [1.0]), "_attached")
    assert not hasattr(vgan_amd.SubspaceEnsemble(_mask(4, [[0, 1]]), [1.0]), "_attached")
    assert "pyod" in vgan_amd.SubspaceABOD.__doc__ and "restatement" in vgan_amd.SubspaceABOD.__doc__
    with pytest.raises(ValueError, match="method must be 'knn', 'lof' or 'kde', got 'abod'"):
        vgan_amd.SubspaceEnsemble(_mask(4, [[0, 1]]), [1.0], method="abod")


def test_defaults_and_constructor_keywords():
    import inspect
    import vgan_amd
    params = inspect.signature(vgan_amd.SubspaceABOD.__init__).parameters
    assert list(params)[1:] == ["subspaces", "proba", "n_neighbors", "engine", "splits", "workspace_bytes", "normalize",
                                "combination", "contamination"]
    ens = vgan_amd.SubspaceABOD(_mask(6, [[0, 1], [2, 3, 5]]), [0.5, 0.5])
    assert ens.n_neighbors == 10 and ens.normalize is None and ens.combination == "sum" and ens.contamination == 0.1
    assert ens.score_center_ is None and ens.plan.count == 2
    for k in (2, 32, np.int64(7)):
        assert vgan_amd.SubspaceABOD(_mask(6, [[0, 1]]), [1.0], n_neighbors=k).n_neighbors == int(k)


@pytest.mark.parametrize("kw,match", [
    (dict(n_neighbors=1), "between 2 and 32"), (dict(n_neighbors=33), "between 2 and 32"),
    (dict(n_neighbors=2.5), "between 2 and 32"), (dict(n_neighbors=True), "between 2 and 32"),
    (dict(n_neighbors=0), "n_neighbors"), (dict(normalize="l2"), "normalize"), (dict(combination="mean"), "combination"),
    (dict(contamination=0.7), "contamination"), (dict(contamination=0), "contamination"), (dict(engine="fast"), "engine"),
    (dict(splits=0), "splits"), (dict(splits=70000), "splits"),
])
def test_constructor_rejects_bad_arguments_without_a_gpu(kw, match):
    import vgan_amd
    with pytest.raises(ValueError, match=match):
        vgan_amd.SubspaceABOD(_mask(6, [[0, 1], [2, 3, 5]]), [0.5, 0.5], **kw)
    with pytest.raises(ValueError, match="proba has 1 entries for 2 subspaces"):
        vgan_amd.SubspaceABOD(_mask(6, [[0, 1], [2, 3, 5]]), [1.0])


def test_fit_rejects_bad_data_before_the_device_is_touched():
    """These raise ValueError with or without a GPU: on the CPU tier a call that reached the device would raise
    VganHipError instead."""
    import vgan_amd
    m = _mask(6, [[0, 1], [2, 3, 5]])
    X = np.random.default_rng(0).normal(size=(10, 6)).astype(np.float32)
    with pytest.raises(ValueError, match=r"n_neighbors \+ 1 reference rows \(11\), got 10"):
        vgan_amd.SubspaceABOD(m, [0.5, 0.5]).fit(X)
    with pytest.raises(ValueError, match="X has 5 features, the subspaces 6"):
        vgan_amd.SubspaceABOD(m, [0.5, 0.5], n_neighbors=3).fit(X[:, :5])
    with pytest.raises(ValueError, match="2-d"):
        vgan_amd.SubspaceABOD(m, [0.5, 0.5], n_neighbors=3).fit(X[0])
    for call in ("decision_function", "predict", "kneighbors"):
        with pytest.raises(RuntimeError, match="SubspaceABOD is not fitted"):
            getattr(vgan_amd.SubspaceABOD(m, [0.5, 0.5]), call)(X)
    with pytest.raises(ValueError, match="method must be 'linear' or 'unify'"):
        vgan_amd.SubspaceABOD(m, [0.5, 0.5]).predict_proba(X, method="erf")


def test_outlier_ensemble_routes_abod_to_the_new_class():
    import vgan_amd
    model = vgan_amd.VGAN_no_kl(epochs=1)
    model.subspaces = _mask(6, [[0, 1], [2, 3, 5], [4]])
    model.proba = np.array([0.5, 0.3, 0.2])
    ens = model.outlier_ensemble(method="abod", n_neighbors=10)
    assert type(ens) is vgan_amd.SubspaceABOD and ens.n_neighbors == 10 and ens.plan.count == 3
    np.testing.assert_array_equal(ens.proba, model.proba)
    ens = model.outlier_ensemble(method="abod", n_neighbors=7, normalize="robust", combination="max", contamination=0.05,
                                 engine="exact", splits=3, workspace_bytes=1 << 20)
    assert (ens.n_neighbors, ens.normalize, ens.combination, ens.contamination) == (7, "robust", "max", 0.05)
    assert (ens.engine, ens.splits, ens.workspace_bytes) == ("exact", 3, 1 << 20)
    with pytest.raises(ValueError, match="between 2 and 32"):
        model.outlier_ensemble(method="abod", n_neighbors=1)
    with pytest.raises(TypeError):
        model.outlier_ensemble(method="abod", knn_method="mean")  # not a keyword of SubspaceABOD
    assert "abod" in vgan_amd.VGAN_no_kl.outlier_ensemble.__doc__


# ---- C ABI: argument checks without a GPU -----------------------------------------------------------------------------------
def test_abod_entries_reject_bad_arguments_without_gpu():
    import ctypes
    import vgan_amd
    lib = vgan_amd.lib.load()
    assert vgan_amd.lib.ABI_VERSION == 11 == lib.vgan_abi_version()
    null = None
    buf = ctypes.create_string_buffer(256)
    p = ctypes.cast(ctypes.addressof(buf) + (-ctypes.addressof(buf)) % 16, ctypes.c_void_p)  # never read

    def rejected(rc):
        msg = lib.vgan_last_error()
        return rc == 1 and b"bad argument" in msg and b"outlier_abod.hip" in msg

    abod = lib.vgan_outlier_abod
    assert rejected(abod(null, 4, 10, p, 4, 10, 4, p, p, 0, 1, p, 5, p, null, 10, null))  # no query rows
    assert rejected(abod(p, 4, 10, null, 4, 10, 4, p, p, 0, 1, p, 5, p, null, 10, null))  # no reference rows
    assert rejected(abod(p, 4, 10, p, 4, 10, 4, null, p, 0, 1, p, 5, p, null, 10, null))  # no feature list
    assert rejected(abod(p, 4, 10, p, 4, 10, 4, p, null, 0, 1, p, 5, p, null, 10, null))  # no feature offsets
    assert rejected(abod(p, 4, 10, p, 4, 10, 4, p, p, 0, 1, null, 5, p, null, 10, null))  # no lists
    assert rejected(abod(p, 4, 10, p, 4, 10, 4, p, p, 0, 1, p, 5, null, null, 10, null))  # no score matrix
    assert rejected(abod(p, 3, 10, p, 4, 10, 4, p, p, 0, 1, p, 5, p, null, 10, null))  # ldq < d
    assert rejected(abod(p, 4, 10, p, 3, 10, 4, p, p, 0, 1, p, 5, p, null, 10, null))  # ldr < d
    assert rejected(abod(p, 4, 10, p, 4, 10, 4, p, p, 0, 1, p, 1, p, null, 10, null))  # k = 1: no pair
    assert rejected(abod(p, 4, 10, p, 4, 10, 4, p, p, 0, 1, p, 33, p, null, 10, null))  # k > 32
    assert rejected(abod(p, 4, 10, p, 4, 4, 4, p, p, 0, 1, p, 5, p, null, 10, null))  # nr < k
    assert rejected(abod(p, 4, 10, p, 4, 10, 4, p, p, 0, 0, p, 5, p, null, 10, null))  # no subspace
    assert rejected(abod(p, 4, 10, p, 4, 10, 4, p, p, -1, 1, p, 5, p, null, 10, null))  # first < 0
    assert rejected(abod(p, 4, 10, p, 4, 10, 4, p, p, 0, 1, p, 5, p, null, 9, null))  # ld_score < nq
    floor = lib.vgan_outlier_abod_floor
    assert rejected(floor(null, 10, 2, 10, 1, p, p, null))
    assert rejected(floor(p, 10, 2, 10, 1, null, p, null))
    assert rejected(floor(p, 10, 2, 10, 1, p, null, null))  # fit without the count
    assert rejected(floor(p, 9, 2, 10, 0, p, null, null))  # ld < n
    assert rejected(floor(p, 10, 0, 10, 0, p, null, null))
    for name in ("vgan_outlier_abod", "vgan_outlier_abod_floor"):
        assert name in vgan_amd.lib.SIGNATURES
    assert len(vgan_amd.lib.SIGNATURES["vgan_outlier_abod"][1]) == 17
