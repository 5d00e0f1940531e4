"""CBLOF over subspaces, CPU tier: a float64 numpy restatement of the contract in the docstring of
vgan_amd.SubspaceCBLOF (restate_lloyd, restate_boundary, restate_cblof), checked against sklearn's KMeans and hand-made
size tables, and the argument validation of the class and of the vgan_cluster_* entry points, which needs no GPU.  The GPU
tier (test_outlier_cblof_gpu.py) holds the kernels to these restatements."""
import functools

import numpy as np
import pytest

BLOB_ROWS = (300, 200, 60, 25, 15)
SAFE_SEEDS = [1, 2, 3, 4, 5, 6]
WIDTHS = [(2, 24), (4, 24), (8, 24), (24, 24), (40, 48), (48, 48)]  # (features of the subspace, features of the data)


# ---- data ------------------------------------------------------------------------------------------------------------
def blobs(seed, d=24):
    """(float32 [600, d], blob index of every row): five Gaussian blobs of 300 / 200 / 60 / 25 / 15 rows, rows permuted."""
    rng = np.random.default_rng(seed)
    centres = rng.normal(scale=6, size=(5, d))
    rows = [centres[b] + rng.normal(size=(m, d)) for b, m in enumerate(BLOB_ROWS)]
    blob = np.repeat(np.arange(5), BLOB_ROWS)
    perm = rng.permutation(sum(BLOB_ROWS))
    return np.concatenate(rows)[perm].astype(np.float32), blob[perm]


def subspace_features(ds, d, draw=0):
    """ds sorted random features of d; draw numbers the draws of one width."""
    return np.sort(np.random.default_rng(1000 * ds + draw).choice(d, ds, replace=False))


def first_row_of_each_blob(blob):
    return np.array([int(np.flatnonzero(blob == b)[0]) for b in range(5)])


# ---- the restatement -------------------------------------------------------------------------------------------------
def sq_dists(A, centres):
    """float64 [n, C]: squared distances of the rows A [n, d_s] to the centres [C, d_s], as sums of squared differences."""
    return ((A[:, None, :] - centres[None, :, :]) ** 2).sum(axis=2)


def lloyd_step(A, centres):
    """One E + M step in float64: (labels, new centres, a cluster emptied).  An empty cluster keeps its centre."""
    labels = sq_dists(A, centres).argmin(axis=1)  # first minimum: the smallest centre index among equals
    new = centres.copy()
    emptied = False
    for c in range(centres.shape[0]):
        rows = labels == c
        if rows.any():
            new[c] = A[rows].mean(axis=0)
        else:
            emptied = True
    return labels, new, emptied


def restate_lloyd(X, feats, centres0, max_iter=300, tol=1e-4):
    """The k-means of the contract in float64 on X[:, feats].  Returns a dict: centers, labels (final float64
    assignment), sizes, inertia, n_iter (M steps), converged (an E step changed no label), emptied (some M step met an
    empty cluster), trajectory (the centres before every M step done, then the final ones), shifts (the summed squared
    centre shift of every M step over the tolerance threshold)."""
    A = np.asarray(X, np.float64)[:, feats]
    centres = np.array(centres0, np.float64)
    C = centres.shape[0]
    threshold = tol * A.var(axis=0).mean()
    labels, n_iter, converged, emptied, trajectory, shifts = None, 0, False, False, [centres.copy()], []
    while n_iter < max_iter:
        new_labels, new, e = lloyd_step(A, centres)
        if labels is not None and (new_labels == labels).all():
            converged = True
            break
        labels, emptied = new_labels, emptied or e
        shift = ((new - centres) ** 2).sum()
        shifts.append(shift / threshold if tol > 0 else np.inf)
        centres = new
        n_iter += 1
        trajectory.append(centres.copy())
        if tol > 0 and shift <= threshold:
            break
    D2 = sq_dists(A, centres)
    labels = D2.argmin(axis=1)
    return dict(centers=centres, labels=labels, sizes=np.bincount(labels, minlength=C), n_iter=n_iter, converged=converged,
                inertia=float(D2[np.arange(len(A)), labels].sum()), emptied=emptied, trajectory=trajectory, shifts=shifts)


def restate_boundary(sizes, alpha=0.9, beta=5.0):
    """(t, large bool [C]) of a size table: the rule of the contract, written as the loop it describes."""
    sizes = [int(v) for v in sizes]
    C, n = len(sizes), sum(sizes)
    order = sorted(range(C), key=lambda c: (-sizes[c], c))
    sz = [sizes[c] for c in order]
    both, only_a, only_b = [], [], []
    for i in range(1, C):
        a = sum(sz[:i]) >= alpha * n
        b = sz[i] == 0 or sz[i - 1] / sz[i] >= beta
        if a and b:
            both.append(i)
        if a:
            only_a.append(i)
        if b:
            only_b.append(i)
    t = (both or only_a or only_b or [C])[0]
    large = np.zeros(C, bool)
    large[order[:t]] = True
    return t, large


def restate_cblof(X, feats, centres, alpha=0.9, beta=5.0, use_weights=False, Xq=None):
    """float64 scores of Xq (None: X itself) for clusters fitted on X: (scores, labels of Xq, sizes, large, t)."""
    centres = np.asarray(centres, np.float64)
    A = np.asarray(X, np.float64)[:, feats]
    sizes = np.bincount(sq_dists(A, centres).argmin(axis=1), minlength=centres.shape[0])
    t, large = restate_boundary(sizes, alpha, beta)
    Q = A if Xq is None else np.asarray(Xq, np.float64)[:, feats]
    D2 = sq_dists(Q, centres)
    labels = D2.argmin(axis=1)
    own = D2[np.arange(len(Q)), labels]
    to_large = D2[:, large].min(axis=1)
    score = np.sqrt(np.where(large[labels], own, to_large))
    if use_weights:
        score = score * sizes[labels]
    return score, labels, sizes, large, t


def engine_bound_use(X, feats, trajectory):
    """max over the centre sets of trajectory, the rows and the two engines of 2 tau / margin: margin the gap between a
    row's two smallest true d2, tau the engine's bound on its error in the smallest (the k = 1 sandwich of
    outlier_checks.py; the Gram bound taken over the data rows, whose hull holds every centre).  Below 1 no engine can
    legitimately give a row another label than the restatement."""
    import outlier_checks as oc
    A = np.asarray(X, np.float64)[:, feats]
    use = 0.0
    for centres in trajectory:
        D2 = np.sort(sq_dists(A, centres), axis=1)
        for engine in oc.ENGINES:
            tau = oc.sandwich_tau(engine, X, X, feats, D2[:, :1])[:, 0]
            with np.errstate(divide="ignore"):
                use = max(use, float((2.0 * tau / (D2[:, 1] - D2[:, 0])).max()))
    return use


def is_safe(X, feats, c0):
    """The precondition of the safe inputs, on the restatement alone: strict convergence, no empty cluster, the boundary
    at t = 3 and engine_bound_use <= 0.5 along the whole trajectory."""
    ref = restate_lloyd(X, feats, c0)
    if not ref["converged"] or ref["emptied"] or restate_cblof(X, feats, ref["centers"])[4] != 3:
        return False
    return engine_bound_use(X, feats, ref["trajectory"]) <= 0.5


@functools.lru_cache(maxsize=None)
def safe_case(seed, ds, d):
    """(X, blob, feats, initial centres) of the safe inputs: C = 5, the first row of each blob, and the first random
    draw of ds features on which blobs(seed) is_safe (in two or four random features of 24 two of the five blobs often
    overlap; which draws qualify is decided by the restatement, never by the code under test)."""
    X, blob = blobs(seed, d)
    rows = first_row_of_each_blob(blob)
    for draw in range(200):
        feats = subspace_features(ds, d, draw)
        c0 = X.astype(np.float64)[rows][:, feats]
        if is_safe(X, feats, c0):
            return X, blob, feats, c0
    raise AssertionError(f"no safe draw of {ds} features for blobs({seed}, {d})")


# ---- restate_lloyd against sklearn -------------------------------------------------------------------------------------
@pytest.mark.parametrize("tol", [0.0, 1e-4])
@pytest.mark.parametrize("ds,d", WIDTHS)
@pytest.mark.parametrize("seed", SAFE_SEEDS)
def test_restate_lloyd_is_sklearn_kmeans(seed, ds, d, tol):
    cluster = pytest.importorskip("sklearn.cluster")
    X, blob, feats, c0 = safe_case(seed, ds, d)
    ref = restate_lloyd(X, feats, c0, tol=tol)
    assert not ref["emptied"], "the two empty-cluster rules differ: this case must not empty a cluster"
    km = cluster.KMeans(n_clusters=5, init=c0, n_init=1, algorithm="lloyd", tol=tol, max_iter=300).fit(X.astype(np.float64)[:, feats])
    np.testing.assert_array_equal(ref["labels"], km.labels_)
    np.testing.assert_allclose(ref["centers"], km.cluster_centers_, rtol=0, atol=1e-12)
    np.testing.assert_allclose(ref["inertia"], km.inertia_, rtol=1e-12)


def test_restate_lloyd_random_rows_against_sklearn():
    """C = 8 from random rows splits blobs; sklearn agrees as long as no cluster empties on the way."""
    cluster = pytest.importorskip("sklearn.cluster")
    X, _ = blobs(3)
    feats = subspace_features(8, 24)
    c0 = X.astype(np.float64)[np.random.default_rng(0).choice(len(X), 8, replace=False)][:, feats]
    ref = restate_lloyd(X, feats, c0, tol=0.0)
    assert ref["converged"] and not ref["emptied"]
    km = cluster.KMeans(n_clusters=8, init=c0, n_init=1, algorithm="lloyd", tol=0.0, max_iter=300).fit(X.astype(np.float64)[:, feats])
    np.testing.assert_array_equal(ref["labels"], km.labels_)
    np.testing.assert_allclose(ref["centers"], km.cluster_centers_, rtol=0, atol=1e-12)


def test_restate_lloyd_empty_cluster_keeps_its_centre_and_max_iter():
    X = np.array([[0.0], [1.0], [10.0], [11.0]], np.float32)
    far = np.array([[0.5], [10.5], [1000.0]])
    ref = restate_lloyd(X, [0], far, tol=0.0)
    assert ref["emptied"] and ref["converged"] and ref["n_iter"] == 1
    np.testing.assert_array_equal(ref["centers"], far)
    np.testing.assert_array_equal(ref["sizes"], [2, 2, 0])
    one = restate_lloyd(blobs(1)[0], [0, 1], blobs(1)[0][:8, :2].astype(np.float64), max_iter=1, tol=0.0)
    assert one["n_iter"] == 1 and not one["converged"]


@pytest.mark.parametrize("seed", SAFE_SEEDS)
def test_safe_inputs_are_safe(seed):
    """What the GPU tier's whole-fit test on safe inputs relies on, on the restatement: strict convergence in a few M
    steps, no empty cluster, the boundary at t = 3 (the 25- and 15-row blobs are small), no row within the engines' error
    of a bisector, and the two small blobs scoring above every other row in the wide subspaces."""
    for ds, d in WIDTHS:
        X, blob, feats, c0 = safe_case(seed, ds, d)
        ref = restate_lloyd(X, feats, c0)
        assert ref["converged"] and not ref["emptied"] and 1 <= ref["n_iter"] <= 8, (ds, ref["n_iter"])
        assert engine_bound_use(X, feats, ref["trajectory"]) <= 0.5
        score, labels, sizes, large, t = restate_cblof(X, feats, ref["centers"])
        assert t == 3 and sorted(sizes[large]) == sorted(sizes)[-3:], (ds, sizes, t)
        if ds >= 24:
            small = blob >= 3
            assert score[small].min() > score[~small].max(), (ds, score[small].min(), score[~small].max())


# ---- the boundary ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sizes,alpha,beta,t,large", [
    ([300, 200, 60, 25, 15], 0.9, 5.0, 3, [1, 1, 1, 0, 0]),       # A alone first holds at i = 3 (560 >= 540); no i has both
    ([500, 450, 40, 10], 0.9, 5.0, 2, [1, 1, 0, 0]),              # both at i = 2: 950 >= 900 and 450 / 40 >= 5
    ([100, 100, 100, 100, 5], 0.95, 5.0, 4, [1, 1, 1, 1, 0]),     # both at i = 4
    ([40, 10, 10, 10, 10, 10, 10], 0.9, 3.9, 6, [1, 1, 1, 1, 1, 1, 0]),   # alpha only: A from i = 6, B only at i = 1
    ([60, 10, 10, 10, 10], 0.99, 5.0, 1, [1, 0, 0, 0, 0]),        # beta only: no prefix reaches 99 rows before i = C
    ([25, 25, 25, 25], 0.99, 5.0, 4, [1, 1, 1, 1]),               # neither: pyod raises, here every cluster is large
    ([10, 0, 90, 0], 0.9, 5.0, 1, [0, 0, 1, 0]),                  # zero sizes: 90 >= 90 and 90 / 10 >= 5
    ([50, 50, 0, 0], 0.9, 5.0, 2, [1, 1, 0, 0]),                  # a zero denominator counts as B
    ([30, 30, 30, 5, 5], 0.9, 5.0, 3, [1, 1, 1, 0, 0]),           # ties in size: index ascending inside a tie
    ([5, 30, 5, 30, 30], 0.9, 5.0, 3, [0, 1, 0, 1, 1]),
])
def test_restate_boundary_on_hand_made_tables(sizes, alpha, beta, t, large):
    from vgan_amd.outlier import large_cluster_boundary
    got_t, got_large = restate_boundary(sizes, alpha, beta)
    assert got_t == t and got_large.tolist() == [bool(v) for v in large]
    prod_t, prod_large = large_cluster_boundary(sizes, alpha, beta)
    assert prod_t == t and prod_large.tolist() == got_large.tolist()


def test_product_boundary_equals_restatement_on_random_tables():
    from vgan_amd.outlier import large_cluster_boundary
    rng = np.random.default_rng(0)
    for _ in range(500):
        C = int(rng.integers(2, 12))
        sizes = rng.integers(0, 40, size=C) * rng.integers(0, 2, size=C) + rng.integers(0, 3, size=C)
        if sizes.sum() == 0:
            continue
        alpha, beta = float(rng.uniform(0.51, 0.99)), float(rng.uniform(1.1, 8))
        want, got = restate_boundary(sizes, alpha, beta), large_cluster_boundary(sizes, alpha, beta)
        assert want[0] == got[0] and want[1].tolist() == got[1].tolist(), (sizes, alpha, beta)


# ---- argument validation without a GPU ---------------------------------------------------------------------------------
def _mask(d, feature_lists):
    m = np.zeros((len(feature_lists), d), bool)
    for s, feats in enumerate(feature_lists):
        m[s, feats] = True
    return m


def test_class_is_exported_and_ensemble_keeps_its_methods():
    import vgan_amd
    assert vgan_amd.SubspaceCBLOF is vgan_amd.outlier.SubspaceCBLOF and "SubspaceCBLOF" in vgan_amd.__all__
    assert issubclass(vgan_amd.SubspaceCBLOF, vgan_amd.outlier._SubspaceScorer)
    assert issubclass(vgan_amd.SubspaceEnsemble, vgan_amd.outlier._SubspaceScorer)
    for name in ["_combine", "predict", "predict_proba", "threshold_", "labels_"]:  # shared, not copied
        assert name not in vars(vgan_amd.SubspaceCBLOF) and name not in vars(vgan_amd.SubspaceEnsemble)
    for name in ["decision_function", "_require_fit"]:  # one copy for the three detectors, on the base
        assert name in vars(vgan_amd.outlier._SubspaceScorer)
        for cls in (vgan_amd.SubspaceCBLOF, vgan_amd.SubspaceEnsemble, vgan_amd.SubspaceABOD):
            assert name not in vars(cls)
    ens = vgan_amd.SubspaceCBLOF(_mask(4, [[0, 1]]), [1.0], n_clusters=2)
    assert not hasattr(vgan_amd.SubspaceCBLOF, "_attached") and not hasattr(ens, "_attached")
    with pytest.raises(ValueError, match="method must be 'knn', 'lof' or 'kde', got 'cblof'"):
        vgan_amd.SubspaceEnsemble(_mask(4, [[0, 1]]), [1.0], method="cblof")


@pytest.mark.parametrize("kw,match", [
    (dict(n_clusters=1), "n_clusters"), (dict(n_clusters=65), "n_clusters"), (dict(n_clusters=8.0), "n_clusters"),
    (dict(n_clusters=True), "n_clusters"), (dict(alpha=0.5), "alpha"), (dict(alpha=1.0), "alpha"), (dict(alpha="a"), "alpha"),
    (dict(beta=1.0), "beta"), (dict(beta=float("inf")), "beta"), (dict(max_iter=0), "max_iter"), (dict(max_iter=2.5), "max_iter"),
    (dict(tol=-1e-9), "tol"), (dict(tol=float("nan")), "tol"), (dict(normalize="l2"), "normalize"),
    (dict(combination="mean"), "combination"), (dict(contamination=0.7), "contamination"), (dict(engine="fast"), "engine"),
    (dict(init="k-means++"), "init"), (dict(init=3.5), "init"),
    (dict(init=[0, 1, 2]), r"shape \(4,\) or \(2, 4\)"), (dict(init=[[0, 1, 2, 3]]), r"shape \(4,\) or \(2, 4\)"),
    (dict(init=[0, 1, 1, 2]), "distinct"), (dict(init=[0, 1, -2, 3]), ">= 0"),
    (dict(init=[np.zeros((4, 2))]), "1 centre arrays for 2 subspaces"),
    (dict(init=[np.zeros((4, 2)), np.zeros((4, 2))]), r"subspace 1 must have shape \(4, 3\)"),
    (dict(init=[np.zeros((4, 2)), np.full((4, 3), np.nan)]), "not finite"),
])
def test_constructor_rejects_bad_arguments_without_a_gpu(kw, match):
    import vgan_amd
    args = dict(n_clusters=4)
    args.update(kw)
    with pytest.raises(ValueError, match=match):
        vgan_amd.SubspaceCBLOF(_mask(6, [[0, 1], [2, 3, 5]]), [0.5, 0.5], **args)
    with pytest.raises(ValueError, match="proba has 1 entries for 2 subspaces"):
        vgan_amd.SubspaceCBLOF(_mask(6, [[0, 1], [2, 3, 5]]), [1.0])


def test_fit_rejects_bad_data_before_the_device_is_touched():
    """These raise ValueError with or without a GPU: on the CPU tier a call that reached the device would raise
    VganHipError instead."""
    import vgan_amd
    m = _mask(6, [[0, 1], [2, 3, 5]])
    X = np.random.default_rng(0).normal(size=(10, 6)).astype(np.float32)
    with pytest.raises(ValueError, match=r"at least n_clusters rows \(4\), got 3"):
        vgan_amd.SubspaceCBLOF(m, [0.5, 0.5], n_clusters=4).fit(X[:3])
    with pytest.raises(ValueError, match=r"at least n_clusters rows \(4\), got 3"):
        vgan_amd.SubspaceCBLOF(m, [0.5, 0.5], n_clusters=4, init=[np.zeros((4, 2)), np.zeros((4, 3))]).fit(X[:3])
    with pytest.raises(ValueError, match="row index 10 is out of range for 10 rows"):
        vgan_amd.SubspaceCBLOF(m, [0.5, 0.5], n_clusters=4, init=[0, 1, 2, 10]).fit(X)
    with pytest.raises(ValueError, match="X has 5 features, the subspaces 6"):
        vgan_amd.SubspaceCBLOF(m, [0.5, 0.5], n_clusters=4).fit(X[:, :5])
    with pytest.raises(ValueError, match="2-d"):
        vgan_amd.SubspaceCBLOF(m, [0.5, 0.5], n_clusters=4).fit(X[0])
    with pytest.raises(RuntimeError, match="SubspaceCBLOF is not fitted"):
        vgan_amd.SubspaceCBLOF(m, [0.5, 0.5], n_clusters=4).decision_function(X)


def test_random_init_draws_the_documented_rows():
    from vgan_amd.outlier import resolve_kmeans_rows
    idx = resolve_kmeans_rows("random", 600, 8, 3, seed=7)
    want = np.random.default_rng(7).choice(600, size=8, replace=False)
    assert idx.shape == (3, 8) and (idx == want).all() and len(set(want.tolist())) == 8


def test_entry_points_validate_before_any_device_call():
    import vgan_amd
    lib = vgan_amd.lib.load()
    null = None
    assert lib.vgan_cluster_lloyd_ws_bytes(0, 8, 1, 1) == -1
    assert b"bad argument" in lib.vgan_last_error()
    assert lib.vgan_cluster_lloyd_ws_bytes(100, 65, 1, 1) == -1
    assert lib.vgan_cluster_lloyd_ws_bytes(100, 8, 2, 1) == -1
    assert lib.vgan_cluster_lloyd_ws_bytes(2500, 8, 2, 7) == 3 * 8 * (7 + 2) * 8  # slices x C x (sum d_s + count) doubles
    assert lib.vgan_cluster_image(null, 8, null, null, null, 0, 1, null, null, null, null) != 0
    assert b"cluster.hip" in lib.vgan_last_error() and b"bad argument" in lib.vgan_last_error()
    assert lib.vgan_cluster_lloyd(null, null, null, 0, 0, 0, null, null, null, 0, 0, 0, 0, 8, 0, null, null, null, null, null, null,
                                  null, null, null, null, 0, 1, null) != 0
    assert b"cluster.hip" in lib.vgan_last_error()
    assert lib.vgan_cluster_final(null, 0, 0, 0, null, null, 0, 8, null, null, null, 0, null, null, null, null, null, 0, null) != 0
    assert b"cluster.hip" in lib.vgan_last_error()
