"""Subspace outlier degree (SOD) over subspaces, CPU tier: the float64 numpy restatement of the contract of
vgan_amd.SubspaceSOD (reference sets from shared nearest neighbours, moments in the order of the set, the summation shape
of the class docstring), pinned to a hand-worked case, to the dense integer product of the incidence matrices, to
numpy.mean / numpy.var and to pyod's scalar loop as it is remembered (there is no pyod here to pin it to; the class
docstring says so); the order rule on hand-made lists; the quality bar on the restatement; and everything of the class and
of the new C-ABI entries that can be checked without a GPU."""
import numpy as np
import pytest

from test_outlier_cpu import restate_neighbors

LANES = 64  # partial sums of V and Q
FORMS = ("pyod", "paper")


@pytest.fixture(autouse=True)
def sod_class():
    """Everything below restates the docstring of this class: without the class there is nothing to restate."""
    import vgan_amd
    return vgan_amd.SubspaceSOD


# ---- the quality recipe of the issue (the GPU tier imports it) -------------------------------------------------------------
def tight_clusters(seed, off=1.5, n=1500, m=15, d=20, C=3, tight=3):
    rng = np.random.default_rng(seed)
    cen = rng.uniform(-4, 4, size=(C, d)); sd = np.ones((C, d))
    tf = [rng.choice(d, tight, replace=False) for _ in range(C)]
    for c in range(C): sd[c, tf[c]] = 0.05
    lab = rng.integers(0, C, n + m)
    X = cen[lab] + sd[lab] * rng.normal(size=(n + m, d))
    y = np.zeros(n + m, int); y[n:] = 1
    for i in range(n, n + m):
        f = rng.choice(tf[lab[i]]); X[i, f] += rng.choice([-1, 1]) * off
    p = rng.permutation(n + m); return X[p].astype(np.float32), y[p]


def roc_auc(scores, y):
    """The Mann-Whitney form, ties counted half."""
    pos, neg = np.asarray(scores)[y == 1], np.asarray(scores)[y == 0]
    return float(((pos[:, None] > neg[None, :]).sum() + 0.5 * (pos[:, None] == neg[None, :]).sum()) / (len(pos) * len(neg)))


# ---- float64 restatement of the contract (SubspaceSOD docstring) -----------------------------------------------------------
def restate_refsets(lists_q, lists_fit, ref_set, exclude_self, self_rows=None):
    """(R int [nq, ref_set], n_unshared): plain loops.  lists_q [nq, k] are the lists of the rows to score, lists_fit [n, k]
    the fit-time lists; exclude_self: row q of lists_q is fitted row q (or self_rows[q], where lists_q is a sample of the
    fitted rows) and is left out of its own set."""
    lists_q, lists_fit = np.asarray(lists_q), np.asarray(lists_fit)
    n = lists_fit.shape[0]
    reverse = [[] for _ in range(n)]
    for j in range(n):
        for m in lists_fit[j]:
            reverse[int(m)].append(j)
    R = np.empty((lists_q.shape[0], ref_set), int)
    n_unshared = 0
    for q in range(lists_q.shape[0]):
        snn = [0] * n
        for m in lists_q[q]:
            for j in reverse[int(m)]:
                snn[j] += 1
        own = -1 if not exclude_self else q if self_rows is None else int(self_rows[q])
        rows = [j for j in range(n) if j != own]
        rows.sort(key=lambda j: (-snn[j], j))
        R[q] = rows[:ref_set]
        n_unshared += snn[rows[ref_set - 1]] == 0
    return R, int(n_unshared)


def incidence(lists, n):
    A = np.zeros((np.asarray(lists).shape[0], n), np.int64)
    np.put_along_axis(A, np.asarray(lists, np.int64), 1, axis=1)
    return A


def restate_refsets_dense(lists_q, lists_fit, ref_set, exclude_self):
    """The same through the dense integer product of the 0/1 incidence matrices (pinned to the loops below): what the GPU
    tier uses on a few hundred rows."""
    n = np.asarray(lists_fit).shape[0]
    # the product in float64 (exact on counts up to 32, and a BLAS call), back to integers
    snn = (incidence(lists_q, n).astype(np.float64) @ incidence(lists_fit, n).T.astype(np.float64)).astype(np.int64)
    key = -snn * n + np.arange(n)[None, :]  # (SNN descending, index ascending) as one integer
    if exclude_self:
        np.fill_diagonal(key, np.iinfo(np.int64).max)
    R = np.argsort(key, axis=1, kind="stable")[:, :ref_set]
    return R, int((np.take_along_axis(snn, R[:, -1:], axis=1) == 0).sum())


def shaped_sum(vals):
    """The summation shape of the docstring along the last axis (positions of F_s): 64 partial sums, partial l sequential over
    the positions l, l + 64, ..., then the partials sequentially in the order l = 0 .. 63.  numpy.cumsum adds sequentially."""
    vals = np.asarray(vals, np.float64)
    pad = (-vals.shape[-1]) % LANES
    v = np.concatenate([vals, np.zeros(vals.shape[:-1] + (pad,))], axis=-1)  # x + 0.0 is x: a lane past d_s adds nothing
    strided = v.reshape(vals.shape[:-1] + (-1, LANES))  # [..., trip, lane]
    partial = np.cumsum(strided, axis=-2)[..., -1, :]
    return np.cumsum(partial, axis=-1)[..., -1]


def restate_sod(Xq, Xr, feats, R, alpha, form):
    """(score float64 [nq], n_relevant int [nq], relevant bool [nq, d_s], mu, v float64 [nq, d_s]) of the reference sets R
    [nq, ref_set] over the features `feats` (ascending).  The sums over the rows of R run sequentially in the order of R
    (a loop over r, vectorised over the rows and features, which keeps every rounding where the scalar loop has it)."""
    feats = np.sort(np.asarray(feats))
    A = np.asarray(Xq, np.float32).astype(np.float64)[:, feats]
    B = np.asarray(Xr, np.float32).astype(np.float64)[:, feats]
    R = np.asarray(R, np.int64)
    ref_set, ds = R.shape[1], len(feats)
    s1 = np.zeros_like(A)
    for r in range(ref_set):
        s1 = s1 + B[R[:, r]]
    mu = s1 / float(ref_set)
    s2 = np.zeros_like(A)
    for r in range(ref_set):
        dlt = B[R[:, r]] - mu
        s2 = s2 + dlt * dlt
    v = s2 / float(ref_set)
    V = shaped_sum(v)
    T = (float(alpha) * V) / float(ds)
    rel = v < T[:, None]
    n_rel = rel.sum(axis=1)
    dq = A - mu
    Q = shaped_sum(np.where(rel, dq * dq, 0.0))
    with np.errstate(divide="ignore", invalid="ignore"):
        score = np.sqrt(Q / n_rel) if form == "pyod" else np.sqrt(Q) / n_rel
    return np.where(n_rel > 0, score, 0.0), n_rel, rel, mu, v


def restate_sod_scalar(Xq, Xr, feats, R, alpha, form):
    """The same with one scalar operation after the other, for the pin of the vectorised form."""
    feats = np.sort(np.asarray(feats))
    out, counts = [], []
    for q in range(len(R)):
        vs, dev2 = [], []
        for f in feats:
            s1 = 0.0
            for r in R[q]:
                s1 = s1 + float(Xr[r, f])
            mu = s1 / float(len(R[q]))
            s2 = 0.0
            for r in R[q]:
                dlt = float(Xr[r, f]) - mu
                s2 = s2 + dlt * dlt
            vs.append(s2 / float(len(R[q])))
            dq = float(Xq[q, f]) - mu
            dev2.append(dq * dq)

        def shaped(vals):
            partial = []
            for lane in range(LANES):
                acc = 0.0
                for x in vals[lane::LANES]:
                    acc = acc + x
                partial.append(acc)
            tot = 0.0
            for p in partial:
                tot = tot + p
            return tot

        T = (float(alpha) * shaped(vs)) / float(len(feats))
        rel = [v < T for v in vs]
        r = sum(rel)
        Q = shaped([x if keep else 0.0 for x, keep in zip(dev2, rel)])
        counts.append(r)
        out.append(0.0 if r == 0 else (np.sqrt(Q / r) if form == "pyod" else np.sqrt(Q) / r))
    return np.array(out), np.array(counts)


def pyod_sod_loop(X, ref_inds, alpha):
    """pyod's SOD._sod as its source is remembered, on given reference sets."""
    ref_set = ref_inds.shape[1]
    anomaly_scores = np.zeros(shape=(X.shape[0],))
    for i in range(X.shape[0]):
        obs = X[i]
        ref = X[ref_inds[i,],]
        means = np.mean(ref, axis=0)
        var_total = np.sum(np.sum(np.square(ref - means))) / ref_set
        var_expect = alpha * var_total / X.shape[1]
        var_actual = np.var(ref, axis=0)
        var_inds = [1 if (j < var_expect) else 0 for j in var_actual]
        rel_dim = np.sum(var_inds)
        if rel_dim != 0:
            anomaly_scores[i] = np.sqrt(np.dot(var_inds, np.square(obs - means)) / rel_dim)
    return anomaly_scores


def restate_sod_fit(X, feats, k, ref_set, alpha, form="pyod"):
    """Fit-time scores of one subspace from the restatement's own float64 neighbours: (score, n_relevant, R, n_unshared)."""
    lists = restate_neighbors(X, X, np.sort(np.asarray(feats)), k, exclude_self=True)[1][:, :k]
    R, n_unshared = restate_refsets_dense(lists, lists, ref_set, True)
    score, n_rel = restate_sod(X, X, feats, R, alpha, form)[:2]
    return score, n_rel, R, n_unshared


def _mask(d, feature_lists):
    m = np.zeros((len(feature_lists), d), bool)
    for s, feats in enumerate(feature_lists):
        m[s, feats] = True
    return m


# ---- the restatement, pinned --------------------------------------------------------------------------------------------------
HAND_LISTS = np.array([[1, 2], [0, 2], [1, 3], [2, 4], [3, 5], [4, 3]])
HAND_X = np.array([[0, 5, 7], [1, 1, 2], [2, 1, 2], [3, 1, 2], [4, 0, 9], [5, 0, 9]], np.float32)


def test_hand_worked_case():
    """Six rows, k = 2, ref_set = 3.  N(0) = {1, 2} shares one row with N(1) = {0, 2}, N(2) = {1, 3} and N(3) = {2, 4} and
    none with N(4), N(5): R(0) = [1, 2, 3], the tie among the three going to the lower index.  Likewise R(2) = [0, 4, 5],
    R(3) = [0, 1, 5], R(5) = [2, 3, 4].  Over R(0) feature 0 is 1, 2, 3 (mean 2, variance 2/3) and features 1 and 2 are
    constant (1 and 2): V = 2/3, T = 0.8 (2/3) / 3 = 0.1778, so features 1 and 2 are relevant and feature 0 is not; row 0
    is (0, 5, 7): Q = 16 + 25 = 41, r = 2: sqrt(41 / 2) in pyod's form, sqrt(41) / 2 in the paper's."""
    for restate in (restate_refsets, restate_refsets_dense):
        R, n_unshared = restate(HAND_LISTS, HAND_LISTS, 3, True)
        assert R[0].tolist() == [1, 2, 3] and R[2].tolist() == [0, 4, 5] and R[3].tolist() == [0, 1, 5] and R[5].tolist() == [2, 3, 4]
        assert n_unshared == 2  # rows 1 and 4 share with two rows only: R(1) = [0, 3, 2], R(4) = [2, 5, 0]
        assert R[1].tolist() == [0, 3, 2] and R[4].tolist() == [2, 5, 0]
        # ref_set = 4: row 3 shares with 0, 1 and 5 only, so its set takes row 2, the lowest index that shares nothing
        R4, n4 = restate(HAND_LISTS, HAND_LISTS, 4, True)
        assert R4[3].tolist() == [0, 1, 5, 2] and R4[0].tolist() == [1, 2, 3, 4] and n4 == 6
    score, n_rel, rel, mu, v = restate_sod(HAND_X, HAND_X, [0, 1, 2], R, 0.8, "pyod")
    assert mu[0].tolist() == [2.0, 1.0, 2.0] and v[0, 1] == 0.0 and v[0, 2] == 0.0 and abs(v[0, 0] - 2.0 / 3.0) < 1e-15
    assert rel[0].tolist() == [False, True, True] and n_rel[0] == 2
    assert abs(score[0] - np.sqrt(20.5)) < 1e-15
    paper = restate_sod(HAND_X, HAND_X, [0, 1, 2], R, 0.8, "paper")[0]
    assert abs(paper[0] - np.sqrt(41.0) / 2.0) < 1e-15
    # alpha = 1 and one feature: v < V / 1 never holds strictly, r = 0, score 0 (pyod's rule)
    one = restate_sod(HAND_X, HAND_X, [0], R, 1.0, "pyod")
    assert (one[1] == 0).all() and (one[0] == 0).all()


def _random_lists(rng, n, nq, k, exclude_self, hub=None):
    """Lists of k distinct rows; with `hub` that row leads every list but its own (a row that sits in n - 1 lists)."""
    out = np.empty((nq, k), int)
    for q in range(nq):
        lead = [hub] if hub is not None and q != hub else []
        pool = np.setdiff1d(np.arange(n), lead + ([q] if exclude_self else []))
        out[q] = lead + list(rng.choice(pool, k - len(lead), replace=False))
    return out


@pytest.mark.parametrize("k,ref_set", [(1, 10), (2, 1), (8, 10), (17, 31), (32, 64)])
def test_shared_neighbours_are_the_dense_integer_product(k, ref_set):
    rng = np.random.default_rng(k)
    n, nq = 90, 37
    fit = _random_lists(rng, n, n, k, True, hub=3)
    new = _random_lists(rng, n, nq, k, False)
    snn = incidence(new, n) @ incidence(fit, n).T
    for q in range(nq):
        for j in range(n):
            assert snn[q, j] == len(set(new[q]) & set(fit[j]))
    for lists, excl in ((fit, True), (new, False)):
        R, nu = restate_refsets(lists, fit, ref_set, excl)
        Rd, nud = restate_refsets_dense(lists, fit, ref_set, excl)
        np.testing.assert_array_equal(R, Rd)
        assert nu == nud
        S = incidence(lists, n) @ incidence(fit, n).T
        for q in range(len(lists)):
            taken = S[q, R[q]]
            assert (np.diff(taken) <= 0).all() and not (excl and q in R[q]) and len(set(R[q])) == ref_set
            rest = np.setdiff1d(np.arange(n), np.append(R[q], q) if excl else R[q])
            assert (S[q, rest] <= taken[-1]).all()  # nothing left out shares more
            assert all(R[q][i] < R[q][i + 1] for i in range(ref_set - 1) if taken[i] == taken[i + 1])
            assert (rest[S[q, rest] == taken[-1]] > R[q][-1]).all()  # a tie at the cut goes to the lower index


def test_order_rule_on_hand_made_lists():
    """k = 1, lists 0 -> 1, 1 -> 0, 2 -> 0, 3 -> 4, 4 -> 3, 5 -> 3.  Rows 1 and 2 share their neighbour 0 with each other
    alone, rows 4 and 5 their neighbour 3; nobody but row 0 lists 1 and nobody but row 3 lists 4, so the sets of rows 0
    and 3 are all tail.  Rows with SNN = 0 fill the tail in ascending index order, and a set that takes one is counted."""
    lists = np.array([[1], [0], [0], [4], [3], [3]])
    R, nu = restate_refsets(lists, lists, 3, True)
    assert R[1].tolist() == [2, 0, 3]   # SNN 1 with row 2, then the tail 0, 3
    assert R[2].tolist() == [1, 0, 3]
    assert R[0].tolist() == [1, 2, 3]   # N(0) = {1}: nobody else lists 1, all tail in index order
    assert R[4].tolist() == [5, 0, 1] and R[5].tolist() == [4, 0, 1]
    assert R[3].tolist() == [0, 1, 2]
    assert nu == 6
    R1, nu1 = restate_refsets(lists, lists, 1, True)
    assert R1[:, 0].tolist() == [1, 2, 1, 0, 5, 4] and nu1 == 2  # rows 0 and 3 alone take a row that shares nothing
    # a tie in SNN goes to the lower index: a new row with the list {0} shares it with rows 1 and 2
    Rn, nun = restate_refsets(np.array([[0]]), lists, 2, False)
    assert Rn[0].tolist() == [1, 2] and nun == 0
    Rn, nun = restate_refsets(np.array([[0]]), lists, 3, False)
    assert Rn[0].tolist() == [1, 2, 0] and nun == 1
    np.testing.assert_array_equal(restate_refsets_dense(lists, lists, 3, True)[0], R)


@pytest.mark.parametrize("ds,ref_set", [(1, 1), (3, 2), (20, 10), (64, 31), (65, 64), (200, 10)])
def test_moments_and_scores_against_numpy_and_the_scalar_loops(ds, ref_set):
    rng = np.random.default_rng(ds + ref_set)
    n, nq, d = 80, 9, 210
    Xr = (rng.normal(size=(n, d)) * rng.uniform(0.01, 3.0, size=d) + 50.0).astype(np.float32)
    Xq = (rng.normal(size=(nq, d)) + 50.0).astype(np.float32)
    feats = np.sort(rng.choice(d, ds, replace=False))
    R = np.array([rng.choice(n, ref_set, replace=False) for _ in range(nq)])
    for alpha in (0.3, 0.8, 1.0):
        for form in FORMS:
            score, n_rel, rel, mu, v = restate_sod(Xq, Xr, feats, R, alpha, form)
            ref = Xr.astype(np.float64)[R][:, :, feats]  # [nq, ref_set, ds]
            assert (np.abs(mu - ref.mean(axis=1)) <= 1e-13 * np.abs(mu)).all()
            assert (np.abs(v - ref.var(axis=1)) <= 1e-13 * v).all()
            if ref_set == 1:
                assert (v == 0).all() and (n_rel == 0).all() and (score == 0).all()  # identical reference rows: r = 0
            scalar, counts = restate_sod_scalar(Xq, Xr, feats, R, alpha, form)
            np.testing.assert_array_equal(score, scalar)
            np.testing.assert_array_equal(n_rel, counts)
            np.testing.assert_array_equal(n_rel, rel.sum(axis=1))
            assert (np.abs(shaped_sum(v) - v.sum(axis=1)) <= 1e-13 * v.sum(axis=1)).all()


@pytest.mark.parametrize("alpha", [0.3, 0.8])
def test_scores_match_pyods_scalar_loop_as_remembered(alpha):
    rng = np.random.default_rng(5)
    X = rng.normal(size=(120, 12)).astype(np.float32)
    X[:, :3] *= 0.05
    lists = restate_neighbors(X, X, np.arange(12), 20, exclude_self=True)[1][:, :20]
    R, _ = restate_refsets(lists, lists, 10, True)
    score = restate_sod(X, X, np.arange(12), R, alpha, "pyod")[0]
    want = pyod_sod_loop(X.astype(np.float64), R, alpha)
    assert (np.abs(score - want) <= 1e-12 * np.abs(want)).all() and (want > 0).any()


# ---- what it detects -------------------------------------------------------------------------------------------------------------
def test_quality_bar_on_the_restatement():
    """Three clusters of 20 features, each tight in three features of its own; 15 rows moved 1.5 along one tight feature of
    their cluster, far inside the marginal range.  SOD with (n_neighbors, ref_set, alpha) = (32, 31, 0.3): mean ROC AUC
    over seeds 0, 1, 2 at least 0.98 and at least 0.2 above sklearn's LOF (k = 20) on the same rows."""
    from sklearn.neighbors import LocalOutlierFactor
    sod, lof = [], []
    for seed in (0, 1, 2):
        X, y = tight_clusters(seed)
        sod.append(roc_auc(restate_sod_fit(X, np.arange(20), 32, 31, 0.3)[0], y))
        lof.append(roc_auc(-LocalOutlierFactor(n_neighbors=20).fit(X).negative_outlier_factor_, y))
    assert np.mean(sod) >= 0.98, sod
    assert np.mean(sod) >= np.mean(lof) + 0.2, (sod, lof)


# ---- the class without a GPU -------------------------------------------------------------------------------------------------
def test_class_is_exported_and_shares_the_tail(sod_class):
    import inspect
    import vgan_amd
    from vgan_amd import outlier
    assert vgan_amd.SubspaceSOD is outlier.SubspaceSOD and "SubspaceSOD" in vgan_amd.__all__
    assert issubclass(sod_class, outlier._NeighborScorer)
    for name in ["_combine", "predict", "predict_proba", "threshold_", "labels_", "decision_function", "kneighbors", "_neighbors"]:
        assert name not in sod_class.__dict__  # shared, not copied
    params = inspect.signature(sod_class.__init__).parameters
    assert list(params)[1:] == ["subspaces", "proba", "n_neighbors", "ref_set", "alpha", "form", "engine", "splits",
                                "workspace_bytes", "normalize", "combination", "contamination"]
    ens = sod_class(_mask(6, [[0, 1], [2, 3, 5]]), [0.5, 0.5])
    assert (ens.n_neighbors, ens.ref_set, ens.alpha, ens.form) == (20, 10, 0.8, "pyod")  # pyod's defaults
    assert ens.normalize is None and ens.combination == "sum" and ens.contamination == 0.1 and ens.plan.count == 2
    assert ens.ops is None  # no constructor touches the device
    assert outlier.SOD_MAX_ROWS >= 1 << 15 and outlier.SOD_MAX_REF == 64 and outlier.SOD_FORMS == {"pyod": 0, "paper": 1}
    assert "SOD_MAX_ROWS" in sod_class.__doc__ and "SubspaceSOD" in outlier.__doc__
    ens = sod_class(_mask(6, [[0, 1]]), [1.0], n_neighbors=np.int64(1), ref_set=np.int64(64), alpha=1, form="paper")
    assert (ens.n_neighbors, ens.ref_set, ens.alpha, ens.form) == (1, 64, 1.0, "paper")  # ref_set is not tied to n_neighbors


@pytest.mark.parametrize("kw,match", [
    (dict(n_neighbors=0), "between 1 and 32"), (dict(n_neighbors=33), "between 1 and 32"),
    (dict(n_neighbors=2.5), "between 1 and 32"), (dict(n_neighbors=True), "between 1 and 32"),
    (dict(ref_set=0), "ref_set must be an integer between 1 and 64"), (dict(ref_set=65), "ref_set"), (dict(ref_set=2.5), "ref_set"),
    (dict(ref_set=True), "ref_set"), (dict(ref_set="10"), "ref_set"),
    (dict(alpha=0.0), r"alpha must be a number in \(0, 1\]"), (dict(alpha=1.5), "alpha"), (dict(alpha=-0.1), "alpha"),
    (dict(alpha=float("nan")), "alpha"), (dict(alpha="0.8"), "alpha"), (dict(alpha=True), "alpha"),
    (dict(form="x"), "form must be 'pyod' or 'paper', got 'x'"), (dict(form=0), "form"),
    (dict(normalize="l2"), "normalize"), (dict(combination="mean"), "combination"), (dict(contamination=0.7), "contamination"),
    (dict(engine="fast"), "engine"), (dict(splits=0), "splits"), (dict(splits=70000), "splits"),
])
def test_constructor_rejects_bad_arguments_without_a_gpu(sod_class, kw, match):
    with pytest.raises(ValueError, match=match):
        sod_class(_mask(6, [[0, 1], [2, 3, 5]]), [0.5, 0.5], **kw)
    with pytest.raises(ValueError, match="proba has 1 entries for 2 subspaces"):
        sod_class(_mask(6, [[0, 1], [2, 3, 5]]), [1.0])


def test_fit_rejects_bad_data_before_the_device_is_touched(sod_class):
    """These raise ValueError with or without a GPU: on the CPU tier a call that reached the device would raise
    VganHipError instead."""
    from vgan_amd import outlier
    m = _mask(6, [[0, 1], [2, 3, 5]])
    X = np.random.default_rng(0).normal(size=(20, 6)).astype(np.float32)
    with pytest.raises(ValueError, match=r"max\(n_neighbors, ref_set\) \+ 1 = 21 fitted rows, got 20"):
        sod_class(m, [0.5, 0.5]).fit(X)
    with pytest.raises(ValueError, match=r"max\(n_neighbors, ref_set\) \+ 1 = 32 fitted rows, got 20"):
        sod_class(m, [0.5, 0.5], n_neighbors=3, ref_set=31).fit(X)
    big = np.broadcast_to(np.zeros((1, 6), np.float32), (outlier.SOD_MAX_ROWS + 1, 6))
    with pytest.raises(ValueError, match=f"SOD_MAX_ROWS = {outlier.SOD_MAX_ROWS} rows, got {outlier.SOD_MAX_ROWS + 1}"):
        sod_class(m, [0.5, 0.5]).fit(big)
    with pytest.raises(ValueError, match="X has 5 features, the subspaces 6"):
        sod_class(m, [0.5, 0.5], n_neighbors=3, ref_set=3).fit(X[:, :5])
    with pytest.raises(ValueError, match="2-d"):
        sod_class(m, [0.5, 0.5], n_neighbors=3, ref_set=3).fit(X[0])
    for call in ("decision_function", "predict", "kneighbors", "reference_set"):
        with pytest.raises(RuntimeError, match="SubspaceSOD is not fitted"):
            getattr(sod_class(m, [0.5, 0.5]), call)(X)
    with pytest.raises(RuntimeError, match="SubspaceSOD is not fitted"):
        sod_class(m, [0.5, 0.5]).relevant_features(0)


def test_outlier_ensemble_routes_sod_to_the_new_class(sod_class):
    import vgan_amd
    model = vgan_amd.VGAN_no_kl(epochs=1)
    model.subspaces = _mask(6, [[0, 1], [2, 3, 5], [4]])
    model.proba = np.array([0.5, 0.3, 0.2])
    ens = model.outlier_ensemble(method="sod", n_neighbors=10)
    assert type(ens) is sod_class and ens.n_neighbors == 10 and ens.ref_set == 10 and ens.plan.count == 3
    np.testing.assert_array_equal(ens.proba, model.proba)
    ens = model.outlier_ensemble(method="sod", n_neighbors=32, ref_set=31, alpha=0.3, form="paper", normalize="robust",
                                 combination="max", contamination=0.05, engine="exact", splits=3, workspace_bytes=1 << 20)
    assert (ens.n_neighbors, ens.ref_set, ens.alpha, ens.form) == (32, 31, 0.3, "paper")
    assert (ens.normalize, ens.combination, ens.contamination) == ("robust", "max", 0.05)
    assert (ens.engine, ens.splits, ens.workspace_bytes) == ("exact", 3, 1 << 20)
    with pytest.raises(ValueError, match="between 1 and 32"):
        model.outlier_ensemble(method="sod", n_neighbors=0)
    with pytest.raises(TypeError):
        model.outlier_ensemble(method="sod", knn_method="mean")  # not a keyword of SubspaceSOD
    assert '"sod"' in vgan_amd.VGAN_no_kl.outlier_ensemble.__doc__
    assert type(model.outlier_ensemble(method="cof", n_neighbors=10)) is vgan_amd.SubspaceCOF


# ---- C ABI: argument checks without a GPU -----------------------------------------------------------------------------------
def test_sod_entries_reject_bad_arguments_without_gpu():
    import ctypes
    import vgan_amd
    lib = vgan_amd.lib.load()
    assert vgan_amd.lib.ABI_VERSION == lib.vgan_abi_version() == 11  # symbols were only added
    null = None
    buf = ctypes.create_string_buffer(256)
    p = ctypes.cast(ctypes.addressof(buf) + (-ctypes.addressof(buf)) % 16, ctypes.c_void_p)  # never read

    def rejected(rc):
        msg = lib.vgan_last_error()
        return rc == 1 and b"bad argument" in msg and b"outlier_sod.hip" in msg

    rev = lib.vgan_sod_reverse_lists
    assert rejected(rev(null, 10, 5, 1, p, p, p, null))  # no lists
    assert rejected(rev(p, 10, 5, 1, null, p, p, null))  # no offsets
    assert rejected(rev(p, 10, 5, 1, p, null, p, null))  # no rows
    assert rejected(rev(p, 10, 5, 1, p, p, null, null))  # no scratch
    assert rejected(rev(p, 10, 0, 1, p, p, p, null))  # k = 0
    assert rejected(rev(p, 40, 33, 1, p, p, p, null))  # k > 32
    assert rejected(rev(p, 5, 5, 1, p, p, p, null))  # n <= k
    assert rejected(rev(p, 32769, 5, 1, p, p, p, null))  # n > VGAN_SOD_MAX_ROWS
    assert rejected(rev(p, 10, 5, 0, p, p, p, null))  # no subspace
    assert rejected(rev(p, 10, 5, 65536, p, p, p, null))
    ref = lib.vgan_sod_reference_sets
    assert rejected(ref(null, 10, p, p, 10, 5, 1, 3, 0, p, null, null))  # no lists
    assert rejected(ref(p, 10, null, p, 10, 5, 1, 3, 0, p, null, null))  # no offsets
    assert rejected(ref(p, 10, p, null, 10, 5, 1, 3, 0, p, null, null))  # no rows
    assert rejected(ref(p, 10, p, p, 10, 5, 1, 3, 0, null, null, null))  # no output
    assert rejected(ref(p, 0, p, p, 10, 5, 1, 3, 0, p, null, null))  # nq = 0
    assert rejected(ref(p, 10, p, p, 10, 0, 1, 3, 0, p, null, null))  # k = 0
    assert rejected(ref(p, 10, p, p, 40, 33, 1, 3, 0, p, null, null))  # k > 32
    assert rejected(ref(p, 10, p, p, 5, 5, 1, 3, 0, p, null, null))  # nr <= k
    assert rejected(ref(p, 10, p, p, 32769, 5, 1, 3, 0, p, null, null))  # nr > VGAN_SOD_MAX_ROWS: the count table
    assert rejected(ref(p, 10, p, p, 10, 5, 1, 0, 0, p, null, null))  # ref_set = 0
    assert rejected(ref(p, 100, p, p, 100, 5, 1, 65, 0, p, null, null))  # ref_set > 64
    assert rejected(ref(p, 10, p, p, 10, 5, 1, 11, 0, p, null, null))  # ref_set > nr
    assert rejected(ref(p, 10, p, p, 10, 5, 1, 10, 1, p, p, null))  # ref_set > nr - 1 with the row itself left out
    assert rejected(ref(p, 9, p, p, 10, 5, 1, 3, 1, p, p, null))  # self excluded, but the queries are not the fitted rows
    assert rejected(ref(p, 10, p, p, 10, 5, 0, 3, 0, p, null, null))  # no subspace
    score = lib.vgan_sod_score

    def call(**kw):
        a = dict(Xq=p, ldq=4, nq=10, Xr=p, ldr=4, nr=10, d=4, feat=p, feat_off=p, first=0, count=1, refset=p, ref_set=3,
                 alpha=0.8, form=0, score=p, score_row=null, ld_score=10, n_relevant=p, mask=null, mask_words=0)
        a.update(kw)
        return score(*a.values(), null)

    for name in ("Xq", "Xr", "feat", "feat_off", "refset", "score", "n_relevant"):
        assert rejected(call(**{name: null})), name
    for kw in (dict(nq=0), dict(nr=0), dict(d=0), dict(ldq=3), dict(ldr=3), dict(first=-1), dict(count=0), dict(count=65536),
               dict(ld_score=9), dict(ref_set=0), dict(ref_set=65), dict(alpha=0.0), dict(alpha=1.5), dict(alpha=float("nan")),
               dict(form=2), dict(form=-1), dict(mask=p, mask_words=0)):
        assert rejected(call(**kw)), kw
    for name, nargs in (("vgan_sod_reverse_lists", 8), ("vgan_sod_reference_sets", 12), ("vgan_sod_score", 22)):
        assert len(vgan_amd.lib.SIGNATURES[name][1]) == nargs
