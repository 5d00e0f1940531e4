"""HiCS contrast and search, CPU tier: the numpy restatement (tests/hics_ref.py) pinned to scipy's ks_2samp, numpy's stable
argsort, brute-force constructions and hand-worked cases; the host functions of vgan_amd.hics against it; the bars the
restated search reaches on the two data recipes; the lifted method dispatch; the C ABI's argument checks."""
import ctypes
import itertools
import math

import numpy as np
import pytest

import hics_ref as R


# ---- the restatement against independent references -------------------------------------------------------------------
@pytest.mark.parametrize("n,w,start", [(2, 1, 0), (2, 1, 1), (2, 2, 0), (3, 1, 2), (17, 1, 9), (17, 5, 0), (17, 5, 12), (17, 17, 0),
                                       (64, 20, 44), (100, 1, 0), (100, 37, 11), (100, 100, 0), (257, 26, 231), (1000, 317, 400)])
def test_deviation_is_the_two_sample_ks_statistic(n, w, start):
    from scipy.stats import ks_2samp
    X = np.random.default_rng(n * 1000 + w).standard_normal((n, 2)).astype(np.float32)
    assert len(np.unique(X[:, 0])) == n and len(np.unique(X[:, 1])) == n  # tie free
    order, _ = R.order_rank(X)
    member = R.conditional_rows(order, (0, 1), w, 1, [start, 0])
    assert member.sum() == w and set(np.flatnonzero(member)) == set(order[0, start:start + w])
    D, m = R.deviation_integers(member, order[1])
    want = ks_2samp(X[member, 1], X[:, 1]).statistic
    assert abs(D / (n * m) - want) <= 1e-15
    if w == n:
        assert D == 0 and m == n


def test_order_and_rank_are_the_stable_argsort():
    rng = np.random.default_rng(3)
    X = rng.integers(-2, 3, size=(300, 6)).astype(np.float32)  # many ties
    X[::7, 1] = -0.0
    X[1::7, 1] = 0.0
    X[:, 2] = 1.5  # constant
    X[:, 3] = rng.standard_normal(300)
    X[150:, :] = X[:150, :]  # duplicated rows
    order, rank = R.order_rank(X)
    want = np.argsort(X + np.float32(0.0), axis=0, kind="stable").T
    assert np.array_equal(order, want)
    for f in range(X.shape[1]):
        assert np.array_equal(rank[f, order[f]], np.arange(300))
    assert np.array_equal(order[2], np.arange(300))


def test_intersection_of_three_slices():
    X = R.dep_data(1, n=50, d=5)
    order, rank = R.order_rank(X)
    member = R.conditional_rows(order, (0, 1, 3), 20, 1, [5, 99, 30])
    want = set(order[0, 5:25]) & set(order[3, 30:50])
    assert set(np.flatnonzero(member)) == want
    D, m = R.deviation_integers(member, order[1])
    brute = max(abs(sum(1 for i in want if rank[1, i] < r) * 50 - r * len(want)) for r in range(1, 51))
    assert (D, m) == (brute, len(want))


# ---- host functions of the library --------------------------------------------------------------------------------------
def test_slice_width():
    from vgan_amd.hics import hics_slice_width
    assert hics_slice_width(1000, 2, 0.1) == 100
    assert hics_slice_width(1000, 3, 0.1) == math.ceil(1000 * 0.1 ** 0.5) == 317
    assert hics_slice_width(2000, 390, 0.1) == math.ceil(2000 * 0.1 ** (1 / 389)) == 1989
    assert hics_slice_width(10, 2, 0.01) == 1  # the floor of one row
    assert hics_slice_width(2, 2, 0.1) == 1 and hics_slice_width(2, 2, 0.5) == 1 and hics_slice_width(2, 3, 0.5) == 2
    assert hics_slice_width(50, 10 ** 6, 0.1) == 50  # k large enough that w = n
    assert hics_slice_width(65, 9, 0.1) == 49
    assert hics_slice_width(100, 1, 0.1) == 0 and hics_slice_width(100, 0, 0.1) == 0
    for n, k, a in itertools.product((2, 3, 65, 1000, 4097), (2, 3, 4, 5, 9, 40), (0.1, 0.5)):
        assert hics_slice_width(n, k, a) == R.slice_width(n, k, a)


def _brute_join(sets):
    k = len(sets[0])
    out = set()
    for a, b in itertools.combinations(sets, 2):
        u = tuple(sorted(set(a) | set(b)))
        if len(u) == k + 1 and sorted(a)[:k - 1] == sorted(b)[:k - 1]:
            out.add(u)
    return sorted(out)


def test_join_is_the_brute_force_construction():
    from vgan_amd.hics import hics_join
    assert hics_join([(0, 1), (0, 2), (1, 2), (3, 4)]) == [(0, 1, 2)]
    assert hics_join([(0, 1, 2), (0, 1, 3), (0, 1, 5), (0, 2, 3)]) == [(0, 1, 2, 3), (0, 1, 2, 5), (0, 1, 3, 5)]
    assert hics_join([(0, 1)]) == [] and hics_join([]) == []
    rng = np.random.default_rng(0)
    for k in (2, 3, 4):
        sets = sorted({tuple(sorted(rng.choice(9, size=k, replace=False).tolist())) for _ in range(40)})
        assert hics_join(sets) == _brute_join(sets) == R.join(sets)
        assert hics_join(sets[::-1] + sets) == _brute_join(sets)  # order and duplicates do not matter


def test_select_and_prune_hand_worked():
    from vgan_amd.hics import hics_prune, hics_select
    sets = [(0, 1), (0, 2), (1, 2), (0, 3)]
    con = [0.5, 0.7, 0.5, 0.1]
    assert hics_select(sets, con, 3).tolist() == [1, 0, 2]  # equal contrasts: features ascending
    assert hics_select(np.asarray(sets), con, 3).tolist() == [1, 0, 2]
    assert hics_select(sets, con, 10).tolist() == [1, 0, 2, 3]
    mixed = [(0, 1, 2), (0, 1), (2, 3), (1, 2)]
    assert hics_select(mixed, [0.4, 0.4, 0.4, 0.9], 4).tolist() == [3, 1, 2, 0]  # equal contrasts: the smaller set first
    #            S          T containing S with one more feature
    pool = [(0, 1), (0, 2), (1, 2), (0, 1, 2), (0, 3), (0, 1, 3), (0, 1, 2, 3)]
    con = [0.5, 0.3, 0.6, 0.55, 0.2, 0.2, 0.9]
    # (0,1): (0,1,2) 0.55 > 0.5 drops it; (0,2): dropped; (1,2): 0.55 < 0.6 stays; (0,1,2): (0,1,2,3) 0.9 drops it;
    # (0,3): (0,1,3) has an EQUAL contrast, stays; (0,1,3): dropped by (0,1,2,3); (0,1,2,3) stays.  (0,1,2,3) does not
    # touch the pairs: it has two more features
    assert hics_prune(pool, con).tolist() == [False, False, True, False, True, False, True]
    assert hics_prune(pool, con).tolist() == R.prune(pool, con)
    rng = np.random.default_rng(5)
    pool = sorted({tuple(sorted(rng.choice(7, size=int(k), replace=False).tolist())) for k in rng.integers(2, 5, size=60)})
    con = rng.integers(0, 4, size=len(pool)) / 4.0  # many equal contrasts
    assert hics_prune(pool, con).tolist() == R.prune(pool, con)
    assert hics_select(pool, con, 17).tolist() == R.select(pool, con, 17)


@pytest.mark.parametrize("n,k,alpha", [(2, 2, 0.1), (65, 2, 0.1), (65, 9, 0.1), (1000, 3, 0.5), (1000, 4, 0.1), (1000, 5, 0.1), (4097, 40, 0.1)])
def test_draws_equal_the_restatement(n, k, alpha):
    from vgan_amd.hics import hics_draws, hics_slice_width
    w = hics_slice_width(n, k, alpha)
    for seed, sid in ((0, 0), (7, (3 << 32) | 5), (2 ** 63 + 11, 2 ** 64 - 1)):
        c, start = hics_draws(n, k, w, 20, seed, sid)
        assert c.shape == (20,) and start.shape == (20, k)
        assert c.min() >= 0 and c.max() < k and start.min() >= 0 and start.max() <= n - w
        for t in range(20):
            cr, sr = R.draw(n, k, w, t, seed, sid)
            assert c[t] == cr and start[t].tolist() == sr
    if k == 5:  # 200 draws miss one of 5 positions with probability 5 * 0.8^200
        c, start = hics_draws(n, k, w, 200, 1, 2)
        assert len(np.unique(c)) == k and len(np.unique(start[:, 4])) > 1  # the second Philox block is in use


def test_random_subspaces():
    from vgan_amd.hics import random_subspaces
    S, p = random_subspaces(20, 50, seed=3)
    assert S.shape == (50, 20) and S.dtype == bool and np.allclose(p, 1 / 50)
    sizes = S.sum(axis=1)
    assert sizes.min() >= 10 and sizes.max() <= 19 and len(np.unique(sizes)) > 3
    assert np.array_equal(S, random_subspaces(20, 50, seed=3)[0]) and not np.array_equal(S, random_subspaces(20, 50, seed=4)[0])
    S, _ = random_subspaces(20, 30, seed=0, min_features=2, max_features=3)
    assert set(S.sum(axis=1)) == {2, 3}
    assert random_subspaces(1, 2)[0].all()
    with pytest.raises(ValueError):
        random_subspaces(5, 3, min_features=4, max_features=3)
    with pytest.raises(ValueError):
        random_subspaces(5, 0)


def test_arguments_are_checked_without_a_device():
    from vgan_amd import HiCS, subspace_contrast
    from vgan_amd.hics import HICS_MAX_ROWS
    assert HICS_MAX_ROWS == 2 ** 18
    for kw in ({"alpha": 0.0}, {"alpha": 1.0}, {"n_iterations": 0}, {"candidate_cutoff": 0}, {"n_subspaces": 0}, {"max_dim": 1},
               {"seed": -1}, {"weights": "rank"}):
        with pytest.raises(ValueError):
            HiCS(**kw)
    two = np.ones((1, 3), dtype=bool)
    with pytest.raises(ValueError, match="HICS_MAX_ROWS"):
        subspace_contrast(np.zeros((HICS_MAX_ROWS + 1, 3), dtype=np.float32), two)
    with pytest.raises(ValueError, match="HICS_MAX_ROWS"):
        subspace_contrast(np.zeros((1, 3), dtype=np.float32), two)
    with pytest.raises(ValueError, match="HICS_MAX_ROWS"):
        HiCS().fit(np.zeros((1, 3), dtype=np.float32))
    with pytest.raises(ValueError):
        subspace_contrast(np.zeros((5, 4), dtype=np.float32), two)  # d differs
    with pytest.raises(ValueError):
        subspace_contrast(np.zeros((5, 3), dtype=np.float32), two, stream_ids=[1, 2])
    with pytest.raises(ValueError):
        HiCS().fit(np.zeros((5, 1), dtype=np.float32))
    with pytest.raises(RuntimeError):
        HiCS().outlier_ensemble()


# ---- what the restated search finds ----------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", range(5))
def test_search_separates_the_planted_dependences(seed):
    res = R.search(R.dep_data(seed), max_dim=4)
    pairs = dict(zip(res["levels"][0]["candidates"], res["levels"][0]["contrast"]))
    triples = dict(zip(res["levels"][1]["candidates"], res["levels"][1]["contrast"]))
    assert len(pairs) == 28 and res["levels"][0]["candidates"] == sorted(pairs)
    assert pairs[(0, 1)] > 0.45
    assert max(v for s, v in pairs.items() if s != (0, 1)) < 0.25
    assert triples[(2, 3, 4)] > 0.22
    assert max(v for s, v in triples.items() if s != (2, 3, 4) and not {0, 1} <= set(s)) < 0.20
    assert res["sets"][0] == (0, 1) and abs(res["proba"].sum() - 1.0) < 1e-12
    assert all(np.diff(res["contrast"]) <= 0)


@pytest.mark.parametrize("seed", range(3))
def test_search_finds_the_hidden_outliers(seed):
    from sklearn.metrics import roc_auc_score
    from sklearn.neighbors import LocalOutlierFactor
    X, y = R.hidden_outlier_data(seed)
    assert all(X[y == 1, f].max() < X[y == 0, f].max() and X[y == 1, f].min() > X[y == 0, f].min() for f in (0, 1))
    res = R.search(X)
    weights = res["contrast"][:10] / res["contrast"][:10].sum()
    score = np.zeros(len(X))
    for z in range(10):
        score += weights[z] * -LocalOutlierFactor(n_neighbors=20).fit(X[:, res["subspaces"][z]]).negative_outlier_factor_
    full = -LocalOutlierFactor(n_neighbors=20).fit(X).negative_outlier_factor_
    assert roc_auc_score(y, score) >= 0.99
    assert roc_auc_score(y, full) < 0.75


# ---- the lifted dispatch ----------------------------------------------------------------------------------------------
DISPATCH = {"knn": "SubspaceEnsemble", "lof": "SubspaceEnsemble", "kde": "SubspaceEnsemble", "cblof": "SubspaceCBLOF",
            "abod": "SubspaceABOD", "cof": "SubspaceCOF", "ecod": "SubspaceECOD", "iforest": "SubspaceIForest", "inne": "SubspaceINNE",
            "mahalanobis": "SubspaceMahalanobis", "mcd": "SubspaceMahalanobis", "gmm": "SubspaceGMM", "hbos": "SubspaceHBOS",
            "loda": "SubspaceLODA", "pca": "SubspacePCA", "ocsvm": "SubspaceOCSVM", "sos": "SubspaceSOS", "dif": "SubspaceDIF",
            "kpca": "SubspaceKPCA", "autoencoder": "SubspaceAutoEncoder", "deepsvdd": "SubspaceDeepSVDD", "sod": "SubspaceSOD"}


def test_dispatch_returns_the_same_classes_from_the_models_and_from_hics():
    import vgan_amd
    subspaces = np.array([[1, 1, 0, 0], [0, 1, 1, 1], [1, 0, 1, 0]], dtype=bool)
    proba = np.array([0.5, 0.25, 0.25])
    model = vgan_amd.VGAN_no_kl.__new__(vgan_amd.VGAN_no_kl)  # no constructor: the dispatch reads two attributes
    model.subspaces, model.proba = subspaces, proba
    found = vgan_amd.HiCS()
    found.subspaces, found.proba = subspaces, proba
    for method, name in DISPATCH.items():
        kw = {"n_neighbors": 3} if method in ("abod", "cof", "sod", "knn", "lof") else {}
        direct = vgan_amd.build_ensemble(subspaces, proba, method=method, **kw)
        for ens in (direct, model.outlier_ensemble(method=method, **kw), found.outlier_ensemble(method=method, **kw)):
            assert type(ens) is getattr(vgan_amd, name)
            assert ens.ops is None  # no constructor touches the device
            assert np.array_equal(ens.proba, proba)
            assert getattr(ens, "robust", False) == (method == "mcd")
            if "n_neighbors" in kw:
                assert ens.n_neighbors == 3
            if name == "SubspaceEnsemble":
                assert ens.method == method
    assert vgan_amd.build_ensemble(subspaces, proba, method="ecod", aggregate="tail").aggregate == "tail"
    with pytest.raises(ValueError):
        vgan_amd.build_ensemble(subspaces, proba, method="no such method")
    assert callable(vgan_amd.VGAN.subspace_contrast) and callable(vgan_amd.VGAN_no_kl.subspace_contrast)


# ---- the C ABI ---------------------------------------------------------------------------------------------------------
def test_entry_points_reject_bad_arguments_without_a_gpu():
    import vgan_amd
    from vgan_amd.hics import HICS_MAX_ROWS
    lib = vgan_amd.lib.load()
    null, p = None, ctypes.c_void_p(64)  # never dereferenced: every call below is rejected first

    def rejected(rc):
        return rc == 1 and b"bad argument" in lib.vgan_last_error() and b"outlier_hics.hip" in lib.vgan_last_error()

    sort = lib.vgan_hics_argsort_columns
    good = [p, 4, 10, 4, p, 16, p, p, null]
    for pos in (0, 4, 6, 7):
        assert rejected(sort(*[null if i == pos else v for i, v in enumerate(good)]))  # a missing pointer
    for pos, bad in ((1, 3), (2, 1), (2, HICS_MAX_ROWS + 1), (3, 0), (5, 8), (5, 12), (5, 32)):  # ldx < d, rows, d, n_pad
        assert rejected(sort(*[bad if i == pos else v for i, v in enumerate(good)]))
    con = lib.vgan_hics_contrast
    good = [p, p, 10, 4, p, p, p, p, 3, 5, 0, 0, p, p, p, p, p, null]
    for pos in (0, 1, 4, 5, 6, 7, 12, 13, 14, 15, 16):
        assert rejected(con(*[null if i == pos else v for i, v in enumerate(good)]))
    for pos, bad in ((2, 1), (2, HICS_MAX_ROWS + 1), (3, 0), (8, 0), (9, 0), (11, 2), (11, -1)):  # n, d, S, M, group
        assert rejected(con(*[bad if i == pos else v for i, v in enumerate(good)]))
    assert rejected(con(*[(65537 if i == 2 else 4 if i == 11 else v) for i, v in enumerate(good)]))  # a wave's maps past 64 KB
    assert rejected(con(*[(2 ** 30 if i == 8 else 50 if i == 9 else 1 if i == 11 else v) for i, v in enumerate(good)]))  # grid
    for name, nargs in (("vgan_hics_argsort_columns", 9), ("vgan_hics_contrast", 18)):
        assert len(vgan_amd.lib.SIGNATURES[name][1]) == nargs
    assert vgan_amd.lib.ABI_VERSION == lib.vgan_abi_version()
