"""HiCS contrast and search on the MI355X (csrc/outlier_hics.hip through vgan_amd.hics) against the numpy restatement of
tests/hics_ref.py, which tests/test_outlier_hics_cpu.py pins.  Everything up to the one division per draw is an integer
and the float64 sum has one order, so every comparison here is exact: order, rank, D, m and c as integers, contrasts bit
for bit."""
import numpy as np
import pytest

import hics_ref as R

pytestmark = pytest.mark.gpu


def _mask(d, lists):
    out = np.zeros((len(lists), d), dtype=bool)
    for z, feats in enumerate(lists):
        out[z, list(feats)] = True
    return out


def _bits(a):
    return np.asarray(a, dtype=np.float64).view(np.int64)


def _tied_data(n, d, seed):
    """float32 [n, d]: column 0 constant, column 1 of few values with both zeros, rows of the second half duplicating the
    first; the rest standard normal."""
    rng = np.random.default_rng(seed)
    X = rng.standard_normal((n, d)).astype(np.float32)
    X[:, 0] = 2.5
    if d > 1:
        X[:, 1] = rng.integers(-1, 2, size=n).astype(np.float32)
        X[::3, 1] *= np.float32(-0.0)  # -0.0 and +0.0 among the zeros
    X[n // 2:2 * (n // 2)] = X[:n // 2]
    return X


def _argsort_on_device(X):
    import torch
    from vgan_amd.hics import ContrastIndex
    index = ContrastIndex(torch.as_tensor(X))
    return index.order.cpu().numpy().astype(np.int64), index.rank.cpu().numpy().astype(np.int64)


def _restate(X, lists, alpha, M, seed, ids):
    order, _ = R.order_rank(X)
    res = [R.contrast(order, tuple(f), alpha, M, seed, int(i)) for f, i in zip(lists, ids)]
    return (np.asarray([r[0] for r in res]), np.stack([r[1] for r in res]), np.stack([r[2] for r in res]),
            np.stack([r[3] for r in res]), np.asarray([r[4] for r in res]))


def _check(X, lists, alpha, M, seed=0, ids=None, **kw):
    from vgan_amd import subspace_contrast
    default_ids = kw.pop("default_ids", False)  # leave stream_ids out: the row position is the id
    ids = np.arange(len(lists)) if ids is None else ids
    want = _restate(X, lists, alpha, M, seed, ids)
    got = subspace_contrast(X, _mask(X.shape[1], lists), alpha=alpha, n_iterations=M, seed=seed, return_draws=True,
                            stream_ids=None if default_ids else ids, **kw)
    assert np.array_equal(got[3], want[3]), "c"
    assert np.array_equal(got[2], want[2]), "m"
    assert np.array_equal(got[1], want[1]), "D"
    assert np.array_equal(_bits(got[0]), _bits(want[0])), "contrast"
    assert got[1].dtype == np.int64 and got[2].dtype == np.int32 and got[0].dtype == np.float64
    return want


# ---- 1. argsort and rank ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("d", [1, 5])
@pytest.mark.parametrize("n", [2, 3, 255, 256, 257, 1000, 2048, 2049, 4099])
def test_argsort_and_rank(n, d):
    from vgan_amd.hics import HICS_SORT_RUN
    assert HICS_SORT_RUN == 2048  # 2049 is the first n above the local sort, 4099 needs two strided stages
    X = _tied_data(n, d, n + d)
    order, rank = _argsort_on_device(X)
    want_order, want_rank = R.order_rank(X)
    assert np.array_equal(order, want_order) and np.array_equal(rank, want_rank)


# ---- 2. the draws --------------------------------------------------------------------------------------------------------
def _mixed_lists(d, seed):
    """k = 2, 3, 4, 5 (the Philox block edge), 9 and d, and two sets below two features, in one call."""
    rng = np.random.default_rng(seed)
    lists = [sorted(rng.choice(d, size=k, replace=False).tolist()) for k in (2, 3, 4, 5, 9)]
    return lists[:2] + [[7]] + lists[2:] + [[], list(range(d)), [0, d - 1]]


@pytest.mark.parametrize("alpha,M", [(0.1, 50), (0.5, 50), (0.1, 1), (0.5, 1)])
@pytest.mark.parametrize("n", [2, 3, 63, 64, 65, 1000, 4097])
def test_draws_and_contrast_equal_the_restatement(n, alpha, M):
    d = 40
    X = R.dep_data(n, n=n, d=d)
    lists = _mixed_lists(d, n)
    want = _check(X, lists, alpha, M, seed=11 + n, default_ids=True)
    short = [z for z, f in enumerate(lists) if len(f) < 2]
    assert len(short) == 2 and not want[0][short].any() and (want[3][short] == -1).all()


@pytest.mark.parametrize("group", [1, 4])
def test_both_workgroup_shapes(group):
    from vgan_amd.hics import ContrastIndex
    X = R.dep_data(5, n=1000, d=12)
    lists = [[0, 1], [2, 3, 4], [0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11], [5, 9]]
    off = np.concatenate([[0], np.cumsum([len(f) for f in lists])])
    index = ContrastIndex(X)
    for alpha, M in ((0.1, 50), (0.5, 7)):  # M = 50 leaves two idle waves in the last group of four
        want = _restate(X, lists, alpha, M, 3, np.arange(4))
        got = index.contrast(np.concatenate(lists), off, alpha, M, 3, np.arange(4), return_draws=True, group=group)
        assert np.array_equal(_bits(got[0]), _bits(want[0])) and np.array_equal(got[1], want[4])
        assert all(np.array_equal(got[2 + i], want[1 + i]) for i in range(3))


@pytest.mark.parametrize("n", [16384, 16385])
def test_the_library_changes_shape_between_these_rows(n):
    """Up to 2^14 rows the library gives a draw to a wave, beyond to a workgroup: the same numbers on both sides."""
    X = R.dep_data(n, n=n, d=8)
    _check(X, [[0, 1], [2, 3, 4], [0, 1, 2, 3, 4, 5, 6, 7], [1, 6]], 0.1, 5, seed=n)


def test_full_slices_select_every_row():
    n = 65
    X = R.dep_data(2, n=n, d=6)
    from vgan_amd.hics import hics_slice_width
    assert hics_slice_width(n, 2, 0.999) == n
    want = _check(X, [[0, 1], [2, 4]], 0.999, 50)
    assert (want[2] == n).all() and (want[1] == 0).all() and not want[0].any()


def test_empty_draws_are_counted():
    from vgan_amd.hics import ContrastIndex
    n, d = 65, 12
    X = np.random.default_rng(8).standard_normal((n, d)).astype(np.float32)
    # alpha = 0.1 leaves about 6 rows a draw at n = 65 and the restatement sees no empty draw; alpha = 0.01 leaves 0.65:
    # w = 37 at k = 9 (the complement path), 7 at k = 3 and 15 at k = 4 (the two-map path)
    lists = [[0, 1, 2, 3, 4, 5, 6, 7, 8], [1, 2, 3, 5, 7, 8, 9, 10, 11], [2, 5, 9], [0, 3, 4, 11]]
    want = _check(X, lists, 0.01, 50)
    assert (want[4] >= 20).all() and ((want[2] == 0).sum(axis=1) == want[4]).all()
    off = np.array([0, 9, 18, 21, 25])
    got = ContrastIndex(X).contrast(np.concatenate(lists), off, 0.01, 50, 0, np.arange(4))
    assert np.array_equal(got[1], want[4]) and np.array_equal(_bits(got[0]), _bits(want[0]))


def test_maximum_inside_one_bitmap_word():
    """Feature 1 is an increasing function of feature 0, so the 7 rows of a slice sit at 7 consecutive positions of the
    comparison feature and |cnt(r) n - r m| peaks at the slice's end: inside a 32-bit word, not at its end."""
    n = 65
    x = np.random.default_rng(4).standard_normal(n).astype(np.float32)
    X = np.stack([x, np.exp(x)], axis=1).astype(np.float32)
    assert len(np.unique(X[:, 1])) == n
    want = _check(X, [[0, 1]], 0.1, 50)
    inside = 0
    for t in range(50):
        c, starts = R.draw(n, 2, 7, t, 0, 0)
        s = starts[1 - c]
        inside += (s >> 5) == ((s + 6) >> 5) and (s + 7) % 32 != 0 and s % 32 != 0
        assert want[1][0, t] == max(s * 7, (n - s - 7) * 7)  # the slice's two ends, worked by hand
    assert inside >= 10


def test_short_subspaces_score_zero_beside_others():
    from vgan_amd import subspace_contrast
    X = R.dep_data(0)
    mask = _mask(8, [[0, 1], [3], [], [2, 3, 4]])
    con, D, m, c = subspace_contrast(X, mask, return_draws=True)
    assert con[1] == 0.0 and con[2] == 0.0 and con[0] > 0.45 and con[3] > 0.22
    assert not D[1:3].any() and not m[1:3].any() and (c[1:3] == -1).all() and (c[[0, 3]] >= 0).all()


# ---- 3. invariance -------------------------------------------------------------------------------------------------------
def test_contrast_does_not_depend_on_chunks_company_or_the_run():
    from vgan_amd import subspace_contrast
    X = R.dep_data(3, n=300, d=10)
    lists = [[0, 1], [2, 3, 4], [1, 5, 6, 7, 8], [4], [0, 9], list(range(10)), [3, 7]]
    mask = _mask(10, lists)
    ids = [(2 << 32) | 5, 7, 2 ** 64 - 1, 3, 0, (5 << 32), 11]
    base = subspace_contrast(X, mask, n_iterations=20, seed=9, stream_ids=ids)
    for ws in (1, 20 * 16, 3 * 20 * 16, 1 << 20):  # one subspace a launch, one, three, all
        assert np.array_equal(_bits(subspace_contrast(X, mask, n_iterations=20, seed=9, stream_ids=ids, workspace_bytes=ws)), _bits(base))
    assert np.array_equal(_bits(subspace_contrast(X, mask, n_iterations=20, seed=9, stream_ids=ids)), _bits(base))
    for z in range(len(lists)):
        alone = subspace_contrast(X, mask[z:z + 1], n_iterations=20, seed=9, stream_ids=[ids[z]])
        assert _bits(alone)[0] == _bits(base)[z]
    assert not np.array_equal(subspace_contrast(X, mask, n_iterations=20, seed=10, stream_ids=ids), base)


def test_the_row_limit():
    """n = HICS_MAX_ROWS: the two maps fill 64 KB of LDS and the scratch words lie behind them."""
    from vgan_amd import subspace_contrast
    from vgan_amd.hics import HICS_MAX_ROWS
    n = HICS_MAX_ROWS
    X = np.random.default_rng(1).standard_normal((n, 3)).astype(np.float32)
    X[:, 1] += X[:, 0]
    order, rank = _argsort_on_device(X)
    want_order, want_rank = R.order_rank(X)
    assert np.array_equal(order, want_order) and np.array_equal(rank, want_rank)
    _check(X, [[0, 1], [0, 1, 2], [1, 2]], 0.1, 2)
    _check(X, [[0, 1, 2]], 0.5, 1)  # 2 w > n: the complement path
    with pytest.raises(ValueError, match="HICS_MAX_ROWS"):
        subspace_contrast(np.zeros((n + 1, 2), dtype=np.float32), np.ones((1, 2), dtype=bool))
    with pytest.raises(ValueError, match="HICS_MAX_ROWS"):
        subspace_contrast(np.zeros((1, 2), dtype=np.float32), np.ones((1, 2), dtype=bool))


def test_nan_input_neither_faults_nor_hangs():
    from vgan_amd import subspace_contrast
    X = R.dep_data(0)
    X[::5, 1] = np.nan
    X[3, 2] = np.inf
    con = subspace_contrast(X, _mask(8, [[0, 1], [1, 2, 3]]))
    assert con.shape == (2,) and np.isfinite(con).all()


# ---- 4. the search ---------------------------------------------------------------------------------------------------------
def test_fit_equals_the_restated_search():
    from vgan_amd import HiCS
    X = R.dep_data(0)
    want = R.search(X, max_dim=4, candidate_cutoff=20, n_subspaces=15)
    got = HiCS(max_dim=4, candidate_cutoff=20, n_subspaces=15).fit(X)
    assert len(got.levels_) == len(want["levels"]) == 3
    for lg, lw in zip(got.levels_, want["levels"]):
        assert lg["k"] == lw["k"] and [tuple(r) for r in lg["candidates"].tolist()] == lw["candidates"]
        assert np.array_equal(_bits(lg["contrast"]), _bits(lw["contrast"]))
        assert lg["kept"].tolist() == lw["kept"] and lg["n_empty"].tolist() == lw["n_empty"]
    assert np.array_equal(got.subspaces, want["subspaces"]) and got.subspaces.dtype == bool
    assert np.array_equal(_bits(got.contrast_), _bits(want["contrast"]))
    assert np.array_equal(_bits(got.proba), _bits(want["proba"]))
    assert np.array_equal(got.n_empty_, want["n_empty"])
    uniform = HiCS(max_dim=3, weights="uniform").fit(X)
    assert np.array_equal(uniform.proba, np.full(len(uniform.proba), 1.0 / len(uniform.proba)))


def test_hics_lof_finds_the_hidden_outliers():
    from sklearn.metrics import roc_auc_score
    from vgan_amd import HiCS, SubspaceEnsemble
    X, y = R.hidden_outlier_data(0)
    found = HiCS(n_subspaces=10).fit(X)
    ens = found.outlier_ensemble(method="lof", n_neighbors=20, X=X)
    assert type(ens) is SubspaceEnsemble and ens.method == "lof"
    assert roc_auc_score(y, ens.decision_scores_) >= 0.99
    assert found.subspaces[0].nonzero()[0].tolist() == [0, 1]


def test_model_subspace_contrast():
    import vgan_amd
    from test_outlier_gpu import _planted
    X = _planted()[:, :10]
    model = vgan_amd.VGAN_no_kl(epochs=2)
    model.fit(X)
    con = model.subspace_contrast(X, n_iterations=10, seed=4)
    assert model.subspaces is not None and con.shape == (model.subspaces.shape[0],) and con.dtype == np.float64
    want = vgan_amd.subspace_contrast(X, model.subspaces, n_iterations=10, seed=4)
    assert np.array_equal(_bits(con), _bits(want))
    assert ((con >= 0) & (con <= 1)).all()
