"""ECOD over the subspaces, CPU tier: the float64 numpy restatement the GPU tests compare against, pinned to scipy
(tail counts to rankdata, skew signs to skew) and to cases worked by hand, and everything of vgan_amd.SubspaceECOD that
runs without a device (argument checks, the chunk rule, the dispatch from the model, the C ABI's argument checks).

The definition (SubspaceECOD's docstring): X as float32, arithmetic in float64, -0.0 as +0.0.  Per feature cl = #{<= x},
cr = #{>= x} among the n fitted rows; fit: ul = -log(cl / n), ur = -log(cr / n); a new row: -log((c + 1) / (n + 1)), the
row scored alone and appended; usk = ul, ur or ul + ur by the fit-time skew sign (-1, +1, 0)."""
import ctypes
import os
import re
import warnings

import numpy as np
import pytest

from conftest import REPO


def _f32(X):
    X = np.asarray(X, dtype=np.float32).astype(np.float64)
    return X + 0.0  # -0.0 + 0.0 is +0.0


def restate_counts(X_fit, X_query):
    """(cl, cr) int64 [nq, d]: upper_bound and n - lower_bound of every query value in the sorted fitted column."""
    A, Q = _f32(X_fit), _f32(X_query)
    n, d = A.shape
    cl, cr = np.empty(Q.shape, np.int64), np.empty(Q.shape, np.int64)
    for f in range(d):
        col = np.sort(A[:, f])
        cl[:, f] = np.searchsorted(col, Q[:, f], side="right")
        cr[:, f] = n - np.searchsorted(col, Q[:, f], side="left")
    return cl, cr


def restate_skew_sign(X_fit):
    """int64 [d]: 0 if m2 == 0 else sign(m3), two passes about mu = sum(x) / n."""
    A = _f32(X_fit)
    mu = A.sum(axis=0) / A.shape[0]
    m2 = ((A - mu) ** 2).sum(axis=0)
    m3 = ((A - mu) ** 3).sum(axis=0)
    return np.where(m2 == 0, 0, np.sign(m3)).astype(np.int64)


def restate_terms(X_fit, X_query=None, signs=None):
    """(ul, ur, usk) float64 [nq, d]; X_query None: the fit rule on X_fit itself.  signs: the fit-time signs (default: those
    of X_fit)."""
    n = np.asarray(X_fit).shape[0]
    g = restate_skew_sign(X_fit) if signs is None else np.asarray(signs)
    cl, cr = restate_counts(X_fit, X_fit if X_query is None else X_query)
    a = 0 if X_query is None else 1
    ul = -np.log((cl + a).astype(np.float64) / float(n + a))
    ur = -np.log((cr + a).astype(np.float64) / float(n + a))
    usk = np.where(g < 0, ul, np.where(g > 0, ur, ul + ur))
    return ul, ur, usk


def restate_ecod(X_fit, X_query, feats_list, aggregate, signs=None):
    """float64 [S, nq]: the per-subspace ECOD scores before the rounding to float32."""
    ul, ur, usk = restate_terms(X_fit, X_query, signs)
    out = np.empty((len(feats_list), ul.shape[0]))
    for s, feats in enumerate(feats_list):
        f = np.asarray(feats)
        if aggregate == "dimension":
            out[s] = np.maximum(np.maximum(ul, ur), usk)[:, f].sum(axis=1)
        elif aggregate == "tail":
            out[s] = np.maximum(np.maximum(ul[:, f].sum(axis=1), ur[:, f].sum(axis=1)), usk[:, f].sum(axis=1))
        else:
            raise ValueError(aggregate)
    return out


def tied_data(n, d, seed):
    """float32 [n, d]: continuous columns, then (as d allows) heavy integer ties, +-0.0 among small integers, a constant
    column and a descending column."""
    rng = np.random.default_rng(seed)
    X = rng.normal(size=(n, d)).astype(np.float32)
    if d > 1:
        X[:, 1] = rng.integers(0, 4, size=n)
    if d > 2:
        X[:, 2] = rng.integers(-1, 2, size=n) * np.where(rng.random(n) < 0.5, 0.0, 1.0)
        X[rng.random(n) < 0.3, 2] = -0.0
    if d > 3:
        X[:, 3] = 2.5
    if d > 4:
        X[:, 4] = np.arange(n, 0, -1)
    return X


def _mask(d, feature_lists):
    m = np.zeros((len(feature_lists), d), bool)
    for s, feats in enumerate(feature_lists):
        m[s, feats] = True
    return m


# ---- the restatement, pinned ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 2, 7, 300])
def test_counts_are_scipys_max_ranks(n):
    from scipy.stats import rankdata
    X = tied_data(n, 6, seed=n)
    cl, cr = restate_counts(X, X)
    A = _f32(X)
    for f in range(6):
        np.testing.assert_array_equal(cl[:, f], rankdata(A[:, f], method="max"))
        np.testing.assert_array_equal(cr[:, f], rankdata(-A[:, f], method="max"))
    assert (cl >= 1).all() and (cr >= 1).all() and (cl + cr >= n + 1).all()  # the row counts itself on both sides


def test_signs_are_scipys_skew_sign():
    from scipy.stats import skew
    rng = np.random.default_rng(2)
    X = np.concatenate([rng.normal(size=(500, 20)), rng.lognormal(size=(500, 3)), -rng.lognormal(size=(500, 3)),
                        np.full((500, 1), 4.0)], axis=1).astype(np.float32)
    got = restate_skew_sign(X)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")  # scipy warns about the constant column, whose NaN is not pinned
        want = skew(_f32(X), axis=0)
    pinned = np.isfinite(want) & (want != 0)
    assert pinned[:26].all() and pinned.sum() >= 26
    np.testing.assert_array_equal(got[pinned], np.sign(want[pinned]).astype(np.int64))
    assert (got[20:23] == 1).all() and (got[23:26] == -1).all() and got[26] == 0  # the constant column: sign 0, not NaN


def test_hand_computed_case():
    """Column 0 = (1, 1, 3, 5, 5): ties, exactly symmetric (mu = 3, m3 = 0, sign 0, usk = ul + ur); column 1 constant (every
    count 5, every term 0)."""
    X = np.array([[1, 7], [1, 7], [3, 7], [5, 7], [5, 7]], np.float32)
    np.testing.assert_array_equal(restate_skew_sign(X), [0, 0])
    cl, cr = restate_counts(X, X)
    np.testing.assert_array_equal(cl[:, 0], [2, 2, 3, 5, 5])
    np.testing.assert_array_equal(cr[:, 0], [5, 5, 3, 2, 2])
    np.testing.assert_array_equal(cl[:, 1], 5)
    np.testing.assert_array_equal(cr[:, 1], 5)
    a, b = -np.log(0.4), -2.0 * np.log(0.6)  # the ends: ul + ur = -log(2/5) + 0; the middle: -log(3/5) twice
    for aggregate in ("dimension", "tail"):
        per = restate_ecod(X, None, [[0], [1], [0, 1]], aggregate)
        np.testing.assert_allclose(per[0], [a, a, b, a, a], rtol=1e-15)
        assert (per[1] == 0).all()
        np.testing.assert_array_equal(per[2], per[0])
    # a new row at 3 / 7: cl = cr = 3 -> (3 + 1) / (5 + 1) on both sides; at 0 / 7: cl = 0 -> 1 / 6, cr = 5 -> 6 / 6
    new = restate_ecod(X, np.array([[3, 7], [0, 7]], np.float32), [[0], [1]], "dimension")
    np.testing.assert_allclose(new[0], [-2.0 * np.log(4.0 / 6.0), -np.log(1.0 / 6.0)], rtol=1e-15)
    np.testing.assert_allclose(new[1], [-2.0 * np.log(6.0 / 6.0), 0.0], atol=0)


def test_the_two_aggregates_differ_where_they_should():
    """Feature 0 right-skewed (usk = ur), feature 1 left-skewed (usk = ul).  A row low in both: "dimension" adds the larger
    tail of each feature, "tail" takes the larger of the summed tails."""
    X = np.array([[0, 0], [1, 9], [2, 10], [3, 11], [10, 12]], np.float32)
    np.testing.assert_array_equal(restate_skew_sign(X), [1, -1])
    dim = restate_ecod(X, None, [[0, 1]], "dimension")[0]
    tail = restate_ecod(X, None, [[0, 1]], "tail")[0]
    np.testing.assert_allclose(dim[0], 2 * -np.log(0.2), rtol=1e-15)  # ul of both features
    np.testing.assert_allclose(tail[0], 2 * -np.log(0.2), rtol=1e-15)
    np.testing.assert_allclose(dim[4], 2 * -np.log(0.2), rtol=1e-15)  # ur of both
    # row 1: feature 0 cl = 2, cr = 4; feature 1 cl = 2, cr = 4
    np.testing.assert_allclose(dim[1], 2 * -np.log(0.4), rtol=1e-15)
    np.testing.assert_allclose(tail[1], 2 * -np.log(0.4), rtol=1e-15)
    # row 3: feature 0 cl = 4, cr = 2 (usk = ur); feature 1 cl = 4, cr = 2 (usk = ul)
    np.testing.assert_allclose(dim[3], 2 * -np.log(0.4), rtol=1e-15)
    np.testing.assert_allclose(tail[3], max(2 * -np.log(0.8), 2 * -np.log(0.4), -np.log(0.4) - np.log(0.8)), rtol=1e-15)
    assert (tail <= dim + 1e-15).all()  # a max of sums never exceeds the sum of maxima


def test_negative_zero_ties_with_zero():
    X = np.array([[-0.0], [0.0], [1.0], [-1.0], [-0.0]], np.float32)
    cl, cr = restate_counts(X, X)
    np.testing.assert_array_equal(cl[:, 0], [4, 4, 5, 1, 4])
    np.testing.assert_array_equal(cr[:, 0], [4, 4, 1, 5, 4])
    q = restate_counts(X, np.array([[-0.0], [0.0]], np.float32))
    np.testing.assert_array_equal(q[0][:, 0], [4, 4])
    np.testing.assert_array_equal(q[1][:, 0], [4, 4])


@pytest.mark.parametrize("aggregate", ["dimension", "tail"])
def test_a_new_row_is_scored_as_if_appended_alone(aggregate):
    """decision_function's rule, literally: append the one row to the training set, recompute by the fit rule with the
    fit-time signs, read off the appended row."""
    X, Y = tied_data(41, 6, seed=3), tied_data(9, 6, seed=4)
    Y[0] = X[5]   # a training row again
    Y[1] = -50.0  # below every minimum
    Y[2] = 500.0  # above every maximum
    feats = [[0, 1, 2], [3], [0, 2, 4, 5], list(range(6))]
    signs = restate_skew_sign(X)
    got = restate_ecod(X, Y, feats, aggregate)
    assert np.isfinite(got).all()
    for i in range(Y.shape[0]):
        appended = restate_ecod(np.vstack([X, Y[i:i + 1]]), None, feats, aggregate, signs=signs)
        np.testing.assert_array_equal(got[:, i], appended[:, -1])
    # and therefore scoring the training rows again is not the fit
    assert not np.array_equal(restate_ecod(X, X, feats, aggregate), restate_ecod(X, None, feats, aggregate))


# ---- the class, without a device ----------------------------------------------------------------------------------------------
def test_constructor_and_argument_errors_touch_no_device():
    import vgan_amd
    from vgan_amd import outlier
    m = _mask(4, [[0, 1], [2, 3]])
    ens = vgan_amd.SubspaceECOD(m, [0.5, 0.5])
    assert ens.aggregate == "dimension" and ens.ops is None and ens.workspace_bytes == outlier.DEFAULT_WORKSPACE_BYTES
    assert (ens.normalize, ens.combination, ens.contamination) == (None, "sum", 0.1)
    assert list(ens.plan.order) == [0, 1]
    for name in ("n_neighbors", "engine", "splits"):
        assert not hasattr(ens, name)
        with pytest.raises(TypeError):
            vgan_amd.SubspaceECOD(m, [0.5, 0.5], **{name: 1})
    for bad in ("sum", "max", None, 1):
        with pytest.raises(ValueError, match="aggregate"):
            vgan_amd.SubspaceECOD(m, [0.5, 0.5], aggregate=bad)
    with pytest.raises(ValueError, match="proba has 3 entries for 2 subspaces"):
        vgan_amd.SubspaceECOD(m, [0.5, 0.25, 0.25])
    with pytest.raises(ValueError, match="normalize"):
        vgan_amd.SubspaceECOD(m, [0.5, 0.5], normalize="l2")
    with pytest.raises(ValueError, match="combination"):
        vgan_amd.SubspaceECOD(m, [0.5, 0.5], combination="mean")
    with pytest.raises(ValueError, match="contamination"):
        vgan_amd.SubspaceECOD(m, [0.5, 0.5], contamination=0.7)
    with pytest.raises(ValueError, match="between 1 and"):
        ens.fit(np.empty((0, 4), np.float32))
    with pytest.raises(ValueError, match="4 features|features"):
        ens.fit(np.zeros((5, 3), np.float32))

    class Tall:  # only its shape is looked at before the row check raises
        shape = (outlier.ECOD_MAX_ROWS + 1, 4)

    assert outlier.ECOD_MAX_ROWS >= 1 << 22
    with pytest.raises(ValueError, match="between 1 and"):
        ens.fit(Tall())
    assert ens.ops is None  # none of this touched the device
    with pytest.raises(RuntimeError, match="not fitted"):
        ens.decision_function(np.zeros((5, 4), np.float32))
    with pytest.raises(RuntimeError, match="not fitted"):
        ens.sorted_columns_


def test_chunk_rows_follow_the_documented_rule():
    from vgan_amd.outlier import ecod_chunk_rows
    # per row: two int32 counts and one float64 term per feature, one float32 score per subspace
    assert ecod_chunk_rows(10, 3, "dimension", 1) == 1
    assert ecod_chunk_rows(10, 3, "dimension", 10 * 16 + 12) == 1
    assert ecod_chunk_rows(10, 3, "dimension", 2 * (10 * 16 + 12)) == 2
    assert ecod_chunk_rows(10, 3, "tail", 5 * (10 * 32 + 12) + 7) == 5
    assert ecod_chunk_rows(784, 500, "dimension", 1 << 30) == (1 << 30) // (784 * 16 + 2000)


def test_outlier_ensemble_routes_ecod_to_the_new_class():
    import vgan_amd
    model = vgan_amd.VGAN_no_kl(epochs=1)
    model.subspaces = _mask(6, [[0, 1], [2, 3, 5], [4]])
    model.proba = np.array([0.5, 0.3, 0.2])
    ens = model.outlier_ensemble(method="ecod")
    assert type(ens) is vgan_amd.SubspaceECOD and ens.aggregate == "dimension" and ens.plan.count == 3
    np.testing.assert_array_equal(ens.proba, model.proba)
    ens = model.outlier_ensemble(method="ecod", n_neighbors=17, aggregate="tail", normalize="robust", combination="max",
                                 contamination=0.05, workspace_bytes=1 << 20)  # n_neighbors is ignored
    assert (ens.aggregate, ens.normalize, ens.combination, ens.contamination, ens.workspace_bytes) == ("tail", "robust", "max", 0.05,
                                                                                                      1 << 20)
    assert not hasattr(ens, "n_neighbors")
    with pytest.raises(TypeError):
        model.outlier_ensemble(method="ecod", engine="exact")  # not a keyword of SubspaceECOD
    assert "ecod" in vgan_amd.VGAN_no_kl.outlier_ensemble.__doc__
    assert "SubspaceECOD" in vgan_amd.__all__


# ---- C ABI: argument checks without a GPU -----------------------------------------------------------------------------------
def test_ecod_entries_reject_bad_arguments_without_gpu():
    import vgan_amd
    from vgan_amd import outlier
    lib = vgan_amd.lib.load()
    header = open(os.path.join(REPO, "include", "vgan_hip.h")).read()
    assert int(re.search(r"#define VGAN_ECOD_SORT_RUN (\d+)", header).group(1)) == outlier.ECOD_SORT_RUN
    assert int(re.search(r"#define VGAN_ECOD_MAX_ROWS (\d+)", header).group(1)) == outlier.ECOD_MAX_ROWS
    run = outlier.ECOD_SORT_RUN
    assert run >= 512 and run & (run - 1) == 0
    null = None
    buf = ctypes.create_string_buffer(256)
    p = ctypes.cast(ctypes.addressof(buf) + (-ctypes.addressof(buf)) % 16, ctypes.c_void_p)  # never read

    def rejected(rc):
        msg = lib.vgan_last_error()
        return rc == 1 and b"bad argument" in msg and b"outlier_ecod.hip" in msg

    sort = lib.vgan_ecod_sort_columns
    assert rejected(sort(null, 4, 10, 4, p, 16, null))  # no data
    assert rejected(sort(p, 4, 10, 4, null, 16, null))  # no output
    assert rejected(sort(p, 3, 10, 4, p, 16, null))  # ldx < d
    assert rejected(sort(p, 4, 0, 4, p, 1, null))  # no rows
    assert rejected(sort(p, 4, outlier.ECOD_MAX_ROWS + 1, 4, p, 1 << 25, null))  # too many rows
    assert rejected(sort(p, 4, 10, 0, p, 16, null))  # no column
    assert rejected(sort(p, 4, 10, 4, p, 8, null))  # n_pad < n
    assert rejected(sort(p, 4, 10, 4, p, 12, null))  # n_pad no power of two
    assert rejected(sort(p, 4, 10, 4, p, 32, null))  # n_pad not the smallest
    skew = lib.vgan_ecod_skew_sign
    assert rejected(skew(null, 16, 10, 4, p, null))
    assert rejected(skew(p, 16, 10, 4, null, null))
    assert rejected(skew(p, 8, 10, 4, p, null))  # ld < n
    assert rejected(skew(p, 16, 0, 4, p, null))
    assert rejected(skew(p, 16, 10, 0, p, null))
    counts = lib.vgan_ecod_tail_counts
    assert rejected(counts(null, 4, 3, 4, p, 16, 10, p, p, null))
    assert rejected(counts(p, 4, 3, 4, null, 16, 10, p, p, null))
    assert rejected(counts(p, 4, 3, 4, p, 16, 10, null, p, null))
    assert rejected(counts(p, 4, 3, 4, p, 16, 10, p, null, null))
    assert rejected(counts(p, 3, 3, 4, p, 16, 10, p, p, null))  # ldq < d
    assert rejected(counts(p, 4, 0, 4, p, 16, 10, p, p, null))  # no query row
    assert rejected(counts(p, 4, 3, 4, p, 8, 10, p, p, null))  # ld < n
    assert rejected(counts(p, 4, 3, 4, p, 16, 0, p, p, null))  # no fitted row
    scores = lib.vgan_ecod_scores
    good = [p, p, 3, 4, p, 10, 0, 0, p, 2, 2, p, p, 3, null]
    for pos in (0, 1, 4, 8, 11, 12):
        assert rejected(scores(*[null if i == pos else v for i, v in enumerate(good)]))  # a missing pointer
    for pos, bad in ((2, 0), (3, 0), (5, 0), (7, 2), (7, -1), (9, 1), (10, 0), (13, 2)):  # rows, d, n, aggregate, ldm < S, S, ld < rows
        assert rejected(scores(*[bad if i == pos else v for i, v in enumerate(good)]))
    for name, nargs in (("vgan_ecod_sort_columns", 7), ("vgan_ecod_skew_sign", 6), ("vgan_ecod_tail_counts", 10),
                        ("vgan_ecod_scores", 15)):
        assert len(vgan_amd.lib.SIGNATURES[name][1]) == nargs
    assert vgan_amd.lib.ABI_VERSION == lib.vgan_abi_version()
