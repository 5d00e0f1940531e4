"""Per-subspace score normalisation, combination rules and decisions of the outlier ensemble (CPU tier): the float64
restatement of the contract in v-gan_amd/outlier.py, pinned to sklearn / scipy / numpy where they are installed, the
planted data set the GPU tier uses, and everything of the feature that needs no device (argument validation, the
decision functions, the C-ABI argument checks)."""
import math

import numpy as np
import pytest

MAD_TO_SIGMA = 0.6744897501960817  # Phi^-1(3 / 4)


# ---- restatement (float64 numpy, from the contract) ----------------------------------------------------------------
def _median(x):
    """Half the sum of the two middle order statistics (the same one twice for odd n)."""
    x = np.sort(np.asarray(x, dtype=np.float64))
    n = x.shape[0]
    return (x[(n - 1) // 2] + x[n // 2]) / 2.0


def restate_stats(per, how):
    """(center, scale) float64 [S] of the rows of per [S, n] (float32 scores taken as float64); zero scale -> 1."""
    per = np.asarray(per)
    center, scale = np.empty(per.shape[0]), np.empty(per.shape[0])
    for s in range(per.shape[0]):
        x = per[s].astype(np.float64)
        if how == "zscore":
            c = x.mean()
            w = math.sqrt(((x - c) ** 2).mean())
        elif how == "robust":
            c = _median(x)
            w = _median(np.abs(x - c)) / MAD_TO_SIGMA
        elif how == "minmax":
            c = x.min()
            w = x.max() - x.min()
        else:
            raise ValueError(how)
        center[s], scale[s] = c, (w if w != 0.0 else 1.0)
    return center, scale


def restate_transform(per, center, scale):
    t = np.asarray(per).astype(np.float64)
    if center is not None:
        t = (t - np.asarray(center)[:, None]) / np.asarray(scale)[:, None]
    return t


def restate_combine(per, proba, center, scale, combination):
    """float64 [n]: sum_s p_s t_s (subspaces in order) or max_s t_s; center / scale None: t_s is the raw score."""
    t = restate_transform(per, center, scale)
    if combination == "max":
        return t.max(axis=0)
    assert combination == "sum"
    out = np.zeros(t.shape[1])
    for s, p in enumerate(np.asarray(proba, dtype=np.float64)):
        out += p * t[s]
    return out


def restate_threshold(scores, contamination):
    """The linear-interpolation percentile at q = 1 - contamination, written out."""
    x = np.sort(np.asarray(scores, dtype=np.float64))
    pos = (1.0 - contamination) * (x.shape[0] - 1)
    lo = int(math.floor(pos))
    hi = min(lo + 1, x.shape[0] - 1)
    return x[lo] + (x[hi] - x[lo]) * (pos - lo)


def restate_proba(train_scores, scores, method):
    train = np.asarray(train_scores, dtype=np.float64)
    s = np.asarray(scores, dtype=np.float64)
    if method == "linear":
        width = train.max() - train.min()
        p = (s - train.min()) / (width if width != 0.0 else 1.0)
    elif method == "unify":
        sigma = math.sqrt(((train - train.mean()) ** 2).mean())
        z = (s - train.mean()) / ((sigma if sigma != 0.0 else 1.0) * math.sqrt(2.0))
        p = np.array([math.erf(v) for v in z])
    else:
        raise ValueError(method)
    p = np.clip(p, 0.0, 1.0)
    return np.stack([1.0 - p, p], axis=1)


# ---- the planted data set --------------------------------------------------------------------------------------------
def planted_band(seed=6, n=2000, m=10, d=30):
    rng = np.random.default_rng(seed)
    X = rng.normal(size=(n + m, d))
    X[:, 1] = X[:, 0] + 0.05 * rng.normal(size=n + m)      # features 0 and 1: a thin diagonal band
    t = np.linspace(-1.5, 1.5, m)
    sg = np.where(np.arange(m) % 2 == 0, 1.0, -1.0)
    X[n:, 0], X[n:, 1] = t + sg, t - sg                      # planted rows: inside both marginals, off the band
    return X.astype(np.float32)


def planted_band_subspaces(seed=6, d=30, wide=6, ds=20):
    rng = np.random.default_rng(seed)
    mask = np.zeros((1 + wide, d), bool)
    mask[0, [0, 1]] = True
    for s in range(1, 1 + wide):
        mask[s, rng.choice(np.arange(2, d), ds, replace=False)] = True
    p = np.full(1 + wide, 0.5 / wide)
    p[0] = 0.5
    return mask, p


def separation(scores, m=10):
    """min over the planted rows (the last m) / max over the inliers: above 1 when every planted row outranks every inlier."""
    return float(scores[-m:].min() / scores[:-m].max())


def _rows(kind, n, rng):
    if kind == "constant":
        return np.full(n, 1.25, dtype=np.float32)
    if kind == "ties":
        return rng.integers(-3, 4, size=n).astype(np.float32)
    return (rng.normal(size=n) * 3.0 - 0.5).astype(np.float32)


CASES = [(kind, n) for kind in ("normal", "ties", "constant") for n in (1, 2, 7, 8, 777, 1000)]


# ---- the restatement against the libraries ---------------------------------------------------------------------------
@pytest.mark.parametrize("kind,n", CASES)
def test_restated_zscore_is_sklearns_standard_scaler(kind, n):
    pre = pytest.importorskip("sklearn.preprocessing")
    x = _rows(kind, n, np.random.default_rng(n))
    sc = pre.StandardScaler().fit(x.astype(np.float64)[:, None])
    c, w = restate_stats(x[None], "zscore")
    np.testing.assert_allclose(c[0], sc.mean_[0], rtol=1e-12, atol=1e-12 * np.abs(x).mean())
    if kind == "constant" or n == 1:
        assert w[0] == 1.0 and sc.scale_[0] == 1.0
    else:
        np.testing.assert_allclose(w[0], sc.scale_[0], rtol=1e-12)
    np.testing.assert_allclose(restate_transform(x[None], c, w)[0], sc.transform(x.astype(np.float64)[:, None])[:, 0], rtol=1e-12,
                               atol=1e-12)


@pytest.mark.parametrize("kind,n", CASES)
def test_restated_minmax_is_sklearns_minmax_scaler(kind, n):
    pre = pytest.importorskip("sklearn.preprocessing")
    x = _rows(kind, n, np.random.default_rng(n))
    sc = pre.MinMaxScaler().fit(x.astype(np.float64)[:, None])
    c, w = restate_stats(x[None], "minmax")
    assert c[0] == sc.data_min_[0]
    assert w[0] == (1.0 if (kind == "constant" or n == 1) else sc.data_range_[0])
    np.testing.assert_allclose(restate_transform(x[None], c, w)[0], sc.transform(x.astype(np.float64)[:, None])[:, 0], rtol=1e-12,
                               atol=1e-15)


@pytest.mark.parametrize("kind,n", CASES)
def test_restated_robust_is_numpys_median_and_scipys_mad(kind, n):
    stats = pytest.importorskip("scipy.stats")
    x = _rows(kind, n, np.random.default_rng(n))
    c, w = restate_stats(x[None], "robust")
    assert c[0] == np.median(x.astype(np.float64))
    mad = stats.median_abs_deviation(x.astype(np.float64), scale="normal")
    if mad == 0.0:
        assert w[0] == 1.0
    else:
        np.testing.assert_allclose(w[0], mad, rtol=1e-14)


@pytest.mark.parametrize("contamination", [0.005, 0.1, 0.25, 0.5])
@pytest.mark.parametrize("n", [1, 2, 11, 2010])
def test_restated_threshold_is_numpys_percentile(n, contamination):
    x = np.random.default_rng(n).normal(size=n)
    np.testing.assert_allclose(restate_threshold(x, contamination), np.percentile(x, 100 * (1 - contamination)), rtol=1e-13)


def test_restated_combination_rules():
    per = np.array([[1.0, 2.0, 4.0], [10.0, 30.0, 20.0]], dtype=np.float32)
    np.testing.assert_array_equal(restate_combine(per, [0.25, 0.75], None, None, "sum"), [7.75, 23.0, 16.0])
    np.testing.assert_array_equal(restate_combine(per, [0.25, 0.75], None, None, "max"), [10.0, 30.0, 20.0])
    c, w = restate_stats(per, "minmax")
    np.testing.assert_array_equal(restate_combine(per, [0.25, 0.75], c, w, "max"), [0.0, 1.0, 1.0])


# ---- the planted data set: what normalisation buys -------------------------------------------------------------------
def _sklearn_knn_scores(X, mask, k=5):
    nb = pytest.importorskip("sklearn.neighbors")
    per = np.empty((mask.shape[0], X.shape[0]), dtype=np.float32)
    for s in range(mask.shape[0]):
        A = X[:, mask[s]].astype(np.float64)
        per[s] = nb.NearestNeighbors(n_neighbors=k).fit(A).kneighbors()[0][:, -1]
    return per


def test_planted_band_needs_normalisation():
    """Seed 6: raw min(planted) / max(inlier) is 0.92 with 5 planted rows among the 10 highest; z-score 2.34, robust 3.06."""
    X = planted_band()
    mask, p = planted_band_subspaces()
    per = _sklearn_knn_scores(X, mask)
    raw = restate_combine(per, p, None, None, "sum")
    assert separation(raw) < 1.0  # at least one inlier outranks a planted row
    assert np.sum(np.argsort(-raw)[:10] >= 2000) < 10
    for how in ("zscore", "robust"):
        c, w = restate_stats(per, how)
        assert separation(restate_combine(per, p, c, w, "sum")) > 1.0, how
        assert separation(restate_combine(per, p, c, w, "max")) > 1.0, how
    assert separation(restate_combine(per, p, None, None, "max")) < 1.0


# ---- validation without a device -------------------------------------------------------------------------------------
_MASK = np.ones((2, 3), bool)

BAD = {"normalize": ["Zscore", "mean", "z-score", "", 1, True, False, b"zscore", ["zscore"]],
       "combination": ["Sum", "mean", "average", None, 0, True, b"max", ["max"]],
       "contamination": [0, 0.0, 0.6, 0.5000001, 1, -0.1, float("nan"), float("inf"), True, False, "0.1", None, [0.1]]}
GOOD = {"normalize": [None, "zscore", "robust", "minmax"], "combination": ["sum", "max"],
        "contamination": [0.5, 0.1, 1e-9, np.float32(0.25), np.float64(0.005)]}


@pytest.mark.parametrize("name", sorted(BAD))
def test_bad_values_are_value_errors_that_name_the_argument(name):
    import vgan_amd
    from vgan_amd import outlier
    check = getattr(outlier, "check_" + name)
    for bad in BAD[name]:
        with pytest.raises(ValueError, match=name):
            check(bad)
        with pytest.raises(ValueError, match=name):  # before default_ops(): no GPU needed
            vgan_amd.SubspaceEnsemble(_MASK, [0.5, 0.5], **{name: bad})
    for good in GOOD[name]:
        got = check(good)
        assert got == good or got is good


def test_existing_messages_keep_their_wording():
    import vgan_amd
    with pytest.raises(ValueError, match="method must be 'knn', 'lof' or 'kde', got 'abod'"):
        vgan_amd.SubspaceEnsemble(_MASK, [0.5, 0.5], method="abod", normalize="nope")


# ---- decisions -------------------------------------------------------------------------------------------------------
def test_decision_threshold_and_labels():
    from vgan_amd.outlier import decision_threshold
    rng = np.random.default_rng(3)
    for n, c in [(2010, 0.005), (100, 0.1), (7, 0.5), (1, 0.1)]:
        x = rng.normal(size=n)
        thr = decision_threshold(x, c)
        assert isinstance(thr, float)
        np.testing.assert_allclose(thr, restate_threshold(x, c), rtol=1e-13)
        assert thr == np.percentile(x, 100 * (1 - c))
    # ties at the threshold are inliers (strict >), constant scores label nothing
    x = np.array([0.0] * 8 + [1.0, 1.0])
    thr = decision_threshold(x, 0.1)
    assert thr == 1.0 and int((x > thr).sum()) == 0
    assert decision_threshold(np.full(5, 2.5), 0.1) == 2.5
    for bad in (0, 0.6, float("nan"), "0.1", True):
        with pytest.raises(ValueError, match="contamination"):
            decision_threshold(x, bad)


@pytest.mark.parametrize("method", ["linear", "unify"])
def test_outlier_probability(method):
    from vgan_amd.outlier import outlier_probability
    rng = np.random.default_rng(4)
    train, new = rng.normal(size=500) * 2 + 1, rng.normal(size=130) * 4 + 1
    got = outlier_probability(train, new, method)
    assert got.dtype == np.float64 and got.shape == (130, 2)
    np.testing.assert_allclose(got, restate_proba(train, new, method), rtol=1e-12, atol=1e-15)
    np.testing.assert_allclose(got.sum(axis=1), 1.0, rtol=1e-15)
    assert got.min() >= 0.0 and got.max() <= 1.0 and (got[:, 1] == 0.0).any()  # the clip is exercised
    const = outlier_probability(np.full(9, 3.0), [2.0, 3.0, 3.5, 9.0], method)
    np.testing.assert_allclose(const, restate_proba(np.full(9, 3.0), [2.0, 3.0, 3.5, 9.0], method), rtol=1e-12)
    assert np.isfinite(const).all()


def test_unify_is_scipys_erf():
    special = pytest.importorskip("scipy.special")
    from vgan_amd.outlier import outlier_probability
    rng = np.random.default_rng(5)
    train, new = rng.normal(size=300), rng.normal(size=50) * 2
    want = np.clip(special.erf((new - train.mean()) / (train.std() * np.sqrt(2))), 0, 1)
    np.testing.assert_allclose(outlier_probability(train, new, "unify")[:, 1], want, rtol=1e-12, atol=1e-15)


def test_unknown_probability_method():
    from vgan_amd.outlier import outlier_probability
    for bad in ("Linear", "erf", None, 1):
        with pytest.raises(ValueError, match="method"):
            outlier_probability([0.0, 1.0], [0.5], bad)


# ---- the C ABI -------------------------------------------------------------------------------------------------------
def test_norm_entries_reject_bad_arguments_without_gpu():
    import ctypes
    import vgan_amd
    lib = vgan_amd.lib.load()
    null = None
    buf = ctypes.create_string_buffer(256)
    p = ctypes.cast(ctypes.addressof(buf) + (-ctypes.addressof(buf)) % 16, ctypes.c_void_p)  # 16-byte aligned, never read
    odd = ctypes.c_void_p(p.value + 8)

    def rejected(rc):
        msg = lib.vgan_last_error()
        return rc == 1 and b"bad argument" in msg and b"outlier_norm.hip" in msg

    def stats(score=p, ld=10, S=3, n=10, mode=1, center=p, scale=p, ws=p, ws_bytes=1 << 20):
        return lib.vgan_outlier_score_stats(score, ld, S, n, mode, center, scale, ws, ws_bytes, null)

    for name in ["score", "center", "scale", "ws"]:
        assert rejected(stats(**{name: null})), name
    for mode in (0, 4, -1):
        assert rejected(stats(mode=mode)), mode
    assert rejected(stats(S=0))
    assert rejected(stats(S=65536))
    assert rejected(stats(n=0))
    assert rejected(stats(ld=9))  # ld < n
    assert rejected(stats(ws=odd))  # workspace not 16-byte aligned
    for mode in (1, 2, 3):
        need = lib.vgan_outlier_score_stats_ws_bytes(3, 10, mode)
        assert need > 0
        assert rejected(stats(mode=mode, ws_bytes=need - 1)), mode
    assert lib.vgan_outlier_score_stats_ws_bytes(500, 50000, 2) == 500 * (32 + 2048)
    for bad in [(0, 10, 1), (3, 0, 1), (3, 10, 0), (3, 10, 4), (65536, 10, 1)]:
        assert lib.vgan_outlier_score_stats_ws_bytes(*bad) == -1 and b"bad argument" in lib.vgan_last_error()

    def combine(score=p, ld=10, S=3, n=10, center=p, scale=p, weights=p, combination=0, out=p):
        return lib.vgan_outlier_combine_normalized(score, ld, S, n, center, scale, weights, combination, out, null)

    for name in ["score", "out", "weights"]:
        assert rejected(combine(**{name: null})), name
    assert rejected(combine(center=p, scale=null))  # center given without scale
    assert rejected(combine(center=null, scale=p))
    for combination in (2, -1):
        assert rejected(combine(combination=combination)), combination
    assert rejected(combine(S=0))
    assert rejected(combine(n=0))
    assert rejected(combine(ld=9))


def test_norm_constants_match_the_header():
    import os
    import re
    from conftest import REPO
    from vgan_amd import outlier
    text = open(os.path.join(REPO, "include", "vgan_hip.h")).read()
    defs = {k: int(v) for k, v in re.findall(r"#define (VGAN_OUTLIER_(?:NORM|COMBINE)_[A-Z]+) (\d+)", text)}
    assert {k: defs["VGAN_OUTLIER_NORM_" + k.upper()] for k in outlier.NORMALIZATIONS} == outlier.NORMALIZATIONS
    assert {k: defs["VGAN_OUTLIER_COMBINE_" + k.upper()] for k in outlier.COMBINATIONS} == outlier.COMBINATIONS
    assert len(defs) == 5
