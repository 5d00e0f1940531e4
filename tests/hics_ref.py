"""TEST INFRASTRUCTURE ONLY: the plain numpy restatement of the HiCS contrast and search, written from the docstring of
vgan_amd.hics.HiCS.  Nothing here calls the library; the Philox words come from small_ops_ref.philox4x32_10.
tests/test_outlier_hics_cpu.py pins these functions (scipy's ks_2samp, numpy's stable argsort, brute-force joins, hand-worked
cases) and tests/test_outlier_hics_gpu.py holds the device to them."""
import math

import numpy as np

from small_ops_ref import philox4x32_10

TAG = 0x48494353
MASK64 = 2 ** 64 - 1


def order_rank(X):
    """(order, rank) int64 [d, n]: rows by (value with -0.0 as +0.0, row index) per column, and the inverse permutation."""
    X = np.asarray(X, dtype=np.float32)
    n, d = X.shape
    rows = np.arange(n)
    order = np.empty((d, n), dtype=np.int64)
    rank = np.empty((d, n), dtype=np.int64)
    for f in range(d):
        col = np.where(X[:, f] == 0, np.float32(0), X[:, f])
        order[f] = np.lexsort((rows, col))
        rank[f, order[f]] = rows
    return order, rank


def slice_width(n, k, alpha):
    return min(n, max(1, math.ceil(n * alpha ** (1.0 / (k - 1)))))


def _words(t, q, seed, stream_id):
    seed, stream_id = int(seed) & MASK64, int(stream_id) & MASK64
    k0 = (seed & 0xFFFFFFFF) ^ (stream_id & 0xFFFFFFFF)
    k1 = (seed >> 32) ^ (stream_id >> 32) ^ 0x5bd1e995
    return [int(w) for w in philox4x32_10((t, q, TAG, 0), k0, k1)]


def draw(n, k, w, t, seed, stream_id):
    """(c, starts): the comparison position of draw t and the slice start of every position (the one of c is unused)."""
    c = (_words(t, 0, seed, stream_id)[0] * k) >> 32
    blocks = [_words(t, 1 + b, seed, stream_id) for b in range((k + 3) // 4)]
    starts = [(blocks[p >> 2][p & 3] * (n - w + 1)) >> 32 for p in range(k)]
    return c, starts


def conditional_rows(order, feats, w, c, starts):
    """bool [n]: the rows that lie in the slice of every position but c."""
    member = np.ones(order.shape[1], dtype=bool)
    for p, f in enumerate(feats):
        if p != c:
            inside = np.zeros_like(member)
            inside[order[f, starts[p]:starts[p] + w]] = True
            member &= inside
    return member


def deviation_integers(member, order_c):
    """(D, m): m = |C| and D = max over r = 1 .. n of |cnt(r) n - r m|, cnt(r) the rows of C among the first r sort positions
    of the comparison feature."""
    n = len(member)
    cnt = np.cumsum(member[order_c].astype(np.int64))
    m = int(cnt[-1])
    r = np.arange(1, n + 1, dtype=np.int64)
    return int(np.abs(cnt * n - r * m).max()), m


def contrast(order, feats, alpha, n_iterations, seed, stream_id):
    """(contrast, D [M], m [M], c [M], n_empty) of one subspace; k < 2: (0.0, zeros, zeros, -1s, 0)."""
    n, k, M = order.shape[1], len(feats), n_iterations
    D, m, c = np.zeros(M, dtype=np.int64), np.zeros(M, dtype=np.int64), np.full(M, -1, dtype=np.int64)
    if k < 2:
        return 0.0, D, m, c, 0
    w = slice_width(n, k, alpha)
    total = 0.0
    for t in range(M):
        c[t], starts = draw(n, k, w, t, seed, stream_id)
        D[t], m[t] = deviation_integers(conditional_rows(order, feats, w, c[t], starts), order[feats[c[t]]])
        if m[t] > 0:
            total += float(D[t]) / float(n * int(m[t]))
    return total / M, D, m, c, int((m == 0).sum())


def join(sets):
    sets = sorted(set(sets))
    out = set()
    for a in sets:
        for b in sets:
            if a < b and a[:-1] == b[:-1]:
                out.add(a + (b[-1],))
    return sorted(out)


def select(sets, contrasts, count):
    return sorted(range(len(sets)), key=lambda i: (-contrasts[i], len(sets[i]), sets[i]))[:count]


def prune(sets, contrasts):
    keep = []
    for S, cS in zip(sets, contrasts):
        beaten = any(len(T) == len(S) + 1 and set(S) < set(T) and cT > cS for T, cT in zip(sets, contrasts))
        keep.append(not beaten)
    return keep


def search(X, alpha=0.1, n_iterations=50, candidate_cutoff=100, n_subspaces=100, max_dim=None, seed=0, weights="contrast"):
    """The search of the HiCS docstring: dict(levels, sets, contrast, n_empty, subspaces, proba)."""
    X = np.asarray(X, dtype=np.float32)
    n, d = X.shape
    order, _ = order_rank(X)
    max_dim = d if max_dim is None else min(max_dim, d)
    cands = [(a, b) for a in range(d) for b in range(a + 1, d)]
    levels, pool, pool_contrast, pool_empty = [], [], [], []
    k = 2
    while cands and k <= max_dim:
        res = [contrast(order, s, alpha, n_iterations, seed, (k << 32) | j) for j, s in enumerate(cands)]
        con = [r[0] for r in res]
        best = select(cands, con, candidate_cutoff)
        kept = [i in set(best) for i in range(len(cands))]
        levels.append({"k": k, "candidates": cands, "contrast": con, "n_empty": [r[4] for r in res], "kept": kept})
        for i in sorted(best):
            pool.append(cands[i])
            pool_contrast.append(con[i])
            pool_empty.append(res[i][4])
        cands = join([cands[i] for i in best])
        k += 1
    keep = prune(pool, pool_contrast)
    pool = [s for s, g in zip(pool, keep) if g]
    pool_contrast = [v for v, g in zip(pool_contrast, keep) if g]
    pool_empty = [v for v, g in zip(pool_empty, keep) if g]
    best = select(pool, pool_contrast, n_subspaces)
    sets = [pool[i] for i in best]
    con = np.asarray([pool_contrast[i] for i in best], dtype=np.float64)
    mask = np.zeros((len(sets), d), dtype=bool)
    for z, s in enumerate(sets):
        mask[z, list(s)] = True
    proba = con / con.sum() if weights == "contrast" and con.sum() > 0 else np.full(len(sets), 1.0 / len(sets))
    return {"levels": levels, "sets": sets, "contrast": con, "n_empty": np.asarray([pool_empty[i] for i in best]),
            "subspaces": mask, "proba": proba}


# ---- the data recipes of the tests ------------------------------------------------------------------------------------
def dep_data(seed, n=400, d=8):
    """float32 standard normals with x1 = x0 + 0.1 eps (a dependent pair) and x4 = sign(x2 x3) |x4| (a triple that is
    pairwise independent)."""
    rng = np.random.default_rng(seed)
    X = rng.standard_normal((n, d)).astype(np.float32)
    X[:, 1] = X[:, 0] + np.float32(0.1) * rng.standard_normal(n).astype(np.float32)
    X[:, 4] = np.sign(X[:, 2] * X[:, 3]) * np.abs(X[:, 4])
    return X


def hidden_outlier_data(seed, n=1000, d=20, n_outliers=15):
    """(X, y): dep_data's structure at [n, d]; the n_outliers rows of y = 1 are rebuilt as x1 = -x0 with 0.7 <= |x0| <= 1.5,
    inside every marginal range and far from the x1 = x0 band."""
    rng = np.random.default_rng(1000 + seed)
    X = dep_data(seed, n, d)
    rows = rng.choice(n, size=n_outliers, replace=False)
    x0 = (rng.uniform(0.7, 1.5, size=n_outliers) * rng.choice([-1.0, 1.0], size=n_outliers)).astype(np.float32)
    X[rows, 0], X[rows, 1] = x0, -x0
    y = np.zeros(n, dtype=np.int64)
    y[rows] = 1
    return X, y
