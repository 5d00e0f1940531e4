"""HiCS: the contrast of a subspace and the high-contrast-subspace search (Keller, Mueller, Boehm, ICDE 2012), the usual
baseline a learned subspace generator is measured against, next to random feature bagging (``random_subspaces``).

``subspace_contrast`` scores any list of feature sets, ``HiCS`` searches for the sets of high contrast and hands them to the
detectors of ``vgan_amd.outlier`` exactly as a trained model hands over its own (``subspaces`` / ``proba`` /
``outlier_ensemble``).  The argsort of the columns and the Monte-Carlo sweep over (subspace, draw) pairs run in
libvgan_hip.so (csrc/outlier_hics.hip); the candidate generation, the cut-off, the pruning and the draws' restatement
(``hics_slice_width``, ``hics_join``, ``hics_select``, ``hics_prune``, ``hics_draws``) are host functions that need no
device.  The definitions are the docstring of ``HiCS``; they and their numpy restatement in tests/hics_ref.py bind.
"""
import math

import numpy as np
import torch

from .ops import default_ops
from .outlier import DEFAULT_WORKSPACE_BYTES, _is_int, _is_real, _matrix_shape, build_ensemble

HICS_MAX_ROWS = 1 << 18  # VGAN_HICS_MAX_ROWS: the two n-bit maps of a draw are 64 KB of LDS
HICS_SORT_RUN = 2048  # VGAN_HICS_SORT_RUN: keys of one LDS-resident run of the column argsort
HICS_PHILOX_TAG = 0x48494353  # VGAN_HICS_PHILOX_TAG: counter word 2 of every draw ("HICS")
HICS_WAVE_GROUP = 4  # VGAN_HICS_WAVE_GROUP: draws of a workgroup when a wave owns a draw
HICS_WEIGHTS = ("contrast", "uniform")
_DRAW_BYTES = 16  # D int64, m int32, c int32 per (subspace, draw)
_MAX_BLOCKS = (1 << 31) - 1
_M32 = np.uint64(0xFFFFFFFF)
_U = np.uint64


def _philox4x32_10(c0, c1, c2, c3, k0, k1):
    """Philox4x32-10 (Salmon et al., SC'11) on uint64 arrays holding 32-bit words; returns the four output words."""
    c0, c1, c2, c3 = (np.asarray(w, dtype=np.uint64) & _M32 for w in (c0, c1, c2, c3))
    k0, k1 = _U(int(k0) & 0xFFFFFFFF), _U(int(k1) & 0xFFFFFFFF)
    for _ in range(10):
        p0, p1 = _U(0xD2511F53) * c0, _U(0xCD9E8D57) * c2
        c0, c1, c2, c3 = (p1 >> _U(32)) ^ c1 ^ k0, p1 & _M32, (p0 >> _U(32)) ^ c3 ^ k1, p0 & _M32
        k0, k1 = (k0 + _U(0x9E3779B9)) & _M32, (k1 + _U(0xBB67AE85)) & _M32
    return c0, c1, c2, c3


def check_hics_params(alpha, n_iterations, seed):
    if not _is_real(alpha) or not 0.0 < float(alpha) < 1.0:
        raise ValueError(f"alpha must be a number in (0, 1), got {alpha!r}")
    if not _is_int(n_iterations) or n_iterations < 1:
        raise ValueError(f"n_iterations must be a positive integer, got {n_iterations!r}")
    if not _is_int(seed) or not 0 <= seed < 2 ** 64:
        raise ValueError(f"seed must be an integer in [0, 2^64), got {seed!r}")
    return float(alpha), int(n_iterations), int(seed)


def check_hics_rows(n):
    if not 2 <= n <= HICS_MAX_ROWS:
        raise ValueError(f"the subspace contrast needs between 2 and HICS_MAX_ROWS = {HICS_MAX_ROWS} rows, got {n}")


def hics_slice_width(n, k, alpha):
    """w = min(n, max(1, ceil(n alpha^(1 / (k - 1))))) in float64: the rows of one conditioning slice of a k-feature
    subspace, chosen so that the k - 1 slices keep about alpha n rows when the features are independent; 0 for k < 2."""
    if k < 2:
        return 0
    return min(int(n), max(1, math.ceil(n * float(alpha) ** (1.0 / (k - 1)))))


def hics_draws(n, k, w, n_iterations, seed, stream_id):
    """The Philox draws of a k-feature subspace with stream id `stream_id`: (c int64 [M], start int64 [M, k]).  c[t] is the
    comparison position of draw t, start[t, p] the first sort position of the slice of position p; start[t, c[t]] is drawn
    and unused."""
    seed, stream_id = int(seed) & (2 ** 64 - 1), int(stream_id) & (2 ** 64 - 1)
    k0 = (seed & 0xFFFFFFFF) ^ (stream_id & 0xFFFFFFFF)
    k1 = (seed >> 32) ^ (stream_id >> 32) ^ 0x5bd1e995
    M, blocks = int(n_iterations), 1 + (int(k) + 3) // 4
    t = np.repeat(np.arange(M, dtype=np.uint64), blocks)
    q = np.tile(np.arange(blocks, dtype=np.uint64), M)
    words = np.stack(_philox4x32_10(t, q, np.full(M * blocks, HICS_PHILOX_TAG, dtype=np.uint64), np.zeros(M * blocks, dtype=np.uint64),
                                    k0, k1), axis=1).reshape(M, blocks, 4)
    c = (words[:, 0, 0] * _U(k)) >> _U(32)
    start = (words[:, 1:, :].reshape(M, -1)[:, :k] * _U(n - w + 1)) >> _U(32)
    return c.astype(np.int64), start.astype(np.int64)


def _as_sets(sets):
    return [tuple(int(f) for f in s) for s in sets]


def hics_join(sets):
    """The apriori join: every two of the given k-feature sets (ascending tuples) that share their first k - 1 features give
    their union; the result is deduplicated and sorted lexicographically.  No subset check is made."""
    groups = {}
    for s in sorted(set(_as_sets(sets))):
        groups.setdefault(s[:-1], []).append(s[-1])
    out = set()
    for head, last in groups.items():
        for i in range(len(last)):
            for j in range(i + 1, len(last)):
                out.add(head + (last[i], last[j]))
    return sorted(out)


def hics_select(sets, contrasts, count):
    """The positions of the `count` best sets by (contrast descending, size ascending, features ascending), best first.
    sets: a list of ascending tuples or an integer matrix [C, k]."""
    contrasts = np.asarray(contrasts, dtype=np.float64)
    if isinstance(sets, np.ndarray) and sets.ndim == 2:
        keys = tuple(sets[:, j] for j in range(sets.shape[1] - 1, -1, -1)) + (-contrasts,)
        return np.lexsort(keys)[:count].astype(np.int64)
    sets = _as_sets(sets)
    order = sorted(range(len(sets)), key=lambda i: (-contrasts[i], len(sets[i]), sets[i]))
    return np.asarray(order[:count], dtype=np.int64)


def hics_prune(sets, contrasts):
    """bool [len(sets)]: False for a set S when a given T with S a subset of T and |T| = |S| + 1 has a strictly higher
    contrast."""
    sets = _as_sets(sets)
    best = {}  # a set -> the highest contrast among the given supersets with one more feature
    for T, cT in zip(sets, contrasts):
        for i in range(len(T)):
            S = T[:i] + T[i + 1:]
            best[S] = max(best.get(S, -math.inf), float(cT))
    return np.asarray([not best.get(S, -math.inf) > float(cS) for S, cS in zip(sets, contrasts)], dtype=bool)


def random_subspaces(d, n_subspaces, seed=0, min_features=None, max_features=None):
    """Feature bagging (Lazarevic and Kumar 2005): (bool [n_subspaces, d], uniform proba).  Every subspace draws its size
    uniformly in [min_features, max_features] (default [d // 2, d - 1], at least 1) and then that many features without
    replacement, all from numpy.random.default_rng(seed)."""
    if not _is_int(d) or d < 1 or not _is_int(n_subspaces) or n_subspaces < 1:
        raise ValueError(f"d and n_subspaces must be positive integers, got {d!r} and {n_subspaces!r}")
    lo = max(1, d // 2) if min_features is None else min_features
    hi = max(lo, d - 1) if max_features is None else max_features
    if not (_is_int(lo) and _is_int(hi) and 1 <= lo <= hi <= d):
        raise ValueError(f"need 1 <= min_features <= max_features <= d, got {lo!r}, {hi!r} with d = {d}")
    rng = np.random.default_rng(seed)
    sizes = rng.integers(lo, hi + 1, size=n_subspaces)
    out = np.zeros((n_subspaces, d), dtype=bool)
    for s, size in enumerate(sizes):
        out[s, rng.choice(d, size=int(size), replace=False)] = True
    return out, np.full(n_subspaces, 1.0 / n_subspaces)


def _shape_of(X):
    shape = tuple(X.shape) if hasattr(X, "shape") else np.asarray(X).shape
    if len(shape) != 2:
        raise ValueError(f"X must be a 2-d matrix, got shape {shape}")
    return shape


class ContrastIndex:
    """The fitted state of the contrast: order and rank of every column of X (int32 [d, n] on the device), and the sweep over
    feature lists.  Built once per data set; ``HiCS.fit`` scores every level against the same index."""

    def __init__(self, X, ops=None):
        check_hics_rows(_shape_of(X)[0])
        self.ops = ops or default_ops()
        X = torch.as_tensor(np.asarray(X) if not isinstance(X, torch.Tensor) else X).to(device="cuda", dtype=torch.float32).contiguous()
        self.n, self.d = X.shape
        n_pad = 1 << (self.n - 1).bit_length()
        keys = torch.empty(self.d, n_pad, dtype=torch.int64, device=X.device)
        self.order = torch.empty(self.d, self.n, dtype=torch.int32, device=X.device)
        self.rank = torch.empty(self.d, self.n, dtype=torch.int32, device=X.device)
        self.ops.hics_argsort_columns(X, keys, self.order, self.rank)

    def contrast(self, feat, feat_off, alpha, n_iterations, seed, stream_ids, workspace_bytes=DEFAULT_WORKSPACE_BYTES,
                 return_draws=False, group=0):
        """feat: the concatenated ascending feature lists, feat_off [S + 1] their offsets.  Returns (contrast float64 [S],
        n_empty int32 [S]) and, with return_draws, (D int64, m int32, c int32), each [S, M].  group forces the draws per workgroup
        (1 or HICS_WAVE_GROUP; 0: the library chooses by n) for measurements and tests; it never changes a result."""
        feat = np.ascontiguousarray(feat, dtype=np.int32)
        feat_off = np.ascontiguousarray(feat_off, dtype=np.int64)
        S, M = len(feat_off) - 1, int(n_iterations)
        if len(feat) and (feat.min() < 0 or feat.max() >= self.d):
            raise ValueError(f"a feature index lies outside [0, {self.d})")
        if feat_off[-1] >= 2 ** 31:
            raise ValueError("the feature lists hold 2^31 entries or more")
        sizes, which = np.unique(np.diff(feat_off), return_inverse=True)
        width = np.asarray([hics_slice_width(self.n, int(k), alpha) for k in sizes], dtype=np.int32)[which]
        ids = np.asarray(stream_ids, dtype=np.uint64).view(np.int64)
        dev = self.order.device
        t_feat, t_off = torch.as_tensor(feat, device=dev), torch.as_tensor(feat_off.astype(np.int32), device=dev)
        t_width, t_ids = torch.as_tensor(width, device=dev), torch.as_tensor(ids, device=dev)
        contrast = torch.empty(S, dtype=torch.float64, device=dev)
        n_empty = torch.empty(S, dtype=torch.int32, device=dev)
        groups = -(-M // (group or 1))
        chunk = int(max(1, min(S, int(workspace_bytes) // (_DRAW_BYTES * M), _MAX_BLOCKS // groups)))
        rows = S if return_draws else chunk
        D = torch.empty(rows * M, dtype=torch.int64, device=dev)
        m = torch.empty(rows * M, dtype=torch.int32, device=dev)
        c = torch.empty(rows * M, dtype=torch.int32, device=dev)
        for s0 in range(0, S, chunk):
            cnt = min(chunk, S - s0)
            o = s0 * M if return_draws else 0
            self.ops.hics_contrast(self.order, self.rank, t_feat, t_off[s0:], t_width[s0:], t_ids[s0:], cnt, M, seed, D[o:], m[o:],
                                   c[o:], contrast[s0:], n_empty[s0:], group=group)
        out = (contrast.cpu().numpy(), n_empty.cpu().numpy())
        if return_draws:
            out += (D.view(S, M).cpu().numpy(), m.view(S, M).cpu().numpy(), c.view(S, M).cpu().numpy())
        return out


def _lists_of(subspaces):
    m = np.asarray(subspaces)
    if m.ndim == 1:
        m = m[None, :]
    if m.ndim != 2 or m.shape[0] < 1 or m.shape[1] < 1:
        raise ValueError(f"subspaces must be a non-empty [S, d] boolean matrix, got shape {m.shape}")
    m = m.astype(bool)
    s, f = np.nonzero(m)  # row-major: the features of a row ascending
    return m.shape[1], f.astype(np.int32), np.concatenate([[0], np.cumsum(m.sum(axis=1))]).astype(np.int64)


def subspace_contrast(X, subspaces, alpha=0.1, n_iterations=50, seed=0, stream_ids=None, workspace_bytes=DEFAULT_WORKSPACE_BYTES,
                      return_draws=False):
    """The HiCS contrast (the ``HiCS`` docstring) of every row of the boolean matrix `subspaces` [S, d] on the rows of X:
    float64 [S].  stream_ids (default: the row position in `subspaces`) name the Philox stream of each subspace, so a
    subspace scored alone with its entry gets the bits it gets among others.  workspace_bytes limits the draws kept per
    launch and never changes a result.  With return_draws also D int64 [S, M], m int32 [S, M] and the comparison positions c
    int32 [S, M] (a subspace with fewer than two features: D = m = 0, c = -1)."""
    alpha, n_iterations, seed = check_hics_params(alpha, n_iterations, seed)
    d, feat, feat_off = _lists_of(subspaces)
    _matrix_shape(X, d)
    S = len(feat_off) - 1
    ids = np.arange(S, dtype=np.uint64) if stream_ids is None else np.asarray([int(i) & (2 ** 64 - 1) for i in stream_ids], dtype=np.uint64)
    if len(ids) != S:
        raise ValueError(f"stream_ids has {len(ids)} entries for {S} subspaces")
    out = ContrastIndex(X).contrast(feat, feat_off, alpha, n_iterations, seed, ids, workspace_bytes, return_draws)
    return (out[0],) + out[2:] if return_draws else out[0]


class HiCS:
    """High-contrast subspaces (Keller, Mueller, Boehm: "HiCS: High Contrast Subspaces for Density-Based Outlier Ranking",
    ICDE 2012) with the Kolmogorov-Smirnov deviation.  ``fit(X)`` searches; ``subspaces`` (bool [S, d]), ``proba``,
    ``contrast_`` (float64 [S]), ``n_empty_`` (int [S]) and ``levels_`` hold the result, and ``outlier_ensemble`` builds any
    detector of ``vgan_amd.outlier`` on them, as the models' ``outlier_ensemble`` does on theirs.

    X is cast to float32 [n, d], 2 <= n <= HICS_MAX_ROWS = 2^18 (the two n-bit maps of a draw are 64 KB of LDS); more rows
    raise ValueError.  NaN input leaves the results unspecified and neither faults nor hangs.

    Order and rank.  order[f, r] is the row at position r of the stable ascending sort of column f, -0.0 taken as +0.0,
    ties to the lower row index; rank[f, order[f, r]] = r.

    Subspace.  Its features in ascending order f_0 < ... < f_{k-1}.  With k < 2 the contrast is exactly 0 and no draw is made.

    Slice width.  w = min(n, max(1, math.ceil(n * alpha ** (1.0 / (k - 1))))), evaluated on the host in float64.

    Draw t (t = 0 .. M - 1, M = n_iterations) of a subspace with stream id `id` uses Philox4x32-10 words with the key k0 =
    lo32(seed) ^ lo32(id), k1 = hi32(seed) ^ hi32(id) ^ 0x5bd1e995 and the counter (t, q, 0x48494353, 0).  Word 0 of block
    q = 0 chooses the comparison position c = (w0 * k) >> 32.  The start of position p is word p & 3 of block q = 1 +
    (p >> 2): start_p = (word * (n - w + 1)) >> 32; the word of p = c is drawn and unused.  slice_p = {order[f_p, start_p +
    j] : 0 <= j < w}; the conditional set C is the intersection of the slices of all p != c, m = |C|.

    Deviation.  cnt(r) = #{rows of C with rank[f_c, .] < r}; D_t = max over r = 1 .. n of |cnt(r) n - r m| in 64-bit
    integers; dev_t = float64(D_t) / float64(n m), and 0 when m = 0 (such draws are counted in ``n_empty_``).  This is the
    two-sample Kolmogorov-Smirnov statistic between the conditional and the full sample of f_c taken on sort positions, so
    ties need no rule.  Welch's t-test deviation, the paper's other choice, is not built.

    Contrast.  (dev_0 + dev_1 + ... + dev_{M-1}) / M, summed in float64 in ascending t.

    Search.  (1) Level 2 is all pairs in lexicographic order.  (2) At level k the candidates are sorted lexicographically and
    candidate j gets the stream id (k << 32) | j.  (3) The candidate_cutoff best by (contrast descending, features
    ascending) are kept.  (4) The next level is the apriori join of the kept sets: two sets that share their first k - 1
    features give their union, deduplicated; no subset check is made.  (5) The search stops when there is no candidate or k
    exceeds max_dim (None: d).  (6) The kept sets of all levels are pooled.  (7) A set S is dropped if a kept T containing S
    with |T| = |S| + 1 has a strictly higher contrast.  (8) The n_subspaces best by (contrast descending, size ascending,
    features ascending) are returned, in that order.

    ``proba`` is contrast / sum(contrast) with weights="contrast" (uniform if that sum is 0) and uniform with
    weights="uniform".  ``levels_`` is a list of dicts, one per level: "k", "candidates" (int32 [C, k]), "contrast" (float64
    [C]), "n_empty" (int32 [C]) and "kept" (bool [C]).

    The defaults are ELKI's as remembered; neither ELKI nor the authors' code was at hand, so nothing is pinned to them:
    this docstring and tests/hics_ref.py bind.  Every number is an integer until the one division per draw, so contrasts are
    bit-identical from run to run and for every workspace_bytes."""

    subspaces = proba = contrast_ = n_empty_ = levels_ = None

    def __init__(self, alpha=0.1, n_iterations=50, candidate_cutoff=100, n_subspaces=100, max_dim=None, seed=0, weights="contrast",
                 workspace_bytes=DEFAULT_WORKSPACE_BYTES):
        self.alpha, self.n_iterations, self.seed = check_hics_params(alpha, n_iterations, seed)
        for name, v in (("candidate_cutoff", candidate_cutoff), ("n_subspaces", n_subspaces)):
            if not _is_int(v) or v < 1:
                raise ValueError(f"{name} must be a positive integer, got {v!r}")
        if max_dim is not None and (not _is_int(max_dim) or max_dim < 2):
            raise ValueError(f"max_dim must be None or an integer >= 2, got {max_dim!r}")
        if weights not in HICS_WEIGHTS:
            raise ValueError(f"weights must be one of {HICS_WEIGHTS}, got {weights!r}")
        self.candidate_cutoff, self.n_subspaces, self.max_dim = int(candidate_cutoff), int(n_subspaces), max_dim
        self.weights, self.workspace_bytes = weights, int(workspace_bytes)

    def fit(self, X):
        shape = _shape_of(X)
        check_hics_rows(shape[0])
        d = shape[1]
        if d < 2:
            raise ValueError(f"the search needs at least 2 features, got {d}")
        index = ContrastIndex(X)
        max_dim = d if self.max_dim is None else min(self.max_dim, d)
        a, b = np.triu_indices(d, 1)
        cands = np.stack([a, b], axis=1).astype(np.int32)
        levels, pool, pool_contrast, pool_empty = [], [], [], []
        k = 2
        while len(cands) and k <= max_dim:
            C = len(cands)
            ids = (np.uint64(k) << np.uint64(32)) | np.arange(C, dtype=np.uint64)
            contrast, n_empty = index.contrast(cands.reshape(-1), np.arange(C + 1, dtype=np.int64) * k, self.alpha, self.n_iterations,
                                               self.seed, ids, self.workspace_bytes)
            best = hics_select(cands, contrast, self.candidate_cutoff)
            kept = np.zeros(C, dtype=bool)
            kept[best] = True
            levels.append({"k": k, "candidates": cands, "contrast": contrast, "n_empty": n_empty, "kept": kept})
            for i in np.flatnonzero(kept):
                pool.append(tuple(int(f) for f in cands[i]))
                pool_contrast.append(float(contrast[i]))
                pool_empty.append(int(n_empty[i]))
            k += 1
            nxt = hics_join([tuple(row) for row in cands[kept]])
            cands = np.asarray(nxt, dtype=np.int32).reshape(len(nxt), k)
        keep = hics_prune(pool, pool_contrast)
        pool = [s for s, g in zip(pool, keep) if g]
        pool_contrast = np.asarray(pool_contrast, dtype=np.float64)[keep]
        pool_empty = np.asarray(pool_empty, dtype=np.int64)[keep]
        best = hics_select(pool, pool_contrast, self.n_subspaces)
        self.subspaces = np.zeros((len(best), d), dtype=bool)
        for z, i in enumerate(best):
            self.subspaces[z, list(pool[i])] = True
        self.contrast_, self.n_empty_, self.levels_ = pool_contrast[best], pool_empty[best], levels
        total = self.contrast_.sum()
        uniform = np.full(len(best), 1.0 / len(best))
        self.proba = self.contrast_ / total if self.weights == "contrast" and total > 0.0 else uniform
        return self

    def outlier_ensemble(self, method="knn", n_neighbors=5, X=None, **kw):
        """A detector of ``vgan_amd.outlier`` on the found subspaces, weighted by ``proba``: the `method` strings and keywords
        are those of the models' ``outlier_ensemble`` (e.g. method="iforest", n_dims=3 for oblique isolation-forest cuts);
        fitted on X when X is given."""
        if self.subspaces is None:
            raise RuntimeError("HiCS is not fitted: call fit(X) first")
        ens = build_ensemble(self.subspaces, self.proba, method=method, n_neighbors=n_neighbors, **kw)
        return ens if X is None else ens.fit(X)
