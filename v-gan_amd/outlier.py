"""Outlier scoring over generated subspaces: a pyod-style ensemble of kNN / LOF / KDE detectors, one per subspace of a
model, combined with the subspace probabilities (``model.subspaces`` / ``model.proba``).

For subspace s with feature set F_s and weight p_s, dist_s(x, y) = sqrt(sum_{f in F_s} (x_f - y_f)^2) on the raw features.
Neighbour lists hold the k reference rows nearest in that distance, ordered by (distance, reference index).  ``fit``
scores the reference set with each row's own index excluded (sklearn's ``kneighbors(X=None)``); ``decision_function``
excludes nothing.  kNN scores are the k-th ("largest"), mean or median distance; LOF is sklearn's LocalOutlierFactor
(positive, larger is more outlying).  KDE is the Gaussian kernel density with bandwidth h_s (d_s = |F_s|):

    log p_s(q) = logsumexp_r(-dist_s(q, r)^2 / (2 h_s^2)) - log N - d_s log h_s - (d_s / 2) log(2 pi),  score_s = -log p_s

kNN, LOF and ``kneighbors`` also take the Manhattan, Chebyshev, Minkowski (p in (0, 8]) and cosine distances (``metric`` /
``p`` of ``SubspaceEnsemble``, whose docstring has the definitions): the Minkowski family on a vector-ALU producer of its own
(csrc/outlier_metric.hpp), the cosine distance as the Gram engine on unit rows; the scores after the lists are metric free.
The density below is over the N reference rows r, which is sklearn's ``KernelDensity(bandwidth=h_s).score_samples`` negated (pyod's KDE);
``fit`` leaves row q's own index out (N = n - 1), ``decision_function`` nothing (N = n).  The ensemble score is
sum_s p_s score_s in float64, subspaces in order.

Normalisation and combination (opt-in; the defaults keep the raw weighted sum).  Only LOF is scale free: a kNN distance
grows like sqrt(d_s) and a KDE -log p linearly with d_s, so raw scores let the widest subspaces decide.  With
``normalize`` set, ``fit`` takes from the n fit-time scores x of every subspace (float32, as float64) a centre c_s and a
scale w_s, both float64 (``score_center_`` / ``score_scale_``, [S] in the given subspace order):

    "zscore"  mean; population standard deviation sqrt(mean((x - c_s)^2))                  (sklearn's StandardScaler)
    "robust"  numpy.median(x); median(abs(x - c_s)) / 0.6744897501960817   (scipy's median_abs_deviation, scale="normal")
    "minmax"  minimum; maximum - minimum                                                     (sklearn's MinMaxScaler)

A scale that would be 0 (constant scores) is 1.  t_s(x) = (float64(x) - c_s) / w_s, or float64(x) without ``normalize``;
``combination`` "sum" gives sum_s p_s t_s(score_s), subspaces in order, "max" gives max_s t_s(score_s) (pyod's
maximization; proba is not used).  ``decision_function`` applies the statistics stored by ``fit`` to the scores of the new
rows (pyod's standardizer(train, test)) and computes none of its own; the per-subspace scores handed out stay the raw
detector scores.  Non-finite scores (NaN input) leave the statistics unspecified; they neither fault nor hang.
``contamination`` sets ``threshold_`` = numpy.percentile(decision_scores_, 100 (1 - contamination)), ``labels_`` =
(decision_scores_ > threshold_), and serves ``predict`` / ``predict_proba`` (pyod's rules, host code on the [n] vector).

All distance, selection and scoring work runs in libvgan_hip.so (csrc/outlier.hip); this module plans the work on the
host (feature lists, chunks of subspaces under a workspace limit) and owns the device buffers.  The statistics, the
transform and the combination run there too (csrc/outlier_norm.hip), on the score matrix the detectors left on the device.

``SubspaceABOD`` is the angle-based detector (FastABOD): it takes the neighbour lists above and scores a row by the variance
of the distance-weighted angles under which it sees pairs of its neighbours (csrc/outlier_abod.hip); its contract (usable
neighbours, the two-pass variance, the floor that degenerate rows take) is that class's docstring.

``SubspaceCOF`` is the connectivity-based detector (COF): on the same neighbour lists it replaces the density of LOF by the
average chaining distance, the cost of walking from a row through its k neighbours along nearest-set edges
(csrc/outlier_cof.hip); its contract (pairwise distances, the two chains, the weights, the ratio against the fitted rows,
the zero-denominator rules and the ceiling degenerate rows take) is that class's docstring.

``SubspaceSOD`` is the subspace outlier degree (SOD), the project's own idea one level down: each row chooses the features
in which it is judged.  From the same neighbour lists it takes, per row, the fitted rows that share the most nearest
neighbours with it (a sparse integer product over the reverse lists, counted in LDS), keeps the features of the subspace in
which that reference set varies little, and measures the row's distance to the reference mean in those features only
(csrc/outlier_sod.hip).  Its contract (lists, shared neighbours and the order among equals, the moments and their
rounding, the summation shape, the threshold, the two score forms, r = 0, new rows, determinism, what is not built) is
that class's docstring.

``SubspaceCBLOF`` is the cluster-based detector: k-means over all subspaces at once and the cluster-based local outlier
factor on its clusters (csrc/cluster.hip); its contract (initial centres, the E and M steps and their precision, the stop
rules, the final float64 assignment, large and small clusters, the score, determinism) is that class's docstring.

``SubspaceECOD`` is the empirical-CDF detector (ECOD): per-feature tail probabilities from one sort per feature, summed
over the features of each subspace as one dense float64 product with the 0/1 subspace mask (csrc/outlier_ecod.hip); it
has no hyper-parameter and never sweeps pairs of rows.  Its contract (tail counts, the fit and the single-row-append
rule, the skew sign, the two aggregates) is that class's docstring.

``SubspaceIForest`` is the isolation forest: random trees per subspace on a few hundred sampled rows each, built and walked
on the device (csrc/outlier_iforest.hip), with path lengths summed in fixed point so that every result is free of any
order; it never sweeps pairs of rows either.  Its contract (samples, node numbering, the leaf rule, the draws, the
threshold, the fixed-point path length, the score) is that class's docstring.

``SubspaceRSHash`` is RS-Hash: per subspace a hundred randomly shifted grids over a few of its non-constant features, each
holding the counts of a few hundred sampled rows per cell, counted and looked up on the device (csrc/outlier_rshash.hip);
linear in the rows, yet a cell is a joint statement about several features.  Its contract (candidates, the host draws,
samples, digits and keys, the plus-one rule, the fixed-point log counts, the score) is that class's docstring.

``SubspaceINNE`` is the nearest-neighbour isolation ensemble (iNNE): per subspace a few hundred estimators of a handful of
sampled rows each, a hypersphere around every sampled row that reaches its nearest other one, and per query row the
isolation ratio of the smallest sphere that covers it (csrc/outlier_inne.hip); local and rotation free where the isolation
forest is global and axis-aligned, and scale free in [0, 1].  Its contract (the sample and its order, the squared distance
and its rounding, radius and nearest centre, the two ratios, the covering rule, the score) is that class's docstring.

``SubspaceMahalanobis`` is the covariance-based detector: a float64 mean and shrunk covariance per subspace, classical or by
deterministic concentration steps (MCD), and the squared Mahalanobis distance as a triangular float64 product on the
matrix unit (csrc/outlier_maha.hip); n d_s^2 per subspace.  Its contract (support, location, covariance, shrinkage and the
OAS rule, the score, the degenerate cases, the C-steps, determinism) is that class's docstring.

``SubspacePCA`` is the principal-component detector: the moments of ``SubspaceMahalanobis``, the eigenpairs of every
subspace's covariance or correlation matrix by a batched fixed-order Jacobi solver, and the weighted squared projections
on the major, the minor or all components as a full float64 product on the matrix unit (csrc/outlier_pca.hip).  Its
contract (scaling, order and sign of the eigenpairs, the component count and set, the weights, the degenerate cases,
determinism) is that class's docstring.

``SubspaceGMM`` is the probabilistic mixture: EM for a few full-covariance Gaussians per subspace, the stop rule decided per
subspace on the device, and the negative log-likelihood as the score (csrc/outlier_gmm.hip, with the factor of
csrc/outlier_maha.hip on the (subspace, component) pairs and the k-means start of csrc/cluster.hip); n C d_s^2 per
iteration.  Its contract (the start, the M and E steps, the loop, freezing, failures, determinism) is that class's docstring.

``SubspaceOCSVM`` is the boundary method: the one-class SVM with the RBF kernel, whose fitted state is a sparse subset of the
rows.  The n x n float32 kernel matrix of every subspace comes from the distance engines, the dual is solved by SMO with one
workgroup per subspace and a stop rule per subspace on the device, and the score is rho minus the kernel sum over the
fitted rows in fixed point (csrc/outlier_ocsvm.hip); n^2 d_s for the matrix, n per SMO step.  Its contract (gamma, the
matrix, the start, the step and its arithmetic, rho, the score, determinism, what is not built) is that class's docstring.

``SubspaceSOS`` is the affinity-based detector (stochastic outlier selection): every fitted row gets a kernel width of its
own, found by the perplexity search of t-SNE on its row of the n x n float32 dissimilarity matrix (the matrix plumbing of
``SubspaceOCSVM``), and a row's score is the probability that no fitted row picks it as a neighbour, a product over the
fitted rows formed as a sum of logarithms in fixed point (csrc/outlier_sos.hip); n^2 d_s for the matrix, about 30 n^2 float64
exponentials for the search.  Its contract (the matrix, the shift, degenerate rows, the search, the two score forms,
determinism) is that class's docstring.

``SubspaceLOCI`` is the proximity detector without a k (the local correlation integral): on the matrix of ``SubspaceSOS`` and a
grid of radii under its largest entry, a row's neighbour count within alpha r against the counts of the rows within r of it, as
two integer sweeps of the matrix, and the largest deviation in local standard deviations as the score (csrc/outlier_loci.hip);
n^2 d_s for the matrix, n^2 R predicated integer additions for the sums.  It sees groups of more than MAX_NEIGHBORS close
anomalous rows, which every neighbour-list detector scores as inliers of their own group.  Its contract (the matrix, the
radii, counts and sums, the score and the best radius, the new-row rule, determinism, what is not built) is that class's
docstring.

``SubspaceDIF`` is the learned-representation detector without the learning (deep isolation forest): per subspace an ensemble
of randomly initialised, never trained MLPs, regenerated from the seed by a counter-based generator, maps the min-max scaled
rows to small representations in one fused fp32 matrix-unit forward that keeps every activation in LDS
(csrc/outlier_dif.hip), and the trees of ``SubspaceIForest`` are grown on every representation and pooled per subspace
(the block entries of csrc/outlier_iforest.hip).  Its contract (scaling, the nets and their weights, the representation and
its precision, the trees and the pooled score, determinism, what is not built) is that class's docstring.

``SubspaceAutoEncoder`` is the detector that learns: one small MLP per subspace trained by Adam on mini-batches to reconstruct the
standardised rows through a bottleneck, one workgroup owning one net for many optimiser steps per launch, the reconstruction
distance as the score (csrc/outlier_ae.hip).  Its contract (scaling, the net and its initial draw, the batches, the float32
operation sequence of a step, the score, determinism, what is not built) is that class's docstring.

``SubspaceDeepSVDD`` is the deep one-class detector: one small encoder without bias per subspace trained by the same loop to map
the standardised rows onto one centre, the squared distance of a row's image from the centre as the score
(csrc/outlier_svdd.hip, on the layer routines of csrc/outlier_mlp.hpp that the autoencoder uses with a bias).  Its contract
(the net, the centre and its center_eps rule, the step, the score, the collapse of bounded activations, what is not built)
is that class's docstring.

``SubspaceHBOS`` and ``SubspaceLODA`` are the histogram detectors, linear in n: equal-width histograms (numpy.linspace's
edges, numpy.histogram's counts, exact integer sums) of every feature (HBOS: -log2 densities summed over a subspace's
features, the dense float64 product of ``SubspaceECOD``) or of sparse random projections of every subspace (LODA: the mean
-log bin probability; the projected values are never stored) (csrc/outlier_hist.hip).  Their contracts (range, edges,
bins, the out-of-range rule, the host draw of the projections and its rounding) are those classes' docstrings.

The classes differ in their scores only.  The constructor tail, the first touch of the device (at the first ``fit``,
never in a constructor), the head and the tail of ``fit``, ``decision_function`` and the tail above (normalize,
combination, contamination, predict) are ``_SubspaceScorer``; the neighbour search and its chunk loop are
``_NeighborScorer``.  A new detector brings its own arguments, a row-count check (``_check_fit_rows``), ``_score`` and the
extra attributes its ``fit`` publishes: the ``_SubspaceScorer`` docstring has the list.

``build_ensemble`` maps a method string to the unfitted detector; the models' ``outlier_ensemble`` and the subspace search of
``vgan_amd.hics`` (HiCS, a source of subspaces beside the trained generator) both go through it.
"""
import inspect
import math
import os

import numpy as np
import torch

from .ops import default_ops

MAX_NEIGHBORS = 32  # VGAN_OUTLIER_MAX_K
# Subspaces with at least this many features go through the fp32 MFMA Gram engine, smaller ones through the exact
# difference engine (the two meet at 32 on the MI355X).
GRAM_MIN_DIMS = 32
ENGINE_ENV = "VGAN_OUTLIER_ENGINE"  # "exact" / "gram" forces one engine for every subspace
ENGINES = {"exact": 0, "gram": 1}
KNN_METHODS = {"largest": 0, "mean": 1, "median": 2}
_LRD, _LOF = 3, 4
KDE_MAX_ROWS = (1 << 23) - 1  # VGAN_OUTLIER_KDE_MAX_ROWS: the fixed-point density sum stays below 2^63
BANDWIDTH_RULES = ("scott", "silverman")
DEFAULT_WORKSPACE_BYTES = 1 << 30
_TARGET_BLOCKS = 512  # two workgroups per CU of the 256 on an MI355X
NORMALIZATIONS = {"zscore": 1, "robust": 2, "minmax": 3}  # VGAN_OUTLIER_NORM_*
COMBINATIONS = {"sum": 0, "max": 1}  # VGAN_OUTLIER_COMBINE_*
PROBA_METHODS = ("linear", "unify")


METRICS = {"euclidean": 0, "manhattan": 1, "chebyshev": 2, "minkowski": 3, "cosine": 4}  # VGAN_OUTLIER_METRIC_*
METRIC_ALIASES = {"l2": "euclidean", "l1": "manhattan", "cityblock": "manhattan"}
MINKOWSKI_FAMILY = ("manhattan", "chebyshev", "minkowski")  # the metrics of the vector-ALU producer (csrc/outlier_metric.hpp)
MAX_P = 8.0  # VGAN_OUTLIER_MAX_P


def _is_int(v):
    return isinstance(v, (int, np.integer)) and not isinstance(v, bool)


def _is_real(v):
    return isinstance(v, (int, float, np.integer, np.floating)) and not isinstance(v, bool)


def check_neighbors(k, least=1):
    if not (_is_int(k) and least <= int(k) <= MAX_NEIGHBORS):
        raise ValueError(f"n_neighbors must be an integer between {least} and {MAX_NEIGHBORS}, got {k!r}")
    return int(k)


def check_reference_rows(n_ref, k, exclude_self):
    need = k + 1 if exclude_self else k
    if n_ref < need:
        what = "fit needs at least n_neighbors + 1" if exclude_self else "scoring needs at least n_neighbors"
        raise ValueError(f"{what} reference rows ({need}), got {n_ref}")


def check_metric(metric, p=None):
    """(name, p): the canonical metric name and the Minkowski exponent (None for every other metric).  Aliases: "l2" is
    "euclidean", "l1" and "cityblock" are "manhattan".  p is a finite float in (0, 8] and is given with "minkowski" only (the
    default there is 2, as in sklearn); "minkowski" with p == 1 IS "manhattan" and with p == 2 "euclidean"."""
    if not isinstance(metric, str) or METRIC_ALIASES.get(metric, metric) not in METRICS:
        raise ValueError(f"metric must be one of {sorted(METRICS) + sorted(METRIC_ALIASES)}, got {metric!r}")
    metric = METRIC_ALIASES.get(metric, metric)
    if metric != "minkowski":
        if p is not None:
            raise ValueError(f"p is the exponent of metric='minkowski'; got p={p!r} with metric={metric!r}")
        return metric, None
    p = 2.0 if p is None else p
    if not _is_real(p) or not (np.isfinite(p) and 0.0 < float(p) <= MAX_P):
        raise ValueError(f"p must be a finite float in (0, {MAX_P:g}], got {p!r}")
    p = float(p)
    if p == 1.0:
        return "manhattan", None
    if p == 2.0:
        return "euclidean", None
    return metric, p


def check_bandwidth(bandwidth):
    """A positive finite float, or the name of one of sklearn's rules ("scott", "silverman")."""
    if isinstance(bandwidth, str):
        if bandwidth not in BANDWIDTH_RULES:
            raise ValueError(f"bandwidth must be a positive float, 'scott' or 'silverman', got {bandwidth!r}")
        return bandwidth
    if not _is_real(bandwidth):
        raise ValueError(f"bandwidth must be a positive float, 'scott' or 'silverman', got {bandwidth!r}")
    if not (np.isfinite(bandwidth) and bandwidth > 0):
        raise ValueError(f"bandwidth must be positive and finite, got {bandwidth!r}")
    return float(bandwidth)


def resolve_bandwidth(bandwidth, n, dims):
    """float64 [S]: h_s per subspace of dims (sizes d_s) for a reference set of n rows; sklearn's KernelDensity rules
    scott n^(-1 / (d_s + 4)) and silverman (n (d_s + 2) / 4)^(-1 / (d_s + 4))."""
    bandwidth = check_bandwidth(bandwidth)
    d = np.asarray(dims, dtype=np.float64)
    if bandwidth == "scott":
        return float(n) ** (-1.0 / (d + 4))
    if bandwidth == "silverman":
        return (float(n) * (d + 2) / 4.0) ** (-1.0 / (d + 4))
    return np.full(d.shape, bandwidth, dtype=np.float64)


def check_kde_rows(n_ref, exclude_self):
    """fit (self excluded) needs 2 reference rows, decision_function 1; the fixed-point sum caps them at KDE_MAX_ROWS."""
    need = 2 if exclude_self else 1
    if n_ref < need:
        what = "fit needs at least 2" if exclude_self else "scoring needs at least 1"
        raise ValueError(f"KDE {what} reference rows, got {n_ref}")
    if n_ref > KDE_MAX_ROWS:
        raise ValueError(f"KDE takes at most {KDE_MAX_ROWS} reference rows, got {n_ref}")


def check_normalize(normalize):
    if normalize is not None and not (isinstance(normalize, str) and normalize in NORMALIZATIONS):
        raise ValueError(f"normalize must be None, 'zscore', 'robust' or 'minmax', got {normalize!r}")
    return normalize


def check_combination(combination):
    if not (isinstance(combination, str) and combination in COMBINATIONS):
        raise ValueError(f"combination must be 'sum' or 'max', got {combination!r}")
    return combination


def check_contamination(contamination):
    """A float in (0, 0.5] (pyod's range)."""
    if not _is_real(contamination):
        raise ValueError(f"contamination must be a float in (0, 0.5], got {contamination!r}")
    if not 0.0 < float(contamination) <= 0.5:  # False for nan
        raise ValueError(f"contamination must be in (0, 0.5], got {contamination!r}")
    return float(contamination)


def decision_threshold(scores, contamination):
    """pyod's threshold_: numpy.percentile(scores, 100 (1 - contamination)); labels are scores > threshold."""
    contamination = check_contamination(contamination)
    return float(np.percentile(np.asarray(scores, dtype=np.float64), 100.0 * (1.0 - contamination)))


def outlier_probability(train_scores, scores, method="linear"):
    """float64 [n, 2]: column 1 the outlier probability of scores, column 0 its complement (pyod's predict_proba).
    "linear": (s - min) / (max - min) over train_scores; "unify": erf((s - mean) / (std sqrt(2))), population std; both
    clipped to [0, 1].  A zero range or std (constant train_scores) counts as 1, the scalers' rule for a constant column."""
    if method not in PROBA_METHODS:
        raise ValueError(f"method must be 'linear' or 'unify', got {method!r}")
    train = np.asarray(train_scores, dtype=np.float64).reshape(-1)
    s = np.asarray(scores, dtype=np.float64).reshape(-1)
    if method == "linear":
        lo, width = train.min(), train.max() - train.min()
        p = (s - lo) / (width if width != 0.0 else 1.0)
    else:
        sigma = train.std()
        z = (s - train.mean()) / ((sigma if sigma != 0.0 else 1.0) * math.sqrt(2.0))
        p = torch.erf(torch.as_tensor(z, dtype=torch.float64)).numpy()
    p = np.clip(p, 0.0, 1.0)
    return np.stack([1.0 - p, p], axis=1)


def _round4(v):
    return (np.asarray(v, dtype=np.int64) + 3) // 4 * 4


class SubspacePlan:
    """Host plan of a subspace set: the subspaces in processing order (exact-engine ones first, each group in the given
    order), their concatenated feature lists, feature offsets and packed column offsets, and chunking."""

    def __init__(self, subspaces, engine="auto", gram_min_dims=GRAM_MIN_DIMS):
        m = np.asarray(subspaces)
        if m.ndim == 1:
            m = m[None, :]
        if m.ndim != 2 or m.shape[0] < 1 or m.shape[1] < 1:
            raise ValueError(f"subspaces must be a non-empty [S, d] boolean matrix, got shape {m.shape}")
        m = m.astype(bool)
        dims = m.sum(axis=1)
        if (dims == 0).any():
            raise ValueError(f"subspace {int(np.flatnonzero(dims == 0)[0])} selects no feature")
        if engine not in ("auto", "exact", "gram"):
            raise ValueError(f"engine must be 'auto', 'exact' or 'gram', got {engine!r}")
        gram = dims >= gram_min_dims if engine == "auto" else np.full(len(dims), engine == "gram")
        self.order = np.argsort(gram, kind="stable").astype(np.int32)  # processing position -> subspace index
        self.given = np.argsort(self.order)  # given subspace index -> processing position
        self.gram = gram[self.order]
        self.dims = dims[self.order].astype(np.int64)
        self.d = m.shape[1]
        self.feat = np.concatenate([np.flatnonzero(m[s]) for s in self.order]).astype(np.int32)
        self.feat_off = np.concatenate([[0], np.cumsum(self.dims)]).astype(np.int32)
        self.col_off = np.concatenate([[0], np.cumsum(_round4(self.dims))]).astype(np.int64)

    @property
    def count(self):
        return len(self.order)

    def chunks(self, rows, limit_bytes, extra_bytes=0, max_count=None):
        """[(first, count, gram)]: consecutive runs of the processing order, one engine each, whose packed blocks of `rows`
        rows (values and norms, float32) plus extra_bytes a subspace fit in limit_bytes; a subspace that alone exceeds it
        forms a chunk of its own.  max_count: the most subspaces of a chunk (None: no limit)."""
        out, first = [], 0
        widths = _round4(self.dims)
        while first < self.count:
            end, used = first, 0
            while end < self.count and self.gram[end] == self.gram[first] and (max_count is None or end - first < max_count):
                need = int(extra_bytes) + int(rows) * (int(widths[end]) + 1) * 4
                if end > first and used + need > limit_bytes:
                    break
                used += need
                end += 1
            out.append((first, end - first, bool(self.gram[first])))
            first = end
        return out


def _matrix_shape(X, d):
    """The shape of X, an array or a tensor on any device, after the checks every entry point makes on the host."""
    shape = tuple(X.shape) if hasattr(X, "shape") else np.asarray(X).shape
    if len(shape) != 2:
        raise ValueError(f"X must be a 2-d matrix, got shape {shape}")
    if shape[1] != d:
        raise ValueError(f"X has {shape[1]} features, the subspaces {d}")
    return shape


def _device_matrix(X, d):
    X = torch.as_tensor(np.asarray(X) if not isinstance(X, torch.Tensor) else X)
    _matrix_shape(X, d)
    return X.to(device="cuda", dtype=torch.float32).contiguous()


class _SubspaceScorer:
    """What every per-subspace detector of this module shares: the constructor tail (_configure), the device copy of the
    subspace table (_attach), the packed blocks, the head of fit (_begin_fit), the tail after the [S, n] score matrix
    (statistics, transform, combination; _publish; threshold, predict) and decision_function.

    A detector provides: an __init__ that keeps its own arguments and calls _configure (no constructor touches the
    device); _check_fit_rows(n), which raises ValueError when fit cannot work on n rows; _score(X, fitting) -> (float64
    [n] ensemble scores, float32 [S, n] per-subspace scores in the given order), both on the device, which ends in
    _combine(per, fitting); and a fit that runs X = _begin_fit(X), builds its fitted state, calls _score(..., fitting=True),
    sets whatever attributes of its own it publishes and returns _publish(scores, per)."""

    ops = None  # the library and the device tables below: set by _attach at the first fit
    _fitted = False  # set by _publish
    _stats = None  # float64 [2, S] on the device (centres, scales), set by fit when normalize is given
    _decisions = None  # (threshold_, labels_), taken from decision_scores_ on first use
    score_center_ = score_scale_ = None

    def _configure(self, subspaces, proba, engine, workspace_bytes, normalize, combination, contamination, plan_engine=None):
        """plan_engine: the one engine group of a metric that has a single producer ("exact": uncentred blocks without
        norms; "gram"); the engine argument and the environment then do not reach the plan."""
        self.normalize = check_normalize(normalize)
        self.combination = check_combination(combination)
        self.contamination = check_contamination(contamination)
        if engine == "auto" and plan_engine is None:
            engine = os.environ.get(ENGINE_ENV, "auto") or "auto"
        self.engine = engine
        self.plan = SubspacePlan(subspaces, engine=engine if plan_engine is None else plan_engine)
        self.proba = np.asarray(proba, dtype=np.float64).reshape(-1)
        if self.proba.shape[0] != self.plan.count:
            raise ValueError(f"proba has {self.proba.shape[0]} entries for {self.plan.count} subspaces")
        self.workspace_bytes = int(workspace_bytes)

    def _attach(self):
        if self.ops is not None:
            return
        self.ops = default_ops()
        dev = "cuda"
        self._table = (torch.as_tensor(self.plan.feat, device=dev), torch.as_tensor(self.plan.feat_off, device=dev),
                       torch.as_tensor(self.plan.col_off, device=dev))
        self._rows = torch.as_tensor(self.plan.order, device=dev)
        self._proba = torch.as_tensor(self.proba, device=dev)

    def _begin_fit(self, X):
        """X on the device, after the host checks of its shape and row count; its column mean goes to _center."""
        self._check_fit_rows(_matrix_shape(X, self.plan.d)[0])
        self._attach()
        X = _device_matrix(X, self.plan.d)
        self._center = torch.empty(X.shape[1], dtype=torch.float32, device=X.device)
        self.ops.col_mean(X, self._center)
        return X

    def _publish(self, scores, per):
        self.decision_scores_ = scores.cpu().numpy()
        self.per_subspace_scores_ = per.cpu().numpy()
        if self.normalize is not None:
            self.score_center_, self.score_scale_ = self._stats.cpu().numpy()
        self._decisions = None
        self._fitted = True
        return self

    def _pack(self, X, first, count, gram, centred=None):
        """(packed block, squared row norms or None) of the chunk; centred on the column mean for the Gram engine, and for
        the exact engine too when centred is True (default: Gram only)."""
        n = X.shape[0]
        cols = int(self.plan.col_off[first + count] - self.plan.col_off[first])
        packed = torch.empty(n * cols, dtype=torch.float32, device=X.device)
        sq = torch.empty(count, n, dtype=torch.float32, device=X.device) if gram else None
        centred = gram if centred is None else centred
        self.ops.outlier_pack(X, self._center if centred else None, self._table, first, count, packed, sq)
        return packed, sq

    def _configure_splits(self, splits):
        if splits is not None and (int(splits) < 1 or int(splits) > 65535):
            raise ValueError(f"splits must be between 1 and 65535, got {splits}")
        self.splits = splits

    def _splits(self, nq, nr, count, cap=64):
        """The reference-row split J of a sweep of nq query rows over nr reference rows in count subspaces: the given
        splits, or enough slices to fill the chip, at most one a 64-row tile and at most cap (None: no cap)."""
        if self.splits is not None:
            return int(self.splits)
        blocks = -(-nq // 64) * count
        J = min(-(-nr // 64), -(-_TARGET_BLOCKS // blocks))
        return int(max(1, J if cap is None else min(J, cap)))

    def _sweep(self, Xq, Xr, scores):
        """float32 [S, nq], rows in the given subspace order: per chunk of the plan the packed blocks of the query rows Xq and
        of the reference rows Xr (one pair of blocks for both when Xq is Xr), a 64-bit accumulator a (subspace, query row),
        and scores((Pq, sqq, nq, Pr, sqr, nr), first, count, (engine, J, acc, per, score rows)), which launches the sweep."""
        nr, nq = Xr.shape[0], Xq.shape[0]
        per = torch.empty(self.plan.count, nq, dtype=torch.float32, device=Xr.device)
        for first, count, gram in self.plan.chunks(nr if Xq is Xr else nr + nq, self.workspace_bytes):
            Pr, sqr = self._pack(Xr, first, count, gram)
            Pq, sqq = (Pr, sqr) if Xq is Xr else self._pack(Xq, first, count, gram)
            acc = torch.empty(count * nq, dtype=torch.int64, device=Xr.device)
            scores((Pq, sqq, nq, Pr, sqr, nr), first, count, (ENGINES["gram" if gram else "exact"], self._splits(nq, nr, count),
                                                               acc, per, self._rows[first:first + count]))
            del Pq, Pr, sqq, sqr, acc
        return per

    def _keep(self, kept, M, first):
        """Files the host copies of the chunk's matrices M [count, ...] in the list kept, under the given subspace order."""
        for z, host in enumerate(M.cpu().numpy()):
            kept[int(self.plan.order[first + z])] = host

    def _combine(self, per, fitting):
        """float64 [n]: the ensemble score of the raw per-subspace scores per [S, n]; fit takes the statistics first."""
        S, n = per.shape
        if fitting and self.normalize is not None:
            self._stats = torch.empty(2, S, dtype=torch.float64, device=per.device)
            self.ops.outlier_score_stats(per, NORMALIZATIONS[self.normalize], self._stats[0], self._stats[1])
        out = torch.empty(n, dtype=torch.float64, device=per.device)
        if self.normalize is None and self.combination == "sum":
            self.ops.outlier_combine(per, self._proba, out)
        else:
            center, scale = (None, None) if self.normalize is None else self._stats
            self.ops.outlier_combine_normalized(per, center, scale, self._proba, COMBINATIONS[self.combination], out)
        return out

    def _decide(self):
        if self._decisions is None:
            threshold = decision_threshold(self.decision_scores_, self.contamination)
            self._decisions = (threshold, (self.decision_scores_ > threshold).astype(int))
        return self._decisions

    @property
    def threshold_(self):
        """numpy.percentile(decision_scores_, 100 (1 - contamination)); taken on first use, so that a fit that never asks
        for a decision does not pay for the percentile on the host."""
        return self._decide()[0]

    @property
    def labels_(self):
        """int [n]: 1 where decision_scores_ exceeds threshold_."""
        return self._decide()[1]

    def _require_fit(self):
        if not self._fitted:
            raise RuntimeError(f"{type(self).__name__} is not fitted: call fit(X_train) first")

    def decision_function(self, X, return_per_subspace=False):
        """Ensemble scores of X against the fitted state (the reference set with nothing excluded, or the clusters),
        float64 [n]; with return_per_subspace=True also the float32 [S, n] per-subspace scores (subspaces in the given
        order)."""
        self._require_fit()
        scores, per = self._score(_device_matrix(X, self.plan.d), fitting=False)
        if return_per_subspace:
            return scores.cpu().numpy(), per.cpu().numpy()
        return scores.cpu().numpy()

    def predict(self, X):
        """int [n]: 1 where decision_function(X) exceeds threshold_ (pyod's predict)."""
        return (self.decision_function(X) > self.threshold_).astype(int)

    def predict_proba(self, X, method="linear"):
        """float64 [n, 2], column 1 the outlier probability: outlier_probability(decision_scores_, decision_function(X))."""
        if method not in PROBA_METHODS:
            raise ValueError(f"method must be 'linear' or 'unify', got {method!r}")
        self._require_fit()
        return outlier_probability(self.decision_scores_, self.decision_function(X), method)


class _NeighborScorer(_SubspaceScorer):
    """The neighbour pipeline (pack -> knn -> refine) of the detectors that score a row from its k nearest reference rows.
    A detector on top of it also calls _configure_neighbors from its __init__ and keeps the reference rows that
    _begin_fit returns in _X; _chunks is the chunk loop of whatever else sweeps the query rows over the reference rows."""

    _X = None
    metric, p = "euclidean", None  # set at construction for the detectors that take a metric (_MetricKeywords)

    def _configure_neighbors(self, n_neighbors, splits, least=1):
        self.n_neighbors = check_neighbors(n_neighbors, least)
        self._configure_splits(splits)

    def _metric_engine(self, engine):
        """The plan_engine of _configure under self.metric: None for the Euclidean distance (the engines by subspace size, as
        ever); "exact" for the Minkowski family, whose one producer reads uncentred blocks without norms; "gram" for the
        cosine distance, which is the Gram engine on unit rows at every d_s.  Either way all subspaces form one engine
        group, so no chunk breaks at d_s = 32."""
        if self.metric == "euclidean":
            return None
        if engine not in ("auto", "exact", "gram"):
            raise ValueError(f"engine must be 'auto', 'exact' or 'gram', got {engine!r}")
        if self.metric in MINKOWSKI_FAMILY:
            if engine != "auto":
                raise ValueError(f"metric {self.metric!r} has one distance producer: engine must be 'auto', got {engine!r}")
            return "exact"
        if engine == "exact":
            raise ValueError("metric 'cosine' runs on the Gram engine: engine must be 'auto' or 'gram', got 'exact'")
        return "gram"

    def _check_fit_rows(self, n):
        check_reference_rows(n, self.n_neighbors, exclude_self=True)

    def _pack_metric(self, X, first, count, gram):
        if self.metric != "cosine":
            return self._pack(X, first, count, gram)
        n = X.shape[0]
        cols = int(self.plan.col_off[first + count] - self.plan.col_off[first])
        packed = torch.empty(n * cols, dtype=torch.float32, device=X.device)
        sq = torch.empty(count, n, dtype=torch.float32, device=X.device)
        self.ops.outlier_pack_unit(X, self._table, first, count, packed, sq)
        return packed, sq

    def _blocks(self, Xq, first, count, gram):
        Pr, sqr = self._pack_metric(self._X, first, count, gram)
        Pq, sqq = (Pr, sqr) if Xq is None else self._pack_metric(Xq, first, count, gram)
        return Pq, sqq, Pr, sqr

    def _chunks(self, Xq, only=None):
        """Yields (first, count, engine, nq, Pq, sqq, Pr, sqr) per chunk of the plan: the packed blocks and squared norms
        of the nq query rows Xq and of the reference rows; Xq None is the reference set itself, whose blocks then serve as
        both.  only: a processing position, for the one chunk of that subspace alone.  The generator keeps no reference to
        the blocks: they are freed when the consumer drops them."""
        nr = self._X.shape[0]
        nq = nr if Xq is None else Xq.shape[0]
        chunks = self.plan.chunks(nr if Xq is None else nr + nq, self.workspace_bytes) if only is None else [
            (only, 1, bool(self.plan.gram[only]))]
        for first, count, gram in chunks:
            yield (first, count, ENGINES["gram" if gram else "exact"], nq, *self._blocks(Xq, first, count, gram))

    def _neighbors(self, Xq, kdist=None, only=None):
        """Yields (first, count, idx, dist) per chunk: the sorted refined lists [count, nq, k] of Xq (None: the reference
        set, self excluded).  kdist (fit only): [S, n] receives the k-th distances in processing order.  only: as for
        _chunks."""
        k, Xr = self.n_neighbors, self._X
        nr = Xr.shape[0]
        for first, count, engine, nq, Pq, sqq, Pr, sqr in self._chunks(Xq, only):
            J = self._splits(nq, nr, count)
            nbr = torch.empty(count, nq, k, dtype=torch.int32, device=Xr.device)
            part_d = part_i = None
            if J > 1:
                part_d = torch.empty(count * J * nq * k, dtype=torch.float32, device=Xr.device)
                part_i = torch.empty(count * J * nq * k, dtype=torch.int32, device=Xr.device)
            metric, p = METRICS[self.metric], 0.0 if self.p is None else self.p
            if self.metric in MINKOWSKI_FAMILY:
                self.ops.outlier_knn_metric(Pq, nq, Pr, nr, self._table, first, count, k, Xq is None, metric, p, J, nbr, part_d, part_i)
            else:  # Euclidean, or cosine as the Gram engine on unit rows
                self.ops.outlier_knn(Pq, sqq, nq, Pr, sqr, nr, self._table, first, count, k, Xq is None, engine, J, nbr, part_d, part_i)
            del Pq, Pr, sqq, sqr, part_d, part_i
            idx = torch.empty_like(nbr)
            dist = torch.empty(count, nq, k, dtype=torch.float32, device=Xr.device)
            kd = None if kdist is None else kdist[first:first + count]
            if self.metric == "euclidean":
                self.ops.outlier_refine(Xr if Xq is None else Xq, Xr, self._table, first, count, nbr, k, idx, dist, kd)
            else:
                self.ops.outlier_refine_metric(Xr if Xq is None else Xq, Xr, self._table, first, count, nbr, k, metric, p, idx, dist, kd)
            yield first, count, idx, dist

    def kneighbors(self, X=None):
        """(dist float32 [S, n, k], idx int32 [S, n, k]) per subspace: the sorted neighbour lists of X, or of the reference
        set itself with self excluded (X=None)."""
        self._require_fit()
        Xq = None if X is None else _device_matrix(X, self.plan.d)
        nq = self._X.shape[0] if Xq is None else Xq.shape[0]
        k = self.n_neighbors
        D = torch.empty(self.plan.count, nq, k, dtype=torch.float32, device=self._X.device)
        I = torch.empty(self.plan.count, nq, k, dtype=torch.int32, device=self._X.device)
        for first, count, idx, dist in self._neighbors(Xq):
            rows = self._rows[first:first + count].long()
            D[rows], I[rows] = dist, idx
        return D.cpu().numpy(), I.cpu().numpy()

    def _fill_degenerate(self, per, fitting, op):
        """Puts the fill value of each subspace into the NaN (degenerate) scores of per [S, n] with op, the detector's
        ops.outlier_*_floor / _ceiling.  Fitting, op takes the fill values (_fill, float64 [S]) and the NaN counts
        (_n_degenerate, int32 [S]) from per; otherwise it applies the stored _fill.  Both are in processing order."""
        if fitting:
            self._fill = torch.empty(self.plan.count, dtype=torch.float64, device=per.device)
            self._n_degenerate = torch.empty(self.plan.count, dtype=torch.int32, device=per.device)
            op(per, self._fill, self._n_degenerate)
        else:
            op(per, self._fill)


class _MetricKeywords(type):
    """Construction of a detector that takes ``metric=`` and ``p=``.  The two are keyword-only arguments of the call of the
    class, not of ``__init__``: the keyword list of ``SubspaceEnsemble.__init__`` is a fixed surface (callers and the
    constructor test read it through ``inspect``), and the distance is not one of the detector's own settings but what its
    neighbour search measures.  The call checks them (check_metric: ValueError), keeps the canonical (metric, p) on the new
    instance and then runs ``__init__`` with the remaining arguments, which finds them there.  ``inspect.signature`` of the
    class shows the full list (the class's ``__signature__``)."""

    def __call__(cls, *args, metric="euclidean", p=None, **kw):
        self = cls.__new__(cls)
        self.metric, self.p = check_metric(metric, p)
        self.__init__(*args, **kw)
        return self


class SubspaceEnsemble(_NeighborScorer, metaclass=_MetricKeywords):
    """kNN / LOF / KDE detector per subspace, probability-weighted sum of the scores (pyod-style: ``fit`` sets
    ``decision_scores_``, ``decision_function`` scores new rows; higher is more outlying).

    method "kde": Gaussian kernel density; bandwidth is a positive float for every subspace (default 1.0, as in pyod and
    sklearn) or "scott" / "silverman", sklearn's rules per subspace from the n rows given to ``fit`` and d_s; ``fit`` sets
    ``bandwidth_``, float64 [S] in the given subspace order.  ``fit`` scores the training set leave-one-out; pyod's
    in-sample ``decision_scores_`` (self included) are ``decision_function(X_train)``.  n_neighbors and knn_method only
    serve kNN / LOF (and ``kneighbors``); kNN / LOF ignore bandwidth.
    engine: "auto" (by subspace size, GRAM_MIN_DIMS), "exact" or "gram"; the environment variable VGAN_OUTLIER_ENGINE
    overrides "auto".  splits: reference-row split J of the neighbour search / density sum (None: chosen to fill the
    chip).  workspace_bytes: limit on the packed subspace blocks of one chunk.

    normalize: None (raw scores), "zscore", "robust" (median / MAD) or "minmax": per-subspace statistics of the fit-time
    scores, published as ``score_center_`` / ``score_scale_`` (float64 [S], given order; None without normalize) and
    applied by ``fit`` and ``decision_function`` alike.  combination: "sum" (probability-weighted) or "max" (pyod's
    maximization; proba is not used).  contamination in (0, 0.5]: after ``fit``, ``threshold_`` is that upper percentile
    of ``decision_scores_`` and ``labels_`` marks the rows above it (both taken on first use); ``predict`` /
    ``predict_proba`` follow pyod.  ``per_subspace_scores_`` and
    ``return_per_subspace`` stay the raw detector scores.  Non-finite scores leave the statistics unspecified.

    metric, p (pyod's / sklearn's arguments of KNN and LOF; keyword-only, ``SubspaceEnsemble(..., metric="euclidean",
    p=None)``: see _MetricKeywords): the distance of "knn", "lof" and ``kneighbors``.  F_s is the
    feature set of subspace s; values are the raw float32 features taken as float64.

    - "euclidean" (alias "l2") is sqrt(sum_f (x_f - y_f)^2), the default.
    - "manhattan" (aliases "l1", "cityblock") is sum_f |x_f - y_f|.
    - "chebyshev" is max_f |x_f - y_f|.
    - "minkowski" with p is (sum_f |x_f - y_f|^p)^(1/p).  p is a finite float in (0, 8] (default 2).  p == 1 is the
      Manhattan path and p == 2 the Euclidean path, bit for bit.  p < 1 is allowed and is not a metric (no triangle
      inequality; sklearn's brute force allows it too).  For p > 2, sums of p-th powers whose float32 image exceeds
      FLT_MAX compare equal in the selection (such pairs are then ranked by index); this is not guarded.
    - "cosine" is 1 - <x, y> / (|x| |y|) over F_s, not centred.  A row whose norm over F_s is exactly 0 is at distance
      exactly 1 from every row, zero rows included; scipy gives NaN there.

    For every metric the neighbour order stays the strict total order (distance, reference index) and exclude_self keeps
    its meaning; exact duplicates give distance exactly 0 under the three Minkowski-family metrics (under "cosine" up to
    the float64 rounding of 1 - cos).  The selection ranks the pairs in float32 (Minkowski family: a vector-ALU sweep over
    the uncentred blocks; cosine: the Gram engine on unit rows, d2 = 2 - 2 cos, at every d_s), the selected k pairs are
    then re-measured in float64 and re-sorted, and everything after the sorted lists (kNN scores, lrd, LOF) is metric free.
    engine with another metric: the Minkowski family has one producer, so "exact" or "gram" raise and VGAN_OUTLIER_ENGINE
    is ignored; "cosine" is always Gram, "exact" raises.  method "kde" takes the Euclidean distance only (the Gaussian
    kernel is Euclidean); p without "minkowski" raises."""

    def __init__(self, subspaces, proba, method="knn", n_neighbors=5, knn_method="largest", bandwidth=1.0, engine="auto",
                 splits=None, workspace_bytes=DEFAULT_WORKSPACE_BYTES, normalize=None, combination="sum", contamination=0.1):
        if method not in ("knn", "lof", "kde"):
            raise ValueError(f"method must be 'knn', 'lof' or 'kde', got {method!r}")
        if knn_method not in KNN_METHODS:
            raise ValueError(f"knn_method must be one of {sorted(KNN_METHODS)}, got {knn_method!r}")
        plan_engine = self._metric_engine(engine)
        if method == "kde" and self.metric != "euclidean":
            raise ValueError(f"method 'kde' takes the Euclidean distance only (the Gaussian kernel is Euclidean), got metric={self.metric!r}")
        self._configure(subspaces, proba, engine, workspace_bytes, normalize, combination, contamination, plan_engine)
        self._configure_neighbors(n_neighbors, splits)
        self.bandwidth = check_bandwidth(bandwidth) if method == "kde" else bandwidth
        self.method, self.knn_method = method, knn_method

    # ---- pipeline --------------------------------------------------------------------------------
    def _check_fit_rows(self, n):
        if self.method == "kde":
            check_kde_rows(n, exclude_self=True)
        else:
            super()._check_fit_rows(n)

    def _density(self, Xq):
        """float32 [S, nq]: -log p_s of Xq (None: the reference set, leave-one-out), rows in the given subspace order."""
        Xr = self._X
        nr = Xr.shape[0]
        per = torch.empty(self.plan.count, nr if Xq is None else Xq.shape[0], dtype=torch.float32, device=Xr.device)
        for first, count, engine, nq, Pq, sqq, Pr, sqr in self._chunks(Xq):
            pivot = torch.empty(count * nq, dtype=torch.int32, device=Xr.device)
            acc = torch.empty(count * nq, dtype=torch.int64, device=Xr.device)
            self.ops.outlier_kde(Pq, sqq, nq, Pr, sqr, nr, self._table, first, count, self._bw, Xq is None, engine,
                                 self._splits(nq, nr, count), pivot, acc, per, self._rows[first:first + count])
            del Pq, Pr, sqq, sqr
        return per

    def _score(self, Xq, fitting):
        if self.method == "kde":
            per = self._density(Xq)
            return self._combine(per, fitting), per
        k = self.n_neighbors
        nq = self._X.shape[0] if Xq is None else Xq.shape[0]
        per = torch.empty(self.plan.count, nq, dtype=torch.float32, device=self._X.device)
        for first, count, idx, dist in self._neighbors(Xq, self._kdist if (fitting and self.method == "lof") else None):
            rows = self._rows[first:first + count]
            if self.method == "knn":
                self.ops.outlier_score(idx, dist, nq, k, count, KNN_METHODS[self.knn_method], score=per, score_row=rows)
                continue
            kd, lrd = self._kdist[first:first + count], self._lrd[first:first + count]
            if fitting:
                self.ops.outlier_score(idx, dist, nq, k, count, _LRD, kdist_ref=kd, nr=nq, lrd_out=lrd)
            self.ops.outlier_score(idx, dist, nq, k, count, _LOF, score=per, score_row=rows, kdist_ref=kd, lrd_ref=lrd,
                                   nr=self._X.shape[0])
        return self._combine(per, fitting), per

    # ---- public surface --------------------------------------------------------------------------
    def fit(self, X, y=None):
        """Keeps X resident as the reference set and scores it (self excluded): decision_scores_, float64 [n]; with
        normalize also score_center_ / score_scale_; threshold_ and labels_ from contamination."""
        self._X = X = self._begin_fit(X)
        n = X.shape[0]
        if self.method == "kde":
            self.bandwidth_ = resolve_bandwidth(self.bandwidth, n, self.plan.dims[self.plan.given])
            self._bw = torch.as_tensor(self.bandwidth_[self.plan.order], device=X.device)
        elif self.method == "lof":
            self._kdist = torch.empty(self.plan.count, n, dtype=torch.float32, device=X.device)
            self._lrd = torch.empty(self.plan.count, n, dtype=torch.float64, device=X.device)
        return self._publish(*self._score(None, fitting=True))


SubspaceEnsemble.__signature__ = inspect.Signature(
    list(inspect.signature(SubspaceEnsemble.__init__).parameters.values())[1:]
    + [inspect.Parameter("metric", inspect.Parameter.KEYWORD_ONLY, default="euclidean"),
       inspect.Parameter("p", inspect.Parameter.KEYWORD_ONLY, default=None)])


# ---- angle-based scores (FastABOD) over the subspaces ----------------------------------------------------------------------
ABOD_MIN_NEIGHBORS = 2  # one pair


class SubspaceABOD(_NeighborScorer):
    """Angle-based outlier detector per subspace (Kriegel, Schubert, Zimek 2008), in its fast form over the k nearest
    neighbours (FastABOD; pyod's ``ABOD`` with its default ``method="fast"``), combined like the detectors of
    SubspaceEnsemble: ``fit`` sets ``decision_scores_``, ``decision_function`` scores new rows; higher is more outlying.

    Per subspace s (features F_s), query row q and its neighbour list N(q): the k reference rows nearest in dist_s, the
    very lists SubspaceEnsemble builds (``fit`` excludes q's own index, ``decision_function`` nothing; ties by (distance,
    index); ``kneighbors`` hands them out).  For a neighbour a, v_a = r_a[F_s] - q[F_s] in float64 from the raw float32
    values (exact) and |v_a|^2 its float64 squared norm; a is usable if |v_a|^2 > 0, and m is the number of usable
    neighbours.  Over the m (m - 1) / 2 unordered pairs of usable neighbours

        w_ab = <v_a, v_b> / (|v_a|^2 |v_b|^2),      score_s(q) = -var(w)

    with var the population variance (numpy.var), two passes (the mean, then the mean squared deviation) in float64 in a
    fixed order, stored as float32 in the [S, n] score matrix; a result below the float32 range is stored as the most
    negative finite float32, never -inf.  Scores are <= 0 and the closer to 0 the more outlying; inside one subspace they
    span many orders of magnitude, so ``normalize="robust"`` or ``"minmax"`` and ``combination="max"`` are what to
    reach for when subspaces are mixed, not a logarithm (-log var is +inf at one pair).

    This is pyod's FastABOD as its source is remembered here (``_calculate_wocs`` skips a pair when one of its points equals
    the query; ``decision_scores_`` is the negated variance); pyod was not at hand to pin it, so the definition above
    and its numpy restatement in tests/test_outlier_abod_cpu.py are what binds, not pyod.

    Degenerate rows.  m < 2 leaves no pair (a row whose neighbours all coincide with it in F_s: common in narrow
    subspaces of discrete features).  pyod returns NaN there, which would poison every sum, percentile and statistic
    downstream.  Such a row sits on a point mass and is as inlying as a row can be, so it takes the floor of its
    subspace: ``score_floor_[s]``, the smallest float32 score among the non-degenerate rows of the subspace at ``fit`` (0
    if there is none).  ``fit`` publishes ``score_floor_`` (float64 [S]) and ``n_degenerate_`` (int [S]) in the given
    subspace order; ``decision_function`` applies the stored floor to its degenerate rows and computes none of its own.
    m = 2 is not degenerate: one pair, variance 0, score 0, as in pyod.

    ``decision_function(X_train)`` is not ``decision_scores_``: there every row is its own nearest neighbour, which is
    unusable, and the other k - 1 form the pairs (the KDE remark of SubspaceEnsemble, for the same reason).

    n_neighbors: 2 .. 32 (default 10, pyod's).  engine, splits, workspace_bytes: as for SubspaceEnsemble.  normalize,
    combination, contamination, ``threshold_``, ``labels_``, ``predict``, ``predict_proba``, return_per_subspace: the
    shared tail; ``per_subspace_scores_`` are the raw scores with the floor applied.  Given the same neighbour lists the
    scores are bit-identical from run to run, and the lists do not depend on splits or workspace_bytes.  The scores run
    in libvgan_hip.so (csrc/outlier_abod.hip)."""

    def __init__(self, subspaces, proba, n_neighbors=10, engine="auto", splits=None, workspace_bytes=DEFAULT_WORKSPACE_BYTES,
                 normalize=None, combination="sum", contamination=0.1):
        self._configure(subspaces, proba, engine, workspace_bytes, normalize, combination, contamination)
        self._configure_neighbors(n_neighbors, splits, least=ABOD_MIN_NEIGHBORS)

    def _score(self, Xq, fitting):
        """(ensemble scores float64 [n], per float32 [S, n] with the floor applied), both on the device."""
        k, dev = self.n_neighbors, self._X.device
        nq = self._X.shape[0] if Xq is None else Xq.shape[0]
        per = torch.empty(self.plan.count, nq, dtype=torch.float32, device=dev)
        for first, count, idx, _ in self._neighbors(Xq):
            self.ops.outlier_abod(self._X if Xq is None else Xq, self._X, self._table, first, count, idx, k, per,
                                  self._rows[first:first + count])
        self._fill_degenerate(per, fitting, self.ops.outlier_abod_floor)
        return self._combine(per, fitting), per

    def fit(self, X, y=None):
        """Keeps X resident as the reference set and scores it (self excluded): decision_scores_ (float64 [n]),
        per_subspace_scores_, score_floor_, n_degenerate_; with normalize also score_center_ / score_scale_."""
        self._X = self._begin_fit(X)
        scores, per = self._score(None, fitting=True)
        self.score_floor_ = self._fill.cpu().numpy()
        self.n_degenerate_ = self._n_degenerate.cpu().numpy().astype(np.int64)
        return self._publish(scores, per)


# ---- connectivity-based scores (COF) over the subspaces ------------------------------------------------------------------------
COF_CHAINS = {"sbn": 0, "rank": 1}  # VGAN_OUTLIER_COF_CHAIN_*


class SubspaceCOF(_NeighborScorer):
    """Connectivity-based outlier factor per subspace (COF: Tang, Chen, Fu, Cheung 2002; pyod's ``COF``), combined like
    the detectors of SubspaceEnsemble: ``fit`` sets ``decision_scores_``, ``decision_function`` scores new rows; higher is
    more outlying.  Where kNN and LOF read the radius of a neighbourhood, COF reads the cost of walking through it: a row
    just off a thin, sparse structure (a line, a curve, a strongly correlated pair of features) looks to LOF like any row
    of that structure, while its chain has to start with one long edge.

    Per subspace s (features F_s), query row q and its refined neighbour list o_1 .. o_k: the very lists SubspaceEnsemble
    and SubspaceABOD build (``fit`` excludes q's own index, ``decision_function`` nothing; ties by (float32 distance,
    index); list position 1 is the nearest; ``kneighbors`` hands them out).  Let o_0 = q.

    Pairwise distances.  d2(a, b) = sum_{f in F_s} (x_a[f] - x_b[f])^2 in float64 from the raw float32 values, features
    in ascending order, for all pairs of the k + 1 points (differences per feature, never n_a + n_b - 2 <a, b>).

    Chain, ``chain="sbn"`` (default; the paper's set-based nearest path).  Start with the set {o_0}.  For i = 1 .. k, add
    the remaining point with the smallest (d2 to the set, list position), the d2 of a point to the set being its minimum
    d2 over the set's members; e_i = sqrt of that d2.  Comparisons are made on d2, never on the square root; a tie goes
    to the lower list position.

    Chain, ``chain="rank"``.  e_i = sqrt(min_{j < i} d2(o_i, o_j)): the points are taken in list order and nothing is
    selected.  This is pyod's ``_cof_fast`` as its source is remembered here; pyod was not at hand to pin it, so the
    definition above and its numpy restatement in tests/test_outlier_cof_cpu.py are what binds, not pyod.

    Average chaining distance.  ac(q) = sum_{i = 1 .. k} w_i e_i with w_i = 2 (k + 1 - i) / (k (k + 1)), all float64, i
    ascending, no atomics and no order that depends on the launch.

    Score.  score_s(q) = ac(q) k / sum_{i = 1 .. k} ac_fit(o_i), where ac_fit are the chaining distances of the fitted
    rows computed at ``fit`` (self excluded).  ``fit`` runs two passes (ac of every row, then the ratio);
    ``decision_function`` computes ac of the new rows and reads the stored ac_fit (the split LOF has with its lrd).  The
    score is stored as float32 in the [S, n] score matrix; a value beyond the float32 range is stored as the largest
    finite float32, never inf.  The score is scale free like LOF (inliers sit around 1), so it sums across subspaces of
    mixed width without ``normalize``.

    Zero denominators (duplicates: common in narrow subspaces of discrete features).  Denominator 0 and ac(q) = 0: the
    score is exactly 1, the row is a point mass among point masses, and it is not degenerate.  Denominator 0 and
    ac(q) > 0: the row is DEGENERATE and takes the ceiling of its subspace, ``score_ceiling_[s]``: the largest float32
    score among the non-degenerate rows of the subspace at ``fit`` (1 if there is none).  ``fit`` publishes
    ``score_ceiling_`` (float64 [S]) and ``n_degenerate_`` (int [S]) in the given subspace order; ``decision_function``
    applies the stored ceiling and computes none of its own (SubspaceABOD's floor, with max in place of min).

    ``decision_function(X_train)`` is not ``decision_scores_``: there every row is its own nearest neighbour and the
    first edge of its chain is 0 (the remark of SubspaceABOD and of the KDE of SubspaceEnsemble, for the same reason).

    n_neighbors: 1 .. 32 (default 20, pyod's).  chain: "sbn" or "rank".  engine, splits, workspace_bytes: as for
    SubspaceEnsemble.  normalize, combination, contamination, ``threshold_``, ``labels_``, ``predict``,
    ``predict_proba``, return_per_subspace: the shared tail; ``per_subspace_scores_`` are the raw scores with the ceiling
    applied.  ``fit`` also publishes ``ac_dist_`` (float64 [S, n], given subspace order): the chaining distances of the
    fitted rows.  Given the same neighbour lists ``ac_dist_`` and the scores are bit-identical from run to run, and the
    lists do not depend on splits or workspace_bytes.  The chain, the ratio and the ceiling run in libvgan_hip.so
    (csrc/outlier_cof.hip)."""

    def __init__(self, subspaces, proba, n_neighbors=20, chain="sbn", engine="auto", splits=None,
                 workspace_bytes=DEFAULT_WORKSPACE_BYTES, normalize=None, combination="sum", contamination=0.1):
        if not (isinstance(chain, str) and chain in COF_CHAINS):
            raise ValueError(f"chain must be 'sbn' or 'rank', got {chain!r}")
        self.chain = chain
        self._configure(subspaces, proba, engine, workspace_bytes, normalize, combination, contamination)
        self._configure_neighbors(n_neighbors, splits)

    def _score(self, Xq, fitting):
        """(ensemble scores float64 [n], per float32 [S, n] with the ceiling applied), both on the device.  Each chunk runs
        both passes: the chaining distances of a subspace depend on that subspace's lists alone."""
        k, dev = self.n_neighbors, self._X.device
        nq = self._X.shape[0] if Xq is None else Xq.shape[0]
        per = torch.empty(self.plan.count, nq, dtype=torch.float32, device=dev)
        for first, count, idx, _ in self._neighbors(Xq):
            ac_ref = self._ac[first:first + count]  # processing order, like _lrd
            ac = ac_ref if fitting else torch.empty(count, nq, dtype=torch.float64, device=dev)
            self.ops.outlier_cof_chain(self._X if Xq is None else Xq, self._X, self._table, first, count, idx, k,
                                       COF_CHAINS[self.chain], ac)
            self.ops.outlier_cof_score(ac, ac_ref, idx, k, per, self._rows[first:first + count])
        self._fill_degenerate(per, fitting, self.ops.outlier_cof_ceiling)
        return self._combine(per, fitting), per

    def fit(self, X, y=None):
        """Keeps X resident as the reference set and scores it (self excluded): decision_scores_ (float64 [n]),
        per_subspace_scores_, ac_dist_, score_ceiling_, n_degenerate_; with normalize also score_center_ / score_scale_."""
        self._X = X = self._begin_fit(X)
        self._ac = torch.empty(self.plan.count, X.shape[0], dtype=torch.float64, device=X.device)
        scores, per = self._score(None, fitting=True)
        self.ac_dist_ = self._ac[torch.as_tensor(self.plan.given, device=X.device)].cpu().numpy()
        self.score_ceiling_ = self._fill.cpu().numpy()
        self.n_degenerate_ = self._n_degenerate.cpu().numpy().astype(np.int64)
        return self._publish(scores, per)


# ---- k-means + CBLOF over the subspaces ----------------------------------------------------------------------------------
MAX_CLUSTERS = 64  # VGAN_CLUSTER_MAX_CLUSTERS: the centres of a subspace are one reference tile of the distance engines
# Lloyd iterations enqueued between two looks at the done flags.  An iteration after a subspace has finished costs its
# launches an early return, a look costs a blocking copy: DESIGN.md section 9 has the measurement behind the value.
POLL_STRIDE = 4


def check_cblof_params(n_clusters, alpha, beta, max_iter, tol):
    if not (_is_int(n_clusters) and 2 <= int(n_clusters) <= MAX_CLUSTERS):
        raise ValueError(f"n_clusters must be an integer between 2 and {MAX_CLUSTERS}, got {n_clusters!r}")
    if not (_is_real(alpha) and 0.5 < float(alpha) < 1.0):
        raise ValueError(f"alpha must be a float in (0.5, 1), got {alpha!r}")
    if not (_is_real(beta) and np.isfinite(beta) and float(beta) > 1.0):
        raise ValueError(f"beta must be a finite float above 1, got {beta!r}")
    if not (_is_int(max_iter) and int(max_iter) >= 1):
        raise ValueError(f"max_iter must be a positive integer, got {max_iter!r}")
    if not (_is_real(tol) and np.isfinite(tol) and float(tol) >= 0.0):
        raise ValueError(f"tol must be a finite float >= 0, got {tol!r}")
    return int(n_clusters), float(alpha), float(beta), int(max_iter), float(tol)


def _index_array(init):
    """init as an integer array if it is one (an ndarray or nested lists of integers), else None."""
    if isinstance(init, np.ndarray):
        return init if init.dtype.kind in "iu" else None
    if isinstance(init, (list, tuple)) and len(init) > 0:
        try:
            a = np.asarray(init)
        except ValueError:  # ragged: a list of centre arrays of different widths
            return None
        return a if a.dtype.kind in "iu" else None
    return None


def check_kmeans_init(init, n_clusters, dims):
    """init as the constructor can judge it, without the data: "random", an integer array of row indices [C] or [S, C]
    (distinct within a subspace), or S float arrays [C, d_s] (dims: the d_s in the given subspace order).  Returns
    "random", ("rows", int64 [S, C]) or ("centers", [float64 [C, d_s]])."""
    S, C = len(dims), n_clusters
    if isinstance(init, str):
        if init != "random":
            raise ValueError(f"init must be 'random', row indices or a list of centre arrays, got {init!r}")
        return "random"
    if _index_array(init) is not None:
        idx = np.asarray(init, dtype=np.int64)
        if idx.ndim == 1:
            idx = np.broadcast_to(idx, (S, idx.shape[0]))
        if idx.ndim != 2 or idx.shape != (S, C):
            raise ValueError(f"init row indices must have shape ({C},) or ({S}, {C}), got {np.asarray(init).shape}")
        if (idx < 0).any():
            raise ValueError("init row indices must be >= 0")
        if (np.diff(np.sort(idx, axis=1), axis=1) == 0).any():
            raise ValueError("init row indices must be distinct within a subspace")
        return "rows", np.ascontiguousarray(idx)
    if isinstance(init, (list, tuple)) or (isinstance(init, np.ndarray) and init.dtype.kind == "f"):
        arrays = [init] if isinstance(init, np.ndarray) and init.ndim == 2 else list(init)
        if len(arrays) != S:
            raise ValueError(f"init holds {len(arrays)} centre arrays for {S} subspaces")
        out = []
        for s, (a, ds) in enumerate(zip(arrays, dims)):
            a = np.asarray(a, dtype=np.float64)
            if a.shape != (C, int(ds)):
                raise ValueError(f"init centres of subspace {s} must have shape ({C}, {int(ds)}), got {a.shape}")
            if not np.isfinite(a).all():
                raise ValueError(f"init centres of subspace {s} are not finite")
            out.append(np.ascontiguousarray(a))
        return "centers", out
    raise ValueError(f"init must be 'random', row indices or a list of centre arrays, got {type(init).__name__}")


def resolve_kmeans_rows(init, n, n_clusters, n_subspaces, seed):
    """int64 [S, C]: the initial rows for n data rows; "random" draws C distinct rows once with
    numpy.random.default_rng(seed) and uses them for every subspace."""
    if n < n_clusters:
        raise ValueError(f"fit needs at least n_clusters rows ({n_clusters}), got {n}")
    if isinstance(init, str):
        idx = np.random.default_rng(seed).choice(n, size=n_clusters, replace=False).astype(np.int64)
        return np.broadcast_to(idx, (n_subspaces, n_clusters)).copy()
    idx = init[1]
    if (idx >= n).any():
        raise ValueError(f"init row index {int(idx.max())} is out of range for {n} rows")
    return idx


def large_cluster_boundary(sizes, alpha, beta):
    """pyod's _set_small_large_clusters on one size table [C]: (t, large bool [C]).  The clusters are ordered by (size
    descending, index ascending); for i = 1 .. C-1, A_i: the first i sizes sum to >= alpha n; B_i: size_(i-1) / size_(i)
    >= beta (a zero denominator counts as holding).  t is the first i with A_i and B_i, failing that the first with A_i,
    failing that the first with B_i; the first t clusters are large.  Where pyod raises (no i at all) t = C: every
    cluster is large."""
    sizes = np.asarray(sizes, dtype=np.int64)
    C = sizes.shape[0]
    order = np.lexsort((np.arange(C), -sizes))
    sz = sizes[order]
    n = int(sz.sum())
    i = np.arange(1, C)
    A = np.cumsum(sz)[:-1] >= alpha * n
    with np.errstate(divide="ignore", invalid="ignore"):
        B = np.where(sz[1:] == 0, True, sz[:-1] / np.where(sz[1:] == 0, 1, sz[1:]) >= beta)
    t = C
    for cond in (A & B, A, B):
        if cond.any():
            t = int(i[np.argmax(cond)])
            break
    large = np.zeros(C, dtype=bool)
    large[order[:t]] = True
    return t, large


class SubspaceCBLOF(_SubspaceScorer):
    """Cluster-based local outlier factor per subspace (He, Xu, Deng 2003; pyod's CBLOF over k-means), combined like the
    detectors of SubspaceEnsemble: ``fit`` sets ``decision_scores_``, ``decision_function`` scores new rows.

    Per subspace s (features F_s, raw values, squared Euclidean distance), C = n_clusters (2 .. 64):

    k-means (Lloyd).  init "random": C distinct rows drawn once with numpy.random.default_rng(seed), the same rows for
    every subspace; or row indices [C] / [S, C]; or S float arrays [C, d_s] (given subspace order).  No k-means++, no
    restarts.  E step: every row takes the centre with the smallest (d2, centre index), d2 from the subspace's float32
    distance engine (exact below GRAM_MIN_DIMS, Gram above, as for kNN; here the operands of both engines are centred on
    the column mean, so that rounding a centre to float32 costs no more than rounding a data row).  M step:
    every centre becomes the mean of its rows, accumulated in float64 from the float32 data; the float64 centre is the
    master copy and the engines' float32 image is derived from it after every update.  A cluster that received no row
    keeps its centre (sklearn relocates it to a far row instead; the two differ whenever a cluster empties).  A
    subspace stops when an E step changes no label (``converged_[s]`` True; no M step follows), or when the summed
    squared centre shift of an M step is <= tol x the mean population variance of its features (sklearn's rule; tol=0
    disables it; ``converged_[s]`` stays False), or after max_iter M steps.  ``n_iter_[s]`` counts the M steps.  After
    the loop one assignment in float64 from the raw rows and the float64 centres gives ``cluster_labels_`` (the exactly
    nearest centre of ``cluster_centers_`` by (d2, index)), ``inertia_`` (the float64 sum of those d2) and
    ``cluster_sizes_``; the float32 engines serve only the iterations.

    Large and small clusters: large_cluster_boundary (pyod's rule, alpha in (0.5, 1), beta > 1) on every subspace's size
    table -> ``large_cluster_mask_``.  Where pyod raises "could not form valid cluster separation" every cluster of that
    subspace counts as large: one odd subspace out of hundreds does not fail the ensemble.

    Score: the float64 distance of a row to its nearest centre if that cluster is large, otherwise to the nearest large
    centre; times the size of the row's cluster with use_weights.  The score matrix is float32 [S, n], and normalize /
    combination / contamination / ``threshold_`` / ``labels_`` (outlier labels, pyod's meaning) / ``predict`` /
    ``predict_proba`` / return_per_subspace are those of SubspaceEnsemble.  ``fit`` scores the training rows with nothing
    excluded: ``decision_function(X_train)`` equals ``decision_scores_`` bit for bit.

    No float atomics: the centre sums run over a fixed partition of the rows (slices by n; inside a slice, row groups
    by n_clusters and d_s), never by the chunk, so labels, centres, ``n_iter_`` and scores are bit-identical from run to
    run and for every workspace_bytes; they may differ between the two engines.  All of it runs in libvgan_hip.so
    (csrc/cluster.hip).  workspace_bytes limits the packed blocks of a chunk as in SubspaceEnsemble; the chunk's
    iteration labels (int32 [count, n]) and the slice partials of the centre sums (float64, ceil(n / 1024) x n_clusters
    x (sum of d_s + count)) come on top of it.

    Two attributes, set after construction, serve tests and measurements and change no result: ``poll_stride`` (Lloyd
    iterations enqueued between two looks at the done flags, default POLL_STRIDE) and ``keep_iteration_labels`` (True:
    ``fit`` also publishes ``last_iteration_labels_``, int32 [S, n], the labels of the last E step, which the float32
    engines took, as opposed to the float64 ``cluster_labels_``)."""

    def __init__(self, subspaces, proba, n_clusters=8, alpha=0.9, beta=5.0, use_weights=False, init="random", max_iter=300,
                 tol=1e-4, seed=0, engine="auto", workspace_bytes=DEFAULT_WORKSPACE_BYTES, normalize=None, combination="sum",
                 contamination=0.1):
        self.n_clusters, self.alpha, self.beta, self.max_iter, self.tol = check_cblof_params(n_clusters, alpha, beta, max_iter, tol)
        self._configure(subspaces, proba, engine, workspace_bytes, normalize, combination, contamination)
        self.init = check_kmeans_init(init, self.n_clusters, self.plan.dims[self.plan.given])
        self.use_weights, self.seed = bool(use_weights), seed
        self.poll_stride = POLL_STRIDE
        self.keep_iteration_labels = False

    # ---- pipeline --------------------------------------------------------------------------------
    def _initial_centers(self, X, n):
        """float64 centres of every subspace in processing order, concatenated ([C, d_s] blocks)."""
        feats = [self.plan.feat[self.plan.feat_off[z]:self.plan.feat_off[z + 1]] for z in range(self.plan.count)]
        if isinstance(self.init, tuple) and self.init[0] == "centers":
            return np.concatenate([self.init[1][s].reshape(-1) for s in self.plan.order])
        idx = resolve_kmeans_rows(self.init, n, self.n_clusters, self.plan.count, self.seed)
        uniq, inv = np.unique(idx, return_inverse=True)
        rows = X[torch.as_tensor(uniq, device=X.device)].cpu().numpy().astype(np.float64)
        inv = inv.reshape(idx.shape)
        return np.concatenate([rows[inv[s]][:, feats[z]].reshape(-1) for z, s in enumerate(self.plan.order)])

    def _tolerance(self, X):
        """float64 [S], processing order: tol x the mean over F_s of the population variance of the feature (float64 numpy
        on a host copy of X, once per fit; tol = 0 skips it)."""
        S = self.plan.count
        if self.tol == 0.0:
            return np.zeros(S)
        host = X.cpu().numpy()
        var = np.concatenate([host[:, c:c + 64].astype(np.float64).var(axis=0) for c in range(0, host.shape[1], 64)])
        return np.array([self.tol * var[self.plan.feat[self.plan.feat_off[z]:self.plan.feat_off[z + 1]]].mean() for z in range(S)])

    def _lloyd_buffers(self, X, first, count, gram):
        """(Pq, sqq, img, img_sq, label, ws, sum of d_s, largest d_s, engine) of a chunk, as vgan_cluster_lloyd takes them:
        the packed block of X, the float32 image of the current centres, the iteration labels (-1) and the workspace."""
        n, C, dev = X.shape[0], self.n_clusters, X.device
        # both engines get operands centred on the column mean here: a centre is a float64 mean, and rounding it to
        # float32 about the mean instead of about 0 keeps that rounding small on data with a large offset
        cols = int(self.plan.col_off[first + count] - self.plan.col_off[first])
        dims = self.plan.dims[first:first + count]
        Pq, sqq = self._pack(X, first, count, gram, centred=True)
        img = torch.empty(C * cols, dtype=torch.float32, device=dev)
        img_sq = torch.empty(count, C, dtype=torch.float32, device=dev) if gram else None
        self.ops.cluster_image(self._centers, C, self._table, first, count, self._center, img, img_sq)
        label = torch.full((count, n), -1, dtype=torch.int32, device=dev)
        ws = torch.empty(self.ops.cluster_lloyd_ws_bytes(n, C, count, int(dims.sum())) // 8, dtype=torch.float64, device=dev)
        return Pq, sqq, img, img_sq, label, ws, int(dims.sum()), int(dims.max()), ENGINES["gram" if gram else "exact"]

    def _lloyd(self, X):
        """Chunks outermost, iterations inside: a chunk is packed once.  The host enqueues poll_stride iterations at a
        time and then reads the chunk's done flags through one pinned buffer."""
        n, S, C, dev = X.shape[0], self.plan.count, self.n_clusters, X.device
        self._changed = torch.zeros(S, dtype=torch.int32, device=dev)
        self._done = torch.zeros(S, dtype=torch.int32, device=dev)
        self._iters = torch.zeros(S, dtype=torch.int32, device=dev)
        self._iteration_labels = torch.empty(S, n, dtype=torch.int32, device=dev) if self.keep_iteration_labels else None
        flags = torch.empty(S, dtype=torch.int32).pin_memory()
        stream = torch.cuda.current_stream()
        for first, count, gram in self.plan.chunks(n, self.workspace_bytes):
            Pq, sqq, img, img_sq, label, ws, total, widest, engine = self._lloyd_buffers(X, first, count, gram)
            launched = 0
            while launched < self.max_iter:
                it = min(max(1, int(self.poll_stride)), self.max_iter - launched)
                self.ops.cluster_lloyd(Pq, sqq, X, self._table, first, count, total, widest, C, engine, self._center, self._tol_var,
                                       self._centers, img, img_sq, label, self._changed, self._done, self._iters, ws, it)
                launched += it
                flags[:count].copy_(self._done[first:first + count], non_blocking=True)
                stream.synchronize()
                if bool((flags[:count] != 0).all()):
                    break
            if self.keep_iteration_labels:
                self._iteration_labels[first:first + count] = label
            del Pq, sqq, img, img_sq, label, ws

    def _final(self, X, want_labels=False):
        """(per float32 [S, n] in the given order, labels int32 [S, n] in processing order or None) of X against the fitted
        centres, float64."""
        S, C, nq = self.plan.count, self.n_clusters, X.shape[0]
        label = torch.empty(S, nq, dtype=torch.int32, device=X.device) if want_labels else None
        per = torch.empty(S, nq, dtype=torch.float32, device=X.device)
        self.ops.cluster_final(X, self._table, S, C, self._centers, self._sizes, large=self._large, use_weights=self.use_weights,
                               label=label, score=per, score_row=self._rows)
        return per, label

    def _score(self, X, fitting):
        per, _ = self._final(X)
        return self._combine(per, fitting), per

    def _check_fit_rows(self, n):
        if not isinstance(self.init, tuple) or self.init[0] == "rows":
            resolve_kmeans_rows(self.init, n, self.n_clusters, self.plan.count, self.seed)  # its checks; the rows come later
        elif n < self.n_clusters:
            raise ValueError(f"fit needs at least n_clusters rows ({self.n_clusters}), got {n}")

    # ---- public surface --------------------------------------------------------------------------
    def fit(self, X, y=None):
        """k-means per subspace on X, then the CBLOF scores of X itself: decision_scores_ (float64 [n]),
        per_subspace_scores_, cluster_centers_, cluster_labels_, cluster_sizes_, large_cluster_mask_, n_iter_,
        converged_, inertia_, all in the given subspace order.  The centres, the sizes and the large-cluster mask are the
        fitted state: X itself is not kept."""
        X = self._begin_fit(X)
        n, S, C, dev = X.shape[0], self.plan.count, self.n_clusters, X.device
        self._centers = torch.as_tensor(self._initial_centers(X, n), device=dev)
        self._tol_var = torch.as_tensor(self._tolerance(X), device=dev)
        self._lloyd(X)
        # final float64 assignment, the host boundary step, the scores
        self._sizes = torch.zeros(S, C, dtype=torch.int64, device=dev)
        labels = torch.empty(S, n, dtype=torch.int32, device=dev)
        inertia = torch.empty(S, dtype=torch.float64, device=dev)
        self.ops.cluster_final(X, self._table, S, C, self._centers, self._sizes, label=labels, inertia=inertia)
        sizes = self._sizes.cpu().numpy()
        large = np.stack([large_cluster_boundary(sizes[z], self.alpha, self.beta)[1] for z in range(S)])
        self._large = torch.as_tensor(large.astype(np.int32), device=dev)
        scores, per = self._score(X, fitting=True)
        g = self.plan.given
        flat, off = self._centers.cpu().numpy(), C * self.plan.feat_off.astype(np.int64)
        self.cluster_centers_ = [flat[off[z]:off[z + 1]].reshape(C, -1).copy() for z in g]
        self.cluster_labels_ = labels.cpu().numpy()[g]
        self.cluster_sizes_ = sizes[g]
        self.large_cluster_mask_ = large[g]
        self.n_iter_ = self._iters.cpu().numpy()[g].astype(np.int64)
        self.converged_ = self._done.cpu().numpy()[g] == 1
        self.inertia_ = inertia.cpu().numpy()[g]
        if self.keep_iteration_labels:
            self.last_iteration_labels_ = self._iteration_labels.cpu().numpy()[g]
            self._iteration_labels = None
        return self._publish(scores, per)

    def predict_clusters(self, X):
        """int32 [S, n]: the nearest fitted centre of every row of X in every subspace (float64, (d2, index) order)."""
        self._require_fit()
        _, label = self._final(_device_matrix(X, self.plan.d), want_labels=True)
        return label.cpu().numpy()[self.plan.given]


# ---- ECOD: empirical-CDF tail probabilities over the subspaces ---------------------------------------------------------
ECOD_MAX_ROWS = 1 << 24  # VGAN_ECOD_MAX_ROWS: the padded columns of the sort stay below 2^25 keys, the counts in int32
ECOD_SORT_RUN = 2048  # VGAN_ECOD_SORT_RUN: keys of one LDS-resident run of the column sort
ECOD_AGGREGATES = {"dimension": 0, "tail": 1}  # VGAN_ECOD_AGGREGATE_*


def check_aggregate(aggregate):
    if not (isinstance(aggregate, str) and aggregate in ECOD_AGGREGATES):
        raise ValueError(f"aggregate must be 'dimension' or 'tail', got {aggregate!r}")
    return aggregate


def ecod_chunk_rows(d, n_subspaces, aggregate, workspace_bytes):
    """Rows of one scoring chunk: the counts (two int32 [rows, d]), the float64 terms ([rows, d], three of them for "tail")
    and the chunk's float32 scores [S, rows] fit in workspace_bytes; at least one row."""
    planes = 3 if check_aggregate(aggregate) == "tail" else 1
    return max(1, int(workspace_bytes) // (int(d) * (8 + 8 * planes) + 4 * int(n_subspaces)))


class SubspaceECOD(_SubspaceScorer):
    """Empirical-CDF outlier detector per subspace (ECOD: Li, Zhao, Hu, Botta, Ionescu, Chen 2022; pyod's ``ECOD``), combined
    like the detectors of SubspaceEnsemble: ``fit`` sets ``decision_scores_``, ``decision_function`` scores new rows; higher
    is more outlying.  No hyper-parameter, no neighbour search, nothing n x n.

    X is cast to float32; all arithmetic is float64 on those values, and -0.0 counts as +0.0.  n is the number of rows
    given to ``fit``, 1 <= n <= ECOD_MAX_ROWS (2^24).  Per feature f, ``fit`` keeps the ascending column
    (``sorted_columns_``, float32 [d, n]) and the sign of its skewness (``skew_sign_``, int [d]): mu = sum(x) / n, m2 =
    sum((x - mu)^2), m3 = sum((x - mu)^3), g_f = 0 if m2 == 0 else sign(m3) (two passes, the same bits from run to run; a
    constant column, where scipy's skew is NaN, has sign 0).

    For a value x of feature f: cl = #{r : X[r, f] <= x}, cr = #{r : X[r, f] >= x} among the n fitted rows.
    ``fit``: ul = -log(cl / n), ur = -log(cr / n) (the row counts itself).  ``decision_function``: ul = -log((cl + 1) /
    (n + 1)), likewise ur: the score pyod gives a row scored alone, appended to the training set; it is never log 0 and
    does not depend on the other rows of the batch, and the skew signs stay those of ``fit``.  So
    ``decision_function(X_train)`` is not ``decision_scores_`` (as with SubspaceABOD).  The quotient is one IEEE division,
    then log.  usk = ul if g_f < 0, ur if g_f > 0, ul + ur if g_f == 0.  Score of a row in subspace s (features F_s):

        aggregate "dimension" (default, pyod's code):  sum_{f in F_s} max(ul, ur, usk)
        aggregate "tail" (the paper's equation):       max(sum_f ul, sum_f ur, sum_f usk)

    rounded to float32 into the [S, n] score matrix; normalize, combination, contamination, ``threshold_``, ``labels_``,
    ``predict``, ``predict_proba`` and return_per_subspace are the shared tail.

    These rules are pyod's as its source is remembered here; pyod was not at hand to pin them (its ``decision_function``
    concatenates the batch to the training set, which is deliberately not done here), so the definition above and its
    numpy restatement in tests/test_outlier_ecod_cpu.py (counts pinned to scipy's rankdata, signs to scipy's skew) are
    what binds, not pyod.

    The tail terms do not depend on the subspace: they are formed once per row chunk and every subspace is a 0/1-masked
    sum of them, one dense float64 product on the matrix unit.  workspace_bytes limits the counts, terms and scores of a
    row chunk (ecod_chunk_rows).  The bits of a score depend on the row's counts alone: scores are bit-identical for every
    workspace_bytes and from run to run.  NaN input leaves the scores unspecified and neither faults nor hangs.  All of it
    runs in libvgan_hip.so (csrc/outlier_ecod.hip)."""

    _host_sorted = None

    def __init__(self, subspaces, proba, aggregate="dimension", workspace_bytes=DEFAULT_WORKSPACE_BYTES, normalize=None,
                 combination="sum", contamination=0.1):
        self.aggregate = check_aggregate(aggregate)
        # no distance engine here: "exact" for every subspace keeps the processing order the given order
        self._configure(subspaces, proba, "exact", workspace_bytes, normalize, combination, contamination)
        del self.engine

    def _check_fit_rows(self, n):
        if not 1 <= n <= ECOD_MAX_ROWS:
            raise ValueError(f"ECOD fit needs between 1 and {ECOD_MAX_ROWS} rows, got {n}")

    def _chunk_rows(self):
        return ecod_chunk_rows(self.plan.d, self.plan.count, self.aggregate, self.workspace_bytes)

    def _score(self, X, fitting):
        nq, d = X.shape
        S, dev = self.plan.count, X.device
        rows = min(self._chunk_rows(), nq)
        planes = 3 if self.aggregate == "tail" else 1
        cl = torch.empty(rows * d, dtype=torch.int32, device=dev)
        cr = torch.empty(rows * d, dtype=torch.int32, device=dev)
        terms = torch.empty(planes * rows * d, dtype=torch.float64, device=dev)
        per = torch.empty(S, nq, dtype=torch.float32, device=dev)
        for r0 in range(0, nq, rows):
            r1 = min(r0 + rows, nq)
            self.ops.ecod_tail_counts(X[r0:r1], self._sorted, self._n, cl, cr)
            self.ops.ecod_scores(cl, cr, r1 - r0, self._sign, self._n, not fitting, ECOD_AGGREGATES[self.aggregate], self._mask, terms,
                                 per[:, r0:r1])
        return self._combine(per, fitting), per

    @property
    def sorted_columns_(self):
        """float32 [d, n]: the ascending columns of the fitted rows (-0.0 as +0.0); copied to the host on first use."""
        self._require_fit()
        if self._host_sorted is None:
            self._host_sorted = self._sorted[:, :self._n].cpu().numpy()
        return self._host_sorted

    def fit(self, X, y=None):
        """Sorts every column of X and takes its skew sign, then scores X itself by the fit rule: decision_scores_ (float64
        [n]), per_subspace_scores_, skew_sign_, sorted_columns_; with normalize also score_center_ / score_scale_.  The
        sorted columns and the signs are the fitted state: X itself is not kept."""
        X = self._begin_fit(X)
        n, d = X.shape
        self._n, self._host_sorted = n, None
        self._sorted = torch.empty(d, 1 << (n - 1).bit_length(), dtype=torch.float32, device=X.device)
        self.ops.ecod_sort_columns(X, self._sorted)
        self._sign = torch.empty(d, dtype=torch.int8, device=X.device)
        self.ops.ecod_skew_sign(self._sorted, n, self._sign)
        mask = np.zeros((d, self.plan.count), dtype=np.float64)  # column = given subspace index
        for z, s in enumerate(self.plan.order):
            mask[self.plan.feat[self.plan.feat_off[z]:self.plan.feat_off[z + 1]], s] = 1.0
        self._mask = torch.as_tensor(mask, device=X.device)
        scores, per = self._score(X, fitting=True)
        self.skew_sign_ = self._sign.cpu().numpy().astype(np.int64)
        return self._publish(scores, per)


# ---- histogram scores: HBOS and LODA over the subspaces ------------------------------------------------------------------
HIST_MAX_BINS = 256  # VGAN_HIST_MAX_BINS: the bin search runs eight halvings
HIST_MAX_ROWS = 1 << 24  # VGAN_HIST_MAX_ROWS: the counts stay in int32
LODA_MAX_PROJECTIONS = 1024  # VGAN_LODA_MAX_PROJECTIONS: the (min, max) pairs of a subspace's projections live in LDS
LODA_MAX_DIMS = 8192  # VGAN_LODA_MAX_DIMS: packed features of one subspace (a row of it is staged in LDS)
_LODA_MAX_RANGE = 65535  # subspaces of one launch (a grid dimension)
_LODA_FLOOR = 1e-12  # what LODA adds to every count before the logarithm


def check_bins(n_bins):
    if not (_is_int(n_bins) and 2 <= int(n_bins) <= HIST_MAX_BINS):
        raise ValueError(f"n_bins must be an integer between 2 and {HIST_MAX_BINS}, got {n_bins!r}")
    return int(n_bins)


def check_hbos_params(alpha, tol):
    if not (_is_real(alpha) and np.isfinite(alpha) and alpha > 0):
        raise ValueError(f"alpha must be a positive number, got {alpha!r}")
    if not (_is_real(tol) and np.isfinite(tol) and tol >= 0):
        raise ValueError(f"tol must be a non-negative number, got {tol!r}")
    return float(alpha), float(tol)


def check_projections(n_projections):
    if not (_is_int(n_projections) and 1 <= int(n_projections) <= LODA_MAX_PROJECTIONS):
        raise ValueError(f"n_projections must be an integer between 1 and {LODA_MAX_PROJECTIONS}, got {n_projections!r}")
    return int(n_projections)


def hbos_chunk_rows(d, n_subspaces, workspace_bytes):
    """Rows of one HBOS scoring chunk: the float64 terms [rows, d] and the chunk's float32 scores [S, rows] fit in
    workspace_bytes; at least one row."""
    return max(1, int(workspace_bytes) // (8 * int(d) + 4 * int(n_subspaces)))


def hbos_term_table(counts, edges, n, alpha, tol):
    """(table float64 [d, B + 1], limits float64 [d, 2]) from the counts [d, B] and edges [d, B + 1] of n fitted rows: step =
    (e_B - e_0) / B, dens[b] = count_b / (n step), table[:, b] = -log2(dens[b] + alpha) for b < B and table[:, B] = -log2(min_b
    dens[b] + alpha), the term of a value outside the limits (e_0 - tol step, e_B + tol step)."""
    counts, edges = np.asarray(counts, dtype=np.float64), np.asarray(edges, dtype=np.float64)
    B = counts.shape[-1]
    lo, hi = edges[..., 0], edges[..., -1]
    step = (hi - lo) / B
    dens = counts / (float(n) * step)[..., None]
    table = np.concatenate([-np.log2(dens + alpha), -np.log2(dens.min(axis=-1) + alpha)[..., None]], axis=-1)
    return table, np.stack([lo - tol * step, hi + tol * step], axis=-1)


def loda_term_table(counts, n):
    """float64 [..., B]: -log(p[b]) with p[b] = (count_b + 1e-12) / (n + B 1e-12), from the counts [..., B] of n fitted rows."""
    counts = np.asarray(counts, dtype=np.float64)
    return -np.log((counts + _LODA_FLOOR) / (float(n) + counts.shape[-1] * _LODA_FLOOR))


def loda_projections(dims, n_projections, seed):
    """(features, weights): per subspace of d_s = dims[s] features an int64 [k, m_s] array of positions within the subspace
    (ascending, distinct) and a float64 [k, m_s] array of weights, m_s = max(1, floor(sqrt(d_s))), drawn from rng =
    numpy.random.default_rng(seed) subspace by subspace and j = 0 .. k - 1: sort(rng.choice(d_s, m_s, replace=False)), then
    rng.standard_normal(m_s)."""
    rng = np.random.default_rng(seed)
    k = int(n_projections)
    features, weights = [], []
    for d_s in np.asarray(dims, dtype=np.int64).reshape(-1):
        m = max(1, math.isqrt(int(d_s)))
        f, w = np.empty((k, m), dtype=np.int64), np.empty((k, m), dtype=np.float64)
        for j in range(k):
            f[j] = np.sort(rng.choice(int(d_s), m, replace=False))
            w[j] = rng.standard_normal(m)
        features.append(f)
        weights.append(w)
    return features, weights


def loda_chunks(dims, n, workspace_bytes):
    """(rows of a row chunk, [(first, count)] subspace ranges): the transient buffer of a LODA launch is the packed block of
    its rows and subspaces, float32 [rows, round4(d_s)] per subspace.  All subspaces form one range and the rows are chunked
    while a row of every subspace fits: rows = min(n, workspace_bytes // (4 sum_s round4(d_s))); below that the chunks are
    single rows and a range takes consecutive subspaces while their rows fit (at least one; never more than 65535)."""
    widths = _round4(np.asarray(dims).reshape(-1))
    limit = int(workspace_bytes)
    rows = int(min(int(n), max(1, limit // (4 * int(widths.sum())))))
    ranges, first = [], 0
    while first < len(widths):
        end, used = first, 0
        while end < len(widths) and end - first < _LODA_MAX_RANGE:
            need = rows * int(widths[end]) * 4
            if end > first and used + need > limit:
                break
            used += need
            end += 1
        ranges.append((first, end - first))
        first = end
    return rows, ranges


class SubspaceHBOS(_SubspaceScorer):
    """Histogram-based outlier score per subspace (HBOS: Goldstein and Dengel 2012; pyod's ``HBOS`` with a fixed number of
    bins), combined like the other detectors of this module: ``fit`` sets ``decision_scores_``, ``decision_function`` scores
    new rows; higher is more outlying.  Linear in n: no neighbour search, no sort, nothing n x n.

    X is cast to float32; all arithmetic is float64 on those values, and -0.0 counts as +0.0.  n is the number of rows
    given to ``fit``, 1 <= n <= HIST_MAX_ROWS (2^24); B = n_bins, an integer from 2 to 256 (pyod's "auto" is not built);
    alpha > 0; tol >= 0.

    The histogram of a column of n values: lo, hi its minimum and maximum (lo == hi: lo - 0.5, lo + 0.5, numpy's rule); step
    = (hi - lo) / B; edges e_j = j * step + lo for j = 0 .. B with two roundings (the product, then the sum) and e_B = hi:
    ``numpy.linspace(lo, hi, B + 1)`` bit for bit.  The bin of a value x is #{j in 1 .. B - 1 : e_j <= x}: the bin
    ``numpy.histogram(col, bins=B)`` counts x in; a value outside [lo, hi] falls into the first or the last bin.  count_b is
    the number of fitted values in bin b.

    Every feature f gets one histogram of its fitted column: dens_f[b] = count_b / (n step_f), term_f[b] = -log2(dens_f[b] +
    alpha).  A scored value x of feature f takes term_f[bin(x)], except where x < lo_f - tol step_f or x > hi_f + tol step_f:
    there it takes -log2(min_b dens_f[b] + alpha).  The score of a row in subspace s is the sum of its terms over the
    features of s, rounded to float32 into the [S, n] score matrix; scores may be negative.  ``fit`` excludes nothing, so
    ``decision_function(X_train)`` equals ``decision_scores_`` bit for bit.

    ``fit`` publishes ``bin_edges_`` (float64 [d, B + 1]) and ``histograms_`` (int64 [d, B]); normalize, combination,
    contamination, ``threshold_``, ``labels_``, ``predict``, ``predict_proba`` and return_per_subspace are the shared tail.

    These rules are pyod's as its source is remembered here; pyod was not at hand to pin them, so the definition above and
    its numpy restatement in tests/test_outlier_hist_cpu.py (edges pinned to numpy.linspace, counts to numpy.histogram) are
    what binds, not pyod.

    The terms do not depend on the subspace: the term tables are built on the host in float64 from the integer counts
    (hbos_term_table) and uploaded; per row chunk the terms are looked up and every subspace is a 0/1-masked sum of them,
    the dense float64 product on the matrix unit that SubspaceECOD runs.  workspace_bytes limits the terms and scores of a
    row chunk (hbos_chunk_rows).  Counts are integer sums and the bits of a score depend on the row alone: scores and
    published arrays are bit-identical for every workspace_bytes, from run to run and for a subspace fitted alone or with
    others.  NaN or infinite input leaves the scores unspecified and neither faults nor hangs.  All of it runs in
    libvgan_hip.so (csrc/outlier_hist.hip)."""

    def __init__(self, subspaces, proba, n_bins=10, alpha=0.1, tol=0.5, workspace_bytes=DEFAULT_WORKSPACE_BYTES, normalize=None,
                 combination="sum", contamination=0.1):
        self.n_bins = check_bins(n_bins)
        self.alpha, self.tol = check_hbos_params(alpha, tol)
        # no distance engine here: "exact" for every subspace keeps the processing order the given order
        self._configure(subspaces, proba, "exact", workspace_bytes, normalize, combination, contamination)
        del self.engine

    def _check_fit_rows(self, n):
        if not 1 <= n <= HIST_MAX_ROWS:
            raise ValueError(f"SubspaceHBOS fit needs between 1 and {HIST_MAX_ROWS} rows, got {n}")

    def _score(self, X, fitting):
        nq, d = X.shape
        S, dev = self.plan.count, X.device
        rows = min(hbos_chunk_rows(d, S, self.workspace_bytes), nq)
        terms = torch.empty(rows * d, dtype=torch.float64, device=dev)
        per = torch.empty(S, nq, dtype=torch.float32, device=dev)
        for r0 in range(0, nq, rows):
            r1 = min(r0 + rows, nq)
            self.ops.hbos_scores(X[r0:r1], self._edges, self._terms, self._limits, self._mask, terms, per[:, r0:r1])
        return self._combine(per, fitting), per

    def fit(self, X, y=None):
        """One histogram per column of X (range, edges, integer counts on the device; the term table on the host), then
        scores X itself: decision_scores_ (float64 [n]), per_subspace_scores_, bin_edges_, histograms_; with normalize also
        score_center_ / score_scale_.  The edges and the term table are the fitted state: X itself is not kept."""
        X = self._begin_fit(X)
        n, d = X.shape
        B, dev = self.n_bins, X.device
        keys = torch.empty(d, 2, dtype=torch.int64, device=dev)
        self.ops.hist_column_range(X, keys)
        self._edges = torch.empty(d, B + 1, dtype=torch.float64, device=dev)
        self.ops.hist_edges(keys, B, self._edges)
        counts = torch.empty(d, B, dtype=torch.int32, device=dev)
        self.ops.hist_column_counts(X, self._edges, counts)
        self.bin_edges_ = self._edges.cpu().numpy()
        self.histograms_ = counts.cpu().numpy().astype(np.int64)
        table, limits = hbos_term_table(self.histograms_, self.bin_edges_, n, self.alpha, self.tol)
        self._terms, self._limits = torch.as_tensor(table, device=dev), torch.as_tensor(limits, device=dev)
        mask = np.zeros((d, self.plan.count), dtype=np.float64)  # column = given subspace index
        for z, s in enumerate(self.plan.order):
            mask[self.plan.feat[self.plan.feat_off[z]:self.plan.feat_off[z + 1]], s] = 1.0
        self._mask = torch.as_tensor(mask, device=dev)
        scores, per = self._score(X, fitting=True)
        return self._publish(scores, per)


class SubspaceLODA(_SubspaceScorer):
    """Lightweight on-line detector of anomalies per subspace (LODA: Pevny 2016; pyod's ``LODA`` with a fixed number of
    bins), combined like the other detectors of this module: ``fit`` sets ``decision_scores_``, ``decision_function`` scores
    new rows; higher is more outlying.  Linear in n.  A projection restricted to a subspace's features is the detector's own
    idea, sparse projections as feature bagging, with the subspaces choosing the bag.

    X is cast to float32; all arithmetic is float64 on those values.  n is the number of rows given to ``fit``, 1 <= n <=
    HIST_MAX_ROWS (2^24); k = n_projections, 1 .. 1024; B = n_bins, an integer from 2 to 256 (pyod's "auto" is not built);
    seed a non-negative integer; a subspace has at most LODA_MAX_DIMS (8192) features.

    Subspace s has d_s features and m_s = max(1, floor(sqrt(d_s))) nonzeros per projection.  The projections are drawn on
    the host, once, by loda_projections(dims, k, seed): rng = numpy.random.default_rng(seed); over the subspaces in the
    given order and j = 0 .. k - 1: idx = sort(rng.choice(d_s, m_s, replace=False)), then w = rng.standard_normal(m_s).
    ``fit`` publishes them as ``projection_features_`` (a list of S int arrays [k, m_s], positions within the subspace) and
    ``projection_weights_`` (S float64 arrays [k, m_s]).  The projected value of a row is z = (((0 + w_0 x_{f_0}) + w_1
    x_{f_1}) + ...), the nonzeros in ascending feature order, every product and every sum rounded on its own: in numpy,
    acc = acc + w[t] * x[:, f_t].

    Projection (s, j) gets one histogram of the n fitted z values, by the rules of SubspaceHBOS: lo, hi the minimum and
    maximum (lo == hi: lo - 0.5, lo + 0.5); step = (hi - lo) / B; e_j = j * step + lo in two roundings, e_B = hi
    (numpy.linspace bit for bit); the bin of z is #{j in 1 .. B - 1 : e_j <= z} (numpy.histogram's bin; outside [lo, hi]
    the first or last bin).  p[b] = (count_b + 1e-12) / (n + B 1e-12).  The score of a row in subspace s is (1 / k) sum_j
    -log(p_{s,j}[bin(z_{s,j})]), rounded to float32 into the [S, n] score matrix; it is never negative.  ``fit`` excludes
    nothing, so ``decision_function(X_train)`` equals ``decision_scores_`` bit for bit.

    ``fit`` publishes ``bin_edges_`` (float64 [S, k, B + 1]) and ``histograms_`` (int64 [S, k, B]); normalize, combination,
    contamination, ``threshold_``, ``labels_``, ``predict``, ``predict_proba`` and return_per_subspace are the shared tail.

    These rules are pyod's as its source is remembered here and are not pinned against pyod; its ``limits[:n_bins - 1]``
    lookup looks like an off-by-one and is deliberately not reproduced.  The definition above and its numpy restatement in
    tests/test_outlier_hist_cpu.py are what binds.

    Nothing n x S x k is stored: z is recomputed by the range, the count and the scoring pass.  workspace_bytes limits the
    packed block of a launch (loda_chunks: a row chunk and a range of subspaces).  Minima, maxima and counts are integer
    atomics, the log-probability tables are built on the host in float64 (loda_term_table) and uploaded, and the sum over j
    runs in an order fixed by k alone: scores and published arrays are bit-identical for every workspace_bytes, from run to
    run and, given the same projections, for a subspace fitted alone or with others.  NaN or infinite input leaves the
    scores unspecified and neither faults nor hangs.  All of it runs in libvgan_hip.so (csrc/outlier_hist.hip)."""

    _proj = None  # (pidx, pw, moff, k) on the device, set by the first fit

    def __init__(self, subspaces, proba, n_projections=100, n_bins=10, seed=0, workspace_bytes=DEFAULT_WORKSPACE_BYTES,
                 normalize=None, combination="sum", contamination=0.1):
        self.n_projections = check_projections(n_projections)
        self.n_bins = check_bins(n_bins)
        self.seed = check_seed(seed)
        # no distance engine here: "exact" for every subspace keeps the processing order the given order
        self._configure(subspaces, proba, "exact", workspace_bytes, normalize, combination, contamination)
        del self.engine
        if int(self.plan.dims.max()) > LODA_MAX_DIMS:
            raise ValueError(f"a subspace has {int(self.plan.dims.max())} features, SubspaceLODA takes at most {LODA_MAX_DIMS}")

    def _check_fit_rows(self, n):
        if not 1 <= n <= HIST_MAX_ROWS:
            raise ValueError(f"SubspaceLODA fit needs between 1 and {HIST_MAX_ROWS} rows, got {n}")

    def _blocks(self, X):
        """Yields (packed block, rows, first row, first subspace, count, widest packed subspace) over the chunks of X."""
        rows, ranges = loda_chunks(self.plan.dims, X.shape[0], self.workspace_bytes)
        for first, count in ranges:
            width = int(_round4(self.plan.dims[first:first + count]).max())
            for r0 in range(0, X.shape[0], rows):
                r1 = min(r0 + rows, X.shape[0])
                yield self._pack(X[r0:r1], first, count, False)[0], r1 - r0, r0, first, count, width

    def _score(self, X, fitting):
        per = torch.empty(self.plan.count, X.shape[0], dtype=torch.float32, device=X.device)
        for packed, rows, r0, first, count, width in self._blocks(X):
            self.ops.loda_scores(packed, rows, self._table, first, count, width, self._proj, self._edges, self._terms, per[:, r0:r0 + rows])
        return self._combine(per, fitting), per

    def fit(self, X, y=None):
        """Draws the projections on the host, takes the range and the integer counts of every projected column on the
        device and the log-probability tables on the host, then scores X itself: decision_scores_ (float64 [n]),
        per_subspace_scores_, projection_features_, projection_weights_, bin_edges_, histograms_; with normalize also
        score_center_ / score_scale_.  The projections, edges and tables are the fitted state: X itself is not kept."""
        X = self._begin_fit(X)
        n, dev = X.shape[0], X.device
        S, k, B = self.plan.count, self.n_projections, self.n_bins
        if self._proj is None:  # they depend on the constructor's arguments alone: a second fit keeps them
            features, weights = loda_projections(self.plan.dims, k, self.seed)
            self.projection_features_, self.projection_weights_ = features, weights
            moff = np.concatenate([[0], np.cumsum([f.shape[1] for f in features])]).astype(np.int64)
            self._proj = (torch.as_tensor(np.concatenate([f.T.reshape(-1) for f in features]).astype(np.int32), device=dev),  # t-major
                          torch.as_tensor(np.concatenate([w.T.reshape(-1) for w in weights]), device=dev),
                          torch.as_tensor(moff, device=dev), k)
        keys = torch.empty(S, k, 2, dtype=torch.int64, device=dev)
        self.ops.hist_reset(keys=keys)
        for packed, rows, _, first, count, width in self._blocks(X):
            self.ops.loda_range(packed, rows, self._table, first, count, width, self._proj, keys)
        self._edges = torch.empty(S, k, B + 1, dtype=torch.float64, device=dev)
        self.ops.hist_edges(keys, B, self._edges)
        counts = torch.empty(S, k, B, dtype=torch.int32, device=dev)
        self.ops.hist_reset(counts=counts)
        for packed, rows, _, first, count, width in self._blocks(X):
            self.ops.loda_counts(packed, rows, self._table, first, count, width, self._proj, self._edges, counts)
        self.bin_edges_ = self._edges.cpu().numpy()
        self.histograms_ = counts.cpu().numpy().astype(np.int64)
        self._terms = torch.as_tensor(loda_term_table(self.histograms_, n), device=dev)
        scores, per = self._score(X, fitting=True)
        return self._publish(scores, per)


# ---- isolation forest: random trees over the subspaces -----------------------------------------------------------------
IFOREST_MAX_TREES = 1024  # VGAN_IFOREST_MAX_TREES
IFOREST_MAX_SAMPLES = 1024  # VGAN_IFOREST_MAX_SAMPLES: the sampled rows of a tree live in LDS
IFOREST_MAX_DIMS = 8192  # VGAN_IFOREST_MAX_DIMS: features of one subspace (a bit per feature and wave in LDS)
IFOREST_MAX_ROWS = (1 << 31) - 1
IFOREST_MAX_PLANE = 16  # VGAN_IFOREST_MAX_PLANE: the features of one oblique cut (n_dims)
IFOREST_AUTO_SAMPLES = 256  # max_samples="auto", sklearn's and pyod's default
_IFOREST_MAX_RANGE = 65535  # subspaces of one launch (a grid dimension)
EULER_GAMMA = 0.5772156649015329


def check_estimators(n_estimators):
    if not (_is_int(n_estimators) and 1 <= int(n_estimators) <= IFOREST_MAX_TREES):
        raise ValueError(f"n_estimators must be an integer between 1 and {IFOREST_MAX_TREES}, got {n_estimators!r}")
    return int(n_estimators)


def check_max_samples(max_samples):
    """ "auto" (256) or an integer between 2 and IFOREST_MAX_SAMPLES; fit takes min(max_samples, n)."""
    if isinstance(max_samples, str) and max_samples == "auto":
        return IFOREST_AUTO_SAMPLES
    if not (_is_int(max_samples) and 2 <= int(max_samples) <= IFOREST_MAX_SAMPLES):
        raise ValueError(f"max_samples must be 'auto' or an integer between 2 and {IFOREST_MAX_SAMPLES}, got {max_samples!r}")
    return int(max_samples)


def check_n_dims(n_dims):
    if not (_is_int(n_dims) and 1 <= int(n_dims) <= IFOREST_MAX_PLANE):
        raise ValueError(f"n_dims must be an integer between 1 and {IFOREST_MAX_PLANE}, got {n_dims!r}")
    return int(n_dims)


def check_seed(seed):
    if not (_is_int(seed) and 0 <= int(seed) < 1 << 64):
        raise ValueError(f"seed must be an integer in [0, 2^64), got {seed!r}")
    return int(seed)


def iforest_path_table(psi):
    """int64 [psi + 1]: cq[m] = rint(c(m) 2^32), c the average path length of an unsuccessful search in a binary search tree
    of m rows: 0 for m <= 1, 1 for m = 2, else 2 (ln(m - 1) + EULER_GAMMA) - 2 (m - 1) / m, in float64."""
    m = np.arange(psi + 1, dtype=np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        c = 2.0 * (np.log(m - 1.0) + EULER_GAMMA) - 2.0 * (m - 1.0) / m
    c[:2] = 0.0
    if psi >= 2:
        c[2] = 1.0
    return np.rint(c * 4294967296.0).astype(np.int64)


def iforest_chunks(n_subspaces, workspace_bytes):
    """(subspaces of a range, rows of a row chunk): the transient buffers of scoring hold an int64 sum and a float32 score
    per (subspace, row), 12 bytes.  All subspaces form one range and the rows are chunked while a row of every subspace
    fits; below that the chunks are single rows and the subspaces are split into ranges, down to one subspace each."""
    cells = max(1, int(workspace_bytes) // 12)
    count = min(int(n_subspaces), cells, _IFOREST_MAX_RANGE)
    return count, max(1, cells // count)


class SubspaceIForest(_SubspaceScorer):
    """Isolation forest per subspace (Liu, Ting, Zhou 2008; sklearn's ``IsolationForest``, pyod's ``IForest``), combined like
    the other detectors of this module: ``fit`` sets ``decision_scores_``, ``decision_function`` scores new rows; higher is
    more outlying.  Nothing n x n: ``fit`` touches max_samples rows per tree, scoring is a short walk per (row, tree).  It is
    invariant to a monotone rescaling of a feature.  There is no ``max_features`` (every feature of the subspace is a
    candidate at every node: the subspaces are the feature bagging) and no ``bootstrap`` (a tree's sample has no repeats).

    X is cast to float32.  n rows are given to ``fit``, 2 <= n <= 2^31 - 1; T = n_estimators (1 .. 1024); psi =
    ``max_samples_`` = min(max_samples, n), max_samples "auto" (256) or 2 .. 1024; seed in [0, 2^64); a subspace has at most
    IFOREST_MAX_DIMS (8192) features.

    Tree (s, t), s the given subspace index, has the stream id = s T + t.  Its sample is the psi rows feistel_perm(i, n,
    seed, id), i = 0 .. psi - 1 (the permutation of vgan_shuffle_index); only the set matters.  Nodes are heap-numbered: root
    1, children 2 i and 2 i + 1; the depth limit is L = ``depth_limit_`` = ceil(log2 psi), so a tree has N = 2^(L + 1) slots,
    slot 0 unused.  A node at depth e holding the row set R, m = |R|, is a leaf if m <= 1, or e == L, or no feature of F_s
    varies on R (a feature is constant on R when its float32 min equals its max, -0.0 taken as +0.0).  Otherwise, with c the
    number of varying features, the Philox4x32-10 words (w0, w1, ., .) of

        counter (node, 0, 0x49464F52, 0),  key k0 = lo32(seed) ^ lo32(id),  k1 = hi32(seed) ^ hi32(id) ^ 0x5bd1e995

    (the key convention of the noise stream) choose the split feature, the j-th varying feature in ascending feature
    order with j = (w0 c) >> 32 in integers (uniform over the varying features: sklearn's distribution), and the threshold:
    lo and hi the feature's min and max on R (-0.0 as +0.0), u = (w1 + 0.5) 2^-32 in float64, p = float32(lo + u (hi - lo)),
    the difference, the product and the sum three separately rounded float64 operations; if p >= hi then p = lo (sklearn's
    rule: both children are non-empty).  A row goes left iff x <= p, compared in float32.

    Path lengths are fixed-point, so that their sums are exact and free of any order: c(m) = 0 for m <= 1, c(2) = 1, else
    2 (ln(m - 1) + 0.5772156649015329) - 2 (m - 1) / m in float64 on the host; cq[m] = rint(c(m) 2^32) as int64 (a table the
    host uploads: the device computes no logarithm).  A row reaching a leaf of depth e and size m in tree t contributes
    (e << 32) + cq[m]; sum[s, i] is the int64 total over the T trees, and

        score[s, i] = float32(exp2(-(double(sum[s, i]) / double(T cq[psi]))))

    in (0, 1]: the paper's s(x, psi).  It equals minus sklearn's ``score_samples``; pyod's ``decision_scores_`` (sklearn's
    ``decision_function`` negated) differ from it by a constant per fit, sklearn's ``offset_``.  A subspace whose features are
    all constant scores exactly 0.5 everywhere.  ``fit`` scores the training rows through all trees, nothing excluded, so
    ``decision_function(X_train)`` equals ``decision_scores_`` bit for bit.

    All of the above depends on row sets only, never on a processing order: trees, sums and scores are bit-identical from
    run to run and for every workspace_bytes, which bounds the transient buffers of scoring (iforest_chunks), not the trees;
    the trees (8 bytes a slot: feature and threshold, or -1 and the leaf's size) are the fitted state, X is not kept.  NaN
    input leaves the results unspecified and neither faults nor hangs: every loop is bounded by L and psi.

    ``fit`` publishes, copied to the host on first use: ``tree_feature_`` int32 [S, T, N] (the split feature as a column of
    X, -1 a leaf, -2 an absent slot), ``tree_threshold_`` float32 [S, T, N] (0 where the slot is not internal) and
    ``tree_size_`` int32 [S, T, N] (the sample rows reaching the node, 0 where absent; those of an internal node are the sum
    of its leaves'); and ``max_samples_``, ``depth_limit_``.  normalize, combination, contamination, ``threshold_``,
    ``labels_``, ``predict``, ``predict_proba`` and return_per_subspace are the shared tail.  The definition above and its
    numpy restatement in tests/test_outlier_iforest_cpu.py (pinned there to sklearn's path lengths and scores) are what
    binds.  All of it runs in libvgan_hip.so (csrc/outlier_iforest.hip).

    **Oblique cuts, n_dims = q >= 2** (the extended isolation forest of Hariri, Carrasco Kind and Brunner, TKDE 2019, with
    the sparse hyperplanes of SCiForest, Liu, Ting, Zhou 2010).  Axis-parallel cuts leave "ghost" low-score regions where
    marginal modes cross: a row there stays inside every marginal range and is isolated late.  With ``n_dims`` = q, an
    integer 2 .. IFOREST_MAX_PLANE (16), every internal node cuts with a random hyperplane over at most q features of the
    subspace; n_dims = 1 (the default) is everything above, the same launches and the same bits.  For q >= 2:

    *Candidates.*  The candidates of subspace s are the features of F_s whose column maximum exceeds the column minimum over
    the fitted rows (float32, -0.0 as +0.0), ascending: ``candidate_features_`` (a list of int32 arrays).  c_s is their
    number, m_s = min(q, c_s).
    *Trees.*  Tree (s, t), its stream id s T + t, its sample, heap numbering, L, the key, cq and the score are those above.
    *Leaves.*  A node at depth e with row set R is a leaf if |R| <= 1, or e == L, or c_s == 0, or all four attempts fail.
    *Attempts.*  Attempt a = 0, 1, 2, 3 of a node uses the Philox4x32-10 blocks at counter (node, 32 a + b, 0x45494600, 0)
    under the tree's key.
    *Positions.*  For i = 0 .. m_s - 1 the word is word i & 3 of block b = 1 + (i >> 2); j = (word (c_s - i)) >> 32 in
    integers; walking the positions already chosen in ascending order, j grows by one for each that is <= j.  The result is
    position i (an index into the candidates): uniform over the m_s-subsets, distinct by construction.
    *Weights.*  For i = 0 .. m_s - 1, t the integer sum of the four words of block b = 5 + i, w_i = float32((double(t) -
    8589934590.0) 2^-32): exact up to the one rounding, Irwin-Hall of four (mean 0, variance 1/3).  Weight i belongs to
    position i.
    *Projection.*  acc = 0.0 in float64; for the chosen positions in ascending order acc = acc + double(w) double(x), the
    product exact, the sum rounded once per term, no fused multiply-add, x with -0.0 as +0.0; zf = float32(acc).
    *Threshold.*  lo and hi are the min and max of zf over R; lo == hi fails the attempt.  Otherwise u = (w1 of block 0 of
    the attempt + 0.5) 2^-32, p = float32(lo + u (hi - lo)) in three separately rounded float64 operations, p >= hi replaced
    by lo; a row goes left iff zf <= p in float32, and both children are non-empty.
    *Score.*  A leaf contributes (e << 32) + cq[size] as above; a subspace with c_s = 0 has root leaves and scores exactly
    0.5; ``decision_function(X_train)`` equals ``decision_scores_`` bit for bit; every loop is bounded by L, psi, 4 and 16.

    Published for q >= 2, copied to the host on first use: ``plane_features_`` int32 [S, T, N, q] (columns of X, ascending,
    -1 in the unused places and everywhere outside internal nodes), ``plane_weights_`` float32 [S, T, N, q] (0 where
    unused), ``tree_attempt_`` int32 [S, T, N] (the successful attempt, -1 a leaf, -2 absent), ``tree_threshold_``,
    ``tree_size_``, and ``tree_feature_`` = plane_features_[..., 0] for an internal node (-1 a leaf, -2 absent).  The fitted
    state is 8 + 8 q bytes a slot.  The restatement is tests/test_outlier_iforest_oblique_cpu.py.

    Not built: ``n_dims="full"`` (a hyperplane over all features of a wide subspace would make the fitted state tens of
    megabytes a subspace, or need the weights regenerated at every step of the walk); Hariri's intercept drawn in the
    bounding box (it can leave a child empty); SCiForest's split-selection criterion."""

    _host_trees = None

    def __init__(self, subspaces, proba, n_estimators=100, max_samples="auto", seed=0, n_dims=1, workspace_bytes=DEFAULT_WORKSPACE_BYTES,
                 normalize=None, combination="sum", contamination=0.1):
        self.n_estimators = check_estimators(n_estimators)
        self.max_samples = max_samples
        self._max_samples = check_max_samples(max_samples)
        self.seed = check_seed(seed)
        self.n_dims = check_n_dims(n_dims)
        # no distance engine here: "exact" for every subspace keeps the processing order the given order
        self._configure(subspaces, proba, "exact", workspace_bytes, normalize, combination, contamination)
        del self.engine
        if int(self.plan.dims.max()) > IFOREST_MAX_DIMS:
            raise ValueError(f"a subspace has {int(self.plan.dims.max())} features, SubspaceIForest takes at most {IFOREST_MAX_DIMS}")

    def _check_fit_rows(self, n):
        if not 2 <= n <= IFOREST_MAX_ROWS:
            raise ValueError(f"SubspaceIForest fit needs between 2 and {IFOREST_MAX_ROWS} rows, got {n}")

    def _ranges(self):
        count, rows = iforest_chunks(self.plan.count, self.workspace_bytes)
        return [(first, min(count, self.plan.count - first)) for first in range(0, self.plan.count, count)], rows

    def path_sums(self, X):
        """int64 [S, n]: the fixed-point path-length sums of the rows of X over the trees of every subspace."""
        self._require_fit()
        X = _device_matrix(X, self.plan.d)
        return self._sums(X, None).cpu().numpy()

    def _sums(self, X, per):
        """Walks X through the trees range by range and row chunk by row chunk; per None: returns the int64 sums [S, nq],
        otherwise fills the float32 scores per [S, nq]."""
        nq = X.shape[0]
        ranges, rows = self._ranges()
        rows = min(rows, nq)
        out = torch.empty(self.plan.count, nq, dtype=torch.int64, device=X.device) if per is None else None
        sums = torch.empty(ranges[0][1] * rows, dtype=torch.int64, device=X.device)
        for first, count in ranges:
            for r0 in range(0, nq, rows):
                r1 = min(r0 + rows, nq)
                if self.n_dims == 1:
                    self.ops.iforest_path_sums(X[r0:r1], self._trees, first, count, self.max_samples_, self.depth_limit_, self._cq, sums)
                else:
                    self.ops.iforest_path_sums_oblique(X[r0:r1], self._trees, *self._planes, first, count, self.max_samples_,
                                                       self.depth_limit_, self._cq, sums)
                if per is None:
                    out[first:first + count, r0:r1] = sums[:count * (r1 - r0)].view(count, r1 - r0)
                else:
                    self.ops.iforest_scores(sums, count, r1 - r0, self._denom, per[first:first + count, r0:r1])
        return out

    def _score(self, X, fitting):
        per = torch.empty(self.plan.count, X.shape[0], dtype=torch.float32, device=X.device)
        self._sums(X, per)
        return self._combine(per, fitting), per

    def _trees_on_host(self):
        self._require_fit()
        if self._host_trees is None:
            nodes = self._trees.cpu().numpy()
            feature = np.ascontiguousarray(nodes[..., 0])
            word = np.ascontiguousarray(nodes[..., 1])
            planes = ()
            if getattr(self, "_planes", None) is not None:  # oblique: word 0 is the attempt, the feature the plane's first column
                planes = (feature, self._planes[0].cpu().numpy(), self._planes[1].cpu().numpy())
                feature = np.where(feature >= 0, planes[1][..., 0], feature).astype(np.int32)
            threshold = np.where(feature >= 0, word.view(np.float32), np.float32(0.0))
            size = np.where(feature == -1, word, 0).astype(np.int32)
            for e in range(self.depth_limit_ - 1, -1, -1):  # an internal node holds what its children hold
                at = np.arange(1 << e, 2 << e)
                inner = feature[..., at] >= 0
                size[..., at] = np.where(inner, size[..., 2 * at] + size[..., 2 * at + 1], size[..., at])
            self._host_trees = (feature, threshold, size) + planes
        return self._host_trees

    def _planes_on_host(self):
        self._require_fit()
        if self.n_dims == 1:
            raise AttributeError("tree_attempt_, plane_features_ and plane_weights_ belong to oblique cuts (n_dims >= 2)")
        return self._trees_on_host()[3:]

    @property
    def tree_attempt_(self):
        """int32 [S, T, N], n_dims >= 2: the successful attempt (0 .. 3) of an internal node, -1 a leaf, -2 an absent slot."""
        return self._planes_on_host()[0]

    @property
    def plane_features_(self):
        """int32 [S, T, N, n_dims], n_dims >= 2: the columns of X of every internal node's hyperplane, ascending; -1 elsewhere."""
        return self._planes_on_host()[1]

    @property
    def plane_weights_(self):
        """float32 [S, T, N, n_dims], n_dims >= 2: the weights of plane_features_, 0 where unused."""
        return self._planes_on_host()[2]

    @property
    def candidate_features_(self):
        """list of int32 arrays, n_dims >= 2: the features of every subspace that vary over the fitted rows, ascending."""
        self._require_fit()
        if self.n_dims == 1:
            raise AttributeError("candidate_features_ belongs to oblique cuts (n_dims >= 2)")
        return self._candidates

    @property
    def tree_feature_(self):
        """int32 [S, T, N]: the split feature of every heap slot as a column of X, -1 for a leaf, -2 for an absent slot."""
        return self._trees_on_host()[0]

    @property
    def tree_threshold_(self):
        """float32 [S, T, N]: the threshold of every internal node (a row goes left iff x <= threshold), 0 elsewhere."""
        return self._trees_on_host()[1]

    @property
    def tree_size_(self):
        """int32 [S, T, N]: the sample rows reaching every node, 0 where the slot is absent."""
        return self._trees_on_host()[2]

    def fit(self, X, y=None):
        """Builds the T trees of every subspace on their samples of X, then scores X itself through them: decision_scores_
        (float64 [n]), per_subspace_scores_, max_samples_, depth_limit_ and, on first use, tree_feature_ / tree_threshold_ /
        tree_size_; with normalize also score_center_ / score_scale_.  With n_dims >= 2 the candidates come first
        (candidate_features_), the trees are oblique, and tree_attempt_ / plane_features_ / plane_weights_ are published
        too.  The trees (and planes) are the fitted state: X itself is not kept."""
        X = self._begin_fit(X)
        n = X.shape[0]
        psi = min(self._max_samples, n)
        self.max_samples_, self.depth_limit_, self._host_trees = psi, (psi - 1).bit_length(), None
        cq = iforest_path_table(psi)
        self._cq = torch.as_tensor(cq, device=X.device)
        self._denom = self.n_estimators * int(cq[psi])
        self._trees = torch.empty(self.plan.count, self.n_estimators, 2 << self.depth_limit_, 2, dtype=torch.int32, device=X.device)
        self._planes = None
        if self.n_dims > 1:
            self._fitted = False
            self._build_oblique(X, psi)
        else:
            for first, count in self._ranges()[0]:
                self.ops.iforest_build(X, self._table, first, count, int(self.plan.dims[first:first + count].max()), psi,
                                       self.depth_limit_, self.seed, self._trees)
        scores, per = self._score(X, fitting=True)
        return self._publish(scores, per)


    def _build_oblique(self, X, psi):
        """The candidates of every subspace from the column ranges of X (SubspaceRSHash.fit's rule), then the oblique trees
        and their planes, range by range."""
        d, dev, S = X.shape[1], X.device, self.plan.count
        keys = torch.empty(d, 2, dtype=torch.int64, device=dev)
        self.ops.hist_column_range(X, keys)  # keys of the float64 images of the float32 min and max, -0.0 as +0.0
        k = keys.cpu().numpy().view(np.uint64)
        lo_hi = np.ascontiguousarray(np.where(k >> np.uint64(63), k & np.uint64(0x7FFFFFFFFFFFFFFF), ~k)).view(np.float64)
        varying = lo_hi[:, 1] > lo_hi[:, 0]
        feats = [self.plan.feat[self.plan.feat_off[z]:self.plan.feat_off[z + 1]] for z in range(S)]
        self._candidates = [f[varying[f]].astype(np.int32) for f in feats]
        off = np.zeros(S + 1, np.int32)
        np.cumsum([len(c) for c in self._candidates], out=off[1:])
        cand = np.concatenate(self._candidates + [np.zeros(1, np.int32)])  # never empty: the entry rejects a null pointer
        shape = tuple(self._trees.shape[:3]) + (self.n_dims,)
        self._planes = (torch.empty(shape, dtype=torch.int32, device=dev), torch.empty(shape, dtype=torch.float32, device=dev))
        cand, off = torch.as_tensor(cand, device=dev), torch.as_tensor(off, device=dev)
        for first, count in self._ranges()[0]:
            self.ops.iforest_build_oblique(X, cand, off, first, count, psi, self.depth_limit_, self.seed, self._trees, *self._planes)


# ---- RS-Hash: counts of randomly shifted grid cells over the subspaces --------------------------------------------------
RSHASH_MAX_COMPONENTS = 1024  # VGAN_RSHASH_MAX_COMPONENTS
RSHASH_MAX_SAMPLES = 4096  # VGAN_RSHASH_MAX_SAMPLES: the sampled rows and their keys live in LDS
RSHASH_MAX_DIMS = 12  # VGAN_RSHASH_MAX_DIMS: r at s = 4096
RSHASH_MAX_ROWS = 1 << 24  # VGAN_RSHASH_MAX_ROWS
RSHASH_AUTO_SAMPLES = 1000  # max_samples="auto", the paper's s


def check_rshash_estimators(n_estimators):
    if not (_is_int(n_estimators) and 1 <= int(n_estimators) <= RSHASH_MAX_COMPONENTS):
        raise ValueError(f"n_estimators must be an integer between 1 and {RSHASH_MAX_COMPONENTS}, got {n_estimators!r}")
    return int(n_estimators)


def check_rshash_samples(max_samples):
    """ "auto" (1000) or an integer between 2 and RSHASH_MAX_SAMPLES; fit takes min(max_samples, n)."""
    if isinstance(max_samples, str) and max_samples == "auto":
        return RSHASH_AUTO_SAMPLES
    if not (_is_int(max_samples) and 2 <= int(max_samples) <= RSHASH_MAX_SAMPLES):
        raise ValueError(f"max_samples must be 'auto' or an integer between 2 and {RSHASH_MAX_SAMPLES}, got {max_samples!r}")
    return int(max_samples)


def rshash_log_table(s):
    """int64 [s + 2]: table[c] = rint(log2(c) 2^32) in float64, table[0] = 0 (no count is 0)."""
    c = np.arange(s + 2, dtype=np.float64)
    c[0] = 1.0
    return np.rint(np.log2(c) * 4294967296.0).astype(np.int64)


def rshash_components(candidate_counts, n_estimators, s, seed):
    """(grid_width float64 [S, T], dims int32 [S, T], positions int32 [S, T, 12], shifts float64 [S, T, 12]): the draws of
    every component, from ONE rng = numpy.random.default_rng(seed), subspace by subspace (c_z = candidate_counts[z] candidate
    features), then component by component, and within a component in this order:

        f = lo + (hi - lo) * rng.random(), lo = 1 / sqrt(s), hi = 1 - lo (as written, also where s < 4 inverts the interval)
        L = log(s) / log(max(2, 1 / f)), r_lo = floor(1 + L / 2), r_hi = max(r_lo, floor(L))
        r = min(rng.integers(r_lo, r_hi + 1), c_z)
        positions = sort(rng.choice(c_z, r, replace=False))   (positions among the candidates in ascending feature order)
        alpha = f * rng.random(r)

    positions is padded with -1 and shifts with 0 past r.  A subspace with c_z = 0 draws nothing: its rows are f = 0, r = 0.
    r never exceeds RSHASH_MAX_DIMS (12) for s <= 4096, and (floor(1 / f) + 4)^r stays below 2^63 (asserted)."""
    rng = np.random.default_rng(seed)
    T, s = int(n_estimators), int(s)
    counts = np.asarray(candidate_counts, dtype=np.int64).reshape(-1)
    S = len(counts)
    width, dims = np.zeros((S, T), np.float64), np.zeros((S, T), np.int32)
    positions, shifts = np.full((S, T, RSHASH_MAX_DIMS), -1, np.int32), np.zeros((S, T, RSHASH_MAX_DIMS), np.float64)
    lo = 1.0 / math.sqrt(s)
    hi = 1.0 - lo
    for z, c in enumerate(counts):
        if c == 0:
            continue
        for t in range(T):
            f = lo + (hi - lo) * rng.random()
            L = math.log(s) / math.log(max(2.0, 1.0 / f))
            r_lo = math.floor(1.0 + L / 2.0)
            r_hi = max(r_lo, math.floor(L))
            r = min(int(rng.integers(r_lo, r_hi + 1)), int(c))
            assert 1 <= r <= RSHASH_MAX_DIMS and (math.floor(1.0 / f) + 4) ** r < 1 << 63
            width[z, t], dims[z, t] = f, r
            positions[z, t, :r] = np.sort(rng.choice(int(c), r, replace=False))
            shifts[z, t, :r] = f * rng.random(r)
    return width, dims, positions, shifts


class SubspaceRSHash(_SubspaceScorer):
    """RS-Hash per subspace (Sathe and Aggarwal, "Subspace Outlier Detection in Linear Time with Randomized Hashing", ICDM
    2016; pyod's ``RSHash`` is not built on it), combined like the other detectors of this module: ``fit`` sets
    ``decision_scores_``, ``decision_function`` scores new rows; higher is more outlying.  Each of T components per subspace
    is a randomly shifted grid of width f over r of the subspace's features and holds how many of s sampled rows fall into
    each occupied cell; a row's score falls with the log of the count of its own cell.  An r-dimensional cell is a joint
    statement about r features, so the score sees a broken correlation that no single feature shows; yet there is no sweep
    over pairs of rows, no tree, no moment and no training: linear in n.  It is itself a subspace method and sits one level
    below the model's subspaces, the way LODA's sparse projections do.  Neither pyod nor the authors' code was at hand:
    the rules are the paper's as remembered, made definite here, so this definition and its numpy restatement in
    tests/test_outlier_rshash_cpu.py are what binds.

    X is cast to float32.  n rows are given to ``fit``, 2 <= n <= 2^24; T = n_estimators (1 .. 1024); s = ``max_samples_`` =
    min(max_samples, n), max_samples "auto" (1000: the paper's) or 2 .. 4096; seed in [0, 2^64).

    Candidate features.  The candidates of subspace z are the features of F_z whose maximum exceeds their minimum over all n
    fitted rows (a range pass on the device), c_z their number: a constant pixel uses up no grid dimension.  A subspace with
    c_z = 0 has no component and scores exactly 0 for every row.

    Draws.  rshash_components(candidate_counts, T, s, seed) draws on the host, from one numpy.random.default_rng(seed),
    subspace by subspace in the given order and component by component, in this order: f = lo + (hi - lo) rng.random() with
    lo = 1 / sqrt(s), hi = 1 - lo; with L = log(s) / log(max(2, 1 / f)), r_lo = floor(1 + L / 2), r_hi = max(r_lo, floor(L)):
    r = min(rng.integers(r_lo, r_hi + 1), c_z); positions = sort(rng.choice(c_z, r, replace=False)) among the candidates in
    ascending feature order; alpha = f rng.random(r).  r <= 12.  The draws are keyed by the subspace's position in the
    given set, as SubspaceDIF's nets are: a subspace fitted alone differs from the same subspace at position 3, and so
    does the same subspace behind others whose candidate counts changed.

    Sample.  Component (z, t) has the stream id = z T + t; its sample is the set of rows feistel_perm(i, n, seed, id), i < s
    (the permutation of vgan_shuffle_index: the sampler of SubspaceIForest and SubspaceINNE).

    Cells.  For each chosen feature j: mn_j and mx_j are the exact float32 minimum and maximum over the sample (-0.0 as
    +0.0), w_j = mx_j - mn_j, x' = (x - mn_j) / w_j if w_j > 0, else 0; y = floor((x' + alpha_j) / f), clamped in float64 to
    [-1, floor(1 / f) + 2] before the conversion (new rows may lie anywhere; NaN goes to -1); digit_j = y + 1.  The
    arithmetic is float64 on the float32 values, every operation rounded on its own (no fused multiply-add): a plain numpy
    loop gives the same integers.  R = floor(1 / f) + 4, and the cell key is the uint64 sum_j digit_j R^j, j over the chosen
    features in ascending order (below 2^32 within the limits above).  Sampled rows produce neither digit 0 nor digit
    R - 1, so cells with those digits always count 0.

    Score.  c_t is the count of the row's cell in component t, 0 if no sampled row fell into it.  At ``fit`` c_t gets plus 1
    unless the row is in the sample of component t; in ``decision_function`` it always gets plus 1 (the paper's rule), so
    c_t >= 1.  table = rshash_log_table(s) is int64 [s + 2], table[c] = rint(log2(c) 2^32), formed on the host in float64 and
    uploaded (the device computes no logarithm); sum[z, i] = sum_t table[c_t] in int64 (a subspace with c_z = 0 holds
    T table[s + 1]) and

        score[z, i] = float32(1 - double(sum[z, i]) / (double(T) double(table[s + 1])))

    in [0, 1], 1 for a row alone in its cell in every component.  It is scale free, so like LOF, COF, iNNE and SOS it sums
    across subspaces of mixed width without ``normalize``.  Because sampled rows count themselves at ``fit``,
    ``decision_function(X_train)`` is NOT ``decision_scores_`` (as with SubspaceECOD and SubspaceSOS): it exceeds every
    count of a sampled row by one.

    Keys, counts, sums and scores are integers up to the final division: bit-identical from run to run, for every
    workspace_bytes (which bounds the transient sums and scores of scoring, iforest_chunks' rule of 12 bytes per subspace
    and row; not the state, not the sorted samples ``fit`` holds while it scores, 4 T s bytes a subspace, and not the
    column-major copy of the scored rows, 4 d bytes a row) and for every split of the query rows.  The fitted state takes 12 T s bytes a subspace; X is not kept.  NaN input leaves the results
    unspecified and neither faults nor hangs.

    ``fit`` publishes, copied to the host on first use: ``cell_key_`` uint64 [S, T, s] (the distinct keys of a component's
    sampled rows, ascending, padded with 2^64 - 1), ``cell_count_`` int32 [S, T, s] (padded with 0), ``n_cells_`` int32
    [S, T], ``sample_min_`` / ``sample_max_`` float32 [S, T, 12] (0 past r) and ``cell_sums_`` int64 [S, n] (the sums of the
    fitted rows; ``cell_sums(X)`` gives those of new rows); and the host tables ``candidate_features_`` (a list of S int
    arrays), ``component_features_`` int32 [S, T, 12] (columns of X, -1 past r), ``component_shift_`` float64 [S, T, 12],
    ``grid_width_`` float64 [S, T], ``component_dims_`` int32 [S, T]; and ``max_samples_``.  normalize, combination,
    contamination, ``threshold_``, ``labels_``, ``predict``, ``predict_proba`` and return_per_subspace are the shared tail.
    All of it runs in libvgan_hip.so (csrc/outlier_rshash.hip; the range pass is csrc/outlier_hist.hip's)."""

    _host_state = None
    _draws = None  # (key, the host draws): a refit with the same candidate counts and sample size keeps them
    # cell sums gather X[row, f] at a fixed f per instruction: from a column-major copy of the query rows the 64 loads of a
    # wave are neighbouring addresses; False reads X as given through L2 (measured: 7.8 times slower at n = 50 000)
    _column_major = True

    def __init__(self, subspaces, proba, n_estimators=100, max_samples="auto", seed=0, workspace_bytes=DEFAULT_WORKSPACE_BYTES,
                 normalize=None, combination="sum", contamination=0.1):
        self.n_estimators = check_rshash_estimators(n_estimators)
        self.max_samples = max_samples
        self._max_samples = check_rshash_samples(max_samples)
        self.seed = check_seed(seed)
        # no distance engine here: "exact" for every subspace keeps the processing order the given order
        self._configure(subspaces, proba, "exact", workspace_bytes, normalize, combination, contamination)
        del self.engine

    def _check_fit_rows(self, n):
        if not 2 <= n <= RSHASH_MAX_ROWS:
            raise ValueError(f"SubspaceRSHash fit needs between 2 and {RSHASH_MAX_ROWS} rows, got {n}")

    def _ranges(self):
        count, rows = iforest_chunks(self.plan.count, self.workspace_bytes)
        return [(first, min(count, self.plan.count - first)) for first in range(0, self.plan.count, count)], rows

    def cell_sums(self, X):
        """int64 [S, n]: the fixed-point log-count sums of the rows of X, scored as new rows, over every subspace."""
        self._require_fit()
        X = _device_matrix(X, self.plan.d)
        return self._sums(X, None, None).cpu().numpy()

    def _sums(self, X, per, samples):
        """Looks the rows of X up range by range and row chunk by row chunk; samples: the fit's sorted samples (X is then the
        fitted matrix), None for new rows.  per None: returns the int64 sums [S, nq]; otherwise fills the float32 scores per
        [S, nq] and returns the sums only at fit."""
        nq = X.shape[0]
        ranges, rows = self._ranges()
        rows = min(rows, nq)
        keep = per is None or samples is not None
        out = torch.empty(self.plan.count, nq, dtype=torch.int64, device=X.device) if keep else None
        sums = torch.empty(ranges[0][1] * rows, dtype=torch.int64, device=X.device)
        Xt = X.t().contiguous() if self._column_major else None
        for first, count in ranges:
            for r0 in range(0, nq, rows):
                r1 = min(r0 + rows, nq)
                Xq = X[r0:r1] if Xt is None else Xt[:, r0:r1]
                self.ops.rshash_cell_sums(Xq, Xt is not None, r0, first, count, self._comp, self._state, samples, self._log_table, sums)
                if keep:
                    out[first:first + count, r0:r1] = sums[:count * (r1 - r0)].view(count, r1 - r0)
                if per is not None:
                    self.ops.rshash_scores(sums, count, r1 - r0, self._denom, per[first:first + count, r0:r1])
        return out

    def _score(self, X, fitting, samples=None):
        per = torch.empty(self.plan.count, X.shape[0], dtype=torch.float32, device=X.device)
        sums = self._sums(X, per, samples)
        if fitting:
            self._fit_sums = sums
        return self._combine(per, fitting), per

    def _on_host(self):
        self._require_fit()
        if self._host_state is None:
            key, cnt, cells, lo, hi = (t.cpu().numpy() for t in self._state)
            self._host_state = (key.view(np.uint64), cnt, cells, lo, hi, self._fit_sums.cpu().numpy())
        return self._host_state

    @property
    def cell_key_(self):
        """uint64 [S, T, s]: the distinct cell keys of every component's sampled rows, ascending, padded with 2^64 - 1."""
        return self._on_host()[0]

    @property
    def cell_count_(self):
        """int32 [S, T, s]: how many sampled rows fell into the cell of cell_key_ at the same place, padded with 0."""
        return self._on_host()[1]

    @property
    def n_cells_(self):
        """int32 [S, T]: the occupied cells of every component."""
        return self._on_host()[2]

    @property
    def sample_min_(self):
        """float32 [S, T, 12]: the minimum of every chosen feature over the component's sample, 0 past r."""
        return self._on_host()[3]

    @property
    def sample_max_(self):
        """float32 [S, T, 12]: the maximum of every chosen feature over the component's sample, 0 past r."""
        return self._on_host()[4]

    @property
    def cell_sums_(self):
        """int64 [S, n]: sum_t table[c_t] of the fitted rows, sampled rows not counting themselves twice."""
        return self._on_host()[5]

    def fit(self, X, y=None):
        """Takes the column ranges of X, draws the components on the host, counts the cells of every component's sample on
        the device and scores X itself: decision_scores_ (float64 [n]), per_subspace_scores_, max_samples_, the host tables
        of the draws and, on first use, cell_key_ / cell_count_ / n_cells_ / sample_min_ / sample_max_ / cell_sums_; with
        normalize also score_center_ / score_scale_.  The cells are the fitted state: X itself is not kept."""
        X = self._begin_fit(X)
        n, d = X.shape
        dev = X.device
        S, T = self.plan.count, self.n_estimators
        s = min(self._max_samples, n)
        self.max_samples_, self._host_state, self._fitted = s, None, False
        keys = torch.empty(d, 2, dtype=torch.int64, device=dev)
        self.ops.hist_column_range(X, keys)  # keys of the float64 images of the float32 min and max, -0.0 as +0.0
        k = keys.cpu().numpy().view(np.uint64)
        lo_hi = np.ascontiguousarray(np.where(k >> np.uint64(63), k & np.uint64(0x7FFFFFFFFFFFFFFF), ~k)).view(np.float64)
        varying = lo_hi[:, 1] > lo_hi[:, 0]
        feats = [self.plan.feat[self.plan.feat_off[z]:self.plan.feat_off[z + 1]] for z in range(S)]
        self.candidate_features_ = [f[varying[f]].astype(np.int32) for f in feats]
        key = (tuple(len(c) for c in self.candidate_features_), T, s, self.seed)
        if self._draws is None or self._draws[0] != key:
            self._draws = (key, rshash_components(key[0], T, s, self.seed))
        width, dims, positions, shifts = self._draws[1]
        columns = np.full((S, T, RSHASH_MAX_DIMS), -1, np.int32)
        for z, cand in enumerate(self.candidate_features_):
            if len(cand):
                columns[z] = np.where(positions[z] >= 0, cand[np.maximum(positions[z], 0)], -1)
        self.grid_width_, self.component_dims_, self.component_features_, self.component_shift_ = width, dims, columns, shifts
        self._comp = tuple(torch.as_tensor(a, device=dev) for a in (dims, columns, shifts, width))
        table = rshash_log_table(s)
        self._log_table = torch.as_tensor(table, device=dev)
        self._denom = T * int(table[s + 1])
        self._state = (torch.empty(S, T, s, dtype=torch.int64, device=dev), torch.empty(S, T, s, dtype=torch.int32, device=dev),
                       torch.empty(S, T, dtype=torch.int32, device=dev), torch.empty(S, T, RSHASH_MAX_DIMS, dtype=torch.float32, device=dev),
                       torch.empty(S, T, RSHASH_MAX_DIMS, dtype=torch.float32, device=dev))
        samples = torch.empty(S, T, s, dtype=torch.int32, device=dev)
        for first, count in self._ranges()[0]:
            self.ops.rshash_build(X, first, count, self.seed, self._comp, self._state, samples)
        scores, per = self._score(X, True, samples)
        return self._publish(scores, per)


# ---- iNNE: isolation by nearest-neighbour ensembles over the subspaces ---------------------------------------------------
INNE_MAX_ESTIMATORS = 1024  # VGAN_INNE_MAX_ESTIMATORS
INNE_MAX_SAMPLES = 1024  # VGAN_INNE_MAX_SAMPLES: the centres of an estimator live in LDS
INNE_MAX_DIMS = 8192  # VGAN_INNE_MAX_DIMS: features of one subspace
INNE_MAX_ROWS = (1 << 31) - 1
INNE_AUTO_SAMPLES = 8  # max_samples="auto", pyod's default
INNE_RATIOS = {"squared": 0, "distance": 1}  # VGAN_INNE_RATIO_*
INNE_STATE_BYTES = 24  # per centre: int32 row, float64 r2, int32 nn, float64 rho
_INNE_MAX_RANGE = 65535  # subspaces of one launch (a grid dimension)


def check_inne_samples(max_samples):
    """ "auto" (8) or an integer between 2 and INNE_MAX_SAMPLES; fit takes min(max_samples, n)."""
    if isinstance(max_samples, str) and max_samples == "auto":
        return INNE_AUTO_SAMPLES
    if not (_is_int(max_samples) and 2 <= int(max_samples) <= INNE_MAX_SAMPLES):
        raise ValueError(f"max_samples must be 'auto' or an integer between 2 and {INNE_MAX_SAMPLES}, got {max_samples!r}")
    return int(max_samples)


def check_inne_ratio(ratio):
    if not (isinstance(ratio, str) and ratio in INNE_RATIOS):
        raise ValueError(f"ratio must be 'squared' or 'distance', got {ratio!r}")
    return ratio


class SubspaceINNE(_SubspaceScorer):
    """Isolation by nearest-neighbour ensembles per subspace (iNNE: Bandaragoda, Ting, Albrecht, Liu, Wells 2018; pyod's
    ``INNE``), combined like the other detectors of this module: ``fit`` sets ``decision_scores_``, ``decision_function``
    scores new rows; higher is more outlying.  Where the isolation forest cuts along single features with a global score,
    iNNE isolates with hyperspheres around a few sampled rows and compares the radius of the sphere that catches a row with
    the radius of that sphere's own nearest neighbour: the score is local and invariant to a rotation of the subspace.  It
    is scale free in [0, 1], so like LOF and COF it sums across subspaces of mixed width without ``normalize``.  ``fit``
    touches T psi^2 pairs of rows per subspace, scoring n T psi.  pyod was not at hand: the rules below are the paper's
    and pyod's as their source is remembered here, not pinned against pyod, so the definition below and its numpy
    restatement in tests/test_outlier_inne_cpu.py are what binds.  Not built: pyod's contamination-shifted sign
    conventions, and ``max_samples`` as a fraction of n.

    X is cast to float32.  n rows are given to ``fit``, 2 <= n <= 2^31 - 1; T = n_estimators (1 .. 1024, default 200:
    pyod's); psi = ``max_samples_`` = min(max_samples, n), max_samples "auto" (8: pyod's) or 2 .. 1024; seed in [0, 2^64); a
    subspace has at most INNE_MAX_DIMS (8192) features.

    Sample.  Estimator (s, t), s the given subspace index, has the stream id = s T + t.  Its centres are the rows c_j =
    feistel_perm(j, n, seed, id), j = 0 .. psi - 1, in that order (the permutation of vgan_shuffle_index, as
    SubspaceIForest uses it); the position j breaks ties below, so the order matters and not only the set.

    Squared distance.  d2(a, b) runs over the features of F_s in ascending order with acc = 0.0 in float64; per feature
    diff = double(a_f) - double(b_f), p = diff * diff, acc = acc + p: three separately rounded operations, no fused
    multiply-add.  Always differences per feature, never |a|^2 + |b|^2 - 2 <a, b>.

    Radius and nearest centre.  For centre j, nn_j is the position i != j with the smallest (d2(c_j, c_i), i), and r2_j =
    d2(c_j, c_nn_j).  Comparisons are on d2, never on square roots.

    Ratio.  With eps = 2^-52, ``ratio="squared"`` (default; pyod's arithmetic as remembered): rho_j = 1.0 - (r2[nn_j] + eps)
    / (r2_j + eps); ``ratio="distance"`` (the paper's): the same with sqrt(r2) in place of r2.  Float64, each operation
    rounded on its own.  r2[nn_j] <= r2_j always, so rho is in [0, 1].

    Isolation score of a row x in estimator (s, t).  Among the centres with d2(x, c_j) <= r2_j (x is covered), the one with
    the smallest (r2_j, j) gives iso = rho_j; if no centre covers x, iso = 1.0.

    Score.  score[s, i] = float32(sum_t iso_t / double(T)): the sum in float64 with t ascending, one division, one rounding
    to float32; in [0, 1].  ``fit`` scores the training rows through all estimators with nothing excluded (as pyod does), so
    ``decision_function(X_train)`` equals ``decision_scores_`` bit for bit.

    Consequences.  A subspace of constant features has every r2 = 0 and every row covered, rho = 1 - eps / eps = 0: it
    scores exactly 0.  A row that coincides with a centre whose r2 is 0 is covered by it.  A row covered by nothing in any
    estimator scores exactly 1.  NaN input leaves the results unspecified and neither faults nor hangs: every loop is
    bounded by psi, T and d_s, and a false comparison means "not covered".

    Fitted state.  X stays resident, as for the neighbour detectors: the centres are read from it by row index.  Beside it
    an estimator keeps 24 bytes per centre (int32 row, float64 r2, int32 nn, float64 rho): 24 T psi bytes per subspace,
    38 400 with the defaults.  ``fit`` publishes, in the given subspace order and copied to the host on first use:
    ``center_rows_`` int32 [S, T, psi], ``radius_sq_`` float64 [S, T, psi], ``center_nn_`` int32 [S, T, psi] (positions),
    ``isolation_ratio_`` float64 [S, T, psi]; and ``max_samples_``.  normalize, combination, contamination,
    ``threshold_``, ``labels_``, ``predict``, ``predict_proba`` and return_per_subspace are the shared tail.

    Nothing above depends on a processing order: the state and the scores are bit-identical from run to run.  Scoring needs
    no transient buffer beside the [S, n] score matrix every detector returns, so ``workspace_bytes`` (kept for the shared
    constructor tail) bounds nothing here and changes no result.  All of it runs in libvgan_hip.so (csrc/outlier_inne.hip)."""

    _host_state = None

    def __init__(self, subspaces, proba, n_estimators=200, max_samples="auto", ratio="squared", seed=0,
                 workspace_bytes=DEFAULT_WORKSPACE_BYTES, normalize=None, combination="sum", contamination=0.1):
        self.n_estimators = check_estimators(n_estimators)
        self.max_samples = max_samples
        self._max_samples = check_inne_samples(max_samples)
        self.ratio = check_inne_ratio(ratio)
        self.seed = check_seed(seed)
        # no distance engine here: "exact" for every subspace keeps the processing order the given order
        self._configure(subspaces, proba, "exact", workspace_bytes, normalize, combination, contamination)
        del self.engine
        if int(self.plan.dims.max()) > INNE_MAX_DIMS:
            raise ValueError(f"a subspace has {int(self.plan.dims.max())} features, SubspaceINNE takes at most {INNE_MAX_DIMS}")

    def _check_fit_rows(self, n):
        if not 2 <= n <= INNE_MAX_ROWS:
            raise ValueError(f"SubspaceINNE fit needs between 2 and {INNE_MAX_ROWS} rows, got {n}")

    def _ranges(self):
        """[(first, count)]: the subspaces of one launch (a grid dimension bounds them)."""
        return [(first, min(_INNE_MAX_RANGE, self.plan.count - first)) for first in range(0, self.plan.count, _INNE_MAX_RANGE)]

    def _score(self, Xq, fitting):
        per = torch.empty(self.plan.count, Xq.shape[0], dtype=torch.float32, device=Xq.device)
        for first, count in self._ranges():
            self.ops.inne_scores(Xq, self._X, self._table, first, count, int(self.plan.dims[first:first + count].max()), self._state,
                                 per[first:first + count])
        return self._combine(per, fitting), per

    def _state_on_host(self):
        self._require_fit()
        if self._host_state is None:
            self._host_state = tuple(a.cpu().numpy() for a in self._state)
        return self._host_state

    @property
    def center_rows_(self):
        """int32 [S, T, psi]: the centres of every estimator as rows of the fitted X, in draw order."""
        return self._state_on_host()[0]

    @property
    def radius_sq_(self):
        """float64 [S, T, psi]: the squared radius of every centre's sphere, d2 to its nearest other centre."""
        return self._state_on_host()[1]

    @property
    def center_nn_(self):
        """int32 [S, T, psi]: the position within its estimator of every centre's nearest other centre."""
        return self._state_on_host()[2]

    @property
    def isolation_ratio_(self):
        """float64 [S, T, psi]: rho of every centre, in [0, 1]."""
        return self._state_on_host()[3]

    def fit(self, X, y=None):
        """Keeps X resident, builds the T estimators of every subspace on their samples of it, then scores X itself through
        them: decision_scores_ (float64 [n]), per_subspace_scores_, max_samples_ and, on first use, center_rows_ / radius_sq_
        / center_nn_ / isolation_ratio_; with normalize also score_center_ / score_scale_."""
        self._X = X = self._begin_fit(X)
        psi = min(self._max_samples, X.shape[0])
        self.max_samples_, self._host_state = psi, None
        shape = (self.plan.count, self.n_estimators, psi)
        kinds = (torch.int32, torch.float64, torch.int32, torch.float64)  # rows, r2, nn, rho
        self._state = tuple(torch.empty(shape, dtype=dt, device=X.device) for dt in kinds)
        for first, count in self._ranges():
            self.ops.inne_build(X, self._table, first, count, int(self.plan.dims[first:first + count].max()), INNE_RATIOS[self.ratio],
                                self.seed, self._state)
        scores, per = self._score(X, fitting=True)
        return self._publish(scores, per)


# ---- Mahalanobis / MCD: covariance-based scores over the subspaces ------------------------------------------------------
MAHA_MAX_DIMS = 1024  # VGAN_MAHA_MAX_DIMS: features of one subspace (its three d_s x d_s float64 matrices stay resident)
MAHA_MAX_ROWS = 1 << 24  # VGAN_MAHA_MAX_ROWS
MAHA_SLAB_ROWS = 1024  # VGAN_MAHA_SLAB_ROWS: rows of one slab of the moment sums, fixed: the partition depends on n alone
MAHA_TILE = 16  # edge of a covariance tile (the f64 MFMA's)
_MAHA_OAS = -1.0  # VGAN_MAHA_SHRINKAGE_OAS
_MAHA_CONSTANT, _MAHA_PIVOT = 1, 2  # VGAN_MAHA_STATUS_*
_MAHA_MAX_RANGE = 65535  # subspaces of one launch (a grid dimension)


def check_shrinkage(shrinkage):
    """A float in [0, 1] (sklearn's ShrunkCovariance) or "oas" (sklearn's OAS rule per subspace)."""
    if isinstance(shrinkage, str):
        if shrinkage != "oas":
            raise ValueError(f"shrinkage must be a float in [0, 1] or 'oas', got {shrinkage!r}")
        return shrinkage
    if not _is_real(shrinkage) or not 0.0 <= float(shrinkage) <= 1.0:  # False for nan
        raise ValueError(f"shrinkage must be a float in [0, 1] or 'oas', got {shrinkage!r}")
    return float(shrinkage)


def check_support_fraction(support_fraction):
    """None (sklearn's rule from n and d_s) or a float in (0, 1]."""
    if support_fraction is None:
        return None
    if not _is_real(support_fraction) or not 0.0 < float(support_fraction) <= 1.0:
        raise ValueError(f"support_fraction must be None or a float in (0, 1], got {support_fraction!r}")
    return float(support_fraction)


def check_csteps(max_csteps):
    if not (_is_int(max_csteps) and int(max_csteps) >= 1):
        raise ValueError(f"max_csteps must be a positive integer, got {max_csteps!r}")
    return int(max_csteps)


def mcd_support_size(n, d_s, support_fraction=None):
    """h_s, the rows of the MCD support of a subspace of d_s features among n rows: min(n, ceil((n + d_s + 1) / 2)) when
    support_fraction is None (sklearn's rule), otherwise int(support_fraction n); ValueError if that is below 2."""
    n, d_s = int(n), int(d_s)
    if support_fraction is None:
        return min(n, (n + d_s + 2) // 2)
    h = int(check_support_fraction(support_fraction) * n)
    if h < 2:
        raise ValueError(f"support_fraction {support_fraction!r} leaves {h} of {n} rows in the support, at least 2 are needed")
    return h


def maha_ranges(dims, workspace_bytes):
    """(the float64 cells of the moment workspace, [(first, count)]): consecutive subspace ranges whose slab sums (8 bytes a
    feature) fit in workspace_bytes; the workspace is never smaller than one subspace's sums or one 16 x 16 tile."""
    dims = [int(v) for v in dims]
    cells = max(int(workspace_bytes) // 8, max(dims), MAHA_TILE * MAHA_TILE)
    out, first = [], 0
    while first < len(dims):
        end, used = first, 0
        while end < len(dims) and end - first < _MAHA_MAX_RANGE and (end == first or used + dims[end] <= cells):
            used += dims[end]
            end += 1
        out.append((first, end - first))
        first = end
    return cells, out


def maha_tiles(dims, first, count):
    """int32 [n_tiles, 3]: (s, ti, tj), tj <= ti < ceil(d_s / 16), for the subspaces first .. first + count - 1."""
    rows = []
    for s in range(first, first + count):
        t = -(-int(dims[s]) // MAHA_TILE)
        ti, tj = np.tril_indices(t)
        rows.append(np.stack([np.full(ti.shape, s), ti, tj], axis=1))
    return np.concatenate(rows).astype(np.int32)


def _launch_ranges(n_subspaces, most=_MAHA_MAX_RANGE):
    """(first, count) of consecutive launches over n_subspaces subspaces, at most `most` (a grid dimension) each."""
    for first in range(0, n_subspaces, most):
        yield first, min(most, n_subspaces - first)


def _split_state(flat, off, shapes=None):
    """The pieces flat[off[i]:off[i + 1]] of a flat fitted-state array as a list of copies, piece i reshaped to shapes[i]."""
    parts = [flat[off[i]:off[i + 1]].copy() for i in range(len(off) - 1)]
    return parts if shapes is None else [p.reshape(shape) for p, shape in zip(parts, shapes)]


class _MomentScorer(_SubspaceScorer):
    """What the covariance detectors (SubspaceMahalanobis, SubspacePCA, SubspaceGMM) share on the host: the constructor
    tail, the layout of the moment launches of csrc/outlier_moments.hpp, and the plain moments themselves."""

    def _configure_moments(self, subspaces, proba, workspace_bytes, normalize, combination, contamination):
        # no distance engine here: "exact" for every subspace keeps the processing order the given order
        self._configure(subspaces, proba, "exact", workspace_bytes, normalize, combination, contamination)
        del self.engine
        if int(self.plan.dims.max()) > MAHA_MAX_DIMS:
            raise ValueError(f"a subspace has {int(self.plan.dims.max())} features, {type(self).__name__} takes at most {MAHA_MAX_DIMS}")

    def _moment_layout(self, n, dev, n_components=None):
        """(device table (feat, feat_off, sq_off), host feat_off, host sq_off, ranges [(first, count)] of subspaces, the
        device tile table of every range, the float64 workspace) of the moment launches for n rows; with n_components = C
        the tables are the expanded ones of gmm_table and a subspace's slab sums are its C (d_s + 1)."""
        dims, C = self.plan.dims, n_components or 1
        if n_components is None:
            feat, feat_off, sq_off = None, self.plan.feat_off, np.concatenate([[0], np.cumsum(dims * dims)]).astype(np.int64)
            cells, ranges = maha_ranges(dims, self.workspace_bytes)
            need = dims
        else:
            feat, feat_off, sq_off = gmm_table(self.plan.feat, self.plan.feat_off, C)
            cells, ranges = gmm_ranges(dims, C, n, self.workspace_bytes)
            need = C * (dims + 1)
        tiles = [maha_tiles(np.repeat(dims, C), first * C, count * C) for first, count in ranges]
        widest = max(int(need[first:first + count].sum()) for first, count in ranges)
        slabs = -(-n // MAHA_SLAB_ROWS)
        most = max(slabs * widest, slabs * MAHA_TILE * MAHA_TILE * max(t.shape[0] for t in tiles))
        # the uploads come last: a copy to the device waits for the work in flight (the column mean of _begin_fit), and the
        # host work above then runs beside it
        table = self._table[:2] if feat is None else tuple(torch.as_tensor(v, device=dev) for v in (feat, feat_off))
        return (table + (torch.as_tensor(sq_off, device=dev),), feat_off, sq_off, ranges, [torch.as_tensor(t, device=dev) for t in tiles],
                torch.empty(min(cells, most), dtype=torch.float64, device=dev))

    def _moments(self, X, support=None, hcount=None):
        """mu and C of every subspace over the rows of its support (None: every row, h_s = n), range by range."""
        if hcount is None:
            hcount = torch.full((self.plan.count,), X.shape[0], dtype=torch.int32, device=X.device)
        for (first, count), tiles in zip(self._ranges, self._tiles):
            dims = self.plan.dims[first:first + count]
            self.ops.maha_moments(X, self._mtable, first, count, int(dims.sum()), int(dims.max()), tiles, support, hcount, self._mean,
                                  self._cov, self._ws)


class SubspaceMahalanobis(_MomentScorer):
    """Squared Mahalanobis distance per subspace under a shrunk covariance, classical or, with robust=True, under a
    deterministic minimum-covariance-determinant estimate (pyod's "linear" family: ``MCD``, and ``PCA`` with all components;
    sklearn's ``EmpiricalCovariance`` / ``ShrunkCovariance`` / ``OAS`` ``.mahalanobis``), combined like the other detectors
    of this module: ``fit`` sets ``decision_scores_``, ``decision_function`` scores new rows; higher is more outlying.  The
    score accounts for the correlation between the features of a subspace, has no neighbour count, bandwidth or tree count,
    and costs n d_s^2 per subspace, nothing n x n.

    X is cast to float32; all arithmetic is float64 on those values.  n rows are given to ``fit``, 2 <= n <= MAHA_MAX_ROWS
    (2^24); a subspace has at most MAHA_MAX_DIMS (1024) features.  Per subspace s (features F_s, d_s of them) and its
    support H_s of h_s rows (every row, h_s = n, when not robust):

        mu_s = (1 / h_s) sum_{i in H_s} x_i                                     the location
        C_s = (1 / h_s) sum_{i in H_s} (x_i - mu_s)(x_i - mu_s)^T               biased, two passes (sklearn's EmpiricalCovariance)
        Sigma_s = (1 - alpha_s) C_s + alpha_s (tr C_s / d_s) I                  sklearn's ShrunkCovariance

    shrinkage is alpha_s for every subspace, a float in [0, 1], or "oas" (sklearn's ``oas``): m = tr C_s / d_s, a = the mean
    of the squared entries of C_s, alpha_s = 1 if (h_s + 1)(a - m^2 / d_s) == 0, otherwise min((a + m^2) / ((h_s + 1)(a -
    m^2 / d_s)), 1).  The default 0.1 is there because constant columns are normal in this project's data (image borders).

    Score: (x - mu_s)^T Sigma_s^-1 (x - mu_s), sklearn's ``.mahalanobis`` and pyod's MCD ``decision_scores_`` up to the
    estimator, computed as ||W_s (x - mu_s)||^2 with W_s = L_s^-1 and L_s the lower Cholesky factor of Sigma_s, so it is never
    negative; rounded to float32 into the [S, n] score matrix.  d^2 grows linearly with d_s, so ``normalize`` is what to
    reach for when subspaces of mixed size are summed.  normalize, combination, contamination, ``threshold_``, ``labels_``,
    ``predict``, ``predict_proba`` and return_per_subspace are the shared tail.  ``fit`` scores the training rows with
    nothing excluded: ``decision_function(X_train)`` equals ``decision_scores_`` bit for bit.

    Degenerate cases go through a per-subspace status word that the host reads once after ``fit``.  tr C_s == 0 (every
    feature constant on the support): every score of that subspace is exactly 0.  A Cholesky pivot that is not positive and
    finite: ``fit`` raises ValueError naming the subspace.  That can only happen with alpha_s = 0 on a singular C_s (or
    non-finite input); the converse does not hold: rounding can leave a singular matrix a tiny positive pivot, which then
    passes with huge scores, so with duplicated or constant features use shrinkage > 0.

    robust=True is a concentration MCD from a single start, deterministic: (1) start from the all-rows estimate; (2) score
    all rows; (3) the new support is the h_s rows with the smallest (float32 score as stored, row index); (4) re-estimate
    mu_s, C_s, alpha_s, W_s on it; repeat from (2) until a support does not change (``converged_[s]``) or max_csteps
    re-estimates have run; ``n_csteps_[s]`` counts the re-estimates.  h_s = mcd_support_size(n, d_s, support_fraction): min(n,
    ceil((n + d_s + 1) / 2)), sklearn's rule, or int(support_fraction n), ValueError below 2.  The published scores are those
    under the final estimate.  Not reproduced: sklearn's random multi-start FastMCD, its consistency correction and its
    reweighting step; Ledoit-Wolf shrinkage.  Limits: with shrinkage the determinant argument for monotone convergence does
    not hold strictly, max_csteps is the bound; and a single classical start breaks down under heavy clustered
    contamination (on the CPU restatement, 1000 x 67 with 30 % of the rows shifted by +6 keeps 124 outliers among the 534 rows
    of the support and ranks them below the inliers).

    Determinism: the moment sums run over slabs of MAHA_SLAB_ROWS rows cut by n alone, each in a fixed order, added in
    ascending slab order; no float atomics.  Scores, supports and every published array are bit-identical from run to run
    and for every workspace_bytes, which limits the slab partials of the moments (maha_ranges: ranges of subspaces, inside
    a range as many slabs and tiles a launch as fit), not the fitted state: mu_s and three d_s x d_s float64 matrices
    (Sigma_s, L_s, W_s) per subspace stay on the device; X is not kept.

    ``fit`` publishes, in the given subspace order and fetched from the device on first use: ``location_`` (list of S
    float64 [d_s]), ``covariance_`` (list of S float64 [d_s, d_s], the shrunk matrix), ``shrinkage_`` (float64 [S]) and, when
    robust, ``support_`` (bool [S, n]), ``n_csteps_`` (int [S]) and ``converged_`` (bool [S]).  The definition above and its
    numpy restatement in tests/test_outlier_maha_cpu.py (pinned there to sklearn) are what binds.  All of it runs in
    libvgan_hip.so (csrc/outlier_maha.hip)."""

    _host_state = None

    def __init__(self, subspaces, proba, shrinkage=0.1, robust=False, support_fraction=None, max_csteps=30,
                 workspace_bytes=DEFAULT_WORKSPACE_BYTES, normalize=None, combination="sum", contamination=0.1):
        self.shrinkage = check_shrinkage(shrinkage)
        self.robust = bool(robust)
        self.support_fraction = check_support_fraction(support_fraction)
        self.max_csteps = check_csteps(max_csteps)
        self._configure_moments(subspaces, proba, workspace_bytes, normalize, combination, contamination)

    def _check_fit_rows(self, n):
        if not 2 <= n <= MAHA_MAX_ROWS:
            raise ValueError(f"SubspaceMahalanobis fit needs between 2 and {MAHA_MAX_ROWS} rows, got {n}")
        if self.robust:
            for d_s in np.unique(self.plan.dims):
                mcd_support_size(n, d_s, self.support_fraction)

    def _prepare(self, n, dev):
        """The tables, the fitted state (mu, and Sigma, L, W at sq_off) and the moment workspace for n rows."""
        S, dims = self.plan.count, self.plan.dims
        self._fitted, self._host_state = False, None
        self._mtable, _, self._sq_off, self._ranges, self._tiles, self._ws = self._moment_layout(n, dev)
        self._mean = torch.empty(int(dims.sum()), dtype=torch.float64, device=dev)
        self._cov, self._L, self._W = (torch.empty(int(self._sq_off[-1]), dtype=torch.float64, device=dev) for _ in range(3))
        self._alpha = torch.empty(S, dtype=torch.float64, device=dev)
        self._status = torch.zeros(S, dtype=torch.int32, device=dev)

    def _factor(self, hcount):
        """alpha, Sigma (over C), L and W of every subspace from its C."""
        alpha = _MAHA_OAS if self.shrinkage == "oas" else self.shrinkage
        for first, count in _launch_ranges(self.plan.count):
            self.ops.maha_factor(self._cov, self._mtable, first, count, int(self.plan.dims[first:first + count].max()), hcount, alpha,
                                 self._L, self._W, self._alpha, self._status)

    def _estimate(self, X, support, hcount):
        self._moments(X, support, hcount)
        self._factor(hcount)

    def _distances(self, X):
        """float32 [S, nq] on the device: the squared distances of the rows of X under the current estimate."""
        per = torch.empty(self.plan.count, X.shape[0], dtype=torch.float32, device=X.device)
        for first, count in _launch_ranges(self.plan.count):
            self.ops.maha_scores(X, self._mtable, first, count, int(self.plan.dims[first:first + count].max()), self._mean, self._W, per)
        return per

    def _score(self, X, fitting):
        per = self._distances(X)
        return self._combine(per, fitting), per

    def _concentrate(self, X, per):
        """The C-steps; returns the scores under the final estimate."""
        S, n, dev = self.plan.count, X.shape[0], X.device
        self._support = torch.ones(S, n, dtype=torch.uint8, device=dev)
        changed = torch.empty(S, dtype=torch.int32, device=dev)
        converged, steps = np.zeros(S, dtype=bool), np.zeros(S, dtype=np.int64)
        for step in range(self.max_csteps):
            for first, count in _launch_ranges(S):
                self.ops.maha_select(per, first, count, self._h, self._support, changed)
            converged |= changed.cpu().numpy() == 0  # a converged support gives the same estimate again, bit for bit
            if converged.all():
                break
            steps[~converged] += 1
            self._estimate(X, self._support, self._h)
            per = self._distances(X)
        self.n_csteps_, self.converged_ = steps, converged
        return per

    def _fetch(self):
        self._require_fit()
        if self._host_state is None:
            self._host_state = (_split_state(self._mean.cpu().numpy(), self.plan.feat_off),
                                _split_state(self._cov.cpu().numpy(), self._sq_off, [(d, d) for d in self.plan.dims]),
                                self._alpha.cpu().numpy(), self._support.cpu().numpy().astype(bool) if self.robust else None)
        return self._host_state

    @property
    def location_(self):
        """List of S float64 [d_s]: mu_s of the final estimate."""
        return self._fetch()[0]

    @property
    def covariance_(self):
        """List of S float64 [d_s, d_s]: the shrunk matrix Sigma_s of the final estimate."""
        return self._fetch()[1]

    @property
    def shrinkage_(self):
        """float64 [S]: alpha_s of the final estimate."""
        return self._fetch()[2]

    @property
    def support_(self):
        """bool [S, n]: the rows of the final support (robust=True only)."""
        if not self.robust:
            raise AttributeError("support_ is published with robust=True only")
        return self._fetch()[3]

    def fit(self, X, y=None):
        """Estimates mu_s and Sigma_s of every subspace (with robust=True by C-steps), then scores X itself: decision_scores_
        (float64 [n]), per_subspace_scores_, location_, covariance_, shrinkage_ and, when robust, support_, n_csteps_,
        converged_; with normalize also score_center_ / score_scale_.  Raises ValueError for a subspace whose Cholesky
        factor does not exist."""
        X = self._begin_fit(X)
        n, S = X.shape[0], self.plan.count
        self._prepare(n, X.device)
        self._estimate(X, None, torch.full((S,), n, dtype=torch.int32, device=X.device))
        per = self._distances(X)
        if self.robust:
            h = [mcd_support_size(n, d_s, self.support_fraction) for d_s in self.plan.dims]
            self._h = torch.as_tensor(np.array(h, dtype=np.int32), device=X.device)
            per = self._concentrate(X, per)
        failed = np.flatnonzero(self._status.cpu().numpy() & _MAHA_PIVOT)
        if failed.size:
            raise ValueError(f"subspace {int(failed[0])}: its covariance has no Cholesky factor (a pivot was not positive and finite: "
                             f"the features are linearly dependent on the support); use shrinkage > 0")
        del self._ws, self._L
        return self._publish(self._combine(per, True), per)


# ---- PCA: principal-component scores over the subspaces --------------------------------------------------------------
PCA_COMPONENT_SETS = ("all", "major", "minor")
PCA_LDS_DIMS = 48  # VGAN_PCA_LDS_DIMS: up to this width the eigensolver keeps M and V in LDS
_PCA_CONSTANT, _PCA_NOT_CONVERGED = 1, 2  # VGAN_PCA_STATUS_*
_PCA_U = 2.0 ** -53


def check_pca_components(n_components, components):
    """n_components: None, an integer >= 1 or a float in (0, 1); components: "all" (n_components must then be None),
    "major" or "minor"."""
    if components not in PCA_COMPONENT_SETS:
        raise ValueError(f"components must be 'all', 'major' or 'minor', got {components!r}")
    if n_components is not None:
        if _is_int(n_components):
            if int(n_components) < 1:
                raise ValueError(f"n_components must be None, an integer >= 1 or a float in (0, 1), got {n_components!r}")
            n_components = int(n_components)
        elif _is_real(n_components) and 0.0 < float(n_components) < 1.0:  # False for nan
            n_components = float(n_components)
        else:
            raise ValueError(f"n_components must be None, an integer >= 1 or a float in (0, 1), got {n_components!r}")
        if components == "all":
            raise ValueError(f"components='all' uses every component: n_components must be None, got {n_components!r}")
    return n_components, components


def check_pca_params(n_components, components, weighted, standardize, shrinkage, max_sweeps):
    """The constructor's checks of SubspacePCA, usable without a device; returns the six values in their canonical types."""
    n_components, components = check_pca_components(n_components, components)
    for name, v in (("weighted", weighted), ("standardize", standardize)):
        if not isinstance(v, (bool, np.bool_)):
            raise ValueError(f"{name} must be True or False, got {v!r}")
    if not _is_real(shrinkage) or not 0.0 <= float(shrinkage) <= 1.0:  # False for nan
        raise ValueError(f"shrinkage must be a float in [0, 1], got {shrinkage!r}")
    if not (_is_int(max_sweeps) and int(max_sweeps) >= 1):
        raise ValueError(f"max_sweeps must be a positive integer, got {max_sweeps!r}")
    return n_components, components, bool(weighted), bool(standardize), float(shrinkage), int(max_sweeps)


def pca_variance_ratio(evals):
    """float64 [d_s]: the eigenvalues clipped at 0 and divided by their sum; all 0 when that sum is 0."""
    lam = np.maximum(np.asarray(evals, dtype=np.float64), 0.0)
    total = lam.sum()
    return lam / total if total > 0.0 else np.zeros_like(lam)


def pca_component_count(evals, n_components):
    """q_s: d_s for None, min(n_components, d_s) for an integer, and for a float f the smallest count whose cumulative
    variance ratio exceeds f: numpy.searchsorted(numpy.cumsum(ratio), f, side="right") + 1, clipped to d_s (sklearn's rule)."""
    d = len(evals)
    if n_components is None:
        return d
    if _is_int(n_components):
        return min(int(n_components), d)
    return min(int(np.searchsorted(np.cumsum(pca_variance_ratio(evals)), float(n_components), side="right")) + 1, d)


def pca_weights(evals, q, components, weighted, shrinkage):
    """(wt float64 [d_s], degenerate bool): w_j for j in J_s ("all": every j; "major": j < q; "minor": j >= q) and 0 outside it.
    w_j = 1 when not weighted, else 1 / ((1 - shrinkage) max(lambda_j, 0) + shrinkage tr / d_s) with tr the sum of the
    eigenvalues as given.  tr == 0: every weight is 0.  degenerate: weighted with shrinkage 0 and a selected lambda_j <= 16
    d_s 2^-53 lambda_1 (the weights are then not to be used)."""
    lam = np.asarray(evals, dtype=np.float64)
    d = lam.shape[0]
    chosen = np.ones(d, dtype=bool) if components == "all" else np.arange(d) < q if components == "major" else np.arange(d) >= q
    tr = float(lam.sum())
    if tr == 0.0 or not chosen.any():
        return np.zeros(d), False
    if not weighted:
        return chosen.astype(np.float64), False
    if shrinkage == 0.0 and (lam[chosen] <= 16 * d * _PCA_U * lam[0]).any():
        return np.zeros(d), True
    shrunk = (1.0 - shrinkage) * np.maximum(lam, 0.0) + shrinkage * tr / d
    wt = np.zeros(d)
    wt[chosen] = 1.0 / shrunk[chosen]
    return wt, False


class SubspacePCA(_MomentScorer):
    """Principal-component outlier scores per subspace (pyod's "linear" family: ``PCA``, as remembered, not pinned against
    pyod; the spectrum is pinned to sklearn's ``StandardScaler`` + ``PCA`` in tests/test_outlier_pca_cpu.py): a row is scored by
    how far it lies along the principal directions of its subspace, the dominant ones (components="major"), the small ones
    (components="minor": with unit weights the reconstruction error off the dominant plane, the score that sees a broken
    correlation structure) or all of them; combined like the other detectors of this module: ``fit`` sets
    ``decision_scores_``, ``decision_function`` scores new rows; higher is more outlying.

    X is cast to float32; all arithmetic is float64 on those values.  n rows are given to ``fit``, 2 <= n <= MAHA_MAX_ROWS
    (2^24); a subspace has at most MAHA_MAX_DIMS (1024) features.  Per subspace s (features F_s, d_s of them):

        mu_s = (1 / n) sum_i x_i,  C_s = (1 / n) sum_i (x_i - mu_s)(x_i - mu_s)^T     SubspaceMahalanobis' moments, bit for bit
        scale_k = sqrt(C_kk), an exact 0 replaced by 1 (standardize=True), or 1       sklearn's StandardScaler rule
        M_s = D^-1 C_s D^-1, D = diag(scale): M_ij = C_ij / (scale_i scale_j)          the correlation matrix; C_s itself if not
        M_s = V^T Lambda V, lambda_1 >= lambda_2 >= ...                              rows of V are the components

    Eigenvalues are in descending order, equal ones in the ascending order of the diagonal position the solver left them
    at; every component is signed so that its entry of largest magnitude (the lowest index on a tie) is positive.  The
    solver is a cyclic Jacobi method with a fixed parallel pair order (include/vgan_hip.h: vgan_pca_eigen has the order and
    the rotation); it stops after the first sweep that rotates nothing (a pair is left alone when |m_pq| <= 2^-53
    sqrt(|m_pp m_qq|)) or after max_sweeps sweeps; ``n_sweeps_[s]`` counts the sweeps run (the last, rotation-free one
    included) and ``converged_[s]`` says whether that last sweep was reached.  A subspace that did not converge is still
    scored with what the sweeps left.

    Component count q_s (``n_components_``): d_s for n_components=None; min(n_components, d_s) for an integer >= 1; for a
    float f in (0, 1) numpy.searchsorted(numpy.cumsum(ratio), f, side="right") + 1 clipped to d_s with ratio =
    ``explained_variance_ratio_[s]`` (sklearn's rule), taken on the host from the fetched eigenvalues.  Component set J_s:
    "all" every component (n_components must be None), "major" the first q_s, "minor" those after the first q_s.

    Score of row i in subspace s: sum_{j in J_s} w_j y_ij^2 with y_i = V_s D_s^-1 (x_i[F_s] - mu_s), evaluated as V ((x - mu)
    (1 / scale)).  w_j = 1 when weighted=False; otherwise w_j = 1 / lambda'_j, lambda'_j = (1 - shrinkage) max(lambda_j, 0) +
    shrinkage tr(M_s) / d_s, with tr(M_s) taken as the float64 sum of the published eigenvalues: the spectrum of sklearn's
    ``ShrunkCovariance``, so that components="all", weighted=True, standardize=False is SubspaceMahalanobis' score.  The
    weights are built on the host (pca_weights) from the fetched eigenvalues.  The sum is rounded to float32 into the [S, n]
    score matrix.  normalize, combination, contamination, ``threshold_``, ``labels_``, ``predict``, ``predict_proba`` and
    return_per_subspace are the shared tail.  ``fit`` excludes nothing: ``decision_function(X_train)`` equals
    ``decision_scores_`` bit for bit.

    Special cases.  tr(M_s) == 0 (every feature constant), or an empty J_s ("minor" with q_s = d_s): every score of the
    subspace is exactly 0.  weighted=True with shrinkage=0 and a selected lambda_j <= 16 d_s 2^-53 lambda_1: ``fit`` raises
    ValueError naming the first such subspace (a constant or duplicated feature among the selected directions); use
    shrinkage > 0, weighted=False or components="major".

    Determinism: the moments are summed over slabs cut by n alone, the rotations of the solver have a fixed order, the
    scoring product a fixed K order, and there is no float atomic: scores, eigenpairs and every published array are
    bit-identical from run to run, for every workspace_bytes (which only limits the slab partials of the moments) and for a
    subspace fitted alone or among others; the score of a row does not depend on where it sits in a call.  mu_s, 1 / scale,
    the weights and V_s stay on the device; X is not kept.

    ``fit`` publishes, in the given subspace order: ``explained_variance_`` (list of S float64 [d_s], the eigenvalues of M_s),
    ``explained_variance_ratio_`` (the eigenvalues clipped at 0, divided by their sum; zeros when that is 0), ``components_``
    (list of S float64 [d_s, d_s], rows are components; fetched on first use), ``location_``, ``scale_`` (lists of S float64
    [d_s]), ``n_components_`` (int [S]), ``n_sweeps_`` (int [S]) and ``converged_`` (bool [S]).

    Not built: randomized / truncated SVD solvers (every subspace gets its full spectrum), ``whiten``, pyod's
    cdist-to-the-eigenvector arithmetic (the projection form above is the one its documentation describes) and incremental
    fitting.  The definition above and its numpy restatement in tests/test_outlier_pca_cpu.py are what binds.  All of it runs
    in libvgan_hip.so (csrc/outlier_pca.hip, the moments in csrc/outlier_maha.hip)."""

    _components = None

    def __init__(self, subspaces, proba, n_components=None, components="all", weighted=True, standardize=True, shrinkage=0.1,
                 max_sweeps=30, workspace_bytes=DEFAULT_WORKSPACE_BYTES, normalize=None, combination="sum", contamination=0.1):
        (self.n_components, self.components, self.weighted, self.standardize, self.shrinkage,
         self.max_sweeps) = check_pca_params(n_components, components, weighted, standardize, shrinkage, max_sweeps)
        self._configure_moments(subspaces, proba, workspace_bytes, normalize, combination, contamination)

    def _check_fit_rows(self, n):
        if not 2 <= n <= MAHA_MAX_ROWS:
            raise ValueError(f"SubspacePCA fit needs between 2 and {MAHA_MAX_ROWS} rows, got {n}")

    def _prepare(self, n, dev):
        """The tables, the fitted state (mu, scale, eigenvalues at feat_off; C and V at sq_off) and the moment workspace."""
        S, dims = self.plan.count, self.plan.dims
        self._fitted, self._components = False, None
        self._mtable, _, self._sq_off, self._ranges, self._tiles, self._ws = self._moment_layout(n, dev)
        self._mean, self._scale, self._evals = (torch.empty(int(dims.sum()), dtype=torch.float64, device=dev) for _ in range(3))
        self._cov, self._V = (torch.empty(int(self._sq_off[-1]), dtype=torch.float64, device=dev) for _ in range(2))
        self._sweeps, self._status = (torch.zeros(S, dtype=torch.int32, device=dev) for _ in range(2))

    def _eigen(self):
        """scale, the eigenvalues and V of every subspace from its C, which is overwritten."""
        for first, count in _launch_ranges(self.plan.count):
            self.ops.pca_eigen(self._cov, self._mtable, first, count, int(self.plan.dims[first:first + count].max()), self.standardize,
                               self.max_sweeps, self._scale, self._evals, self._V, self._sweeps, self._status)

    def _select(self, dev):
        """Host: q_s and the weights from the fetched eigenvalues; uploads the weights and 1 / scale."""
        S, off = self.plan.count, self.plan.feat_off
        evals, scale = self._evals.cpu().numpy(), self._scale.cpu().numpy()
        status = self._status.cpu().numpy()
        self.explained_variance_ = _split_state(evals, off)
        self.explained_variance_ratio_ = [pca_variance_ratio(lam) for lam in self.explained_variance_]
        self.scale_ = _split_state(scale, off)
        self.n_components_ = np.array([pca_component_count(lam, self.n_components) for lam in self.explained_variance_], dtype=np.int64)
        self.n_sweeps_ = self._sweeps.cpu().numpy().astype(np.int64)
        self.converged_ = (status & _PCA_NOT_CONVERGED) == 0
        self._constant = (status & _PCA_CONSTANT) != 0
        wt = np.zeros_like(evals)
        for s in range(S):
            if self._constant[s]:
                continue
            w, degenerate = pca_weights(self.explained_variance_[s], int(self.n_components_[s]), self.components, self.weighted,
                                        self.shrinkage)
            if degenerate:
                raise ValueError(f"subspace {s}: a selected eigenvalue is at most 16 d_s 2^-53 of the largest (a constant or duplicated "
                                 f"feature), so 1 / lambda is not a weight; use shrinkage > 0, weighted=False or components='major'")
            wt[off[s]:off[s + 1]] = w
        self._wt = torch.as_tensor(wt, device=dev)
        self._inv_scale = torch.as_tensor(1.0 / scale, device=dev)

    def _distances(self, X):
        """float32 [S, nq] on the device: the weighted squared projections of the rows of X."""
        per = torch.empty(self.plan.count, X.shape[0], dtype=torch.float32, device=X.device)
        for first, count in _launch_ranges(self.plan.count):
            self.ops.pca_scores(X, self._mtable, first, count, int(self.plan.dims[first:first + count].max()), self._mean,
                                self._inv_scale, self._V, self._wt, per)
        return per

    def _score(self, X, fitting):
        per = self._distances(X)
        return self._combine(per, fitting), per

    @property
    def components_(self):
        """List of S float64 [d_s, d_s]: row j the j-th principal direction of M_s."""
        self._require_fit()
        if self._components is None:
            self._components = _split_state(self._V.cpu().numpy(), self._sq_off, [(d, d) for d in self.plan.dims])
        return self._components

    def fit(self, X, y=None):
        """The moments, the eigenpairs, q_s and the weights of every subspace, then the scores of X itself: decision_scores_
        (float64 [n]), per_subspace_scores_, explained_variance_, explained_variance_ratio_, components_, location_, scale_,
        n_components_, n_sweeps_, converged_; with normalize also score_center_ / score_scale_.  Raises ValueError for a
        subspace whose selected spectrum cannot be inverted (weighted=True, shrinkage=0)."""
        X = self._begin_fit(X)
        self._prepare(X.shape[0], X.device)
        self._moments(X)
        self._eigen()
        self.location_ = _split_state(self._mean.cpu().numpy(), self.plan.feat_off)
        self._select(X.device)
        del self._ws, self._cov
        scores, per = self._score(X, fitting=True)
        return self._publish(scores, per)


# ---- Gaussian mixtures: EM per subspace, the negative log-likelihood as the score ------------------------------------
GMM_MAX_COMPONENTS = 32  # VGAN_GMM_MAX_COMPONENTS: the log probabilities of a row's components live in LDS
_GMM_CONVERGED, _GMM_FAILED = 1, 2  # VGAN_GMM_DONE_*
_GMM_ROW_BLOCK = 64  # rows of one E-step workgroup: the lower bound is summed per block, then per slab


def check_gmm_params(n_components, reg_covar, tol, max_iter, kmeans_max_iter):
    if not (_is_int(n_components) and 1 <= int(n_components) <= GMM_MAX_COMPONENTS):
        raise ValueError(f"n_components must be an integer between 1 and {GMM_MAX_COMPONENTS}, got {n_components!r}")
    if not (_is_real(reg_covar) and np.isfinite(reg_covar) and float(reg_covar) >= 0.0):
        raise ValueError(f"reg_covar must be a finite float >= 0, got {reg_covar!r}")
    if not (_is_real(tol) and np.isfinite(tol) and float(tol) >= 0.0):
        raise ValueError(f"tol must be a finite float >= 0, got {tol!r}")
    if not (_is_int(max_iter) and int(max_iter) >= 1):
        raise ValueError(f"max_iter must be a positive integer, got {max_iter!r}")
    if not (_is_int(kmeans_max_iter) and int(kmeans_max_iter) >= 1):
        raise ValueError(f"kmeans_max_iter must be a positive integer, got {kmeans_max_iter!r}")
    return int(n_components), float(reg_covar), float(tol), int(max_iter), int(kmeans_max_iter)


def check_gmm_init(init, n_components, n_subspaces):
    """init as the constructor can judge it, without the data: "kmeans", or an integer array of labels [n] or [S, n] with
    values in [0, n_components).  Returns "kmeans" or ("labels", int64 [n] or [S, n])."""
    if isinstance(init, str):
        if init != "kmeans":
            raise ValueError(f"init must be 'kmeans' or an integer array of labels, got {init!r}")
        return "kmeans"
    labels = _index_array(init)
    if labels is None:
        raise ValueError(f"init must be 'kmeans' or an integer array of labels, got {type(init).__name__}")
    labels = np.asarray(labels, dtype=np.int64)
    if labels.ndim not in (1, 2) or (labels.ndim == 2 and labels.shape[0] != n_subspaces):
        raise ValueError(f"init labels must have shape (n,) or ({n_subspaces}, n), got {labels.shape}")
    if (labels < 0).any() or (labels >= n_components).any():
        raise ValueError(f"init labels must lie in [0, {n_components}), got {int(labels.min())} .. {int(labels.max())}")
    return "labels", np.ascontiguousarray(labels)


def resolve_gmm_labels(init, n, n_subspaces):
    """int64 [S, n]: the labels of ("labels", array) for n data rows, an [n] array repeated for every subspace."""
    labels = init[1]
    if labels.shape[-1] != n:
        raise ValueError(f"init labels cover {labels.shape[-1]} rows, fit was given {n}")
    return np.broadcast_to(labels, (n_subspaces, n))


def gmm_table(feat, feat_off, n_components):
    """(feat int32, feat_off int32 [S C + 1], sq_off int64 [S C + 1]): the expanded subspace table whose entry e = s C + c is
    component c of subspace s: the feature list of s repeated C times, the running sums of d_s and of d_s^2 accordingly."""
    feat, feat_off, C = np.asarray(feat), np.asarray(feat_off), int(n_components)
    lists = [feat[feat_off[s]:feat_off[s + 1]] for s in range(len(feat_off) - 1)]
    dims = np.repeat(np.diff(feat_off).astype(np.int64), C)
    return (np.concatenate([np.tile(f, C) for f in lists]).astype(np.int32), np.concatenate([[0], np.cumsum(dims)]).astype(np.int32),
            np.concatenate([[0], np.cumsum(dims * dims)]).astype(np.int64))


def gmm_ranges(dims, n_components, n, workspace_bytes):
    """(the float64 cells of the moment workspace, [(first, count)]): consecutive subspace ranges whose responsibilities (8 C n
    bytes a subspace) fit in workspace_bytes, whose slab sums (C (d_s + 1) float64 a subspace) fit in the workspace and
    whose C count entries fit one launch; a range is never smaller than one subspace, the workspace never smaller than one
    subspace's sums or one 16 x 16 tile."""
    dims, C = [int(v) for v in dims], int(n_components)
    need = [C * (v + 1) for v in dims]
    cells = max(int(workspace_bytes) // 8, max(need), MAHA_TILE * MAHA_TILE)
    most = max(1, min(int(workspace_bytes) // (8 * C * int(n)), _MAHA_MAX_RANGE // C))
    out, first = [], 0
    while first < len(dims):
        end, used = first, 0
        while end < len(dims) and end - first < most and (end == first or used + need[end] <= cells):
            used += need[end]
            end += 1
        out.append((first, end - first))
        first = end
    return cells, out


class SubspaceGMM(_MomentScorer):
    """Negative log-likelihood per subspace under a Gaussian mixture of n_components = C full-covariance components fitted
    by EM (pyod's ``GMM``; sklearn's ``GaussianMixture(covariance_type="full", n_init=1)`` and minus its ``score_samples``),
    combined like the other detectors of this module: ``fit`` sets ``decision_scores_``, ``decision_function`` scores new
    rows; higher is more outlying.  A single covariance per subspace (SubspaceMahalanobis) is blind to rows that fall between
    the modes of multi-modal data; the mixture sees them at n C d_s^2 per EM iteration, nothing n x n, and keeps C small
    matrices per subspace.

    X is cast to float32; all arithmetic is float64 on those values.  n rows are given to ``fit``, max(2, C) <= n <=
    MAHA_MAX_ROWS (2^24); a subspace has at most MAHA_MAX_DIMS (1024) features; 1 <= C <= GMM_MAX_COMPONENTS (32).  Per
    subspace s (features F_s, d_s of them) and component c:

        start    hard labels l_i in [0, C) become one-hot responsibilities r_ic; one M step follows.
        M step   nk_c = sum_i r_ic + 10 eps (eps the float64 machine epsilon);  mu_c = sum_i r_ic x_i / nk_c;
                 Sigma_c = sum_i r_ic (x_i - mu_c)(x_i - mu_c)^T / nk_c + reg_covar I  (two passes);  w_c = nk_c / sum_c nk_c.
        E step   lp_ic = -0.5 (d_s log 2pi + ||W_c (x_i - mu_c)||^2) - sum_j log L_c[j, j] + log w_c, L_c the lower Cholesky
                 factor of Sigma_c and W_c = L_c^-1;  ln_i = logsumexp_c lp_ic (the maximum subtracted first);
                 r_ic = exp(lp_ic - ln_i), evaluated as exp(lp_ic - max) / sum_c exp(lp_ic - max): the same number without the
                 half ulp of ln_i, so that a row of responsibilities sums to 1 within a few ulps;  lb = (1 / n) sum_i ln_i.
        loop     lb_prev = -inf; for it = 1 .. max_iter: E step (lb), M step, then |lb - lb_prev| < tol stops the subspace at
                 this it (``converged_[s]``), otherwise lb_prev = lb.  ``n_iter_[s]`` = it; ``lower_bound_[s]`` is the last lb,
                 which belongs to the parameters before the last M step, as in sklearn.  tol = 0 never fires and runs
                 max_iter iterations.  No warning is raised.
        score    -ln_i under the final parameters, rounded to float32 into the [S, n] score matrix.

    init "kmeans" (default) takes the labels from SubspaceCBLOF(subspaces, proba, n_clusters=C, init="random", seed=seed,
    max_iter=kmeans_max_iter) fitted on the same X (its ``cluster_labels_``); with C = 1 every label is 0 and no k-means
    runs.  Or an integer array of labels [n] or [S, n] (given subspace order).  An empty component follows the formulas: mu
    = 0, Sigma = reg_covar I, w about 2e-15 / n, as sklearn's would.  normalize, combination, contamination, ``threshold_``,
    ``labels_``, ``predict`` (outlier labels), ``predict_proba`` and return_per_subspace are the shared tail.  ``fit`` scores
    the training rows with nothing left out: ``decision_function(X_train)`` equals ``decision_scores_`` bit for bit.

    Failures: a Cholesky pivot that is not positive and finite, or tr Sigma_c == 0, can only occur with reg_covar = 0.  The
    device marks such a subspace done so that it does not hold up the loop; ``fit`` reads the status once at the end and
    raises ValueError naming the subspace and the component.

    Freezing and determinism: the device decides the stop of a subspace at the exact iteration and a stopped subspace keeps
    its parameters bit for bit while the others go on; the host only looks at the done flags every ``poll_stride``
    iterations (an attribute, default POLL_STRIDE; no result depends on it).  The moment and lower-bound sums run over slabs
    of MAHA_SLAB_ROWS rows cut by n alone, each in a fixed order, added in ascending order; no float atomics; an element of
    the E step sees k ascending wherever its row sits.  Every published array and score is bit-identical from run to run,
    for every workspace_bytes, for every poll_stride, and for a subspace fitted alone or together with others.
    workspace_bytes limits the responsibilities of a range of subspaces (8 C n bytes a subspace, never less than one
    subspace) and the slab partials of the moments (gmm_ranges); iterations are outermost, the ranges inside them.  The
    fitted state stays on the device: mu_c, Sigma_c, W_c, the log-determinants and the log-weights; X is not kept.

    ``fit`` publishes, in the given subspace order: ``weights_`` (float64 [S, C]), ``means_`` (list of S float64 [C, d_s]),
    ``covariances_`` (list of S float64 [C, d_s, d_s]), ``n_iter_`` (int [S]), ``converged_`` (bool [S]) and
    ``lower_bound_`` (float64 [S]); and ``kmeans_labels_`` (int [S, n]): the start labels that init "kmeans" took from the
    k-means, None after every other fit (explicit labels, or C = 1, where no k-means runs).  Not built: covariance_type other than "full", n_init > 1, k-means++ starts,
    warm_start, AIC / BIC and the prediction of components.  The definition above and its numpy restatement in
    tests/test_outlier_gmm_cpu.py (pinned there to sklearn) are what binds.  All of it runs in libvgan_hip.so
    (csrc/outlier_gmm.hip, the Cholesky factor and its inverse in csrc/outlier_maha.hip, the k-means start in
    csrc/cluster.hip)."""

    _host_state = None

    def __init__(self, subspaces, proba, n_components=2, reg_covar=1e-6, tol=1e-3, max_iter=100, init="kmeans", kmeans_max_iter=30,
                 seed=0, workspace_bytes=DEFAULT_WORKSPACE_BYTES, normalize=None, combination="sum", contamination=0.1):
        self.n_components, self.reg_covar, self.tol, self.max_iter, self.kmeans_max_iter = check_gmm_params(
            n_components, reg_covar, tol, max_iter, kmeans_max_iter)
        self._configure_moments(subspaces, proba, workspace_bytes, normalize, combination, contamination)
        self.init = check_gmm_init(init, self.n_components, self.plan.count)
        self.seed = check_seed(seed)
        self._subspaces = np.asarray(subspaces).astype(bool)
        self.poll_stride = POLL_STRIDE

    def _check_fit_rows(self, n):
        if not max(2, self.n_components) <= n <= MAHA_MAX_ROWS:
            raise ValueError(f"SubspaceGMM fit needs between {max(2, self.n_components)} (n_components, and at least 2) and "
                             f"{MAHA_MAX_ROWS} rows, got {n}")
        if self.init != "kmeans":
            resolve_gmm_labels(self.init, n, self.plan.count)

    def _prepare(self, n, dev):
        """The expanded table, the fitted state (per entry e = s C + c: mu at feat_off[e]; Sigma, L, W at sq_off[e]; nk, w,
        log w, the log-determinant, the factor's status), the loop's flags and the buffers of a range for n rows."""
        S, C = self.plan.count, self.n_components
        self._fitted, self._host_state = False, None
        self._etable, feat_off, sq_off, self._ranges, self._tiles, self._ws = self._moment_layout(n, dev, C)
        self._efeat_off, self._esq_off = feat_off, sq_off
        f64 = dict(dtype=torch.float64, device=dev)
        largest = max(count for _, count in self._ranges)
        self._resp = torch.empty(largest * C * n, **f64)
        self._lbpart = torch.empty(largest * -(-n // _GMM_ROW_BLOCK), **f64)
        self._mean = torch.empty(int(feat_off[-1]), **f64)
        self._cov, self._L, self._W = (torch.empty(int(sq_off[-1]), **f64) for _ in range(3))
        self._nk, self._weights, self._logw, self._logdet, self._alpha = (torch.empty(S * C, **f64) for _ in range(5))
        self._status = torch.zeros(S * C, dtype=torch.int32, device=dev)
        self._hcount = torch.full((S * C,), n, dtype=torch.int32, device=dev)  # the factor reads it for the OAS rule only
        self._done = torch.zeros(S, dtype=torch.int32, device=dev)
        self._iters = torch.zeros(S, dtype=torch.int32, device=dev)
        self._lb = torch.full((S,), float("nan"), **f64)
        self._lb_prev = torch.full((S,), float("-inf"), **f64)

    def _start_labels(self, X):
        """int64 [S, n] on the device: the hard labels the first M step starts from."""
        S, n, C = self.plan.count, X.shape[0], self.n_components
        self.kmeans_labels_ = None  # a refit never shows the labels of an earlier one
        if self.init != "kmeans":
            return torch.as_tensor(resolve_gmm_labels(self.init, n, S).copy(), device=X.device)  # broadcast_to gives a read-only view
        if C == 1:
            return torch.zeros(S, n, dtype=torch.int64, device=X.device)
        km = SubspaceCBLOF(self._subspaces, self.proba, n_clusters=C, init="random", seed=self.seed, max_iter=self.kmeans_max_iter)
        self.kmeans_labels_ = km.fit(X).cluster_labels_
        return torch.as_tensor(self.kmeans_labels_.astype(np.int64), device=X.device)

    def _moments(self, X, i):
        """nk, w, log w, mu and Sigma of range i from the responsibilities in _resp."""
        (first, count), C = self._ranges[i], self.n_components
        dims = self.plan.dims[first:first + count]
        self.ops.gmm_moments(X, self._etable, C, first, count, C * int(dims.sum()), int(dims.max()), self._tiles[i], self._resp, self._done,
                             self.reg_covar, self._nk, self._weights, self._logw, self._mean, self._cov, self._ws)

    def _factor(self, i):
        """L, W = L^-1 and the log-determinants of range i.  Shrinkage 0 leaves the covariance as it is, so a frozen subspace
        gets the same matrices again."""
        (first, count), C = self._ranges[i], self.n_components
        self.ops.maha_factor(self._cov, self._etable, first * C, count * C, int(self.plan.dims[first:first + count].max()), self._hcount,
                             0.0, self._L, self._W, self._alpha, self._status)
        self.ops.gmm_logdet(self._L, self._etable, C, first, count, self._logdet)

    def _converge(self, i, iteration, n):
        """The stop rule of `iteration` for range i (0: only a failed factor is looked at)."""
        first, count = self._ranges[i]
        self.ops.gmm_converge(self._lbpart if iteration else None, n, self.n_components, first, count, self._status, self.tol, iteration,
                              self._done, self._iters, self._lb, self._lb_prev)

    def _m_step(self, X, i, iteration):
        self._moments(X, i)
        self._factor(i)
        self._converge(i, iteration, X.shape[0])

    def _e_step(self, X, i):
        (first, count), C = self._ranges[i], self.n_components
        self.ops.gmm_estep(X, self._etable, C, first, count, int(self.plan.dims[first:first + count].max()), self._mean, self._W,
                           self._logdet, self._logw, done=self._done, resp=self._resp, lb_partial=self._lbpart)

    def _em_start(self, X, labels):
        """The one-hot responsibilities of the labels (int64 [S, n] on the device) and the first M step, range by range."""
        C, n = self.n_components, X.shape[0]
        for i, (first, count) in enumerate(self._ranges):
            resp = self._resp[:count * C * n].view(count, C, n)
            resp.zero_()
            resp.scatter_(1, labels[first:first + count].unsqueeze(1), 1.0)
            self._m_step(X, i, 0)

    def _em(self, X, labels):
        """Iterations outermost, ranges inside.  The host enqueues poll_stride iterations at a time and then reads the done
        flags through one pinned buffer; the device has stopped every subspace at its own iteration."""
        S = self.plan.count
        self._em_start(X, labels)
        flags = torch.empty(S, dtype=torch.int32).pin_memory()
        stream = torch.cuda.current_stream()
        launched = 0
        while launched < self.max_iter:
            steps = min(max(1, int(self.poll_stride)), self.max_iter - launched)
            for it in range(launched + 1, launched + steps + 1):
                for i in range(len(self._ranges)):
                    self._e_step(X, i)
                    self._m_step(X, i, it)
            launched += steps
            flags.copy_(self._done, non_blocking=True)
            stream.synchronize()
            if bool((flags != 0).all()):
                break

    def _score(self, X, fitting):
        C = self.n_components
        per = torch.empty(self.plan.count, X.shape[0], dtype=torch.float32, device=X.device)
        for first, count in _launch_ranges(self.plan.count, _MAHA_MAX_RANGE // C):
            self.ops.gmm_estep(X, self._etable, C, first, count, int(self.plan.dims[first:first + count].max()), self._mean, self._W,
                               self._logdet, self._logw, score=per)
        return self._combine(per, fitting), per

    def _fetch(self):
        self._require_fit()
        if self._host_state is None:
            S, C, d = self.plan.count, self.n_components, self.plan.dims
            self._host_state = (self._weights.cpu().numpy().reshape(S, C).copy(),
                                _split_state(self._mean.cpu().numpy(), self._efeat_off[::C], [(C, v) for v in d]),
                                _split_state(self._cov.cpu().numpy(), self._esq_off[::C], [(C, v, v) for v in d]))
        return self._host_state

    @property
    def weights_(self):
        """float64 [S, C]: w_c of the final parameters."""
        return self._fetch()[0]

    @property
    def means_(self):
        """List of S float64 [C, d_s]: mu_c of the final parameters."""
        return self._fetch()[1]

    @property
    def covariances_(self):
        """List of S float64 [C, d_s, d_s]: Sigma_c of the final parameters (reg_covar on the diagonal)."""
        return self._fetch()[2]

    def fit(self, X, y=None):
        """EM per subspace on X from the start labels, then the scores of X itself under the final parameters:
        decision_scores_ (float64 [n]), per_subspace_scores_, weights_, means_, covariances_, n_iter_, converged_,
        lower_bound_; with normalize also score_center_ / score_scale_.  Raises ValueError for a component whose covariance
        has no Cholesky factor."""
        X = self._begin_fit(X)
        labels = self._start_labels(X)
        self._prepare(X.shape[0], X.device)
        self._em(X, labels)
        C = self.n_components
        self.n_iter_ = self._iters.cpu().numpy().astype(np.int64)
        self.converged_ = self._done.cpu().numpy() == _GMM_CONVERGED
        self.lower_bound_ = self._lb.cpu().numpy()
        failed = np.flatnonzero(self._status.cpu().numpy())
        if failed.size:
            raise ValueError(f"subspace {int(failed[0]) // C}, component {int(failed[0]) % C}: its covariance has no Cholesky factor (a "
                             f"pivot was not positive and finite, or its trace is 0: the features are linearly dependent on the rows "
                             f"of the component); use reg_covar > 0")
        del self._ws, self._L, self._resp, self._lbpart
        scores, per = self._score(X, fitting=True)
        return self._publish(scores, per)


OCSVM_MAX_ROWS = 1 << 15  # VGAN_OCSVM_MAX_ROWS: the fixed-point score sum stays below 2^63 and a kernel matrix below 2^32 bytes
OCSVM_LDS_ROWS = 2048  # VGAN_OCSVM_LDS_ROWS: up to here a launch of the solver keeps a and G in LDS
OCSVM_STORAGE = {"auto": 0, "global": 1, "lds": 2, "wide": 3}  # VGAN_OCSVM_STORAGE_*
OCSVM_SMO_STRIDE = 128  # SMO steps of one launch
OCSVM_GAMMA_RULES = ("scale", "auto")
_OCSVM_CONVERGED = 1  # VGAN_OCSVM_DONE_CONVERGED


def check_ocsvm_params(nu, gamma, tol, max_iter):
    """nu in (0, 1]; gamma a positive finite float, "scale" or "auto"; tol > 0; max_iter None or an integer >= 1."""
    if not (_is_real(nu) and 0.0 < float(nu) <= 1.0):  # False for nan
        raise ValueError(f"nu must be a float in (0, 1], got {nu!r}")
    if isinstance(gamma, str):
        if gamma not in OCSVM_GAMMA_RULES:
            raise ValueError(f"gamma must be a positive float, 'scale' or 'auto', got {gamma!r}")
    elif not (_is_real(gamma) and np.isfinite(gamma) and gamma > 0):
        raise ValueError(f"gamma must be a positive float, 'scale' or 'auto', got {gamma!r}")
    else:
        gamma = float(gamma)
    if not (_is_real(tol) and np.isfinite(tol) and tol > 0):
        raise ValueError(f"tol must be positive and finite, got {tol!r}")
    if max_iter is not None and not (_is_int(max_iter) and 1 <= int(max_iter) < 2 ** 31):
        raise ValueError(f"max_iter must be None or an integer between 1 and 2^31 - 1, got {max_iter!r}")
    return float(nu), gamma, float(tol), None if max_iter is None else int(max_iter)


def check_ocsvm_rows(n):
    if not 2 <= n <= OCSVM_MAX_ROWS:
        raise ValueError(f"the one-class SVM takes between 2 and {OCSVM_MAX_ROWS} fitted rows, got {n}")


def ocsvm_gamma(gamma, dims, var=None):
    """float64 [S]: gamma_s per subspace of dims (sizes d_s).  "scale": 1 / (d_s var_s), var_s the variance over all entries of
    the subspace's block (var [S]), taken as 1.0 where it is 0 (sklearn's rule); "auto": 1 / d_s; a float: itself."""
    d = np.asarray(dims, dtype=np.float64)
    if gamma == "scale":
        var = np.asarray(var, dtype=np.float64)
        return 1.0 / (d * np.where(var == 0.0, 1.0, var))
    if gamma == "auto":
        return 1.0 / d
    return np.full(d.shape, float(gamma), dtype=np.float64)


def ocsvm_block_variance(col_mean, col_ssd, n, feats):
    """The float64 variance over the n x d_s entries of the columns feats, from every column's mean and its sum of squared
    deviations from that mean: (sum_f ssd_f + n sum_f (mean_f - mu)^2) / (n d_s), mu the mean of the column means."""
    mean, ssd = np.asarray(col_mean, np.float64)[feats], np.asarray(col_ssd, np.float64)[feats]
    mu = mean.mean()
    return float((ssd.sum() + n * ((mean - mu) ** 2).sum()) / (n * len(feats)))


def ocsvm_start(nu, n):
    """(m, a_m) of libsvm's start: m = int(nu n) rows at 1 and, when m < n, row m at nu n - m (0.0 for m = n)."""
    m = int(nu * n)
    return m, (nu * n - m if m < n else 0.0)


def ocsvm_chunks(plan, n, limit_bytes):
    """[(first, count, gram)]: SubspacePlan.chunks with the n x n float32 kernel matrix of every subspace next to its packed
    block, at most 65535 subspaces (a launch's grid) a chunk."""
    return plan.chunks(n, limit_bytes, extra_bytes=4 * int(n) * int(n), max_count=65535)


def _resolve_rbf_gamma(plan, gamma, X):
    """float64 [S] in processing order: ocsvm_gamma with, for "scale", the block variances over all rows of X (on the device)."""
    var = None
    if gamma == "scale":
        Xd = X.double()
        mean = Xd.mean(dim=0)
        ssd = ((Xd - mean) ** 2).sum(dim=0)
        mean, ssd = mean.cpu().numpy(), ssd.cpu().numpy()
        var = [ocsvm_block_variance(mean, ssd, X.shape[0], plan.feat[plan.feat_off[z]:plan.feat_off[z + 1]])
               for z in range(plan.count)]
    return ocsvm_gamma(gamma, plan.dims, var)


class SubspaceOCSVM(_SubspaceScorer):
    """One-class SVM per subspace (Schoelkopf et al. 2001; sklearn's OneClassSVM(kernel="rbf", shrinking=False), pyod's OCSVM),
    combined like the detectors of SubspaceEnsemble: ``fit`` sets ``decision_scores_``, ``decision_function`` scores new rows,
    higher is more outlying.  Only the RBF kernel is built: no linear, poly or sigmoid kernel (no coef0 / degree), no
    shrinking, no kernel cache.  This docstring is the contract.

    Kernel.  K_s(x, y) = exp(-gamma_s d_s(x, y)^2) on the raw features of subspace s.  gamma is a positive float, "scale" or
    "auto".  "scale" is 1 / (d_s var), var the float64 variance over all n x d_s entries of the subspace's block, 1.0 where
    that variance is 0 (sklearn's rule); "auto" is 1 / d_s.  The default is "scale": this project's data is not
    standardised.  ``fit`` publishes ``gamma_``, float64 [S].  The per-column float64 means and sums of squared deviations
    come from torch on the device and are combined per subspace on the host (ocsvm_block_variance).

    Kernel matrix.  ``fit`` builds K, float32 [n, n], per subspace from the float32 distance engines (exact below
    GRAM_MIN_DIMS, Gram above with operands centred on the column mean, as for KDE): an entry is the float32 exp of float32(-gamma_s
    d2).  The diagonal is stored as exactly 1.  K need not be bitwise symmetric; every use below names its row.  Subspaces
    are chunked so that count n n 4 bytes plus the packed blocks fit workspace_bytes; a subspace that alone exceeds it forms
    a chunk of its own.  ``fit`` takes 2 to 2^15 rows.

    Dual and start (libsvm's scaling).  Minimise 1/2 a^T K a subject to 0 <= a_t <= 1 and sum a = nu n, nu in (0, 1].  m =
    int(nu n) on the host; a_t = 1 for t < m, a_m = nu n - m when m < n, the rest 0.  G = K a starts as the sum over the
    nonzero rows r in ascending order, G_t += (double)K[r, t] a_r, every product and every sum rounded on its own.

    Iteration: WSS2 of Fan, Chen and Lin 2005, all float64 with K widened from float32, every operation rounded on its own
    (nothing is contracted into an FMA).
      1. i is the lowest index with the largest -G_t among a_t < 1; Gmax = -G_i; Gmax2 is the largest G_t among a_t > 0.
      2. Stop as converged if no such i exists or if Gmax + Gmax2 < tol.
      3. Among t with a_t > 0 and b_t = Gmax + G_t > 0 take q_t = 2.0 - 2.0 K[i, t], and q_t = 1e-12 if q_t <= 0; j is the
         lowest index with the smallest -(b_t b_t) / q_t.  Stop as converged if there is none.
      4. delta = (G_i - G_j) / q_j, s = a_i + a_j, a_i -= delta, a_j += delta, then libsvm's four clips for equal labels, in
         libsvm's order, with C = 1.
      5. For every t, G_t = G_t + (K[i, t] da_i + K[j, t] da_j).
      6. n_iter += 1.
    (libsvm itself keeps the highest index on a tie of either selection; ties between float64 gradients of real data are
    rare, and the lowest index is this class's rule.)  After max_iter updates the subspace stops with ``converged_`` False;
    max_iter=None means 100 n.  Every subspace stops on its own and keeps a and G bit for bit while the others go on.

    rho is the mean of G_t over 0 < a_t < 1.  With no such row it is (max G over a_t = 1 + min G over a_t = 0) / 2.  With one of
    those two sets empty as well (nu = 1: every a_t is 1) it is the other side's bound: libsvm's formula is infinite there,
    this is this class's own rule.

    Score.  score_s(x) = rho_s - sum_r a_r K_s(x_r, x): minus sklearn's ``decision_function``, pyod's ``decision_scores_``.
    ``fit`` keeps X resident and scores the training rows through the same sweep as ``decision_function``, excluding
    nothing: ``decision_function(X_train)`` equals ``decision_scores_`` bit for bit.  The sweep is the distance engines over
    all fitted rows (rows with a_r = 0 add no term; the diagonal rule of the kernel matrix does not apply).  Each term a_r K(q,
    r) lies in [0, 1] and is added as rint(term 2^44) in 64-bit fixed point, exact below 2^63 for n <= 2^15; rho enters as
    rint(rho 2^44), and the integer difference times 2^-44 is rounded to float32.  The sum has no order: scores are
    bit-identical from run to run, for every splits and workspace_bytes, and for a subspace fitted alone or with others.  A
    subspace whose features are all constant has K = 1 everywhere, takes 0 iterations and scores exactly 0.

    Published: the common attributes; ``dual_coef_`` float64 [S, n]; ``support_``, a list of S index arrays (a_t > 0);
    ``n_support_`` [S]; ``intercept_`` = -rho, float64 [S]; ``gamma_``; ``n_iter_`` [S]; ``converged_`` [S]; all in the given
    subspace order.

    engine, splits (the reference-row split of the kernel-matrix and scoring sweeps), normalize, combination and
    contamination are those of SubspaceEnsemble.  Four attributes, set after construction, serve tests and measurements
    and change no result: ``smo_stride`` (SMO steps of one launch, default OCSVM_SMO_STRIDE), ``poll_stride`` (launches
    between two looks at the done flags, default POLL_STRIDE), ``storage`` ("auto", "lds", "global" or "wide": whether a launch
    keeps a and G in LDS or in place, the latter with 256 or 1024 threads) and ``keep_kernel_matrix`` (True: ``fit`` also publishes ``kernel_matrix_``, a list of S float32 [n, n] arrays,
    the matrices the solver read)."""

    _X = None

    def __init__(self, subspaces, proba, nu=0.5, gamma="scale", tol=1e-3, max_iter=None, engine="auto", splits=None,
                 workspace_bytes=DEFAULT_WORKSPACE_BYTES, normalize=None, combination="sum", contamination=0.1):
        self.nu, self.gamma, self.tol, self.max_iter = check_ocsvm_params(nu, gamma, tol, max_iter)
        self._configure(subspaces, proba, engine, workspace_bytes, normalize, combination, contamination)
        self._configure_splits(splits)
        self.smo_stride, self.poll_stride, self.storage = OCSVM_SMO_STRIDE, POLL_STRIDE, "auto"
        self.keep_kernel_matrix = False

    # ---- pipeline --------------------------------------------------------------------------------
    def _check_fit_rows(self, n):
        check_ocsvm_rows(n)

    def _resolve_gamma(self, X):
        """float64 [S] in processing order."""
        return _resolve_rbf_gamma(self.plan, self.gamma, X)

    def _kernel_matrix(self, X, first, count, gram):
        n = X.shape[0]
        P, sq = self._pack(X, first, count, gram)
        K = torch.empty(count, n, n, dtype=torch.float32, device=X.device)
        self.ops.ocsvm_kernel_matrix(P, sq, n, self._table, first, count, self._gamma, ENGINES["gram" if gram else "exact"],
                                     self._splits(n, n, count), K)
        return K

    def _smo(self, K, first, count, max_iter, flags):
        """The solver on the chunk's matrices: the start, then launches of smo_stride steps; the host looks at the chunk's
        done flags through one pinned buffer every poll_stride launches.  At most max_iter steps are ever enqueued."""
        n = K.shape[1]
        a, g = self._alpha[first:first + count], self._G[first:first + count]
        done, iters = self._done[first:first + count], self._iters[first:first + count]
        self.ops.ocsvm_init(K, *ocsvm_start(self.nu, n), a, g, done, iters)
        stream = torch.cuda.current_stream()
        launched = 0
        while launched < max_iter:
            for _ in range(max(1, int(self.poll_stride))):
                steps = min(max(1, int(self.smo_stride)), max_iter - launched)
                if steps <= 0:
                    break
                self.ops.ocsvm_smo(K, self.tol, max_iter, steps, a, g, done, iters, OCSVM_STORAGE[self.storage])
                launched += steps
            flags[:count].copy_(done, non_blocking=True)
            stream.synchronize()
            if bool((flags[:count] != 0).all()):
                break
        self.ops.ocsvm_rho(a, g, self._rho[first:first + count])

    def _score(self, Xq, fitting):
        per = self._sweep(Xq, self._X, lambda blocks, first, count, tail: self.ops.ocsvm_scores(
            *blocks, self._table, first, count, self._gamma, self._alpha, self._rho, *tail))
        return self._combine(per, fitting), per

    # ---- public surface --------------------------------------------------------------------------
    def fit(self, X, y=None):
        """The kernel matrices and the SMO loop per subspace of X, then the scores of X itself: decision_scores_ (float64 [n]),
        per_subspace_scores_, dual_coef_, support_, n_support_, intercept_, gamma_, n_iter_, converged_; with normalize also
        score_center_ / score_scale_.  X stays resident as the fitted rows."""
        self._X = X = self._begin_fit(X)
        n, S, dev = X.shape[0], self.plan.count, X.device
        gamma = self._resolve_gamma(X)
        self._gamma = torch.as_tensor(gamma, device=dev)
        self._alpha = torch.empty(S, n, dtype=torch.float64, device=dev)
        self._G = torch.empty(S, n, dtype=torch.float64, device=dev)
        self._rho = torch.empty(S, dtype=torch.float64, device=dev)
        self._done = torch.zeros(S, dtype=torch.int32, device=dev)
        self._iters = torch.zeros(S, dtype=torch.int32, device=dev)
        max_iter = 100 * n if self.max_iter is None else self.max_iter
        flags = torch.empty(S, dtype=torch.int32).pin_memory()
        kept = [None] * S
        for first, count, gram in ocsvm_chunks(self.plan, n, self.workspace_bytes):
            K = self._kernel_matrix(X, first, count, gram)
            self._smo(K, first, count, max_iter, flags)
            if self.keep_kernel_matrix:
                self._keep(kept, K, first)
            del K
        del self._G
        scores, per = self._score(X, fitting=True)
        g = self.plan.given
        self.gamma_ = gamma[g]
        self.dual_coef_ = self._alpha.cpu().numpy()[g]
        self.support_ = [np.flatnonzero(a > 0.0) for a in self.dual_coef_]
        self.n_support_ = np.array([len(s) for s in self.support_], dtype=np.int64)
        self.intercept_ = -self._rho.cpu().numpy()[g]
        self.n_iter_ = self._iters.cpu().numpy()[g].astype(np.int64)
        self.converged_ = self._done.cpu().numpy()[g] == _OCSVM_CONVERGED
        if self.keep_kernel_matrix:
            self.kernel_matrix_ = kept
        return self._publish(scores, per)


# ---- kernel PCA: the reconstruction error in the feature space of an RBF kernel over landmark rows ------------------------
KPCA_MAX_LANDMARKS = 1024  # VGAN_KPCA_MAX_LANDMARKS = VGAN_MAHA_MAX_DIMS: the eigensolver's limit
KPCA_AUTO_LANDMARKS = 256  # max_samples="auto"
KPCA_MAX_ROWS = MAHA_MAX_ROWS  # rows of one fit or one decision_function call
_KPCA_SLAB = 64  # query rows of a scoring workgroup: row slabs are multiples of it


def check_kpca_landmarks(landmarks):
    """None, or an integer array [m] of distinct row indices >= 0, 2 <= m <= KPCA_MAX_LANDMARKS; returned as int64."""
    if landmarks is None:
        return None
    idx = _index_array(landmarks)
    if idx is None or idx.ndim != 1:
        raise ValueError("landmarks must be None or a one-dimensional integer array of row indices")
    idx = np.ascontiguousarray(idx, dtype=np.int64)
    if not 2 <= idx.shape[0] <= KPCA_MAX_LANDMARKS:
        raise ValueError(f"landmarks must hold between 2 and {KPCA_MAX_LANDMARKS} rows, got {idx.shape[0]}")
    if (idx < 0).any():
        raise ValueError("landmarks must be >= 0")
    if (np.diff(np.sort(idx)) == 0).any():
        raise ValueError("landmarks must be distinct")
    return idx


def check_kpca_params(n_components, gamma, max_samples, landmarks, eig_tol, max_sweeps, seed):
    """The constructor's checks of SubspaceKPCA, usable without a device: n_components None, an integer >= 1 or a float in
    (0, 1); gamma as for SubspaceOCSVM; max_samples "auto" (256) or an integer between 2 and KPCA_MAX_LANDMARKS; landmarks as
    check_kpca_landmarks; eig_tol a float in [0, 1); max_sweeps an integer >= 1; seed an integer in [0, 2^64).  Returns the
    seven values in their canonical types."""
    n_components, _ = check_pca_components(n_components, "major")
    _, gamma, _, _ = check_ocsvm_params(0.5, gamma, 1e-3, None)
    if not (isinstance(max_samples, str) and max_samples == "auto"):
        if not (_is_int(max_samples) and 2 <= int(max_samples) <= KPCA_MAX_LANDMARKS):
            raise ValueError(f"max_samples must be 'auto' or an integer between 2 and {KPCA_MAX_LANDMARKS}, got {max_samples!r}")
        max_samples = int(max_samples)
    if not (_is_real(eig_tol) and 0.0 <= float(eig_tol) < 1.0):  # False for nan
        raise ValueError(f"eig_tol must be a float in [0, 1), got {eig_tol!r}")
    if not (_is_int(max_sweeps) and int(max_sweeps) >= 1):
        raise ValueError(f"max_sweeps must be a positive integer, got {max_sweeps!r}")
    return n_components, gamma, max_samples, check_kpca_landmarks(landmarks), float(eig_tol), int(max_sweeps), check_seed(seed)


def resolve_kpca_landmarks(landmarks, max_samples, n, seed):
    """int64 [m]: the landmark rows for n fitted rows.  landmarks given: themselves (every index below n).  Otherwise m = min(n,
    256) for "auto", min(max_samples, n) for an integer, and the rows are numpy.sort(numpy.random.default_rng(seed).choice(n, m,
    replace=False))."""
    if landmarks is not None:
        if (landmarks >= n).any():
            raise ValueError(f"landmark row {int(landmarks.max())} is out of range for {n} rows")
        return landmarks
    m = min(n, KPCA_AUTO_LANDMARKS if max_samples == "auto" else max_samples)
    return np.sort(np.random.default_rng(seed).choice(n, m, replace=False)).astype(np.int64)


def kpca_weights(evals, n_components, eig_tol):
    """(wt float64 [m], q, n_usable) from the eigenvalues of a centred kernel matrix in descending order.  Component j is usable
    iff lambda_j > eig_tol lambda_0 (none when lambda_0 <= 0); q = n_usable for None, min(n_components, n_usable) for an
    integer, pca_component_count over the usable eigenvalues for a float; wt_j = 1 / lambda_j for j < q and 0 beyond."""
    lam = np.asarray(evals, dtype=np.float64)
    usable = int(np.count_nonzero(lam > eig_tol * lam[0])) if lam[0] > 0.0 else 0
    q = pca_component_count(lam[:usable], n_components) if usable else 0
    wt = np.zeros(lam.shape[0])
    wt[:q] = 1.0 / lam[:q]
    return wt, q, usable


def kpca_fit_chunks(plan, m, limit_bytes):
    """[(first, count, gram)]: SubspacePlan.chunks with the m x m kernel matrix (float32) and centred matrix (float64) of every
    subspace next to its packed landmark block, at most 65535 subspaces (a launch's grid) a chunk."""
    return plan.chunks(m, limit_bytes, extra_bytes=12 * int(m) * int(m), max_count=65535)


def kpca_chunks(plan, m, rows, limit_bytes):
    """[(first, count, gram, slab)]: consecutive runs of the processing order, one engine each, scored `slab` query rows at a
    time (a multiple of 64, or all `rows`).  A piece is one subspace times 64 rows (all rows when there are fewer): its float32
    kernel block (m a row), float64 row means and packed query block (values and norms), plus the subspace's packed landmark
    block.  A run takes subspaces while their pieces fit in limit_bytes, then as many rows a slab as still fit; a piece that
    alone exceeds limit_bytes forms a chunk of its own."""
    out, first = [], 0
    widths = _round4(plan.dims)
    least = min(int(rows), _KPCA_SLAB)
    while first < plan.count:
        end, fixed, per_row = first, 0, 0
        while end < plan.count and plan.gram[end] == plan.gram[first] and end - first < 65535:
            f, r = int(m) * (int(widths[end]) + 1) * 4, int(m) * 4 + 8 + (int(widths[end]) + 1) * 4
            if end > first and fixed + f + (per_row + r) * least > limit_bytes:
                break
            fixed, per_row = fixed + f, per_row + r
            end += 1
        slab = max((int(limit_bytes) - fixed) // per_row // _KPCA_SLAB * _KPCA_SLAB, least)
        out.append((first, end - first, bool(plan.gram[first]), min(slab, int(rows))))
        first = end
    return out


class SubspaceKPCA(_SubspaceScorer):
    """Kernel PCA novelty scores per subspace (Hoffmann 2007: the reconstruction error in the feature space of an RBF kernel;
    sklearn's ``KernelPCA`` for the decomposition, pinned in tests/test_outlier_kpca_cpu.py; pyod's ``KPCA`` score as
    remembered, not pinned), combined like the other detectors of this module: ``fit`` sets ``decision_scores_``,
    ``decision_function`` scores new rows; higher is more outlying.  It is the nonlinear ``SubspacePCA(components="minor",
    weighted=False)``: a row is scored by what of its feature-space image the leading kernel components do not explain, so
    it also finds rows that sit inside the data (the centre of a ring).  This docstring is the contract.

    Landmarks.  m = min(n, 256) for max_samples="auto", else min(max_samples, n) with max_samples in 2 .. 1024
    (KPCA_MAX_LANDMARKS, the eigensolver's limit).  The rows are numpy.sort(numpy.random.default_rng(seed).choice(n, m,
    replace=False)), drawn once on the host and the same for every subspace (SubspaceCBLOF's stance: a subspace fitted alone
    gives the same bits as one fitted with others); ``landmarks`` may be an integer array [m] of distinct row indices
    instead, used in the given order.  ``fit`` copies the m landmark rows and keeps them; X itself does not stay resident,
    so ``fit`` takes 2 to 2^24 rows.  Published: ``landmark_rows_``.

    Kernel.  K_s(x, y) = exp(-gamma_s d_s(x, y)^2) on the raw features of subspace s; gamma follows exactly the rules and
    helpers of SubspaceOCSVM (a positive float, "scale" = 1 / (d_s var) with var the float64 variance over all n x d_s entries
    of the fitted block, 1.0 where it is 0, or "auto" = 1 / d_s; ocsvm_gamma, ocsvm_block_variance).  ``gamma_`` is float64 [S].

    Fit, per subspace.  K, float32 [m, m], is SubspaceOCSVM's kernel matrix on the packed landmark block (the float32 exp of
    float32(-gamma_s d2), d2 from the distance engines; the diagonal exactly 1).  It is not bitwise symmetric, so only the
    entries K[r][c] with r <= c are read; K' is the symmetric matrix they define.  colmean_c = (the float64 sum of K'[r][c] over
    r ascending) / m; tot = (the sum of colmean_c over c ascending) / m; Kc[i][j] = ((K'[i][j] - colmean_j) - colmean_i) + tot for
    i <= j, written to both places.  Every operation is rounded on its own and there is no product, so numpy gives the same
    bits.  The eigenpairs of Kc are SubspacePCA's solver's (vgan_pca_eigen with standardize = 0): eigenvalues descending,
    ties by position, each vector a_j a unit vector signed by its entry of largest magnitude; ``n_sweeps_`` and
    ``converged_`` as for SubspacePCA.  Component j is usable iff lambda_j > eig_tol lambda_0: K has float32 entries, so
    eigenvalues around m 2^-24 are rounding noise, and a centred matrix always has one zero eigenvalue (``n_usable_``).
    n_components=None takes every usable component, an integer q the first q usable ones, a float in (0, 1) follows
    pca_component_count's cumulative rule over the usable eigenvalues (``n_components_``).  The weight of component j is w_j =
    1 / lambda_j where selected and 0 otherwise (kpca_weights, on the host from the fetched eigenvalues).

    Score of a row x (the same path for ``fit`` and ``decision_function``, nothing excluded).  k_c = float32 exp(float32(-gamma_s
    d2(x, landmark c))) from the distance engines, without a diagonal rule.  rowmean is the float64 mean of the k_c: 64 partial
    sums, partial l over the columns l, l + 64, ... ascending, combined by the xor butterfly 32, 16, 8, 4, 2, 1, divided by
    m.  z_c = ((k_c - rowmean) - colmean_c) + tot.  y_j = sum_c a_j[c] z_c on the float64 matrix unit, c ascending.  proj =
    sum_j w_j y_j^2 in SubspacePCA's order.  pot = (1.0 - 2.0 rowmean) + tot.  score = float32(max(pot - proj, 0.0)): with
    y_j / sqrt(lambda_j) sklearn's ``KernelPCA.transform``, this is k(x, x) - 2 mean_c k_c + tot - ||transform(x)||^2.

    Special cases and invariants.  A subspace of constant features has K = 1 everywhere, Kc = 0 exactly, no usable component
    and pot = 0: every row scores exactly 0.  ``decision_function(X_train)`` equals ``decision_scores_`` bit for bit.  Every
    sum has one order and there is no atomic: scores and every published array are bit-identical from run to run, for every
    workspace_bytes, for every splits, and for a subspace fitted alone or with others.

    Published, beside the common attributes and in the given subspace order: ``eigenvalues_`` (list of S float64 [m]),
    ``components_`` (list of S float64 [m, m], row j = a_j; fetched on first use), ``n_components_``, ``n_usable_``,
    ``n_sweeps_`` (int [S]), ``converged_`` (bool [S]), ``column_mean_`` (float64 [S, m]), ``total_mean_`` (float64 [S]),
    ``gamma_``, ``landmark_rows_`` (int64 [m]).  ``kernel_rows(X, s)`` returns the float32 [n, m] block the scorer reads for
    subspace s.  One attribute, set after construction, serves tests and changes no result: ``keep_kernel_matrix`` (True:
    ``fit`` also publishes ``kernel_matrix_``, a list of S float32 [m, m] arrays, the matrices the centring read).

    engine, splits (the landmark split of the two distance sweeps), normalize, combination and contamination are those of
    SubspaceEnsemble; workspace_bytes bounds the kernel and centred matrices of a fit chunk and the kernel block, row means
    and packed blocks of a scoring chunk (kpca_fit_chunks, kpca_chunks).

    Not built: other kernels, pyod's ``sampling`` / ``subset_size`` names, a precomputed kernel, more than 1024 landmarks (a
    blocked or Lanczos eigensolver), pre-images and sklearn's ``fit_inverse_transform``.  All of it runs in libvgan_hip.so
    (csrc/outlier_kpca.hip; the kernel matrix in csrc/outlier_ocsvm.hip, the eigensolver in csrc/outlier_pca.hip)."""

    _components = None

    def __init__(self, subspaces, proba, n_components=None, gamma="scale", max_samples="auto", landmarks=None, eig_tol=1e-6,
                 max_sweeps=30, seed=0, engine="auto", splits=None, workspace_bytes=DEFAULT_WORKSPACE_BYTES, normalize=None,
                 combination="sum", contamination=0.1):
        (self.n_components, self.gamma, self.max_samples, self.landmarks, self.eig_tol, self.max_sweeps,
         self.seed) = check_kpca_params(n_components, gamma, max_samples, landmarks, eig_tol, max_sweeps, seed)
        self._configure(subspaces, proba, engine, workspace_bytes, normalize, combination, contamination)
        self._configure_splits(splits)
        self.keep_kernel_matrix = False

    # ---- pipeline --------------------------------------------------------------------------------
    def _check_fit_rows(self, n):
        if not 2 <= n <= KPCA_MAX_ROWS:
            raise ValueError(f"SubspaceKPCA fit needs between 2 and {KPCA_MAX_ROWS} rows, got {n}")

    def _decompose(self, kept):
        """The kernel matrix, its centring and its eigenpairs for every subspace, chunk by chunk."""
        m, dev = self._m, self._L.device
        chunks = kpca_fit_chunks(self.plan, m, self.workspace_bytes)
        most = max(count for _, count, _ in chunks)
        syn = (None, torch.as_tensor(np.arange(most + 1, dtype=np.int32) * m, device=dev),
               torch.as_tensor(np.arange(most + 1, dtype=np.int64) * m * m, device=dev))
        scale = torch.empty(most * m, dtype=torch.float64, device=dev)
        for first, count, gram in chunks:
            P, sq = self._pack(self._L, first, count, gram)
            K = torch.empty(count, m, m, dtype=torch.float32, device=dev)
            self.ops.ocsvm_kernel_matrix(P, sq, m, self._table, first, count, self._gamma, ENGINES["gram" if gram else "exact"],
                                         self._splits(m, m, count, cap=None), K)
            Kc = torch.empty(count * m * m, dtype=torch.float64, device=dev)
            self.ops.kpca_center(K, self._col_mean[first:first + count], self._total[first:first + count], Kc)
            self.ops.pca_eigen(Kc, syn, 0, count, m, False, self.max_sweeps, scale[:count * m], self._evals[first:first + count].view(-1),
                               self._V[first:first + count].view(-1), self._sweeps[first:first + count],
                               self._status[first:first + count])
            if kept is not None:
                self._keep(kept, K, first)
            del P, sq, K, Kc

    def _select(self):
        """Host: the usable components, q_s and the weights from the fetched eigenvalues; uploads the weights."""
        evals = self._evals.cpu().numpy()
        picks = [kpca_weights(lam, self.n_components, self.eig_tol) for lam in evals]
        self._wt = torch.as_tensor(np.stack([p[0] for p in picks]), device=self._evals.device)
        g = self.plan.given
        self.eigenvalues_ = [evals[z].copy() for z in g]
        self.n_components_ = np.array([picks[z][1] for z in g], dtype=np.int64)
        self.n_usable_ = np.array([picks[z][2] for z in g], dtype=np.int64)
        self.n_sweeps_ = self._sweeps.cpu().numpy()[g].astype(np.int64)
        self.converged_ = (self._status.cpu().numpy()[g] & _PCA_NOT_CONVERGED) == 0

    def _kernel_rows(self, Xs, Pr, sqr, first, count, gram):
        """float32 [count, rows, m] on the device: the kernel block of the rows Xs against the chunk's landmark block."""
        rows = Xs.shape[0]
        Pq, sqq = self._pack(Xs, first, count, gram)
        R = torch.empty(count, rows, self._m, dtype=torch.float32, device=Xs.device)
        self.ops.kpca_kernel_rows(Pq, sqq, rows, Pr, sqr, self._m, self._table, first, count, self._gamma,
                                  ENGINES["gram" if gram else "exact"], self._splits(rows, self._m, count, cap=None), R)
        return R

    def _score(self, Xq, fitting):
        nq = Xq.shape[0]
        if nq > KPCA_MAX_ROWS:
            raise ValueError(f"SubspaceKPCA scores at most {KPCA_MAX_ROWS} rows a call, got {nq}")
        per = torch.empty(self.plan.count, nq, dtype=torch.float32, device=Xq.device)
        for first, count, gram, slab in kpca_chunks(self.plan, self._m, nq, self.workspace_bytes):
            Pr, sqr = self._pack(self._L, first, count, gram)
            for r0 in range(0, nq, slab):
                rows = min(slab, nq - r0)
                R = self._kernel_rows(Xq[r0:r0 + rows], Pr, sqr, first, count, gram)
                mean = torch.empty(count, rows, dtype=torch.float64, device=Xq.device)
                self.ops.kpca_row_means(R, mean)
                self.ops.kpca_scores(R, first, mean, self._col_mean, self._total, self._V, self._wt, per[:, r0:r0 + rows],
                                     self._rows[first:first + count])
                del R, mean
            del Pr, sqr
        return self._combine(per, fitting), per

    # ---- public surface --------------------------------------------------------------------------
    def kernel_rows(self, X, s):
        """float32 [n, m]: exp(-gamma_s d2) of the rows of X against the landmark rows in subspace s (given order), the block
        the scorer reads."""
        self._require_fit()
        if not (_is_int(s) and 0 <= int(s) < self.plan.count):
            raise ValueError(f"s must be a subspace index between 0 and {self.plan.count - 1}, got {s!r}")
        Xq = _device_matrix(X, self.plan.d)
        z = int(self.plan.given[int(s)])
        gram = bool(self.plan.gram[z])
        Pr, sqr = self._pack(self._L, z, 1, gram)
        return self._kernel_rows(Xq, Pr, sqr, z, 1, gram)[0].cpu().numpy()

    @property
    def components_(self):
        """List of S float64 [m, m]: row j the coefficients a_j of the j-th kernel component over the landmarks."""
        self._require_fit()
        if self._components is None:
            V = self._V.cpu().numpy()
            self._components = [V[z].copy() for z in self.plan.given]
        return self._components

    def fit(self, X, y=None):
        """The landmarks, their kernel matrix, its centring and eigenpairs, q_s and the weights of every subspace, then the
        scores of X itself: decision_scores_ (float64 [n]), per_subspace_scores_, eigenvalues_, components_, n_components_,
        n_usable_, n_sweeps_, converged_, column_mean_, total_mean_, gamma_, landmark_rows_; with normalize also score_center_
        / score_scale_.  Only the landmark rows stay resident."""
        X = self._begin_fit(X)
        n, S, dev = X.shape[0], self.plan.count, X.device
        self._fitted, self._components = False, None
        rows = resolve_kpca_landmarks(self.landmarks, self.max_samples, n, self.seed)
        self._m = m = int(rows.shape[0])
        self._L = X[torch.as_tensor(rows, device=dev)].contiguous()
        gamma = _resolve_rbf_gamma(self.plan, self.gamma, X)
        self._gamma = torch.as_tensor(gamma, device=dev)
        self._col_mean, self._evals = (torch.empty(S, m, dtype=torch.float64, device=dev) for _ in range(2))
        self._total = torch.empty(S, dtype=torch.float64, device=dev)
        self._V = torch.empty(S, m, m, dtype=torch.float64, device=dev)
        self._sweeps, self._status = (torch.zeros(S, dtype=torch.int32, device=dev) for _ in range(2))
        kept = [None] * S if self.keep_kernel_matrix else None
        self._decompose(kept)
        self._select()
        scores, per = self._score(X, fitting=True)
        g = self.plan.given
        self.gamma_ = gamma[g]
        self.column_mean_ = self._col_mean.cpu().numpy()[g]
        self.total_mean_ = self._total.cpu().numpy()[g]
        self.landmark_rows_ = rows.copy()
        if kept is not None:
            self.kernel_matrix_ = kept
        return self._publish(scores, per)


SOS_MIN_ROWS = 3  # VGAN_SOS_MIN_ROWS: 1 < perplexity < n - 1 needs three rows
SOS_MAX_ROWS = 1 << 15  # VGAN_SOS_MAX_ROWS: the fixed-point score sum stays below 2^63 and a row of the matrix fits the LDS of a CU
SOS_WAVE_ROWS = 2048  # VGAN_SOS_WAVE_ROWS: up to here the search gives a row to one wave, beyond to a workgroup of 1024 threads
SOS_METRICS = {"euclidean": 0, "sqeuclidean": 1}  # VGAN_SOS_METRIC_*
SOS_STORAGE = {"auto": 0, "wave": 1, "block": 2}  # VGAN_SOS_STORAGE_*
_SOS_DEGENERATE, _SOS_UNCONVERGED = 1, 2  # VGAN_SOS_FLAG_*


def check_sos_params(perplexity, metric, tol, max_iter):
    """perplexity a finite float > 1 (fit checks it against n); metric "euclidean" or "sqeuclidean"; tol > 0 and finite; max_iter
    an integer >= 1."""
    if not (_is_real(perplexity) and np.isfinite(perplexity) and float(perplexity) > 1.0):
        raise ValueError(f"perplexity must be a finite float above 1, got {perplexity!r}")
    if not (isinstance(metric, str) and metric in SOS_METRICS):
        raise ValueError(f"metric must be 'euclidean' or 'sqeuclidean', got {metric!r}")
    if not (_is_real(tol) and np.isfinite(tol) and tol > 0):
        raise ValueError(f"tol must be positive and finite, got {tol!r}")
    if not (_is_int(max_iter) and 1 <= int(max_iter) < 2 ** 31):
        raise ValueError(f"max_iter must be an integer between 1 and 2^31 - 1, got {max_iter!r}")
    return float(perplexity), metric, float(tol), int(max_iter)


def check_sos_rows(n):
    if not SOS_MIN_ROWS <= n <= SOS_MAX_ROWS:
        raise ValueError(f"stochastic outlier selection takes between {SOS_MIN_ROWS} and {SOS_MAX_ROWS} fitted rows, got {n}")


def check_sos_perplexity(perplexity, n):
    """1 < perplexity < n - 1: between the entropy of one neighbour and that of all n - 1 other rows."""
    if not 1.0 < perplexity < n - 1:
        raise ValueError(f"perplexity must lie strictly between 1 and n - 1 = {n - 1}, got {perplexity!r}")


def sos_chunks(plan, n, limit_bytes):
    """[(first, count, gram)]: the chunks of ocsvm_chunks, whose n x n float32 matrices and packed blocks these are too."""
    return ocsvm_chunks(plan, n, limit_bytes)


def sos_constant_score(n):
    """What every row of a subspace of constant features scores, up to the fixed-point grid: each of the n - 1 other rows
    binds to it with probability 1 / (n - 1)."""
    return np.float32((1.0 - 1.0 / (n - 1)) ** (n - 1))


class SubspaceSOS(_SubspaceScorer):
    """Stochastic outlier selection per subspace (Janssens, Huszar, Postma, van den Herik 2012; pyod's SOS; the perplexity
    search is t-SNE's, sklearn's ``_binary_search_perplexity``), combined like the detectors of SubspaceEnsemble: ``fit`` sets
    ``decision_scores_``, ``decision_function`` scores new rows, higher is more outlying.  A score is a probability in [0, 1]
    and needs no ``normalize`` to be summed across subspaces of mixed width.  pyod's metrics other than the two below, a
    precomputed dissimilarity matrix and any truncated affinity matrix for more than 2^15 rows are not built.  This
    docstring is the contract.

    Dissimilarity matrix.  ``fit`` builds D_s, float32 [n, n], per subspace from the float32 distance engines (exact below
    GRAM_MIN_DIMS, Gram above with operands centred on the column mean, as for KDE and OCSVM).  metric "euclidean" (the
    default, pyod's): an entry is sqrtf of the engine's float32 d2; "sqeuclidean" (the paper's exp(-d^2 / 2 sigma^2)): d2
    itself.  D[i, j] is the engine's value with row j as the query and row i as the reference row.  The diagonal is never
    read.  D need not be bitwise symmetric; every use below names its row.  Subspaces are chunked so that count n n 4 bytes
    plus the packed blocks fit workspace_bytes (sos_chunks); a subspace that alone exceeds it forms a chunk of its own.  ``fit``
    takes 3 to 2^15 rows and keeps X resident.  perplexity is a float with 1 < perplexity < n - 1: the constructor checks
    perplexity > 1 and finite, ``fit``, which knows n, the rest.  tol > 0 and finite; max_iter an integer of 1 or more.

    Per fitted row i, all float64 with D widened from float32, every operation rounded on its own (nothing is contracted
    into an FMA): over j != i, dmin_i = min_j D[i, j], e_j = D[i, j] - dmin_i >= 0, and m_i the number of j with e_j = 0.  The
    shift changes neither the binding probabilities nor the entropy; it takes the place of pyod's "divide beta by 10 on NaN"
    branch, because the row sum can no longer underflow to 0.

    Degenerate rows.  If m_i >= perplexity the entropy can never fall to log(perplexity) (duplicates in narrow subspaces of
    discrete features, constant subspaces).  Then beta_i = inf, Z_i = m_i, n_iter = 0, and the row's affinity to a row at
    dissimilarity d is 1 if d <= dmin_i, else 0: the uniform distribution over its tied nearest rows.  ``n_degenerate_[s]``
    counts these rows.

    Search for the other rows.  beta = 1, lo = 0, hi = inf.  At each step a_j = exp(-(beta e_j)), Z = sum_j a_j, H = log(Z) +
    beta ((sum_j e_j a_j) / Z) and diff = H - log(perplexity), the last logarithm taken once on the host (the C library's).  Stop
    if |diff| <= tol; otherwise stop if max_iter updates have run, and the row counts in ``n_unconverged_[s]``; otherwise, if
    diff > 0: lo = beta, and beta = 2 beta while hi is inf, else (beta + hi) / 2; if diff <= 0: hi = beta, and beta = (beta + lo) /
    2.  This is pyod's loop and sklearn's.  The order of the two sums is the implementation's own.  Z_i and dmin_i, taken at
    the final beta, are part of the fitted state.

    Scores.  For a row q at dissimilarity d_i to fitted row i, a_i = exp(-(beta_i (d_i - dmin_i))), or the degenerate rule.  At
    ``fit`` row j reads d_i = D[j, i], its own row of the matrix, leaves i = j out and binds with b = min(a_i / Z_i, 1), the
    term t_i = -log1p(-b).  ``decision_function`` scores a new row alone, as appended to the fitted set and visible to the
    fitted rows with their widths as fitted (the stance of ECOD's): b = a_i / (Z_i + a_i), so t_i = log1p(a_i / Z_i), which is
    inf where a_i overflows; d_i comes from the engine with the new row as query.  Either way the term is min(t_i, 128), added
    as rint(term 2^40) in 64-bit fixed point, exact below 2^63 for n <= 2^15 (the device of the OCSVM scores).  The
    per-subspace score is float32(exp(-(sum 2^-40))): the probability that no fitted row binds to the row.  The sum has no
    order: scores are bit-identical from run to run, for every splits and workspace_bytes, and for a subspace fitted alone or
    with others.  ``decision_function(X_train)`` is not ``decision_scores_``: there every row meets itself at dissimilarity
    0.  A subspace of constant features scores float32((1 - 1/(n-1))^(n-1)) up to the fixed-point grid, the same for every row
    (sos_constant_score).

    Published: the common attributes; ``beta_`` float64 [S, n]; ``n_iter_`` int32 [S, n]; ``n_degenerate_`` and
    ``n_unconverged_`` int64 [S]; all in the given subspace order.

    engine, splits (the reference-row split of the matrix and scoring sweeps), normalize, combination and contamination are
    those of SubspaceEnsemble.  Two attributes, set after construction, serve tests and measurements and change no result:
    ``storage`` ("auto", "wave" or "block": whether the search gives a row to one wave or to a workgroup of 1024 threads; "wave"
    takes at most SOS_WAVE_ROWS rows) and ``keep_distance_matrix`` (True: ``fit`` also publishes ``distance_matrix_``, a list of S
    float32 [n, n] arrays, the matrices the search read)."""

    _X = None

    def __init__(self, subspaces, proba, perplexity=4.5, metric="euclidean", tol=1e-5, max_iter=200, engine="auto", splits=None,
                 workspace_bytes=DEFAULT_WORKSPACE_BYTES, normalize=None, combination="sum", contamination=0.1):
        self.perplexity, self.metric, self.tol, self.max_iter = check_sos_params(perplexity, metric, tol, max_iter)
        self._configure(subspaces, proba, engine, workspace_bytes, normalize, combination, contamination)
        self._configure_splits(splits)
        self.storage = "auto"
        self.keep_distance_matrix = False

    # ---- pipeline --------------------------------------------------------------------------------
    def _check_fit_rows(self, n):
        check_sos_rows(n)
        check_sos_perplexity(self.perplexity, n)

    def _distance_matrix(self, X, first, count, gram):
        n = X.shape[0]
        P, sq = self._pack(X, first, count, gram)
        D = torch.empty(count, n, n, dtype=torch.float32, device=X.device)
        self.ops.sos_distance_matrix(P, sq, n, self._table, first, count, SOS_METRICS[self.metric],
                                     ENGINES["gram" if gram else "exact"], self._splits(n, n, count), D)
        return D

    def _search(self, D, first, count, iters, flags):
        """The perplexity search of every row of the chunk's matrices."""
        rng = slice(first, first + count)
        self.ops.sos_fit(D, self.perplexity, self.tol, self.max_iter, self._beta[rng], self._dmin[rng], self._Z[rng], iters[rng],
                         flags[rng], SOS_STORAGE[self.storage])

    def _score_fitted(self, D, first, count, per):
        """The scores of the fitted rows themselves, from the chunk's stored matrices."""
        rng = slice(first, first + count)
        self.ops.sos_fit_scores(D, self._beta[rng], self._dmin[rng], self._Z[rng], per, self._rows[rng])

    def _score(self, Xq, fitting):
        """The new-row form (Xq is never the fitted tensor itself); fit scores its own rows from the stored matrices, chunk by
        chunk (_score_fitted)."""
        per = self._sweep(Xq, self._X, lambda blocks, first, count, tail: self.ops.sos_scores(
            *blocks, self._table, first, count, SOS_METRICS[self.metric], self._beta, self._dmin, self._Z, *tail))
        return self._combine(per, fitting), per

    # ---- public surface --------------------------------------------------------------------------
    def fit(self, X, y=None):
        """The dissimilarity matrices, the perplexity search of every row and the scores of X itself: decision_scores_ (float64
        [n]), per_subspace_scores_, beta_, n_iter_, n_degenerate_, n_unconverged_; with normalize also score_center_ /
        score_scale_.  X stays resident as the fitted rows."""
        self._X = X = self._begin_fit(X)
        n, S, dev = X.shape[0], self.plan.count, X.device
        self._beta = torch.empty(S, n, dtype=torch.float64, device=dev)
        self._dmin = torch.empty(S, n, dtype=torch.float64, device=dev)
        self._Z = torch.empty(S, n, dtype=torch.float64, device=dev)
        iters = torch.empty(S, n, dtype=torch.int32, device=dev)
        flags = torch.empty(S, n, dtype=torch.int32, device=dev)
        per = torch.empty(S, n, dtype=torch.float32, device=dev)
        kept = [None] * S
        for first, count, gram in sos_chunks(self.plan, n, self.workspace_bytes):
            D = self._distance_matrix(X, first, count, gram)
            self._search(D, first, count, iters, flags)
            self._score_fitted(D, first, count, per)
            if self.keep_distance_matrix:
                self._keep(kept, D, first)
            del D
        g = self.plan.given
        self.beta_ = self._beta.cpu().numpy()[g]
        self.n_iter_ = iters.cpu().numpy()[g]
        flags = flags.cpu().numpy()[g]
        self.n_degenerate_ = (flags == _SOS_DEGENERATE).sum(axis=1).astype(np.int64)
        self.n_unconverged_ = (flags == _SOS_UNCONVERGED).sum(axis=1).astype(np.int64)
        if self.keep_distance_matrix:
            self.distance_matrix_ = kept
        return self._publish(self._combine(per, fitting=True), per)


# ---- local correlation integral: neighbour counts against those of the neighbourhood, over a grid of radii ---------------
LOCI_MIN_ROWS = 2  # VGAN_LOCI_MIN_ROWS: r_max is the largest off-diagonal entry
LOCI_MAX_ROWS = 1 << 15  # VGAN_LOCI_MAX_ROWS: m S2 and S1^2 stay below 2^60
LOCI_MAX_RADII = 64  # VGAN_LOCI_MAX_RADII


def check_loci_params(alpha, n_min, n_radii, radii_per_octave, k_sigma):
    """alpha in (0, 1]; n_min an integer >= 1 (fit checks it against n); n_radii an integer from 1 to LOCI_MAX_RADII;
    radii_per_octave positive and finite; k_sigma positive."""
    if not (_is_real(alpha) and 0.0 < float(alpha) <= 1.0):
        raise ValueError(f"alpha must lie in (0, 1], got {alpha!r}")
    if not (_is_int(n_min) and 1 <= int(n_min) < 2 ** 31):
        raise ValueError(f"n_min must be an integer of 1 or more, got {n_min!r}")
    if not (_is_int(n_radii) and 1 <= int(n_radii) <= LOCI_MAX_RADII):
        raise ValueError(f"n_radii must be an integer between 1 and {LOCI_MAX_RADII}, got {n_radii!r}")
    if not (_is_real(radii_per_octave) and np.isfinite(radii_per_octave) and float(radii_per_octave) > 0.0):
        raise ValueError(f"radii_per_octave must be positive and finite, got {radii_per_octave!r}")
    if not (_is_real(k_sigma) and float(k_sigma) > 0.0):  # false for nan
        raise ValueError(f"k_sigma must be positive, got {k_sigma!r}")
    return float(alpha), int(n_min), int(n_radii), float(radii_per_octave), float(k_sigma)


def check_loci_rows(n, n_min):
    if not LOCI_MIN_ROWS <= n <= LOCI_MAX_ROWS:
        raise ValueError(f"the local correlation integral takes between {LOCI_MIN_ROWS} and {LOCI_MAX_ROWS} fitted rows, got {n}")
    if n_min > n:
        raise ValueError(f"n_min must not exceed the number of fitted rows {n}, got {n_min}")


def loci_radii(r_max, n_radii, radii_per_octave, alpha):
    """(r, a) float32 [..., R]: the sampling radii r_j = float32(float64(r_max) exp2(-(R - 1 - j) / radii_per_octave)), ascending
    with r_{R-1} = r_max, and the counting radii a_j = float32(alpha float64(r_j)); r_max float32 [...]."""
    r_max = np.asarray(r_max, dtype=np.float32)
    steps = np.exp2(-(n_radii - 1 - np.arange(n_radii, dtype=np.float64)) / float(radii_per_octave))
    r = (r_max.astype(np.float64)[..., None] * steps).astype(np.float32)
    return r, (float(alpha) * r.astype(np.float64)).astype(np.float32)


def loci_chunks(plan, n, n_radii, limit_bytes):
    """[(first, count, gram)]: the chunks of sos_chunks with, next to a subspace's n x n float32 matrix, its n x R counts and sums
    (int32 cnt and m, int64 S1 and S2)."""
    return plan.chunks(n, limit_bytes, extra_bytes=4 * int(n) * int(n) + 24 * int(n) * int(n_radii), max_count=65535)


class SubspaceLOCI(_SubspaceScorer):
    """The local correlation integral per subspace over a fixed grid of radii (LOCI: Papadimitriou, Kitagawa, Gibbons,
    Faloutsos, ICDE 2003; pyod's ``LOCI``), combined like the detectors of SubspaceEnsemble: ``fit`` sets ``decision_scores_``,
    ``decision_function`` scores new rows, higher is more outlying.  It is the proximity detector without a k: a row's
    neighbour count within alpha r is compared with the counts of the rows within r of it, at every radius r of the grid, and the
    score is the largest deviation in units of the local standard deviation (MDEF / sigma_MDEF); the paper flags a score above
    k_sigma = 3, which needs no contamination guess.  A group of more than 32 anomalous rows that lie close together, which
    every detector with a neighbour list of at most MAX_NEIGHBORS rows scores as inliers of its own group, stands out at the
    radii that reach beyond the group.  Not built: the exact LOCI over the critical radii of every row (the grid below takes
    their place), aLOCI's quad-tree approximation, metrics other than the Euclidean one, and more than 2^15 fitted rows.  This
    docstring is the contract.

    Distance matrix.  Per subspace s, D is the float32 Euclidean matrix of SubspaceSOS (``vgan_sos_distance_matrix``'s bits, written
    by ``vgan_loci_distance_matrix``, which also takes 2 rows: sqrtf of
    the engines' float32 d2, exact below GRAM_MIN_DIMS, Gram above with operands centred on the column mean), D[c][q] with the
    subject row q as the query.  Every kernel takes the diagonal as 0 whatever is stored.  Subspaces are chunked so that the
    matrices, the counts and sums and the packed blocks fit workspace_bytes (loci_chunks); X stays resident.

    Radii.  r_max[s] is the largest off-diagonal entry of D, an exact float32 maximum that has no order.  On the host
    (loci_radii), with R = n_radii: r_j = float32(float64(r_max) * exp2(-(R - 1 - j) / radii_per_octave)), j = 0 .. R-1, ascending,
    r_{R-1} = r_max; the counting radii are a_j = float32(alpha * float64(r_j)).  ``radii_`` float32 [S, R] publishes r.

    Counts and sums, with c over the fitted rows (the row itself included, through the zero diagonal) and every comparison
    made in float32: cnt[q, j] = #{c : D[c][q] <= a_j} (int32); m[p, j] = #{c : D[c][p] <= r_j}; S1[p, j] = the sum over those c of
    cnt[c, j]; S2[p, j] = the sum over those c of cnt[c, j]^2 (int64).

    Score.  num = S1 - cnt[p, j] m and den = m S2 - S1^2, both int64, exact because n <= 2^15 keeps both products below 2^60;
    den >= 0.  Radius j is valid for p iff m >= n_min and den > 0.  The per-subspace score is float32(max(0, max over valid j
    of float64(num) / sqrt(float64(den)))).  ``best_radius_[s, p]`` is the lowest j attaining a positive maximum and -1 where
    the score is 0.  A subspace of constant features has r_max = 0 and scores exactly 0 everywhere.  ``fit`` takes 2 to 2^15
    rows and raises when n_min > n.

    New rows.  ``decision_function`` scores a new row alone, as appended to the fitted set, with the fitted counts unchanged
    (the stance of SubspaceECOD and SubspaceSOS).  Over the fitted rows c, with d the engine's float32 distance (the new row
    as query): A_j = #{d <= a_j}, M_j = #{d <= r_j}, T1_j = the sum of cnt[c, j] and T2_j the sum of cnt[c, j]^2 over the rows of
    M_j, added as 64-bit integers; then cnt_x = A + 1, m = M + 1, S1 = T1 + cnt_x, S2 = T2 + cnt_x^2 and the same rule with the
    stored ``radii_``.  So ``decision_function(X_train)`` is not ``decision_scores_``.

    Everything up to one division and one square root per (row, radius) is an integer and has no order: counts, sums, scores
    and ``best_radius_`` are bit-identical from run to run, for every splits and workspace_bytes, and for a subspace fitted
    alone or with others.

    Published: the common attributes; ``radii_`` float32 [S, R]; ``best_radius_`` int32 [S, n]; ``neighbor_counts_`` int32
    [S, n, R] (cnt); ``flagged_`` bool [S, n], the per-subspace score above k_sigma, and ``n_flagged_`` int64 [S]; all in the
    given subspace order.  ``distance_rows(X, s)`` gives the float32 [n, n_fitted] distances of the rows of X that
    ``decision_function`` counts in subspace s, ``row_sums(X, s)`` the integers (A, M, T1, T2) it forms from them.

    engine, splits (the reference-row split of the matrix and new-row sweeps), normalize, combination and contamination are
    those of SubspaceEnsemble.  Two attributes, set after construction, serve tests and measurements and change no result:
    ``keep_sums`` (True: ``fit`` also publishes ``sampling_counts_`` int32 (m), ``sum_counts_`` and ``sum_sq_counts_`` int64 (S1,
    S2), all [S, n, R]) and ``keep_distance_matrix`` (True: ``distance_matrix_``, a list of S float32 [n, n] arrays, the matrices
    the sweeps read)."""

    _X = None

    def __init__(self, subspaces, proba, alpha=0.5, n_min=20, n_radii=32, radii_per_octave=4.0, k_sigma=3.0, engine="auto",
                 splits=None, workspace_bytes=DEFAULT_WORKSPACE_BYTES, normalize=None, combination="sum", contamination=0.1):
        self.alpha, self.n_min, self.n_radii, self.radii_per_octave, self.k_sigma = check_loci_params(
            alpha, n_min, n_radii, radii_per_octave, k_sigma)
        self._configure(subspaces, proba, engine, workspace_bytes, normalize, combination, contamination)
        self._configure_splits(splits)
        self.keep_sums = False
        self.keep_distance_matrix = False

    # ---- pipeline --------------------------------------------------------------------------------
    def _check_fit_rows(self, n):
        check_loci_rows(n, self.n_min)

    def _distance_matrix(self, X, first, count, gram):
        n = X.shape[0]
        P, sq = self._pack(X, first, count, gram)
        D = torch.empty(count, n, n, dtype=torch.float32, device=X.device)
        self.ops.loci_distance_matrix(P, sq, n, self._table, first, count, ENGINES["gram" if gram else "exact"],
                                      self._splits(n, n, count), D)
        return D

    def _set_radii(self, D, first, count):
        """The chunk's radii from its matrices: r_max on the device (an exact maximum off the diagonal), the grid on the host."""
        r_max = torch.empty(count, dtype=torch.float32, device=D.device)
        self.ops.loci_rmax(D, r_max)
        r, a = loci_radii(r_max.cpu().numpy(), self.n_radii, self.radii_per_octave, self.alpha)
        self._r[first:first + count] = torch.as_tensor(r, device=D.device)
        self._a[first:first + count] = torch.as_tensor(a, device=D.device)

    def _counts(self, D, first, count):
        self.ops.loci_counts(D, self._a[first:first + count], self._cnt[first:first + count])

    def _sums(self, D, first, count):
        shape, dev = (count, D.shape[1], self.n_radii), D.device
        m = torch.empty(shape, dtype=torch.int32, device=dev)
        S1, S2 = (torch.empty(shape, dtype=torch.int64, device=dev) for _ in range(2))
        self.ops.loci_sums(D, self._r[first:first + count], self._cnt[first:first + count], m, S1, S2)
        return m, S1, S2

    def _finish(self, sums, first, count, per, best):
        self.ops.loci_finish(self._cnt[first:first + count], *sums, self.n_min, per, self._rows[first:first + count], best)

    def _score(self, Xq, fitting, best=None):
        """The new-row form (Xq is never the fitted tensor itself); fit scores its own rows from the stored matrices."""
        nq, nr, R = Xq.shape[0], self._X.shape[0], self.n_radii
        per = torch.empty(self.plan.count, nq, dtype=torch.float32, device=Xq.device)
        for first, count, gram in self.plan.chunks(nr + nq, self.workspace_bytes, extra_bytes=32 * nq * R, max_count=65535):
            Pr, sqr = self._pack(self._X, first, count, gram)
            Pq, sqq = self._pack(Xq, first, count, gram)
            acc = torch.empty(count, nq, 4, R, dtype=torch.int64, device=Xq.device)
            self.ops.loci_scores(Pq, sqq, nq, Pr, sqr, nr, self._table, first, count, self._r, self._a, self._cnt, self.n_min,
                                 ENGINES["gram" if gram else "exact"], self._splits(nq, nr, count), acc, per,
                                 self._rows[first:first + count], best)
            del Pr, sqr, Pq, sqq, acc
        return self._combine(per, fitting), per

    def _rows_of(self, X, s):
        """(distances float32 [nq, n], integers int64 [nq, 4, R]) of the rows of X in subspace s, from the entry that scores them."""
        self._require_fit()
        if not (_is_int(s) and 0 <= int(s) < self.plan.count):
            raise ValueError(f"s must be a subspace index between 0 and {self.plan.count - 1}, got {s!r}")
        Xq = _device_matrix(X, self.plan.d)
        z = int(self.plan.given[int(s)])
        gram = bool(self.plan.gram[z])
        nq, nr = Xq.shape[0], self._X.shape[0]
        Pr, sqr = self._pack(self._X, z, 1, gram)
        Pq, sqq = self._pack(Xq, z, 1, gram)
        acc = torch.empty(1, nq, 4, self.n_radii, dtype=torch.int64, device=Xq.device)
        dist = torch.empty(nq, nr, dtype=torch.float32, device=Xq.device)
        score = torch.empty(1, nq, dtype=torch.float32, device=Xq.device)
        self.ops.loci_scores(Pq, sqq, nq, Pr, sqr, nr, self._table, z, 1, self._r, self._a, self._cnt, self.n_min,
                             ENGINES["gram" if gram else "exact"], self._splits(nq, nr, 1), acc, score, dist_out=dist)
        return dist.cpu().numpy(), acc[0].cpu().numpy()

    # ---- public surface --------------------------------------------------------------------------
    def distance_rows(self, X, s):
        """float32 [n, n_fitted]: the distances of the rows of X to the fitted rows in subspace s (given order) that
        ``decision_function`` counts."""
        return self._rows_of(X, s)[0]

    def row_sums(self, X, s):
        """(A, M, T1, T2), int64 [n, R] each: the integers ``decision_function`` forms for the rows of X in subspace s."""
        return tuple(self._rows_of(X, s)[1].transpose(1, 0, 2))

    def decision_function(self, X, return_per_subspace=False, return_best_radius=False):
        """As _SubspaceScorer.decision_function; with return_best_radius=True also the int32 [S, n] best radius indices of the
        new rows (last)."""
        if not return_best_radius:
            return super().decision_function(X, return_per_subspace)
        self._require_fit()
        Xq = _device_matrix(X, self.plan.d)
        best = torch.empty(self.plan.count, Xq.shape[0], dtype=torch.int32, device=Xq.device)
        scores, per = self._score(Xq, fitting=False, best=best)
        out = (scores.cpu().numpy(),) + ((per.cpu().numpy(),) if return_per_subspace else ())
        return out + (best.cpu().numpy(),)

    def fit(self, X, y=None):
        """The distance matrices, the radii, the counts and sums and the scores of X itself: decision_scores_ (float64 [n]),
        per_subspace_scores_, radii_, best_radius_, neighbor_counts_, flagged_, n_flagged_; with normalize also score_center_ /
        score_scale_.  X stays resident as the fitted rows."""
        self._X = X = self._begin_fit(X)
        n, S, R, dev = X.shape[0], self.plan.count, self.n_radii, X.device
        self._r = torch.empty(S, R, dtype=torch.float32, device=dev)
        self._a = torch.empty(S, R, dtype=torch.float32, device=dev)
        self._cnt = torch.empty(S, n, R, dtype=torch.int32, device=dev)
        per = torch.empty(S, n, dtype=torch.float32, device=dev)
        best = torch.empty(S, n, dtype=torch.int32, device=dev)
        kept, kept_sums = [None] * S, [[None] * S for _ in range(3)]
        for first, count, gram in loci_chunks(self.plan, n, R, self.workspace_bytes):
            D = self._distance_matrix(X, first, count, gram)
            self._set_radii(D, first, count)
            self._counts(D, first, count)
            sums = self._sums(D, first, count)
            self._finish(sums, first, count, per, best)
            if self.keep_distance_matrix:
                self._keep(kept, D, first)
            if self.keep_sums:
                for held, v in zip(kept_sums, sums):
                    self._keep(held, v, first)
            del D, sums
        g = self.plan.given
        self.radii_ = self._r.cpu().numpy()[g]
        self.neighbor_counts_ = self._cnt.cpu().numpy()[g]
        self.best_radius_ = best.cpu().numpy()
        if self.keep_distance_matrix:
            self.distance_matrix_ = kept
        if self.keep_sums:
            self.sampling_counts_, self.sum_counts_, self.sum_sq_counts_ = (np.stack(v) for v in kept_sums)
        self._publish(self._combine(per, fitting=True), per)
        self.flagged_ = self.per_subspace_scores_.astype(np.float64) > self.k_sigma
        self.n_flagged_ = self.flagged_.sum(axis=1).astype(np.int64)
        return self


# ---- deep isolation forest: isolation trees on random-MLP representations of the subspaces ------------------------------
DIF_MAX_REPRESENTATIONS = 256  # VGAN_DIF_MAX_NETS
DIF_MAX_HIDDEN = 3  # VGAN_DIF_MAX_HIDDEN
DIF_MAX_WIDTH = 512  # VGAN_DIF_MAX_WIDTH: an activation tile of 32 rows stays in LDS
DIF_MAX_DIM = 64  # VGAN_DIF_MAX_OUT
DIF_MAX_DIMS = 8192  # features of one subspace
DIF_MAX_ROWS = 1 << 24  # VGAN_DIF_MAX_ROWS (and VGAN_HIST_MAX_ROWS: the column range)
DIF_ROW_TILE = 32  # VGAN_DIF_ROW_TILE: rows of one workgroup of the forward
DIF_K_TILE = 64  # VGAN_DIF_K_TILE: features of one staged tile of layer 0
DIF_ACTIVATIONS = {"tanh": 0, "relu": 1}  # VGAN_DIF_ACT_*
DIF_PHILOX_TAG = 0x44494600  # counter word 2 of a weight draw is DIF_PHILOX_TAG + layer
_DIF_MAX_RANGE = 65535  # blocks of one launch (a grid dimension)


def check_representations(n_representations):
    if not (_is_int(n_representations) and 1 <= int(n_representations) <= DIF_MAX_REPRESENTATIONS):
        raise ValueError(f"n_representations must be an integer between 1 and {DIF_MAX_REPRESENTATIONS}, got {n_representations!r}")
    return int(n_representations)


def check_hidden(hidden):
    """A tuple of 0 to DIF_MAX_HIDDEN widths, each 1 .. DIF_MAX_WIDTH; () is a random linear projection."""
    try:
        widths = tuple(hidden)
    except TypeError:
        raise ValueError(f"hidden must be a tuple of at most {DIF_MAX_HIDDEN} widths, got {hidden!r}") from None
    if len(widths) > DIF_MAX_HIDDEN:
        raise ValueError(f"hidden must hold at most {DIF_MAX_HIDDEN} widths, got {len(widths)}")
    for w in widths:
        if not (_is_int(w) and 1 <= int(w) <= DIF_MAX_WIDTH):
            raise ValueError(f"a hidden width must be an integer between 1 and {DIF_MAX_WIDTH}, got {w!r}")
    return tuple(int(w) for w in widths)


def check_representation_dim(representation_dim):
    if not (_is_int(representation_dim) and 1 <= int(representation_dim) <= DIF_MAX_DIM):
        raise ValueError(f"representation_dim must be an integer between 1 and {DIF_MAX_DIM}, got {representation_dim!r}")
    return int(representation_dim)


def check_activation(activation):
    if activation not in DIF_ACTIVATIONS:
        raise ValueError(f"activation must be 'tanh' or 'relu', got {activation!r}")
    return activation


def dif_block_floats(dims, hidden, q):
    """int64, like dims: the float32 elements of one block's weights for a subspace of that many features: layer l stored as
    [K_l rounded up to 8, in quads][K_{l+1}][4], layer after layer (include/vgan_hip.h)."""
    k = (np.asarray(dims, dtype=np.int64) + 7) // 8 * 8
    total = np.zeros_like(k)
    for width in tuple(hidden) + (q,):
        total = total + width * k
        k = np.int64((width + 7) // 8 * 8)
    return total


def dif_chunks(weight_bytes, q, rows, workspace_bytes, whole_rows=False):
    """(blocks of a chunk, rows of a row chunk).  Per block the transient buffers hold its weights (weight_bytes: those of
    the widest subspace), and per row q float32 of R and one int64 sum, 4 q + 8 bytes.  While a block with all `rows` rows
    fits, as many blocks as fit form a chunk (at most 65535, a grid dimension) and the rows are not chunked; below that a
    chunk is one block and the rows are chunked, down to single rows; a row chunk never exceeds DIF_MAX_ROWS.  whole_rows (fit: the trees of a block are grown on its
    whole R) never chunks the rows and raises ValueError, naming the bytes, when one block's R does not fit."""
    ws, per_row = int(workspace_bytes), 4 * int(q) + 8
    if not whole_rows:
        rows = min(int(rows), DIF_MAX_ROWS)  # rows of one launch
    if whole_rows and int(rows) * 4 * int(q) > ws:
        raise ValueError(f"SubspaceDIF fit needs {int(rows) * 4 * int(q)} bytes of workspace for the representation of one block "
                         f"({rows} rows x {q} columns, float32), workspace_bytes is {ws}")
    block = int(weight_bytes) + int(rows) * per_row
    if whole_rows or block <= ws:
        return max(1, min(ws // block, _DIF_MAX_RANGE)), int(rows)
    return 1, max(1, min((ws - int(weight_bytes)) // per_row, int(rows)))


class SubspaceDIF(_SubspaceScorer):
    """Deep isolation forest per subspace (Xu, Pang, Wang, Wang: "Deep Isolation Forest for Anomaly Detection", TKDE 2023;
    pyod's ``DIF``), combined like the other detectors of this module: an ensemble of randomly initialised, never trained
    MLPs maps the rows of a subspace to small representations, and isolation trees are grown on every representation.
    Axis-parallel cuts in a random non-linear representation are oblique, curved cuts in the data, so rows that break a
    correlation structure while staying inside every marginal range are isolated early, where the plain isolation forest
    finds them late.  Like every isolation method it does not find outliers that sit INSIDE the data (the centre of a ring).
    Nothing is trained and no weight is stored: the nets are regenerated from the seed.  The defaults are pyod's
    (n_ensemble 50, n_estimators 6, max_samples 256, hidden_neurons [500, 100], representation_dim 20, tanh, no bias).  Not
    built: the paper's deviation-enhanced score (DEAS), pyod's ``skip_connection``, other activations.

    Sizes.  X is cast to float32.  S subspaces, r = n_representations (1 .. 256), T = n_estimators (1 .. 1024); psi =
    ``max_samples_`` = min(max_samples, n), max_samples "auto" (256) or 2 .. 1024 (SubspaceIForest's rule); q =
    representation_dim (1 .. 64); hidden a tuple of 0 to 3 widths, each 1 .. 512 (() is a random linear projection);
    activation "tanh" or "relu"; seed in [0, 2^64); a subspace has at most 8192 features; ``fit`` takes 2 .. 2^24 rows.

    Scaling.  At ``fit``, per feature f, lo_f and hi_f are the float32 min and max over the fitted rows, -0.0 taken as +0.0
    (``feature_min_``, ``feature_max_``, float32 [d]); z = float32((double(x) - double(lo_f)) / (double(hi_f) - double(lo_f))),
    exactly 0 for a constant column.  New rows use the stored lo and hi and are not clipped.  (The data here is not
    standardised, and an unscaled input saturates tanh.)

    Nets.  Block b = s r + j is representation j of the given subspace index s.  Its net has the layer sizes K_0 = d_s, the
    hidden widths, q; no bias; the activation after every layer but the last; no skip connection.  The weight W_l[o, i] of
    block b has the linear index e = o K_l + i (for layer 0, i is the position in the subspace's ascending feature list).
    With the Philox4x32-10 words of

        counter (lo32(e >> 2), hi32(e >> 2), 0x44494600 + l, 0),  key k0 = lo32(seed) ^ lo32(b),  k1 = hi32(seed) ^ hi32(b) ^ 0x5bd1e995

    (the key convention of the noise stream and of SubspaceIForest), w = word e & 3, u = (w + 0.5) 2^-32 in float64 and
    W = float32((2 u - 1) c_l), c_l = 1 / sqrt(K_l) formed on the host in float64: torch's default ``nn.Linear`` init,
    U(-1 / sqrt(fan_in), 1 / sqrt(fan_in)).  The nets are keyed by the subspace's POSITION: a subspace fitted alone (position
    0) gets other nets than the same subspace at position 3.

    Representation.  R[b, i, :] is the net of block b applied to z of row i restricted to F_s.  Products accumulate in
    float32 on the fp32-input matrix unit; tanh is float32(tanh(double(a))) of the float32 pre-activation a, relu is
    max(a, 0).  An element of R depends on its row, its block and its column only: it is bit-identical from run to run, for
    every split of the rows or blocks over launches (so for every workspace_bytes) and whichever other blocks share a launch.

    Trees.  For every block, T trees are grown on the float32 matrix R[b] [n, q], all q columns candidates, by the rules
    of SubspaceIForest exactly (sampling by feistel_perm, the Philox node words, thresholds, the depth limit L = ceil(log2
    psi), leaves), with the stream id = b T + t.  sum[b, i] is that class's int64 fixed-point path sum, and the subspace pools
    its r T trees:

        score[s, i] = float32(exp2(-(double(sum_j sum[s r + j, i]) / double(r T cq[psi]))))

    in (0, 1].  A subspace of constant features has R = 0, every tree one leaf of psi rows, and scores exactly 0.5.
    ``decision_function(X_train)`` equals ``decision_scores_`` bit for bit.  Scores, trees and R are bit-identical from run to
    run and for every workspace_bytes, which bounds the transient buffers (dif_chunks: weights, R and sums of a chunk of
    blocks), not the trees; ``fit`` raises ValueError, naming the bytes, when the R of one block does not fit it.  NaN input
    leaves the results unspecified and neither faults nor hangs.

    Fitted state: the trees, lo, hi and the seed; no weights and no X.  ``fit`` publishes, copied to the host on first use,
    ``tree_feature_`` int32 [S, r, T, N] (the split column of the representation, 0 .. q - 1; -1 a leaf, -2 an absent slot),
    ``tree_threshold_`` float32 and ``tree_size_`` int32 of the same shape, N = 2^(L + 1); and ``max_samples_``,
    ``depth_limit_``, ``feature_min_``, ``feature_max_``.  ``representation(X, s, j)`` returns R of block s r + j as float32
    [n, q] and ``layer_weights(s, j)`` its weights as float32 [K_{l + 1}, K_l] per layer: both are for inspection and tests.
    normalize, combination, contamination, ``threshold_``, ``labels_``, ``predict``, ``predict_proba`` and
    return_per_subspace are the shared tail.  pyod is not pinned here: this definition and its numpy restatement in
    tests/test_outlier_dif_cpu.py are what binds.  All of it runs in libvgan_hip.so (csrc/outlier_dif.hip for the weights and
    the fused forward, csrc/outlier_iforest.hip for the trees)."""

    _host_trees = None

    def __init__(self, subspaces, proba, n_representations=50, n_estimators=6, max_samples="auto", hidden=(500, 100),
                 representation_dim=20, activation="tanh", seed=0, workspace_bytes=DEFAULT_WORKSPACE_BYTES, normalize=None,
                 combination="sum", contamination=0.1):
        self.n_representations = check_representations(n_representations)
        self.n_estimators = check_estimators(n_estimators)
        self.max_samples = max_samples
        self._max_samples = check_max_samples(max_samples)
        self.hidden = check_hidden(hidden)
        self.representation_dim = check_representation_dim(representation_dim)
        self.activation = check_activation(activation)
        self.seed = check_seed(seed)
        # no distance engine here: "exact" for every subspace keeps the processing order the given order
        self._configure(subspaces, proba, "exact", workspace_bytes, normalize, combination, contamination)
        del self.engine
        if int(self.plan.dims.max()) > DIF_MAX_DIMS:
            raise ValueError(f"a subspace has {int(self.plan.dims.max())} features, SubspaceDIF takes at most {DIF_MAX_DIMS}")
        self._net = (self.n_representations, self.hidden, self.representation_dim, DIF_ACTIVATIONS[self.activation])
        self._block_floats = dif_block_floats(self.plan.dims, self.hidden, self.representation_dim)  # per subspace
        self._weight_bytes = 4 * int(self._block_floats.max())

    def _check_fit_rows(self, n):
        if not 2 <= n <= DIF_MAX_ROWS:
            raise ValueError(f"SubspaceDIF fit needs between 2 and {DIF_MAX_ROWS} rows, got {n}")

    def _attach(self):
        if self.ops is not None:
            return
        super()._attach()
        widths = np.asarray(self.hidden + (self.representation_dim,), dtype=np.float64)
        scale = np.empty((self.plan.count, len(widths)), dtype=np.float64)
        scale[:, 0] = 1.0 / np.sqrt(self.plan.dims.astype(np.float64))
        scale[:, 1:] = 1.0 / np.sqrt(widths[:-1])
        self._scale = torch.as_tensor(scale, device="cuda")

    def _weights(self, first, count, W=None):
        """(W, w_off) of the blocks first .. first + count - 1, W filled on the device."""
        sizes = self._block_floats[np.arange(first, first + count) // self.n_representations]
        off = np.concatenate([[0], np.cumsum(sizes)])
        total = int(off[-1])
        if W is None:
            W = torch.empty(total, dtype=torch.float32, device="cuda")
        w_off = torch.as_tensor(off[:-1].astype(np.int64), device="cuda")
        self.ops.dif_weights(self._table[1], self._net, first, count, self._scale, self.seed, W, w_off, total)
        return W, w_off

    def layer_weights(self, s, j):
        """The weights of representation j of subspace s: a list of float32 [K_{l + 1}, K_l], one per layer."""
        s, j = int(s), int(j)
        if not (0 <= s < self.plan.count and 0 <= j < self.n_representations):
            raise ValueError(f"no representation {j} of subspace {s}: {self.plan.count} subspaces of {self.n_representations}")
        self._attach()
        flat = self._weights(s * self.n_representations + j, 1)[0].cpu().numpy()
        out, at, k = [], 0, int(self.plan.dims[s])
        for width in self.hidden + (self.representation_dim,):
            ld = (k + 7) // 8 * 8
            out.append(flat[at:at + width * ld].reshape(ld // 4, width, 4).transpose(1, 0, 2).reshape(width, ld)[:, :k].copy())
            at, k = at + width * ld, width
        return out

    def representation(self, X, s, j):
        """float32 [n, q]: R of block s r + j for the rows of X, scaled by the fitted lo and hi."""
        self._require_fit()
        s, j = int(s), int(j)
        if not (0 <= s < self.plan.count and 0 <= j < self.n_representations):
            raise ValueError(f"no representation {j} of subspace {s}: {self.plan.count} subspaces of {self.n_representations}")
        X = _device_matrix(X, self.plan.d)
        b = s * self.n_representations + j
        W, w_off = self._weights(b, 1)
        R = torch.empty(1, X.shape[0], self.representation_dim, dtype=torch.float32, device=X.device)
        self.ops.dif_represent(X, self._table, self._lo, self._hi, self._net, b, 1, W, w_off, R)
        return R[0].cpu().numpy()

    def path_sums(self, X):
        """int64 [S, n]: the fixed-point path-length sums of the rows of X over the r T trees of every subspace."""
        self._require_fit()
        return self._pooled_sums(_device_matrix(X, self.plan.d), build=False).cpu().numpy()

    def _pooled_sums(self, X, build):
        """int64 [S, nq]: the path sums of the rows of X pooled over the r blocks of every subspace, chunk of blocks by chunk
        of blocks and row chunk by row chunk; build: grows the trees of every block on its R first (all rows in one chunk)."""
        nq, dev = X.shape[0], X.device
        r, q, psi, L = self.n_representations, self.representation_dim, self.max_samples_, self.depth_limit_
        blocks, rows = dif_chunks(self._weight_bytes, q, nq, self.workspace_bytes, whole_rows=build)
        n_blocks = self.plan.count * r
        blocks = min(blocks, n_blocks)
        pooled = torch.zeros(self.plan.count, nq, dtype=torch.int64, device=dev)
        W = torch.empty(blocks * (self._weight_bytes // 4), dtype=torch.float32, device=dev)
        R = torch.empty(blocks * rows * q, dtype=torch.float32, device=dev)
        sums = torch.empty(blocks * rows, dtype=torch.int64, device=dev)
        for first in range(0, n_blocks, blocks):
            count = min(blocks, n_blocks - first)
            _, w_off = self._weights(first, count, W)
            owner = torch.arange(first, first + count, device=dev) // r
            for r0 in range(0, nq, rows):
                m = min(rows, nq - r0)
                Rc = R[:count * m * q].view(count, m, q)
                self.ops.dif_represent(X[r0:r0 + m], self._table, self._lo, self._hi, self._net, first, count, W, w_off, Rc)
                if build:
                    self.ops.iforest_build_blocks(Rc, first, psi, L, self.seed, self._flat_trees)
                self.ops.iforest_path_sums_blocks(Rc, self._flat_trees, first, psi, L, self._cq, sums)
                pooled[:, r0:r0 + m].index_add_(0, owner, sums[:count * m].view(count, m))  # int64: exact in any order
        return pooled

    def _scores(self, X, fitting):
        pooled = self._pooled_sums(X, build=fitting)
        per = torch.empty(self.plan.count, X.shape[0], dtype=torch.float32, device=X.device)
        for s0 in range(0, self.plan.count, _IFOREST_MAX_RANGE):
            s1 = min(s0 + _IFOREST_MAX_RANGE, self.plan.count)
            self.ops.iforest_scores(pooled[s0:s1], s1 - s0, X.shape[0], self._denom, per[s0:s1])
        return self._combine(per, fitting), per

    def _score(self, X, fitting):
        return self._scores(X, False)

    _trees_on_host = SubspaceIForest._trees_on_host

    @property
    def tree_feature_(self):
        """int32 [S, r, T, N]: the split column of the representation of every heap slot, -1 for a leaf, -2 for an absent slot."""
        return self._trees_on_host()[0]

    @property
    def tree_threshold_(self):
        """float32 [S, r, T, N]: the threshold of every internal node (a row goes left iff R <= threshold), 0 elsewhere."""
        return self._trees_on_host()[1]

    @property
    def tree_size_(self):
        """int32 [S, r, T, N]: the sample rows reaching every node, 0 where the slot is absent."""
        return self._trees_on_host()[2]

    def fit(self, X, y=None):
        """Takes the column ranges of X, then block by block regenerates the net, forms R for all rows, grows the T trees on
        it and walks the rows through them: decision_scores_ (float64 [n]), per_subspace_scores_, max_samples_, depth_limit_,
        feature_min_, feature_max_ and, on first use, tree_feature_ / tree_threshold_ / tree_size_; with normalize also
        score_center_ / score_scale_.  The trees, lo and hi are the fitted state: neither X nor any weight is kept."""
        n = _matrix_shape(X, self.plan.d)[0]
        self._check_fit_rows(n)
        dif_chunks(self._weight_bytes, self.representation_dim, n, self.workspace_bytes, whole_rows=True)  # raises before the device is touched
        X = self._begin_fit(X)
        d, dev = X.shape[1], X.device
        keys = torch.empty(d, 2, dtype=torch.int64, device=dev)
        self.ops.hist_column_range(X, keys)  # keys of the float64 images of the float32 min and max, -0.0 as +0.0
        k = keys.cpu().numpy().view(np.uint64)
        bits = np.where(k >> np.uint64(63), k & np.uint64(0x7FFFFFFFFFFFFFFF), ~k)
        lo_hi = np.ascontiguousarray(bits).view(np.float64).astype(np.float32)
        self.feature_min_, self.feature_max_ = lo_hi[:, 0].copy(), lo_hi[:, 1].copy()
        self._lo, self._hi = torch.as_tensor(self.feature_min_, device=dev), torch.as_tensor(self.feature_max_, device=dev)
        psi = min(self._max_samples, n)
        self.max_samples_, self.depth_limit_, self._host_trees = psi, (psi - 1).bit_length(), None
        cq = iforest_path_table(psi)
        self._cq = torch.as_tensor(cq, device=dev)
        self._denom = self.n_representations * self.n_estimators * int(cq[psi])
        self._trees = torch.empty(self.plan.count, self.n_representations, self.n_estimators, 2 << self.depth_limit_, 2,
                                  dtype=torch.int32, device=dev)
        self._flat_trees = self._trees.view(self.plan.count * self.n_representations, self.n_estimators, 2 << self.depth_limit_, 2)
        self._fitted = False
        scores, per = self._scores(X, True)
        return self._publish(scores, per)


# ---- autoencoders: one small MLP per subspace, trained on the device, the reconstruction distance as the score ---------
AE_MAX_HIDDEN = 3  # VGAN_AE_MAX_HIDDEN: encoder widths; the net has twice as many layers
AE_MAX_WIDTH = 128  # VGAN_AE_MAX_WIDTH
AE_MAX_DIMS = 1024  # VGAN_AE_MAX_DIMS: features of one subspace (the SubspaceMahalanobis limit)
AE_MAX_BATCH = 256  # VGAN_AE_MAX_BATCH
AE_MAX_ROWS = 1 << 24  # VGAN_AE_MAX_ROWS
AE_ROW_TILE = 32  # VGAN_AE_ROW_TILE: rows of one workgroup of the scoring forward
AE_LDS_FLOATS = 38912  # VGAN_AE_LDS_FLOATS: the activations of a batch stay in LDS up to here, else in a scratch slice
AE_ACTIVATIONS = {"tanh": 0, "relu": 1}  # VGAN_AE_ACT_*
AE_PHILOX_TAG = 0x41450000  # counter word 2 of an initial draw is AE_PHILOX_TAG + layer
AE_MAX_LAUNCH_STEPS = 65536  # VGAN_AE_MAX_LAUNCH_STEPS
# Multiply-adds of one training launch of one net (a step costs 3 B P of them: forward, passed-down error, gradient): a launch
# runs AE_LAUNCH_MACS // (3 B P) steps, at least one.  Measured on an MI355X: the largest net (d_s 1024, hidden (128, 128, 128),
# B 256: 3.1e8 a step, so one step a launch) takes 12.1 ms a launch with 8 nets in flight and 36.0 ms with 256 (their
# activations in the scratch buffer); the default net at d_s = 375 (B 32, 51 to 53 steps a launch) 8.0 ms with 50 nets and 9.6
# ms with 256.  All far below a second on a shared machine.
AE_LAUNCH_MACS = 1 << 28
_AE_MAX_RANGE = 65535  # blocks of one launch (a grid dimension)


def check_ae_hidden(hidden):
    """A tuple of 1 to AE_MAX_HIDDEN encoder widths, each 1 .. AE_MAX_WIDTH; the decoder mirrors it."""
    try:
        widths = tuple(hidden)
    except TypeError:
        raise ValueError(f"hidden must be a tuple of 1 to {AE_MAX_HIDDEN} widths, got {hidden!r}") from None
    if not 1 <= len(widths) <= AE_MAX_HIDDEN:
        raise ValueError(f"hidden must hold between 1 and {AE_MAX_HIDDEN} widths, got {len(widths)}")
    for w in widths:
        if not (_is_int(w) and 1 <= int(w) <= AE_MAX_WIDTH):
            raise ValueError(f"a hidden width must be an integer between 1 and {AE_MAX_WIDTH}, got {w!r}")
    return tuple(int(w) for w in widths)


def check_ae_params(epochs, batch_size, lr, beta1, beta2, eps, weight_decay):
    if not (_is_int(epochs) and int(epochs) >= 0):
        raise ValueError(f"epochs must be a non-negative integer, got {epochs!r}")
    if not (_is_int(batch_size) and 1 <= int(batch_size) <= AE_MAX_BATCH):
        raise ValueError(f"batch_size must be an integer between 1 and {AE_MAX_BATCH}, got {batch_size!r}")
    if not (_is_real(lr) and 0.0 <= float(lr) < float("inf")):
        raise ValueError(f"lr must be a non-negative number, got {lr!r}")
    for name, beta in (("beta1", beta1), ("beta2", beta2)):
        if not (_is_real(beta) and 0.0 <= float(beta) < 1.0):
            raise ValueError(f"{name} must be a number in [0, 1), got {beta!r}")
    if not (_is_real(eps) and 0.0 < float(eps) < float("inf")):
        raise ValueError(f"eps must be a positive number, got {eps!r}")
    if not (_is_real(weight_decay) and 0.0 <= float(weight_decay) < float("inf")):
        raise ValueError(f"weight_decay must be a non-negative number, got {weight_decay!r}")
    return int(epochs), int(batch_size), float(lr), float(beta1), float(beta2), float(eps), float(weight_decay)


def ae_layer_sizes(d_s, hidden):
    """[(K_l, N_l)] of the net of a subspace of d_s features: d_s, the encoder widths, mirrored, d_s."""
    widths = [int(d_s)] + [int(w) for w in hidden] + [int(w) for w in tuple(hidden)[-2::-1]] + [int(d_s)]
    return list(zip(widths[:-1], widths[1:]))


def _mlp_param_count(sizes, bias):
    """P of a net of the layer sizes [(K_l, N_l)]: sum_l (K_l + bias) N_l, bias 1 or 0."""
    return sum((K + int(bias)) * N for K, N in sizes)


def _mlp_act_floats(sizes, widest, rows, train, output_kept):
    """The float32 cells of the activations of `rows` rows (pitches are widths | 1) of a net of the layer sizes [(K_l, N_l)]:
    z, every layer's output (the last one's only when training, as the output error, unless the scoring forward keeps it
    too: output_kept) and, when training, one passed-down error of the widest given width (csrc/outlier_mlp.hpp)."""
    per_row = (sizes[0][0] | 1) + sum(N | 1 for _, N in sizes[:-1]) + ((sizes[-1][1] | 1) if train or output_kept else 0)
    return (per_row + ((int(widest) | 1) if train else 0)) * int(rows)


def _mlp_net_bytes(params, act):
    """12 P and, when the `act` activation cells of a batch do not fit AE_LDS_FLOATS, the net's slice of the scratch buffer."""
    return 12 * params + (4 * act if act > AE_LDS_FLOATS else 0)


def ae_param_count(d_s, hidden):
    """P: the parameters of one net, sum_l (K_l + 1) N_l."""
    return _mlp_param_count(ae_layer_sizes(d_s, hidden), True)


def ae_act_floats(d_s, hidden, rows, train):
    """The float32 cells of the activations of `rows` rows (pitches are widths | 1): z and the hidden layers and, when
    training, the output error and one passed-down error of the widest hidden layer (csrc/outlier_mlp.hpp)."""
    return _mlp_act_floats(ae_layer_sizes(d_s, hidden), max(hidden), rows, train, False)


def ae_net_bytes(d_s, hidden, batch, max_dims=None):
    """The bytes one net needs while it trains: theta, m and v (12 P) and, when the activations of a batch of the widest
    subspace (max_dims, default d_s) do not fit AE_LDS_FLOATS, its slice of the scratch buffer."""
    return _mlp_net_bytes(ae_param_count(d_s, hidden), ae_act_floats(d_s if max_dims is None else max_dims, hidden, batch, True))


def ae_chunks(net_bytes, workspace_bytes, owner="SubspaceAutoEncoder"):
    """[(first, count)]: consecutive runs of nets whose training state fits workspace_bytes, at most 65535 each; every chunk
    trains to the end before the next begins.  ValueError, naming the bytes (and the owner class), when one net alone does
    not fit."""
    out, first, ws = [], 0, int(workspace_bytes)
    sizes = [int(v) for v in net_bytes]
    for s, need in enumerate(sizes):
        if need > ws:
            raise ValueError(f"{owner} needs {need} bytes of workspace for the net of subspace {s} with its moments, "
                             f"workspace_bytes is {ws}")
    while first < len(sizes):
        end, used = first, 0
        while end < len(sizes) and end - first < _AE_MAX_RANGE and used + sizes[end] <= ws:
            used += sizes[end]
            end += 1
        out.append((first, end - first))
        first = end
    return out


def ae_launch_steps(params, batch):
    """The steps of one training launch for nets of at most `params` parameters: AE_LAUNCH_MACS // (3 B P), 1 .. 65536."""
    return int(max(1, min(AE_LAUNCH_MACS // (3 * int(batch) * int(params)), AE_MAX_LAUNCH_STEPS)))


def ae_bias_corrections(beta1, beta2, steps):
    """float64 [steps, 2]: 1 - beta1^t and 1 - beta2^t for t = 1 .. steps (numpy's float64 power)."""
    t = np.arange(1, int(steps) + 1, dtype=np.float64)
    return np.stack([1.0 - np.float64(beta1) ** t, 1.0 - np.float64(beta2) ** t], axis=1)


class _MlpScorer(_SubspaceScorer):
    """One small MLP per subspace, trained on the device by Adam on mini-batches of the standardised rows, the shared part of
    SubspaceAutoEncoder and SubspaceDeepSVDD (whose docstrings are the definitions): the arguments, the scaling, the chunks of
    nets that each train to the end, the cut of the steps into launches, the scoring forward over row tiles and the weights.
    A subclass sets the traits below; what it adds to a chunk, a train launch or a scoring launch goes through _begin_chunk and
    _target.  All of it runs in libvgan_hip.so (csrc/outlier_mlp.hpp)."""

    _layer_sizes = None  # staticmethod (d_s, hidden) -> [(K_l, N_l)]
    _bias = None  # a bias in every layer: weights_ holds (W_l, b_l) pairs, else W_l alone
    _output_kept = None  # the scoring forward keeps the last layer's output among the activations
    _entries = None  # the names of ops' init, train and scores
    _raw = None  # ops' scores takes the buffer of the raw output under this keyword
    _host_weights = None

    def __init__(self, subspaces, proba, hidden, activation, epochs, batch_size, lr, beta1, beta2, eps, weight_decay, seed, workspace_bytes,
                 normalize, combination, contamination):
        self.hidden = check_ae_hidden(hidden)
        self.activation = check_activation(activation)
        (self.epochs, self.batch_size, self.lr, self.beta1, self.beta2, self.eps,
         self.weight_decay) = check_ae_params(epochs, batch_size, lr, beta1, beta2, eps, weight_decay)
        self.seed = check_seed(seed)
        # no distance engine here: "exact" for every subspace keeps the processing order the given order
        self._configure(subspaces, proba, "exact", workspace_bytes, normalize, combination, contamination)
        del self.engine
        self._max_dims = int(self.plan.dims.max())
        if self._max_dims > AE_MAX_DIMS:
            raise ValueError(f"a subspace has {self._max_dims} features, {type(self).__name__} takes at most {AE_MAX_DIMS}")
        self._net = (self.hidden, AE_ACTIVATIONS[self.activation])
        self._params = np.array([_mlp_param_count(self._layer_sizes(d_s, self.hidden), self._bias) for d_s in self.plan.dims], dtype=np.int64)

    def _act_floats(self, rows, train):
        """The activation cells of `rows` rows of the widest subspace: what a launch reserves per workgroup."""
        return _mlp_act_floats(self._layer_sizes(self._max_dims, self.hidden), max(self.hidden), rows, train, self._output_kept)

    def _check_fit_rows(self, n):
        if not 2 <= n <= AE_MAX_ROWS:
            raise ValueError(f"{type(self).__name__} fit needs between 2 and {AE_MAX_ROWS} rows, got {n}")

    def _attach(self):
        if self.ops is not None:
            return
        super()._attach()
        fan_in = np.array([[K for K, _ in self._layer_sizes(d_s, self.hidden)] for d_s in self.plan.dims], dtype=np.float64)
        self._init_scale = torch.as_tensor(1.0 / np.sqrt(fan_in), device="cuda")
        self._w_off_host = np.concatenate([[0], np.cumsum(self._params)]).astype(np.int64)
        self._w_off = torch.as_tensor(self._w_off_host[:-1].copy(), device="cuda")

    def _column_moments(self, X):
        """(mean, variance) float64 [d] on the host: vgan_maha_moments over the d one-feature subspaces, the two-pass slab sums
        whose bits depend on n alone."""
        n, d = X.shape
        dev = X.device
        ones = np.ones(d, dtype=np.int64)
        table = (torch.arange(d, dtype=torch.int32, device=dev), torch.arange(d + 1, dtype=torch.int32, device=dev),
                 torch.arange(d + 1, dtype=torch.int64, device=dev))
        cells, ranges = maha_ranges(ones, self.workspace_bytes)
        mean, var = (torch.empty(d, dtype=torch.float64, device=dev) for _ in range(2))
        hcount = torch.full((d,), n, dtype=torch.int32, device=dev)
        slabs = -(-n // MAHA_SLAB_ROWS)
        for first, count in ranges:
            tiles = torch.as_tensor(maha_tiles(ones, first, count), device=dev)
            ws = torch.empty(min(cells, slabs * MAHA_TILE * MAHA_TILE * count), dtype=torch.float64, device=dev)
            self.ops.maha_moments(X, table, first, count, count, 1, tiles, None, hcount, mean, var, ws)
        return mean.cpu().numpy(), var.cpu().numpy()

    def _fit_scaling(self, X):
        """location_, scale_ (sd 1 for a constant column), their device copies and the flags of the constant subspaces."""
        dev = X.device
        mean, var = self._column_moments(X)
        self.location_ = mean
        with np.errstate(invalid="ignore"):
            self.scale_ = np.where(var > 0.0, np.sqrt(var), 1.0)
        self._scaling = (torch.as_tensor(self.location_, device=dev), torch.as_tensor(self.scale_, device=dev))
        off = self.plan.feat_off
        self._constant = np.array([not (var[self.plan.feat[off[s]:off[s + 1]]] != 0.0).any() for s in range(self.plan.count)])
        self._skip = torch.as_tensor(self._constant.astype(np.int32), device=dev)

    def _forward_tiles(self, nq, widest, extra_bytes=0):
        """(row tiles of one forward launch over `widest` blocks, its scratch buffer or None): all tiles of nq rows, or as many
        as keep the scratch slices (and extra_bytes per (block, tile)) within workspace_bytes, at least one."""
        act = self._act_floats(AE_ROW_TILE, False)
        spill = act > AE_LDS_FLOATS
        tiles = -(-nq // AE_ROW_TILE)
        per_tile = (4 * act if spill else 0) + extra_bytes
        if per_tile:
            tiles = int(max(1, min(tiles, self.workspace_bytes // (per_tile * widest))))
        scratch = torch.empty(widest * tiles * act, dtype=torch.float32, device="cuda") if spill else None
        return tiles, scratch

    def _begin_fit_state(self, dev):
        """What a subclass allocates per fit beside the weights."""

    def _begin_chunk(self, X, first, count, state, s_off):
        """What a subclass takes from the initialised, untrained nets of a chunk."""

    def _target(self, first, count):
        """The arguments a subclass's train and scores entries take for the blocks first .. first + count - 1, as a tuple."""
        return ()

    def _train(self, X, batch, chunks):
        """Initialises every chunk of nets and trains it to the end; the weights go to _theta, the step losses to the returned
        [S, steps] matrix."""
        n, dev = X.shape[0], X.device
        S, steps = self.plan.count, self.epochs * (n // batch)
        init, train, _ = (getattr(self.ops, name) for name in self._entries)
        corr = torch.as_tensor(ae_bias_corrections(self.beta1, self.beta2, steps), device=dev)
        loss = torch.zeros(S, max(steps, 1), dtype=torch.float32, device=dev)
        adam = (self.lr, self.beta1, self.beta2, self.eps, self.weight_decay)
        act = self._act_floats(batch, True)
        for first, count in chunks:
            sizes = self._params[first:first + count]
            off = np.concatenate([[0], np.cumsum(3 * sizes)]).astype(np.int64)
            state = torch.empty(int(off[-1]), dtype=torch.float32, device=dev)
            s_off = torch.as_tensor(off[:-1].copy(), device=dev)
            init(self._table[1], self._net, first, count, self._init_scale, self.seed, state, s_off, int(off[-1]))
            self._begin_chunk(X, first, count, state, s_off)
            scratch = torch.empty(count * act, dtype=torch.float32, device=dev) if act > AE_LDS_FLOATS else None
            per_launch = ae_launch_steps(int(sizes.max()), batch)
            for g0 in range(0, steps, per_launch):
                train(X, self._table, self._scaling, self._skip, self._net, first, count, self._max_dims, batch, self.seed, g0,
                      corr[g0:g0 + per_launch], adam, *self._target(first, count), state, s_off, loss[first:first + count], scratch)
            for z in range(count):
                at = int(self._w_off_host[first + z])
                self._theta[at:at + int(sizes[z])].copy_(state[int(off[z]):int(off[z]) + int(sizes[z])])
            del state, scratch
        return loss[:, :steps]

    def _distances(self, X, only=None):
        """float32 [S, nq] on the device: the scores of the rows of X under every net; only = s: the raw output of net s
        [nq, its output width] instead."""
        nq, dev = X.shape[0], X.device
        scores = getattr(self.ops, self._entries[2])
        ranges = list(_launch_ranges(self.plan.count, _AE_MAX_RANGE)) if only is None else [(only, 1)]
        tiles, scratch = self._forward_tiles(nq, max(count for _, count in ranges))
        rows = tiles * AE_ROW_TILE
        if only is None:
            out = torch.empty(self.plan.count, nq, dtype=torch.float32, device=dev)
        else:
            out = torch.empty(nq, self._layer_sizes(int(self.plan.dims[only]), self.hidden)[-1][1], dtype=torch.float32, device=dev)
        for first, count in ranges:
            for r0 in range(0, nq, rows):
                where = {"score": out[first:first + count, r0:]} if only is None else {self._raw: out[r0:r0 + rows]}
                scores(X[r0:r0 + rows], self._table, self._scaling, self._skip, self._net, first, count, self._max_dims, self._theta,
                       self._w_off[first:first + count], *(self._target(first, count) if only is None else ()), scratch=scratch, **where)
        return out

    def _score(self, X, fitting):
        per = self._distances(X)
        return self._combine(per, fitting), per

    def _output(self, X, s):
        """float32 [n, width] on the host: the raw output of the net of subspace s on the rows of X."""
        self._require_fit()
        s = int(s)
        if not 0 <= s < self.plan.count:
            raise ValueError(f"no subspace {s}: {self.plan.count} subspaces")
        return self._distances(_device_matrix(X, self.plan.d), only=s).cpu().numpy()

    @property
    def weights_(self):
        """List of S lists with one entry per layer: (W_l float32 [N_l, K_l], b_l float32 [N_l]) with a bias, else W_l."""
        self._require_fit()
        if self._host_weights is None:
            flat, out = self._theta.cpu().numpy(), []
            for s, d_s in enumerate(self.plan.dims):
                at, layers = int(self._w_off_host[s]), []
                for K, N in self._layer_sizes(d_s, self.hidden):
                    W = flat[at:at + K * N].reshape(K, N).T.copy()
                    layers.append((W, flat[at + K * N:at + (K + 1) * N].copy()) if self._bias else W)
                    at += (K + int(self._bias)) * N
                out.append(layers)
            self._host_weights = out
        return self._host_weights

    def _publish_fit_state(self):
        """What a subclass publishes after the training beside the losses."""

    def fit(self, X, y=None):
        """Takes the column means and deviations of X, then chunk of subspaces by chunk initialises the nets (Deep SVDD: and
        takes their centres) and runs all epochs (steps-per-launch by ae_launch_steps), and scores X through the trained
        nets: decision_scores_ (float64 [n]), per_subspace_scores_, location_, scale_, loss_history_, n_steps_, what the
        subclass publishes (center_, n_clamped_) and, on first use, weights_; with normalize also score_center_ / score_scale_."""
        n = _matrix_shape(X, self.plan.d)[0]
        self._check_fit_rows(n)
        batch = min(self.batch_size, n)
        act = self._act_floats(batch, True)
        chunks = ae_chunks([_mlp_net_bytes(int(P), act) for P in self._params], self.workspace_bytes,
                           type(self).__name__)  # raises before the device is touched
        X = self._begin_fit(X)
        self._fitted, self._host_weights = False, None
        self._fit_scaling(X)
        self._theta = torch.empty(int(self._w_off_host[-1]), dtype=torch.float32, device=X.device)
        self._begin_fit_state(X.device)
        steps = n // batch
        self.n_steps_ = self.epochs * steps
        loss = self._train(X, batch, chunks).cpu().numpy().astype(np.float64).reshape(self.plan.count, self.epochs, steps)
        self.loss_history_ = np.cumsum(loss, axis=2)[:, :, -1] / steps  # cumsum adds in step order
        self._publish_fit_state()
        scores, per = self._score(X, fitting=True)
        return self._publish(scores, per)


class SubspaceAutoEncoder(_MlpScorer):
    """Autoencoder per subspace (pyod's ``AutoEncoder``), combined like the other detectors of this module: a small MLP is
    trained to reconstruct the standardised rows of the subspace through a bottleneck, and a row is scored by the Euclidean
    norm of its reconstruction error.  It is the one detector here that LEARNS a representation: rows that leave a curved
    low-dimensional structure while staying inside every marginal range and close to the covariance ellipsoid are found by
    it and by none of the linear detectors.  All S nets train at once, one workgroup per net running many optimiser steps
    per launch.  The defaults are pyod's as remembered (hidden [64, 32], relu, 100 epochs, batch 32, Adam lr 1e-3, weight
    decay 1e-5).  Not built: dropout and batch normalisation (pyod's defaults use both), a validation split and early
    stopping, other optimisers and losses, several nets per subspace, a VAE.  The deep one-class objective is SubspaceDeepSVDD.

    Sizes.  X is cast to float32.  hidden: 1 to 3 encoder widths, each 1 .. 128; activation "relu" or "tanh"; batch_size 1 ..
    256; epochs >= 0; 0 <= beta1, beta2 < 1; eps > 0; lr, weight_decay >= 0; seed in [0, 2^64); a subspace has at most 1024
    features; ``fit`` takes 2 .. 2^24 rows.

    Scaling.  At ``fit``, per feature f, mean_f and the population variance are taken in float64, deterministically (the
    two-pass slab sums of SubspacePCA's ``location_`` and ``scale_``); sd_f = sqrt(variance), 1 where the variance is 0
    (sklearn's StandardScaler).  ``location_``, ``scale_``: float64 [d].  z = float32((double(x) - mean_f) / sd_f), exactly 0
    for a constant column.  New rows use the stored values.

    Net.  The subspace at position s has the layer sizes d_s, h_1 .. h_L, h_{L-1} .. h_1, d_s (2 L layers l = 0 .. 2 L - 1, layer
    l mapping K_l inputs to N_l outputs), a bias in every layer, the activation after every layer but the last, a linear
    output.  relu is max(a, 0); tanh is float32(tanh(double(a))) of the float32 pre-activation a (SubspaceDIF's).

    Initialisation.  torch's ``nn.Linear`` default, U(-1 / sqrt(K_l), 1 / sqrt(K_l)) for weights and biases, drawn as
    SubspaceDIF draws: with the Philox4x32-10 words of

        counter (lo32(e >> 2), hi32(e >> 2), 0x41450000 + l, 0),  key k0 = lo32(seed) ^ lo32(s),  k1 = hi32(seed) ^ hi32(s) ^ 0x5bd1e995

    w = word e & 3, u = (w + 0.5) 2^-32 in float64, value = float32((2 u - 1) c_l), c_l = 1 / sqrt(K_l) formed on the host in
    float64; W_l[o, i] has e = o K_l + i (for layer 0, i is the position in the ascending feature list), b_l[o] has e = N_l K_l +
    o.  m = v = 0.  The nets are keyed by the subspace's POSITION, like SubspaceDIF's.

    Batches.  B = min(batch_size, n); an epoch has n // B steps (the last partial batch is dropped); row j of step i of epoch e
    is feistel_perm(i B + j, n, seed, e), the same for every subspace.  The global step g = e (n // B) + i has t = g + 1.
    ``n_steps_`` = epochs (n // B).  epochs = 0 scores with the untrained net.

    One step, all in float32 unless said; fma(a, b, c) is a b + c rounded once.
      forward     pre_l[i, o] = (fma-chain over k ascending, from 0, of h_{l-1}[i, k] W_l[o, k]) + b_l[o]; h_l = act(pre_l), h_{-1} =
                  z, out = pre_{2L-1}.
      loss        r[i, f] = out[i, f] - z[i, f]; rowsum_i = fma-chain over f ascending of r r; loss = (sum over i ascending of
                  rowsum_i) / float32(B d_s): the batch loss before the update, the mean squared error.
      backward    D_{2L-1}[i, f] = r[i, f] float32(2 / (B d_s)) (the factor formed in float64); for l from the last layer down:
                  down[i, k] = fma-chain over o ascending of D_l[i, o] W_l[o, k] with the weights BEFORE their update;
                  D_{l-1}[i, k] = down[i, k] act'(h_{l-1}[i, k]), act' = (h > 0 ? 1 : 0) for relu and fma(-h, h, 1) for tanh.
      gradient    g = fma-chain over the batch rows i ascending of D_l[i, o] h_{l-1}[i, k]; for a bias the factor h is 1.
      Adam        g = fma(wd, theta, g); m = fma(b1, m, omb1 g); v = fma(b2, v, (omb2 g) g); theta = theta - (lrc m) / (sqrt(v) / sc2
                  + eps) with b1, b2, eps, wd the float32 roundings of beta1, beta2, eps, weight_decay, omb = float32(1 - beta)
                  formed in float64, lrc = float32(lr / c1_t), sc2 = float32(sqrt(c2_t)), c1_t = 1 - beta1^t and c2_t = 1 -
                  beta2^t formed ON THE HOST in float64 (numpy's power) and handed over per step: torch's
                  ``Adam(weight_decay=)``, with beta1 = 0 m is the gradient itself.  Weight decay acts on the biases too.
    No value depends on how the steps are cut into launches, on workspace_bytes (which cuts the subspaces into chunks that
    each train to the end: ae_chunks) or on the other subspaces of a launch: weights, losses and scores are bit-identical
    from run to run and across all of these.  ``fit`` raises ValueError, naming the bytes, when one net with its moments
    does not fit workspace_bytes.

    Score.  score[s, i] = float32(sqrt(sum_f (out[i, f] - z[i, f])^2)): the float32 differences squared and summed in float64
    in ascending f.  It depends on the row and the subspace only, and grows like sqrt(d_s): with subspaces of different sizes
    ``normalize`` is the argument to reach for.  ``fit`` scores the training rows through the trained net with the kernel of
    ``decision_function``, so ``decision_function(X_train)`` equals ``decision_scores_`` bit for bit.  A subspace whose features
    are all constant is not trained (its weights stay the initial ones, its losses are 0) and scores exactly 0.  NaN input
    leaves the results unspecified and neither faults nor hangs.

    Fitted state: the weights, ``location_``, ``scale_`` and the seed; neither X nor the moments are kept.  ``fit`` publishes
    ``weights_`` (a list of S lists of (W_l float32 [N_l, K_l], b_l float32 [N_l]), fetched on first use), ``loss_history_``
    (float64 [S, epochs]: the float32 step losses of an epoch summed in float64 in step order and divided by their number),
    ``n_steps_``, ``location_``, ``scale_``.  ``reconstruct(X, s)`` returns float32 [n, d_s], the output of net s on the
    standardised rows: for inspection and the tests.  normalize, combination, contamination, ``threshold_``, ``labels_``,
    ``predict``, ``predict_proba`` and return_per_subspace are the shared tail.  pyod is not pinned here: this definition and
    its numpy restatement in tests/test_outlier_ae_cpu.py are what binds.  All of it runs in libvgan_hip.so
    (csrc/outlier_ae.hip on the MLP core of csrc/outlier_mlp.hpp, which Deep SVDD shares; the column moments in
    csrc/outlier_maha.hip)."""

    _layer_sizes = staticmethod(ae_layer_sizes)
    _bias, _output_kept = True, False
    _entries, _raw = ("ae_init", "ae_train", "ae_scores"), "recon"

    def __init__(self, subspaces, proba, hidden=(64, 32), activation="relu", epochs=100, batch_size=32, lr=1e-3, beta1=0.9, beta2=0.999,
                 eps=1e-8, weight_decay=1e-5, seed=0, workspace_bytes=DEFAULT_WORKSPACE_BYTES, normalize=None, combination="sum",
                 contamination=0.1):
        super().__init__(subspaces, proba, hidden, activation, epochs, batch_size, lr, beta1, beta2, eps, weight_decay, seed, workspace_bytes,
                         normalize, combination, contamination)

    def reconstruct(self, X, s):
        """float32 [n, d_s]: the output of the net of subspace s on the rows of X, standardised by the fitted location_ and scale_."""
        return self._output(X, s)


# ---- Deep SVDD: one small encoder per subspace, trained on the device onto one point, the squared distance as the score ----------
SVDD_MAX_OUT = 128  # VGAN_SVDD_MAX_OUT: the output dimension q = hidden[-1] (AE_MAX_WIDTH)
SVDD_PHILOX_TAG = 0x53564400  # VGAN_SVDD_PHILOX_TAG: counter word 2 of an initial draw is SVDD_PHILOX_TAG + layer


def check_svdd_hidden(hidden):
    """A tuple of 1 to AE_MAX_HIDDEN layer widths, each 1 .. AE_MAX_WIDTH; the last is the output dimension q."""
    return check_ae_hidden(hidden)


def check_svdd_center(center, center_eps, count, q):
    """(center, center_eps): center None or a float32 [count, q] array built from a real array [q] (every subspace) or
    [count, q]; center_eps a finite number >= 0."""
    if not (_is_real(center_eps) and 0.0 <= float(center_eps) < float("inf")):
        raise ValueError(f"center_eps must be a non-negative number, got {center_eps!r}")
    if center is None:
        return None, float(center_eps)
    try:
        c = np.asarray(center, dtype=np.float64)
    except (TypeError, ValueError):
        raise ValueError(f"center must be None or a real array of shape ({q},) or ({count}, {q})") from None
    if c.shape == (q,):
        c = np.broadcast_to(c, (count, q))
    if c.shape != (count, q):
        raise ValueError(f"center must be None or a real array of shape ({q},) or ({count}, {q}), got shape {np.shape(center)}")
    return np.ascontiguousarray(c, dtype=np.float32), float(center_eps)


def svdd_layer_sizes(d_s, hidden):
    """[(K_l, N_l)] of the encoder of a subspace of d_s features: d_s, h_1 .. h_L."""
    widths = [int(d_s)] + [int(w) for w in hidden]
    return list(zip(widths[:-1], widths[1:]))


def svdd_param_count(d_s, hidden):
    """P: the parameters of one net, sum_l K_l N_l (no bias)."""
    return _mlp_param_count(svdd_layer_sizes(d_s, hidden), False)


def svdd_act_floats(d_s, hidden, rows, train):
    """The float32 cells of the activations of `rows` rows (pitches are widths | 1): z and every layer's output and, when
    training, one passed-down error of the widest layer (csrc/outlier_mlp.hpp)."""
    return _mlp_act_floats(svdd_layer_sizes(d_s, hidden), max(hidden), rows, train, True)


def svdd_net_bytes(d_s, hidden, batch, max_dims=None):
    """The bytes one net needs while it trains: theta, m and v (12 P) and, when the activations of a batch of the widest
    subspace (max_dims, default d_s) do not fit AE_LDS_FLOATS, its slice of the scratch buffer."""
    return _mlp_net_bytes(svdd_param_count(d_s, hidden), svdd_act_floats(d_s if max_dims is None else max_dims, hidden, batch, True))


class SubspaceDeepSVDD(_MlpScorer):
    """Deep SVDD per subspace (Ruff et al., ICML 2018, the one-class objective; pyod's ``DeepSVDD``), combined like the other
    detectors of this module: a small encoder WITHOUT BIAS is trained to map the standardised rows of the subspace onto one
    point c, and a row is scored by the squared distance of its image from c.  Where SubspaceAutoEncoder reconstructs a row
    through a bottleneck, this pulls the normal rows together and lets the others stay away.  All S nets train at once, one
    workgroup per net running many optimiser steps per launch.  Defaults: hidden (64, 32), relu, 100 epochs, batch 32, Adam
    lr 1e-3, weight decay 1e-5 (the autoencoder's).  Not built: the soft-boundary objective (``nu``, a radius), autoencoder
    pre-training (pyod's ``use_ae``), dropout, a validation split, pyod's ``l2_regularizer`` scale (its default 0.1 is not
    reproduced; the weight decay 1e-5 is the autoencoder's).

    Sizes.  X is cast to float32.  hidden: 1 to 3 widths, each 1 .. 128, the last is the output dimension q; activation
    "relu" or "tanh"; batch_size 1 .. 256; epochs >= 0; 0 <= beta1, beta2 < 1; eps > 0; lr, weight_decay, center_eps >= 0;
    seed in [0, 2^64); a subspace has at most 1024 features; ``fit`` takes 2 .. 2^24 rows.

    Scaling.  SubspaceAutoEncoder's exactly: float64 column mean and population deviation (``location_``, ``scale_``: float64
    [d]), sd 1 for a constant column, z = float32((double(x) - mean_f) / sd_f).  New rows use the stored values.

    Net.  The subspace at position s has the layer sizes d_s, h_1 .. h_L (L layers l = 0 .. L - 1, layer l mapping K_l inputs to
    N_l outputs), NO BIAS anywhere (with one the objective is minimised by a constant output), the activation after every
    layer but the last, a linear output of q = h_L coordinates.  relu is max(a, 0); tanh is float32(tanh(double(a))).

    Initialisation.  W_l[o, i] = float32((2 u - 1) c_l), c_l = 1 / sqrt(K_l) formed on the host in float64, e = o K_l + i, u = (w +
    0.5) 2^-32 in float64 with w the word e & 3 of Philox4x32-10 at

        counter (lo32(e >> 2), hi32(e >> 2), 0x53564400 + l, 0),  key k0 = lo32(seed) ^ lo32(s),  k1 = hi32(seed) ^ hi32(s) ^ 0x5bd1e995

    (SubspaceAutoEncoder's rule under another tag, so the nets are not the autoencoder's).  m = v = 0.  The nets are keyed by
    the subspace's POSITION.

    Centre.  center = None: the untrained net runs over all n fitted rows; mean_j is the float64 sum of double(out[i, j]) over
    the rows of a tile of 32 consecutive rows (rows ascending), then over the tiles ascending, divided by n.  Where |mean_j| <
    center_eps the coordinate becomes -center_eps when mean_j < 0 and +center_eps otherwise (exact and negative zero go to
    +center_eps; Ruff's code leaves a 0 in place); center_eps = 0 disables the rule.  c_j = float32 of the result.  The value
    depends neither on how the rows are cut into launches nor on workspace_bytes.  center = a real array [q] (every
    subspace) or [S, q] is used as given, rounded to float32.  ``center_`` (float32 [S, q]) and ``n_clamped_`` (int [S]: the
    coordinates the rule moved; 0 with a given centre) are published.  The centre stays fixed during the training.

    Batches.  SubspaceAutoEncoder's: B = min(batch_size, n), n // B steps per epoch, row j of step i of epoch e is
    feistel_perm(i B + j, n, seed, e); ``n_steps_`` = epochs (n // B); epochs = 0 scores with the untrained net.

    One step, all in float32 unless said; fma(a, b, c) is a b + c rounded once.
      forward     pre_l[i, o] = fma-chain over k ascending, from 0, of h_{l-1}[i, k] W_l[o, k]; h_l = act(pre_l), h_{-1} = z, out =
                  pre_{L-1}.  No bias is added.
      loss        r[i, j] = out[i, j] - c_j; rowsum_i = fma-chain over j ascending of r r; loss = (sum over i ascending of
                  rowsum_i) / float32(B): the batch loss before the update.
      backward    D_{L-1}[i, j] = r[i, j] float32(2 / B) (the factor formed in float64); for l from the last layer down:
                  down[i, k] = fma-chain over o ascending of D_l[i, o] W_l[o, k] with the weights BEFORE their update;
                  D_{l-1}[i, k] = down[i, k] act'(h_{l-1}[i, k]), act' = (h > 0 ? 1 : 0) for relu and fma(-h, h, 1) for tanh.
      gradient    g = fma-chain over the batch rows i ascending of D_l[i, o] h_{l-1}[i, k].
      Adam        SubspaceAutoEncoder's sequence: g = fma(wd, theta, g); m = fma(b1, m, omb1 g); v = fma(b2, v, (omb2 g) g);
                  theta = theta - (lrc m) / (sqrt(v) / sc2 + eps), the bias corrections formed on the host in float64.
    Weights, centre, losses and scores are bit-identical from run to run, for every workspace_bytes (which cuts the
    subspaces into chunks that each train to the end), for every cut of the steps into launches and for every split of
    the query rows.  ``fit`` raises ValueError, naming the bytes, when one net with its moments does not fit workspace_bytes.

    Score.  score[s, i] = float32(sum_j double(r_j)^2), r_j = out[i, j] - c_j the float32 difference, j ascending: the SQUARED
    distance to the centre, as in pyod and the paper.  ``fit`` scores the training rows with the kernel of
    ``decision_function``, so ``decision_function(X_train)`` equals ``decision_scores_`` bit for bit.  A subspace whose features
    are all constant is not trained: it scores exactly 0, has losses 0 and a centre of zeros (also under a given centre).
    NaN input leaves the results unspecified and neither faults nor hangs: every loop is bounded by its counts.

    Collapse.  With tanh, or any bounded activation, and no bias the net can drive every output to 0: the loss then sticks
    at |c|^2 and every row scores the same.  relu is the default for that reason.  On the ring recipe of
    tests/test_outlier_kpca_cpu.py (outliers inside the data) the float64 restatement with hidden (16, 4) and 50 epochs
    reaches an AUC of 0.9999 to 1.000 with relu (seeds 0 to 4) and 0.38 to 0.55 with tanh (the loss stuck at 0.0400 = |c|^2),
    against 0.16 to 0.34 for the covariance.

    Fitted state: the weights, the centres, ``location_``, ``scale_`` and the seed; neither X nor the moments are kept.
    ``fit`` publishes ``weights_`` (a list of S lists of W_l float32 [N_l, K_l], fetched on first use), ``center_``,
    ``n_clamped_``, ``loss_history_`` (float64 [S, epochs]: the float32 step losses of an epoch summed in float64 in step
    order and divided by their number), ``n_steps_``, ``location_``, ``scale_``.  ``embed(X, s)`` returns float32 [n, q], the
    output of net s on the standardised rows: for inspection and the tests.  normalize, combination, contamination,
    ``threshold_``, ``labels_``, ``predict``, ``predict_proba`` and return_per_subspace are the shared tail.  pyod is not pinned
    here: this definition and its numpy restatement in tests/test_outlier_svdd_cpu.py are what binds.  All of it runs in
    libvgan_hip.so (csrc/outlier_svdd.hip on the MLP core of csrc/outlier_mlp.hpp, which the autoencoder shares; the
    column moments in csrc/outlier_maha.hip)."""

    _layer_sizes = staticmethod(svdd_layer_sizes)
    _bias, _output_kept = False, True
    _entries, _raw = ("svdd_init", "svdd_train", "svdd_scores"), "embed"

    def __init__(self, subspaces, proba, hidden=(64, 32), activation="relu", epochs=100, batch_size=32, lr=1e-3, beta1=0.9, beta2=0.999,
                 eps=1e-8, weight_decay=1e-5, center=None, center_eps=0.1, seed=0, workspace_bytes=DEFAULT_WORKSPACE_BYTES, normalize=None,
                 combination="sum", contamination=0.1):
        super().__init__(subspaces, proba, hidden, activation, epochs, batch_size, lr, beta1, beta2, eps, weight_decay, seed, workspace_bytes,
                         normalize, combination, contamination)
        self.center, self.center_eps = check_svdd_center(center, center_eps, self.plan.count, self.hidden[-1])

    def _centers(self, X, first, count, state, s_off):
        """The centres of the untrained nets of a chunk into _center[first : first + count] and _n_clamped: the tile sums of
        every row chunk are folded into one running float64 sum in tile order."""
        n, dev, q = X.shape[0], X.device, self.hidden[-1]
        tiles, scratch = self._forward_tiles(n, count, extra_bytes=8 * q)
        rows = tiles * AE_ROW_TILE
        tile_sums = torch.empty(count * tiles * q, dtype=torch.float64, device=dev)
        run = torch.zeros(count * q, dtype=torch.float64, device=dev)
        for r0 in range(0, n, rows):
            self.ops.svdd_center(X[r0:r0 + rows], self._table, self._scaling, self._skip, self._net, first, count, self._max_dims, state, s_off,
                                 tile_sums, run, n if r0 + rows >= n else 0, self.center_eps, self._center[first:first + count],
                                 self._n_clamped[first:first + count], scratch)

    def _begin_fit_state(self, dev):
        S, q = self.plan.count, self.hidden[-1]
        given = np.zeros((S, q), np.float32) if self.center is None else np.where(self._constant[:, None], np.float32(0), self.center)
        self._center = torch.as_tensor(np.ascontiguousarray(given, dtype=np.float32), device=dev)
        self._n_clamped = torch.zeros(S, dtype=torch.int32, device=dev)

    def _begin_chunk(self, X, first, count, state, s_off):
        if self.center is None:
            self._centers(X, first, count, state, s_off)

    def _target(self, first, count):
        return (self._center[first:first + count],)

    def _publish_fit_state(self):
        self.center_ = self._center.cpu().numpy()
        self.n_clamped_ = self._n_clamped.cpu().numpy().astype(np.int64)

    def embed(self, X, s):
        """float32 [n, q]: the output of the net of subspace s on the rows of X, standardised by the fitted location_ and scale_."""
        return self._output(X, s)


# ---- subspace outlier degree (SOD) over the subspaces ---------------------------------------------------------------------------
SOD_MAX_ROWS = 1 << 15  # VGAN_SOD_MAX_ROWS: the shared-neighbour counts of all fitted rows are one byte each in a 32 KiB LDS table
SOD_MAX_REF = 64  # VGAN_SOD_MAX_REF
SOD_FORMS = {"pyod": 0, "paper": 1}  # VGAN_SOD_FORM_*
SOD_LANES = 64  # partial sums of V and Q: the summation shape of the class docstring


def check_sod_params(ref_set, alpha, form):
    if not (_is_int(ref_set) and 1 <= int(ref_set) <= SOD_MAX_REF):
        raise ValueError(f"ref_set must be an integer between 1 and {SOD_MAX_REF}, got {ref_set!r}")
    if not (_is_real(alpha) and 0.0 < float(alpha) <= 1.0):
        raise ValueError(f"alpha must be a number in (0, 1], got {alpha!r}")
    if not (isinstance(form, str) and form in SOD_FORMS):
        raise ValueError(f"form must be 'pyod' or 'paper', got {form!r}")
    return int(ref_set), float(alpha), form


class SubspaceSOD(_NeighborScorer):
    """Subspace outlier degree per subspace (SOD: Kriegel, Kroeger, Schubert, Zimek 2009; pyod's ``SOD``), combined like the
    detectors of SubspaceEnsemble: ``fit`` sets ``decision_scores_``, ``decision_function`` scores new rows; higher is more
    outlying.  Every distance detector here weighs all d_s features of a subspace alike, so a row that departs in two or
    three of several hundred, in a direction in which its own neighbourhood is tight, is drowned by the spread of the
    rest.  SOD lets each row choose the features in which it is judged: those in which the rows most similar to it vary
    little.  It also says in which features a row is an outlier (``relevant_features``).

    Everything is per subspace s, with features F_s in ascending order and d_s = |F_s|.

    1. Lists.  N(j) is the refined neighbour list of fitted row j at ``fit``: the n_neighbors nearest fitted rows, j itself
       excluded, ordered by (float32 distance, index): the very lists of SubspaceEnsemble (``kneighbors``).  For a new row q,
       N(q) is its list among the fitted rows with nothing excluded.
    2. Shared neighbours.  SNN(x, j) = |N(x) n N(j)|, the lists taken as sets of row indices, for every fitted j; at ``fit``
       j != x.
    3. Reference set.  R(x) is the first ref_set fitted rows in the order (SNN descending, row index ascending).  Rows with
       SNN = 0 take part in that order: a set that cannot be filled from rows that share something takes the lowest
       indices that share nothing, and ``n_unshared_[s]`` counts the fitted rows whose set had to.  A new row is scored
       alone against the fitted state, whatever else is in the batch (the stance of SubspaceECOD and SubspaceSOS), so
       ``decision_function(X_train)`` is not ``decision_scores_``: there a row's list starts with the row itself, and the
       row may sit in its own reference set.
    4. Moments, float64 from the raw float32 values, every difference, square, sum and quotient rounded on its own (no
       fused multiply-add), the rows r of R(x) in the order of R:
           mu_f = (sum_r X[r, f]) / ref_set,      v_f = (sum_r (X[r, f] - mu_f)^2) / ref_set.
    5. Threshold.  V = sum_{f in F_s} v_f in this shape: 64 partial sums, partial l the sequential sum over the positions
       l, l + 64, l + 128, ... of F_s (ascending), starting from 0; then the 64 partials added sequentially in the order
       l = 0 .. 63, starting from 0 (``numpy.cumsum`` of the strided slices, then of the partials).  T = (alpha V) / d_s.
       Feature f is relevant iff v_f < T, strictly; r is the number of relevant features.
    6. Score.  Q = the sum of (x_f - mu_f)^2 over the relevant features in the same shape (a feature that is not relevant
       adds nothing).  form "pyod": sqrt(Q / r); form "paper": sqrt(Q) / r; r = 0 gives 0 (pyod's rule): a reference set of
       identical rows has r = 0, and so has a subspace of constant features.  The per-subspace score is that float64 value
       rounded once to float32.

    These are pyod's rules and the paper's as they are remembered here, made definite where they leave a choice (the order
    among equal SNN, rows that share nothing, the summation shape, new rows).  pyod was not at hand to pin them, so the
    definition above and its numpy restatement in tests/test_outlier_sod_cpu.py are what binds, not pyod.  Not built:
    pyod's transductive ``decision_function`` (it ranks the new rows among themselves), reference sets by distance,
    n_neighbors above 32, weights on the reference rows.

    n_neighbors: 1 .. 32 (default 20, pyod's).  ref_set: 1 .. 64 (default 10, pyod's); it is not tied to n_neighbors, the
    ranking runs over all fitted rows.  alpha: in (0, 1] (default 0.8, pyod's).  The defaults are pyod's; variances taken
    from ten rows are noisy, and when few features matter a larger ref_set with a smaller alpha (31 and 0.3) is what works
    (README).  form: "pyod" or "paper".  ``fit`` needs at least max(n_neighbors, ref_set) + 1 rows and takes at most
    SOD_MAX_ROWS = 2^15: the shared-neighbour counts of all fitted rows live as one byte each in a table in LDS, and 2^15 rows
    are the 32 KiB of it that still leave four workgroups a compute unit.  engine, splits, workspace_bytes: as for
    SubspaceEnsemble.  normalize, combination, contamination, ``threshold_``, ``labels_``, ``predict``, ``predict_proba``,
    return_per_subspace: the shared tail.

    ``fit`` publishes, in the given subspace order: ``reference_set_`` (int32 [S, n, ref_set]), ``n_relevant_`` (int32
    [S, n]) and ``n_unshared_`` (int [S]).  ``reference_set(X)`` returns the sets of new rows, ``relevant_features(s, X=None)``
    the features of subspace s in which each row was judged, bool [n, d] in the model's feature coordinates.

    The fitted state keeps, besides X, the reverse lists (for every fitted m the rows whose list holds m, a CSR per
    subspace built from the lists by an integer count, a scan and a fill): about 4 S n n_neighbors bytes, and 4 S n ref_set
    for the sets.  The lists themselves are not read again after ``fit`` and are not kept (``kneighbors`` forms them anew),
    which halves the 8 S n n_neighbors bytes that keeping both would take.  SNN is a sparse integer product over the
    reverse lists, O(n_neighbors mean|RN|) per row and never an n x n sweep; counts are integers, so reference sets, ``n_relevant_``, the relevance masks and the scores are bit-identical from run to
    run, for every splits and workspace_bytes, and for a subspace fitted alone or with others.  The kernels are in
    libvgan_hip.so (csrc/outlier_sod.hip)."""

    def __init__(self, subspaces, proba, n_neighbors=20, ref_set=10, alpha=0.8, form="pyod", engine="auto", splits=None,
                 workspace_bytes=DEFAULT_WORKSPACE_BYTES, normalize=None, combination="sum", contamination=0.1):
        self.ref_set, self.alpha, self.form = check_sod_params(ref_set, alpha, form)
        self._configure(subspaces, proba, engine, workspace_bytes, normalize, combination, contamination)
        self._configure_neighbors(n_neighbors, splits)

    def _check_fit_rows(self, n):
        least = max(self.n_neighbors, self.ref_set) + 1
        if n < least:
            raise ValueError(f"need at least max(n_neighbors, ref_set) + 1 = {least} fitted rows, got {n}")
        if n > SOD_MAX_ROWS:
            raise ValueError(f"SubspaceSOD fits at most SOD_MAX_ROWS = {SOD_MAX_ROWS} rows, got {n}")

    def _sets(self, idx, first, count, out=None, n_unshared=None):
        """int32 [count, nq, ref_set]: the reference sets of the lists idx against the fitted reverse lists of the chunk; with
        n_unshared (fit) idx are the fitted lists themselves and a row is left out of its own set."""
        if out is None:
            out = torch.empty(count, idx.shape[1], self.ref_set, dtype=torch.int32, device=idx.device)
        self.ops.sod_reference_sets(idx, self._rn_off[first:first + count], self._rn_rows[first:first + count], self._X.shape[0],
                                    n_unshared is not None, out, n_unshared)
        return out

    def _score(self, Xq, fitting):
        """(ensemble scores float64 [n], per float32 [S, n]), both on the device.  A chunk runs every stage: a subspace's sets
        depend on its own lists alone."""
        dev, n = self._X.device, self._X.shape[0]
        nq = n if Xq is None else Xq.shape[0]
        per = torch.empty(self.plan.count, nq, dtype=torch.float32, device=dev)
        for first, count, idx, _ in self._neighbors(Xq):
            if fitting:
                cursor = torch.empty(count, n, dtype=torch.int32, device=dev)
                self.ops.sod_reverse_lists(idx, self._rn_off[first:first + count], self._rn_rows[first:first + count], cursor)
                ref = self._sets(idx, first, count, self._ref[first:first + count], self._unshared[first:first + count])
                n_rel = self._n_rel[first:first + count]
            else:
                ref = self._sets(idx, first, count)
                n_rel = torch.empty(count, nq, dtype=torch.int32, device=dev)
            self.ops.sod_score(self._X if Xq is None else Xq, self._X, self._table, first, count, ref, self.alpha,
                               SOD_FORMS[self.form], per, self._rows[first:first + count], n_rel)
        return self._combine(per, fitting), per

    def fit(self, X, y=None):
        """Keeps X and the reverse lists resident and scores X (self excluded): decision_scores_ (float64 [n]),
        per_subspace_scores_, reference_set_, n_relevant_, n_unshared_; with normalize also score_center_ / score_scale_."""
        self._X = X = self._begin_fit(X)
        S, n, k, dev = self.plan.count, X.shape[0], self.n_neighbors, X.device
        self._rn_off = torch.empty(S, n + 1, dtype=torch.int32, device=dev)  # processing order, like everything below
        self._rn_rows = torch.empty(S, n * k, dtype=torch.int32, device=dev)
        self._ref = torch.empty(S, n, self.ref_set, dtype=torch.int32, device=dev)
        self._n_rel = torch.empty(S, n, dtype=torch.int32, device=dev)
        self._unshared = torch.empty(S, dtype=torch.int32, device=dev)
        scores, per = self._score(None, fitting=True)
        given = torch.as_tensor(self.plan.given, device=dev)
        self.reference_set_ = self._ref[given].cpu().numpy()
        self.n_relevant_ = self._n_rel[given].cpu().numpy()
        self.n_unshared_ = self._unshared[given].cpu().numpy().astype(np.int64)
        return self._publish(scores, per)

    def reference_set(self, X):
        """int32 [S, n, ref_set], given subspace order: the reference sets of the new rows X among the fitted rows."""
        self._require_fit()
        Xq = _device_matrix(X, self.plan.d)
        out = torch.empty(self.plan.count, Xq.shape[0], self.ref_set, dtype=torch.int32, device=Xq.device)
        for first, count, idx, _ in self._neighbors(Xq):
            out[self._rows[first:first + count].long()] = self._sets(idx, first, count)
        return out.cpu().numpy()

    def relevant_features(self, s, X=None):
        """bool [n, d] in the model's feature coordinates: the features of subspace s (its index in the given order) in
        which each row was judged; X None: the fitted rows, from reference_set_.  Row i has n_relevant_[s, i] of them."""
        self._require_fit()
        if not (_is_int(s) and 0 <= int(s) < self.plan.count):
            raise ValueError(f"s must be a subspace index between 0 and {self.plan.count - 1}, got {s!r}")
        pos = int(self.plan.given[int(s)])
        dev = self._X.device
        if X is None:
            Xq, ref = self._X, self._ref[pos:pos + 1]
        else:
            Xq = _device_matrix(X, self.plan.d)
            ref = self._sets(next(self._neighbors(Xq, only=pos))[2], pos, 1)
        nq, ds = Xq.shape[0], int(self.plan.dims[pos])
        words = 2 * (-(-ds // SOD_LANES))
        mask = torch.zeros(1, nq, words, dtype=torch.int32, device=dev)
        scratch = torch.empty(1, nq, dtype=torch.float32, device=dev)
        self.ops.sod_score(Xq, self._X, self._table, pos, 1, ref.contiguous(), self.alpha, SOD_FORMS[self.form], scratch, None,
                           torch.empty(1, nq, dtype=torch.int32, device=dev), mask)
        bits = np.unpackbits(mask[0].cpu().numpy().view(np.uint8), axis=1, bitorder="little")[:, :ds].astype(bool)
        out = np.zeros((nq, self.plan.d), dtype=bool)
        out[:, self.plan.feat[self.plan.feat_off[pos]:self.plan.feat_off[pos + 1]]] = bits
        return out


# ---- one detector per method string ----------------------------------------------------------------------------------
_METHOD_CLASSES = {"cblof": SubspaceCBLOF, "ecod": SubspaceECOD, "iforest": SubspaceIForest, "inne": SubspaceINNE,
                   "mahalanobis": SubspaceMahalanobis, "gmm": SubspaceGMM, "hbos": SubspaceHBOS, "loda": SubspaceLODA,
                   "pca": SubspacePCA, "ocsvm": SubspaceOCSVM, "sos": SubspaceSOS, "loci": SubspaceLOCI, "dif": SubspaceDIF, "kpca": SubspaceKPCA,
                   "autoencoder": SubspaceAutoEncoder, "deepsvdd": SubspaceDeepSVDD, "rshash": SubspaceRSHash}
_NEIGHBOR_CLASSES = {"abod": SubspaceABOD, "cof": SubspaceCOF, "sod": SubspaceSOD}


def build_ensemble(subspaces, proba, method="knn", n_neighbors=5, **kw):
    """The unfitted detector that the `method` string of ``outlier_ensemble`` names, over any boolean subspace matrix and its
    weights: the models' ``outlier_ensemble`` and ``HiCS.outlier_ensemble`` both end here.  "abod", "cof" and "sod" take
    n_neighbors; "mcd" is SubspaceMahalanobis(robust=True); the classes of _METHOD_CLASSES do not use n_neighbors; every
    other string ("knn", "lof", "kde", or an unknown one, which it rejects) goes to SubspaceEnsemble."""
    if method == "mcd":
        return SubspaceMahalanobis(subspaces, proba, robust=True, **kw)
    if method in _METHOD_CLASSES:
        return _METHOD_CLASSES[method](subspaces, proba, **kw)
    if method in _NEIGHBOR_CLASSES:
        return _NEIGHBOR_CLASSES[method](subspaces, proba, n_neighbors=n_neighbors, **kw)
    return SubspaceEnsemble(subspaces, proba, method=method, n_neighbors=n_neighbors, **kw)
