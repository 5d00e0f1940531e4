"""Subspace outlier scoring on one GPU: the fused HIP path (vgan_amd.SubspaceEnsemble, fit = self-excluded scoring of the
training set) against a plain-torch GPU baseline over 4096-row query blocks, per subspace:
  --method knn (default): kNN "largest"; baseline torch.cdist + topk.
  --method kde: Gaussian KDE (--bandwidth, default 1.0); baseline torch.cdist + torch.logsumexp.
Subspaces come from approx_subspace_dist of a briefly trained VGAN_no_kl, so their sizes are the ones a user gets.
Prints one JSON line: per configuration the median time of both paths over warm repetitions, the fused path's rate
against the fp32 peak (2 n^2 sum d_s flops per distance sweep: one for kNN, two for KDE), and the largest relative
difference of the two paths' ensemble scores.
--sweep adds the engine crossover: exact vs Gram engine on subspaces of a fixed size (kNN).
  --method cblof: k-means + CBLOF (vgan_amd.SubspaceCBLOF) at C = 8 and C = 64 from the same random rows, tol = 0 and a
    fixed max_iter (--iters): fit time, time per Lloyd iteration, fit time per polling stride; baseline (a) per subspace
    torch.cdist + argmin + index_add_ on the GPU with the float64 score tail in torch, (b) sklearn's KMeans (lloyd, same
    init and iteration count) on the CPUs for a sample of the subspaces, scaled to all of them; and the E step composed
    from vgan_outlier_knn with k = 1 over the centres against one whole iteration (assign + update) on the same operands.
  --method abod: angle-based scores (vgan_amd.SubspaceABOD) at k = 10 and 32: (a) its fit against the kNN fit with the same
    k on the same subspaces (the difference is what ABOD adds to the neighbour search); (b) the ABOD launches alone on
    the resident neighbour lists against a torch baseline handed the same lists (gather, float64 bmm, masked two-pass
    variance), with the largest relative score difference of the two; (c) the gather bandwidth and the float64
    multiply-add rate of (b) from n sum_s k d_s 4 B and n sum_s k^2 d_s multiply-adds (the kernel pads k to 8, 16 or 32
    and forms the whole k x k matrix: the executed count is given as well).  --no-baselines leaves the torch path out
    (for a run under a profiler), --shape d,n,S picks one shape.
  --method cof: connectivity-based scores (vgan_amd.SubspaceCOF, the set-based nearest chain) at k = 10 and 32 on the shapes
    of the ABOD leg: (a) its fit against the kNN fit with the same k on the same subspaces (cof_over_knn: what the chain,
    the ratio and the ceiling add to the neighbour search); (b) the chain launches alone on the resident neighbour lists
    against a torch baseline handed the same lists (gather, float64 torch.cdist from the differences, k vectorised arg-min
    steps), with the largest relative difference of the two chaining distances; (c) the gather bandwidth and the float64
    multiply-add rate of (b), nominal (k + 1)^2 and executed (8 T)^2 + 1 per row and feature.  --no-baselines and --shape
    as for abod.
  --method ecod: empirical-CDF scores (vgan_amd.SubspaceECOD, aggregate "dimension"): fit and decision_function (the
    training rows as queries) against (a) a float64 torch restatement on the same GPU (torch.sort, torch.searchsorted,
    the terms, one float64 matmul with the mask) and (b) numpy on the host (sort and searchsorted per feature, then a loop
    over the subspaces); the fit split into its calls (sort, skew signs, tail counts, terms + product; the terms alone
    from a call with a one-column mask); and the masked sums as the dense float64 product against the plain gather-sum
    kernel of tools/ecod_gather.hip on the same terms (build it into tools/bin/libecod_gather.so first: its header has
    the line), with the largest relative difference of the two.  product_s is terms + product minus terms alone: a
    difference of two call times, not a kernel time.
  --method iforest: isolation forest (vgan_amd.SubspaceIForest, 100 trees on 256 rows each): fit and decision_function (the
    training rows as queries); the fit split into its calls (build, path sums, scores); sklearn's IsolationForest(
    n_estimators=100, n_jobs=16) fitted and scored per subspace on the CPUs for a sample of the subspaces, scaled to all of
    them; and the kNN fit (k = 5) of SubspaceEnsemble on the same subspaces.  walk_steps_per_s counts S T n walks of the
    measured mean depth.  With --n-dims q >= 2 the forest cuts with hyperplanes over q features: the row holds fit, its build
    and walk launches, decision_function and the bytes of the fitted state, and from the same process the axis-parallel
    forest (axis_*) and SubspaceDIF's fit on the same rows; no sklearn or kNN leg.
  --method inne: nearest-neighbour isolation scores (vgan_amd.SubspaceINNE, 200 estimators of 8 centres each) on the shapes of
    the isolation-forest leg: fit and decision_function (the training rows as queries); the fit split into its calls
    (build, scores), with the float64 rate of the scoring pass counted as three operations per (row, centre, feature); the
    numpy restatement of the definition on 16 CPU threads (the estimators dealt to the threads; the build in full, the
    scores on 2 000 rows scaled to n) for a sample of the subspaces scaled to all of them, and whether its scores are
    bit-equal to the device's; the kNN fit (k = 5) of SubspaceEnsemble on the same subspaces; and the scoring pass over
    subspaces of scattered columns against subspaces of neighbouring columns (what a packed copy would offer).
  --method mahalanobis: covariance-based scores (vgan_amd.SubspaceMahalanobis, shrinkage 0.1): fit and decision_function (the
    training rows as queries), classical and robust (max_csteps 30); the classical fit split into its calls (moments,
    factor, scores); (a) a float64 torch restatement on the same GPU (per subspace: gather, mean, centred product,
    torch.linalg.cholesky, solve_triangular, the squared column norms) and (b) sklearn's ShrunkCovariance(0.1).fit /
    .mahalanobis per subspace on the host, for a sample of the subspaces scaled to all of them.
  --method gmm: Gaussian-mixture scores (vgan_amd.SubspaceGMM, C = 4, reg_covar 1e-6) from random start labels with tol = 0
    and max_iter = 10, so that every path runs the same ten EM iterations: fit and decision_function (the training rows as
    queries); one iteration split into its calls (E step, moments, factor + log-determinants), the E step's rate counted as
    the full product 2 n C sum d_s^2 (what vgan_maha_scores is counted as in outlier_maha_bench.json); and sklearn's
    GaussianMixture(max_iter=10, tol=0) from the same start (weights, means and precisions after the first M step) on the
    host for a sample of the subspaces, scaled to all of them.
  --method hbos / --method loda: the histogram scores (vgan_amd.SubspaceHBOS, 10 bins; vgan_amd.SubspaceLODA, 100
    projections of 10 bins) on the shapes of the ECOD leg: fit and decision_function (the training rows as queries); the
    fit split into its stages (HBOS: range, edges, count, lookup + product, the lookup alone from a call with a one-column
    mask; LODA: whole passes over the chunks, each with its packing: pack alone, range, count, projection + lookup + mean);
    (a) a float64 torch restatement on the same GPU and (b) numpy on the host (numpy.histogram and searchsorted per
    column; LODA for a sample of the subspaces, scaled to all of them); and the ECOD fit on the same subspaces.
  --method pca: principal-component scores (vgan_amd.SubspacePCA: all components, weighted, standardised, shrinkage 0.1): fit
    and decision_function (the training rows as queries); the fit split into its launches (moments, the Jacobi eigen
    solve, the scoring product, the latter also with components="minor", n_components=0.9); SubspaceMahalanobis' fit and
    its triangular scoring product at the same shape beside them; sklearn's StandardScaler + PCA fitted per subspace on the
    host for a sample of the subspaces, scaled to all of them; and (eigen_by_width) the eigen solve alone on one subspace of
    16, 64, 256 features and of the widest width the table held, with its sweep count.
  --method ocsvm: one-class SVM scores (vgan_amd.SubspaceOCSVM, nu 0.1, gamma "scale", tol 1e-3, a 16 GiB workspace so that a
    chunk holds many kernel matrices): fit and decision_function (the training rows as queries); the fit split into its
    stages (kernel matrices, the SMO loop with its start and rho, scoring), each behind a synchronisation; the SMO steps
    per subspace (minimum, median, maximum) and the time of one step of the longest subspace of a chunk; the SMO stage
    with a and G in LDS (where they fit) and in place with 256 and with 1024 threads; and sklearn's OneClassSVM(kernel="rbf", shrinking=False) fitted and
    scored per subspace on the host for a sample of the subspaces, scaled to all of them.
  --method sos: stochastic outlier selection (vgan_amd.SubspaceSOS, perplexity 30, tol 1e-5, a 16 GiB workspace) on the shapes of
    the OCSVM leg: fit and decision_function (the training rows as queries); the fit split into its stages (dissimilarity
    matrices, the perplexity search, the scores from the stored matrices), each behind a synchronisation; the search steps per
    row (mean, maximum) and the float64 exponentials per second of the search; the search with a row per wave (where it fits)
    and per workgroup of 1024 threads; the same rules in numpy on the host with 16 threads (matrix, search and scores
    separately) for a sample of the subspaces, scaled to all of them; and the LOF fit (k = 20) on the same rows.
  --method loci: the local correlation integral (vgan_amd.SubspaceLOCI at its defaults: 32 radii at 4 an octave, alpha 0.5, n_min 20,
    a 16 GiB workspace) on d = 784, S = 50 sampled, n = 2000 and 10^4: fit and decision_function (the training rows as queries);
    the fit split into its stages (distance matrices, r_max and the radii, counts, sums, finish), each behind a synchronisation;
    the (pair, radius) rate of the counts and the sums sweeps, the latter also as a share of the chip's vector-ALU rate at the
    vector instructions the sweep spends on one; the SubspaceSOS (perplexity 30) and LOF (k = 20) fits on the same rows; and the
    same rules in numpy on the host with 16 threads for a sample of the subspaces, scaled to all of them.
  --method dif: deep isolation forest (vgan_amd.SubspaceDIF at its defaults: 50 random nets d_s -> 500 -> 100 -> 20 per subspace,
    6 trees of 256 rows on each) on d = 10 at n = 10^4 and d = 784 at n = 10^4 and 5 10^4, S = 50 sampled: fit and
    decision_function (the training rows as queries); one pass over all blocks split into its calls, each behind a
    synchronisation (weights, representation, tree build, walk), with the fp32 rate of the representation against the
    fp32-matrix peak; the same rows through SubspaceIForest with n_estimators = 300 = r T; the same layers run UNFUSED on the
    library's other pieces for a sample of the subspaces (torch scales and gathers the subspace once, then per block and
    layer one vgan_gemm_grouped product on the weights of vgan_dif_weights and torch.tanh), scaled to all of them; and numpy
    (float32 products and tanh) plus sklearn's IsolationForest(6 trees, n_jobs=16) per block on 16 CPU threads for 2
    subspaces and 2 000 rows, scaled to all rows and subspaces.
  --method rshash: RS-Hash (vgan_amd.SubspaceRSHash at its defaults: 100 components on 1 000 sampled rows each) on d = 784, S = 50
    sampled, n = 2000, 10^4 and 5 10^4: fit (a new detector each time, so with the host draws), refit and decision_function (the
    training rows as new rows); the three stages of the fit
    launched alone on the fitted state (build, cell sums with the in-sample test, scores) and the host's share (the range pass
    and its copy, the draws); the cell sums as (row, component) pairs a second; the cell sums reading X row-major through L2
    against reading a column-major copy (the copy timed with it); IN THE SAME RUN SubspaceIForest (100 trees), SubspaceHBOS
    and SubspaceDIF at their defaults on the same rows; and the same rules in numpy on 16 host threads (the components of a
    subspace dealt to a thread pool, the device's samples given) for two subspaces, scaled to all of them and compared.
  --method sod: the subspace outlier degree (vgan_amd.SubspaceSOD) at d = 784, S = 50 sampled, n = 2000 and 10^4, with pyod's
    defaults (n_neighbors 20, ref_set 10, alpha 0.8) and with (32, 31, 0.3): fit and decision_function (the training rows as
    new rows) beside the LOF fit with the same n_neighbors on the same rows; the fit split into the neighbour lists (pack,
    search, refine) and, launched alone on the resident lists, the reverse lists, the reference sets and the scores; the
    LDS increments per second of the reference sets (sum over m of |RN(m)|^2) and the gather bandwidth of the scores (every
    reference value is read four times).
  --method kpca: kernel PCA novelty scores (vgan_amd.SubspaceKPCA at its defaults, a 16 GiB workspace) at d = 784, S = 50 sampled, n
    = 2000 and 10^4, with 256 landmarks (max_samples="auto") and with 1024: fit and decision_function (the training rows as
    queries); one fit and one decision_function split into their calls, each behind a synchronisation (packing, landmark
    kernel matrix, centring, eigensolver, kernel rows, row means plus scores), with the sweeps taken; the SubspacePCA and
    SubspaceOCSVM (nu 0.1) fits on the same rows; and sklearn's KernelPCA(eigen_solver="dense") fitted on the landmark rows
    and transforming all rows per subspace on 16 host threads for a sample of the subspaces, scaled to all of them.
  --method ae: autoencoders (vgan_amd.SubspaceAutoEncoder at its defaults: d_s -> 64 -> 32 -> 64 -> d_s, relu, 100 epochs of
    batches of 32, Adam) at d = 784, S = 50 sampled, n = 2000 and 10^4: fit and decision_function (the training rows as new
    rows); one fit split into scaling (the column moments), training (all launches, with the microseconds per optimiser
    step and the steps per launch) and scoring, each behind a synchronisation; the same nets trained in torch on the GPU as
    padded torch.bmm batches (all S nets in one [S, B, d_max] batch, the padded outputs masked, torch.optim.Adam with the
    same weight decay, one torch.randperm per epoch) for a sample of the steps, scaled to all of them; and the LOF fit (k =
    20) on the same rows.
  --method deepsvdd: Deep SVDD encoders (vgan_amd.SubspaceDeepSVDD at its defaults: d_s -> 64 -> 32 without bias, relu, 100
    epochs of batches of 32, Adam) on the shapes of --method ae: fit and decision_function; one fit split into scaling,
    centre (init plus the forward over all rows and the fold), training (microseconds per optimiser step) and scoring,
    each behind a synchronisation; IN THE SAME RUN SubspaceAutoEncoder with hidden (64, 32) on the same rows (fit, training,
    microseconds per step) and the LOF fit (k = 20); and the same encoders trained in torch on the GPU as padded torch.bmm
    batches with torch.optim.Adam for a sample of the steps.
  --method hics: the HiCS search (vgan_amd.HiCS at its defaults) at d = 784, n = 2000 and 10^4: fit, and its split into the
    column argsort, level 2 (all 306 936 pairs x 50 draws, under the library's workgroup shape and under both forced ones)
    and the higher levels (their candidates replayed on the resident index), with draws per second; subspace_contrast of the
    50 sampled subspaces of a two-epoch model (350 to 390 features each, the complement path); and the numpy restatement
    in 16 spawned processes on 256 of the pairs and 16 of the model's subspaces, scaled to all and compared bit for bit.
--method metric measures the metrics of the neighbour search (d = 784, 50 sampled subspaces of a two-epoch model, n = 2000 and
    10^4, k = 20): the LOF fit under euclidean, manhattan, chebyshev, minkowski (p = 0.5) and cosine in one session; the
    Minkowski-family sweep alone (vgan_outlier_knn_metric on resident blocks) as pair-features per second and, for Manhattan
    and Chebyshev at two vector operations a pair-feature, as a share of the vector peak; torch.cdist(p=1) + topk per subspace
    on the GPU; and sklearn's brute-force Manhattan LOF on 16 threads on two subspaces, scaled to all.
--normalize {zscore,robust,minmax} measures score normalisation instead (kNN, k = 5, the three configurations of the KDE
table): the median warm fit time with normalize=None, with the given mode, and of the host alternative (the raw fit, then
the numpy statistics and combination on the score matrix fit copied to the host), plus the device statistics and combine
launches on their own.  --out also writes the JSON to a file."""
import argparse
import gc
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import vgan_amd  # noqa: E402

FP32_PEAK = 157.3e12  # MI355X fp32 vector / MFMA dense peak (MI355X_MICROARCH)


def timed(fn, reps):
    fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append(time.perf_counter() - t0)
    return float(np.median(ts)), [round(t, 5) for t in ts]


def baseline(X, subspaces, proba, k, block=4096):
    n = X.shape[0]
    out = torch.zeros(n, dtype=torch.float64, device=X.device)
    for s in range(len(subspaces)):
        Xs = X[:, torch.as_tensor(np.flatnonzero(subspaces[s]), device=X.device)].contiguous()
        kth = torch.empty(n, dtype=torch.float32, device=X.device)
        for q0 in range(0, n, block):
            D = torch.cdist(Xs[q0:q0 + block], Xs)
            D[torch.arange(D.shape[0], device=X.device), torch.arange(q0, q0 + D.shape[0], device=X.device)] = float("inf")
            kth[q0:q0 + block] = torch.topk(D, k, dim=1, largest=False).values[:, k - 1]
        out += float(proba[s]) * kth.double()
    return out


def baseline_kde(X, subspaces, proba, bandwidths, block=4096):
    n = X.shape[0]
    out = torch.zeros(n, dtype=torch.float64, device=X.device)
    for s in range(len(subspaces)):
        Xs = X[:, torch.as_tensor(np.flatnonzero(subspaces[s]), device=X.device)].contiguous()
        ds, h = Xs.shape[1], float(bandwidths[s])
        score = torch.empty(n, dtype=torch.float32, device=X.device)
        for q0 in range(0, n, block):
            D = torch.cdist(Xs[q0:q0 + block], Xs)
            L = D * D * (-0.5 / (h * h))
            L[torch.arange(L.shape[0], device=X.device), torch.arange(q0, q0 + L.shape[0], device=X.device)] = float("-inf")
            score[q0:q0 + block] = -(torch.logsumexp(L, dim=1) - np.log(n - 1) - ds * np.log(h) - 0.5 * ds * np.log(2 * np.pi))
        out += float(proba[s]) * score.double()
    return out


def subspaces_for(d, n, count, seed):
    rng = np.random.default_rng(seed)
    X = rng.normal(size=(n, d)).astype(np.float32)
    X[:, 1] = X[:, 0] + 0.1 * X[:, 1]
    model = vgan_amd.VGAN_no_kl(epochs=2, batch_size=min(500, n))
    model.fit(X[:min(n, 5000)])
    model.approx_subspace_dist(count)
    m, p = model.subspaces, model.proba
    # the model's training engine holds a captured HIP graph: release it here, not at a garbage collection that may fall
    # inside the next model's capture (destroying a graph is not permitted while a stream captures)
    del model
    gc.collect()
    torch.cuda.synchronize()
    return X, m, p


def run_config(d, n, count, k, reps, with_baseline, method="knn", bandwidth=1.0):
    X, m, p = subspaces_for(d, n, count, seed=d + n + count)
    Xd = torch.as_tensor(X, device="cuda")
    if method == "kde":
        ens = vgan_amd.SubspaceEnsemble(m, p, method="kde", bandwidth=bandwidth)
    else:
        ens = vgan_amd.SubspaceEnsemble(m, p, method="knn", n_neighbors=k)
    t_fused, ts = timed(lambda: ens.fit(Xd), reps)
    dims = m.sum(axis=1)
    flops = (2 if method == "kde" else 1) * 2.0 * n * n * float(dims.sum())
    row = {"method": method, "d": d, "n": n, "S_sampled": count, "S_distinct": int(len(m)),
           **({"bandwidth": bandwidth} if method == "kde" else {"k": k}),
           "d_s_min": int(dims.min()), "d_s_median": float(np.median(dims)), "d_s_max": int(dims.max()),
           "gram_subspaces": int(ens.plan.gram.sum()), "fused_s": round(t_fused, 5), "fused_reps_s": ts,
           "fused_tflops": round(flops / t_fused / 1e12, 2), "fused_frac_fp32_peak": round(flops / t_fused / FP32_PEAK, 4)}
    if with_baseline:
        if method == "kde":
            base = lambda: baseline_kde(Xd, m, p, ens.bandwidth_)  # noqa: E731
        else:
            base = lambda: baseline(Xd, m, p, k)  # noqa: E731
        t_base, tb = timed(base, reps)
        want = base().cpu().numpy()
        row.update({"torch_s": round(t_base, 5), "torch_reps_s": tb, "speedup": round(t_base / t_fused, 2),
                    "max_rel_diff_vs_torch": float(np.max(np.abs(ens.decision_scores_ - want) / np.maximum(np.abs(want), 1e-12)))})
    return row


def baseline_cblof(X, subspaces, proba, rows, C, iters, alpha=0.9, beta=5.0):
    """Per subspace on the GPU: iters Lloyd iterations (float32 cdist + argmin, float64 index_add_ means, an empty cluster
    keeps its centre), then the float64 assignment and CBLOF scores; the boundary on the host as in the product."""
    from vgan_amd.outlier import large_cluster_boundary
    n = X.shape[0]
    out = torch.zeros(n, dtype=torch.float64, device=X.device)
    rows = torch.as_tensor(rows, device=X.device)
    for s in range(len(subspaces)):
        Xs = X[:, torch.as_tensor(np.flatnonzero(subspaces[s]), device=X.device)].contiguous()
        X64 = Xs.double()
        cen = X64[rows].clone()
        ones = torch.ones(n, dtype=torch.float64, device=X.device)
        for _ in range(iters):
            lab = torch.cdist(Xs, cen.float()).argmin(dim=1)
            sums = torch.zeros_like(cen).index_add_(0, lab, X64)
            cnt = torch.zeros(C, dtype=torch.float64, device=X.device).index_add_(0, lab, ones)
            cen = torch.where(cnt[:, None] > 0, sums / cnt.clamp(min=1.0)[:, None], cen)
        D = torch.cdist(X64, cen)
        lab = D.argmin(dim=1)
        sizes = torch.bincount(lab, minlength=C).cpu().numpy()
        large = torch.as_tensor(large_cluster_boundary(sizes, alpha, beta)[1], device=X.device)
        own = D.gather(1, lab[:, None])[:, 0]
        score = torch.where(large[lab], own, D[:, large].min(dim=1).values).float()
        out += float(proba[s]) * score.double()
    return out


def cblof_baselines(row, ens, X, Xd, m, p, rows, C, iters, reps, t_fit, sklearn_sample):
    S = len(m)
    # (a) torch on the same GPU
    t_base, tb = timed(lambda: baseline_cblof(Xd, m, p, rows, C, iters), reps)
    want = baseline_cblof(Xd, m, p, rows, C, iters).cpu().numpy()
    rel = np.abs(ens.decision_scores_ - want) / np.maximum(np.abs(want), 1e-12)
    row.update({"torch_s": round(t_base, 5), "torch_reps_s": tb, "speedup_vs_torch": round(t_base / t_fit, 2),
                "max_rel_diff_vs_torch": float(rel.max()), "median_rel_diff_vs_torch": float(np.median(rel)),
                "rows_beyond_1e-5_vs_torch": int((rel > 1e-5).sum())})
    # (b) sklearn on the CPUs, a sample of the subspaces scaled to all of them
    try:
        from sklearn.cluster import KMeans
        import warnings
        pick = np.unique(np.linspace(0, S - 1, min(S, sklearn_sample)).astype(int))
        X64 = X.astype(np.float64)
        t0 = time.perf_counter()
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            for s in pick:
                f = np.flatnonzero(m[s])
                KMeans(n_clusters=C, init=X64[rows][:, f], n_init=1, algorithm="lloyd", max_iter=iters, tol=0.0).fit(X64[:, f])
        t_sk = (time.perf_counter() - t0) * S / len(pick)
        row.update({"sklearn_s": round(t_sk, 4), "sklearn_subspaces_timed": int(len(pick)), "speedup_vs_sklearn": round(t_sk / t_fit, 1)})
    except ImportError:
        row["sklearn_s"] = None


def run_cblof(d, n, count, C, reps, iters, baselines=True, sklearn_sample=20):
    X, m, p = subspaces_for(d, n, count, seed=d + n + count)
    Xd = torch.as_tensor(X, device="cuda")
    S, dims = len(m), m.sum(axis=1)
    rows = np.random.default_rng(0).choice(n, C, replace=False)

    def make(max_iter, stride=None):
        ens = vgan_amd.SubspaceCBLOF(m, p, n_clusters=C, init=rows, tol=0.0, max_iter=max_iter)
        if stride is not None:
            ens.poll_stride = stride
        return ens

    ens = make(iters)
    t_fit, ts = timed(lambda: ens.fit(Xd), reps)
    one = make(1)
    t_one, _ = timed(lambda: one.fit(Xd), reps)
    row = {"method": "cblof", "d": d, "n": n, "S_sampled": count, "S_distinct": S, "n_clusters": C, "max_iter": iters,
           "d_s_min": int(dims.min()), "d_s_median": float(np.median(dims)), "d_s_max": int(dims.max()),
           "gram_subspaces": int(ens.plan.gram.sum()), "n_iter_min": int(ens.n_iter_.min()), "n_iter_max": int(ens.n_iter_.max()),
           "fit_s": round(t_fit, 5), "fit_reps_s": ts, "fit_max_iter_1_s": round(t_one, 5),
           "per_iteration_s": round((t_fit - t_one) / max(iters - 1, 1), 6), "poll_stride_default": ens.poll_stride}
    dflt = vgan_amd.SubspaceCBLOF(m, p, n_clusters=C, init=rows, max_iter=iters)  # tol = 1e-4: the variances are taken too
    row["fit_default_tol_s"] = round(timed(lambda: dflt.fit(Xd), reps)[0], 5)
    row["n_iter_default_tol_min_max"] = [int(dflt.n_iter_.min()), int(dflt.n_iter_.max())]
    for stride in (1, 2, 4, 8, 16):
        e = make(iters, stride)
        row[f"fit_stride_{stride}_s"] = round(timed(lambda: e.fit(Xd), reps)[0], 5)
    if baselines:
        cblof_baselines(row, ens, X, Xd, m, p, rows, C, iters, reps, t_fit, sklearn_sample)
    # the E step composed from vgan_outlier_knn (k = 1, the centres as reference rows) against one whole iteration
    ops, dev = ens.ops, Xd.device
    jobs = []
    for first, cnt, gram in ens.plan.chunks(n, ens.workspace_bytes):
        Pq, sqq, img, img_sq, label, ws, tot, mx, eng = ens._lloyd_buffers(Xd, first, cnt, gram)
        jobs.append((first, cnt, eng, Pq, sqq, img, img_sq, tot, mx, ws, torch.empty(cnt, n, 1, dtype=torch.int32, device=dev), label))
    centers = ens._centers.clone()
    state = torch.zeros(3, S, dtype=torch.int32, device=dev)

    def knn_sweep():
        for first, cnt, eng, Pq, sqq, img, img_sq, _, _, _, nbr, _ in jobs:
            ops.outlier_knn(Pq, sqq, n, img, img_sq, C, ens._table, first, cnt, 1, False, eng, 1, nbr)

    def iteration():
        state.zero_()
        for first, cnt, eng, Pq, sqq, img, img_sq, tot, mx, ws, _, label in jobs:
            label.fill_(-1)
            ops.cluster_lloyd(Pq, sqq, Xd, ens._table, first, cnt, tot, mx, C, eng, ens._center, ens._tol_var, centers, img, img_sq,
                              label, state[0], state[1], state[2], ws, 1)

    row["knn_k1_sweep_s"] = round(timed(knn_sweep, max(reps, 5))[0], 6)
    row["one_iteration_s"] = round(timed(iteration, max(reps, 5))[0], 6)
    return row


def baseline_abod(X, feats, idx, block=8192):
    """torch on the same GPU from the same neighbour lists idx [n, k] of one subspace: float64 [n], NaN without a pair."""
    n, k = idx.shape
    Xs = X[:, feats].double()
    out = torch.empty(n, dtype=torch.float64, device=X.device)
    upper = torch.triu(torch.ones(k, k, dtype=torch.bool, device=X.device), diagonal=1)
    for q0 in range(0, n, block):
        V = Xs[idx[q0:q0 + block].long()] - Xs[q0:q0 + block, None, :]
        G = torch.bmm(V, V.transpose(1, 2))
        n2 = torch.diagonal(G, dim1=1, dim2=2)
        use = (n2 > 0)[:, :, None] & (n2 > 0)[:, None, :] & upper
        W = torch.where(use, G / (n2[:, :, None] * n2[:, None, :]), torch.zeros_like(G))
        cnt = use.sum(dim=(1, 2)).double()
        mean = W.sum(dim=(1, 2)) / cnt
        dev = torch.where(use, (W - mean[:, None, None]) ** 2, torch.zeros_like(G))
        out[q0:q0 + block] = -(dev.sum(dim=(1, 2)) / cnt)
    return out


def run_abod(d, n, count, k, reps, baselines=True):
    X, m, p = subspaces_for(d, n, count, seed=d + n + count)
    Xd = torch.as_tensor(X, device="cuda")
    S, dims = len(m), m.sum(axis=1)
    abod = vgan_amd.SubspaceABOD(m, p, n_neighbors=k)
    knn = vgan_amd.SubspaceEnsemble(m, p, method="knn", n_neighbors=k)
    t_abod, ta = timed(lambda: abod.fit(Xd), reps)
    t_knn, tk = timed(lambda: knn.fit(Xd), reps)
    # the launches alone, on the resident lists of the fit
    lists = [(first, cnt, idx) for first, cnt, idx, _ in abod._neighbors(None)]
    per = torch.empty(S, n, dtype=torch.float32, device="cuda")

    def launches():
        for first, cnt, idx in lists:
            abod.ops.outlier_abod(Xd, Xd, abod._table, first, cnt, idx, k, per, abod._rows[first:first + cnt])

    t_launch, tl = timed(launches, max(reps, 5))
    kp = 8 if k <= 8 else 16 if k <= 16 else 32
    gather_bytes = 4.0 * n * k * float(dims.sum())
    row = {"method": "abod", "d": d, "n": n, "S_sampled": count, "S_distinct": S, "k": k,
           "d_s_min": int(dims.min()), "d_s_median": float(np.median(dims)), "d_s_max": int(dims.max()),
           "abod_fit_s": round(t_abod, 5), "abod_fit_reps_s": ta, "knn_fit_s": round(t_knn, 5), "knn_fit_reps_s": tk,
           "abod_added_s": round(t_abod - t_knn, 5), "abod_over_knn": round(t_abod / t_knn, 3),
           "abod_launch_s": round(t_launch, 6), "abod_launch_reps_s": tl, "n_degenerate": int(abod.n_degenerate_.sum()),
           "gather_bytes": gather_bytes, "gather_GBps": round(gather_bytes / t_launch / 1e9, 1),
           "fp64_fma_nominal": float(n) * k * k * float(dims.sum()),
           "fp64_fma_nominal_per_s": round(float(n) * k * k * float(dims.sum()) / t_launch / 1e12, 3),
           "fp64_fma_executed_per_s": round(float(n) * kp * kp * float(dims.sum()) / t_launch / 1e12, 3)}
    if baselines:
        order = abod.plan.order
        feats = [torch.as_tensor(np.flatnonzero(m[s]), device="cuda") for s in range(S)]
        want = torch.empty(S, n, dtype=torch.float64, device="cuda")

        def torch_path():
            for first, cnt, idx in lists:
                for z in range(cnt):
                    s = int(order[first + z])
                    want[s] = baseline_abod(Xd, feats[s], idx[z])

        t_base, tb = timed(torch_path, reps)
        launches()
        got, ref = per.double(), want
        ok = ~torch.isnan(ref)
        rel = (got[ok] - ref[ok]).abs() / ref[ok].abs().clamp(min=1e-300)
        row.update({"torch_s": round(t_base, 5), "torch_reps_s": tb, "launch_speedup_vs_torch": round(t_base / t_launch, 2),
                    "max_rel_diff_vs_torch": float(rel.max()) if rel.numel() else 0.0,
                    "nan_rows_agree": bool((torch.isnan(per) == torch.isnan(ref)).all())})
    return row


def baseline_cof(X, feats, idx, block=2048):
    """torch on the same GPU from the same neighbour lists idx [n, k] of one subspace: the average chaining distance of the
    set-based nearest path, float64 [n].  The pairwise distances come from the differences (no Gram form)."""
    n, k = idx.shape
    Xs = X[:, feats].double()
    out = torch.empty(n, dtype=torch.float64, device=X.device)
    w = torch.tensor([2.0 * (k + 1 - i) / (k * (k + 1)) for i in range(1, k + 1)], dtype=torch.float64, device=X.device)
    for q0 in range(0, n, block):
        P = torch.cat([Xs[q0:q0 + block, None, :], Xs[idx[q0:q0 + block].long()]], dim=1)
        D2 = torch.cdist(P, P, compute_mode="donot_use_mm_for_euclid_dist") ** 2
        rows = torch.arange(P.shape[0], device=X.device)
        dist = D2[:, 0, 1:].clone()
        taken = torch.zeros_like(dist, dtype=torch.bool)
        ac = torch.zeros(P.shape[0], dtype=torch.float64, device=X.device)
        for i in range(k):
            m, j = dist.masked_fill(taken, float("inf")).min(dim=1)
            ac += w[i] * m.sqrt()
            taken[rows, j] = True
            dist = torch.minimum(dist, D2[rows, j + 1, 1:])
        out[q0:q0 + block] = ac
    return out


def run_cof(d, n, count, k, reps, baselines=True):
    X, m, p = subspaces_for(d, n, count, seed=d + n + count)
    Xd = torch.as_tensor(X, device="cuda")
    S, dims = len(m), m.sum(axis=1)
    cof = vgan_amd.SubspaceCOF(m, p, n_neighbors=k)
    knn = vgan_amd.SubspaceEnsemble(m, p, method="knn", n_neighbors=k)
    t_cof, tc = timed(lambda: cof.fit(Xd), reps)
    t_knn, tk = timed(lambda: knn.fit(Xd), reps)
    # the launches alone, on the resident lists of the fit
    lists = [(first, cnt, idx) for first, cnt, idx, _ in cof._neighbors(None)]
    ac = torch.empty(S, n, dtype=torch.float64, device="cuda")
    per = torch.empty(S, n, dtype=torch.float32, device="cuda")

    def chain_launches():
        for first, cnt, idx in lists:
            cof.ops.outlier_cof_chain(Xd, Xd, cof._table, first, cnt, idx, k, 0, ac[first:first + cnt])

    def score_launches():
        for first, cnt, idx in lists:
            cof.ops.outlier_cof_score(ac[first:first + cnt], ac[first:first + cnt], idx, k, per, cof._rows[first:first + cnt])

    t_launch, tl = timed(chain_launches, max(reps, 5))
    t_score, _ = timed(score_launches, max(reps, 5))
    kp = 8 if k <= 8 else 16 if k <= 16 else 32
    gather_bytes = 4.0 * n * (k + 1) * float(dims.sum())
    row = {"method": "cof", "chain": "sbn", "d": d, "n": n, "S_sampled": count, "S_distinct": S, "k": k,
           "d_s_min": int(dims.min()), "d_s_median": float(np.median(dims)), "d_s_max": int(dims.max()),
           "cof_fit_s": round(t_cof, 5), "cof_fit_reps_s": tc, "knn_fit_s": round(t_knn, 5), "knn_fit_reps_s": tk,
           "cof_added_s": round(t_cof - t_knn, 5), "cof_over_knn": round(t_cof / t_knn, 3),
           "chain_launch_s": round(t_launch, 6), "chain_launch_reps_s": tl, "chain_launch_over_knn_fit": round(t_launch / t_knn, 4),
           "score_launch_s": round(t_score, 6), "n_degenerate": int(cof.n_degenerate_.sum()),
           "gather_bytes": gather_bytes, "gather_GBps": round(gather_bytes / t_launch / 1e9, 1),
           "fp64_fma_nominal": float(n) * (k + 1) * (k + 1) * float(dims.sum()),
           "fp64_fma_nominal_per_s": round(float(n) * (k + 1) * (k + 1) * float(dims.sum()) / t_launch / 1e12, 3),
           "fp64_fma_executed_per_s": round(float(n) * (kp * kp + 1) * float(dims.sum()) / t_launch / 1e12, 3)}
    if baselines:
        order = cof.plan.order
        feats = [torch.as_tensor(np.flatnonzero(m[s]), device="cuda") for s in range(S)]
        want = torch.empty(S, n, dtype=torch.float64, device="cuda")

        def torch_path():
            for first, cnt, idx in lists:
                for z in range(cnt):
                    want[first + z] = baseline_cof(Xd, feats[int(order[first + z])], idx[z])

        t_base, tb = timed(torch_path, reps)
        chain_launches()
        rel = (ac - want).abs() / want.abs().clamp(min=1e-300)
        row.update({"torch_s": round(t_base, 5), "torch_reps_s": tb, "launch_speedup_vs_torch": round(t_base / t_launch, 2),
                    "max_rel_diff_vs_torch": float(rel.max())})
    return row


def torch_ecod(X, mask64, n, sorted_cols=None, sign=None):
    """The float64 torch restatement on the GPU: (scores [S, nq] float32, sorted, sign); sorted_cols None: the fit on X."""
    fitting = sorted_cols is None
    Xc = (X + 0.0).double()
    if fitting:
        sorted_cols = torch.sort(Xc, dim=0).values.t().contiguous()
        mu = Xc.sum(dim=0) / n
        e = Xc - mu
        m2, m3 = (e * e).sum(dim=0), (e * e * e).sum(dim=0)
        sign = torch.where(m2 == 0, torch.zeros_like(m3), torch.sign(m3))
    q = Xc.t().contiguous()
    cl = torch.searchsorted(sorted_cols, q, right=True).t()
    cr = n - torch.searchsorted(sorted_cols, q, right=False).t()
    a = 0 if fitting else 1
    ul, ur = -torch.log((cl + a).double() / (n + a)), -torch.log((cr + a).double() / (n + a))
    usk = torch.where(sign < 0, ul, torch.where(sign > 0, ur, ul + ur))
    O = torch.maximum(torch.maximum(ul, ur), usk)
    return (O @ mask64).t().float().contiguous(), sorted_cols, sign


def numpy_ecod(X, m, p):
    """numpy on the host: sort and searchsorted per feature, then one masked sum per subspace; float64 [n]."""
    A = X.astype(np.float64) + 0.0
    n, d = A.shape
    mu = A.sum(axis=0) / n
    m2, m3 = ((A - mu) ** 2).sum(axis=0), ((A - mu) ** 3).sum(axis=0)
    sign = np.where(m2 == 0, 0.0, np.sign(m3))
    O = np.empty_like(A)
    for f in range(d):
        col = np.sort(A[:, f])
        ul = -np.log(np.searchsorted(col, A[:, f], side="right") / n)
        ur = -np.log((n - np.searchsorted(col, A[:, f], side="left")) / n)
        usk = ul if sign[f] < 0 else ur if sign[f] > 0 else ul + ur
        O[:, f] = np.maximum(np.maximum(ul, ur), usk)
    out = np.zeros(n)
    for s in range(len(m)):
        out += p[s] * O[:, np.flatnonzero(m[s])].sum(axis=1).astype(np.float32).astype(np.float64)
    return out


def load_gather():
    import ctypes
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "bin", "libecod_gather.so")
    if not os.path.exists(path):
        raise SystemExit(f"{path} is missing: build it with the hipcc line in the header of tools/ecod_gather.hip")
    fn = ctypes.CDLL(path).ecod_gather_sum
    fn.restype = ctypes.c_int
    fn.argtypes = [ctypes.c_void_p, ctypes.c_long, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p,
                   ctypes.c_long, ctypes.c_void_p]
    return fn


def run_ecod(d, n, count, reps, baselines=True, random_masks=False):
    """random_masks: `count` random subspaces (every feature with probability 0.3) on N(0, 1) data instead of a model's: the
    product-against-gather comparison at a chosen S."""
    from vgan_amd.outlier import ECOD_AGGREGATES
    if random_masks:
        rng = np.random.default_rng(d + n + count)
        X = rng.normal(size=(n, d)).astype(np.float32)
        m = rng.random((count, d)) < 0.3
        m[np.arange(count), rng.integers(d, size=count)] = True
        p = np.full(count, 1.0 / count)
    else:
        X, m, p = subspaces_for(d, n, count, seed=d + n + count)
    Xd = torch.as_tensor(X, device="cuda")
    S, dims = len(m), m.sum(axis=1)
    ens = vgan_amd.SubspaceECOD(m, p)
    t_fit, tf = timed(lambda: ens.fit(Xd), reps)
    t_dec, td = timed(lambda: ens.decision_function(Xd), reps)
    ops, dev, inner = ens.ops, Xd.device, max(reps, 5)
    rows = min(ens._chunk_rows(), n)
    sorted_cols, sign = torch.empty_like(ens._sorted), torch.empty_like(ens._sign)
    cl, cr = (torch.empty(rows * d, dtype=torch.int32, device=dev) for _ in range(2))
    terms = torch.empty(rows * d, dtype=torch.float64, device=dev)
    per = torch.empty(S, n, dtype=torch.float32, device=dev)
    one = torch.ones(d, 1, dtype=torch.float64, device=dev)
    per_one = torch.empty(1, n, dtype=torch.float32, device=dev)
    agg = ECOD_AGGREGATES["dimension"]
    t_sort, _ = timed(lambda: ops.ecod_sort_columns(Xd, sorted_cols), inner)
    t_skew, _ = timed(lambda: ops.ecod_skew_sign(sorted_cols, n, sign), inner)
    r1 = min(rows, n)  # the split below is taken on the first chunk and scaled by the number of rows
    t_counts, _ = timed(lambda: ops.ecod_tail_counts(Xd[:r1], sorted_cols, n, cl, cr), inner)
    t_scores, _ = timed(lambda: ops.ecod_scores(cl, cr, r1, sign, n, False, agg, ens._mask, terms, per[:, :r1]), inner)
    t_terms, _ = timed(lambda: ops.ecod_scores(cl, cr, r1, sign, n, False, agg, one, terms, per_one[:, :r1]), inner)
    gather = load_gather()
    feat, feat_off = ens._table[0], ens._table[1]  # the processing order is the given order here
    out_g = torch.empty(S, n, dtype=torch.float32, device=dev)
    stream = torch.cuda.current_stream().cuda_stream

    def gather_sum():
        rc = gather(terms.data_ptr(), r1, d, feat.data_ptr(), feat_off.data_ptr(), S, out_g.data_ptr(), n, stream)
        assert rc == 0, rc

    t_gather, _ = timed(gather_sum, inner)
    ops.ecod_scores(cl, cr, r1, sign, n, False, agg, ens._mask, terms, per[:, :r1])
    gather_sum()
    a, b = per[:, :r1].double(), out_g[:, :r1].double()
    scale = n / r1
    t_product = max(t_scores - t_terms, 0.0)
    row = {"method": "ecod", "d": d, "n": n, "S_sampled": None if random_masks else count, "S_distinct": S, "aggregate": "dimension",
           "subspaces": "random, density 0.3" if random_masks else "approx_subspace_dist",
           "d_s_min": int(dims.min()), "d_s_median": float(np.median(dims)), "d_s_max": int(dims.max()),
           "row_chunks": -(-n // rows), "fit_s": round(t_fit, 6), "fit_reps_s": tf, "decision_function_s": round(t_dec, 6),
           "decision_function_reps_s": td, "sort_s": round(t_sort, 6), "skew_s": round(t_skew, 6),
           "counts_s": round(t_counts * scale, 6), "terms_and_product_s": round(t_scores * scale, 6),
           "terms_alone_s": round(t_terms * scale, 6), "product_s": round(t_product * scale, 6),
           "gather_sum_s": round(t_gather * scale, 6),
           "product_over_gather": round(t_product / t_gather, 3) if t_gather > 0 else None,
           "product_fp64_gflops": round(2.0 * r1 * d * S / max(t_product, 1e-9) / 1e9, 1),
           "max_rel_diff_product_vs_gather": float(((a - b).abs() / b.abs().clamp(min=1e-300)).max())}
    if baselines:
        mask64 = ens._mask
        t_tfit, ttf = timed(lambda: torch_ecod(Xd, mask64, n), reps)
        want, sc, sg = torch_ecod(Xd, mask64, n)
        t_tdec, ttd = timed(lambda: torch_ecod(Xd, mask64, n, sc, sg), reps)
        got = torch.as_tensor(ens.per_subspace_scores_, device=dev).double()
        rel = (got - want.double()).abs() / want.double().abs().clamp(min=1e-300)
        t0 = time.perf_counter()
        host = numpy_ecod(X, m, p)
        t_host = time.perf_counter() - t0
        row.update({"torch_fit_s": round(t_tfit, 6), "torch_fit_reps_s": ttf, "torch_decision_function_s": round(t_tdec, 6),
                    "torch_decision_function_reps_s": ttd, "fit_speedup_vs_torch": round(t_tfit / t_fit, 2),
                    "decision_function_speedup_vs_torch": round(t_tdec / t_dec, 2), "max_rel_diff_vs_torch": float(rel.max()),
                    "skew_signs_agree_with_torch": bool((sg.cpu().numpy() == ens.skew_sign_).all()),
                    "numpy_host_fit_s": round(t_host, 4), "fit_speedup_vs_numpy": round(t_host / t_fit, 1),
                    "max_rel_diff_vs_numpy": float(np.max(np.abs(ens.decision_scores_ - host) / np.maximum(np.abs(host), 1e-300)))})
    return row


def torch_histograms(Z, B):
    """(edges [P, B + 1], counts [P, B]) of the columns of the float64 matrix Z [n, P], in torch on the device."""
    lo, hi = Z.min(dim=0).values, Z.max(dim=0).values
    same = lo == hi
    lo, hi = torch.where(same, lo - 0.5, lo), torch.where(same, hi + 0.5, hi)
    step = (hi - lo) / B
    edges = torch.arange(B + 1, dtype=torch.float64, device=Z.device)[None, :] * step[:, None] + lo[:, None]
    edges[:, B] = hi
    bins = torch.searchsorted(edges[:, 1:B].contiguous(), Z.t().contiguous(), right=True)
    counts = torch.zeros(Z.shape[1], B, dtype=torch.int64, device=Z.device).scatter_add_(1, bins, torch.ones_like(bins))
    return edges, counts


def torch_hbos(X, mask64, B, alpha, tol):
    """float32 [S, n]: the float64 torch restatement of the HBOS fit on the GPU."""
    Z = (X + 0.0).double()
    n = Z.shape[0]
    edges, counts = torch_histograms(Z, B)
    step = (edges[:, B] - edges[:, 0]) / B
    dens = counts.double() / (n * step)[:, None]
    term = -torch.log2(dens + alpha)
    rare = -torch.log2(dens.min(dim=1).values + alpha)
    bins = torch.searchsorted(edges[:, 1:B].contiguous(), Z.t().contiguous(), right=True)
    T = torch.gather(term, 1, bins)
    outside = (Z.t() < (edges[:, 0] - tol * step)[:, None]) | (Z.t() > (edges[:, B] + tol * step)[:, None])
    T = torch.where(outside, rare[:, None], T)
    return (mask64.t() @ T).float().contiguous()


def numpy_hbos(X, m, p, B, alpha, tol):
    """numpy on the host: numpy.histogram and searchsorted per feature, then one masked sum per subspace; float64 [n]."""
    A = X.astype(np.float64) + 0.0
    n, d = A.shape
    T = np.empty_like(A)
    for f in range(d):
        counts, edges = np.histogram(A[:, f], bins=B)
        step = (edges[-1] - edges[0]) / B
        dens = counts / (n * step)
        T[:, f] = -np.log2(dens + alpha)[np.searchsorted(edges[1:B], A[:, f], side="right")]  # the fitted rows are never outside
    out = np.zeros(n)
    for s in range(len(m)):
        out += p[s] * T[:, np.flatnonzero(m[s])].sum(axis=1).astype(np.float32).astype(np.float64)
    return out


def hist_row_head(method, d, n, count, S, dims, ens, Xd, reps):
    t_fit, tf = timed(lambda: ens.fit(Xd), reps)
    t_dec, td = timed(lambda: ens.decision_function(Xd), reps)
    return {"method": method, "d": d, "n": n, "S_sampled": count, "S_distinct": S, "n_bins": ens.n_bins,
            "d_s_min": int(dims.min()), "d_s_median": float(np.median(dims)), "d_s_max": int(dims.max()),
            "fit_s": round(t_fit, 6), "fit_reps_s": tf, "decision_function_s": round(t_dec, 6), "decision_function_reps_s": td}


def ecod_beside(row, m, p, Xd, reps):
    ecod = vgan_amd.SubspaceECOD(m, p)
    t_ecod, te = timed(lambda: ecod.fit(Xd), reps)
    row.update({"ecod_fit_s": round(t_ecod, 6), "ecod_fit_reps_s": te, "ecod_over_fit": round(t_ecod / row["fit_s"], 2)})


def run_hbos(d, n, count, reps, baselines=True):
    from vgan_amd.outlier import hbos_chunk_rows, hbos_term_table
    X, m, p = subspaces_for(d, n, count, seed=d + n + count)
    Xd = torch.as_tensor(X, device="cuda")
    S, dims = len(m), m.sum(axis=1)
    ens = vgan_amd.SubspaceHBOS(m, p)
    row = hist_row_head("hbos", d, n, count, S, dims, ens, Xd, reps)
    ops, dev, inner, B = ens.ops, Xd.device, max(reps, 5), ens.n_bins
    rows = min(hbos_chunk_rows(d, S, ens.workspace_bytes), n)
    keys = torch.empty(d, 2, dtype=torch.int64, device=dev)
    edges, counts = torch.empty_like(ens._edges), torch.empty(d, B, dtype=torch.int32, device=dev)
    terms = torch.empty(rows * d, dtype=torch.float64, device=dev)
    per = torch.empty(S, n, dtype=torch.float32, device=dev)
    one = torch.ones(d, 1, dtype=torch.float64, device=dev)
    per_one = torch.empty(1, n, dtype=torch.float32, device=dev)
    t_range, _ = timed(lambda: ops.hist_column_range(Xd, keys), inner)
    t_edges, _ = timed(lambda: ops.hist_edges(keys, B, edges), inner)
    t_count, _ = timed(lambda: ops.hist_column_counts(Xd, edges, counts), inner)
    t_scores, _ = timed(lambda: ops.hbos_scores(Xd[:rows], ens._edges, ens._terms, ens._limits, ens._mask, terms, per[:, :rows]), inner)
    t_lookup, _ = timed(lambda: ops.hbos_scores(Xd[:rows], ens._edges, ens._terms, ens._limits, one, terms, per_one[:, :rows]), inner)
    t0 = time.perf_counter()
    hbos_term_table(counts.cpu().numpy(), edges.cpu().numpy(), n, ens.alpha, ens.tol)
    t_host = time.perf_counter() - t0
    scale = n / rows  # the split of scoring is taken on the first chunk and scaled by the number of rows
    t_product = max(t_scores - t_lookup, 0.0)
    row.update({"row_chunks": -(-n // rows), "range_s": round(t_range, 6), "edges_s": round(t_edges, 6), "count_s": round(t_count, 6),
                "count_copy_and_host_table_s": round(t_host, 6), "lookup_and_product_s": round(t_scores * scale, 6),
                "lookup_alone_s": round(t_lookup * scale, 6), "product_s": round(t_product * scale, 6),
                "range_gb_s": round(4.0 * n * d / t_range / 1e9, 1), "count_gb_s": round(4.0 * n * d / t_count / 1e9, 1),
                "product_fp64_gflops": round(2.0 * rows * d * S / max(t_product, 1e-9) / 1e9, 1)})
    ecod_beside(row, m, p, Xd, reps)
    if baselines:
        t_torch, tt = timed(lambda: torch_hbos(Xd, ens._mask, B, ens.alpha, ens.tol), reps)
        want = torch_hbos(Xd, ens._mask, B, ens.alpha, ens.tol).double()
        got = torch.as_tensor(ens.per_subspace_scores_, device=dev).double()
        t0 = time.perf_counter()
        host = numpy_hbos(X, m, p, B, ens.alpha, ens.tol)
        t_np = time.perf_counter() - t0
        row.update({"torch_fit_s": round(t_torch, 6), "torch_fit_reps_s": tt, "fit_speedup_vs_torch": round(t_torch / row["fit_s"], 2),
                    "max_abs_diff_vs_torch": float((got - want).abs().max()), "numpy_host_fit_s": round(t_np, 4),
                    "fit_speedup_vs_numpy": round(t_np / row["fit_s"], 1),
                    "max_abs_diff_vs_numpy": float(np.max(np.abs(ens.decision_scores_ - host)))})
    return row


def torch_loda(X, feats, features, weights, B):
    """float32 [S, n]: a float64 torch restatement of the LODA fit on the GPU, subspace by subspace (a dense projection
    matrix and one matmul: its z differ from the contract's in the last bits, so a value may change its bin)."""
    n = X.shape[0]
    out = torch.empty(len(feats), n, dtype=torch.float32, device=X.device)
    for s, f in enumerate(feats):
        k, d_s = features[s].shape[0], len(f)
        W = np.zeros((d_s, k))
        W[features[s], np.arange(k)[:, None]] = weights[s]
        Z = X[:, torch.as_tensor(f, device=X.device)].double() @ torch.as_tensor(W, device=X.device)
        edges, counts = torch_histograms(Z, B)
        term = -torch.log((counts.double() + 1e-12) / (n + B * 1e-12))
        bins = torch.searchsorted(edges[:, 1:B].contiguous(), Z.t().contiguous(), right=True)
        out[s] = torch.gather(term, 1, bins).mean(dim=0).float()
    return out


def numpy_loda_one(Xs, features, weights, B):
    n, k = Xs.shape[0], features.shape[0]
    W = np.zeros((Xs.shape[1], k))
    W[features, np.arange(k)[:, None]] = weights
    Z = Xs.astype(np.float64) @ W
    total = np.zeros(n)
    for j in range(k):
        counts, edges = np.histogram(Z[:, j], bins=B)
        total += -np.log((counts + 1e-12) / (n + B * 1e-12))[np.searchsorted(edges[1:B], Z[:, j], side="right")]
    return total / k


def run_loda(d, n, count, reps, baselines=True, numpy_sample=8):
    from vgan_amd.outlier import loda_chunks, loda_projections, loda_term_table
    X, m, p = subspaces_for(d, n, count, seed=d + n + count)
    Xd = torch.as_tensor(X, device="cuda")
    S, dims = len(m), m.sum(axis=1)
    ens = vgan_amd.SubspaceLODA(m, p)
    row = hist_row_head("loda", d, n, count, S, dims, ens, Xd, reps)
    ops, dev, inner = ens.ops, Xd.device, max(reps, 5)
    k, B = ens.n_projections, ens.n_bins
    rows, ranges = loda_chunks(ens.plan.dims, n, ens.workspace_bytes)
    keys = torch.empty(S, k, 2, dtype=torch.int64, device=dev)
    counts = torch.empty(S, k, B, dtype=torch.int32, device=dev)
    per = torch.empty(S, n, dtype=torch.float32, device=dev)

    def pack_pass():
        for _ in ens._blocks(Xd):
            pass

    def range_pass():
        ops.hist_reset(keys=keys)
        for packed, r, _, first, cnt, width in ens._blocks(Xd):
            ops.loda_range(packed, r, ens._table, first, cnt, width, ens._proj, keys)

    def count_pass():
        ops.hist_reset(counts=counts)
        for packed, r, _, first, cnt, width in ens._blocks(Xd):
            ops.loda_counts(packed, r, ens._table, first, cnt, width, ens._proj, ens._edges, counts)

    def score_pass():
        for packed, r, r0, first, cnt, width in ens._blocks(Xd):
            ops.loda_scores(packed, r, ens._table, first, cnt, width, ens._proj, ens._edges, ens._terms, per[:, r0:r0 + r])

    t0 = time.perf_counter()
    loda_projections(ens.plan.dims, k, ens.seed)
    t_draw = time.perf_counter() - t0
    t_pack, _ = timed(pack_pass, inner)
    t_range, _ = timed(range_pass, inner)
    t_count, _ = timed(count_pass, inner)
    t_score, _ = timed(score_pass, inner)
    t0 = time.perf_counter()
    loda_term_table(counts.cpu().numpy(), n)
    t_host = time.perf_counter() - t0
    nonzeros = float(sum(f.size for f in ens.projection_features_))  # sum_s k m_s
    row.update({"n_projections": k, "row_chunks": -(-n // rows), "subspace_ranges": len(ranges), "draw_projections_host_s": round(t_draw, 4),
                "pack_pass_s": round(t_pack, 6), "range_pass_s": round(t_range, 6), "count_pass_s": round(t_count, 6),
                "score_pass_s": round(t_score, 6), "count_copy_and_host_table_s": round(t_host, 6),
                "projection_fp64_gflops_of_score_pass": round(2.0 * n * nonzeros / max(t_score - t_pack, 1e-9) / 1e9, 1)})
    ecod_beside(row, m, p, Xd, reps)
    if baselines:
        feats = [np.flatnonzero(m[s]) for s in range(S)]
        args = (Xd, feats, ens.projection_features_, ens.projection_weights_, B)
        t_torch, tt = timed(lambda: torch_loda(*args), reps)
        want = torch_loda(*args).double()
        got = torch.as_tensor(ens.per_subspace_scores_, device=dev).double()
        pick = np.unique(np.linspace(0, S - 1, min(S, numpy_sample)).astype(int))
        t0 = time.perf_counter()
        diff = 0.0
        for s in pick:
            host = numpy_loda_one(X[:, feats[s]], ens.projection_features_[s], ens.projection_weights_[s], B)
            diff = max(diff, float(np.abs(host - ens.per_subspace_scores_[s]).mean()))
        t_np = (time.perf_counter() - t0) * S / len(pick)
        row.update({"torch_fit_s": round(t_torch, 6), "torch_fit_reps_s": tt, "fit_speedup_vs_torch": round(t_torch / row["fit_s"], 2),
                    "mean_abs_diff_vs_torch": float((got - want).abs().mean()), "numpy_host_fit_s": round(t_np, 4),
                    "numpy_subspaces_timed": int(len(pick)), "fit_speedup_vs_numpy": round(t_np / row["fit_s"], 1),
                    "mean_abs_diff_vs_numpy_max": diff})
    return row


def run_iforest_oblique(d, n, count, reps, q):
    """--n-dims q >= 2: fit, its build and walk launches alone, decision_function and the fitted state of the oblique forest;
    beside it, in the same process, the axis-parallel forest and SubspaceDIF on the same rows."""
    X, m, p = subspaces_for(d, n, count, seed=d + n + count)
    Xd = torch.as_tensor(X, device="cuda")
    S, dims = len(m), m.sum(axis=1)
    ens = vgan_amd.SubspaceIForest(m, p, n_dims=q)
    t_fit, tf = timed(lambda: ens.fit(Xd), reps)
    t_dec, td = timed(lambda: ens.decision_function(Xd), reps)
    ops, inner = ens.ops, max(reps, 5)
    T, psi, L = ens.n_estimators, ens.max_samples_, ens.depth_limit_
    trees, planes = torch.empty_like(ens._trees), tuple(torch.empty_like(t) for t in ens._planes)
    sums = torch.empty(S * n, dtype=torch.int64, device="cuda")
    cand = [c for c in ens.candidate_features_]
    off = np.zeros(S + 1, np.int32)
    np.cumsum([len(c) for c in cand], out=off[1:])
    cand_d, off_d = torch.as_tensor(np.concatenate(cand + [np.zeros(1, np.int32)]), device="cuda"), torch.as_tensor(off, device="cuda")
    t_build, _ = timed(lambda: ops.iforest_build_oblique(Xd, cand_d, off_d, 0, S, psi, L, ens.seed, trees, *planes), inner)
    t_sums, _ = timed(lambda: ops.iforest_path_sums_oblique(Xd, ens._trees, *ens._planes, 0, S, psi, L, ens._cq, sums), inner)
    depth = float((sums.view(S, n) >> 32).double().mean()) / T  # the mean number of steps of a walk
    row = {"method": "iforest", "n_dims": q, "d": d, "n": n, "S_sampled": count, "S_distinct": S, "n_estimators": T, "max_samples": psi,
           "d_s_min": int(dims.min()), "d_s_median": float(np.median(dims)), "d_s_max": int(dims.max()),
           "fit_s": round(t_fit, 6), "fit_reps_s": tf, "decision_function_s": round(t_dec, 6), "decision_function_reps_s": td,
           "build_s": round(t_build, 6), "path_sums_s": round(t_sums, 6),
           "state_bytes": int(ens._trees.numel() * 4 + sum(t.numel() * 4 for t in ens._planes)), "mean_depth": round(depth, 3),
           "walk_steps_per_s": round(S * T * n * depth / t_sums / 1e9, 2), "walk_steps_unit": "1e9 steps / s",
           "build_loads_nominal": float(psi) * float(np.minimum(dims, q).sum()) * T * L,
           "walk_gathers_nominal": float(S) * T * n * depth * q}
    flat = vgan_amd.SubspaceIForest(m, p)
    t_flat, tl = timed(lambda: flat.fit(Xd), reps)
    flat_trees = torch.empty_like(flat._trees)
    t_fb, _ = timed(lambda: ops.iforest_build(Xd, flat._table, 0, S, int(dims.max()), psi, L, flat.seed, flat_trees), inner)
    t_fs, _ = timed(lambda: ops.iforest_path_sums(Xd, flat._trees, 0, S, psi, L, flat._cq, sums), inner)
    t_fd, _ = timed(lambda: flat.decision_function(Xd), reps)
    row.update({"axis_fit_s": round(t_flat, 6), "axis_fit_reps_s": tl, "axis_build_s": round(t_fb, 6), "axis_path_sums_s": round(t_fs, 6),
                "axis_decision_function_s": round(t_fd, 6), "axis_state_bytes": int(flat._trees.numel() * 4),
                "axis_build_loads_nominal": float(psi) * float(dims.sum()) * T * L})
    dif = vgan_amd.SubspaceDIF(m, p)
    t_dif, tdf = timed(lambda: dif.fit(Xd), reps)
    row.update({"dif_fit_s": round(t_dif, 6), "dif_fit_reps_s": tdf})
    return row


def run_iforest(d, n, count, reps, baselines=True, sklearn_sample=8, n_dims=1):
    if n_dims > 1:
        return run_iforest_oblique(d, n, count, reps, n_dims)
    X, m, p = subspaces_for(d, n, count, seed=d + n + count)
    Xd = torch.as_tensor(X, device="cuda")
    S, dims = len(m), m.sum(axis=1)
    ens = vgan_amd.SubspaceIForest(m, p)
    t_fit, tf = timed(lambda: ens.fit(Xd), reps)
    t_dec, td = timed(lambda: ens.decision_function(Xd), reps)
    ops, inner = ens.ops, max(reps, 5)
    T, psi, L = ens.n_estimators, ens.max_samples_, ens.depth_limit_
    trees = torch.empty_like(ens._trees)
    sums = torch.empty(S * n, dtype=torch.int64, device="cuda")
    per = torch.empty(S, n, dtype=torch.float32, device="cuda")
    t_build, _ = timed(lambda: ops.iforest_build(Xd, ens._table, 0, S, int(dims.max()), psi, L, ens.seed, trees), inner)
    t_sums, _ = timed(lambda: ops.iforest_path_sums(Xd, ens._trees, 0, S, psi, L, ens._cq, sums), inner)
    t_scores, _ = timed(lambda: ops.iforest_scores(sums, S, n, ens._denom, per), inner)
    depth = float((sums.view(S, n) >> 32).double().mean()) / T  # the mean number of steps of a walk
    row = {"method": "iforest", "d": d, "n": n, "S_sampled": count, "S_distinct": S, "n_estimators": T, "max_samples": psi,
           "d_s_min": int(dims.min()), "d_s_median": float(np.median(dims)), "d_s_max": int(dims.max()),
           "fit_s": round(t_fit, 6), "fit_reps_s": tf, "decision_function_s": round(t_dec, 6), "decision_function_reps_s": td,
           "build_s": round(t_build, 6), "path_sums_s": round(t_sums, 6), "scores_s": round(t_scores, 6),
           "tree_bytes": int(ens._trees.numel() * 4), "mean_depth": round(depth, 3),
           "walk_steps_per_s": round(S * T * n * depth / t_sums / 1e9, 2), "walk_steps_unit": "1e9 steps / s",
           "build_loads_nominal": float(psi) * float(dims.sum()) * T * L}
    knn = vgan_amd.SubspaceEnsemble(m, p, method="knn", n_neighbors=5)
    t_knn, tk = timed(lambda: knn.fit(Xd), reps)
    row.update({"knn_fit_s": round(t_knn, 5), "knn_fit_reps_s": tk, "knn_over_iforest_fit": round(t_knn / t_fit, 2)})
    if baselines:
        try:
            from sklearn.ensemble import IsolationForest
            pick = np.unique(np.linspace(0, S - 1, min(S, sklearn_sample)).astype(int))
            t_sk_fit = t_sk_score = 0.0
            rank = []
            for s in pick:
                Xs = np.ascontiguousarray(X[:, np.flatnonzero(m[s])])
                t0 = time.perf_counter()
                model = IsolationForest(n_estimators=100, n_jobs=16, random_state=0).fit(Xs)
                t1 = time.perf_counter()
                theirs = -model.score_samples(Xs)
                t_sk_score += time.perf_counter() - t1
                t_sk_fit += t1 - t0
                ours = ens.per_subspace_scores_[s].astype(np.float64)
                rank.append(float(np.corrcoef(np.argsort(np.argsort(ours)), np.argsort(np.argsort(theirs)))[0, 1]))
            scale = S / len(pick)
            row.update({"sklearn_trees_s": round(t_sk_fit * scale, 4), "sklearn_score_s": round(t_sk_score * scale, 4),
                        "sklearn_fit_and_score_s": round((t_sk_fit + t_sk_score) * scale, 4), "sklearn_subspaces_timed": int(len(pick)),
                        "fit_speedup_vs_sklearn": round((t_sk_fit + t_sk_score) * scale / t_fit, 1),
                        "rank_correlation_with_sklearn_min": round(min(rank), 4)})
        except ImportError:
            row["sklearn_fit_and_score_s"] = None
    return row


def torch_maha(X, feats, alpha):
    """float32 [S, n]: the squared Mahalanobis distances of the contract, float64 torch on the device, subspace by subspace."""
    n = X.shape[0]
    per = torch.empty(len(feats), n, dtype=torch.float32, device=X.device)
    for s, f in enumerate(feats):
        Z = X[:, f].double()
        Z = Z - Z.mean(dim=0)
        C = Z.T @ Z / n
        Sigma = (1.0 - alpha) * C
        Sigma.diagonal().add_(alpha * torch.trace(C) / C.shape[0])
        L = torch.linalg.cholesky(Sigma)  # raises where the factor does not exist
        Y = torch.linalg.solve_triangular(L, Z.T, upper=False)
        per[s] = (Y * Y).sum(dim=0).float()
    return per


def run_maha(d, n, count, reps, baselines=True, sklearn_sample=8):
    X, m, p = subspaces_for(d, n, count, seed=d + n + count)
    Xd = torch.as_tensor(X, device="cuda")
    S, dims = len(m), m.sum(axis=1)
    ens = vgan_amd.SubspaceMahalanobis(m, p)
    t_fit, tf = timed(lambda: ens.fit(Xd), reps)
    t_dec, td = timed(lambda: ens.decision_function(Xd), reps)
    robust = vgan_amd.SubspaceMahalanobis(m, p, robust=True)
    t_rob, tr = timed(lambda: robust.fit(Xd), reps)
    inner = max(reps, 5)
    ens._prepare(n, Xd.device)
    hcount = torch.full((S,), n, dtype=torch.int32, device="cuda")
    t_mom, _ = timed(lambda: ens._moments(Xd, None, hcount), inner)

    def factor():  # the factor overwrites C with Sigma: every repetition starts from fresh moments
        ens._moments(Xd, None, hcount)
        ens._factor(hcount)
    t_mf, _ = timed(factor, inner)
    t_sc, _ = timed(lambda: ens._distances(Xd), inner)
    ens.fit(Xd)
    flops = 2.0 * n * float((dims.astype(np.float64) ** 2).sum())
    row = {"method": "mahalanobis", "d": d, "n": n, "S_sampled": count, "S_distinct": S, "d_s_min": int(dims.min()),
           "d_s_median": float(np.median(dims)), "d_s_max": int(dims.max()), "fit_s": round(t_fit, 6), "fit_reps_s": tf,
           "decision_function_s": round(t_dec, 6), "decision_function_reps_s": td, "robust_fit_s": round(t_rob, 6),
           "robust_fit_reps_s": tr, "robust_csteps_max": int(robust.n_csteps_.max()), "robust_converged": int(robust.converged_.sum()),
           "moments_s": round(t_mom, 6), "factor_s": round(t_mf - t_mom, 6), "scores_s": round(t_sc, 6),
           "scores_full_product_tflops": round(flops / t_sc / 1e12, 3), "moments_full_product_tflops": round(flops / t_mom / 1e12, 3),
           "state_bytes": int(3 * 8 * (dims.astype(np.int64) ** 2).sum())}
    if baselines:
        feats = [torch.as_tensor(np.flatnonzero(m[s]), device="cuda") for s in range(S)]
        ours = ens.per_subspace_scores_.astype(np.float64)
        try:
            t_torch, tt = timed(lambda: torch_maha(Xd, feats, 0.1), reps)
            theirs = torch_maha(Xd, feats, 0.1).cpu().numpy().astype(np.float64)
            row.update({"torch_f64_s": round(t_torch, 6), "torch_f64_reps_s": tt, "fit_speedup_vs_torch": round(t_torch / t_fit, 2),
                        "max_rel_diff_vs_torch": float(np.max(np.abs(ours - theirs) / np.maximum(np.abs(theirs), 1e-300)))})
        except RuntimeError as e:  # the baseline's own failure (hipBLAS could not allocate at d = 784, n = 5e4) is recorded, not hidden
            row.update({"torch_f64_s": None, "torch_f64_error": str(e).splitlines()[0]})
        try:
            from sklearn.covariance import ShrunkCovariance
            pick = np.unique(np.linspace(0, S - 1, min(S, sklearn_sample)).astype(int))
            t_sk, worst = 0.0, 0.0
            for s in pick:
                Xs = np.ascontiguousarray(X[:, np.flatnonzero(m[s])]).astype(np.float64)
                t0 = time.perf_counter()
                dist = ShrunkCovariance(shrinkage=0.1).fit(Xs).mahalanobis(Xs)
                t_sk += time.perf_counter() - t0
                worst = max(worst, float(np.max(np.abs(ours[s] - dist) / np.maximum(np.abs(dist), 1e-300))))
            scale = S / len(pick)
            row.update({"sklearn_fit_and_score_s": round(t_sk * scale, 4), "sklearn_subspaces_timed": int(len(pick)),
                        "fit_speedup_vs_sklearn": round(t_sk * scale / t_fit, 1), "max_rel_diff_vs_sklearn": worst})
        except ImportError:
            row["sklearn_fit_and_score_s"] = None
    return row


def run_pca(d, n, count, reps, baselines=True, sklearn_sample=8):
    """SubspacePCA (all components, weighted, standardised) at one shape: fit and decision_function, the eigen launch and the
    scoring launch on their own, SubspaceMahalanobis beside them, sklearn's StandardScaler + PCA on a sample of subspaces."""
    X, m, p = subspaces_for(d, n, count, seed=d + n + count)
    Xd = torch.as_tensor(X, device="cuda")
    S, dims = len(m), m.sum(axis=1)
    ens = vgan_amd.SubspacePCA(m, p)
    t_fit, tf = timed(lambda: ens.fit(Xd), reps)
    t_dec, td = timed(lambda: ens.decision_function(Xd), reps)
    inner = max(reps, 5)
    t_sc, _ = timed(lambda: ens._distances(Xd), inner)
    minor = vgan_amd.SubspacePCA(m, p, components="minor", n_components=0.9, weighted=False).fit(Xd)
    t_minor, _ = timed(lambda: minor._distances(Xd), inner)
    probe = vgan_amd.SubspacePCA(m, p)
    probe._begin_fit(Xd)
    probe._prepare(n, Xd.device)
    t_mom, _ = timed(lambda: probe._moments(Xd), inner)

    def eigen():  # the solver overwrites C: every repetition starts from fresh moments
        probe._moments(Xd)
        probe._eigen()
    t_me, _ = timed(eigen, reps)
    maha = vgan_amd.SubspaceMahalanobis(m, p)
    t_maha_fit, _ = timed(lambda: maha.fit(Xd), reps)
    t_maha_sc, _ = timed(lambda: maha._distances(Xd), inner)
    flops = 2.0 * n * float((dims.astype(np.float64) ** 2).sum())
    row = {"method": "pca", "d": d, "n": n, "S_sampled": count, "S_distinct": S, "d_s_min": int(dims.min()),
           "d_s_median": float(np.median(dims)), "d_s_max": int(dims.max()), "fit_s": round(t_fit, 6), "fit_reps_s": tf,
           "decision_function_s": round(t_dec, 6), "decision_function_reps_s": td, "moments_s": round(t_mom, 6),
           "eigen_s": round(t_me - t_mom, 6), "scores_s": round(t_sc, 6), "scores_minor_0.9_s": round(t_minor, 6),
           "scores_tflops": round(flops / t_sc / 1e12, 3), "sweeps_max": int(ens.n_sweeps_.max()),
           "sweeps_median": float(np.median(ens.n_sweeps_)), "converged": int(ens.converged_.sum()),
           "mahalanobis_fit_s": round(t_maha_fit, 6), "mahalanobis_scores_s": round(t_maha_sc, 6),
           "scores_over_mahalanobis_scores": round(t_sc / t_maha_sc, 2), "state_bytes": int(8 * (dims.astype(np.int64) ** 2).sum())}
    if baselines:
        try:
            from sklearn.decomposition import PCA
            from sklearn.preprocessing import StandardScaler
            pick = np.unique(np.linspace(0, S - 1, min(S, sklearn_sample)).astype(int))
            t_sk, worst = 0.0, 0.0
            for s in pick:
                Xs = np.ascontiguousarray(X[:, np.flatnonzero(m[s])]).astype(np.float64)
                t0 = time.perf_counter()
                model = PCA().fit(StandardScaler().fit_transform(Xs))
                t_sk += time.perf_counter() - t0
                k = len(model.explained_variance_)
                want = model.explained_variance_ * (n - 1) / n
                worst = max(worst, float(np.max(np.abs(ens.explained_variance_[s][:k] - want)) / want[0]))
            scale = S / len(pick)
            row.update({"sklearn_fit_s": round(t_sk * scale, 4), "sklearn_subspaces_timed": int(len(pick)),
                        "fit_speedup_vs_sklearn": round(t_sk * scale / t_fit, 1), "max_eigenvalue_diff_vs_sklearn_over_lambda_1": worst})
        except ImportError:
            row["sklearn_fit_s"] = None
    return row


def run_pca_widths(n, widths, reps):
    """The eigen launch alone on one subspace of each width (the first features of a d = 784 synthetic set): time and sweeps."""
    rows = []
    for w in widths:
        X = np.random.default_rng(784 + n).normal(size=(n, 784)).astype(np.float32)
        X[:, 1] = X[:, 0] + 0.1 * X[:, 1]
        m = np.zeros((1, 784), bool)
        m[0, np.random.default_rng(w).choice(784, w, replace=False)] = True
        Xd = torch.as_tensor(X, device="cuda")
        probe = vgan_amd.SubspacePCA(m, [1.0])
        probe._begin_fit(Xd)
        probe._prepare(n, Xd.device)
        t_mom, _ = timed(lambda: probe._moments(Xd), reps)

        def eigen():
            probe._moments(Xd)
            probe._eigen()
        t_me, _ = timed(eigen, reps)
        rows.append({"d_s": int(w), "n": n, "eigen_s": round(t_me - t_mom, 6), "sweeps": int(probe._sweeps.cpu()[0]),
                     "status": int(probe._status.cpu()[0])})
        print(json.dumps(rows[-1]), file=sys.stderr, flush=True)
    return rows


def run_gmm(d, n, count, reps, baselines=True, sklearn_sample=3, C=4, iters=10):
    X, m, p = subspaces_for(d, n, count, seed=d + n + count)
    Xd = torch.as_tensor(X, device="cuda")
    S, dims = len(m), m.sum(axis=1)
    labels = np.random.default_rng(0).integers(0, C, size=n)
    ens = vgan_amd.SubspaceGMM(m, p, n_components=C, init=labels, tol=0.0, max_iter=iters)
    t_fit, tf = timed(lambda: ens.fit(Xd), reps)
    t_dec, td = timed(lambda: ens.decision_function(Xd), reps)
    ours = ens.per_subspace_scores_.astype(np.float64)
    # one iteration, call by call, on the state the start leaves (the responsibilities a range finds are the last range's)
    inner = max(reps, 5)
    ens._prepare(n, Xd.device)
    ens._em_start(Xd, torch.as_tensor(np.broadcast_to(labels, (S, n)).copy(), device="cuda"))
    ranges = range(len(ens._ranges))
    t_e, _ = timed(lambda: [ens._e_step(Xd, i) for i in ranges], inner)
    t_mom, _ = timed(lambda: [ens._moments(Xd, i) for i in ranges], inner)
    t_fac, _ = timed(lambda: [ens._factor(i) for i in ranges], inner)
    flops = 2.0 * n * C * float((dims.astype(np.float64) ** 2).sum())
    row = {"method": "gmm", "d": d, "n": n, "S_sampled": count, "S_distinct": S, "n_components": C, "em_iterations": iters,
           "d_s_min": int(dims.min()), "d_s_median": float(np.median(dims)), "d_s_max": int(dims.max()), "ranges": len(ens._ranges),
           "fit_s": round(t_fit, 6), "fit_reps_s": tf, "decision_function_s": round(t_dec, 6), "decision_function_reps_s": td,
           "estep_s": round(t_e, 6), "moments_s": round(t_mom, 6), "factor_s": round(t_fac, 6),
           "estep_full_product_tflops": round(flops / t_e / 1e12, 3), "moments_full_product_tflops": round(flops / t_mom / 1e12, 3),
           "iteration_share_estep_moments_factor": [round(t / (t_e + t_mom + t_fac), 3) for t in (t_e, t_mom, t_fac)],
           "state_bytes": int(2 * 8 * C * (dims.astype(np.int64) ** 2).sum())}
    if baselines:
        try:
            import warnings
            from sklearn.mixture import GaussianMixture
            pick = np.unique(np.linspace(0, S - 1, min(S, sklearn_sample)).astype(int))
            R = np.zeros((n, C))
            R[np.arange(n), labels] = 1.0
            nk = R.sum(axis=0) + 10.0 * np.finfo(np.float64).eps
            t_sk, worst = 0.0, 0.0
            for s in pick:
                Xs = np.ascontiguousarray(X[:, np.flatnonzero(m[s])]).astype(np.float64)
                mu = R.T @ Xs / nk[:, None]
                prec = []
                for c in range(C):
                    E = Xs - mu[c]
                    Sigma = (R[:, c] * E.T) @ E / nk[c]
                    Sigma.flat[::Xs.shape[1] + 1] += 1e-6
                    prec.append(np.linalg.inv(Sigma))
                gm = GaussianMixture(n_components=C, reg_covar=1e-6, tol=0.0, max_iter=iters, weights_init=nk / nk.sum(), means_init=mu,
                                     precisions_init=np.stack(prec))
                t0 = time.perf_counter()
                with warnings.catch_warnings():
                    warnings.simplefilter("ignore")  # ten iterations at tol = 0 do not converge, by design
                    theirs = -gm.fit(Xs).score_samples(Xs)
                t_sk += time.perf_counter() - t0
                worst = max(worst, float(np.max(np.abs(ours[s] - theirs) / np.maximum(np.abs(theirs), 1e-300))))
            scale = S / len(pick)
            row.update({"sklearn_fit_and_score_s": round(t_sk * scale, 4), "sklearn_subspaces_timed": int(len(pick)),
                        "fit_speedup_vs_sklearn": round(t_sk * scale / (t_fit + t_dec), 1), "max_rel_diff_vs_sklearn": worst})
        except ImportError:
            row["sklearn_fit_and_score_s"] = None
    return row


def host_normalized(per, proba, mode):
    """The numpy alternative to csrc/outlier_norm.hip: float64 statistics per row of per [S, n], transform, weighted sum."""
    x = per.astype(np.float64)
    if mode == "zscore":
        c, w = x.mean(axis=1), x.std(axis=1)
    elif mode == "robust":
        c = np.median(x, axis=1)
        w = np.median(np.abs(x - c[:, None]), axis=1) / 0.6744897501960817
    else:
        c = x.min(axis=1)
        w = x.max(axis=1) - c
    w[w == 0.0] = 1.0
    x -= c[:, None]
    x /= w[:, None]
    return np.asarray(proba) @ x


def run_normalize(d, n, count, mode, reps):
    from vgan_amd.outlier import COMBINATIONS, NORMALIZATIONS
    X, m, p = subspaces_for(d, n, count, seed=d + n + count)
    Xd = torch.as_tensor(X, device="cuda")
    raw = vgan_amd.SubspaceEnsemble(m, p, method="knn", n_neighbors=5)
    ens = vgan_amd.SubspaceEnsemble(m, p, method="knn", n_neighbors=5, normalize=mode)
    # the three paths differ by tens of microseconds at the small shapes: warm all of them, then time them in turn
    paths = [lambda: raw.fit(Xd), lambda: ens.fit(Xd), lambda: host_normalized(raw.fit(Xd).per_subspace_scores_, p, mode)]
    for fn in paths * 3:
        fn()
    torch.cuda.synchronize()
    times = [[], [], []]
    for _ in range(reps):
        for ts, fn in zip(times, paths):
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            ts.append(time.perf_counter() - t0)
    (t_raw, t_dev, t_host), (r_raw, r_dev, r_host) = [float(np.median(ts)) for ts in times], [[round(t, 6) for t in ts] for ts in times]
    want = host_normalized(raw.per_subspace_scores_, p, mode)
    per = torch.as_tensor(raw.per_subspace_scores_, device="cuda")
    c, w = (torch.empty(len(m), dtype=torch.float64, device="cuda") for _ in range(2))
    out = torch.empty(n, dtype=torch.float64, device="cuda")
    t_stats, _ = timed(lambda: ens.ops.outlier_score_stats(per, NORMALIZATIONS[mode], c, w), reps)
    t_comb, _ = timed(lambda: ens.ops.outlier_combine_normalized(per, c, w, ens._proba, COMBINATIONS["sum"], out), reps)
    return {"normalize": mode, "d": d, "n": n, "S_sampled": count, "S_distinct": int(len(m)), "k": 5,
            "fit_raw_s": round(t_raw, 6), "fit_raw_reps_s": r_raw, "fit_normalized_s": round(t_dev, 6), "fit_normalized_reps_s": r_dev,
            "fit_raw_plus_host_s": round(t_host, 6), "fit_raw_plus_host_reps_s": r_host,
            "device_added_s": round(t_dev - t_raw, 6), "host_added_s": round(t_host - t_raw, 6),
            "device_adds_less_than_host": bool(t_dev - t_raw < t_host - t_raw),
            "stats_launches_s": round(t_stats, 6), "combine_launch_s": round(t_comb, 6),
            "max_abs_diff_vs_host": float(np.max(np.abs(ens.decision_scores_ - want)))}


def normalize_launches(mode, reps, S=500, n=50_000):
    """The statistics and combine launches alone on a full [S, n] score matrix (approx_subspace_dist returns few distinct
    subspaces at d = 10, so the fit rows above see a small matrix), against numpy on the same matrix on the host."""
    from vgan_amd.outlier import COMBINATIONS, NORMALIZATIONS
    ops = vgan_amd.ops.default_ops()
    rng = np.random.default_rng(S + n)
    per_host = (rng.gamma(4.0, size=(S, n)) * rng.uniform(0.5, 20.0, size=(S, 1))).astype(np.float32)
    p = np.full(S, 1.0 / S)
    per, pd = torch.as_tensor(per_host, device="cuda"), torch.as_tensor(p, device="cuda")
    stats = torch.empty(2, S, dtype=torch.float64, device="cuda")
    out = torch.empty(n, dtype=torch.float64, device="cuda")
    t_stats, _ = timed(lambda: ops.outlier_score_stats(per, NORMALIZATIONS[mode], stats[0], stats[1]), max(reps, 5))
    t_comb, _ = timed(lambda: ops.outlier_combine_normalized(per, stats[0], stats[1], pd, COMBINATIONS["sum"], out), max(reps, 5))
    t0 = time.perf_counter()
    want = host_normalized(per_host, p, mode)
    t_host = time.perf_counter() - t0
    passes = {"zscore": 2, "robust": 12, "minmax": 1}[mode]
    return {"normalize": mode, "S": S, "n": n, "matrix_bytes": 4 * S * n, "stats_launches_s": round(t_stats, 6),
            "stats_passes": passes, "stats_read_GBps": round(passes * 4.0 * S * n / t_stats / 1e9, 1),
            "combine_launch_s": round(t_comb, 6), "combine_read_GBps": round(4.0 * S * n / t_comb / 1e9, 1),
            "host_numpy_s": round(t_host, 4), "max_abs_diff_vs_host": float(np.max(np.abs(out.cpu().numpy() - want)))}


OCSVM_WORKSPACE = 16 << 30


def run_ocsvm(d, n, count, reps, baselines=True, nu=0.1, sample=4):
    from vgan_amd.outlier import OCSVM_LDS_ROWS, ocsvm_chunks
    X, m, p = subspaces_for(d, n, count, seed=d + n + count)
    Xd = torch.as_tensor(X, device="cuda")
    ens = vgan_amd.SubspaceOCSVM(m, p, nu=nu, workspace_bytes=OCSVM_WORKSPACE)
    t_fit, fit_reps = timed(lambda: ens.fit(Xd), reps)
    t_dec, dec_reps = timed(lambda: ens.decision_function(Xd), reps)
    dims, iters = m.sum(axis=1), ens.n_iter_
    chunks = ocsvm_chunks(ens.plan, n, OCSVM_WORKSPACE)
    stages = {}

    def staged(name, fn):
        def wrapped(*a, **kw):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            out = fn(*a, **kw)
            torch.cuda.synchronize()
            stages[name] = stages.get(name, 0.0) + time.perf_counter() - t0
            return out
        return wrapped

    def staged_fit(storage):
        other = vgan_amd.SubspaceOCSVM(m, p, nu=nu, workspace_bytes=OCSVM_WORKSPACE)
        other.storage = storage
        for name, attr in (("kernel_matrix", "_kernel_matrix"), ("smo", "_smo"), ("scoring", "_score")):
            setattr(other, attr, staged(name, getattr(other, attr)))
        best = None
        for _ in range(max(reps, 2)):  # the first pass warms up
            stages.clear()
            other.fit(Xd)
            best = dict(stages) if best is None or stages["smo"] < best["smo"] else best
        assert np.array_equal(other.dual_coef_, ens.dual_coef_) and np.array_equal(other.decision_scores_, ens.decision_scores_)
        return {k: round(v, 5) for k, v in best.items()}

    split = staged_fit("auto")
    longest = sum(int(iters[ens.plan.order[first:first + cnt]].max()) for first, cnt, _ in chunks)  # steps on the critical path
    row = {"method": "ocsvm", "d": d, "n": n, "nu": nu, "S_sampled": count, "S_distinct": int(len(m)), "d_s_min": int(dims.min()),
           "d_s_median": float(np.median(dims)), "d_s_max": int(dims.max()), "gram_subspaces": int(ens.plan.gram.sum()),
           "chunks": len(chunks), "kernel_matrix_bytes": 4 * n * n * int(len(m)), "fit_s": round(t_fit, 5), "fit_reps_s": fit_reps,
           "decision_function_s": round(t_dec, 5), "decision_function_reps_s": dec_reps, "fit_stages_s": split,
           "kernel_matrix_TFLOPs": round(2.0 * n * n * float(dims.sum()) / split["kernel_matrix"] / 1e12, 2),
           "n_iter_min": int(iters.min()), "n_iter_median": float(np.median(iters)), "n_iter_max": int(iters.max()),
           "n_support_median": float(np.median(ens.n_support_)), "converged": bool(ens.converged_.all()),
           "smo_steps_total": int(iters.sum()), "smo_steps_on_the_critical_path": longest,
           "smo_us_per_critical_step": round(split["smo"] / max(longest, 1) * 1e6, 2)}
    row["smo_stage_s_by_storage"] = {where: staged_fit(where)["smo"]
                                     for where in (("lds",) if n <= OCSVM_LDS_ROWS else ()) + ("global", "wide")}
    if baselines:
        from sklearn.svm import OneClassSVM
        pick = np.unique(np.linspace(0, len(m) - 1, min(sample, len(m))).astype(int))
        t_host, worst, host_iters = 0.0, 0.0, []
        for s in pick:
            Z = X[:, np.flatnonzero(m[s])].astype(np.float64)
            t0 = time.perf_counter()
            ref = OneClassSVM(kernel="rbf", gamma="scale", nu=nu, tol=1e-3, shrinking=False, cache_size=4000).fit(Z)
            want = -ref.decision_function(Z)
            t_host += time.perf_counter() - t0
            host_iters.append(int(np.ravel(ref.n_iter_)[0]))
            worst = max(worst, float(np.abs(ens.per_subspace_scores_[s] - want).max()))
        row.update({"sklearn_subspaces_timed": [int(s) for s in pick], "sklearn_fit_and_score_s_scaled": round(t_host / len(pick) * len(m), 3),
                    "sklearn_n_iter": host_iters, "device_n_iter_same_subspaces": [int(iters[s]) for s in pick],
                    "max_abs_score_diff_vs_sklearn": worst, "speedup_vs_sklearn": round(t_host / len(pick) * len(m) / t_fit, 1)})
    return row


class _StagedOps:
    """The kernel provider with every call of the named entries behind a synchronisation, its time added to a stage."""

    def __init__(self, ops, names, stages):
        self._ops, self._names, self._stages = ops, names, stages

    def __getattr__(self, name):
        fn = getattr(self._ops, name)
        stage = self._names.get(name)
        if stage is None:
            return fn

        def wrapped(*a, **kw):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            out = fn(*a, **kw)
            torch.cuda.synchronize()
            self._stages[stage] = self._stages.get(stage, 0.0) + time.perf_counter() - t0
            return out
        return wrapped


KPCA_STAGES = {"ocsvm_kernel_matrix": "kernel_matrix", "kpca_center": "centring", "pca_eigen": "eigen", "kpca_kernel_rows": "kernel_rows",
               "kpca_row_means": "scores", "kpca_scores": "scores", "outlier_pack": "pack"}


def run_kpca(d, n, count, reps, baselines=True, max_samples="auto", sample=4):
    X, m, p = subspaces_for(d, n, count, seed=d + n + count)
    Xd = torch.as_tensor(X, device="cuda")
    ens = vgan_amd.SubspaceKPCA(m, p, max_samples=max_samples, workspace_bytes=OCSVM_WORKSPACE)
    t_fit, fit_reps = timed(lambda: ens.fit(Xd), reps)
    t_dec, dec_reps = timed(lambda: ens.decision_function(Xd), reps)
    dims, L = m.sum(axis=1), len(ens.landmark_rows_)
    stages = {}
    other = vgan_amd.SubspaceKPCA(m, p, max_samples=max_samples, workspace_bytes=OCSVM_WORKSPACE)
    other._attach()
    other.ops = _StagedOps(other.ops, KPCA_STAGES, stages)
    other.fit(Xd)
    assert np.array_equal(other.decision_scores_, ens.decision_scores_)
    fit_stages = {k: round(v, 5) for k, v in stages.items()}
    stages.clear()
    other.decision_function(Xd)
    dec_stages = {k: round(v, 5) for k, v in stages.items()}
    row = {"method": "kpca", "d": d, "n": n, "landmarks": L, "S_sampled": count, "S_distinct": int(len(m)), "d_s_min": int(dims.min()),
           "d_s_median": float(np.median(dims)), "d_s_max": int(dims.max()), "gram_subspaces": int(ens.plan.gram.sum()),
           "fit_s": round(t_fit, 5), "fit_reps_s": fit_reps, "decision_function_s": round(t_dec, 5), "decision_function_reps_s": dec_reps,
           "fit_stages_s": fit_stages, "decision_function_stages_s": dec_stages,
           "eigen_share_of_fit": round(fit_stages["eigen"] / sum(fit_stages.values()), 3),
           "sweeps_min": int(ens.n_sweeps_.min()), "sweeps_median": float(np.median(ens.n_sweeps_)), "sweeps_max": int(ens.n_sweeps_.max()),
           "converged": bool(ens.converged_.all()), "n_usable_median": float(np.median(ens.n_usable_)),
           "kernel_rows_TFLOPs": round(2.0 * n * L * float(dims.sum()) / dec_stages["kernel_rows"] / 1e12, 2),
           "scores_f64_TFLOPs": round(2.0 * n * L * float(ens.n_components_.sum()) / dec_stages["scores"] / 1e12, 2)}
    if baselines:
        from sklearn.decomposition import KernelPCA
        from threadpoolctl import threadpool_limits
        row["pca_fit_s"] = round(timed(lambda: vgan_amd.SubspacePCA(m, p).fit(Xd), reps)[0], 5)
        row["ocsvm_fit_s"] = round(timed(lambda: vgan_amd.SubspaceOCSVM(m, p, nu=0.1, workspace_bytes=OCSVM_WORKSPACE).fit(Xd), reps)[0], 5)
        pick = np.unique(np.linspace(0, len(m) - 1, min(sample, len(m))).astype(int))
        t_host = 0.0
        with threadpool_limits(limits=16):
            for s in pick:
                Z = X[:, np.flatnonzero(m[s])].astype(np.float64)
                t0 = time.perf_counter()
                ref = KernelPCA(kernel="rbf", gamma=float(ens.gamma_[s]), eigen_solver="dense").fit(Z[ens.landmark_rows_])
                ref.transform(Z)
                t_host += time.perf_counter() - t0
        row.update({"sklearn_subspaces_timed": [int(s) for s in pick], "sklearn_threads": 16,
                    "sklearn_fit_and_transform_s_scaled": round(t_host / len(pick) * len(m), 3),
                    "speedup_vs_sklearn": round(t_host / len(pick) * len(m) / (t_fit + t_dec), 1)})
    return row


def numpy_sos_one(Xs, perplexity, tol=1e-5, max_iter=200, threads=16, block=256):
    """(scores float64 [n], steps per row, seconds of matrix / search / scores): SubspaceSOS's rules for one subspace in numpy,
    float64 throughout, blocks of rows spread over a pool of `threads` threads (numpy's exp and sums release the GIL)."""
    from concurrent.futures import ThreadPoolExecutor
    n = Xs.shape[0]
    t0 = time.perf_counter()
    sq = (Xs * Xs).sum(axis=1)
    Dm = np.sqrt(np.maximum(sq[:, None] + sq[None, :] - 2.0 * (Xs @ Xs.T), 0.0))
    np.fill_diagonal(Dm, np.inf)
    t1 = time.perf_counter()
    log_perplexity = np.log(perplexity)
    beta, dmin, Z, steps = np.ones(n), Dm.min(axis=1), np.empty(n), np.zeros(n, np.int64)

    def search(lo_row):
        rows = slice(lo_row, min(n, lo_row + block))
        E = Dm[rows] - dmin[rows, None]
        m = (E == 0.0).sum(axis=1)
        b, lo, hi = beta[rows].copy(), np.zeros(E.shape[0]), np.full(E.shape[0], np.inf)
        z, it = m.astype(np.float64), np.zeros(E.shape[0], np.int64)
        b[m >= perplexity] = np.inf
        act = np.flatnonzero(m < perplexity)
        while act.size:
            e = E[act]
            a = np.exp(-(b[act, None] * e))
            zz = a.sum(axis=1)
            with np.errstate(invalid="ignore"):
                ss = np.where(a > 0.0, e * a, 0.0).sum(axis=1)  # the row's own entry: inf times 0
            diff = (np.log(zz) + b[act] * (ss / zz)) - log_perplexity
            z[act] = zz
            go = (np.abs(diff) > tol) & (it[act] < max_iter)
            act, up, bb = act[go], diff[go] > 0.0, b[act][go]
            lo_old, hi_old = lo[act], hi[act]
            lo[act], hi[act] = np.where(up, bb, lo_old), np.where(up, hi_old, bb)
            b[act] = np.where(up, np.where(np.isinf(hi_old), 2.0 * bb, (bb + hi_old) / 2.0), (bb + lo_old) / 2.0)
            it[act] += 1
        beta[rows], Z[rows], steps[rows] = b, z, it + (m < perplexity)

    with ThreadPoolExecutor(threads) as pool:
        list(pool.map(search, range(0, n, block)))
        t2 = time.perf_counter()
        deg = np.isinf(beta)
        total = np.zeros(n)

        def terms(lo_row):  # fitted rows lo_row ..: their terms for every scored row
            rows = slice(lo_row, min(n, lo_row + block))
            E = Dm[rows] - dmin[rows, None]
            with np.errstate(invalid="ignore", divide="ignore"):
                a = np.where(deg[rows, None], (E <= 0.0).astype(np.float64), np.exp(-(np.where(deg[rows], 0.0, beta[rows])[:, None] * E)))
                return np.minimum(-np.log1p(-np.minimum(a / Z[rows, None], 1.0)), 128.0).sum(axis=0)

        for part in pool.map(terms, range(0, n, block)):
            total += part
    return np.exp(-total), steps, (t1 - t0, t2 - t1, time.perf_counter() - t2)


def run_sos(d, n, count, reps, baselines=True, perplexity=30.0, sample=2):
    from vgan_amd.outlier import SOS_WAVE_ROWS, sos_chunks
    X, m, p = subspaces_for(d, n, count, seed=d + n + count)
    Xd = torch.as_tensor(X, device="cuda")
    ens = vgan_amd.SubspaceSOS(m, p, perplexity=perplexity, workspace_bytes=OCSVM_WORKSPACE)
    t_fit, fit_reps = timed(lambda: ens.fit(Xd), reps)
    t_dec, dec_reps = timed(lambda: ens.decision_function(Xd), reps)
    dims = m.sum(axis=1)
    stages = {}

    def staged(name, fn):
        def wrapped(*a, **kw):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            out = fn(*a, **kw)
            torch.cuda.synchronize()
            stages[name] = stages.get(name, 0.0) + time.perf_counter() - t0
            return out
        return wrapped

    def staged_fit(storage):
        other = vgan_amd.SubspaceSOS(m, p, perplexity=perplexity, workspace_bytes=OCSVM_WORKSPACE)
        other.storage = storage
        for name, attr in (("matrix", "_distance_matrix"), ("search", "_search"), ("scores", "_score_fitted")):
            setattr(other, attr, staged(name, getattr(other, attr)))
        best = None
        for _ in range(max(reps, 2)):  # the first pass warms up
            stages.clear()
            other.fit(Xd)
            best = dict(stages) if best is None or stages["search"] < best["search"] else best
        assert np.array_equal(other.beta_, ens.beta_) and np.array_equal(other.decision_scores_, ens.decision_scores_)
        return {k: round(v, 5) for k, v in best.items()}

    split = staged_fit("auto")
    searched = np.isfinite(ens.beta_)
    evaluations = float((ens.n_iter_[searched] + 1).sum())  # an evaluation of the entropy per update, and the one that stops
    row = {"method": "sos", "d": d, "n": n, "perplexity": perplexity, "S_sampled": count, "S_distinct": int(len(m)),
           "d_s_min": int(dims.min()), "d_s_median": float(np.median(dims)), "d_s_max": int(dims.max()),
           "gram_subspaces": int(ens.plan.gram.sum()), "chunks": len(sos_chunks(ens.plan, n, OCSVM_WORKSPACE)),
           "distance_matrix_bytes": 4 * n * n * int(len(m)), "fit_s": round(t_fit, 5), "fit_reps_s": fit_reps,
           "decision_function_s": round(t_dec, 5), "decision_function_reps_s": dec_reps, "fit_stages_s": split,
           "matrix_TFLOPs": round(2.0 * n * n * float(dims.sum()) / split["matrix"] / 1e12, 2),
           "search_steps_per_row_mean": round(evaluations / max(int(searched.sum()), 1), 2),
           "search_steps_per_row_max": int(ens.n_iter_.max()) + 1, "n_degenerate": int(ens.n_degenerate_.sum()),
           "n_unconverged": int(ens.n_unconverged_.sum()),
           "search_f64_exp_per_s": round(evaluations * (n - 1) / split["search"], 0),
           "scores_f64_exp_per_s": round(float(len(m)) * n * (n - 1) / split["scores"], 0)}
    row["search_stage_s_by_storage"] = {where: staged_fit(where)["search"] for where in (("wave",) if n <= SOS_WAVE_ROWS else ()) + ("block",)}
    lof = vgan_amd.SubspaceEnsemble(m, p, method="lof", n_neighbors=20)
    row["lof_k20_fit_s"], row["lof_k20_fit_reps_s"] = timed(lambda: lof.fit(Xd), reps)
    row["lof_k20_fit_s"] = round(row["lof_k20_fit_s"], 5)
    if baselines:
        pick = np.unique(np.linspace(0, len(m) - 1, min(sample, len(m))).astype(int))
        host, worst, host_steps = np.zeros(3), 0.0, 0.0
        for s in pick:
            scores, steps, times = numpy_sos_one(X[:, np.flatnonzero(m[s])].astype(np.float64), perplexity)
            host += times
            host_steps += float(steps.sum())
            worst = max(worst, float(np.abs(ens.per_subspace_scores_[s] - scores).max()))
        scale = len(m) / len(pick)
        row.update({"numpy16_subspaces_timed": [int(s) for s in pick],
                    "numpy16_stages_s_scaled": {k: round(float(v) * scale, 3) for k, v in zip(("matrix", "search", "scores"), host)},
                    "numpy16_fit_s_scaled": round(float(host.sum()) * scale, 3),
                    "numpy16_search_f64_exp_per_s": round(host_steps * (n - 1) / host[1], 0),
                    "max_abs_score_diff_vs_numpy": worst, "speedup_vs_numpy16": round(float(host.sum()) * scale / t_fit, 1),
                    "search_speedup_vs_numpy16": round(float(host[1]) * scale / split["search"], 1)})
    return row


VALU_LANE_OPS_PER_S = 256 * 4 * 32 * 2.4e9  # CUs x SIMDs x lanes a clock x clock: the fp32 vector rate of 157.3 TFLOPS in FMAs
LOCI_SUMS_OPS_PER_PAIR_RADIUS = 6.6  # vector instructions of the sums sweep's inner loop per (pair, radius), counted in its ISA


def numpy_loci_one(Xs, n_radii=32, radii_per_octave=4.0, alpha=0.5, n_min=20, threads=16, block=256):
    """(scores float32 [n], seconds of matrix / counts / sums / finish): SubspaceLOCI's rules for one subspace in numpy, the
    matrix float32 from float64 squared distances, blocks of subject rows spread over a pool of `threads` threads."""
    from concurrent.futures import ThreadPoolExecutor
    from vgan_amd.outlier import loci_radii
    n = Xs.shape[0]
    t0 = time.perf_counter()
    sq = (Xs * Xs).sum(axis=1)
    Dm = np.sqrt(np.maximum(sq[:, None] + sq[None, :] - 2.0 * (Xs @ Xs.T), 0.0)).astype(np.float32)
    np.fill_diagonal(Dm, 0.0)
    r, a = loci_radii(Dm.max(), n_radii, radii_per_octave, alpha)
    t1 = time.perf_counter()
    cnt = np.empty((n, n_radii), np.int64)
    m, S1, S2 = (np.empty((n, n_radii), np.int64) for _ in range(3))

    def counts(lo):
        blk = Dm[:, lo:lo + block]
        for j in range(n_radii):
            cnt[lo:lo + block, j] = (blk <= a[j]).sum(axis=0)

    def sums(lo):
        blk = Dm[:, lo:lo + block]
        for j in range(n_radii):
            inside = (blk <= r[j]).astype(np.float64)  # sums below 2^53: exact in float64
            m[lo:lo + block, j] = inside.sum(axis=0)
            S1[lo:lo + block, j] = cf[:, j] @ inside
            S2[lo:lo + block, j] = cf2[:, j] @ inside

    with ThreadPoolExecutor(threads) as pool:
        list(pool.map(counts, range(0, n, block)))
        t2 = time.perf_counter()
        cf = cnt.astype(np.float64)
        cf2 = cf * cf
        list(pool.map(sums, range(0, n, block)))
    t3 = time.perf_counter()
    num, den = S1 - cnt * m, m * S2 - S1 * S1
    with np.errstate(divide="ignore", invalid="ignore"):
        ratio = np.where((m >= n_min) & (den > 0), num / np.sqrt(den.astype(np.float64)), -np.inf)
    scores = np.maximum(ratio.max(axis=1), 0.0).astype(np.float32)
    return scores, (t1 - t0, t2 - t1, t3 - t2, time.perf_counter() - t3)


def run_loci(d, n, count, reps, baselines=True, sample=2):
    from vgan_amd.outlier import loci_chunks
    X, m, p = subspaces_for(d, n, count, seed=d + n + count)
    Xd = torch.as_tensor(X, device="cuda")
    ens = vgan_amd.SubspaceLOCI(m, p, workspace_bytes=OCSVM_WORKSPACE)
    t_fit, fit_reps = timed(lambda: ens.fit(Xd), reps)
    t_dec, dec_reps = timed(lambda: ens.decision_function(Xd), reps)
    dims, R = m.sum(axis=1), ens.n_radii
    stages = {}

    def staged(name, fn):
        def wrapped(*a, **kw):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            out = fn(*a, **kw)
            torch.cuda.synchronize()
            stages[name] = stages.get(name, 0.0) + time.perf_counter() - t0
            return out
        return wrapped

    other = vgan_amd.SubspaceLOCI(m, p, workspace_bytes=OCSVM_WORKSPACE)
    for name, attr in (("matrix", "_distance_matrix"), ("radii", "_set_radii"), ("counts", "_counts"), ("sums", "_sums"),
                       ("finish", "_finish")):
        setattr(other, attr, staged(name, getattr(other, attr)))
    split = None
    for _ in range(max(reps, 2)):  # the first pass warms up
        stages.clear()
        other.fit(Xd)
        split = dict(stages) if split is None or stages["sums"] < split["sums"] else split
    assert np.array_equal(other.decision_scores_, ens.decision_scores_) and np.array_equal(other.best_radius_, ens.best_radius_)
    split = {k: round(v, 5) for k, v in split.items()}
    pair_radii = float(len(m)) * n * n * R
    rate = pair_radii / split["sums"]
    row = {"method": "loci", "d": d, "n": n, "n_radii": R, "radii_per_octave": ens.radii_per_octave, "alpha": ens.alpha,
           "n_min": ens.n_min, "S_sampled": count, "S_distinct": int(len(m)), "d_s_min": int(dims.min()),
           "d_s_median": float(np.median(dims)), "d_s_max": int(dims.max()), "gram_subspaces": int(ens.plan.gram.sum()),
           "chunks": len(loci_chunks(ens.plan, n, R, OCSVM_WORKSPACE)), "distance_matrix_bytes": 4 * n * n * int(len(m)),
           "fit_s": round(t_fit, 5), "fit_reps_s": fit_reps, "decision_function_s": round(t_dec, 5),
           "decision_function_reps_s": dec_reps, "fit_stages_s": split,
           "matrix_TFLOPs": round(2.0 * n * n * float(dims.sum()) / split["matrix"] / 1e12, 2),
           "counts_pair_radii_per_s": round(pair_radii / split["counts"], 0), "sums_pair_radii_per_s": round(rate, 0),
           "sums_vector_ops_per_pair_radius": LOCI_SUMS_OPS_PER_PAIR_RADIUS,
           "sums_share_of_vector_alu_rate": round(rate * LOCI_SUMS_OPS_PER_PAIR_RADIUS / VALU_LANE_OPS_PER_S, 3),
           "n_flagged_mean": float(ens.n_flagged_.mean())}
    sos = vgan_amd.SubspaceSOS(m, p, perplexity=30.0, workspace_bytes=OCSVM_WORKSPACE)
    row["sos_fit_s"], row["sos_fit_reps_s"] = timed(lambda: sos.fit(Xd), reps)
    row["sos_fit_s"] = round(row["sos_fit_s"], 5)
    lof = vgan_amd.SubspaceEnsemble(m, p, method="lof", n_neighbors=20)
    row["lof_k20_fit_s"], row["lof_k20_fit_reps_s"] = timed(lambda: lof.fit(Xd), reps)
    row["lof_k20_fit_s"] = round(row["lof_k20_fit_s"], 5)
    if baselines:
        pick = np.unique(np.linspace(0, len(m) - 1, min(sample, len(m))).astype(int))
        host, worst = np.zeros(4), 0.0
        for s in pick:
            scores, times = numpy_loci_one(X[:, np.flatnonzero(m[s])].astype(np.float64), R, ens.radii_per_octave, ens.alpha, ens.n_min)
            host += times
            worst = max(worst, float(np.abs(ens.per_subspace_scores_[s] - scores).max()))
        scale = len(m) / len(pick)
        row.update({"numpy16_subspaces_timed": [int(s) for s in pick],
                    "numpy16_stages_s_scaled": {k: round(float(v) * scale, 3) for k, v in zip(("matrix", "counts", "sums", "finish"), host)},
                    "numpy16_fit_s_scaled": round(float(host.sum()) * scale, 3),
                    "max_abs_score_diff_vs_numpy": worst, "speedup_vs_numpy16": round(float(host.sum()) * scale / t_fit, 1)})
    return row


def sweep(n, reps):
    rng = np.random.default_rng(0)
    rows = []
    for ds in [4, 8, 16, 24, 32, 48, 64, 128]:
        d = max(ds, 128)
        X = torch.as_tensor(rng.normal(size=(n, d)).astype(np.float32), device="cuda")
        m = np.zeros((16, d), bool)
        for s in range(16):
            m[s, rng.choice(d, ds, replace=False)] = True
        row = {"d_s": ds, "n": n, "S": 16, "k": 5}
        for engine in ["exact", "gram"]:
            ens = vgan_amd.SubspaceEnsemble(m, np.full(16, 1 / 16), n_neighbors=5, engine=engine)
            t, _ = timed(lambda: ens.fit(X), reps)
            row[f"{engine}_s"] = round(t, 5)
        rows.append(row)
    return rows


def numpy_inne_one(Xs, rows, Q, threads=16):
    """The restatement of SubspaceINNE for one subspace (Xs: its columns of X; rows int [T, psi]: the centres the device drew;
    Q: the query rows): float64, a loop over the features, the estimators dealt to `threads` threads.  (seconds of the build,
    seconds of the scores, the scores [len(Q)])."""
    from concurrent.futures import ThreadPoolExecutor
    T, psi = rows.shape
    eps = 2.0 ** -52

    def d2(A, B):
        acc = np.zeros((A.shape[0], B.shape[0]))
        diff = np.empty_like(acc)
        for f in range(A.shape[1]):
            np.subtract(A[:, None, f], B[None, :, f], out=diff)
            np.multiply(diff, diff, out=diff)
            np.add(acc, diff, out=acc)
        return acc

    def build(t):
        C = Xs[rows[t]].astype(np.float64)
        D = d2(C, C)
        D[np.arange(psi), np.arange(psi)] = np.inf
        nn = D.argmin(axis=1)
        r2 = D[np.arange(psi), nn]
        return C, r2, 1.0 - (r2[nn] + eps) / (r2 + eps)

    def score(t):
        C, r2, rho = spheres[t]
        covered = d2(Q64, C) <= r2[None, :]
        at = np.where(covered, r2[None, :], np.inf).argmin(axis=1)
        return np.where(covered.any(axis=1), rho[at], 1.0)

    Q64 = Q.astype(np.float64)
    with ThreadPoolExecutor(threads) as pool:
        t0 = time.perf_counter()
        spheres = list(pool.map(build, range(T)))
        t1 = time.perf_counter()
        iso = list(pool.map(score, range(T)))
        t2 = time.perf_counter()
    total = np.zeros(len(Q))
    for v in iso:
        total = total + v
    return t1 - t0, t2 - t1, total / float(T)


def run_inne(d, n, count, reps, baselines=True, numpy_sample=2, numpy_rows=2000):
    X, m, p = subspaces_for(d, n, count, seed=d + n + count)
    Xd = torch.as_tensor(X, device="cuda")
    S, dims = len(m), m.sum(axis=1)
    ens = vgan_amd.SubspaceINNE(m, p)
    t_fit, tf = timed(lambda: ens.fit(Xd), reps)
    t_dec, td = timed(lambda: ens.decision_function(Xd), reps)
    ops, inner = ens.ops, max(reps, 5)
    T, psi = ens.n_estimators, ens.max_samples_
    state = tuple(torch.empty_like(a) for a in ens._state)
    per = torch.empty(S, n, dtype=torch.float32, device="cuda")
    ratio = vgan_amd.outlier.INNE_RATIOS[ens.ratio]
    t_build, _ = timed(lambda: ops.inne_build(ens._X, ens._table, 0, S, int(dims.max()), ratio, ens.seed, state), inner)
    t_scores, _ = timed(lambda: ops.inne_scores(ens._X, ens._X, ens._table, 0, S, int(dims.max()), ens._state, per), inner)
    pair_features = float(n) * T * psi * float(dims.sum())  # (row, centre, feature) triples of one scoring pass
    row = {"method": "inne", "d": d, "n": n, "S_sampled": count, "S_distinct": S, "n_estimators": T, "max_samples": psi, "ratio": ens.ratio,
           "d_s_min": int(dims.min()), "d_s_median": float(np.median(dims)), "d_s_max": int(dims.max()),
           "fit_s": round(t_fit, 6), "fit_reps_s": tf, "decision_function_s": round(t_dec, 6), "decision_function_reps_s": td,
           "build_s": round(t_build, 6), "scores_s": round(t_scores, 6), "state_bytes": int(S * T * psi * vgan_amd.outlier.INNE_STATE_BYTES),
           "scores_fp64_tflops": round(3.0 * pair_features / t_scores / 1e12, 3),
           "scores_fp64_note": "three float64 operations per (row, centre, feature)"}
    knn = vgan_amd.SubspaceEnsemble(m, p, method="knn", n_neighbors=5)
    t_knn, tk = timed(lambda: knn.fit(Xd), reps)
    row.update({"knn_fit_s": round(t_knn, 5), "knn_fit_reps_s": tk, "knn_over_inne_fit": round(t_knn / t_fit, 2)})
    if baselines:
        pick = np.unique(np.linspace(0, S - 1, min(S, numpy_sample)).astype(int))
        nq = min(n, numpy_rows)
        t_np_build = t_np_scores = 0.0
        equal = True
        for s in pick:
            Xs = np.ascontiguousarray(X[:, np.flatnonzero(m[s])])
            tb, ts, host = numpy_inne_one(Xs, ens.center_rows_[s].astype(np.int64), Xs[:nq])
            t_np_build, t_np_scores = t_np_build + tb, t_np_scores + ts * n / nq
            equal = equal and bool(np.array_equal(host.astype(np.float32), ens.per_subspace_scores_[s, :nq]))
        scale = S / len(pick)
        row.update({"numpy_16_threads_build_s": round(t_np_build * scale, 4), "numpy_16_threads_scores_s": round(t_np_scores * scale, 4),
                    "numpy_16_threads_fit_s": round((t_np_build + t_np_scores) * scale, 4), "numpy_subspaces_timed": int(len(pick)),
                    "numpy_rows_timed": int(nq), "fit_speedup_vs_numpy": round((t_np_build + t_np_scores) * scale / t_fit, 1),
                    "scores_bit_equal_to_numpy": equal})
    return row


def run_inne_gather(n, width, S, reps, d=784):
    """The scoring pass over S subspaces of `width` features each of a d-wide matrix, the features scattered over the columns
    (what the subspaces look like) against one run of neighbouring columns (what a packed copy would offer, up to the row
    stride): whether gathering Xq[row, feat[f]] as given costs anything."""
    rng = np.random.default_rng(n + width + S)
    X = torch.as_tensor(rng.normal(size=(n, d)).astype(np.float32), device="cuda")
    out = {"n": n, "d": d, "d_s": width, "S": S}
    for name in ("scattered", "neighbouring"):
        m = np.zeros((S, d), bool)
        for s in range(S):
            cols = np.sort(rng.choice(d, width, replace=False)) if name == "scattered" else np.arange(width) + (s * 7) % (d - width)
            m[s, cols] = True
        ens = vgan_amd.SubspaceINNE(m, np.full(S, 1.0 / S)).fit(X)
        per = torch.empty(S, n, dtype=torch.float32, device="cuda")
        t, ts = timed(lambda: ens.ops.inne_scores(ens._X, ens._X, ens._table, 0, S, width, ens._state, per), max(reps, 5))
        out[name + "_scores_s"], out[name + "_scores_reps_s"] = round(t, 6), ts
    out["scattered_over_neighbouring"] = round(out["scattered_scores_s"] / out["neighbouring_scores_s"], 3)
    return out


def dif_stage_times(ens, Xd):
    """Seconds of one pass over all blocks as fit makes it, per call, each behind a synchronisation."""
    from vgan_amd.outlier import dif_chunks
    n, q, r = Xd.shape[0], ens.representation_dim, ens.n_representations
    blocks, _ = dif_chunks(ens._weight_bytes, q, n, ens.workspace_bytes, whole_rows=True)
    n_blocks = ens.plan.count * r
    blocks = min(blocks, n_blocks)
    W = torch.empty(blocks * (ens._weight_bytes // 4), dtype=torch.float32, device="cuda")
    R = torch.empty(blocks * n * q, dtype=torch.float32, device="cuda")
    sums = torch.empty(blocks * n, dtype=torch.int64, device="cuda")
    trees = torch.empty_like(ens._flat_trees)
    t = {"weights_s": 0.0, "represent_s": 0.0, "build_s": 0.0, "walk_s": 0.0}

    def lap(name, fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        t[name] += time.perf_counter() - t0

    for first in range(0, n_blocks, blocks):
        count = min(blocks, n_blocks - first)
        box = {}
        lap("weights_s", lambda: box.update(w=ens._weights(first, count, W)))
        w_off = box["w"][1]
        Rc = R[:count * n * q].view(count, n, q)
        lap("represent_s", lambda: ens.ops.dif_represent(Xd, ens._table, ens._lo, ens._hi, ens._net, first, count, W, w_off, Rc))
        lap("build_s", lambda: ens.ops.iforest_build_blocks(Rc, first, ens.max_samples_, ens.depth_limit_, ens.seed, trees))
        lap("walk_s", lambda: ens.ops.iforest_path_sums_blocks(Rc, trees, first, ens.max_samples_, ens.depth_limit_, ens._cq, sums))
    return {k: round(v, 6) for k, v in t.items()}, blocks


def dif_unfused(ens, Xd, pick):
    """(seconds, largest |difference| to the fused R) of the representations of the subspaces `pick` through one grouped-GEMM
    launch per block and layer with torch.tanh between them, on a scaled and gathered copy of the subspace."""
    r, q, n = ens.n_representations, ens.representation_dim, Xd.shape[0]
    widths = ens.hidden + (q,)
    worst, total = 0.0, 0.0
    for s in pick:
        cols = torch.as_tensor(ens.plan.feat[ens.plan.feat_off[s]:ens.plan.feat_off[s + 1]].astype(np.int64), device="cuda")
        d_s = int(cols.numel())
        flat, _ = ens._weights(s * r, r)
        size, mats = flat.numel() // r, []
        for j in range(r):  # the library keeps a layer quad-major for its own forward: row-major copies for the grouped products
            at, k = j * size, d_s
            for w in widths:
                ld = (k + 7) // 8 * 8
                mats.append(flat[at:at + w * ld].view(ld // 4, w, 4).permute(1, 0, 2).reshape(w, ld).contiguous())
                at, k = at + w * ld, w
        acts = [torch.empty(n, w, dtype=torch.float32, device="cuda") for w in widths]

        def run():
            lo, hi = ens._lo[cols].double(), ens._hi[cols].double()
            Z = torch.where(hi == lo, torch.zeros((), dtype=torch.float64, device="cuda"), (Xd[:, cols].double() - lo) / (hi - lo)).float()
            for j in range(r):
                k, h = d_s, Z
                for layer, w in enumerate(widths):
                    ens.ops.gemm_grouped([("NT", h, mats[j * len(widths) + layer][:, :k], acts[layer])])
                    if layer + 1 < len(widths):
                        torch.tanh_(acts[layer]) if ens.activation == "tanh" else torch.relu_(acts[layer])
                    k, h = w, acts[layer]

        t, _ = timed(run, 3)
        total += t
        fused = torch.as_tensor(ens.representation(Xd, s, r - 1), device="cuda")
        worst = max(worst, float((fused - acts[-1]).abs().max()))
    return total, worst


def dif_host(X, ens, pick, rows, threads=16):
    """Seconds of numpy (float32 products, tanh) and sklearn's IsolationForest per block on the host for the subspaces `pick` and
    the first `rows` rows: (representation, trees and scores)."""
    from sklearn.ensemble import IsolationForest
    r = ens.n_representations
    t_rep = t_forest = 0.0
    lo, hi = ens.feature_min_.astype(np.float64), ens.feature_max_.astype(np.float64)
    for s in pick:
        cols = ens.plan.feat[ens.plan.feat_off[s]:ens.plan.feat_off[s + 1]]
        weights = [ens.layer_weights(s, j) for j in range(r)]
        t0 = time.perf_counter()
        with np.errstate(divide="ignore", invalid="ignore"):
            Z = np.where(hi[cols] == lo[cols], 0.0, (X[:rows, cols].astype(np.float64) - lo[cols]) / (hi[cols] - lo[cols])).astype(np.float32)
        reps = []
        for j in range(r):
            h = Z
            for layer, w in enumerate(weights[j]):
                h = h @ w.T
                if layer + 1 < len(weights[j]):
                    h = np.tanh(h) if ens.activation == "tanh" else np.maximum(h, 0)
            reps.append(h)
        t1 = time.perf_counter()
        for h in reps:
            forest = IsolationForest(n_estimators=ens.n_estimators, max_samples=min(256, rows), n_jobs=threads, random_state=0).fit(h)
            forest.score_samples(h)
        t_rep, t_forest = t_rep + t1 - t0, t_forest + time.perf_counter() - t1
    return t_rep, t_forest


def run_dif(d, n, count, reps, baselines=True, sample=2, host_rows=2000):
    X, m, p = subspaces_for(d, n, count, seed=d + n + count)
    Xd = torch.as_tensor(X, device="cuda")
    S, dims = len(m), m.sum(axis=1)
    ens = vgan_amd.SubspaceDIF(m, p)
    t_fit, tf = timed(lambda: ens.fit(Xd), reps)
    t_dec, td = timed(lambda: ens.decision_function(Xd), reps)
    r, T, q = ens.n_representations, ens.n_estimators, ens.representation_dim
    widths = (0,) + ens.hidden + (q,)
    inner = sum(a * b for a, b in zip(widths[1:-1], widths[2:]))
    flop = 2.0 * n * r * float((dims * widths[1] + inner).sum())
    stages, blocks = dif_stage_times(ens, Xd)
    row = {"method": "dif", "d": d, "n": n, "S_sampled": count, "S_distinct": S, "n_representations": r, "n_estimators": T,
           "max_samples": ens.max_samples_, "hidden": list(ens.hidden), "representation_dim": q, "activation": ens.activation,
           "d_s_min": int(dims.min()), "d_s_median": float(np.median(dims)), "d_s_max": int(dims.max()),
           "fit_s": round(t_fit, 6), "fit_reps_s": tf, "decision_function_s": round(t_dec, 6), "decision_function_reps_s": td,
           "blocks_per_chunk": blocks, **stages, "represent_flop": flop,
           "represent_fp32_tflops": round(flop / stages["represent_s"] / 1e12, 2),
           "represent_fraction_of_fp32_matrix_peak": round(flop / stages["represent_s"] / FP32_PEAK, 4),
           "state_bytes": int(ens._trees.numel() * 4 + 2 * 4 * d)}
    forest = vgan_amd.SubspaceIForest(m, p, n_estimators=min(r * T, 1024))
    t_if, ti = timed(lambda: forest.fit(Xd), reps)
    row.update({"iforest_trees": forest.n_estimators, "iforest_fit_s": round(t_if, 6), "iforest_fit_reps_s": ti,
                "dif_over_iforest_fit": round(t_fit / t_if, 2)})
    if baselines:
        pick = np.unique(np.linspace(0, S - 1, min(S, sample)).astype(int))
        share = float((dims[pick] * widths[1] + inner).sum()) / float((dims * widths[1] + inner).sum())  # of the flop
        t_un, diff = dif_unfused(ens, Xd, pick)
        nq = min(n, host_rows)
        t_rep, t_forest = dif_host(X, ens, pick, nq)
        row.update({"unfused_subspaces_timed": int(len(pick)), "unfused_represent_s": round(t_un / share, 6),
                    "unfused_over_fused_represent": round(t_un / share / stages["represent_s"], 2),
                    "unfused_largest_abs_difference": diff,
                    "host_subspaces_timed": int(len(pick)), "host_rows_timed": int(nq),
                    "numpy_16_threads_represent_s": round(t_rep / share * n / nq, 3),
                    "sklearn_16_threads_trees_s": round(t_forest * S / len(pick) * n / nq, 3),
                    "fit_speedup_vs_host": round((t_rep / share + t_forest * S / len(pick)) * n / nq / t_fit, 1)})
    return row


def numpy_rshash_component(X, rows, cols, alpha, f, table, fitting):
    """int64 [n]: table[c] of every row of X for one component, by the rules of SubspaceRSHash in plain numpy."""
    sub = X[:, cols].astype(np.float64)
    mn, mx = sub[rows].min(axis=0), sub[rows].max(axis=0)
    w = mx - mn
    with np.errstate(divide="ignore", invalid="ignore"):
        t = np.where(w > 0, (sub - mn) / w, 0.0)
    y = np.clip(np.floor((t + alpha) / f), -1.0, np.floor(1.0 / f) + 2.0).astype(np.int64) + 1
    R = int(np.floor(1.0 / f)) + 4
    key = (y * R ** np.arange(len(cols), dtype=np.int64)).sum(axis=1)
    keys, counts = np.unique(key[rows], return_counts=True)
    at = np.minimum(np.searchsorted(keys, key), len(keys) - 1)
    c = np.where(keys[at] == key, counts[at], 0) + 1
    if fitting:
        c[rows] -= 1
    return table[c]


def rshash_host(X, ens, samples, pick):
    """(seconds of the numpy fit sums of the subspaces `pick` on 16 threads, whether they equal the device's)."""
    from multiprocessing.pool import ThreadPool
    table = ens._log_table.cpu().numpy()
    equal = True
    with ThreadPool(16) as pool:
        t0 = time.perf_counter()
        for z in pick:
            jobs = [(X, samples[z, t], ens.component_features_[z, t, :r], ens.component_shift_[z, t, :r], ens.grid_width_[z, t], table, True)
                    for t, r in enumerate(ens.component_dims_[z]) if r > 0]
            total = sum(pool.starmap(numpy_rshash_component, jobs)) if jobs else np.full(X.shape[0], ens._denom)
            equal = equal and bool(np.array_equal(total, ens.cell_sums_[z]))
        return time.perf_counter() - t0, equal


def run_rshash(d, n, count, reps, baselines=True, sample=2):
    from vgan_amd.outlier import rshash_components
    X, m, p = subspaces_for(d, n, count, seed=d + n + count)
    Xd = torch.as_tensor(X, device="cuda")
    S, dims = len(m), m.sum(axis=1)
    ens = vgan_amd.SubspaceRSHash(m, p)
    t_fit, tf = timed(lambda: ens.fit(Xd), reps)  # warm: a refit keeps the host draws
    t_first, tff = timed(lambda: vgan_amd.SubspaceRSHash(m, p).fit(Xd), reps)  # a new detector draws its components first
    t_dec, td = timed(lambda: ens.decision_function(Xd), reps)
    ops, inner = ens.ops, max(reps, 5)
    T, s = ens.n_estimators, ens.max_samples_
    state = tuple(torch.empty_like(a) for a in ens._state)
    samples = torch.empty(S, T, s, dtype=torch.int32, device="cuda")
    sums = torch.empty(S * n, dtype=torch.int64, device="cuda")
    per = torch.empty(S, n, dtype=torch.float32, device="cuda")
    keys = torch.empty(d, 2, dtype=torch.int64, device="cuda")
    t_range, _ = timed(lambda: (ops.hist_column_range(Xd, keys), keys.cpu()), inner)
    t0 = time.perf_counter()
    rshash_components([len(c) for c in ens.candidate_features_], T, s, ens.seed)
    t_draw = time.perf_counter() - t0
    t_build, _ = timed(lambda: ops.rshash_build(Xd, 0, S, ens.seed, ens._comp, state, samples), inner)
    for a, b in zip(state, ens._state):
        assert torch.equal(a, b)
    t_sums, _ = timed(lambda: ops.rshash_cell_sums(Xd, False, 0, 0, S, ens._comp, ens._state, samples, ens._log_table, sums), inner)
    assert np.array_equal(sums.view(S, n).cpu().numpy(), ens.cell_sums_)
    t_new, _ = timed(lambda: ops.rshash_cell_sums(Xd, False, 0, 0, S, ens._comp, ens._state, None, ens._log_table, sums), inner)
    row_major = sums.clone()
    t_copy, _ = timed(lambda: Xd.t().contiguous(), inner)
    Xt = Xd.t().contiguous()
    t_col, _ = timed(lambda: ops.rshash_cell_sums(Xt, True, 0, 0, S, ens._comp, ens._state, None, ens._log_table, sums), inner)
    assert torch.equal(sums, row_major)
    t_scores, _ = timed(lambda: ops.rshash_scores(sums, S, n, ens._denom, per), inner)
    live = int((ens.component_dims_ > 0).sum())
    row = {"method": "rshash", "d": d, "n": n, "S_sampled": count, "S_distinct": S, "n_estimators": T, "max_samples": s,
           "d_s_min": int(dims.min()), "d_s_median": float(np.median(dims)), "d_s_max": int(dims.max()),
           "candidates_median": float(np.median([len(c) for c in ens.candidate_features_])),
           "r_mean": round(float(ens.component_dims_[ens.component_dims_ > 0].mean()), 2),
           "cells_mean": round(float(ens.n_cells_[ens.component_dims_ > 0].mean()), 1),
           "fit_s": round(t_first, 6), "fit_reps_s": tff, "refit_s": round(t_fit, 6), "refit_reps_s": tf,
           "decision_function_s": round(t_dec, 6), "decision_function_reps_s": td,
           "range_pass_and_copy_s": round(t_range, 6), "draws_host_s": round(t_draw, 6), "build_s": round(t_build, 6),
           "cell_sums_fit_s": round(t_sums, 6), "cell_sums_new_rows_s": round(t_new, 6), "scores_s": round(t_scores, 6),
           "pairs_per_s_fit": round(live * float(n) / t_sums / 1e9, 2), "pairs_per_s_new_rows": round(live * float(n) / t_new / 1e9, 2),
           "pairs_unit": "1e9 (row, component) pairs / s",
           "x_row_major_through_l2_s": round(t_new, 6), "x_column_major_copy_s": round(t_col, 6), "x_transpose_s": round(t_copy, 6),
           "x_layout_kept": "column-major copy" if ens._column_major else "row-major through L2",
           "state_bytes": int(12 * S * T * s + 2 * 4 * 12 * S * T + 4 * S * T)}
    for name, other in (("iforest", vgan_amd.SubspaceIForest(m, p)), ("hbos", vgan_amd.SubspaceHBOS(m, p)), ("dif", vgan_amd.SubspaceDIF(m, p))):
        t_o, to = timed(lambda: other.fit(Xd), reps)
        t_od, tod = timed(lambda: other.decision_function(Xd), reps)
        row.update({f"{name}_fit_s": round(t_o, 6), f"{name}_fit_reps_s": to, f"{name}_decision_function_s": round(t_od, 6),
                    f"{name}_over_rshash_fit": round(t_o / t_first, 2)})
        del other
    if baselines:
        pick = np.unique(np.linspace(0, S - 1, min(S, sample)).astype(int))
        t_np, equal = rshash_host(X, ens, samples.cpu().numpy(), pick)
        row.update({"numpy_subspaces_timed": int(len(pick)), "numpy_16_threads_fit_sums_s": round(t_np * S / len(pick), 3),
                    "numpy_sums_equal_the_device": equal, "fit_speedup_vs_numpy": round(t_np * S / len(pick) / t_first, 1)})
    return row


def ae_torch_bmm(Xd, ens, steps):
    """Seconds per optimiser step of the nets of ens trained in torch on the GPU: every layer one torch.baddbmm over all S
    nets, the first and last layer padded to the widest subspace (the padded inputs are zero, the padded outputs masked out of
    the loss), relu, the sum of the per-net mean squared errors, torch.optim.Adam(weight_decay=); `steps` steps are timed
    after 20 warm ones."""
    dev, S, dims = Xd.device, ens.plan.count, ens.plan.dims
    n, dmax, B = Xd.shape[0], int(dims.max()), min(ens.batch_size, Xd.shape[0])
    mean, sd = ens._scaling
    Z = ((Xd.double() - mean) / sd).float()
    z = torch.zeros(S, n, dmax, device=dev)
    mask = torch.zeros(S, 1, dmax, device=dev)
    for s in range(S):
        f = torch.as_tensor(ens.plan.feat[ens.plan.feat_off[s]:ens.plan.feat_off[s + 1]].astype(np.int64), device=dev)
        z[s, :, :len(f)] = Z[:, f]
        mask[s, 0, :len(f)] = 1.0 / (B * len(f))
    widths = [dmax] + list(ens.hidden) + list(ens.hidden[-2::-1]) + [dmax]
    params = []
    for K, N in zip(widths[:-1], widths[1:]):
        bound = 1.0 / np.sqrt(K)
        params.append(((torch.rand(S, K, N, device=dev) * 2 - 1) * bound).requires_grad_())
        params.append(((torch.rand(S, 1, N, device=dev) * 2 - 1) * bound).requires_grad_())
    opt = torch.optim.Adam(params, lr=ens.lr, betas=(ens.beta1, ens.beta2), eps=ens.eps, weight_decay=ens.weight_decay)
    per_epoch = n // B

    def run(count):
        perm = None
        for g in range(count):
            if g % per_epoch == 0:
                perm = torch.randperm(n, device=dev)
            i = g % per_epoch
            zb = z[:, perm[i * B:(i + 1) * B]]
            h = zb
            for l in range(0, len(params), 2):
                h = torch.baddbmm(params[l + 1], h, params[l])
                if l + 2 < len(params):
                    h = torch.relu(h)
            loss = (((h - zb) ** 2) * mask).sum()
            opt.zero_grad(set_to_none=True)
            loss.backward()
            opt.step()

    run(20)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    run(steps)
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / steps


def run_ae(d, n, count, reps, baselines=True, torch_steps=300):
    from vgan_amd.outlier import ae_chunks, ae_launch_steps, ae_net_bytes
    X, m, p = subspaces_for(d, n, count, seed=d + n + count)
    Xd = torch.as_tensor(X, device="cuda")
    S, dims = len(m), m.sum(axis=1)
    ens = vgan_amd.SubspaceAutoEncoder(m, p)
    t_fit, tf = timed(lambda: ens.fit(Xd), reps)
    t_dec, td = timed(lambda: ens.decision_function(Xd), reps)
    batch = min(ens.batch_size, n)
    chunks = ae_chunks([ae_net_bytes(d_s, ens.hidden, batch, ens._max_dims) for d_s in ens.plan.dims], ens.workspace_bytes)
    t_scale, _ = timed(lambda: ens._column_moments(Xd), reps)
    t_train, tt = timed(lambda: ens._train(Xd, batch, chunks), reps)
    t_score, _ = timed(lambda: ens._score(Xd, False), reps)
    params = int(ens._params.sum())
    row = {"method": "ae", "d": d, "n": n, "S_sampled": count, "S_distinct": S, "hidden": list(ens.hidden), "activation": ens.activation,
           "epochs": ens.epochs, "batch_size": batch, "d_s_min": int(dims.min()), "d_s_median": float(np.median(dims)),
           "d_s_max": int(dims.max()), "parameters": params, "n_steps": ens.n_steps_, "chunks": len(chunks),
           "steps_per_launch": ae_launch_steps(int(ens._params.max()), batch),
           "fit_s": round(t_fit, 5), "fit_reps_s": tf, "decision_function_s": round(t_dec, 6), "decision_function_reps_s": td,
           "scaling_s": round(t_scale, 6), "training_s": round(t_train, 5), "training_reps_s": tt, "scoring_s": round(t_score, 6),
           "training_us_per_step": round(t_train / ens.n_steps_ * 1e6, 2),
           "training_state_bytes_per_step": 4 * 5 * params,  # theta read twice (forward, passed-down error), theta, m, v read and written
           "loss_first_epoch_mean": float(ens.loss_history_[:, 0].mean()), "loss_last_epoch_mean": float(ens.loss_history_[:, -1].mean())}
    lof = vgan_amd.SubspaceEnsemble(m, p, method="lof", n_neighbors=20)
    t_lof, tl = timed(lambda: lof.fit(Xd), reps)
    row.update({"lof_k20_fit_s": round(t_lof, 5), "lof_k20_fit_reps_s": tl, "ae_over_lof_fit": round(t_fit / t_lof, 1)})
    if baselines:
        t_step = ae_torch_bmm(Xd, ens, torch_steps)
        row.update({"torch_bmm_steps_timed": torch_steps, "torch_bmm_us_per_step": round(t_step * 1e6, 2),
                    "torch_bmm_training_s": round(t_step * ens.n_steps_, 3),
                    "training_speedup_vs_torch_bmm": round(t_step * ens.n_steps_ / t_train, 2)})
    return row


def svdd_torch_bmm(Xd, ens, steps):
    """Seconds per optimiser step of the encoders of ens trained in torch on the GPU: every layer one torch.bmm over all S
    nets (no bias), the first layer padded to the widest subspace (the padded inputs are zero), relu, the sum over the nets
    of the batch mean of |out - c|^2, torch.optim.Adam(weight_decay=); `steps` steps are timed after 20 warm ones."""
    dev, S, dims = Xd.device, ens.plan.count, ens.plan.dims
    n, dmax, B = Xd.shape[0], int(dims.max()), min(ens.batch_size, Xd.shape[0])
    mean, sd = ens._scaling
    Z = ((Xd.double() - mean) / sd).float()
    z = torch.zeros(S, n, dmax, device=dev)
    for s in range(S):
        f = torch.as_tensor(ens.plan.feat[ens.plan.feat_off[s]:ens.plan.feat_off[s + 1]].astype(np.int64), device=dev)
        z[s, :, :len(f)] = Z[:, f]
    widths = [dmax] + list(ens.hidden)
    params = [((torch.rand(S, K, N, device=dev) * 2 - 1) / np.sqrt(K)).requires_grad_() for K, N in zip(widths[:-1], widths[1:])]
    center = ens._center[:, None, :]
    opt = torch.optim.Adam(params, lr=ens.lr, betas=(ens.beta1, ens.beta2), eps=ens.eps, weight_decay=ens.weight_decay)
    per_epoch = n // B

    def run(count):
        perm = None
        for g in range(count):
            if g % per_epoch == 0:
                perm = torch.randperm(n, device=dev)
            i = g % per_epoch
            h = z[:, perm[i * B:(i + 1) * B]]
            for l, W in enumerate(params):
                h = torch.bmm(h, W)
                if l + 1 < len(params):
                    h = torch.relu(h)
            loss = ((h - center) ** 2).sum() / B
            opt.zero_grad(set_to_none=True)
            loss.backward()
            opt.step()

    run(20)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    run(steps)
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / steps


def run_svdd(d, n, count, reps, baselines=True, torch_steps=300):
    from vgan_amd.outlier import ae_chunks, ae_launch_steps, ae_net_bytes, svdd_net_bytes
    X, m, p = subspaces_for(d, n, count, seed=d + n + count)
    Xd = torch.as_tensor(X, device="cuda")
    S, dims = len(m), m.sum(axis=1)
    ens = vgan_amd.SubspaceDeepSVDD(m, p)
    t_fit, tf = timed(lambda: ens.fit(Xd), reps)
    t_dec, td = timed(lambda: ens.decision_function(Xd), reps)
    batch = min(ens.batch_size, n)
    chunks = ae_chunks([svdd_net_bytes(d_s, ens.hidden, batch, ens._max_dims) for d_s in ens.plan.dims], ens.workspace_bytes, "SubspaceDeepSVDD")
    t_scale, _ = timed(lambda: ens._column_moments(Xd), reps)
    t_all, tt = timed(lambda: ens._train(Xd, batch, chunks), reps)  # init, centre and every training launch
    epochs, ens.epochs = ens.epochs, 0
    t_center, _ = timed(lambda: ens._train(Xd, batch, chunks), reps)  # init and centre alone
    ens.epochs = epochs
    t_train = t_all - t_center
    t_score, _ = timed(lambda: ens._score(Xd, False), reps)
    params = int(ens._params.sum())
    row = {"method": "deepsvdd", "d": d, "n": n, "S_sampled": count, "S_distinct": S, "hidden": list(ens.hidden), "activation": ens.activation,
           "epochs": ens.epochs, "batch_size": batch, "d_s_min": int(dims.min()), "d_s_median": float(np.median(dims)),
           "d_s_max": int(dims.max()), "parameters": params, "n_steps": ens.n_steps_, "chunks": len(chunks),
           "steps_per_launch": ae_launch_steps(int(ens._params.max()), batch),
           "fit_s": round(t_fit, 5), "fit_reps_s": tf, "decision_function_s": round(t_dec, 6), "decision_function_reps_s": td,
           "scaling_s": round(t_scale, 6), "center_s": round(t_center, 6), "training_s": round(t_train, 5), "center_plus_training_reps_s": tt,
           "scoring_s": round(t_score, 6), "training_us_per_step": round(t_train / ens.n_steps_ * 1e6, 2),
           "n_clamped_mean": float(ens.n_clamped_.mean()),
           "loss_first_epoch_mean": float(ens.loss_history_[:, 0].mean()), "loss_last_epoch_mean": float(ens.loss_history_[:, -1].mean())}
    ae = vgan_amd.SubspaceAutoEncoder(m, p, hidden=ens.hidden)
    t_ae_fit, taf = timed(lambda: ae.fit(Xd), reps)
    ae_chunk = ae_chunks([ae_net_bytes(d_s, ae.hidden, batch, ae._max_dims) for d_s in ae.plan.dims], ae.workspace_bytes)
    t_ae_train, tat = timed(lambda: ae._train(Xd, batch, ae_chunk), reps)
    row.update({"ae_fit_s": round(t_ae_fit, 5), "ae_fit_reps_s": taf, "ae_training_s": round(t_ae_train, 5), "ae_training_reps_s": tat,
                "ae_training_us_per_step": round(t_ae_train / ae.n_steps_ * 1e6, 2),
                "step_time_over_ae": round(t_train / ens.n_steps_ / (t_ae_train / ae.n_steps_), 3)})
    lof = vgan_amd.SubspaceEnsemble(m, p, method="lof", n_neighbors=20)
    t_lof, tl = timed(lambda: lof.fit(Xd), reps)
    row.update({"lof_k20_fit_s": round(t_lof, 5), "lof_k20_fit_reps_s": tl, "deepsvdd_over_lof_fit": round(t_fit / t_lof, 1)})
    if baselines:
        t_step = svdd_torch_bmm(Xd, ens, torch_steps)
        row.update({"torch_bmm_steps_timed": torch_steps, "torch_bmm_us_per_step": round(t_step * 1e6, 2),
                    "torch_bmm_training_s": round(t_step * ens.n_steps_, 3),
                    "training_speedup_vs_torch_bmm": round(t_step * ens.n_steps_ / t_train, 2)})
    return row


def run_sod(d, n, count, k, ref_set, alpha, reps):
    """SubspaceSOD fit and decision_function (the training rows as new rows), the fit split into its stages on the resident
    lists, beside the LOF fit with the same n_neighbors on the same rows in the same run."""
    X, m, p = subspaces_for(d, n, count, seed=d + n + count)
    Xd = torch.as_tensor(X, device="cuda")
    S, dims = len(m), m.sum(axis=1)
    sod = vgan_amd.SubspaceSOD(m, p, n_neighbors=k, ref_set=ref_set, alpha=alpha)
    lof = vgan_amd.SubspaceEnsemble(m, p, method="lof", n_neighbors=k)
    t_fit, tf = timed(lambda: sod.fit(Xd), reps)
    t_lof, tl = timed(lambda: lof.fit(Xd), reps)
    t_dec, td = timed(lambda: sod.decision_function(Xd), reps)
    t_lists, _ = timed(lambda: [None for _ in sod._neighbors(None)], reps)
    lists = [(first, cnt, idx) for first, cnt, idx, _ in sod._neighbors(None)]
    cursor = torch.empty(S, n, dtype=torch.int32, device="cuda")
    per = torch.empty(S, n, dtype=torch.float32, device="cuda")

    def reverse_launches():
        for first, cnt, idx in lists:
            sod.ops.sod_reverse_lists(idx, sod._rn_off[first:first + cnt], sod._rn_rows[first:first + cnt], cursor[:cnt])

    def set_launches():
        for first, cnt, idx in lists:
            sod._sets(idx, first, cnt, sod._ref[first:first + cnt], sod._unshared[first:first + cnt])

    def score_launches():
        for first, cnt, idx in lists:
            sod.ops.sod_score(sod._X, sod._X, sod._table, first, cnt, sod._ref[first:first + cnt], alpha, 0, per,
                              sod._rows[first:first + cnt], sod._n_rel[first:first + cnt])

    t_rev, _ = timed(reverse_launches, max(reps, 5))
    t_sets, ts = timed(set_launches, max(reps, 5))
    t_score, tsc = timed(score_launches, max(reps, 5))
    rn = (sod._rn_off[:, 1:] - sod._rn_off[:, :-1]).double()
    # the scoring launch reads every reference row's feature four times (two sums, formed for V and again for the mask and Q)
    gather_bytes = 4.0 * 4.0 * n * ref_set * float(dims.sum())
    increments = float((rn * rn).sum())  # sum over m of |RN(m)|^2: a row x adds |RN(m)| for each m in N(x)
    return {"method": "sod", "d": d, "n": n, "S_sampled": count, "S_distinct": S, "n_neighbors": k, "ref_set": ref_set, "alpha": alpha,
            "d_s_min": int(dims.min()), "d_s_median": float(np.median(dims)), "d_s_max": int(dims.max()),
            "sod_fit_s": round(t_fit, 5), "sod_fit_reps_s": tf, "lof_fit_s": round(t_lof, 5), "lof_fit_reps_s": tl,
            "sod_over_lof": round(t_fit / t_lof, 3), "decision_function_s": round(t_dec, 5), "decision_function_reps_s": td,
            "lists_s": round(t_lists, 5), "reverse_lists_s": round(t_rev, 6), "reference_sets_s": round(t_sets, 6),
            "reference_sets_reps_s": ts, "scores_s": round(t_score, 6), "scores_reps_s": tsc,
            "sod_stages_over_lists": round((t_rev + t_sets + t_score) / t_lists, 3),
            "reverse_list_max": int(rn.max()), "increments": increments,
            "increments_per_s": round(increments / t_sets / 1e9, 3), "n_unshared": int(sod.n_unshared_.sum()),
            "n_relevant_median": float(np.median(sod.n_relevant_)),
            "score_gather_bytes": gather_bytes, "score_gather_GBps": round(gather_bytes / t_score / 1e9, 1)}


VALU_PEAK_OPS = FP32_PEAK / 2  # vector-ALU operations per second: the fp32 peak counts a fused multiply-add as two
METRIC_ARMS = [("euclidean", None), ("manhattan", None), ("chebyshev", None), ("minkowski", 0.5), ("cosine", None)]


def run_metric(d, n, count, k, reps, baselines=True, sklearn_sample=2):
    """The LOF fit under each of the five metrics in one session (the Euclidean fit is the yardstick); the Minkowski-family
    sweep (vgan_outlier_knn_metric on resident blocks) alone, as pair-features per second and, for Manhattan and Chebyshev,
    whose pair-feature costs two vector operations, as a share of the vector peak; torch.cdist(p=1) + topk per subspace on
    the GPU; sklearn's brute-force Manhattan LOF on 16 threads on sklearn_sample subspaces, scaled to all."""
    X, m, p = subspaces_for(d, n, count, seed=d + n + count)
    Xd = torch.as_tensor(X, device="cuda")
    S, dims = len(m), m.sum(axis=1)
    row = {"method": "metric", "d": d, "n": n, "S_sampled": count, "S_distinct": S, "n_neighbors": k, "d_s_min": int(dims.min()),
           "d_s_median": float(np.median(dims)), "d_s_max": int(dims.max()), "lof_fit_s": {}, "lof_fit_reps_s": {}, "sweep": {}}
    fitted = {}
    for metric, pw in METRIC_ARMS:
        name = metric if pw is None else f"{metric}_p{pw:g}"
        ens = vgan_amd.SubspaceEnsemble(m, p, method="lof", n_neighbors=k, metric=metric, p=pw)
        t, ts = timed(lambda: ens.fit(Xd), reps)
        row["lof_fit_s"][name], row["lof_fit_reps_s"][name] = round(t, 5), ts
        fitted[name] = ens
    row["lof_fit_over_euclidean"] = {name: round(t / row["lof_fit_s"]["euclidean"], 3) for name, t in row["lof_fit_s"].items()}
    padded = -(-n // 64) * 64
    pair_features = float(padded) * padded * float(((dims + 3) // 4 * 4).sum())
    for name, code, pw in (("manhattan", 1, 0.0), ("chebyshev", 2, 0.0), ("minkowski_p0.5", 3, 0.5)):
        ens = fitted[name]
        chunks = [(first, cnt, Pq) for first, cnt, _, _, Pq, _, _, _ in ens._chunks(None)]
        nbr = torch.empty(S, n, k, dtype=torch.int32, device="cuda")
        J = {first: ens._splits(n, n, cnt) for first, cnt, _ in chunks}
        parts = {first: (torch.empty(cnt * J[first] * n * k, dtype=torch.float32, device="cuda"),
                         torch.empty(cnt * J[first] * n * k, dtype=torch.int32, device="cuda")) for first, cnt, _ in chunks}

        def sweep_launches():
            for first, cnt, P in chunks:
                ens.ops.outlier_knn_metric(P, n, P, n, ens._table, first, cnt, k, True, code, pw, J[first], nbr[first:first + cnt],
                                           *(parts[first] if J[first] > 1 else (None, None)))

        t, ts = timed(sweep_launches, max(reps, 5))
        entry = {"s": round(t, 6), "reps_s": ts, "splits": sorted(set(J.values())), "pair_features_per_s": round(pair_features / t, 1)}
        if code != 3:
            entry["valu_ops_per_s"] = round(2.0 * pair_features / t, 1)
            entry["frac_vector_peak"] = round(2.0 * pair_features / t / VALU_PEAK_OPS, 4)
        row["sweep"][name] = entry
        del chunks, parts, nbr
    if baselines:
        feats = [torch.as_tensor(np.flatnonzero(m[s]), device="cuda") for s in range(S)]

        def torch_l1():
            out = []
            for f in feats:
                Xs = Xd[:, f].contiguous()
                for q0 in range(0, n, 4096):
                    D = torch.cdist(Xs[q0:q0 + 4096], Xs, p=1.0)
                    D[torch.arange(D.shape[0], device="cuda"), torch.arange(q0, q0 + D.shape[0], device="cuda")] = float("inf")
                    out.append(torch.topk(D, k, dim=1, largest=False))
            return out

        t, ts = timed(torch_l1, reps)
        row.update({"torch_cdist_p1_topk_s": round(t, 5), "torch_cdist_p1_topk_reps_s": ts,
                    "torch_over_manhattan_sweep": round(t / row["sweep"]["manhattan"]["s"], 3)})
        from sklearn.neighbors import LocalOutlierFactor
        pick = list(range(min(sklearn_sample, S)))
        t0 = time.perf_counter()
        for s in pick:
            LocalOutlierFactor(n_neighbors=k, algorithm="brute", metric="manhattan", n_jobs=16).fit(X[:, np.flatnonzero(m[s])])
        t_sk = (time.perf_counter() - t0) * S / len(pick)
        row.update({"sklearn_brute_manhattan_16_threads_scaled_s": round(t_sk, 3), "sklearn_subspaces_timed": len(pick),
                    "sklearn_over_manhattan_fit": round(t_sk / row["lof_fit_s"]["manhattan"], 1)})
    return row


def _hics_numpy_contrasts(job):
    """Worker of run_hics: the plain numpy restatement of the contrast (tests/hics_ref.py's, with the library's vectorised
    draws) for a list of feature sets; runs in a spawned process that never touches the GPU."""
    from vgan_amd.hics import hics_draws, hics_slice_width
    order, sets, ids, alpha, M, seed = job
    n = order.shape[1]
    r = np.arange(1, n + 1, dtype=np.int64)
    out = []
    for feats, sid in zip(sets, ids):
        k = len(feats)
        w = hics_slice_width(n, k, alpha)
        c, start = hics_draws(n, k, w, M, seed, sid)
        total = 0.0
        for t in range(M):
            member = np.ones(n, dtype=bool)
            for p, f in enumerate(feats):
                if p != c[t]:
                    inside = np.zeros(n, dtype=bool)
                    inside[order[f, start[t, p]:start[t, p] + w]] = True
                    member &= inside
            cnt = np.cumsum(member[order[feats[c[t]]]].astype(np.int64))
            m = int(cnt[-1])
            if m:
                total += float(np.abs(cnt * n - r * m).max()) / float(n * m)
        out.append(total / M)
    return out


def _hics_numpy(pool, workers, order, sets, ids, alpha, M, seed):
    """(seconds, contrasts) of the restatement over `sets`, dealt to the pool's workers in equal parts."""
    parts = [(order, sets[i::workers], ids[i::workers], alpha, M, seed) for i in range(workers)]
    t0 = time.perf_counter()
    res = pool.map(_hics_numpy_contrasts, parts)
    dt = time.perf_counter() - t0
    out = np.empty(len(sets))
    for i, r in enumerate(res):
        out[i::workers] = r
    return dt, out


def run_hics(d, n, count, reps, pool, workers=16, numpy_pairs=256, numpy_wide=16):
    """HiCS at its defaults on X [n, d]: the fit split into the argsort, level 2 (under both workgroup shapes) and the higher
    levels (their candidates replayed on the resident index), the contrast of the model's `count` sampled subspaces, and the
    numpy restatement in `workers` processes on a sample of the level-2 pairs and of the model's subspaces, scaled up."""
    from vgan_amd.hics import HICS_WAVE_GROUP, ContrastIndex, HiCS
    X, m, p = subspaces_for(d, n, count, seed=d + n + count)
    Xd = torch.as_tensor(X, device="cuda")
    search = HiCS()
    alpha, M, seed = search.alpha, search.n_iterations, search.seed
    t_fit, tf = timed(lambda: search.fit(Xd), reps)
    t_sort, ts = timed(lambda: ContrastIndex(Xd), reps)
    index = ContrastIndex(Xd)

    def level(lv, group=0):
        cands = lv["candidates"]
        ids = (np.uint64(lv["k"]) << np.uint64(32)) | np.arange(len(cands), dtype=np.uint64)
        return index.contrast(cands.reshape(-1), np.arange(len(cands) + 1, dtype=np.int64) * lv["k"], alpha, M, seed, ids, group=group)

    lv2, higher = search.levels_[0], search.levels_[1:]
    t_l2, tl2 = timed(lambda: level(lv2), reps)
    t_l2_block, _ = timed(lambda: level(lv2, 1), reps)
    t_l2_wave, _ = timed(lambda: level(lv2, HICS_WAVE_GROUP), reps) if n <= 65536 else (None, None)
    t_high, th = timed(lambda: [level(lv) for lv in higher], reps)
    draws2 = len(lv2["candidates"]) * M
    draws_high = sum(len(lv["candidates"]) for lv in higher) * M
    dims = m.sum(axis=1)
    t_model, tm = timed(lambda: vgan_amd.subspace_contrast(Xd, m), reps)
    _, feat, feat_off = vgan_amd.hics._lists_of(m)
    t_model_sweep, _ = timed(lambda: index.contrast(feat, feat_off, alpha, M, seed, np.arange(len(m), dtype=np.uint64)), reps)
    t_model_block, _ = timed(lambda: index.contrast(feat, feat_off, alpha, M, seed, np.arange(len(m), dtype=np.uint64), group=1), reps)
    t_model_wave, _ = timed(lambda: index.contrast(feat, feat_off, alpha, M, seed, np.arange(len(m), dtype=np.uint64),
                                                   group=HICS_WAVE_GROUP), reps) if n <= 65536 else (None, None)
    widths = np.asarray([vgan_amd.hics.hics_slice_width(n, int(k), alpha) for k in dims])
    marks = float(((dims - 1) * np.minimum(n - widths, widths)).sum()) * M  # bits set or cleared by all draws
    row = {"method": "hics", "d": d, "n": n, "alpha": alpha, "n_iterations": M, "candidate_cutoff": search.candidate_cutoff,
           "fit_s": round(t_fit, 4), "fit_reps_s": tf, "argsort_s": round(t_sort, 5), "argsort_reps_s": ts,
           "level2_candidates": len(lv2["candidates"]), "level2_s": round(t_l2, 4), "level2_reps_s": tl2,
           "level2_draws_per_s": round(draws2 / t_l2), "level2_workgroup_per_draw_s": round(t_l2_block, 4),
           "level2_wave_per_draw_s": None if t_l2_wave is None else round(t_l2_wave, 4),
           "levels": [{"k": lv["k"], "candidates": len(lv["candidates"])} for lv in search.levels_],
           "higher_levels_s": round(t_high, 4), "higher_levels_reps_s": th,
           "higher_levels_draws_per_s": round(draws_high / t_high) if draws_high else None,
           "fit_host_remainder_s": round(t_fit - t_sort - t_l2 - t_high, 4),
           "found": int(len(search.subspaces)), "best_contrast": float(search.contrast_[0]),
           "model_subspaces": int(len(m)), "model_d_s_min": int(dims.min()), "model_d_s_median": float(np.median(dims)),
           "model_d_s_max": int(dims.max()), "model_subspace_contrast_s": round(t_model, 6), "model_subspace_contrast_reps_s": tm,
           "model_sweep_s": round(t_model_sweep, 6), "model_sweep_workgroup_per_draw_s": round(t_model_block, 6),
           "model_sweep_wave_per_draw_s": None if t_model_wave is None else round(t_model_wave, 6),
           "model_marks": marks, "model_marks_per_s": round(marks / t_model_sweep)}
    if pool is not None:
        order = index.order.cpu().numpy().astype(np.int64)
        pick = np.random.default_rng(0).choice(len(lv2["candidates"]), size=min(numpy_pairs, len(lv2["candidates"])), replace=False)
        pick.sort()
        sets = [tuple(int(f) for f in lv2["candidates"][i]) for i in pick]
        ids = [(2 << 32) | int(i) for i in pick]
        t_np, got = _hics_numpy(pool, workers, order, sets, ids, alpha, M, seed)
        same = bool(np.array_equal(got.view(np.int64), lv2["contrast"][pick].view(np.int64)))
        wide = list(range(min(numpy_wide, len(m))))
        t_np_wide, got_wide = _hics_numpy(pool, workers, order, [tuple(np.flatnonzero(m[z]).tolist()) for z in wide], wide, alpha, M, seed)
        want_wide = vgan_amd.subspace_contrast(Xd, m[wide])
        row.update({"numpy_workers": workers, "numpy_pairs_timed": len(sets), "numpy_pairs_s": round(t_np, 3),
                    "numpy_level2_scaled_s": round(t_np * len(lv2["candidates"]) / len(sets), 1),
                    "level2_speedup_vs_numpy": round(t_np * len(lv2["candidates"]) / len(sets) / t_l2, 1),
                    "numpy_pairs_bit_equal": same, "numpy_model_subspaces_timed": len(wide), "numpy_model_subspaces_s": round(t_np_wide, 3),
                    "numpy_model_scaled_s": round(t_np_wide * len(m) / len(wide), 2),
                    "model_sweep_speedup_vs_numpy": round(t_np_wide * len(m) / len(wide) / t_model_sweep, 1),
                    "numpy_model_bit_equal": bool(np.array_equal(got_wide.view(np.int64), want_wide.view(np.int64)))})
    return row


def run_hics_shapes(d, rows, reps, M=50, alpha=0.1):
    """All pairs of d independent Gaussian features, M draws each, under a workgroup per draw and a wave per draw, per n."""
    from vgan_amd.hics import HICS_WAVE_GROUP, ContrastIndex
    a, b = np.triu_indices(d, 1)
    feat = np.stack([a, b], axis=1).astype(np.int32).reshape(-1)
    off = np.arange(len(a) + 1, dtype=np.int64) * 2
    ids = np.arange(len(a), dtype=np.uint64)
    out = []
    for n in rows:
        X = torch.as_tensor(np.random.default_rng(n).standard_normal((n, d)).astype(np.float32), device="cuda")
        index = ContrastIndex(X)
        t_block, _ = timed(lambda: index.contrast(feat, off, alpha, M, 0, ids, group=1), reps)
        t_wave, _ = timed(lambda: index.contrast(feat, off, alpha, M, 0, ids, group=HICS_WAVE_GROUP), reps)
        out.append({"d": d, "n": n, "pairs": len(a), "n_iterations": M, "workgroup_per_draw_s": round(t_block, 6),
                    "wave_per_draw_s": round(t_wave, 6), "wave_over_workgroup": round(t_wave / t_block, 3)})
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--sweep", action="store_true")
    ap.add_argument("--quick", action="store_true", help="small shapes only (a rehearsal)")
    ap.add_argument("--method", choices=["knn", "kde", "cblof", "abod", "cof", "ecod", "iforest", "inne", "mahalanobis", "gmm", "hbos", "loda", "pca", "ocsvm", "sos", "dif", "sod", "kpca", "ae", "deepsvdd", "hics", "metric", "loci", "rshash"], default="knn")
    ap.add_argument("--n-dims", type=int, default=1, help="iforest: features of an oblique cut (SubspaceIForest's n_dims); from 2 on the "
                    "row also times the axis-parallel forest and SubspaceDIF on the same rows")
    ap.add_argument("--iters", type=int, default=20, help="cblof: Lloyd iterations of every path")
    ap.add_argument("--no-baselines", action="store_true", help="cblof / abod / cof / ecod / iforest / inne / mahalanobis / gmm / hbos / loda / pca / ocsvm / sos / loci / dif / kpca / ae / deepsvdd / rshash: the fused path only (for a run under a profiler)")
    ap.add_argument("--bandwidth", default="1.0", help="KDE bandwidth: a float, 'scott' or 'silverman'")
    ap.add_argument("--normalize", choices=["zscore", "robust", "minmax"], action="append",
                    help="measure score normalisation (repeat for several modes)")
    ap.add_argument("--shape", help="abod / cof / ecod / iforest / inne / mahalanobis / gmm / hbos / loda / pca / ocsvm / sos / loci / dif / sod / kpca / ae / deepsvdd / rshash: one shape d,n,S_sampled instead of the table's (for a run under a profiler)")
    ap.add_argument("--out", help="also write the JSON result to this file")
    args = ap.parse_args()
    bandwidth = args.bandwidth if args.bandwidth in ("scott", "silverman") else float(args.bandwidth)
    pool = None
    if args.method == "hics" and not args.no_baselines:
        # the numpy workers are spawned before this process touches the GPU and never open it themselves
        import multiprocessing
        pool = multiprocessing.get_context("spawn").Pool(16)
        pool.map(abs, range(16))
    assert torch.cuda.is_available(), "outlier_bench needs an MI355X"
    configs = [(10, 10_000, 50, 5, True), (10, 10_000, 50, 20, True), (10, 50_000, 500, 5, True), (10, 50_000, 500, 20, False),
               (784, 10_000, 50, 5, True), (784, 10_000, 50, 20, False), (784, 50_000, 50, 5, False)]
    if args.method == "kde":
        configs = [(10, 10_000, 50, 0, True), (10, 50_000, 500, 0, True), (784, 10_000, 50, 0, True)]
    if args.quick:
        configs = [(10, 2000, 20, 5, True), (784, 2000, 10, 5, True)]
    out = {"tool": "outlier_bench", "device": torch.cuda.get_device_name(0), "configs": []}
    if args.normalize:
        shapes = [(10, 2000, 20), (784, 2000, 10)] if args.quick else [(10, 10_000, 50), (10, 50_000, 500), (784, 10_000, 50)]
        for mode in args.normalize:
            for d, n, count in shapes:
                out["configs"].append(run_normalize(d, n, count, mode, args.reps))
                print(json.dumps(out["configs"][-1]), file=sys.stderr, flush=True)
        if not args.quick:
            out["launches_on_a_full_matrix"] = [normalize_launches(mode, args.reps) for mode in args.normalize]
        configs = []
    if args.method == "cblof":
        shapes = [(10, 2000, 20), (784, 2000, 10)] if args.quick else [(10, 10_000, 50), (10, 50_000, 500), (784, 10_000, 50)]
        for d, n, count in shapes:
            for C in (8, 64):
                out["configs"].append(run_cblof(d, n, count, C, args.reps, args.iters, baselines=not args.no_baselines))
                print(json.dumps(out["configs"][-1]), file=sys.stderr, flush=True)
        configs = []
    if args.method == "cof":
        shapes = [(10, 2000, 20), (784, 2000, 10)] if args.quick else [(10, 10_000, 50), (10, 50_000, 500), (784, 10_000, 50),
                                                                         (784, 50_000, 50)]
        if args.shape:
            shapes = [tuple(int(v) for v in args.shape.split(","))]
        for d, n, count in shapes:
            for k in (10, 32):
                out["configs"].append(run_cof(d, n, count, k, args.reps, baselines=not args.no_baselines))
                print(json.dumps(out["configs"][-1]), file=sys.stderr, flush=True)
        configs = []
    if args.method == "abod":
        shapes = [(10, 2000, 20), (784, 2000, 10)] if args.quick else [(10, 10_000, 50), (10, 50_000, 500), (784, 10_000, 50),
                                                                         (784, 50_000, 50)]
        if args.shape:
            shapes = [tuple(int(v) for v in args.shape.split(","))]
        for d, n, count in shapes:
            for k in (10, 32):
                out["configs"].append(run_abod(d, n, count, k, args.reps, baselines=not args.no_baselines))
                print(json.dumps(out["configs"][-1]), file=sys.stderr, flush=True)
        configs = []
    if args.method == "ecod":
        shapes = [(10, 2000, 20), (784, 2000, 10)] if args.quick else [(10, 10_000, 50), (10, 50_000, 500), (784, 10_000, 50),
                                                                         (784, 50_000, 50)]
        if args.shape:
            shapes = [tuple(int(v) for v in args.shape.split(","))]
        for d, n, count in shapes:
            out["configs"].append(run_ecod(d, n, count, args.reps, baselines=not args.no_baselines))
            print(json.dumps(out["configs"][-1]), file=sys.stderr, flush=True)
        if not args.shape:  # the dense product against the gather-sum at chosen S, small and wide
            grid = [(10, 2000, 64), (784, 2000, 64)] if args.quick else [(10, 50_000, 64), (10, 50_000, 512), (784, 50_000, 64),
                                                                         (784, 50_000, 512)]
            out["product_vs_gather"] = [run_ecod(d, n, S, args.reps, baselines=False, random_masks=True) for d, n, S in grid]
        configs = []
    if args.method in ("hbos", "loda"):
        shapes = [(10, 2000, 20), (784, 2000, 10)] if args.quick else [(10, 10_000, 50), (10, 50_000, 500), (784, 10_000, 50),
                                                                         (784, 50_000, 50)]
        if args.shape:
            shapes = [tuple(int(v) for v in args.shape.split(","))]
        for d, n, count in shapes:
            out["configs"].append((run_hbos if args.method == "hbos" else run_loda)(d, n, count, args.reps, baselines=not args.no_baselines))
            print(json.dumps(out["configs"][-1]), file=sys.stderr, flush=True)
        configs = []
    if args.method == "iforest":
        shapes = [(10, 2000, 20), (784, 2000, 10)] if args.quick else [(10, 10_000, 50), (10, 50_000, 500), (784, 10_000, 50),
                                                                         (784, 50_000, 50)]
        if args.shape:
            shapes = [tuple(int(v) for v in args.shape.split(","))]
        for d, n, count in shapes:
            out["configs"].append(run_iforest(d, n, count, args.reps, baselines=not args.no_baselines, n_dims=args.n_dims))
            print(json.dumps(out["configs"][-1]), file=sys.stderr, flush=True)
        configs = []
    if args.method == "inne":
        shapes = [(10, 2000, 20), (784, 2000, 10)] if args.quick else [(10, 10_000, 50), (10, 50_000, 500), (784, 10_000, 50),
                                                                         (784, 50_000, 50)]
        if args.shape:
            shapes = [tuple(int(v) for v in args.shape.split(","))]
        for d, n, count in shapes:
            out["configs"].append(run_inne(d, n, count, args.reps, baselines=not args.no_baselines))
            print(json.dumps(out["configs"][-1]), file=sys.stderr, flush=True)
        if not args.shape:  # the gather of the query features as given against neighbouring columns, narrow and three feature tiles wide
            grid = [(2000, 8, 16), (2000, 80, 16)] if args.quick else [(50_000, 8, 64), (50_000, 80, 64)]
            out["gather_vs_neighbouring_columns"] = [run_inne_gather(n, width, S, args.reps) for n, width, S in grid]
        configs = []
    if args.method == "mahalanobis":
        shapes = [(10, 2000, 20), (784, 2000, 10)] if args.quick else [(10, 10_000, 50), (10, 50_000, 500), (784, 10_000, 50),
                                                                         (784, 50_000, 50)]
        if args.shape:
            shapes = [tuple(int(v) for v in args.shape.split(","))]
        for d, n, count in shapes:
            out["configs"].append(run_maha(d, n, count, args.reps, baselines=not args.no_baselines))
            print(json.dumps(out["configs"][-1]), file=sys.stderr, flush=True)
        configs = []
    if args.method == "pca":
        shapes = [(10, 2000, 20), (784, 2000, 10)] if args.quick else [(10, 10_000, 50), (10, 50_000, 500), (784, 10_000, 50),
                                                                         (784, 50_000, 50)]
        if args.shape:
            shapes = [tuple(int(v) for v in args.shape.split(","))]
        widest = 0
        for d, n, count in shapes:
            out["configs"].append(run_pca(d, n, count, args.reps, baselines=not args.no_baselines))
            print(json.dumps(out["configs"][-1]), file=sys.stderr, flush=True)
            widest = max(widest, out["configs"][-1]["d_s_max"])
        if not args.shape:  # the solver alone per width: 16, 64, 256 and the widest subspace the table above held
            out["eigen_by_width"] = run_pca_widths(2000 if args.quick else 10_000, sorted({16, 64, 256, widest}), args.reps)
        configs = []
    if args.method == "ocsvm":
        shapes = [(10, 2000, 20), (784, 2000, 10)] if args.quick else [(10, 2000, 50), (10, 10_000, 50), (784, 2000, 50), (784, 10_000, 50)]
        if args.shape:
            shapes = [tuple(int(v) for v in args.shape.split(","))]
        for d, n, count in shapes:
            out["configs"].append(run_ocsvm(d, n, count, args.reps, baselines=not args.no_baselines))
            print(json.dumps(out["configs"][-1]), file=sys.stderr, flush=True)
        configs = []
    if args.method == "kpca":
        shapes = [(10, 2000, 20), (784, 2000, 10)] if args.quick else [(784, 2000, 50), (784, 10_000, 50)]
        if args.shape:
            shapes = [tuple(int(v) for v in args.shape.split(","))]
        for max_samples in ("auto",) if args.quick else ("auto", 1024):
            for d, n, count in shapes:
                out["configs"].append(run_kpca(d, n, count, args.reps, baselines=not args.no_baselines, max_samples=max_samples))
                print(json.dumps(out["configs"][-1]), file=sys.stderr, flush=True)
        configs = []
    if args.method == "sos":
        shapes = [(10, 2000, 20), (784, 2000, 10)] if args.quick else [(10, 2000, 50), (10, 10_000, 50), (784, 2000, 50), (784, 10_000, 50)]
        if args.shape:
            shapes = [tuple(int(v) for v in args.shape.split(","))]
        for d, n, count in shapes:
            out["configs"].append(run_sos(d, n, count, args.reps, baselines=not args.no_baselines))
            print(json.dumps(out["configs"][-1]), file=sys.stderr, flush=True)
        configs = []
    if args.method == "loci":
        shapes = [(10, 2000, 20), (784, 2000, 10)] if args.quick else [(784, 2000, 50), (784, 10_000, 50)]
        if args.shape:
            shapes = [tuple(int(v) for v in args.shape.split(","))]
        for d, n, count in shapes:
            out["configs"].append(run_loci(d, n, count, args.reps, baselines=not args.no_baselines, sample=2 if n <= 2000 else 1))
            print(json.dumps(out["configs"][-1]), file=sys.stderr, flush=True)
        configs = []
    if args.method == "sod":
        shapes = [(784, 2000, 10)] if args.quick else [(784, 2000, 50), (784, 10_000, 50)]
        if args.shape:
            shapes = [tuple(int(v) for v in args.shape.split(","))]
        for d, n, count in shapes:
            for k, ref_set, alpha in ((20, 10, 0.8), (32, 31, 0.3)):
                out["configs"].append(run_sod(d, n, count, k, ref_set, alpha, args.reps))
                print(json.dumps(out["configs"][-1]), file=sys.stderr, flush=True)
        configs = []
    if args.method == "dif":
        shapes = [(10, 2000, 20), (784, 2000, 10)] if args.quick else [(10, 10_000, 50), (784, 10_000, 50), (784, 50_000, 50)]
        if args.shape:
            shapes = [tuple(int(v) for v in args.shape.split(","))]
        for d, n, count in shapes:
            out["configs"].append(run_dif(d, n, count, args.reps, baselines=not args.no_baselines))
            print(json.dumps(out["configs"][-1]), file=sys.stderr, flush=True)
        configs = []
    if args.method == "ae":
        shapes = [(20, 500, 8)] if args.quick else [(784, 2000, 50), (784, 10_000, 50)]
        if args.shape:
            shapes = [tuple(int(v) for v in args.shape.split(","))]
        for d, n, count in shapes:
            out["configs"].append(run_ae(d, n, count, args.reps, baselines=not args.no_baselines))
            print(json.dumps(out["configs"][-1]), file=sys.stderr, flush=True)
        configs = []
    if args.method == "deepsvdd":
        shapes = [(20, 500, 8)] if args.quick else [(784, 2000, 50), (784, 10_000, 50)]
        if args.shape:
            shapes = [tuple(int(v) for v in args.shape.split(","))]
        for d, n, count in shapes:
            out["configs"].append(run_svdd(d, n, count, args.reps, baselines=not args.no_baselines))
            print(json.dumps(out["configs"][-1]), file=sys.stderr, flush=True)
        configs = []
    if args.method == "hics":
        shapes = [(20, 500, 8)] if args.quick else [(784, 2000, 50), (784, 10_000, 50)]
        if args.shape:
            shapes = [tuple(int(v) for v in args.shape.split(","))]
        for d, n, count in shapes:
            out["configs"].append(run_hics(d, n, count, args.reps, pool))
            print(json.dumps(out["configs"][-1]), file=sys.stderr, flush=True)
        if pool is not None:
            pool.close()
            pool.join()
        if not args.shape:  # where the two workgroup shapes of the draw kernel meet
            out["workgroup_shapes"] = run_hics_shapes(64, [1024, 4096] if args.quick else [4096, 16384, 32768, 65536], args.reps)
        configs = []
    if args.method == "rshash":
        shapes = [(20, 500, 8)] if args.quick else [(784, 2000, 50), (784, 10_000, 50), (784, 50_000, 50)]
        if args.shape:
            shapes = [tuple(int(v) for v in args.shape.split(","))]
        for d, n, count in shapes:
            out["configs"].append(run_rshash(d, n, count, args.reps, baselines=not args.no_baselines))
            print(json.dumps(out["configs"][-1]), file=sys.stderr, flush=True)
        configs = []
    if args.method == "metric":
        shapes = [(784, 2000, 10)] if args.quick else [(784, 2000, 50), (784, 10_000, 50)]
        if args.shape:
            shapes = [tuple(int(v) for v in args.shape.split(","))]
        for d, n, count in shapes:
            out["configs"].append(run_metric(d, n, count, 20, args.reps, baselines=not args.no_baselines))
            print(json.dumps(out["configs"][-1]), file=sys.stderr, flush=True)
        configs = []
    if args.method == "gmm":
        shapes = [(10, 2000, 20), (784, 2000, 10)] if args.quick else [(10, 10_000, 50), (10, 50_000, 500), (784, 10_000, 50),
                                                                         (784, 50_000, 50)]
        if args.shape:
            shapes = [tuple(int(v) for v in args.shape.split(","))]
        for d, n, count in shapes:
            out["configs"].append(run_gmm(d, n, count, args.reps, baselines=not args.no_baselines))
            print(json.dumps(out["configs"][-1]), file=sys.stderr, flush=True)
        configs = []
    for d, n, count, k, with_base in configs:
        out["configs"].append(run_config(d, n, count, k, args.reps, with_base, args.method, bandwidth))
        print(json.dumps(out["configs"][-1]), file=sys.stderr, flush=True)
    if args.sweep:
        out["engine_sweep"] = sweep(2000 if args.quick else 10_000, args.reps)
    print(json.dumps(out))
    if args.out:
        with open(args.out, "w") as f:
            json.dump(out, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
