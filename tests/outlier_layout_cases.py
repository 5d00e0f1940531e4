"""What tests/test_outlier_layout_gpu.py sweeps and tests/test_outlier_layout_cpu.py pins without a device: the table of
C-ABI entries that read a raw data matrix through a leading dimension, the detector cases, their shapes and their data.

A new detector joins in two places: a Case below (its class, the smallest parameters of its own test_outlier_*_gpu.py, and
its public methods that take a matrix), and, for every new entry point with an ldx / ldq / ldr parameter, a name in
ENTRY_TABLE.  The CPU module fails until both are there.
"""
import numpy as np

from test_outlier_ecod_cpu import _mask, tied_data  # noqa: F401  (tied_data: the HiCS direct call of the GPU module)
from test_outlier_maha_cpu import raw_data

# Every prototype of include/vgan_hip.h from vgan_outlier_pack to the end of the file that has a parameter named ldx, ldq or
# ldr.  The ops.HipOps method of an entry is its name without the "vgan_" prefix.
ENTRY_TABLE = [
    "vgan_outlier_pack", "vgan_outlier_refine", "vgan_outlier_pack_unit", "vgan_outlier_refine_metric",
    "vgan_outlier_abod", "vgan_outlier_cof_chain",
    "vgan_cluster_lloyd", "vgan_cluster_final",
    "vgan_ecod_sort_columns", "vgan_ecod_tail_counts",
    "vgan_hist_column_range", "vgan_hist_column_counts", "vgan_hbos_scores",
    "vgan_iforest_build", "vgan_iforest_path_sums",
    "vgan_rshash_build",
    "vgan_dif_represent",
    "vgan_ae_train", "vgan_ae_scores",
    "vgan_svdd_center", "vgan_svdd_train", "vgan_svdd_scores",
    "vgan_inne_build", "vgan_inne_scores",
    "vgan_maha_moments", "vgan_maha_scores",
    "vgan_gmm_moments", "vgan_gmm_estep",
    "vgan_pca_scores",
    "vgan_sod_score",
    "vgan_hics_argsort_columns",
]

# ---- shapes: the smallest at which these kernels can still go wrong ------------------------------------------------------
DIM = 37  # off every multiple of 4: the pad of an "aligned" leading dimension is not empty
N_FIT, N_QUERY = 130, 67  # two 64-row tiles plus 2; one tile plus 3
CONSTANT = 3  # the constant column; it lies in the subspaces of width 5, 33 and 37
# widths 1 (a single feature), 5 (one off the packed width 4), 33 (one past the 32-feature block), 37 (all features)
FEATURES = [[7], [1, 2, 3, 4, 5], list(range(2, 35)), list(range(DIM))]
PROBA = [0.1, 0.2, 0.3, 0.4]
HICS_ROWS = (1, 3, 130)


def mask():
    return _mask(DIM, FEATURES)


def data():
    """(fitted rows float32 [130, 37], query rows float32 [67, 37]): one draw of test_outlier_maha_cpu.raw_data, split."""
    Z = raw_data(N_FIT + N_QUERY, DIM, seed=11, constant=CONSTANT)
    return Z[:N_FIT].copy(), Z[N_FIT:].copy()


# ---- the public methods that take a matrix, beyond fit and decision_function --------------------------------------------
def _kneighbors(ens, Y):
    return ens.kneighbors(Y)


def _per_subspace(name):
    """method(Y, s) for the subspaces of width 5 and 33 (given order)"""
    return lambda ens, Y: [getattr(ens, name)(Y, s) for s in (1, 2)]


def _plain(name):
    return lambda ens, Y: getattr(ens, name)(Y)


QUERIES = {
    "SubspaceEnsemble": [("kneighbors", _kneighbors)],
    "SubspaceABOD": [("kneighbors", _kneighbors)],
    "SubspaceCOF": [("kneighbors", _kneighbors)],
    "SubspaceSOD": [("kneighbors", _kneighbors), ("reference_set", _plain("reference_set")),
                    ("relevant_features", lambda ens, Y: [ens.relevant_features(s, Y) for s in (1, 2)])],
    "SubspaceCBLOF": [("predict_clusters", _plain("predict_clusters"))],
    "SubspaceIForest": [("path_sums", _plain("path_sums"))],
    "SubspaceRSHash": [("cell_sums", _plain("cell_sums"))],
    "SubspaceKPCA": [("kernel_rows", _per_subspace("kernel_rows"))],
    "SubspaceLOCI": [("distance_rows", _per_subspace("distance_rows")), ("row_sums", _per_subspace("row_sums")),
                     ("best_radius", lambda ens, Y: ens.decision_function(Y, return_per_subspace=True, return_best_radius=True))],
    "SubspaceDIF": [("path_sums", _plain("path_sums")),
                    ("representation", lambda ens, Y: [ens.representation(Y, s, j) for s, j in ((1, 0), (2, 3))])],
    "SubspaceAutoEncoder": [("reconstruct", _per_subspace("reconstruct"))],
    "SubspaceDeepSVDD": [("embed", _per_subspace("embed"))],
}


class Case:
    """One detector configuration of the sweep.  flat: the subspaces (given order) whose scores are constant over the rows by
    the definition of the score, not by a fault; see the note where such a case is made.  The sweep asserts that they ARE
    constant, so a flat entry cannot hide a subspace that varies."""

    def __init__(self, id, cls, flat=(), **kw):
        self.id, self.cls, self.kw, self.flat = id, cls, kw, tuple(flat)
        self.queries = [] if kw.get("method") == "kde" else QUERIES.get(cls, [])

    def build(self):
        import vgan_amd
        return getattr(vgan_amd, self.cls)(mask(), PROBA, **self.kw)

    def __repr__(self):
        return self.id


KNN_KINDS = [("knn-largest", dict(method="knn", knn_method="largest")), ("knn-mean", dict(method="knn", knn_method="mean")),
             ("knn-median", dict(method="knn", knn_method="median")), ("lof", dict(method="lof")),
             ("kde", dict(method="kde", bandwidth="scott"))]
ENGINES = ("exact", "gram")
METRICS = [("manhattan", {}), ("chebyshev", {}), ("minkowski", dict(p=3.0)), ("cosine", {})]

CASES = [Case(f"{name}-{engine}", "SubspaceEnsemble", n_neighbors=5, engine=engine, **kw) for name, kw in KNN_KINDS for engine in ENGINES]
# The cosine distance between two rows of ONE feature of the same sign is 0, and every value of raw_data is about +100: the
# kNN distances of the width-1 subspace are all 0 by definition, in every layout.
CASES += [Case(f"{method}-{metric}", "SubspaceEnsemble", flat=(0,) if metric == "cosine" else (), method=method, n_neighbors=5,
               metric=metric, **kw) for metric, kw in METRICS for method in ("knn", "lof")]
CASES += [
    Case("abod", "SubspaceABOD", n_neighbors=6),
    Case("cof", "SubspaceCOF", n_neighbors=6),
    Case("cblof", "SubspaceCBLOF", n_clusters=3, init="random", seed=3, max_iter=30),
    Case("ecod", "SubspaceECOD"),
    Case("hbos", "SubspaceHBOS", n_bins=10),
    Case("loda", "SubspaceLODA", n_projections=9, n_bins=10, seed=3),
    Case("iforest", "SubspaceIForest", n_estimators=5, max_samples=64, seed=1),
    Case("rshash", "SubspaceRSHash", n_estimators=17, max_samples=128, seed=1),
    Case("inne", "SubspaceINNE", n_estimators=17, max_samples=16, seed=1),
    Case("mahalanobis", "SubspaceMahalanobis"),
    Case("mcd", "SubspaceMahalanobis", robust=True),
    Case("pca", "SubspacePCA"),
    Case("gmm", "SubspaceGMM", n_components=2, reg_covar=0.05, seed=3),
    Case("ocsvm", "SubspaceOCSVM", nu=0.3),
    Case("kpca", "SubspaceKPCA", n_components=3, max_samples=33),
    Case("sos", "SubspaceSOS", perplexity=4.5),
    Case("loci", "SubspaceLOCI", n_min=5, n_radii=4),
    Case("dif", "SubspaceDIF", n_representations=4, n_estimators=5, hidden=(16, 8), representation_dim=6, seed=21),
    Case("autoencoder", "SubspaceAutoEncoder", hidden=(5, 3), activation="tanh", epochs=3, batch_size=16, seed=7),
    Case("deepsvdd", "SubspaceDeepSVDD", hidden=(5, 3), activation="tanh", epochs=3, batch_size=16, seed=7),
    # SOD in ONE feature: the threshold T = alpha v_f / 1 is below v_f for alpha < 1, so no feature is relevant and the score
    # is 0 (r = 0 gives 0, step 6 of the class's definition), in every layout.
    Case("sod", "SubspaceSOD", flat=(0,), n_neighbors=8, ref_set=6, alpha=0.8),
]
CASE_IDS = [c.id for c in CASES]
assert len(set(CASE_IDS)) == len(CASES)
