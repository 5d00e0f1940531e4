"""CPU companion of tests/test_outlier_layout_gpu.py: proof that its sweep skips nothing, without a device.

  * The entry table the GPU module commits to cover (outlier_layout_cases.ENTRY_TABLE) equals the set of prototypes of
    include/vgan_hip.h, from vgan_outlier_pack to the end of the file, that take a raw matrix through a leading dimension
    named ldx, ldq or ldr.  A new such entry point fails this module until it is listed, and the GPU module then fails until
    a padded matrix reaches it.
  * The detector list of the sweep equals the Subspace* classes vgan_amd exports, SubspaceEnsemble runs in every
    combination the sweep promises, and every case constructs (constructors touch no device).
"""
import os
import re

import numpy as np

from conftest import REPO
import outlier_layout_cases as cases

LD_NAMES = ("ldx", "ldq", "ldr")


def raw_matrix_entries():
    """[name] in header order: the prototypes from vgan_outlier_pack on with a parameter named ldx, ldq or ldr"""
    text = open(os.path.join(REPO, "include", "vgan_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    text = re.sub(r"//[^\n]*", "", text)
    start = re.search(r"\bvgan_outlier_pack\s*\(", text).start()
    out = []
    for m in re.finditer(r"\b(vgan_[a-z0-9_]+)\s*\(([^;{}]*?)\)\s*;", text[start:], flags=re.S):
        params = [re.findall(r"[A-Za-z_][A-Za-z0-9_]*", p)[-1] for p in m.group(2).split(",") if re.search(r"[A-Za-z_]", p)]
        if any(p in LD_NAMES for p in params):
            out.append(m.group(1))
    return out


def test_entry_table_is_the_headers_raw_matrix_surface():
    got = raw_matrix_entries()
    assert len(got) == len(set(got)) and len(cases.ENTRY_TABLE) == len(set(cases.ENTRY_TABLE))
    assert "vgan_outlier_pack" in got and "vgan_hics_argsort_columns" in got  # the first and the last section were parsed
    missing, stale = sorted(set(got) - set(cases.ENTRY_TABLE)), sorted(set(cases.ENTRY_TABLE) - set(got))
    assert not missing, f"entries that take a raw matrix but are not in ENTRY_TABLE (no padded layout reaches them): {missing}"
    assert not stale, f"ENTRY_TABLE names no prototype with ldx / ldq / ldr: {stale}"


def test_every_entry_has_its_ops_method():
    """the GPU module records ops.HipOps calls by method name: an entry's method is its name without the prefix"""
    from vgan_amd.ops import HipOps
    for name in cases.ENTRY_TABLE:
        assert callable(getattr(HipOps, name[len("vgan_"):], None)), name


def test_detector_list_is_the_exported_one():
    import vgan_amd
    exported = {n for n in vgan_amd.__all__ if n.startswith("Subspace")}
    assert exported == {n for n in dir(vgan_amd) if n.startswith("Subspace")}
    swept = {c.cls for c in cases.CASES}
    assert swept == exported, (sorted(exported - swept), sorted(swept - exported))


def test_ensemble_and_mahalanobis_combinations_are_complete():
    ens = [c for c in cases.CASES if c.cls == "SubspaceEnsemble"]
    kinds = {(c.kw["method"], c.kw.get("knn_method", "largest") if c.kw["method"] == "knn" else None, c.kw.get("engine"),
              c.kw.get("metric", "euclidean")) for c in ens}
    want = {(m, k, e, "euclidean") for m, k in (("knn", "largest"), ("knn", "mean"), ("knn", "median"), ("lof", None), ("kde", None))
            for e in ("exact", "gram")}
    want |= {(m, "largest" if m == "knn" else None, None, metric) for m in ("knn", "lof")
             for metric in ("manhattan", "chebyshev", "minkowski", "cosine")}
    assert kinds == want and len(ens) == len(want)
    assert {bool(c.kw.get("robust")) for c in cases.CASES if c.cls == "SubspaceMahalanobis"} == {False, True}


def test_every_case_constructs_and_names_real_methods():
    for c in cases.CASES:
        ens = c.build()
        assert type(ens).__name__ == c.cls and ens.plan.count == 4 and ens.plan.d == cases.DIM
        for name in ("fit", "decision_function"):
            assert callable(getattr(ens, name))
    import vgan_amd
    for cls, queries in cases.QUERIES.items():
        assert any(c.cls == cls for c in cases.CASES), cls
        for label, _ in queries:
            assert label == "best_radius" or callable(getattr(getattr(vgan_amd, cls), label)), (cls, label)


def test_shapes_and_data_are_the_issues():
    m = cases.mask()
    assert m.shape == (4, cases.DIM) and m.sum(axis=1).tolist() == [1, 5, 33, 37] and cases.DIM % 4 != 0
    assert len(set(cases.PROBA)) == 4 and abs(sum(cases.PROBA) - 1.0) < 1e-12
    X, Y = cases.data()
    assert X.shape == (130, 37) and Y.shape == (67, 37) and X.dtype == Y.dtype == np.float32
    for Z in (X, Y):
        const = [f for f in range(cases.DIM) if Z[:, f].min() == Z[:, f].max()]
        assert const == [cases.CONSTANT]
    assert [cases.CONSTANT in f for f in cases.FEATURES] == [False, True, True, True]
    assert cases.HICS_ROWS == (1, 3, 130)
