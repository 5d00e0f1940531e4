"""The reference, the bounds and the case tables of tests/gemm_ref.py, checked without a GPU: the float64 reference agrees with exact
rational arithmetic and the float32 slab sum with a Python loop; every bound of every case of the GPU tier has teeth
(max(bound) < the smallest term) and respects its cap; mutants of the reference -- the last term dropped, the K tail past the
last whole K tile dropped, an operand row or column shifted by one, the bias of the neighbouring column, a slab left out, a split
slice left out -- all violate the bound, at every element they touch; and the library's own host-side path queries
(vgan_*_path, include/vgan_hip.h) name, for every row of the tables and every layout variant, the kernel the row expects, and
every code of the four enums is reached by some row (the in-launch K split, which tests/test_chain_ksplit_gpu.py owns, aside)."""
import ctypes
import os
import re
from fractions import Fraction

import numpy as np
import pytest

import gemm_ref as ref
from conftest import REPO
from vgan_amd import lib

DATA = {"fwd": ref.fwd_data, "bwi": ref.bwi_data, "bwp": ref.bwp_data}
LINEAR_CASES = ref.FWD_CASES + ref.BWI_CASES + ref.BWP_CASES
_cache = {}


def data_of(c):
    if c.name not in _cache:
        _cache[c.name] = ref.grp_data(c) if c.family == "grp" else DATA[c.family](c)
    return _cache[c.name]


def products_of(c):
    """[(A64 [M, K], B64 [K, N], offset [N] or None, want, bound, smallest term, K tile)] of a case's products"""
    d = data_of(c)
    if c.family == "grp":
        return [(q.a, q.b, None, q.want, q.bound, q.floor, 32 if e == "T64" else 128) for q, e in zip(d, c.engines)]
    off = d.b.astype(np.float64) if c.family == "fwd" and c.bias else None
    return [(d.A, d.B, off, d.want, d.bound, c.lo ** 2, c.ktile)]


# ---- the enums of the header and their names in the binding ---------------------------------------------------------------------
def header_enum(name):
    text = open(os.path.join(REPO, "include", "vgan_hip.h")).read()
    body = re.search(r"enum %s \{(.*?)\};" % name, text, flags=re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    return [(m.group(1), int(m.group(2))) for m in re.finditer(r"(VGAN_[A-Z0-9_]+) = (\d+)", body)]


@pytest.mark.parametrize("enum,prefix,names", [
    ("vgan_linear_forward_path_code", "VGAN_LINEAR_FORWARD_", lib.LINEAR_FORWARD_PATHS),
    ("vgan_linear_backward_input_path_code", "VGAN_LINEAR_BACKWARD_INPUT_", lib.LINEAR_BACKWARD_INPUT_PATHS),
    ("vgan_linear_backward_params_path_code", "VGAN_LINEAR_BACKWARD_PARAMS_", lib.LINEAR_BACKWARD_PARAMS_PATHS),
    ("vgan_gemm_grouped_path_code", "VGAN_GEMM_GROUPED_", lib.GEMM_GROUPED_PATHS), ("vgan_gemm_engine", "VGAN_GEMM_ENGINE_", lib.GEMM_ENGINES)])
def test_binding_names_the_header_enums(enum, prefix, names):
    entries = header_enum(enum)
    if entries[-1][0].endswith("_PATHS"):
        assert entries.pop() == (prefix + "PATHS", len(names))
    assert entries == [(prefix + n, i) for i, n in enumerate(names)]


# ---- the reference --------------------------------------------------------------------------------------------------------------
def exact_dot(a, b):
    return sum((Fraction(float(x)) * Fraction(float(y)) for x, y in zip(a, b)), Fraction(0))


@pytest.mark.parametrize("case", [ref.FWD_CASES[9], ref.FWD_CASES[36], ref.BWI_CASES[18], ref.BWP_CASES[9], ref.BWP_CASES[52], ref.GRP_FOUR[1],
                                  ref.GRP_NTNT[4]], ids=repr)
def test_reference_is_the_exact_product_of_the_float32_operands(case):
    for A, B, off, want, bound, floor, ktile in products_of(case):
        K = A.shape[1]
        for i, j in {(0, 0), (A.shape[0] - 1, B.shape[1] - 1), (A.shape[0] // 2, B.shape[1] // 3)}:
            exact = exact_dot(A[i], B[:, j]) + (Fraction(float(off[j])) if off is not None else 0)
            # a float64 product sum of K terms: K 2^-53 sum |a b| to first order, doubled
            assert abs(Fraction(float(want[i, j])) - exact) <= K * 2.0 ** -52 * float(np.abs(A[i]) @ np.abs(B[:, j]) + 1.0)
    d = data_of(case)
    if case.family == "fwd":  # the product form really is x . W^T of the float32 operands, slabs summed in float32 first
        assert np.array_equal(d.A, ref.slab_sum32(d.xs).astype(np.float64)) and np.array_equal(d.B, d.W.astype(np.float64).T)
    if case.family == "bwp":
        assert np.array_equal(d.A, d.dy.astype(np.float64).T) and np.array_equal(d.B, ref.slab_sum32(d.xs).astype(np.float64))
        for i in (0, case.out - 1):
            assert abs(Fraction(float(d.want_db[i])) - sum(Fraction(float(v)) for v in d.dy[:, i])) <= case.n * 2.0 ** -52 * case.n
    if case.family == "grp" and case.problems[0].kind == "NT2":  # (A . B^T) . D^T, all in float64
        q = d[0]
        a, b, dd = q.A.astype(np.float64), q.B.astype(np.float64), q.D.astype(np.float64)
        np.testing.assert_allclose(q.want, (a @ b.T) @ dd.T, rtol=1e-13)
        i, j = 3, 5
        exact = sum((exact_dot(a[i], b[h]) * Fraction(float(dd[j, h])) for h in range(b.shape[0])), Fraction(0))
        assert abs(Fraction(float(q.want[i, j])) - exact) <= 2.0 ** -40 * abs(exact)


def test_slab_sum_is_the_float32_ascending_loop():
    rng = np.random.default_rng(5)
    slabs = ref.draw_slabs(rng, (7, 9), 3)
    got = ref.slab_sum32(slabs)
    assert got.dtype == np.float32
    for i in range(7):
        for j in range(9):
            acc = np.float32(slabs[0, i, j])
            for s in (1, 2):
                acc = np.float32(acc + np.float32(slabs[s, i, j]))
            assert acc == got[i, j]
    # ascending order matters: some element of the other order differs, so the restatement pins the order too
    big = ref.draw_slabs(np.random.default_rng(6), (64, 64), 3)
    assert (ref.slab_sum32(big) != ref.slab_sum32(big[::-1])).any()
    assert (np.abs(ref.slab_sum32(big)) >= 0.5 * (1 - 2.0 ** -20)).all() and (np.abs(ref.slab_sum32(big)) <= 1.0 + 2.0 ** -20).all()


def test_split_rows_and_slices():
    assert ref.split_rows(5, 3) == [(0, 4), (4, 5), (5, 5)]
    assert ref.split_rows(8, 8) == [(0, 4), (4, 8)] + [(8, 8)] * 6
    assert ref.split_rows(100, 3) == [(0, 36), (36, 72), (72, 100)]
    assert [b - a for a, b in ref.split_rows(97, 8)] == [16] * 6 + [1, 0]
    assert ref.splitk_slices(100, 2) == [(0, 64), (64, 100)] and ref.splitk_slices(133, 3) == [(0, 64), (64, 128), (128, 133)]
    assert ref.splitk_slices(100, 3) is None and ref.splitk_slices(64, 3) is None


# ---- every bound has teeth and respects its cap ---------------------------------------------------------------------------------
@pytest.mark.parametrize("case", LINEAR_CASES + ref.GRP_CASES, ids=repr)
def test_bounds_have_teeth_and_respect_the_cap(case):
    for A, B, off, want, bound, floor, ktile in products_of(case):
        assert min(np.abs(A).min() * np.abs(B).min(), floor) >= floor * (1 - 1e-6)  # the smallest term really is that large
        ref.teeth(bound, case.lo, floor)
        ref.cap_ok(bound, want)
    if case.family == "bwp" and case.db:
        d = data_of(case)
        ref.teeth(d.bound_db, case.lo, case.lo)
        ref.cap_ok(d.bound_db, d.want_db)


# ---- mutants --------------------------------------------------------------------------------------------------------------------
def caught(mutant, want, bound):
    return np.abs(mutant - want) > bound


def plus(prod, off):
    return prod if off is None else prod + off


@pytest.mark.parametrize("case", LINEAR_CASES + ref.GRP_CASES, ids=repr)
def test_mutants_of_the_product_violate_the_bound(case):
    for A, B, off, want, bound, floor, ktile in products_of(case):
        M, K = A.shape
        N = B.shape[1]
        assert caught(plus(A[:, :K - 1] @ B[:K - 1], off), want, bound).all(), "last term dropped"
        assert caught(plus(A[:, 1:] @ B[1:], off), want, bound).all(), "first term dropped"
        assert caught(plus(A @ B + A[:, K - 1:] @ B[K - 1:], off), want, bound).all(), "last term doubled"
        kt = K // ktile * ktile
        if 0 < kt < K:
            assert caught(plus(A[:, :kt] @ B[:kt], off), want, bound).all(), "K tail dropped"
        if M > 1:
            i = M // 2
            A2 = A.copy()
            A2[i] = A[i + 1 if i + 1 < M else i - 1]
            assert caught(plus(A2 @ B, off), want, bound)[i].all(), "operand row shifted"
        if N > 1:
            j = N // 2
            B2 = B.copy()
            B2[:, j] = B[:, j + 1 if j + 1 < N else j - 1]
            assert caught(plus(A @ B2, off), want, bound)[:, j].all(), "operand column shifted"
        if off is not None and N > 1:
            assert caught(A @ B + np.roll(off, 1), want, bound).all(), "bias of the neighbouring column"
            assert caught(A @ B, want, bound).all(), "bias left out"


@pytest.mark.parametrize("case", [c for c in LINEAR_CASES if getattr(c, "nslabs", 1) > 1], ids=repr)
def test_a_slab_left_out_violates_the_bound(case):
    d = data_of(case)
    for s in range(case.nslabs):
        x = ref.slab_sum32(np.delete(d.xs, s, axis=0)).astype(np.float64)
        if case.family == "fwd":
            mutant = plus(x @ d.B, d.b.astype(np.float64) if case.bias else None)
        else:
            mutant = d.A @ x
        assert caught(mutant, d.want, d.bound).all(), s


@pytest.mark.parametrize("case", [c for c in ref.BWP_CASES if c.splits > 1] + ref.GRP_SPLITK, ids=repr)
def test_a_split_slice_left_out_violates_the_bound(case):
    if case.family == "bwp":
        d = data_of(case)
        jobs = [(d.A, d.B, d.want, d.bound, ref.split_rows(case.n, case.splits))]
        assert any(a == b for a, b in jobs[0][4]) == (case.n <= 8 or case.splits == 8)  # the tables do hold empty slices
    else:
        jobs = [(q.a, q.b, q.want, q.bound, ref.splitk_slices(p.k, p.splitk)) for q, p in zip(data_of(case), case.problems) if p.splitk > 1]
    for A, B, want, bound, slices in jobs:
        assert slices[0][0] == 0 and slices[-1][1] == A.shape[1] and all(a[1] == b[0] for a, b in zip(slices, slices[1:]))
        for k0, k1 in slices:
            if k1 > k0:
                keep = np.r_[0:k0, k1:A.shape[1]]
                assert caught(A[:, keep] @ B[keep], want, bound).all(), (k0, k1)
        if case.family == "bwp" and case.db:
            d = data_of(case)
            for k0, k1 in slices:
                if k1 == k0 + 1:  # (a longer slice of db sums randomly signed terms: not certain, see gemm_ref)
                    assert caught(d.want_db - A[:, k0:k1].sum(1), d.want_db, d.bound_db).all()


@pytest.mark.parametrize("case", [c for c in ref.BWP_CASES if c.db], ids=repr)
def test_mutants_of_db_violate_the_bound(case):
    d = data_of(case)
    assert caught(d.A[:, :-1].sum(1), d.want_db, d.bound_db).all(), "last row dropped"
    if case.out > 1 and case.n == 1:
        assert caught(np.roll(d.want_db, 1), d.want_db, d.bound_db).all(), "db of the neighbouring column"


# ---- path coverage, by the library's own queries --------------------------------------------------------------------------------
def linear_paths(cases, query, names):
    seen = set()
    loaded = lib.load()
    for c in cases:
        codes = {}
        for variant in ref.VARIANTS:
            code = query(loaded, c, variant)
            assert code >= 0, (c.name, variant, loaded.vgan_last_error())
            codes[variant] = names[code]
            assert names[code] == ref.expected(c.path, variant), (c.name, variant, names[code])
        seen.update(codes.values())
    return seen


def test_forward_table_reaches_every_kernel():
    assert linear_paths(ref.FWD_CASES, ref.fwd_path, lib.LINEAR_FORWARD_PATHS) == set(lib.LINEAR_FORWARD_PATHS)


def test_backward_input_table_reaches_every_kernel():
    assert linear_paths(ref.BWI_CASES, ref.bwi_path, lib.LINEAR_BACKWARD_INPUT_PATHS) == set(lib.LINEAR_BACKWARD_INPUT_PATHS)


def test_backward_params_table_reaches_every_kernel():
    assert linear_paths(ref.BWP_CASES, ref.bwp_path, lib.LINEAR_BACKWARD_PARAMS_PATHS) == set(lib.LINEAR_BACKWARD_PARAMS_PATHS)


def test_grouped_tables_reach_every_launch_and_engine():
    seen, kinds = set(), set()
    for c in ref.GRP_CASES:
        for variant in ref.VARIANTS:
            code, engine = ref.grp_path(lib, c, variant)
            assert code >= 0, (c.name, variant, lib.load().vgan_last_error())
            got = [lib.GEMM_ENGINES[e] for e in engine]
            assert lib.GEMM_GROUPED_PATHS[code] == ref.expected(c.path, variant), (c.name, variant, lib.GEMM_GROUPED_PATHS[code])
            assert got == (c.engines if variant == "aligned" else c.scalar_engines), (c.name, variant, got)
            seen.add(lib.GEMM_GROUPED_PATHS[code])
            kinds.update((p.kind, e, ref.vec_of(lib.GEMM_GROUPED_PATHS[code]) if e != "KS16" else 4) for p, e in zip(c.problems, got))
    # the in-launch K split has its own tests (test_chain_ksplit_gpu.py)
    assert seen == set(lib.GEMM_GROUPED_PATHS) - {"KS16_SPLIT"}
    # every kind on every engine at both vector widths (16 waves: vector only; NT_NT: 64 x 64 only)
    want = {(k, e, v) for k in ref.KINDS for e in ("T64", "KS4") for v in (1, 4)} | {(k, "KS16", 4) for k in ref.KINDS}
    assert want | {("NT2", "T64", 1), ("NT2", "T64", 4)} == kinds


def test_grouped_query_names_the_in_launch_split_and_refuses_what_the_launch_refuses():
    loaded = lib.load()
    c = ref.GRP_FOUR[2]  # the 16-wave group
    arr = ref.grp_fake_problems(lib, c, "aligned")
    engine = (ctypes.c_int32 * 4)()
    kparts = (ctypes.c_int32 * 4)(1, 2, 4, 1)
    assert lib.GEMM_GROUPED_PATHS[loaded.vgan_gemm_grouped_path(arr, 4, None, kparts, engine)] == "KS16_SPLIT"
    assert [lib.GEMM_ENGINES[e] for e in engine] == ["KS16"] * 4
    assert lib.GEMM_GROUPED_PATHS[loaded.vgan_gemm_grouped_path(arr, 4, None, (ctypes.c_int32 * 4)(1, 1, 1, 1), None)] == "KS16"
    assert loaded.vgan_gemm_grouped_path(ref.grp_fake_problems(lib, c, "shifted"), 4, None, kparts, engine) < 0  # no 16-wave launch: no split
    assert loaded.vgan_gemm_grouped_path(arr, 0, None, None, None) < 0 and loaded.vgan_gemm_grouped_path(None, 1, None, None, None) < 0
    assert loaded.vgan_gemm_grouped_path(arr, 5, None, None, None) < 0
    for p in ref.GRP_SPLITK_REFUSED:  # a K slice would be empty
        assert ref.splitk_slices(p.k, p.splitk) is None
        code, _ = ref.grp_path(lib, ref.grp([p], "T256_V4", ["T64"]), "aligned")
        assert code < 0 and b"bad argument" in loaded.vgan_last_error()
    # the optimiser epilogue does not go with a split problem
    bad = ref.grp([ref.gp("NN", 8, 8, 100, splitk=2)], "T256_V4_EPI", ["T64"], epi=True)
    assert ref.grp_path(lib, bad, "aligned")[0] < 0


def test_linear_queries_refuse_what_the_entry_points_refuse():
    loaded = lib.load()
    a = ref.fake(0, "aligned")
    assert loaded.vgan_linear_forward_path(None, 8, 1, 0, a, 8, None, a, 8, 4, 4, 4) < 0
    assert loaded.vgan_linear_forward_path(a, 3, 1, 0, a, 8, None, a, 8, 4, 4, 4) < 0  # ldx < in
    assert loaded.vgan_linear_forward_path(a, 8, 0, 0, a, 8, None, a, 8, 4, 4, 4) < 0  # no slab
    assert loaded.vgan_linear_forward_path(a, 8, 1, 0, a, 8, None, a, 8, 4, 4, 4) == lib.LINEAR_FORWARD_PATHS.index("T64_V4")
    assert loaded.vgan_linear_backward_input_path(a, 8, a, 8, None, 8, 4, 4, 4) < 0
    assert loaded.vgan_linear_backward_input_path(a, 8, a, 3, a, 8, 4, 4, 4) < 0
    assert loaded.vgan_linear_backward_params_path(a, 8, a, 8, 1, 0, a, 8, None, 4, 4, 4, 65, 64) < 0  # more than 64 slices
    assert loaded.vgan_linear_backward_params_path(a, 8, a, 8, 1, 0, a, 8, None, 4, 4, 4, 2, 0) < 0   # slices without a slab stride
    assert b"bad argument" in loaded.vgan_last_error()
    assert loaded.vgan_linear_backward_params_path(a, 8, a, 8, 1, 0, a, 8, None, 4, 4, 4, 1, 0) == lib.LINEAR_BACKWARD_PARAMS_PATHS.index("T64_V4")
