"""Padded-row and shifted-base layouts on every outlier entry point that reads a raw data matrix (GPU tier, ``-m gpu``).

include/vgan_hip.h gives every such entry a leading dimension (ldx, ldq, ldr) and ops.py passes X.stride(0): a row stride
beyond d and a base that is not 16-byte aligned are legal inputs of the ABI.  This module runs every public detector class of
vgan_amd.outlier on such matrices and demands the bits of the contiguous run.

The lever   Every detector takes its device matrix from vgan_amd.outlier._device_matrix.  The module replaces that one
            function: the replacement copies the matrix into a Guarded allocation of tests/test_small_ops_gpu.py (NaN in
            every pad element between the rows and in a guard band on both sides, optionally a base shifted by one float),
            asserts the stride and the base alignment it produced, counts its calls and returns the [n, d] view.  The product
            code is unchanged.  hics.py converts on its own: vgan_hics_argsort_columns gets a direct call.
The sweep   outlier_layout_cases.CASES (every Subspace* class; SubspaceEnsemble in 18 combinations): fit(X),
            decision_function(Y, return_per_subspace=True) and the class's other public methods that take a matrix, under

                pair   fitted matrix                          query matrix
                base   contiguous                             contiguous
                A      ld 45 (1 mod 4), aligned base          ld 64 (multiple of 4, well beyond d), aligned base
                B      ld 44 (multiple of 4), base + 1 float  ld 49 (1 mod 4), base + 1 float

            at d = 37, 130 fitted and 67 query rows, subspaces of width 1, 5, 33 and 37 with unequal weights.  The two
            matrices of a pair never share a stride: a kernel that applies the wrong one reads NaN or the wrong row.
The bar     Bit equality with the base run, floats compared as uint32 / uint64: per_subspace_scores_, decision_scores_, the
            outputs of decision_function and of the other methods, and every published fitted attribute (every public name
            that ends in "_": trees, sorted columns, bin edges, histograms, supports, covariances, centres, labels,
            thresholds, score_center_ / score_scale_ ...).  A layout changes addresses only; each detector's own module
            asserts run-to-run bit identity, and test_base_layout_is_bit_reproducible restates that precondition here.  The
            independent float64 references stay in the detectors' own modules, which pin the contiguous run.
            No entry picks a kernel by the alignment or the stride of a raw matrix (the float4 accesses of csrc/outlier* and
            csrc/cluster.hip are on packed blocks, weights and LDS only), so the bar has no exception.
            Also: scores are finite and not constant over the rows of any subspace (but Case.flat, where the definition of
            the score makes them constant -- the cosine distance on one positive feature, SOD on one feature -- and they are
            asserted constant); the lever's call count shows that both matrices were padded; after each run
            every guarded input allocation is byte-identical to what it held: no kernel writes its input, its pads or its
            guard bands.
The record  Every ops.HipOps method is wrapped while the sweep runs; test_every_entry_was_reached prints, per entry of
            ENTRY_TABLE, the calls that carried a padded matrix inside a guarded allocation, and fails on an entry never
            reached that way.  tests/test_outlier_layout_cpu.py pins ENTRY_TABLE to the header.
The teeth   LAYOUT_FAULTS: three wrong views planted from the test side (each addresses only elements of the allocation it
            was cut from); the equalities above must fail for each.

Measured on an MI355X: the 127 tests of the module take 3.4 s by pytest's count, 1.3 s of it between the module's import and
its last test; the slowest case (the first, which loads the library) 0.26 s, every other below 0.25 s.  All 40 cases gave the
bits of their contiguous run on both pairs; the sweep reached 30 of the 31 entries, vgan_hics_argsort_columns by direct call.
"""
import collections
import time

import numpy as np
import pytest
import torch

import outlier_layout_cases as cases
from test_small_ops_gpu import Guarded, ld_for, shift_for

pytestmark = pytest.mark.gpu

D = cases.DIM
# (leading dimension, base shift in floats, ld mod 4) of the fitted and of the query matrix; None: contiguous
PAIRS = {
    "base": dict(fit=None, query=None),
    "A": dict(fit=(ld_for(D, "oddld"), shift_for("aligned"), 1), query=(ld_for(D, "aligned", 24), shift_for("aligned"), 0)),
    "B": dict(fit=(ld_for(D, "shifted"), shift_for("shifted"), 0), query=(ld_for(D, "oddld", 8), shift_for("shifted"), 1)),
}
assert all(p["fit"][0] != p["query"][0] and min(p["fit"][0], p["query"][0]) > D for k, p in PAIRS.items() if k != "base")

RECORD = collections.Counter()  # ops method -> calls of the sweep with a padded matrix of a guarded allocation
DIRECT = collections.Counter()  # the same, of the direct calls of this module
SWEPT = set()  # case ids that ran on a padded pair
BASE = {}  # case id -> the outputs of the contiguous run
T0 = time.time()


class Lever:
    """The replacement of vgan_amd.outlier._device_matrix."""

    def __init__(self, original):
        self.original, self.pair, self.role, self.direct = original, "base", "fit", False
        self.made, self.calls = [], collections.Counter()

    def begin(self, pair):
        self.pair, self.role, self.made, self.calls = pair, "fit", [], collections.Counter()

    def __call__(self, X, d):
        x = self.original(X, d)
        self.calls[self.role] += 1
        layout = PAIRS[self.pair][self.role]
        if layout is None:
            assert x.is_contiguous()
            return x
        ld, shift, mod4 = layout
        g = Guarded(x.shape[0], d, ld, shift=shift, data=x.cpu().numpy())
        assert g.t.shape == x.shape and g.t.stride() == (ld, 1) and ld > d and ld % 4 == mod4
        assert g.t.data_ptr() % 16 == (4 * shift) % 16 and torch.equal(g.t, x)
        self.made.append(g)
        return g.t

    def adopt(self, g):
        self.made.append(g)
        return g

    def owner(self, t):
        """the guarded allocation a padded matrix argument lies in, or None"""
        if not (isinstance(t, torch.Tensor) and t.is_cuda and t.dim() == 2 and t.stride(1) == 1 and t.stride(0) > t.shape[1]):
            return None
        base = t.untyped_storage().data_ptr()
        for g in self.made:
            if g.buf.untyped_storage().data_ptr() == base:
                return g
        return None

    def untouched(self):
        torch.cuda.synchronize()
        for g in self.made:
            g.untouched()


@pytest.fixture
def lever(monkeypatch):
    """_device_matrix replaced, every HipOps method recording its padded operands"""
    import vgan_amd.outlier as outlier
    from vgan_amd.ops import default_ops
    lv = Lever(outlier._device_matrix)
    monkeypatch.setattr(outlier, "_device_matrix", lv)
    ops = default_ops()
    for name in dir(ops):
        fn = getattr(ops, name)
        if name.startswith("_") or not callable(fn):
            continue

        def recording(*a, _fn=fn, _name=name, **kw):
            out = _fn(*a, **kw)  # a refused call raises here and is not counted
            if any(lv.owner(t) is not None for t in (*a, *kw.values())):
                (DIRECT if lv.direct else RECORD)[_name] += 1
            return out
        monkeypatch.setattr(ops, name, recording)
    lv.ops = ops
    return lv


@pytest.fixture(scope="module")
def XY():
    return cases.data()


# ---- running one case and comparing two runs ------------------------------------------------------------------------------
def published(ens):
    """every public name of the fitted detector that ends in "_": instance attributes and properties alike"""
    out = {}
    for name in sorted(set(dir(ens))):
        if name.startswith("_") or not name.endswith("_"):
            continue
        try:
            value = getattr(ens, name)
        except Exception as e:  # an attribute this configuration does not publish: the same in every layout
            value = f"raises {type(e).__name__}"
        if not callable(value):
            out[name] = value
    return out


def run_case(case, pair, lever, XY):
    X, Y = XY
    lever.begin(pair)
    ens = case.build()
    ens.fit(X)
    out = {"fit": published(ens)}
    lever.role = "query"
    out["decision_function"] = ens.decision_function(Y, return_per_subspace=True)
    for label, call in case.queries:
        out[label] = call(ens, Y)
    lever.untouched()
    assert lever.calls["fit"] >= 1 and lever.calls["query"] >= 1 + len(case.queries), dict(lever.calls)
    if pair != "base":
        want = lever.calls["fit"] + lever.calls["query"]
        assert len(lever.made) == want and all(g.ld > D for g in lever.made), "a matrix of the pair was not padded"
        assert {g.ld for g in lever.made} == {PAIRS[pair]["fit"][0], PAIRS[pair]["query"][0]}
        SWEPT.add(case.id)
    return out


def bits(v):
    if isinstance(v, torch.Tensor):
        v = v.detach().cpu().numpy()
    if isinstance(v, (float, np.floating)):
        v = np.asarray(v, dtype=np.float64)
    if isinstance(v, np.ndarray):
        if v.dtype == object:
            return [bits(e) for e in v.tolist()]
        v = np.ascontiguousarray(v)
        if v.dtype.kind == "f":
            return v.view({2: np.uint16, 4: np.uint32, 8: np.uint64}[v.dtype.itemsize])
        return v
    if isinstance(v, dict):
        return {k: bits(e) for k, e in v.items()}
    if isinstance(v, (list, tuple)):
        return [bits(e) for e in v]
    return v


def differences(a, b, path="out"):
    """[path] of every leaf at which two outputs differ in type, shape, dtype or bits"""
    a, b = bits(a), bits(b)
    if type(a) is not type(b):
        return [f"{path}: {type(a).__name__} against {type(b).__name__}"]
    if isinstance(a, dict):
        if a.keys() != b.keys():
            return [f"{path}: names {sorted(set(a) ^ set(b))}"]
        return [p for k in a for p in differences(a[k], b[k], f"{path}.{k}")]
    if isinstance(a, list):
        if len(a) != len(b):
            return [f"{path}: {len(a)} against {len(b)} items"]
        return [p for i, (x, y) in enumerate(zip(a, b)) for p in differences(x, y, f"{path}[{i}]")]
    if isinstance(a, np.ndarray):
        if a.shape != b.shape or a.dtype != b.dtype:
            return [f"{path}: {a.dtype}{a.shape} against {b.dtype}{b.shape}"]
        return [] if np.array_equal(a, b) else [f"{path}: {int((a != b).sum())} of {a.size} elements differ"]
    return [] if a == b else [f"{path}: {a!r} against {b!r}"]


def base_of(case, lever, XY):
    if case.id not in BASE:
        BASE[case.id] = run_case(case, "base", lever, XY)
    return BASE[case.id]


def check_scores(case, out):
    """finite, and not constant over the rows of any subspace but those of Case.flat"""
    for name, per in (("per_subspace_scores_", out["fit"]["per_subspace_scores_"]), ("decision_function", out["decision_function"][1])):
        assert per.dtype == np.float32 and per.shape[0] == 4 and np.isfinite(per).all(), (case.id, name)
        for s in range(4):
            assert (per[s].min() == per[s].max()) == (s in case.flat), (case.id, name, s, float(per[s].min()), float(per[s].max()))
    assert np.isfinite(out["fit"]["decision_scores_"]).all() and np.isfinite(out["decision_function"][0]).all()
    assert out["fit"]["decision_scores_"].shape == (cases.N_FIT,) and out["decision_function"][0].shape == (cases.N_QUERY,)


# ---- the sweep -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", cases.CASES, ids=cases.CASE_IDS)
def test_base_layout_is_bit_reproducible(case, lever, XY):
    """The precondition of the bar: two contiguous runs give the same bits; their scores are finite and not constant."""
    first = base_of(case, lever, XY)
    again = run_case(case, "base", lever, XY)
    assert not lever.made
    diff = differences(first, again)
    assert not diff, diff
    check_scores(case, first)


@pytest.mark.parametrize("pair", ["A", "B"])
@pytest.mark.parametrize("case", cases.CASES, ids=cases.CASE_IDS)
def test_padded_layouts_give_the_bits_of_the_contiguous_run(case, pair, lever, XY):
    want = base_of(case, lever, XY)
    got = run_case(case, pair, lever, XY)
    diff = differences(want, got)
    assert not diff, diff


# ---- direct calls where the lever does not reach ------------------------------------------------------------------------
def hics_argsort(lever, n, pair):
    """(order, rank) of vgan_hics_argsort_columns on tied_data [n, 37] in the fitted-matrix layout of the pair"""
    x = cases.tied_data(n, D, seed=n)
    lever.begin(pair)
    lever.direct = True
    layout = PAIRS[pair]["fit"]
    if layout is None:
        X = torch.as_tensor(x, device="cuda")
    else:
        g = lever.adopt(Guarded(n, D, layout[0], shift=layout[1], data=x))
        assert g.t.stride(0) == layout[0] and g.t.data_ptr() % 16 == (4 * layout[1]) % 16
        X = g.t
    keys = torch.empty(D, 1 << (n - 1).bit_length(), dtype=torch.int64, device="cuda")
    order = torch.full((D, n), -1, dtype=torch.int32, device="cuda")
    rank = torch.full((D, n), -1, dtype=torch.int32, device="cuda")
    lever.ops.hics_argsort_columns(X, keys, order, rank)
    lever.untouched()
    lever.direct = False
    return order.cpu().numpy(), rank.cpu().numpy()


@pytest.mark.parametrize("n", cases.HICS_ROWS)
def test_hics_argsort_columns_on_padded_layouts(n, lever):
    """order and rank bit-equal to the contiguous call.  The entry's contract is 2 <= n: a single row is refused with the
    bad-argument status before any launch, and must be refused alike, outputs and input untouched, in every layout."""
    if n < 2:
        from vgan_amd.lib import VganHipError
        for pair in ("base", "A", "B"):
            with pytest.raises(VganHipError, match="bad argument"):
                hics_argsort(lever, n, pair)
            lever.untouched()
        return
    order, rank = hics_argsort(lever, n, "base")
    assert np.array_equal(np.sort(order, axis=1), np.tile(np.arange(n, dtype=np.int32), (D, 1)))  # a permutation per column
    assert np.array_equal(np.take_along_axis(rank, order, axis=1), np.tile(np.arange(n, dtype=np.int32), (D, 1)))
    for pair in ("A", "B"):
        got_order, got_rank = hics_argsort(lever, n, pair)
        assert np.array_equal(got_order, order) and np.array_equal(got_rank, rank), pair


# ---- proof that the harness has teeth -------------------------------------------------------------------------------------
def _inside(lever, t, view_elems):
    """the wrong view [offset, offset + view_elems) lies in the rows of the allocation t was cut from"""
    g = lever.owner(t)
    assert g is not None
    assert g.start <= t.storage_offset() and t.storage_offset() + view_elems <= g.start + g.rows * g.ld, "the planted view leaves its buffer"


def fault_fitted_ld_is_d(lever, X, *rest, _call):
    """ECOD's sort reads the fitted matrix with ld = d instead of its stride"""
    n, d = X.shape
    _inside(lever, X, n * d)
    return _call(X.as_strided((n, d), (d, 1), X.storage_offset()), *rest)


def fault_query_with_fitted_stride(lever, Xq, *rest, _call):
    """the Mahalanobis scores read the query matrix with the fitted matrix's stride"""
    n, d = Xq.shape
    ld = PAIRS[lever.pair]["fit"][0]
    _inside(lever, Xq, (n - 1) * ld + d)
    return _call(Xq.as_strided((n, d), (ld, 1), Xq.storage_offset()), *rest)


def fault_feature_index_d(lever, Xq, *rest, _call):
    """HBOS reads features 1 .. d: its last feature index is d, the first pad element of every row.  (HBOS takes no feature
    list, its table is 0 .. d - 1; the view moved by one column is that table moved by one.)"""
    n, d = Xq.shape
    assert Xq.stride(0) > d
    _inside(lever, Xq, (n - 1) * Xq.stride(0) + d + 1)
    return _call(Xq.as_strided((n, d), Xq.stride(), Xq.storage_offset() + 1), *rest)


LAYOUT_FAULTS = {"fitted matrix read with ld = d": ("ecod", "ecod_sort_columns", fault_fitted_ld_is_d),
                 "query matrix read with the fitted stride": ("mahalanobis", "maha_scores", fault_query_with_fitted_stride),
                 "feature index d, one past the row": ("hbos", "hbos_scores", fault_feature_index_d)}


@pytest.mark.parametrize("pair", ["A", "B"])
@pytest.mark.parametrize("fault", list(LAYOUT_FAULTS))
def test_planted_layout_fault_is_detected(fault, pair, lever, XY, monkeypatch, capsys):
    case_id, method, plant = LAYOUT_FAULTS[fault]
    case = cases.CASES[cases.CASE_IDS.index(case_id)]
    want = base_of(case, lever, XY)
    call, planted = getattr(lever.ops, method), collections.Counter()

    def wrong(X, *rest, **kw):
        assert not kw
        planted[method] += 1
        return plant(lever, X, *rest, _call=call)
    monkeypatch.setattr(lever.ops, method, wrong)
    swept, record = set(SWEPT), RECORD.copy()
    got = run_case(case, pair, lever, XY)  # reads NaN or wrong rows inside its own buffer; writes no input (checked there)
    SWEPT.intersection_update(swept)  # a run with a planted fault is no sweep of its case and adds nothing to the record
    RECORD.clear()
    RECORD.update(record)
    diff = differences(want, got)
    assert planted[method] and diff, f"planted fault not detected: {fault}"
    with capsys.disabled():
        print(f"\nplanted layout fault, pair {pair}: {fault}: detected ({len(diff)} outputs differ, e.g. {diff[0]})")


# ---- proof that nothing was skipped ---------------------------------------------------------------------------------------
def test_every_entry_was_reached(lever, XY, capsys):
    """Every entry of ENTRY_TABLE was called with a padded matrix of a guarded allocation, by the sweep or by a direct call.
    Run alone (-k), this test first runs on pair A whatever case the session has not swept."""
    for case in cases.CASES:
        if case.id not in SWEPT:
            run_case(case, "A", lever, XY)
    if not DIRECT["hics_argsort_columns"]:
        hics_argsort(lever, 3, "A")
    rows = [(name, RECORD[name[len("vgan_"):]], DIRECT[name[len("vgan_"):]]) for name in cases.ENTRY_TABLE]
    with capsys.disabled():
        print("\nentry: calls with a padded operand (sweep, direct)")
        for name, swept, direct in rows:
            print(f"  {name}: {swept}, {direct}")
        print(f"  {sum(1 for _, s, _ in rows if s)} of {len(rows)} entries reached by the sweep; direct calls only: "
              f"{[n for n, s, dct in rows if not s and dct]}; wall time of the module so far {time.time() - T0:.1f} s")
    missed = [name for name, swept, direct in rows if not swept and not direct]
    assert not missed, f"no padded matrix reached {missed}"
    assert SWEPT == set(cases.CASE_IDS)
