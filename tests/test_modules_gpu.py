"""GPU tier of the operator-boundary tests: the modules of vgan_amd/modules.py -- what src/models/*.py re-exports and a user calls
unchanged -- on an MI355X, on every autograd path, against the float64 restatements and derived bounds of tests/modules_ref.py
(pinned without a GPU by tests/test_modules_cpu.py, which also shows that the check functions used here reject seven named
defects).  Run with ``-m gpu``.

  a. Linear chains through _LinearFn (Generator_big, Encoder, Decoder, Detector, hip_linear without bias): the module is bit-equal
     to the same chain built by hand from hip_linear calls, and every layer's y, dx, dW, db is within its own product bound of
     float64 on that layer's own device inputs; input with and without grad, a frozen weight, a frozen bias, a non-contiguous
     dy, gradients through both outputs of the Detector.
  b. the upper_softmax module, forward and backward, every element (no entry within 1e-5 / d of the snap threshold).
  c. vgan_rbf_multi_kernel_matrix and vgan_rbf_kernel_matrix called directly in sentinel buffers (class Guarded of
     test_gemm_kernels_gpu.py): NaN pads on the inputs, NaN-filled outputs with guard bands, ldk > m, lddk != ldk, the layouts
     "aligned", "shifted" and "oddld" (the last two run VEC = 1), n_kernels 1 to 8, dK given and dK = None (K the same bits),
     a planted pair of duplicate rows, the calibrated bandwidth and 1e-3 / 1e3 times it, a second launch with the same bits.
  d. RBF.forward / _RBFMatrixFn: K within the bound and bit-equal to the direct kernel call on the padded operand, Z.grad
     within its bound for a non-symmetric upstream G handed over as a transposed view (N = 64 runs vgan_mmd_backward's vector
     kernel, the others its scalar one), the calibrated and the frozen bandwidth.
  e. / f. MMDLossConstrained on equal and unequal row counts: loss and every gradient within its bound, for X only, Y only, both
     and neither, U with and without grad, tied column maxima, the fused and the general kernel, an upstream scale of 2.5.
  g. a second backward on a retained graph gives the same bits for every Function; two live graphs do not disturb each other.

Every case asserts its caps (modules_ref: a vacuous bound hides errors) from the reference alone before a device result is
looked at (a chain layer's reference is formed on that layer's own device inputs, so its caps are asserted before its outputs
are compared).  The bar is err <= bound, never a fraction of it.

Measured worst err / bound per family (one full run on an MI355X, what test_record_of_the_worst_ratios prints; records, not
bars): chain fwd 0.275, dx 0.380, dW 0.470, db 0.174 (the one-term products of the (1, 1, 5) chains, where a single float32
rounding is a quarter to a half of K 2u |a b|); softmax fwd 0.188, bwd 0.322; K 0.829 and dK 0.829, both at the bandwidth 1e-3
times the calibrated one with a single kernel, where an exponential just below 2^-126 comes back as zero against the 2^-126 term
of the bound -- at the calibrated bandwidth the worst is K 0.100 and dK 0.104 (vgan_rbf_kernel_matrix: 0.100), at 1e3 times it
0.035 and 0.059, through RBF.forward 0.063; Z.grad 0.042; loss 0.007; loss gradients 0.200 (dU, one rounding against 4u |dU|;
dX and dY stay below 0.05).  Every bit-equality above held on the device as stated.  The 99 tests take about four seconds.

Two defects came out of this file and its CPU tier and are fixed in vgan_amd/modules.py: _MMDLossUnequalFn.backward scaled its
saved dK/dL in place, so a second backward on a retained graph raised; and _LinearFn.backward (like every other hand-over) relied
on contiguous(), which keeps the stride-0 layout of an expanded [1, 1] gradient, so Encoder(1, d) on one row under
.sum().backward() was refused by the provider (test_linear_chain_modules[1-1-5-enc], mode "sum").
"""
import collections

import numpy as np
import pytest
import torch

import mmd_ref as mr
import modules_ref as ref
from cpu_ops import CpuOps
from test_gemm_kernels_gpu import Guarded, bits, ops, twice  # noqa: F401  (ops: the module-scoped HipOps fixture)
from vgan_amd import lib as vlib
from vgan_amd import modules as M

pytestmark = pytest.mark.gpu

WORST = collections.defaultdict(float)
DEV = "cuda"


def tiles_of(n, mode):
    return CpuOps.build_tiles(None, n, mode).numpy()  # the library's host-side table builder


def note(name, rec):
    print(name, " ".join(f"{k} {v:.3f}" for k, v in rec.items()))


# ================================================================================================ a. Linear chains
@pytest.mark.parametrize("kind", ref.CHAIN_KINDS)
@pytest.mark.parametrize("n,L,d", ref.CHAIN_SHAPES)
def test_linear_chain_modules(ops, kind, n, L, d):
    for mode in ref.CHAIN_MODES:
        run = ref.run_chain(M, kind, n, L, d, mode, DEV)
        ref.chain_caps(run.recs)
        note(f"{kind} ({n}, {L}, {d}) [{mode}]", ref.check_chain(run, WORST))


@pytest.mark.parametrize("n,L,d", ref.CHAIN_SHAPES)
def test_hip_linear_without_bias(ops, n, L, d):
    got, want, bound = ref.run_nobias(M, n, d, 2 * L, DEV)
    for g, w, b, fam in zip(got, want, bound, ("chain fwd", "chain dx", "chain dW")):
        ref.gr.cap_ok(b, w)
        WORST[fam] = max(WORST[fam], ref.ratio_of(g, w, b))


# ================================================================================================ b. upper_softmax
@pytest.mark.parametrize("n,d", ref.SOFTMAX_SHAPES)
def test_upper_softmax_module(ops, n, d):
    x = ref.softmax_logits(n, d)
    assert ref.snap_clear(x)
    g = ref.rng_for(f"softmax g/{n}/{d}").normal(size=(n, d)).astype(np.float32)
    note(f"upper_softmax ({n}, {d})", ref.check_softmax(ref.run_softmax(M, x, g, DEV), x, g, WORST))


# ================================================================================================ c. the RBF matrix kernels, direct
@pytest.mark.parametrize("index", range(len(ref.RBF_DIRECT)), ids=[f"{m}x{p}" for m, p in ref.RBF_DIRECT])
def test_rbf_multi_kernel_matrix_direct(ops, index):
    m, p = ref.RBF_DIRECT[index]
    Z, sq, bw = ref.rbf_operand(m, p, "direct")
    z64, s64 = Z.astype(np.float64), sq.astype(np.float64)
    off = ~np.eye(m, dtype=bool)
    for variant, kernel, factor in ref.direct_plan(index):
        mults = ref.multipliers(*kernel)
        bwf = np.float32(bw * np.float32(factor))
        r = ref.rbf_matrix_ref(z64, s64, bwf, mults)
        if factor != 1e-3:  # (the one factor that cannot keep the cap: module docstring of modules_ref)
            mr.cap_ok(r.bK, r.K, ref.CAP_FP32), mr.cap_ok(r.bdK, r.dK, ref.CAP_FP32)
        sh = ref.shift_for(variant)
        Zg = Guarded(m, p, ref.ld_for(p, variant), sh, data=Z)          # columns [p, ldz) and the guards hold NaN
        sqg, bwg = Guarded(1, m, shift=sh, data=sq), Guarded(1, 1, data=[bwf])
        Kg, dKg = Guarded(m, m, ref.ld_for(m, variant), sh), Guarded(m, m, ref.ld_for(m, variant, 8), sh)  # ldk > m, lddk != ldk
        K, dK = twice(lambda: ops.rbf_multi_kernel_matrix(Zg.t, sqg.vec, bwg.vec, mults, Kg.t, dKg.t), [(Kg, True), (dKg, True)], [Zg, sqg, bwg])
        Kg.reset(), dKg.reset()
        ops.rbf_multi_kernel_matrix(Zg.t, sqg.vec, bwg.vec, mults, Kg.t, None)
        torch.cuda.synchronize()
        assert np.array_equal(bits(Kg.check()), bits(K)), "K differs between dK given and dK = None"
        dKg.untouched()
        assert np.isfinite(K).all() and np.isfinite(dK).all()
        rk, rd = ref.ratio_of(K[0], r.K, r.bK), ref.ratio_of(dK[0], r.dK, r.bdK)
        if factor == 1e-3:
            zero = ref.underflown(r)
            assert not K[0][zero].any() and not dK[0][zero].any(), "an underflown element is not exactly zero"
            assert m == 1 or zero[off].mean() > 0.4
        WORST["K"], WORST["dK"] = max(WORST["K"], rk), max(WORST["dK"], rd)
        print(f"rbf multi ({m}, {p}) [{variant}] {kernel} bw x {factor:g}: worst err / bound K {rk:.3f} dK {rd:.3f}")


@pytest.mark.parametrize("m,p", ref.RBF_DIRECT)
def test_rbf_kernel_matrix_direct(ops, m, p):
    Z, sq, bw = ref.rbf_operand(m, p, "direct")
    alpha = np.float32(1.0 / bw)
    r = ref.rbf_single_ref(Z.astype(np.float64), sq.astype(np.float64), alpha)
    mr.cap_ok(r.bK, r.K, ref.CAP_FP32)
    results = []
    for variant in ref.VARIANTS:
        sh = ref.shift_for(variant)
        Zg, sqg = Guarded(m, p, ref.ld_for(p, variant), sh, data=Z), Guarded(1, m, shift=sh, data=sq)
        Kg = Guarded(m, m, ref.ld_for(m, variant), sh)
        (K,) = twice(lambda: ops.rbf_kernel_matrix(Zg.t, sqg.vec, float(alpha), Kg.t), [(Kg, True)], [Zg, sqg])
        assert (bits(np.diag(K[0])) == 0x3F800000).all(), "the diagonal is not exactly 1.0f"
        rk = ref.ratio_of(K[0], r.K, r.bK)
        WORST["K"] = max(WORST["K"], rk)
        results.append(K[0])
        print(f"rbf single ({m}, {p}) [{variant}]: worst err / bound {rk:.3f}")
    assert np.array_equal(bits(results[1]), bits(results[2])), "the two VEC = 1 layouts differ"


def test_rbf_matrix_kernels_refuse_bad_arguments(ops):
    """alpha <= 0, n_kernels 0 and 9: host-side argument checks that return VGAN_ERR_ARG before any launch
    (csrc/twosample.hip, the VGAN_CHECK_ARG lines of vgan_rbf_kernel_matrix and vgan_rbf_multi_kernel_matrix)."""
    Z, sq, bw = ref.rbf_operand(5, 4, "direct")
    Zg, sqg, bwg, Kg = Guarded(5, 4, data=Z), Guarded(1, 5, data=sq), Guarded(1, 1, data=[bw]), Guarded(5, 5)
    for alpha in (0.0, -1.0):
        with pytest.raises(vlib.VganHipError):
            ops.rbf_kernel_matrix(Zg.t, sqg.vec, alpha, Kg.t)
    for mults in ([], [1.0] * 9):
        with pytest.raises(vlib.VganHipError):
            ops.rbf_multi_kernel_matrix(Zg.t, sqg.vec, bwg.vec, mults, Kg.t, None)
    torch.cuda.synchronize()
    Kg.untouched()


# ================================================================================================ d. RBF.forward / _RBFMatrixFn
@pytest.mark.parametrize("N,p", ref.RBF_MODULE)
def test_rbf_module(ops, N, p):
    Z, _, _ = ref.rbf_operand(N, p, "module")
    Z2 = (Z * np.float32(0.5)).astype(np.float32)
    G = ref.rng_for(f"G/{N}/{p}").normal(size=(N, N)).astype(np.float32)
    z64, sq64 = ref.given_norms(ref.pad_rows(Z))
    want_bw, bw_bound = ref.bandwidth_ref(z64, sq64, ref.whole_table(tiles_of, N), N)
    for kernel in ref.KERNELS:
        for data in (Z, Z2):  # the caps, from the reference alone
            r0 = ref.rbf_module_ref(data, G, np.float32(want_bw), kernel)
            mr.cap_ok(r0.bK, r0.K, ref.CAP_FP32), mr.cap_ok(r0.bdK, r0.dK, ref.CAP_FP32), ref.gr.cap_ok(r0.bdZ, r0.dZ)
        got = ref.run_rbf(M, ops, Z, G, kernel, DEV)  # the first call calibrates
        assert abs(got.bw - want_bw) <= bw_bound
        rec = ref.check_rbf(got, ref.rbf_module_ref(Z, G, np.float32(got.bw), kernel), WORST)
        for k in (got.k, None):  # a second call on other data uses the frozen value; so does a bandwidth given as a float
            again = ref.run_rbf(M, ops, Z2, G, kernel, DEV, bandwidth=got.bw, k=k)
            assert again.bw == got.bw
            ref.check_rbf(again, ref.rbf_module_ref(Z2, G, np.float32(got.bw), kernel), WORST)
        note(f"RBF ({N}, {p}) {kernel}", rec)


# ================================================================================================ e. / f. MMDLossConstrained
def loss_case(name, nx, ny, nu, p, d, ties=False):
    X, Y, Um = ref.loss_data(name, nx, ny, nu, p, d, ties=ties)
    z64, sq64 = ref.given_norms(ref.pad_rows(X, Y))
    equal = nx == ny == nu
    for kernel in ref.LOSS_KERNELS if not ties else ref.LOSS_KERNELS[:1]:
        for need in ref.NEEDS:
            table = tiles_of(nx, 2 if need[0] else (1 if need[1] else 0)) if equal else ref.whole_table(tiles_of, nx + ny)
            want_bw, bw_bound = ref.bandwidth_ref(z64, sq64, table, nx if equal else nx + ny)
            ref.loss_caps(ref.mmd_loss_ref(X, Y, Um, ref.WEIGHT, np.float32(want_bw), kernel, gl=ref.GL, tiles_of=tiles_of))
            for u_grad in ((False, True) if need[0] == need[1] else (False,)):
                got = ref.run_loss(M, X, Y, Um, kernel, need, DEV, u_grad=u_grad, gl=ref.GL)  # a fresh kernel: calibrates
                assert abs(got.bw - want_bw) <= bw_bound
                r = ref.mmd_loss_ref(X, Y, Um, ref.WEIGHT, np.float32(got.bw), kernel, gl=ref.GL, tiles_of=tiles_of)
                note(f"loss {name} ({nx}, {ny}, {nu}, {p}, {d}) {kernel} need {need} U {u_grad}", ref.check_loss(got, r, need, u_grad, WORST))


@pytest.mark.parametrize("n,p,d", ref.EQUAL_CASES)
def test_mmd_loss_equal_rows(ops, n, p, d):
    loss_case("eq", n, n, n, p, d)


def test_mmd_loss_tied_column_maxima(ops):
    """U from upper_softmax: many exact ties at 1; the penalty gradient goes to the lowest row."""
    loss_case("ties", 33, 33, 33, 5, 9, ties=True)


@pytest.mark.parametrize("nx,ny,nu,p,d", ref.UNEQUAL_CASES)
def test_mmd_loss_unequal_rows(ops, nx, ny, nu, p, d):
    loss_case("uneq", nx, ny, nu, p, d)


# ================================================================================================ g. repeat and isolation
@pytest.mark.parametrize("kernel", [(5, 2.0), (3, 3.0)], ids=str)
@pytest.mark.parametrize("case", [("eq", 65, 65, 65, 33, 4), ("eq", 64, 64, 64, 4, 4), ("uneq", 33, 70, 12, 5, 7), ("uneq", 64, 2, 64, 4, 4)], ids=str)
def test_second_backward_of_the_loss(ops, case, kernel):
    name, nx, ny, nu, p, d = case
    ref.second_backward_of_the_loss(M, ref.loss_data(name, nx, ny, nu, p, d), kernel, DEV)


def test_second_backward_of_the_rbf_matrix_the_softmax_and_the_chain(ops):
    ref.second_backward_of_the_others(M, ops, DEV)


@pytest.mark.parametrize("case", [("eq", 33, 33, 33, 5, 9), ("uneq", 33, 70, 12, 5, 7)], ids=str)
def test_two_live_graphs_from_one_loss_fn(ops, case):
    name, nx, ny, nu, p, d = case
    ref.two_live_graphs(M, ref.loss_data(name, nx, ny, nu, p, d), DEV)


def test_record_of_the_worst_ratios():
    """Prints what this run measured (the figures of the module docstring come from such a run)."""
    for family in ref.FAMILIES:
        print(f"worst err / bound, {family}: {WORST[family]:.3f}")
    assert all(v <= 1.0 for v in WORST.values())
