"""CPU tier of the operator-boundary tests (vgan_amd/modules.py): no GPU needed.

  * pins tests/modules_ref.py to things that are not this project's kernels: oracle/torch_port (PortRBF, port_mmd_loss,
    port_upper_softmax under float64 autograd) and fixture F7 (written by the reference) for unequal row counts;
  * runs the REAL modules over tests/cpu_ops.CpuOps (vgan_amd.modules.default_ops replaced per test with monkeypatch) through
    every case table of the GPU tier and the GPU tier's own check functions, at a float64 provider's tolerance (half a bound);
  * pins the host logic: which gradients arrive, the upstream scale, a second backward on a retained graph (all three MMD
    paths and the chain), two live graphs from one loss_fn, the frozen-bandwidth hand-over, the re-exports of src/models;
  * teeth: named mutations of the provider, each rejected by the GPU tier's check functions wherever it can bite;
  * every cap of modules_ref on every case, from the reference alone.
"""
import collections

import numpy as np
import pytest
import torch

import mmd_ref as mr
import modules_ref as ref
import small_ops_ref as sr
from conftest import load_golden
from cpu_ops import CpuOps
from oracle import torch_port as port
from vgan_amd import modules as M

HALF = 0.5  # a float64 provider rounds each result to float32 once: at most half of any bound of modules_ref


@pytest.fixture(scope="module")
def cpu_ops():
    return CpuOps()


@pytest.fixture
def cpu(monkeypatch, cpu_ops):
    monkeypatch.setattr(M, "default_ops", lambda: cpu_ops)
    return cpu_ops


def tiles_of(n, mode):
    return CpuOps.build_tiles(None, n, mode).numpy()


def use(monkeypatch, provider):
    monkeypatch.setattr(M, "default_ops", lambda: provider)
    return provider


def t64(a, grad=False):
    return torch.tensor(np.asarray(a, dtype=np.float64), requires_grad=grad)


# =============================================================================================== the references are pinned
@pytest.mark.parametrize("kernel", ref.KERNELS, ids=str)
@pytest.mark.parametrize("N,p", ref.RBF_MODULE)
def test_rbf_reference_against_the_port(N, p, kernel):
    Z, _, _ = ref.rbf_operand(N, p, "module")
    G = ref.rng_for(f"G/{N}/{p}").normal(size=(N, N)).astype(np.float32)
    pk = port.PortRBF(*kernel)
    Zr = t64(Z, True)
    Kr = pk(Zr)
    (Kr * t64(G)).sum().backward()
    r = ref.rbf_module_ref(Z, G, np.float32(float(pk.bandwidth)), kernel)
    mr.cap_ok(r.bK, r.K, ref.CAP_FP32), mr.cap_ok(r.bdK, r.dK, ref.CAP_FP32), ref.gr.cap_ok(r.bdZ, r.dZ)
    assert ref.ratio_of(r.K, Kr.detach().numpy(), r.bK) <= HALF
    assert ref.ratio_of(r.dZ, Zr.grad.numpy(), r.bdZ) <= HALF
    table = ref.whole_table(tiles_of, N)
    want, bound = ref.bandwidth_ref(r.z64, r.sq64, table, N)
    assert abs(want - float(pk.bandwidth)) <= HALF * bound and bound <= ref.CAP * want  # a sum: gemm_ref's cap


def loss_cases():
    out = [("eq", n, n, n, p, d) for n, p, d in ref.EQUAL_CASES] + [("uneq",) + c for c in ref.UNEQUAL_CASES]
    return out


@pytest.mark.parametrize("kernel", ref.LOSS_KERNELS, ids=str)
@pytest.mark.parametrize("case", loss_cases(), ids=str)
def test_loss_reference_against_the_port(case, kernel):
    name, nx, ny, nu, p, d = case
    X, Y, Um = ref.loss_data(name, nx, ny, nu, p, d)
    pk = port.PortRBF(*kernel)
    Xr, Yr, Ur = t64(X, True), t64(Y, True), t64(Um, True)
    (port.port_mmd_loss(pk, Xr, Yr, Ur, ref.WEIGHT) * ref.GL).backward()
    r = ref.mmd_loss_ref(X, Y, Um, ref.WEIGHT, np.float32(float(pk.bandwidth)), kernel, gl=ref.GL, tiles_of=tiles_of)
    ref.loss_caps(r)
    want = float(port.port_mmd_loss(pk, Xr, Yr, Ur, ref.WEIGHT).detach())
    assert abs(r.loss - want) <= HALF * r.bloss
    assert r.bloss <= ref.CAP * abs(r.loss), "vacuous loss bound (gemm_ref's cap: the loss is a sum)"
    assert ref.ratio_of(r.dX, Xr.grad.numpy(), r.bdX) <= HALF and ref.ratio_of(r.dY, Yr.grad.numpy(), r.bdY) <= HALF
    assert np.array_equal(r.dU != 0, Ur.grad.numpy() != 0)  # unique column maxima: no tie rule involved
    np.testing.assert_allclose(r.dU, Ur.grad.numpy(), rtol=1e-14, atol=0)


def test_loss_reference_against_fixture_f7():
    g = load_golden("f7_mmd_unequal.npz")
    for k in (0, 1):
        X, Y, Um = g[f"X{k}"], g[f"Y{k}"], g[f"U{k}"]
        r = ref.mmd_loss_ref(X, Y, Um, float(g["weight"]), np.float32(float(g[f"bw{k}_f64"])), (5, 2.0))
        ref.loss_caps(r)
        assert abs(r.loss - float(g[f"loss{k}_f64"])) <= HALF * r.bloss
        assert ref.ratio_of(r.dX, g[f"dX{k}_f64"], r.bdX) <= HALF and ref.ratio_of(r.dY, g[f"dY{k}_f64"], r.bdY) <= HALF
        np.testing.assert_allclose(r.dU, g[f"dU{k}_f64"], rtol=1e-12, atol=0)
        z64, sq64 = ref.given_norms(ref.pad_rows(X, Y))
        want, bound = ref.bandwidth_ref(z64, sq64, ref.whole_table(tiles_of, z64.shape[0]), z64.shape[0])
        assert abs(want - float(g[f"bw{k}_f64"])) <= HALF * bound


def test_tie_rule_is_the_column_key_rule():
    """dU of the reference goes to the LOWEST row among equal column maxima, as small_ops_ref.colkey_ref packs it."""
    X, Y, Um = ref.loss_data("ties", 33, 33, 33, 5, 9, ties=True)
    assert any((Um[:, j] == 1).sum() > 1 for j in range(9)), "the case must hold tied maxima"
    r = ref.mmd_loss_ref(X, Y, Um, ref.WEIGHT, np.float32(10.0), (5, 2.0), tiles_of=tiles_of)
    for j in range(9):
        assert r.rows[j] == int(np.flatnonzero(Um[:, j] == Um[:, j].max())[0])
        assert np.flatnonzero(r.dU[:, j]).tolist() == [r.rows[j]]


@pytest.mark.parametrize("n,d", ref.SOFTMAX_SHAPES)
def test_softmax_reference_against_the_port_and_the_snap_margin(n, d):
    x = ref.softmax_logits(n, d)
    assert ref.snap_clear(x), "an entry within 1e-5 / d of the snap threshold"
    S = sr.softmax64(x)
    got = port.port_upper_softmax(t64(x)).numpy()
    want = np.where(S >= 1.0 / d, 1.0, S)
    np.testing.assert_allclose(got, want, rtol=1e-12, atol=0)
    assert float((ref.softmax_bound(x) / np.maximum(S, ref.TINY)).max()) <= 2e-4 + 1.0  # (rows that underflow are held by 2^-126 alone)
    if n >= 3:
        assert x[1].max() - x[1].min() == 200.0


# =============================================================================================== caps of the direct kernel cases
@pytest.mark.parametrize("index", range(len(ref.RBF_DIRECT)))
def test_direct_rbf_caps_and_provider(cpu_ops, index):
    m, p = ref.RBF_DIRECT[index]
    Z, sq, bw = ref.rbf_operand(m, p, "direct")
    z64, s64 = Z.astype(np.float64), sq.astype(np.float64)
    for variant, kernel, factor in ref.direct_plan(index):
        bwf = np.float32(bw * np.float32(factor))
        r = ref.rbf_matrix_ref(z64, s64, bwf, ref.multipliers(*kernel))
        if factor != 1e-3:  # (module docstring of modules_ref: the one factor that cannot keep the cap)
            mr.cap_ok(r.bK, r.K, ref.CAP_FP32), mr.cap_ok(r.bdK, r.dK, ref.CAP_FP32)
        else:
            off = ~np.eye(m, dtype=bool)
            if m >= 3:
                off[m - 1, m // 2] = off[m // 2, m - 1] = False
            assert m == 1 or ref.underflown(r)[off].mean() > 0.4, "the underflow property must have elements to look at"
        K, dK = torch.zeros(m, m), torch.zeros(m, m)
        cpu_ops.rbf_multi_kernel_matrix(torch.as_tensor(Z), torch.as_tensor(sq), torch.as_tensor([bwf]), ref.multipliers(*kernel), K, dK)
        assert ref.ratio_of(K.numpy(), r.K, r.bK) <= HALF and ref.ratio_of(dK.numpy(), r.dK, r.bdK) <= HALF
    alpha = np.float32(1.0 / bw)
    r = ref.rbf_single_ref(z64, s64, alpha)
    mr.cap_ok(r.bK, r.K, ref.CAP_FP32)
    K = torch.zeros(m, m)
    cpu_ops.rbf_kernel_matrix(torch.as_tensor(Z), torch.as_tensor(sq), float(alpha), K)
    assert ref.ratio_of(K.numpy(), r.K, r.bK) <= HALF


# =============================================================================================== the real modules over CpuOps
def chain_cases():
    return [(kind, n, L, d, mode) for (n, L, d) in ref.CHAIN_SHAPES for kind in ref.CHAIN_KINDS for mode in ref.CHAIN_MODES]


@pytest.mark.parametrize("kind,n,L,d,mode", chain_cases())
def test_chains_over_the_cpu_provider(cpu, kind, n, L, d, mode):
    run = ref.run_chain(M, kind, n, L, d, mode, "cpu")
    ref.chain_caps(run.recs)
    rec = ref.check_chain(run)
    assert max(rec.values()) <= HALF


@pytest.mark.parametrize("n,L,d", ref.CHAIN_SHAPES)
def test_hip_linear_without_bias_over_the_cpu_provider(cpu, n, L, d):
    got, want, bound = ref.run_nobias(M, n, d, 2 * L, "cpu")
    for g, w, b in zip(got, want, bound):
        ref.gr.cap_ok(b, w)
        assert ref.ratio_of(g, w, b) <= HALF


@pytest.mark.parametrize("n,d", ref.SOFTMAX_SHAPES)
def test_upper_softmax_module_over_the_cpu_provider(cpu, n, d):
    x = ref.softmax_logits(n, d)
    g = ref.rng_for(f"softmax g/{n}/{d}").normal(size=(n, d)).astype(np.float32)
    got = ref.run_softmax(M, x, g, "cpu")
    rec = ref.check_softmax(got, x, g)
    assert max(rec.values()) <= HALF


@pytest.mark.parametrize("kernel", ref.KERNELS, ids=str)
@pytest.mark.parametrize("N,p", ref.RBF_MODULE)
def test_rbf_module_over_the_cpu_provider(cpu, N, p, kernel):
    Z, _, _ = ref.rbf_operand(N, p, "module")
    G = ref.rng_for(f"G/{N}/{p}").normal(size=(N, N)).astype(np.float32)
    got = ref.run_rbf(M, cpu, Z, G, kernel, "cpu")
    r = ref.rbf_module_ref(Z, G, np.float32(got.bw), kernel)
    want, bound = ref.bandwidth_ref(r.z64, r.sq64, ref.whole_table(tiles_of, N), N)
    assert abs(got.bw - want) <= HALF * bound
    assert max(ref.check_rbf(got, r).values()) <= HALF
    # a second call on other data uses the frozen value; so does a kernel that is given the bandwidth as a float
    Z2 = (Z * np.float32(0.5)).astype(np.float32)
    for k in (got.k, None):
        again = ref.run_rbf(M, cpu, Z2, G, kernel, "cpu", bandwidth=got.bw, k=k)
        assert again.bw == got.bw
        assert max(ref.check_rbf(again, ref.rbf_module_ref(Z2, G, np.float32(got.bw), kernel)).values()) <= HALF


@pytest.mark.parametrize("need", ref.NEEDS, ids=str)
@pytest.mark.parametrize("kernel", ref.LOSS_KERNELS, ids=str)
@pytest.mark.parametrize("case", loss_cases(), ids=str)
def test_loss_module_over_the_cpu_provider(cpu, case, kernel, need):
    name, nx, ny, nu, p, d = case
    X, Y, Um = ref.loss_data(name, nx, ny, nu, p, d)
    for u_grad in (False, True):
        got = ref.run_loss(M, X, Y, Um, kernel, need, "cpu", u_grad=u_grad, gl=ref.GL)
        r = ref.mmd_loss_ref(X, Y, Um, ref.WEIGHT, np.float32(got.bw), kernel, gl=ref.GL, tiles_of=tiles_of)
        ref.loss_caps(r)
        assert max(ref.check_loss(got, r, need, u_grad).values()) <= HALF
        z64, sq64 = r.z64, r.sq64
        table = tiles_of(nx, 2 if need[0] else (1 if need[1] else 0)) if name == "eq" else ref.whole_table(tiles_of, r.N)
        want, bound = ref.bandwidth_ref(z64, sq64, table, nx if name == "eq" else r.N)
        assert abs(got.bw - want) <= HALF * bound


def test_loss_module_with_tied_maxima_over_the_cpu_provider(cpu):
    X, Y, Um = ref.loss_data("ties", 33, 33, 33, 5, 9, ties=True)
    got = ref.run_loss(M, X, Y, Um, (5, 2.0), (True, True), "cpu", u_grad=True, gl=ref.GL)
    r = ref.mmd_loss_ref(X, Y, Um, ref.WEIGHT, np.float32(got.bw), (5, 2.0), gl=ref.GL, tiles_of=tiles_of)
    assert max(ref.check_loss(got, r, (True, True), True).values()) <= HALF


# =============================================================================================== host logic
class Recorder(CpuOps):
    def __init__(self):
        super().__init__()
        self.wg = []

    def mmd_gram(self, Z, sq, n, p, bw, tiles, calibrate, Wg, wrow0, partial, multipliers=None):
        self.wg.append(Wg)
        super().mmd_gram(Z, sq, n, p, bw, tiles, calibrate, Wg, wrow0, partial, multipliers=multipliers)


@pytest.mark.parametrize("kernel", [(5, 2.0), (3, 3.0)], ids=str)
def test_forward_only_allocates_no_weights(monkeypatch, kernel):
    rec = use(monkeypatch, Recorder())
    X, Y, Um = ref.loss_data("eq", 33, 33, 33, 5, 9)
    got = ref.run_loss(M, X, Y, Um, kernel, (False, False), "cpu")
    assert not got.requires_grad and got.loss_t.grad_fn is None and all(w is None for w in rec.wg) and len(rec.wg) == 2
    rec.wg.clear()
    ref.run_loss(M, X, Y, Um, kernel, (False, True), "cpu")
    assert rec.wg[-1].shape == (33, 66)  # gradient to Y only: the Y rows of W


@pytest.mark.parametrize("case", [("eq", 33, 33, 33, 5, 9), ("uneq", 33, 70, 12, 5, 7)], ids=str)
def test_upstream_scale_multiplies_every_gradient(cpu, case):
    name, nx, ny, nu, p, d = case
    X, Y, Um = ref.loss_data(name, nx, ny, nu, p, d)
    one = ref.run_loss(M, X, Y, Um, (5, 2.0), (True, True), "cpu", u_grad=True)
    scaled = ref.run_loss(M, X, Y, Um, (5, 2.0), (True, True), "cpu", u_grad=True, gl=ref.GL)
    for a, b in ((one.dX, scaled.dX), (one.dY, scaled.dY), (one.dU, scaled.dU)):
        assert ref.same_bits((a * np.float32(ref.GL)).astype(np.float32), b)


@pytest.mark.parametrize("kernel", [(5, 2.0), (3, 3.0)], ids=str)
@pytest.mark.parametrize("case", loss_cases(), ids=str)
def test_second_backward_on_a_retained_graph_gives_the_same_bits(cpu, case, kernel):
    """All MMD paths (equal rows: fused and general kernel; unequal rows).  On the unequal path this raised before the backward
    stopped scaling its saved dK/dL in place."""
    name, nx, ny, nu, p, d = case
    ref.second_backward_of_the_loss(M, ref.loss_data(name, nx, ny, nu, p, d), kernel, "cpu")


def test_second_backward_of_the_rbf_matrix_the_softmax_and_the_chain(cpu):
    ref.second_backward_of_the_others(M, cpu, "cpu")


def test_unequal_first_backward_equals_the_in_place_form(cpu):
    """The values are the products the backward formed before it stopped writing into its saved tensor: restated here (dK/dL
    scaled block by block IN PLACE, then the provider's backward product) and compared bit for bit."""
    for nx, ny, nu, p, d in ref.UNEQUAL_CASES:
        X, Y, Um = ref.loss_data("uneq", nx, ny, nu, p, d)
        got = ref.run_loss(M, X, Y, Um, (5, 2.0), (True, True), "cpu", gl=ref.GL)
        N, pp, Np = nx + ny, ref.round4(p), ref.round4(nx + ny)
        Z = torch.as_tensor(ref.pad_rows(X, Y))
        sq = torch.empty(N)
        cpu.row_sqnorm(Z, sq, pp)
        K, W = torch.zeros(N, Np), torch.zeros(N, Np)
        cpu.rbf_multi_kernel_matrix(Z, sq, torch.as_tensor([got.bw], dtype=torch.float32), mr.multipliers(5, 2.0), K, W)
        W[:nx, :nx].mul_(2.0 / (float(nx) * nx))
        W[:nx, nx:N].mul_(-2.0 / (float(nx) * ny))
        W[nx:, :nx].mul_(-2.0 / (float(nx) * ny))
        W[nx:, nx:N].mul_(2.0 / (float(ny) * ny))
        out = torch.empty(N, pp)
        cpu.mmd_backward(W, Z, 0, N, N, pp, None, out)
        out = (out[:, :p] * torch.tensor(ref.GL)).numpy()
        assert ref.same_bits(out[:nx], got.dX) and ref.same_bits(out[nx:], got.dY)


@pytest.mark.parametrize("case", [("eq", 33, 33, 33, 5, 9), ("uneq", 33, 70, 12, 5, 7)], ids=str)
def test_two_live_graphs_from_one_loss_fn(cpu, case):
    name, nx, ny, nu, p, d = case
    ref.two_live_graphs(M, ref.loss_data(name, nx, ny, nu, p, d), "cpu")


@pytest.mark.parametrize("case", [("eq", 33, 33, 33, 5, 9), ("uneq", 33, 70, 12, 5, 7)], ids=str)
def test_frozen_bandwidth_hand_over(cpu, case):
    name, nx, ny, nu, p, d = case
    X, Y, Um = ref.loss_data(name, nx, ny, nu, p, d)
    first = ref.run_loss(M, X, Y, Um, (5, 2.0), (False, True), "cpu")
    left = first.loss_fn.bandwidth
    assert torch.is_tensor(left) and left.dim() == 0 and left.dtype == torch.float32
    again = ref.run_loss(M, X, Y, Um, None, (False, True), "cpu", loss_fn=first.loss_fn)
    as_float = ref.run_loss(M, X, Y, Um, (5, 2.0), (False, True), "cpu", bandwidth=float(left))
    as_tensor = ref.run_loss(M, X, Y, Um, (5, 2.0), (False, True), "cpu", bandwidth=torch.tensor(float(left), dtype=torch.float64))
    for other in (again, as_float, as_tensor):
        assert other.loss == first.loss and ref.same_bits(other.dY, first.dY) and other.bw == first.bw


class Strict(CpuOps):
    """CpuOps that refuses the layouts HipOps and the C ABI refuse: a float32 matrix needs a unit inner stride and a row stride
    of at least its width (the row stride IS the leading dimension the kernel is given)."""


def _strict(name):
    def method(self, *args, **kw):
        for t in list(args) + list(kw.values()):
            if torch.is_tensor(t) and t.dim() == 2 and t.dtype == torch.float32:
                assert t.stride(1) == 1 and t.stride(0) >= t.shape[1], f"{name}: shape {tuple(t.shape)} strides {t.stride()}"
        return getattr(CpuOps, name)(self, *args, **kw)
    return method


for _name in ("linear_forward", "linear_backward_input", "linear_backward_params", "upper_softmax_forward", "mask_backward", "colmax",
              "row_sqnorm", "rbf_multi_kernel_matrix", "mmd_backward", "mmd_gram", "rows_dot"):
    setattr(Strict, _name, _strict(_name))


def test_every_matrix_reaches_the_provider_in_a_layout_the_abi_accepts(monkeypatch):
    """contiguous() keeps the stride of a size-1 dimension: the expanded scalar that .sum().backward() hands a [1, 1] output
    (Encoder(1, d) on one row) reached vgan_linear_backward_input with strides (0, 0), which HipOps refuses.  Found by the GPU
    tier; pinned here on every chain, the softmax module and the smallest loss shapes."""
    use(monkeypatch, Strict())
    for n, L, d in ref.CHAIN_SHAPES:
        for kind in ref.CHAIN_KINDS:
            for mode in ("all", "sum"):
                ref.check_chain(ref.run_chain(M, kind, n, L, d, mode, "cpu"))
    for n, d in ref.SOFTMAX_SHAPES:
        x = ref.softmax_logits(n, d)
        xt = ref.to_dev(x, "cpu", True)
        M.upper_softmax()(xt).sum().backward()
    for name, nx, ny, nu, p, d in loss_cases()[:2] + loss_cases()[5:7]:
        X, Y, Um = ref.loss_data(name, nx, ny, nu, p, d)
        ref.run_loss(M, X, Y, Um, (5, 2.0), (True, True), "cpu", u_grad=True)
    k = M.RBF(3, 3.0)
    Zt = ref.to_dev(np.ones((1, 1)), "cpu", True).expand(1, 1)
    k.bandwidth = 1.0
    k(Zt).sum().backward()


def test_reexports_are_the_module_classes():
    import src.models.Detector as D
    import src.models.Generator as G
    import src.models.Mmd_loss_constrained as L
    assert D.Detector is M.Detector and D.Encoder is M.Encoder and D.Decoder is M.Decoder
    assert G.Generator_big is M.Generator_big and G.upper_softmax is M.upper_softmax
    assert L.MMDLossConstrained is M.MMDLossConstrained and L.RBF is M.RBF


# =============================================================================================== teeth
MUTATIONS = ["gK not symmetrised", "pad column [N, round4(N)) of K counted in a block mean",
             "XY scale applied to the YX block with the wrong sign", "dK returned for k < n_kernels - 1 only",
             "penalty gradient on the highest tied row", "db skipped when the weight is frozen",
             "dx of the first layer formed from the second layer's W"]


class Mutant(CpuOps):
    """CpuOps with one named defect.  nx: the X row count of the case, for the defects that live in a block of W."""

    def __init__(self, name, nx=None, frozen=False):
        super().__init__()
        assert name in MUTATIONS
        self.m, self.nx, self.frozen, self.N, self.seen = name, nx, frozen, None, []

    def mmd_backward(self, Wg, Z, wrow0, nr, ncols, p, mul, out, **kw):
        r = torch.arange(nr)[:, None] + wrow0
        c = torch.arange(Wg.shape[1])[None, :]
        if self.m == MUTATIONS[0]:  # W = 2 gK * dK on one side of the diagonal and nothing on the other, for (gK + gK^T) * dK
            Wg = torch.where(c > r, 2.0 * Wg[:nr], torch.where(c < r, torch.zeros(()), Wg[:nr]))
        if self.m == MUTATIONS[2]:
            Wg = torch.where((r >= self.nx) & (c < self.nx), -Wg[:nr], Wg[:nr])
        super().mmd_backward(Wg, Z, wrow0, nr, ncols, p, mul, out, **kw)

    def rbf_multi_kernel_matrix(self, Z, sq, bw, multipliers, K, dK=None):
        super().rbf_multi_kernel_matrix(Z, sq, bw, multipliers, K, dK)
        self.N = Z.shape[0]
        if self.m == MUTATIONS[1] and K.shape[1] > self.N:
            K[:, self.N:] = K[:, self.N - 1:self.N]
        if self.m == MUTATIONS[3] and dK is not None:
            dK.zero_()
            if len(multipliers) > 1:
                super().rbf_multi_kernel_matrix(Z, sq, bw, multipliers[:-1], torch.empty_like(K), dK)

    def mmd_gram(self, Z, sq, n, p, bw, tiles, calibrate, Wg, wrow0, partial, multipliers=None):
        super().mmd_gram(Z, sq, n, p, bw, tiles, calibrate, Wg, wrow0, partial, multipliers=multipliers)
        if self.m == MUTATIONS[3] and Wg is not None:
            mults = list(mr.multipliers(5, 2.0) if multipliers is None else multipliers)[:-1]
            super().mmd_gram(Z, sq, n, p, bw, tiles, False, Wg, wrow0, torch.empty_like(partial), multipliers=mults)

    def rows_dot(self, A, B, out, broadcast_b=False):
        if self.m == MUTATIONS[1] and self.N is not None:
            ld = A.stride(0)
            c0 = A.storage_offset() % ld
            if c0 + A.shape[1] == self.N and ld > self.N:
                A = torch.as_strided(A, (A.shape[0], ld - c0), A.stride(), A.storage_offset())
                B = torch.ones(1, ld - c0)
        super().rows_dot(A, B, out, broadcast_b)

    def colmax(self, S, row_offset, part, colkey, from_softmax=True):
        super().colmax(S, row_offset, part, colkey, from_softmax)
        if self.m == MUTATIONS[4]:
            s = S.numpy()
            top = np.array([np.flatnonzero(s[:, j] == s[:, j].max())[-1] for j in range(s.shape[1])], dtype=np.uint64)
            keys = (s.max(0).astype(np.float32).view(np.uint32).astype(np.uint64) << np.uint64(32)) | (np.uint64(0xFFFFFFFF) - top - np.uint64(row_offset))
            colkey.copy_(torch.as_tensor(keys.view(np.int64)))

    def linear_backward_params(self, dy, x, dW, db, **kw):
        super().linear_backward_params(dy, x, dW, db, **kw)
        if self.m == MUTATIONS[5] and self.frozen and db is not None and dW.shape == self.frozen:
            db.zero_()

    def linear_forward(self, x, W, b, y, **kw):
        if not any(W.data_ptr() == s.data_ptr() for s in self.seen):
            self.seen.append(W)
        super().linear_forward(x, W, b, y, **kw)

    def linear_backward_input(self, dy, W, dx):
        if self.m == MUTATIONS[6] and W.data_ptr() == self.seen[0].data_ptr():
            W = torch.as_tensor(np.resize(self.seen[1].detach().numpy(), tuple(W.shape)))
        super().linear_backward_input(dy, W, dx)


def rejected(fn):
    with pytest.raises(AssertionError):
        fn()


def loss_run_and_check(X, Y, Um, kernel, need, u_grad):
    got = ref.run_loss(M, X, Y, Um, kernel, need, "cpu", u_grad=u_grad, gl=ref.GL, bandwidth=None)
    ref.check_loss(got, ref.mmd_loss_ref(X, Y, Um, ref.WEIGHT, np.float32(got.bw), kernel, gl=ref.GL, tiles_of=tiles_of), need, u_grad)


@pytest.mark.parametrize("mutation", [MUTATIONS[0], MUTATIONS[2], MUTATIONS[3]])
@pytest.mark.parametrize("case", loss_cases(), ids=str)
def test_teeth_weight_mutations_in_the_loss(monkeypatch, case, mutation):
    name, nx, ny, nu, p, d = case
    X, Y, Um = ref.loss_data(name, nx, ny, nu, p, d)
    use(monkeypatch, Mutant(mutation, nx=nx))
    for kernel in ref.LOSS_KERNELS:
        for need in ref.NEEDS[:3]:
            if name == "eq" and mutation == MUTATIONS[0]:
                continue  # the fused path never forms gK + gK^T on the host: its mirror store is the Gram kernel's (test_mmd_kernels_*)
            if mutation == MUTATIONS[2] and not need[1]:
                continue  # the YX block reaches the gradient to Y only
            rejected(lambda: loss_run_and_check(X, Y, Um, kernel, need, False))
    use(monkeypatch, CpuOps())
    loss_run_and_check(X, Y, Um, (5, 2.0), (True, True), False)  # the unmutated provider passes the same check


@pytest.mark.parametrize("mutation", [MUTATIONS[0], MUTATIONS[3]])
@pytest.mark.parametrize("kernel", ref.KERNELS, ids=str)
@pytest.mark.parametrize("N,p", ref.RBF_MODULE)
def test_teeth_weight_mutations_in_the_rbf_matrix(monkeypatch, N, p, kernel, mutation):
    Z, _, _ = ref.rbf_operand(N, p, "module")
    G = ref.rng_for(f"G/{N}/{p}").normal(size=(N, N)).astype(np.float32)
    mut = use(monkeypatch, Mutant(mutation))

    def run():
        got = ref.run_rbf(M, mut, Z, G, kernel, "cpu")
        ref.check_rbf(got, ref.rbf_module_ref(Z, G, np.float32(got.bw), kernel))
    rejected(run)


@pytest.mark.parametrize("case", [c for c in ref.UNEQUAL_CASES if (c[0] + c[1]) % 4], ids=str)
def test_teeth_pad_columns_in_a_block_mean(monkeypatch, case):
    nx, ny, nu, p, d = case
    X, Y, Um = ref.loss_data("uneq", nx, ny, nu, p, d)
    use(monkeypatch, Mutant(MUTATIONS[1]))
    for kernel in ref.LOSS_KERNELS:
        for need in ref.NEEDS:
            rejected(lambda: loss_run_and_check(X, Y, Um, kernel, need, False))


def test_teeth_penalty_gradient_on_the_highest_tied_row(monkeypatch):
    X, Y, Um = ref.loss_data("ties", 33, 33, 33, 5, 9, ties=True)
    use(monkeypatch, Mutant(MUTATIONS[4]))
    rejected(lambda: loss_run_and_check(X, Y, Um, (5, 2.0), (True, True), True))
    Xu, Yu, _ = ref.loss_data("uneq", 33, 70, 33, 5, 9)
    rejected(lambda: loss_run_and_check(Xu, Yu, Um, (5, 2.0), (False, False), True))


@pytest.mark.parametrize("kind", ref.CHAIN_KINDS)
@pytest.mark.parametrize("n,L,d", ref.CHAIN_SHAPES)
def test_teeth_chain_mutations(monkeypatch, kind, n, L, d):
    mod, _ = ref.chain_module(M, kind, L, d)
    use(monkeypatch, Mutant(MUTATIONS[5], frozen=tuple(ref.chain_layers(mod, kind)[1].weight.shape)))
    rejected(lambda: ref.check_chain(ref.run_chain(M, kind, n, L, d, "weight frozen", "cpu")))
    for mode in ("all", "sum"):
        use(monkeypatch, Mutant(MUTATIONS[6]))  # (a fresh one: it keeps the weights it has seen)
        rejected(lambda: ref.check_chain(ref.run_chain(M, kind, n, L, d, mode, "cpu")))


def test_every_mutation_has_a_test():
    import inspect
    import sys
    src = inspect.getsource(sys.modules[__name__])
    assert all(src.count(f"MUTATIONS[{i}]") >= 2 for i in range(len(MUTATIONS)))
    assert collections.Counter(MUTATIONS).most_common(1)[0][1] == 1
