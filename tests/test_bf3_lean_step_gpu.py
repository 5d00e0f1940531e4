"""The bf16x3 step without the fp32 operand copy (GPU tier).

The mask / projection launch stops writing the fp32 operand Z (write_z = 0) and the 64-wide MMD backward rebuilds the two numbers
per element it took from Z -- from the data row `xrow[i]`, the softmax S and the centre (vgan_mmd_backward_bf3_rm_rebuild).  That
removes work and must not change one bit of the result: every comparison here is exact.
Shapes: d = 80 (a 16-wide last column tile, a K tile three quarters padding), d = 112, d = 128 (no padding), d = 48 (one partial
tile), with the penalty weight 0 and 10 where a penalty exists.
(The second change of that round, a trimmed K tail of the 64-wide product, measured no gain and is not in the tree:
profiles/README.md.)
"""
import numpy as np
import pytest
import torch

from cpu_ops import CpuOps
from oracle import vgan_oracle as orc

pytestmark = pytest.mark.gpu

SHAPES = [(128, 80), (128, 112), (192, 128), (64, 48)]
I16 = dict(dtype=torch.int16, device="cuda")


@pytest.fixture(scope="module")
def ops():
    from vgan_amd.ops import HipOps
    return HipOps()


def dev(a, dtype=torch.float32):
    return torch.as_tensor(np.ascontiguousarray(a)).to(device="cuda", dtype=dtype)


def bf(t):
    """bf16 bit patterns as floats: -0 == +0, and nothing else compares equal by accident"""
    return t.view(torch.bfloat16).float()


_CASES = {}


def kernel_case(ops, n, d):
    """One batch through the mask / projection launch in both forms (shared by the tests of a shape, left unchanged)."""
    if (n, d) in _CASES:
        return _CASES[(n, d)]
    rng = np.random.default_rng(1000 * n + d)
    rows_total = 3 * n + 5
    data = (rng.normal(size=(rows_total, d)) * 0.7 + rng.normal(size=(1, d)) * 2.0).astype(np.float32)
    logits = rng.normal(size=(n, d)).astype(np.float32)
    # beforehand, on the CPU: every row has mask entries on both sides of the 1/d threshold (u = s and u = 1)
    S_cpu, U_cpu = torch.zeros(n, d), torch.zeros(n, d)
    CpuOps().upper_softmax_forward(torch.as_tensor(logits), S_cpu, U_cpu)
    below = S_cpu.numpy() < np.float32(1.0 / d)
    assert below.any(1).all() and (~below).any(1).all()
    assert ((U_cpu.numpy() == 1.0) == ~below).all()
    perm = rng.permutation(rows_total)[:n].astype(np.int32)
    c = {"n": n, "d": d, "kp": (d + 63) // 64 * 64, "kn": (2 * n + 63) // 64 * 64}
    c["data"], c["logits"], c["perm"] = dev(data), dev(logits), dev(perm.reshape(1, n), torch.int32)
    c["cursor"] = torch.zeros(1, dtype=torch.int64, device="cuda")
    c["center"] = torch.zeros(d, device="cuda")
    ops.col_mean(c["data"], c["center"])
    rowsel = dict(row_cursor=c["cursor"], row_batches=1, row_stride=n, center=c["center"])
    kp = c["kp"]
    c["S"], c["Z"], c["sq"] = torch.zeros(n, d, device="cuda"), torch.zeros(2 * n, d, device="cuda"), torch.zeros(2 * n, device="cuda")
    c["Zh"], c["Zl"] = torch.zeros(2 * n, kp, **I16), torch.zeros(2 * n, kp, **I16)
    ops.mask_project_forward_bf3(c["logits"], c["data"], c["perm"], c["S"], c["Z"], c["sq"], c["Zh"], c["Zl"], None, None, **rowsel)
    # the same launch with write_z = 0: everything but Z as before, Z untouched, xrow = the batch's data rows
    S2, Z2, sq2 = torch.zeros(n, d, device="cuda"), torch.full((2 * n, d), float("nan"), device="cuda"), torch.zeros(2 * n, device="cuda")
    Zh2, Zl2 = torch.zeros(2 * n, kp, **I16), torch.zeros(2 * n, kp, **I16)
    c["xrow"] = torch.full((n,), -1, dtype=torch.int32, device="cuda")
    ops.mask_project_forward_bf3(c["logits"], c["data"], c["perm"], S2, Z2, sq2, Zh2, Zl2, None, None, write_z=False, xrow=c["xrow"], **rowsel)
    torch.cuda.synchronize()
    assert torch.equal(S2, c["S"]) and torch.equal(sq2, c["sq"]) and torch.equal(Zh2, c["Zh"]) and torch.equal(Zl2, c["Zl"])
    assert bool(torch.isnan(Z2).all()), "write_z = 0 must leave Z alone"
    assert torch.equal(c["xrow"], c["perm"][0])
    below_gpu = (c["S"] < 1.0 / d)
    assert bool(below_gpu.any(1).all()) and bool((~below_gpu).any(1).all())
    # a bandwidth of the size the calibration would set: mean squared distance of the operand rows
    zz = c["Z"].double()
    c["bw"] = (torch.cdist(zz, zz) ** 2).sum().div(2 * n * (2 * n - 1)).float().reshape(1)
    _CASES[(n, d)] = c
    return c


def gram(ops, c, tiles=None, store=True):
    n, kn = c["n"], c["kn"]
    tiles = ops.build_tiles(n, 1) if tiles is None else tiles
    Wh, Wl = (torch.zeros(n, kn, **I16), torch.zeros(n, kn, **I16)) if store else (None, None)
    partial = torch.full((tiles.shape[0], 4), float("nan"), device="cuda")
    colpart = torch.zeros(ops.colmax_chunks(n) * c["d"], dtype=torch.int64, device="cuda")
    ops.mmd_gram_bf3(c["Zh"], c["Zl"], c["sq"], n, c["bw"], tiles, Wh, Wl, n, partial, c["S"], 0, colpart, True, tile=64)
    torch.cuda.synchronize()
    return Wh, Wl, partial, colpart


@pytest.mark.parametrize("slabs", [1, 2])
@pytest.mark.parametrize("n,d", SHAPES)
def test_backward_rebuilt_operands_equal_operands_read_from_z(ops, n, d, slabs):
    """gU slabs of vgan_mmd_backward_bf3_rm_rebuild (x, s and the centre in, no Z) against the existing entry point reading the
    Z the forward wrote, its X half as multiplier and the centre as shift: torch.equal, with and without X-X tiles riding in
    the launch -- whose sums equal those of the Gram launch on the same tiles."""
    c = kernel_case(ops, n, d)
    Wh, Wl, _, _ = gram(ops, c)
    assert float(bf(Wh).abs().max()) > 0
    rebuild = ops.bwd_rebuild(c["data"], c["xrow"], c["S"], c["center"])
    table = ops.build_tiles(n, 1)
    xx_tiles = table[(table[:, 4] & 3) == 0][-3:].contiguous()
    assert xx_tiles.shape[0] > 0
    nxx = xx_tiles.shape[0]
    want_part = gram(ops, c, xx_tiles, store=False)[2]
    for with_xx in (False, True):
        a = torch.full((slabs, n, d), float("nan"), device="cuda")
        b = torch.full((slabs, n, d), float("nan"), device="cuda")
        pa, pb = torch.full((nxx, 4), float("nan"), device="cuda"), torch.full((nxx, 4), float("nan"), device="cuda")
        xa = ops.xx_job(c["Zh"], c["Zl"], c["sq"], xx_tiles, c["bw"], pa) if with_xx else None
        xb = ops.xx_job(c["Zh"], c["Zl"], c["sq"], xx_tiles, c["bw"], pb) if with_xx else None
        ops.mmd_backward_bf3_rm(Wh, Wl, c["Zh"], c["Zl"], 2 * n, c["Z"], n, n, d, c["Z"][:n], a[0], slabs, n * d, mul_shift=c["center"],
                                tile=64, xx=xa)
        ops.mmd_backward_bf3_rm_rebuild(Wh, Wl, c["Zh"], c["Zl"], 2 * n, n, d, rebuild, b[0], slabs, n * d, xx=xb)
        torch.cuda.synchronize()
        assert bool(torch.isfinite(a).all()) and float(a.abs().max()) > 0
        assert torch.equal(a, b)
        if with_xx:
            assert torch.equal(pa[:, 0], want_part[:, 0]) and torch.equal(pb[:, 0], want_part[:, 0]) and float(pb[:, 0].abs().min()) > 0


def run_engine(ops, monkeypatch, n, d, pen, z_fp32, graph, slots=None):
    """8 steps over 3 batches per epoch (two new epoch tables on the way) -> (parameters, losses, bandwidth, engine facts)"""
    from vgan_amd.modules import Generator_big
    from vgan_amd.trainer import NoKLStepEngine
    monkeypatch.setenv("VGAN_Z_FP32", "1" if z_fp32 else "0")
    if slots is not None:
        monkeypatch.setenv("VGAN_GRAM_SLOTS", str(slots))
    nb = 3
    rng = np.random.default_rng(7 * n + d)
    data = (rng.normal(size=(nb * n + 11, d)) * 0.7 + rng.normal(size=(1, d)) * 2.0).astype(np.float32)
    gen = Generator_big(orc.latent_size(d), d)
    with torch.no_grad():
        for q, v in zip(gen.parameters(), orc.synthetic_generator_params(d, seed=3)):
            q.copy_(torch.as_tensor(v))
    gen = gen.to("cuda")
    eng = NoKLStepEngine(ops, gen, dev(data), n, nb, noise="device", use_graph=graph, loss_accum_scale=1.0, mmd_precision="bf16x3",
                         penalty_weight=pen)
    assert eng.lean == (not z_fp32) and eng.bsplits >= 1
    losses, left, epoch = [], 8, 0
    both_sides = None
    while left > 0:
        eng.shuffle_epoch(epoch)
        steps = min(nb, left)
        if graph:
            eng.run_steps(steps)
            losses.append(float(eng.loss))
        else:
            for _ in range(steps):
                eng.step()
                losses.append(float(eng.loss))
                if both_sides is None:
                    below = eng.S < 1.0 / d
                    both_sides = bool(below.any(1).all()) and bool((~below).any(1).all())
        left -= steps
        epoch += 1
    assert eng.steps_done == 8 and all(np.isfinite(losses))
    if graph:
        assert eng.graph is not None
    else:
        assert both_sides, "the generator's masks must have entries on both sides of 1/d in every row"
    params = [q.detach().clone() for q in gen.parameters()]
    return params, losses, float(eng.bw), eng.xx_late_in_backward


# (n = 256 with 30 Gram slots: 6 of the 10 X-X tiles ride in the backward launch -- the rebuilt epilogue beside the X-X job)
@pytest.mark.parametrize("n,d,pen,slots", [(128, 80, 0.0, None), (128, 80, 10.0, None), (128, 112, 10.0, None), (192, 128, 10.0, None),
                                            (64, 48, 0.0, None), (64, 48, 10.0, None), (256, 80, 10.0, 30)])
def test_engine_lean_step_equals_step_with_fp32_operand(ops, monkeypatch, n, d, pen, slots):
    """Eight steps across two new epoch tables (the batch cursor moves under `xrow`): the step without the fp32 Z against
    VGAN_Z_FP32=1, eager and through run_steps graphs -- all generator parameters, the losses and the bandwidth bit-equal;
    and the new path twice, bit-equal to itself."""
    for graph in (False, True):
        old = run_engine(ops, monkeypatch, n, d, pen, True, graph, slots)
        new = run_engine(ops, monkeypatch, n, d, pen, False, graph, slots)
        again = run_engine(ops, monkeypatch, n, d, pen, False, graph, slots)
        assert old[3] == new[3] == (slots is not None)
        for other in (new, again):
            assert old[1] == other[1] and old[2] == other[2]
            for a, b in zip(old[0], other[0]):
                assert torch.equal(a, b)
