"""GPU parity tests: every C-ABI entry point (through vgan_amd.ops.HipOps -> libvgan_hip.so) against the
CPU oracle and the golden fixtures generated from the reference.  Run with ``-m gpu`` on an MI355X.
(The small row / feed / reduction / optimiser kernels have direct edge-shape tests of their own: tests/test_small_ops_gpu.py.)
(The modules of vgan_amd/modules.py have float64 tests on every autograd path: tests/modules_ref.py, test_modules_cpu.py, test_modules_gpu.py.)

Tolerances (fp32 path, stated per level as SURVEY.md section 7 asks):
  op level     <= 2e-5 relative (exact for mask decisions / integer outputs)
  loss         <= 1e-4 absolute (BASELINE.json north_star), typically ~1e-6
  gradients    <= 1e-3 of the tensor's max magnitude (fp32 Gram cancellation), typically ~1e-5
  masks        Hamming distance 0 on the pinned c1 trajectory
"""
import os

import numpy as np
import pytest
import torch

from conftest import load_golden
from oracle import vgan_oracle as orc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ops():
    from vgan_amd.ops import HipOps
    return HipOps()


def dev(a, dtype=torch.float32):
    return torch.as_tensor(np.ascontiguousarray(a)).to(device="cuda", dtype=dtype)


def host(t):
    return t.detach().cpu().numpy()


# ------------------------------------------------------------------------------ Linear
def test_linear_backward_input_ragged_width_in_padded_rows(ops):
    """dx = dy . W with a width that is no multiple of 4 (the decoder's input gradient: L = 49) when W's rows are padded to one:
    the vector staging path reads the pad, stores only the true columns, and leaves the rest of dx alone."""
    rng = np.random.default_rng(5)
    n, kin, out = 2048, 49, 784
    Wp = dev(rng.normal(size=(out, 52)) / np.sqrt(kin))        # columns 49..51: pad with arbitrary content
    dy = dev(rng.normal(size=(n, out)))
    dx = torch.full((n, 52), 7.0, device="cuda")
    ops.linear_backward_input(dy, Wp[:, :kin], dx[:, :kin])
    ref = host(dy).astype(np.float64) @ host(Wp[:, :kin]).astype(np.float64)
    np.testing.assert_allclose(host(dx[:, :kin]), ref, rtol=0, atol=2e-5 * np.abs(ref).max())
    assert (host(dx[:, kin:]) == 7.0).all()


@pytest.mark.parametrize("n,kin,out", [(128, 1, 2), (100, 49, 98), (64, 20, 12), (1024, 392, 784), (130, 196, 392), (8, 4, 4),
                                       (2048, 788, 49), (300, 130, 33), (512, 256, 40)])  # the last three: narrow-output forward
def test_linear_forward_backward(ops, n, kin, out):
    rng = np.random.default_rng(n + kin)
    x, W, b = rng.normal(size=(n, kin)), rng.normal(size=(out, kin)) / np.sqrt(kin), rng.normal(size=(out,))
    dy = rng.normal(size=(n, out))
    xd, Wd, bd, dyd = dev(x), dev(W), dev(b), dev(dy)
    y = torch.empty(n, out, device="cuda")
    ops.linear_forward(xd, Wd, bd, y)
    ref = x.astype(np.float32).astype(np.float64) @ W.astype(np.float32).astype(np.float64).T + b.astype(np.float32)
    np.testing.assert_allclose(host(y), ref, rtol=0, atol=2e-5 * np.abs(ref).max())
    dx = torch.empty(n, kin, device="cuda")
    ops.linear_backward_input(dyd, Wd, dx)
    ref = dy.astype(np.float32).astype(np.float64) @ W.astype(np.float32)
    np.testing.assert_allclose(host(dx), ref, rtol=0, atol=2e-5 * np.abs(ref).max())
    dW = torch.empty(out, kin, device="cuda")
    db = torch.empty(out, device="cuda")
    ops.linear_backward_params(dyd, xd, dW, db)
    ref = dy.astype(np.float32).astype(np.float64).T @ x.astype(np.float32)
    np.testing.assert_allclose(host(dW), ref, rtol=0, atol=2e-5 * np.abs(ref).max())
    np.testing.assert_allclose(host(db), dy.astype(np.float32).astype(np.float64).sum(0), rtol=0, atol=2e-5 * np.abs(dy).sum(0).max())
    # split-K slabs over the batch rows + fixed-order reduction
    for splits in (3, 8):
        stride = (out * kin + out + 7) // 4 * 4
        slab = torch.full((splits, stride), float("nan"), device="cuda")
        dWs, dbs = slab[0, :out * kin].view(out, kin), slab[0, out * kin:out * kin + out]
        ops.linear_backward_params(dyd, xd, dWs, dbs, splits, stride)
        red = torch.empty(out * kin + out, device="cuda")
        ops.reduce_slabs(slab, stride, splits, red)
        np.testing.assert_allclose(host(red[:out * kin]).reshape(out, kin), ref, rtol=0, atol=2e-5 * np.abs(ref).max())
        np.testing.assert_allclose(host(red[out * kin:]), dy.astype(np.float32).astype(np.float64).sum(0), rtol=0,
                                   atol=2e-5 * np.abs(dy).sum(0).max())


# ------------------------------------------------------------------------------ upper_softmax / projection
F1 = ["f1_ops_n8_d4.npz", "f1_ops_n64_d12.npz", "f1_ops_n128_d20.npz", "f1_ops_n512_d166.npz"]


@pytest.mark.parametrize("name", F1)
def test_mask_project_forward_golden(ops, name):
    g = load_golden(name)
    logits, X = g["logits"], g["X"]
    n, d = logits.shape
    dp = (d + 3) // 4 * 4
    perm = np.random.default_rng(0).permutation(n).astype(np.int32)
    data = np.zeros_like(X)
    data[perm] = X  # data[perm[i]] = X[i]: exercises the fused batch gather
    S = torch.empty(n, d, device="cuda")
    U = torch.empty(n, d, device="cuda")
    Z = torch.zeros(2 * n, dp, device="cuda")
    sq = torch.empty(2 * n, device="cuda")
    ops.mask_project_forward(dev(logits), dev(data), dev(perm, torch.int32), S, U, Z[:n], Z[n:], sq[:n], sq[n:])
    Ur = g["U_f32"]
    assert np.array_equal(host(U) == 1, Ur == 1), "mask decisions differ from the reference"
    np.testing.assert_allclose(host(U), Ur, rtol=2e-5, atol=0)
    np.testing.assert_allclose(host(Z[:n, :d]), X, rtol=0, atol=0)
    np.testing.assert_allclose(host(Z[n:, :d]), host(U) * X, rtol=1e-6, atol=0)
    np.testing.assert_allclose(host(sq), (host(Z).astype(np.float64) ** 2).sum(1), rtol=1e-5)
    # backward of upper_softmax with the reference's upstream gradient
    dl = torch.empty(n, d, device="cuda")
    ops.mask_backward(dev(g["gU"]), S, None, 0.0, 0, dl)
    ref = g["dlogits_f32"]
    np.testing.assert_allclose(host(dl), ref, rtol=0, atol=5e-5 * np.abs(ref).max())


@pytest.mark.parametrize("n,d", [(72, 2048), (40, 4096), (24, 1500), (16, 4100)])
def test_mask_project_forward_backward_wide_rows(ops, n, d):
    """The row-in-registers mask kernels beyond d = 1024 (8 and 16 float4 per lane: c4 / c5 widths), a width that is no
    multiple of 256, and one past 4096 (generic kernels) against the float64 oracle: softmax values, mask decisions away from the
    threshold, the projected rows, both row norms, the slab-summing backward with the penalty keys."""
    rng = np.random.default_rng(n + d)
    logits = (rng.normal(size=(n, d)) * 2.0).astype(np.float32)
    X = rng.normal(size=(3 * n, d)).astype(np.float32)
    perm = rng.permutation(3 * n)[:n].astype(np.int32)
    center = X.mean(0).astype(np.float32)
    S, U = torch.empty(n, d, device="cuda"), torch.empty(n, d, device="cuda")
    Z = torch.zeros(2 * n, d, device="cuda")
    sq = torch.empty(2 * n, device="cuda")
    ops.mask_project_forward(dev(logits), dev(X), dev(perm, torch.int32), S, U, Z[:n], Z[n:], sq[:n], sq[n:], center=dev(center))
    Ur, sr = orc.upper_softmax_forward(logits.astype(np.float64))
    np.testing.assert_allclose(host(S), sr, rtol=2e-5, atol=1e-12)
    clear = np.abs(sr * d - 1.0) > 1e-4                       # decisions within fp32 rounding of the threshold may flip
    assert np.array_equal((host(U) == 1)[clear], (Ur == 1)[clear])
    Xb = X[perm].astype(np.float64)
    np.testing.assert_allclose(host(Z[:n]), Xb - center, rtol=0, atol=1e-6)
    np.testing.assert_allclose(host(Z[n:]), host(U).astype(np.float64) * Xb - center, rtol=0, atol=2e-6)
    np.testing.assert_allclose(host(sq), (host(Z).astype(np.float64) ** 2).sum(1), rtol=1e-5)
    # backward: two slabs of upstream gradient, penalty keys pointing at rows of this batch
    g0, g1 = rng.normal(size=(n, d)).astype(np.float32), rng.normal(size=(n, d)).astype(np.float32)
    slabs = dev(np.stack([g0, g1]))
    arg = rng.integers(0, n, size=d)
    colkey = dev(((np.uint64(1) << np.uint64(32)) | (np.uint64(0xFFFFFFFF) - arg.astype(np.uint64))).astype(np.uint64).view(np.int64), torch.int64)
    dl = torch.empty(n, d, device="cuda")
    ops.mask_backward(slabs[0], S, colkey, 10.0, 0, dl, nslabs=2, slab_stride=n * d)
    want = CpuOps_mask_backward(g0.astype(np.float64) + g1, host(S).astype(np.float64), arg, 10.0, d)
    np.testing.assert_allclose(host(dl), want, rtol=0, atol=5e-5 * np.abs(want).max())


def CpuOps_mask_backward(g, s, arg, pen_weight, d):
    """float64 restatement of the mask backward with the penalty gradient -w/d at the column arg-max rows
    (Mmd_loss_constrained.py:46-50 through Generator.py:19-21)."""
    g = g.copy()
    g[arg, np.arange(d)] += -pen_weight / d
    return orc.upper_softmax_backward(g, s)


# ------------------------------------------------------------------------------ MMD
def run_mmd(ops, X, Y, U, weight, bw=None, grad_mode=1):
    n, p = X.shape
    d = U.shape[1]
    pp = (p + 3) // 4 * 4
    Z = torch.zeros(2 * n, pp, device="cuda")
    Z[:n, :p] = dev(X)
    Z[n:, :p] = dev(Y)
    sq = torch.empty(2 * n, device="cuda")
    ops.row_sqnorm(Z, sq, pp)
    tiles = ops.build_tiles(n, grad_mode)
    partial = torch.empty(tiles.shape[0], 4, device="cuda")
    stats = torch.empty(4, dtype=torch.float64, device="cuda")
    bwt = torch.empty(1, device="cuda")
    if bw is None:
        ops.mmd_gram(Z, sq, n, pp, None, tiles, True, None, 0, partial)
        ops.mmd_reduce(partial, tiles, stats)
        ops.mmd_set_bandwidth(stats, n, bwt)
    else:
        bwt.fill_(float(bw))
    nr, wrow0 = {0: (0, 0), 1: (n, n), 2: (2 * n, 0)}[grad_mode]
    Wg = torch.full((max(nr, 1), 2 * n), float("nan"), device="cuda")
    ops.mmd_gram(Z, sq, n, pp, bwt, tiles, False, Wg if grad_mode else None, wrow0, partial)
    ops.mmd_reduce(partial, tiles, stats)
    colpart = torch.empty(ops.colmax_chunks(n) * d, dtype=torch.int64, device="cuda")
    colkey = torch.empty(d, dtype=torch.int64, device="cuda")
    ops.colmax(dev(U), 0, colpart, colkey, False)
    loss = torch.empty(1, device="cuda")
    ops.mmd_loss(stats, colkey, n, d, weight, loss)
    dZ = None
    if grad_mode:
        dZ = torch.empty(nr, pp, device="cuda")
        ops.mmd_backward(Wg, Z, wrow0, nr, 2 * n, pp, None, dZ)
        assert not torch.isnan(Wg).any(), "tile table left part of Wg unwritten"
        # split-K slabs of the same product must sum to it
        slabs = torch.full((3, nr, pp), float("nan"), device="cuda")
        ops.mmd_backward(Wg, Z, wrow0, nr, 2 * n, pp, None, slabs[0], 3, nr * pp)
        np.testing.assert_allclose(host(slabs.sum(0)), host(dZ), rtol=0, atol=1e-5 * float(dZ.abs().max()) + 1e-9)
        dZ = host(dZ)[:, :p]
    return dict(loss=float(loss), bw=float(bwt), stats=host(stats), dZ=dZ, colkey=host(colkey))


@pytest.mark.parametrize("name", F1)
def test_mmd_forward_backward_golden(ops, name):
    g = load_golden(name)
    X = g["X"]
    U = g["U_f32"]
    Y = U * X
    r = run_mmd(ops, X, Y, U, 10.0)
    assert abs(r["loss"] - float(g["loss_f64"])) < 1e-4  # north-star bar, vs the reference's fp64 answer
    assert abs(r["loss"] - float(g["loss_f32"])) < 2e-5
    np.testing.assert_allclose(r["bw"], float(g["bw_f64"]), rtol=1e-5)
    if "dY_f64" in g:
        ref = g["dY_f64"]
    else:
        ref = g["dY_f32"]
    np.testing.assert_allclose(r["dZ"], ref, rtol=0, atol=1e-3 * np.abs(ref).max())
    # frozen-bandwidth call on perturbed Y
    r2 = run_mmd(ops, X, Y * np.float32(0.9), U, 10.0, bw=float(g["bw_f32"]))
    assert abs(r2["loss"] - float(g["loss2_f32"])) < 2e-5
    ref2 = g.get("dY2_f64", g["dY2_f32"])
    np.testing.assert_allclose(r2["dZ"], ref2, rtol=0, atol=1e-3 * np.abs(ref2).max())


@pytest.mark.parametrize("n,p", [(100, 20), (65, 7), (200, 33), (256, 64)])
def test_mmd_all_rows_gradient_vs_oracle(ops, n, p):
    """grad_mode 2 (gradient to X and Y, as the detector phase of VGAN.fit needs) on ragged shapes."""
    rng = np.random.default_rng(n * p)
    X = rng.normal(size=(n, p)).astype(np.float32)
    Y = (X * rng.uniform(0.2, 1.0, size=(n, p))).astype(np.float32)
    U = rng.uniform(0.01, 1.0, size=(n, p)).astype(np.float32)
    r = run_mmd(ops, X, Y, U, 3.0, grad_mode=2)
    f = orc.mmd_forward(X.astype(np.float64), Y.astype(np.float64), U.astype(np.float64), 3.0)
    assert abs(r["loss"] - f["loss"]) < 2e-5
    np.testing.assert_allclose(r["bw"], f["bw"], rtol=1e-5)
    # oracle gradient for all rows through torch autograd of the op-for-op port (fp64)
    from oracle import torch_port as port
    Xt = torch.tensor(X, dtype=torch.float64, requires_grad=True)
    Yt = torch.tensor(Y, dtype=torch.float64, requires_grad=True)
    loss = port.port_mmd_loss(port.PortRBF(), Xt, Yt, torch.tensor(U, dtype=torch.float64), 3.0)
    loss.backward()
    ref = np.vstack([Xt.grad.numpy(), Yt.grad.numpy()])
    np.testing.assert_allclose(r["dZ"], ref, rtol=0, atol=1e-3 * np.abs(ref).max())
    # arg-max rows of the penalty
    rows = 0xFFFFFFFF - (r["colkey"] & 0xFFFFFFFF)
    assert np.array_equal(rows, U.argmax(0))


def test_adadelta_vs_oracle(ops):
    rng = np.random.default_rng(3)
    N = 100003
    p, g = rng.normal(size=N).astype(np.float32), rng.normal(size=N).astype(np.float32) * 1e-3
    sq, acc = (rng.random(N) * 1e-6).astype(np.float32), (rng.random(N) * 1e-6).astype(np.float32)
    pd, gd, sd, ad = dev(p), dev(g), dev(sq), dev(acc)
    ops.adadelta_step(pd, gd, sd, ad, 0.007, 0.9, 1e-6, 0.04, 1.0)
    pr, sr, ar = orc.adadelta_step(p.astype(np.float64), g.astype(np.float64), sq.astype(np.float64), acc.astype(np.float64),
                                   0.007, 0.04)
    np.testing.assert_allclose(host(pd), pr, rtol=0, atol=2e-7)
    np.testing.assert_allclose(host(sd), sr, rtol=1e-5, atol=1e-12)
    np.testing.assert_allclose(host(ad), ar, rtol=1e-4, atol=1e-12)


def test_noise_stream(ops):
    ctr = torch.zeros(1, dtype=torch.int64, device="cuda")
    z = torch.empty(1024, 49, device="cuda")
    ops.noise_normal(z, 777, ctr, 0)
    a = host(z).copy()
    ops.noise_normal(z, 777, ctr, 0)
    assert np.array_equal(a, host(z)), "same (seed, step) must reproduce"
    # strided layout with the homogeneous ones column: same draws, independent of the row stride
    zp = torch.zeros(1024, 52, device="cuda")
    ops.noise_normal(zp, 777, ctr, 0, cols=49, ones_col=49)
    assert np.array_equal(host(zp)[:, :49], a) and (host(zp)[:, 49] == 1).all() and (host(zp)[:, 50:] == 0).all()
    ctr += 1
    ops.noise_normal(z, 777, ctr, 0)
    b = host(z)
    assert not np.array_equal(a, b)
    for s in (a, b):
        assert abs(s.mean()) < 0.02 and abs(s.std() - 1) < 0.02 and np.isfinite(s).all()
        assert abs(np.mean(s ** 4) - 3.0) < 0.2  # kurtosis of a normal
    assert abs(np.corrcoef(a.ravel(), b.ravel())[0, 1]) < 0.02


# ------------------------------------------------------------------------------ full steps
def make_engine(ops, params, data, n, nb=1, graph=False, noise="host", **kw):
    from vgan_amd.modules import Generator_big
    from vgan_amd.trainer import NoKLStepEngine
    d = data.shape[1]
    gen = Generator_big(orc.latent_size(d), d)
    with torch.no_grad():
        for q, v in zip(gen.parameters(), params):
            q.copy_(torch.as_tensor(v))
    gen = gen.to("cuda")
    eng = NoKLStepEngine(ops, gen, dev(data), n, nb, noise=noise, use_graph=graph, loss_accum_scale=1.0, **kw)
    return eng, gen


@pytest.mark.parametrize("mode", ["collapsed", "layered"])
@pytest.mark.parametrize("cfg,precision", [("c1", "fp32"), ("c2", "fp32"), ("c2", "bf16x3")])
def test_full_step_golden(ops, cfg, mode, precision):
    """Two full steps against the reference's own numbers (fixture F2).  BASELINE.json configs[1] (c2: musk, d=166, batch=512)
    is specified as bf16: it runs in both arithmetic modes (`auto` would pick the fp32 MFMA at that size)."""
    g = load_golden(f"f2_step_{cfg}.npz")
    batch, noise = g["batch"], g["noise"]
    n = batch.shape[0]
    eng, gen = make_engine(ops, [g[f"param0_{i}"] for i in range(8)], batch, n, generator_mode=mode, mmd_precision=precision)
    assert eng.precision == precision
    eng.set_epoch_batches(torch.arange(n).view(1, n))
    for step in range(2):
        eng.set_noise(torch.as_tensor(noise))
        eng.step()
        assert abs(float(eng.loss) - float(g[f"loss{step}"])) < 2e-5
        for i in range(8):
            ref = g[f"grad{step}_{i}"]
            got = host(eng.grad_view(i))
            np.testing.assert_allclose(got, ref, rtol=0, atol=1e-3 * max(np.abs(ref).max(), 1e-8))
            np.testing.assert_allclose(host(eng.fp.view(eng.fp.flat, i)), g[f"param{step + 1}_{i}"], rtol=0, atol=5e-6)
    np.testing.assert_allclose(float(eng.bw), float(g["bw"]), rtol=1e-5)


@pytest.mark.parametrize("graph,mode", [(False, "collapsed"), (True, "collapsed"), (True, "layered")])
def test_trajectory_c1_golden(ops, graph, mode):
    """BASELINE.json configs[0]: d=20, batch=128, 200 steps of VGAN_no_kl.fit on the recorded batches/noise."""
    g = load_golden("f3_traj_c1.npz")
    data = g["data"]
    eng, gen = make_engine(ops, [g[f"param0_{i}"] for i in range(8)], data, 128, nb=10, graph=graph, generator_mode=mode,
                           lr=float(g["lr"]), weight_decay=float(g["weight_decay"]))
    hist = torch.zeros(200, device="cuda")
    for t in range(200):
        if t % 10 == 0:
            eng.set_epoch_batches(torch.as_tensor(g["idx"][t:t + 10].astype(np.int64)))
        eng.set_noise(torch.as_tensor(g["noise"][t]))
        eng.step()
        hist[t:t + 1].copy_(eng.loss)
    losses = host(hist)
    assert np.abs(losses - g["losses"]).max() < 1e-4, np.abs(losses - g["losses"]).max()
    np.testing.assert_allclose(float(eng.bw), float(g["bw"]), rtol=1e-5)
    logits = eng.generator_logits(torch.as_tensor(g["mask_noise"]))
    S = torch.empty_like(logits)
    U = torch.empty_like(logits)
    ops.upper_softmax_forward(logits, S, U)
    masks = host(U) >= np.float32(1.0 / 20)
    assert np.array_equal(masks, g["masks"]), f"Hamming distance {(masks != g['masks']).sum()}"
    for i in range(8):
        np.testing.assert_allclose(host(eng.fp.view(eng.fp.flat, i)), g[f"paramT_{i}"], rtol=0, atol=2e-4)
    # the module the engine re-homed must see the trained parameters
    assert torch.equal(next(gen.parameters()).data, eng.W[0])


@pytest.mark.parametrize("mode", ["collapsed", "layered"])
def test_c3_step_vs_fp64_reference(ops, mode):
    """BASELINE.json metric config (d=784, batch=1024): MMD^2 loss within 1e-4 of the reference's fp64 value."""
    g = load_golden("f5_c3_scalars.npz")
    n, d = 1024, 784
    data = orc.synthetic_dataset("c3", rows=2048)[:n]
    z = np.random.default_rng(5).normal(size=(n, orc.latent_size(d))).astype(np.float32)
    eng, _ = make_engine(ops, orc.synthetic_generator_params(d), data, n, generator_mode=mode, mmd_precision="fp32")
    eng.set_epoch_batches(torch.arange(n).view(1, n))
    eng.set_noise(torch.as_tensor(z))
    eng.step()
    assert abs(float(eng.loss) - float(g["loss_f64"])) < 1e-4
    np.testing.assert_allclose(float(eng.bw), float(g["bw_f64"]), rtol=1e-5)
    nn = float(n) * n
    st = host(eng.stats)
    np.testing.assert_allclose(st[0] / nn, float(g["xx_f64"]), rtol=1e-5)
    np.testing.assert_allclose(st[1] / nn, float(g["xy_f64"]), rtol=1e-5)
    np.testing.assert_allclose(st[2] / nn, float(g["yy_f64"]), rtol=1e-5)
    U = torch.empty(n, d, device="cuda")
    ops.mask_from_softmax(eng.S, U)
    assert int((host(U) >= np.float32(1 / d)).sum()) == int(g["nsel_f64"])
    for i in range(8):
        gn = np.sqrt((host(eng.grad_view(i)).astype(np.float64) ** 2).sum())
        np.testing.assert_allclose(gn, float(g[f"gnorm_f64_{i}"]), rtol=5e-3)
    np.testing.assert_allclose(host(eng.grad_view(6))[:8, :16], g["g6slice_f64"], rtol=0,
                               atol=5e-3 * np.abs(g["g6slice_f64"]).max())


def test_full_size_properties(ops):
    """Size-independent properties at the metric's full size (n=1024, d=784)."""
    n, d = 1024, 784
    rng = np.random.default_rng(11)
    X = orc.synthetic_dataset("c3", rows=n, seed=3)
    ones = np.ones((n, d), dtype=np.float32)
    # (1) identical samples: MMD^2 == 0 up to fp32 rounding and its gradient vanishes
    r = run_mmd(ops, X, X.copy(), ones, 0.0)
    assert abs(r["loss"]) < 1e-5
    assert np.abs(r["dZ"]).max() < 1e-6
    # (2) invariance under a permutation of the batch rows (sums are order independent up to rounding)
    U = rng.uniform(0.0, 1.0, size=(n, d)).astype(np.float32)
    Y = (U > 0.5).astype(np.float32) * X
    a = run_mmd(ops, X, Y, U, 10.0)
    perm = rng.permutation(n)
    b = run_mmd(ops, X[perm], Y[perm], U[perm], 10.0)
    assert abs(a["loss"] - b["loss"]) < 2e-6
    np.testing.assert_allclose(a["bw"], b["bw"], rtol=1e-6)
    np.testing.assert_allclose(a["dZ"][perm], b["dZ"], rtol=0, atol=1e-4 * np.abs(a["dZ"]).max())
    # (3) block statistics: diagonal included (each K_ii = 5), so every block mean is in (0, 5]
    st = a["stats"][:3] / (n * n)
    assert (st > 0).all() and (st <= 5.0 + 1e-6).all()


# ------------------------------------------------------------------------------ module / user surface
def test_modules_autograd_matches_port(ops):
    from oracle import torch_port as port
    from src.models.Generator import Generator_big
    from src.models.Mmd_loss_constrained import MMDLossConstrained, RBF
    g = load_golden("f2_step_c1.npz")
    batch, noise = torch.tensor(g["batch"]), torch.tensor(g["noise"])
    gen = Generator_big(1, 20)
    with torch.no_grad():
        for q, i in zip(gen.parameters(), range(8)):
            q.copy_(torch.tensor(g[f"param0_{i}"]))
    assert list(gen.state_dict().keys()) == [f"main.{k}.{w}" for k in range(4) for w in ("weight", "bias")]
    gen = gen.cuda()
    loss_fn = MMDLossConstrained(weight=10, kernel=RBF())
    U = gen(noise.cuda())
    loss = loss_fn(batch.cuda(), U * batch.cuda(), U)
    loss.backward()
    assert abs(float(loss) - float(g["loss0"])) < 2e-5
    np.testing.assert_allclose(float(loss_fn.bandwidth), float(g["bw"]), rtol=1e-5)
    for i, q in enumerate(gen.parameters()):
        ref = g[f"grad0_{i}"]
        np.testing.assert_allclose(host(q.grad), ref, rtol=0, atol=1e-3 * max(np.abs(ref).max(), 1e-8))
    del port


@pytest.mark.parametrize("nk,mf", [(5, 2.0), (3, 3.0), (6, 1.5), (1, 2.0)])
def test_rbf_module_forward_matrix_and_general_kernels(ops, nk, mf):
    """The operator boundary of src/models/Mmd_loss_constrained.py:5-26 beyond the fused default: RBF(n_kernels, mul_factor)
    .forward(Z) returns the N x N kernel matrix (first call calibrates and freezes the bandwidth) with autograd to Z, and
    MMDLossConstrained runs with any such kernel -- against the float64 op-for-op port (oracle/torch_port.py)."""
    from oracle import torch_port as port
    from src.models.Mmd_loss_constrained import MMDLossConstrained, RBF
    rng = np.random.default_rng(nk * 10 + int(mf * 10))
    N, p = 150, 22
    Z = rng.normal(size=(N, p)).astype(np.float32)
    k = RBF(n_kernels=nk, mul_factor=mf)
    assert torch.equal(k.bandwidth_multipliers, mf ** (torch.arange(nk) - nk // 2))
    Zt = dev(Z).requires_grad_(True)
    K = k(Zt)
    pk = port.PortRBF(nk, mf)
    Zr = torch.tensor(Z, dtype=torch.float64, requires_grad=True)
    Kr = pk(Zr)
    assert K.shape == (N, N)
    np.testing.assert_allclose(float(k.bandwidth), float(pk.bandwidth), rtol=1e-5)
    np.testing.assert_allclose(host(K), Kr.detach().numpy(), rtol=0, atol=2e-5)
    G = rng.normal(size=(N, N)).astype(np.float32)
    (K * dev(G)).sum().backward()
    (Kr * torch.tensor(G, dtype=torch.float64)).sum().backward()
    np.testing.assert_allclose(host(Zt.grad), Zr.grad.numpy(), rtol=0, atol=1e-3 * float(Zr.grad.abs().max()))
    # second call: frozen bandwidth (Mmd_loss_constrained.py:16-22)
    K2 = k(dev(Z * 0.5))
    np.testing.assert_allclose(host(K2), pk(torch.tensor(Z * 0.5, dtype=torch.float64)).numpy(), rtol=0, atol=2e-5)
    # the loss with this kernel, gradient to both X and Y
    n = 70
    X = rng.normal(size=(n, p)).astype(np.float32)
    Y = (X * rng.uniform(0.2, 1.0, size=(n, p))).astype(np.float32)
    U = rng.uniform(0.01, 1.0, size=(n, p)).astype(np.float32)
    loss_fn = MMDLossConstrained(weight=3.0, kernel=RBF(n_kernels=nk, mul_factor=mf))
    Xt, Yt = dev(X).requires_grad_(True), dev(Y).requires_grad_(True)
    loss = loss_fn(Xt, Yt, dev(U))
    loss.backward()
    Xr, Yr = torch.tensor(X, dtype=torch.float64, requires_grad=True), torch.tensor(Y, dtype=torch.float64, requires_grad=True)
    pk2 = port.PortRBF(nk, mf)
    lr = port.port_mmd_loss(pk2, Xr, Yr, torch.tensor(U, dtype=torch.float64), 3.0)
    lr.backward()
    assert abs(float(loss.detach()) - float(lr.detach())) < 2e-5
    np.testing.assert_allclose(float(loss_fn.bandwidth), float(pk2.bandwidth), rtol=1e-5)
    for got, ref in ((Xt.grad, Xr.grad), (Yt.grad, Yr.grad)):
        np.testing.assert_allclose(host(got), ref.numpy(), rtol=0, atol=1e-3 * float(ref.abs().max()))
    with pytest.raises(ValueError):
        loss_fn(dev(X), dev(Y[:, :3]), dev(U))  # different column counts
    with pytest.raises(ValueError):
        RBF(n_kernels=9)


def test_mmd_loss_with_unequal_row_counts_golden():
    """MMDLossConstrained on X [n_x, p], Y [n_y, p] with n_x != n_y and a U of its own row count (the reference's block means
    over n_x^2, n_x n_y, n_y^2 entries, Mmd_loss_constrained.py:46-49) against fixture F7, written by the reference itself:
    loss within the 1e-4 bar of its float64 value (and 2e-5 of its float32 one), calibrated bandwidth, dX, dY, dU, and a
    second call on the frozen bandwidth."""
    from vgan_amd.modules import MMDLossConstrained, RBF
    g = load_golden("f7_mmd_unequal.npz")
    w = float(g["weight"])
    for k in (0, 1):
        X, Y, U = (dev(g[f"{a}{k}"]).requires_grad_(True) for a in "XYU")
        loss_fn = MMDLossConstrained(weight=w, kernel=RBF())
        loss = loss_fn(X, Y, U)
        loss.backward()
        assert abs(float(loss.detach()) - float(g[f"loss{k}_f64"])) < 1e-4
        assert abs(float(loss.detach()) - float(g[f"loss{k}_f32"])) < 2e-5
        np.testing.assert_allclose(float(loss_fn.bandwidth), float(g[f"bw{k}_f64"]), rtol=1e-5)
        for t, name in ((X, "dX"), (Y, "dY"), (U, "dU")):
            ref = g[f"{name}{k}_f64"]
            np.testing.assert_allclose(host(t.grad), ref, rtol=0, atol=1e-3 * np.abs(ref).max(), err_msg=name)
        Y2 = dev(g[f"Y{k}"] * np.float32(1.1) + np.float32(0.05)).requires_grad_(True)
        loss2 = loss_fn(X.detach(), Y2, U.detach())   # frozen bandwidth; gradient to Y only
        loss2.backward()
        assert abs(float(loss2.detach()) - float(g[f"loss2{k}_f64"])) < 1e-4
        ref = g[f"dY2{k}_f64"]
        np.testing.assert_allclose(host(Y2.grad), ref, rtol=0, atol=1e-3 * np.abs(ref).max())


def test_fit_drop_in_matches_reference_run():
    """VGAN_no_kl(...).fit(X) through the reference's import path, with the noise drawn from torch's CPU
    generator like the reference's CPU path: same seed -> same init, same shuffles, same noise, so the
    epoch losses and the 500 sampled masks must reproduce the reference's own run (fixture f3)."""
    from src.vgan import VGAN_no_kl
    from src.models.Mmd_loss_constrained import MMDLossConstrained
    MMDLossConstrained.__init__.__defaults__[0].bandwidth = None  # fresh process-wide RBF
    g = load_golden("f3_traj_c1.npz")
    model = VGAN_no_kl(batch_size=128, epochs=20, seed=777)
    model.noise_source = "host"
    model.verbose = False
    model.fit(g["data"])
    np.testing.assert_allclose(model.train_history["generator_loss"], g["epoch_losses"], rtol=0, atol=1e-4)
    np.testing.assert_allclose(float(model.bandwidth), float(g["bw"]), rtol=1e-5)
    masks = model.generate_subspaces(500)
    assert masks.dtype == torch.bool and masks.shape == (500, 20) and masks.is_cuda
    assert np.array_equal(host(masks), g["masks"])
    model.approx_subspace_dist()
    assert abs(model.proba.sum() - 1) < 1e-12
    # device-noise (Philox) run: different stream, statistically equivalent training
    MMDLossConstrained.__init__.__defaults__[0].bandwidth = None
    m2 = VGAN_no_kl(batch_size=128, epochs=20, seed=777)
    m2.verbose = False
    m2.fit(g["data"])
    assert abs(m2.train_history["generator_loss"][-1] - g["epoch_losses"][-1]) < 0.3


def test_vgan_kernel_learning_fit_matches_reference_run():
    """VGAN.fit (detector + generator alternation, src/vgan.py:178-353) on the HIP operators under autograd, against the
    reference's own 12-epoch run (fixture f4): same seed -> same N(0, 0.1) init, shuffles and CPU noise draws.
    Tolerance 5e-3 on the epoch losses (observed 1.4e-3): with N(0, 0.1) weights the generator's logits are ~1e-3, its
    softmax is uniform to 1e-4 and about half of all entries sit within fp32 rounding of the 1/d threshold, so a few
    mask bits differ between any two fp32 implementations (the steps before the first mask-dependent one agree to 1e-6)."""
    from src.vgan import VGAN
    from src.models.Mmd_loss_constrained import MMDLossConstrained
    MMDLossConstrained.__init__.__defaults__[0].bandwidth = None
    g = load_golden("f4_kl_c1.npz")
    model = VGAN(batch_size=128, epochs=12)
    model.verbose = False
    model.noise_source = "host"
    model.fit(g["data"])
    gl, dl = np.array(model.train_history["generator_loss"]), np.array(model.train_history["detector_loss"])
    assert np.isnan(gl[0]) and np.isnan(g["generator_loss"][0])          # no generator epoch yet (src/vgan.py:232-233)
    np.testing.assert_allclose(gl[1:], g["generator_loss"][1:], rtol=0, atol=5e-3)
    np.testing.assert_allclose(dl, g["detector_loss"], rtol=0, atol=5e-3)
    np.testing.assert_allclose(float(model.bandwidth), float(g["bw"]), rtol=1e-3)
    for i, q in enumerate(model.generator.parameters()):
        assert np.array_equal(host(q), g[f"genT_{i}"])                    # reference quirk: the generator never trains here
    for i, q in enumerate(model.detector.parameters()):
        np.testing.assert_allclose(host(q), g[f"detT_{i}"], rtol=0, atol=1e-3)
        assert bool(q.requires_grad) == bool(g[f"detT_rg_{i}"])           # encoder-freeze quirk reproduced
    masks = model.generate_subspaces(500)
    assert (host(masks) != g["masks"]).mean() < 0.05
    MMDLossConstrained.__init__.__defaults__[0].bandwidth = None


@pytest.mark.parametrize("n,d,rows", [(500, 166, 1500), (96, 33, 300), (250, 784, 500), (600, 901, 1250), (600, 900, 1250)])
def test_ragged_shapes_trajectory_vs_oracle(ops, n, d, rows):
    """Default-like batch sizes that are no multiple of the 64-wide tile (the reference's default is 500), feature counts
    that are no multiple of 4, and an epoch with a dropped remainder: 6 steps against the fp64 oracle.  The precision
    mode is the engine's own choice ("auto"): fp32 kernels for the first three shapes, split-bf16 for the last two -- with
    the two-launch forward (d = 901) and with the fused forward on a batch that is no multiple of the 64-row tile (d = 900)."""
    rng = np.random.default_rng(n + d)
    data = (rng.normal(size=(rows, d)) * rng.uniform(0.5, 2.0, size=(1, d))).astype(np.float32)
    params = orc.synthetic_generator_params(d, seed=3)
    L = orc.latent_size(d)
    nb = rows // n
    eng, _ = make_engine(ops, params, data, n, nb=nb, graph=True)
    assert eng.precision == ("bf16x3" if 2 * n * d >= (1 << 20) else "fp32")
    assert eng.fused_prepare == (eng.precision == "bf16x3" and d % 4 == 0)
    ref = orc.NoKLTrainer([p.astype(np.float64) for p in params])
    perm = np.stack([rng.permutation(rows)[:n] for _ in range(nb)])
    eng.set_epoch_batches(torch.as_tensor(perm))
    for t in range(6):
        z = rng.normal(size=(n, L)).astype(np.float32)
        eng.set_noise(torch.as_tensor(z))
        eng.step()
        want = ref.step(data[perm[t % nb]].astype(np.float64), z.astype(np.float64))
        assert abs(float(eng.loss) - want["loss"]) < 1e-4, (t, float(eng.loss), want["loss"])
    np.testing.assert_allclose(float(eng.bw), ref.bw, rtol=1e-5)
    for i in range(8):
        np.testing.assert_allclose(host(eng.fp.view(eng.fp.flat, i)), ref.params[i], rtol=0, atol=1e-4)


def test_c2_fit_end_to_end_device_noise():
    """BASELINE.json configs[1] stand-in (musk-like, d=166, batch=512): a short fit with the Philox noise feed trains
    (loss finite, bandwidth frozen after the first step, masks well-formed, run folder written like the reference's)."""
    import tempfile, os
    from src.vgan import VGAN_no_kl
    from src.models.Mmd_loss_constrained import MMDLossConstrained
    MMDLossConstrained.__init__.__defaults__[0].bandwidth = None
    X = orc.synthetic_dataset("c2")
    with tempfile.TemporaryDirectory() as tmp:
        run = os.path.join(tmp, "run")
        model = VGAN_no_kl(batch_size=512, epochs=4, seed=11, path_to_directory=run)
        model.verbose = False
        model.fit(X)
        hist = model.train_history["generator_loss"]
        assert len(hist) == 4 and np.isfinite(hist).all()
        assert set(os.listdir(run)) >= {"models", "params.csv", "train_history"}
        sd = torch.load(os.path.join(run, "models", "generator_0.pt"), weights_only=True)
        assert list(sd) == [f"main.{k}.{w}" for k in range(4) for w in ("weight", "bias")]
        m2 = VGAN_no_kl(seed=11)
        m2.load_models(os.path.join(run, "models", "generator_0.pt"), ndims=166)
        assert torch.equal(m2.generate_subspaces(64), model.generate_subspaces(64))
    u = model.generate_subspaces(100)
    assert u.shape == (100, 166) and u.dtype == torch.bool and u.any(dim=1).all()
    MMDLossConstrained.__init__.__defaults__[0].bandwidth = None


def test_two_fits_in_one_process_share_the_bandwidth():
    """The reference's shared-RBF quirk (Mmd_loss_constrained.py:35: ONE default RBF per process): a second fit finds the
    bandwidth already frozen by the first.  Its engine then never calibrates: its first step must run eagerly (first-ever
    launches of the bf16x3 kernels, the one-off noise draw) and only the later ones replay a captured graph."""
    from src.vgan import VGAN_no_kl
    from src.models.Mmd_loss_constrained import MMDLossConstrained
    MMDLossConstrained.__init__.__defaults__[0].bandwidth = None
    a = VGAN_no_kl(batch_size=128, epochs=2, seed=1)
    a.verbose = False
    a.fit(orc.synthetic_dataset("c1", rows=512))
    bw = float(a.bandwidth)
    rng = np.random.default_rng(3)
    b = VGAN_no_kl(batch_size=1024, epochs=2, seed=2)   # 2 n d >= 2^20: the engine picks the split-bf16 kernels
    b.verbose = False
    b.fit(rng.normal(size=(3072, 512)).astype(np.float32))
    assert b._engine.precision == "bf16x3" and b._engine.graph is not None and b._engine.steps_done == 6
    assert float(b.bandwidth) == bw and float(b._engine.bw) == bw
    assert np.isfinite(b.train_history["generator_loss"]).all()
    MMDLossConstrained.__init__.__defaults__[0].bandwidth = None


@pytest.mark.parametrize("n,d,nb,precision", [(128, 20, 5, "fp32"), (1024, 784, 16, "bf16x3"), (256, 100, 20, "fp32")])
def test_run_steps_blocks_equal_single_steps(ops, n, d, nb, precision):
    """NoKLStepEngine.run_steps (blocks of steps replayed from ONE graph launch; the device-side step counter picks the batch
    and keys the noise) against the same steps launched one graph at a time: epoch losses, bandwidth and all eight parameter
    tensors bit for bit over three epochs, including an epoch length that is no multiple of the block (nb = 20, block 16)."""
    rng = np.random.default_rng(n + d)
    data = rng.normal(size=(nb * n + 7, d)).astype(np.float32)
    params = orc.synthetic_generator_params(d, seed=3)
    runs = []
    for blocks in (True, False):
        eng, gen = make_engine(ops, params, data, n, nb=nb, graph=True, noise="device", mmd_precision=precision)
        losses = []
        for epoch in range(3):
            eng.shuffle_epoch(epoch)
            if blocks:
                eng.run_steps(nb)
            else:
                for _ in range(nb):
                    eng.step()
            losses.append(eng.epoch_loss())
        assert eng.steps_done == 3 * nb and int(eng.step_counter.item()) == 3 * nb
        if blocks:
            assert eng.graph_multi is not None and eng.steps_per_graph == min(16, nb)
        runs.append((losses, float(eng.bw.item()), [host(q).copy() for q in gen.parameters()]))
    assert runs[0][0] == runs[1][0] and runs[0][1] == runs[1][1]
    assert all(np.isfinite(runs[0][0]))
    for a, b in zip(runs[0][2], runs[1][2]):
        assert np.array_equal(a, b)


def test_device_shuffle_and_mask_unique(ops):
    """SURVEY 8f rank 4 on the device: vgan_shuffle_epoch equals the host evaluation of the same counter-based permutation
    (a bijection: distinct rows, different every epoch) and a fit driven by it trains; vgan_mask_unique equals
    np.unique(masks, axis=0, return_counts=True) -- rows, order and counts -- which approx_subspace_dist now uses."""
    for N, count in ((16384, 16384), (5001, 4096), (3, 2)):
        perm = torch.full((count,), -1, dtype=torch.int32, device="cuda")
        ops.shuffle_epoch(perm, N, 777, 5)
        got = host(perm)
        assert got.tolist() == [ops.shuffle_index(i, N, 777, 5) for i in range(count)]
        assert len(set(got.tolist())) == count and got.min() >= 0 and got.max() < N
    rng = np.random.default_rng(12)
    for n, d in ((1, 20), (500, 20), (500, 64), (777, 65), (1000, 784)):
        base = rng.random((max(n // 7, 1), d)) < 0.4
        masks = base[rng.integers(0, base.shape[0], size=n)]
        masks[rng.integers(0, n, size=n // 10), rng.integers(0, d, size=n // 10)] ^= True
        u, c = ops.mask_unique(torch.as_tensor(masks).cuda())
        ur, cr = np.unique(masks, axis=0, return_counts=True)
        assert np.array_equal(host(u), ur) and np.array_equal(c.numpy(), cr), (n, d)
    from src.vgan import VGAN_no_kl
    from src.models.Mmd_loss_constrained import MMDLossConstrained
    MMDLossConstrained.__init__.__defaults__[0].bandwidth = None
    model = VGAN_no_kl(batch_size=128, epochs=4, seed=3)
    model.verbose, model.shuffle_source = False, "device"
    model.fit(orc.synthetic_dataset("c1", rows=700))
    assert np.isfinite(model.train_history["generator_loss"]).all()
    perm = host(model._engine.perm)
    assert perm.shape == (5, 128) and len(set(perm.ravel().tolist())) == 640
    model.approx_subspace_dist(subspace_count=300)
    ur, cr = np.unique(host(model.generate_subspaces(300)), axis=0, return_counts=True)
    assert np.array_equal(model.subspaces, ur) and np.allclose(model.proba, cr / cr.sum())
    MMDLossConstrained.__init__.__defaults__[0].bandwidth = None


def test_reference_saved_checkpoint_and_run_folder_interchange():
    """f6: a run folder written by the REFERENCE.  Its generator_0.pt goes through this build's load_models (weights-only)
    and generate_subspaces returns the masks the reference itself sampled from it; a fit of this build with the same
    hyper-parameters writes the same files, the same params.csv text and a generator_loss CSV of the same shape."""
    import tempfile
    from conftest import REPO
    from src.vgan import VGAN_no_kl
    from src.models.Mmd_loss_constrained import MMDLossConstrained
    g = load_golden("f6_ref_run.npz")
    m = VGAN_no_kl(seed=5)
    m.load_models(os.path.join(REPO, "tests", "golden", "f6_ref_generator_c1.pt"), ndims=20)
    masks = m.generate_subspaces(64)
    assert np.array_equal(host(masks), g["masks"])
    MMDLossConstrained.__init__.__defaults__[0].bandwidth = None
    with tempfile.TemporaryDirectory() as tmp:
        run = os.path.join(tmp, "run")
        model = VGAN_no_kl(batch_size=128, epochs=3, seed=5, path_to_directory=run)
        model.verbose = False
        model.noise_source = "host"
        model.fit(orc.synthetic_dataset("c1", rows=640))
        assert sorted(os.listdir(run)) == list(g["files"]) and sorted(os.listdir(os.path.join(run, "models"))) == list(g["model_files"])
        assert open(os.path.join(run, "params.csv")).read() == str(g["params_csv"])
        ours = np.loadtxt(os.path.join(run, "train_history", "generator_loss_0.csv"), ndmin=1)
        ref = np.array([float(v) for v in str(g["loss_csv"]).split()])
        np.testing.assert_allclose(ours, ref, rtol=0, atol=1e-4)      # same seed, same RNG order: the reference's own epoch losses
        sd = torch.load(os.path.join(run, "models", "generator_0.pt"), weights_only=True)
        for i, v in enumerate(sd.values()):
            np.testing.assert_allclose(host(v), g[f"param_{i}"], rtol=0, atol=2e-5)
    MMDLossConstrained.__init__.__defaults__[0].bandwidth = None


# ------------------------------------------------------------------------------ split-bf16 ("bf16x3") MMD mode
def test_bf3_prepare_and_kernels_vs_fp64(ops):
    n, d = 1024, 784
    rng = np.random.default_rng(21)
    X = orc.synthetic_dataset("c3", rows=n, seed=5)
    U = np.where(rng.random((n, d)) < 0.5, 1.0, rng.random((n, d)) * 1e-3).astype(np.float32)
    Y = U * X
    kp, kn = 832, 2048
    Z = torch.zeros(2 * n, d, device="cuda")
    Z[:n], Z[n:] = dev(X), dev(Y)
    i16 = dict(dtype=torch.int16, device="cuda")
    Zh, Zl, ZTh, ZTl = (torch.full((2 * n, kp), 7, **i16), torch.full((2 * n, kp), 7, **i16), torch.full((kp, kn), 7, **i16),
                        torch.full((kp, kn), 7, **i16))
    ops.mmd_bf3_prepare(Z, 2 * n, d, Zh, Zl, ZTh, ZTl)
    zh, zl = Zh.view(torch.bfloat16).float(), Zl.view(torch.bfloat16).float()
    assert torch.equal(zh[:, :d], Z.to(torch.bfloat16).float())                       # hi = RNE bf16 of z
    assert float((zh[:, :d] + zl[:, :d] - Z).abs().max()) <= 2.0 ** -16 * float(Z.abs().max())
    assert float(zh[:, d:].abs().max()) == 0 and float(zl[:, d:].abs().max()) == 0
    assert torch.equal(ZTh[:, :2 * n], Zh.t()) and torch.equal(ZTl[:, :2 * n], Zl.t())
    # Gram + backward on the split operands against the fp64 oracle
    sq = torch.empty(2 * n, device="cuda")
    ops.row_sqnorm(Z, sq, d)
    f = orc.mmd_forward(X.astype(np.float64), Y.astype(np.float64), U.astype(np.float64), 0.0)
    bw = torch.full((1,), float(f["bw"]), device="cuda")
    tiles = ops.build_tiles(n, 1)
    partial = torch.empty(tiles.shape[0], 4, device="cuda")
    Wh, Wl = torch.zeros(n, kn, **i16), torch.zeros(n, kn, **i16)
    ops.mmd_gram_bf3(Zh, Zl, sq, n, bw, tiles, Wh, Wl, n, partial)
    stats = torch.empty(4, dtype=torch.float64, device="cuda")
    ops.mmd_reduce(partial, tiles, stats)
    st = host(stats) / (float(n) * n)
    assert abs((st[0] - 2 * st[1] + st[2]) - f["mmd2"]) < 2e-5
    np.testing.assert_allclose(st[:3], [f["xx"], f["xy"], f["yy"]], rtol=2e-5)
    out = torch.empty(n, d, device="cuda")
    ops.mmd_backward_bf3(Wh, Wl, ZTh, ZTl, Z, n, n, d, None, out)
    dY, _ = orc.mmd_backward(X.astype(np.float64), Y.astype(np.float64), U.astype(np.float64), 0.0, f["bw"])
    np.testing.assert_allclose(host(out), dY, rtol=0, atol=1e-3 * np.abs(dY).max())
    for splits in (2, 3, 40):  # split-K slabs (40 > K tiles: trailing slabs are empty and must come back zero)
        slabs = torch.full((splits, n, d), float("nan"), device="cuda")
        ops.mmd_backward_bf3(Wh, Wl, ZTh, ZTl, Z, n, n, d, None, slabs[0], splits, n * d)
        np.testing.assert_allclose(host(slabs.sum(0)), host(out), rtol=0, atol=1e-5 * float(out.abs().max()) + 1e-9)


@pytest.mark.parametrize("n,d,nr_of,tile,splits", [(1024, 784, 1, 0, 2), (300, 130, 1, 64, 1), (250, 901, 2, 64, 3), (512, 1000, 1, 128, 2),
                                                    (192, 200, 2, 128, 1)])
def test_backward_bf3_rowmajor_operand_equals_transposed_operand(ops, n, d, nr_of, tile, splits):
    """vgan_mmd_backward_bf3_rm (B fragments out of Z's ROW-MAJOR split images by ds_read_b64_tr_b16) against
    vgan_mmd_backward_bf3 on the transposed copies of the same images: the same products in the same order, so the outputs
    must be bit-identical -- 64- and 128-wide tiles, ragged row counts, feature counts that are no multiple of the tile,
    split-K slabs, gradient rows for the Y half or for all rows, multiplier with shift.
    (Per element and per slab against float64, at the tile and K edges: tests/test_mmd_bwd_bf3_gpu.py.)"""
    rng = np.random.default_rng(n + d)
    N = 2 * n
    kp, kn = (d + 63) // 64 * 64, (N + 63) // 64 * 64
    dp = (d + 3) // 4 * 4
    Z = torch.zeros(N, dp, device="cuda")
    Z[:, :d] = dev(rng.normal(size=(N, d)).astype(np.float32))
    i16 = dict(dtype=torch.int16, device="cuda")
    Zh, Zl, ZTh, ZTl = torch.zeros(N, kp, **i16), torch.zeros(N, kp, **i16), torch.zeros(kp, kn, **i16), torch.zeros(kp, kn, **i16)
    ops.mmd_bf3_prepare(Z, N, d, Zh, Zl, ZTh, ZTl)
    nr, wrow0 = (n, n) if nr_of == 1 else (N, 0)
    W = (rng.normal(size=(nr, N)) * 1e-3).astype(np.float32)
    Wt = dev(W)
    Wh, Wl = torch.zeros(nr, kn, **i16), torch.zeros(nr, kn, **i16)
    hi = Wt.to(torch.bfloat16)
    Wh[:, :N] = hi.view(torch.int16)
    Wl[:, :N] = (Wt - hi.float()).to(torch.bfloat16).view(torch.int16)
    mul = dev(rng.normal(size=(nr, dp)).astype(np.float32))
    shift = dev(rng.normal(size=(dp,)).astype(np.float32))
    a = torch.full((splits, nr, dp), float("nan"), device="cuda")
    b = torch.full((splits, nr, dp), float("nan"), device="cuda")
    ops.mmd_backward_bf3(Wh, Wl, ZTh, ZTl, Z, wrow0, nr, d, mul, a[0], splits, nr * dp, mul_shift=shift, tile=tile)
    ops.mmd_backward_bf3_rm(Wh, Wl, Zh, Zl, N, Z, wrow0, nr, d, mul, b[0], splits, nr * dp, mul_shift=shift, tile=tile)
    torch.cuda.synchronize()
    assert torch.equal(a[:, :, :d], b[:, :, :d])
    w64 = (Wh.view(torch.bfloat16).double() + Wl.view(torch.bfloat16).double())[:, :N]
    z64 = (Zh.view(torch.bfloat16).double() + Zl.view(torch.bfloat16).double())[:, :d]
    want = 2.0 * (w64.sum(1, keepdim=True) * Z[wrow0:wrow0 + nr, :d].double() - w64 @ z64) * (mul[:, :d].double() + shift[:d].double())
    got = b.sum(0)[:, :d].double()
    assert float((got - want).abs().max()) <= 2e-5 * float(want.abs().max())
    if tile != 128 and nr_of == 1:
        # the same launch carrying X-X tiles of the Gram as surplus workgroups (vgan_mmd_backward_bf3_rm_xx): the product is
        # untouched and the tiles' sums equal those of the Gram launch on the same tiles, bit for bit
        sq = torch.empty(N, device="cuda")
        ops.row_sqnorm(Z, sq, dp)
        bw = torch.full((1,), float(d), device="cuda")
        table = ops.build_tiles(n, 1)
        xx_tiles = table[(table[:, 4] & 3) == 0][-5:].contiguous()
        want_part, got_part = torch.zeros(5, 4, device="cuda"), torch.full((5, 4), float("nan"), device="cuda")
        ops.mmd_gram_bf3(Zh, Zl, sq, n, bw, xx_tiles, None, None, 0, want_part)
        c = torch.full((splits, nr, dp), float("nan"), device="cuda")
        ops.mmd_backward_bf3_rm(Wh, Wl, Zh, Zl, N, Z, wrow0, nr, d, mul, c[0], splits, nr * dp, mul_shift=shift, tile=64,
                                xx=ops.xx_job(Zh, Zl, sq, xx_tiles, bw, got_part))
        torch.cuda.synchronize()
        if tile == 64:
            assert torch.equal(c[:, :, :d], b[:, :, :d])
        assert torch.equal(got_part[:, 0], want_part[:, 0]) and float(want_part[:, 0].abs().min()) > 0


@pytest.mark.parametrize("mode", ["collapsed"])
def test_c3_step_bf16x3_vs_fp64_reference(ops, mode):
    """The metric configuration in split-bf16 mode: loss within the 1e-4 bar of the reference's fp64 value."""
    g = load_golden("f5_c3_scalars.npz")
    n, d = 1024, 784
    data = orc.synthetic_dataset("c3", rows=2048)[:n]
    z = np.random.default_rng(5).normal(size=(n, orc.latent_size(d))).astype(np.float32)
    eng, _ = make_engine(ops, orc.synthetic_generator_params(d), data, n, generator_mode=mode, mmd_precision="bf16x3")
    eng.set_epoch_batches(torch.arange(n).view(1, n))
    eng.set_noise(torch.as_tensor(z))
    eng.step()
    assert abs(float(eng.loss) - float(g["loss_f64"])) < 1e-4, float(eng.loss) - float(g["loss_f64"])
    for i in range(8):
        gn = np.sqrt((host(eng.grad_view(i)).astype(np.float64) ** 2).sum())
        np.testing.assert_allclose(gn, float(g[f"gnorm_f64_{i}"]), rtol=5e-3)
    np.testing.assert_allclose(host(eng.grad_view(6))[:8, :16], g["g6slice_f64"], rtol=0, atol=5e-3 * np.abs(g["g6slice_f64"]).max())


def test_trajectory_c2_like_bf16x3_vs_oracle(ops):
    """Six steps at d=166, batch=500 (ragged tiles) in split-bf16 mode against the fp64 oracle."""
    n, d, rows = 500, 166, 1500
    rng = np.random.default_rng(99)
    data = (rng.normal(size=(rows, d)) * rng.uniform(0.5, 2.0, size=(1, d))).astype(np.float32)
    params = orc.synthetic_generator_params(d, seed=3)
    L = orc.latent_size(d)
    eng, _ = make_engine(ops, params, data, n, nb=3, graph=True, mmd_precision="bf16x3")
    ref = orc.NoKLTrainer([p.astype(np.float64) for p in params])
    perm = np.stack([rng.permutation(rows)[:n] for _ in range(3)])
    eng.set_epoch_batches(torch.as_tensor(perm))
    for t in range(6):
        z = rng.normal(size=(n, L)).astype(np.float32)
        eng.set_noise(torch.as_tensor(z))
        eng.step()
        want = ref.step(data[perm[t % 3]].astype(np.float64), z.astype(np.float64))
        assert abs(float(eng.loss) - want["loss"]) < 1e-4, (t, float(eng.loss), want["loss"])
    for i in range(8):
        np.testing.assert_allclose(host(eng.fp.view(eng.fp.flat, i)), ref.params[i], rtol=0, atol=1e-4)


@pytest.mark.parametrize("bf3", [False, True])
def test_finalize_job_riding_in_backward_equals_standalone_finalize(ops, bf3):
    """vgan_finalize_job: the step tail executed by the surplus workgroup of a backward launch writes exactly what
    vgan_mmd_finalize writes (stats, column keys, loss, accumulators), and the backward product is unchanged."""
    n, d = 320, 200
    rng = np.random.default_rng(17)
    X = rng.normal(size=(n, d)).astype(np.float32)
    Y = (X * rng.uniform(0.2, 1.0, size=(n, d))).astype(np.float32)
    S = rng.uniform(0.0, 2.0 / d, size=(n, d)).astype(np.float32)
    Z = torch.zeros(2 * n, d, device="cuda")
    Z[:n], Z[n:] = dev(X), dev(Y)
    sq = torch.empty(2 * n, device="cuda")
    ops.row_sqnorm(Z, sq, d)
    tiles = ops.build_tiles(n, 1)
    bw = torch.full((1,), 37.0, device="cuda")
    partial = torch.empty(tiles.shape[0], 4, device="cuda")
    chunks = ops.colmax_chunks(n)
    colpart = torch.empty(chunks * d, dtype=torch.int64, device="cuda")
    if bf3:
        kp, kn = (d + 63) // 64 * 64, (2 * n + 63) // 64 * 64
        i16 = dict(dtype=torch.int16, device="cuda")
        Zh, Zl = torch.zeros(2 * n, kp, **i16), torch.zeros(2 * n, kp, **i16)
        ZTh, ZTl = torch.zeros(kp, kn, **i16), torch.zeros(kp, kn, **i16)
        Wh, Wl = torch.zeros(n, kn, **i16), torch.zeros(n, kn, **i16)
        ops.mmd_bf3_prepare(Z, 2 * n, d, Zh, Zl, ZTh, ZTl)
        ops.mmd_gram_bf3(Zh, Zl, sq, n, bw, tiles, Wh, Wl, n, partial, dev(S), 0, colpart, True)
    else:
        Wg = torch.zeros(n, 2 * n, device="cuda")
        ops.mmd_gram_colmax(Z, sq, n, d, bw, tiles, Wg, n, partial, dev(S), 0, colpart, True)

    def outputs():
        return dict(colkey=torch.zeros(d, dtype=torch.int64, device="cuda"), stats=torch.zeros(4, dtype=torch.float64, device="cuda"),
                    loss=torch.zeros(1, device="cuda"), accum=torch.full((1,), 0.5, device="cuda"),
                    counter=torch.full((1,), 41, dtype=torch.int64, device="cuda"), out=torch.zeros(2, n, d, device="cuda"))

    def backward(o, job):
        if bf3:
            ops.mmd_backward_bf3(Wh, Wl, ZTh, ZTl, Z, n, n, d, None, o["out"][0], 2, n * d, job)
        else:
            ops.mmd_backward(Wg, Z, n, n, 2 * n, d, None, o["out"][0], 2, n * d, job)

    a, b = outputs(), outputs()
    ops.mmd_finalize(partial, tiles, colpart, chunks, a["colkey"], n, d, 10.0, a["stats"], a["loss"], a["accum"], 0.25, a["counter"])
    backward(a, None)
    job = ops.finalize_job(partial, tiles, colpart, chunks, b["colkey"], n, d, 10.0, b["stats"], b["loss"], b["accum"], 0.25, b["counter"])
    backward(b, job)
    torch.cuda.synchronize()
    for k in a:
        assert torch.equal(a[k], b[k]), k
    assert int(a["counter"]) == 42 and float(a["loss"]) != 0.0


# ---- adversarial operands for the two precision modes ---------------------------------------------
def adversarial_case(name, n, d, rows, seed=0):
    """Unstandardised inputs that a 16-bit-operand Gram must survive.  Returns (data, generator params)."""
    rng = np.random.default_rng(seed + 7)
    params = orc.synthetic_generator_params(d, seed=3)
    base = rng.normal(size=(rows, d))
    if name == "offset10":        # every feature mu/sigma = 10
        data = base + 10.0
    elif name == "offset100":     # mu/sigma = 100
        data = base + 100.0
    elif name == "scales":        # unstandardised feature scales over six decades, offsets of a few sigma
        sc = 10.0 ** rng.uniform(-3, 3, size=(1, d))
        data = (base + rng.uniform(-3, 3, size=(1, d))) * sc
    elif name in ("neardup", "neardup_offset100"):
        # Y ~ X: a generator whose last layer is damped (logits vary by ~1e-3 over the batch: far above fp32 resolution, far
        # below the 5/d margin of the 1/d threshold) and whose bias masks only 5 features, so U = 1 elsewhere, the XY and YY
        # blocks nearly repeat XX and the bandwidth stays near the sigma^2 scale while (second variant) every row carries a
        # common offset of 100 sigma -- the worst case for an uncentred operand
        data = base + (100.0 if name.endswith("100") else 0.0)
        params[6] = params[6] * np.float32(5e-3)
        b4 = np.zeros(d, np.float32)
        b4[rng.choice(d, size=5, replace=False)] = -6.0
        params[7] = b4
    else:
        raise ValueError(name)
    return np.ascontiguousarray(data, dtype=np.float32), params


def oracle_step_with_decisions(params, data, z, weight, snapped, max_ties=8):
    """oracle.step_forward_backward in float64 with the `s >= 1/d` decisions of upper_softmax (Generator.py:19-21) taken from
    `snapped` (the GPU's).  With ~8e5 softmax values per batch a handful sit within fp32 rounding of the threshold, where any
    two fp32 implementations (the reference's included) may decide differently; such ties are accepted only if the float64
    value is within 1e-5 relative of 1/d, and at most `max_ties` of them."""
    p64 = [p.astype(np.float64) for p in params]
    X, z = data.astype(np.float64), z.astype(np.float64)
    logits, acts = orc.generator_forward(p64, z)
    s = orc.softmax_rows(logits)
    d = s.shape[1]
    ties = snapped != (s >= 1.0 / d)
    assert ties.sum() <= max_ties and (np.abs(s[ties] * d - 1.0) < 1e-5).all(), f"{int(ties.sum())} decisions differ beyond rounding"
    U = np.where(snapped, 1.0, s)
    f = orc.mmd_forward(X, U * X, U, weight)
    dY, dUp = orc.mmd_backward(X, U * X, U, weight, f["bw"])
    gs = np.where(snapped, 0.0, dY * X + dUp)
    dlogits = s * (gs - (gs * s).sum(axis=1, keepdims=True))
    return dict(loss=f["loss"], bw=f["bw"], grads=orc.generator_backward(p64, acts, dlogits), ties=int(ties.sum()))


ADVERSARIAL = ["offset10", "offset100", "scales", "neardup", "neardup_offset100"]


@pytest.mark.parametrize("precision", ["fp32", "bf16x3"])
@pytest.mark.parametrize("case", ADVERSARIAL)
def test_adversarial_operands_whole_step_vs_fp64(ops, case, precision):
    """One whole training step at the metric's size (n=1024, d=784) on inputs with large per-feature offsets, scales
    spanning six decades and near-duplicate [X ; Y] halves, in BOTH precision modes, against the float64 oracle: loss within
    the 1e-4 bar, bandwidth to 1e-5, every parameter gradient within 1e-3 of its largest entry.  What makes this hold is
    the centred operand (trainer.NoKLStepEngine.center) and row norms taken from the split values."""
    n, d = 1024, 784
    data, params = adversarial_case(case, n, d, rows=n)
    z = np.random.default_rng(5).normal(size=(n, orc.latent_size(d))).astype(np.float32)
    eng, _ = make_engine(ops, params, data, n, mmd_precision=precision)
    eng.set_epoch_batches(torch.arange(n).view(1, n))
    eng.set_noise(torch.as_tensor(z))
    eng.step()
    want = oracle_step_with_decisions(params, data, z, 10.0, host(eng.S) >= np.float32(1.0 / d))
    assert abs(float(eng.loss) - float(want["loss"])) < 1e-4, (float(eng.loss), float(want["loss"]))
    np.testing.assert_allclose(float(eng.bw), float(want["bw"]), rtol=1e-5)
    for i in range(8):
        ref = want["grads"][i]
        np.testing.assert_allclose(host(eng.grad_view(i)), ref, rtol=0, atol=1e-3 * max(np.abs(ref).max(), 1e-12), err_msg=f"param {i}")


# ---- a long trajectory at the metric's size against the fp32 CPU port ------------------------------
C3_TRAJ_STEPS = 200
_c3_port_cache = {}


def c3_port_trajectory():
    """200 steps of the op-for-op PyTorch-CPU port (fp32, the reference's own arithmetic) at d=784, batch=1024 on recorded
    batches and noise; computed once per session (~20 s on the GPU box's cores) and shared by both precision modes."""
    if not _c3_port_cache:
        from oracle import torch_port as port
        n, d = 1024, 784
        L = orc.latent_size(d)
        data = orc.synthetic_dataset("c3", rows=4 * n)
        params = orc.synthetic_generator_params(d)
        rng = np.random.default_rng(2024)
        idx = np.stack([rng.permutation(4 * n)[:n] for _ in range(C3_TRAJ_STEPS)])
        noise = rng.normal(size=(C3_TRAJ_STEPS, n, L)).astype(np.float32)
        mask_noise = rng.normal(size=(500, L)).astype(np.float32)
        torch.set_num_threads(max(1, min(16, len(os.sched_getaffinity(0)))))
        tr = port.PortNoKL(params)
        losses = [tr.step(torch.as_tensor(data[idx[t]]), torch.as_tensor(noise[t])) for t in range(C3_TRAJ_STEPS)]
        with torch.no_grad():
            masks = (tr.generator(torch.as_tensor(mask_noise)) >= 1.0 / d).numpy()
        _c3_port_cache.update(data=data, params=params, idx=idx, noise=noise, mask_noise=mask_noise, losses=np.array(losses),
                              masks=masks, final=[p.detach().numpy().copy() for p in tr.params], bw=float(tr.kernel.bandwidth))
    return _c3_port_cache


@pytest.mark.parametrize("precision", ["fp32", "bf16x3"])
def test_trajectory_c3_200_steps_vs_cpu_port(ops, precision):
    """200 training steps at the metric's configuration (d=784, batch=1024), HIP-graph replayed, against the fp32 CPU port
    on identical batches and noise, in both precision modes: EVERY step's loss within the 1e-4 bar (so the first step
    beyond it, if any, fails the test and is printed), the trained parameters within 2e-4, and the 500 x 784 subspace
    masks sampled from the trained generator within 0.2 % of the port's (threshold ties, cf. oracle_step_with_decisions)."""
    c = c3_port_trajectory()
    n, d = 1024, 784
    eng, _ = make_engine(ops, c["params"], c["data"], n, nb=1, graph=True, mmd_precision=precision)
    hist = torch.zeros(C3_TRAJ_STEPS, device="cuda")
    for t in range(C3_TRAJ_STEPS):
        eng.set_epoch_batches(torch.as_tensor(c["idx"][t:t + 1].astype(np.int64)))
        eng.set_noise(torch.as_tensor(c["noise"][t]))
        eng.step()
        hist[t:t + 1].copy_(eng.loss)
    diff = np.abs(host(hist) - c["losses"])
    over = np.nonzero(diff > 1e-4)[0]
    print(f"[c3 trajectory, {precision}] max |dloss| = {diff.max():.2e} at step {int(diff.argmax())}; loss {c['losses'][0]:.4f} -> "
          f"{c['losses'][-1]:.4f}; first step over the 1e-4 bar: {int(over[0]) if over.size else None}")
    assert over.size == 0, f"first divergence at step {int(over[0])}: |dloss| = {diff[over[0]]:.2e}"
    np.testing.assert_allclose(float(eng.bw), c["bw"], rtol=1e-5)
    for i in range(8):
        np.testing.assert_allclose(host(eng.fp.view(eng.fp.flat, i)), c["final"][i], rtol=0, atol=2e-4)
    logits = eng.generator_logits(torch.as_tensor(c["mask_noise"]))
    S, U = torch.empty_like(logits), torch.empty_like(logits)
    ops.upper_softmax_forward(logits, S, U)
    hamming = float(((host(U) >= np.float32(1.0 / d)) != c["masks"]).mean())
    assert hamming < 2e-3, hamming


# ---- BASELINE.json configs[3] / configs[4] at their full single-GPU sizes -------------------------------------------
def _dy_rows_fp64(Z, n, bw, rows):
    """Rows of dLoss/dY in float64 from the closed form: dY_i = (4/n^2) [sum_{j in Y} K'_ij (y_i - y_j)
    - sum_{a in X} K'_ia (y_i - x_a)], K' = dK/dL of the 5-bandwidth RBF.  O(N d) per row, so usable at any size;
    test_dy_rows_helper_matches_oracle pins it to oracle.mmd_backward."""
    Z = np.asarray(Z)
    out = []
    sc = orc.rbf_scales(bw, np.dtype(np.float64))
    for i in rows:
        zi = Z[n + i].astype(np.float64)
        diff = zi[None, :] - Z.astype(np.float64)            # [2n, d]
        L = (diff * diff).sum(1)
        dK = sum(-np.exp(-L / s) / s for s in sc)              # [2n]
        sign = np.concatenate([-np.ones(n), np.ones(n)])
        out.append((4.0 / (float(n) * n)) * ((sign * dK)[:, None] * diff).sum(0))
    return np.stack(out)


def test_dy_rows_helper_matches_oracle():
    f = load_golden("f1_ops_n64_d12.npz")
    X, U = f["X"].astype(np.float64), f["U_f64"]
    Y = U * X
    n = X.shape[0]
    bw = float(orc.mmd_forward(X, Y, U, 0.0)["bw"])
    dY, _ = orc.mmd_backward(X, Y, U, 0.0, bw)
    rows = [0, 5, n - 1]
    np.testing.assert_allclose(_dy_rows_fp64(np.vstack([X, Y]), n, bw, rows), dY[rows], rtol=1e-9, atol=1e-14)


@pytest.mark.parametrize("precision", ["fp32", "bf16x3"])
def test_c4_full_size_step_vs_fp64_oracle(ops, precision):
    """configs[3] (d=2048, batch=4096) on one GPU: loss / bandwidth of one whole step against the fp64 oracle (bar 1e-4),
    sampled rows of the backward product against the closed form, and the 8-rank row sharding of the same batch
    (tile tables of ranks 0..7) summing to the single-rank statistics."""
    n, d = 4096, 2048
    L = orc.latent_size(d)
    data = orc.synthetic_dataset("c4", rows=n)
    params = orc.synthetic_generator_params(d, seed=4)
    z = np.random.default_rng(44).normal(size=(n, L)).astype(np.float32)
    eng, _ = make_engine(ops, params, data, n, mmd_precision=precision)
    eng.set_epoch_batches(torch.arange(n).view(1, n))
    eng.set_noise(torch.as_tensor(z))
    eng.step()
    p64 = [p.astype(np.float64) for p in params]
    logits, _ = orc.generator_forward(p64, z.astype(np.float64))
    U, _ = orc.upper_softmax_forward(logits)
    X = data.astype(np.float64)
    want = orc.mmd_forward(X, U * X, U, 10.0)
    assert abs(float(eng.loss) - float(want["loss"])) < 1e-4, (float(eng.loss), float(want["loss"]))
    np.testing.assert_allclose(float(eng.bw), float(want["bw"]), rtol=1e-5)
    # backward product rows: gU = dY * X summed over the split-K slabs
    rows = [0, 1234, n - 1]
    Zh = host(eng.Z)[:, :d]
    dY = _dy_rows_fp64(Zh, n, float(want["bw"]), rows)
    gU = host(eng.gU_slabs.sum(0))[:, :d]
    np.testing.assert_allclose(gU[rows], dY * data[rows], rtol=0, atol=2e-4 * np.abs(dY * data[rows]).max())
    # data-parallel sharding of this batch over 8 ranks: per-rank block sums add up to the single-rank statistics
    single = host(eng.stats).copy()
    tot = np.zeros(4)
    st = torch.empty(4, dtype=torch.float64, device="cuda")
    for r in range(8):
        tiles = ops.build_tiles(n, 1, r, 8)
        part = torch.empty(tiles.shape[0], 4, device="cuda")
        if precision == "bf16x3":
            ops.mmd_gram_bf3(eng.Zh, eng.Zl, eng.sqn, n, eng.bw, tiles, None, None, 0, part)
        else:
            ops.mmd_gram(eng.Z, eng.sqn, n, eng.dp, eng.bw, tiles, False, None, 0, part)
        ops.mmd_reduce(part, tiles, st, True)
        tot += host(st)
    np.testing.assert_allclose(tot[:3], single[:3], rtol=1e-7)  # per-tile sums are fp32: tile shape changes their rounding


def test_c5_full_size_properties(ops):
    """configs[4] (d=4096, batch=8192, 5 kernels) on one GPU, where the oracle no longer finishes in seconds:
    (1) a generator with zero weights gives U = 1, Y = X, so the whole step must return MMD^2 = 0 and a vanishing gradient;
    (2) the fp32-MFMA and the split-bf16 kernels, two independent implementations, agree on loss, bandwidth and gradient;
    (3) sampled rows of the backward product match the float64 closed form."""
    n, d = 8192, 4096
    L = orc.latent_size(d)
    data = orc.synthetic_dataset("c5", rows=n)
    z = np.random.default_rng(55).normal(size=(n, L)).astype(np.float32)
    zero = [np.zeros_like(p) for p in orc.synthetic_generator_params(d)]
    eng, _ = make_engine(ops, zero, data, n, mmd_precision="bf16x3")
    eng.set_epoch_batches(torch.arange(n).view(1, n))
    eng.set_noise(torch.as_tensor(z))
    eng.step()
    assert abs(float(eng.loss)) < 1e-6, float(eng.loss)
    assert float(eng.gU_slabs.sum(0).abs().max()) < 1e-9
    del eng
    torch.cuda.empty_cache()
    params = orc.synthetic_generator_params(d, seed=5)
    res = {}
    for precision in ("fp32", "bf16x3"):
        eng, _ = make_engine(ops, params, data, n, mmd_precision=precision)
        eng.set_epoch_batches(torch.arange(n).view(1, n))
        eng.set_noise(torch.as_tensor(z))
        eng.step()
        res[precision] = dict(loss=float(eng.loss), bw=float(eng.bw), stats=host(eng.stats).copy(),
                              gU=host(eng.gU_slabs.sum(0))[:, :d], Z=host(eng.Z)[:, :d] if precision == "fp32" else None)
        del eng
        torch.cuda.empty_cache()
    a, b = res["fp32"], res["bf16x3"]
    assert abs(a["loss"] - b["loss"]) < 2e-6 and 0.0 < a["loss"] < 20.0
    np.testing.assert_allclose(a["bw"], b["bw"], rtol=1e-6)
    np.testing.assert_allclose(a["stats"][:3], b["stats"][:3], rtol=2e-6)
    scale = np.abs(a["gU"]).max()
    assert scale > 0 and np.abs(a["gU"] - b["gU"]).max() < 2e-4 * scale
    rows = [3, 4097, n - 1]
    dY = _dy_rows_fp64(a["Z"], n, a["bw"], rows)
    for name in ("fp32", "bf16x3"):
        np.testing.assert_allclose(res[name]["gU"][rows], dY * data[rows], rtol=0, atol=2e-4 * np.abs(dY * data[rows]).max())


@pytest.mark.parametrize("case", ["chain_c3", "ragged", "single_long_k"])
def test_gemm_grouped_vs_numpy(ops, case):
    """vgan_gemm_grouped: NN / NT / TN products of one launch against float64 numpy (shapes of the collapsed generator at
    c3, shapes that are no multiple of 4 -- the scalar staging path -- and a single tall-skinny product)."""
    rng = np.random.default_rng(31)
    T = lambda *shape: torch.as_tensor(rng.normal(size=shape).astype(np.float32)).cuda()
    if case == "chain_c3":
        e = [52, 100, 200, 396, 788]
        M4, Wt4, B3, B2, At3 = T(e[4], e[0]), T(e[4], e[3]), T(e[4], e[2]), T(e[4], e[1]), T(e[3], e[0])
        probs = [("TN", Wt4, M4), ("TN", B3, M4), ("TN", B2, M4), ("NT", M4, At3)]
    elif case == "ragged":
        probs = [("NN", T(37, 45), T(45, 70)), ("NT", T(130, 19), T(67, 19)), ("TN", T(301, 33), T(301, 9))]
    else:
        probs = [("NN", T(96, 1000), T(1000, 40))]
    full = []
    for kind, A, B in probs:
        a, b = host(A).astype(np.float64), host(B).astype(np.float64)
        want = a @ b if kind == "NN" else a @ b.T if kind == "NT" else a.T @ b
        C = torch.full(want.shape, float("nan"), device="cuda")
        full.append((kind, A, B, C, want))
    ops.gemm_grouped([(k, A, B, C) for k, A, B, C, _ in full])
    for kind, A, B, C, want in full:
        np.testing.assert_allclose(host(C), want, rtol=0, atol=2e-5 * np.abs(want).max(), err_msg=kind)
    # strided views (leading dimension > width) as the engine passes them
    big = T(64, 80)
    A, B = big[:, :52], T(40, 52)
    C = torch.zeros(64, 48, device="cuda")
    ops.gemm_grouped([("NT", A, B, C[:, :40])])
    np.testing.assert_allclose(host(C[:, :40]), host(A).astype(np.float64) @ host(B).astype(np.float64).T, rtol=0, atol=1e-4)
    assert float(C[:, 40:].abs().max()) == 0.0


def test_two_stage_logits_schedule_vs_golden(ops, monkeypatch):
    """The opt-in two-launch generator forward (VGAN_LOGITS_2STAGE=1: logits = (([z|1] . Wt_1^T) . Wt_2^T) . B_3^T with the first
    two products as one two-stage tile) against fixture F2 (c2), like the default schedule."""
    monkeypatch.setenv("VGAN_LOGITS_2STAGE", "1")
    g = load_golden("f2_step_c2.npz")
    batch, noise = g["batch"], g["noise"]
    n = batch.shape[0]
    eng, gen = make_engine(ops, [g[f"param0_{i}"] for i in range(8)], batch, n)
    assert eng.two_stage_logits
    eng.set_epoch_batches(torch.arange(n).view(1, n))
    for step in range(2):
        eng.set_noise(torch.as_tensor(noise))
        eng.step()
        assert abs(float(eng.loss) - float(g[f"loss{step}"])) < 2e-5
        for i in range(8):
            np.testing.assert_allclose(host(eng.fp.view(eng.fp.flat, i)), g[f"param{step + 1}_{i}"], rtol=0, atol=5e-6)


def test_gemm_grouped_two_stage_tile(ops):
    """vgan_gemm_problem kind NT_NT: C = (A . B^T) . D^T formed tile by tile in ONE launch (the logits' first half riding with the
    chain products), beside ordinary products, against float64 numpy -- the step's shapes, ragged shapes (rows, both inner
    dimensions and columns no multiples of the tile), and the same bits twice."""
    rng = np.random.default_rng(5)
    T = lambda *shape: torch.as_tensor(rng.normal(size=shape).astype(np.float32)).cuda()
    for (m, k, k2, n) in [(1024, 52, 100, 200), (130, 20, 36, 72), (64, 8, 132, 64), (200, 260, 516, 100)]:
        A, B, D = T(m, k), T(k2, k), T(n, k2)
        other_a, other_b = T(100, 52), T(52, 40)
        outs = []
        for rep in range(2):
            C = torch.full((m, n), float("nan"), device="cuda")
            O = torch.full((100, 40), float("nan"), device="cuda")
            ws = torch.full((((m + 63) // 64) * ((n + 63) // 64) * 64 * ((k2 + 3) // 4 * 4),), float("nan"), device="cuda")
            ops.gemm_grouped([("NN", other_a, other_b, O), ("NT2", A, B, C, D, ws)])
            outs.append((host(C).copy(), host(O).copy()))
        a, b, d = (host(x).astype(np.float64) for x in (A, B, D))
        want = (a @ b.T) @ d.T
        np.testing.assert_allclose(outs[0][0], want, rtol=0, atol=3e-5 * np.abs(want).max(), err_msg=str((m, k, k2, n)))
        np.testing.assert_allclose(outs[0][1], host(other_a).astype(np.float64) @ host(other_b).astype(np.float64), rtol=0, atol=1e-4)
        assert np.array_equal(outs[0][0], outs[1][0])


def test_gemm_grouped_split_k_slabs(ops):
    """vgan_gemm_problem.splitk: the contraction cut into slices run by different workgroups, partial products in slabs that
    vgan_reduce_slabs sums (the chain products of c4 / c5: long contraction, few output tiles).  All three kinds in one launch
    beside an unsplit product, ragged slice lengths (K no multiple of the slice), against float64 numpy; and two runs give
    the same bits (no atomics)."""
    rng = np.random.default_rng(77)
    T = lambda *shape: torch.as_tensor(rng.normal(size=shape).astype(np.float32)).cuda()
    probs = [("TN", T(1100, 260), T(1100, 132), 5), ("NN", T(516, 1028), T(1028, 132), 4), ("NT", T(200, 900), T(136, 900), 3),
             ("NT", T(260, 132), T(516, 132), 1)]
    outs = []
    for rep in range(2):
        launch, dst = [], []
        for kind, A, B, sp in probs:
            m, n = (A.shape[1] if kind == "TN" else A.shape[0]), (B.shape[0] if kind == "NT" else B.shape[1])
            if sp > 1:
                slabs = torch.full((sp, m, n), float("nan"), device="cuda")
                launch.append((kind, A, B, slabs, sp))
                dst.append((slabs, torch.empty(m, n, device="cuda"), sp))
            else:
                C = torch.full((m, n), float("nan"), device="cuda")
                launch.append((kind, A, B, C))
                dst.append((None, C, 1))
        ops.gemm_grouped(launch)
        for slabs, C, sp in dst:
            if sp > 1:
                ops.reduce_slabs(slabs, C.numel(), sp, C)
        outs.append([host(C).copy() for _, C, _ in dst])
    for (kind, A, B, sp), got, again in zip(probs, outs[0], outs[1]):
        a, b = host(A).astype(np.float64), host(B).astype(np.float64)
        want = a @ b if kind == "NN" else a @ b.T if kind == "NT" else a.T @ b
        np.testing.assert_allclose(got, want, rtol=0, atol=2e-5 * np.abs(want).max(), err_msg=f"{kind} x{sp}")
        assert np.array_equal(got, again)


@pytest.mark.parametrize("n,d,mode", [(1024, 784, 1), (384, 200, 2), (300, 130, 1), (640, 96, 2)])
def test_gram_bf3_tile128_equals_tile64(ops, n, d, mode):
    """The 128x128 and the 256x128 (loader-wave) split-bf16 Gram kernels against the 64x64 one on the same operands: same
    block sums (to fp32 summation order), same gradient weights (the hi halves bit-equal; hi + lo to the pair's 2^-16
    resolution, since the compiler contracts the epilogue's fp32 expressions differently in the kernels), same column keys --
    ragged row / column counts, mirrored stores of the symmetric blocks and of XY (mode 2), short contractions (d = 96:
    three K stages, one in the prologue only)."""
    rng = np.random.default_rng(n + d)
    Zf = torch.as_tensor(rng.normal(size=(2 * n, d)).astype(np.float32) * 0.3).cuda()
    S = torch.as_tensor(rng.uniform(0, 2.0 / d, size=(n, d)).astype(np.float32)).cuda()
    sq = torch.empty(2 * n, device="cuda")
    ops.row_sqnorm(Zf, sq, d)
    kp, kn = (d + 63) // 64 * 64, (2 * n + 63) // 64 * 64
    i16 = dict(dtype=torch.int16, device="cuda")
    Zh, Zl = torch.zeros(2 * n, kp, **i16), torch.zeros(2 * n, kp, **i16)
    ops.mmd_bf3_prepare(Zf, 2 * n, d, Zh, Zl)
    bw = torch.full((1,), float(d) * 0.2, device="cuda")
    nr, wrow0 = (n, n) if mode == 1 else (2 * n, 0)
    res = {}
    for tile in (64, 128, 256):
        tiles = ops.build_tiles(n, mode, tile=tile)
        partial = torch.zeros(tiles.shape[0], 4, device="cuda")
        Wh, Wl = torch.full((nr, kn), 0x7FC0, **i16), torch.full((nr, kn), 0x7FC0, **i16)
        colpart = torch.zeros(ops.colmax_chunks(n) * d, dtype=torch.int64, device="cuda")
        ops.mmd_gram_bf3(Zh, Zl, sq, n, bw, tiles, Wh, Wl, wrow0, partial, S, 0, colpart, True, tile=tile)
        stats = torch.zeros(4, dtype=torch.float64, device="cuda")
        ops.mmd_reduce(partial, tiles, stats, True)
        res[tile] = (host(stats), Wh[:, :2 * n].clone(), Wl[:, :2 * n].clone(), colpart.clone())
    val = lambda h, l: (h.to(torch.int32) << 16).view(torch.float32).double() + (l.to(torch.int32) << 16).view(torch.float32).double()
    a = res[64]
    for tile in (128, 256):
        b = res[tile]
        np.testing.assert_allclose(a[0][:3], b[0][:3], rtol=1e-6, err_msg=str(tile))
        assert torch.equal(a[3], b[3])
        assert not bool((a[1] == 0x7FC0).any()) and not bool((b[1] == 0x7FC0).any()), f"part of W left unwritten ({tile})"
        wa, wb = val(a[1], a[2]), val(b[1], b[2])
        assert float((wa - wb).abs().max()) <= 5e-5 * float(wa.abs().max()), tile
        assert float((a[1] != b[1]).double().mean()) < 1e-3, tile  # hi halves differ only where w sits on a bf16 rounding boundary


@pytest.mark.parametrize("n,d,mode,parts", [(1024, 520, 1, 2), (512, 4096, 2, 4), (640, 1030, 1, 4), (2304, 512, 1, 2)])
def test_gram_bf3_wide_tail_split(ops, n, d, mode, parts):
    """tile = 256 with the tail workspace (include/vgan_hip.h, tail_ws): the tiles of a short last round are computed by 2 or 4
    workgroups each, split over K, and finished by the last one to arrive.  Against the same launch without workspace:
    block sums and gradient weights to fp32 summation order, identical column keys, every W element written; the same bits
    launch after launch (the sums run in part order, whoever arrives last) and the tickets back at zero.  (2304, 512): 342 tiles =
    one full round of 256 + 86 split in two; the others have a single short round.)"""
    rng = np.random.default_rng(n + d)
    Zf = torch.as_tensor((rng.normal(size=(2 * n, d)) * (6.0 / np.sqrt(d))).astype(np.float32)).cuda()
    S = torch.as_tensor(rng.uniform(0, 2.0 / d, size=(n, d)).astype(np.float32)).cuda()
    sq = torch.empty(2 * n, device="cuda")
    ops.row_sqnorm(Zf, sq, d)
    kp, kn = (d + 63) // 64 * 64, (2 * n + 63) // 64 * 64
    i16 = dict(dtype=torch.int16, device="cuda")
    Zh, Zl = torch.zeros(2 * n, kp, **i16), torch.zeros(2 * n, kp, **i16)
    ops.mmd_bf3_prepare(Zf, 2 * n, d, Zh, Zl)
    bw = torch.full((1,), 30.0, device="cuda")  # |z_i - z_j|^2 ~ 72 whatever d: kernels well inside (0, 1)
    nr, wrow0 = (n, n) if mode == 1 else (2 * n, 0)
    tiles = ops.build_tiles(n, mode, tile=256)
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    r = tiles.shape[0] % min(cus, 256)
    assert 0 < r and parts * r <= min(cus, 256) and kp // 32 // parts >= 8, "the case does not split the way its name says"
    ws = ops.gram_tail_workspace("cuda")
    res = []
    for tail in (None, ws, ws, ws):
        partial = torch.zeros(tiles.shape[0], 4, device="cuda")
        Wh, Wl = torch.full((nr, kn), 0x7FC0, **i16), torch.full((nr, kn), 0x7FC0, **i16)
        colpart = torch.zeros(ops.colmax_chunks(n) * d, dtype=torch.int64, device="cuda")
        ops.mmd_gram_bf3(Zh, Zl, sq, n, bw, tiles, Wh, Wl, wrow0, partial, S, 0, colpart, True, tile=256, tail_ws=tail)
        stats = torch.zeros(4, dtype=torch.float64, device="cuda")
        ops.mmd_reduce(partial, tiles, stats, True)
        res.append((host(stats), Wh[:, :2 * n].clone(), Wl[:, :2 * n].clone(), colpart.clone(), partial.clone()))
    assert int(ws[-1024:].abs().sum()) == 0, "tickets not reset"
    val = lambda h, l: (h.to(torch.int32) << 16).view(torch.float32).double() + (l.to(torch.int32) << 16).view(torch.float32).double()
    a, b = res[0], res[1]
    np.testing.assert_allclose(a[0][:3], b[0][:3], rtol=1e-6)
    assert torch.equal(a[3], b[3])
    assert not bool((b[1] == 0x7FC0).any()), "part of W left unwritten"
    wa, wb = val(a[1], a[2]), val(b[1], b[2])
    assert float((wa - wb).abs().max()) <= 5e-5 * float(wa.abs().max())
    assert not torch.equal(a[4], b[4]) or parts == 1, "the split launch did not split (same bits as the whole tiles)"
    for c in res[2:]:
        assert torch.equal(b[1], c[1]) and torch.equal(b[2], c[2]) and torch.equal(b[4], c[4]), "split launch not reproducible"


@pytest.mark.parametrize("n,d,nr_of,splits", [(512, 1000, 1, 2), (300, 130, 2, 1), (1024, 2048, 1, 4), (200, 64, 1, 3)])
def test_backward_bf3_wide_tiles(ops, n, d, nr_of, splits):
    """vgan_mmd_backward_bf3_rm on 256 x 128 output tiles (GemmBF3Wide::run_bt: 8 consumer + 4 loader waves, B fragments by
    transposed LDS reads of Z's row-major images, row sums of W taken by the loader waves from the landed LDS image) against
    float64 on the same split operands and against the 64-wide kernel: ragged rows, features no multiple of the tile, split-K
    slabs, gradient rows for the Y half or all rows, multiplier with shift; twice the same bits.
    (Per element and per slab against float64, at the tile and K edges: tests/test_mmd_bwd_bf3_gpu.py.)"""
    rng = np.random.default_rng(n + d)
    N = 2 * n
    kp, kn = (d + 63) // 64 * 64, (N + 63) // 64 * 64
    dp = (d + 3) // 4 * 4
    Z = torch.zeros(N, dp, device="cuda")
    Z[:, :d] = dev(rng.normal(size=(N, d)).astype(np.float32))
    i16 = dict(dtype=torch.int16, device="cuda")
    Zh, Zl = torch.zeros(N, kp, **i16), torch.zeros(N, kp, **i16)
    ops.mmd_bf3_prepare(Z, N, d, Zh, Zl)
    nr, wrow0 = (n, n) if nr_of == 1 else (N, 0)
    Wt = dev((rng.normal(size=(nr, N)) * 1e-3).astype(np.float32))
    Wh, Wl = torch.zeros(nr, kn, **i16), torch.zeros(nr, kn, **i16)
    hi = Wt.to(torch.bfloat16)
    Wh[:, :N] = hi.view(torch.int16)
    Wl[:, :N] = (Wt - hi.float()).to(torch.bfloat16).view(torch.int16)
    mul = dev(rng.normal(size=(nr, dp)).astype(np.float32))
    shift = dev(rng.normal(size=(dp,)).astype(np.float32))
    outs = {}
    for key, tile in (("wide", 256), ("again", 256), ("t64", 64)):
        o = torch.full((splits, nr, dp), float("nan"), device="cuda")
        ops.mmd_backward_bf3_rm(Wh, Wl, Zh, Zl, N, Z, wrow0, nr, d, mul, o[0], splits, nr * dp, mul_shift=shift, tile=tile)
        outs[key] = o[:, :, :d].clone()
    torch.cuda.synchronize()
    assert torch.equal(outs["wide"], outs["again"])
    w64 = (Wh.view(torch.bfloat16).double() + Wl.view(torch.bfloat16).double())[:, :N]
    z64 = (Zh.view(torch.bfloat16).double() + Zl.view(torch.bfloat16).double())[:, :d]
    want = 2.0 * (w64.sum(1, keepdim=True) * Z[wrow0:wrow0 + nr, :d].double() - w64 @ z64) * (mul[:, :d].double() + shift[:d].double())
    got = outs["wide"].sum(0).double()
    assert float((got - want).abs().max()) <= 2e-5 * float(want.abs().max())
    assert float((got - outs["t64"].sum(0).double()).abs().max()) <= 2e-5 * float(want.abs().max())


@pytest.mark.parametrize("n,d,mode,splits", [(1024, 520, 1, 1), (640, 300, 2, 1), (1024, 2048, 1, 2), (512, 256, 1, 3), (512, 256, 1, 6)])
def test_row_sums_from_the_wide_gram(ops, n, d, mode, splits):
    """The tile-256 Gram launch leaves the row sums of the stored W per 128-column slot (rs_part), and the 256 x 128 backward
    kernel folds them instead of summing W's rows with its loader waves: every cell of rs_part equals the float64 sum of the
    stored hi + lo weights over its slot (direct and mirrored stores, the tail-split tiles, ragged last slot), and the backward
    product with rs_part equals the one without to fp32 rounding of the row sums -- two K slabs of whole slots use it, three
    slabs of 384 = 3 x 128 columns use it, six slabs of 192 columns cut the slots and fall back to the loader sums."""
    rng = np.random.default_rng(n + d)
    N = 2 * n
    dp = (d + 3) // 4 * 4
    Z = torch.zeros(N, dp, device="cuda")
    Z[:, :d] = dev((rng.normal(size=(N, d)) * (6.0 / np.sqrt(d))).astype(np.float32))
    sq = torch.empty(N, device="cuda")
    ops.row_sqnorm(Z, sq, d)
    kp, kn = (d + 63) // 64 * 64, (N + 63) // 64 * 64
    i16 = dict(dtype=torch.int16, device="cuda")
    Zh, Zl = torch.zeros(N, kp, **i16), torch.zeros(N, kp, **i16)
    ops.mmd_bf3_prepare(Z, N, d, Zh, Zl)
    bw = torch.full((1,), 30.0, device="cuda")
    nr, wrow0 = (n, n) if mode == 1 else (N, 0)
    tiles = ops.build_tiles(n, mode, tile=256)
    partial = torch.zeros(tiles.shape[0], 4, device="cuda")
    Wh, Wl = torch.zeros(nr, kn, **i16), torch.zeros(nr, kn, **i16)
    rs_part = torch.full(((N + 127) // 128, nr), float("nan"), device="cuda")
    ops.mmd_gram_bf3(Zh, Zl, sq, n, bw, tiles, Wh, Wl, wrow0, partial, tile=256, tail_ws=ops.gram_tail_workspace("cuda"), rs_part=rs_part)
    w64 = (Wh.view(torch.bfloat16).double() + Wl.view(torch.bfloat16).double())[:, :N]
    assert not bool(torch.isnan(rs_part).any()), "a slot of rs_part was left unwritten"
    pad = torch.zeros(nr, rs_part.shape[0] * 128, dtype=torch.float64, device="cuda")
    pad[:, :N] = w64
    want_rs = pad.view(nr, -1, 128).sum(2).t()
    assert float((rs_part.double() - want_rs).abs().max()) <= 4e-6 * float(want_rs.abs().max())
    mul = dev(rng.normal(size=(nr, dp)).astype(np.float32))
    outs = {}
    for key, rsp in (("loaders", None), ("gram", rs_part), ("again", rs_part)):
        o = torch.full((splits, nr, dp), float("nan"), device="cuda")
        ops.mmd_backward_bf3_rm(Wh, Wl, Zh, Zl, N, Z, wrow0, nr, d, mul, o[0], splits, nr * dp, tile=256, rs_part=rsp)
        outs[key] = o[:, :, :d].clone()
    assert torch.equal(outs["gram"], outs["again"])
    z64 = (Zh.view(torch.bfloat16).double() + Zl.view(torch.bfloat16).double())[:, :d]
    want = 2.0 * (w64.sum(1, keepdim=True) * Z[wrow0:wrow0 + nr, :d].double() - w64 @ z64) * mul[:, :d].double()
    scale = float((w64.abs().sum(1, keepdim=True) * Z[wrow0:wrow0 + nr, :d].abs().double()).max())
    for key in ("loaders", "gram"):
        assert float((outs[key].sum(0).double() - want).abs().max()) <= 1e-5 * scale, key
    kchunk = ((kn // 64 + splits - 1) // splits) * 64
    if splits == 1 or kchunk % 128 == 0:
        assert not torch.equal(outs["gram"], outs["loaders"]), "rs_part was not used (same bits as the loader sums)"
    else:
        assert torch.equal(outs["gram"], outs["loaders"]), "a K split that cuts a slot must fall back to the loader sums"


def test_two_sample_kernels_and_check_if_myopic(ops):
    """vgan_rbf_kernel_matrix / vgan_rows_dot against numpy, and check_if_myopic end to end on the GPU against the oracle's
    restatement of torch-two-sample (parity unpinned against that absent dependency)."""
    rng = np.random.default_rng(8)
    Z = rng.normal(size=(150, 28)).astype(np.float32) * 0.5
    Zd = dev(Z)
    sq = torch.empty(150, device="cuda")
    ops.row_sqnorm(Zd, sq, 28)
    K = torch.zeros(152, 152, device="cuda")
    ops.rbf_kernel_matrix(Zd, sq, 0.3, K[:150])
    want = orc.two_sample_kernel_matrix(Z[:75], Z[75:], 0.3)
    np.testing.assert_allclose(host(K)[:150, :150], want, rtol=0, atol=2e-6)
    assert float(K[:, 150:].abs().max()) == 0.0
    A, B = dev(rng.normal(size=(37, 152)).astype(np.float32)), dev(rng.normal(size=(37, 152)).astype(np.float32))
    out = torch.empty(37, dtype=torch.float64, device="cuda")
    ops.rows_dot(A, B, out)
    np.testing.assert_allclose(host(out), (host(A).astype(np.float64) * host(B)).sum(1), rtol=1e-12)
    ops.rows_dot(A, B[3:4], out, broadcast_b=True)
    np.testing.assert_allclose(host(out), (host(A).astype(np.float64) * host(B)[3]).sum(1), rtol=1e-12)

    import sys
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    from test_host_logic import _myopic_reference
    from src.vgan import VGAN_no_kl
    from src.models.Mmd_loss_constrained import MMDLossConstrained
    MMDLossConstrained.__init__.__defaults__[0].bandwidth = None
    g = load_golden("f3_traj_c1.npz")
    model = VGAN_no_kl(batch_size=128, epochs=3, seed=777)
    model.verbose = False
    model.fit(g["data"])
    df = model.check_if_myopic(g["data"], bandwidth=0.5, count=200, n_permutations=300)
    want = _myopic_reference(model, g["data"], [0.5], 200, 300)
    np.testing.assert_allclose(df.to_numpy()[0].astype(float), want, rtol=0, atol=2.0 / 300)


@pytest.mark.parametrize("n,d", [(256, 166), (192, 70)])
def test_kl_step_engine_hip_vs_cpu_provider(ops, n, d):
    """VGAN.fit's step engine (kl_trainer.KLStepEngine) at musk-like sizes: the HIP kernels against the float64 numpy
    provider of tests/cpu_ops.py on identical parameters, batches and noise -- two detector steps (encoder trainable, then
    frozen), one generator-phase step: loss terms, bandwidth and every detector parameter."""
    from cpu_ops import CpuOps
    from vgan_amd.kl_trainer import KLStepEngine
    from vgan_amd.modules import Decoder, Detector, Encoder, Generator_big
    rng = np.random.default_rng(n + d)
    L = orc.latent_size(d)
    data = (rng.normal(size=(3 * n, d)) * rng.uniform(0.5, 1.5, size=(1, d))).astype(np.float32)
    torch.manual_seed(5)
    gen0, det0 = Generator_big(L, d), Detector(L, d, Encoder, Decoder)
    for mod in (gen0, det0):
        for q in mod.parameters():
            q.data.normal_(0.0, 0.1)
    state_g, state_d = {k: v.clone() for k, v in gen0.state_dict().items()}, {k: v.clone() for k, v in det0.state_dict().items()}
    res = {}
    for name, provider, device in (("hip", ops, "cuda"), ("cpu", CpuOps(), "cpu")):
        gen, det = Generator_big(L, d), Detector(L, d, Encoder, Decoder)
        gen.load_state_dict(state_g), det.load_state_dict(state_d)
        gen, det = gen.to(device), det.to(device)
        eng = KLStepEngine(provider, gen, det, torch.as_tensor(data).to(device), n, lr_D=0.007, weight_decay=0.04, penalty_weight=10.0)
        r2 = np.random.default_rng(1)
        sums = []
        for step, (kind, enc_train) in enumerate([("d", True), ("d", False), ("g", False)]):
            idx = torch.as_tensor(r2.permutation(3 * n)[:n])
            z = torch.as_tensor(r2.normal(size=(n, L)).astype(np.float32))
            if kind == "d":
                eng.detector_step(idx, z, train_encoder=enc_train)
            else:
                eng.generator_phase_step(idx, z)
            sums.append(eng.epoch_sums())
        res[name] = (np.array(sums), float(eng.bw), [q.detach().cpu().numpy().copy() for q in det.parameters()])
    np.testing.assert_allclose(res["hip"][0], res["cpu"][0], rtol=0, atol=1e-4)
    np.testing.assert_allclose(res["hip"][1], res["cpu"][1], rtol=1e-5)
    for a, b in zip(res["hip"][2], res["cpu"][2]):
        np.testing.assert_allclose(a, b, rtol=0, atol=2e-5)


def test_kl_step_engine_c3_size_vs_port(ops):
    """VGAN.fit's step engine at the metric's size (d=784, batch=1024, L=49) against oracle/torch_port.PortKL -- the op-for-op
    autograd port of the reference's two step bodies, pinned to the reference's own run by fixture f4
    (tests/test_oracle_golden.py) -- on identical parameters, batches and noise, over 22 steps in the order a fit runs them
    (src/vgan.py:251-332): a detector epoch of four steps with the encoder still trainable, five generator-phase epochs of two
    steps (the first one freezes the detector), a SECOND detector epoch of four steps with the encoder frozen, four more
    generator-phase steps.  Every step's MMD term and squared-error terms, the bandwidth, and all sixteen detector tensors at
    the end."""
    from oracle import torch_port as port
    from vgan_amd.kl_trainer import KLStepEngine
    from vgan_amd.modules import Decoder, Detector, Encoder, Generator_big
    n, d = 1024, 784
    L = orc.latent_size(d)
    rng = np.random.default_rng(77)
    data = orc.synthetic_dataset("c3", rows=4 * n)
    gen_params = orc.synthetic_generator_params(d, seed=9)      # well-separated softmax: threshold ties are rare
    gen, det = Generator_big(L, d), Detector(L, d, Encoder, Decoder)
    with torch.no_grad():
        for q, v in zip(gen.parameters(), gen_params):
            q.copy_(torch.as_tensor(v))
        for q in det.parameters():                               # the reference's weights_init: N(0, 0.1) weights, zero bias
            q.copy_(torch.as_tensor(rng.normal(0.0, 0.1, size=tuple(q.shape)).astype(np.float32)) if q.dim() == 2 else torch.zeros_like(q))
    det_params = [q.detach().numpy().copy() for q in det.parameters()]
    tr = port.PortKL(gen_params, det_params, lr_D=0.007, weight_decay=0.04, weight=10.0)
    eng = KLStepEngine(ops, gen.cuda(), det.cuda(), dev(data), n, 0.007, 0.04, 10.0)
    torch.set_num_threads(max(1, min(16, len(os.sched_getaffinity(0)))))
    schedule = [("d", True)] * 4 + [("g", False)] * 10 + [("d", False)] * 4 + [("g", False)] * 4
    for kind, enc_train in schedule:
        idx = rng.permutation(4 * n)[:n]
        z = rng.normal(size=(n, L)).astype(np.float32)
        X, zt = torch.as_tensor(data[idx]), torch.as_tensor(z)
        if kind == "d":
            eng.detector_step(torch.as_tensor(idx), zt, train_encoder=enc_train)
            _, want_mmd, want_mse = tr.detector_step(X, zt)
        else:
            eng.generator_phase_step(torch.as_tensor(idx), zt)
            want_mmd, want_mse = tr.generator_phase_step(X, zt), None
        got_mmd, got_mse = eng.epoch_sums()
        ties = int(((host(eng.S) >= np.float32(1.0 / d)) != (tr.subspaces(zt).numpy() == 1.0)).sum())
        assert ties <= 8, ties
        assert abs(got_mmd - want_mmd) < 1e-4, (kind, enc_train, got_mmd, want_mmd)
        if want_mse is not None:
            np.testing.assert_allclose(got_mse, want_mse, rtol=1e-4)
    np.testing.assert_allclose(float(eng.bw), float(tr.kernel.bandwidth), rtol=1e-5)
    for q, ref in zip(det.parameters(), tr.det):
        np.testing.assert_allclose(host(q), ref.detach().numpy(), rtol=0, atol=2e-5)


def test_kl_resident_feed_equals_per_step_feed(ops):
    """VGAN.fit's feed on the GPU: the epoch table walked by the device-side step counter inside the captured graphs gives,
    bit for bit, the steps the per-step host feed gives; device noise + device shuffle reproduce themselves."""
    from kl_cases import kl_resident_feed_equals_per_step_feed
    kl_resident_feed_equals_per_step_feed(ops, torch.device("cuda"))


@pytest.mark.parametrize("centred", [False, True])
@pytest.mark.parametrize("n,d", [(1024, 784), (264, 1024), (72, 20), (128, 100)])
def test_mask_project_forward_bf3_equals_two_launches(ops, n, d, centred):
    """vgan_mask_project_forward_bf3 (mask/projection fused with the bf16x3 operand preparation) is bit-identical to
    vgan_mask_project_forward (norm_split) followed by vgan_mmd_bf3_prepare: S, Z, row norms, and all four split images --
    with and without the centring vector; the norms are those of the split values hi + lo."""
    rng = np.random.default_rng(n * 7 + d)
    rows_total = 3 * n
    data = dev((rng.normal(size=(rows_total, d)) + (5.0 if centred else 0.0)).astype(np.float32))
    center = torch.empty(d, device="cuda")
    ops.col_mean(data, center)
    np.testing.assert_allclose(host(center), host(data).astype(np.float64).mean(0), rtol=1e-6, atol=1e-7)
    center = center if centred else None
    logits = dev((rng.normal(size=(n, d)) * 2.0).astype(np.float32))
    perm = torch.as_tensor(np.stack([rng.permutation(rows_total)[:n] for _ in range(2)]).astype(np.int32)).cuda()
    cursor = torch.full((1,), 3, dtype=torch.int64, device="cuda")  # 3 % 2 -> second index row
    dp, kp, kn = (d + 3) // 4 * 4, (d + 63) // 64 * 64, (2 * n + 63) // 64 * 64
    i16 = dict(dtype=torch.int16, device="cuda")

    def buffers():
        return dict(S=torch.zeros(n, d, device="cuda"), Z=torch.zeros(2 * n, dp, device="cuda"), sq=torch.zeros(2 * n, device="cuda"),
                    Zh=torch.zeros(2 * n, kp, **i16), Zl=torch.zeros(2 * n, kp, **i16), ZTh=torch.zeros(kp, kn, **i16),
                    ZTl=torch.zeros(kp, kn, **i16))

    a, b = buffers(), buffers()
    sel = dict(row_cursor=cursor, row_batches=2, row_stride=n)
    ops.mask_project_forward(logits, data, perm, a["S"], None, a["Z"][:n], a["Z"][n:], a["sq"][:n], a["sq"][n:], center=center,
                             norm_split=True, **sel)
    ops.mmd_bf3_prepare(a["Z"], 2 * n, d, a["Zh"], a["Zl"], a["ZTh"], a["ZTl"])
    assert ops.bf3_fusable(n, d, logits.stride(0), data.stride(0), dp)
    ops.mask_project_forward_bf3(logits, data, perm, b["S"], b["Z"], b["sq"], b["Zh"], b["Zl"], b["ZTh"], b["ZTl"], center=center, **sel)
    torch.cuda.synchronize()
    for k in a:
        assert torch.equal(a[k], b[k]), k
    assert float(a["Z"][:n, :d].abs().sum()) > 0 and int((a["ZTh"] != 0).sum()) > 0
    # what was written: Z = [X - c ; fl(U*X) - c], sq = |hi + lo|^2
    X = host(data)[host(perm)[1]]
    c = host(center) if centred else np.zeros(d, np.float32)
    assert np.array_equal(host(a["Z"][:n, :d]), X - c)
    zhat = a["Zh"].view(torch.bfloat16).double() + a["Zl"].view(torch.bfloat16).double()
    np.testing.assert_allclose(host(a["sq"]), host((zhat * zhat).sum(1)), rtol=2e-6)


@pytest.mark.parametrize("n,d", [(1024, 784), (264, 1024), (72, 20), (128, 100)])
def test_logits_inside_the_mask_forward_launch(ops, n, d):
    """`chain=`: logits = [z|1] . At_4^T formed inside the mask / projection launch (both the fp32-mode kernel and the fused
    bf16x3 one) against the separate logits launch followed by the same kernel: softmax to fp32 rounding (the two products
    associate the sum over k differently), identical mask decisions except within rounding of the 1/d threshold, and the
    operand images / norms following from them."""
    rng = np.random.default_rng(n + 3 * d)
    L = orc.latent_size(d)
    e0 = (L + 1 + 3) // 4 * 4
    za = torch.zeros(n, e0, device="cuda")
    za[:, :L] = dev(rng.normal(size=(n, L)).astype(np.float32))
    za[:, L] = 1.0
    At4 = torch.zeros(d + 4, e0, device="cuda")
    At4[:d, :L + 1] = dev((rng.normal(size=(d, L + 1)) * 0.5).astype(np.float32))
    data = dev(rng.normal(size=(2 * n, d)).astype(np.float32))
    perm = torch.as_tensor(rng.permutation(2 * n)[:n].astype(np.int32)).cuda()
    center = torch.empty(d, device="cuda")
    ops.col_mean(data, center)
    logits = torch.empty(n, d, device="cuda")
    ops.linear_forward(za, At4[:d], None, logits)
    chain = ops.logits_chain(za, At4[:d])
    dp, kp = (d + 3) // 4 * 4, (d + 63) // 64 * 64
    i16 = dict(dtype=torch.int16, device="cuda")

    def buffers():
        return dict(S=torch.zeros(n, d, device="cuda"), Z=torch.zeros(2 * n, dp, device="cuda"), sq=torch.zeros(2 * n, device="cuda"),
                    Zh=torch.zeros(2 * n, kp, **i16), Zl=torch.zeros(2 * n, kp, **i16))

    for fused in (False, True):
        a, b = buffers(), buffers()
        if fused:
            ops.mask_project_forward_bf3(logits, data, perm, a["S"], a["Z"], a["sq"], a["Zh"], a["Zl"], None, None, center=center)
            ops.mask_project_forward_bf3(None, data, perm, b["S"], b["Z"], b["sq"], b["Zh"], b["Zl"], None, None, center=center, chain=chain)
        else:
            ops.mask_project_forward(logits, data, perm, a["S"], None, a["Z"][:n], a["Z"][n:], a["sq"][:n], a["sq"][n:], center=center)
            ops.mask_project_forward(None, data, perm, b["S"], None, b["Z"][:n], b["Z"][n:], b["sq"][:n], b["sq"][n:], center=center, chain=chain)
        torch.cuda.synchronize()
        sa, sb = host(a["S"]).astype(np.float64), host(b["S"]).astype(np.float64)
        np.testing.assert_allclose(sb, sa, rtol=5e-5, atol=1e-12)
        tau = np.float32(1.0 / d)
        flips = (host(a["S"]) >= tau) != (host(b["S"]) >= tau)
        assert flips.sum() <= 4 and (np.abs(sa[flips] * d - 1.0) < 1e-4).all(), int(flips.sum())
        same = ~flips.any(axis=1)
        assert torch.equal(a["Z"][:n], b["Z"][:n]) and torch.equal(a["sq"][:n], b["sq"][:n])          # the X half does not see the logits
        np.testing.assert_allclose(host(b["Z"][n:])[same], host(a["Z"][n:])[same], rtol=1e-4, atol=1e-6)
        np.testing.assert_allclose(host(b["sq"][n:])[same], host(a["sq"][n:])[same], rtol=1e-4)
        ref = host(za).astype(np.float64) @ host(At4[:d]).astype(np.float64).T
        want = np.exp(ref - ref.max(1, keepdims=True))
        want /= want.sum(1, keepdims=True)
        np.testing.assert_allclose(sb, want, rtol=2e-5, atol=1e-12)


def test_integration_stub_from_this_file():
    """The ctypes binding printed in INTEGRATION.md (section 2) is executed as written and checked against the oracle."""
    import re
    from conftest import REPO
    text = open(os.path.join(REPO, "INTEGRATION.md")).read()
    block = [b for b in re.findall(r"```python\n(.*?)```", text, flags=re.S) if "def mmd2" in b]
    assert len(block) == 1
    ns = {}
    cwd = os.getcwd()
    os.chdir(REPO)  # the stub opens the library by its path relative to the repository root
    try:
        exec(block[0], ns)
    finally:
        os.chdir(cwd)
    rng = np.random.default_rng(4)
    X = rng.normal(size=(200, 24)).astype(np.float32)
    Y = (X * rng.uniform(0.3, 1.0, size=X.shape)).astype(np.float32)
    loss, bw = ns["mmd2"](dev(X), dev(Y))
    want = orc.mmd_forward(X.astype(np.float64), Y.astype(np.float64), np.ones_like(X, dtype=np.float64), 0.0)
    assert abs(float(loss) - float(want["mmd2"])) < 1e-5 and abs(float(bw) / float(want["bw"]) - 1) < 1e-5
