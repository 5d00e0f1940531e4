"""CPU tier for the small kernels of the training step: pins the numpy restatements of tests/small_ops_ref.py -- the
references tests/test_small_ops_gpu.py holds the device to -- against things that are NOT this project's kernels:
the Random123 known answers (Philox), torch's bfloat16 rounding (the operand split), the library's host-side
evaluation of the shuffle, and the CpuOps provider the CPU tier runs the step engine on.

It also MEASURES the noise bar: NOISE_F32_CHAIN_ERR is the largest distance, in units of 2^-24 r, between the
Box-Muller chain evaluated op for op in numpy float32 and its float64 restatement, over the first 2^20 quads of
(seed 777, step 3).  tests/test_small_ops_gpu.py reads it from this module; the device bar is four times this value.
"""
import functools

import numpy as np
import pytest
import torch

import small_ops_ref as ref
from cpu_ops import CpuOps
from oracle import vgan_oracle as orc

SHUFFLE_N = [1, 2, 3, 4, 5, 15, 16, 17, 255, 256, 257, 5001, 65536, 65537]
SHUFFLE_KEYS = [(0, 0), (7, 3), (0xDEADBEEF12345678, 1), (0xFFFFFFFF00000001, 0x100000002), (12345, 2 ** 40 + 17)]


# ---------------------------------------------------------------------------------------------- Philox
@pytest.mark.parametrize("ctr,key,want", [
    ((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
    ((0xffffffff,) * 4, (0xffffffff, 0xffffffff), (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
    ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0), (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1)),
])
def test_philox_known_answers(ctr, key, want):
    """The three Philox4x32-10 vectors of Random123's kat_vectors."""
    got = ref.philox4x32_10([np.array([c], dtype=np.uint64) for c in ctr], *key)
    assert tuple(int(w[0]) for w in got) == want
    # vectorised: the same counter in a batch among others
    batch = [np.array([1, c, 2], dtype=np.uint64) for c in ctr]
    got = ref.philox4x32_10(batch, *key)
    assert tuple(int(w[1]) for w in got) == want


def test_noise_keying_separates_seed_step_and_stream():
    """Every word of the (seed, step, stream_id) triple reaches the generator: changing any half of any of them changes
    the draws, and the counter's high step word is not aliased to the low one."""
    base = ref.noise_words(8, 777, 3, 0)
    others = [(778, 3, 0), (777 + (1 << 32), 3, 0), (777, 4, 0), (777, 3 + (1 << 32), 0), (777, 3, 1), (777, 3, 1 << 33),
              (777, 3 << 32, 0)]
    seen = [base.tobytes()]
    for t in others:
        w = ref.noise_words(8, *t)
        assert w.tobytes() not in seen, t
        seen.append(w.tobytes())
    # seed ^ stream_id: equal XORs collide by construction -- the documented keying, restated
    assert np.array_equal(ref.noise_words(4, 5, 0, 6), ref.noise_words(4, 6, 0, 5))


# ---------------------------------------------------------------------------------------------- noise bar (measured)
def _measure_noise_chain():
    """(largest distance in units of 2^-24 r, the float64 reference draws) over the first 2^20 quads of (seed 777, step 3)"""
    nq = 1 << 20
    z, r = ref.noise_normal_ref(nq, 4, 777, 3, 0)
    z32 = ref.noise_normal_f32_chain(nq, 777, 3, 0).reshape(nq, 4).astype(np.float64)
    live = r > 0
    assert (z32[~live] == 0).all() and (z[~live] == 0).all()
    return float((np.abs(z32 - z)[live] / (2.0 ** -24 * r[live])).max()), z


@functools.lru_cache(maxsize=None)
def _noise_f32_chain_err():
    return _measure_noise_chain()[0]          # (only the scalar is kept)


def __getattr__(name):
    """NOISE_F32_CHAIN_ERR and NOISE_DEVICE_BAR are module constants measured on first use (about a second of numpy), so
    that collecting this module, or the GPU module that reads them, costs nothing.
    NOISE_F32_CHAIN_ERR: numpy's float32 libm against the float64 restatement, see the module docstring.
    NOISE_DEVICE_BAR: four times that -- logf / sqrtf / sincosf of the device may each be an ulp or two looser than
    numpy's, and the chain has four such steps."""
    if name == "NOISE_F32_CHAIN_ERR":
        return _noise_f32_chain_err()
    if name == "NOISE_DEVICE_BAR":
        return 4.0 * _noise_f32_chain_err()
    raise AttributeError(name)


def test_noise_reference_chain_error_and_moments():
    import test_small_ops_cpu as me
    err, z = _measure_noise_chain()
    print(f"noise float32 chain error: {err:.3f} x 2^-24 r  ->  device bar {4 * err:.2f}")
    assert err == me.NOISE_F32_CHAIN_ERR and me.NOISE_DEVICE_BAR == 4.0 * err
    # a float32 chain cannot be better than the rounding of its result (0.5) nor sanely worse than a dozen roundings
    assert 0.5 <= err <= 16.0, err
    assert np.isfinite(z).all()
    assert abs(z.mean()) < 2e-3 and abs(z.std() - 1.0) < 2e-3          # 4.2e6 draws: sigma of the mean is 4.9e-4
    assert abs(np.mean(z ** 4) - 3.0) < 0.02                           # kurtosis of a normal (sigma 4.8e-3)
    assert abs(np.corrcoef(z[:, 0], z[:, 1])[0, 1]) < 3e-3 and abs(np.corrcoef(z[:, 0], z[:, 2])[0, 1]) < 3e-3


def test_noise_reference_layout():
    """element 4q + e is row-major over [rows, cols]; a count that is no multiple of 4 drops the tail of the last quad"""
    a, ra = ref.noise_normal_ref(3, 5, 99, 1, 2)
    b, rb = ref.noise_normal_ref(4, 4, 99, 1, 2)
    assert np.array_equal(a.reshape(-1), b.reshape(-1)[:15]) and np.array_equal(ra.reshape(-1), rb.reshape(-1)[:15])
    u = ref.u01(np.array([0, 255, 256, 0xFFFFFFFF], dtype=np.uint64))
    assert u.dtype == np.float32 and u[0] == np.float32(2.0 ** -25) and u[1] == u[0] and u[2] == np.float32(1.5 * 2.0 ** -24)
    assert u[3] == np.float32(1.0)                                      # 16777215.5 rounds to even in float32


# ---------------------------------------------------------------------------------------------- shuffle
@functools.lru_cache(maxsize=None)
def _lib():
    from vgan_amd import lib
    return lib.load()


def _host_perm(idx, N, seed, epoch):
    L = _lib()
    return np.array([L.vgan_shuffle_index(int(i), int(N), seed & (2 ** 64 - 1), epoch & (2 ** 64 - 1)) for i in idx], dtype=np.int64)


@pytest.mark.parametrize("N", SHUFFLE_N)
def test_feistel_ref_equals_host_entry_point(N):
    idx = np.arange(N)
    for seed, epoch in SHUFFLE_KEYS:
        got = ref.feistel_perm_ref(idx, N, seed, epoch)
        assert np.array_equal(np.sort(got), idx), (N, seed, epoch)      # a bijection of [0, N)
        assert np.array_equal(got, _host_perm(idx, N, seed, epoch)), (N, seed, epoch)   # every index, every key
    if N > 5:
        assert not np.array_equal(ref.feistel_perm_ref(idx, N, 7, 3), ref.feistel_perm_ref(idx, N, 7, 4))


def test_feistel_ref_at_the_largest_train_size():
    N = 2 ** 31 - 1
    idx = np.concatenate([np.arange(100), np.random.default_rng(0).integers(0, N, size=200), [N - 1, N - 2]])
    for seed, epoch in SHUFFLE_KEYS[1:4]:
        got = ref.feistel_perm_ref(idx, N, seed, epoch)
        assert ((got >= 0) & (got < N)).all()
        assert np.array_equal(got, _host_perm(idx, N, seed, epoch))
    assert ref.feistel_half_bits(N) == 16 and ref.feistel_half_bits(1) == 1 and ref.feistel_half_bits(5) == 2
    assert ref.feistel_half_bits(65536) == 8 and ref.feistel_half_bits(65537) == 9


# ---------------------------------------------------------------------------------------------- bf16 split
def split_probe_values():
    """ties of hi in both directions, values whose lo is itself a tie, signed zeros, negatives, 1e-30 .. 1e30; no denormals"""
    base = list(ref.SPLIT_TIES)
    rng = np.random.default_rng(11)
    mags = 10.0 ** rng.uniform(-30, 30, size=4000) * rng.choice([-1.0, 1.0], size=4000)
    scaled = [v * s for v in base for s in (1.0, 2.0 ** -40, 2.0 ** 50, 3.0)]
    return np.array(base + scaled + list(mags) + list(rng.normal(size=4000)), dtype=np.float32)


def test_split_bf16_ref_equals_torch_bit_for_bit():
    x = split_probe_values()
    assert np.isfinite(x).all() and ((x == 0) | (np.abs(x) > 1e-37)).all()
    hi, lo = ref.split_bf16_ref(x)
    t = torch.as_tensor(x)
    thi = t.bfloat16()
    tlo = (t - thi.float()).bfloat16()
    assert np.array_equal(hi, thi.view(torch.int16).numpy().view(np.uint16))
    assert np.array_equal(lo, tlo.view(torch.int16).numpy().view(np.uint16))
    # the planted ties really are ties: 1 + 2^-8 goes DOWN to the even 1.0, 1 + 3 2^-8 goes UP to 1 + 2^-6
    assert ref.bf16_value(hi[0]) == 1.0 and ref.bf16_value(hi[1]) == np.float32(1 + 2.0 ** -6)
    assert ref.bf16_value(lo[7]) == np.float32(2.0 ** -9) and ref.bf16_value(lo[8]) == np.float32(2.0 ** -9 * (1 + 2.0 ** -6))
    # hi + lo keeps 16 significant bits and is an exact float32 sum
    v = ref.split_value_ref(x)
    assert np.array_equal(v.astype(np.float64), ref.bf16_value(hi).astype(np.float64) + ref.bf16_value(lo).astype(np.float64))
    nz = x != 0
    assert (np.abs(v[nz].astype(np.float64) - x[nz]) <= 2.0 ** -16 * np.abs(x[nz])).all()


def test_threshold_constant_is_the_float32_quotient():
    """upper_mask_ref takes float32(1/d) from a float64 quotient, the kernels divide in float32: the same number for
    every width the GPU file uses"""
    for d in sorted(set(ref.WIDTHS) | {2, 5, 7, 20, 166, 640}):
        assert np.float32(1.0 / d) == np.float32(1.0) / np.float32(d), d


# ---------------------------------------------------------------------------------------------- CpuOps against the restatements
def _t(a, dtype=None):
    return torch.as_tensor(np.ascontiguousarray(a), dtype=dtype)


@pytest.fixture(scope="module")
def cpu():
    return CpuOps()


def test_cpuops_gathers_agree(cpu):
    rng = np.random.default_rng(1)
    N, n, d, nb, stride = 40, 7, 10, 3, 12
    data = rng.normal(size=(N, d)).astype(np.float32)
    data[:, :4] = split_probe_values()[:4]
    table = rng.integers(0, N, size=(nb + 1) * stride).astype(np.int32)
    center = rng.normal(size=d).astype(np.float32)
    for cursor, off in [(None, 0), (0, 2), (3, 5), (2 ** 40 + 1, 1)]:
        cur = _t(np.array([cursor], dtype=np.int64)) if cursor is not None else None
        sel = ref.row_sel_ref(table, cursor, nb, stride, off, n)
        out, sq = torch.zeros(n, d), torch.zeros(n)
        cpu.gather_rows(_t(data), _t(table), out, sq, cur, nb, stride, off)
        assert np.array_equal(out.numpy(), data[sel])
        np.testing.assert_allclose(sq.numpy(), (data[sel].astype(np.float64) ** 2).sum(1), rtol=1e-6)
        for c in (None, center):
            want = data[sel] - c if c is not None else data[sel]
            Zh, Zl = torch.zeros(n, 64, dtype=torch.int16), torch.zeros(n, 64, dtype=torch.int16)
            cpu.gather_rows_split(_t(data), _t(table), _t(c) if c is not None else None, out, sq, True, Zh, Zl, cur, nb, stride, off)
            assert np.array_equal(out.numpy(), want)
            hi, lo = ref.split_bf16_ref(want)
            assert np.array_equal(Zh[:, :d].numpy().view(np.uint16), hi) and np.array_equal(Zl[:, :d].numpy().view(np.uint16), lo)
            np.testing.assert_allclose(sq.numpy(), (ref.split_value_ref(want).astype(np.float64) ** 2).sum(1), rtol=1e-6)
    sel = ref.row_sel_ref(None, None, 1, 0, 4, n)
    out = torch.zeros(n, d)
    cpu.gather_rows(_t(data), None, out, None, row_offset=4)
    assert np.array_equal(out.numpy(), data[sel]) and np.array_equal(sel, np.arange(4, 4 + n))


def test_cpuops_mask_and_colmax_agree(cpu):
    rng = np.random.default_rng(2)
    n, d = 70, 9
    S = (ref.softmax64(rng.normal(size=(n, d)) * 2)).astype(np.float32)
    S[:, 3] = S[5, 3]                                   # a tied column: the lowest row wins
    S[10, 0] = np.float32(1.0 / d)                      # exactly the threshold: not below it
    U = torch.zeros(n, d)
    cpu.mask_from_softmax(_t(S), U)
    assert np.array_equal(U.numpy(), ref.upper_mask_ref(S)) and U[10, 0] == 1.0
    for from_softmax in (True, False):
        Uin = ref.upper_mask_ref(S) if from_softmax else S
        key = torch.zeros(d, dtype=torch.int64)
        cpu.colmax(_t(S), 100, None, key, from_softmax)
        want = ref.colkey_ref(Uin, 100)
        assert np.array_equal(key.numpy().view(np.uint64), want)
        rows = ref.colkey_rows(want) - 100
        assert rows[3] == 0
        assert np.array_equal(Uin[rows, np.arange(d)], Uin.max(axis=0))
    # the float64 mask backward of CpuOps and the restatement
    g = [rng.normal(size=(n, d)).astype(np.float32) for _ in range(2)]
    keys = ref.colkey_ref(ref.upper_mask_ref(S), 100)
    slabs = _t(np.stack(g))
    dl = torch.zeros(n, d)
    cpu.mask_backward(slabs[0], _t(S), _t(keys.view(np.int64)), 10.0, 100, dl, nslabs=2, slab_stride=n * d)
    want = ref.mask_backward_ref(g, S, keys, 10.0, 100)
    np.testing.assert_allclose(dl.numpy(), want, rtol=0, atol=5e-5 * np.abs(want).max())


def test_cpuops_reductions_agree(cpu):
    rng = np.random.default_rng(3)
    n, d = 11, 13
    t, p = rng.normal(size=(n, d)).astype(np.float32), rng.normal(size=(n, d)).astype(np.float32)
    part, g = torch.zeros(3, dtype=torch.float64), torch.zeros(n, d)
    cpu.mse_grad(_t(t), _t(p), 2.0 / 143, part, g)
    df = p - t
    assert np.array_equal(g.numpy(), np.float32(2.0 / 143) * df)
    rows = (df.astype(np.float64) ** 2).sum(1)
    np.testing.assert_allclose(part.numpy(), [rows[0:4].sum(), rows[4:8].sum(), rows[8:].sum()], rtol=1e-12)
    out = torch.tensor([2.0])
    cpu.sum_f64(part, 3, 0.5, out, accumulate=True)
    np.testing.assert_allclose(float(out), 2.0 + 0.5 * rows.sum(), rtol=2.0 ** -23)
    cpu.sum_f64(part, 2, 0.5, out, accumulate=False)
    np.testing.assert_allclose(float(out), 0.5 * rows[:8].sum(), rtol=2.0 ** -23)
    slabs = rng.normal(size=(3, 20)).astype(np.float32)
    dst = torch.zeros(17)
    cpu.reduce_slabs(_t(slabs), 20, 3, dst)
    assert np.array_equal(dst.numpy(), ref.sum_slabs_f32([slabs[s, :17] for s in range(3)]))


def test_cpuops_pack_and_packed_optimiser_agree(cpu):
    rng = np.random.default_rng(4)
    W, b = rng.normal(size=(5, 3)).astype(np.float32), rng.normal(size=5).astype(np.float32)
    P = torch.full((7, 6), 9.0)
    cpu.homogeneous_pack([(_t(W), _t(b), P)])
    assert np.array_equal(P[:6, :4].numpy(), ref.homogeneous_ref(W, b)) and (P[6] == 9).all() and (P[:, 4:] == 9).all()
    W2, b2 = torch.zeros(5, 3), torch.zeros(5)
    cpu.homogeneous_pack([(W2, b2, P)], unpack=True)
    assert np.array_equal(W2.numpy(), W) and np.array_equal(b2.numpy(), b)
    # packed optimiser: mapped elements follow the float64 rule, unmapped ones (and unmapped packed offsets) are left alone
    N = 200
    pmap = rng.permutation(N).astype(np.int32)
    dead = rng.random(N) < 0.05
    dead[:2] = True
    pmap[dead] = -1
    p, gp = rng.uniform(-1, 1, size=N).astype(np.float32), (rng.normal(size=N) * 1e-3).astype(np.float32)
    sq, acc = (rng.random(N) * 1e-6).astype(np.float32), (rng.random(N) * 1e-6).astype(np.float32)
    pt, st, at, wt = _t(p.copy()), _t(sq.copy()), _t(acc.copy()), torch.full((N,), 7.0)
    cpu.adadelta_step_packed(pt, _t(pmap), _t(gp), wt, st, at, 0.007, 0.9, 1e-6, 0.04, 0.25)
    live = ~dead
    pr, sr, ar = orc.adadelta_step(p[live].astype(np.float64), gp[pmap[live]].astype(np.float64) * 0.25, sq[live].astype(np.float64),
                                   acc[live].astype(np.float64), 0.007, 0.04)
    np.testing.assert_allclose(pt.numpy()[live], pr, rtol=0, atol=2e-7)
    np.testing.assert_allclose(st.numpy()[live], sr, rtol=1e-5, atol=1e-12)
    np.testing.assert_allclose(at.numpy()[live], ar, rtol=1e-4, atol=1e-12)
    assert np.array_equal(pt.numpy()[dead], p[dead]) and np.array_equal(st.numpy()[dead], sq[dead]) and np.array_equal(at.numpy()[dead], acc[dead])
    w = wt.numpy()
    assert np.array_equal(w[pmap[live]], pt.numpy()[live])
    untouched = np.ones(N, dtype=bool)
    untouched[pmap[live]] = False
    assert (w[untouched] == 7.0).all()
