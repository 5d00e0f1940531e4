"""CPU tier for the small kernels of the training step: pins the numpy restatements of tests/small_ops_ref.py -- the
references tests/test_small_ops_gpu.py holds the device to -- against things that are NOT this project's kernels:
the Random123 known answers (Philox), torch's bfloat16 rounding (the operand split), the library's host-side
evaluation of the shuffle, and the CpuOps provider the CPU tier runs the step engine on.

It also MEASURES the noise bar: NOISE_F32_CHAIN_ERR is the largest distance, in units of 2^-24 r, between the
Box-Muller chain evaluated op for op in numpy float32 and its float64 restatement, over the first 2^20 quads of
(seed 777, step 3).  tests/test_small_ops_gpu.py reads it from this module; the device bar is four times this value.

For the mask / projection forward (tests/test_mask_forward_gpu.py) it pins mask_forward_ref to CpuOps, shows that
check_mask_forward accepts a correct float32 implementation and rejects every fault of MASK_FWD_MUTATIONS, and asserts that
the GPU module's case lists reach every kernel instantiation and keep clear of the 1/d threshold.
"""
import collections
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


# ---------------------------------------------------------------------------------------------- mask / projection forward
def _mask_case(n, d, centre, sel_mode="table3-cnb1", e0=None, planted=True):
    """the inputs of one forward case as tests/test_mask_forward_gpu.py draws them, on the host: logits with the planted rows,
    a data set, a three-batch row table with the cursor one past row_batches and row_offset 3, the planted data row"""
    from test_small_ops_gpu import edge_logits
    rng = np.random.default_rng(7 * n + d)
    lg = edge_logits(rng, n, d) if e0 is None else ref.chain_inputs(rng, n, d, e0)
    N, nb, off = n + 5, 3, 3
    stride = off + n + 2
    data = (rng.normal(size=(N, d)) * 2.0 + 0.5).astype(np.float32)
    table = rng.integers(0, N, size=(nb + 2) * stride).astype(np.int32)
    sel = dict(table=table, cursor=nb + 1, row_batches=nb, row_stride=stride, row_offset=off)
    want = ref.row_sel_ref(table, nb + 1, nb, stride, off, n)
    if planted and not centre:
        data[want[2]] = ref.planted_data_row(rng, d)
    center = rng.normal(size=d).astype(np.float32) if centre else None
    return lg, data, sel, want, center


def _check(out, lg, data, want, center, norm_split, **kw):
    S64, X, _ = ref.mask_forward_ref(lg, data, want, center)
    delta = ref.chain_delta(*lg) if isinstance(lg, tuple) else None
    return ref.check_mask_forward(out, S64, X, center, norm_split=norm_split, delta=delta, sel=want, const_rows=[2], lin_rows=[1], **kw)


MASK_FWD_MUTATION_CASES = [  # mutation, n, d, centre, norm_split
    ("ragged chunk left out of the sum", 8, 260, True, False), ("ragged chunk left out of the sum", 8, 516, True, False),
    ("ragged chunk left out of the sum", 8, 772, False, True),
    # (the true maximum of the 200-wide row lies 100 above the first chunk's: expf overflows and the row is NaN; at d = 260 the
    # first chunk's maximum is within 3.1 of it and the fault changes roundings only)
    ("row max over the first chunk", 8, 516, True, False), ("row max over the first chunk", 8, 1024, False, True),
    ("norms of unsplit values", 8, 64, False, True), ("norms of unsplit values", 8, 1024, False, True),
    ("centre kept where U == 1", 8, 20, True, False), ("selector without the cursor modulo", 8, 20, True, True),
    ("selector without row_offset", 8, 20, False, False), ("row group unwritten", 72, 8, True, True), ("hi and lo swapped", 16, 12, True, True),
    ("transposed image shifted by a row group", 16, 12, False, True), ("<= in the mask", 8, 20, True, False), ("<= in the mask", 8, 784, False, True),
]


def test_every_mask_forward_mutation_is_listed():
    assert {m for m, *_ in MASK_FWD_MUTATION_CASES} == set(ref.MASK_FWD_MUTATIONS)


@pytest.mark.parametrize("mutation,n,d,centre,norm_split", MASK_FWD_MUTATION_CASES)
def test_check_mask_forward_accepts_the_restatement_and_rejects_each_mutation(mutation, n, d, centre, norm_split):
    """check_mask_forward on the emulated outputs of a correct float32 implementation passes (whole and with every optional
    output left out); on the outputs of each fault of MASK_FWD_MUTATIONS it raises"""
    lg, data, sel, want, center = _mask_case(n, d, centre)
    good = ref.emulate_mask_forward(lg, data, center=center, norm_split=norm_split, **sel)
    worst = _check(good, lg, data, want, center, norm_split)
    assert set(worst) == {"S", "near", "Zy", "sqx", "sqy"} and all(v <= 1.0 for v in worst.values())
    lean = {k: good[k] for k in ("S", "sqy", "Zh", "Zl")}                   # write_x = 0, write_z = 0
    _check(lean, lg, data, want, center, norm_split, z_from=dict(Zx=good["Zx"], Zy=good["Zy"]), x_half=False)
    bad = ref.emulate_mask_forward(lg, data, center=center, norm_split=norm_split, mutation=mutation, **sel)
    with pytest.raises(AssertionError):
        _check(bad, lg, data, want, center, norm_split)


def test_check_mask_forward_on_in_launch_logits():
    """the chain bar: float32 products of za . At4^T summed in another order pass; a k column left out does not"""
    n, d, e0 = 8, 260, 20
    lg, data, sel, want, center = _mask_case(n, d, True, e0=e0)
    za, At = lg
    lg32 = np.zeros((n, d), dtype=np.float32)
    for k in range(e0):                                              # an fma-free float32 chain: two roundings per term
        lg32 += za[:, k:k + 1] * At[None, :, k]
    good = ref.emulate_mask_forward(lg32, data, center=center, **sel)
    assert _check(good, lg, data, want, center, False)["S"] <= 1.0
    short = ref.emulate_mask_forward((za[:, 1:], At[:, 1:]), data, center=center, **sel)
    with pytest.raises(AssertionError):
        _check(short, lg, data, want, center, False)


@pytest.mark.parametrize("n,d", [(8, 20), (5, 260)])
def test_mask_forward_ref_agrees_with_cpuops(cpu, n, d):
    """The two test-side statements of the forward do not drift.  CpuOps rounds u * x to float32 before it subtracts c, the
    restatement (and the kernels' fma) round once: the difference is one rounding of u * x, so the pin gets 2^-24 |u x| on
    top of the one-rounding bar."""
    lg, data, sel, want, center = _mask_case(n, d, True)
    S64, X, Xc = ref.mask_forward_ref(lg, data, want, center)
    S, U, Zx, Zy, sqx, sqy = torch.zeros(n, d), torch.zeros(n, d), torch.zeros(n, d + 4), torch.zeros(n, d + 4), torch.zeros(n), torch.zeros(n)
    cpu.mask_project_forward(_t(lg), _t(data), _t(sel["table"]), S, U, Zx, Zy, sqx, sqy, _t(np.array([sel["cursor"]], dtype=np.int64)),
                             sel["row_batches"], sel["row_stride"], sel["row_offset"], center=_t(center), norm_split=True)
    np.testing.assert_allclose(S.numpy(), S64, rtol=2e-5, atol=2.0 ** -126)
    u = U.numpy()
    assert np.array_equal(u, ref.upper_mask_ref(S.numpy()))
    assert np.array_equal(Zx[:, :d].numpy(), Xc) and (Zx[:, d:] == 0).all()
    ux = u.astype(np.float64) * X.astype(np.float64)
    wantzy = ux - center.astype(np.float64)
    bar = 2.0 ** -24 * np.abs(wantzy) * (1 + 2.0 ** -20) + 2.0 ** -149 + 2.0 ** -24 * np.abs(ux)
    assert (np.abs(Zy[:, :d].numpy().astype(np.float64) - wantzy) <= bar).all()
    for sq, rows in ((sqx, Zx), (sqy, Zy)):
        np.testing.assert_allclose(sq.numpy(), (ref.split_value_ref(rows[:, :d].numpy()).astype(np.float64) ** 2).sum(1), rtol=1e-6)
    # the emulated outputs are the restatement's own: they pass its check with room to spare
    assert ref.emulate_mask_forward(lg, data, center=center, norm_split=True, **sel)["xrow"].tolist() == want.tolist()


def test_expected_kernel_known_answers():
    ek = ref.expected_kernel
    assert ek("fwd", 784, 1024, [0], [784, 784, 784]) == "vec<4>" and ek("fwd", 784, 5, [0, 4], [784]) == "generic"
    assert ek("fwd", 166, 512, [0], [168]) == "generic" and ek("fwd", 4096, 3, [0], [4096]) == "vec<16>" and ek("fwd", 4100, 3, [0], [4100]) == "generic"
    assert ek("fwd", 1028, 8, [0], [1028], chain=True) == "invalid" and ek("fwd", 1024, 8, [0], [1028], chain=True) == "vec_chain<4>"
    assert ek("fwd", 260, 5, [0], [261]) == "generic" and ek("fwd", 260, 5, [0], [261], chain=True) == "invalid"
    assert ek("bf3", 784, 1024, [0], [784], zt=True) == "bf3<4,zt>" and ek("bf3", 784, 1024, [0], [784]) == "split<4>"
    assert ek("bf3", 256, 8, [0], [256]) == "bf3<1,lean>" and ek("bf3", 260, 8, [0], [260]) == "split<2>"
    assert ek("bf3", 260, 8, [0], [260], chain=True) == "bf3_chain<2>" and ek("bf3", 260, 8, [0], [260], chain=True, zt=True) == "invalid"
    assert ek("bf3", 260, 12, [0], [260]) == "invalid" and ek("bf3", 1028, 8, [0], [1028]) == "invalid"


def test_the_mask_forward_gpu_cases_reach_every_kernel():
    """The dispatch rule of csrc/rows.hip restated (expected_kernel) over the GPU module's case lists: all 23 instantiations are
    reached -- each test there re-derives the name from the buffers it really passes -- so that the edges stay visited, or
    this test says so, if the dispatch changes."""
    import test_mask_forward_gpu as g
    reached = collections.Counter([g.fwd_dispatch(c) for c in g.FWD_CASES] + [g.bf3_dispatch(c) for c in g.BF3_CASES])
    assert len(ref.MASK_FWD_KERNELS) == 23 and set(reached) == set(ref.MASK_FWD_KERNELS), sorted(set(ref.MASK_FWD_KERNELS) ^ set(reached))
    assert g.fwd_dispatch(g.FWD_CHAIN_INVALID) == "invalid"
    # every unaligned view falls back to the generic kernel; the opt-in boundaries of the dynamic LDS are visited on both sides
    assert all(g.fwd_dispatch(c) == "generic" for c in g.FWD_PATHS) and len({c.d for c in g.FWD_PATHS}) == 6
    for cases in (g.FWD_CHAIN, g.BF3_ZT, g.BF3_CHAIN):
        assert {1016, 1020, 1024} <= {c.d for c in cases}
    assert {c.n // 8 for c in g.BF3_ZT} == {1, 2, 9, 17} and {c.n for c in g.FWD_CHAIN} == {5, 8}


def test_the_mask_forward_gpu_cases_keep_clear_of_the_threshold():
    """Every GPU case's logits, on the host: each random row has mask entries on both sides of 1/d (d > 1) and at most 0.5 % of
    a case's random-row entries lie within 1e-4 of the threshold, where the float64 decision is not asserted."""
    import test_mask_forward_gpu as g
    worst = 0.0
    for c in g.FWD_CASES + g.BF3_CASES:
        assert np.float32(1.0 / c.d) == np.float32(1.0) / np.float32(c.d), c.d   # (upper_mask_ref's threshold is the kernels')
        _, lg = g.case_logits(c)
        S64 = ref.mask_forward_ref(lg, np.zeros((1, c.d), dtype=np.float32), [0])[0]
        rand = np.ones(c.n, dtype=bool)
        rand[[1, 2] if c.n >= 3 else []] = False
        if c.d == 1 or not rand.any():
            continue
        below = S64[rand] * c.d < 1.0
        assert below.any(1).all() and (~below).any(1).all(), c
        near = float((np.abs(S64[rand] * c.d - 1.0) <= 1e-4).mean())
        assert near <= 0.005, (c, near)
        worst = max(worst, near)
    print(f"largest share of threshold-near entries over the GPU cases: {worst:.4%}")
