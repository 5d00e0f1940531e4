"""GPU tier for the small kernels of the training step -- the row, feed, reduction and optimiser kernels of
csrc/rows.hip, optim.hip, feed.hip, twosample.hip and row_sqnorm / col_mean of mmd.hip -- each called DIRECTLY through
vgan_amd.ops.HipOps at tile, vector-width and grid-cap edges and compared with the plain numpy restatements of
tests/small_ops_ref.py (which tests/test_small_ops_cpu.py pins without a GPU).  Run with ``-m gpu`` on an MI355X.

Conventions
  * Sentinels.  Every output lives in a padded allocation with a guard band on either side, filled with NaN (float) or
    -1 / 0x5A5A (integer); every test asserts that nothing outside the contracted region changed (class Guarded).  The
    pads of INPUTS hold NaN too, so a kernel that reads past a row poisons its result.
  * Paths.  Where an entry point picks a 16-byte-per-lane kernel or a scalar one, every shape runs on both: "aligned"
    (multiple-of-4 leading dimensions, 16-byte aligned bases), "shifted" (the view starts one float into its allocation)
    and "oddld" (a leading dimension that is no multiple of 4).  Unaligned views are legal inputs of the ABI.
  * Shapes.  n in {1, 3, 4, 5, 63, 64, 65, 130, 1024}, d in {1, 3, 4, 63, 64, 65, 252, 256, 260, 784, 1024, 1028, 2048,
    4096, 4100, 1500} (+ 640, the one width with three float4 per lane): the union of the edges, not the product.

Bars (each derived, or the project's own, never fitted to the device's output)
  bit-equal      gathers (float32 x - c), bf16 split images, mask-from-softmax, column keys, mse_grad's g (one float32
                 product), reduce_slabs (float32 sum in ascending slab order), pack / unpack, shuffle, copies, and every
                 "same work through another launch" comparison (vec against scalar path, riders against stand-alone).
  sq             (ceil(d/64) + 8) 2^-23 relative to the float64 sum of squares: a lane adds ceil(d/64) terms (one rounding of
                 2^-24 per fma, fewer on the vector path), the wave butterfly adds 6, the result is rounded once.
  softmax S      rtol 2e-5 (the project's op-level bar, tests/test_hip_parity.py) + atol 2^-126 (below the smallest normal
                 float32 a result has no relative precision left, and may be flushed).
  decisions      equal to the float64 ones wherever |S d - 1| > 1e-4 (the project's convention); U is bit-equal to the mask
                 of the kernel's OWN S everywhere.
  mask backward  5e-5 max|want| (the project's), against a float64 restatement that takes the float32 decisions S < 1/d
                 from the input S and sums the slabs in float32 ascending order, as the contract says.
  mse, sum_f64   2^-23 |want|: float64 accumulation (error ~1e-16 n), ONE rounding to float32 (2^-24), one more with
                 accumulate (inputs are non-negative, so the partial results do not cancel).
  mse_grad part  1e-12 relative: a float64 sum of at most 4 x 4100 non-negative terms in another order (4e-16 sqrt-ish).
  col_mean       2^-23 |want| + 2^-40 mean|x_j|: float64 accumulation of float32 data, one division, one rounding.
  rows_dot       1e-12 sum|a b|: float64 products (exact) summed in another order.
  Adadelta       the project's one-step bars against the float64 oracle (p atol 2e-7, sq rtol 1e-5, acc rtol 1e-4, both with
                 atol 1e-12); three times them after three steps.  The p bar is absolute, and half an ulp of a float32 in
                 [4, 8) is already 2.4e-7: no kernel can meet 2e-7 there.  So those tests draw the parameters from
                 [-1.5, 1.5] (a generator's weights are below 1) and NEVER run the optimiser on |p| >= 2 -- the inputs
                 are narrowed, the bar is not widened.  test_adadelta_step_large_parameters covers |p| in [2, 8) with the
                 same sq / acc bars and an ulp-scaled p bar per step of 2^-24 |p| + 1e-7: the rounding of the final fma
                 (half an ulp <= 2^-24 |p|) plus what the project's 2e-7 leaves for everything else once its own half ulp
                 at |p| < 1.5 (9e-8) is taken out; below 1.5 it is tighter than 2e-7.
  noise          |got - want| <= NOISE_DEVICE_BAR 2^-24 r element-wise with r the Box-Muller radius.  The constant is
                 MEASURED from the reference alone by tests/test_small_ops_cpu.py: the float32 chain of numpy against the
                 float64 restatement is off by at most NOISE_F32_CHAIN_ERR = 3.51 (x 2^-24 r) over the first 2^20 quads of
                 (seed 777, step 3); the device gets four times that, 14.05, because its logf / sqrtf / sincosf may each be
                 an ulp or two looser than numpy's and the chain has four such steps.
"""
import numpy as np
import pytest
import torch

import small_ops_ref as ref
from oracle import vgan_oracle as orc
import test_small_ops_cpu as cpu_tier  # NOISE_F32_CHAIN_ERR / NOISE_DEVICE_BAR: measured there, on first use
from test_small_ops_cpu import SHUFFLE_KEYS, SHUFFLE_N

pytestmark = pytest.mark.gpu

GUARD = 64  # elements of guard band on either side of every allocation (keeps 16-byte alignment for every dtype used)
PATHS = ["aligned", "shifted", "oddld"]
SHAPES = [(1, 1), (3, 3), (4, 4), (5, 63), (63, 64), (64, 65), (65, 252), (130, 256), (1024, 260), (5, 784), (4, 1024), (3, 1028),
          (5, 2048), (3, 4096), (4, 4100), (63, 1500), (5, 640)]
assert {n for n, _ in SHAPES} == set(ref.N_EDGES) and {d for _, d in SHAPES} == set(ref.WIDTHS) | {640}


@pytest.fixture(scope="module")
def ops():
    from vgan_amd.ops import HipOps
    return HipOps()


def host(t):
    return t.detach().cpu().numpy()


def dev(a, dtype=None):
    return torch.as_tensor(np.ascontiguousarray(a), dtype=dtype).to("cuda")


def round4(v):
    return (v + 3) // 4 * 4


def ld_for(d, path, extra=4):
    """a leading dimension > d: a multiple of 4 unless the path is "oddld" (then = 1 mod 4)"""
    return round4(d) + extra + (1 if path == "oddld" else 0)


def shift_for(path):
    return 1 if path == "shifted" else 0


class Guarded:
    """A [rows, cols] view with row stride ld inside a sentinel-filled allocation [guard | shift | rows x ld | guard]."""

    def __init__(self, rows, cols, ld=None, dtype=torch.float32, shift=0, data=None):
        ld = cols if ld is None else ld
        assert ld >= cols
        self.rows, self.cols, self.ld, self.start, self.dtype = rows, cols, ld, GUARD + shift, dtype
        self.fill = float("nan") if dtype.is_floating_point else (0x5A5A if dtype == torch.int16 else -1)
        self.buf = torch.full((self.start + rows * ld + GUARD,), self.fill, dtype=dtype, device="cuda")
        self.t = self.buf.as_strided((rows, cols), (ld, 1), self.start)
        assert self.t.data_ptr() % 16 == (shift * self.buf.element_size()) % 16
        if data is not None:
            self.t.copy_(dev(data, dtype))
        self.before = host(self.buf).copy()

    @property
    def flat(self):
        """the contiguous 1-D view of a one-row allocation"""
        assert self.rows == 1
        return self.buf[self.start:self.start + self.cols]

    def _inside(self, rows, cols):
        m = np.zeros(self.buf.numel(), dtype=bool)
        for r in range(self.rows if rows is None else rows):
            m[self.start + r * self.ld:self.start + r * self.ld + (self.cols if cols is None else cols)] = True
        return m

    def check(self, rows=None, cols=None, written=True):
        """Host copy of the contracted region [rows, cols] after asserting that every element outside it still holds what
        it held before the call (the sentinel, or the input's pad).  written: the region itself holds no sentinel."""
        h = host(self.buf)
        m = self._inside(rows, cols)
        assert np.array_equal(h[~m].view(np.uint8), self.before[~m].view(np.uint8)), "write outside the contracted region"
        rows, cols = (self.rows if rows is None else rows), (self.cols if cols is None else cols)
        out = h[m].reshape(rows, cols)
        if written and self.dtype.is_floating_point:
            assert not np.isnan(out).any(), "contracted region not fully written"
        return out

    def untouched(self):
        assert np.array_equal(host(self.buf).view(np.uint8), self.before.view(np.uint8)), "buffer was written"


def sq_bar(d):
    return (-(-d // 64) + 8) * 2.0 ** -23


def assert_sq(got, vals32, d):
    want = (np.asarray(vals32, dtype=np.float32).astype(np.float64) ** 2).sum(axis=1)
    err = np.abs(got.astype(np.float64) - want)
    assert (err <= sq_bar(d) * want).all(), (float((err / np.maximum(want, 1e-300)).max()), sq_bar(d))


def make_data(rng, N, d, path):
    """data set [N, d] holding the split probes in its leading columns, in a guarded allocation on the given path"""
    x = (rng.normal(size=(N, d)) * 2.0 + 0.5).astype(np.float32)
    k = min(d, len(ref.SPLIT_TIES))
    x[:, :k] = np.asarray(ref.SPLIT_TIES[:k], dtype=np.float32) * np.float32(2.0) ** rng.integers(-3, 4, size=(N, 1)).astype(np.float32)
    x[0, :k] = ref.SPLIT_TIES[:k]
    return x, Guarded(N, d, ld_for(d, path), shift=shift_for(path), data=x)


class Sel:
    """one RowSel configuration: the device arguments and the restated row indices"""

    def __init__(self, rng, N, n, mode):
        self.kw, self.table, self.cursor = dict(row_cursor=None, row_batches=1, row_stride=0, row_offset=0), None, None
        if mode.startswith("identity"):
            off = 0 if mode == "identity0" else N - n
            self.kw["row_offset"] = off
            self.want = ref.row_sel_ref(None, None, 1, 0, off, n)
            return
        nb = 1 if mode.startswith("table1") else 3
        off = 0 if mode.endswith("off0") else 3
        stride = off + n + 2
        # (two batches more than row_batches: a selector that forgot the modulo still reads inside the table)
        table = rng.integers(0, N, size=(nb + 2) * stride).astype(np.int32)
        cursor = {"none": None, "c0": 0, "cnb": nb, "cnb1": nb + 1, "huge": 2 ** 40 + 1}[mode.split("-")[1]]
        self.table = dev(table, torch.int32)
        self.cursor = dev(np.array([cursor], dtype=np.int64)) if cursor is not None else None
        self.kw = dict(row_cursor=self.cursor, row_batches=nb, row_stride=stride, row_offset=off)
        self.want = ref.row_sel_ref(table, cursor, nb, stride, off, n)


SEL_MODES = ["identity0", "identityN", "table1-none-off0", "table1-cnb1", "table3-none", "table3-c0", "table3-cnb", "table3-cnb1-off0",
             "table3-huge"]


# ================================================================================================ gather
@pytest.mark.parametrize("path", PATHS)
@pytest.mark.parametrize("n,d", SHAPES)
def test_gather_rows_and_split_at_edge_shapes(ops, n, d, path):
    """out bit-equal to data[sel] (- center), Zh / Zl bit-equal to the restated split with the columns d..kp untouched, sq
    within its bar of the float64 sum -- of the split values with norm_split; table selection with a device cursor."""
    rng = np.random.default_rng(1000 * n + d)
    N = n + 5
    x, data = make_data(rng, N, d, path)
    sel = Sel(rng, N, n, "table3-cnb1")
    ldo, kp, sh = ld_for(d, path, 8), ld_for(d, path, 12) + (2 if path == "oddld" else 0), shift_for(path)
    # vgan_gather_rows
    out, sq = Guarded(n, d, ldo, shift=sh), Guarded(1, n)
    ops.gather_rows(data.t, sel.table, out.t, sq.flat, **sel.kw)
    assert np.array_equal(out.check().view(np.uint32), x[sel.want].view(np.uint32))
    assert_sq(sq.check()[0], x[sel.want], d)
    data.untouched()
    # vgan_gather_rows_split: centred, plain norms; then uncentred (the planted ties survive), norms of the split values
    center = rng.normal(size=d).astype(np.float32)
    cg = Guarded(1, d, data=center[None])
    for c, cdev, norm_split in ((center, cg.flat, False), (None, None, True)):
        want = (x[sel.want] - c) if c is not None else x[sel.want]
        out, sq = Guarded(n, d, ldo, shift=sh), Guarded(1, n)
        Zh, Zl = Guarded(n, d, kp, torch.int16, shift=2 * sh), Guarded(n, d, kp, torch.int16, shift=2 * sh)
        ops.gather_rows_split(data.t, sel.table, cdev, out.t, sq.flat, norm_split, Zh.t, Zl.t, n=n, **sel.kw)
        assert np.array_equal(out.check().view(np.uint32), want.view(np.uint32))
        hi, lo = ref.split_bf16_ref(want)
        assert np.array_equal(Zh.check(written=False).view(np.uint16), hi), "hi image"
        assert np.array_equal(Zl.check(written=False).view(np.uint16), lo), "lo image"
        assert_sq(sq.check()[0], ref.split_value_ref(want) if norm_split else want, d)
    data.untouched()


@pytest.mark.parametrize("kernel", ["gather_rows", "split_vec", "split_scalar"])
@pytest.mark.parametrize("mode", SEL_MODES)
def test_row_selection_modes(ops, kernel, mode):
    """RowSel against its restatement: identity with an offset; a row table with row_stride / row_offset and 1 or 3 batches;
    no cursor, a device cursor at 0, at row_batches, one past it, and at 2^40 + 1 (the modulo is taken in 64 bits)."""
    rng = np.random.default_rng(len(mode) * 7 + len(kernel))
    n, d, N = 37, (63 if kernel == "split_scalar" else 64), 90
    x, data = make_data(rng, N, d, "aligned")
    sel = Sel(rng, N, n, mode)
    out, sq = Guarded(n, d, d + 4), Guarded(1, n)
    if kernel == "gather_rows":
        ops.gather_rows(data.t, sel.table, out.t, sq.flat, **sel.kw)
    else:
        ops.gather_rows_split(data.t, sel.table, None, out.t, sq.flat, False, None, None, n=n, **sel.kw)
    assert np.array_equal(out.check().view(np.uint32), x[sel.want].view(np.uint32))
    assert_sq(sq.check()[0], x[sel.want], d)


@pytest.mark.parametrize("d,path", [(260, "aligned"), (260, "shifted"), (63, "aligned")])
@pytest.mark.parametrize("combo", [1, 2, 3, 4, 5, 6, 7])
def test_gather_rows_split_optional_outputs(ops, d, path, combo):
    """every combination of the optional outputs (out = 1, sq = 2, Zh / Zl = 4) the ABI allows, with and without norm_split;
    vgan_gather_rows with sq = None"""
    rng = np.random.default_rng(combo * 100 + d)
    n, N = 65, 80
    x, data = make_data(rng, N, d, path)
    center = rng.normal(size=d).astype(np.float32)
    cdev = dev(center)
    sel = Sel(rng, N, n, "table3-cnb1")
    want = x[sel.want] - center
    hi, lo = ref.split_bf16_ref(want)
    for norm_split in (False, True):
        out = Guarded(n, d, d + 8, shift=shift_for(path)) if combo & 1 else None
        sq = Guarded(1, n) if combo & 2 else None
        Zh, Zl = (Guarded(n, d, round4(d) + 4, torch.int16), Guarded(n, d, round4(d) + 4, torch.int16)) if combo & 4 else (None, None)
        ops.gather_rows_split(data.t, sel.table, cdev, out.t if out else None, sq.flat if sq else None, norm_split,
                              Zh.t if Zh else None, Zl.t if Zl else None, n=n, **sel.kw)
        if out:
            assert np.array_equal(out.check().view(np.uint32), want.view(np.uint32))
        if sq:
            assert_sq(sq.check()[0], ref.split_value_ref(want) if norm_split else want, d)
        if Zh:
            assert np.array_equal(Zh.check(written=False).view(np.uint16), hi) and np.array_equal(Zl.check(written=False).view(np.uint16), lo)
    if combo == 1:
        out = Guarded(n, d, d + 8)
        ops.gather_rows(data.t, sel.table, out.t, None, **sel.kw)
        assert np.array_equal(out.check().view(np.uint32), x[sel.want].view(np.uint32))
    data.untouched()


# ================================================================================================ softmax / mask
def edge_logits(rng, n, d):
    x = (rng.normal(size=(n, d)) * 2.0).astype(np.float32)
    if n >= 3:
        x[1] = np.linspace(-100.0, 100.0, d, dtype=np.float32)   # a 200-wide spread: the small S underflow to 0
        x[2] = np.float32(1.25)                                   # a constant row: every S is 1/d up to rounding
    return x


@pytest.mark.parametrize("path", ["aligned", "oddld"])
@pytest.mark.parametrize("n,d", SHAPES)
def test_upper_softmax_forward_at_edge_shapes(ops, n, d, path):
    rng = np.random.default_rng(7 * n + d)
    x = edge_logits(rng, n, d)
    lg = Guarded(n, d, ld_for(d, path), data=x)
    S, U = Guarded(n, d), Guarded(n, d)
    ops.upper_softmax_forward(lg.t, S.t, U.t)
    s, u = S.check(), U.check()
    want = ref.softmax64(x)
    np.testing.assert_allclose(s, want, rtol=2e-5, atol=2.0 ** -126)
    assert np.array_equal(u.view(np.uint32), ref.upper_mask_ref(s).view(np.uint32)), "U is not the mask of the stored S"
    clear = np.abs(want * d - 1.0) > 1e-4
    assert np.array_equal((u == 1)[clear], (want >= 1.0 / d)[clear])
    if n >= 3:
        if d >= 64:
            assert (s[1] == 0).any() and s[1].argmax() == d - 1
        np.testing.assert_allclose(s[2], 1.0 / d, rtol=2.0 ** -22)
    lg.untouched()
    S2 = Guarded(n, d)
    ops.upper_softmax_forward(lg.t, S2.t, None)                  # U = None is accepted
    assert np.array_equal(S2.check().view(np.uint32), s.view(np.uint32))


@pytest.mark.parametrize("n,d", [(1, 1), (5, 3), (65, 64), (130, 65), (3, 4100), (64, 784)])
def test_mask_from_softmax_bit_exact_padded(ops, n, d):
    rng = np.random.default_rng(n + d)
    tau = np.float32(1.0 / d)
    near = np.array([np.nextafter(tau, np.float32(0)), tau, np.nextafter(tau, np.float32(2)), 0.0, 1.0, tau * np.float32(0.5)], dtype=np.float32)
    s = np.where(rng.random((n, d)) < 0.5, rng.choice(near, size=(n, d)), (rng.random((n, d)) * 2.0 / d).astype(np.float32)).astype(np.float32)
    S = Guarded(n, d, d + 3, data=s)
    U = Guarded(n, d, d + 9, shift=1)
    ops.mask_from_softmax(S.t, U.t)
    assert np.array_equal(U.check().view(np.uint32), ref.upper_mask_ref(s).view(np.uint32))
    S.untouched()


# ================================================================================================ colmax
@pytest.mark.parametrize("from_softmax", [True, False])
@pytest.mark.parametrize("n,d", [(1, 1), (1, 65), (3, 64), (63, 63), (64, 64), (65, 65), (130, 260), (1024, 63), (200, 784)])
def test_colmax_keys_and_chunks(ops, n, d, from_softmax):
    """Keys equal the restatement exactly: ragged n and d, a padded leading dimension, row_offset > 0, planted exact ties
    (the lowest row wins), a column of zeros (from_softmax only: a given U must be positive); every chunk row of the partial
    launch is the restatement over that chunk's rows alone and their maximum is the finished key."""
    rng = np.random.default_rng(n * 31 + d)
    s = (rng.random((n, d)) * 2.0 / d).astype(np.float32) + np.float32(1e-6)
    if d >= 3:
        s[:, 1] = s[0, 1]                                        # every row ties
        if n >= 3:
            s[n // 2:, 2] = np.float32(0.75)                     # the maximum first appears mid-way, then repeats to the end
    if from_softmax:
        s[:, 0] = 0.0
    row_offset = 1000 + n
    S = Guarded(n, d, d + 5, data=s)
    u = ref.upper_mask_ref(s) if from_softmax else s
    chunks = ops.colmax_chunks(n)
    assert chunks == -(-n // 64)
    part, key = Guarded(1, chunks * d, dtype=torch.int64), Guarded(1, d, dtype=torch.int64)
    ops.colmax(S.t, row_offset, part.flat, key.flat, from_softmax)
    want = ref.colkey_ref(u, row_offset)
    got = key.check()[0].view(np.uint64)
    assert np.array_equal(got, want)
    rows = ref.colkey_rows(got) - row_offset
    assert np.array_equal(u[rows, np.arange(d)], u.max(axis=0)) and np.array_equal(rows, u.argmax(axis=0))
    part2 = Guarded(1, chunks * d, dtype=torch.int64)
    ops.colmax_partial(S.t, row_offset, part2.flat, from_softmax)
    p2 = part2.check()[0].view(np.uint64).reshape(chunks, d)
    for c in range(chunks):
        assert np.array_equal(p2[c], ref.colkey_pack_ref(u, row_offset)[64 * c:64 * (c + 1)].max(axis=0)), c
    assert np.array_equal(p2.max(axis=0), want)
    assert np.array_equal(part.check()[0].view(np.uint64).reshape(chunks, d), p2)
    S.untouched()


# ================================================================================================ mask backward
MB_CASES = [  # n, d, nslabs, path, keys
    (5, 252, 1, "aligned", True), (65, 252, 2, "aligned", True), (3, 260, 3, "aligned", True), (5, 640, 2, "aligned", True),
    (130, 784, 3, "aligned", True), (4, 1024, 2, "aligned", False), (5, 2048, 3, "aligned", True), (3, 4096, 2, "aligned", True),
    (63, 1500, 2, "aligned", True), (1, 4, 3, "aligned", True),
    (4, 4100, 2, "aligned", True), (5, 63, 3, "aligned", True), (3, 65, 1, "aligned", False), (1, 1, 2, "aligned", True), (4, 3, 2, "aligned", True),
    (130, 784, 3, "shifted", True), (5, 784, 2, "oddld", True), (65, 784, 2, "oddstride", True), (3, 1028, 1, "shifted", True),
]


@pytest.mark.parametrize("n,d,nslabs,path,keys", MB_CASES)
def test_mask_backward_every_kernel_and_path(ops, n, d, nslabs, path, keys):
    """Every NT of the row-in-registers kernel (d = 252, 260, 640, 784 / 1024, 2048 / 1500, 4096) and the scalar kernel four ways
    (d > 4096, d % 4 != 0, and d = 784 pushed off the vector path by a shifted base, an odd leading dimension or an odd slab
    stride); 1 to 3 slabs; no keys, and keys whose rows fall partly outside [row_offset, row_offset + n)."""
    rng = np.random.default_rng(n * 13 + d + nslabs)
    sh = shift_for(path)
    ldg, lds, ldo = ld_for(d, path, 4), ld_for(d, path, 8), ld_for(d, path, 12)
    s = ref.softmax64(rng.normal(size=(n, d)) * 2.0).astype(np.float32)
    g = [rng.normal(size=(n, d)).astype(np.float32) for _ in range(nslabs)]
    stride = n * ldg + (5 if path == "oddstride" else 8)
    gbuf = Guarded(1, (nslabs - 1) * stride + n * ldg, shift=sh)
    for q in range(nslabs):
        gbuf.buf.as_strided((n, d), (ldg, 1), gbuf.start + q * stride).copy_(dev(g[q]))
    gbuf.before = host(gbuf.buf).copy()
    S = Guarded(n, d, lds, shift=sh, data=s)
    row_offset, colkey, kd = 10, None, None
    if keys:
        r = rng.integers(-3, n + 3, size=d)
        r[0] = 0
        colkey = ((np.uint64(0x3F800000) << np.uint64(32)) | (np.uint64(0xFFFFFFFF) - (row_offset + r).astype(np.uint64)))
        kd = dev(colkey.view(np.int64))
    out = Guarded(n, d, ldo, shift=sh)
    ops.mask_backward(gbuf.buf.as_strided((n, d), (ldg, 1), gbuf.start), S.t, kd, 10.0, row_offset, out.t, nslabs=nslabs, slab_stride=stride)
    want = ref.mask_backward_ref(g, s, colkey, 10.0, row_offset)
    got = out.check()
    print(f"mask_backward n={n} d={d}: max err {np.abs(got - want).max():.3e}, bar {5e-5 * np.abs(want).max():.3e}")
    np.testing.assert_allclose(got, want, rtol=0, atol=5e-5 * np.abs(want).max())
    gbuf.untouched(), S.untouched()


# ================================================================================================ reductions
@pytest.mark.parametrize("n,d", [(1, 1), (3, 5), (65, 63), (130, 260), (1024, 784)])
def test_mse_and_sum_f64(ops, n, d):
    rng = np.random.default_rng(n + 3 * d)
    a, b = rng.normal(size=(n, d)).astype(np.float32), rng.normal(size=(n, d)).astype(np.float32)
    A, B = Guarded(n, d, d + 3, data=a), Guarded(n, d, d + 6, shift=1, data=b)
    df = (a - b).astype(np.float64)
    scale = np.float32(0.37)
    want = float(scale) * (df * df).sum()
    out = Guarded(1, 1)
    ops.mse(A.t, B.t, scale, out.flat, accumulate=False)
    got = float(out.check()[0, 0])
    assert abs(got - want) <= 2.0 ** -23 * abs(want), (got, want)
    out.flat.fill_(2.5)
    ops.mse(A.t, B.t, scale, out.flat, accumulate=True)
    assert abs(float(out.check()[0, 0]) - (2.5 + want)) <= 2.0 ** -23 * (2.5 + want)
    A.untouched(), B.untouched()
    # vgan_sum_f64 over n * d float64 values
    v = rng.random(n * d) * 3.0
    src = Guarded(1, n * d, dtype=torch.float64, data=v[None])
    for count in sorted({1, n * d // 2 + 1, n * d}):
        want = 1.75 * v[:count].sum()
        out = Guarded(1, 1)
        ops.sum_f64(src.flat, count, 1.75, out.flat, accumulate=False)
        assert abs(float(out.check()[0, 0]) - want) <= 2.0 ** -23 * want
        out.flat.fill_(0.125)
        ops.sum_f64(src.flat, count, 1.75, out.flat, accumulate=True)
        assert abs(float(out.check()[0, 0]) - (0.125 + want)) <= 2.0 ** -23 * (0.125 + want)
    src.untouched()


@pytest.mark.parametrize("n,d", [(1, 1), (3, 65), (5, 4100), (63, 64), (130, 63), (1022, 260)])
def test_mse_grad(ops, n, d):
    rng = np.random.default_rng(n + d)
    t, p = rng.normal(size=(n, d)).astype(np.float32), rng.normal(size=(n, d)).astype(np.float32)
    T, P = Guarded(n, d, d + 1, data=t), Guarded(n, d, d + 2, data=p)
    nb = (n + 3) // 4
    part, g = Guarded(1, nb, dtype=torch.float64), Guarded(n, d, d + 3)
    gscale = 2.0 / (n * d)
    ops.mse_grad(T.t, P.t, gscale, part.flat, g.t)
    df = p - t
    assert np.array_equal(g.check().view(np.uint32), (np.float32(gscale) * df).view(np.uint32))
    rows = np.zeros(4 * nb)
    rows[:n] = (df.astype(np.float64) ** 2).sum(axis=1)
    want = rows.reshape(nb, 4).sum(axis=1)
    assert (np.abs(part.check()[0] - want) <= 1e-12 * want).all()
    T.untouched(), P.untouched()


@pytest.mark.parametrize("rows", [1, 15, 16, 17, 5000])
@pytest.mark.parametrize("d", [1, 65, 260])
def test_col_mean(ops, rows, d):
    rng = np.random.default_rng(rows + d)
    x = (1e3 + rng.normal(size=(rows, d)) * np.linspace(0.1, 30.0, d)).astype(np.float32)
    X = Guarded(rows, d, d + 3, data=x)
    out = Guarded(1, d)
    ops.col_mean(X.t, out.flat)
    want = x.astype(np.float64).mean(axis=0)
    err = np.abs(out.check()[0].astype(np.float64) - want)
    assert (err <= 2.0 ** -23 * np.abs(want) + 2.0 ** -40 * np.abs(x).mean(axis=0)).all(), float((err / np.abs(want)).max())
    X.untouched()


@pytest.mark.parametrize("rows,p", [(1, 1), (3, 63), (4, 64), (5, 65), (65, 260), (130, 784), (1024, 100), (7, 4100)])
def test_row_sqnorm(ops, rows, p):
    rng = np.random.default_rng(rows + p)
    z = rng.normal(size=(rows, p)).astype(np.float32)
    Z = Guarded(rows, p, p + 5, data=z)
    sq = Guarded(1, rows)
    ops.row_sqnorm(Z.t, sq.flat, p)
    assert_sq(sq.check()[0], z, p)
    Z.untouched()


@pytest.mark.parametrize("rows,cols", [(1, 1), (3, 63), (5, 65), (66, 130), (131, 1000)])
def test_rows_dot(ops, rows, cols):
    rng = np.random.default_rng(rows * cols)
    a, b = rng.normal(size=(rows, cols)).astype(np.float32), rng.normal(size=(rows, cols)).astype(np.float32)
    A, B = Guarded(rows, cols, cols + 1, data=a), Guarded(rows, cols, cols + 6, data=b)
    out = Guarded(1, rows, dtype=torch.float64)
    ops.rows_dot(A.t, B.t, out.flat)
    prod = a.astype(np.float64) * b.astype(np.float64)
    assert (np.abs(out.check()[0] - prod.sum(axis=1)) <= 1e-12 * np.abs(prod).sum(axis=1)).all()
    out = Guarded(1, rows, dtype=torch.float64)
    ops.rows_dot(A.t, B.t[rows - 1:rows], out.flat, broadcast_b=True)
    prod = a.astype(np.float64) * b[rows - 1].astype(np.float64)
    assert (np.abs(out.check()[0] - prod.sum(axis=1)) <= 1e-12 * np.abs(prod).sum(axis=1)).all()
    A.untouched(), B.untouched()


# ================================================================================================ optimiser
COUNTS = [1, 3, 4, 5, 100003, 5_000_003]  # the last: past the 2048-workgroup cap of the grid on both paths
HYPER = dict(lr=0.007, rho=0.9, eps=1e-6, weight_decay=0.04, grad_scale=0.25)


def adadelta_state(rng, count):
    p = rng.uniform(-1.5, 1.5, size=count).astype(np.float32)
    sq, acc = (rng.random(count) * 1e-6).astype(np.float32), (rng.random(count) * 1e-6).astype(np.float32)
    return p, sq, acc


def assert_adadelta(got, want, steps, what):
    (p, sq, acc), (pr, sr, ar) = got, want
    np.testing.assert_allclose(p, pr, rtol=0, atol=steps * 2e-7, err_msg=what)
    np.testing.assert_allclose(sq, sr, rtol=steps * 1e-5, atol=steps * 1e-12, err_msg=what)
    np.testing.assert_allclose(acc, ar, rtol=steps * 1e-4, atol=steps * 1e-12, err_msg=what)


@pytest.mark.parametrize("nslabs", [1, 3])
@pytest.mark.parametrize("count", COUNTS)
def test_adadelta_step_paths_slabs_and_three_steps(ops, count, nslabs):
    """vgan_adadelta_step against the float64 oracle after one and after three steps (fresh gradients each), on the vector
    path, on the scalar path reached by a shifted base, and (slabs) by a slab stride that is no multiple of 4; the three
    paths inline the same adadelta_one and must agree bit for bit."""
    rng = np.random.default_rng(count + nslabs)
    p0, sq0, acc0 = adadelta_state(rng, count)
    grads = [[(rng.normal(size=count) * 1e-3).astype(np.float32) for _ in range(nslabs)] for _ in range(3)]
    want, st = [], tuple(v.astype(np.float64) for v in (p0, sq0, acc0))
    for step in range(3):
        g = ref.sum_slabs_f32(grads[step]).astype(np.float64) * HYPER["grad_scale"]
        st = orc.adadelta_step(st[0], g, st[1], st[2], HYPER["lr"], HYPER["weight_decay"], HYPER["rho"], HYPER["eps"])
        want.append(st)
    variants = [("vector", 0, round4(count) + 8), ("shifted", 1, round4(count) + 8)] + ([("oddstride", 0, round4(count) + 5)] if nslabs > 1 else [])
    results = {}
    for name, sh, stride in variants:
        P, SQ, ACC = (Guarded(1, count, shift=sh, data=v[None]) for v in (p0, sq0, acc0))
        G = Guarded(1, (nslabs - 1) * stride + count, shift=sh)
        res = []
        for step in range(3):
            for q in range(nslabs):
                G.buf[G.start + q * stride:G.start + q * stride + count].copy_(dev(grads[step][q]))
            G.before = host(G.buf).copy()
            ops.adadelta_step(P.flat, G.flat[:count], SQ.flat, ACC.flat, HYPER["lr"], HYPER["rho"], HYPER["eps"], HYPER["weight_decay"],
                              HYPER["grad_scale"], nslabs=nslabs, slab_stride=stride)
            res.append(tuple(b.check()[0] for b in (P, SQ, ACC)))
            G.untouched()
        assert_adadelta(res[0], want[0], 1, f"{name} step 1")
        assert_adadelta(res[2], want[2], 3, f"{name} step 3")
        results[name] = res
    for name in results:
        for step in range(3):
            for a, b, what in zip(results["vector"][step], results[name][step], ("p", "sq", "acc")):
                assert np.array_equal(a.view(np.uint32), b.view(np.uint32)), f"{what} of the {name} path differs from the vector path at step {step + 1}"


def test_adadelta_step_large_parameters(ops):
    """|p| in [2, 8), which the tests above leave out because the project's absolute p bar cannot hold there: the p bar is
    2^-24 |p| + 1e-7 per step (module docstring), sq / acc keep theirs; vector and scalar path, one and three steps."""
    rng = np.random.default_rng(28)
    count = 100003
    p0 = (rng.uniform(2.0, 8.0, size=count) * rng.choice([-1.0, 1.0], size=count)).astype(np.float32)
    assert (np.abs(p0) >= 2).all() and (np.abs(p0) >= 4).sum() > count // 2
    _, sq0, acc0 = adadelta_state(rng, count)
    grads = [(rng.normal(size=count) * 1e-3).astype(np.float32) for _ in range(3)]
    want, st = [], tuple(v.astype(np.float64) for v in (p0, sq0, acc0))
    for g in grads:
        st = orc.adadelta_step(st[0], g.astype(np.float64) * HYPER["grad_scale"], st[1], st[2], HYPER["lr"], HYPER["weight_decay"],
                               HYPER["rho"], HYPER["eps"])
        want.append(st)
    results = []
    for sh in (0, 1):
        P, SQ, ACC = (Guarded(1, count, shift=sh, data=v[None]) for v in (p0, sq0, acc0))
        res = []
        for g in grads:
            G = Guarded(1, count, shift=sh, data=g[None])
            ops.adadelta_step(P.flat, G.flat, SQ.flat, ACC.flat, HYPER["lr"], HYPER["rho"], HYPER["eps"], HYPER["weight_decay"],
                              HYPER["grad_scale"])
            res.append(tuple(b.check()[0] for b in (P, SQ, ACC)))
            G.untouched()
        for steps in (1, 3):
            (p, sq, acc), (pr, sr, ar) = res[steps - 1], want[steps - 1]
            err = np.abs(p.astype(np.float64) - pr)
            bar = steps * (2.0 ** -24 * np.abs(pr) + 1e-7)
            print(f"adadelta |p| in [2, 8), shift {sh}, step {steps}: worst p error {float((err / bar).max()):.3f} of its bar")
            assert (err <= bar).all(), float((err / bar).max())
            np.testing.assert_allclose(sq, sr, rtol=steps * 1e-5, atol=steps * 1e-12)
            np.testing.assert_allclose(acc, ar, rtol=steps * 1e-4, atol=steps * 1e-12)
        results.append(res)
    for a, b in zip(results[0], results[1]):
        for x, y in zip(a, b):
            assert np.array_equal(x.view(np.uint32), y.view(np.uint32)), "vector and scalar path differ"


@pytest.mark.parametrize("nslabs", [1, 3])
@pytest.mark.parametrize("count", COUNTS)
def test_reduce_slabs_bit_equal(ops, count, nslabs):
    rng = np.random.default_rng(count * 3 + nslabs)
    slabs = [rng.normal(size=count).astype(np.float32) for _ in range(nslabs)]
    want = ref.sum_slabs_f32(slabs)
    for sh_src, sh_dst, stride in [(0, 0, round4(count) + 4), (1, 0, round4(count) + 4), (0, 1, round4(count) + 4), (0, 0, round4(count) + 7)]:
        src = Guarded(1, (nslabs - 1) * stride + count, shift=sh_src)
        for q in range(nslabs):
            src.buf[src.start + q * stride:src.start + q * stride + count].copy_(dev(slabs[q]))
        src.before = host(src.buf).copy()
        dst = Guarded(1, count, shift=sh_dst)
        ops.reduce_slabs(src.flat, stride, nslabs, dst.flat)
        assert np.array_equal(dst.check()[0].view(np.uint32), want.view(np.uint32)), (sh_src, sh_dst, stride)
        src.untouched()


# ================================================================================================ packed optimiser / packing
@pytest.mark.parametrize("count", [1000, 784 * 785])  # the second: past the 2048-workgroup cap
def test_adadelta_step_packed(ops, count):
    """A permuted index map with ~5 % padding entries: mapped elements meet the adadelta_step bars, unmapped state and
    unmapped packed offsets are untouched, w_packed[pmap[i]] is p[i]; with next_noise the draw is the stand-alone
    noise_normal(stream_id 0) bit for bit and the optimiser's outputs do not change by a bit."""
    rng = np.random.default_rng(count)
    pmap = rng.permutation(count).astype(np.int32)
    dead = rng.random(count) < 0.05
    dead[[0, count - 1]] = True
    pmap[dead] = -1
    live = ~dead
    p0, sq0, acc0 = adadelta_state(rng, count)
    gp = (rng.normal(size=count) * 1e-3).astype(np.float32)
    pr, sr, ar = orc.adadelta_step(p0[live].astype(np.float64), gp[pmap[live]].astype(np.float64) * HYPER["grad_scale"],
                                   sq0[live].astype(np.float64), acc0[live].astype(np.float64), HYPER["lr"], HYPER["weight_decay"],
                                   HYPER["rho"], HYPER["eps"])
    pm, gd = dev(pmap, torch.int32), Guarded(1, count, data=gp[None])
    ctr = dev(np.array([2 ** 32 + 5], dtype=np.int64))
    rows, cols, ld = 130, 49, 52
    first = None
    for noise in (False, True):
        P, SQ, ACC = (Guarded(1, count, data=v[None]) for v in (p0, sq0, acc0))
        W = Guarded(1, count)
        Z = Guarded(rows, ld) if noise else None
        kw = dict(next_noise=Z.t, noise_cols=cols, noise_ones_col=cols, seed=0xABCDEF0123456789, step_counter=ctr) if noise else {}
        ops.adadelta_step_packed(P.flat, pm, gd.flat, W.flat, SQ.flat, ACC.flat, HYPER["lr"], HYPER["rho"], HYPER["eps"],
                                 HYPER["weight_decay"], HYPER["grad_scale"], **kw)
        got = tuple(b.check()[0] for b in (P, SQ, ACC))
        assert_adadelta(tuple(v[live] for v in got), (pr, sr, ar), 1, "mapped elements")
        for v, v0, what in zip(got, (p0, sq0, acc0), ("p", "sq", "acc")):
            assert np.array_equal(v[dead].view(np.uint32), v0[dead].view(np.uint32)), f"unmapped {what} changed"
        w = W.check(written=False)[0]
        assert np.array_equal(w[pmap[live]].view(np.uint32), got[0][live].view(np.uint32))
        hole = np.ones(count, dtype=bool)
        hole[pmap[live]] = False
        assert hole.sum() == dead.sum() and np.isnan(w[hole]).all(), "unmapped packed offsets were written"
        gd.untouched()
        if not noise:
            first = got + (w,)
            continue
        for a, b in zip(first, got + (w,)):
            assert np.array_equal(a.view(np.uint32), b.view(np.uint32)), "the noise rider changed the optimiser's outputs"
        alone = Guarded(rows, ld)
        ops.noise_normal(alone.t, 0xABCDEF0123456789, ctr, 0, cols=cols, ones_col=cols)
        z = Z.check(cols=cols + 1)
        assert np.array_equal(z.view(np.uint32), alone.check(cols=cols + 1).view(np.uint32))
        assert (z[:, cols] == 1).all()
        assert_noise(z[:, :cols], rows, cols, 0xABCDEF0123456789, 2 ** 32 + 5, 0)


def test_homogeneous_pack_three_layers_one_launch(ops):
    rng = np.random.default_rng(9)
    sizes = [(784, 784), (3, 5), (1, 1)]  # (out, in): one launch, the grid sized by the largest
    layers, hostl = [], []
    for k, (out, kin) in enumerate(sizes):
        W, b = rng.normal(size=(out, kin)).astype(np.float32), rng.normal(size=out).astype(np.float32)
        Wg, bg = Guarded(out, kin, kin + 3 + k, data=W), Guarded(1, out, data=b[None])
        P = Guarded(out + 1, kin + 1, kin + 1 + 5 + k, shift=k % 2)
        layers.append((Wg, bg, P))
        hostl.append((W, b))
    ops.homogeneous_pack([(Wg.t, bg.flat, P.t) for Wg, bg, P in layers])
    for (Wg, bg, P), (W, b) in zip(layers, hostl):
        assert np.array_equal(P.check().view(np.uint32), ref.homogeneous_ref(W, b).view(np.uint32))
        Wg.untouched(), bg.untouched()
    # unpack into fresh buffers restores W and b and leaves P alone
    fresh = []
    for (Wg, bg, P), (out, kin) in zip(layers, sizes):
        P.before = host(P.buf).copy()
        fresh.append((Guarded(out, kin, kin + 2), Guarded(1, out)))
    ops.homogeneous_pack([(W2.t, b2.flat, P.t) for (W2, b2), (_, _, P) in zip(fresh, layers)], unpack=True)
    for (W2, b2), (_, _, P), (W, b) in zip(fresh, layers, hostl):
        assert np.array_equal(W2.check().view(np.uint32), W.view(np.uint32)) and np.array_equal(b2.check()[0].view(np.uint32), b.view(np.uint32))
        P.untouched()


# ================================================================================================ noise
def assert_noise(got, rows, cols, seed, step, stream_id):
    want, r = ref.noise_normal_ref(rows, cols, seed, step, stream_id)
    err = np.abs(got.astype(np.float64) - want)
    unit = 2.0 ** -24 * r
    worst = float((err[r > 0] / unit[r > 0]).max()) if (r > 0).any() else 0.0
    print(f"noise [{rows}, {cols}] seed {seed:#x} step {step} stream {stream_id}: worst {worst:.2f} x 2^-24 r (bar {cpu_tier.NOISE_DEVICE_BAR:.2f})")
    assert (err <= cpu_tier.NOISE_DEVICE_BAR * unit).all(), worst


NOISE_KEYS = [(777, 0, 0), (777, 1, 0), (777, 2 ** 32, 0), (777, 2 ** 32 + 1, 0), (777, 3, 1), (777, 3, 2 ** 33),
              (0xDEADBEEF00000309, 3, 0), (0x8000000000000309, 2 ** 32 + 1, 2 ** 33 + 1)]


@pytest.mark.parametrize("rows,cols", [(1, 1), (3, 5), (1024, 49), (2100, 1000)])  # the last: past the grid cap
def test_noise_normal_against_the_philox_restatement(ops, rows, cols):
    assert abs(cpu_tier.NOISE_F32_CHAIN_ERR - 3.51) < 0.25 and cpu_tier.NOISE_DEVICE_BAR == 4 * cpu_tier.NOISE_F32_CHAIN_ERR
    seen = []
    for seed, step, stream in (NOISE_KEYS if rows * cols < 10 ** 6 else NOISE_KEYS[3:8:2]):
        ctr = dev(np.array([step], dtype=np.int64))
        Z = Guarded(rows, cols, cols + 3)
        ops.noise_normal(Z.t, seed, ctr, stream)
        z = Z.check()
        assert_noise(z, rows, cols, seed, step, stream)
        assert all(not np.array_equal(z, o) for o in seen), "two different (seed, step, stream) triples gave the same draws"
        seen.append(z)
        if rows * cols < 10 ** 6:   # padded layout with the ones column: the same draws, independent of ld
            Zp = Guarded(rows, cols + 1, cols + 6, shift=1)
            ops.noise_normal(Zp.t, seed, ctr, stream, cols=cols, ones_col=cols)
            zp = Zp.check()
            assert np.array_equal(zp[:, :cols].view(np.uint32), z.view(np.uint32)) and (zp[:, cols] == 1).all()
    Z = Guarded(rows, cols)
    ops.noise_normal(Z.t, 777, None, 0)                           # no step counter reads as step 0
    assert_noise(Z.check(), rows, cols, 777, 0, 0)
    if rows * cols < 10 ** 6:
        assert np.array_equal(Z.check().view(np.uint32), seen[0].view(np.uint32))


# ================================================================================================ shuffle
@pytest.mark.parametrize("N", SHUFFLE_N + [10 ** 6])
def test_shuffle_epoch_against_the_feistel_restatement(ops, N):
    for seed, epoch in SHUFFLE_KEYS:
        for count in sorted({N, max(1, N // 3)}):
            perm = Guarded(1, count, dtype=torch.int32)
            ops.shuffle_epoch(perm.flat, N, seed, epoch)
            got = perm.check()[0].astype(np.int64)
            assert np.array_equal(got, ref.feistel_perm_ref(np.arange(count), N, seed, epoch)), (N, seed, epoch, count)
            if count == N:
                assert np.array_equal(np.sort(got), np.arange(N))
    if N > 5:
        a, b = Guarded(1, N, dtype=torch.int32), Guarded(1, N, dtype=torch.int32)
        ops.shuffle_epoch(a.flat, N, 7, 3)
        ops.shuffle_epoch(b.flat, N, 7, 4)
        assert not np.array_equal(a.check(), b.check())


# ================================================================================================ grouped riders
@pytest.mark.parametrize("widths", [[1, 2, 4, 8, 20], [49, 98, 196, 392, 784]], ids=["c1", "c3"])
def test_grouped_riders_equal_the_stand_alone_launches(ops, widths):
    """The last product launch of a collapsed step (Gt_k = M_k . At_{k-1}^T, k = 4, 3, 2) with the copy, the Adadelta epilogue
    (+ the element-wise layer Gt_1) and the next noise draw riding in it: each rider's outputs are bit-equal to the same
    work done by a plain gemm_grouped followed by the stand-alone launch (copy_, adadelta_step_packed, noise_normal)."""
    rng = np.random.default_rng(sum(widths))
    e = [round4(w + 1) for w in widths]
    poff = [0]
    for k in range(1, 5):
        poff.append(poff[-1] + e[k] * e[k - 1])
    offsets, off = [], 0
    for k in range(1, 5):
        for numel in (widths[k] * widths[k - 1], widths[k]):
            offsets.append(off)
            off += round4(numel)
    total = off
    pmap = np.full(total, -1, dtype=np.int32)
    for k in range(1, 5):
        wk, wk1 = widths[k], widths[k - 1]
        r = np.arange(wk, dtype=np.int32)[:, None] * e[k - 1]
        ow, ob = offsets[2 * (k - 1)], offsets[2 * (k - 1) + 1]
        pmap[ow:ow + wk * wk1] = (poff[k - 1] + r + np.arange(wk1, dtype=np.int32)[None, :]).reshape(-1)
        pmap[ob:ob + wk] = (poff[k - 1] + r + wk1).reshape(-1)
    M = [None, None] + [dev((rng.normal(size=(e[k], e[0])) * 1e-2).astype(np.float32)) for k in (2, 3, 4)]
    At = [None] + [dev(rng.normal(size=(e[k], e[0])).astype(np.float32)) for k in (1, 2, 3)]
    g1 = (rng.normal(size=(e[1], e[0])) * 1e-2).astype(np.float32)
    p0, sq0, acc0 = adadelta_state(rng, total)
    src = dev(rng.normal(size=3001).astype(np.float32))
    ctr = dev(np.array([11], dtype=np.int64))
    nrows, L = 128, widths[0]
    hyper = dict(lr=HYPER["lr"], rho=HYPER["rho"], eps=HYPER["eps"], weight_decay=HYPER["weight_decay"], grad_scale=HYPER["grad_scale"])

    def fresh():
        Gt_all = torch.full((poff[-1],), float("nan"), device="cuda")
        Gt = [None] + [Gt_all[poff[k - 1]:poff[k]].view(e[k], e[k - 1]) for k in range(1, 5)]
        Gt[1].copy_(dev(g1))
        Wt_all = Guarded(1, poff[-1])
        Wt = [None] + [Wt_all.flat[poff[k - 1]:poff[k]].view(e[k], e[k - 1]) for k in range(1, 5)]
        state = tuple(Guarded(1, total, data=v[None]) for v in (p0, sq0, acc0))
        return Gt_all, Gt, Wt_all, Wt, state

    def problems(Gt):
        return [("NT", M[4], At[3], Gt[4]), ("NT", M[3], At[2], Gt[3]), ("NT", M[2], At[1], Gt[2])]

    # stand-alone: plain products, then copy, packed optimiser, noise
    Gt_all, Gt, Wt_all, Wt, (P, SQ, ACC) = fresh()
    ops.gemm_grouped(problems(Gt))
    assert not torch.isnan(Gt_all).any()
    ops.adadelta_step_packed(P.flat, dev(pmap, torch.int32), Gt_all, Wt_all.flat, SQ.flat, ACC.flat, **hyper)
    Za = Guarded(nrows, L + 1, round4(L + 1) + 4)
    ops.noise_normal(Za.t, 4242, ctr, 0, cols=L, ones_col=L)
    alone = [host(Gt_all)] + [b.check(written=False)[0] for b in (P, SQ, ACC, Wt_all)] + [Za.check()]
    # the same work riding in the product launch
    Gt_all, Gt, Wt_all, Wt, (P, SQ, ACC) = fresh()
    dst = Guarded(1, src.numel())
    Zb = Guarded(nrows, L + 1, round4(L + 1) + 4)
    layers = [(Wt[k], offsets[2 * (k - 1)], offsets[2 * (k - 1) + 1], widths[k], widths[k - 1]) for k in (4, 3, 2, 1)]
    ops.gemm_grouped(problems(Gt), copy=(src, dst.flat),
                     adadelta=dict(p=P.flat, sq=SQ.flat, acc=ACC.flat, layers=layers, extra_grad=Gt[1], **hyper),
                     noise=dict(next_noise=Zb.t, noise_cols=L, noise_ones_col=L, seed=4242, step_counter=ctr))
    rider = [host(Gt_all)] + [b.check(written=False)[0] for b in (P, SQ, ACC, Wt_all)] + [Zb.check()]
    assert np.array_equal(dst.check()[0].view(np.uint32), host(src).view(np.uint32)), "copy rider"
    for a, b, what in zip(alone, rider, ("products", "p", "sq", "acc", "w_packed", "noise")):
        assert np.array_equal(a.view(np.uint32), b.view(np.uint32)), f"{what}: the rider differs from the stand-alone launch"
    dead = pmap < 0
    assert np.array_equal(rider[1][dead].view(np.uint32), p0[dead].view(np.uint32)) and np.isnan(rider[4]).sum() == poff[-1] - (~dead).sum()
    assert_noise(rider[5][:, :L], nrows, L, 4242, 11, 0)
