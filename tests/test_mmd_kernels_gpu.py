"""The four RBF/MMD Gram kernels and the fp32 backward product on an MI355X, element by element against float64.

Reference and bounds: tests/mmd_ref.py (dense float64 L, K, W on the operands and the float32 row norms the kernel is given;
first-order, order-independent error bounds derived there, none tuned; tests/test_mmd_kernels_cpu.py pins the reference, the
bounds and their caps without a GPU).  Every output buffer starts as a sentinel (NaN; 0x7FC0 for the bf16 images): everything
the tile table owns must be written, everything else -- rows and columns past the image, columns [2n, ldw) -- must still hold
it.  Every case first asserts that its bound means something (max(bound) <= cap * max|W|), then prints its worst err / bound.

Layout variants of the fp32 Gram, and what is asserted of them:
  * ldw = 2n, ldw = 2n + 1 (the mirrored store falls back to its scalar form) and a W view one float into its allocation run
    the instructions of the aligned launch in the same order and differ only in the store that moves the finished registers:
    W and the tile sums are bit for bit those of the aligned launch.
  * ldz = p with p % 4 != 0 (ldz = p + 1 where p % 4 == 0), an aligned ldz with p % 4 != 0, and a Z view one float into its
    allocation all run the VEC = 1 instantiation: bit for bit equal among themselves.  Against the aligned launch (VEC = 4,
    another instantiation of the template, so another compilation of the epilogue) they are held to the bound.

Worst err / bound measured on an MI355X (the figures the tests print; the kernels use a tenth to a fifth of the bounds):
  fp32 Gram, W:            0.123 (33, 4)  0.117 (65, 7)  0.109 (100, 20)  0.107 (130, 33)  0.102 (128, 32)  0.066 (64, 64)
                           0.033 (96, 200); the same in grad_mode 1 and 2
  fp32 Gram, tile sums:    K 0.023, calibration L 0.030 (both at (65, 7)); general kernels (3 x 3.0, 6 x 1.5), W and sums: 0.063
  fp32 Gram, VEC = 1:      0.117 / 0.107 / 0.102 -- the worst of the aligned launch; all variants came out bit-equal to it
  split-bf16 Gram, W:      0.186 (65, 96)  0.146 (100, 130)  0.124 (130, 200)  0.194 (128, 65)  0.104 (192, 250)  0.170 (33, 70)
                           0.257 (65, 40)  0.270 (128, 64) -- the two kp = 64 cases; the same figure for tiles 64, 128 and 256
                           (and for 256 with the tail workspace lent, which at these sizes runs the same code: see
                           test_bf3_gram_weights_and_tile_sums); tile sums 0.004; rs_part 0.008
  row-sharded tables:      fp32 W 0.123, split-bf16 W 0.191, statistics summed over the ranks 0.001
  fp32 backward:           0.005 (65, 7)  0.003 (100, 20)  0.005 (96, 200)
"""
import functools

import numpy as np
import pytest
import torch

import mmd_ref as ref

pytestmark = pytest.mark.gpu

NAN = float("nan")
SENT16 = 0x7FC0


@pytest.fixture(scope="module")
def ops():
    from vgan_amd.ops import HipOps
    return HipOps()


def dev(a, dtype=torch.float32):
    return torch.as_tensor(np.ascontiguousarray(a)).to(dtype).cuda()


def host(t):
    return t.detach().cpu().numpy()


def round4(v):
    return (int(v) + 3) // 4 * 4


def owned(n, mode, rank=0, world=1):
    if world > 1:
        lo, hi = n * rank // world, n * (rank + 1) // world
        return hi - lo, n + lo
    return {1: (n, n), 2: (2 * n, 0)}[mode]


class Image:
    """A [rows, cols] view with row stride ld, `offset` elements into a sentinel-filled allocation with slack on both sides."""

    def __init__(self, rows, cols, ld, offset=0, dtype=torch.float32, sentinel=NAN):
        self.rows, self.cols, self.ld, self.offset, self.sentinel = rows, cols, ld, offset, sentinel
        self.flat = torch.full((offset + rows * ld + 64,), sentinel, dtype=dtype, device="cuda")
        self.view = torch.as_strided(self.flat, (rows, cols), (ld, 1), offset)

    def untouched(self, flat_host):
        return np.isnan(flat_host) if self.sentinel != self.sentinel else flat_host == np.int16(self.sentinel)

    def read(self, written):
        """The image on the host, after asserting: every element of `written` was written, nothing else in the allocation was."""
        f = host(self.flat)
        own = np.zeros(f.size, dtype=bool)
        rr, cc = np.nonzero(written)
        own[self.offset + rr * self.ld + cc] = True
        still = self.untouched(f)
        assert not still[own].any(), f"{int(still[own].sum())} owned elements were left unwritten"
        assert still[~own].all(), f"{int((~still[~own]).sum())} elements outside the table's image were written"
        return f[self.offset + np.arange(self.rows)[:, None] * self.ld + np.arange(self.cols)[None, :]]


def new_partial(ntiles):
    return torch.full((ntiles + 2, 4), NAN, device="cuda")


def read_partial(partial, ntiles):
    p = host(partial)
    assert not np.isnan(p[:ntiles, :2]).any() and np.isnan(p[ntiles:]).all()
    return p[:ntiles]


def worst_ratio(err, bound):
    return float((err / np.maximum(bound, 1e-300)).max())


def check_within(got, want, bound, what):
    err = np.abs(np.asarray(got, dtype=np.float64) - want)
    w = worst_ratio(err, bound)
    assert (err <= bound).all(), f"{what}: worst err / bound {w:.3f}, {int((err > bound).sum())} elements outside"
    return w


# ------------------------------------------------------------------------------------------------------ fp32 operands
@functools.lru_cache(maxsize=None)
def fp32_operands(n, p):
    """Z zero-padded to a multiple of 4 columns on the device (the aligned launch), its float32 row norms from the row-norm
    kernel (read back: the reference takes the norms the Gram kernel is given), the calibrated bandwidth."""
    from vgan_amd.ops import HipOps
    Z, _, bw = ref.make_case(n, p)
    pp = round4(p)
    Zd = torch.zeros(2 * n, pp, device="cuda")
    Zd[:, :p] = dev(Z)
    sq = torch.empty(2 * n, device="cuda")
    HipOps().row_sqnorm(Zd, sq, pp)
    return dict(Z=Z, Zd=Zd, sq=sq, s64=host(sq).astype(np.float64), z64=Z.astype(np.float64), bw=bw, bwd=dev([bw]), pp=pp)


@functools.lru_cache(maxsize=None)
def fp32_reference(n, p, mults=None):
    c = fp32_operands(n, p)
    L, K, W = ref.dense_weights(c["z64"], c["s64"], n, c["bw"], mults)
    wb = ref.weight_bound(c["z64"], c["s64"], n, c["bw"], p, mults)  # (the aligned launch's zero columns add no rounding)
    ref.cap_ok(wb, W, ref.CAP_FP32)
    for a in (L, K, W, wb):
        a.setflags(write=False)
    return L, K, W, wb


def fp32_sum_bound(tb, n, p, tile, mults=None, calibrate=False):
    c = fp32_operands(n, p)
    return ref.sum_bound(tb, c["z64"], c["s64"], n, c["bw"], p, tile, mults, calibrate)


def launch_fp32(ops, n, p, tiles, img, wrow0, Zd=None, p_arg=None, mults=None, calibrate=False, colmax=None):
    c = fp32_operands(n, p)
    Zd = c["Zd"] if Zd is None else Zd
    p_arg = c["pp"] if p_arg is None else p_arg
    partial = new_partial(tiles.shape[0])
    Wg = img.view if img is not None else None
    if calibrate:
        ops.mmd_gram(Zd, c["sq"], n, p_arg, None, tiles, True, None, 0, partial)
    elif mults is not None:
        ops.mmd_gram_general(Zd, c["sq"], n, p_arg, c["bwd"], tiles, mults, Wg, wrow0, partial)
    elif colmax is not None:
        ops.mmd_gram_colmax(Zd, c["sq"], n, p_arg, c["bwd"], tiles, Wg, wrow0, partial, colmax[0], 0, colmax[1], True)
    else:
        ops.mmd_gram(Zd, c["sq"], n, p_arg, c["bwd"], tiles, False, Wg, wrow0, partial)
    torch.cuda.synchronize()
    return read_partial(partial, tiles.shape[0])


@pytest.mark.parametrize("mode", [1, 2])
@pytest.mark.parametrize("n,p", ref.FP32_CASES)
def test_fp32_gram_weights_and_tile_sums(ops, n, p, mode):
    """vgan_mmd_gram, its calibration launch, vgan_mmd_gram_colmax and vgan_mmd_gram_general (3 kernels x 3.0, 6 x 1.5)."""
    L, K, W, wb = fp32_reference(n, p)
    tiles = ops.build_tiles(n, mode)
    tb = host(tiles)
    nr, wrow0 = owned(n, mode)
    ldw = round4(2 * n) + 4
    want, written = ref.scatter(tb, W, wrow0, nr, 64)
    bimg, _ = ref.scatter(tb, wb, wrow0, nr, 64)
    assert written.all()
    img = Image(nr, 2 * n, ldw)
    part = launch_fp32(ops, n, p, tiles, img, wrow0)
    got = img.read(written)
    rw = check_within(got, want, bimg, "W")
    rk = check_within(part[:, 0], ref.tile_sums(tb, K, 64), fp32_sum_bound(tb, n, p, 64), "tile sums of K")
    cal = launch_fp32(ops, n, p, tiles, None, 0, calibrate=True)
    rl = check_within(cal[:, 1], ref.tile_sums(tb, L, 64), fp32_sum_bound(tb, n, p, 64, calibrate=True), "tile sums of L")
    # the colmax launch: the same W and partials bit for bit, the column keys of colmax_partial
    rng = np.random.default_rng(n + p)
    S = dev(rng.uniform(0, 2.0 / p, size=(n, p)).astype(np.float32))
    chunks = ops.colmax_chunks(n)
    colpart = torch.zeros(chunks * p, dtype=torch.int64, device="cuda")
    colwant = torch.zeros(chunks * p, dtype=torch.int64, device="cuda")
    img2 = Image(nr, 2 * n, ldw)
    part2 = launch_fp32(ops, n, p, tiles, img2, wrow0, colmax=(S, colpart))
    ops.colmax_partial(S, 0, colwant, True)
    assert np.array_equal(img2.read(written), got) and np.array_equal(part2[:, :2], part[:, :2])
    assert torch.equal(colpart, colwant)
    rg = []
    for nk, mf in ref.FP32_MULTS:
        mults = tuple(ref.multipliers(nk, mf))
        _, Kg, Wgen, wbg = fp32_reference(n, p, mults)
        img3 = Image(nr, 2 * n, ldw)
        part3 = launch_fp32(ops, n, p, tiles, img3, wrow0, mults=mults)
        rg.append(check_within(img3.read(written), ref.scatter(tb, Wgen, wrow0, nr, 64)[0], ref.scatter(tb, wbg, wrow0, nr, 64)[0],
                               f"W general {nk} x {mf}"))
        rg.append(check_within(part3[:, 0], ref.tile_sums(tb, Kg, 64), fp32_sum_bound(tb, n, p, 64, mults), f"tile sums general {nk} x {mf}"))
    print(f"fp32 gram ({n}, {p}) mode {mode}: worst err/bound W {rw:.3f}, sum K {rk:.3f}, sum L {rl:.3f}, general W/sums {max(rg):.3f}")


@pytest.mark.parametrize("mode", [1, 2])
@pytest.mark.parametrize("n,p", [(65, 7), (130, 33), (128, 32)])
def test_fp32_gram_layout_variants(ops, n, p, mode):
    """See the module docstring for what runs which instructions."""
    c = fp32_operands(n, p)
    L, K, W, wb = fp32_reference(n, p)
    tiles = ops.build_tiles(n, mode)
    tb = host(tiles)
    nr, wrow0 = owned(n, mode)
    want, written = ref.scatter(tb, W, wrow0, nr, 64)
    bimg, _ = ref.scatter(tb, wb, wrow0, nr, 64)
    sb = fp32_sum_bound(tb, n, p, 64)
    ksum = ref.tile_sums(tb, K, 64)
    base = Image(nr, 2 * n, round4(2 * n) + 4)
    pbase = launch_fp32(ops, n, p, tiles, base, wrow0)
    gbase = base.read(written)
    check_within(gbase, want, bimg, "aligned")
    # W layouts: the same bits
    for ldw, off in ((2 * n, 0), (2 * n + 1, 0), (round4(2 * n) + 4, 1)):
        img = Image(nr, 2 * n, ldw, off)
        part = launch_fp32(ops, n, p, tiles, img, wrow0)
        assert np.array_equal(img.read(written), gbase), (ldw, off)
        assert np.array_equal(part[:, :2], pbase[:, :2]), (ldw, off)
    # Z layouts: VEC = 1
    Z = c["Z"]
    variants = []
    ldz = p if p % 4 else p + 1
    z1 = torch.full((2 * n, ldz), NAN if ldz > p else 0.0, device="cuda")
    z1[:, :p] = dev(Z)
    variants.append(("ldz", z1, p))
    if p % 4:
        variants.append(("p % 4", c["Zd"], p))
    flat = torch.zeros(2 * n * c["pp"] + 8, device="cuda")
    z3 = torch.as_strided(flat, (2 * n, c["pp"]), (c["pp"], 1), 1)
    z3.copy_(c["Zd"])
    variants.append(("base + 4 bytes", z3, c["pp"]))
    first = None
    worst = 0.0
    for name, Zv, p_arg in variants:
        img = Image(nr, 2 * n, round4(2 * n) + 4)
        part = launch_fp32(ops, n, p, tiles, img, wrow0, Zd=Zv, p_arg=p_arg)
        got = img.read(written)
        worst = max(worst, check_within(got, want, bimg, name), check_within(part[:, 0], ksum, sb, name + " sums"))
        check_within(got, gbase, bimg, name + " against the aligned launch")
        if first is None:
            first = (got, part)
        else:
            assert np.array_equal(got, first[0]) and np.array_equal(part[:, :2], first[1][:, :2]), name
    print(f"fp32 gram layouts ({n}, {p}) mode {mode}: worst err/bound of the VEC = 1 launches {worst:.3f}, "
          f"bit-equal to the aligned launch: {np.array_equal(first[0], gbase)}")


# ------------------------------------------------------------------------------------------------------ split-bf16 operands
def bf16_value(t):
    return (host(t).view(np.uint16).astype(np.uint32) << 16).view(np.float32).astype(np.float64)


@functools.lru_cache(maxsize=None)
def bf3_operands(n, d):
    from vgan_amd.ops import HipOps
    ops = HipOps()
    Z, _, bw = ref.make_case(n, d)
    dp, kp = round4(d), (d + 63) // 64 * 64
    Zd = torch.zeros(2 * n, dp, device="cuda")
    Zd[:, :d] = dev(Z)
    sq = torch.empty(2 * n, device="cuda")
    ops.row_sqnorm(Zd, sq, d)
    Zh = torch.zeros(2 * n, kp, dtype=torch.int16, device="cuda")
    Zl = torch.zeros(2 * n, kp, dtype=torch.int16, device="cuda")
    ops.mmd_bf3_prepare(Zd, 2 * n, d, Zh, Zl)
    torch.cuda.synchronize()
    zz = (bf16_value(Zh), bf16_value(Zl))  # the images read back from the device
    assert np.array_equal(zz[0][:, :d], ref.split_bf16(Z)[0]) and not zz[0][:, d:].any() and not zz[1][:, d:].any()
    s64 = host(sq).astype(np.float64)
    L, K, W = ref.dense_weights(zz, s64, n, bw)
    wb = ref.weight_bound(zz, s64, n, bw, 3 * kp, pair=True)
    ref.cap_ok(wb, W, ref.CAP_BF3)
    return dict(Zh=Zh, Zl=Zl, sq=sq, bwd=dev([bw]), bw=bw, zz=zz, s64=s64, K=K, W=W, wb=wb, kp=kp)


def launch_bf3(ops, n, d, tiles, tile, nr, wrow0, written, **kw):
    c = bf3_operands(n, d)
    kn = (2 * n + 63) // 64 * 64
    Wh = Image(nr, 2 * n, kn, 0, torch.int16, SENT16)
    Wl = Image(nr, 2 * n, kn, 0, torch.int16, SENT16)
    partial = new_partial(tiles.shape[0])
    ops.mmd_gram_bf3(c["Zh"], c["Zl"], c["sq"], n, c["bwd"], tiles, Wh.view, Wl.view, wrow0, partial, tile=tile, **kw)
    torch.cuda.synchronize()
    hi, lo = Wh.read(written), Wl.read(written)
    val = lambda a: (a.view(np.uint16).astype(np.uint32) << 16).view(np.float32).astype(np.float64)
    return val(hi) + val(lo), read_partial(partial, tiles.shape[0])


def check_bf3(ops, n, d, tiles, tile, nr, wrow0, **kw):
    c = bf3_operands(n, d)
    tb = host(tiles)
    want, written = ref.scatter(tb, c["W"], wrow0, nr, tile)
    bimg, _ = ref.scatter(tb, c["wb"], wrow0, nr, tile)
    assert written.all()
    got, part = launch_bf3(ops, n, d, tiles, tile, nr, wrow0, written, **kw)
    rw = check_within(got, want, bimg, f"W tile {tile}")
    sb = ref.sum_bound(tb, c["zz"], c["s64"], n, c["bw"], 3 * c["kp"], tile)
    rk = check_within(part[:, 0], ref.tile_sums(tb, c["K"], tile), sb, f"tile sums tile {tile}")
    return got, part, rw, rk


@pytest.mark.parametrize("mode", [1, 2])
@pytest.mark.parametrize("n,d", ref.BF3_CASES)
def test_bf3_gram_weights_and_tile_sums(ops, n, d, mode):
    """mmd_gram_bf3_kernel<64>, mmd_gram_bf3_big_kernel and mmd_gram_bf3_wide_kernel (the per-slot row sums where n % 128 == 0):
    hi + lo of the stored pair against scatter() on the split operands.  The 256-wide kernel also runs with the tail workspace
    handed in, which here only checks that lending it changes nothing: vgan_mmd_gram_bf3 splits a tail tile over K only when a
    part keeps at least 8 stages (kp >= 512), so at these sizes parts stays 1 and none of the slab, ticket or last-part code
    runs.  test_gram_bf3_wide_tail_split (test_hip_parity.py) remains the only cover of the split path.  (65, 40) and (128, 64):
    kp = 64, the shortest contraction (mmd_ref.py, BF3_CASES)."""
    nr, wrow0 = owned(n, mode)
    out = []
    for tile in (64, 128, 256):
        tiles = ops.build_tiles(n, mode, tile=tile)
        got, part, rw, rk = check_bf3(ops, n, d, tiles, tile, nr, wrow0)
        out.append(f"tile {tile}: W {rw:.3f}, sums {rk:.3f}")
        if tile != 256:
            continue
        _, _, rw, rk = check_bf3(ops, n, d, tiles, tile, nr, wrow0, tail_ws=ops.gram_tail_workspace("cuda"))
        out.append(f"tile 256 + tail_ws: W {rw:.3f}, sums {rk:.3f}")
        if n % 128 == 0:
            slots = (2 * n + 127) // 128
            rs_part = torch.full((slots, nr), NAN, device="cuda")
            got, _, _, _ = check_bf3(ops, n, d, tiles, tile, nr, wrow0, rs_part=rs_part)
            pad = np.zeros((nr, slots * 128))
            pad[:, :2 * n] = got
            want_rs = pad.reshape(nr, slots, 128).sum(2).T
            brs = 128 * 2.0 ** -23 * np.abs(pad).reshape(nr, slots, 128).sum(2).T  # a float32 sum of 128 terms, in any order
            rs = host(rs_part)
            assert not np.isnan(rs).any(), "a slot of rs_part was left unwritten"
            out.append(f"rs_part {check_within(rs, want_rs, brs, 'rs_part'):.3f}")
    print(f"bf3 gram ({n}, {d}) mode {mode}: worst err/bound " + "; ".join(out))


# ------------------------------------------------------------------------------------------------------ row-sharded tables
@pytest.mark.parametrize("n,world", ref.SHARD_CASES)
def test_row_sharded_tables_fp32_and_bf3(ops, n, world):
    """Every rank's Wg [hi - lo, 2n] with wrow0 = n + lo is rows n + lo .. n + hi of the dense W, on the fp32 Gram and on the
    64-wide split-bf16 Gram; the ranks' reduced statistics add up to the dense block sums, as the single-rank table's do.
    All ranks run in this process, one after another."""
    p, d = ref.SHARD_P, ref.SHARD_D
    L, K, W, wb = fp32_reference(n, p)
    cb = bf3_operands(n, d)
    blocks = lambda M: np.array([M[:n, :n].sum(), M[n:, :n].sum(), M[n:, n:].sum()])
    total, total_b, tb_bound = np.zeros(4), np.zeros(4), np.zeros(4)
    total3, total3_b = np.zeros(4), np.zeros(4)
    rw = rw3 = 0.0
    for rank in range(world):
        tiles = ops.build_tiles(n, 1, rank, world)
        tb = host(tiles)
        nr, wrow0 = owned(n, 1, rank, world)
        want, written = ref.scatter(tb, W, wrow0, nr, 64)
        assert written.all() and np.array_equal(want, W[wrow0:wrow0 + nr])
        img = Image(nr, 2 * n, round4(2 * n) + 4)
        part = launch_fp32(ops, n, p, tiles, img, wrow0)
        rw = max(rw, check_within(img.read(written), W[wrow0:wrow0 + nr], wb[wrow0:wrow0 + nr], f"fp32 rank {rank}"))
        sb = fp32_sum_bound(tb, n, p, 64)
        check_within(part[:, 0], ref.tile_sums(tb, K, 64), sb, f"fp32 sums rank {rank}")
        partial = dev(part)
        stats = torch.zeros(4, dtype=torch.float64, device="cuda")
        ops.mmd_reduce(partial, tiles, stats, True)
        total += host(stats)
        total_b += ref.reduce_stats(tb, sb)
        # the 64-wide split-bf16 Gram on the same table
        got, part3, r3, _ = check_bf3(ops, n, d, tiles, 64, nr, wrow0)
        assert np.array_equal(ref.scatter(tb, cb["W"], wrow0, nr, 64)[0], cb["W"][wrow0:wrow0 + nr])
        rw3 = max(rw3, r3)
        ops.mmd_reduce(dev(part3), tiles, stats, True)
        total3 += host(stats)
        total3_b += ref.reduce_stats(tb, ref.sum_bound(tb, cb["zz"], cb["s64"], n, cb["bw"], 3 * cb["kp"], 64))
    rs = check_within(total[:3], blocks(K), total_b[:3], "fp32 statistics over the ranks")
    rs3 = check_within(total3[:3], blocks(cb["K"]), total3_b[:3], "bf3 statistics over the ranks")
    # the single-rank table's statistics meet the same dense sums within their own bounds: the two agree within the sum of both
    tiles = ops.build_tiles(n, 1)
    tb = host(tiles)
    part = launch_fp32(ops, n, p, tiles, None, 0)
    stats = torch.zeros(4, dtype=torch.float64, device="cuda")
    ops.mmd_reduce(dev(part), tiles, stats, True)
    one_b = ref.reduce_stats(tb, fp32_sum_bound(tb, n, p, 64))
    check_within(host(stats)[:3], blocks(K), one_b[:3], "fp32 statistics of the single-rank table")
    assert (np.abs(host(stats)[:3] - total[:3]) <= one_b[:3] + total_b[:3]).all()
    print(f"sharded n = {n}, world = {world}: worst err/bound fp32 W {rw:.3f}, bf3 W {rw3:.3f}, statistics fp32 {rs:.3f}, bf3 {rs3:.3f}")


# ------------------------------------------------------------------------------------------------------ fp32 backward, direct
@pytest.mark.parametrize("n,p", ref.BWD_CASES)
def test_fp32_backward_direct(ops, n, p):
    """vgan_mmd_backward on a random W against float64 on the same float32 operands: gradient rows of the Y half, of all rows
    and of a shard; without mul, with mul alone and with mul + mul_shift; 1, 3 and 40 split-K slabs (at 40 most slabs are empty and come back
    exactly zero); (65, 7) with ldz = 7 and ldw = 130 runs the VEC = 1 instantiation."""
    rng = np.random.default_rng(7 * n + p)
    N = 2 * n
    Z = rng.normal(size=(N, p)).astype(np.float32)
    Zd = dev(Z)
    z64 = Z.astype(np.float64)
    worst = 0.0
    for nr, wrow0 in ((n, n), (N, 0), (32, n + 32)):
        Wm = (rng.normal(size=(nr, N)) * 1e-3).astype(np.float32)
        Wd = dev(Wm)
        w64 = Wm.astype(np.float64)
        mul = rng.normal(size=(nr, p)).astype(np.float32)
        shift = rng.normal(size=(p,)).astype(np.float32)
        for with_mul, with_shift in ((False, False), (True, False), (True, True)):
            m64 = mul.astype(np.float64) + (shift.astype(np.float64) if with_shift else 0.0) if with_mul else None
            want = ref.backward_ref(w64, z64, wrow0, nr, m64)
            bound = ref.backward_bound(w64, z64, wrow0, nr, N, m64)
            for splits in (1, 3, 40):
                ldo = p + 3
                slabs = torch.full((splits, nr, ldo), NAN, device="cuda")
                ops.mmd_backward(Wd, Zd, wrow0, nr, N, p, dev(mul) if with_mul else None, slabs[0, :, :p], splits, nr * ldo,
                                 mul_shift=dev(shift) if with_shift else None)
                torch.cuda.synchronize()
                o = host(slabs).astype(np.float64)
                assert np.isnan(o[:, :, p:]).all() and not np.isnan(o[:, :, :p]).any()
                kchunk = ((N + splits - 1) // splits + 63) // 64 * 64
                live = (N + kchunk - 1) // kchunk
                assert live < splits or splits < 40
                assert not o[live:, :, :p].any(), "an empty slab is not exactly zero"
                for s in range(live):  # every slab against its own columns
                    lo, hi = s * kchunk, min((s + 1) * kchunk, N)
                    wz = np.zeros_like(w64)
                    wz[:, lo:hi] = w64[:, lo:hi]
                    check_within(o[s, :, :p], ref.backward_ref(wz, z64, wrow0, nr, m64),
                                 ref.backward_bound(wz, z64, wrow0, nr, hi - lo, m64), f"slab {s} of {splits}")
                worst = max(worst, check_within(o[:, :, :p].sum(0), want, bound, f"nr {nr} wrow0 {wrow0} mul {with_mul} shift {with_shift} splits {splits}"))
    print(f"fp32 backward ({n}, {p}): worst err/bound {worst:.3f}")
