"""The split-bf16 MMD backward product on an MI355X, element by element and slab by slab against float64: the four kernels behind
launch_backward_bf3 (mmd_backward_bf3_kernel<64, RM>, mmd_backward_bf3_big_kernel<RM>, mmd_backward_bf3_wide_kernel and the
GemmBF3 / GemmBF3Big / GemmBF3Wide loops `run` and `run_bt`) through vgan_mmd_backward_bf3_rm and vgan_mmd_backward_bf3, and
vgan_mmd_bf3_prepare.  (The _rm_rebuild and _xx entry points are pinned bit for bit to _rm on 64-wide tiles in
test_bf3_lean_step_gpu.py and test_hip_parity.py.)

Reference and bound: tests/mmd_ref.py, 'split-bf16 backward' (float64 on the very images the kernel is given, Wl.Zl left out on
both sides; a first-order, order-independent bound, nothing tuned; tests/test_mmd_bwd_bf3_cpu.py checks without a GPU that at
every case here the bound respects its cap and rejects a product with a term dropped or added).  The shapes are the smallest
that reach each schedule (mmd_ref.BWD_BF3_CASES).

Every operand sits in a guard allocation (Image): Wh, Wl [nr, kn + 8] with zero in the columns [N, kn) and bf16 NaN in
[kn, kn + 8) and after the last row; Zh, Zl with exactly N rows and NaN after them; ZTh, ZTl [kp, kn] from vgan_mmd_bf3_prepare
with NaN after them; the fp32 Z with ldz = p and NaN after row N; mul with ldmul = p + 1; the slabs with ldo = p + 3 in a
NaN-filled allocation.  After every launch every element of [nr, p] of every slab must be written, nothing else in the
allocation, and no NaN may appear: a read past an operand's end is multiplied by W's zero padding, which only a NaN shows.

Worst err / bound measured on an MI355X (the figures the tests print; over every row range, multiplier variant, slab count and
slab, and the slab sums; the bound is the criterion, these are the record):
  (n, p)        tile 64   tile 128   tile 256          term isolation, every tile alike:   Wh = 0   Zh = 0   Wh = Zh = 0
  (32, 7)        0.003     0.003                         (65, 65)                            0.008    0.009    0.009
  (33, 64)       0.008     0.008                         (100, 130)                          0.002    0.002    0.002
  (65, 65)       0.008     0.008
  (100, 130)     0.007     0.007                       row sums handed in (rs_part), tile 256, (128, 130): 0.405 (the bound of
  (130, 200)     0.007     0.007                       a two-cell sum is small)
  (65, 40)       0.008     0.008      0.008
  (130, 130)     0.008     0.008      0.008
  (128, 130)     0.007     0.006      0.007
The kernels use under a hundredth of the bound, which is an any-order worst case over K terms; what the bound still rejects is
measured in tests/test_mmd_bwd_bf3_cpu.py (a dropped cross term puts 24 % to 93 % of the elements outside).  Checked once by hand
that the net bites on the device too: with Wh.Zl dropped in GemmBF3::run_bt, Wl.Zl in place of Wl.Zh in GemmBF3Big's products and
s0 = 0 in the slot fold, every backward test of this file failed (the three prepare tests passed).
"""
import functools

import numpy as np
import pytest
import torch

import mmd_ref as ref
from test_mmd_kernels_gpu import SENT16, Image, check_within, dev, host

pytestmark = pytest.mark.gpu

@pytest.fixture(scope="module")
def ops():
    from vgan_amd.ops import HipOps
    return HipOps()


def image16(rows, cols, ld, values64=None):
    """A guard allocation of bf16 NaN holding the bf16 values `values64` (float64 [rows, <= cols], zero to the right)."""
    img = Image(rows, cols, ld, 0, torch.int16, SENT16)
    bits = np.zeros((rows, cols), dtype=np.uint16)
    if values64 is not None:
        bits[:, :values64.shape[1]] = ref.bf16_bits(values64)
    img.view.copy_(torch.as_tensor(bits.view(np.int16)))
    return img


def image32(values32, ld):
    rows, cols = values32.shape
    img = Image(rows, cols, ld)
    img.view.copy_(torch.as_tensor(np.array(values32, dtype=np.float32)))  # (a copy: the case data is read-only)
    return img


def bits_of(img, rows, cols):
    """The uint16 image on the host (guards not checked: these are operands)."""
    f = host(img.flat).view(np.uint16)
    return f[img.offset + np.arange(rows)[:, None] * img.ld + np.arange(cols)[None, :]]


@functools.lru_cache(maxsize=None)
def operands(n, p):
    """The device images of a case (see the module docstring); ZTh / ZTl come from vgan_mmd_bf3_prepare and are checked against
    the host's split of Z, as are the row-major images the same launch writes."""
    from vgan_amd.ops import HipOps
    d = ref.bwd_bf3_data(n, p)
    N, kn, kp = d["N"], d["kn"], d["kp"]
    c = dict(d=d, Z=image32(d["Z"], p), Zh=image16(N, kp, kp, d["zh"][:N]), Zl=image16(N, kp, kp, d["zl"][:N]),
             Zh0=image16(N, kp, kp), ZTh=Image(kp, kn, kn, 0, torch.int16, SENT16), ZTl=Image(kp, kn, kn, 0, torch.int16, SENT16),
             ZTh0=image16(kp, kn, kn))
    sh, sl = torch.zeros(N, kp, dtype=torch.int16, device="cuda"), torch.zeros(N, kp, dtype=torch.int16, device="cuda")
    HipOps().mmd_bf3_prepare(dev(d["Z"]), N, p, sh, sl, c["ZTh"].view, c["ZTl"].view)
    torch.cuda.synchronize()
    every = np.ones((kp, kn), dtype=bool)
    for T, s, z in ((c["ZTh"], sh, d["zh"]), (c["ZTl"], sl, d["zl"])):
        want = np.zeros((kp, kn), dtype=np.uint16)
        want[:p] = ref.bf16_bits(z.T)
        assert np.array_equal(T.read(every).view(np.uint16), want), "the transposed image is not the host's split of Z"
        assert np.array_equal(host(s).view(np.uint16)[:, :p], want[:p, :N].T) and not host(s)[:, p:].any()
    c["ranges"] = []
    for rg in d["ranges"]:
        nr = rg["nr"]
        c["ranges"].append(dict(rg, Wh=image16(nr, kn, kn + 8, rg["wh"]), Wl=image16(nr, kn, kn + 8, rg["wl"]), Wh0=image16(nr, kn, kn + 8),
                                mulimg=image32(rg["mul"], p + 1), shiftimg=image32(rg["shift"][None, :], p),
                                zrow=d["Z"][rg["wrow0"]:rg["wrow0"] + nr].astype(np.float64)))
    return c


def launch(ops, c, rg, entry, tile, splits, variant, wh0=False, zh0=False, rs_part=None):
    """One launch into a fresh NaN-filled slab allocation; returns the slabs [splits, nr, p] as float64 after the sentinel
    checks: all of [nr, p] of every slab written, nothing else, no NaN."""
    d = c["d"]
    nr, p, ldo = rg["nr"], d["p"], d["p"] + 3
    out = Image(splits * nr, p, ldo)
    mul = rg["mulimg"].view if variant != "none" else None
    shift = rg["shiftimg"].view[0] if variant == "mul+shift" else None
    Wh = (rg["Wh0"] if wh0 else rg["Wh"]).view
    first = torch.as_strided(out.flat, (nr, p), (ldo, 1), 0)
    if entry == "rm":
        ops.mmd_backward_bf3_rm(Wh, rg["Wl"].view, (c["Zh0"] if zh0 else c["Zh"]).view, c["Zl"].view, d["N"], c["Z"].view, rg["wrow0"], nr, p,
                                mul, first, splits, nr * ldo, mul_shift=shift, tile=tile, rs_part=rs_part)
    else:
        ops.mmd_backward_bf3(Wh, rg["Wl"].view, (c["ZTh0"] if zh0 else c["ZTh"]).view, c["ZTl"].view, c["Z"].view, rg["wrow0"], nr, p, mul,
                             first, splits, nr * ldo, mul_shift=shift, tile=tile)
    torch.cuda.synchronize()
    f = host(out.flat)  # (Image.read's checks, on the row structure instead of an index list: the 40-slab images are large)
    body = f[:splits * nr * ldo].reshape(splits * nr, ldo)
    assert np.isnan(body[:, p:]).all() and np.isnan(f[splits * nr * ldo:]).all(), "elements outside [nr, p] of the slabs were written"
    assert not np.isnan(body[:, :p]).any(), "an element of a slab was left unwritten, or a NaN was read into it"
    return body[:, :p].reshape(splits, nr, p).astype(np.float64)


@functools.lru_cache(maxsize=None)
def reference(n, p, ri, variant, splits, wh0=False, zh0=False):
    """[(want, bound)] of the live slabs, each on its own columns with K = its own length, and (want, bound) of the whole."""
    d = ref.bwd_bf3_data(n, p)
    rg = d["ranges"][ri]
    zrow = d["Z"][rg["wrow0"]:rg["wrow0"] + rg["nr"]].astype(np.float64)
    wh = np.zeros_like(rg["wh"]) if wh0 else rg["wh"]
    zh = np.zeros_like(d["zh"]) if zh0 else d["zh"]
    m64 = ref.bwd_bf3_mul64(rg, variant)
    args = (wh, rg["wl"], zh, d["zl"], zrow, m64)
    exact = wh0 and zh0
    _, live, slabs = ref.bf3_slabs(d["kn"], splits)
    per = [(ref.backward_bf3_ref(*args, k0, k1), ref.backward_bf3_bound(*args, k0, k1, exact_acc=exact)) for k0, k1 in slabs]
    whole = (ref.backward_bf3_ref(*args), ref.backward_bf3_bound(*args, exact_acc=exact))
    ref.cap_ok(whole[1], whole[0], ref.CAP_BWD_BF3)
    return per, whole


def check_slabs(o, n, p, ri, variant, splits, what, **iso):
    per, whole = reference(n, p, ri, variant, splits, **iso)
    live = len(per)
    assert live <= splits and (splits < 40 or live < splits)
    assert not o[live:].any(), f"{what}: an empty slab is not exactly zero"
    w = 0.0
    for s, (want, bound) in enumerate(per):
        w = max(w, check_within(o[s], want, bound, f"{what} slab {s} of {splits}"))
    return max(w, check_within(o.sum(0), whole[0], whole[1], f"{what} sum of {splits} slabs"))


def tiles_of(n, p):
    return (64, 128, 256) if (n, p) in ref.BWD_BF3_WIDE else (64, 128)


@pytest.mark.parametrize("n,p", ref.BWD_BF3_CASES)
def test_backward_bf3_per_element_and_per_slab(ops, n, p):
    """vgan_mmd_backward_bf3_rm and vgan_mmd_backward_bf3 with tiles 64 and 128 forced (256 on the three wide cases, row-major
    operand only): every live slab against the reference restricted to its own columns, the slab sum against the whole, empty
    slabs exactly zero; row-major equals transposed bit for bit; the transposed entry point with tile 256 equals it with tile 128
    (the fallback); every launch twice, the same bits."""
    c = operands(n, p)
    worst = {t: 0.0 for t in tiles_of(n, p)}
    for ri, rg in enumerate(c["ranges"]):
        for variant in ref.BWD_BF3_MULS:
            for splits in ref.bwd_bf3_splits(n):
                tr128 = None
                for tile in tiles_of(n, p):
                    what = f"({n}, {p}) nr {rg['nr']} wrow0 {rg['wrow0']} {variant} tile {tile}"
                    rm = launch(ops, c, rg, "rm", tile, splits, variant)
                    assert np.array_equal(rm, launch(ops, c, rg, "rm", tile, splits, variant)), f"{what}: not reproducible"
                    tr = launch(ops, c, rg, "tr", tile, splits, variant)
                    assert np.array_equal(tr, launch(ops, c, rg, "tr", tile, splits, variant)), f"{what}: transposed, not reproducible"
                    if tile == 128:
                        tr128 = tr
                    if tile == 256:
                        assert np.array_equal(tr, tr128), f"{what}: transposed images with tile 256 must run the 128-wide kernel"
                        worst[128] = max(worst[128], check_slabs(tr, n, p, ri, variant, splits, what + " transposed"))
                    else:
                        assert np.array_equal(rm, tr), f"{what}: row-major and transposed operands differ"
                    worst[tile] = max(worst[tile], check_slabs(rm, n, p, ri, variant, splits, what))
    print(f"bf3 backward ({n}, {p}): worst err/bound " + ", ".join(f"tile {t}: {w:.3f}" for t, w in worst.items()))


@pytest.mark.parametrize("n,p", [(65, 65), (100, 130)])
def test_backward_bf3_term_isolation(ops, n, p):
    """All three tiles with a zero image in place of Wh (acc must be Wl.Zh alone), of Zh (Wh.Zl alone) and of both: acc must then
    be exactly zero -- Wl.Zl is never formed -- and out = 2 rs z (mul + shift) to the row sum's and the epilogue's rounding.  The bound
    is formed from the images given and shrinks with them."""
    c = operands(n, p)
    worst = {}
    for wh0, zh0 in ((True, False), (False, True), (True, True)):
        key = "Wh = 0" if not zh0 else "Zh = 0" if not wh0 else "Wh = Zh = 0"
        for ri, rg in enumerate(c["ranges"]):
            for variant in ref.BWD_BF3_MULS:
                for splits in (1, 2):
                    for tile in (64, 128, 256):
                        what = f"({n}, {p}) {key} nr {rg['nr']} {variant} tile {tile}"
                        rm = launch(ops, c, rg, "rm", tile, splits, variant, wh0, zh0)
                        worst[key, tile] = max(worst.get((key, tile), 0.0), check_slabs(rm, n, p, ri, variant, splits, what, wh0=wh0, zh0=zh0))
                        if tile != 256:
                            assert np.array_equal(rm, launch(ops, c, rg, "tr", tile, splits, variant, wh0, zh0)), what
    print(f"bf3 backward isolation ({n}, {p}): worst err/bound " + ", ".join(f"{k} tile {t}: {w:.3f}" for (k, t), w in worst.items()))


def test_backward_bf3_wide_rs_part(ops):
    """mmd_backward_bf3_wide_kernel with the row sums handed in.  rs_part is written by the test with values unrelated to W, so
    the output follows it only if the kernel folds exactly the slab's slots s0 .. s1 with stride ldrs at the clamped row: one
    slab folds both slots, two slabs (kchunk = 128) one slot each; four slabs (kchunk = 64) cut the slots, and the launch must
    ignore rs_part -- filled with NaN there -- and equal the launch without it bit for bit."""
    n, p = 128, 130
    c = operands(n, p)
    d = c["d"]
    rng = np.random.default_rng(5)
    worst = 0.0
    for ri, rg in enumerate(c["ranges"]):
        nr = rg["nr"]
        cells = (rng.normal(size=(2, nr)) * 1e-2).astype(np.float32)
        rsimg = image32(cells, nr + 5)
        nanimg = Image(2, nr, nr + 5)
        m64s = {v: ref.bwd_bf3_mul64(rg, v) for v in ref.BWD_BF3_MULS}
        for variant in ref.BWD_BF3_MULS:
            for splits in (1, 2):
                what = f"rs_part nr {nr} {variant} splits {splits}"
                o = launch(ops, c, rg, "rm", 256, splits, variant, rs_part=rsimg.view)
                assert np.array_equal(o, launch(ops, c, rg, "rm", 256, splits, variant, rs_part=rsimg.view)), what
                args = (rg["wh"], rg["wl"], d["zh"], d["zl"], rg["zrow"], m64s[variant])
                _, live, slabs = ref.bf3_slabs(d["kn"], splits)
                total_w, total_b = 0.0, 0.0
                for s, (k0, k1) in enumerate(slabs):
                    mine = cells[k0 >> 7:(k1 + 127) >> 7].astype(np.float64)
                    want = ref.backward_bf3_ref(*args, k0, k1, rs=mine.sum(0))
                    bound = ref.backward_bf3_bound(*args, k0, k1, rs_cells=mine)
                    worst = max(worst, check_within(o[s], want, bound, f"{what} slab {s}"))
                    total_w, total_b = total_w + want, total_b + bound
                ref.cap_ok(total_b, total_w, ref.CAP_BWD_BF3)
            plain = launch(ops, c, rg, "rm", 256, 4, variant)
            assert np.array_equal(plain, launch(ops, c, rg, "rm", 256, 4, variant, rs_part=nanimg.view)), f"nr {nr} {variant}: rs_part not ignored"
    print(f"bf3 backward rs_part (128, 130): worst err/bound {worst:.3f}")


@pytest.mark.parametrize("rows,p", [(66, 7), (130, 65), (200, 130)])
def test_bf3_prepare_images_pads_and_guards(ops, rows, p):
    """vgan_mmd_bf3_prepare: hi = RNE bf16(z) and lo = bf16(z - hi) exactly; every pad cell -- Zh/Zl[:, p:kp], ZT[:, rows:kn],
    ZT[p:kp, :] -- written zero over a non-zero fill; nothing past the images touched; and the scalar path (ldz % 4 != 0, or a
    base 4 bytes off 16-byte alignment) bit-equal to the aligned vector launch.  Z's own pad columns hold NaN."""
    rng = np.random.default_rng(rows + p)
    Z = rng.normal(size=(rows, p)).astype(np.float32)
    kp, kn = ref.pad64(p), ref.pad64(rows)
    zh, zl = ref.split_bf16(Z)
    want_h, want_l = np.zeros((rows, kp), dtype=np.uint16), np.zeros((rows, kp), dtype=np.uint16)
    want_h[:, :p], want_l[:, :p] = ref.bf16_bits(zh), ref.bf16_bits(zl)
    ld4 = (p + 3) // 4 * 4
    odd = p if p % 4 else p + 1
    first = None
    for name, ldz, off in (("aligned", ld4, 0), ("ldz % 4 != 0", odd, 0), ("base + 4 bytes", ld4, 1)):
        zimg = Image(rows, p, ldz, off)
        zimg.view.copy_(torch.as_tensor(Z))
        assert (zimg.view.data_ptr() % 16 == 0) == (off == 0)
        imgs = [Image(rows, kp, kp, 0, torch.int16, SENT16), Image(rows, kp, kp, 0, torch.int16, SENT16),
                Image(kp, kn, kn, 0, torch.int16, SENT16), Image(kp, kn, kn, 0, torch.int16, SENT16)]
        ops.mmd_bf3_prepare(zimg.view, rows, p, *(i.view for i in imgs))
        torch.cuda.synchronize()
        got = [i.read(np.ones((i.rows, i.cols), dtype=bool)).view(np.uint16) for i in imgs]  # all written, the guards untouched
        assert np.array_equal(got[0], want_h), f"{name}: hi is not the RNE bf16 of z"
        assert np.array_equal(got[1], want_l), f"{name}: lo is not bf16(z - hi)"
        for t, w in ((got[2], want_h), (got[3], want_l)):
            assert np.array_equal(t[:, :rows], w.T) and not t[:, rows:].any() and not t[p:].any(), f"{name}: transposed image"
        if first is None:
            first = got
        assert all(np.array_equal(a, b) for a, b in zip(got, first)), f"{name}: differs from the aligned launch"
    # the row-major images alone (no transposed copies asked for)
    imgs = [Image(rows, kp, kp, 0, torch.int16, SENT16), Image(rows, kp, kp, 0, torch.int16, SENT16)]
    zimg = Image(rows, p, ld4)
    zimg.view.copy_(torch.as_tensor(Z))
    ops.mmd_bf3_prepare(zimg.view, rows, p, imgs[0].view, imgs[1].view)
    torch.cuda.synchronize()
    for i, w in zip(imgs, (want_h, want_l)):
        assert np.array_equal(i.read(np.ones((rows, kp), dtype=bool)).view(np.uint16), w)
