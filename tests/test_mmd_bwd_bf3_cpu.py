"""The float64 reference and the bound of the split-bf16 MMD backward product (tests/mmd_ref.py, 'split-bf16 backward'), checked
without a GPU at every case of tests/test_mmd_bwd_bf3_gpu.py: the bound respects its cap (max(bound) <= 2e-3 max |want|), a
float32 numpy emulation of the product stays inside it, and the same emulation with Wh.Zl dropped, with Wl.Zh dropped, with
Wl.Zl added or with the row sum taken over Wh only falls outside it -- while some of those mutants pass the old global criterion
2e-5 max |want| (Wl.Zl added: on a true split it is 2^-16 of the product and under 0.03 of the bound; it is rejected on the three
small rows with a fat lo image every W carries, mmd_ref.BWD_BF3_SMALL, and at the term-isolation cases); the slab bookkeeping (kchunk, live slabs, the slabs' references sum to the whole) and the library's tile rule
(vgan_mmd_backward_bf3_tile, a host function) at its boundaries."""
import numpy as np
import pytest

import mmd_ref as ref
from vgan_amd import lib

ISOLATION_CASES = [(65, 65), (100, 130)]
ISOLATIONS = ["Wh = 0", "Zh = 0", "Wh = Zh = 0"]


def cases(n, p):
    """(label, wh, wl, zh, zl, zrow, mul64, mul32, shift32) of every whole-product case of the GPU tier at this shape."""
    d = ref.bwd_bf3_data(n, p)
    for rg in d["ranges"]:
        zrow = d["Z"][rg["wrow0"]:rg["wrow0"] + rg["nr"]].astype(np.float64)
        for variant in ref.BWD_BF3_MULS:
            m32 = None if variant == "none" else rg["mul"]
            s32 = rg["shift"] if variant == "mul+shift" else None
            yield (rg["nr"], rg["wrow0"], variant), rg["wh"], rg["wl"], d["zh"], d["zl"], zrow, ref.bwd_bf3_mul64(rg, variant), m32, s32


def isolate(which, wh, zh):
    return (np.zeros_like(wh) if "Wh" in which else wh), (np.zeros_like(zh) if "Zh" in which else zh)


@pytest.mark.parametrize("n,p", ref.BWD_BF3_CASES)
def test_cap_emulation_and_the_four_mutations(n, p):
    caps, inside, old_pass = [], [], 0
    caught = {m: [] for m in ref.BWD_BF3_MUTATIONS}
    for label, wh, wl, zh, zl, zrow, m64, m32, s32 in cases(n, p):
        want = ref.backward_bf3_ref(wh, wl, zh, zl, zrow, m64)
        bound = ref.backward_bf3_bound(wh, wl, zh, zl, zrow, m64)
        caps.append(ref.cap_ok(bound, want, ref.CAP_BWD_BF3))
        got = ref.emulate_backward_bf3(wh, wl, zh, zl, zrow, m32, s32).astype(np.float64)
        inside.append(float((np.abs(got - want) / bound).max()))
        assert inside[-1] <= 1.0, (label, inside[-1])
        for mutation in ref.BWD_BF3_MUTATIONS:
            bad = ref.emulate_backward_bf3(wh, wl, zh, zl, zrow, m32, s32, mutation=mutation).astype(np.float64)
            err = np.abs(bad - want)
            frac = float((err > bound).mean())
            assert frac > 0, f"{label}: '{mutation}' stays inside the bound"
            caught[mutation].append(frac)
            old_pass += err.max() <= 2e-5 * np.abs(want).max()
    print(f"bf3 backward ({n}, {p}): max(bound) / max|want| {min(caps):.2e} .. {max(caps):.2e}, emulation worst err/bound {max(inside):.3f}, "
          + ", ".join(f"{m}: {min(v):.0%} .. {max(v):.0%} outside" for m, v in caught.items())
          + f"; {old_pass} mutants pass the old criterion 2e-5 max|want|")


def test_some_mutant_passes_the_old_global_criterion():
    """The per-element bound is the stricter check: over the GPU tier's cases some mutant that the bound rejects (asserted
    above for every one) has max |err| <= 2e-5 max |want|, the criterion of test_hip_parity.py."""
    n_pass = 0
    for n, p in ref.BWD_BF3_CASES:
        for label, wh, wl, zh, zl, zrow, m64, m32, s32 in cases(n, p):
            want = ref.backward_bf3_ref(wh, wl, zh, zl, zrow, m64)
            bound = ref.backward_bf3_bound(wh, wl, zh, zl, zrow, m64)
            for mutation in ref.BWD_BF3_MUTATIONS:
                err = np.abs(ref.emulate_backward_bf3(wh, wl, zh, zl, zrow, m32, s32, mutation=mutation).astype(np.float64) - want)
                n_pass += bool(err.max() <= 2e-5 * np.abs(want).max() and (err > bound).any())
    assert n_pass >= 1
    print(f"{n_pass} mutants pass 2e-5 max|want| and are rejected by the bound")


@pytest.mark.parametrize("which", ISOLATIONS)
@pytest.mark.parametrize("n,p", ISOLATION_CASES)
def test_term_isolation_cases_respect_the_cap(n, p, which):
    """The GPU tier zeroes Wh, Zh or both: the bound, formed from the images given, shrinks with them and must still mean
    something.  With both zero acc is exactly zero (the one product left, Wl.Zl, is never formed)."""
    both = which == "Wh = Zh = 0"
    for label, wh, wl, zh, zl, zrow, m64, m32, s32 in cases(n, p):
        a, c = isolate(which, wh, zh)
        want = ref.backward_bf3_ref(a, wl, c, zl, zrow, m64)
        bound = ref.backward_bf3_bound(a, wl, c, zl, zrow, m64, exact_acc=both)
        ref.cap_ok(bound, want, ref.CAP_BWD_BF3)
        full = ref.backward_bf3_bound(wh, wl, zh, zl, zrow, m64)
        assert (bound <= full).all() and bound.max() < (0.05 if both or "Wh" in which else 1.0) * full.max()
        if both:
            assert np.array_equal(want, ref.backward_bf3_ref(a, wl, c, np.zeros_like(zl), zrow, m64))  # acc = 0
        got = ref.emulate_backward_bf3(a, wl, c, zl, zrow, m32, s32).astype(np.float64)
        assert (np.abs(got - want) <= bound).all(), label
        # the term the kernel must not form is visible against the shrunken bound
        bad = ref.emulate_backward_bf3(a, wl, c, zl, zrow, m32, s32, mutation="Wl.Zl added").astype(np.float64)
        assert (np.abs(bad - want) > bound).any(), label


@pytest.mark.parametrize("n,p", ref.BWD_BF3_CASES)
def test_slab_bookkeeping(n, p):
    d = ref.bwd_bf3_data(n, p)
    kn = d["kn"]
    assert kn == ref.pad64(2 * n) and kn % 64 == 0
    for splits in ref.bwd_bf3_splits(n):
        kchunk, live, slabs = ref.bf3_slabs(kn, splits)
        assert kchunk == -(-(kn // 64) // splits) * 64 and live == -(-kn // kchunk) and len(slabs) == live <= splits
        assert slabs[0][0] == 0 and slabs[-1][1] == kn and all(a[1] == b[0] for a, b in zip(slabs, slabs[1:]))
        assert all((k1 - k0) % 64 == 0 and 0 < k1 - k0 <= kchunk for k0, k1 in slabs)
        if splits == 40:
            assert live < splits
        if splits == 4:
            assert kn == 256 and kchunk == 64 and live == 4  # two 32-deep stages of the 256-wide loop: nk = 2 < NST
        for label, wh, wl, zh, zl, zrow, m64, m32, s32 in cases(n, p):
            whole = ref.backward_bf3_ref(wh, wl, zh, zl, zrow, m64)
            parts = sum(ref.backward_bf3_ref(wh, wl, zh, zl, zrow, m64, k0, k1) for k0, k1 in slabs)
            assert np.abs(parts - whole).max() <= 1e-12 * np.abs(whole).max()
            # the slabs' bounds add up to no more than the whole's (K and the sums both shrink)
            assert (sum(ref.backward_bf3_bound(wh, wl, zh, zl, zrow, m64, k0, k1) for k0, k1 in slabs)
                    <= ref.backward_bf3_bound(wh, wl, zh, zl, zrow, m64) * (1 + 1e-12)).all()
    assert ref.bf3_slabs(64, 1) == (64, 1, [(0, 64)]) and ref.bf3_slabs(320, 2) == (192, 2, [(0, 192), (192, 320)])
    assert ref.bf3_slabs(320, 3) == (128, 3, [(0, 128), (128, 256), (256, 320)]) and ref.bf3_slabs(192, 40)[:2] == (64, 3)


def test_a_slab_that_takes_its_neighbours_columns_cancels_in_the_sum_but_not_per_slab():
    """What the per-slab check is for: move one K tile from slab 1 to slab 0.  The sum is unchanged, each slab is wrong."""
    n, p = 130, 200
    label, wh, wl, zh, zl, zrow, m64, m32, s32 = next(cases(n, p))
    kchunk, live, slabs = ref.bf3_slabs(ref.pad64(2 * n), 2)
    (a0, a1), (b0, b1) = slabs
    moved = [ref.backward_bf3_ref(wh, wl, zh, zl, zrow, m64, a0, a1 + 64), ref.backward_bf3_ref(wh, wl, zh, zl, zrow, m64, b0 + 64, b1)]
    whole = ref.backward_bf3_ref(wh, wl, zh, zl, zrow, m64)
    assert (np.abs(moved[0] + moved[1] - whole) <= ref.backward_bf3_bound(wh, wl, zh, zl, zrow, m64)).all()
    for got, (k0, k1) in zip(moved, slabs):
        err = np.abs(got - ref.backward_bf3_ref(wh, wl, zh, zl, zrow, m64, k0, k1))
        assert (err > ref.backward_bf3_bound(wh, wl, zh, zl, zrow, m64, k0, k1)).mean() > 0.9


def test_tile_rule_at_its_boundaries():
    """vgan_mmd_backward_bf3_tile: a forced edge comes back as given; 256 x 128 tiles need nr >= 256 and wide_tiles * splits >=
    256; 128-wide tiles need big_tiles * splits >= 512; otherwise 64."""
    rule = lib.load().vgan_mmd_backward_bf3_tile
    for nr, p, splits in ((1, 1, 1), (32, 7, 40), (256, 128 * 256, 1), (100000, 100000, 64)):
        for tile in (64, 128, 256):
            assert rule(nr, p, splits, tile) == tile
    # wide_tiles = ceil(p / 128) * ceil(nr / 256)
    assert rule(256, 128 * 256, 1, 0) == 256 and rule(256, 128 * 255 + 1, 1, 0) == 256
    assert rule(256, 128 * 255, 1, 0) == 64       # 255 wide tiles; 510 big tiles
    assert rule(255, 128 * 256, 1, 0) == 128      # nr < 256: no wide tiles, but 512 big tiles
    assert rule(255, 128 * 1000, 1, 0) == 128
    assert rule(256, 128 * 64, 4, 0) == 256 and rule(256, 128 * 51, 5, 0) == 64 and rule(256, 128 * 52, 5, 0) == 256
    assert rule(257, 128 * 128, 1, 0) == 256 and rule(257, 128 * 127, 1, 0) == 64  # 254 wide tiles, 3 * 127 = 381 big tiles
    # big_tiles = ceil(p / 128) * ceil(nr / 128)
    assert rule(128, 128 * 512, 1, 0) == 128 and rule(128, 128 * 511, 1, 0) == 64 and rule(128, 128 * 511 + 1, 1, 0) == 128
    assert rule(129, 128 * 256, 1, 0) == 128 and rule(129, 128 * 255, 1, 0) == 64
    assert rule(128, 128 * 73, 7, 0) == 64 and rule(128, 128 * 74, 7, 0) == 128   # 511 and 518
    assert rule(64, 64, 1, 0) == 64 and rule(1, 1, 64, 0) == 64
