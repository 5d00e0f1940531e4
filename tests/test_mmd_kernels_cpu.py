"""The float64 reference and the error bounds of tests/mmd_ref.py, checked without a GPU: the tile tables scatter to the dense
W and sum to the dense block sums (every grad_mode, every rank of the row-sharded tables, tiles 64 / 128 / 256); the dense W
reproduces the oracle's closed-form gradient; the existing per-tile float64 providers agree with it; a float32 emulation of
the fp32 Gram kernel stays inside the bounds, and the bounds respect their caps, at every case of the GPU tier; and one wrong
element on a ragged tile edge is rejected by the element-wise comparison while the old 1e-3 * max|dZ| criterion lets it pass."""
import numpy as np
import pytest
import torch

import mmd_ref as ref
from cpu_ops import CpuOps
from oracle import vgan_oracle as orc
from vgan_amd import lib

TABLE_N = [33, 65, 100, 128, 130, 192]
TABLE_TILES = [64, 128, 256]


def table(n, mode, rank=0, world=1, tile=64):
    flat, cnt = lib.build_tiles(n, mode, rank, world, tile)
    return np.asarray(flat, dtype=np.int64).reshape(cnt, 8)


def owned(n, mode, rank=0, world=1):
    """(nr, wrow0) of the W image a table writes."""
    if world > 1:
        lo, hi = n * rank // world, n * (rank + 1) // world
        return hi - lo, n + lo
    return {0: (0, 0), 1: (n, n), 2: (2 * n, 0)}[mode]


@pytest.fixture(scope="module")
def dense():
    cache = {}

    def get(n):
        if n not in cache:
            Z, sq, bw = ref.make_case(n, 5)
            z64 = Z.astype(np.float64)
            cache[n] = (z64, sq.astype(np.float64), bw) + ref.dense_weights(z64, sq.astype(np.float64), n, bw)
        return cache[n]
    return get


def block_sums(M, n):
    return np.array([M[:n, :n].sum(), M[n:, :n].sum(), M[n:, n:].sum()])


@pytest.mark.parametrize("tile", TABLE_TILES)
@pytest.mark.parametrize("n", TABLE_N)
def test_tables_scatter_to_the_dense_weights_and_sum_to_the_block_sums(dense, n, tile):
    z64, s64, bw, L, K, W = dense(n)
    want = block_sums(K, n)
    lsum = L.sum()
    for mode in (0, 1, 2):
        tb = table(n, mode, tile=tile)
        nr, wrow0 = owned(n, mode)
        img, written, clash = ref.scatter(tb, W, wrow0, nr, tile, with_clash=True)
        assert written.all(), (mode, "unwritten elements")
        assert clash <= 1e-12 * np.abs(W).max(), (mode, clash)
        if nr:
            assert np.abs(img - W[wrow0:wrow0 + nr]).max() <= 1e-12 * np.abs(W).max()
        st = ref.reduce_stats(tb, ref.tile_sums(tb, K, tile), ref.tile_sums(tb, L, tile))
        np.testing.assert_allclose(st[:3], want, rtol=1e-12)
        np.testing.assert_allclose(st[3], lsum, rtol=1e-12)
    for world in (2, 3, 4):
        total = np.zeros(4)
        for rank in range(world):
            tb = table(n, 1, rank, world, tile)
            nr, wrow0 = owned(n, 1, rank, world)
            img, written, clash = ref.scatter(tb, W, wrow0, nr, tile, with_clash=True)
            assert written.all(), (world, rank, "unwritten elements")
            assert clash <= 1e-12 * np.abs(W).max()
            assert np.abs(img - W[wrow0:wrow0 + nr]).max() <= 1e-12 * np.abs(W).max()
            total += ref.reduce_stats(tb, ref.tile_sums(tb, K, tile), ref.tile_sums(tb, L, tile))
        np.testing.assert_allclose(total[:3], want, rtol=1e-12)
        np.testing.assert_allclose(total[3], lsum, rtol=1e-12)


@pytest.mark.parametrize("n,p", [(33, 4), (65, 7), (100, 20)])
def test_dense_weights_reproduce_the_oracle_gradient(n, p):
    Z, _, bw = ref.make_case(n, p)
    z64 = Z.astype(np.float64)
    s64 = (z64 * z64).sum(1)  # the oracle takes its own norms
    _, _, W = ref.dense_weights(z64, s64, n, bw)
    dZ = ref.backward_ref(W, z64, 0, 2 * n)
    Uo = np.ones((n, p))
    dX, dY, _ = orc.mmd_backward(z64[:n], z64[n:], Uo, 1.0, float(bw), with_dx=True)
    dY1, _ = orc.mmd_backward(z64[:n], z64[n:], Uo, 1.0, float(bw))
    scale = np.abs(dZ).max()
    assert np.abs(dZ[:n] - dX).max() <= 1e-12 * scale
    assert np.abs(dZ[n:] - dY).max() <= 1e-12 * scale
    assert np.abs(ref.backward_ref(W[n:], z64, n, n) - dY1).max() <= 1e-12 * scale


@pytest.mark.parametrize("mults", [None, ref.multipliers(3, 3.0), ref.multipliers(6, 1.5)])
@pytest.mark.parametrize("n,p,mode,rank,world", [(65, 7, 1, 0, 1), (100, 20, 2, 0, 1), (100, 20, 1, 1, 3)])
def test_fp32_provider_agrees_with_the_dense_reference(n, p, mode, rank, world, mults):
    Z, sq, bw = ref.make_case(n, p)
    z64, s64 = Z.astype(np.float64), sq.astype(np.float64)
    L, K, W = ref.dense_weights(z64, s64, n, bw, mults)
    tb = table(n, mode, rank, world)
    nr, wrow0 = owned(n, mode, rank, world)
    Wg = torch.full((nr, 2 * n), float("nan"), dtype=torch.float64)
    partial = torch.zeros(len(tb), 4, dtype=torch.float64)
    ops = CpuOps()
    tt = torch.as_tensor(tb, dtype=torch.int32)
    ops.mmd_gram(torch.as_tensor(Z), torch.as_tensor(sq), n, p, torch.tensor([float(bw)]), tt, False, Wg, wrow0, partial, multipliers=mults)
    img, written = ref.scatter(tb, W, wrow0, nr, 64)
    assert written.all() and not torch.isnan(Wg).any()
    assert np.abs(Wg.numpy() - img).max() <= 1e-12 * np.abs(W).max()
    # (the provider rounds its sums to float32)
    np.testing.assert_allclose(partial[:, 0].numpy(), ref.tile_sums(tb, K, 64), rtol=2.0 ** -23)
    ops.mmd_gram(torch.as_tensor(Z), torch.as_tensor(sq), n, p, None, tt, True, None, 0, partial)
    np.testing.assert_allclose(partial[:, 1].numpy(), ref.tile_sums(tb, L, 64), rtol=2.0 ** -23)


@pytest.mark.parametrize("tile", TABLE_TILES)
@pytest.mark.parametrize("n,d,mode", [(65, 96, 1), (100, 130, 2)])
def test_bf3_provider_agrees_with_the_dense_reference(n, d, mode, tile):
    Z, sq, bw = ref.make_case(n, d)
    zh, zl = ref.split_bf16(Z)
    kp = (d + 63) // 64 * 64
    Zh, Zl = torch.zeros(2 * n, kp, dtype=torch.int16), torch.zeros(2 * n, kp, dtype=torch.int16)
    Zh[:, :d] = torch.as_tensor(zh).to(torch.bfloat16).view(torch.int16)
    Zl[:, :d] = torch.as_tensor(zl).to(torch.bfloat16).view(torch.int16)
    L, K, W = ref.dense_weights((zh.astype(np.float64), zl.astype(np.float64)), sq.astype(np.float64), n, bw)
    tb = table(n, mode, tile=tile)
    nr, wrow0 = owned(n, mode)
    Wh, Wl = torch.full((nr, 2 * n), 0x7FC0, dtype=torch.int16), torch.full((nr, 2 * n), 0x7FC0, dtype=torch.int16)
    partial = torch.zeros(len(tb), 4)
    CpuOps().mmd_gram_bf3(Zh, Zl, torch.as_tensor(sq), n, torch.tensor([float(bw)]), torch.as_tensor(tb, dtype=torch.int32), Wh, Wl, wrow0,
                          partial, tile=tile)
    got = Wh.view(torch.bfloat16).double().numpy() + Wl.view(torch.bfloat16).double().numpy()
    img, written = ref.scatter(tb, W, wrow0, nr, tile)
    assert written.all()
    assert (np.abs(got - img) <= (1e-12 + 2.0 ** -16) * np.abs(img)).all()
    np.testing.assert_allclose(partial[:, 0].double().numpy(), ref.tile_sums(tb, K, tile), rtol=2.0 ** -23)


def fp32_bound_ratio(n, p, mults):
    Z, sq, bw = ref.make_case(n, p)
    z64, s64 = Z.astype(np.float64), sq.astype(np.float64)
    L, K, W = ref.dense_weights(z64, s64, n, bw, mults)
    bound = ref.weight_bound(z64, s64, n, bw, p, mults)
    cap = ref.cap_ok(bound, W, ref.CAP_FP32)
    K32, W32 = ref.emulate_gram_fp32(Z, sq, n, bw, mults)
    worst = float((np.abs(W32.astype(np.float64) - W) / bound).max())
    # the per-element part of the sum bound, on the emulation's K
    slope = sum(np.exp(-L / sc) / sc for sc in ref.scales(bw, mults))
    kb = slope * ref.l_bound(z64, s64, L, p) + ref.C_EPI * ref.U * K
    worst_k = float((np.abs(K32.astype(np.float64) - K) / kb).max())
    return cap, worst, worst_k


@pytest.mark.parametrize("mults", [None] + [ref.multipliers(*m) for m in ref.FP32_MULTS], ids=["default", "3x3.0", "6x1.5"])
@pytest.mark.parametrize("n,p", ref.FP32_CASES + [(n, ref.SHARD_P) for n, _ in ref.SHARD_CASES])
def test_float32_emulation_stays_inside_the_bounds_and_the_caps_hold(n, p, mults):
    cap, worst, worst_k = fp32_bound_ratio(n, p, mults)
    print(f"fp32 ({n}, {p}) max(bound) / max|W| {cap:.2e}, emulation worst err/bound: W {worst:.3f}, K {worst_k:.3f}")
    assert worst <= 1.0 and worst_k <= 1.0


@pytest.mark.parametrize("n,d", ref.BF3_CASES + [(n, ref.SHARD_D) for n, _ in ref.SHARD_CASES])
def test_split_bf16_caps_hold(n, d):
    Z, sq, bw = ref.make_case(n, d)
    zh, zl = ref.split_bf16(Z)
    zz = (zh.astype(np.float64), zl.astype(np.float64))
    s64 = sq.astype(np.float64)
    _, _, W = ref.dense_weights(zz, s64, n, bw)
    kp = (d + 63) // 64 * 64
    cap = ref.cap_ok(ref.weight_bound(zz, s64, n, bw, 3 * kp, pair=True), W, ref.CAP_BF3)
    print(f"bf3 ({n}, {d}) max(bound) / max|W| {cap:.2e}")


def test_one_wrong_element_on_a_ragged_edge_is_rejected_where_the_old_criterion_passes():
    """n = 100, grad_mode 2, 64-wide tiles: the XX tile (0, 64) is ragged (36 columns) and mirrored.  One stored element of it
    is put off by 1e-3 relative, in the direct image and, separately, in the mirrored one.  The element-wise comparison against
    scatter() within weight_bound rejects both; the old criterion -- dZ from the same W within 1e-3 * max|dZ| -- accepts both."""
    n, p = 100, 20
    Z, sq, bw = ref.make_case(n, p)
    z64, s64 = Z.astype(np.float64), sq.astype(np.float64)
    _, _, W = ref.dense_weights(z64, s64, n, bw)
    bound = ref.weight_bound(z64, s64, n, bw, p)
    ref.cap_ok(bound, W, ref.CAP_FP32)
    tb = table(n, 2)
    edge = [r for r in tb.tolist() if r[0] == 0 and r[1] == 64 and (r[4] & ref.TF_SLOT) == 0]
    assert len(edge) == 1 and edge[0][3] == n and edge[0][4] & ref.TF_MIRROR and edge[0][4] & ref.TF_STORE
    img, written = ref.scatter(tb, W, 0, 2 * n, 64)
    assert written.all()
    dz = ref.backward_ref(img, z64, 0, 2 * n)
    i, j = 63, 99  # last row, last valid column of the ragged tile
    for (r, c), what in (((i, j), "direct"), ((j, i), "mirrored")):
        bad = img.copy()
        bad[r, c] *= 1.0 + 1e-3
        err = np.abs(bad - W)
        assert (err <= bound).sum() == err.size - 1 and err[r, c] > bound[r, c], what
        dz_bad = ref.backward_ref(bad, z64, 0, 2 * n)
        assert np.abs(dz_bad - dz).max() <= 1e-3 * np.abs(dz).max(), what  # the old criterion does not see it


def test_bf3_gram_rejects_a_row_stride_that_breaks_the_vector_stores():
    """The split-bf16 epilogues store 16 bytes at a time wherever the element offset is a multiple of 8; with the bases they are
    given that is a 16-byte aligned address only if ldw % 8 == 0, which vgan_mmd_gram_bf3 therefore checks (before any launch:
    the call below needs no GPU; its tile edge, 7, is one the next check of the host function rejects as well, so that no
    regression of this check can end in a launch on these host addresses)."""
    import ctypes
    L = lib.load()
    buf = torch.zeros(4096, dtype=torch.int16)
    f32 = torch.zeros(64)
    p16, pf = ctypes.c_void_p(buf.data_ptr()), ctypes.c_void_p(f32.data_ptr())
    assert buf.data_ptr() % 16 == 0 and f32.data_ptr() % 16 == 0
    tiles = torch.zeros(8, dtype=torch.int32)
    rc = L.vgan_mmd_gram_bf3(p16, p16, 64, pf, 8, pf, ctypes.c_void_p(tiles.data_ptr()), 1, 7, p16, p16, 20, 8, pf, None, 0, 0, 0, None, 0, 0,
                             None, 0, None, 0, None)
    assert rc != 0 and b"ldw % 8 == 0" in L.vgan_last_error()
