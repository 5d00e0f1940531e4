"""In-launch K split of the chain products: argument checks of the two entry points and the trainer's `auto` rule (no GPU)."""
import ctypes

import pytest


def _lib():
    import vgan_amd
    return vgan_amd.lib, vgan_amd.lib.load()


def _fake(nbytes=4096):
    """A 16-byte aligned address that is never dereferenced: every call below is rejected before any launch."""
    buf = ctypes.create_string_buffer(nbytes + 16)
    return buf, ctypes.c_void_p(ctypes.addressof(buf) + (-ctypes.addressof(buf)) % 16)


def _rejected(lib, rc, needle):
    msg = lib.vgan_last_error()
    return rc == 1 and b"bad argument" in msg and needle in msg


def test_linear_ksplit_rejects_bad_arguments():
    _, lib = _lib()
    keep, p = _fake()
    f = lib.vgan_linear_backward_params_ksplit
    need = lib.vgan_linear_backward_params_ksplit_ws_bytes(52, 36, 4)
    assert need > 0
    assert _rejected(lib, f(p, 36, p, 52, p, 52, 300, 52, 36, 4, None, need, None), b"ws != nullptr")       # no workspace
    assert _rejected(lib, f(p, 36, p, 52, p, 52, 300, 52, 36, 4, p, need - 1, None), b"ws_bytes >= need")    # too small
    assert _rejected(lib, f(p, 36, p, 52, p, 52, 300, 52, 36, 0, p, need, None), b"parts >= 1")
    assert _rejected(lib, f(p, 36, p, 52, p, 52, 300, 52, 36, 9, p, 1 << 30, None), b"parts >= 1")
    assert _rejected(lib, f(p, 36, p, 52, p, 52, 300, 52, 36, 16, p, 1 << 30, None), b"parts >= 1")
    assert _rejected(lib, f(p, 38, p, 52, p, 52, 300, 52, 38, 2, p, 1 << 30, None), b"out % 4 == 0")         # not the 16-wave contract
    del keep


def test_ws_bytes_queries_are_monotone_in_parts():
    mod, lib = _lib()
    sizes = [lib.vgan_linear_backward_params_ksplit_ws_bytes(52, 784, parts) for parts in range(1, 9)]
    assert sizes[0] == 0 and all(b > a for a, b in zip(sizes, sizes[1:]))
    assert sizes[3] == 256 + 50 * 4 * 4096  # 25 x 2 tiles: tickets (padded to 256 bytes), then 4 slabs of 4 KB per tile
    assert lib.vgan_linear_backward_params_ksplit_ws_bytes(52, 784, 9) == 0 == lib.vgan_linear_backward_params_ksplit_ws_bytes(52, 784, 0)
    keep, p = _fake()
    q = (mod.GemmProblem * 2)()
    for x, (m, n, k) in zip(q, [(100, 52, 784), (36, 52, 784)]):
        x.a, x.b, x.c, x.kind, x.m, x.n, x.k, x.lda, x.ldb, x.ldc, x.splitk = p.value, p.value, p.value, mod.GEMM_TN, m, n, k, m, n, n, 1
    sizes = []
    for parts in range(1, 9):
        kp = (ctypes.c_int32 * 2)(parts, 1)
        sizes.append(lib.vgan_gemm_grouped_ksplit_ws_bytes(q, 2, kp))
    assert sizes[0] == 0 and all(b > a for a, b in zip(sizes, sizes[1:]))
    assert sizes[1] == 256 + 8 * 2 * 4096  # only the split problem's 4 x 2 tiles count
    del keep


def test_grouped_ksplit_rejects_bad_arguments():
    mod, lib = _lib()
    keep, p = _fake()
    f = lib.vgan_gemm_grouped_ksplit
    q = (mod.GemmProblem * 2)()

    def fill(splitk=1, k=784):
        for x, m in zip(q, (100, 36)):
            x.a, x.b, x.c, x.kind, x.m, x.n, x.k, x.lda, x.ldb, x.ldc, x.splitk = p.value, p.value, p.value, mod.GEMM_TN, m, 52, k, m, 52, 52, splitk

    fill()
    kp = (ctypes.c_int32 * 2)(4, 1)
    need = lib.vgan_gemm_grouped_ksplit_ws_bytes(q, 2, kp)
    assert need > 0
    assert _rejected(lib, f(q, 2, None, kp, None, need, None), b"ws != nullptr")
    assert _rejected(lib, f(q, 2, None, kp, p, need - 1, None), b"ws_bytes >= need")
    for bad in (0, 9, -1):
        assert _rejected(lib, f(q, 2, None, (ctypes.c_int32 * 2)(1, bad), p, 1 << 30, None), b"kparts[i] >= 1")
    fill(splitk=2)
    assert _rejected(lib, f(q, 2, None, kp, p, 1 << 30, None), b"splitk <= 1")   # slabs of C or the in-launch combine: not both
    fill(k=64)
    assert _rejected(lib, f(q, 2, None, kp, p, 1 << 30, None), b"!ksplit || ks16")  # not a launch of the 16-wave tiles
    del keep


def test_auto_rule_splits_only_the_measured_shapes(monkeypatch):
    from vgan_amd.trainer import CHAIN_KPARTS_AUTO, _round4, chain_kparts
    from vgan_amd.synth import latent_size

    def launches(n, d):
        """(tiles, K) of the M_4 launch and of the first chain-backward launch of a one-rank collapsed engine."""
        L = latent_size(d)
        e0, dp = _round4(L + 1), _round4(d)
        t32 = lambda r, c: ((r + 31) // 32) * ((c + 31) // 32)
        return (t32(dp, e0), n), e0

    for n, d in [(128, 20), (512, 166)]:  # c1, c2
        (tiles, k), e0 = launches(n, d)
        assert chain_kparts("auto", tiles, k) == 1
        # the TN group's contraction is e_4 = round4(d + 1) <= 168 there: below the rule's K whatever its tile count
        for t in range(1, 257):
            assert chain_kparts("auto", t, _round4(d + 1)) == 1
    (tiles, k), e0 = launches(1024, 784)  # c3: 25 x 2 tiles, K = 1024
    assert (tiles, k) == (50, 1024) and chain_kparts("auto", tiles, k) == CHAIN_KPARTS_AUTO
    assert chain_kparts("auto", tiles, k, chain_flops=True) == 1
    assert chain_kparts("auto", 200, 4100) == 1  # many tiles (c4 / c5 sizes): the chip is full already
    assert [chain_kparts(str(v), 3, 128) for v in (1, 2, 4, 8)] == [1, 2, 4, 8]  # the measurement knob forces a count
    with pytest.raises(ValueError):
        chain_kparts("3", 50, 1024)
