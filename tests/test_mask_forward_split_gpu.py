"""The lean fused mask forward with one batch row per workgroup (mask_forward_bf3_split_kernel, csrc/rows.hip) against the
one-wave-per-row kernel it replaces for 256 < d <= 1024: every output bit for bit.

Reference: the same inputs through mask_forward_bf3_kernel, which vgan_mask_project_forward_bf3_ex still launches whenever
the transposed images are asked for (ZTh / ZTl given: write_x, kn a multiple of 64 that is at least 2n).  With None, None
the launch goes to the split kernel when d > 256.  Shapes: the smallest at which each wave count and each ragged last chunk
occurs; (8, 256) stays on the old kernel on both sides and guards the dispatch boundary."""
import numpy as np
import pytest
import torch

from cpu_ops import CpuOps

pytestmark = pytest.mark.gpu

# (n, d): NT = 2 with one valid lane in the second wave; NT = 2 full; NT = 3 with one valid lane in the last chunk; NT = 4 with
# four valid lanes in the last wave (the c3 width); NT = 4 full; NT = 1 (old kernel on both sides)
SHAPES = [(8, 260), (8, 512), (16, 516), (24, 784), (8, 1024), (8, 256)]
I16 = dict(dtype=torch.int16, device="cuda")
SENT16, SENTF = 7, -123.5
BATCHES, CURSOR = 3, 4  # a 3-batch epoch table with the cursor at 4: batch 1 is the one used


@pytest.fixture(scope="module")
def ops():
    from vgan_amd.ops import HipOps
    return HipOps()


def dev(a, dtype=torch.float32):
    return torch.as_tensor(np.ascontiguousarray(a)).to(device="cuda", dtype=dtype)


def bits(t):
    return t.view(torch.int32)


_INPUTS, _REFS = {}, {}


def inputs(ops, n, d):
    """Inputs of one shape, shared by its tests and left unchanged."""
    if (n, d) in _INPUTS:
        return _INPUTS[(n, d)]
    rng = np.random.default_rng(7000 * n + d)
    rows_total = BATCHES * n + 5
    data = (rng.normal(size=(rows_total, d)) * 0.7 + rng.normal(size=(1, d)) * 2.0).astype(np.float32)
    logits = (rng.normal(size=(n, d)) * 10.0).astype(np.float32)
    logits[0, :] = 0.25             # all equal: s == 1/d, at the threshold
    logits[1, :] = 0.0
    logits[1, (3 * d) // 4] = 50.0  # a single dominant entry
    # beforehand, on the CPU: the random rows have mask entries on both sides of the 1/d threshold
    S_cpu, U_cpu = torch.zeros(n, d), torch.zeros(n, d)
    CpuOps().upper_softmax_forward(torch.as_tensor(logits), S_cpu, U_cpu)
    below = S_cpu.numpy()[2:] < np.float32(1.0) / np.float32(d)
    assert below.any(1).all() and (~below).any(1).all()
    table = np.stack([rng.permutation(rows_total)[:n] for _ in range(BATCHES)]).astype(np.int32)
    c = {"n": n, "d": d, "kp": (d + 63) // 64 * 64, "kn": (2 * n + 63) // 64 * 64, "table_cpu": table}
    c["data"], c["logits"], c["table"] = dev(data), dev(logits), dev(table, torch.int32)
    c["cursor"] = torch.full((1,), CURSOR, dtype=torch.int64, device="cuda")
    c["center"] = torch.zeros(d, device="cuda")
    ops.col_mean(c["data"], c["center"])
    _INPUTS[(n, d)] = c
    return c


def launch(ops, c, use_table, use_center, split, write_x=True, write_z=True):
    """One launch into fresh, sentinel-filled outputs.  split=False passes the transposed images: the old kernel."""
    n, d, kp, kn = c["n"], c["d"], c["kp"], c["kn"]
    o = {"S": torch.full((n, d), SENTF, device="cuda"), "Z": torch.full((2 * n, d), float("nan"), device="cuda"),
         "sq": torch.full((2 * n,), SENTF, device="cuda"), "Zh": torch.full((2 * n, kp), SENT16, **I16),
         "Zl": torch.full((2 * n, kp), SENT16, **I16), "xrow": torch.full((n,), -1, dtype=torch.int32, device="cuda")}
    ZTh, ZTl = (None, None) if split else (torch.zeros(kp, kn, **I16), torch.zeros(kp, kn, **I16))
    rowsel = dict(row_cursor=c["cursor"], row_batches=BATCHES, row_stride=n) if use_table else {}
    ops.mask_project_forward_bf3(c["logits"], c["data"], c["table"] if use_table else None, o["S"], o["Z"], o["sq"], o["Zh"], o["Zl"], ZTh, ZTl,
                                 center=c["center"] if use_center else None, write_x=write_x, write_z=write_z, xrow=o["xrow"], **rowsel)
    torch.cuda.synchronize()
    return o


def reference(ops, c, use_table, use_center):
    key = (c["n"], c["d"], use_table, use_center)
    if key not in _REFS:
        _REFS[key] = launch(ops, c, use_table, use_center, split=False)
    return _REFS[key]


def assert_same(got, ref, names):
    for k in names:
        a, b = got[k], ref[k]
        assert torch.equal(a, b), k
        if a.dtype == torch.float32:
            assert torch.equal(bits(a), bits(b)), k + " (bits)"


@pytest.mark.parametrize("use_center", [True, False], ids=["centre", "nocentre"])
@pytest.mark.parametrize("use_table", [True, False], ids=["table", "identity"])
@pytest.mark.parametrize("n,d", SHAPES)
def test_split_forward_is_bit_identical(ops, n, d, use_table, use_center):
    c = inputs(ops, n, d)
    ref = reference(ops, c, use_table, use_center)
    got = launch(ops, c, use_table, use_center, split=True)
    assert_same(got, ref, ["S", "sq", "xrow", "Zh", "Zl", "Z"])
    want_rows = torch.as_tensor(c["table_cpu"][CURSOR % BATCHES] if use_table else np.arange(n, dtype=np.int32))
    assert torch.equal(got["xrow"].cpu(), want_rows)
    # the threshold row and the dominant row came out as the mask expects them (no NaN, a full row of s == 1/d)
    assert bool(torch.isfinite(got["S"]).all()) and bool((got["S"][0] == float(np.float32(1.0) / np.float32(d))).all())
    assert bool((got["Zh"][:, d:] == SENT16).all()) and bool((got["Zl"][:, d:] == SENT16).all())


@pytest.mark.parametrize("n,d", SHAPES)
def test_write_z_off_leaves_z_alone(ops, n, d):
    c = inputs(ops, n, d)
    ref = reference(ops, c, True, True)
    got = launch(ops, c, True, True, split=True, write_z=False)
    assert bool(torch.isnan(got["Z"]).all()), "write_z = 0 must leave Z alone"
    assert_same(got, ref, ["S", "sq", "xrow", "Zh", "Zl"])


@pytest.mark.parametrize("write_z", [True, False], ids=["z", "noz"])
@pytest.mark.parametrize("n,d", SHAPES)
def test_write_x_off_leaves_the_x_halves_alone(ops, n, d, write_z):
    c = inputs(ops, n, d)
    ref = reference(ops, c, True, True)
    got = launch(ops, c, True, True, split=True, write_x=False, write_z=write_z)
    assert bool((got["Zh"][:n] == SENT16).all()) and bool((got["Zl"][:n] == SENT16).all()) and bool((got["sq"][:n] == SENTF).all())
    assert bool(torch.isnan(got["Z"][:n]).all())
    assert torch.equal(got["Zh"][n:], ref["Zh"][n:]) and torch.equal(got["Zl"][n:], ref["Zl"][n:])
    assert torch.equal(bits(got["sq"][n:]), bits(ref["sq"][n:]))
    assert_same(got, ref, ["S", "xrow"])
    if write_z:
        assert torch.equal(bits(got["Z"][n:]), bits(ref["Z"][n:]))
    else:
        assert bool(torch.isnan(got["Z"]).all())


def test_split_forward_is_deterministic(ops):
    c = inputs(ops, 24, 784)
    a = launch(ops, c, True, True, split=True)
    b = launch(ops, c, True, True, split=True)
    assert_same(a, b, ["S", "sq", "xrow", "Zh", "Zl", "Z"])
