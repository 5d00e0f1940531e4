"""GPU tier for the mask / projection forward of every training step (csrc/rows.hip): vgan_mask_project_forward,
vgan_mask_project_forward_bf3 and _ex, called DIRECTLY through vgan_amd.ops.HipOps on every dispatch path and held to the
float64 restatement mask_forward_ref by check_mask_forward (tests/small_ops_ref.py).  tests/test_small_ops_cpu.py pins that
restatement, shows that every check bites, and asserts that the case lists below reach every kernel instantiation
(expected_kernel restates the dispatch rule; every test here re-derives it from the addresses and leading dimensions it
actually passes).  The equality tests (bf3 == two launches, split == old kernel) stay where they are: these tests hold the
near end of that chain to the truth.  Run with ``-m gpu`` on an MI355X.

Conventions: those of tests/test_small_ops_gpu.py, imported -- Guarded sentinel buffers (NaN / 0x5A5A, guard bands, NaN pads
of the inputs), Sel / SEL_MODES, the paths aligned / shifted / oddld, make_data with its split-tie probes, edge_logits.
Leading dimensions are larger than d everywhere; kp > d and kn > 2n are multiples of 64 with sentinel pads.

Bars (each derived, or the project's own; nothing fitted to the device)
  S          rtol 2e-5 + atol 2^-126 against softmax64 (the project's op-level bar).  With chain= the in-launch logit is an fma
             chain of e0 terms, off by at most delta_i = e0 2^-24 max_j sum_k |z_ik a_jk|; a row's softmax then moves by at
             most 2 delta_i relative: rtol 2e-5 + 2 delta_i per row.
  U          bit-equal to upper_mask_ref of the kernel's OWN S everywhere; decisions equal to the float64 ones wherever
             |S64 d - 1| > 1e-4 (the project's convention); at most 0.5 % of a case's random-row entries may be that near.
             d = 1: S == 1 and U == 1 exactly.
  Zx         bit-equal to float32 x - c (x without a centre).
  Zy         |Zy - (u x - c)| <= 2^-24 |u x - c| (1 + 2^-20) + 2^-149 with u the device's own mask and the right-hand side in
             float64: the one rounding of project_centred (fma(u, x, -c)), i.e. half an ulp, plus slack for the evaluation.
  sqx, sqy   sq_bar(d) against the float64 sum of squares of the device's own Z rows -- of split_value_ref of them with
             norm_split and always for the bf3 entry points; for write_z = 0 the rows of a write_z = 1 run of the same inputs.
  Zh, Zl     bit-equal to split_bf16_ref of the Z the same launch wrote; ZTh / ZTl the transposes of Zh / Zl.
  xrow       the restated selector.
Planted (n >= 3): a constant logits row (S == float32(1)/float32(d) exactly, U == 1: catches <= for <), the 200-wide linspace
row (underflow to 0, argmax d - 1), and -- without a centre -- a data row of +-2^k (1 + 2^-9 + 3 2^-19) selected by the
constant logits row, whose split norm is 1.14e-5 relative below its plain norm (4 to 10.6 sq bars).

Left out on purpose: the X-X rider (xx=), NaN / inf inputs, timing, any inspection of compiled code.
Each test prints one line with the largest error / bar ratio per quantity: observations, not thresholds.
"""
import collections
import itertools

import numpy as np
import pytest
import torch

import small_ops_ref as ref
from test_small_ops_gpu import (Guarded, SEL_MODES, Sel, dev, edge_logits, host, ld_for, make_data, ops,  # noqa: F401 (ops: fixture)
                                shift_for)

pytestmark = pytest.mark.gpu

Fwd = collections.namedtuple("Fwd", "n d path U zx centre norm_split sel e0", defaults=("aligned", True, True, True, False, "table3-cnb1", None))
Bf3 = collections.namedtuple("Bf3", "n d zt write_x write_z xrow centre sel e0", defaults=(True, True, True, True, True, "table3-cnb1-off0", None))

# ---- vgan_mask_project_forward ---------------------------------------------------------------------------------------------
# generic: 1, 3, 63, 65 (and 4100, past 4096) | NT 1: 4, 252, 256 | 2: 260, 512 | 3: 516, 640, 768 | 4: 772, 784, 1024 | 8: 1028, 1500, 2048 |
# 16: 2052, 4096.  Four rows per workgroup: n = 1 and 5 leave waves without a row.
FWD_WIDTHS = [1, 3, 63, 65, 4, 252, 256, 260, 512, 516, 640, 768, 772, 784, 1024, 1028, 1500, 2048, 2052, 4096, 4100]
FWD_ROWS = [1, 3, 4, 5, 63, 65]
FWD_EDGES = [Fwd(FWD_ROWS[k % 6], d, centre=k % 3 != 0, norm_split=k % 2 == 1) for k, d in enumerate(FWD_WIDTHS)]
# unaligned views are legal and must give the generic kernel's result: one width per NT
FWD_PATHS = [Fwd(n, d, path) for path in ("shifted", "oddld") for n, d in [(5, 256), (3, 260), (4, 640), (65, 784), (5, 1500), (3, 4096)]]
# options at one width per kernel: no U | the x-ahead form | no centre, split norms (the planted data row) | no centre, plain norms
FWD_OPTIONS = [c for d in (63, 252, 512, 768, 1024, 2048, 2052) for c in (
    Fwd(4, d, U=False), Fwd(5, d, zx=False, norm_split=True), Fwd(5, d, centre=False, norm_split=True), Fwd(4, d, centre=False))]
FWD_SELECT = [Fwd(37, d, centre=False, norm_split=True, sel=mode) for d in (64, 63) for mode in SEL_MODES]
# chain=: e0 = 4, 16, 20 are less than one chunk of kChainK = 16, exactly one, and a ragged second; d = 1016, 1020, 1024 straddle
# the 64 KB opt-in of the stage (16 rows of chain_pitch(d) floats: 65 280, 65 536, 65 792 bytes); n = 5 puts three rowless waves
# through the staging barriers
CHAIN_WIDTHS = [4, 260, 516, 784, 1016, 1020, 1024]
FWD_CHAIN = [Fwd(5 if k % 2 == 0 else 8, d, centre=k % 3 != 0, norm_split=k % 2 == 1, e0=e0)
             for k, (d, e0) in enumerate(itertools.product(CHAIN_WIDTHS, (4, 16, 20)))]
FWD_CHAIN += [c for d in (4, 260, 516, 784) for c in (Fwd(5, d, U=False, e0=16), Fwd(8, d, zx=False, centre=False, norm_split=True, e0=20))]
FWD_CHAIN_INVALID = Fwd(5, 260, "oddld", e0=16)
FWD_CASES = FWD_EDGES + FWD_PATHS + FWD_OPTIONS + FWD_SELECT + FWD_CHAIN

# ---- vgan_mask_project_forward_bf3 / _ex -----------------------------------------------------------------------------------
# transposed images: the tile is 64 (d + 8) bytes of dynamic LDS -- 65 536 at d = 1016, past the 64 KB opt-in at 1020 and 1024;
# n = 8, 16, 72, 136 are 1, 2, 9 and 17 row groups: the XCD map grp = (b % 8) C + b / 8 runs with C = 1, 1, 2, 3 and with
# trailing empty workgroups
BF3_ZT = [Bf3(n, d, centre=k % 2 == 0) for k, (n, d) in enumerate(
    [(8, 4), (16, 256), (72, 260), (136, 516), (72, 784), (16, 1016), (8, 1020), (136, 1024), (136, 4), (72, 1016), (16, 784), (8, 260),
     (16, 640), (8, 768), (136, 260), (72, 516)])]
# lean (no transposed images): d = 4, 252, 256 run mask_forward_bf3_kernel, wider rows the split kernel; write_x, write_z, xrow
BF3_LEAN = [Bf3((8, 16, 72)[(k + j) % 3], d, zt=False, write_x=wx, write_z=wz, xrow=(k + j) % 2 == 0, centre=j % 2 == 0)
            for k, d in enumerate([4, 252, 256, 260, 512, 516, 784, 1024]) for j, (wx, wz) in enumerate([(1, 1), (1, 0), (0, 1), (0, 0)])]
BF3_CHAIN = [Bf3(n, d, zt=False, e0=e0, centre=k % 2 == 0, xrow=k % 2 == 1, write_z=k % 3 != 0) for k, (n, d, e0) in enumerate(
    [(8, 4, 4), (72, 256, 16), (8, 260, 20), (72, 512, 16), (8, 640, 20), (72, 516, 4), (8, 784, 16), (72, 1024, 20), (8, 1016, 16), (72, 1020, 4)])]
# the row table with a device cursor past row_batches is the default selector above; here the other forms
BF3_SELECT = [Bf3(16, 784, zt=zt, sel=mode) for zt in (True, False) for mode in ("identity0", "table1-none-off0", "table3-c0-off0")]
BF3_CASES = BF3_ZT + BF3_LEAN + BF3_CHAIN + BF3_SELECT


def case_id(c):
    flags = [k for k in c._fields[2:] if k not in ("sel", "e0", "path", "norm_split") and not getattr(c, k)]
    return "-".join([f"n{c.n}", f"d{c.d}"] + ([c.path] if getattr(c, "path", "aligned") != "aligned" else []) + [f"no_{k}" for k in flags] +
                    (["norm_split"] if getattr(c, "norm_split", False) else []) +
                    ([c.sel] if c.sel != type(c)._field_defaults["sel"] else []) + ([f"e0_{c.e0}"] if c.e0 else []))


def _rows_total(c):
    return 90 if c.n == 37 else c.n + 5


def case_logits(c):
    """(rng, logits [n, d] or (za, At4)): the recipe default_rng(7 n + d), normal * 2.0 with the planted rows -- drawn first,
    without a GPU, so that the CPU tier can look at every case's softmax"""
    rng = np.random.default_rng(7 * c.n + c.d)
    return rng, (edge_logits(rng, c.n, c.d) if c.e0 is None else ref.chain_inputs(rng, c.n, c.d, c.e0))


def fwd_dispatch(c):
    """the kernel a Fwd case is expected to launch, from the addresses (mod 16) and leading dimensions the test will pass"""
    sh, lds = 4 * shift_for(c.path), [ld_for(c.d, c.path), ld_for(c.d, c.path, 8)] + ([] if c.e0 else [ld_for(c.d, c.path)])
    return ref.expected_kernel("fwd", c.d, c.n, [sh], lds, chain=c.e0 is not None)


def bf3_dispatch(c):
    return ref.expected_kernel("bf3", c.d, c.n, [0], [ld_for(c.d, "aligned"), ld_for(c.d, "aligned", 8)], chain=c.e0 is not None, zt=c.zt)


def _report(capsys, line):
    with capsys.disabled():
        print("\n    " + line, end="")


def _line(c, kernel, worst):
    return f"{case_id(c)} [{kernel}]: " + ", ".join(f"{k} {v:.4f}" if k == "near" else f"{k} {v:.3f}" for k, v in worst.items())


def region(g, r0, r1, c0=0, c1=None):
    """host copy of rows r0 .. r1, columns c0 .. c1 of a Guarded after asserting that nothing else in its allocation changed"""
    c1 = g.cols if c1 is None else c1
    h = host(g.buf)
    m = np.zeros(h.size, dtype=bool)
    for r in range(r0, r1):
        m[g.start + r * g.ld + c0:g.start + r * g.ld + c1] = True
    assert np.array_equal(h[~m].view(np.uint8), g.before[~m].view(np.uint8)), "write outside the contracted region"
    out = h[m].reshape(r1 - r0, c1 - c0)
    assert not (g.dtype.is_floating_point and np.isnan(out).any()), "contracted region not fully written"
    return out


class Inputs:
    """the device inputs of one case and their host copies"""

    def __init__(self, c, path):
        n, d, sh = c.n, c.d, shift_for(path)
        rng, lg = case_logits(c)
        self.lg, self.N = lg, _rows_total(c)
        self.x, self.data = make_data(rng, self.N, d, path)
        self.sel = Sel(rng, self.N, n, c.sel)
        self.const_rows, self.lin_rows = ([2], [1]) if n >= 3 else ([], [])
        if not c.centre and n >= 3 and d <= 1024:  # the planted data row, selected by the constant logits row (U == 1: Zy is x)
            self.x[self.sel.want[2]] = ref.planted_data_row(rng, d)
            self.data.t.copy_(dev(self.x))
            self.data.before = host(self.data.buf).copy()
        self.center = rng.normal(size=d).astype(np.float32) if c.centre else None
        self.C = Guarded(1, d, shift=sh, data=self.center[None]) if c.centre else None
        self.guards = [self.data] + ([self.C] if c.centre else [])
        self.delta = None
        if c.e0 is None:
            self.L = Guarded(n, d, ld_for(d, path), shift=sh, data=lg)
            self.guards.append(self.L)
        else:  # ldza > e0, ldat > e0 (a multiple of 4 on every path: the entry point requires it of At_4)
            za, At = lg
            self.za, self.At = Guarded(n, c.e0, c.e0 + 4 + sh, data=za), Guarded(d, c.e0, c.e0 + 8, data=At)
            self.guards += [self.za, self.At]
            self.delta = ref.chain_delta(za, At)
            rand = np.ones(n, dtype=bool)
            rand[self.const_rows + self.lin_rows] = False
            # (the inputs are scaled so: the chain bar of a random row stays inside the 1e-4 the decisions leave out)
            assert (2e-5 + 2 * self.delta[rand] < 1e-4).all()
        self.S64, self.X, _ = ref.mask_forward_ref(lg, self.x, self.sel.want, self.center)

    def chain(self, ops):
        return ops.logits_chain(self.za.t, self.At.t) if self.delta is not None else None

    def untouched(self):
        for g in self.guards:
            g.untouched()


# ================================================================================================ vgan_mask_project_forward
def launch_forward(ops, c, inp):
    n, d, sh = c.n, c.d, shift_for(c.path)
    ldz = ld_for(d, c.path, 8)
    o = dict(S=Guarded(n, d, shift=sh), U=Guarded(n, d, shift=sh) if c.U else None, Zx=Guarded(n, d, ldz, shift=sh) if c.zx else None,
             Zy=Guarded(n, d, ldz, shift=sh), sqx=Guarded(1, n) if c.zx else None, sqy=Guarded(1, n))
    t = lambda k: None if o[k] is None else (o[k].flat if k.startswith("sq") else o[k].t)
    L = None if c.e0 else inp.L
    bases = [g.t.data_ptr() for g in [L or inp.za, inp.data, inp.C, o["S"], o["U"], o["Zx"], o["Zy"]] if g is not None]
    lds = [inp.data.ld, ldz] + ([L.ld] if L else [])
    kernel = ref.expected_kernel("fwd", d, n, bases, lds, chain=c.e0 is not None)
    assert kernel == fwd_dispatch(c)
    ops.mask_project_forward(L.t if L else None, inp.data.t, inp.sel.table, t("S"), t("U"), t("Zx"), t("Zy"), t("sqx"), t("sqy"),
                             center=inp.C.flat if inp.C else None, norm_split=c.norm_split, chain=inp.chain(ops), **inp.sel.kw)
    torch.cuda.synchronize()
    return o, kernel


@pytest.mark.parametrize("c", FWD_CASES, ids=case_id)
def test_mask_project_forward(ops, capsys, c):
    inp = Inputs(c, c.path)
    o, kernel = launch_forward(ops, c, inp)
    assert kernel == ("generic" if c.path != "aligned" else kernel)
    out = {k: (None if g is None else (g.check()[0] if k.startswith("sq") else g.check())) for k, g in o.items()}
    inp.untouched()
    worst = ref.check_mask_forward(out, inp.S64, inp.X, inp.center, norm_split=c.norm_split, delta=inp.delta, const_rows=inp.const_rows,
                                   lin_rows=inp.lin_rows)
    _report(capsys, _line(c, kernel, worst))


def test_chain_off_the_vector_path_is_an_argument_error(ops):
    """the in-launch logits need the row-in-registers kernel: an odd leading dimension returns the invalid-argument error and
    nothing is launched (every output keeps its sentinels)"""
    from vgan_amd.lib import VganHipError
    c = FWD_CHAIN_INVALID
    assert fwd_dispatch(c) == "invalid"
    inp = Inputs(c, c.path)
    o = dict(S=Guarded(c.n, c.d), Zy=Guarded(c.n, c.d, ld_for(c.d, c.path, 8)), sqy=Guarded(1, c.n))
    with pytest.raises(VganHipError):
        ops.mask_project_forward(None, inp.data.t, inp.sel.table, o["S"].t, None, None, o["Zy"].t, None, o["sqy"].flat, center=inp.C.flat,
                                 chain=inp.chain(ops), **inp.sel.kw)
    torch.cuda.synchronize()
    for g in o.values():
        g.untouched()
    inp.untouched()


# ================================================================================================ vgan_mask_project_forward_bf3(_ex)
I16 = torch.int16


def launch_bf3(ops, c, inp, write_x=None, write_z=None):
    n, d = c.n, c.d
    write_x, write_z = (c.write_x if write_x is None else write_x), (c.write_z if write_z is None else write_z)
    kp, kn, ldz = (d // 64 + 1) * 64, (2 * n // 64 + 1) * 64, ld_for(d, "aligned", 8)
    o = dict(S=Guarded(n, d), Z=Guarded(2 * n, d, ldz), sq=Guarded(1, 2 * n), Zh=Guarded(2 * n, d, kp, I16), Zl=Guarded(2 * n, d, kp, I16),
             ZTh=Guarded(kp, 2 * n, kn, I16) if c.zt else None, ZTl=Guarded(kp, 2 * n, kn, I16) if c.zt else None,
             xrow=Guarded(1, n, dtype=torch.int32) if c.xrow else None)
    L = None if c.e0 else inp.L
    bases = [g.t.data_ptr() for g in [L or inp.za, inp.data, inp.C, o["S"], o["Z"], o["Zh"], o["Zl"], o["ZTh"], o["ZTl"]] if g is not None]
    kernel = ref.expected_kernel("bf3", d, n, bases, [inp.data.ld, ldz] + ([L.ld] if L else []), chain=c.e0 is not None, zt=c.zt)
    assert kernel == bf3_dispatch(c)
    kw = dict(inp.sel.kw)
    assert kw.pop("row_offset") == 0  # (this entry point has none)
    ops.mask_project_forward_bf3(L.t if L else None, inp.data.t, inp.sel.table, o["S"].t, o["Z"].t, o["sq"].flat, o["Zh"].t, o["Zl"].t,
                                 o["ZTh"].t if c.zt else None, o["ZTl"].t if c.zt else None, center=inp.C.flat if inp.C else None,
                                 write_x=bool(write_x), chain=inp.chain(ops), write_z=bool(write_z), xrow=o["xrow"].flat if c.xrow else None, **kw)
    torch.cuda.synchronize()
    return o, kernel


def collect_bf3(c, o, write_x, write_z):
    """the launch's outputs as check_mask_forward takes them; what write_x = 0 / write_z = 0 leave out keeps its sentinels"""
    n, d = c.n, c.d
    r0 = 0 if write_x else n
    sq = region(o["sq"], 0, 1, r0, 2 * n)[0]
    out = dict(S=o["S"].check(), sqy=sq[-n:])
    if write_x:
        out["sqx"] = sq[:n]
    if write_z:
        z = region(o["Z"], r0, 2 * n)
        out["Zy"] = z[-n:]
        if write_x:
            out["Zx"] = z[:n]
    else:
        o["Z"].untouched()
    for k in ("Zh", "Zl"):
        out[k] = np.zeros((2 * n, d), dtype=np.int16)
        out[k][r0:] = region(o[k], r0, 2 * n)
    if c.zt:
        out["ZTh"], out["ZTl"] = o["ZTh"].check(rows=d, cols=2 * n), o["ZTl"].check(rows=d, cols=2 * n)
    if c.xrow:
        out["xrow"] = o["xrow"].check()[0]
    return out


@pytest.mark.parametrize("c", BF3_CASES, ids=case_id)
def test_mask_project_forward_bf3(ops, capsys, c):
    inp = Inputs(c, "aligned")
    o, kernel = launch_bf3(ops, c, inp)
    out = collect_bf3(c, o, c.write_x, c.write_z)
    z_from = None
    if not c.write_z:  # the norms and images are those of the Z a Z-writing run of the same inputs leaves
        o2, _ = launch_bf3(ops, c, inp, write_x=1, write_z=1)
        full = collect_bf3(c, o2, 1, 1)
        z_from = dict(Zx=full["Zx"], Zy=full["Zy"])
        assert np.array_equal(full["S"].view(np.uint32), out["S"].view(np.uint32))
    inp.untouched()
    worst = ref.check_mask_forward(out, inp.S64, inp.X, inp.center, norm_split=True, delta=inp.delta, z_from=z_from, x_half=bool(c.write_x),
                                   sel=inp.sel.want, const_rows=inp.const_rows, lin_rows=inp.lin_rows)
    _report(capsys, _line(c, kernel, worst))
