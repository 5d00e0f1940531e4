"""GPU tier for the dense fp32-MFMA products -- vgan_linear_forward, vgan_linear_backward_input, vgan_linear_backward_params
(csrc/linear.hip) and vgan_gemm_grouped (csrc/grouped.hip), i.e. GemmTile (64 x 64 x 32) and GemmTileKS (32 x 32, K tile 128 split
over 4 or 16 waves) of csrc/gemm_core.hpp -- each called DIRECTLY through vgan_amd.ops.HipOps at the tile, K-tile and dispatch
edges of tests/gemm_ref.py and compared, element by element, with the float64 reference and the derived bounds of that file
(which tests/test_gemm_kernels_cpu.py pins without a GPU).  Run with ``-m gpu`` on an MI355X.

Conventions (those of test_small_ops_gpu.py)
  * Sentinels.  Every output lives in a NaN-filled allocation with a guard band on both sides (class Guarded); after every
    launch everything the contract owns is written and nothing else changed -- the guards, the columns [width, ld) of every
    row, the gap between slabs and one spare slab beyond the count.  Every input's pads and guards hold NaN too, so a read past a
    row or past the matrix poisons the result, and every input is compared with its image from before the launch.
    One documented exception: vgan_linear_backward_input on its vector tall-skinny kernel with a ragged `in` reads W's columns
    [in, round4(in)) -- NaN here as well.  A NaN in column j of W can only reach column j of dx, and those columns are computed
    and not stored, so the stored columns must still be finite and within the bound (case bwi-65x5x128).
  * Layouts.  "aligned", "shifted" (every view starts one float into its allocation) and "oddld" (leading dimensions = 1 mod 4);
    the last two are legal ABI inputs and run the VEC = 1 instantiations.
  * Slabs the kernels WRITE (`splits`, `splitk`) are summed on the host in float32 in ascending order before the comparison;
    each slab is also held to the bound of its own slice, and the slab of an empty slice must be all zeros (db included).

Per case: the result is within the per-element bound; a second launch gives the same bits; variants that run the same engine
(codes that differ in the vector width only: same LDS image, same MFMA chain) are bit-equal, the scalar ones among themselves
included; different engines (64 x 64, 4-wave, 16-wave) sum in different orders and are held to the bound only; a grouped problem
launched alone is bit-equal to the same problem inside a group of four wherever the query says its engine and vector width
are unchanged; and after each call the library's path query for those very arguments names the kernel the table expects.

One pair is NOT bit-equal by construction and is held to the bound instead: db of vgan_linear_backward_params between the vector
and the scalar layout.  db is the side sum of the MC stager (gemm_core.hpp), not an MFMA chain: Stager<.., MC, 4> keeps float4
partial sums per thread, folds its NV registers and then adds NTH / 16 = 16 LDS rows per column, Stager<.., MC, 1> adds NTH / 64 = 4
rows of per-thread sums that each cover four times as many contraction rows -- two different summation trees.  dW is bit-equal.

Measured worst err / bound per family (one full run on an MI355X; records, not bars): forward 0.201, backward input 0.245,
backward params dW 0.442 and db 0.169, grouped NN 0.313, NT 0.212, TN 0.154, NT_NT 0.061.  Every bit-equality above held on
the device as stated, the vector against the scalar layout of dW and of every forward, backward-input and grouped product
included; the 204 tests of the file take about three seconds.
"""
import collections

import numpy as np
import pytest
import torch

import gemm_ref as ref
from vgan_amd import lib as vlib

pytestmark = pytest.mark.gpu

GUARD = 64  # floats of guard band on either side of every allocation (keeps the 16-byte alignment)
WORST = collections.defaultdict(float)


@pytest.fixture(scope="module")
def ops():
    from vgan_amd.ops import HipOps
    return HipOps()


def host(t):
    return t.detach().cpu().numpy()


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


class Guarded:
    """nslabs [rows, cols] views with row stride ld, slab_stride floats apart, inside a NaN-filled allocation
    [guard | shift | slab 0 | gap | slab 1 ... | spare slabs | guard]."""

    def __init__(self, rows, cols, ld=None, shift=0, nslabs=1, slab_stride=0, spare=0, data=None):
        ld = cols if ld is None else ld
        assert ld >= cols and (nslabs + spare == 1 or slab_stride >= rows * ld)
        self.rows, self.cols, self.ld, self.nslabs, self.start = rows, cols, ld, nslabs, GUARD + shift
        self.slab_stride = slab_stride if nslabs + spare > 1 else 0
        body = (nslabs + spare - 1) * self.slab_stride + rows * ld
        self.buf = torch.full((self.start + body + GUARD,), float("nan"), dtype=torch.float32, device="cuda")
        self.t = self.view(0)
        assert self.t.data_ptr() % 16 == (4 * shift) % 16
        if data is not None:
            data = np.asarray(data, dtype=np.float32).reshape(nslabs, rows, cols)
            for s in range(nslabs):
                self.view(s).copy_(torch.as_tensor(data[s]).cuda())
        self.before = host(self.buf).copy()

    def view(self, s):
        return self.buf.as_strided((self.rows, self.cols), (self.ld, 1), self.start + s * self.slab_stride)

    @property
    def vec(self):
        """the 1-D view of a one-row allocation"""
        assert self.rows == 1
        return self.buf[self.start:self.start + self.cols]

    def cube(self):
        """the contiguous [nslabs, rows, cols] view (ld == cols, slabs back to back)"""
        assert self.ld == self.cols and self.slab_stride == self.rows * self.cols
        return self.buf.as_strided((self.nslabs, self.rows, self.cols), (self.slab_stride, self.cols, 1), self.start)

    def reset(self):
        self.buf.copy_(torch.as_tensor(self.before).cuda())

    def check(self, written=True):
        """Host copy [nslabs, rows, cols] of what the contract owns, after asserting that every other element still holds what it
        held before the call; written: the owned region holds no NaN."""
        h = host(self.buf)
        m = np.zeros(h.size, dtype=bool)
        for s in range(self.nslabs):
            for r in range(self.rows):
                o = self.start + s * self.slab_stride + r * self.ld
                m[o:o + self.cols] = True
        assert np.array_equal(h[~m].view(np.uint8), self.before[~m].view(np.uint8)), "write outside the contracted region"
        out = h[m].reshape(self.nslabs, self.rows, self.cols)
        if written:
            assert not np.isnan(out).any(), "contracted region not fully written"
        return out

    def untouched(self):
        assert np.array_equal(host(self.buf).view(np.uint8), self.before.view(np.uint8)), "buffer was written"


def twice(launch, outputs, inputs):
    """Run the launch twice from the same sentinel state: same bits, inputs untouched.  Returns the checked outputs."""
    launch()
    torch.cuda.synchronize()
    first = [o.check(written=w) for o, w in outputs]
    for i in inputs:
        i.untouched()
    for o, _ in outputs:
        o.reset()
    launch()
    torch.cuda.synchronize()
    for (o, w), f in zip(outputs, first):
        if w:
            assert np.array_equal(bits(o.check()), bits(f)), "a second launch gave other bits"
    return first


def record(family, name, variant, ratio):
    WORST[family] = max(WORST[family], ratio)
    print(f"{name} [{variant}] worst err / bound {ratio:.3f}")


def same_engine_bit_equal(results, what="result"):
    """results: {variant: (code, array)}: variants whose codes share an engine hold the same bits"""
    by_engine = collections.defaultdict(list)
    for variant, (code, arr) in results.items():
        by_engine[ref.engine_of(code)].append((variant, arr))
    for engine, group in by_engine.items():
        for variant, arr in group[1:]:
            assert np.array_equal(bits(arr), bits(group[0][1])), f"{what}: {group[0][0]} and {variant} differ on engine {engine}"


# ---- vgan_linear_forward --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", ref.FWD_CASES, ids=repr)
def test_linear_forward(ops, c):
    d = ref.fwd_data(c)
    results = {}
    for variant in ref.VARIANTS:
        L = ref.fwd_layout(c, variant)
        x = Guarded(c.n, c.kin, L.ldx, L.shift, nslabs=c.nslabs, slab_stride=L.xs, data=d.xs)
        W = Guarded(c.out, c.kin, L.ldw, L.shift, data=d.W)
        b = Guarded(1, c.out, shift=L.shift, data=d.b) if c.bias else None
        y = Guarded(c.n, c.out, L.ldy, L.shift)
        bv = b.vec if c.bias else None
        (got,) = twice(lambda: ops.linear_forward(x.t, W.t, bv, y.t, x_nslabs=c.nslabs, x_slab_stride=L.xs), [(y, True)],
                       [x, W] + ([b] if c.bias else []))
        record("forward", c.name, variant, ref.worst_ratio(got[0], d.want, d.bound))
        code = ops.linear_forward_path(x.t, W.t, bv, y.t, x_nslabs=c.nslabs, x_slab_stride=L.xs)
        assert code == ref.expected(c.path, variant), (variant, code)
        assert code == vlib.LINEAR_FORWARD_PATHS[ref.fwd_path(ops.lib, c, variant)]  # the fake addresses of the CPU tier agree
        results[variant] = (code, got[0])
    same_engine_bit_equal(results)


# ---- vgan_linear_backward_input -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", ref.BWI_CASES, ids=repr)
def test_linear_backward_input(ops, c):
    d = ref.bwi_data(c)
    results = {}
    for variant in ref.VARIANTS:
        L = ref.bwi_layout(c, variant)
        dy = Guarded(c.n, c.out, L.lddy, L.shift, data=d.dy)
        W = Guarded(c.out, c.kin, L.ldw, L.shift, data=d.W)  # columns [in, ldw) hold NaN: see the module docstring
        dx = Guarded(c.n, c.kin, L.lddx, L.shift)
        (got,) = twice(lambda: ops.linear_backward_input(dy.t, W.t, dx.t), [(dx, True)], [dy, W])
        record("backward_input", c.name, variant, ref.worst_ratio(got[0], d.want, d.bound))
        code = ops.linear_backward_input_path(dy.t, W.t, dx.t)
        assert code == ref.expected(c.path, variant), (variant, code)
        assert code == vlib.LINEAR_BACKWARD_INPUT_PATHS[ref.bwi_path(ops.lib, c, variant)]
        results[variant] = (code, got[0])
    same_engine_bit_equal(results)


# ---- vgan_linear_backward_params ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", ref.BWP_CASES, ids=repr)
def test_linear_backward_params(ops, c):
    d = ref.bwp_data(c)
    slices = ref.split_rows(c.n, c.splits)
    results, results_db = {}, {}
    for variant in ref.VARIANTS:
        L = ref.bwp_layout(c, variant)
        spare = 1 if c.splits > 1 else 0
        dy = Guarded(c.n, c.out, L.lddy, L.shift, data=d.dy)
        x = Guarded(c.n, c.kin, L.ldx, L.shift, nslabs=c.nslabs, slab_stride=L.xs, data=d.xs)
        dW = Guarded(c.out, c.kin, L.lddw, L.shift, nslabs=c.splits, slab_stride=L.slab, spare=spare)
        db = Guarded(1, c.out, shift=L.shift, nslabs=c.splits, slab_stride=L.slab, spare=spare) if c.db else None
        dbv = db.vec if c.db else None
        kw = dict(splits=c.splits, slab_stride=L.slab, x_nslabs=c.nslabs, x_slab_stride=L.xs)
        got = twice(lambda: ops.linear_backward_params(dy.t, x.t, dW.t, dbv, **kw), [(dW, True)] + ([(db, True)] if c.db else []), [dy, x])
        for s, (k0, k1) in enumerate(slices if c.splits > 1 else []):
            a, b = d.A[:, k0:k1], d.B[k0:k1]
            if k1 == k0:  # an empty slice: its slab is all zeros
                assert not got[0][s].any() and (not c.db or not got[1][s].any()), f"slab {s} of an empty slice is not zero"
                continue
            ref.worst_ratio(got[0][s], a @ b, ref.product_bound(a, b, k1 - k0))
            if c.db:
                ref.worst_ratio(got[1][s, 0], a.sum(1), (k1 - k0) * 2.0 * ref.U * np.abs(a).sum(1))
        dw_sum = ref.slab_sum32(got[0])  # float32, ascending slab order, on the host
        record("backward_params dW", c.name, variant, ref.worst_ratio(dw_sum, d.want, d.bound))
        code = ops.linear_backward_params_path(dy.t, x.t, dW.t, dbv, **kw)
        assert code == ref.expected(c.path, variant), (variant, code)
        assert code == vlib.LINEAR_BACKWARD_PARAMS_PATHS[ref.bwp_path(ops.lib, c, variant)]
        results[variant] = (code, got[0])
        if c.db:
            db_sum = ref.slab_sum32(got[1])[0]
            record("backward_params db", c.name, variant, ref.worst_ratio(db_sum, d.want_db, d.bound_db))
            results_db[variant] = (code, got[1])  # grouped by the full code: the side sum differs between V4 and V1 (module docstring)
    same_engine_bit_equal(results, "dW")
    by_code = collections.defaultdict(list)
    for variant, (code, arr) in results_db.items():
        by_code[code].append(arr)
    for arrs in by_code.values():
        assert all(np.array_equal(bits(a), bits(arrs[0])) for a in arrs[1:]), "db differs between layouts of one kernel"


# ---- vgan_gemm_grouped ----------------------------------------------------------------------------------------------------------
class Problem:
    """One grouped problem on the device: guarded operands, the tuple ops.gemm_grouped takes, and its check."""

    def __init__(self, p, q, variant):
        self.p, self.q = p, q
        sh, ld = ref.shift_for(variant), lambda cols: ref.ld_for(cols, variant)
        sa, sb, sc, sd = ref.grp_shapes(p)
        self.A = Guarded(sa[0], sa[1], ld(sa[1]), sh, data=q.A)
        self.B = Guarded(sb[0], sb[1], ld(sb[1]), sh, data=q.B)
        self.inputs = [self.A, self.B]
        if p.splitk > 1:  # slabs of C, m * ldc apart; the binding takes them as one contiguous [splitk, m, n] tensor
            self.C = Guarded(p.m, p.n, p.n, sh, nslabs=p.splitk, slab_stride=p.m * p.n, spare=1)
            self.arg = (p.kind, self.A.t, self.B.t, self.C.cube(), p.splitk)
        else:
            self.C = Guarded(p.m, p.n, ld(p.n), sh)
            self.arg = (p.kind, self.A.t, self.B.t, self.C.t)
        self.outputs = [(self.C, True)]
        if p.kind == "NT2":
            self.D = Guarded(sd[0], sd[1], ld(sd[1]), sh, data=q.D)
            tiles = -(-p.m // 64) * -(-p.n // 64)
            self.scratch = Guarded(1, tiles * 64 * ref.round4(p.k2))  # NaN before the launch; owned by it, contents unspecified
            self.inputs.append(self.D)
            self.outputs.append((self.scratch, False))
            self.arg = ("NT2", self.A.t, self.B.t, self.C.t, self.D.t, self.scratch.vec)

    def verify(self, slabs):
        """slabs [splitk, m, n] as checked by Guarded: each slab against its own K slice, their float32 sum against the bound"""
        p, q = self.p, self.q
        if p.splitk > 1:
            for s, (k0, k1) in enumerate(ref.splitk_slices(p.k, p.splitk)):
                a, b = q.a[:, k0:k1], q.b[k0:k1]
                ref.worst_ratio(slabs[s], a @ b, ref.product_bound(a, b, k1 - k0))
        return ref.worst_ratio(ref.slab_sum32(slabs), q.want, q.bound)


def run_group(ops, specs, data, variant, name, epi=False):
    """Launch the problems `specs` (with their data) as one group, twice; every product within its bound.
    Returns (launch code, [engine per problem], [C slabs per problem])."""
    probs = [Problem(p, q, variant) for p, q in zip(specs, data)]
    args = [pr.arg for pr in probs]
    extra = {}
    state = []
    if epi:  # layer i = the leading [m, n - 1 | 1] of problem i; only the product written to C is checked here
        total = sum(p.m * p.n for p in specs)
        rng = np.random.default_rng(3)
        state = [torch.as_tensor(rng.uniform(-1, 1, total).astype(np.float32)).cuda(), torch.zeros(total, device="cuda"), torch.zeros(total, device="cuda")]
        layers, off = [], 0
        for p in specs:
            layers.append((torch.zeros(p.m, p.n, device="cuda"), off, off + p.m * (p.n - 1), p.m, p.n - 1))
            off += p.m * p.n
        extra = dict(adadelta=dict(p=state[0], sq=state[1], acc=state[2], lr=1.0, layers=layers))
    outputs = [o for pr in probs for o in pr.outputs]
    got = twice(lambda: ops.gemm_grouped(args, **extra), outputs, [i for pr in probs for i in pr.inputs])
    assert all(bool(torch.isfinite(t).all()) for t in state)
    code, engines = ops.gemm_grouped_path(args, **extra)
    cs, it = [], iter(got)
    for pr in probs:
        c = next(it)
        for _ in pr.outputs[1:]:
            next(it)
        record("grouped " + ("NT_NT" if pr.p.kind == "NT2" else pr.p.kind), f"{name}:{pr.p.name}", variant, pr.verify(c))
        cs.append(c)
    return code, engines, cs


def vec_width(code):
    return 4 if code.startswith("KS16") else ref.vec_of(code)


@pytest.mark.parametrize("c", ref.GRP_SINGLE + ref.GRP_SPLITK + ref.GRP_NTNT + ref.GRP_EPI, ids=repr)
def test_gemm_grouped(ops, c):
    data = ref.grp_data(c)
    results = collections.defaultdict(dict)
    for variant in ref.VARIANTS:
        code, engines, cs = run_group(ops, c.problems, data, variant, c.name, epi=c.epi)
        assert code == ref.expected(c.path, variant), (variant, code)
        assert engines == (c.engines if variant == "aligned" else c.scalar_engines), (variant, engines)
        fake_code, fake_engines = ref.grp_path(vlib, c, variant)  # the fake addresses of the CPU tier agree
        assert vlib.GEMM_GROUPED_PATHS[fake_code] == code and [vlib.GEMM_ENGINES[e] for e in fake_engines] == engines
        for i, (e, arr) in enumerate(zip(engines, cs)):
            results[i][variant] = (e, arr)  # same tile engine, whatever the vector width: same bits
    for i, res in results.items():
        same_engine_bit_equal(res, f"problem {i}")


@pytest.mark.parametrize("c", ref.GRP_FOUR, ids=repr)
def test_gemm_grouped_of_four_equals_the_problems_alone(ops, c):
    data = ref.grp_data(c)
    compared = 0
    for variant in ref.VARIANTS:
        code, engines, cs = run_group(ops, c.problems, data, variant, c.name)
        assert code == ref.expected(c.path, variant), (variant, code)
        assert engines == (c.engines if variant == "aligned" else c.scalar_engines), (variant, engines)
        for i, p in enumerate(c.problems):
            code1, engines1, cs1 = run_group(ops, [p], [data[i]], variant, c.name + "/alone")
            if engines1[0] == engines[i] and vec_width(code1) == vec_width(code):
                assert np.array_equal(bits(cs1[0]), bits(cs[i])), f"{p.name} [{variant}]: alone and in the group differ on {engines[i]}"
                compared += 1
    assert compared >= 4  # the comparison is not vacuous for any group of the table


@pytest.mark.parametrize("p", ref.GRP_SPLITK_REFUSED, ids=repr)
def test_gemm_grouped_refuses_an_empty_k_slice(ops, p):
    (q,) = ref.grp_data(ref.grp([p], "T256_V4", ["T64"]))
    pr = Problem(p, q, "aligned")
    with pytest.raises(vlib.VganHipError):
        ops.gemm_grouped([pr.arg])
    with pytest.raises(vlib.VganHipError):
        ops.gemm_grouped_path([pr.arg])
    torch.cuda.synchronize()
    pr.C.untouched()


def test_record_of_the_worst_ratios():
    """Prints what this run measured (the figures of the module docstring come from such a run)."""
    for family in sorted(WORST):
        print(f"worst err / bound, {family}: {WORST[family]:.3f}")
    assert all(v <= 1.0 for v in WORST.values())
