"""TEST INFRASTRUCTURE ONLY: the float64 reference of the dense fp32 products (vgan_linear_forward, vgan_linear_backward_input,
vgan_linear_backward_params, vgan_gemm_grouped), their per-element error bounds, the input generator and the case tables of
tests/test_gemm_kernels_gpu.py.  tests/test_gemm_kernels_cpu.py pins all of it without a GPU.  The product never imports this file.

Reference
---------
The float32 operands are taken exactly, as float64, and the plain product is formed: forward y = x W^T (+ the float32 bias),
backward input dx = dy W, backward params dW = dy^T x and db = the float64 column sums of dy, grouped NN / NT / TN likewise and
NT_NT = (A B^T) D^T.  An operand GIVEN as slabs (x_nslabs > 1) is first summed in float32 in ascending slab order (slab_sum32) --
that is what the contract of include/vgan_hip.h says the staging does, and numpy restates it bit for bit -- and only the sum
enters the float64 product.  Outputs WRITTEN as slabs (`splits` of vgan_linear_backward_params, `splitk` of a grouped problem)
are compared after summing: every case of these tables sums them on the host, in float32, in ascending slab order
(slab_sum32 again; vgan_reduce_slabs does the same on the device and has its own tests in test_small_ops_gpu.py).

Bounds (u = 2^-24, the unit roundoff of float32; per element, first order, order independent, nothing fitted to a device)
-----------------------------------------------------------------------------------------------------------------------------
product of K terms            K 2u sum_k |a_k b_k|
    a float32 sum of K products in ANY order (MFMA chain, waves, K tiles) is off by at most K u sum |a_k b_k| to first
    order: each term passes through at most K roundings (the fused multiply-add rounds once per term, every partial sum it
    then sits in rounds once more, at most K - 1 times), each relative to a partial sum that is at most sum |a_k b_k|.
    Factor 2: the project's own margin (check_product of tests/test_chain_ksplit_gpu.py).
forward with bias             (K + 1) 2u (sum_k |a_k b_k| + |b|)
    the bias is one more term and one more rounding.
slabs summed afterwards       (K + splits) 2u sum_k |a_k b_k|
    a term is rounded at most (rows of its slice) times inside its slab and at most `splits` times more while the slabs are
    added; no term passes through more roundings than K + splits.  db of a split launch is such a product too (b_k = 1).
slab-GIVEN operand            the product bound on the float32-summed operand
    the slab sum is restated bit-exactly (same order, same format), so it adds nothing.
db                            K 2u sum_k |dy_k|          (a product with b_k = 1)
NT_NT                         (k + k2) 2u (|A| |B|^T |D|^T)
    H = A B^T carries k u |A||B|^T per element (it is stored as float32: that rounding is one of the k), the second product
    adds k2 u |H||D|^T, and |H| <= |A||B|^T, so (k + k2) u |A||B|^T|D|^T covers both to first order; doubled as above.

Inputs that give the bounds teeth
---------------------------------
draw(): magnitudes uniform in [lo, 1], lo = 0.5 unless the case says otherwise, so every term a_k b_k is at least lo^2 in
magnitude.  teeth() asserts max(bound) < lo^2 for every case: one dropped, doubled or misplaced term moves an element by more
than its bound.  K^2 2^-23 mean|ab| < lo^2 stops holding with lo = 0.5 near K = 1400, so the K >= 2044 cases draw from [0.9, 1].
Signs: random ALONG THE CONTRACTION and shared by the two operands, alternating along the output index --
sign(a_ik) = (-1)^i t_k, sign(b_kj) = t_k (-1)^j with t random.  Both operands then look randomly signed to a kernel, but the K
terms of one output element all carry the sign (-1)^(i+j).  Independent random signs were the first draft and made the mutants
of test_gemm_kernels_cpu.py a matter of luck: the four terms of a K tail, or the rows of a split slice, cancel below the bound in
some element of some case (fwd 64 x 68 x 65 did).  With agreeing signs ANY set of m dropped or doubled terms moves the element
by at least m lo^2, a row or column taken from its neighbour flips the sign of every term (>= 2 K lo^2), and nothing is left
to chance; the error bound itself does not care about signs.  The bias alternates too, b_j = (-1)^j |b_j|, so the bias of the
neighbouring column is off by >= 2 lo.  For NT_NT, H = A B^T inherits the structure (every |h| >= k lo^2), so a term h d of the
second product is at least k lo^3: teeth() is given that floor for those problems.  db is a column sum over the randomly signed
index, so only its single-term mutant is certain; the others are asserted where they hold by construction (n = 1 slices).
cap_ok() asserts max(bound) <= CAP max|want|, the guard of mmd_ref.py against a vacuous bound.  CAP = 2e-2: the bound grows like
K^2 2^-23 mean|ab| and the largest elements of a K-term sum of random signs like 3 sqrt(K) rms|ab|, so their ratio is about
K^1.5 2^-23 / 3 -- 4e-3 at K = 2048, the longest contraction of the tables -- and the one-element outputs, whose only value
may sit well below its rms, get a factor 5 on top.  (With per-element teeth the cap is the lesser check; it stays for symmetry.)

Tables
------
Every row names the path code (include/vgan_hip.h) it expects on the "aligned" layout; on "shifted" (every view starts one
float into its allocation) and "oddld" (leading dimensions = 1 mod 4) the scalar counterpart SCALAR_OF[code] is expected.
test_gemm_kernels_cpu.py asks the library's own path queries about every row and fails on a row whose code differs and on a
code no row reaches.  Changes against the first draft of the tables:
  * wide-grid rule of vgan_linear_backward_params, (out, in) = (385, 384): the 16-wave kernel stages both operands with
    output-contiguous float4, so it needs out % 4 == 0.  The pair n = 2048 / 2044 runs at (388, 384) -- still 42 tiles of
    64 x 64 -- and (385, 384) at n = 2048 stays as the scalar 4-wave case of the same rule.
"""
import types
import zlib

import numpy as np

U = 2.0 ** -24
CAP = 2e-2
VARIANTS = ["aligned", "shifted", "oddld"]
FAKE_BASE = 0x40000000  # the CPU tier's fake addresses: only nullness and alignment are looked at

SCALAR_OF = {"T64_V4": "T64_V1", "T64_V1": "T64_V1", "T64_V4_SLABS": "T64_V1_SLABS", "T64_V1_SLABS": "T64_V1_SLABS",
             "KS4_V4": "KS4_V1", "KS4_V1": "KS4_V1", "KS16_V4": "KS4_V1",
             "T256_V4": "T256_V1", "T256_V1": "T256_V1", "T256_V4_EPI": "T256_V1_EPI", "T256_V1_EPI": "T256_V1_EPI", "KS16": "T256_V1"}


def round4(v):
    return (v + 3) // 4 * 4


def engine_of(code):
    """The tile engine and stager family of a path code: codes that differ only in the vector width share it."""
    return code.replace("_V4", "").replace("_V1", "")


def vec_of(code):
    return 1 if "_V1" in code else 4


def expected(code, variant):
    return code if variant == "aligned" else SCALAR_OF[code]


def ld_for(cols, variant, extra=4):
    """a leading dimension > cols: a multiple of 4 unless the variant is "oddld" (then = 1 mod 4)"""
    return round4(cols) + extra + (1 if variant == "oddld" else 0)


def shift_for(variant):
    return 1 if variant == "shifted" else 0


def slab_stride_for(rows, ld, odd=False):
    """slabs of a [rows, ld] image: a multiple of 4 floats apart with a gap, or (odd) = 1 mod 4"""
    return round4(rows * ld) + 8 + (1 if odd else 0)


def fake(index, variant):
    """a fake operand address with the alignment the variant gives a real one"""
    return FAKE_BASE + 0x100000 * index + 4 * shift_for(variant)


def rng_for(name):
    return np.random.default_rng(zlib.crc32(name.encode()))


def alt(n):
    return (-1.0) ** np.arange(n)


def signs(rng, n):
    return rng.choice([-1.0, 1.0], size=n)


def draw(rng, shape, lo=0.5, rows=None, cols=None):
    """float32 magnitudes uniform in [lo, 1]; the sign of element (i, j) is rows[i] * cols[j] (see the module docstring)"""
    v = rng.uniform(lo, 1.0, size=shape)
    if rows is not None:
        v = v * np.asarray(rows)[:, None]
    if cols is not None:
        v = v * np.asarray(cols)[None, :]
    return v.astype(np.float32)


def draw_bias(rng, n, lo=0.5):
    return (rng.uniform(lo, 1.0, size=n) * alt(n)).astype(np.float32)


def draw_slabs(rng, shape, nslabs, lo=0.5, rows=None, cols=None):
    """nslabs float32 slabs whose float32 ascending sum has magnitudes in [lo, 1] (to an ulp): random fractions of one draw"""
    x = draw(rng, shape, lo, rows, cols)
    if nslabs == 1:
        return x[None]
    parts, rest = [], x.copy()
    for _ in range(nslabs - 1):
        p = (x * rng.uniform(0.2, 0.4, size=shape).astype(np.float32)).astype(np.float32)
        parts.append(p)
        rest = (rest - p).astype(np.float32)
    return np.stack(parts + [rest])


def slab_sum32(slabs):
    """float32 sum of slabs[0], slabs[1], ... in that order"""
    acc = np.asarray(slabs[0], dtype=np.float32).copy()
    for s in slabs[1:]:
        acc = (acc + np.asarray(s, dtype=np.float32)).astype(np.float32)
    return acc


def split_rows(n, splits):
    """Row slices of vgan_linear_backward_params: ceil(n / splits) rows rounded up to a multiple of 4; trailing slices may be
    empty (n = 5, splits = 3: 4, 1 and 0 rows)."""
    kchunk = round4(-(-n // splits))
    return [(min(s * kchunk, n), min((s + 1) * kchunk, n)) for s in range(splits)]


def splitk_slices(k, splitk):
    """K slices of a grouped problem: ceil(k / splitk) rounded up to the 32-deep K tile; None where a slice would be empty
    (the library refuses those)."""
    kchunk = (-(-k // splitk) + 31) // 32 * 32
    if (splitk - 1) * kchunk >= k:
        return None
    return [(s * kchunk, min((s + 1) * kchunk, k)) for s in range(splitk)]


# ---- bounds ----------------------------------------------------------------------------------------------------------------
def product_bound(a64, b64, roundings):
    """roundings * 2u * (|a| |b|), a64 [M, K], b64 [K, N]"""
    return roundings * 2.0 * U * (np.abs(a64) @ np.abs(b64))


def teeth(bound, lo, floor=None):
    """max(bound) < the smallest magnitude a term can have (lo^2 unless given)"""
    floor = lo * lo if floor is None else floor
    worst = float(np.max(bound))
    assert worst < floor, f"toothless bound: max(bound) = {worst:.3e} >= smallest term {floor:.3e} -- change the case"
    return worst / floor


def cap_ok(bound, want, cap=CAP):
    ratio = float(np.max(bound) / np.abs(want).max())
    assert ratio <= cap, f"vacuous bound: max(bound) = {ratio:.3e} of max |want|, cap {cap:.1e} -- change the case"
    return ratio


def worst_ratio(got, want, bound):
    """max err / bound, after asserting err <= bound element-wise"""
    err = np.abs(np.asarray(got, dtype=np.float64) - want)
    ratio = float((err / np.maximum(bound, 1e-300)).max())
    assert (err <= bound).all(), f"worst err / bound = {ratio:.3f} at {np.unravel_index(np.argmax(err / np.maximum(bound, 1e-300)), err.shape)}"
    return ratio


# ---- cases ------------------------------------------------------------------------------------------------------------------
class Case(types.SimpleNamespace):
    def __repr__(self):
        return self.name


def _name(prefix, dims, **flags):
    return prefix + "-" + "x".join(str(d) for d in dims) + "".join(f"-{k}{'' if v is True else v}" for k, v in flags.items() if v not in (None, False))


def fwd(n, kin, out, path, bias=True, nslabs=1, slab_odd=False, lo=0.5):
    return Case(family="fwd", n=n, kin=kin, out=out, path=path, bias=bias, nslabs=nslabs, slab_odd=slab_odd, lo=lo, ktile=32 if path.startswith("T64") else 128,
                name=_name("fwd", (n, kin, out), nobias=not bias, xs=nslabs if nslabs > 1 else None, odd=slab_odd))


def bwi(n, kin, out, path, tight_ldw=False, lo=0.5):
    return Case(family="bwi", n=n, kin=kin, out=out, path=path, tight_ldw=tight_ldw, lo=lo, ktile=32 if path.startswith("T64") else 128,
                name=_name("bwi", (n, kin, out), tight=tight_ldw))


def bwp(out, kin, n, path, db=True, splits=1, nslabs=1, slab_odd=False, lo=0.5):
    return Case(family="bwp", n=n, kin=kin, out=out, path=path, db=db, splits=splits, nslabs=nslabs, slab_odd=slab_odd, lo=lo,
                ktile=32 if path.startswith("T64") else 128,
                name=_name("bwp", (out, kin, n), nodb=not db, sp=splits if splits > 1 else None, xs=nslabs if nslabs > 1 else None, odd=slab_odd))


# (rows, cols, K) of the 64 x 64 engine: output edges (1, 1) (5, 3) (63, 64) (64, 65) (65, 63) (130, 4) and K edges 1 3 4 31 32 33 36
# 64 65 68 96 97 100 (one to four K tiles; multiples of 4 for the vector path), K >= 128 at (385, 384) = 42 tiles; of the 32 x 32
# engine: output edges (1, 1) (31, 33) (32, 32) (33, 31) (65, 5) (300, 36) and K edges 128 129 130 132 252 256 260 388 508 512 516 1028;
# the dispatch neighbours K 127 / 128 and 32 / 36 tiles.  Written per family, because which of them are vector cases differs:
# forward needs K % 4 == 0, backward input K and cols, backward params rows and cols (its K, the batch, is free).
FWD_CASES = [  # fwd(n, in, out, path): rows = n, cols = out, K = in
    fwd(1, 1, 1, "T64_V1"), fwd(5, 3, 3, "T64_V1"), fwd(63, 4, 64, "T64_V4"), fwd(64, 31, 65, "T64_V1"), fwd(65, 32, 63, "T64_V4"),
    fwd(130, 33, 4, "T64_V1"), fwd(1, 36, 1, "T64_V4"), fwd(5, 64, 3, "T64_V4"), fwd(63, 65, 64, "T64_V1"), fwd(64, 68, 65, "T64_V4"),
    fwd(65, 96, 63, "T64_V4"), fwd(130, 97, 4, "T64_V1"), fwd(64, 100, 64, "T64_V4"), fwd(65, 32, 63, "T64_V4", bias=False),
    fwd(385, 128, 384, "T64_V4"), fwd(385, 129, 384, "T64_V1"), fwd(385, 132, 384, "T64_V4"),
    fwd(65, 127, 5, "T64_V1"), fwd(65, 128, 5, "KS4_V4"), fwd(512, 128, 256, "KS4_V4"), fwd(513, 128, 256, "T64_V4"),
    fwd(1, 128, 1, "KS4_V4"), fwd(31, 129, 33, "KS4_V1"), fwd(32, 130, 32, "KS4_V1"), fwd(33, 132, 31, "KS4_V4"),
    fwd(33, 132, 31, "KS4_V4", bias=False), fwd(65, 252, 5, "KS4_V4"), fwd(300, 256, 36, "KS4_V4"), fwd(32, 260, 32, "KS4_V4"),
    fwd(33, 388, 31, "KS4_V4"), fwd(300, 508, 36, "KS4_V4"), fwd(300, 512, 36, "KS16_V4"), fwd(300, 512, 36, "KS16_V4", bias=False),
    fwd(65, 516, 5, "KS16_V4"), fwd(31, 1028, 33, "KS16_V4"),
    # slab-given x: always the 64 x 64 engine, whatever K
    fwd(65, 36, 63, "T64_V4_SLABS", nslabs=2), fwd(64, 68, 65, "T64_V4_SLABS", nslabs=3), fwd(5, 33, 3, "T64_V1_SLABS", nslabs=2),
    fwd(130, 97, 4, "T64_V1_SLABS", nslabs=3), fwd(65, 36, 63, "T64_V1_SLABS", nslabs=2, slab_odd=True),
    fwd(33, 132, 31, "T64_V4_SLABS", nslabs=2, bias=False),
]

BWI_CASES = [  # bwi(n, in, out, path): rows = n, cols = in, K = out
    bwi(1, 1, 1, "T64_V1"), bwi(5, 3, 3, "T64_V1"), bwi(63, 64, 4, "T64_V4"), bwi(64, 65, 31, "T64_V1"), bwi(65, 63, 32, "T64_V1"),
    bwi(130, 4, 33, "T64_V1"), bwi(1, 1, 36, "T64_V1"), bwi(5, 4, 64, "T64_V4"), bwi(63, 64, 65, "T64_V1"), bwi(64, 68, 68, "T64_V4"),
    bwi(65, 64, 96, "T64_V4"), bwi(130, 4, 97, "T64_V1"), bwi(64, 64, 100, "T64_V4"), bwi(130, 4, 36, "T64_V4"),
    bwi(385, 384, 128, "T64_V4"), bwi(385, 384, 129, "T64_V1"), bwi(385, 384, 132, "T64_V4"),
    bwi(65, 5, 127, "T64_V1"),
    bwi(65, 5, 128, "KS4_V4"),                  # ragged `in` on the vector tall-skinny kernel: ldw >= round4(in), W's pad columns are read
    bwi(65, 5, 128, "KS4_V1", tight_ldw=True),  # the same shape with ldw == in: the scalar tall-skinny kernel
    bwi(512, 256, 128, "KS4_V4"), bwi(513, 256, 128, "T64_V4"),
    bwi(1, 1, 128, "KS4_V4"), bwi(31, 33, 129, "KS4_V1"), bwi(32, 32, 130, "KS4_V1"), bwi(33, 31, 132, "KS4_V4"), bwi(65, 5, 252, "KS4_V4"),
    bwi(300, 36, 256, "KS4_V4"), bwi(32, 32, 260, "KS4_V4"), bwi(33, 31, 388, "KS4_V4"), bwi(300, 36, 508, "KS4_V4"),
    bwi(300, 36, 512, "KS4_V4"), bwi(65, 5, 516, "KS4_V4"), bwi(31, 33, 1028, "KS4_V4"),
]

BWP_CASES = [  # bwp(out, in, n, path): rows = out, cols = in, K = n
    bwp(1, 1, 1, "T64_V1"), bwp(5, 3, 3, "T64_V1"), bwp(63, 64, 4, "T64_V1"), bwp(64, 65, 31, "T64_V1"), bwp(65, 63, 32, "T64_V1"),
    bwp(130, 4, 33, "T64_V1"), bwp(4, 4, 36, "T64_V4"), bwp(8, 4, 64, "T64_V4"), bwp(64, 64, 65, "T64_V4"), bwp(64, 68, 68, "T64_V4"),
    bwp(68, 64, 96, "T64_V4"), bwp(132, 4, 97, "T64_V4"), bwp(64, 64, 100, "T64_V4"), bwp(63, 64, 33, "T64_V1"),
    bwp(385, 384, 128, "T64_V1"), bwp(388, 384, 129, "T64_V4"), bwp(388, 384, 132, "T64_V4"),
    bwp(36, 32, 300, "T64_V4"),  # db given: the 64 x 64 kernel whatever the contraction (10 K tiles)
    bwp(68, 64, 96, "T64_V4", db=False), bwp(65, 63, 33, "T64_V1", db=False),
    # the three tall-skinny kernels (db NULL, splits 1, no slabs)
    bwp(68, 4, 127, "T64_V4", db=False), bwp(68, 4, 128, "KS4_V4", db=False),
    bwp(1, 1, 128, "KS4_V1", db=False), bwp(32, 32, 128, "KS4_V4", db=False), bwp(31, 33, 129, "KS4_V1", db=False),
    bwp(32, 32, 130, "KS4_V4", db=False), bwp(36, 32, 132, "KS4_V4", db=False), bwp(33, 31, 132, "KS4_V1", db=False),
    bwp(68, 4, 252, "KS4_V4", db=False), bwp(65, 5, 252, "KS4_V1", db=False), bwp(300, 36, 252, "KS4_V4", db=False),
    bwp(300, 36, 256, "KS16_V4", db=False), bwp(32, 32, 260, "KS16_V4", db=False), bwp(36, 32, 388, "KS16_V4", db=False),
    bwp(300, 36, 508, "KS16_V4", db=False), bwp(300, 36, 512, "KS16_V4", db=False), bwp(68, 8, 516, "KS16_V4", db=False),
    bwp(32, 36, 1028, "KS16_V4", db=False), bwp(31, 33, 1028, "KS4_V1", db=False),
    bwp(512, 256, 128, "KS4_V4", db=False), bwp(516, 256, 128, "T64_V4", db=False),
    # the wide-grid rule (at most 512 tiles and n >= 2048): see the module docstring for (388, 384)
    bwp(388, 384, 2048, "KS16_V4", db=False, lo=0.9), bwp(388, 384, 2044, "T64_V4", db=False, lo=0.9),
    bwp(385, 384, 2048, "KS4_V1", db=False, lo=0.9),
    # row slices: 36 + 36 + 28; 6 x 16 + 1 + one empty; 4 + 1 + one empty; 4 + 4 + six empty
    bwp(68, 64, 100, "T64_V4", splits=3), bwp(68, 64, 100, "T64_V4", splits=3, db=False), bwp(65, 63, 97, "T64_V1", splits=8),
    bwp(5, 3, 5, "T64_V1", splits=3), bwp(8, 4, 8, "T64_V4", splits=8),
    # slab-given x
    bwp(68, 64, 36, "T64_V4_SLABS", nslabs=2), bwp(65, 63, 33, "T64_V1_SLABS", nslabs=2), bwp(68, 64, 100, "T64_V4_SLABS", nslabs=2, splits=3),
    bwp(68, 64, 36, "T64_V1_SLABS", nslabs=2, slab_odd=True), bwp(36, 32, 300, "T64_V4_SLABS", nslabs=2, db=False),
]


def gp(kind, m, n, k, splitk=1, k2=0):
    return Case(kind=kind, m=m, n=n, k=k, splitk=splitk, k2=k2, name=f"{kind}{m}x{n}x{k}" + (f"s{splitk}" if splitk > 1 else "") + (f"h{k2}" if k2 else ""))


def grp(problems, path, engines, scalar_engines=None, epi=False, lo=0.5):
    """engines: per problem on the aligned layout; scalar_engines: on the other two (default: KS16 becomes KS4)"""
    scalar_engines = [("KS4" if e == "KS16" else e) for e in engines] if scalar_engines is None else scalar_engines
    return Case(family="grp", problems=problems, path=path, engines=engines, scalar_engines=scalar_engines, epi=epi, lo=lo,
                name="grp-" + "+".join(p.name for p in problems) + ("-epi" if epi else ""))


KINDS = ["NN", "NT", "TN"]
# one problem per launch, every kind: (m, n, k, path, engine[, scalar engine])
_SINGLE = [(1, 1, 1, "T256_V1", "T64"), (65, 63, 33, "T256_V1", "T64"), (64, 65, 31, "T256_V1", "T64"), (130, 4, 97, "T256_V1", "T64"),
           (4, 4, 4, "T256_V4", "T64"), (68, 64, 36, "T256_V4", "T64"), (64, 68, 68, "T256_V4", "T64"),
           (64, 64, 92, "T256_V4", "T64"), (64, 64, 96, "KS16", "KS16", "T64"),  # kmin 92 / 96; K = 96 is ONE partial 128-deep K tile
           (33, 31, 129, "T256_V1", "KS4"), (31, 33, 1028, "T256_V1", "KS4"),
           (32, 32, 128, "KS16", "KS16"), (36, 32, 132, "KS16", "KS16"), (300, 36, 256, "KS16", "KS16"), (32, 36, 1028, "KS16", "KS16"),
           (68, 4, 516, "KS16", "KS16")]
GRP_SINGLE = [grp([gp(kind, m, n, k)], path, [eng[0]], [eng[-1]] if len(eng) > 1 else None) for kind in KINDS for (m, n, k, path, *eng) in _SINGLE]
# launch thresholds: 256 tiles of 32 x 32 in all (16-wave launch) against 272; 512 per problem (4-wave tiles) against 528
GRP_SINGLE += [grp([gp("NN", 512, 512, 128)], "KS16", ["KS16"]), grp([gp("NN", 516, 512, 128)], "T256_V4", ["KS4"]),
               grp([gp("NT", 512, 1024, 128)], "T256_V4", ["KS4"]), grp([gp("TN", 512, 1028, 128)], "T256_V4", ["T64"])]

GRP_FOUR = [
    # problem boundaries in the 1-D grid: a first problem of one tile, a last one with ragged tiles
    grp([gp("NN", 4, 4, 36), gp("NT", 68, 64, 36), gp("TN", 64, 68, 68), gp("NN", 132, 68, 36)], "T256_V4", ["T64"] * 4),
    # a 64 x 64 problem beside 4-wave ones (k = 4 keeps the launch off the 16-wave kernel)
    grp([gp("NN", 68, 64, 36), gp("NT", 36, 32, 132), gp("TN", 36, 32, 256), gp("NN", 4, 4, 4)], "T256_V4", ["T64", "KS4", "KS4", "T64"]),
    grp([gp("NN", 32, 32, 128), gp("NT", 36, 32, 132), gp("TN", 300, 36, 256), gp("NN", 68, 4, 516)], "KS16", ["KS16"] * 4),
    grp([gp("NN", 1, 1, 1), gp("NT", 65, 63, 33), gp("TN", 33, 31, 129), gp("NN", 31, 33, 130)], "T256_V1", ["T64", "T64", "KS4", "KS4"]),
    grp([gp("TN", 4, 4, 4), gp("TN", 33, 31, 129), gp("NT", 130, 4, 97), gp("NT", 300, 36, 256)], "T256_V1", ["T64", "KS4", "T64", "KS4"]),
]

# splitk with a ragged last slice (100 = 64 + 36; 132 = 64 + 64 + 4; 133 = 64 + 64 + 5), alone and beside an unsplit problem
GRP_SPLITK = [grp([gp("NN", 68, 64, 100, splitk=2)], "T256_V4", ["T64"]), grp([gp("NT", 68, 64, 132, splitk=3)], "T256_V4", ["T64"]),
              grp([gp("TN", 65, 63, 133, splitk=3)], "T256_V1", ["T64"]), grp([gp("TN", 68, 64, 132, splitk=3), gp("NN", 64, 68, 68)], "T256_V4", ["T64", "T64"]),
              grp([gp("NN", 36, 32, 260, splitk=2), gp("NT", 36, 32, 132)], "T256_V4", ["T64", "KS4"])]
GRP_SPLITK_REFUSED = [gp("NN", 68, 64, 100, splitk=3), gp("TN", 68, 64, 64, splitk=3)]  # a slice would be empty: VGAN_ERR_ARG

# NT_NT: k2 1 4 63 64 65 132, m and n no multiples of 64, beside an ordinary product; k2 % 4 == 0 is the vector path
GRP_NTNT = [grp([gp("NT2", 68, 132, 36, k2=k2), gp("NN", 64, 68, 68)], "T256_V4" if k2 % 4 == 0 else "T256_V1", ["T64", "T64"]) for k2 in (1, 4, 63, 64, 65, 132)]
GRP_NTNT += [grp([gp("NT2", 65, 130, 33, k2=65)], "T256_V1", ["T64"]), grp([gp("NT2", 68, 132, 132, k2=64)], "T256_V4", ["T64"])]

# the optimiser epilogue's instantiations: only the product they write is checked here (the update has its own tests)
GRP_EPI = [grp([gp("NN", 8, 8, 36)], "T256_V4_EPI", ["T64"], epi=True), grp([gp("TN", 36, 32, 132)], "T256_V4_EPI", ["KS4"], epi=True)]

GRP_CASES = GRP_SINGLE + GRP_FOUR + GRP_SPLITK + GRP_NTNT + GRP_EPI


# ---- data, reference and bound of a case --------------------------------------------------------------------------------------
def fwd_data(c):
    rng = rng_for(c.name)
    t = signs(rng, c.kin)
    xs = draw_slabs(rng, (c.n, c.kin), c.nslabs, c.lo, alt(c.n), t)
    W = draw(rng, (c.out, c.kin), c.lo, alt(c.out), t)
    b = draw_bias(rng, c.out, c.lo) if c.bias else None
    x64, w64 = slab_sum32(xs).astype(np.float64), W.astype(np.float64)
    want = x64 @ w64.T
    mag = np.abs(x64) @ np.abs(w64).T
    if b is not None:
        want = want + b.astype(np.float64)
        mag = mag + np.abs(b.astype(np.float64))
    return Case(xs=xs, W=W, b=b, A=x64, B=w64.T, want=want, bound=(c.kin + (1 if c.bias else 0)) * 2.0 * U * mag)


def bwi_data(c):
    rng = rng_for(c.name)
    t = signs(rng, c.out)
    dy, W = draw(rng, (c.n, c.out), c.lo, alt(c.n), t), draw(rng, (c.out, c.kin), c.lo, t, alt(c.kin))
    a, b = dy.astype(np.float64), W.astype(np.float64)
    return Case(dy=dy, W=W, A=a, B=b, want=a @ b, bound=product_bound(a, b, c.out))


def bwp_data(c):
    rng = rng_for(c.name)
    t = signs(rng, c.n)
    dy = draw(rng, (c.n, c.out), c.lo, t, alt(c.out))
    xs = draw_slabs(rng, (c.n, c.kin), c.nslabs, c.lo, t, alt(c.kin))
    a, b = dy.astype(np.float64).T, slab_sum32(xs).astype(np.float64)
    r = c.n + (c.splits if c.splits > 1 else 0)
    return Case(dy=dy, xs=xs, A=a, B=b, want=a @ b, bound=product_bound(a, b, r), want_db=a.sum(1), bound_db=r * 2.0 * U * np.abs(a).sum(1))


def grp_problem_data(p, lo, seed):
    """A, B (, D) as the kind stores them, the product form A64 [m, K] . B64 [K, n] of the (last) product, want, bound and the
    smallest magnitude one of its terms can have."""
    rng = rng_for(f"{seed}/{p.name}")
    two = p.kind == "NT2"
    t, u = signs(rng, p.k), signs(rng, max(p.k2, 1))
    A = draw(rng, (p.k, p.m), lo, t, alt(p.m)) if p.kind == "TN" else draw(rng, (p.m, p.k), lo, alt(p.m), t)
    if two:
        B = draw(rng, (p.k2, p.k), lo, u, t)
    else:
        B = draw(rng, (p.n, p.k), lo, alt(p.n), t) if p.kind == "NT" else draw(rng, (p.k, p.n), lo, t, alt(p.n))
    a = A.astype(np.float64).T if p.kind == "TN" else A.astype(np.float64)
    b = B.astype(np.float64).T if p.kind in ("NT", "NT2") else B.astype(np.float64)
    if not two:
        r = p.k + (p.splitk if p.splitk > 1 else 0)
        return Case(A=A, B=B, D=None, a=a, b=b, want=a @ b, bound=product_bound(a, b, r), floor=lo * lo, K=p.k)
    D = draw(rng, (p.n, p.k2), lo, alt(p.n), u)
    h, d = a @ b, D.astype(np.float64).T
    return Case(A=A, B=B, D=D, a=h, b=d, want=h @ d, bound=(p.k + p.k2) * 2.0 * U * (np.abs(a) @ np.abs(b) @ np.abs(d)), floor=p.k * lo ** 3, K=p.k2)


def grp_data(c):
    return [grp_problem_data(p, c.lo, c.name) for p in c.problems]


# ---- the path queries on fake (CPU tier) or real (GPU tier) addresses ---------------------------------------------------------
def fwd_layout(c, variant):
    ldx = ld_for(c.kin, variant)
    return Case(ldx=ldx, ldw=ld_for(c.kin, variant, 8), ldy=ld_for(c.out, variant), shift=shift_for(variant),
                xs=slab_stride_for(c.n, ldx, c.slab_odd) if c.nslabs > 1 else 0)


def fwd_path(lib, c, variant, addr=None):
    L = fwd_layout(c, variant)
    x, W, b, y = addr or [fake(i, variant) for i in range(4)]
    return lib.vgan_linear_forward_path(x, L.ldx, c.nslabs, L.xs, W, L.ldw, b if c.bias else None, y, L.ldy, c.n, c.kin, c.out)


def bwi_layout(c, variant):
    return Case(lddy=ld_for(c.out, variant), ldw=c.kin if c.tight_ldw else ld_for(c.kin, variant), lddx=ld_for(c.kin, variant, 8), shift=shift_for(variant))


def bwi_path(lib, c, variant, addr=None):
    L = bwi_layout(c, variant)
    dy, W, dx = addr or [fake(i, variant) for i in range(3)]
    return lib.vgan_linear_backward_input_path(dy, L.lddy, W, L.ldw, dx, L.lddx, c.n, c.kin, c.out)


def bwp_layout(c, variant):
    ldx, lddw = ld_for(c.kin, variant), ld_for(c.kin, variant, 8)
    return Case(lddy=ld_for(c.out, variant), ldx=ldx, lddw=lddw, shift=shift_for(variant),
                xs=slab_stride_for(c.n, ldx, c.slab_odd) if c.nslabs > 1 else 0,
                slab=slab_stride_for(c.out, lddw) if c.splits > 1 else 0)


def bwp_path(lib, c, variant, addr=None):
    L = bwp_layout(c, variant)
    dy, x, dW, db = addr or [fake(i, variant) for i in range(4)]
    return lib.vgan_linear_backward_params_path(dy, L.lddy, x, L.ldx, c.nslabs, L.xs, dW, L.lddw, db if c.db else None, c.n, c.kin, c.out,
                                                c.splits, L.slab)


def grp_shapes(p):
    """stored shapes of A, B, C (, D) of a problem"""
    a = (p.k, p.m) if p.kind == "TN" else (p.m, p.k)
    b = (p.k2, p.k) if p.kind == "NT2" else (p.n, p.k) if p.kind == "NT" else (p.k, p.n)
    return a, b, (p.m, p.n), ((p.n, p.k2) if p.kind == "NT2" else None)


def grp_fake_problems(lib_mod, c, variant):
    """ctypes problem array of a group on fake addresses; C of a splitk problem is contiguous, as the binding requires"""
    arr = (lib_mod.GemmProblem * len(c.problems))()
    code = {"NN": lib_mod.GEMM_NN, "NT": lib_mod.GEMM_NT, "TN": lib_mod.GEMM_TN, "NT2": lib_mod.GEMM_NT_NT}
    for i, (q, p) in enumerate(zip(arr, c.problems)):
        sa, sb, sc, sd = grp_shapes(p)
        q.a, q.b, q.c = fake(8 * i, variant), fake(8 * i + 1, variant), fake(8 * i + 2, variant)
        q.kind, q.m, q.n, q.k, q.splitk = code[p.kind], p.m, p.n, p.k, p.splitk
        q.lda, q.ldb, q.ldc = ld_for(sa[1], variant), ld_for(sb[1], variant), (p.n if p.splitk > 1 else ld_for(p.n, variant))
        if sd is not None:
            q.d, q.scratch, q.ldd, q.k2 = fake(8 * i + 3, variant), fake(8 * i + 4, "aligned"), ld_for(sd[1], variant), p.k2
    return arr


def grp_fake_extras(lib_mod, c):
    """extras of an optimiser-epilogue case on fake addresses: layer i = the leading [m, n - 1 | 1] of problem i"""
    x = lib_mod.GroupedExtras()
    x.adadelta, x.p, x.sq_avg, x.acc_delta = 1, fake(40, "aligned"), fake(41, "aligned"), fake(42, "aligned")
    x.lr, x.rho, x.eps, x.grad_scale = 1.0, 0.9, 1e-6, 1.0
    off = 0
    for L, p in zip(x.layer, c.problems):
        L.w_packed, L.off_w, L.off_b, L.ldp, L.out, L.inp = fake(43, "aligned"), off, off + p.m * (p.n - 1), p.n, p.m, p.n - 1
        off += p.m * p.n
    return x


def grp_path(lib_mod, c, variant):
    """(code, engines) the library names for a group on fake addresses"""
    import ctypes
    lib = lib_mod.load()
    arr = grp_fake_problems(lib_mod, c, variant)
    engine = (ctypes.c_int32 * len(c.problems))()
    x = ctypes.byref(grp_fake_extras(lib_mod, c)) if c.epi else None
    return lib.vgan_gemm_grouped_path(arr, len(c.problems), x, None, engine), list(engine)
