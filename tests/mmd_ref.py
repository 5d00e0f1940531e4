"""TEST INFRASTRUCTURE ONLY: a dense float64 reference of the RBF/MMD Gram launch and of the backward product that consumes
its gradient weights, with first-order error bounds for the float32 kernels.  The product never imports this file.

What the Gram kernels compute per element (i, j) of the 2n x 2n matrix over Z = [X; Y]:

    g_ij = z_i . z_j                      L_ij = max(s_i + s_j - 2 g_ij, 0)         (s = the row norms the kernel is GIVEN)
    K_ij = sum_k exp(-L_ij / sc_k)        dK/dL = -sum_k exp(-L_ij / sc_k) / sc_k
    W_ij = sgn * 2/n^2 * dK/dL            sgn = +1 on XX and YY, -1 on XY and YX

with sc_k = float32(bw * mult_k).  Each tile of the table leaves sum(K) over its valid elements in partial[t, 0] (the
calibration launch: sum(L) in partial[t, 1]) and, under its flags, W directly (STORE) and transposed (MIRROR).

Error bounds (u = 2^-24, the unit roundoff of float32; all first order, none tuned)
-------------------------------------------------------------------------------
dg_ij = 2 * kterms * u * sum_k |z_ik z_jk|
    the order-independent bound kterms * u * sum |a_k b_k| of a float32 summation of kterms products, times the factor 2
    of margin test_chain_ksplit_gpu.py uses.  kterms = p for the fp32 kernel, 3 * kp for the split-bf16 kernels (three MFMA
    products per k, over the padded contraction); for those, sum_k |z_ik z_jk| is taken over |hi| + |lo|, which bounds
    |hi hi'| + |hi lo'| + |lo hi'|.  The dropped lo.lo' term is on both sides of the comparison (see dense_weights).
dL_ij = 2 dg_ij + 4u (s_i + s_j + 2 |g_ij|) + 4u L_ij
    (A DEVIATION from the form dL = 2 dg + 4u (s_i + s_j + 2 |g|) with the argument's scaling inside c: the last term, 4u L,
    takes the exponent argument's share out of the constant.  Reason below.)
    2 dg: g enters L doubled.  4u (...): the two float32 roundings of s_i + s_j - 2 g, each at most u times the largest
    intermediate, doubled for margin.  4u L: the exponent argument is L * c with c = -log2(e) / scale formed in float32 -- the
    constant (u), the scale (u), the division (u) and the product L * c (u) -- and a relative error e of the ARGUMENT is
    exactly a relative error e of L, whatever power of t it ends up in (the t^16 term sees it sixteen-fold, which is what
    |dw/dL| below already weighs).  Writing it as an error of L keeps it right for every L / bw, where a constant times |w|
    would hold only while L / (4 bw) stays below about 16.
dw_ij = |dw/dL| dL_ij + C_EPI u |w_ij|  (+ 2^-16 |w_ij| for a stored bf16 pair)
    |dw/dL| = 2/n^2 sum_k exp(-L / sc_k) / sc_k^2, in float64.  C_EPI = 64 covers what happens after the argument is formed:
    v_exp_f32 is good to 1 ulp = 2u on t; the squaring chain t -> t^2 -> t^4 -> t^8 -> t^16 doubles the relative error and
    adds one rounding per step, (2m + m - 1) u for t^m, so 47u at m = 16 and less for the others; the four additions of the
    positive terms (3u along the deepest path; the multiplications by 1/4, 1/2, 2, 4 are exact); the factor
    -sgn * 2 / (n^2 bw) (n^2 exact, one product, one division: 2u) and its product with the sum (u): 53u, rounded up to 64u.
    The general kernel (one exp per scale, fma with 1/scale) stays below that: 2u + 2u (1/scale) + u + 5u (sum) + 3u.
    2^-16 |w|: hi = bf16(w), lo = bf16(w - hi) keep 16 significant bits; the resolution the existing bf3 tests use.
dK_ij = |dK/dL| dL_ij + C_EPI u K_ij, |dK/dL| = sum_k exp(-L / sc_k) / sc_k, the same chain without the final factor.
tile sum: sum over the tile of dK_ij + m u sum |K_ij|, m = the tile's element count (float32 summation in any order).
    Calibration: the same with dL_ij and L_ij.
backward: out = 2 (rs_i z_ij - acc_ij) mul_ij, rs_i = sum_k W_ik, acc_ij = sum_k W_ik Z_kj over K columns:
    each float32 sum within K * 2^-23 * sum_k |a_k b_k| (check_product of test_chain_ksplit_gpu.py), carried through:
    2 K 2^-23 (sum_k |W_ik| |z_ij| + sum_k |W_ik Z_kj|) |mul_ij|, plus 8u (|rs_i z_ij| + |acc_ij|) |mul_ij| for the epilogue's
    four roundings (product, difference, mul + shift, final product), doubled.

split-bf16 backward (backward_bf3_ref / backward_bf3_bound): the kernels are GIVEN the four bf16 images Wh, Wl [nr, K] and
    Zh, Zl [K, p] and the fp32 row z the epilogue reads, and compute, in float32,
        acc_ij = sum_k (Wh_ik Zh_kj + Wh_ik Zl_kj + Wl_ik Zh_kj)     (three MFMA products per k; Wl.Zl is NOT formed)
        rs_i   = sum_k (Wh_ik + Wl_ik)                              (2 K terms)
        out_ij = 2 (rs_i z_ij - acc_ij) (mul_ij + shift_j)
    The reference is that expression in float64 on the same images (as gram_bf3 does for the Gram: the dropped term is on both
    sides).  Every product of two bf16 values is exact in float32, so only the summations round: a float32 sum of m terms t_k
    in ANY order is within m u sum |t_k| to first order, m 2^-23 sum |t_k| with the factor 2 of margin used throughout this file
    (check_product of test_chain_ksplit_gpu.py).  rs has m = 2 K terms |Wh| and |Wl|; acc has m = 3 K terms whose magnitudes
    sum to at most (|Wh| + |Wl|) . (|Zh| + |Zl|) (that also counts |Wl Zl|, 2^-16 of the total).  K is the PADDED length of the
    slab's K range, which is what the loops run over.  Carried through out = 2 (...) m:
        2 * 2^-23 * (2 K sum_k (|Wh| + |Wl|)_ik |z_ij|  +  3 K ((|Wh| + |Wl|) . (|Zh| + |Zl|))_ij) |mul_ij + shift_j|
        + 8u (|rs_i z_ij| + |acc_ij|) |mul_ij + shift_j|          (the epilogue's four roundings, doubled, as for `backward`)
    With the row sums handed in (rs_part: S slot cells per row, summed in float32) the first term is S sum_s |cell_s| |z| in
    place of 2 K sum_k (...).  With both hi images zero acc is exactly zero and the second term is left out (exact_acc).
    CAP_BWD_BF3: max(bound) <= 2e-3 max |want| for every case of the GPU tier (tests/test_mmd_bwd_bf3_cpu.py).

A vacuous bound hides errors: every case asserts max(bound) <= cap * max |W| (cap_ok) before it looks at a kernel's output.
"""
import functools

import numpy as np

from oracle import vgan_oracle as orc

TF_SLOT, TF_TWICE, TF_STORE, TF_MIRROR, TF_NEG = 3, 4, 8, 16, 32
U = 2.0 ** -24
C_EPI = 64.0
CAP_FP32, CAP_BF3 = 2e-4, 5e-4

# the case lists of the GPU tier; the CPU tier checks every bound and cap on them first
FP32_CASES = [(33, 4), (65, 7), (100, 20), (130, 33), (128, 32), (64, 64), (96, 200)]
FP32_MULTS = [(3, 3.0), (6, 1.5)]
# (192, 300) of the first list broke the cap (max(bound) = 5.5e-4 of max |W|) and became (192, 250).  (65, 40) and (128, 64) have
# kp = 64, the shortest contraction there is: ONE K tile of the 64- and 128-wide kernels (GemmBF3 / GemmBF3Big, BK = 64: the
# prologue's tile and no refill) and nk = 2 < NST = 3 stages of the 256-wide one.  Read before they were run: GemmBF3Wide::loader
# issues stages 1 and 2 only under nk > 1 and nk > 2, waits vmcnt(12) for stage 0 with one younger stage in flight and vmcnt(0)
# for stage 1 ahead of B(1); loaders and both consumer groups pass P + 2 nk + 1 barriers for every nk; GemmBF3Big::pingpong
# guards both refills (kt + 1 < nk, 1 < nk) and passes 2 nk + 1 barriers in both groups.
BF3_CASES = [(65, 96), (100, 130), (130, 200), (128, 65), (192, 250), (33, 70), (65, 40), (128, 64)]
SHARD_CASES = [(96, 3), (128, 2), (100, 4)]  # (n, world)
SHARD_P, SHARD_D = 20, 96  # features of the fp32 / split-bf16 operands of the sharded cases
BWD_CASES = [(65, 7), (100, 20), (96, 200)]


def tile_shape(tile):
    return (256, 128) if tile == 256 else (tile, tile)


def multipliers(nk, mf):
    """RBF(n_kernels, mul_factor): mul_factor ** (k - n_kernels // 2)."""
    return [float(mf) ** (k - nk // 2) for k in range(nk)]


def make_case(n, p, seed=0):
    """Standard-normal X, Y = X * U(0.2, 1), both float32; Z = [X; Y]; sq = the float32 row norms; bw = the calibrated
    bandwidth sum(L) / (N^2 - N) as a float32."""
    rng = np.random.default_rng(1000 * n + p + seed)
    X = rng.normal(size=(n, p)).astype(np.float32)
    Y = (X * rng.uniform(0.2, 1.0, size=(n, p))).astype(np.float32)
    Z = np.vstack([X, Y])
    z64 = Z.astype(np.float64)
    sq = (z64 * z64).sum(1).astype(np.float32)
    s = sq.astype(np.float64)
    L = np.maximum(s[:, None] + s[None, :] - 2.0 * z64 @ z64.T, 0.0)
    N = 2 * n
    bw = np.float32(L.sum() / (N * N - N))
    return Z, sq, bw


def split_bf16(x):
    """hi = bf16(x) (round to nearest even), lo = bf16(x - hi), as float32 arrays holding bf16 values."""
    import torch
    t = torch.as_tensor(np.ascontiguousarray(x, dtype=np.float32))
    hi = t.to(torch.bfloat16)
    lo = (t - hi.float()).to(torch.bfloat16)
    return hi.float().numpy(), lo.float().numpy()


def scales(bw, mults=None):
    if mults is None:
        return orc.rbf_scales(float(bw), np.float64)
    return (np.float32(float(bw)) * np.asarray(mults, dtype=np.float32)).astype(np.float64)


def gram_fp32(z64):
    return z64 @ z64.T


def gram_bf3(zh64, zl64):
    a = zh64 @ zl64.T
    return zh64 @ zh64.T + a + a.T


def dense_from_gram(g, sq64, n, bw, mults=None):
    s = np.asarray(sq64, dtype=np.float64)
    L = np.maximum(s[:, None] + s[None, :] - 2.0 * g, 0.0)
    K, dK = np.zeros_like(L), np.zeros_like(L)
    for sc in scales(bw, mults):
        e = np.exp(-L / sc)
        K += e
        dK -= e / sc
    sgn = np.ones_like(L)
    sgn[:n, n:] = -1.0
    sgn[n:, :n] = -1.0
    return L, K, sgn * 2.0 / (float(n) * n) * dK


def dense_weights(z64, sq64, n, bw, multipliers=None):
    """The full 2n x 2n float64 L, K and W.  z64: the float32 operand widened -- or a pair (zh64, zl64) of the split-bf16
    images, for which the Gram term is zh zh' + zh zl' + zl zh'.  sq64: the float32 row norms the kernel is given, widened."""
    g = gram_bf3(*z64) if isinstance(z64, tuple) else gram_fp32(z64)
    return dense_from_gram(g, sq64, n, bw, multipliers)


def tile_rows_cols(row, tile):
    T, TC = tile_shape(tile)
    r0, c0, rlim, clim = row[:4]
    return np.arange(r0, min(r0 + T, rlim)), np.arange(c0, min(c0 + TC, clim))


def tile_sums(table, K, tile):
    """Per-tile float64 sum of K over [r0, min(r0 + T, rlim)) x [c0, min(c0 + TC, clim))."""
    out = np.zeros(len(table))
    for t, row in enumerate(np.asarray(table).tolist()):
        ri, cj = tile_rows_cols(row, tile)
        out[t] = K[np.ix_(ri, cj)].sum()
    return out


def scatter(table, W, wrow0, nr, tile, with_clash=False):
    """The [nr, 2n] image the table's flags prescribe -- STORE: W[ri, cj] at [ri - wrow0, cj]; MIRROR: its transpose at
    [cj - wrow0, ri] -- and the boolean mask of the written elements.  with_clash: also the largest disagreement between two
    writes of one element."""
    N = W.shape[1]
    img = np.full((nr, N), np.nan)
    written = np.zeros((nr, N), dtype=bool)
    clash = 0.0

    def put(rows, cols, vals):
        nonlocal clash
        ix = np.ix_(rows, cols)
        both = written[ix]
        if both.any():
            clash = max(clash, float(np.abs(img[ix] - vals)[both].max()))
        img[ix] = vals
        written[ix] = True

    for row in np.asarray(table).tolist():
        fl = row[4]
        if not fl & TF_STORE:
            continue
        ri, cj = tile_rows_cols(row, tile)
        w = W[np.ix_(ri, cj)]
        put(ri - wrow0, cj, w)
        if fl & TF_MIRROR:
            put(cj - wrow0, ri, w.T)
    return (img, written, clash) if with_clash else (img, written)


def reduce_stats(table, part_k, part_l=None):
    """mmd_reduce in float64: block sums by slot, TWICE tiles doubled; [3] = sum of L over the full matrix (XY counted twice)."""
    st = np.zeros(4)
    for t, row in enumerate(np.asarray(table).tolist()):
        fl = row[4]
        w = 2.0 if fl & TF_TWICE else 1.0
        st[fl & TF_SLOT] += w * part_k[t]
        if part_l is not None:
            st[3] += (2.0 if (fl & TF_SLOT) == 1 else w) * part_l[t]
    return st


def _abs_gram(z64):
    if isinstance(z64, tuple):
        a = np.abs(z64[0]) + np.abs(z64[1])
    else:
        a = np.abs(z64)
    return a @ a.T


def l_bound(z64, sq64, L, kterms, arg_scale=True):
    """dL (module docstring); arg_scale=False leaves out the exponent argument's term (the calibration launch has no exponent)."""
    g = gram_bf3(*z64) if isinstance(z64, tuple) else gram_fp32(z64)
    s = np.asarray(sq64, dtype=np.float64)
    dg = 2.0 * kterms * U * _abs_gram(z64)
    return 2.0 * dg + 4.0 * U * (s[:, None] + s[None, :] + 2.0 * np.abs(g)) + (4.0 * U * L if arg_scale else 0.0)


def weight_bound(z64, sq64, n, bw, kterms, multipliers=None, pair=False):
    """dw, dense 2n x 2n (module docstring).  pair: the weights are stored as a bf16 hi/lo pair."""
    L, K, W = dense_weights(z64, sq64, n, bw, multipliers)
    dL = l_bound(z64, sq64, L, kterms)
    slope = sum(np.exp(-L / sc) / sc ** 2 for sc in scales(bw, multipliers)) * 2.0 / (float(n) * n)
    return slope * dL + (C_EPI * U + (2.0 ** -16 if pair else 0.0)) * np.abs(W)


def sum_bound(table, z64, sq64, n, bw, kterms, tile, multipliers=None, calibrate=False):
    """Per-tile bound of partial[t, 0] (calibrate: of partial[t, 1])."""
    L, K, _ = dense_weights(z64, sq64, n, bw if not calibrate else 1.0, multipliers)
    dL = l_bound(z64, sq64, L, kterms, arg_scale=not calibrate)
    if calibrate:
        per, mag = dL, L
    else:
        slope = sum(np.exp(-L / sc) / sc for sc in scales(bw, multipliers))
        per, mag = slope * dL + C_EPI * U * K, K
    out = np.zeros(len(table))
    for t, row in enumerate(np.asarray(table).tolist()):
        ri, cj = tile_rows_cols(row, tile)
        ix = np.ix_(ri, cj)
        out[t] = per[ix].sum() + ri.size * cj.size * U * np.abs(mag[ix]).sum()
    return out


def cap_ok(bound, W, cap):
    """The bound must mean something: max(bound) <= cap * max |W|.  Returns the ratio for the record."""
    ratio = float(np.max(bound) / np.abs(W).max())
    assert ratio <= cap, f"vacuous bound: max(bound) = {ratio:.3e} of max |W|, cap {cap:.1e} -- change the case"
    return ratio


def backward_ref(W64, z64, wrow0, nr, mul64=None):
    """2 (rowsum(W) z - W Z) * mul in float64 for W [nr, ncols], Z [ncols, p]."""
    r = 2.0 * (W64.sum(1, keepdims=True) * z64[wrow0:wrow0 + nr] - W64 @ z64)
    return r if mul64 is None else r * mul64


def backward_bound(W64, z64, wrow0, nr, kterms, mul64=None):
    """Module docstring, 'backward'."""
    aw, az = np.abs(W64), np.abs(z64)
    zr = az[wrow0:wrow0 + nr]
    m = 1.0 if mul64 is None else np.abs(mul64)
    acc, rs = aw @ az, aw.sum(1, keepdims=True)
    return (2.0 * kterms * 2.0 ** -23 * (rs * zr + acc) + 8.0 * U * (np.abs(W64.sum(1, keepdims=True)) * zr + np.abs(W64 @ z64))) * m


def emulate_gram_fp32(Z32, sq32, n, bw32, mults=None):
    """A float32 numpy emulation of mmd_gram_kernel's arithmetic (float32 matmul, float32 exp2 of the scaled argument, the
    squaring chain or one exp per scale): K and W as float32 2n x 2n."""
    f = np.float32
    g = Z32 @ Z32.T
    L = np.maximum((sq32[:, None] + sq32[None, :]) - f(2) * g, f(0)).astype(f)
    nn = f(n) * f(n)
    sgn = np.ones_like(L)
    sgn[:n, n:] = -1
    sgn[n:, :n] = -1
    if mults is None:
        c2 = f(-1.4426950408889634) / (f(4) * bw32)
        t = np.exp2(L * c2).astype(f)
        t2 = t * t
        t4 = t2 * t2
        t8 = t4 * t4
        t16 = t8 * t8
        K = ((t + t2) + (t4 + t8)) + t16
        W = (-sgn * f(2) / (nn * bw32)) * (((f(0.25) * t + f(0.5) * t2) + (t4 + f(2) * t8)) + f(4) * t16)
        return K.astype(f), W.astype(f)
    K, dk = np.zeros_like(L), np.zeros_like(L)
    for m in mults:
        sc = f(bw32 * f(m))
        e = np.exp2(L * (f(-1.4426950408889634) / sc)).astype(f)
        K = K + e
        dk = (e * (f(1) / sc) + dk).astype(f)
    return K.astype(f), ((-sgn * f(2) / nn) * dk).astype(f)


# ------------------------------------------------------------------------------------------------ split-bf16 backward product
CAP_BWD_BF3 = 2e-3
# (n, p) of tests/test_mmd_bwd_bf3_gpu.py, the smallest shapes that reach each schedule (N = 2n rows of Z, kn = N padded to 64):
# (32, 7) one K tile, p < 64, odd ldz; (33, 64) two K tiles, zrows 2 past a tile; (65, 65) three, one column into a second
# panel; (100, 130) kp = 192 < 256: the 128-wide kernel's clamp of feature rows; (65, 40) and (130, 130) ragged on 256 x 128
# tiles; (128, 130) nr = 128 and nr = 256 on them
BWD_BF3_CASES = [(32, 7), (33, 64), (65, 65), (100, 130), (130, 200), (65, 40), (130, 130), (128, 130)]
BWD_BF3_WIDE = [(65, 40), (130, 130), (128, 130)]  # tile 256 is forced here (row-major operand only)
BWD_BF3_MULS = ["none", "mul", "mul+shift"]
BWD_BF3_MUTATIONS = ["Wh.Zl dropped", "Wl.Zh dropped", "Wl.Zl added", "row sum over Wh only"]


# The kernels are handed raw images, so the test is free in them.  Most rows of W are a true split (hi = bf16(w), lo = bf16(w - hi),
# |lo| <= 2^-9 |hi|): there Wl.Zl is 2^-16 of the product against a bound of about K 2^-22 of it, and no element-wise bound can see
# that term added.  Three rows of every W are therefore SMALL (2^-20 of the others) with a lo image as large as the hi image: on
# them each of the three products, and the fourth that must not be formed, weighs as much as the whole, and an error there is
# far below any tolerance scaled by max |want| -- the wrong element in a small-magnitude row that a global criterion lets pass.
BWD_BF3_SMALL = 2.0 ** -20


def bwd_bf3_small_rows(nr):
    return [1, nr // 2, nr - 1]


def pad64(v):
    return (int(v) + 63) // 64 * 64


def bwd_bf3_ranges(n):
    """(nr, wrow0) as in test_fp32_backward_direct: the Y half, all rows, and from n = 64 on a shard."""
    return [(n, n), (2 * n, 0)] + ([(32, n + 32)] if n >= 64 else [])


def bwd_bf3_splits(n):
    """1, 2, 3 and 40 slabs (live < splits: empty slabs); kn = 256 also 4: klen = 64, two stages of the 256-wide loop."""
    return [1, 2, 3, 40] + ([4] if pad64(2 * n) == 256 else [])


def bf3_slabs(kn, splits):
    """kchunk, live and the [k0, k1) column ranges of the live slabs, as launch_backward_bf3 cuts them (whole K tiles of 64)."""
    kchunk = ((kn // 64 + splits - 1) // splits) * 64
    live = (kn + kchunk - 1) // kchunk
    return kchunk, live, [(s * kchunk, min((s + 1) * kchunk, kn)) for s in range(live)]


def bf16_bits(x):
    """The uint16 images of a float32 array that holds bf16 values."""
    b = np.ascontiguousarray(x, dtype=np.float32).view(np.uint32)
    assert not (b & 0xFFFF).any()
    return (b >> 16).astype(np.uint16)


def bf16_from_bits(b):
    return (np.asarray(b).view(np.uint16).astype(np.uint32) << 16).view(np.float32).astype(np.float64)


@functools.lru_cache(maxsize=None)
def bwd_bf3_data(n, p):
    """The operands of a case, read-only: fp32 Z [N, p]; its split images zh, zl [kn, p] as float64 (rows past N zero); per
    row range W's split images wh, wl [nr, kn] (columns past N zero), mul [nr, p] and shift [p] as float32."""
    rng = np.random.default_rng(10007 * n + p)
    N, kn = 2 * n, pad64(2 * n)
    Z = rng.normal(size=(N, p)).astype(np.float32)
    zh, zl = np.zeros((kn, p)), np.zeros((kn, p))
    zh[:N], zl[:N] = split_bf16(Z)
    ranges = []
    for nr, wrow0 in bwd_bf3_ranges(n):
        W = (rng.normal(size=(nr, N)) * 1e-3).astype(np.float32)
        wh, wl = np.zeros((nr, kn)), np.zeros((nr, kn))
        wh[:, :N], wl[:, :N] = split_bf16(W)
        for r in bwd_bf3_small_rows(nr):
            wh[r, :N] = split_bf16(rng.normal(size=N) * 1e-3 * BWD_BF3_SMALL)[0]
            wl[r, :N] = split_bf16(rng.normal(size=N) * 2e-3 * BWD_BF3_SMALL)[0]
        mul =rng.normal(size=(nr, p)).astype(np.float32)
        shift = rng.normal(size=(p,)).astype(np.float32)
        ranges.append(dict(nr=nr, wrow0=wrow0, wh=wh, wl=wl, mul=mul, shift=shift))
    for a in [Z, zh, zl] + [r[k] for r in ranges for k in ("wh", "wl", "mul", "shift")]:
        a.setflags(write=False)
    return dict(n=n, p=p, N=N, kn=kn, kp=pad64(p), Z=Z, zh=zh, zl=zl, ranges=ranges)


def bwd_bf3_mul64(rg, variant):
    """mul + shift in float64, or None."""
    if variant == "none":
        return None
    m = rg["mul"].astype(np.float64)
    return m + rg["shift"].astype(np.float64) if variant == "mul+shift" else m


def backward_bf3_ref(wh, wl, zh, zl, zrow, mul64=None, k0=0, k1=None, rs=None):
    """Module docstring, 'split-bf16 backward', over the columns [k0, k1) of W = rows of Z.  zrow: the fp32 rows of Z the
    epilogue reads, [nr, p] float64.  rs [nr]: row sums handed in (rs_part) instead of summed from the images."""
    k1 = wh.shape[1] if k1 is None else k1
    a, b, c, d = wh[:, k0:k1], wl[:, k0:k1], zh[k0:k1], zl[k0:k1]
    acc = a @ c + a @ d + b @ c
    r = (a + b).sum(1) if rs is None else np.asarray(rs, dtype=np.float64)
    out = 2.0 * (r[:, None] * zrow - acc)
    return out if mul64 is None else out * mul64


def backward_bf3_bound(wh, wl, zh, zl, zrow, mul64=None, k0=0, k1=None, rs_cells=None, exact_acc=False):
    """Module docstring, 'split-bf16 backward'.  K = k1 - k0, padded.  rs_cells [S, nr]: the slot cells the row sum is folded from."""
    k1 = wh.shape[1] if k1 is None else k1
    a, b, c, d = wh[:, k0:k1], wl[:, k0:k1], zh[k0:k1], zl[k0:k1]
    K = k1 - k0
    az = np.abs(zrow)
    aw = np.abs(a) + np.abs(b)
    acc = a @ c + a @ d + b @ c
    if rs_cells is None:
        rs, rs_term = (a + b).sum(1), 2.0 * K * aw.sum(1)
    else:
        cells = np.asarray(rs_cells, dtype=np.float64)
        rs, rs_term = cells.sum(0), cells.shape[0] * np.abs(cells).sum(0)
    prod_term = 0.0 if exact_acc else 3.0 * K * (aw @ (np.abs(c) + np.abs(d)))
    bound = 2.0 * 2.0 ** -23 * (rs_term[:, None] * az + prod_term) + 8.0 * U * (np.abs(rs)[:, None] * az + np.abs(acc))
    return bound if mul64 is None else bound * np.abs(mul64)


def emulate_backward_bf3(wh, wl, zh, zl, zrow, mul32=None, shift32=None, k0=0, k1=None, mutation=None):
    """A float32 numpy emulation of the kernels' arithmetic (float32 products and sums, the epilogue's four roundings), with
    one of BWD_BF3_MUTATIONS applied."""
    f = np.float32
    k1 = wh.shape[1] if k1 is None else k1
    a, b, c, d = (x.astype(f) for x in (wh[:, k0:k1], wl[:, k0:k1], zh[k0:k1], zl[k0:k1]))
    acc = np.zeros((a.shape[0], c.shape[1]), dtype=f)  # small terms first
    if mutation == "Wl.Zl added":
        acc = acc + b @ d
    if mutation != "Wl.Zh dropped":
        acc = acc + b @ c
    if mutation != "Wh.Zl dropped":
        acc = acc + a @ d
    acc = (acc + a @ c).astype(f)
    rs = (a.sum(1) if mutation == "row sum over Wh only" else (a + b).sum(1)).astype(f)
    out = f(2) * (rs[:, None] * zrow.astype(f) - acc)
    if mul32 is not None:
        out = out * (mul32 + shift32 if shift32 is not None else mul32)
    return out.astype(f)
