"""TEST INFRASTRUCTURE ONLY: plain numpy restatements of the small kernels of the training step (csrc/rows.hip,
optim.hip, feed.hip, twosample.hip, row_sqnorm / col_mean of mmd.hip), written from include/vgan_hip.h and the formulas
in the kernels' header comments.  Nothing here calls the library: tests/test_small_ops_cpu.py pins these functions
(known answers, torch, the host entry point of the shuffle) and tests/test_small_ops_gpu.py holds the device to them.
"""
import numpy as np

M32 = np.uint64(0xFFFFFFFF)

#: the edge shapes of the GPU file (batch rows, feature widths)
N_EDGES = [1, 3, 4, 5, 63, 64, 65, 130, 1024]
WIDTHS = [1, 3, 4, 63, 64, 65, 252, 256, 260, 784, 1024, 1028, 2048, 4096, 4100, 1500]
_U = np.uint64


# ---------------------------------------------------------------------------------------------- Philox / noise
PHILOX_M0, PHILOX_M1 = _U(0xD2511F53), _U(0xCD9E8D57)
PHILOX_W0, PHILOX_W1 = _U(0x9E3779B9), _U(0xBB67AE85)


def philox4x32_10(counter_words, k0, k1):
    """Philox4x32-10 (Salmon et al., SC'11).  counter_words: four uint64 arrays (or scalars) holding 32-bit words;
    k0, k1: the key words.  Returns the four output words as uint64 arrays masked to 32 bits."""
    c0, c1, c2, c3 = (np.asarray(w, dtype=np.uint64) & M32 for w in counter_words)
    k0, k1 = _U(int(k0) & 0xFFFFFFFF), _U(int(k1) & 0xFFFFFFFF)
    for _ in range(10):
        p0, p1 = PHILOX_M0 * c0, PHILOX_M1 * c2           # 32 x 32 -> 64 bit products: no overflow in uint64
        c0, c1, c2, c3 = (p1 >> _U(32)) ^ c1 ^ k0, p1 & M32, (p0 >> _U(32)) ^ c3 ^ k1, p0 & M32
        k0, k1 = (k0 + PHILOX_W0) & M32, (k1 + PHILOX_W1) & M32
    return c0, c1, c2, c3


def u01(x):
    """(float32(x >> 8) + 0.5) * 2^-24 evaluated in float32, as the kernel does.  The sum is exact below 2^23 and rounds
    to even above it, so the largest word gives exactly 1.0 (r = 0): restated, not idealised."""
    k = (np.asarray(x, dtype=np.uint64) >> _U(8)).astype(np.float32)
    return (k + np.float32(0.5)) * np.float32(2.0 ** -24)


def noise_words(nq, seed, step, stream_id):
    """The four Philox words of the quads 0 .. nq-1 of the (seed, step, stream_id) stream: [4, nq] uint64."""
    seed, step, stream_id = int(seed) & (2 ** 64 - 1), int(step) & (2 ** 64 - 1), int(stream_id) & (2 ** 64 - 1)
    q = np.arange(nq, dtype=np.uint64)
    k0 = (seed & 0xFFFFFFFF) ^ (stream_id & 0xFFFFFFFF)
    k1 = (seed >> 32) ^ (stream_id >> 32) ^ 0x5bd1e995
    ctr = (q & M32, q >> _U(32), np.full(nq, step & 0xFFFFFFFF, dtype=np.uint64), np.full(nq, step >> 32, dtype=np.uint64))
    return np.stack(philox4x32_10(ctr, k0, k1))


TWO_PI_F32 = np.float32(6.283185307179586)


def noise_normal_ref(rows, cols, seed, step, stream_id):
    """vgan_noise_normal in float64: returns (z [rows, cols], r [rows, cols]) with r the Box-Muller radius behind every
    element.  Only the angle keeps its one float32 rounding (float32(2 pi) * u), because a rounding of the angle is
    amplified by r; everything else is float64."""
    count = rows * cols
    nq = (count + 3) // 4
    u = u01(noise_words(nq, seed, step, stream_id))                       # [4, nq] float32
    out = np.empty((nq, 4))
    rad = np.empty((nq, 4))
    for h in range(2):
        r = np.sqrt(-2.0 * np.log(u[2 * h].astype(np.float64)))
        theta = (TWO_PI_F32 * u[2 * h + 1]).astype(np.float64)            # float32 product, then exact
        out[:, 2 * h], out[:, 2 * h + 1] = r * np.cos(theta), r * np.sin(theta)
        rad[:, 2 * h] = rad[:, 2 * h + 1] = r
    return out.reshape(-1)[:count].reshape(rows, cols), rad.reshape(-1)[:count].reshape(rows, cols)


def noise_normal_f32_chain(nq, seed, step, stream_id):
    """The same chain evaluated op for op in numpy float32 (logf, sqrtf, sinf, cosf, the two products): what a float32
    implementation with correctly-behaved libm gives.  Flat [4 nq]."""
    u = u01(noise_words(nq, seed, step, stream_id))
    out = np.empty((nq, 4), dtype=np.float32)
    for h in range(2):
        r = np.sqrt(np.float32(-2.0) * np.log(u[2 * h]))
        theta = TWO_PI_F32 * u[2 * h + 1]
        out[:, 2 * h], out[:, 2 * h + 1] = r * np.cos(theta), r * np.sin(theta)
    assert out.dtype == np.float32
    return out.reshape(-1)


# ---------------------------------------------------------------------------------------------- shuffle
def feistel_half_bits(N):
    w = 1
    while w < 32 and (1 << (2 * w)) < N:
        w += 1
    return w


def _feistel_mix(x, k):
    """x, k: uint64 arrays holding 32-bit words; every product is reduced mod 2^32."""
    x = (x ^ k) & M32
    x = (x * _U(0x9E3779B1)) & M32
    x ^= x >> _U(15)
    x = (x * _U(0x85EBCA77)) & M32
    x ^= x >> _U(13)
    x = (x * _U(0xC2B2AE3D)) & M32
    x ^= x >> _U(16)
    return x


def feistel_perm_ref(i, N, seed, epoch):
    """perm[i] of vgan_shuffle_epoch / vgan_shuffle_index: a balanced Feistel network of 2w bits (w = feistel_half_bits(N)),
    8 rounds with the keyed mixer above, cycle-walked until the value is below N.  i: array of indices < N."""
    N, seed, epoch = int(N), int(seed) & (2 ** 64 - 1), int(epoch) & (2 ** 64 - 1)
    w = feistel_half_bits(N)
    mask = _U((1 << w) - 1) if w < 32 else M32
    k0 = _U((seed & 0xFFFFFFFF) ^ 0xA511E9B3)
    k1 = _U((seed >> 32) ^ (epoch & 0xFFFFFFFF))
    k2 = _U((epoch >> 32) ^ 0x63D83595)
    v = np.array(i, dtype=np.uint64).reshape(-1)
    todo = np.ones(v.shape, dtype=bool)
    while todo.any():
        x = v[todo]
        l, r = (x >> _U(w)) & mask, x & mask
        for q in range(8):
            rk = _feistel_mix(np.full(1, (int(k0) + 0x9E3779B9 * q) & 0xFFFFFFFF, dtype=np.uint64), k1) ^ k2
            f = _feistel_mix(r, rk) & mask
            l, r = r, l ^ f
        v[todo] = (l << _U(w)) | r
        todo = v >= _U(N)
    return v.astype(np.int64).reshape(np.shape(i))


# ---------------------------------------------------------------------------------------------- bf16 split
_T8 = 2.0 ** -8
#: probes of the split: exact round-to-even ties of hi in both directions (1 + 2^-8 goes down to 1, 1 + 3 2^-8 up to
#: 1 + 2^-6), values whose lo is itself a tie (index 7, 8, 9) or a near-tie, signed zeros and ordinary values
SPLIT_TIES = [1 + _T8, 1 + 3 * _T8, 1 + 5 * _T8, -(1 + _T8), -(1 + 3 * _T8), 2 + 2 * _T8, 2 + 6 * _T8,
              1 + _T8 / 2 * (1 + _T8), 1 + _T8 / 2 * (1 + 3 * _T8), -(1 + _T8 / 4 * (1 + _T8)), 1 + _T8 / 2 + _T8 * _T8,
              0.0, -0.0, 1.0, -1.0, 0.1, -0.3, 3.14159274, 65504.0, 1 - 2.0 ** -24, 1 + 2.0 ** -23]


def _bf16_rne_bits(x32):
    b = np.ascontiguousarray(x32, dtype=np.float32).view(np.uint32).astype(np.uint64)
    return (((b + _U(0x7FFF) + ((b >> _U(16)) & _U(1))) >> _U(16)) & _U(0xFFFF)).astype(np.uint16)


def bf16_value(bits):
    return (np.asarray(bits, dtype=np.uint16).astype(np.uint32) << np.uint32(16)).view(np.float32)


def split_bf16_ref(x32):
    """z = hi + lo with hi = bf16(z), lo = bf16(z - hi): integer round-to-nearest-even on the float32 bit pattern, the
    difference taken in float32.  Returns (hi_bits, lo_bits) as uint16.  (No NaN / denormal handling: not asserted.)"""
    x32 = np.ascontiguousarray(x32, dtype=np.float32)
    hi = _bf16_rne_bits(x32)
    lo = _bf16_rne_bits(x32 - bf16_value(hi))
    return hi, lo


def split_value_ref(x32):
    hi, lo = split_bf16_ref(x32)
    return bf16_value(hi) + bf16_value(lo)       # float32 sum (exact: both are multiples of ulp(x) below 2|x|)


# ---------------------------------------------------------------------------------------------- mask / column keys
def softmax64(logits):
    x = np.asarray(logits, dtype=np.float64)
    e = np.exp(x - x.max(axis=1, keepdims=True))
    return e / e.sum(axis=1, keepdims=True)


def upper_mask_ref(S32):
    S32 = np.asarray(S32, dtype=np.float32)
    return np.where(S32 < np.float32(1.0 / S32.shape[1]), S32, np.float32(1.0)).astype(np.float32)


def colkey_pack_ref(U, row_offset):
    """every element's key: (bits(u) << 32) | (0xFFFFFFFF - row)"""
    U = np.ascontiguousarray(U, dtype=np.float32)
    rows = (int(row_offset) + np.arange(U.shape[0], dtype=np.uint64))[:, None]
    return (U.view(np.uint32).astype(np.uint64) << _U(32)) | (M32 - rows)


def colkey_ref(U, row_offset):
    """the column maximum of the keys: the largest u wins, the LOWEST row among equals"""
    return colkey_pack_ref(U, row_offset).max(axis=0)


def colkey_rows(keys):
    return (M32 - (np.asarray(keys, dtype=np.uint64) & M32)).astype(np.int64)


def mask_backward_ref(g_slabs, S32, colkey, pen_weight, row_offset):
    """vgan_mask_backward in float64.  g_slabs: list of float32 [n, d] slabs, summed in ascending order in float32 (the
    contract); the decisions S < 1/d are the float32 ones (S is an input); everything after that is float64."""
    S32 = np.asarray(S32, dtype=np.float32)
    n, d = S32.shape
    g32 = np.array(g_slabs[0], dtype=np.float32)
    for b in g_slabs[1:]:
        g32 = g32 + np.asarray(b, dtype=np.float32)
    g = g32.astype(np.float64)
    if colkey is not None:
        r = colkey_rows(colkey) - int(row_offset)
        for j in range(d):
            if 0 <= r[j] < n:
                g[r[j], j] += float(np.float32(-np.float32(pen_weight) / np.float32(d)))
    s = S32.astype(np.float64)
    gs = np.where(S32 < np.float32(1.0 / d), g, 0.0)
    return s * (gs - (gs * s).sum(axis=1, keepdims=True))


# ---------------------------------------------------------------------------------------------- row selection
def row_sel_ref(rows, cursor, row_batches, row_stride, row_offset, n):
    """RowSel: batch row i is data row rows[(cursor % row_batches) * row_stride + row_offset + i]; cursor None reads as 0;
    rows None is the identity map row_offset + i."""
    i = np.arange(n, dtype=np.int64)
    if rows is None:
        return int(row_offset) + i
    b = (int(cursor) % int(row_batches)) if cursor is not None else 0
    return np.asarray(rows).reshape(-1)[b * int(row_stride) + int(row_offset) + i].astype(np.int64)


# ---------------------------------------------------------------------------------------------- optimiser / packing
def sum_slabs_f32(slabs):
    """ascending-order float32 sum of a list of equally shaped float32 arrays"""
    a = np.array(slabs[0], dtype=np.float32)
    for b in slabs[1:]:
        a = a + np.asarray(b, dtype=np.float32)
    return a


def homogeneous_ref(W, b):
    """[[W, b], [0, 1]]"""
    out, kin = W.shape
    P = np.zeros((out + 1, kin + 1), dtype=np.float32)
    P[:out, :kin], P[:out, kin], P[out, kin] = W, b, 1.0
    return P


# ---------------------------------------------------------------------------------------------- mask / projection forward
# vgan_mask_project_forward, vgan_mask_project_forward_bf3(_ex) of csrc/rows.hip: tests/test_mask_forward_gpu.py holds every
# kernel behind them to mask_forward_ref through check_mask_forward; tests/test_small_ops_cpu.py pins the restatement to
# CpuOps and shows that every check bites (MASK_FWD_MUTATIONS).
MASK_CHUNK = 256  # columns one pass of a wave covers: 64 lanes x float4


def expected_kernel(entry, d, n, bases, lds, chain=False, zt=False, xx=False):
    """The dispatch rule of csrc/rows.hip restated: the kernel an entry point launches.  entry: "fwd"
    (vgan_mask_project_forward) or "bf3" (vgan_mask_project_forward_bf3 / _ex); bases: the byte addresses of every buffer
    the vector kernels access 16 bytes at a time; lds: every leading dimension, in elements; zt: transposed images asked
    for.  "invalid": the entry point returns the invalid-argument error without launching."""
    aligned = all(int(b) % 16 == 0 for b in bases) and all(int(v) % 4 == 0 for v in lds)
    nt = (d // 4 + 63) // 64
    if entry == "fwd":
        if d % 4 == 0 and d <= (1024 if chain else 4096) and aligned:
            nt = nt if nt <= 4 else (8 if nt <= 8 else 16)
            return f"vec_chain<{nt}>" if chain else f"vec<{nt}>"
        return "invalid" if chain else "generic"
    assert entry == "bf3"
    if not (d % 4 == 0 and d <= 1024 and n % 8 == 0 and aligned) or ((chain or xx) and zt):
        return "invalid"
    if not (zt or xx or chain) and nt >= 2:
        return f"split<{nt}>"
    if xx:
        return f"bf3_xx_chain<{nt}>" if chain else f"bf3_xx<{nt}>"
    return f"bf3_chain<{nt}>" if chain else (f"bf3<{nt},zt>" if zt else f"bf3<{nt},lean>")


#: every instantiation the GPU module has to reach (the X-X rider is left out on purpose, see its docstring)
MASK_FWD_KERNELS = (["generic"] + [f"vec<{nt}>" for nt in (1, 2, 3, 4, 8, 16)] + [f"vec_chain<{nt}>" for nt in (1, 2, 3, 4)] +
                    [f"bf3<{nt},zt>" for nt in (1, 2, 3, 4)] + ["bf3<1,lean>"] + [f"bf3_chain<{nt}>" for nt in (1, 2, 3, 4)] +
                    [f"split<{nt}>" for nt in (2, 3, 4)])


def planted_data_row(rng, d):
    """+-2^k (1 + 2^-9 + 3 2^-19): hi = 2^k, lo = 2^(k-9), and the 16-bit split drops 3 2^-19 = 2^-17.4 relative from every
    entry with the entry's sign.  The norm of the split values is 1.14e-5 relative below the norm of the values -- 10.6 sq
    bars at d <= 64, 4.0 at d = 1024 -- so norms taken from unsplit values under norm_split show."""
    v = rng.choice([-1.0, 1.0], size=d) * 2.0 ** rng.integers(-3, 4, size=d) * (1 + 2.0 ** -9 + 3 * 2.0 ** -19)
    assert np.array_equal(v.astype(np.float32).astype(np.float64), v)
    return v.astype(np.float32)


def chain_inputs(rng, n, d, e0):
    """za [n, e0], At4 [d, e0] of the in-launch logits with the planted rows of edge_logits: the last k column of At4 holds the
    200-wide linspace and only row 1 of za reads it (za[1] = e_last: the logits are exact), row 2 of za is zero (a constant
    logits row); the other rows draw logits of standard deviation 2 from the first e0 - 1 columns."""
    za = rng.normal(size=(n, e0)).astype(np.float32)
    At = (rng.normal(size=(d, e0)) * 2.0 / np.sqrt(e0 - 1)).astype(np.float32)
    za[:, e0 - 1] = 0.0
    At[:, e0 - 1] = np.linspace(-100.0, 100.0, d, dtype=np.float32)
    if n >= 3:
        za[1], za[2] = 0.0, 0.0
        za[1, e0 - 1] = 1.0
    return za, At


def chain_delta(za, At4):
    """delta_i = e0 2^-24 max_j sum_k |z_ik a_jk|: what an fma chain of e0 terms can be off by, per row, in float64"""
    za, At4 = np.asarray(za, dtype=np.float64), np.asarray(At4, dtype=np.float64)
    return za.shape[1] * 2.0 ** -24 * (np.abs(za) @ np.abs(At4).T).max(axis=1)


def mask_forward_ref(logits, data, sel_rows, center=None):
    """logits: float32 [n, d], or (za, At4) for the in-launch logits za . At4^T (float64 products of the float32 inputs).
    Returns (S64, X, Xc): the float64 softmax, the selected data rows and float32 X - center (X itself without one)."""
    if isinstance(logits, tuple):
        lg = np.asarray(logits[0], dtype=np.float32).astype(np.float64) @ np.asarray(logits[1], dtype=np.float32).astype(np.float64).T
    else:
        lg = np.asarray(logits, dtype=np.float32).astype(np.float64)
    X = np.ascontiguousarray(np.asarray(data, dtype=np.float32)[np.asarray(sel_rows)])
    return softmax64(lg), X, (X - np.asarray(center, dtype=np.float32) if center is not None else X)


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view({2: np.uint16, 4: np.uint32, 8: np.uint64}[a.dtype.itemsize])


def check_mask_forward(out, S64, X, center=None, norm_split=False, delta=None, z_from=None, x_half=True, sel=None,
                       const_rows=(), lin_rows=()):
    """Holds one launch's outputs to the restatement (bars: module docstring of tests/test_mask_forward_gpu.py).
    out: dict of host arrays, a missing or None entry is an output the launch did not write -- S [n, d]; U [n, d]; Zx, Zy
    [n, d] (the halves of Z); sqx, sqy [n]; Zh, Zl [2n, d] uint16 (x_half False: their X rows are not looked at); ZTh, ZTl
    [d, 2n]; xrow [n].  z_from: {"Zx", "Zy"} of a run of the same inputs that wrote Z, for a launch that did not.
    delta: chain_delta() when the logits were formed in the launch.  const_rows / lin_rows: the planted logits rows.
    Returns {quantity: largest error / bar} (and "near": the share of threshold-near entries left out of the decisions)
    for the caller to print, never to assert on."""
    from test_small_ops_gpu import assert_sq, sq_bar  # the project's norm bar: imported where it lives, not copied
    S64 = np.asarray(S64, dtype=np.float64)
    n, d = S64.shape
    worst = {}
    get = lambda k: None if out.get(k) is None else np.asarray(out[k])
    # S
    s = get("S")
    assert s.dtype == np.float32 and s.shape == (n, d)
    rtol = 2e-5 + (2.0 * np.asarray(delta, dtype=np.float64)[:, None] if delta is not None else 0.0)
    bar = rtol * S64 + 2.0 ** -126
    err = np.abs(s.astype(np.float64) - S64)
    assert (err <= bar).all(), f"S: {float(np.nanmax(err / bar)):.3f} of its bar (or NaN)"
    worst["S"] = float((err / bar).max())
    tau = np.float32(1.0) / np.float32(d)
    u = upper_mask_ref(s)
    for r in const_rows:
        assert (s[r] == tau).all() and (u[r] == 1).all(), "constant logits row: S must be float32(1)/float32(d) exactly, U 1"
    for r in lin_rows:
        assert s[r].argmax() == d - 1 and (d < 64 or (s[r] == 0).any()), "200-wide row"
    if d == 1:
        assert (s == 1).all() and (u == 1).all()
    # U and the decisions
    if get("U") is not None:
        assert np.array_equal(_bits(get("U")), _bits(u)), "U is not the mask of the stored S"
    clear = np.abs(S64 * d - 1.0) > 1e-4
    assert np.array_equal((u == 1)[clear], (S64 >= 1.0 / d)[clear]), "a decision differs from the float64 one"
    rand = np.ones(n, dtype=bool)
    rand[list(const_rows) + list(lin_rows)] = False
    near = float((~clear[rand]).mean()) if rand.any() and d > 1 else 0.0
    assert near <= 0.005, f"{near:.4f} of the random rows' entries are within 1e-4 of the threshold"
    worst["near"] = near
    # Z = [X - c ; U X - c]
    c32 = np.asarray(center, dtype=np.float32) if center is not None else None
    Xc = (X - c32) if c32 is not None else X
    Zx, Zy = get("Zx"), get("Zy")
    if Zx is not None:
        assert np.array_equal(_bits(Zx), _bits(Xc)), "Zx is not float32 x - c"
    if Zy is not None:
        want = u.astype(np.float64) * X.astype(np.float64) - (c32.astype(np.float64) if c32 is not None else 0.0)
        bar = 2.0 ** -24 * np.abs(want) * (1 + 2.0 ** -20) + 2.0 ** -149
        err = np.abs(Zy.astype(np.float64) - want)
        assert (err <= bar).all(), f"Zy: {float(np.nanmax(err / bar)):.3f} of the one-rounding bar (or NaN)"
        worst["Zy"] = float((err / bar).max())
    # norms: of the launch's own Z rows (of a Z-writing run of the same inputs where this one wrote none)
    Zx_n = Zx if Zx is not None else (z_from or {}).get("Zx")
    Zy_n = Zy if Zy is not None else (z_from or {}).get("Zy")
    for name, rows in (("sqx", Zx_n), ("sqy", Zy_n)):
        got = get(name)
        if got is None:
            continue
        vals = split_value_ref(rows) if norm_split else np.asarray(rows, dtype=np.float32)
        truth = (vals.astype(np.float64) ** 2).sum(axis=1)
        assert got.shape == (n,)
        assert_sq(got, vals, d)
        worst[name] = float((np.abs(got.astype(np.float64) - truth) / np.maximum(sq_bar(d) * truth, 1e-300)).max())
    # split images
    Zh, Zl = get("Zh"), get("Zl")
    if Zh is not None:
        assert Zh.shape == Zl.shape == (2 * n, d)
        for half, rows in ((slice(0, n), Zx_n if x_half else None), (slice(n, 2 * n), Zy_n)):
            if rows is None:
                continue
            hi, lo = split_bf16_ref(rows)
            assert np.array_equal(_bits(Zh[half]), hi), "hi image"
            assert np.array_equal(_bits(Zl[half]), lo), "lo image"
        for name, rm in (("ZTh", Zh), ("ZTl", Zl)):
            if get(name) is not None:
                assert x_half and np.array_equal(_bits(get(name)), _bits(rm).T), name + " is not the transpose of the row-major image"
    if get("xrow") is not None:
        assert np.array_equal(get("xrow").astype(np.int64), np.asarray(sel, dtype=np.int64)), "xrow"
    return worst


MASK_FWD_MUTATIONS = ["ragged chunk left out of the sum", "row max over the first chunk", "norms of unsplit values", "centre kept where U == 1",
                      "selector without the cursor modulo", "selector without row_offset", "row group unwritten", "hi and lo swapped",
                      "transposed image shifted by a row group", "<= in the mask"]


def emulate_mask_forward(logits, data, table, cursor, row_batches, row_stride, row_offset, center=None, norm_split=False, mutation=None):
    """What a correct float32 implementation writes (every optional output included), computed op for op in numpy float32
    where the order of operations matters (the softmax) and by one rounding of the float64 value elsewhere -- or, with
    `mutation`, what one of the faults of MASK_FWD_MUTATIONS writes.  The `out` of check_mask_forward."""
    assert mutation is None or mutation in MASK_FWD_MUTATIONS
    if isinstance(logits, tuple):
        x = (np.asarray(logits[0], dtype=np.float64) @ np.asarray(logits[1], dtype=np.float64).T).astype(np.float32)
    else:
        x = np.asarray(logits, dtype=np.float32)
    n, d = x.shape
    last = MASK_CHUNK * ((d - 1) // MASK_CHUNK)  # first column of the last chunk
    with np.errstate(over="ignore", invalid="ignore"):
        m = (x[:, :MASK_CHUNK] if mutation == "row max over the first chunk" else x).max(axis=1, keepdims=True)
        e = np.exp(x - m)
        tot = (e[:, :last] if mutation == "ragged chunk left out of the sum" else e).sum(axis=1, keepdims=True, dtype=np.float32)
        s = (e / tot).astype(np.float32)
    tau = np.float32(1.0) / np.float32(d)
    u = np.where((s <= tau) if mutation == "<= in the mask" else (s < tau), s, np.float32(1.0)).astype(np.float32)
    if mutation == "selector without the cursor modulo":
        sel = row_sel_ref(table, cursor, 2 ** 62, row_stride, row_offset, n)
    elif mutation == "selector without row_offset":
        sel = row_sel_ref(table, cursor, row_batches, row_stride, 0, n)
    else:
        sel = row_sel_ref(table, cursor, row_batches, row_stride, row_offset, n)
    X = np.asarray(data, dtype=np.float32)[sel]
    c32 = np.asarray(center, dtype=np.float32) if center is not None else np.zeros(d, dtype=np.float32)
    Zx = X - c32
    Zy = (u.astype(np.float64) * X.astype(np.float64) - c32.astype(np.float64)).astype(np.float32)
    if mutation == "centre kept where U == 1":
        Zy = np.where(u == 1, X, Zy)
    Z = np.concatenate([Zx, Zy])
    vals = split_value_ref(Z) if norm_split and mutation != "norms of unsplit values" else Z
    sq = (vals.astype(np.float64) ** 2).sum(axis=1).astype(np.float32)
    Zh, Zl = split_bf16_ref(Z)
    if mutation == "hi and lo swapped":
        Zh, Zl = Zl, Zh
    ZTh, ZTl = Zh.T.copy(), Zl.T.copy()
    if mutation == "transposed image shifted by a row group":
        ZTh, ZTl = np.roll(ZTh, 8, axis=1), np.roll(ZTl, 8, axis=1)
    out = dict(S=s, U=u, Zx=Zx, Zy=Zy, sqx=sq[:n], sqy=sq[n:], Zh=Zh, Zl=Zl, ZTh=ZTh, ZTl=ZTl, xrow=sel.astype(np.int32))
    if mutation == "row group unwritten":  # the last group of 8 batch rows keeps its sentinels
        g = slice(n - 8, n)
        for k in ("S", "U", "Zx", "Zy", "sqx", "sqy"):
            out[k] = out[k].copy()
            out[k][g] = np.nan
        for k in ("Zh", "Zl"):
            out[k] = out[k].copy()
            out[k][g], out[k][n + n - 8:] = 0x5A5A, 0x5A5A
        out["xrow"][g] = -1
    return out
