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
