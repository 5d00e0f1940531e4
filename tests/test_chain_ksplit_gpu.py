"""In-launch K split of the long-K chain products (vgan_linear_backward_params_ksplit, vgan_gemm_grouped_ksplit) on an MI355X.

Reference and bound: the float64 product on the host; per element |err| <= K * 2^-23 * sum_k |a_k b_k| -- the
order-independent bound of an fp32 summation of K terms (K * 2^-24 * sum |a_k b_k| to first order) with a factor 2 of
margin.  No tuned tolerance.  Besides: parts = 1 is the unsplit launch bit for bit; the result does not depend on which part
arrives last (same bits on every call, eager and graph replay); every launch leaves its tickets at 0."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ops():
    from vgan_amd.ops import HipOps
    return HipOps()


def dev(a):
    return torch.as_tensor(np.ascontiguousarray(a, dtype=np.float32)).cuda()


def check_product(got, a64, b64, k):
    """got ~ a64 @ b64 (float64 operands holding the float32 inputs exactly) within the summation bound."""
    want = a64 @ b64
    bound = k * 2.0 ** -23 * (np.abs(a64) @ np.abs(b64))
    err = np.abs(got.double().cpu().numpy() - want)
    worst = float((err / np.maximum(bound, 1e-300)).max())
    print(f"K={k} max |err| {err.max():.3e}, worst err/bound {worst:.3f}")
    assert (err <= bound).all(), worst


def tickets(ws, count):
    return ws[:count].cpu().numpy()


def repeat_and_replay(launch, out, ws, ntickets):
    """Three eager calls and three replays of a captured call all give the same bits, and the tickets are back at 0."""
    results = []
    for _ in range(3):
        out.fill_(float("nan"))
        launch()
        results.append(out.clone())
    torch.cuda.synchronize()
    assert torch.equal(results[0], results[1]) and torch.equal(results[0], results[2])
    if ws is not None:
        assert not tickets(ws, ntickets).any()
    graph = torch.cuda.CUDAGraph()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        with torch.cuda.graph(graph, stream=side):
            launch()
    for _ in range(3):
        out.fill_(float("nan"))
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(out, results[0])
    if ws is not None:
        assert not tickets(ws, ntickets).any()
    return results[0]


# ---- M_4-style product dW = dy^T x ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,out,kin,parts", [(300, 36, 52, 4),  # kchunk 128: parts of 128 / 128 / 44 rows and an EMPTY fourth one;
                                                                # ragged tiles in both output dimensions, ragged last K tile
                                             (1024, 64, 32, 1), (1024, 64, 32, 2), (1024, 64, 32, 4), (1024, 64, 32, 8)])
def test_linear_backward_params_ksplit(ops, n, out, kin, parts):
    rng = np.random.default_rng(100 + parts)
    dy, x = rng.normal(size=(n, out)).astype(np.float32), rng.normal(size=(n, kin)).astype(np.float32)
    dyd, xd = dev(dy), dev(x)
    dW = torch.empty(out, kin, device="cuda")
    tiles = ((out + 31) // 32) * ((kin + 31) // 32)
    nbytes = ops.linear_backward_params_ksplit_ws_bytes(kin, out, parts)
    assert (nbytes == 0) == (parts == 1)
    ws = ops.ksplit_workspace(nbytes) if parts > 1 else None
    got = repeat_and_replay(lambda: ops.linear_backward_params_ksplit(dyd, xd, dW, parts, ws), dW, ws, tiles)
    check_product(got, dy.astype(np.float64).T, x.astype(np.float64), n)
    if parts == 1:
        plain = torch.empty_like(dW)
        ops.linear_backward_params(dyd, xd, plain, None)
        assert torch.equal(got, plain)


# ---- grouped launch ---------------------------------------------------------------------------------------------------------
def fold_job_inputs(ops):
    """A small complete step tail (mode 0) to ride as the `fold` job: its outputs depend on nothing the products write."""
    n, d = 64, 8
    rng = np.random.default_rng(5)
    tiles = ops.build_tiles(n, 1, 0, 1, device="cuda", tile=64)
    partial = dev(rng.random(size=4 * tiles.shape[0]))
    chunks = ops.colmax_chunks(n)
    u = rng.random(size=(chunks, d)).astype(np.float32) * 0.5 + 0.25
    keys = (u.view(np.uint32).astype(np.int64) << 32) | (0xFFFFFFFF - rng.integers(0, n, size=(chunks, d)))
    colpart = torch.as_tensor(keys.reshape(-1)).cuda()
    return n, d, tiles, partial, chunks, colpart


def fold_outputs(d):
    return dict(colkey=torch.zeros(d, dtype=torch.int64, device="cuda"), stats=torch.zeros(4, dtype=torch.float64, device="cuda"),
                loss=torch.zeros(1, device="cuda"), accum=torch.full((1,), 0.5, device="cuda"),
                counter=torch.full((1,), 41, dtype=torch.int64, device="cuda"))


def test_grouped_ksplit_tn_with_copy_and_fold(ops):
    """Three TN products in one launch, two of them split (2 parts: 128 + 72; 4 parts of K = 784: 256 / 256 / 256 / 16), one
    not; a copy rider and a fold job ride along and give what they give in the unsplit launch."""
    rng = np.random.default_rng(11)
    shapes = [(40, 52, 200, 2), (100, 52, 784, 4), (36, 52, 784, 1)]  # m, n, k, parts
    A = [rng.normal(size=(k, m)).astype(np.float32) for m, n, k, _ in shapes]
    B = [rng.normal(size=(k, n)).astype(np.float32) for m, n, k, _ in shapes]
    Ad, Bd = [dev(a) for a in A], [dev(b) for b in B]
    C = torch.empty(sum(m for m, _, _, _ in shapes), 52, device="cuda")
    rows = np.cumsum([0] + [m for m, _, _, _ in shapes])
    Cs = [C[rows[i]:rows[i + 1]] for i in range(3)]
    problems = [("TN", Ad[i], Bd[i], Cs[i]) for i in range(3)]
    kparts = [p for _, _, _, p in shapes]
    src = dev(rng.normal(size=3000))
    n, d, tiles, partial, chunks, colpart = fold_job_inputs(ops)

    def run(split):
        dst, fo = torch.zeros_like(src), fold_outputs(d)
        job = ops.finalize_job(partial, tiles, colpart, chunks, fo["colkey"], n, d, 10.0, fo["stats"], fo["loss"], fo["accum"], 0.25,
                               fo["counter"])
        C.fill_(float("nan"))
        ops.gemm_grouped(problems, copy=(src, dst), fold=job, **split)
        torch.cuda.synchronize()
        return C.clone(), dst, fo

    unsplit, dst0, fold0 = run({})
    ntick = sum(((m + 31) // 32) * ((n_ + 31) // 32) for m, n_, _, p in shapes if p > 1)
    ws = ops.ksplit_workspace(ops.gemm_grouped_ksplit_ws_bytes(problems, kparts))
    split, dst1, fold1 = run(dict(kparts=kparts, ksplit_ws=ws))
    assert not tickets(ws, ntick).any()
    assert torch.equal(dst0, src) and torch.equal(dst1, src)
    for key in fold0:
        assert torch.equal(fold0[key], fold1[key]), key
    assert int(fold1["counter"]) == 42 and float(fold1["loss"]) != 0.0
    assert torch.equal(split[rows[2]:], unsplit[rows[2]:])  # the unsplit problem: the same tile code, the same bits
    for i, (m, n_, k, _) in enumerate(shapes):
        check_product(split[rows[i]:rows[i + 1]], A[i].astype(np.float64).T, B[i].astype(np.float64), k)
    # kparts all 1 is the unsplit launch itself
    C.fill_(float("nan"))
    ops.gemm_grouped(problems, kparts=[1, 1, 1])
    assert torch.equal(C, unsplit)
    # determinism, ticket reset, graph replay (products only: the fold job advances a counter on every call)
    got = repeat_and_replay(lambda: ops.gemm_grouped(problems, kparts=kparts, ksplit_ws=ws), C, ws, ntick)
    assert torch.equal(got, split)


@pytest.mark.parametrize("kind", ["NN", "NT"])
def test_grouped_ksplit_nn_nt(ops, kind):
    """m = n = 36, k = 300 in 2 parts (256 + 44)."""
    rng = np.random.default_rng(17)
    m = n = 36
    k = 300
    a = rng.normal(size=(m, k)).astype(np.float32)
    b = rng.normal(size=(k, n) if kind == "NN" else (n, k)).astype(np.float32)
    ad, bd = dev(a), dev(b)
    C = torch.empty(m, n, device="cuda")
    problems = [(kind, ad, bd, C)]
    ws = ops.ksplit_workspace(ops.gemm_grouped_ksplit_ws_bytes(problems, [2]))
    got = repeat_and_replay(lambda: ops.gemm_grouped(problems, kparts=[2], ksplit_ws=ws), C, ws, 4)
    b64 = b.astype(np.float64)
    check_product(got, a.astype(np.float64), b64 if kind == "NN" else b64.T, k)
