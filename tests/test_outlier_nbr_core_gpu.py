"""The shared core of the detectors on the refined neighbour lists (csrc/outlier_nbr.hpp) at its edges, on the MI355X: the ops
entries called directly on hand-made lists, against the restatements and the bars of test_outlier_abod_*.py and
test_outlier_cof_*.py.

One launch covers the subspace widths 1 (64 neighbours in one load), 2, 31, 32 and 64 (exact ends of the 32-feature block,
where the prefetch guard flips), 33 and 65 (a last block of one feature).  k sits on both sides of every pair-block edge
(8 | 16 | 32), nq in 1, 3, 4, 5 leaves surplus waves in the only workgroup and in the last one, nr is k + 1 and 40.  The query
matrix is not the reference matrix, both have a row stride beyond d (NaN in the padding), and the scores go to a matrix wider
than nq whose untouched cells must keep a sentinel."""
import numpy as np
import pytest

from test_outlier_abod_cpu import restate_abod_from_lists, restate_floor
from test_outlier_abod_gpu import _check_rows as check_abod_rows
from test_outlier_cof_cpu import CHAINS, restate_ceiling, restate_cof_chain, restate_cof_from_lists
from test_outlier_cof_gpu import MIN_GAP, _check_ac, _check_rows as check_cof_rows

pytestmark = pytest.mark.gpu

D, LDQ, LDR = 70, 75, 83
WIDTHS = [1, 2, 31, 32, 33, 64, 65]
NQS = [1, 3, 4, 5]
SENTINEL = -7.0
FEATS = [np.sort(np.random.default_rng(11).choice(D, w, replace=False)) for w in WIDTHS]
S = len(WIDTHS)


@pytest.fixture(scope="module")
def ops():
    from vgan_amd.ops import HipOps
    return HipOps()


def _padded(X, ld):
    """X on the device as the leading columns of a NaN matrix of row stride ld."""
    import torch
    buf = torch.full((X.shape[0], ld), float("nan"), dtype=torch.float32, device="cuda")
    buf[:, :X.shape[1]] = torch.as_tensor(X)
    return buf[:, :X.shape[1]]


def _table():
    import torch
    feat = torch.as_tensor(np.concatenate(FEATS).astype(np.int32), device="cuda")
    off = torch.as_tensor(np.concatenate([[0], np.cumsum(WIDTHS)]).astype(np.int32), device="cuda")
    return feat, off, None


def _case(k, nq, nr, seed):
    """(Xq, Xr, idx int32 [S, nq, k] of distinct reference rows) from one seed."""
    rng = np.random.default_rng(seed)
    Xq, Xr = rng.normal(size=(nq, D)).astype(np.float32), rng.normal(size=(nr, D)).astype(np.float32)
    idx = np.array([[rng.permutation(nr)[:k] for _ in range(nq)] for _ in range(S)], np.int32)
    return Xq, Xr, idx


def _score_matrix(nq, permute, seed):
    """(the matrix [S + 2, nq + 3] of sentinels, its [:, :nq] view, score_row on the device or None, the rows as numpy)."""
    import torch
    full = torch.full((S + 2, nq + 3), SENTINEL, dtype=torch.float32, device="cuda")
    rows = np.random.default_rng(seed).permutation(S + 2)[:S].astype(np.int32) if permute else np.arange(S, dtype=np.int32)
    return full, full[:, :nq], torch.as_tensor(rows, device="cuda") if permute else None, rows


def _untouched(full, rows, nq):
    got = full.cpu().numpy()
    keep = np.ones(got.shape, bool)
    keep[rows, :nq] = False
    return (got[keep] == SENTINEL).all()


@pytest.mark.parametrize("k", [2, 8, 9, 16, 17, 32])
def test_abod_on_hand_made_lists(k, ops):
    """Every row within one float32 ulp of restate_abod_from_lists, degenerate rows NaN and then exactly the floor.  With
    missing slots (-1 and nr in the list) the kernel promises that the slot is unusable, as if the entry were not in the
    list: the index is never dereferenced, the slot is staged as exactly 0, its norm is 0 and no pair takes it.  The
    restatement therefore runs on the list with those entries dropped; rows left with fewer than two neighbours are
    degenerate."""
    import torch
    for n_case, (nq, nr, missing, permute) in enumerate((nq, nr, m, p) for nq in NQS for nr in (k + 1, 40)
                                                        for m, p in ((False, False), (True, True))):
        Xq, Xr, idx = _case(k, nq, nr, 1000 * k + n_case)
        if missing:
            rng = np.random.default_rng(n_case)
            hole = rng.random(idx.shape) < 0.3
            idx[hole] = np.where(rng.random(idx.shape) < 0.5, -1, nr)[hole]
        full, view, score_row, rows = _score_matrix(nq, permute, n_case)
        ops.outlier_abod(_padded(Xq, LDQ), _padded(Xr, LDR), _table(), 0, S, torch.as_tensor(idx, device="cuda"), k, view, score_row)
        assert _untouched(full, rows, nq)
        raw = full.cpu().numpy()[rows, :nq]
        want = np.array([[restate_abod_from_lists(Xq[[q]], Xr, FEATS[s], idx[s, q][(idx[s, q] >= 0) & (idx[s, q] < nr)][None, :])[0]
                          for q in range(nq)] for s in range(S)])
        np.testing.assert_array_equal(np.isnan(raw), np.isnan(want))
        assert missing or not np.isnan(want).any()
        per, floor, ndeg = restate_floor(raw)
        value = torch.empty(S + 2, dtype=torch.float64, device="cuda")
        count = torch.empty(S + 2, dtype=torch.int32, device="cuda")
        ops.outlier_abod_floor(view, value, count)
        assert _untouched(full, rows, nq)
        got = full.cpu().numpy()[rows, :nq]
        np.testing.assert_array_equal(got, per)
        np.testing.assert_array_equal(value.cpu().numpy()[rows], floor)
        np.testing.assert_array_equal(count.cpu().numpy()[rows], ndeg)
        for s in range(S):
            check_abod_rows(got[s], want[s], floor[s])


@pytest.mark.parametrize("chain", CHAINS)
@pytest.mark.parametrize("k", [1, 2, 8, 9, 16, 17, 32])
def test_cof_on_hand_made_lists(k, chain, ops):
    """The chaining distances within (d_s + k + 8) 2^-53 of restate_cof_chain (its smallest chain gap asserted first), the
    scores within one float32 ulp of restate_cof_from_lists: the bars of test_outlier_cof_gpu.py.  Lists with missing slots
    are left out: the chain kernel stages an index outside the reference set as the zero vector and keeps k, so the slot is a
    point at the origin, not a dropped entry, and the restatement on the shortened list disagrees with it (before the shared
    core as well); SubspaceCOF never passes such a list."""
    import torch
    for n_case, (nq, nr, permute) in enumerate((nq, nr, p) for nq in NQS for nr in (k + 1, 40) for p in (False, True)):
        Xq, Xr, idx = _case(k, nq, nr, 2000 * k + n_case)
        idx_dev = torch.as_tensor(idx, device="cuda")
        ac = torch.full((S + 1, nq), SENTINEL, dtype=torch.float64, device="cuda")
        ops.outlier_cof_chain(_padded(Xq, LDQ), _padded(Xr, LDR), _table(), 0, S, idx_dev, k, CHAINS.index(chain), ac[:S])
        got_ac = ac.cpu().numpy()
        assert (got_ac[S] == SENTINEL).all()
        for s in range(S):
            want, gap = restate_cof_chain(Xq, Xr, FEATS[s], idx[s], chain)
            assert gap.min() >= MIN_GAP, (s, nq, nr, float(gap.min()))
            _check_ac(got_ac[s], want, WIDTHS[s], k)
        ac_ref = np.random.default_rng(n_case).uniform(0.5, 2.0, size=(S, nr))
        full, view, score_row, rows = _score_matrix(nq, permute, n_case)
        ops.outlier_cof_score(ac[:S], torch.as_tensor(ac_ref, device="cuda"), idx_dev, k, view, score_row)
        assert _untouched(full, rows, nq)
        got = full.cpu().numpy()[rows, :nq]
        for s in range(S):
            check_cof_rows(got[s], restate_cof_from_lists(got_ac[s], ac_ref[s], idx[s]), 1.0)


@pytest.mark.parametrize("n", [1, 255, 256, 257, 1025])
@pytest.mark.parametrize("entry, restate, default", [("outlier_abod_floor", restate_floor, 0.0),
                                                     ("outlier_cof_ceiling", restate_ceiling, 1.0)])
def test_fill_kernel_in_both_directions(entry, restate, default, n, ops):
    """Rows with no NaN, all NaN (the default, n_degenerate = n) and mixed, in a matrix wider than n: the fit takes the
    extreme, the count and the filled row exactly as the restatement does; fit = 0 applies a stored value that is not the
    row's own extreme and writes neither the value nor a count."""
    import torch
    rng = np.random.default_rng(n)
    raw = rng.normal(size=(3, n)).astype(np.float32)
    raw[1] = np.nan
    raw[2, rng.random(n) < 0.4] = np.nan
    raw[2, -1] = np.nan if n > 1 else raw[2, -1]
    full = torch.full((3, n + 5), SENTINEL, dtype=torch.float32, device="cuda")
    full[:, :n] = torch.as_tensor(raw)
    value = torch.full((3,), 99.0, dtype=torch.float64, device="cuda")
    count = torch.full((3,), -1, dtype=torch.int32, device="cuda")
    getattr(ops, entry)(full[:, :n], value, count)
    per, want_value, ndeg = restate(raw)
    assert want_value[1] == default and ndeg[1] == n and ndeg[0] == 0
    np.testing.assert_array_equal(full.cpu().numpy()[:, :n], per)
    np.testing.assert_array_equal(value.cpu().numpy(), want_value)
    np.testing.assert_array_equal(count.cpu().numpy(), ndeg)
    assert (full.cpu().numpy()[:, n:] == SENTINEL).all()

    stored = np.array([3.5, -2.25, 0.125])
    full[:, :n] = torch.as_tensor(raw)
    value = torch.as_tensor(stored, device="cuda")
    getattr(ops, entry)(full[:, :n], value)
    np.testing.assert_array_equal(full.cpu().numpy()[:, :n], restate(raw, stored)[0])
    np.testing.assert_array_equal(value.cpu().numpy(), stored)
    assert (full.cpu().numpy()[:, n:] == SENTINEL).all()
