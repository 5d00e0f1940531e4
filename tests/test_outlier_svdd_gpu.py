"""Deep SVDD over the subspaces on the MI355X (csrc/outlier_svdd.hip through vgan_amd.SubspaceDeepSVDD and vgan_amd.ops), against
the numpy restatement of test_outlier_svdd_cpu.py.

The initial draw is bit-equal to the restatement.  The forward (embed) is compared per element with the float64 net on the
device's own weights within the first-order bound of test_outlier_svdd_cpu.py; the centre is the restated two-level sum of the
device's OWN outputs, bit for bit; a step is checked from the device's OWN state (theta, m, v read before and after): m and v
against the float64 gradient at the device's theta within their bounds, theta against the float64 Adam formula on the device's
new moments within 2u (8 |step| + |theta|), the loss within its bound.  Everything else is exact: every cut of the steps into
launches, of the rows into calls and of the subspaces into chunks gives the same bits."""
import functools

import numpy as np
import pytest

from gemm_ref import worst_ratio
from test_outlier_ae_cpu import ARC_AUC_COV, ARC_SEEDS, DEFAULT_HP, STEP_D, STEP_SEED, U, arc_data, batch_rows, restate_moments, restate_scaling, step_features, step_matrix
from test_outlier_ecod_cpu import _mask
from test_outlier_iforest_cpu import auc
from test_outlier_kpca_cpu import ring
from test_outlier_norm_gpu import _check_scores
from test_outlier_svdd_cpu import (ARC_AUC_SVDD, ARC_NET, AUC_MARGIN, RING_AUC_COV, RING_AUC_SVDD, RING_NET, RING_SEEDS, TRAJ, TRAJ_SEEDS, TRAJ_YARDSTICK,
                                   check_step, clamp_center, layer_sizes, max_weight_deviation, restate_center, restate_fit, restate_forward,
                                   restate_init, traj_case, two_level_mean)

pytestmark = pytest.mark.gpu

ACT = {"tanh": 0, "relu": 1}
STEP_HIDDEN = (5, 3)
NETS = [(1,), (3, 2), (33, 7), (128, 64, 2)]


def _ops():
    from vgan_amd.ops import default_ops
    return default_ops()


def _dev(a):
    import torch
    return torch.as_tensor(np.ascontiguousarray(a), device="cuda")


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _table(feats_list):
    feat = np.concatenate([np.asarray(f) for f in feats_list]).astype(np.int32)
    off = np.concatenate([[0], np.cumsum([len(f) for f in feats_list])]).astype(np.int32)
    return _dev(feat), _dev(off), None


def _init_scale(dims, hidden):
    return _dev(1.0 / np.sqrt(np.array([[K for K, _ in layer_sizes(d_s, hidden)] for d_s in dims], dtype=np.float64)))


def _params_of(dims, hidden):
    return np.array([sum(K * N for K, N in layer_sizes(d_s, hidden)) for d_s in dims], dtype=np.int64)


def _device_init(table, dims, hidden, first, count, seed):
    """(state, s_off, host offsets) of vgan_svdd_init for the blocks first .. first + count - 1."""
    import torch
    sizes = _params_of(dims, hidden)[first:first + count]
    off = np.concatenate([[0], np.cumsum(3 * sizes)]).astype(np.int64)
    state = torch.full((int(off[-1]),), float("nan"), dtype=torch.float32, device="cuda")  # the entry zeroes the moments itself
    s_off = _dev(off[:-1])
    _ops().svdd_init(table[1], (tuple(hidden), 0), first, count, _init_scale(dims, hidden), seed, state, s_off, int(off[-1]))
    return state, s_off, off


def _unpack(flat, d_s, hidden):
    """(Ws, m, v) as lists of W [N, K] from the K-major state of one block."""
    P = int(_params_of([d_s], hidden)[0])
    out = []
    for part in range(3):
        at, layers = part * P, []
        for K, N in layer_sizes(d_s, hidden):
            layers.append(flat[at:at + K * N].reshape(K, N).T.copy())
            at += K * N
        out.append(layers)
    return out


def _blocks(state, off, dims, hidden):
    flat = state.cpu().numpy()
    return [_unpack(flat[off[z]:off[z + 1]], d_s, hidden) for z, d_s in enumerate(dims)]


def _step_mask():
    return _mask(STEP_D + 2, step_features())


# ---- 1. the initial draw ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("hidden", NETS)
def test_init_equals_the_restatement_bit_for_bit(hidden):
    """Subspaces of 1, 2, 31, 32, 33 and 70 features (rows that straddle the 4 words of a Philox call), all six in one call and the
    blocks 2 .. 4 alone (position keying), a seed that crosses the 32-bit halves of the key; the moments are zero."""
    dims = [1, 2, 31, 32, 33, 70]
    table = _table([np.arange(d_s) for d_s in dims])
    for first, count in ((0, 6), (2, 3)):
        state, _, off = _device_init(table, dims, hidden, first, count, STEP_SEED)
        for z, (Ws, m, v) in enumerate(_blocks(state, off, dims[first:first + count], hidden)):
            want = restate_init(STEP_SEED, first + z, dims[first + z], hidden)
            for W, Ww, mW, vW in zip(Ws, want, m, v):
                np.testing.assert_array_equal(_bits(W), _bits(Ww), err_msg=f"{hidden} block {first + z}")
                assert not mW.any() and not vW.any()


# ---- 2. the forward (epochs = 0) ----------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _untrained(hidden, activation):
    import vgan_amd
    X = step_matrix(70)
    return X, vgan_amd.SubspaceDeepSVDD(_step_mask(), np.full(5, 0.2), hidden=hidden, activation=activation, epochs=0, seed=STEP_SEED).fit(X)


def _check_forward(ens, Y, activation, mask, subspaces):
    """embed within the bound of the float64 net on the device's own weights; the score against the float64 sum of the float32
    differences of the device's own output: the squares are exact in float64, their sum costs a few 2^-53, the rounding to
    float32 at most u: 2u score."""
    worst = 0.0
    z_all = restate_scaling(Y, ens.location_, ens.scale_)
    _, per = ens.decision_function(Y, return_per_subspace=True)
    for s in subspaces:
        z = z_all[:, mask[s]]
        h, E, _ = restate_forward(z, ens.weights_[s], activation)
        got = ens.embed(Y, s)
        assert got.dtype == np.float32 and got.shape == (len(Y), ens.hidden[-1])
        worst = max(worst, worst_ratio(got, h[-1], E[-1]))
        r = (got - ens.center_[s][None, :]).astype(np.float32).astype(np.float64)
        want = (r * r).sum(axis=1)
        assert (np.abs(per[s] - want) <= 2.0 * U * want).all(), s
    return worst


@pytest.mark.parametrize("activation", ["relu", "tanh"])
@pytest.mark.parametrize("hidden", NETS)
def test_embed_stays_within_the_bound_and_is_split_invariant(hidden, activation):
    """Query rows 1, 31, 32, 33 and 70 across the 32-row tile; subspaces of 1, 3, 33 and 70 features and a constant one."""
    X, ens = _untrained(hidden, activation)
    mask = _step_mask()
    np.testing.assert_allclose(ens.location_, restate_moments(X)[0], rtol=1e-13, atol=1e-300)
    np.testing.assert_allclose(ens.scale_, restate_moments(X)[1], rtol=1e-12)
    assert ens.n_steps_ == 0 and ens.loss_history_.shape == (5, 0)
    for s, d_s in enumerate((1, 3, 33, 70, 2)):  # untrained: the weights are the initial draw
        for W, Ww in zip(ens.weights_[s], restate_init(STEP_SEED, s, d_s, hidden)):
            np.testing.assert_array_equal(_bits(W), _bits(Ww))
    worst = 0.0
    for n in (1, 31, 32, 33, 70):
        worst = max(worst, _check_forward(ens, step_matrix(n, seed=n), activation, mask, range(4)))
    print(f"{hidden} {activation}: worst err / bound {worst:.3f}")
    assert worst <= 1.0
    Y = step_matrix(70, seed=70)
    whole, whole_per = ens.decision_function(Y, return_per_subspace=True)
    cuts = ((0, 1), (1, 34), (34, 70))
    parts = [ens.decision_function(Y[a:b], return_per_subspace=True)[1] for a, b in cuts]
    np.testing.assert_array_equal(_bits(np.concatenate(parts, axis=1)), _bits(whole_per))
    for s in (0, 2, 3, 4):
        emb = np.concatenate([ens.embed(Y[a:b], s) for a, b in cuts])
        np.testing.assert_array_equal(_bits(emb), _bits(ens.embed(Y, s)))
    assert (whole_per[4] == 0.0).all() and not ens.embed(Y, 4).any()  # the constant subspace: z = 0 through a net without bias
    np.testing.assert_array_equal(ens.decision_function(X), ens.decision_scores_)


def test_embed_of_a_wide_net_runs_from_the_scratch_buffer():
    """d_s = 1024 with hidden (128, 128): the activations of a 32-row tile do not fit LDS and live in the scratch slices; the same
    bound, the same centre and the same bits under a workspace that holds one row tile at a time."""
    import vgan_amd
    from vgan_amd import outlier as o
    assert o.svdd_act_floats(1024, (128, 128), 32, False) > o.AE_LDS_FLOATS
    rng = np.random.default_rng(8)
    X, Y = rng.normal(size=(40, 1024)).astype(np.float32), rng.normal(size=(65, 1024)).astype(np.float32)
    kw = dict(hidden=(128, 128), activation="tanh", epochs=0, seed=3)
    ens = vgan_amd.SubspaceDeepSVDD(np.ones((1, 1024), bool), [1.0], **kw).fit(X)
    worst = _check_forward(ens, Y, "tanh", np.ones((1, 1024), bool), [0])
    print(f"worst err / bound {worst:.3f}")
    assert worst <= 1.0
    want, emb = ens.decision_function(Y), ens.embed(Y, 0)
    ens.workspace_bytes = 1
    np.testing.assert_array_equal(ens.decision_function(Y), want)
    np.testing.assert_array_equal(_bits(ens.embed(Y, 0)), _bits(emb))
    tight = vgan_amd.SubspaceDeepSVDD(np.ones((1, 1024), bool), [1.0], workspace_bytes=o.svdd_net_bytes(1024, (128, 128), 32), **kw).fit(X)
    np.testing.assert_array_equal(_bits(tight.center_), _bits(ens.center_))  # the centre from one row tile a call


# ---- 3. the centre ------------------------------------------------------------------------------------------------------------------
CENTER_CASE = dict(hidden=(33, 7), activation="relu", s=3, center_eps=0.1)


def test_center_is_the_two_level_sum_of_the_devices_own_outputs():
    """center_ and n_clamped_ of every net against the restated rule on the device's own embed output, bit for bit; the chosen
    case (subspace 3, hidden (33, 7), relu) has float64 means that the rule moves to +center_eps, to -center_eps and leaves
    alone, each farther from center_eps and from 0 than the forward bound of a device mean, so the device takes the same branch;
    the same bits when the rows come in calls of one tile."""
    import torch
    X, mask = step_matrix(70), _step_mask()
    for hidden, activation in ((CENTER_CASE["hidden"], CENTER_CASE["activation"]), ((3, 2), "tanh"), ((128, 64, 2), "relu")):
        _, ens = _untrained(hidden, activation)
        assert ens.center_.dtype == np.float32 and ens.center_.shape == (5, hidden[-1]) and ens.n_clamped_.shape == (5,)
        for s in range(4):
            c, clamped = clamp_center(two_level_mean(ens.embed(X, s)), 0.1)
            np.testing.assert_array_equal(_bits(ens.center_[s]), _bits(c), err_msg=f"{hidden} subspace {s}")
            assert ens.n_clamped_[s] == clamped
        assert not ens.center_[4].any() and ens.n_clamped_[4] == 0  # the constant subspace
    _, ens = _untrained(CENTER_CASE["hidden"], CENTER_CASE["activation"])
    s, eps = CENTER_CASE["s"], CENTER_CASE["center_eps"]
    z = restate_scaling(X, ens.location_, ens.scale_)[:, mask[s]]
    c, clamped, mean, E_mean = restate_center(z, ens.weights_[s], CENTER_CASE["activation"], eps)
    print(f"means {mean}, bounds {E_mean}")
    up, down, kept = (mean >= 0) & (np.abs(mean) < eps), (mean < 0) & (np.abs(mean) < eps), np.abs(mean) >= eps
    assert up.any() and down.any() and kept.any()
    assert (np.abs(np.abs(mean) - eps) > E_mean).all() and (np.abs(mean) > E_mean).all()
    assert (c[up] == np.float32(eps)).all() and (c[down] == np.float32(-eps)).all() and clamped == up.sum() + down.sum()
    assert ens.n_clamped_[s] == clamped and (ens.center_[s][up] == np.float32(eps)).all() and (ens.center_[s][down] == np.float32(-eps)).all()
    assert (np.abs(ens.center_[s][kept].astype(np.float64) - mean[kept]) <= E_mean[kept] + U * np.abs(mean[kept])).all()
    # the rows in calls of 32, 32 and 6 against one call of 70
    q = CENTER_CASE["hidden"][-1]
    Xd = _dev(X)
    results = []
    for cuts in (((0, 70),), ((0, 32), (32, 64), (64, 70))):
        run = torch.zeros(5 * q, dtype=torch.float64, device="cuda")
        tiles = torch.full((5 * 3 * q,), float("nan"), dtype=torch.float64, device="cuda")
        center = torch.full((5, q), float("nan"), dtype=torch.float32, device="cuda")
        clamped_d = torch.full((5,), -1, dtype=torch.int32, device="cuda")
        for a, b in cuts:
            _ops().svdd_center(Xd[a:b], ens._table, ens._scaling, ens._skip, ens._net, 0, 5, 70, ens._theta, ens._w_off, tiles, run,
                               70 if b == 70 else 0, eps, center, clamped_d)
        results.append((center.cpu().numpy(), clamped_d.cpu().numpy(), run.cpu().numpy()))
    np.testing.assert_array_equal(_bits(results[0][0]), _bits(ens.center_))
    np.testing.assert_array_equal(results[0][1], ens.n_clamped_)
    np.testing.assert_array_equal(_bits(results[1][0]), _bits(results[0][0]))
    np.testing.assert_array_equal(results[1][1], results[0][1])
    np.testing.assert_array_equal(results[1][2], results[0][2])


def test_a_given_center_is_used_as_it_is_and_center_eps_zero_disables_the_rule():
    import vgan_amd
    X, mask = step_matrix(70), _step_mask()
    given = np.array([[0.01, -2.5], [0.0, 0.3], [1e-3, 1e-3], [-0.05, 0.05], [7.0, 7.0]], np.float64)
    ens = vgan_amd.SubspaceDeepSVDD(mask, np.full(5, 0.2), hidden=(3, 2), center=given, epochs=1, batch_size=16, seed=STEP_SEED).fit(X)
    np.testing.assert_array_equal(_bits(ens.center_[:4]), _bits(given[:4].astype(np.float32)))  # no clamp on a given centre
    assert not ens.center_[4].any() and not ens.n_clamped_.any()
    for s in range(4):
        r = (ens.embed(X, s) - ens.center_[s][None, :]).astype(np.float32).astype(np.float64)
        want = (r * r).sum(axis=1)
        assert (np.abs(ens.per_subspace_scores_[s] - want) <= 2.0 * U * want).all()
    shared = vgan_amd.SubspaceDeepSVDD(mask, np.full(5, 0.2), hidden=(3, 2), center=[0.5, -0.5], epochs=0, seed=STEP_SEED).fit(X)
    np.testing.assert_array_equal(shared.center_[:4], np.tile(np.array([0.5, -0.5], np.float32), (4, 1)))
    free = vgan_amd.SubspaceDeepSVDD(mask, np.full(5, 0.2), hidden=(33, 7), center_eps=0.0, epochs=0, seed=STEP_SEED).fit(X)
    for s in range(4):
        np.testing.assert_array_equal(_bits(free.center_[s]), _bits(two_level_mean(free.embed(X, s)).astype(np.float32)))
    assert not free.n_clamped_.any() and (np.abs(free.center_[3]) < 0.1).any()


# ---- 4. one step from the device's own state ------------------------------------------------------------------------------------------
def _step_setup(n, hidden, activation, seed=STEP_SEED):
    X = step_matrix(n)
    feats = step_features()
    dims = [len(f) for f in feats]
    mean, sd = restate_moments(X)
    assert sd[STEP_D] == 1.0 and sd[STEP_D + 1] == 1.0
    table = _table(feats)
    state, s_off, off = _device_init(table, dims, hidden, 0, len(dims), seed)
    skip = _dev(np.array([0, 0, 0, 0, 1], np.int32))
    z = restate_scaling(X, mean, sd)
    center = np.zeros((5, hidden[-1]), np.float32)
    for s in range(4):  # the restated centre of the untrained net: any fixed point serves a step
        center[s] = restate_center(z[:, feats[s]], restate_init(seed, s, dims[s], hidden), activation)[0]
    return dict(X=X, Xd=_dev(X), z=z, feats=feats, dims=dims, table=table, scaling=(_dev(mean), _dev(sd)), skip=skip, state=state, s_off=s_off,
                off=off, hidden=hidden, seed=seed, center=center, center_d=_dev(center))


def _train(c, activation, B, g0, steps, hp, loss, scratch=None):
    from vgan_amd.outlier import ae_bias_corrections
    corr = _dev(ae_bias_corrections(hp["beta1"], hp["beta2"], g0 + steps)[g0:])
    _ops().svdd_train(c["Xd"], c["table"], c["scaling"], c["skip"], (tuple(c["hidden"]), ACT[activation]), 0, len(c["dims"]), max(c["dims"]), B,
                      c["seed"], g0, corr, (hp["lr"], hp["beta1"], hp["beta2"], hp["eps"], hp["weight_decay"]), c["center_d"], c["state"],
                      c["s_off"], loss, scratch)


def _scratch_for(c, B):
    import torch
    from vgan_amd import outlier as o
    act = o.svdd_act_floats(max(c["dims"]), c["hidden"], B, True)
    return torch.empty(len(c["dims"]) * act, dtype=torch.float32, device="cuda") if act > o.AE_LDS_FLOATS else None


def _check_single_step(c, activation, B, g, hp, loss):
    """Runs the global step g alone and checks it from the state read before and after."""
    n = c["X"].shape[0]
    before = _blocks(c["state"], c["off"], c["dims"], c["hidden"])
    _train(c, activation, B, g, 1, hp, loss, _scratch_for(c, B))
    after = _blocks(c["state"], c["off"], c["dims"], c["hidden"])
    losses = loss.cpu().numpy()
    rows = batch_rows(g, n, B, c["seed"])
    worst = 0.0
    for s in range(4):
        z = c["z"][rows][:, c["feats"][s]]
        worst = max(worst, check_step(before[s], after[s], losses[s, g], z, c["center"][s], g + 1, hp, activation))
    for part_before, part_after in zip(before[4], after[4]):  # the constant subspace is untouched
        for a, b in zip(part_before, part_after):
            np.testing.assert_array_equal(_bits(a), _bits(b))
    assert losses[4, g] == 0.0
    return worst


@pytest.mark.parametrize("beta1", [0.0, 0.9])
@pytest.mark.parametrize("B", [1, 2, 31, 32, 33, 65])
def test_one_step_from_the_devices_own_state(B, beta1):
    """Subspaces of 1, 3, 33 and 70 features (the widest with a duplicated column) and a constant one; n = B, B + 1 and 2 B + 3 (at
    least 2 rows); steps 1 and 2 alone, steps 3 .. 5 in one launch, then step 6 alone; relu for even B, tanh for odd.  With beta1 =
    0 the checked m is the gradient itself."""
    import torch
    activation = "relu" if B % 2 == 0 else "tanh"
    hp = dict(DEFAULT_HP, beta1=beta1, weight_decay=1e-2)
    worst = 0.0
    for n in (B, B + 1, 2 * B + 3):
        if n < 2:
            continue
        c = _step_setup(n, STEP_HIDDEN, activation)
        loss = torch.full((5, 6), float("nan"), dtype=torch.float32, device="cuda")
        for g in (0, 1):
            worst = max(worst, _check_single_step(c, activation, B, g, hp, loss))
        _train(c, activation, B, 2, 3, hp, loss)
        worst = max(worst, _check_single_step(c, activation, B, 5, hp, loss))
        assert np.isfinite(loss.cpu().numpy()).all()
    print(f"B {B} beta1 {beta1} {activation}: worst err / bound {worst:.3f}")
    assert worst <= 1.0


def test_one_step_of_a_wide_net_with_the_batch_in_the_scratch_buffer():
    """B = 256 with hidden (128, 64, 2): the activations of the batch do not fit LDS; the same checks, and 1 + 1 steps equal 2."""
    import torch
    from vgan_amd import outlier as o
    hidden, B, n = (128, 64, 2), 256, 300
    assert o.svdd_act_floats(70, hidden, B, True) > o.AE_LDS_FLOATS
    hp = dict(DEFAULT_HP, weight_decay=1e-2)
    c = _step_setup(n, hidden, "tanh")
    loss = torch.zeros(5, 2, dtype=torch.float32, device="cuda")
    worst = max(_check_single_step(c, "tanh", B, g, hp, loss) for g in (0, 1))
    print(f"worst err / bound {worst:.3f}")
    assert worst <= 1.0
    twice = _step_setup(n, hidden, "tanh")
    loss2 = torch.zeros(5, 2, dtype=torch.float32, device="cuda")
    _train(twice, "tanh", B, 0, 2, hp, loss2, _scratch_for(twice, B))
    np.testing.assert_array_equal(_bits(twice["state"].cpu().numpy()), _bits(c["state"].cpu().numpy()))
    np.testing.assert_array_equal(_bits(loss2.cpu().numpy()), _bits(loss.cpu().numpy()))


# ---- 5. cut invariance and determinism ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("activation", ["relu", "tanh"])
def test_seven_steps_are_the_same_bits_for_every_cut_into_launches(activation):
    import torch
    B, n, hp = 33, 70, DEFAULT_HP
    results = []
    for cut in ((7,), (1,) * 7, (3, 4)):
        c = _step_setup(n, STEP_HIDDEN, activation)
        loss = torch.zeros(5, 7, dtype=torch.float32, device="cuda")
        g = 0
        for steps in cut:
            _train(c, activation, B, g, steps, hp, loss)
            g += steps
        results.append((c["state"].cpu().numpy(), loss.cpu().numpy()))
    for state, loss in results[1:]:
        np.testing.assert_array_equal(_bits(state), _bits(results[0][0]))
        np.testing.assert_array_equal(_bits(loss), _bits(results[0][1]))
    assert (results[0][1][:4] > 0).all()


CLASS_KW = dict(hidden=(5, 3), activation="tanh", epochs=3, batch_size=16, seed=7)


@functools.lru_cache(maxsize=None)
def _fitted():
    import vgan_amd
    X = step_matrix(70, seed=5)
    mask = _step_mask()
    return X, mask, vgan_amd.SubspaceDeepSVDD(mask, np.full(5, 0.2), **CLASS_KW).fit(X)


def test_class_is_bit_identical_for_every_workspace_and_run():
    import vgan_amd
    from vgan_amd import outlier as o
    X, mask, ens = _fitted()
    np.testing.assert_array_equal(ens.decision_function(X), ens.decision_scores_)  # bit for bit
    assert ens.n_steps_ == 3 * (70 // 16) and ens.loss_history_.shape == (5, 3) and ens.loss_history_.dtype == np.float64
    assert (ens.per_subspace_scores_[4] == 0.0).all() and (ens.loss_history_[4] == 0.0).all() and not ens.center_[4].any()  # the constant subspace
    assert (ens.per_subspace_scores_[:4] > 0.0).all()
    again = vgan_amd.SubspaceDeepSVDD(mask, np.full(5, 0.2), **CLASS_KW).fit(X)
    sizes = [o.svdd_net_bytes(d_s, (5, 3), 16, 70) for d_s in (1, 3, 33, 70, 2)]
    widest = max(sizes)
    tight = vgan_amd.SubspaceDeepSVDD(mask, np.full(5, 0.2), workspace_bytes=widest, **CLASS_KW).fit(X)
    chunks = o.ae_chunks(sizes, widest, "SubspaceDeepSVDD")
    assert (3, 1) in chunks and len(chunks) >= 3  # the widest net trains alone
    for other in (again, tight):
        np.testing.assert_array_equal(other.decision_scores_, ens.decision_scores_)
        np.testing.assert_array_equal(_bits(other.per_subspace_scores_), _bits(ens.per_subspace_scores_))
        np.testing.assert_array_equal(other.loss_history_, ens.loss_history_)
        np.testing.assert_array_equal(_bits(other.center_), _bits(ens.center_))
        np.testing.assert_array_equal(other.n_clamped_, ens.n_clamped_)
        for s in range(5):
            for W, Ww in zip(other.weights_[s], ens.weights_[s]):
                np.testing.assert_array_equal(_bits(W), _bits(Ww))
    with pytest.raises(ValueError, match=f"needs {widest} bytes of workspace"):
        vgan_amd.SubspaceDeepSVDD(mask, np.full(5, 0.2), workspace_bytes=widest - 1, **CLASS_KW).fit(X)
    # the class trains what the restatement trains: the losses of the epochs against the float64 run from the device's centre
    z = restate_scaling(X, ens.location_, ens.scale_)[:, mask[2]]
    _, losses = restate_fit(z, restate_init(7, 2, 33, (5, 3)), ens.center_[2], "tanh", 3, 16, 7, DEFAULT_HP)
    np.testing.assert_allclose(ens.loss_history_[2], losses.reshape(3, 4).mean(axis=1), rtol=1e-4)


# ---- 6. a short trajectory ---------------------------------------------------------------------------------------------------------------
def test_twelve_steps_stay_within_eight_yardsticks_of_the_float64_run():
    """d_s = 5, hidden (4, 2), B = 8, 12 steps from the restated centre: per weight within 8 x TRAJ_YARDSTICK (the measured deviation
    of the float32 emulation) of the float64 restatement."""
    import torch
    worst = 0.0
    for seed in TRAJ_SEEDS:
        X, z, p0 = traj_case(seed)
        mean, sd = restate_moments(X)
        center = restate_center(z, p0, TRAJ["activation"])[0]
        table = _table([np.arange(TRAJ["d_s"])])
        state, s_off, off = _device_init(table, [TRAJ["d_s"]], TRAJ["hidden"], 0, 1, seed)
        c = dict(Xd=_dev(X), table=table, scaling=(_dev(mean), _dev(sd)), skip=_dev(np.zeros(1, np.int32)), hidden=TRAJ["hidden"], dims=[TRAJ["d_s"]],
                 seed=seed, state=state, s_off=s_off, center_d=_dev(center[None, :]))
        loss = torch.zeros(1, TRAJ["steps"], dtype=torch.float32, device="cuda")
        _train(c, TRAJ["activation"], TRAJ["B"], 0, TRAJ["steps"], DEFAULT_HP, loss)
        got = _blocks(state, off, [TRAJ["d_s"]], TRAJ["hidden"])[0][0]
        p64, losses = restate_fit(z, p0, center, TRAJ["activation"], None, TRAJ["B"], seed, DEFAULT_HP, steps=TRAJ["steps"])
        worst = max(worst, max_weight_deviation(got, p64))
        np.testing.assert_allclose(loss.cpu().numpy()[0], losses, rtol=1e-4)
    print(f"worst per-weight deviation {worst:.3e}, allowed {8 * TRAJ_YARDSTICK:.3e}")
    assert worst <= 8 * TRAJ_YARDSTICK


# ---- 7. the recipes and the model route ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", ARC_SEEDS)
def test_arc_recipe_on_the_device(seed):
    """The AUC is within AUC_MARGIN of the restatement's recorded value and above every covariance AUC; the loss falls."""
    import vgan_amd
    X, y = arc_data(seed)
    ens = vgan_amd.SubspaceDeepSVDD(np.ones((1, 6), bool), [1.0], seed=seed, **ARC_NET).fit(X)
    ours = auc(ens.per_subspace_scores_[0].astype(np.float64), y)
    print(f"seed {seed}: device {ours:.4f}, restatement {ARC_AUC_SVDD[seed]:.4f}, covariance {ARC_AUC_COV[seed]:.4f}; "
          f"loss {ens.loss_history_[0, 0]:.4f} -> {ens.loss_history_[0, -1]:.6f}")
    assert abs(ours - ARC_AUC_SVDD[seed]) <= AUC_MARGIN and ours > max(ARC_AUC_COV.values())
    assert ens.loss_history_.shape == (1, 50) and ens.loss_history_[0, -1] < ens.loss_history_[0, 0]


@pytest.mark.parametrize("seed", RING_SEEDS)
def test_ring_recipe_on_the_device(seed):
    import vgan_amd
    X, y = ring(seed)
    ens = vgan_amd.SubspaceDeepSVDD(np.ones((1, 6), bool), [1.0], seed=seed, **RING_NET).fit(X)
    ours = auc(ens.per_subspace_scores_[0].astype(np.float64), y.astype(bool))
    print(f"seed {seed}: device {ours:.4f}, restatement {RING_AUC_SVDD[seed]:.4f}, covariance {RING_AUC_COV[seed]:.4f}; "
          f"loss {ens.loss_history_[0, 0]:.4f} -> {ens.loss_history_[0, -1]:.6f}")
    assert abs(ours - RING_AUC_SVDD[seed]) <= AUC_MARGIN and ours > max(RING_AUC_COV.values())
    assert ens.loss_history_.shape == (1, 50) and ens.loss_history_[0, -1] < ens.loss_history_[0, 0]


def test_model_route_and_shared_tail():
    import vgan_amd
    X, mask, ens = _fitted()
    proba = np.array([0.1, 0.2, 0.3, 0.25, 0.15])
    model = vgan_amd.VGAN.__new__(vgan_amd.VGAN)
    model.subspaces, model.proba = mask, proba
    tail = model.outlier_ensemble(method="deepsvdd", X=X, normalize="zscore", combination="max", contamination=0.2, **CLASS_KW)
    assert isinstance(tail, vgan_amd.SubspaceDeepSVDD)
    np.testing.assert_array_equal(_bits(tail.per_subspace_scores_), _bits(ens.per_subspace_scores_))  # the raw scores are the same
    Y = step_matrix(40, seed=6)
    got, per = tail.decision_function(Y, return_per_subspace=True)
    _check_scores(got, per, proba, tail.score_center_, tail.score_scale_, "max")
    assert tail.labels_.sum() == (tail.decision_scores_ > tail.threshold_).sum() and 0 < tail.labels_.sum() <= 0.2 * 70 + 1
    np.testing.assert_array_equal(tail.predict(Y), (got > tail.threshold_).astype(int))
    assert tail.predict_proba(Y).shape == (40, 2)
    plain = model.outlier_ensemble(method="deepsvdd", X=X, **CLASS_KW)
    got, per = plain.decision_function(Y, return_per_subspace=True)
    _check_scores(got, per, proba, None, None, "sum")
