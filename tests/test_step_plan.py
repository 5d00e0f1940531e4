"""The step engine's decision table (v-gan_amd/step_plan.py) against tests/golden/step_plans.json.gz, which
tools/record_step_plans.py recorded from the engine BEFORE the plan was split from the allocator (commit in the file): for every
workload, 1/8 shard, constructor option, knob and edge shape, on the CPU stand-in and on a stand-in with HipOps's capabilities."""
import dataclasses
import hashlib
import importlib.util
import inspect
import os

import pytest
import torch

from conftest import REPO
from cpu_ops import CpuOps

_spec = importlib.util.spec_from_file_location("record_step_plans", os.path.join(REPO, "tools", "record_step_plans.py"))
rec = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(rec)

DOC = rec.load_plans()
CASES = DOC["cases"]
PROVIDERS = {"cpu": CpuOps, "hip": rec.hip_plan_ops}
_ops = {}


def provider(key):
    if key not in _ops:
        _ops[key] = PROVIDERS[key]()
    return _ops[key]


def plan_of(case, ops, knobs=None):
    """plan_step for a recorded case, without an engine: the constructor's arguments, the knobs of the case's environment."""
    from vgan_amd.step_plan import Knobs, plan_step
    from vgan_amd.synth import latent_size
    n, d = case["n"], case["d"]
    L = latent_size(d)
    kw = dict(force_exchange=False, generator_mode=None, mmd_precision=None, overlap_exchange=None, fuse_update=None, front=None,
              chain_assoc=None)
    kw.update(case["kwargs"])
    if knobs is None:
        knobs = Knobs.from_env(case["env"])
    return plan_step(ops, n=n, d=d, data_stride=d, latent=L, widths=[L, 2 * L, 4 * L, 8 * L, d], world=case["world"], rank=case["rank"],
                     knobs=knobs, **kw)


def check_plan(plan, want, ops, case):
    got = rec._plain(dataclasses.asdict(plan))
    for name, value in want.items():
        if name == "tiles_sha":  # the table the allocator builds from the plan is the recorded one
            table = ops.build_tiles(case["n"], 1, case["rank"], case["world"], device="cpu", tile=plan.gram_tile, split=plan.tile_split)
            table = table[0] if plan.tile_split else table
            assert hashlib.sha256(table.contiguous().numpy().tobytes()).hexdigest()[:16] == value, (case["name"], name)
        else:
            assert got[name] == value, (case["name"], name, got[name], value)


def test_fixture_covers_what_it_must():
    assert len(DOC["recorded_at_commit"]) == 40
    names = {c["name"] for c in CASES}
    for w in ("c1", "c2", "c3", "c4", "c5"):
        assert {w, f"{w}/dp8r0", f"{w}/dp8r3", f"{w}/dp8r7"} <= names
    from vgan_amd.step_plan import Knobs
    variables = {k for c in CASES for k in c["env"]}
    assert len(variables) == len(dataclasses.fields(Knobs)) == 22   # every knob is moved off its default somewhere
    assert variables == {f.metadata["var"] for f in dataclasses.fields(Knobs)} and Knobs() == Knobs.from_env({})
    by_name = {c["name"]: c for c in CASES}
    hip_c3 = by_name["c3"]["hip"]["plan"]   # what the MI355X product path decides at c3 (the CPU stand-in lacks both capabilities)
    assert (hip_c3["lean"], hip_c3["m4_kparts"], hip_c3["tn_kparts"]) == (True, 4, 4)
    assert (by_name["c3"]["cpu"]["plan"]["lean"], by_name["c3"]["cpu"]["plan"]["m4_kparts"]) == (False, 1)
    assert sum("error" in c["cpu"] for c in CASES) >= 20


@pytest.mark.parametrize("key", ["cpu", "hip"])
def test_plan_step_returns_every_recorded_decision_without_an_engine(key, monkeypatch):
    for var in [v for v in os.environ if v.startswith("VGAN_")]:
        monkeypatch.delenv(var)
    ops = provider(key)
    for case in CASES:
        want = case[key]
        if "error" in want:
            with pytest.raises(Exception) as err:
                plan_of(case, ops)
            assert [type(err.value).__name__, str(err.value)] == want["error"], case["name"]
        else:
            check_plan(plan_of(case, ops), want["plan"], ops, case)


def test_explicit_knobs_ignore_the_environment(monkeypatch):
    """plan_step reads no environment: with a Knobs in hand, contradictory VGAN_* variables change nothing."""
    from vgan_amd.step_plan import Knobs
    by_name = {c["name"]: c for c in CASES}
    cases = [by_name[k] for k in ("c3", "c4/dp8r3", "c3/VGAN_XX_RIDE=1", "c1/VGAN_GENERATOR=layered", "n256d20/slots30/late=m4/in_m4=1")]
    knobs = [Knobs.from_env(c["env"]) for c in cases]
    contrary = {"VGAN_GENERATOR": "wide", "VGAN_FUSE_UPDATE": "1", "VGAN_DP_FRONT": "replicated", "VGAN_CHAIN_ASSOC": "flops",
                "VGAN_CHAIN_SPLITK": "0", "VGAN_MMD_PRECISION": "fp32", "VGAN_BWD_TILE": "wide", "VGAN_BWD_OPERAND": "transposed",
                "VGAN_BWD_SPLITS": "7", "VGAN_FUSED_PREPARE": "0", "VGAN_CHAIN_IN_MASK": "1", "VGAN_LOGITS_2STAGE": "1", "VGAN_GRAM_TILE": "64",
                "VGAN_GRAM_TAIL": "0", "VGAN_RS_FROM_GRAM": "0", "VGAN_OVERLAP": "1", "VGAN_XX_RIDE": "0", "VGAN_XX_IN_M4": "0",
                "VGAN_GRAM_SLOTS": "1", "VGAN_XX_LATE": "m4", "VGAN_CHAIN_KPARTS": "3", "VGAN_Z_FP32": "1"}
    for var, value in contrary.items():
        monkeypatch.setenv(var, value)
    for key in PROVIDERS:
        for case, k in zip(cases, knobs):
            check_plan(plan_of(case, provider(key), knobs=k), case[key]["plan"], provider(key), case)


def test_side_stream_follows_the_overlap_argument():
    """(`_side` needs a HIP device, so the recorded CPU engines never had one: the rule is stated here.)"""
    c3 = next(c for c in CASES if c["name"] == "c3")
    for overlap, want in [(None, False), (False, False), (True, True), ("serial", False)]:
        plan = plan_of(dict(c3, kwargs=dict(overlap_exchange=overlap)), provider("cpu"))
        assert plan.side_stream is want and plan.overlap is (overlap is not None and bool(overlap))


@pytest.mark.parametrize("key", ["cpu", "hip"])
def test_engine_has_the_recorded_decisions_and_buffers(key):
    """Every engine of the fixture up to n = 1024, built now: the recorded attribute values, and the recorded shape, dtype and
    None-ness of every tensor attribute, with nothing missing."""
    ops = provider(key)
    built = 0
    for case in CASES:
        if case["n"] > 1024:
            continue
        want = case[key]
        if "error" in want:
            with pytest.raises(Exception) as err:
                rec.build_engine(case, ops)
            assert [type(err.value).__name__, str(err.value)] == want["error"], case["name"]
            continue
        plan, tensors = rec.describe_engine(rec.build_engine(case, ops))
        wrong = {k: (plan.get(k, "<missing>"), v) for k, v in want["plan"].items() if plan.get(k, "<missing>") != v}
        assert not wrong, (case["name"], wrong)
        missing = {k: v for k, v in want["tensors"].items() if k not in tensors or tensors[k] != v}
        assert not missing, (case["name"], {k: (tensors.get(k, "<missing>"), v) for k, v in missing.items()})
        built += 1
    assert built >= 150


def test_constructor_reads_no_environment():
    from vgan_amd import step_plan
    from vgan_amd.trainer import NoKLStepEngine
    assert "environ" not in inspect.getsource(NoKLStepEngine.__init__)
    assert "environ" not in inspect.getsource(step_plan.plan_step)
    eng = rec.build_engine(dict(n=128, d=20, world=1, rank=0, kwargs={}, env={}), provider("cpu"))
    assert isinstance(eng.plan, step_plan.StepPlan) and isinstance(eng.tiles, torch.Tensor)
    with pytest.raises(dataclasses.FrozenInstanceError):
        eng.plan.lean = True
