"""Every schedule the step plan can select still computes what it computed before the plan was split from the allocator:
tests/golden/step_plan_traj.json holds, per variant, the loss bits of three steps (the first calibrates), the bandwidth bits and
the SHA-256 of the flat parameters, recorded by tools/record_step_plans.py --trajectories on an MI355X at the commit named in
the file -- eagerly and through the captured graph, each twice.  Every variant's two recordings were bit-identical, so every
variant is compared bit for bit."""
import importlib.util
import json
import os

import pytest

from conftest import GOLDEN, REPO

pytestmark = pytest.mark.gpu

_spec = importlib.util.spec_from_file_location("record_step_plans", os.path.join(REPO, "tools", "record_step_plans.py"))
rec = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(rec)

with open(os.path.join(GOLDEN, "step_plan_traj.json")) as _f:
    DOC = json.load(_f)
RECORDED = {v["name"]: v for v in DOC["variants"]}


def test_fixture_holds_every_variant_and_each_was_repeatable():
    assert list(RECORDED) == [v["name"] for v in rec.TRAJ_VARIANTS] and len(RECORDED) == 16
    for v in rec.TRAJ_VARIANTS:
        want = RECORDED[v["name"]]
        assert {k: want.get(k) for k in v} == json.loads(json.dumps(v))   # the variant is still what was recorded
        assert want["eager_repeatable"] and want["graph_repeatable"] and len(want["eager"]["loss_bits"]) == DOC["steps"] == 3


@pytest.mark.parametrize("how", ["eager", "graph"])
@pytest.mark.parametrize("variant", rec.TRAJ_VARIANTS, ids=[v["name"] for v in rec.TRAJ_VARIANTS])
def test_variant_reproduces_its_recorded_trajectory_bit_for_bit(variant, how):
    got = rec.run_trajectory(variant, use_graph=(how == "graph"))
    want = RECORDED[variant["name"]][how]
    print(variant["name"], how, got["losses"], want["losses"])
    assert got["loss_bits"] == want["loss_bits"]
    assert got["bw_bits"] == want["bw_bits"]
    assert got["params_sha256"] == want["params_sha256"]
