"""Records what NoKLStepEngine decides and computes, through its public constructor and attribute reads only, so that the same
file runs unchanged on any commit.  Two fixtures come out of it (both are compared against by tests/test_step_plan*.py):

  --plans         (no GPU)  tests/golden/step_plans.json.gz (gzipped JSON, ~0.6 MB of text): for every case of `plan_cases()` the schedule decisions of the engine
                            built on the CPU stand-in, the shape / dtype / None-ness of every tensor attribute, or the error the
                            constructor raises.  Every case is recorded twice: on the stand-in as it is ("cpu") and on a
                            construct-only stand-in that declares HipOps's capabilities ("hip": bf3_rebuild, chain_ksplit, workspace
                            sizes from the library), which is what the MI355X product path decides.
  --trajectories  (MI355X)  tests/golden/step_plan_traj.json: for every variant of TRAJ_VARIANTS three steps (the first one
                            calibrates) eagerly and through the captured graph, each run twice: per-step loss bits, bandwidth bits
                            and the SHA-256 of the flat parameters after the last step.

    python tools/record_step_plans.py --plans [--out FILE]
    python tools/record_step_plans.py --trajectories [--out FILE]
"""
import argparse
import contextlib
import gzip
import hashlib
import json
import os
import struct
import subprocess
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.join(ROOT, "tests")):
    if _p not in sys.path:
        sys.path.insert(0, _p)
GOLDEN = os.path.join(ROOT, "tests", "golden")

# every schedule decision the step methods, bench.py and tools/ read from the engine
PLAN_ATTRS = ["mode", "exchange", "front_sharded", "fuse_update", "chain_flops", "fwd_split", "bwd_split", "precision", "bf3",
              "bwd_tile", "splits", "bsplits", "rm_backward", "fused_prepare", "chain_in_mask", "two_stage_logits", "gram_tile",
              "overlap", "x_ahead", "xx_ride", "xx_in_m4", "xx_late_in_backward", "n_main", "m4_kparts", "tn_kparts", "lean",
              "col_chunks", "nl", "lo", "dp", "e", "kp", "kn"]
WORKLOADS = {"c1": (128, 20), "c2": (512, 166), "c3": (1024, 784), "c4": (4096, 2048), "c5": (8192, 4096)}


@contextlib.contextmanager
def vgan_env(env):
    """Exactly `env` among the VGAN_* variables while the block runs; the caller's environment comes back afterwards."""
    saved = {k: v for k, v in os.environ.items() if k.startswith("VGAN_")}
    for k in saved:
        del os.environ[k]
    os.environ.update(env)
    try:
        yield
    finally:
        for k in [k for k in os.environ if k.startswith("VGAN_")]:
            del os.environ[k]
        os.environ.update(saved)


def hip_plan_ops():
    """The CPU stand-in with HipOps's capabilities declared: good for CONSTRUCTING an engine (no step runs on it)."""
    from cpu_ops import CpuOps
    import vgan_amd
    import ctypes
    _lib = vgan_amd.lib

    class HipPlanOps(CpuOps):
        name = "cpu stand-in with HipOps's capabilities (construction only)"
        bf3_rebuild = True
        chain_ksplit = True

        def linear_backward_params_ksplit_ws_bytes(self, kin, out, parts):
            return int(self.lib.vgan_linear_backward_params_ksplit_ws_bytes(int(kin), int(out), int(parts)))

        def ksplit_workspace(self, nbytes, device=None):
            return torch.zeros(max(int(nbytes), 16) // 4 + 4, dtype=torch.int32)

        def gemm_grouped_ksplit_ws_bytes(self, problems, kparts):
            arr = (_lib.GemmProblem * len(problems))()
            for q, (kind, A, B, C) in zip(arr, problems):
                assert kind == "TN"
                (k, m), (k2, n) = A.shape, B.shape
                assert k == k2 and tuple(C.shape) == (m, n)
                q.a, q.b, q.c, q.kind, q.m, q.n, q.k = A.data_ptr(), B.data_ptr(), C.data_ptr(), _lib.GEMM_TN, m, n, k
                q.lda, q.ldb, q.ldc, q.splitk = A.stride(0), B.stride(0), C.stride(0), 1
            kp = (ctypes.c_int32 * len(problems))(*[int(v) for v in kparts])
            return int(self.lib.vgan_gemm_grouped_ksplit_ws_bytes(arr, len(problems), kp))

    return HipPlanOps()


# ---- plans -----------------------------------------------------------------------------------------------------------
def plan_cases():
    """[{name, n, d, world, rank, kwargs, env}]: the workloads, their 1/8 shards, every constructor option, every knob moved off
    its default one at a time, the shapes the existing tests force and the edge shapes where a rule flips."""
    cases = []

    def add(name, n, d, world=1, rank=0, kwargs=None, env=None):
        cases.append(dict(name=name, n=n, d=d, world=world, rank=rank, kwargs=kwargs or {}, env=env or {}))

    for w, (n, d) in WORKLOADS.items():
        add(w, n, d)
        for rank in (0, 3, 7):
            add(f"{w}/dp8r{rank}", n, d, 8, rank)
    options = [("layered", dict(generator_mode="layered")), ("fp32", dict(mmd_precision="fp32")), ("bf16x3", dict(mmd_precision="bf16x3")),
               ("exchange", dict(force_exchange=True)), ("replicated", dict(front="replicated", force_exchange=True)),
               ("sharded", dict(front="sharded", force_exchange=True)), ("sharded-no-exchange", dict(front="sharded")),
               ("sharded-layered", dict(front="sharded", force_exchange=True, generator_mode="layered")),
               ("overlap", dict(overlap_exchange=True)), ("overlap-serial", dict(overlap_exchange="serial")),
               ("overlap-off", dict(overlap_exchange=False)), ("overlap-sharded", dict(overlap_exchange=True, front="sharded", force_exchange=True)),
               ("fuse", dict(fuse_update=True)), ("fuse-off", dict(fuse_update=False)), ("fuse-flops", dict(fuse_update=True, chain_assoc="flops")),
               ("depth", dict(chain_assoc="depth")), ("flops", dict(chain_assoc="flops")),
               ("bad-mode", dict(generator_mode="wide")), ("bad-front", dict(front="both")), ("bad-assoc", dict(chain_assoc="breadth")),
               ("bad-precision", dict(mmd_precision="fp16")), ("overlap-fp32", dict(overlap_exchange=True, mmd_precision="fp32")),
               ("layered-bf16x3-overlap", dict(generator_mode="layered", mmd_precision="bf16x3", overlap_exchange=True))]
    for w in ("c1", "c3", "c4"):
        for name, kw in options:
            add(f"{w}/{name}", *WORKLOADS[w], kwargs=kw)
    for name, kw in options[:8]:
        add(f"c4/dp8r3/{name}", *WORKLOADS["c4"], 8, 3, kwargs=kw)
    knobs = {"VGAN_GENERATOR": ["layered", "wide"], "VGAN_FUSE_UPDATE": ["1", "true"], "VGAN_DP_FRONT": ["replicated", "sharded", "both"],
             "VGAN_CHAIN_ASSOC": ["depth", "flops", "breadth"], "VGAN_CHAIN_SPLITK": ["0"], "VGAN_MMD_PRECISION": ["fp32", "bf16x3", "fp16"],
             "VGAN_BWD_TILE": ["64", "128", "256", "wide"], "VGAN_BWD_OPERAND": ["transposed"], "VGAN_BWD_SPLITS": ["0", "1", "3"],
             "VGAN_FUSED_PREPARE": ["0"], "VGAN_CHAIN_IN_MASK": ["1"], "VGAN_LOGITS_2STAGE": ["1"], "VGAN_GRAM_TILE": ["64", "128", "256", "32"],
             "VGAN_GRAM_TAIL": ["0"], "VGAN_RS_FROM_GRAM": ["0"], "VGAN_OVERLAP": ["1", "0", "serial"], "VGAN_XX_RIDE": ["1"],
             "VGAN_XX_IN_M4": ["0"], "VGAN_GRAM_SLOTS": ["30", "400", "520"], "VGAN_XX_LATE": ["m4"], "VGAN_CHAIN_KPARTS": ["1", "2", "4", "8", "3"],
             "VGAN_Z_FP32": ["1"]}
    for var, values in knobs.items():
        for v in values:
            for w in ("c1", "c3", "c4"):
                add(f"{w}/{var}={v}", *WORKLOADS[w], env={var: v})
            add(f"c1/bf16x3/{var}={v}", *WORKLOADS["c1"], kwargs=dict(mmd_precision="bf16x3"), env={var: v})
            add(f"c4/dp8r3/{var}={v}", *WORKLOADS["c4"], 8, 3, env={var: v})
            add(f"c3/flops/{var}={v}", *WORKLOADS["c3"], kwargs=dict(chain_assoc="flops"), env={var: v})
    # the shapes tests/test_host_logic.py forces
    for late in ("backward", "m4"):
        for in_m4 in ("1", "0"):
            add(f"n256d20/slots30/late={late}/in_m4={in_m4}", 256, 20, kwargs=dict(mmd_precision="bf16x3"),
                env={"VGAN_GRAM_SLOTS": "30", "VGAN_XX_LATE": late, "VGAN_XX_IN_M4": in_m4})
    add("n128d96/kparts4", 128, 96, env={"VGAN_CHAIN_KPARTS": "4"})
    add("n256d20/bf16x3/tile256", 256, 20, kwargs=dict(mmd_precision="bf16x3"), env={"VGAN_GRAM_TILE": "256"})
    # edges where a rule flips
    for prec in ("fp32", "bf16x3"):
        add(f"d21/{prec}", 128, 21, kwargs=dict(mmd_precision=prec))
        add(f"n192/{prec}", 192, 20, kwargs=dict(mmd_precision=prec))
        add(f"n100/{prec}", 100, 20, kwargs=dict(mmd_precision=prec))
        for n in (128, 256):
            for tile in ("128", "256"):
                add(f"n{n}/{prec}/tile{tile}", n, 20, kwargs=dict(mmd_precision=prec), env={"VGAN_GRAM_TILE": tile})
                add(f"n{n}/{prec}/tile{tile}/dp2r1", n, 20, 2, 1, kwargs=dict(mmd_precision=prec), env={"VGAN_GRAM_TILE": tile})
    add("d21/bf16x3/ride+mask", 128, 21, kwargs=dict(mmd_precision="bf16x3"), env={"VGAN_XX_RIDE": "1", "VGAN_CHAIN_IN_MASK": "1"})
    add("c3/ride+in_m4", *WORKLOADS["c3"], env={"VGAN_XX_RIDE": "1"})
    add("c3/mask+2stage", *WORKLOADS["c3"], env={"VGAN_CHAIN_IN_MASK": "1", "VGAN_LOGITS_2STAGE": "1"})
    add("c3/no-prepare+mask", *WORKLOADS["c3"], env={"VGAN_CHAIN_IN_MASK": "1", "VGAN_FUSED_PREPARE": "0"})
    add("c3/transposed+overlap", *WORKLOADS["c3"], kwargs=dict(overlap_exchange=True), env={"VGAN_BWD_OPERAND": "transposed"})
    add("c3/transposed+slots", *WORKLOADS["c3"], env={"VGAN_BWD_OPERAND": "transposed", "VGAN_GRAM_SLOTS": "400"})
    add("c3/bwd-tile128+slots", *WORKLOADS["c3"], env={"VGAN_BWD_TILE": "128", "VGAN_GRAM_SLOTS": "400"})
    add("c4/sharded+transposed", *WORKLOADS["c4"], 8, 3, env={"VGAN_BWD_OPERAND": "transposed"})
    add("c5/dp8r3/tile128", *WORKLOADS["c5"], 8, 3, env={"VGAN_GRAM_TILE": "128"})
    add("c5/dp8r3/tile64", *WORKLOADS["c5"], 8, 3, env={"VGAN_GRAM_TILE": "64"})
    add("c5/dp8r3/fp32", *WORKLOADS["c5"], 8, 3, kwargs=dict(mmd_precision="fp32"))
    add("c5/dp8r3/no-tail", *WORKLOADS["c5"], 8, 3, env={"VGAN_GRAM_TAIL": "0"})
    add("n100/dp8", 100, 20, 8, 0)
    add("n1000/dp3r2", 1000, 20, 3, 2)
    add("n1026/dp3r2", 1026, 20, 3, 2)
    assert len({c["name"] for c in cases}) == len(cases)
    return cases


def build_engine(case, ops):
    """The case's engine through the public constructor (zero data: no decision reads a value)."""
    from vgan_amd.modules import Generator_big
    from vgan_amd.synth import latent_size
    from vgan_amd.trainer import NoKLStepEngine
    n, d = case["n"], case["d"]
    with vgan_env(case["env"]):
        gen = Generator_big(latent_size(d), d)
        return NoKLStepEngine(ops, gen, torch.zeros(n, d), n, 2, noise="host", rank=case["rank"], world=case["world"], **case["kwargs"])


def _plain(v):
    if isinstance(v, dict):
        return {str(k): _plain(x) for k, x in v.items()}
    if isinstance(v, (list, tuple)):
        return [_plain(x) for x in v]
    return v


def _tensor_entry(v):
    if v is None:
        return None
    return str(v.dtype).replace("torch.", "") + str(list(v.shape)).replace(" ", "")  # e.g. "float32[128,20]"


def describe_engine(eng):
    """(decisions, tensors) of a constructed engine, as JSON-ready values."""
    plan = {a: _plain(getattr(eng, a)) for a in PLAN_ATTRS if hasattr(eng, a)}
    plan["gram_tail"] = eng.gram_tail_ws is not None
    plan["rs_from_gram"] = eng.rs_part is not None
    plan["n_tiles"] = int(eng.tiles.shape[0])
    plan["tiles_sha"] = hashlib.sha256(eng.tiles.contiguous().numpy().tobytes()).hexdigest()[:16]
    plan["cal_shares_tiles"] = eng.tiles_cal is eng.tiles
    tensors = {}
    for name, v in vars(eng).items():
        if v is None or isinstance(v, torch.Tensor):
            tensors[name] = _tensor_entry(v)
        elif isinstance(v, (list, tuple)) and v and all(x is None or isinstance(x, torch.Tensor) for x in v):
            tensors[name] = [_tensor_entry(x) for x in v]
    return plan, tensors


def record_case(case, ops):
    try:
        eng = build_engine(case, ops)
    except Exception as e:  # noqa: BLE001 -- the error IS the record
        return {"error": [type(e).__name__, str(e)]}
    plan, tensors = describe_engine(eng)
    return {"plan": plan, "tensors": tensors}


def git_head():
    try:
        return subprocess.run(["git", "-C", ROOT, "rev-parse", "HEAD"], capture_output=True, text=True, check=True).stdout.strip()
    except Exception:  # noqa: BLE001
        return None


def record_plans(out, commit=None):
    """The file keeps every distinct table of tensor attributes once (`tensor_sets`; a record holds its index), and writes
    "=cpu" for a "hip" record equal to the "cpu" one."""
    from cpu_ops import CpuOps
    providers = {"cpu": CpuOps(), "hip": hip_plan_ops()}
    records, tensor_sets, index = [], [], {}
    for case in plan_cases():
        rec = dict(case)
        for key, ops in providers.items():
            r = record_case(case, ops)
            if "tensors" in r:
                sig = json.dumps(r["tensors"], sort_keys=True)
                if sig not in index:
                    index[sig] = len(tensor_sets)
                    tensor_sets.append(r["tensors"])
                r["tensors"] = index[sig]
            rec[key] = r
        if rec["hip"] == rec["cpu"]:
            rec["hip"] = "=cpu"
        records.append(rec)
        print(case["name"], {k: ("error" if "error" in rec[k] else "ok") for k in providers}, flush=True)
    text = ('{"recorded_at_commit": %s,\n"plan_attrs": %s,\n"cases": [\n' % (json.dumps(commit or git_head()), json.dumps(PLAN_ATTRS)) +
            ",\n".join(json.dumps(r, sort_keys=True, separators=(",", ":")) for r in records) + '\n],\n"tensor_sets": [\n' +
            ",\n".join(json.dumps(t, sort_keys=True, separators=(",", ":")) for t in tensor_sets) + "\n]}\n")
    with open(out, "wb") as f, gzip.GzipFile(fileobj=f, mode="wb", filename="", mtime=0) as z:  # (no name, no time: same bytes every run)
        z.write(text.encode())


def load_plans(path=None):
    """The records of step_plans.json.gz with the two space savers undone."""
    with gzip.open(path or os.path.join(GOLDEN, "step_plans.json.gz"), "rt") as f:
        doc = json.load(f)
    for rec in doc["cases"]:
        if rec["hip"] == "=cpu":
            rec["hip"] = rec["cpu"]
        for key in ("cpu", "hip"):
            if "tensors" in rec[key] and isinstance(rec[key]["tensors"], int):
                rec[key] = dict(rec[key], tensors=doc["tensor_sets"][rec[key]["tensors"]])
    return doc


# ---- trajectories ----------------------------------------------------------------------------------------------------
TRAJ_VARIANTS = [
    dict(name="fp32", n=128, d=20),
    dict(name="layered", n=128, d=20, kwargs=dict(generator_mode="layered")),
    dict(name="bf16x3", n=128, d=20, kwargs=dict(mmd_precision="bf16x3")),
    dict(name="bf16x3-z-fp32", n=128, d=20, kwargs=dict(mmd_precision="bf16x3"), env={"VGAN_Z_FP32": "1"}),
    dict(name="bf16x3-xx-ride", n=128, d=20, kwargs=dict(mmd_precision="bf16x3"), env={"VGAN_XX_RIDE": "1"}),
    dict(name="chain-in-mask", n=128, d=20, env={"VGAN_CHAIN_IN_MASK": "1"}),
    dict(name="logits-2stage", n=128, d=20, env={"VGAN_LOGITS_2STAGE": "1"}),
    dict(name="fuse-update", n=128, d=20, kwargs=dict(fuse_update=True)),
    dict(name="overlap", n=128, d=20, kwargs=dict(overlap_exchange=True)),
    dict(name="chain-flops", n=128, d=20, kwargs=dict(chain_assoc="flops")),
    dict(name="bf16x3-gram-tile-128", n=128, d=20, kwargs=dict(mmd_precision="bf16x3"), env={"VGAN_GRAM_TILE": "128"}),
    dict(name="bf16x3-transposed", n=128, d=20, kwargs=dict(mmd_precision="bf16x3"), env={"VGAN_BWD_OPERAND": "transposed"}),
    dict(name="slots30-late-backward", n=256, d=20, kwargs=dict(mmd_precision="bf16x3"), env={"VGAN_GRAM_SLOTS": "30", "VGAN_XX_LATE": "backward"}),
    dict(name="slots30-late-m4", n=256, d=20, kwargs=dict(mmd_precision="bf16x3"), env={"VGAN_GRAM_SLOTS": "30", "VGAN_XX_LATE": "m4"}),
    dict(name="bf16x3-gram-tile-256", n=256, d=20, kwargs=dict(mmd_precision="bf16x3"), env={"VGAN_GRAM_TILE": "256"}),
    dict(name="d96-chain-kparts-4", n=128, d=96, env={"VGAN_CHAIN_KPARTS": "4"}),
]
TRAJ_STEPS = 3


def _traj_inputs(d):
    """Data and generator parameters: fixture f3 (c1) as it is at d = 20; at another width the fixture's columns repeated with
    a per-column scale, and the synthetic initialisation of that width."""
    from vgan_amd.synth import synthetic_generator_params
    g = np.load(os.path.join(GOLDEN, "f3_traj_c1.npz"), allow_pickle=False)
    data = g["data"]
    if d == data.shape[1]:
        return data, [g[f"param0_{i}"] for i in range(8)]
    reps = -(-d // data.shape[1])
    wide = np.tile(data, (1, reps))[:, :d] * (1.0 + 0.01 * np.arange(d, dtype=np.float32))[None, :]
    return np.ascontiguousarray(wide.astype(np.float32)), synthetic_generator_params(d)


def _bits(x):
    return struct.unpack("<I", struct.pack("<f", float(x)))[0]


def run_trajectory(variant, use_graph, ops=None, device="cuda"):
    """Three steps of one variant on `device`: {"loss_bits": [..], "bw_bits": .., "params_sha256": ..}."""
    from vgan_amd.modules import Generator_big
    from vgan_amd.ops import HipOps
    from vgan_amd.synth import latent_size
    from vgan_amd.trainer import NoKLStepEngine
    n, d = variant["n"], variant["d"]
    data, params = _traj_inputs(d)
    table = np.stack([np.random.default_rng(11 + b).permutation(data.shape[0])[:n] for b in range(TRAJ_STEPS)])
    with vgan_env(variant.get("env", {})):
        gen = Generator_big(latent_size(d), d)
        with torch.no_grad():
            for q, v in zip(gen.parameters(), params):
                q.copy_(torch.as_tensor(v))
        eng = NoKLStepEngine(ops or HipOps(), gen.to(device), torch.as_tensor(data).to(device), n, TRAJ_STEPS, seed=777, noise="device",
                             use_graph=use_graph, loss_accum_scale=1.0, **variant.get("kwargs", {}))
        eng.set_epoch_batches(torch.as_tensor(table.astype(np.int64)))
        losses = []
        for _ in range(TRAJ_STEPS):
            eng.step()
            losses.append(_bits(eng.step_loss()))
        if use_graph and device != "cpu":
            assert eng.graph is not None, "the step was not captured"
        flat = eng.fp.flat.detach().cpu().contiguous().numpy()
        return {"loss_bits": losses, "bw_bits": _bits(eng.bw.cpu()[0]), "params_sha256": hashlib.sha256(flat.tobytes()).hexdigest(),
                "losses": [struct.unpack("<f", struct.pack("<I", b))[0] for b in losses]}


def record_trajectories(out, commit=None):
    assert torch.cuda.is_available(), "--trajectories needs an MI355X"
    records = []
    for variant in TRAJ_VARIANTS:
        rec = dict(variant)
        for key, use_graph in (("eager", False), ("graph", True)):
            runs = [run_trajectory(variant, use_graph) for _ in range(2)]
            rec[key] = runs[0]
            rec[key + "_repeatable"] = runs[0] == runs[1]
            if runs[0] != runs[1]:
                rec[key + "_second_run"] = runs[1]
        records.append(rec)
        print(variant["name"], {k: rec[k + "_repeatable"] for k in ("eager", "graph")}, rec["eager"]["losses"], flush=True)
        with open(out, "w") as f:  # (kept current after every variant)
            f.write('{"recorded_at_commit": %s, "steps": %d, "variants": [\n' % (json.dumps(commit or git_head()), TRAJ_STEPS))
            f.write(",\n".join(json.dumps(r, sort_keys=True) for r in records) + "\n]}\n")  # one variant per line


if __name__ == "__main__":
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--plans", action="store_true")
    ap.add_argument("--trajectories", action="store_true")
    ap.add_argument("--out", default=None)
    ap.add_argument("--commit", default=None, help="hash to record (default: git HEAD; for a tree without its .git)")
    args = ap.parse_args()
    if args.plans:
        record_plans(args.out or os.path.join(GOLDEN, "step_plans.json.gz"), args.commit)
    if args.trajectories:
        record_trajectories(args.out or os.path.join(GOLDEN, "step_plan_traj.json"), args.commit)
