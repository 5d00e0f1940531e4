"""SHA-256 of the raw bytes of every output of the trained-MLP detectors (SubspaceAutoEncoder, SubspaceDeepSVDD), for comparing two
trees bit for bit on one GPU (profiles/mlp_core_hashes.txt).

  mlp_core_hashes.py --tree DIR --out FILE     one process per tree: `output | hash dtype[shape]` per line
  mlp_core_hashes.py --compare PARENT CHILD --out FILE [--parent-name NAME]
                                               one line per detector and setting, each differing output listed too

d = 64 with two columns held constant; subspaces of 1, 3, 17 and 33 varying features, all 64 features, and the two constant columns
alone (never trained, scores 0).  n fit rows and 70 new rows from a second seed, 3 epochs, every combination of hidden, activation,
batch_size and workspace_bytes (2^30, and the bytes of the largest single net, which cuts the nets into chunks).  Deep SVDD runs
each with the centre taken from the data (center_eps 0.1) and with a given [S, q] centre.  One spill case per class: d = 1024, one
subspace of all features, hidden (128, 128), batch 256, n = 300, 1 epoch: the training and the scoring kernel work in the scratch
buffer."""
import argparse
import hashlib
import itertools
import os
import sys

import numpy as np

D, CONSTANT, WIDTHS, NEW_ROWS, EPOCHS = 64, (5, 40), (1, 3, 17, 33), 70, 3
NS = (2, 33, 70)
HIDDEN = ((1,), (3, 2), (33, 7), (128, 64, 2))
ACTIVATIONS = ("relu", "tanh")
BATCHES = (1, 32, 256)
SPILL = {"d": 1024, "hidden": (128, 128), "batch": 256, "n": 300, "epochs": 1}


def digest(a):
    a = np.ascontiguousarray(a)
    return f"{hashlib.sha256(a.tobytes()).hexdigest()[:32]} {a.dtype}{list(a.shape)}"


def data(n, seed, d=D, constant=CONSTANT):
    X = np.random.default_rng(seed).normal(size=(n, d)).astype(np.float32)
    X[:, list(constant)] = np.float32(1.5)
    return X


def subspaces():
    rng = np.random.default_rng(7)
    varying = np.setdiff1d(np.arange(D), CONSTANT)
    mask = np.zeros((len(WIDTHS) + 2, D), bool)
    for s, w in enumerate(WIDTHS):
        mask[s, rng.choice(varying, w, replace=False)] = True
    mask[len(WIDTHS)] = True
    mask[len(WIDTHS) + 1, list(CONSTANT)] = True
    return mask


def outputs(ens, Xq, svdd):
    """(label, array) of everything a fitted detector publishes and returns"""
    flat = [w for layers in ens.weights_ for layer in layers for w in (layer if isinstance(layer, tuple) else (layer,))]
    outs = [("weights_", np.concatenate([w.ravel() for w in flat])), ("loss_history_", ens.loss_history_),
            ("per_subspace_scores_", ens.per_subspace_scores_), ("decision_scores_", ens.decision_scores_),
            ("decision_function", ens.decision_function(Xq)), ("location_", ens.location_), ("scale_", ens.scale_)]
    raw = ens.embed if svdd else ens.reconstruct
    outs += [(f"{raw.__name__}(Xq, {s})", raw(Xq, s)) for s in range(ens.plan.count)]
    if svdd:
        outs += [("center_", ens.center_), ("n_clamped_", ens.n_clamped_)]
    return outs


def run(out):
    import vgan_amd
    from vgan_amd import outlier as o
    print("hashing the outputs of", vgan_amd.lib.LIB_PATH, file=sys.stderr)
    mask = subspaces()
    S, dims = mask.shape[0], mask.sum(axis=1)
    proba = np.full(S, 1.0 / S)
    classes = (("ae", vgan_amd.SubspaceAutoEncoder, o.ae_net_bytes, False), ("svdd", vgan_amd.SubspaceDeepSVDD, o.svdd_net_bytes, True))
    for n in NS:
        X, Xq = data(n, 100 + n), data(NEW_ROWS, 200 + n)
        for hidden, activation, batch in itertools.product(HIDDEN, ACTIVATIONS, BATCHES):
            given = np.random.default_rng(300 + hidden[-1]).normal(size=(S, hidden[-1])).astype(np.float32)
            for name, cls, net_bytes, svdd in classes:
                single = max(net_bytes(int(d_s), hidden, min(batch, n), int(dims.max())) for d_s in dims)
                for ws, (mode, kw) in itertools.product((1 << 30, single), ((("data", {"center": None, "center_eps": 0.1}), ("given", {"center": given}))
                                                                            if svdd else (("-", {}),))):
                    ens = cls(mask, proba, hidden=hidden, activation=activation, batch_size=batch, epochs=EPOCHS, workspace_bytes=ws, **kw).fit(X)
                    head = f"{name} n={n} hidden={','.join(map(str, hidden))} {activation} batch={batch} ws={'2^30' if ws == 1 << 30 else 'net'} center={mode}"
                    for label, a in outputs(ens, Xq, svdd):
                        out.write(f"{head} {label} | {digest(a)}\n")
    d = SPILL["d"]
    X, Xq = data(SPILL["n"], 400, d, ()), data(NEW_ROWS, 401, d, ())
    for name, cls, _, svdd in classes:
        ens = cls(np.ones((1, d), bool), np.ones(1), hidden=SPILL["hidden"], batch_size=SPILL["batch"], epochs=SPILL["epochs"]).fit(X)
        for label, a in outputs(ens, Xq, svdd):
            out.write(f"{name} spill d={d} n={SPILL['n']} hidden={','.join(map(str, SPILL['hidden']))} relu batch={SPILL['batch']} {label} | {digest(a)}\n")


def compare(parent, child, out, parent_name):
    """One line per (detector, n, hidden, activation, workspace, centre): the SHA-256 over the per-output lines of its batch sizes,
    parent and child; an output that differs is also listed on its own."""
    rows = []
    for path in (parent, child):
        with open(path) as f:
            rows.append([line.rstrip("\n").split(" | ") for line in f if line.strip()])
    assert [r[0] for r in rows[0]] == [r[0] for r in rows[1]], "the two runs list different outputs"
    groups = {}
    for p, c in zip(*rows):
        words = p[0].split()
        at = next(i for i, w in enumerate(words) if w.startswith("batch="))
        head = " ".join(w for i, w in enumerate(words[:at + 3 if "spill" not in words else at + 1]) if i != at)
        g = groups.setdefault(head, {"batches": [], "lines": ([], [])})
        g["batches"] += [words[at][6:]] if words[at][6:] not in g["batches"] else []
        g["lines"][0].append(" | ".join(p))
        g["lines"][1].append(" | ".join(c))
    differ = [(p, c) for p, c in zip(*rows) if p[1] != c[1]]
    out.write(f"# SHA-256 (first 32 hex digits) of the raw bytes of every output of SubspaceAutoEncoder (ae) and SubspaceDeepSVDD (svdd), parent\n"
              f"# ({parent_name}) and this tree, one process each on one MI355X (tools/mlp_core_hashes.py).  d = {D}, columns {CONSTANT[0]} and {CONSTANT[1]}\n"
              f"# constant; subspaces of {', '.join(map(str, WIDTHS))} varying features, all {D} features, and the two constant columns alone (not trained,\n"
              f"# scores 0); fit rows n, {NEW_ROWS} new rows from a second seed, {EPOCHS} epochs; ws: workspace_bytes 2^30 or the bytes of the largest\n"
              f"# single net (the nets train in several chunks); center: taken from the data (center_eps 0.1) or a given [S, q] array.\n"
              f"# spill: d = {SPILL['d']}, one subspace of all features, hidden {SPILL['hidden']}, batch {SPILL['batch']}, n = {SPILL['n']}, {SPILL['epochs']} epoch: the training and\n"
              f"# the scoring kernel keep the activations in the scratch buffer.\n"
              f"# Outputs per fit: weights_ (flattened in order), loss_history_, per_subspace_scores_, decision_scores_, decision_function\n"
              f"# on the new rows, location_, scale_, reconstruct / embed of the new rows for every subspace, and center_, n_clamped_ (svdd).\n"
              f"# Every output is hashed on its own with its dtype and shape; a line below is the hash over those of one setting, all its\n"
              f"# batch sizes.  {len(rows[0])} outputs in {len(groups)} lines, {len(differ)} outputs differ.\n"
              f"# columns: detector and setting | batch sizes | outputs | parent | child\n")
    for head, g in groups.items():
        hp, hc = (hashlib.sha256("\n".join(lines).encode()).hexdigest()[:32] for lines in g["lines"])
        out.write(f"{head} | {','.join(g['batches'])} | {len(g['lines'][0])} | {hp} | {hc}{'' if hp == hc else '   [DIFF]'}\n")
    for p, c in differ:
        out.write(f"[DIFF] {p[0]} | {p[1]} | {c[1]}\n")
    return len(differ)


def main():
    ap = argparse.ArgumentParser(description=__doc__)
    ap.add_argument("--tree", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))), help="the tree whose vgan_amd runs")
    ap.add_argument("--compare", nargs=2, metavar=("PARENT", "CHILD"))
    ap.add_argument("--parent-name", default="parent")
    ap.add_argument("--out", required=True)
    args = ap.parse_args()
    with open(args.out, "w") as out:
        if args.compare:
            sys.exit(1 if compare(*args.compare, out, args.parent_name) else 0)
        sys.path.insert(0, os.path.abspath(args.tree))
        run(out)


if __name__ == "__main__":
    main()
