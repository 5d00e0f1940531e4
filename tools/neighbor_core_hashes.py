"""SHA-256 of the raw bytes of every output of the detectors on the refined neighbour lists (SubspaceABOD, SubspaceCOF with both
chains), for comparing two trees bit for bit on one GPU (profiles/neighbor_core_hashes.txt).

  neighbor_core_hashes.py --tree DIR --out FILE     one process per tree: `output | hash dtype[shape]` per line
  neighbor_core_hashes.py --compare PARENT CHILD --out FILE [--parent-name NAME]
                                                    one line per detector and setting, each differing output listed too

d = 256, five subspaces of 1, 3, 17, 33 and 200 features, n fit rows and 70 new rows from a second seed.  Data "normal": standard
normal float32.  Data "dup": integers 0 .. 2, so that the rows of the two narrow subspaces are duplicates of each other (degenerate
rows, the floor and the ceiling) while the wide ones stay distinct."""
import argparse
import hashlib
import os
import sys

import numpy as np

D, WIDTHS, NEW_ROWS = 256, (1, 3, 17, 33, 200), 70
NS = (3, 70, 301)
KS = (2, 8, 9, 16, 17, 32)
SETTINGS = [(ws, splits) for ws in (1 << 30, 1) for splits in (None, 1, 3)]
DUP_SETTINGS = [(1 << 30, None), (1, 3)]


def digest(a):
    a = np.ascontiguousarray(a)
    return f"{hashlib.sha256(a.tobytes()).hexdigest()[:32]} {a.dtype}{list(a.shape)}"


def data(kind, n, seed):
    rng = np.random.default_rng(seed)
    if kind == "dup":
        return rng.integers(0, 3, size=(n, D)).astype(np.float32)
    return rng.normal(size=(n, D)).astype(np.float32)


def run(out):
    import vgan_amd
    print("hashing the outputs of", vgan_amd.lib.LIB_PATH, file=sys.stderr)
    rng = np.random.default_rng(7)
    mask = np.zeros((len(WIDTHS), D), bool)
    for s, w in enumerate(WIDTHS):
        mask[s, rng.choice(D, w, replace=False)] = True
    proba = np.full(len(WIDTHS), 1.0 / len(WIDTHS))
    for kind in ("normal", "dup"):
        for n in NS:
            X, Xq = data(kind, n, 100 + n), data(kind, NEW_ROWS, 200 + n)
            for ws, splits in (SETTINGS if kind == "normal" else DUP_SETTINGS):
                for k in ((2,) if n == 3 else KS):
                    detectors = [("abod", vgan_amd.SubspaceABOD, {}, k)]
                    for chain in ("sbn", "rank"):
                        detectors += [(f"cof-{chain}", vgan_amd.SubspaceCOF, {"chain": chain}, kk) for kk in ((k,) if n == 3 or k != 2 else (1, 2))]
                    for name, cls, kw, kk in detectors:
                        ens = cls(mask, proba, n_neighbors=kk, splits=splits, workspace_bytes=ws, **kw).fit(X)
                        outs = [("per_subspace_scores_", ens.per_subspace_scores_), ("decision_scores_", ens.decision_scores_),
                                ("n_degenerate_", ens.n_degenerate_)]
                        if name == "abod":
                            outs.append(("score_floor_", ens.score_floor_))
                        else:
                            outs += [("ac_dist_", ens.ac_dist_), ("score_ceiling_", ens.score_ceiling_)]
                        outs.append(("decision_function", ens.decision_function(Xq)))
                        for label, (dist, idx) in (("kneighbors", ens.kneighbors()), ("kneighbors(Xq)", ens.kneighbors(Xq))):
                            outs += [(label + ".dist", dist), (label + ".idx", idx)]
                        for label, a in outs:
                            out.write(f"data={kind} n={n} ws={ws} splits={splits} {name} k={kk} {label} | {digest(a)}\n")


def compare(parent, child, out, parent_name):
    """One line per (data, n, ws, splits, detector): the SHA-256 over the per-output lines of all its k, parent and child; an
    output that differs is also listed on its own."""
    rows = []
    for path in (parent, child):
        with open(path) as f:
            rows.append([line.rstrip("\n").split(" | ") for line in f if line.strip()])
    assert [r[0] for r in rows[0]] == [r[0] for r in rows[1]], "the two runs list different outputs"
    groups = {}
    for p, c in zip(*rows):
        head, k = p[0].split(" k=")[0], p[0].split(" k=")[1].split()[0]
        g = groups.setdefault(head, {"ks": [], "lines": ([], [])})
        g["ks"] += [k] if k not in g["ks"] else []
        g["lines"][0].append(" | ".join(p))
        g["lines"][1].append(" | ".join(c))
    differ = [(p, c) for p, c in zip(*rows) if p[1] != c[1]]
    out.write(f"# SHA-256 (first 32 hex digits) of the raw bytes of every output of the detectors on the refined neighbour lists, parent\n"
              f"# ({parent_name}) and this tree, one process each on one MI355X (tools/neighbor_core_hashes.py).  d = {D}, five subspaces of\n"
              f"# {', '.join(map(str, WIDTHS))} features (engine auto), fit rows n, {NEW_ROWS} new rows from a second seed, splits and workspace_bytes\n"
              f"# (ws) as listed; n = 3 runs at k = 2.  data=dup: integer data 0 .. 2, whose rows in the two narrow subspaces are duplicates,\n"
              f"# so that the degenerate rows and the fill kernel (floor, ceiling, n_degenerate_) are hashed; data=normal has none.\n"
              f"# Outputs per fit: per_subspace_scores_, decision_scores_, n_degenerate_, score_floor_ (abod) or ac_dist_ and score_ceiling_\n"
              f"# (cof), decision_function on the new rows, kneighbors and kneighbors(new rows) as dist and idx.  Every output is hashed on\n"
              f"# its own with its dtype and shape; a line below is the hash over those of one detector at one setting, all its k.\n"
              f"# {len(rows[0])} outputs in {len(groups)} lines, {len(differ)} outputs differ.\n# columns: setting and detector | k | outputs | parent | child\n")
    for head, g in groups.items():
        hp, hc = (hashlib.sha256("\n".join(lines).encode()).hexdigest()[:32] for lines in g["lines"])
        out.write(f"{head} | {','.join(g['ks'])} | {len(g['lines'][0])} | {hp} | {hc}{'' if hp == hc else '   [DIFF]'}\n")
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
