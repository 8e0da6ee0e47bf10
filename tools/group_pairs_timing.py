"""Per-frame cost of the group-pair interaction energy matrix over a stored trajectory: snb_evaluate_group_pair_energies against the only
route the parent commit has, one subset per group.

    python tools/group_pairs_timing.py --baseline-tree DIR [--configs c3,c2] [--frames 200] [--repeats 3] [--rounds 2] [--limit SECONDS]

Frames: the bench workload of the config and F - 1 seeded Gaussian perturbations of 0.02 nm of it, resident on the device, in the
config's precision; constant box.

  leg A   the parent commit: an engine with n_subsets = 8 whose subsets ARE an 8-label partition (every solute blob one label, the solvent
          cut into slabs along x by molecule), snb_evaluate_frames with include_reciprocal = 0, every slice, device output.  It uses only
          entry points of the PARENT commit and runs as a child process on a built tree of that commit (--baseline-tree: `git archive` of
          the parent, built beforehand), because the binding checks every declared symbol against the library it loads.
  leg B   snb_evaluate_group_pair_energies of this tree with the same 8 labels on an engine with the config's OWN subsets, with device
          output (call + snb_synchronize) and with host output.
  leg C   the same call with a residue-like labelling: the solute in about 300 runs of consecutive atoms, the solvent as one group.  The
          parent commit has no route to it (an engine with 300 subsets): a figure only.

Legs alternate A / B / C / A / B / C, one fresh child process per leg, each under its own time limit; the chain ends at the first
failure.  A child prints one JSON line per variant with the per-frame wall time of every repeat; the parent prints the medians and the
spread (max - min) of the repeats and appends one aggregate line per config to profiles/group_pairs_timing.jsonl.

    python tools/group_pairs_timing.py --leg A|B|C --tree DIR --config c3 ...      (what a child runs)
"""
import argparse
import ctypes
import json
import os
import subprocess
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
TAG = "GROUP_PAIRS_TIMING "


def labels8(w):
    """An 8-label partition of a bench workload: every solute subset (a blob) one label, the solvent (subset 0, molecules of 3 atoms) cut
    into 8 - (n_subsets - 1) slabs of equal molecule count along x."""
    subset = np.asarray(w["subset"]); nsub = int(w["nsub"])
    lab = np.zeros(len(subset), dtype=np.int32)
    for s in range(1, nsub):
        lab[subset == s] = s - 1
    solvent = np.flatnonzero(subset == 0)
    nslab = 8 - (nsub - 1)
    x = w["pos"][solvent[::3], 0]
    rank = np.empty(len(x), dtype=np.int64); rank[np.argsort(x, kind="stable")] = np.arange(len(x))
    lab[solvent] = (nsub - 1) + np.repeat(rank * nslab // len(x), 3)[:len(solvent)]
    return lab, 8


def labels_residues(w, target=300):
    """The solute in about `target` runs of consecutive atoms (never across a subset change), the solvent as one last group."""
    subset = np.asarray(w["subset"])
    solute = np.flatnonzero(subset != 0)
    run = max(1, -(-len(solute) // target))
    lab = np.zeros(len(subset), dtype=np.int32)
    g = 0
    for s in np.unique(subset[solute]):
        idx = np.flatnonzero(subset == s)
        lab[idx] = g + np.arange(len(idx)) // run
        g = int(lab[idx].max()) + 1
    lab[subset == 0] = g
    return lab, g + 1


def child(args):
    sys.path.insert(0, os.path.abspath(args.tree))
    import bench
    import __graft_entry__
    import torch
    pkg = __graft_entry__._pkg()
    name = args.config
    n_target, Lbox, nsub, method, grid, dgrid, prec = bench.CONFIGS[name]
    w = bench.build_workload(n_target, Lbox, nsub, np.random.default_rng(bench.SEED))
    isd = prec == "double"; dt = torch.float64 if isd else torch.float32
    n = len(w["q"]); F = args.frames
    g = torch.Generator(device="cuda").manual_seed(4242)
    base = torch.tensor(w["pos"], dtype=dt, device="cuda")
    frames = torch.empty((F, n, 3), dtype=dt, device="cuda")
    frames[0] = base
    for f in range(1, F):
        frames[f] = base + 0.02 * torch.randn(base.shape, generator=g, device="cuda", dtype=dt)
    lab, G = labels_residues(w) if args.leg == "C" else labels8(w)
    lab = np.ascontiguousarray(lab, dtype=np.int32)
    if args.leg == "A":      # the labels as the engine's subsets
        w = dict(w); w["subset"] = lab; w["nsub"] = G; w["lam"] = np.ones((G * (G + 1) // 2, 2))
    eng = bench.Engine(pkg, w, method, grid, dgrid, prec, 0, 0, 1, 0.1, 1 << 30)
    eng.set_timing_interval(0)
    P = G * (G + 1) // 2

    def call_a(out):
        b = eng.capi.SnbFrameBatch()
        b.n_frames = F; b.positions = frames.data_ptr(); b.is_device = 1; b.is_double = int(isd); b.stride4 = 0
        b.mode = 1; b.include_direct = 1; b.include_reciprocal = 0
        rows = torch.empty((F, P, 2), dtype=torch.float64, device="cuda")
        b.slice_energies = rows.data_ptr(); b.out_is_device = 1
        eng.ok(eng.L.snb_evaluate_frames(eng.h, ctypes.byref(b)))
        eng.sync()
        return rows

    def call_b(out):
        b = eng.capi.SnbGroupPairBatch()
        b.n_frames = F; b.positions = frames.data_ptr(); b.is_device = 1; b.is_double = int(isd); b.stride4 = 0
        b.n_groups = G; b.group_of_atom = lab.ctypes.data_as(ctypes.POINTER(ctypes.c_int32))
        if out == "device":
            rows = torch.empty((F, P, 2), dtype=torch.float64, device="cuda")
            b.pair_energies = rows.data_ptr(); b.out_is_device = 1
        else:
            rows = np.empty((F, P, 2))
            b.pair_energies = rows.ctypes.data_as(ctypes.c_void_p); b.out_is_device = 0
        eng.ok(eng.L.snb_evaluate_group_pair_energies(eng.h, ctypes.byref(b)))
        if out == "device":
            eng.sync()
        return rows

    for out in (("device",) if args.leg == "A" else ("device", "host")):
        run = (lambda: call_a(out)) if args.leg == "A" else (lambda: call_b(out))
        run(); eng.sync(); torch.cuda.synchronize()      # warm-up: buffers, the first rebuilds of the engine
        snap = eng.capi.SnbFrameStats(); eng.ok(eng.L.snb_get_frame_stats(eng.h, ctypes.byref(snap)))
        per = []
        for _ in range(args.repeats):
            t0 = time.perf_counter()
            run()
            per.append((time.perf_counter() - t0) * 1e3 / F)
        st = eng.capi.SnbFrameStats(); eng.ok(eng.L.snb_get_frame_stats(eng.h, ctypes.byref(st)))
        rec = {"config": name, "leg": args.leg, "out": out, "frames": F, "groups": G, "per_frame_ms": [round(x, 4) for x in per],
               "built_beside": int(st.n_built_beside - snap.n_built_beside), "built_in_line": int(st.n_built_in_line - snap.n_built_in_line)}
        print(TAG + json.dumps(rec), flush=True)
    eng.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--baseline-tree")
    ap.add_argument("--configs", default="c3,c2")
    ap.add_argument("--frames", type=int, default=200)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--limit", type=int, default=240)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "group_pairs_timing.jsonl"))
    ap.add_argument("--leg", choices=["A", "B", "C"])
    ap.add_argument("--tree", default=ROOT)
    ap.add_argument("--config", default="c3")
    args = ap.parse_args()
    if args.leg:
        return child(args)
    if not args.baseline_tree or not os.path.isdir(args.baseline_tree):
        sys.exit("--baseline-tree DIR: a built tree of the parent commit (leg A runs there)")
    lines = []
    for name in args.configs.split(","):
        runs = {}
        for _ in range(args.rounds):
            for leg, tree in (("A", args.baseline_tree), ("B", ROOT), ("C", ROOT)):
                cmd = ["timeout", "-k", "10", str(args.limit), sys.executable, os.path.abspath(__file__), "--leg", leg, "--tree", tree, "--config", name,
                       "--frames", str(args.frames), "--repeats", str(args.repeats)]
                p = subprocess.run(cmd, stdout=subprocess.PIPE, text=True)
                if p.returncode != 0:
                    sys.exit("leg %s of %s ended with status %d: stopping here" % (leg, name, p.returncode))
                for line in p.stdout.splitlines():
                    if line.startswith(TAG):
                        print(line, flush=True)
                        r = json.loads(line[len(TAG):])
                        agg = runs.setdefault((r["leg"], r["out"]), dict(r, per_frame_ms=[]))
                        agg["per_frame_ms"] += r["per_frame_ms"]
                        agg["built_beside"] = r["built_beside"]; agg["built_in_line"] = r["built_in_line"]
        a = runs[("A", "device")]["per_frame_ms"]
        rec = {"config": name, "frames": args.frames, "samples_per_leg": len(a), "a_groups": runs[("A", "device")]["groups"],
               "a_median_ms": round(float(np.median(a)), 4), "a_spread_ms": round(max(a) - min(a), 4)}
        for (leg, out), r in sorted(runs.items()):
            if leg == "A":
                continue
            v = r["per_frame_ms"]; key = "%s_%s" % (leg.lower(), out)
            rec[key + "_groups"] = r["groups"]
            rec[key + "_median_ms"] = round(float(np.median(v)), 4); rec[key + "_spread_ms"] = round(max(v) - min(v), 4)
            rec[key + "_built_beside"] = r["built_beside"]; rec[key + "_built_in_line"] = r["built_in_line"]
        lines.append(json.dumps(rec))
        print(lines[-1], flush=True)
    with open(args.out, "a", encoding="utf-8") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
