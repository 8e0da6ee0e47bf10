"""Per-frame cost of per-group forces over a stored trajectory: snb_evaluate_group_forces against the hand-written loop.

    python tools/group_force_frames_timing.py --baseline-tree DIR [--configs c3,c2] [--frames 200] [--loop-frames N] [--states 11]
                                              [--repeats 3] [--rounds 2] [--limit SECONDS]

Frames: the bench workload of the config and F - 1 seeded Gaussian perturbations of 0.02 nm of it, resident on the device, in the
config's precision; constant box.  Groups: one per 3 consecutive atoms of the solvent subset (a water molecule), one per 12 consecutive
atoms elsewhere (a coarse-grained site).  Lambda states: K = 0 (the raw rows alone) and K = --states seeded tables in [0, 1] (rows and
state forces).

  leg A   the per-frame loop a caller writes by hand: snb_set_positions (device pointer), snb_rebuild_neighbors (the frames are unrelated
          coordinates), snb_evaluate_atom_forces with host output (synchronises, moves the [N][n_subsets][2][3] table), the group sums in
          NumPy (np.add.reduceat over the gathered rows: the fastest form NumPy offers) and, with K > 0, forcesFromAtomForces per state
          before its group sum.  It uses only entry points of the PARENT commit and runs as a child process on a built tree of that commit
          (--baseline-tree: `git archive` of the parent, built beforehand), because the binding checks every declared symbol against the
          library it loads.  Its per-frame cost does not depend on F: --loop-frames (default F) runs it over the first N frames only.
  leg B   snb_evaluate_group_forces of this tree, with device output (call + snb_synchronize) and with host output.
  leg I   leg B with SNB_FRAMES_IN_LINE set: every frame's list built in line.

Legs alternate A / B / I / A / B / I, one fresh child process per leg, each under its own time limit; the chain ends at the first
failure.  A child prints one JSON line per variant with the per-frame wall time of every repeat; the parent prints the medians and the
spread (max - min) of the repeats and appends one aggregate line per config to profiles/group_forces_timing.jsonl.

    python tools/group_force_frames_timing.py --leg A|B --tree DIR --config c3 ...      (what a child runs)
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


def make_groups(subset):
    """CSR (start, atoms) of the tool's groups: runs of 3 atoms inside the solvent subset (0), runs of 12 elsewhere, never across a subset change."""
    subset = np.asarray(subset)
    cuts = np.flatnonzero(np.diff(subset)) + 1
    starts = []
    for a, b in zip(np.concatenate([[0], cuts]), np.concatenate([cuts, [len(subset)]])):
        starts.append(np.arange(a, b, 3 if subset[a] == 0 else 12))
    start = np.concatenate(starts + [[len(subset)]]).astype(np.int32)
    return start, np.arange(len(subset), dtype=np.int32)


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
    start, atoms = make_groups(w["subset"])
    G = len(start) - 1
    S = nsub * (nsub + 1) // 2
    eng = bench.Engine(pkg, w, method, grid, dgrid, prec, 0, 0, 1, 0.1, 1 << 30)
    eng.set_timing_interval(0)
    frame_bytes = n * 3 * (8 if isd else 4)
    table = np.zeros((n, nsub, 2, 3))
    ip = lambda a: a.ctypes.data_as(ctypes.POINTER(ctypes.c_int32))
    dp = lambda a: a.ctypes.data_as(ctypes.POINTER(ctypes.c_double))
    kern = pkg.HipCalcSlicedNonbondedForceKernel

    def loop_a(K, lam):
        Fa = min(F, args.loop_frames or F)
        ptr = frames.data_ptr(); first = start[:-1].astype(np.int64)
        rows = np.empty((Fa, G, nsub, 2, 3)); st = np.empty((Fa, max(K, 1), G, 3))
        for f in range(Fa):
            eng.ok(eng.L.snb_set_positions(eng.h, ctypes.c_void_p(ptr + f * frame_bytes), 1, int(isd), 0))
            eng.ok(eng.L.snb_rebuild_neighbors(eng.h))      # unrelated coordinates: the list of the previous frame is of no use
            eng.ok(eng.L.snb_evaluate_atom_forces(eng.h, 1, 1, table.ctypes.data_as(ctypes.c_void_p), 0))
            rows[f] = np.add.reduceat(table[atoms], first, axis=0)      # (no group of the tool is empty)
            for k in range(K):
                st[f, k] = np.add.reduceat(kern.forcesFromAtomForces(table, w["subset"], lam[k])[atoms], first, axis=0)
        return Fa

    def call_b(K, lam, out):
        b = eng.capi.SnbGroupForceBatch()
        b.n_frames = F; b.positions = frames.data_ptr(); b.is_device = 1; b.is_double = int(isd); b.stride4 = 0
        b.include_direct = 1; b.include_reciprocal = 1; b.n_groups = G; b.group_start = ip(start); b.group_atoms = ip(atoms)
        b.n_states = K
        if K:
            b.state_lambdas = dp(lam)
        if out == "device":
            rows = torch.empty((F, G, nsub, 2, 3), dtype=torch.float64, device="cuda"); st = torch.empty((F, max(K, 1), G, 3), dtype=torch.float64, device="cuda")
            b.group_forces = rows.data_ptr(); b.state_forces = st.data_ptr() if K else None; b.out_is_device = 1
        else:
            rows = np.empty((F, G, nsub, 2, 3)); st = np.empty((F, max(K, 1), G, 3))
            b.group_forces = rows.ctypes.data_as(ctypes.c_void_p); b.state_forces = st.ctypes.data_as(ctypes.c_void_p) if K else None; b.out_is_device = 0
        eng.ok(eng.L.snb_evaluate_group_forces(eng.h, ctypes.byref(b)))
        if out == "device":
            eng.sync()
        return F

    for K in (0, args.states):
        lam = np.ascontiguousarray(np.random.default_rng(77).uniform(0.0, 1.0, (max(K, 1), S, 2)))
        for out in (("loop",) if args.leg == "A" else ("device", "host")):
            run = (lambda: loop_a(K, lam)) if args.leg == "A" else (lambda: call_b(K, lam, out))
            run(); eng.sync(); torch.cuda.synchronize()      # warm-up: buffers, the first two rebuilds of the engine
            per = []; snap = None
            if args.leg != "A":      # (the counters are cumulative: what the timed repeats add is reported)
                snap = eng.capi.SnbFrameStats(); eng.ok(eng.L.snb_get_frame_stats(eng.h, ctypes.byref(snap)))
            ran = F
            for _ in range(args.repeats):
                t0 = time.perf_counter()
                ran = run()
                per.append((time.perf_counter() - t0) * 1e3 / ran)
            rec = {"config": name, "leg": args.leg, "out": out, "states": K, "frames": ran, "groups": G, "per_frame_ms": [round(x, 4) for x in per]}
            if args.leg != "A":
                st = eng.capi.SnbFrameStats(); eng.ok(eng.L.snb_get_frame_stats(eng.h, ctypes.byref(st)))
                rec.update(built_beside=int(st.n_built_beside - snap.n_built_beside), built_in_line=int(st.n_built_in_line - snap.n_built_in_line),
                           side_discarded=int(st.n_side_discarded - snap.n_side_discarded))
            print("GROUP_FORCE_TIMING " + json.dumps(rec), flush=True)
    eng.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--baseline-tree")
    ap.add_argument("--configs", default="c3,c2")
    ap.add_argument("--frames", type=int, default=200)
    ap.add_argument("--loop-frames", type=int, default=0)
    ap.add_argument("--states", type=int, default=11)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--limit", type=int, default=300)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "group_forces_timing.jsonl"))
    ap.add_argument("--leg", choices=["A", "B", "I"])
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
            for leg, tree in (("A", args.baseline_tree), ("B", ROOT), ("I", ROOT)):
                cmd = ["timeout", "-k", "10", str(args.limit), sys.executable, os.path.abspath(__file__), "--leg", leg, "--tree", tree, "--config", name,
                       "--frames", str(args.frames), "--loop-frames", str(args.loop_frames), "--states", str(args.states), "--repeats", str(args.repeats)]
                env = dict(os.environ)
                if leg == "I":
                    env["SNB_FRAMES_IN_LINE"] = "1"
                p = subprocess.run(cmd, stdout=subprocess.PIPE, text=True, env=env)
                if p.returncode != 0:
                    sys.exit("leg %s of %s ended with status %d: stopping here" % (leg, name, p.returncode))
                for line in p.stdout.splitlines():
                    if line.startswith("GROUP_FORCE_TIMING "):
                        print(line, flush=True)
                        r = json.loads(line[len("GROUP_FORCE_TIMING "):])
                        agg = runs.setdefault((r["leg"], r["out"], r["states"]), dict(r, per_frame_ms=[]))
                        agg["per_frame_ms"] += r["per_frame_ms"]
                        for k in ("built_beside", "built_in_line", "side_discarded"):
                            if k in r:
                                agg[k] = r[k]
        for K in (0, args.states):
            a = runs[("A", "loop", K)]
            rec = {"config": name, "states": K, "frames": args.frames, "loop_frames": a["frames"], "groups": a["groups"], "samples_per_leg": len(a["per_frame_ms"]),
                   "a_median_ms": round(float(np.median(a["per_frame_ms"])), 4), "a_spread_ms": round(max(a["per_frame_ms"]) - min(a["per_frame_ms"]), 4)}
            for (leg, out, k), r in sorted(runs.items()):
                if leg == "A" or k != K:
                    continue
                v = r["per_frame_ms"]; key = "%s_%s" % ("b" if leg == "B" else "in_line", out)
                rec[key + "_median_ms"] = round(float(np.median(v)), 4); rec[key + "_spread_ms"] = round(max(v) - min(v), 4)
                rec[key + "_built_beside"] = r.get("built_beside"); rec[key + "_built_in_line"] = r.get("built_in_line")
                rec[key + "_below_a_by_more_than_a_spread"] = bool(rec["a_median_ms"] - rec[key + "_median_ms"] > rec["a_spread_ms"])
            lines.append(json.dumps(rec))
            print(lines[-1], flush=True)
    with open(args.out, "a", encoding="utf-8") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
