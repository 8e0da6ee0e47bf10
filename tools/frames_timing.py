"""Per-frame cost of a stored trajectory's slice energies: snb_evaluate_frames against the hand-written per-frame loop.

    python tools/frames_timing.py --baseline-tree DIR [--configs c3,c2] [--frames 200] [--repeats 3] [--rounds 2] [--limit SECONDS]

Frames: the bench workload of the config and F - 1 seeded Gaussian perturbations of 0.02 nm of it, resident on the device, in the
config's precision.  Box: constant, or scaled (with the coordinates) by 1 + 0.0005 (f mod 3), i.e. another box every frame.

  leg A   the per-frame loop a caller writes by hand: snb_set_box (changing box), snb_set_positions (device pointer),
          snb_rebuild_neighbors (the frames are unrelated coordinates), energy-only snb_execute, snb_get_slice_energies (synchronises).  It uses only entry points of the PARENT commit and runs as a child process
          on a built tree of that commit (--baseline-tree: `git archive` of the parent, built beforehand), because the binding checks every
          declared symbol against the library it loads: the parent's library cannot be loaded by this tree's binding.
  leg B   snb_evaluate_frames of this tree, with device output (call + snb_synchronize) and with host output.
  leg I   leg B with SNB_FRAMES_IN_LINE set: the same call with every frame's list built in line -- what building beside the step buys
          (or costs) inside one library.

Each for mode 1 (every slice) and mode 2 (the config's bound slices), constant and changing box.  Legs alternate A / B / I / A / B / I, one fresh
child process per leg, each under its own time limit; the chain ends at the first failure.  A child prints one JSON line per variant
with the per-frame wall time of every repeat; the parent prints the medians and the spread (max - min) of the repeats and appends the
aggregate lines to profiles/frames_timing.jsonl.

    python tools/frames_timing.py --leg A|B --tree DIR --config c3 ...      (what a child runs)
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


def _scale(f):
    return 1.0 + 0.0005 * (f % 3)


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
    n = len(w["q"]); S = nsub * (nsub + 1) // 2; F = args.frames
    g = torch.Generator(device="cuda").manual_seed(4242)
    base = torch.tensor(w["pos"], dtype=dt, device="cuda")
    frames = {"const": torch.empty((F, n, 3), dtype=dt, device="cuda")}
    frames["const"][0] = base
    for f in range(1, F):
        frames["const"][f] = base + 0.02 * torch.randn(base.shape, generator=g, device="cuda", dtype=dt)
    scales = torch.tensor([_scale(f) for f in range(F)], dtype=dt, device="cuda").reshape(F, 1, 1)
    frames["change"] = frames["const"] * scales
    box0 = bench.workload_box(w)
    boxes = {"const": None, "change": np.ascontiguousarray(np.stack([box0 * _scale(f) for f in range(F)]))}
    bound = (np.abs(w["lam"] - 1.0).max(axis=1) > 0).astype(np.int32)
    dp = lambda a: a.ctypes.data_as(ctypes.POINTER(ctypes.c_double))
    eng = bench.Engine(pkg, w, method, grid, dgrid, prec, 0, 0, 1, 0.1, 1 << 30)
    eng.set_timing_interval(0)
    eng.set_energy_slices(bound)
    out_h = np.zeros((S, 2))
    frame_bytes = n * 3 * (8 if isd else 4)

    def loop_a(mode, kind):
        fr = frames[kind]; bx = boxes[kind]; ptr = fr.data_ptr()
        for f in range(F):
            if bx is not None:
                eng.ok(eng.L.snb_set_box(eng.h, dp(bx[f])))
            eng.ok(eng.L.snb_set_positions(eng.h, ctypes.c_void_p(ptr + f * frame_bytes), 1, int(isd), 0))
            eng.ok(eng.L.snb_rebuild_neighbors(eng.h))      # unrelated coordinates: the list of the previous frame is of no use (a box change asks for it anyway)
            eng.ok(eng.L.snb_execute(eng.h, 0, mode, 1, 1, None))
            eng.ok(eng.L.snb_get_slice_energies(eng.h, dp(out_h)))

    def call_b(mode, kind, out):
        b = eng.capi.SnbFrameBatch()
        b.n_frames = F; b.positions = frames[kind].data_ptr(); b.is_device = 1; b.is_double = int(isd); b.stride4 = 0
        if boxes[kind] is not None:
            b.boxes = dp(boxes[kind])
        b.mode = mode; b.include_direct = 1; b.include_reciprocal = 1
        if out == "device":
            rows = torch.empty((F, S, 2), dtype=torch.float64, device="cuda")
            b.slice_energies = rows.data_ptr(); b.out_is_device = 1
        else:
            rows = np.empty((F, S, 2))
            b.slice_energies = rows.ctypes.data_as(ctypes.c_void_p); b.out_is_device = 0
        eng.ok(eng.L.snb_evaluate_frames(eng.h, ctypes.byref(b)))
        if out == "device":
            eng.sync()
        return rows

    for kind in ("const", "change"):
        if boxes[kind] is None:
            eng.ok(eng.L.snb_set_box(eng.h, dp(np.ascontiguousarray(box0))))
        for mode in (1, 2):
            for out in (("loop",) if args.leg == "A" else ("device", "host")):
                snap = None
                run = (lambda: loop_a(mode, kind)) if args.leg == "A" else (lambda: call_b(mode, kind, out))
                run(); eng.sync(); torch.cuda.synchronize()      # warm-up: buffers, the first two rebuilds of the engine
                per = []
                if args.leg != "A":      # (the counters are cumulative: what the timed repeats add is reported)
                    snap = eng.capi.SnbFrameStats(); eng.ok(eng.L.snb_get_frame_stats(eng.h, ctypes.byref(snap)))
                for _ in range(args.repeats):
                    t0 = time.perf_counter()
                    run()
                    per.append((time.perf_counter() - t0) * 1e3 / F)
                rec = {"config": name, "leg": args.leg, "mode": mode, "box": kind, "out": out, "frames": F, "per_frame_ms": [round(x, 4) for x in per]}
                if args.leg != "A":
                    st = eng.capi.SnbFrameStats(); eng.ok(eng.L.snb_get_frame_stats(eng.h, ctypes.byref(st)))
                    rec.update(built_beside=int(st.n_built_beside - snap.n_built_beside), built_in_line=int(st.n_built_in_line - snap.n_built_in_line),
                               side_discarded=int(st.n_side_discarded - snap.n_side_discarded))
                print("FRAMES_TIMING " + json.dumps(rec), flush=True)
    eng.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--baseline-tree")
    ap.add_argument("--configs", default="c3,c2")
    ap.add_argument("--frames", type=int, default=200)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--limit", type=int, default=240)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "frames_timing.jsonl"))
    ap.add_argument("--leg", choices=["A", "B", "I"])
    ap.add_argument("--tree", default=ROOT)
    ap.add_argument("--config", default="c3")
    args = ap.parse_args()
    if args.leg:
        return child(args)
    if not args.baseline_tree or not os.path.isdir(args.baseline_tree):
        sys.exit("--baseline-tree DIR: a built tree of the parent commit (leg A runs there)")
    runs = {}
    for name in args.configs.split(","):
        for _ in range(args.rounds):
            for leg, tree in (("A", args.baseline_tree), ("B", ROOT), ("I", ROOT)):
                cmd = ["timeout", "-k", "10", str(args.limit), sys.executable, os.path.abspath(__file__), "--leg", leg, "--tree", tree, "--config", name,
                       "--frames", str(args.frames), "--repeats", str(args.repeats)]
                env = dict(os.environ)
                if leg == "I":
                    env["SNB_FRAMES_IN_LINE"] = "1"
                p = subprocess.run(cmd, stdout=subprocess.PIPE, text=True, env=env)
                if p.returncode != 0:
                    sys.exit("leg %s of %s ended with status %d: stopping here" % (leg, name, p.returncode))
                for line in p.stdout.splitlines():
                    if line.startswith("FRAMES_TIMING "):
                        print(line, flush=True)
                        r = json.loads(line[len("FRAMES_TIMING "):])
                        key = (r["config"], r["mode"], r["box"], r["leg"], r["out"])
                        agg = runs.setdefault(key, dict(r, per_frame_ms=[]))
                        agg["per_frame_ms"] += r["per_frame_ms"]
                        for k in ("built_beside", "built_in_line", "side_discarded"):
                            if k in r:
                                agg[k] = r[k]
    lines = []
    for key in sorted(runs):
        r = runs[key]; v = r["per_frame_ms"]
        r["median_ms"] = round(float(np.median(v)), 4); r["spread_ms"] = round(max(v) - min(v), 4)
        if r["leg"] != "A":
            a = runs.get((r["config"], r["mode"], r["box"], "A", "loop"))
            if a:
                av = a["per_frame_ms"]
                r["a_median_ms"] = round(float(np.median(av)), 4); r["a_spread_ms"] = round(max(av) - min(av), 4)
                r["gain_ms"] = round(r["a_median_ms"] - r["median_ms"], 4)
                r["gain_beyond_a_spread"] = bool(r["gain_ms"] > r["a_spread_ms"])
        lines.append(json.dumps(r))
        print(lines[-1], flush=True)
    with open(args.out, "a", encoding="utf-8") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
