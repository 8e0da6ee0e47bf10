"""Cost of snb_evaluate_atom_energies against energy-only and forces steps, on the bench workloads.

    python tools/atom_energies_timing.py [--configs c3,c2] [--steps K] [--warmup W] [--repeats R] [--out profiles/atom_energies_timing.jsonl]

Per config one engine and one process; after a warm-up of every kind, R rounds that alternate three regions of K back-to-back evaluations at
fixed coordinates (no rebuild inside a region, kernel timers off), each timed with HIP events around the region:
  energy         energy-only steps, every slice (snb_execute with include_forces = 0, include_energy = 1)
  forces         forces-only steps (the replayed step graph), forces fetched into a device buffer
  atom_energies  snb_evaluate_atom_energies, device output
One JSON line per config: the median and the spread (min, max) of the R per-evaluation times of each kind, and the ratios of the medians.
"""
import argparse
import ctypes
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402
import __graft_entry__  # noqa: E402,F401  (puts the package, tests/ and oracle/ on sys.path)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--configs", default="c3,c2")
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=None, help="append the JSON lines to this file as well")
    args = ap.parse_args()
    import torch
    pkg = __graft_entry__._pkg()
    for name in args.configs.split(","):
        n_target, Lbox, nsub, method, grid, dgrid, prec = bench.CONFIGS[name]
        w = bench.build_workload(n_target, Lbox, nsub, np.random.default_rng(bench.SEED))
        isd = prec == "double"
        dt = torch.float64 if isd else torch.float32
        n = len(w["q"])
        eng = bench.Engine(pkg, w, method, grid, dgrid, prec, 0, 0, 1, 0.1, 1 << 30)
        eng.set_timing_interval(0)
        pos = torch.tensor(w["pos"], dtype=dt, device="cuda")
        forces = torch.zeros((n, 3), dtype=dt, device="cuda")
        table = torch.zeros((n, nsub, 2), dtype=torch.float64, device="cuda")
        eng.set_positions_device(pos.data_ptr(), isd)

        def step(kind):
            if kind == "forces":
                eng.execute(False); eng.forces_to(forces.data_ptr(), isd)
            elif kind == "energy":
                eng.ok(eng.L.snb_execute(eng.h, 0, 1, 1, 1, None))
            else:
                eng.ok(eng.L.snb_evaluate_atom_energies(eng.h, 1, 1, ctypes.c_void_p(table.data_ptr()), 1))

        kinds = ("energy", "forces", "atom_energies")
        step("forces"); eng.sync()
        for kind in kinds:
            for _ in range(args.warmup):
                step(kind)
        eng.sync(); torch.cuda.synchronize()
        times = {k: [] for k in kinds}
        for _ in range(args.repeats):
            for kind in kinds:
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(args.steps):
                    step(kind)
                e1.record(); eng.sync(); torch.cuda.synchronize()
                times[kind].append(e0.elapsed_time(e1) / args.steps)
        rec = {"config": name, "atoms": n, "subsets": nsub, "precision": prec, "steps": args.steps, "repeats": args.repeats}
        for kind in kinds:
            t = np.array(times[kind])
            rec[kind + "_ms"] = round(float(np.median(t)), 4); rec[kind + "_ms_min"] = round(float(t.min()), 4); rec[kind + "_ms_max"] = round(float(t.max()), 4)
        rec["atom_energies_vs_energy"] = round(rec["atom_energies_ms"] / rec["energy_ms"], 3)
        rec["atom_energies_vs_forces"] = round(rec["atom_energies_ms"] / rec["forces_ms"], 3)
        rec["rebuilds"] = int(eng.stats().n_rebuilds)
        line = json.dumps(rec)
        print(line, flush=True)
        if args.out:
            with open(args.out, "a", encoding="utf-8") as f:
                f.write(line + "\n")
        eng.close()


if __name__ == "__main__":
    main()
