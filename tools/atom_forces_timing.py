"""Cost of snb_evaluate_atom_forces against what gives the same table today: 2 S forces steps with one-hot lambdas.

    python tools/atom_forces_timing.py [--configs c3,c2] [--tables K] [--warmup W] [--repeats R] [--out profiles/atom_forces_timing.jsonl]

Per config one engine and one process; after a warm-up of both legs, R rounds that alternate two regions of K tables each at fixed
coordinates (no rebuild inside a region, kernel timers off), each timed with HIP events around the region:
  one_hot      leg A, per table: for every (slice, term) snb_set_lambdas with that entry 1 and every other 0, a forces-only snb_execute,
               snb_get_forces into a device buffer [2 S][N][3] -- entry points this call shares no code with; the host work of
               snb_set_lambdas lies inside the timed region (it is part of what the user pays on this route)
  atom_forces  leg B, per table: one snb_evaluate_atom_forces, device output
One JSON line per config: the median and the spread (min, max, max - min) of the R per-table times of each leg and the ratio of the medians.
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
    ap.add_argument("--tables", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "atom_forces_timing.jsonl"), help="append the JSON lines to this file")
    args = ap.parse_args()
    import torch
    pkg = __graft_entry__._pkg()
    dp = lambda a: a.ctypes.data_as(ctypes.POINTER(ctypes.c_double))
    for name in args.configs.split(","):
        n_target, Lbox, nsub, method, grid, dgrid, prec = bench.CONFIGS[name]
        w = bench.build_workload(n_target, Lbox, nsub, np.random.default_rng(bench.SEED))
        isd = prec == "double"
        dt = torch.float64 if isd else torch.float32
        n = len(w["q"]); S = nsub * (nsub + 1) // 2
        eng = bench.Engine(pkg, w, method, grid, dgrid, prec, 0, 0, 1, 0.1, 1 << 30)
        eng.set_timing_interval(0)
        pos = torch.tensor(w["pos"], dtype=dt, device="cuda")
        forces = torch.zeros((2 * S, n, 3), dtype=dt, device="cuda")
        table = torch.zeros((n, nsub, 2, 3), dtype=torch.float64, device="cuda")
        eng.set_positions_device(pos.data_ptr(), isd)
        one_hot = []
        for k in range(2 * S):
            lam = np.zeros((S, 2)); lam.reshape(-1)[k] = 1.0
            one_hot.append(lam)

        def leg(kind):
            if kind == "one_hot":
                for k, lam in enumerate(one_hot):
                    eng.ok(eng.L.snb_set_lambdas(eng.h, dp(lam)))
                    eng.execute(False); eng.forces_to(forces[k].data_ptr(), isd)
            else:
                eng.ok(eng.L.snb_evaluate_atom_forces(eng.h, 1, 1, ctypes.c_void_p(table.data_ptr()), 1))

        kinds = ("one_hot", "atom_forces")
        eng.execute(False); eng.sync()
        for kind in kinds:
            for _ in range(args.warmup):
                leg(kind)
        eng.sync(); torch.cuda.synchronize()
        times = {k: [] for k in kinds}
        for _ in range(args.repeats):
            for kind in kinds:
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(args.tables):
                    leg(kind)
                e1.record(); eng.sync(); torch.cuda.synchronize()
                times[kind].append(e0.elapsed_time(e1) / args.tables)
        rec = {"config": name, "atoms": n, "subsets": nsub, "one_hot_steps": 2 * S, "precision": prec, "tables": args.tables, "repeats": args.repeats}
        for kind in kinds:
            t = np.array(times[kind])
            rec[kind + "_ms"] = round(float(np.median(t)), 4); rec[kind + "_ms_min"] = round(float(t.min()), 4); rec[kind + "_ms_max"] = round(float(t.max()), 4)
            rec[kind + "_ms_spread"] = round(float(t.max() - t.min()), 4)
        rec["one_hot_vs_atom_forces"] = round(rec["one_hot_ms"] / rec["atom_forces_ms"], 3)
        rec["rebuilds"] = int(eng.stats().n_rebuilds)
        line = json.dumps(rec)
        print(line, flush=True)
        if args.out:
            with open(args.out, "a", encoding="utf-8") as f:
                f.write(line + "\n")
        eng.close()


if __name__ == "__main__":
    main()
