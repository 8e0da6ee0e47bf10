"""Cost of energy-only steps (snb_execute with include_forces == 0) against forces steps, on the bench workloads.

    python tools/energy_only_timing.py [--configs c3,c2] [--steps K] [--warmup W] [--only KIND]

Per config, K back-to-back steps of each kind at fixed coordinates (no rebuild inside a region, kernel timers off, so forces steps
replay their step graph), timed with HIP events around the region:
  forces          forces only (the replayed step graph)
  forces_deriv    forces + the energies of the bound slices (the bench's c3 step: include_energy = 2)
  energy          energy-only, every slice (include_energy = 1): OpenMM getState(getEnergy=True) without forces
  energy_bound    energy-only, the bench's bound slices (include_energy = 2): MBAR re-analysis / getParameterDerivatives without forces
and a Monte Carlo barostat trial: box and coordinates scaled by 1.005, one energy-only step (the box change rebuilds the lists), read the
energy (synchronises); then the forces step at the restored box (which rebuilds again).  One JSON line per config.

--only KIND runs just the K steps of one kind after a single untimed step (for  rocprofv3 --kernel-trace --stats -- python ...).
"""
import argparse
import ctypes
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402
import __graft_entry__  # noqa: E402,F401  (puts the package, tests/ and oracle/ on sys.path)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--configs", default="c3,c2")
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--trials", type=int, default=10)
    ap.add_argument("--only", choices=["forces", "forces_deriv", "energy", "energy_bound"])
    args = ap.parse_args()
    import torch
    pkg = __graft_entry__._pkg()
    for name in args.configs.split(","):
        n_target, Lbox, nsub, method, grid, dgrid, prec = bench.CONFIGS[name]
        w = bench.build_workload(n_target, Lbox, nsub, np.random.default_rng(bench.SEED))
        isd = prec == "double"
        dt = torch.float64 if isd else torch.float32
        n = len(w["q"]); S = nsub * (nsub + 1) // 2
        eng = bench.Engine(pkg, w, method, grid, dgrid, prec, 0, 0, 1, 0.1, 1 << 30)
        eng.set_timing_interval(0)
        bound = (np.abs(w["lam"] - 1.0).max(axis=1) > 0).astype(np.int32)
        eng.set_energy_slices(bound)
        pos = torch.tensor(w["pos"], dtype=dt, device="cuda")
        forces = torch.zeros((n, 3), dtype=dt, device="cuda")
        eng.set_positions_device(pos.data_ptr(), isd)

        def step(kind):
            if kind == "forces":
                eng.execute(False); eng.forces_to(forces.data_ptr(), isd)
            elif kind == "forces_deriv":
                eng.execute(2, fetch=False); eng.forces_to(forces.data_ptr(), isd)
            else:
                eng.ok(eng.L.snb_execute(eng.h, 0, 1 if kind == "energy" else 2, 1, 1, None))

        if args.only:
            step(args.only); eng.sync(); torch.cuda.synchronize()
            for _ in range(args.steps):
                step(args.only)
            eng.sync(); torch.cuda.synchronize()
            print(json.dumps({"config": name, "only": args.only, "steps": args.steps}))
            eng.close()
            continue
        rec = {"config": name, "atoms": n, "precision": prec, "steps": args.steps}
        step("forces"); eng.sync()
        for kind in ("forces", "forces_deriv", "energy", "energy_bound"):
            for _ in range(args.warmup):
                step(kind)
            eng.sync(); torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(args.steps):
                step(kind)
            e1.record(); eng.sync(); torch.cuda.synchronize()
            rec[kind + "_ms"] = round(e0.elapsed_time(e1) / args.steps, 4)
        rec["energy_vs_forces"] = round(rec["energy_ms"] / rec["forces_ms"], 3)
        rec["energy_bound_vs_forces"] = round(rec["energy_bound_ms"] / rec["forces_ms"], 3)
        # barostat trial
        dp = lambda a: a.ctypes.data_as(ctypes.POINTER(ctypes.c_double))
        box = np.ascontiguousarray(bench.workload_box(w)); box2 = np.ascontiguousarray(box * 1.005)
        pos2 = pos * 1.005
        e = ctypes.c_double(0.0)
        trial, back = [], []
        for _ in range(args.trials):
            eng.sync()
            t0 = time.perf_counter()
            eng.ok(eng.L.snb_set_box(eng.h, dp(box2))); eng.set_positions_device(pos2.data_ptr(), isd)
            eng.ok(eng.L.snb_execute(eng.h, 0, 1, 1, 1, ctypes.byref(e)))      # (synchronises: the trial's energy)
            t1 = time.perf_counter()
            eng.ok(eng.L.snb_set_box(eng.h, dp(box))); eng.set_positions_device(pos.data_ptr(), isd)
            step("forces"); eng.sync()
            t2 = time.perf_counter()
            trial.append((t1 - t0) * 1e3); back.append((t2 - t1) * 1e3)
        rec["barostat_trial_ms"] = round(float(np.median(trial)), 3)
        rec["forces_step_after_trial_ms"] = round(float(np.median(back)), 3)
        rec["rebuilds"] = int(eng.stats().n_rebuilds)
        print(json.dumps(rec), flush=True)
        eng.close()


if __name__ == "__main__":
    main()
