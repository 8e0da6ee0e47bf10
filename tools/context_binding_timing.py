"""What the context binding (snb_bind_context) buys per step, on c3, in one process.

    python tools/context_binding_timing.py [--config c3] [--steps 200] [--rounds 3] [--order spatial|random] [--bound-only]

Three forms of the same step at fixed coordinates (no rebuild inside a region, kernel timers off: every step replays its graph), as a
context-order posq / fixed-point force buffer would be served:
  A  the form before the binding: the unbound engine with the OpenMM adapter's three kernels launched on the same stream around every
     snb_execute (tools/context_adapter_kernels.hip: posq -> user-order positions, user-order forces -> fixed-point buffer with three
     atomics per atom, slice energies -> derivative buffer)
  B  the bound engine: snb_execute alone
  C  the plain unbound step with no adapter kernels (the floor: it delivers user-order floats, not what the context needs)
run alternating A/B/C/A/B/C... in regions of --steps steps timed with HIP events, for forces-only steps and for derivative steps
(include_energy = 2).  One JSON line: per form and step kind the per-round times, their median and spread (ms per step), B/A, B - C,
and the per-kernel stamps of the gather pass and the last interpolation (SNB_K_GATHER, SNB_K_INTERPOLATE) of forms B and C from a few
eager steps.  SNB_CTX_ATOMIC_ADD=1 in the environment runs B's force delivery with 64-bit atomics instead of plain read-modify-write.

--order: the context's atom order.  `spatial` (default): atoms sorted by the 0.6 nm cell they lie in, as a GPU platform that re-sorts its
atoms for locality keeps them; `random`: a seeded random permutation, the worst case for the scattered side of every form (A gathers
12 bytes per atom from user order, B adds 3 x 8 bytes per atom into context order).

--bound-only runs just form B's forces-only steps after one untimed step (for  rocprofv3 --kernel-trace --stats -- python ...).
"""
import argparse
import ctypes
import json
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402
import __graft_entry__  # noqa: E402,F401  (puts the package, tests/ and oracle/ on sys.path)

ADAPTER_SRC = os.path.join(ROOT, "tools", "context_adapter_kernels.hip")
ADAPTER_LIB = os.path.join(ROOT, os.environ.get("OUT", "tools_out"), "libcontext_adapter_kernels.so")


def adapter_lib():
    if not os.path.exists(ADAPTER_LIB) or os.path.getmtime(ADAPTER_LIB) < os.path.getmtime(ADAPTER_SRC):
        os.makedirs(os.path.dirname(ADAPTER_LIB), exist_ok=True)
        subprocess.check_call([os.environ.get("HIPCC", "/opt/rocm/bin/hipcc"), "-O3", "-fPIC", "-shared", "--offload-arch=gfx950", ADAPTER_SRC, "-o", ADAPTER_LIB])
    L = ctypes.CDLL(ADAPTER_LIB)
    vp, i32 = ctypes.c_void_p, ctypes.c_int32
    L.adapter_gather_positions.argtypes = [vp, vp, vp, i32, i32, vp]; L.adapter_gather_positions.restype = None
    L.adapter_add_forces.argtypes = [vp, vp, vp, i32, i32, i32, vp]; L.adapter_add_forces.restype = None
    L.adapter_add_derivatives.argtypes = [vp, vp, i32, vp, i32, vp]; L.adapter_add_derivatives.restype = None
    return L


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="c3")
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--order", choices=["spatial", "random"], default="spatial")
    ap.add_argument("--bound-only", action="store_true")
    args = ap.parse_args()
    if args.bound_only:
        os.environ.setdefault("SNB_OVERLAP", "0")
    import torch
    pkg = __graft_entry__._pkg()
    capi = pkg.capi
    own = torch.cuda.Stream(); torch.cuda.set_stream(own)
    stream = torch.cuda.current_stream().cuda_stream
    n_target, Lbox, nsub, method, grid, dgrid, prec = bench.CONFIGS[args.config]
    w = bench.build_workload(n_target, Lbox, nsub, np.random.default_rng(bench.SEED))
    isd = prec == "double"
    dt = torch.float64 if isd else torch.float32
    n = len(w["q"]); S = nsub * (nsub + 1) // 2
    bound_slices = (np.abs(w["lam"] - 1.0).max(axis=1) > 0).astype(np.int32)
    slots = np.full((S, 2), -1, dtype=np.int32)
    slots[bound_slices != 0] = np.arange(2 * int(bound_slices.sum()), dtype=np.int32).reshape(-1, 2)
    # the context's view
    g = torch.Generator().manual_seed(1)
    if args.order == "random":
        atom_index = torch.randperm(n, generator=g).to(torch.int32).cuda()
    else:
        cell = np.floor(np.mod(w["pos"], Lbox) / 0.6).astype(np.int64)
        atom_index = torch.tensor(np.lexsort((cell[:, 2], cell[:, 1], cell[:, 0])).astype(np.int32)).cuda()
    padded = (n + 31) // 32 * 32 + 64
    posq = torch.zeros((padded, 4), dtype=dt, device="cuda")
    posq[:n, :3] = torch.tensor(w["pos"], dtype=dt, device="cuda")[atom_index.long()]
    fbuf = torch.zeros((3, padded), dtype=torch.int64, device="cuda")
    ebuf = torch.zeros(1, dtype=torch.float64, device="cuda"); dbuf = torch.zeros(2 * S, dtype=torch.float64, device="cuda")
    dslots = torch.tensor(slots.reshape(-1), dtype=torch.int32, device="cuda")

    def engine():
        e = bench.Engine(pkg, w, method, grid, dgrid, prec, 0, 0, 1, 0.1, 1 << 30, stream=stream)
        e.set_timing_interval(0); e.set_energy_slices(bound_slices)
        return e

    # B: bound
    eb = engine()
    b = capi.SnbContextBinding()
    b.posq = posq.data_ptr(); b.atom_index = atom_index.data_ptr(); b.is_double = int(isd); b.padded_n = padded
    b.force_buffer = fbuf.data_ptr(); b.energy_buffer = ebuf.data_ptr(); b.deriv_buffer = dbuf.data_ptr()
    b.deriv_slot = slots.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)); b.energy_is_double = 1
    torch.cuda.synchronize()
    eb.ok(eb.L.snb_bind_context(eb.h, ctypes.byref(b)))

    def step_b(deriv):
        eb.ok(eb.L.snb_execute(eb.h, 1, 2 if deriv else 0, 1, 1, None))

    if args.bound_only:
        step_b(False); eb.sync()
        for _ in range(args.steps):
            step_b(False)
        eb.sync(); torch.cuda.synchronize()
        print(json.dumps({"config": args.config, "only": "bound forces", "steps": args.steps}))
        eb.close()
        return
    # A: unbound + the adapter's kernels; C: unbound, plain
    A = adapter_lib()
    ea, ec = engine(), engine()
    user_pos = torch.zeros((n, 4), dtype=dt, device="cuda")
    user_f = torch.zeros((n, 3), dtype=dt, device="cuda"); plain_f = torch.zeros((n, 3), dtype=dt, device="cuda")
    ea.set_force_output(user_f.data_ptr(), isd, 0)
    slice_dev = ctypes.c_void_p()
    ea.ok(ea.L.snb_slice_energies_device(ea.h, ctypes.byref(slice_dev)))
    pos_c = torch.tensor(w["pos"], dtype=dt, device="cuda")
    ec.set_force_output(plain_f.data_ptr(), isd, 0)
    ec.set_positions_device(pos_c.data_ptr(), isd)

    def step_a(deriv):
        A.adapter_gather_positions(posq.data_ptr(), atom_index.data_ptr(), user_pos.data_ptr(), n, int(isd), stream)
        ea.ok(ea.L.snb_set_positions(ea.h, ctypes.c_void_p(user_pos.data_ptr()), 1, int(isd), 1))
        ea.ok(ea.L.snb_execute(ea.h, 1, 2 if deriv else 0, 1, 1, None))
        A.adapter_add_forces(user_f.data_ptr(), atom_index.data_ptr(), fbuf.data_ptr(), n, padded, int(isd), stream)
        if deriv:
            A.adapter_add_derivatives(slice_dev, dslots.data_ptr(), 2 * S, dbuf.data_ptr(), 1, stream)

    def step_c(deriv):
        ec.ok(ec.L.snb_execute(ec.h, 1, 2 if deriv else 0, 1, 1, None))

    forms = {"A": step_a, "B": step_b, "C": step_c}
    rec = {"config": args.config, "order": args.order, "atoms": n, "precision": prec, "steps": args.steps, "rounds": args.rounds,
           "force_add": "atomic" if os.environ.get("SNB_CTX_ATOMIC_ADD") else "read-modify-write"}
    for deriv in (False, True):
        kind = "deriv" if deriv else "forces"
        times = {k: [] for k in forms}
        for k, f in forms.items():
            for _ in range(args.warmup):
                f(deriv)
        torch.cuda.synchronize()
        for _ in range(args.rounds):
            for k, f in forms.items():
                fbuf.zero_()
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(args.steps):
                    f(deriv)
                e1.record(); torch.cuda.synchronize()
                times[k].append(e0.elapsed_time(e1) / args.steps)
        for k in forms:
            rec["%s_%s_ms" % (k, kind)] = [round(t, 4) for t in times[k]]
            rec["%s_%s_median_ms" % (k, kind)] = round(float(np.median(times[k])), 4)
            rec["%s_%s_spread_ms" % (k, kind)] = round(float(max(times[k]) - min(times[k])), 4)
        rec["B_over_A_" + kind] = round(rec["B_%s_median_ms" % kind] / rec["A_%s_median_ms" % kind], 4)
        rec["B_minus_C_%s_us" % kind] = round(1e3 * (rec["B_%s_median_ms" % kind] - rec["C_%s_median_ms" % kind]), 2)
    # per-kernel stamps of the gather pass and the last interpolation, from eager (serial, stamped) steps
    for k, e, f in (("B", eb, step_b), ("C", ec, step_c)):
        e.set_timing_interval(1); e.reset_timers()
        for _ in range(12):
            f(False)
        st = e.stats()
        for slot, nm in ((0, "gather"), (7, "interpolate")):
            if st.n_kernel_timed[slot]:
                rec["%s_%s_us" % (k, nm)] = round(1e3 * st.sum_kernel_ms[slot] / st.n_kernel_timed[slot], 2)
    print(json.dumps(rec), flush=True)
    for e in (ea, eb, ec):
        e.close()


if __name__ == "__main__":
    main()
