"""(GPU box) Two builds of the engine on the same small system, bit for bit.

Usage: python tools/ab_bits.py LIB_A LIB_B [--bound] [--out FILE]

Each library (an experimental or an older build of the same ABI, loaded through SNB_LIB_PATH) evaluates the droplet of
tests/test_gpu_derivative_tiles.py -- 3000 atoms, four subsets by lattice site: masked and unmasked tiles, a padded last block, work
items of one tile and of eight, free j-slots -- in a fresh child process of its own, in mixed precision and direct space only
(include_reciprocal = 0): a forces-only step, a derivative step (every other slice wanted) and an energy step.  Mixed precision sums the
direct-space forces in 64-bit fixed point, so they do not depend on the order in which waves arrive: the forces of the three steps must
agree in every bit, and any difference is a difference in the pair arithmetic.  The raw slice energies of the derivative and the energy
step are double-precision sums of per-wave partial sums added in order of arrival; they are compared exactly and the largest relative
difference is printed (anything above 1e-12 fails: a reordered sum of these sizes stays far below that).
--bound: the same with a bound context-order buffer (snb_bind_context; tests/test_gpu_context_binding.py View); the int64 buffer is
compared as well.  Exit status 0: identical."""
import argparse
import json
import os
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "oracle")):
    if p not in sys.path:
        sys.path.insert(0, p)


def child(out, bound):
    import importlib
    if bound:      # (torch creates its HIP context first, as tests/conftest.py does: after an engine's it finds no device)
        import torch
        torch.cuda.init()
    snb = importlib.import_module("openmm-nonbonded-slicing_amd")
    import test_gpu_derivative_tiles as DT
    force, pos, box = DT.droplet(snb.SlicedNonbondedForce, 4)
    st = DT.Stepper(snb, force, pos, box, "mixed")
    view = None
    if bound:
        import torch
        import test_gpu_context_binding as CB
        view = CB.View(pos, False, 23)
        torch.cuda.synchronize()
        st.kern.bindContextBuffers(view.posq.data_ptr(), view.atom_index.data_ptr(), view.padded, forceBuffer=view.buf.data_ptr(), posqIsDouble=False)
        st.ctx.setPositions(np.zeros((st.n, 3)))
    k = st.kern

    def step(include_energy):
        import ctypes
        k._push_state(st.ctx)
        k._check(k._lib.snb_execute(k._h, 1, include_energy, 1, 0, None))
        f = np.zeros((st.n, 3))
        k._check(k._lib.snb_get_forces(k._h, f.ctypes.data_as(ctypes.c_void_p), 0, 1, 0))
        e = np.zeros((st.S, 2))
        if include_energy:
            k._check(k._lib.snb_get_slice_energies(k._h, DT._dp(e)))
        return f, e

    res = {}
    mask = np.zeros(st.S, dtype=np.int32); mask[0::2] = 1
    st.wanted(mask)
    res["f_forces"], _ = step(0)
    res["f_derivative"], res["e_derivative"] = step(2)
    st.wanted(np.ones(st.S, dtype=np.int32))
    res["f_energy"], res["e_energy"] = step(1)
    res["e_derivative"] = res["e_derivative"] * mask[:, None]
    if bound:
        assert k._lib.snb_synchronize(k._h) == 0
        res["bound_units"] = view.delivered_units().cpu().numpy()
    s = st.stats()
    res["n_tiles"] = np.array([s.n_tiles])
    np.savez(out, **res)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("libs", nargs="*"); ap.add_argument("--bound", action="store_true"); ap.add_argument("--out"); ap.add_argument("--child")
    a = ap.parse_args()
    if a.child:
        child(a.child, a.bound)
        return 0
    assert len(a.libs) == 2, "two library paths"
    got = []
    with tempfile.TemporaryDirectory() as tmp:
        for i, lib in enumerate(a.libs):
            out = os.path.join(tmp, "r%d.npz" % i)
            env = dict(os.environ, SNB_LIB_PATH=os.path.abspath(lib))
            subprocess.run([sys.executable, os.path.abspath(__file__), "--child", out] + (["--bound"] if a.bound else []), env=env, check=True, timeout=300)
            got.append(dict(np.load(out)))
    A, B = got
    report = {"libs": a.libs, "bound": a.bound, "n_tiles": [int(A["n_tiles"][0]), int(B["n_tiles"][0])], "identical": True}
    for key in sorted(A):
        if key == "n_tiles":
            continue
        x, y = A[key], B[key]
        if key.startswith("e_"):
            rel = float(np.max(np.abs(x - y) / np.maximum(np.abs(x), 1.0)))
            report[key] = {"exactly_equal": bool(np.array_equal(x, y)), "max_rel_diff": rel, "nonzero_entries": int(np.count_nonzero(x))}
            ok = rel <= 1e-12 and np.count_nonzero(x) > 0
        else:
            same = x.tobytes() == y.tobytes()
            report[key] = {"bit_identical": bool(same), "differing_components": int(np.count_nonzero(x != y)), "max_abs": float(np.max(np.abs(x.astype(np.float64))))}
            ok = same and np.count_nonzero(x) > 0
        report["identical"] = report["identical"] and bool(ok)
    line = json.dumps(report)
    print(line)
    if a.out:
        with open(a.out, "a") as f:
            f.write(line + "\n")
    return 0 if report["identical"] else 1


if __name__ == "__main__":
    sys.exit(main())
