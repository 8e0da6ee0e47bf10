"""The mesh-size census on the GPU (-m gpu): every (R1, R2) instantiation of the reciprocal path against a reference (the table and what each
row is there for: tests/mesh_census.py; its completeness against the build: tests/test_mesh_census.py).

Transform level: snb_test_fft3d (k_fftZ, k_fftStrided on y and, through the x hook, on x) on each of the sixteen pair sizes on each axis in turn, batch 1 and 3,
both precisions, against numpy.fft.rfftn in double -- at the bars of test_gpu_parity.py test_fft_against_numpy.

Pipeline level: every row in single and double precision (two rows in mixed), reciprocal part alone, against the oracle at the bars and rules
of tests/recip_systems.py: an energy + forces + derivatives step, two forces-only steps (the second replays the captured graph), an energy-only
step (the `..., true>` kernels).  Every case runs in a child process of its own with the row's environment and SNB_VERBOSE=1: the switches
are read once per process, and the engine's mesh line is how a case knows which instantiations ran -- it must state the row's splits word for
word, the sort columns and spreader that tests/mesh_census.py plan() expects, and the stamp slots must show the row's pipeline."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import mesh_census as M
import recip_systems as R
import shell_systems as S

pytestmark = pytest.mark.gpu

# ---- transform level ------------------------------------------------------------------------------------------------------------------
SHAPES = (lambda n: (n, 20, 22), lambda n: (21, n, 20), lambda n: (20, 22, n))          # the other two axes: short staged sizes
FFT_TOL = {"double": 1e-10, "single": 2e-4}


@pytest.mark.parametrize("prec", ["double", "single"])
@pytest.mark.parametrize("axis", [0, 1, 2], ids=["x", "y", "z"])
def test_pair_sizes_against_numpy(axis, prec, snb):
    """Spectrum within tol of max |ref|, scaled round trip within 10 tol, for every pair size on this axis; a failure names the sizes."""
    import ctypes
    L = snb.capi.lib()
    dp = ctypes.POINTER(ctypes.c_double)
    rng = np.random.default_rng(17 + axis)
    tol = FFT_TOL[prec]
    failures = []
    for n in M.SIZES:
        for batch in (1, 3):
            nx, ny, nz = SHAPES[axis](n)
            a = rng.standard_normal((batch, nx, ny, nz))
            spec = np.zeros((batch, nx, ny, nz // 2 + 1, 2)); rt = np.zeros_like(a)
            st = L.snb_test_fft3d(1 if prec == "double" else 0, 0, batch, nx, ny, nz, a.ctypes.data_as(dp), spec.ctypes.data_as(dp), rt.ctypes.data_as(dp))
            assert st == 0, (n, batch, st)
            ref = np.fft.rfftn(a, axes=(1, 2, 3))
            es = np.abs(spec[..., 0] + 1j * spec[..., 1] - ref).max() / np.abs(ref).max()
            er = np.abs(rt / (nx * ny * nz) - a).max()
            print("fft %s %s n %d batch %d: spectrum %.2e of max |ref|, round trip %.2e" % ("xyz"[axis], prec, n, batch, es, er))
            if not (es < tol and er < 10 * tol):
                failures.append("n = %d on %s, batch %d, %s: spectrum %.2e (bar %.0e), round trip %.2e (bar %.0e)" % (n, "xyz"[axis], batch, prec, es, tol, er, 10 * tol))
    assert not failures, "\n".join(failures)


# ---- pipeline level -------------------------------------------------------------------------------------------------------------------
_CHILD = r'''
import sys, json, importlib
sys.path[:0] = [ROOT, ROOT + "/tests", ROOT + "/oracle"]
import numpy as np
import mesh_census as M
import recip_systems as R
snb = importlib.import_module("openmm-nonbonded-slicing_amd")
name, prec = sys.argv[1], sys.argv[2]
row = M.by_name(name)
s = M.system(row)
fo, eo = R.oracle_eval(s)
tol = R.TOLS[prec]
eng = R.Engine(snb, s, prec, padding=M.PADDING, interval=M.INTERVAL)
out = dict(forces=[], energies=[])
def forces(what, f):
    rec = R.compare(s, f, fo, tol)
    out["forces"].append(dict(what=what, ok=bool(rec["ok"] and np.isfinite(f).all()), worst=rec["max_err"], median=rec["median_err"], report=R.report(rec)))
def energies(what, se):
    ok, worst = R.compare_energies(se, eo, tol)
    out["energies"].append(dict(what=what, ok=bool(ok and np.isfinite(se).all()), worst=float(worst)))
f, se, e = eng.step_energy_forces()
st = eng.stats()
out.update(stamps=[int(x) for x in st.n_kernel_timed], grid=[int(x) for x in st.grid], host=int(st.n_host_rebuilds))
forces("energy + forces step", f); energies("energy + forces step", se)
for k in range(2):
    forces("forces-only step %d" % k, eng.step_forces())
energies("energy-only step", eng.step_energy_only())
st = eng.stats()
out.update(rebuilds=int(st.n_rebuilds), overruns=int(st.n_list_overruns), strays=int(st.n_spread_strays))
eng.close()
print("RESULT " + json.dumps(out))
'''


def run_row(name, prec, timeout=240):
    """The case in a child process: (result dict, the engine's coulomb mesh lines)."""
    row = M.by_name(name)
    e = {k: v for k, v in os.environ.items() if not k.startswith("SNB_")}
    e["SNB_VERBOSE"] = "1"; e.update(row["env"])
    r = subprocess.run([sys.executable, "-c", "ROOT = %r\n" % S.ROOT + _CHILD, name, prec], env=e, capture_output=True, text=True, timeout=timeout)
    assert r.returncode == 0, (name, prec, r.returncode, r.stderr[-3000:])
    res = json.loads([l for l in r.stdout.splitlines() if l.startswith("RESULT ")][-1][7:])
    return res, [l for l in r.stderr.splitlines() if l.startswith("[snb] coulomb mesh ")]


def check_row(name, prec, res, lines):
    """Every assertion of a pipeline case; returns the failures as text."""
    row = M.by_name(name)
    plan = M.plan(row, prec)
    bad = []
    for rec in res["forces"]:
        print("%s %s %s: forces worst %.2e median %.2e | %s" % (name, prec, rec["what"], rec["worst"], rec["median"], rec["report"]))
        if not rec["ok"]:
            bad.append("%s: %s" % (rec["what"], rec["report"]))
    for rec in res["energies"]:
        print("%s %s %s: slice energies worst %.2e" % (name, prec, rec["what"], rec["worst"]))
        if not rec["ok"]:
            bad.append("%s: slice energies off by %.2e" % (rec["what"], rec["worst"]))
    t = res["stamps"]
    print("%s %s: stamps %s; %s" % (name, prec, t, lines[:1]))
    if tuple(res["grid"]) != row["grid"]:
        bad.append("mesh %s, not the row's" % res["grid"])
    if res["host"] != 0 or res["rebuilds"] != 1 or res["overruns"] != 0:
        bad.append("lists: host rebuilds %d, rebuilds %d, overruns %d" % (res["host"], res["rebuilds"], res["overruns"]))
    if prec != "double" and plan["path"] != row["path"]:
        bad.append("the table's plan for this row is %s, the row says %s" % (plan["path"], row["path"]))
    if not (t[1] > 0 and t[4] > 0 and t[7] > 0):
        bad.append("no spreader, x / plane kernel or interpolation stamp: %s" % t)
    if plan["path"] == "plane" and not (t[2] > 0 and t[3] == 0 and t[5] == 0):
        bad.append("not the plane path behind the merge kernel: %s" % t)
    if plan["path"] == "three-pass" and not (t[3] > 0 and t[5] > 0 and t[2] > 0):
        bad.append("not the three-pass pipeline: %s" % t)
    if not lines:
        bad.append("no mesh line")
    else:
        l = lines[0]
        cx, cy = plan["cells"]
        want = ["mesh %d x %d x %d: " % row["grid"], "of %d x %d cells, " % (cx, cy), M.mesh_line_tail(row)]
        want.append(("own-atoms spreader planned (slabs %d, margin 1)" % plan["slabs"]) if plan["own"] else ("scanning brick spreader" if plan["bricks"] else "atomic spreader"))
        for w in want:
            if w not in l:
                bad.append("mesh line lacks %r: %s" % (w, l))
    return bad


MIXED = ("S64", "P5")          # a square plane and a rectangular one
CASES = [(r["name"], p) for r in M.ROWS for p in ("single", "double")] + [(n, "mixed") for n in MIXED]


@pytest.mark.parametrize("name,prec", CASES, ids=["%s-%s" % c for c in CASES])
def test_row(name, prec):
    res, lines = run_row(name, prec)
    bad = check_row(name, prec, res, lines)
    assert not bad, "\n".join(bad)
