"""The reciprocal-space census on the GPU (-m gpu): the HIP engine evaluated with include_direct = 0, include_reciprocal = 1 against the oracle
evaluated the same way, on cells with three unequal lengths under meshes of three unequal sizes (tests/recip_systems.py; the instrument is proven
on the CPU in tests/test_recip_census.py).  Bars: 1e-3 single / mixed, 1e-5 double.  Slice energies |dE| <= tol max(|E|, 1) on every slice and
both terms; forces |dF_i| <= tol max(|F_rec,i|, F_med) on every atom, F_med the oracle's median reciprocal force over the atoms on the mesh.
Every case also takes one full step (direct + reciprocal) at the suite's total-scale rule."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import recip_systems as R
import shell_systems as S

pytestmark = pytest.mark.gpu

PRECISIONS = ("single", "mixed", "double")
# (system, precision, host_neighbor_build): every system on the builder the engine chooses, the triclinic ones on the host builder as well
CASES = [(n, p, 0) for n in R.SYSTEMS for p in PRECISIONS] + [(n, p, 1) for n in R.FORCED_HOST for p in PRECISIONS]
DRIFT = np.array([0.012, 0.011, 0.010])          # per step; two steps: 0.038 nm, with the jitter under skin / 2 = 0.05
_FRAMES = {}


def _drift_frames(s):
    """Two frames after a common translation plus a small jitter each (float coordinates): atoms cross mesh-cell, brick and column borders
    while the sorted order of the first step stays in use."""
    if s["name"] not in _FRAMES:
        rng = np.random.default_rng(3)
        frames, pos = [], s["pos"]
        for _ in range(2):
            pos = S.to_float(pos + rng.uniform(-0.003, 0.003, pos.shape) + DRIFT)
            f = dict(s); f["pos"] = pos
            frames.append(f)
        assert np.linalg.norm(frames[1]["pos"] - s["pos"], axis=1).max() < 0.05
        _FRAMES[s["name"]] = frames
    return _FRAMES[s["name"]]


def _recip_ok(s, f, se, prec, what, failures):
    fo, eo = R.oracle_eval(s)
    assert (f is None or np.isfinite(f).all()) and (se is None or np.isfinite(se).all()), (what, "NaN")
    if f is not None:
        rec = R.compare(s, f, fo, R.TOLS[prec])
        print("%s %s %s: forces %s" % (s["name"], prec, what, R.report(rec)))
        if not rec["ok"]:
            failures.append("%s, %s: %s" % (what, prec, R.report(rec)))
    if se is not None:
        ok, worst = R.compare_energies(se, eo, R.TOLS[prec])
        print("%s %s %s: slice energies worst %.2e" % (s["name"], prec, what, worst))
        if not ok:
            failures.append("%s, %s: slice energies off by %.2e\n%s\n%s" % (what, prec, worst, se, eo))
        if s["name"] == "subsets5":
            assert all((se[R.sl(3, j)] == 0).all() for j in range(5)), ("the slices of the empty subset must be exactly 0", se)


@pytest.mark.parametrize("name,prec,host_build", CASES, ids=["%s%s-%s" % (n, "-host" if h else "", p) for n, p, h in CASES])
def test_census(name, prec, host_build, snb):
    """Reciprocal-only: without a skin an energy + forces + derivatives step (the raw slice energies are the dE/dlambda of every slice); with a
    skin of 0.1 nm and a list life of ten steps four forces-only steps (eager, captured, replayed twice), an energy-only step and two steps
    after a drift of 0.02 nm each without a re-sort.  Then one full step against the oracle's total at the suite's rule.  No atom is exempt.
    host_build: lists from the host builder, which gives the triclinic cell no sort columns -- its meshes are spread with global atomics."""
    s = R.build(name)
    tol = R.TOLS[prec]
    host = name in R.HOST_BUILT or bool(host_build)
    failures = []
    # 1. no skin
    eng = R.Engine(snb, s, prec, host_build=host_build)
    f, se, e = eng.step_energy_forces()
    st = eng.stats()
    pipe, stamps = R.pipeline(st, s["method"])
    print("%s%s %s: pipeline: %s; stamps %s; mesh %s / %s; host rebuilds %d" % (name, " (host builder)" if host_build else "", prec, pipe, stamps, list(st.grid), list(st.dgrid), st.n_host_rebuilds))
    _recip_ok(s, f, se, prec, "no skin, energy + forces step", failures)
    _, eo = R.oracle_eval(s)
    assert abs(e - (s["lam"] * eo).sum()) <= tol * (np.abs(s["lam"]) * np.maximum(np.abs(eo), 1.0)).sum(), (e, (s["lam"] * eo).sum())
    if s["method"] != 3:
        assert tuple(st.grid) == s["grid"] and (s["method"] != 5 or tuple(st.dgrid) == s["dgrid"]), (list(st.grid), list(st.dgrid))
    _check_pipeline(name, prec, stamps, host_build)
    # 3. one full step, on the same engine
    eng.direct = 1
    f, se, e = eng.step_energy_forces()
    ft, et = R.oracle_eval(s, direct=True)
    ok, worst, atom = R.compare_total(s, f, ft, tol)
    eok, eworst = R.compare_energies(se, et, tol)
    print("%s %s full step: forces worst %.2e of max(|F_total|, 1) (atom %d), slice energies %.2e" % (name, prec, worst, atom, eworst))
    if not (ok and eok):
        failures.append("full step, %s: forces %.2e (atom %d), slice energies %.2e" % (prec, worst, atom, eworst))
    assert (st.n_host_rebuilds > 0) == host and eng.stats().n_list_overruns == 0, (int(st.n_host_rebuilds), host)
    eng.close()
    # 2. skin 0.1, a rebuild every tenth step
    eng = R.Engine(snb, s, prec, padding=0.1, interval=10, host_build=host_build)
    for k in range(4):
        _recip_ok(s, eng.step_forces(), None, prec, "skin, forces-only step %d" % k, failures)
    _recip_ok(s, None, eng.step_energy_only(), prec, "skin, energy-only step", failures)
    for k, fr in enumerate(_drift_frames(s)):
        eng.set_frame(fr)
        f = eng.step_forces() if k == 0 else eng.step_energy_forces()[0]
        _recip_ok(fr, f, eng.slice_energies() if k else None, prec, "skin, drift step %d" % k, failures)
    st = eng.stats()
    print("%s %s skin: rebuilds %d, host %d, strays %d, overruns %d" % (name, prec, st.n_rebuilds, st.n_host_rebuilds, st.n_spread_strays, st.n_list_overruns))
    assert st.n_rebuilds == 1 and st.n_list_overruns == 0 and st.n_host_rebuilds == (1 if host else 0), (int(st.n_rebuilds), int(st.n_list_overruns), int(st.n_host_rebuilds))
    eng.close()
    assert not failures, "\n".join(failures)


# What the stamp slots of the first (eager) step must show, as tests/test_gpu_parity.py reads them: slot 2 is the merge kernel of the own-atoms
# spreader or a forward z pass of its own -- the atomic spreader always has one; it stays empty only when the brick spreader did the z pass
# itself; slot 4 is the x kernel or the plane
# kernel, slots 3 and 5 the y passes of the three-pass pipeline -- absent on the plane path, which only single-precision arithmetic has and
# only the own-atoms spreader feeds: no y passes means that this spreader ran, not merely that it was planned.  Slots 8 .. 15: the same for the dispersion mesh.
# (on lists of the GPU builder: the host builder gives the triclinic cell no sort columns, hence no own-atoms spreader and no plane path)
PLANE_PATH = ("ortho", "ortho_ljpme_tiling", "ortho_ljpme_fallback", "unwrapped", "on_mesh", "subsets5", "triclinic_unequal", "triclinic_unequal_ljpme", "blob")
_SWITCHED = ("SNB_NO_FUSED_Z", "SNB_NO_OWN_SPREAD", "SNB_OWN_SLABS", "SNB_FFT_TWOPASS", "SNB_NO_PLANE_FFT", "SNB_NO_RECT_PLANES")


def _check_pipeline(name, prec, t, host_build=0):
    if name == "ortho_ewald":
        assert sum(t[1:8]) == 0, t
        return
    assert t[1] > 0 and t[4] > 0 and t[7] > 0, t
    if any(k in os.environ for k in _SWITCHED):
        return
    if name in PLANE_PATH and not host_build and prec != "double":
        assert t[2] > 0 and t[3] == 0 and t[5] == 0, ("own-atoms spreader and plane path on rectangular planes (40 x 54; the ball: 60 x 64)", t)
    if prec == "double":
        assert t[3] > 0 and t[5] > 0, ("three-pass pipeline", t)
    if name == "ortho_ljpme_fallback" or host_build:          # (the atomic spreader never does the z pass itself)
        o = 8 if name == "ortho_ljpme_fallback" else 0
        assert t[o + 1] > 0 and t[o + 2] > 0 and t[o + 3] > 0 and t[o + 5] > 0, ("atomic spreader, z pass of its own, three-pass pipeline", t)


def test_axis_permutations_on_the_engine(snb):
    """`ortho` in double precision, evaluated three times with the axes permuted cyclically (positions, cell, mesh): x is the slab / sort
    axis, y the other column axis, z the line axis, so each length and each mesh size takes each role.  Forces, permuted back, and slice
    energies must agree within the double bar; no oracle involved."""
    s = R.build("ortho")
    got = []
    for k in range(3):
        t = R.permuted(s, k)
        eng = R.Engine(snb, t, "double")
        f, se, _ = eng.step_energy_forces()
        st = eng.stats()
        assert tuple(st.grid) == t["grid"] and st.n_host_rebuilds == 0
        eng.close()
        got.append((R.permuted_back(f, k), se))
    for k in (1, 2):
        rec = R.compare(s, got[k][0], got[0][0], R.TOLS["double"])
        ok, worst = R.compare_energies(got[k][1], got[0][1], R.TOLS["double"])
        print("permutation %d: %s; slice energies %.2e" % (k, R.report(rec), worst))
        assert rec["ok"] and ok, (k, R.report(rec), worst)


_CHILD = r'''
import sys, json, importlib
sys.path[:0] = [ROOT, ROOT + "/tests", ROOT + "/oracle"]
import numpy as np
import recip_systems as R
snb = importlib.import_module("openmm-nonbonded-slicing_amd")
mode, prec = sys.argv[1], sys.argv[2]
out = {}
for arg in sys.argv[3:]:
    name, host_build = arg.split(":")[0], int(":" in arg)
    sys.stderr.write("SYSTEM %s\n" % arg); sys.stderr.flush()
    s = R.build(name)
    eng = R.Engine(snb, s, prec, padding=0.1, interval=10, host_build=host_build)
    f, se, _ = eng.step_energy_forces()
    st = eng.stats()
    out[arg] = dict(stamps=[int(x) for x in st.n_kernel_timed], host=int(st.n_host_rebuilds), finite=bool(np.isfinite(f).all() and np.isfinite(se).all()))
    if mode == "compare":
        fo, eo = R.oracle_eval(s)
        steps = []
        for k in range(3):
            rec = R.compare(s, f, fo, R.TOLS[prec])
            steps.append(dict(ok=rec["ok"], report=R.report(rec)))
            f = eng.step_forces()
        eok, eworst = R.compare_energies(se, eo, R.TOLS[prec])
        out[arg].update(steps=steps, energies_ok=eok, energies_worst=eworst)
    eng.close()
print("RESULT " + json.dumps(out))
'''


def _child(mode, prec, names, env):
    e = {k: v for k, v in os.environ.items() if not k.startswith("SNB_")}
    e["SNB_VERBOSE"] = "1"; e.update(env)
    r = subprocess.run([sys.executable, "-c", "ROOT = %r\n" % S.ROOT + _CHILD, mode, prec] + list(names), env=e, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    res = json.loads([l for l in r.stdout.splitlines() if l.startswith("RESULT ")][-1][7:])
    lines = {}
    cur = None
    for l in r.stderr.splitlines():
        if l.startswith("SYSTEM "):
            cur = l[7:]; lines[cur] = []
        elif cur and " mesh " in l and l.startswith("[snb]"):
            lines[cur].append(l)
    return res, lines


@pytest.mark.parametrize("switch", ["SNB_NO_OWN_SPREAD", "SNB_NO_FUSED_Z", "SNB_NO_PLANE_FFT", "SNB_NO_FIXED_SPREAD"])
def test_alternative_kernels(switch):
    """`ortho`, single precision, reciprocal-only, under the switches that select the other spreaders and the three-pass pipeline (read once
    per process: child processes): an energy + forces step and two forces-only steps against the oracle.  That the switch took effect is read
    from the stamp slots of the first step: without a switch `ortho` runs the own-atoms spreader (slot 2: its merge kernel) and behind it the
    plane path (no y passes in slots 3 / 5) -- test_census asserts that.  The brick spreader that SNB_NO_OWN_SPREAD selects does the z pass of a
    5 x 6 x 48 brick itself (6 KB of brick and 13 KB of FFT buffers in LDS), so slot 2 stays empty.  SNB_NO_FIXED_SPREAD changes the accumulator of the same kernels from fixed
    point to double, which no stamp shows: for that switch parity is all there is to check."""
    res, _ = _child("compare", "single", ["ortho"], {switch: "1"})
    r = res["ortho"]
    t = r["stamps"]
    print(switch, t, [s["report"] for s in r["steps"]], r["energies_worst"])
    assert all(s["ok"] for s in r["steps"]) and r["energies_ok"], r
    assert t[1] > 0 and t[4] > 0 and t[7] > 0 and r["host"] == 0, t
    if switch == "SNB_NO_OWN_SPREAD":
        assert t[2] == 0 and t[3] > 0 and t[5] > 0, ("the brick spreader with the z pass fused, which does not feed the plane path", t)
    if switch == "SNB_NO_FUSED_Z":
        assert t[2] > 0 and t[3] > 0 and t[5] > 0, ("own-atoms spreader, z pass of its own, so no plane path", t)
    if switch == "SNB_NO_PLANE_FFT":
        assert t[2] > 0 and t[3] > 0 and t[5] > 0, t
    if switch == "SNB_NO_FIXED_SPREAD":
        assert t[2] > 0 and t[3] == 0 and t[5] == 0, ("the same kernels as without a switch", t)


def test_every_system_reaches_the_kernels_it_is_there_for():
    """The spreader planned for every mesh, from the engine's own account of it at the rebuild (SNB_VERBOSE), beside the stamp slots of the
    step that followed -- one child process, one energy + forces step per system in single precision, no comparison (test_census makes those):
    sort columns of 5 x 6 cells with the own-atoms spreader, a dispersion mesh in bricks of 2 x 3 columns, one that does not tile the columns
    (atomic spreader), a z line of 260 points (scanning brick spreader), the bricks of the ball, and the triclinic cell on both builders: the
    GPU builder cuts it into sort columns and bricks like a rectangular one, the host builder leaves it without, which is the fallback to global
    atomics on both meshes.  Sort columns and bricks settle atomic against brick kernels for good; the own-atoms spreader is planned at the
    rebuild and can still be declined at the launch -- that it ran is seen where the plane path follows it (no y-pass stamps: `ortho` here,
    and every single and mixed case of test_census on that mesh); elsewhere the line is the plan."""
    names = list(R.SYSTEMS) + [n + ":host" for n in R.FORCED_HOST]
    res, lines = _child("plan", "single", names, {})
    first = lambda name, mesh: next(l for l in lines[name] if "%s mesh" % mesh in l)
    for name, r in res.items():
        print(name, r["stamps"], lines.get(name))
        assert r["finite"], name
        assert (r["host"] > 0) == (name in R.HOST_BUILT or name.endswith(":host")), (name, r["host"])
    l = first("ortho", "coulomb")
    assert "mesh 40 x 54 x 48: sort columns 8 x 9 of 5 x 6 cells" in l and "bricks of 1 x 1 columns, own-atoms spreader planned" in l, l
    t = res["ortho"]["stamps"]
    assert t[2] > 0 and t[3] == 0 and t[5] == 0, ("the planned own-atoms spreader ran: the plane path followed it", t)
    l = first("ortho_ljpme_tiling", "dispersion")
    assert "mesh 24 x 27 x 24" in l and "bricks of 2 x 3 columns, own-atoms spreader planned" in l, l
    assert "atomic spreader" in first("ortho_ljpme_fallback", "dispersion") and "own-atoms spreader planned" in first("ortho_ljpme_fallback", "coulomb")
    for mesh in ("coulomb", "dispersion"):
        l = first("triclinic_unequal_ljpme:host", mesh)
        assert "sort columns 0 x 0" in l and "atomic spreader" in l, l
        assert "bricks of" in first("triclinic_unequal_ljpme", mesh)          # (the GPU builder: sort columns in fractional coordinates)
    l = first("triclinic_unequal:host", "coulomb")
    assert "sort columns 0 x 0" in l and "atomic spreader" in l, l
    l = first("long_z", "coulomb")
    assert "mesh 25 x 25 x 260" in l and "of 5 x 5 cells" in l and "scanning brick spreader" in l, l
    l = first("blob", "coulomb")
    assert "sort columns 6 x 8 of 10 x 8 cells" in l and "own-atoms spreader planned" in l, l
    l = first("ortho_small", "coulomb")
    assert "sort columns 2 x 5 of 10 x 5 cells" in l, l
    assert lines.get("ortho_ewald", []) == []
