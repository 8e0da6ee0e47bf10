"""The step stream as bench.py drives it (-m gpu): coordinates moved in place on torch's stream, snb_execute + snb_get_forces, no
synchronisation until the end, a fixed rebuild interval whose lists are built beside the steps (engine.hip startSideBuild /
finishSideBuild) and replayed step graphs brought up to date with hipGraphExecUpdate while earlier launches may still be queued.

test_unfenced_steps_match_fenced_steps_bit_for_bit runs that stream on the 24k workload in child processes (the switches are read once
per process, and a child that faults does not take pytest with it) under the engine's switch sets, and holds it against the same
steps fenced, against the other switch sets and against the oracle.  test_bench_last_timed_step_matches_the_oracle runs bench.py itself
and checks what its last timed step computed (--dump-outputs) against the oracle at full size.  Tolerances: 1e-3 single / mixed, 1e-5
double, relative with the reference's max(|x|, 1) scaling (openmmapi/include/internal/AssertionUtilities.h:7-26)."""
import hashlib
import json
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import bench
import parity_tools as pt

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOL = {"single": 1e-3, "mixed": 1e-3, "double": 1e-5}
SUMMARY = r"rebuilds: (\d+), of them (\d+) built beside the steps; (\d+) side builds discarded"

# The 24k run: a rebuild every 8 executes over 55 steps -> rebuilds at 0, 8, ..., 48.  The first one waits for its padded count; the
# second is sized by a prediction from the first, which this walk exceeds (31168 padded atoms against 30560: repeated in line with the
# exact count), so the third is sized by a new prediction, in line too (engine.hip sideBuildPossible: only a list built with the predicted
# count in use may be followed by a side build).  24, 32, 40 and 48 are built beside the steps (started `sideLead` executes early) and
# exchanged at those steps.  Every fifth step (4, 9, ..., 54) is a derivative-only step, the last one included.
STEPS, INTERVAL = 55, 8
REBUILDS = list(range(0, STEPS, INTERVAL))
EXCHANGES = [24, 32, 40, 48]
DERIVATIVE = [i for i in range(STEPS) if i % 5 == 4]
# the last step on an old list, every rebuild after the first and the step after it, every derivative step, the final step
CHECK = sorted(set([r - 1 for r in REBUILDS[2:]] + REBUILDS[1:] + [r + 1 for r in REBUILDS[1:]] + DERIVATIVE + [STEPS - 1]))

_PIPE_SCRIPT = r'''
import sys, json, hashlib
import numpy as np, torch, importlib
sys.path[:0] = [ROOT, ROOT + "/tests", ROOT + "/oracle"]
import bench
snb = importlib.import_module("openmm-nonbonded-slicing_amd")
prec, modes, out = sys.argv[1], sys.argv[2].split(","), sys.argv[3]
STEPS, INTERVAL, CHECK, config = int(sys.argv[4]), int(sys.argv[5]), json.loads(sys.argv[6]), sys.argv[7]
own = torch.cuda.Stream(); torch.cuda.set_stream(own)      # a stream of torch's own for the walk and the engine, as bench.py has
n_target, Lbox, nsub, method, grid, dgrid, _ = bench.CONFIGS[config]
w = bench.build_workload(n_target, Lbox, nsub, np.random.default_rng(bench.SEED))
n = len(w["q"]); isd = prec == "double"; dt = torch.float64 if isd else torch.float32
S = 10
deriv_slices = (np.abs(w["lam"] - 1.0).max(axis=1) > 0).astype(np.int32)
walk_rng = np.random.default_rng(bench.SEED + 1)      # bench.py's random walk: sixteen fixed fields, a sign per step
walk = [torch.tensor(walk_rng.normal(0.0, 0.0015, (n, 3)), dtype=dt, device="cuda") for _ in range(16)]
walk_sign = walk_rng.choice([-1.0, 1.0], size=1 << 16)
pos0 = torch.tensor(w["pos"], dtype=dt, device="cuda")
res = {}; arrays = {}
for mode in modes:
    fenced = mode == "fenced"
    eng = bench.Engine(snb, w, method, grid, dgrid, prec, 0, 0, 1, 0.1, INTERVAL, stream=torch.cuda.current_stream().cuda_stream)
    pos = pos0.clone()
    forces = torch.zeros((n, 3), dtype=dt, device="cuda")
    hist = torch.zeros((STEPS, n, 3), dtype=dt, device="cuda"); phist = torch.zeros((STEPS, n, 3), dtype=dt, device="cuda")
    eng.set_force_output(forces.data_ptr(), isd)
    eng.set_energy_slices(deriv_slices)
    eng.set_timing_interval(5)      # eager stamped steps between the replayed ones
    torch.cuda.synchronize()
    for i in range(STEPS):
        pos.add_(walk[i % 16], alpha=float(walk_sign[i]))
        eng.set_positions_device(pos.data_ptr(), isd)
        if i % 5 == 4:
            eng.execute(2, fetch=False)
        else:
            eng.execute(False)
        eng.forces_to(forces.data_ptr(), isd)
        hist[i].copy_(forces); phist[i].copy_(pos)      # (stream order: what this step computed, from the positions it saw)
        if fenced:
            eng.sync(); torch.cuda.synchronize()
    eng.sync(); torch.cuda.synchronize()
    se = eng.slice_energies(S)
    st = eng.stats()
    h = hist.cpu().numpy()
    res[mode] = dict(sha=[hashlib.sha1(h[i].tobytes()).hexdigest() for i in range(STEPS)], rebuilds=int(st.n_rebuilds),
                     host_rebuilds=int(st.n_host_rebuilds), overruns=int(st.n_list_overruns))
    if not arrays:
        arrays = dict(forces=h[CHECK], pos=phist.cpu().numpy()[CHECK], energies=se[deriv_slices != 0])
    eng.close()
    sys.stderr.flush()
np.savez(out, **arrays)
print("RESULT " + json.dumps(res))
'''

# Switch sets (the engine's own test switches, engine.hip).  SNB_OVERLAP_MIN_TILES=0 under all of them: the 24k list has far fewer tiles
# than the threshold below which the overlapped step is skipped, and the bench workload runs overlapped.
BASE_ENV = {"SNB_OVERLAP_MIN_TILES": "0", "SNB_VERBOSE": "1"}
SWITCH_SETS = {
    "default": {},
    "no_graph_update": {"SNB_NO_GRAPH_UPDATE": "1"},
    "eager_rebuild_step": {"SNB_EAGER_REBUILD_STEP": "1"},
    "publish_copy": {"SNB_NB_PUBLISH_WAIT_MS": "0"},
    "no_overlap": {"SNB_OVERLAP": "0"},
    "side_lead_1": {"SNB_SIDE_LEAD": "1"},
    "side_reject": {"SNB_SIDE_REJECT": "1"},
    "inline": {"SNB_SIDE_REBUILD": "0"},
}
# the same lists from the same positions: bit for bit the default's forces.  SNB_OVERLAP=0 (one launch of the tile kernel after the
# reciprocal pipeline instead of two beside it) belongs here too: mixed precision sums forces in 64-bit fixed point, so the order in
# which launches claim work items does not show
SAME_LISTS = ("no_graph_update", "eager_rebuild_step", "publish_copy", "no_overlap")
# lists built from other positions (the lead-1 build copies the positions one step before the exchange, a discarded side build and the
# in-line rebuild use those of the exchange step itself, the default those three steps before): another sort order, other image offsets,
# other float rounding of the pair displacements.  Measured on MI355X against the default over the checked steps, relative to
# max(|F|, 1): 2.2e-4 (lead 1) and 2.7e-4 (discarded / in line) raw, 5.8e-5 and 5.7e-5 once each atom is allowed the force of its
# truncation-band pairs -- the worst atom has no band pair: its net force is the small remainder of large pair forces, each computed in
# float from displacements rounded another way.  The bound is 3.5 times that, five times under the oracle tolerance; a pair dropped from
# a list moves an atom by far more.  The raw spread (band pairs taken by one list and not the other) is held to 3.7 times its measured
# value, so that a list dropping pairs near the cutoff shows there too.
OTHER_LISTS = ("side_lead_1", "side_reject", "inline")
CROSS_LIST_TOL = 2e-4
CROSS_LIST_RAW_TOL = 1e-3


def _child_env(extra):
    e = {k: v for k, v in os.environ.items() if not k.startswith("SNB_")}      # nothing but the switches of the case
    e.update(BASE_ENV); e.update(extra)
    return e


def _run_child(prec, modes, extra, tmp_path, tag, config="small", steps=STEPS, interval=INTERVAL, check=CHECK):
    out = str(tmp_path / ("%s.npz" % tag))
    r = subprocess.run([sys.executable, "-c", "ROOT = %r\n" % ROOT + _PIPE_SCRIPT, prec, ",".join(modes), out, str(steps), str(interval), json.dumps(check), config],
                       env=_child_env(extra), capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, (tag, r.returncode, r.stderr[-3000:])
    res = json.loads([l for l in r.stdout.splitlines() if l.startswith("RESULT ")][-1][7:])
    summaries = re.findall(SUMMARY, r.stderr)
    assert len(summaries) == len(modes), (tag, r.stderr[-2000:])
    for mode, (rebuilds, side, discarded) in zip(modes, summaries):
        res[mode]["summary"] = dict(rebuilds=int(rebuilds), side=int(side), discarded=int(discarded))
    with np.load(out) as z:
        arrays = {k: z[k] for k in z.files}
    return res, arrays, r.stderr


_ORACLE = {}
_BAND = {}


def _oracle(w, pos):
    """Oracle forces and slice energies of the 24k workload at these positions (cached: every switch set walks the same positions)."""
    key = hashlib.sha1(np.ascontiguousarray(pos, dtype=np.float64).tobytes()).hexdigest()
    if key not in _ORACLE:
        w2 = dict(w); w2["pos"] = np.ascontiguousarray(pos, dtype=np.float64)
        fo, so, _, _ = bench.oracle_eval(w2, 4, 54, 0)
        _ORACLE[key] = (fo, so)
    return _ORACLE[key]


def _oracle_errors(w, arrays, deriv_slices):
    """Worst force error over the checked steps (step by step) and the error of the final step's derivative slice energies."""
    ferr = {}
    for k, step in enumerate(CHECK):
        fo, so = _oracle(w, arrays["pos"][k])
        f = arrays["forces"][k].astype(np.float64)
        ferr[step] = float(np.max(np.linalg.norm(f - fo, axis=1) / np.maximum(np.linalg.norm(fo, axis=1), 1.0)))
    so = _oracle(w, arrays["pos"][CHECK.index(STEPS - 1)])[1][deriv_slices != 0]
    eerr = float(np.max(np.abs(arrays["energies"] - so) / np.maximum(np.abs(so), 1.0)))
    return ferr, eerr


def _cross_list_spread(w, pos, fa, fb):
    """Largest force difference between two runs on other lists over the checked steps, relative to max(|F|, 1): raw, after each atom's
    truncation-band allowance, and over the atoms without a band pair.  The lists place an atom at other image offsets, so a pair whose
    r^2 lies within float rounding of cutoff^2 (tests/parity_tools.py) may be taken by one run and not by the other."""
    raw = excess = outside = 0.0
    for k in range(len(CHECK)):
        key = hashlib.sha1(np.ascontiguousarray(pos[k], dtype=np.float64).tobytes()).hexdigest()
        if key not in _BAND:
            w2 = dict(w); w2["pos"] = np.ascontiguousarray(pos[k], dtype=np.float64)
            _BAND[key] = pt.band_allowance(w2, 4, 54, 0, pt.band_rel(w2, "mixed"))[0]
        allow = _BAND[key]
        err = np.linalg.norm(fb[k] - fa[k], axis=1); den = np.maximum(np.linalg.norm(fa[k], axis=1), 1.0)
        raw = max(raw, float((err / den).max()))
        excess = max(excess, float((np.maximum(err - allow, 0.0) / den).max()))
        outside = max(outside, float((err / den)[allow == 0].max()))
    return raw, excess, outside


def test_unfenced_steps_match_fenced_steps_bit_for_bit(tmp_path, snb):
    """bench.py's timed loop on the 24k workload (PME 54^3), mixed precision, a rebuild every 8 executes: four list exchanges beside the
    steps, derivative-only steps every fifth step, eager stamped steps every fifth execute.  Each switch set runs the 55 steps twice in one
    child -- unfenced (no synchronisation until the end) and fenced (eng.sync + torch.cuda.synchronize after every step) -- on fresh
    engines, keeping every step's forces on the device.

    * Fenced and unfenced: every step bit for bit (64-bit fixed-point force sums; both build their lists from the same stream-ordered
      snapshot of the positions, so a fence must not change a bit).
    * Switch sets that build the same lists from the same positions (SAME_LISTS): bit for bit the default's steps.
    * Switch sets that build from other positions (OTHER_LISTS): within CROSS_LIST_TOL of max(|F|, 1) of the default after the band
      allowance (measured 5.8e-5, see OTHER_LISTS), within CROSS_LIST_RAW_TOL without it; a discarded side build repeated in line gives the in-line run bit for bit.
    * The checked steps (the last step on an old list, every exchange and the step after it, every derivative step, the final step) and
      the final derivative slice energies against the oracle at 1e-3.
    * Rebuild counts: exactly the seven the interval implies, none on the host, no list overrun; four side builds taken (or, with
      SNB_SIDE_REJECT, four discarded; in line, none).  With SNB_NB_PUBLISH_WAIT_MS=0 the totals of every side build were read through
      the fallback copy on the side-build stream (engine.hip waitForTotals).
    Then single and double precision with the default switches, unfenced, against the oracle (single-precision float atomics are not
    bitwise reproducible: no digests)."""
    w = bench.build_workload(24000, 6.2145, 4, np.random.default_rng(bench.SEED))
    deriv_slices = (np.abs(w["lam"] - 1.0).max(axis=1) > 0).astype(np.int32)
    got, arr, report = {}, {}, {}
    for tag, extra in SWITCH_SETS.items():
        res, arrays, stderr = _run_child("mixed", ["unfenced", "fenced"], extra, tmp_path, tag)
        got[tag], arr[tag] = res, arrays
        un, fe = res["unfenced"], res["fenced"]
        first = next((i for i in range(STEPS) if un["sha"][i] != fe["sha"][i]), None)
        assert first is None, "%s: unfenced step %d differs from the fenced one (rebuilds at %s)" % (tag, first, REBUILDS)
        for mode in ("unfenced", "fenced"):
            m = res[mode]
            assert m["host_rebuilds"] == 0 and m["overruns"] == 0, (tag, mode, m)
            assert m["rebuilds"] == len(REBUILDS) and m["summary"]["rebuilds"] == len(REBUILDS), (tag, mode, m)
            want = (0, 0) if tag == "inline" else ((0, len(EXCHANGES)) if tag == "side_reject" else (len(EXCHANGES), 0))
            assert (m["summary"]["side"], m["summary"]["discarded"]) == want, (tag, mode, m["summary"])
        if tag == "publish_copy":
            copies = re.findall(r"copied on the side-build stream", stderr)
            assert len(copies) == 2 * len(EXCHANGES), (tag, stderr[-2000:])      # (both modes: every exchange read its totals through the copy)
        ferr, eerr = _oracle_errors(w, arrays, deriv_slices)
        report[tag] = dict(worst_force_err=max(ferr.values()), worst_step=max(ferr, key=ferr.get), energy_err=eerr)
        assert all(e < TOL["mixed"] for e in ferr.values()), (tag, ferr)
        assert eerr < TOL["mixed"], (tag, eerr)
    ref = got["default"]["unfenced"]["sha"]
    fd = arr["default"]["forces"].astype(np.float64)
    for tag in OTHER_LISTS:
        f = arr[tag]["forces"].astype(np.float64)
        raw, excess, outside = _cross_list_spread(w, arr["default"]["pos"], fd, f)
        report[tag].update(spread_raw=raw, spread_after_band_allowance=excess, spread_outside_band=outside)
        report[tag]["first_step_unlike_default"] = next((i for i in range(STEPS) if got[tag]["unfenced"]["sha"][i] != ref[i]), None)
    print("PIPELINE " + json.dumps(report))
    for prec in ("single", "double"):
        res, arrays, _ = _run_child(prec, ["unfenced"], {}, tmp_path, prec)
        m = res["unfenced"]
        assert m["host_rebuilds"] == 0 and m["overruns"] == 0 and m["rebuilds"] == len(REBUILDS), (prec, m)
        assert (m["summary"]["side"], m["summary"]["discarded"]) == (len(EXCHANGES), 0), (prec, m["summary"])
        ferr, eerr = _oracle_errors(w, arrays, deriv_slices)
        report[prec] = dict(worst_force_err=max(ferr.values()), worst_step=max(ferr, key=ferr.get), energy_err=eerr)
        assert all(e < TOL[prec] for e in ferr.values()), (prec, ferr)
        assert eerr < TOL[prec], (prec, eerr)
        print("PIPELINE %s %s" % (prec, json.dumps(report[prec])))
    for tag in SAME_LISTS:
        first = next((i for i in range(STEPS) if got[tag]["unfenced"]["sha"][i] != ref[i]), None)
        assert first is None, "%s: step %d differs from the default run" % (tag, first)
    for tag in OTHER_LISTS:
        assert report[tag]["spread_after_band_allowance"] <= CROSS_LIST_TOL and report[tag]["spread_outside_band"] <= CROSS_LIST_TOL, (tag, report[tag])
        assert report[tag]["spread_raw"] <= CROSS_LIST_RAW_TOL, (tag, report[tag])
    first = next((i for i in range(STEPS) if got["side_reject"]["unfenced"]["sha"][i] != got["inline"]["unfenced"]["sha"][i]), None)
    assert first is None, "side_reject: step %d differs from the in-line run" % first


def _bench_positions(w, dtype, warmup, steps):
    """The coordinates of bench.py's last timed step, rebuilt on the host by bench.py's own recipe: the sixteen walk fields and the
    sign table from SEED + 1, then the step indices in the order main() issues them -- fenced_step(0), the 250 - W preconditioning steps
    (1 << 20 | i), the warm-up steps 1..W, the timed steps W+1..W+K.  Float additions of +-field are exact to reproduce."""
    n = len(w["q"])
    rng = np.random.default_rng(bench.SEED + 1)
    walk = [rng.normal(0.0, 0.0015, (n, 3)).astype(dtype) for _ in range(16)]
    sign = rng.choice([-1.0, 1.0], size=1 << 16)
    pos = w["pos"].astype(dtype)
    order = [0] + [1 << 20 | i for i in range(max(0, 250 - warmup))] + list(range(1, warmup + 1)) + list(range(warmup + 1, warmup + steps + 1))
    for i in order:
        pos = pos + walk[i % 16] if sign[i % len(sign)] > 0 else pos - walk[i % 16]
    return pos


# bench.py issues 251 executes before its timed region -- fenced_step(0), 250 - W preconditioning steps, W warm-up steps: indices 0..250 --
# so timed step K is execute 250 + K.  With the default rebuild interval of 20 the lists change at every multiple of 20, built beside the
# steps from the third rebuild on: the positions are copied aside after execute 20 k - 4 and the build runs beside the three executes in
# between.  The child runs with SNB_VERBOSE, whose lines name the execute after which each side build starts and the execute at which its
# list takes over.  (name, extra arguments, W, K, rebuilds in the timed region)
BENCH_RUNS = [
    # execute 280: the last timed step is the one at which the side-built list takes over
    ("c3_single_exchange_step", [], 10, 30, 2),
    # execute 279: the last step on the old list, with the next one built beside it
    ("c3_mixed_last_step_on_old_list", ["--precision", "mixed"], 10, 29, 1),
]
BENCH_INTERVAL, SIDE_LEAD = 20, 3
# Mixed precision sums forces in 64-bit fixed point, 2^32 per kJ/mol/nm (as the reference's GPU platforms do): a sum beyond 2^31 kJ/mol/nm
# wraps.  bench.py's walk moves every atom on its own and by execute 279 has pushed a few solute atoms to 0.036 nm of a non-excluded
# neighbour, with forces of 1e11 kJ/mol/nm; those atoms, and only those, are left out of the mixed-precision comparison.
FIXED_POINT_RANGE = 2.0 ** 31


def test_bench_last_timed_step_matches_the_oracle(tmp_path, snb):
    """bench.py itself (plain run, --dump-outputs) on c3 -- 300k atoms, 4 subsets, PME 120^3, derivative steps -- with the step counts
    chosen so that its last timed step is a list-exchange step (single precision) and the last step on the oldest list (mixed).  Its
    forces and derivative slice energies against the oracle at the positions of that step, rebuilt on the host, at 1e-3 with the
    truncation-band allowance of tests/parity_tools.py, as test_gpu_fullsize.py does; in mixed precision over every atom but those whose
    force lies beyond the fixed-point range (FIXED_POINT_RANGE).  The walk also pulls some excluded partners within picometres of each
    other (778 atoms within 0.02 nm by execute 280, the closest pair 0.0008 nm apart): their exclusion correction is held to the
    tolerance like every other force (direct.hip exclusionG).  Measured on MI355X: exchange step (single) 2.6e-4 forces and
    2.6e-5 slice energies; last step on the old list (mixed) 2.5e-4 and 7.6e-6, 2 atoms beyond the fixed-point range left out."""
    n_target, Lbox, nsub, method, grid, dgrid, _ = bench.CONFIGS["c3"]
    w = bench.build_workload(n_target, Lbox, nsub, np.random.default_rng(bench.SEED))
    deriv_slices = (np.abs(w["lam"] - 1.0).max(axis=1) > 0).astype(np.int32)
    report = {}
    for name, extra, warmup, steps, rebuilds in BENCH_RUNS:
        prec = "mixed" if "mixed" in extra else "single"
        out = tmp_path / name
        cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--config", "c3", "--warmup", str(warmup), "--steps", str(steps),
               "--dump-outputs", str(out)] + extra
        r = subprocess.run(cmd, env=_child_env({}), cwd=ROOT, capture_output=True, text=True, timeout=900)      # (SNB_VERBOSE: BASE_ENV)
        assert r.returncode == 0, (name, r.returncode, r.stderr[-3000:])
        line = json.loads([l for l in r.stdout.splitlines() if l.startswith("{")][-1])
        c = line["config"]
        assert c["rebuild_beside_steps"] is True and c["host_rebuilds"] == 0, (name, c)
        assert c["rebuilds_in_timed_region"] == rebuilds, (name, c["rebuilds_in_timed_region"])
        last = 250 + steps
        taken = [int(x) for x in re.findall(r"side-built list in use from execute (\d+)", r.stderr)]
        started = [int(x) for x in re.findall(r"side build started after execute (\d+)", r.stderr)]
        assert taken and started, (name, r.stderr[-2000:])
        if last % BENCH_INTERVAL == 0:      # the last timed step is an exchange
            assert taken[-1] == last and started[-1] == last - SIDE_LEAD - 1, (name, taken, started)
        else:      # the last step on the old list: the list in use came in an interval ago, the next one is being built beside it
            assert (last + 1) % BENCH_INTERVAL == 0, (name, last)
            assert taken[-1] == last + 1 - BENCH_INTERVAL and started[-1] == last - SIDE_LEAD, (name, taken, started)
        f = np.load(out / "forces.npy").astype(np.float64)
        se = np.load(out / "derivative_slice_energies.npy")
        w2 = dict(w); w2["pos"] = np.ascontiguousarray(_bench_positions(w, np.float32, warmup, steps).astype(np.float64))
        fo, so, _, _ = bench.oracle_eval(w2, method, grid, dgrid)
        fa, ea, nband = pt.band_allowance(w2, method, grid, dgrid, pt.band_rel(w2, prec))
        sel = deriv_slices != 0
        keep = np.ones(len(fo), dtype=bool)
        if prec == "mixed":
            keep = np.abs(fo).max(axis=1) < FIXED_POINT_RANGE
            assert (~keep).sum() <= 16, (name, int((~keep).sum()))
        rec = pt.compare(f[keep], se, fo[keep], so[sel], TOL[prec], fa[keep], ea[sel])
        err = np.linalg.norm(f - fo, axis=1) / np.maximum(np.linalg.norm(fo, axis=1), 1.0)
        rec.update(band_pairs=nband, exempt_atoms=int((~keep).sum()), max_force_rel_err_exempt=float(err[~keep].max()) if (~keep).any() else 0.0)
        report[name] = rec
        print("BENCH_ORACLE %s %s" % (name, json.dumps(rec)))
        assert rec["ok"], (name, rec)
        assert rec["max_force_rel_err_outside_band"] <= TOL[prec], (name, rec)


def test_fallback_totals_copy_waits_for_the_side_build_at_full_size(tmp_path, snb):
    """The fallback read of a side build's totals (engine.hip waitForTotals, forced by SNB_NB_PUBLISH_WAIT_MS=0) on c3 -- 300k atoms, mixed
    precision, a rebuild every 20 executes -- with the side build started one execute ahead (SNB_SIDE_LEAD=1), where it is still running
    when the rebuild falls due.  Unfenced against fenced, bit for bit over 61 steps.  Measured on MI355X before the copy was moved to the
    side-build stream: on the live stream it read tiles 0, work items 0 + 0, overflow 0 at the exchange of execute 40, the list was taken
    into use with no tiles, and every step until the next rebuild lost its pair forces."""
    res, _, stderr = _run_child("mixed", ["unfenced", "fenced"], {"SNB_NB_PUBLISH_WAIT_MS": "0", "SNB_SIDE_LEAD": "1"}, tmp_path, "c3_copy",
                                config="c3", steps=61, interval=20, check=[])
    un, fe = res["unfenced"], res["fenced"]
    first = next((i for i in range(61) if un["sha"][i] != fe["sha"][i]), None)
    assert first is None, "unfenced step %d differs from the fenced one" % first
    for mode in ("unfenced", "fenced"):
        m = res[mode]
        assert m["host_rebuilds"] == 0 and m["overruns"] == 0 and m["summary"]["rebuilds"] == 4, (mode, m)
        assert res[mode]["summary"]["side"] >= 1, (mode, res[mode]["summary"])
    side = re.findall(r"copied on the side-build stream \(tiles (\d+), work items (\d+) \+ (\d+), overflow (\d+), padded (\d+)\)", stderr)
    assert len(side) >= 2 and all(int(t) > 0 and int(a) + int(b) > 0 and int(p) >= 300000 for t, a, b, _, p in side), side
