"""Context binding (-m gpu): snb_bind_context / snb_context_order_changed (include/snb.h, ABI 7).  The caller names a GPU context's own
buffers once -- posq in the context's reordered atom order with its atom-index permutation, the 64-bit fixed-point force buffer
([3][padded_n], 2^32 per kJ/mol/nm, added to), the energy and energy-parameter-derivative accumulators -- and a step is snb_set_box +
snb_execute: no staging buffer, no kernel outside the step, no host synchronisation.

The tests build the context's view with torch: a seeded random permutation, posq[slot] = (pos[atom_index[slot]], junk), padded_n = N
rounded up to 32 plus 64, the force buffer pre-filled with seeded int64 values P (|P| <= 2^40).  Delivered force of user atom u =
(buf - P)[d, slot(u)] / 2^32.  Tolerances against the oracle are the suite's (tests/test_gpu_pipeline.py TOL); bound against unbound in
mixed precision is held to 2 units of 2^-32 per component for |F| < 1e5 kJ/mol/nm: each path rounds once at the 2^-32 level, and the
double sum of the fixed-point and reciprocal parts carries < 2^-53 |F| 2^32 < 1 unit there."""
import ctypes
import json
import os
import re
import subprocess
import sys
import time

import numpy as np
import pytest

import bench
import systems

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOL = {"single": 1e-3, "mixed": 1e-3, "double": 1e-5}
FIXED = 4294967296.0
UNITS = 2                      # bound vs unbound, mixed precision, in units of 2^-32 (see the module docstring)
FMAX = 1e5


class View:
    """A context's buffers for `pos` ([N][3], user order), all on torch's current stream."""

    def __init__(self, pos, isd, seed, n_derivs=0, energy_double=True):
        import torch
        self.torch = torch
        n = self.n = len(pos)
        g = torch.Generator().manual_seed(seed)
        self.dt = torch.float64 if isd else torch.float32
        self.isd = isd
        self.atom_index = torch.randperm(n, generator=g).to(torch.int32).cuda()
        self.padded = (n + 31) // 32 * 32 + 64
        self.posq = torch.randn((self.padded, 4), generator=g).to(self.dt).cuda() * 50.0      # junk in .w and in the padding records
        self.posq[:n, :3] = torch.as_tensor(np.asarray(pos), dtype=self.dt).cuda()[self.atom_index.long()]
        self.P = torch.randint(-(1 << 40), (1 << 40) + 1, (3, self.padded), generator=g, dtype=torch.int64).cuda()
        self.buf = self.P.clone()
        et = torch.float64 if energy_double else torch.float32
        self.energy_double = energy_double
        self.E0 = torch.tensor([1234.5], dtype=et).cuda()
        self.ebuf = self.E0.clone()
        self.D0 = (torch.arange(max(n_derivs, 1), dtype=et) * 3.0 + 17.0).cuda()
        self.dbuf = self.D0.clone()

    def binding(self, capi, deriv_slot=None, force=True, energy=True):
        b = capi.SnbContextBinding()
        b.posq = self.posq.data_ptr(); b.atom_index = self.atom_index.data_ptr(); b.is_double = int(self.isd); b.padded_n = self.padded
        b.force_buffer = self.buf.data_ptr() if force else None
        b.energy_buffer = self.ebuf.data_ptr() if energy else None
        if deriv_slot is not None:
            self._slots = np.ascontiguousarray(deriv_slot, dtype=np.int32)
            b.deriv_buffer = self.dbuf.data_ptr(); b.deriv_slot = self._slots.ctypes.data_as(ctypes.POINTER(ctypes.c_int32))
        b.energy_is_double = int(self.energy_double)
        return b

    def delivered_units(self):
        """(buf - P) mapped back to user order: int64 [N][3], in units of 2^-32 kJ/mol/nm."""
        torch = self.torch
        d = (self.buf - self.P)[:, :self.n]
        out = torch.empty((self.n, 3), dtype=torch.int64, device="cuda")
        out[self.atom_index.long()] = d.t()
        return out

    def delivered(self):
        return self.delivered_units().double().cpu().numpy() / FIXED

    def padding_untouched(self):
        return bool(self.torch.equal(self.buf[:, self.n:], self.P[:, self.n:]))


@pytest.fixture
def own(snb):
    """A stream of torch's own as the current stream for the test (the walk, the context's buffers and the engine share it, as in bench.py),
    and torch's default stream back in place afterwards: the tests that follow in the process must not inherit it."""
    import torch
    before = torch.cuda.current_stream()
    stream = torch.cuda.Stream()
    torch.cuda.set_stream(stream)
    try:
        yield stream
    finally:
        torch.cuda.synchronize()
        torch.cuda.set_stream(before)


def _ferr(f, fo):
    return float(np.max(np.linalg.norm(f - fo, axis=1) / np.maximum(np.linalg.norm(fo, axis=1), 1.0)))


def _rel(a, b):
    return abs(a - b) / max(abs(b), 1.0)


def _w24k():
    return bench.build_workload(24000, 6.2145, 4, np.random.default_rng(bench.SEED))


def _engine(snb, w, prec, interval=1 << 30, padding=0.1):
    import torch
    return bench.Engine(snb, w, 4, 54, 0, prec, 0, 0, 1, padding, interval, stream=torch.cuda.current_stream().cuda_stream)


# name, n, nsub, method, L, cutoff, pme, ljpme, switch, kmax
PARITY = [
    ("pme_24000_n4", 24000, 4, 4, 6.2145, 1.0, (2.6283, 54, 54, 54), None, False, None),
    ("ljpme_3000_n4", 3000, 4, 5, 3.2, 1.0, (2.6283, 28, 28, 28), (2.6283, 20, 20, 20), False, None),
    ("rf_switch_3000_n3", 3000, 3, 2, 3.2, 1.0, None, None, True, None),
    ("ewald_1500_n3", 1500, 3, 3, 2.6, 1.0, (2.6283, 0, 0, 0), None, False, (11, 11, 11)),
    ("nocutoff_60_n2", 60, 2, 0, 0.9, 1.0, None, None, False, None),
]


@pytest.mark.parametrize("prec", ["single", "mixed", "double"])
@pytest.mark.parametrize("case", PARITY, ids=[c[0] for c in PARITY])
def test_bound_step_matches_the_oracle(case, prec, snb, oracle):
    """One forces + energy step through the host layer (context.py bindContextBuffers): delivered forces, the energy added to the energy
    buffer and the derivatives added to the derivative buffer against oracle.evaluate; the 3 (padded_n - N) padding entries of the force
    buffer equal P bit for bit; posq is bit-identical before and after."""
    import torch
    name, n, nsub, method, L, cutoff, pme, ljpme, switch, kmax = case
    F = snb.SlicedNonbondedForce
    force, pos, box = systems.random_box(F, n, nsub, method, L, cutoff, pme=pme, ljpme=ljpme, switch=switch)
    okw = {}
    if kmax:
        force.ewaldKmax = kmax; okw["kmax"] = kmax
    o = oracle.evaluate(force, np.asarray(pos, dtype=float), box, None, True, True, **okw)
    system = snb.System()
    for _ in range(n):
        system.addParticle(1.0)
    system.setDefaultPeriodicBoxVectors(*np.asarray(box, dtype=float))
    system.addForce(force)
    ctx = snb.Context(system, precision=prec)
    kern = ctx._kernelFor(force)
    names = sorted(o["derivatives"])
    isd = prec == "double"
    v = View(pos, isd, 11, n_derivs=len(names))
    posq0 = v.posq.clone()
    torch.cuda.synchronize()
    kern.bindContextBuffers(v.posq.data_ptr(), v.atom_index.data_ptr(), v.padded, forceBuffer=v.buf.data_ptr(), energyBuffer=v.ebuf.data_ptr(),
                            derivBuffer=v.dbuf.data_ptr() if names else None, derivNames=names, posqIsDouble=isd, energyIsDouble=True)
    ctx.setPositions(np.zeros((n, 3)))      # (the host positions are not used while bound)
    st = ctx.getState(getEnergy=True, getForces=True, getParameterDerivatives=True)
    assert st.getPotentialEnergy() == 0.0      # as the reference's GPU kernels: everything stays on the device
    assert kern._lib.snb_synchronize(kern._h) == 0
    err = _ferr(v.delivered(), o["forces"])
    e = float(v.ebuf.cpu()[0] - v.E0.cpu()[0])
    d = (v.dbuf - v.D0).cpu().numpy()
    print("BOUND_PARITY %s %s force %.3g energy %.3g" % (name, prec, err, _rel(e, o["energy"])))
    assert err <= TOL[prec], err
    assert _rel(e, o["energy"]) <= TOL[prec], (e, o["energy"])
    for k, nm in enumerate(names):
        assert _rel(float(d[k]), o["derivatives"][nm]) <= TOL[prec], (nm, float(d[k]), o["derivatives"][nm])
    assert v.padding_untouched()
    assert torch.equal(v.posq.view(torch.int64 if isd else torch.int32), posq0.view(torch.int64 if isd else torch.int32))
    # the user-order read-back still works after a bound step
    f = np.zeros((n, 3))
    assert kern._lib.snb_get_forces(kern._h, f.ctypes.data_as(ctypes.c_void_p), 0, 1, 0) == 0
    assert _ferr(f, o["forces"]) <= TOL[prec]


def test_bound_and_unbound_engines_give_the_same_numbers(snb, own):
    """SNB_MIXED on the 24k workload: an unbound engine (snb_get_forces, double) and a bound one agree to UNITS of 2^-32 per component
    for |F| < 1e5; two bound runs of the same step give identical int64 buffers."""
    import torch
    w = _w24k(); n = len(w["q"])
    eng = _engine(snb, w, "mixed")
    pos = torch.tensor(w["pos"], dtype=torch.float32, device="cuda")
    fu = torch.zeros((n, 3), dtype=torch.float64, device="cuda")
    eng.set_positions_device(pos.data_ptr(), False); eng.execute(False); eng.forces_to(fu.data_ptr(), True); eng.sync()
    eng.close()
    runs = []
    for _ in range(2):
        v = View(w["pos"], False, 5)
        b = v.binding(snb.capi)
        e2 = _engine(snb, w, "mixed")
        e2.ok(e2.L.snb_bind_context(e2.h, ctypes.byref(b)))
        e2.execute(False); e2.sync()
        runs.append(v.delivered_units().clone())
        assert v.padding_untouched()
        e2.close()
    assert torch.equal(runs[0], runs[1])
    keep = fu.abs() < FMAX
    diff = ((fu * FIXED) - runs[0].double()).abs()[keep]
    print("BOUND_VS_UNBOUND max units %.3f over %d components" % (float(diff.max()), int(keep.sum())))
    assert float(diff.max()) <= UNITS


# ---- the step stream (child processes: the switches are read once per process) ----
STEPS, INTERVAL = 40, 8
_STREAM_SCRIPT = r'''
import sys, json, ctypes
import numpy as np, torch, importlib
sys.path[:0] = [ROOT, ROOT + "/tests", ROOT + "/oracle"]
import bench
import test_gpu_context_binding as T
snb = importlib.import_module("openmm-nonbonded-slicing_amd")
interval, reorder_at, out = int(sys.argv[1]), json.loads(sys.argv[2]), sys.argv[3]
STEPS = T.STEPS
own = torch.cuda.Stream(); torch.cuda.set_stream(own)
w = bench.build_workload(24000, 6.2145, 4, np.random.default_rng(bench.SEED))
n = len(w["q"]); S = 10
deriv_slices = (np.abs(w["lam"] - 1.0).max(axis=1) > 0).astype(np.int32)
slots = np.full((S, 2), -1, dtype=np.int32)
slots[deriv_slices != 0] = np.arange(2 * int(deriv_slices.sum()), dtype=np.int32).reshape(-1, 2)
walk_rng = np.random.default_rng(bench.SEED + 1)
walk = [torch.tensor(walk_rng.normal(0.0, 0.0015, (n, 3)), dtype=torch.float32, device="cuda") for _ in range(16)]
walk_sign = walk_rng.choice([-1.0, 1.0], size=1 << 16)
res = {}; arrays = {}
for mode in ["unbound", "bound"] + (["reordered"] if reorder_at else []):
    eng = bench.Engine(snb, w, 4, 54, 0, "mixed", 0, 0, 1, 0.1, interval, stream=torch.cuda.current_stream().cuda_stream)
    eng.set_energy_slices(deriv_slices)
    eng.set_timing_interval(5)
    hist = torch.zeros((STEPS, n, 3), dtype=torch.float64, device="cuda")
    phist = torch.zeros((STEPS, n, 3), dtype=torch.float32, device="cuda")
    dhist = torch.zeros((STEPS, 2 * S), dtype=torch.float64, device="cuda")
    pos = torch.tensor(w["pos"], dtype=torch.float32, device="cuda")
    if mode == "unbound":
        forces = torch.zeros((n, 3), dtype=torch.float64, device="cuda")
    else:
        v = T.View(w["pos"], False, 7, n_derivs=2 * S)
        b = v.binding(snb.capi, deriv_slot=slots)
        eng.ok(eng.L.snb_bind_context(eng.h, ctypes.byref(b)))
    torch.cuda.synchronize()
    for i in range(STEPS):
        if mode == "reordered" and i in reorder_at:      # the context re-sorts its atoms: new permutation, posq and the force buffer's contents moved with it
            new = torch.randperm(n, generator=torch.Generator().manual_seed(100 + i)).to(torch.int32).cuda()
            old = v.atom_index.long()
            upos = torch.empty((n, 4), dtype=v.dt, device="cuda"); upos[old] = v.posq[:n]
            uP = torch.empty((3, n), dtype=torch.int64, device="cuda"); uP[:, old] = v.P[:, :n]
            v.posq[:n] = upos[new.long()]; v.P[:, :n] = uP[:, new.long()]; v.buf.copy_(v.P)
            v.atom_index.copy_(new)
            eng.ok(eng.L.snb_context_order_changed(eng.h))
        step = walk[i % 16] * float(walk_sign[i])
        pos.add_(step)
        if mode == "unbound":
            eng.set_positions_device(pos.data_ptr(), False)
        else:
            v.posq[:n, :3] += step[v.atom_index.long()]      # in place, in context order
        if i % 5 == 4:
            eng.ok(eng.L.snb_execute(eng.h, 1, 2, 1, 1, None))
        else:
            eng.ok(eng.L.snb_execute(eng.h, 1, 0, 1, 1, None))
        if mode == "unbound":
            eng.forces_to(forces.data_ptr(), True); hist[i].copy_(forces * T.FIXED)
        else:
            hist[i].copy_(v.delivered_units().double()); v.buf.copy_(v.P)
            dhist[i].copy_(v.dbuf - v.D0); v.dbuf.copy_(v.D0)
        phist[i].copy_(pos)
    eng.sync(); torch.cuda.synchronize()
    st = eng.stats()
    res[mode] = dict(rebuilds=int(st.n_rebuilds), overruns=int(st.n_list_overruns), host_rebuilds=int(st.n_host_rebuilds))
    if mode != "unbound":
        res[mode]["padding_untouched"] = v.padding_untouched()
        res[mode]["posq_matches_walk"] = bool(torch.equal(v.posq[:n, :3], pos[v.atom_index.long()]))
    arrays[mode] = hist.cpu().numpy()
    if mode == "bound":
        arrays["pos"] = phist.cpu().numpy(); arrays["derivs"] = dhist.cpu().numpy()
    eng.close()
    sys.stderr.flush()
np.savez(out, slots=slots, **arrays)
print("RESULT " + json.dumps(res))
'''


def _run_stream(tmp_path, tag, interval, reorder_at, extra_env):
    out = str(tmp_path / (tag + ".npz"))
    env = {k: v for k, v in os.environ.items() if not k.startswith("SNB_")}
    env.update({"SNB_VERBOSE": "1"}); env.update(extra_env)
    r = subprocess.run([sys.executable, "-c", "ROOT = %r\n" % ROOT + _STREAM_SCRIPT, str(interval), json.dumps(reorder_at), out],
                       env=env, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, (tag, r.returncode, r.stderr[-3000:])
    res = json.loads([l for l in r.stdout.splitlines() if l.startswith("RESULT ")][-1][7:])
    with np.load(out) as z:
        arrays = {k: z[k] for k in z.files}
    return res, arrays, r.stderr


_ORACLE = {}


def _oracle_checks(w, arrays, steps):
    """Forces of `steps` and the derivative slice energies of the derivative steps among them, bound run against the oracle."""
    import hashlib
    worst_f = worst_d = 0.0
    slots = arrays["slots"]
    for i in steps:
        w2 = dict(w); w2["pos"] = np.ascontiguousarray(arrays["pos"][i], dtype=np.float64)
        key = hashlib.sha1(w2["pos"].tobytes()).hexdigest()      # (every run walks the same positions)
        if key not in _ORACLE:
            _ORACLE[key] = bench.oracle_eval(w2, 4, 54, 0)[:2]
        fo, so = _ORACLE[key]
        f = arrays["bound"][i] / FIXED
        keep = np.abs(fo).max(axis=1) < 2.0 ** 31      # (the fixed-point range, as in tests/test_gpu_pipeline.py)
        worst_f = max(worst_f, _ferr(f[keep], fo[keep]))
        if i % 5 == 4:
            for s in range(slots.shape[0]):
                for t in range(2):
                    if slots[s, t] >= 0:
                        worst_d = max(worst_d, _rel(float(arrays["derivs"][i][slots[s, t]]), float(so[s, t])))
    return worst_f, worst_d


def _units(a, b):
    """Largest difference in units of 2^-32 over the components whose force lies inside |F| < FMAX."""
    keep = np.abs(a) < FMAX * FIXED
    return float(np.abs(a - b)[keep].max())


@pytest.mark.parametrize("env", [{}, {"SNB_OVERLAP_MIN_TILES": "0"}], ids=["default", "overlapped"])
def test_bound_step_stream_fixed_interval_and_reordering(env, tmp_path, snb):
    """40 steps of an in-place random walk on posq, no synchronisation until the end, a rebuild every 8 executes (lists built beside the
    steps), every fifth step a derivative-only step: every step of the bound engine agrees with the unbound engine driven by the same walk
    to UNITS, with the same rebuild and overrun counts; the last step and the derivative steps match the oracle.  Then the same run with
    the context order re-drawn before executes 13 and 22 -- the second while a side build is pending -- mapped back to user order: every step
    equals the un-reordered run to UNITS, and the call itself rebuilt nothing."""
    w = _w24k()
    reorder_at = [13, 22]
    res, arr, stderr = _run_stream(tmp_path, "fixed", INTERVAL, reorder_at, env)
    un, bo, ro = res["unbound"], res["bound"], res["reordered"]
    assert bo["padding_untouched"] and ro["padding_untouched"] and bo["posq_matches_walk"] and ro["posq_matches_walk"]
    assert bo["rebuilds"] == un["rebuilds"] == ro["rebuilds"] and bo["rebuilds"] >= len(range(0, STEPS, INTERVAL)), res
    assert bo["overruns"] == un["overruns"] == ro["overruns"] and bo["host_rebuilds"] == 0, res
    per_step = [_units(arr["unbound"][i], arr["bound"][i]) for i in range(STEPS)]
    per_step_r = [_units(arr["bound"][i], arr["reordered"][i]) for i in range(STEPS)]
    print("BOUND_STREAM units vs unbound %.3f, reordered vs bound %.3f" % (max(per_step), max(per_step_r)))
    assert max(per_step) <= UNITS, per_step
    assert max(per_step_r) <= UNITS, per_step_r
    # the second re-draw fell where a side build was pending (third engine of the child: the last block of SNB_VERBOSE lines)
    started = [int(x) for x in re.findall(r"side build started after execute (\d+)", stderr)]
    taken = [int(x) for x in re.findall(r"side-built list in use from execute (\d+)", stderr)]
    assert any(a < 22 <= b and b - a <= INTERVAL for a in started for b in taken), (started, taken)
    wf, wd = _oracle_checks(w, arr, [STEPS - 1] + [i for i in range(STEPS) if i % 5 == 4][-2:])
    print("BOUND_STREAM oracle force %.3g derivative %.3g" % (wf, wd))
    assert wf <= TOL["mixed"] and wd <= TOL["mixed"], (wf, wd)


@pytest.mark.parametrize("env", [{}, {"SNB_OVERLAP_MIN_TILES": "0"}], ids=["default", "overlapped"])
def test_bound_step_stream_displacement_triggered(env, tmp_path, snb):
    """The same walk with rebuild_interval = -100: the step on which the watch's flag is seen depends on host timing, so the run is held
    against the oracle only -- the last step and every derivative step -- with no list overrun."""
    w = _w24k()
    res, arr, _ = _run_stream(tmp_path, "auto", -100, [], env)
    assert res["bound"]["overruns"] == 0 and res["bound"]["padding_untouched"] and res["bound"]["posq_matches_walk"], res
    wf, wd = _oracle_checks(w, arr, sorted(set([STEPS - 1] + [i for i in range(STEPS) if i % 5 == 4])))
    print("BOUND_AUTO oracle force %.3g derivative %.3g rebuilds %d" % (wf, wd, res["bound"]["rebuilds"]))
    assert wf <= TOL["mixed"] and wd <= TOL["mixed"], (wf, wd)


@pytest.mark.parametrize("energy_double", [True, False], ids=["double_buffers", "float_buffers"])
def test_energy_and_derivatives_on_the_device(energy_double, snb, own):
    """energy_buffer and deriv_buffer pre-filled with known values.  A mode-1 step with energy == NULL adds sum lambda E: against the same
    step's snb_get_slice_energies to 1e-12 relative (double) or 2 * 2^-23 * max(|E|, |E0|) (float: one rounding of the sum, one of the add),
    and against the oracle at TOL.  A mode-2 step adds each bound raw slice energy to its slot -- two (slice, term) pairs share slot 0 --
    and leaves energy_buffer bit-identical; an energy-only step does the same and leaves force_buffer bit-identical.  None of these
    calls synchronises: they return while a long torch kernel queued ahead of them is still running."""
    import torch
    w = _w24k(); S = 10
    lam = np.asarray(w["lam"]).reshape(S, 2)
    fo, so, _, _ = bench.oracle_eval(w, 4, 54, 0)
    need = (np.abs(lam - 1.0).max(axis=1) > 0).astype(np.int32)
    sl = [int(s) for s in np.nonzero(need)[0]]
    slots = np.full((S, 2), -1, dtype=np.int32)
    k = 1
    for s in sl:
        for t in range(2):
            slots[s, t] = k; k += 1
    slots[sl[0], 0] = 0; slots[sl[0], 1] = 0      # two pairs, one slot
    v = View(w["pos"], False, 9, n_derivs=k, energy_double=energy_double)
    eng = _engine(snb, w, "mixed")
    eng.set_energy_slices(need)
    eng.set_timing_interval(0)
    b = v.binding(snb.capi, deriv_slot=slots)
    eng.ok(eng.L.snb_bind_context(eng.h, ctypes.byref(b)))
    eng.execute(False); eng.sync()      # warm-up: the first execute rebuilds and reads its totals back
    # how long the queue-filler runs (measured once, synchronised)
    a = torch.randn((4096, 4096), device="cuda")
    def filler():
        x = a
        for _ in range(60):
            x = torch.mm(x, a) * 1e-3
        return x
    filler(); torch.cuda.synchronize()
    t0 = time.perf_counter(); filler(); torch.cuda.synchronize(); t_fill = time.perf_counter() - t0
    box = bench.workload_box(w)
    dp = box.ctypes.data_as(ctypes.POINTER(ctypes.c_double))

    def unsynchronised(calls):
        """Runs `calls` behind the filler; fails when they took as long as the filler although the stream had to be waited for."""
        keepalive = filler()
        t0 = time.perf_counter()
        calls()
        dt = time.perf_counter() - t0
        busy = not own.query()
        del keepalive
        if not busy:      # the stream has drained: the calls either blocked on it, or the host was slow -- tell by their duration
            assert dt < 0.5 * t_fill, "the calls took %.1f ms beside a %.1f ms queue: they synchronised" % (dt * 1e3, t_fill * 1e3)
        return busy

    # mode 1, forces + energy
    v.buf.copy_(v.P); v.ebuf.copy_(v.E0); v.dbuf.copy_(v.D0); torch.cuda.synchronize()
    seen = [unsynchronised(lambda: (eng.ok(eng.L.snb_set_box(eng.h, dp)), eng.ok(eng.L.snb_execute(eng.h, 1, 1, 1, 1, None))))]
    eng.sync()
    se = eng.slice_energies(S)
    want = float((lam * se).sum())
    got = float(v.ebuf.double().cpu()[0] - v.E0.double().cpu()[0])
    if energy_double:
        assert abs(got - want) <= 1e-12 * max(abs(want), abs(float(v.E0[0]))), (got, want)
    else:
        assert abs(got - want) <= 2 * 2.0 ** -23 * max(abs(want), abs(float(v.E0[0]))), (got, want)      # (the difference of the two floats is exact in double)
    assert _rel(got, float((lam * so).sum())) <= TOL["mixed"]
    assert _ferr(v.delivered(), fo) <= TOL["mixed"]
    # a derivative slot: the raw energy converted to the buffer's type (one rounding each) and added (one rounding each, of a partial sum of
    # at most three terms): float 4 roundings of 2^-24 on 3 x the largest term = 6 * 2^-23; double the same count of 2^-53, held to 1e-12
    rt = 1e-12 if energy_double else 6 * 2.0 ** -23

    def check_derivs(se_now, tag):
        d = (v.dbuf.double() - v.D0.double()).cpu().numpy()
        exp = np.zeros(k)
        for s in sl:
            for t in range(2):
                exp[slots[s, t]] += se_now[s, t]
        scale = np.maximum(np.maximum(np.abs(exp), np.abs(v.D0.double().cpu().numpy())), np.abs(se_now).max())
        assert np.all(np.abs(d - exp) <= rt * scale), (tag, d, exp)
        assert _rel(float(d[0]), float(so[sl[0], 0] + so[sl[0], 1])) <= TOL["mixed"], tag

    check_derivs(se, "mode 1")
    # mode 2, forces + derivatives: the energy buffer stays as it is
    v.buf.copy_(v.P); v.dbuf.copy_(v.D0); e_before = v.ebuf.clone(); torch.cuda.synchronize()
    seen.append(unsynchronised(lambda: (eng.ok(eng.L.snb_set_box(eng.h, dp)), eng.ok(eng.L.snb_execute(eng.h, 1, 2, 1, 1, None)))))
    eng.sync()
    assert torch.equal(v.ebuf, e_before)
    check_derivs(eng.slice_energies(S), "mode 2")
    assert _ferr(v.delivered(), fo) <= TOL["mixed"]
    # energy-only steps: the force buffer stays as it is
    for mode in (1, 2):
        v.dbuf.copy_(v.D0); v.ebuf.copy_(v.E0); f_before = v.buf.clone(); torch.cuda.synchronize()
        seen.append(unsynchronised(lambda: eng.ok(eng.L.snb_execute(eng.h, 0, mode, 1, 1, None))))
        eng.sync()
        assert torch.equal(v.buf, f_before), mode
        check_derivs(eng.slice_energies(S), "energy-only mode %d" % mode)
        got = float(v.ebuf.double().cpu()[0] - v.E0.double().cpu()[0])
        if mode == 1:
            assert _rel(got, float((lam * so).sum())) <= TOL["mixed"]
        else:
            assert got == 0.0
    print("BOUND_ENERGY calls returned with the queue still busy: %s (filler %.0f ms)" % (seen, t_fill * 1e3))
    eng.close()


def test_binding_contract(snb, own):
    """Invalid bindings are rejected before any kernel uses them; sharded engines refuse; snb_set_positions while bound is a state error;
    a bound force buffer and snb_set_force_output replace one another; after an unbind and snb_set_positions the engine gives the forces it
    gave unbound."""
    import torch
    capi = snb.capi
    w = _w24k(); n = len(w["q"])
    eng = _engine(snb, w, "mixed")
    pos = torch.tensor(w["pos"], dtype=torch.float32, device="cuda")
    f0 = torch.zeros((n, 3), dtype=torch.float64, device="cuda")
    eng.set_positions_device(pos.data_ptr(), False); eng.execute(False); eng.forces_to(f0.data_ptr(), True); eng.sync()
    v = View(w["pos"], False, 3)
    torch.cuda.synchronize()
    bind = lambda b: eng.L.snb_bind_context(eng.h, ctypes.byref(b))
    b = v.binding(capi); b.padded_n = n - 1
    assert bind(b) == capi.SNB_ERR_INVALID_ARGUMENT
    b = v.binding(capi); b.posq = None
    assert bind(b) == capi.SNB_ERR_INVALID_ARGUMENT
    b = v.binding(capi); b.atom_index = None
    assert bind(b) == capi.SNB_ERR_INVALID_ARGUMENT
    dup = v.atom_index.clone(); dup[5] = dup[6]; torch.cuda.synchronize()      # one in-range duplicate: not a permutation
    b = v.binding(capi); b.atom_index = dup.data_ptr()
    assert bind(b) == capi.SNB_ERR_INVALID_ARGUMENT
    assert b"permutation" in eng.L.snb_last_error(eng.h)
    assert eng.L.snb_context_order_changed(eng.h) == capi.SNB_ERR_STATE      # nothing is bound
    # still unbound and unharmed
    f1 = torch.zeros_like(f0); eng.execute(False); eng.forces_to(f1.data_ptr(), True); eng.sync()
    assert torch.equal(f0, f1)
    b = v.binding(capi)
    assert bind(b) == capi.SNB_OK
    assert eng.L.snb_set_positions(eng.h, ctypes.c_void_p(pos.data_ptr()), 1, 0, 0) == capi.SNB_ERR_STATE
    eng.execute(False); eng.sync()
    assert float(((f0 * FIXED) - v.delivered_units().double()).abs()[f0.abs() < FMAX].max()) <= UNITS
    # a force output set while bound takes the place of the bound force buffer: user-order floats there, the fixed-point buffer left alone
    out = torch.zeros((n, 3), dtype=torch.float64, device="cuda")
    v.buf.copy_(v.P); torch.cuda.synchronize()
    eng.set_force_output(out.data_ptr(), True, 0)
    eng.execute(False); eng.sync()
    assert torch.equal(v.buf, v.P) and torch.equal(out, f0)
    # ... and binding a force buffer again takes the place of the force output; a binding without one delivers no forces at all
    out.zero_(); torch.cuda.synchronize()
    assert bind(v.binding(capi)) == capi.SNB_OK
    eng.execute(False); eng.sync()
    assert float(out.abs().max()) == 0.0 and not torch.equal(v.buf, v.P)
    v.buf.copy_(v.P); torch.cuda.synchronize()
    assert bind(v.binding(capi, force=False)) == capi.SNB_OK
    eng.execute(False); eng.sync()
    f3 = torch.zeros_like(f0); eng.forces_to(f3.data_ptr(), True); eng.sync()
    assert torch.equal(v.buf, v.P) and torch.equal(f3, f0)
    assert eng.L.snb_bind_context(eng.h, None) == capi.SNB_OK
    eng.set_positions_device(pos.data_ptr(), False)
    f2 = torch.zeros_like(f0); eng.execute(False); eng.forces_to(f2.data_ptr(), True); eng.sync()
    assert torch.equal(f0, f2)
    eng.close()
    sh = bench.Engine(snb, w, 4, 54, 0, "mixed", 0, 0, 2, 0.1, 20, stream=torch.cuda.current_stream().cuda_stream)
    b = v.binding(capi)
    assert sh.L.snb_bind_context(sh.h, ctypes.byref(b)) == capi.SNB_ERR_UNSUPPORTED
    sh.close()
