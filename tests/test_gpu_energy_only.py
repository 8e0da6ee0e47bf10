"""Energy-only evaluations (-m gpu): snb_execute with include_forces == 0 (include/snb.h).  Such a step produces the slice energies
(all of them, or the slices of snb_set_energy_slices in mode 2) with the energy-only kernels -- no force arithmetic, no force stores, no
inverse transforms or interpolation on the reciprocal side -- and leaves the forces of the last forces step readable (across a rebuild
of its own, too) and the force output buffer exactly as they were; it never captures or updates a step graph itself."""
import ctypes

import numpy as np
import pytest

import bench
import parity_tools as pt
import systems

pytestmark = pytest.mark.gpu

TOLS = {"single": 1e-3, "double": 1e-5, "mixed": 1e-3}
# energy-only against the same engine's energy step at the same positions.  The slice sums are double atomics whose order changes from run to
# run; on the cross slices whose direct and reciprocal halves cancel that order alone moves a double-precision slice by ~1e-12 of max(|E|, 1)
# (seen: 1.05e-12 on the 24k box), so double is held to 1e-11
SAME_STEP = {"single": 1e-6, "mixed": 1e-6, "double": 1e-11}
K_SPREAD, K_FFT_Y_INV, K_FFT_Z_INV, K_INTERPOLATE = 1, 5, 6, 7


def _w24k():
    return bench.build_workload(24000, 6.2145, 4, np.random.default_rng(bench.SEED))


def _dev(a, isd):
    import torch
    return torch.tensor(np.asarray(a), dtype=torch.float64 if isd else torch.float32, device="cuda")


def _energy_only(eng, mode=1):
    eng.ok(eng.L.snb_execute(eng.h, 0, mode, 1, 1, None))


def _rel(a, b):
    return float(np.max(np.abs(a - b) / np.maximum(np.abs(b), 1.0)))


def _at(w, pos, scale=1.0):
    """The workload with other coordinates (and the box scaled by `scale`), for the oracle."""
    v = dict(w); v["pos"] = np.ascontiguousarray(pos, dtype=np.float64); v["L"] = w["L"] * scale
    return v


@pytest.mark.parametrize("prec", ["single", "mixed", "double"])
def test_energy_only_step_leaves_forces_and_force_output_alone(prec, snb):
    """A force output registered with accumulate = 1 is not added to by an energy-only step, and snb_get_forces still returns the forces
    of the last forces step, bit for bit."""
    import torch
    w = _w24k(); n = len(w["q"]); isd = prec == "double"
    eng = bench.Engine(snb, w, 4, 54, 0, prec, 0, 0, 1, 0.1, 1 << 30)
    p1 = _dev(w["pos"], isd)
    p2 = p1 + 0.01 * torch.randn(p1.shape, generator=torch.Generator(device="cuda").manual_seed(3), device="cuda", dtype=p1.dtype)
    out = torch.full((n, 3), 7.25, dtype=p1.dtype, device="cuda")
    eng.set_force_output(out.data_ptr(), isd, 1)
    eng.set_positions_device(p1.data_ptr(), isd); eng.execute(False); eng.sync()
    assert not torch.equal(out, torch.full_like(out, 7.25))      # the forces step did add to it
    before = out.clone()
    f1 = torch.zeros((n, 3), dtype=p1.dtype, device="cuda"); eng.forces_to(f1.data_ptr(), isd); eng.sync()
    eng.set_positions_device(p2.data_ptr(), isd)
    for mode in (1, 2):
        _energy_only(eng, mode); eng.sync()
        assert torch.equal(out, before), mode
        f2 = torch.zeros_like(f1); eng.forces_to(f2.data_ptr(), isd); eng.sync()
        assert torch.equal(f1, f2), mode
    assert np.isfinite(eng.slice_energies(10)).all()
    eng.close()


@pytest.mark.parametrize("method,dgrid", [(4, 0), (5, 27)])
def test_energy_only_steps_run_no_inverse_chain(method, dgrid, snb):
    """Per-kernel stamps of timed energy-only steps: the spreader runs, the inverse y / z transforms and the interpolation of either mesh
    do not.  (A forces step afterwards stamps the interpolation: the slots do work.)"""
    w = _w24k()
    eng = bench.Engine(snb, w, method, 54, dgrid, "single", 0, 0, 1, 0.1, 1 << 30)
    pos = _dev(w["pos"], False)
    eng.set_positions_device(pos.data_ptr(), False)
    eng.execute(False); eng.sync()
    eng.set_timing_interval(1); eng.reset_timers()
    for _ in range(4):
        _energy_only(eng, 1)
    st = eng.stats()
    assert st.n_kernel_timed[K_SPREAD] > 0
    for k in (K_FFT_Y_INV, K_FFT_Z_INV, K_INTERPOLATE):
        assert st.n_kernel_timed[k] == 0 and st.n_kernel_timed[k + 8] == 0, k
    if method == 5:
        assert st.n_kernel_timed[K_SPREAD + 8] > 0
    eng.reset_timers(); eng.execute(False)
    assert eng.stats().n_kernel_timed[K_INTERPOLATE] > 0
    eng.close()


@pytest.mark.parametrize("prec", ["single", "mixed", "double"])
@pytest.mark.parametrize("method,dgrid", [(2, 0), (4, 0), (5, 27)])
def test_energy_only_vs_oracle_24k(method, dgrid, prec, snb):
    """Energy-only mode 1 (total and every slice) and mode 2 (two selected slices) against the oracle on the bench's 24k-atom box (RF,
    PME, LJPME), and against the same engine's energy step at the same positions."""
    w = _w24k(); S = 10; isd = prec == "double"
    lam = np.asarray(w["lam"]).reshape(S, 2)
    fo, so, _, _ = bench.oracle_eval(w, method, 54, dgrid)
    eng = bench.Engine(snb, w, method, 54, dgrid, prec, 0, 0, 1, 0.1, 1 << 30)
    pos = _dev(w["pos"], isd)
    eng.set_positions_device(pos.data_ptr(), isd)
    _energy_only(eng, 1)
    se = eng.slice_energies(S)
    assert _rel(se, so) < TOLS[prec]
    etot, eo = float((lam * se).sum()), float((lam * so).sum())
    assert abs(etot - eo) / max(abs(eo), 1.0) < TOLS[prec]
    mask = np.zeros(S, dtype=np.int32); mask[[2, 9]] = 1
    eng.set_energy_slices(mask)
    _energy_only(eng, 2)
    sel = eng.slice_energies(S)
    assert _rel(sel[mask == 1], so[mask == 1]) < TOLS[prec]
    eng.set_energy_slices(np.ones(S, dtype=np.int32))
    e_full = eng.execute(True)      # the forces + energy step at the same positions
    sf = eng.slice_energies(S)
    assert _rel(se, sf) <= SAME_STEP[prec], (_rel(se, sf), se, sf)
    assert abs(etot - e_full) / max(abs(e_full), 1.0) <= SAME_STEP[prec]
    eng.close()


def test_ewald_energy_only_vs_oracle(snb, oracle):
    """Classic Ewald: structure factors and slice energies, no force pass (through the Python kernel)."""
    F = snb.SlicedNonbondedForce
    force, pos, box = systems.random_box(F, 1500, 3, 3, 2.6, 1.0, pme=(2.6283, 0, 0, 0))
    force.ewaldKmax = (11, 11, 11)
    want = oracle.evaluate(force, pos, box, kmax=(11, 11, 11))
    for prec in ("single", "mixed", "double"):
        ctx = _context(snb, force, pos, box, prec)
        kern = ctx._kernelFor(force)
        assert _rel(kern.computeSliceEnergies(ctx), want["slice_energies"]) < TOLS[prec]
        e = ctx.getState(getEnergy=True).getPotentialEnergy()
        assert abs(e - want["energy"]) / max(abs(want["energy"]), 1.0) < TOLS[prec]


def test_energy_only_steps_do_not_disturb_forces_steps(snb):
    """Mixed precision (bitwise reproducible forces), no timed steps, no rebuild inside the window: an engine that runs an energy-only step
    at other coordinates after every forces step gives the forces of an engine that runs only the forces steps, bit for bit -- its step
    graph is replayed, not dropped or re-captured.  With a fixed rebuild interval of 6 (side-built lists exchanged while energy-only steps
    are queued, and counted by them) both engines agree with the oracle on the last step."""
    import torch
    w = _w24k(); n = len(w["q"])
    g = torch.Generator(device="cuda").manual_seed(11)
    base = _dev(w["pos"], False)
    P = [base]
    for _ in range(7):
        P.append(P[-1] + 0.002 * torch.randn(base.shape, generator=g, device="cuda"))
    Q = [p + 0.02 * torch.randn(base.shape, generator=g, device="cuda") for p in P]
    for interval in (1 << 30, 6):
        A = bench.Engine(snb, w, 4, 54, 0, "mixed", 0, 0, 1, 0.3, interval)
        B = bench.Engine(snb, w, 4, 54, 0, "mixed", 0, 0, 1, 0.3, interval)
        for e in (A, B):
            e.set_timing_interval(0)
        fa = torch.zeros((n, 3), dtype=torch.float32, device="cuda"); fb = torch.zeros_like(fa)
        for k in range(8):
            A.set_positions_device(P[k].data_ptr(), False); A.execute(False); A.forces_to(fa.data_ptr(), False)
            B.set_positions_device(P[k].data_ptr(), False); B.execute(False); B.forces_to(fb.data_ptr(), False)
            B.set_positions_device(Q[k].data_ptr(), False); _energy_only(B, 1)
            A.sync(); B.sync()
            if interval > 8:
                assert torch.equal(fa, fb), k
        if interval == 6:
            fo, _, _, _ = bench.oracle_eval(_at(w, P[7].double().cpu().numpy()), 4, 54, 0)
            for f in (fa, fb):
                err = np.linalg.norm(f.double().cpu().numpy() - fo, axis=1) / np.maximum(np.linalg.norm(fo, axis=1), 1.0)
                assert err.max() < TOLS["mixed"], err.max()
        A.close(); B.close()


def test_barostat_trial_energy_only(snb):
    """A Monte Carlo barostat trial: box scaled by 1.005 with the coordinates, one energy-only step (a box change rebuilds the lists),
    then the box and coordinates restored and the MD step goes on."""
    import torch
    w = _w24k(); n = len(w["q"]); S = 10; s = 1.005
    fo, so, _, _ = bench.oracle_eval(w, 4, 54, 0)
    _, so2, _, _ = bench.oracle_eval(_at(w, w["pos"] * s, s), 4, 54, 0)
    eng = bench.Engine(snb, w, 4, 54, 0, "single", 0, 0, 1, 0.1, 1 << 30)
    pos = _dev(w["pos"], False); pos2 = _dev(w["pos"] * s, False)
    f = torch.zeros((n, 3), dtype=torch.float32, device="cuda")
    eng.set_positions_device(pos.data_ptr(), False); eng.execute(False); eng.sync()
    r0 = eng.stats().n_rebuilds
    box = bench.workload_box(w)
    dp = lambda a: a.ctypes.data_as(ctypes.POINTER(ctypes.c_double))
    box2 = np.ascontiguousarray(box * s)
    eng.ok(eng.L.snb_set_box(eng.h, dp(box2)))
    eng.set_positions_device(pos2.data_ptr(), False); _energy_only(eng, 1)
    assert eng.stats().n_rebuilds > r0
    assert _rel(eng.slice_energies(S), so2) < TOLS["single"]
    eng.ok(eng.L.snb_set_box(eng.h, dp(np.ascontiguousarray(box))))
    eng.set_positions_device(pos.data_ptr(), False); eng.execute(False); eng.forces_to(f.data_ptr(), False); eng.sync()
    err = np.linalg.norm(f.double().cpu().numpy() - fo, axis=1) / np.maximum(np.linalg.norm(fo, axis=1), 1.0)
    assert err.max() < TOLS["single"], err.max()
    eng.close()


def test_energy_only_c3_at_full_size(snb):
    """c3 (300k atoms, single precision): energy-only mode 1 and mode 2 against the oracle, with the truncation-band allowance of the
    full-size parity tests (tests/parity_tools.py)."""
    n_target, Lbox, nsub, method, grid, dgrid, _ = bench.CONFIGS["c3"]
    w, fo, so, _, _, fa, ea, _ = pt.fullsize_case("c3", "single")
    S = nsub * (nsub + 1) // 2
    eng = bench.Engine(snb, w, method, grid, dgrid, "single", 0, 0, 1, 0.1, 1 << 30)
    pos = _dev(w["pos"], False)
    eng.set_positions_device(pos.data_ptr(), False)
    _energy_only(eng, 1)
    se = eng.slice_energies(S)
    rec = pt.compare(fo, se, fo, so, TOLS["single"], fa, ea)
    assert rec["ok"], rec
    mask = np.zeros(S, dtype=np.int32); mask[[0, S - 1]] = 1
    eng.set_energy_slices(mask)
    _energy_only(eng, 2)
    sel = eng.slice_energies(S)
    sel[mask == 0] = so[mask == 0]
    rec = pt.compare(fo, sel, fo, so, TOLS["single"], fa, ea)
    assert rec["ok"], rec
    eng.close()


def _context(snb, force, pos, box, prec):
    system = snb.System()
    for _ in range(force.getNumParticles()):
        system.addParticle(1.0)
    system.setDefaultPeriodicBoxVectors(*box)
    system.addForce(force)
    ctx = snb.Context(system, precision=prec, device=0)
    ctx.setPositions(pos)
    return ctx


@pytest.mark.parametrize("prec", ["single", "double"])
def test_python_energy_only_paths(prec, snb, oracle):
    """computeSliceEnergies (all slices and a selection) and getState(getEnergy=True) followed by getState(getForces=True) give the
    oracle's energies and forces."""
    F = snb.SlicedNonbondedForce
    force, pos, box = systems.random_box(F, 3000, 4, F.PME, 3.2, 1.0, pme=(2.6283, 28, 28, 28))
    want = oracle.evaluate(force, pos, box)
    ctx = _context(snb, force, pos, box, prec)
    kern = ctx._kernelFor(force)
    tol = TOLS[prec]
    e = ctx.getState(getEnergy=True).getPotentialEnergy()
    assert abs(e - want["energy"]) / max(abs(want["energy"]), 1.0) < tol
    f = ctx.getState(getForces=True).getForces()
    err = np.linalg.norm(f - want["forces"], axis=1) / np.maximum(np.linalg.norm(want["forces"], axis=1), 1.0)
    assert err.max() < tol, err.max()
    assert _rel(kern.computeSliceEnergies(ctx), want["slice_energies"]) < tol
    sel = kern.computeSliceEnergies(ctx, slices=[1, 7])
    assert np.isnan(sel[[0, 2, 3, 4, 5, 6, 8, 9]]).all()
    assert _rel(sel[[1, 7]], want["slice_energies"][[1, 7]]) < tol
    f2 = ctx.getState(getForces=True).getForces()      # the selection did not stick: a full step after it
    assert np.abs(f2 - f).max() <= 1e-3 * max(1.0, np.abs(f).max())


def test_sharded_energy_only_steps_sum_to_the_oracle(snb):
    """Sharded engines (energies per rank, the meshes not lambda-mixed): the energy-only steps of the ranks add up to the oracle's slice
    energies, and each rank keeps the forces of its last forces step."""
    import torch
    w = bench.build_workload(12000, 4.932, 4, np.random.default_rng(bench.SEED))
    _, so, _, _ = bench.oracle_eval(w, 4, 42, 0)
    n = len(w["q"])
    pos = _dev(w["pos"], True)
    moved = pos + 0.002 * torch.randn(pos.shape, generator=torch.Generator(device="cuda").manual_seed(5), device="cuda", dtype=pos.dtype)      # (inside skin / 2: no rebuild)
    etot = np.zeros_like(so)
    for rank in range(2):
        eng = bench.Engine(snb, w, 4, 42, 0, "double", 0, rank, 2, 0.05, 1 << 30)
        f1 = torch.zeros((n, 3), dtype=torch.float64, device="cuda"); f2 = torch.zeros_like(f1)
        eng.set_positions_device(moved.data_ptr(), True); eng.execute(False); eng.forces_to(f1.data_ptr(), True)
        eng.set_positions_device(pos.data_ptr(), True); _energy_only(eng, 1)
        etot += eng.slice_energies(so.shape[0])
        eng.forces_to(f2.data_ptr(), True); eng.sync()
        assert torch.equal(f1, f2), rank
        eng.close()
    assert _rel(etot, so) < TOLS["double"]


def _box_to(eng, box):
    eng.ok(eng.L.snb_set_box(eng.h, np.ascontiguousarray(box, dtype=np.float64).ctypes.data_as(ctypes.POINTER(ctypes.c_double))))


def _host_forces(eng, n, isd):
    out = np.zeros((n, 3), dtype=np.float64 if isd else np.float32)
    eng.ok(eng.L.snb_get_forces(eng.h, out.ctypes.data_as(ctypes.c_void_p), 0, int(isd), 0))
    return out


@pytest.mark.parametrize("prec", ["single", "mixed", "double"])
def test_forces_survive_a_barostat_trial_rebuild(prec, snb):
    """Forces step at P1, read f1; a barostat trial -- box scaled by 1.005, coordinates scaled and moved (a barostat scales molecule
    centres), one energy-only step, whose box change rebuilds and re-sorts the atoms -- then the box restored: snb_get_forces returns f1 bit
    for bit, into a device and into a host buffer, also after a second trial; the next forces step replaces them."""
    import torch
    w = _w24k(); n = len(w["q"]); isd = prec == "double"; s = 1.005
    eng = bench.Engine(snb, w, 4, 54, 0, prec, 0, 0, 1, 0.1, 1 << 30)
    g = torch.Generator(device="cuda").manual_seed(7)
    p1 = _dev(w["pos"], isd)
    trials = [p1 * s + 0.03 * torch.randn(p1.shape, generator=g, device="cuda", dtype=p1.dtype) for _ in range(2)]
    box = bench.workload_box(w)
    eng.set_positions_device(p1.data_ptr(), isd); eng.execute(False)
    f1 = torch.zeros((n, 3), dtype=p1.dtype, device="cuda"); eng.forces_to(f1.data_ptr(), isd); eng.sync()
    h1 = _host_forces(eng, n, isd)
    for p2 in trials:
        r0 = eng.stats().n_rebuilds
        _box_to(eng, box * s); eng.set_positions_device(p2.data_ptr(), isd); _energy_only(eng, 1)
        assert eng.stats().n_rebuilds > r0
        _box_to(eng, box); eng.set_positions_device(p1.data_ptr(), isd)
        f2 = torch.zeros_like(f1); eng.forces_to(f2.data_ptr(), isd); eng.sync()
        assert torch.equal(f1, f2)
        assert np.array_equal(h1, _host_forces(eng, n, isd))
    eng.execute(False)      # (rebuilds: the box changed back)
    f3 = torch.zeros_like(f1); eng.forces_to(f3.data_ptr(), isd); eng.sync()
    a, b = f1.double().cpu().numpy(), f3.double().cpu().numpy()
    err = np.linalg.norm(a - b, axis=1) / np.maximum(np.linalg.norm(a, axis=1), 1.0)
    assert err.max() < 1e-4, err.max()      # same coordinates and box; only the list and the summation order may differ
    eng.close()


@pytest.mark.parametrize("interval,steps", [(3, 3), (6, 12)])
def test_forces_survive_a_fixed_interval_rebuild_in_an_energy_only_step(interval, steps, snb):
    """The rebuild of a fixed interval falls on an energy-only step: in line (interval 3), or, with interval 6 at the engine's third rebuild,
    as the exchange of a list built beside the steps.  snb_get_forces still returns the last forces step's forces, bit for bit."""
    import torch
    w = _w24k(); n = len(w["q"])
    g = torch.Generator(device="cuda").manual_seed(13)
    P = [_dev(w["pos"], False)]
    for _ in range(steps):
        P.append(P[-1] + 0.005 * torch.randn(P[0].shape, generator=g, device="cuda"))
    Q = P[steps] + 0.03 * torch.randn(P[0].shape, generator=g, device="cuda")
    eng = bench.Engine(snb, w, 4, 54, 0, "single", 0, 0, 1, 0.3, interval)
    eng.set_timing_interval(0)
    f = torch.zeros((n, 3), dtype=torch.float32, device="cuda")
    for k in range(steps):
        eng.set_positions_device(P[k].data_ptr(), False); eng.execute(False)
    eng.forces_to(f.data_ptr(), False); eng.sync()
    r0 = eng.stats().n_rebuilds
    eng.set_positions_device(Q.data_ptr(), False); _energy_only(eng, 1)
    f2 = torch.zeros_like(f); eng.forces_to(f2.data_ptr(), False); eng.sync()
    assert torch.equal(f, f2)
    if interval <= 4:
        assert eng.stats().n_rebuilds > r0
    eng.close()
