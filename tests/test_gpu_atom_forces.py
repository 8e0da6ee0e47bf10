"""Per-atom forces by partner subset and term (-m gpu): snb_evaluate_atom_forces (include/snb.h).

Ground truth is the oracle alone (tests/atom_force_truth.py): 2 S evaluations with lambda one-hot at (slice, term), whose forces on the
slice's two subsets are the two columns.  Truths do not depend on the precision mode: they are computed once per (workload, method) and
shared -- every precision, double included, is given the float-rounded coordinates (parity_tools.float_positions), so that engine and
oracle see identical inputs.  Tolerances are the project's TOLS under the reference's scale rule on 3-vectors,
||got - want|| / max(||want||, 1) per (atom, column, term).  Single and mixed precision allow an atom the force of ITS cutoff-band pairs
(parity_tools.band_allowance, lambdas all 1) on each of its columns; fewer than 1 % of the atoms may carry such a pair.
The 24k-atom box takes the GPU list builder, the brick spreader and the plane path; 60 atoms is below the builder's 64-atom floor and takes
the host lists and the per-pair-wrap kernels.  One-hot oracle evaluations at 24k atoms in this module: 3 x 20 (methods) + 12 (triclinic,
3 subsets) + 6 (lists in use, 2 subsets), plus 5 at the workloads' own lambdas."""
import ctypes

import numpy as np
import pytest

import atom_force_truth as aft
import bench
import parity_tools
import systems

pytestmark = pytest.mark.gpu

TOLS = {"single": 1e-3, "double": 1e-5, "mixed": 1e-3}
S4 = 10
METHODS = {"rf": (2, 54, 0), "pme": (4, 54, 0), "ljpme": (5, 54, 27)}


def _dev(a, isd):
    import torch
    return torch.tensor(np.asarray(a), dtype=torch.float64 if isd else torch.float32, device="cuda")


def _table(eng, n, nsub, direct=1, recip=1):
    out = np.full((n, nsub, 2, 3), np.nan)
    eng.ok(eng.L.snb_evaluate_atom_forces(eng.h, direct, recip, out.ctypes.data_as(ctypes.c_void_p), 0))
    return out


def _ones(w):
    v = dict(w)
    v["lam"] = np.ones_like(w["lam"])
    return v


class _Case:
    """One workload at float-rounded coordinates: truth tables, the oracle's forces at its own lambdas and the band allowance, per
    method, computed on first use and kept for the module."""

    def __init__(self, w):
        self.w = parity_tools.float_positions(w)
        self.nsub = w["nsub"]
        self._tables, self._forces, self._bands = {}, {}, {}

    def table(self, key):
        if key not in self._tables:
            m, g, dg = key
            self._tables[key] = aft.truth_table(aft.workload_evaluator(self.w, m, g, dg), self.w["subset"], self.nsub)
        return self._tables[key]

    def forces(self, key):
        if key not in self._forces:
            m, g, dg = key
            self._forces[key] = bench.oracle_eval(self.w, m, g, dg)[0]
        return self._forces[key]

    def allowance(self, key, prec):
        """[N] force of an atom's cutoff-band pairs at lambda = 1 (zero in double precision); fewer than 1 % of the atoms carry one."""
        n = len(self.w["q"])
        if prec == "double":
            return np.zeros(n)
        if key not in self._bands:
            m, g, dg = key
            fa, _, npairs = parity_tools.band_allowance(_ones(self.w), m, g, dg, parity_tools.band_rel(self.w, "single"))
            print("band pairs %d, atoms with one %d of %d" % (npairs, int((fa > 0).sum()), n))
            self._bands[key] = fa
        fa = self._bands[key]
        assert (fa > 0).sum() < 0.01 * n
        return fa


@pytest.fixture(scope="module")
def t24():
    return _Case(bench.build_workload(24000, 6.2145, 4, np.random.default_rng(bench.SEED)))


def _check_table(tab, case, key, prec, snb, label):
    """Every atom and every column against the truth; the table contracted with the workload's own lambdas against the oracle's forces."""
    w = case.w
    assert np.isfinite(tab).all()
    fa = case.allowance(key, prec)
    e_col = aft.rel(tab, case.table(key), fa)
    got = snb.HipCalcSlicedNonbondedForceKernel.forcesFromAtomForces(tab, w["subset"], w["lam"])
    want = case.forces(key)
    e_sum = float((np.maximum(np.linalg.norm(got - want, axis=1) - fa, 0.0) / np.maximum(np.linalg.norm(want, axis=1), 1.0)).max())
    print("%s %s: worst column %.3e (without allowance %.3e), contracted with the lambdas %.3e" % (label, prec, e_col, aft.rel(tab, case.table(key)), e_sum))
    assert e_col < TOLS[prec], e_col
    assert e_sum < TOLS[prec], e_sum
    return e_col


# ---- 1. the 24k box: RF, PME, LJPME x single, mixed, double ---------------------------------------------------------------------------
@pytest.mark.parametrize("prec", ["single", "mixed", "double"])
@pytest.mark.parametrize("name", ["rf", "pme", "ljpme"])
def test_24k_table_against_the_oracle(name, prec, t24, snb):
    w = t24.w; n = len(w["q"]); isd = prec == "double"
    m, g, dg = METHODS[name]
    eng = bench.Engine(snb, w, m, g, dg, prec, 0, 0, 1, 0.1, 1 << 30)
    pos = _dev(w["pos"], isd)
    eng.set_positions_device(pos.data_ptr(), isd)
    tab = _table(eng, n, 4)
    _check_table(tab, t24, METHODS[name], prec, snb, name)
    eng.close()


# ---- 2. 60 atoms, 3 subsets, every entry -----------------------------------------------------------------------------------------------
SMALL = {"NoCutoff": {}, "CutoffNonPeriodic": {}, "CutoffPeriodic": {}, "PME": dict(pme=(2.6283, 20, 20, 20)),
         "LJPME": dict(pme=(2.6283, 20, 20, 20), ljpme=(2.6283, 12, 12, 12)), "CutoffPeriodic+switch": dict(switch=True)}


def _small_force(snb, method, offsets=False):
    F = snb.SlicedNonbondedForce
    force, pos, box = systems.random_box(F, 60, 3, getattr(F, method.split("+")[0]), 2.05, 1.0, **SMALL[method])
    if offsets:
        force.addGlobalParameter("shift", 0.0)
        for i, dq in ((3, 0.5), (17, -0.3), (41, 0.4), (58, 0.25)):
            force.addParticleParameterOffset("shift", i, dq, 0.02, 0.1)
    pos = np.asarray(pos, dtype=np.float64).astype(np.float32).astype(np.float64)      # what a single-precision engine is given
    return force, pos, box


def _context(snb, force, pos, box, prec):
    system = snb.System()
    for _ in range(force.getNumParticles()):
        system.addParticle(1.0)
    system.setDefaultPeriodicBoxVectors(*box)
    system.addForce(force)
    ctx = snb.Context(system, precision=prec, device=0)
    ctx.setPositions(pos)
    return ctx


@pytest.fixture(scope="module")
def small_truths(snb, oracle):
    cache = {}

    def get(method, offsets=False, parameters=None):
        key = (method, offsets, tuple(sorted((parameters or {}).items())))
        if key not in cache:
            force, pos, box = _small_force(snb, method, offsets)
            cache[key] = aft.truth_table(aft.force_evaluator(oracle, force, pos, box, parameters), aft.force_subsets(force), 3)
        return cache[key]
    return get


@pytest.mark.parametrize("prec", ["double", "single"])
@pytest.mark.parametrize("method", list(SMALL))
def test_60_atoms_every_entry_against_its_truth(method, prec, snb, small_truths):
    force, pos, box = _small_force(snb, method)
    if "switch" in method:
        assert force.getUseSwitchingFunction()
    ctx = _context(snb, force, pos, box, prec)
    tab = ctx.getAtomForces(force)
    assert tab.shape == (60, 3, 2, 3)
    want = small_truths(method)
    assert np.abs(want[..., 0, :]).max() > 1.0 and np.abs(want[..., 1, :]).max() > 1.0
    err = aft.rel(tab, want)
    print("%s %s: worst entry %.3e" % (method, prec, err))
    assert err < TOLS[prec], err
    assert ctx._kernelFor(force).getStats().n_host_rebuilds > 0      # (the host lists: below the GPU builder's floor)


# ---- 3. triclinic ----------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def tric():
    """The 24k box with three subsets (water and two blobs: 12 one-hot evaluations), sheared."""
    return _Case(bench.shear_workload(bench.build_workload(24000, 6.2145, 3, np.random.default_rng(bench.SEED))))


@pytest.mark.parametrize("prec", ["single", "double"])
def test_triclinic_24k(prec, tric, snb):
    w = tric.w; n = len(w["q"]); isd = prec == "double"
    eng = bench.Engine(snb, w, 4, 54, 0, prec, 0, 0, 1, 0.1, 1 << 30)
    pos = _dev(w["pos"], isd)
    eng.set_positions_device(pos.data_ptr(), isd)
    tab = _table(eng, n, 3)
    _check_table(tab, tric, (4, 54, 0), prec, snb, "triclinic pme")
    eng.close()


# ---- 4. separation of the parts --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("prec", ["single", "double"])
@pytest.mark.parametrize("name", ["pme", "ljpme"])
def test_direct_and_reciprocal_parts_separate(name, prec, t24, snb):
    w = t24.w; n = len(w["q"]); isd = prec == "double"
    m, g, dg = METHODS[name]
    eng = bench.Engine(snb, w, m, g, dg, prec, 0, 0, 1, 0.1, 1 << 30)
    pos = _dev(w["pos"], isd)
    eng.set_positions_device(pos.data_ptr(), isd)
    full = _table(eng, n, 4); direct = _table(eng, n, 4, 1, 0); recip = _table(eng, n, 4, 0, 1)
    err = aft.rel(direct + recip, full)
    print("%s %s: direct + reciprocal against the full table: %.3e" % (name, prec, err))
    assert err < TOLS[prec]
    assert np.abs(recip[:, :, 0]).max() > 1.0
    if name == "pme":
        assert not recip[:, :, 1].any()      # (PME: the mesh carries no vdW term)
    else:
        assert np.abs(recip[:, :, 1]).max() > 1e-3
    # direct space is pair forces alone: what J puts on I and what I puts on J cancel, slice by slice
    scale = np.linalg.norm(direct, axis=-1).max()
    tl = np.linalg.norm(aft.third_law(direct, w["subset"], 4), axis=-1).max()
    print("third law, direct only: %.3e of the largest column norm %.3e" % (tl / scale, scale))
    assert tl < TOLS[prec] * scale
    eng.close()


# ---- 5. classic Ewald ------------------------------------------------------------------------------------------------------------------
def test_classic_ewald_direct_only(snb, oracle):
    capi = snb.capi; L = capi.lib()
    F = snb.SlicedNonbondedForce
    force, epos, box = systems.random_box(F, 1500, 3, F.Ewald, 2.6, 1.0, pme=(2.6283, 0, 0, 0))
    force.ewaldKmax = (11, 11, 11)
    ctx = _context(snb, force, epos, box, "double")
    kern = ctx._kernelFor(force)
    etab = np.zeros((1500, 3, 2, 3)); eptr = etab.ctypes.data_as(ctypes.c_void_p)
    kern._push_state(ctx)
    assert L.snb_evaluate_atom_forces(kern._h, 1, 1, eptr, 0) == capi.SNB_ERR_UNSUPPORTED
    assert L.snb_evaluate_atom_forces(kern._h, 0, 1, eptr, 0) == capi.SNB_ERR_UNSUPPORTED
    with pytest.raises(snb.OpenMMException):
        ctx.getAtomForces(force)
    etab = ctx.getAtomForces(force, includeReciprocal=False)
    esub = aft.force_subsets(force)
    want = aft.truth_table(aft.force_evaluator(oracle, force, epos, box, include_reciprocal=False, kmax=(11, 11, 11)), esub, 3)
    err = aft.rel(etab, want)
    print("classic Ewald, direct only, double: worst entry %.3e" % err)
    assert err < TOLS["double"], err


# ---- 6. contract: the call writes only the table ---------------------------------------------------------------------------------------
def _device_doubles(ptr, count):
    """A torch view of `count` doubles at a raw device address."""
    import torch

    class _Raw:
        __cuda_array_interface__ = {"shape": (count,), "typestr": "<f8", "data": (int(ptr), False), "version": 2}
    return torch.as_tensor(_Raw(), device="cuda")


def _ferr(f, fo, fa):
    return float((np.maximum(np.linalg.norm(f - fo, axis=1) - fa, 0.0) / np.maximum(np.linalg.norm(fo, axis=1), 1.0)).max())


@pytest.mark.parametrize("rebuild", [False, True])
def test_call_writes_only_the_table(rebuild, t24, snb):
    """Mixed precision.  Forces steps with energies, then the call: snb_get_forces, a registered accumulate-mode force output, the slice-
    energy buffer (host copy and device buffer) and snb_stats.n_timed are what they were, bit for bit -- also when the call itself
    performs the due rebuild (fixed interval 2: the third evaluation).  A following forces step matches the oracle."""
    import torch
    w = t24.w; n = len(w["q"]); key = METHODS["pme"]
    eng = bench.Engine(snb, w, 4, 54, 0, "mixed", 0, 0, 1, 0.1, 2 if rebuild else 1 << 30)
    pos = _dev(w["pos"], False)
    out = torch.full((n, 3), 7.25, dtype=torch.float32, device="cuda")
    eng.set_force_output(out.data_ptr(), False, 1)
    eng.set_positions_device(pos.data_ptr(), False)
    eng.execute(True); eng.execute(True)
    eng.sync()
    f_before = torch.zeros((n, 3), dtype=torch.float32, device="cuda"); eng.forces_to(f_before.data_ptr(), False); eng.sync()
    out_before = out.clone()
    se_before = eng.slice_energies(S4)
    dev = ctypes.c_void_p(); eng.ok(eng.L.snb_slice_energies_device(eng.h, ctypes.byref(dev)))
    dev_before = _device_doubles(dev.value, 2 * S4).clone()
    timed_before = eng.stats().n_timed; r0 = eng.stats().n_rebuilds
    tab = _table(eng, n, 4)
    assert eng.stats().n_rebuilds == r0 + (1 if rebuild else 0)
    assert aft.rel(tab, t24.table(key), t24.allowance(key, "mixed")) < TOLS["mixed"]
    f_after = torch.zeros_like(f_before); eng.forces_to(f_after.data_ptr(), False); eng.sync()
    assert torch.equal(f_before, f_after)
    assert torch.equal(out, out_before)
    assert np.array_equal(eng.slice_energies(S4), se_before)
    dev2 = ctypes.c_void_p(); eng.ok(eng.L.snb_slice_energies_device(eng.h, ctypes.byref(dev2)))
    assert dev2.value == dev.value and torch.equal(_device_doubles(dev.value, 2 * S4), dev_before)
    assert eng.stats().n_timed == timed_before
    eng.execute(False)
    eng.forces_to(f_after.data_ptr(), False); eng.sync()
    err = _ferr(f_after.double().cpu().numpy(), t24.forces(key), t24.allowance(key, "mixed"))
    print("forces step after the call (rebuild inside it: %s): %.3e" % (rebuild, err))
    assert err < TOLS["mixed"]
    eng.close()


def test_bound_context_buffers_stay(t24, snb):
    """posq in a random context order: after a bound forces step with energies and derivatives, the call leaves posq and the binding's
    force, energy and derivative buffers bit for bit what they were, and its table (USER order) matches the oracle."""
    import torch
    from test_gpu_context_binding import View
    w = t24.w; n = len(w["q"]); key = METHODS["pme"]
    v = View(w["pos"], False, seed=23, n_derivs=2 * S4)
    eng = bench.Engine(snb, w, 4, 54, 0, "single", 0, 0, 1, 0.1, 1 << 30)
    slots = np.arange(2 * S4, dtype=np.int32).reshape(S4, 2)
    b = v.binding(snb.capi, deriv_slot=slots)
    torch.cuda.synchronize()
    eng.ok(eng.L.snb_bind_context(eng.h, ctypes.byref(b)))
    eng.ok(eng.L.snb_execute(eng.h, 1, 1, 1, 1, None))
    torch.cuda.synchronize()
    assert not torch.equal(v.buf, v.P) and not torch.equal(v.ebuf, v.E0) and not torch.equal(v.dbuf, v.D0)      # (the step delivered)
    posq0, buf0, ebuf0, dbuf0 = v.posq.clone(), v.buf.clone(), v.ebuf.clone(), v.dbuf.clone()
    got = _table(eng, n, 4)
    torch.cuda.synchronize()
    assert torch.equal(v.posq, posq0) and torch.equal(v.buf, buf0) and torch.equal(v.ebuf, ebuf0) and torch.equal(v.dbuf, dbuf0)
    err = aft.rel(got, t24.table(key), t24.allowance(key, "single"))
    print("bound engine against the oracle: %.3e" % err)
    assert err < TOLS["single"]
    eng.close()


# ---- 7. lists in use -------------------------------------------------------------------------------------------------------------------
def test_call_in_the_middle_of_a_lists_life(snb):
    """Padding 0.1, a fixed rebuild interval of 8, positions nudged on the device before every step: after four steps the call uses the
    list as it is (no rebuild) and its table matches the oracle at the current positions.  Two subsets: 6 one-hot evaluations."""
    import torch
    w = bench.build_workload(24000, 6.2145, 2, np.random.default_rng(bench.SEED)); n = len(w["q"])
    eng = bench.Engine(snb, w, 4, 54, 0, "double", 0, 0, 1, 0.1, 8)
    g = torch.Generator(device="cuda").manual_seed(29)
    pos = _dev(w["pos"], True)
    eng.set_positions_device(pos.data_ptr(), True)
    for _ in range(4):
        eng.execute(False)
        pos += 0.004 * torch.randn(pos.shape, generator=g, device="cuda", dtype=torch.float64)
        eng.set_positions_device(pos.data_ptr(), True)
    eng.sync()
    r0 = eng.stats().n_rebuilds
    tab = _table(eng, n, 2)
    assert eng.stats().n_rebuilds == r0
    v = dict(w); v["pos"] = np.ascontiguousarray(pos.cpu().numpy())
    assert np.abs(v["pos"] - w["pos"]).max() > 0.01
    want = aft.truth_table(aft.workload_evaluator(v, 4, 54, 0), w["subset"], 2)
    err = aft.rel(tab, want)
    print("mid-life list, double: worst column %.3e" % err)
    assert err < TOLS["double"], err
    eng.close()


# ---- 8. parameter offsets --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("prec", ["double", "single"])
def test_table_follows_the_global_parameters(prec, snb, small_truths):
    force, pos, box = _small_force(snb, "PME", offsets=True)
    ctx = _context(snb, force, pos, box, prec)
    at0 = ctx.getAtomForces(force)
    assert aft.rel(at0, small_truths("PME", True, {"shift": 0.0})) < TOLS[prec]
    ctx.setParameter("shift", 0.7)
    at1 = ctx.getAtomForces(force)
    want = small_truths("PME", True, {"shift": 0.7})
    assert aft.rel(want, small_truths("PME", True, {"shift": 0.0})) > 0.1      # (the offsets matter)
    err = aft.rel(at1, want)
    print("offsets %s: worst entry %.3e" % (prec, err))
    assert err < TOLS[prec], err


# ---- 9. device output ------------------------------------------------------------------------------------------------------------------
def test_device_output_equals_host_output(t24, snb):
    """Two calls from the same state on a quiescent engine, one to the host, one to the device.  The table's double atomics arrive in
    another order on every run, so the two agree to the rounding of the sums, not bit for bit.  The bound: an entry
    is the double sum of at most T ~ 1e3 flushed partial sums (runs of tiles on the i-side, tiles on the j-side), themselves identical
    in both calls (a wave's own arithmetic is ordered); re-ordering a double sum moves it by at most T eps sum|terms| with eps = 1.1e-16,
    and sum|terms| of a column stays below 1e4 times max(||entry||, 1) on this box (the largest column norm is 3.7e3 kJ/mol/nm): 1e-9.
    A wrong permutation or a stale staging table is off by whole entries."""
    import torch
    w = t24.w; n = len(w["q"])
    eng = bench.Engine(snb, w, 4, 54, 0, "mixed", 0, 0, 1, 0.1, 1 << 30)
    pos = _dev(w["pos"], False)
    eng.set_positions_device(pos.data_ptr(), False)
    host = _table(eng, n, 4)
    dev = torch.full((n, 4, 2, 3), float("nan"), dtype=torch.float64, device="cuda")
    eng.ok(eng.L.snb_evaluate_atom_forces(eng.h, 1, 1, ctypes.c_void_p(dev.data_ptr()), 1))
    eng.sync()
    got = dev.cpu().numpy()
    assert np.isfinite(got).all()
    err = aft.rel(got, host)
    print("device against host output: %.3e (bit for bit: %s)" % (err, np.array_equal(got, host)))
    assert err < 1e-9
    eng.close()


def test_table_ignores_the_selection_of_an_earlier_step(t24, snb):
    """The table takes every slice whatever the last snb_execute selected: a derivative-only forces step with slice 0 alone selected
    (snb_set_energy_slices, include_energy == 2) between two tables of one state changes neither the table (the bound of two tables of one
    state, above) nor, bit for bit, what snb_get_forces returned right after the step."""
    import torch
    w = t24.w; n = len(w["q"])
    eng = bench.Engine(snb, w, 4, 54, 0, "mixed", 0, 0, 1, 0.1, 1 << 30)
    pos = _dev(w["pos"], False)
    eng.set_positions_device(pos.data_ptr(), False)
    before = _table(eng, n, 4)
    eng.set_energy_slices([1] + [0] * (S4 - 1))
    eng.ok(eng.L.snb_execute(eng.h, 1, 2, 1, 1, None))
    f_step = torch.zeros((n, 3), dtype=torch.float32, device="cuda"); eng.forces_to(f_step.data_ptr(), False); eng.sync()
    after = _table(eng, n, 4)
    assert np.isfinite(after).all() and np.abs(after).max() > 1.0
    err = aft.rel(after, before)
    print("table after a selective step against the table before: %.3e" % err)
    assert err < 1e-9
    f_after = torch.zeros_like(f_step); eng.forces_to(f_after.data_ptr(), False); eng.sync()
    assert torch.equal(f_step, f_after)
    eng.close()


# ---- 10. refusals ----------------------------------------------------------------------------------------------------------------------
def test_refusals(t24, snb):
    capi = snb.capi; L = capi.lib()
    w = t24.w; n = len(w["q"])
    out = np.zeros((n, 4, 2, 3)); optr = out.ctypes.data_as(ctypes.c_void_p)
    eng = bench.Engine(snb, w, 2, 54, 0, "single", 0, 0, 1, 0.1, 1 << 30)
    pos = _dev(w["pos"], False)
    eng.set_positions_device(pos.data_ptr(), False)
    assert L.snb_evaluate_atom_forces(eng.h, 1, 1, None, 0) == capi.SNB_ERR_INVALID_ARGUMENT
    assert L.snb_evaluate_atom_forces(eng.h, 0, 0, optr, 0) == capi.SNB_ERR_INVALID_ARGUMENT
    assert eng.stats().n_rebuilds == 0 and not out.any()      # (refused before anything was enqueued: no list was built, nothing written)
    assert L.snb_evaluate_atom_forces(eng.h, 1, 1, optr, 0) == capi.SNB_OK
    assert eng.stats().n_rebuilds == 1 and out.any()
    eng.close()
    sharded = bench.Engine(snb, w, 4, 54, 0, "single", 0, 0, 2, 0.1, 1 << 30)
    sharded.set_positions_device(pos.data_ptr(), False)
    assert L.snb_evaluate_atom_forces(sharded.h, 1, 1, optr, 0) == capi.SNB_ERR_UNSUPPORTED
    assert sharded.stats().n_rebuilds == 0
    sharded.close()
    # particles, box or positions missing: what snb_execute returns in that state
    cfg = capi.SnbConfig()
    cfg.abi_version = capi.SNB_ABI_VERSION; cfg.n_atoms = 96; cfg.n_subsets = 2; cfg.method = 2; cfg.cutoff = 1.0; cfg.rf_dielectric = 78.3
    cfg.shard_count = 1
    h = ctypes.c_void_p()
    assert L.snb_create(ctypes.byref(cfg), ctypes.byref(h)) == capi.SNB_OK
    small = np.zeros((96, 2, 2, 3)); sptr = small.ctypes.data_as(ctypes.c_void_p)
    dp = lambda a: a.ctypes.data_as(ctypes.POINTER(ctypes.c_double))

    def same_refusal():
        st = L.snb_evaluate_atom_forces(h, 1, 1, sptr, 0)
        assert st != capi.SNB_OK and st == L.snb_execute(h, 0, 1, 1, 1, None)
        assert not small.any()
    same_refusal()                                                                        # nothing set
    q = np.zeros(96); sg = np.full(96, 0.3); ep = np.full(96, 0.5); sub = (np.arange(96) % 2).astype(np.int32)
    assert L.snb_set_particles(h, dp(q), dp(sg), dp(ep), sub.ctypes.data_as(ctypes.POINTER(ctypes.c_int32))) == capi.SNB_OK
    same_refusal()                                                                        # no positions
    xyz = np.ascontiguousarray(systems.jittered_lattice(96, 3.0, np.random.default_rng(1)))
    assert L.snb_set_positions(h, xyz.ctypes.data_as(ctypes.c_void_p), 0, 1, 0) == capi.SNB_OK
    same_refusal()                                                                        # no box
    assert L.snb_set_box(h, dp(np.ascontiguousarray(np.diag([3.0, 3.0, 3.0]).reshape(9)))) == capi.SNB_OK
    assert L.snb_evaluate_atom_forces(h, 1, 1, sptr, 0) == capi.SNB_OK
    assert small[:, :, 1].any() and not small[:, :, 0].any()      # (q = 0: Lennard-Jones forces alone)
    L.snb_destroy(h)
