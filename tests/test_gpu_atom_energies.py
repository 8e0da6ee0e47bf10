"""Per-atom interaction energies with every subset (-m gpu): snb_evaluate_atom_energies (include/snb.h).

Ground truth is the oracle alone (tests/atom_energy_truth.py): atom a moved into a subset of its own, the oracle's raw slice energies of that
system, the singled-out rule.  Truths do not depend on the precision mode: they are computed once per (workload, method) and shared.
Tolerances are the project's (tests/test_gpu_energy_only.py TOLS) under the reference's scale rule |got - want| / max(|want|, 1), per table
entry and per reduced slice.  The 24k-atom box takes the GPU list builder, the brick spreader and the plane path; 60 atoms is below the
builder's 64-atom floor and takes the host lists and the per-pair-wrap kernels."""
import ctypes

import numpy as np
import pytest

import atom_energy_truth as aet
import bench
import systems

pytestmark = pytest.mark.gpu

TOLS = {"single": 1e-3, "double": 1e-5, "mixed": 1e-3}
S4 = 10
METHODS = {"rf": (2, 54, 0), "pme": (4, 54, 0), "ljpme": (5, 54, 27)}


def _w24k():
    return bench.build_workload(24000, 6.2145, 4, np.random.default_rng(bench.SEED))


def _dev(a, isd):
    import torch
    return torch.tensor(np.asarray(a), dtype=torch.float64 if isd else torch.float32, device="cuda")


def _table(eng, n, nsub, direct=1, recip=1):
    out = np.full((n, nsub, 2), np.nan)
    eng.ok(eng.L.snb_evaluate_atom_energies(eng.h, direct, recip, out.ctypes.data_as(ctypes.c_void_p), 0))
    return out


def _probes(w):
    """Ten atoms: the first and last atom of each of the four subsets (the 40-atom subset included), a blob atom with 1-2, 1-3 and 1-4
    partners on both sides, a water hydrogen (epsilon = 0, excluded partners)."""
    sub = w["subset"]
    p = []
    for s in range(4):
        idx = np.flatnonzero(sub == s)
        p += [int(idx[0]), int(idx[-1])]
    blob = np.flatnonzero(sub == 1)
    p.append(int(blob[len(blob) // 2]))
    water = np.flatnonzero(sub == 0)
    p.append(int(water[1]))
    assert len(set(p)) == 10 and w["epsilon"][p[-1]] == 0.0 and w["epsilon"][int(water[0])] > 0.0
    assert sub[p[8] - 3] == 1 and sub[p[8] + 3] == 1
    return p


class _Truths:
    """Oracle results of the 24k box per method, computed on first use and kept for the module."""

    def __init__(self):
        self.w = _w24k()
        self.probes = _probes(self.w)
        self._slices, self._rows = {}, {}

    def slices(self, name, direct=1, recip=1):
        key = (name, direct, recip)
        if key not in self._slices:
            m, g, dg = METHODS[name]
            self._slices[key] = bench.oracle_eval(self.w, m, g, dg, direct, recip)[1]
        return self._slices[key]

    def rows(self, name):
        if name not in self._rows:
            m, g, dg = METHODS[name]
            self._rows[name] = aet.truth_table(aet.workload_evaluator(self.w, m, g, dg), self.w["subset"], 4, self.probes)
        return self._rows[name]


@pytest.fixture(scope="module")
def t24():
    return _Truths()


def _check_sum_rule(table, subset, nsub, want, tol, snb):
    lo, hi = aet.reduce_by_sum_rule(table, subset, nsub)
    errs = (aet.rel(lo, want), aet.rel(hi, want), aet.rel(snb.HipCalcSlicedNonbondedForceKernel.sliceEnergiesFromAtomEnergies(table, subset), want))
    print("sum rule: worst %.3e (rows of I %.3e, rows of J %.3e)" % (max(errs), errs[0], errs[1]))
    assert max(errs) < tol, errs
    return max(errs)


def _check_rows(table, rows, tol):
    worst = max(aet.rel(table[a], row) for a, row in rows.items())
    print("probe rows: worst %.3e over %d atoms" % (worst, len(rows)))
    for a, row in rows.items():
        assert aet.rel(table[a], row) < tol, (a, table[a], row)
    return worst


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
    assert np.isfinite(tab).all()
    print("%s %s:" % (name, prec))
    _check_sum_rule(tab, w["subset"], 4, t24.slices(name), TOLS[prec], snb)
    _check_rows(tab, t24.rows(name), TOLS[prec])
    eng.close()


# ---- 2. 60 atoms, 3 subsets, every atom ------------------------------------------------------------------------------------------------
SMALL = {"NoCutoff": {}, "CutoffNonPeriodic": {}, "CutoffPeriodic": {}, "PME": dict(pme=(2.6283, 20, 20, 20)),
         "LJPME": dict(pme=(2.6283, 20, 20, 20), ljpme=(2.6283, 12, 12, 12))}


def _small_force(snb, method, offsets=False):
    F = snb.SlicedNonbondedForce
    force, pos, box = systems.random_box(F, 60, 3, getattr(F, method), 2.05, 1.0, **SMALL[method])
    if offsets:
        force.addGlobalParameter("shift", 0.0)
        for i, dq in ((3, 0.5), (17, -0.3), (41, 0.4), (58, 0.25)):
            force.addParticleParameterOffset("shift", i, dq, 0.02, 0.1)
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
            cache[key] = aet.truth_table(aet.force_evaluator(oracle, force, pos, box, parameters), aet.force_subsets(force), 3)
        return cache[key]
    return get


@pytest.mark.parametrize("prec", ["double", "single"])
@pytest.mark.parametrize("method", list(SMALL))
def test_60_atoms_every_atom_against_its_truth(method, prec, snb, small_truths):
    force, pos, box = _small_force(snb, method)
    ctx = _context(snb, force, pos, box, prec)
    tab = ctx.getAtomEnergies(force)
    assert tab.shape == (60, 3, 2)
    err = aet.rel(tab, small_truths(method))
    print("%s %s: worst entry %.3e" % (method, prec, err))
    assert err < TOLS[prec], err
    assert ctx._kernelFor(force).getStats().n_host_rebuilds > 0      # (the host lists: below the GPU builder's floor)


# ---- 3. triclinic ----------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def tric(t24):
    w = bench.shear_workload(t24.w)
    probes = [t24.probes[2], t24.probes[7], t24.probes[9]]      # first blob atom, last atom of the 40-atom subset, the water hydrogen
    return dict(w=w, slices=bench.oracle_eval(w, 4, 54, 0)[1], rows=aet.truth_table(aet.workload_evaluator(w, 4, 54, 0), w["subset"], 4, probes))


@pytest.mark.parametrize("prec", ["single", "double"])
def test_triclinic_24k(prec, tric, snb):
    w = tric["w"]; n = len(w["q"]); isd = prec == "double"
    eng = bench.Engine(snb, w, 4, 54, 0, prec, 0, 0, 1, 0.1, 1 << 30)
    pos = _dev(w["pos"], isd)
    eng.set_positions_device(pos.data_ptr(), isd)
    tab = _table(eng, n, 4)
    _check_sum_rule(tab, w["subset"], 4, tric["slices"], TOLS[prec], snb)
    _check_rows(tab, tric["rows"], TOLS[prec])
    eng.close()


# ---- 4. separation ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("prec", ["single", "double"])
def test_direct_and_reciprocal_parts_separate(prec, t24, snb):
    w = t24.w; n = len(w["q"]); isd = prec == "double"
    eng = bench.Engine(snb, w, 4, 54, 0, prec, 0, 0, 1, 0.1, 1 << 30)
    pos = _dev(w["pos"], isd)
    eng.set_positions_device(pos.data_ptr(), isd)
    full = _table(eng, n, 4); direct = _table(eng, n, 4, 1, 0); recip = _table(eng, n, 4, 0, 1)
    err = aet.rel(direct + recip, full)
    print("direct + reciprocal against the full table: %.3e" % err)
    assert err < TOLS[prec]
    assert not recip[..., 1].any()      # (PME: the mesh carries no vdW term)
    _check_sum_rule(direct, w["subset"], 4, t24.slices("pme", 1, 0), TOLS[prec], snb)
    _check_sum_rule(recip, w["subset"], 4, t24.slices("pme", 0, 1), TOLS[prec], snb)
    eng.close()


# ---- 5. contract: the call writes only the table ---------------------------------------------------------------------------------------
def _device_doubles(ptr, count):
    """A torch view of `count` doubles at a raw device address."""
    import torch

    class _Raw:
        __cuda_array_interface__ = {"shape": (count,), "typestr": "<f8", "data": (int(ptr), False), "version": 2}
    return torch.as_tensor(_Raw(), device="cuda")


def test_call_leaves_forces_outputs_energies_and_timers_alone(t24, snb):
    """Mixed precision (bitwise reproducible forces).  A forces step, an energy step, the call: afterwards snb_get_forces, a registered
    accumulate-mode force output, the slice-energy buffer (host copy and device buffer) and snb_stats.n_timed are what they were, bit for
    bit; two replayed forces steps after the call equal those of a twin engine that never made it."""
    import torch
    w = t24.w; n = len(w["q"])
    g = torch.Generator(device="cuda").manual_seed(17)
    p1 = _dev(w["pos"], False)
    p2 = p1 + 0.004 * torch.randn(p1.shape, generator=g, device="cuda")
    p3 = p2 + 0.004 * torch.randn(p1.shape, generator=g, device="cuda")
    A = bench.Engine(snb, w, 4, 54, 0, "mixed", 0, 0, 1, 0.3, 1 << 30)
    B = bench.Engine(snb, w, 4, 54, 0, "mixed", 0, 0, 1, 0.3, 1 << 30)
    outs = []
    for e in (A, B):
        out = torch.full((n, 3), 7.25, dtype=torch.float32, device="cuda")
        e.set_force_output(out.data_ptr(), False, 1)
        outs.append(out)
        e.set_positions_device(p1.data_ptr(), False); e.execute(False)                                  # forces step
        e.set_positions_device(p2.data_ptr(), False); e.ok(e.L.snb_execute(e.h, 0, 1, 1, 1, None))      # energy step
        e.sync()
    f_before = torch.zeros((n, 3), dtype=torch.float32, device="cuda"); A.forces_to(f_before.data_ptr(), False); A.sync()
    out_before = outs[0].clone()
    se_before = A.slice_energies(S4)
    dev = ctypes.c_void_p(); A.ok(A.L.snb_slice_energies_device(A.h, ctypes.byref(dev)))
    dev_before = _device_doubles(dev.value, 2 * S4).clone()
    timed_before = A.stats().n_timed
    tab = _table(A, n, 4)
    assert np.isfinite(tab).all() and np.abs(tab).max() > 1.0
    f_after = torch.zeros_like(f_before); A.forces_to(f_after.data_ptr(), False); A.sync()
    assert torch.equal(f_before, f_after)
    assert torch.equal(outs[0], out_before)
    assert np.array_equal(A.slice_energies(S4), se_before)
    assert torch.equal(_device_doubles(dev.value, 2 * S4), dev_before)
    assert A.stats().n_timed == timed_before
    fa = torch.zeros_like(f_before); fb = torch.zeros_like(f_before)
    for p in (p3, p1):
        for e, f in ((A, fa), (B, fb)):
            e.set_positions_device(p.data_ptr(), False); e.execute(False); e.forces_to(f.data_ptr(), False); e.sync()
        assert torch.equal(fa, fb)
        assert torch.equal(outs[0], outs[1])
    A.close(); B.close()


# ---- 6. a rebuild inside the call ------------------------------------------------------------------------------------------------------
def test_rebuild_inside_the_call(t24, snb):
    """A fixed rebuild interval of 2: the third evaluation since the last rebuild is due one.  Before it the solute atoms move far past the
    skin (the list in memory would miss pairs): the call rebuilds by itself and the sum rule holds against the oracle at the new positions."""
    w = t24.w; n = len(w["q"])
    eng = bench.Engine(snb, w, 4, 54, 0, "double", 0, 0, 1, 0.1, 2)
    pos = _dev(w["pos"], True)
    eng.set_positions_device(pos.data_ptr(), True)
    _table(eng, n, 4); _table(eng, n, 4)
    rng = np.random.default_rng(5)
    moved = w["pos"] + rng.uniform(-0.12, 0.12, w["pos"].shape) * (w["subset"] != 0)[:, None]      # up to 0.2 nm against a skin of 0.1
    pos2 = _dev(moved, True)
    eng.set_positions_device(pos2.data_ptr(), True)
    r0 = eng.stats().n_rebuilds
    tab = _table(eng, n, 4)
    assert eng.stats().n_rebuilds == r0 + 1
    v = dict(w); v["pos"] = np.ascontiguousarray(moved)
    _check_sum_rule(tab, w["subset"], 4, bench.oracle_eval(v, 4, 54, 0)[1], TOLS["double"], snb)
    eng.close()


# ---- 7. parameter offsets --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("prec", ["double", "single"])
def test_table_follows_the_global_parameters(prec, snb, small_truths):
    force, pos, box = _small_force(snb, "PME", offsets=True)
    ctx = _context(snb, force, pos, box, prec)
    at0 = ctx.getAtomEnergies(force)
    assert aet.rel(at0, small_truths("PME", True, {"shift": 0.0})) < TOLS[prec]
    ctx.setParameter("shift", 0.7)
    at1 = ctx.getAtomEnergies(force)
    want = small_truths("PME", True, {"shift": 0.7})
    assert aet.rel(want, small_truths("PME", True, {"shift": 0.0})) > 0.1      # (the offsets matter)
    err = aet.rel(at1, want)
    print("offsets %s: worst entry %.3e" % (prec, err))
    assert err < TOLS[prec], err


# ---- 8. bound context ------------------------------------------------------------------------------------------------------------------
def test_bound_context_gives_the_unbound_table(t24, snb):
    """posq in a random context order: the table, in USER order, equals the unbound engine's; posq, the force, energy and derivative
    buffers of the binding are untouched."""
    import torch
    from test_gpu_context_binding import View
    w = t24.w; n = len(w["q"])
    ref = bench.Engine(snb, w, 4, 54, 0, "single", 0, 0, 1, 0.1, 1 << 30)
    pos = _dev(w["pos"], False)
    ref.set_positions_device(pos.data_ptr(), False)
    want = _table(ref, n, 4)
    ref.close()
    v = View(w["pos"], False, seed=23, n_derivs=2 * S4)
    eng = bench.Engine(snb, w, 4, 54, 0, "single", 0, 0, 1, 0.1, 1 << 30)
    slots = np.arange(2 * S4, dtype=np.int32).reshape(S4, 2)
    b = v.binding(snb.capi, deriv_slot=slots)
    torch.cuda.synchronize()
    eng.ok(eng.L.snb_bind_context(eng.h, ctypes.byref(b)))
    posq0 = v.posq.clone()
    got = _table(eng, n, 4)
    torch.cuda.synchronize()
    err = aet.rel(got, want)
    print("bound against unbound: %.3e" % err)
    assert err < TOLS["single"]
    assert torch.equal(v.posq, posq0) and torch.equal(v.buf, v.P) and torch.equal(v.ebuf, v.E0) and torch.equal(v.dbuf, v.D0)
    _check_rows(got, t24.rows("pme"), TOLS["single"])
    eng.close()


# ---- 9. device output ------------------------------------------------------------------------------------------------------------------
def test_device_output_equals_host_output(t24, snb):
    import torch
    w = t24.w; n = len(w["q"])
    eng = bench.Engine(snb, w, 4, 54, 0, "mixed", 0, 0, 1, 0.1, 1 << 30)
    pos = _dev(w["pos"], False)
    eng.set_positions_device(pos.data_ptr(), False)
    host = _table(eng, n, 4)
    dev = torch.full((n, 4, 2), float("nan"), dtype=torch.float64, device="cuda")
    eng.ok(eng.L.snb_evaluate_atom_energies(eng.h, 1, 1, ctypes.c_void_p(dev.data_ptr()), 1))
    eng.sync()
    got = dev.cpu().numpy()
    assert np.isfinite(got).all()
    # (the table's double atomics arrive in another order on every run: equal to rounding of the sums, not bit for bit)
    assert aet.rel(got, host) < 1e-9
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
    err = aet.rel(after, before)
    print("table after a selective step against the table before: %.3e" % err)
    assert err < 1e-9
    f_after = torch.zeros_like(f_step); eng.forces_to(f_after.data_ptr(), False); eng.sync()
    assert torch.equal(f_step, f_after)
    eng.close()


# ---- 10. status codes ------------------------------------------------------------------------------------------------------------------
def test_status_codes(t24, snb, oracle):
    capi = snb.capi; L = capi.lib()
    w = t24.w; n = len(w["q"])
    out = np.zeros((n, 4, 2)); optr = out.ctypes.data_as(ctypes.c_void_p)
    eng = bench.Engine(snb, w, 2, 54, 0, "single", 0, 0, 1, 0.1, 1 << 30)
    pos = _dev(w["pos"], False)
    eng.set_positions_device(pos.data_ptr(), False)
    assert L.snb_evaluate_atom_energies(eng.h, 1, 1, None, 0) == capi.SNB_ERR_INVALID_ARGUMENT
    assert L.snb_evaluate_atom_energies(eng.h, 0, 0, optr, 0) == capi.SNB_ERR_INVALID_ARGUMENT
    assert eng.stats().n_rebuilds == 0      # (refused before anything was enqueued)
    assert L.snb_evaluate_atom_energies(eng.h, 1, 1, optr, 0) == capi.SNB_OK
    eng.close()
    sharded = bench.Engine(snb, w, 4, 54, 0, "single", 0, 0, 2, 0.1, 1 << 30)
    sharded.set_positions_device(pos.data_ptr(), False)
    assert L.snb_evaluate_atom_energies(sharded.h, 1, 1, optr, 0) == capi.SNB_ERR_UNSUPPORTED
    sharded.close()
    # classic Ewald: the reciprocal sum is refused, direct-only works (and reduces to the oracle's direct-space slice energies)
    F = snb.SlicedNonbondedForce
    force, epos, box = systems.random_box(F, 1500, 3, F.Ewald, 2.6, 1.0, pme=(2.6283, 0, 0, 0))
    force.ewaldKmax = (11, 11, 11)
    ctx = _context(snb, force, epos, box, "double")
    kern = ctx._kernelFor(force)
    etab = np.zeros((1500, 3, 2)); eptr = etab.ctypes.data_as(ctypes.c_void_p)
    kern._push_state(ctx)
    assert L.snb_evaluate_atom_energies(kern._h, 1, 1, eptr, 0) == capi.SNB_ERR_UNSUPPORTED
    assert L.snb_evaluate_atom_energies(kern._h, 0, 1, eptr, 0) == capi.SNB_ERR_UNSUPPORTED
    with pytest.raises(snb.OpenMMException):
        ctx.getAtomEnergies(force)
    etab = ctx.getAtomEnergies(force, includeReciprocal=False)
    # (raw slice energies without the dispersion correction, which the force asks for by default and the table does not attribute)
    esub = aet.force_subsets(force)
    want = aet.force_evaluator(oracle, force, epos, box, include_reciprocal=False, kmax=(11, 11, 11))(esub, 3)
    _check_sum_rule(etab, esub, 3, want, TOLS["double"], snb)
    # particles, box or positions missing: what snb_execute returns in that state
    cfg = capi.SnbConfig()
    cfg.abi_version = capi.SNB_ABI_VERSION; cfg.n_atoms = 96; cfg.n_subsets = 2; cfg.method = 2; cfg.cutoff = 1.0; cfg.rf_dielectric = 78.3
    cfg.shard_count = 1
    h = ctypes.c_void_p()
    assert L.snb_create(ctypes.byref(cfg), ctypes.byref(h)) == capi.SNB_OK
    small = np.zeros((96, 2, 2)); sptr = small.ctypes.data_as(ctypes.c_void_p)
    dp = lambda a: a.ctypes.data_as(ctypes.POINTER(ctypes.c_double))

    def same_refusal():
        st = L.snb_evaluate_atom_energies(h, 1, 1, sptr, 0)
        assert st != capi.SNB_OK and st == L.snb_execute(h, 0, 1, 1, 1, None)
    same_refusal()                                                                        # nothing set
    q = np.zeros(96); sg = np.full(96, 0.3); ep = np.full(96, 0.5); sub = (np.arange(96) % 2).astype(np.int32)
    assert L.snb_set_particles(h, dp(q), dp(sg), dp(ep), sub.ctypes.data_as(ctypes.POINTER(ctypes.c_int32))) == capi.SNB_OK
    same_refusal()                                                                        # no positions
    xyz = np.ascontiguousarray(systems.jittered_lattice(96, 3.0, np.random.default_rng(1)))
    assert L.snb_set_positions(h, xyz.ctypes.data_as(ctypes.c_void_p), 0, 1, 0) == capi.SNB_OK
    same_refusal()                                                                        # no box
    assert L.snb_set_box(h, dp(np.ascontiguousarray(np.diag([3.0, 3.0, 3.0]).reshape(9)))) == capi.SNB_OK
    assert L.snb_evaluate_atom_energies(h, 1, 1, sptr, 0) == capi.SNB_OK
    L.snb_destroy(h)
