"""Van der Waals census on the GPU: Lennard-Jones alone -- the switching function, the far range, LJPME's direct dispersion term --
against the oracle and against the closed form (tests/vdw_census.py; tests/test_vdw_census.py proves the instrument on the CPU).

Every other oracle comparison judges LJ inside a charged, dense lattice whose forces are thousands of kJ/mol/nm: a forces-only step with
no switching function at all passes them.  Here the systems are uncharged (the Coulomb columns of every output must be zero), the floor of
the per-atom comparison is the oracle's median force, and each row is asserted to have run the kernels it is there for (n_host_rebuilds,
ewald_poly_mask; skipped, they alone, when an SNB_* switch that reroutes the pair kernel is set).

 (a) bulk against the oracle, direct space alone, single / mixed / double, switching distances 0.6 and 0.9 of the cutoff: forces-only steps
     (eager, captured, replayed twice, on positions that drift on an unchanged list), energy + forces, energy only, derivative only, and on
     the RF and PME-R0 rows at sd = 0.9 the vdW columns of the three tables.  lj_big runs the GPU builder, i.e. k_directPacked<MC, POLY, E,
     SWITCH = true, FIXED> and k_directPackedEnergy<MC, POLY, true> in single and mixed precision and k_direct<double, MC, false, ..> in
     double; lj_small runs host lists with per-pair wrapping, i.e. k_direct<Real, MC, true, ..> and k_directEnergy<Real, MC, true>
 (b) radial dimers against the closed form E = 4 eps (x^12 - x^6) S(tt) (LJPME: against the oracle), both builders
 (c) the energy + forces step of single precision on the scalar tile kernel, k_direct<float, MC, false, true, ..>, in a child process under
     SNB_SCALAR_ENERGY_KERNEL
 (d) one planted defect on hardware: an engine created with a switching distance of 0.909 against an oracle at 0.9 must fail
"""
import json
import os
import subprocess
import sys

import pytest

import vdw_census as V

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PRECISIONS = ("single", "mixed", "double")
BULK = [(n, r) for n in ("lj_big", "lj_small") for r in V.PERIODIC_ROWS] + [("nonperiodic", "NonPeriodic"), ("nocutoff_cloud", "NoCutoff")]
GPU_BUILT = ("lj_big", "nonperiodic")
DIMERS = [(r, s, h) for r in ("RF", "PME-R0", "PME-R2") for s in V.SWITCH_FRACTIONS for h in (0, 1)] + [(r, 0.9, h) for r in ("LJPME-R0", "LJPME-R4") for h in (0, 1)]


def _identity(rec, row, prec, gpu_built):
    """The kernels named for the row are the ones that ran: the list builder and the guard's decisions."""
    if V.rerouted():
        return
    assert (rec["host_rebuilds"] == 0) == gpu_built, (rec["host_rebuilds"], "the GPU builder" if gpu_built else "the host lists")
    if V.ROWS[row][1] is not None:
        assert rec["mask"] == V.expected_mask(row, prec), (rec["mask"], "the guard's decisions are not the ones the CPU test derives")


def _check(rec, what, prec, tol):
    """Prints every figure, then asserts: a failure names the case (system, row, switching distance, precision), the step and the atom."""
    for step, err, detail in rec["checks"]:
        print("VDW %s | %s | %s | %.3e | %s" % (what, prec, step, err, detail))
    print("VDW %s | %s | mask %d, host rebuilds %d, Coulomb columns up to %.1e%s" % (what, prec, rec["mask"], rec["host_rebuilds"], rec["coulomb"],
                                                                                    "" if rec.get("floor") is None else ", F_med %.3f" % rec["floor"]))
    assert rec["finite"], "%s %s: a NaN or an infinity in the engine's output" % (what, prec)
    assert rec["coulomb"] <= tol, "%s %s: the system is uncharged, a Coulomb column holds %.3e" % (what, prec, rec["coulomb"])
    for step, err, detail in rec["checks"]:
        assert err <= tol, "%s %s, step %s: %.3e over %.0e (%s)" % (what, prec, step, err, tol, detail)


@pytest.mark.parametrize("prec", PRECISIONS)
@pytest.mark.parametrize("sdf", V.SWITCH_FRACTIONS)
@pytest.mark.parametrize("name,row", BULK, ids=["%s-%s" % b for b in BULK])
def test_bulk_against_the_oracle(name, row, sdf, prec, snb, oracle):
    rec = V.bulk_case(snb, name, row, sdf, prec, tables=(row in V.TABLE_ROWS and sdf == 0.9))
    _check(rec, "%s %s sd %.1f" % (name, row, sdf), prec, V.BARS[prec])
    _identity(rec, row, prec, name in GPU_BUILT)
    if row != "NoCutoff" and not V.rerouted():      # (NoCutoff has no list radius: it rebuilds on every step)
        assert rec["drift_rebuilds"] == 1 and rec["overruns"] == 0, ("the drifted steps must run on the list of the first", rec["drift_rebuilds"], rec["overruns"])


@pytest.mark.parametrize("prec", PRECISIONS)
@pytest.mark.parametrize("row,sdf,host", DIMERS, ids=["%s-%.1f-%s" % (r, s, "host" if h else "gpu") for r, s, h in DIMERS])
def test_dimers_against_the_closed_form(row, sdf, host, prec, snb, oracle):
    rec = V.dimer_case(snb, row, sdf, prec, host)
    what = "dimers %s sd %.1f %s builder" % (row, sdf, "host" if host else "GPU")
    assert rec["zero"], "%s %s: a pair beyond the cutoff, or an epsilon = 0 atom, has a force" % (what, prec)
    _check(rec, what, prec, 1.0)      # (dimer_case reports in units of each dimer's bar, the Coulomb columns aside)
    assert rec["coulomb"] <= V.BARS[prec]
    _identity(rec, row, prec, not host)


def test_scalar_energy_kernel_in_single_precision(tmp_path):
    """The switches are read once per process: a fresh python under SNB_SCALAR_ENERGY_KERNEL runs RF and PME-R0 on lj_big in single
    precision, energy + forces, on k_direct<float, MC, false, true, ..>."""
    out = tmp_path / "scalar.json"
    env = dict(os.environ, SNB_SCALAR_ENERGY_KERNEL="1")
    r = subprocess.run(["timeout", "-k", "10", "120", sys.executable, os.path.join(ROOT, "tests", "vdw_census.py"), "scalar", str(out)], env=env, capture_output=True, text=True)
    assert r.returncode == 0, "the child process exited with %d:\n%s" % (r.returncode, r.stderr[-4000:])
    with open(out) as f:
        recs = json.load(f)
    for row, sdf in V.SCALAR_CASES:
        rec = recs["%s %.1f" % (row, sdf)]
        _check(rec, "scalar energy kernel lj_big %s sd %.1f" % (row, sdf), "single", V.BARS["single"])
        assert rec["host_rebuilds"] == 0
        if not any(k in os.environ for k in ("SNB_EWALD_ERFC", "SNB_EWALD_POLY_ALWAYS")):
            assert rec["mask"] == V.expected_mask(row, "single")


@pytest.mark.parametrize("prec", ["single", "double"])
@pytest.mark.parametrize("row", ["RF", "PME-R0"])
def test_planted_defect_fails_on_hardware(row, prec, snb, oracle):
    """An engine created with a switching distance of 0.909 against an oracle at 0.9: more than half of the atoms over the bar, with
    ordinary finite numbers (tests/test_vdw_census.py: 94 % between the oracle and itself)."""
    rec = V.bulk_case(snb, "lj_big", row, 0.9, prec, steps=("ef",), engine_sd=0.909)
    print("VDW planted sd 0.909 lj_big %s | %s | flagged %.3f | %s" % (row, prec, rec["flagged"], "; ".join("%s %.3e" % c[:2] for c in rec["checks"])))
    assert rec["finite"]
    assert rec["flagged"] > 0.5, "the census cannot see a switching distance 1 % off"
    _identity(rec, row, prec, True)
