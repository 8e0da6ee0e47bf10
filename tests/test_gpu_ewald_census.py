"""Ewald-parameter census on the GPU: the pair kernels' direct-space Ewald terms off the benchmark's alpha.

The kernels evaluate erfc / exp terms with polynomials of fixed degree, fitted for z = alpha (cutoff + padding + 0.02); the fit error
grows fast with z, and csrc/ewald_fit.h keeps a polynomial only where its measured residual passes a guard.  Every other
oracle comparison of the suite sits at z <= 2.94; the rows of tests/ewald_census.py walk z from 1.1 to 4.8.

 (a) bulk: systems.random_box against the oracle, direct space alone (include_reciprocal = 0: no mesh error hides or mimics anything),
     every step kind the polynomials live in, at the parity bars with max(|x|, 1) scaling; the polynomial mask the CPU guard predicts
     (tests/test_ewald_fit_cpu.py) is asserted, so a fallback that stayed away cannot pass by luck.  3000 atoms in 3.2 nm run on host
     lists with per-pair wrapping, i.e. on the scalar tile kernel, which has polynomials in double precision only: those cases test
     double precision and, in single and mixed, the analytic branches.  13 824 atoms in 6 nm run the GPU builder (asserted:
     n_host_rebuilds == 0; it never builds per-pair-wrap lists) and so, in single and mixed precision, the packed kernels: rows R0 .. R6
     there, with every float mask 3, 2 and 0, plus classic Ewald and LJPME
 (b) radial dimers against the closed form, no oracle: nothing cancels, a failure names the radius; forces-only, energy + forces and
     energy-only steps (the three ways the single-precision switch is taken)
 (c) control: the forces-only steps of (a) at 13 824 atoms and the dimers of (b), each in a child process under SNB_EWALD_POLY_ALWAYS
     (the behaviour before the guard), must fail on R3 and R4 in single and on R4 in double, with ordinary finite numbers, and pass on R0
"""
import json
import os
import subprocess
import sys

import pytest

import ewald_census as EC

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PRECISIONS = ("single", "mixed", "double")

BULK = ([(r, EC.PME, "small") for r in EC.ROWS] + [("R0", EC.LJPME, "small"), ("R4", EC.LJPME, "small"), ("R4D", EC.LJPME, "small"), ("R4", EC.EWALD, "small")]
        # the packed single-precision kernels: every float mask (R0, R6: 3; R1: 2, i.e. forces-only and energy + forces steps without, the
        # energy-only step with its polynomial; R2 .. R5: 0), classic Ewald, LJPME
        + [(r, EC.PME, "big") for r in ("R0", "R1", "R2", "R3", "R4", "R5", "R6")] + [("R1", EC.EWALD, "big"), ("R4", EC.EWALD, "big"), ("R1", EC.LJPME, "big")])
DIMERS = ([(r, EC.PME, h) for r in ("R0", "R3", "R4", "R7") for h in (0, 1)] + [(r, EC.PME, 0) for r in ("R1", "R2", "R6")] + [("R1", EC.EWALD, 0)]
          + [(r, EC.LJPME, h) for r in ("R0", "R4", "R4D") for h in (0, 1)])


def _check(rec, what, prec, tol):
    print("%s %s: mask %d, host rebuilds %d, %s" % (what, prec, rec["mask"], rec["host_rebuilds"], ", ".join("%s %.3e" % kv for kv in rec["errors"].items())), rec.get("worst", ""))
    assert rec["finite"], "%s: a NaN or an infinity in the engine's output" % what
    for step, err in rec["errors"].items():
        assert err <= tol, "%s %s, step %s: %.3e over %.0e %s" % (what, prec, step, err, tol, rec.get("worst", ""))


@pytest.mark.parametrize("prec", PRECISIONS)
@pytest.mark.parametrize("name,method,size", BULK, ids=["%s-%d-%s" % b for b in BULK])
def test_bulk_direct_space_against_the_oracle(name, method, size, prec, snb, oracle):
    rec = bulk_case(snb, oracle, name, prec, method, size)
    _check(rec, "bulk %s method %d %s" % (name, method, size), prec, EC.TOLS[prec])
    assert rec["mask"] == EC.engine_mask(EC.row_of(name), prec, method), (rec["mask"], "the guard's decisions are not the ones the CPU test derives")
    if name == "R0":
        assert rec["mask"] == (3 if EC.is_float(prec) else (5 if method == EC.LJPME else 1))      # the benchmark point: every polynomial the kernels have
    assert (rec["host_rebuilds"] == 0) == (size == "big"), rec["host_rebuilds"]      # 3000 atoms in 3.2 nm: the host lists; 13 824 in 6 nm: the GPU builder


def bulk_case(snb, oracle, name, prec, method, size):
    return EC.bulk_case(snb, oracle, name, prec, method, EC.BULK_BIG if size == "big" else EC.BULK_SMALL, tables=(size == "small" and method == EC.PME and name in EC.TABLE_ROWS))


@pytest.mark.parametrize("prec", PRECISIONS)
@pytest.mark.parametrize("name,method,host", DIMERS, ids=["%s-%d-%s" % (r, m, "host" if h else "gpu") for r, m, h in DIMERS])
def test_dimers_against_the_closed_form(name, method, host, prec, snb):
    rec = EC.dimer_case(snb, name, prec, method, host)
    _check(rec, "dimers %s method %d %s builder" % (name, method, "host" if host else "GPU"), prec, EC.TOLS[prec])
    assert rec["outside_zero"], "a pair beyond the cutoff has a force"
    assert rec["mask"] == EC.engine_mask(EC.row_of(name), prec, method)
    assert (rec["host_rebuilds"] > 0) == bool(host), rec["host_rebuilds"]


def _control(kind, tmp_path):
    """The control cases in a fresh process with SNB_EWALD_POLY_ALWAYS set (the switches are read once per process)."""
    out = tmp_path / "control.json"
    env = dict(os.environ, SNB_EWALD_POLY_ALWAYS="1")
    env.pop("SNB_EWALD_ERFC", None)
    r = subprocess.run(["timeout", "-k", "10", "120", sys.executable, os.path.join(ROOT, "tests", "ewald_census.py"), "control", kind, str(out)], env=env, capture_output=True, text=True)
    assert r.returncode == 0, "the control process exited with %d:\n%s" % (r.returncode, r.stderr[-4000:])
    with open(out) as f:
        return json.load(f)


@pytest.mark.parametrize("kind", ["bulk", "dimers"])
def test_control_unguarded_polynomials_fail_where_the_cpu_emulation_says(kind, tmp_path):
    control = _control(kind, tmp_path)
    for name, prec in EC.CONTROL:
        rec = control["%s %s %s" % (kind, name, prec)]
        tol = EC.TOLS[prec]
        print("control %s %s %s: mask %d, %s" % (kind, name, prec, rec["mask"], ", ".join("%s %.3e" % kv for kv in rec["errors"].items())), rec.get("worst", ""))
        assert rec["finite"], "control %s %s %s: a NaN or an infinity, not a polynomial's error" % (kind, name, prec)
        assert rec["mask"] == EC.engine_mask(EC.ROWS[name], prec, EC.PME, control=True)
        forces = [v for k, v in rec["errors"].items() if k in ("f1", "f2", "f")]      # the forces-only steps: the polynomials live there in both precisions
        assert forces
        if prec in EC.ROWS[name]["parent_fails"]:
            assert min(forces) > tol, "the unguarded polynomials pass on %s %s: the row cannot see the defect" % (name, prec)
        else:
            assert name == "R0" and max(rec["errors"].values()) <= tol
