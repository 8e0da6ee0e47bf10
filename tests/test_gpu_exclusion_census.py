"""Exclusion and exception census on the GPU: the Ewald exclusion corrections and the 1-4 exceptions alone, against closed forms
(tests/exclusion_census.py; tests/test_exclusion_census.py proves the instrument on the CPU).

The systems are gases of isolated molecules evaluated in direct space only: the tile loop finds no pair with a non-zero term, so every force,
slice energy and table entry is the two O(N) lists' and has a float64 closed form per pair.  Per case (row, method, cell, exceptions_periodic,
list builder) and precision, on one engine (the eager step has one of its own):

   f eager / f captured / f replay 1, 2     forces only: disable_graph = 1; captured; replayed on the same list after a seeded drift
                                            -- the list blocks of k_directPacked<., ENERGY = false> (single, mixed) / k_direct (double)
   f offsets / f offsets back               a global parameter moves charges of excluded atoms and chargeProd / epsilon of 1-4 exceptions
                                            between two replayed steps, no rebuild
   f crossed                                atoms of the straddling chains cross a face on the unchanged list
   ef forces / energies / total             energy + forces -- the list blocks of the ENERGY instantiations of k_directPacked / k_direct
   e energies                               energy only, every slice -- the list blocks of k_directPackedEnergy / k_directEnergy
                                            (exclusionAtomsBody / exceptionsBody<., true, FORCES = false>, wantE true throughout)
   d .. / d after mask change ..            derivative only (include_forces = 1, include_energy = 2) with a mask that wants some slices:
                                            k_directPackedSelected (k_directPacked<LJPME, ., true> under LJPME, k_direct in double), list
                                            bodies <., true, true>: forces for every pair, the wantE branches for the energies
   e masked .. / e masked after ..          energy only with the same masks (include_forces = 0, include_energy = 2): the FORCES = false
                                            list bodies with sliceNeed zero on some slices -- the `!FORCES && !wantE` skip
   atomE, atomF, groupPairs, groupE, groupF the tables: PairEnergy / PairForce::exclusion and ::exception through atom_table.h's
                                            walkers, grouppairs.hip's list loops (groupE / groupF on the R0 rows)

Asserted: every output finite; atoms with no expected contribution have exactly zero force; per-atom force error
|F - F_exp| / max(|F_exp|, floor) <= BARS[prec] (floor 1 kJ/mol/nm, on the uncharged LJPME copy the median non-zero |F_exp|); energies and
table entries through ewald_census.rel at the same bars; which builder ran and that no list overran (skipped under a rerouting SNB_*
switch); on the uncharged copy every Coulomb column exactly zero.  One `XCL ...` line per check leaves the measured errors in the log.

The stand-alone list kernels.  Every tile kernel carries the lists in its own launch, so none of the steps above launches k_pairLists<., false>,
k_pairLists<., true> or k_pairListsEnergy.  test_stand_alone_list_kernels runs three cases (PME, LJPME, the uncharged copy; single and
double) in a child process under SNB_NO_FUSED_LISTS, where the engine launches the lists on their own in every step: the same steps then
reach those three kernels, in float and in double.  Which kernel ran is the switch's doing (engine.hip), not something snb_stats reports.

Control on hardware: an engine created with exceptions_periodic = 1, judged against expected values at 0, is over the bar on exactly the
atoms of the straddling molecules -- a legal configuration with another answer.
"""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import exclusion_census as X

pytestmark = pytest.mark.gpu
PRECISIONS = ("single", "mixed", "double")


def _identity(rec, case):
    if X.rerouted():
        return
    assert (rec["host_rebuilds"] > 0) == bool(case[4]), (rec["host_rebuilds"], "the host lists" if case[4] else "the GPU builder")
    assert rec["overruns"] == 0
    assert rec["rebuilds"] == 1, ("every step must run on the list of the first", rec["rebuilds"])


def _judge(rec, case, what, prec):
    tol = X.BARS[prec]
    for step, err, detail in rec["checks"]:
        print("XCL %s | %s | %s | %.3e | %s" % (what, prec, step, err, detail))
    print("XCL %s | %s | host rebuilds %d, rebuilds %d, overruns %d, Coulomb columns up to %.1e" % (what, prec, rec["host_rebuilds"], rec["rebuilds"], rec["overruns"], rec["coulomb"]))
    assert rec["finite"], "%s %s: a NaN or an infinity in the engine's output" % (what, prec)
    assert rec["zero_ok"], "%s %s: an atom with no expected contribution has a force" % (what, prec)
    if case[5]:
        assert rec["coulomb"] == 0.0, "%s %s: the system is uncharged, a Coulomb column holds %.3e" % (what, prec, rec["coulomb"])
    for step, err, detail in rec["checks"]:
        assert err <= tol, "row %s, %s, step %s: %.3e over %.0e (%s)" % (what, prec, step, err, tol, detail)
    _identity(rec, case)


@pytest.mark.parametrize("prec", PRECISIONS)
@pytest.mark.parametrize("case", X.CASES, ids=[X.case_id(c) for c in X.CASES])
def test_lists_against_the_closed_form(case, prec, snb):
    _judge(X.run_case(snb, case, prec), case, X.case_id(case), prec)


def test_stand_alone_list_kernels(tmp_path):
    """The switches are read once per process: a fresh python under SNB_NO_FUSED_LISTS runs every step of STANDALONE_CASES with the lists
    as a launch of their own -- k_pairLists<float | double, false | true> and k_pairListsEnergy<float | double>."""
    out = tmp_path / "standalone.json"
    env = dict(os.environ, **{X.STANDALONE_SWITCH: "1"})
    r = subprocess.run(["timeout", "-k", "10", "120", sys.executable, os.path.join(os.path.dirname(os.path.abspath(__file__)), "exclusion_census.py"), "standalone", str(out)],
                       env=env, capture_output=True, text=True)
    assert r.returncode == 0, "the child process exited with %d:\n%s" % (r.returncode, r.stderr[-4000:])
    with open(out) as f:
        recs = json.load(f)
    for case in X.STANDALONE_CASES:
        for prec in X.STANDALONE_PRECISIONS:
            _judge(recs["%s %s" % (X.case_id(case), prec)], case, "stand-alone lists %s" % X.case_id(case), prec)


@pytest.mark.parametrize("prec", ["single", "double"])
@pytest.mark.parametrize("case", X.CONTROL_CASES[:3], ids=[X.case_id(c) for c in X.CONTROL_CASES[:3]])
def test_planted_defect_is_flagged_on_hardware(case, prec, snb):
    """exceptions_periodic = 1 in the engine, 0 in the expected values: exactly the atoms of the straddling molecules are over the bar
    (tests/test_exclusion_census.py: they differ by two bars and more, every other atom not at all)."""
    rec = X.run_case(snb, case, prec, engine_periodic=1, steps="control")
    s = X.build(case[0], case[1], prec, case[2], case[3], case[5])
    want = sorted(X.control_atoms(s).tolist())
    got = sorted(rec["flagged"]["f captured"].tolist())
    print("XCL control %s | %s | flagged %d atoms, straddling %d | %s" % (X.case_id(case), prec, len(got), len(want), "; ".join("%s %.3e" % c[:2] for c in rec["checks"])))
    assert rec["finite"]
    assert got == want, "flagged but not straddling: %s; straddling but not flagged: %s" % (sorted(set(got) - set(want))[:10], sorted(set(want) - set(got))[:10])
