"""Per-atom interaction energies (snb_evaluate_atom_energies, include/snb.h): the entry point's prototype, export and binding, and the
pure-numpy helpers of the Python kernel against oracle truths on a 40-atom box.  No GPU needed."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import atom_energy_truth as aet
import systems

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_prototype_compiles_against_the_header(tmp_path):
    """A function pointer of the exact prototype takes the symbol: any other declaration in snb.h is an incompatible-pointer error."""
    src = tmp_path / "proto.c"
    src.write_text('#include "snb.h"\n'
                   'snb_status (*fp)(snb_handle, int32_t, int32_t, double*, int32_t) = snb_evaluate_atom_energies;\n'
                   'int main(void) { return fp == 0; }\n')
    subprocess.check_call(["gcc", "-Werror", "-Wall", "-pedantic-errors", "-c", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(tmp_path / "proto.o")])


def test_entry_point_is_exported_listed_and_typed(snb):
    capi = snb.capi
    assert "snb_evaluate_atom_energies" in capi.SYMBOLS
    assert getattr(ctypes.CDLL(capi.LIB_PATH), "snb_evaluate_atom_energies") is not None
    L = capi.lib()
    assert L.snb_evaluate_atom_energies.argtypes == [ctypes.c_void_p, ctypes.c_int32, ctypes.c_int32, ctypes.c_void_p, ctypes.c_int32]
    assert L.snb_evaluate_atom_energies(None, 1, 1, None, 0) == capi.SNB_ERR_INVALID_ARGUMENT      # a null handle is refused before anything else
    assert capi.SNB_ABI_VERSION == 8 and L.snb_abi_version() == 8      # additive


@pytest.fixture(scope="module", params=["PME", "CutoffPeriodic"])
def small(request, snb, oracle):
    """40 atoms, 3 subsets, periodic: the oracle's slice energies of the system as it is and the truth row of every atom."""
    F = snb.SlicedNonbondedForce
    force, pos, box = systems.random_box(F, 40, 3, getattr(F, request.param), 2.05, 1.0, pme=(2.6283, 20, 20, 20))
    subset = aet.force_subsets(force)
    ev = aet.force_evaluator(oracle, force, pos, box)
    return dict(subset=subset, slices=ev(subset, 3), truth=aet.truth_table(ev, subset, 3))


def test_slice_energies_from_atom_energies(small, snb):
    """The singled-out rule implies the sum rule: the truth table reduces to the oracle's slice energies of the unmodified system."""
    K = snb.HipCalcSlicedNonbondedForceKernel
    got = K.sliceEnergiesFromAtomEnergies(small["truth"], small["subset"])
    assert got.shape == (6, 2)
    assert aet.rel(got, small["slices"]) <= 1e-9
    lo, hi = aet.reduce_by_sum_rule(small["truth"], small["subset"], 3)      # (either half of the table gives an off-diagonal slice)
    assert aet.rel(lo, small["slices"]) <= 1e-9 and aet.rel(hi, small["slices"]) <= 1e-9


def test_group_atom_energies(small, snb):
    K = snb.HipCalcSlicedNonbondedForceKernel
    truth, subset = small["truth"], small["subset"]
    groups = [list(range(a, min(a + 7, 40))) for a in range(0, 40, 7)]      # a partition into "residues" of 7 atoms (the last has 5)
    g = K.groupAtomEnergies(truth, groups)
    assert g.shape == (len(groups), 3, 2)
    np.testing.assert_allclose(g[1], truth[7:14].sum(axis=0), rtol=0, atol=1e-12)
    np.testing.assert_allclose(g.sum(axis=0), truth.sum(axis=0), rtol=0, atol=1e-9)
    by_subset = K.groupAtomEnergies(truth, [np.flatnonzero(subset == s) for s in range(3)])      # groups = the subsets: the column sums per subset
    for s in range(3):
        np.testing.assert_allclose(by_subset[s], truth[subset == s].sum(axis=0), rtol=0, atol=1e-12)
    assert K.groupAtomEnergies(truth, [[], [3]]).shape == (2, 3, 2) and not K.groupAtomEnergies(truth, [[]]).any()
