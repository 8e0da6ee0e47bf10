"""Per-atom forces by subset and term (snb_evaluate_atom_forces, include/snb.h): the entry point's prototype, export and binding, and the
pure-numpy helpers of the Python kernel against oracle truths on a 40-atom box.  No GPU needed."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import atom_force_truth as aft
import systems

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_prototype_compiles_against_the_header(tmp_path):
    """A function pointer of the exact prototype takes the symbol: any other declaration in snb.h is an incompatible-pointer error."""
    src = tmp_path / "proto.c"
    src.write_text('#include "snb.h"\n'
                   'snb_status (*fp)(snb_handle, int32_t, int32_t, double*, int32_t) = snb_evaluate_atom_forces;\n'
                   'int main(void) { return fp == 0; }\n')
    subprocess.check_call(["gcc", "-Werror", "-Wall", "-pedantic-errors", "-c", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(tmp_path / "proto.o")])


def test_entry_point_is_exported_listed_and_typed(snb):
    capi = snb.capi
    assert "snb_evaluate_atom_forces" in capi.SYMBOLS
    assert getattr(ctypes.CDLL(capi.LIB_PATH), "snb_evaluate_atom_forces") is not None
    L = capi.lib()
    assert L.snb_evaluate_atom_forces.argtypes == [ctypes.c_void_p, ctypes.c_int32, ctypes.c_int32, ctypes.c_void_p, ctypes.c_int32]
    assert L.snb_evaluate_atom_forces(None, 1, 1, None, 0) == capi.SNB_ERR_INVALID_ARGUMENT      # a null handle is refused before anything else
    assert capi.SNB_ABI_VERSION == 8 and L.snb_abi_version() == 8      # additive


@pytest.fixture(scope="module", params=["PME", "CutoffPeriodic"])
def small(request, snb, oracle):
    """40 atoms, 3 subsets, periodic: the truth table (full and direct-only) and an evaluator of the oracle's forces at any lambda state."""
    F = snb.SlicedNonbondedForce
    force, pos, box = systems.random_box(F, 40, 3, getattr(F, request.param), 2.05, 1.0, pme=(2.6283, 20, 20, 20))
    subset = aft.force_subsets(force)
    ev = aft.force_evaluator(oracle, force, pos, box)
    direct = aft.truth_table(aft.force_evaluator(oracle, force, pos, box, include_reciprocal=False), subset, 3)
    return dict(subset=subset, ev=ev, truth=aft.truth_table(ev, subset, 3), direct=direct)


def test_forces_from_atom_forces(small, snb):
    """Linearity in the lambdas: the truth table contracted with a lambda state is the oracle's force at that state."""
    K = snb.HipCalcSlicedNonbondedForceKernel
    truth, subset = small["truth"], small["subset"]
    assert truth.shape == (40, 3, 2, 3) and np.abs(truth).max() > 1.0
    for lam in (np.ones((6, 2)), np.random.default_rng(11).uniform(0.0, 1.0, (6, 2))):
        want = small["ev"](lam)
        got = K.forcesFromAtomForces(truth, subset, lam)
        assert got.shape == (40, 3)
        err = float((np.linalg.norm(got - want, axis=1) / np.maximum(np.linalg.norm(want, axis=1), 1.0)).max())
        assert err <= 1e-9, err
        np.testing.assert_allclose(got, aft.contract(truth, subset, lam), rtol=0, atol=1e-9)      # (the helper against the sum written out)


def test_group_atom_forces(small, snb):
    K = snb.HipCalcSlicedNonbondedForceKernel
    truth, subset = small["truth"], small["subset"]
    groups = [list(range(a, min(a + 7, 40))) for a in range(0, 40, 7)]      # a partition into "residues" of 7 atoms (the last has 5)
    g = K.groupAtomForces(truth, groups)
    assert g.shape == (len(groups), 3, 2, 3)
    np.testing.assert_allclose(g[1], truth[7:14].sum(axis=0), rtol=0, atol=1e-12)
    np.testing.assert_allclose(g.sum(axis=0), truth.sum(axis=0), rtol=0, atol=1e-9)
    by_subset = K.groupAtomForces(truth, [np.flatnonzero(subset == s) for s in range(3)])
    for s in range(3):
        np.testing.assert_allclose(by_subset[s], truth[subset == s].sum(axis=0), rtol=0, atol=1e-12)
    assert K.groupAtomForces(truth, [[], [3]]).shape == (2, 3, 2, 3) and not K.groupAtomForces(truth, [[]]).any()


def test_direct_truth_obeys_the_third_law_slice_by_slice(small):
    """Without the reciprocal part every contribution is a pair force: what subset J puts on subset I and what I puts on J cancel."""
    tl = aft.third_law(small["direct"], small["subset"], 3)
    assert np.abs(tl).max() <= 1e-9, np.abs(tl).max()
    assert np.abs(small["direct"]).max() > 1.0
