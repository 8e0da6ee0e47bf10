"""Per-group interaction energies over stored frames (snb_evaluate_group_energies, include/snb.h): the layout of snb_group_batch as gcc
sees it against the ctypes mirror, the entry point's prototype, export and binding, the CSR helper of the Python kernel, and the oracle
truth rule of tests/group_energy_truth.py against the summed rows of tests/atom_energy_truth.py on a 40-atom box.  No GPU needed."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import atom_energy_truth as aet
import group_energy_truth as get
import systems

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BATCH = ["n_frames", "positions", "is_device", "is_double", "stride4", "boxes", "include_direct", "include_reciprocal", "n_groups", "group_start",
         "group_atoms", "group_energies", "out_is_device"]


def test_group_batch_layout_matches_c_compiler(snb, tmp_path):
    B = snb.capi.SnbGroupBatch
    assert [f[0] for f in B._fields_] == BATCH
    fmt = " ".join(["%zu"] * (len(BATCH) + 1))
    args = ", ".join(["sizeof(snb_group_batch)"] + ["offsetof(snb_group_batch, %s)" % m for m in BATCH])
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "snb.h"\nint main(){printf("%s\\n", %s);return 0;}\n' % (fmt, args))
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = [int(x) for x in subprocess.check_output([str(exe)]).split()]
    assert got == [ctypes.sizeof(B)] + [getattr(B, m).offset for m in BATCH]


def test_prototype_compiles_against_the_header(tmp_path):
    """A function pointer of the exact prototype takes the symbol: any other declaration in snb.h is an incompatible-pointer error."""
    src = tmp_path / "proto.c"
    src.write_text('#include "snb.h"\n'
                   'snb_status (*fp)(snb_handle, const snb_group_batch*) = snb_evaluate_group_energies;\n'
                   'int main(void) { return fp == 0; }\n')
    subprocess.check_call(["gcc", "-Werror", "-Wall", "-pedantic-errors", "-c", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(tmp_path / "proto.o")])


def test_entry_point_is_exported_listed_and_typed(snb):
    capi = snb.capi
    assert "snb_evaluate_group_energies" in capi.SYMBOLS
    assert getattr(ctypes.CDLL(capi.LIB_PATH), "snb_evaluate_group_energies") is not None
    L = capi.lib()
    assert L.snb_evaluate_group_energies.argtypes == [ctypes.c_void_p, ctypes.POINTER(capi.SnbGroupBatch)]
    assert L.snb_evaluate_group_energies(None, None) == capi.SNB_ERR_INVALID_ARGUMENT      # a null batch / handle is refused before anything else
    assert L.snb_evaluate_group_energies(None, ctypes.byref(capi.SnbGroupBatch())) == capi.SNB_ERR_INVALID_ARGUMENT
    assert capi.SNB_ABI_VERSION == 8 and L.snb_abi_version() == 8      # additive


def test_groups_to_csr(snb):
    K = snb.HipCalcSlicedNonbondedForceKernel
    groups = [[0, 1, 2], [2, 3], [], [5, 5, 1], range(6, 9), np.array([4])]      # overlapping, empty, an index twice, any iterable
    start, atoms = K.groupsToCSR(groups)
    assert start.dtype == np.int32 and atoms.dtype == np.int32 and atoms.flags["C_CONTIGUOUS"]
    assert start.tolist() == [0, 3, 5, 5, 8, 11, 12]
    assert atoms.tolist() == [0, 1, 2, 2, 3, 5, 5, 1, 6, 7, 8, 4]
    for g, lst in enumerate(groups):
        assert atoms[start[g]:start[g + 1]].tolist() == [int(a) for a in lst]
    # the reduction groupAtomEnergies does over the same lists, written through the CSR form
    table = np.random.default_rng(3).standard_normal((9, 3, 2))
    want = K.groupAtomEnergies(table, groups)
    got = np.stack([table[atoms[start[g]:start[g + 1]]].sum(axis=0) for g in range(len(groups))])
    np.testing.assert_allclose(got, want, rtol=0, atol=1e-15)
    assert not want[2].any() and np.allclose(want[3], 2 * table[5] + table[1])
    start, atoms = K.groupsToCSR([[], []])      # only empty groups
    assert start.tolist() == [0, 0, 0] and atoms.shape == (0,)


@pytest.mark.parametrize("method", ["PME", "CutoffPeriodic", "LJPME"])
def test_moved_group_rule_reproduces_the_summed_atom_rows(method, snb, oracle):
    """The rule of group_energy_truth -- one oracle evaluation per (group, subset) part -- against the sum of the singled-out rows of
    atom_energy_truth (one evaluation per atom), 40 atoms in 3 subsets: groups inside a subset, across subsets, a whole subset (its
    subset left empty), every atom, an empty group, an index listed twice."""
    F = snb.SlicedNonbondedForce
    force, pos, box = systems.random_box(F, 40, 3, getattr(F, method), 2.05, 1.0, pme=(2.6283, 20, 20, 20), ljpme=(2.6283, 12, 12, 12))
    subset = aet.force_subsets(force)
    ev = aet.force_evaluator(oracle, force, pos, box)
    rows = aet.truth_table(ev, subset, 3)
    one = np.flatnonzero(subset == 1)
    groups = [list(one[:3]), list(range(0, 7)), list(range(33, 40)), list(one), list(range(40)), [], [int(one[0]), 5, int(one[0])]]
    got = get.truth(ev, subset, 3, groups)
    want = np.stack([rows[np.asarray(g, dtype=np.int64)].sum(axis=0) if len(g) else np.zeros((3, 2)) for g in groups])
    err = aet.rel(got, want)
    print("%s: moved-group rule against summed atom rows: %.3e" % (method, err))
    assert err <= 1e-9, err
    assert not got[5].any()
