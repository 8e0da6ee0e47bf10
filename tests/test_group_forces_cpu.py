"""Per-group forces over stored frames (snb_evaluate_group_forces, include/snb.h): the layout of snb_group_force_batch as gcc sees it against
the ctypes mirror, the entry point's prototype, export and binding, the NumPy statement of state_forces (groupForcesAtStates) against a
hand-written triple loop, and the state truth of tests/group_force_truth.py (the oracle's plain forces at a lambda state, summed per
group) against the contracted one-hot truth table on a 40-atom box.  No GPU needed."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import atom_force_truth as aft
import group_force_truth as gft
import systems

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BATCH = ["n_frames", "positions", "is_device", "is_double", "stride4", "boxes", "include_direct", "include_reciprocal", "n_groups", "group_start",
         "group_atoms", "group_forces", "out_is_device", "n_states", "state_lambdas", "state_forces"]


def test_group_force_batch_layout_matches_c_compiler(snb, tmp_path):
    B = snb.capi.SnbGroupForceBatch
    assert [f[0] for f in B._fields_] == BATCH
    fmt = " ".join(["%zu"] * (len(BATCH) + 1))
    args = ", ".join(["sizeof(snb_group_force_batch)"] + ["offsetof(snb_group_force_batch, %s)" % m for m in BATCH])
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "snb.h"\nint main(){printf("%s\\n", %s);return 0;}\n' % (fmt, args))
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = [int(x) for x in subprocess.check_output([str(exe)]).split()]
    assert got == [ctypes.sizeof(B)] + [getattr(B, m).offset for m in BATCH]
    # the frames and the groups sit where snb_group_batch has them
    A = snb.capi.SnbGroupBatch
    for m in BATCH[:11] + ["out_is_device"]:
        assert getattr(A, m).offset == getattr(B, m).offset, m
    assert A.group_energies.offset == B.group_forces.offset


def test_prototype_compiles_against_the_header(tmp_path):
    """A function pointer of the exact prototype takes the symbol: any other declaration in snb.h is an incompatible-pointer error."""
    src = tmp_path / "proto.c"
    src.write_text('#include "snb.h"\n'
                   'snb_status (*fp)(snb_handle, const snb_group_force_batch*) = snb_evaluate_group_forces;\n'
                   'int main(void) { return fp == 0; }\n')
    subprocess.check_call(["gcc", "-Werror", "-Wall", "-pedantic-errors", "-c", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(tmp_path / "proto.o")])


def test_entry_point_is_exported_listed_and_typed(snb):
    capi = snb.capi
    assert "snb_evaluate_group_forces" in capi.SYMBOLS
    assert getattr(ctypes.CDLL(capi.LIB_PATH), "snb_evaluate_group_forces") is not None
    L = capi.lib()
    assert L.snb_evaluate_group_forces.argtypes == [ctypes.c_void_p, ctypes.POINTER(capi.SnbGroupForceBatch)]
    assert L.snb_evaluate_group_forces(None, None) == capi.SNB_ERR_INVALID_ARGUMENT      # a null batch / handle is refused before anything else
    assert L.snb_evaluate_group_forces(None, ctypes.byref(capi.SnbGroupForceBatch())) == capi.SNB_ERR_INVALID_ARGUMENT
    assert capi.SNB_ABI_VERSION == 8 and L.snb_abi_version() == 8      # additive


def test_group_forces_at_states_against_the_triple_loop(snb):
    """groupForcesAtStates(table, subsets, groups, states)[k][g] = sum_{i in g} sum_J sum_t states[k][slice(s_i, J)][t] table[i][J][t],
    written out: groups across subsets, overlapping, empty, with an index listed twice."""
    K = snb.HipCalcSlicedNonbondedForceKernel
    rng = np.random.default_rng(5)
    n, nsub = 23, 3
    S = nsub * (nsub + 1) // 2
    table = rng.standard_normal((n, nsub, 2, 3))
    subsets = rng.integers(0, nsub, n)
    states = rng.uniform(0.0, 1.0, (4, S, 2))
    groups = [[0, 1, 2], list(range(n)), [], [5, 5, 1], list(np.flatnonzero(subsets == 1)), range(6, 20)]
    got = K.groupForcesAtStates(table, subsets, groups, states)
    assert got.shape == (4, len(groups), 3)
    want = np.zeros_like(got)
    for k in range(4):
        for g, atoms in enumerate(groups):
            for i in atoms:
                for J in range(nsub):
                    for t in range(2):
                        want[k, g] += states[k, aft.slice_index(int(subsets[i]), J), t] * table[i, J, t]
    np.testing.assert_allclose(got, want, rtol=0, atol=1e-12)
    assert not got[:, 2].any()
    # all lambdas 1: the plain sum over columns and terms
    ones = K.groupForcesAtStates(table, subsets, groups, np.ones((1, S, 2)))
    np.testing.assert_allclose(ones[0], K.groupAtomForces(table, groups).sum(axis=(1, 2)), rtol=0, atol=1e-12)


@pytest.mark.parametrize("method", ["PME", "CutoffPeriodic", "LJPME"])
def test_state_truth_is_the_contracted_table_summed_per_group(method, snb, oracle):
    """40 atoms in 3 subsets: the oracle's plain forces at lambda_k summed over a group (state_truth: one evaluation per state) against
    contract(truth_table, subset, lambda_k) summed over the group (2 S one-hot evaluations): groups inside a subset, across subsets, a
    whole subset, every atom, an empty group, an index listed twice.  And the rows: the table summed per group, column by column."""
    F = snb.SlicedNonbondedForce
    force, pos, box = systems.random_box(F, 40, 3, getattr(F, method), 2.05, 1.0, pme=(2.6283, 20, 20, 20), ljpme=(2.6283, 12, 12, 12))
    subset = aft.force_subsets(force)
    ev = aft.force_evaluator(oracle, force, pos, box)
    table = aft.truth_table(ev, subset, 3)
    assert np.abs(table).max() > 1.0
    one = np.flatnonzero(subset == 1)
    groups = [list(one[:3]), list(range(0, 7)), list(range(33, 40)), list(one), list(range(40)), [], [int(one[0]), 5, int(one[0])]]
    rows = gft.rows_truth(table, groups)
    assert rows.shape == (len(groups), 3, 2, 3) and not rows[5].any()
    np.testing.assert_allclose(rows[6], 2 * table[one[0]] + table[5], rtol=0, atol=1e-9)
    np.testing.assert_allclose(rows, gft.rows(ev, subset, 3, groups), rtol=0, atol=1e-9)
    rng = np.random.default_rng(13)
    for lam in (np.ones((6, 2)), rng.uniform(0.0, 1.0, (6, 2)), rng.uniform(0.0, 1.0, (6, 2))):
        got = gft.state_truth(ev(lam), groups)
        want = np.stack([aft.contract(table, subset, lam)[np.asarray(g, dtype=np.int64)].sum(axis=0) if len(g) else np.zeros(3) for g in groups])
        err = gft.rel(got, want)
        print("%s: state truth against the contracted table, per group: %.3e" % (method, err))
        assert err <= 1e-9, err
        assert not got[5].any()
