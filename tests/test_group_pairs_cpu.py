"""Group-pair interaction energy matrix (snb_evaluate_group_pair_energies, include/snb.h): the layout of snb_group_pair_batch as gcc sees it
against the ctypes mirror, the entry point's prototype, export and binding, the three helpers of the Python kernel, and the oracle truth
rule of tests/group_pair_truth.py on the 40-atom box: against the oracle's own direct-only slice energies, under the merge rule, and
against the direct-only rows of tests/group_energy_truth.py.  No GPU needed."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import atom_energy_truth as aet
import group_energy_truth as get
import group_pair_truth as gpt
import systems

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BATCH = ["n_frames", "positions", "is_device", "is_double", "stride4", "boxes", "n_groups", "group_of_atom", "pair_energies", "out_is_device"]
# Two oracle evaluations of the same pairs, summed in another order, under the reference's scale rule |got - want| / max(|want|, 1): the
# 5e-15 class of the neighbouring truth tests on this box.  The oracle alone meets it (printed below: 2e-16 .. 3.3e-15 over the three
# rules and both methods; the worst is the NoCutoff merge rule).
SAME_PAIRS = 5e-15


def test_group_pair_batch_layout_matches_c_compiler(snb, tmp_path):
    B = snb.capi.SnbGroupPairBatch
    assert [f[0] for f in B._fields_] == BATCH
    fmt = " ".join(["%zu"] * (len(BATCH) + 1))
    args = ", ".join(["sizeof(snb_group_pair_batch)"] + ["offsetof(snb_group_pair_batch, %s)" % m for m in BATCH])
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
                   'snb_status (*fp)(snb_handle, const snb_group_pair_batch*) = snb_evaluate_group_pair_energies;\n'
                   'int main(void) { return fp == 0; }\n')
    subprocess.check_call(["gcc", "-Werror", "-Wall", "-pedantic-errors", "-c", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(tmp_path / "proto.o")])


def test_entry_point_is_exported_listed_and_typed(snb):
    capi = snb.capi
    assert "snb_evaluate_group_pair_energies" in capi.SYMBOLS
    assert getattr(ctypes.CDLL(capi.LIB_PATH), "snb_evaluate_group_pair_energies") is not None
    L = capi.lib()
    assert L.snb_evaluate_group_pair_energies.argtypes == [ctypes.c_void_p, ctypes.POINTER(capi.SnbGroupPairBatch)]
    assert L.snb_evaluate_group_pair_energies(None, None) == capi.SNB_ERR_INVALID_ARGUMENT      # a null batch / handle is refused before anything else
    assert L.snb_evaluate_group_pair_energies(None, ctypes.byref(capi.SnbGroupPairBatch())) == capi.SNB_ERR_INVALID_ARGUMENT
    assert capi.SNB_ABI_VERSION == 8 and L.snb_abi_version() == 8      # additive


def test_python_helpers(snb):
    K = snb.HipCalcSlicedNonbondedForceKernel
    # groupPairIndex: the slice indexing, symmetric
    assert [K.groupPairIndex(g, h) for g, h in ((0, 0), (1, 0), (0, 1), (1, 1), (2, 0), (2, 2), (3, 1), (4095, 4095))] == [0, 1, 1, 2, 3, 5, 7, 4096 * 4097 // 2 - 1]
    for g in range(7):
        for h in range(7):
            assert K.groupPairIndex(g, h) == aet.slice_index(g, h) == snb.sliceIndex(g, h)
    with pytest.raises(snb.OpenMMException):
        K.groupPairIndex(-1, 0)
    # groupPairMatrix: [..., P, 2] -> symmetric [..., G, G, 2]
    G = 5; P = G * (G + 1) // 2
    rows = np.random.default_rng(5).standard_normal((3, 2, P, 2))
    full = K.groupPairMatrix(rows, G)
    assert full.shape == (3, 2, G, G, 2)
    for g in range(G):
        for h in range(G):
            assert np.array_equal(full[:, :, g, h], rows[:, :, K.groupPairIndex(g, h)])
    assert np.array_equal(full, np.swapaxes(full, -3, -2))
    assert K.groupPairMatrix(rows[0, 0], G).shape == (G, G, 2)
    with pytest.raises(snb.OpenMMException):
        K.groupPairMatrix(rows, G + 1)
    # labelsFromGroups: disjoint lists -> labels, -1 elsewhere; overlap refused
    lab = K.labelsFromGroups([[0, 1, 2], [], range(5, 7), np.array([4])], 9)
    assert lab.dtype == np.int32 and lab.tolist() == [0, 0, 0, -1, 3, 2, 2, -1, -1]
    with pytest.raises(snb.OpenMMException, match="listed twice"):
        K.labelsFromGroups([[0, 1], [1, 2]], 4)
    with pytest.raises(snb.OpenMMException, match="listed twice"):
        K.labelsFromGroups([[3, 3]], 4)
    with pytest.raises(snb.OpenMMException):
        K.labelsFromGroups([[4]], 4)


def _box40(snb, method):
    F = snb.SlicedNonbondedForce
    return systems.random_box(F, 40, 3, getattr(F, method), 2.05, 1.0, pme=(2.6283, 20, 20, 20))


@pytest.mark.parametrize("method", ["PME", "NoCutoff"])
def test_truth_rule_on_the_40_atom_box(method, snb, oracle):
    """(i) labels = subsets: the matrix IS the oracle's direct-only slice energies, exactly; (ii) the merge rule: merging labels g, h gives
    M'[gg] = M[gg] + M[hh] + M[gh] and M'[gk] = M[gk] + M[hk]; (iii) with every atom labelled, sum_h (1 + delta_gh) M[g][h] is the
    direct-only row of the group-energy truth, per term, summed over the subsets.
    This test runs the oracle and tests/group_pair_truth.py alone -- no entry point of the library -- so, unlike the other tests of this
    file, it does not depend on the engine having the call."""
    force, pos, box = _box40(snb, method)
    subset = aet.force_subsets(force)
    ev = gpt.direct_force_evaluator(oracle, force, pos, box)
    # (i)
    direct = np.asarray(ev(subset, 3))
    M3 = gpt.truth(ev, subset, 3)
    assert M3.shape == (6, 2) and np.array_equal(M3, direct)
    full = np.asarray(aet.force_evaluator(oracle, force, pos, box)(subset, 3))
    if method == "PME":
        assert np.abs(full - direct).max() > 1.0      # (the evaluator really leaves the reciprocal part out)
    else:
        assert np.array_equal(full, direct)
    # a labelling of its own: i % 5, and the same with -1 on a third of the atoms (those rows lose pairs, none gains)
    lab = np.arange(40) % 5
    M = gpt.truth(ev, lab, 5)
    assert M.shape == (15, 2) and np.abs(M).max() > 1.0
    err_total = aet.rel(M.sum(axis=0), direct.sum(axis=0))
    # (ii)
    worst = 0.0
    for g, h in ((0, 1), (1, 4), (2, 3)):
        lab2 = np.where(lab == h, g, np.where(lab > h, lab - 1, lab))
        worst = max(worst, aet.rel(gpt.truth(ev, lab2, 4), gpt.merged(M, 5, g, h)))
    # (iii)
    dev = aet.force_evaluator(oracle, force, pos, box, include_reciprocal=False)
    rows = get.truth(dev, subset, 3, [np.flatnonzero(lab == g) for g in range(5)]).sum(axis=1)      # [G][2]
    err_rows = aet.rel(gpt.group_totals(M, 5), rows)
    # unlabelled atoms: the kept rows are those of the labelled atoms among themselves
    lab3 = np.where(np.arange(40) % 3 == 0, -1, lab)
    M_part = gpt.truth(ev, lab3, 5)
    sub6 = gpt.relabelled(lab3, 5)
    assert (sub6 == 5).sum() == 14 and np.array_equal(M_part, np.asarray(ev(sub6, 6))[:15])
    print("%s: total %.3e, merge rule %.3e, group rows %.3e" % (method, err_total, worst, err_rows))
    assert err_total <= SAME_PAIRS and worst <= SAME_PAIRS and err_rows <= SAME_PAIRS, (err_total, worst, err_rows)
