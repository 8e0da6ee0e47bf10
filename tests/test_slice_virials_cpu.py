"""Per-slice virial tensors without a GPU: the oracle's ground truth against closed statements, the C ABI of snb_evaluate_slice_virials
(include/snb.h) and the NumPy helpers.  Additive: the ABI version stays 8."""
import ctypes
import importlib
import os
import subprocess

import numpy as np
import pytest

import slice_virial_truth as svt
import systems

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BATCH = ["n_frames", "positions", "is_device", "is_double", "stride4", "boxes", "include_direct", "include_reciprocal", "slice_virials", "out_is_device",
         "n_states", "state_lambdas", "state_virials"]


@pytest.fixture(scope="module")
def cluster(snb, oracle):
    """60 atoms, 3 subsets, NoCutoff, exclusions and 1-4s: the truth from the oracle, once."""
    F = snb.SlicedNonbondedForce
    force, pos, _ = systems.random_box(F, 60, 3, F.NoCutoff, 2.05, 1.0)
    w, e, worst = svt.truth(svt.force_energy(oracle, force), pos, None)
    print("60-atom cluster: stencils at h and 2h differ by %.3e of the entry's scale" % worst)
    return force, pos, w, e


def test_coulomb_virial_trace_is_the_coulomb_energy(cluster):
    """The Coulomb energy of a cluster is homogeneous of degree -1 in the coordinates: tr W[s][0] = E[s][0]."""
    _, _, w, e = cluster
    assert np.abs(e[:, 0]).max() > 10.0
    tr = w[:, 0, :3].sum(axis=1)
    err = np.abs(tr - e[:, 0]) / np.maximum(np.abs(e[:, 0]), 1.0)
    print("trace against energy: worst %.3e" % err.max())
    assert err.max() < svt.BAR


def test_truth_equals_the_written_out_pair_sum(cluster):
    force, pos, w, e = cluster
    want = svt.pair_sum(force, pos)
    assert svt.frobenius(want)[:, 0].min() > 1.0 and svt.frobenius(want)[:, 1].min() > 0.0      # (every slice and both terms carry something)
    err = svt.ratios(w, want, e)
    print("stencil against sum d_a d_b f: worst %.3e" % err.max())
    assert err.max() < svt.BAR
    # symmetric tensors whose shear entries are not small: a transposed or dropped component would show
    assert (np.abs(want[..., 3:]).max(axis=-1) > 1e-3 * svt.frobenius(want)).all()


def test_truth_refuses_a_pair_in_the_cutoff_shell(snb, oracle):
    F = snb.SlicedNonbondedForce
    force, pos, box = systems.random_box(F, 60, 3, F.CutoffPeriodic, 2.05, 1.0)
    i, j, r = svt.pair_distances(pos, box)
    k = int(np.argmin(np.abs(r - 1.0)))
    d = pos[i[k]] - pos[j[k]]
    d -= np.round(d / 2.05) * 2.05
    bad = np.array(pos); bad[i[k]] += d / r[k] * (1.0 - r[k] + 1e-4)      # the closest pair to the cutoff moved to r_c + 1e-4
    with pytest.raises(AssertionError, match="within 4 h r_c"):
        svt.truth(svt.force_energy(oracle, force), bad, box, r_c=1.0)
    cleared, rounds = svt.clear_shell(bad, box, 1.0, 8.0 * svt.H, np.random.default_rng(5))
    assert rounds >= 1 and len(svt.shell_pairs(cleared, box, 1.0, 8.0 * svt.H)[0]) == 0
    assert np.abs(cleared - bad).max() <= 0.01 * rounds + 1e-6


def _layout(tmp_path, struct, members):
    fmt = " ".join(["%zu"] * (len(members) + 1))
    args = ", ".join(["sizeof(%s)" % struct] + ["offsetof(%s, %s)" % (struct, m) for m in members])
    src = tmp_path / (struct + ".c")
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "snb.h"\nint main(){printf("%s\\n", %s);return 0;}\n' % (fmt, args))
    exe = tmp_path / struct
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    return [int(x) for x in subprocess.check_output([str(exe)]).split()]


def test_virial_batch_layout_matches_c_compiler(snb, tmp_path):
    B = snb.capi.SnbVirialBatch
    assert [f[0] for f in B._fields_] == BATCH
    assert _layout(tmp_path, "snb_virial_batch", BATCH) == [ctypes.sizeof(B)] + [getattr(B, m).offset for m in BATCH]


def test_entry_point_is_exported_and_listed(snb):
    capi = snb.capi
    assert "snb_evaluate_slice_virials" in capi.SYMBOLS
    assert ctypes.CDLL(capi.LIB_PATH).snb_evaluate_slice_virials is not None
    L = capi.lib()
    assert L.snb_evaluate_slice_virials(None, None) == capi.SNB_ERR_INVALID_ARGUMENT      # a null batch / handle is refused before anything else
    assert L.snb_evaluate_slice_virials(None, ctypes.byref(capi.SnbVirialBatch())) == capi.SNB_ERR_INVALID_ARGUMENT


def test_abi_version_is_still_8(snb):
    assert snb.capi.SNB_ABI_VERSION == 8
    assert snb.capi.lib().snb_abi_version() == 8


def test_numpy_helpers_against_written_out_loops(snb):
    ctxmod = importlib.import_module(snb.__name__ + ".context")
    K = snb.HipCalcSlicedNonbondedForceKernel
    rng = np.random.default_rng(11)
    rows = rng.normal(size=(4, 6, 2, 6))      # [F][S][2][6], S = 6: three subsets
    m = K.virialMatrix(rows)
    assert m.shape == (4, 6, 2, 3, 3)
    for f in range(4):
        for s in range(6):
            for t in range(2):
                for c, (a, b) in enumerate(svt.COMPONENTS):
                    assert m[f, s, t, a, b] == rows[f, s, t, c] and m[f, s, t, b, a] == rows[f, s, t, c]
    lam = rng.uniform(0.0, 1.0, (5, 6, 2))
    got = K.virialsAtStates(rows, lam)
    assert got.shape == (4, 5, 6)
    want = np.zeros((4, 5, 6))
    for f in range(4):
        for k in range(5):
            for s in range(6):
                for t in range(2):
                    want[f, k] += lam[k, s, t] * rows[f, s, t]
    assert np.abs(got - want).max() < 1e-13
    assert np.abs(K.virialsAtStates(rows[0], lam) - want[0]).max() < 1e-13      # (a single frame's rows)
    kin = rng.normal(size=6)
    p = K.pressureFromVirial(want[0, 0], 27.0, kin)
    for c in range(6):
        assert p[c] == (want[0, 0, c] + kin[c]) / 27.0
    assert np.array_equal(K.pressureFromVirial(want[0, 0], 27.0), want[0, 0] / 27.0)
    pm = K.pressureFromVirial(K.virialMatrix(want[0, 0]), 27.0, K.virialMatrix(kin))
    assert pm.shape == (3, 3) and np.array_equal(pm, K.virialMatrix(p))
    # 1 kJ/mol/nm^3 in bar: 1e3 J / N_A / 1e-27 m^3 / 1e5 Pa
    assert abs(ctxmod.KJ_PER_MOL_NM3_IN_BAR - 1e3 / 6.02214076e23 / 1e-27 / 1e5) < 1e-9
    assert "16.6053906717" in K.pressureFromVirial.__doc__ or "16.6053906717" in ctxmod.pressureFromVirial.__doc__
