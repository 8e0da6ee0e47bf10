"""The reciprocal-space census on the CPU: proves the instrument (tests/recip_systems.py) before the GPU is asked, with the oracle alone.
Every system builds and has a finite oracle; the oracle itself is checked off the cube (lattice shifts, cyclic axis permutations, F = -dE/dx
of the reciprocal part alone -- the probe on which the reference's own Reference PME fails when nx != nz, Quirk Q1); and the comparison flags
every planted defect while the unperturbed input flags nothing."""
import numpy as np
import pytest

import recip_systems as R
import shell_systems as S

DOUBLE = R.TOLS["double"]


@pytest.mark.parametrize("name", list(R.SYSTEMS))
def test_system_builds_and_the_oracle_is_finite(name):
    """Prints the reciprocal force scale, F_med and how much wider the total-scale allowance tol max(|F_total|, 1) is than the new one."""
    s = R.build(name)
    n = len(s["q"])
    assert np.array_equal(s["pos"], S.to_float(s["pos"])), "coordinates must be float32 values"
    assert s["lam"].shape == (s["nsub"] * (s["nsub"] + 1) // 2, 2) and (s["lam"] == 0).any() and (s["lam"][[R.sl(i, j) for i in range(s["nsub"]) for j in range(i)]] != 1).all()
    b = s["box"]
    assert len({b[0, 0], b[1, 1], b[2, 2]}) == 3 or name == "blob", "three unequal cell lengths"
    mesh = s["kmax"] if s["method"] == 3 else s["grid"]
    assert len(set(mesh)) == (2 if name == "long_z" else 3), mesh
    fr, er = R.oracle_eval(s)
    ft, et = R.oracle_eval(s, direct=True)
    assert np.isfinite(fr).all() and np.isfinite(er).all() and np.isfinite(ft).all() and np.isfinite(et).all()
    floor = R.force_floor(s, fr)
    assert floor > 1.0, floor
    ratio = np.maximum(np.linalg.norm(ft, axis=1), 1.0) / np.maximum(np.linalg.norm(fr, axis=1), floor)
    print("%s: %d atoms, |F_rec| median %.1f max %.1f, F_med %.1f, |F_total| median %.1f; total-scale allowance / reciprocal allowance: median %.1f x"
          % (name, n, np.median(np.linalg.norm(fr, axis=1)), np.linalg.norm(fr, axis=1).max(), floor, np.median(np.linalg.norm(ft, axis=1)), np.median(ratio)))
    rec = R.compare(s, fr, fr, DOUBLE)
    assert rec["ok"] and rec["max_err"] == 0.0
    assert (name in R.HOST_BUILT) == (not (R.gpu_builder_applies(s, 0.0) and R.gpu_builder_applies(s, 0.1))), "HOST_BUILT must follow the engine's rule"
    assert R.gpu_builder_applies(s, 0.0) == R.gpu_builder_applies(s, 0.1)
    if name == "subsets5":
        sub = s["subset"]
        assert (sub == 3).sum() == 0 and (sub == 4).sum() == 1 and (sub == 2).sum() > 1000 and (s["q"][sub == 2] == 0).all()
        for j in range(5):
            assert (er[R.sl(3, j)] == 0).all(), "slices of the empty subset"
    if name == "on_mesh":
        h = np.diagonal(b) / np.asarray(s["grid"])
        snapped = np.abs(s["pos"][::9] / h - np.round(s["pos"][::9] / h)).max()
        assert snapped < 1e-5, snapped
        for d in range(3):
            for k, v in zip(s["special"][6 * d:6 * d + 6], R.on_mesh_values(b[d, d])):
                x = s["pos"][k, d]
                assert x == float(np.float32(v)) and np.signbit(x) == np.signbit(v) and (x < b[d, d]), (k, d, x, v)
    if name == "unwrapped":
        w = np.floor(s["pos"] / np.diagonal(b))
        assert w.min() == -3 and w.max() == 3
    if name == "blob":
        assert (s["subset"] == 2).sum() <= 64 < (s["subset"] == 0).sum()          # (a few dozen gas atoms around thousands in the ball)


@pytest.mark.parametrize("name", ["ortho_ljpme_tiling", "triclinic_unequal_ljpme", "ortho_ewald"])
def test_oracle_is_invariant_under_lattice_shifts(name):
    """Atoms moved by up to +-3 lattice vectors: the reciprocal forces and slice energies stay, at the double bar."""
    s = R.build(name)
    f0, e0 = R.oracle_eval(s)
    t = dict(s)
    rng = np.random.default_rng(5)
    t["pos"] = np.ascontiguousarray(s["pos"] + rng.integers(-3, 4, s["pos"].shape).astype(float) @ s["box"])
    f1, e1 = R.oracle_eval(t)
    rec = R.compare(s, f1, f0, DOUBLE)
    ok, worst = R.compare_energies(e1, e0, DOUBLE)
    print(R.report(rec), "energies %.2e" % worst)
    assert rec["ok"] and ok, R.report(rec)
    assert rec["max_err"] < 1e-8 and worst < 1e-8          # (what the oracle gives is rounding: far under the bar the engine is held to)


@pytest.mark.parametrize("name", ["ortho_ljpme_tiling", "ortho_ljpme_fallback", "ortho_small", "ortho_ewald", "long_z"])
def test_oracle_is_equivariant_under_cyclic_axis_permutations(name):
    """Positions, cell and meshes permuted cyclically: forces permute, slice energies stay -- each length and each mesh size in each role."""
    s = R.build(name)
    f0, e0 = R.oracle_eval(s)
    for k in (1, 2):
        f1, e1 = R.oracle_eval(R.permuted(s, k))
        rec = R.compare(s, R.permuted_back(f1, k), f0, DOUBLE)
        ok, worst = R.compare_energies(e1, e0, DOUBLE)
        print(k, R.report(rec), "energies %.2e" % worst)
        assert rec["ok"] and ok, R.report(rec)
        assert rec["max_err"] < 1e-8 and worst < 1e-8


@pytest.mark.parametrize("name", ["ortho_ljpme_fallback", "triclinic_unequal_ljpme", "ortho_small", "ortho_ewald"])
def test_oracle_reciprocal_force_is_the_gradient_of_the_reciprocal_energy(name):
    """F = -dE/dx with E = sum lambda E_slice, reciprocal part alone, by central differences on a few atoms and all three axes, lambda != 1.
    (The reference's Reference PME misses this by 3.9e2 when nx != nz.)  h = 2e-5 nm: the truncation error F''' h^2 / 6 is 1e-7 of the force,
    the rounding of E (1e5 kJ/mol at 1e-16) / h about 1e-6 kJ/mol/nm -- both far inside 1e-5 F_med."""
    s = R.build(name)
    f0, _ = R.oracle_eval(s)
    floor = R.force_floor(s, f0)
    h = 2e-5
    rng = np.random.default_rng(9)
    worst = 0.0
    for a in rng.choice(len(s["q"]), 3, replace=False):
        for d in range(3):
            e = []
            for sign in (1, -1):
                t = dict(s); t["pos"] = s["pos"].copy(); t["pos"][a, d] += sign * h
                e.append(float((t["lam"] * R.oracle_eval(t)[1]).sum()))
            fd = -(e[0] - e[1]) / (2 * h)
            worst = max(worst, abs(fd - f0[a, d]) / max(np.linalg.norm(f0[a]), floor))
    print("%s: F + dE/dx worst %.2e of max(|F|, F_med = %.1f)" % (name, worst, floor))
    assert worst <= DOUBLE, worst


def _victim(s, fo):
    """An atom with a large charge away from the special ones: the atom of the planted defects."""
    return int(np.argsort(-np.abs(s["q"]))[3])


@pytest.mark.parametrize("name", ["ortho", "ortho_ljpme_tiling", "triclinic_unequal", "ortho_small", "long_z", "blob"])
def test_planted_defects_are_flagged(name):
    """The comparison fed the oracle against a perturbed oracle, at the single-precision bar: an atom whose charge never reached the mesh (its
    neighbours are flagged; the atom itself is left out), an atom one mesh cell off along the middle axis, an atom 1/16 cell off.  The
    unperturbed input flags nothing."""
    s = R.build(name)
    fo, eo = R.oracle_eval(s)
    tol = R.TOLS["single"]
    assert R.compare(s, fo.copy(), fo, tol)["flagged"] == []
    a = _victim(s, fo)
    t = dict(s); t["q"] = s["q"].copy(); t["q"][a] = 0.0
    f, _ = R.oracle_eval(t)
    rec = R.compare(s, f, fo, tol, leave_out=(a,))
    print("charge of atom %d absent: %d neighbours flagged, worst %.2e" % (a, len(rec["flagged"]), rec["max_err"]))
    assert len(rec["flagged"]) >= 3 and a not in rec["flagged"], R.report(rec)
    d = np.linalg.norm(S._min_image(s, s["pos"] - s["pos"][a]), axis=1)
    # its neighbours of its own subset (lambda = 1; a slice at lambda = 0 feels nothing) -- the field of a charge reaches far: many more are flagged
    near = np.where((d > 0) & (d < 0.45) & (s["subset"] == s["subset"][a]) & (s["q"] != 0))[0]
    assert len(near) >= 2 and set(int(k) for k in near) <= set(rec["flagged"]), ("its neighbours must be among the flagged", near)
    cell = s["box"][1] / s["grid"][1]          # one mesh cell along the middle axis
    for frac in (1.0, 1.0 / 16.0):
        t = dict(s); t["pos"] = s["pos"].copy(); t["pos"][a] += frac * cell
        f, _ = R.oracle_eval(t)
        rec = R.compare(s, f, fo, tol)
        own = np.linalg.norm(f[a] - fo[a])
        print("atom %d moved %.4f cell: its own reciprocal force moves by %.2f (allowance %.3f), %d atoms flagged" % (a, frac, own, tol * max(np.linalg.norm(fo[a]), rec["floor"]), len(rec["flagged"])))
        assert a in rec["flagged"], R.report(rec)
