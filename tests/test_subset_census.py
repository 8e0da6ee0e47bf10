"""The subset-count census on the CPU: proves the instrument (tests/subset_census.py) with the oracle alone, and the LDS arithmetic behind the
guard of snb_create (csrc/pme_sizes.h) with a stand-alone driver under ASan + UBSan.  The GPU part is tests/test_gpu_subset_census.py."""
import os
import subprocess

import numpy as np
import pytest

import recip_systems as R
import shell_systems as S
import subset_census as C

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("row", list(C.ROWS))
def test_row_builds_and_the_special_subsets_are_what_they_claim(row):
    s = C.build(row)
    n, method, dgrid, precs = C.ROWS[row]
    sub, q = s["subset"], s["q"]
    assert s["nsub"] == n and s["method"] == method and s["grid"] == R.ORTHO_GRID and s["dgrid"] == tuple(dgrid) and len(q) == 13608
    count = np.bincount(sub, minlength=n)
    print(row, count.tolist())
    u, e, o = C.uncharged(n), C.empty(n), C.single(n)
    assert len({u, e, o, 0, n - 3}) == 5
    assert count[e] == 0 and count[o] == 1 and count[u] > 500 and (q[sub == u] == 0).all() and (s["epsilon"][sub == u] != 0).all()
    # the slabs: those of recip_systems._slabs over nsub, the empty one's with n - 3, the last one's with 0, but for the one atom
    slab = R._slabs(s["pos"], 1, S.ORTHO_LENGTHS[1], n)
    want = np.where(slab == e, n - 3, np.where(slab == o, 0, slab))
    atom = int(np.where(sub == o)[0][0])
    assert want[atom] == 0 and (np.delete(sub, atom) == np.delete(want, atom)).all() and atom == int(np.where(want == 0)[0][100])
    assert q[atom] != 0
    live = C.live_subsets(s)
    assert live == [i for i in range(n) if i not in (u, e)] and all(count[i] > 500 for i in live if i != o)
    # the lambda table: every value its own, none 0 or 1, as stated
    lam = s["lam"]
    assert lam.shape == (n * (n + 1) // 2, 2) and len(np.unique(lam)) == lam.size and lam.min() >= 0.05 and lam.max() <= 0.95
    k = np.arange(len(lam)) + 1
    assert np.allclose(lam[:, 0], 0.05 + 0.9 * ((k * 0.6180339887) % 1.0), atol=1e-12) and np.allclose(lam[:, 1], 0.05 + 0.9 * ((k * 0.4142135623) % 1.0), atol=1e-12)
    assert np.abs(np.diff(np.sort(lam[:, 0]))).min() > 1e-4          # (far above the float rounding of a lambda)
    assert all(C.slice_pair(R.sl(i, j)) == (i, j) for i in range(n) for j in range(i + 1))
    fo, eo = R.oracle_eval(s)
    assert np.isfinite(fo).all() and np.isfinite(eo).all() and R.force_floor(s, fo) > 1.0
    assert all((eo[R.sl(e, j)] == 0).all() for j in range(n)), "slices of the empty subset"
    assert all(eo[R.sl(u, j), 0] == 0 for j in range(n)), "Coulomb slices of the uncharged subset"
    assert int(C.derivative_mask(s).sum()) == 6
    assert all(p in ("single", "mixed", "double") for p in precs)


@pytest.mark.parametrize("row", list(C.ROWS))
def test_energy_bar(row):
    """The mesh sums are positive on live subsets; the mesh term of the bar decides at most 5 % of a row's live off-diagonal slices and stays
    under 1 kJ/mol; the bar passes the oracle itself and fails the oracle's table with two rows swapped, in every precision of the row."""
    s = C.build(row)
    n = s["nsub"]
    _, eo = R.oracle_eval(s)
    m = C.mesh_sums(s, eo)
    rho = C.rho_min()
    assert 3.5e-3 < rho < 4.5e-3, rho
    scale, floor = C.energy_scale(s, eo, "single")
    for t in range(2 if s["method"] == 5 else 1):
        live = C.live_subsets(s, t)
        assert (m[live, t] > 0).all(), (t, m[:, t])
        # the cap counts the slices between slabs; the one-atom subset's slices (its spectrum is flat, |E| a few kJ/mol) are shown beside them
        slabs = [i for i in live if i != C.single(n)]
        off = [R.sl(i, j) for i in slabs for j in slabs if j < i]
        lone = [R.sl(C.single(n), j) for j in slabs]
        decided, decided_lone = int(floor[off, t].sum()), int(floor[lone, t].sum())
        print("%s term %d: rho_min %.3e, the mesh term decides %d of %d live off-diagonal slices, at most %.3f kJ/mol (and %d of the %d slices of the one-atom subset, at most %.3f); median |E| %.0f"
              % (row, t, rho, decided, len(off), R.TOLS["single"] * (scale[off, t] * floor[off, t]).max(), decided_lone, len(lone),
                 R.TOLS["single"] * (scale[lone, t] * floor[lone, t]).max(), np.median(np.abs(eo[off, t]))))
        assert decided <= 0.05 * len(off), (decided, len(off))
        assert R.TOLS["single"] * (scale[off, t] * floor[off, t]).max() <= 0.9 and decided_lone <= 1 and R.TOLS["single"] * (scale[lone, t] * floor[lone, t]).max() <= 0.02
        assert not floor[[k for k in range(len(eo)) if k not in off + lone], t].any(), "the mesh term applies to live off-diagonal slices alone"
    assert not C.energy_scale(s, eo, "double")[1].any() and (C.energy_scale(s, eo, "double")[0] == np.maximum(np.abs(eo), 1.0)).all()
    live = C.live_subsets(s)
    for prec in C.ROWS[row][3]:
        assert C.compare_energies(s, eo, eo, prec)[0]
        for a, b in ((live[1], live[2]), (live[-2], live[-3])):          # two rows (i, .) of the table exchanged: an index into it off by a subset
            se = eo.copy()
            for j in range(n):
                se[R.sl(a, j)], se[R.sl(b, j)] = eo[R.sl(b, j)].copy(), eo[R.sl(a, j)].copy()
            ok, worst, where, _ = C.compare_energies(s, se, eo, prec)
            assert not ok and worst > 10 * R.TOLS[prec], (a, b, worst, where)
        se = eo.copy(); se[R.sl(C.empty(n), 0), 0] = 1e-9
        assert not C.compare_energies(s, se, eo, prec)[0], "a slice of the empty subset that is not exactly 0"


def test_the_bar_changes_nothing_on_ortho():
    """On the slice that defines rho_min the mesh term equals |E| by construction; the oracle's threaded sums differ in their last bits between
    evaluations (a few ulps, 1e-15), so the mesh term takes over only above a margin of 1e-9.  Checked against two fresh evaluations, whichever
    one rho_min was taken from."""
    s = R.build("ortho")
    rho = C.rho_min()
    for k in range(2):          # (raw slice energies do not depend on the lambdas: another table is another entry of the oracle's cache)
        t = dict(s); t["lam"] = s["lam"] * (0.5 + 0.25 * k)
        _, eo = R.oracle_eval(t)
        m = C.mesh_sums(s, eo)[:, 0]
        ratio = max(rho * np.sqrt(m[i] * m[j]) / abs(eo[R.sl(i, j), 0]) for i in range(3) for j in range(i))
        assert abs(ratio - 1.0) < 1e-12 < C.MARGIN, ratio
        scale, floor = C.energy_scale(s, eo, "single")
        assert not floor.any() and (scale == np.maximum(np.abs(eo), 1.0)).all()


@pytest.mark.parametrize("row", ["n13", "n17", "n20"])
def test_a_lambda_taken_from_the_next_slice_is_flagged(row):
    """Sensitivity of the force comparison to the lambda table: for every slice among the subsets that hold a charged atom, the oracle is
    evaluated with that slice's Coulomb lambda replaced by the next slice's, and recip_systems.compare at the single bar must flag an atom.
    The one exemption is the diagonal of the single-atom subset, which carries no force at all."""
    s = C.build(row)
    n = s["nsub"]
    fo, _ = R.oracle_eval(s)
    live = C.live_subsets(s)
    tol = R.TOLS["single"]
    assert R.compare(s, fo.copy(), fo, tol)["flagged"] == []
    missed, weakest = [], np.inf
    slices = [R.sl(i, j) for i in live for j in live if j <= i]
    for k in slices:
        t = dict(s); t["lam"] = s["lam"].copy()
        t["lam"][k, 0] = s["lam"][(k + 1) % len(s["lam"]), 0]
        f, _ = R.oracle_eval(t)
        rec = R.compare(s, f, fo, tol)
        if rec["ok"]:
            missed.append(C.slice_pair(k))
        else:
            weakest = min(weakest, rec["max_err"])
    print("%s: %d of %d slices caught, missed %s; the weakest catch is %.1f bars" % (row, len(slices) - len(missed), len(slices), missed, weakest / tol))
    assert missed == [(C.single(n), C.single(n))], missed


# ---- the LDS arithmetic of the guard ---------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def sizes(tmp_path_factory):
    """tests/pme_sizes_check.cpp under ASan + UBSan: its sweep must pass; returns its rows {(nx, nsub, real bytes, budget KB): (NB, total)}."""
    exe = tmp_path_factory.mktemp("pme_sizes") / "pme_sizes_check"
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I", os.path.join(ROOT, "openmm-nonbonded-slicing_amd", "csrc"), os.path.join(ROOT, "tests", "pme_sizes_check.cpp"), "-o", str(exe)])
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.splitlines()[-1] == "OK", "pme_sizes_check exited with %d:\n%s" % (r.returncode, r.stderr[-4000:])
    rows = {}
    for line in r.stdout.splitlines():
        if line.startswith("row "):
            v = [int(x) for x in line.split()[1:]]
            rows[tuple(v[:4])] = (v[4], v[5])
    return rows


def test_sizes_sweep_is_clean_and_the_census_rows_get_their_columns(sizes):
    """nx in 20 .. 260 x 1 .. 64 subsets x both arithmetics (in the driver): NB in {1, 2, 4, 8}, the request equal to the kernel's own carve-up
    and within the device's LDS exactly when the guard accepts.  Here: the rows of the census get the columns per work-group they are there for,
    by the header and by the restatement the GPU test prints."""
    for (row, prec), nb in C.EXPECT_NB.items():
        n, method, dgrid, _ = C.ROWS[row]
        rb = 8 if prec == "double" else 4
        assert sizes[40, n, rb, C.CONV_LDS_KB][0] == nb, (row, prec, sizes[40, n, rb, C.CONV_LDS_KB])
        assert C.conv_lds(40, n, rb) == sizes[40, n, rb, C.CONV_LDS_KB]
        if method == 5:
            assert C.conv_lds(dgrid[0], n, rb) == sizes[dgrid[0], n, rb, C.CONV_LDS_KB]
    assert set(C.EXPECT_NB) == {c for c in C.CASES if c[0] != "n7"}
    for key, val in sizes.items():
        assert C.conv_lds(*key) == val, key
    assert sizes[40, 20, 4, 16][0] == 1 and sizes[40, 20, 4, 32][0] == 2 and sizes[40, 12, 4, 72][0] == 8 and sizes[40, 3, 4, 72][0] == 8
    assert all((54 * 25) % nb for nb in (4, 8)), "ny nzc = 1350 columns: every row at NB = 4 or 8 ends in a partial work-group (NB = 2 divides them)"
