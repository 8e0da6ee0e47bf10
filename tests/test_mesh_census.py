"""The mesh-size census on the CPU: the table of tests/mesh_census.py is legal, the oracle evaluates every row, and the rows between them name
every instantiation of the six (R1, R2) kernel families that the build holds -- read from the kernel names of the gfx950 code objects, so a
pair added to the FFT-pair or plane-pair list (csrc/pme_plan.h), or a new thread-count variant without a census row fails here, without a GPU.
The engine's planner (csrc/pme_plan.h) runs here too, as a stand-alone program: its splits are the rows' words, its decisions those of
mesh_census.plan().  The GPU leg (tests/test_gpu_mesh_census.py) asserts that the engine's own mesh line states each row's splits."""
import copy
import os
import subprocess

import numpy as np
import pytest

import mesh_census as M
import recip_systems as R
import shell_systems as S
from test_host_cpu import _device_kernel_notes

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("name", [r["name"] for r in M.ROWS])
def test_row_is_legal_and_the_oracle_is_finite(name, snb):
    row = M.by_name(name)
    L = snb.capi.lib()
    assert all(L.snb_legal_grid_size(n) == n for n in row["grid"]), row["grid"]
    assert row["nsub"] in (2, 5) and row["path"] in ("plane", "three-pass")
    fft, pl, kind = M.splits(row)
    for n, (a, b) in zip(row["grid"], fft + pl):          # a stated split is a factorisation of its axis (or 0 * 0)
        assert a * b in (0, n) and a <= b, (name, n, a, b)
    assert (kind == "none") == (pl[0][0] == 0 or pl[1][0] == 0)
    assert (kind == "static") <= (row["grid"][0] == row["grid"][1] and pl[0] == pl[1])
    nx, ny, nz = row["grid"]
    for prec in ("single", "double"):
        p = M.plan(row, prec)
        assert p["path"] == (row["path"] if prec == "single" else "three-pass"), (name, prec, p)
        if p["own"]:
            assert (nz // p["slabs"]) % 2 == 0 and nz // p["slabs"] >= 4
    s = M.system(row)
    assert len(s["q"]) == M.N_ATOMS and s["nsub"] == row["nsub"] and set(s["subset"]) == set(range(row["nsub"]))
    assert R.gpu_builder_applies(s, M.PADDING) and R.gpu_builder_applies(s, 0.0), "lists from the GPU builder: sort columns exist"
    f, e = R.oracle_eval(s)
    assert np.isfinite(f).all() and np.isfinite(e).all() and R.force_floor(s, f) > 1.0
    assert len(set(r["name"] for r in M.ROWS)) == len(M.ROWS)


def _library(snb):
    notes = _device_kernel_notes(snb)
    if notes is None:
        pytest.skip("ROCm binutils not installed")
    return M.library_keys(notes)


def test_rows_name_every_instantiation_of_the_build(snb):
    """keys of the rows + keys of UNREACHED == keys of the six families in the library, the two tables disjoint; the same for the thread-count
    variants (k_spreadMerge 256 / 512 per precision, k_convolveX<double, .., 256>, k_planeXY 768, k_fftZInvMix<A, B, 512> per z pair)."""
    lib_keys, lib_variants = _library(snb)
    assert len(lib_keys) > 150 and {k[0] for k in lib_keys} == {"k_spreadMerge", "k_fftZInvMix", "k_fftZ", "k_fftStrided", "k_convolveX", "k_planeXY"}
    missing, stale, overlap = M.completeness(M.ROWS, M.UNREACHED, lib_keys)
    assert not missing, ("instantiations without a census row", sorted(missing, key=str))
    assert not stale, ("the tables name kernels the build does not hold", sorted(stale, key=str))
    assert not overlap, sorted(overlap, key=str)
    for key, why in M.UNREACHED.items():
        assert len(why) == 3 and all(why), key
    _, variants = M.table_keys(M.ROWS)
    assert variants == lib_variants, (sorted(lib_variants - variants, key=str), sorted(variants - lib_variants, key=str))
    for need in (("k_spreadMerge", "float", 512), ("k_spreadMerge", "double", 512), ("k_convolveX", "double", 256), ("k_planeXY", None, 768), ("k_fftZInvMix", None, 256)):
        assert need in variants, need
    # the sixteen line lengths are those of the library's pairs, and every one has its wide inverse z kernel named
    pairs = {(k[2], k[3]) for k in lib_keys if k[0] == "k_fftZ" and k[2]}
    assert sorted(a * b for a, b in pairs) == list(M.SIZES)
    assert {v[1:3] for v in variants if len(v) == 4} == pairs
    # which rows the run-time plane kernel's radices come from: every radix first and second on x and on y, but for the listed roles
    # (the radices are not template arguments: they are taken from the rows' own words, which the GPU leg holds against the engine's)
    seen = {(axis, pos, M.splits(r)[1][axis][pos]) for r in M.ROWS for axis in (0, 1) for pos in (0, 1)
            if M.splits(r)[2] == "run-time" and M.plan(r, "single")["path"] == "plane"}
    for rdx in (5, 6, 7, 8, 9, 10, 12, 15, 16):
        for axis in (0, 1):
            for pos in (0, 1):
                if (axis, pos, rdx) == (1, 1, 5):
                    assert "radix 5 as second factor on y" in M.UNREACHED_ROLES and (axis, pos, rdx) not in seen
                else:
                    assert (axis, pos, rdx) in seen, ("run-time plane kernel: radix %d never %s on %s" % (rdx, ("first", "second")[pos], "xy"[axis]))
    for role, (_, _, _, shown_by) in M.UNREACHED_ROLES.items():
        r = M.by_name(shown_by)
        assert r["path"] == "three-pass" and not r["env"] and r["grid"][1] == 25


def test_completeness_check_reports_a_removed_row(snb):
    """Control: without the one row that holds the 16 * 16 z line on the plane path, exactly that row's own keys are reported missing."""
    lib_keys, lib_variants = _library(snb)
    rows = [copy.deepcopy(r) for r in M.ROWS if r["name"] != "Z256"]
    assert len(rows) == len(M.ROWS) - 1
    missing, stale, overlap = M.completeness(rows, M.UNREACHED, lib_keys)
    assert missing == {("k_spreadMerge", "float", 16, 16), ("k_spreadMerge", "double", 16, 16), ("k_fftZInvMix", 16, 16)}, sorted(missing, key=str)
    own, own_variants = M.table_keys([M.by_name("Z256")])
    assert missing <= own and not stale and not overlap
    _, variants = M.table_keys(rows)
    assert lib_variants - variants == {("k_fftZInvMix", 16, 16, 512)} and ("k_fftZInvMix", 16, 16, 512) in own_variants


# ---- the planner on the CPU ---------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def planner(tmp_path_factory):
    """tests/pme_plan_check.cpp (csrc/pme_plan.h, csrc/host_lists.h) under ASan + UBSan; the header alone first, with every warning an error and
    no HIP include path."""
    csrc = os.path.join(ROOT, "openmm-nonbonded-slicing_amd", "csrc")
    flags = ["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-I", csrc]
    tmp = tmp_path_factory.mktemp("pme_plan")
    alone = tmp / "header_alone.cpp"
    alone.write_text('#include "pme_plan.h"\n')
    subprocess.check_call(flags + ["-fsyntax-only", str(alone)])
    exe = tmp / "pme_plan_check"
    subprocess.check_call(flags + ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", os.path.join(ROOT, "tests", "pme_plan_check.cpp"), "-o", str(exe)])

    def run(row, prec):
        env = {k: v for k, v in os.environ.items() if not k.startswith("SNB_")}
        env.update(row["env"])
        args = [str(v) for v in row["grid"] + (row["nsub"], 8 if prec == "double" else 4) + tuple(S.ORTHO_LENGTHS) + (M.N_ATOMS, M.PADDING)]
        r = subprocess.run([str(exe)] + args, capture_output=True, text=True, env=env)
        assert r.returncode == 0 and not r.stderr, "pme_plan_check %s exited with %d:\n%s" % (" ".join(args), r.returncode, r.stderr[-4000:])
        return dict(line.split(" ", 1) for line in r.stdout.splitlines())
    return run


@pytest.mark.parametrize("name", [r["name"] for r in M.ROWS])
def test_planner_states_the_rows_splits_and_agrees_with_plan(name, planner):
    """The engine's planner, run on the CPU: the splits it prints are the row's own words (until now only the GPU leg saw the engine's), and
    everything else it decides -- sort columns, bricks, slabs, whether the own-atoms spreader runs, the fused z pass, the pipeline, the thread
    counts -- is what mesh_census.plan() restates."""
    row = M.by_name(name)
    for prec in ("single", "double"):
        got, want = planner(row, prec), M.plan(row, prec)
        assert got["fft"] == row["fft"] and got["plane"] == row["plane"], (name, prec, got)
        assert tuple(int(v) for v in got["cells"].split()) == want["cells"], (name, prec, got, want)
        assert bool(int(got["bricks"])) == want["bricks"] and got["group"] == ("1 1" if want["bricks"] else "0 0"), (name, prec, got, want)      # (columns of 5+ cells: one per brick)
        assert bool(int(got["own"])) == want["own"] and (int(got["slabs"]) if want["own"] else 0) == want["slabs"] and got["margin"] == "1", (name, prec, got, want)
        assert bool(int(got["fuse"])) == want["fuse"] and got["path"] == want["path"], (name, prec, got, want)
        for k in ("zmix_nt", "convx_nt", "plane_nt") + (("merge_nt",) if "merge_nt" in want else ()):
            assert int(got[k]) == want[k], (name, prec, k, got, want)
