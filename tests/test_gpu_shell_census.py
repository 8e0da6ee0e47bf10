"""The cutoff-shell census on the GPU (-m gpu): the HIP engine against the oracle on systems in which ONE lost, doubled or wrongly imaged pair
near the cutoff fails the ordinary per-atom comparison (tests/shell_systems.py; the instrument is proven on the CPU in tests/test_shell_census.py).
Every comparison uses the suite's bars (1e-3 single / mixed, 1e-5 double, max(|x|, 1) scaling), on every atom: the band around the cutoff is
empty by construction, so there is no allowance.  A failure is printed as pairs: atom, partner, distance, image."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import shell_systems as S

pytestmark = pytest.mark.gpu

NB_CAP_TILES = 768 // 32          # neighbor.hip NB_CAP / 32: tiles per published chunk
CASES = [(g, t, p) for g, t, precs in S.CENSUS for p in precs]


def _forces_ok(s, f, prec, what):
    fo, _ = S.oracle_eval(s)
    rec = S.compare(s, f, fo, S.TOLS[prec])
    print("%s %s %s: max %.2e median %.2e" % (rec["system"], prec, what, rec["max_err"], rec["median_err"]))
    assert rec["ok"], "%s, %s\n%s" % (what, prec, S.report(rec))


def _energies_ok(s, se, prec, what):
    _, so = S.oracle_eval(s)
    ok, worst = S.compare_energies(se, so, S.TOLS[prec])
    print("%s/%s %s %s: slice energies max %.2e" % (s["name"], s["topology"], prec, what, worst))
    assert ok, "%s, %s: slice energies off by %.2e\n%s\n%s" % (what, prec, worst, se, so)


@pytest.mark.parametrize("geometry,topology,prec", CASES, ids=["%s-%s-%s" % c for c in CASES])
def test_census(geometry, topology, prec, snb):
    """Every geometry x topology, without a skin and with one of 0.1 nm: an energy + forces + derivatives step (the raw slice energies are the
    dE/dlambda of every slice), four forces-only steps (with the skin the list lives ten steps: the second captures the step graph, the third and fourth replay it), an energy-only
    step; on the GPU builder wherever it applies, and through the chunked publication in the dense ball (asserted there from the tile and block
    counters; at the density of water a block gathers about 570 owned entries after the exact pruning, under the 736 at which a chunk is
    published, and the two counters cannot show the blocks that exceed it, so nothing is asserted on that system)."""
    s = S.build(geometry, topology)
    assert len(S.band_pairs(s)[0]) == 0
    for padding in (0.0, 0.1):
        eng = S.Engine(snb, s, prec, padding=padding, interval=10 if padding else 1)
        what = "padding %.1f" % padding
        f, se, e = eng.step_energy_forces()
        _forces_ok(s, f, prec, what + ", energy + forces step")
        _energies_ok(s, se, prec, what + ", energy + forces step")
        _, so = S.oracle_eval(s)
        # (the total the call returns is the sum of the slices, all lambdas being 1: held to the sum of the slices' own bars)
        assert abs(e - so.sum()) <= S.TOLS[prec] * np.maximum(np.abs(so), 1.0).sum(), (what, e, so.sum())
        for k in range(4):          # with a skin: the first runs eagerly (timed), the second captures the step graph, the third and fourth replay it
            _forces_ok(s, eng.step_forces(), prec, what + ", forces-only step %d" % k)
        _energies_ok(s, eng.step_energy_only(), prec, what + ", energy-only step")
        st = eng.stats()
        assert st.n_tiles > 0
        if geometry not in S.HOST_BUILT:
            assert st.n_host_rebuilds == 0, (what, int(st.n_host_rebuilds))
        else:
            assert st.n_host_rebuilds > 0 and st.n_host_rebuilds == st.n_rebuilds, (what, int(st.n_host_rebuilds), int(st.n_rebuilds))
        if geometry == "blob_in_gas":
            # more tiles per block, on average, than one chunk holds: blocks of the ball were published in several chunks
            print("%s %s: %d tiles in %d blocks, %.1f per block" % (s["name"], what, st.n_tiles, st.n_blocks, st.n_tiles / st.n_blocks))
            assert st.n_tiles > NB_CAP_TILES * st.n_blocks, (int(st.n_tiles), int(st.n_blocks))
        assert st.n_list_overruns == 0
        eng.close()


def _walk(snb, frames, prec, padding, interval, energy_steps=()):
    eng = S.Engine(snb, frames[0], prec, padding=padding, interval=interval)
    for k, f in enumerate(frames):
        eng.set_frame(f)
        if k in energy_steps:
            fr, se, _ = eng.step_energy_forces()
            _energies_ok(f, se, prec, "step %d" % k)
        else:
            fr = eng.step_forces()
        _forces_ok(f, fr, prec, "step %d of the walk (padding %.2f, interval %d)" % (k, padding, interval))
        st = eng.stats()
        assert st.n_list_overruns == 0 and st.n_host_rebuilds == 0, (k, int(st.n_list_overruns), int(st.n_host_rebuilds))
    rebuilds = int(st.n_rebuilds)
    eng.close()
    return rebuilds


_SIDE_SCRIPT = r'''
import sys, json, importlib
sys.path[:0] = [ROOT, ROOT + "/tests", ROOT + "/oracle"]
import numpy as np
import shell_systems as S
snb = importlib.import_module("openmm-nonbonded-slicing_amd")
prec = sys.argv[1]
s = S.build("lattice_dense", "long")
frames = S.trajectory(s, 34, 0.002, 31)
assert S.max_displacement(frames, 13) < 0.05          # a list serves ten steps and may be three steps old when it comes into use
eng = S.Engine(snb, s, prec, padding=0.1, interval=10)
out = {"steps": []}
for k, f in enumerate(frames):
    eng.set_frame(f)
    fr = eng.step_forces()
    fo, _ = S.oracle_eval(f)
    rec = S.compare(f, fr, fo, S.TOLS[prec])
    st = eng.stats()
    out["steps"].append({"ok": rec["ok"], "max_err": rec["max_err"], "report": S.report(rec), "overruns": int(st.n_list_overruns), "host": int(st.n_host_rebuilds)})
out["rebuilds"] = int(eng.stats().n_rebuilds)
eng.close()
print("RESULT " + json.dumps(out))
'''


@pytest.mark.parametrize("prec", ["single", "mixed"])
def test_list_life_fixed_interval_with_side_built_lists(prec):
    """Skin 0.1 nm, a rebuild every tenth step: from the third rebuild on the list is built beside the steps, from positions three executes old.
    Every step of the walk against the oracle (a child process: the engine reports its side builds on stderr under SNB_VERBOSE, which is read
    once per process)."""
    import re
    e = dict(os.environ); e["SNB_VERBOSE"] = "1"
    for k in ("SNB_SIDE_REBUILD", "SNB_SIDE_LEAD", "SNB_SIDE_REJECT"):
        e.pop(k, None)
    r = subprocess.run([sys.executable, "-c", "ROOT = %r\n" % S.ROOT + _SIDE_SCRIPT, prec], env=e, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    res = json.loads([l for l in r.stdout.splitlines() if l.startswith("RESULT ")][-1][7:])
    for k, st in enumerate(res["steps"]):
        assert st["ok"] and st["overruns"] == 0 and st["host"] == 0, (k, st["report"], st)
    m = re.search(r"rebuilds: (\d+), of them (\d+) built beside the steps; (\d+) side builds discarded", r.stderr)
    assert m, r.stderr[-1500:]
    assert res["rebuilds"] == 4 and int(m.group(2)) == 2 and int(m.group(3)) == 0, (res["rebuilds"], m.groups())      # steps 0, 10, 20, 30; the last two beside


def test_list_life_automatic_rebuilds(snb):
    """rebuild_interval = -200: the displacement watch decides.  A walk that forces several rebuilds, every step against the oracle."""
    s = S.build("lattice_dilute", "chains")
    frames = S.trajectory(s, 30, 0.004, 41)
    rebuilds = _walk(snb, frames, "single", 0.1, -200, energy_steps=(7, 22))
    assert 2 <= rebuilds < 30, rebuilds


@pytest.mark.parametrize("prec", ["single", "double"])
def test_list_life_box_rescale_sequence(prec, snb):
    """A barostat-like sequence: box and coordinates rescaled between steps of a walk, lists rebuilt every third step with a skin."""
    s = S.build("lattice_dense", "far14_periodic")
    scales = (1.0, 1.01, 1.01, 0.995, 0.995, 1.0, 1.004, 1.004)
    frames = S.trajectory(s, len(scales), 0.002, 51, scales=scales)
    _walk(snb, frames, prec, 0.05, 3, energy_steps=(0, 4))


@pytest.mark.parametrize("prec", ["single", "double"])
def test_list_life_atoms_cross_cell_faces(prec, snb):
    """A walk long enough that atoms cross the faces of the cell while one list is in use (skin 0.2 nm, a rebuild every 30th step): the image a
    tile was built with must follow the atom.  The dilute lattice: every partner is a far one."""
    s = dict(S.build("lattice_dilute", "none"))
    s["pos"] = S.to_float(s["pos"] - 0.229); s["name"] = "lattice_dilute_shifted"          # a lattice plane on every face of the cell
    frames = S.trajectory(s, 36, 0.003, 61)
    assert S.max_displacement(frames, 33) < 0.1
    L = s["box"][0, 0]
    crossed = (np.floor(frames[29]["pos"] / L) != np.floor(frames[0]["pos"] / L)).any(axis=1).sum()
    assert crossed >= 30, crossed
    rebuilds = _walk(snb, frames, prec, 0.2, 30, energy_steps=(29,))
    assert rebuilds == 2, rebuilds


@pytest.mark.parametrize("world", [2, 3])
@pytest.mark.parametrize("prec", ["single", "double"])
def test_sharded_partial_forces_sum_to_the_oracle(world, prec, snb):
    s = S.build("lattice_dense", "long")
    total = np.zeros_like(s["pos"]); etot = 0.0
    for rank in range(world):
        eng = S.Engine(snb, s, prec, padding=0.05, interval=1 << 30, rank=rank, world=world)
        f, se, _ = eng.step_energy_forces()
        total += f; etot = etot + se
        assert eng.stats().n_host_rebuilds == 0
        eng.close()
    _forces_ok(s, total, prec, "%d ranks" % world)
    _energies_ok(s, etot, prec, "%d ranks" % world)


def test_uneven_shard_blocks_with_an_empty_rank(snb):
    """snb_set_shard_blocks: i-block ranges (0, 0), (0, 5), (5, 16) of period 16 -- one rank owns nothing, one is re-ranged after its first step."""
    s = S.build("sparse_subsets", "long")
    total = np.zeros_like(s["pos"])
    for rank, (b, e) in enumerate([(0, 0), (0, 5), (5, 16)]):
        eng = S.Engine(snb, s, "single", padding=0.05, interval=1 << 30, rank=rank, world=3)
        if rank == 2:
            eng.step_forces()
        eng.set_shard_blocks(b, e, 16)
        total += eng.step_forces()
        if rank == 0:
            assert eng.stats().n_tiles == 0
        eng.close()
    _forces_ok(s, total, "single", "uneven block ranges")


@pytest.mark.parametrize("geometry", ["lattice_dense", "lattice_dilute", "small_box"])
@pytest.mark.parametrize("prec", ["single", "mixed", "double"])
def test_control_a_cutoff_shrunk_by_2e_4_flags_exactly_the_atoms_of_the_gap(geometry, prec, snb):
    """End-to-end control on the device: the engine is given rc - 2e-4, the oracle keeps rc.  The atoms over the bar must be exactly the atoms
    of the pairs between the two radii (predicted from the geometry; the band is empty around both radii): the census sees single pairs on
    hardware, and the engine is not altered to show it."""
    shrink = 2e-4
    s = S.build_control(geometry, shrink)
    assert len(S.band_pairs(s)[0]) == 0 and len(S.band_pairs(s, s["rc"] - shrink)[0]) == 0
    fo, _ = S.oracle_eval(s)
    atoms, gap = S.gap_atoms(s, fo, shrink, S.TOLS["single"])
    assert len(gap) >= (3 if geometry == "small_box" else 50)
    for padding in (0.0, 0.1):
        eng = S.Engine(snb, s, prec, padding=padding, interval=10, cutoff=s["rc"] - shrink)
        f = eng.step_forces()
        eng.close()
        rec = S.compare(s, f, fo, S.TOLS["single"])          # (the single-precision bar in every precision: the prediction is made for it)
        assert rec["flagged"] == atoms, "%d pairs in the gap, %d atoms predicted, %d flagged\n%s" % (len(gap), len(atoms), len(rec["flagged"]), S.report(rec))
        if prec == "double":
            # at the double bar a lost pair is worth hundreds of bars: nothing cancels, every atom of the gap is over it
            rec = S.compare(s, f, fo, S.TOLS["double"])
            assert rec["flagged"] == atoms, S.report(rec)
        # and with the right cutoff the same engine passes
    eng = S.Engine(snb, s, prec)
    _forces_ok(s, eng.step_forces(), prec, "control system at the full cutoff")
    eng.close()


@pytest.mark.parametrize("cell", ["cubic", "triclinic"])
@pytest.mark.parametrize("prec", ["single", "mixed", "double"])
def test_dimer_gas_against_the_closed_form(prec, cell, snb):
    """4096 isolated dimers (8192 atoms) in a 40 nm cell at separations rc (1 -+ delta), delta down to 2e-5 (single, mixed) and 1e-9 (double); bonds across
    every face, edge and corner.  Inside the cutoff the force is K q q / r^2 along the axis, outside exactly zero; the slice energies are the sums of K q q (1/r - 1/rc)
    over the inside dimers of each diagonal slice, and the total is their sum; no oracle involved.  With
    and without a skin, on the GPU builder and on the host builder."""
    d = S.dimer_gas(prec, None if cell == "cubic" else S.TRICLINIC * (40.0 / 6.0))
    assert len(S.dimer_images(d) - {(0, 0, 0)}) == 26
    failures = []
    for host in (0, 1):
        for padding in (0.0, 0.1):
            eng = S.Engine(snb, d, prec, padding=padding, interval=10 if padding else 1, host_build=host)
            what = "%s builder, padding %.1f" % ("host" if host else "GPU", padding)
            f, se, e = eng.step_energy_forces()
            ok, msg = S.compare_dimers(d, f, S.TOLS[prec])
            if not ok:
                failures.append("%s, energy + forces step: %s" % (what, msg))
            want = d["expected_slice_energies"]
            ok, worst = S.compare_energies(se, want, S.TOLS[prec])
            print("%s %s %s: slice energies max %.2e, total %.6f (closed form %.6f)" % (d["name"], prec, what, worst, e, want.sum()))
            if not ok:
                failures.append("%s: slice energies off by %.2e: %s, closed form %s" % (what, worst, se[:, 0], want[:, 0]))
            if not abs(e - want.sum()) <= S.TOLS[prec] * np.maximum(np.abs(want), 1.0).sum():
                failures.append("%s: total energy %r, closed form %r" % (what, e, want.sum()))
            ok, msg = S.compare_dimers(d, eng.step_forces(), S.TOLS[prec])
            if not ok:
                failures.append("%s, forces-only step: %s" % (what, msg))
            st = eng.stats()
            assert (st.n_host_rebuilds > 0) == bool(host), (what, int(st.n_host_rebuilds))
            eng.close()
    assert not failures, "\n".join(failures)
