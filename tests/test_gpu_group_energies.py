"""Per-group interaction energies over stored frames (-m gpu): snb_evaluate_group_energies (include/snb.h).

The atom-energy table of snb_evaluate_atom_energies summed over lists of atoms on the device, at the engine's current state and for every
frame of a batch.  Ground truth is the oracle: its raw slice energies through the sum rule for groups that are whole subsets, the
moved-group rule of tests/group_energy_truth.py for probe groups, the all-atom truth table of tests/atom_energy_truth.py at 60 atoms.
Frames, workload and the oracle cache are those of tests/test_gpu_frames.py (float32-representable coordinates, so that engines of every
precision and the oracle see identical inputs); tolerances are the project's TOLS and SAME_STEP under |got - want| / max(|want|, 1) per entry.
The 24k-atom box takes the GPU list builder, the bricks, the plane path and the side builds; 60 atoms take host lists and per-pair wrap."""
import ctypes
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import atom_energy_truth as aet
import bench
import group_energy_truth as gtruth
import parity_tools as pt
import systems
import test_gpu_frames as tgf
from test_gpu_atom_energies import SMALL, _context, _device_doubles, _small_force, small_truths      # noqa: F401 (small_truths: a fixture)

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOLS = tgf.TOLS
SAME_STEP = tgf.SAME_STEP      # two evaluations of the same frame on different lists
SAME_TABLE = 1e-9              # two sums over the same kind of table (test_device_output_equals_host_output of the atom-energy tests)
METHODS = {"rf": (2, 0), "pme": (4, 0), "ljpme": (5, 27)}
S4 = 10

_CACHE = {}


def _w24k():
    return tgf._w24k()


def _ip(a):
    return a.ctypes.data_as(ctypes.POINTER(ctypes.c_int32))


def _dp(a):
    return a.ctypes.data_as(ctypes.POINTER(ctypes.c_double))


def _engine(snb, name, prec, w=None, world=1, padding=0.1):
    m, dg = METHODS[name]
    return bench.Engine(snb, w if w is not None else _w24k(), m, 54, dg, prec, 0, 0, world, padding, 1 << 30)


def _subset_groups(w):
    return [np.flatnonzero(w["subset"] == s) for s in range(4)]


def _groups24(w):
    """Subsets first (rows 0..3), then: every atom (overlapping the others), an empty group, a group with an index listed twice, and runs
    of 7 user atoms covering all atoms (the last run is shorter) -- lists of all ~24000 atoms, ~22800, 960, 240, 40, 7, 3 and 0 atoms: both
    mappings of the group kernel, several chunks per long group, more than one work-group of short ones."""
    n = len(w["q"])
    groups = _subset_groups(w) + [np.arange(n), np.zeros(0, dtype=np.int64), np.array([5, n - 1, 5])]
    groups += [np.arange(a, min(a + 7, n)) for a in range(0, n, 7)]
    return groups


def _probe_groups(w):
    """7 consecutive blob atoms of subset 1, one water molecule, the 40-atom subset."""
    blob = np.flatnonzero(w["subset"] == 1); water = np.flatnonzero(w["subset"] == 0); small = np.flatnonzero(w["subset"] == 3)
    mid = len(blob) // 2
    assert len(small) == 40 and w["epsilon"][water[0]] > 0 and w["epsilon"][water[1]] == 0 and w["epsilon"][water[2]] == 0
    return [blob[mid:mid + 7], water[:3], small]


def _csr(snb, groups):
    return snb.HipCalcSlicedNonbondedForceKernel.groupsToCSR(groups)


def _grouped(snb, table, groups):
    return snb.HipCalcSlicedNonbondedForceKernel.groupAtomEnergies(table, groups)


def _call(eng, csr, nsub, frames=None, isd=False, boxes=None, dev_in=True, dev_out=False, direct=1, recip=1, expect=None, n_frames=None, out=True):
    """One snb_evaluate_group_energies call; frames None: positions == NULL (the engine's current state).  Returns [F][G][nsub][2] as a NumPy
    array (the output is pre-filled with NaN); with expect the status is asserted and returned."""
    import torch
    start, atoms = csr
    G = len(start) - 1
    b = eng.capi.SnbGroupBatch()
    b.n_groups = G; b.group_start = _ip(start); b.group_atoms = _ip(atoms if len(atoms) else np.zeros(1, dtype=np.int32))
    b.include_direct = direct; b.include_reciprocal = recip; b.is_double = int(isd); b.stride4 = 0
    keep = []
    F = 1 if frames is None else len(frames)
    if frames is not None:
        if dev_in:
            d = tgf._dev(frames, isd); keep.append(d)
            b.positions = d.data_ptr(); b.is_device = 1
        else:
            h = np.ascontiguousarray(frames, dtype=np.float64 if isd else np.float32); keep.append(h)
            b.positions = h.ctypes.data_as(ctypes.c_void_p); b.is_device = 0
    b.n_frames = F if n_frames is None else n_frames
    if boxes is not None:
        bx = np.ascontiguousarray(np.asarray(boxes, dtype=np.float64).reshape(-1, 9)); keep.append(bx)
        b.boxes = _dp(bx)
    if dev_out:
        rows = torch.full((max(F, 1), G, nsub, 2), float("nan"), dtype=torch.float64, device="cuda")
        b.group_energies = rows.data_ptr() if out else None; b.out_is_device = 1
    else:
        rows = np.full((max(F, 1), G, nsub, 2), np.nan)
        b.group_energies = rows.ctypes.data_as(ctypes.c_void_p) if out else None; b.out_is_device = 0
    status = eng.L.snb_evaluate_group_energies(eng.h, ctypes.byref(b))
    if expect is not None:
        assert status == expect, (status, expect, eng.L.snb_last_error(eng.h))
        return status
    eng.ok(status)
    if dev_out:
        eng.sync()
        rows = rows.cpu().numpy()
    return rows


def _table(eng, n, nsub):
    out = np.full((n, nsub, 2), np.nan)
    eng.ok(eng.L.snb_evaluate_atom_energies(eng.h, 1, 1, out.ctypes.data_as(ctypes.c_void_p), 0))
    return out


def _sum_rule_error(rows, so, nsub=4):
    """rows [nsub][nsub][2]: the groups that are the subsets.  sum_{i in I} A[i][J] = E[slice(I, J)], halved on the diagonal."""
    worst = 0.0
    for i in range(nsub):
        for j in range(nsub):
            worst = max(worst, aet.rel(rows[i][j] * (0.5 if i == j else 1.0), so[aet.slice_index(i, j)]))
    return worst


def _hand_loop(snb, eng, frames, isd, groups, boxes=None):
    """The loop a caller writes by hand: per frame snb_set_box, snb_set_positions, snb_rebuild_neighbors (unrelated coordinates),
    snb_evaluate_atom_energies with host output, groupAtomEnergies in numpy."""
    n = frames.shape[1]
    out = []
    for f in range(len(frames)):
        if boxes is not None:
            eng.ok(eng.L.snb_set_box(eng.h, _dp(np.ascontiguousarray(boxes[f], dtype=np.float64).reshape(9))))
        p = tgf._dev(frames[f], isd)
        eng.set_positions_device(p.data_ptr(), isd)
        eng.rebuild()
        out.append(_grouped(snb, _table(eng, n, 4), groups))
    return np.stack(out)


# ---- 1. the current state against the table ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("prec", ["single", "double"])
@pytest.mark.parametrize("name", ["rf", "pme", "ljpme"])
def test_current_state_equals_the_grouped_table(name, prec, snb):
    """positions == NULL: the group rows against snb_evaluate_atom_energies + groupAtomEnergies on the same engine and list.  Both sides sum
    the same kind of table: SAME_TABLE."""
    w = _w24k(); n = len(w["q"]); isd = prec == "double"
    groups = _groups24(w); csr = _csr(snb, groups)
    eng = _engine(snb, name, prec)
    pos = tgf._dev(w["pos"], isd)
    eng.set_positions_device(pos.data_ptr(), isd)
    got = _call(eng, csr, 4)
    assert got.shape == (1, len(groups), 4, 2) and np.isfinite(got).all()      # every entry written
    want = _grouped(snb, _table(eng, n, 4), groups)
    err = aet.rel(got[0], want)
    dev = _call(eng, csr, 4, dev_out=True)
    assert np.isfinite(dev).all()
    err_dev = aet.rel(dev[0], want)
    print("%s %s: group rows against the grouped table %.3e (device output %.3e)" % (name, prec, err, err_dev))
    assert not got[0][5].any()      # the empty group
    assert np.abs(got[0][:5]).max() > 1.0
    assert err < SAME_TABLE and err_dev < SAME_TABLE, (err, err_dev)
    eng.close()


# ---- 2. frames against the oracle -------------------------------------------------------------------------------------------------------
def _probe_truth(f, frames):
    key = ("probe", f)
    if key not in _CACHE:
        w = _w24k()
        _CACHE[key] = gtruth.truth(aet.workload_evaluator(tgf._at(w, frames[f]), 4, 54, 0), w["subset"], 4, _probe_groups(w))
    return _CACHE[key]


@pytest.mark.parametrize("prec", ["single", "mixed", "double"])
@pytest.mark.parametrize("name", ["rf", "pme", "ljpme"])
def test_frames_against_the_oracle(name, prec, snb):
    """F = 5: at every frame the four subset groups satisfy the sum rule against the oracle's slice energies of that frame; PME in single
    and double: three probe groups at the first and the last frame against the moved-group truth; device frames with host output, with
    device output, and host frames (pinned staging) against each other."""
    w = _w24k(); isd = prec == "double"; frames = tgf._frames(5)
    m, dg = METHODS[name]
    groups = _groups24(w) + _probe_groups(w); csr = _csr(snb, groups)
    eng = _engine(snb, name, prec)
    host = _call(eng, csr, 4, frames, isd)
    dev = _call(eng, csr, 4, frames, isd, dev_out=True)
    up = _call(eng, csr, 4, frames, isd, dev_in=False)
    for rows in (host, dev, up):
        assert rows.shape == (5, len(groups), 4, 2) and np.isfinite(rows).all()
    for f in range(5):
        _, so = tgf._oracle(m, dg, ("frame", f), frames[f])
        for what, rows in (("host", host), ("device", dev), ("uploaded", up)):
            err = _sum_rule_error(rows[f][:4], so)
            print("%s %s frame %d %s output: sum rule %.3e" % (name, prec, f, what, err))
            assert err < TOLS[prec], (f, what, err)
    if name == "pme" and prec != "mixed":
        for f in (0, 4):
            want = _probe_truth(f, frames)
            err = aet.rel(host[f][-3:], want)
            print("pme %s frame %d: probe groups %.3e" % (prec, f, err))
            assert err < TOLS[prec], (f, err)
    same = max(aet.rel(dev, host), aet.rel(up, host))
    print("%s %s: host output, device output and uploaded frames against each other: %.3e" % (name, prec, same))
    assert same < SAME_TABLE, same
    eng.close()


# ---- 3. the batch against the hand-written loop -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("prec", ["single", "mixed", "double"])
def test_batch_against_the_hand_written_loop(prec, snb):
    """PME, F = 5: the batch on one engine, the per-frame loop (snb_set_positions, snb_rebuild_neighbors, snb_evaluate_atom_energies with
    host output, numpy reduction) on a second one, every group row: SAME_STEP.  (Measured on an MI355X: 2.4e-12 single and mixed, 7.6e-13
    double -- the lists of the two paths order an atom's sums alike, and the group sums use no atomics.)"""
    w = _w24k(); isd = prec == "double"; frames = tgf._frames(5)
    groups = _groups24(w); csr = _csr(snb, groups)
    eng = _engine(snb, "pme", prec)
    got = _call(eng, csr, 4, frames, isd)
    other = _engine(snb, "pme", prec)
    want = _hand_loop(snb, other, frames, isd, groups)
    err = aet.rel(got, want)
    print("pme %s: batch against the hand-written loop %.3e" % (prec, err))
    assert err <= SAME_STEP[prec], err
    eng.close(); other.close()


# ---- 4. the pipeline --------------------------------------------------------------------------------------------------------------------
def _pipeline_case(snb):
    """A warm engine (three forces steps, two forced rebuilds), a constant-box batch of 8 with device output: rows and counter deltas."""
    w = _w24k(); frames = tgf._frames(8, seed=23)
    groups = _groups24(w); csr = _csr(snb, groups)
    eng = _engine(snb, "pme", "single")
    pos = tgf._dev(w["pos"], False)
    eng.set_positions_device(pos.data_ptr(), False)
    eng.execute(False); eng.rebuild(); eng.execute(False); eng.rebuild(); eng.execute(False); eng.sync()
    s0 = eng.stats(); f0 = tgf._fstats(eng)
    rows = _call(eng, csr, 4, frames, False, dev_out=True)
    s1 = eng.stats(); f1 = tgf._fstats(eng)
    rec = dict(batches=int(f1.n_batches - f0.n_batches), frames=int(f1.n_frames - f0.n_frames), beside=int(f1.n_built_beside - f0.n_built_beside),
               in_line=int(f1.n_built_in_line - f0.n_built_in_line), discarded=int(f1.n_side_discarded - f0.n_side_discarded),
               rebuilds=int(s1.n_rebuilds - s0.n_rebuilds), overruns=int(s1.n_list_overruns - s0.n_list_overruns), timed=int(s1.n_timed - s0.n_timed),
               last_batch_ms=float(f1.last_batch_ms))
    eng.close()
    return rows, rec


_IN_LINE_SCRIPT = r'''
import sys, json, importlib
sys.path[:0] = [ROOT, ROOT + "/tests", ROOT + "/oracle"]
import numpy as np
import torch
torch.cuda.init()      # (as the snb fixture of tests/conftest.py: torch creates its HIP context before the first engine)
import test_gpu_group_energies as T
snb = importlib.import_module("openmm-nonbonded-slicing_amd")
rows, rec = T._pipeline_case(snb)
np.save(sys.argv[1], rows)
print("RESULT " + json.dumps(rec))
'''


def test_the_pipeline_ran(snb, tmp_path):
    """All but the first frame -- and at most one discarded side build -- are built beside the previous frame's pass; the same batch under
    SNB_FRAMES_IN_LINE (a child process: the switches are read once per process) builds all 8 in line and gives the same rows."""
    rows, rec = _pipeline_case(snb)
    print("pipelined:", rec)
    assert np.isfinite(rows).all()
    assert rec["batches"] == 1 and rec["frames"] == 8
    assert rec["beside"] + rec["in_line"] == 8
    assert rec["in_line"] <= 2
    assert rec["overruns"] == 0
    assert rec["rebuilds"] >= 8      # frame steps count as rebuilds ...
    assert rec["timed"] == 0         # ... and never in the timers
    assert rec["last_batch_ms"] == 0.0      # device output: the call did not end in a synchronise
    e = dict(os.environ); e["SNB_FRAMES_IN_LINE"] = "1"
    out = str(tmp_path / "in_line.npy")
    r = subprocess.run([sys.executable, "-c", "ROOT = %r\n" % ROOT + _IN_LINE_SCRIPT, out], env=e, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    res = json.loads([l for l in r.stdout.splitlines() if l.startswith("RESULT ")][-1][7:])
    print("in line:", res)
    assert res["frames"] == 8 and res["in_line"] == 8 and res["beside"] == 0
    err = aet.rel(rows, np.load(out))
    print("pipelined against in-line rows: %.3e" % err)
    assert err <= SAME_STEP["single"], err


# ---- 5. per-frame boxes, triclinic ------------------------------------------------------------------------------------------------------
def test_frames_with_their_own_boxes(snb):
    """Box and coordinates scaled by 1, 1.005, 1.005, 0.995, 1 (double precision): the sum rule against the oracle on the scaled workload
    at every frame -- the background term uses the frame's volume -- and every box change built in line."""
    w = _w24k(); scales = [1.0, 1.005, 1.005, 0.995, 1.0]
    frames = np.stack([w["pos"] * s for s in scales])
    boxes = np.stack([bench.workload_box(w) * s for s in scales])
    csr = _csr(snb, _subset_groups(w))
    eng = _engine(snb, "pme", "double")
    before = tgf._fstats(eng).n_built_in_line
    rows = _call(eng, csr, 4, frames, True, boxes=boxes)
    assert np.isfinite(rows).all()
    for f, s in enumerate(scales):
        _, so = tgf._oracle(4, 0, ("scaled", s), frames[f], s)
        err = _sum_rule_error(rows[f], so)
        print("scale %.3f frame %d: sum rule %.3e" % (s, f, err))
        assert err < TOLS["double"], (f, err)
    changes = sum(1 for f in range(1, 5) if scales[f] != scales[f - 1])
    assert tgf._fstats(eng).n_built_in_line - before >= changes
    eng.close()


def _sheared():
    if "shear" not in _CACHE:
        w = pt.float_positions(bench.shear_workload(_w24k()))
        rng = np.random.default_rng(41)
        frames = np.stack([w["pos"], w["pos"] + 0.02 * rng.standard_normal(w["pos"].shape)]).astype(np.float32).astype(np.float64)
        so = [bench.oracle_eval(tgf._at(w, frames[f]), 4, 54, 0)[1] for f in range(2)]
        _CACHE["shear"] = (w, np.ascontiguousarray(frames), so)
    return _CACHE["shear"]


@pytest.mark.parametrize("prec", ["single", "double"])
def test_triclinic_frames(prec, snb):
    w, frames, so = _sheared(); isd = prec == "double"
    eng = _engine(snb, "pme", prec, w=w)
    rows = _call(eng, _csr(snb, _subset_groups(w)), 4, frames, isd)
    for f in range(2):
        err = _sum_rule_error(rows[f], so[f])
        print("triclinic %s frame %d: sum rule %.3e" % (prec, f, err))
        assert err < TOLS[prec], (f, err)
    eng.close()


# ---- 6. 60 atoms: host lists, per-pair wrap, through Python ------------------------------------------------------------------------------
def _small_frames(snb, oracle, method, groups):
    """Frame 0: the system's own coordinates; frames 1 and 2: seeded perturbations of 0.02 nm (float32-representable), with the moved-group
    truth of every group."""
    key = ("small", method)
    if key not in _CACHE:
        force, pos, box = _small_force(snb, method)
        rng = np.random.default_rng(43)
        moved = np.stack([pos + 0.02 * rng.standard_normal(pos.shape) for _ in range(2)]).astype(np.float32).astype(np.float64)
        frames = np.ascontiguousarray(np.concatenate([pos[None], moved]))
        sub = aet.force_subsets(force)
        _CACHE[key] = (frames, [gtruth.truth(aet.force_evaluator(oracle, force, frames[f], box), sub, 3, groups) for f in (1, 2)])
    return _CACHE[key]


@pytest.mark.parametrize("prec", ["double", "single"])
@pytest.mark.parametrize("method", list(SMALL))
def test_60_atoms_through_python(method, prec, snb, oracle, small_truths):
    groups = [list(range(a, min(a + 7, 60))) for a in range(0, 60, 7)]
    force, pos, box = _small_force(snb, method)
    ctx = _context(snb, force, pos, box, prec)
    want0 = _grouped(snb, small_truths(method), groups)      # the all-atom truth table, grouped
    got = ctx.getGroupEnergies(force, groups)
    assert got.shape == (len(groups), 3, 2)
    err = aet.rel(got, want0)
    print("%s %s: getGroupEnergies %.3e" % (method, prec, err))
    assert err < TOLS[prec], err
    frames, want12 = _small_frames(snb, oracle, method, groups)
    kern = ctx._kernelFor(force)
    rows = kern.computeGroupEnergiesForFrames(ctx, groups, frames if prec == "double" else frames.astype(np.float32))
    assert rows.shape == (3, len(groups), 3, 2) and np.isfinite(rows).all()
    for f, want in enumerate([want0] + want12):
        err = aet.rel(rows[f], want)
        print("%s %s frame %d: %.3e" % (method, prec, f, err))
        assert err < TOLS[prec], (f, err)
    assert kern.getStats().n_host_rebuilds > 0      # (the host lists: below the GPU builder's floor)
    st = kern.getFrameStats()
    assert st.n_batches == 1 and st.n_frames == 3 and st.n_built_in_line == 3 and st.n_built_beside == 0
    assert aet.rel(ctx.getGroupEnergies(force, groups), want0) < TOLS[prec]      # the context's own state is in place again


# ---- 7. contract: the call writes only its output ---------------------------------------------------------------------------------------
def test_batch_leaves_forces_outputs_energies_and_timers_alone(snb):
    """Mixed precision (bitwise reproducible forces).  A forces step, an energy step, a 3-frame batch in another box: afterwards
    snb_get_forces, a registered accumulate-mode force output, the slice-energy buffer (host copy and device buffer) and snb_stats.n_timed
    are what they were, bit for bit; the next execute rebuilds, and two forces steps equal those of a twin engine that never made the call
    and was told to rebuild: positions and box are the caller's again.  The same for the call with positions == NULL (no rebuild then)."""
    import torch
    w = _w24k(); n = len(w["q"]); s = 1.005
    frames = tgf._frames(3, seed=29) * s
    boxes = np.stack([bench.workload_box(w) * s] * 3)
    csr = _csr(snb, _groups24(w))
    g = torch.Generator(device="cuda").manual_seed(17)
    p1 = tgf._dev(w["pos"], False)
    p2 = p1 + 0.004 * torch.randn(p1.shape, generator=g, device="cuda")
    p3 = p2 + 0.004 * torch.randn(p1.shape, generator=g, device="cuda")
    A = _engine(snb, "pme", "mixed", padding=0.3); B = _engine(snb, "pme", "mixed", padding=0.3)
    outs = []
    for e in (A, B):
        out = torch.full((n, 3), 7.25, dtype=torch.float32, device="cuda")
        e.set_force_output(out.data_ptr(), False, 1)
        outs.append(out)
        e.set_positions_device(p1.data_ptr(), False); e.execute(False)                                  # forces step
        e.set_positions_device(p2.data_ptr(), False); e.ok(e.L.snb_execute(e.h, 0, 1, 1, 1, None))      # energy step
        e.sync()
    f_before = torch.zeros((n, 3), dtype=torch.float32, device="cuda"); A.forces_to(f_before.data_ptr(), False); A.sync()
    out_before = outs[0].clone()
    se_before = A.slice_energies(S4)
    dev = ctypes.c_void_p(); A.ok(A.L.snb_slice_energies_device(A.h, ctypes.byref(dev)))
    dev_before = _device_doubles(dev.value, 2 * S4).clone()
    timed_before = A.stats().n_timed

    def untouched():
        f_after = torch.zeros_like(f_before); A.forces_to(f_after.data_ptr(), False); A.sync()
        assert torch.equal(f_before, f_after)
        assert torch.equal(outs[0], out_before)
        assert np.array_equal(A.slice_energies(S4), se_before)
        assert torch.equal(_device_doubles(dev.value, 2 * S4), dev_before)
        assert A.stats().n_timed == timed_before

    now = _call(A, csr, 4)      # positions == NULL: the state of the energy step
    assert np.isfinite(now).all() and np.abs(now).max() > 1.0
    untouched()
    rows = _call(A, csr, 4, frames, False, boxes=boxes)
    assert np.isfinite(rows).all() and np.abs(rows).max() > 1.0
    untouched()
    B.rebuild()
    fa = torch.zeros_like(f_before); fb = torch.zeros_like(f_before)
    for k, p in enumerate((p3, p1)):
        r0 = A.stats().n_rebuilds
        for e, f in ((A, fa), (B, fb)):
            e.set_positions_device(p.data_ptr(), False); e.execute(False); e.forces_to(f.data_ptr(), False); e.sync()
        if k == 0:
            assert A.stats().n_rebuilds == r0 + 1      # the lists in memory belonged to the last frame
        assert torch.equal(fa, fb)
        assert torch.equal(outs[0], outs[1])
    A.close(); B.close()


# ---- 8. bound context -------------------------------------------------------------------------------------------------------------------
def test_bound_context(snb):
    """posq in a random context order: positions == NULL gives the unbound rows and leaves the binding's buffers alone; frames are refused."""
    import torch
    from test_gpu_context_binding import View
    w = _w24k(); csr = _csr(snb, _groups24(w))
    ref = _engine(snb, "pme", "single")
    pos = tgf._dev(w["pos"], False)
    ref.set_positions_device(pos.data_ptr(), False)
    want = _call(ref, csr, 4)
    ref.close()
    v = View(w["pos"], False, seed=23, n_derivs=2 * S4)
    eng = _engine(snb, "pme", "single")
    slots = np.arange(2 * S4, dtype=np.int32).reshape(S4, 2)
    b = v.binding(snb.capi, deriv_slot=slots)
    torch.cuda.synchronize()
    eng.ok(eng.L.snb_bind_context(eng.h, ctypes.byref(b)))
    posq0 = v.posq.clone()
    got = _call(eng, csr, 4)
    torch.cuda.synchronize()
    err = aet.rel(got, want)
    print("bound against unbound: %.3e" % err)
    assert np.isfinite(got).all() and err < TOLS["single"]
    assert torch.equal(v.posq, posq0) and torch.equal(v.buf, v.P) and torch.equal(v.ebuf, v.E0) and torch.equal(v.dbuf, v.D0)
    f0 = tgf._fstats(eng); r0 = eng.stats().n_rebuilds
    assert _call(eng, csr, 4, tgf._frames(5)[:2], False, expect=snb.capi.SNB_ERR_STATE) == snb.capi.SNB_ERR_STATE
    f1 = tgf._fstats(eng)
    assert (f1.n_batches, f1.n_frames) == (f0.n_batches, f0.n_frames) and eng.stats().n_rebuilds == r0
    assert torch.equal(v.buf, v.P) and torch.equal(v.ebuf, v.E0) and torch.equal(v.dbuf, v.D0)
    eng.close()


# ---- 9. status codes --------------------------------------------------------------------------------------------------------------------
def test_status_codes(snb, oracle):
    capi = snb.capi; INVALID = capi.SNB_ERR_INVALID_ARGUMENT
    w = _w24k(); n = len(w["q"]); frames = tgf._frames(5)
    eng = _engine(snb, "rf", "single")
    pos = tgf._dev(w["pos"], False)
    eng.set_positions_device(pos.data_ptr(), False)
    good = _csr(snb, [[0, 1, 2], [], [7, 8]])

    def state():
        f = tgf._fstats(eng)
        return (int(eng.stats().n_rebuilds), int(f.n_batches), int(f.n_frames), int(f.n_built_in_line), int(f.n_built_beside))
    before = state()
    assert eng.L.snb_evaluate_group_energies(eng.h, None) == INVALID
    assert eng.L.snb_evaluate_group_energies(None, ctypes.byref(capi.SnbGroupBatch())) == INVALID
    _call(eng, good, 4, frames, False, out=False, expect=INVALID)                                  # NULL group_energies
    b = capi.SnbGroupBatch(); b.n_frames = 1; b.n_groups = 3; b.include_direct = 1; b.include_reciprocal = 1
    sink = np.zeros((3, 4, 2)); b.group_energies = sink.ctypes.data_as(ctypes.c_void_p)
    b.group_atoms = _ip(good[1])
    assert eng.L.snb_evaluate_group_energies(eng.h, ctypes.byref(b)) == INVALID                     # NULL group_start
    b.group_start = _ip(good[0]); b.group_atoms = None
    assert eng.L.snb_evaluate_group_energies(eng.h, ctypes.byref(b)) == INVALID                     # NULL group_atoms
    b.group_atoms = _ip(good[1]); b.n_groups = 0
    assert eng.L.snb_evaluate_group_energies(eng.h, ctypes.byref(b)) == INVALID                     # n_groups < 1
    _call(eng, (np.array([1, 3, 3, 5], dtype=np.int32), good[1]), 4, frames, False, expect=INVALID)      # group_start not starting at 0
    _call(eng, (np.array([0, 3, 2, 5], dtype=np.int32), good[1]), 4, frames, False, expect=INVALID)      # ... decreasing
    for bad in (n, -1):
        _call(eng, _csr(snb, [[0, 1], [2], [3, bad, 4]]), 4, frames, False, expect=INVALID)          # an index outside [0, N)
        assert b"group 2" in eng.L.snb_last_error(eng.h), eng.L.snb_last_error(eng.h)
    _call(eng, good, 4, frames, False, direct=0, recip=0, expect=INVALID)                          # both include flags 0
    _call(eng, good, 4, frames, False, n_frames=-1, expect=INVALID)                                # negative n_frames
    _call(eng, good, 4, None, False, n_frames=2, expect=INVALID)                                   # positions == NULL with n_frames != 1
    boxes = np.stack([bench.workload_box(w)] * 5); boxes[3] = np.diag([1.9, 6.2145, 6.2145]).reshape(9)
    _call(eng, good, 4, frames, False, boxes=boxes, expect=capi.SNB_ERR_BOX_TOO_SMALL)
    assert b"frame 3" in eng.L.snb_last_error(eng.h)
    boxes[3] = bench.workload_box(w); boxes[3][1] = 0.1      # not in reduced form
    _call(eng, good, 4, frames, False, boxes=boxes, expect=INVALID)
    assert b"frame 3" in eng.L.snb_last_error(eng.h)
    assert _call(eng, good, 4, frames, False, n_frames=0, expect=capi.SNB_OK) == capi.SNB_OK       # n_frames == 0: no work
    assert state() == before      # nothing was enqueued
    rows = _call(eng, good, 4, frames[:2], False)      # and the engine serves the next call
    assert np.isfinite(rows).all() and not rows[:, 1].any()
    eng.close()
    sharded = _engine(snb, "pme", "single", world=2)
    sharded.set_positions_device(pos.data_ptr(), False)
    _call(sharded, good, 4, frames, False, expect=capi.SNB_ERR_UNSUPPORTED)
    _call(sharded, good, 4, None, False, expect=capi.SNB_ERR_UNSUPPORTED)
    sharded.close()
    # classic Ewald: the reciprocal sum is refused, direct-only works and reduces to the oracle's direct-space slice energies
    F = snb.SlicedNonbondedForce
    force, epos, box = systems.random_box(F, 1500, 3, F.Ewald, 2.6, 1.0, pme=(2.6283, 0, 0, 0))
    force.ewaldKmax = (11, 11, 11)
    ctx = _context(snb, force, epos, box, "double")
    esub = aet.force_subsets(force)
    egroups = [np.flatnonzero(esub == s) for s in range(3)]
    with pytest.raises(snb.OpenMMException):
        ctx.getGroupEnergies(force, egroups)
    with pytest.raises(snb.OpenMMException):
        ctx.getGroupEnergies(force, egroups, includeDirect=False)
    rows = ctx.getGroupEnergies(force, egroups, includeReciprocal=False)
    want = aet.force_evaluator(oracle, force, epos, box, include_reciprocal=False, kmax=(11, 11, 11))(esub, 3)
    err = _sum_rule_error(rows, want, 3)
    print("Ewald, direct only: sum rule %.3e" % err)
    assert err < TOLS["double"], err
    frames3 = np.stack([epos, epos])
    kern = ctx._kernelFor(force)
    with pytest.raises(snb.OpenMMException):
        kern.computeGroupEnergiesForFrames(ctx, egroups, frames3)
    both = kern.computeGroupEnergiesForFrames(ctx, egroups, frames3, includeReciprocal=False)
    assert both.shape == (2, 3, 3, 2)
    for f in range(2):
        assert _sum_rule_error(both[f], want, 3) < TOLS["double"], f
