"""Group-pair interaction energy matrix, direct space (-m gpu): snb_evaluate_group_pair_energies (include/snb.h).

Ground truth is the oracle alone (tests/group_pair_truth.py): every atom's subset replaced by its label, the unlabelled atoms in one extra
subset, the oracle's direct-only raw slice energies.  One oracle evaluation per (system, labelling), shared by the precision modes.
Coordinates are float32-representable, so that engines of every precision and the oracle see identical inputs.  Error rule: |got - want| /
max(|want|, 1) per entry; bars: the project's TOLS, SAME_STEP (two evaluations of one frame on different lists) and SAME_TABLE (two sums
over the same lists).  40 atoms take the host lists and the per-pair-wrap kernels; the 13824-atom lattice of the parity tests (the smallest
system of the suite the GPU list builder takes that carries exclusions and 1-4 exceptions) takes the image-coded tiles."""
import ctypes
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import atom_energy_truth as aet
import bench
import group_pair_truth as gpt
import shell_systems
import systems
import test_gpu_frames as tgf

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOLS = tgf.TOLS
SAME_STEP = tgf.SAME_STEP
SAME_TABLE = 1e-9
_CACHE = {}


def _f32(a):
    return np.ascontiguousarray(np.asarray(a).astype(np.float32).astype(np.float64))


def _ip(a):
    return a.ctypes.data_as(ctypes.POINTER(ctypes.c_int32))


def _context(snb, force, pos, box, prec):
    system = snb.System()
    for _ in range(force.getNumParticles()):
        system.addParticle(1.0)
    system.setDefaultPeriodicBoxVectors(*box)
    system.addForce(force)
    ctx = snb.Context(system, precision=prec, device=0)
    ctx.setPositions(pos)
    return ctx


def _call(capi, L, h, labels, G, frames=None, isd=False, boxes=None, dev_in=True, dev_out=False, stride4=False, expect=None, n_frames=None, out=True, null_labels=False):
    """One snb_evaluate_group_pair_energies call on the handle h; frames None: positions == NULL (the engine's current state).  Returns
    [F][P][2] as a NumPy array (the output is pre-filled with NaN); with expect the status is asserted and returned."""
    import torch
    lab = np.ascontiguousarray(labels, dtype=np.int32)
    P = gpt.num_pairs(max(G, 1)) if G <= 4096 else 1
    b = capi.SnbGroupPairBatch()
    b.n_groups = G; b.group_of_atom = None if null_labels else _ip(lab)
    b.is_double = int(isd); b.stride4 = int(stride4)
    keep = []
    F = 1 if frames is None else len(frames)
    if frames is not None:
        fr = np.asarray(frames)
        if stride4:
            fr = np.concatenate([fr, np.full(fr.shape[:2] + (1,), 7.5)], axis=2)      # (the fourth component is ignored)
        if dev_in:
            d = tgf._dev(fr, isd); keep.append(d)
            b.positions = d.data_ptr(); b.is_device = 1
        else:
            hbuf = np.ascontiguousarray(fr, dtype=np.float64 if isd else np.float32); keep.append(hbuf)
            b.positions = hbuf.ctypes.data_as(ctypes.c_void_p); b.is_device = 0
    b.n_frames = F if n_frames is None else n_frames
    if boxes is not None:
        bx = np.ascontiguousarray(np.asarray(boxes, dtype=np.float64).reshape(-1, 9)); keep.append(bx)
        b.boxes = bx.ctypes.data_as(ctypes.POINTER(ctypes.c_double))
    if dev_out:
        rows = torch.full((max(F, 1), P, 2), float("nan"), dtype=torch.float64, device="cuda")
        b.pair_energies = rows.data_ptr() if out else None; b.out_is_device = 1
    else:
        rows = np.full((max(F, 1), P, 2), np.nan)
        b.pair_energies = rows.ctypes.data_as(ctypes.c_void_p) if out else None; b.out_is_device = 0
    status = L.snb_evaluate_group_pair_energies(h, ctypes.byref(b))
    if expect is not None:
        assert status == expect, (status, expect, L.snb_last_error(h))
        return status
    assert status == 0, (status, L.snb_last_error(h))
    if dev_out:
        assert L.snb_synchronize(h) == 0
        rows = rows.cpu().numpy()
    return rows


def _kcall(snb, ctx, force, labels, G, **kw):
    """The same through a Python context's engine: its state (parameters, box, positions) is pushed first."""
    kern = ctx._kernelFor(force)
    if kw.get("frames") is None:
        kern._push_state(ctx)
    else:
        kern._push_frame_state(ctx)
    return _call(snb.capi, kern._lib, kern._h, labels, G, **kw)


# ---- 1. the 40-atom box: host lists, per-pair wrap ------------------------------------------------------------------------------------------
BOX40 = {"NoCutoff": (0, {}), "CutoffPeriodic": (2, {}), "CutoffPeriodic+switch": (2, dict(switch=True)), "Ewald": (3, dict(pme=(2.6283, 0, 0, 0))),
         "PME": (4, dict(pme=(2.6283, 20, 20, 20))), "LJPME": (5, dict(pme=(2.6283, 20, 20, 20), ljpme=(2.6283, 12, 12, 12)))}


def _box40(snb, name):
    F = snb.SlicedNonbondedForce
    m, kw = BOX40[name]
    force, pos, box = systems.random_box(F, 40, 3, m, 2.05, 1.0, **kw)
    if name == "Ewald":
        force.ewaldKmax = (5, 5, 5)
    return force, _f32(pos), box


def _labellings40():
    i = np.arange(40)
    return {"mod5": (i % 5, 5), "own": (i, 40), "one": (np.zeros(40, dtype=int), 1), "third_out": (np.where(i % 3 == 1, -1, i % 4), 4)}


def _truth40(snb, oracle, name, which):
    key = ("box40", name, which)
    if key not in _CACHE:
        force, pos, box = _box40(snb, name)
        kw = dict(kmax=(5, 5, 5)) if name == "Ewald" else {}
        lab, G = _labellings40()[which]
        _CACHE[key] = gpt.truth(gpt.direct_force_evaluator(oracle, force, pos, box, **kw), lab, G)
    return _CACHE[key]


@pytest.mark.parametrize("prec", ["single", "mixed", "double"])
@pytest.mark.parametrize("name", list(BOX40))
def test_40_atom_box(name, prec, snb, oracle):
    """Methods 0, 2 (with and without switch), 3 (classic Ewald: the call must WORK), 4, 5; labellings i % 5, every atom its own group (the
    matrix is the pair-energy table), one label for all, -1 on a third of the atoms."""
    force, pos, box = _box40(snb, name)
    ctx = _context(snb, force, pos, box, prec)
    K = snb.HipCalcSlicedNonbondedForceKernel
    for which, (lab, G) in _labellings40().items():
        want = _truth40(snb, oracle, name, which)
        got = ctx.getGroupPairEnergies(force, lab, numGroups=G)
        assert got.shape == (gpt.num_pairs(G), 2) and np.isfinite(got).all()
        err = aet.rel(got, want)
        print("%s %s %s: %.3e" % (name, prec, which, err))
        assert err < TOLS[prec], (which, err)
        assert np.abs(got).max() > 1.0
    # the frames method of the Python kernel: the same coordinates twice, float32 and float64, every list built in line on the host
    lab, G = _labellings40()["mod5"]
    kern = ctx._kernelFor(force)
    for frames in (np.stack([pos, pos]), np.stack([pos, pos]).astype(np.float32)):
        rows = kern.computeGroupPairEnergiesForFrames(ctx, lab, frames, numGroups=G)
        assert rows.shape == (2, 15, 2)
        assert max(aet.rel(rows[f], _truth40(snb, oracle, name, "mod5")) for f in range(2)) < TOLS[prec]
    assert kern.getFrameStats().n_frames == 4 and kern.getFrameStats().n_built_beside == 0
    own = K.groupPairMatrix(ctx.getGroupPairEnergies(force, np.arange(40), numGroups=40), 40)
    assert own.shape == (40, 40, 2) and not own[np.arange(40), np.arange(40)].any()      # (box > 2 cutoffs: no atom meets an image of itself)
    assert ctx._kernelFor(force).getStats().n_host_rebuilds > 0      # (the host lists: below the GPU builder's floor)


# ---- 2. the 13824-atom lattice: GPU lists, image-coded tiles -----------------------------------------------------------------------------
MEDIUM = {"PME": (4, dict(pme=(2.6283, 54, 54, 54))), "LJPME": (5, dict(pme=(2.6283, 54, 54, 54), ljpme=(2.6283, 24, 24, 24)))}
N_MED, L_MED = 13824, 6.0


def _medium(snb, name, n=N_MED, triclinic=False):
    F = snb.SlicedNonbondedForce
    m, kw = MEDIUM[name]
    force, pos, box = systems.random_box(F, n, 3, m, L_MED, 1.0, **kw)
    force.setUseDispersionCorrection(False)      # (the matrix never holds it; case (d) compares with the engine's own slice energies)
    if triclinic:
        pos = (pos / L_MED) @ shell_systems.TRICLINIC      # the jittered lattice, sheared with the cell
        box = shell_systems.TRICLINIC.copy()
    return force, _f32(pos), box


def _labellings_medium(n, subset):
    i = np.arange(n)
    runs = np.where((i // 180) % 2 == 0, i // 3, 100000 + i // 12)      # runs of 3 and of 12 consecutive user atoms: chains of 4 are cut by label borders
    _, runs = np.unique(runs, return_inverse=True)      # (2898 labels at 13824 atoms: 4.2 M rows)
    return {"runs": (runs, int(runs.max()) + 1), "mod37": (i % 37, 37), "one": (np.zeros(n, dtype=int), 1), "subsets": (np.asarray(subset), 3)}


def _truth_medium(snb, oracle, name, which, n=N_MED, triclinic=False, labels=None, pos=None, box=None, key=None):
    key = ("medium", name, which, n, triclinic) if key is None else key
    if key not in _CACHE:
        force, p0, b0 = _medium(snb, name, n, triclinic)
        lab, G = labels if labels is not None else _labellings_medium(n, aet.force_subsets(force))[which]
        _CACHE[key] = gpt.truth(gpt.direct_force_evaluator(oracle, force, p0 if pos is None else pos, b0 if box is None else box), lab, G)
    return _CACHE[key]


def _raw_direct_slices(ctx, force):
    """The engine's own raw slice energies of an energy-only snb_execute(0, 1, 1, 0)."""
    kern = ctx._kernelFor(force)
    kern._push_state(ctx)
    kern._check(kern._lib.snb_execute(kern._h, 0, 1, 1, 0, None))
    sl = np.zeros((kern.numSlices, 2))
    kern._check(kern._lib.snb_get_slice_energies(kern._h, sl.ctypes.data_as(ctypes.POINTER(ctypes.c_double))))
    return sl


@pytest.mark.parametrize("prec", ["single", "mixed", "double"])
@pytest.mark.parametrize("name", list(MEDIUM))
def test_gpu_lists_every_accumulation_path(name, prec, snb, oracle):
    """(a) runs of 3 and 12 consecutive atoms (exclusion and 1-4 pairs cross labels), (b) i % 37 (~32 distinct labels on both sides of every
    tile: the widest LDS block), (c) one label (the wave-uniform register path; the entry is the sum of all direct-only slice energies),
    (d) labels = subsets, against the oracle AND the engine's own raw slice energies."""
    force, pos, box = _medium(snb, name)
    subset = aet.force_subsets(force)
    ctx = _context(snb, force, pos, box, prec)
    results = {}
    for which, (lab, G) in _labellings_medium(N_MED, subset).items():
        want = _truth_medium(snb, oracle, name, which)
        got = ctx.getGroupPairEnergies(force, lab, numGroups=G)
        assert got.shape == (gpt.num_pairs(G), 2) and np.isfinite(got).all()
        err = aet.rel(got, want)
        print("%s %s %s: %.3e (largest |entry| %.3e)" % (name, prec, which, err, np.abs(want).max()))
        assert err < TOLS[prec], (which, err)
        results[which] = got
    direct = _truth_medium(snb, oracle, name, "subsets")
    err_one = aet.rel(results["one"][0], direct.sum(axis=0))
    own = _raw_direct_slices(ctx, force)
    err_own = aet.rel(results["subsets"], own)
    print("%s %s: one label against the summed slices %.3e; labels = subsets against the engine's own raw slice energies %.3e" % (name, prec, err_one, err_own))
    assert err_one < TOLS[prec] and err_own < TOLS[prec], (err_one, err_own)
    assert ctx._kernelFor(force).getStats().n_host_rebuilds == 0      # the image-coded tile path is what ran


@pytest.mark.parametrize("prec", ["single", "mixed", "double"])
@pytest.mark.parametrize("name", list(MEDIUM))
def test_atom_count_off_the_block_size_and_empty_groups(name, prec, snb, oracle):
    """(e) 13801 atoms (no multiple of 32: padding slots in the last block of every subset), labels 0, 2, 5 of G = 7 in use and a tenth of
    the atoms unlabelled: the rows of the empty groups are zeros."""
    n = 13801
    force, pos, box = _medium(snb, name, n)
    i = np.arange(n)
    lab = np.where(i % 10 == 9, -1, np.array([0, 2, 5])[(i // 5) % 3]); G = 7
    want = _truth_medium(snb, oracle, name, "sparse", n, labels=(lab, G))
    ctx = _context(snb, force, pos, box, prec)
    got = ctx.getGroupPairEnergies(force, lab, numGroups=G)
    err = aet.rel(got, want)
    print("13801 atoms %s %s: %.3e" % (name, prec, err))
    assert err < TOLS[prec], err
    used = {gpt.slice_index(a, b) for a in (0, 2, 5) for b in (0, 2, 5)}
    for k in range(gpt.num_pairs(G)):
        assert (k in used) == bool(got[k].any()), k
    assert ctx._kernelFor(force).getStats().n_host_rebuilds == 0


# ---- 3. triclinic ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("prec", ["single", "mixed", "double"])
def test_triclinic_cell(prec, snb, oracle):
    force, pos, box = _medium(snb, "PME", triclinic=True)
    lab, G = _labellings_medium(N_MED, aet.force_subsets(force))["runs"]
    want = _truth_medium(snb, oracle, "PME", "runs", triclinic=True)
    ctx = _context(snb, force, pos, box, prec)
    got = ctx.getGroupPairEnergies(force, lab, numGroups=G)
    err = aet.rel(got, want)
    print("triclinic %s: %.3e" % (prec, err))
    assert err < TOLS[prec], err
    assert ctx._kernelFor(force).getStats().n_host_rebuilds == 0


# ---- 4. frames -------------------------------------------------------------------------------------------------------------------------
SCALE3 = 1.00390625      # 1 + 2^-8: the scaled box edge 6.0234375 is a float32, as the coordinates are -- a single-precision engine and the oracle see the same cell


def _frames_medium(snb):
    """F = 4: the lattice, two seeded perturbations of 0.02 nm in the same box, a fourth in a box (and with coordinates) scaled by SCALE3."""
    if "frames" not in _CACHE:
        force, pos, box = _medium(snb, "PME")
        rng = np.random.default_rng(47)
        fr = [pos] + [pos + 0.02 * rng.standard_normal(pos.shape) for _ in range(3)]
        fr[3] = fr[3] * SCALE3
        _CACHE["frames"] = (_f32(np.stack(fr)), np.stack([box, box, box, box * SCALE3]))
    return _CACHE["frames"]


def _frames_case(snb, prec):
    """A context at frame 0, one evaluation of its own state (a first list), then the batch with device frames and host output: rows and
    the frame-counter deltas."""
    force, pos, box = _medium(snb, "PME")
    frames, boxes = _frames_medium(snb)
    lab, G = _labellings_medium(N_MED, aet.force_subsets(force))["mod37"]
    ctx = _context(snb, force, frames[0], box, prec)
    kern = ctx._kernelFor(force)
    first = ctx.getGroupPairEnergies(force, lab, numGroups=G)
    f0 = kern.getFrameStats(); s0 = kern.getStats()
    rows = _kcall(snb, ctx, force, lab, G, frames=frames, isd=prec == "double", boxes=boxes)
    f1 = kern.getFrameStats(); s1 = kern.getStats()
    rec = dict(batches=int(f1.n_batches - f0.n_batches), frames=int(f1.n_frames - f0.n_frames), beside=int(f1.n_built_beside - f0.n_built_beside),
               in_line=int(f1.n_built_in_line - f0.n_built_in_line), rebuilds=int(s1.n_rebuilds - s0.n_rebuilds), timed=int(s1.n_timed - s0.n_timed),
               host_rebuilds=int(s1.n_host_rebuilds))
    return ctx, force, (lab, G), first, rows, rec


_IN_LINE_SCRIPT = r'''
import sys, json, importlib
sys.path[:0] = [ROOT, ROOT + "/tests", ROOT + "/oracle"]
import numpy as np
import torch
torch.cuda.init()      # (as the snb fixture of tests/conftest.py: torch creates its HIP context before the first engine)
import test_gpu_group_pairs as T
snb = importlib.import_module("openmm-nonbonded-slicing_amd")
rows, rec = T._frames_case(snb, sys.argv[2])[4:]
np.save(sys.argv[1], rows)
print("RESULT " + json.dumps(rec))
'''


@pytest.mark.parametrize("prec", ["single", "mixed", "double"])
def test_frames(prec, snb, oracle, tmp_path):
    """Every frame against the oracle; the batch against four single positions == NULL evaluations; the run under SNB_FRAMES_IN_LINE (a
    child process: the switches are read once per process) against the default; the frame counters; device output against host output;
    float / double and stride-4 positions against each other."""
    isd = prec == "double"
    frames, boxes = _frames_medium(snb)
    ctx, force, (lab, G), first, rows, rec = _frames_case(snb, prec)
    print("default run:", rec)
    assert rows.shape == (4, gpt.num_pairs(G), 2) and np.isfinite(rows).all()
    assert rec["batches"] == 1 and rec["frames"] == 4 and rec["beside"] >= 1 and rec["beside"] + rec["in_line"] == 4
    assert rec["rebuilds"] >= 4 and rec["timed"] == 0 and rec["host_rebuilds"] == 0
    for f in range(4):
        want = _truth_medium(snb, oracle, "PME", "mod37", pos=frames[f], box=boxes[f], key=("frame", f))
        err = aet.rel(rows[f], want)
        print("frame %d %s: %.3e" % (f, prec, err))
        assert err < TOLS[prec], (f, err)
    assert aet.rel(rows[0], first) <= SAME_STEP[prec]
    # four single evaluations of the context's own state
    worst = 0.0
    for f in range(4):
        ctx.setPeriodicBoxVectors(*boxes[f]); ctx.setPositions(frames[f])
        ctx._kernelFor(force)._check(ctx._kernelFor(force)._lib.snb_rebuild_neighbors(ctx._kernelFor(force)._h))      # (unrelated coordinates)
        worst = max(worst, aet.rel(rows[f], ctx.getGroupPairEnergies(force, lab, numGroups=G)))
    print("batch against single evaluations %s: %.3e" % (prec, worst))
    assert worst <= SAME_STEP[prec], worst
    ctx.setPeriodicBoxVectors(*boxes[0]); ctx.setPositions(frames[0])
    # device output, the other coordinate type, stride-4 and host frames
    dev = _kcall(snb, ctx, force, lab, G, frames=frames, isd=isd, boxes=boxes, dev_out=True)
    err_dev = aet.rel(dev, rows)
    other = _kcall(snb, ctx, force, lab, G, frames=frames, isd=not isd, boxes=boxes)
    s4 = _kcall(snb, ctx, force, lab, G, frames=frames, isd=isd, boxes=boxes, stride4=True)
    up = _kcall(snb, ctx, force, lab, G, frames=frames, isd=isd, boxes=boxes, dev_in=False)
    err_in = max(aet.rel(other, rows), aet.rel(s4, rows), aet.rel(up, rows))
    print("%s: device against host output %.3e; float / double, stride-4 and host frames %.3e" % (prec, err_dev, err_in))
    assert err_dev < SAME_TABLE and err_in <= SAME_STEP[prec], (err_dev, err_in)
    # the same batch with every list built in line
    e = dict(os.environ); e["SNB_FRAMES_IN_LINE"] = "1"
    out = str(tmp_path / "in_line.npy")
    r = subprocess.run([sys.executable, "-c", "ROOT = %r\n" % ROOT + _IN_LINE_SCRIPT, out, prec], env=e, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    res = json.loads([l for l in r.stdout.splitlines() if l.startswith("RESULT ")][-1][7:])
    print("in line:", res)
    assert res["frames"] == 4 and res["in_line"] == 4 and res["beside"] == 0
    err = aet.rel(rows, np.load(out))
    print("pipelined against in-line rows %s: %.3e" % (prec, err))
    assert err <= SAME_STEP[prec], err


# ---- 5. the call writes only its output -------------------------------------------------------------------------------------------------
S4 = 10


def _labels24(w):
    n = len(w["q"])
    return np.where(np.arange(n) % 11 == 10, -1, w["subset"] * 2 + (np.arange(n) // 3) % 2).astype(np.int32), 8


def _engine24(snb, name="pme", prec="mixed", world=1, padding=0.1):
    m, dg = {"rf": (2, 0), "pme": (4, 0)}[name]
    return bench.Engine(snb, tgf._w24k(), m, 54, dg, prec, 0, 0, world, padding, 1 << 30)


def _truth24(f, frames):
    key = ("w24", f)
    if key not in _CACHE:
        w = tgf._w24k(); lab, G = _labels24(w)
        _CACHE[key] = gpt.truth(gpt.direct_workload_evaluator(tgf._at(w, frames[f]), 4, 54, 0), lab, G)
    return _CACHE[key]


def test_call_and_batch_leave_forces_outputs_and_energies_alone(snb):
    """Mixed precision (bitwise reproducible forces).  A forces step and an energy step; then a call with positions == NULL and a 3-frame
    batch: snb_get_forces, a registered accumulate-mode force output and the slice-energy buffer (host copy and device buffer) are bit for
    bit what they were, no timer counted; the next snb_execute rebuilds and still matches the oracle."""
    import torch
    from test_gpu_atom_energies import _device_doubles
    w = tgf._w24k(); n = len(w["q"]); lab, G = _labels24(w)
    frames = tgf._frames(3, seed=29)
    A = _engine24(snb)
    p1 = tgf._dev(w["pos"], False)
    g = torch.Generator(device="cuda").manual_seed(17)
    p2 = p1 + 0.004 * torch.randn(p1.shape, generator=g, device="cuda")
    out = torch.full((n, 3), 7.25, dtype=torch.float32, device="cuda")
    A.set_force_output(out.data_ptr(), False, 1)
    A.set_positions_device(p1.data_ptr(), False); A.execute(False)
    A.set_positions_device(p2.data_ptr(), False); A.ok(A.L.snb_execute(A.h, 0, 1, 1, 1, None))
    A.sync()
    f_before = torch.zeros((n, 3), dtype=torch.float32, device="cuda"); A.forces_to(f_before.data_ptr(), False); A.sync()
    out_before = out.clone()
    se_before = A.slice_energies(S4)
    dev = ctypes.c_void_p(); A.ok(A.L.snb_slice_energies_device(A.h, ctypes.byref(dev)))
    dev_before = _device_doubles(dev.value, 2 * S4).clone()
    timed_before = A.stats().n_timed

    def untouched():
        f_after = torch.zeros_like(f_before); A.forces_to(f_after.data_ptr(), False); A.sync()
        assert torch.equal(f_before, f_after)
        assert torch.equal(out, out_before)
        assert np.array_equal(A.slice_energies(S4), se_before)
        assert torch.equal(_device_doubles(dev.value, 2 * S4), dev_before)
        assert A.stats().n_timed == timed_before

    now = _call(snb.capi, A.L, A.h, lab, G)
    assert np.isfinite(now).all() and np.abs(now).max() > 1.0
    untouched()
    rows = _call(snb.capi, A.L, A.h, lab, G, frames=frames)
    assert np.isfinite(rows).all()
    err = max(aet.rel(rows[f], _truth24(f, frames)) for f in (0, 2))
    print("24k mixed, frames 0 and 2 against the oracle: %.3e" % err)
    assert err < TOLS["mixed"], err
    untouched()
    r0 = A.stats().n_rebuilds
    A.set_positions_device(p1.data_ptr(), False)
    A.ok(A.L.snb_execute(A.h, 0, 1, 1, 1, None))
    assert A.stats().n_rebuilds == r0 + 1      # the lists in memory belonged to the last frame
    _, so = tgf._oracle(4, 0, ("frame", 0), tgf._frames(5)[0])
    err = aet.rel(A.slice_energies(S4), so)
    print("the next energy step against the oracle: %.3e" % err)
    assert err < TOLS["mixed"], err
    A.close()


# ---- 6. bound context -------------------------------------------------------------------------------------------------------------------
def test_bound_context(snb):
    """posq in a random context order: positions == NULL gives the unbound matrix and leaves the binding's buffers alone; frames are refused."""
    import torch
    from test_gpu_context_binding import View
    w = tgf._w24k(); lab, G = _labels24(w)
    ref = _engine24(snb, prec="single", padding=0.1)
    pos = tgf._dev(w["pos"], False)
    ref.set_positions_device(pos.data_ptr(), False)
    want = _call(snb.capi, ref.L, ref.h, lab, G)
    ref.close()
    v = View(w["pos"], False, seed=23, n_derivs=2 * S4)
    eng = _engine24(snb, prec="single", padding=0.1)
    slots = np.arange(2 * S4, dtype=np.int32).reshape(S4, 2)
    b = v.binding(snb.capi, deriv_slot=slots)
    torch.cuda.synchronize()
    eng.ok(eng.L.snb_bind_context(eng.h, ctypes.byref(b)))
    posq0 = v.posq.clone()
    got = _call(snb.capi, eng.L, eng.h, lab, G)
    torch.cuda.synchronize()
    err = aet.rel(got, want)
    print("bound against unbound: %.3e" % err)
    assert np.isfinite(got).all() and err <= SAME_STEP["single"]
    assert torch.equal(v.posq, posq0) and torch.equal(v.buf, v.P) and torch.equal(v.ebuf, v.E0) and torch.equal(v.dbuf, v.D0)
    f0 = tgf._fstats(eng); r0 = eng.stats().n_rebuilds
    _call(snb.capi, eng.L, eng.h, lab, G, frames=tgf._frames(5)[:2], expect=snb.capi.SNB_ERR_STATE)
    f1 = tgf._fstats(eng)
    assert (f1.n_batches, f1.n_frames) == (f0.n_batches, f0.n_frames) and eng.stats().n_rebuilds == r0
    assert torch.equal(v.buf, v.P) and torch.equal(v.ebuf, v.E0) and torch.equal(v.dbuf, v.D0)
    eng.close()


# ---- 7. refusals ------------------------------------------------------------------------------------------------------------------------
def test_refusals(snb):
    capi = snb.capi; INVALID = capi.SNB_ERR_INVALID_ARGUMENT
    w = tgf._w24k(); n = len(w["q"]); frames = tgf._frames(5); lab, G = _labels24(w)
    eng = _engine24(snb, "rf", "single", padding=0.1)
    pos = tgf._dev(w["pos"], False)
    eng.set_positions_device(pos.data_ptr(), False)
    call = lambda *a, **kw: _call(capi, eng.L, eng.h, *a, **kw)
    before_rows = call(lab, G)

    def state():
        f = tgf._fstats(eng)
        return (int(eng.stats().n_rebuilds), int(f.n_batches), int(f.n_frames), int(f.n_built_in_line), int(f.n_built_beside))
    before = state()

    def intact():
        assert state() == before
        assert aet.rel(call(lab, G), before_rows) < SAME_TABLE      # a following evaluation equals the one before
        assert state() == before
    assert eng.L.snb_evaluate_group_pair_energies(eng.h, None) == INVALID                       # NULL batch
    assert eng.L.snb_evaluate_group_pair_energies(None, ctypes.byref(capi.SnbGroupPairBatch())) == INVALID      # NULL handle
    call(lab, G, frames=frames, null_labels=True, expect=INVALID)                                # NULL group_of_atom
    call(lab, G, frames=frames, out=False, expect=INVALID)                                       # NULL pair_energies
    intact()
    for bad_g in (0, -3, 4097):
        call(np.zeros(n, dtype=np.int32), bad_g, frames=frames, expect=INVALID)                  # n_groups outside 1 .. 4096
    intact()
    for atom, value in ((0, G), (n - 1, -2), (1234, 4096)):
        bad = lab.copy(); bad[atom] = value
        call(bad, G, frames=frames, expect=INVALID)                                              # a label outside [-1, G)
        assert ("atom %d:" % atom).encode() in eng.L.snb_last_error(eng.h), eng.L.snb_last_error(eng.h)
        call(bad, G, expect=INVALID)
    intact()
    call(lab, G, frames=frames, n_frames=-1, expect=INVALID)                                     # negative n_frames
    call(lab, G, n_frames=2, expect=INVALID)                                                     # positions == NULL with n_frames != 1
    intact()
    boxes = np.stack([bench.workload_box(w)] * 5); boxes[3] = np.diag([1.9, 6.2145, 6.2145]).reshape(9)
    call(lab, G, frames=frames, boxes=boxes, expect=capi.SNB_ERR_BOX_TOO_SMALL)
    assert b"frame 3" in eng.L.snb_last_error(eng.h)
    boxes[3] = bench.workload_box(w); boxes[3][1] = 0.1      # not in reduced form
    call(lab, G, frames=frames, boxes=boxes, expect=INVALID)
    assert b"frame 3" in eng.L.snb_last_error(eng.h)
    intact()
    assert call(lab, G, frames=frames, n_frames=0, expect=capi.SNB_OK) == capi.SNB_OK            # n_frames == 0: no work
    intact()
    rows = call(lab, G, frames=frames[:2])      # and the engine serves the next call
    assert np.isfinite(rows).all() and np.abs(rows).max() > 1.0
    eng.close()
    sharded = _engine24(snb, "pme", "single", world=2, padding=0.1)
    sharded.set_positions_device(pos.data_ptr(), False)
    _call(capi, sharded.L, sharded.h, lab, G, frames=frames, expect=capi.SNB_ERR_UNSUPPORTED)
    _call(capi, sharded.L, sharded.h, lab, G, expect=capi.SNB_ERR_UNSUPPORTED)
    sharded.close()
