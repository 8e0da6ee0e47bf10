"""Per-group forces over stored frames, by subset and at lambda states (-m gpu): snb_evaluate_group_forces (include/snb.h, DESIGN.md
section 4.12).

The force table of snb_evaluate_atom_forces summed over lists of atoms on the device, and contracted per atom with K lambda states, at the
engine's current state and for every frame of a batch.  Ground truth is the oracle (tests/group_force_truth.py): the one-hot truth table
summed per group for the raw rows, the oracle's plain forces at lambda_k summed per group for the states.  Frames, workload and the oracle
cache are those of tests/test_gpu_frames.py (float32-representable coordinates, so that engines of every precision and the oracle see
identical inputs).  The tolerance against the oracle is the per-atom criterion of tests/test_gpu_atom_forces.py carried to a group by the
triangle inequality:  ||got_g - want_g|| <= sum_{i in g} (TOLS[prec] max(||want_i||, 1) + allow_i)  per (group, column, term) and per
(group, state), allow_i the force of atom i's cutoff-band pairs at lambda = 1 of that frame (parity_tools.band_allowance; zero in double);
fewer than 1 % of a frame's atoms may carry one (checked on the CPU for the 0.02 nm frames in use: 178 to 196 of 23998 atoms).
The 24k-atom box takes the GPU list builder, the bricks, the plane path and the side builds; 60 atoms take host lists and per-pair wrap."""
import ctypes

import numpy as np
import pytest

import atom_force_truth as aft
import bench
import group_force_truth as gft
import parity_tools as pt
import test_gpu_frames as tgf
from test_gpu_atom_forces import SMALL, _context, _device_doubles, _small_force, small_truths      # noqa: F401 (small_truths: a fixture)

pytestmark = pytest.mark.gpu

TOLS = {"single": 1e-3, "double": 1e-5, "mixed": 1e-3}      # that of tests/test_gpu_atom_forces.py
SAME_STEP = tgf.SAME_STEP      # two evaluations of the same frame on different lists, per table entry
SAME_TABLE = 1e-9              # two sums over the same table
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
    """The four subsets (rows 0..3); every atom (~94 chunks); lists of exactly 32, 33, 256 and 257 atoms drawn from all atoms (both sides
    of the longest list one thread takes, and of one chunk); one list with five atoms of each subset; an empty list; a list with an index
    twice; runs of 7 user atoms covering all atoms (more than one work-group of short lists)."""
    n = len(w["q"])
    rng = np.random.default_rng(53)
    groups = _subset_groups(w) + [np.arange(n)]
    groups += [rng.choice(n, size=k, replace=False) for k in (32, 33, 256, 257)]
    groups += [np.concatenate([np.flatnonzero(w["subset"] == s)[:5] for s in range(4)]), np.zeros(0, dtype=np.int64), np.array([5, n - 1, 5])]
    groups += [np.arange(a, min(a + 7, n)) for a in range(0, n, 7)]
    return groups


EMPTY = 10      # index of the empty list in _groups24


def _states(w, K):
    """[K][S][2]: K = 3: all ones, the workload's own lambdas, a seeded random table in [0, 1]; K = 1: the workload's own."""
    own = np.asarray(w["lam"], dtype=np.float64)
    if K == 1:
        return np.ascontiguousarray(own[None])
    return np.ascontiguousarray(np.stack([np.ones_like(own), own, np.random.default_rng(59).uniform(0.0, 1.0, own.shape)]))


def _csr(snb, groups):
    return snb.HipCalcSlicedNonbondedForceKernel.groupsToCSR(groups)


def _call(eng, csr, nsub, frames=None, isd=False, boxes=None, dev_in=True, dev_out=False, direct=1, recip=1, expect=None, n_frames=None, rows=True,
          states=None, n_states=None, state_out=True):
    """One snb_evaluate_group_forces call; frames None: positions == NULL (the engine's current state).  Returns (rows [F][G][nsub][2][3] or
    None, state forces [F][K][G][3] or None) as NumPy arrays (the outputs are pre-filled with NaN); with expect the status is asserted and
    returned."""
    import torch
    start, atoms = csr
    G = len(start) - 1
    b = eng.capi.SnbGroupForceBatch()
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
    K = 0 if states is None else len(states)
    b.n_states = K if n_states is None else n_states
    if K:
        lam = np.ascontiguousarray(states, dtype=np.float64); keep.append(lam)
        b.state_lambdas = _dp(lam)
    b.out_is_device = int(dev_out)
    if dev_out:
        out = torch.full((max(F, 1), G, nsub, 2, 3), float("nan"), dtype=torch.float64, device="cuda")
        st = torch.full((max(F, 1), max(K, 1), G, 3), float("nan"), dtype=torch.float64, device="cuda")
        b.group_forces = out.data_ptr() if rows else None; b.state_forces = st.data_ptr() if (K and state_out) else None
    else:
        out = np.full((max(F, 1), G, nsub, 2, 3), np.nan); st = np.full((max(F, 1), max(K, 1), G, 3), np.nan)
        b.group_forces = out.ctypes.data_as(ctypes.c_void_p) if rows else None
        b.state_forces = st.ctypes.data_as(ctypes.c_void_p) if (K and state_out) else None
    status = eng.L.snb_evaluate_group_forces(eng.h, ctypes.byref(b))
    if expect is not None:
        assert status == expect, (status, expect, eng.L.snb_last_error(eng.h))
        _CACHE["last outputs"] = (out, st)
        return status
    eng.ok(status)
    if dev_out:
        eng.sync()
        out = out.cpu().numpy(); st = st.cpu().numpy()
    return (out if rows else None), (st if K else None)


def _table(eng, n, nsub):
    out = np.full((n, nsub, 2, 3), np.nan)
    eng.ok(eng.L.snb_evaluate_atom_forces(eng.h, 1, 1, out.ctypes.data_as(ctypes.c_void_p), 0))
    return out


def _numpy_outputs(snb, table, subset, groups, states):
    K = snb.HipCalcSlicedNonbondedForceKernel
    return K.groupAtomForces(table, groups), K.groupForcesAtStates(table, subset, groups, states)


def _sizes(groups):
    return np.array([len(g) for g in groups], dtype=np.float64)


def _worst_ratio(got, want, bound):
    """max ||got - want|| / bound over the entries (3-vectors); an entry whose bound is zero (the empty list) must be met exactly."""
    err = np.linalg.norm(np.asarray(got) - np.asarray(want), axis=-1)
    bound = np.broadcast_to(bound, err.shape)
    assert not err[bound == 0].any()
    return float((err[bound > 0] / bound[bound > 0]).max())


def _scaled_by_atoms(got, want, groups, per_entry):
    """The worst ||got - want|| / max(||want||, 1) per (group, ...) in units of per_entry x (atoms in the group): test 3's bound."""
    n = _sizes(groups)
    scale = np.maximum(np.linalg.norm(want, axis=-1), 1.0)
    shape = [1] * scale.ndim
    shape[list(scale.shape).index(len(groups))] = len(groups)
    return _worst_ratio(got, want, per_entry * n.reshape(shape) * scale)


# ---- 1. the current state against the table ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("prec", ["single", "double"])
@pytest.mark.parametrize("name", ["rf", "pme", "ljpme"])
def test_current_state_equals_the_grouped_table(name, prec, snb):
    """positions == NULL: rows and state forces against groupAtomForces and groupForcesAtStates of the engine's own
    snb_evaluate_atom_forces from the same state and list -- the sharp check of the reduction and of the contraction (the table itself is
    held to the oracle by tests/test_gpu_atom_forces.py).  Both sides sum the same kind of table: SAME_TABLE.  Device output the same; K = 3
    and K = 1."""
    w = _w24k(); n = len(w["q"]); isd = prec == "double"
    groups = _groups24(w); csr = _csr(snb, groups); states = _states(w, 3)
    assert len(groups[EMPTY]) == 0 and [len(g) for g in groups[5:9]] == [32, 33, 256, 257]
    eng = _engine(snb, name, prec)
    pos = tgf._dev(w["pos"], isd)
    eng.set_positions_device(pos.data_ptr(), isd)
    rows, st = _call(eng, csr, 4, states=states)
    assert rows.shape == (1, len(groups), 4, 2, 3) and st.shape == (1, 3, len(groups), 3)
    assert np.isfinite(rows).all() and np.isfinite(st).all()      # every entry written
    want_rows, want_st = _numpy_outputs(snb, _table(eng, n, 4), w["subset"], groups, states)
    drows, dst = _call(eng, csr, 4, states=states, dev_out=True)
    assert np.isfinite(drows).all() and np.isfinite(dst).all()
    _, st1 = _call(eng, csr, 4, rows=False, states=_states(w, 1))
    errs = dict(rows=gft.rel(rows[0], want_rows), states=gft.rel(st[0], want_st), rows_dev=gft.rel(drows[0], want_rows), states_dev=gft.rel(dst[0], want_st),
                one_state=gft.rel(st1[0][0], want_st[1]))
    print("%s %s: against the grouped table %s" % (name, prec, {k: "%.3e" % v for k, v in errs.items()}))
    assert not rows[0][EMPTY].any() and not st[0][:, EMPTY].any()      # the empty group
    assert np.abs(rows[0][:5]).max() > 1.0 and np.abs(st[0]).max() > 1.0
    assert max(errs.values()) < SAME_TABLE, errs
    eng.close()


# ---- 2. frames against the oracle -------------------------------------------------------------------------------------------------------
def _truth_rows(name, f, frames):
    """The one-hot truth table of frame f: per method, shared by the precisions."""
    key = ("table", name, f)
    if key not in _CACHE:
        m, dg = METHODS[name]; w = _w24k()
        _CACHE[key] = aft.truth_table(aft.workload_evaluator(tgf._at(w, frames[f]), m, 54, dg), w["subset"], 4)
    return _CACHE[key]


def _truth_forces(name, f, frames, states):
    """[K][N][3]: the oracle's plain forces of frame f at every state (the workload's own lambdas through the cache of test_gpu_frames)."""
    key = ("forces", name, f)
    if key not in _CACHE:
        m, dg = METHODS[name]; w = _w24k(); out = []
        for lam in states:
            if np.array_equal(lam, w["lam"]):
                out.append(tgf._oracle(m, dg, ("frame", f), frames[f])[0])
            else:
                v = tgf._at(w, frames[f]); v["lam"] = np.ascontiguousarray(lam)
                out.append(bench.oracle_eval(v, m, 54, dg)[0])
        _CACHE[key] = np.stack(out)
    return _CACHE[key]


def _allowance(name, f, frames, prec):
    """[N] force of an atom's cutoff-band pairs at lambda = 1 in frame f (zero in double precision); fewer than 1 % of the atoms carry one."""
    w = _w24k(); n = len(w["q"])
    if prec == "double":
        return np.zeros(n)
    key = ("band", name, f)
    if key not in _CACHE:
        m, dg = METHODS[name]
        v = tgf._at(w, frames[f]); v["lam"] = np.ones_like(w["lam"])
        _CACHE[key] = pt.band_allowance(v, m, 54, dg, pt.band_rel(v, "single"))[0]
    fa = _CACHE[key]
    assert (fa > 0).sum() < 0.01 * n, (f, int((fa > 0).sum()))
    return fa


def _bounds(per_atom_want, allow, groups, tol):
    """sum_{i in g} (tol max(||want_i||, 1) + allow_i) per group and per leading entry of want_i: [G] + want.shape[1:-1]."""
    norms = np.linalg.norm(per_atom_want, axis=-1)
    per_atom = tol * np.maximum(norms, 1.0) + allow.reshape((-1,) + (1,) * (norms.ndim - 1))
    return gft.group_sum(per_atom, groups)


@pytest.mark.parametrize("prec", ["single", "mixed", "double"])
@pytest.mark.parametrize("name", ["rf", "pme", "ljpme"])
def test_frames_against_the_oracle(name, prec, snb):
    """F = 4, K = 3, device frames, host output: the state forces of every frame against the oracle's forces at each state summed per
    group; the raw rows of the first and the last frame against the summed one-hot truth table; at least one list built beside a pass."""
    w = _w24k(); isd = prec == "double"; frames = tgf._frames(4)
    groups = _groups24(w); csr = _csr(snb, groups); states = _states(w, 3)
    eng = _engine(snb, name, prec)
    before = tgf._fstats(eng)
    rows, st = _call(eng, csr, 4, frames, isd, states=states)
    after = tgf._fstats(eng)
    assert rows.shape == (4, len(groups), 4, 2, 3) and st.shape == (4, 3, len(groups), 3)
    assert np.isfinite(rows).all() and np.isfinite(st).all()
    assert after.n_batches - before.n_batches == 1 and after.n_frames - before.n_frames == 4
    assert after.n_built_beside - before.n_built_beside >= 1
    for f in range(4):
        fa = _allowance(name, f, frames, prec)
        fo = _truth_forces(name, f, frames, states)
        for k in range(3):
            ratio = _worst_ratio(st[f][k], gft.state_truth(fo[k], groups), _bounds(fo[k], fa, groups, TOLS[prec]))
            print("%s %s frame %d state %d: worst error / bound %.3e" % (name, prec, f, k, ratio))
            assert ratio <= 1.0, (f, k, ratio)
        if f in (0, 3):
            table = _truth_rows(name, f, frames)
            ratio = _worst_ratio(rows[f], gft.rows_truth(table, groups), _bounds(table, fa, groups, TOLS[prec]))
            print("%s %s frame %d rows: worst error / bound %.3e" % (name, prec, f, ratio))
            assert ratio <= 1.0, (f, ratio)
    assert not rows[:, EMPTY].any() and not st[:, :, EMPTY].any()
    eng.close()


# ---- 3. the batch against the hand-written loop -----------------------------------------------------------------------------------------
def _hand_loop(snb, eng, frames, isd, groups, states, boxes=None):
    """The loop a caller writes by hand: per frame snb_set_box, snb_set_positions, snb_rebuild_neighbors (unrelated coordinates),
    snb_evaluate_atom_forces with host output, groupAtomForces and groupForcesAtStates in NumPy."""
    w = _w24k(); n = frames.shape[1]
    rows, st = [], []
    for f in range(len(frames)):
        if boxes is not None:
            eng.ok(eng.L.snb_set_box(eng.h, _dp(np.ascontiguousarray(boxes[f], dtype=np.float64).reshape(9))))
        p = tgf._dev(frames[f], isd)
        eng.set_positions_device(p.data_ptr(), isd)
        eng.rebuild()
        r, s = _numpy_outputs(snb, _table(eng, n, 4), w["subset"], groups, states)
        rows.append(r); st.append(s)
    return np.stack(rows), np.stack(st)


@pytest.mark.parametrize("prec", ["single", "mixed", "double"])
def test_batch_against_the_hand_written_loop(prec, snb):
    """PME, F = 4, K = 3: the batch on one engine, the per-frame loop on a second one.  Two lists order an entry's sums differently
    (SAME_STEP per table entry), and a group adds as many such entries as it has atoms: SAME_STEP[prec] x (atoms in the group) under
    ||got - want|| / max(||want||, 1).  The measured worst ratio to that bound is printed.  (On an MI355X: rows 3.3e-6 single and mixed,
    0.44 double -- the 40-atom subset's own column, the same figure on every run: other image offsets under close pairs; states 2.6e-8
    and 2.6e-3.)"""
    w = _w24k(); isd = prec == "double"; frames = tgf._frames(4)
    groups = _groups24(w); csr = _csr(snb, groups); states = _states(w, 3)
    eng = _engine(snb, "pme", prec)
    rows, st = _call(eng, csr, 4, frames, isd, states=states)
    other = _engine(snb, "pme", prec)
    want_rows, want_st = _hand_loop(snb, other, frames, isd, groups, states)
    r_rows = _scaled_by_atoms(rows, want_rows, groups, SAME_STEP[prec])
    r_st = _scaled_by_atoms(st, want_st, groups, SAME_STEP[prec])
    print("pme %s: batch against the hand-written loop, worst error / (SAME_STEP x atoms): rows %.3e, states %.3e" % (prec, r_rows, r_st))
    assert r_rows <= 1.0 and r_st <= 1.0, (r_rows, r_st)
    eng.close(); other.close()


# ---- 4. input and output variants -------------------------------------------------------------------------------------------------------
def test_host_frames_and_states_only(snb):
    """Single precision, F = 4: frames uploaded from the host (pinned staging) and a call with group_forces == NULL (states only, K = 1 and
    K = 3, device output) against the batch of device frames with both outputs: the bound of the hand-written loop."""
    w = _w24k(); frames = tgf._frames(4)
    groups = _groups24(w); csr = _csr(snb, groups); states = _states(w, 3)
    eng = _engine(snb, "pme", "single")
    rows, st = _call(eng, csr, 4, frames, False, states=states)
    up_rows, up_st = _call(eng, csr, 4, frames, False, states=states, dev_in=False)
    none, only = _call(eng, csr, 4, frames, False, states=states, rows=False, dev_out=True)
    _, only1 = _call(eng, csr, 4, frames, False, states=_states(w, 1), rows=False)
    plain, no_states = _call(eng, csr, 4, frames, False)      # K = 0: the rows alone
    assert none is None and no_states is None and np.isfinite(only).all() and np.isfinite(only1).all() and only1.shape == (4, 1, len(groups), 3)
    ratios = dict(uploaded_rows=_scaled_by_atoms(up_rows, rows, groups, SAME_STEP["single"]), uploaded_states=_scaled_by_atoms(up_st, st, groups, SAME_STEP["single"]),
                  states_only=_scaled_by_atoms(only, st, groups, SAME_STEP["single"]), one_state=_scaled_by_atoms(only1[:, 0], st[:, 1], groups, SAME_STEP["single"]),
                  rows_only=_scaled_by_atoms(plain, rows, groups, SAME_STEP["single"]))
    print("variants, worst error / (SAME_STEP x atoms): %s" % {k: "%.3e" % v for k, v in ratios.items()})
    assert max(ratios.values()) <= 1.0, ratios
    eng.close()


def test_frames_with_their_own_boxes(snb):
    """Box and coordinates scaled by 1, 1.005, 1.005, 0.995 (double precision, the workload's own lambdas as the one state): the state
    forces against the oracle on the scaled workload at every frame, and every box change built in line."""
    w = _w24k(); scales = [1.0, 1.005, 1.005, 0.995]
    frames = np.stack([w["pos"] * s for s in scales])
    boxes = np.stack([bench.workload_box(w) * s for s in scales])
    groups = _groups24(w); csr = _csr(snb, groups)
    eng = _engine(snb, "pme", "double")
    before = tgf._fstats(eng).n_built_in_line
    rows, st = _call(eng, csr, 4, frames, True, boxes=boxes, states=_states(w, 1))
    assert np.isfinite(rows).all() and np.isfinite(st).all()
    zero = np.zeros(len(w["q"]))
    for f, s in enumerate(scales):
        fo, _ = tgf._oracle(4, 0, ("scaled", s), frames[f], s)
        ratio = _worst_ratio(st[f][0], gft.state_truth(fo, groups), _bounds(fo, zero, groups, TOLS["double"]))
        print("scale %.3f frame %d: worst error / bound %.3e" % (s, f, ratio))
        assert ratio <= 1.0, (f, ratio)
    changes = sum(1 for f in range(1, 4) if scales[f] != scales[f - 1])
    assert tgf._fstats(eng).n_built_in_line - before >= changes
    eng.close()


def test_triclinic_frames(snb):
    """The sheared 24k box, two frames, double precision: the state forces (all ones, the workload's own lambdas) against the oracle."""
    w = pt.float_positions(bench.shear_workload(_w24k()))
    rng = np.random.default_rng(41)
    frames = np.ascontiguousarray(np.stack([w["pos"], w["pos"] + 0.02 * rng.standard_normal(w["pos"].shape)]).astype(np.float32).astype(np.float64))
    groups = _groups24(w); csr = _csr(snb, groups); states = _states(w, 3)[:2]
    eng = _engine(snb, "pme", "double", w=w)
    rows, st = _call(eng, csr, 4, frames, True, states=states)
    zero = np.zeros(len(w["q"]))
    for f in range(2):
        for k in range(2):
            v = tgf._at(w, frames[f]); v["lam"] = np.ascontiguousarray(states[k])
            fo = bench.oracle_eval(v, 4, 54, 0)[0]
            ratio = _worst_ratio(st[f][k], gft.state_truth(fo, groups), _bounds(fo, zero, groups, TOLS["double"]))
            print("triclinic frame %d state %d: worst error / bound %.3e" % (f, k, ratio))
            assert ratio <= 1.0, (f, k, ratio)
    assert np.isfinite(rows).all()
    eng.close()


# ---- 5. 60 atoms: host lists, per-pair wrap, through Python ------------------------------------------------------------------------------
def _small_frames(snb, oracle, method):
    """Frame 0: the system's own coordinates; frames 1 and 2: seeded perturbations of 0.02 nm (float32-representable), with the one-hot
    truth table of each."""
    key = ("small", method)
    if key not in _CACHE:
        force, pos, box = _small_force(snb, method)
        rng = np.random.default_rng(43)
        moved = np.stack([pos + 0.02 * rng.standard_normal(pos.shape) for _ in range(2)]).astype(np.float32).astype(np.float64)
        frames = np.ascontiguousarray(np.concatenate([pos[None], moved]))
        sub = aft.force_subsets(force)
        _CACHE[key] = (frames, [aft.truth_table(aft.force_evaluator(oracle, force, frames[f], box), sub, 3) for f in (1, 2)])
    return _CACHE[key]


@pytest.mark.parametrize("prec", ["double", "single"])
@pytest.mark.parametrize("method", list(SMALL))
def test_60_atoms_through_python(method, prec, snb, oracle, small_truths):
    groups = [list(range(a, min(a + 7, 60))) for a in range(0, 60, 7)] + [list(range(60)), [], [3, 59, 3]]
    force, pos, box = _small_force(snb, method)
    sub = aft.force_subsets(force)
    states = np.stack([np.ones((6, 2)), np.random.default_rng(61).uniform(0.0, 1.0, (6, 2))])
    ctx = _context(snb, force, pos, box, prec)
    zero = np.zeros(60)

    def check(got_rows, got_st, table, label):
        r = _worst_ratio(got_rows, gft.rows_truth(table, groups), _bounds(table, zero, groups, TOLS[prec]))
        worst = [r]
        for k in range(2):
            fo = aft.contract(table, sub, states[k])      # (the oracle's plain forces at the state: tests/test_group_forces_cpu.py)
            worst.append(_worst_ratio(got_st[k], gft.state_truth(fo, groups), _bounds(fo, zero, groups, TOLS[prec])))
        print("%s %s %s: worst error / bound: rows %.3e, states %.3e %.3e" % (method, prec, label, worst[0], worst[1], worst[2]))
        assert max(worst) <= 1.0, worst

    table0 = small_truths(method)
    first = ctx.getGroupForces(force, groups)
    assert first.shape == (len(groups), 3, 2, 3)
    got_rows, got_st = ctx.getGroupForces(force, groups, lambdaStates=states)
    assert got_st.shape == (2, len(groups), 3)
    check(got_rows, got_st, table0, "getGroupForces")
    frames, tables12 = _small_frames(snb, oracle, method)
    kern = ctx._kernelFor(force)
    rows, st = kern.computeGroupForcesForFrames(ctx, groups, frames if prec == "double" else frames.astype(np.float32), lambdaStates=states)
    assert rows.shape == (3, len(groups), 3, 2, 3) and st.shape == (3, 2, len(groups), 3) and np.isfinite(rows).all() and np.isfinite(st).all()
    for f, table in enumerate([table0] + tables12):
        check(rows[f], st[f], table, "frame %d" % f)
    assert kern.computeGroupForcesForFrames(ctx, groups, frames[:2]).shape == (2, len(groups), 3, 2, 3)      # without states: the rows alone
    assert kern.getStats().n_host_rebuilds > 0      # (the host lists: below the GPU builder's floor)
    fs = kern.getFrameStats()
    assert fs.n_batches == 2 and fs.n_frames == 5 and fs.n_built_in_line == 5 and fs.n_built_beside == 0
    again = ctx.getGroupForces(force, groups)      # the context's own state is in place again
    assert _scaled_by_atoms(again, first, groups, SAME_STEP[prec]) <= 1.0
    check(again, got_st, table0, "afterwards")


# ---- 6. contract: the call writes only its outputs --------------------------------------------------------------------------------------
def test_batch_leaves_forces_outputs_energies_and_timers_alone(snb):
    """Mixed precision (bitwise reproducible forces).  A forces step, an energy step, the per-atom force table; then the call with
    positions == NULL and a 3-frame batch in another box: afterwards snb_get_forces, a registered accumulate-mode force output, the
    slice-energy buffer (host copy and device buffer), the timer sums and snb_stats.n_timed are what they were, bit for bit; a following
    snb_evaluate_atom_forces gives the table it gave before (it rebuilds after the batch: the lists in memory were the last frame's), and
    two forces steps equal those of a twin engine that never made the calls: positions and box are the caller's again."""
    import torch
    w = _w24k(); n = len(w["q"]); s = 1.005
    frames = tgf._frames(3, seed=29) * s
    boxes = np.stack([bench.workload_box(w) * s] * 3)
    csr = _csr(snb, _groups24(w)); states = _states(w, 3)
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
    tab_before = _table(A, n, 4)
    f_before = torch.zeros((n, 3), dtype=torch.float32, device="cuda"); A.forces_to(f_before.data_ptr(), False); A.sync()
    out_before = outs[0].clone()
    se_before = A.slice_energies(S4)
    dev = ctypes.c_void_p(); A.ok(A.L.snb_slice_energies_device(A.h, ctypes.byref(dev)))
    dev_before = _device_doubles(dev.value, 2 * S4).clone()
    st0 = A.stats()
    timers_before = (st0.n_timed, st0.sum_direct_ms, st0.sum_recip_ms, st0.sum_total_ms, list(st0.sum_kernel_ms), list(st0.n_kernel_timed))

    def untouched():
        f_after = torch.zeros_like(f_before); A.forces_to(f_after.data_ptr(), False); A.sync()
        assert torch.equal(f_before, f_after)
        assert torch.equal(outs[0], out_before)
        assert np.array_equal(A.slice_energies(S4), se_before)
        assert torch.equal(_device_doubles(dev.value, 2 * S4), dev_before)
        st = A.stats()
        assert (st.n_timed, st.sum_direct_ms, st.sum_recip_ms, st.sum_total_ms, list(st.sum_kernel_ms), list(st.n_kernel_timed)) == timers_before

    now, now_st = _call(A, csr, 4, states=states)      # positions == NULL: the state of the energy step
    assert np.isfinite(now).all() and np.isfinite(now_st).all() and np.abs(now).max() > 1.0
    untouched()
    err = aft.rel(_table(A, n, 4), tab_before)
    print("the table after the call with positions == NULL: %.3e" % err)
    assert err < SAME_TABLE
    rows, st = _call(A, csr, 4, frames, False, boxes=boxes, states=states)
    assert np.isfinite(rows).all() and np.isfinite(st).all() and np.abs(rows).max() > 1.0
    untouched()
    r0 = A.stats().n_rebuilds
    err = aft.rel(_table(A, n, 4), tab_before)
    assert A.stats().n_rebuilds == r0 + 1      # the lists in memory belonged to the last frame
    # Another list stores other image offsets: single-precision coordinates differ by their rounding, and a cutoff-band pair may fall on
    # the other side.  Each table is held to the oracle at TOLS plus the band allowance (tests/test_gpu_atom_forces.py), so the two differ
    # by less than 2 TOLS plus the allowances; asserted at TOLS without an allowance.  (Measured on an MI355X: 4.3e-5.)
    print("the table after the batch (another list): %.3e" % err)
    assert err <= TOLS["mixed"]
    untouched()
    A.rebuild(); B.rebuild()
    fa = torch.zeros_like(f_before); fb = torch.zeros_like(f_before)
    for p in (p3, p1):
        for e, f in ((A, fa), (B, fb)):
            e.set_positions_device(p.data_ptr(), False); e.execute(False); e.forces_to(f.data_ptr(), False); e.sync()
        assert torch.equal(fa, fb)
        assert torch.equal(outs[0], outs[1])
    A.close(); B.close()


# ---- 7. bound context -------------------------------------------------------------------------------------------------------------------
def test_bound_context(snb):
    """posq in a random context order: positions == NULL gives the unbound outputs and leaves the binding's buffers alone; frames are refused."""
    import torch
    from test_gpu_context_binding import View
    w = _w24k(); groups = _groups24(w); csr = _csr(snb, groups); states = _states(w, 3)
    ref = _engine(snb, "pme", "single")
    pos = tgf._dev(w["pos"], False)
    ref.set_positions_device(pos.data_ptr(), False)
    want_rows, want_st = _call(ref, csr, 4, states=states)
    ref.close()
    v = View(w["pos"], False, seed=23, n_derivs=2 * S4)
    eng = _engine(snb, "pme", "single")
    slots = np.arange(2 * S4, dtype=np.int32).reshape(S4, 2)
    b = v.binding(snb.capi, deriv_slot=slots)
    torch.cuda.synchronize()
    eng.ok(eng.L.snb_bind_context(eng.h, ctypes.byref(b)))
    posq0 = v.posq.clone()
    rows, st = _call(eng, csr, 4, states=states)
    torch.cuda.synchronize()
    r_rows = _scaled_by_atoms(rows, want_rows, groups, SAME_STEP["single"]); r_st = _scaled_by_atoms(st, want_st, groups, SAME_STEP["single"])
    print("bound against unbound, worst error / (SAME_STEP x atoms): rows %.3e, states %.3e" % (r_rows, r_st))
    assert np.isfinite(rows).all() and np.isfinite(st).all() and r_rows <= 1.0 and r_st <= 1.0
    assert torch.equal(v.posq, posq0) and torch.equal(v.buf, v.P) and torch.equal(v.ebuf, v.E0) and torch.equal(v.dbuf, v.D0)
    f0 = tgf._fstats(eng); r0 = eng.stats().n_rebuilds
    assert _call(eng, csr, 4, tgf._frames(4)[:2], False, states=states, expect=snb.capi.SNB_ERR_STATE) == snb.capi.SNB_ERR_STATE
    f1 = tgf._fstats(eng)
    assert (f1.n_batches, f1.n_frames) == (f0.n_batches, f0.n_frames) and eng.stats().n_rebuilds == r0
    assert torch.equal(v.buf, v.P) and torch.equal(v.ebuf, v.E0) and torch.equal(v.dbuf, v.D0)
    eng.close()


# ---- 8. status codes --------------------------------------------------------------------------------------------------------------------
def test_status_codes(snb):
    capi = snb.capi; INVALID = capi.SNB_ERR_INVALID_ARGUMENT
    w = _w24k(); n = len(w["q"]); frames = tgf._frames(4)
    eng = _engine(snb, "rf", "single")
    pos = tgf._dev(w["pos"], False)
    eng.set_positions_device(pos.data_ptr(), False)
    good = _csr(snb, [[0, 1, 2], [], [7, 8]]); states = _states(w, 3)

    def state():
        f = tgf._fstats(eng)
        return (int(eng.stats().n_rebuilds), int(f.n_batches), int(f.n_frames), int(f.n_built_in_line), int(f.n_built_beside))
    before = state()
    assert eng.L.snb_evaluate_group_forces(eng.h, None) == INVALID
    assert eng.L.snb_evaluate_group_forces(None, ctypes.byref(capi.SnbGroupForceBatch())) == INVALID
    _call(eng, good, 4, frames, False, rows=False, expect=INVALID)                                 # NULL group_forces with n_states == 0
    _call(eng, good, 4, frames, False, states=states, state_out=False, expect=INVALID)             # states without state_forces
    _call(eng, good, 4, frames, False, n_states=2, expect=INVALID)                                 # states without state_lambdas
    _call(eng, good, 4, frames, False, n_states=-1, expect=INVALID)                                # negative n_states
    b = capi.SnbGroupForceBatch(); b.n_frames = 1; b.n_groups = 3; b.include_direct = 1; b.include_reciprocal = 1
    sink = np.zeros((3, 4, 2, 3)); b.group_forces = sink.ctypes.data_as(ctypes.c_void_p)
    b.group_atoms = _ip(good[1])
    assert eng.L.snb_evaluate_group_forces(eng.h, ctypes.byref(b)) == INVALID                       # NULL group_start
    b.group_start = _ip(good[0]); b.group_atoms = None
    assert eng.L.snb_evaluate_group_forces(eng.h, ctypes.byref(b)) == INVALID                       # NULL group_atoms
    b.group_atoms = _ip(good[1]); b.n_groups = 0
    assert eng.L.snb_evaluate_group_forces(eng.h, ctypes.byref(b)) == INVALID                       # n_groups < 1
    _call(eng, (np.array([1, 3, 3, 5], dtype=np.int32), good[1]), 4, frames, False, expect=INVALID)      # group_start not starting at 0
    _call(eng, (np.array([0, 3, 2, 5], dtype=np.int32), good[1]), 4, frames, False, expect=INVALID)      # ... decreasing
    for bad in (n, -1):
        _call(eng, _csr(snb, [[0, 1], [2], [3, bad, 4]]), 4, frames, False, states=states, expect=INVALID)      # an index outside [0, N)
        assert b"group 2" in eng.L.snb_last_error(eng.h), eng.L.snb_last_error(eng.h)
    _call(eng, good, 4, frames, False, direct=0, recip=0, expect=INVALID)                          # both include flags 0
    _call(eng, good, 4, frames, False, n_frames=-1, expect=INVALID)                                # negative n_frames
    _call(eng, good, 4, None, False, n_frames=2, expect=INVALID)                                   # positions == NULL with n_frames != 1
    boxes = np.stack([bench.workload_box(w)] * 4); boxes[3] = np.diag([1.9, 6.2145, 6.2145]).reshape(9)
    _call(eng, good, 4, frames, False, boxes=boxes, states=states, expect=capi.SNB_ERR_BOX_TOO_SMALL)
    assert b"frame 3" in eng.L.snb_last_error(eng.h)
    boxes[3] = bench.workload_box(w); boxes[3][1] = 0.1      # not in reduced form
    _call(eng, good, 4, frames, False, boxes=boxes, expect=INVALID)
    assert b"frame 3" in eng.L.snb_last_error(eng.h)
    assert _call(eng, good, 4, frames, False, states=states, n_frames=0, expect=capi.SNB_OK) == capi.SNB_OK      # n_frames == 0: no work
    out, st = _CACHE.pop("last outputs")
    assert np.isnan(out).all() and np.isnan(st).all()      # ... and the outputs untouched
    assert state() == before      # nothing was enqueued
    rows, st = _call(eng, good, 4, frames[:2], False, states=states)      # and the engine serves the next call
    assert np.isfinite(rows).all() and np.isfinite(st).all() and not rows[:, 1].any() and not st[:, :, 1].any()
    eng.close()
    sharded = _engine(snb, "pme", "single", world=2)
    sharded.set_positions_device(pos.data_ptr(), False)
    _call(sharded, good, 4, frames, False, expect=capi.SNB_ERR_UNSUPPORTED)
    _call(sharded, good, 4, None, False, states=states, expect=capi.SNB_ERR_UNSUPPORTED)
    sharded.close()


def test_classic_ewald(snb, oracle):
    """The reciprocal sum of classic Ewald is refused; direct-only works and gives the grouped direct-space truth table."""
    import systems
    F = snb.SlicedNonbondedForce
    force, epos, box = systems.random_box(F, 1500, 3, F.Ewald, 2.6, 1.0, pme=(2.6283, 0, 0, 0))
    force.ewaldKmax = (11, 11, 11)
    ctx = _context(snb, force, epos, box, "double")
    esub = aft.force_subsets(force)
    egroups = [np.flatnonzero(esub == s) for s in range(3)] + [list(range(0, 1500, 3))]
    with pytest.raises(snb.OpenMMException):
        ctx.getGroupForces(force, egroups)
    with pytest.raises(snb.OpenMMException):
        ctx.getGroupForces(force, egroups, includeDirect=False)
    rows = ctx.getGroupForces(force, egroups, includeReciprocal=False)
    table = aft.truth_table(aft.force_evaluator(oracle, force, epos, box, include_reciprocal=False, kmax=(11, 11, 11)), esub, 3)
    ratio = _worst_ratio(rows, gft.rows_truth(table, egroups), _bounds(table, np.zeros(1500), egroups, TOLS["double"]))
    print("Ewald, direct only: worst error / bound %.3e" % ratio)
    assert ratio <= 1.0, ratio
    kern = ctx._kernelFor(force)
    frames2 = np.stack([epos, epos])
    with pytest.raises(snb.OpenMMException):
        kern.computeGroupForcesForFrames(ctx, egroups, frames2)
    both = kern.computeGroupForcesForFrames(ctx, egroups, frames2, includeReciprocal=False)
    assert both.shape == (2, 4, 3, 2, 3)
    for f in range(2):
        assert _worst_ratio(both[f], gft.rows_truth(table, egroups), _bounds(table, np.zeros(1500), egroups, TOLS["double"])) <= 1.0, f
