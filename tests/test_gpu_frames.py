"""Frame batches (-m gpu): snb_evaluate_frames (include/snb.h) -- the raw slice energies of F stored frames in one call, the list of
frame f + 1 built beside the energy-only step of frame f.  Against the oracle at every frame, against the hand-written per-frame loop,
with per-frame boxes, with lambda states, on host-built lists, at full size; what the pipeline counted; what the engine is afterwards.
Tolerances are those of tests/test_gpu_energy_only.py (TOLS, SAME_STEP), with the max(|x|, 1) scaling of the reference.

Frames are the workload's coordinates and seeded Gaussian perturbations of 0.02 nm of them, rounded to float32 and widened back, so
that engines of every precision and the oracle see identical inputs (tests/parity_tools.py, "Identical inputs")."""
import ctypes

import numpy as np
import pytest

import bench
import parity_tools as pt
import systems

pytestmark = pytest.mark.gpu

TOLS = {"single": 1e-3, "double": 1e-5, "mixed": 1e-3}
SAME_STEP = {"single": 1e-6, "mixed": 1e-6, "double": 1e-11}
S24 = 10
METHODS = [(2, 0), (4, 0), (5, 27)]

_W = {}
_ORACLE = {}      # (method, frame key) -> (forces, slice energies)


def _w24k():
    if "w" not in _W:
        _W["w"] = pt.float_positions(bench.build_workload(24000, 6.2145, 4, np.random.default_rng(bench.SEED)))
    return _W["w"]


def _frames(count, seed=17):
    """[count][N][3] float64, float32-representable: the workload, then seeded perturbations of 0.02 nm of it."""
    key = ("frames", count, seed)
    if key not in _W:
        w = _w24k(); rng = np.random.default_rng(seed)
        fr = [w["pos"]] + [w["pos"] + 0.02 * rng.standard_normal(w["pos"].shape) for _ in range(count - 1)]
        _W[key] = np.ascontiguousarray(np.stack(fr).astype(np.float32).astype(np.float64))
    return _W[key]


def _at(w, pos, scale=1.0):
    v = dict(w); v["pos"] = np.ascontiguousarray(pos, dtype=np.float64); v["L"] = w["L"] * scale
    return v


def _oracle(method, dgrid, key, pos, scale=1.0):
    k = (method, key)
    if k not in _ORACLE:
        fo, so, _, _ = bench.oracle_eval(_at(_w24k(), pos, scale), method, 54, dgrid)
        _ORACLE[k] = (fo, so)
    return _ORACLE[k]


def _rel(a, b):
    return float(np.max(np.abs(a - b) / np.maximum(np.abs(b), 1.0)))


def _dev(a, isd):
    import torch
    return torch.tensor(np.asarray(a), dtype=torch.float64 if isd else torch.float32, device="cuda")


def _dp(a):
    return a.ctypes.data_as(ctypes.POINTER(ctypes.c_double))


def _fstats(eng):
    st = eng.capi.SnbFrameStats()
    eng.ok(eng.L.snb_get_frame_stats(eng.h, ctypes.byref(st)))
    return st


def _batch(eng, frames, isd, S, boxes=None, mode=1, dev_in=True, dev_out=False, states=None, expect=0):
    """One snb_evaluate_frames call.  Returns (rows [F][S][2], state energies [F][K] or None) as NumPy arrays; with expect != 0 the status."""
    import torch
    F = len(frames)
    b = eng.capi.SnbFrameBatch()
    b.n_frames = F; b.is_double = int(isd); b.stride4 = 0; b.mode = mode; b.include_direct = 1; b.include_reciprocal = 1
    keep = []
    if dev_in:
        d = _dev(frames, isd); keep.append(d)
        b.positions = d.data_ptr(); b.is_device = 1
    else:
        h = np.ascontiguousarray(frames, dtype=np.float64 if isd else np.float32); keep.append(h)
        b.positions = h.ctypes.data_as(ctypes.c_void_p); b.is_device = 0
    if boxes is not None:
        bx = np.ascontiguousarray(np.asarray(boxes, dtype=np.float64).reshape(F, 9)); keep.append(bx)
        b.boxes = _dp(bx)
    K = 0 if states is None else len(states)
    if K:
        lam = np.ascontiguousarray(states, dtype=np.float64); keep.append(lam)
        b.n_states = K; b.state_lambdas = _dp(lam)
    if dev_out:
        rows = torch.full((F, S, 2), float("nan"), dtype=torch.float64, device="cuda")
        st = torch.full((F, max(K, 1)), float("nan"), dtype=torch.float64, device="cuda")
        b.slice_energies = rows.data_ptr(); b.state_energies = st.data_ptr() if K else None; b.out_is_device = 1
    else:
        rows = np.full((F, S, 2), np.nan); st = np.full((F, max(K, 1)), np.nan)
        b.slice_energies = rows.ctypes.data_as(ctypes.c_void_p); b.state_energies = st.ctypes.data_as(ctypes.c_void_p) if K else None; b.out_is_device = 0
    status = eng.L.snb_evaluate_frames(eng.h, ctypes.byref(b))
    if expect:
        assert status == expect, (status, eng.L.snb_last_error(eng.h))
        return status
    eng.ok(status)
    if dev_out:
        eng.sync()
        rows = rows.cpu().numpy(); st = st.cpu().numpy()
    return rows, (st if K else None)


def _hand_loop(eng, frames, isd, S, boxes=None):
    """The per-frame path: snb_set_box, snb_set_positions, energy-only snb_execute, snb_get_slice_energies -- with snb_rebuild_neighbors per
    frame: the frames are unrelated coordinates (a 0.02 nm perturbation moves one atom in ten further than skin / 2 = 0.05 nm), and a fixed
    rebuild interval does not notice that by itself."""
    out = np.zeros((len(frames), S, 2))
    for f in range(len(frames)):
        if boxes is not None:
            eng.ok(eng.L.snb_set_box(eng.h, _dp(np.ascontiguousarray(boxes[f], dtype=np.float64).reshape(9))))
        p = _dev(frames[f], isd)
        eng.set_positions_device(p.data_ptr(), isd)
        eng.rebuild()
        eng.ok(eng.L.snb_execute(eng.h, 0, 1, 1, 1, None))
        out[f] = eng.slice_energies(S)
    return out


@pytest.mark.parametrize("prec", ["single", "mixed", "double"])
@pytest.mark.parametrize("method,dgrid", METHODS)
def test_frames_vs_oracle_and_vs_per_frame_path(method, dgrid, prec, snb):
    """F = 5 frames, RF / PME / LJPME in every precision: every row and slice against the oracle at that frame; host output and device
    output of the same batch against each other (not bit for bit: the slice sums are double atomics); host frames against device frames;
    and the hand-written per-frame loop on a second engine against the batch."""
    isd = prec == "double"; frames = _frames(5)
    eng = bench.Engine(snb, _w24k(), method, 54, dgrid, prec, 0, 0, 1, 0.1, 1 << 30)
    host, _ = _batch(eng, frames, isd, S24, dev_out=False)
    dev, _ = _batch(eng, frames, isd, S24, dev_out=True)
    up, _ = _batch(eng, frames, isd, S24, dev_in=False)      # host frames through the pinned staging
    for rows in (host, dev, up):
        assert rows.shape == (5, S24, 2) and np.isfinite(rows).all()
    for f in range(5):
        _, so = _oracle(method, dgrid, ("frame", f), frames[f])
        for name, rows in (("host", host), ("device", dev), ("uploaded", up)):
            err = _rel(rows[f], so)
            print("method %d %s frame %d %s output: %.3e" % (method, prec, f, name, err))
            assert err < TOLS[prec], (f, name, err)
    same = _rel(host, dev)
    print("host against device output: %.3e" % same)
    assert same <= SAME_STEP[prec], same
    assert np.array_equal(eng.slice_energies(S24), up[4])      # the engine's own buffer keeps the last frame of the last batch
    other = bench.Engine(snb, _w24k(), method, 54, dgrid, prec, 0, 0, 1, 0.1, 1 << 30)
    loop = _hand_loop(other, frames, isd, S24)
    err = _rel(host, loop)
    print("batch against the per-frame path: %.3e" % err)
    assert err < TOLS[prec], err
    eng.close(); other.close()


def test_frames_with_their_own_boxes(snb):
    """Box and coordinates scaled by 1, 1.005, 1.005, 0.995, 1: every frame against the oracle on the scaled workload (the closed-form
    terms use the frame's volume), and every box change built in line."""
    w = _w24k(); scales = [1.0, 1.005, 1.005, 0.995, 1.0]
    frames = np.stack([w["pos"] * s for s in scales])
    boxes = np.stack([bench.workload_box(w) * s for s in scales])
    eng = bench.Engine(snb, w, 4, 54, 0, "double", 0, 0, 1, 0.1, 1 << 30)
    before = _fstats(eng).n_built_in_line
    rows, _ = _batch(eng, frames, True, S24, boxes=boxes)
    assert np.isfinite(rows).all()
    for f, s in enumerate(scales):
        _, so = _oracle(4, 0, ("scaled", s), frames[f], s)
        err = _rel(rows[f], so)
        print("scale %.3f frame %d: %.3e" % (s, f, err))
        assert err < TOLS["double"], (f, err)
    changes = sum(1 for f in range(1, 5) if scales[f] != scales[f - 1])
    assert _fstats(eng).n_built_in_line - before >= changes
    # the engine's box is its own again: the per-frame path at the original box gives frame 0
    eng.set_positions_device(_dev(frames[0], True).data_ptr(), True)
    eng.ok(eng.L.snb_execute(eng.h, 0, 1, 1, 1, None))
    assert _rel(eng.slice_energies(S24), rows[0]) < TOLS["double"]
    eng.close()


def test_the_pipeline_ran(snb):
    """A warm engine (three forces steps, two forced rebuilds), a constant-box batch of 8: all but the first frame -- and at most one
    discarded side build -- are built beside the previous frame's step."""
    w = _w24k(); frames = _frames(8, seed=23)
    eng = bench.Engine(snb, w, 4, 54, 0, "single", 0, 0, 1, 0.1, 1 << 30)
    pos = _dev(w["pos"], False)
    eng.set_positions_device(pos.data_ptr(), False)
    eng.execute(False); eng.rebuild(); eng.execute(False); eng.rebuild(); eng.execute(False); eng.sync()
    s0 = eng.stats(); f0 = _fstats(eng)
    rows, _ = _batch(eng, frames, False, S24, dev_out=True)
    assert np.isfinite(rows).all()
    s1 = eng.stats(); f1 = _fstats(eng)
    print("built beside %d, in line %d, side builds discarded %d, rebuilds %d" % (f1.n_built_beside - f0.n_built_beside, f1.n_built_in_line - f0.n_built_in_line,
                                                                                  f1.n_side_discarded - f0.n_side_discarded, s1.n_rebuilds - s0.n_rebuilds))
    assert f1.n_batches - f0.n_batches == 1
    assert f1.n_frames - f0.n_frames == 8
    assert (f1.n_built_beside + f1.n_built_in_line) - (f0.n_built_beside + f0.n_built_in_line) == 8
    assert f1.n_built_in_line - f0.n_built_in_line <= 2
    assert s1.n_list_overruns == s0.n_list_overruns
    assert s1.n_rebuilds - s0.n_rebuilds >= 8      # frame steps count as rebuilds
    assert f1.last_batch_ms == 0.0      # device output: the call did not end in a synchronise
    eng.close()


def test_mode_2_and_lambda_states(snb):
    w = _w24k(); frames = _frames(5)
    eng = bench.Engine(snb, w, 4, 54, 0, "single", 0, 0, 1, 0.1, 1 << 30)
    mask = np.zeros(S24, dtype=np.int32); mask[[2, 9]] = 1
    eng.set_energy_slices(mask)
    sel, _ = _batch(eng, frames, False, S24, mode=2)
    for f in range(5):
        _, so = _oracle(4, 0, ("frame", f), frames[f])
        assert _rel(sel[f][mask == 1], so[mask == 1]) < TOLS["single"], f
    lam = np.random.default_rng(5).uniform(0.0, 1.0, (3, S24, 2))
    assert _batch(eng, frames, False, S24, mode=2, states=lam, expect=eng.capi.SNB_ERR_INVALID_ARGUMENT) == eng.capi.SNB_ERR_INVALID_ARGUMENT
    for dev_out in (False, True):
        rows, st = _batch(eng, frames, False, S24, mode=1, states=lam, dev_out=dev_out)
        assert st.shape == (5, 3) and np.isfinite(st).all()
        for f in range(5):
            for k in range(3):
                want = float((lam[k] * rows[f]).sum()); bound = 4 * S24 * 2.0 ** -52 * float(np.abs(lam[k] * rows[f]).sum())
                assert abs(st[f, k] - want) <= bound, (f, k, st[f, k], want, bound)
    eng.close()


def test_the_engine_afterwards(snb):
    """Mixed precision (forces reproducible bit for bit).  A: forces step at P, a batch of other frames in another box, then
    snb_get_forces and the registered force output are what they were; the next forces step at P equals, bit for bit, that of an engine
    that never ran a batch and was told to rebuild, and agrees with the oracle."""
    import torch
    w = _w24k(); n = len(w["q"]); s = 1.005
    frames = _frames(4, seed=29) * s
    boxes = np.stack([bench.workload_box(w) * s] * 4)
    P = _dev(w["pos"], False)
    fo, _ = _oracle(4, 0, ("frame", 0), w["pos"])
    got = {}
    for name in ("A", "B"):
        eng = bench.Engine(snb, w, 4, 54, 0, "mixed", 0, 0, 1, 0.1, 1 << 30)
        eng.set_timing_interval(0)
        out = torch.full((n, 3), 7.25, dtype=torch.float32, device="cuda")
        eng.set_force_output(out.data_ptr(), False, 1)
        eng.set_positions_device(P.data_ptr(), False); eng.execute(False)
        f1 = torch.zeros((n, 3), dtype=torch.float32, device="cuda"); eng.forces_to(f1.data_ptr(), False); eng.sync()
        before = out.clone()
        if name == "A":
            rows, _ = _batch(eng, frames, False, S24, boxes=boxes)
            assert np.isfinite(rows).all()
            f2 = torch.zeros_like(f1); eng.forces_to(f2.data_ptr(), False); eng.sync()
            assert torch.equal(f1, f2)
            assert torch.equal(out, before)
        else:
            eng.rebuild()
        r0 = eng.stats().n_rebuilds
        eng.execute(False)
        f3 = torch.zeros_like(f1); eng.forces_to(f3.data_ptr(), False); eng.sync()
        assert eng.stats().n_rebuilds > r0      # the lists in memory belonged to the last frame
        assert not torch.equal(out, before)      # a forces step does add to the registered output
        got[name] = f3
        err = np.linalg.norm(f3.double().cpu().numpy() - fo, axis=1) / np.maximum(np.linalg.norm(fo, axis=1), 1.0)
        assert err.max() < TOLS["mixed"], (name, err.max())
        eng.close()
    assert torch.equal(got["A"], got["B"])


def test_validation(snb):
    import torch
    w = _w24k(); n = len(w["q"]); frames = _frames(5); capi = snb.capi
    eng = bench.Engine(snb, w, 4, 54, 0, "single", 0, 0, 1, 0.1, 1 << 30)
    b = capi.SnbFrameBatch()      # n_frames = 0, everything else null
    assert eng.L.snb_evaluate_frames(eng.h, ctypes.byref(b)) == capi.SNB_OK
    b.n_frames = -1
    assert eng.L.snb_evaluate_frames(eng.h, ctypes.byref(b)) == capi.SNB_ERR_INVALID_ARGUMENT
    b.n_frames = 2; b.mode = 1
    assert eng.L.snb_evaluate_frames(eng.h, ctypes.byref(b)) == capi.SNB_ERR_INVALID_ARGUMENT      # null pointers
    assert _batch(eng, frames, False, S24, mode=3, expect=capi.SNB_ERR_INVALID_ARGUMENT)
    f0 = _fstats(eng)
    boxes = np.stack([bench.workload_box(w)] * 5); boxes[3] = np.diag([1.9, 6.2145, 6.2145]).reshape(9)
    assert _batch(eng, frames, False, S24, boxes=boxes, expect=capi.SNB_ERR_BOX_TOO_SMALL)
    assert b"frame 3" in eng.L.snb_last_error(eng.h)
    boxes[3] = bench.workload_box(w); boxes[3][1] = 0.1      # not in reduced form
    assert _batch(eng, frames, False, S24, boxes=boxes, expect=capi.SNB_ERR_INVALID_ARGUMENT)
    assert b"frame 3" in eng.L.snb_last_error(eng.h)
    f1 = _fstats(eng)
    assert (f1.n_frames, f1.n_batches, f1.n_built_in_line) == (f0.n_frames, f0.n_batches, f0.n_built_in_line)      # nothing was enqueued
    # bound engine
    posq = torch.zeros((n, 4), dtype=torch.float32, device="cuda"); posq[:, :3] = _dev(w["pos"], False)
    index = torch.arange(n, dtype=torch.int32, device="cuda")
    cb = capi.SnbContextBinding(); cb.posq = posq.data_ptr(); cb.atom_index = index.data_ptr(); cb.is_double = 0; cb.padded_n = n
    eng.ok(eng.L.snb_bind_context(eng.h, ctypes.byref(cb)))
    assert _batch(eng, frames, False, S24, expect=capi.SNB_ERR_STATE)
    eng.ok(eng.L.snb_bind_context(eng.h, None))
    rows, _ = _batch(eng, frames[:2], False, S24)      # unbound again: served
    assert np.isfinite(rows).all()
    eng.close()
    sharded = bench.Engine(snb, w, 4, 54, 0, "single", 0, 0, 2, 0.1, 1 << 30)
    assert _batch(sharded, frames, False, S24, expect=capi.SNB_ERR_UNSUPPORTED)
    sharded.close()


def _context(snb, force, pos, box, prec):
    system = snb.System()
    for _ in range(force.getNumParticles()):
        system.addParticle(1.0)
    system.setDefaultPeriodicBoxVectors(*box)
    system.addForce(force)
    ctx = snb.Context(system, precision=prec, device=0)
    ctx.setPositions(pos)
    return ctx


@pytest.mark.parametrize("prec", ["single", "double"])
@pytest.mark.parametrize("method", ["NoCutoff", "CutoffNonPeriodic"])
def test_host_built_lists_through_python(method, prec, snb, oracle):
    """Lists built on the host / a non-periodic system: every frame in line, through computeSliceEnergiesForFrames."""
    F = snb.SlicedNonbondedForce
    force, pos, box = systems.random_box(F, 1500, 3, getattr(F, method), 3.0, 1.0)
    rng = np.random.default_rng(31)
    frames = np.stack([pos] + [pos + 0.02 * rng.standard_normal(pos.shape) for _ in range(2)]).astype(np.float32).astype(np.float64)
    ctx = _context(snb, force, frames[0], box, prec)      # (the context's own coordinates: frame 0, as rounded)
    kern = ctx._kernelFor(force)
    got = kern.computeSliceEnergiesForFrames(ctx, frames if prec == "double" else frames.astype(np.float32))
    assert got.shape == (3, 6, 2) and np.isfinite(got).all()
    want = [oracle.evaluate(force, frames[f], box)["slice_energies"] for f in range(3)]
    for f in range(3):
        err = _rel(got[f], want[f])
        print("%s %s frame %d: %.3e" % (method, prec, f, err))
        assert err < TOLS[prec], (f, err)
    st = kern.getFrameStats()
    assert st.n_frames == 3 and st.n_built_in_line == 3 and st.n_built_beside == 0
    lam = np.random.default_rng(7).uniform(0.0, 1.0, (2, 6, 2))
    sel = kern.computeSliceEnergiesForFrames(ctx, frames, slices=[1, 4])
    assert np.isnan(sel[:, [0, 2, 3, 5]]).all()
    for f in range(3):
        assert _rel(sel[f][[1, 4]], want[f][[1, 4]]) < TOLS[prec], f
    rows, states = kern.computeSliceEnergiesForFrames(ctx, frames, lambdaStates=lam)
    assert states.shape == (3, 2)
    assert np.allclose(states, np.einsum("kst,fst->fk", lam, rows), rtol=1e-12, atol=1e-9)
    # the context's own evaluation is undisturbed
    assert _rel(kern.computeSliceEnergies(ctx), want[0]) < TOLS[prec]


@pytest.mark.parametrize("prec", ["single", "double"])
def test_python_frames_from_a_device_pointer(prec, snb, oracle):
    """computeSliceEnergiesForFrames with positionsDevicePointer (a torch tensor's address) and numFrames: a periodic PME system, against
    the oracle and against the same frames given as a host array."""
    F = snb.SlicedNonbondedForce; isd = prec == "double"
    force, pos, box = systems.random_box(F, 3000, 4, F.PME, 3.2, 1.0, pme=(2.6283, 28, 28, 28))
    rng = np.random.default_rng(37)
    frames = np.stack([pos] + [pos + 0.02 * rng.standard_normal(pos.shape) for _ in range(3)]).astype(np.float32).astype(np.float64)
    ctx = _context(snb, force, frames[0], box, prec)
    kern = ctx._kernelFor(force)
    dev = _dev(frames, isd)
    got = kern.computeSliceEnergiesForFrames(ctx, positionsDevicePointer=(dev.data_ptr(), isd), numFrames=4)
    host = kern.computeSliceEnergiesForFrames(ctx, frames if isd else frames.astype(np.float32))
    assert got.shape == (4, 10, 2) and np.isfinite(got).all()
    for f in range(4):
        want = oracle.evaluate(force, frames[f], box)["slice_energies"]
        assert _rel(got[f], want) < TOLS[prec], (f, _rel(got[f], want))
    assert _rel(got, host) < TOLS[prec]      # same frames, lists built again: the order of the sums differs


def test_frames_c3_at_full_size(snb):
    """c3 (300k atoms, single precision), F = 3 times the same coordinates, constant box: frame 0 against the oracle with the
    truncation-band allowance of the full-size parity tests; frames 1 and 2 -- other lists, the third built beside the second's step --
    equal frame 0 within SAME_STEP."""
    n_target, Lbox, nsub, method, grid, dgrid, _ = bench.CONFIGS["c3"]
    w, fo, so, _, _, fa, ea, _ = pt.fullsize_case("c3", "single")
    S = nsub * (nsub + 1) // 2
    eng = bench.Engine(snb, w, method, grid, dgrid, "single", 0, 0, 1, 0.1, 1 << 30)
    frames = np.stack([w["pos"]] * 3)
    rows, _ = _batch(eng, frames, False, S, dev_out=True)
    assert np.isfinite(rows).all()
    rec = pt.compare(fo, rows[0], fo, so, TOLS["single"], fa, ea)
    assert rec["ok"], rec
    for f in (1, 2):
        err = _rel(rows[f], rows[0])
        print("frame %d against frame 0: %.3e" % (f, err))
        assert err <= SAME_STEP["single"], (f, err)
    st = _fstats(eng)
    print("built beside %d, in line %d, discarded %d" % (st.n_built_beside, st.n_built_in_line, st.n_side_discarded))
    assert st.n_built_beside + st.n_built_in_line == 3
    eng.close()
