"""Per-slice virial tensors, at the current state and over stored frames (-m gpu): snb_evaluate_slice_virials (include/snb.h, DESIGN.md
section 4.14).

Ground truth is the oracle alone (tests/slice_virial_truth.py): W = -dE_raw/dh along the six deformations of box and atoms, a 4-point
stencil of the oracle's raw slice energies, with an empty cutoff shell and the self-consistency of the stencil ASSERTED on every truth.
The error of a (slice, term) is the Frobenius norm of the six components' differences (off-diagonals twice) over
max(||want||_F, |E_raw[s][t]|, 1); the bars are the project's TOLS of tests/test_gpu_atom_forces.py, 1e-3 single and mixed, 1e-5 double.
No allowance is added in any precision: the single-precision Coulomb rows of cross slices stay inside the bar on these systems as they
are (the worst ratios are printed per case and recorded in DESIGN.md section 4.14).  Two evaluations of one state agree within SAME_STEP of
tests/test_gpu_frames.py.  The systems are small: 600 atoms in 3 nm and 60 atoms run on host-built lists and the per-pair-wrap kernels
(the box is too small for the GPU builder), 4096 sparse atoms in 12 nm on the GPU builder's lists; the 24k-atom box of the other GPU tests,
whose cutoff shell cannot be emptied, is held to its twin on host-built lists.  Every engine and the oracle are given float32-representable
coordinates; truths are computed once per (system, flags) and shared."""
import ctypes
import importlib
import types

import numpy as np
import pytest

import slice_virial_truth as svt
import systems
from test_gpu_atom_forces import TOLS, _context, _device_doubles
from test_gpu_frames import SAME_STEP

pytestmark = pytest.mark.gpu

L3, RC = 3.0, 1.0
MESH, DMESH = (3.0, 30, 32, 36), (3.0, 24, 27, 30)      # three different sizes per mesh
METHODS = {
    "rf": dict(method="CutoffPeriodic", kw=dict(switch=True)),
    "pme": dict(method="PME", kw=dict(pme=MESH)),
    "ljpme": dict(method="LJPME", kw=dict(pme=MESH, ljpme=DMESH)),
}
TRICLINIC = np.array([[3.0, 0.0, 0.0], [0.4, 3.1, 0.0], [-0.3, 0.5, 2.9]])
FLAGS = {"both": (True, True), "direct": (True, False), "reciprocal": (False, True)}

_SYSTEMS, _TRUTHS = {}, {}


def _dp(a):
    return a.ctypes.data_as(ctypes.POINTER(ctypes.c_double))


def _system(snb, name):
    """(force, positions, box or None, cutoff or None) of a named system; positions float32-representable, the cutoff shell cleared."""
    if name in _SYSTEMS:
        return _SYSTEMS[name]
    F = snb.SlicedNonbondedForce
    rng = np.random.default_rng(71)
    if name in METHODS:
        m = METHODS[name]
        force, pos, box = systems.random_box(F, 600, 3, getattr(F, m["method"]), L3, RC, **m["kw"])
        assert force.getUseDispersionCorrection() and force.getNumExceptions() > 0
    elif name == "triclinic":
        force, pos, _ = systems.random_box(F, 600, 3, F.PME, L3, RC, pme=MESH)
        box = TRICLINIC.copy(); pos = (pos / L3) @ box      # the lattice in the cell's own fractional coordinates
    elif name == "nine":      # 9 subsets, 45 slices; subset 4 handed to subset 5: a subset without atoms in the middle (the last slab holds none either)
        force, pos, box = systems.random_box(F, 600, 9, F.PME, L3, RC, pme=MESH)
        for i in range(600):
            if force.getParticleSubset(i) == 4:
                force.setParticleSubset(i, 5)
    elif name == "sparse":      # the smallest box the GPU list builder accepts with few enough pairs near the cutoff to clear its shell
        force, pos, box = systems.random_box(F, 4096, 3, F.PME, 12.0, RC, pme=(3.0, 36, 40, 45))
    elif name == "ewald":
        force, pos, box = systems.random_box(F, 600, 3, F.Ewald, L3, RC, pme=(3.0, 0, 0, 0))
        force.ewaldKmax = (11, 11, 11)
    else:      # 60 atoms: host-built lists
        force, pos, box = systems.random_box(F, 60, 3, getattr(F, name), 2.05, RC)
        if name == "NoCutoff":
            _SYSTEMS[name] = (force, np.asarray(pos, dtype=np.float64).astype(np.float32).astype(np.float64), None, None)
            return _SYSTEMS[name]
        box = None
    pos, rounds = svt.clear_shell(pos, box, RC, 8.0 * svt.H * RC, rng)
    print("%s: cutoff shell cleared in %d rounds" % (name, rounds))
    _SYSTEMS[name] = (force, pos, box, RC)
    return _SYSTEMS[name]


def _truth(snb, oracle, name, flags="both"):
    """(W[S][2][6], E_raw[S][2]) of a system under the given include flags, from the oracle."""
    if (name, flags) not in _TRUTHS:
        force, pos, box, rc = _system(snb, name)
        d, r = FLAGS[flags]
        kw = dict(kmax=(11, 11, 11)) if name == "ewald" else {}
        w, e, worst = svt.truth(svt.force_energy(oracle, force, None, d, r, **kw), pos, box, rc)
        print("truth %s %s: stencils at h and 2h differ by %.3e of the entry's scale" % (name, flags, worst))
        _TRUTHS[(name, flags)] = (w, e)
    return _TRUTHS[(name, flags)]


def _ctx(snb, name, prec):
    force, pos, box, _ = _system(snb, name)
    ctx = _context(snb, force, pos, box if box is not None else np.diag([2.05, 2.05, 2.05]), prec)
    return ctx, ctx._kernelFor(force), force


def _check(got, snb, oracle, name, flags, prec, label):
    want, e = _truth(snb, oracle, name, flags)
    assert got.shape == want.shape and np.isfinite(got).all()
    r = svt.ratios(got, want, e)
    print("%s %s %s: worst ratio Coulomb %.3e, vdW %.3e" % (label, flags, prec, r[:, 0].max(), r[:, 1].max()))
    assert r.max() < TOLS[prec], r
    return want, e


# ---- 1. against the truth: RF, PME, LJPME x single, mixed, double x both flags, direct only, reciprocal only -----------------------------
@pytest.mark.parametrize("prec", ["single", "mixed", "double"])
@pytest.mark.parametrize("name", list(METHODS))
def test_600_atoms_against_the_truth(name, prec, snb, oracle):
    ctx, kern, force = _ctx(snb, name, prec)
    got = {f: ctx.getSliceVirials(force, includeDirect=d, includeReciprocal=r) for f, (d, r) in FLAGS.items()}
    want, e = _check(got["both"], snb, oracle, name, "both", prec, name)
    assert svt.frobenius(want)[:, 0].min() > 1.0 and svt.frobenius(want)[:, 1].max() > 1.0      # every slice carries a tensor
    _check(got["direct"], snb, oracle, name, "direct", prec, name)
    wr, _ = _check(got["reciprocal"], snb, oracle, name, "reciprocal", prec, name)
    if name == "rf":
        assert not got["reciprocal"].any() and not wr.any()
    else:
        assert svt.frobenius(wr[:, 0]).max() > 1.0
        if name == "ljpme":
            assert svt.frobenius(wr[:, 1]).max() > 1.0
        else:      # PME: the mesh carries no vdW term, and the dispersion correction goes with the direct part
            assert not wr[:, 1].any() and not got["reciprocal"][:, 1].any()
    parts = svt.ratios(got["direct"] + got["reciprocal"], got["both"], e)
    print("%s %s: direct + reciprocal against both: %.3e" % (name, prec, parts.max()))
    assert parts.max() < SAME_STEP[prec]


# ---- 1b. the GPU list builder: image codes instead of the per-pair wrap ------------------------------------------------------------------
@pytest.mark.parametrize("prec", ["single", "double"])
def test_4096_atoms_on_gpu_built_lists(prec, snb, oracle):
    """A 3 nm box is too small for the GPU list builder (it asks for four block edges and two list radii per box edge), so the 600-atom
    systems run on host-built lists and the per-pair-wrap kernels.  4096 atoms in 12 nm take the GPU builder, whose tiles carry periodic
    image codes, and stay sparse enough for the cutoff shell to be cleared."""
    ctx, kern, force = _ctx(snb, "sparse", prec)
    got = ctx.getSliceVirials(force)
    st = kern.getStats()
    assert st.n_host_rebuilds == 0 and st.n_rebuilds == 1      # (the GPU list builder)
    want, _ = _check(got, snb, oracle, "sparse", "both", prec, "4096 atoms")
    assert svt.frobenius(want)[:, 0].min() > 1.0


def _engine24(snb, w, prec, host_build):
    """bench.Engine on the 24k-atom PME workload, with the choice of list builder."""
    import bench
    eng = bench.Engine.__new__(bench.Engine)
    eng.capi = snb.capi; eng.L = snb.capi.lib(); eng.h = ctypes.c_void_p()
    cfg = eng.capi.SnbConfig()
    cfg.abi_version = eng.capi.SNB_ABI_VERSION; cfg.n_atoms = len(w["q"]); cfg.n_subsets = w["nsub"]; cfg.method = 4
    cfg.precision = {"single": 0, "double": 1, "mixed": 2}[prec]; cfg.cutoff = bench.CUTOFF; cfg.rf_dielectric = 78.3
    cfg.alpha = bench.ALPHA; cfg.grid[0] = cfg.grid[1] = cfg.grid[2] = 54; cfg.alpha_d = bench.ALPHA; cfg.dgrid[0] = cfg.dgrid[1] = cfg.dgrid[2] = 1
    cfg.neighbor_padding = 0.1; cfg.rebuild_interval = 1 << 30; cfg.shard_count = 1; cfg.host_neighbor_build = int(host_build)
    eng.ok(eng.L.snb_create(ctypes.byref(cfg), ctypes.byref(eng.h)), create=True)
    ip = lambda a: a.ctypes.data_as(ctypes.POINTER(ctypes.c_int32))
    eng.ok(eng.L.snb_set_particles(eng.h, _dp(w["q"]), _dp(w["sigma"]), _dp(w["epsilon"]), ip(w["subset"])))
    eng.ok(eng.L.snb_set_exceptions(eng.h, len(w["exc_qq"]), ip(w["exc_pairs"]), _dp(w["exc_qq"]), _dp(w["exc_sigma"]), _dp(w["exc_eps"]), None))
    eng.ok(eng.L.snb_set_lambdas(eng.h, _dp(np.ascontiguousarray(w["lam"]))))
    eng.ok(eng.L.snb_set_box(eng.h, _dp(bench.workload_box(w))))
    pos = np.ascontiguousarray(w["pos"], dtype=np.float64)
    eng.ok(eng.L.snb_set_positions(eng.h, pos.ctypes.data_as(ctypes.c_void_p), 0, 1, 0))
    eng._pos = pos; eng._lib = eng.L; eng._h = eng.h; eng.numSlices = w["nsub"] * (w["nsub"] + 1) // 2
    return eng


@pytest.mark.parametrize("prec", ["single", "double"])
def test_24k_bricks_and_gpu_lists_equal_host_lists(prec, snb, oracle):
    """The 24k-atom box of the other GPU tests takes the GPU list builder, the brick spreader and -- in a step -- the plane path, which this
    call must leave for the three-pass transforms.  Its cutoff shell cannot be emptied (24 000 pairs within 8 h r_c of the cutoff), so there
    is no strain truth for it; instead the engine on its own choice of builder is held to a twin on host-built lists -- per-pair wrap, no
    sort columns for the own-atoms spreader's plane-major spectrum -- the path the small systems check against the oracle.  Both lie
    within TOLS of one truth, so they are asked to agree within TOLS; the scale takes |E_raw| from the oracle."""
    import test_gpu_frames as tgf
    w = tgf._w24k()
    if "e24" not in _TRUTHS:
        import bench
        _TRUTHS["e24"] = bench.oracle_eval(w, 4, 54, 0)[1]
    a = _engine24(snb, w, prec, False); b = _engine24(snb, w, prec, True)
    (sa, ra, _), (sb, rb, _) = _batch(a), _batch(b)
    assert sa == 0 and sb == 0
    assert a.stats().n_host_rebuilds == 0 and b.stats().n_host_rebuilds == 1
    err = svt.ratios(ra[0], rb[0], _TRUTHS["e24"])
    print("24k %s: GPU-built lists and bricks against host-built lists: Coulomb %.3e, vdW %.3e" % (prec, err[:, 0].max(), err[:, 1].max()))
    assert np.isfinite(ra).all() and svt.frobenius(rb[0])[:, 0].min() > 1.0
    assert err.max() < TOLS[prec]
    part = {f: _batch(a, direct=int(d), recip=int(r))[1][0] for f, (d, r) in FLAGS.items() if f != "both"}      # the parts add up on this path as well
    parts = svt.ratios(part["direct"] + part["reciprocal"], ra[0], _TRUTHS["e24"])
    assert parts.max() < SAME_STEP[prec]
    a.close(); b.close()


# ---- 2. a triclinic PME cell ------------------------------------------------------------------------------------------------------------
def test_triclinic_pme_cell(snb, oracle):
    ctx, kern, force = _ctx(snb, "triclinic", "double")
    got = ctx.getSliceVirials(force)
    want, _ = _check(got, snb, oracle, "triclinic", "both", "double", "triclinic pme")
    assert np.abs(want[:, 0, 3:]).max() > 1.0      # (shear components that matter)
    _check(ctx.getSliceVirials(force, includeDirect=False), snb, oracle, "triclinic", "reciprocal", "double", "triclinic pme")


# ---- 3. host-built lists ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("prec", ["double", "single"])
@pytest.mark.parametrize("name", ["NoCutoff", "CutoffNonPeriodic"])
def test_60_atoms_on_host_built_lists(name, prec, snb, oracle):
    ctx, kern, force = _ctx(snb, name, prec)
    got = ctx.getSliceVirials(force)
    assert kern.getStats().n_host_rebuilds > 0      # (below the GPU builder's floor)
    want, e = _check(got, snb, oracle, name, "both", prec, name)
    if name == "NoCutoff":      # the Coulomb energy is homogeneous of degree -1: tr W[s][0] = E[s][0]
        tr = np.abs(got[:, 0, :3].sum(axis=1) - e[:, 0]) / np.maximum(np.abs(e[:, 0]), 1.0)
        print("NoCutoff %s: trace against the oracle's Coulomb energy %.3e" % (prec, tr.max()))
        assert tr.max() < TOLS[prec]
    # a non-periodic system has no box terms: nothing but pairs, whatever the flags
    only = ctx.getSliceVirials(force, includeReciprocal=False)
    assert svt.ratios(only, got, e).max() < SAME_STEP[prec]


# ---- 4. subset counts -------------------------------------------------------------------------------------------------------------------
def test_nine_subsets_one_of_them_empty(snb, oracle):
    ctx, kern, force = _ctx(snb, "nine", "double")
    got = ctx.getSliceVirials(force)
    assert got.shape == (45, 2, 6)
    _check(got, snb, oracle, "nine", "both", "double", "9 subsets")
    held = {force.getParticleSubset(i) for i in range(600)}
    assert 4 not in held and len(held) >= 7      # (the 600 lattice sites stop short of the last slab: subset 8 has no atoms either)
    empty = sorted({svt.slice_index(i, j) for i in range(9) if i not in held for j in range(9)})
    assert not got[empty].any()      # exactly zero
    live = [s for s in range(45) if s not in empty]
    assert (svt.frobenius(got[live, 0]) > 0.0).all()


# ---- 5. frames --------------------------------------------------------------------------------------------------------------------------
def _batch(kern, frames=None, boxes=None, isd=True, dev_in=False, dev_out=False, direct=1, recip=1, states=None, rows=True, n_frames=None, n_states=None,
           state_out=True):
    """One raw snb_evaluate_slice_virials call.  Returns (status, rows [F][S][2][6] or None, states [F][K][6] or None); outputs pre-filled with NaN."""
    import torch
    lib = kern._lib; S = kern.numSlices
    b = importlib.import_module("openmm-nonbonded-slicing_amd").capi.SnbVirialBatch()
    keep = []
    F = 1 if frames is None else len(frames)
    if frames is not None:
        if dev_in:
            d = torch.tensor(np.asarray(frames), dtype=torch.float64 if isd else torch.float32, device="cuda"); keep.append(d)
            b.positions = d.data_ptr(); b.is_device = 1
        else:
            h = np.ascontiguousarray(frames, dtype=np.float64 if isd else np.float32); keep.append(h)
            b.positions = h.ctypes.data_as(ctypes.c_void_p); b.is_device = 0
    b.is_double = int(isd); b.stride4 = 0
    b.n_frames = F if n_frames is None else n_frames
    if boxes is not None:
        bx = np.ascontiguousarray(np.asarray(boxes, dtype=np.float64).reshape(-1, 9)); keep.append(bx)
        b.boxes = _dp(bx)
    b.include_direct = direct; b.include_reciprocal = recip
    K = 0 if states is None else len(states)
    b.n_states = K if n_states is None else n_states
    if K:
        lam = np.ascontiguousarray(states, dtype=np.float64); keep.append(lam)
        b.state_lambdas = _dp(lam)
    b.out_is_device = int(dev_out)
    if dev_out:
        out = torch.full((max(F, 1), S, 2, 6), float("nan"), dtype=torch.float64, device="cuda")
        st = torch.full((max(F, 1), max(K, 1), 6), float("nan"), dtype=torch.float64, device="cuda")
        b.slice_virials = out.data_ptr() if rows else None; b.state_virials = st.data_ptr() if (K and state_out) else None
    else:
        out = np.full((max(F, 1), S, 2, 6), np.nan); st = np.full((max(F, 1), max(K, 1), 6), np.nan)
        b.slice_virials = out.ctypes.data_as(ctypes.c_void_p) if rows else None
        b.state_virials = st.ctypes.data_as(ctypes.c_void_p) if (K and state_out) else None
    status = lib.snb_evaluate_slice_virials(kern._h, ctypes.byref(b))
    if status == 0 and dev_out:
        assert lib.snb_synchronize(kern._h) == 0
        out = out.cpu().numpy(); st = st.cpu().numpy()
    return status, (out if rows else None), (st if K else None)


def _frames(pos, count, seed=13):
    rng = np.random.default_rng(seed)
    fr = [pos] + [pos + 0.02 * rng.standard_normal(pos.shape) for _ in range(count - 1)]
    return np.ascontiguousarray(np.stack(fr).astype(np.float32).astype(np.float64))


def _states(S):
    return np.ascontiguousarray(np.stack([np.ones((S, 2)), np.random.default_rng(59).uniform(0.0, 1.0, (S, 2)), np.zeros((S, 2))]))


@pytest.mark.parametrize("prec,dev_in,name", [("double", True, "sparse"), ("single", False, "pme"), ("mixed", True, "sparse")])
def test_four_frames_the_third_in_a_box_of_its_own(prec, dev_in, name, snb, oracle):
    """600 atoms: every frame's list is built in line, on the host.  4096 atoms: the GPU builder, the next frame's list beside the pass."""
    ctx, kern, force = _ctx(snb, name, prec)
    _, pos, box, _ = _system(snb, name)
    isd = prec == "double"
    frames = _frames(pos, 4)
    boxes = np.stack([box, box, box * 1.01, box]); frames[2] *= 1.01
    frames = np.ascontiguousarray(frames.astype(np.float32).astype(np.float64))
    S = kern.numSlices; lam = _states(S)
    if ("frame energies", name) not in _TRUTHS:      # |E_raw| of the scale rule, per frame, from the oracle
        _TRUTHS[("frame energies", name)] = np.stack([oracle.evaluate(force, frames[f], boxes[f])["slice_energies"] for f in range(4)])
    e = _TRUTHS[("frame energies", name)]
    kern._push_frame_state(ctx)
    fs0 = kern.getFrameStats(); n0, b0 = fs0.n_frames, fs0.n_batches
    status, rows, st = _batch(kern, frames, boxes, isd=isd, dev_in=dev_in, states=lam)
    assert status == 0 and np.isfinite(rows).all() and np.isfinite(st).all()
    fs = kern.getFrameStats()
    assert (fs.n_frames, fs.n_batches) == (n0 + 4, b0 + 1) and fs.n_built_beside + fs.n_built_in_line >= 4
    print("%s %s: lists built beside %d, in line %d" % (name, prec, fs.n_built_beside, fs.n_built_in_line))
    # the package's own entry gives the same numbers (host frames as float64: what a double engine reads, and exact for float32-representable ones)
    if isd:
        prows, pst = kern.computeSliceVirialsForFrames(ctx, frames, boxes, lambdaStates=lam)
        assert svt.ratios(prows, rows, e).max() < SAME_STEP[prec]
        assert np.abs(pst - st).max() <= 1e-9 * np.maximum(np.abs(st).max(), 1.0)
    # every row against the current-state call at that frame
    for f in range(4):
        ctx.setPeriodicBoxVectors(*boxes[f]); ctx.setPositions(frames[f])
        now = kern.computeSliceVirials(ctx)
        err = svt.ratios(rows[f], now, e[f]).max()
        print("frame %d %s: row against the current-state call %.3e" % (f, prec, err))
        assert err < SAME_STEP[prec]
    assert svt.ratios(rows[2], rows[0], e[0]).max() > 1e-3      # (the frames differ)
    # the states are the rows contracted, to 1e-12 of the scale
    K = snb.HipCalcSlicedNonbondedForceKernel
    want = K.virialsAtStates(rows, lam)
    scale = np.maximum(np.abs(np.einsum("kst,fstc->fkc", np.abs(lam), np.abs(rows))), 1.0)
    assert (np.abs(st - want) <= 1e-12 * scale).all()
    assert not st[:, 2].any()      # (all lambdas zero)
    # states only
    status, none, st2 = _batch(kern, frames, boxes, isd=isd, dev_in=dev_in, states=lam, rows=False)
    assert status == 0 and none is None
    assert (np.abs(st2 - st) <= SAME_STEP[prec] * scale).all()
    # device output
    status, drows, dst = _batch(kern, frames, boxes, isd=isd, dev_in=dev_in, states=lam, dev_out=True)
    assert status == 0 and np.isfinite(drows).all()
    assert svt.ratios(drows, rows, e).max() < SAME_STEP[prec] and (np.abs(dst - st) <= SAME_STEP[prec] * scale).all()


# ---- 6. the call writes only its outputs ------------------------------------------------------------------------------------------------
def test_call_leaves_forces_outputs_energies_and_timers_alone(snb, oracle):
    """Mixed precision (bitwise reproducible forces).  A forces step with energies into a registered accumulate-mode force output; then the
    call with positions == NULL and a 3-frame batch in another box: snb_get_forces, the force output, the slice-energy buffer (host copy and
    device buffer) and the timer sums are what they were, bit for bit."""
    import torch
    ctx, kern, force = _ctx(snb, "pme", "mixed")
    _, pos, box, _ = _system(snb, "pme")
    L = kern._lib; h = kern._h; n = 600; S = kern.numSlices
    out = torch.full((n, 3), 7.25, dtype=torch.float32, device="cuda")
    assert L.snb_set_force_output(h, ctypes.c_void_p(out.data_ptr()), 0, 1) == 0
    ctx.getState(getEnergy=True, getForces=True)
    assert L.snb_synchronize(h) == 0

    def forces():
        f = torch.zeros((n, 3), dtype=torch.float32, device="cuda")
        assert L.snb_get_forces(h, ctypes.c_void_p(f.data_ptr()), 1, 0, 0) == 0 and L.snb_synchronize(h) == 0
        return f

    def energies():
        e = np.zeros((S, 2)); assert L.snb_get_slice_energies(h, _dp(e)) == 0
        return e

    def timers():
        st = kern.getStats()
        return (st.n_timed, st.sum_direct_ms, st.sum_recip_ms, st.sum_total_ms, list(st.sum_kernel_ms), list(st.n_kernel_timed))
    f_before = forces(); out_before = out.clone(); se_before = energies()
    assert f_before.abs().max() > 1.0 and np.abs(se_before).max() > 1.0 and not torch.equal(out_before, torch.full_like(out, 7.25))
    dev = ctypes.c_void_p(); assert L.snb_slice_energies_device(h, ctypes.byref(dev)) == 0
    dev_before = _device_doubles(dev.value, 2 * S).clone()
    t_before = timers()

    def untouched():
        assert torch.equal(forces(), f_before) and torch.equal(out, out_before)
        assert np.array_equal(energies(), se_before) and torch.equal(_device_doubles(dev.value, 2 * S), dev_before)
        assert timers() == t_before
    now = kern.computeSliceVirials(ctx)
    assert np.isfinite(now).all() and np.abs(now).max() > 1.0
    untouched()
    frames = _frames(pos, 3, seed=29) * 1.005
    rows = kern.computeSliceVirialsForFrames(ctx, frames.astype(np.float32), np.stack([box * 1.005] * 3), lambdaStates=_states(S))[0]
    assert np.isfinite(rows).all() and np.abs(rows).max() > 1.0
    untouched()
    # the context's own state is the caller's again: the same tensor as before the batch
    again = kern.computeSliceVirials(ctx)
    assert svt.ratios(again, now, _truth(snb, oracle, "pme")[1]).max() < SAME_STEP["mixed"]
    untouched()


# ---- 7. a bound context -----------------------------------------------------------------------------------------------------------------
def test_bound_context(snb, oracle):
    import torch
    from test_gpu_context_binding import View
    ctx, kern, force = _ctx(snb, "pme", "single")
    _, pos, box, _ = _system(snb, "pme")
    S = kern.numSlices
    free = kern.computeSliceVirials(ctx)
    v = View(pos, False, 23)
    torch.cuda.synchronize()
    kern.bindContextBuffers(v.posq.data_ptr(), v.atom_index.data_ptr(), v.padded, forceBuffer=v.buf.data_ptr(), posqIsDouble=False)
    ctx.setPositions(np.zeros((600, 3)))      # (the host positions are not used while bound)
    posq0, buf0 = v.posq.clone(), v.buf.clone()
    bound = kern.computeSliceVirials(ctx)
    assert kern._lib.snb_synchronize(kern._h) == 0
    assert torch.equal(v.posq, posq0) and torch.equal(v.buf, buf0)
    err = svt.ratios(bound, free, _truth(snb, oracle, "pme")[1]).max()
    print("bound against unbound: %.3e" % err)
    assert err < SAME_STEP["single"]
    capi = snb.capi
    status, _, _ = _batch(kern, _frames(pos, 2), isd=True)
    assert status == capi.SNB_ERR_STATE and b"context is bound" in kern._lib.snb_last_error(kern._h)
    kern.unbindContextBuffers()


# ---- 8. status codes --------------------------------------------------------------------------------------------------------------------
def test_status_codes(snb, oracle):
    capi = snb.capi
    ctx, kern, force = _ctx(snb, "pme", "single")
    _, pos, box, _ = _system(snb, "pme")
    S = kern.numSlices; lam = _states(S)
    kern._push_state(ctx)
    r0 = kern.getStats().n_rebuilds
    fr = _frames(pos, 2)
    INV = capi.SNB_ERR_INVALID_ARGUMENT
    assert kern._lib.snb_evaluate_slice_virials(kern._h, None) == INV
    assert kern._lib.snb_evaluate_slice_virials(None, ctypes.byref(capi.SnbVirialBatch())) == INV
    assert _batch(kern, rows=False)[0] == INV                                        # both outputs NULL
    assert _batch(kern, fr, rows=False)[0] == INV
    assert _batch(kern, states=lam, n_states=-1)[0] == INV                           # negative n_states
    assert _batch(kern, fr, n_frames=-1)[0] == INV                                   # negative n_frames
    assert _batch(kern, states=lam, state_out=False)[0] == INV                       # states without state_virials
    st, _, _ = _batch(kern, n_states=2)                                              # ... without state_lambdas
    assert st == INV
    assert _batch(kern, direct=0, recip=0)[0] == INV                                 # both include flags 0
    assert _batch(kern, n_frames=2)[0] == INV                                        # positions == NULL: n_frames must be 1
    assert kern.getStats().n_rebuilds == r0      # refused before anything was enqueued
    status, rows, _ = _batch(kern, fr, n_frames=0)
    assert status == 0 and np.isnan(rows).all() and kern.getStats().n_rebuilds == r0      # no frames: no work
    # box errors: those of snb_evaluate_frames, with the frame index
    small = np.stack([box, np.diag([1.5, 3.0, 3.0])])
    assert _batch(kern, fr, small)[0] == capi.SNB_ERR_BOX_TOO_SMALL and b"frame 1" in kern._lib.snb_last_error(kern._h)
    skew = box.copy(); skew[0, 1] = 0.1
    assert _batch(kern, fr, np.stack([skew, box]))[0] == INV and b"frame 0" in kern._lib.snb_last_error(kern._h)
    assert kern.getStats().n_rebuilds == r0
    assert _batch(kern, fr)[0] == 0
    # sharded engines
    cfg = capi.SnbConfig()
    cfg.abi_version = capi.SNB_ABI_VERSION; cfg.n_atoms = 600; cfg.n_subsets = 3; cfg.method = 2; cfg.cutoff = 1.0; cfg.rf_dielectric = 78.3
    cfg.shard_rank = 0; cfg.shard_count = 2
    h = ctypes.c_void_p()
    assert kern._lib.snb_create(ctypes.byref(cfg), ctypes.byref(h)) == capi.SNB_OK
    sharded = types.SimpleNamespace(_lib=kern._lib, _h=h, numSlices=6)
    assert _batch(sharded)[0] == capi.SNB_ERR_UNSUPPORTED and _batch(sharded, fr)[0] == capi.SNB_ERR_UNSUPPORTED
    assert _batch(sharded, direct=0, recip=0)[0] == INV      # (the argument checks come first)
    kern._lib.snb_destroy(h)
    # classic Ewald: the k-sum is refused, direct space works
    ectx, ekern, eforce = _ctx(snb, "ewald", "double")
    ekern._push_state(ectx)
    assert _batch(ekern)[0] == capi.SNB_ERR_UNSUPPORTED and _batch(ekern, recip=1, direct=0)[0] == capi.SNB_ERR_UNSUPPORTED
    with pytest.raises(snb.OpenMMException):
        ectx.getSliceVirials(eforce)
    _check(ectx.getSliceVirials(eforce, includeReciprocal=False), snb, oracle, "ewald", "direct", "double", "classic Ewald")
