"""Derivative steps (snb_execute with include_energy == 2) of the packed pair kernel: a tile whose slice is wanted (snb_set_energy_slices)
accumulates its own raw energies and reduces them at its end, every other tile takes the forces-only path with no energy state alive
across it (direct.hip, E_TILES).  The cases are the smallest shapes at which that bookkeeping can go wrong; the truth is always the CPU
oracle, never an energy step of the engine, and the tolerances are those of tests/test_gpu_parity.py.

Systems: 3000 atoms as a dense droplet (lattice spacing 0.24 nm, the density of the parity suite's boxes) in the middle of a 14.5 nm cell (cutoff 0.7 nm).
The GPU neighbour builder needs 4 block edges + 2 list radii below the cell edge and sizes a block edge as cbrt(32 V / N) of the whole cell,
so few atoms stay on it only in a roomy cell; the Coulomb mesh is coarse for that cell, which the oracle shares.  Subset labels go by
lattice site, so every 32-atom block faces blocks of every subset and its tile list is a sequence of short slice runs."""
import ctypes

import numpy as np
import pytest

import kat_cases as K
import systems

TOLS = {"single": 1e-3, "mixed": 1e-3}      # as tests/test_gpu_parity.py
N, SIDE, CELL, CUTOFF, MESH = 3000, 3.6, 14.5, 0.7, 48
PME = (2.6283, MESH, MESH, MESH)


def _ip(a):
    return a.ctypes.data_as(ctypes.POINTER(ctypes.c_int32))


def _dp(a):
    return a.ctypes.data_as(ctypes.POINTER(ctypes.c_double))


def site_labels(n, nsub, pair_z=True):
    """Subset of lattice site (ix, iy, iz) of systems.jittered_lattice: (ix + iy + iz // 2) % nsub.  Consecutive indices are neighbours along
    z, so of a bonded chain a, a+1, a+2, a+3 (systems.random_box) the 1-2 pairs lie inside one subset or straddle two, and the 1-3 and
    scaled 1-4 pairs straddle two."""
    m = int(np.ceil(n ** (1.0 / 3.0)))
    g = np.stack(np.meshgrid(np.arange(m), np.arange(m), np.arange(m), indexing="ij"), -1).reshape(-1, 3)[:n]
    return (g[:, 0] + g[:, 1] + (g[:, 2] // 2 if pair_z else g[:, 2])) % nsub


def droplet(F, nsub, method=4, labels=None, ljpme=None, switch=False, box=None, n=N, side=SIDE, cutoff=CUTOFF, pme=PME):
    force, pos, _ = systems.random_box(F, n, nsub, method, side, cutoff, pme=pme, ljpme=ljpme, switch=switch)
    box = np.diag([CELL, CELL, CELL]).astype(float) if box is None else np.asarray(box, dtype=float)
    pos = pos + 0.5 * (box[0, 0] - side)
    labels = site_labels(n, nsub) if labels is None else labels
    for i in range(n):
        force.setParticleSubset(i, int(labels[i]))
    return force, pos, box


class Stepper:
    """One context; derivative steps with any wanted set, straight through the C interface."""

    def __init__(self, snb, force, pos, box, precision, **opts):
        system = snb.System()
        for _ in range(force.getNumParticles()):
            system.addParticle(1.0)
        system.setDefaultPeriodicBoxVectors(*box)
        system.addForce(force)
        self.ctx = snb.Context(system, precision=precision, **opts)
        self.kern = self.ctx._kernelFor(force)
        self.n = force.getNumParticles()
        self.S = self.kern.numSlices
        self.ctx.setPositions(pos)

    def wanted(self, mask):
        mask = np.ascontiguousarray(mask, dtype=np.int32)
        self.kern._check(self.kern._lib.snb_set_energy_slices(self.kern._h, _ip(mask)))

    def step(self, include_forces=1, include_energy=2):
        k = self.kern
        k._push_state(self.ctx)
        k._check(k._lib.snb_execute(k._h, include_forces, include_energy, 1, 1, None))
        f = np.zeros((self.n, 3))
        if include_forces:
            k._check(k._lib.snb_get_forces(k._h, f.ctypes.data_as(ctypes.c_void_p), 0, 1, 0))
        e = np.zeros((self.S, 2))
        k._check(k._lib.snb_get_slice_energies(k._h, _dp(e)))
        return f, e

    def stats(self):
        return self.kern.getStats()


def check_forces(fo, f, tol, what=""):
    err = np.linalg.norm(fo - f, axis=1) / np.maximum(np.linalg.norm(fo, axis=1), 1.0)
    print("%s max force error %.3g (tolerance %g)" % (what, err.max(), tol))
    assert err.max() <= tol, "%s max force error %g at atom %d" % (what, err.max(), int(err.argmax()))


def check_slices(so, e, mask, tol, what=""):
    for s in np.flatnonzero(mask):
        for t in range(2):
            print("%s slice %d term %d: oracle %.9g engine %.9g" % (what, s, t, so[s, t], e[s, t]))
            K.assertEqualTo(so[s, t], e[s, t], tol)


VARIANTS = [
    # name, precision, method, ljpme, switch
    ("single_pme", "single", 4, None, False),
    ("mixed_pme", "mixed", 4, None, False),                              # fixed-point force accumulation
    ("mixed_ljpme", "mixed", 5, (2.6283, 24, 24, 24), False),
    ("mixed_pme_switch", "mixed", 4, None, True),
]


@pytest.fixture(scope="module")
def F(snb):
    return snb.SlicedNonbondedForce


@pytest.fixture(scope="module")
def oev(oracle):
    def _o(force, positions, box, parameters=None):
        return oracle.evaluate(force, np.asarray(positions, dtype=float), box, parameters, True, True)
    return _o


_TRUTH = {}


def truth(oev, key, force, pos, box, params):
    """The oracle's answer for a system of this module, computed once and shared (never modified)."""
    if key not in _TRUTH:
        o = oev(force, pos, box, params)
        o["forces"].setflags(write=False); o["slice_energies"].setflags(write=False)
        _TRUTH[key] = o
    return _TRUTH[key]


@pytest.mark.gpu
@pytest.mark.parametrize("variant", VARIANTS, ids=[v[0] for v in VARIANTS])
def test_wanted_and_unwanted_tiles_alternate_and_wanted_tiles_carry_masks(variant, snb, F, oev):
    """Four subsets by lattice site: each block's list alternates between wanted and unwanted slices, run after run.  The wanted set is
    every other slice, then the others, so that each of the ten slices -- the four diagonal ones, whose tiles (the block's own among them)
    carry exclusion masks, and the six that the bonded and the scaled 1-4 pairs straddle -- is checked once as wanted and the forces twice."""
    name, prec, method, ljpme, switch = variant
    force, pos, box = droplet(F, 4, method=method, ljpme=ljpme, switch=switch)
    st = Stepper(snb, force, pos, box, prec)
    o = truth(oev, name[name.index("_") + 1:], force, pos, box, dict(st.ctx.getParameters()))
    for first in (0, 1):
        mask = np.zeros(st.S, dtype=np.int32); mask[first::2] = 1
        st.wanted(mask)
        f, e = st.step()
        check_forces(o["forces"], f, TOLS[prec], "wanted %d::2" % first)
        check_slices(o["slice_energies"], e, mask, TOLS[prec], "wanted %d::2" % first)
    s = st.stats()
    assert s.n_tiles > 0 and s.n_host_rebuilds == 0


@pytest.mark.gpu
def test_wanted_tile_ends_an_item_is_an_item_and_is_padded(snb, F, oev):
    """Subset 3 is 37 scattered atoms: two blocks, the second with 5 atoms and 27 padding slots.  The sorted order goes by subset first, so
    the tiles against subset 3 come last in the lists that hold any, the lists of the two subset-3 blocks are one or two tiles long, and every
    tile with the second block on either side is partial.  Wanted: the slices with subset 3, one at a time and together; padding slots must
    add nothing."""
    labels = site_labels(N, 3)
    labels[np.arange(N) % 83 == 7] = 3
    assert (labels == 3).sum() == 37
    force, pos, box = droplet(F, 4, labels=labels)
    st = Stepper(snb, force, pos, box, "single")
    o = truth(oev, "sparse3", force, pos, box, dict(st.ctx.getParameters()))
    with3 = sorted(snb.sliceIndex(a, 3) for a in range(4))
    assert len(set(with3)) == 4
    sets = [[s] for s in with3] + [with3]
    for want in sets:
        mask = np.zeros(st.S, dtype=np.int32); mask[want] = 1
        st.wanted(mask)
        f, e = st.step()
        check_forces(o["forces"], f, TOLS["single"], "wanted %s" % want)
        check_slices(o["slice_energies"], e, mask, TOLS["single"], "wanted %s" % want)
    s = st.stats()
    assert s.n_tiles > 0 and s.n_host_rebuilds == 0


@pytest.mark.gpu
def test_no_slice_wanted_writes_no_energy(snb, F, oev):
    """Empty wanted set: the forces are the oracle's, as a forces-only step's are, and the tile kernel adds nothing to the energy partitions --
    the slice energies read back are those of an energy-only step on the same empty set (closed-form terms alone), bit for bit."""
    force, pos, box = droplet(F, 4)
    st = Stepper(snb, force, pos, box, "single")
    o = truth(oev, "pme", force, pos, box, dict(st.ctx.getParameters()))
    st.wanted(np.zeros(st.S, dtype=np.int32))
    _, base = st.step(include_forces=0)
    f, e = st.step()
    check_forces(o["forces"], f, TOLS["single"], "nothing wanted")
    print("energy-only step, empty set:", base.ravel()); print("derivative step, empty set:", e.ravel())
    assert np.array_equal(base, e)
    f0, _ = st.step(include_energy=0)
    check_forces(o["forces"], f0, TOLS["single"], "forces only")
    s = st.stats()
    assert s.n_tiles > 0 and s.n_host_rebuilds == 0


@pytest.mark.gpu
def test_all_slices_wanted_per_tile_against_oracle(snb, F, oev):
    """include_energy == 2 with every slice wanted: each tile reduces its own sums (against one reduction per run of tiles on energy
    steps); every raw slice energy must be the oracle's."""
    force, pos, box = droplet(F, 4)
    st = Stepper(snb, force, pos, box, "single")
    o = truth(oev, "pme", force, pos, box, dict(st.ctx.getParameters()))
    mask = np.ones(st.S, dtype=np.int32)
    st.wanted(mask)
    f, e = st.step()
    check_forces(o["forces"], f, TOLS["single"], "all wanted")
    check_slices(o["slice_energies"], e, mask, TOLS["single"], "all wanted")
    assert st.stats().n_host_rebuilds == 0


@pytest.mark.gpu
def test_wanted_set_changes_between_replayed_steps(snb, F, oev):
    """The wanted set lives in device memory the kernel reads: changed between two steps of the same captured graph, with no rebuild in
    between, the second step's energies follow the new set."""
    force, pos, box = droplet(F, 4)
    st = Stepper(snb, force, pos, box, "single", neighbor_padding=0.1, rebuild_interval=100)
    o = truth(oev, "pme", force, pos, box, dict(st.ctx.getParameters()))
    a = np.zeros(st.S, dtype=np.int32); a[[1, 3, 4]] = 1
    b = np.zeros(st.S, dtype=np.int32); b[[0, 2, 4, 9]] = 1
    st.wanted(a)
    for _ in range(3):      # (the first step is eager, the next ones replay its graph)
        f, e = st.step()
    check_slices(o["slice_energies"], e, a, TOLS["single"], "set a")
    rebuilds = st.stats().n_rebuilds
    st.wanted(b)
    f, e = st.step()
    check_forces(o["forces"], f, TOLS["single"], "set b")
    check_slices(o["slice_energies"], e, b, TOLS["single"], "set b")
    st.wanted(a)
    f, e = st.step()
    check_slices(o["slice_energies"], e, a, TOLS["single"], "set a again")
    s = st.stats()
    assert s.n_rebuilds == rebuilds and s.n_host_rebuilds == 0


@pytest.mark.gpu
def test_small_triclinic_cell(snb, F, oev):
    """A small triclinic cell (per-pair wrapping: the scalar tile kernel, which keeps its run-based bookkeeping) under the same alternating
    wanted sets."""
    n, L = 1500, 2.6
    box = np.array([[L, 0, 0], [0.3, L, 0], [-0.2, 0.4, L]])
    force, pos, _ = systems.random_box(F, n, 3, 4, L, 1.0, pme=(2.6283, 24, 24, 24))
    labels = site_labels(n, 3)
    for i in range(n):
        force.setParticleSubset(i, int(labels[i]))
    st = Stepper(snb, force, pos, box, "single")
    o = truth(oev, "triclinic", force, pos, box, dict(st.ctx.getParameters()))
    for first in (0, 1):
        mask = np.zeros(st.S, dtype=np.int32); mask[first::2] = 1
        st.wanted(mask)
        f, e = st.step()
        check_forces(o["forces"], f, TOLS["single"], "wanted %d::2" % first)
        check_slices(o["slice_energies"], e, mask, TOLS["single"], "wanted %d::2" % first)


def _selected_kernels(snb):
    import test_host_cpu
    notes = test_host_cpu._device_kernel_notes(snb)
    if notes is None:
        pytest.skip("ROCm binutils not installed")
    return notes, {n: v for n, v in notes.items() if n.startswith("void k_directPackedSelected<")}


def test_selected_kernels_use_no_scratch(snb):
    """Host side, from the built code object's metadata (as test_host_cpu.py::test_hot_kernels_use_no_scratch): the per-tile derivative
    kernels report no private segment and no spilled registers, and stay at four waves per SIMD."""
    notes, sel = _selected_kernels(snb)
    print(sorted(sel.items()))
    assert len(sel) == 10, sorted(sel)      # NoCutoff (1 x FIXED), reaction field and Ewald (POLY x FIXED each); not LJPME, not the switching function
    assert not {n: v for n, v in sel.items() if v[0] > 0 or v[2] > 0 or v[1] > 128}, sel


def test_selected_kernel_stays_within_eight_registers_of_the_forces_kernel(snb):
    """The benchmark's instantiations (PME, polynomial Ewald): at most 8 registers more than the forces-only kernel they shadow (115 against
    108 in this build; 119 while the i-atoms' 64-bit index and the work counters' per-lane address were held across the tile loop)."""
    notes, sel = _selected_kernels(snb)
    for fixed in ("false", "true"):
        forces = notes["void k_directPacked<2, true, false, false, %s>" % fixed]
        mine = sel["void k_directPackedSelected<2, true, %s>" % fixed]
        print("PME, FIXED = %s: forces-only %d registers, selected %d" % (fixed, forces[1], mine[1]))
        assert mine[1] <= forces[1] + 8, (mine, forces)
