"""Shell-sensitive systems of the cutoff-shell census (tests/test_shell_census.py on the CPU, tests/test_gpu_shell_census.py on the GPU).

Why.  Every other parity system here is a PME or reaction-field box whose pair force at the cutoff is 0.1-0.3 kJ/mol/nm while |F| per atom
runs into the thousands: a pair lost, doubled or taken through the wrong image near the cutoff moves an atom by 1e-5 .. 1e-4 of the scale
the 1e-3 bar is taken from.  The systems below use CutoffPeriodic / CutoffNonPeriodic with a reaction-field dielectric of 1 (krf = 0,
crf = 1/rc: plain Coulomb, truncated), charges +-1 and epsilon = 0: a pair at the cutoff pushes with 138.9 kJ/mol/nm, several times the
bar of either of its atoms, so ONE wrong far pair fails the ordinary per-atom comparison -- and the report names it.

Rules of the generator.
 * Float coordinates: every coordinate is rounded to float32 and widened back (as parity_tools.float_positions), so engine and oracle are
   given the same numbers in every precision.
 * Empty truncation band: the potential jumps at the cutoff, so no pair may sit where rounding decides its side.  One atom of every pair with
   |r^2 / rc^2 - 1| < 4 * parity_tools.band_rel is nudged by about 1e-3 nm until orc_cutoff_band_pairs finds none.  The empty band is a
   condition the tests assert, not an allowance: no atom is left out of any comparison.
 * A system is a dict of arrays (no per-particle Python objects): ``oracle_eval`` feeds them to the oracle's C entry point, ``Engine`` to the
   C ABI of include/snb.h.
"""
import ctypes
import hashlib
import os
import sys

import numpy as np

import parity_tools
import systems

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RC = 1.0
K_COULOMB = 138.93545764438198          # ONE_4PI_EPS0, kJ nm / (mol e^2)
TOLS = {"single": 1e-3, "mixed": 1e-3, "double": 1e-5}
SHELL_LO = 0.9                          # the shell is 0.9 rc <= r < rc
MARGIN = 3.0                            # every shell pair must clear MARGIN * tol * max(|Fi|, |Fj|, 1)
TRICLINIC = np.array([[6.0, 0.0, 0.0], [1.5, 6.0, 0.0], [-1.2, 2.0, 6.0]])
# cells with three unequal lengths (every other cell of the suite has one length on all three axes): the sites of their lattices are counted
# per axis so that the spacing is the same along each, 0.2667 nm
ORTHO_LENGTHS = (5.6, 6.4, 7.2)
ORTHO_SITES = (21, 24, 27)
TRICLINIC_UNEQUAL = np.array([[5.6, 0.0, 0.0], [1.4, 6.4, 0.0], [-1.2, 2.0, 7.2]])


def _orc():
    p = os.path.join(ROOT, "oracle")
    if p not in sys.path:
        sys.path.insert(0, p)
    import oracle
    return oracle


def _dp(a): return a.ctypes.data_as(ctypes.POINTER(ctypes.c_double))
def _ip(a): return a.ctypes.data_as(ctypes.POINTER(ctypes.c_int))


def to_float(pos):
    return np.ascontiguousarray(np.asarray(pos, dtype=np.float64).astype(np.float32).astype(np.float64))


# ---- the system record -----------------------------------------------------------------------------------------------------------
def make_system(name, pos, box, q, subset, nsub, rc=RC):
    n = len(q)
    s = dict(name=name, pos=to_float(pos), box=None if box is None else np.ascontiguousarray(box, dtype=np.float64).reshape(3, 3),
             method=1 if box is None else 2, rc=float(rc), nsub=int(nsub), subset=np.ascontiguousarray(subset, dtype=np.int32),
             q=np.ascontiguousarray(q, dtype=np.float64), sigma=np.full(n, 0.3), epsilon=np.zeros(n),
             exc_pairs=np.zeros((0, 2), dtype=np.int32), exc_qq=np.zeros(0), exc_sigma=np.zeros(0), exc_eps=np.zeros(0),
             exceptions_periodic=False, topology="none")
    S = nsub * (nsub + 1) // 2
    s["lam"] = np.ones((S, 2))
    return s


def box9(s):
    return np.ascontiguousarray(np.diag([1e6, 1e6, 1e6]) if s["box"] is None else s["box"], dtype=np.float64).reshape(9)


def _cfg(s, cutoff=None):
    o = _orc()
    cfg = o.OrcConfig()
    cfg.n_atoms = len(s["q"]); cfg.n_subsets = s["nsub"]; cfg.method = s["method"]; cfg.cutoff = s["rc"] if cutoff is None else cutoff
    cfg.rf_dielectric = 1.0; cfg.exceptions_periodic = int(s["exceptions_periodic"])
    cfg.include_direct = 1; cfg.include_reciprocal = 1; cfg.background_term = 1; cfg.correct_q1 = 1
    return cfg


_ORACLE = {}


def oracle_eval(s, cutoff=None, extra=None):
    """(forces [N][3], slice energies [S][2]) of the oracle.  cutoff: another cutoff than the system's.  extra: additional exceptions
    [(i, j, chargeProd)] (the mutations of the CPU tests).  Results are kept for the session, keyed by everything that reaches the oracle."""
    L = _orc().lib()
    cfg = _cfg(s, cutoff)
    pairs, qq, sg, ep = s["exc_pairs"], s["exc_qq"], s["exc_sigma"], s["exc_eps"]
    if extra:
        pairs = np.concatenate([pairs, np.array([[a, b] for a, b, _ in extra], dtype=np.int32).reshape(-1, 2)])
        qq = np.concatenate([qq, np.array([c for _, _, c in extra], dtype=np.float64)])
        sg = np.concatenate([sg, np.full(len(extra), 0.3)]); ep = np.concatenate([ep, np.zeros(len(extra))])
    m = len(qq)
    pairs = np.ascontiguousarray(pairs if m else np.zeros((1, 2)), dtype=np.int32)
    qq, sg, ep = (np.ascontiguousarray(a if m else np.zeros(1), dtype=np.float64) for a in (qq, sg, ep))
    box = box9(s)
    h = hashlib.sha1()
    for a in (s["pos"], box, s["q"], s["subset"], pairs[:m], qq[:m]):
        h.update(np.ascontiguousarray(a).tobytes()); h.update(b"|")
    h.update(bytes(cfg))
    key = h.hexdigest()
    if key not in _ORACLE:
        n = len(s["q"])
        f = np.zeros((n, 3)); se = np.zeros((s["lam"].shape[0], 2))
        rc = L.orc_evaluate(ctypes.byref(cfg), _dp(s["pos"]), _dp(box), _dp(s["q"]), _dp(s["sigma"]), _dp(s["epsilon"]), _ip(s["subset"]), m,
                            _ip(pairs), _dp(qq), _dp(sg), _dp(ep), _dp(np.ascontiguousarray(s["lam"])), None, _dp(f), _dp(se))
        assert rc == 0, rc
        while len(_ORACLE) > 400:
            _ORACLE.pop(next(iter(_ORACLE)))
        _ORACLE[key] = (f, se)
    f, se = _ORACLE[key]
    return f.copy(), se.copy()


# ---- pair sets ---------------------------------------------------------------------------------------------------------------------
def _pairs_between(s, r2lo, r2hi):
    """Non-excluded pairs with r2lo <= r^2 < r2hi (minimum image where periodic): (ij [P][2], r [P], |F| [P]), by the oracle's diagnostic."""
    L = _orc().lib()
    mid = 0.5 * (r2lo + r2hi); rel = (r2hi - r2lo) / (r2hi + r2lo)
    assert 0 < rel <= 0.1, rel
    cfg = _cfg(s, float(np.sqrt(mid)))
    m = len(s["exc_qq"])
    pairs = np.ascontiguousarray(s["exc_pairs"] if m else np.zeros((1, 2)), dtype=np.int32)
    box = box9(s)
    cap = 1 << 18
    while True:
        ij = np.zeros((cap, 2), dtype=np.int32); vals = np.zeros((cap, 4))
        cnt = L.orc_cutoff_band_pairs(ctypes.byref(cfg), _dp(s["pos"]), _dp(box), _dp(s["q"]), _dp(s["sigma"]), _dp(s["epsilon"]), _ip(s["subset"]), m,
                                      _ip(pairs), _dp(np.ascontiguousarray(s["lam"])), float(rel), cap, _ip(ij), _dp(vals))
        assert cnt >= 0, cnt
        if cnt <= cap:
            break
        cap = int(cnt) + 16
    return ij[:cnt].copy(), vals[:cnt, 0].copy(), vals[:cnt, 1].copy()


def band_rel4(s):
    """Relative half-width in r^2 of the band the generator keeps empty: four times parity_tools.band_rel for the system's coordinate range."""
    return 4.0 * parity_tools.band_rel(s, "single")


def band_pairs(s, rc=None):
    """Pairs within the truncation band of the cutoff (the system's, or rc): the set that must be empty."""
    rc = s["rc"] if rc is None else rc
    rel = band_rel4(s)
    return _pairs_between(s, rc * rc * (1.0 - rel), rc * rc * (1.0 + rel))


def pairs_in_range(s, rlo, rhi):
    """Non-excluded pairs with rlo <= r < rhi, in as many calls as the diagnostic's width limit asks for."""
    edges = [rlo * rlo]
    while edges[-1] < rhi * rhi * (1 - 1e-15):
        edges.append(min(rhi * rhi, edges[-1] * 1.2))
    out = [_pairs_between(s, a, b) for a, b in zip(edges[:-1], edges[1:])]
    ij = np.concatenate([o[0] for o in out]); r = np.concatenate([o[1] for o in out]); f = np.concatenate([o[2] for o in out])
    _, first = np.unique(ij[:, 0].astype(np.int64) * len(s["q"]) + ij[:, 1], return_index=True)      # (a pair on a seam of two calls)
    return ij[first], r[first], f[first]


_SHELL = {}


def shell_pairs(s):
    """(ij, r, |F|) of every non-excluded pair in the shell SHELL_LO * rc <= r < rc; kept per system."""
    key = (s["name"], s["topology"], hashlib.sha1(s["pos"].tobytes()).hexdigest())
    if key not in _SHELL:
        _SHELL[key] = pairs_in_range(s, SHELL_LO * s["rc"], s["rc"])
    return _SHELL[key]


def pair_image(s, i, j):
    """(kx, ky, kz): the lattice image of atom j that atom i sees, x_j + kx a + ky b + kz c (zeros without periodicity)."""
    if s["box"] is None:
        return (0, 0, 0)
    b = s["box"]; d = s["pos"][j] - s["pos"][i]
    k2 = -np.floor(d[2] / b[2, 2] + 0.5); d = d + k2 * b[2]
    k1 = -np.floor(d[1] / b[1, 1] + 0.5); d = d + k1 * b[1]
    k0 = -np.floor(d[0] / b[0, 0] + 0.5)
    return (int(k0), int(k1), int(k2))


def clear_band(s, seed=1, radii=None):
    """Nudges one atom of every band pair by about 1e-3 nm, until the band is empty -- around the cutoff, or around every radius of `radii`.
    Returns the number of atoms moved."""
    rng = np.random.default_rng(seed)
    radii = (s["rc"],) if radii is None else radii
    moved = 0
    for _ in range(50):
        ij = np.concatenate([band_pairs(s, rc)[0] for rc in radii])
        if len(ij) == 0:
            return moved
        atoms = np.unique(ij[:, 1])
        s["pos"][atoms] = to_float(s["pos"][atoms] + rng.normal(0.0, 1e-3, (len(atoms), 3)))
        moved += len(atoms)
    raise AssertionError("%s: the truncation band does not empty" % s["name"])


# ---- geometries ----------------------------------------------------------------------------------------------------------------------
def _charges(n, rng):
    return rng.choice([-1.0, 1.0], n)


def _slabs(pos, L, nsub):
    return np.minimum((np.mod(pos[:, 0], L) / L * nsub).astype(int), nsub - 1)


def _lattice(name, n, L, nsub, seed, jitter=0.05):
    rng = np.random.default_rng(seed)
    pos = systems.jittered_lattice(n, L, rng, jitter)
    return make_system(name, pos, np.diag([L, L, L]), _charges(n, rng), _slabs(pos, L, nsub), nsub)


def lattice_sites(sites, lengths, rng, jitter=0.05):
    """mx x my x mz jittered sites in a cell of Lx x Ly x Lz (systems.jittered_lattice assumes a cube); z runs fastest."""
    m = np.asarray(sites); L = np.asarray(lengths, dtype=np.float64)
    g = np.stack(np.meshgrid(np.arange(m[0]), np.arange(m[1]), np.arange(m[2]), indexing="ij"), -1).reshape(-1, 3)
    return (g + 0.5) * (L / m) + rng.uniform(-jitter, jitter, (len(g), 3))


def orthorhombic():
    """13 608 atoms on 21 x 24 x 27 sites in 5.6 x 6.4 x 7.2 nm (52.7 / nm^3), three slab subsets along y: no two faces are the same
    distance apart, and the subset borders run across the sort columns' other axis."""
    rng = np.random.default_rng(111)
    pos = lattice_sites(ORTHO_SITES, ORTHO_LENGTHS, rng)
    sub = np.minimum((np.mod(pos[:, 1], ORTHO_LENGTHS[1]) / ORTHO_LENGTHS[1] * 3).astype(int), 2)
    return make_system("orthorhombic", pos, np.diag(ORTHO_LENGTHS), _charges(len(pos), rng), sub, 3)


def triclinic_unequal():
    """The same lattice sheared with a reduced cell whose three diagonal entries differ."""
    rng = np.random.default_rng(112)
    pos = lattice_sites(ORTHO_SITES, ORTHO_LENGTHS, rng)
    sub = _slabs(pos, ORTHO_LENGTHS[0], 3)
    return make_system("triclinic_unequal", (pos / np.asarray(ORTHO_LENGTHS)) @ TRICLINIC_UNEQUAL, TRICLINIC_UNEQUAL, _charges(len(pos), rng), sub, 3)


def lattice_dense():
    """13 824 atoms, L = 6 nm (64 / nm^3), three slab subsets."""
    return _lattice("lattice_dense", 13824, 6.0, 3, 101)


def lattice_dilute():
    """13 824 atoms, L = 11 nm: few partners per atom, every one of them far."""
    return _lattice("lattice_dilute", 13824, 11.0, 3, 102)


def water_density():
    """24 000 atoms, L = 6.2145 nm (the number density of water), four slab subsets."""
    return _lattice("water_density", 24000, 6.2145, 4, 103)


def blob_in_gas():
    """A dense ball (158 / nm^3: at 200 the largest |F| leaves the weakest shell pair 2.9 bars, under the 3 asked for) in a gas of a few
    dozen scattered atoms, in a 20 nm cell: the sorted order jumps from atom to atom in the gas (a block each) and the sort columns, sized for the
    whole cell, cut the ball into wide thin slabs whose neighbourhoods are published in several chunks."""
    rng = np.random.default_rng(104)
    L, a = 20.0, 0.185
    m = int(np.ceil(2 * 2.5 / a))
    g = (np.stack(np.meshgrid(np.arange(m), np.arange(m), np.arange(m), indexing="ij"), -1).reshape(-1, 3) - 0.5 * (m - 1)) * a
    ball = g[np.linalg.norm(g, axis=1) < 2.4]
    ball = ball + rng.uniform(-0.02, 0.02, ball.shape) + 0.5 * L
    gas = systems.jittered_lattice(64, L, rng, 0.5)
    gas = gas[np.linalg.norm(gas - 0.5 * L, axis=1) > 2.4 + 0.3]
    pos = np.concatenate([ball, gas])
    sub = np.concatenate([np.where(ball[:, 0] < 0.5 * L, 0, 1), np.full(len(gas), 2)])
    return make_system("blob_in_gas", pos, np.diag([L, L, L]), _charges(len(pos), rng), sub, 3)


def sparse_subsets():
    """The three sparse subsets of test_sparse_subsets_stay_on_gpu_builder: scattered single atoms, a hollow shell, a sphere on the box corner."""
    s = _lattice("sparse_subsets", 13824, 6.0, 4, 105)
    n, L, pos = 13824, 6.0, s["pos"]
    sub = np.zeros(n, dtype=np.int32)
    r = np.linalg.norm(pos - 0.5 * L, axis=1)
    sub[(r > 2.2) & (r < 2.6)] = 2
    dc = pos - L * np.round(pos / L)
    sub[np.linalg.norm(dc, axis=1) < 1.3] = 3
    sub[np.arange(n) % 97 == 5] = 1
    s["subset"] = sub
    return s


def triclinic():
    """The jittered lattice sheared with the TRICLINIC cell of the parity tests."""
    rng = np.random.default_rng(106)
    n, L = 13824, 6.0
    pos = systems.jittered_lattice(n, L, rng, 0.05)
    sub = _slabs(pos, L, 3)
    return make_system("triclinic", (pos / L) @ TRICLINIC, TRICLINIC, _charges(n, rng), sub, 3)


def small_box():
    """L = 2.05 nm: host-built lists, per-pair wrap (a pair sees at most one image, but the box is barely two cutoffs wide)."""
    return _lattice("small_box", 600, 2.05, 2, 107)


def tiny(n):
    """n atoms in a 2.4 nm box: 63 (host lists), 64 and 65 (the GPU builder's threshold), 97 (partial blocks)."""
    return _lattice("tiny_%d" % n, n, 2.4, 2, 108 + n, jitter=0.1)


def nonperiodic_cloud():
    """CutoffNonPeriodic, away from the origin."""
    rng = np.random.default_rng(109)
    n, L = 13824, 6.0
    pos = systems.jittered_lattice(n, L, rng, 0.05)
    sub = _slabs(pos, L, 3)
    return make_system("nonperiodic_cloud", pos + np.array([-7.3, 4.1, 12.0]), None, _charges(n, rng), sub, 3)


def unwrapped():
    """A third of the atoms moved by whole box vectors into [-L, 2L]: the engine must wrap them, the pairs are the same."""
    rng = np.random.default_rng(110)
    n, L = 13824, 6.0
    pos = systems.jittered_lattice(n, L, rng, 0.05)
    sub = _slabs(pos, L, 3)
    who = rng.random(n) < 1.0 / 3.0
    shift = rng.integers(-1, 2, (n, 3)) * L
    pos = np.where(who[:, None], pos + shift, pos)
    return make_system("unwrapped", pos, np.diag([L, L, L]), _charges(n, rng), sub, 3)


GEOMETRIES = {
    "lattice_dense": lattice_dense, "lattice_dilute": lattice_dilute, "water_density": water_density, "blob_in_gas": blob_in_gas,
    "sparse_subsets": sparse_subsets, "triclinic": triclinic, "small_box": small_box, "tiny_63": lambda: tiny(63), "tiny_64": lambda: tiny(64),
    "tiny_65": lambda: tiny(65), "tiny_97": lambda: tiny(97), "nonperiodic_cloud": nonperiodic_cloud, "unwrapped": unwrapped, "orthorhombic": orthorhombic, "triclinic_unequal": triclinic_unequal,
}


# ---- topologies ----------------------------------------------------------------------------------------------------------------------
def _min_image(s, d):
    if s["box"] is None:
        return d
    b = s["box"]
    d = d - np.floor(d[:, 2] / b[2, 2] + 0.5)[:, None] * b[2]
    d = d - np.floor(d[:, 1] / b[1, 1] + 0.5)[:, None] * b[1]
    return d - np.floor(d[:, 0] / b[0, 0] + 0.5)[:, None] * b[0]


def _set_exceptions(s, pairs, qq):
    pairs = np.asarray(pairs, dtype=np.int64).reshape(-1, 2)
    lo, hi = pairs.min(axis=1), pairs.max(axis=1)
    _, first = np.unique(lo * len(s["q"]) + hi, return_index=True)          # one exception per pair
    first = np.sort(first)
    s["exc_pairs"] = np.ascontiguousarray(pairs[first], dtype=np.int32); s["exc_qq"] = np.ascontiguousarray(np.asarray(qq, dtype=np.float64)[first])
    s["exc_sigma"] = np.full(len(first), 0.3); s["exc_eps"] = np.zeros(len(first))


def topology_chains(s):
    """The chains of systems.random_box: four consecutive indices, 1-2 and 1-3 excluded, 1-4 scaled."""
    n, q = len(s["q"]), s["q"]
    pairs, qq = [], []
    for a in range(0, n - 3, 4):
        for i, j in ((a, a + 1), (a + 1, a + 2), (a + 2, a + 3), (a, a + 2), (a + 1, a + 3)):
            pairs.append((i, j)); qq.append(0.0)
        pairs.append((a, a + 3)); qq.append(0.8333 * q[a] * q[a + 3])
    _set_exceptions(s, pairs, qq)
    s["topology"] = "chains"


def topology_long(s, seed=7):
    """Long exclusions: excluded pairs at any r < rc -- a share of the shell pairs, pairs closer in, and hub atoms that carry 40 or more
    exclusions each (the builder resolves exclusions per published chunk, in queues of 128)."""
    rng = np.random.default_rng(seed)
    n = len(s["q"])
    ij, _, _ = pairs_in_range(s, SHELL_LO * s["rc"], s["rc"])
    pairs = [ij[rng.choice(len(ij), min(1500, len(ij) // 8), replace=False)]]
    ij2, _, _ = pairs_in_range(s, 0.6 * s["rc"], 0.75 * s["rc"])
    pairs.append(ij2[rng.choice(len(ij2), min(1500, len(ij2) // 8), replace=False)])
    hubs = rng.choice(n, min(24, n // 16), replace=False)
    for h in hubs:
        r = np.linalg.norm(_min_image(s, s["pos"] - s["pos"][h]), axis=1)
        near = np.where((r < s["rc"]) & (r > 0))[0]
        take = near if len(near) <= 56 else rng.choice(near, 56, replace=False)
        pairs.append(np.stack([np.full(len(take), h), take], axis=1))
    pairs = np.concatenate(pairs)
    _set_exceptions(s, pairs, np.zeros(len(pairs)))
    s["topology"] = "long"
    s["hubs"] = hubs


def topology_far14(s, periodic, seed=9):
    """1-4 exceptions with non-zero chargeProd beyond the cutoff (1.0 <= r < 1.6 by minimum image), a share of them across box faces, with
    exceptions_periodic either way (false: the exception is evaluated at the plain difference of the coordinates, whatever the box)."""
    rng = np.random.default_rng(seed)
    n = len(s["q"])
    pairs = []
    for a in rng.choice(n, min(300, n // 4), replace=False):
        dplain = s["pos"] - s["pos"][a]
        d = _min_image(s, dplain)
        r = np.linalg.norm(d, axis=1)
        cand = np.where((r >= 1.0 * s["rc"]) & (r < 1.6 * s["rc"]))[0]
        if len(cand) == 0:
            continue
        crossing = cand[np.linalg.norm(d[cand] - dplain[cand], axis=1) > 0.5]
        pick = crossing if (len(crossing) and rng.random() < 0.5) else cand
        pairs.append((a, int(rng.choice(pick))))
    pairs = np.array(pairs)
    _set_exceptions(s, pairs, 0.5 * s["q"][pairs[:, 0]] * s["q"][pairs[:, 1]])
    s["exceptions_periodic"] = bool(periodic)
    s["topology"] = "far14_periodic" if periodic else "far14_plain"


TOPOLOGIES = {"none": lambda s: None, "chains": topology_chains, "long": topology_long,
              "far14_periodic": lambda s: topology_far14(s, True), "far14_plain": lambda s: topology_far14(s, False)}

_BUILT = {}


def build(geometry, topology="none"):
    """The system of a geometry and a topology, float coordinates, band cleared; built once per session (callers must not modify it)."""
    key = (geometry, topology)
    if key not in _BUILT:
        s = GEOMETRIES[geometry]()
        clear_band(s)                      # (before the topology: an excluded pair in the band would hide from the check, and come back with another topology)
        TOPOLOGIES[topology](s)
        assert len(band_pairs(s)[0]) == 0
        _BUILT[key] = s
    return _BUILT[key]


def build_control(geometry, shrink):
    """The bare system of a geometry with the band empty around rc AND around rc - shrink: for the control in which the engine is given the
    shrunken cutoff and the oracle the full one."""
    key = (geometry, "control", shrink)
    if key not in _BUILT:
        s = GEOMETRIES[geometry]()
        s["name"] += "_control"
        clear_band(s, radii=(s["rc"], s["rc"] - shrink))
        _BUILT[key] = s
    return _BUILT[key]


def trajectory(s, steps, sigma, seed, scales=None):
    """`steps` frames of a seeded walk with normal steps of `sigma` nm per coordinate, starting at the system itself; every frame has float
    coordinates and an empty band.  scales: a box factor per frame (coordinates and box are scaled with it, from the first frame's).
    Returns a list of systems that share everything but pos and box."""
    rng = np.random.default_rng(seed)
    frames = []
    pos = s["pos"].copy()
    for k in range(steps):
        f = dict(s)
        c = 1.0 if scales is None else scales[k]
        f["pos"] = to_float(pos * c)
        if s["box"] is not None:
            f["box"] = s["box"] * c
        f["name"] = "%s_frame%d" % (s["name"], k)
        clear_band(f, seed=seed + 1 + k)
        frames.append(f)
        pos = f["pos"] / c + rng.normal(0.0, sigma, pos.shape)
    return frames


def max_displacement(frames, life):
    """Largest distance an atom covers between two frames at most `life` frames apart (box scales taken out): what a list of that life, built
    at any of the frames, has to absorb in half its skin."""
    worst = 0.0
    unit = [f["pos"] * (frames[0]["box"][0, 0] / f["box"][0, 0] if f["box"] is not None else 1.0) for f in frames]
    for a in range(len(frames)):
        for b in range(a + 1, min(a + life + 1, len(frames))):
            worst = max(worst, float(np.linalg.norm(unit[b] - unit[a], axis=1).max()))
    return worst


# ---- the comparison ------------------------------------------------------------------------------------------------------------------
def compare(s, f, fo, tol, worst=6):
    """The suite's per-atom comparison, |dF| / max(|F|, 1) <= tol with the oracle's |F|, and a report that can be read as pairs: the atoms
    over the bar, and for the worst of them their shell partners with distance and image.  Returns a dict; ``ok`` is the verdict,
    ``flagged`` the sorted atoms over the bar."""
    fn = np.linalg.norm(fo, axis=1)
    err = np.linalg.norm(np.asarray(f) - fo, axis=1) / np.maximum(fn, 1.0)
    flagged = np.where(~(err <= tol))[0]
    rec = {"ok": len(flagged) == 0, "flagged": [int(a) for a in flagged], "max_err": float(np.nanmax(err)) if len(err) else 0.0,
           "median_err": float(np.median(err)), "tol": tol, "system": "%s/%s" % (s["name"], s["topology"]), "worst": []}
    if len(flagged):
        ij, r, fp = shell_pairs(s)
        for a in flagged[np.argsort(-np.nan_to_num(err[flagged], nan=np.inf))][:worst]:
            mine = np.where((ij[:, 0] == a) | (ij[:, 1] == a))[0]
            df = np.asarray(f)[a] - fo[a]
            partners = []
            for k in mine:
                b = int(ij[k, 1] if ij[k, 0] == a else ij[k, 0])
                partners.append({"j": b, "r": float(r[k]), "image": pair_image(s, int(a), b), "pair_force": float(fp[k]),
                                 "flagged": bool(err[b] > tol)})
            partners.sort(key=lambda p: (not p["flagged"], -p["r"]))
            rec["worst"].append({"i": int(a), "err": float(err[a]), "abs_dF": float(np.linalg.norm(df)), "abs_F": float(fn[a]), "shell_partners": partners})
    return rec


def report(rec, partners=4):
    if rec["ok"]:
        return "%s: ok, max %.2e (tol %.0e)" % (rec["system"], rec["max_err"], rec["tol"])
    lines = ["%s: %d atoms over %.0e (max %.2e): %s" % (rec["system"], len(rec["flagged"]), rec["tol"], rec["max_err"], rec["flagged"][:24])]
    for w in rec["worst"]:
        lines.append("  atom %d: err %.2e, |dF| %.3f of |F| %.1f; shell partners (flagged ones first):" % (w["i"], w["err"], w["abs_dF"], w["abs_F"]))
        for p in w["shell_partners"][:partners]:
            lines.append("    pair (%d, %d), r %.7f, image %s, pair force %.2f%s" % (w["i"], p["j"], p["r"], p["image"], p["pair_force"], " [partner flagged too]" if p["flagged"] else ""))
    return "\n".join(lines)


def shell_margins(s, fo, tol):
    """Per shell pair, pair force / (tol * max(|Fi|, |Fj|, 1)): the factor by which losing that pair alone would exceed the bar."""
    ij, r, fp = shell_pairs(s)
    fn = np.maximum(np.linalg.norm(fo, axis=1), 1.0)
    return fp / (tol * np.maximum(fn[ij[:, 0]], fn[ij[:, 1]]))


def gap_atoms(s, fo, shrink, tol, need=2.0, cancelled_below=None):
    """The atoms a cutoff shrunk by `shrink` must move over the bar: those of the pairs with rc - shrink <= r < rc.  Predicted from the
    geometry alone; where an atom has several pairs in the gap their forces are summed (K q q d / r^3), and the prediction only stands if
    every such sum is still worth `need` bars -- two for an engine, which may itself be up to one bar from the oracle; just over one where
    the oracle is compared with itself -- asserted here (cancelled_below: atoms whose pairs in the gap cancel to less than that many bars are
    predicted to stay under the bar and are left out of the returned atoms; only the exact self-comparison of the oracle uses it), so that a gap in which two pairs cancel is never used.  Returns (sorted atoms, pairs [P][2])."""
    ij, r, _ = pairs_in_range(s, s["rc"] - shrink, s["rc"])
    d = _min_image(s, s["pos"][ij[:, 1]] - s["pos"][ij[:, 0]])
    fpair = -K_COULOMB * (s["q"][ij[:, 0]] * s["q"][ij[:, 1]])[:, None] * d / (r ** 3)[:, None]          # on atom i; minus that on atom j
    lost = np.zeros_like(fo)
    np.add.at(lost, ij[:, 0], fpair); np.add.at(lost, ij[:, 1], -fpair)
    atoms = np.unique(ij.ravel())
    bars = np.linalg.norm(lost[atoms], axis=1) / (tol * np.maximum(np.linalg.norm(fo[atoms], axis=1), 1.0))
    if cancelled_below is not None:
        atoms, bars = atoms[bars >= cancelled_below], bars[bars >= cancelled_below]
    assert len(atoms) == 0 or bars.min() >= need, "gap of %g: atom %d keeps %.2f bars only" % (shrink, atoms[bars.argmin()], bars.min())
    return [int(a) for a in atoms], ij


def compare_energies(se, so, tol):
    """Slice energies with the reference's max(|x|, 1) scaling; returns (ok, worst relative error)."""
    err = np.abs(np.asarray(se) - so) / np.maximum(np.abs(so), 1.0)
    return bool((err <= tol).all()), float(err.max())


# ---- the dimer gas -------------------------------------------------------------------------------------------------------------------
DIMER_DELTAS = {"single": (1e-2, 1e-3, 1e-4, 2e-5), "mixed": (1e-2, 1e-3, 1e-4, 2e-5),
                "double": (1e-2, 1e-3, 1e-4, 2e-5, 1e-5, 1e-6, 1e-7, 1e-8, 1e-9)}


def dimer_gas(precision, box=None, seed=77, sites=16, spacing=2.5):
    """Isolated pairs with a closed-form answer: sites^3 dimers (4096: 8192 atoms) on a lattice of centres `spacing` nm apart (more than rc + padding + 1 nm), random
    orientations, separations rc (1 -+ delta) for the deltas of the precision, inside and outside the cutoff in turn.  The lattice starts at
    the origin, so the bonds of the first layer of every axis cross a face, those of the first rows an edge; four dimers around the origin are
    laid along the four body diagonals so that every corner image occurs (they are excluded from one another: the gas stays a gas of pairs).
    Every atom has one partner; its force is K q_i q_j / r^2 along the axis, or exactly zero.  box: None for the cube, or a 3 x 3 reduced
    cell of which the lattice takes the fractional coordinates (the triclinic variant).  Coordinates are float32 values in single and mixed
    precision and full doubles in double precision (the double engine decides in double from double coordinates); r is what the stored
    coordinates give.  Returns the system with ``partner``, ``r``, ``inside``, ``delta`` and ``expected`` forces."""
    rng = np.random.default_rng(seed)
    L = sites * spacing
    cell = np.diag([L, L, L]) if box is None else np.asarray(box, dtype=np.float64)
    deltas = DIMER_DELTAS[precision]
    g = np.stack(np.meshgrid(np.arange(sites), np.arange(sites), np.arange(sites), indexing="ij"), -1).reshape(-1, 3).astype(float)
    centres = (g / sites) @ cell
    nd = len(centres)
    u = rng.normal(size=(nd, 3)); u /= np.linalg.norm(u, axis=1)[:, None]
    # the four corner dimers: site (0,0,0) and three more centres moved next to it, along the body diagonals
    diag = np.array([[1, 1, 1], [1, -1, -1], [-1, 1, -1], [-1, -1, 1]]) / np.sqrt(3.0)
    corner = [0, 1, sites, sites * sites]                  # sites (0,0,0), (0,0,1), (0,1,0), (1,0,0)
    offs = np.array([[0.0, 0.0, 0.0], [0.12, -0.1, 0.15], [-0.14, 0.11, -0.09], [0.1, 0.13, -0.12]])
    for k, d in enumerate(corner):
        centres[d] = offs[k]; u[d] = diag[k]
    which = rng.integers(0, len(deltas), nd); inside = rng.random(nd) < 0.5
    for k, d in enumerate(corner):
        inside[d] = True; which[d] = k % len(deltas)
    delta = np.asarray(deltas)[which]
    target = RC * np.where(inside, 1.0 - delta, 1.0 + delta)
    a = centres - 0.5 * target[:, None] * u; b = centres + 0.5 * target[:, None] * u
    pos = np.concatenate([a, b])
    # wrap into the cell (the bonds that cross a face then need the image)
    frac = pos @ np.linalg.inv(cell)
    pos = (frac - np.floor(frac)) @ cell
    if precision != "double":
        pos = to_float(pos)
    q = np.concatenate([np.ones(nd), -np.ones(nd)])
    like =rng.random(nd) < 0.5                              # half of the dimers repel
    q[nd:][like] = 1.0
    sub = (np.arange(2 * nd) % 2).astype(np.int32)
    s = make_system("dimer_gas_%s%s" % (precision, "" if box is None else "_triclinic"), pos, cell, q, sub, 2)
    if precision == "double":
        s["pos"] = np.ascontiguousarray(pos)                 # (make_system rounds to float)
    ca = np.array(corner)
    cross = [(int(x), int(y)) for i, x in enumerate(np.concatenate([ca, ca + nd])) for y in np.concatenate([ca, ca + nd])[i + 1:] if (x % nd) != (y % nd)]
    _set_exceptions(s, cross, np.zeros(len(cross)))
    s["topology"] = "corner_exclusions"
    partner = np.concatenate([np.arange(nd) + nd, np.arange(nd)])
    d = _min_image(s, s["pos"][partner] - s["pos"])
    r = np.linalg.norm(d, axis=1)
    ins = r < RC
    expected = np.where(ins[:, None], -K_COULOMB * (q * q[partner])[:, None] * d / (r ** 3)[:, None], 0.0)
    # slice energies: both atoms of dimer k are in subset k % 2 (the number of dimers is even), so the pairs fill the two diagonal slices,
    # K q q (1 / r - 1 / rc) each (reaction field with krf = 0, crf = 1 / rc); the cross slice is empty
    epair = np.where(ins[:nd], K_COULOMB * q[:nd] * q[nd:] * (1.0 / r[:nd] - 1.0 / RC), 0.0)
    eslices = np.zeros((3, 2))
    eslices[0, 0] = epair[0::2].sum(); eslices[2, 0] = epair[1::2].sum()
    s.update(partner=partner, r=r, inside=ins, delta=np.concatenate([delta, delta]), expected=expected, intended_inside=np.concatenate([inside, inside]),
             expected_slice_energies=eslices)
    return s


def dimer_images(s):
    """The set of lattice images (kx, ky, kz) under which an atom of the gas sees its partner."""
    b = s["box"]; d = s["pos"][s["partner"]] - s["pos"]
    k2 = -np.floor(d[:, 2] / b[2, 2] + 0.5); d = d + k2[:, None] * b[2]
    k1 = -np.floor(d[:, 1] / b[1, 1] + 0.5); d = d + k1[:, None] * b[1]
    k0 = -np.floor(d[:, 0] / b[0, 0] + 0.5)
    return set(zip(k0.astype(int).tolist(), k1.astype(int).tolist(), k2.astype(int).tolist()))


def compare_dimers(s, f, tol):
    """Per atom against the closed form: zero where the partner is outside the cutoff (exactly), K q q / r^2 along the axis inside.  Returns
    (ok, message); the message names the worst dimers by separation, side and image."""
    f = np.asarray(f); ex = s["expected"]
    err = np.linalg.norm(f - ex, axis=1) / np.maximum(np.linalg.norm(ex, axis=1), 1.0)
    bad = np.where(~np.where(s["inside"], err <= tol, (f == 0).all(axis=1)))[0]
    if len(bad) == 0:
        return True, "%s: ok" % s["name"]
    lines = ["%s: %d atoms wrong" % (s["name"], len(bad))]
    by_delta = {}
    for a in bad:
        by_delta.setdefault((float(s["delta"][a]), bool(s["inside"][a])), []).append(int(a))
    for (dl, ins), atoms in sorted(by_delta.items()):
        a = atoms[0]
        lines.append("  delta %.0e %s the cutoff: %d atoms, e.g. pair (%d, %d), r = rc %+.3e, image %s, got |F| %.4f, expected %.4f"
                     % (dl, "inside" if ins else "outside", len(atoms), a, int(s["partner"][a]), s["r"][a] - RC, pair_image(s, a, int(s["partner"][a])),
                        np.linalg.norm(f[a]), np.linalg.norm(ex[a])))
    return False, "\n".join(lines)


# ---- a thin driver of the C ABI ------------------------------------------------------------------------------------------------------
class Engine:
    """The HIP engine on a system record, through include/snb.h (host arrays in, host arrays out)."""

    def __init__(self, snb, s, precision, padding=0.0, interval=1, host_build=0, rank=0, world=1, cutoff=None):
        self.capi = snb.capi; self.L = snb.capi.lib(); self.h = ctypes.c_void_p(); self.s = s; self.n = len(s["q"])
        cfg = self.capi.SnbConfig()
        cfg.abi_version = self.capi.SNB_ABI_VERSION; cfg.n_atoms = self.n; cfg.n_subsets = s["nsub"]; cfg.method = s["method"]
        cfg.precision = {"single": 0, "double": 1, "mixed": 2}[precision]; cfg.device = 0
        cfg.cutoff = s["rc"] if cutoff is None else cutoff; cfg.rf_dielectric = 1.0; cfg.exceptions_periodic = int(s["exceptions_periodic"])
        cfg.neighbor_padding = padding; cfg.rebuild_interval = interval; cfg.shard_rank = rank; cfg.shard_count = world
        cfg.host_neighbor_build = host_build
        self.configure(cfg)
        self.ok(self.L.snb_create(ctypes.byref(cfg), ctypes.byref(self.h)), create=True)
        ip = lambda a: a.ctypes.data_as(ctypes.POINTER(ctypes.c_int32))
        self.ok(self.L.snb_set_particles(self.h, _dp(s["q"]), _dp(s["sigma"]), _dp(s["epsilon"]), ip(s["subset"])))
        m = len(s["exc_qq"])
        if m:
            self.ok(self.L.snb_set_exceptions(self.h, m, ip(s["exc_pairs"]), _dp(s["exc_qq"]), _dp(s["exc_sigma"]), _dp(s["exc_eps"]), None))
        else:
            self.ok(self.L.snb_set_exceptions(self.h, 0, None, None, None, None, None))
        self.ok(self.L.snb_set_lambdas(self.h, _dp(np.ascontiguousarray(s["lam"]))))
        self.set_frame(s)

    direct, recip = 1, 1          # include_direct, include_reciprocal of every step (tests/recip_systems.py evaluates the reciprocal part alone)

    def configure(self, cfg):
        """Further fields of the snb_config before snb_create (the Ewald / PME parameters of tests/recip_systems.py)."""

    def ok(self, st, create=False):
        if st != 0:
            raise RuntimeError("snb error %d: %s" % (st, (self.L.snb_last_error(None if create else self.h) or b"").decode()))

    def close(self):
        if self.h:
            self.L.snb_destroy(self.h); self.h = ctypes.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def set_frame(self, s):
        """Box and coordinates of a frame (a system record with the same atoms)."""
        if s["box"] is not None:
            self.ok(self.L.snb_set_box(self.h, _dp(box9(s))))
        self._pos = np.ascontiguousarray(s["pos"], dtype=np.float64)
        self.ok(self.L.snb_set_positions(self.h, self._pos.ctypes.data_as(ctypes.c_void_p), 0, 1, 0))

    def set_shard_blocks(self, begin, end, period):
        self.ok(self.L.snb_set_shard_blocks(self.h, int(begin), int(end), int(period)))

    def forces(self):
        out = np.zeros((self.n, 3))
        self.ok(self.L.snb_get_forces(self.h, out.ctypes.data_as(ctypes.c_void_p), 0, 1, 0))
        return out

    def slice_energies(self):
        out = np.zeros((self.s["lam"].shape[0], 2))
        self.ok(self.L.snb_get_slice_energies(self.h, _dp(out)))
        return out

    def step_energy_forces(self):
        """An energy + forces step: (forces, raw slice energies -- the dE/dlambda of every slice --, total energy)."""
        e = ctypes.c_double(0.0)
        self.ok(self.L.snb_execute(self.h, 1, 1, self.direct, self.recip, ctypes.byref(e)))
        return self.forces(), self.slice_energies(), e.value

    def step_forces(self):
        """A forces-only step (the second one onward replays the captured graph)."""
        self.ok(self.L.snb_execute(self.h, 1, 0, self.direct, self.recip, None))
        return self.forces()

    def step_energy_only(self):
        self.ok(self.L.snb_execute(self.h, 0, 1, self.direct, self.recip, None))
        return self.slice_energies()

    def stats(self):
        st = self.capi.SnbStats(); self.ok(self.L.snb_get_stats(self.h, ctypes.byref(st))); return st


# ---- the census: geometry x topology x the precisions it runs in -----------------------------------------------------------------------
# Every geometry with every topology that applies (far14_periodic has no meaning without a periodic box), in all three precisions: the whole
# census costs the GPU suite well under a tenth of its time (docs/MEASUREMENT_LOG.md), so no precision had to be cut on the larger geometries.
_ALL = ("single", "mixed", "double")
CENSUS = [(g, t, _ALL) for g in GEOMETRIES for t in TOPOLOGIES if not (g == "nonperiodic_cloud" and t == "far14_periodic")]
# geometries whose lists the engine builds on the host: fewer than 64 atoms, or a cell narrower than two list radii plus four mean block edges
# (which at 2.4 nm takes a few thousand atoms: the 64-atom threshold itself is only ever met in such cells)
HOST_BUILT = ("small_box", "tiny_63", "tiny_64", "tiny_65", "tiny_97")
