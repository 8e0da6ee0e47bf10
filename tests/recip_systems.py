"""Systems and comparison of the reciprocal-space census (tests/test_recip_census.py on the CPU, tests/test_gpu_recip_census.py on the GPU).

Why.  (1) Every rectangular cell of the other tests is a cube, and the one triclinic cell has the same length on its three diagonal entries:
taking nx where ny belongs, or box[0] where box[4] belongs, passes all of them.  The reference's own tests are cubic too -- its Reference PME
indexes wrongly when nx != nz (Quirk Q1) -- so cell shape is where PME code is known to go wrong.  (2) The reciprocal kernels are
only ever judged inside the total force, at 1e-3 of max(|F_total|, 1) with |F_total| in the thousands to tens of thousands against a
reciprocal part of about a thousand: an error of 1 .. 6 % of an atom's reciprocal force passes.

So the systems below have three unequal cell lengths (and meshes of three unequal sizes), and the engine is evaluated with include_direct = 0,
include_reciprocal = 1 against the oracle evaluated the same way.

The comparison.  Slice energies: |dE| <= tol max(|E_oracle|, 1), reciprocal-only, every slice, both terms.  Forces: every atom,
|dF_i| <= tol max(|F_rec,i|, F_med), where F_med is the oracle's median reciprocal force magnitude over the atoms that carry a charge (or, with
LJPME, a c6).  The floor is not 1: the rounding noise of a float mesh is common to all atoms and follows the field, not one atom's net force
(tests/test_gpu_fullsize.py: median 1e-5 .. 3e-5 of the force, worst atom of 1e6 on a 180^3 mesh 0.027 on 215), so an atom whose reciprocal
force happens to cancel would fail a per-atom relative bar with nothing wrong.  F_med comes from the oracle alone and is printed with every case.

A system is a dict of arrays like those of shell_systems.py, with the Ewald / PME parameters beside them."""
import ctypes
import hashlib

import numpy as np

import shell_systems as S

TOLS = S.TOLS
ALPHA = 2.6283
ORTHO_GRID, ORTHO_DGRID_TILING, ORTHO_DGRID_FALLBACK = (40, 54, 48), (24, 27, 24), (20, 27, 24)


def sl(i, j):
    return max(i, j) * (max(i, j) + 1) // 2 + min(i, j)


# ---- the system record -------------------------------------------------------------------------------------------------------------
def _particles(n, rng):
    """Charges and LJ parameters as systems.random_box draws them."""
    q = rng.uniform(0.2, 0.8, n) * rng.choice([-1.0, 1.0], n)
    q -= q.mean()
    return q, rng.uniform(0.25, 0.35, n), rng.uniform(0.2, 1.0, n)


def _lambdas(nsub):
    """(Coulomb, vdW) per slice: none of the off-diagonal slices at 1, one Coulomb value 0."""
    lam = np.ones((nsub * (nsub + 1) // 2, 2))
    vals = [0.0, 0.9, 0.7, 0.3, 0.45, 0.6, 0.8, 0.4, 0.95, 0.5]
    k = 0
    for i in range(nsub):
        for j in range(i):
            lam[sl(i, j)] = (vals[k % 10], vals[(k + 1) % 10]); k += 2
    if nsub == 1:
        lam[0] = (0.7, 0.9)
    return lam


def _slabs(pos, axis, length, nsub):
    return np.minimum((np.mod(pos[:, axis], length) / length * nsub).astype(int), nsub - 1)


def make(name, pos, box, method, nsub, subset, rng, grid=(0, 0, 0), dgrid=(0, 0, 0), kmax=(0, 0, 0), chains=True):
    n = len(pos)
    q, sig, eps = _particles(n, rng)
    s = S.make_system(name, pos, box, q, subset, nsub)
    s.update(method=method, sigma=sig, epsilon=eps, alpha=ALPHA, alpha_d=ALPHA, grid=tuple(grid), dgrid=tuple(dgrid), kmax=tuple(kmax), lam=_lambdas(nsub))
    if chains:          # the chains of systems.random_box (1-2 and 1-3 excluded, 1-4 scaled): they matter to the full step only
        S.topology_chains(s)
    return s


def carriers(s):
    """The atoms that put something on a mesh: a charge, or with LJPME a c6."""
    c = s["q"] != 0
    return c | (s["epsilon"] != 0) if s["method"] == 5 else c


# ---- the systems ---------------------------------------------------------------------------------------------------------------------
def ortho(method=4, dgrid=(0, 0, 0), name="ortho"):
    """21 x 24 x 27 = 13 608 atoms in 5.6 x 6.4 x 7.2 nm, PME 40 x 54 x 48 (sort columns 8 x 9 of 5 x 6 cells), three subset slabs along y."""
    rng = np.random.default_rng(201)
    pos = S.lattice_sites(S.ORTHO_SITES, S.ORTHO_LENGTHS, rng)
    return make(name, pos, np.diag(S.ORTHO_LENGTHS), method, 3, _slabs(pos, 1, S.ORTHO_LENGTHS[1], 3), rng, ORTHO_GRID, dgrid)


def ortho_ljpme_tiling():
    """LJPME, dispersion mesh 24 x 27 x 24: 3 x 3 cells per sort column, bricks of 2 x 3 columns."""
    return ortho(5, ORTHO_DGRID_TILING, "ortho_ljpme_tiling")


def ortho_ljpme_fallback():
    """LJPME, dispersion mesh 20 x 27 x 24: 20 cells do not tile 8 columns, the dispersion mesh is spread with global atomics."""
    return ortho(5, ORTHO_DGRID_FALLBACK, "ortho_ljpme_fallback")


def ortho_small():
    """7 x 9 x 10 = 630 atoms in 2.05 x 2.6 x 3.3 nm, mesh 20 x 25 x 32: host-built lists, per-pair wrap."""
    rng = np.random.default_rng(202)
    L = (2.05, 2.6, 3.3)
    pos = S.lattice_sites((7, 9, 10), L, rng)
    return make("ortho_small", pos, np.diag(L), 4, 2, _slabs(pos, 1, L[1], 2), rng, (20, 25, 32))


def triclinic_unequal(method=4):
    """The lattice of `ortho` sheared with a reduced cell whose diagonal is 5.6, 6.4, 7.2.  The GPU builder cuts sort columns in fractional
    coordinates, so there the meshes get bricks like those of `ortho`; only the host builder leaves a cell that is not rectangular without
    sort columns, and its meshes to the spreader with global atomics (pme.hip launchPmeSpread's fallback) -- the census runs this system on
    both builders (FORCED_HOST)."""
    rng = np.random.default_rng(203)
    pos = S.lattice_sites(S.ORTHO_SITES, S.ORTHO_LENGTHS, rng)
    sub = _slabs(pos, 1, S.ORTHO_LENGTHS[1], 3)
    return make("triclinic_unequal" + ("_ljpme" if method == 5 else ""), (pos / np.asarray(S.ORTHO_LENGTHS)) @ S.TRICLINIC_UNEQUAL, S.TRICLINIC_UNEQUAL, method, 3, sub, rng,
                ORTHO_GRID, ORTHO_DGRID_TILING if method == 5 else (0, 0, 0))


def ortho_ewald():
    """10 x 12 x 13 = 1560 atoms in 2.4 x 2.8 x 3.2 nm, classic Ewald with kmax = (7, 9, 11)."""
    rng = np.random.default_rng(204)
    L = (2.4, 2.8, 3.2)
    pos = S.lattice_sites((10, 12, 13), L, rng)
    return make("ortho_ewald", pos, np.diag(L), 3, 3, _slabs(pos, 1, L[1], 3), rng, kmax=(7, 9, 11))


def long_z():
    """6 x 6 x 64 = 2304 atoms in 3.0 x 3.25 x 31.2 nm, mesh 25 x 25 x 260: a z line of more than 256 points, which the planner of the own-atoms spreader
    declines (csrc/pme_plan.h ownSpread): the scanning brick spreader runs.  Bricks
    of 260 points fit the spreader's LDS only as 5 x 5 columns, and 25 is the one legal size whose only divisor from 5 to 16 is 5: nx = ny here,
    over unequal lengths."""
    rng = np.random.default_rng(205)
    L = (3.0, 3.25, 31.2)
    pos = S.lattice_sites((6, 6, 64), L, rng, jitter=0.1)
    return make("long_z", pos, np.diag(L), 4, 2, _slabs(pos, 2, L[2], 2), rng, (25, 25, 260))


def blob():
    """The dense ball in a gas of shell_systems.blob_in_gas (20 nm cell) with these charges under PME, mesh 60 x 64 x 72: crowded bricks and
    empty ones.  No LJ, as there: the ball is packed at 0.185 nm."""
    g = S.blob_in_gas()
    rng = np.random.default_rng(206)
    s = make("blob", g["pos"], g["box"], 4, 3, g["subset"], rng, (60, 64, 72), chains=False)
    s["epsilon"] = np.zeros(len(s["q"]))
    return s


def unwrapped():
    """`ortho` with every atom moved by up to +-3 lattice vectors per axis."""
    s = ortho(name="unwrapped")
    rng = np.random.default_rng(207)
    s["pos"] = S.to_float(s["pos"] + rng.integers(-3, 4, s["pos"].shape) * np.asarray(S.ORTHO_LENGTHS))
    return s


def on_mesh_values(length):
    """0.0, -0.0, the float32 next below L, and -1e-7 .. -1e-9 nm."""
    return [0.0, -0.0, float(np.nextafter(np.float32(length), np.float32(0.0))), -1e-7, -1e-8, -1e-9]


def on_mesh():
    """`ortho` with every ninth atom snapped to a node of the mesh, and eighteen atoms of the first lattice layer of an axis with that
    coordinate at 0.0, -0.0, the float32 next below L or just under zero (each value on each axis; the atoms are two sites apart).  Those
    eighteen lose their LJ term: moved onto a face they may sit within 0.06 nm of the atom across it."""
    s = ortho(name="on_mesh")
    L = np.asarray(S.ORTHO_LENGTHS); h = L / np.asarray(ORTHO_GRID); m = S.ORTHO_SITES
    pos = s["pos"].copy()
    pos[::9] = np.round(pos[::9] / h) * h
    special = []
    for d in range(3):
        for j, v in enumerate(on_mesh_values(L[d])):
            site = [2 * j + 1, 2 * j + 1, 2 * j + 1]; site[d] = 0; site[(d + 1) % 3] = 3 + 2 * d
            k = (site[0] * m[1] + site[1]) * m[2] + site[2]
            pos[k, d] = v; s["epsilon"][k] = 0.0
            special.append(k)
    s["special"] = np.array(special)
    assert len(set(special)) == 18
    s["pos"] = np.ascontiguousarray(pos.astype(np.float32).astype(np.float64))
    return s


def subsets5():
    """`ortho` in five subsets: 0 and 1 ordinary slabs, 2 a slab whose charges are all 0, 3 without atoms, 4 a single atom."""
    s = ortho(name="subsets5")
    sub = _slabs(s["pos"], 1, S.ORTHO_LENGTHS[1], 3).astype(np.int32)
    s["q"] = np.where(sub == 2, 0.0, s["q"])
    sub[int(np.where(sub == 0)[0][100])] = 4
    s["subset"] = np.ascontiguousarray(sub); s["nsub"] = 5; s["lam"] = _lambdas(5)
    return s


SYSTEMS = {
    "ortho": ortho, "ortho_ljpme_tiling": ortho_ljpme_tiling, "ortho_ljpme_fallback": ortho_ljpme_fallback, "ortho_small": ortho_small,
    "triclinic_unequal": triclinic_unequal, "triclinic_unequal_ljpme": lambda: triclinic_unequal(5), "ortho_ewald": ortho_ewald, "long_z": long_z,
    "blob": blob, "unwrapped": unwrapped, "on_mesh": on_mesh, "subsets5": subsets5,
}
# systems whose lists the engine builds on the host: a cell narrower than two list radii plus four mean block edges
HOST_BUILT = ("ortho_small", "ortho_ewald", "long_z")
# systems the GPU census also runs with host_neighbor_build = 1: a cell that is not rectangular gets no sort columns from the host builder, so
# both meshes reach the spreader with global atomics
FORCED_HOST = ("triclinic_unequal", "triclinic_unequal_ljpme")
_BUILT = {}


def build(name):
    """The system, built once per session (callers must not modify it)."""
    if name not in _BUILT:
        _BUILT[name] = SYSTEMS[name]()
    return _BUILT[name]


def gpu_builder_applies(s, padding):
    """The engine's own rule (engine.hip gpuRebuild): every cell length must exceed four mean block edges plus two list radii."""
    b = s["box"]
    a = np.cbrt(32.0 * b[0, 0] * b[1, 1] * b[2, 2] / len(s["q"]))
    return len(s["q"]) >= 64 and all(4.0 * a + 2.0 * (s["rc"] + padding) < b[d, d] for d in range(3))


def permuted(s, k):
    """The system with its axes permuted cyclically: new axis d is old axis (d + k) % 3 -- positions, cell, meshes, kmax."""
    assert np.count_nonzero(s["box"] - np.diag(np.diagonal(s["box"]))) == 0
    p = [(d + k) % 3 for d in range(3)]
    t = dict(s)
    t["name"] = "%s_perm%d" % (s["name"], k)
    t["pos"] = np.ascontiguousarray(s["pos"][:, p]); t["box"] = np.diag(np.diagonal(s["box"])[p])
    for key in ("grid", "dgrid", "kmax"):
        t[key] = tuple(s[key][d] for d in p)
    return t


def permuted_back(f, k):
    out = np.empty_like(f)
    out[:, [(d + k) % 3 for d in range(3)]] = f
    return out


# ---- the oracle ------------------------------------------------------------------------------------------------------------------------
_ORACLE = {}


def oracle_eval(s, direct=False, recip=True):
    """(forces [N][3], raw slice energies [S][2]) of the oracle, by default of the reciprocal part alone; kept for the session."""
    o = S._orc(); L = o.lib()
    cfg = o.OrcConfig()
    cfg.n_atoms = len(s["q"]); cfg.n_subsets = s["nsub"]; cfg.method = s["method"]; cfg.cutoff = s["rc"]; cfg.rf_dielectric = 1.0
    cfg.alpha = s["alpha"]; cfg.alpha_d = s["alpha_d"]
    for d in range(3):
        cfg.grid[d] = s["grid"][d]; cfg.dgrid[d] = max(s["dgrid"][d], 1); cfg.kmax[d] = s["kmax"][d]
    cfg.exceptions_periodic = int(s["exceptions_periodic"])
    cfg.include_direct = int(direct); cfg.include_reciprocal = int(recip); cfg.background_term = 1; cfg.correct_q1 = 1
    m = len(s["exc_qq"])
    pairs = np.ascontiguousarray(s["exc_pairs"] if m else np.zeros((1, 2)), dtype=np.int32)
    qq, sg, ep = (np.ascontiguousarray(a if m else np.zeros(1), dtype=np.float64) for a in (s["exc_qq"], s["exc_sigma"], s["exc_eps"]))
    pos = np.ascontiguousarray(s["pos"], dtype=np.float64); box = S.box9(s); lam = np.ascontiguousarray(s["lam"], dtype=np.float64)
    q, sig, eps = (np.ascontiguousarray(s[k], dtype=np.float64) for k in ("q", "sigma", "epsilon"))
    sub = np.ascontiguousarray(s["subset"], dtype=np.int32)
    h = hashlib.sha1()
    for a in (pos, box, q, sig, eps, sub, pairs[:m], qq[:m], sg[:m], ep[:m], lam):
        h.update(a.tobytes()); h.update(b"|")
    h.update(bytes(cfg))
    key = h.hexdigest()
    if key not in _ORACLE:
        f = np.zeros((len(q), 3)); se = np.zeros((lam.shape[0], 2))
        rc = L.orc_evaluate(ctypes.byref(cfg), S._dp(pos), S._dp(box), S._dp(q), S._dp(sig), S._dp(eps), S._ip(sub), m, S._ip(pairs), S._dp(qq), S._dp(sg), S._dp(ep),
                            S._dp(lam), None, S._dp(f), S._dp(se))
        assert rc == 0, rc
        while len(_ORACLE) > 200:
            _ORACLE.pop(next(iter(_ORACLE)))
        _ORACLE[key] = (f, se)
    f, se = _ORACLE[key]
    return f.copy(), se.copy()


# ---- the comparison --------------------------------------------------------------------------------------------------------------------
def force_floor(s, fo):
    """F_med: the median reciprocal force magnitude of the oracle over the atoms that carry a charge (or a c6)."""
    return float(np.median(np.linalg.norm(fo, axis=1)[carriers(s)]))


def compare(s, f, fo, tol, leave_out=()):
    """|dF_i| <= tol max(|F_rec,i|, F_med) on every atom (leave_out: atoms a planted defect removed on purpose).  fo: the oracle's
    reciprocal-only forces.  Returns a dict; ``ok`` is the verdict, ``flagged`` the sorted atoms over the bar."""
    fn = np.linalg.norm(fo, axis=1)
    floor = force_floor(s, fo)
    df = np.linalg.norm(np.asarray(f) - fo, axis=1)
    err = df / np.maximum(fn, floor)
    bad = ~(err <= tol)
    bad[list(leave_out)] = False
    flagged = np.where(bad)[0]
    w = int(np.nanargmax(np.where(np.isnan(err), np.inf, err)))
    return {"ok": len(flagged) == 0, "flagged": [int(a) for a in flagged], "max_err": float(err[w]), "median_err": float(np.median(err)), "floor": floor,
            "worst_atom": w, "worst_dF": float(df[w]), "worst_F": float(fn[w]), "tol": tol, "system": s["name"], "err": err}


def report(rec):
    return "%s: F_med %.1f, worst %.2e (atom %d: |dF| %.4f of |F_rec| %.1f), median %.2e, %d atoms over %.0e%s" % (
        rec["system"], rec["floor"], rec["max_err"], rec["worst_atom"], rec["worst_dF"], rec["worst_F"], rec["median_err"], len(rec["flagged"]), rec["tol"],
        (": %s" % rec["flagged"][:16]) if rec["flagged"] else "")


def compare_total(s, f, fo, tol):
    """The suite's rule for a full step: |dF| <= tol max(|F_total|, 1)."""
    err = np.linalg.norm(np.asarray(f) - fo, axis=1) / np.maximum(np.linalg.norm(fo, axis=1), 1.0)
    return bool((err <= tol).all()), float(np.nanmax(err)), int(np.nanargmax(err))


compare_energies = S.compare_energies


# ---- the engine ----------------------------------------------------------------------------------------------------------------------
class Engine(S.Engine):
    """shell_systems.Engine with the Ewald / PME parameters of the record; reciprocal-only unless ``direct`` is set."""

    def __init__(self, snb, s, precision, direct=0, **kw):
        self.direct = direct
        super().__init__(snb, s, precision, **kw)

    def configure(self, cfg):
        s = self.s
        cfg.alpha = s["alpha"]; cfg.alpha_d = s["alpha_d"]
        for d in range(3):
            cfg.grid[d] = s["grid"][d]; cfg.dgrid[d] = s["dgrid"][d]; cfg.kmax[d] = s["kmax"][d]


def pipeline(st, method):
    """Which reciprocal pipeline ran, from the stamp slots of the timed (eager) steps (include/snb.h SNB_K_*): slot 1 the spreader, 2 the
    merge kernel of the own-atoms spreader or a forward z pass of its own (absent only when the brick spreader did the z pass itself), 3 / 5 the y passes of the three-pass pipeline (absent on the plane
    path, which only the own-atoms spreader feeds: no y passes means that spreader ran), 4 the x kernel or the plane kernel; 8 .. 15 the same for the dispersion mesh."""
    t = [int(x) for x in st.n_kernel_timed]
    out = []
    for name, o in (("coulomb", 0),) + ((("dispersion", 8),) if method == 5 else ()):
        if t[o + 1] == 0 and t[o + 4] == 0:
            out.append("%s: no mesh kernels" % name)
            continue
        out.append("%s: %s, %s" % (name, "brick spreader with the z pass fused" if t[o + 2] == 0 else "merge kernel or z pass of its own",
                                   "plane path" if (t[o + 3] == 0 and t[o + 5] == 0) else "three-pass y / x / y"))
    return "; ".join(out), t
