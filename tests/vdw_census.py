"""Van der Waals census: the systems, the closed forms, the comparison rule and the child-process entry shared by
tests/test_vdw_census.py (CPU) and tests/test_gpu_vdw_census.py (GPU).

Why.  Every other oracle comparison that carries Lennard-Jones judges it inside systems.random_box, a charged lattice of 0.22 .. 0.25 nm
spacing whose per-atom force is the repulsive core plus Coulomb, thousands of kJ/mol/nm: at the bar tol max(|F|, 1) everything LJ does
beyond about 1.3 sigma is invisible -- the switching function can be turned off entirely without a test noticing.  The systems below are
UNCHARGED, so LJ stands alone (the Coulomb columns of every output are asserted to be zero), on a lattice of 0.40 nm spacing where the
far range of the potential is the whole force, and the floor of the per-atom comparison is the oracle's median force, not 1.

 * lj_big: 20^3 atoms in 8 nm, the GPU list builder (packed kernels in single and mixed precision); lj_small: 9^3 atoms in 3.6 nm, host
   lists with per-pair wrapping (a block of 32 atoms of one subset spans its sort column's whole height, so no block satisfies
   extent + 2 R < L, csrc/host_lists.h: the scalar kernels in float as well); nonperiodic: lj_big's atoms under CutoffNonPeriodic; nocutoff_cloud:
   97 atoms, NoCutoff with use_switch = 1, which must be ignored.
 * rows: reaction field, PME at the Ewald rows R0 and R2 of tests/ewald_census.py (float masks 3 and 0), LJPME at R0 and R4 (double masks
   7 and 0), each at the switching distances 0.6 and 0.9 of the cutoff, direct space alone.
 * radial dimers against the closed form E = 4 eps (x^12 - x^6) S(tt), no oracle.

A system is a dict of arrays as in tests/shell_systems.py, with `use_switch`, `sd` (the switching distance), `padding` and the Ewald
parameters beside them."""
import ctypes
import hashlib
import math
import os
import sys

import numpy as np

# The module is also the program of the census's child process (`python tests/vdw_census.py scalar OUT.json`), which starts without
# pytest's conftest: the repository root (bench.py, the package), oracle/ and tests/ must be importable before the imports below.
_ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (_ROOT, os.path.join(_ROOT, "oracle"), os.path.join(_ROOT, "tests")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import ewald_census as EC      # noqa: E402
import recip_systems as R
import shell_systems as S

BARS = EC.BARS
RC, SPACING, JITTER = 1.0, 0.40, 0.03
SWITCH_FRACTIONS = (0.6, 0.9)
NOCUTOFF, NONPERIODIC, RF, PME, LJPME = 0, 1, 2, 4, 5
NSUB = 4
DRIFT_SIGMA, DRIFT_FRAMES = 0.004, 4
#            method, Ewald row of ewald_census.ROWS (alpha, padding, the guard's masks)
ROWS = {"RF": (RF, None), "PME-R0": (PME, "R0"), "PME-R2": (PME, "R2"), "LJPME-R0": (LJPME, "R0"), "LJPME-R4": (LJPME, "R4"),
        "NonPeriodic": (NONPERIODIC, None), "NoCutoff": (NOCUTOFF, None)}
PERIODIC_ROWS = ("RF", "PME-R0", "PME-R2", "LJPME-R0", "LJPME-R4")
TABLE_ROWS = ("RF", "PME-R0")
MESH = {"lj_big": 32, "lj_small": 20, "dimers": 48}      # (the meshes stay idle: direct space only)
# SNB_* switches that send a step to another pair kernel, list builder or Ewald branch than the one a row names: with one of them in the
# environment the identity assertions (n_host_rebuilds, ewald_poly_mask) are skipped, the comparisons stay
REROUTING = ("SNB_SCALAR_ENERGY_KERNEL", "SNB_EWALD_ERFC", "SNB_EWALD_POLY_ALWAYS", "SNB_HOST_TRICLINIC")


def rerouted():
    return any(k in os.environ for k in REROUTING)


sl = R.sl


# ---- the lattice systems -----------------------------------------------------------------------------------------------------------
def _lambdas():
    """(Coulomb, vdW) per slice: every off-diagonal vdW value off 1, one of them 0."""
    lam = np.ones((NSUB * (NSUB + 1) // 2, 2))
    vals = iter([0.0, 0.9, 0.7, 0.3, 0.45, 0.6])
    for i in range(NSUB):
        for j in range(i):
            lam[sl(i, j), 1] = next(vals)
    return lam


def _lattice(name, m, seed):
    """m^3 uncharged LJ atoms on a lattice of 0.40 nm, jitter +-0.03 (z runs fastest: neighbours along z are adjacent indices).
    sigma 0.28 .. 0.36, epsilon 0.3 .. 1.2; 5 % of the atoms have epsilon = 0, half of those sigma = 1.0 (the water-hydrogen convention), and
    eight of the latter sit 0.1 nm from the heavy atom before them in their chain (an excluded pair).  Subsets 0 .. 2 at random, subset 3 holds
    epsilon = 0 atoms only.  Chains of four along z as systems.random_box builds them: 1-2 (0.4 nm) and 1-3 (0.8 nm) excluded, 1-4 (1.2 nm, beyond
    the cutoff) an exception with epsilon != 0; a second family of 1-4 exceptions joins atoms two sites apart along x (0.8 nm)."""
    rng = np.random.default_rng(seed)
    n, L = m ** 3, m * SPACING
    g = np.stack(np.meshgrid(np.arange(m), np.arange(m), np.arange(m), indexing="ij"), -1).reshape(-1, 3)
    pos = (g + 0.5) * SPACING + rng.uniform(-JITTER, JITTER, (n, 3))
    sigma, eps = rng.uniform(0.28, 0.36, n), rng.uniform(0.3, 1.2, n)
    dead = rng.permutation(n)[:int(round(0.05 * n))]
    eps[dead] = 0.0
    sigma[dead[::2]] = 1.0
    subset = rng.integers(0, 3, n)
    subset[dead[np.arange(len(dead)) % 4 < 2]] = 3
    chain_pos = np.where(g[:, 2] < 4 * (m // 4), g[:, 2] % 4, -1)
    hydrogens = [int(a) for a in dead[::2] if chain_pos[a] >= 1 and eps[a - 1] > 0][:8]
    for a in hydrogens:
        u = rng.normal(size=3)
        pos[a] = pos[a - 1] + 0.1 * u / np.linalg.norm(u)
    pairs, esig, eeps = [], [], []

    def add(i, j, sg, ep):
        pairs.append((i, j)); esig.append(sg); eeps.append(ep)

    def one_four(i, j):
        e = 0.5 * math.sqrt(eps[i] * eps[j])
        add(i, j, min(0.5 * (sigma[i] + sigma[j]), 0.36), e if e > 0 else 0.3)

    far14, near14 = [], []
    for a in np.nonzero(chain_pos == 0)[0]:
        a = int(a)
        for i, j in ((a, a + 1), (a + 1, a + 2), (a + 2, a + 3), (a, a + 2), (a + 1, a + 3)):
            add(i, j, 1.0, 0.0)
        far14.append(len(pairs)); one_four(a, a + 3)
    for a in np.nonzero((g[:, 0] % 4 == 0) & (g[:, 0] + 2 < m) & ((g[:, 1] + 2 * g[:, 2]) % 5 == 0))[0]:
        near14.append(len(pairs)); one_four(int(a), int(a) + 2 * m * m)
    s = S.make_system(name, pos, np.diag([L, L, L]), np.zeros(n), subset, NSUB, rc=RC)
    s.update(sigma=sigma, epsilon=eps, lam=_lambdas(), exc_pairs=np.ascontiguousarray(pairs, dtype=np.int32), exc_qq=np.zeros(len(pairs)),
             exc_sigma=np.asarray(esig), exc_eps=np.asarray(eeps), exceptions_periodic=False, topology="chains", hydrogens=hydrogens, dead=np.sort(dead),
             far14=np.asarray(far14), near14=np.asarray(near14), L=L)
    s.update(method=RF, use_switch=1, sd=0.9 * RC, padding=0.1, alpha=0.0, alpha_d=0.0, grid=(0, 0, 0), dgrid=(0, 0, 0), kmax=(0, 0, 0))
    s["pos"] = clear_cutoff_band(s)
    return s


def _nocutoff_cloud():
    """97 atoms of a 5^3 lattice, no cell: NoCutoff with use_switch = 1."""
    rng = np.random.default_rng(313)
    g = np.stack(np.meshgrid(np.arange(5), np.arange(5), np.arange(5), indexing="ij"), -1).reshape(-1, 3)[:97]
    pos = (g + 0.5) * SPACING + rng.uniform(-JITTER, JITTER, (97, 3)) + np.array([3.1, -2.2, 0.7])
    s = S.make_system("nocutoff_cloud", pos, None, np.zeros(97), rng.integers(0, NSUB, 97), NSUB, rc=RC)
    eps = rng.uniform(0.3, 1.2, 97)
    eps[s["subset"] == 3] = 0.0
    a = np.arange(0, 96, 4)
    pairs = np.concatenate([np.stack([a, a + 1], 1), np.stack([a, a + 3], 1)])
    s.update(sigma=rng.uniform(0.28, 0.36, 97), epsilon=eps, lam=_lambdas(), exc_pairs=np.ascontiguousarray(pairs, dtype=np.int32), exc_qq=np.zeros(len(pairs)),
             exc_sigma=np.full(len(pairs), 0.3), exc_eps=np.concatenate([np.zeros(len(a)), np.full(len(a), 0.4)]), topology="chains", L=None)
    s.update(method=NOCUTOFF, use_switch=1, sd=0.9 * RC, padding=0.0, alpha=0.0, alpha_d=0.0, grid=(0, 0, 0), dgrid=(0, 0, 0), kmax=(0, 0, 0))
    return s


def band_pairs(s, pos=None):
    """The non-excluded pairs within ewald_census.CUTOFF_BAND of the cutoff, by the oracle's diagnostic (minimum image where periodic)."""
    t = dict(s, method=RF if s["box"] is not None else NONPERIODIC)
    if pos is not None:
        t["pos"] = np.ascontiguousarray(pos)
    rc = s["rc"]
    ij, r, _ = S._pairs_between(t, (rc - EC.CUTOFF_BAND) ** 2, (rc + EC.CUTOFF_BAND) ** 2)
    return ij, r


def clear_cutoff_band(s, pos=None):
    """ewald_census.clear_cutoff_band (one atom of every pair within CUTOFF_BAND of the cutoff moves 1e-4 nm outward along the pair's axis,
    float coordinates) with the pairs found by the oracle's band diagnostic: all pairs in numpy are 2 GB at 8000 atoms.  The LJPME rows have
    no switching function, and the LJ force still jumps by about 0.017 kJ/mol/nm at the cutoff, several single-precision bars: no pair
    may sit where rounding decides its side."""
    pos = np.array(s["pos"] if pos is None else pos, dtype=np.float64)
    for _ in range(20):
        ij, r = band_pairs(s, pos)
        if len(ij) == 0:
            return pos
        d = S._min_image(s, pos[ij[:, 1]] - pos[ij[:, 0]])
        pos[ij[:, 1]] += 1e-4 * d / np.linalg.norm(d, axis=1)[:, None]
        pos = S.to_float(pos)
    raise AssertionError("the cutoff band does not clear")


_BUILT, _FRAMES = {}, {}


def build(name):
    """lj_big, lj_small, nonperiodic or nocutoff_cloud, built once per session (callers must not modify it)."""
    if name not in _BUILT:
        if name == "lj_big":
            s = _lattice(name, 20, 311)
        elif name == "lj_small":
            s = _lattice(name, 9, 312)
        elif name == "nonperiodic":
            s = dict(build("lj_big"), name=name, box=None, method=NONPERIODIC)
        else:
            assert name == "nocutoff_cloud", name
            s = _nocutoff_cloud()
        _BUILT[name] = s
    return _BUILT[name]


def frames(name):
    """DRIFT_FRAMES coordinate sets: the system's own, then a seeded walk with normal steps of DRIFT_SIGMA nm per coordinate; float
    coordinates, the cutoff band cleared in each.  nonperiodic shares lj_big's (its pairs are a subset of the periodic ones)."""
    key = "lj_big" if name == "nonperiodic" else name
    if key not in _FRAMES:
        s = build(key)
        rng = np.random.default_rng(7)
        out = [s["pos"]]
        for _ in range(DRIFT_FRAMES - 1):
            p = S.to_float(out[-1] + rng.normal(0.0, DRIFT_SIGMA, out[-1].shape))
            out.append(clear_cutoff_band(s, p) if s["box"] is not None else p)
        _FRAMES[key] = out
    return _FRAMES[key]


def case_system(name, row, sdf, frame=0):
    """The system of a census case: `name` under the method and Ewald parameters of `row`, switching distance sdf * cutoff, frame `frame`."""
    method, ew = ROWS[row]
    t = dict(build(name), method=method, use_switch=1, sd=sdf * RC, pos=frames(name)[frame])
    if ew is not None:
        e = EC.ROWS[ew]
        mesh = MESH[name]
        t.update(alpha=e["alpha"], alpha_d=e["alpha"], padding=e["padding"], grid=(mesh,) * 3, dgrid=(mesh,) * 3 if method == LJPME else (0, 0, 0))
    t["name"] = "%s %s sd %.1f" % (name, row, sdf)
    return t


def gpu_builder_applies(s, padding=None):
    """The engine's own rule (engine.hip gpuRebuild): every cell length must exceed four mean block edges plus two list radii."""
    return R.gpu_builder_applies(s, s["padding"] if padding is None else padding)


# ---- the oracle ----------------------------------------------------------------------------------------------------------------------
_ORACLE = {}


def oracle_eval(s):
    """(forces [N][3], raw slice energies [S][2]) of the oracle's direct-space part for a system record, everything read from the record
    (use_switch and sd included); kept for the session, keyed by everything that reaches the oracle."""
    o = S._orc(); L = o.lib()
    cfg = o.OrcConfig()
    cfg.n_atoms = len(s["q"]); cfg.n_subsets = s["nsub"]; cfg.method = s["method"]; cfg.cutoff = s["rc"]; cfg.rf_dielectric = 1.0
    cfg.use_switch = int(s["use_switch"]); cfg.switch_distance = s["sd"]
    cfg.alpha = s["alpha"]; cfg.alpha_d = s["alpha_d"]
    for d in range(3):
        cfg.grid[d] = s["grid"][d]; cfg.dgrid[d] = max(s["dgrid"][d], 1); cfg.kmax[d] = s["kmax"][d]
    cfg.exceptions_periodic = int(s["exceptions_periodic"])
    cfg.include_direct = 1; cfg.include_reciprocal = 0; cfg.background_term = 1; cfg.correct_q1 = 1
    m = len(s["exc_qq"])
    pairs = np.ascontiguousarray(s["exc_pairs"] if m else np.zeros((1, 2)), dtype=np.int32)
    qq, sg, ep = (np.ascontiguousarray(a if m else np.zeros(1), dtype=np.float64) for a in (s["exc_qq"], s["exc_sigma"], s["exc_eps"]))
    pos = np.ascontiguousarray(s["pos"], dtype=np.float64); box = S.box9(s); lam = np.ascontiguousarray(s["lam"], dtype=np.float64)
    q, sig, eps = (np.ascontiguousarray(s[k], dtype=np.float64) for k in ("q", "sigma", "epsilon"))
    sub = np.ascontiguousarray(s["subset"], dtype=np.int32)
    assert lam.shape == (s["nsub"] * (s["nsub"] + 1) // 2, 2)
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
        while len(_ORACLE) > 600:
            _ORACLE.pop(next(iter(_ORACLE)))
        _ORACLE[key] = (f, se)
    f, se = _ORACLE[key]
    return f.copy(), se.copy()


def subset_evaluator(s):
    """evaluator(subset, nsub) of tests/atom_energy_truth.py and tests/group_pair_truth.py: raw slice energies, every lambda 1."""
    def ev(subset, nsub):
        return oracle_eval(dict(s, subset=np.ascontiguousarray(subset, dtype=np.int32), nsub=nsub, lam=np.ones((nsub * (nsub + 1) // 2, 2))))[1]
    return ev


def lambda_evaluator(s):
    """evaluator(lam) of tests/atom_force_truth.py.  The systems are uncharged: a Coulomb-only lambda table gives exact zeros without asking."""
    def ev(lam):
        lam = np.asarray(lam, dtype=np.float64)
        if not lam[:, 1].any():
            assert not s["q"].any()
            return np.zeros((len(s["q"]), 3))
        return oracle_eval(dict(s, lam=lam))[0]
    return ev


# ---- the comparison rule -----------------------------------------------------------------------------------------------------------------
def force_floor(s, fo):
    """F_med: the oracle's median force magnitude over the atoms with epsilon > 0."""
    return float(np.median(np.linalg.norm(fo, axis=-1)[s["epsilon"] > 0]))


def compare_forces(s, f, fo, tol, floor=None):
    """|dF_i| <= tol max(|F_i|, F_med) on every atom -- the floor rule of the reciprocal census, not a floor of 1: an epsilon = 0 atom must
    stay below tol F_med.  fo: the oracle's forces ([N][3], or a table column).  A dict; ``flagged`` are the atoms over the bar."""
    fn = np.linalg.norm(fo, axis=-1)
    floor = force_floor(s, fo) if floor is None else floor
    df = np.linalg.norm(np.asarray(f) - fo, axis=-1)
    denom = np.maximum(fn, floor)
    err = np.where(df == 0, 0.0, df / np.where(denom > 0, denom, 1.0))
    err = np.where((denom == 0) & (df > 0), np.inf, err)
    flagged = np.where(~(err <= tol))[0]
    w = int(np.argmax(np.where(np.isnan(err), np.inf, err)))
    return dict(ok=len(flagged) == 0, flagged=[int(a) for a in flagged], max_err=float(err[w]), median_err=float(np.median(err)), floor=floor, worst_atom=w,
                worst_dF=float(df[w]), worst_F=float(fn[w]), tol=tol, err=err)


def energy_err(got, want):
    """Worst |dE| / max(|E|, 1)."""
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    return float(np.max(np.abs(got - want) / np.maximum(np.abs(want), 1.0))) if got.size else 0.0


def table_force_err(s, got, want):
    """The force rule per column of the vdW half of an atom-force table [N][nsub][2][3]: (worst error, column, atom); the floor of column J
    is the oracle's median over the epsilon > 0 atoms of that column."""
    worst = (0.0, 0, 0)
    for J in range(want.shape[1]):
        rec = compare_forces(s, got[:, J, 1], want[:, J, 1], 1.0)
        if rec["max_err"] > worst[0]:
            worst = (rec["max_err"], J, rec["worst_atom"])
    return worst


# ---- the engine ------------------------------------------------------------------------------------------------------------------------
class Engine(R.Engine):
    """recip_systems.Engine, direct space alone, with the record's switching function and list padding."""

    def __init__(self, snb, s, precision, host_build=0, sd=None):
        self._sd = s["sd"] if sd is None else sd
        super().__init__(snb, s, precision, direct=1, padding=s["padding"], interval=10 if s["padding"] > 0 else 1, host_build=host_build)
        self.recip = 0

    def configure(self, cfg):
        cfg.use_switch = int(self.s["use_switch"]); cfg.switch_distance = self._sd
        if self.s["method"] in (PME, LJPME):
            super().configure(cfg)

    def step_derivative(self, mask):
        """A derivative-only step (include_energy = 2) on the slices of `mask`: (forces, raw slice energies); the mask is put back."""
        ip = lambda a: a.ctypes.data_as(ctypes.POINTER(ctypes.c_int32))
        m = np.ascontiguousarray(mask, dtype=np.int32)
        self.ok(self.L.snb_set_energy_slices(self.h, ip(m)))
        self.ok(self.L.snb_execute(self.h, 1, 2, self.direct, self.recip, None))
        out = self.forces(), self.slice_energies()
        self.ok(self.L.snb_set_energy_slices(self.h, ip(np.ones(len(m), dtype=np.int32))))
        return out

    def atom_energies(self):
        out = np.full((self.n, self.s["nsub"], 2), np.nan)
        self.ok(self.L.snb_evaluate_atom_energies(self.h, 1, 0, out.ctypes.data_as(ctypes.c_void_p), 0))
        return out

    def atom_forces(self):
        out = np.full((self.n, self.s["nsub"], 2, 3), np.nan)
        self.ok(self.L.snb_evaluate_atom_forces(self.h, 1, 0, out.ctypes.data_as(ctypes.c_void_p), 0))
        return out

    def group_pairs(self, labels, G):
        lab = np.ascontiguousarray(labels, dtype=np.int32)
        out = np.full((G * (G + 1) // 2, 2), np.nan)
        b = self.capi.SnbGroupPairBatch()
        b.n_frames = 1; b.n_groups = G; b.group_of_atom = lab.ctypes.data_as(ctypes.POINTER(ctypes.c_int32))
        b.pair_energies = out.ctypes.data_as(ctypes.c_void_p); b.out_is_device = 0
        self.ok(self.L.snb_evaluate_group_pair_energies(self.h, ctypes.byref(b)))
        return out


# ---- (a) bulk, against the oracle ------------------------------------------------------------------------------------------------------
GROUPS = 12
DERIVATIVE_SLICES = (sl(1, 0), sl(2, 2))      # the mask of the derivative-only step: the slice at lambda = 0 and a diagonal one


def group_labels(n):
    """12 labels at random, about one atom in thirteen unlabelled."""
    return np.random.default_rng(17).integers(-1, GROUPS, n)


def probes(s):
    """The rows of the atom-energy table that are checked: chain ends, atoms of every subset, epsilon = 0 atoms, a hydrogen, a 0.8 nm exception."""
    p = [0, len(s["q"]) - 1, int(s["hydrogens"][0]), int(s["exc_pairs"][s["near14"][0], 0])]
    p += [int(np.nonzero(s["subset"] == k)[0][5]) for k in range(NSUB)]
    return sorted(set(p))


def bulk_case(snb, name, row, sdf, prec, tables=False, steps=("f", "ef", "e", "d"), engine_sd=None):
    """One engine on a census case.  Steps: 'f' four forces-only steps (eager, captured, replayed twice) on positions that drift on an
    unchanged list, the oracle re-evaluated on each; 'ef' energy + forces; 'e' energy only (include_forces = 0); 'd' derivative only
    (include_energy = 2) on DERIVATIVE_SLICES, the selected vdW energies and every atom's force; with `tables` the vdW columns of the three
    tables.  engine_sd: the planted defect, an engine created with another switching distance than the oracle's.  Returns {'checks': [(what,
    error, detail)] in units of the rule's denominators, 'coulomb': the largest |x| of a Coulomb column, 'finite', 'mask', 'host_rebuilds',
    'floor', 'flagged': the share of atoms over the bar on the 'ef' step, 'drift_rebuilds' / 'overruns': n_rebuilds and n_list_overruns after the
    forces-only steps}."""
    import atom_energy_truth as aet
    import atom_force_truth as aft
    import group_pair_truth as gpt
    tol = BARS[prec]
    last = DRIFT_FRAMES - 1 if "f" in steps else 0
    sys_of = lambda k: case_system(name, row, sdf, k)
    eng = Engine(snb, sys_of(0), prec, sd=engine_sd)
    checks, coulomb, finite, flagged, floor, drift_rebuilds, overruns = [], 0.0, True, None, None, None, None

    def forces(what, s, f):
        nonlocal finite, floor
        fo, _ = oracle_eval(s)
        rec = compare_forces(s, f, fo, tol)
        finite &= bool(np.isfinite(f).all())
        floor = rec["floor"]
        checks.append((what, rec["max_err"], "atom %d: |dF| %.3e of |F| %.3e, F_med %.3e" % (rec["worst_atom"], rec["worst_dF"], rec["worst_F"], rec["floor"])))
        return rec

    def energies(what, s, se, only=None):
        nonlocal finite, coulomb
        _, so = oracle_eval(s)
        k = np.arange(len(so)) if only is None else np.asarray(only)
        finite &= bool(np.isfinite(se[k]).all())
        coulomb = max(coulomb, float(np.abs(se[k, 0]).max()))
        assert not so[:, 0].any()
        checks.append((what, energy_err(se[k, 1], so[k, 1]), "vdW slice energies"))

    if "f" in steps:
        for k in range(DRIFT_FRAMES):
            s = sys_of(k)
            eng.set_frame(s)
            forces("f%d" % k, s, eng.step_forces())
        st = eng.stats()
        drift_rebuilds, overruns = int(st.n_rebuilds), int(st.n_list_overruns)
    s = sys_of(last)
    eng.set_frame(s)
    if "ef" in steps:
        f, se, e = eng.step_energy_forces()
        flagged = len(forces("ef forces", s, f)["flagged"]) / float(len(s["q"]))
        energies("ef energies", s, se)
        finite &= bool(np.isfinite(e))
        checks.append(("ef total", energy_err(e, float((s["lam"] * oracle_eval(s)[1]).sum())), "sum lambda E"))
    if "e" in steps:
        energies("e energies", s, eng.step_energy_only())
    if "d" in steps:
        mask = np.zeros(len(s["lam"]), dtype=np.int32); mask[list(DERIVATIVE_SLICES)] = 1
        f, se = eng.step_derivative(mask)
        forces("d forces", s, f)
        energies("d energies", s, se, only=DERIVATIVE_SLICES)
    if tables:
        tabE, tabF = eng.atom_energies(), eng.atom_forces()
        lab = group_labels(len(s["q"]))
        mat = eng.group_pairs(lab, GROUPS)
        finite &= bool(np.isfinite(tabE).all() and np.isfinite(tabF).all() and np.isfinite(mat).all())
        coulomb = max(coulomb, float(np.abs(tabE[..., 0]).max()), float(np.abs(tabF[:, :, 0]).max()), float(np.abs(mat[:, 0]).max()))
        want = aet.truth_table(subset_evaluator(s), s["subset"], NSUB, probes(s))
        checks.append(("atomE", max(energy_err(tabE[a][:, 1], r[:, 1]) for a, r in want.items()), "probe rows %s" % sorted(want)))
        err, J, a = table_force_err(s, tabF, aft.truth_table(lambda_evaluator(s), s["subset"], NSUB))
        checks.append(("atomF", err, "column %d, atom %d" % (J, a)))
        checks.append(("groupPairs", energy_err(mat[:, 1], gpt.truth(subset_evaluator(s), lab, GROUPS)[:, 1]), "%d labels" % GROUPS))
    st = eng.stats()
    rec = dict(checks=checks, coulomb=coulomb, finite=finite, mask=int(st.ewald_poly_mask), host_rebuilds=int(st.n_host_rebuilds), rebuilds=int(st.n_rebuilds),
               floor=floor, flagged=flagged, drift_rebuilds=drift_rebuilds, overruns=overruns)
    eng.close()
    return rec


def expected_mask(row, prec):
    method, ew = ROWS[row]
    return EC.engine_mask(EC.ROWS[ew], prec, method) if ew is not None else 0


# ---- (b) radial dimers, against the closed form ----------------------------------------------------------------------------------------
DIMER_SITES, DIMER_SPACING = 7, 2.2          # 343 dimers in a 15.4 nm cell: one ulp of a coordinate stays below 1e-6 nm
FILLER_SITES = 15                            # 3375 atoms with epsilon = 0 between the dimers: they take the cell over the GPU builder's threshold
N_SWITCH, N_OUTSIDE = 220, 9
DIMER_LAMBDAS = (1.0, 0.7, 0.5)              # vdW lambda of the slices (0, 0), (1, 0), (1, 1)


def switch_value(tt):
    """S = 1 - 10 tt^3 + 15 tt^4 - 6 tt^5 and dS/dtt, in the factored form (1 - tt)^3 (1 + 3 tt + 6 tt^2), which is the same polynomial
    without the cancellation at tt -> 1 (the expanded form loses 1e-16 / S of its value there, above 1e-12 from S = 1e-4 on)."""
    tt = np.clip(tt, 0.0, 1.0)
    return (1.0 - tt) ** 3 * (1.0 + 3.0 * tt + 6.0 * tt * tt), -30.0 * tt * tt * (1.0 - tt) ** 2


def closed_form(r, sij, eij, sd, rc=RC, use_switch=True):
    """(E, F = -dE/dr, scale) of E = 4 eps (x^12 - x^6) S(tt), x = sigma / r, tt = (r - sd) / (rc - sd) clamped to [0, 1]; scale: the sum
    of the absolute values of the terms of F, 4 eps (12 x^12 + 6 x^6) / r S + 4 eps (x^12 + x^6) |S'|.  Zero at and beyond the cutoff."""
    r = np.asarray(r, dtype=np.float64)
    x6 = (sij / r) ** 6; x12 = x6 * x6
    w = rc - sd
    sw, dsw = switch_value((r - sd) / w) if use_switch else (np.ones_like(r), np.zeros_like(r))
    dsw = dsw / w
    e0, de0 = 4.0 * eij * (x12 - x6), -4.0 * eij * (12.0 * x12 - 6.0 * x6) / r
    ins = r < rc
    scale = 4.0 * eij * (12.0 * x12 + 6.0 * x6) / r * sw + 4.0 * eij * (x12 + x6) * np.abs(dsw)
    return np.where(ins, e0 * sw, 0.0), np.where(ins, -(de0 * sw + e0 * dsw), 0.0), np.where(ins, scale, 0.0)


def is_float(prec):
    return EC.is_float(prec)


def tt_limit(prec, sdf, cell=DIMER_SITES * DIMER_SPACING):
    """The tt beyond which the relative bar tol * scale cannot be asked of an engine of this precision -- a calculation, not a measurement.
    Towards tt -> 1, S behaves like 10 (1 - tt)^3 and S' like 30 (1 - tt)^2 / w, while what rounding leaves does not shrink with them:
     * r: the engine re-images atoms by whole cells, so its r differs from the r of the given coordinates by up to one ulp u of a coordinate
       (float: 9.5e-7 nm in a cell of 8 .. 16 nm; double: 1.8e-15), which moves F by u |dF/dr|, where the S'' = 60 (1 - tt) / w^2 term wins;
     * the switch polynomials as the kernels and the reference write them (Horner, expanded form): each rounding is at most half an ulp of an
       intermediate no larger than the sum of the absolute coefficients, 32 for S and 120 / w for S', so S is off by up to 32 eps and S' by
       up to 120 eps / w in absolute terms (eps = 2^-24 or 2^-53), however small they have become;
     * 16 eps of the scale for the rest of the pair arithmetic.
    Returns the smallest tt >= 0.5 at which their sum reaches tol * scale for a sigma of the dimers' range (epsilon cancels)."""
    tol, w, sd = BARS[prec], RC * (1.0 - sdf), RC * sdf
    eps = 2.0 ** -24 if is_float(prec) else 2.0 ** -53
    u = float(np.spacing(np.float32(cell))) if is_float(prec) else float(np.spacing(np.float64(cell)))
    tt = np.sort(1.0 - np.logspace(-9.0, math.log10(0.5), 6000))
    limit = 1.0
    for sij in (0.45, 0.6):
        r = sd + w * tt
        x6 = (sij / r) ** 6; x12 = x6 * x6
        sw, dsw = switch_value(tt)
        dsw = np.abs(dsw) / w
        d2sw = np.abs(60.0 * tt * (1.0 - tt) * (1.0 - 2.0 * tt)) / (w * w)
        e0, de0, d2e0 = 4.0 * (x12 + x6), 4.0 * (12.0 * x12 + 6.0 * x6) / r, 4.0 * (156.0 * x12 + 42.0 * x6) / (r * r)
        scale = de0 * sw + e0 * dsw
        moved = u * (d2e0 * sw + 2.0 * de0 * dsw + e0 * d2sw) + 32.0 * eps * de0 + 120.0 * eps / w * e0 + 16.0 * eps * scale
        over = np.nonzero(moved >= tol * scale)[0]
        if len(over):
            limit = min(limit, float(tt[over[0]]))
    return limit


def _float_neighbours(x):
    """The nearest float32 values to either side of the double x."""
    f = np.float32(x)
    lo = f if float(f) <= x else np.nextafter(f, np.float32(0.0))
    return float(lo), float(np.nextafter(lo, np.float32(np.inf)))


def special_radii(sdf):
    """Radii laid exactly (along x from an atom at x = 0, so that r is the float itself): the nearest floats to either side of the switching
    distance, tt = 0.5, the float next below the cutoff, and 1e-5 to either side of the cutoff."""
    sd = RC * sdf
    lo, hi = _float_neighbours(sd)
    return [lo, hi, float(np.float32(sd + 0.5 * (RC - sd))), float(np.nextafter(np.float32(RC), np.float32(0.0))), float(np.float32(RC * (1.0 - 1e-5))), float(np.float32(RC * (1.0 + 1e-5)))]


_DIMERS = {}


def dimer_gas(sdf, row="RF"):
    """A gas of isolated LJ dimers in the style of ewald_census.ewald_dimers: 343 dimers on a lattice of centres 2.2 nm apart that starts
    at the origin (bonds cross faces, edges and, the dimer at the origin, the corner), random orientations, unequal parameters inside a dimer
    (sigma_ij 0.45 .. 0.6 from sigma_i != sigma_j, epsilon_ij 0.5 .. 4 from epsilon_i != epsilon_j: Lorentz-Berthelot is under test), float
    coordinates.  Radii: 220 spread evenly over the switch region, about 100 from 0.9 sigma_ij up to the switching distance, special_radii,
    two more just inside the cutoff and nine beyond it (up to 1.05 rc: partners of other dimers stay beyond the cutoff).  3375 atoms with
    epsilon = 0 fill the space between.  `expected` forces, `scale` and `expected_slice_energies` from closed_form, r in double from the
    float coordinates; under LJPME `expected` is None (the caller takes the oracle: the potential shifts have no short closed form)."""
    key = (sdf, row)
    if key in _DIMERS:
        return _DIMERS[key]
    method, ew = ROWS[row]
    rng = np.random.default_rng(79)
    sd, w = RC * sdf, RC * (1.0 - sdf)
    m, L = DIMER_SITES, DIMER_SITES * DIMER_SPACING
    g = np.stack(np.meshgrid(np.arange(m), np.arange(m), np.arange(m), indexing="ij"), -1).reshape(-1, 3).astype(float)
    centres = g * DIMER_SPACING
    nd = len(centres)
    u = rng.normal(size=(nd, 3)); u /= np.linalg.norm(u, axis=1)[:, None]
    u[0] = np.ones(3) / math.sqrt(3.0)
    sij, eij = rng.uniform(0.45, 0.6, nd), rng.uniform(0.5, 4.0, nd)
    special = special_radii(sdf)
    ns = len(special)
    sites = np.arange(1, 1 + ns)      # sites (0, 0, 1 ..): their centres have x = 0
    u[m * m + sites] = np.array([0.0, 1.0, 0.0])      # their neighbours (1, 0, 1 ..) lie along y: 1.2 nm and more from the special atom at x = r
    rest = np.setdiff1d(np.arange(nd), sites)
    nb = len(rest) - N_SWITCH - 2 - N_OUTSIDE
    frac = np.linspace(0.0, 1.0, nb, endpoint=False)
    target = np.zeros(nd)
    order = rng.permutation(rest)
    lo = 0.9 * sij[order[:nb]]
    target[order[:nb]] = lo + frac * (sd - lo)
    target[order[nb:nb + N_SWITCH]] = sd + w * (np.arange(N_SWITCH) + 0.5) / N_SWITCH
    target[order[nb + N_SWITCH:nb + N_SWITCH + 2]] = RC * (1.0 - np.array([1e-4, 1e-3]))
    target[order[nb + N_SWITCH + 2:]] = RC * (1.0 + np.array([1e-4, 3e-4, 1e-3, 3e-3, 1e-2, 2e-2, 3e-2, 4e-2, 5e-2]))
    a, b = centres - 0.5 * target[:, None] * u, centres + 0.5 * target[:, None] * u
    a[sites] = centres[sites]; b[sites] = centres[sites] + np.array([1.0, 0.0, 0.0]) * np.asarray(special)[:, None]
    fm = FILLER_SITES
    fg = np.stack(np.meshgrid(np.arange(fm), np.arange(fm), np.arange(fm), indexing="ij"), -1).reshape(-1, 3)
    filler = (fg + 0.5) * (L / fm) + rng.uniform(-0.1, 0.1, (fm ** 3, 3))
    pos = np.concatenate([a, b, filler])
    pos = S.to_float(pos - np.floor(pos / L) * L)
    n = len(pos)
    delta = rng.uniform(0.1, 0.3, nd) * rng.choice([-1.0, 1.0], nd)
    k = rng.uniform(0.5, 2.0, nd)
    sigma = np.concatenate([sij * (1.0 + delta), sij * (1.0 - delta), np.full(fm ** 3, 0.3)])
    eps = np.concatenate([eij * k, eij / k, np.zeros(fm ** 3)])
    sub = np.concatenate([np.arange(nd) % 2, (np.arange(nd) // 2) % 2, np.full(fm ** 3, 2)]).astype(np.int32)
    s = S.make_system("dimers %s sd %.1f" % (row, sdf), pos, np.diag([L, L, L]), np.zeros(n), sub, 3, rc=RC)
    lam = np.ones((6, 2)); lam[:3, 1] = DIMER_LAMBDAS; lam[3:, 1] = 0.9
    s.update(sigma=sigma, epsilon=eps, lam=lam, method=method, use_switch=1, sd=sd, padding=0.1, alpha=0.0, alpha_d=0.0, grid=(0, 0, 0), dgrid=(0, 0, 0), kmax=(0, 0, 0), L=L, nd=nd)
    if ew is not None:
        e = EC.ROWS[ew]
        s.update(alpha=e["alpha"], alpha_d=e["alpha"], padding=e["padding"], grid=(MESH["dimers"],) * 3, dgrid=(MESH["dimers"],) * 3 if method == LJPME else (0, 0, 0))
    partner = np.concatenate([np.arange(nd) + nd, np.arange(nd)])
    d = -S._min_image(s, s["pos"][partner] - s["pos"][:2 * nd])      # r_i - r_partner
    r = np.linalg.norm(d, axis=1)
    sij2, eij2 = np.concatenate([sij, sij]), np.concatenate([eij, eij])
    slice_of = np.array([sl(int(sub[i]), int(sub[partner[i]])) for i in range(2 * nd)])
    lam_of = lam[slice_of, 1]
    E, F, scale = closed_form(r, sij2, eij2, sd, use_switch=(method != LJPME))
    es = np.zeros((6, 2))
    np.add.at(es[:, 1], slice_of[:nd], E[:nd])
    s.update(partner=partner, r=r, tt=(r - sd) / w, inside=r < RC, sij=sij2, eij=eij2, slice_of=slice_of, lam_of=lam_of, axis=d / r[:, None],
             expected=None if method == LJPME else (lam_of * F)[:, None] * d / r[:, None], scale=lam_of * scale,
             expected_slice_energies=None if method == LJPME else es, special_sites=sites)
    _DIMERS[key] = s
    return s


def in_switch_region(s):
    """The dimer atoms whose separation lies in the switch region, sd < r < rc."""
    return (s["r"] > s["sd"]) & s["inside"]


def near_cutoff(s, prec):
    """The dimer atoms of the switch region beyond tt_limit: held to the absolute bar tol * scale(tt_limit)."""
    return in_switch_region(s) & (s["tt"] > tt_limit(prec, s["sd"] / RC))


def dimer_bars(s, prec):
    """tol * scale per dimer atom; beyond tt_limit tol * scale(tt_limit) with the dimer's own parameters.  (Under LJPME no switching
    function acts: the scale is that of the plain LJ terms everywhere.)"""
    tol = BARS[prec]
    bar = tol * s["scale"]
    if s["method"] != LJPME:
        far = near_cutoff(s, prec)
        sd = s["sd"]
        rl = sd + (RC - sd) * tt_limit(prec, sd / RC)
        bar = np.where(far, tol * s["lam_of"] * closed_form(np.full(len(bar), rl), s["sij"], s["eij"], sd)[2], bar)
    return bar


def compare_dimers(s, f, prec, expected=None):
    """Per dimer atom against the closed form (or `expected`): |dF| <= the bar of dimer_bars inside the cutoff, exactly zero beyond it and
    on the filler atoms.  Returns (worst error in bars, zero_ok, description of the worst atom)."""
    nd2 = 2 * s["nd"]
    f = np.asarray(f)
    ex = s["expected"] if expected is None else expected[:nd2]
    ins = s["inside"]
    bars = dimer_bars(s, prec)
    err = np.linalg.norm(f[:nd2] - ex, axis=1)[ins] / bars[ins]
    zero_ok = bool((f[:nd2][~ins] == 0).all() and (f[nd2:] == 0).all())
    w = np.nonzero(ins)[0][int(np.argmax(np.where(np.isnan(err), np.inf, err)))]
    return float(np.max(np.where(np.isnan(err), np.inf, err))), zero_ok, "atom %d: r = %.7f nm, tt = %.5f, sigma_ij %.3f, epsilon_ij %.2f, |F| %.3e, bar %.3e" % (
        w, s["r"][w], s["tt"][w], s["sij"][w], s["eij"][w], np.linalg.norm(ex[w]), bars[w])


def dimer_case(snb, row, sdf, prec, host):
    """Forces-only, energy + forces and energy-only steps of the dimer gas on one engine: {'checks': [(step, error, detail)] -- forces in
    units of the dimer's bar, energies in units of tol --, 'zero': exact zeros beyond the cutoff, 'coulomb', 'finite', 'mask', 'host_rebuilds'}."""
    s = dimer_gas(sdf, row)
    tol = BARS[prec]
    eng = Engine(snb, s, prec, host_build=host)
    f1 = eng.step_forces()
    f2, se, _ = eng.step_energy_forces()
    se_only = eng.step_energy_only()
    st = eng.stats()
    mask, hostn = int(st.ewald_poly_mask), int(st.n_host_rebuilds)
    eng.close()
    expected = es = None
    if s["method"] == LJPME:
        expected, es = oracle_eval(s)
    else:
        es = s["expected_slice_energies"]
    checks, zero = [], True
    for what, f in (("f", f1), ("ef forces", f2)):
        err, z, worst = compare_dimers(s, f, prec, expected)
        checks.append((what, err, worst)); zero &= z
    for what, e in (("ef energies", se), ("e energies", se_only)):
        checks.append((what, energy_err(e[:, 1], es[:, 1]) / tol, "vdW slice energies"))
    finite = bool(np.isfinite(f1).all() and np.isfinite(f2).all() and np.isfinite(se).all() and np.isfinite(se_only).all())
    return dict(checks=checks, zero=zero, coulomb=float(max(np.abs(se[:, 0]).max(), np.abs(se_only[:, 0]).max())), finite=finite, mask=mask, host_rebuilds=hostn)


def kernel_form_float32(s):
    """The pair force of the dimers by the kernels' formula (direct.hip tileSteps) in float32 numpy, from r rounded to float32: what
    single-precision pair arithmetic gives with nothing wrong.  Returns the signed force magnitudes of the dimer atoms, in float64."""
    f32 = np.float32
    r = s["r"].astype(f32)
    sig, eps4 = s["sij"].astype(f32), (4.0 * s["eij"]).astype(f32)
    inv = f32(1.0) / r
    s2 = (sig * inv) * (sig * inv); s6 = s2 * s2 * s2
    es6 = eps4 * s6
    fLJ = es6 * (f32(12.0) * s6 - f32(6.0))      # -r dE/dr
    e0 = es6 * (s6 - f32(1.0))
    sd, iw = f32(s["sd"]), f32(1.0 / (RC - s["sd"]))
    tt = np.maximum((r - sd) * iw, f32(0.0))
    sw = f32(1.0) + tt * tt * tt * (f32(-10.0) + tt * (f32(15.0) - tt * f32(6.0)))
    dsw = tt * tt * (f32(-30.0) + tt * (f32(60.0) - tt * f32(30.0))) * iw
    fLJ = fLJ * sw - e0 * dsw * r
    return np.where(s["inside"], (fLJ * inv).astype(np.float64) * s["lam_of"], 0.0)


# ---- (c) the child process: energy steps of single precision on the scalar tile kernel ----------------------------------------------------
SCALAR_CASES = [(row, sdf) for row in ("RF", "PME-R0") for sdf in SWITCH_FRACTIONS]


def main(argv):
    """`scalar OUT.json`: the energy + forces step of SCALAR_CASES on lj_big in single precision, in this process's environment (the test
    sets SNB_SCALAR_ENERGY_KERNEL: the switches are read once per process)."""
    import importlib
    import json
    snb = importlib.import_module("openmm-nonbonded-slicing_amd")
    assert argv[1] == "scalar"
    out = {}
    for row, sdf in SCALAR_CASES:
        rec = bulk_case(snb, "lj_big", row, sdf, "single", steps=("ef",))
        out["%s %.1f" % (row, sdf)] = rec
    with open(argv[2], "w") as f:
        json.dump(out, f)
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv))
