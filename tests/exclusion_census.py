"""Exclusion and exception census: the two O(N) pair lists of every Ewald / PME / LJPME step -- the Ewald exclusion corrections and the 1-4
exceptions -- against closed forms (tests/test_exclusion_census.py proves the instrument on the CPU, tests/test_gpu_exclusion_census.py
runs it on the GPU).

Why.  The lists' arithmetic lives in exclusionAtomsBody / exceptionsBody (csrc/direct.hip) and is restated for the tables in pair_energy.h,
atomforce.hip, atom_table.h and grouppairs.hip.  Every other test sees it inside charged lattices whose forces are thousands of kJ/mol/nm,
at three radii, or under a cutoff method where the erf correction does not run.

The systems are gases of isolated molecules.  Every exception is an exclusion and separate molecules are farther apart than cutoff + padding +
0.05 nm, so a direct-space-only evaluation consists of the two lists and nothing else: every force, slice energy and table entry has a
per-pair closed form in float64 (ReferenceSlicedLJCoulombIxn.cpp:449-506, ReferenceSlicedLJCoulomb14.cpp:61-95), evaluated from the
coordinates as given -- the plain difference where exceptions_periodic is false, the minimum image where it is true.  With r_ij = r_i - r_j,
x = alpha r, y = (alpha_d r)^2:

    Coulomb correction   F_i = -lambda_C K q_i q_j g(x) r_ij / r^3,   g(x) = erf(x) - 2 x exp(-x^2) / sqrt(pi);   E = -K q_i q_j erf(x) / r
                         (erf(x) <= 1e-6: E = -2 alpha K q_i q_j / sqrt(pi), no force)
    dispersion (LJPME)   F_i = +lambda_L 6 c6 h4(y) r_ij / r^8,   E = c6 h3(y) / r^6,   c6 = 4 (sigma_i sigma_j)^3 sqrt(eps_i eps_j),
                         h3(y) = 1 - exp(-y) (1 + y + y^2/2),   h4(y) = h3(y) - exp(-y) y^3/6
    1-4 exception        F_i = (lambda_L 4 eps (12 s^12 - 6 s^6) + lambda_C K qq / r) r_ij / r^2,   E = (K qq / r, 4 eps (s^12 - s^6)),  s = sigma / r

g, h3 and h4 cancel for small arguments (g to 0.752 x^3, h4 to y^4 / 24): they are evaluated by series there, in float64 -- the double formula
of g has lost six digits at x = 1e-5, that of h4 all of them at y = 1e-4.

Molecule kinds, in one system so that they share waves (build()):
 1 excluded dimers, a radial scan from 0.08 nm to 1.4 rc with a cluster of separations within 1 % of x = 0.5 (the switch of pair_math.h:
   exclusionG), both charge signs, a zero charge on one end, every slice of three subsets;
 2 close pairs, log-spaced from 0.002 nm (1e-4 nm in double precision) to 0.2 nm, Drude-like: small charges (see the coordinate
   condition below) and epsilon = 0; in double precision two more pairs below and above the erf > 1e-6 threshold, the one below coincident
   (r = 0) on the PME rows;
 3 chains of four, 1-2 and 1-3 excluded, 1-4 an exception with chargeProd and epsilon, 1-4 distances 0.3 .. 1.26 nm, a third of them across
   a face, an edge or the corner;
 4 clusters of a hub and 47 satellites within 0.5 nm, all 1128 pairs excluded;
   14 lone charged atoms, and a lattice of inert filler atoms (q = 0, epsilon = 0) with no exclusion at all, which interact with nothing and
   take the cell over the GPU builder's threshold;
 5 (uncharged=True) a copy of kinds 1, 2 and 4 without charges, sigma 0.1 .. 0.35, epsilon 0.05 .. 0.6, separations 0.05 .. 0.8 nm, for LJPME:
   the dispersion correction at its own scale.

Two conditions on the instrument, asserted by the CPU test: coordinate sensitivity (coordinate_condition) and isolation (isolation_pairs).

Choices the conditions forced.  The cell is 14 nm (125 sites 2.8 nm apart: a 1.4 nm dimer next to another still leaves cutoff + padding +
0.05 nm), so one float ulp of the largest coordinate is 9.5e-7 nm wherever an atom sits: a close pair at 0.002 nm with unit charges would
move by four quarter-bars.  In single and mixed precision the five close pairs below 0.006 nm therefore carry |q| = 0.2 (worst ratio of
the condition 0.64, row R4) and the fifteen from 0.0067 nm to 0.2 nm unit charges (worst ratio 0.57: there the bar is relative and one
ulp is 1.4e-4 of r); in double precision, where the ulp is 1.8e-15 nm, they carry unit charges from 1e-4 nm and the two threshold pairs sit
on ordinary interior sites.  The close pairs have epsilon = 0 on the charged LJPME rows: at 0.002 nm the double closed form of h4 that the
reference and the double kernels use has no digit left, and the dispersion correction is judged on the uncharged copy, from 0.05 nm.  The
GPU builder needs 4 mean block edges + 2 list radii inside the cell, 3800 atoms at this size: the 4096 fillers.
"""
import ctypes
import math
import os
import sys

import numpy as np

# The module is also the program of the census's child process (`python tests/exclusion_census.py standalone OUT.json`), which starts
# without pytest's conftest: the repository root (bench.py, the package), oracle/ and tests/ must be importable before the imports below.
_ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (_ROOT, os.path.join(_ROOT, "oracle"), os.path.join(_ROOT, "tests")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import ewald_census as EC      # noqa: E402
import recip_systems as R
import shell_systems as S

BARS = EC.BARS
K = S.K_COULOMB
PME, LJPME, EWALD = EC.PME, EC.LJPME, EC.EWALD
NSUB = 3
SITES, SPACING = 5, 2.8                      # 125 sites, 14 nm: every coordinate below 16, one float ulp 9.5e-7 nm
LENGTH = SITES * SPACING
TRICLINIC = np.array([[LENGTH, 0.0, 0.0], [1.5, LENGTH, 0.0], [-1.0, 1.9, LENGTH]])      # reduced, b_x, c_x, c_y non-zero, every coordinate still below 16
FILLER = 16                                  # 4096 inert atoms
ISOLATION_EXTRA = 0.05
SERIES_SWITCH = 0.5                          # pair_math.h exclusionG
ERF_THRESHOLD = 1e-6
X_THRESHOLD = 8.862269e-7                    # erf(x) = 1e-6
CLOSE_Q = 0.2                                # |q| of the close pairs below CLOSE_UNIT_FROM in single and mixed precision, from the coordinate condition
CLOSE_UNIT_FROM = 0.006                      # nm: from here on the close pairs carry unit charges in every precision
GROUPS = 7
REROUTING = ("SNB_SCALAR_ENERGY_KERNEL", "SNB_EWALD_ERFC", "SNB_EWALD_POLY_ALWAYS", "SNB_HOST_TRICLINIC")

# (row, method, cell, exceptions_periodic, host builder, uncharged): R0, R2, R4 and R4D, SNB_Ewald on cubes only, both builders, both cells
CASES = [
    ("R0", EWALD, "cubic", 0, 1, False), ("R2", EWALD, "cubic", 1, 0, False), ("R4", EWALD, "cubic", 0, 0, False),
    ("R0", PME, "cubic", 0, 0, False), ("R0", PME, "triclinic", 1, 0, False), ("R0", PME, "triclinic", 0, 1, False),
    ("R2", PME, "cubic", 1, 1, False), ("R2", PME, "triclinic", 0, 0, False),
    ("R4", PME, "cubic", 0, 1, False), ("R4", PME, "cubic", 1, 0, False), ("R4", PME, "triclinic", 1, 0, False),
    ("R4D", LJPME, "cubic", 0, 0, False), ("R4D", LJPME, "cubic", 1, 1, False), ("R4D", LJPME, "triclinic", 1, 1, False), ("R4D", LJPME, "triclinic", 0, 0, False),
    ("R4D", LJPME, "cubic", 0, 0, True), ("R4D", LJPME, "triclinic", 1, 1, True), ("R0", LJPME, "cubic", 1, 0, True),
]
CONTROL_CASES = [c for c in CASES if c[3] == 0 and c[1] != LJPME]      # the hardware control: exceptions_periodic = 1 where 0 is expected
GROUP_TABLE_ROWS = ("R0",)                   # the rows that also run snb_evaluate_group_energies / snb_evaluate_group_forces


def case_id(c):
    return "%s-%s-%s-p%d-%s%s" % (c[0], {EWALD: "ewald", PME: "pme", LJPME: "ljpme"}[c[1]], c[2], c[3], "host" if c[4] else "gpu", "-uncharged" if c[5] else "")


def rerouted():
    return any(k in os.environ for k in REROUTING)


def sl(i, j):
    return max(i, j) * (max(i, j) + 1) // 2 + min(i, j)


def lambdas():
    """(Coulomb, vdW) per slice: twelve distinct values, none of them 0 or 1."""
    S_ = NSUB * (NSUB + 1) // 2
    return np.array([[0.35 + 0.1 * k, 0.92 - 0.08 * k] for k in range(S_)])


# ---- the radial functions, float64 --------------------------------------------------------------------------------------------------
_erf = np.vectorize(math.erf, otypes=[np.float64])


def g_series(x, nterms=14):
    """(4 / sqrt(pi)) x^3 sum_n (-1)^n x^(2n) / (n! (2n + 3))."""
    x = np.asarray(x, dtype=np.float64)
    x2 = x * x
    s = np.zeros_like(x); p = np.ones_like(x)
    for n in range(nterms):
        s += p / (2 * n + 3)
        p = -p * x2 / (n + 1)
    return 4.0 / math.sqrt(math.pi) * x * x2 * s


def g_formula(x):
    x = np.asarray(x, dtype=np.float64)
    return _erf(x) - 2.0 * x * np.exp(-x * x) / math.sqrt(math.pi)


def g(x, nterms=None):
    """g(x); nterms: the planted defect, the series below the switch truncated."""
    x = np.asarray(x, dtype=np.float64)
    small = x < SERIES_SWITCH
    return np.where(small, g_series(np.where(small, x, 0.0), 14 if nterms is None else nterms), g_formula(x))


def h_series(y, first):
    """exp(-y) sum_{k >= first} y^k / k!  =  1 - exp(-y) sum_{k < first} y^k / k!: every term positive."""
    y = np.asarray(y, dtype=np.float64)
    t = y ** first / math.factorial(first)
    s = np.zeros_like(y)
    for k in range(first, first + 40):
        s += t
        t = t * y / (k + 1)
    return np.exp(-y) * s


def h_formula(y, first):
    y = np.asarray(y, dtype=np.float64)
    return 1.0 - np.exp(-y) * sum(y ** k / math.factorial(k) for k in range(first))


def h(y, first):
    y = np.asarray(y, dtype=np.float64)
    small = y < 2.0
    return np.where(small, h_series(np.where(small, y, 0.0), first), h_formula(y, first))


# ---- the systems ---------------------------------------------------------------------------------------------------------------------
def _unit(rng, n=1):
    u = rng.normal(size=(n, 3))
    return u / np.linalg.norm(u, axis=1)[:, None]


def dimer_radii(alpha, rc):
    """55 separations: 0.08 nm .. 1.4 rc, through and beyond the cutoff, and seven within 1 % of alpha r = 0.5."""
    around = 0.5 / alpha * (1.0 + np.array([-1e-2, -3e-3, -1e-4, 0.0, 1e-4, 3e-3, 1e-2]))
    scan = np.concatenate([np.geomspace(0.08, 0.9 * rc, 34), rc * np.array([0.97, 0.995, 0.9999, 1.0001, 1.005, 1.03, 1.1, 1.2, 1.3, 1.4])])
    return np.concatenate([around, scan[:48]])


def build(row, method, precision, cell="cubic", periodic=0, uncharged=False, seed=5):
    """The census system of a row: a record of shell_systems.make_system with the Ewald parameters, the exceptions, and per atom `mol`
    (molecule, -1: filler), `kind` (1 .. 4, 0: lone or filler); `crossers`: (atom, axis) of the straddling chains' atoms that sit 0.01 nm
    inside a face (measured along the cell's axis)."""
    key = (row, method, precision, cell, int(periodic), bool(uncharged), seed)
    if key in _BUILT:
        return _BUILT[key]
    rw = EC.row_of(row)
    rc, alpha, alpha_d = rw["cutoff"], rw["alpha"], rw.get("alpha_d", rw["alpha"])
    rng = np.random.default_rng(seed)
    dbl = precision == "double"
    box = np.diag([LENGTH] * 3) if cell == "cubic" else TRICLINIC
    sites = np.stack(np.meshgrid(np.arange(SITES), np.arange(SITES), np.arange(SITES), indexing="ij"), -1).reshape(-1, 3)
    on_face = (sites == 0).any(axis=1)
    outer = [tuple(t) for t in sites[on_face]]
    inner = [tuple(t) for t in sites[~on_face]]
    inner = [inner[k] for k in rng.permutation(len(inner))]
    # the straddling chains: the corner, the three edges, six faces
    strad = [(0, 0, 0), (0, 0, 2), (0, 3, 0), (1, 0, 0), (0, 2, 3), (0, 4, 1), (3, 0, 2), (1, 0, 4), (2, 3, 0), (4, 1, 0)]
    outer = [t for t in outer if t not in strad]
    outer = [outer[k] for k in rng.permutation(len(outer))]
    mols = []          # (kind, site, offsets [m][3], q [m], sigma, epsilon, subset [m], pairs [(a, b, qq, sigma, eps)], crosser or None)

    def lj(m):
        return rng.uniform(0.1, 0.35, m), rng.uniform(0.05, 0.6, m)

    # kind 1: dimers
    radii = np.concatenate([np.geomspace(0.05, 0.8, 30), 0.5 / alpha_d * np.array([0.7, 1.0, 1.4])]) if uncharged else dimer_radii(alpha, rc)
    combos = [(i, j) for i in range(NSUB) for j in range(i + 1)]
    for k, r in enumerate(radii):
        u = _unit(rng)[0]
        q = np.array([rng.choice([1.0, 0.5]), rng.choice([1.0, -1.0, 0.5, -0.5])])
        if k % 9 == 4:
            q[1] = 0.0
        sg, ep = lj(2)
        mols.append((1, None, np.array([-0.5 * r * u, 0.5 * r * u]), q, sg, ep, np.array(combos[k % 6]), [(0, 1, 0.0, 0.3, 0.0)], None))
    # kind 2: close pairs
    close = np.geomspace(0.05, 0.2, 8) if uncharged else np.geomspace(1e-4 if dbl else 2e-3, 0.2, 20)
    for k, r in enumerate(close):
        qc = 1.0 if (dbl or r >= CLOSE_UNIT_FROM) else CLOSE_Q
        u = _unit(rng)[0]
        sg, ep = lj(2)
        if not uncharged:
            ep = np.zeros(2)
        mols.append((2, "inner", np.array([np.zeros(3), r * u]), np.array([qc, -qc if k % 3 else qc]), sg, ep, np.array(combos[(k + 2) % 6]), [(0, 1, 0.0, 0.3, 0.0)], None))
    if dbl and not uncharged:
        thr = X_THRESHOLD / alpha
        for r in (0.0 if method == PME else 0.8 * thr, 1.25 * thr):
            mols.append((2, "inner", np.array([np.zeros(3), [r, 0.0, 0.0]]), np.array([1.0, -1.0]), np.full(2, 0.3), np.zeros(2), np.array([1, 0]), [(0, 1, 0.0, 0.3, 0.0)], None))
    # kind 3: chains of four
    if not uncharged:
        for k in range(30):
            b = (0.2, 0.16, 0.25, 0.34, 0.42)[k % 5] if k < len(strad) else (0.1, 0.16, 0.25, 0.34, 0.42)[k % 5]
            site = strad[k] if k < len(strad) else "inner"
            if k < len(strad):
                zero = np.array(site) == 0
                u = zero * 1.0 + rng.normal(0.0, 0.15, 3)
                u /= np.linalg.norm(u)
            else:
                u = _unit(rng)[0]
            off = np.outer(np.array([-1.5, -0.5, 0.5, 1.5]) * b, u) + rng.normal(0.0, 0.02, (4, 3))
            crosser = None
            if k < len(strad):
                ax = int(np.argmax(zero))
                fo = off @ np.linalg.inv(box) * LENGTH         # in units of the cell's axes (the faces of a triclinic cell are oblique)
                fo = fo - fo[1] * zero                         # atom 1 onto the corner / edge / face ...
                fo[:, ax] += 0.01                              # ... and 0.01 nm inside along the first straddled axis
                assert (fo[0][zero] < -0.03).all() and fo[1, ax] > 0
                off = fo / LENGTH @ box
                crosser = (1, ax)
            q = rng.choice([0.4, -0.4, 0.8, -0.6], 4)
            sg, ep = lj(4)
            pairs = [(0, 1, 0.0, 0.3, 0.0), (1, 2, 0.0, 0.3, 0.0), (2, 3, 0.0, 0.3, 0.0), (0, 2, 0.0, 0.3, 0.0), (1, 3, 0.0, 0.3, 0.0),
                     (0, 3, 0.8333 * q[0] * q[3], rng.uniform(0.2, 0.35), rng.uniform(0.1, 0.5))]
            mols.append((3, site, off, q, sg, ep, (k + np.array([0, 1, 2, 0])) % NSUB, pairs, crosser))
    # kind 4: clusters
    for k in range(8):
        while True:
            sat = _unit(rng, 47) * np.cbrt(rng.uniform(0.02, 1.0, 47))[:, None] * 0.5
            off = np.concatenate([np.zeros((1, 3)), sat])
            dd = np.linalg.norm(off[:, None] - off[None], axis=-1) + np.eye(48)
            if dd.min() > 0.06:
                break
        q = rng.choice([0.3, -0.3, 0.6, -0.5, 0.0], 48)
        q[0] = 0.6
        sg, ep = lj(48)
        pairs = [(a, b, 0.0, 0.3, 0.0) for a in range(48) for b in range(a + 1, 48)]
        mols.append((4, "inner", off, q, sg, ep, rng.integers(0, NSUB, 48), pairs, None))
    # lone charged atoms
    for k in range(14):
        sg, ep = lj(1)
        mols.append((0, None, np.zeros((1, 3)), np.array([rng.choice([1.0, -1.0])]), sg, ep, np.array([k % NSUB]), [], None))
    # sites: kind 2 and 4 and the other chains inside, the rest wherever a site is left (the outer ones first: their bonds cross faces)
    free_inner, free_outer = list(inner), list(outer)
    placed = []
    for m in mols:
        if isinstance(m[1], tuple):
            placed.append(m[1])
        elif m[1] == "inner":
            placed.append(free_inner.pop())
        else:
            placed.append(None)
    for k, m in enumerate(mols):
        if placed[k] is None:
            placed[k] = free_outer.pop() if free_outer else free_inner.pop()
    # fillers
    fil = (np.stack(np.meshgrid(np.arange(FILLER), np.arange(FILLER), np.arange(FILLER), indexing="ij"), -1).reshape(-1, 3) + 0.5) / FILLER
    fil = (fil + rng.uniform(-0.2, 0.2, fil.shape) / FILLER) @ box
    if (sum(len(m[3]) for m in mols) + len(fil)) % 32 == 0:      # the atom count must not be a multiple of 32
        fil = fil[:-1]
    order = rng.permutation(len(mols) + len(fil))
    pos, q, sg, ep, sub, mol, kind, exc, crossers = [], [], [], [], [], [], [], [], []
    n = 0
    for o in order:
        if o >= len(mols):
            pos.append(fil[o - len(mols)][None]); q.append([0.0]); sg.append([0.3]); ep.append([0.0]); sub.append([int(o) % NSUB]); mol.append([-1]); kind.append([0])
            n += 1
            continue
        kd, _, off, mq, msg, mep, msub, pairs, crosser = mols[o]
        centre = (np.array(placed[o]) / SITES) @ box
        pos.append(centre + off); q.append(np.zeros(len(mq)) if uncharged else mq); sg.append(msg); ep.append(mep if method == LJPME else np.zeros(len(mq)))
        sub.append(msub); mol.append(np.full(len(mq), o)); kind.append(np.full(len(mq), kd))
        exc += [(n + a, n + b, 0.0 if uncharged else qq, s14, 0.0 if uncharged else e14) for a, b, qq, s14, e14 in pairs]
        if crosser is not None:
            crossers.append((n + crosser[0], crosser[1]))
        n += len(mq)
    pos = np.concatenate(pos)
    if n % 32 == 0:
        raise AssertionError("the atom count must not be a multiple of 32")
    frac = pos @ np.linalg.inv(box)
    pos = (frac - np.floor(frac)) @ box
    s = S.make_system("exclusions_%s" % case_id((row, method, cell, periodic, 0, uncharged)), pos, box, np.concatenate(q), np.concatenate(sub), NSUB, rc=rc)
    s["pos"] = np.ascontiguousarray(pos) if dbl else S.to_float(pos)
    s.update(method=method, alpha=alpha, alpha_d=alpha_d, grid=(32, 32, 32), dgrid=(32, 32, 32) if method == LJPME else (0, 0, 0), kmax=EC.EWALD_KMAX if method == EWALD else (0, 0, 0),
             sigma=np.concatenate(sg), epsilon=np.concatenate(ep), lam=lambdas(), exceptions_periodic=bool(periodic), topology="molecules",
             mol=np.concatenate(mol), kind=np.concatenate(kind), crossers=crossers, row=row, precision=precision, padding=rw["padding"], uncharged=bool(uncharged))
    e = np.array(exc)
    s["exc_pairs"] = np.ascontiguousarray(e[:, :2], dtype=np.int32); s["exc_qq"] = np.ascontiguousarray(e[:, 2]); s["exc_sigma"] = np.ascontiguousarray(e[:, 3]); s["exc_eps"] = np.ascontiguousarray(e[:, 4])
    _BUILT[key] = s
    return s


_BUILT = {}


def carriers(s):
    return (s["q"] != 0) | (s["epsilon"] != 0) | (s["mol"] >= 0)


def isolation_pairs(s, pos=None):
    """The non-excluded pairs within cutoff + padding + 0.05 nm among the atoms that carry anything (the fillers have q = 0 and
    epsilon = 0: whatever pair they are in is exactly zero), by the oracle's pair diagnostic: must be empty."""
    keep = np.nonzero(carriers(s))[0]
    new = -np.ones(len(s["q"]), dtype=np.int64); new[keep] = np.arange(len(keep))
    t = dict(s)
    for k in ("q", "sigma", "epsilon", "subset"):
        t[k] = np.ascontiguousarray(s[k][keep])
    t["pos"] = np.ascontiguousarray((s["pos"] if pos is None else pos)[keep])
    t["exc_pairs"] = np.ascontiguousarray(new[s["exc_pairs"]], dtype=np.int32)
    t["method"] = 2; t["exceptions_periodic"] = True
    ij, r, _ = S.pairs_in_range(t, 1e-3, s["rc"] + s["padding"] + ISOLATION_EXTRA)
    return keep[ij], r


# ---- the closed form -------------------------------------------------------------------------------------------------------------------
def pair_terms(s, pos=None, periodic=None, q=None, exc=None, defect=None):
    """Per exception pair, from the coordinates as given: i, j, d = r_i - r_j [P][3], r, slice, the force coefficients (F_i += lambda c d,
    F_j -= lambda c d) and raw energies of the Coulomb part (correction + 1-4) and the vdW part (dispersion correction + 1-4), the
    correction's and the exception's apart: cC, c14C, cL, c14L, eC, eL.  q: other charges; exc: other (chargeProd, sigma, epsilon) of the exceptions (the
    parameter-offset pass).  defect: 'image', 'series3', 'lj6', 'dropped' (the planted defects of the CPU control; 'lambda' acts in forces())."""
    pos = s["pos"] if pos is None else np.asarray(pos)
    q = s["q"] if q is None else q
    qq14, sg14, ep14 = (s["exc_qq"], s["exc_sigma"], s["exc_eps"]) if exc is None else exc
    i, j = s["exc_pairs"][:, 0].astype(np.int64), s["exc_pairs"][:, 1].astype(np.int64)
    per = bool(s["exceptions_periodic"]) if periodic is None else bool(periodic)
    d = pos[i] - pos[j]
    if per or defect == "image":
        d = S._min_image(s, d)
    r = np.linalg.norm(d, axis=1)
    alpha, alpha_d = s["alpha"], s["alpha_d"]
    x = alpha * r
    qq = K * q[i] * q[j]
    with np.errstate(divide="ignore", invalid="ignore"):
        has_force = _erf(x) > ERF_THRESHOLD
        cC = np.where(has_force, -qq * g(x, 3 if defect == "series3" else None) / r ** 3, 0.0)
        eC = np.where(has_force, -qq * _erf(x) / r, -2.0 * alpha * qq / math.sqrt(math.pi))
        cL = np.zeros_like(r); eL = np.zeros_like(r)
        if s["method"] == LJPME:
            c6 = 4.0 * (s["sigma"][i] * s["sigma"][j]) ** 3 * np.sqrt(s["epsilon"][i] * s["epsilon"][j])
            y = (alpha_d * r) ** 2
            cL = np.where(c6 != 0, 6.0 * c6 * h(y, 4) / r ** 8, 0.0)
            eL = np.where(c6 != 0, c6 * h(y, 3) / r ** 6, 0.0)
        is14 = (qq14 != 0) | (ep14 != 0)
        s6 = np.where(is14, (sg14 / r) ** 6, 0.0)
        c14L = np.where(is14, 4.0 * ep14 * ((6.0 if defect == "lj6" else 12.0) * s6 - 6.0) * s6 / r ** 2, 0.0)
        c14C = np.where(is14, K * qq14 / r ** 3, 0.0)
        e14L = np.where(is14, 4.0 * ep14 * (s6 - 1.0) * s6, 0.0)
        e14C = np.where(is14, K * qq14 / r, 0.0)
    t = dict(i=i, j=j, d=d, r=r, x=x, slice=np.array([sl(a, b) for a, b in zip(s["subset"][i], s["subset"][j])]),
             cC=cC, c14C=c14C, cL=cL, c14L=c14L, eC=eC + e14C, eL=eL + e14L)
    if defect == "dropped":      # one satellite dropped from the first hub's list
        k = dropped_pair(s)
        for key in ("cC", "c14C", "cL", "c14L", "eC", "eL"):
            t[key] = t[key].copy(); t[key][k] = 0.0
    return t


def dropped_pair(s):
    hub = int(np.nonzero(s["kind"] == 4)[0][0])
    mine = np.nonzero(s["exc_pairs"][:, 0] == hub)[0]
    if s["uncharged"]:
        return int(mine[5])
    return int(mine[np.nonzero(s["q"][s["exc_pairs"][mine, 1]] != 0)[0][2]])


def forces(s, t, lam=None, defect=None):
    """F [N][3] at the lambdas."""
    lam = s["lam"] if lam is None else lam
    lc = lam[t["slice"], 1 if defect == "lambda" else 0]
    c = lc * t["cC"] + lam[t["slice"], 0] * t["c14C"] + lam[t["slice"], 1] * (t["cL"] + t["c14L"])
    f = np.zeros((len(s["q"]), 3))
    np.add.at(f, t["i"], c[:, None] * t["d"]); np.add.at(f, t["j"], -c[:, None] * t["d"])
    return f


def slice_energies(s, t):
    e = np.zeros((len(s["lam"]), 2))
    np.add.at(e[:, 0], t["slice"], t["eC"]); np.add.at(e[:, 1], t["slice"], t["eL"])
    return e


def atom_energy_table(s, t):
    """A[a][J] = (Coulomb, vdW): the raw energies of atom a's pairs with the atoms of subset J."""
    A = np.zeros((len(s["q"]), NSUB, 2))
    for a, b in ((t["i"], t["j"]), (t["j"], t["i"])):
        np.add.at(A[:, :, 0], (a, s["subset"][b]), t["eC"]); np.add.at(A[:, :, 1], (a, s["subset"][b]), t["eL"])
    return A


def atom_force_table(s, t):
    """G[a][J][term]: the force on atom a from its pairs with the atoms of subset J, every lambda 1."""
    G = np.zeros((len(s["q"]), NSUB, 2, 3))
    for a, b, sign in ((t["i"], t["j"], 1.0), (t["j"], t["i"], -1.0)):
        np.add.at(G[:, :, 0], (a, s["subset"][b]), sign * (t["cC"] + t["c14C"])[:, None] * t["d"])
        np.add.at(G[:, :, 1], (a, s["subset"][b]), sign * (t["cL"] + t["c14L"])[:, None] * t["d"])
    return G


def group_labels(n):
    """Labels -1 .. GROUPS - 1 that follow neither the subsets nor the molecules: runs of three atoms, every eighth run unlabelled."""
    return ((np.arange(n) // 3) % (GROUPS + 1) - 1).astype(np.int32)


def group_pair_matrix(s, t, lab):
    M = np.zeros((GROUPS * (GROUPS + 1) // 2, 2))
    a, b = lab[t["i"]], lab[t["j"]]
    k = (a >= 0) & (b >= 0)
    row = np.array([sl(x, y) for x, y in zip(a[k], b[k])], dtype=np.int64)
    np.add.at(M[:, 0], row, t["eC"][k]); np.add.at(M[:, 1], row, t["eL"][k])
    return M


def groups_of(lab):
    return [np.nonzero(lab == g)[0] for g in range(GROUPS)]


def expected(s, pos=None, periodic=None, q=None, exc=None, defect=None):
    t = pair_terms(s, pos, periodic, q, exc, defect)
    return dict(terms=t, forces=forces(s, t, defect=defect), energies=slice_energies(s, t))


def partners(s, t, a):
    """The partner of atom a with the largest pair force: (b, r, alpha r)."""
    k = np.nonzero((t["i"] == a) | (t["j"] == a))[0]
    if len(k) == 0:
        return (-1, float("nan"), float("nan"))
    c = np.abs(t["cC"] + t["c14C"] + t["cL"] + t["c14L"])[k] * t["r"][k]
    m = k[int(np.nanargmax(np.nan_to_num(c)))]
    return (int(t["j"][m] if t["i"][m] == a else t["i"][m]), float(t["r"][m]), float(t["x"][m]))


# ---- the comparison --------------------------------------------------------------------------------------------------------------------
def force_floor(s, fexp):
    """1 kJ/mol/nm on the charged systems (ewald_census.dimer_case); on the uncharged copy the median non-zero |F_exp| (vdw_census)."""
    if not s["uncharged"]:
        return 1.0
    fn = np.linalg.norm(fexp, axis=1)
    return float(np.median(fn[fn > 0]))


def compare_forces(s, f, fexp, tol, floor=None):
    """|F - F_exp| / max(|F_exp|, floor) per atom: {'err' [N], 'flagged': atoms over tol, 'zero_ok': atoms with no expected contribution have
    exactly zero force, 'worst'}."""
    f = np.asarray(f, dtype=np.float64)
    floor = force_floor(s, fexp) if floor is None else floor
    fn = np.linalg.norm(fexp, axis=1)
    err = np.linalg.norm(f - fexp, axis=1) / np.maximum(fn, floor)
    none = ~(fexp != 0).any(axis=1)
    bad = ~(err <= tol)
    return dict(err=err, flagged=np.nonzero(bad)[0], zero_ok=bool((f[none] == 0).all()), worst=int(np.nanargmax(np.where(np.isnan(err), np.inf, err))), floor=floor,
                max_err=float(np.max(np.where(np.isnan(err), np.inf, err))))


def describe(s, t, a):
    b, r, x = partners(s, t, a)
    return "atom %d (kind %d, q %+.2f), partner %d, r = %.6g nm, alpha r = %.4g" % (a, s["kind"][a], s["q"][a], b, r, x)


def coordinate_condition(s, tol, pos=None):
    """Moving any one coordinate of an atom by one ulp of the largest coordinate in the cell (a float ulp in single and mixed precision, a
    double ulp where the engine is given doubles) must change the atom's expected force by less than a quarter of its bar.  The lists are
    linear in the pairs, so the change is the sum over the atom's pairs of the pair force's derivative: evaluated by moving, per axis, every
    atom i of a pair (the partner then sees the same change).  Returns the worst ratio change / (tol max(|F|, floor) / 4) and its atom."""
    pos = s["pos"] if pos is None else pos
    big = float(np.abs(pos).max())
    ulp = float(np.spacing(big)) if s["precision"] == "double" else float(np.spacing(np.float32(big)))
    step = max(ulp, 1e-9)           # (numerical derivative in float64: the change is linear in the step up to where r itself is a few steps)
    base = expected(s, pos)
    f0 = base["forces"]; t0 = base["terms"]
    bar = 0.25 * tol * np.maximum(np.linalg.norm(f0, axis=1), force_floor(s, f0))
    worst = np.zeros(len(pos))
    c0 = s["lam"][t0["slice"], 0] * (t0["cC"] + t0["c14C"]) + s["lam"][t0["slice"], 1] * (t0["cL"] + t0["c14L"])
    f0p = c0[:, None] * t0["d"]
    for ax in range(3):
        # every pair with its i-atom moved: the change of that pair's force is the change of both atoms' forces from this pair
        d = t0["d"].copy(); d[:, ax] += step
        moved = _pair_force(s, t0, d)
        dfp = (moved - f0p) * (ulp / step)
        acc = np.zeros((len(pos), 3))
        np.add.at(acc, t0["i"], dfp); np.add.at(acc, t0["j"], dfp)      # the moved atom: all its pairs change (to first order alike from either end)
        one = np.zeros(len(pos)); n1 = np.linalg.norm(dfp, axis=1)
        np.maximum.at(one, t0["i"], n1); np.maximum.at(one, t0["j"], n1)      # its partners: the one pair
        worst = np.maximum(worst, np.maximum(np.linalg.norm(acc, axis=1), one))
    ratio = worst / bar
    a = int(np.argmax(ratio))
    return float(ratio[a]), a, ulp


def _pair_force(s, t0, d):
    """lambda c(r) d of every pair at other separations (coordinate_condition)."""
    r = np.linalg.norm(d, axis=1)
    x = s["alpha"] * r
    i, j = t0["i"], t0["j"]
    qq = K * s["q"][i] * s["q"][j]
    lam = s["lam"][t0["slice"]]
    with np.errstate(divide="ignore", invalid="ignore"):
        c = np.where(_erf(x) > ERF_THRESHOLD, -lam[:, 0] * qq * g(x) / r ** 3, 0.0)
        if s["method"] == LJPME:
            c6 = 4.0 * (s["sigma"][i] * s["sigma"][j]) ** 3 * np.sqrt(s["epsilon"][i] * s["epsilon"][j])
            c = c + np.where(c6 != 0, lam[:, 1] * 6.0 * c6 * h((s["alpha_d"] * r) ** 2, 4) / r ** 8, 0.0)
        is14 = (s["exc_qq"] != 0) | (s["exc_eps"] != 0)
        s6 = np.where(is14, (s["exc_sigma"] / r) ** 6, 0.0)
        c = c + np.where(is14, (lam[:, 1] * 4.0 * s["exc_eps"] * (12.0 * s6 - 6.0) * s6 + lam[:, 0] * K * s["exc_qq"] / r) / r ** 2, 0.0)
    return np.nan_to_num(c)[:, None] * d


def straddling_atoms(s, pos=None):
    """The atoms of the pairs whose minimum image is not the plain difference, and all atoms of their molecules."""
    pos = s["pos"] if pos is None else pos
    i, j = s["exc_pairs"][:, 0], s["exc_pairs"][:, 1]
    d = pos[i] - pos[j]
    crossing = np.linalg.norm(S._min_image(s, d) - d, axis=1) > 1e-9
    mols = np.unique(s["mol"][i[crossing]])
    return np.nonzero(np.isin(s["mol"], mols) & (s["mol"] >= 0))[0]


def control_atoms(s, pos=None):
    """The atoms the hardware control must flag: those of the straddling molecules that take part in a pair with a non-zero term (rows
    without LJPME: a pair that has its dispersion term alone moves by less than a bar)."""
    assert s["method"] != LJPME
    t = pair_terms(s, pos)
    k = (t["cC"] != 0) | (t["c14C"] != 0) | (t["c14L"] != 0)
    active = np.zeros(len(s["q"]), dtype=bool)
    active[t["i"][k]] = True; active[t["j"][k]] = True
    strad = straddling_atoms(s, pos)
    return strad[active[strad]]


# ---- frames ------------------------------------------------------------------------------------------------------------------------------
def frames(s, count=3, seed=11):
    """Frame 0 is the system; the others move every molecule rigidly by a seeded step of at most 0.012 nm per axis from frame 0 (well inside
    padding / 2; rigid, so that no close pair changes its separation by more than rounding) and, the close pairs aside, every atom by a
    further 1e-3 nm.  The last frame is `crossed`: frame 0 with the crossers of the straddling chains moved 0.02 nm through their face."""
    rng = np.random.default_rng(seed)
    conv = (lambda p: np.ascontiguousarray(p)) if s["precision"] == "double" else S.to_float
    out = [s["pos"]]
    nm = int(s["mol"].max()) + 1
    for _ in range(count - 1):
        shift = np.clip(rng.normal(0.0, 0.005, (nm + 1, 3)), -0.012, 0.012)
        p = s["pos"] + shift[s["mol"]] * (s["mol"] >= 0)[:, None]
        p = p + np.where((s["kind"] != 2)[:, None], np.clip(rng.normal(0.0, 1e-3, p.shape), -3e-3, 3e-3), 0.0)
        out.append(conv(p))
    p = s["pos"].copy()
    for a, ax in s["crossers"]:
        p[a] -= 0.02 * s["box"][ax] / s["box"][ax, ax]
    return out, conv(p)


# ---- the engine ------------------------------------------------------------------------------------------------------------------------
_ip = lambda a: a.ctypes.data_as(ctypes.POINTER(ctypes.c_int32))


class Engine(R.Engine):
    """recip_systems.Engine, direct space alone, a rebuild interval that no case reaches; eager: disable_graph = 1; periodic: the engine's
    exceptions_periodic where it is not the record's (the hardware control)."""

    def __init__(self, snb, s, precision, host_build=0, eager=False, periodic=None):
        self._eager = eager
        if periodic is not None:
            s = dict(s); s["exceptions_periodic"] = bool(periodic)
        super().__init__(snb, s, precision, direct=1, padding=s["padding"], interval=100, host_build=host_build)
        self.recip = 0

    def configure(self, cfg):
        super().configure(cfg)
        cfg.disable_graph = int(self._eager)

    def set_positions(self, pos):
        self._pos = np.ascontiguousarray(pos, dtype=np.float64)
        self.ok(self.L.snb_set_positions(self.h, self._pos.ctypes.data_as(ctypes.c_void_p), 0, 1, 0))

    def set_offsets(self, atoms, dq, excs, dexc):
        """One global parameter: charge deltas on `atoms`, (chargeProd, sigma, epsilon) deltas on the exceptions `excs`."""
        pa = np.ascontiguousarray(atoms, dtype=np.int32); pg = np.zeros(len(pa), dtype=np.int32)
        pd = np.ascontiguousarray(np.stack([dq, np.zeros(len(pa)), np.zeros(len(pa))], axis=1))
        ea = np.ascontiguousarray(excs, dtype=np.int32); eg = np.zeros(len(ea), dtype=np.int32); ed = np.ascontiguousarray(dexc, dtype=np.float64)
        self.ok(self.L.snb_set_parameter_offsets(self.h, 1, len(pa), _ip(pa), _ip(pg), S._dp(pd), len(ea), _ip(ea), _ip(eg), S._dp(ed)))

    def set_global(self, value):
        v = np.array([value], dtype=np.float64)
        self.ok(self.L.snb_set_global_parameters(self.h, 1, S._dp(v)))

    def step_derivative(self, mask):
        m = np.ascontiguousarray(mask, dtype=np.int32)
        self.ok(self.L.snb_set_energy_slices(self.h, _ip(m)))
        self.ok(self.L.snb_execute(self.h, 1, 2, self.direct, self.recip, None))
        return self.forces(), self.slice_energies()

    def step_energy_only_masked(self, mask):
        """An energy-only step on the slices of `mask` (include_forces = 0, include_energy = 2): the FORCES = false list bodies with
        sliceNeed zero on some slices, i.e. their `!wantE` skip."""
        m = np.ascontiguousarray(mask, dtype=np.int32)
        self.ok(self.L.snb_set_energy_slices(self.h, _ip(m)))
        self.ok(self.L.snb_execute(self.h, 0, 2, self.direct, self.recip, None))
        return self.slice_energies()

    def all_slices(self):
        self.ok(self.L.snb_set_energy_slices(self.h, _ip(np.ones(len(self.s["lam"]), dtype=np.int32))))

    def atom_energies(self):
        out = np.full((self.n, NSUB, 2), np.nan)
        self.ok(self.L.snb_evaluate_atom_energies(self.h, 1, 0, out.ctypes.data_as(ctypes.c_void_p), 0))
        return out

    def atom_forces(self):
        out = np.full((self.n, NSUB, 2, 3), np.nan)
        self.ok(self.L.snb_evaluate_atom_forces(self.h, 1, 0, out.ctypes.data_as(ctypes.c_void_p), 0))
        return out

    def group_pairs(self, lab):
        lab = np.ascontiguousarray(lab, dtype=np.int32)
        out = np.full((GROUPS * (GROUPS + 1) // 2, 2), np.nan)
        b = self.capi.SnbGroupPairBatch()
        b.n_frames = 1; b.n_groups = GROUPS; b.group_of_atom = _ip(lab); b.pair_energies = out.ctypes.data_as(ctypes.c_void_p); b.out_is_device = 0
        self.ok(self.L.snb_evaluate_group_pair_energies(self.h, ctypes.byref(b)))
        return out

    def _groups(self, b, groups):
        start = np.zeros(len(groups) + 1, dtype=np.int32); start[1:] = np.cumsum([len(g) for g in groups])
        atoms = np.ascontiguousarray(np.concatenate(groups), dtype=np.int32)
        b.n_frames = 1; b.include_direct = 1; b.include_reciprocal = 0; b.n_groups = len(groups); b.group_start = _ip(start); b.group_atoms = _ip(atoms); b.out_is_device = 0
        return start, atoms

    def group_energies(self, groups):
        out = np.full((len(groups), NSUB, 2), np.nan)
        b = self.capi.SnbGroupBatch()
        keep = self._groups(b, groups)
        b.group_energies = out.ctypes.data_as(ctypes.c_void_p)
        self.ok(self.L.snb_evaluate_group_energies(self.h, ctypes.byref(b)))
        del keep
        return out

    def group_forces(self, groups):
        out = np.full((len(groups), NSUB, 2, 3), np.nan)
        b = self.capi.SnbGroupForceBatch()
        keep = self._groups(b, groups)
        b.group_forces = out.ctypes.data_as(ctypes.c_void_p); b.n_states = 0
        self.ok(self.L.snb_evaluate_group_forces(self.h, ctypes.byref(b)))
        del keep
        return out


# ---- a case on the GPU -------------------------------------------------------------------------------------------------------------------
MASK_A = (sl(1, 0), sl(2, 2))
MASK_B = (sl(0, 0), sl(2, 1), sl(2, 0))


def offset_plan(s):
    """The parameter-offset pass: charge deltas (+0.3 and -0.25 in turn) on the second atom of every third molecule among the dimers
    and chains, chargeProd (+0.2) and epsilon (+0.15) deltas on every second 1-4 exception, per unit of the one global parameter."""
    first = []
    for m in np.unique(s["mol"][(s["kind"] == 1) | (s["kind"] == 3)])[::3]:
        first.append(int(np.nonzero(s["mol"] == m)[0][1]))
    atoms = np.array(first, dtype=np.int32)
    dq = np.where(np.arange(len(atoms)) % 2 == 0, 0.3, -0.25)
    excs = np.nonzero((s["exc_qq"] != 0) | (s["exc_eps"] != 0))[0][::2].astype(np.int32)
    dexc = np.stack([np.full(len(excs), 0.2), np.zeros(len(excs)), np.full(len(excs), 0.15)], axis=1) if len(excs) else np.zeros((0, 3))
    return atoms, dq, excs, dexc


def at_global(s, plan, value):
    """(charges, (chargeProd, sigma, epsilon)) at a value of the global parameter."""
    atoms, dq, excs, dexc = plan
    q = s["q"].copy(); q[atoms] += value * dq
    qq, sg, ep = s["exc_qq"].copy(), s["exc_sigma"].copy(), s["exc_eps"].copy()
    if len(excs):
        qq[excs] += value * dexc[:, 0]; sg[excs] += value * dexc[:, 1]; ep[excs] += value * dexc[:, 2]
    return q, (qq, sg, ep)


def run_case(snb, case, prec, engine_periodic=None, steps="all"):
    """Every step of the census on one case: {'checks': [(step, error in units of the bar's denominator, detail)], 'finite', 'zero_ok',
    'flagged': {step: atoms over the bar}, 'host_rebuilds', 'rebuilds', 'overruns'}.  engine_periodic: the hardware control -- the engine's
    exceptions_periodic, the expected values stay those of the record."""
    row, method, cell, periodic, host, uncharged = case
    s = build(row, method, prec, cell, periodic, uncharged)
    tol = BARS[prec]
    checks, flagged = [], {}
    state = dict(finite=True, zero=True, coulomb=0.0)

    def fcheck(step, f, ex):
        rec = compare_forces(s, f, ex["forces"], tol)
        state["finite"] &= bool(np.isfinite(f).all()); state["zero"] &= rec["zero_ok"]
        flagged[step] = rec["flagged"]
        checks.append((step, rec["max_err"], describe(s, ex["terms"], rec["worst"])))

    def echeck(step, got, want, detail, entry=None):
        got = np.asarray(got, dtype=np.float64)
        state["finite"] &= bool(np.isfinite(got).all())
        if got.ndim >= 2:      # (Coulomb, vdW) on the last axis
            state["coulomb"] = max(state["coulomb"], float(np.abs(got[..., 0]).max()))
        want = np.asarray(want, dtype=np.float64)
        if np.isfinite(got).all() and got.size:
            e = np.abs(got - want) / np.maximum(np.abs(want), 1.0)
            k = np.unravel_index(int(np.argmax(e)), e.shape)
            detail = "%s: worst entry %s, got %.9g, expected %.9g%s" % (detail, list(int(x) for x in k), got[k], want[k], entry(k) if entry else "")
        checks.append((step, EC.rel(got, want) if np.isfinite(got).all() else float("inf"), detail))

    fr, crossed = frames(s)
    if steps == "all":
        eng = Engine(snb, s, prec, host_build=host, eager=True, periodic=engine_periodic)
        fcheck("f eager", eng.step_forces(), expected(s))
        eng.close()
    eng = Engine(snb, s, prec, host_build=host, periodic=engine_periodic)
    plan = offset_plan(s)
    if not uncharged:
        eng.set_offsets(*plan)
    for k, p in enumerate(fr if steps == "all" else fr[:1]):
        eng.set_positions(p)
        fcheck("f captured" if k == 0 else "f replay %d" % k, eng.step_forces(), expected(s, p))
    if steps != "all":
        st = eng.stats()
        out = dict(checks=checks, flagged=flagged, finite=state["finite"], zero_ok=state["zero"], host_rebuilds=int(st.n_host_rebuilds), rebuilds=int(st.n_rebuilds), overruns=int(st.n_list_overruns))
        eng.close()
        return out
    # the parameter-offset pass, between two replayed steps
    if not uncharged:
        eng.set_global(0.5)
        q5, exc5 = at_global(s, plan, 0.5)
        fcheck("f offsets", eng.step_forces(), expected(s, fr[-1], q=q5, exc=exc5))
        eng.set_global(0.0)
        fcheck("f offsets back", eng.step_forces(), expected(s, fr[-1]))
    # atoms of the straddling chains cross a face on the unchanged list
    eng.set_positions(crossed)
    exc_ = expected(s, crossed)
    fcheck("f crossed", eng.step_forces(), exc_)
    # energies on the crossed frame
    f, se, e = eng.step_energy_forces()
    fcheck("ef forces", f, exc_)
    echeck("ef energies", se, exc_["energies"], "slice energies")
    echeck("ef total", [e], [float((s["lam"] * exc_["energies"]).sum())], "sum lambda E")
    echeck("e energies", eng.step_energy_only(), exc_["energies"], "slice energies")
    for name, mask in (("d", MASK_A), ("d after mask change", MASK_B)):
        m = np.zeros(len(s["lam"]), dtype=np.int32); m[list(mask)] = 1
        f, se = eng.step_derivative(m)
        fcheck("%s forces" % name, f, exc_)
        echeck("%s energies" % name, se[list(mask)], exc_["energies"][list(mask)], "slices %s" % (mask,))
    for name, mask in (("e masked", MASK_A), ("e masked after mask change", MASK_B)):      # energy only, some slices wanted: the !FORCES && !wantE skip
        m = np.zeros(len(s["lam"]), dtype=np.int32); m[list(mask)] = 1
        echeck("%s energies" % name, eng.step_energy_only_masked(m)[list(mask)], exc_["energies"][list(mask)], "slices %s" % (mask,))
    eng.all_slices()
    st = eng.stats()
    rebuilds, overruns, host_rebuilds = int(st.n_rebuilds), int(st.n_list_overruns), int(st.n_host_rebuilds)
    # the tables
    t = exc_["terms"]
    lab = group_labels(len(s["q"]))
    echeck("atomE", eng.atom_energies(), atom_energy_table(s, t), "every entry", entry=lambda k: " (%s)" % describe(s, t, int(k[0])))
    G = atom_force_table(s, t)
    tabF = eng.atom_forces()
    state["finite"] &= bool(np.isfinite(tabF).all())
    state["coulomb"] = max(state["coulomb"], float(np.abs(tabF[:, :, 0]).max()))
    worst = (0.0, 0, 0, 0)
    for J in range(NSUB):
        for term in range(2):
            rec = compare_forces(s, tabF[:, J, term], G[:, J, term], tol, floor=force_floor(s, exc_["forces"]))
            state["zero"] &= rec["zero_ok"]
            if rec["max_err"] >= worst[0]:
                worst = (rec["max_err"], J, term, rec["worst"])
    checks.append(("atomF", worst[0], "column %d term %d, %s" % (worst[1], worst[2], describe(s, t, worst[3]))))
    echeck("groupPairs", eng.group_pairs(lab), group_pair_matrix(s, t, lab), "%d labels" % GROUPS)
    if row in GROUP_TABLE_ROWS:
        groups = groups_of(lab)
        echeck("groupE", eng.group_energies(groups), np.stack([atom_energy_table(s, t)[g].sum(axis=0) for g in groups]), "%d groups" % GROUPS)
        gf = eng.group_forces(groups)
        want = np.stack([G[g].sum(axis=0) for g in groups])
        state["finite"] &= bool(np.isfinite(gf).all())
        state["coulomb"] = max(state["coulomb"], float(np.abs(gf[:, :, 0]).max()))
        checks.append(("groupF", float(np.max(np.linalg.norm(gf - want, axis=-1) / np.maximum(np.linalg.norm(want, axis=-1), force_floor(s, exc_["forces"])))), "%d groups" % GROUPS))
    eng.close()
    return dict(checks=checks, flagged=flagged, finite=state["finite"], zero_ok=state["zero"], host_rebuilds=host_rebuilds, rebuilds=rebuilds, overruns=overruns, coulomb=state["coulomb"])


# ---- the stand-alone list kernels: a child process under SNB_NO_FUSED_LISTS ---------------------------------------------------------------
# Every tile kernel carries the two lists as extra work-groups of its own launch, so no step of an ordinary process launches k_pairLists or
# k_pairListsEnergy.  With SNB_NO_FUSED_LISTS set (read once per process, csrc/switches.h) the engine hands the tile kernel no lists and
# launches them on their own (engine.hip, the `listsDone` branch of the step): k_pairLists<Real, false> on forces-only steps,
# k_pairLists<Real, true> on energy + forces and derivative steps, k_pairListsEnergy<Real> on energy-only steps, masked ones included.
STANDALONE_SWITCH = "SNB_NO_FUSED_LISTS"
STANDALONE_CASES = [CASES[4], CASES[11], CASES[16]]      # PME R0 triclinic p1 GPU builder, LJPME R4D cubic p0 GPU builder, uncharged LJPME R4D triclinic p1 host lists
STANDALONE_PRECISIONS = ("single", "double")


def main(argv):
    """`standalone OUT.json`: run_case on STANDALONE_CASES in this process's environment, which must have the switch set."""
    import importlib
    import json
    assert argv[1] == "standalone" and os.environ.get(STANDALONE_SWITCH) == "1"
    snb = importlib.import_module("openmm-nonbonded-slicing_amd")
    out = {}
    for case in STANDALONE_CASES:
        for prec in STANDALONE_PRECISIONS:
            rec = run_case(snb, case, prec)
            del rec["flagged"]
            out["%s %s" % (case_id(case), prec)] = rec
    with open(argv[2], "w") as f:
        json.dump(out, f)
    return 0


# ---- float32 emulation of the dispersion factors (csrc/pair_math.h dispersionExclusion) -----------------------------------------------
DISPERSION_SWITCH = 1.0


def dispersion_factors_float32(y, series=True):
    """(h3, h4) as the float kernels form them from y = (alpha_d r)^2 in float32: below DISPERSION_SWITCH the nested series
    h4 = exp(-y) y^4/24 (1 + y/5 (1 + y/6 (.. (1 + y/13)))), h3 = h4 + exp(-y) y^3/6; above it (and everywhere with series=False, the
    arithmetic before the series) 1 - exp(-y) (1 + y + y^2/2 (+ y^3/6))."""
    f = np.float32
    y = np.asarray(y, dtype=np.float32)
    e = np.exp(-y.astype(np.float64)).astype(np.float32)          # (__expf: a couple of ulp; taken as correctly rounded here)
    y2 = y * y; y3 = y2 * y
    h3f = f(1) - e * (f(1) + y + f(0.5) * y2)
    h4f = f(1) - e * (f(1) + y + f(0.5) * y2 + y3 * f(1.0 / 6.0))
    if not series:
        return h3f, h4f
    p = np.ones_like(y)
    for k in range(13, 4, -1):
        p = f(1) + y * f(1.0 / k) * p
    h4s = e * (y2 * y2 * f(1.0 / 24.0)) * p
    h3s = h4s + e * (y3 * f(1.0 / 6.0))
    small = y < f(DISPERSION_SWITCH)
    return np.where(small, h3s, h3f), np.where(small, h4s, h4f)


if __name__ == "__main__":
    sys.exit(main(sys.argv))
