"""Ewald-parameter census: the rows, the guard's expected decisions and the helpers shared by tests/test_ewald_fit_cpu.py (CPU) and
tests/test_gpu_ewald_census.py (GPU).

The pair kernels evaluate the direct-space Ewald terms with polynomials of fixed degree whose error grows fast with
z = alpha (cutoff + padding + 0.02); csrc/ewald_fit.h measures the residuals and keeps a polynomial only where they pass its guard.
The rows walk z from 1.1 to 4.8: alpha = sqrt(-ln(2 tol)) / cutoff for the Ewald error tolerances 5e-4 (the benchmark's), 1e-5 and 1e-6.

`use`: the guard's decisions (bit 0 force factor Bt, bit 1 energy Et, bit 2 dispersion Gd with alpha_d = alpha; the float column without
bit 2, which no float kernel has) per kernel arithmetic,
as tests/test_ewald_fit_cpu.py derives them from the fit itself; the GPU census asserts that the engine reports them
(snb_stats.ewald_poly_mask), so that a fallback that silently stayed away cannot pass by luck.  `parent_fails`: the precisions whose
Coulomb forces miss the parity bar where the polynomials are used regardless (SNB_EWALD_POLY_ALWAYS), by the CPU emulation.
"""
import math

FORCE, ENERGY, DISPERSION = 1, 2, 4
K_COULOMB = 138.935456
BARS = {"single": 1e-3, "mixed": 1e-3, "double": 1e-5}

ROWS = {
    #        cutoff  alpha   padding  use: float, double            where the unguarded polynomials fail
    "R0": dict(cutoff=1.0, alpha=2.6283, padding=0.1, use=(3, 7), parent_fails=()),      # the benchmark point: every polynomial stays
    "R1": dict(cutoff=1.0, alpha=2.6283, padding=0.3, use=(2, 7), parent_fails=()),
    "R2": dict(cutoff=1.0, alpha=3.2900, padding=0.1, use=(0, 5), parent_fails=()),
    "R3": dict(cutoff=1.0, alpha=3.2900, padding=0.3, use=(0, 4), parent_fails=("single",)),
    "R4": dict(cutoff=1.0, alpha=3.6221, padding=0.3, use=(0, 0), parent_fails=("single", "double")),
    "R5": dict(cutoff=0.8, alpha=3.2854, padding=0.3, use=(0, 5), parent_fails=()),
    "R6": dict(cutoff=1.2, alpha=2.1903, padding=0.0, use=(3, 7), parent_fails=()),
    "R7": dict(cutoff=1.0, alpha=1.0, padding=0.1, use=(3, 7), parent_fails=()),
}
# LJPME with unequal parameters: R4 with alpha_d = 2.0, whose dispersion polynomial passes (z_d = 2.64) while the Coulomb ones do not.
# A fit that swapped the two would keep Bt and drop Gd.
R4D = dict(cutoff=1.0, alpha=3.6221, alpha_d=2.0, padding=0.3, use=(0, 4), parent_fails=("single", "double"))

PME, LJPME, EWALD = 4, 5, 3


def is_float(precision):
    return precision in ("single", "mixed", 0, 2)


def engine_mask(row, precision, method, control=False):
    """snb_stats.ewald_poly_mask of an engine on this row: the guard's decisions (all of them under SNB_EWALD_POLY_ALWAYS) for the
    polynomials the kernels of that precision have -- Bt and Et in single and mixed precision, Bt and (LJPME) Gd in double."""
    have = (FORCE | ENERGY) if is_float(precision) else (FORCE | (DISPERSION if method == LJPME else 0))
    return have if control else row["use"][0 if is_float(precision) else 1] & have


def alpha_of_tolerance(tol, cutoff):
    return math.sqrt(-math.log(2.0 * tol)) / cutoff


# ====================================================================================================================================
# GPU side (tests/test_gpu_ewald_census.py; `python tests/ewald_census.py control bulk|dimers OUT.json` is the control's child process)
# ====================================================================================================================================
def _np():
    import numpy as np
    return np


TOLS = BARS
BULK_SMALL, BULK_BIG = (3000, 3.2, 28, 20), (13824, 6.0, 48, 24)      # atoms, cell, Coulomb mesh, dispersion mesh (the meshes stay idle: direct space only)
TABLE_ROWS = ("R0", "R3", "R4")
EWALD_KMAX = (5, 5, 5)


def row_of(name):
    return R4D if name == "R4D" else ROWS[name]


def rel(got, want):
    np = _np()
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    return float(np.max(np.abs(got - want) / np.maximum(np.abs(want), 1.0))) if got.size else 0.0


def force_rel(got, want):
    np = _np()
    return float(np.max(np.linalg.norm(np.asarray(got) - want, axis=-1) / np.maximum(np.linalg.norm(want, axis=-1), 1.0)))


# ---- (a) bulk, against the oracle ----------------------------------------------------------------------------------------------------
def bulk_force(snb, name, method, size, derivatives):
    import systems
    np = _np()
    row = row_of(name)
    n, L, mesh, dmesh = size
    F = snb.SlicedNonbondedForce
    force, pos, box = systems.random_box(F, n, 3, method, L, row["cutoff"], pme=(row["alpha"], mesh, mesh, mesh) if method != EWALD else (row["alpha"], 0, 0, 0),
                                         ljpme=(row.get("alpha_d", row["alpha"]), dmesh, dmesh, dmesh) if method == LJPME else None, derivatives=derivatives)
    if method == EWALD:
        force.ewaldKmax = EWALD_KMAX
    pos = np.asarray(pos, dtype=np.float64).astype(np.float32).astype(np.float64)      # what a single-precision engine is given
    return force, pos, box


CUTOFF_BAND = 1e-5


def clear_cutoff_band(pos, L, rc):
    """Float coordinates with no pair within CUTOFF_BAND of the cutoff.  The oracle decides r < rc in double and a single-precision engine in
    float from coordinates it has wrapped and shifted, so a pair within a few 1e-7 nm of rc can fall on either side; at alpha rc = 1 the
    Ewald force still jumps by K q q 0.57 / rc^2 (up to 50 kJ/mol/nm) there, far over the bar, with nothing wrong in either.  As
    shell_systems.clear_band does for the shell census, one atom of every such pair is moved 1e-4 nm outward along the pair's axis."""
    np = _np()
    pos = np.array(pos, dtype=np.float64)
    iu, ju = np.triu_indices(len(pos), 1)
    for _ in range(20):
        d = pos[ju] - pos[iu]
        d -= L * np.rint(d / L)
        r = np.sqrt(np.einsum("ij,ij->i", d, d))
        k = np.nonzero(np.abs(r - rc) < CUTOFF_BAND)[0]
        if len(k) == 0:
            return pos
        pos[ju[k]] += 1e-4 * d[k] / r[k][:, None]
        pos = pos.astype(np.float32).astype(np.float64)
    raise AssertionError("the cutoff band does not clear")


def _context(snb, force, box, prec, row):
    system = snb.System()
    for _ in range(force.getNumParticles()):
        system.addParticle(1.0)
    system.setDefaultPeriodicBoxVectors(*box)
    system.addForce(force)
    force.setForceGroup(0); force.setReciprocalSpaceForceGroup(1)
    return snb.Context(system, precision=prec, neighbor_padding=row["padding"], rebuild_interval=10 if row["padding"] > 0 else 1)


DIRECT = 1      # the force group of the direct-space part


def bulk_case(snb, oracle, name, prec, method, size, tables=False, forces_only=False):
    """One engine pair (with and without derivative bindings) on a row: {'errors': {step: worst error in units of max(|x|, 1)}, 'finite',
    'mask', 'host_rebuilds'}.  Steps: 'efd' energy + forces + derivatives, 'f1' / 'f2' forces only at nudged positions (the second a
    replayed graph), 'e' energy only, and with `tables` 'atomE' (probe rows) / 'atomF' (every entry), direct space alone throughout.
    forces_only: the 'f1' / 'f2' steps alone (the control, which is about them)."""
    import atom_energy_truth as aet
    import atom_force_truth as aft
    np = _np()
    row = row_of(name)
    okw = dict(kmax=EWALD_KMAX) if method == EWALD else {}
    errors, finite = {}, True

    def ora(force, pos, box):
        return oracle.evaluate(force, pos, box, None, True, False, **okw)

    # energy + forces + derivatives
    mask = host = None
    if not forces_only:
        force, pos, box = bulk_force(snb, name, method, size, True)
        if size[0] <= 4000:
            pos = clear_cutoff_band(pos, size[1], row["cutoff"])
        ctx = _context(snb, force, box, prec, row)
        ctx.setPositions(pos)
        st = ctx.getState(getEnergy=True, getForces=True, getParameterDerivatives=True, groups=DIRECT)
        kern = ctx._kernelFor(force)
        o = ora(force, pos, box)
        d = st.getEnergyParameterDerivatives()
        got = [st.getPotentialEnergy(), *kern.lastSliceEnergies.ravel(), *[d[k] for k in sorted(o["derivatives"])]]
        want = [o["energy"], *o["slice_energies"].ravel(), *[o["derivatives"][k] for k in sorted(o["derivatives"])]]
        finite &= bool(np.isfinite(got).all() and np.isfinite(st.getForces()).all())
        errors["efd"] = max(rel(got, want), force_rel(st.getForces(), o["forces"]))
        stats = kern.getStats()
        mask, host = int(stats.ewald_poly_mask), int(stats.n_host_rebuilds)
        del ctx, kern

    # forces only (no derivative bindings: the plain forces-only step), then energy only, then the tables, on one engine
    force, pos, box = bulk_force(snb, name, method, size, False)
    ctx = _context(snb, force, box, prec, row)
    rng = np.random.default_rng(7)
    clear = size[0] <= 4000      # (all pairs in numpy: the small systems; the large ones run at alpha rc >= 2.6, where the jump is 200 times smaller)
    for k in (0, 1, 2):
        if clear:
            pos = clear_cutoff_band(pos, size[1], row["cutoff"])
        ctx.setPositions(pos)
        f = ctx.getState(getForces=True, groups=DIRECT).getForces()
        finite &= bool(np.isfinite(f).all())
        if k:      # (step 0 is the eager first step)
            errors["f%d" % k] = force_rel(f, ora(force, pos, box)["forces"])
        pos = (pos + rng.normal(0.0, 0.004, pos.shape)).astype(np.float32).astype(np.float64)
    if forces_only:
        st = ctx._kernelFor(force).getStats()
        return dict(errors=errors, finite=finite, mask=int(st.ewald_poly_mask), host_rebuilds=int(st.n_host_rebuilds))
    if clear:
        pos = clear_cutoff_band(pos, size[1], row["cutoff"])
    ctx.setPositions(pos)
    o = ora(force, pos, box)
    e = ctx.getState(getEnergy=True, groups=DIRECT).getPotentialEnergy()
    se = ctx._kernelFor(force).lastSliceEnergies
    finite &= bool(np.isfinite(e) and np.isfinite(se).all())
    errors["e"] = max(rel(e, o["energy"]), rel(se, o["slice_energies"]))
    assert int(ctx._kernelFor(force).getStats().ewald_poly_mask) == mask
    if tables:
        sub = aft.force_subsets(force)
        tabF = ctx.getAtomForces(force, includeReciprocal=False)
        tabE = ctx.getAtomEnergies(force, includeReciprocal=False)
        finite &= bool(np.isfinite(tabF).all() and np.isfinite(tabE).all())
        errors["atomF"] = aft.rel(tabF, aft.truth_table(aft.force_evaluator(oracle, force, pos, box, None, True, False, **okw), sub, 3))
        probes = (0, 1, 1499, 2999)      # chain ends and middles, all three subsets
        rows = aet.truth_table(aet.force_evaluator(oracle, force, pos, box, None, True, False, **okw), sub, 3, probes)
        errors["atomE"] = max(aet.rel(tabE[a], r) for a, r in rows.items())
    return dict(errors=errors, finite=finite, mask=mask, host_rebuilds=host)


# ---- (b) radial dimers, against the closed form --------------------------------------------------------------------------------------
def dimer_radii(rc, rmin=0.08):
    """312 separations: 150 from rmin to 0.8 rc, 150 over the last fifth up to rc (1 - 1e-4), 12 beyond the cutoff."""
    np = _np()
    return np.concatenate([np.linspace(rmin, 0.8 * rc, 150, endpoint=False), np.linspace(0.8 * rc, rc * (1.0 - 1e-4), 150),
                           rc * (1.0 + np.array([1e-4, 3e-4, 1e-3, 3e-3, 1e-2, 2e-2, 4e-2, 6e-2, 8e-2, 0.1, 0.2, 0.28]))])


def ewald_dimers(name, method, precision, seed=78, sites=16, spacing=2.5):
    """shell_systems.dimer_gas under Ewald: 4096 isolated dimers in a 40 nm cell, random orientations, bonds across faces, edges and (the
    dimer at the origin) the corner; no exclusions, which under Ewald would bring their erf corrections into the direct part; separations cycle through dimer_radii, charges (1 | 0.5) x (+-1 | +-0.5); with LJPME sigma in
    0.25 .. 0.4, epsilon in 0.01 .. 0.03, like charges only and separations from 0.2 nm (at 0.08 nm the r^-12 wall is a force of 3e10 kJ/mol/nm, past the 2^31
    of the fixed-point sums of mixed precision, and the slice energies would be those few pairs alone).  The LJPME parameters keep the
    bar tol max(|F|, 1) answerable in float: a coordinate near 40 nm is a multiple of 3.8e-6 nm, the engine re-images atoms by whole cells,
    so its r differs from the r of the given coordinates by up to ~4e-6 nm, (2 + 13) 1e-5 of a Coulomb + r^-12 force at 0.3 nm.  Where an
    attractive Coulomb force of hundreds of kJ/mol/nm cancels against the wall (or a deep LJ well against a repulsion) to |F| < 1, that is
    tens of bars with nothing wrong; with like charges and a shallow well no two large terms of opposite sign meet.  The dispersion term
    under test stays 15 bars (single) to 1500 bars (double) tall at 0.6 nm.  Both signs of q q are on the PME rows.  Direct space only: `expected` forces and `expected_slice_energies` in float64 from erfc / exp
    (ReferenceSlicedLJCoulombIxn.cpp:367-445 as oracle/snb_oracle.c ewald_pair restates it), zero beyond the cutoff."""
    import shell_systems as S
    np = _np()
    row = row_of(name)
    rc, alpha, alpha_d = row["cutoff"], row["alpha"], row.get("alpha_d", row["alpha"])
    rng = np.random.default_rng(seed)
    L = sites * spacing
    cell = np.diag([L, L, L])
    g = np.stack(np.meshgrid(np.arange(sites), np.arange(sites), np.arange(sites), indexing="ij"), -1).reshape(-1, 3).astype(float)
    centres = g * spacing
    nd = len(centres)
    u = rng.normal(size=(nd, 3)); u /= np.linalg.norm(u, axis=1)[:, None]
    u[0] = np.ones(3) / np.sqrt(3.0)      # the dimer at the origin lies along the body diagonal: its bond crosses the corner
    radii = dimer_radii(rc, 0.2 if method == LJPME else 0.08)
    target = radii[rng.permutation(nd) % len(radii)]
    pos = np.concatenate([centres - 0.5 * target[:, None] * u, centres + 0.5 * target[:, None] * u])
    pos = pos - np.floor(pos / L) * L
    if precision != "double":
        pos = S.to_float(pos)
    qa = rng.choice([1.0, 0.5], nd); qb = rng.choice([1.0, -1.0, 0.5, -0.5], nd)
    if method == LJPME:
        qb = np.abs(qb)      # like charges only, see below
    q = np.concatenate([qa, qb])
    sub = (np.arange(2 * nd) % 2).astype(np.int32)
    s = S.make_system("ewald_dimers_%s_%d_%s" % (name, method, precision), pos, cell, q, sub, 2, rc=rc)
    s["pos"] = np.ascontiguousarray(pos)
    s.update(method=method, alpha=alpha, alpha_d=alpha_d, grid=(32, 32, 32), dgrid=(32, 32, 32) if method == LJPME else (0, 0, 0), kmax=EWALD_KMAX if method == EWALD else (0, 0, 0))
    if method == LJPME:
        s["sigma"] = rng.uniform(0.25, 0.4, 2 * nd); s["epsilon"] = rng.uniform(0.01, 0.03, 2 * nd)
    partner = np.concatenate([np.arange(nd) + nd, np.arange(nd)])
    d = -S._min_image(s, s["pos"][partner] - s["pos"])      # r_i - r_partner
    r = np.linalg.norm(d, axis=1)
    ins = r < rc
    erfc = np.vectorize(math.erfc, otypes=[np.float64])
    qq = K_COULOMB * q * q[partner]
    fac = qq * (erfc(alpha * r) + 2.0 * alpha * r / math.sqrt(math.pi) * np.exp(-(alpha * r) ** 2)) / r ** 3
    ecoul = qq * erfc(alpha * r) / r
    evdw = np.zeros_like(r)
    if method == LJPME:
        sg, ep = s["sigma"], s["epsilon"]
        sij, e4 = 0.5 * (sg + sg[partner]), 4.0 * np.sqrt(ep * ep[partner])
        c6c6 = (2.0 * sg ** 3 * np.sqrt(ep)) * (2.0 * sg[partner] ** 3 * np.sqrt(ep[partner]))
        s6 = (sij / r) ** 6
        x = (alpha_d * r) ** 2; xc = (alpha_d * rc) ** 2
        fac = fac + e4 * (12.0 * s6 - 6.0) * s6 / r ** 2 + 6.0 * c6c6 / r ** 8 * (1.0 - np.exp(-x) * (1.0 + x + x * x / 2.0 + x ** 3 / 6.0))
        sc6 = (sij / rc) ** 6
        evdw = (e4 * (s6 - 1.0) * s6 + c6c6 / r ** 6 * (1.0 - np.exp(-x) * (1.0 + x + x * x / 2.0)) + e4 * (1.0 - sc6) * sc6
                - c6c6 / rc ** 6 * (1.0 - math.exp(-xc) * (1.0 + xc + xc * xc / 2.0)))
    expected = np.where(ins[:, None], fac[:, None] * d, 0.0)
    es = np.zeros((3, 2))
    for k, e in enumerate((ecoul, evdw)):
        pair = np.where(ins[:nd], e[:nd], 0.0)
        es[0, k] = pair[0::2].sum(); es[2, k] = pair[1::2].sum()
    s.update(partner=partner, r=r, inside=ins, expected=expected, expected_slice_energies=es)
    return s


def dimer_case(snb, name, prec, method, host):
    """Forces-only, energy + forces and energy-only steps of the dimer gas on one engine: {'errors': {'f', 'ef', 'e', 'eo'}, 'finite', 'outside_zero',
    'worst': the separation and charges of the worst atom, 'mask', 'host_rebuilds'}."""
    import recip_systems as RS
    np = _np()
    row = row_of(name)
    s = ewald_dimers(name, method, prec)
    eng = RS.Engine(snb, s, prec, direct=1, padding=row["padding"], interval=10 if row["padding"] > 0 else 1, host_build=host)
    eng.recip = 0
    f1 = eng.step_forces()
    f2, se, _ = eng.step_energy_forces()
    se_only = eng.step_energy_only()
    st = eng.stats()
    mask, hostn, rebuilds = int(st.ewald_poly_mask), int(st.n_host_rebuilds), int(st.n_rebuilds)
    eng.close()
    ex = s["expected"]
    finite = bool(np.isfinite(f1).all() and np.isfinite(f2).all() and np.isfinite(se).all() and np.isfinite(se_only).all())
    errs = [np.linalg.norm(f - ex, axis=1) / np.maximum(np.linalg.norm(ex, axis=1), 1.0) for f in (f1, f2)]
    w = int(np.nanargmax(np.maximum(errs[0], errs[1])))
    outside_zero = bool((f1[~s["inside"]] == 0).all() and (f2[~s["inside"]] == 0).all())
    return dict(errors=dict(f=float(errs[0].max()), ef=float(errs[1].max()), e=rel(se, s["expected_slice_energies"]), eo=rel(se_only, s["expected_slice_energies"])), finite=finite, outside_zero=outside_zero,
                worst="atom %d: r = %.5f nm, q q = %+.2f" % (w, s["r"][w], s["q"][w] * s["q"][s["partner"][w]]), mask=mask, host_rebuilds=hostn, rebuilds=rebuilds)


# ---- (c) the control's child process ---------------------------------------------------------------------------------------------------
CONTROL = [("R0", "single"), ("R0", "double"), ("R3", "single"), ("R4", "single"), ("R4", "double")]      # (R3 in double stays inside its bar unguarded too)


def main(argv):
    """`control bulk|dimers OUT.json`: the forces-only steps of the bulk cases (PME, 13 824 atoms: in 3.2 nm the lists wrap per pair, and
    that kernel has polynomials in double precision only) or the dimer cases (PME, GPU builder) of CONTROL in this process's environment."""
    import importlib
    import json
    import os
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    for p in (root, os.path.join(root, "oracle"), os.path.join(root, "tests")):
        if p not in sys.path:
            sys.path.insert(0, p)
    import oracle
    snb = importlib.import_module("openmm-nonbonded-slicing_amd")
    assert argv[1] == "control" and argv[2] in ("bulk", "dimers")
    out = {}
    for name, prec in CONTROL:
        out["%s %s %s" % (argv[2], name, prec)] = bulk_case(snb, oracle, name, prec, PME, BULK_BIG, forces_only=True) if argv[2] == "bulk" else dimer_case(snb, name, prec, PME, 0)
    with open(argv[3], "w") as f:
        json.dump(out, f)
    return 0


if __name__ == "__main__":
    import sys
    sys.exit(main(sys.argv))
