"""The van der Waals census on the CPU: proves the instrument (tests/vdw_census.py) before the GPU is asked, with the oracle alone.  The
conditions on the inputs hold (float coordinates, the builder inequality, the cleared cutoff band, the chains' geometry, the cap on the
dimers near the cutoff); the closed form and the oracle agree on the dimers; the comparison flags every planted defect -- the switching
function off, the switching distance 1 % or 0.1 % off, alpha_d 1 % off, one atom's sigma 1 % larger -- and the oracle against itself flags
nothing.

Figures at the single-precision bar (docs/MEASUREMENT_LOG.md): switch off 94.7 .. 95.0 % of the atoms (worst atom 43 .. 121 bars, slice
energies up to 15 .. 69 bars); sd x 1.01 at sd = 0.6 20.6 .. 22.1 %, at sd = 0.9 94.4 .. 94.7 %; sd x 1.001 at sd = 0.9 23.0 .. 24.7 %, at
sd = 0.6 none (worst atom 0.5 bars: below what the bar can see); alpha_d x 1.01 90.8 .. 95.0 %.  The asserted lower bounds keep a margin."""
import numpy as np
import pytest

import ewald_census as EC
import shell_systems as S
import vdw_census as V

SINGLE = V.BARS["single"]
LATTICES = ("lj_big", "lj_small")


@pytest.mark.parametrize("name", LATTICES)
def test_lattice_inputs(name):
    s = V.build(name)
    n, L = len(s["q"]), s["L"]
    assert n == (8000 if name == "lj_big" else 729) and L == pytest.approx(8.0 if name == "lj_big" else 3.6)
    assert not s["q"].any(), "the systems are uncharged: LJ stands alone"
    # the builder inequality, at both paddings of the rows (engine.hip gpuRebuild): 7.28 and 7.68 < 8.0; 3.6 nm takes the host lists
    for pad in (0.1, 0.3):
        assert V.gpu_builder_applies(s, pad) == (name == "lj_big")
    assert 4.0 * np.cbrt(32.0 * L ** 3 / n) + 2.0 * (V.RC + 0.1) == pytest.approx(7.28, abs=0.01)
    # parameters
    eps, sig, sub = s["epsilon"], s["sigma"], s["subset"]
    dead = eps == 0
    assert dead.sum() == round(0.05 * n) and abs((sig[dead] == 1.0).sum() - 0.5 * dead.sum()) <= 1 and not (sig[~dead] == 1.0).any()
    assert ((sig[sig != 1.0] >= 0.28) & (sig[sig != 1.0] <= 0.36)).all() and ((eps[~dead] >= 0.3) & (eps[~dead] <= 1.2)).all()
    assert (sub == 3).any() and dead[sub == 3].all() and dead[sub != 3].any(), "subset 3 holds epsilon = 0 atoms only; others are spread over 0 .. 2"
    for k in range(3):
        assert 0.25 * n < (sub == k).sum() < 0.4 * n
    blocks = [len(set(sub[b:b + 32][sub[b:b + 32] < 3])) for b in range(0, n - 31, 32)]
    assert min(blocks) == 3, "subsets at random, not in slabs: every run of 32 atoms mixes all three"
    lam = s["lam"]
    off = [V.sl(i, j) for i in range(V.NSUB) for j in range(i)]
    assert (lam[off, 1] != 1).all() and (lam[off, 1] == 0).sum() == 1 and (lam[[V.sl(i, i) for i in range(V.NSUB)], 1] == 1).all()
    # topology: 1-2 at 0.4 and 1-3 at 0.8 excluded, 1-4 beyond the cutoff and a second family at 0.8 with epsilon != 0; hydrogens 0.1 nm from a heavy atom
    pairs = s["exc_pairs"]
    r = np.linalg.norm(s["pos"][pairs[:, 1]] - s["pos"][pairs[:, 0]], axis=1)      # (exceptions are not periodic: the plain difference)
    far, near = s["far14"], s["near14"]
    excl = np.setdiff1d(np.arange(len(pairs)), np.concatenate([far, near]))
    assert (s["exc_eps"][excl] == 0).all() and (s["exc_eps"][far] > 0).all() and (s["exc_eps"][near] > 0).all() and len(near) >= 30
    hyd = set(s["hydrogens"])
    plain = np.array([k for k in range(len(pairs)) if not (hyd & set(pairs[k].tolist()))])
    assert (r[np.intersect1d(far, plain)] > V.RC + 0.08).all() and (np.abs(r[np.intersect1d(far, plain)] - 1.2) < 0.11).all()
    assert (np.abs(r[np.intersect1d(near, plain)] - 0.8) < 0.11).all(), "the second family of 1-4 pairs lies inside the switch region of sd = 0.6"
    gap = pairs[excl, 1] - pairs[excl, 0]
    e12, e13 = np.intersect1d(excl[gap == 1], plain), np.intersect1d(excl[gap == 2], plain)
    assert (np.abs(r[e12] - 0.4) < 0.11).all() and (np.abs(r[e13] - 0.8) < 0.11).all() and ((r[e13] > 0.6) & (r[e13] < V.RC)).all()
    assert len(hyd) == 8
    for a in hyd:
        assert eps[a] == 0 and sig[a] == 1.0 and eps[a - 1] > 0 and np.linalg.norm(s["pos"][a] - s["pos"][a - 1]) == pytest.approx(0.1, abs=5e-4)
        assert any(set(p.tolist()) == {a - 1, a} for p in pairs[excl]), "the hydrogen and its heavy atom are an excluded pair"
    # frames: float coordinates, the cutoff band empty, the drift inside half the skin
    fr = V.frames(name)
    assert len(fr) == V.DRIFT_FRAMES
    for p in fr:
        assert np.array_equal(p, S.to_float(p)), "coordinates must be float32 values"
        assert len(V.band_pairs(s, p)[0]) == 0, "a pair within 1e-5 nm of the cutoff"
    if name == "lj_small":      # (all pairs in numpy: the same band by ewald_census's own search)
        assert np.array_equal(EC.clear_cutoff_band(fr[0], L, V.RC), fr[0]) and np.array_equal(EC.clear_cutoff_band(fr[-1], L, V.RC), fr[-1])
    drift = max(float(np.linalg.norm(p - fr[0], axis=1).max()) for p in fr)
    print("%s: largest displacement over the drift %.4f nm" % (name, drift))
    assert 0.01 < drift < 0.05, "the drifted positions must stay on the list built for the first (padding 0.1: half of it)"


def test_small_systems():
    s = V.build("nocutoff_cloud")
    assert len(s["q"]) == 97 and s["box"] is None and s["use_switch"] == 1 and not s["q"].any()
    t = V.case_system("nocutoff_cloud", "NoCutoff", 0.9)
    f1, e1 = V.oracle_eval(t)
    f0, e0 = V.oracle_eval(dict(t, use_switch=0))
    assert np.array_equal(f1, f0) and np.array_equal(e1, e0), "NoCutoff ignores the switching function"
    assert V.force_floor(t, f1) > 1.0
    t = V.case_system("nonperiodic", "NonPeriodic", 0.9)
    assert t["box"] is None and t["method"] == V.NONPERIODIC and np.array_equal(t["pos"], V.build("lj_big")["pos"])
    f1, e1 = V.oracle_eval(t)
    f0, _ = V.oracle_eval(dict(t, use_switch=0))
    assert V.force_floor(t, f1) > 1.0 and len(V.compare_forces(t, f0, f1, SINGLE)["flagged"]) > 0.85 * len(f1)


@pytest.mark.parametrize("sdf", V.SWITCH_FRACTIONS)
@pytest.mark.parametrize("row", V.PERIODIC_ROWS)
@pytest.mark.parametrize("name", LATTICES)
def test_planted_defects_are_flagged(name, row, sdf):
    """The comparison rule fed the oracle against a perturbed oracle at the single-precision bar."""
    t = V.case_system(name, row, sdf)
    n = len(t["q"])
    fo, so = V.oracle_eval(t)
    floor = V.force_floor(t, fo)
    fn = np.linalg.norm(fo, axis=1)
    print("%s: F_med %.3f, |F| max %.1f, the epsilon = 0 atoms up to %.3f" % (t["name"], floor, fn.max(), fn[t["epsilon"] == 0].max()))
    assert np.isfinite(fo).all() and np.isfinite(so).all() and not so[:, 0].any() and 1.0 < floor < 20.0
    rec = V.compare_forces(t, fo.copy(), fo, SINGLE)
    assert rec["ok"] and rec["max_err"] == 0.0 and V.energy_err(so, so) == 0.0, "the oracle against itself flags nothing"

    def flagged(defect):
        f, se = V.oracle_eval(defect)
        rec = V.compare_forces(t, f, fo, SINGLE)
        e = np.abs(se[:, 1] - so[:, 1]) / np.maximum(np.abs(so[:, 1]), 1.0) / SINGLE
        return len(rec["flagged"]) / float(n), rec, float(e.max())

    if V.ROWS[row][0] == V.LJPME:
        f0, s0 = V.oracle_eval(dict(t, use_switch=0))
        assert np.array_equal(f0, fo) and np.array_equal(s0, so), "LJPME with and without use_switch is bit-identical in the oracle (Q2)"
        share, rec, e = flagged(dict(t, alpha_d=t["alpha_d"] * 1.01))
        print("  alpha_d x 1.01: %.1f %% of the atoms flagged, worst %.1f bars, slice energies up to %.1f bars" % (100 * share, rec["max_err"] / SINGLE, e))
        assert share > 0.8
    else:
        share, rec, e = flagged(dict(t, use_switch=0))
        print("  switch off: %.1f %% of the atoms flagged, worst %.1f bars, slice energies up to %.1f bars" % (100 * share, rec["max_err"] / SINGLE, e))
        assert share > 0.85 and rec["max_err"] > 30 * SINGLE and e > 10
        share, rec, e = flagged(dict(t, sd=t["sd"] * 1.01))
        print("  sd x 1.01: %.1f %%, worst %.1f bars" % (100 * share, rec["max_err"] / SINGLE))
        assert share > (0.15 if sdf == 0.6 else 0.85)
        share, rec, e = flagged(dict(t, sd=t["sd"] * 1.001))
        print("  sd x 1.001: %.1f %%, worst %.1f bars" % (100 * share, rec["max_err"] / SINGLE))
        if sdf == 0.9:
            assert share > 0.15
    a = int(np.nonzero(t["epsilon"] > 0)[0][100])
    sg = t["sigma"].copy(); sg[a] *= 1.01
    share, rec, e = flagged(dict(t, sigma=sg))
    print("  sigma of atom %d x 1.01: %d atoms flagged, atom %d at %.1f bars" % (a, len(rec["flagged"]), a, rec["err"][a] / SINGLE))
    assert a in rec["flagged"] and 0 < len(rec["flagged"]) < 0.05 * n, "one atom's sigma must flag that atom and its neighbours only"


@pytest.mark.parametrize("sdf", V.SWITCH_FRACTIONS)
def test_dimer_gas(sdf):
    s = V.dimer_gas(sdf)
    nd, nd2, L = s["nd"], 2 * s["nd"], s["L"]
    assert L < 16.0 and np.spacing(np.float32(L)) < 1e-6, "one ulp of a coordinate below 1e-6 nm"
    assert np.array_equal(s["pos"], S.to_float(s["pos"]))
    assert V.gpu_builder_applies(s, 0.1) and V.gpu_builder_applies(s, 0.3), "the filler atoms take the gas over the GPU builder's threshold"
    # isolated: the only partner of a dimer atom within the cutoff is its own, and only when the dimer is inside; fillers keep their distance
    p = s["pos"][:nd2]
    d = p[:, None, :] - p[None, :, :]
    d -= L * np.rint(d / L)
    r = np.sqrt((d ** 2).sum(-1)); np.fill_diagonal(r, 99.0)
    assert np.array_equal((r < V.RC + 0.1).sum(1), (s["r"] < V.RC + 0.1).astype(int)) and np.array_equal(np.argmin(r, axis=1)[s["inside"]], s["partner"][s["inside"]])
    d = s["pos"][nd2:, None, :] - p[None, :, :]
    d -= L * np.rint(d / L)
    assert np.sqrt((d ** 2).sum(-1)).min() > 0.05 and (s["epsilon"][nd2:] == 0).all()
    # Lorentz-Berthelot is under test: unequal parameters inside every dimer, sigma_ij 0.45 .. 0.6, epsilon_ij up to 4
    sg, ep, pa = s["sigma"][:nd2], s["epsilon"][:nd2], s["partner"]
    assert (np.abs(sg - sg[pa]) > 0.08).all() and (np.abs(ep / ep[pa] - 1.0) > 1e-3).all()
    assert np.allclose(0.5 * (sg + sg[pa]), s["sij"]) and np.allclose(np.sqrt(ep * ep[pa]), s["eij"]) and s["sij"].min() >= 0.45 and s["sij"].max() <= 0.6 and 3.5 < s["eij"].max() <= 4.0
    # radii: from 0.9 sigma_ij, 200 and more over the switch region, the specials, both sides of the cutoff
    rr, tt = s["r"][:nd], s["tt"][:nd]
    sw = V.in_switch_region(s)[:nd]
    assert sw.sum() >= 200 and np.diff(np.sort(tt[sw])).max() < 0.01, "the switch region is covered without gaps"
    assert (rr >= 0.9 * s["sij"][:nd] - 1e-6).all() and (rr < 0.95 * s["sij"][:nd]).any() and ((rr < s["sd"]).sum() > 80)
    special = V.special_radii(sdf)
    assert np.array_equal(rr[s["special_sites"]], special), "the special radii are met exactly"
    lo, hi = special[:2]
    assert lo <= s["sd"] < hi and hi == float(np.nextafter(np.float32(lo), np.float32(2.0))) and special[2] == pytest.approx(s["sd"] + 0.5 * (V.RC - s["sd"]), abs=1e-7)
    assert special[3] < V.RC and float(np.nextafter(np.float32(special[3]), np.float32(2.0))) == V.RC and special[4] < V.RC < special[5]
    assert (~s["inside"][:nd]).sum() >= 10 and rr.max() < 1.06
    images = S.dimer_images(dict(s, pos=s["pos"][:nd2]))
    assert {(0, 0, 0), (1, 0, 0), (0, 1, 0), (0, 0, 1), (1, 1, 1)} <= {tuple(abs(k) for k in im) for im in images} and any(sum(1 for k in im if k) == 2 for im in images), "bonds cross faces, edges and the corner"
    # the closed form against the oracle
    fo, so = V.oracle_eval(s)
    err = np.linalg.norm(fo[:nd2] - s["expected"], axis=1) / np.maximum(s["scale"], 1.0)
    eerr = V.energy_err(so[:, 1], s["expected_slice_energies"][:, 1])
    print("dimers sd %.1f: closed form against the oracle: forces %.2e, slice energies %.2e" % (sdf, err.max(), eerr))
    assert err.max() < 1e-12 and eerr < 1e-12 and not fo[nd2:].any() and not so[:, 0].any()
    assert not fo[:nd2][~s["inside"]].any() and not s["expected"][~s["inside"]].any()
    # near the cutoff: the derived limit and the cap
    for prec in ("single", "mixed", "double"):
        lim = V.tt_limit(prec, sdf)
        share = V.near_cutoff(s, prec).sum() / float(V.in_switch_region(s).sum())
        print("  %s: tt_limit %.6f, %.1f %% of the switch-region dimers beyond it" % (prec, lim, 100 * share))
        assert 0.9 < lim < 1.0 and share <= 0.05, "at most 5 % of the switch-region dimers may fall under the absolute bar"
        bars = V.dimer_bars(s, prec)
        assert (bars[s["inside"]] > 0).all() and (bars >= V.BARS[prec] * s["scale"] * (1 - 1e-12)).all(), "the absolute bar is never below the relative one"
    assert V.tt_limit("double", sdf) > V.tt_limit("single", sdf)


@pytest.mark.parametrize("sdf", V.SWITCH_FRACTIONS)
def test_float32_pair_arithmetic_meets_the_dimer_bars(sdf):
    """The kernels' formula in float32 numpy on the dimers, from r rounded to float32, against the float64 closed form: inside the bars of
    the rule with room to spare, and over the relative bar tol * scale only beyond tt_limit -- so the limit narrows the inputs where
    rounding, not arithmetic, decides, and nowhere else."""
    s = V.dimer_gas(sdf)
    nd2 = 2 * s["nd"]
    k = V.kernel_form_float32(s)
    f = np.concatenate([k[:, None] * s["axis"], np.zeros((len(s["q"]) - nd2, 3))])
    err, zero, worst = V.compare_dimers(s, f, "single")
    ins = s["inside"]
    raw = np.abs(k - np.einsum("ij,ij->i", s["expected"], s["axis"]))[ins] / (SINGLE * s["scale"][ins])
    over = s["tt"][ins][raw > 1.0]
    print("float32 pair arithmetic, sd %.1f: worst %.3f bars (%s); over tol * scale alone: %d atoms, from tt = %.5f (tt_limit %.5f)" % (
        sdf, err, worst, len(over), over.min() if len(over) else 1.0, V.tt_limit("single", sdf)))
    assert err < 0.5 and zero
    assert len(over) == 0 or over.min() > V.tt_limit("single", sdf)
