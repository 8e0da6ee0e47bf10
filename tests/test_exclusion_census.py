"""The exclusion and exception census on the CPU: proves the instrument of tests/exclusion_census.py before tests/test_gpu_exclusion_census.py
relies on it.

 * the float64 series of g, h3, h4 against their closed forms where both are good, and the closed forms' own loss where they are not
 * the closed form against the oracle's direct-space-only evaluation (another implementation: a loop over pairs in C)
 * the two conditions: coordinate sensitivity and isolation, on every case, precision and frame
 * the tables' bookkeeping: every table reduces to the slice energies / contracts to the forces
 * the closed form through the instrument unchanged passes; five planted defects are flagged, on exactly the atoms they touch
 * the hardware control's prediction: expected values at exceptions_periodic = 1 against 0 differ on exactly the straddling molecules
 * the float32 emulation of the LJPME dispersion factors: the series of pair_math.h: dispersionExclusion a decade under the bar, and
   what the plain formula gave before it
"""
import math

import numpy as np
import pytest

import exclusion_census as X
import recip_systems as R

PRECISIONS = ("single", "double")          # (mixed precision is given the coordinates of single)
CONTROL_CASES = [X.CASES[3], X.CASES[14], X.CASES[6]]      # PME R0 cubic p0, LJPME R4D triclinic p0, PME R2 cubic p1


def _ids(cases):
    return [X.case_id(c) for c in cases]


def _system(case, prec):
    return X.build(case[0], case[1], prec, case[2], case[3], case[5])


def test_series_against_the_closed_forms():
    x = np.linspace(0.25, 0.5, 101)
    assert np.max(np.abs(X.g_series(x) / X.g_formula(x) - 1.0)) < 1e-12
    assert np.max(np.abs(X.g(np.array([0.4999999, 0.5, 0.5000001])) / X.g_formula(np.array([0.4999999, 0.5, 0.5000001])) - 1.0)) < 1e-12
    # the double formula loses what the cancellation of its two terms costs: 2e-11 at x = 0.0025, 1e-6 and more at x = 1e-5 (two terms of
    # 1e-5 that cancel to 7.5e-16) -- below the switch the series is the reference
    assert abs(float(X.g_formula(0.0025) / X.g_series(0.0025)) - 1.0) < 1e-9
    assert abs(float(X.g_formula(1e-5) / X.g_series(1e-5)) - 1.0) > 1e-9
    assert abs(float(X.g_series(1e-3)) / (4.0 / (3.0 * math.sqrt(math.pi)) * 1e-9) - 1.0) < 1e-6      # 0.752 x^3
    y = np.linspace(0.5, 2.0, 101)
    for first in (3, 4):
        assert np.max(np.abs(X.h_series(y, first) / X.h_formula(y, first) - 1.0)) < 1e-12
        assert abs(float(X.h_series(1e-3, first)) / (1e-3 ** first / math.factorial(first)) - 1.0) < 2e-3
    assert abs(float(X.h(np.array(2.0), 4) / X.h_formula(2.0, 4)) - 1.0) < 1e-13


@pytest.mark.parametrize("case", [X.CASES[0], X.CASES[4], X.CASES[11], X.CASES[13], X.CASES[16]], ids=_ids([X.CASES[0], X.CASES[4], X.CASES[11], X.CASES[13], X.CASES[16]]))
def test_closed_form_against_the_oracle(case, oracle):
    """Direct space only, the oracle's loop over all pairs: nothing but the two lists may contribute (the isolation condition, seen from the
    other side), and their sums are the closed form's.  Single-precision coordinates: separations from 0.002 nm, where the oracle's double
    formulas are still good to 1e-8 of the floor."""
    s = _system(case, "single")
    fo, so = R.oracle_eval(s, direct=True, recip=False)
    ex = X.expected(s)
    rec = X.compare_forces(s, fo, ex["forces"], 1e-5 if case[5] else 1e-7)
    assert len(rec["flagged"]) == 0 and rec["zero_ok"], (rec["max_err"], X.describe(s, ex["terms"], rec["worst"]))
    assert X.EC.rel(so, ex["energies"]) < 1e-9
    if case[5]:
        assert not so[:, 0].any() and not ex["energies"][:, 0].any()


@pytest.mark.parametrize("prec", PRECISIONS)
@pytest.mark.parametrize("case", X.CASES, ids=_ids(X.CASES))
def test_conditions(case, prec, oracle):
    s = _system(case, prec)
    n = len(s["q"])
    assert n % 32 != 0 and n < 6000
    assert R.gpu_builder_applies(s, s["padding"]), "the GPU builder must apply, or half of the builder coverage is lost"
    fr, crossed = X.frames(s)
    for k, p in enumerate(fr + [crossed]):
        ratio, a, ulp = X.coordinate_condition(s, X.BARS[prec], p)
        assert ratio < 1.0, "frame %d: one ulp (%.2e nm) moves %s by %.2f of a quarter bar" % (k, ulp, X.describe(s, X.expected(s, p)["terms"], a), ratio)
        ij, r = X.isolation_pairs(s, p)
        assert len(r) == 0, "frame %d: %d non-excluded pairs within %.2f nm, e.g. %s at %.3f" % (k, len(r), s["rc"] + s["padding"] + X.ISOLATION_EXTRA, ij[0], r[0])
        assert np.abs(p - fr[0]).max() <= 0.0201 and np.linalg.norm(p - fr[0], axis=1).max() < 0.4 * s["padding"]      # well inside padding / 2
    assert len(s["crossers"]) == (0 if case[5] else 10)
    inv = np.linalg.inv(s["box"]) * X.LENGTH
    for a, ax in s["crossers"]:
        assert 0 < (fr[0][a] @ inv)[ax] < 0.02 and (crossed[a] @ inv)[ax] < 0          # through the face at 0 of the cell's axis


@pytest.mark.parametrize("prec", PRECISIONS)
@pytest.mark.parametrize("case", [X.CASES[3], X.CASES[13], X.CASES[15]], ids=_ids([X.CASES[3], X.CASES[13], X.CASES[15]]))
def test_what_the_systems_contain(case, prec):
    s = _system(case, prec)
    t = X.pair_terms(s, periodic=1)          # (the molecules as they are built: minimum image)
    rw = X.EC.row_of(case[0])
    kind_of_pair = s["kind"][t["i"]]
    assert set(np.unique(t["slice"][kind_of_pair == 1])) == set(range(6)), "every slice occurs among the dimers"
    lam = s["lam"]
    assert len(np.unique(lam)) == lam.size and lam.min() > 0 and lam.max() < 1
    x = t["x"][kind_of_pair == 1]
    r = t["r"][kind_of_pair == 1]
    if not case[5]:
        assert ((x > 0.4949) & (x < 0.5)).sum() >= 3 and ((x >= 0.5) & (x < 0.5051)).sum() >= 3, "the switch of the series is bracketed"
        assert r.max() > 1.39 * rw["cutoff"] and ((r > rw["cutoff"]) & (r < 1.01 * rw["cutoff"])).any() and r.min() < 0.081
        close = t["r"][(kind_of_pair == 2)]
        assert close.min() < (1.01e-4 if prec == "double" else 2.01e-3) and close.max() > 0.19
        r14 = t["r"][(s["exc_qq"] != 0)]
        assert len(r14) == 30 and (r14 < rw["cutoff"]).sum() >= 8 and (r14 > rw["cutoff"]).sum() >= 8
        strad = X.straddling_atoms(s)
        chains = np.unique(s["mol"][s["kind"] == 3])
        assert len(np.unique(s["mol"][strad][s["kind"][strad] == 3])) * 3 == len(chains), "a third of the chains straddle"
        if prec == "double":
            thr = X.X_THRESHOLD / s["alpha"]
            assert (close < thr).sum() == 1 and ((close > thr) & (close < 2 * thr)).sum() == 1
            assert (close == 0).sum() == (1 if case[1] == X.PME else 0)
    else:
        assert not s["q"].any() and r.min() >= 0.05 - 1e-6 and r.max() <= 0.8 + 1e-6
        assert s["sigma"][s["epsilon"] > 0].min() >= 0.1 and s["sigma"][s["epsilon"] > 0].max() <= 0.35 and s["epsilon"].max() <= 0.6
    counts = np.bincount(np.concatenate([t["i"], t["j"]]), minlength=len(s["q"]))
    assert (counts == 47).sum() == 8 * 48 and (counts[s["mol"] < 0] == 0).all() and (counts == 0).sum() > 4000
    # lists of 47 and of 0 in one wave: the engine sorts by subset and space into blocks of 32 atoms of one subset (blockSubset), two blocks
    # to a wave.  No cluster has 32 atoms of one subset, so no block can be filled by one cluster alone, the next cluster is a site away, and
    # fillers of every subset lie inside each cluster's bounding sphere or right beside it.  (Necessary, not sufficient: the order itself is
    # the engine's and no ABI call returns it.)
    for m in np.unique(s["mol"][s["kind"] == 4]):
        atoms = np.nonzero(s["mol"] == m)[0]
        assert np.bincount(s["subset"][atoms], minlength=X.NSUB).max() < 32
        hub = s["pos"][atoms[0]]
        near = np.linalg.norm(X.S._min_image(s, s["pos"] - hub), axis=1) < 1.2
        assert set(s["subset"][near & (s["mol"] < 0)].tolist()) == set(range(X.NSUB)), "fillers of every subset within 1.2 nm of the hub"


@pytest.mark.parametrize("prec", PRECISIONS)
@pytest.mark.parametrize("case", CONTROL_CASES + [X.CASES[15]], ids=_ids(CONTROL_CASES + [X.CASES[15]]))
def test_tables_reduce_to_the_step(case, prec):
    """The closed form's tables against its own forces and slice energies, by the sum rules the engine's tables obey."""
    s = _system(case, prec)
    ex = X.expected(s)
    t = ex["terms"]
    A, G = X.atom_energy_table(s, t), X.atom_force_table(s, t)
    sub = s["subset"]
    for i in range(X.NSUB):
        for j in range(X.NSUB):
            want = ex["energies"][X.sl(i, j)] * (2.0 if i == j else 1.0)
            assert np.allclose(A[sub == i, j].sum(axis=0), want, rtol=1e-10, atol=1e-9)
    lam = s["lam"]
    f = np.zeros_like(ex["forces"])
    for j in range(X.NSUB):
        for term in range(2):
            f += np.array([lam[X.sl(a, j), term] for a in sub])[:, None] * G[:, j, term]
    assert np.allclose(f, ex["forces"], rtol=1e-10, atol=1e-9)
    lab = X.group_labels(len(sub))
    assert lab.min() == -1 and lab.max() == X.GROUPS - 1
    M = X.group_pair_matrix(s, t, lab)
    both = (lab[t["i"]] >= 0) & (lab[t["j"]] >= 0)
    assert np.allclose(M.sum(axis=0), [t["eC"][both].sum(), t["eL"][both].sum()], rtol=1e-10, atol=1e-9)
    split = sum(1 for m in np.unique(s["mol"][s["mol"] >= 0]) if len(np.unique(lab[s["mol"] == m])) > 1)
    assert split > 20, "the labels split molecules"


# ---- the controls ----------------------------------------------------------------------------------------------------------------------
def _touched(s, t, dcoef, tol, fexp):
    """The atoms a change of the pairs' force coefficients by `dcoef` (lambdas included) moves over the bar, from the pairs alone."""
    df = np.zeros_like(fexp)
    np.add.at(df, t["i"], dcoef[:, None] * t["d"]); np.add.at(df, t["j"], -dcoef[:, None] * t["d"])
    return set(np.nonzero(np.linalg.norm(df, axis=1) > tol * np.maximum(np.linalg.norm(fexp, axis=1), X.force_floor(s, fexp)))[0].tolist())


@pytest.mark.parametrize("prec", PRECISIONS)
@pytest.mark.parametrize("case", CONTROL_CASES, ids=_ids(CONTROL_CASES))
def test_unchanged_passes_and_planted_defects_are_flagged(case, prec):
    s = _system(case, prec)
    tol = X.BARS[prec]
    ex = X.expected(s)
    t = ex["terms"]
    rec = X.compare_forces(s, ex["forces"], ex["forces"], tol)
    assert len(rec["flagged"]) == 0 and rec["zero_ok"] and rec["max_err"] == 0.0
    lamC, lamL = s["lam"][t["slice"], 0], s["lam"][t["slice"], 1]
    q = s["q"]
    qq = X.K * q[t["i"]] * q[t["j"]]
    kind = s["kind"]

    def flagged(defect):
        return set(X.compare_forces(s, X.expected(s, defect=defect)["forces"], ex["forces"], tol)["flagged"].tolist())

    # (1) the minimum image where the plain difference belongs
    got = flagged("image")
    if case[3] == 0 and case[1] != X.LJPME:
        assert got == set(X.control_atoms(s).tolist()) and len(got) > 100
        assert {3} <= set(kind[sorted(got)].tolist())
    elif case[3] == 0:      # (LJPME: a straddling pair with its dispersion term alone moves by less than a bar)
        coul = (t["cC"] != 0) | (t["c14C"] != 0) | (t["c14L"] != 0)
        strad = set(X.straddling_atoms(s).tolist())
        assert got <= strad and got >= (strad & (set(t["i"][coul].tolist()) | set(t["j"][coul].tolist()))) and len(got) > 100
    else:
        assert got == set()          # (the record already uses the minimum image)
    # (2) the series below x = 0.5 cut to three terms
    small = t["x"] < X.SERIES_SWITCH
    with np.errstate(divide="ignore", invalid="ignore"):
        d2 = np.where(small & (qq != 0) & (t["x"] > 1e-6), -lamC * qq * (X.g_series(t["x"], 3) - X.g_series(t["x"])) / t["r"] ** 3, 0.0)
    want = _touched(s, t, d2, tol, ex["forces"])
    assert flagged("series3") == want
    if prec == "double":
        assert len(want) > 20 and all(((t["x"] > 0.15) & small)[(t["i"] == a) | (t["j"] == a)].any() for a in want)
    # (3) the 1-4 LJ term with 6 in place of 12
    is14 = s["exc_eps"] != 0
    s6 = np.where(is14, (s["exc_sigma"] / np.where(t["r"] > 0, t["r"], 1.0)) ** 6, 0.0)
    d3 = np.where(is14, lamL * 4.0 * s["exc_eps"] * (-6.0 * s6) * s6 / np.where(t["r"] > 0, t["r"], 1.0) ** 2, 0.0)
    want = _touched(s, t, d3, tol, ex["forces"])
    assert flagged("lj6") == want and len(want) >= 4
    assert all(kind[a] == 3 for a in want)
    # (4) one satellite dropped from a hub's list
    k = X.dropped_pair(s)
    assert flagged("dropped") == {int(t["i"][k]), int(t["j"][k])}
    assert kind[t["i"][k]] == 4 and (t["i"] == t["i"][k]).sum() == 47
    # (5) lambda_vdW in place of lambda_C on the correction
    d5 = (lamL - lamC) * t["cC"]
    want = _touched(s, t, d5, tol, ex["forces"])
    assert flagged("lambda") == want and len(want) > 200
    # the energies see (2) .. (4) too (the lambdas do not enter raw slice energies)
    assert X.EC.rel(X.expected(s, defect="dropped")["energies"], ex["energies"]) > tol


@pytest.mark.parametrize("prec", PRECISIONS)
@pytest.mark.parametrize("case", X.CONTROL_CASES, ids=_ids(X.CONTROL_CASES))
def test_prediction_of_the_hardware_control(case, prec):
    """An engine with exceptions_periodic = 1 judged against expected values at 0: the answer differs on the atoms of the straddling
    molecules by at least two bars (an engine may itself be one bar off) and on no other atom at all."""
    s = _system(case, prec)
    tol = X.BARS[prec]
    f0, f1 = X.expected(s, periodic=0)["forces"], X.expected(s, periodic=1)["forces"]
    want = X.control_atoms(s)
    err = X.compare_forces(s, f1, f0, tol)["err"]
    assert len(want) > 100 and (err[want] > 2.0 * tol).all(), err[want].min() / tol
    rest = np.setdiff1d(np.arange(len(s["q"])), want)
    assert (f1[rest] == f0[rest]).all()


# ---- the float32 emulation of the LJPME dispersion factors ------------------------------------------------------------------------------
def test_dispersion_factors_in_float32():
    """y = (alpha_d r)^2 from the smallest separation of the uncharged copy (0.05 nm at alpha_d = 2.0: alpha_d r = 0.1) through the switch of
    pair_math.h: dispersionExclusion (y = 1) and on to alpha_d r = 3.  The series stays a decade under the bar of 1e-3; above the switch
    the plain formula does too.  Before the series the plain formula ran everywhere: its loss is asserted, so that this test says what was
    wrong (this emulation's figures for the force factor at alpha_d r = 0.25 and 0.375: 1.1e-1 and 3.2e-3; the series: 3.2e-7 at worst)."""
    ar = np.concatenate([np.geomspace(0.1, 1.0, 2000, endpoint=False), np.linspace(1.0, 3.0, 2001)])
    y = (ar.astype(np.float32) ** 2).astype(np.float32)
    y64 = y.astype(np.float64)
    want3, want4 = X.h(y64, 3), X.h(y64, 4)
    new3, new4 = X.dispersion_factors_float32(y)
    e3, e4 = np.abs(new3 / want3 - 1.0), np.abs(new4 / want4 - 1.0)
    print("XCL dispersion factors, float32 series: worst relative error energy %.2e force %.2e (below the switch %.2e %.2e)" % (e3.max(), e4.max(), e3[y < 1].max(), e4[y < 1].max()))
    assert e3.max() < 1e-4 and e4.max() < 1e-4
    old3, old4 = X.dispersion_factors_float32(y, series=False)
    o3, o4 = np.abs(old3 / want3 - 1.0), np.abs(old4 / want4 - 1.0)
    at = lambda v: int(np.argmin(np.abs(ar - v)))
    print("XCL dispersion factors, float32 formula: force %.1e at 0.25, %.1e at 0.375, worst %.1e; energy %.1e at 0.25, worst %.1e" % (o4[at(0.25)], o4[at(0.375)], o4.max(), o3[at(0.25)], o3.max()))
    assert o4[ar < 0.3].max() > 1e-2 and o3[ar < 0.3].max() > 1e-4
