"""The Ewald polynomial fit and its guard (csrc/ewald_fit.h) on the CPU.

tests/ewald_fit_check.cpp is compiled once per session with g++ under ASan + UBSan and run as a child process per (row, precision); no
GPU, nothing loaded into python.  For every row of ewald_census.ROWS (and the unequal-alpha LJPME row) and both kernel arithmetics:

 1  the residuals the header reports are not optimistic: each >= 0.9 x the checker's own evaluation (exact functions in long double at
    4001 radii in [0.05, cutoff], its own Horner loops)
 2  every polynomial the guard keeps meets the guard's conditions on that independent evaluation: K r |dBt| and 6 c6 r |dGd| of the
    reference pair (|qq| = 1, sigma = 0.4, eps = 1) at most half the precision's bar, |dEt| <= 1.5e-7 / cutoff
 3  the decisions are the ones ewald_census.ROWS lists (the GPU census asserts the engine reports those); the benchmark row keeps all
    three polynomials in both arithmetics, so bench.py's kernels are the ones they were
 4  an emulation of the Coulomb forces of systems.random_box (3000 atoms, L = 3.2): the polynomial's pair errors, in the kernel's
    arithmetic, summed per atom and taken relative to max(|F|, 1).  With the guard's decisions at most 1/20 of the bar on every row;
    with the guard ignored above the bar on the rows marked in `parent_fails`, i.e. the rows can see the defect.
"""
import math
import os
import subprocess

import numpy as np
import pytest

import ewald_census as EC
import systems

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ALL_ROWS = dict(EC.ROWS, R4D=EC.R4D)
PRECISIONS = ("single", "double")


@pytest.fixture(scope="session")
def checker(tmp_path_factory):
    exe = tmp_path_factory.mktemp("ewald_fit") / "ewald_fit_check"
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I", os.path.join(ROOT, "openmm-nonbonded-slicing_amd", "csrc"), os.path.join(ROOT, "tests", "ewald_fit_check.cpp"), "-o", str(exe)])
    return exe


@pytest.fixture(scope="session")
def fits(checker):
    """(row, precision) -> the checker's output, with LJPME so that all three polynomials are fitted."""
    out = {}
    for name, row in ALL_ROWS.items():
        for k, prec in enumerate(PRECISIONS):
            r = subprocess.run([str(checker), repr(row["alpha"]), repr(row.get("alpha_d", row["alpha"])), repr(row["cutoff"]), repr(row["padding"]), str(EC.LJPME), str(k)],
                               capture_output=True, text=True)
            assert r.returncode == 0, "ewald_fit_check exited with %d:\n%s" % (r.returncode, r.stderr[-4000:])
            d = {}
            for line in r.stdout.splitlines():
                key, *vals = line.split()
                d[key] = np.array([float(v) for v in vals]) if key.startswith("coef") else (int(vals[0]) if key in ("use", "degF") else float(vals[0]))
            out[name, prec] = d
    return out


CASES = [(n, p) for n in ALL_ROWS for p in PRECISIONS]


@pytest.mark.parametrize("name,prec", CASES)
def test_reported_residuals_are_not_optimistic(fits, name, prec):
    d = fits[name, prec]
    assert d["degF"] == (11 if prec == "single" else 16) and len(d["coefF"]) == d["degF"] + 1
    for key in ("errF", "errE", "errD", "pairF", "sysE", "pairD"):
        print("%s %s %s: reported %.3e, independent %.3e" % (name, prec, key, d[key], d["indep_" + key]))
        assert np.isfinite(d[key]) and d[key] >= 0.9 * d["indep_" + key], (name, prec, key, d[key], d["indep_" + key])


@pytest.mark.parametrize("name,prec", CASES)
def test_kept_polynomials_meet_the_guard_on_the_independent_evaluation(fits, name, prec):
    d, row = fits[name, prec], ALL_ROWS[name]
    bar = EC.BARS[prec]
    c6 = 4.0 * 1.0 * 0.4 ** 6
    if d["use"] & EC.FORCE:
        assert EC.K_COULOMB * d["indep_pairF"] <= 0.5 * bar
    if d["use"] & EC.DISPERSION:
        assert 6.0 * c6 * d["indep_pairD"] <= 0.5 * bar
    if d["use"] & EC.ENERGY:
        assert d["indep_sysE"] <= 1.5e-7 / row["cutoff"]
    # and a dropped one fails its condition: the guard is no stricter than stated
    if not d["use"] & EC.FORCE:
        assert EC.K_COULOMB * d["pairF"] > 0.5 * bar
    if not d["use"] & EC.DISPERSION:
        assert 6.0 * c6 * d["pairD"] > 0.5 * bar
    if not d["use"] & EC.ENERGY:
        assert d["sysE"] > 1.5e-7 / row["cutoff"]


@pytest.mark.parametrize("name,prec", CASES)
def test_decisions_are_the_ones_the_gpu_census_asserts(fits, name, prec):
    have = (EC.FORCE | EC.ENERGY) if prec == "single" else 7      # (no float kernel has a dispersion polynomial: the table leaves that bit out)
    assert fits[name, prec]["use"] & have == ALL_ROWS[name]["use"][PRECISIONS.index(prec)]


def test_benchmark_row_keeps_every_polynomial(fits):
    row = EC.ROWS["R0"]
    assert (row["cutoff"], row["alpha"], row["padding"]) == (1.0, 2.6283, 0.1)      # bench.py's workload
    for prec in PRECISIONS:
        assert fits["R0", prec]["use"] == EC.FORCE | EC.ENERGY | EC.DISPERSION


def test_rows_are_the_tolerances_they_claim():
    for name, tol in (("R0", 5e-4), ("R2", 1e-5), ("R4", 1e-6), ("R5", 5e-4), ("R6", 5e-4)):
        assert abs(EC.alpha_of_tolerance(tol, EC.ROWS[name]["cutoff"]) - EC.ROWS[name]["alpha"]) < 1e-3      # (the rows carry the alphas rounded to four figures)


# ------------------------------------------------------------------------------------------------------------------------------------
# 4: the emulation
# ------------------------------------------------------------------------------------------------------------------------------------
class _Recorder:
    """Stands in for SlicedNonbondedForce in systems.random_box: keeps the charges and the excluded pairs."""
    PME = EC.PME

    def __init__(self, nsub):
        self.q, self.excl = [], []

    def addParticle(self, q, sig, eps):
        self.q.append(q)

    def addException(self, a, b, *rest):
        self.excl.append((a, b))

    def __getattr__(self, name):
        return lambda *a, **k: None


@pytest.fixture(scope="session")
def box_pairs():
    """Every non-excluded pair of the 3000-atom box within 1.2 nm (the largest cutoff), minimum image: i, j, delta, r, q_i q_j."""
    n, L = 3000, 3.2
    f, pos, _ = systems.random_box(_Recorder, n, 3, EC.PME, L, 1.0)
    q = np.array(f.q)
    iu, ju = np.triu_indices(n, 1)
    d = pos[iu] - pos[ju]
    d -= L * np.rint(d / L)
    r = np.sqrt(np.einsum("ij,ij->i", d, d))
    excl = {a * n + b for a, b in f.excl} | {b * n + a for a, b in f.excl}
    keep = (r < 1.2) & ~np.isin(iu * n + ju, np.fromiter(excl, dtype=np.int64))
    return dict(n=n, i=iu[keep], j=ju[keep], d=d[keep], r=r[keep], qq=q[iu[keep]] * q[ju[keep]])


_erf = np.vectorize(math.erf, otypes=[np.float64])


def kernel_horner(coef, r2max, r2, f32):
    """The polynomial as the kernel evaluates it.  float: every FMA as a float64 product and sum rounded once more to float32 (the product
    of two floats is exact in float64)."""
    if not f32:
        t = r2 * (2.0 / r2max) - 1.0
        v = np.full_like(t, coef[-1])
        for c in coef[-2::-1]:
            v = v * t + c
        return v
    t = (r2.astype(np.float32).astype(np.float64) * np.float64(np.float32(2.0 / r2max)) - 1.0).astype(np.float32)
    v = np.full_like(t, np.float32(coef[-1]))
    for c in coef[-2::-1]:
        v = (v.astype(np.float64) * t.astype(np.float64) + np.float64(np.float32(c))).astype(np.float32)
    return v.astype(np.float64)


def emulate(bp, row, d, prec):
    """(error with the polynomial in use, reference force norms): per-atom |sum of pair errors| / max(|F|, 1) of the direct-space Coulomb force."""
    a, rc = row["alpha"], row["cutoff"]
    m = bp["r"] < rc
    r, qq, delta = bp["r"][m], bp["qq"][m], bp["d"][m]
    z = a * r
    bt = (_erf(z) - 2.0 * z / math.sqrt(math.pi) * np.exp(-z * z)) / r ** 3
    exact = EC.K_COULOMB * qq * (1.0 / r ** 3 - bt)      # force on i = this * delta
    dbt = kernel_horner(d["coefF"], d["r2max"], r * r, prec == "single") - bt
    F, dF = np.zeros((bp["n"], 3)), np.zeros((bp["n"], 3))
    for acc, s in ((F, exact), (dF, -EC.K_COULOMB * qq * dbt)):
        np.add.at(acc, bp["i"][m], s[:, None] * delta); np.add.at(acc, bp["j"][m], -s[:, None] * delta)
    return np.max(np.linalg.norm(dF, axis=1) / np.maximum(np.linalg.norm(F, axis=1), 1.0))


@pytest.mark.parametrize("name,prec", [(n, p) for n in EC.ROWS for p in PRECISIONS])
def test_emulated_forces(fits, box_pairs, name, prec):
    row, d, bar = EC.ROWS[name], fits[name, prec], EC.BARS[prec]
    always = emulate(box_pairs, row, d, prec)
    guarded = always if d["use"] & EC.FORCE else 0.0      # (the analytic branch is not the polynomial's error)
    print("%s %s: emulated force error with the polynomial %.3e (%.3g bars); polynomial %s" % (name, prec, always, always / bar, "kept" if d["use"] & EC.FORCE else "dropped"))
    assert np.isfinite(always)
    assert guarded <= bar / 20.0
    if prec in row["parent_fails"]:
        assert always > bar, "the row no longer shows the defect"
