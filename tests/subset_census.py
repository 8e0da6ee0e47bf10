"""Systems, lambda table and bars of the subset-count census (tests/test_subset_census.py on the CPU, tests/test_gpu_subset_census.py on the GPU).

Why.  The engine takes any n_subsets >= 1, no other test runs more than 8, and the reciprocal pipeline changes its code at exactly the counts
above: from 9 subsets on a single-precision engine leaves the plane path for the three-pass pipeline, whose x kernel (pme.hip k_convolveX) mixes
the spectra with the lambda matrix in one of three forms -- 4 x 4 x 1 matrix-core instructions up to 4 subsets, 16 x 16 x 4 ones up to 16 (K
chunks nK = (nsub + 3) / 4: the third and fourth had never run, nor a partly filled last group of output rows), a scalar loop above -- and
sizes its columns per work-group NB = 8, 4, 2, 1 from the subset count (csrc/pme_sizes.h).

The systems are the lattice of recip_systems.ortho cut into nsub slabs along y, with the three special subsets of recip_systems.subsets5, under
a lambda table that gives every slice a value of its own, diagonals included: with 78 or more slices a transposed or shifted index into the
lambda matrix must not land on an equal value.

Forces: recip_systems.compare unchanged.  Slice energies in single and mixed precision:

    |dE_IJ| <= tol max(|E_IJ|, 1, rho_min sqrt(M_II M_JJ))

M_II is the mesh sum of the diagonal slice -- the oracle's reciprocal E_II less the closed-form self term -- and rho_min the smallest
|E_IJ| / sqrt(M_II M_JJ) over the off-diagonal slices of recip_systems.ortho, from the oracle alone.  The rounding noise of a float mesh sum
follows the spectra that enter it, sqrt(M_II M_JJ), not |E_IJ|: two thin slabs far apart have a small E_IJ between large spectra.  The third
term asks the absolute mesh accuracy that the reciprocal census already asks on its own hardest slice (on `ortho` it changes nothing); the CPU
test asserts that it decides at most 5 % of a row's live off-diagonal slices.  Double precision keeps the suite's rule, and so does the
dispersion term in every precision: its kernel has one sign, the diagonal mesh sums hold the close pairs inside a slab and dwarf the sums
between slabs (|E_IJ| of a few kJ/mol), so rho_min sqrt(M_II M_JJ) would decide 18 of the 45 slab pairs of the LJPME row -- a bar that is
mostly floor is no bar, and max(|E|, 1) is the stricter one."""
import numpy as np

import recip_systems as R
import shell_systems as S

TOLS = R.TOLS
GOLD, SILVER = 0.6180339887, 0.4142135623
# the mesh term takes over only where it exceeds max(|E|, 1) by this much: on the slice of `ortho` that defines rho_min the two are equal by
# construction, and the oracle's threaded sums differ in their last bits from one evaluation to the next
MARGIN = 1e-9

# row -> (subsets, method, dispersion mesh, precisions)
ROWS = {
    "n7": (7, 4, (0, 0, 0), ("single",)),                      # plane path: k_fftZInvMix with more than 4 subsets and the three special ones
    "n9": (9, 4, (0, 0, 0), ("single",)),                      # first count off the plane path; nK = 3
    "n12": (12, 4, (0, 0, 0), ("single", "mixed", "double")),
    "n13": (13, 4, (0, 0, 0), ("single",)),                    # nK = 4, a partly filled last group of output rows
    "n16": (16, 4, (0, 0, 0), ("single",)),                    # last count of the matrix-core form
    "n17": (17, 4, (0, 0, 0), ("single", "mixed")),            # first count of the scalar float form
    "n20": (20, 4, (0, 0, 0), ("single", "double")),
    "n12_ljpme": (12, 5, R.ORTHO_DGRID_TILING, ("single", "double")),      # the mix with term = 1
}
CASES = [(row, prec) for row, r in ROWS.items() for prec in r[3]]
# columns per work-group of k_convolveX on the Coulomb mesh (nx = 40) at the default budget; `mixed` runs the float kernels
EXPECT_NB = {("n9", "single"): 8, ("n12", "single"): 8, ("n12", "mixed"): 8, ("n13", "single"): 8, ("n12_ljpme", "single"): 8,
             ("n16", "single"): 4, ("n17", "single"): 4, ("n17", "mixed"): 4, ("n20", "single"): 4, ("n12", "double"): 4, ("n12_ljpme", "double"): 4,
             ("n20", "double"): 2}
CONV_LDS_KB = 72          # switches.h SNB_CONV_LDS_KB


def conv_lds(nx, nsub, real_bytes, lds_kb=CONV_LDS_KB):
    """(NB, dynamic LDS bytes) of the x kernel: csrc/pme_sizes.h restated (tests/pme_sizes_check.cpp prints the header's own for the census rows,
    and the CPU test holds the two together)."""
    per_col = 2 * nx * nsub * 2 * real_bytes + nx * real_bytes
    nb = 8
    while nb > 1 and per_col * nb > lds_kb * 1024:
        nb >>= 1
    return nb, per_col * nb + nx * 2 * real_bytes


def lambdas(nsub):
    """(Coulomb, vdW) of slice s: 0.05 + 0.9 frac((s + 1) phi), phi the golden ratio's and sqrt(2)'s fractional part -- all distinct, none 0 or 1."""
    s = np.arange(nsub * (nsub + 1) // 2) + 1.0
    return np.ascontiguousarray(np.stack([0.05 + 0.9 * np.mod(s * GOLD, 1.0), 0.05 + 0.9 * np.mod(s * SILVER, 1.0)], axis=1))


def uncharged(nsub): return nsub // 2
def empty(nsub): return nsub - 2
def single(nsub): return nsub - 1


def many(nsub, method=4, dgrid=(0, 0, 0), name=None):
    """The `ortho` lattice (13 608 atoms, 5.6 x 6.4 x 7.2 nm, mesh 40 x 54 x 48) in nsub slabs along y; then, as recip_systems.subsets5: subset
    nsub // 2 keeps its atoms and loses its charges, subset nsub - 2 gets no atoms (its slab joins nsub - 3), subset nsub - 1 is one atom (its
    slab joins subset 0; the atom is the 101st of subset 0)."""
    assert nsub >= 7
    s = R.ortho(method, dgrid, name or "many%d" % nsub)
    sub = R._slabs(s["pos"], 1, S.ORTHO_LENGTHS[1], nsub).astype(np.int32)
    sub[sub == empty(nsub)] = nsub - 3
    sub[sub == single(nsub)] = 0
    s["q"] = np.where(sub == uncharged(nsub), 0.0, s["q"])
    sub[int(np.where(sub == 0)[0][100])] = single(nsub)
    s["subset"] = np.ascontiguousarray(sub); s["nsub"] = nsub; s["lam"] = lambdas(nsub)
    return s


_BUILT = {}


def build(row):
    """The system of a row, built once per session (callers must not modify it).  `ortho`: the three slabs of recip_systems, as they are."""
    if row == "ortho":
        return R.build("ortho")
    if row not in _BUILT:
        nsub, method, dgrid, _ = ROWS[row]
        _BUILT[row] = many(nsub, method, dgrid, row)
    return _BUILT[row]


def live_subsets(s, term=0):
    """The subsets that put something on the mesh of a term: a charged atom, or (dispersion) an atom with a c6."""
    w = (s["q"] != 0) if term == 0 else (s["epsilon"] != 0)
    return [i for i in range(s["nsub"]) if (w & (s["subset"] == i)).any()]


# ---- the energy bar --------------------------------------------------------------------------------------------------------------------
def self_terms(s):
    """[nsub][2]: the closed-form self terms in the oracle's diagonal slices: -K alpha / sqrt(pi) sum q^2, and (LJPME) + alpha_d^6 / 12 sum c6^2
    with c6 = 8 sigma^3 epsilon."""
    out = np.zeros((s["nsub"], 2))
    for i in range(s["nsub"]):
        m = s["subset"] == i
        out[i, 0] = -S.K_COULOMB * s["alpha"] / np.sqrt(np.pi) * (s["q"][m] ** 2).sum()
        if s["method"] == 5:
            out[i, 1] = s["alpha_d"] ** 6 / 12.0 * ((8.0 * s["sigma"][m] ** 3 * s["epsilon"][m]) ** 2).sum()
    return out


def mesh_sums(s, eo):
    """M[nsub][2]: the diagonal mesh sums, the oracle's reciprocal E_II less the self term, as magnitudes: the dispersion kernel is negative at
    every wave vector, so its mesh sums are taken with the opposite sign.  Positive for every live subset (asserted on the CPU).
    eo: reciprocal-only slice energies of the oracle."""
    diag = np.array([eo[R.sl(i, i)] for i in range(s["nsub"])])
    return (diag - self_terms(s)) * np.array([1.0, -1.0])


_RHO = []


def rho_min():
    """The smallest |E_IJ| / sqrt(M_II M_JJ) over the off-diagonal Coulomb slices of `ortho` (3 slabs), from the oracle."""
    if not _RHO:
        s = R.build("ortho")
        _, eo = R.oracle_eval(s)
        m = mesh_sums(s, eo)[:, 0]
        assert (m > 0).all(), m
        _RHO.append(min(abs(eo[R.sl(i, j), 0]) / np.sqrt(m[i] * m[j]) for i in range(3) for j in range(i)))
    return _RHO[0]


def energy_scale(s, eo, prec):
    """scale[S][2] with the bar |dE| <= tol scale, and floor[S][2]: where the mesh term decides.  eo: the oracle's reciprocal-only slice energies."""
    scale = np.maximum(np.abs(eo), 1.0)
    floor = np.zeros(scale.shape, dtype=bool)
    if prec == "double":
        return scale, floor
    m = mesh_sums(s, eo)
    rho = rho_min()
    for i in range(s["nsub"]):
        for j in range(i):
            f = rho * np.sqrt(max(m[i, 0], 0.0) * max(m[j, 0], 0.0))
            k = R.sl(i, j)
            if f > scale[k, 0] * (1.0 + MARGIN):
                scale[k, 0] = f; floor[k, 0] = True
    return scale, floor


def compare_energies(s, se, eo, prec):
    """Raw reciprocal-only slice energies against the oracle's at the bar above.  Returns (ok, worst error in units of the bar's scale, the
    slice and term of the worst, worst absolute error); the slices of the empty subset must be exactly 0."""
    se = np.asarray(se)
    scale, _ = energy_scale(s, eo, prec)
    err = np.abs(se - eo) / scale
    k, t = np.unravel_index(int(np.nanargmax(np.where(np.isnan(err), np.inf, err))), err.shape)
    ok = bool((err <= TOLS[prec]).all())
    if s["nsub"] >= 7:
        e = empty(s["nsub"])
        ok = ok and all((se[R.sl(e, j)] == 0).all() for j in range(s["nsub"]))
    return ok, float(err[k, t]), (int(k), int(t)), float(np.abs(se - eo).max())


def slice_pair(k):
    """(i, j), i >= j, of slice k."""
    i = int((np.sqrt(8 * k + 1) - 1) // 2)
    while i * (i + 1) // 2 > k:
        i -= 1
    while (i + 1) * (i + 2) // 2 <= k:
        i += 1
    return i, k - i * (i + 1) // 2


def derivative_mask(s):
    """Six wanted slices for a derivative-only step -- one full group of four in the x kernel's flush and a remainder of two -- with a
    diagonal, a slice of the uncharged subset and a slice of the empty one among them."""
    n = s["nsub"]
    want = [R.sl(1, 1), R.sl(uncharged(n), 1), R.sl(empty(n), 2), R.sl(n - 3, 0), R.sl(single(n), n - 3), R.sl(3, 2)]
    assert len(set(want)) == 6
    mask = np.zeros(len(s["lam"]), dtype=np.int32)
    mask[want] = 1
    return mask
