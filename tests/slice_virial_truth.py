"""Ground truth of the per-slice virial tensors (snb_evaluate_slice_virials), from the oracle alone -- never from the engine.

W[s][t][c] = -dE_raw[s][t]/dh along the six deformations x'_a = x_a + h x_b, (a, b) = xx, yy, zz, xy, xz, yz: the matrix I + h e_a e_b^T
applied to every position and to every box row (a < b adds a higher component into a lower one, so the box stays lower-triangular).  The
derivative is the 4-point stencil at +-h and +-2h, h = 1e-4, of oracle.evaluate(...)["slice_energies"]: 24 evaluations.

Two conditions are ASSERTED on every call, not measured:

1. Empty cutoff shell.  No pair lies within 4 h r_c of the cutoff (minimum image; plain distance for a non-periodic system).  A pair that
   crosses the cutoff during the stencil puts the impulsive term of the truncated potential into the truth, which the forces -- and the
   engine's virial at fixed pair set -- do not have.  clear_shell() nudges offending atoms until the shell is empty.
2. Self-consistency.  The stencil at step h and the same stencil at step 2h (+-2h, +-4h: 12 more evaluations; the deformation reaches 4 h,
   which is what condition 1 covers) agree to within one tenth of the double-precision bar (1e-5) times the entry's scale,
   max(||W||_F, |E_raw[s][t]|, 1).  Their truncation errors are h^4 f^(5) / 30 and 16 times that -- 1e-11 of the entry for r^-12 -- so the
   difference measures the rounding noise of the energies divided by h.  (The two CENTRAL differences at h and 2h cannot serve: they
   differ by h^2 f''' / 2, 1e-6 of the entry for r^-12, the size of the bar itself.)
"""
import numpy as np

H = 1e-4
BAR = 0.1 * 1e-5      # one tenth of the double-precision bar
COMPONENTS = ((0, 0), (1, 1), (2, 2), (0, 1), (0, 2), (1, 2))      # xx, yy, zz, xy, xz, yz


def slice_index(i, j):
    return i * (i + 1) // 2 + j if i > j else j * (j + 1) // 2 + i


def deform(pos, box, a, b, h):
    """x'_a = x_a + h x_b on the positions [N][3] and on the box rows [3][3] (None: non-periodic)."""
    m = np.eye(3); m[a, b] += h
    return np.asarray(pos, dtype=np.float64) @ m.T, (None if box is None else np.asarray(box, dtype=np.float64).reshape(3, 3) @ m.T)


def frobenius(rows):
    """Frobenius norm of symmetric tensors given as rows [..., 6]: the off-diagonal entries count twice."""
    rows = np.asarray(rows, dtype=np.float64)
    return np.sqrt((rows[..., :3] ** 2).sum(axis=-1) + 2.0 * (rows[..., 3:] ** 2).sum(axis=-1))


def scale_of(want, energies):
    """max(||want||_F, |E_raw[s][t]|, 1) per (slice, term)."""
    return np.maximum(np.maximum(frobenius(want), np.abs(np.asarray(energies))), 1.0)


def ratios(got, want, energies):
    """||got - want||_F / scale per (slice, term) -> [S][2]."""
    return frobenius(np.asarray(got, dtype=np.float64) - np.asarray(want, dtype=np.float64)) / scale_of(want, energies)


def pair_distances(pos, box):
    """Distances of all pairs i < j, minimum image in the lower-triangular box (OpenMM's getDeltaRPeriodic), plain when box is None."""
    pos = np.asarray(pos, dtype=np.float64)
    i, j = np.triu_indices(len(pos), 1)
    d = pos[i] - pos[j]
    if box is not None:
        bx = np.asarray(box, dtype=np.float64).reshape(3, 3)
        for k in (2, 1, 0):
            d -= np.floor(d[:, k] / bx[k, k] + 0.5)[:, None] * bx[k]
    return i, j, np.sqrt((d * d).sum(axis=1))


def shell_pairs(pos, box, r_c, margin):
    """The pairs (i, j) whose distance lies within `margin` of the cutoff.  Thousands of atoms in a rectangular cell: the candidates from a
    periodic k-d tree instead of all pairs."""
    pos = np.asarray(pos, dtype=np.float64)
    if len(pos) > 2000 and box is not None:
        from scipy.spatial import cKDTree
        bx = np.asarray(box, dtype=np.float64).reshape(3, 3)
        assert not (bx - np.diag(np.diag(bx))).any()
        edges = np.diag(bx)
        inside = np.mod(pos, edges)
        inside = np.where(inside >= edges, 0.0, inside)
        near = cKDTree(inside, boxsize=edges).query_pairs(r_c + margin, output_type="ndarray")
        d = pos[near[:, 0]] - pos[near[:, 1]]
        d -= np.round(d / edges) * edges
        hit = np.abs(np.sqrt((d * d).sum(axis=1)) - r_c) < margin
        return near[hit, 0], near[hit, 1]
    i, j, r = pair_distances(pos, box)
    hit = np.abs(r - r_c) < margin
    return i[hit], j[hit]


def clear_shell(pos, box, r_c, margin, rng, rounds=200, single=True):
    """Positions with no pair within `margin` of the cutoff: an offending atom is nudged by at most 0.01 nm and the shell is checked again.
    single: the result is rounded to float32 (what an engine of any precision is given) before every check."""
    pos = np.array(pos, dtype=np.float64)
    for n in range(rounds):
        if single:
            pos = pos.astype(np.float32).astype(np.float64)
        i, _ = shell_pairs(pos, box, r_c, margin)
        if len(i) == 0:
            return pos, n
        for a in np.unique(i):
            pos[a] += rng.uniform(-0.01, 0.01, 3) / np.sqrt(3.0)
    raise AssertionError("clear_shell: the cutoff shell is not empty after %d rounds" % rounds)


def _stencil(energy, pos, box, a, b, h):
    e = {k: energy(*deform(pos, box, a, b, k * h)) for k in (-2, -1, 1, 2)}
    return -(-e[2] + 8.0 * e[1] - 8.0 * e[-1] + e[-2]) / (12.0 * h)


def truth(energy, pos, box, r_c=None, h=H):
    """W[S][2][6], E_raw[S][2] and the worst self-consistency ratio.  energy(pos, box) returns the oracle's raw slice energies [S][2];
    r_c: the cutoff whose shell must be empty (None: a method without a cutoff)."""
    pos = np.asarray(pos, dtype=np.float64)
    if r_c is not None:
        i, j = shell_pairs(pos, box, r_c, 4.0 * h * r_c)
        assert len(i) == 0, "a pair within 4 h r_c of the cutoff: atoms %s" % list(zip(i.tolist(), j.tolist()))[:4]
    e0 = np.asarray(energy(pos, box), dtype=np.float64)
    w = np.zeros(e0.shape + (6,)); w2 = np.zeros_like(w)
    for c, (a, b) in enumerate(COMPONENTS):
        w[..., c] = _stencil(energy, pos, box, a, b, h)
        w2[..., c] = _stencil(energy, pos, box, a, b, 2.0 * h)
    worst = float(ratios(w2, w, e0).max())
    assert worst < BAR, "the stencils at h and 2h differ by %.3e of the entry's scale" % worst
    return w, e0, worst


def force_energy(oracle, force, parameters=None, include_direct=True, include_reciprocal=True, **kw):
    """energy(pos, box) for a SlicedNonbondedForce: the raw slice energies of oracle.evaluate."""
    def energy(pos, box):
        return oracle.evaluate(force, pos, box, parameters, include_direct, include_reciprocal, **kw)["slice_energies"]
    return energy


def pair_sum(force, pos):
    """W[S][2][6] of a NoCutoff system written out: sum over the pairs of d_a d_b f, f = -E'(r) / r, Lorentz-Berthelot pairs less the
    exceptions, plus the exceptions with their own parameters."""
    ONE_4PI_EPS0 = 138.93545764438198
    pos = np.asarray(pos, dtype=np.float64)
    n = force.getNumParticles(); nsub = force.getNumSubsets()
    par = np.array([force.getParticleParameters(i) for i in range(n)], dtype=np.float64)
    sub = [force.getParticleSubset(i) for i in range(n)]
    w = np.zeros((nsub * (nsub + 1) // 2, 2, 6))

    def add(i, j, qq, sig, eps):
        d = pos[i] - pos[j]
        r2 = float(d @ d); r = np.sqrt(r2)
        s6 = (sig / r) ** 6
        f = (ONE_4PI_EPS0 * qq / (r2 * r), 4.0 * eps * (12.0 * s6 * s6 - 6.0 * s6) / r2)
        for t in range(2):
            for c, (a, b) in enumerate(COMPONENTS):
                w[slice_index(sub[i], sub[j]), t, c] += d[a] * d[b] * f[t]
    special = set()
    for k in range(force.getNumExceptions()):
        i, j, qq, sig, eps = force.getExceptionParameters(k)
        special.add((min(i, j), max(i, j)))
        if qq != 0.0 or eps != 0.0:
            add(i, j, float(qq), float(sig), float(eps))
    for i in range(n):
        for j in range(i + 1, n):
            if (i, j) not in special:
                add(i, j, par[i, 0] * par[j, 0], 0.5 * (par[i, 1] + par[j, 1]), np.sqrt(par[i, 2] * par[j, 2]))
    return w
