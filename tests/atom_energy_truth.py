"""Ground truth of the per-atom interaction energies (snb_evaluate_atom_energies), from the oracle alone -- never from the engine.

The singled-out rule: move atom a of subset I alone into a new subset n = n_subsets; with E' the raw slice energies of that (n + 1)-subset
system (lambdas all 1, no dispersion correction),

    A[a][J] = E'[slice(n, J)]  (J != I),        A[a][I] = E'[slice(n, I)] + 2 E'[slice(n, n)] .

`evaluator(subset, nsub)` returns the oracle's raw slice energies [(nsub (nsub + 1) / 2), 2] for a subset assignment; the two factories
below make one from a bench workload (bench.oracle_eval) and from a SlicedNonbondedForce (oracle.evaluate)."""
import numpy as np


def slice_index(i, j):
    return i * (i + 1) // 2 + j if i > j else j * (j + 1) // 2 + i


def singled_out(evaluator, subset, nsub, a):
    """Row A[a] = [nsub][2] of the table."""
    sub = np.array(subset, dtype=np.int32)
    own = int(sub[a])
    sub[a] = nsub
    e = evaluator(sub, nsub + 1)
    row = np.array([e[slice_index(nsub, j)] for j in range(nsub)], dtype=np.float64)
    row[own] += 2.0 * e[slice_index(nsub, nsub)]
    return row


def truth_table(evaluator, subset, nsub, atoms=None):
    """{atom: row} for the atoms named (default: every atom, as an array [N][nsub][2])."""
    if atoms is None:
        return np.stack([singled_out(evaluator, subset, nsub, a) for a in range(len(subset))])
    return {int(a): singled_out(evaluator, subset, nsub, int(a)) for a in atoms}


def reduce_by_sum_rule(table, subset, nsub):
    """The slice energies a table implies, written out independently of the package's helper: both halves of an off-diagonal slice are
    returned (from the atoms of I against J and from the atoms of J against I), the diagonal halved."""
    table = np.asarray(table); subset = np.asarray(subset)
    lo = np.zeros((nsub * (nsub + 1) // 2, 2)); hi = np.zeros_like(lo)
    for i in range(nsub):
        rows = table[subset == i].sum(axis=0)
        for j in range(nsub):
            if i == j:
                lo[slice_index(i, i)] = hi[slice_index(i, i)] = 0.5 * rows[i]
            elif i > j:
                hi[slice_index(i, j)] = rows[j]
            else:
                lo[slice_index(i, j)] = rows[j]
    return lo, hi


def rel(got, want):
    """The reference's scale rule |got - want| / max(|want|, 1), worst entry."""
    got = np.asarray(got, dtype=np.float64); want = np.asarray(want, dtype=np.float64)
    return float(np.max(np.abs(got - want) / np.maximum(np.abs(want), 1.0)))


def workload_evaluator(w, method, grid, dgrid, include_direct=1, include_reciprocal=1):
    import bench

    def ev(subset, nsub):
        v = dict(w)
        v["subset"] = np.ascontiguousarray(subset, dtype=np.int32); v["nsub"] = nsub
        v["lam"] = np.ones((nsub * (nsub + 1) // 2, 2))
        return bench.oracle_eval(v, method, grid, dgrid, include_direct, include_reciprocal)[1]
    return ev


class _Resubset:
    """A SlicedNonbondedForce seen with another subset assignment, every lambda 1 and no dispersion correction (what oracle.resolve reads)."""

    def __init__(self, force, subset, nsub):
        self._f, self._sub, self._n = force, subset, nsub

    def __getattr__(self, name):
        return getattr(self._f, name)

    def getNumSubsets(self): return self._n
    def getParticleSubset(self, i): return int(self._sub[i])
    def getNumScalingParameters(self): return 0
    def getNumEnergyParameterDerivatives(self): return 0
    def getUseDispersionCorrection(self): return False


def force_evaluator(oracle, force, pos, box, parameters=None, include_direct=True, include_reciprocal=True, **kw):
    def ev(subset, nsub):
        return oracle.evaluate(_Resubset(force, subset, nsub), pos, box, parameters, include_direct, include_reciprocal, **kw)["slice_energies"]
    return ev


def force_subsets(force):
    return np.array([force.getParticleSubset(i) for i in range(force.getNumParticles())], dtype=np.int32)
