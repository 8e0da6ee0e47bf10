"""Ground truth of the per-atom forces by subset and term (snb_evaluate_atom_forces), from the oracle alone -- never from the engine.

E_raw is linear in the lambdas, so the oracle's forces with lambda one-hot at (slice s = (I, J), term t) are -dE_raw[s][t]/dr: on the
atoms of I they are column J of the table, on the atoms of J (I != J) column I, and on every other atom exactly zero (asserted).  2 S
evaluations give the whole table G[N][nsub][2][3].

`evaluator(lam)` returns the oracle's forces [N][3] for a lambda table [S][2]; the two factories below make one from a bench workload
(bench.oracle_eval) and from a SlicedNonbondedForce (oracle.evaluate with 2 S scaling parameters, one per (slice, term))."""
import numpy as np


def slice_index(i, j):
    return i * (i + 1) // 2 + j if i > j else j * (j + 1) // 2 + i


def truth_table(evaluator, subset, nsub):
    """G[N][nsub][2][3] from 2 S one-hot evaluations."""
    subset = np.asarray(subset)
    S = nsub * (nsub + 1) // 2
    table = np.zeros((len(subset), nsub, 2, 3))
    for i in range(nsub):
        for j in range(i + 1):
            s = slice_index(i, j)
            in_i, in_j = subset == i, subset == j
            for t in range(2):
                lam = np.zeros((S, 2)); lam[s, t] = 1.0
                f = np.asarray(evaluator(lam), dtype=np.float64)
                assert f.shape == (len(subset), 3)
                assert not f[~(in_i | in_j)].any(), "slice (%d, %d) term %d: a force on an atom outside the slice's subsets" % (i, j, t)
                table[in_i, j, t] = f[in_i]
                if i != j:
                    table[in_j, i, t] = f[in_j]
    return table


def contract(table, subset, lam):
    """F[N][3] = sum_J sum_t lam[slice(s_i, J)][t] G[i][J][t], written out independently of the package's helper."""
    table = np.asarray(table); subset = np.asarray(subset); lam = np.asarray(lam)
    out = np.zeros((table.shape[0], 3))
    for a in range(table.shape[0]):
        for j in range(table.shape[1]):
            for t in range(2):
                out[a] += lam[slice_index(int(subset[a]), j), t] * table[a, j, t]
    return out


def third_law(table, subset, nsub):
    """sum_{i in I} G[i][J][t] + sum_{j in J} G[j][I][t] for every slice and term, [S][2][3] (once, not twice, on the diagonal): zero for
    pair forces."""
    table = np.asarray(table); subset = np.asarray(subset)
    out = np.zeros((nsub * (nsub + 1) // 2, 2, 3))
    for i in range(nsub):
        for j in range(i + 1):
            out[slice_index(i, j)] = table[subset == i, j].sum(axis=0) + (table[subset == j, i].sum(axis=0) if i != j else 0.0)
    return out


def errors(got, want, allow=None):
    """The reference's scale rule on 3-vectors, ||got - want|| / max(||want||, 1) per (i, J, t) -> [N][nsub][2].  allow [N]: an absolute
    allowance per atom (the force of its cutoff-band pairs), granted to every one of its columns before the division."""
    got = np.asarray(got, dtype=np.float64); want = np.asarray(want, dtype=np.float64)
    err = np.linalg.norm(got - want, axis=-1)
    if allow is not None:
        err = np.maximum(err - np.asarray(allow).reshape((-1,) + (1,) * (err.ndim - 1)), 0.0)
    return err / np.maximum(np.linalg.norm(want, axis=-1), 1.0)


def rel(got, want, allow=None):
    """... worst entry."""
    return float(errors(got, want, allow).max())


def workload_evaluator(w, method, grid, dgrid, include_direct=1, include_reciprocal=1):
    import bench

    def ev(lam):
        v = dict(w)
        v["lam"] = np.ascontiguousarray(lam, dtype=np.float64)
        return bench.oracle_eval(v, method, grid, dgrid, include_direct, include_reciprocal)[0]
    return ev


class _OneHot:
    """A SlicedNonbondedForce seen with 2 S scaling parameters of its own, one per (slice, term), and no dispersion correction (what
    oracle.resolve reads): parameters={name(s, t): value} sets the lambda table entry by entry."""

    def __init__(self, force):
        self._f = force
        n = force.getNumSubsets()
        self._sp = []
        for i in range(n):
            for j in range(i + 1):
                for t in range(2):
                    self._sp.append((self.name(slice_index(i, j), t), i, j, t == 0, t == 1))

    @staticmethod
    def name(s, t):
        return "__slice%d_term%d" % (s, t)

    def __getattr__(self, name):
        return getattr(self._f, name)

    def getNumScalingParameters(self): return len(self._sp)
    def getScalingParameter(self, k): return self._sp[k]
    def getNumEnergyParameterDerivatives(self): return 0
    def getUseDispersionCorrection(self): return False


def force_evaluator(oracle, force, pos, box, parameters=None, include_direct=True, include_reciprocal=True, **kw):
    view = _OneHot(force)

    def ev(lam):
        lam = np.asarray(lam)
        par = dict(parameters or {})
        for s in range(lam.shape[0]):
            for t in range(2):
                par[view.name(s, t)] = float(lam[s, t])
        return oracle.evaluate(view, pos, box, par, include_direct, include_reciprocal, **kw)["forces"]
    return ev


def force_subsets(force):
    return np.array([force.getParticleSubset(i) for i in range(force.getNumParticles())], dtype=np.int32)
