"""Ground truth of the group-pair interaction energy matrix (snb_evaluate_group_pair_energies), from the oracle alone -- never from the engine.

The relabelling rule: every atom's subset is replaced by its label, the unlabelled atoms (label -1) go to one extra subset G, and the
oracle's DIRECT-ONLY raw slice energies of that (G + 1)-subset system (lambdas all 1, no dispersion correction) are the matrix: row
slice(g, h) for g, h < G; the rows of the extra subset are dropped.  One oracle evaluation per (system, labelling).

`evaluator(subset, nsub)` is that of tests/atom_energy_truth.py, made with include_reciprocal = 0: direct_workload_evaluator and
direct_force_evaluator below do that."""
import numpy as np

import atom_energy_truth as aet
from atom_energy_truth import slice_index      # noqa: F401 (the row of a label pair)


def num_pairs(G):
    return G * (G + 1) // 2


def direct_workload_evaluator(w, method, grid, dgrid):
    return aet.workload_evaluator(w, method, grid, dgrid, include_direct=1, include_reciprocal=0)


def direct_force_evaluator(oracle, force, pos, box, parameters=None, **kw):
    return aet.force_evaluator(oracle, force, pos, box, parameters, include_direct=True, include_reciprocal=False, **kw)


def relabelled(labels, G):
    """The subset assignment the rule evaluates: the labels, with -1 replaced by the extra subset G."""
    lab = np.asarray(labels, dtype=np.int64).reshape(-1)
    assert ((lab >= -1) & (lab < G)).all()
    return np.where(lab < 0, G, lab).astype(np.int32)


def truth(evaluator, labels, G):
    """M = [G (G + 1) / 2][2].  (slice(g, h) < G (G + 1) / 2 exactly when both labels are below G: the kept rows are the first ones.)"""
    e = np.asarray(evaluator(relabelled(labels, G), G + 1), dtype=np.float64)
    assert e.shape == (num_pairs(G + 1), 2)
    return np.array(e[:num_pairs(G)])


def merged(M, G, g, h):
    """The matrix of the labelling in which label h is merged into label g (g < h; the labels above h move down by one): what the merge
    rule M'[gg] = M[gg] + M[hh] + M[gh], M'[gk] = M[gk] + M[hk] says, written out for every row."""
    assert 0 <= g < h < G
    new = lambda a: g if a == h else (a - 1 if a > h else a)
    out = np.zeros((num_pairs(G - 1), 2))
    for a in range(G):
        for b in range(a + 1):
            out[slice_index(new(a), new(b))] += M[slice_index(a, b)]
    return out


def group_totals(M, G):
    """T[g] = sum_h (1 + delta_gh) M[g][h]: the pairs of group g with everything, those inside g from both ends -- what the direct-only row
    of the group-energy table (tests/group_energy_truth.py), summed over the subsets, holds when every atom is labelled."""
    out = np.zeros((G, 2))
    for g in range(G):
        for h in range(G):
            out[g] += (2.0 if g == h else 1.0) * M[slice_index(g, h)]
    return out
