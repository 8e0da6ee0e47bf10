"""Ground truth of the per-group interaction energies (snb_evaluate_group_energies), from the oracle alone -- never from the engine.

The moved-group rule: a group P that lies in one subset I is moved whole into a new subset n = n_subsets; with E' the raw slice energies of
that (n + 1)-subset system (lambdas all 1, no dispersion correction),

    B[P][J] = E'[slice(n, J)]  (J != I),        B[P][I] = E'[slice(n, I)] + 2 E'[slice(n, n)]

-- the pairs of P with the rest of I once, the pairs inside P (and P's self terms) from both ends, as the rows of the atom-energy table count
them.  A group that spans subsets is the sum of its per-subset parts: one oracle evaluation per part, whatever the part's size.  An index
listed k times counts k times: the list is peeled into layers of distinct atoms.

`evaluator(subset, nsub)` is that of tests/atom_energy_truth.py (workload_evaluator, force_evaluator)."""
import numpy as np

from atom_energy_truth import slice_index


def part_row(evaluator, subset, nsub, atoms, own):
    """B[P] = [nsub][2] for distinct atoms P, all of subset `own`."""
    sub = np.array(subset, dtype=np.int32)
    atoms = np.asarray(atoms, dtype=np.int64)
    assert len(np.unique(atoms)) == len(atoms) and (sub[atoms] == own).all()
    sub[atoms] = nsub
    e = evaluator(sub, nsub + 1)
    row = np.array([e[slice_index(nsub, j)] for j in range(nsub)], dtype=np.float64)
    row[own] += 2.0 * e[slice_index(nsub, nsub)]
    return row


def group_row(evaluator, subset, nsub, atoms):
    """B[g] = [nsub][2] for any list of atom indices: empty (zeros), across subsets, with repeats."""
    subset = np.asarray(subset)
    row = np.zeros((nsub, 2))
    idx, count = np.unique(np.asarray(list(atoms), dtype=np.int64), return_counts=True)
    for layer in range(int(count.max()) if len(count) else 0):
        members = idx[count > layer]
        for own in np.unique(subset[members]):
            row += part_row(evaluator, subset, nsub, members[subset[members] == own], int(own))
    return row


def truth(evaluator, subset, nsub, groups):
    """[G][nsub][2] for a list of groups."""
    return np.stack([group_row(evaluator, subset, nsub, g) for g in groups])
