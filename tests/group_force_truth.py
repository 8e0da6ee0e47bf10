"""Ground truth of the per-group forces (snb_evaluate_group_forces), from the oracle alone -- never from the engine.

rows:    group_forces[g][J][t] = sum_{i in g} G[i][J][t], with G the one-hot truth table of tests/atom_force_truth.py (2 S oracle
         evaluations for all groups at once).
states:  state_forces[k][g] = sum_{i in g} F_i(lambda_k), with F(lambda_k) the oracle's PLAIN forces at lambda state k: one oracle evaluation
         per (frame, state), no one-hot evaluations -- E_raw is linear in the lambdas, so this is the contraction of the table
         (atom_force_truth.contract), which tests/test_group_forces_cpu.py checks on a 40-atom box.

A group is any list of atom indices: empty (zeros), across subsets, overlapping others; an index listed k times counts k times."""
import numpy as np

from atom_force_truth import truth_table


def group_sum(per_atom, groups):
    """[G] + per_atom.shape[1:]: the per-atom array summed over each list."""
    per_atom = np.asarray(per_atom, dtype=np.float64)
    out = np.zeros((len(groups),) + per_atom.shape[1:])
    for g, atoms in enumerate(groups):
        idx = np.asarray(list(atoms), dtype=np.int64)
        if len(idx):
            out[g] = per_atom[idx].sum(axis=0)
    return out


def rows_truth(table, groups):
    """[G][nsub][2][3] from a truth table [N][nsub][2][3]."""
    return group_sum(table, groups)


def rows(evaluator, subset, nsub, groups):
    """... from an evaluator of tests/atom_force_truth.py (2 S one-hot evaluations)."""
    return rows_truth(truth_table(evaluator, subset, nsub), groups)


def state_truth(forces_at_lambda_k, groups):
    """[G][3]: the oracle's plain forces [N][3] at lambda state k summed over each list."""
    f = np.asarray(forces_at_lambda_k, dtype=np.float64)
    assert f.ndim == 2 and f.shape[1] == 3
    return group_sum(f, groups)


def errors(got, want, bound=None):
    """||got - want|| / max(||want||, 1) over the last axis (3-vectors); with bound (same shape as the norms): ||got - want|| / bound."""
    err = np.linalg.norm(np.asarray(got, dtype=np.float64) - np.asarray(want, dtype=np.float64), axis=-1)
    return err / (np.maximum(np.linalg.norm(want, axis=-1), 1.0) if bound is None else bound)


def rel(got, want):
    e = errors(got, want)
    return float(e.max()) if e.size else 0.0
