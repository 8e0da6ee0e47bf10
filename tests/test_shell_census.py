"""The cutoff-shell census on the CPU: proves the instrument (tests/shell_systems.py) before the GPU is asked.  For every system of the census
the truncation band is empty and every shell pair is worth at least three bars of either of its atoms; removing, doubling or cutting off
known shell pairs in the ORACLE makes the suite's comparison flag exactly the atoms of those pairs, and the report names the pair."""
import numpy as np
import pytest

import shell_systems as S

CASES = sorted(set((g, t) for g, t, _ in S.CENSUS))


@pytest.mark.parametrize("geometry,topology", CASES, ids=["%s-%s" % c for c in CASES])
def test_band_is_empty_and_every_shell_pair_clears_three_bars(geometry, topology):
    s = S.build(geometry, topology)
    assert np.array_equal(s["pos"], S.to_float(s["pos"])), "coordinates must be float32 values"
    ij, r, _ = S.band_pairs(s)
    assert len(ij) == 0, "pairs in the truncation band: %s" % [(int(a), int(b), float(x)) for (a, b), x in zip(ij[:5], r[:5])]
    fo, _ = S.oracle_eval(s)
    sij, sr, sf = S.shell_pairs(s)
    assert len(sij) > 100 and sr.min() >= S.SHELL_LO * s["rc"] * (1 - 1e-12) and sr.max() < s["rc"]
    assert np.allclose(sf, S.K_COULOMB / sr ** 2, rtol=1e-12)          # charges +-1, krf = 0: plain Coulomb
    for prec in ("single", "double"):
        m = S.shell_margins(s, fo, S.TOLS[prec])
        k = int(m.argmin())
        print("%s/%s %s: %d shell pairs, weakest %.2f bars (pair %d-%d, r %.4f), median %.1f" % (geometry, topology, prec, len(m), m[k], sij[k, 0], sij[k, 1], sr[k], np.median(m)))
        assert m[k] >= S.MARGIN, "shell pair (%d, %d) at r = %.5f is worth %.2f bars only: thin the system" % (sij[k, 0], sij[k, 1], sr[k], m[k])


def test_topologies_are_what_they_claim():
    s = S.build("lattice_dense", "long")
    per_atom = np.bincount(s["exc_pairs"].ravel(), minlength=len(s["q"]))
    assert (per_atom >= 40).sum() >= 20, "hub atoms must carry 40 or more exclusions"
    d = np.linalg.norm(S._min_image(s, s["pos"][s["exc_pairs"][:, 1]] - s["pos"][s["exc_pairs"][:, 0]]), axis=1)
    assert ((d >= S.SHELL_LO) & (d < 1.0)).sum() >= 1000 and (d < 0.75).sum() >= 1000 and d.max() < 1.0
    sorted_x = np.argsort(s["pos"][:, 0])          # (any spatial order will do: partners of a hub are spread over far more than one block of 32)
    rank = np.empty(len(sorted_x), dtype=int); rank[sorted_x] = np.arange(len(sorted_x))
    assert (np.abs(rank[s["exc_pairs"][:, 0]] - rank[s["exc_pairs"][:, 1]]) > 32).mean() > 0.9
    for periodic in (True, False):
        s = S.build("lattice_dense", "far14_periodic" if periodic else "far14_plain")
        assert s["exceptions_periodic"] == periodic and (s["exc_qq"] != 0).all()
        plain = s["pos"][s["exc_pairs"][:, 1]] - s["pos"][s["exc_pairs"][:, 0]]
        d = np.linalg.norm(S._min_image(s, plain), axis=1)
        assert d.min() >= 1.0 and d.max() < 1.6
        assert (np.linalg.norm(plain, axis=1) > 3.0).sum() >= 30, "a share of the exceptions must cross a box face"
    s = S.build("unwrapped")
    out = ((s["pos"] < 0) | (s["pos"] >= 6.0)).any(axis=1)
    assert 0.15 < out.mean() < 0.4 and s["pos"].min() > -6.0 and s["pos"].max() < 12.0


def test_shell_pairs_agree_with_a_kd_tree():
    """The pair sets come from the oracle's diagnostic; an independent search (SciPy's periodic KD-tree) must find the same shell."""
    from scipy.spatial import cKDTree
    s = S.build("lattice_dense")
    L = s["box"][0, 0]
    t = cKDTree(np.mod(s["pos"], L), boxsize=L)
    inner = t.query_pairs(S.SHELL_LO * s["rc"], output_type="ndarray")
    outer = t.query_pairs(s["rc"], output_type="ndarray")
    key = lambda p: set((p.min(axis=1).astype(np.int64) * len(s["q"]) + p.max(axis=1)).tolist())
    ij, r, _ = S.shell_pairs(s)
    mine = key(ij)
    theirs = key(outer) - key(inner)
    edge = {k for k in mine ^ theirs}
    assert len(mine) == len(ij)
    # query_pairs includes r == its radius and measures in its own rounding: only pairs within 1e-9 of a shell border may differ
    for k in edge:
        a, b = divmod(k, len(s["q"]))
        d = np.linalg.norm(S._min_image(s, (s["pos"][b] - s["pos"][a])[None])[0])
        assert min(abs(d - S.SHELL_LO), abs(d - 1.0)) < 1e-9, (a, b, d)
    assert len(edge) < 5


def _mutation_pairs(s, fo, count=20, seed=5, plain_image_only=False):
    """`count` seeded shell pairs, the weakest first.  plain_image_only: among the pairs that the two atoms see at the plain difference of
    their coordinates (the only ones an exception can double where exceptions are not periodic)."""
    ij, r, fp = S.shell_pairs(s)
    m = S.shell_margins(s, fo, S.TOLS["single"])
    ok = np.arange(len(ij))
    if plain_image_only:
        d = s["pos"][ij[:, 1]] - s["pos"][ij[:, 0]]
        ok = np.where(np.abs(np.linalg.norm(d, axis=1) - r) < 1e-9)[0]
    weakest = int(ok[m[ok].argmin()])
    rng = np.random.default_rng(seed)
    rest = [int(k) for k in rng.permutation(ok) if k != weakest]
    picks = [weakest] + rest[:count - 1]
    assert len(picks) == min(count, len(ok)) and len(picks) >= 12, len(picks)
    return [(int(ij[k, 0]), int(ij[k, 1]), float(r[k])) for k in picks], (int(ij[m.argmin(), 0]), int(ij[m.argmin(), 1]))


MUTATED = CASES


@pytest.mark.parametrize("geometry,topology", MUTATED, ids=["%s-%s" % c for c in MUTATED])
@pytest.mark.parametrize("mutation", ["removed", "doubled"])
def test_one_wrong_shell_pair_flags_exactly_its_two_atoms(geometry, topology, mutation):
    """Twenty seeded shell pairs, the weakest among them, one at a time, on every system of the census: the oracle evaluates the system with
    the pair removed (a zero exception) or doubled (an exception with chargeProd = 2 q_i q_j: the exception replaces the pair), and the
    comparison at either bar must flag the two atoms of that pair, no other, and name the pair with its distance and image.  A doubled pair:
    the exception is evaluated without cutoff or reaction field, K qq / r^2 -- with krf = 0 the force of the pair itself, twice.  Where
    exceptions are not periodic the exception sees the plain difference of the coordinates, so the doubled pairs are drawn from those the atoms
    see at that image (twenty of them all the same, their weakest included); the system's weakest pair of all is always among the removed."""
    s = S.build(geometry, topology)
    fo, _ = S.oracle_eval(s)
    plain = mutation == "doubled" and not (s["exceptions_periodic"] and s["box"] is not None) and s["box"] is not None
    pairs, weakest = _mutation_pairs(s, fo, plain_image_only=plain)
    if mutation == "removed":
        assert (pairs[0][0], pairs[0][1]) == weakest
    done = 0
    for i, j, r in pairs:
        if plain:
            assert S.pair_image(s, i, j) == (0, 0, 0)
        f, _ = S.oracle_eval(s, extra=[(i, j, 0.0 if mutation == "removed" else 2.0 * s["q"][i] * s["q"][j])])
        for prec in ("single", "double"):
            rec = S.compare(s, f, fo, S.TOLS[prec])
            assert rec["flagged"] == sorted((i, j)), (mutation, i, j, r, S.report(rec))
        w = rec["worst"][0]
        other = j if w["i"] == i else i
        assert w["shell_partners"][0]["j"] == other and w["shell_partners"][0]["flagged"], S.report(rec)
        assert abs(w["shell_partners"][0]["r"] - r) < 1e-12 and w["shell_partners"][0]["image"] == S.pair_image(s, w["i"], other)
        assert abs(w["abs_dF"] - S.K_COULOMB / r ** 2) < 1e-6 * S.K_COULOMB
        assert "pair (%d, %d)" % (w["i"], other) in S.report(rec)
        done += 1
    assert done == len(pairs) and done >= 12, done          # (20 wherever the shell holds as many; the smallest systems have over a hundred)


@pytest.mark.parametrize("geometry,topology", MUTATED, ids=["%s-%s" % c for c in MUTATED])
def test_a_shrunken_cutoff_flags_exactly_the_atoms_of_the_pairs_in_the_gap(geometry, topology):
    """The oracle with its cutoff shrunk by 2e-4 (and by 4e-5: a handful of pairs) against itself: the flagged atoms are the atoms of the
    pairs between the two cutoffs, as the diagnostic lists them -- the CPU rehearsal of the control the GPU suite runs on the engine."""
    s = S.build(geometry, topology)
    fo, _ = S.oracle_eval(s)
    for shrink in (2e-4, 4e-5):
        atoms, gap = S.gap_atoms(s, fo, shrink, S.TOLS["single"], need=1.05, cancelled_below=0.95)
        if shrink == 2e-4 and len(s["q"]) > 1000:
            assert len(gap) > 20
        f, _ = S.oracle_eval(s, cutoff=s["rc"] - shrink)
        rec = S.compare(s, f, fo, S.TOLS["single"])
        assert rec["flagged"] == atoms, (shrink, len(gap), S.report(rec))


def test_trajectories_keep_float_coordinates_and_an_empty_band():
    s = S.build("lattice_dense", "chains")
    frames = S.trajectory(s, 4, 0.004, 21, scales=(1.0, 1.01, 1.01, 0.995))
    assert frames[0]["pos"] is not s["pos"] and np.array_equal(frames[0]["pos"], s["pos"])
    for k, f in enumerate(frames):
        assert np.array_equal(f["pos"], S.to_float(f["pos"])) and len(S.band_pairs(f)[0]) == 0
        assert np.allclose(f["box"], s["box"] * (1.0, 1.01, 1.01, 0.995)[k])
    again = S.trajectory(s, 4, 0.004, 21, scales=(1.0, 1.01, 1.01, 0.995))
    assert all(np.array_equal(a["pos"], b["pos"]) for a, b in zip(frames, again))


@pytest.mark.parametrize("precision", ["single", "double"])
@pytest.mark.parametrize("cell", ["cubic", "triclinic"])
def test_dimer_gas_is_a_gas_of_pairs_with_every_image(precision, cell):
    from scipy.spatial import cKDTree
    box = None if cell == "cubic" else S.TRICLINIC * (40.0 / 6.0)
    d = S.dimer_gas(precision, box)
    n = len(d["q"])
    assert n == 8192 and len(d["partner"]) == 2 * 4096 and (d["inside"] == d["intended_inside"]).all()
    # every requested offset occurs on both sides of the cutoff, and the stored coordinates realise it to well within the offset
    for dl in S.DIMER_DELTAS[precision]:
        for inside in (True, False):
            sel = (d["delta"] == dl) & (d["inside"] == inside)
            assert sel.sum() >= 50
            off = np.abs(d["r"][sel] - S.RC)
            assert (off > 0.25 * dl).all() and (off < 1.75 * dl).all(), (dl, inside, off.min(), off.max())
    # isolation: within rc + padding (0.1) + a margin, an atom sees its partner and, around the corner, excluded atoms only
    b = d["box"]
    imgs = np.array([[i, j, k] for i in (-1, 0, 1) for j in (-1, 0, 1) for k in (-1, 0, 1)], dtype=float) @ b
    allpos = (d["pos"][None] + imgs[:, None]).reshape(-1, 3)
    keep = np.where((np.abs(allpos @ np.linalg.inv(b) - 0.5) < 0.5 + 0.06).all(axis=1))[0]
    tree = cKDTree(allpos[keep])
    excl = set(map(tuple, np.sort(d["exc_pairs"], axis=1).tolist()))
    for i, near in enumerate(tree.query_ball_point(d["pos"], 1.3)):
        for a in set(int(keep[k]) % n for k in near) - {i, int(d["partner"][i])}:
            assert (min(i, a), max(i, a)) in excl, (i, a)
    images = S.dimer_images(d)
    assert len(images - {(0, 0, 0)}) == 26, sorted(images)
    # the closed form is the oracle's answer
    f, _ = S.oracle_eval(d)
    ok, msg = S.compare_dimers(d, f, 1e-12)
    assert ok, msg
    _, so = S.oracle_eval(d)
    assert np.allclose(so, d["expected_slice_energies"], rtol=0, atol=1e-9 * np.abs(d["expected_slice_energies"]).max()), (so, d["expected_slice_energies"])
    print(d["name"], "closed-form slice energies", d["expected_slice_energies"][:, 0])
    # and a lost pair, or one kept beyond the cutoff, is reported with its offset
    f2 = f.copy(); a = int(np.where(d["inside"] & (d["delta"] == S.DIMER_DELTAS[precision][-1]))[0][0]); f2[a] = 0
    ok, msg = S.compare_dimers(d, f2, S.TOLS[precision])
    assert not ok and "delta %.0e inside" % S.DIMER_DELTAS[precision][-1] in msg and "pair (%d, %d)" % (a, d["partner"][a]) in msg
    f3 = f.copy(); a = int(np.where(~d["inside"])[0][0]); f3[a] = [1e-30, 0, 0]
    assert not S.compare_dimers(d, f3, S.TOLS[precision])[0]
