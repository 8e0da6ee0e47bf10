"""The subset-count census on the GPU (-m gpu): 7 to 20 subsets through the reciprocal pipeline, the HIP engine evaluated with
include_direct = 0, include_reciprocal = 1 against the oracle evaluated the same way (tests/subset_census.py; the instrument is proven on the
CPU in tests/test_subset_census.py).  Bars: 1e-3 single / mixed, 1e-5 double.  Forces |dF_i| <= tol max(|F_rec,i|, F_med) on every atom; raw
slice energies |dE| <= tol max(|E|, 1, rho_min sqrt(M_II M_JJ)) (Coulomb, single and mixed; max(|E|, 1) otherwise) on every slice and both
terms, the slices of the empty subset exactly 0.  Every row also takes one full step (direct + reciprocal) at the suite's total-scale rule.
The stamps assert the pipeline a row is there for: the plane path at 7 subsets, the three-pass pipeline -- whose x kernel mixes the spectra
with the lambda matrix -- from 9 on.  The columns per work-group of that kernel (printed; csrc/pme_sizes.h) are 8, 4 or 2 by row and precision,
1 and 2 again in child processes under SNB_CONV_LDS_KB."""
import ctypes
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import recip_systems as R
import shell_systems as S
import subset_census as C

pytestmark = pytest.mark.gpu

_SWITCHED = ("SNB_NO_FUSED_Z", "SNB_NO_OWN_SPREAD", "SNB_OWN_SLABS", "SNB_FFT_TWOPASS", "SNB_NO_PLANE_FFT", "SNB_NO_RECT_PLANES", "SNB_CONV_LDS_KB", "SNB_MIX_16X16")


def _recip_ok(s, f, se, prec, what, failures, mask=None):
    """Forces and / or raw slice energies of a reciprocal-only step against the oracle; mask: the wanted slices of a derivative-only step."""
    fo, eo = R.oracle_eval(s)
    assert (f is None or np.isfinite(f).all()) and (se is None or np.isfinite(se[mask != 0] if mask is not None else se).all()), (what, "NaN")
    if f is not None:
        rec = R.compare(s, f, fo, R.TOLS[prec])
        print("%s %s %s: forces %s" % (s["name"], prec, what, R.report(rec)))
        if not rec["ok"]:
            failures.append("%s, %s: %s" % (what, prec, R.report(rec)))
    if se is not None:
        if mask is not None:          # (the other entries are unspecified after such a step)
            se = np.where(mask[:, None] != 0, se, eo)
        ok, worst, (k, t), dmax = C.compare_energies(s, se, eo, prec)
        print("%s %s %s: slice energies worst %.2e of the bar's scale (slice %s term %d), largest |dE| %.3g kJ/mol" % (s["name"], prec, what, worst, C.slice_pair(k), t, dmax))
        if not ok:
            failures.append("%s, %s: slice energies off by %.2e of the bar's scale at slice %s term %d (engine %r, oracle %r), or a slice of the empty subset is not 0"
                            % (what, prec, worst, C.slice_pair(k), t, se[k, t], eo[k, t]))


def _check_pipeline(row, prec, t, method):
    assert t[1] > 0 and t[4] > 0 and t[7] > 0, t
    if any(k in os.environ for k in _SWITCHED):
        return
    for o in (0, 8) if method == 5 else (0,):
        if row == "n7" and prec != "double":
            assert t[o + 2] > 0 and t[o + 3] == 0 and t[o + 5] == 0, ("own-atoms spreader and plane path", t)
        else:
            assert t[o + 3] > 0 and t[o + 4] > 0 and t[o + 5] > 0, ("three-pass pipeline: the lambda mix runs in the x kernel", t)


@pytest.mark.parametrize("row,prec", C.CASES, ids=["%s-%s" % c for c in C.CASES])
def test_census(row, prec, snb):
    """Reciprocal-only: without a skin an energy + forces step (forces, every raw slice energy, the total against sum lambda E_oracle) and, on
    the same engine, one full step; with a skin of 0.1 nm and a list life of ten steps two forces-only steps and an energy-only step."""
    s = C.build(row)
    tol = R.TOLS[prec]
    rb = 8 if prec == "double" else 4
    failures = []
    eng = R.Engine(snb, s, prec)
    f, se, e = eng.step_energy_forces()
    st = eng.stats()
    pipe, stamps = R.pipeline(st, s["method"])
    print("%s %s: pipeline: %s; stamps %s; x kernel: %s columns per work-group, %d bytes of LDS%s" % (
        row, prec, pipe, stamps, *C.conv_lds(s["grid"][0], s["nsub"], rb), ("; dispersion mesh %s, %d" % C.conv_lds(s["dgrid"][0], s["nsub"], rb)) if s["method"] == 5 else ""))
    _recip_ok(s, f, se, prec, "no skin, energy + forces step", failures)
    _, eo = R.oracle_eval(s)
    scale, _ = C.energy_scale(s, eo, prec)
    assert abs(e - (s["lam"] * eo).sum()) <= tol * (np.abs(s["lam"]) * scale).sum(), (e, (s["lam"] * eo).sum())
    assert tuple(st.grid) == s["grid"] and (s["method"] != 5 or tuple(st.dgrid) == s["dgrid"]), (list(st.grid), list(st.dgrid))
    _check_pipeline(row, prec, stamps, s["method"])
    if row != "n7":
        assert C.conv_lds(s["grid"][0], s["nsub"], rb)[0] == C.EXPECT_NB[row, prec]
    # one full step, on the same engine
    eng.direct = 1
    f, se, e = eng.step_energy_forces()
    ft, et = R.oracle_eval(s, direct=True)
    ok, worst, atom = R.compare_total(s, f, ft, tol)
    eok = bool((np.abs(se - et) <= tol * np.maximum(np.abs(et), scale)).all())
    eworst = float((np.abs(se - et) / np.maximum(np.abs(et), scale)).max())
    print("%s %s full step: forces worst %.2e of max(|F_total|, 1) (atom %d), slice energies %.2e" % (row, prec, worst, atom, eworst))
    if not (ok and eok):
        failures.append("full step, %s: forces %.2e (atom %d), slice energies %.2e" % (prec, worst, atom, eworst))
    st = eng.stats()
    assert st.n_host_rebuilds == 0 and st.n_list_overruns == 0, (int(st.n_host_rebuilds), int(st.n_list_overruns))
    eng.close()
    # skin 0.1, a rebuild every tenth step
    eng = R.Engine(snb, s, prec, padding=0.1, interval=10)
    for k in range(2):
        _recip_ok(s, eng.step_forces(), None, prec, "skin, forces-only step %d" % k, failures)
    _recip_ok(s, None, eng.step_energy_only(), prec, "skin, energy-only step", failures)
    st = eng.stats()
    assert st.n_rebuilds == 1 and st.n_list_overruns == 0 and st.n_host_rebuilds == 0, (int(st.n_rebuilds), int(st.n_list_overruns), int(st.n_host_rebuilds))
    eng.close()
    assert not failures, "\n".join(failures)


@pytest.mark.parametrize("row,prec", [("n13", "single"), ("n20", "double")])
def test_derivative_only_steps_with_a_sparse_mask(row, prec, snb):
    """include_energy == 2 with six wanted slices: the x kernel's flush takes one full group of four and a remainder of two, among them a
    diagonal, a slice of the uncharged subset and one of the empty subset.  Two steps (the second replays); the wanted entries at the bars,
    the forces as on any step."""
    s = C.build(row)
    mask = C.derivative_mask(s)
    failures = []
    eng = R.Engine(snb, s, prec, padding=0.1, interval=10)
    eng.ok(eng.L.snb_set_energy_slices(eng.h, mask.ctypes.data_as(ctypes.POINTER(ctypes.c_int32))))
    for k in range(2):
        eng.ok(eng.L.snb_execute(eng.h, 1, 2, 0, 1, None))
        se = eng.slice_energies()
        assert (se[R.sl(C.empty(s["nsub"]), 2)] == 0).all()
        _recip_ok(s, eng.forces(), se, prec, "derivative-only step %d" % k, failures, mask=mask)
    st = eng.stats()
    assert st.n_host_rebuilds == 0 and st.n_list_overruns == 0
    eng.close()
    assert not failures, "\n".join(failures)


def test_two_ranks_sum_to_the_oracle(snb):
    """`n12`, single precision, as two ranks of six meshes each: a rank's interpolation loops over its meshes with the lambda of (atom's
    subset, mesh's subset) -- no mix in k-space -- and takes the slice energies there too.  The summed forces and raw slice energies against the
    oracle; the slices of the empty subset exactly 0.  Six meshes run the plane path, whose inverse z pass transforms the meshes of two
    subsets as one complex line, so the empty subset's mesh carries the rounding of its partner's (1.7e-4 kJ/mol in a slice when a rank
    summed 1/2 q psi over it): a sharded rank's interpolation skips the meshes of subsets without atoms (PmeParams::emptyGrids)."""
    s = C.build("n12")
    total = np.zeros_like(s["pos"]); etot = 0.0
    for rank in range(2):
        eng = R.Engine(snb, s, "single", padding=0.05, interval=1 << 30, rank=rank, world=2)
        f, se, _ = eng.step_energy_forces()
        total += f; etot = etot + se
        st = eng.stats()
        print("rank %d: pipeline: %s; stamps %s" % ((rank,) + R.pipeline(st, s["method"])))
        assert st.n_host_rebuilds == 0 and st.n_list_overruns == 0
        eng.close()
    failures = []
    print("two ranks: slices of the empty subset, largest |E| %.3g kJ/mol" % max(np.abs(etot[R.sl(C.empty(12), j)]).max() for j in range(12)))
    _recip_ok(s, total, etot, "single", "two ranks", failures)
    assert not failures, "\n".join(failures)


_CHILD = r'''
import sys, json, importlib
sys.path[:0] = [ROOT, ROOT + "/tests", ROOT + "/oracle"]
import numpy as np
import recip_systems as R
import subset_census as C
snb = importlib.import_module("openmm-nonbonded-slicing_amd")
row, prec = sys.argv[1], sys.argv[2]
s = C.build(row)
fo, eo = R.oracle_eval(s)
eng = R.Engine(snb, s, prec, padding=0.1, interval=10)
f, se, _ = eng.step_energy_forces()
st = eng.stats()
out = dict(stamps=[int(x) for x in st.n_kernel_timed], host=int(st.n_host_rebuilds), overruns=int(st.n_list_overruns), steps=[])
for k in range(2):
    rec = R.compare(s, f, fo, R.TOLS[prec])
    out["steps"].append(dict(ok=bool(np.isfinite(f).all()) and rec["ok"], report=R.report(rec)))
    if k == 0:
        f = eng.step_forces()
ok, worst, where, dmax = C.compare_energies(s, se, eo, prec)
out.update(energies_ok=bool(np.isfinite(se).all()) and ok, energies_worst=worst, energies_where=where)
eng.close()
print("RESULT " + json.dumps(out))
'''
CHILDREN = [("n20", "single", {"SNB_CONV_LDS_KB": "16"}, 1), ("n20", "single", {"SNB_CONV_LDS_KB": "32"}, 2), ("n12", "single", {"SNB_MIX_16X16": "1"}, 8),
            ("ortho", "single", {"SNB_MIX_16X16": "1", "SNB_NO_PLANE_FFT": "1"}, 8), ("n20", "single", {}, 4), ("n20", "double", {}, 2)]


@pytest.mark.parametrize("row,prec,env,nb", CHILDREN, ids=["%s-%s-%s" % (r, p, "-".join("%s=%s" % kv for kv in e.items())) for r, p, e, _ in CHILDREN])
def test_switched_forms_of_the_x_kernel(row, prec, env, nb):
    """Reciprocal-only, under switches read once per process (child processes): one and two columns per work-group on `n20` (SNB_CONV_LDS_KB),
    the 16 x 16 x 4 matrix-core mix named by its switch on `n12` (above 4 subsets the switch selects nothing new: the case pins that) and at one
    K chunk on the three subsets of `ortho` taken off the plane path.  An energy + forces step and a forces-only step against the oracle; the
    stamps show the three-pass pipeline.  The columns per work-group are read from the launch itself (its SNB_VERBOSE line), not restated:
    without a switch too, 4 on `n20` single and 2 in double."""
    s = C.build(row)
    assert C.conv_lds(s["grid"][0], s["nsub"], 8 if prec == "double" else 4, int(env.get("SNB_CONV_LDS_KB", C.CONV_LDS_KB)))[0] == nb
    e = {k: v for k, v in os.environ.items() if not k.startswith("SNB_")}
    e["SNB_VERBOSE"] = "1"; e.update(env)
    r = subprocess.run([sys.executable, "-c", "ROOT = %r\n" % S.ROOT + _CHILD, row, prec], env=e, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    res = json.loads([l for l in r.stdout.splitlines() if l.startswith("RESULT ")][-1][7:])
    t = res["stamps"]
    launched = [l for l in r.stderr.splitlines() if l.startswith("[snb] x kernel, coulomb mesh:")]
    print(row, prec, env, t, launched, [x["report"] for x in res["steps"]], res["energies_worst"], res["energies_where"])
    want = "nx %d, %d subsets, %d columns per work-group, %d bytes of LDS" % (s["grid"][0], s["nsub"], nb, C.conv_lds(s["grid"][0], s["nsub"], 8 if prec == "double" else 4, int(env.get("SNB_CONV_LDS_KB", C.CONV_LDS_KB)))[1])
    assert launched and all(l.endswith(want) for l in launched), (launched, want)
    assert all(x["ok"] for x in res["steps"]) and res["energies_ok"], res
    assert t[1] > 0 and t[3] > 0 and t[4] > 0 and t[5] > 0 and t[7] > 0 and res["host"] == 0 and res["overruns"] == 0, t


def _config(snb, n_subsets, method, precision, grid=(0, 0, 0)):
    cfg = snb.capi.SnbConfig()
    cfg.abi_version = snb.capi.SNB_ABI_VERSION; cfg.n_atoms = 64; cfg.n_subsets = n_subsets; cfg.method = method
    cfg.precision = {"single": 0, "double": 1}[precision]; cfg.device = 0; cfg.cutoff = 1.0; cfg.rf_dielectric = 1.0
    cfg.rebuild_interval = 1; cfg.shard_count = 1; cfg.alpha = R.ALPHA; cfg.alpha_d = R.ALPHA
    for d in range(3):
        cfg.grid[d] = grid[d]
    return cfg


def test_an_engine_whose_lds_need_exceeds_the_device_is_refused(snb):
    """Double precision, mesh 180 x 20 x 20, 32 subsets: the x kernel would need 188 640 bytes of LDS at one column per work-group beside 256 static ones.
    snb_create returns SNB_ERR_UNSUPPORTED with the numbers in the message and creates nothing; the same mesh in single precision (94 320
    bytes) is created.  78 subsets (3081 slices, 49 296 bytes in the pair-list energy kernels) are refused with any method, 77 are not."""
    L = snb.capi.lib()
    assert [L.snb_legal_grid_size(n) for n in (180, 20)] == [180, 20]
    UNSUPPORTED = 6
    h = ctypes.c_void_p()
    st = L.snb_create(ctypes.byref(_config(snb, 32, 4, "double", (180, 20, 20))), ctypes.byref(h))
    msg = (L.snb_last_error(None) or b"").decode()
    print(st, msg)
    assert st == UNSUPPORTED and not h.value and all(w in msg for w in ("180", "32", "188896", "double")), (st, msg)
    st = L.snb_create(ctypes.byref(_config(snb, 32, 4, "single", (180, 20, 20))), ctypes.byref(h))
    assert st == 0 and h.value, (st, (L.snb_last_error(None) or b"").decode())
    L.snb_destroy(h)
    h = ctypes.c_void_p()
    st = L.snb_create(ctypes.byref(_config(snb, 78, 2, "single")), ctypes.byref(h))
    msg = (L.snb_last_error(None) or b"").decode()
    print(st, msg)
    assert st == UNSUPPORTED and not h.value and "78" in msg and "3081" in msg and "49296" in msg, (st, msg)
    st = L.snb_create(ctypes.byref(_config(snb, 77, 2, "single")), ctypes.byref(h))
    assert st == 0 and h.value, (st, (L.snb_last_error(None) or b"").decode())
    L.snb_destroy(h)
