"""The mesh-size census: a table of PME meshes that between them reach every (R1, R2) instantiation of the reciprocal path's six kernel
families (csrc/pme_plan.h: the macro lists of FFT pairs, plane pairs and plane radices), on one set of atoms (tests/test_mesh_census.py on the CPU,
tests/test_gpu_mesh_census.py on the GPU).  It sits on tests/recip_systems.py: same oracle, same comparison, same bars.

The atoms are the lattice of `ortho` (13 608 atoms in 5.6 x 6.4 x 7.2 nm, alpha 2.6283) in 2 or in 5 slabs along y.  The mesh of a row does not
follow the cell's proportions: engine and oracle share it, so a coarse or a fine axis only moves the error both have in common.

Where a row's splits come from.  The table does not compute splitTwoPass / splitPlane (csrc/pme_plan.h): every row STATES the splits it is there for,
in the words of the engine's own SNB_VERBOSE mesh line (engine.hip describeMesh: "fft splits x a*b y a*b z a*b, plane splits x a*b y a*b
(static | run-time | none)"), and the GPU leg asserts that the engine printed exactly that for the row.  The CPU leg reduces the stated splits
to kernel keys and holds them against the kernel names in the built gfx950 code objects, and runs the engine's planner itself
(tests/pme_plan_check.cpp) against the stated splits.

What the splits do not settle -- which pipeline a mesh gets, whether the merge kernel fuses the z pass, the thread counts -- follows from sizes
and LDS budgets; plan() below repeats that arithmetic (host_lists.h sortColumns; csrc/pme_plan.h brickGeometry, ownSpreadMargin,
ownSpread, planePath, zMix, convxThreads).  The CPU leg holds it against the planner field by field; the GPU leg checks the part of it
that shows: the sort columns, the planned spreader and its slabs from the mesh line, the pipeline from the stamp slots.

Kernel keys: (family, Real where the family has one, R1, R2, energy-only flag where the family has one); 0, 0 are the staged / run-time forms.
Thread-count variants are kept beside them as (family, Real or None, threads), and ("k_fftZInvMix", R1, R2, 512) per z pair."""
import re

import numpy as np

import recip_systems as R
import shell_systems as S

PADDING, INTERVAL = 0.02, 10          # the skin of every census engine: lists live ten steps, the spreader's margin stays one cell on every mesh here
N_ATOMS = S.ORTHO_SITES[0] * S.ORTHO_SITES[1] * S.ORTHO_SITES[2]
NO_PLANE = {"SNB_NO_PLANE_FFT": "1"}


def _row(name, grid, nsub, fft, plane, path, env=None):
    """path: the pipeline of the single-precision mesh, "plane" or "three-pass" (double precision always takes the three-pass pipeline)."""
    return dict(name=name, grid=tuple(grid), nsub=nsub, fft=fft, plane=plane, path=path, env=dict(env or {}))


# ---- the table ------------------------------------------------------------------------------------------------------------------------
# S rows: the ten square planes of the plane-pair list -- k_planeXY<A, B, 1024> and its energy-only twin -- with five subsets.  The bricks of a fine
#   plane leave room for a short z line only (a brick of doubles within 60 KB, host_lists.h sortColumns): 96, 120 and 128 get z lines outside
#   the pair list, which are the staged <0, 0> forms of k_spreadMerge and k_fftZInvMix.
# P rows: rectangular planes for the run-time kernel k_planeXY<0, 0>.  Their x sizes are 5*5, 5*6, 16*16, 15*16, 12*15, 6*7, 10*12, 7*8, 8*9, 9*10
#   and their y sizes 16*16, 15*16, 5*6, 5*8, 6*7, 12*15, 7*8, 10*12, 9*10, 8*9: every radix of the plane-radix list first and second on x and on
#   y, except 5 second on y (UNREACHED_ROLES).  The Z rows add further splits.
# Z rows: the z pairs the S and P rows cannot hold.  A z line of 108 .. 256 points fuses its forward pass into the merge kernel only over
#   columns of 25 .. 42 cells (pme_plan.h ownSpread: 120 KB of LDS; double precision at nz = 256: 5 x 5 cells, 116 KB), so these planes are small.
#   S, P and Z rows together hold every z pair with five subsets: k_spreadMerge fused in both precisions, k_fftZInvMix<A, B, 512>.
# L rows: every pair size once on x, once on y, once on z on the three-pass pipeline: k_convolveX (x), k_fftStrided (y), k_fftZ (z) in double
#   precision, and in single precision under SNB_NO_PLANE_FFT=1 (below 129 points nothing else takes the single-precision mesh off the plane
#   path).  Large sizes sit beside small ones: 1 .. 3.5 million points.
# F70: sizes outside every list on all three axes (44 = 4 * 11 has no plane split: three-pass without a switch): the staged <0, 0> forms of
#   k_convolveX, k_fftStrided and k_fftZ.  T768: k_planeXY<A, B, 768>.  U25: see UNREACHED_ROLES.
# Every case runs in a child process with the row's environment and SNB_VERBOSE=1 (the switches are read once per process).
ROWS = [
    _row('S42', (42, 42, 100), 5, 'x 6*7 y 6*7 z 10*10', 'x 6*7 y 6*7 (static)', 'plane'),
    _row('S54', (54, 54, 128), 5, 'x 6*9 y 6*9 z 8*16', 'x 6*9 y 6*9 (static)', 'plane'),
    _row('S64', (64, 64, 96), 5, 'x 8*8 y 8*8 z 8*12', 'x 8*8 y 8*8 (static)', 'plane'),
    _row('S80', (80, 80, 64), 5, 'x 8*10 y 8*10 z 8*8', 'x 8*10 y 8*10 (static)', 'plane'),
    _row('S90', (90, 90, 42), 5, 'x 9*10 y 9*10 z 6*7', 'x 9*10 y 9*10 (static)', 'plane'),
    _row('S96', (96, 96, 40), 5, 'x 8*12 y 8*12 z 0*0', 'x 8*12 y 8*12 (static)', 'plane'),
    _row('S100', (100, 100, 54), 5, 'x 10*10 y 10*10 z 6*9', 'x 10*10 y 10*10 (static)', 'plane'),
    _row('S108', (108, 108, 42), 5, 'x 9*12 y 9*12 z 6*7', 'x 9*12 y 9*12 (static)', 'plane'),
    _row('S120', (120, 120, 32), 5, 'x 10*12 y 10*12 z 0*0', 'x 10*12 y 10*12 (static)', 'plane'),
    _row('S128', (128, 128, 30), 5, 'x 8*16 y 8*16 z 0*0', 'x 8*16 y 8*16 (static)', 'plane'),
    _row('P1', (25, 256, 90), 5, 'x 0*0 y 16*16 z 9*10', 'x 5*5 y 16*16 (run-time)', 'plane'),
    _row('P2', (30, 240, 80), 2, 'x 0*0 y 15*16 z 8*10', 'x 5*6 y 15*16 (run-time)', 'plane'),
    _row('P3', (256, 30, 90), 5, 'x 16*16 y 0*0 z 9*10', 'x 16*16 y 5*6 (run-time)', 'plane'),
    _row('P4', (240, 40, 80), 2, 'x 15*16 y 0*0 z 8*10', 'x 15*16 y 5*8 (run-time)', 'plane'),
    _row('P5', (180, 42, 80), 5, 'x 12*15 y 6*7 z 8*10', 'x 12*15 y 6*7 (run-time)', 'plane'),
    _row('P6', (42, 180, 64), 2, 'x 6*7 y 12*15 z 8*8', 'x 6*7 y 12*15 (run-time)', 'plane'),
    _row('P7', (120, 56, 64), 5, 'x 10*12 y 0*0 z 8*8', 'x 10*12 y 7*8 (run-time)', 'plane'),
    _row('P8', (56, 120, 54), 2, 'x 0*0 y 10*12 z 6*9', 'x 7*8 y 10*12 (run-time)', 'plane'),
    _row('P9', (72, 90, 54), 5, 'x 0*0 y 9*10 z 6*9', 'x 8*9 y 9*10 (run-time)', 'plane'),
    _row('P10', (90, 72, 54), 2, 'x 9*10 y 0*0 z 6*9', 'x 9*10 y 8*9 (run-time)', 'plane'),
    _row('Z256', (25, 30, 256), 5, 'x 0*0 y 0*0 z 16*16', 'x 5*5 y 5*6 (run-time)', 'plane'),
    _row('Z240', (35, 40, 240), 5, 'x 0*0 y 0*0 z 15*16', 'x 5*7 y 5*8 (run-time)', 'plane'),
    _row('Z192', (45, 50, 192), 5, 'x 0*0 y 0*0 z 12*16', 'x 5*9 y 5*10 (run-time)', 'plane'),
    _row('Z180', (36, 42, 180), 5, 'x 0*0 y 6*7 z 12*15', 'x 6*6 y 6*7 (run-time)', 'plane'),
    _row('Z160', (42, 56, 160), 5, 'x 6*7 y 0*0 z 10*16', 'x 6*7 y 7*8 (run-time)', 'plane'),
    _row('Z144', (49, 36, 144), 5, 'x 0*0 y 0*0 z 12*12', 'x 7*7 y 6*6 (run-time)', 'plane'),
    _row('Z120', (40, 30, 120), 5, 'x 0*0 y 0*0 z 10*12', 'x 5*8 y 5*6 (run-time)', 'plane'),
    _row('Z108', (35, 30, 108), 5, 'x 0*0 y 0*0 z 9*12', 'x 5*7 y 5*6 (run-time)', 'plane'),
    _row('L42', (42, 256, 100), 2, 'x 6*7 y 16*16 z 10*10', 'x 6*7 y 16*16 (run-time)', 'three-pass', env={'SNB_NO_PLANE_FFT': '1'}),
    _row('L54', (54, 240, 108), 2, 'x 6*9 y 15*16 z 9*12', 'x 6*9 y 15*16 (run-time)', 'three-pass', env={'SNB_NO_PLANE_FFT': '1'}),
    _row('L64', (64, 192, 120), 2, 'x 8*8 y 12*16 z 10*12', 'x 8*8 y 12*16 (run-time)', 'three-pass', env={'SNB_NO_PLANE_FFT': '1'}),
    _row('L80', (80, 180, 128), 2, 'x 8*10 y 12*15 z 8*16', 'x 8*10 y 12*15 (run-time)', 'three-pass', env={'SNB_NO_PLANE_FFT': '1'}),
    _row('L90', (90, 160, 96), 2, 'x 9*10 y 10*16 z 8*12', 'x 9*10 y 10*16 (run-time)', 'three-pass', env={'SNB_NO_PLANE_FFT': '1'}),
    _row('L96', (96, 144, 90), 2, 'x 8*12 y 12*12 z 9*10', 'x 8*12 y 12*12 (run-time)', 'three-pass', env={'SNB_NO_PLANE_FFT': '1'}),
    _row('L100', (100, 128, 80), 2, 'x 10*10 y 8*16 z 8*10', 'x 10*10 y 8*16 (run-time)', 'three-pass', env={'SNB_NO_PLANE_FFT': '1'}),
    _row('L108', (108, 120, 64), 2, 'x 9*12 y 10*12 z 8*8', 'x 9*12 y 10*12 (run-time)', 'three-pass', env={'SNB_NO_PLANE_FFT': '1'}),
    _row('L120', (120, 108, 54), 2, 'x 10*12 y 9*12 z 6*9', 'x 10*12 y 9*12 (run-time)', 'three-pass', env={'SNB_NO_PLANE_FFT': '1'}),
    _row('L128', (128, 100, 42), 2, 'x 8*16 y 10*10 z 6*7', 'x 8*16 y 10*10 (run-time)', 'three-pass', env={'SNB_NO_PLANE_FFT': '1'}),
    _row('L144', (144, 96, 256), 2, 'x 12*12 y 8*12 z 16*16', 'x 12*12 y 8*12 (run-time)', 'three-pass', env={'SNB_NO_PLANE_FFT': '1'}),
    _row('L160', (160, 90, 240), 2, 'x 10*16 y 9*10 z 15*16', 'x 10*16 y 9*10 (run-time)', 'three-pass', env={'SNB_NO_PLANE_FFT': '1'}),
    _row('L180', (180, 80, 192), 2, 'x 12*15 y 8*10 z 12*16', 'x 12*15 y 8*10 (run-time)', 'three-pass', env={'SNB_NO_PLANE_FFT': '1'}),
    _row('L192', (192, 64, 180), 2, 'x 12*16 y 8*8 z 12*15', 'x 12*16 y 8*8 (run-time)', 'three-pass', env={'SNB_NO_PLANE_FFT': '1'}),
    _row('L240', (240, 54, 160), 2, 'x 15*16 y 6*9 z 10*16', 'x 15*16 y 6*9 (run-time)', 'three-pass', env={'SNB_NO_PLANE_FFT': '1'}),
    _row('L256', (256, 42, 144), 2, 'x 16*16 y 6*7 z 12*12', 'x 16*16 y 6*7 (run-time)', 'three-pass', env={'SNB_NO_PLANE_FFT': '1'}),
    _row('F70', (70, 44, 132), 2, 'x 0*0 y 0*0 z 0*0', 'x 7*10 y 0*0 (none)', 'three-pass'),
    _row('U25', (30, 25, 48), 2, 'x 0*0 y 0*0 z 0*0', 'x 5*6 y 5*5 (run-time)', 'three-pass'),
    _row('T768', (64, 64, 48), 2, 'x 8*8 y 8*8 z 0*0', 'x 8*8 y 8*8 (static)', 'plane', env={'SNB_PLANE_NT': '768'}),
]

# the sixteen line lengths of the FFT-pair list: the x sizes of the L rows (tests/test_mesh_census.py holds them against the build)
SIZES = tuple(sorted(r["grid"][0] for r in ROWS if r["name"].startswith("L")))

# Instantiations (keys as above) no constructible mesh reaches, with the condition that declines them: {key: (file, function, condition)}.
# Empty: every instantiation of the six families has a row.
UNREACHED = {
}

# Roles of the run-time plane kernel that no mesh can give it: {role: (file, function, condition, the row that shows the fallback)}
UNREACHED_ROLES = {
    "radix 5 as second factor on y": ("pme_plan.h", "planePath", "5 is second only in 25 = 5 * 5 (splitPlane orders r1 <= r2), and an odd ny is declined: (d.ny & 1)", "U25"),
}


def by_name(name, rows=None):
    return next(r for r in (ROWS if rows is None else rows) if r["name"] == name)


# ---- the system of a row ----------------------------------------------------------------------------------------------------------------
def system(row):
    """`ortho`'s lattice and particles under the row's mesh, in row["nsub"] slabs along y."""
    rng = np.random.default_rng(201)
    pos = S.lattice_sites(S.ORTHO_SITES, S.ORTHO_LENGTHS, rng)
    nsub = row["nsub"]
    return R.make("census_%s" % row["name"], pos, np.diag(S.ORTHO_LENGTHS), 4, nsub, R._slabs(pos, 1, S.ORTHO_LENGTHS[1], nsub), rng, row["grid"], chains=False)


# ---- the stated splits ------------------------------------------------------------------------------------------------------------------
def splits(row):
    """((rx1, rx2), (ry1, ry2), (rz1, rz2)), ((px1, px2), (py1, py2)), kind -- parsed from the row's own words."""
    f = re.fullmatch(r"x (\d+)\*(\d+) y (\d+)\*(\d+) z (\d+)\*(\d+)", row["fft"])
    p = re.fullmatch(r"x (\d+)\*(\d+) y (\d+)\*(\d+) \((static|run-time|none)\)", row["plane"])
    assert f and p, row
    f = [int(v) for v in f.groups()]
    q = [int(v) for v in p.groups()[:4]]
    return ((f[0], f[1]), (f[2], f[3]), (f[4], f[5])), ((q[0], q[1]), (q[2], q[3])), p.group(5)


def mesh_line_tail(row):
    """What the engine's SNB_VERBOSE mesh line must end with for this row."""
    return "; fft splits %s, plane splits %s" % (row["fft"], row["plane"])


# ---- the planner's arithmetic ---------------------------------------------------------------------------------------------------------
def _own_line_stride(rz, fixed):
    per = 4 if fixed else 2
    st = (rz + per - 1) // per * per
    while ((st * (1 if fixed else 2)) & 7) != 4:
        st += per
    return st


def plan(row, prec):
    """What the engine does with the row's mesh in one precision, from the sizes and LDS budgets alone (the splits are the row's)."""
    nx, ny, nz = row["grid"]
    nsub, env = row["nsub"], row["env"]
    fft, pl, kind = splits(row)
    flt = prec != "double"
    real = 4 if flt else 8
    out = dict(real="float" if flt else "double")
    # host_lists.h sortColumns: whole mesh cells, 5 .. 16 wide, nearest the mean block edge, a brick of doubles within 60 KB
    L = S.ORTHO_LENGTHS
    a = np.cbrt(32.0 * L[0] * L[1] * L[2] / N_ATOMS)

    def pick(m, length):
        best, err = 0, 1e300
        for d in range(5, min(16, m) + 1):
            if m % d == 0 and abs(d * length / m - a) < err:
                best, err = d, abs(d * length / m - a)
        return best
    px, py = pick(nx, L[0]), pick(ny, L[1])
    bricks = px > 0 and py > 0 and 8 * px * py * nz <= 60 * 1024
    out.update(cells=(px, py) if bricks else (0, 0), bricks=bricks)
    # pme_plan.h ownSpreadMargin, ownSpread: margin 1 at this skin; slabs: the fewest whose region fits 40 KB (then 64 KB), more up to ~400 work-groups
    margin = max(1, int(np.ceil(0.5 * PADDING * max(nx / L[0], ny / L[1]) + 0.01)))
    assert margin == 1, row
    fixed = flt and "SNB_NO_FIXED_SPREAD" not in env
    acc = 4 if fixed else 8
    slabs = 0
    if bricks and px + 6 <= nx and py + 6 <= ny and nz <= 256:
        for budget in (40, 64):
            for k in range(2, 33):
                sz = nz // k
                if nz % k or sz < 4 or sz & 1:
                    continue
                if acc * (px + 6) * (py + 6) * (sz + 4) <= budget * 1024:
                    slabs = k
                    break
            if slabs:
                break
        if slabs:
            for k in range(slabs + 1, 17):
                if (nx // px) * (ny // py) * slabs >= 400:
                    break
                if nz % k == 0 and nz // k >= 8 and not (nz // k) & 1:
                    slabs = k
    # ... what can still decline it at the launch, the merge kernel's threads, the fused z pass
    own = slabs >= 2
    if own:
        sz = nz // slabs
        own = acc * (px + 6) * (py + 6) * _own_line_stride(sz + 4, fixed) <= 64 * 1024 and nsub * (nx // px) * (ny // py) * slabs * (px + 6) * (py + 6) * (sz + 4) < 2 ** 31
        cmax = 4 if fixed else 2
        chunk = cmax if sz % cmax == 0 else (2 if fixed and sz % 2 == 0 else 1)
        out["merge_nt"] = 512 if px * py * (nz // chunk) > 6 * 256 else 256
    nb = (px * py + 1) // 2
    fuse = own and "SNB_NO_FUSED_Z" not in env and 2 * real * (2 * nz * (nb + 1) + nz) <= 120 * 1024
    out.update(own=own, slabs=slabs if own else 0, fuse=fuse)
    # pme_plan.h planePath (ok, buffers), zMix, convxThreads
    static = kind == "static"
    plane_lds = 8 * (nx * (ny | 1) + nx + (0 if static else ny))
    plane = (flt and fuse and "SNB_NO_PLANE_FFT" not in env and kind != "none" and ny % 2 == 0 and nsub <= 8 and plane_lds <= 156 * 1024
             and nx * (ny | 1) * 8 <= 156 * 1024)
    out["path"] = "plane" if plane else "three-pass"
    out["zmix_nt"] = 512 if 8 * ((nsub + 1) // 2) >= 24 and fft[2][0] else 256      # (the staged <0, 0> form exists at 256 threads only)
    out["convx_nt"] = 256 if (not flt and max(fft[0]) > 12) else 512
    out["plane_nt"] = int(env.get("SNB_PLANE_NT", 1024))
    return out


def keys(row, prec):
    """(kernel keys, thread-count variants) the row reaches in one precision: an energy + forces step, forces-only steps, an energy-only step."""
    fft, pl, kind = splits(row)
    p = plan(row, prec)
    real = p["real"]
    k, v = set(), set()
    if p["fuse"]:
        k.add(("k_spreadMerge", real) + fft[2])
        v.add(("k_spreadMerge", real, p["merge_nt"]))
    if p["path"] == "plane":
        ab = pl[0] if kind == "static" else (0, 0)
        k.add(("k_planeXY",) + ab + (False,)); k.add(("k_planeXY",) + ab + (True,))
        v.add(("k_planeXY", None, p["plane_nt"] if kind == "static" else 1024))
        k.add(("k_fftZInvMix",) + fft[2])
        v.add(("k_fftZInvMix", None, p["zmix_nt"]))
        if p["zmix_nt"] == 512 and fft[2][0]:
            v.add(("k_fftZInvMix",) + fft[2] + (512,))
    else:
        k.add(("k_fftZ", real) + fft[2])
        k.add(("k_fftStrided", real) + fft[1])
        k.add(("k_convolveX", real) + fft[0] + (False,)); k.add(("k_convolveX", real) + fft[0] + (True,))
        v.add(("k_convolveX", real, p["convx_nt"]))
    return k, v


def table_keys(rows, precisions=("single", "double")):
    k, v = set(), set()
    for row in rows:
        for prec in precisions:
            a, b = keys(row, prec)
            k |= a; v |= b
    return k, v


# ---- the kernels of the build ---------------------------------------------------------------------------------------------------------
_FAMILIES = (
    (r"void k_spreadMerge<(float|double), (?:true|false), true, (\d+), (\d+), (\d+)>$", lambda m: (("k_spreadMerge", m[1], int(m[2]), int(m[3])), ("k_spreadMerge", m[1], int(m[4])))),
    (r"void k_fftZInvMix<(\d+), (\d+), (\d+)>$", lambda m: (("k_fftZInvMix", int(m[1]), int(m[2])), ("k_fftZInvMix", None, int(m[3])))),
    (r"void k_fftZ<(float|double), (?:true|false), (\d+), (\d+)>$", lambda m: (("k_fftZ", m[1], int(m[2]), int(m[3])), None)),
    (r"void k_fftStrided<(float|double), (\d+), (\d+)>$", lambda m: (("k_fftStrided", m[1], int(m[2]), int(m[3])), None)),
    (r"void k_convolveX<(float|double), (\d+), (\d+), (\d+), (true|false)>$", lambda m: (("k_convolveX", m[1], int(m[2]), int(m[3]), m[5] == "true"), ("k_convolveX", m[1], int(m[4])))),
    (r"void k_planeXY<(\d+), (\d+), (\d+), (true|false)>$", lambda m: (("k_planeXY", int(m[1]), int(m[2]), m[4] == "true"), ("k_planeXY", None, int(m[3])))),
)


def library_keys(names):
    """(kernel keys, thread-count variants) of the six families among the demangled kernel names of the build."""
    k, v = set(), set()
    for n in names:
        for pattern, reduce in _FAMILIES:
            m = re.match(pattern, n)
            if m:
                key, var = reduce(m)
                k.add(key)
                if var:
                    v.add(var)
                if key[0] == "k_fftZInvMix" and key[1] and var[2] == 512:
                    v.add(key + (512,))
    return k, v


def completeness(rows, unreached, lib_keys):
    """(missing, stale, overlap): library keys neither reached nor listed as unreached; keys named by the tables that the library lacks;
    keys in both tables."""
    reached, _ = table_keys(rows)
    listed = set(unreached)
    return lib_keys - reached - listed, (reached | listed) - lib_keys, reached & listed
