"""CPU-only checks of the host side: the interface mirror's error behaviour, and that the C-ABI library loads and
exports every symbol include/snb.h declares (no compute calls: there is no GPU here)."""
import ctypes
import os
import re

import numpy as np
import pytest


def test_header_symbols_exported(snb):
    capi = snb.capi
    capi.build()
    L = capi.lib()
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    header = open(os.path.join(root, "include", "snb.h")).read()
    declared = set(re.findall(r"\b(snb_[a-z0-9_]+)\s*\(", header))
    assert declared == set(capi.SYMBOLS), declared ^ set(capi.SYMBOLS)
    for name in declared:
        assert hasattr(L, name)
    assert L.snb_abi_version() == capi.SNB_ABI_VERSION


def test_struct_layout_matches_header(snb):
    capi = snb.capi
    # sizes follow from the field lists in include/snb.h (natural alignment)
    assert ctypes.sizeof(capi.SnbConfig) == 8 * 4 + 4 * 8 + 6 * 4 + 8 + 3 * 4 + 4 + 8 + 3 * 4 + 2 * 4 + 4 + 8
    assert ctypes.sizeof(capi.SnbStats) == 7 * 8 + 6 * 4 + 4 * 8 + 3 * 8 + 8 + 8 + 8 + 16 * 8 + 16 * 8 + 8 + 8


def test_struct_layout_matches_c_compiler(snb, tmp_path):
    """sizeof/offsetof as gcc sees include/snb.h must equal the ctypes mirror used by the Python binding."""
    import subprocess
    capi = snb.capi
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "snb.h"\nint main(){printf("%zu %zu %zu %zu %zu %zu %zu\\n", sizeof(snb_config), offsetof(snb_config, cutoff), '
                   'offsetof(snb_config, dgrid), offsetof(snb_config, neighbor_padding), offsetof(snb_config, stream), sizeof(snb_stats), offsetof(snb_stats, sum_direct_ms));return 0;}\n')
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-I", os.path.join(root, "include"), str(src), "-o", str(exe)])
    got = [int(x) for x in subprocess.check_output([str(exe)]).split()]
    C, S = capi.SnbConfig, capi.SnbStats
    want = [ctypes.sizeof(C), C.cutoff.offset, C.dgrid.offset, C.neighbor_padding.offset, C.stream.offset, ctypes.sizeof(S), S.sum_direct_ms.offset]
    assert got == want, (got, want)


def test_legal_grid_sizes(snb):
    L = snb.capi.lib()
    # no prime factor above 13: the rule of the reference's GPU platforms (platforms/common/include/FFT3DFactory.h:31-47)
    for n, want in [(80, 80), (116, 117), (118, 120), (173, 175), (87, 88), (89, 90), (121, 121), (5, 6), (97, 98), (1021, 1024), (23, 24), (143, 143)]:
        assert L.snb_legal_grid_size(n) == want


def test_create_without_gpu_fails_loudly(snb):
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    capi = snb.capi
    cfg = capi.SnbConfig(); cfg.abi_version = capi.SNB_ABI_VERSION; cfg.n_atoms = 2; cfg.n_subsets = 1; cfg.method = 0; cfg.precision = 0
    h = ctypes.c_void_p()
    st = capi.lib().snb_create(ctypes.byref(cfg), ctypes.byref(h))
    assert st == capi.SNB_ERR_HIP and not h
    assert b"no HIP device" in capi.lib().snb_last_error(None)
    f = snb.SlicedNonbondedForce(1); f.addParticle(0, 1, 0); f.addParticle(0, 1, 0)
    s = snb.System(); s.addParticle(1); s.addParticle(1); s.addForce(f)
    with pytest.raises(snb.OpenMMException):
        snb.Context(s)


def test_dispersion_coefficients_host_helper_matches_oracle(snb, oracle):
    rng = np.random.default_rng(0)
    n, nsub = 500, 3
    f = snb.SlicedNonbondedForce(nsub)
    f.setNonbondedMethod(2); f.setCutoffDistance(1.1); f.setUseSwitchingFunction(True); f.setSwitchingDistance(0.9)
    for i in range(n):
        f.addParticle(0.0, rng.choice([0.3, 0.31, 0.25]), rng.choice([0.5, 0.7])); f.setParticleSubset(i, int(rng.integers(0, nsub)))
    want = oracle.dispersion_coefficients(f)
    sig = np.array([f.getParticleParameters(i)[1] for i in range(n)]); eps = np.array([f.getParticleParameters(i)[2] for i in range(n)])
    sub = np.array([f.getParticleSubset(i) for i in range(n)], dtype=np.int32)
    out = np.zeros(nsub * (nsub + 1) // 2)
    dp = ctypes.POINTER(ctypes.c_double)
    st = snb.capi.lib().snb_compute_dispersion_coefficients(n, nsub, sig.ctypes.data_as(dp), eps.ctypes.data_as(dp), sub.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)),
                                                           1.1, 1, 0.9, out.ctypes.data_as(dp))
    assert st == 0
    np.testing.assert_allclose(out, want, rtol=1e-12)


def test_scaling_parameter_clash_rules(snb):
    # python/tests/TestSlicedNonbondedForce.py:51-67
    f = snb.SlicedNonbondedForce(2)
    f.addGlobalParameter("lambda", 1.0); f.addGlobalParameter("lambda2", 1.0)
    f.addScalingParameter("lambda", 0, 1, True, True)
    with pytest.raises(snb.OpenMMException):
        f.addScalingParameter("lambda2", 0, 1, True, False)
    with pytest.raises(snb.OpenMMException):
        f.addScalingParameter("lambda2", 1, 0, False, True)
    f.addScalingParameter("lambda2", 1, 1, True, False)
    with pytest.raises(snb.OpenMMException):
        f.addScalingParameter("lambda", 0, 0, False, False)
    with pytest.raises(snb.OpenMMException):
        f.addScalingParameter("nope", 0, 0, True, True)
    with pytest.raises(snb.OpenMMException):
        f.setParticleSubset(0, 0)   # no particles yet: index out of range
    f.addParticle(0, 1, 0)
    with pytest.raises(snb.OpenMMException):
        f.setParticleSubset(0, 2)
    assert f.getNumSlices() == 3 and snb.sliceIndex(1, 0) == 1 and snb.sliceIndex(1, 1) == 2
    f.addEnergyParameterDerivative("lambda")
    with pytest.raises(snb.OpenMMException):
        f.addEnergyParameterDerivative("lambda")
    assert f.getEnergyParameterDerivativeName(0) == "lambda"


def test_calc_pme_parameters_reproduce_the_survey_sizes(snb):
    """calcPMEParameters (context.py; OpenMM's NonbondedForceImpl::calcPMEParameters, third-party, restated) against the values
    SURVEY.md section 8 derives from the published formula for the benchmark boxes: Ewald tolerance 5e-4, cutoff 1.0 nm =>
    alpha = sqrt(-ln 1e-3) = 2.6283 /nm, mesh >= 8.013 L: 96k atoms (L = 9.865) -> 80, 300k (14.42) -> 116 raw -> 120 FFT-legal,
    1M (21.54) -> 173 raw -> 175 legal; LJPME dispersion mesh at half the density: 87 raw -> 90 legal."""
    from importlib import import_module
    ctx = import_module("openmm-nonbonded-slicing_amd.context")
    F = snb.SlicedNonbondedForce
    L_ = snb.capi.lib()
    for L, raw, legal in ((9.865, 80, 80), (14.42, 116, 117), (21.54, 173, 175)):      # (13-smooth rounding: 116 -> 117 = 9 x 13; the bench passes its 120^3 explicitly)
        f = F(1); f.setNonbondedMethod(F.PME); f.setCutoffDistance(1.0); f.setEwaldErrorTolerance(5e-4)
        box = [[L, 0, 0], [0, L, 0], [0, 0, L]]
        a, nx, ny, nz = ctx.calcPMEParameters(f, box, False)
        assert abs(a - 2.6283) < 1e-4 and (nx, ny, nz) == (raw, raw, raw)
        assert L_.snb_legal_grid_size(raw) == legal
    f = F(1); f.setNonbondedMethod(F.LJPME); f.setCutoffDistance(1.0); f.setEwaldErrorTolerance(5e-4)
    a, nx, ny, nz = ctx.calcPMEParameters(f, [[21.54, 0, 0], [0, 21.54, 0], [0, 0, 21.54]], True)
    assert (nx, ny, nz) == (87, 87, 87) and L_.snb_legal_grid_size(87) == 88
    # explicit parameters win over the tolerance
    f.setPMEParameters(3.1, 24, 30, 36)
    assert ctx.calcPMEParameters(f, [[5, 0, 0], [0, 5, 0], [0, 0, 5]], False) == (3.1, 24, 30, 36)


def _device_kernel_notes(snb):
    """{demangled kernel name: (scratch bytes per lane, VGPRs, spilled VGPRs)} of every kernel in the built engine, read from the gfx950 code
    objects inside csrc/*.o (objcopy -> clang-offload-bundler -> llvm-readelf --notes).  None when the ROCm binutils are not installed."""
    import glob
    import re
    import shutil
    import subprocess
    import tempfile
    llvm = "/opt/rocm/lib/llvm/bin"
    tools = [shutil.which("objcopy"), os.path.join(llvm, "clang-offload-bundler"), os.path.join(llvm, "llvm-readelf"), shutil.which("c++filt")]
    if not all(t and os.path.exists(t) for t in tools):
        return None
    snb.capi.build()
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    out = {}
    with tempfile.TemporaryDirectory() as tmp:
        for obj in sorted(glob.glob(os.path.join(root, "openmm-nonbonded-slicing_amd", "csrc", "*.o"))):
            fat, dev = os.path.join(tmp, "fat.bin"), os.path.join(tmp, "dev.o")
            subprocess.run([tools[0], "-O", "binary", "--only-section=.hip_fatbin", obj, fat], check=True)
            if not os.path.exists(fat) or os.path.getsize(fat) == 0:
                continue
            subprocess.run([tools[1], "--unbundle", "--type=o", "--input=" + fat, "--targets=hipv4-amdgcn-amd-amdhsa--gfx950", "--output=" + dev], check=True)
            notes = subprocess.run([tools[2], "--notes", dev], check=True, capture_output=True, text=True).stdout
            names = re.findall(r"^\s+\.name:\s+(\S+)$", notes, re.M)
            scratch = re.findall(r"\.private_segment_fixed_size:\s+(\d+)", notes)
            vgpr = re.findall(r"\.vgpr_count:\s+(\d+)", notes)
            spill = re.findall(r"\.vgpr_spill_count:\s+(\d+)", notes)
            assert len(names) == len(scratch) == len(vgpr) == len(spill), obj
            plain = subprocess.run([tools[3]], input="\n".join(names), capture_output=True, text=True, check=True).stdout.split("\n")
            for n, s, v, sp in zip(plain, scratch, vgpr, spill):
                out[n.replace("snb::", "").split("(")[0]] = (int(s), int(v), int(sp))
    return out


def test_hot_kernels_use_no_scratch(snb):
    """VERDICT r03 item 2 / ADVICE r03: the first build of the plane kernel (commit 4c00133) evaluated the reciprocal-space kernel value inside
    its first inverse pass, sat at the 128-VGPR cap of a 1024-thread work-group with 11 spilled registers (48 B of scratch per lane) and
    faulted on the 54^3 test mesh; the cause could not be separated between a code-generation defect of that instantiation and the
    provisioning of scratch for a spilling 1024-thread work-group (docs/MEASUREMENT_LOG.md, round 4).  Either way the exposure is a
    kernel of the per-step chain that spills.  This test keeps that visible at build time: no kernel of the single-precision step
    (gather, forces-only pair kernel, own-atoms spreader, merge, plane kernel, mix + inverse z, brick interpolation, finish) may use scratch,
    and the kernels that do (energy pair kernel, neighbour builder, double-precision x pass ...) must stay on the list below."""
    notes = _device_kernel_notes(snb)
    if notes is None:
        pytest.skip("ROCm binutils not installed")
    assert len(notes) > 100
    hot = ("k_planeXY<", "k_fftZInvMix<", "k_planeEterm<float", "k_spreadOwn<float", "k_spreadMerge<float", "k_interpolateBricks<float",
           "k_gatherPositions<float", "k_finishForces<float")
    offenders = {n: v for n, v in notes.items() if v[0] > 0 and any(h in n for h in hot) and "k_fftZInvMix<0, 0" not in n}
    assert not offenders, offenders
    # forces-only packed pair kernel of the PME / LJPME methods (template arguments MC = 2 / 3, POLY, ENERGY = false, SWITCH = false, FIXED): the
    # kernel of every plain step of the bench configs (the reaction-field instantiation spills two registers)
    def plain_pme_pair(n):
        m = re.match(r"void k_directPacked<(\d), (true|false), (true|false), (true|false), (true|false)>", n)
        return bool(m) and m.group(1) in "23" and m.group(3) == "false" and m.group(4) == "false"
    pair = {n: v for n, v in notes.items() if plain_pme_pair(n) and v[0] > 0}
    assert sum(plain_pme_pair(n) for n in notes) == 8
    assert not pair, pair
    allowed = ("k_directPacked<", "k_direct<", "k_nbBuildTiles<", "k_convolveX<", "k_spreadMerge<double", "k_spreadBrick<", "k_fftZInvMix<0, 0", "k_fftStrided<double",
               "k_fftZ<double", "k_interpolateBricks<double", "k_interpolate<", "k_pairLists<", "k_ewald", "k_spread<")
    unexpected = {n: v for n, v in notes.items() if v[0] > 0 and not any(a in n for a in allowed)}
    assert not unexpected, unexpected
    # the double-precision tile kernel, with and without the run-time tests of the Ewald polynomials (template argument POLYALL):
    # neither form may spill (the testing instantiations reach 244 of 256 registers)
    tile64 = {n: v for n, v in notes.items() if n.startswith("void k_direct<double")}
    assert len(tile64) == 24, sorted(tile64)
    assert not {n: v for n, v in tile64.items() if v[0] > 0 or v[2] > 0}, tile64
    users = sorted((v[0], n) for n, v in notes.items() if v[0] > 0)
    print("kernels with scratch: %d of %d; largest: %s" % (len(users), len(notes), users[-3:]))
