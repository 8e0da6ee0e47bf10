"""Host side of the packed pair kernels' addressing (no GPU).

1. Register budget, from the built code object's metadata as tests/test_host_cpu.py::test_hot_kernels_use_no_scratch reads it: the
   benchmark's forces kernel k_directPacked<2, true, false, false, FIXED> stays within 14 allocation units of 8 VGPRs (at most 112), its
   derivative kernel k_directPackedSelected<2, true, FIXED> within 15 (at most 120), neither uses scratch, and the instantiations with
   64-bit indices (namespace wide) sit in the same units -- directVgprUnits, which asks for the 32-bit ones, speaks for both, and the
   co-residency arithmetic of the overlapped step (engine.hip) rests on these units.
2. The guard that chooses between them (csrc/pair_addressing.h), compiled with the host compiler into tests/pair_addressing_check.cpp:
   32-bit byte offsets only while every array indexed that way stays below 2^31 bytes."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FORCES_UNITS, SELECTED_UNITS = 14, 15


def _units(vgprs):
    return (vgprs + 7) // 8


def test_register_units_of_the_benchmark_pair_kernels(snb):
    import test_host_cpu
    notes = test_host_cpu._device_kernel_notes(snb)
    if notes is None:
        pytest.skip("ROCm binutils not installed")
    for fixed in ("false", "true"):
        for prefix in ("", "wide::"):
            forces = notes["void %sk_directPacked<2, true, false, false, %s>" % (prefix, fixed)]
            selected = notes["void %sk_directPackedSelected<2, true, %s>" % (prefix, fixed)]
            print("FIXED = %s %s: forces kernel %d VGPRs, derivative kernel %d VGPRs (scratch %d / %d bytes)" % (fixed, prefix or "32-bit", forces[1], selected[1], forces[0], selected[0]))
            assert forces[0] == 0 and forces[2] == 0 and selected[0] == 0 and selected[2] == 0, (forces, selected)
            assert _units(forces[1]) <= FORCES_UNITS, forces
            assert _units(selected[1]) <= SELECTED_UNITS, selected
        for kernel in ("k_directPacked<2, true, false, false, %s>" % fixed, "k_directPackedSelected<2, true, %s>" % fixed):
            assert _units(notes["void " + kernel][1]) == _units(notes["void wide::" + kernel][1]), kernel


@pytest.fixture(scope="module")
def guard(tmp_path_factory):
    exe = tmp_path_factory.mktemp("pair_addressing") / "pair_addressing_check"
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "openmm-nonbonded-slicing_amd", "csrc"),
                           os.path.join(ROOT, "tests", "pair_addressing_check.cpp"), "-o", str(exe)])
    def run(cases):
        text = "".join("%d %d %d %d %d\n" % c for c in cases)
        out = subprocess.run([str(exe)], input=text, capture_output=True, text=True, check=True).stdout.split()
        assert len(out) == len(cases)
        return [int(v) for v in out]
    return run


M24, G2 = 1 << 24, 1 << 31


def test_guard_picks_64_bit_indices_when_an_array_would_pass_2_to_31_bytes(guard):
    # atomSlots, fs, fixed, tile capacity, mask-tile capacity -> 1: 32-bit offsets
    cases = [
        ((96000, 1, 0, 400000, 40000), 1),                 # the benchmark's size, float accumulators
        ((96000, 1, 1, 400000, 40000), 1),                 # ... and fixed point
        ((3008, 4, 1, 5000, 600), 1),                      # an (x, y, z, -) record of 64-bit words per atom
        ((M24 - 32, 16, 1, 1000, 10), 1),                  # (2^24 - 32) x 128 bytes: just below 2^31
        ((M24, 16, 1, 1000, 10), 0),                       # 2^24 x 16 x 8 bytes = 2^31: the force array passes the limit
        ((M24, 8, 1, 1000, 10), 1),                        # 2^30 bytes
        ((M24, 32, 0, 1000, 10), 0),                       # 2^24 x 32 x 4 bytes = 2^31
        ((G2 // 4, 1, 0, 1000, 10), 0),                    # 2^29 float slots = 2^31 bytes
        ((M24 + 32, 1, 0, 1000, 10), 0),                   # beyond the 24-bit multiply that forms the offset
        ((1000, M24 // 4, 0, 1000, 10), 0),                # ... on its other operand
        ((96000, 1, 0, M24, 10), 0),                       # tileJ: 2^24 tiles x 128 bytes = 2^31
        ((96000, 1, 0, M24 - 1, 10), 1),
        ((96000, 1, 0, 1000, M24), 0),                     # masks likewise
        ((96000, 1, 0, 1000, M24 - 1), 1),
        ((96000, 0, 0, 1000, 10), 0),                      # no stride: never the 32-bit form
        ((0, 1, 0, 0, 0), 1),                              # nothing allocated yet (the constructor's query for the register units)
    ]
    got = guard([c for c, _ in cases])
    assert got == [w for _, w in cases], [(c, w, g) for (c, w), g in zip(cases, got) if w != g]
    # whatever the guard lets through stays below 2^31 bytes in every array
    for (atoms, fs, fixed, tiles, masks), g in zip((c for c, _ in cases), got):
        if g:
            assert atoms * fs * (8 if fixed else 4) < G2 and tiles * 128 < G2 and masks * 128 < G2
