"""Build-time checks of the energy-only kernels (steps with include_forces == 0, include/snb.h): every one is in the gfx950 code objects
and none uses scratch (read from the ELF notes, as test_host_cpu.py's scratch check does)."""
import re

import pytest

from test_host_cpu import _device_kernel_notes


def test_energy_only_kernels_are_built_without_scratch(snb):
    notes = _device_kernel_notes(snb)
    if notes is None:
        pytest.skip("ROCm binutils not installed")
    families = {
        "packed pair kernel": r"void k_directPackedEnergy<[0-3], (true|false), (true|false)>$",
        "scalar pair kernel": r"void k_directEnergy<(float|double), [0-3], (true|false)>$",
        "pair lists": r"void k_pairListsEnergy<(float|double)>$",
        "plane kernel": r"void k_planeXY<\d+, \d+, 1024, true>$",
        "x pass": r"void k_convolveX<(float|double), \d+, \d+, (256|512), true>$",
    }
    for what, pattern in families.items():
        found = {n: v for n, v in notes.items() if re.match(pattern, n)}
        assert found, what
        scratch = {n: v for n, v in found.items() if v[0] > 0 and not n.startswith("void k_convolveX<double")}
        assert not scratch, (what, scratch)
    # every method of the packed path: RF, Ewald/PME, LJPME, with the polynomial Ewald factor and with the switch
    for inst in ("1, false, false", "1, false, true", "2, true, false", "2, true, true", "3, true, false"):
        assert "void k_directPackedEnergy<%s>" % inst in notes, inst
    # double precision: every method class, with and without per-pair wrapping
    for mc in range(4):
        for wrap in ("true", "false"):
            assert "void k_directEnergy<double, %d, %s>" % (mc, wrap) in notes
