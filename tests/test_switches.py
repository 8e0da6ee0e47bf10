"""The engine's SNB_* environment switches: csrc/switches.h is the one place that reads them, and DESIGN.md section 4.5,
tools/switch_matrix.sh and the switches the tests set for their child processes name nothing it does not declare.  No GPU needed."""
import glob
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "openmm-nonbonded-slicing_amd", "csrc")
SWITCHES_H = os.path.join(CSRC, "switches.h")
NAME = re.compile(r"\bSNB_[A-Za-z0-9_]+")

# SNB_* names that are not switches of the engine: what the Python side and the tools read for themselves, the OpenMM adapter's two
# variables (integration/openmm_hip/), the compile-time experiment of direct.hip -- and the constants of the C ABI (include/snb.h)
NOT_ENGINE = {"SNB_LIB_PATH", "SNB_NEIGHBOR_PADDING", "SNB_REBUILD_INTERVAL", "SNB_EXP_NO_JATOMICS"}
NOT_ENGINE_PREFIXES = ("SNB_BENCH_", "SNB_DBG_")


def _read(path):
    with open(path, encoding="utf-8") as f:
        return f.read()


def _declared():
    names = re.findall(r'"(SNB_[A-Z0-9_]+)"', _read(SWITCHES_H))
    assert names, "no switch declared in csrc/switches.h"
    return set(names)


def _abi_constants():
    return set(NAME.findall(_read(os.path.join(ROOT, "include", "snb.h"))))


def _engine_names(text):
    abi = _abi_constants()
    return {n for n in NAME.findall(text) if n not in NOT_ENGINE and not n.startswith(NOT_ENGINE_PREFIXES) and n not in abi}


def test_getenv_is_called_in_switches_h_only():
    sources = sorted(glob.glob(os.path.join(CSRC, "*.hip")) + glob.glob(os.path.join(CSRC, "*.h")))
    assert SWITCHES_H in sources and len(sources) > 3
    callers = [os.path.basename(p) for p in sources if re.search(r"\bgetenv\s*\(", _read(p))]
    assert callers == ["switches.h"], callers


def test_every_switch_is_declared_once():
    names = re.findall(r'^\s*(?:bool|int|long long|double) \w+ = .*?"(SNB_[A-Z0-9_]+)"', _read(SWITCHES_H), flags=re.M)
    assert len(names) == len(set(names)), sorted(n for n in set(names) if names.count(n) > 1)
    assert set(names) == _declared()


def test_design_section_4_5_lists_exactly_the_declared_switches():
    design = _read(os.path.join(ROOT, "DESIGN.md"))
    section = design[design.index("### 4.5 Switches"):design.index("### 4.6 ")]
    rows = re.findall(r"^\| `(SNB_[A-Z0-9_]+)` \|", section, flags=re.M)      # first cell of every table row
    assert len(rows) == len(set(rows)), sorted(n for n in set(rows) if rows.count(n) > 1)
    declared = _declared()
    assert set(rows) == declared, {"only in DESIGN.md": sorted(set(rows) - declared), "only in switches.h": sorted(declared - set(rows))}
    assert "SNB_EXP_NO_JATOMICS" in section and "SNB_EXP_NO_JATOMICS" not in declared      # the compile-time experiment, under its own heading


def test_switch_matrix_names_only_declared_switches():
    tokens = re.findall(r"\b(SNB_[A-Z0-9_]+)=", _read(os.path.join(ROOT, "tools", "switch_matrix.sh")))
    assert len(tokens) > 30
    assert set(tokens) <= _declared(), sorted(set(tokens) - _declared())


def test_tests_set_only_declared_switches():
    # every SNB_* name in the suite that is neither an ABI constant nor on the list above must be a switch: that covers each name a
    # test puts into a child's environment (and the ones it only mentions)
    declared = _declared()
    me = os.path.abspath(__file__)
    seen = set()
    for path in sorted(glob.glob(os.path.join(ROOT, "tests", "*.py"))):
        if os.path.abspath(path) == me:
            continue
        names = _engine_names(_read(path))
        seen |= names
        assert names <= declared, (os.path.basename(path), sorted(names - declared))
    assert {"SNB_VERBOSE", "SNB_OVERLAP", "SNB_SIDE_REBUILD"} <= seen      # (the scan does see the child environments of the GPU tests)
