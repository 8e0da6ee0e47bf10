"""snb_context_binding (include/snb.h, ABI 7) as gcc lays it out against the ctypes mirror the Python binding passes.  No GPU needed."""
import ctypes
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MEMBERS = ["posq", "atom_index", "is_double", "padded_n", "force_buffer", "energy_buffer", "deriv_buffer", "deriv_slot", "energy_is_double"]


def test_context_binding_layout_matches_c_compiler(snb, tmp_path):
    capi = snb.capi
    B = capi.SnbContextBinding
    assert [f[0] for f in B._fields_] == MEMBERS
    fmt = " ".join(["%zu"] * (len(MEMBERS) + 1))
    args = ", ".join(["sizeof(snb_context_binding)"] + ["offsetof(snb_context_binding, %s)" % m for m in MEMBERS])
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "snb.h"\nint main(){printf("%s\\n", %s);return 0;}\n' % (fmt, args))
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = [int(x) for x in subprocess.check_output([str(exe)]).split()]
    want = [ctypes.sizeof(B)] + [getattr(B, m).offset for m in MEMBERS]
    assert got == want, (got, want)


def test_binding_entry_points_are_declared(snb):
    capi = snb.capi
    assert capi.SNB_ABI_VERSION == 8
    assert {"snb_bind_context", "snb_context_order_changed"} <= set(capi.SYMBOLS)
    L = capi.lib()
    assert L.snb_bind_context(None, None) == capi.SNB_ERR_INVALID_ARGUMENT      # a null handle is refused before anything else
    assert L.snb_context_order_changed(None) == capi.SNB_ERR_INVALID_ARGUMENT
