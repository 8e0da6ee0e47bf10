"""snb_frame_batch / snb_frame_stats (include/snb.h) as gcc lays them out against the ctypes mirrors the Python binding passes, and the
two entry points of frame batches.  Additive: the ABI version stays 7.  No GPU needed."""
import ctypes
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BATCH = ["n_frames", "positions", "is_device", "is_double", "stride4", "boxes", "mode", "include_direct", "include_reciprocal", "slice_energies",
         "out_is_device", "n_states", "state_lambdas", "state_energies"]
STATS = ["n_batches", "n_frames", "n_built_beside", "n_built_in_line", "n_side_discarded", "last_batch_ms"]


def _layout(tmp_path, struct, members):
    fmt = " ".join(["%zu"] * (len(members) + 1))
    args = ", ".join(["sizeof(%s)" % struct] + ["offsetof(%s, %s)" % (struct, m) for m in members])
    src = tmp_path / (struct + ".c")
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "snb.h"\nint main(){printf("%s\\n", %s);return 0;}\n' % (fmt, args))
    exe = tmp_path / struct
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    return [int(x) for x in subprocess.check_output([str(exe)]).split()]


def test_frame_batch_layout_matches_c_compiler(snb, tmp_path):
    B = snb.capi.SnbFrameBatch
    assert [f[0] for f in B._fields_] == BATCH
    assert _layout(tmp_path, "snb_frame_batch", BATCH) == [ctypes.sizeof(B)] + [getattr(B, m).offset for m in BATCH]


def test_frame_stats_layout_matches_c_compiler(snb, tmp_path):
    T = snb.capi.SnbFrameStats
    assert [f[0] for f in T._fields_] == STATS
    assert _layout(tmp_path, "snb_frame_stats", STATS) == [ctypes.sizeof(T)] + [getattr(T, m).offset for m in STATS]


def test_frame_entry_points_are_exported_and_listed(snb):
    capi = snb.capi
    assert {"snb_evaluate_frames", "snb_get_frame_stats"} <= set(capi.SYMBOLS)
    L = ctypes.CDLL(capi.LIB_PATH)
    for name in ("snb_evaluate_frames", "snb_get_frame_stats"):
        assert getattr(L, name) is not None
    L = capi.lib()
    assert L.snb_evaluate_frames(None, None) == capi.SNB_ERR_INVALID_ARGUMENT      # a null batch / handle is refused before anything else
    assert L.snb_get_frame_stats(None, None) == capi.SNB_ERR_INVALID_ARGUMENT


def test_abi_version_is_8(snb):
    assert snb.capi.SNB_ABI_VERSION == 8
    assert snb.capi.lib().snb_abi_version() == 8
    with open(os.path.join(ROOT, "include", "snb.h"), encoding="utf-8") as f:
        assert "#define SNB_ABI_VERSION 8\n" in f.read()
