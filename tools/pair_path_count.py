"""(CPU) Static VALU count of a packed pair kernel's tile loop, from the assembly hipcc emits with the Makefile's flags.

Usage: python tools/pair_path_count.py [--asm FILE | --source FILE] [KERNEL ...]
       (default kernels: the benchmark's forces kernel and its derivative kernel)

For every named kernel (the demangled name without `snb::`, e.g. "k_directPacked<2, true, false, false, false>") it prints
  * its registers and scratch as the code object's metadata states them,
  * the VALU instructions (every `v_*` mnemonic, as SQ_INSTS_VALU counts them) of each inner trip: the innermost loops that hold a
    v_rsq_f32, unmasked (two v_cmp per pair step) or masked (four), with the non-DPP v_mov instructions inside them listed one by one,
  * the per-tile part on the unmasked path: the tile loop (the loop around the trips) is walked from its header to its back edge the way
    a wave with no masked tile, no padding slot and a further tile to go runs it -- an `else` region (s_andn2_saveexec) and a region that
    leads only into trips that path does not take (masked ones, and the energy body of a derivative kernel's wanted tiles, which runs
    fewer pair steps per trip) are skipped, every other conditional branch falls through, the trips themselves are left out -- and the
    VALU instructions met are divided by the number of tiles the loop body holds (one per trip taken).
--asm reads an assembly file instead of compiling (e.g. one kept from another commit); --source compiles another copy of direct.hip."""
import argparse
import os
import re
import shlex
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "openmm-nonbonded-slicing_amd", "csrc")
DEFAULT = ["k_directPacked<2, true, false, false, false>", "k_directPackedSelected<2, true, false>"]


def makefile_var(name):
    text = open(os.path.join(CSRC, "Makefile")).read()
    m = re.search(r"^%s \?= (.*)$" % name, text, re.M)
    return m.group(1).strip()


def compile_asm(source, out):
    flags = makefile_var("CXXFLAGS").replace("$(ARCH)", makefile_var("ARCH"))
    cmd = [makefile_var("HIPCC")] + shlex.split(flags) + ["-I", CSRC, "--cuda-device-only", "-S", source, "-o", out]
    subprocess.run(cmd, check=True, stderr=subprocess.DEVNULL)


def demangle(names):
    out = subprocess.run(["c++filt"], input="\n".join(names), capture_output=True, text=True, check=True).stdout.split("\n")
    return [n.replace("snb::", "") for n in out]


def functions(lines):
    """{mangled name: (first line, last line)} of every function body in the file."""
    spans, start, name = {}, None, None
    for i, l in enumerate(lines):
        m = re.match(r"^(_Z\w+):", l)
        if m and start is None:
            name, start = m.group(1), i
        elif l.startswith(".Lfunc_end") and start is not None:
            spans[name] = (start, i); start = None
    return spans


def metadata(text, mangled):
    i = text.index(".name:           " + mangled + "\n")
    seg = text[i:i + 1500]
    g = lambda k: int(re.search(r"\.%s:\s+(\d+)" % k, seg).group(1))
    return g("vgpr_count"), g("sgpr_count"), g("private_segment_fixed_size"), g("vgpr_spill_count")


def mnemonic(line):
    l = line.split(";")[0].strip()
    if not l or l.endswith(":") or l.startswith("."):
        return None
    return l.split()[0]


def is_valu(mn):
    return mn is not None and mn.startswith("v_")


class Loop:
    def __init__(self, label, first, last):
        self.label, self.first, self.last = label, first, last      # header label line .. backward branch line


def loops_of(lines, lo, hi):
    """Natural loops as the printer lays them out: a label and the last backward branch to it."""
    where = {}
    for i in range(lo, hi):
        m = re.match(r"^(\.LBB\d+_\d+):", lines[i])
        if m:
            where[m.group(1)] = i
    found = {}
    for i in range(lo, hi):
        m = re.match(r"\s+s_c?branch\w*\s+(\.LBB\d+_\d+)", lines[i])
        if m and m.group(1) in where and where[m.group(1)] <= i:
            found[m.group(1)] = Loop(m.group(1), where[m.group(1)], i)
    return sorted(found.values(), key=lambda L: L.first), where


def analyse(lines, lo, hi):
    loops, where = loops_of(lines, lo, hi)
    def count(a, b, pred):
        return sum(1 for i in range(a, b + 1) if pred(mnemonic(lines[i])))
    trips = []
    for L in loops:
        inner = [M for M in loops if M is not L and L.first <= M.first and M.last <= L.last]
        if inner or not count(L.first, L.last, lambda m: m == "v_rsq_f32_e32"):
            continue
        rsq = count(L.first, L.last, lambda m: m == "v_rsq_f32_e32")
        cmp_ = count(L.first, L.last, lambda m: m is not None and m.startswith("v_cmp"))
        movs = [lines[i].strip() for i in range(L.first, L.last + 1)
                if (mnemonic(lines[i]) or "").startswith("v_mov") and "dpp" not in lines[i]]
        trips.append(dict(loop=L, valu=count(L.first, L.last, is_valu), steps=rsq // 2, masked=cmp_ > rsq, movs=movs))
    # the tile loop: the smallest loop that holds trips
    outer = [L for L in loops if any(L.first < t["loop"].first and t["loop"].last < L.last for t in trips)]
    tile_loops = [L for L in outer if not any(M is not L and L.first <= M.first and M.last <= L.last for M in outer)]
    per_tile = []
    for T in tile_loops:
        mine = [t for t in trips if T.first < t["loop"].first and t["loop"].last < T.last]
        most = max(t["steps"] for t in mine)
        for t in mine:      # the path's own trips: the forces body, unmasked (a derivative kernel's energy body runs fewer steps per trip)
            t["other"] = t["masked"] or t["steps"] < most
        i, valu, tiles, guard = T.first, 0, 0, 0
        while i <= T.last and guard < 100000:
            guard += 1
            l = lines[i]
            t = next((t for t in mine if t["loop"].first == i), None)
            if t is not None:                       # a trip: left out (unmasked ones count the tiles)
                tiles += 0 if t["other"] else 1
                i = t["loop"].last + 1
                continue
            mn = mnemonic(l)
            if is_valu(mn):
                valu += 1
            m = re.match(r"\s+(s_c?branch\w*)\s+(\.LBB\d+_\d+)", l)
            if m and m.group(2) in where:
                tgt = where[m.group(2)]
                if i == T.last:
                    break
                if m.group(1) == "s_branch" and tgt > i:
                    i = tgt; continue
                between = [t for t in mine if i < t["loop"].first and t["loop"].last < tgt]
                if m.group(1).startswith("s_cbranch") and tgt > i and between and all(t["other"] for t in between):
                    i = tgt; continue      # a region that leads only into trips the path does not take
                if m.group(1).startswith("s_cbranch_exec") and tgt > i:
                    prev = next((mnemonic(lines[k]) for k in range(i - 1, i - 4, -1) if mnemonic(lines[k]) and mnemonic(lines[k]).startswith("s_")
                                 and "saveexec" in mnemonic(lines[k])), "")
                    if prev.startswith("s_andn2_saveexec") and not between:
                        i = tgt; continue
            i += 1
        per_tile.append(dict(loop=T, valu=valu, tiles=tiles))
    return trips, per_tile


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--asm"); ap.add_argument("--source", default=os.path.join(CSRC, "direct.hip")); ap.add_argument("kernels", nargs="*")
    a = ap.parse_args()
    with tempfile.TemporaryDirectory() as tmp:
        path = a.asm
        if path is None:
            path = os.path.join(tmp, "direct.s")
            compile_asm(a.source, path)
        text = open(path).read()
    lines = text.split("\n")
    spans = functions(lines)
    mangled = sorted(spans)
    plain = dict(zip((re.sub(r"^void ", "", d).split("(")[0] for d in demangle(mangled)), mangled))
    status = 0
    for want in a.kernels or DEFAULT:
        key = next((k for k in plain if k.replace(" ", "") == want.replace(" ", "")), None)
        if key is None:
            print("%s: no such kernel in %s" % (want, path)); status = 1; continue
        lo, hi = spans[plain[key]]
        vgpr, sgpr, scratch, spill = metadata(text, plain[key])
        print("%s\n  registers: %d VGPRs (%d allocation units of 8), %d SGPRs; scratch %d bytes per lane, %d spilled VGPRs" % (key, vgpr, (vgpr + 7) // 8, sgpr, scratch, spill))
        trips, per_tile = analyse(lines, lo, hi)
        for t in trips:
            print("  trip %-12s %-8s %d pair steps: %3d VALU, %d non-DPP v_mov" % (t["loop"].label, "masked" if t["masked"] else "unmasked", t["steps"], t["valu"], len(t["movs"])))
            for m in t["movs"]:
                print("      " + re.sub(r"\s+", " ", m))
        for T in per_tile:
            if T["tiles"]:
                print("  tile loop %s: %d VALU outside the trips on the unmasked path of %d tiles = %.1f per tile" % (T["loop"].label, T["valu"], T["tiles"], T["valu"] / T["tiles"]))
    return status


if __name__ == "__main__":
    sys.exit(main())
