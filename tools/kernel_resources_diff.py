#!/usr/bin/env python3
"""
Compare the BUILT gfx950 kernels of two trees, object by object: what a refactor of device code must leave alone.

    python tools/kernel_resources_diff.py PARENT_CSRC BRANCH_CSRC [object names without .o ...]

For every kernel of every named object (default: the families on the complex FP64 MFMA blocks of tbk_zmfma.h) one row:
scratch, LDS, VGPR + AGPR and the waves per SIMD the registers allow (min(8, 512 // (ceil((vgpr + agpr) / 8) * 8))) of
both builds, the count of each FP64 arithmetic instruction (a changed count is the early sign of a changed FMA
contraction), the v_accvgpr moves, and whether the two instruction streams are equal instruction by instruction.
Exit status 1 when a kernel is missing on one side, uses scratch, changes its LDS, loses a wave per SIMD or changes an
FP64 count.  Reads the objects through tools/dpp_hazard_lint.py (kernel_resources, disassemble, parse).
"""

import os
import re
import subprocess
import sys
import tempfile

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import dpp_hazard_lint as lint  # noqa: E402

OBJECTS = ["tbk_green", "tbk_dm", "tbk_chi", "tbk_berry", "tbk_optics", "tbk_surface", "tbk_ensemble", "tbk_channels",
           "tbk_device_green"]
FP64 = ["v_fma_f64", "v_fmac_f64", "v_mul_f64", "v_add_f64", "v_mfma_f64_16x16x4_f64", "v_div_scale_f64", "v_div_fmas_f64",
        "v_div_fixup_f64", "v_rcp_f64"]


def lds_bytes(obj, workdir):
    """{kernel: .group_segment_fixed_size} of the code object's metadata."""
    code = lint.unbundle(obj, workdir)
    text = subprocess.run([os.path.join(lint.LLVM, "llvm-readelf"), "--notes", code], check=True, stdout=subprocess.PIPE,
                          universal_newlines=True).stdout
    out, lds = {}, None
    for line in text.splitlines():
        found = re.match(r"\s*-?\s*\.(name|group_segment_fixed_size):\s*(\S+)", line)
        if not found:
            continue
        if found.group(1) == "group_segment_fixed_size":
            lds = int(found.group(2))
        elif lds is not None:  # the kernel's .name follows its sizes (argument records carry names too, before them)
            out[found.group(2)] = lds
            lds = None
    return out


def waves(res):
    regs = (res["vgpr"] + res["agpr"] + 7) // 8 * 8
    return max(1, min(8, 512 // max(regs, 8)))


def kernels(obj, workdir):
    """{kernel: record} of one object."""
    res = lint.kernel_resources(obj, workdir)
    lds = lds_bytes(obj, workdir)
    out = {}
    for name, instrs, _ in lint.parse(lint.disassemble(obj, workdir)):
        if name not in res:
            continue
        counts = {m: 0 for m in FP64}
        acc = 0
        for mnemonic, _ops in instrs:
            base = mnemonic[:-4] if mnemonic.endswith("_e64") or mnemonic.endswith("_e32") else mnemonic
            if base in counts:
                counts[base] += 1
            acc += mnemonic.startswith("v_accvgpr")
        out[name] = dict(res[name], lds=lds.get(name, -1), waves=waves(res[name]), fp64=counts, acc=acc, stream=instrs)
    return out


def main(argv):
    if len(argv) < 2:
        print(__doc__)
        return 2
    parent, branch, names = argv[0], argv[1], argv[2:] or OBJECTS
    bad = 0
    print("# kernel | scratch | LDS | VGPR+AGPR parent -> branch | waves/SIMD | FP64 counts (%s) | v_accvgpr | stream" % " ".join(
        m.replace("v_", "").replace("_f64", "") for m in FP64))
    with tempfile.TemporaryDirectory() as workdir:
        for obj in names:
            a = kernels(os.path.join(parent, obj + ".o"), workdir)
            b = kernels(os.path.join(branch, obj + ".o"), workdir)
            print("%s.o: %d kernels, %d in the parent" % (obj, len(b), len(a)))
            for name in sorted(set(a) | set(b)):
                if name not in a or name not in b:
                    print("  %s: only in the %s  FAIL" % (name, "parent" if name in a else "branch"))
                    bad += 1
                    continue
                p, q = a[name], b[name]
                why = []
                if q["scratch"] or p["scratch"]:
                    why.append("scratch")
                if p["lds"] != q["lds"]:
                    why.append("LDS")
                if q["waves"] < p["waves"]:
                    why.append("waves")
                if p["fp64"] != q["fp64"]:
                    why.append("FP64 counts")
                bad += bool(why)
                counts = " ".join("%d" % q["fp64"][m] if p["fp64"][m] == q["fp64"][m] else "%d->%d" % (p["fp64"][m], q["fp64"][m])
                                  for m in FP64)
                print("  %s | %d | %d | %d+%d -> %d+%d | %d -> %d | %s | %d -> %d | %s%s" % (
                    name, q["scratch"], q["lds"], p["vgpr"], p["agpr"], q["vgpr"], q["agpr"], p["waves"], q["waves"], counts,
                    p["acc"], q["acc"], "identical" if p["stream"] == q["stream"] else "differs",
                    "  FAIL: " + ", ".join(why) if why else ""))
    print("verdict: %s" % ("%d kernel(s) FAIL" % bad if bad else "every kernel keeps its names, scratch 0, LDS, waves per SIMD and FP64 counts"))
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
