#!/usr/bin/env python3
"""Static instruction census of one kernel of a translation unit of csrc/ (--unit, default render), whole body and main loop.

Builds ray-tracing-cuda_amd/csrc/<unit>.hip to gfx950 assembly with the Makefile's flags (no GPU needed) -- or reads
an assembly file made that way (--asm) -- and prints, for every kernel whose symbol holds --kernel:

  * the code object's metadata: VGPRs, SGPRs, spilled VGPR dwords / SGPRs, scratch bytes, static LDS, occupancy;
  * instruction counts by class for the whole kernel and for its MAIN LOOP: the backward branch with the longest span
    inside the kernel (render_body.h's `for (;;)`: everything from the loop header's label to that back edge).

These are STATIC counts -- instructions in the text, not instructions executed: a branch not taken, or a loop inside the
main loop, counts once.  They say what the compiler emitted for a mode, not what a query costs.

  tools/loop_census.py --kernel 'render_kernelILj2ELj0E' [--unit render] [--asm render.s] [--label before] [--json out.json]

--json merges the result into the file under --label (profiles/list_fast_census.json keeps before and after).
"""
import argparse
import json
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "ray-tracing-cuda_amd", "csrc")
CLASSES = ("valu", "lane_moves", "salu", "scalar_branches", "smem", "lds", "vmem", "spill_accesses", "waits", "other")


def makefile_flags():
    """FLAGS of csrc/Makefile, $(ARCH) resolved to gfx950."""
    for line in open(os.path.join(CSRC, "Makefile")):
        m = re.match(r"FLAGS\s*:=\s*(.*)", line)
        if m:
            return m.group(1).replace("$(ARCH)", "gfx950").split()
    raise SystemExit("no FLAGS in csrc/Makefile")


def build_asm(unit, out, extra):
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    cmd = [hipcc] + makefile_flags() + extra + ["--cuda-device-only", "-S", unit + ".hip", "-o", out]
    subprocess.run(cmd, cwd=CSRC, check=True, stderr=subprocess.DEVNULL)


def classify(op):
    if op.startswith(("v_readlane", "v_writelane", "v_readfirstlane")):
        return "lane_moves" if not op.startswith("v_readfirstlane") else "valu"
    if op.startswith("v_"):
        return "valu"
    if op.startswith("s_cbranch"):
        return "scalar_branches"
    if op.startswith(("s_load", "s_buffer_load", "s_memtime", "s_memrealtime")):
        return "smem"
    if op.startswith(("s_waitcnt", "s_nop", "s_sleep", "s_barrier", "s_endpgm", "s_setprio", "s_branch", "s_code_end")):
        return "waits" if op.startswith("s_waitcnt") else "other"
    if op.startswith("s_"):
        return "salu"
    if op.startswith("ds_"):
        return "lds"
    if op.startswith("scratch_"):
        return "spill_accesses"
    if op.startswith(("global_", "flat_", "buffer_")):
        return "vmem"
    return "other"


def count(lines):
    c = dict.fromkeys(CLASSES, 0)
    for op, _ in lines:
        c[classify(op)] += 1
    c["instructions"] = len(lines)
    return c


def kernel_bodies(asm_text):
    """{symbol: [(line number, text)]} for every .globl function of type @function."""
    lines = asm_text.split("\n")
    out, cur, name = {}, None, None
    for i, ln in enumerate(lines):
        m = re.match(r"^(_Z\w+):", ln)
        if m and cur is None:
            name, cur = m.group(1), []
            continue
        if cur is not None:
            if ln.startswith(".Lfunc_end"):
                out[name] = cur
                cur = None
            else:
                cur.append(ln)
    return out


def census(body):
    """body: the kernel's text lines.  Returns (whole, loop, (header label, span in instructions))."""
    ins, labels = [], {}
    for ln in body:
        s = ln.split(";")[0].strip()
        if not s:
            continue
        m = re.match(r"^(\.L\w+):", s)
        if m:
            labels[m.group(1)] = len(ins)
            continue
        if s.startswith("."):
            continue
        parts = s.split(None, 1)
        ins.append((parts[0], parts[1] if len(parts) > 1 else ""))
    best = None
    for i, (op, args) in enumerate(ins):
        if op.startswith(("s_cbranch", "s_branch")):
            t = labels.get(args.strip())
            if t is not None and t <= i and (best is None or i - t > best[1] - best[0]):
                best = (t, i, args.strip())
    if best is None:
        return count(ins), None, None
    return count(ins), count(ins[best[0]:best[1] + 1]), (best[2], best[1] - best[0] + 1)


def metadata(asm_text, symbol):
    """The kernel's entry of .amdgpu_metadata (the notes kernel_regs.sh reads from a built library)."""
    m = re.search(r"\.name:\s+%s\n" % re.escape(symbol), asm_text)
    blk = ""
    if m:  # an entry runs from its first key (.agpr_count: the keys are sorted) to the next entry's
        start = asm_text.rfind("- .agpr_count", 0, m.start())
        end = asm_text.find("- .agpr_count", m.end())
        blk = asm_text[start:end if end >= 0 else len(asm_text)]
    g = lambda k: int((re.search(r"\.%s:\s+(\d+)" % k, blk) or [0, -1])[1])
    occ = re.search(r"^%s:.*?; Occupancy: (\d+)" % re.escape(symbol), asm_text, re.S | re.M)
    return {"vgpr": g("vgpr_count"), "sgpr": g("sgpr_count"), "vgpr_spill_dwords": g("vgpr_spill_count"),
            "sgpr_spills": g("sgpr_spill_count"), "scratch_bytes": g("private_segment_fixed_size"),
            "static_lds_bytes": g("group_segment_fixed_size"), "occupancy_waves_per_simd": int(occ.group(1)) if occ else -1}


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--kernel", required=True, help="substring of the mangled kernel symbol")
    ap.add_argument("--unit", default="render", help="the translation unit of csrc/ to build: render, calls, queries, ...")
    ap.add_argument("--asm", help="assembly of a unit made with the Makefile's flags (default: build --unit)")
    ap.add_argument("--extra", default="", help="extra hipcc flags for the build")
    ap.add_argument("--json", help="merge the result into this JSON file")
    ap.add_argument("--label", default="census", help="key of the result in --json")
    a = ap.parse_args()
    with tempfile.TemporaryDirectory() as tmp:
        path = a.asm
        if not path:
            path = os.path.join(tmp, a.unit + ".s")
            build_asm(a.unit, path, a.extra.split())
        text = open(path).read()
    found = {k: v for k, v in kernel_bodies(text).items() if a.kernel in k}
    if not found:
        raise SystemExit("no kernel symbol holds %r" % a.kernel)
    result = {}
    for sym, body in found.items():
        whole, loop, hdr = census(body)
        result[sym] = {"counts_are": "static (instructions in the text, not executed)", "metadata": metadata(text, sym),
                       "whole_kernel": whole, "main_loop": loop,
                       "main_loop_header": hdr[0] if hdr else None}
        print(sym)
        print("  metadata  " + "  ".join("%s %d" % kv for kv in result[sym]["metadata"].items()))
        print("  STATIC counts       %-12s %s" % ("whole kernel", "main loop (%s)" % (hdr[0] if hdr else "none")))
        for k in CLASSES + ("instructions",):
            print("  %-18s %12d %12s" % (k, whole[k], loop[k] if loop else "-"))
    if a.json:
        doc = json.load(open(a.json)) if os.path.exists(a.json) else {}
        doc[a.label] = result
        with open(a.json, "w") as fh:
            json.dump(doc, fh, indent=1, sort_keys=True)
            fh.write("\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
