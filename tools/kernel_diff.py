#!/usr/bin/env python3
"""Per-symbol comparison of two gfx950 assembly files (no GPU): which kernels changed by an instruction?  Any unit with
kernels will do: render.hip, calls.hip, queries.hip, sched.hip, frame.hip, paths.hip, filters.hip, direct.hip, advance.hip.

Both files are made as tools/loop_census.py makes its own (the Makefile's flags, --cuda-device-only -S), one from the
tree before a change and one from the tree after it, unit by unit, with --same '.' when no symbol at all may move:

  git archive <parent> ray-tracing-cuda_amd/csrc include | tar -x -C /tmp/parent
  for u in render calls queries sched frame paths filters direct advance; do
    (cd /tmp/parent/ray-tracing-cuda_amd/csrc && hipcc <FLAGS> --cuda-device-only -S $u.hip -o /tmp/before_$u.s)
    (cd ray-tracing-cuda_amd/csrc && hipcc <FLAGS> --cuda-device-only -S $u.hip -o /tmp/after_$u.s)
    tools/kernel_diff.py /tmp/before_$u.s /tmp/after_$u.s --same 'render_kernel|probe_kernel'
  done

A kernel that moved from one unit to another is compared through the units' assembly files concatenated (cat) on
either side: every symbol is found by its name, wherever in the text it stands.

The diagnostic flavour (make check1) is the same commands with -DRTMI_CHECK_MARGINS -DRTMI_CHECK_EVERY=1 behind <FLAGS>.

A kernel's text is its instructions and labels with comments, directives and blank lines dropped and the function's
number taken out of its local labels (.LBB12_3 -> .LBB_3), so that a kernel added or removed elsewhere in the unit does not
show; its metadata entry (registers, spills, scratch, LDS) is compared too.  Prints one line per symbol that differs, is
new or is gone, then the totals; with --same REGEX exits 1 if a symbol matching it differs, is new or is gone.
"""
import argparse
import re
import sys

from loop_census import kernel_bodies, metadata


def text_of(body):
    out = []
    for ln in body:
        s = ln.split(";")[0].strip()
        if not s or (s.startswith(".") and not re.match(r"^\.L\w+:", s)):
            continue
        out.append(re.sub(r"\.LBB\d+_", ".LBB_", s))
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("before")
    ap.add_argument("after")
    ap.add_argument("--same", default=None, help="regex of symbols that must be unchanged")
    a = ap.parse_args()
    ta, tb = open(a.before).read(), open(a.after).read()
    ka, kb = kernel_bodies(ta), kernel_bodies(tb)
    must = re.compile(a.same) if a.same else None
    same = changed = held = 0
    broken = []
    for name in sorted(set(ka) | set(kb)):
        if name not in ka or name not in kb:
            what = "new" if name not in ka else "gone"
        elif text_of(ka[name]) != text_of(kb[name]):
            what = "text differs (%d -> %d lines)" % (len(text_of(ka[name])), len(text_of(kb[name])))
        elif metadata(ta, name) != metadata(tb, name):
            what = "metadata differs"
        else:
            same += 1
            held += bool(must and must.search(name))
            continue
        changed += 1
        print("%s: %s" % (name, what))
        if must and must.search(name):
            broken.append(name)
    print("%d symbols identical, %d differ, new or gone" % (same, changed))
    if must:
        print("%d symbols matching --same are identical, %d are not" % (held, len(broken)))
    return 1 if broken else 0


if __name__ == "__main__":
    sys.exit(main())
