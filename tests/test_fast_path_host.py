"""The fast path's host side: which trace kernel a launch gets (kernels.h: fast_path_mode), asked through the ABI as a pure
function (rtmi_fast_path_kernel: no device, no scene), the new entries in both builds of the library, the option field
that took the place of rtmi_render_opts.reserved, and the fast kernels in the code object.  No GPU involved."""
import ctypes as C
import itertools
import os
import re
import subprocess
import tempfile

import pytest

import common
import rtmi
from abi_host import LIBS

GENERAL, QUEUE, CHAINS = 0, 1, 2
NAMES = ("enabled", "variant", "n_mats", "mats_in_lds", "pairs_in_lds", "unsigned_colours", "det_safe", "width", "height",
         "lane_stride", "priorities", "chains", "resumed", "tile_cost")
# C2's second launch: everything the chain kernel was compiled for
COMMON = dict(enabled=1, variant=2, n_mats=9, mats_in_lds=1, pairs_in_lds=1, unsigned_colours=1, det_safe=1, width=1024,
              height=1024, lane_stride=1, priorities=1, chains=1, resumed=1, tile_cost=1)
# kernel variant bits (scene_dev.h): F_SPHERE 1, F_TRIS 2, F_SGROUP 4, F_BVH 8, F_TEX 16, F_DEFOCUS 32
LIST_TRIANGLES = 2


def kernel(**kw):
    f = dict(COMMON, **kw)
    assert sorted(f) == sorted(NAMES)
    arr = (C.c_int32 * rtmi.FAST_PATH_FACTS)(*[f[n] for n in NAMES])
    return rtmi.lib().rtmi_fast_path_kernel(arr)


def test_the_common_launches_get_the_fast_kernels():
    assert len(NAMES) == rtmi.FAST_PATH_FACTS
    assert kernel() == CHAINS                                      # C2 / a C4 shard: the resumed, planned launch
    assert kernel(chains=0) == QUEUE                               # the full C4 frame: scheduled, queued
    assert kernel(chains=0, resumed=0, tile_cost=0) == QUEUE       # a first pass, an image-order frame
    assert kernel(chains=0, resumed=0, tile_cost=1) == QUEUE
    assert kernel(n_mats=1) == CHAINS and kernel(n_mats=16) == CHAINS
    assert kernel(width=1, height=1 << 20, chains=0) == QUEUE      # the binary32 jitter's own bounds
    assert kernel(enabled=7) == CHAINS                             # (any non-zero switch is on)


@pytest.mark.parametrize("chains", [0, 1])
def test_every_pinned_condition_is_needed(chains):
    """One fact changed at a time: each sends the launch to the general kernel."""
    want = CHAINS if chains else QUEUE
    assert kernel(chains=chains) == want
    for change in (dict(enabled=0), dict(variant=0), dict(variant=LIST_TRIANGLES | 1), dict(variant=LIST_TRIANGLES | 8),
                   dict(variant=LIST_TRIANGLES | 16), dict(variant=LIST_TRIANGLES | 32), dict(variant=63), dict(n_mats=17),
                   dict(n_mats=0), dict(n_mats=300), dict(mats_in_lds=0), dict(pairs_in_lds=0), dict(unsigned_colours=0),
                   dict(det_safe=0), dict(width=1000), dict(height=768), dict(width=0), dict(width=1 << 21), dict(height=1 << 21),
                   dict(lane_stride=2), dict(lane_stride=16), dict(lane_stride=0), dict(priorities=0)):
        assert kernel(chains=chains, **change) == GENERAL, change


def test_the_chain_kernel_is_for_resumed_passes_with_tile_costs():
    """Planned chains without a first pass behind them (no launch_render caller makes one today): the general kernel,
    never the queue kernel, which has no chain code at all."""
    assert kernel(resumed=0) == GENERAL
    assert kernel(tile_cost=0) == GENERAL
    assert kernel(resumed=0, tile_cost=0) == GENERAL


def test_truth_table_against_the_rule_restated():
    """All 2^11 combinations of the yes / no facts (the others at their good and one bad value) against the rule of
    include/rtmi.h written out here."""
    flags = ("enabled", "mats_in_lds", "pairs_in_lds", "unsigned_colours", "det_safe", "priorities", "chains", "resumed", "tile_cost")
    others = [dict(), dict(variant=3), dict(n_mats=17), dict(width=640), dict(lane_stride=4)]
    for bits in itertools.product((0, 1), repeat=len(flags)):
        f = dict(zip(flags, bits))
        for o in others:
            common = all(f[k] for k in flags[:6]) and not o
            want = GENERAL if not common else QUEUE if not f["chains"] else CHAINS if f["resumed"] and f["tile_cost"] else GENERAL
            assert kernel(**f, **o) == want, (f, o)


def test_null_arguments_are_refused_before_any_device_call():
    L = rtmi.lib()
    assert L.rtmi_fast_path_kernel(None) == -1
    assert L.rtmi_render_mode_ex(None, None, None, None, 9) == -1
    b = rtmi.SceneBuilder(1)
    out = (C.c_int32 * 9)()
    assert L.rtmi_render_mode_ex(b.h, C.byref(rtmi.make_frame(8, 8, 1)), None, out, -1) == -1
    assert L.rtmi_render_mode_ex(b.h, C.byref(rtmi.make_frame(8, 8, 1)), None, out, 9) == -1  # (not committed)
    assert b"committed" in L.rtmi_last_error()


def test_entries_are_exported_by_both_builds_and_the_header_agrees():
    names = [s[0] for s in rtmi.SYMBOLS]
    for path in LIBS:
        lib = C.CDLL(path)
        for e in ("rtmi_render_mode_ex", "rtmi_fast_path_kernel"):
            assert e in names and hasattr(lib, e), (path, e)
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    src = ('#include <stdio.h>\n#include <stddef.h>\n#include "rtmi.h"\nint main(void) { printf("%d %d %zu %zu", RTMI_MODE_FIELDS, '
           'RTMI_FAST_PATH_FACTS, sizeof(rtmi_render_opts), offsetof(rtmi_render_opts, fast_path)); return 0; }\n')
    with tempfile.TemporaryDirectory() as tmp:
        c, exe = os.path.join(tmp, "s.c"), os.path.join(tmp, "s")
        with open(c, "w") as fh:
            fh.write(src)
        subprocess.check_call(["cc", "-I", os.path.join(root, "include"), c, "-o", exe])
        got = [int(x) for x in subprocess.check_output([exe], text=True).split()]
    assert got == [rtmi.MODE_FIELDS, rtmi.FAST_PATH_FACTS, C.sizeof(rtmi.RenderOpts), rtmi.RenderOpts.fast_path.offset]
    assert got[2] == 88  # the struct did not grow: fast_path is the word that was `reserved`


def test_fast_path_option_is_validated():
    L = rtmi.lib()
    b = rtmi.SceneBuilder(1)
    fr = rtmi.make_frame(8, 8, 1)
    dummy = C.c_void_p(16)  # never dereferenced: argument checks come first
    for bad in (2, -2, 100):
        o = rtmi.render_opts(fast_path=bad)
        assert L.rtmi_render_ex(b.h, C.byref(fr), C.byref(o), dummy, dummy, None, None) == -1, bad
        assert b"out of range" in L.rtmi_last_error()
    for good in (-1, 0, 1):
        o = rtmi.render_opts(fast_path=good)
        assert L.rtmi_render_ex(b.h, C.byref(fr), C.byref(o), dummy, dummy, None, None) == -1
        assert b"committed" in L.rtmi_last_error(), good  # (it got past the options)


def test_fast_kernels_are_in_both_builds_at_six_waves_per_simd():
    """render_kernel<F_TRIS, kFastChains = 255>, <F_TRIS, kFastQueue = 383> and the first pass's probe_kernel<F_TRIS, 383>:
    present, no static LDS (render_body.h addresses LDS by byte offsets), and -- the product build -- at most 80 VGPRs,
    the six-waves-per-SIMD step the list kernel is held at."""
    want = ("render_kernelILj2ELj255E", "render_kernelILj2ELj383E", "probe_kernelILj2ELj383E")
    for lib in LIBS:
        seen = set()
        for name, blk in common.kernel_notes(lib).items():
            for w in want:
                if w in name:
                    seen.add(w)
                    assert re.search(r"\.group_segment_fixed_size:\s+0\b", blk), (lib, name)
                    if lib == LIBS[0]:
                        assert int(re.search(r"\.vgpr_count:\s+(\d+)", blk).group(1)) <= 80, (lib, name)
        assert seen == set(want), (lib, seen)
