"""Common ground of the host-side tests of the C ABI: where the two builds of the library lie, the header's constants
restated, a frame and a null-ish pointer for the argument checks that come before any HIP call, and how a refusal and a
kernel's metadata are read."""
import ctypes as C
import os
import re

import rtmi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHECK_LIB = os.path.join(ROOT, "ray-tracing-cuda_amd", "lib", "librtmi_check1.so")
QUERY_VARIANTS = 8  # launch_cfg.h: kQueryVariants
F_DEFOCUS = 32      # scene_dev.h
OK, ERR_INVALID, ERR_DEPTH = 0, -1, -5  # include/rtmi.h
LIBS = [rtmi.LIB_PATH, os.path.join(os.path.dirname(rtmi.LIB_PATH), "librtmi_check1.so")]


# ------------------------------------------------------------------ refusals before any HIP call
DUMMY = C.c_void_p(16)  # never dereferenced: argument checks come first


def _frame(**kw):
    f = dict(height=20, width=28, spp=4, max_depth=8, post=False)
    f.update(kw)
    return rtmi.make_frame(f["height"], f["width"], f["spp"], f["max_depth"], f["post"], f.get("rank", 0), f.get("world", 1))


def _refused(rc, word, code=ERR_INVALID):
    """The call was refused with `code`, and rtmi_last_error says why in words that hold `word`."""
    assert rc == code, "returned %d, expected %d" % (rc, code)
    msg = rtmi.lib().rtmi_last_error()
    assert msg and word in msg, "the refusal says %r, expected %r in it" % (msg, word)
    return True


def _count(blk, key):
    return int(re.search(r"\.%s:\s+(\d+)" % key, blk).group(1))


def _waves(vgprs):
    """Waves per SIMD that a kernel's VGPR count allows on gfx950: 512 registers in granules of 8, eight waves at most."""
    return min(8, 512 // (-(-vgprs // 8) * 8))
