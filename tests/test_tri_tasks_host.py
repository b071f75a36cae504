"""The culled list scan's per-triangle records on the host side: what scene.hip puts into them, the LDS a launch asks
for, and the kernels' code-object metadata after the change.  No GPU involved."""
import re

import numpy as np
import pytest

import common
import rtmi
import tri_tasks_worlds as worlds
from abi_host import LIBS, _count, _waves

TRIPTS_ABSENT = 1  # scene_dev.h
TRI_SECOND = 1


def _builder(fill, seed=7):
    b = rtmi.SceneBuilder(seed)
    fill(b)
    return b


def _cornell():
    return common.build_scene(rtmi.SceneBuilder(common.scene_seed("cornell_box")), "cornell_box", 1.0)


WORLDS = {"cornell_box": _cornell, "mixed_list": lambda: _builder(worlds.mixed_list(7)),
          "long_list": lambda: _builder(worlds.long_list(130))}


@pytest.mark.parametrize("name", sorted(WORLDS))
def test_records_hold_the_corners_float32_differences_and_the_hot_records_edges(name):
    tp, ht, co = WORLDS[name]().list_records()
    n = len(tp)
    assert n >= 5 and tp.shape == (n, 2, 12) and ht.shape == (n, 2, 16) and co.shape == (n, 4, 3)
    f = tp.view(np.float32)
    lone = (ht[:, 1, 13] & TRI_SECOND) == 0  # a lone Triangle's second HotTri is inert
    assert name != "mixed_list" or (lone.sum() == 4 and (~lone).sum() == 3)
    assert name != "cornell_box" or not lone.any()
    for which, (a, b, c) in enumerate(((0, 1, 2), (1, 2, 3))):
        rows = np.ones(n, bool) if which == 0 else ~lone
        want = np.concatenate([co[:, a], co[:, b] - co[:, a], co[:, c] - co[:, a]], axis=1)  # float32 arithmetic
        assert want.dtype == np.float32
        assert np.array_equal(f[rows, which, :9].view(np.uint32), want[rows].view(np.uint32)), (name, which)
        assert np.array_equal(tp[rows, which, :9], ht[rows, which, :9]), (name, which)  # HotTri: p0, e1, e2 first
        assert (tp[rows, which, 9] == 0).all() and (tp[:, which, 10:] == 0).all()
    # absent seconds: flagged, and nothing else is
    assert np.array_equal((tp[:, 1, 9] & TRIPTS_ABSENT) != 0, lone)
    assert (tp[:, 0, 9] == 0).all()
    assert (tp[lone, 1, :9] == 0).all()


def test_c2_still_fits_six_workgroups_per_cu():
    """C2: cornell_box at depth 50 in workgroups of 256 lanes -- six of them are the six waves per SIMD the list kernels
    are built for, and a compute unit's 160 KiB of LDS must hold all six."""
    lds = _cornell().render_lds_bytes(50, 256)
    assert 0 < lds and 6 * lds <= 160 * 1024, lds
    # the records are staged: two of 48 bytes per pair more than a launch without the culled scan would ask for
    assert _builder(worlds.long_list(130)).render_lds_bytes(50, 256) < _builder(worlds.long_list(128)).render_lds_bytes(50, 256)


# (vgpr_count, vgpr_spill_count, sgpr_spill_count) of the fast list kernels before the per-triangle tasks
FAST_BEFORE = {"render_kernelILj2ELj255E": (80, 0, 5), "render_kernelILj2ELj383E": (80, 3, 13),
               "probe_kernelILj2ELj383E": (80, 3, 13)}
# waves per SIMD of every kernel that holds a closest_hit before the change, by its VGPR count then (tools/kernel_regs.sh)
VGPRS_BEFORE = {
    "render_kernelILj2ELj0E": 80, "render_kernelILj3ELj0E": 117, "render_kernelILj7ELj0E": 128, "render_kernelILj19ELj0E": 96,
    "render_kernelILj63ELj0E": 168, "probe_kernelILj2ELj0E": 80, "probe_kernelILj3ELj0E": 117, "probe_kernelILj7ELj0E": 128,
    "probe_kernelILj19ELj0E": 96, "probe_kernelILj63ELj0E": 168, "query_kernelILj18E": 76, "query_kernelILj19E": 91,
    "query_kernelILj23E": 110, "query_kernelILj26E": 123, "query_kernelILj31E": 163, "occlusion_kernelILj18E": 77,
    "occlusion_kernelILj19E": 89, "occlusion_kernelILj23E": 115, "occlusion_kernelILj26E": 126, "occlusion_kernelILj31E": 160,
    "trace_kernelILj18E": 103, "trace_kernelILj19E": 96, "trace_kernelILj23E": 128, "trace_kernelILj26E": 140,
    "feature_kernelILj50E": 108, "budget_kernelILj50E": 108, "feature_kernelILj51E": 96, "budget_kernelILj51E": 96,
    "feature_kernelILj55E": 128, "budget_kernelILj55E": 128, "feature_kernelILj58E": 152, "budget_kernelILj58E": 152,
    "feature_kernelILj63E": 168, "budget_kernelILj63E": 168}


def test_the_kernels_hold_their_occupancy_steps():
    """The product build: both fast kernels at 80 VGPRs with no more spilled VGPRs or SGPRs than before, every other
    kernel of the triangle scan at the waves per SIMD it had, and no static LDS anywhere (both builds)."""
    notes = common.kernel_notes(LIBS[0])

    def block(key):
        got = [blk for name, blk in notes.items() if key in name]
        assert len(got) == 1, (key, len(got))
        return got[0]

    for key, (vgprs, vspill, sspill) in FAST_BEFORE.items():
        blk = block(key)
        assert _count(blk, "vgpr_count") <= 80 and _waves(_count(blk, "vgpr_count")) == _waves(vgprs) == 6, key
        assert _count(blk, "vgpr_spill_count") <= vspill, key
        assert _count(blk, "sgpr_spill_count") <= sspill, key
    for key, vgprs in VGPRS_BEFORE.items():
        assert _waves(_count(block(key), "vgpr_count")) >= _waves(vgprs), (key, vgprs)
    for lib in LIBS:
        for name, blk in common.kernel_notes(lib).items():
            if re.search(r"(render|probe|query|occlusion|trace|feature|budget)_kernel", name):
                assert re.search(r"\.group_segment_fixed_size:\s+0\b", blk), (lib, name)
