"""The fast list kernels' fold by one LDS minimum per ray (closest_hit.h, RUN_TRIS, steps (b) and (c)) against the oracle,
bit for bit: image, per-pixel ray counts, final RNG states, ray total (tests/parity.py).

The three kernels compiled for the common list frame post one 64-bit key per accepted pair of a flush, (bits of t) << 32 |
place in the chunk, and each ray reads its smallest; a flush that holds a task with both triangles accepted and the second
nearer is redone in list order, and such tasks are counted in rtmi_debug_counters' word 16.  The stacked sheets and the
mixed list of tests/tri_tasks_worlds.py put 64 to 448 tasks into a wave's flush, equal t's and lone triangles among them;
tests/min_fold_worlds.py builds the world whose flushes take the ordered path and says how many of its tasks must;
the Cornell box runs every pinned kernel.  Every case asserts which kernel its launch used (rtmi_render_mode), and the
general kernel (fast_path = -1), which keeps the fold in list order, must give the same buffers.  No tolerances."""
import ctypes as C
import functools
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import min_fold_worlds as mf
import rtmi
import tri_tasks_worlds as worlds
from abi_host import CHECK_LIB, ROOT
from pair_slab_worlds import LAUNCHES, assert_launch
from parity import assert_same_frame, bits, build_pair, gpu_frame, oracle_frame
from rtmi import scenes

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

ONE_LAUNCH = dict(lane_stride=1, schedule=0)  # image order: the whole frame by kFastQueue
SHEETS = {"sheets_%d%s" % (n, "_light" if light else ""): worlds.sheets(n, light) for n in (2, 3, 4, 7) for light in (False, True)}
SHEETS["mixed_list"] = worlds.mixed_list(7)


def ordered_count(b):
    c = (C.c_ulonglong * 40)()
    assert rtmi.lib().rtmi_debug_counters(b.h, c, None) == 0
    return int(c[mf.ORDERED_WORD])


def assert_same_buffers(a, b, what):
    assert a.total == b.total and np.array_equal(a.counts, b.counts) and np.array_equal(a.states, b.states), what
    assert np.array_equal(bits(a.image), bits(b.image)), what


@pytest.mark.parametrize("side,spp", [(16, 4), (16, 8), (8, 8)], ids=["16x16x4", "16x16x8", "thin"])
@pytest.mark.parametrize("world", sorted(SHEETS))
def test_sheets_and_mixed_list(world, side, spp):
    """16 x 16: four full waves.  8 x 8: one tile in a grid with far more lanes than pixels, most of them workers without
    a ray of their own, whose key slots nobody reads.  A pinned kernel takes a priority table for granted and a frame
    gets one from eight samples on (capi.hip: plan_render), so the frames of 4 samples -- the shape of
    tests/test_gpu_tri_tasks.py -- are the general kernel's whatever is asked, and the frames of 8 the pinned one's."""
    ob, pb = build_pair(SHEETS[world], 7)
    want = oracle_frame(ob, side, side, spp, 8)
    fast = gpu_frame(pb, side, side, spp, 8, opts=dict(fast_path=1, **ONE_LAUNCH))
    assert fast.mode["fast_path"] == (1 if spp >= 8 else 0) and fast.mode["scheduled"] == 0 and fast.mode["lane_stride"] == 1, fast.mode
    assert_same_frame(fast, want, "%s %d x %d, pinned kernel" % (world, side, side))
    general = gpu_frame(pb, side, side, spp, 8, opts=dict(fast_path=-1, **ONE_LAUNCH))
    assert general.mode["fast_path"] == 0, general.mode
    assert_same_buffers(fast, general, "%s %d x %d, pinned against general" % (world, side, side))


@functools.lru_cache(maxsize=None)
def ordered_pair():
    return build_pair(mf.ordered_world, mf.SEED)


def test_ordered_world_takes_the_ordered_path():
    """Every ray of this frame is a camera ray the host can restate (tests/test_min_fold_host.py holds the restatement and
    asks it for at least 8 tasks of the ordered kind): the device must count at least as many, and the frame is the
    oracle's."""
    ob, pb = ordered_pair()
    O, D = mf.frame_rays(ob.camera_get())
    need, both, _ = mf.ordered_tasks(O, D)
    assert need >= 8, (need, both)
    want = oracle_frame(ob, mf.SIDE, mf.SIDE, mf.SPP, mf.DEPTH)
    assert want.total == mf.SIDE * mf.SIDE * mf.SPP, "every path is its camera ray"
    g = gpu_frame(pb, mf.SIDE, mf.SIDE, mf.SPP, mf.DEPTH, opts=dict(fast_path=1, **ONE_LAUNCH))
    counted = ordered_count(pb)
    print("mode", g.mode, "ordered tasks: host", need, "of", both, "with both accepted; device", counted)
    assert g.mode["fast_path"] == 1 and g.mode["scheduled"] == 0 and g.mode["lane_stride"] == 1, g.mode
    assert_same_frame(g, want, "ordered world, pinned kernel")
    assert counted >= need, (counted, need)
    general = gpu_frame(pb, mf.SIDE, mf.SIDE, mf.SPP, mf.DEPTH, opts=dict(fast_path=-1, **ONE_LAUNCH))
    assert general.mode["fast_path"] == 0 and ordered_count(pb) == 0, general.mode  # (the word is the pinned kernels' alone)
    assert_same_buffers(g, general, "ordered world, pinned against general")


def test_ordered_world_in_two_launches():
    """64 x 64 x 64 (chains are planned from 64 samples on): the probe kernel for 32 of them, then the planned chains --
    the other two pinned kernels on the same world."""
    ob, pb = ordered_pair()
    spp, opts = LAUNCHES["planned"]
    want = oracle_frame(ob, 64, 64, spp, mf.DEPTH)
    g = gpu_frame(pb, 64, 64, spp, mf.DEPTH, opts=opts)
    print("mode", g.mode)
    assert_launch(g.mode, "planned")
    assert_same_frame(g, want, "ordered world, probe and chains")
    assert ordered_count(pb) > 0  # (the second launch's: the word is zeroed with the per-launch words)


@pytest.mark.parametrize("launch", sorted(LAUNCHES))
def test_cornell_box_through_every_pinned_kernel(launch):
    """64 x 64 x 64 at depth 50.  planned: probe_kernel<kFastQueue> renders the first 32 samples and
    render_kernel<kFastChains> resumes them; queue: render_kernel<kFastQueue> renders all 64 (one launch)."""
    _, opts = LAUNCHES[launch]
    ob, pb = cornell_pair()
    g = gpu_frame(pb, 64, 64, 64, 50, opts=opts)
    print("mode", g.mode, "ordered tasks", ordered_count(pb))
    assert_launch(g.mode, launch)
    assert_same_frame(g, cornell_oracle(), "cornell box, " + launch)


@functools.lru_cache(maxsize=None)
def cornell_pair():
    return build_pair(lambda b: scenes.cornell_box(b, 1.0), scenes.SCENE_SEEDS.get("cornell_box", 1024))


@functools.lru_cache(maxsize=None)
def cornell_oracle():
    return oracle_frame(cornell_pair()[0], 64, 64, 64, 50)


def test_the_check_build_agrees_on_every_query():
    """librtmi_check1.so answers every query a second time with the plain scan (tests/min_fold_check.py): the ordered
    world in one launch and in two, the sheets and the mixed list; every query re-done, no disagreement, and the ordered
    world did take the ordered path."""
    assert os.path.exists(CHECK_LIB), "librtmi_check1.so missing: run __graft_entry__.build() (make -C csrc check1)"
    env = dict(os.environ, RTMI_LIB_PATH=CHECK_LIB)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "min_fold_check.py")], env=env, cwd=ROOT,
                       stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-4000:]
    out = json.loads(r.stdout[r.stdout.index("{"):])
    assert len(out) == 2 + 2 * len(SHEETS), sorted(out)
    for tag, v in out.items():
        assert v["fast_path"] == 1, (tag, v)
        assert v["re_done"] == v["rays"] > 0, (tag, v)
        assert v["disagreements"] == 0, (tag, v)
        if tag.startswith("ordered"):
            assert v["ordered_tasks"] > 0, (tag, v)
