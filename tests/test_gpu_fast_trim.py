"""The trimmed fast list kernels against the general kernel and the oracle, bit for bit: image, per-pixel ray counts,
final RNG states, ray total (tests/parity.py).

The three kernels compiled for the common list frame take their wave votes straight from a compare, form the LDS address
of a staged triangle record with one 24-bit multiply-add, and fold a path's radiance through a table of 16 colours of 16
bytes whose rows the nibbles of the id stack address (kernels.h: trims_votes, trims_mul24, trims_fold_rgb).  None of it
changes the arithmetic on a value, so every frame must be the oracle's and the general kernel's (fast_path = -1, which
keeps every instruction it had).  Every case asserts which kernel its launches used (rtmi_render_mode).

A pinned kernel takes a priority table for granted, which a frame has from eight samples on, and chains are planned from
64 samples on with a first pass of 32 (capi.hip: plan_render): the frames of 8 samples are render_kernel<kFastQueue>'s,
the frames of 64 are probe_kernel<kFastQueue>'s for 32 samples and render_kernel<kFastChains>'s for the rest.  No
tolerances."""
import functools

import numpy as np
import pytest

import fast_trim_worlds as ft
import min_fold_worlds as mf
import tri_tasks_worlds as worlds
from pair_slab_worlds import PLANNED, assert_launch
from parity import assert_same_frame, bits, build_pair, gpu_frame, oracle_frame
from rtmi import scenes

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

QUEUE = dict(lane_stride=1, schedule=0)  # image order, one launch: the whole frame by kFastQueue
LAUNCHES = {"queue": (8, QUEUE), "planned": (64, PLANNED)}
DEPTHS = (1, 2, 3, 4, 5, 6, 7, 8, 9, 50)  # both parities of the top nibble, every remainder of the four-level loop


def assert_same_buffers(a, b, what):
    assert a.total == b.total and np.array_equal(a.counts, b.counts) and np.array_equal(a.states, b.states), what
    assert np.array_equal(bits(a.image), bits(b.image)), what


def check_launch(mode, launch, fast=1):
    if launch == "planned":
        assert_launch(mode, "planned", fast)
    else:
        assert mode["fast_path"] == fast and mode["scheduled"] == 0 and mode["planned_chains"] == 0 and mode["lane_stride"] == 1, mode
        assert mode["wave_priority_every"] > 0, mode


def pinned_general_oracle(ob, pb, side, depth, launch, what, fast=1):
    """The frame by the launch's pinned kernels, by the general kernel and by the oracle: all three the same."""
    spp, opts = LAUNCHES[launch]
    want = oracle_frame(ob, side, side, spp, depth)
    got = gpu_frame(pb, side, side, spp, depth, opts=dict(fast_path=1, **opts))
    check_launch(got.mode, launch, fast)
    assert_same_frame(got, want, "%s, asked for the pinned kernel" % what)
    general = gpu_frame(pb, side, side, spp, depth, opts=dict(fast_path=-1, **opts))
    check_launch(general.mode, launch, 0)
    assert_same_buffers(got, general, "%s, pinned against general" % what)
    return want


@functools.lru_cache(maxsize=None)
def cornell_pair():
    return build_pair(lambda b: scenes.cornell_box(b, 1.0), scenes.SCENE_SEEDS.get("cornell_box", 1024))


@functools.lru_cache(maxsize=None)
def world_pair(name):
    fill = {"box16": ft.box(16), "box17": ft.box(17), "full_list": ft.full_list()}[name]
    return build_pair(fill, 13)


@pytest.mark.parametrize("launch", sorted(LAUNCHES))
@pytest.mark.parametrize("depth", DEPTHS)
def test_cornell_box_at_every_depth(depth, launch):
    """16 x 16: four tiles.  queue: 8 samples by render_kernel<kFastQueue>; planned: 64, probe_kernel<kFastQueue> then
    render_kernel<kFastChains>.  A path of n levels folds n / 4 groups of four, then a pair, with a lone top level before
    them when n is odd: depths 1 to 9 hold every combination, 50 the benchmark's."""
    ob, pb = cornell_pair()
    pinned_general_oracle(ob, pb, 16, depth, launch, "cornell box 16 x 16, depth %d, %s" % (depth, launch))


@pytest.mark.parametrize("launch", sorted(LAUNCHES))
def test_cornell_box_in_one_tile(launch):
    """8 x 8 at depth 50: one tile in a grid with far more lanes than pixels."""
    ob, pb = cornell_pair()
    pinned_general_oracle(ob, pb, 8, 50, launch, "cornell box 8 x 8, %s" % launch)


@pytest.mark.parametrize("launch", sorted(LAUNCHES))
def test_sixteen_materials_read_sixteen_rows(launch):
    """Every material scatters and every colour component differs from every other, so a row read for the wrong nibble
    shows; the frame is lit (the sky through the ceiling's slot) and so is not the zero any product would give."""
    ob, pb = world_pair("box16")
    want = pinned_general_oracle(ob, pb, 16, 50, launch, "room of 16 materials, %s" % launch)
    assert float(want.image.max()) > 0.05 and len(np.unique(bits(want.image))) > 100, "the room is lit"


def test_seventeen_materials_take_the_general_kernel():
    """One material more than nibbles can name: asked for the fast path, the launch reports the general kernel."""
    ob, pb = world_pair("box17")
    spp, opts = LAUNCHES["queue"]
    g = gpu_frame(pb, 16, 16, spp, 50, opts=dict(fast_path=1, **opts))
    assert g.mode["fast_path"] == 0 and g.mode["lane_stride"] == 1, g.mode
    assert_same_frame(g, oracle_frame(ob, 16, 16, spp, 50), "room of 17 materials")


@pytest.mark.parametrize("launch", sorted(LAUNCHES))
def test_longest_staged_list_largest_workgroup(launch):
    """kLdsPairs pairs at depth 50 in workgroups of 256 lanes: the largest record index the staged table has, and the
    largest id-stack offsets."""
    ob, pb = world_pair("full_list")
    assert pb.pair_slabs()[0].shape[0] == ft.LDS_PAIRS + 1, "kLdsPairs pairs and the padding record"
    spp, opts = LAUNCHES[launch]
    LAUNCHES_256 = dict(opts, threads_per_block=256)
    want = oracle_frame(ob, 16, 16, spp, 50)
    got = gpu_frame(pb, 16, 16, spp, 50, opts=dict(fast_path=1, **LAUNCHES_256))
    check_launch(got.mode, launch)
    assert_same_frame(got, want, "full list, %s" % launch)
    general = gpu_frame(pb, 16, 16, spp, 50, opts=dict(fast_path=-1, **LAUNCHES_256))
    check_launch(general.mode, launch, 0)
    assert_same_buffers(got, general, "full list, pinned against general, %s" % launch)


SHEETS = {"sheets_%d%s" % (n, "_light" if light else ""): worlds.sheets(n, light) for n in (2, 3, 4, 7) for light in (False, True)}
SHEETS["mixed_list"] = worlds.mixed_list(7)
SHEETS["ordered_world"] = mf.ordered_world


@pytest.mark.parametrize("world", sorted(SHEETS))
def test_sheets_mixed_and_ordered_worlds(world):
    """The worlds of the fold by minimum (tests/test_gpu_min_fold.py): 64 to 448 shared tasks per flush, lone triangles,
    equal t's, and the world whose flushes are redone in list order -- the flush loop's votes are the trimmed ones."""
    ob, pb = build_pair(SHEETS[world], mf.SEED if world == "ordered_world" else 7)
    pinned_general_oracle(ob, pb, 16, 8, "queue", world)
