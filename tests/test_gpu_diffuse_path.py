"""The diffuse kernels against the general kernel and the oracle, bit for bit: image, per-pixel ray counts, final RNG
states, ray total (tests/parity.py).

A scene whose materials are all Lambertians or lights gets the three fast list kernels once more, compiled for it
(kernels.h: PIN_DIFFUSE): no metal or dielectric text, and a lane whose path ends taking the next sample's
two camera draws with the first trip of the rejection sampler.  None of it changes an operation on a
value or the order of a pixel's draws, so every frame must be the oracle's and the general kernel's (fast_path = -1),
and the states behind a pixel's last sample the oracle's -- a draw too many or too few at a pixel's end shows there.

Every case asserts which kernels its launches were (rtmi_render_pins): 895 = kFastQueue | PIN_DIFFUSE from the queue,
767 = kFastChains | PIN_DIFFUSE on planned chains; 383 and 255 without the pin; 0 the general kernel or no first pass.
A pinned kernel takes a priority table for granted, which a frame has from eight samples on, and chains are planned from
64 samples on: the frames of 8 samples are render_kernel<895>'s, the frames of 64 are probe_kernel<895>'s for 32 samples
and render_kernel<767>'s for the rest.  No tolerances."""
import functools

import numpy as np
import pytest

import diffuse_worlds as dw
from pair_slab_worlds import PLANNED
from parity import assert_same_frame, bits, build_pair, gpu_frame, oracle_frame

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

PIN_DIFFUSE = 512
QUEUE_PINS, CHAIN_PINS = 383, 255
QUEUE = dict(lane_stride=1, schedule=0)  # image order, one launch
LAUNCHES = {"queue": (8, QUEUE), "planned": (64, PLANNED)}  # PLANNED: a first pass of 32 samples from the queue, then chains
DEPTHS = (1, 2, 3, 9, 50)


@functools.lru_cache(maxsize=None)
def pair(world):
    fill, seed = dw.WORLDS[world]
    return build_pair(fill, seed)


@functools.lru_cache(maxsize=None)
def oracle(world, side, spp, depth):
    """One oracle frame per (world, shape), shared by the cases that need it; read-only (parity.oracle_frame)."""
    return oracle_frame(pair(world)[0], side, side, spp, depth)


def expected_pins(launch, diffuse):
    extra = PIN_DIFFUSE if diffuse else 0
    return (0, QUEUE_PINS | extra) if launch == "queue" else (QUEUE_PINS | extra, CHAIN_PINS | extra)


def assert_same_buffers(a, b, what):
    assert a.total == b.total and np.array_equal(a.counts, b.counts) and np.array_equal(a.states, b.states), what
    assert np.array_equal(bits(a.image), bits(b.image)), what


def pinned_general_oracle(world, side, depth, launch, diffuse=True, spp=None, opts=None, want=None):
    """The frame by the launch's pinned kernels -- asserted to be the diffuse ones, or not -- by the general kernel and by
    the oracle: all three the same."""
    what = "%s %d x %d, depth %d, %s" % (world, side, side, depth, launch)
    pb = pair(world)[1]
    if spp is None:
        spp, opts = LAUNCHES[launch]
    want = want or oracle(world, side, spp, depth)
    fast = dict(fast_path=1, **opts)
    assert dw.render_pins(pb, side, spp, depth, fast) == expected_pins(launch, diffuse), what
    got = gpu_frame(pb, side, side, spp, depth, opts=fast)
    assert got.mode["fast_path"] == 1 and got.mode["lane_stride"] == 1, got.mode
    assert got.mode["planned_chains"] == (launch == "planned"), got.mode
    assert_same_frame(got, want, "%s, asked for the pinned kernel" % what)
    slow = dict(fast_path=-1, **opts)
    assert dw.render_pins(pb, side, spp, depth, slow) == (0, 0), what
    general = gpu_frame(pb, side, side, spp, depth, opts=slow)
    assert_same_buffers(got, general, "%s, pinned against general" % what)
    return got, want


@pytest.mark.parametrize("launch", sorted(LAUNCHES))
@pytest.mark.parametrize("depth", DEPTHS)
@pytest.mark.parametrize("side", (16, 8))
def test_cornell_box(side, depth, launch):
    """16 x 16 is four tiles, 8 x 8 one tile in a grid with far more lanes than pixels.  Depth 1 ends every path at its
    second hit, so nearly every iteration restarts most lanes; 2, 3 and 9 hold both parities of the id stack's top nibble
    and a fold shorter than one group of four; 50 is the benchmark's."""
    pinned_general_oracle("cornell_box", side, depth, launch)


@pytest.mark.parametrize("launch", sorted(LAUNCHES))
@pytest.mark.parametrize("depth", (3, 50))
def test_an_unused_metal_keeps_the_kernels_that_were(depth, launch):
    """The fact is the material table's: one metal that no primitive has, and the launches are 383 / 255 again.  The
    image, the ray counts and ALL the RNG states are the plain Cornell box's -- neither builder draws for a material, so
    pixel 0's state needs no exception -- and the diffuse kernels' frame of that box is this frame."""
    spp, opts = LAUNCHES[launch]
    plain = oracle("cornell_box", 16, spp, depth)
    got, _ = pinned_general_oracle("unused_metal", 16, depth, launch, diffuse=False, want=plain)
    diffuse = gpu_frame(pair("cornell_box")[1], 16, 16, spp, depth, opts=dict(fast_path=1, **opts))
    assert_same_buffers(got, diffuse, "with and without the unused metal, %s" % launch)


@pytest.mark.parametrize("launch", sorted(LAUNCHES))
@pytest.mark.parametrize("world", ("panel_room", "sky_room"))
def test_rooms_of_sixteen_materials(world, launch):
    """The panel is material 15, the last a nibble names; the sky room has no light and sixteen rows of colours.  Either
    way most paths end once, lit: at the panel or in the sky."""
    _, want = pinned_general_oracle(world, 16, 50, launch)
    assert float(want.image.max()) > 0.05 and len(np.unique(bits(want.image))) > 100, "the room is lit"


def test_one_sample_behind_the_first_pass():
    """65 samples with a first pass of 64: every pixel's last sample is its first in the chains launch, so every path's
    end is a pixel's end, where a restarting lane must draw nothing.  The states are the oracle's."""
    opts = dict(lane_stride=1, schedule=2, plan=2, probe_spp=64)
    got, _ = pinned_general_oracle("cornell_box", 16, 50, "planned", spp=65, opts=opts)
    assert got.mode["first_pass_samples"] == 64 and got.mode["first_pass_resumed"] == 1, got.mode


def test_two_samples_behind_the_first_pass():
    """66: one restart per pixel in the chains launch, then the pixel's end."""
    opts = dict(lane_stride=1, schedule=2, plan=2, probe_spp=64)
    pinned_general_oracle("cornell_box", 16, 9, "planned", spp=66, opts=opts)


def test_a_frame_of_one_sample():
    """One sample per pixel.  Such a frame has no wave priorities (they start at eight samples), which every pinned kernel
    takes for granted: its one launch is the general kernel's, and says so."""
    ob, pb = pair("cornell_box")
    assert dw.render_pins(pb, 16, 1, 50, dict(fast_path=1, **QUEUE)) == (0, 0)
    got = gpu_frame(pb, 16, 16, 1, 50, opts=dict(fast_path=1, **QUEUE))
    assert got.mode["fast_path"] == 0, got.mode
    assert_same_frame(got, oracle("cornell_box", 16, 1, 50), "cornell box, one sample")
