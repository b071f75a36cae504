"""The list kernel's compile-time fast path (kernels.h: the mode word; render_body.h) against the general kernel.

A launch of a list-triangle scene whose run-time modes are all the common ones runs a kernel compiled for exactly those
modes.  Nothing about a pixel may depend on which kernel rendered it: for the Cornell box and a random list-triangle scene
of at most 16 materials, on power-of-two frames rendered as planned chains, from the queue and in image order, the image,
the per-pixel ray counts, the final RNG states and the ray total are bit-identical with the fast path on and forced off,
and rtmi_render_mode reports which kernel it was.  Launches outside the pinned modes -- 17 materials, a signed colour, a
frame that is no power of two, a thin frame, a sphere, priorities off -- report the general kernel and match the oracle.
"""
import pytest

from parity import assert_same_frame, build_pair, gpu_frame, oracle_frame
from rtmi import scenes
from worlds import random_list

pytestmark = pytest.mark.gpu


def cornell(b, aspect):
    scenes.cornell_box(b, aspect)


def pair(fill, h, w):
    return build_pair(lambda b: fill(b, w / h), 11)


SCENES = [("cornell_box", cornell), ("random_list", random_list())]
# (a) planned chains on a resumed pass: 8,192 tiles, more pixels than the grid has lanes and at most 1.5 tiles per wave, 128 samples; (b) a scheduled frame whose
# second launch draws from the queue; (c) a short frame in image order.  The small frames name lane_stride = 1: left to
# itself a frame with fewer pixels than the grid has lanes is spread thin, which is the general kernel's.
FRAMES = [("planned", 512, 1024, 128, 10, dict(), dict(scheduled=1, first_pass_resumed=1, planned_chains=1)),
          ("queued", 128, 128, 64, 10, dict(schedule=2, plan=0, lane_stride=1), dict(scheduled=1, planned_chains=0)),
          ("image_order", 64, 64, 8, 50, dict(schedule=0, lane_stride=1), dict(scheduled=0, planned_chains=0))]


@pytest.mark.parametrize("frame", FRAMES, ids=[f[0] for f in FRAMES])
@pytest.mark.parametrize("scene", SCENES, ids=[s[0] for s in SCENES])
def test_fast_and_general_kernels_render_the_same_bits(scene, frame):
    _, fill = scene
    _, h, w, spp, depth, opts, want_mode = frame
    _, pb = pair(fill, h, w)
    fast = gpu_frame(pb, h, w, spp, depth, opts=dict(fast_path=1, **opts))
    general = gpu_frame(pb, h, w, spp, depth, opts=dict(fast_path=-1, **opts))
    assert fast.mode["fast_path"] == 1 and general.mode["fast_path"] == 0, (fast.mode, general.mode)
    for k, v in want_mode.items():
        assert fast.mode[k] == v and general.mode[k] == v, (k, fast.mode, general.mode)
    assert fast.mode["lane_stride"] == 1 and fast.mode["wave_priority_every"] > 0
    assert {k: v for k, v in fast.mode.items() if k != "fast_path"} == {k: v for k, v in general.mode.items() if k != "fast_path"}
    assert fast.total > h * w * spp  # the scene is in view
    assert_same_frame(fast, general, "fast against general")


def test_default_is_the_fast_path_and_it_matches_the_oracle():
    """No option named: the fast kernel, and its frame is the oracle's bit for bit."""
    ob, pb = pair(random_list(), 32, 64)
    g = gpu_frame(pb, 32, 64, 8, 12, opts=dict(lane_stride=1))
    assert g.mode["fast_path"] == 1, g.mode
    assert_same_frame(g, oracle_frame(ob, 32, 64, 8, 12), "default")


NEGATIVE = [("17_materials", random_list(n_mats=17), 32, 64, dict(lane_stride=1)),
            ("signed_colour", random_list(signed=True), 32, 64, dict(lane_stride=1)),
            ("not_a_power_of_two", random_list(), 24, 40, dict(lane_stride=1)),
            ("thin_frame", random_list(), 32, 64, dict()),
            ("sphere", random_list(sphere=True), 32, 64, dict(lane_stride=1)),
            ("priorities_off", random_list(), 32, 64, dict(lane_stride=1, wave_priority=0))]


@pytest.mark.parametrize("case", NEGATIVE, ids=[c[0] for c in NEGATIVE])
def test_launches_outside_the_pinned_modes_use_the_general_kernel(case):
    """Each case differs from the launch of test_default_is_the_fast_path_and_it_matches_the_oracle in the one thing it
    is named after; asked for the fast path, it reports the general kernel and renders the oracle's frame."""
    name, fill, h, w, opts = case
    ob, pb = pair(fill, h, w)
    g = gpu_frame(pb, h, w, 8, 12, opts=dict(fast_path=1, **opts))
    assert g.mode["fast_path"] == 0, g.mode
    if name == "thin_frame":
        assert g.mode["lane_stride"] > 1, g.mode
    else:
        assert g.mode["lane_stride"] == 1, g.mode
    assert (g.mode["wave_priority_every"] == 0) == (name == "priorities_off"), g.mode
    assert_same_frame(g, oracle_frame(ob, h, w, 8, 12), name)
