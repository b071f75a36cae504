"""The trace loop's one normalisation site (render_body.h: kOwesBit) against the oracle, bit for bit.

The two fast list kernels leave a Lambertian bounce's direction raw and normalise it at the top of the next iteration,
in the call that normalises the new camera rays.  Every value still goes through the operations it went through, so
the image, the per-pixel ray counts, the final RNG states and the ray total must be the oracle's, whatever shares a
wave: paths cut by the depth limit while they owe, lanes that never owe (metal, dielectric), a wave sent through the
IEEE forms by one camera ray (tests/test_deferred_normalise_host.py).  The general kernels and the caller-owned trace,
budget and feature kernels do not defer and are instruction for instruction what they were (kernels.h: defers_unit;
NOTES.md): the general-kernel cases and the budget case below are guards on that.

Which kernel renders a 64 x 64 frame (capi.hip: plan_render).  Left to itself the frame is spread thin, one pixel per
several lanes, and is not scheduled (it has fewer pixels than the grid has lanes): one launch of the general kernel.
With lane_stride = 1, as tests/test_gpu_fast_path.py names it, that one launch is kFastQueue.  kFastChains is the second
launch of a planned frame, which a frame this small is only when asked: schedule = 2, plan = 2, from 64 samples on; with
32 of them in the first pass that pass has wave priorities and is kFastQueue too.  rtmi_render_mode says what each
call was, and every case asserts it.
"""
import functools

import numpy as np
import pytest

from budgetlib import OracleReplay, Shards
from pair_slab_worlds import LAUNCHES, assert_launch
from parity import assert_same_frame, build_pair, gpu_frame, oracle_frame
from rtmi import scenes
from worlds import SIDE, random_list, slow_camera

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

H = W = SIDE


def cornell(b, aspect):
    scenes.cornell_box(b, aspect)


def spheres(b, aspect):
    scenes.spheres(b, aspect)


def cornell_slow_camera(b, aspect):
    """The Cornell box seen by the raw camera whose corner pixel leaves unit3_rn_twice's domain."""
    scenes.cornell_box(b, aspect)
    b.camera_raw(*slow_camera())


WORLDS = {"cornell_box": (cornell, scenes.SCENE_SEEDS.get("cornell_box", 1024)),
          "spheres": (spheres, scenes.SCENE_SEEDS.get("spheres", 1024)),
          "mixed_list": (random_list(), 11),  # metal with and without fuzz, dielectric, Lambertian: on the fast path
          "slow_camera": (cornell_slow_camera, 1024)}


@functools.lru_cache(maxsize=None)
def pair(world):
    fill, seed = WORLDS[world]
    return build_pair(lambda b: fill(b, W / H), seed)


@functools.lru_cache(maxsize=None)
def oracle(world, spp, depth):
    """Computed once per frame, read by every case of it."""
    return oracle_frame(pair(world)[0], H, W, spp, depth)


def gpu(world, spp, depth, **opts):
    """The same through rtmi_render_ex, and what rtmi_render_mode says of the call."""
    return gpu_frame(pair(world)[1], H, W, spp, depth, opts=opts or None)


def assert_is_the_oracles(got, want, what):
    assert got.total > H * W, what  # the world is in view
    assert_same_frame(got, want, what)


# ------------------------------------------------------------------ the Cornell box, 64 x 64, depth 50
def test_frame_with_no_option_named():
    """40 samples as a caller gets them: whatever kernel the library picks, the oracle's frame."""
    g = gpu("cornell_box", 40, 50)
    print("mode", g.mode)
    assert_is_the_oracles(g, oracle("cornell_box", 40, 50), "default options")


@pytest.mark.parametrize("launch", sorted(LAUNCHES))
def test_fast_kernels(launch):
    """queue: kFastQueue alone.  planned: both launches, kFastQueue then kFastChains on the pass it left."""
    spp, opts = LAUNCHES[launch]
    g = gpu("cornell_box", spp, 50, **opts)
    print("mode", g.mode)
    assert_launch(g.mode, launch)
    assert_is_the_oracles(g, oracle("cornell_box", spp, 50), launch)


def test_scheduled_frame_resumed_from_the_queue():
    """40 samples with a schedule forced on them: two first samples, the rest by kFastQueue on a resumed pass."""
    g = gpu("cornell_box", 40, 50, lane_stride=1, schedule=2)
    print("mode", g.mode)
    assert g.mode["fast_path"] == 1 and g.mode["scheduled"] == 1 and g.mode["first_pass_resumed"] == 1, g.mode
    assert g.mode["planned_chains"] == 0, g.mode
    assert_is_the_oracles(g, oracle("cornell_box", 40, 50), "resumed queue")


@pytest.mark.parametrize("launch", sorted(LAUNCHES))
def test_general_kernel_is_the_guard(launch):
    spp, opts = LAUNCHES[launch]
    g = gpu("cornell_box", spp, 50, fast_path=-1, **opts)
    assert_launch(g.mode, launch, fast=0)
    assert_is_the_oracles(g, oracle("cornell_box", spp, 50), "general kernel, " + launch)


@pytest.mark.parametrize("fast_path", [1, -1], ids=["fast", "general"])
def test_image_order_frame_is_one_launch(fast_path):
    """8 samples: no schedule, one launch that draws from the queue (fast: kFastQueue alone)."""
    g = gpu("cornell_box", 8, 50, lane_stride=1, fast_path=fast_path)
    assert g.mode["scheduled"] == 0 and g.mode["fast_path"] == (1 if fast_path == 1 else 0), g.mode
    assert_is_the_oracles(g, oracle("cornell_box", 8, 50), "image order")


@pytest.mark.parametrize("launch", sorted(LAUNCHES))
@pytest.mark.parametrize("depth", [1, 2])
def test_depth_limit_cuts_paths_that_owe(depth, launch):
    """Depth 1: every Lambertian bounce owes a normalisation and its path ends at the next hit.  The mark is cleared
    where the debt is paid, before that hit is looked at, so the lane's next sample starts at depth 0 without it."""
    spp, opts = LAUNCHES[launch]
    g = gpu("cornell_box", spp, depth, **opts)
    assert_launch(g.mode, launch)
    assert_is_the_oracles(g, oracle("cornell_box", spp, depth), "depth %d, %s" % (depth, launch))


# ------------------------------------------------------------------ lanes that never owe
def test_spheres_metal_and_dielectric_never_defer():
    """Metal with and without fuzz and dielectric beside Lambertian (a sphere scene: the general kernel)."""
    g = gpu("spheres", 16, 8)
    assert g.mode["fast_path"] == 0, g.mode
    assert_is_the_oracles(g, oracle("spheres", 16, 8), "spheres")


def test_fast_kernels_mix_lanes_that_owe_with_lanes_that_do_not():
    """The same materials on list triangles, where the fast kernels run: a wave holds Lambertian lanes that owe, metal
    and dielectric lanes that normalised once in their branch, and new camera rays."""
    g = gpu("mixed_list", 16, 8, lane_stride=1)
    assert g.mode["fast_path"] == 1, g.mode
    assert_is_the_oracles(g, oracle("mixed_list", 16, 8), "mixed list")


# ------------------------------------------------------------------ the slow form
@pytest.mark.parametrize("launch", sorted(LAUNCHES))
def test_one_camera_ray_sends_the_wave_through_the_ieee_forms(launch):
    """Some samples of one pixel have target - origin with v.v >= 2^100 (tests/test_deferred_normalise_host.py): in
    those iterations the whole wave, its Lambertian lanes that owe included, normalises by division and sqrtf."""
    spp, opts = LAUNCHES[launch]
    g = gpu("slow_camera", spp, 50, **opts)
    assert_launch(g.mode, launch)
    want = oracle("slow_camera", spp, 50)
    assert want.counts.min() >= spp * 2, "every path of this camera bounces off a wall"
    assert_is_the_oracles(g, want, "slow form, " + launch)


# ------------------------------------------------------------------ the caller-owned kernels
def test_budget_kernel_is_the_guard():
    """rtmi_render_budget on the frame, three samples everywhere, against the oracle replayed a sample at a time.  The
    trace, budget and feature kernels do not defer and compile to the instructions they had (NOTES.md, "Deferred
    normalisation": compared per symbol in both builds), so one of the three stands guard; tests/test_gpu_trace.py and
    tests/test_gpu_features.py hold the other two to the oracle as before."""
    budget = np.full(H * W, 3)
    got = Shards("cornell_box", 50, 3, 1, h=H, w=W).render_budget(budget).results()
    OracleReplay("cornell_box", 50, h=H, w=W).add(budget).assert_equal(got, "budget")
