"""Worlds and launches for the slab table of the fast list kernels (tests/test_pair_slab_host.py,
tests/test_gpu_pair_slab.py, tests/pair_slab_check.py).  Each `fill(b, aspect)` works on a product or an oracle builder.

The constants are those of ray-tracing-cuda_amd/csrc/margins.h, restated: the tests hold the library to the numbers, not
to its own header."""
import numpy as np

import tri_tasks_worlds as worlds
from rtmi import scenes
from tri_tasks_worlds import v3

EPS32 = 2.0 ** -24        # kEps32
DIST_SLACK = 2.0 ** -16   # kDistSlack
ORIGIN_REACH = 8.0        # kOriginReach
SLAB_ROUND_EPS = 8.0      # kSlabRoundEps
PAD_OF_EXTENT, PAD_OF_MAGNITUDE, PAD_FLOOR = 1e-4, 1e-5, 1e-30  # fixed_pad, in binary32 in the library

SIDE = 64
QUEUE = dict(lane_stride=1)  # one launch from the queue: kFastQueue
PLANNED = dict(lane_stride=1, schedule=2, plan=2, probe_spp=32)  # 32 samples from the queue, the rest kFastChains
LAUNCHES = {"queue": (40, QUEUE), "planned": (64, PLANNED)}


def assert_launch(mode, launch, fast=1):
    assert mode["fast_path"] == fast and mode["lane_stride"] == 1 and mode["wave_priority_every"] > 0, mode
    if launch == "queue":
        assert mode["scheduled"] == 0 and mode["planned_chains"] == 0, mode
    else:
        assert mode["scheduled"] == 1 and mode["first_pass_resumed"] == 1 and mode["planned_chains"] == 1, mode
        assert mode["first_pass_samples"] == 32, mode


def widening(list_mag):
    """delta_c + r_c: what a slab's half extent carries beyond the pair's padded bounds (binary64)."""
    return (DIST_SLACK + SLAB_ROUND_EPS * EPS32) * (ORIGIN_REACH + 1.0) * float(list_mag)


def cornell(b, aspect):
    scenes.cornell_box(b, aspect)


def mixed_list(b, aspect):
    worlds.mixed_list(7)(b)


def sheets_4_light(b, aspect):
    worlds.sheets(4, True)(b)


def thin_pair(b, aspect):
    """The mixed list and, in front of it, a lone triangle whose sharpest angle is 0.95 degrees -- below kThinSine, so
    that its pair is unbounded: a candidate of every ray."""
    worlds.mixed_list(7)(b)
    b.triangle([v3(-3, -1, 0.5), v3(3, -1, 0.5), v3(3, -0.9, 0.5)], b.lambertian(v3(0.3, 0.6, 0.4)))


def cornell_axis_aligned(b, aspect):
    """The Cornell box seen by a raw camera whose frame is axis-aligned and has no height: a slit at the camera's own
    y, so that EVERY camera ray has a y direction component of exactly zero, and the central columns an x component next
    to zero (a frame with height reaches an exact zero in its central pixels only when the jitter draws below 2^-19:
    once in 200 such frames).  The clamped reciprocals of 1e30 then meet k and tc at their largest, 2.8e32."""
    scenes.cornell_box(b, aspect)
    pos = np.array([278, 278, -800], dtype=np.float32)
    b.camera_raw(pos, np.array([-2, 278, 0], dtype=np.float32), np.array([560, 0, 0], dtype=np.float32),
                 np.array([0, 0, 0], dtype=np.float32))


def cornell_from(factor):
    """The Cornell box seen from the z axis, `factor` x kOriginReach x list_mag in front of it, through a frame that lies
    inside the box's opening."""
    def fill(b, aspect):
        scenes.cornell_box(b, aspect)
        mag = cornell_list_mag()
        z = np.float32(-factor * ORIGIN_REACH * mag)
        pos = np.array([278, 278, z], dtype=np.float32)
        half = np.float32(270.0)  # inside the box's opening, 555 wide, at z = 0: every camera ray enters the box
        b.camera_raw(pos, np.array([278 - half, 278 - half, 0], dtype=np.float32), np.array([2 * half, 0, 0], dtype=np.float32),
                     np.array([0, 2 * half, 0], dtype=np.float32))
    return fill


def cornell_list_mag():
    import rtmi
    b = rtmi.SceneBuilder(1024)
    scenes.cornell_box(b, 1.0)
    return b.pair_slabs()[2]


WORLDS = {"cornell_box": (cornell, scenes.SCENE_SEEDS.get("cornell_box", 1024), 50),
          "mixed_list": (mixed_list, 7, 8),
          "sheets_4_light": (sheets_4_light, 7, 8),
          "thin_pair": (thin_pair, 7, 8),
          "axis_aligned": (cornell_axis_aligned, 1024, 50),
          "inside_reach": (cornell_from(0.99), 1024, 50),
          "beyond_reach": (cornell_from(1.01), 1024, 50)}
