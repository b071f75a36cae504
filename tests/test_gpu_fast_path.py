"""The list kernel's compile-time fast path (kernels.h: the mode word; render_body.h) against the general kernel.

A launch of a list-triangle scene whose run-time modes are all the common ones runs a kernel compiled for exactly those
modes.  Nothing about a pixel may depend on which kernel rendered it: for the Cornell box and a random list-triangle scene
of at most 16 materials, on power-of-two frames rendered as planned chains, from the queue and in image order, the image,
the per-pixel ray counts, the final RNG states and the ray total are bit-identical with the fast path on and forced off,
and rtmi_render_mode reports which kernel it was.  Launches outside the pinned modes -- 17 materials, a signed colour, a
frame that is no power of two, a thin frame, a sphere, priorities off -- report the general kernel and match the oracle.
"""
import numpy as np
import pytest

import oraclelib
import rtmi
from rtmi import scenes
from rtmi.scenes import v3, PI_D

pytestmark = pytest.mark.gpu


def cornell(b, aspect):
    scenes.cornell_box(b, aspect)


def random_list(n_mats=12, signed=False, sphere=False):
    """A world list of parallelograms, boxes and lone triangles with n_mats materials, every one of them used."""
    def fill(b, aspect):
        rng = np.random.default_rng(77)
        b.camera_pinhole(v3(0, 1.0, 3.0), v3(0, 0.6, -1), v3(0, 1, 0), PI_D / 3, aspect)
        mats = [b.metal(v3(0.8, 0.8, 0.7), 0.0), b.metal(v3(0.7, 0.8, 0.9), 0.3), b.dielectric(v3(1, 1, 1), 1.5),
                b.diffuse_light(b.constant_texture(v3(3, 3, 3)))]
        first = v3(-0.4, 0.5, 0.6) if signed else v3(0.4, 0.5, 0.6)
        mats += [b.lambertian(first)] + [b.lambertian(v3(*rng.uniform(0.2, 0.9, 3))) for _ in range(n_mats - 5)]
        assert len(mats) == n_mats
        for i in range(max(n_mats, 14)):
            c = np.array([rng.uniform(-2.0, 2.0), rng.uniform(0.0, 1.8), rng.uniform(-3.5, -0.5)])
            m = mats[4 + i % (n_mats - 4)] if i >= 3 else mats[i]
            if i % 5 == 4:
                e = rng.uniform(0.2, 0.5, 3)
                b.parallelepiped([v3(*c), v3(c[0] + e[0], c[1], c[2]), v3(c[0], c[1] + e[1], c[2]), v3(c[0], c[1], c[2] + e[2])], m)
            elif i % 5 == 3:
                b.triangle([v3(*c), v3(*(c + rng.uniform(-0.5, 0.5, 3))), v3(*(c + rng.uniform(-0.5, 0.5, 3)))], m)
            else:
                b.parallelogram([v3(*c), v3(*(c + rng.uniform(-0.5, 0.5, 3))), v3(*(c + rng.uniform(-0.5, 0.5, 3)))], m)
        if sphere:
            b.sphere(v3(0.3, 0.5, -1.2), 0.5, mats[5])
        b.parallelogram([v3(-3, -0.01, -5), v3(3, -0.01, -5), v3(-3, -0.01, 1)], mats[4])
        b.parallelogram([v3(-1, 3.2, -3), v3(1, 3.2, -3), v3(-1, 3.2, -1)], mats[3])
        b.sky()
    return fill


def gpu(fill, h, w, spp, depth, **opts):
    """(image, per-pixel ray counts, final RNG states, ray total, mode) of one render through the C ABI."""
    import torch
    b = rtmi.SceneBuilder(11)
    fill(b, w / h)
    b.commit()
    R = rtmi.Renderer(b, h, w, spp, depth, True).init_rng()
    ro = rtmi.render_opts(**opts)
    R.render(opts=ro)
    R.check()
    img, cnt = R.untile()
    torch.cuda.synchronize()
    return img.cpu().numpy(), cnt.cpu().numpy().astype(np.uint32), R.states.cpu().numpy(), R.total_rays(), R.mode(ro)


def oracle(fill, h, w, spp, depth):
    b = oraclelib.OracleBuilder(11)
    fill(b, w / h)
    rgb, rays, _, total = b.render(h, w, spp, depth, post=True)
    return rgb, rays, total


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
    fast = gpu(fill, h, w, spp, depth, fast_path=1, **opts)
    general = gpu(fill, h, w, spp, depth, fast_path=-1, **opts)
    assert fast[4]["fast_path"] == 1 and general[4]["fast_path"] == 0, (fast[4], general[4])
    for k, v in want_mode.items():
        assert fast[4][k] == v and general[4][k] == v, (k, fast[4], general[4])
    assert fast[4]["lane_stride"] == 1 and fast[4]["wave_priority_every"] > 0
    assert {k: v for k, v in fast[4].items() if k != "fast_path"} == {k: v for k, v in general[4].items() if k != "fast_path"}
    assert fast[3] == general[3], "ray totals %d vs %d" % (fast[3], general[3])
    assert fast[3] > h * w * spp  # the scene is in view
    assert np.array_equal(fast[1], general[1]), "%d pixels with different ray counts" % (fast[1] != general[1]).sum()
    assert np.array_equal(fast[2], general[2]), "final RNG states differ"
    assert np.array_equal(fast[0].view(np.uint32), general[0].view(np.uint32)), np.abs(fast[0] - general[0]).max()


def test_default_is_the_fast_path_and_it_matches_the_oracle():
    """No option named: the fast kernel, and its frame is the oracle's bit for bit."""
    fill = random_list()
    g = gpu(fill, 32, 64, 8, 12, lane_stride=1)
    assert g[4]["fast_path"] == 1, g[4]
    o = oracle(fill, 32, 64, 8, 12)
    assert g[3] == o[2] and np.array_equal(g[1], o[1]) and np.array_equal(g[0], o[0], equal_nan=True)


NEGATIVE = [("17_materials", random_list(n_mats=17), 32, 64, dict(lane_stride=1)),
            ("signed_colour", random_list(signed=True), 32, 64, dict(lane_stride=1)),
            ("not_a_power_of_two", random_list(), 24, 40, dict(lane_stride=1)),
            ("thin_frame", random_list(), 32, 64, dict()),
            ("sphere", random_list(sphere=True), 32, 64, dict(lane_stride=1)),
            ("priorities_off", random_list(), 32, 64, dict(lane_stride=1, wave_priority=0))]


@pytest.mark.parametrize("case", NEGATIVE, ids=[c[0] for c in NEGATIVE])
def test_launches_outside_the_pinned_modes_use_the_general_kernel(case):
    """Each case differs from test_default_is_the_fast_path_and_it_matches_the_oracle's launch in the one thing it is
    named after; asked for the fast path, it reports the general kernel and renders the oracle's frame."""
    name, fill, h, w, opts = case
    g = gpu(fill, h, w, 8, 12, fast_path=1, **opts)
    assert g[4]["fast_path"] == 0, g[4]
    if name == "thin_frame":
        assert g[4]["lane_stride"] > 1, g[4]
    else:
        assert g[4]["lane_stride"] == 1, g[4]
    assert (g[4]["wave_priority_every"] == 0) == (name == "priorities_off"), g[4]
    o = oracle(fill, h, w, 8, 12)
    assert g[3] == o[2], "ray totals %d vs %d" % (g[3], o[2])
    assert np.array_equal(g[1], o[1]), "%d pixels with different ray counts" % (g[1] != o[1]).sum()
    assert np.array_equal(g[0], o[0], equal_nan=True), np.abs(g[0] - o[0]).max()
