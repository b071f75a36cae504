"""The fast list kernels' cull in centre / half-extent form (closest_hit.h: RTMI_CULL_SLAB) against the oracle, bit for bit.

The three kernels compiled for the common list frame test every pair of the world list against the PairSlab table: three
FMAs per axis, the distance slack in the table instead of per ray (tests/test_pair_slab_host.py holds the table to its
budget).  A cull may only drop pairs no triangle test could accept, so the image, the per-pixel ray counts, the final RNG
states and the ray total must be the oracle's: on the Cornell box, on lists of lone triangles and parallelograms, on
sheets that are all candidates of every ray, with an unbounded record, with direction components of zero, and from a
camera just inside the table's reach.  Just beyond it the library must pick the general kernel, which keeps the per-ray
slack.  Frames are 64 x 64 with lane_stride = 1; rtmi_render_mode says which kernel each call used and every case asserts
it (tests/test_gpu_deferred_normalise.py explains the two launches).  No tolerances anywhere.
"""
import functools
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import rtmi
import pair_slab_worlds as psw
from abi_host import CHECK_LIB, ROOT
from pair_slab_worlds import assert_launch
from parity import assert_same_frame, build_pair, gpu_frame, oracle_frame

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

H = W = psw.SIDE


@functools.lru_cache(maxsize=None)
def pair(world):
    fill, seed, _ = psw.WORLDS[world]
    return build_pair(lambda b: fill(b, W / H), seed)


@functools.lru_cache(maxsize=None)
def oracle(world, spp):
    """Computed once per frame, read by every case of it."""
    return oracle_frame(pair(world)[0], H, W, spp, psw.WORLDS[world][2])


def gpu(world, spp, **opts):
    return gpu_frame(pair(world)[1], H, W, spp, psw.WORLDS[world][2], opts=opts)


def assert_is_the_oracles(got, want, what):
    assert got.total > H * W, what  # the world is in view
    assert_same_frame(got, want, what)


FAST_WORLDS = ["cornell_box", "mixed_list", "sheets_4_light", "thin_pair", "axis_aligned", "inside_reach"]


@pytest.mark.parametrize("launch", sorted(psw.LAUNCHES))
@pytest.mark.parametrize("world", FAST_WORLDS)
def test_fast_kernels_cull_by_slab(world, launch):
    """queue: kFastQueue alone.  planned: kFastQueue for 32 samples, then kFastChains on the pass it left."""
    spp, opts = psw.LAUNCHES[launch]
    g = gpu(world, spp, **opts)
    print("mode", g.mode)
    assert_launch(g.mode, launch)
    assert_is_the_oracles(g, oracle(world, spp), "%s, %s" % (world, launch))


@pytest.mark.parametrize("launch", sorted(psw.LAUNCHES))
def test_camera_beyond_the_reach_gets_the_general_kernel(launch):
    """1.01 x kOriginReach x list_mag out: the table's slack no longer covers the camera rays' origins, the plan must
    say so (fast_path == 0) and the general kernel, with its per-ray slack, renders the oracle's frame."""
    spp, opts = psw.LAUNCHES[launch]
    g = gpu("beyond_reach", spp, **opts)
    print("mode", g.mode)
    assert_launch(g.mode, launch, fast=0)
    assert_is_the_oracles(g, oracle("beyond_reach", spp), "beyond reach, " + launch)


def test_camera_update_across_the_reach_changes_the_kernel():
    """The predicate is asked per launch of the scene's current camera: the same committed scene is a fast launch from
    inside the reach, a general one after rtmi_camera_update moved the camera beyond it, and a fast one again."""
    fill, seed, depth = psw.WORLDS["inside_reach"]
    b = rtmi.SceneBuilder(seed)
    fill(b, 1.0)
    b.commit()
    inside = b.camera_get().copy()
    tmp = rtmi.SceneBuilder(seed)
    psw.WORLDS["beyond_reach"][0](tmp, 1.0)
    beyond = tmp.camera_get().copy()
    R = rtmi.Renderer(b, H, W, 8, depth, True)
    ro = rtmi.render_opts(lane_stride=1)
    assert R.mode(ro)["fast_path"] == 1
    b.camera_update(beyond)
    assert R.mode(ro)["fast_path"] == 0
    b.camera_update(inside)
    assert R.mode(ro)["fast_path"] == 1


def test_the_worlds_are_what_the_cases_say():
    """Every pair of the sheets is a candidate of every camera ray; the thin pair's record is unbounded; the axis-aligned
    camera's rays have a y direction component of exactly zero; the far cameras see the box."""
    assert (oracle("sheets_4_light", 40).counts >= 40 * 5).all()
    fill, seed, _ = psw.WORLDS["thin_pair"]
    b = rtmi.SceneBuilder(seed)
    fill(b, 1.0)
    sl, _, _ = b.pair_slabs()
    assert (np.isinf(sl[:-1, 3:6]).all(axis=1)).sum() == 1
    # the axis-aligned camera: target - position in the binary32 operations of the camera ray, at both ends of the
    # jitter's range: y is zero for every pixel, x within a pixel of zero in the two central columns
    fill, seed, _ = psw.WORLDS["axis_aligned"]
    b = rtmi.SceneBuilder(seed)
    fill(b, 1.0)
    pos, llc, hor, ver = b.camera_get()[:4]
    F = np.float32
    for r in (F(2.0 ** -33), F(1.0)):
        f = (r + np.arange(W + 1, dtype=F)) * F(1.0 / W)
        d = ((llc[None, :] + f[:, None] * hor[None, :]).astype(F)[:, None, :] + f[None, :, None] * ver[None, None, :]).astype(F) - pos
        assert (d[..., 1] == 0).all() and (d[..., 2] == 800).all()
        assert np.abs(d[W // 2, :, 0]).max() <= 560.0 / W
    for world in ("inside_reach", "beyond_reach"):
        assert oracle(world, 40).counts.min() >= 2 * 40, world  # every path of these cameras bounces off a wall


def test_the_check_build_agrees_on_every_query():
    """librtmi_check1.so answers every query a second time with the plain, unculled scan (tests/pair_slab_check.py): the
    same worlds in both launches, every query re-done, no disagreement."""
    assert os.path.exists(CHECK_LIB), "librtmi_check1.so missing: run __graft_entry__.build() (make -C csrc check1)"
    env = dict(os.environ, RTMI_LIB_PATH=CHECK_LIB)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "pair_slab_check.py")], env=env, cwd=ROOT,
                       stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-4000:]
    out = json.loads(r.stdout[r.stdout.index("{"):])
    assert len(out) == 2 * len(psw.WORLDS), sorted(out)
    for tag, v in out.items():
        assert v["fast_path"] == (0 if tag.startswith("beyond_reach") else 1), (tag, v)
        assert v["re_done"] == v["rays"] > 0, (tag, v)
        assert v["disagreements"] == 0, (tag, v)
