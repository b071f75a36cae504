"""Parity cases added in round 3 (all through the C ABI, against the oracle):
  * the raw-frame Camera constructor (camera.cu:40-47) on the GPU path;
  * world lists long enough to leave the first 32-pair chunk of the culled scan, to fill its LDS staging (128 pairs)
    and to fall back to the plain scan beyond it -- with coincident entries for the tie rules (hitable_list.cu:18),
    flat and through nested lists whose flattened length crosses those limits;
  * the triangle-soup worlds of the round-2 fuzz campaign (tools/gpu_fuzz.py) that once overran the wave-wide
    search stack (gpurun_out/r02b_fuzz.log: a GPU memory fault within the first 400 soups), as a regression;
  * two renders of ONE scene in flight on two streams, each with its own rtmi_render_opts.d_scratch;
  * rtmi_render_status / rtmi_gather (one rank).
"""
import ctypes as C

import numpy as np
import pytest

import rtmi
from parity import assert_same_frame, build_pair, gpu_frame, oracle_frame
from rtmi.scenes import v3, PI_D
from worlds import (_quilt, far_sphere_cloud, far_view_world, grazing_world, needle_list_world, needle_world, sliver_fan,
                    soup_world)

pytestmark = pytest.mark.gpu


def render_pair(fill, h, w, spp, depth, post=True, seed=11, camera=None, opts=None):
    """The same world on the product and on the oracle, a frame of each: (gpu, oracle).  `opts`: a dict of
    rtmi.render_opts arguments for the product's render."""
    if camera is None:
        camera = lambda b: b.camera_pinhole(v3(0, 1.0, 3.0), v3(0, 0.6, -1), v3(0, 1, 0), PI_D / 3, w / h)
    ob, pb = build_pair(fill, seed, camera)
    return gpu_frame(pb, h, w, spp, depth, post, opts), oracle_frame(ob, h, w, spp, depth, post)


def assert_same(g, o, what="frame"):
    """NaN-tolerant, as this file always compared: a NaN must sit in the same pixel channel of both frames."""
    assert_same_frame(g, o, what, nan_ok=True)


# ------------------------------------------------------------------ camera.cu:40-47
def test_raw_frame_camera_on_the_gpu_path():
    """Camera(position, lower_left_corner, horizontal, vertical): the scene supplies the frame itself; u, v, w stay
    unset and RayAt only reads the four vectors (camera.cu:40-47, 57-70).  An off-axis, sheared frame."""
    def cam(b):
        b.camera_raw(v3(0.3, 1.2, 3.0), v3(-2.1, -0.9, 0.4), v3(4.0, 0.3, -0.2), v3(0.25, 2.6, 0.1))

    def fill(b):
        b.sphere(v3(0, -100.5, -1), 100.0, b.lambertian(v3(0.5, 0.6, 0.4)))
        b.sphere(v3(0, 0.5, -1), 0.5, b.metal(v3(0.8, 0.8, 0.9), 0.05))
        b.parallelepiped([v3(-1.6, 0, -1.2), v3(-0.9, 0, -1.2), v3(-1.6, 0.8, -1.2), v3(-1.6, 0, -0.5)], b.lambertian(v3(0.7, 0.3, 0.3)))
        b.parallelogram([v3(-1, 3, -2), v3(1, 3, -2), v3(-1, 3, 0)], b.diffuse_light(b.constant_texture(v3(4, 4, 4))))
        b.sky()
    g, o = render_pair(fill, 36, 52, 4, 10, camera=cam)
    assert_same(g, o)
    assert o.total > 36 * 52 * 4 * 1.5  # the scene is in view


@pytest.mark.parametrize("n,boxes_every", [(34, 0), (40, 0), (100, 0), (108, 0), (140, 0), (30, 3), (300, 5)])
def test_long_world_lists_match_the_full_scan(n, boxes_every):
    """34 / 40 entries (+ duplicates, floor, light): past the first 32-pair chunk of the culled scan; 100 / 108:
    several chunks, up to its 128-pair LDS staging; 140 / 300 (with boxes: ~650 pairs): beyond it, the plain
    wave-uniform walk.  Duplicated entries make equal-t ties within and across chunks."""
    state = np.random.default_rng(4000 + n + boxes_every).bit_generator.state

    def fill(b):
        rng = np.random.default_rng(0)
        rng.bit_generator.state = state
        _quilt(b, n, rng, boxes_every)
    g, o = render_pair(fill, 40, 56, 3, 12)
    assert_same(g, o)


@pytest.mark.parametrize("per_list", [30, 50])
def test_nested_lists_whose_flattened_length_crosses_the_staging_limit(per_list):
    """Three stretches of `per_list` parallelograms in HitableLists nested two deep, plus top-level entries: 95 pairs
    (inside the culled scan's staging) and 155 (outside: plain walk); hitable_list.cuh:8."""
    state = np.random.default_rng(77 + per_list).bit_generator.state

    def fill(b):
        rng = np.random.default_rng(0)
        rng.bit_generator.state = state
        mats = [b.lambertian(v3(*rng.uniform(0.2, 0.9, 3))) for _ in range(4)] + [b.metal(v3(0.9, 0.9, 0.9), 0.1)]

        def pg():
            c = np.array([rng.uniform(-2, 2), rng.uniform(0, 1.8), rng.uniform(-3.5, -0.5)])
            b.parallelogram([v3(*c), v3(*(c + rng.uniform(-0.4, 0.4, 3))), v3(*(c + rng.uniform(-0.4, 0.4, 3)))],
                            mats[int(rng.integers(0, len(mats)))])
        b.sky()
        b.list_begin()
        for _ in range(per_list):
            pg()
        b.list_begin()
        for _ in range(per_list):
            pg()
        b.list_end()
        for _ in range(per_list):
            pg()
        b.list_end()
        for _ in range(4):
            pg()
        b.parallelogram([v3(-1, 3.2, -3), v3(1, 3.2, -3), v3(-1, 3.2, -1)], b.diffuse_light(b.constant_texture(v3(3, 3, 3))))
    g, o = render_pair(fill, 36, 48, 3, 10)
    assert_same(g, o)


def test_triangle_soups_of_the_round_2_campaign():
    """Soup seeds 0..399 in one go (the campaign that produced the recorded fault ran `gpu_fuzz.py 0 300 400`): every
    k_min class (1, 2, 3, 8, 64, 2048), duplicated faces, dielectrics of index 1 that pass straight through tens of
    faces.  No abandoned search (rtmi_render_status inside Renderer.untile / total_rays) and no differing pixel."""
    bad = []
    classes = set()
    for seed in range(400):
        fill, h, w, spp, depth, what = soup_world(seed)
        classes.update(k for _, k, _ in what)
        g, o = render_pair(fill, h, w, spp, depth, post=False, seed=300 + seed,
                           camera=lambda b, a=w / h: b.camera_pinhole(v3(0, 0.8, 1.8), v3(0, 0.4, -2), v3(0, 1, 0), PI_D / 3, a))
        try:
            assert_same(g, o, "soup %d" % seed)
        except AssertionError as e:
            bad.append((str(e), what))
    assert classes == {1, 2, 3, 8, 64, 2048}
    assert not bad, bad[:5]


# ------------------------------------------------------------------ two renders of one scene in flight
def test_two_streams_render_one_scene_concurrently():
    """rtmi_render_opts.d_scratch holds ALL per-call state (queue cursors, ray total, completion flag, scheduler
    buffers): two shards of one committed scene rendered on two streams at once, longest-first scheduling forced,
    equal what each gives alone -- image, ray counts, ray totals."""
    import torch
    import common
    h = w = 96
    spp, depth = 64, 12
    b = common.build_scene(rtmi.SceneBuilder(1024), "cornell_box", 1.0).commit()
    alone = []
    for r in range(2):
        R = rtmi.Renderer(b, h, w, spp, depth, True, rank=r, world_size=2).init_rng()
        R.render(opts=rtmi.render_opts(schedule=2))
        torch.cuda.synchronize()
        alone.append((R.tiles.clone(), R.ray_counts.clone(), R.total_rays()))
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    Rs, scratch = [], []
    for r in range(2):
        R = rtmi.Renderer(b, h, w, spp, depth, True, rank=r, world_size=2).init_rng()
        Rs.append(R)
        scratch.append(R.new_scratch())
    torch.cuda.synchronize()
    for _ in range(3):  # several rounds: the two launches overlap in some of them at least
        for r in range(2):
            with torch.cuda.stream(streams[r]):
                Rs[r].init_rng()
                Rs[r].render(opts=rtmi.render_opts(schedule=2, scratch=scratch[r]))
        torch.cuda.synchronize()
        for r in range(2):
            assert Rs[r].total_rays(scratch[r]) == alone[r][2]
            assert torch.equal(Rs[r].ray_counts, alone[r][1])
            assert torch.equal(Rs[r].tiles, alone[r][0])
    # a scratch that is too small is refused before anything is launched
    small = torch.zeros(64, dtype=torch.int64, device="cuda")
    with pytest.raises(rtmi.RtmiError):
        Rs[0].render(opts=rtmi.render_opts(scratch=small))


def test_render_status_and_single_rank_gather():
    import torch
    import common
    L = rtmi.lib()
    b = common.build_scene(rtmi.SceneBuilder(1024), "cornell_box", 1.0).commit()
    R = rtmi.Renderer(b, 24, 24, 2, 5).init_rng()
    R.render()
    rays = C.c_uint64(0)
    assert L.rtmi_render_status(b.h, None, C.byref(rays), None) == 0 and rays.value == R.total_rays() > 0
    assert L.rtmi_render_status(b.h, None, None, None) == 0  # the ray total is optional
    # world_size 1: rtmi_gather is the device copy into the root's buffer, no communicator needed
    allt = torch.full_like(R.tiles, -1.0)
    assert L.rtmi_gather(None, C.byref(R.frame), C.c_void_p(R.tiles.data_ptr()), C.c_void_p(allt.data_ptr()), 0, None) == 0
    torch.cuda.synchronize()
    assert torch.equal(allt, R.tiles)
    two = rtmi.make_frame(24, 24, 2, 5, rank=0, world_size=2)
    assert L.rtmi_gather(None, C.byref(two), C.c_void_p(R.tiles.data_ptr()), C.c_void_p(allt.data_ptr()), 0, None) == -1
    assert b"communicator" in L.rtmi_last_error()
    assert L.rtmi_reduce_sum(None, C.byref(R.frame), C.c_void_p(R.tiles.data_ptr()), 0, None) == 0


def test_a_frame_whose_pixels_could_overrun_their_query_counter_is_refused():
    """A pixel's closest-hit queries -- at most max_depth + 1 per sample (ray_tracing.cu:22-26) -- are counted in 31 bits
    (bit 31 of its ray_counts word is the scheduler's mark): rtmi_render refuses spp * (max_depth + 1) > 2^31 - 1 and says
    why, instead of wrapping the counter (the reference counts nothing; include/rtmi.h: RTMI_MAX_PIXEL_QUERIES)."""
    import common
    import os
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "rtmi.h")).read()
    assert "#define RTMI_MAX_PIXEL_QUERIES 2147483647" in hdr
    L = rtmi.lib()
    b = common.build_scene(rtmi.SceneBuilder(1024), "cornell_box", 1.0).commit()
    for spp, depth in (((1 << 31) - 1, 1), ((1 << 31) // 11 + 1, 10), ((1 << 31) // 65 + 1, 64)):
        R = rtmi.Renderer(b, 8, 8, spp, depth).init_rng()
        with pytest.raises(Exception):
            R.render()
        assert b"RTMI_MAX_PIXEL_QUERIES" in L.rtmi_last_error()
    R = rtmi.Renderer(b, 8, 8, 3, 64).init_rng()  # (the deepest legal depth renders)
    R.render()
    assert R.total_rays() > 0


# ------------------------------------------------------------------ long sphere runs (grouped scan)
@pytest.mark.parametrize("n,seed", [(32, 0), (33, 1), (100, 2), (257, 3), (700, 4)])
def test_long_sphere_runs_match_the_full_scan(n, seed):
    """Stretches of 32 or more consecutive spheres go through the grouped scan (closest_hit.h): spatial groups of
    16, per-lane pre-test, shared binary64 tests, an order-free fold -- smallest accepted t, FIRST in list order among
    equal ones (hitable_list.cu:18).  Clouds with verbatim duplicates (equal t from different list positions),
    concentric shells (far roots: rays that start inside a sphere, sphere.cu:32-38), glass and mirrors that send
    rays back through the cloud from the far side, two runs separated by a parallelogram, and a camera INSIDE one of
    the spheres."""
    state = np.random.default_rng(9000 + seed).bit_generator.state

    def fill(b):
        rng = np.random.default_rng(0)
        rng.bit_generator.state = state
        mats = [b.lambertian(v3(*rng.uniform(0.2, 0.9, 3))) for _ in range(4)] + \
               [b.metal(v3(0.85, 0.85, 0.8), 0.0), b.metal(v3(0.7, 0.8, 0.9), 0.4), b.dielectric(v3(1, 1, 1), 1.5),
                b.dielectric(v3(0.95, 1, 0.95), 1.0), b.diffuse_light(b.constant_texture(v3(2.5, 2.5, 2.5)))]
        b.sphere(v3(0, -1000.0, 0), 1000.0, mats[0])
        made = []
        half = n // 2
        for i in range(n):
            if i == half:
                b.parallelogram([v3(-2, 0.0, -4.5), v3(2, 0.0, -4.5), v3(-2, 2.5, -4.5)], mats[4])  # splits the run
            k = rng.integers(0, 10)
            if k == 0 and made:  # verbatim duplicate with another material: equal roots, the first must win
                c, r = made[int(rng.integers(0, len(made)))]
            elif k == 1 and made:  # concentric shell around an earlier sphere
                c, r0 = made[int(rng.integers(0, len(made)))]
                r = r0 * float(rng.uniform(1.05, 1.6))
            else:
                c = np.array([rng.uniform(-2.5, 2.5), rng.uniform(0.1, 2.2), rng.uniform(-4.0, 1.0)])
                r = float(rng.uniform(0.05, 0.35))
            made.append((c, r))
            b.sphere(v3(*c), r, mats[int(rng.integers(0, len(mats)))])
        b.sphere(v3(0, 1.0, 3.0), 0.6, mats[7])  # the camera sits inside this one (index-1 glass)
        b.sky()
    g, o = render_pair(fill, 40, 56, 3, 12)
    assert_same(g, o)


def test_a_ray_through_more_spheres_than_candidate_slots():
    """48 concentric shells (and 40 more spheres elsewhere, so that the run is grouped): every ray towards the centre
    passes through all of them -- more candidates than a lane's 16 slots -- and its wave answers the run with the
    plain loop instead (closest_hit.h: `overflowed`)."""
    def fill(b):
        rng = np.random.default_rng(5)
        glass = b.dielectric(v3(1, 1, 1), 1.0)   # index 1: rays go straight through every shell
        tint = b.dielectric(v3(0.97, 0.99, 0.97), 1.0)
        core = b.lambertian(v3(0.8, 0.3, 0.2))
        for k in range(48):
            b.sphere(v3(0, 1.0, -1.5), 0.25 + 0.02 * k, tint if k % 3 else glass)
        b.sphere(v3(0, 1.0, -1.5), 0.2, core)
        for _ in range(40):
            b.sphere(v3(rng.uniform(-2.5, 2.5), rng.uniform(0.1, 2.0), rng.uniform(-4, 0)), float(rng.uniform(0.05, 0.2)),
                     b.lambertian(v3(*rng.uniform(0.2, 0.9, 3))))
        b.sphere(v3(0, -1000.0, 0), 1000.0, b.lambertian(v3(0.5, 0.5, 0.5)))
        b.sky()
    g, o = render_pair(fill, 32, 40, 2, 60)
    assert_same(g, o)


@pytest.mark.parametrize("angle", [5.0, 1.4, 0.5, 0.1])
@pytest.mark.parametrize("dist", [1e2, 1e3, 4e3, 2e4])
def test_far_false_accepts_outside_their_leaf_box(angle, dist):
    """Millimetre slivers (apex angles from 5 degrees down to 0.1) seen from 1e2 .. 2e4 away, the mesh FIRST in the
    world list (t_to is still +infinity when BVH::Hit is entered) and reference leaves of 8 faces.  From that far the
    binary32 triangle test (utils.cu:49-85) accepts rays that pass a sliver at many times its width -- streaks tens of
    pixels long -- but the reference only reports such a face if the ray also crosses the exact, unpadded boxes on the
    way to its leaf (bvh.cu:6-30), which such a ray usually does not.  The search must find the face (distance
    slack of the search boxes), and the replay of the reference's box tests must then drop it: a box none of whose
    planes qualifies has no crossing time, whatever t_to is (the round-3 fix in aabb_crossing_time).
    Documents the sliver regime as well: at these angles and distances the frames still agree bit for bit."""
    faces = sliver_fan(angle)
    h, w, spp, depth = 48, 64, 2, 3

    def fill(b):
        pos = v3(0.3 * dist * 0.01, dist * np.sin(0.6), dist * np.cos(0.6))
        b.camera_pinhole(pos, v3(0.0, 0, 0.0), v3(0, 1, 0), float(2.0 * np.arctan(0.03 / dist)), w / h)
        b.bvh(faces, b.lambertian(v3(0.8, 0.8, 0.8)), k_min=8)
        b.sky()
    ob, pb = build_pair(fill, 9)
    assert_same(gpu_frame(pb, h, w, spp, depth), oracle_frame(ob, h, w, spp, depth), "angle %g from %g" % (angle, dist))


def test_far_views_and_thin_faces():
    """Far-view worlds 0..299 of the fuzz campaign, bit for bit -- and the worlds in which thin faces once slipped through
    the search: seeds 1527, 1674, 1675, 1774 (0.6-degree slivers of 6 .. 25 mm seen from 60 .. 800 away: the binary32
    triangle test's false accepts reach further from such a face than the 2^-16 distance slack of the search boxes;
    until round 3 these four differed on a handful of pixels and were the documented limit of the exactness claim).
    Every node of the search tree now widens its children's boxes by what the thinnest face below it asks for
    (scene.hip: face_slack_exponent, QNode4::slack_exp)."""
    for seed in list(range(300)) + [1527, 1674, 1675, 1774]:
        fill, cam, h, w, spp, depth, what = far_view_world(seed)
        g, o = render_pair(fill, h, w, spp, depth, post=False, seed=500 + seed, camera=cam)
        assert_same(g, o, (seed, what))


def test_needles_and_grazing_views_match_the_oracle():
    """Needles (smallest angles of 0.5 .. 0.005 degrees, faces up to a metre) and sheets seen from a fraction of a degree
    above their plane, from 10 .. 1e4 away.  The needle seeds are worlds in which the every-query margin check
    (tools/gpu_check_margins.py meshes, -DRTMI_CHECK_MARGINS -DRTMI_CHECK_EVERY=1) found rays the search had lost before
    the nodes carried their slack exponent (40 of 1,500 worlds; 0 with it)."""
    for seed in (9, 120, 199, 224, 253, 322, 329, 336, 354, 367) + tuple(range(20)):
        fill, h, w, spp, depth = needle_world(seed)
        g, o = render_pair(lambda b: fill(b), h, w, spp, depth, post=False, seed=500 + seed, camera=lambda b: None)
        assert_same(g, o, ("needle", seed))
    for seed in range(30):
        fill, h, w, spp, depth = grazing_world(seed)
        g, o = render_pair(lambda b: fill(b), h, w, spp, depth, post=False, seed=500 + seed, camera=lambda b: None)
        assert_same(g, o, ("grazing", seed))


def test_thin_world_list_triangles_and_far_sphere_clouds_match_the_oracle():
    """The needles as Triangle / Parallelogram hitables of the world list: the culled list scan never culls a pair
    thinner than 1.8 degrees (scene.hip: push_pair) -- with padded bounds like any other pair's, 128 of 1,500 such
    worlds had rays the scan lost (the seeds below are ten of them).  And sphere clouds from 10 .. 2e4 away (the grouped
    sphere scan's margins: 0 of 1,500 worlds disagreed in the every-query check)."""
    for seed in (9, 10, 36, 38, 57, 86, 120, 122, 138, 156) + tuple(range(200, 210)):
        fill, h, w, spp, depth = needle_list_world(seed)
        g, o = render_pair(lambda b: fill(b), h, w, spp, depth, post=False, seed=500 + seed, camera=lambda b: None)
        assert_same(g, o, ("needle list", seed))
    for seed in range(16):
        fill, h, w, spp, depth = far_sphere_cloud(seed)
        g, o = render_pair(lambda b: fill(b), h, w, spp, depth, post=False, seed=500 + seed, camera=lambda b: None)
        assert_same(g, o, ("sphere cloud", seed))


def test_adversarial_worlds_on_the_scheduled_paths_match_the_oracle():
    """The culled scans share their candidate tests across a wave, so which rays share one matters; the worlds above are
    small enough that the default renders them in one unscheduled launch.  Here seeds of every family go through
    the scheduled paths: resumed after a first pass (mesh frames: the head's pixel weight classes), and in a mode of
    other wave shapes -- mesh frames: the head's outlier tiles one pixel to a wave (sparse_stride=64); list frames: one
    pixel per 16 lanes.  Bit for bit against the oracle, and every render resumed."""
    mesh_modes = (dict(schedule=2), dict(schedule=2, sparse_stride=64))
    list_modes = (dict(schedule=2), dict(schedule=2, lane_stride=16))

    def check(what, seed, fill, h, w, spp, depth, modes, camera=lambda b: None):
        for kw in modes:
            g, o = render_pair(fill, h, w, max(spp, 4), depth, post=False, seed=500 + seed, camera=camera, opts=kw)
            assert g.mode["first_pass_resumed"] == 1, (what, seed, kw, g.mode)
            assert_same(g, o, (what, seed, kw))

    for seed in tuple(range(20)) + (1527, 1674, 1675, 1774):  # (the known sliver cases last)
        fill, cam, h, w, spp, depth, what = far_view_world(seed)
        check("far view", seed, fill, h, w, spp, depth, mesh_modes, camera=cam)
    for seed in (9, 120, 199, 224, 253) + tuple(range(10)):
        fill, h, w, spp, depth = needle_world(seed)
        check("needle", seed, fill, h, w, spp, depth, mesh_modes)
    for seed in range(15):
        fill, h, w, spp, depth = grazing_world(seed)
        check("grazing", seed, fill, h, w, spp, depth, mesh_modes)
    for seed in (9, 10, 36, 38, 57, 86, 120, 122, 138, 156) + tuple(range(200, 205)):
        fill, h, w, spp, depth = needle_list_world(seed)
        check("needle list", seed, fill, h, w, spp, depth, list_modes)
    for seed in range(10):
        fill, h, w, spp, depth = far_sphere_cloud(seed)
        check("sphere cloud", seed, fill, h, w, spp, depth, list_modes)


def test_scheduling_modes_do_not_change_a_bit():
    """Round 4's scheduling -- wave priorities (longest remaining chain first within a SIMD), planned tile chains with
    tile claims and take-over, thin frames (one pixel per 2..16 lanes) -- only decides which lane renders which pixel
    when: image, per-pixel ray counts, final RNG states and the ray total are those of the plain queue, bit for bit.
    List scenes (cornell: culled pair scan; spheres: grouped scan) and a mesh scene (priorities only)."""
    import common
    cases = (("cornell_box", 256, 256, 64, 12), ("spheres", 128, 160, 64, 8), ("bunny", 96, 96, 64, 10))
    modes = (dict(schedule=0, plan=0, wave_priority=0, lane_stride=1),  # the plain queue, image order
             dict(schedule=2, plan=0, wave_priority=0, lane_stride=1),  # longest-first queue
             dict(schedule=2, plan=0, wave_priority=16, lane_stride=1),  # + priorities
             dict(schedule=2, plan=2, wave_priority=16, lane_stride=1),  # planned chains
             dict(schedule=2, plan=2, wave_priority=1, lane_stride=1, blocks_per_cu=1),  # chains of many tiles, one workgroup per CU
             dict(schedule=2, plan=2, wave_priority=64, lane_stride=1, probe_spp=1),
             dict(schedule=0, plan=0, wave_priority=4, lane_stride=4),  # thin
             dict(schedule=2, plan=2, wave_priority=16, lane_stride=16),  # thin (the plan gives way to the queue)
             dict(schedule=2, plan=2, wave_priority=16, lane_stride=1, first_pass=0),  # a discarded probe instead of a first pass
             dict(schedule=2, plan=0, wave_priority=16, lane_stride=1, first_pass=4, probe_spp=0),  # a quarter of the samples first
             dict(schedule=2, plan=2, wave_priority=16, lane_stride=1, first_pass=1, probe_spp=63),
             dict())  # the defaults
    for name, h, w, spp, depth in cases:
        b = common.build_scene(rtmi.SceneBuilder(common.scene_seed(name)), name, w / h).commit()
        want = None
        for kw in modes:
            R = rtmi.Renderer(b, h, w, spp, depth, True).init_rng()
            R.render(opts=rtmi.render_opts(**kw))
            R.check()
            got = (R.tiles.cpu().numpy(), R.ray_counts.cpu().numpy(), R.states.cpu().numpy(), R.total_rays())
            if want is None:
                want = got
                assert got[3] > h * w * spp
                continue
            assert got[3] == want[3], (name, kw)
            for x, y in zip(got[:3], want[:3]):
                assert np.array_equal(x, y), (name, kw)


def test_the_queue_drawn_in_batches_renders_every_pixel_once():
    """List frames take their work items from the queue a batch per WAVE and atomic (render_body.h: up to 64 in a first
    pass of a few samples, up to 16 in longest-first order, fewer towards the end of the queue, the waiting lanes only in
    image order).  Ragged frames (padding items inside the batches), shards, a grid of one workgroup per CU (hundreds of
    items per wave: full batches) and of one block only: same image, ray counts and RNG states as the image-order queue."""
    import common
    cases = (("cornell_box", 250, 203, 40, 12, 0, 1), ("spheres", 264, 200, 36, 8, 0, 1), ("cornell_box", 333, 517, 33, 6, 1, 3),
             ("birthday", 200, 264, 34, 10, 2, 3))
    modes = (dict(schedule=0, wave_priority=0), dict(schedule=2, plan=0), dict(schedule=2, plan=0, blocks_per_cu=1),
             dict(schedule=2, plan=0, blocks_per_cu=1, probe_spp=1), dict(schedule=2, plan=0, blocks_per_cu=1, first_pass=0),
             dict(schedule=2, plan=0, blocks_per_cu=1, threads_per_block=64), dict())
    for name, h, w, spp, depth, rank, world in cases:
        b = common.build_scene(rtmi.SceneBuilder(common.scene_seed(name)), name, w / h).commit()
        want = None
        for kw in modes:
            R = rtmi.Renderer(b, h, w, spp, depth, True, rank=rank, world_size=world).init_rng()
            R.render(opts=rtmi.render_opts(**kw))
            R.check()
            got = (R.tiles.cpu().numpy(), R.ray_counts.cpu().numpy(), R.states.cpu().numpy(), R.total_rays())
            if want is None:
                want = got
                assert got[3] > (h * w // world) * spp // 2
                continue
            assert got[3] == want[3], (name, kw)
            for x, y in zip(got[:3], want[:3]):
                assert np.array_equal(x, y, equal_nan=True), (name, kw)


def test_bench_shard_and_sweep_paths():
    """bench.py --shard r/G and --shard-sweep G on a small workload: the one-GPU estimate of G-GPU strong scaling (each
    shard rendered as rank r of G would render it).  The shards' ray totals add up to the full frame's."""
    import json
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "LOCAL_RANK", "WORLD_SIZE")}
    r = subprocess.run([sys.executable, os.path.join(root, "bench.py"), "--workload", "c1", "--shard-sweep", "2"],
                       capture_output=True, text=True, timeout=600, env=env)
    assert r.returncode == 0, r.stdout + r.stderr
    sw = json.loads([l for l in r.stdout.splitlines() if l.startswith("{")][0])["shard_sweep"]
    assert sw["G"] == 2 and len(sw["shards"]) == 2 and sw["ray_total_matches"] and sw["predicted_speedup"] > 0
    r = subprocess.run([sys.executable, os.path.join(root, "bench.py"), "--workload", "c1", "--shard", "1/2", "--steps", "2",
                        "--no-extra", "--no-cpu-baseline"], capture_output=True, text=True, timeout=600, env=env)
    assert r.returncode == 0, r.stdout + r.stderr
    line = json.loads([l for l in r.stdout.splitlines() if l.startswith("{")][0])
    assert line["n_gpus"] == 1 and "shard 1 only" in line["config"]["workload"] and line["value"] > 0


def test_bench_plain_run_and_its_dumped_outputs(tmp_path):
    """A plain bench.py run times --steps steps and carries nothing of what --full adds; --dump-outputs writes what the
    last step returned -- the Python binding's render of the same workload, bit for bit -- and, for a frame whose outputs
    pass 64 MB, the same seeded sample of pixels of each array."""
    import json
    import os
    import subprocess
    import sys
    import common
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "LOCAL_RANK", "WORLD_SIZE")}

    def bench(out, *args):
        r = subprocess.run([sys.executable, os.path.join(root, "bench.py"), "--steps", "2", "--warmup", "1",
                            "--dump-outputs", str(out)] + list(args), capture_output=True, text=True, timeout=600, env=env)
        assert r.returncode == 0, r.stdout + r.stderr
        return json.loads([l for l in r.stdout.splitlines() if l.startswith("{")][0])

    line = bench(tmp_path / "c1", "--workload", "c1")
    assert line["steps"] == 2 and line["ms_per_step"] > 0 and line["value"] > 0 and line["unit"] == "Mrays/s"
    assert "cpu_baseline" not in line and "extra" not in line["config"] and "shard_sweep" not in line["config"]
    img, cnt = np.load(str(tmp_path / "c1" / "image.npy")), np.load(str(tmp_path / "c1" / "ray_counts.npy"))
    assert img.dtype == np.float32 and img.shape == (256, 256, 3) and cnt.dtype == np.float64 and cnt.shape == (256, 256)
    want, rays, _, total, _ = common.gpu_render("spheres", 256, 256, 16, 8)
    assert np.array_equal(img, want) and np.array_equal(cnt, rays.astype(np.float64))
    assert np.load(str(tmp_path / "c1" / "rays_per_step.npy")).tolist() == [float(total)] == [line["config"]["rays_per_step"]]

    # 2048 x 2048: 80 MB of outputs, so a sample of 64 MB at most
    bench(tmp_path / "big", "--scene", "spheres", "--size", "2048", "--spp", "1", "--depth", "2")
    files = sorted(os.listdir(str(tmp_path / "big")))
    assert files == ["image.npy", "ray_counts.npy", "rays_per_step.npy", "sample_index.npy"], files
    assert sum(os.path.getsize(str(tmp_path / "big" / f)) for f in files) <= 64 << 20
    idx = np.load(str(tmp_path / "big" / "sample_index.npy")).astype(np.int64)
    assert len(idx) > 2 << 20 and (np.diff(idx) > 0).all() and idx[-1] < 2048 * 2048
    want, rays, _, _, _ = common.gpu_render("spheres", 2048, 2048, 1, 2)
    assert np.array_equal(np.load(str(tmp_path / "big" / "image.npy")), want.reshape(-1, 3)[idx])
    assert np.array_equal(np.load(str(tmp_path / "big" / "ray_counts.npy")), rays.reshape(-1)[idx].astype(np.float64))


def test_render_mode_reports_the_schedule_of_the_baseline_configs():
    """rtmi_render_mode: what rtmi_render_ex decides before it launches anything, on BASELINE's five configurations (their
    frame shapes; nothing is rendered): C2 and the C4 / C5 shards are planned chains after a first pass of the frame's own
    samples, the mesh frame comes from the queue after two, C1 is a thin unscheduled frame with priorities every four."""
    import rtmi
    import common
    def mode(name, side, spp, depth, rank=0, world=1, **kw):
        b = common.build_scene(rtmi.SceneBuilder(common.scene_seed(name)), name, 1.0).commit()
        R = rtmi.Renderer(b, side, side, spp, depth, True, rank=rank, world_size=world)
        opts = rtmi.render_opts(**kw) if kw else None
        m, shape = R.mode(opts), R.launch_shape(opts)
        assert m["waves"] == shape["blocks"] * shape["threads"] // 64, (m, shape)  # both reports read one plan
        return m
    c2 = mode("cornell_box", 1024, 1024, 50)
    assert c2["scheduled"] == 1 and c2["first_pass_resumed"] == 1 and c2["first_pass_samples"] == 64 and c2["planned_chains"] == 1
    assert c2["wave_priority_every"] == 16 and c2["lane_stride"] == 1 and c2["tiles"] == 16384 and c2["tiles"] <= 3 * c2["waves"]
    c4 = mode("cornell_box", 2048, 4096, 50, rank=3, world=8)
    assert c4["planned_chains"] == 1 and c4["first_pass_samples"] == 64 and c4["tiles"] == 8192
    c5 = mode("birthday", 4096, 8192, 10, rank=0, world=8)
    assert c5["planned_chains"] == 1 and c5["tiles"] == 32768 and c5["tiles"] <= 8 * c5["waves"]
    c3 = mode("bunny", 1024, 512, 10)
    assert c3["scheduled"] == 1 and c3["first_pass_samples"] == 2 and c3["first_pass_resumed"] == 1 and c3["planned_chains"] == 0
    c1 = mode("spheres", 256, 16, 8)
    assert c1["scheduled"] == 0 and c1["first_pass_samples"] == 0 and c1["lane_stride"] == 4 and c1["wave_priority_every"] == 4
    # per-call options reach the decision
    assert mode("cornell_box", 1024, 1024, 50, plan=0)["planned_chains"] == 0
    assert mode("cornell_box", 1024, 1024, 50, first_pass=0)["first_pass_resumed"] == 0
    assert mode("cornell_box", 1024, 1024, 50, schedule=0)["scheduled"] == 0
    assert mode("cornell_box", 1024, 1024, 50, wave_priority=0) ["planned_chains"] == 0  # the plan needs the priorities
    assert mode("cornell_box", 1024, 128, 50)["planned_chains"] == 0  # 2.67 tiles per wave at 128 spp: the queue


def test_bench_n_rank_code_with_real_rendering_on_one_gpu():
    """bench.py --gpus 2 and 3 with its one-GPU test hook (every rank on cuda:0, exchange over gloo): the N-rank code of
    the bench -- per-rank shards, barrier-bracketed timing, max over ranks, the gather of the tile buffers, untile on rank
    0, the per-rank kernel times -- with real rendering.  The ray total of the ranks' shards is the single-rank frame's."""
    import json
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_PORT")}

    def run(n, extra=None):
        e = dict(env, **(extra or {}))
        r = subprocess.run([sys.executable, os.path.join(root, "bench.py"), "--gpus", str(n), "--workload", "c1", "--steps", "2",
                            "--warmup", "1", "--no-cpu-baseline", "--no-extra", "--rank-timeout", "300"],
                           capture_output=True, text=True, timeout=600, env=e)
        assert r.returncode == 0, r.stdout + r.stderr
        lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
        assert len(lines) == 1, r.stdout
        return json.loads(lines[0])

    one = run(1)
    for n in (2, 3):
        d = run(n, {"RTMI_BENCH_TEST_ONE_GPU": "1"})
        assert d["n_gpus"] == n and d["config"]["n_ranks_seen"] == n and len(d["config"]["kernel_ms_per_rank"]) == n
        assert "test_one_gpu" in d and d["scaling"] == "strong"
        assert d["config"]["rays_per_step"] == one["config"]["rays_per_step"]
        assert d["value"] > 0 and d["ms_per_step"] > 0 and "RCCL gather" in d["config"]["workload"]


def test_everything_at_once_variant():
    """A world that needs every kernel feature together (the F_ALL specialisation): a grouped sphere run, world-list
    pairs, two meshes (one with texture coordinates under an image texture), a defocus camera."""
    from rtmi import scenes

    def cam(b):
        b.camera_defocus(v3(0, 1.2, 3.2), v3(0, 0.6, -1), v3(0, 1, 0), PI_D / 3, 48 / 36, 0.08, 4.0)

    def fill(b):
        rng = np.random.default_rng(12)
        mats = [b.lambertian(v3(*rng.uniform(0.2, 0.9, 3))) for _ in range(3)] + [b.metal(v3(0.9, 0.9, 0.9), 0.05), b.dielectric(v3(1, 1, 1), 1.5)]
        tex = b.lambertian_tex(b.image_texture(scenes.procedural_earthmap(32, 64)))
        b.parallelogram([v3(-4, 0, -6), v3(4, 0, -6), v3(-4, 0, 2)], mats[0])
        for _ in range(40):
            b.sphere(v3(rng.uniform(-2.5, 2.5), rng.uniform(0.1, 1.8), rng.uniform(-4, 0.5)), float(rng.uniform(0.05, 0.3)),
                     mats[int(rng.integers(0, 5))])
        b.sphere(v3(1.2, 0.5, -0.5), 0.5, tex)
        for k in range(5):
            b.parallelepiped([v3(-2 + k, 0, -2.5), v3(-1.6 + k, 0, -2.5), v3(-2 + k, 0.5, -2.5), v3(-2 + k, 0, -2.1)], mats[k % 5])
        n = 60
        base = rng.uniform(-0.5, 0.5, (n, 1, 3)) + np.array([-1.0, 0.8, -1.5])
        faces = (base + rng.uniform(-0.2, 0.2, (n, 3, 3))).astype(np.float32)
        uvs = rng.uniform(0, 1, (n, 6)).astype(np.float32)
        b.bvh(faces, tex, uvs=uvs, k_min=8)
        b.bvh((faces + np.float32(1.5)).astype(np.float32), mats[3], k_min=2)
        b.parallelogram([v3(-1, 3.2, -3), v3(1, 3.2, -3), v3(-1, 3.2, -1)], b.diffuse_light(b.constant_texture(v3(3, 3, 3))))
        b.sky()
    g, o = render_pair(fill, 36, 48, 3, 10, camera=cam)
    # the image-textured sphere's texel choice goes through acosf / atan2f (two libms): the north-star tolerance there
    assert g.total == o.total or abs(g.total - o.total) <= 4
    rel = np.sqrt(((g.image.astype(np.float64) - o.image) ** 2).sum() / (o.image.astype(np.float64) ** 2).sum())
    assert rel <= 1e-3, rel
    assert (g.counts == o.counts).mean() > 0.99
