"""Randomised-scene parity: seeded random worlds mixing every primitive and material kind,
random cameras (pinhole and defocus), frame shapes, depth limits and post/raw modes, rendered
through the C ABI and compared bit for bit with the oracle.  Complements the fixed scenes: it
exercises list orders, run boundaries (sphere / triangle / sky interleavings), nested boxes,
single triangles between parallelograms, several BVHs per world and material-table sizes on
both sides of the uint8/uint16 id-stack switch."""
import numpy as np
import pytest

import rtmi
from parity import assert_same_frame, build_pair, gpu_frame, oracle_frame
from rtmi.scenes import v3, PI_D
from worlds import SCHEDULER_PATHS, random_case, scheduler_mesh_world

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("seed", list(range(12)))
def test_random_world_bit_exact(seed):
    fill, h, w, spp, depth, post, _ = random_case(seed)
    ob, pb = build_pair(fill, 77 + seed)
    assert_same_frame(gpu_frame(pb, h, w, spp, depth, post), oracle_frame(ob, h, w, spp, depth, post), "seed %d" % seed)


def _layer_stack(n_layers, rng, jitter):
    """Quads perpendicular to the x axis, one after another along it: a ray travelling along x
    finds a hit in every layer, i.e. in far more reference leaves than the kernel's per-lane
    candidate list has slots."""
    faces = []
    for k in range(n_layers):
        x = -2.0 + 4.0 * k / max(n_layers - 1, 1)
        dx = rng.uniform(-jitter, jitter, 4)
        p = [np.array([x + dx[0], -0.6, -2.6]), np.array([x + dx[1], 0.9, -2.6]),
             np.array([x + dx[2], 0.9, -1.2]), np.array([x + dx[3], -0.6, -1.2])]
        faces.append([p[0], p[1], p[2]])
        faces.append([p[0], p[2], p[3]])
    return np.asarray(faces, dtype=np.float32)


@pytest.mark.parametrize("case", [
    # (layers, leaf size, material, jitter): leaves of 1..3 faces give 2x..0.7x leaves per layer
    # floor: a sphere selects the double-precision kernel variant, a parallelogram the float one
    (40, 1, "dielectric", 0.0, "sphere"), (40, 2, "dielectric", 0.02, "pgram"), (25, 3, "dielectric", 0.05, "pgram"),
    (12, 2, "lambertian", 0.0, "pgram"), (64, 2, "metal", 0.01, "sphere"), (40, 2048, "dielectric", 0.02, "pgram"),
    (40, 1, "dielectric", 0.0, "pgram"),
])
def test_many_hit_leaves_along_one_ray(case):
    """Mesh rays that hold hits in tens of reference leaves at once (more than kHitSlots):
    the search defers the leaves beyond its list to further passes; the result must still be
    the reference's in-order walk, bit for bit."""
    n_layers, k_min, kind, jitter, floor = case
    h, w, spp, depth = 24, 40, 3, 30

    def fill(b):
        rng = np.random.default_rng(4242)
        # the camera looks along +x through the whole stack
        b.camera_pinhole(v3(-4.5, 0.2, -1.9), v3(0, 0.15, -1.9), v3(0, 1, 0), PI_D / 4, w / h)
        if kind == "dielectric":
            m = b.dielectric(v3(0.95, 0.97, 0.99), 1.0)  # index 1: goes straight on, every layer is met
        elif kind == "metal":
            m = b.metal(v3(0.9, 0.9, 0.9), 0.3)
        else:
            m = b.lambertian(v3(0.7, 0.6, 0.5))
        b.bvh(_layer_stack(n_layers, rng, jitter), m, k_min=k_min)
        if floor == "sphere":
            b.sphere(v3(0, -100.7, -2), 100.0, b.lambertian(v3(0.5, 0.5, 0.5)))
        else:
            b.parallelogram([v3(-50, -0.7, -50), v3(50, -0.7, -50), v3(-50, -0.7, 50)], b.lambertian(v3(0.5, 0.5, 0.5)))
        b.sky()
    ob, pb = build_pair(fill, 5)
    o = oracle_frame(ob, h, w, spp, depth, post=False)
    assert o.total > h * w * spp * (2 if kind == "dielectric" else 1)  # paths do continue through the stack
    assert_same_frame(gpu_frame(pb, h, w, spp, depth, post=False), o, str(case))


@pytest.mark.parametrize("seed", [0, 1, 2, 3])
def test_scheduler_paths_agree_on_random_mesh_worlds(seed):
    """Mesh-heavy random worlds rendered six ways -- image order, forced longest-first (probe,
    outlier pixels spread one per 16 lanes, their waves working for them alone), as two interleaved
    shards, with the outlier spreading switched off, with one outlier pixel per wave, and without the
    helper-wave rule -- must give the same image, ray counts and ray total bit for bit.  (The oracle
    comparison of such worlds is test_random_world_bit_exact; this one is large enough for the
    scheduler to matter: 192x256 at 64 spp.)"""
    fill, h, w, spp, depth = scheduler_mesh_world(seed)
    pb = rtmi.SceneBuilder(90 + seed)
    fill(pb)
    pb.commit()
    plain = gpu_frame(pb, h, w, spp, depth, opts=SCHEDULER_PATHS[0][1])
    for world, opts in SCHEDULER_PATHS[1:]:
        assert_same_frame(gpu_frame(pb, h, w, spp, depth, opts=opts, world=world), plain, "%d shard(s), %s" % (world, opts))
    assert plain.total > h * w * spp * 1.2


def _nested_world(b, rng):
    """Lists inside lists (hitable_list.cuh:8), with coincident surfaces across nesting levels so that
    the tie rules of hitable_list.cu:12-20 decide pixels: the nested call accepts its first hit
    unconditionally and the parent then demands a strictly nearer one."""
    def col():
        return v3(*rng.uniform(0.1, 0.9, 3))
    mats = [b.lambertian(col()), b.lambertian(col()), b.metal(col(), float(rng.uniform(0, 0.4))), b.dielectric(v3(1, 1, 1), 1.5),
            b.diffuse_light(b.constant_texture(v3(3, 3, 3)))]

    def wall(z, m, dx=0.0):
        b.parallelogram([v3(-1.5 + dx, -0.2, z), v3(1.5 + dx, -0.2, z), v3(-1.5 + dx, 1.8, z)], mats[m])

    b.sky()
    b.list_begin()                      # A
    wall(-2.0, 0)                       #   back wall, material 0 ...
    b.list_begin()                      #   B inside A
    wall(-2.0, 1, 0.7)                  #     ... overlapped by a coincident wall of material 1 (a tie, first wins)
    b.sphere(v3(-0.6, 0.5, -1.0), 0.45, mats[2])
    b.list_begin()                      #     C inside B
    b.parallelepiped([v3(0.3, 0.0, -1.4), v3(0.9, 0.0, -1.4), v3(0.3, 0.7, -1.4), v3(0.3, 0.0, -0.8)], mats[3])
    b.parallelogram([v3(0.3, 0.0, -0.8), v3(0.9, 0.0, -0.8), v3(0.3, 0.7, -0.8)], mats[1])  # coincident with a box face
    b.list_end()
    b.list_end()
    b.triangle([v3(-1.4, 1.2, -1.9), v3(-0.4, 1.2, -1.9), v3(-0.9, 1.9, -1.9)], mats[4])
    b.list_end()
    b.list_begin()                      # an empty list, then one holding only the floor
    b.list_end()
    b.list_begin()
    b.sphere(v3(0, -100.2, -1), 100.0, mats[0])
    b.list_end()
    wall(-2.0, 2, -0.9)                 # and a coincident wall at world level, after the nested ones
    for _ in range(int(rng.integers(0, 3))):
        b.sphere(v3(*rng.uniform(-1, 1, 2), -1.0 + float(rng.uniform(-0.3, 0.3))), float(rng.uniform(0.1, 0.3)), mats[int(rng.integers(0, 4))])


@pytest.mark.parametrize("seed", [0, 1, 2, 3])
def test_nested_lists_match_the_nested_oracle(seed):
    """The library inlines nested HitableLists; the oracle builds them as real nested objects whose
    Hit() calls recurse (hitable_list.cu:7-25).  Image, ray counts and ray total must agree bit for
    bit -- including where coincident surfaces of different nesting levels tie."""
    h, w, spp, depth = 40, 52, 4, 12

    def fill(b):
        b.camera_pinhole(v3(0, 0.8, 2.2), v3(0, 0.6, -1), v3(0, 1, 0), PI_D / 3, w / h)
        _nested_world(b, np.random.default_rng(900 + seed))
    ob, pb = build_pair(fill, 31 + seed)
    assert_same_frame(gpu_frame(pb, h, w, spp, depth), oracle_frame(ob, h, w, spp, depth), "seed %d" % seed)


def _clump(n, rng, spread):
    """n faces around one point: centroids nearly coincide, so the search tree's splits fall back
    to medians and the tree is as deep as it gets for n faces."""
    c = rng.uniform(-0.2, 0.2, (n, 1, 3)) * spread + np.array([0.0, 0.3, -2.0])
    return (c + rng.uniform(-0.5, 0.5, (n, 3, 3))).astype(np.float32)


@pytest.mark.parametrize("case", [
    # (frame h, w, spp, depth, faces per mesh, reference leaf size, meshes): frames of at most 16 pixels keep every
    # search at <= 16 rays, i.e. on the top-table start; 5 x 13 starts dense and thins out towards the end of the frame
    (3, 5, 9, 12, 600, 2, 1), (4, 4, 7, 20, 1, 2048, 3), (2, 8, 6, 12, 2500, 1, 2), (2, 2, 40, 30, 300, 4, 2),
    (5, 13, 5, 12, 900, 3, 2), (3, 5, 9, 12, 70, 2048, 1),
])
def test_sparse_waves_start_from_the_top_table(case):
    """Waves with a handful of rays (tiny frames) on deep, clumped meshes with small reference leaves:
    the search starts from the mesh's table of sub-trees, runs in its four- and two-lanes-per-entry
    modes, and the replay reads leaf-path rows of 8, 16 and 32 words, from LDS and from global memory."""
    h, w, spp, depth, n_faces, k_min, n_meshes = case

    def fill(b):
        rng = np.random.default_rng(977)
        b.camera_pinhole(v3(0.1, 0.4, 1.2), v3(0, 0.3, -2.0), v3(0, 1, 0), PI_D / 5, w / h)
        mats = [b.dielectric(v3(0.95, 0.97, 0.99), 1.2), b.metal(v3(0.9, 0.85, 0.8), 0.2), b.lambertian(v3(0.8, 0.7, 0.6))]
        for i in range(n_meshes):
            b.bvh(_clump(n_faces, rng, 0.05 if i == 0 else 1.0), mats[i % 3], k_min=k_min)
        b.parallelogram([v3(-50, -0.7, -50), v3(50, -0.7, -50), v3(-50, -0.7, 50)], b.lambertian(v3(0.5, 0.5, 0.5)))
        b.sky()
    ob, pb = build_pair(fill, 31)
    o = oracle_frame(ob, h, w, spp, depth, post=False)
    assert o.total > h * w * spp  # the meshes are in view
    assert_same_frame(gpu_frame(pb, h, w, spp, depth, post=False), o, str(case))
