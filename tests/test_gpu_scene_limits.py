"""Scenes on both sides of the kernels' size switches, against the oracle bit for bit:
  * the material table: the width of the id stack (4-bit rows up to 16 materials, bytes up to 256, uint16 up to 65536,
    the image-textured variants' 32-bit layer words beyond), with every visible material at a boundary index and a
    colour that depends on all of its index bits, so a truncated id changes the pixel;
  * sphere runs at the grouping limit (65,535 spheres grouped, 65,536 scanned one by one), one material per sphere;
  * worlds of many meshes: per-mesh top tables, list-order ties between meshes, nested lists, and the LDS staging of
    reference nodes (kLdsNodes) and leaf paths (kLdsPaths) running out inside a later mesh.
Renders compare image, per-pixel ray counts, final RNG states and the ray total; rtmi_intersect / rtmi_occluded compare
every answer."""
import numpy as np
import pytest

import querylib as ql
import rtmi
from parity import assert_same_frame, build_pair, gpu_frame, oracle_frame
from rtmi.scenes import v3, PI_D, procedural_bunny_mesh

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

H, W, SPP = 20, 28, 3
RESUMED = dict(schedule=2)  # the first pass (samples [0, s1)), then every pixel resumed
SPARSE_1 = dict(schedule=2, sparse_stride=1)
LANES_16 = dict(schedule=2, lane_stride=16)


# ------------------------------------------------------------------ rendering both sides
def pair(fill):
    """The same world on the oracle and on the product (committed), the product's behind a Recorder."""
    return build_pair(fill, 5, record=True)


def assert_same(g, o, what):
    """NaN-tolerant, as this file always compared: a NaN must sit in the same pixel channel of both frames."""
    assert_same_frame(g, o, what, nan_ok=True)


def queries_agree(ob, rec, seed, n_family=200, identities=True):
    """rtmi_intersect (kind, t, normal, material, u, v, entry) and rtmi_occluded with t_max just below and just above
    each hit, against the oracle; no abandoned search in either."""
    O, D = ql.make_rays(ob, seed, n_family)
    raw = ql.gpu_intersect(rec.b, O, D).raw.cpu().numpy()
    bad = ql.compare(raw, ob, O, D, rec)
    assert not bad, bad[:4]
    # `entry` / `element` on a sample: a world of just that hitable (or face) gives the same t for the same ray
    if identities:  # (replays the recorded scene once per sample: not for tables of 65536 materials)
        bad = ql.check_identities(rec.b, rec, seed, O, D, raw, np.random.default_rng(seed))
        assert not bad, bad[:4]
    t = ql.oracle_t(ob, O, D)
    fin = np.isfinite(t)
    below = np.where(fin, np.nextafter(t, np.float32(0)), np.float32(1e30)).astype(np.float32)
    above = np.where(fin, np.nextafter(t, np.float32(np.inf)), np.float32(1e30)).astype(np.float32)
    for tm, what in ((below, "t_max below the hits"), (above, "t_max above the hits")):
        ql.agree(rec.b, O, D, tm, ql.filtered(t, tm), what)
    return raw


# ------------------------------------------------------------------ 1. material-table widths
WIDTHS = (16, 17, 256, 257, 512, 513, 65536, 65537, 70000)
BOUNDARY = (0, 15, 16, 255, 256, 511, 512, 65535, 65536)
DEPTHS = (1, 2, 63, 64)


def colour(i):
    """A colour in [0.15, 0.95]^3 from a 32-bit mix of the index: every index bit moves it."""
    h = (i * 0x9E3779B1 + 0x7F4A7C15) & 0xFFFFFFFF
    h ^= h >> 15
    h = (h * 0x2C1B3C6D) & 0xFFFFFFFF
    h ^= h >> 12
    return v3(*(0.15 + 0.8 * ((h >> s) & 255) / 255.0 for s in (0, 8, 16)))


def special(n):
    """Index -> kind of the visible materials: the boundary indices that exist, and n - 1."""
    idx = sorted({b for b in BOUNDARY if b < n} | {n - 1})
    kinds = ("lambertian", "metal", "dielectric", "lambertian", "metal", "light", "lambertian", "metal", "lambertian",
             "dielectric")
    out = {i: kinds[k % len(kinds)] for k, i in enumerate(idx)}
    out[0] = "lambertian"  # the ground
    out[15] = "mirror"     # the left wall
    if n > 65535:
        out[65535] = "mirror"  # the right wall
    out[n - 1] = "lambertian" if n - 1 not in (15, 65535) else out[n - 1]
    out[n // 2] = "light"  # (the lamp on the ceiling)
    return out


def material_world(b, n, signed=False, textured=None):
    """n materials; the visible primitives use the boundary indices.  A closed box of mirrors keeps some
    paths bouncing to the depth limit; the light is a lamp inside (index n // 2) and the lights among the boundary
    indices.  `signed`: the ground's green is -0.0 (the fold then adds 0 to every product).  `textured`: the
    material at this index reads an image texture (a parallelogram uses it)."""
    b.camera_pinhole(v3(0, 1.1, 2.0), v3(0, 0.5, -1), v3(0, 1, 0), PI_D / 3, W / H)
    spec = special(n)
    tex = None
    if textured is not None:
        rng = np.random.default_rng(3)
        tex = b.image_texture(rng.integers(0, 256, (8, 16, 4), dtype=np.uint8))
    light_tex = {}
    for i in range(n):
        c = colour(i)
        k = spec.get(i, "lambertian")
        if i == textured:
            b.lambertian_tex(tex)
        elif i == 0 and signed:
            b.lambertian(v3(c[0], -0.0, c[2]))
        elif k == "lambertian":
            b.lambertian(c)
        elif k == "metal":
            b.metal(c, 0.2)
        elif k == "mirror":
            b.metal(np.float32(0.05) + np.float32(0.95) * c / c.max(), 0.0)
        elif k == "dielectric":
            b.dielectric(c, 1.5)
        else:
            light_tex[i] = b.constant_texture(np.float32(3.0) * c)
            b.diffuse_light(light_tex[i])
    b.parallelogram([v3(-3, 0, -4), v3(3, 0, -4), v3(-3, 0, 2)], 0)  # ground
    left, right = 15, (65535 if n > 65535 else 15)
    b.parallelogram([v3(-2.2, 0, -4), v3(-2.2, 0, 2), v3(-2.2, 2.5, -4)], left)
    b.parallelogram([v3(2.2, 0, -4), v3(2.2, 2.5, -4), v3(2.2, 0, 2)], right)
    b.parallelogram([v3(-2.2, 2.5, -4), v3(2.2, 2.5, -4), v3(-2.2, 2.5, 2.4)], left)  # ceiling, back and front
    b.parallelogram([v3(-2.2, 0, -4), v3(2.2, 0, -4), v3(-2.2, 2.5, -4)], right)     # walls close the box: paths
    b.parallelogram([v3(-2.2, 0, 2.4), v3(-2.2, 2.5, 2.4), v3(2.2, 0, 2.4)], left)   # end at a light or the limit
    b.sphere(v3(0.4, 2.1, -2.5), 0.3, n // 2)
    vis = [i for i in sorted(spec) if i not in (0, 15, 65535, n // 2)]
    for k, i in enumerate(vis):
        x = -1.7 + 3.4 * (k + 0.5) / max(len(vis), 1)
        b.sphere(v3(x, 0.3 + 0.25 * (k % 2), -1.2 - 0.4 * (k % 3)), 0.3, i)
    if textured is not None:
        b.parallelogram([v3(-1.2, 0.05, -3.5), v3(1.2, 0.05, -3.5), v3(-1.2, 1.8, -3.5)], textured)
    b.sky()


def test_boundary_colours_differ_from_their_truncations():
    for i in BOUNDARY + (65537 - 1, 70000 - 1):
        for mask in (0xF, 0xFF, 0xFFFF):
            if i & mask != i:
                assert not np.array_equal(colour(i), colour(i & mask)), (i, mask)


@pytest.mark.parametrize("n", WIDTHS)
def test_material_table_widths(n):
    ob, rec = pair(lambda b: material_world(b, n))
    assert rec.b.stats()["materials"] == n
    for depth in DEPTHS:
        o = oracle_frame(ob, H, W, SPP, depth)
        assert depth < 2 or o.total > H * W * SPP * 1.5  # paths bounce
        assert_same(gpu_frame(rec.b, H, W, SPP, depth), o, "%d materials, depth %d" % (n, depth))


@pytest.mark.parametrize("n", WIDTHS)
def test_material_table_widths_signed_colour(n):
    ob, rec = pair(lambda b: material_world(b, n, signed=True))
    for depth in (2, 63):
        assert_same(gpu_frame(rec.b, H, W, SPP, depth), oracle_frame(ob, H, W, SPP, depth),
                    "%d materials, signed, depth %d" % (n, depth))


def test_image_textured_parallelogram_above_65535():
    ob, rec = pair(lambda b: material_world(b, 70000, textured=66000))
    for depth in (2, 64):
        assert_same(gpu_frame(rec.b, H, W, SPP, depth), oracle_frame(ob, H, W, SPP, depth), "textured, depth %d" % depth)


@pytest.mark.parametrize("n", (65537, 70000))
def test_material_ids_above_65535_resumed_and_sharded(n):
    ob, rec = pair(lambda b: material_world(b, n))
    o = oracle_frame(ob, H, W, SPP, 10)
    assert_same(gpu_frame(rec.b, H, W, SPP, 10, opts=RESUMED), o, "%d materials, resumed" % n)
    assert_same(gpu_frame(rec.b, H, W, SPP, 10, world=3), o, "%d materials, 3 shards" % n)


@pytest.mark.parametrize("n", (256, 257, 65536, 65537, 70000))
def test_intersect_reports_material_ids_of_any_width(n):
    ob, rec = pair(lambda b: material_world(b, n))
    raw = queries_agree(ob, rec, seed=n, n_family=150, identities=n < 1000)
    assert (raw[:, 6] >= 65536).any() == (n > 65536)  # the rays do reach the high-index materials


# ------------------------------------------------------------------ 2. sphere runs at the grouping limit
def sphere_run_world(b, n_run, short_run):
    """n_run spheres in 64 nested lists of up to 1024, each with its own material (spheres.cu's shape, 256 x 256 on the
    ground); then a parallelogram, and `short_run` more spheres (a short run, grouped: scene.hip), then the sky.  Every
    sphere's material is its own, so n_run + 1 + short_run materials."""
    side = 256
    b.camera_pinhole(v3(128, 14, 170), v3(128, 0, 150), v3(0, 1, 0), PI_D / 4, 1.0)
    for i in range(n_run + 1 + short_run):
        c = colour(i)
        if i % 3 == 0 or i == n_run:
            b.lambertian(c)
        elif i % 3 == 1:
            b.metal(c, 0.1)
        else:
            b.dielectric(c, 1.5)
    for first in range(0, n_run, 1024):
        b.list_begin()
        for i in range(first, min(n_run, first + 1024)):
            x, z = i % side, i // side
            b.sphere(v3(x + 0.5, 0.35, z + 0.5), 0.4, i)
        b.list_end()
    b.parallelogram([v3(0, -0.05, 0), v3(side, -0.05, 0), v3(0, -0.05, side)], n_run)  # the ground
    for j in range(short_run):
        b.sphere(v3(120 + 0.9 * (j % 8), 1.2, 150 + 0.9 * (j // 8)), 0.3, n_run + 1 + j)
    b.sky()


@pytest.mark.parametrize("n_run,short_run", [(65535, 0), (65536, 0), (65536, 40)])
def test_sphere_runs_at_the_grouping_limit(n_run, short_run):
    ob, rec = pair(lambda b: sphere_run_world(b, n_run, short_run))
    s = rec.b.stats()
    assert s["spheres"] == n_run + short_run and s["materials"] == n_run + 1 + short_run
    assert (s["materials"] > 65536) == (n_run > 65535)  # the ungrouped runs also hold material ids above 65535
    o = oracle_frame(ob, 16, 16, 2, 3)
    assert o.total > 16 * 16 * 2 * 1.5
    assert_same(gpu_frame(rec.b, 16, 16, 2, 3), o, "%d + %d spheres" % (n_run, short_run))


# ------------------------------------------------------------------ 3. many meshes
_MESH = {}


def mesh(n):
    if n not in _MESH:
        m = procedural_bunny_mesh(n).reshape(-1, 3).astype(np.float64)
        m = (m - m.mean(0)) / (m.max(0) - m.min(0)).max()  # unit size, centred
        _MESH[n] = m.astype(np.float32)
    return _MESH[n]


def many_mesh_world(b, n_meshes, k_min, mesh_n):
    """n_meshes meshes on a grid, interleaved with spheres, triangles and parallelograms (BVH runs of one) and in blocks
    of their own (long runs); every fifth mesh is repeated verbatim in the next entry with another material (equal t:
    the first wins); every seventh sits in a nested list."""
    side = int(np.ceil(np.sqrt(n_meshes)))
    sp = 1.1
    ctr = v3(sp * (side - 1) / 2, 0, -sp * (side - 1) / 2)
    b.camera_pinhole(ctr + v3(0, 0.9 * side + 1.5, 1.1 * side + 2.0), ctr, v3(0, 1, 0), PI_D / 3, W / H)
    mats = [b.lambertian(v3(0.8, 0.4, 0.3)), b.metal(v3(0.8, 0.85, 0.9), 0.05), b.dielectric(v3(1, 1, 1), 1.5),
            b.lambertian(v3(0.3, 0.6, 0.8)), b.lambertian(v3(0.6, 0.6, 0.2))]
    light = b.diffuse_light(b.constant_texture(v3(4, 4, 4)))
    base = mesh(mesh_n)
    b.parallelogram([v3(-50, -0.5, 50), v3(50, -0.5, 50), v3(-50, -0.5, -50)], mats[3])
    for i in range(n_meshes):
        x, z = i % side, i // side
        off = v3(sp * x, 0, -sp * z)
        faces = (base * np.float32(0.9 + 0.1 * (i % 3)) + off).reshape(-1, 9).astype(np.float32)
        nested = i % 7 == 3
        if nested:
            b.list_begin()
        b.bvh(faces, mats[i % 3], k_min=k_min)
        if i % 5 == 1:
            b.bvh(faces, mats[3 + i % 2], k_min=k_min)
        if i < n_meshes // 2:  # the first half interleaved with other kinds; the second half one long run
            if i % 3 == 0:
                b.sphere(off + v3(0.45, 0.45, 0.3), 0.12, mats[(i + 1) % 5])
            elif i % 3 == 1:
                b.triangle([off + v3(-0.5, 0.6, 0.4), off + v3(0.5, 0.6, 0.4), off + v3(0, 1.0, 0.2)], mats[(i + 2) % 5])
            else:
                b.parallelogram([off + v3(-0.5, -0.45, 0.5), off + v3(0.5, -0.45, 0.5), off + v3(-0.5, 0.2, 0.5)],
                                mats[i % 5])
        if nested:
            b.list_end()
    b.sphere(ctr + v3(0, 3 + side, 0), 1.0 + 0.2 * side, light)
    b.sky()


def one_mesh_nodes(k_min, mesh_n):
    b = rtmi.SceneBuilder(0)
    b.camera_pinhole(v3(0, 0, 3), v3(0, 0, 0), v3(0, 1, 0), 1.0, 1.0)
    b.bvh(mesh(mesh_n).reshape(-1, 9), b.lambertian(v3(0.5, 0.5, 0.5)), k_min=k_min)
    return b.stats()["bvh_nodes"]


def leaf_path_words_at_least(nodes):
    """A reference tree of `nodes` nodes has (nodes + 1) / 2 leaves, each with a row of its code and at least
    ceil(log2(leaves)) node words."""
    leaves = (nodes + 1) // 2
    return leaves * (1 + int(np.ceil(np.log2(max(leaves, 1)))))


MESH_CASES = [(2, 2, 4), (9, 8, 4), (64, 2, 2), (300, 2048, 2), (64, 2048, 3)]


@pytest.mark.parametrize("n_meshes,k_min,mesh_n", MESH_CASES)
def test_many_meshes(n_meshes, k_min, mesh_n):
    ob, rec = pair(lambda b: many_mesh_world(b, n_meshes, k_min, mesh_n))
    s = rec.b.stats()
    per = one_mesh_nodes(k_min, mesh_n)
    n_bvh = n_meshes + len(range(1, n_meshes, 5))
    assert s["bvh_nodes"] == n_bvh * per
    if k_min <= 8 and n_meshes >= 9:
        # the staging limits run out inside a later mesh: the first meshes' nodes and leaf paths are in LDS, the rest
        # are read from global memory
        assert per < 512 < s["bvh_nodes"]
        assert leaf_path_words_at_least(per) < 1024 < n_bvh * leaf_path_words_at_least(per)
    depth = 6
    o = oracle_frame(ob, H, W, 2, depth)
    assert o.total > H * W * 2 * 1.2
    for opts, what in ((None, "default"), (SPARSE_1, "sparse_stride=1"), (LANES_16, "lane_stride=16")):
        assert_same(gpu_frame(rec.b, H, W, 2, depth, opts=opts), o, "%d meshes, %s" % (n_meshes, what))
    raw = queries_agree(ob, rec, seed=n_meshes, n_family=300)
    kinds = raw[:, 7]
    assert (kinds == rtmi.RTMI_HIT_MESH).sum() >= 5
    entries = rec.entries()
    mesh_entries = {int(e) for e, k in zip(raw[:, 8], kinds) if k == rtmi.RTMI_HIT_MESH}
    assert all(entries[e][0] == "bvh" for e in mesh_entries)
    assert len(mesh_entries) >= min(n_meshes, 2)  # more than one mesh answers
    # a duplicated mesh never wins over its original: the tie goes to the earlier entry
    dup = {i + 1 for i, e in enumerate(entries[:-1]) if e[0] == "bvh" and entries[i + 1][0] == "bvh" and
           np.array_equal(np.asarray(e[1][0]), np.asarray(entries[i + 1][1][0]))}
    assert dup and not (mesh_entries & dup)
    for e, el in zip(raw[:, 8], raw[:, 9]):
        if entries[e][0] == "bvh":
            assert 0 <= el < len(np.asarray(entries[e][1][0]).reshape(-1, 9))
