"""The cases on which the oracle is compared with the reference's own code, shared by tests/test_ref_parity.py (oracle
against the reference renderer built for the CPU, live), tests/golden/make_golden.py --ref (which records the reference
renderer's outputs as tests/golden/ref_*.npz), tests/test_ref_golden.py (oracle against those records) and
tests/test_gpu_ref_golden.py (librtmi against them).

Everything here drives a *builder* (rtmi/scenes.py): OracleBuilder, RefBuilder and rtmi.SceneBuilder all take it.  The
inputs of every probe (rays, records, RNG states) are tables of numbers; the recorded fixtures hold the tables
themselves, so a comparison never depends on regenerating them.
"""
import numpy as np

import common
from rtmi import scenes
from rtmi.scenes import PI_D, v3

SEEDS = (1024, 10086)  # Main() and DistributedMain() (utils.cu)
DEPTH = 10  # TRACE_DEPTH_LIMIT

# name, H, W, spp: the goldens' small shapes; every one is rendered with both seeds, post-processed and raw
FRAMES = [
    ("cornell_box", 24, 32, 4),
    ("spheres", 24, 32, 2),
    ("bunny", 24, 32, 2),
    ("bunny_split", 16, 16, 2),
    ("birthday", 24, 32, 4),
    ("sky_only", 16, 24, 2),
    ("furnace", 16, 16, 4),
    ("mixed", 20, 28, 4),
    ("nested_lists", 20, 26, 4),
]


def frame_file(name, h, w, spp, post):
    return "ref_%s_%dx%d_s%d_d%d_%s.npz" % (name, h, w, spp, DEPTH, "post" if post else "raw")


def nested_lists(b, aspect):
    """The world of tests/scenes/nested_lists.cu through the builder protocol: lists in lists, with coincident
    surfaces at different nesting levels."""
    b.camera_pinhole(v3(0, 0.8, 2.2), v3(0, 0.6, -1), v3(0, 1, 0), PI_D / 3, aspect)
    m0 = b.lambertian(v3(0.2, 0.6, 0.8))
    m1 = b.lambertian(v3(0.8, 0.3, 0.2))
    m2 = b.metal(v3(0.7, 0.7, 0.6), 0.25)
    m3 = b.dielectric(v3(1, 1, 1), 1.5)
    m4 = b.diffuse_light(b.constant_texture(v3(3, 3, 3)))
    f32 = np.float32

    def wall(z, m, dx):
        x0, x1 = f32(f32(-1.5) + f32(dx)), f32(f32(1.5) + f32(dx))
        b.parallelogram([v3(x0, -0.2, z), v3(x1, -0.2, z), v3(x0, 1.8, z)], m)

    b.sky()
    b.list_begin()
    wall(-2.0, m0, 0.0)
    b.list_begin()
    wall(-2.0, m1, 0.7)
    b.sphere(v3(-0.6, 0.5, -1.0), 0.45, m2)
    b.list_begin()
    b.parallelepiped([v3(0.3, 0.0, -1.4), v3(0.9, 0.0, -1.4), v3(0.3, 0.7, -1.4), v3(0.3, 0.0, -0.8)], m3)
    b.parallelogram([v3(0.3, 0.0, -0.8), v3(0.9, 0.0, -0.8), v3(0.3, 0.7, -0.8)], m1)
    b.list_end()
    b.list_end()
    b.triangle([v3(-1.4, 1.2, -1.9), v3(-0.4, 1.2, -1.9), v3(-0.9, 1.9, -1.9)], m4)
    b.list_end()
    b.list_begin()
    b.list_end()
    b.list_begin()
    b.sphere(v3(0, -100.2, -1), 100.0, m0)
    b.list_end()
    wall(-2.0, m2, -0.9)


_SPLIT_MESH = []


def split_mesh():
    """2352 faces: more than BVHNode's leaf size of 2048, so the root splits once."""
    if not _SPLIT_MESH:
        _SPLIT_MESH.append(scenes.procedural_bunny_mesh(14))
        assert _SPLIT_MESH[0].shape[0] > 2048
    return _SPLIT_MESH[0]


def build_frame_scene(b, name, aspect):
    """Scene `name` of FRAMES on builder b; the BVH scenes at the reference's own leaf size."""
    if name == "nested_lists":
        nested_lists(b, aspect)
    elif name == "bunny":
        scenes.bunny(b, aspect, common.small_mesh(), k_min=2048)
    elif name == "bunny_split":
        scenes.bunny(b, aspect, split_mesh(), k_min=2048)
    else:
        common.build_scene(b, name, aspect)
    return b


# ---------------------------------------------------------------------------------------------- probe worlds
def ties_mesh(n=2400, seed=5):
    """n faces whose first vertices take only six distinct x: the BVH's sort key (positions_[0].x) ties massively."""
    rng = np.random.default_rng(seed)
    p0 = np.stack([rng.integers(0, 6, n) * 0.25 - 0.6, rng.uniform(-0.7, 0.7, n), rng.uniform(-0.7, 0.7, n)], axis=1)
    f = p0[:, None, :] + np.concatenate([np.zeros((n, 1, 3)), rng.uniform(-0.15, 0.15, (n, 2, 3))], axis=1)
    return np.ascontiguousarray(f.astype(np.float32))


def coincident_mesh():
    """Forty faces, each present twice with different texture coordinates: in a BVH leaf the later copy must win."""
    rng = np.random.default_rng(11)
    f = rng.uniform(-0.8, 0.8, (40, 3, 3)).astype(np.float32)
    faces = np.concatenate([f, f[::-1]], axis=0)
    uvs = rng.uniform(0, 1, (80, 3, 2)).astype(np.float32)
    return np.ascontiguousarray(faces), np.ascontiguousarray(uvs)


def _w_sphere(b):
    b.sphere(v3(0.1, -0.2, 0.3), 0.9, b.lambertian(v3(0.5, 0.5, 0.5)))


def _w_triangle(b):
    b.triangle([v3(-0.9, -0.7, 0.1), v3(0.8, -0.6, -0.2), v3(0.1, 0.9, 0.3)], b.lambertian(v3(0.5, 0.5, 0.5)))


def _w_parallelogram(b):
    b.parallelogram([v3(-0.7, -0.6, 0.2), v3(0.6, -0.7, -0.1), v3(-0.5, 0.7, 0.3)], b.lambertian(v3(0.5, 0.5, 0.5)))


def _w_box_corner(b):
    b.parallelepiped([v3(-0.6, -0.5, -0.4), v3(0.5, -0.4, -0.5), v3(-0.7, 0.6, -0.3), v3(-0.5, -0.6, 0.7)],
                     b.lambertian(v3(0.5, 0.5, 0.5)))


def _w_box_lengths(b):
    a = np.float32(0.37)
    b.parallelepiped_lengths(v3(0.9, 1.1, 0.7), b.lambertian(v3(0.5, 0.5, 0.5)),
                             lambda p: scenes.rotate_y(p, a) + v3(-0.4, -0.5, -0.3))


def _w_sky(b):
    b.sky()


def _w_tie_list(b):
    """Two entries with equal t everywhere they overlap (the first must win), then a nearer one behind them in the list."""
    m = [b.lambertian(v3(0.1 * i, 0.5, 0.5)) for i in range(1, 4)]
    b.parallelogram([v3(-0.8, -0.8, 0.0), v3(0.8, -0.8, 0.0), v3(-0.8, 0.8, 0.0)], m[0])
    b.parallelogram([v3(-0.8, -0.8, 0.0), v3(0.8, -0.8, 0.0), v3(-0.8, 0.8, 0.0)], m[1])
    b.sphere(v3(0.5, 0.5, 0.0), 0.3, m[2])


def _w_nested(b):
    m = [b.lambertian(v3(0.1 * i, 0.5, 0.5)) for i in range(1, 5)]
    b.parallelogram([v3(-0.8, -0.8, 0.0), v3(0.2, -0.8, 0.0), v3(-0.8, 0.8, 0.0)], m[0])
    b.list_begin()
    b.parallelogram([v3(-0.4, -0.8, 0.0), v3(0.8, -0.8, 0.0), v3(-0.4, 0.8, 0.0)], m[1])
    b.list_begin()
    b.sphere(v3(0.0, 0.0, 0.0), 0.4, m[2])
    b.parallelogram([v3(-0.8, -0.3, 0.0), v3(0.8, -0.3, 0.0), v3(-0.8, 0.3, 0.0)], m[3])
    b.list_end()
    b.list_begin()
    b.list_end()
    b.list_end()
    b.sky()


def _w_bvh_coincident(b):
    faces, uvs = coincident_mesh()
    b.bvh(faces, b.lambertian(v3(0.5, 0.5, 0.5)), uvs=uvs)


def _w_bvh_ties(b):
    b.bvh(ties_mesh(), b.lambertian(v3(0.5, 0.5, 0.5)))


def _w_bvh_2048(b):
    b.bvh(split_mesh()[:2048] * np.float32(8.0) + v3(0.1, -0.9, 0.0), None)


def _w_bvh_2049(b):
    b.bvh(split_mesh()[:2049] * np.float32(8.0) + v3(0.1, -0.9, 0.0), None)


def _w_bvh_split(b):
    b.bvh(split_mesh() * np.float32(8.0) + v3(0.1, -0.9, 0.0), b.lambertian(v3(0.5, 0.5, 0.5)))


# the oracle variant (oraclelib.host_variant) under which a world's records are bit-equal to the host build's
PROBE_VARIANT = {"sphere": 1, "tie_list": 1, "nested": 1, "bvh_ties": 2}  # 1: worlds that hold a sphere

# world -> (builder function, rays in the random part of its table)
PROBE_WORLDS = {
    "sphere": (_w_sphere, 1500), "triangle": (_w_triangle, 1000), "parallelogram": (_w_parallelogram, 1000),
    "box_corner": (_w_box_corner, 1000), "box_lengths": (_w_box_lengths, 1000), "sky": (_w_sky, 100),
    "tie_list": (_w_tie_list, 800), "nested": (_w_nested, 800), "bvh_coincident": (_w_bvh_coincident, 800),
    "bvh_ties": (_w_bvh_ties, 300), "bvh_2048": (_w_bvh_2048, 150), "bvh_2049": (_w_bvh_2049, 150),
    "bvh_split": (_w_bvh_split, 200),
}


def build_probe_world(b, name):
    PROBE_WORLDS[name][0](b)
    return b


NO_UV_WORLDS = ("bvh_ties", "bvh_2048", "bvh_2049", "bvh_split")


def defined_columns(name, hit, rec, mat):
    """(N, 6) bool: the fields of the records {t, u, v, nx, ny, nz} that the reference's code defines.  Sky::Hit writes
    only t and the material, and a BVH face without texture coordinates writes no u, v: the rest of such a record is
    whatever its HitRecord held before, uninitialised in the reference and zero in the oracle.  Nothing on the render
    path reads those fields (the Sky's material takes the hit point; the reference's meshes without texture coordinates
    carry constant textures)."""
    keep = np.repeat(hit.astype(bool)[:, None], 6, axis=1)
    sky = (mat == -1) & (rec[:, 0] == 1e9) if name not in NO_UV_WORLDS else np.zeros(len(hit), dtype=bool)
    keep[sky, 1:] = False
    if name in NO_UV_WORLDS:
        keep[:, 1:3] = False
    return keep


def _unit(v):
    return v / np.linalg.norm(v, axis=-1, keepdims=True)


def run_probes(b, table):
    """table (N, 8) float64 {origin, direction, t_from, t_to} -> (hit uint8 (N,), record float64 (N, 6), material
    int32 (N,)); the record and material of a miss are zero / -1."""
    n = table.shape[0]
    hit = np.zeros(n, dtype=np.uint8)
    rec = np.zeros((n, 6), dtype=np.float64)
    mat = np.full(n, -1, dtype=np.int32)
    for i in range(n):
        h, r, m = b.probe_hit(table[i, 0:3], table[i, 3:6], table[i, 6], table[i, 7])
        if h:
            hit[i], rec[i], mat[i] = 1, r, m
    return hit, rec, mat


def probe_table(b, name, seed=2024, scale=1.0):
    """The probe rays of world `name`, built on builder b (which holds that world).

    Random part: origins in a shell around the unit-sized world, or inside it (a sphere seen from inside, a box from
    inside), aimed at random points of it, so most rays hit; a tenth aimed at the silhouette of the unit sphere around
    the aim point's centre, for grazing rays.  Range [1e-3, inf).
    Edge part, from the records of the first 120 hits: the same ray with t_to exactly the hit's t, and one ulp below;
    t_from exactly t, and one ulp above; and a ray leaving the hit point itself, whose nearest root is a self-hit
    around the 1e-3 threshold."""
    rng = np.random.default_rng(seed + sum(map(ord, name)))
    n = max(40, int(PROBE_WORLDS[name][1] * scale))  # scale < 1: the shorter tables recorded under tests/golden/
    inside = rng.uniform(0, 1, n) < 0.3
    o = np.where(inside[:, None], rng.uniform(-0.5, 0.5, (n, 3)), _unit(rng.normal(size=(n, 3))) * rng.uniform(1.5, 4, (n, 1)))
    target = rng.uniform(-0.8, 0.8, (n, 3))
    graze = rng.uniform(0, 1, n) < 0.1
    if name == "sphere":  # the silhouette as seen from o: points at distance r from the centre, at right angles to the view
        c, r = np.array([0.1, -0.2, 0.3]), 0.9
        side = _unit(np.cross(c - o, rng.normal(size=(n, 3))))
        dist = np.linalg.norm(c - o, axis=1, keepdims=True)
        tang = c + side * r * np.sqrt(np.maximum(1 - (r / np.maximum(dist, r)) ** 2, 0)) * (1 + rng.uniform(-2e-7, 2e-7, (n, 1)))
        tang = tang + (o - c) * (r / np.maximum(dist, r)) ** 2
        target = np.where((graze & ~inside)[:, None], tang, target)
    d = _unit(target - o)
    o32, d32 = o.astype(np.float32).astype(np.float64), d.astype(np.float32).astype(np.float64)
    base = np.concatenate([o32, d32, np.full((n, 1), 1e-3), np.full((n, 1), np.inf)], axis=1)
    hit, rec, _ = run_probes(b, base)
    rows = [base]
    idx = np.flatnonzero(hit)[:max(10, int(120 * scale))]
    for i in idx:
        t = rec[i, 0]
        for t_from, t_to in ((1e-3, t), (1e-3, np.nextafter(t, 0)), (t, np.inf), (np.nextafter(t, np.inf), np.inf)):
            rows.append(np.concatenate([base[i, :6], [t_from, t_to]])[None])
        p = (base[i, 0:3].astype(np.float32) + np.float32(t) * base[i, 3:6].astype(np.float32)).astype(np.float64)
        for nd in (-base[i, 3:6], _unit(rng.normal(size=3)).astype(np.float32).astype(np.float64)):
            rows.append(np.concatenate([p, nd, [1e-3, np.inf]])[None])
            rows.append(np.concatenate([p, nd, [0.0, np.inf]])[None])
    return np.ascontiguousarray(np.concatenate(rows, axis=0))


# ---------------------------------------------------------------------------------------------- scatter
def scatter_materials(b):
    """Every material kind; returns their names in index order."""
    b.lambertian(v3(0.3, 0.6, 0.9))
    b.lambertian_tex(b.image_texture(scenes.procedural_earthmap(16, 36)))
    b.metal(v3(0.7, 0.6, 0.5), 0.0)
    b.metal(v3(0.7, 0.6, 0.5), 0.3)
    b.metal(v3(0.7, 0.6, 0.5), 1.7)  # clamped to 1 by the constructor
    b.dielectric(v3(0.9, 1.0, 0.8), 1.5)
    b.dielectric(v3(1, 1, 1), 2.4)
    b.diffuse_light(b.constant_texture(v3(4, 3, 2)))
    b.diffuse_light(b.image_texture(scenes.procedural_earthmap(16, 36)))
    return ["lambertian", "lambertian_image", "metal_mirror", "metal_fuzz", "metal_fuzz_clamped", "dielectric_1.5",
            "dielectric_2.4", "light", "light_image"]


def scatter_table(n_per_material=400, seed=99):
    """(N, 16) float64 {material, origin, direction, t, u, v, normal} and (N, 6) uint32 RNG states.  A quarter of the
    rays leave the surface (dot(d, n) >= 0: Lambertian and Metal refuse, Dielectric refracts outwards or reflects
    totally); incidence angles are uniform on the sphere, so both sides of every critical angle are covered; u and v
    include 0 and 1 exactly."""
    import oraclelib
    rng = np.random.default_rng(seed)
    n_mat = 9
    n = n_mat * n_per_material
    mat = np.repeat(np.arange(n_mat), n_per_material)
    o = rng.uniform(-2, 2, (n, 3))
    d = _unit(rng.normal(size=(n, 3)))
    nrm = _unit(rng.normal(size=(n, 3)))
    flip = np.sign(np.sum(d * nrm, axis=1, keepdims=True))
    leaving = rng.uniform(0, 1, (n, 1)) < 0.25
    nrm = nrm * np.where(leaving, flip, -flip)
    t = rng.uniform(0.01, 5, (n, 1))
    uv = rng.uniform(0, 1, (n, 2))
    uv[::17] = np.round(uv[::17])
    tab = np.concatenate([mat[:, None], o, d, t, uv, nrm], axis=1)
    tab[:, 1:] = tab[:, 1:].astype(np.float32).astype(np.float64)
    states = oraclelib.rng_init(4242, n)
    return np.ascontiguousarray(tab), states


def run_scatter(b, table, states):
    """-> (scattered uint8 (N,), out float32 (N, 12), states after uint32 (N, 6))"""
    n = table.shape[0]
    sc = np.zeros(n, dtype=np.uint8)
    out = np.zeros((n, 12), dtype=np.float32)
    after = states.copy()
    for i in range(n):
        r = table[i]
        s, o = b.probe_scatter_ex(int(r[0]), r[1:4], r[4:7], r[7], r[8], r[9], r[10:13], after[i])
        sc[i], out[i] = s, o
    return sc, out, after


# ---------------------------------------------------------------------------------------------- camera
def build_camera(b, kind):
    if kind == "pinhole":
        b.camera_pinhole(v3(13, 2, 3), v3(0.3, -0.2, 0.1), v3(0.1, 1, 0.05), PI_D / 9, 4.0 / 3.0)
    elif kind == "defocus":
        b.camera_defocus(v3(13, 2, 3), v3(0.3, -0.2, 0.1), v3(0, 1, 0), PI_D / 7, 1.5, 0.35, 9.5)
    elif kind == "raw":
        b.camera_raw(v3(0.5, 0.25, 3), v3(-2.1, -1.3, -0.7), v3(4.3, 0.1, -0.2), v3(0.2, 2.9, 0.1))
    else:
        raise KeyError(kind)
    return b


CAMERAS = ("pinhole", "defocus", "raw")


def camera_table(seed=5):
    """(N, 2) float64 screen points: the four corners, the centre, then random ones; and (N, 6) uint32 RNG states."""
    import oraclelib
    rng = np.random.default_rng(seed)
    xy = np.concatenate([np.array([[-1, -1], [1, -1], [-1, 1], [1, 1], [0, 0]], dtype=np.float64), rng.uniform(-1, 1, (195, 2))])
    return xy, oraclelib.rng_init(31337, xy.shape[0])


def run_camera(b, xy, states):
    """-> (frame float32 (4, 3) {position, lower-left corner, horizontal, vertical}, rays float32 (N, 6), states after)"""
    after = states.copy()
    rays = np.stack([b.probe_camera_ray(xy[i, 0], xy[i, 1], after[i]) for i in range(xy.shape[0])])
    return b.camera_get()[:4].copy(), rays, after


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view({4: np.uint32, 8: np.uint64}[a.dtype.itemsize]) if a.dtype.kind == "f" else a
