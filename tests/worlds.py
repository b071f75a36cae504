"""Worlds that more than one test file or tool builds: the long lists, soups, far views, needles, grazing sheets and
sphere clouds of the fuzz campaigns (tools/gpu_fuzz.py, tests/margin_campaign.py), the random worlds, the random list of
the fast-path tests, and the raw camera that leaves the normalisation's fast domain.  Each `fill(b)` works on a product
or an oracle builder."""
import numpy as np

import rtmi
from rtmi.scenes import v3, PI_D


# ------------------------------------------------------------------ long world lists
def _quilt(b, n, rng, boxes_every=0, dup_every=7):
    """n world-list entries (parallelograms; every `boxes_every`-th a box = six pairs) scattered in front of the
    camera, every `dup_every`-th entry repeated verbatim a little later (equal t: the first must win)."""
    mats = [b.lambertian(v3(*rng.uniform(0.2, 0.9, 3))) for _ in range(5)] + \
           [b.metal(v3(0.8, 0.8, 0.7), 0.0), b.metal(v3(0.7, 0.8, 0.9), 0.3), b.dielectric(v3(1, 1, 1), 1.5)]
    light = b.diffuse_light(b.constant_texture(v3(3, 3, 3)))
    made = []
    for i in range(n):
        c = np.array([rng.uniform(-2.2, 2.2), rng.uniform(0.0, 2.0), rng.uniform(-3.5, -0.5)])
        m = mats[int(rng.integers(0, len(mats)))]
        if boxes_every and i % boxes_every == boxes_every - 1:
            e = rng.uniform(0.15, 0.4, 3)
            pts = [v3(*c), v3(c[0] + e[0], c[1], c[2]), v3(c[0], c[1] + e[1], c[2]), v3(c[0], c[1], c[2] + e[2])]
            b.parallelepiped(pts, m)
            made.append(("box", pts, m))
        else:
            e1, e2 = rng.uniform(-0.45, 0.45, 3), rng.uniform(-0.45, 0.45, 3)
            pts = [v3(*c), v3(*(c + e1)), v3(*(c + e2))]
            b.parallelogram(pts, m)
            made.append(("pg", pts, m))
        if dup_every and i % dup_every == dup_every - 1:
            kind, pts, _ = made[int(rng.integers(0, len(made)))]
            other = mats[int(rng.integers(0, len(mats)))]
            (b.parallelepiped if kind == "box" else b.parallelogram)(pts, other)
    b.parallelogram([v3(-3, -0.01, -5), v3(3, -0.01, -5), v3(-3, -0.01, 1)], mats[0])
    b.parallelogram([v3(-1, 3.2, -3), v3(1, 3.2, -3), v3(-1, 3.2, -1)], light)
    b.sky()


# ------------------------------------------------------------------ triangle soups (round-2 fuzz campaign)
def soup_world(seed):
    """The triangle soups of the second fuzz campaign (tools/gpu_fuzz.py).  Returns (fill, h, w, spp, depth, description)."""
    rng = np.random.default_rng(50000 + seed)
    h, w = int(rng.integers(16, 49)), int(rng.integers(16, 65))
    spp, depth = int(rng.integers(1, 5)), int(rng.choice([2, 8, 20, 50]))
    n_mesh = int(rng.integers(1, 4))
    soups = []
    for _ in range(n_mesh):
        n = int(rng.choice([1, 5, 40, 300, 1500]))
        c = rng.uniform(-1.2, 1.2, 3)
        c[1] = abs(c[1]) * 0.5 + 0.2
        c[2] -= 2.0
        spread = float(rng.choice([0.05, 0.4, 1.0]))
        base = rng.uniform(-spread, spread, (n, 1, 3)) + c
        size = float(rng.choice([0.05, 0.3, 0.9]))
        f = (base + rng.uniform(-size, size, (n, 3, 3))).astype(np.float32)
        if rng.integers(0, 3) == 0:  # duplicated faces: equal t, ties by reference index
            f = np.concatenate([f, f[: max(1, n // 3)]], 0)
        soups.append((f, int(rng.choice([1, 2, 3, 8, 64, 2048])), int(rng.integers(0, 4))))
    floor_sphere = bool(rng.integers(0, 2))

    def fill(b):
        ms = [b.lambertian(v3(0.8, 0.7, 0.6)), b.metal(v3(0.9, 0.9, 0.8), 0.1), b.dielectric(v3(1, 1, 1), 1.0),
              b.dielectric(v3(0.9, 1, 0.9), 1.5)]
        for f, kmin, mi in soups:
            b.bvh(f, ms[mi], k_min=kmin)
        if floor_sphere:
            b.sphere(v3(0, -100.5, -1), 100.0, ms[0])
        else:
            b.parallelogram([v3(-30, -0.5, -30), v3(30, -0.5, -30), v3(-30, -0.5, 30)], ms[0])
        b.sky()
    return fill, h, w, spp, depth, [(s[0].shape[0], s[1], s[2]) for s in soups]


# ------------------------------------------------------------------ far views of thin faces
def sliver_fan(angle_deg, n=64, size=2e-3, seed=3):
    """n thin triangles (apex angle `angle_deg`, legs of `size`) scattered over a 4 cm patch around the origin."""
    rng = np.random.default_rng(seed)
    faces = []
    a = np.deg2rad(angle_deg)
    for _ in range(n):
        c = np.array([rng.uniform(-0.02, 0.02), rng.uniform(-1e-3, 1e-3), rng.uniform(-0.02, 0.02)])
        th = rng.uniform(0, 2 * np.pi)
        u = np.array([np.cos(th), 0.05 * rng.uniform(-1, 1), np.sin(th)])
        v = np.array([np.cos(th + a), 0.05 * rng.uniform(-1, 1), np.sin(th + a)])
        faces.append([c, c + size * u, c + size * v])
    return np.asarray(faces, dtype=np.float32)


def far_view_world(seed):
    """Third campaign of tools/gpu_fuzz.py: a small mesh seen from 10 .. 2e4 away, first or last in the world list,
    fat or thin faces, reference leaves of 1 .. 64 faces.  Returns (fill, camera, h, w, spp, depth, description)."""
    rng = np.random.default_rng(90000 + seed)
    h, w = int(rng.integers(16, 49)), int(rng.integers(16, 65))
    spp, depth = int(rng.integers(1, 4)), int(rng.choice([1, 3, 8]))
    dist = float(10 ** rng.uniform(1, 4.3))
    n = int(rng.choice([8, 64, 300]))
    size = float(10 ** rng.uniform(-3.3, -1.5))
    patch = float(rng.choice([0.01, 0.04, 0.2]))
    thin = float(rng.choice([1.0, 0.1, 0.01]))
    c = rng.uniform(-patch, patch, (n, 1, 3)) * np.array([1, 0.05, 1])
    e = rng.uniform(-size, size, (n, 3, 3))
    e[:, 2] = e[:, 1] * (1 - thin) + e[:, 2] * thin  # third corner close to the second: a sliver
    faces = (c + e).astype(np.float32)
    kmin = int(rng.choice([1, 2, 8, 64]))
    mesh_first = bool(rng.integers(0, 2))
    elev = float(rng.uniform(0.05, 1.4))
    metal = seed % 3 == 0

    def cam(b):
        pos = v3(0.3 * dist * 0.01, dist * np.sin(elev), dist * np.cos(elev))
        b.camera_pinhole(pos, v3(0, 0, 0), v3(0, 1, 0), float(2.0 * np.arctan(1.5 * patch / dist)), w / h)

    def fill(b):
        mat = b.metal(v3(0.9, 0.9, 0.9), 0.0) if metal else b.lambertian(v3(0.8, 0.8, 0.8))
        if not mesh_first:
            b.sky()
        b.bvh(faces, mat, k_min=kmin)
        if mesh_first:
            b.sky()
    probe = rtmi.SceneBuilder(1)
    probe.camera_pinhole(v3(0, 0, 1), v3(0, 0, 0), v3(0, 1, 0), 1.0, 1.0)
    probe.bvh(faces, probe.lambertian(v3(1, 1, 1)), k_min=kmin)
    what = dict(dist=round(dist, 1), n=n, size=round(size, 5), thin=thin, kmin=kmin, mesh_first=mesh_first,
                slivers=int(probe.sliver_faces()))
    return fill, cam, h, w, spp, depth, what


def grazing_world(seed):
    """A sheet of faces of 1 .. 30 cm seen from 30 .. 3e3 away at 0.02 .. 3 degrees above its plane: the regime in
    which the triangle test's determinant is smallest (rays nearly inside the faces' planes).  Returns (fill -- camera
    included --, h, w, spp, depth).  Shared with tools/gpu_check_margins.py."""
    rng = np.random.default_rng(70000 + seed)
    n = int(rng.choice([16, 100, 400]))
    size = float(10 ** rng.uniform(-2, -0.5))
    dist = float(10 ** rng.uniform(1.5, 3.5))
    elev = float(np.radians(10 ** rng.uniform(-1.7, 0.5)))
    patch = 1.0
    c = rng.uniform(-patch, patch, (n, 1, 3)) * np.array([1, 0.002, 1])
    e = rng.uniform(-size, size, (n, 3, 3)) * np.array([1, float(rng.choice([0.0, 0.02, 0.3])), 1])
    faces = (c + e).astype(np.float32)
    kmin = int(rng.choice([1, 4, 64]))
    h, w = 24, 96

    def fill(b):
        pos = v3(0.2 * dist * 0.01, dist * np.sin(elev), dist * np.cos(elev))
        b.camera_pinhole(pos, v3(0, 0, 0), v3(0, 1, 0), float(2.0 * np.arctan(1.2 * patch * max(np.sin(elev), 0.02) / dist)), w / h)
        mat = b.metal(v3(0.9, 0.9, 0.9), 0.0) if seed % 2 else b.lambertian(v3(0.8, 0.8, 0.8))
        b.bvh(faces, mat, k_min=kmin)
        b.sky()
    return fill, h, w, 8, 3


def needle_world(seed):
    """Needles: faces of 1 cm .. 1 m whose third corner sits 1e-2 .. 1e-4 of an edge away from the second (smallest
    angles of 0.5 .. 0.005 degrees), seen from 10 .. 1e4 away; reference leaves of 1 .. 64 faces.  Returns (fill --
    camera included --, h, w, spp, depth).  Shared with tools/gpu_check_margins.py."""
    rng = np.random.default_rng(60000 + seed)
    n = int(rng.choice([8, 64, 300]))
    size = float(10 ** rng.uniform(-2, 0))
    thin = float(10 ** rng.uniform(-4, -2))
    dist = float(10 ** rng.uniform(1, 4))
    patch = float(rng.choice([0.05, 0.5, 2.0]))
    c = rng.uniform(-patch, patch, (n, 1, 3)) * np.array([1, 0.2, 1])
    e = rng.uniform(-size, size, (n, 3, 3))
    e[:, 2] = e[:, 1] * (1 - thin) + e[:, 2] * thin
    faces = (c + e).astype(np.float32)
    kmin = int(rng.choice([1, 2, 8, 64]))
    elev = float(rng.uniform(0.05, 1.4))
    h, w = 32, 48

    def fill(b):
        pos = v3(0.3 * dist * 0.01, dist * np.sin(elev), dist * np.cos(elev))
        b.camera_pinhole(pos, v3(0, 0, 0), v3(0, 1, 0), float(2.0 * np.arctan(1.5 * (patch + size) / dist)), w / h)
        mat = b.metal(v3(0.9, 0.9, 0.9), 0.0) if seed % 3 == 0 else b.lambertian(v3(0.8, 0.8, 0.8))
        if seed % 2:
            b.sky()
        b.bvh(faces, mat, k_min=kmin)
        if not seed % 2:
            b.sky()
    return fill, h, w, 4, 3


def needle_list_world(seed):
    """The needle worlds' faces as Triangle and Parallelogram hitables of the world list (the culled list scan's
    bounds instead of the mesh search's boxes).  Returns (fill -- camera included --, h, w, spp, depth)."""
    rng = np.random.default_rng(61000 + seed)
    n = int(rng.choice([6, 40, 150]))
    size = float(10 ** rng.uniform(-2, 0))
    thin = float(10 ** rng.uniform(-4, -2))
    dist = float(10 ** rng.uniform(1, 4))
    patch = float(rng.choice([0.05, 0.5, 2.0]))
    c = rng.uniform(-patch, patch, (n, 1, 3)) * np.array([1, 0.2, 1])
    e = rng.uniform(-size, size, (n, 3, 3))
    e[:, 2] = e[:, 1] * (1 - thin) + e[:, 2] * thin
    faces = (c + e).astype(np.float32)
    pgram = rng.integers(0, 2, n)
    elev = float(rng.uniform(0.05, 1.4))
    h, w = 32, 48

    def fill(b):
        pos = v3(0.3 * dist * 0.01, dist * np.sin(elev), dist * np.cos(elev))
        b.camera_pinhole(pos, v3(0, 0, 0), v3(0, 1, 0), float(2.0 * np.arctan(1.5 * (patch + size) / dist)), w / h)
        mat = b.metal(v3(0.9, 0.9, 0.9), 0.0) if seed % 3 == 0 else b.lambertian(v3(0.8, 0.8, 0.8))
        if seed % 2:
            b.sky()
        for i in range(n):
            P = [v3(*faces[i, j]) for j in range(3)]
            if pgram[i]:
                b.parallelogram(P, mat)
            else:
                b.triangle(P, mat)
        if not seed % 2:
            b.sky()
    return fill, h, w, 4, 3


def far_sphere_cloud(seed):
    """40 .. 400 spheres of radius 1e-3 .. 1 (one size class per world, or mixed) seen from 10 .. 2e4 away: the grouped
    sphere scan's bounds and binary32 pre-tests at a distance.  Returns (fill -- camera included --, h, w, spp, depth)."""
    rng = np.random.default_rng(62000 + seed)
    n = int(rng.choice([40, 120, 400]))
    rad = float(10 ** rng.uniform(-3, 0))
    mixed = bool(rng.integers(0, 2))
    dist = float(10 ** rng.uniform(1, 4.3))
    patch = float(rng.choice([0.2, 2.0, 20.0]))
    cs = rng.uniform(-patch, patch, (n, 3))
    rs = rad * (10 ** rng.uniform(-1, 1, n) if mixed else np.ones(n))
    elev = float(rng.uniform(0.05, 1.4))
    h, w = 32, 48

    def fill(b):
        pos = v3(0.3 * dist * 0.01, dist * np.sin(elev), dist * np.cos(elev))
        b.camera_pinhole(pos, v3(0, 0, 0), v3(0, 1, 0), float(2.0 * np.arctan(1.5 * (patch + rad) / dist)), w / h)
        mats = [b.lambertian(v3(0.8, 0.8, 0.8)), b.metal(v3(0.9, 0.9, 0.9), 0.0), b.dielectric(v3(1, 1, 1), 1.5)]
        if seed % 2:
            b.sky()
        for i in range(n):
            b.sphere(v3(*cs[i]), float(rs[i]), mats[i % 3])
        if not seed % 2:
            b.sky()
    return fill, h, w, 4, 6


def random_world(b, rng, n_objects, many_materials=False):
    def col(lo=0.05, hi=0.95):
        return v3(*rng.uniform(lo, hi, 3))

    mats = []
    n_mats = 300 if many_materials else int(rng.integers(3, 9))
    for _ in range(n_mats):
        k = rng.integers(0, 10)
        if k < 5:
            mats.append(b.lambertian(col()))
        elif k < 7:
            mats.append(b.metal(col(0.3, 1.0), float(rng.choice([0.0, rng.uniform(0.05, 0.9), 1.7]))))
        elif k < 9:
            mats.append(b.dielectric(col(0.7, 1.0), float(rng.uniform(1.1, 2.0))))
        else:
            mats.append(b.diffuse_light(b.constant_texture(col(1.0, 6.0))))
    light = b.diffuse_light(b.constant_texture(v3(5, 5, 5)))

    def pick():
        return mats[int(rng.integers(0, len(mats)))]

    b.sphere(v3(0, -100.5, -1), 100.0, mats[0])
    sky_at = int(rng.integers(0, n_objects))
    for i in range(n_objects):
        if i == sky_at:
            b.sky()
        c = rng.uniform(-2.5, 2.5, 3)
        c[1] = abs(c[1]) * 0.6
        c[2] -= 2.0
        k = rng.integers(0, 6)
        if k == 0:
            b.sphere(v3(*c), float(rng.uniform(0.15, 0.6)), pick())
        elif k == 1:
            e1, e2 = rng.uniform(-0.8, 0.8, 3), rng.uniform(-0.8, 0.8, 3)
            b.parallelogram([v3(*c), v3(*(c + e1)), v3(*(c + e2))], pick())
        elif k == 2:
            e = rng.uniform(0.2, 0.7, 3)
            b.parallelepiped([v3(*c), v3(c[0] + e[0], c[1], c[2]), v3(c[0], c[1] + e[1], c[2]),
                              v3(c[0], c[1], c[2] + e[2])], pick())
        elif k == 3:
            b.triangle([v3(*c), v3(*(c + rng.uniform(-0.9, 0.9, 3))), v3(*(c + rng.uniform(-0.9, 0.9, 3)))], pick())
        elif k == 4:
            ang = np.float32(rng.uniform(0, 3.0))
            off = v3(*c)
            from rtmi.scenes import rotate_y
            b.parallelepiped_lengths(v3(*rng.uniform(0.2, 0.7, 3)), pick(), lambda p, a=ang, o=off: rotate_y(p, a) + o)
        else:
            n = int(rng.integers(1, 40))
            base = rng.uniform(-0.4, 0.4, (n, 1, 3)) + c
            faces = (base + rng.uniform(-0.25, 0.25, (n, 3, 3))).astype(np.float32)
            b.bvh(faces, pick(), k_min=int(rng.choice([2, 8, 2048])))
    b.parallelogram([v3(-1, 3.5, -3), v3(1, 3.5, -3), v3(-1, 3.5, -1)], light)


def random_case(seed):
    """A seeded random world with its frame, depth limit, post / raw mode and camera (pinhole or defocus).  Returns
    (fill -- camera included --, h, w, spp, depth, post, n_objects)."""
    rng = np.random.default_rng(1000 + seed)
    h, w = int(rng.integers(9, 41)), int(rng.integers(9, 57))
    spp, depth = int(rng.integers(1, 7)), int(rng.choice([1, 3, 10, 25, 64]))
    post = bool(rng.integers(0, 2))
    n_objects = int(rng.integers(3, 14))
    state = rng.bit_generator.state

    def fill(b):
        rng.bit_generator.state = state  # every builder sees the same random stream
        if seed % 4 == 3:
            b.camera_defocus(v3(0, 1.0, 2.5), v3(0, 0.4, -2), v3(0, 1, 0), PI_D / 3, w / h, 0.2, 4.0)
        else:
            b.camera_pinhole(v3(0, 1.0, 2.5), v3(0, 0.4, -2), v3(0, 1, 0), PI_D / 3, w / h)
        random_world(b, rng, n_objects, seed % 6 == 5)
    return fill, h, w, spp, depth, post, n_objects


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


def scheduler_mesh_world(seed):
    """Mesh-heavy random worlds at a frame large enough for the scheduler to matter: one to three copies of a bunny
    mesh on a sphere or a parallelogram.  Returns (fill -- camera included --, h, w, spp, depth)."""
    from rtmi.scenes import procedural_bunny_mesh
    rng = np.random.default_rng(500 + seed)
    h, w, spp, depth = 192, 256, 64, int(rng.choice([6, 12, 30]))
    mesh = procedural_bunny_mesh(int(rng.integers(10, 24)))
    copies = [(int(rng.integers(0, 3)), int(rng.choice([4, 64, 2048]))) for _ in range(int(rng.integers(1, 4)))]

    def fill(b):
        b.camera_pinhole(v3(0.0, 0.16, -0.55), v3(0.0, 0.1, 0.0), v3(0, 1, 0), PI_D / 4, w / h)
        mats = [b.lambertian(v3(1, 1, 1)), b.metal(v3(0.9, 0.85, 0.8), 0.05), b.dielectric(v3(0.95, 0.95, 1.0), 1.4)]
        for k, (mat, k_min) in enumerate(copies):
            off = np.array([0.17 * (k - 1), 0.0, 0.05 * k], dtype=np.float32)
            b.bvh((mesh + off).astype(np.float32), mats[mat], k_min=k_min)
        if seed % 2:
            b.sphere(v3(0, -100.0 + 0.03, 0), 100.0, b.lambertian(v3(0.5, 0.6, 0.5)))
        else:
            b.parallelogram([v3(-5, 0.03, -5), v3(5, 0.03, -5), v3(-5, 0.03, 5)], b.lambertian(v3(0.5, 0.6, 0.5)))
        b.sky()
    return fill, h, w, spp, depth


# (shards, render options) of the ways such a world is rendered; all must give the first one's frame
SCHEDULER_PATHS = ((1, dict(schedule=0)),                    # image order
                   (1, dict(schedule=2)),                    # forced longest-first
                   (2, dict(schedule=2)),                    # as two interleaved shards
                   (1, dict(schedule=2, sparse_stride=1)),   # outlier pixels packed 64 to a wave
                   (1, dict(schedule=2, sparse_stride=64)),  # ... or one to a wave
                   (1, dict(schedule=2, exclusive=0)))       # ... or sharing their wave with ordinary pixels


# ------------------------------------------------------------------ the slow-form camera (tests/test_deferred_normalise_host.py)
F32 = np.float32
SIDE = 64
# v.v / A^2 = x^2 + y^2 is at most 1 + (65 / 64)^2 = 2.0315 in the corner pixel and at most (63 / 64)^2 + (65 / 64)^2 =
# 2.0004 or 1 + 1 = 2 outside it: 2^100 / A^2 = 2.004 lies between, about 0.39 of the corner pixel's area beyond it
SLOW_A = F32(2.0 ** 50 / np.sqrt(2.004))
SLOW_ORIGIN = np.array([278, 278, 100], dtype=F32)  # inside the Cornell box, looking along +x / +y at two of its walls


def slow_camera():
    """(position, lower-left corner, horizontal, vertical) of the raw camera."""
    return SLOW_ORIGIN, SLOW_ORIGIN.copy(), np.array([SLOW_A, 0, 0], dtype=F32), np.array([0, SLOW_A, 0], dtype=F32)
