"""What the texel tests share (tests/test_texlib_host.py, tests/test_gpu_texel.py, tests/test_gpu_features.py):
ImageTexture::Value and the sphere's GetUV restated in numpy, a set of high-contrast textures in which no two texels share
a colour, two enclosed worlds that carry them on spheres, parallelograms and a mesh, and the ray families aimed at the
places where a lookup can go wrong -- texel centres and boundaries, the seam, the poles, the axes.  No test lives here."""
import collections
import functools

import numpy as np

import oraclelib
from querylib import Recorder, v3

F32 = np.float32
PI_F = F32(3.14159265358979323846264338327950288)


# ------------------------------------------------------------------ ImageTexture::Value, restated
def texel_index(h, w, u, v):
    """(row, column) ImageTexture::Value reads (image_texture.cu:9-38 as oracle.cc restates it): the flip in binary64,
    then binary32 wrap, scale, floor and clamp.  u, v binary64 from the record."""
    v = 1.0 - float(v)
    fu, fv = F32(u), F32(v)
    fu, fv = F32(fu - np.floor(fu)), F32(fv - np.floor(fv))
    ix, iy = int(np.floor(F32(fu * F32(w)))), int(np.floor(F32(fv * F32(h))))
    return max(0, min(iy, h - 1)), max(0, min(ix, w - 1))


def image_value(rgba, u, v):
    """ImageTexture::Value (image_texture.cu:9-38 as oracle.cc restates it): u, v binary64 from the record."""
    iy, ix = texel_index(rgba.shape[0], rgba.shape[1], u, v)
    return rgba[iy, ix, :3].astype(F32) / F32(255.0)


# ------------------------------------------------------------------ Sphere::GetUV, with acos / atan2 in binary64
def sphere_uv_truth(n):
    """sphere.cu:60-63 on binary32 normals n (.., 3): acos and atan2 are taken in binary64 (numpy's arctan2 honours signed
    zeros) and rounded once; every other step is the source's own binary32 operation.  Returns (u, v), float32."""
    n = np.asarray(n, dtype=F32)
    x, y, z = n[..., 0], n[..., 1], n[..., 2]
    theta = np.arccos((-y).astype(np.float64)).astype(F32)
    phi = (np.arctan2((-z).astype(np.float64), x.astype(np.float64)).astype(F32) + PI_F).astype(F32)
    u = (phi / (F32(2) * PI_F)).astype(F32)
    v = (theta / PI_F).astype(F32)
    return u, v


# ------------------------------------------------------------------ the textures
SHAPES = [(1, 1), (1, 7), (7, 1), (5, 3), (16, 36), (64, 64), (63, 65), (3, 1000)]  # (height, width)
LIGHT_SHAPE = (6, 10)  # the image of the textured emitter
PITCHED = SHAPES.index((63, 65))  # 4 * 65 is no pitch hipMallocPitch hands out
COLUMN_STRIDE = {(3, 1000): 5}  # `centres` visits every fifth column of the widest image


def distinct_image(rng, h, w):
    """Uniform random RGBA8 in which no two texels have the same colour (duplicates are drawn again)."""
    img = rng.integers(0, 256, (h, w, 4), dtype=np.uint8)
    while True:
        rgb = img.reshape(-1, 4)[:, :3].astype(np.uint32)
        key = rgb[:, 0] | (rgb[:, 1] << 8) | (rgb[:, 2] << 16)
        _, first, counts = np.unique(key, return_index=True, return_counts=True)
        if (counts == 1).all():
            return img
        dup = np.setdiff1d(np.arange(h * w), first)
        img.reshape(-1, 4)[dup] = rng.integers(0, 256, (len(dup), 4), dtype=np.uint8)


@functools.lru_cache(maxsize=None)
def textures():
    """The images of SHAPES, then the emitter's."""
    rng = np.random.default_rng(2024)
    return [distinct_image(rng, h, w) for h, w in SHAPES + [LIGHT_SHAPE]]


def padded_rows(img, width):
    """img's rows inside rows of `width` texels; the padding holds a colour no texel of img has (asserted)."""
    h, w = img.shape[:2]
    colours = {tuple(c) for c in img.reshape(-1, 4)[:, :3].tolist()}
    pad = next(c for c in ((a, a, 255 - a) for a in range(256)) if c not in colours)
    out = np.empty((h, width, 4), dtype=np.uint8)
    out[:, :, :3] = pad
    out[:, :, 3] = 7
    out[:, :w] = img
    assert not (out[:, w:, :3].reshape(-1, 1, 3) == img[:, :, :3].reshape(1, -1, 3)).all(2).any()
    return out


# ------------------------------------------------------------------ the worlds
LIGHT = len(SHAPES)  # index of the emitter's image in textures()
L_BOX = 14.0
# centre, radius, image: power-of-two and other radii, centres with zero and non-zero components.  Rays start at
# c + 3 r n: the balls of radius 3 r around the centres meet neither each other's spheres nor the flat surfaces of tex_all.
SPHERES = [((-7, -7, 0), 1.5, 0), ((0, -7, 0), 0.5, 1), ((7, -7, 0), 1.25, 2), ((-7, 0, 0), 0.75, 3),
           ((7, 0, 0.75), 1.3, 4), ((-7, 7, 0), 1.4, 5), ((0, 7, 0), 1.0, PITCHED), ((7, 7, 0), 1.5, 7),
           ((0, 0, 4), 1.25, LIGHT)]
MESH_TEX = 4
MESH_AT = (-2.0, -2.0)
CAMERA = ((0, 0, 13), (0, 0, 0), (0, 1, 0), 1.2)

# texture ids and material ids by image (index into textures()), the enclosure's material, the plain mesh's (or None)
Layout = collections.namedtuple("Layout", "texs mats white plain")


def fill(b, name, aspect=1.0, upload=None):
    """tex_spheres: a closed box of constant white light around one Lambertian sphere per image of SHAPES and one
    emitting sphere of the light's image.  tex_all: the same, plus a stack of unit parallelograms p0 = (0, 0, -k),
    e1 = x, e2 = y, one per image (the last one emits), a two-face mesh with uvs, and a plain mesh.  `upload(b, k, img)`
    replaces b.image_texture for image k."""
    assert name in ("tex_spheres", "tex_all")
    pos, at, up, fov = CAMERA
    b.camera_pinhole(v3(*pos), v3(*at), v3(*up), fov, aspect)
    texs = [(upload or (lambda b, k, img: b.image_texture(img)))(b, k, img) for k, img in enumerate(textures())]
    mats = [b.diffuse_light(t) if k == LIGHT else b.lambertian_tex(t) for k, t in enumerate(texs)]
    white = b.diffuse_light(b.constant_texture(v3(1, 1, 1)))
    L = L_BOX
    b.parallelepiped([v3(-L, -L, -L), v3(L, -L, -L), v3(-L, L, -L), v3(-L, -L, L)], white)
    for c, r, k in SPHERES:
        b.sphere(v3(*c), r, mats[k])
    plain = None
    if name == "tex_all":
        for k in range(len(mats)):
            b.parallelogram([v3(0, 0, -k), v3(1, 0, -k), v3(0, 1, -k)], mats[k])
        x, y = MESH_AT
        faces = np.array([[[x, y, 0], [x + 1, y, 0], [x, y + 1, 0]], [[x + 1, y, 0], [x + 1, y + 1, 0], [x, y + 1, 0]]], dtype=F32)
        uvs = np.array([[0.0, 0.0, 1.0, 0.0, 0.0, 1.0], [1.0, 0.0, 1.0, 1.0, 0.0, 1.0]], dtype=F32)
        b.bvh(faces, mats[MESH_TEX], uvs=uvs, k_min=2048)
        plain = b.lambertian(v3(0.25, 0.5, 0.75))
        b.bvh(faces * F32(0.5) + np.array([2.5, -0.5, 0], dtype=F32), plain, k_min=2048)
    return Layout(texs, mats, white, plain)


def material_image(layout):
    """material id -> its image (textured materials only)."""
    return {m: textures()[k] for k, m in enumerate(layout.mats)}


def build(name, aspect=1.0, upload=None, seed=7):
    """(committed product scene, its Recorder, oracle builder, Layout, seed)."""
    import rtmi
    rec = Recorder(rtmi.SceneBuilder(seed))
    lay = fill(rec, name, aspect, upload)
    ob = build_oracle(name, aspect, seed)[0]
    rec.b.commit()
    return rec.b, rec, ob, lay, seed


def build_oracle(name, aspect=1.0, seed=7):
    ob = oraclelib.OracleBuilder(seed)
    return ob, fill(ob, name, aspect)


def pitched_upload(width):
    """An `upload` for fill(): image PITCHED through the C ABI from rows of `width` texels, the others packed."""
    import ctypes as C
    import rtmi

    def upload(b, k, img):
        if k != PITCHED:
            return b.image_texture(img)
        rows = padded_rows(img, width)
        b._keep.append(rows)
        t = rtmi.lib().rtmi_image_texture(b.h, rows.ctypes.data_as(C.POINTER(C.c_uint8)), img.shape[0], img.shape[1], 4 * width)
        assert t >= 0
        return t
    return upload


# ------------------------------------------------------------------ the ray families
FAMILIES = ("centres", "edges", "seam", "poles", "axes", "pgram", "mesh")
SPHERE_FAMILIES = FAMILIES[:5]
TINY = (1.4e-45, 1e-40, 2.0 ** -126, 1e-7, 1e-4)  # the smallest subnormal, a subnormal, the smallest normal, ..
ULPS = (0, 1, -1, 2, -2, 4, -4)
COARSE_ULPS = (1, -1, 2, -2, 4, -4, 16, -16)

# O, D (N, 3) float32; family (N,) index into FAMILIES; target (N,): the sphere (index into SPHERES) or the image of the
# flat surface; info (N, 3) int: centres (row, column, 0); edges (0: a column boundary u = k / W | 1: a row boundary
# v = k / H, k, the row | column the ray is aimed at); else zeros
Rays = collections.namedtuple("Rays", "O D family target info")


def normal_at(u, v):
    """The binary64 unit normal whose GetUV is (u, v); a component that is zero but for the rounding of pi is zero, so
    that an origin on the seam or on an axis can be stepped across it by ulps of zero."""
    theta, a = np.pi * np.asarray(v, dtype=np.float64), 2 * np.pi * np.asarray(u, dtype=np.float64) - np.pi
    n = np.stack([np.sin(theta) * np.cos(a), -np.cos(theta), -np.sin(theta) * np.sin(a)], axis=-1)
    return np.where(np.abs(n) < 1e-12, 0.0, n)


def tangent_at(u, v, axis):
    """d normal / du (axis 0) or / dv (axis 1), up to scale."""
    theta, a = np.pi * np.asarray(v, dtype=np.float64), 2 * np.pi * np.asarray(u, dtype=np.float64) - np.pi
    if axis == 0:
        return np.stack([-np.sin(theta) * np.sin(a), 0 * a, -np.sin(theta) * np.cos(a)], axis=-1)
    return np.stack([np.cos(theta) * np.cos(a), np.sin(theta), -np.cos(theta) * np.sin(a)], axis=-1)


def step_ulps(x, k):
    """float32 x moved k units in the last place (towards +inf for k > 0)."""
    x = np.asarray(x, dtype=F32).copy()
    for _ in range(abs(int(k))):
        x = np.nextafter(x, F32(np.inf if k > 0 else -np.inf))
    return x


def from_normals(c, r, n):
    """Origin c + 3 r n and direction -n, in binary32."""
    n = np.asarray(n).astype(F32).reshape(-1, 3)
    O = (np.asarray(c, dtype=F32) + (F32(3) * F32(r)) * n).astype(F32)
    return O, (-n).astype(F32)


def centre_uv(h, w, iy, ix):
    """The (u, v) at the middle of texel (iy, ix): Value flips v."""
    return (np.asarray(ix) + 0.5) / w, 1.0 - (np.asarray(iy) + 0.5) / h


def sphere_rays(s):
    """The five families on sphere s of SPHERES: lists of (family, O, D, info)."""
    c, r, k = SPHERES[s]
    h, w = textures()[k].shape[:2]
    out = []
    # centres
    iy, ix = np.meshgrid(np.arange(h), np.arange(0, w, COLUMN_STRIDE.get((h, w), 1)), indexing="ij")
    iy, ix = iy.reshape(-1), ix.reshape(-1)
    O, D = from_normals(c, r, normal_at(*centre_uv(h, w, iy, ix)))
    out.append(("centres", O, D, np.stack([iy, ix, 0 * ix], axis=1)))
    # edges: every boundary, the origin stepped across it
    for axis, other in ((0, h), (1, w)):
        for kb in (range(w + 1) if axis == 0 else range(1, h)):  # (v = 0 and v = 1 are the poles' family)
            aim = kb % other
            if axis == 0:
                u, v = kb / w, centre_uv(h, w, aim, 0)[1]
            else:
                u, v = centre_uv(h, w, 0, aim)[0], kb / h
            O0, D0 = from_normals(c, r, normal_at(u, v))
            j = int(np.argmax(np.abs(tangent_at(u, v, axis))))
            # ulps of the component itself -- of zero on the seam, where subnormals choose between u = 0 and u = 1.0
            # exactly, which both read column 0 -- and ulps of the origin's largest component: the hit point is rounded
            # to those, and on the seam they reach the float below 1.0, the last column
            steps = [step_ulps(O0[0, j], e) for e in ULPS]
            steps += [F32(O0[0, j] + F32(e) * np.spacing(np.abs(O0).max())) for e in COARSE_ULPS]
            O = np.repeat(O0, len(steps), axis=0)
            O[:, j] = steps
            out.append(("edges", O, np.repeat(D0, len(steps), axis=0), np.tile([axis, kb, aim], (len(steps), 1))))
    # seam and poles: a component is (origin offset, direction); signed zeros go into both, each sign on its own
    zeros = [(F32(a), F32(b)) for a in (0.0, -0.0) for b in (0.0, -0.0)]
    r3 = F32(3) * F32(r)
    tiny = [(F32(r3 * F32(sg * t)), F32(-sg * t)) for t in TINY for sg in (1, -1)]

    def place(cj, off):
        return off if cj == 0 else F32(F32(cj) + off)  # (0 + -0 is +0: a zero centre keeps the offset's sign)

    O, D = [], []
    for oz, dz in zeros + tiny:
        O.append([F32(c[0]) - r3, F32(c[1]), place(c[2], oz)]), D.append([F32(1), F32(0), dz])
    out.append(("seam", np.array(O, dtype=F32), np.array(D, dtype=F32), np.zeros((len(O), 3), int)))
    O, D = [], []
    same_sign = [zeros[0], zeros[3]]
    for sy in (1, -1):
        for ox, dx in zeros + tiny:
            for oz, dz in (zeros if (ox, dx) in zeros else same_sign) + tiny:
                O.append([place(c[0], ox), F32(c[1]) + F32(sy) * r3, place(c[2], oz)]), D.append([dx, F32(-sy), dz])
    out.append(("poles", np.array(O, dtype=F32), np.array(D, dtype=F32), np.zeros((len(O), 3), int)))
    O, D = from_normals(c, r, [(1, 0, 0), (-1, 0, 0), (0, 0, 1), (0, 0, -1)])
    out.append(("axes", O, D, np.zeros((4, 3), int)))
    return out


def axis_values(n):
    """The coordinates a flat family visits along an axis of n texels: k / n and its two float neighbours, the texels'
    middles, 0, 1, 1 - 2^-24, 2^-24 .. 2^-60."""
    k = (np.arange(n + 1, dtype=np.float64) / n).astype(F32)
    vals = np.concatenate([k, np.nextafter(k[1:], F32(0)), np.nextafter(k[:-1], F32(1)), ((np.arange(n) + 0.5) / n).astype(F32),
                           [0.0, 1.0, 1.0 - 2.0 ** -24], 2.0 ** -np.arange(24.0, 61.0, 4.0)]).astype(F32)
    return np.unique(vals)


def flat_points(h, w):
    """(x, y) in the unit square: x over the column values at a row's middle and at y = 0, y over the row values at
    x = 0 (where the parallelogram's v is 1 - y exactly) and at a column's middle."""
    xs, ys = axis_values(w), axis_values(h)
    x_mid, y_mid = F32((w // 2 + 0.5) / w), F32((h // 2 + 0.5) / h)
    pts = [(x, y0) for y0 in (y_mid, F32(0)) for x in xs] + [(x0, y) for x0 in (F32(0), x_mid) for y in ys]
    return np.array(pts, dtype=F32)


def flat_rays(family, k):
    """Rays along -z onto the unit square of parallelogram k of the stack, or of the mesh."""
    h, w = textures()[k].shape[:2]
    p = flat_points(h, w)
    x0, y0, z0 = (0.0, 0.0, -float(k)) if family == "pgram" else (MESH_AT[0], MESH_AT[1], 0.0)
    O = np.stack([F32(x0) + p[:, 0], F32(y0) + p[:, 1], np.full(len(p), z0 + 0.25, dtype=F32)], axis=1).astype(F32)
    D = np.tile(np.array([0, 0, -1], dtype=F32), (len(p), 1))
    return O, D, p


@functools.lru_cache(maxsize=None)
def rays(name):
    """Every family of world `name` as one Rays."""
    O, D, fam, tgt, info = [], [], [], [], []

    def add(family, o, d, t, i):
        O.append(o), D.append(d), info.append(np.asarray(i, dtype=np.int64).reshape(len(o), 3))
        fam.append(np.full(len(o), FAMILIES.index(family))), tgt.append(np.full(len(o), t))

    for s in range(len(SPHERES)):
        for family, o, d, i in sphere_rays(s):
            add(family, o, d, s, i)
    if name == "tex_all":
        for k in range(len(textures())):
            o, d, p = flat_rays("pgram", k)
            add("pgram", o, d, k, np.zeros((len(o), 3)))
        o, d, p = flat_rays("mesh", MESH_TEX)
        add("mesh", o, d, MESH_TEX, np.zeros((len(o), 3)))
    return Rays(np.ascontiguousarray(np.concatenate(O), dtype=F32), np.ascontiguousarray(np.concatenate(D), dtype=F32),
                np.concatenate(fam), np.concatenate(tgt), np.concatenate(info))


def family(r, name):
    return np.flatnonzero(r.family == FAMILIES.index(name))


def oracle_primary_rays(ob, h, w):
    """The oracle's camera rays of the first sample of every pixel of an h x w frame, row-major: RenderPixel's
    binary64 coordinates (oracle.cc) from the two jitter draws, then RayAt."""
    import ctypes as C
    L = oraclelib.lib()
    states = oraclelib.rng_init(ob.seed, h * w)
    states[0] = ob.state0
    rays_ = np.zeros((h * w, 6), dtype=F32)
    for p in range(h * w):
        st = states[p]
        ptr = st.ctypes.data_as(C.POINTER(C.c_uint32))
        r1 = float(L.orc_random_float(C.c_float(0.0), C.c_float(1.0), ptr))
        r2 = float(L.orc_random_float(C.c_float(0.0), C.c_float(1.0), ptr))
        i, j = divmod(p, w)
        x, y = (r1 + float(j)) / float(w), (r2 + float(h - i)) / float(h)
        rays_[p] = ob.probe_camera_ray(2 * x - 1, 2 * y - 1, st)
    return np.ascontiguousarray(rays_[:, :3]), np.ascontiguousarray(rays_[:, 3:])


def sphere_census(layout, O, D, t, mat):
    """(rays whose hit lies on a textured Lambertian sphere, rays whose hit lies on the textured light's sphere): by
    the hit's material and its distance from that sphere's centre (tex_all has the same materials on flat surfaces)."""
    with np.errstate(all="ignore"):
        Dn = D / np.linalg.norm(D, axis=1, keepdims=True)
    P = O.astype(np.float64) + np.asarray(t, dtype=np.float64)[:, None] * Dn
    count = [0, 0]
    for c, r, k in SPHERES:
        on = (np.asarray(mat) == layout.mats[k]) & (np.abs(np.linalg.norm(P - np.array(c, dtype=np.float64), axis=1) - r) < 1e-3)
        count[k == LIGHT] += int(on.sum())
    return tuple(count)


def oracle_records(ob, O, D):
    """probe_hit of every ray: hit (N,) bool, out (N, 6) float64 {t, u, v, normal}, material (N,)."""
    hit, out, mat = np.zeros(len(O), bool), np.zeros((len(O), 6)), np.full(len(O), -1, np.int32)
    for i in range(len(O)):
        hit[i], out[i], mat[i] = ob.probe_hit(O[i], D[i])
    return hit, out, mat
