"""What the ray-query tests share (rtmi_intersect, rtmi_occluded, rtmi_trace and the tests built on them): the recording
builder, the query worlds, the ray families, the device calls and the comparison with OracleBuilder.probe_hit."""
import numpy as np
import torch

import common
import oraclelib
import rtmi
from parity import bits

ADDS = {"sphere": rtmi.RTMI_HIT_SPHERE, "triangle": rtmi.RTMI_HIT_TRIANGLE, "parallelogram": rtmi.RTMI_HIT_PARALLELOGRAM,
        "parallelepiped": rtmi.RTMI_HIT_PARALLELEPIPED, "parallelepiped_lengths": rtmi.RTMI_HIT_PARALLELEPIPED,
        "sky": rtmi.RTMI_HIT_SKY, "bvh": rtmi.RTMI_HIT_MESH}

SPHERE_UV_TOL = 1e-6  # device acosf / atan2f against the host's (the birthday scene's texel tolerance rests on the same)


class Recorder:
    """A builder that passes every call on and keeps the list of them (entries are the rtmi_add_* calls)."""

    def __init__(self, b):
        self.b, self.calls = b, []

    def __getattr__(self, name):
        f = getattr(self.b, name)
        if not callable(f):
            return f

        def call(*a, **k):
            r = f(*a, **k)
            self.calls.append((name, a, k))
            return r
        return call

    def entries(self):
        return [c for c in self.calls if c[0] in ADDS]


def v3(x, y, z):
    return np.array([x, y, z], dtype=np.float32)


# ------------------------------------------------------------------ worlds
def _cam(b, pos=(0, 1, 6), at=(0, 0, 0)):
    b.camera_pinhole(v3(*pos), v3(*at), v3(0, 1, 0), 0.9, 1.0)


def world_no_sky(b):
    _cam(b)
    m = [b.lambertian(v3(0.8, 0.3, 0.3)), b.metal(v3(0.9, 0.9, 0.9), 0.1), b.dielectric(v3(1, 1, 1), 1.5)]
    b.sphere(v3(0, 0, 0), 1.0, m[0])
    b.sphere(v3(1.5, 0.2, -0.5), 0.6, m[1])
    b.parallelogram([v3(-4, -1, -4), v3(4, -1, -4), v3(-4, -1, 4)], m[0])
    b.triangle([v3(-2, 0, -2), v3(-1, 2, -2), v3(-3, 1.5, -1)], m[2])
    b.parallelepiped([v3(2, -1, 1), v3(3, -1, 1), v3(2, 0, 1), v3(2, -1, 2)], m[1])


def world_empty(b):
    _cam(b)


def world_nested(b):
    _cam(b)
    m = b.lambertian(v3(0.5, 0.7, 0.2))
    n = b.metal(v3(0.7, 0.7, 0.7), 0.0)
    b.sphere(v3(0, -100.5, 0), 100.0, m)
    b.list_begin()
    b.sphere(v3(0, 0, 0), 0.5, n)
    b.list_begin()
    b.triangle([v3(-1, 0, -1), v3(1, 0, -1), v3(0, 1.5, -1)], m)
    b.parallelogram([v3(-2, -0.5, -2), v3(2, -0.5, -2), v3(-2, 2, -2)], n)
    b.list_end()
    b.sphere(v3(0.8, 0.1, 0.5), 0.3, m)
    b.list_end()
    b.sky()
    b.parallelepiped([v3(-1.5, -0.5, 0.5), v3(-1, -0.5, 0.5), v3(-1.5, 0.5, 0.5), v3(-1.5, -0.5, 1)], m)


def quilt(n_pairs, seed=0):
    def fill(b):
        rng = np.random.default_rng(seed + n_pairs)
        _cam(b, (0, 0, 8))
        mats = [b.lambertian(v3(0.8, 0.8, 0.8)), b.metal(v3(0.9, 0.9, 0.9), 0.0)]
        b.sky()
        for i in range(n_pairs):
            c = rng.uniform(-2.5, 2.5, 3).astype(np.float32)
            e = rng.uniform(-0.6, 0.6, (2, 3)).astype(np.float32)
            P = [c, c + e[0], c + e[1]]
            if i % 2:
                b.parallelogram(P, mats[i % 2])
            else:
                b.triangle(P, mats[i % 2])
    return fill


def many_materials(b):
    rng = np.random.default_rng(5)
    _cam(b, (0, 0, 8))
    b.sky()
    for i in range(600):
        m = b.lambertian(v3(i / 600, 0.5, 1 - i / 600))
        c = rng.uniform(-2.5, 2.5, 3).astype(np.float32)
        e = rng.uniform(-0.4, 0.4, (2, 3)).astype(np.float32)
        b.triangle([c, c + e[0], c + e[1]], m)


def textured_mesh(b):
    """A mesh with texture coordinates (Face<true>) next to one without, after a list: u, v interpolated per face."""
    _cam(b, (0, 1.5, 4))
    faces = common.small_mesh(6)
    uvs = np.random.default_rng(3).uniform(0, 1, (faces.shape[0], 6)).astype(np.float32)
    m = b.lambertian(v3(0.6, 0.6, 0.6))
    b.sky()
    b.parallelogram([v3(-3, -1.2, -3), v3(3, -1.2, -3), v3(-3, -1.2, 3)], m)
    b.bvh(faces, m, uvs=uvs, k_min=16)
    b.bvh(faces * np.float32(0.5) + np.float32(1.1), m, k_min=2048)

SCENE_WORLDS = ["cornell_box", "spheres", "bunny", "bunny_kmin4", "birthday", "mixed", "furnace", "sky_only"]

CUSTOM_WORLDS = {"no_sky": world_no_sky, "empty": world_empty, "nested": world_nested, "quilt_3": quilt(3),
                 "quilt_40": quilt(40), "quilt_300": quilt(300), "materials_600": many_materials,
                 "textured_mesh": textured_mesh}


def build(name):
    """(product scene, its Recorder, oracle builder, seed)."""
    if name in CUSTOM_WORLDS:
        seed = 7
        rec = Recorder(rtmi.SceneBuilder(seed))
        ob = oraclelib.OracleBuilder(seed)
        CUSTOM_WORLDS[name](rec)
        CUSTOM_WORLDS[name](ob)
    else:
        scene, kw = name, {}
        if name == "bunny_kmin4":
            scene, kw = "bunny", {"k_min": 4}
        seed = common.scene_seed(scene)
        rec = Recorder(rtmi.SceneBuilder(seed))
        common.build_scene(rec, scene, 1.0, **kw)
        ob = common.build_scene(oraclelib.OracleBuilder(seed), scene, 1.0, **kw)
    rec.b.commit()
    return rec.b, rec, ob, seed


def one_primitive_world(rec, seed, entry, element):
    """An oracle world holding only entry `entry` (a mesh entry: only its face `element`), materials and camera as
    recorded."""
    ob = oraclelib.OracleBuilder(seed)
    k = -1
    for name, a, kw in rec.calls:
        if name in ("list_begin", "list_end", "random_float"):
            continue
        if name in ADDS:
            k += 1
            if k != entry:
                continue
            if name == "bvh":
                faces = np.asarray(a[0], dtype=np.float32).reshape(-1, 9)[element:element + 1]
                kw = dict(kw)
                if kw.get("uvs") is not None:
                    kw["uvs"] = np.asarray(kw["uvs"], dtype=np.float32).reshape(-1, 6)[element:element + 1]
                a = (faces,) + tuple(a[1:])
        getattr(ob, name)(*a, **kw)
    return ob


# ------------------------------------------------------------------ rays
def oracle_answers(ob, O, D):
    hit = np.zeros(len(O), dtype=bool)
    out = np.zeros((len(O), 6))
    mat = np.full(len(O), -1, dtype=np.int32)
    for i in range(len(O)):
        h, o, m = ob.probe_hit(O[i], D[i])
        hit[i], out[i], mat[i] = h, o, m
    return hit, out, mat


def unit_vectors(rng, n):
    v = rng.normal(size=(n, 3))
    return (v / np.linalg.norm(v, axis=1, keepdims=True)).astype(np.float32)


def make_rays(ob, seed, n_family=1000):
    """Camera rays, secondary rays from their first hits, random origins inside and far outside the scene's bounds,
    axis-aligned and grazing rays.  float32 (N, 3) origins and directions."""
    rng = np.random.default_rng(seed)
    states = oraclelib.rng_init(seed, n_family)
    cam = np.array([ob.probe_camera_ray(rng.random(), rng.random(), states[i]) for i in range(n_family)], dtype=np.float32)
    O, D = [cam[:, :3]], [cam[:, 3:]]
    hit, out, _ = oracle_answers(ob, cam[:, :3], cam[:, 3:])
    solid = hit & (out[:, 0] < 1e8)  # (not Sky)
    pos = cam[0, :3]
    if solid.any():
        t = out[solid, 0].astype(np.float32)[:, None]
        P = cam[solid, :3] + t * cam[solid, 3:]  # ray_tracing.cu:32 in binary32
        N = out[solid, 3:6].astype(np.float32)
        # secondary rays from the hit points: self-intersection at 1e-3 is the reference's to decide
        O.append(P), D.append(unit_vectors(rng, len(P)))
        O.append(P), D.append(N + unit_vectors(rng, len(P)))
        # grazing: nearly inside the hit surface's plane, aimed at the hit point from a little way off
        tang = np.cross(N, unit_vectors(rng, len(P))).astype(np.float32)
        tang /= np.maximum(np.linalg.norm(tang, axis=1, keepdims=True), 1e-12).astype(np.float32)
        g = (tang + np.float32(1e-3) * rng.uniform(-1, 1, (len(P), 1)).astype(np.float32) * N).astype(np.float32)
        O.append((P - np.float32(0.5) * g).astype(np.float32)), D.append(g)
        lo, hi = P.min(0), P.max(0)
    else:
        lo, hi = pos - 2, pos + 2
    ext = np.maximum(hi - lo, 1e-2)
    inside = (lo + rng.random((n_family, 3)) * ext).astype(np.float32)
    O.append(inside), D.append(unit_vectors(rng, n_family))
    far = (lo + ext / 2 + unit_vectors(rng, n_family) * np.float32(50 * ext.max())).astype(np.float32)
    aim = (lo + rng.random((n_family, 3)) * ext).astype(np.float32)
    O.append(far), D.append((aim - far).astype(np.float32))
    axis = np.zeros((n_family, 3), dtype=np.float32)
    axis[np.arange(n_family), rng.integers(0, 3, n_family)] = rng.choice([-1.0, 1.0], n_family)
    O.append((lo + rng.random((n_family, 3)) * ext).astype(np.float32)), D.append(axis)
    return np.ascontiguousarray(np.concatenate(O), dtype=np.float32), np.ascontiguousarray(np.concatenate(D), dtype=np.float32)


def gpu_intersect(b, O, D, t_max=None, stream=None):
    o = torch.from_numpy(O).cuda()
    d = torch.from_numpy(D).cuda()
    tm = None if t_max is None else torch.from_numpy(np.ascontiguousarray(t_max, dtype=np.float32)).cuda()
    if stream is None:
        h = b.intersect(o, d, tm)
    else:
        with torch.cuda.stream(stream):
            h = b.intersect(o, d, tm)
    h.check()  # the abandoned word stays 0
    return h


def compare(raw, ob, O, D, rec=None, idx=None):
    """Every record of `raw` ((N, 12) int32 numpy) against the oracle; returns a list of mismatch descriptions."""
    idx = np.arange(len(O)) if idx is None else idx
    hit, out, mat = oracle_answers(ob, O[idx], D[idx])
    raw = raw[idx]
    f = raw.view(np.float32)
    kind = raw[:, 7]
    bad = []

    def note(i, what):
        if len(bad) < 12:
            bad.append((int(idx[i]), what, O[idx[i]].tolist(), D[idx[i]].tolist(), out[i].tolist(), raw[i].tolist()))

    entries = rec.entries() if rec is not None else None
    for i in range(len(idx)):
        if hit[i] != (kind[i] != rtmi.RTMI_HIT_NONE):
            note(i, "hit")
            continue
        if not hit[i]:
            if not (np.isinf(f[i, 0]) and f[i, 0] > 0 and raw[i, 6] == -1):
                note(i, "no-hit record")
            continue
        if bits(out[i, 0]) != bits(f[i, 0]):
            note(i, "t")
            continue
        if entries is not None:
            e = raw[i, 8]
            if not (0 <= e < len(entries)) or ADDS[entries[e][0]] != kind[i]:
                note(i, "entry/kind")
                continue
        if kind[i] == rtmi.RTMI_HIT_SKY:
            continue
        if (bits(out[i, 3:6]) != bits(f[i, 3:6])).any():
            note(i, "normal")
        if mat[i] != raw[i, 6]:
            note(i, "material")
        if kind[i] == rtmi.RTMI_HIT_SPHERE:
            if np.abs(out[i, 1:3] - f[i, 1:3]).max() > SPHERE_UV_TOL:
                note(i, "sphere uv")
        elif (bits(out[i, 1:3]) != bits(f[i, 1:3])).any():
            note(i, "uv")
    return bad


def check_identities(b, rec, seed, O, D, raw, rng, samples=24):
    """entry / element: a one-primitive world of that hitable (or face) answers the same t for the same ray."""
    kind = raw[:, 7]
    f = raw.view(np.float32)
    cand = np.nonzero((kind != rtmi.RTMI_HIT_NONE) & (kind != rtmi.RTMI_HIT_SKY))[0]
    bad = []
    # a sample over the kinds present, each kind represented
    pick = []
    for k in np.unique(kind[cand]):
        c = cand[kind[cand] == k]
        pick += list(rng.choice(c, min(len(c), samples), replace=False))
    for i in pick:
        ob = one_primitive_world(rec, seed, int(raw[i, 8]), int(raw[i, 9]))
        h, out, _ = ob.probe_hit(O[i], D[i])
        if not h or bits(out[0]) != bits(f[i, 0]):
            bad.append((int(i), raw[i].tolist(), h, out.tolist()))
    return bad

F32_INF = np.float32(np.inf)


def oracle_t(ob, O, D):
    """float32(t) of the oracle's closest hit per ray, +inf where there is none."""
    t = np.full(len(O), F32_INF, dtype=np.float32)
    for i in range(len(O)):
        h, out, _ = ob.probe_hit(O[i], D[i])
        if h:
            t[i] = np.float32(out[0])
    return t


def filtered(t, tm):
    """The definition: a hit, and float32(t) <= t_max (NaN t_max: clear; None: no limit)."""
    if tm is None:
        return np.isfinite(t)
    with np.errstate(invalid="ignore"):
        return np.isfinite(t) & (t <= tm)


def gpu_occluded(b, O, D, tm=None, out=None):
    o, d = torch.from_numpy(np.ascontiguousarray(O)).cuda(), torch.from_numpy(np.ascontiguousarray(D)).cuda()
    t = None if tm is None else torch.from_numpy(np.ascontiguousarray(tm, dtype=np.float32)).cuda()
    r = b.occluded(o, d, t, out=out).check()  # d_counts[0] (abandoned searches) stays 0
    return r.mask.cpu().numpy(), r.fallback_rays()


def gpu_filtered(b, O, D, tm=None):
    o, d = torch.from_numpy(np.ascontiguousarray(O)).cuda(), torch.from_numpy(np.ascontiguousarray(D)).cuda()
    t = None if tm is None else torch.from_numpy(np.ascontiguousarray(tm, dtype=np.float32)).cuda()
    return (b.intersect(o, d, t).check().kind != rtmi.RTMI_HIT_NONE).cpu().numpy()


def agree(b, O, D, tm, want, what):
    """The occlusion answer equals `want` (the oracle's) and rtmi_intersect's filtered answer; returns fallback rays."""
    got, fb = gpu_occluded(b, O, D, tm)
    ref = gpu_filtered(b, O, D, tm)
    bad = np.nonzero(got != want)[0]
    assert len(bad) == 0, (what, len(bad), [(int(i), O[i].tolist(), D[i].tolist(), None if tm is None else float(tm[i]))
                                             for i in bad[:8]])
    assert np.array_equal(ref, want), (what, "rtmi_intersect disagrees with the oracle", np.nonzero(ref != want)[0][:8])
    return fb


def glm_normalize(v):
    """glm::normalize in binary32: v * (1 / sqrt((x*x + y*y) + z*z)) (vecmath.hpp:40-53)."""
    v = np.asarray(v, dtype=np.float32)
    x, y, z = v[..., 0], v[..., 1], v[..., 2]
    s = np.sqrt((x * x + y * y) + z * z).astype(np.float32)
    return (v * (np.float32(1) / s)[..., None]).astype(np.float32)
