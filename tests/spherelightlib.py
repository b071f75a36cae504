"""What the tests of sphere table lights share (rtmi_scene_light_kinds): the table with its sphere records and the step of
both rtmi_direct_sample and rtmi_direct_sample_mis on such a table restated in numpy from include/rtmi.h
("rtmi_scene_light_kinds"), and the scenes.  Everything the flat lights' tests already have comes from directlib and
mislib.  No test lives here."""
import math

import numpy as np

import directlib as dl
import mislib as ml
import rtmi
from directlib import F0, F1, f32
from querylib import v3

INF = f32(np.inf)
F2 = f32(2)
FLAT, SPHERES = 1, 2  # include/rtmi.h: RTMI_LIGHTS_*
KIND_SPHERE = 2       # rtmi_light.kind


# ------------------------------------------------------------------ the table
def spheres_of(rec):
    """(entry, centre float32 (3,), radius as the call gave it, material) per Sphere of a Recorder's scene, in the
    flattened list's order."""
    return [(entry, np.asarray(a[0], dtype=f32).reshape(3), float(a[1]), int(a[2]))
            for entry, (name, a, _) in enumerate(rec.entries()) if name == "sphere"]


def light_table(hot, pairs, mats, spheres, kinds):
    """The table of include/rtmi.h with rtmi_scene_light_kinds(kinds): directlib.light_table's flat records, then (kinds
    == 3) one record per sphere table light, W, cdf and scale over the whole table."""
    flat = dl.light_table(hot, pairs, mats)
    if kinds == FLAT:
        return flat
    rows, w = [], []
    for r in flat:  # the unrounded areas and weights of the flat records, by directlib's expressions
        a, b = r["e1"].astype(np.float64), r["e2"].astype(np.float64)
        c = np.array([a[1] * b[2] - b[1] * a[2], a[2] * b[0] - b[2] * a[0], a[0] * b[1] - b[0] * a[1]])
        ln = math.sqrt((c[0] * c[0] + c[1] * c[1]) + c[2] * c[2])
        ar = 0.5 * ln if r["kind"] == 1 else ln
        rgb = r["emission"]
        rows.append((r, ar))
        w.append(ar * ((abs(float(rgb[0])) + abs(float(rgb[1]))) + abs(float(rgb[2]))))
    n_flat = len(rows)
    zero = np.zeros(3, f32)
    for entry, c, r, m in spheres:
        if not 0 <= m < len(mats) or mats[m][0] != dl.LIGHT or mats[m][1] is None:
            continue
        rgb = mats[m][1]
        if not np.isfinite(rgb).all() or not rgb.any() or not np.isfinite(c).all():
            continue
        if not (math.isfinite(r) and r > 0):
            continue
        with np.errstate(all="ignore"):
            R = f32(r)
            R2 = f32(R * R)
        if not (np.isfinite(R) and R > 0 and np.isfinite(R2) and R2 > 0):
            continue
        ar = 4 * math.pi * r * r
        rec = np.zeros((), dtype=rtmi.LIGHT_DTYPE)
        rec["p0"], rec["e1"], rec["e2"], rec["n"] = c, np.array([R, R2, 0], f32), zero, zero
        rec["emission"], rec["area"], rec["kind"], rec["entry"], rec["element"], rec["material"] = rgb, f32(ar), KIND_SPHERE, entry, 0, m
        rows.append((rec, ar))
        w.append(ar * ((abs(float(rgb[0])) + abs(float(rgb[1]))) + abs(float(rgb[2]))))
    tab = np.zeros((len(rows),), dtype=rtmi.LIGHT_DTYPE)
    W, run = 0.0, 0.0
    for x in w:
        W += x
    for j, (r, ar) in enumerate(rows):
        tab[j] = r
        run += w[j]
        with np.errstate(all="ignore"):
            tab[j]["cdf"] = f32(run / W)
            tab[j]["scale"] = f32(ar * W / (w[j] * math.pi)) if j < n_flat else f32(2 * W / w[j])
    if len(rows):
        tab[-1]["cdf"] = F1
    return tab


def table_of(rec, kinds=FLAT | SPHERES):
    """The restated table of a Recorder's scene (host only)."""
    hot = rec.b.list_records()[1][:, 0, :]
    return light_table(hot, dl.pairs_of(rec), dl.materials_of(rec), spheres_of(rec), kinds)


# ------------------------------------------------------------------ the geometry, one rounding per operation
def _r(x):
    return np.asarray(x, dtype=f32)


def cone(c, R2, x):
    """The shared geometry of a sphere light (centres c (k, 3), R2 (k,)) from the points x (k, 3): wc, d2c, outside, om."""
    with np.errstate(all="ignore"):
        wc = _r(_r(c) - _r(x))
        d2c = dl._dot(wc, wc)
        outside = d2c > R2
        s2 = _r(R2 / d2c)
        cm = _r(np.sqrt(_r(_r(d2c - R2) / d2c)))
        om = _r(s2 / _r(F1 + cm))
    return wc, d2c, outside, om


def draw11(st, idx):
    """CudaRandomFloat(-1, 1): draw01 * 2 + (-1)."""
    return _r(_r(dl.draw01(st, idx) * F2) + f32(-1))


def disc_draws(st, idx):
    """The rejection loop for the rows idx of st, advanced in place: (cp, sp, trips) with (a, b) the first pair of
    CudaRandomFloat(-1, 1) draws whose s = a a + b b has s > 0 && s <= 1, cp = a / sqrt(s), sp = b / sqrt(s)."""
    idx = np.asarray(idx, dtype=np.int64)
    a, b, s = np.zeros(len(idx), f32), np.zeros(len(idx), f32), np.zeros(len(idx), f32)
    trips = np.zeros(len(idx), np.int64)
    todo = np.arange(len(idx))
    while len(todo):
        aa = draw11(st, idx[todo])
        bb = draw11(st, idx[todo])
        ss = _r(_r(aa * aa) + _r(bb * bb))
        a[todo], b[todo], s[todo] = aa, bb, ss
        trips[todo] += 1
        todo = todo[~((ss > 0) & (ss <= 1))]
    ls = _r(np.sqrt(s))
    return _r(a / ls), _r(b / ls), trips


def frame(w):
    """Duff et al.'s branch-free basis (u, v) around the axes w (k, 3)."""
    wx, wy, wz = w[:, 0], w[:, 1], w[:, 2]
    with np.errstate(all="ignore"):
        sg = np.where(wz >= 0, F1, f32(-1)).astype(f32)
        ka = _r(f32(-1) / _r(sg + wz))
        kb = _r(_r(wx * wy) * ka)
        u = np.stack([_r(F1 + _r(_r(sg * _r(wx * wx)) * ka)), _r(sg * kb), _r(-sg * wx)], axis=1)
        v = np.stack([kb, _r(sg + _r(_r(wy * wy) * ka)), -wy], axis=1)
    return _r(u), _r(v)


def sample_sphere(c, R2, x, N, r1, cp, sp):
    """SAMPLE's arithmetic for a sphere light from the draws on: a dict of every intermediate the tests look at (wi, t,
    cs, om, outside, valid, w, u, v, ct, q)."""
    with np.errstate(all="ignore"):
        wc, d2c, outside, om = cone(c, R2, x)
        dc = _r(np.sqrt(d2c))
        h = _r(r1 * om)
        ct = _r(F1 - h)
        st2 = _r(h * _r(F2 - h))
        st = _r(np.sqrt(st2))
        w = _r(wc / dc[:, None])
        u, v = frame(w)
        sc, ss = _r(st * cp), _r(st * sp)
        wi = _r(_r(_r(ct[:, None] * w) + _r(sc[:, None] * u)) + _r(ss[:, None] * v))
        tc = _r(dc * ct)
        q = _r(R2 - _r(d2c * st2))
        q = np.where(q > 0, q, F0).astype(f32)
        t = _r(tc - _r(np.sqrt(q)))
        cs = dl._dot(_r(N), wi)
        valid = outside & (cs > 0) & (t > 0) & (t < INF)
    return dict(wi=wi, t=t, cs=cs, om=om, outside=outside, valid=valid, w=w, u=u, v=v, ct=ct, q=q, dc=dc, d2c=d2c)


def sphere_a(c, om, scale):
    """a = (c * om) * scale: the scattered ray's density over the light sample's is a : 1 (c: cs in SAMPLE, carry.w in
    WEIGH)."""
    with np.errstate(all="ignore"):
        return _r(_r(_r(c) * _r(om)) * _r(scale))


def sphere_weight(a):
    """WEIGH's w: (a > 0 && a + 1 < +inf) ? a / (a + 1) : +0.0f, and whether it came from the division."""
    a = _r(a)
    with np.errstate(all="ignore"):
        s = _r(a + F1)
        div = (a > 0) & (s < INF)
        w = np.where(div, _r(a / s), F0).astype(f32)
    return w, div


# ------------------------------------------------------------------ the light of a hit
def sphere_light_of_hit(tab, H):
    """Per hit record the sphere table light j of a SPHERE hit, -1 for none: the first j with tab[j].entry == hit.entry,
    if that record is of kind 2."""
    H = np.asarray(H, dtype=np.int32).reshape(-1, 12)
    kind, entry = H[:, 7], H[:, 8]
    first = np.full(len(H), -1, dtype=np.int64)
    able = (kind == rtmi.RTMI_HIT_SPHERE) & (entry >= 0)
    for j in range(len(tab) - 1, -1, -1):
        first[able & (entry == tab["entry"][j])] = j
    ok = first >= 0
    ok[ok] = tab["kind"][first[ok]] == KIND_SPHERE
    return np.where(ok, first, -1)


# ------------------------------------------------------------------ the step
def step(tab, mat_kinds, ps, step_no, sample, cand=None, mis=True):
    """rtmi_direct_sample_mis (mis=False: rtmi_direct_sample, the carry untouched) on a table that may hold sphere lights,
    in numpy, on a mislib.PathState in place; the other arguments are directlib.step's."""
    n = len(ps.O)
    c = np.arange(n) if cand is None else np.asarray(cand, dtype=np.int64)
    c = c[c < n]
    mat_kinds = np.asarray(mat_kinds, dtype=np.int64)
    light_mat = np.zeros(len(mat_kinds), bool)
    light_mat[tab["material"][tab["kind"] != KIND_SPHERE]] = True  # (no bit for a sphere light: it is known by its record)
    ps.SD[c], ps.DR[c], ps.ST[c] = 0, 0, 0
    was = (ps.flags[c] & 1) != 0
    ps.flags[c] &= ~np.uint32(1)
    stepped = ps.steps[c] == step_no + 1
    s, was = c[stepped], was[stepped]
    mat, kind = ps.H[s, 6].astype(np.int64), ps.H[s, 7]
    mat_ok = (mat >= 0) & (mat < len(mat_kinds))
    msafe = np.where(mat_ok, mat, 0)
    # the sphere light of a flagged SPHERE hit, seen from the vertex before
    sj = sphere_light_of_hit(tab, ps.H[s])
    on = was & (sj >= 0)
    i, j = s[on], sj[on]
    _, _, outside, om = cone(tab["p0"][j], tab["e1"][j, 1], ps.O[i])
    i, j, om = i[outside], j[outside], om[outside]
    if mis:
        # WEIGH, flat lights: mislib.step's text
        lj = ml.light_of_hit(tab, ps.H[s])
        wg = was & (lj >= 0)
        fi, fj = s[wg], lj[wg]
        if len(fi):
            cw = ps.C[fi]
            with np.errstate(all="ignore"):
                cl = np.abs(dl._dot(tab["n"][fj], cw[:, :3]))
                t = ps.H[fi, 0].view(f32)
                w, div = ml.scatter_weight(ml.mis_a(cw[:, 3], cl, tab["scale"][fj]), (t * t).astype(f32))
                ps.E[fi] = np.where(div[:, None], (ps.E[fi] * w[:, None]).astype(f32), F0)
        ps.counts[1] += np.uint64(len(fi))
        # WEIGH, sphere lights
        if len(i):
            w, div = sphere_weight(sphere_a(ps.C[i, 3], om, tab["scale"][j]))
            with np.errstate(all="ignore"):
                ps.E[i] = np.where(div[:, None], (ps.E[i] * w[:, None]).astype(f32), F0)
        ps.counts[1] += np.uint64(len(i))
    else:
        on_light = mat_ok & np.isin(kind, dl.SURFACE_KINDS) & (light_mat[msafe] if len(mat_kinds) else False)
        drop = was & on_light
        ps.E[s[drop]] = 0
        ps.E[i] = 0
        ps.counts[1] += np.uint64(drop.sum() + len(i))
    # SAMPLE
    scattered = (ps.D[s] != 0).any(1)
    samp = scattered & mat_ok & ((mat_kinds[msafe] == dl.LAMBERTIAN) if len(mat_kinds) else False)
    if not sample or len(tab) == 0:
        samp[:] = False
    p = s[samp]
    ps.flags[p] |= np.uint32(1)
    ps.counts[0] += np.uint64(len(p))
    if len(p) == 0:
        return ps
    r0, r1 = dl.draw01(ps.LS, p), dl.draw01(ps.LS, p)
    j = np.searchsorted(tab["cdf"], r0, side="left")  # the smallest j with r0 <= cdf[j]
    sph = tab["kind"][j] == KIND_SPHERE
    x, N, A = ps.O[p], ps.H[p, 3:6].view(f32), ps.A[p]
    valid = np.zeros(len(p), bool)
    wi, tm, dr = np.zeros((len(p), 3), f32), np.zeros(len(p), f32), np.zeros((len(p), 3), f32)
    with np.errstate(all="ignore"):
        if (~sph).any():  # a flat light: directlib's and mislib's text
            k = np.flatnonzero(~sph)
            jk, r1k = j[k], r1[k]
            r2k = dl.draw01(ps.LS, p[k])
            flip = (tab["kind"][jk] == 1) & ((r1k + r2k).astype(f32) > F1)
            r1k, r2k = np.where(flip, (F1 - r1k).astype(f32), r1k), np.where(flip, (F1 - r2k).astype(f32), r2k)
            p0, e1, e2, ln = tab["p0"][jk], tab["e1"][jk], tab["e2"][jk], tab["n"][jk]
            q = ((p0 + (r1k[:, None] * e1).astype(f32)).astype(f32) + (r2k[:, None] * e2).astype(f32)).astype(f32)
            w = (q - x[k]).astype(f32)
            d2 = dl._dot(w, w)
            dist = np.sqrt(d2).astype(f32)
            wk = (w / dist[:, None]).astype(f32)
            cs = dl._dot(N[k], wk)
            cl = np.abs(dl._dot(ln, wk))
            valid[k] = (d2 > 0) & (cs > 0) & (cl > 0) & (dist < INF)
            if mis:
                g = ml.sample_g(ml.mis_a(cs, cl, tab["scale"][jk]), d2)
            else:
                g = (((cs * cl).astype(f32) / d2).astype(f32) * tab["scale"][jk]).astype(f32)
            wi[k], tm[k] = wk, (dist * f32(0.999)).astype(f32)
            dr[k] = ((A[k] * tab["emission"][jk]).astype(f32) * g[:, None]).astype(f32)
        if sph.any():  # a sphere light
            k = np.flatnonzero(sph)
            jk = j[k]
            cp, sp, _ = disc_draws(ps.LS, p[k])
            o = sample_sphere(tab["p0"][jk], tab["e1"][jk, 1], x[k], N[k], r1[k], cp, sp)
            a = sphere_a(o["cs"], o["om"], tab["scale"][jk])
            g = _r(a / _r(a + F1)) if mis else a
            valid[k], wi[k], tm[k] = o["valid"], o["wi"], _r(o["t"] * f32(0.999))
            dr[k] = ((A[k] * tab["emission"][jk]).astype(f32) * g[:, None]).astype(f32)
        if mis:
            ps.C[p] = np.concatenate([ps.D[p], dl._dot(N, ps.D[p])[:, None]], axis=1)
    v = p[valid]
    ps.SO[v], ps.SD[v], ps.ST[v], ps.DR[v] = x[valid], wi[valid], tm[valid], dr[valid]
    return ps


# ------------------------------------------------------------------ the scenes
BULBS = (((5, 7, 4.5), 1.5, (6, 6, 5)), ((2, 3, 7), 0.6, (1, 3, 6)))
SMALL_BULBS = (((5, 7, 4.5), 0.5, (48, 48, 40)), ((2, 3, 7), 0.25, (5, 15, 30)))


def room(b, bulbs):
    """directlib.lamp_room's room, camera, box, metal and dielectric spheres, with no parallelogram lamp and no emissive
    triangle: lit by emissive spheres (centre, radius, emission) alone."""
    b.camera_pinhole(v3(5, 5, 9.5), v3(5, 4, 0), v3(0, 1, 0), math.pi / 3, 1.0)
    white = b.lambertian(v3(0.73, 0.73, 0.73))
    red = b.lambertian(v3(0.65, 0.05, 0.05))
    green = b.lambertian(v3(0.12, 0.45, 0.15))
    blue = b.lambertian(v3(0.2, 0.3, 0.8))
    b.parallelogram([v3(0, 0, 0), v3(10, 0, 0), v3(0, 0, 10)], white)      # floor
    b.parallelogram([v3(0, 10, 0), v3(10, 10, 0), v3(0, 10, 10)], white)   # ceiling
    b.parallelogram([v3(0, 0, 0), v3(0, 10, 0), v3(0, 0, 10)], red)        # x = 0
    b.parallelogram([v3(10, 0, 0), v3(10, 10, 0), v3(10, 0, 10)], green)   # x = 10
    b.parallelogram([v3(0, 0, 0), v3(10, 0, 0), v3(0, 10, 0)], white)      # z = 0
    b.parallelogram([v3(0, 0, 10), v3(10, 0, 10), v3(0, 10, 10)], white)   # z = 10, behind the camera
    for c, r, le in bulbs:
        b.sphere(v3(*c), r, b.diffuse_light(b.constant_texture(v3(*le))))
    b.parallelepiped([v3(2, 0, 2), v3(4, 0, 2), v3(2, 3, 2), v3(2, 0, 4)], blue)
    b.sphere(v3(7, 1.5, 3), 1.5, b.metal(v3(0.8, 0.8, 0.8), 0.1))
    b.sphere(v3(6, 1, 6.5), 1.0, b.dielectric(v3(1, 1, 1), 1.5))
    return b


def bulb_room(b):
    return room(b, BULBS)


def small_bulb_room(b):
    return room(b, SMALL_BULBS)


def enclosing_light(b):
    """A Lambertian sphere and a box inside one emissive sphere of radius 50, the camera inside: no vertex can sample the
    light."""
    b.camera_pinhole(v3(0, 1, 6), v3(0, 0, 0), v3(0, 1, 0), 0.9, 1.0)
    b.sphere(v3(0, 0, 0), 50.0, b.diffuse_light(b.constant_texture(v3(1, 0.9, 0.8))))
    b.sphere(v3(0, 0, 0), 1.0, b.lambertian(v3(0.7, 0.6, 0.5)))
    b.parallelepiped([v3(2, -1, -1), v3(3, -1, -1), v3(2, 0.5, -1), v3(2, -1, 0)], b.lambertian(v3(0.3, 0.6, 0.8)))
    return b


def shared_material_world(b):
    """A flat light and a sphere light on ONE material, an emissive sphere that is no table light (radius < 0, inside a
    glass shell's place) on it too, a sphere light in a nested list, over a Lambertian floor."""
    b.camera_pinhole(v3(0, 2, 8), v3(0, 1, 0), v3(0, 1, 0), 0.9, 1.0)
    grey = b.lambertian(v3(0.6, 0.6, 0.6))
    lamp = b.diffuse_light(b.constant_texture(v3(4, 3, 2)))
    b.parallelogram([v3(-6, 0, -6), v3(6, 0, -6), v3(-6, 0, 6)], grey)
    b.parallelogram([v3(-1, 4, -1), v3(1, 4, -1), v3(-1, 4, 1)], lamp)
    b.sphere(v3(2.5, 2, 0), 0.75, lamp)
    b.sphere(v3(-2.5, 1, 1), -0.5, lamp)
    b.list_begin()
    b.sphere(v3(0, 1, -2), 1.0, grey)
    b.list_begin()
    b.sphere(v3(-3, 3, -2), 0.4, b.diffuse_light(b.constant_texture(v3(0.5, 2, 9))))
    b.list_end()
    b.list_end()
    return b


def rejected_spheres_world(b):
    """Emissive spheres that are no table lights -- radius 0, < 0, so large that R * R overflows, so small
    that it underflows, image-textured, black, a non-finite emission -- beside one that is."""
    b.camera_pinhole(v3(0, 1, 6), v3(0, 0, 0), v3(0, 1, 0), 0.9, 1.0)
    lamp = b.diffuse_light(b.constant_texture(v3(2, 1, 0)))
    b.parallelogram([v3(-4, -1, -4), v3(4, -1, -4), v3(-4, -1, 4)], b.lambertian(v3(0.5, 0.5, 0.5)))
    for k, r in enumerate((0.0, -1.0, 1e30, 1e-30, 1e-300)):  # (rtmi_add_sphere refuses a non-finite radius itself)
        b.sphere(v3(-3 + k, 3, 0), r, lamp)
    b.sphere(v3(0, 2, 0), 0.5, b.diffuse_light(b.image_texture(np.full((2, 2, 4), 255, np.uint8))))
    b.sphere(v3(1, 2, 0), 0.5, b.diffuse_light(b.constant_texture(v3(0, 0, 0))))
    b.sphere(v3(2, 2, 0), 0.5, b.diffuse_light(b.constant_texture(v3(1, float("inf"), 1))))
    b.sphere(v3(-1, 2, 0), 0.5, lamp)  # the one table light
    return b


def many_mixed_lights_world(n_lights=1100):
    """directlib.many_lights_world with every third light a small emissive sphere: a table beyond the LDS staging whose
    sphere records lie behind its flat ones."""
    def fill(b):
        b.camera_pinhole(v3(0, 2, 9), v3(0, 1, 0), v3(0, 1, 0), 0.9, 1.0)
        grey = b.lambertian(v3(0.6, 0.6, 0.6))
        b.parallelogram([v3(-8, 0, -8), v3(8, 0, -8), v3(-8, 0, 8)], grey)
        b.parallelepiped([v3(-1, 0, -1), v3(1, 0, -1), v3(-1, 2, -1), v3(-1, 0, 1)], b.lambertian(v3(0.8, 0.4, 0.2)))
        rng = np.random.default_rng(n_lights)
        mats = [b.diffuse_light(b.constant_texture(v3(*rng.uniform(0.5, 8, 3)))) for _ in range(7)]
        done = 0
        while done < n_lights:
            b.list_begin()
            for k in range(done, min(done + 550, n_lights)):
                x, z = -6 + 12 * (k % 40) / 40, -6 + 12 * (k // 40) / 40
                s = 0.05 + 0.2 * rng.random()
                if k % 3 == 2:
                    b.sphere(v3(x, 5, z), 0.5 * s, mats[k % 7])
                else:
                    b.triangle([v3(x, 5, z), v3(x + s, 5, z), v3(x, 5 + 0.1 * rng.random(), z + s)], mats[k % 7])
            b.list_end()
            done = min(done + 550, n_lights)
    return fill


def with_kinds(fill, spheres=True):
    """The scene program `fill` with light_kinds(spheres) called first."""
    def prog(b):
        b.light_kinds(spheres=spheres)
        return fill(b)
    return prog


def light_kinds_raw(b, kinds):
    """rtmi_scene_light_kinds on a builder (or None for a null scene), through the C ABI: the return code."""
    return rtmi.lib().rtmi_scene_light_kinds(b.h if b is not None else None, kinds)
