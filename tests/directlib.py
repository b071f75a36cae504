"""What the next-event-estimation tests share (rtmi_scene_lights, rtmi_direct_sample, rtmi_path_fold_direct): the light
table, the step and the fold restated in numpy (held to hand-worked cases by tests/test_direct_host.py), the lamp_room
scene, and the device calls through the C ABI with canaries behind every array.  No test lives here."""
import ctypes as C
import math

import numpy as np

import bouncelib
import oraclelib
import rtmi
from querylib import ADDS, Recorder, v3
from rtmi import scenes

f32 = np.float32
F0, F1 = f32(0), f32(1)
CANARY_I = 0x5a5a5a5a
CANARY_F = f32(-7.25)
PAD = 64
LAMBERTIAN, LIGHT = 0, 3  # scene_dev.h: MatKind
SURFACE_KINDS = (rtmi.RTMI_HIT_TRIANGLE, rtmi.RTMI_HIT_PARALLELOGRAM, rtmi.RTMI_HIT_PARALLELEPIPED)


# ------------------------------------------------------------------ the generator (XORWOW, curand_uniform)
def draw01(st, idx):
    """CudaRandomFloat(0, 1) for the rows idx of st ((n, 6) uint32: d, v0..v4), advanced in place: x * 2^-32 + 2^-33 in
    binary32, in (0, 1]."""
    s = st[idx].astype(np.uint64)
    m = np.uint64(0xffffffff)
    d, v0, v1, v2, v3_, v4 = (s[:, k] for k in range(6))
    t = v0 ^ (v0 >> np.uint64(2))
    n4 = ((v4 ^ ((v4 << np.uint64(4)) & m)) ^ (t ^ ((t << np.uint64(1)) & m))) & m
    d = (d + np.uint64(362437)) & m
    st[idx] = np.stack([d, v1, v2, v3_, v4, n4], axis=1).astype(np.uint32)
    x = ((n4 + d) & m).astype(np.uint32)
    return (x.astype(f32) * f32(2.0 ** -32) + f32(2.0 ** -33)).astype(f32)


# ------------------------------------------------------------------ the light table
def materials_of(rec):
    """(kind, rgb or None for an image texture) per material handle of a Recorder's scene, in handle order."""
    texs, mats = [], []
    for name, a, _ in rec.calls:
        if name == "constant_texture":
            texs.append(np.asarray(a[0], dtype=f32).reshape(3))
        elif name == "image_texture":
            texs.append(None)
        elif name == "lambertian":
            mats.append((LAMBERTIAN, np.asarray(a[0], dtype=f32).reshape(3)))
        elif name == "lambertian_tex":
            mats.append((LAMBERTIAN, texs[a[0]]))
        elif name == "metal":
            mats.append((1, np.asarray(a[0], dtype=f32).reshape(3)))
        elif name == "dielectric":
            mats.append((2, np.asarray(a[0], dtype=f32).reshape(3)))
        elif name == "diffuse_light":
            mats.append((LIGHT, texs[a[0]]))
    return mats


def pairs_of(rec):
    """(entry, kind, element) per pair of world-list triangle records, in the flattened list's order."""
    out = []
    for entry, (name, _, _) in enumerate(rec.entries()):
        kind = ADDS[name]
        if kind == rtmi.RTMI_HIT_PARALLELEPIPED:
            out += [(entry, kind, face) for face in range(6)]
        elif kind in (rtmi.RTMI_HIT_TRIANGLE, rtmi.RTMI_HIT_PARALLELOGRAM):
            out.append((entry, kind, 0))
    return out


def light_table(hot, pairs, mats):
    """The table of include/rtmi.h ("direct") from the pairs' first HotTri records (hot: (P, 16) uint32 -- p0, e1, e2, n,
    material), their (entry, kind, element) and the materials: a record array of rtmi.LIGHT_DTYPE."""
    hot = np.asarray(hot, dtype=np.uint32).reshape(-1, 16)
    rows, area, w = [], [], []
    for p, (entry, kind, element) in enumerate(pairs):
        g = hot[p, :12].view(f32)
        m = int(hot[p, 12].view(np.int32))
        if not 0 <= m < len(mats) or mats[m][0] != LIGHT or mats[m][1] is None:
            continue
        rgb = mats[m][1]
        if not np.isfinite(rgb).all() or not rgb.any():
            continue
        a, b = g[3:6].astype(np.float64), g[6:9].astype(np.float64)
        with np.errstate(all="ignore"):
            c = np.array([a[1] * b[2] - b[1] * a[2], a[2] * b[0] - b[2] * a[0], a[0] * b[1] - b[0] * a[1]])
            if not np.isfinite(c).all() or not c.any():
                continue
            ln = math.sqrt((c[0] * c[0] + c[1] * c[1]) + c[2] * c[2])
        tri = kind == rtmi.RTMI_HIT_TRIANGLE
        ar = 0.5 * ln if tri else ln
        rows.append((g[0:3], g[3:6], g[6:9], g[9:12], rgb, f32(ar), F0, F0, 1 if tri else 0, entry, element, m))
        area.append(ar)
        w.append(ar * ((abs(float(rgb[0])) + abs(float(rgb[1]))) + abs(float(rgb[2]))))
    tab = np.zeros((len(rows),), dtype=rtmi.LIGHT_DTYPE)
    W, run = 0.0, 0.0
    for x in w:
        W += x
    for j, r in enumerate(rows):
        tab[j] = r
        run += w[j]
        with np.errstate(all="ignore"):
            tab[j]["cdf"] = f32(run / W)
            tab[j]["scale"] = f32(area[j] * W / (w[j] * math.pi))
    if len(rows):
        tab[-1]["cdf"] = F1
    return tab


def table_of(rec):
    """The restated table of a Recorder's scene (host only: the HotTri records come from the flatten pass)."""
    hot = rec.b.list_records()[1][:, 0, :]
    return light_table(hot, pairs_of(rec), materials_of(rec))


def same_table(a, b):
    """Field by field, bit for bit."""
    if a.shape != b.shape:
        return False
    return all(np.array_equal(np.ascontiguousarray(a[k]).view(np.uint32), np.ascontiguousarray(b[k]).view(np.uint32))
               for k in rtmi.LIGHT_DTYPE.names)


# ------------------------------------------------------------------ the step
def _dot(a, b):
    return ((a[:, 0] * b[:, 0] + a[:, 1] * b[:, 1]).astype(f32) + a[:, 2] * b[:, 2]).astype(f32)


class PathState:
    """The arrays one rtmi_direct_sample reads and writes, on the host: O, D (n, 3) float32; H (n, 12) int32 hit records;
    steps (n,) uint32; E, A (n, 3) float32 (one layer); LS (n, 6) uint32 light states; flags (n,) uint32; the outputs SO, SD
    (n, 3), ST (n,), DR (n, 3) float32; counts (2,) uint64."""

    FIELDS = ("O", "D", "H", "steps", "E", "A", "LS", "flags", "SO", "SD", "ST", "DR", "counts")

    def __init__(self, O, D, H, steps, E, A, LS, flags=None, seed=5):
        n = len(O)
        rng = np.random.default_rng(seed + n)
        self.O, self.D = np.array(O, dtype=f32).reshape(n, 3), np.array(D, dtype=f32).reshape(n, 3)
        self.H = np.array(H, dtype=np.int32).reshape(n, 12)
        self.steps = np.array(steps, dtype=np.uint32).reshape(n)
        self.E, self.A = np.array(E, dtype=f32).reshape(n, 3), np.array(A, dtype=f32).reshape(n, 3)
        self.LS = np.array(LS, dtype=np.uint32).reshape(n, 6)
        self.flags = np.zeros(n, np.uint32) if flags is None else np.array(flags, dtype=np.uint32).reshape(n)
        # the outputs start as recognisable junk: what a call leaves alone shows
        self.SO, self.SD = rng.uniform(1, 2, (n, 3)).astype(f32), rng.uniform(1, 2, (n, 3)).astype(f32)
        self.ST, self.DR = rng.uniform(1, 2, n).astype(f32), rng.uniform(1, 2, (n, 3)).astype(f32)
        self.counts = np.array([3, 5], dtype=np.uint64)

    def copy(self):
        c = object.__new__(PathState)
        for k in self.FIELDS:
            setattr(c, k, getattr(self, k).copy())
        return c


def step(tab, mat_kinds, ps, step_no, sample, cand=None):
    """rtmi_direct_sample in numpy, on a PathState in place.  tab: the light table; mat_kinds: the kind of every material;
    cand: the candidates' path indices (None: all), entries >= n dropped, distinct."""
    n = len(ps.O)
    c = np.arange(n) if cand is None else np.asarray(cand, dtype=np.int64)
    c = c[c < n]
    mat_kinds = np.asarray(mat_kinds, dtype=np.int64)
    light_mat = np.zeros(len(mat_kinds), bool)
    light_mat[tab["material"]] = True
    ps.SD[c], ps.DR[c], ps.ST[c] = 0, 0, 0
    was = (ps.flags[c] & 1) != 0
    ps.flags[c] &= ~np.uint32(1)
    stepped = ps.steps[c] == step_no + 1
    s, was = c[stepped], was[stepped]
    mat, kind = ps.H[s, 6].astype(np.int64), ps.H[s, 7]
    mat_ok = (mat >= 0) & (mat < len(mat_kinds))
    msafe = np.where(mat_ok, mat, 0)
    on_light = mat_ok & np.isin(kind, SURFACE_KINDS) & (light_mat[msafe] if len(mat_kinds) else False)
    drop = was & on_light
    ps.E[s[drop]] = 0
    ps.counts[1] += np.uint64(drop.sum())
    scattered = (ps.D[s] != 0).any(1)
    samp = scattered & mat_ok & ((mat_kinds[msafe] == LAMBERTIAN) if len(mat_kinds) else False)
    if not sample or len(tab) == 0:
        samp[:] = False
    p = s[samp]
    ps.flags[p] |= np.uint32(1)
    ps.counts[0] += np.uint64(len(p))
    if len(p) == 0:
        return ps
    r0, r1, r2 = draw01(ps.LS, p), draw01(ps.LS, p), draw01(ps.LS, p)
    j = np.searchsorted(tab["cdf"], r0, side="left")  # the smallest j with r0 <= cdf[j]
    with np.errstate(all="ignore"):
        flip = (tab["kind"][j] == 1) & ((r1 + r2).astype(f32) > F1)
        r1, r2 = np.where(flip, (F1 - r1).astype(f32), r1), np.where(flip, (F1 - r2).astype(f32), r2)
        p0, e1, e2, ln = tab["p0"][j], tab["e1"][j], tab["e2"][j], tab["n"][j]
        q = ((p0 + (r1[:, None] * e1).astype(f32)).astype(f32) + (r2[:, None] * e2).astype(f32)).astype(f32)
        x = ps.O[p]
        w = (q - x).astype(f32)
        d2 = _dot(w, w)
        dist = np.sqrt(d2).astype(f32)
        wi = (w / dist[:, None]).astype(f32)
        N = ps.H[p, 3:6].view(f32)
        cs = _dot(N, wi)
        cl = np.abs(_dot(ln, wi))
        valid = (d2 > 0) & (cs > 0) & (cl > 0) & (dist < f32(np.inf))
        g = (((cs * cl).astype(f32) / d2).astype(f32) * tab["scale"][j]).astype(f32)
        dr = ((ps.A[p] * tab["emission"][j]).astype(f32) * g[:, None]).astype(f32)
        tm = (dist * f32(0.999)).astype(f32)
    v = p[valid]
    ps.SO[v], ps.SD[v], ps.ST[v], ps.DR[v] = x[valid], wi[valid], tm[valid], dr[valid]
    return ps


# ------------------------------------------------------------------ the fold
def fold_direct(dirs, steps, E, A, Dk, occ, layers=None):
    """rtmi_path_fold_direct in binary32: rtmi_path_fold (bouncelib.fold) with T[k] = occ[k] ? E[k] : E[k] + D[k] for
    E[k].  E, A, Dk (L, n, 3) float32; occ (L, n) uint8."""
    E, Dk = np.asarray(E, dtype=f32), np.asarray(Dk, dtype=f32)
    with np.errstate(all="ignore"):
        T = np.where(np.asarray(occ).astype(bool)[..., None], E, (E + Dk).astype(f32))
    return bouncelib.fold(dirs, steps, T, A, layers)


# ------------------------------------------------------------------ the lamp_room scene
LAMP_ROOM_SEED = 77


def lamp_room(b):
    """A closed room of six Lambertian parallelograms with the camera inside, a parallelogram lamp under the ceiling, a
    lone emissive triangle of another colour, a Lambertian box, a metal and a dielectric sphere.  No Sky: every photon
    comes from a table light."""
    b.camera_pinhole(v3(5, 5, 9.5), v3(5, 4, 0), v3(0, 1, 0), math.pi / 3, 1.0)
    white = b.lambertian(v3(0.73, 0.73, 0.73))
    red = b.lambertian(v3(0.65, 0.05, 0.05))
    green = b.lambertian(v3(0.12, 0.45, 0.15))
    blue = b.lambertian(v3(0.2, 0.3, 0.8))
    lamp = b.diffuse_light(b.constant_texture(v3(3, 3, 2.5)))
    glow = b.diffuse_light(b.constant_texture(v3(0.5, 1.5, 3)))
    b.parallelogram([v3(0, 0, 0), v3(10, 0, 0), v3(0, 0, 10)], white)      # floor
    b.parallelogram([v3(0, 10, 0), v3(10, 10, 0), v3(0, 10, 10)], white)   # ceiling
    b.parallelogram([v3(0, 0, 0), v3(0, 10, 0), v3(0, 0, 10)], red)        # x = 0
    b.parallelogram([v3(10, 0, 0), v3(10, 10, 0), v3(10, 0, 10)], green)   # x = 10
    b.parallelogram([v3(0, 0, 0), v3(10, 0, 0), v3(0, 10, 0)], white)      # z = 0
    b.parallelogram([v3(0, 0, 10), v3(10, 0, 10), v3(0, 10, 10)], white)   # z = 10, behind the camera
    b.parallelogram([v3(2, 8.5, 2), v3(8, 8.5, 2), v3(2, 8.5, 8)], lamp)
    b.triangle([v3(1.5, 4.5, 1), v3(1.5, 4.5, 8), v3(1.5, 9.5, 4.5)], glow)
    b.parallelepiped([v3(2, 0, 2), v3(4, 0, 2), v3(2, 3, 2), v3(2, 0, 4)], blue)
    b.sphere(v3(7, 1.5, 3), 1.5, b.metal(v3(0.8, 0.8, 0.8), 0.1))
    b.sphere(v3(6, 1, 6.5), 1.0, b.dielectric(v3(1, 1, 1), 1.5))
    return b


def odd_lights_world(rec):
    """Lights that are not table lights -- on a sphere, on a mesh, image-textured, black, degenerate -- beside one in a
    nested list, which is the only one in the table."""
    b = rec
    b.camera_pinhole(v3(0, 1, 6), v3(0, 0, 0), v3(0, 1, 0), 0.9, 1.0)
    grey = b.lambertian(v3(0.5, 0.5, 0.5))
    lamp = b.diffuse_light(b.constant_texture(v3(2, 0, -4)))
    img = b.diffuse_light(b.image_texture(np.full((2, 2, 4), 255, np.uint8)))
    black = b.diffuse_light(b.constant_texture(v3(0, 0, 0)))
    b.sphere(v3(0, 0, 0), 1.0, lamp)
    b.bvh(scenes.procedural_bunny_mesh(2), lamp)
    b.parallelogram([v3(-4, -1, -4), v3(4, -1, -4), v3(-4, -1, 4)], grey)
    b.parallelogram([v3(-1, 3, -1), v3(1, 3, -1), v3(-1, 3, 1)], img)
    b.triangle([v3(2, 3, -1), v3(3, 3, -1), v3(2, 3, 1)], black)
    b.list_begin()
    b.sphere(v3(3, 0, 0), 0.5, grey)
    b.list_begin()
    b.triangle([v3(-2, 2, 0), v3(-1, 2, 0), v3(-2, 2, 2)], lamp)
    b.list_end()
    b.list_end()
    b.triangle([v3(0, 4, 0), v3(1, 4, 0), v3(2, 4, 0)], lamp)  # collinear: e1 x e2 = 0


def many_lights_world(n_lights=1100):
    """More table lights than the step stages in LDS: small emissive triangles in a grid under a ceiling, in nested lists of
    at most 550 (a HitableList holds 1024 entries), over a Lambertian floor and beside a box."""
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
                b.triangle([v3(x, 5, z), v3(x + s, 5, z), v3(x, 5 + 0.1 * rng.random(), z + s)], mats[k % 7])
            b.list_end()
            done = min(done + 550, n_lights)
    return fill


def build_custom(fill, seed=LAMP_ROOM_SEED, oracle=False):
    """(committed product scene, its Recorder[, oracle builder]) of a scene program `fill(builder)`."""
    rec = Recorder(rtmi.SceneBuilder(seed))
    fill(rec)
    rec.b.commit()
    if oracle:
        ob = oraclelib.OracleBuilder(seed)
        fill(ob)
        return rec.b, rec, ob
    return rec.b, rec


def mat_kinds_of(rec):
    return np.array([k for k, _ in materials_of(rec)], dtype=np.int64)


# ------------------------------------------------------------------ device calls
def _guarded(a, canary):
    """A device copy of the flat array a with PAD canary words behind it."""
    import torch
    a = np.ascontiguousarray(a).reshape(-1)
    full = np.concatenate([a, np.full(PAD, canary, dtype=a.dtype)])
    if full.dtype == np.uint32:
        full = full.view(np.int32)
    elif full.dtype == np.uint64:
        full = full.view(np.int64)
    return torch.from_numpy(full).cuda()


def ptr(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


def device_step(b, ps, step_no, sample, list_in=None, n_list=None, count_in=None, counts=True):
    """One rtmi_direct_sample through the C ABI on device copies of a PathState, canaries behind every array; returns
    (rc, the PathState as the call left it, whether every canary survived)."""
    import torch
    n = len(ps.O)
    if n_list is None:
        n_list = n if list_in is None else len(list_in)
    ci = np.uint32(CANARY_I)
    dev = {"O": _guarded(ps.O, CANARY_F), "D": _guarded(ps.D, CANARY_F), "H": _guarded(ps.H, np.int32(CANARY_I)),
           "steps": _guarded(ps.steps, ci), "E": _guarded(ps.E, CANARY_F), "A": _guarded(ps.A, CANARY_F),
           "LS": _guarded(np.ascontiguousarray(ps.LS.T), ci), "flags": _guarded(ps.flags, ci),
           "SO": _guarded(ps.SO, CANARY_F), "SD": _guarded(ps.SD, CANARY_F), "ST": _guarded(ps.ST, CANARY_F),
           "DR": _guarded(ps.DR, CANARY_F), "counts": _guarded(ps.counts, np.uint64(CANARY_I))}
    lst = None if list_in is None else _guarded(np.asarray(list_in, dtype=np.uint32), ci)
    cnt = None if count_in is None else _guarded(np.array([count_in], dtype=np.uint32), ci)
    rc = rtmi.lib().rtmi_direct_sample(b.h, n, ptr(lst), n_list, ptr(cnt), step_no, 1 if sample else 0, ptr(dev["O"]), ptr(dev["D"]),
                                       ptr(dev["H"]), ptr(dev["steps"]), ptr(dev["E"]), ptr(dev["A"]), ptr(dev["LS"]),
                                       ptr(dev["flags"]), ptr(dev["SO"]), ptr(dev["SD"]), ptr(dev["ST"]), ptr(dev["DR"]),
                                       ptr(dev["counts"]) if counts else None, C.c_void_p(torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    out, intact = object.__new__(PathState), True
    for k in PathState.FIELDS:
        ref = getattr(ps, k)
        raw = dev[k].cpu().numpy()
        if ref.dtype in (np.uint32, np.uint64):
            raw = raw.view(ref.dtype)
        body, tail = raw[:ref.size], raw[ref.size:]
        intact = intact and bool((tail.view(np.uint8) == np.full(PAD, CANARY_F if ref.dtype == f32 else CANARY_I,
                                                                  dtype=ref.dtype).view(np.uint8)).all())
        setattr(out, k, body.reshape(6, n).T.copy() if k == "LS" else body.reshape(ref.shape).copy())
    return rc, out, intact


def diff(a, b):
    """The fields in which two PathStates differ bit for bit (an empty list: none)."""
    return [k for k in PathState.FIELDS
            if not np.array_equal(np.ascontiguousarray(getattr(a, k)).view(np.uint8), np.ascontiguousarray(getattr(b, k)).view(np.uint8))]


def real_paths(b, O, D, seed, n_steps, compact=True):
    """The state of n real paths after n_steps steps of the trace loop on the scene b: a PathState whose rays, hit records,
    step counts and layers are those of the last step, with light states of their own; and the list that step used."""
    import torch
    n = len(O)
    o, d = torch.from_numpy(np.ascontiguousarray(O, dtype=f32)).cuda(), torch.from_numpy(np.ascontiguousarray(D, dtype=f32)).cuda()
    states = rtmi.rng_states(seed, n)
    last = {}

    def each(k, r):
        if k == n_steps - 1:
            last["list"] = None if r.paths is None else r.paths.index[:r.paths.n()].cpu().numpy().view(np.uint32).copy()
            last["H"] = r.hits.raw.cpu().numpy().copy()
    st = b.trace_steps(o, d, states, n_steps, each=each, compact=compact).check()
    LS = bouncelib.host_states(rtmi.rng_states(seed + 1, n, first=n))
    k = n_steps - 1
    ps = PathState(st.origins.cpu().numpy(), st.directions.cpu().numpy(), last["H"], st.steps.cpu().numpy().view(np.uint32),
                   st.emitted[k].cpu().numpy(), st.attenuation[k].cpu().numpy(), LS)
    return ps, last["list"]


def camera_rays(ob, h, w, spp, seed):
    """The h x w camera rays of an oracle builder's camera, spp jittered samples each: (O, D) float32 (h * w * spp, 3), made
    on the host from a numpy generator (the rays are the test's input, not the render's)."""
    rng = np.random.default_rng(seed)
    cam = np.asarray(ob.camera_get(), dtype=np.float64).reshape(7, 3)  # position, llc, horizontal, vertical, u, v, w
    n = h * w * spp
    px = np.repeat(np.arange(h * w), spp)
    x = ((px % w) + rng.random(n)) / w
    y = ((px // w) + rng.random(n)) / h
    T = cam[1][None, :] + x[:, None] * cam[2][None, :] + y[:, None] * cam[3][None, :]
    Dv = (T - cam[0][None, :]).astype(np.float64)
    Dv /= np.linalg.norm(Dv, axis=1, keepdims=True)
    return np.ascontiguousarray(np.tile(cam[0], (n, 1)), dtype=f32), np.ascontiguousarray(Dv, dtype=f32)


def moments(X):
    """(mean, variance) per channel in binary64."""
    X = np.asarray(X, dtype=np.float64)
    return X.mean(0), X.var(0, ddof=1)
