"""Every draw-dependent branch of the hot path at CHOSEN draws (tests/steerlib.py; DESIGN.md "Steered draws").

A state from a seed reaches the sampler's point (0, 0, 0), the reversed normal, a sum exactly at the rejection threshold
or a run of twelve rejections by luck or never.  Here the states are made for the draws: the step (rtmi_bounce,
rtmi_bounce_list), the trace (rtmi_trace), the render kernels and the light sampling are each run with steered states
among ordinary ones and compared with the oracle bit for bit.  Where the oracle's value is a NaN the device's must be a
NaN at the same place, with any payload; nothing else is tolerated.  Every degenerate case also asserts from the oracle's
own record that it was reached: the state advanced by the expected draws, a hit followed by the NaN ray's miss, a NaN
radiance under a Sky.

The case builders (`*_case`) are host code -- the oracle and numpy -- and cached; only the functions that take a
committed scene touch the device."""
import ctypes as C
import functools

import numpy as np
import pytest

import common
import directlib as dl
import mislib
import oraclelib
import rtmi
import steerlib as S
from bouncelib import dev, dev_states, fold, host_states, oracle_trace
from pair_slab_worlds import PLANNED
from parity import Frame, assert_same_frame, bits, states_rowmajor
from querylib import CUSTOM_WORLDS, Recorder, compare, glm_normalize, v3
from rtmi import scenes
from worlds import random_list

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

f32 = np.float32
N = 192  # three waves
CANARY = f32(-7.25)
CANARY_HIT = 0x5a5a5a5a
U32P = C.POINTER(C.c_uint32)
LAMBERTIAN, METAL = 0, 1  # scene_dev.h: MatKind (directlib.materials_of)


# ------------------------------------------------------------------ shared helpers
def pair(fill, seed):
    """(oracle builder, Recorder over the committed product builder) of one world."""
    ob, rec = oraclelib.OracleBuilder(seed), Recorder(rtmi.SceneBuilder(seed))
    fill(ob)
    fill(rec)
    rec.b.commit()
    return ob, rec


def advanced(state, k):
    s = np.array(state, dtype=np.uint32).reshape(1, 6)
    for _ in range(k):
        S.rng_next(s)
    return s[0]


def same_or_nan(got, want):
    """Bit for bit, except that where `want` holds a NaN `got` must hold a NaN too, with any payload."""
    got, want = np.asarray(got, dtype=f32), np.asarray(want, dtype=f32)
    wn = np.isnan(want)
    return got.shape == want.shape and np.array_equal(np.isnan(got), wn) and np.array_equal(bits(got)[~wn], bits(want)[~wn])


def is_axis(n):
    n = np.asarray(n, dtype=f32)
    return int((n != 0).sum()) == 1 and float(np.abs(n).max()) == 1.0


def has_sky(rec):
    return any(c[0] == "sky" for c in rec.calls)


# ================================================================== a. one step
TEXTURE = np.random.default_rng(5).integers(0, 256, (8, 8, 4), dtype=np.uint8)
MATERIALS = {"lambertian": lambda b: b.lambertian(v3(0.5, 0.25, 0.75)),
             "lambertian_tex": lambda b: b.lambertian_tex(b.image_texture(TEXTURE)),
             "metal0": lambda b: b.metal(v3(0.9, 0.8, 0.7), 0.0),
             "metal_quarter": lambda b: b.metal(v3(0.9, 0.8, 0.7), 0.25),
             "metal1": lambda b: b.metal(v3(0.9, 0.8, 0.7), 1.0),
             "dielectric": lambda b: b.dielectric(v3(1, 1, 1), 1.5)}
SAMPLES = ("lambertian", "lambertian_tex", "metal_quarter", "metal1")  # the materials whose Scatter runs the sampler
STEP_SEED = 21
# positions of the steered paths: two waves, a path on each of the four surfaces (position % 4); wave 2 is all ordinary
STEERED = ((5, 70), (7, 64))


def step_world(material):
    """Four surfaces that face up, side by side under rays that come straight down: a floor parallelogram (y = 0), a lone
    triangle (y = 0.5), a parallelepiped's top face (y = 1) and a one-face mesh (y = 0.25)."""
    def fill(b):
        b.camera_pinhole(v3(0, 3, 9), v3(0, 0, 0), v3(0, 1, 0), 0.9, 1.0)
        m = MATERIALS[material](b)
        b.parallelogram([v3(-8, 0, -1), v3(-4, 0, -1), v3(-8, 0, 1)], m)
        b.triangle([v3(-3, 0.5, -1), v3(-1, 0.5, -1), v3(-3, 0.5, 1)], m)
        b.parallelepiped([v3(1, 0, -1), v3(3, 0, -1), v3(1, 1, -1), v3(1, 0, 1)], m)
        face = np.array([[5, 0.25, -1, 7, 0.25, -1, 5, 0.25, 1]], dtype=f32)
        b.bvh(face, m, uvs=np.array([[0.1, 0.2, 0.9, 0.3, 0.4, 0.8]], dtype=f32), k_min=4)
    return fill


@functools.lru_cache(maxsize=None)
def step_pair(material):
    return pair(step_world(material), STEP_SEED)


def step_rays():
    """N rays straight down, path i onto surface i % 4, at points well inside it."""
    rng = np.random.default_rng(9)
    a, c = rng.uniform(0.05, 0.45, N), rng.uniform(0.05, 0.45, N)
    x0 = np.array([-8, -3, 1, 5], dtype=np.float64)[np.arange(N) % 4]
    span = np.array([4, 2, 2, 2], dtype=np.float64)[np.arange(N) % 4]
    O = np.stack([x0 + span * a, np.full(N, 3.0), -1 + 2 * c], axis=1).astype(f32)
    D = np.tile(np.array([0, -1, 0], dtype=f32), (N, 1))
    return np.ascontiguousarray(O), np.ascontiguousarray(D)


def oracle_step(ob, O, D, states, idx):
    """What one iteration of Trace gives paths idx: {i: (scattered, 12 floats {att, origin, dir, emitted}, state after,
    normal)} from the oracle's Hit, Scatter and Emit."""
    out = {}
    for i in idx:
        hit, rec, mat = ob.probe_hit(O[i], D[i])
        assert hit and mat >= 0, int(i)
        st = states[i].copy()
        sc, o12 = ob.probe_scatter_ex(mat, O[i], D[i], rec[0], rec[1], rec[2], rec[3:6], st)
        out[int(i)] = (sc, o12, st, rec[3:6].astype(f32))
    return out


class Step:
    """One rtmi_bounce (paths = False) or rtmi_bounce_list (paths = None: the identity list; else an index array) on
    device copies of (O, D, states (n, 6)), canaries in every output, everything read back."""

    def __init__(self, b, O, D, states, steps=None, paths=False):
        n = len(O)
        self.o, self.d, self.st = dev(O), dev(D), dev_states(states)
        em = torch.full((n, 3), float(CANARY), dtype=torch.float32, device="cuda")
        at = torch.full((n, 3), float(CANARY), dtype=torch.float32, device="cuda")
        raw = torch.full((n, 12), CANARY_HIT, dtype=torch.int32, device="cuda")
        cnt = dev(np.zeros(n, np.int32) if steps is None else steps, np.int32)
        if paths is False:
            r = b.bounce(self.o, self.d, self.st, emitted=em, attenuation=at, hits=raw, steps=cnt)
        else:
            lst = None if paths is None else rtmi.Paths(dev(np.asarray(paths, dtype=np.int32), np.int32))
            r = b.bounce_list(lst, self.o, self.d, self.st, emitted=em, attenuation=at, hits=raw, steps=cnt)
        r.check()
        self.O, self.D, self.S = self.o.cpu().numpy(), self.d.cpu().numpy(), host_states(self.st)
        self.E, self.A, self.raw = r.emitted.cpu().numpy(), r.attenuation.cpu().numpy(), r.hits.raw.cpu().numpy()
        self.steps, self.stepped = r.steps.cpu().numpy(), r.stepped()


def assert_step_is_the_oracles(s, want, O, what):
    for i, (sc, o12, st, _) in want.items():
        where = (what, i)
        assert sc, where  # (every surface faces the ray)
        assert s.steps[i] == 1, where
        assert np.array_equal(s.S[i], st), (where, "state")
        assert np.array_equal(bits(s.E[i]), bits(o12[9:12])), (where, "emitted")
        assert np.array_equal(bits(s.A[i]), bits(o12[0:3])), (where, "attenuation")
        assert np.array_equal(bits(s.O[i]), bits(o12[3:6])), (where, "origin")
        with np.errstate(all="ignore"):
            assert same_or_nan(glm_normalize(s.D[i]), o12[6:9]), (where, "direction", s.D[i].tolist(), o12[6:9].tolist())


def assert_same_words(a, b, idx, what):
    """Paths idx of steps a and b hold the same words (NaNs of a at the NaNs of b)."""
    for name in ("O", "D", "E", "A"):
        assert same_or_nan(getattr(a, name)[idx], getattr(b, name)[idx]), (what, name)
    assert np.array_equal(a.S[idx], b.S[idx]), (what, "states")
    assert np.array_equal(a.raw[idx], b.raw[idx]), (what, "hit records")
    assert np.array_equal(a.steps[idx], b.steps[idx]), (what, "steps")


def assert_untouched(s, idx, O, D, states, steps, what):
    assert same_or_nan(s.O[idx], O[idx]) and same_or_nan(s.D[idx], D[idx]), what
    assert np.array_equal(s.S[idx], states[idx]) and np.array_equal(s.steps[idx], steps[idx]), what
    assert (s.E[idx] == CANARY).all() and (s.A[idx] == CANARY).all() and (s.raw[idx] == CANARY_HIT).all(), what


@pytest.mark.parametrize("material", sorted(MATERIALS))
def test_one_step_at_steered_draws(material):
    """rtmi_bounce and rtmi_bounce_list on 192 paths, every named point at two positions in different waves.  The steered
    paths are the oracle's; every OTHER path holds the words it holds when the steered states are swapped for ordinary ones
    -- the test of the division forms of trace_helpers.h on ordinary operands, which a wave takes only with such a
    neighbour -- and that ordinary batch is the oracle's path by path.  Then the documented difference, as documented."""
    ob, rec = step_pair(material)
    b = rec.b
    O, D = step_rays()
    base = oraclelib.rng_init(STEP_SEED, N, first=500)
    every = np.arange(N)
    # the ordinary batch: the oracle's, hit records included
    ref = Step(b, O, D, base)
    want = oracle_step(ob, O, D, base, every)
    assert ref.stepped == N
    assert_step_is_the_oracles(ref, want, O, material)
    assert compare(ref.raw, ob, O, D, rec) == []
    normals = {i: w[3] for i, w in want.items()}
    assert all(is_axis(n) and n[1] == 1 for n in normals.values())
    # a list in descending order that leaves every seventh path out, the steered positions never
    keep = np.array([i for i in every[::-1] if i % 7 != 3 or i in (5, 70, 7, 64)], dtype=np.int32)
    out = np.setdiff1d(every, keep)
    ref_list = Step(b, O, D, base, paths=keep)
    assert ref_list.stepped == len(keep)
    assert_same_words(ref_list, ref, keep, "listed against plain")
    assert_untouched(ref_list, out, O, D, base, np.zeros(N, np.int32), "unlisted")
    nan_seen = 0
    for name in S.POINT_NAMES:
        for pos in STEERED:
            states = base.copy()
            for k, i in enumerate(pos):
                states[i] = S.point_state(name, normals[i], d=0x5000 + 16 * k)
            pos = list(pos)
            others = np.setdiff1d(every, pos)
            what = "%s, %s at %s" % (material, name, pos)
            steered = oracle_step(ob, O, D, states, pos)
            for i in pos:  # the oracle's own record that the case is the named one
                sc, o12, st, _ = steered[i]
                draws = 0 if material not in SAMPLES else 3 if S.ACCEPTED[name] else 6
                assert np.array_equal(st, advanced(states[i], draws)), (what, "draws")
                nan = (material.startswith("lambertian") and name in S.NAN_LAMBERTIAN) or \
                      (material == "metal1" and name in S.NAN_METAL_FUZZ1)
                assert np.isnan(o12[6:9]).all() == np.isnan(o12[6:9]).any() == nan, (what, o12[6:9].tolist())
            runs = [("rtmi_bounce", Step(b, O, D, states), ref, every),
                    ("rtmi_bounce_list, identity", Step(b, O, D, states, paths=None), ref, every),
                    ("rtmi_bounce_list, a list", Step(b, O, D, states, paths=keep), ref_list, keep)]
            for entry, s, plain, listed in runs:
                assert s.stepped == len(listed), (what, entry)
                assert_step_is_the_oracles(s, steered, O, (what, entry))
                assert np.array_equal(s.raw[pos], plain.raw[pos]), (what, entry, "hit records of the steered paths")
                assert_same_words(s, plain, np.intersect1d(others, listed), (what, entry, "the other paths"))
            assert_untouched(runs[2][1], out, O, D, states, np.zeros(N, np.int32), (what, "unlisted"))
            bad = [i for i in pos if np.isnan(steered[i][1][6:9]).any()]
            if not bad:
                continue
            # the documented difference (include/rtmi.h): the next step skips a bad scattered ray, the path stays alive
            # with the steps it has, and the fold cuts it as Trace cuts an alive path -- where Trace follows the NaN
            nan_seen += len(bad)
            first = runs[0][1]
            for i in bad:
                assert np.isnan(first.D[i]).any() or not first.D[i].any(), (what, first.D[i].tolist())
            second = Step(b, first.O, first.D, first.S, steps=first.steps)
            assert_untouched(second, np.array(bad), first.O, first.D, first.S, first.steps, (what, "second step"))
            assert (second.steps[others] == 2).all()  # (every other path scattered, and was stepped again)
            E, A = np.stack([first.E, second.E]), np.stack([first.A, second.A])
            got = rtmi.path_fold(dev(second.D), dev(second.steps, np.int32), dev(E), dev(A)).cpu().numpy()
            assert same_or_nan(got, fold(second.D, second.steps, E, A)), (what, "fold")
            for i in bad:  # one layer: E[0] for a zero direction (ended), E[0] + A[0] * 0 for a NaN one (alive, cut)
                assert np.array_equal(bits(got[i]), bits((first.E[i] + (first.A[i] * f32(0))).astype(f32))), (what, "fold", i)
                assert not np.isnan(got[i]).any()
    expected = {"lambertian": 3, "lambertian_tex": 3, "metal1": 2}.get(material, 0) * 4
    assert nan_seen == expected, (material, nan_seen)


# ================================================================== b. rtmi_trace
DEPTHS = (2, 3, 10)
TRACE_POSITIONS = [3, 9, 17, 30, 41, 59, 66, 70, 85, 99, 110, 127, 22, 77, 50, 120, 1, 63]  # waves 0 and 1; wave 2 is ordinary


class _Fuzz1:
    """A builder that passes every call on, with every Metal's fuzz set to 1: the reflection of a ray that comes in along
    the reversed normal is then cancelled exactly by the sampler's point -n."""

    def __init__(self, b):
        self.b = b

    def __getattr__(self, name):
        return getattr(self.b, name)

    def metal(self, rgb, fuzz):
        return self.b.metal(rgb, 1.0)


@functools.lru_cache(maxsize=None)
def trace_pair(name, fuzz1):
    wrap = _Fuzz1 if fuzz1 else (lambda b: b)
    if name in CUSTOM_WORLDS:
        seed = 7
        return pair(lambda b: CUSTOM_WORLDS[name](wrap(b)), seed) + (seed,)
    scene, kw = (("bunny", {"k_min": 4}) if name == "bunny_kmin4" else (name, {}))
    seed = common.scene_seed(scene)
    return pair(lambda b: common.build_scene(wrap(b), scene, 1.0, **kw), seed) + (seed,)


@functools.lru_cache(maxsize=None)
def trace_case(name, fuzz1=False):
    """192 rays of a query world and their states, the first bounce of up to 18 of them steered: `zero` on rays that hit
    a Lambertian, `minus_n` on rays that hit a Lambertian with an axis normal, `metal_cancel` (worlds with fuzz 1) on
    axis rays that hit a Metal head on; the other paths of the first two waves scatter on a Lambertian too where the world
    has such rays, the third wave holds whatever is left (misses, metals, lights).  The rays run along the axes from origins on a grid of 2^-6, so that the raw
    camera's o + d is exact and the ray's direction is the axis itself.  Returns (ob, rec, seed, O, D, states,
    {position: point name})."""
    ob, rec, seed = trace_pair(name, fuzz1)
    kinds = dl.mat_kinds_of(rec)
    rng = np.random.default_rng(4000 + len(name))
    # the scene's extent: the first hits of a grid of camera rays
    P = []
    for y in np.linspace(-0.9, 0.9, 16):
        for x in np.linspace(-0.9, 0.9, 16):
            ray = ob.probe_camera_ray(x, y)
            hit, out, _ = ob.probe_hit(ray[:3], ray[3:])
            if hit and out[0] < 1e8:
                P.append(ray[:3] + f32(out[0]) * ray[3:])
    P = np.array(P)
    lo, hi = np.percentile(P, 10, axis=0), np.percentile(P, 90, axis=0)  # (a ground sphere is hit out to the horizon)
    lo, hi = lo - 0.1 * (hi - lo), hi + 0.25 * (hi - lo)
    n_cand = 4000
    O = (np.round((lo + rng.random((n_cand, 3)) * (hi - lo)) * 64) / 64).astype(f32)
    D = np.zeros((n_cand, 3), dtype=f32)
    D[np.arange(n_cand), rng.integers(0, 3, n_cand)] = rng.choice([-1.0, 1.0], n_cand)
    assert np.array_equal((O + D).astype(f32) - O, D)  # exact: the raw camera's direction is D
    zero, minus_n, cancel, diffuse, rest = [], [], [], [], []
    for i in range(n_cand):
        hit, out, mat = ob.probe_hit(O[i], D[i])
        n = out[3:6].astype(f32)
        if hit and mat >= 0 and not float(np.dot(D[i], n)) < 0:  # (from inside a sphere: Scatter returns false, nothing is drawn)
            rest.append(i)
        elif hit and mat >= 0 and kinds[mat] == LAMBERTIAN and is_axis(n) and len(minus_n) < 6:
            minus_n.append((i, n))
        elif hit and mat >= 0 and kinds[mat] == LAMBERTIAN and len(zero) < 6:
            zero.append((i, n))
        elif fuzz1 and hit and mat >= 0 and kinds[mat] == METAL and is_axis(n) and np.array_equal(D[i], -n) and len(cancel) < 6:
            cancel.append((i, n))
        elif hit and mat >= 0 and kinds[mat] == LAMBERTIAN:
            diffuse.append(i)
        else:
            rest.append(i)
    if len(zero) < 4:  # a world of axis-aligned surfaces only: `zero` needs no particular normal
        zero += minus_n[3:]
        minus_n = minus_n[:3]
    steered = [(i, n, "zero") for i, n in zero] + [(i, n, "minus_n") for i, n in minus_n] + [(i, n, "metal_cancel") for i, n in cancel]
    assert len(steered) <= len(TRACE_POSITIONS)
    # the steered paths' neighbours, waves 0 and 1, are rays that scatter on a Lambertian at their first hit as far as
    # there are such rays: they normalise a new direction in the very iteration the steered lane's is degenerate, and
    # so go through the division forms with it
    near = diffuse[:128]
    order = np.array(near + rest[:N - len(near)], dtype=np.int64)
    assert len(order) == N and len(near) >= 32, (name, len(near))
    names = {}
    for k, (i, n, point) in enumerate(steered):
        order[TRACE_POSITIONS[k]] = i
        names[TRACE_POSITIONS[k]] = (point, n)
    O, D = np.ascontiguousarray(O[order]), np.ascontiguousarray(D[order])
    states = oraclelib.rng_init(seed + 1, N, first=777)
    for pos, (point, n) in names.items():
        # (an axis for `zero` on a surface that has none: the point does not depend on it)
        states[pos] = S.point_state(point, n if is_axis(n) else (0, 1, 0), lead=(S.CENTRE, S.CENTRE), d=0x7000 + pos)
    return ob, rec, seed, O, D, states, {p: v[0] for p, v in names.items()}


def run_trace_case(name, fuzz1, need):
    """rtmi_trace of the case at depths 2, 3 and 10 against the oracle's Trace: radiance, ray counts, final states."""
    ob, rec, seed, O, D, states, names = trace_case(name, fuzz1)
    b = rec.b
    got_points = sorted(names.values())
    for point, least in need.items():
        assert got_points.count(point) >= least, (name, point, got_points)
    sky = has_sky(rec)
    for depth in DEPTHS:
        o_rgb, o_rays, o_fin, dirs, handed = oracle_trace(ob, O, D, states, depth)
        assert np.array_equal(bits(dirs), bits(D))
        for pos, point in names.items():  # the oracle's own record: the hit, the sampler's three draws, the NaN ray's query
            where = (name, depth, pos, point)
            assert o_rays[pos] == 2 and np.array_equal(o_fin[pos], advanced(states[pos], 5)), where
            assert np.isnan(o_rgb[pos]).all() if sky else not o_rgb[pos].any(), (where, o_rgb[pos].tolist())
        st = dev_states(handed)
        tr = b.trace(dev(O), dev(D), st, depth, count_rays=True).check()
        rgb, rays, fin = tr.rgb.cpu().numpy(), tr.rays.cpu().numpy().view(np.uint32), host_states(st)
        wn = np.isnan(o_rgb)
        bad = np.flatnonzero((np.isnan(rgb) != wn).any(1) | ((bits(rgb) != bits(o_rgb)) & ~wn).any(1) | (rays != o_rays) |
                             (fin != o_fin).any(1))
        assert bad.size == 0, (name, depth, bad[:8].tolist(), [names.get(int(i)) for i in bad[:8]], rgb[bad[:4]].tolist(),
                               o_rgb[bad[:4]].tolist(), rays[bad[:4]].tolist(), o_rays[bad[:4]].tolist())
        assert tr.total_rays() == int(o_rays.sum())
    if sky:
        assert np.isnan(o_rgb).any(1).sum() == len(names)  # no NaN but the steered ones'


@pytest.mark.parametrize("name", ["cornell_box", "quilt_40"])
def test_trace_follows_the_nan_ray_list_only(name):
    """Worlds of list triangles alone, both under a Sky (the NaN ray finds it: the radiance is NaN): the Cornell box, all
    axis-aligned Lambertians, and forty patches of Lambertian and Metal.  The NaN direction goes through the pair cull with
    its clamped reciprocals and the shared triangle tests (DESIGN.md "Steered draws": why each loop terminates)."""
    run_trace_case(name, False, {"zero": 3, "minus_n": 3} if name == "cornell_box" else {"zero": 4})


@pytest.mark.parametrize("name,fuzz1", [("no_sky", False), ("nested", False), ("spheres", False), ("no_sky", True), ("nested", True)])
def test_trace_follows_the_nan_ray_spheres(name, fuzz1):
    """Worlds with spheres: the discriminant culls of the plain loop and, in `spheres`, the grouped scan, which a NaN ray
    overflows into the plain loop.  With every fuzz at 1 the Metal's cancelled reflection joins the Lambertian cases."""
    need = {"zero": 2} if name == "spheres" else {"zero": 2, "minus_n": 2}
    if fuzz1:
        need["metal_cancel"] = 1
    run_trace_case(name, fuzz1, need)


@pytest.mark.parametrize("name", ["textured_mesh", "bunny_kmin4"])
def test_trace_follows_the_nan_ray_meshes(name):
    """Worlds with meshes: the NaN ray passes the root pre-test, walks the whole 4-wide tree and fails every triangle test."""
    run_trace_case(name, False, {"zero": 4})


# ================================================================== c. the render kernels
QUEUE = dict(lane_stride=1, schedule=0)
LAUNCHES = {"queue": (8, QUEUE), "planned": (64, PLANNED)}
RENDER_DEPTH = 9
SCENES = {"cornell_box": (lambda b: scenes.cornell_box(b, 1.0), scenes.SCENE_SEEDS["cornell_box"], 16, 16, (895, 767)),
          "random_list": (lambda b: random_list()(b, 2.0), 11, 32, 64, (383, 255))}
POINTS_IN_FRAMES = ("zero", "minus_n", "plus_n", "boundary_accept", "boundary_reject", "corner", "zero", "minus_n")


@functools.lru_cache(maxsize=None)
def render_pair(scene):
    fill, seed, h, w, _ = SCENES[scene]
    return pair(fill, seed)


def centre_hit(ob, h, w, idx, jitter=(0.5, 0.5)):
    """The oracle's first hit of pixel idx's ray with the given jitter (ray_tracing.cu:68-73): (hit, record, material)."""
    i, j = divmod(int(idx), w)
    x = 2 * ((float(f32(jitter[0])) + float(j)) / float(w)) - 1
    y = 2 * ((float(f32(jitter[1])) + float(h - i)) / float(h)) - 1
    ray = ob.probe_camera_ray(x, y)
    return ob.probe_hit(ray[:3], ray[3:])


@functools.lru_cache(maxsize=None)
def render_case(scene):
    """The frame's states, some of them steered: (states (h * w, 6), {pixel: point name}, {pixel: run length}).  Draws 1
    and 2 of a steered pixel are the pixel's centre, draws 3 to 5 a named point for the normal of the Lambertian its centre
    ray hits.  Two steered pixels share a wave's tile of 8 x 8, the others are spread over the other tiles, and every
    tile with such a surface gets one degenerate pixel (`zero` or `minus_n`); the frame's first and
    last pixel are steered too (to a point where their centre ray hits such a surface, else to jitter draws 0xffffffff and
    0).  Two more pixels start with a run of twelve or more rejections behind their own jitter."""
    _, seed, h, w, _ = SCENES[scene]
    ob, rec = render_pair(scene)
    kinds = dl.mat_kinds_of(rec)
    normal = {}
    for idx in range(h * w):
        hit, out, mat = centre_hit(ob, h, w, idx)
        if hit and mat >= 0 and kinds[mat] == LAMBERTIAN and is_axis(out[3:6]):
            normal[idx] = out[3:6].astype(f32)
    tile = lambda idx: (idx // w // 8, idx % w // 8)
    by_tile = {}
    for idx in sorted(normal):
        by_tile.setdefault(tile(idx), []).append(idx)
    first, last = 0, h * w - 1
    shared = next(t for t in sorted(by_tile) if len(by_tile[t]) >= 8 and t not in (tile(first), tile(last)))
    chosen = [by_tile[shared][1], by_tile[shared][6]]
    spread = [t for t in sorted(by_tile, key=lambda t: (t[0] * 7 + t[1] * 3) % 11) if t != shared]  # tiles all over the frame
    for turn in range(4):  # (16 x 16 has four tiles in all: a second round takes another pixel of each)
        for t in spread:
            cand = [p for p in by_tile[t][turn + 1::5] if p not in (first, last)]
            if len(chosen) < len(POINTS_IN_FRAMES) and cand:
                chosen.append(cand[0])
    assert len(chosen) == len(set(chosen)) == len(POINTS_IN_FRAMES) and len({tile(p) for p in chosen}) >= 3, chosen
    states = oraclelib.rng_init(seed, h * w)
    states[0] = ob.state0  # (pixel 0 continues the scene program's stream)
    points = dict(zip(chosen, POINTS_IN_FRAMES))
    # ... and one degenerate pixel in every tile that has none yet: each pulls its wave through the division forms once,
    # at the first bounce, and a wrong division form shows in few of the lanes that go with it
    for k, t in enumerate(sorted(by_tile)):
        if not any(tile(p) == t and points[p] in S.NAN_LAMBERTIAN for p in points):
            spare = [p for p in by_tile[t] if p not in points and p not in (first, last)]
            if spare:
                points[spare[len(spare) // 3]] = ("zero", "minus_n")[k % 2]
    for idx, point in ((first, "zero"), (last, "minus_n")):
        if idx in normal:
            points[idx] = point
        else:
            states[idx] = S.state_for([0xffffffff, 0] if idx == first else [0, 0xffffffff], d=0x9000 + idx)
    for idx, point in points.items():
        states[idx] = S.point_state(point, normal[idx], lead=(S.CENTRE, S.CENTRE), d=0x9000 + idx)
    # the long runs: a state of the family on a pixel whose ray, with the state's OWN jitter, hits a Lambertian
    run_states, run_len = S.search_runs(min_run=12, skip=2)
    runs, taken = {}, set(points) | {first, last}
    free = [p for p in sorted(normal) if p not in taken][3::7]
    for st, length in zip(run_states, run_len):
        if len(runs) == 2:
            break
        jit = S.rng_01_of(S.draws_of(st, 2))
        for idx in free:
            hit, out, mat = centre_hit(ob, h, w, idx, jit)
            if idx not in runs and hit and mat >= 0 and kinds[mat] == LAMBERTIAN:
                states[idx] = st
                runs[idx] = int(length)
                break
    assert len(runs) == 2, runs
    return states, points, runs


def render_pins(pb, h, w, spp, depth, opts):
    """(first pass, finishing launch): the mode words of the kernels a render of this frame would launch."""
    R = rtmi.Renderer(pb, h, w, spp, depth, True)
    out = (C.c_uint32 * 2)()
    with torch.cuda.device(R.device):
        rc = R.L.rtmi_render_pins(R.scene.h, C.byref(R.frame), C.byref(rtmi.render_opts(**opts)), out)
    assert rc == 0, R.L.rtmi_last_error()
    return int(out[0]), int(out[1])


def steered_frame(pb, h, w, spp, depth, states, opts=None, post=True):
    """parity.gpu_frame with the renderer's state planes overwritten, behind init_rng, by `states` ((h * w, 6), row-major)."""
    ro = rtmi.render_opts(**opts) if opts is not None else None
    R = rtmi.Renderer(pb, h, w, spp, depth, post).init_rng()
    pm = rtmi.pixel_map(R.frame)
    planes = R.states.cpu().numpy().view(np.uint32).copy()
    planes[:, pm >= 0] = states[pm[pm >= 0]].T
    R.states.copy_(torch.from_numpy(planes.view(np.int32)))
    R.render(opts=ro)
    R.check()
    total = R.total_rays()
    img, cnt = R.untile()
    torch.cuda.synchronize()
    return Frame(img.cpu().numpy(), cnt.cpu().numpy().astype(np.uint32), states_rowmajor([R.states], h, w), total, R.mode(ro))


def oracle_steered(ob, h, w, spp, depth, states, post=True):
    rgb, rays, fin, total = ob.render(h, w, spp, depth, post=post, states=states.copy())
    return Frame(rgb, rays, fin, total, None)


def assert_same_buffers(a, b, what):
    assert a.total == b.total and np.array_equal(a.counts, b.counts) and np.array_equal(a.states, b.states), what
    assert same_or_nan(a.image, b.image), what


@pytest.mark.parametrize("scene", sorted(SCENES))
def test_steered_pixels_are_what_they_are_named(scene):
    """The oracle's own record of the steered pixels, one sample each.  At depth 1 Trace makes the hit, Scatter and the
    query that ends the path: the state has advanced by the two jitter draws and the sampler's 3, 6 or 3 (run + 1).  At the
    renders' depth a degenerate pixel makes exactly two queries -- the hit and the NaN ray's -- and its radiance is NaN
    under the Sky (0 in a world without one).  (Host work, but it holds the GPU cases up: a scene that changes fails here.)"""
    _, _, h, w, _ = SCENES[scene]
    ob, rec = render_pair(scene)
    states, points, runs = render_case(scene)
    assert set(POINTS_IN_FRAMES) <= set(points.values()) and len(points) >= 8
    one = oracle_steered(ob, h, w, 1, 1, states, post=False)
    for idx, point in points.items():
        assert np.array_equal(one.states[idx], advanced(states[idx], 2 + (3 if S.ACCEPTED[point] else 6))), (idx, point)
        assert one.counts.reshape(-1)[idx] == 2
    for idx, length in runs.items():
        assert length >= 12 and np.array_equal(one.states[idx], advanced(states[idx], 2 + 3 * (length + 1))), (idx, length)
    deep = oracle_steered(ob, h, w, 1, RENDER_DEPTH, states, post=False)
    nan = [idx for idx, point in points.items() if point in S.NAN_LAMBERTIAN]
    assert len(nan) >= 4
    for idx in nan:
        assert deep.counts.reshape(-1)[idx] == 2, idx
        px = deep.image.reshape(-1, 3)[idx]
        assert np.isnan(px).all() if has_sky(rec) else not px.any(), (idx, px.tolist())
    if has_sky(rec):
        assert np.isnan(deep.image.reshape(-1, 3)).any(1).sum() == len(nan)


@pytest.mark.parametrize("launch", sorted(LAUNCHES))
@pytest.mark.parametrize("scene", sorted(SCENES))
def test_render_kernels_at_steered_draws(scene, launch):
    """The frame by the launch's pinned kernels, by the general kernel and by the oracle, from the same steered states:
    image (NaNs where the oracle's are), per-pixel ray counts, final states, ray total."""
    _, _, h, w, (queue_pins, chain_pins) = SCENES[scene]
    ob, rec = render_pair(scene)
    states, points, runs = render_case(scene)
    spp, opts = LAUNCHES[launch]
    what = "%s, %s" % (scene, launch)
    want = oracle_steered(ob, h, w, spp, RENDER_DEPTH, states)
    fast_opts, slow_opts = dict(fast_path=1, **opts), dict(fast_path=-1, **opts)
    pins = (0, queue_pins) if launch == "queue" else (queue_pins, chain_pins)
    assert render_pins(rec.b, h, w, spp, RENDER_DEPTH, fast_opts) == pins, what
    assert render_pins(rec.b, h, w, spp, RENDER_DEPTH, slow_opts) == (0, 0), what
    fast = steered_frame(rec.b, h, w, spp, RENDER_DEPTH, states, fast_opts)
    assert fast.mode["fast_path"] == 1 and fast.mode["planned_chains"] == (launch == "planned"), fast.mode
    assert_same_frame(fast, want, what + ", the pinned kernels", nan_ok=True)
    general = steered_frame(rec.b, h, w, spp, RENDER_DEPTH, states, slow_opts)
    assert general.mode["fast_path"] == 0, general.mode
    assert_same_frame(general, want, what + ", the general kernel", nan_ok=True)
    assert_same_buffers(fast, general, what + ", pinned against general")


# ------------------------------------------------------------------ jitter and lens extremes
EXTREMES = [(0, 0), (0xffffffff, 0), (0, 0xffffffff), (0xffffffff, 0xffffffff)]


def camera_pair(camera, h, w):
    def fill(b):
        if camera == "pinhole":
            scenes.cornell_box(b, w / h)
        else:
            scenes.mixed(b, w / h)
            b.camera_defocus([0.5, 1.5, 6], [0, 0.8, 0], [0, 1, 0], np.pi / 4, w / h, 0.3, 5.5)
    return pair(fill, 1024)


@pytest.mark.parametrize("hw", [(16, 16), (24, 40)], ids=lambda hw: "%dx%d" % hw)
@pytest.mark.parametrize("camera", ["pinhole", "defocus"])
def test_jitter_and_lens_extremes_on_the_corner_pixels(camera, hw):
    """Draws 0 and 0xffffffff -- jitter 2^-33 and exactly 1.0, so xf == 1.0 on the last column -- on the four corner
    pixels, in both assignments; the defocus camera's lens draws get the same extremes.  16 x 16 takes the binary32 jitter
    form, 24 x 40 the binary64 one.  rtmi_camera_rays and a render of two samples against the oracle."""
    h, w = hw
    ob, rec = camera_pair(camera, h, w)
    corners = [0, w - 1, (h - 1) * w, h * w - 1]
    for turn in (0, 1):
        states = oraclelib.rng_init(1024, h * w)
        states[0] = ob.state0
        for k, idx in enumerate(corners):
            draws = list(EXTREMES[(k + turn) % 4])
            if camera == "defocus":
                draws += list(EXTREMES[(k + 2 * turn + 1) % 4])
            states[idx] = S.state_for(draws, d=0xa000 + idx)
        # the rays
        R = rtmi.Renderer(rec.b, h, w, 1, 5, post=False).init_rng()
        pm = rtmi.pixel_map(R.frame)
        planes = R.states.cpu().numpy().view(np.uint32).copy()
        planes[:, pm >= 0] = states[pm[pm >= 0]].T
        R.states.copy_(torch.from_numpy(planes.view(np.int32)))
        o, d = R.camera_rays(0)
        O, D, after = o.cpu().numpy(), d.cpu().numpy(), host_states(R.states)
        L = oraclelib.lib()
        for q in np.flatnonzero(pm >= 0):
            idx = int(pm[q])
            if idx not in corners and idx % 7:
                continue
            s = states[idx].copy()
            r1 = float(L.orc_random_float(C.c_float(0.0), C.c_float(1.0), s.ctypes.data_as(U32P)))
            r2 = float(L.orc_random_float(C.c_float(0.0), C.c_float(1.0), s.ctypes.data_as(U32P)))
            i, j = divmod(idx, w)
            x, y = 2 * ((r1 + float(j)) / float(w)) - 1, 2 * ((r2 + float(h - i)) / float(h)) - 1
            ray = ob.probe_camera_ray(x, y, s)
            where = (camera, hw, turn, idx)
            if idx in corners:
                assert {r1, r2} <= {2.0 ** -33, 1.0}, where
            assert np.array_equal(bits(O[q]), bits(ray[:3])), where
            assert np.array_equal(bits(glm_normalize(D[q])), bits(ray[3:])), where
            assert np.array_equal(after[q], s), where
        # the render
        got = steered_frame(rec.b, h, w, 2, 5, states, post=False)
        assert_same_frame(got, oracle_steered(ob, h, w, 2, 5, states, post=False), "%s %dx%d turn %d" % (camera, h, w, turn),
                          nan_ok=True)


# ================================================================== d. light sampling
LIGHT_SEED = 31
UP = lambda x: np.nextafter(f32(x), f32(2))
R0_CASES = [(0.25, 0), (0.5, 1), (0.75, 2), (1.0, 3), (UP(0.25), 1), (UP(0.5), 2), (UP(0.75), 3), (2.0 ** -33, 0)]  # (r0, light)
R12_CASES = [(0.5, 0.5), (0.5, 0.5 + 2.0 ** -24), (0.5, 0.5 + 2.0 ** -23)]  # r1 + r2: 1, rounds to 1, the first sum above 1


def four_lights(b):
    """A Lambertian floor under four lights of area 16 and the same emission -- three parallelograms and one triangle --
    so the cdf is 0.25, 0.5, 0.75, 1 exactly."""
    b.camera_pinhole(v3(0, 1, 9), v3(0, 1, 0), v3(0, 1, 0), 0.9, 1.0)
    grey = b.lambertian(v3(0.6, 0.6, 0.6))
    lamp = b.diffuse_light(b.constant_texture(v3(3, 3, 3)))
    b.parallelogram([v3(-4, 0, -4), v3(4, 0, -4), v3(-4, 0, 4)], grey)
    b.parallelogram([v3(-4, 2, -4), v3(0, 2, -4), v3(-4, 2, 0)], lamp)
    b.triangle([v3(0, 2.5, -4), v3(4, 2.5, -4), v3(0, 2.5, 4)], lamp)
    b.parallelogram([v3(-4, 2, 0), v3(0, 2, 0), v3(-4, 2, 4)], lamp)
    b.parallelogram([v3(0, 2, 0), v3(4, 2, 0), v3(0, 2, 4)], lamp)
    return b


def inside(light, so, sd):
    """Barycentric coordinates, in binary64, of the point where the ray (so, sd) meets the light's plane: (u, v) for a
    parallelogram, (u, v, 1 - u - v) for a triangle -- and 1 - u, 1 - v for the parallelogram's far edges."""
    p0, e1, e2 = (np.asarray(light[k], dtype=np.float64) for k in ("p0", "e1", "e2"))
    so, sd = np.asarray(so, dtype=np.float64), np.asarray(sd, dtype=np.float64)
    nrm = np.cross(e1, e2)
    t = np.dot(p0 - so, nrm) / np.dot(sd, nrm)
    rel = so + t * sd - p0
    u = np.dot(np.cross(rel, e2), nrm) / np.dot(nrm, nrm)
    v = np.dot(np.cross(e1, rel), nrm) / np.dot(nrm, nrm)
    return (u, v, 1 - u - v) if int(light["kind"]) == 1 else (u, v, 1 - u, 1 - v)


def test_light_selection_ties_and_the_triangle_flip():
    """rtmi_direct_sample and rtmi_direct_sample_mis with the LIGHT states steered: r0 exactly a cdf entry ("smallest j with
    r0 <= cdf[j]"), one ulp above it, 2^-33 and 1.0; (r1, r2) with r1 + r2 exactly 1, 1 + 2^-24 (which rounds to 1: no flip)
    and 1 + 2^-23 (the flip).  Both entries against their numpy restatements bit for bit; the picked light asserted; and,
    independent of the restatements, the sample point lies inside that light in binary64 (coordinates >= -2^-22)."""
    b, rec = dl.build_custom(four_lights, seed=LIGHT_SEED)
    tab, kinds = dl.table_of(rec), dl.mat_kinds_of(rec)
    assert dl.same_table(b.lights(), tab)
    assert tab["cdf"].tolist() == [0.25, 0.5, 0.75, 1.0] and tab["kind"].tolist() == [0, 1, 0, 0]
    rng = np.random.default_rng(3)
    O = np.stack([rng.uniform(-2, 2, N), np.full(N, 1.5), rng.uniform(-2, 2, N)], axis=1).astype(f32)
    D = np.tile(np.array([0, -1, 0], dtype=f32), (N, 1))
    ps, _ = dl.real_paths(b, O, D, LIGHT_SEED, 1)
    assert (ps.steps == 1).all() and (ps.D != 0).any(1).all()  # every path scattered on the floor
    cases = [(r0, j, r12) for r0, j in R0_CASES for r12 in R12_CASES]
    where = {}
    for k, (r0, j, (r1, r2)) in enumerate(cases):
        pos = (k * 5 + 2) % 128  # waves 0 and 1, spread; wave 2 keeps its seeded light states
        assert pos not in where
        ps.LS[pos] = S.state_for([S.draw_for_01(r0), S.draw_for_01(r1), S.draw_for_01(r2)], d=0xb000 + k)
        where[pos] = (f32(r0), j, f32(r1), f32(r2))
    for pos, (r0, j, r1, r2) in where.items():  # the rule itself, on the table
        assert int(np.searchsorted(tab["cdf"], r0, side="left")) == j, (pos, float(r0))
    for entry, state, lib in (("rtmi_direct_sample", ps, dl), ("rtmi_direct_sample_mis", mislib.PathState.of(ps), mislib)):
        want = lib.step(tab, kinds, state.copy(), 0, 1)
        rc, got, intact = lib.device_step(b, state, 0, 1)
        assert rc == 0 and intact, (entry, rtmi.lib().rtmi_last_error())
        bad = lib.diff(got, want)
        assert bad == [], (entry, bad, [np.flatnonzero((bits(getattr(got, k)) != bits(getattr(want, k))).reshape(N, -1).any(1))[:8]
                                        for k in bad if k != "counts"])
        for pos, (r0, j, r1, r2) in where.items():
            assert got.ST[pos] > 0, (entry, pos)  # a valid sample: the floor faces every light
            assert np.array_equal(got.LS[pos], advanced(ps.LS[pos], 3)), (entry, pos)
            coords = inside(tab[j], got.SO[pos], got.SD[pos])
            assert min(coords) >= -2.0 ** -22, (entry, pos, j, coords)
            others = [min(inside(tab[k], got.SO[pos], got.SD[pos])) for k in range(4) if k != j and tab["p0"][k][1] == tab["p0"][j][1]]
            assert all(c < -1e-3 for c in others), (entry, pos, j, others)  # ... and in no other light of that plane
            if int(tab["kind"][j]) == 1:  # the triangle: on its hypotenuse, a step of 2^-24 past it, or flipped back inside
                flipped = f32(r1 + r2) > 1
                assert flipped == (r2 == f32(0.5 + 2.0 ** -23)), (pos, float(r1), float(r2))
                assert abs(coords[2] - (2.0 ** -23 if flipped else float(1 - np.float64(r1) - np.float64(r2)))) < 2.0 ** -22, coords
