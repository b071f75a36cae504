"""Sphere table lights without a device: rtmi_scene_light_kinds' refusals and binding, the table's sphere records on
flattened scenes, and the numpy restatement of the step (tests/spherelightlib.py) held to closed forms in binary64 -- the
cone's opening, the frame, the direction inside the cone, the distance to the sphere, the draws the rejection loop takes,
the two sides of the balance weight, and the estimator's mean against the analytic irradiance of a sphere."""
import inspect
import math
import os
import re

import numpy as np
import pytest

import directlib as dl
import mislib as ml
import rtmi
import spherelightlib as sl
from abi_host import ERR_INVALID
from parity import bits
from querylib import Recorder

f32 = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _scene(fill, seed=dl.LAMP_ROOM_SEED):
    rec = Recorder(rtmi.SceneBuilder(seed))
    fill(rec)
    return rec


# ------------------------------------------------------------------ the entry and its binding
def test_the_symbol_is_declared_and_bound():
    header = open(os.path.join(ROOT, "include", "rtmi.h")).read()
    assert "rtmi_scene_light_kinds" in [s[0] for s in rtmi.SYMBOLS]
    assert re.search(r"\bint rtmi_scene_light_kinds\(rtmi_scene \*s, uint32_t kinds\);", header)
    assert re.search(r"#define RTMI_LIGHTS_FLAT\s+1u", header) and re.search(r"#define RTMI_LIGHTS_SPHERES\s+2u", header)
    assert "#define RTMI_VERSION 3" in header  # added without a version change
    assert str(inspect.signature(rtmi.SceneBuilder.light_kinds)) == "(self, spheres=False)"


@pytest.mark.parametrize("kinds", [0, 2, 4, 7, 5, 0x80000001, 0xffffffff])
def test_other_values_are_refused_with_a_reason(kinds):
    b = rtmi.SceneBuilder(1)
    assert sl.light_kinds_raw(b, kinds) == ERR_INVALID
    assert b"RTMI_LIGHTS_FLAT" in rtmi.lib().rtmi_last_error()


def test_a_null_scene_is_refused_and_1_and_3_are_accepted():
    assert sl.light_kinds_raw(None, 3) == ERR_INVALID
    assert b"null scene" in rtmi.lib().rtmi_last_error()
    b = rtmi.SceneBuilder(1)
    assert sl.light_kinds_raw(b, 1) == 0 and sl.light_kinds_raw(b, 3) == 0 and sl.light_kinds_raw(b, 1) == 0
    assert b.light_kinds(spheres=True) is b and b.light_kinds() is b


def _lit(spheres, flat=False, seed=dl.LAMP_ROOM_SEED):
    """(Recorder, restated table, material kinds) of a scene that opts in and holds a Lambertian floor (material 0, entry
    0), optionally a flat lamp, and the emissive spheres (centre, radius, emission): the tables of the tests below come
    from a scene program through the new entry, as a caller's would."""
    def fill(b):
        b.light_kinds(spheres=True)
        b.camera_pinhole(sl.v3(0, 1, 6), sl.v3(0, 0, 0), sl.v3(0, 1, 0), 0.9, 1.0)
        b.parallelogram([sl.v3(-4, -9, -4), sl.v3(4, -9, -4), sl.v3(-4, -9, 4)], b.lambertian(sl.v3(0.5, 0.5, 0.5)))
        if flat:
            b.parallelogram([sl.v3(-1, 9, -1), sl.v3(1, 9, -1), sl.v3(-1, 9, 1)], b.diffuse_light(b.constant_texture(sl.v3(2, 2, 2))))
        mats = {}
        for c, r, le in spheres:
            le = tuple(float(v) for v in le)
            if le not in mats:
                mats[le] = b.diffuse_light(b.constant_texture(sl.v3(*le)))
            b.sphere(np.asarray(c, f32), float(r), mats[le])
    rec = _scene(fill, seed)
    return rec, sl.table_of(rec), dl.mat_kinds_of(rec)


def test_a_non_finite_radius_never_reaches_the_table():
    rec = Recorder(rtmi.SceneBuilder(1))
    rec.light_kinds(spheres=True)
    rec.camera_pinhole(sl.v3(0, 1, 6), sl.v3(0, 0, 0), sl.v3(0, 1, 0), 0.9, 1.0)
    lamp = rec.diffuse_light(rec.constant_texture(sl.v3(1, 1, 1)))
    for r in (float("inf"), float("-inf"), float("nan")):
        with pytest.raises(rtmi.RtmiError):
            rec.sphere(sl.v3(0, 0, 0), r, lamp)
    rec.sphere(sl.v3(0, 0, 0), 1.0, lamp)
    tab = sl.table_of(rec)
    assert len(rec.entries()) == 1 and len(tab) == 1 and tab["e1"][0].tolist() == [1, 1, 0]


# ------------------------------------------------------------------ the restated table
def test_restated_table_of_bulb_room():
    rec = _scene(sl.with_kinds(sl.bulb_room))
    tab = sl.table_of(rec)
    assert len(tab) == 2 and (tab["kind"] == 2).all() and tab["entry"].tolist() == [6, 7] and (tab["element"] == 0).all()
    for j, (c, r, le) in enumerate(sl.BULBS):
        assert np.array_equal(tab["p0"][j], np.array(c, f32)) and np.array_equal(tab["emission"][j], np.array(le, f32))
        assert tab["e1"][j].tolist() == [f32(r), f32(f32(r) * f32(r)), 0] and not tab["e2"][j].any() and not tab["n"][j].any()
        assert tab["area"][j] == f32(4 * math.pi * r * r)
    w = [4 * math.pi * r * r * sum(le) for _, r, le in sl.BULBS]
    assert tab["cdf"].tolist() == [f32(w[0] / (w[0] + w[1])), 1.0]
    assert tab["scale"].tolist() == [f32(2 * (w[0] + w[1]) / w[0]), f32(2 * (w[0] + w[1]) / w[1])]
    assert len(sl.table_of(rec, sl.FLAT)) == 0 and dl.same_table(sl.table_of(rec, sl.FLAT), dl.table_of(rec))


def test_restated_table_keeps_flat_records_first_and_rejects_what_it_must():
    rec = _scene(sl.with_kinds(sl.shared_material_world))
    tab, flat = sl.table_of(rec), dl.table_of(rec)
    assert tab["kind"].tolist() == [0, 2, 2] and tab["entry"].tolist() == [1, 2, 5] and len(flat) == 1
    for k in ("p0", "e1", "e2", "n", "emission", "area", "kind", "entry", "element", "material"):
        assert np.array_equal(bits(tab[k][:1]), bits(flat[k]))
    assert tab["material"][0] == tab["material"][1] != tab["material"][2]
    assert tab["cdf"][-1] == 1 and (np.diff(tab["cdf"]) > 0).all()
    # P_j = w_j / W: a flat record's scale is area / (P_j pi), a sphere's 2 / P_j
    P = np.diff(np.concatenate([[0], tab["cdf"].astype(np.float64)]))
    assert np.allclose(tab["scale"][0], 4.0 / (P[0] * math.pi), rtol=1e-5) and np.allclose(tab["scale"][1:], 2 / P[1:], rtol=1e-5)
    rec = _scene(sl.with_kinds(sl.rejected_spheres_world))
    tab = sl.table_of(rec)
    assert len(tab) == 1 and tab["kind"][0] == 2 and tab["entry"][0] == len(rec.entries()) - 1 and tab["scale"][0] == 2
    rec = _scene(sl.with_kinds(dl.odd_lights_world))
    tab = sl.table_of(rec)
    assert tab["kind"].tolist() == [1, 2] and tab["entry"].tolist() == [6, 0]  # the lone triangle first, then the sphere


# ------------------------------------------------------------------ the restatement against closed forms
def _cases(n=600, seed=3):
    """Random (vertex, sphere, draws): dc / R from 1.001 to 1e4 (log-uniform), axes of every direction with wz of both
    signs, and -- the first rows -- wz = +1 and wz = -1 exactly."""
    rng = np.random.default_rng(seed)
    R = rng.uniform(0.05, 3, n)
    ratio = np.exp(rng.uniform(math.log(1.001), math.log(1e4), n))
    ratio[:8] = [1.001, 1.001, 1e4, 1e4, 1.5, 1.5, 30, 30]
    axis = rng.normal(size=(n, 3))
    axis /= np.linalg.norm(axis, axis=1, keepdims=True)
    axis[:8] = [(0, 0, 1), (0, 0, -1)] * 4
    x = rng.uniform(-2, 2, (n, 3))
    x[:8] = 0  # (so that wc is the axis times dc exactly)
    R[:8] = 0.5
    c = x + axis * (ratio * R)[:, None]
    R = R.astype(f32)
    N = axis + 0.4 * rng.normal(size=(n, 3))
    N /= np.linalg.norm(N, axis=1, keepdims=True)
    st = rng.integers(0, 1 << 32, (n, 6), dtype=np.uint64).astype(np.uint32)
    return c.astype(f32), R, (R * R).astype(f32), x.astype(f32), N.astype(f32), st, ratio


def test_the_cone_frame_direction_and_distance_hold_their_closed_forms():
    c0, R0, _, x, N, st, ratio = _cases()
    n = len(c0)
    # the spheres as the table of an opted-in scene holds them: centre, R and R2 are the records' words
    _, tab, _ = _lit([(c0[i], float(R0[i]), (1, 1, 1)) for i in range(n)])
    assert len(tab) == n and (tab["kind"] == 2).all() and tab["entry"].tolist() == list(range(1, n + 1))
    c, R, R2 = tab["p0"].copy(), tab["e1"][:, 0].copy(), tab["e1"][:, 1].copy()
    assert np.array_equal(c, c0) and np.array_equal(R, R0) and np.array_equal(R2, (R0 * R0).astype(f32))
    idx = np.arange(n)
    r1 = dl.draw01(st, idx)
    cp, sp, _ = sl.disc_draws(st, idx)
    o = sl.sample_sphere(c, R2, x, N, r1, cp, sp)
    c64, x64, R264 = c.astype(np.float64), x.astype(np.float64), R2.astype(np.float64)
    wc = c64 - x64
    d2 = (wc * wc).sum(1)
    assert o["outside"].all() and (ratio.min() < 1.01) and (ratio.max() > 9e3)
    # d2c itself against |c - x|^2 in binary64: three roundings a term (the difference, the square, its sum) and no
    # cancellation among the positive terms, so at most (1 + 2^-24)^5 - 1 relative
    rel = np.abs(o["d2c"].astype(np.float64) - d2) / d2
    print("d2c: worst relative error %.3g (bound %.3g)" % (rel.max(), 5.5 * 2.0 ** -24))
    assert (rel <= 5.5 * 2.0 ** -24).all()
    # om against 1 - sqrt(1 - R2 / d2c), formed without cancellation in binary64 from the R2 and d2c the step holds: 4 ulp
    # of the binary32 result (d2c's own rounding, bounded above, is the vertex's and not om's: close to the surface it
    # alone moves the cone's opening by tens of ulp, whatever the expression)
    s2 = R264 / o["d2c"].astype(np.float64)
    om = s2 / (1 + np.sqrt(1 - s2))
    err = np.abs(o["om"].astype(np.float64) - om) / np.spacing(o["om"]).astype(np.float64)
    print("om: worst %.2f ulp, at dc / R = %.4f" % (err.max(), ratio[err.argmax()]))
    assert (err <= 4).all()
    s2 = R264 / d2
    # the frame is orthonormal, wz = +-1 included
    w, u, v = (o[k].astype(np.float64) for k in "wuv")
    assert (w[:8, 2] == [1, -1] * 4).all() and (w[:, 2] < 0).sum() > n // 4 and (w[:, 2] > 0).sum() > n // 4
    for a, b, want in ((u, u, 1), (v, v, 1), (w, w, 1), (u, v, 0), (u, w, 0), (v, w, 0)):
        assert np.abs((a * b).sum(1) - want).max() <= 1e-6
    # the direction is a unit vector inside the cone (cos to the axis >= cos theta_max, to rounding)
    wi = o["wi"].astype(np.float64)
    assert np.abs((wi * wi).sum(1) - 1).max() <= 1e-5
    cos_axis = (wi * wc).sum(1) / np.sqrt(d2)
    assert (cos_axis >= np.sqrt(1 - s2) - 1e-6).all() and (cos_axis <= 1 + 1e-6).all()
    # the point x + t wi lies on the sphere wherever the ray does not graze it
    far = o["q"].astype(np.float64) > 1e-3 * R264
    assert far.sum() > n // 2
    p = x64 + o["t"].astype(np.float64)[:, None] * wi
    dist = np.sqrt(((p - c64) ** 2).sum(1))
    tol = 1e-4 * (np.sqrt(d2) + R.astype(np.float64))
    assert (np.abs(dist - R.astype(np.float64))[far] <= tol[far]).all()
    assert (o["t"][far] > 0).all() and (o["t"].astype(np.float64)[far] <= np.sqrt(d2)[far]).all()  # the NEAR intersection


TWO_BULBS = [((1.5, 3, 0.5), 1.0, (1, 1, 1)), ((-2, 1.5, -1), 0.3, (1, 1, 1))]  # (emission 1: d_direct is albedo * g)


def _vertices(n, seed, D=None):
    """n Lambertian vertices (material 0) on the plane y = 0 under TWO_BULBS, normals around +y, attenuation and emitted 1,
    stepped by step 0, with light states of their own: a mislib.PathState."""
    rng = np.random.default_rng(seed)
    O = np.stack([rng.uniform(-3, 3, n), np.zeros(n), rng.uniform(-3, 3, n)], axis=1).astype(f32)
    Nv = np.array([0, 1, 0]) + 0.3 * rng.normal(size=(n, 3))
    Nv = (Nv / np.linalg.norm(Nv, axis=1, keepdims=True)).astype(f32)
    H = np.zeros((n, 12), np.int32)
    H[:, 3:6] = Nv.view(np.int32)
    H[:, 6], H[:, 7] = 0, rtmi.RTMI_HIT_PARALLELOGRAM
    st = rng.integers(0, 1 << 32, (n, 6), dtype=np.uint64).astype(np.uint32)
    one = np.ones((n, 3), f32)
    return ml.PathState(O, one if D is None else D, H, np.ones(n, np.uint32), one, one, st)


def test_the_rejection_loop_consumes_the_draws_it_should():
    """Through the restated step on the table of an opted-in scene (two bulbs and a flat lamp): a vertex that picks a
    sphere advances its light state by 2 + 2 x trips draws, one that picks the flat lamp by three, and a replay of the draws
    one by one ends in the same state with the same azimuth."""
    _, tab, kinds = _lit(TWO_BULBS, flat=True)
    assert tab["kind"].tolist() == [0, 2, 2]
    n = 4000
    ps = _vertices(n, 8)
    ps.steps[1::2] = 5  # every other path is not stepped: it keeps every word
    before = ps.LS.copy()
    out = sl.step(tab, kinds, ps.copy(), 0, 1, mis=False)
    assert np.array_equal(out.LS[1::2], before[1::2]) and int(out.counts[0]) == 3 + n // 2
    idx = np.arange(0, n, 2)
    replay = before.copy()
    j = np.searchsorted(tab["cdf"], dl.draw01(replay, idx), side="left")
    sph = tab["kind"][j] == 2
    assert sph.sum() > n // 8 and (~sph).sum() > n // 8
    adv = ((out.LS[idx, 0] - before[idx, 0]).astype(np.uint32) // np.uint32(362437)).astype(np.int64)  # d += 362437 a draw
    assert (adv[~sph] == 3).all()
    dl.draw01(replay, idx)  # r1
    after_r1 = replay.copy()
    cp, sp, trips = sl.disc_draws(replay, idx[sph])
    assert np.array_equal(adv[sph], 2 + 2 * trips) and np.array_equal(replay[idx[sph]], out.LS[idx[sph]])
    for k, i in enumerate(idx[sph][:300]):  # pair by pair from a copy, stopping at the first pair inside the disc
        s1 = after_r1.copy()
        for t in range(1, 100):
            a, b = sl.draw11(s1, np.array([i])), sl.draw11(s1, np.array([i]))
            s = f32(f32(a[0] * a[0]) + f32(b[0] * b[0]))
            if s > 0 and s <= 1:
                break
        assert trips[k] == t and np.array_equal(s1[i], out.LS[i])
        assert cp[k] == f32(a[0] / np.sqrt(s)) and sp[k] == f32(b[0] / np.sqrt(s))
    assert trips.min() == 1 and trips.max() > 1 and abs(trips.mean() - 4 / math.pi) < 0.06
    assert np.abs(cp.astype(np.float64) ** 2 + sp.astype(np.float64) ** 2 - 1).max() < 1e-6
    # the azimuth is uniform: the four quadrants take a quarter each
    quad = np.array([((cp > 0) & (sp > 0)).mean(), ((cp < 0) & (sp > 0)).mean(), ((cp < 0) & (sp < 0)).mean(), ((cp > 0) & (sp < 0)).mean()])
    assert np.abs(quad - 0.25).max() < 5 * math.sqrt(0.25 * 0.75 / len(cp))


def test_the_weights_close():
    """The a that SAMPLE forms and the a that WEIGH forms from the carry are the same word when cs == carry.w, through the
    restated steps on the table of an opted-in scene.  With attenuation and emission 1 the plain SAMPLE's d_direct IS its
    a = (cs * om) * scale.  The same vertices then scatter exactly along the sampled direction wi: the MIS SAMPLE leaves
    (wi, N . wi) = (wi, cs) in the carry, the path hits the bulb it sampled, and WEIGH's factor on an emission of 1 must be
    a / (a + 1) of SAMPLE's a, bit for bit; the light sample's weight 1 / (a + 1) closes the sum."""
    _, tab, kinds = _lit(TWO_BULBS)
    assert tab["kind"].tolist() == [2, 2] and (tab["emission"] == 1).all()
    n = 2000
    ps = _vertices(n, 11)
    sampled = sl.step(tab, kinds, ps.copy(), 0, 1, mis=False)
    valid = sampled.ST > 0
    assert valid.sum() > n // 2
    a_sample = sampled.DR[:, 0]  # (1 * 1) * g, g = a
    assert np.array_equal(bits(sampled.DR[:, 1]), bits(a_sample)) and (a_sample[valid] > 0).all()
    replay = ps.LS.copy()
    j = np.searchsorted(tab["cdf"], dl.draw01(replay, np.arange(n)), side="left")
    # the same draws again, now scattering along wi: the carry gets cs
    again = _vertices(n, 11, D=np.where(valid[:, None], sampled.SD, 1).astype(f32))
    mis = sl.step(tab, kinds, again, 0, 1, mis=True)
    assert np.array_equal(bits(mis.SD), bits(sampled.SD)) and np.array_equal(mis.LS, sampled.LS)
    g = mis.DR[:, 0]
    assert np.array_equal(bits(g[valid]), bits((a_sample / (a_sample + f32(1))).astype(f32)[valid]))  # SAMPLE's MIS term
    # one step on: the path ended on the bulb it sampled; d_origins stayed at the vertex
    nxt = mis.copy()
    nxt.steps[:] = 2
    nxt.D[:] = 0
    nxt.H[:, 7], nxt.H[:, 8] = rtmi.RTMI_HIT_SPHERE, tab["entry"][j]
    nxt.E[:] = 1
    weighed = sl.step(tab, kinds, nxt.copy(), 1, 0, mis=True)
    w, div = sl.sphere_weight(a_sample)
    assert div[valid].all() and np.array_equal(bits(weighed.E[valid, 0]), bits(w[valid]))
    assert np.array_equal(bits(weighed.E[valid, 0]), bits(g[valid]))  # a / (a + 1) on both sides
    light = (f32(1) / (a_sample + f32(1))).astype(f32)
    assert np.abs(w[valid].astype(np.float64) + light[valid].astype(np.float64) - 1).max() < 2e-7
    # a vertex whose sample was invalid (the bulb below its horizon) still weighs what it finds, with its own N . d
    assert int(weighed.counts[1]) - 5 == n and (weighed.E[~valid] <= 1).all()
    dropped = sl.step(tab, kinds, nxt.copy(), 1, 0, mis=False)
    assert not dropped.E.any() and np.array_equal(bits(dropped.C), bits(nxt.C))


def test_a_vertex_inside_or_on_the_sphere_samples_nothing_and_keeps_what_it_hits():
    _, tab, kinds = _lit([((0, 0, 0), 2.0, (1, 1, 1))])
    assert len(tab) == 1 and tab["e1"][0].tolist() == [2, 4, 0] and tab["entry"][0] == 1 and tab["scale"][0] == 2
    O = np.array([(0, 0, 0), (1, 0.5, 0), (2, 0, 0), (0, 0, -2), (0, 1.9999, 0)], f32)  # centre, inside, on, on, inside
    m = len(O)
    H = np.zeros((m, 12), np.int32)
    H[:, 3:6] = np.array([(0, 1, 0)] * m, f32).view(np.int32)
    H[:, 6], H[:, 7], H[:, 8] = 0, rtmi.RTMI_HIT_SPHERE, 1
    E = np.full((m, 3), 7, f32)
    st = np.random.default_rng(2).integers(0, 1 << 32, (m, 6), dtype=np.uint64).astype(np.uint32)
    ps = ml.PathState(O, np.ones((m, 3), f32), H, np.ones(m, np.uint32), E, E, st, flags=np.ones(m, np.uint32))
    for mis in (False, True):
        out = sl.step(tab, kinds, ps.copy(), 0, 1, mis=mis)
        assert (out.E == 7).all() and int(out.counts[1]) == 5  # kept, not counted
        assert (out.SD == 0).all() and (out.DR == 0).all() and (out.ST == 0).all() and (out.flags == 1).all()
        assert int(out.counts[0]) == 3 + m and not np.array_equal(out.LS, ps.LS)  # sampled (invalid), the draws taken
    outside = ps.copy()
    outside.O[:] = (0, 3, 0)
    for mis in (False, True):
        out = sl.step(tab, kinds, outside.copy(), 0, 0, mis=mis)
        assert (out.E != 7).all() and int(out.counts[1]) == 5 + m  # the same hits from outside are weighed or dropped


# ------------------------------------------------------------------ the estimator integrates
def test_the_estimator_integrates_to_the_irradiance_of_the_spheres():
    """A Lambertian point under two sphere lights and beside a flat one, the restated table's cdf and scale, 2^18 restated
    samples of the plain step: the mean of the direct term over the paths that picked a sphere must be
    albedo * Le * (R / d)^2 * cos(theta) per sphere (its irradiance pi Le (R / d)^2 cos(theta), fully above the horizon,
    times albedo / pi) within 5 standard errors per channel."""
    def fill(b):
        b.light_kinds(spheres=True)
        b.camera_pinhole(sl.v3(0, 1, 6), sl.v3(0, 0, 0), sl.v3(0, 1, 0), 0.9, 1.0)
        b.parallelogram([sl.v3(-4, 0, -4), sl.v3(4, 0, -4), sl.v3(-4, 0, 4)], b.lambertian(sl.v3(0.5, 0.5, 0.5)))
        b.parallelogram([sl.v3(-1, 6, -1), sl.v3(1, 6, -1), sl.v3(-1, 6, 1)], b.diffuse_light(b.constant_texture(sl.v3(1, 1, 1))))
        b.sphere(sl.v3(1.5, 3, 0.5), 1.0, b.diffuse_light(b.constant_texture(sl.v3(4, 2, 1))))
        b.sphere(sl.v3(-2, 1.5, -1), 0.3, b.diffuse_light(b.constant_texture(sl.v3(1, 5, 9))))
    rec = _scene(fill)
    tab = sl.table_of(rec)
    assert tab["kind"].tolist() == [0, 2, 2]
    n = 1 << 18
    x, Nv, albedo = np.array([0.25, 0, 0.5], f32), np.array([0, 1, 0], f32), np.array([0.5, 0.7, 0.9], f32)
    H = np.zeros((n, 12), np.int32)
    H[:, 3:6] = Nv.view(np.int32)
    H[:, 6], H[:, 7] = 0, rtmi.RTMI_HIT_PARALLELOGRAM
    st = np.random.default_rng(5).integers(0, 1 << 32, (n, 6), dtype=np.uint64).astype(np.uint32)
    ps = ml.PathState(np.tile(x, (n, 1)), np.tile(np.array([0, 1, 0], f32), (n, 1)), H, np.ones(n, np.uint32), np.zeros((n, 3), f32),
                      np.tile(albedo, (n, 1)), st)
    picked = np.searchsorted(tab["cdf"], dl.draw01(st.copy(), np.arange(n)), side="left")
    out = sl.step(tab, dl.mat_kinds_of(rec), ps, 0, 1, mis=False)
    assert int(out.counts[0]) == 3 + n
    for j in (1, 2):
        c, R, Le = tab["p0"][j].astype(np.float64), float(tab["e1"][j, 0]), tab["emission"][j].astype(np.float64)
        wc = c - x
        d = math.sqrt((wc * wc).sum())
        cos_t = wc[1] / d
        assert cos_t > R / d  # fully above the horizon
        want = albedo * Le * (R / d) ** 2 * cos_t
        Y = np.where((picked == j)[:, None], out.DR.astype(np.float64), 0)  # this light's share of the one-sample estimate
        mean, se = Y.mean(0), Y.std(0, ddof=1) / math.sqrt(n)
        print("light %d: mean %s  analytic %s  standard error %s" % (j, mean, want, se))
        assert (se > 0).all() and (np.abs(mean - want) <= 5 * se).all()
        assert (se <= 0.02 * want).all(), "the test is not sharp"
        on = picked == j
        assert (out.ST[on] > 0).all() and (np.abs(out.ST[on] / 0.999 - (d - R)) <= math.sqrt(d * d - R * R) - (d - R) + 1e-4).all()
