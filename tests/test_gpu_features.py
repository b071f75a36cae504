"""rtmi_render_features / rtmi_resolve_features / Renderer.render_budget(features=True) on the GPU, bit for bit against
the oracle replayed a sample at a time (tests/test_gpu_budget.py: OracleReplay).

The oracle side of the features needs nothing new in oracle/: the state BEFORE each sample of each pixel is known, two
``orc_random_float(0, 1)`` draws from a copy of it give the jitter, RenderPixel's binary64 formula (oracle.cc:704-707)
restated in Python floats gives the camera coordinates, ``probe_camera_ray`` the primary ray (it consumes the lens draws),
``probe_hit`` the record (t, u, v, normal, material; material -1 at t = 1e9 is Sky), and a recording proxy around the
builder the material's colour.  Emitters and Sky: the oracle's own ``render(.., spp=1, max_depth=1, pixel_ids=[p])`` from
a copy of the pre-sample state is exactly the emitted colour of the primary hit.  Everything is accumulated in numpy
binary32 in sample order and compared in row-major pixel space.

Two places where this file does not follow the issue to the letter, because the letter would test the wrong thing:
  - ``probe_hit`` builds ``Ray(o, d)``, which normalises d once more; ``probe_camera_ray``'s direction is already the
    render's.  Where that third normalisation is not the identity in binary32, the probe is handed a direction whose
    normalisation IS the render's direction (``preimage``) -- asserted, never skipped.
  - ``probe_scatter`` leaves the record's u, v at 0, so its attenuation is not the texel at the hit.  An image-textured
    Lambertian's colour is ImageTexture::Value restated in numpy (``image_value``: floor, compare, an integer index, one
    division) on ``probe_hit``'s u, v; the restatement is pinned to the oracle's own code on every image-textured EMITTER
    hit, where the oracle's render gives the value."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import common
import oraclelib
import rtmi
from rtmi import scenes
from abi_host import CHECK_LIB, ROOT
from budgetlib import ADAPTIVE, H, W, OracleReplay, Shards, assert_same_results, plan_rule, random_budget, resolve_rule
from parity import same
from querylib import glm_normalize
from texlib import image_value

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

F32 = np.float32
FEATURES = ("albedo", "normal", "depth", "coverage")
PI_D = scenes.PI_D


def v3(x, y, z):
    return np.array([x, y, z], dtype=F32)


# ------------------------------------------------------------------ the scenes
def textured(b, aspect):
    """Image textures with no libm in the way (parallelogram and mesh uvs are sums and products): a textured Lambertian
    wall, a textured emitter, a textured mesh with uvs, a constant Lambertian floor, Sky behind."""
    b.camera_pinhole(v3(0, 1, 6), v3(0, 1, 0), v3(0, 1, 0), PI_D / 4, aspect)
    rng = np.random.default_rng(8)
    img = rng.integers(0, 256, (8, 8, 4)).astype(np.uint8)
    tex = b.image_texture(img)
    wall = b.lambertian_tex(tex)
    lamp = b.diffuse_light(tex)
    b.sky()
    b.parallelogram([v3(-2.5, 0, -1), v3(0, 0, -1), v3(-2.5, 2, -1)], wall)
    b.parallelogram([v3(0.2, 1.2, -0.5), v3(2.2, 1.2, -0.5), v3(0.2, 2.4, -0.5)], lamp)
    b.parallelogram([v3(-3, 0, -2), v3(3, 0, -2), v3(-3, 0, 3)], b.lambertian(v3(0.6, 0.5, 0.4)))
    faces = np.array([[[0.2, 0.0, 0.5], [2.0, 0.0, 0.5], [0.2, 1.1, 0.0]],
                      [[2.0, 0.0, 0.5], [2.0, 1.1, 0.0], [0.2, 1.1, 0.0]]], dtype=F32)
    uvs = np.array([[0.0, 0.0, 1.0, 0.0, 0.0, 1.0], [1.0, 0.0, 1.0, 1.0, 0.0, 1.0]], dtype=F32)
    b.bvh(faces, wall, uvs=uvs, k_min=2048)


def build_named(name):
    return lambda b, aspect: common.build_scene(b, name, aspect)


BUILDERS = {"textured": textured}


def scene_builder(name):
    return BUILDERS.get(name) or build_named(name)


# ------------------------------------------------------------------ the GPU side
class FShards(Shards):
    """tests/test_gpu_budget.py's Shards with a scene program of this file's choosing and the feature buffers."""

    def __init__(self, name, depth, cap, world=1, h=H, w=W):
        self.name, self.h, self.w, self.world = name, h, w, world
        self.b = rtmi.SceneBuilder(common.scene_seed(name))
        scene_builder(name)(self.b, w / h)
        self.b.commit()
        self.R = [rtmi.Renderer(self.b, h, w, cap, depth, post=False, rank=r, world_size=world).init_rng()
                  for r in range(world)]
        self.pm = [rtmi.pixel_map(R.frame) for R in self.R]
        for R in self.R:
            R._budget_buffers()
            R._feature_buffers()

    def render_features(self, rowmajor, which=FEATURES, null_struct=False, lib=None):
        """rtmi_render_features through the C ABI with the buffers named in `which` (None: feat == NULL)."""
        L = lib or rtmi.lib()
        for R, bt in zip(self.R, self.scatter(rowmajor)):
            feat = rtmi.feature_bufs(**{k: getattr(R, k) for k in which})
            rc = L.rtmi_render_features(R.scene.h, C.byref(R.frame), C.c_void_p(bt.data_ptr()), C.c_void_p(R.states.data_ptr()),
                                        C.c_void_p(R.sum.data_ptr()), C.c_void_p(R.sq.data_ptr()),
                                        C.c_void_p(R.samples.data_ptr()), C.c_void_p(R.budget_rays.data_ptr()),
                                        None if null_struct else C.byref(feat), C.c_void_p(R.d_work.data_ptr()), R._stream())
            assert rc == 0, L.rtmi_last_error()
            R.budget_abandoned += R.d_work[0]
        for R in self.R:
            R.check()
            assert int(R.d_work[0].item()) == 0, "abandoned mesh searches"
        return self

    def render_budget(self, rowmajor, count_rays=True, features=False):
        for R, bt in zip(self.R, self.scatter(rowmajor)):
            R.render_budget(bt, count_rays=count_rays, features=features)
        for R in self.R:
            R.check()
            assert int(R.d_work[0].item()) == 0, "abandoned mesh searches"
        return self

    def features(self):
        return {k: self.gather(k) for k in FEATURES}

    def work(self):
        torch.cuda.synchronize()
        return [R.d_work[:2].cpu().numpy().copy() for R in self.R]


# ------------------------------------------------------------------ the oracle side
class Recorder:
    """A thin proxy around a builder: forwards every call, keeps the arguments of the material and texture constructors."""

    def __init__(self, b):
        self._b, self.mats, self.texs = b, {}, {}

    def __getattr__(self, k):
        return getattr(self._b, k)

    def constant_texture(self, rgb):
        t = self._b.constant_texture(rgb)
        self.texs[t] = ("constant", np.asarray(rgb, dtype=F32).copy())
        return t

    def image_texture(self, rgba):
        t = self._b.image_texture(rgba)
        self.texs[t] = ("image", np.ascontiguousarray(rgba, dtype=np.uint8).copy())
        return t

    def lambertian(self, rgb):
        m = self._b.lambertian(rgb)
        self.mats[m] = ("colour", np.asarray(rgb, dtype=F32).copy())
        return m

    def metal(self, rgb, fuzz):
        m = self._b.metal(rgb, fuzz)
        self.mats[m] = ("colour", np.asarray(rgb, dtype=F32).copy())
        return m

    def dielectric(self, rgb, index):
        m = self._b.dielectric(rgb, index)
        self.mats[m] = ("colour", np.asarray(rgb, dtype=F32).copy())
        return m

    def lambertian_tex(self, tex):
        m = self._b.lambertian_tex(tex)
        self.mats[m] = ("lambertian_tex", tex)
        return m

    def diffuse_light(self, tex):
        m = self._b.diffuse_light(tex)
        self.mats[m] = ("light", tex)
        return m


_SCALES = (F32(1) + np.arange(8192, dtype=F32) / F32(8192)).astype(F32)
_NUDGES = np.array([(a, b, c) for a in (0, 1, -1) for b in (0, 1, -1) for c in (0, 1, -1)], dtype=np.int32)


def preimage(d):
    """A direction whose glm::normalize is d, bit for bit: d itself wherever normalising a unit vector is the identity,
    else the first of d's neighbours (each component at most an ulp away) times a scale in [1, 2) that is mapped onto d."""
    d = np.ascontiguousarray(d, dtype=F32)
    if np.array_equal(glm_normalize(d).view(np.uint32), d.view(np.uint32)):
        return d
    for nudge in _NUDGES:
        near = (d.view(np.int32) + nudge).view(F32)  # (sign-magnitude: +-1 on the bits is +-1 ulp)
        cand = (near[None, :] * _SCALES[:, None]).astype(F32)
        ok = (glm_normalize(cand).view(np.uint32) == d.view(np.uint32)).all(axis=1)
        if ok.any():
            return cand[int(np.argmax(ok))].copy()
    raise AssertionError("no direction found that Ray's constructor maps onto %r" % (d,))


class FeatureReplay(OracleReplay):
    """OracleReplay that also accumulates the first-hit features of every sample it replays."""

    def __init__(self, name, depth, h=H, w=W):
        self.h, self.w, self.depth = h, w, depth
        seed = common.scene_seed(name)
        self.ob = Recorder(oraclelib.OracleBuilder(seed))
        scene_builder(name)(self.ob, w / h)
        n = h * w
        self.states = oraclelib.rng_init(seed, n)
        self.states[0] = self.ob.state0
        self.sum, self.sq = np.zeros((n, 3), F32), np.zeros((n, 3), F32)
        self.samples, self.rays = np.zeros(n, np.uint32), np.zeros(n, np.uint32)
        self.albedo, self.normal = np.zeros((n, 3), F32), np.zeros((n, 3), F32)
        self.depth_sum, self.coverage = np.zeros(n, F32), np.zeros(n, np.uint32)
        self.kinds = {"none": 0, "sky": 0, "colour": 0, "texel": 0, "light": 0, "image_light": 0}
        self.primary_rays = {}  # (first sample only) pixel -> (origin, direction handed to the probe)

    def emitted(self, p):
        rgb, _, _, _ = self.ob.render(self.h, self.w, 1, 1, post=False, pixel_ids=[p], states=self.states.copy(), threads=1)
        return rgb.reshape(-1, 3)[p].copy()

    def sample_features(self, p):
        L = oraclelib.lib()
        st = self.states[p].copy()
        ptr = st.ctypes.data_as(C.POINTER(C.c_uint32))
        r1 = float(L.orc_random_float(C.c_float(0.0), C.c_float(1.0), ptr))
        r2 = float(L.orc_random_float(C.c_float(0.0), C.c_float(1.0), ptr))
        i, j = divmod(int(p), self.w)
        x = (r1 + float(j)) / float(self.w)  # oracle.cc:704-707, in binary64
        y = (r2 + float(self.h - i)) / float(self.h)
        x, y = 2 * x - 1, 2 * y - 1
        ray = self.ob.probe_camera_ray(x, y, st)
        o, d = ray[:3].copy(), preimage(ray[3:])
        if self.samples[p] == 0:
            self.primary_rays[int(p)] = (o, d)
        hit, rec, mat = self.ob.probe_hit(o, d)
        if not hit:
            self.kinds["none"] += 1
            return
        if mat < 0:  # Sky: its colour, nothing else
            assert rec[0] == 1e9
            self.kinds["sky"] += 1
            self.albedo[p] = self.albedo[p] + self.emitted(p)
            return
        kind, arg = self.ob.mats[mat]
        if kind == "colour":
            alb = arg
            self.kinds["colour"] += 1
        else:
            tkind, targ = self.ob.texs[arg]
            if kind == "light":
                alb = self.emitted(p)
                self.kinds["image_light" if tkind == "image" else "light"] += 1
                want = image_value(targ, rec[1], rec[2]) if tkind == "image" else targ
                assert same(alb, want), "the restated texture value differs from the oracle's own Emit"
            else:
                alb = image_value(targ, rec[1], rec[2]) if tkind == "image" else targ
                self.kinds["texel" if tkind == "image" else "colour"] += 1
        self.coverage[p] += 1
        self.depth_sum[p] = self.depth_sum[p] + F32(rec[0])
        self.normal[p] = self.normal[p] + rec[3:6].astype(F32)
        self.albedo[p] = self.albedo[p] + np.asarray(alb, dtype=F32)

    def add(self, budget):
        budget = np.asarray(budget).reshape(-1).astype(np.int64)
        for k in range(int(budget.max()) if budget.size else 0):
            ids = np.nonzero(budget > k)[0].astype(np.int32)
            for p in ids:  # from the states BEFORE this sample
                self.sample_features(p)
            rgb, rays, self.states, _ = self.ob.render(self.h, self.w, 1, self.depth, post=False, pixel_ids=ids,
                                                       states=self.states)
            x = rgb.reshape(-1, 3)[ids]
            self.sum[ids] = self.sum[ids] + x
            self.sq[ids] = self.sq[ids] + x * x
            self.samples[ids] += 1
            self.rays[ids] += rays.reshape(-1)[ids]
        for a in (self.sum, self.sq, self.albedo, self.normal, self.depth_sum):
            assert a.dtype == F32
        return self

    def features(self):
        return {"albedo": self.albedo, "normal": self.normal, "depth": self.depth_sum, "coverage": self.coverage}

    def assert_features_equal(self, got, what="", albedo_rel_l2=None):
        assert np.array_equal(got["coverage"].view(np.uint32), self.coverage), what + ": coverage"
        assert same(got["depth"], self.depth_sum), what + ": depth"
        assert same(got["normal"], self.normal), what + ": normal"
        if albedo_rel_l2 is None:
            assert same(got["albedo"], self.albedo), what + ": albedo"
        else:
            err = common.rel_l2(got["albedo"], self.albedo)
            print("%s: albedo rel L2 against the replay %.3g (bound %g)" % (what, err, albedo_rel_l2))
            assert err <= albedo_rel_l2, (what, err)


def check_features_match_the_replay(name, depth, world, lib=None):
    budget = random_budget(31 + len(name))
    assert (budget == 0).sum() > H * W // 10 and budget.max() == 9
    s = FShards(name, depth, 9, world).render_features(budget, lib=lib)
    o = FeatureReplay(name, depth).add(budget)
    o.assert_equal(s.results(), name)
    o.assert_features_equal(s.features(), name)
    return o


# ------------------------------------------------------------------ 1. features against the oracle replay
@pytest.mark.parametrize("world", [1, 3])
@pytest.mark.parametrize("name,depth", [("cornell_box", 50), ("spheres", 10), ("bunny", 10), ("mixed", 10), ("sky_only", 10)])
def test_features_match_the_oracle_replay(name, depth, world):
    o = check_features_match_the_replay(name, depth, world)
    print(name, o.kinds)
    if name == "sky_only":
        assert o.kinds["sky"] > 0 and not o.coverage.any() and o.albedo.any()
    else:
        assert o.kinds["colour"] > 0 and o.coverage.any()
    if name == "cornell_box":
        assert o.kinds["light"] > 0, "no primary ray met the light"


# ------------------------------------------------------------------ 2. image textures
def test_image_textures_exact_without_libm():
    o = check_features_match_the_replay("textured", 10, 1)
    print(o.kinds)
    for k in ("texel", "image_light", "colour", "sky"):
        assert o.kinds[k] > 20, (k, o.kinds)
    assert len(np.unique(o.albedo[o.coverage > 0], axis=0)) > 30, "the texels are not told apart"


def test_birthday_within_the_textured_sphere_tolerance():
    """The image-textured sphere's uv go through acosf / atan2f of two libms (1e-3): the albedo within
    that, coverage, depth and normal exact; the render outputs against rtmi_render_budget (the oracle's sums differ by
    the same texels)."""
    name, depth = "birthday", 10
    budget = random_budget(40)
    s = FShards(name, depth, 9).render_features(budget)
    o = FeatureReplay(name, depth).add(budget)
    assert o.kinds["texel"] > 20
    o.assert_features_equal(s.features(), name, albedo_rel_l2=1e-3)
    assert_same_results(s.results(), FShards(name, depth, 9).render_budget(budget).results(), name)
    got = s.results()
    assert np.array_equal(got["samples"].view(np.uint32), o.samples) and np.array_equal(got["states"].view(np.uint32), o.states)


# ------------------------------------------------------------------ 3. the features change nothing else
@pytest.mark.parametrize("name,depth", [("cornell_box", 50), ("bunny", 10), ("textured", 10)])
def test_features_change_nothing_else(name, depth):
    budget = random_budget(17)
    plain = FShards(name, depth, 9).render_budget(budget)
    want, want_work = plain.results(), plain.work()
    full = FShards(name, depth, 9).render_features(budget)
    full_features = full.features()
    assert_same_results(full.results(), want, name + ": all four")
    assert np.array_equal(full.work()[0], want_work[0])
    for k in FEATURES:
        one = FShards(name, depth, 9).render_features(budget, which=(k,))
        assert_same_results(one.results(), want, name + ": only " + k)
        assert np.array_equal(one.work()[0], want_work[0]), k
        got = one.features()
        assert same(got[k], full_features[k]), k
        for other in FEATURES:
            if other != k:
                assert not got[other].any(), (k, other)
    for kw in (dict(null_struct=True), dict(which=())):  # feat == NULL, all four null: rtmi_render_budget
        none = FShards(name, depth, 9).render_features(budget, **kw)
        assert_same_results(none.results(), want, name + ": no feature buffer")
        assert np.array_equal(none.work()[0], want_work[0])
        assert not any(v.any() for v in none.features().values())


# ------------------------------------------------------------------ 4. passes add up
@pytest.mark.parametrize("name,depth", [("cornell_box", 50), ("bunny", 10), ("spheres", 10)])
def test_two_feature_calls_equal_one(name, depth):
    b1, b2 = random_budget(11, hi=6), random_budget(12, hi=6)
    two = FShards(name, depth, 12).render_budget(b1, features=True).render_budget(b2, features=True)
    one = FShards(name, depth, 12).render_budget(b1 + b2, features=True)
    assert_same_results(two.results(), one.results(), name)
    assert_same_results(two.features(), one.features(), name)
    assert np.array_equal(one.features()["coverage"] <= (b1 + b2), np.ones(H * W, bool))


# ------------------------------------------------------------------ 5. what is left alone
@pytest.mark.parametrize("world", [1, 3])
def test_zero_budget_and_padding_items_keep_their_feature_words(world):
    name, depth = "cornell_box", 10
    budget = random_budget(3)
    s = FShards(name, depth, 9, world)
    for R in s.R:
        R.albedo.fill_(0.25), R.normal.fill_(-0.5), R.depth.fill_(3.0), R.coverage.fill_(7)
    for R, bt in zip(s.R, s.scatter(budget, pad=5)):
        R.render_budget(bt, features=True).check()
    for r, pm in enumerate(s.pm):
        b_item = np.zeros(pm.shape, np.int64)
        b_item[pm >= 0] = budget[pm[pm >= 0]]
        idle = (pm < 0) | (b_item == 0)
        assert (pm < 0).any() and ((pm >= 0) & (b_item == 0)).any()
        assert (s.raw("albedo")[r][idle] == F32(0.25)).all() and (s.raw("normal")[r][idle] == F32(-0.5)).all()
        assert (s.raw("depth")[r][idle] == F32(3.0)).all() and (s.raw("coverage")[r][idle] == 7).all()
    o = FeatureReplay(name, depth)
    o.albedo[:], o.normal[:], o.depth_sum[:], o.coverage[:] = 0.25, -0.5, 3.0, 7
    o.add(budget).assert_features_equal(s.features(), "from the sentinel")


# ------------------------------------------------------------------ 6. sample 0 does not depend on the depth
@pytest.mark.parametrize("name", ["spheres", "textured"])
def test_first_sample_features_do_not_depend_on_the_depth(name):
    """The camera's draws come before Trace's, so the first sample's primary ray is the same at every depth."""
    got = [FShards(name, depth, 1).render_budget(np.ones(H * W, np.int64), features=True).features() for depth in (1, 10, 50)]
    assert got[0]["coverage"].any()
    assert_same_results(got[0], got[1], name + ": depth 1 against 10")
    assert_same_results(got[0], got[2], name + ": depth 1 against 50")


# ------------------------------------------------------------------ 7. agreement with rtmi_intersect
@pytest.mark.parametrize("name,depth", [("bunny", 10), ("cornell_box", 10)])
def test_features_agree_with_intersect(name, depth):
    s = FShards(name, depth, 1).render_budget(np.ones(H * W, np.int64), features=True)
    o = FeatureReplay(name, depth).add(np.ones(H * W, np.int64))
    O = np.stack([o.primary_rays[p][0] for p in range(H * W)]).astype(F32)
    D = np.stack([o.primary_rays[p][1] for p in range(H * W)]).astype(F32)
    hits = s.b.intersect(torch.from_numpy(O).cuda(), torch.from_numpy(D).cuda()).check()
    kind, t, nrm = hits.kind.cpu().numpy(), hits.t.cpu().numpy(), hits.normal.cpu().numpy()
    solid = (kind != rtmi.RTMI_HIT_NONE) & (kind != rtmi.RTMI_HIT_SKY)
    got = s.features()
    assert solid.any() and np.array_equal(got["coverage"].view(np.uint32), solid.astype(np.uint32))
    assert same(got["depth"][solid], t[solid])
    # (+0) + x is x bit for bit except for x = -0, which the addition turns into +0: the zeroed buffer's one sample is
    # the hit's normal by VALUE, and bit for bit once -0 components are written as +0
    assert same(got["normal"][solid], np.ascontiguousarray(nrm[solid]) + F32(0))
    assert not got["depth"][~solid].any() and not got["normal"][~solid].any()


# ------------------------------------------------------------------ 8. resolve
def test_resolve_features_matches_the_numpy_rule():
    s = FShards("mixed", 10, 9, world=3).render_budget(random_budget(5), features=True)
    seen_n0 = seen_c0 = False
    parts = []
    for R, pm in zip(s.R, s.pm):
        out = R.resolve_features()
        n, c = R.samples.cpu().numpy().view(np.uint32), R.coverage.cpu().numpy().view(np.uint32)
        want = resolve_rule(n, R.albedo.cpu().numpy(), R.normal.cpu().numpy(), R.depth.cpu().numpy(), c, pixel=pm >= 0)
        for name, g, w_ in zip(out._fields, out, want):
            assert same(g.cpu().numpy(), w_), name
        seen_n0 |= bool(((pm >= 0) & (n == 0)).any())
        seen_c0 |= bool(((pm >= 0) & (n > 0) & (c == 0)).any())
        parts.append(out)
    assert seen_n0 and seen_c0, "the case needs pixels without samples and pixels whose samples all missed"
    # the 3-channel buffers through untile as they are, depth and alpha by their bits
    R = s.R[0]
    cat = lambda k: torch.cat([getattr(p, k) for p in parts], 0).contiguous()
    img, dep = R.untile(cat("albedo"), cat("depth"))
    nrm, alpha = R.untile(cat("normal"), cat("alpha"))
    torch.cuda.synchronize()
    assert dep.dtype == torch.float32 and alpha.dtype == torch.float32
    rm = {k: np.zeros((H * W,) + tuple(getattr(parts[0], k).shape[1:]), F32) for k in parts[0]._fields}
    for p, pm in zip(parts, s.pm):
        for k in rm:
            rm[k][pm[pm >= 0]] = getattr(p, k).cpu().numpy()[pm >= 0]
    assert same(img.cpu().numpy().reshape(-1, 3), rm["albedo"]) and same(nrm.cpu().numpy().reshape(-1, 3), rm["normal"])
    assert same(dep.cpu().numpy().reshape(-1), rm["depth"]) and same(alpha.cpu().numpy().reshape(-1), rm["alpha"])


# ------------------------------------------------------------------ 9. adaptive
def test_render_adaptive_carries_the_features():
    name, depth = "cornell_box", 10
    plain = FShards(name, depth, 64)
    res0 = plain.R[0].render_adaptive(**ADAPTIVE)
    assert res0.features is None
    s = FShards(name, depth, 64)
    res = s.R[0].render_adaptive(features=True, **ADAPTIVE)
    assert (res.passes, res.total_samples) == (res0.passes, res0.total_samples)
    assert same(res.tiles.cpu().numpy(), res0.tiles.cpu().numpy()) and same(res.samples.cpu().numpy(), res0.samples.cpu().numpy())
    assert_same_results(s.results(), plain.results(), "adaptive with features")
    o = FeatureReplay(name, depth)
    while True:
        budget = plan_rule(o.samples, o.sum, o.sq, ADAPTIVE["min_spp"], ADAPTIVE["max_spp"], ADAPTIVE["step"],
                           ADAPTIVE["tolerance"], ADAPTIVE["floor"])
        if not budget.any():
            break
        o.add(budget)
    o.assert_equal(s.results(), name)
    o.assert_features_equal(s.features(), name)
    pm = s.pm[0]
    want = resolve_rule(o.samples, o.albedo, o.normal, o.depth_sum, o.coverage)
    for k, w_ in zip(res.features._fields, want):
        assert same(getattr(res.features, k).cpu().numpy()[pm >= 0], w_[pm[pm >= 0]]), k


# ------------------------------------------------------------------ 10. shares no device state
def test_feature_call_runs_beside_a_render_on_the_same_scene():
    name, depth, spp = "bunny", 10, 16
    budget = random_budget(9, hi=16)
    alone = FShards(name, depth, spp).render_budget(budget, features=True)
    want, want_features = alone.results(), alone.features()
    R0 = rtmi.Renderer(alone.b, 64, 64, spp, depth, post=False).init_rng()
    R0.render().check()
    want_tiles, want_rays = R0.tiles.cpu().numpy(), R0.ray_counts.cpu().numpy()

    Rb, R1 = alone.R[0], rtmi.Renderer(alone.b, 64, 64, spp, depth, post=False).init_rng()
    bt = alone.scatter(budget)[0]
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    for _ in range(3):  # (three rounds on fresh buffers: the two calls overlap in at least some)
        Rb.init_rng(), R1.init_rng()
        for t in (Rb.sum, Rb.sq, Rb.samples, Rb.budget_rays, Rb.albedo, Rb.normal, Rb.depth, Rb.coverage):
            t.zero_()
        torch.cuda.synchronize()
        R1.render()
        with torch.cuda.stream(side):
            Rb.render_budget(bt, features=True)
        torch.cuda.synchronize()
        R1.check(), Rb.check()
        assert int(Rb.d_work[0].item()) == 0
        assert same(R1.tiles.cpu().numpy(), want_tiles) and same(R1.ray_counts.cpu().numpy(), want_rays)
        assert_same_results(alone.results(), want, "beside a render")
        assert_same_results(alone.features(), want_features, "beside a render")


# ------------------------------------------------------------------ 11. the check build
def test_check_build_matches_the_oracle_replay():
    """librtmi_check1.so compiles the feature kernels too (its margin re-query stays render-only): loaded in a process of
    its own, it passes the replay comparison on the Cornell box."""
    assert os.path.exists(CHECK_LIB), "librtmi_check1.so missing: __graft_entry__.build() builds it"
    env = dict(os.environ, RTMI_LIB_PATH=CHECK_LIB)
    env["PYTHONPATH"] = os.pathsep.join([os.path.join(ROOT, "ray-tracing-cuda_amd"), os.path.join(ROOT, "tests")])
    r = subprocess.run([sys.executable, os.path.abspath(__file__)], env=env, cwd=ROOT, stdout=subprocess.PIPE,
                       stderr=subprocess.PIPE, text=True, timeout=600)
    assert r.returncode == 0 and "check build ok" in r.stdout, (r.stdout[-2000:], r.stderr[-4000:])


if __name__ == "__main__":
    assert rtmi.LIB_PATH == CHECK_LIB or "check1" in rtmi.LIB_PATH, rtmi.LIB_PATH
    check_features_match_the_replay("cornell_box", 50, 1)
    print("check build ok")
