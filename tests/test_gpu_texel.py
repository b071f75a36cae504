"""Image-texture lookups on the GPU, bit for bit: the ray families of tests/texlib.py (texel centres and boundaries, the
seam, the poles, the axes, and the same on parallelograms and a mesh) through rtmi_bounce, rtmi_intersect, rtmi_trace,
rtmi_render, rtmi_render_budget and rtmi_render_features.

Only acosf / atan2f of the sphere's u, v differ between the device's libm and the host's; everything after them is
deterministic.  So the sphere's u, v are held within SPHERE_UV_TOL of the oracle's and of a binary64 restatement
(texlib.sphere_uv_truth), and everything else -- the texel, byte / 255, the step's attenuation and emission, the fold, the
feature albedo -- to the oracle handed the DEVICE's own u, v (OracleBuilder.probe_scatter_ex takes them as arguments).  On
parallelograms and meshes no libm is involved and the oracle's own u, v are used.  tests/test_texlib_host.py shows on the
CPU that the families reach what they are for.

The largest |u - truth| and |v - truth| of the device over the 33,082 sphere rays of each world, and the rays per family
on which the device and the oracle read different texels, are printed by test 1 and recorded in its docstring and in
NOTES.md ("Image-textured spheres: what the 1e-6 holds")."""
import functools
import types

import numpy as np
import pytest

import oraclelib
import rtmi
import texlib
from bouncelib import dev, dev_states, host_states
from parity import bits
from querylib import SPHERE_UV_TOL, compare, glm_normalize, gpu_intersect
from texlib import F32, FAMILIES, LIGHT, family, image_value, sphere_uv_truth, texel_index, textures

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

NAMES = ("tex_spheres", "tex_all")
SPHERE = rtmi.RTMI_HIT_SPHERE


# ------------------------------------------------------------------ the worlds and one step of every ray
@functools.lru_cache(maxsize=None)
def world(name, aspect=1.0, pitched=False):
    b, rec, ob, lay, seed = texlib.build(name, aspect, texlib.pitched_upload(80) if pitched else None)
    return types.SimpleNamespace(b=b, rec=rec, ob=ob, lay=lay, seed=seed, images=texlib.material_image(lay))


@functools.lru_cache(maxsize=None)
def family_rays(name):
    """The families of a world, the oracle's records of them and the states they are stepped from."""
    r = texlib.rays(name)
    hit, out, mat = texlib.oracle_records(world(name).ob, r.O, r.D)
    assert hit.all()
    return r, out, mat, oraclelib.rng_init(world(name).seed + 1, len(r.O), first=4242)


def step(w, O, D, S):
    """One rtmi_bounce with hits on device copies, everything read back."""
    o, d, st = dev(O), dev(D), dev_states(S)
    r = w.b.bounce(o, d, st, hits=True).check()
    assert r.stepped() == len(O)
    return types.SimpleNamespace(O=o.cpu().numpy(), D=d.cpu().numpy(), S=host_states(st), E=r.emitted.cpu().numpy(),
                                 A=r.attenuation.cpu().numpy(), raw=r.hits.raw.cpu().numpy())


@functools.lru_cache(maxsize=None)
def stepped(name, pitched=False):
    r, out, mat, S = family_rays(name)
    return step(world(name, 1.0, pitched), r.O, r.D, S)


@functools.lru_cache(maxsize=None)
def intersected(name):
    r = texlib.rays(name)
    return gpu_intersect(world(name).b, r.O, r.D).raw.cpu().numpy()


def scatter_mismatch(w, s, i, O, D, S, rec, mat, u, v):
    """Step s of path i against Scatter and Emit of the oracle handed (u, v); None, or what differs."""
    state = S[i].copy()
    sc, o12 = w.ob.probe_scatter_ex(int(mat), O[i], D[i], rec[0], float(u), float(v), rec[3:6], state)
    if not np.array_equal(bits(s.E[i]), bits(o12[9:12])):
        return "emitted"
    if not np.array_equal(s.S[i], state):
        return "state"
    if sc:
        if not np.array_equal(bits(s.A[i]), bits(o12[0:3])):
            return "attenuation"
        if not np.array_equal(bits(s.O[i]), bits(o12[3:6])):
            return "origin"
        if not np.array_equal(bits(glm_normalize(s.D[i])), bits(o12[6:9])):
            return "direction"
    elif bits(s.A[i]).any() or bits(s.D[i]).any() or not np.array_equal(bits(s.O[i]), bits(O[i])):
        return "an ended path's outputs"
    return None


# ------------------------------------------------------------------ 1. the step, exact
@pytest.mark.parametrize("name", NAMES)
def test_the_step_is_the_oracles_with_the_devices_uv(name):
    """Every ray of every family, none excluded: the record as querylib.compare holds it (t, normal, material, kind and
    entry exact; a sphere's u, v within SPHERE_UV_TOL), the sphere's u, v within the same of the binary64 restatement, and
    attenuation, emission, scattered ray and state exactly the oracle's Scatter and Emit with the device's own u, v -- on
    `centres` with the oracle's u, v as well, half a texel (2.4e-4 at the least) being far more than 1e-6.

    MI355X, both worlds alike: max |u - truth| 1.19e-07 (edges, ray 506 on sphere 1), max |v - truth| 1.19e-07 (edges, ray
    1431 on sphere 3); rays on which device and oracle read different texels: centres 0 of 9,457 (asserted), edges 396
    of 20,295, seam 5 of 126, poles 0 of 3,168, axes 0 of 36 (printed, not bounded: they are why the oracle is handed
    the device's u, v)."""
    w, (r, out, mat, S), s = world(name), family_rays(name), stepped(name)
    assert compare(s.raw, w.ob, r.O, r.D, w.rec) == []
    f, kind = s.raw.view(F32), s.raw[:, 7]
    sphere = kind == SPHERE
    assert np.array_equal(sphere, r.family < len(texlib.SPHERE_FAMILIES))
    tu, tv = sphere_uv_truth(f[:, 3:6])
    du = np.where(sphere, np.abs(f[:, 1].astype(np.float64) - tu), 0)
    dv = np.where(sphere, np.abs(f[:, 2].astype(np.float64) - tv), 0)
    for what, dd in (("u", du), ("v", dv)):
        i = int(np.argmax(dd))
        print("%s device: max |%s - truth| = %.3g at %s ray %d (sphere %d), normal %r" %
              (name, what, dd[i], FAMILIES[r.family[i]], i, r.target[i], f[i, 3:6].tolist()))
    assert du.max() <= SPHERE_UV_TOL and dv.max() <= SPHERE_UV_TOL
    centres = r.family == FAMILIES.index("centres")
    bad, other_texel = [], dict.fromkeys(texlib.SPHERE_FAMILIES, 0)
    for i in range(len(r.O)):
        u, v = (f[i, 1], f[i, 2]) if sphere[i] else out[i, 1:3]
        what = scatter_mismatch(w, s, i, r.O, r.D, S, out[i], mat[i], u, v)
        if what is None and centres[i]:
            what = scatter_mismatch(w, s, i, r.O, r.D, S, out[i], mat[i], out[i, 1], out[i, 2])
            what = what and what + " (the oracle's own u, v)"
        if what is not None:
            bad.append((i, FAMILIES[r.family[i]], int(r.target[i]), what, r.O[i].tolist(), r.D[i].tolist(), s.raw[i].tolist()))
        if sphere[i]:
            h, wd = w.images[mat[i]].shape[:2]
            other_texel[FAMILIES[r.family[i]]] += texel_index(h, wd, f[i, 1], f[i, 2]) != texel_index(h, wd, out[i, 1], out[i, 2])
    print(name, "rays on which the device and the oracle read different texels:",
          {k: "%d of %d" % (n, len(family(r, k))) for k, n in other_texel.items()})
    assert bad == [], (len(bad), bad[:6])
    assert other_texel["centres"] == 0


# ------------------------------------------------------------------ 2. the two copies of the sphere's formula
@pytest.mark.parametrize("name", NAMES)
def test_intersect_and_the_step_record_the_same_bits(name):
    """The step's record is rtmi_intersect's, u and v of the signed-zero seam and pole rays included.

    This does NOT compare the two restatements of sphere.cu:60-63: rtmi_bounce writes its record through resolve_hit
    (query_body.h), the function rtmi_intersect runs, while the u, v of render_body.h go nowhere but into tex_fetch.  The
    two are compared where the second one shows, in the texel: test 1 holds the step's attenuation -- fetched at
    render_body.h's u, v -- to Value at the record's u, v, on 20,295 rays that straddle every texel boundary by ulps.
    A render_body.h that multiplies by 1 / (2 pi) where query_body.h divides fails it; one that writes 0.f - nrm.z for
    -nrm.z passes everything, and must: it turns u = 0 into u = 1.0 and nothing else, and the wrap reads column 0 for
    both (NOTES.md, "Image-textured spheres")."""
    q, s = intersected(name), stepped(name)
    differ = np.flatnonzero((q[:, 1:3] != s.raw[:, 1:3]).any(1))
    r = texlib.rays(name)
    assert differ.size == 0, (differ.size, [(int(i), FAMILIES[r.family[i]], q[i, :10].tolist(), s.raw[i, :10].tolist()) for i in differ[:6]])
    assert np.array_equal(q[:, :10], s.raw[:, :10])


# ------------------------------------------------------------------ 3. surfaces with no libm in the way
def test_flat_surfaces_exact_end_to_end():
    """Parallelograms and mesh faces: the whole record (compare, in test 1) and the step with the ORACLE's u, v -- at
    v = 0 (row 0), v = 2^-24 (the last row), u = 1.0 (column 0) and every boundary of every shape; here also against the
    restated Value directly."""
    w, (r, out, mat, S), s = world("tex_all"), family_rays("tex_all"), stepped("tex_all")
    flat = np.flatnonzero(r.family >= len(texlib.SPHERE_FAMILIES))
    f = s.raw.view(F32)
    assert len(flat) > 10000 and np.array_equal(bits(f[flat, 1:3]), bits(out[flat, 1:3]))
    rows_seen = set()
    for i in flat:
        img = w.images[mat[i]]
        texel = image_value(img, out[i, 1], out[i, 2])
        light = mat[i] == w.lay.mats[LIGHT]
        assert np.array_equal(bits(s.E[i] if light else s.A[i]), bits(texel)), (i, r.O[i].tolist())
        assert not (s.A[i] if light else s.E[i]).any()
        if out[i, 2] in (0.0, 2.0 ** -24):
            rows_seen.add((img.shape[0], float(out[i, 2]), texel_index(img.shape[0], img.shape[1], out[i, 1], out[i, 2])[0]))
    for img in textures():
        h = img.shape[0]
        assert (h, 0.0, 0) in rows_seen and (h, 2.0 ** -24, h - 1) in rows_seen, (h, sorted(rows_seen))


# ------------------------------------------------------------------ 4. trace and fold
def expected_depth2(w, O, D, S):
    """Trace at depth 2 of rays (O, D) from states S inside the white enclosure: the oracle's Hit, Scatter and Emit, a
    sphere's u, v taken from rtmi_intersect.  The second query's ray is the device step's (its direction normalised
    once, as Ray's constructor finds it), held to the oracle's Scatter here.  Returns radiance, queries, final states, the
    first hit's albedo, whether the path ended within the two queries, and the first hits' records."""
    n = len(O)
    q1 = gpu_intersect(w.b, O, D).raw.cpu().numpy()
    s1 = step(w, O, D, S)
    assert np.array_equal(q1[:, :10], s1.raw[:, :10])
    alive = (s1.D != 0).any(1)
    q2 = np.zeros_like(q1)
    if alive.any():
        q2[alive] = gpu_intersect(w.b, s1.O[alive], s1.D[alive]).raw.cpu().numpy()
    rgb, rays, fin = np.zeros((n, 3), F32), np.zeros(n, np.int32), S.copy()
    albedo, ended = np.zeros((n, 3), F32), np.zeros(n, bool)
    for i in range(n):
        hit, rec, mat = w.ob.probe_hit(O[i], D[i])
        assert hit and mat >= 0, i
        u, v = q1[i].view(F32)[1:3] if q1[i, 7] == SPHERE else rec[1:3]
        sc, o12 = w.ob.probe_scatter_ex(mat, O[i], D[i], rec[0], float(u), float(v), rec[3:6], fin[i])
        assert sc == bool(alive[i]), i
        albedo[i] = o12[0:3] if sc else o12[9:12]
        if not sc:
            rgb[i], rays[i], ended[i] = o12[9:12], 1, True
            continue
        assert np.array_equal(bits(s1.O[i]), bits(o12[3:6])) and np.array_equal(bits(glm_normalize(s1.D[i])), bits(o12[6:9])), i
        hit2, rec2, mat2 = w.ob.probe_hit(s1.O[i], s1.D[i])
        assert hit2 and mat2 >= 0, i
        u2, v2 = q2[i].view(F32)[1:3] if q2[i, 7] == SPHERE else rec2[1:3]
        sc2, p12 = w.ob.probe_scatter_ex(mat2, s1.O[i], s1.D[i], rec2[0], float(u2), float(v2), rec2[3:6], fin[i])
        ended[i] = not sc2
        rgb[i] = (o12[9:12] + (o12[0:3] * p12[9:12]).astype(F32)).astype(F32)  # ray_tracing.cu:50-52: E1 + A1 * (E2 + A2 * 0)
        rays[i] = 3 if sc2 else 2  # (a path that is alive at the depth limit has made the query that finds it there)
    return types.SimpleNamespace(rgb=rgb, rays=rays, states=fin, albedo=albedo, ended=ended, q1=q1, q2=q2)


def trace(w, O, D, S, depth):
    st = dev_states(S)
    t = w.b.trace(dev(O), dev(D), st, depth, count_rays=True).check()
    return t.rgb.cpu().numpy(), t.rays.cpu().numpy(), host_states(st)


@functools.lru_cache(maxsize=None)
def traced(name, pitched=False):
    r, out, mat, S = family_rays(name)
    return trace(world(name, 1.0, pitched), r.O, r.D, S, 2)


@pytest.mark.parametrize("name", NAMES)
def test_trace_returns_the_texel(name):
    """Inside the white enclosure a depth-2 path from a textured Lambertian returns 0 + texel * (1, 1, 1), a path onto
    the textured light its texel after one query: rtmi_trace equals Value at rtmi_intersect's u, v bit for bit, queries
    and final states are the oracle's, and a deeper stack of layers (depth 10) folds to the same radiance wherever the
    path has ended by then."""
    w, (r, out, mat, S) = world(name), family_rays(name)
    want = expected_depth2(w, r.O, r.D, S)
    rgb, rays, fin = traced(name)
    bad = np.flatnonzero((bits(rgb) != bits(want.rgb)).any(1) | (rays != want.rays) | (fin != want.states).any(1))
    assert bad.size == 0, (bad.size, [(int(i), FAMILIES[r.family[i]], rgb[i].tolist(), want.rgb[i].tolist(), int(rays[i]),
                                       int(want.rays[i])) for i in bad[:6]])
    # the statement itself, wherever the scattered ray reaches the enclosure (nearly everywhere: the spheres are far apart)
    sphere = np.flatnonzero(r.family < len(texlib.SPHERE_FAMILIES))
    f = want.q1.view(F32)
    open_sky = 0
    for i in sphere:
        light = mat[i] == w.lay.mats[LIGHT]
        if light or want.q2[i, 6] == w.lay.white:
            open_sky += 1
            assert np.array_equal(bits(rgb[i]), bits(image_value(w.images[mat[i]], f[i, 1], f[i, 2]))), i
            assert rays[i] == (1 if light else 2)
    assert open_sky > 0.9 * len(sphere), (open_sky, len(sphere))
    assert want.ended.mean() > 0.9
    rgb10, rays10, fin10 = trace(w, r.O, r.D, S, 10)
    e = want.ended
    assert np.array_equal(bits(rgb10[e]), bits(rgb[e])) and np.array_equal(rays10[e], rays[e]) and np.array_equal(fin10[e], fin[e])
    assert (rays10[~e] > 2).all()


# ------------------------------------------------------------------ 5. render, budget, features
def frame_case(name, h, wd, spp, ranks):
    """The expected sums of an h x wd frame at depth 2 from the frame's own camera rays, sample by sample, and the three
    render entries against them, for every rank of `ranks`."""
    w = world(name, wd / h)
    spheres = light = 0
    for rank in range(ranks):
        new = lambda: rtmi.Renderer(w.b, h, wd, spp, 2, post=False, rank=rank, world_size=ranks).init_rng()
        R = new()
        pm = rtmi.pixel_map(R.frame)
        px = np.flatnonzero(pm >= 0)
        states = host_states(R.states)
        total, albedo = np.zeros((len(px), 3), F32), np.zeros((len(px), 3), F32)
        rays = np.zeros(len(px), np.int32)
        for sample in range(spp):
            R.states.copy_(dev_states(states))
            o, d = R.camera_rays(sample)
            O, D, S = o.cpu().numpy()[px], d.cpu().numpy()[px], host_states(R.states)
            want = expected_depth2(w, np.ascontiguousarray(O), np.ascontiguousarray(D), S[px])
            total, albedo, rays = (total + want.rgb).astype(F32), (albedo + want.albedo).astype(F32), rays + want.rays
            states = S
            states[px] = want.states
            if sample == 0:
                a, c = texlib.sphere_census(w.lay, O, D, want.q1.view(F32)[:, 0], want.q1[:, 6])
                spheres, light = spheres + a, light + c
        what = (name, h, wd, spp, rank, ranks)
        if spp == 1:  # the statement itself: white on the enclosure, the texel on a sphere whose path reaches the enclosure
            f = want.q1.view(F32)
            for i in range(len(px)):
                m = int(want.q1[i, 6])
                if m == w.lay.white:
                    assert np.array_equal(bits(total[i]), bits(np.ones(3, F32))), (what, i)
                elif want.q1[i, 7] == SPHERE and (m == w.lay.mats[LIGHT] or want.q2[i, 6] == w.lay.white):
                    assert np.array_equal(bits(total[i]), bits(image_value(w.images[m], f[i, 1], f[i, 2]))), (what, i)
        R = new().render()
        R.check()
        assert np.array_equal(bits(R.tiles.cpu().numpy()[px]), bits(total)), what
        assert np.array_equal(R.ray_counts.cpu().numpy()[px], rays) and np.array_equal(host_states(R.states), states), what
        budget = dev(np.where(pm >= 0, spp, 0), np.int32)
        for features in (False, True):
            R = new().render_budget(budget, features=features)
            R.check()
            assert np.array_equal(bits(R.sum.cpu().numpy()[px]), bits(total)), (what, features)
            assert (R.samples.cpu().numpy()[px] == spp).all() and np.array_equal(R.budget_rays.cpu().numpy()[px], rays), (what, features)
            assert np.array_equal(host_states(R.states), states), (what, features)
        assert np.array_equal(bits(R.albedo.cpu().numpy()[px]), bits(albedo)), what
        assert (R.coverage.cpu().numpy()[px] == spp).all()
    return spheres, light


@pytest.mark.parametrize("ranks", [1, 3])
@pytest.mark.parametrize("h,wd", [(16, 16), (20, 24)])
@pytest.mark.parametrize("name", NAMES)
def test_frames_are_the_texels(name, h, wd, ranks):
    """1 spp, depth 2: the pixel is the texel on a textured sphere, white on the enclosure, the material's rule elsewhere."""
    spheres, light = frame_case(name, h, wd, 1, ranks)
    assert spheres >= 20 and light >= 5, (spheres, light)


def test_two_samples_add_in_sample_order():
    frame_case("tex_all", 16, 16, 2, 1)


# ------------------------------------------------------------------ 6. pitch
def test_a_pitched_upload_reads_the_same_texels():
    """The 63 x 65 image from rows of 80 texels (a caller pitch of 320 bytes; the padding holds a colour no texel has):
    the step and the trace give the bits the packed upload gives."""
    a, b = stepped("tex_spheres"), stepped("tex_spheres", True)
    for k in ("O", "D", "S", "E", "A", "raw"):
        assert np.array_equal(bits(getattr(a, k)), bits(getattr(b, k))), k
    for x, y in zip(traced("tex_spheres"), traced("tex_spheres", True)):
        assert np.array_equal(bits(x), bits(y))
    r = texlib.rays("tex_spheres")
    assert (r.target == [k for _, _, k in texlib.SPHERES].index(texlib.PITCHED)).sum() > 4000
