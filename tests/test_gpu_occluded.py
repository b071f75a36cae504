"""rtmi_occluded / SceneBuilder.occluded, ray by ray, against two sources that must agree bit for bit:

  * the oracle: OracleBuilder.probe_hit(o, d) -- HitableList::Hit(Ray(o, d), 1e-3, inf) of the reference's own objects
    -- then the filter float32(t) <= t_max;
  * rtmi_intersect(...).kind != RTMI_HIT_NONE on the same batch with the same t_max.

The occlusion kernel bounds the traversal by t_max and stops early, which is exact except where quirk g8 makes the
bounded mesh walk refuse what the unbounded one accepts; such rays go to the exact fallback, which a
constructed world below exercises."""
import numpy as np
import pytest

import oraclelib
import rtmi
from querylib import (CUSTOM_WORLDS, F32_INF, SCENE_WORLDS, agree, build, filtered, gpu_filtered, gpu_occluded, make_rays, oracle_t,
                      textured_mesh, v3)

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")


def t_max_families(t, rng):
    """Random and boundary t_max families around the closest hits t (float32, +inf: none)."""
    n = len(t)
    base = np.where(np.isfinite(t), t, np.float32(10.0)).astype(np.float32)
    fam = {
        "none": None,
        "scaled": (base * rng.uniform(0.2, 2.0, n)).astype(np.float32),
        "log": np.exp(rng.uniform(np.log(1e-4), np.log(1e3), n)).astype(np.float32),
        "at_t": base,
        "below_t": np.nextafter(base, np.float32(0)).astype(np.float32),
        "above_t": np.nextafter(base, F32_INF).astype(np.float32),
        "specials": rng.choice(np.array([0, -1, np.nan, np.inf, 1e9, np.nextafter(np.float32(1e9), np.float32(0)), 1e-3,
                                         np.nextafter(np.float32(1e-3), np.float32(0))], dtype=np.float32), n),
    }
    return fam


# ------------------------------------------------------------------ the query worlds (tests/querylib.py)
@pytest.mark.parametrize("name", SCENE_WORLDS + sorted(CUSTOM_WORLDS))
def test_occluded_matches_the_oracle(name):
    b, rec, ob, seed = build(name)
    O, D = make_rays(ob, 2000 + len(name))
    t = oracle_t(ob, O, D)
    rng = np.random.default_rng(seed + 17)
    for fam, tm in t_max_families(t, rng).items():
        agree(b, O, D, tm, filtered(t, tm), (name, fam))


def test_boundary_t_max_on_spheres_rounds_like_the_filter():
    """Spheres make the record's t a double: t_max = float32(t) must keep a hit whose double t lies above float32(t)
    (the bounded pass's seed is the largest double that rounds to <= t_max, not t_max itself), and one ulp below
    must drop it."""
    b, rec, ob, seed = build("spheres")
    O, D = make_rays(ob, 31)
    t64 = np.full(len(O), np.inf)
    for i in range(len(O)):
        h, out, _ = ob.probe_hit(O[i], D[i])
        if h:
            t64[i] = out[0]
    t = t64.astype(np.float32)
    above = np.isfinite(t64) & (t64 < 1e8) & (t64 > t.astype(np.float64))  # the double rounds DOWN to t*
    assert above.sum() > 100, above.sum()  # the case is real
    for fam, tm in (("at_t", t), ("below_t", np.nextafter(t, np.float32(0)).astype(np.float32)),
                    ("above_t", np.nextafter(t, F32_INF).astype(np.float32))):
        tm = np.where(np.isfinite(t), tm, np.float32(5.0)).astype(np.float32)
        want = filtered(t, tm)
        agree(b, O, D, tm, want, fam)
        if fam == "at_t":
            assert want[above].all()
        if fam == "below_t":
            assert not want[above].any()


def test_sky_and_special_t_max():
    """Sky answers at t = 1e9: it occludes exactly the rays whose t_max >= 1e9; NaN, 0 and negative t_max are clear."""
    b, rec, ob, seed = build("sky_only")
    rng = np.random.default_rng(4)
    n = 600
    O = rng.uniform(-5, 5, (n, 3)).astype(np.float32)
    D = rng.normal(size=(n, 3)).astype(np.float32)
    specials = np.array([0, -1, np.nan, np.inf, 1e9, np.nextafter(np.float32(1e9), np.float32(0)), -np.inf, 1.0],
                        dtype=np.float32)
    tm = specials[np.arange(n) % len(specials)]
    want = np.isin(np.arange(n) % len(specials), [3, 4])  # inf, 1e9
    assert np.array_equal(filtered(oracle_t(ob, O, D), tm), want)
    agree(b, O, D, tm, want, "sky")
    agree(b, O, D, None, np.ones(n, dtype=bool), "sky, no limit")
    # a world with geometry and Sky: the same specials against the oracle
    b, rec, ob, seed = build("nested")
    O, D = make_rays(ob, 8)
    tm = specials[np.arange(len(O)) % len(specials)]
    agree(b, O, D, tm, filtered(oracle_t(ob, O, D), tm), "nested")


def test_bad_rays_change_no_other_answer():
    for name in ("cornell_box", "bunny", "spheres"):
        b, rec, ob, seed = build(name)
        O, D = make_rays(ob, 77)
        rng = np.random.default_rng(1)
        tm = (oracle_t(ob, O, D) * rng.uniform(0.5, 1.5, len(O))).astype(np.float32)
        tm[~np.isfinite(tm)] = 50.0
        ref, _ = gpu_occluded(b, O, D, tm)
        Ob, Db = O.copy(), D.copy()
        which = np.arange(len(O)) % 11 == 3
        for j, i in enumerate(np.nonzero(which)[0]):
            r = j % 6
            if r == 0:
                Ob[i, 0] = np.nan
            elif r == 1:
                Db[i, 1] = np.inf
            elif r == 2:
                Db[i] = 0.0
            elif r == 3:
                Ob[i, 2] = -np.inf
            elif r == 4:
                Db[i] = 1e30  # |d|^2 overflows
            else:
                Db[i] = 1e-30  # |d|^2 underflows
        got, _ = gpu_occluded(b, Ob, Db, tm)
        assert not got[which].any(), name
        assert np.array_equal(got[~which], ref[~which]), name
        # and a batch without the bad rays at all
        good, _ = gpu_occluded(b, O[~which], D[~which], tm[~which])
        assert np.array_equal(good, ref[~which]), name


def two_meshes_mixed(b):
    textured_mesh(b)
    m = b.metal(v3(0.8, 0.8, 0.8), 0.2)
    b.sphere(v3(1.6, 0.3, 0.4), 0.5, m)
    b.triangle([v3(-2, -1, -1), v3(-1, 1.5, -1.5), v3(-2.5, 0.5, 0.5)], m)
    b.sphere(v3(-0.8, -0.7, 1.2), 0.35, m)


def test_two_meshes_triangles_and_spheres():
    CUSTOM_WORLDS["occ_two_meshes_mixed"] = two_meshes_mixed
    try:
        b, rec, ob, seed = build("occ_two_meshes_mixed")
    finally:
        del CUSTOM_WORLDS["occ_two_meshes_mixed"]
    O, D = make_rays(ob, 12)
    t = oracle_t(ob, O, D)
    for fam, tm in t_max_families(t, np.random.default_rng(12)).items():
        agree(b, O, D, tm, filtered(t, tm), fam)


def g8_world(b, with_sphere=False):
    """A mesh of four faces, two reference leaves (k_min = 2; faces sort by their first vertex's x): leaf 0 holds a
    wall at x = 5 and a face in the plane y = -1 that stretches its box to x in [2, 10].  A ray from inside that box
    along +x meets the wall at t = 5 - x0, but leaves the box (its only crossing of the box's surface) at t = 10 - x0:
    with t_to below that, AABB::Hit refuses the box (quirk g8), while the unbounded walk enters it and hits the wall."""
    b.camera_pinhole(v3(0, 0, 30), v3(5, 0, 0), v3(0, 1, 0), 0.9, 1.0)
    m = b.lambertian(v3(0.5, 0.5, 0.5))
    faces = np.array([
        [2, -1, -1, 10, -1, -1, 10, -1, 1.5],   # leaf 0: y = -1, stretches the box
        [5, -1, -1, 5, 1, -1, 5, 0, 1.5],       # leaf 0: the wall at x = 5
        [500, 5, 5, 501, 5, 5, 500, 6, 5],      # leaf 1, off the rays' way: it makes the mesh 600 long, so that a
        [600, 5, 5, 601, 5, 5, 600, 6, 5],      # t_max below 30 (1/20 of that) keeps the bounded walk
    ], dtype=np.float32)
    b.bvh(faces, m, k_min=2)
    if with_sphere:
        b.sphere(v3(0, 30, 0), 1.0, m)  # (binary64 records: the other engine type)


@pytest.mark.parametrize("with_sphere", [False, True])
def test_g8_world_is_answered_by_the_fallback(with_sphere):
    seed = 9
    b, ob = rtmi.SceneBuilder(seed), oraclelib.OracleBuilder(seed)
    g8_world(b, with_sphere)
    g8_world(ob, with_sphere)
    b.commit()
    rng = np.random.default_rng(2)
    n = 256
    x0 = rng.uniform(2.2, 4.8, n).astype(np.float32)
    O = np.stack([x0, rng.uniform(-0.3, 0.3, n), rng.uniform(-0.3, 0.3, n)], 1).astype(np.float32)
    D = np.tile(np.array([[1, 0, 0]], dtype=np.float32), (n, 1))
    wall, leave = (np.float32(5) - x0), (np.float32(10) - x0)
    tm = (wall + rng.uniform(0.05, 0.95, n).astype(np.float32) * (leave - wall)).astype(np.float32)  # between the two
    tm[::4] = (leave[::4] + np.float32(1)).astype(np.float32)  # beyond the box's exit: the bounded walk enters it
    t = oracle_t(ob, O, D)
    want = filtered(t, tm)
    assert want.all()  # every ray hits the wall within its t_max
    bounded = np.array([ob.probe_hit(O[i], D[i], 1e-3, float(tm[i]))[0] for i in range(n)])
    g8 = ~bounded
    assert g8.sum() > n // 2, g8.sum()  # the case is real: Hit(ray, 1e-3, t_max) misses what the filter keeps
    assert bounded[::4].all()
    fb = agree(b, O, D, tm, want, "g8")
    assert fb > 0
    assert fb == g8.sum(), (fb, g8.sum())  # exactly the refused rays went to the fallback
    # longer rays from inside the mesh's bounds (t_max >= 1/20 of its extent) walk from +inf: no fallback needed
    tm_long = (tm + np.float32(40)).astype(np.float32)
    assert filtered(t, tm_long).all()
    assert agree(b, O, D, tm_long, filtered(t, tm_long), "g8, long") == 0


def test_ambient_occlusion_rays_on_the_bunny():
    b, rec, ob, seed = build("bunny")
    cam = ob.camera_get()
    rng = np.random.default_rng(6)
    n = 1 << 16
    xy = rng.random((n, 2)).astype(np.float32)
    O = np.repeat(cam[0][None].astype(np.float32), n, 0)
    D = (cam[1] + xy[:, :1] * cam[2] + xy[:, 1:] * cam[3] - cam[0]).astype(np.float32)
    h = b.intersect(torch.from_numpy(O).cuda(), torch.from_numpy(D).cuda()).check()
    kind = h.kind.cpu().numpy()
    sel = kind == rtmi.RTMI_HIT_MESH
    t = h.t.cpu().numpy()[sel]
    N = h.normal.cpu().numpy()[sel]
    Dn = D[sel] / np.linalg.norm(D[sel], axis=1, keepdims=True).astype(np.float32)
    P = (O[sel] + t[:, None] * Dn).astype(np.float32)
    u = rng.normal(size=P.shape).astype(np.float32)
    u /= np.linalg.norm(u, axis=1, keepdims=True)
    A = (N + u).astype(np.float32)  # about the normal
    ext = float(np.ptp(P, axis=0).max())
    m = len(P)
    for frac in (0.02, 0.2, np.inf):
        tm = np.full(m, np.float32(frac * ext), dtype=np.float32)
        ref = gpu_filtered(b, P, A, tm)
        got, fb = gpu_occluded(b, P, A, tm)
        assert np.array_equal(got, ref), (frac, int((got != ref).sum()))
        if frac == 0.2:
            assert 0 < ref.sum() < m, (frac, int(ref.sum()))  # (at 2 % hardly any ray is occluded)
        elif not np.isfinite(frac):
            assert ref.all()  # the scene has Sky
        idx = rng.choice(m, 3000, replace=False)
        want = filtered(oracle_t(ob, P[idx], A[idx]), tm[idx])
        assert np.array_equal(got[idx], want), frac


def test_four_million_rays_against_intersect():
    b, rec, ob, seed = build("bunny")
    cam = ob.camera_get()
    n = 1 << 22
    g = torch.Generator(device="cuda").manual_seed(13)
    xy = torch.rand((n, 2), generator=g, device="cuda", dtype=torch.float32)
    c = torch.from_numpy(np.ascontiguousarray(cam[:4], dtype=np.float32)).cuda()
    o = c[0].expand(n, 3).contiguous()
    d = (c[1] + xy[:, :1] * c[2] + xy[:, 1:] * c[3] - c[0]).contiguous()
    tm = torch.rand((n,), generator=g, device="cuda").contiguous()  # (the bunny is 0.5 from the camera)
    ref = b.intersect(o, d, tm).check().kind != rtmi.RTMI_HIT_NONE
    out = torch.zeros((n,), dtype=torch.bool, device="cuda")
    r = b.occluded(o, d, tm, out=out).check()
    assert r.mask.data_ptr() == out.data_ptr()
    assert torch.equal(out, ref), int((out != ref).sum())
    assert 0 < int(ref.sum()) < n


def test_batch_shapes_and_out_buffer():
    b, rec, ob, seed = build("cornell_box")
    O, D = make_rays(ob, 5)
    tm = np.full(len(O), np.float32(300.0), dtype=np.float32)
    ref, _ = gpu_occluded(b, O, D, tm)
    for n in (1, 63, 65):
        assert np.array_equal(gpu_occluded(b, O[:n], D[:n], tm[:n])[0], ref[:n]), n
    assert gpu_occluded(b, O[:0], D[:0], tm[:0])[0].shape == (0,)
    out = torch.full((len(O),), 7, dtype=torch.uint8, device="cuda")
    got, _ = gpu_occluded(b, O, D, tm, out=out)
    assert np.array_equal(out.cpu().numpy(), ref.astype(np.uint8))  # every byte written, 0 or 1
