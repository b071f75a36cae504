"""tests/texlib.py on the CPU, against the oracle alone: the restated ImageTexture::Value is the oracle's on every shape,
the ray families reach the texels, boundaries, seam and pole values they are for, and the binary64 restatement of the
sphere's GetUV stays within the project's tolerance of the host libm's.  What makes tests/test_gpu_texel.py mean
something; no GPU involved."""
import functools

import numpy as np
import pytest

import oraclelib
import texlib
from parity import bits
from querylib import SPHERE_UV_TOL, v3
from texlib import F32, FAMILIES, SPHERES, family, image_value, sphere_uv_truth, texel_index, textures


# ------------------------------------------------------------------ the textures
def test_no_two_texels_of_an_image_share_a_colour():
    assert [t.shape[:2] for t in textures()] == texlib.SHAPES + [texlib.LIGHT_SHAPE]
    for img in textures():
        assert img.dtype == np.uint8 and len(np.unique(img.reshape(-1, 4)[:, :3], axis=0)) == img.shape[0] * img.shape[1]
    rows = texlib.padded_rows(textures()[texlib.PITCHED], 80)
    assert rows.shape == (63, 80, 4) and np.array_equal(rows[:, :65], textures()[texlib.PITCHED])


def axis_grid(n):
    k = np.arange(n + 1) / n
    near = np.concatenate([k, np.nextafter(k.astype(F32), F32(-1)), np.nextafter(k.astype(F32), F32(2))]).astype(np.float64)
    special = np.array([0.0, 1.0, 1.0 + 2.0 ** -24, 1.0 - 2.0 ** -24, 2.0 ** -24, 2.0 ** -60, -2.0 ** -24, 1.5, -0.25])
    return np.concatenate([special, near]), special


@pytest.mark.parametrize("k", range(len(textures())))
def test_image_value_is_the_oracles(k):
    """ImageTexture::Value read through a textured Lambertian's attenuation and a textured light's emission."""
    img = textures()[k]
    h, w = img.shape[:2]
    ob = oraclelib.OracleBuilder(1)
    t = ob.image_texture(img)
    lam, light = ob.lambertian_tex(t), ob.diffuse_light(t)
    o, d, n = v3(0, 0, 1), v3(0, 0, -1), v3(0, 0, 1)
    (us, u_special), (vs, v_special) = axis_grid(w), axis_grid(h)
    grid = [(u, v) for u in us for v in v_special] + [(u, v) for u in u_special for v in vs]
    state = oraclelib.rng_init(5, 1)[0]
    seen = set()
    for u, v in grid:
        want = image_value(img, u, v)
        sc, out = ob.probe_scatter_ex(lam, o, d, 1.0, u, v, n, state.copy())
        assert sc and np.array_equal(bits(out[0:3]), bits(want)) and not out[9:12].any(), (k, u, v)
        sc, out = ob.probe_scatter_ex(light, o, d, 1.0, u, v, n, state.copy())
        assert not sc and np.array_equal(bits(out[9:12]), bits(want)), (k, u, v)
        seen.add(texel_index(h, w, u, v))
    assert {i for i, _ in seen} == set(range(h)) and {j for _, j in seen} == set(range(w))
    # the flip: v = 0 reads row 0, the smallest v above it the last row; u = 1 wraps onto column 0
    assert texel_index(h, w, 0.0, 0.0) == (0, 0) and texel_index(h, w, 0.0, 2.0 ** -24) == (h - 1, 0)
    assert texel_index(h, w, 1.0, 1.0) == (0, 0) and texel_index(h, w, 1.0 - 2.0 ** -24, 0.5)[1] == w - 1


# ------------------------------------------------------------------ the families, by the oracle alone
@functools.lru_cache(maxsize=None)
def records():
    ob, lay = texlib.build_oracle("tex_all")
    r = texlib.rays("tex_all")
    hit, out, mat = texlib.oracle_records(ob, r.O, r.D)
    return r, lay, hit, out, mat


def test_every_ray_meets_its_own_surface():
    r, lay, hit, out, mat = records()
    assert hit.all()
    for s in range(len(SPHERES)):
        idx = np.flatnonzero((r.target == s) & (r.family < len(texlib.SPHERE_FAMILIES)))
        assert len(idx) and (mat[idx] == lay.mats[SPHERES[s][2]]).all(), s
        assert np.allclose(out[idx, 0], 2 * SPHERES[s][1], rtol=1e-4), s  # (the near side of its own sphere)
    for name in ("pgram", "mesh"):
        idx = family(r, name)
        assert len(idx) and (mat[idx] == np.array(lay.mats)[r.target[idx]]).all(), name
        assert np.array_equal(out[idx, 0], np.full(len(idx), 0.25)), name
    # the same rays of the spheres make up tex_spheres
    rs = texlib.rays("tex_spheres")
    n = len(rs.O)
    assert n == int((r.family < len(texlib.SPHERE_FAMILIES)).sum())
    assert np.array_equal(bits(rs.O), bits(r.O[:n])) and np.array_equal(bits(rs.D), bits(r.D[:n]))
    print({f: len(family(r, f)) for f in FAMILIES})


def test_centres_visit_every_texel():
    r, lay, hit, out, mat = records()
    idx = family(r, "centres")
    for i in idx:
        h, w = textures()[SPHERES[r.target[i]][2]].shape[:2]
        assert texel_index(h, w, out[i, 1], out[i, 2]) == (r.info[i, 0], r.info[i, 1]), i
    for s, (_, _, k) in enumerate(SPHERES):
        h, w = textures()[k].shape[:2]
        got = {(a, b) for a, b in r.info[idx[r.target[idx] == s], :2].tolist()}
        assert got == {(a, b) for a in range(h) for b in range(0, w, texlib.COLUMN_STRIDE.get((h, w), 1))}, s


def test_edges_select_both_sides_of_every_boundary():
    r, lay, hit, out, mat = records()
    idx = family(r, "edges")
    sel = collections_of(r, out, idx)
    for s, (_, _, k) in enumerate(SPHERES):
        h, w = textures()[k].shape[:2]
        for kb in range(w + 1):  # the boundary u = kb / w, on row `aim`: columns kb - 1 and kb (the seam: w - 1 and 0)
            aim = kb % h
            assert {(aim, (kb - 1) % w), (aim, kb % w)} <= sel[(s, 0, kb)], (s, "u", kb, sel[(s, 0, kb)])
        for kb in range(1, h):  # the boundary v = kb / h, on column `aim`: rows h - kb - 1 and h - kb
            aim = kb % w
            assert {(h - kb - 1, aim), (h - kb, aim)} <= sel[(s, 1, kb)], (s, "v", kb, sel[(s, 1, kb)])


def collections_of(r, out, idx):
    sel = {}
    for i in idx:
        h, w = textures()[SPHERES[r.target[i]][2]].shape[:2]
        sel.setdefault((int(r.target[i]), int(r.info[i, 0]), int(r.info[i, 1])), set()).add(texel_index(h, w, out[i, 1], out[i, 2]))
    return sel


def test_seam_and_poles_reach_the_exact_values():
    r, lay, hit, out, mat = records()
    seam, poles = family(r, "seam"), family(r, "poles")
    u, v = out[:, 1], out[:, 2]
    assert (u[seam] == 0.0).any() and (u[seam] == 1.0).any(), np.unique(u[seam])
    assert (v[poles] == 0.0).any() and (v[poles] == 1.0).any() and set(np.unique(v[poles])) == {0.0, 1.0}
    for value in (0.0, 0.25, 0.5, 0.75, 1.0):
        assert (u[poles] == value).any(), (value, np.unique(u[poles]))
    # the signed zeros of the normal decide: both signs of z at the seam, all four sign pairs at the poles
    nz = F32(out[seam, 5])
    assert (bits(nz) == 0).any() and (bits(nz) == 0x80000000).any()
    pairs = {(int(a), int(b)) for a, b in zip(bits(F32(out[poles, 3])), bits(F32(out[poles, 5])))}
    assert {(a, b) for a in (0, 0x80000000) for b in (0, 0x80000000)} <= pairs
    sub = np.abs(out[np.concatenate([seam, poles]), 3:6])
    assert ((sub > 0) & (sub < 2.0 ** -126)).any(), "no subnormal normal component"
    axes = family(r, "axes")
    assert set(np.unique(u[axes])) <= {0.0, 0.25, 0.5, 0.75, 1.0} and (v[axes] == 0.5).all()


def test_flat_families_reach_the_intended_floats():
    r, lay, hit, out, mat = records()
    for k in range(len(textures())):
        h, w = textures()[k].shape[:2]
        idx = np.flatnonzero((r.family == FAMILIES.index("pgram")) & (r.target == k))
        O, D, p = texlib.flat_rays("pgram", k)
        assert np.array_equal(bits(O), bits(r.O[idx]))
        x, y = p[:, 0], p[:, 1]
        first = x.astype(np.float64) + y.astype(np.float64) <= 1.0  # the triangle (p0, p1, p2): u = x
        assert first.sum() > len(p) // 2
        assert np.array_equal(bits(out[idx[first], 1]), bits(x[first])), k
        on_axis = x == 0  # there v = (float)(1 - y) + 0
        assert np.array_equal(bits(out[idx[on_axis], 2]), bits((1.0 - y[on_axis].astype(np.float64)).astype(F32))), k
        u, v = out[idx, 1], out[idx, 2]
        for value in (0.0, 1.0):
            assert (u == value).any() and (v == value).any(), (k, value)
        assert (v == 2.0 ** -24).any() and (u == F32(1 - 2.0 ** -24)).any()
        sel = {texel_index(h, w, a, b) for a, b in zip(u, v)}
        assert {i for i, _ in sel} == set(range(h)) and {j for _, j in sel} == set(range(w)), k
        for kb in range(1, w):  # the boundary itself is among the u values, and a float either side
            at = F32(kb / w)
            assert (u == at).any() and (u == np.nextafter(at, F32(0))).any() and (u == np.nextafter(at, F32(1))).any(), (k, kb)
    idx = family(r, "mesh")
    h, w = textures()[texlib.MESH_TEX].shape[:2]
    sel = {texel_index(h, w, a, b) for a, b in zip(out[idx, 1], out[idx, 2])}
    assert {i for i, _ in sel} == set(range(h)) and {j for _, j in sel} == set(range(w))


# ------------------------------------------------------------------ sphere_uv_truth against the host libm
def test_sphere_uv_truth_within_the_tolerance_of_the_host_libm():
    """Largest |u - truth| and |v - truth| of the oracle's GetUV (the host's acosf / atan2f) over all 33,082 sphere rays
    (glibc 2.35, x86-64): 1.19e-07 for u (centres, ray 2140 on sphere 4) and 1.19e-07 for v (centres, ray 2044 on sphere
    4), two units in the last place of a value in [0.5, 1) -- the figures in NOTES.md.  Were it above SPHERE_UV_TOL, the
    project's tolerance would not hold for the host libm either."""
    r, lay, hit, out, mat = records()
    idx = np.flatnonzero(r.family < len(texlib.SPHERE_FAMILIES))
    tu, tv = sphere_uv_truth(out[idx, 3:6].astype(F32))
    du, dv = np.abs(out[idx, 1] - tu.astype(np.float64)), np.abs(out[idx, 2] - tv.astype(np.float64))
    for what, dd in (("u", du), ("v", dv)):
        i = int(np.argmax(dd))
        print("host libm: max |%s - truth| = %.3g at %s ray %d (sphere %d), normal %r" %
              (what, dd[i], FAMILIES[r.family[idx[i]]], idx[i], r.target[idx[i]], out[idx[i], 3:6].tolist()))
    assert du.max() < SPHERE_UV_TOL and dv.max() < SPHERE_UV_TOL
    # the restatement is not vacuous: the exact values come out exactly
    assert (tu == 0).any() and (tu == 1).any() and (tu == F32(0.5)).any() and (tv == 0).any() and (tv == 1).any()


# ------------------------------------------------------------------ what a small frame sees of the worlds
@pytest.mark.parametrize("h,w", [(16, 16), (20, 24)])
@pytest.mark.parametrize("name", ["tex_spheres", "tex_all"])
def test_small_frames_see_the_textured_spheres(name, h, w):
    """The render checks of tests/test_gpu_texel.py run on the first sample's camera rays: enough of them meet textured
    Lambertian spheres (20) and the textured light (5)."""
    ob, lay = texlib.build_oracle(name, w / h)
    O, D = texlib.oracle_primary_rays(ob, h, w)
    hit, out, mat = texlib.oracle_records(ob, O, D)
    assert hit.all()
    spheres, light = texlib.sphere_census(lay, O, D, out[:, 0], mat)
    print(name, h, w, "primary rays on textured Lambertian spheres:", spheres, "on the textured light:", light)
    assert spheres >= 20 and light >= 5
