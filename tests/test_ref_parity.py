"""The oracle against the reference's own code.

oracle/_ref/libref.so is the reference's translation units, unchanged, compiled for the CPU with the oracle's flags
against the stand-in headers of oracle/refshim/ (oracle/Makefile).  Both sides are g++ builds with one libm on one
host, so every comparison here is an equality of bits: float and double results through their integer views, final RNG
states, per-pixel query counts.  The cases are those of tests/refcases.py.

Three operations differ between the two builds for reasons outside the reference's text; each is named, and held to
the tightest statement that is exact ("shared assumptions of oracle and reference build"):
  * sphere.cu's pow(discriminant, 0.5) is the host libm's pow there and a correctly rounded sqrt in the oracle: with the
    oracle switched to pow (oraclelib.host_variant) every bit agrees; unswitched, only t may differ, by one ulp.
  * thrust::sort is std::sort there and a stable sort in the oracle: a mesh whose sort keys tie is compared with the
    oracle switched to std::sort; a mesh without ties is compared as it is.
  * g++ evaluates DiskRand's two draws right to left, the oracle left to right: the defocus camera is compared with the
    oracle's draws switched, and the RNG state after (which no order changes) unswitched too.
A record's fields that the reference leaves indeterminate (u, v and the normal of a Sky hit; u, v of a BVH face
without texture coordinates) are not compared: refcases.defined_columns.

Skipped, with the reason, where neither libref.so nor a reference checkout to build it from exists.
"""
import numpy as np
import pytest

import oraclelib
import refcases as rc
from refcases import bits
import reflib

pytestmark = pytest.mark.skipif(not reflib.available(), reason=reflib.SKIP_REASON)


def assert_same_bits(a, b, what):
    a, b = bits(a), bits(b)
    assert a.shape == b.shape, what
    assert np.array_equal(a, b), "%s: %d of %d values differ" % (what, int((a != b).sum()), a.size)


def probe_both(name, variant=0):
    with oraclelib.host_variant(variant):
        o = rc.build_probe_world(oraclelib.OracleBuilder(1), name)
        table = rc.probe_table(o, name)
        res_o = rc.run_probes(o, table)
    res_r = rc.run_probes(rc.build_probe_world(reflib.RefBuilder(1), name), table)
    return table, res_o, res_r


def assert_probes_equal(name, table, res_o, res_r, skip_t=False):
    (hit_o, rec_o, mat_o), (hit_r, rec_r, mat_r) = res_o, res_r
    assert hit_o.sum() > table.shape[0] // 4, "%s: too few rays hit to test anything" % name
    assert np.array_equal(hit_o, hit_r), "%s: hit flags differ on %d rays" % (name, int((hit_o != hit_r).sum()))
    assert np.array_equal(mat_o, mat_r), "%s: materials differ" % name
    keep = rc.defined_columns(name, hit_r, rec_r, mat_r)
    if skip_t:
        keep[:, 0] = False
    assert_same_bits(np.where(keep, rec_o, 0.0), np.where(keep, rec_r, 0.0), name + ": records {t,u,v,normal}")


EXACT_WORLDS = [w for w in rc.PROBE_WORLDS if w not in ("sphere", "bvh_ties")]


@pytest.mark.parametrize("name", EXACT_WORLDS)
def test_probe_hit(name):
    """world->Hit on single primitives, lists with ties, nested lists and BVHs (a leaf with coincident faces, 2048 and
    2049 faces either side of the split threshold, a mesh that splits): random, grazing and inside rays, hits exactly
    at t_to and t_from and one ulp past them, and self-hits around 1e-3."""
    table, res_o, res_r = probe_both(name, rc.PROBE_VARIANT.get(name, 0))  # a world with a sphere: its root by pow
    assert_probes_equal(name, table, res_o, res_r)


def test_probe_hit_sphere():
    """From outside, inside and grazing.  Bit-equal with the oracle's root taken by pow as the host build does; as the
    oracle stands (sqrt), everything but t is bit-equal and t differs by at most one ulp (sqrt is correctly rounded
    and glibc's pow is within one ulp)."""
    table, res_o, res_r = probe_both("sphere", oraclelib.VARIANT_SPHERE_ROOT_POW)
    assert_probes_equal("sphere", table, res_o, res_r)
    res_d = rc.run_probes(rc.build_probe_world(oraclelib.OracleBuilder(1), "sphere"), table)
    assert_probes_equal("sphere", table, res_d, res_r, skip_t=True)
    t_d, t_r = res_d[1][:, 0], res_r[1][:, 0]
    lo, hi = np.nextafter(t_r, -np.inf), np.nextafter(t_r, np.inf)
    assert ((t_d == t_r) | (t_d == lo) | (t_d == hi)).all()


def test_probe_hit_bvh_with_tied_sort_keys():
    """A mesh of 2400 faces with six distinct sort keys: which faces land left and right of the split is the sort's
    choice among equals.  With the oracle's sort switched to std::sort, as thrust::sort stands in the host build, every
    record is bit-equal."""
    table, res_o, res_r = probe_both("bvh_ties", oraclelib.VARIANT_UNSTABLE_SORT)
    assert_probes_equal("bvh_ties", table, res_o, res_r)


def test_scatter():
    """Material::Scatter and Emit: Lambertian (constant and image-textured; the rejection loop's draw count shows in
    the state after), Metal at fuzz 0, 0.3 and clamped, Dielectric at two indices entering, leaving and at total
    internal reflection (the reference's Dielectric has no Schlick term: it refracts or ends the path), DiffuseLight."""
    o, r = oraclelib.OracleBuilder(1), reflib.RefBuilder(1)
    names = rc.scatter_materials(o)
    assert rc.scatter_materials(r) == names
    table, states = rc.scatter_table()
    sc_o, out_o, st_o = rc.run_scatter(o, table, states)
    sc_r, out_r, st_r = rc.run_scatter(r, table, states)
    per = sc_o.reshape(len(names), -1).sum(axis=1)
    n = table.shape[0] // len(names)
    for k, nm in enumerate(names):  # the table reaches both outcomes of every material that has two
        assert (per[k] == 0) if nm.startswith("light") else (0 < per[k] < n), (nm, per[k])
    assert np.array_equal(sc_o, sc_r)
    assert_same_bits(out_o, out_r, "attenuation, scattered ray, emitted")
    assert np.array_equal(st_o, st_r), "RNG states after Scatter differ"
    lam = table[:, 0] < 2
    assert ((st_o != states).any(axis=1)[lam] == (sc_o[lam] == 1)).all(), "Lambertian draws iff it scatters"


@pytest.mark.parametrize("kind", rc.CAMERAS)
def test_camera(kind):
    """The three constructors' frames, RayAt at the corners, the centre and random points, and the defocus draws."""
    xy, states = rc.camera_table()
    variant = oraclelib.VARIANT_DISKRAND_RTL if kind == "defocus" else 0
    with oraclelib.host_variant(variant):
        f_o, rays_o, st_o = rc.run_camera(rc.build_camera(oraclelib.OracleBuilder(1), kind), xy, states)
    f_r, rays_r, st_r = rc.run_camera(rc.build_camera(reflib.RefBuilder(1), kind), xy, states)
    assert_same_bits(f_o, f_r, "camera frame")
    assert_same_bits(rays_o, rays_r, "camera rays")
    assert np.array_equal(st_o, st_r)
    assert (st_o != states).any() == (kind == "defocus")
    if kind == "defocus":  # unswitched: the same two draws in the other order, so the same state after
        _, rays_d, st_d = rc.run_camera(rc.build_camera(oraclelib.OracleBuilder(1), kind), xy, states)
        assert np.array_equal(st_d, st_r)
        assert not np.array_equal(rays_d, rays_r)


def test_rng_init_and_random_float():
    """CudaRandomInit over a grid of 64-thread blocks and CudaRandomFloat, both seeds."""
    for seed in rc.SEEDS:
        st_o, st_r = oraclelib.rng_init(seed, 200), reflib.rng_init(seed, 200)
        assert np.array_equal(st_o, st_r)
        o, r = oraclelib.OracleBuilder(seed), reflib.RefBuilder(seed)
        a = np.array([o.random_float(mn, mx) for mn, mx in [(0, 1), (-1, 1), (0, 0.9), (0, 0.5)] * 50])
        b = np.array([r.random_float(mn, mx) for mn, mx in [(0, 1), (-1, 1), (0, 0.9), (0, 0.5)] * 50])
        assert_same_bits(a, b, "CudaRandomFloat")
        assert np.array_equal(o.state0, r.state0)


def test_bvh_default_mesh_splits_and_matches():
    """procedural_bunny_mesh at its default: 69,312 faces, so BVHNode splits six levels deep at the reference's leaf
    size.  The bunny scene on it, both seeds."""
    from rtmi import scenes
    mesh = scenes.procedural_bunny_mesh()
    assert mesh.shape[0] > 2048
    h, w, spp = 12, 16, 2
    for seed in rc.SEEDS:  # as the oracle stands: its sort keys tie in pairs (two triangles of a quad share a corner)
        o = oraclelib.OracleBuilder(seed)
        scenes.bunny(o, w / h, mesh.copy(), k_min=2048)
        res_o = o.render(h, w, spp, rc.DEPTH, threads=1)
        r = reflib.RefBuilder(seed)
        scenes.bunny(r, w / h, mesh.copy(), k_min=2048)
        res_r = r.render(h, w, spp)
        assert_same_frames(res_o, res_r, "bunny, default mesh, seed %d" % seed)
        assert (res_o[1] > spp).any(), "no path left the first surface"


def assert_same_frames(res_o, res_r, what):
    (rgb_o, rays_o, st_o, tot_o), (rgb_r, rays_r, st_r, tot_r) = res_o, res_r
    assert tot_o == tot_r, "%s: total queries %d vs %d" % (what, tot_o, tot_r)
    assert np.array_equal(rays_o, rays_r), "%s: per-pixel query counts differ" % what
    assert np.array_equal(st_o, st_r), "%s: final RNG states differ" % what
    assert_same_bits(rgb_o, rgb_r, what + ": image")


@pytest.mark.parametrize("post", [True, False], ids=["post", "raw"])
@pytest.mark.parametrize("seed", rc.SEEDS)
@pytest.mark.parametrize("name,h,w,spp", rc.FRAMES, ids=[f[0] for f in rc.FRAMES])
def test_frames(name, h, w, spp, seed, post):
    """Every scene of rtmi/scenes.py and the nested-lists world, at the goldens' small shapes and depth 10, as the
    oracle stands (no variant): image, final states and per-pixel counts.  The spheres scene draws its layout from
    pixel 0's stream on either side's own generator."""
    o = rc.build_frame_scene(oraclelib.OracleBuilder(seed), name, w / h)
    r = rc.build_frame_scene(reflib.RefBuilder(seed), name, w / h)
    assert np.array_equal(o.state0, r.state0)
    assert_same_frames(o.render(h, w, spp, rc.DEPTH, post=post, threads=1), r.render(h, w, spp, post=post),
                       "%s seed %d" % (name, seed))


def test_get_workload():
    L, R = oraclelib.lib(), reflib.lib()
    for spp in [1, 7, 20, 100, 200, 1024]:
        for world in [1, 2, 3, 4, 7, 8, 16]:
            for rank in range(world):
                assert L.orc_get_workload(rank, world, spp) == R.ref_get_workload(rank, world, spp)
