"""The shared candidate tests of the culled list scan, one triangle per lane (closest_hit.h, RUN_TRIS, step (b)).

Renders are compared with the oracle bit for bit -- image, per-pixel ray counts, final RNG states, ray total -- and
queries on the bits of t, u, v, normal, entry and element, on worlds that put a chosen number of (ray, pair) tasks into a
wave's flush (tests/tri_tasks_worlds.py): n stacked sheets give a full wave 64 (n - 1) pair tasks, i.e. 128 (n - 1)
triangle tests in rounds of 64; a wave's region holds kListTasks = 192 pair tasks, so seven sheets (384) flush twice with
lanes left waiting.  No tolerances anywhere."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import rtmi
import tri_tasks_worlds as worlds
from abi_host import CHECK_LIB, ROOT
from parity import assert_same_frame, build_pair, gpu_frame, oracle_frame
from querylib import check_identities, compare, filtered, gpu_filtered, gpu_intersect, gpu_occluded, make_rays, oracle_t

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

SEED = 7


def render_both(fill, side, spp=4, depth=8):
    ob, pb = build_pair(fill, SEED)
    o = oracle_frame(ob, side, side, spp, depth)
    assert_same_frame(gpu_frame(pb, side, side, spp, depth), o, "%d x %d" % (side, side))
    return pb, o.counts


@pytest.mark.parametrize("light", [False, True])
@pytest.mark.parametrize("n", [2, 3, 4, 7])
def test_stacked_sheets(n, light):
    """64, 128, 192 and 384 pair tasks per full wave: round boundaries at 32, 64 and 96 triangle tests (the waves at the
    frame's rim carry fewer rays), exactly kListTasks, and a flush that leaves lanes waiting.  The light behind the stack
    is one more candidate of every ray: 128, 192, 256 and 448."""
    b, rays = render_both(worlds.sheets(n, light), 16)
    assert b.stats()["parallelograms"] == 4 + n + (1 if light else 0)
    assert (rays >= 4 * (n + 1)).all() or n == 7  # every path crosses the whole stack (seven sheets: as far as depth 8 lets it)


def test_mixed_list_of_lone_triangles_and_parallelograms():
    b, rays = render_both(worlds.mixed_list(7), 16, spp=8)
    st = b.stats()
    assert st["triangles"] == 4 and st["parallelograms"] == 3 and rays.max() > 8


@pytest.mark.parametrize("world", ["sheets_4_light", "sheets_7", "mixed_list"])
def test_thin_frame(world):
    """8 x 8: one tile, and the grid has far more lanes than pixels -- most lanes are workers without a ray of their own."""
    fill = {"sheets_4_light": worlds.sheets(4, True), "sheets_7": worlds.sheets(7), "mixed_list": worlds.mixed_list(7)}[world]
    render_both(fill, 8, spp=8)


def test_spheres_next_to_pairs_carry_a_binary64_bound():
    b, rays = render_both(worlds.spheres_and_pairs, 16)
    assert b.stats()["spheres"] == 2 and b.stats()["parallelograms"] >= 4


@pytest.mark.parametrize("n_pairs", [130, 200])
def test_long_lists_gather_their_records(n_pairs):
    b, _ = render_both(worlds.long_list(n_pairs), 16, spp=2, depth=6)
    assert b.stats()["triangles"] + b.stats()["parallelograms"] == n_pairs > 128  # beyond kLdsPairs


def _query_world(fill):
    ob, rec = build_pair(fill, SEED, record=True)
    return rec.b, rec, ob


@pytest.mark.parametrize("world", ["textured", "mixed_list", "long_list_130"])
def test_intersect_bits_through_the_result_words(world):
    """rtmi_intersect runs the image-texture variant: the winner's u and v come back through the tasks' result words.
    The batch is no multiple of 64."""
    fill = {"textured": worlds.textured, "mixed_list": worlds.mixed_list(7), "long_list_130": worlds.long_list(130)}[world]
    b, rec, ob = _query_world(fill)
    O, D = make_rays(ob, 31, n_family=150)
    n = len(O) - (1 if len(O) % 64 == 0 else 0)
    O, D = np.ascontiguousarray(O[:n]), np.ascontiguousarray(D[:n])
    assert n % 64 != 0 and n > 600
    raw = gpu_intersect(b, O, D).raw.cpu().numpy()
    bad = compare(raw, ob, O, D, rec)
    assert not bad, (world, bad)
    # entry and element: the one hitable they name, alone in an oracle world, answers the same t
    bad = check_identities(b, rec, SEED, O, D, raw, np.random.default_rng(SEED), samples=8)
    assert not bad, (world, bad)
    hits = raw[:, 7]
    assert (hits == rtmi.RTMI_HIT_PARALLELOGRAM).sum() > 50
    if world != "textured":
        assert (hits == rtmi.RTMI_HIT_TRIANGLE).sum() > 50


@pytest.mark.parametrize("world", ["sheets_4", "sheets_7_light", "mixed_list"])
def test_occluded_at_and_around_a_sheets_t(world):
    """t_max on, one ulp below and one above the t of the nearest surface and of the one behind it: rtmi_occluded equals
    the oracle's filtered answer and rtmi_intersect's."""
    fill = {"sheets_4": worlds.sheets(4), "sheets_7_light": worlds.sheets(7, True), "mixed_list": worlds.mixed_list(7)}[world]
    b, rec, ob = _query_world(fill)
    O, D = make_rays(ob, 5, n_family=100)
    t1 = oracle_t(ob, O, D)
    # the surface behind the nearest: the oracle's closest hit from just beyond it
    t2 = np.full(len(O), np.float32(np.inf), dtype=np.float32)
    for i in np.nonzero(np.isfinite(t1) & (t1 < 1e8))[0]:
        h, out, _ = ob.probe_hit(O[i], D[i], t_from=float(np.nextafter(t1[i], np.float32(np.inf))))
        if h and out[0] < 1e8:
            t2[i] = np.float32(out[0])
    assert np.isfinite(t2).sum() > 50
    for which, t in (("nearest", t1), ("behind", t2)):
        base = np.where(np.isfinite(t), t, np.float32(10.0)).astype(np.float32)
        for fam, tm in (("at", base), ("below", np.nextafter(base, np.float32(0))), ("above", np.nextafter(base, np.float32(np.inf)))):
            want = filtered(t1, tm)
            got, _ = gpu_occluded(b, O, D, tm)
            assert np.array_equal(got, want), (world, which, fam, np.nonzero(got != want)[0][:8])
            assert np.array_equal(gpu_filtered(b, O, D, tm), want), (world, which, fam)


def test_the_check_build_agrees_on_every_query():
    """librtmi_check1.so answers every query a second time with the plain scan: no disagreement on the sheets or the
    mixed list, whole or thin."""
    assert os.path.exists(CHECK_LIB), "librtmi_check1.so missing: run __graft_entry__.build() (make -C csrc check1)"
    env = dict(os.environ, RTMI_LIB_PATH=CHECK_LIB)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "tri_tasks_check.py")], env=env, cwd=ROOT,
                       stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-4000:]
    out = json.loads(r.stdout[r.stdout.index("{"):])
    assert len(out) == 11, sorted(out)
    for tag, v in out.items():
        assert v["re_done"] == v["rays"] > 0, (tag, v)
        assert v["disagreements"] == 0, (tag, v)
