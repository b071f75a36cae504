"""rtmi_occluded_list / SceneBuilder.occluded_list on the GPU.  The yardstick is rtmi_occluded itself on the same rays (held
to the CPU oracle by tests/test_gpu_occluded.py): a listed path gets its byte, every other byte is kept, the counts are
those of an rtmi_occluded call on the gathered candidate rays.  Then the oracle directly, the g8 fallback in list form, bad
rays among the candidates, a list eight times the resident grid, the direct loop with the list form against the loop
without it, and the check build's second answer for every candidate."""
import functools
import json
import os
import subprocess
import sys

import numpy as np
import pytest

if __name__ == "__main__":  # (the check build's process: no conftest has put the package on the path)
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "ray-tracing-cuda_amd"))

import common
import directlib as dl
import occludedlistlib as ol
import oraclelib
import rtmi
from bouncelistlib import BAD_KINDS, make_bad
from querylib import CUSTOM_WORLDS, F32_INF, SCENE_WORLDS, build, filtered, make_rays, oracle_t, textured_mesh, v3

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHECK_LIB = os.path.join(ROOT, "ray-tracing-cuda_amd", "lib", "librtmi_check1.so")
SIZES = (1, 63, 64, 65, 4133)  # chunk edges and a ragged last chunk


def two_meshes_mixed(b):
    """tests/test_gpu_occluded.py's world of two meshes, a triangle and spheres, restated."""
    textured_mesh(b)
    m = b.metal(v3(0.8, 0.8, 0.8), 0.2)
    b.sphere(v3(1.6, 0.3, 0.4), 0.5, m)
    b.triangle([v3(-2, -1, -1), v3(-1, 1.5, -1.5), v3(-2.5, 0.5, 0.5)], m)
    b.sphere(v3(-0.8, -0.7, 1.2), 0.35, m)


def build_world(name):
    if name != "occ_two_meshes_mixed":
        return build(name)
    CUSTOM_WORLDS[name] = two_meshes_mixed
    try:
        return build(name)
    finally:
        del CUSTOM_WORLDS[name]


def t_max_families(t, rng):
    """tests/test_gpu_occluded.py's families around the closest hits t (float32, +inf: none), restated."""
    n = len(t)
    base = np.where(np.isfinite(t), t, np.float32(10.0)).astype(np.float32)
    return {
        "none": None,
        "scaled": (base * rng.uniform(0.2, 2.0, n)).astype(np.float32),
        "log": np.exp(rng.uniform(np.log(1e-4), np.log(1e3), n)).astype(np.float32),
        "at_t": base,
        "below_t": np.nextafter(base, np.float32(0)).astype(np.float32),
        "above_t": np.nextafter(base, F32_INF).astype(np.float32),
        "specials": rng.choice(np.array([0, -1, np.nan, np.inf, 1e9, np.nextafter(np.float32(1e9), np.float32(0)), 1e-3,
                                         np.nextafter(np.float32(1e-3), np.float32(0))], dtype=np.float32), n),
    }


def closest_t(b, O, D):
    """float32 t of rtmi_intersect's closest hit per ray, +inf where there is none (only to place the t_max families)."""
    h = b.intersect(torch.from_numpy(O).cuda(), torch.from_numpy(D).cuda()).check()
    return np.where(h.kind.cpu().numpy() != rtmi.RTMI_HIT_NONE, h.t.cpu().numpy(), F32_INF).astype(np.float32)


# ------------------------------------------------------------------ 1. a listed ray gets rtmi_occluded's byte
@pytest.mark.parametrize("name", SCENE_WORLDS + sorted(CUSTOM_WORLDS) + ["occ_two_meshes_mixed"])
def test_a_listed_ray_gets_rtmi_occluded_s_byte_and_everything_else_is_kept(name):
    b, rec, ob, seed = build_world(name)
    O, D = make_rays(ob, 3000 + len(name), n_family=1040)  # (at least four families of 1040: enough for 4133)
    rng = np.random.default_rng(seed + 23)
    pick = rng.permutation(len(O))[:max(SIZES)]  # every family of rays in every prefix
    O, D = np.ascontiguousarray(O[pick]), np.ascontiguousarray(D[pick])
    fams = t_max_families(closest_t(b, O, D), rng)
    fallback = 0
    for n in SIZES:
        for fam, tm in fams.items():
            r = ol.Rays(O[:n], D[:n], None if tm is None else tm[:n])
            ref, ref_counts = ol.occluded(b, r)
            assert ref_counts[0] == 0 and set(np.unique(ref)) <= {0, 1}, (name, n, fam)
            for kind in ol.LIST_KINDS:
                lst, n_list, cnt = ol.make_list(kind, n, rng)
                counts = ol.check_list(b, r, ref, lst, n_list, cnt, (name, n, fam, kind))
                assert counts[0] == 0, (name, n, fam, kind)  # no abandoned search
                fallback += int(counts[1])
    print("%s: %d rays answered by the fallback over all lists" % (name, fallback))


def test_no_counters_and_nothing_to_do():
    b, rec, ob, seed = build("cornell_box")
    O, D = make_rays(ob, 5, n_family=40)
    r = ol.Rays(O, D, np.full(len(O), 300.0, np.float32))
    ref, _ = ol.occluded(b, r)
    rc, got, _, intact = ol.occluded_list(b, r, None, r.n, None, counts=False)  # a null d_counts: the stand-in words
    assert rc == 0 and intact and np.array_equal(got, ref)
    for lst, n_list in ((None, 0), (np.arange(4, dtype=np.uint32), 0)):
        rc, got, counts, intact = ol.occluded_list(b, r, lst, n_list, None)
        assert rc == 0 and intact and (got == ol.FILL).all() and not counts.any()
    empty = ol.Rays(O[:0], D[:0])
    rc, got, counts, intact = ol.occluded_list(b, empty, np.arange(4, dtype=np.uint32), 4, None)  # n == 0
    assert rc == 0 and intact and not counts.any()
    # through the binding: out=None starts as zeros, so unlisted paths read "clear"; out is updated in place
    idx = torch.arange(0, r.n, 2, dtype=torch.int32, device="cuda")
    q = b.occluded_list(rtmi.Paths(idx), r.o, r.d, r.tm).check()
    want = np.zeros(r.n, np.uint8)
    want[::2] = ref[::2]
    assert np.array_equal(q.raw.cpu().numpy(), want)
    out = torch.full((r.n,), 7, dtype=torch.uint8, device="cuda")
    q = b.occluded_list(rtmi.Paths(idx, torch.tensor([3], dtype=torch.int32, device="cuda")), r.o, r.d, r.tm, out=out)
    want = np.full(r.n, 7, np.uint8)
    want[:6:2] = ref[:6:2]
    assert q.raw.data_ptr() == out.data_ptr() and np.array_equal(out.cpu().numpy(), want)
    assert np.array_equal(b.occluded_list(None, r.o, r.d, r.tm).raw.cpu().numpy(), ref)  # None: the identity


# ------------------------------------------------------------------ 2. against the oracle directly
@pytest.mark.parametrize("name", ["spheres", "bunny"])
def test_listed_rays_match_the_oracle(name):
    """spheres: binary64 records, so t_max = float32(t) must keep a hit whose double t lies above it (the seed rounding of
    occlusion_seed); bunny: the mesh engine."""
    b, rec, ob, seed = build(name)
    O, D = make_rays(ob, 41, n_family=300)
    rng = np.random.default_rng(seed + 5)
    lst = rng.permutation(len(O))[:len(O) // 3].astype(np.uint32)
    t = np.full(len(O), F32_INF, dtype=np.float32)
    t[lst] = oracle_t(ob, O[lst], D[lst])
    base = np.where(np.isfinite(t), t, np.float32(5.0)).astype(np.float32)
    for fam, tm in (("none", None), ("at_t", base), ("below_t", np.nextafter(base, np.float32(0)).astype(np.float32)),
                    ("above_t", np.nextafter(base, F32_INF).astype(np.float32)),
                    ("scaled", (base * rng.uniform(0.2, 2.0, len(O))).astype(np.float32))):
        rc, got, counts, intact = ol.occluded_list(b, ol.Rays(O, D, tm), lst, len(lst), None)
        assert rc == 0 and intact and counts[0] == 0, (name, fam)
        want = np.full(len(O), ol.FILL, np.uint8)
        want[lst] = filtered(t[lst], None if tm is None else tm[lst])
        bad = np.flatnonzero(got != want)
        assert len(bad) == 0, (name, fam, len(bad), [(int(i), O[i].tolist(), D[i].tolist()) for i in bad[:8]])
        if fam == "at_t":
            assert want[lst].sum() > len(lst) // 8, (name, int(want[lst].sum()))  # the case is real


# ------------------------------------------------------------------ 3. the fallback
@pytest.mark.parametrize("with_sphere", [False, True])
def test_g8_world_in_list_form_is_answered_by_the_fallback(with_sphere):
    b = rtmi.SceneBuilder(9)
    ol.g8_world(b, with_sphere)
    b.commit()
    n = 256
    O, D, tm = ol.g8_rays(n)
    r = ol.Rays(O, D, tm)
    ref, ref_counts = ol.occluded(b, r)
    assert ref.all() and ref_counts[0] == 0 and ref_counts[1] > n // 2  # (test_gpu_occluded.py holds this to the oracle)
    rng = np.random.default_rng(3)
    for kind in ol.LIST_KINDS:
        lst, n_list, cnt = ol.make_list(kind, n, rng)
        counts = ol.check_list(b, r, ref, lst, n_list, cnt, kind)  # answers and counts equal the gathered call's
        at = ol.listed(n, lst, n_list, cnt)
        assert counts[1] <= len(at) and (counts[1] > 0) == (len(at) > 0), (kind, counts.tolist(), len(at))


# ------------------------------------------------------------------ 4. bad rays
@pytest.mark.parametrize("name", ["cornell_box", "bunny", "spheres"])
def test_bad_rays_among_the_candidates_answer_zero_and_change_no_other_answer(name):
    b, rec, ob, seed = build(name)
    O, D = make_rays(ob, 77, n_family=300)
    rng = np.random.default_rng(1)
    tm = (closest_t(b, O, D) * rng.uniform(0.5, 1.5, len(O))).astype(np.float32)
    tm[~np.isfinite(tm)] = 50.0
    ref, _ = ol.occluded(b, ol.Rays(O, D, tm))
    Ob, Db = O.copy(), D.copy()
    which = np.arange(len(O)) % 11 == 3
    for j, i in enumerate(np.flatnonzero(which)):
        make_bad(Ob, Db, i, BAD_KINDS[j % len(BAD_KINDS)])
    want_all = np.where(which, 0, ref).astype(np.uint8)
    assert ref[which].any(), name  # some of the rays made bad were occluded before
    r = ol.Rays(Ob, Db, tm)
    for kind in ("null_count", "subset_strays", "duplicates"):
        lst, n_list, cnt = ol.make_list(kind, len(O), rng)
        rc, got, counts, intact = ol.occluded_list(b, r, lst, n_list, cnt)
        assert rc == 0 and intact and counts[0] == 0, (name, kind)
        assert np.array_equal(got, ol.expect(want_all, len(O), lst, n_list, cnt)), (name, kind)
    # a list of the bad rays alone: every answer 0, and a list without them: rtmi_occluded's
    bad = np.flatnonzero(which).astype(np.uint32)
    rc, got, _, intact = ol.occluded_list(b, r, bad, len(bad), None)
    assert rc == 0 and intact and not got[which].any() and (got[~which] == ol.FILL).all(), name
    good = np.flatnonzero(~which).astype(np.uint32)
    rc, got, _, intact = ol.occluded_list(b, r, good, len(good), None)
    assert rc == 0 and intact and np.array_equal(got[~which], ref[~which]) and (got[which] == ol.FILL).all(), name


# ------------------------------------------------------------------ 5. a list longer than the grid
def test_four_million_shuffled_entries_are_walked_in_strides():
    """2^22 entries over 2^22 rays: eight times the 256 compute units x 2048 lanes that can be resident, so every wave takes
    further chunks by its number (the size of test_four_million_rays_against_intersect)."""
    b, rec, ob, seed = build("cornell_box")
    cam = ob.camera_get()
    n = 1 << 22
    g = torch.Generator(device="cuda").manual_seed(17)
    xy = torch.rand((n, 2), generator=g, device="cuda", dtype=torch.float32)
    c = torch.from_numpy(np.ascontiguousarray(cam[:4], dtype=np.float32)).cuda()
    o = c[0].expand(n, 3).contiguous()
    d = (c[1] + xy[:, :1] * c[2] + xy[:, 1:] * c[3] - c[0]).contiguous()
    t = b.intersect(o, d).check().t
    tm = (torch.where(torch.isfinite(t), t, torch.full_like(t, 100.0)) *
          (0.5 + torch.rand((n,), generator=g, device="cuda"))).contiguous()  # about half below the closest hit
    ref = b.occluded(o, d, tm).check()
    perm = torch.randperm(n, generator=g, device="cuda").to(torch.int32)
    out = torch.full((n,), ol.FILL, dtype=torch.uint8, device="cuda")
    q = b.occluded_list(rtmi.Paths(perm), o, d, tm, out=out).check()
    assert q.raw.data_ptr() == out.data_ptr()
    assert torch.equal(out, ref.raw), int((out != ref.raw).sum())
    assert torch.equal(q.counts, ref.counts)
    assert 0 < int(ref.raw.sum()) < n


# ------------------------------------------------------------------ 6. the loop
@functools.lru_cache(maxsize=None)
def loop_scene(name):
    if name == "lamp_room":
        return dl.build_custom(dl.lamp_room)[0], dl.LAMP_ROOM_SEED
    seed = common.scene_seed(name)
    b = rtmi.SceneBuilder(seed)
    common.build_scene(b, name, 1.0)
    b.commit()
    return b, seed


def _loop(b, O, D, seed, depth, compact, shadow):
    n = len(O)
    states = rtmi.rng_states(seed, n)
    ls = rtmi.rng_states(seed, n, first=n)
    st = b.trace_steps(torch.from_numpy(O).cuda(), torch.from_numpy(D).cuda(), states, depth, compact=compact, direct=True,
                       light_states=ls, shadow=shadow).check()
    return st, states, ls


@pytest.mark.parametrize("compact", [True, "full"])
@pytest.mark.parametrize("name", ["cornell_box", "lamp_room"])
def test_the_direct_loop_is_the_same_with_the_list_form(name, compact):
    """trace_steps(direct=True, shadow="list") against shadow="all": every field of Steps and both state tensors bit for
    bit.  (The emitted and attenuation stacks are allocated uninitialised and a step writes only the paths it steps, so
    their layers are compared where a step wrote them -- steps > k -- which is all that either loop defines.)"""
    b, seed = loop_scene(name)
    n, depth = 4133, 6
    O, D = dl.camera_rays(b, 32, 32, -(-n // 1024), 105)
    pick = np.random.default_rng(5).permutation(len(O))[:n]
    O, D = np.ascontiguousarray(O[pick]), np.ascontiguousarray(D[pick])
    p, ps, pl = _loop(b, O, D, seed, depth, compact, "all")
    q, qs, ql = _loop(b, O, D, seed, depth, compact, "list")
    i32 = torch.int32
    assert torch.equal(ps, qs) and torch.equal(pl, ql)
    assert torch.equal(p.rgb.view(i32), q.rgb.view(i32))
    assert torch.equal(p.steps, q.steps) and torch.equal(p.alive, q.alive) and torch.equal(p.flags, q.flags)
    assert torch.equal(p.origins.view(i32), q.origins.view(i32)) and torch.equal(p.directions.view(i32), q.directions.view(i32))
    assert torch.equal(p.direct.view(i32), q.direct.view(i32))
    assert torch.equal(p.occluded, q.occluded), int((p.occluded != q.occluded).sum())
    assert len(p.works) == len(q.works) == depth
    for k in range(depth):
        made = p.steps > k
        assert torch.equal(p.emitted[k].view(i32)[made], q.emitted[k].view(i32)[made]), k
        assert torch.equal(p.attenuation[k].view(i32)[made], q.attenuation[k].view(i32)[made]), k
        assert torch.equal(p.works[k][:2], q.works[k][:2]), k  # abandoned searches (0) and paths stepped
    assert 0 < int(q.occluded.sum()) and bool((q.direct != 0).any())  # shadow rays were shot, and some were blocked
    assert bool(q.rgb.isfinite().all())


# ------------------------------------------------------------------ 7. the check build
def test_every_candidate_agrees_with_the_unculled_answer():
    """librtmi_check1.so answers every candidate that is a path a second time with the unculled engine
    (rtmi_occluded_list_check_counts, only in that build): re-done equals the in-range candidates, no disagreement.  A
    diagnostic build, so it runs in a process of its own (this file, run as a script, RTMI_LIB_PATH pointing at it)."""
    assert os.path.exists(CHECK_LIB), "librtmi_check1.so missing: run __graft_entry__.build() (make -C csrc check1)"
    env = dict(os.environ, RTMI_LIB_PATH=CHECK_LIB)
    r = subprocess.run([sys.executable, os.path.abspath(__file__)], env=env, cwd=ROOT, stdout=subprocess.PIPE,
                       stderr=subprocess.PIPE, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-4000:]
    out = json.loads(r.stdout[r.stdout.index("{"):])
    assert sorted(out) == ["bunny", "cornell_box"], sorted(out)
    for name, v in out.items():
        assert v["lists"] == len(ol.LIST_KINDS), (name, v)
        assert v["re_done"] == v["in_range"] > 0, (name, v)
        assert v["disagreements"] == 0 and v["abandoned"] == 0, (name, v)
        assert 0 < v["occluded"] < v["in_range"], (name, v)


def _campaign():
    assert os.path.samefile(rtmi.LIB_PATH, CHECK_LIB), rtmi.LIB_PATH
    L = rtmi.lib()
    out = {}
    for name in ("cornell_box", "bunny"):  # a list world and a mesh world
        b, rec, ob, seed = build(name)
        O, D = make_rays(ob, 19, n_family=300)
        rng = np.random.default_rng(seed)
        t = closest_t(b, O, D)
        base = np.where(np.isfinite(t), t, np.float32(10.0)).astype(np.float32)
        r = ol.Rays(O, D, (base * rng.uniform(0.3, 3.0, len(O))).astype(np.float32))
        v = {"lists": 0, "in_range": 0, "re_done": 0, "disagreements": 0, "abandoned": 0, "occluded": 0}
        for kind in ol.LIST_KINDS:
            lst, n_list, cnt = ol.make_list(kind, r.n, rng)
            rc, got, counts, intact, check = ol.occluded_list(b, r, lst, n_list, cnt, lib=L, check=True)
            assert rc == 0 and intact, L.rtmi_last_error()
            at = ol.listed(r.n, lst, n_list, cnt)
            v["lists"] += 1
            v["in_range"] += len(at)
            v["re_done"] += int(check[0])
            v["disagreements"] += int(check[1])
            v["abandoned"] += int(counts[0])
            v["occluded"] += int((got[at] == 1).sum())
        out[name] = v
    print(json.dumps(out, indent=1))


if __name__ == "__main__":
    _campaign()
