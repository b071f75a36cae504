"""Sphere table lights on the GPU (rtmi_scene_light_kinds): the table against its restatement word for word, the step of
rtmi_direct_sample and rtmi_direct_sample_mis against tests/spherelightlib.py bit for bit -- on real paths of bulb_room,
on synthetic vertices inside, on and far from a sphere light, on a table beyond the LDS staging --, a scene that opted in
without an emissive sphere getting the bits it always got, the loops leaving the paths alone, a light that encloses the
scene changing nothing, and the loops' radiance having rtmi_trace's expectation and less variance on rooms lit by bulbs."""
import functools

import numpy as np
import pytest

import directlib as dl
import mislib as ml
import rtmi
import spherelightlib as sl
from abi_host import ERR_INVALID
from parity import bits

pytestmark = pytest.mark.gpu
f32 = np.float32
SIZES = [1, 63, 64, 65, 300]
KINDS = (rtmi.RTMI_HIT_NONE, rtmi.RTMI_HIT_SPHERE, rtmi.RTMI_HIT_TRIANGLE, rtmi.RTMI_HIT_PARALLELOGRAM,
         rtmi.RTMI_HIT_PARALLELEPIPED, rtmi.RTMI_HIT_MESH, rtmi.RTMI_HIT_SKY)
MODES = [False, True]  # rtmi_direct_sample, rtmi_direct_sample_mis

# name -> (scene program, what light_kinds is told: None for no call)
SCENES = {"bulb_room": (sl.bulb_room, True), "small_bulb_room": (sl.small_bulb_room, True), "enclosing": (sl.enclosing_light, True),
          "shared": (sl.shared_material_world, True), "rejected": (sl.rejected_spheres_world, True),
          "many_mixed": (sl.many_mixed_lights_world(), True), "odd_lights_3": (dl.odd_lights_world, True),
          "odd_lights_1": (dl.odd_lights_world, False), "odd_lights": (dl.odd_lights_world, None),
          "lamp_room_3": (dl.lamp_room, True), "lamp_room_1": (dl.lamp_room, False), "lamp_room": (dl.lamp_room, None),
          "bulb_room_1": (sl.bulb_room, False)}


@functools.lru_cache(maxsize=None)
def scene(name):
    """(committed scene, its Recorder, seed)."""
    fill, spheres = SCENES[name]
    b, rec = dl.build_custom(fill if spheres is None else sl.with_kinds(fill, spheres))
    return b, rec, dl.LAMP_ROOM_SEED


@functools.lru_cache(maxsize=None)
def tables(name):
    _, rec, _ = scene(name)
    return sl.table_of(rec, sl.FLAT | sl.SPHERES if SCENES[name][1] else sl.FLAT), dl.mat_kinds_of(rec)


def rays_of(name, n, seed=0):
    b, _, _ = scene(name)
    O, D = dl.camera_rays(b, 32, 32, -(-n // 1024), 100 + seed)
    pick = np.random.default_rng(seed).permutation(len(O))[:n]
    return np.ascontiguousarray(O[pick]), np.ascontiguousarray(D[pick])


def _cand(n, lst):
    cand = lst.get("list_in")
    if cand is not None:
        end = min(lst.get("n_list", len(cand)), lst.get("count_in", len(cand)) if lst.get("count_in") is not None else len(cand))
        return np.asarray(cand, dtype=np.int64)[:end]
    if lst.get("count_in") is not None:
        return np.arange(min(n, lst["count_in"]))
    return None


def _check_step(name, ps, step_no, sample, what, mis, **lst):
    b, _, _ = scene(name)
    tab, kinds = tables(name)
    want = sl.step(tab, kinds, ps.copy(), step_no, sample, _cand(len(ps.O), lst), mis=mis)
    rc, got, intact = ml.device_step(b, ps, step_no, sample, mis=mis, **lst)
    assert rc == 0, rtmi.lib().rtmi_last_error()
    assert intact, (what, "a canary behind an array was overwritten")
    bad = ml.diff(got, want)
    assert bad == [], (what, mis, bad, [np.flatnonzero((bits(getattr(got, k)) != bits(getattr(want, k))).reshape(len(ps.O), -1).any(1))[:6]
                                        for k in bad if k != "counts"])
    return want


def _every_list(name, ps, lst, k, sample, mis):
    n = len(ps.O)
    w = _check_step(name, ps, k, sample, "null list", mis)
    if lst is None:
        return w
    _check_step(name, ps, k, sample, "the step's list", mis, list_in=lst)
    _check_step(name, ps, k, sample, "a count below n_list", mis, list_in=lst, count_in=len(lst) // 2)
    _check_step(name, ps, k, sample, "a null list cut by its count", mis, count_in=n // 2)
    holes = lst.copy()
    holes[::3] = np.resize(np.array([n, n + 5, 0x80000000, 0xffffffff], np.uint32), len(holes[::3]))
    _check_step(name, ps, k, sample, "entries >= n", mis, list_in=holes)
    return w


# ------------------------------------------------------------------ 1. the table
@pytest.mark.parametrize("name", ["odd_lights_3", "bulb_room", "shared", "rejected", "many_mixed", "lamp_room_3"])
def test_the_table_is_the_restated_one_word_for_word(name):
    b, rec, _ = scene(name)
    got, want = b.lights(), tables(name)[0]
    assert dl.same_table(got, want), (got, want)
    assert got["cdf"][-1] == 1 and (np.diff(got["kind"] == 2) >= 0).all()  # the flat records first
    if name == "odd_lights_3":
        assert got["kind"].tolist() == [1, 2] and got["entry"].tolist() == [6, 0]
    if name == "bulb_room":
        assert got["kind"].tolist() == [2, 2] and got["entry"].tolist() == [6, 7]
    if name == "shared":
        assert got["kind"].tolist() == [0, 2, 2] and got["entry"].tolist() == [1, 2, 5]  # entry 5: a sphere in a nested list
    if name == "rejected":
        assert len(got) == 1 and got["entry"][0] == len(rec.entries()) - 1
    if name == "many_mixed":
        assert len(got) == 1100 and (got["kind"] == 2).sum() == 366 and (got["kind"][:734] != 2).all()
    if name == "lamp_room_3":
        assert dl.same_table(got, dl.table_of(rec)) and (got["kind"] != 2).all()


@pytest.mark.parametrize("with_call,without", [("odd_lights_1", "odd_lights"), ("lamp_room_1", "lamp_room")])
def test_without_the_option_the_table_is_what_it_was(with_call, without):
    b1, rec1, _ = scene(with_call)
    b0, rec0, _ = scene(without)
    assert dl.same_table(b1.lights(), b0.lights()) and dl.same_table(b0.lights(), dl.table_of(rec0))
    assert (b0.lights()["kind"] != 2).all()
    assert len(scene("bulb_room_1")[0].lights()) == 0


# ------------------------------------------------------------------ 9. the entry after commit
def test_after_commit_the_option_is_refused():
    b, _, _ = scene("bulb_room")
    before = b.lights()
    for kinds in (1, 3):
        assert sl.light_kinds_raw(b, kinds) == ERR_INVALID
        assert b"commit" in rtmi.lib().rtmi_last_error()
    with pytest.raises(rtmi.RtmiError):
        b.light_kinds(spheres=False)
    assert dl.same_table(b.lights(), before)


# ------------------------------------------------------------------ 2. the step on real paths
@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("n_steps", [1, 3])
@pytest.mark.parametrize("mis", MODES)
def test_step_is_the_restatement_on_real_paths(mis, n_steps, n):
    name = "bulb_room"
    b, _, seed = scene(name)
    O, D = rays_of(name, n, n_steps)
    p1, lst1 = dl.real_paths(b, O, D, seed + n, n_steps)
    ps = ml.PathState.of(p1)
    ps.flags = np.random.default_rng(n + n_steps).integers(0, 4, n).astype(np.uint32)  # bit 1 is the caller's
    k = n_steps - 1
    first = _every_list(name, ps, lst1, k, 1, mis)
    _every_list(name, ps, lst1, k, 0, mis)
    # the same paths one step on, with the flags and carries the sampling step left: WEIGH / DROP on real hits
    p2, lst2 = dl.real_paths(b, O, D, seed + n, n_steps + 1)
    nxt = ml.PathState.of(p2, carry=first.C)
    nxt.flags, nxt.LS = first.flags.copy(), first.LS.copy()
    counted = 0
    for sample in (1, 0):
        w = _every_list(name, nxt, lst2, k + 1, sample, mis)
        counted += int(w.counts[1]) - 5
    if n == 300:
        assert int(first.counts[0]) - 3 > n // 8, "the case samples nothing"
        assert (first.ST > 0).sum() > n // 16, "no valid sample among the paths"
        if n_steps == 1:
            assert counted > 0, "no flagged path hit a bulb"


# ------------------------------------------------------------------ 2. synthetic vertices and hits
def _synthetic():
    """Flagged and unflagged paths of the scene "shared" that step 0 stepped: vertices at the centre of, inside, on
    (d2c == R2), just outside and 1e4 R from the sphere light A (entry 2; it shares its material with the flat light of
    entry 1), inside and beside the sphere light B (entry 5), x hit records over every entry (3: an emissive sphere that
    is no table light) x every kind x elements, normals facing anywhere, carries of every sort."""
    tab, kinds = tables("shared")
    A, B = tab[1], tab[2]
    cA, RA, cB = A["p0"].astype(np.float64), float(A["e1"][0]), B["p0"].astype(np.float64)
    origins = [cA, cA + (0.1, 0.1, 0), cA + (RA, 0, 0), cA + (0, RA, 0), cA + (0, 0, -RA), (float(np.nextafter(f32(cA[0] + RA), f32(10))), cA[1], cA[2]),
               cA + (1e4 * RA, 0, 0), cA + (0, -0.6e4 * RA, 0.8e4 * RA), cB, cB + (0.1, 0, 0.2), (0, 0, 0), (0, 0.5, 3), (-4, 0, -4), (1, 3.9, 0)]
    entries = [-1, 0, 1, 2, 3, 4, 5, 6, 1000, 1 << 30, -(1 << 31)]
    rows = [(k, e, f) for e in entries for k in KINDS for f in (-1, 0, 1, 7)]
    n = len(rows) * len(origins)
    rng = np.random.default_rng(n)
    rep = np.tile(np.array(rows, dtype=np.int64), (len(origins), 1))
    O = np.repeat(np.array(origins, dtype=np.float64), len(rows), axis=0).astype(f32)
    H = np.zeros((n, 12), np.int32)
    H[:, 7], H[:, 8], H[:, 9] = rep[:, 0], rep[:, 1].astype(np.int32), rep[:, 2]
    H[:, 0] = np.resize(np.array([0.5, 2.0, 1e-3, 0.0, np.inf, np.nan], f32), n).view(np.int32)
    Nv = rng.normal(size=(n, 3))
    H[:, 3:6] = (Nv / np.linalg.norm(Nv, axis=1, keepdims=True)).astype(f32).view(np.int32)
    H[:, 6] = rng.integers(-1, len(kinds) + 1, n)
    H[rng.random(n) < 0.5, 6] = 0  # half the vertices Lambertian: they sample
    carries = np.array([(0, 1, 0, 1), (0.6, 0.8, 0, 0.5), (0, 1, 0, 0), (0, 1, 0, -0.5), (0, 1, 0, -0.0), (0, 1, 0, np.nan), (0, 1, 0, np.inf),
                        (1e30, 1e30, 1e30, 1e30), (0.3, -0.5, 0.81, 0.77), (0, 0, 1, 1e-30)], f32)
    Cw = carries[rng.integers(0, len(carries), n)]
    D = rng.normal(size=(n, 3)).astype(f32)
    D[rng.random(n) < 0.3] = 0
    E, Aa = rng.uniform(0.5, 4, (n, 3)).astype(f32), rng.uniform(0, 1, (n, 3)).astype(f32)
    LS = rng.integers(0, 1 << 32, (n, 6), dtype=np.uint64).astype(np.uint32)
    flags = np.where(rng.random(n) < 0.8, 1, 2).astype(np.uint32)
    ps = ml.PathState(O, D, H, np.ones(n, np.uint32), E, Aa, LS, flags=flags, carry=Cw)
    where = np.repeat(np.arange(len(origins)), len(rows))
    return ps, tab, where


@pytest.mark.parametrize("mis", MODES)
def test_synthetic_vertices_inside_on_and_far_from_a_sphere_light(mis):
    ps, tab, where = _synthetic()
    kinds = tables("shared")[1]
    assert tab["material"][0] == tab["material"][1]  # a flat light and a sphere light on one material
    kind, entry, flagged = ps.H[:, 7], ps.H[:, 8], (ps.flags & 1) != 0
    onA, onB, on3 = (kind == rtmi.RTMI_HIT_SPHERE) & (entry == 2), (kind == rtmi.RTMI_HIT_SPHERE) & (entry == 5), (kind == rtmi.RTMI_HIT_SPHERE) & (entry == 3)
    for sample in (0, 1):
        w = _check_step("shared", ps, 0, sample, "synthetic", mis)
        same = (bits(w.E) == bits(ps.E)).all(1)
        # a vertex at the centre of, inside or on A keeps what it finds on A; one outside is weighed or dropped
        assert onA[where <= 4].any() and same[onA & (where <= 4)].all()
        out = onA & flagged & (where >= 5)
        assert out.sum() > 20 and (~same[out]).any()
        if not mis:
            assert (w.E[out] == 0).all()
        else:
            assert ((np.abs(w.E[out]) <= np.abs(ps.E[out])) | np.isnan(w.E[out])).all()
        far = out & np.isin(where, (6, 7))
        assert far.any()
        assert same[onA & ~flagged].all() and same[on3].all()  # unflagged; an emissive sphere that is no table light
        assert same[onB & np.isin(where, (8, 9))].all() and (~same[onB & flagged & (where <= 7)]).any()
        # the flat light that shares A's material behaves as ever, and a SPHERE hit on its entry has no light
        assert same[(kind == rtmi.RTMI_HIT_SPHERE) & (entry == 1)].all()
        if sample:
            # SAMPLE: a vertex inside or on the light it picked gets the invalid outputs; far away the sample is valid
            smp = (w.flags & 1) != 0
            LS = ps.LS.copy()
            idx = np.flatnonzero(smp)
            j = np.full(len(ps.O), -1)
            j[idx] = np.searchsorted(tab["cdf"], dl.draw01(LS, idx), side="left")
            inA = smp & (j == 1) & (where <= 4)
            assert inA.sum() > 5 and (w.ST[inA] == 0).all() and (w.DR[inA] == 0).all() and (w.SD[inA] == 0).all()
            farA = smp & (j == 1) & np.isin(where, (6, 7))
            assert farA.sum() > 5 and (w.ST[farA] > 0).any()
            valid = w.ST > 0
            away = smp & (j >= 1) & valid
            Nn = ps.H[:, 3:6].view(f32)
            assert away.any() and ((Nn[away] * w.SD[away]).sum(1) > 0).all()  # never a sample behind the surface
            assert (np.abs((w.SD[valid].astype(np.float64) ** 2).sum(1) - 1) < 1e-5).all()
            # the state advanced by 3 draws for a flat light, by 2 + 2 trips for a sphere
            adv = (w.LS[:, 0] - ps.LS[:, 0]).astype(np.uint32) // np.uint32(362437)
            assert (adv[smp & (j == 0)] == 3).all() and (adv[smp & (j >= 1)] % 2 == 0).all() and (adv[smp & (j >= 1)] >= 4).all()
            assert (adv[~smp] == 0).all() and (adv[smp & (j >= 1)] > 4).any()


def test_unlisted_and_unstepped_paths_keep_every_word():
    name = "bulb_room"
    b, _, seed = scene(name)
    n = 300
    O, D = rays_of(name, n, 9)
    p1, lst = dl.real_paths(b, O, D, seed, 2, compact=False)
    ps = ml.PathState.of(p1)
    ps.flags[:] = 1
    ps.steps[5::13] += 1  # (a later step's count)
    for mis in MODES:
        for sample in (1, 0):
            w = _check_step(name, ps, 1, sample, "unstepped paths mixed in", mis)
            off = ps.steps != 2
            assert off.sum() > 20 and (w.flags[off] == 0).all() and (w.SD[off] == 0).all() and (w.DR[off] == 0).all()
            for k in ("C", "E", "LS", "SO"):
                assert np.array_equal(bits(getattr(w, k)[off]), bits(getattr(ps, k)[off])), k
            half = np.arange(0, n, 2, dtype=np.uint32)
            w = _check_step(name, ps, 1, sample, "every other path listed", mis, list_in=half)
            for k in ml.PathState.FIELDS:
                if k != "counts":
                    assert np.array_equal(bits(getattr(w, k)[1::2]), bits(getattr(ps, k)[1::2])), k


# ------------------------------------------------------------------ 3. a table beyond the LDS staging
@pytest.mark.parametrize("mis", MODES)
def test_a_table_beyond_the_lds_staging(mis):
    name = "many_mixed"
    b, _, seed = scene(name)
    tab, kinds = tables(name)
    assert len(tab) == 1100 > 1024
    n = 300
    O, D = rays_of(name, n, 2)
    p1, lst1 = dl.real_paths(b, O, D, seed, 1)
    ps = ml.PathState.of(p1)
    first = _check_step(name, ps, 0, 1, "1100 lights", mis)
    assert int(first.counts[0]) - 3 > n // 4
    _check_step(name, ps, 0, 1, "1100 lights, listed", mis, list_in=lst1)
    LS = ps.LS.copy()
    smp = np.flatnonzero(first.flags & 1)
    j = np.searchsorted(tab["cdf"], dl.draw01(LS, smp), side="left")
    assert (tab["kind"][j] == 2).any() and (tab["kind"][j] != 2).any() and (j >= 1024).any()
    # WEIGH / DROP against lights deep in the table: every sampled path is sent into a light of its own choosing
    nxt = first.copy()
    nxt.steps[:] = 2
    j = np.random.default_rng(4).integers(0, 1100, n)
    sph = tab["kind"][j] == 2
    nxt.H[:, 7] = np.where(sph, rtmi.RTMI_HIT_SPHERE, rtmi.RTMI_HIT_TRIANGLE)
    nxt.H[:, 8], nxt.H[:, 9], nxt.H[:, 6] = tab["entry"][j], 0, tab["material"][j]
    nxt.H[:, 0] = np.random.default_rng(5).uniform(0.01, 6, n).astype(f32).view(np.int32)
    nxt.E[:] = tab["emission"][j]
    w = _check_step(name, nxt, 1, 0, "1100 lights, weighed", mis)
    assert int(w.counts[1]) - 5 == int((first.flags & 1).sum())  # (every vertex lies on the floor or the box: outside)
    assert (sl.sphere_light_of_hit(tab, nxt.H)[sph] == j[sph]).all() and (ml.light_of_hit(tab, nxt.H)[~sph] == j[~sph]).all()


# ------------------------------------------------------------------ 4. opted in, no emissive sphere
@pytest.mark.parametrize("mis", MODES)
def test_opting_in_without_an_emissive_sphere_changes_no_bit(mis):
    b3, b1 = scene("lamp_room_3")[0], scene("lamp_room_1")[0]
    assert dl.same_table(b3.lights(), b1.lights())
    for n in SIZES:
        O, D = rays_of("lamp_room_1", n, 3)
        p1, lst = dl.real_paths(b1, O, D, dl.LAMP_ROOM_SEED + n, 2)
        ps = ml.PathState.of(p1)
        ps.flags[:] = np.random.default_rng(n).integers(0, 2, n)
        for sample in (1, 0):
            rc1, got1, ok1 = ml.device_step(b1, ps, 1, sample, list_in=lst, mis=mis)
            rc3, got3, ok3 = ml.device_step(b3, ps, 1, sample, list_in=lst, mis=mis)
            assert rc1 == 0 and rc3 == 0 and ok1 and ok3 and ml.diff(got1, got3) == []
            tab, kinds = tables("lamp_room_1")
            want = (ml.step if mis else dl.step)(tab, kinds, ps.copy(), 1, sample, lst)
            assert ml.diff(got3, want) == [] if mis else dl.diff(got3, want) == []


# ------------------------------------------------------------------ 5. 6. the loops
def _loop(b, O, D, seed, depth, direct):
    import torch
    n = len(O)
    o, d = torch.from_numpy(O).cuda(), torch.from_numpy(D).cuda()
    states = rtmi.rng_states(seed, n)
    ls = rtmi.rng_states(seed, n, first=n)
    ls0 = ls.clone()
    hits = []
    st = b.trace_steps(o, d, states, depth, each=lambda k, r: hits.append(r.hits.raw.clone()), compact=True,
                       direct=direct, light_states=ls if direct else None).check()
    return st, states, hits, ls, ls0


def test_the_paths_of_the_mis_loop_are_the_plain_loop_s():
    import torch
    name = "bulb_room"
    b, _, seed = scene(name)
    n, depth = 300, 6
    O, D = rays_of(name, n, 5)
    p, ps, ph, _, _ = _loop(b, O, D, seed, depth, False)
    q, qs, qh, ls, ls0 = _loop(b, O, D, seed, depth, "mis")
    t, tstates, _, lt, _ = _loop(b, O, D, seed, depth, True)
    assert torch.equal(ps, qs) and torch.equal(ps, tstates) and torch.equal(p.steps, q.steps) and torch.equal(p.steps, t.steps)
    assert torch.equal(p.origins.view(torch.int32), q.origins.view(torch.int32))
    assert torch.equal(p.directions.view(torch.int32), q.directions.view(torch.int32))
    changed = 0
    top = np.abs(tables(name)[0]["emission"]).max(0)
    for k in range(depth):
        made = (p.steps > k).cpu().numpy()
        assert np.array_equal(bits(p.attenuation[k].cpu().numpy())[made], bits(q.attenuation[k].cpu().numpy())[made])
        assert np.array_equal(ph[k].cpu().numpy()[made], qh[k].cpu().numpy()[made])
        pe, qe, te = (x.emitted[k].cpu().numpy()[made] for x in (p, q, t))
        assert ((qe >= 0) & (qe <= pe)).all() and ((te == 0) | (bits(te) == bits(pe))).all()
        changed += int((bits(qe) != bits(pe)).any(1).sum())
        # the weighted direct term is at most the attenuation times the brightest light
        assert (q.direct[k].cpu().numpy()[made] <= q.attenuation[k].cpu().numpy()[made] * top).all()
    assert changed > 0 and not torch.equal(ls, ls0)
    assert torch.equal(ls, lt) and torch.equal(q.flags, t.flags) and torch.equal(q.occluded, t.occluded)
    assert not torch.equal(p.rgb, q.rgb) and torch.isfinite(q.rgb).all() and torch.isfinite(t.rgb).all()


@pytest.mark.parametrize("depth", [1, 3, 8])
def test_a_light_that_encloses_the_scene_changes_nothing(depth):
    """Every vertex lies inside the one sphere light: every sample is invalid, every emission is kept, and the radiance
    of both loops is the plain loop's bit for bit."""
    import torch
    name = "enclosing"
    b, _, seed = scene(name)
    assert b.lights()["kind"].tolist() == [2]
    O, D = rays_of(name, 4096, depth)
    p, ps, _, _, _ = _loop(b, O, D, seed, depth, False)
    for direct in (True, "mis"):
        q, qs, _, ls, ls0 = _loop(b, O, D, seed, depth, direct)
        assert torch.equal(ps, qs)
        assert torch.equal(p.rgb.view(torch.int32), q.rgb.view(torch.int32)), direct
        assert not q.direct.any() and not q.occluded.any()
        for k in range(depth):
            made = (p.steps > k).cpu().numpy()
            assert np.array_equal(bits(p.emitted[k].cpu().numpy())[made], bits(q.emitted[k].cpu().numpy())[made])
        assert depth == 1 or not torch.equal(ls, ls0)  # the vertices did sample: the draws were taken
    assert (p.rgb > 0).any()


# ------------------------------------------------------------------ 7. 8. the same expectation as Trace, less variance
@functools.lru_cache(maxsize=None)
def estimators(name, spp, depth):
    """(n, {estimator: (mean, variance)}) per channel in binary64 of the same 32 x 32 x spp camera rays in the same run:
    "trace" rtmi_trace's radiance X, "direct" the direct=True loop's, "mis" the direct="mis" loop's."""
    import torch
    b, _, seed = scene(name)
    O, D = dl.camera_rays(b, 32, 32, spp, 31)
    n = len(O)
    o, d = torch.from_numpy(O).cuda(), torch.from_numpy(D).cuda()
    out = {}
    X = b.trace(o, d, rtmi.rng_states(seed, n), depth).check().rgb.double()
    out["trace"] = (X.mean(0).cpu().numpy(), X.var(0, unbiased=True).cpu().numpy())
    del X
    for k, (what, direct) in enumerate((("direct", True), ("mis", "mis"))):
        Y = b.trace_steps(o, d, rtmi.rng_states(seed + 1 + k, n), depth, compact=True, direct=direct,
                          light_states=rtmi.rng_states(seed + 1 + k, n, first=n)).check().rgb.double()
        out[what] = (Y.mean(0).cpu().numpy(), Y.var(0, unbiased=True).cpu().numpy())
        del Y
    for what, (m, v) in out.items():
        print("%s %s: n %d  mean %s  var %s" % (name, what, n, m, v))
    vx = out["trace"][1].sum()
    print("%s: sum var / sum var X: direct=True %.4f  mis %.4f" % (name, out["direct"][1].sum() / vx, out["mis"][1].sum() / vx))
    return n, out


@pytest.mark.parametrize("what", ["mis", "direct"])
def test_bulb_room_has_trace_s_expectation(what):
    """32 x 32 x 1024 camera rays (n = 2^20), depth 6; 5 sigma, and the test must be sharp: 5 sigma <= 2 % of mean X.
    The CPU oracle's Trace on bulb_room, 512^2 x 1 spp, depth 6, seed 77: mean X 1.160 / 1.155 / 0.988, var X 4.79 / 4.78 /
    3.45, so 5 sqrt(2 var X / n) / mean X is 1.30 / 1.31 / 1.30 % at n = 2^20: the cap holds while var Y <= 3.7 var X, and
    the theory expects var Y < var X."""
    n, est = estimators("bulb_room", 1024, 6)
    (mx, vx), (my, vy) = est["trace"], est[what]
    rhs = 5 * np.sqrt(vx / n + vy / n)
    print("bulb_room %s: |mean X - mean Y| %s  5 sigma %s  cap %s  (5 sigma / mean X %s)" % (what, np.abs(mx - my), rhs, 0.02 * mx, rhs / mx))
    assert n == 1 << 20
    assert (rhs <= 0.02 * mx).all(), "the test is not sharp: 5 sigma above 2 % of mean X"
    assert (np.abs(mx - my) <= rhs).all()


def test_both_loops_lower_the_variance_where_the_bulbs_are_small():
    """small_bulb_room (radii 0.5 and 0.25; the CPU oracle gives plain Trace a relative variance of about 29), 32 x 32 x
    256 camera rays, depth 6: the summed variance of the direct="mis" loop and of the direct=True loop are each below
    rtmi_trace's.  No ratio is set; the ratios are printed."""
    n, est = estimators("small_bulb_room", 256, 6)
    vx = est["trace"][1].sum()
    print("small_bulb_room: var / var X: mis %.5f  direct=True %.5f  (relative variance of X %s)"
          % (est["mis"][1].sum() / vx, est["direct"][1].sum() / vx, est["trace"][1] / est["trace"][0] ** 2))
    assert est["mis"][1].sum() < vx and est["direct"][1].sum() < vx


# ------------------------------------------------------------------ 10. the renderer
def test_render_rays_passes_mis_through_on_bulb_room():
    import torch
    b, _, seed = scene("bulb_room")
    depth, spp = 5, 3
    r = rtmi.Renderer(b, 32, 32, spp, max_depth=depth, post=False).init_rng()
    r.render_rays(direct="mis")
    assert r.light_states.shape == (6, r.items) and int(r.samples.max()) == spp and r.carry.shape == (r.items, 4)
    # the same loop by hand: camera_rays + trace_steps + sample_add
    m = rtmi.Renderer(b, 32, 32, spp, max_depth=depth, post=False).init_rng()
    ls = rtmi.rng_states(b.seed, m.items, first=m.items, device=m.device)
    for sample in range(spp):
        o, d = m.camera_rays(sample)
        st = b.trace_steps(o, d, m.states, depth, compact=True, direct="mis", light_states=ls)
        m.sample_add(sample, st.rgb, st.steps + st.alive.to(torch.int32))
    torch.cuda.synchronize()
    assert torch.equal(r.sum.view(torch.int32), m.sum.view(torch.int32)) and torch.equal(r.sq.view(torch.int32), m.sq.view(torch.int32))
    assert torch.equal(r.samples, m.samples) and torch.equal(r.budget_rays, m.budget_rays) and torch.equal(r.states, m.states)
    assert torch.equal(r.light_states, ls)
    plain = rtmi.Renderer(b, 32, 32, spp, max_depth=depth, post=False).init_rng()
    plain.render_rays()
    assert torch.equal(r.states, plain.states) and not torch.equal(r.sum, plain.sum) and torch.isfinite(r.sum).all()
