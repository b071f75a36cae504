"""Next-event estimation on the GPU: rtmi_scene_lights, rtmi_direct_sample and rtmi_path_fold_direct against their numpy
restatements (tests/directlib.py) bit for bit, the loop with direct sampling leaving the paths of the plain loop alone,
and its radiance having rtmi_trace's expectation -- statistically on lamp_room and the Cornell box, analytically on the
furnace -- with less variance where small lights light the scene."""
import ctypes as C
import functools

import numpy as np
import pytest

import bouncelib
import common
import directlib as dl
import rtmi
from bouncelistlib import BAD_KINDS, make_bad
from parity import bits
from querylib import Recorder

pytestmark = pytest.mark.gpu
f32 = np.float32
SIZES = [1, 63, 64, 65, 4133]


@functools.lru_cache(maxsize=None)
def scene(name):
    """(committed scene, its Recorder, seed) of a scene program, of lamp_room, odd_lights or many_lights."""
    custom = {"lamp_room": dl.lamp_room, "odd_lights": dl.odd_lights_world, "many_lights": dl.many_lights_world()}
    if name in custom:
        b, rec = dl.build_custom(custom[name])
        return b, rec, dl.LAMP_ROOM_SEED
    seed = common.scene_seed(name)
    rec = Recorder(rtmi.SceneBuilder(seed))
    common.build_scene(rec, name, 1.0)
    rec.b.commit()
    return rec.b, rec, seed


def rays_of(name, n, seed=0):
    """n camera rays of the scene (its 32 x 32 frame, as many samples as n takes), float32 (n, 3) each."""
    b, _, _ = scene(name)
    O, D = dl.camera_rays(b, 32, 32, -(-n // 1024), 100 + seed)
    pick = np.random.default_rng(seed).permutation(len(O))[:n]
    return np.ascontiguousarray(O[pick]), np.ascontiguousarray(D[pick])


# ------------------------------------------------------------------ the table
@pytest.mark.parametrize("name,count", [("cornell_box", 1), ("furnace", 6), ("mixed", 1), ("sky_only", 0), ("odd_lights", 1),
                                        ("lamp_room", 2), ("many_lights", 1100)])
def test_table_is_the_restatement(name, count):
    b, rec, _ = scene(name)
    got, want = b.lights(), dl.table_of(rec)
    assert len(got) == count == rtmi.lib().rtmi_scene_light_count(b.h)
    assert dl.same_table(got, want), [k for k in rtmi.LIGHT_DTYPE.names if not np.array_equal(bits(got[k]), bits(want[k]))]
    if count:
        assert got["cdf"][-1] == 1 and (np.diff(got["cdf"]) >= 0).all()
    # a camera move leaves the table alone; a short or empty read is allowed
    b.camera_update(b.camera_get())
    assert dl.same_table(b.lights(), want)
    one = np.zeros((1,), rtmi.LIGHT_DTYPE)
    assert rtmi.lib().rtmi_scene_lights(b.h, one.ctypes.data_as(C.c_void_p), 1) == 0
    assert count == 0 or dl.same_table(one, want[:1])
    assert rtmi.lib().rtmi_scene_lights(b.h, None, 0) == 0 and rtmi.lib().rtmi_scene_lights(b.h, None, 1) < 0


def test_nested_light_is_the_only_table_light():
    b, rec, _ = scene("odd_lights")
    t = b.lights()
    assert t["entry"].tolist() == [6] and t["kind"].tolist() == [1] and t["emission"][0].tolist() == [2, 0, -4]


# ------------------------------------------------------------------ the step against the restatement
def _check_step(b, rec, ps, step_no, sample, what, **lst):
    tab, kinds = dl.table_of(rec), dl.mat_kinds_of(rec)
    cand = lst.get("list_in")
    if cand is not None:
        end = min(lst.get("n_list", len(cand)), lst.get("count_in", len(cand)) if lst.get("count_in") is not None else len(cand))
        cand = np.asarray(cand, dtype=np.int64)[:end]
    elif lst.get("n_list") is not None or lst.get("count_in") is not None:
        end = min(lst.get("n_list") if lst.get("n_list") is not None else len(ps.O),
                  lst.get("count_in") if lst.get("count_in") is not None else len(ps.O))
        cand = np.arange(end)
    want = dl.step(tab, kinds, ps.copy(), step_no, sample, cand)
    rc, got, intact = dl.device_step(b, ps, step_no, sample, **lst)
    assert rc == 0, rtmi.lib().rtmi_last_error()
    assert intact, (what, "a canary behind an array was overwritten")
    bad = dl.diff(got, want)
    assert bad == [], (what, bad, [np.flatnonzero((bits(getattr(got, k)) != bits(getattr(want, k))).reshape(len(ps.O), -1).any(1))[:6]
                                   for k in bad if k != "counts"])
    return want


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("name,n_steps", [("cornell_box", 1), ("cornell_box", 3), ("lamp_room", 1), ("lamp_room", 3)])
def test_step_is_the_restatement(name, n_steps, n):
    b, rec, seed = scene(name)
    O, D = rays_of(name, n, n_steps)
    ps, lst = dl.real_paths(b, O, D, seed + n, n_steps)
    rng = np.random.default_rng(n + n_steps)
    ps.flags = rng.integers(0, 4, n).astype(np.uint32)  # some previous vertices sampled; bit 1 is the caller's
    k = n_steps - 1
    sampled = 0
    for sample in (1, 0):
        w = _check_step(b, rec, ps, k, sample, "null list")
        sampled += int(w.counts[0]) - 3
        _check_step(b, rec, ps, k, sample, "the step's list", list_in=lst)
        _check_step(b, rec, ps, k, sample, "a count below n_list", list_in=lst, count_in=len(lst) // 2)
        _check_step(b, rec, ps, k, sample, "a null list cut by its count", count_in=n // 2)
        holes = lst.copy()
        holes[::3] = np.resize(np.array([n, n + 5, 0x80000000, 0xffffffff], np.uint32), len(holes[::3]))
        _check_step(b, rec, ps, k, sample, "entries >= n", list_in=holes)
        _check_step(b, rec, ps, k, sample, "a reversed list", list_in=lst[::-1].copy())
    if n >= 63:
        assert sampled > 0, "the case samples no light at all"


@pytest.mark.parametrize("n_steps", [1, 3])
def test_paths_not_stepped_by_this_step_are_cleared(n_steps):
    """Bad rays of every kind never step (the plain loop, all paths candidates), ended paths stop stepping, and a step
    count that is not this step's is no business of this call's: shadow direction, t_max and d_direct zeroed, the flag
    cleared, nothing else touched."""
    b, rec, seed = scene("cornell_box")
    n = 330
    O, D = rays_of("cornell_box", n, 9)
    for k, i in enumerate(range(0, n, 11)):
        make_bad(O, D, i, BAD_KINDS[k % len(BAD_KINDS)])
    ps, lst = dl.real_paths(b, O, D, seed, n_steps, compact=False)
    assert lst is None and (ps.steps[::11] == 0).all() and (ps.steps == n_steps).sum() > n // 10
    ps.flags[:] = 1
    ps.steps[5::13] += 1  # (a later step's count)
    for sample in (1, 0):
        w = _check_step(b, rec, ps, n_steps - 1, sample, "bad rays mixed in")
        off = ps.steps != n_steps
        assert (w.flags[off] == 0).all() and (w.SD[off] == 0).all() and (w.ST[off] == 0).all() and (w.DR[off] == 0).all()
        assert np.array_equal(bits(w.E[off]), bits(ps.E[off])) and np.array_equal(w.LS[off], ps.LS[off])


def test_a_table_beyond_the_lds_staging_is_searched_in_global_memory():
    b, rec, seed = scene("many_lights")
    assert len(b.lights()) == 1100 > 1024
    n = 4133
    O, D = rays_of("many_lights", n, 2)
    ps, lst = dl.real_paths(b, O, D, seed, 1)
    w = _check_step(b, rec, ps, 0, 1, "1100 lights")
    assert int(w.counts[0]) - 3 > n // 4
    _check_step(b, rec, ps, 0, 1, "1100 lights, listed", list_in=lst)


def test_a_list_longer_than_the_grid_is_walked_in_strides():
    """The grid is capped at 8 workgroups of 256 lanes per compute unit (direct_body.h: kDirectBlocksPerCu): with more
    candidates than that a wave takes further chunks by its number."""
    import torch
    b, rec, seed = scene("cornell_box")
    n = torch.cuda.get_device_properties(0).multi_processor_count * 8 * 256 + 4133
    O, D = rays_of("cornell_box", n, 8)
    ps, lst = dl.real_paths(b, O, D, seed, 1)
    w = _check_step(b, rec, ps, 0, 1, "beyond one round of the grid")
    assert int(w.counts[0]) - 3 > n // 2
    _check_step(b, rec, ps, 0, 1, "beyond one round of the grid, listed", list_in=lst[::-1].copy())


def test_no_counters_and_nothing_to_do():
    b, rec, seed = scene("cornell_box")
    O, D = rays_of("cornell_box", 65, 4)
    ps, lst = dl.real_paths(b, O, D, seed, 1)
    want = dl.step(dl.table_of(rec), dl.mat_kinds_of(rec), ps.copy(), 0, 1)
    want.counts = ps.counts.copy()
    rc, got, intact = dl.device_step(b, ps, 0, 1, counts=False)
    assert rc == 0 and intact and dl.diff(got, want) == []
    rc, got, intact = dl.device_step(b, ps, 0, 1, n_list=0)
    assert rc == 0 and intact and dl.diff(got, ps) == []
    rc, got, intact = dl.device_step(b, ps, 0, 1, list_in=lst, count_in=0)
    assert rc == 0 and intact and dl.diff(got, ps) == []


# ------------------------------------------------------------------ nothing else moves
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


def test_the_paths_of_the_direct_loop_are_the_plain_loop_s():
    import torch
    b, _, seed = scene("cornell_box")
    n, depth = 4133, 6
    O, D = rays_of("cornell_box", n, 5)
    p, ps, ph, _, _ = _loop(b, O, D, seed, depth, False)
    q, qs, qh, ls, ls0 = _loop(b, O, D, seed, depth, True)
    assert torch.equal(ps, qs) and torch.equal(p.steps, q.steps)
    assert torch.equal(p.origins.view(torch.int32), q.origins.view(torch.int32))
    assert torch.equal(p.directions.view(torch.int32), q.directions.view(torch.int32))
    dropped = 0
    for k in range(depth):
        made = (p.steps > k).cpu().numpy()  # the paths step k stepped: the layers of the others are never written
        assert np.array_equal(bits(p.attenuation[k].cpu().numpy())[made], bits(q.attenuation[k].cpu().numpy())[made])
        assert np.array_equal(ph[k].cpu().numpy()[made], qh[k].cpu().numpy()[made])
        pe, qe = bits(p.emitted[k].cpu().numpy())[made], bits(q.emitted[k].cpu().numpy())[made]
        assert ((qe == pe) | (qe == 0)).all()  # every emitted word is the plain loop's or +0.0f
        dropped += int((qe != pe).any(1).sum())
    assert dropped > 0 and not torch.equal(ls, ls0)
    assert q.direct is not None and q.occluded.shape == (depth, n) and q.flags.shape == (n,) and p.direct is None
    assert not torch.equal(p.rgb, q.rgb)


@pytest.mark.parametrize("name", ["cornell_box", "lamp_room"])
def test_depth_one_is_rtmi_trace(name):
    import torch
    b, _, seed = scene(name)
    O, D = rays_of(name, 1000, 6)
    q, qs, _, ls, ls0 = _loop(b, O, D, seed, 1, True)
    ts = rtmi.rng_states(seed, len(O))
    t = b.trace(torch.from_numpy(O).cuda(), torch.from_numpy(D).cuda(), ts, 1).check()
    assert torch.equal(t.rgb.view(torch.int32), q.rgb.view(torch.int32)) and torch.equal(ts, qs) and torch.equal(ls, ls0)


@pytest.mark.parametrize("name", ["sky_only", "spheres"])
@pytest.mark.parametrize("depth", [0, 1, 3, 8])
def test_without_table_lights_every_depth_is_rtmi_trace(name, depth):
    import torch
    b, _, seed = scene(name)
    assert len(b.lights()) == 0
    O, D = rays_of(name, 1000, 7)
    q, qs, _, ls, ls0 = _loop(b, O, D, seed, depth, True)
    ts = rtmi.rng_states(seed, len(O))
    t = b.trace(torch.from_numpy(O).cuda(), torch.from_numpy(D).cuda(), ts, depth).check()
    assert torch.equal(t.rgb.view(torch.int32), q.rgb.view(torch.int32)) and torch.equal(ts, qs)
    assert torch.equal(ls, ls0), "the light states were touched without a table light"


# ------------------------------------------------------------------ the fold
@pytest.mark.parametrize("n", [1, 65, 4133])
def test_fold_is_the_restatement_and_reduces_to_the_plain_fold(n):
    import torch
    rng = np.random.default_rng(n)
    L = 7
    E, A = rng.uniform(0, 2, (L, n, 3)).astype(f32), rng.uniform(0, 1, (L, n, 3)).astype(f32)
    Dk = rng.uniform(0, 3, (L, n, 3)).astype(f32)
    occ = rng.integers(0, 2, (L, n)).astype(np.uint8)
    dirs = rng.uniform(-1, 1, (n, 3)).astype(f32)
    dirs[::3] = 0
    dirs[1::9] = (-0.0, 0.0, -0.0)
    steps = rng.integers(0, L + 3, n).astype(np.int32)
    t = [torch.from_numpy(x).cuda() for x in (dirs, steps, E, A, Dk, occ)]
    got = rtmi.path_fold_direct(*t).cpu().numpy()
    assert np.array_equal(bits(got), bits(dl.fold_direct(dirs, steps, E, A, Dk, occ)))
    plain = rtmi.path_fold(*t[:4]).cpu().numpy()
    zero = rtmi.path_fold_direct(t[0], t[1], t[2], t[3], torch.zeros_like(t[4]), t[5]).cpu().numpy()
    shut = rtmi.path_fold_direct(t[0], t[1], t[2], t[3], t[4], torch.ones_like(t[5]).view(torch.bool)).cpu().numpy()
    assert np.array_equal(bits(zero), bits(plain)) and np.array_equal(bits(shut), bits(plain))
    assert n == 1 or not np.array_equal(bits(got), bits(plain))


# ------------------------------------------------------------------ the same expectation as Trace
LAMP_ROOM_SPP = 512  # the oracle's Trace on the CPU: 5 sqrt(2 var X / n) = 1.8 % of mean X at n = 2^19, 2.5 % at 2^18


@functools.lru_cache(maxsize=None)
def both_estimators(name, spp, depth):
    """(n, mean X, var X, mean Y, var Y) per channel in binary64: X rtmi_trace's radiance, Y the direct loop's, of the same
    32 x 32 x spp camera rays in the same run."""
    import torch
    b, _, seed = scene(name)
    O, D = dl.camera_rays(b, 32, 32, spp, 31)
    n = len(O)
    o, d = torch.from_numpy(O).cuda(), torch.from_numpy(D).cuda()
    X = b.trace(o, d, rtmi.rng_states(seed, n), depth).check().rgb.double()
    Y = b.trace_steps(o, d, rtmi.rng_states(seed + 1, n), depth, compact=True, direct=True,
                      light_states=rtmi.rng_states(seed + 1, n, first=n)).check().rgb.double()
    out = (n,) + tuple(v.cpu().numpy() for v in (X.mean(0), X.var(0, unbiased=True), Y.mean(0), Y.var(0, unbiased=True)))
    print("%s: n %d  mean X %s  var X %s  mean Y %s  var Y %s" % ((name,) + out))
    return out


def _same_expectation(name, spp, depth):
    n, mx, vx, my, vy = both_estimators(name, spp, depth)
    rhs = 5 * np.sqrt(vx / n + vy / n)
    print("%s: |mean X - mean Y| %s  5 sigma %s  cap %s" % (name, np.abs(mx - my), rhs, 0.02 * mx))
    assert (rhs <= 0.02 * mx).all(), "the test is not sharp: 5 sigma above 2 % of mean X"
    assert (np.abs(mx - my) <= rhs).all()


def test_lamp_room_has_trace_s_expectation():
    _same_expectation("lamp_room", LAMP_ROOM_SPP, 6)


def test_cornell_box_has_trace_s_expectation():
    _same_expectation("cornell_box", 256, 10)


def test_direct_sampling_lowers_the_variance_on_lamp_room():
    n, mx, vx, my, vy = both_estimators("lamp_room", LAMP_ROOM_SPP, 6)
    print("lamp_room: sum var Y / sum var X = %.4f" % (vy.sum() / vx.sum()))
    assert vy.sum() < vx.sum()


def test_furnace_sphere_paths_average_the_albedo():
    """Paths whose primary hit is the furnace's sphere: plain Trace gives exactly rho = 0.5; the direct loop's mean at depth
    4 is within 5 standard errors of it per channel."""
    import torch
    b, _, seed = scene("furnace")
    O, D = dl.camera_rays(b, 32, 32, 64, 17)
    o, d = torch.from_numpy(O).cuda(), torch.from_numpy(D).cuda()
    on_sphere = b.intersect(o, d).check().kind == rtmi.RTMI_HIT_SPHERE
    o, d = o[on_sphere].contiguous(), d[on_sphere].contiguous()
    n = len(o)
    assert n > 10000
    X = b.trace(o, d, rtmi.rng_states(seed, n), 4).check().rgb
    assert (X == 0.5).all()
    Y = b.trace_steps(o, d, rtmi.rng_states(seed, n), 4, compact=True, direct=True,
                      light_states=rtmi.rng_states(seed, n, first=n)).check().rgb.double()
    mean, se = Y.mean(0).cpu().numpy(), (Y.var(0, unbiased=True) / n).sqrt().cpu().numpy()
    print("furnace: n %d  mean %s  standard error %s" % (n, mean, se))
    assert (se > 0).all() and (np.abs(mean - 0.5) <= 5 * se).all()


# ------------------------------------------------------------------ the renderer
def test_render_rays_passes_direct_through():
    import torch
    b, _, seed = scene("cornell_box")
    r = rtmi.Renderer(b, 32, 32, 4, max_depth=5, post=False).init_rng()
    r.render_rays(direct=True)
    assert r.light_states.shape == (6, r.items) and int(r.samples.max()) == 4
    plain = rtmi.Renderer(b, 32, 32, 4, max_depth=5, post=False).init_rng()
    plain.render_rays()
    assert torch.equal(r.states, plain.states)  # the same paths
    assert torch.equal(r.budget_rays, plain.budget_rays) and not torch.equal(r.sum, plain.sum)
    assert torch.isfinite(r.sum).all() and getattr(plain, "light_states", None) is None
