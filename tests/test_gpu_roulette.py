"""Russian roulette on the GPU: rtmi_path_roulette against its numpy restatement (tests/roulettelib.py) word for word -- on
real paths, with every kind of list, at draws steered onto the survival boundary --; the loop with it composing with the
compaction and reducing to the plain loop; rtmi_trace_roulette per path the loop's states, ray counts, counters and the
forward product of the loop's stacks, bit for bit; and both having rtmi_trace's expectation while they kill paths."""
import ctypes as C
import functools

import numpy as np
import pytest

import bouncelib
import common
import directlib as dl
import mislib as ml
import roulettelib as rl
import rtmi
import steerlib
from abi_host import ERR_DEPTH, _refused
from parity import bits
from rtmi import _abi, wavefront

pytestmark = pytest.mark.gpu
f32 = np.float32
CUSTOM = {"lamp_room": dl.lamp_room, "close_lamp_room": ml.close_lamp_room, "mesh_lamp_room": rl.mesh_lamp_room,
          "textured_room": rl.textured_room}
FUSED_SCENES = ["cornell_box", "lamp_room", "close_lamp_room", "spheres", "mixed", "sky_only", "furnace", "mesh_lamp_room",
                "textured_room"]


@functools.lru_cache(maxsize=None)
def scene(name):
    """(committed scene, seed)."""
    if name in CUSTOM:
        return dl.build_custom(CUSTOM[name])[0], dl.LAMP_ROOM_SEED
    seed = common.scene_seed(name)
    return common.build_scene(rtmi.SceneBuilder(seed), name, 1.0).commit(), seed


@functools.lru_cache(maxsize=None)
def host_rays(name, n):
    """n camera rays of the scene's 16 x 16 frame (as many samples as n takes), float32 (n, 3) each."""
    b, _ = scene(name)
    O, D = dl.camera_rays(b, 16, 16, -(-n // 256), 300 + n)
    pick = np.random.default_rng(n).permutation(len(O))[:n]
    return np.ascontiguousarray(O[pick]), np.ascontiguousarray(D[pick])


@functools.lru_cache(maxsize=None)
def rays_of(name, n):
    import torch
    O, D = host_rays(name, n)
    return torch.from_numpy(O).cuda(), torch.from_numpy(D).cuda()


# ------------------------------------------------------------------ 1. the step against its restatement
@functools.lru_cache(maxsize=None)
def paths_of(name, n, n_steps):
    """(RouletteState of n real paths after n_steps steps of the loop, with states of their own and throughputs on both
    sides of 1; the list the last step used)."""
    b, seed = scene(name)
    O, D = host_rays(name, n)
    ps, lst = dl.real_paths(b, O, D, seed, n_steps)
    S = bouncelib.host_states(rtmi.rng_states(seed + 2, n))
    T = np.random.default_rng(n + n_steps).uniform(0.02, 1.6, (n, 3)).astype(f32)
    return rl.RouletteState(ps.steps, ps.D, ps.A, S, T), lst


def _cand(n, lst):
    cand = lst.get("list_in")
    count = lst.get("count_in")
    if cand is not None:
        end = min(lst.get("n_list", len(cand)), len(cand) if count is None else count)
        return np.asarray(cand, dtype=np.int64)[:end]
    if lst.get("n_list") is not None or count is not None:
        return np.arange(min(n if lst.get("n_list") is None else lst["n_list"], n if count is None else count))
    return None


def _check_step(ps, step_no, first_step, p_min, what, **lst):
    want = rl.step(ps.copy(), step_no, first_step, p_min, _cand(len(ps.D), lst))
    if lst.get("counts") is False:  # a null d_counts: the call has nowhere to count, and the host's two words stay
        want.counts = ps.counts.copy()
    rc, got, intact = rl.device_step(ps, step_no, first_step, p_min, **lst)
    assert rc == 0, rtmi.lib().rtmi_last_error()
    assert intact, (what, "a canary around an array was overwritten")
    bad = rl.diff(got, want)
    assert bad == [], (what, bad, [np.flatnonzero((bits(getattr(got, k)) != bits(getattr(want, k))).reshape(len(ps.D), -1).any(1))[:6]
                                   for k in bad if k != "counts"])
    return want


@pytest.mark.parametrize("p_min", [2.0 ** -10, 0.05, 1.0])
@pytest.mark.parametrize("first_step", [0, 2])
@pytest.mark.parametrize("n", [1, 63, 64, 65, 257, 1000])
@pytest.mark.parametrize("name", ["cornell_box", "lamp_room", "mixed"])
def test_step_is_the_restatement_word_for_word(name, n, first_step, p_min):
    for n_steps in (2, 3):  # step 1: below first_step = 2; step 2: played
        ps, lst = paths_of(name, n, n_steps)
        k = n_steps - 1
        w = _check_step(ps, k, first_step, p_min, "null list")
        _check_step(ps, k, first_step, p_min, "the step's list", list_in=lst)
        _check_step(ps, k, first_step, p_min, "a device count shorter than the list", list_in=lst, count_in=len(lst) // 2)
        _check_step(ps, k, first_step, p_min, "a null list cut by its count", count_in=n // 2)
        _check_step(ps, k, first_step, p_min, "a host bound below the list", list_in=lst, n_list=len(lst) // 3)
        holes = lst.copy()
        holes[::3] = np.resize(np.array([n, n + 5, n, 0x80000000, 0xffffffff, n + 5], np.uint32), len(holes[::3]))
        _check_step(ps, k, first_step, p_min, "entries >= n, some of them twice", list_in=holes)
        _check_step(ps, k, first_step, p_min, "every other path unlisted", list_in=lst[::2].copy())
        _check_step(ps, k, first_step, p_min, "no counters", counts=False)
        if n >= 257:
            played = int(w.counts[0]) - 3
            assert (played > 0) == (k >= first_step), "the case plays nothing, or plays below first_step"
            if k >= first_step and p_min < 1:
                assert int(w.counts[1]) - 5 > 0, "the case kills nothing"


def test_unlisted_not_stepped_and_ended_paths_keep_every_bit():
    ps, lst = paths_of("lamp_room", 1000, 3)
    listed = lst[::2].copy()
    rc, got, intact = rl.device_step(ps, 2, 0, 0.05, list_in=listed)
    assert rc == 0 and intact
    n = len(ps.D)
    unlisted = np.setdiff1d(np.arange(n), listed.astype(np.int64))
    not_stepped = np.flatnonzero(ps.steps != 3)
    ended = np.flatnonzero((ps.steps == 3) & ~ps.D.any(1))
    assert len(unlisted) > 100 and len(not_stepped) > 0 and len(ended) > 0, "the case has no such path"
    rc, all_cand, intact = rl.device_step(ps, 2, 0, 0.05)  # every path a candidate
    assert rc == 0 and intact
    for who, run in ((unlisted, got), (not_stepped, all_cand), (ended, all_cand)):
        for k in ("steps", "D", "A", "S", "T"):
            a, was = getattr(run, k)[who], getattr(ps, k)[who]
            assert np.array_equal(np.ascontiguousarray(a).view(np.uint8), np.ascontiguousarray(was).view(np.uint8)), k
    assert (bits(got.T) != bits(ps.T)).any() and int(got.counts[0]) > 3


# ------------------------------------------------------------------ 2. the steered boundary
def _boundary_draws(p):
    """(x_lo, x_hi): the draw words of the largest CudaRandomFloat(0, 1) that is <= p and of the smallest above it (the
    draw is monotone in its word: tests/test_roulette_host.py)."""
    u = lambda x: steerlib.rng_01_of(np.array([x], dtype=np.uint64).astype(np.uint32))[0]
    lo, hi = 0, 0xffffffff
    assert u(lo) <= p < u(hi)
    while hi - lo > 1:
        mid = (lo + hi) // 2
        if u(mid) <= p:
            lo = mid
        else:
            hi = mid
    return lo, hi


@pytest.mark.parametrize("p,p_min", [(0.3, 0.05), (0.73, 0.05), (0.05, 0.05), (2.0 ** -10, 2.0 ** -10)])
def test_the_draw_that_is_p_survives_and_the_next_one_up_is_killed(p, p_min):
    """t = (p, p / 2, p / 4) exactly (the throughput is 1), so the survival probability is the chosen binary32 p -- or the
    floor, where the attenuation is made smaller still.  Lanes 0 and 63 of a wave, and lane 0 of the next, draw exactly p
    in one run (where p is a draw; 2^-10 is none: the largest draw below it) and the next draw above it in the other; every
    other lane draws 1/2."""
    n = 130
    p = f32(p)
    at_floor = float(p) == float(f32(p_min)) and p < 0.1
    a = np.array([p, p / f32(2), p / f32(4)], f32) * (f32(0.5) if at_floor else f32(1))  # (below the floor: q < p_min)
    A, D = np.tile(a, (n, 1)), np.tile(f32([0, 0, 1]), (n, 1))
    lanes = [0, 63, 64]
    x_lo, x_hi = _boundary_draws(p)
    u_of = lambda x: steerlib.rng_01_of(np.array([x], dtype=np.uint64).astype(np.uint32))[0]
    assert u_of(x_lo) <= p < u_of(x_hi) and x_hi == x_lo + 1
    assert p < 2.0 ** -9 or (u_of(x_lo) == p and u_of(x_hi) == np.nextafter(p, f32(2)))  # (p itself, and the next binary32 up)
    for x, survives in ((x_lo, True), (x_hi, False)):
        draws = np.full((n, 1), 0x80000000, np.uint64)
        draws[lanes, 0] = x
        ps = rl.RouletteState(np.full(n, 1), D, A, steerlib.state_for(draws), counts=(0, 0))
        want = _check_step(ps, 0, 0, p_min, "steered draw %#x" % x)
        for i in lanes:
            if survives:
                inv = f32(1) / p
                assert np.array_equal(bits(want.A[i]), bits((a * inv).astype(f32))) and want.D[i].tolist() == [0, 0, 1]
            else:
                assert not want.A[i].any() and not want.D[i].any() and not want.T[i].any()
        others_live = 0.5 <= float(p)
        killed = (0 if survives else 3) + (0 if others_live else n - 3)
        assert want.counts.tolist() == [n, killed]


# ------------------------------------------------------------------ 3. the loop composes
def _same_paths(a, b, depth):
    """Two Steps hold the same paths: rays, steps, radiance, and every layer a path reached."""
    import torch
    assert torch.equal(a.steps, b.steps) and torch.equal(a.alive, b.alive)
    assert np.array_equal(bits(a.directions.cpu().numpy()), bits(b.directions.cpu().numpy()))
    assert np.array_equal(bits(a.origins.cpu().numpy()), bits(b.origins.cpu().numpy()))
    assert np.array_equal(bits(a.rgb.cpu().numpy()), bits(b.rgb.cpu().numpy()))
    steps = a.steps.cpu().numpy()
    for k in range(depth):
        m = steps > k
        for x, y in ((a.emitted, b.emitted), (a.attenuation, b.attenuation)):
            assert np.array_equal(bits(x[k].cpu().numpy()[m]), bits(y[k].cpu().numpy()[m])), k


@pytest.mark.parametrize("name", ["cornell_box", "lamp_room"])
def test_compacted_loop_with_roulette_is_the_uncompacted_one(name):
    import torch
    b, seed = scene(name)
    o, d = rays_of(name, 1000)
    depth = 12
    sc, states_c, rule_c, killed_c = rl.loop_of(b, o, d, seed, depth, 0, 0.05, compact=True)
    su, states_u, rule_u, killed_u = rl.loop_of(b, o, d, seed, depth, 0, 0.05, compact=False)
    _same_paths(sc, su, depth)
    assert torch.equal(states_c, states_u) and np.array_equal(killed_c, killed_u)
    assert rule_c.counts.tolist() == rule_u.counts.tolist() and int(rule_c.counts[1]) == int(killed_c.sum()) > 0
    assert np.array_equal(bits(rule_c.throughput.cpu().numpy()), bits(rule_u.throughput.cpu().numpy()))
    # a killed path is an ended one for the fold: its radiance is its stacks' fold like anyone's
    want = bouncelib.fold(sc.directions.cpu().numpy(), sc.steps.cpu().numpy(), sc.emitted.cpu().numpy(), sc.attenuation.cpu().numpy())
    assert np.array_equal(bits(sc.rgb.cpu().numpy()), bits(want))
    assert not sc.rgb.cpu().numpy()[killed_c].any()


@pytest.mark.parametrize("compact", [False, True])
@pytest.mark.parametrize("name", ["cornell_box", "lamp_room"])
def test_first_step_at_the_depth_is_the_plain_loop(name, compact):
    import torch
    b, seed = scene(name)
    o, d = rays_of(name, 1000)
    depth = 6
    for first_step in (depth, depth - 1):  # (the last step is never played: first_step = depth - 1 plays nothing either)
        sr, states_r, rule, killed = rl.loop_of(b, o, d, seed, depth, first_step, 0.05, compact=compact)
        s0 = rtmi.rng_states(seed, 1000)
        sp = b.trace_steps(o, d, s0, depth, compact=compact).check()
        _same_paths(sr, sp, depth)
        assert torch.equal(states_r, s0) and rule.counts.tolist() == [0, 0] and not killed.any()
        t = b.trace(o, d, rtmi.rng_states(seed, 1000), depth).check()
        assert np.array_equal(bits(sr.rgb.cpu().numpy()), bits(t.rgb.cpu().numpy()))


def test_roulette_with_direct_light_leaves_the_direct_layers_unscaled():
    """With direct="mis" the roulette plays behind the step's direct sampling: D[k] is formed from the unscaled A[k], so the
    direct stack of the loop with roulette equals the plain mis loop's on every layer up to a path's first roulette."""
    b, seed = scene("lamp_room")
    o, d = rays_of("lamp_room", 1000)
    depth, first = 8, 3
    sr, _, rule, killed = rl.loop_of(b, o, d, seed, depth, first, 0.05, direct="mis")
    sp = b.trace_steps(o, d, rtmi.rng_states(seed, 1000), depth, compact=True, direct="mis",
                       light_states=rtmi.rng_states(seed, 1000, first=1000)).check()
    for k in range(first + 1):  # (step `first` itself samples before it plays)
        m = (sr.steps.cpu().numpy() > k) & (sp.steps.cpu().numpy() > k)
        assert np.array_equal(bits(sr.direct[k].cpu().numpy()[m]), bits(sp.direct[k].cpu().numpy()[m])), k
    assert int(rule.counts[0]) > 0 and killed.any()
    want = dl.fold_direct(sr.directions.cpu().numpy(), sr.steps.cpu().numpy(), sr.emitted.cpu().numpy(), sr.attenuation.cpu().numpy(),
                          sr.direct.cpu().numpy(), sr.occluded.cpu().numpy())
    assert np.array_equal(bits(sr.rgb.cpu().numpy()), bits(want))


# ------------------------------------------------------------------ 4. the fused kernel against the loop
def check_against_the_loop(name, n, depth, first_step, p_min=0.05):
    import torch
    b, seed = scene(name)
    o, d = rays_of(name, n)
    s = seed + n + depth
    st, states, rule, killed = rl.loop_of(b, o, d, s, depth, first_step, p_min)
    want = rl.expected_radiance(st, killed)
    got = rl.fused(b, o, d, rtmi.rng_states(s, n), depth, first_step, p_min)
    assert got["intact"], "a canary around an output was overwritten"
    steps, alive = st.steps.cpu().numpy(), st.alive.cpu().numpy()
    # the one documented difference: a bad scattered ray -- alive by its direction, yet the loop no longer steps it
    excluded = alive & (steps < depth)
    assert excluded.sum() * 1000 <= n, (name, n, depth, int(excluded.sum()))
    ok = ~excluded
    bad = np.flatnonzero((bits(got["rgb"]) != bits(want)).any(1) & ok)
    assert bad.size == 0, (name, n, depth, first_step, bad[:8], got["rgb"][bad[:4]], want[bad[:4]])
    assert np.array_equal(got["states"][:, ok], states.cpu().numpy()[:, ok]), "the path states are not the loop's"
    assert np.array_equal(got["rays"][ok], (steps + alive)[ok])
    played, dead = (0, 0) if rule.counts is None else (int(x) for x in rule.counts.cpu())
    if not excluded.any():
        assert got["counts"].tolist() == [played, dead] and dead == int(killed.sum())
    assert got["work"][0] == 0 and got["work"][1] == got["rays"].sum()
    return st, got, killed


@pytest.mark.parametrize("first_step", [0, 3])
@pytest.mark.parametrize("depth", [0, 1, 2, 6, 50])
@pytest.mark.parametrize("n", [1, 64, 65, 1000])
@pytest.mark.parametrize("name", FUSED_SCENES)
def test_fused_is_the_loop_bit_for_bit(name, n, depth, first_step):
    st, got, killed = check_against_the_loop(name, n, depth, first_step)
    if depth == 0:
        assert not got["rgb"].any() and got["counts"].tolist() == [0, 0]
    if depth <= first_step + 1:
        assert got["counts"].tolist() == [0, 0]  # (nothing is played behind the last vertex)
    if n == 1000 and depth >= 6 and name in ("cornell_box", "lamp_room", "close_lamp_room"):  # (closed rooms: paths go deep)
        assert got["counts"][0] > 0 and killed.any(), "the case plays or kills nothing"
        assert not got["rgb"][killed].any()
    if n == 1000 and depth >= 2 and first_step == 0 and name == "furnace":
        assert got["counts"][0] > 0


@pytest.mark.parametrize("p_min", [2.0 ** -10, 0.25, 1.0])
def test_fused_floors(p_min):
    st, got, killed = check_against_the_loop("lamp_room", 1000, 12, 1, p_min)
    assert got["counts"][0] > 0
    if p_min == 1.0:  # p = 1: u <= 1 always: everything survives, nothing is scaled
        assert got["counts"][1] == 0


@pytest.mark.parametrize("name", ["cornell_box", "mesh_lamp_room"])
def test_first_step_at_the_depth_is_rtmi_trace(name):
    import torch
    b, seed = scene(name)
    n, depth = 1000, 6
    o, d = rays_of(name, n)
    s0 = rtmi.rng_states(seed, n)
    t = b.trace(o, d, s0, depth, count_rays=True).check()
    got = rl.fused(b, o, d, rtmi.rng_states(seed, n), depth, depth, 0.05)
    assert got["intact"] and got["counts"].tolist() == [0, 0]
    assert np.array_equal(got["states"], s0.cpu().numpy()) and np.array_equal(got["rays"], t.rays.cpu().numpy())
    sp = b.trace_steps(o, d, rtmi.rng_states(seed, n), depth, compact=True).check()
    want = rl.forward(~sp.alive.cpu().numpy(), sp.steps.cpu().numpy(), sp.emitted.cpu().numpy(), sp.attenuation.cpu().numpy())
    assert np.array_equal(bits(got["rgb"]), bits(want))
    # the fold of the same stacks: the other rounding order of the same product
    assert np.allclose(got["rgb"], t.rgb.cpu().numpy(), rtol=2 * (depth + 1) * 2.0 ** -24, atol=0)


def test_bad_rays_are_left_out():
    import torch
    name, n, depth = "lamp_room", 300, 6
    b, seed = scene(name)
    o, d = (t.clone() for t in rays_of(name, n))
    bad = np.array([0, 5, 63, 64, 127, 299])
    o[bad[0::2], 1] = float("nan")
    d[bad[1::2]] = 0.0
    good = np.setdiff1d(np.arange(n), bad)
    s0 = rtmi.rng_states(seed, n)
    got = rl.fused(b, o, d, s0, depth, 0, 0.05)
    assert got["intact"]
    assert not got["rgb"][bad].any() and not got["rays"][bad].any()
    assert np.array_equal(got["states"][:, bad], s0.cpu().numpy()[:, bad])
    ref = rl.fused(b, o[good].contiguous(), d[good].contiguous(), s0[:, good].contiguous(), depth, 0, 0.05)
    assert np.array_equal(bits(got["rgb"][good]), bits(ref["rgb"])) and np.array_equal(got["rays"][good], ref["rays"])
    assert np.array_equal(got["states"][:, good], ref["states"]) and got["counts"].tolist() == ref["counts"].tolist()
    assert torch.isnan(o).any()


def test_depth_outside_its_range_and_python_refusals():
    b, seed = scene("lamp_room")
    o, d = rays_of("lamp_room", 64)
    s = rtmi.rng_states(seed, 64)
    for depth in (-1, rtmi.MAX_DEPTH + 1):
        a = _abi.TraceRouletteArgs()
        a.size, a.n, a.max_depth, a.p_min = C.sizeof(_abi.TraceRouletteArgs), 64, depth, 0.05
        a.d_origins, a.d_dirs, a.d_states = o.data_ptr(), d.data_ptr(), s.data_ptr()
        a.d_radiance = a.d_work = 16
        assert _refused(rtmi.lib().rtmi_trace_roulette(b.h, C.byref(a), None), b"depth", ERR_DEPTH)
        with pytest.raises(rtmi.RtmiError):
            b.trace_roulette(o, d, s, depth)
    with pytest.raises(rtmi.RtmiError):
        b.trace_roulette(o, d, s, 4, p_min=0.0)
    with pytest.raises(rtmi.RtmiError):
        b.trace_roulette(o, d, s[:, :32], 4)
    r = b.trace_roulette(o[:0], d[:0], s[:, :0].contiguous(), 4)  # launches nothing
    assert r.rgb.shape == (0, 3) and r.counts.tolist() == [0, 0]
    f = b.trace_roulette(o, d, s, 12, first_step=0, count_rays=True).check()
    assert isinstance(f, wavefront.TraceRoulette) and f.total_rays() == int(f.rays.sum()) and int(f.counts[0]) > 0


# ------------------------------------------------------------------ 5. the expectation
def _report(name, what, n, mx, vx, my, vy, rays_x, rays_y, counts):
    rhs = 5 * np.sqrt(vx / n + vy / n)
    print("%s %s: n %d  mean X %s  mean Y %s  |diff| %s  5 sigma %s  cap %s  var Y / var X %.4f  queries per path %.3f -> %.3f  "
          "played %d  killed %d" % (name, what, n, mx, my, np.abs(mx - my), rhs, 0.02 * mx, vy.sum() / vx.sum(), rays_x, rays_y,
                                    counts[0], counts[1]))
    return rhs


@functools.lru_cache(maxsize=None)
def plain(name, spp, depth):
    """rtmi_trace on the 32 x 32 x spp camera rays of the scene: (o, d, n, mean, variance, queries per path)."""
    import torch
    b, seed = scene(name)
    O, D = dl.camera_rays(b, 32, 32, spp, 31)
    o, d = torch.from_numpy(O).cuda(), torch.from_numpy(D).cuda()
    n = len(O)
    t = b.trace(o, d, rtmi.rng_states(seed, n), depth, count_rays=True).check()
    X = t.rgb.double()
    return o, d, n, X.mean(0).cpu().numpy(), X.var(0, unbiased=True).cpu().numpy(), float(t.rays.double().mean())


def _same_expectation(name, spp, depth, what, first_step):
    """The method of tests/test_gpu_direct_mis.py: the means of two independent runs over the same n rays differ by at most
    5 sigma of their difference, and the test is sharp -- 5 sigma is at most 2 % of the mean."""
    b, seed = scene(name)
    o, d, n, mx, vx, rays_x = plain(name, spp, depth)
    if what == "fused":
        f = b.trace_roulette(o, d, rtmi.rng_states(seed + 1, n), depth, first_step=first_step, count_rays=True).check()
        Y, rays_y, counts = f.rgb.double(), float(f.rays.double().mean()), f.counts.tolist()
    else:
        rule = wavefront.Roulette(first_step)
        st = b.trace_steps_roulette(o, d, rtmi.rng_states(seed + 2, n), depth, rule, compact=True, direct="mis",
                                    light_states=rtmi.rng_states(seed + 2, n, first=n)).check()
        Y, rays_y, counts = st.rgb.double(), float((st.steps + st.alive).double().mean()), rule.counts.tolist()
    my, vy = Y.mean(0).cpu().numpy(), Y.var(0, unbiased=True).cpu().numpy()
    rhs = _report(name, what, n, mx, vx, my, vy, rays_x, rays_y, counts)
    assert counts[1] > 0 and rays_y < rays_x, "no path was killed, or the paths did not get shorter: the test shows nothing"
    assert (rhs <= 0.02 * mx).all(), "the test is not sharp: 5 sigma above 2 % of mean X"
    assert (np.abs(mx - my) <= rhs).all()


@pytest.mark.parametrize("what", ["fused", "mis_loop"])
def test_lamp_room_has_trace_s_expectation(what):
    _same_expectation("lamp_room", 512, 50, what, 3)


@pytest.mark.parametrize("what", ["fused", "mis_loop"])
def test_cornell_box_has_trace_s_expectation(what):
    _same_expectation("cornell_box", 256, 50, what, 3)


@pytest.mark.parametrize("what", ["fused", "mis_loop"])
def test_furnace_sphere_paths_keep_the_albedo(what):
    """Paths whose primary hit is the furnace's sphere, at depth 50: plain Trace gives exactly rho = 0.5 (closed form), and
    roulette from the first vertex on -- survival probability 0.5, survivors weighted 2 -- must not move the mean: within
    5 standard errors of 0.5 per channel."""
    import torch
    b, seed = scene("furnace")
    O, D = dl.camera_rays(b, 32, 32, 64, 17)
    o, d = torch.from_numpy(O).cuda(), torch.from_numpy(D).cuda()
    on_sphere = b.intersect(o, d).check().kind == rtmi.RTMI_HIT_SPHERE
    o, d = o[on_sphere].contiguous(), d[on_sphere].contiguous()
    n = len(o)
    assert n > 10000
    t = b.trace(o, d, rtmi.rng_states(seed, n), 50, count_rays=True).check()
    assert (t.rgb == 0.5).all()
    if what == "fused":
        f = b.trace_roulette(o, d, rtmi.rng_states(seed + 1, n), 50, first_step=0, count_rays=True).check()
        Y, rays_y, counts = f.rgb.double(), float(f.rays.double().mean()), f.counts.tolist()
    else:
        rule = wavefront.Roulette(0)
        st = b.trace_steps_roulette(o, d, rtmi.rng_states(seed + 2, n), 50, rule, compact=True, direct="mis",
                                    light_states=rtmi.rng_states(seed + 2, n, first=n)).check()
        Y, rays_y, counts = st.rgb.double(), float((st.steps + st.alive).double().mean()), rule.counts.tolist()
    mean, se = Y.mean(0).cpu().numpy(), (Y.var(0, unbiased=True) / n).sqrt().cpu().numpy()
    print("furnace %s: n %d  mean %s  standard error %s  queries per path %.3f -> %.3f  played %d  killed %d"
          % (what, n, mean, se, float(t.rays.double().mean()), rays_y, counts[0], counts[1]))
    assert counts[1] > 0 and rays_y < float(t.rays.double().mean())
    assert (se > 0).all() and (np.abs(mean - 0.5) <= 5 * se).all()
