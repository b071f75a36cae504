"""rtmi_bounce / rtmi_path_fold / SceneBuilder.trace_steps on the GPU: every step against the oracle's Hit, Scatter and
Emit, the composed loop against the oracle's Trace and against rtmi_trace, the device fold against the numpy fold
(tests/bouncelib.py, held to hand-worked cases by tests/test_bounce_host.py), and the edges -- all bit for bit."""
import ctypes as C
import functools

import numpy as np
import pytest

import common
import oraclelib
import rtmi
from abi_host import ERR_INVALID, OK
from bouncelib import dev, dev_states, fold, hit_point, host_states, oracle_trace, sky_emit, world
from parity import bits
from querylib import CUSTOM_WORLDS, SCENE_WORLDS, compare, glm_normalize

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

WORLDS = SCENE_WORLDS + sorted(CUSTOM_WORLDS)
DEPTHS = (0, 1, 8, 50)
# Worlds in which no path can be alive at step 2, whatever the code does.  furnace: the only scatterer is one convex
# Lambertian sphere inside an enclosure of lights, so a path scatters once at most and its second query ends on a light.
# quilt_3: three small patches in front of Sky; of the 256 rays four scatter at all, and none of those finds a second patch.
SHORT_WORLDS = ("furnace", "quilt_3")
CANARY = np.float32(-7.25)
CANARY_HIT = 0x5a5a5a5a


def steppable(O, D):
    """The rays a step takes: finite, and a direction that normalises to a finite non-zero vector."""
    with np.errstate(all="ignore"):
        u = glm_normalize(D)
    return np.isfinite(O).all(1) & np.isfinite(D).all(1) & (D != 0).any(1) & np.isfinite(u).all(1) & (u != 0).any(1)


class Step:
    """One rtmi_bounce call on device copies of (O, D, states (n, 6)), canaries in every output, everything read back."""

    def __init__(self, b, O, D, states, steps=None, hits=True, count=True, stream=None):
        n = len(O)
        self.o, self.d, self.st = dev(O), dev(D), dev_states(states)
        em = torch.full((n, 3), float(CANARY), dtype=torch.float32, device="cuda")
        at = torch.full((n, 3), float(CANARY), dtype=torch.float32, device="cuda")
        raw = torch.full((n, 12), CANARY_HIT, dtype=torch.int32, device="cuda") if hits else False
        cnt = dev(np.zeros(n, np.int32) if steps is None else steps, np.int32) if count else None
        if stream is None:
            self.r = b.bounce(self.o, self.d, self.st, emitted=em, attenuation=at, hits=raw, steps=cnt)
        else:
            stream.wait_stream(torch.cuda.current_stream())  # (the copies and canaries above were enqueued there)
            with torch.cuda.stream(stream):
                self.r = b.bounce(self.o, self.d, self.st, emitted=em, attenuation=at, hits=raw, steps=cnt)

    def read(self):
        r = self.r.check()
        self.O, self.D, self.S = self.o.cpu().numpy(), self.d.cpu().numpy(), host_states(self.st)
        self.E, self.A = r.emitted.cpu().numpy(), r.attenuation.cpu().numpy()
        self.raw = None if r.hits is None else r.hits.raw.cpu().numpy()
        self.steps = None if r.steps is None else r.steps.cpu().numpy()
        self.stepped = r.stepped()
        return self


def untouched(s, idx, O, D, states, steps):
    """Paths idx of step s kept every word: rays, states and counts as they came in, the canaries in the outputs."""
    assert np.array_equal(bits(s.O[idx]), bits(O[idx])) and np.array_equal(bits(s.D[idx]), bits(D[idx]))
    assert np.array_equal(s.S[idx], states[idx])
    assert (s.E[idx] == CANARY).all() and (s.A[idx] == CANARY).all()
    if s.raw is not None:
        assert (s.raw[idx] == CANARY_HIT).all()
    if s.steps is not None:
        assert np.array_equal(s.steps[idx], steps[idx])


# ------------------------------------------------------------------ 1. each step against the oracle
@pytest.mark.parametrize("name", WORLDS)
def test_each_step_matches_the_oracle(name):
    """Eight steps, each held to the oracle's Hit, Scatter and Emit path by path -- and the number of paths each step
    takes to the oracle's own Trace of the same rays: Trace's k-th query is step k.

    Every world except `empty` and `sky_only` must have paths alive at step 2 (the third step).  Two worlds cannot, by the
    oracle's own Trace of these 256 rays (SHORT_WORLDS): there the count is held to the oracle's, zero, and paths must be
    alive at step 1.  Paths taken per step on an MI355X, equal to the oracle's counts: furnace 256, 12, 0; quilt_3 256, 4, 0;
    the smallest third step elsewhere is textured_mesh's 256, 128, 1."""
    b, rec, ob, seed, O0, D0, Dn0 = world(name)
    n = len(O0)
    # the oracle's own path lengths: Trace at depth 8 through the raw camera, from the states the device is handed
    _, o_rays, _, dirs, S = oracle_trace(ob, O0, D0, oraclelib.rng_init(seed + 1, n, first=4242), 8)
    assert np.array_equal(bits(dirs), bits(Dn0))
    O, D = O0.copy(), Dn0.copy()
    steps = np.zeros(n, np.int32)
    alive_at = []
    for k in range(8):
        s = Step(b, O, D, S, steps).read()
        go = steppable(O, D)
        idx = np.flatnonzero(go)
        assert s.stepped == len(idx) == int((o_rays > k).sum()), (name, k)
        alive_at.append(len(idx))
        untouched(s, np.flatnonzero(~go), O, D, S, steps)
        if k == 0:
            assert go.all()
        assert np.array_equal(s.steps[idx], steps[idx] + 1)
        assert compare(s.raw, ob, O, D, rec, idx=idx) == [], (name, k)
        sky = []
        for i in idx:
            where = (name, k, int(i))
            hit, out, mat = ob.probe_hit(O[i], D[i])
            zero_d = not s.D[i].any()
            if not hit or mat < 0:  # nothing, or Sky: the path ends, nothing is drawn
                assert (bits(s.A[i]) == 0).all() and (bits(s.D[i]) == 0).all(), where
                assert np.array_equal(bits(s.O[i]), bits(O[i])) and np.array_equal(s.S[i], S[i]), where
                if hit:
                    sky.append(i)
                    p = hit_point(O[i], glm_normalize(D[i]), out[0])
                    assert np.array_equal(bits(s.E[i]), bits(sky_emit(p)[0])), where
                else:
                    assert (bits(s.E[i]) == 0).all(), where
                continue
            state = S[i].copy()
            sc, o12 = ob.probe_scatter_ex(mat, O[i], D[i], out[0], out[1], out[2], out[3:6], state)
            assert sc == (not zero_d), where
            assert np.array_equal(bits(s.E[i]), bits(o12[9:12])), where
            assert np.array_equal(s.S[i], state), where
            if sc:
                assert np.array_equal(bits(s.A[i]), bits(o12[0:3])), where
                assert np.array_equal(bits(s.O[i]), bits(o12[3:6])), where
                assert np.array_equal(bits(glm_normalize(s.D[i])), bits(o12[6:9])), where
            else:
                assert (bits(s.A[i]) == 0).all() and (bits(s.D[i]) == 0).all(), where
                assert np.array_equal(bits(s.O[i]), bits(O[i])), where
        if k == 0 and sky:
            # the restatement of Sky's Emit is itself the oracle's: Trace at depth 1 of a ray that hits Sky returns it
            sky = np.array(sky[:32])
            rgb, rays, _, dirs, _ = oracle_trace(ob, O0[sky], D0[sky], S[sky], 1)
            assert np.array_equal(bits(dirs), bits(Dn0[sky])) and (rays == 1).all()
            assert np.array_equal(bits(rgb), bits(s.E[sky])), name
        O, D, S, steps = s.O, s.D, s.S, s.steps
    print(name, "paths taken per step:", alive_at)
    if name in SHORT_WORLDS:
        assert alive_at[1] > 0 and alive_at[2] == int((o_rays > 2).sum()) == 0, alive_at
    elif name not in ("empty", "sky_only"):
        assert alive_at[2] > 0, (name, alive_at)


# ------------------------------------------------------------------ 2. the composed loop against the oracle's Trace
@pytest.mark.parametrize("name", WORLDS)
def test_trace_steps_match_the_oracle(name):
    b, rec, ob, seed, O, D, Dn = world(name)
    n = len(O)
    for depth in DEPTHS:
        states = oraclelib.rng_init(seed + depth, n, first=12345)
        o_rgb, o_rays, o_fin, dirs, handed = oracle_trace(ob, O, D, states, depth)
        assert np.array_equal(bits(dirs), bits(Dn))
        st = dev_states(handed)
        o, d = dev(O), dev(Dn)
        r = b.trace_steps(o, d, st, depth).check()
        assert np.array_equal(bits(o.cpu().numpy()), bits(O)) and np.array_equal(bits(d.cpu().numpy()), bits(Dn))  # copies
        rgb, cnt = r.rgb.cpu().numpy(), r.steps.cpu().numpy() + r.alive.cpu().numpy()
        bad = np.flatnonzero((bits(rgb) != bits(o_rgb)).any(1) | (cnt != o_rays) | (host_states(st) != o_fin).any(1))
        assert bad.size == 0, (name, depth, bad[:8].tolist(), rgb[bad[:4]].tolist(), o_rgb[bad[:4]].tolist(),
                               cnt[bad[:4]].tolist(), o_rays[bad[:4]].tolist())
        assert len(r.works) == depth and r.emitted.shape == (max(depth, 1), n, 3)


# ------------------------------------------------------------------ 3. the composed loop against rtmi_trace
@functools.lru_cache(maxsize=None)
def composed(name, depth):
    """64 x 64 camera rays of a scene through rtmi_trace and through trace_steps, from the same states; all on the host."""
    seed = common.scene_seed(name)
    b = common.build_scene(rtmi.SceneBuilder(seed), name, 1.0).commit()
    R = rtmi.Renderer(b, 64, 64, 1, depth, post=False)
    R.init_rng()
    o, d = R.camera_rays(0)
    st_a, st_b = R.states.clone(), R.states.clone()
    tr = b.trace(o, d, st_a, depth, count_rays=True).check()
    r = b.trace_steps(o, d, st_b, depth).check()
    out = dict(trace_rgb=tr.rgb.cpu().numpy(), trace_rays=tr.rays.cpu().numpy(), trace_total=tr.total_rays(),
               trace_states=host_states(st_a), states=host_states(st_b), rgb=r.rgb.cpu().numpy(),
               steps=r.steps.cpu().numpy(), alive=r.alive.cpu().numpy(), dirs=r.directions.cpu().numpy(),
               E=r.emitted.cpu().numpy(), A=r.attenuation.cpu().numpy(), stepped=[int(w[1].item()) for w in r.works])
    return out


CASES = [("cornell_box", 50), ("birthday", 10)]


@pytest.mark.parametrize("name,depth", CASES)
def test_trace_steps_reproduce_rtmi_trace(name, depth):
    c = composed(name, depth)
    assert np.array_equal(bits(c["rgb"]), bits(c["trace_rgb"])), np.flatnonzero((bits(c["rgb"]) != bits(c["trace_rgb"])).any(1))[:8]
    assert np.array_equal(c["steps"] + c["alive"], c["trace_rays"])
    assert np.array_equal(c["states"], c["trace_states"])
    assert sum(c["stepped"]) == int(c["steps"].sum()) and sum(c["stepped"]) + int(c["alive"].sum()) == c["trace_total"]
    assert c["steps"].max() >= 2, "no path bounced"


# ------------------------------------------------------------------ 4. the device fold against the numpy fold
@pytest.mark.parametrize("name,depth", CASES)
def test_path_fold_matches_the_numpy_fold(name, depth):
    c = composed(name, depth)
    n = len(c["steps"])
    want = fold(c["dirs"], c["steps"], c["E"], c["A"])
    assert np.array_equal(bits(want), bits(c["rgb"]))
    # fewer layers than some paths' steps, canaries (NaN) on both sides of both stacks: the clamp reads nothing outside
    L = (int(c["steps"].max()) + 1) // 2
    assert 1 <= L < depth and (c["steps"] > L).any() and (c["steps"] <= L).any()
    bufs = []
    for stack in (c["E"], c["A"]):
        buf = torch.full((L + 2, n, 3), float("nan"), dtype=torch.float32, device="cuda")
        buf[1:L + 1] = dev(stack[:L])
        bufs.append(buf)
    out = rtmi.path_fold(dev(c["dirs"]), dev(c["steps"], np.int32), bufs[0][1:L + 1], bufs[1][1:L + 1])
    got = out.cpu().numpy()
    assert not np.isnan(got).any()
    inside = c["steps"] <= L
    assert np.array_equal(bits(got[inside]), bits(want[inside]))
    assert np.array_equal(bits(got), bits(fold(c["dirs"], c["steps"], c["E"][:L], c["A"][:L])))  # the clamp as the numpy fold has it
    for buf in bufs:
        assert torch.isnan(buf[0]).all() and torch.isnan(buf[L + 1]).all()


# ------------------------------------------------------------------ 5. edge cases
def _world():
    b, rec, ob, seed, O, D, Dn = world("no_sky")
    return b, ob, seed, O, D, Dn


@pytest.mark.parametrize("n", [0, 1, 63, 65])
def test_batch_sizes(n):
    b, ob, seed, O, D, Dn = _world()
    O, D, Dn = O[:n], D[:n], Dn[:n]
    states = oraclelib.rng_init(seed, max(n, 1), first=7)[:n]
    o_rgb, o_rays, o_fin, dirs, handed = oracle_trace(ob, O, D, states, 10)
    st = dev_states(handed)
    r = b.trace_steps(dev(O).reshape(n, 3), dev(Dn).reshape(n, 3), st, 10).check()
    assert r.rgb.shape == (n, 3)
    assert np.array_equal(bits(r.rgb.cpu().numpy()), bits(o_rgb))
    assert np.array_equal(r.steps.cpu().numpy() + r.alive.cpu().numpy(), o_rays) and np.array_equal(host_states(st), o_fin)
    s = Step(b, O.reshape(n, 3), Dn.reshape(n, 3), handed.reshape(n, 6)).read()
    assert s.stepped == n and (s.steps == 1).all() and s.E.shape == (n, 3)


def test_bad_rays_are_left_out():
    b, ob, seed, O, D, Dn = _world()
    n = len(O)
    states = oraclelib.rng_init(seed, n, first=99)
    good = Step(b, O, Dn, states).read()
    bad = np.arange(3, n, 7)
    O2, D2 = O.copy(), Dn.copy()
    kinds = [(O2, 0, np.nan), (D2, 1, np.inf), (D2, None, 0.0), (O2, 2, -np.inf), (D2, None, 1e-30), (D2, None, 1e30)]
    for k, i in enumerate(bad):
        arr, col, val = kinds[k % len(kinds)]
        if col is None:
            arr[i] = val
        else:
            arr[i, col] = val
    # 1e-30 / 1e30 components: |d|^2 underflows / overflows, so the direction does not normalise
    assert not steppable(O2, D2)[bad].any()
    s = Step(b, O2, D2, states).read()
    untouched(s, bad, O2, D2, states, np.zeros(n, np.int32))
    ok = np.setdiff1d(np.arange(n), bad)
    assert s.stepped == len(ok) and good.stepped == n
    for a, g in ((s.O, good.O), (s.D, good.D), (s.E, good.E), (s.A, good.A)):
        assert np.array_equal(bits(a[ok]), bits(g[ok]))
    assert np.array_equal(s.S[ok], good.S[ok]) and np.array_equal(s.raw[ok], good.raw[ok]) and (s.steps[ok] == 1).all()


def test_inactive_camera_items_flow_through_untouched():
    """A budget map with zeros on a ragged 20 x 12 frame: rtmi_camera_rays writes a zero ray for every inactive item and
    padding, and a step leaves those alone."""
    name = "cornell_box"
    b = common.build_scene(rtmi.SceneBuilder(common.scene_seed(name)), name, 1.0).commit()
    R = rtmi.Renderer(b, 12, 20, 2, 8, post=False)
    R.init_rng()
    pixel_of = rtmi.pixel_map(R.frame)
    budget = np.where(np.arange(R.items) % 3 == 0, 0, 2).astype(np.int32)
    o, d = R.camera_rays(0, dev(budget, np.int32))
    O, D, S = o.cpu().numpy(), d.cpu().numpy(), host_states(R.states)
    inactive = (pixel_of < 0) | (budget == 0)
    assert (pixel_of < 0).any() and (bits(D[inactive]) == 0).all() and (D[~inactive] != 0).any(1).all()
    s = Step(b, O, D, S).read()
    untouched(s, np.flatnonzero(inactive), O, D, S, np.zeros(R.items, np.int32))
    assert s.stepped == int((~inactive).sum()) and (s.steps[~inactive] == 1).all()
    assert (s.E[~inactive] != CANARY).all() and (s.raw[~inactive, 7] != rtmi.RTMI_HIT_NONE).all()


def test_null_hits_and_steps_change_no_other_output():
    b, ob, seed, O, D, Dn = _world()
    states = oraclelib.rng_init(seed, len(O), first=5)
    a = Step(b, O, Dn, states).read()
    c = Step(b, O, Dn, states, hits=False, count=False).read()
    assert c.raw is None and c.steps is None and c.stepped == a.stepped == len(O)
    for x, y in ((a.O, c.O), (a.D, c.D), (a.E, c.E), (a.A, c.A)):
        assert np.array_equal(bits(x), bits(y))
    assert np.array_equal(a.S, c.S)


def test_two_streams_with_their_own_work():
    b, ob, seed, O, D, Dn = _world()
    O, Dn = np.tile(O, (8, 1)), np.tile(Dn, (8, 1))
    states = oraclelib.rng_init(seed, len(O))
    ref = Step(b, O, Dn, states).read()
    torch.cuda.synchronize()
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    t1, t2 = Step(b, O, Dn, states, stream=s1), Step(b, O, Dn, states, stream=s2)
    torch.cuda.synchronize()
    assert t1.r.work.data_ptr() != t2.r.work.data_ptr()
    for t in (t1.read(), t2.read()):
        for x, y in ((t.O, ref.O), (t.D, ref.D), (t.E, ref.E), (t.A, ref.A)):
            assert np.array_equal(bits(x), bits(y))
        assert np.array_equal(t.S, ref.S) and np.array_equal(t.raw, ref.raw) and t.stepped == ref.stepped


def test_arguments_refused_on_a_committed_scene():
    b, ob, seed, O, D, Dn = _world()
    n = len(O)
    o, d, st = dev(O), dev(Dn), rtmi.rng_states(seed, n)
    em, at = torch.empty_like(o), torch.empty_like(o)
    with pytest.raises(rtmi.RtmiError):
        b.bounce(o, d, st[:, :-1].contiguous())
    with pytest.raises(rtmi.RtmiError):
        b.bounce(o, d, st.to(torch.int64))
    with pytest.raises(rtmi.RtmiError):
        b.bounce(o.cpu(), d.cpu(), st)
    with pytest.raises(rtmi.RtmiError):
        b.bounce(o, d.t().contiguous().t(), st)  # not contiguous: the step could not write into it
    with pytest.raises(rtmi.RtmiError):
        b.bounce(o, d, st, emitted=em[:-1])
    for depth in (-1, 65):
        with pytest.raises(rtmi.RtmiError):
            b.trace_steps(o, d, st, depth)
    L = rtmi.lib()
    work = torch.zeros((rtmi.TRACE_WORK_WORDS,), dtype=torch.int64, device=o.device)
    p = lambda t: C.c_void_p(t.data_ptr())
    full = [p(o), p(d), p(st), p(em), p(at)]
    for k in range(5):
        args = list(full)
        args[k] = None
        assert L.rtmi_bounce(b.h, n, *args, None, None, p(work), None) == ERR_INVALID, k
    assert L.rtmi_bounce(b.h, n, *full, None, None, None, None) == ERR_INVALID
    assert L.rtmi_bounce(b.h, -1, *full, None, None, p(work), None) == ERR_INVALID
    assert L.rtmi_bounce(b.h, 0, *full, None, None, p(work), None) == OK and int(work.abs().sum().item()) == 0
    steps = torch.zeros((n,), dtype=torch.int32, device=o.device)
    for layers in (0, 65):
        assert L.rtmi_path_fold(n, layers, p(d), p(steps), p(em), p(at), p(em), None) == ERR_INVALID
    if torch.cuda.device_count() > 1:
        with torch.cuda.device(1):
            assert L.rtmi_bounce(b.h, n, *full, None, None, p(work), None) == ERR_INVALID
            with pytest.raises(rtmi.RtmiError):
                b.bounce(o.to("cuda:1"), d.to("cuda:1"), st.to("cuda:1"))
    torch.cuda.synchronize()
    assert np.array_equal(bits(o.cpu().numpy()), bits(O)) and np.array_equal(bits(d.cpu().numpy()), bits(Dn))  # nothing ran


# ------------------------------------------------------------------ 6. `each` is live
def test_each_can_end_paths():
    """A callback that zeroes the direction of every path whose step hit the metal ends exactly those paths, there."""
    b, rec, ob, seed, O, D, Dn = world("nested")  # (a world with Sky: a path that is cut loses the light it would have found)
    n, depth, metal = len(O), 8, 1  # (world_nested: material 1 is the metal)
    st_ref, st_cut = rtmi.rng_states(seed, n, first=31), rtmi.rng_states(seed, n, first=31)
    o, d = dev(O), dev(Dn)
    mats, alive_in = [], []

    def record(k, r):
        alive_in.append((r.steps.cpu().numpy() == k + 1))  # the paths this step took
        mats.append(r.hits.material.cpu().numpy().copy())
    ref = b.trace_steps(o, d, st_ref, depth, each=record).check()
    took, mats = np.array(alive_in), np.array(mats)
    on_metal = took & (mats == metal)
    assert on_metal[1:].any() and (~on_metal.any(0)).any()  # paths end at their first step, at later ones, or never
    first = np.where(on_metal.any(0), on_metal.argmax(0), depth)  # the step at which the callback ends the path

    def cut(k, r):
        stepped = r.steps == k + 1
        r.directions[stepped & (r.hits.material == metal)] = 0.0
    res = b.trace_steps(o, d, st_cut, depth, each=cut).check()
    steps, alive = res.steps.cpu().numpy(), res.alive.cpu().numpy()
    ref_steps, ref_alive = ref.steps.cpu().numpy(), ref.alive.cpu().numpy()
    ended = first < depth
    assert np.array_equal(steps[ended], first[ended] + 1) and not alive[ended].any()
    assert np.array_equal(steps[~ended], ref_steps[~ended]) and np.array_equal(alive[~ended], ref_alive[~ended])
    rgb = res.rgb.cpu().numpy()
    assert np.array_equal(bits(rgb[~ended]), bits(ref.rgb.cpu().numpy()[~ended]))
    want = fold(res.directions.cpu().numpy(), steps, res.emitted.cpu().numpy(), res.attenuation.cpu().numpy())
    assert np.array_equal(bits(rgb), bits(want))
    changed = (bits(rgb[ended]) != bits(ref.rgb.cpu().numpy()[ended])).any(1)
    assert changed.any()  # the cut shows in the radiance
