"""rtmi_path_compact / rtmi_bounce_list / SceneBuilder.trace_steps(compact=...) on the GPU: the compaction against its
numpy restatement (tests/bouncelistlib.py, held to hand-worked cases by tests/test_bounce_list_host.py), a listed step
against rtmi_bounce word for word, the compacted loop against the plain loop, rtmi_trace and the oracle's Trace, and the
edges -- all bit for bit."""
import ctypes as C
import functools

import numpy as np
import pytest

import common
import oraclelib
import rtmi
from abi_host import ERR_INVALID, OK
from bouncelib import dev, dev_states, host_states, oracle_trace, world
from bouncelistlib import (BAD_KINDS, CANARY_F, CANARY_INDEX, P, PATTERNS, SCAN_THREADS, Compaction, check_compaction, compact,
                           dev_u32, live, make_bad, ptr, rays)
from parity import bits
from querylib import CUSTOM_WORLDS, SCENE_WORLDS

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

WORLDS = SCENE_WORLDS + sorted(CUSTOM_WORLDS)
CANARY_HIT = 0x5a5a5a5a
# every size at which the compaction takes another path: a wave's chunk of 64, a workgroup's P entries, more than one
# workgroup, and more workgroups than the scan has lanes (each of its lanes then sums two counts in a row)
SIZES = [0, 1, 63, 64, 65, P - 1, P, P + 1, 2 * P + 1, SCAN_THREADS * P + P + 1]


# ------------------------------------------------------------------ 1. the compaction against numpy
@pytest.mark.parametrize("n", SIZES)
def test_compaction_of_all_paths_matches_numpy(n):
    for pattern in PATTERNS:
        if n == 0 and pattern != "all":
            continue
        O, D = rays(n, pattern)
        want = compact(O, D)
        if n > 0:
            assert len(want) == {"all": n, "none": 0, "alternating": (n + 1) // 2, "last": 1}.get(pattern, len(want)), pattern
        if pattern == "mixed" and n >= 64:
            assert 0 < len(want) < n
        check_compaction(Compaction(O, D).read(), O, D, want)


@pytest.mark.parametrize("n", [65, P + 1, 2 * P + 1])
def test_compaction_of_a_list_keeps_the_lists_order(n):
    rng = np.random.default_rng(n)
    O, D = rays(n, "mixed", seed=1)
    sub = np.sort(rng.choice(n, (2 * n) // 3, replace=False)).astype(np.uint32)  # a random ascending subset
    want = compact(O, D, sub)
    assert 0 < len(want) < len(sub) and (np.diff(want.astype(np.int64)) > 0).all()
    check_compaction(Compaction(O, D, sub).read(), O, D, want)
    # a device count that cuts the list short: live entries behind it are ignored
    cut = len(sub) // 2
    assert live(O, D)[sub[cut:]].any()
    check_compaction(Compaction(O, D, sub, count_in=cut).read(), O, D, compact(O, D, sub, count_in=cut))
    check_compaction(Compaction(O, D, sub, count_in=0).read(), O, D, np.zeros(0, np.uint32))
    check_compaction(Compaction(O, D, sub, count_in=len(sub) + 1000).read(), O, D, want)  # ... and never lengthens it
    # the host's bound below the list's length, with and without a count
    check_compaction(Compaction(O, D, sub, n_list=cut).read(), O, D, compact(O, D, sub, n_list=cut))
    # a null list shorter than n
    check_compaction(Compaction(O, D, n_list=n - 3).read(), O, D, compact(O, D, n_list=n - 3))
    check_compaction(Compaction(O, D, count_in=n // 2).read(), O, D, compact(O, D, count_in=n // 2))
    # a permuted list comes out in its own order; entries that are no paths are dropped
    perm = rng.permutation(sub)
    perm[::7] = (n, n + 1, 1 << 31, 0xffffffff)[n % 4]
    got = Compaction(O, D, perm).read()
    check_compaction(got, O, D, compact(O, D, perm))
    assert (np.diff(got.out.astype(np.int64)) < 0).any() and (got.out < n).all()
    # a list longer than n (every path twice is not a list for a step, but the compaction keeps it entry by entry)
    twice = np.concatenate([sub, sub[::-1]])
    check_compaction(Compaction(O, D, twice).read(), O, D, compact(O, D, twice))


def test_compaction_through_the_binding_ping_pongs():
    n = 2 * P + 77
    O, D = rays(n, "mixed", seed=2)
    o, d = dev(O), dev(D)
    a = rtmi.path_compact(o, d)
    assert a.index.shape == (n,) and a.index.dtype == torch.int32 and a.count.shape == (1,)
    want = compact(O, D)
    assert a.n() == len(want) and np.array_equal(a.index[:a.n()].cpu().numpy().view(np.uint32), want)
    # end every third live path, compact the list: the list's own live ones, ascending
    D2 = D.copy()
    D2[want[::3]] = 0.0
    d2 = dev(D2)
    out = rtmi.Paths(torch.full((n + 5,), CANARY_INDEX, dtype=torch.int32, device="cuda"), torch.zeros(1, dtype=torch.int32, device="cuda"))
    b = rtmi.path_compact(o, d2, a, out=out)
    assert b is out and b.n() == len(want) - len(want[::3])
    assert np.array_equal(b.index[:b.n()].cpu().numpy().view(np.uint32), compact(O, D2, want))
    assert (b.index[b.n():] == CANARY_INDEX).all()
    with pytest.raises(rtmi.RtmiError):
        rtmi.path_compact(o, d2, a, out=a)
    with pytest.raises(rtmi.RtmiError):
        rtmi.path_compact(o, d2, a, out=rtmi.Paths(out.index[:4], out.count))  # no room for every candidate
    with pytest.raises(rtmi.RtmiError):
        rtmi.path_compact(o, d2, rtmi.Paths(a.index.to(torch.int64), a.count))


# ------------------------------------------------------------------ device steps through the C ABI
class ListStep:
    """One rtmi_bounce_list (plain=True: rtmi_bounce) on device copies of (O, D, states (n, 6)), canaries in every output,
    everything read back."""

    def __init__(self, b, O, D, states, lst=None, n_list=None, count=None, steps=None, plain=False, stream=None):
        n = len(O)
        self.o, self.d, self.st = dev(O).reshape(n, 3), dev(D).reshape(n, 3), dev_states(states)
        self.em = torch.full((n, 3), float(CANARY_F), dtype=torch.float32, device="cuda")
        self.at = torch.full((n, 3), float(CANARY_F), dtype=torch.float32, device="cuda")
        self.hits = torch.full((n, 12), CANARY_HIT, dtype=torch.int32, device="cuda")
        self.cnt = dev(np.zeros(n, np.int32) if steps is None else steps, np.int32)
        self.work = torch.zeros((rtmi.TRACE_WORK_WORDS,), dtype=torch.int64, device="cuda")
        # (a list or a count that is on the device already is used where it is)
        self.lst = lst if lst is None or isinstance(lst, torch.Tensor) else dev_u32(lst)
        self.count = count if count is None or isinstance(count, torch.Tensor) else dev_u32([count])
        if n_list is None:
            n_list = n if lst is None else len(lst)
        s = torch.cuda.current_stream()
        if stream is not None:
            stream.wait_stream(s)  # (the copies and canaries above were enqueued there)
            s = stream
        L = rtmi.lib()
        tail = (ptr(self.o), ptr(self.d), ptr(self.st), ptr(self.em), ptr(self.at), ptr(self.hits), ptr(self.cnt), ptr(self.work),
                C.c_void_p(s.cuda_stream))
        if plain:
            self.rc = L.rtmi_bounce(b.h, n, *tail)
        else:
            self.rc = L.rtmi_bounce_list(b.h, n, ptr(self.lst), n_list, ptr(self.count), *tail)

    def read(self):
        assert self.rc == OK, rtmi.lib().rtmi_last_error()
        torch.cuda.synchronize()
        self.O, self.D, self.S = self.o.cpu().numpy(), self.d.cpu().numpy(), host_states(self.st)
        self.E, self.A, self.raw = self.em.cpu().numpy(), self.at.cpu().numpy(), self.hits.cpu().numpy()
        self.steps = self.cnt.cpu().numpy()
        w = self.work.cpu().numpy()
        self.abandoned, self.stepped = int(w[0]), int(w[1])
        return self


def same_on(s, ref, idx):
    """Paths idx of step s hold what step ref gave them, word for word."""
    for a, g in ((s.O, ref.O), (s.D, ref.D), (s.E, ref.E), (s.A, ref.A)):
        assert np.array_equal(bits(a[idx]), bits(g[idx]))
    assert np.array_equal(s.S[idx], ref.S[idx]) and np.array_equal(s.raw[idx], ref.raw[idx])
    assert np.array_equal(s.steps[idx], ref.steps[idx])


def untouched(s, idx, O, D, states, steps):
    """Paths idx of step s kept every word: rays, states and counts as they came in, the canaries in the outputs."""
    assert np.array_equal(bits(s.O[idx]), bits(O[idx])) and np.array_equal(bits(s.D[idx]), bits(D[idx]))
    assert np.array_equal(s.S[idx], states[idx])
    assert (s.E[idx] == CANARY_F).all() and (s.A[idx] == CANARY_F).all() and (s.raw[idx] == CANARY_HIT).all()
    assert np.array_equal(s.steps[idx], steps[idx])


def check_listed(b, O, D, S, steps, ref, listed, **how):
    """A step of the paths `listed` (what the list given by `how` names) against ref, the plain step of all paths."""
    n = len(O)
    s = ListStep(b, O, D, S, steps=steps, **how).read()
    listed = np.asarray(listed, dtype=np.int64)
    rest = np.setdiff1d(np.arange(n), listed)
    same_on(s, ref, listed)
    untouched(s, rest, O, D, S, steps)
    assert s.abandoned == 0 and s.stepped == int(live(O, D)[listed].sum())
    return s


# ------------------------------------------------------------------ 2. the list is the step's
def test_a_compactions_count_is_what_the_step_steps():
    b, rec, ob, seed, O, D, Dn = world("no_sky")
    n = len(O)
    O, Dn = O.copy(), Dn.copy()
    for k, i in enumerate(range(2, n, 5)):
        make_bad(O, Dn, i, BAD_KINDS[k % len(BAD_KINDS)])
    alive = live(O, Dn)
    assert 0 < alive.sum() < n
    o, d, st = dev(O), dev(Dn), rtmi.rng_states(seed, n)
    paths = rtmi.path_compact(o, d)
    r = b.bounce_list(paths, o, d, st).check()
    assert r.paths is paths and paths.n() == r.stepped() == int(alive.sum())
    # the same rays listed as they are, dead ones included: the step skips exactly those the compaction drops
    o, d = dev(O), dev(Dn)
    every = rtmi.Paths(torch.arange(n, dtype=torch.int32, device="cuda"))
    assert b.bounce_list(every, o, d, rtmi.rng_states(seed, n)).check().stepped() == int(alive.sum())


# ------------------------------------------------------------------ 3. a listed step is rtmi_bounce
@pytest.mark.parametrize("name", WORLDS)
def test_a_listed_step_is_rtmi_bounce(name):
    """A random half of the paths through rtmi_bounce_list against rtmi_bounce on a copy, for two steps: the second takes
    the rays the first left, ended paths among them."""
    b, rec, ob, seed, O, D, Dn = world(name)
    n = len(O)
    rng = np.random.default_rng(seed + 5)
    O, D, S, steps = O, Dn, oraclelib.rng_init(seed + 3, n, first=77), np.zeros(n, np.int32)
    for k in range(2):
        lst = np.sort(rng.choice(n, n // 2, replace=False))
        ref = ListStep(b, O, D, S, steps=steps, plain=True).read()
        assert ref.abandoned == 0
        check_listed(b, O, D, S, steps, ref, lst, lst=lst)
        if k == 0:
            assert ref.stepped == n
        O, D, S, steps = ref.O, ref.D, ref.S, ref.steps


@pytest.mark.parametrize("name", ["cornell_box", "bunny"])
def test_the_ways_to_name_a_list(name):
    b, rec, ob, seed, O, D, Dn = world(name)
    n = len(O)
    rng = np.random.default_rng(seed + 6)
    S0 = oraclelib.rng_init(seed + 4, n, first=5)
    first = ListStep(b, O, Dn, S0, plain=True).read()
    O, D, S, steps = first.O, first.D, first.S, first.steps  # the second step's rays: some paths have ended
    assert 0 < live(O, D).sum() < n
    ref = ListStep(b, O, D, S, steps=steps, plain=True).read()
    lst = np.sort(rng.choice(n, n // 2, replace=False)).astype(np.uint32)
    check_listed(b, O, D, S, steps, ref, np.arange(n - 100), n_list=n - 100)             # a null list and n_list < n
    check_listed(b, O, D, S, steps, ref, np.arange(n))                                   # the identity
    check_listed(b, O, D, S, steps, ref, lst[:40], lst=lst, count=40)                    # a device count below n_list
    check_listed(b, O, D, S, steps, ref, lst, lst=lst, count=len(lst) + 9)               # ... and one above it
    check_listed(b, O, D, S, steps, ref, lst[:70], lst=lst, n_list=70)                   # the host's bound below the list
    check_listed(b, O, D, S, steps, ref, np.arange(33), count=33)                        # a count on the identity
    check_listed(b, O, D, S, steps, ref, lst, lst=rng.permutation(lst))                  # a permuted list
    wild = lst.copy()
    wild[::9] = [n, n + 5, (1 << 31) + 3, 0xffffffff, n + 64][: len(wild[::9])] + [n] * max(0, len(wild[::9]) - 5)
    check_listed(b, O, D, S, steps, ref, wild[wild < n], lst=wild)                       # entries >= n are skipped
    s = check_listed(b, O, D, S, steps, ref, [], lst=lst, count=0)                       # an empty list
    assert s.stepped == 0


# ------------------------------------------------------------------ 4. the loop composes
@functools.lru_cache(maxsize=None)
def composed(name, depth):
    """64 x 64 camera rays of a scene through rtmi_trace and through the three loops, from the same states; on the host."""
    seed = common.scene_seed(name)
    b = common.build_scene(rtmi.SceneBuilder(seed), name, 1.0).commit()
    R = rtmi.Renderer(b, 64, 64, 1, depth, post=False)
    R.init_rng()
    o, d = R.camera_rays(0)
    st = R.states.clone()
    tr = b.trace(o, d, st, depth, count_rays=True).check()
    out = dict(trace=dict(rgb=tr.rgb.cpu().numpy(), rays=tr.rays.cpu().numpy(), total=tr.total_rays(), states=host_states(st)))
    for key, kw in (("plain", {}), ("compact", dict(compact=True)), ("full", dict(compact="full"))):
        st = R.states.clone()
        listed = []
        each = None if key == "plain" else (lambda k, r: listed.append(r.paths))
        r = b.trace_steps(o, d, st, depth, each=each, hits=False, **kw).check()
        out[key] = dict(rgb=r.rgb.cpu().numpy(), steps=r.steps.cpu().numpy(), alive=r.alive.cpu().numpy(),
                        dirs=r.directions.cpu().numpy(), states=host_states(st), stepped=[int(w[1].item()) for w in r.works],
                        lists=len(set(id(p) for p in listed)), none=sum(p is None for p in listed))
    return out


@pytest.mark.parametrize("name,depth", [("cornell_box", 50), ("birthday", 10)])
def test_the_compacted_loops_reproduce_the_plain_loop_and_rtmi_trace(name, depth):
    c = composed(name, depth)
    tr, plain = c["trace"], c["plain"]
    assert plain["steps"].max() >= 2, "no path bounced"
    for key in ("compact", "full"):
        r = c[key]
        assert np.array_equal(bits(r["rgb"]), bits(tr["rgb"])) and np.array_equal(bits(r["rgb"]), bits(plain["rgb"])), key
        assert np.array_equal(r["steps"], plain["steps"]) and np.array_equal(r["steps"] + r["alive"], tr["rays"]), key
        assert np.array_equal(r["states"], tr["states"]) and np.array_equal(bits(r["dirs"]), bits(plain["dirs"])), key
        assert r["stepped"] == plain["stepped"], key  # step by step the same paths
        # the stepped counts sum to rtmi_trace's queries, less the final counting query of the paths still alive
        assert sum(r["stepped"]) == int(r["steps"].sum()) == tr["total"] - int(r["alive"].sum()), key
        assert r["lists"] == 2 and r["none"] == 0, key  # two lists, ping-ponged, handed to `each`


@pytest.mark.parametrize("name", WORLDS)
def test_the_compacted_loops_match_the_oracle(name):
    b, rec, ob, seed, O, D, Dn = world(name)
    n = len(O)
    for depth in (0, 1, 8):
        states = oraclelib.rng_init(seed + depth, n, first=12345)
        o_rgb, o_rays, o_fin, dirs, handed = oracle_trace(ob, O, D, states, depth)
        assert np.array_equal(bits(dirs), bits(Dn))
        for mode in (True, "full"):
            st = dev_states(handed)
            r = b.trace_steps(dev(O), dev(Dn), st, depth, compact=mode).check()
            rgb, cnt = r.rgb.cpu().numpy(), r.steps.cpu().numpy() + r.alive.cpu().numpy()
            bad = np.flatnonzero((bits(rgb) != bits(o_rgb)).any(1) | (cnt != o_rays) | (host_states(st) != o_fin).any(1))
            assert bad.size == 0, (name, depth, mode, bad[:8].tolist())
            assert len(r.works) == depth
            assert sum(int(w[1].item()) for w in r.works) == int(o_rays.sum()) - int(r.alive.sum().item())


def test_a_revived_path_needs_the_full_compaction():
    """`each` revives, after step 1, a path that step 0 ended: the plain loop and compact="full" step it again, the
    incremental compaction -- which starts from the list of the step before -- never sees it."""
    b, rec, ob, seed, O, D, Dn = world("nested")
    n, depth = len(O), 4
    ended = {}

    def revive(k, r):
        if k == 0:
            dead = (r.directions == 0).all(dim=1)
            ended["i"] = int(torch.nonzero(dead)[0])  # a path that ended in step 0 (Sky, or a light)
        if k == 1:
            r.directions[ended["i"]] = torch.tensor([0.0, 1.0, 0.0], device="cuda")
    runs = {}
    for mode in (False, True, "full"):
        st = rtmi.rng_states(seed, n, first=3)
        runs[mode] = b.trace_steps(dev(O), dev(Dn), st, depth, each=revive, compact=mode).check()
    i = ended["i"]
    assert int(runs[False].steps[i]) >= 2 and int(runs[True].steps[i]) == 1
    assert torch.equal(runs["full"].steps, runs[False].steps)
    # (the revived path skipped a step, so its layers have a hole no step wrote: its radiance is the hook's business)
    others = torch.arange(n, device="cuda") != i
    for mode in (True, "full"):
        assert torch.equal(runs[mode].rgb.view(torch.int32)[others], runs[False].rgb.view(torch.int32)[others])
        assert torch.equal(runs[mode].steps[others], runs[False].steps[others])


# ------------------------------------------------------------------ 5. edges
def _world():
    b, rec, ob, seed, O, D, Dn = world("no_sky")
    return b, ob, seed, O, D, Dn


@pytest.mark.parametrize("n", [0, 1, 63, 65])
def test_batch_sizes(n):
    b, ob, seed, O, D, Dn = _world()
    O, D, Dn = O[:n].reshape(n, 3), D[:n].reshape(n, 3), Dn[:n].reshape(n, 3)
    states = oraclelib.rng_init(seed, max(n, 1), first=7)[:n].reshape(n, 6)
    o_rgb, o_rays, o_fin, dirs, handed = oracle_trace(ob, O, D, states, 10)
    for mode in (True, "full"):
        st = dev_states(handed)
        r = b.trace_steps(dev(O).reshape(n, 3), dev(Dn).reshape(n, 3), st, 10, compact=mode).check()
        assert r.rgb.shape == (n, 3) and np.array_equal(bits(r.rgb.cpu().numpy()), bits(o_rgb))
        assert np.array_equal(r.steps.cpu().numpy() + r.alive.cpu().numpy(), o_rays) and np.array_equal(host_states(st), o_fin)
    s = ListStep(b, O, Dn, handed).read()
    assert s.stepped == n and (s.steps == 1).all() and s.E.shape == (n, 3)
    check_compaction(Compaction(O, Dn).read(), O, Dn, np.arange(n, dtype=np.uint32))
    p = rtmi.path_compact(dev(O).reshape(n, 3), dev(Dn).reshape(n, 3))
    assert p.n() == n and b.bounce_list(p, dev(O).reshape(n, 3), dev(Dn).reshape(n, 3), dev_states(handed)).check().stepped() == n


def test_nan_filled_stacks_around_the_layers():
    """The loop by hand on stacks with a NaN layer on either side and NaN in every layer: a listed step writes its paths'
    words of its layer only, and the fold reads nothing a step did not write."""
    b, ob, seed, O, D, Dn = _world()
    n, depth = len(O), 6
    st_a, st_b = rtmi.rng_states(seed, n, first=21), rtmi.rng_states(seed, n, first=21)
    want = b.trace(dev(O), dev(Dn), st_a, depth).check()
    o, d = dev(O), dev(Dn)
    E = torch.full((depth + 2, n, 3), float("nan"), dtype=torch.float32, device="cuda")
    A = torch.full((depth + 2, n, 3), float("nan"), dtype=torch.float32, device="cuda")
    steps = torch.zeros((n,), dtype=torch.int32, device="cuda")
    paths, stepped = None, []
    for k in range(depth):
        paths = rtmi.path_compact(o, d, paths)
        stepped.append(b.bounce_list(paths, o, d, st_b, emitted=E[1 + k], attenuation=A[1 + k], steps=steps).check().stepped())
    rgb = rtmi.path_fold(d, steps, E[1:depth + 1], A[1:depth + 1])
    assert torch.equal(rgb.view(torch.int32), want.rgb.view(torch.int32)) and torch.equal(st_a, st_b)
    assert stepped[0] == n and stepped[-1] < n
    for buf in (E, A):
        assert torch.isnan(buf[0]).all() and torch.isnan(buf[depth + 1]).all()
        assert torch.isnan(buf[depth][steps < depth]).all()  # the last layer of the paths that were no longer listed


def test_two_streams_with_their_own_work_and_scratch():
    b, ob, seed, O, D, Dn = _world()
    O, Dn = np.tile(O, (8, 1)), np.tile(Dn, (8, 1))
    n = len(O)
    Dn[1::3] = 0.0
    states = oraclelib.rng_init(seed, n)
    want = compact(O, Dn)
    ref = ListStep(b, O, Dn, states, lst=want).read()
    torch.cuda.synchronize()
    runs = []
    for s in (torch.cuda.Stream(), torch.cuda.Stream()):
        c = Compaction(O, Dn, stream=s)  # its own scratch
        # the listed step on the same stream, from the list and the count where the compaction leaves them; its own d_work
        t = ListStep(b, O, Dn, states, lst=c.list_out, n_list=n, count=c.count_out[1:2], stream=s)
        runs.append((c, t))
    torch.cuda.synchronize()
    assert runs[0][1].work.data_ptr() != runs[1][1].work.data_ptr()
    assert runs[0][0].scratch.data_ptr() != runs[1][0].scratch.data_ptr()
    for c, t in runs:
        check_compaction(c.read(), O, Dn, want)
        t.read()
        same_on(t, ref, want.astype(np.int64))
        untouched(t, np.setdiff1d(np.arange(n), want), O, Dn, states, np.zeros(n, np.int32))
        assert t.stepped == ref.stepped == len(want)


def test_arguments_refused_on_a_committed_scene():
    b, ob, seed, O, D, Dn = _world()
    n = len(O)
    o, d, st = dev(O), dev(Dn), rtmi.rng_states(seed, n)
    em, at = torch.full_like(o, float(CANARY_F)), torch.full_like(o, float(CANARY_F))
    lst = torch.arange(n, dtype=torch.int32, device="cuda")
    out = torch.full((n,), CANARY_INDEX, dtype=torch.int32, device="cuda")
    cnt, cnt2 = torch.full((1,), n, dtype=torch.int32, device="cuda"), torch.full((1,), CANARY_INDEX, dtype=torch.int32, device="cuda")
    scratch = torch.full((4,), CANARY_INDEX, dtype=torch.int32, device="cuda")
    work = torch.zeros((rtmi.TRACE_WORK_WORDS,), dtype=torch.int64, device="cuda")
    L = rtmi.lib()
    step = lambda n_, l_, nl_, c_, *rest: L.rtmi_bounce_list(b.h, n_, l_, nl_, c_, *rest, None, None, ptr(work), None)
    full = [ptr(o), ptr(d), ptr(st), ptr(em), ptr(at)]
    for k in range(5):
        args = list(full)
        args[k] = None
        assert step(n, ptr(lst), n, ptr(cnt), *args) == ERR_INVALID, k
    assert L.rtmi_bounce_list(b.h, n, ptr(lst), n, ptr(cnt), *full, None, None, None, None) == ERR_INVALID
    assert step(-1, ptr(lst), n, ptr(cnt), *full) == ERR_INVALID
    assert step(n, ptr(lst), -1, ptr(cnt), *full) == ERR_INVALID
    assert step(n, ptr(lst), 1 << 31, ptr(cnt), *full) == ERR_INVALID
    assert step(n, None, n + 1, None, *full) == ERR_INVALID
    assert step(0, None, 0, None, *full) == OK and int(work.abs().sum().item()) == 0  # n == 0: d_work as it is
    comp = lambda n_, l_, nl_, c_, lo=out, co=cnt2, sc=scratch, o_=o, d_=d: L.rtmi_path_compact(
        n_, ptr(o_), ptr(d_), l_, nl_, c_, ptr(lo), ptr(co), ptr(sc), None)
    assert comp(-1, None, 0, None) == ERR_INVALID and comp(n, None, -1, None) == ERR_INVALID
    assert comp(n, ptr(lst), 1 << 31, None) == ERR_INVALID and comp(n, None, n + 1, None) == ERR_INVALID
    assert comp(n, ptr(lst), n, None, lo=lst) == ERR_INVALID and comp(n, ptr(lst), n, ptr(cnt), co=cnt) == ERR_INVALID
    for k in ("lo", "co", "sc", "o_", "d_"):
        assert comp(n, ptr(lst), n, ptr(cnt), **{k: None}) == ERR_INVALID, k
    with pytest.raises(rtmi.RtmiError):
        b.bounce_list(rtmi.Paths(lst.to(torch.int64)), o, d, st)
    with pytest.raises(rtmi.RtmiError):
        b.bounce_list(rtmi.Paths(lst, cnt.to(torch.int64)), o, d, st)
    with pytest.raises(rtmi.RtmiError):
        b.bounce_list(lst, o, d, st)  # a bare tensor is not a list
    with pytest.raises(rtmi.RtmiError):
        b.bounce_list(rtmi.Paths(lst, cnt), o, d, st[:, :-1].contiguous())
    if torch.cuda.device_count() > 1:
        with torch.cuda.device(1):
            assert step(n, ptr(lst), n, ptr(cnt), *full) == ERR_INVALID
            with pytest.raises(rtmi.RtmiError):
                b.bounce_list(None, o.to("cuda:1"), d.to("cuda:1"), st.to("cuda:1"))
    torch.cuda.synchronize()
    # nothing ran
    assert np.array_equal(bits(o.cpu().numpy()), bits(O)) and np.array_equal(bits(d.cpu().numpy()), bits(Dn))
    assert (em == float(CANARY_F)).all() and (at == float(CANARY_F)).all() and int(work.abs().sum().item()) == 0
    assert (out == CANARY_INDEX).all() and (cnt2 == CANARY_INDEX).all() and (scratch == CANARY_INDEX).all()
    assert torch.equal(lst, torch.arange(n, dtype=torch.int32, device="cuda")) and int(cnt.item()) == n
    # n_list == 0 writes the count and nothing else; for the step it resets d_work and steps nothing
    assert comp(n, None, 0, None) == OK and step(n, ptr(lst), 0, None, *full) == OK
    torch.cuda.synchronize()
    assert int(cnt2.item()) == 0 and (out == CANARY_INDEX).all() and (scratch == CANARY_INDEX).all()
    assert int(work.abs().sum().item()) == 0 and (em == float(CANARY_F)).all()
