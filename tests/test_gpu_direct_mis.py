"""rtmi_direct_sample_mis on the GPU: the step against its numpy restatement (tests/mislib.py) bit for bit -- on real
paths whose carries a real step before wrote, against rtmi_direct_sample in the same run, on synthetic hits of every
kind, on a table beyond the LDS staging and a list beyond one round of the grid --, the direct="mis" loop leaving the
plain loop's paths alone and reducing to rtmi_trace where it must, its radiance having rtmi_trace's expectation on
lamp_room, the Cornell box, close_lamp_room and the furnace, and its variance below the unweighted sampler's where a
lamp lies close to a wall."""
import ctypes as C
import functools

import numpy as np
import pytest

import common
import directlib as dl
import mislib as ml
import rtmi
from abi_host import ERR_INVALID
from bouncelistlib import BAD_KINDS, make_bad
from parity import bits
from querylib import Recorder

pytestmark = pytest.mark.gpu
f32 = np.float32
SIZES = [1, 63, 64, 65, 4133]
KINDS = (rtmi.RTMI_HIT_NONE, rtmi.RTMI_HIT_SPHERE, rtmi.RTMI_HIT_TRIANGLE, rtmi.RTMI_HIT_PARALLELOGRAM,
         rtmi.RTMI_HIT_PARALLELEPIPED, rtmi.RTMI_HIT_MESH, rtmi.RTMI_HIT_SKY)


@functools.lru_cache(maxsize=None)
def scene(name):
    """(committed scene, its Recorder, seed) of a scene program, or of one of directlib's and mislib's scenes."""
    custom = {"lamp_room": dl.lamp_room, "close_lamp_room": ml.close_lamp_room, "odd_lights": dl.odd_lights_world,
              "many_lights": dl.many_lights_world()}
    if name in custom:
        b, rec = dl.build_custom(custom[name])
        return b, rec, dl.LAMP_ROOM_SEED
    seed = common.scene_seed(name)
    rec = Recorder(rtmi.SceneBuilder(seed))
    common.build_scene(rec, name, 1.0)
    rec.b.commit()
    return rec.b, rec, seed


@functools.lru_cache(maxsize=None)
def tables(name):
    _, rec, _ = scene(name)
    return dl.table_of(rec), dl.mat_kinds_of(rec)


def rays_of(name, n, seed=0):
    """n camera rays of the scene (its 32 x 32 frame, as many samples as n takes), float32 (n, 3) each."""
    b, _, _ = scene(name)
    O, D = dl.camera_rays(b, 32, 32, -(-n // 1024), 100 + seed)
    pick = np.random.default_rng(seed).permutation(len(O))[:n]
    return np.ascontiguousarray(O[pick]), np.ascontiguousarray(D[pick])


def _cand(n, lst):
    cand = lst.get("list_in")
    if cand is not None:
        end = min(lst.get("n_list", len(cand)), lst.get("count_in", len(cand)) if lst.get("count_in") is not None else len(cand))
        return np.asarray(cand, dtype=np.int64)[:end]
    if lst.get("n_list") is not None or lst.get("count_in") is not None:
        return np.arange(min(lst.get("n_list") if lst.get("n_list") is not None else n,
                             lst.get("count_in") if lst.get("count_in") is not None else n))
    return None


def _check_step(name, ps, step_no, sample, what, **lst):
    b, _, _ = scene(name)
    tab, kinds = tables(name)
    want = ml.step(tab, kinds, ps.copy(), step_no, sample, _cand(len(ps.O), lst))
    rc, got, intact = ml.device_step(b, ps, step_no, sample, **lst)
    assert rc == 0, rtmi.lib().rtmi_last_error()
    assert intact, (what, "a canary behind an array was overwritten")
    bad = ml.diff(got, want)
    assert bad == [], (what, bad, [np.flatnonzero((bits(getattr(got, k)) != bits(getattr(want, k))).reshape(len(ps.O), -1).any(1))[:6]
                                   for k in bad if k != "counts"])
    return want


def _every_list(name, ps, lst, k, sample):
    n = len(ps.O)
    w = _check_step(name, ps, k, sample, "null list")
    _check_step(name, ps, k, sample, "the step's list", list_in=lst)
    _check_step(name, ps, k, sample, "a count below n_list", list_in=lst, count_in=len(lst) // 2)
    _check_step(name, ps, k, sample, "a null list cut by its count", count_in=n // 2)
    holes = lst.copy()
    holes[::3] = np.resize(np.array([n, n + 5, 0x80000000, 0xffffffff], np.uint32), len(holes[::3]))
    _check_step(name, ps, k, sample, "entries >= n", list_in=holes)
    _check_step(name, ps, k, sample, "a reversed list", list_in=lst[::-1].copy())
    return w


# ------------------------------------------------------------------ 1. the step on real paths
@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("name,n_steps", [("cornell_box", 1), ("cornell_box", 3), ("lamp_room", 1), ("lamp_room", 3)])
def test_step_is_the_restatement_on_real_paths_and_real_carries(name, n_steps, n):
    b, _, seed = scene(name)
    O, D = rays_of(name, n, n_steps)
    p1, lst1 = dl.real_paths(b, O, D, seed + n, n_steps)
    ps = ml.PathState.of(p1)
    ps.flags = np.random.default_rng(n + n_steps).integers(0, 4, n).astype(np.uint32)  # bit 1 is the caller's
    k = n_steps - 1
    first = _every_list(name, ps, lst1, k, 1)
    _every_list(name, ps, lst1, k, 0)
    # the same paths one step on, with the flags and carries the sampling step left: WEIGH on real carries
    p2, lst2 = dl.real_paths(b, O, D, seed + n, n_steps + 1)
    nxt = ml.PathState.of(p2, carry=first.C)
    nxt.flags, nxt.LS = first.flags.copy(), first.LS.copy()
    weighed = 0
    for sample in (1, 0):
        w = _every_list(name, nxt, lst2, k + 1, sample)
        weighed += int(w.counts[1]) - 5
    if n >= 4133:
        assert int(first.counts[0]) - 3 > n // 4 and weighed > 0, "the case samples or weighs nothing"


# ------------------------------------------------------------------ 2. the same run against rtmi_direct_sample
@pytest.mark.parametrize("name", ["cornell_box", "lamp_room"])
def test_shadow_rays_flags_and_states_are_rtmi_direct_sample_s(name):
    b, _, seed = scene(name)
    tab, kinds = tables(name)
    n = 4133
    O, D = rays_of(name, n, 2)
    p1, lst1 = dl.real_paths(b, O, D, seed, 2)
    ps = ml.PathState.of(p1)
    first = ml.step(tab, kinds, ps.copy(), 1, 1)
    p2, lst2 = dl.real_paths(b, O, D, seed, 3)
    nxt = ml.PathState.of(p2, carry=first.C)
    nxt.flags, nxt.LS = first.flags.copy(), first.LS.copy()
    for sample in (1, 0):
        rc0, plain, ok0 = ml.device_step(b, nxt, 2, sample, list_in=lst2, mis=False)
        rc1, mis, ok1 = ml.device_step(b, nxt, 2, sample, list_in=lst2, mis=True)
        assert rc0 == 0 and rc1 == 0 and ok0 and ok1
        for k in ("SO", "SD", "ST", "flags", "LS", "O", "D", "H", "steps", "A"):
            assert np.array_equal(bits(getattr(plain, k)), bits(getattr(mis, k))), k
        assert plain.counts[0] == mis.counts[0]
        touched0 = (bits(plain.E) != bits(nxt.E)).any(1)
        touched1 = (bits(mis.E) != bits(nxt.E)).any(1)
        assert np.array_equal(touched0, touched1) and plain.counts[1] == mis.counts[1] == 5 + touched0.sum() and touched0.sum() > 0
        assert np.array_equal(bits(plain.C), bits(nxt.C))  # rtmi_direct_sample knows no carry
        # |d_direct| <= |attenuation * emission_j|, j from the same draw
        listed = np.zeros(n, bool)
        listed[lst2] = True
        sampled = listed & ((mis.flags & 1) != 0)
        LS = nxt.LS.copy()
        idx = np.flatnonzero(sampled)
        j = np.searchsorted(tab["cdf"], dl.draw01(LS, idx), side="left")
        bound = np.abs((nxt.A[idx] * tab["emission"][j]).astype(f32))
        assert (np.abs(mis.DR[idx]) <= bound).all() and (mis.DR[listed & ~sampled] == 0).all()
        assert sample == 0 or (mis.DR[idx] != 0).any()


# ------------------------------------------------------------------ 3. synthetic WEIGH cases
def _synthetic(name, extra_entries=()):
    """Paths that step 0 stepped, all flagged, whose hit records run over every table light's entry (and entries that
    have no light) x every kind x elements -1 .. 7, with carries and distances of every sort."""
    b, rec, _ = scene(name)
    tab, kinds = tables(name)
    entries = sorted(set(tab["entry"].tolist()) | {-1, 0, 1, int(tab["entry"].max()) + 1, int(tab["entry"].max()) + 1000, 1 << 30,
                                                    -(1 << 31)} | set(extra_entries))
    rows = [(k, e, f) for e in entries for k in KINDS for f in range(-1, 8)]
    carries = [(0, 1, 0, 1), (0.6, 0.8, 0, 0.5), (0, 1, 0, 0), (0, 1, 0, -0.5), (0, 1, 0, -0.0), (np.nan, 1, 0, 1), (0, 1, 0, np.nan),
               (np.inf, 0, 0, 1), (0, 1, 0, np.inf), (1e30, 1e30, 1e30, 1e30), (0, 0, 0, 1), (0.3, -0.5, 0.81, 0.77)]
    ts = [0.5, 2.0, 1e-3, 0.0, np.inf, 1e25, np.nan, 1e-30]
    n = len(rows) * len(carries)
    rng = np.random.default_rng(len(rows))
    H = np.zeros((n, 12), np.int32)
    rep = np.repeat(np.array(rows, dtype=np.int64), len(carries), axis=0)
    H[:, 7], H[:, 8], H[:, 9] = rep[:, 0], rep[:, 1].astype(np.int32), rep[:, 2]
    H[:, 0] = np.resize(np.array(ts, f32), n).view(np.int32)
    none = H[:, 7] == rtmi.RTMI_HIT_NONE
    H[none, 0] = f32(np.inf).view(np.int32)  # t = +inf with kind NONE
    Nv = rng.normal(size=(n, 3))
    H[:, 3:6] = (Nv / np.linalg.norm(Nv, axis=1, keepdims=True)).astype(f32).view(np.int32)
    H[:, 6] = rng.integers(-1, len(kinds) + 1, n)  # every material, and two that are none
    Cw = np.tile(np.array(carries, f32), (len(rows), 1))
    D = rng.normal(size=(n, 3)).astype(f32)
    D[rng.random(n) < 0.5] = 0  # half the paths ended
    O = rng.uniform(-1, 1, (n, 3)).astype(f32)
    E, A = rng.uniform(0.5, 4, (n, 3)).astype(f32), rng.uniform(0, 1, (n, 3)).astype(f32)
    LS = rng.integers(0, 1 << 32, (n, 6), dtype=np.uint64).astype(np.uint32)
    ps = ml.PathState(O, D, H, np.ones(n, np.uint32), E, A, LS, flags=np.full(n, 1, np.uint32), carry=Cw)
    return ps, tab


@pytest.mark.parametrize("name", ["furnace", "odd_lights", "lamp_room"])
def test_weigh_on_synthetic_hits(name):
    extra = {"odd_lights": (0, 1, 2, 6)}.get(name, ())
    ps, tab = _synthetic(name, extra)
    n = len(ps.O)
    for sample in (0, 1):
        w = _check_step(name, ps, 0, sample, "synthetic hits")
        j = ml.light_of_hit(tab, ps.H)
        kept = j < 0
        assert np.array_equal(bits(w.E[kept]), bits(ps.E[kept])), "a hit without a light lost emission"
        assert int(w.counts[1]) - 5 == int((~kept).sum()) > 0
        kind, entry, element = ps.H[:, 7], ps.H[:, 8], ps.H[:, 9]
        # what must be among the cases, and what became of it
        assert (kept[~np.isin(kind, dl.SURFACE_KINDS)]).all() and kept[entry < 0].all() and kept[entry > tab["entry"].max()].all()
        cw, t = ps.C[~kept], ps.H[~kept, 0].view(f32)
        with np.errstate(all="ignore"):
            zero = ~((cw[:, 3] > 0) & (t > 0) & np.isfinite(t * t))
        assert zero.any() and (bits(w.E[~kept][zero]) == 0).all(), "a weight that cannot be formed is +0.0f"
        good = np.isfinite(cw).all(1) & (cw[:, 3] > 0) & (t > 0) & (t < 10) & (np.abs(cw[:, :3]).max(1) <= 1)
        assert good.any() and (w.E[~kept][good] <= ps.E[~kept][good]).all() and (w.E[~kept][good] >= 0).all()
    if name == "furnace":
        assert len(tab) == 6 and sorted(tab["element"].tolist()) == list(range(6))
        box = (kind == rtmi.RTMI_HIT_PARALLELEPIPED) & (entry == tab["entry"][0])
        for f in range(6):
            assert (j[box & (element == f)] == np.flatnonzero(tab["element"] == f)[0]).all()
        assert kept[box & ((element < 0) | (element > 5))].all()  # element 7 among them
    if name == "odd_lights":
        lamp = int(tab["material"][0])
        shares = (ps.H[:, 6] == lamp) & np.isin(kind, (rtmi.RTMI_HIT_SPHERE, rtmi.RTMI_HIT_MESH)) & np.isin(entry, (0, 1))
        assert shares.any() and kept[shares].all()  # a sphere and a mesh face with the table light's material
        assert tab["entry"].tolist() == [6] and (j[(kind == rtmi.RTMI_HIT_TRIANGLE) & (entry == 6)] == 0).all()
    if name == "lamp_room":
        pg = int(np.flatnonzero(tab["kind"] == 0)[0])
        second = (kind == rtmi.RTMI_HIT_PARALLELOGRAM) & (entry == tab["entry"][pg]) & (element == 1)
        assert second.any() and (j[second] == pg).all()  # the second triangle of a parallelogram


# ------------------------------------------------------------------ 4. table size and list length
def test_a_table_beyond_the_lds_staging():
    name = "many_lights"
    b, _, seed = scene(name)
    tab, kinds = tables(name)
    assert len(tab) == 1100 > 1024
    n = 4133
    O, D = rays_of(name, n, 2)
    p1, lst1 = dl.real_paths(b, O, D, seed, 1)
    ps = ml.PathState.of(p1)
    first = _check_step(name, ps, 0, 1, "1100 lights")
    assert int(first.counts[0]) - 3 > n // 4
    _check_step(name, ps, 0, 1, "1100 lights, listed", list_in=lst1)
    # WEIGH against lights deep in the table: every sampled path is sent into a light of its own choosing
    nxt = first.copy()
    nxt.steps[:] = 2
    j = np.random.default_rng(4).integers(0, 1100, n)
    nxt.H[:, 7], nxt.H[:, 8], nxt.H[:, 9] = rtmi.RTMI_HIT_TRIANGLE, tab["entry"][j], 0
    nxt.H[:, 0] = np.random.default_rng(5).uniform(0.01, 6, n).astype(f32).view(np.int32)
    nxt.E[:] = tab["emission"][j]
    w = _check_step(name, nxt, 1, 0, "1100 lights, weighed")
    assert int(w.counts[1]) - 5 == int((first.flags & 1).sum())
    assert (ml.light_of_hit(tab, nxt.H) == j).all()


def test_a_list_beyond_one_round_of_the_grid():
    """The grid is capped at 8 workgroups of 256 lanes per compute unit: 2^19 lanes on 256 compute units.  A list of
    2^19 + 65 entries, most of them >= n (dropped), the paths spread over it to its last chunk."""
    name = "cornell_box"
    b, _, seed = scene(name)
    tab, kinds = tables(name)
    n, length = 4133, (1 << 19) + 65
    O, D = rays_of(name, n, 8)
    p1, _ = dl.real_paths(b, O, D, seed, 1)
    ps = ml.PathState.of(p1)
    ps.flags[:] = np.random.default_rng(1).integers(0, 2, n)
    lst = np.resize(np.array([n, 0xffffffff, n + 77, 0x80000000], np.uint32), length)
    at = np.sort(np.random.default_rng(2).choice(length - 65, n - 65, replace=False))
    lst[at] = np.arange(n - 65, dtype=np.uint32)
    lst[length - 65:] = np.arange(n - 65, n, dtype=np.uint32)  # the tail beyond the grid's stride
    w = _check_step(name, ps, 0, 1, "2^19 + 65 entries", list_in=lst)
    assert int(w.counts[0]) - 3 > n // 2
    _check_step(name, ps, 0, 1, "2^19 + 65 entries, count 2^19 + 1", list_in=lst, count_in=(1 << 19) + 1)


# ------------------------------------------------------------------ 5. unstepped and unlisted paths, arguments
def test_unstepped_and_unlisted_paths_keep_their_carry():
    name = "cornell_box"
    b, _, seed = scene(name)
    n = 330
    O, D = rays_of(name, n, 9)
    for k, i in enumerate(range(0, n, 11)):
        make_bad(O, D, i, BAD_KINDS[k % len(BAD_KINDS)])
    p1, lst = dl.real_paths(b, O, D, seed, 2, compact=False)
    assert lst is None
    ps = ml.PathState.of(p1)
    ps.flags[:] = 1
    ps.steps[5::13] += 1  # (a later step's count)
    for sample in (1, 0):
        w = _check_step(name, ps, 1, sample, "bad rays mixed in")
        off = ps.steps != 2
        assert off.sum() > 30 and (w.flags[off] == 0).all() and (w.SD[off] == 0).all() and (w.DR[off] == 0).all()
        for k in ("C", "E", "LS", "SO"):
            assert np.array_equal(bits(getattr(w, k)[off]), bits(getattr(ps, k)[off])), k
        half = np.arange(0, n, 2, dtype=np.uint32)
        w = _check_step(name, ps, 1, sample, "every other path listed", list_in=half)
        for k in ml.PathState.FIELDS:
            if k != "counts":
                assert np.array_equal(bits(getattr(w, k)[1::2]), bits(getattr(ps, k)[1::2])), k


def test_no_counters_nothing_to_do_and_bad_arguments():
    import torch
    name = "cornell_box"
    b, _, seed = scene(name)
    tab, kinds = tables(name)
    O, D = rays_of(name, 65, 4)
    p1, lst = dl.real_paths(b, O, D, seed, 1)
    ps = ml.PathState.of(p1)
    ps.flags[:] = 1
    want = ml.step(tab, kinds, ps.copy(), 0, 1)
    want.counts = ps.counts.copy()
    rc, got, intact = ml.device_step(b, ps, 0, 1, counts=False)
    assert rc == 0 and intact and ml.diff(got, want) == []
    rc, got, intact = ml.device_step(b, ps, 0, 1, n_list=0)
    assert rc == 0 and intact and ml.diff(got, ps) == []
    rc, got, intact = ml.device_step(b, ps, 0, 1, list_in=lst, count_in=0)
    assert rc == 0 and intact and ml.diff(got, ps) == []
    # every new RTMI_ERR_INVALID case, on arrays a launch could use: nothing is written
    n = len(ps.O)
    g = dl._guarded
    dev = {k: g(np.ascontiguousarray(getattr(ps, k).T) if k == "LS" else getattr(ps, k),
                dl.CANARY_F if getattr(ps, k).dtype == f32 else getattr(ps, k).dtype.type(dl.CANARY_I)) for k in ml.PathState.FIELDS}
    before = {k: v.clone() for k, v in dev.items()}
    L, stream = rtmi.lib(), C.c_void_p(torch.cuda.current_stream().cuda_stream)

    def call(change):
        a = ml.mis_args(n, None, n, None, 0, 1, dev)
        change(a)
        return L.rtmi_direct_sample_mis(b.h, C.byref(a), stream)
    assert call(lambda a: None) == 0
    torch.cuda.synchronize()
    assert not all(torch.equal(dev[k], before[k]) for k in dev)
    before = {k: v.clone() for k, v in dev.items()}
    bad = {"size - 8": lambda a: setattr(a, "size", a.size - 8), "size + 8": lambda a: setattr(a, "size", a.size + 8),
           "size 0": lambda a: setattr(a, "size", 0), "reserved": lambda a: setattr(a, "reserved", 1),
           "null carry": lambda a: setattr(a, "d_carry", None), "carry + 4": lambda a: setattr(a, "d_carry", a.d_carry + 4),
           "carry + 8": lambda a: setattr(a, "d_carry", a.d_carry + 8), "null hits": lambda a: setattr(a, "d_hits", None),
           "null direct": lambda a: setattr(a, "d_direct", None), "n < 0": lambda a: setattr(a, "n", -1),
           "n_list > n": lambda a: setattr(a, "n_list", n + 1), "step": lambda a: setattr(a, "step", rtmi.MAX_DEPTH)}
    for what, change in bad.items():
        assert call(change) == ERR_INVALID, what
    assert L.rtmi_direct_sample_mis(b.h, None, stream) == ERR_INVALID
    assert L.rtmi_direct_sample_mis(None, C.byref(ml.mis_args(n, None, n, None, 0, 1, dev)), stream) == ERR_INVALID
    torch.cuda.synchronize()
    assert all(torch.equal(dev[k], before[k]) for k in dev)
    # a null carry is fine where nothing is launched
    a = ml.mis_args(n, None, 0, None, 0, 1, dev)
    a.d_carry = None
    assert L.rtmi_direct_sample_mis(b.h, C.byref(a), stream) == 0


# ------------------------------------------------------------------ 6. 7. the loop
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


@pytest.mark.parametrize("name", ["cornell_box", "close_lamp_room"])
def test_the_paths_of_the_mis_loop_are_the_plain_loop_s(name):
    import torch
    b, _, seed = scene(name)
    n, depth = 4133, 6
    O, D = rays_of(name, n, 5)
    p, ps, ph, _, _ = _loop(b, O, D, seed, depth, False)
    q, qs, qh, ls, ls0 = _loop(b, O, D, seed, depth, "mis")
    t, _, _, lt, _ = _loop(b, O, D, seed, depth, True)
    assert torch.equal(ps, qs) and torch.equal(p.steps, q.steps)
    assert torch.equal(p.origins.view(torch.int32), q.origins.view(torch.int32))
    assert torch.equal(p.directions.view(torch.int32), q.directions.view(torch.int32))
    weighed = 0
    top = np.abs(tables(name)[0]["emission"]).max(0)
    for k in range(depth):
        made = (p.steps > k).cpu().numpy()  # the paths step k stepped: the layers of the others are never written
        assert np.array_equal(bits(p.attenuation[k].cpu().numpy())[made], bits(q.attenuation[k].cpu().numpy())[made])
        assert np.array_equal(ph[k].cpu().numpy()[made], qh[k].cpu().numpy()[made])
        pe, qe = p.emitted[k].cpu().numpy()[made], q.emitted[k].cpu().numpy()[made]
        assert ((qe >= 0) & (qe <= pe)).all()  # every emitted word is the plain loop's times a weight in [0, 1]
        weighed += int((bits(qe) != bits(pe)).any(1).sum())
        # the direct term is at most the attenuation times the brightest table light; direct=True's is unbounded
        assert (q.direct[k].cpu().numpy()[made] <= q.attenuation[k].cpu().numpy()[made] * top).all()
    assert weighed > 0 and not torch.equal(ls, ls0)
    assert torch.equal(ls, lt) and torch.equal(q.flags, t.flags)  # the draws and flags of direct=True
    assert q.carry.shape == (n, 4) and q.carry.dtype == torch.float32 and p.carry is None and t.carry is None
    assert q.direct is not None and q.occluded.shape == (depth, n) and torch.equal(q.occluded, t.occluded)
    assert not torch.equal(p.rgb, q.rgb) and not torch.equal(t.rgb, q.rgb) and torch.isfinite(q.rgb).all()


@pytest.mark.parametrize("name", ["cornell_box", "lamp_room"])
def test_depth_one_is_rtmi_trace(name):
    import torch
    b, _, seed = scene(name)
    O, D = rays_of(name, 1000, 6)
    q, qs, _, ls, ls0 = _loop(b, O, D, seed, 1, "mis")
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
    q, qs, _, ls, ls0 = _loop(b, O, D, seed, depth, "mis")
    ts = rtmi.rng_states(seed, len(O))
    t = b.trace(torch.from_numpy(O).cuda(), torch.from_numpy(D).cuda(), ts, depth).check()
    assert torch.equal(t.rgb.view(torch.int32), q.rgb.view(torch.int32)) and torch.equal(ts, qs)
    assert torch.equal(ls, ls0), "the light states were touched without a table light"


def test_direct_takes_false_true_or_mis():
    import torch
    b, _, seed = scene("cornell_box")
    O, D = rays_of("cornell_box", 64, 1)
    with pytest.raises(rtmi.RtmiError):
        b.trace_steps(torch.from_numpy(O).cuda(), torch.from_numpy(D).cuda(), rtmi.rng_states(seed, 64), 2, direct="balance",
                      light_states=rtmi.rng_states(seed, 64, first=64))


# ------------------------------------------------------------------ 8. 9. the same expectation as Trace, less variance
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
    print("%s: sum var / sum var X: direct=True %.4f  mis %.4f;  var(mis) / var(direct=True) %.4f"
          % (name, out["direct"][1].sum() / vx, out["mis"][1].sum() / vx, out["mis"][1].sum() / out["direct"][1].sum()))
    return n, out


def _same_expectation(name, spp, depth):
    n, est = estimators(name, spp, depth)
    (mx, vx), (my, vy) = est["trace"], est["mis"]
    rhs = 5 * np.sqrt(vx / n + vy / n)
    print("%s: |mean X - mean Y| %s  5 sigma %s  cap %s  (5 sigma / mean X %s)" % (name, np.abs(mx - my), rhs, 0.02 * mx, rhs / mx))
    assert (rhs <= 0.02 * mx).all(), "the test is not sharp: 5 sigma above 2 % of mean X"
    assert (np.abs(mx - my) <= rhs).all()


def test_lamp_room_has_trace_s_expectation():
    _same_expectation("lamp_room", 512, 6)


def test_cornell_box_has_trace_s_expectation():
    _same_expectation("cornell_box", 256, 10)


def test_close_lamp_room_has_trace_s_expectation():
    """The oracle's Trace on the CPU (724^2 x 1 spp): mean X 0.2676 / 0.3069 / 0.3280, var X 0.3595 / 0.3755 / 0.4330, so
    5 sqrt(2 var X / n) / mean X is 1.55 % / 1.38 % / 1.39 % at n = 2^20: the cap holds while var Y <= 2.3 var X."""
    _same_expectation("close_lamp_room", 1024, 6)


def test_mis_lowers_the_variance_where_the_lamp_is_close():
    n, est = estimators("close_lamp_room", 1024, 6)
    assert est["mis"][1].sum() < est["direct"][1].sum()


def test_mis_lowers_the_variance_on_lamp_room():
    n, est = estimators("lamp_room", 512, 6)
    assert est["mis"][1].sum() < est["trace"][1].sum()


def test_furnace_sphere_paths_average_the_albedo():
    """Paths whose primary hit is the furnace's sphere: plain Trace gives exactly rho = 0.5; the mis loop's mean at depth 4
    is within 5 standard errors of it per channel."""
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
    Y = b.trace_steps(o, d, rtmi.rng_states(seed, n), 4, compact=True, direct="mis",
                      light_states=rtmi.rng_states(seed, n, first=n)).check().rgb.double()
    mean, se = Y.mean(0).cpu().numpy(), (Y.var(0, unbiased=True) / n).sqrt().cpu().numpy()
    print("furnace: n %d  mean %s  standard error %s" % (n, mean, se))
    assert (se > 0).all() and (np.abs(mean - 0.5) <= 5 * se).all()


# ------------------------------------------------------------------ 10. the renderer
def test_render_rays_passes_mis_through():
    import torch
    b, _, seed = scene("cornell_box")
    r = rtmi.Renderer(b, 32, 32, 4, max_depth=5, post=False).init_rng()
    r.render_rays(direct="mis")
    assert r.light_states.shape == (6, r.items) and int(r.samples.max()) == 4
    assert r.carry.shape == (r.items, 4) and r.carry.dtype == torch.float32
    plain = rtmi.Renderer(b, 32, 32, 4, max_depth=5, post=False).init_rng()
    plain.render_rays()
    nee = rtmi.Renderer(b, 32, 32, 4, max_depth=5, post=False).init_rng()
    nee.render_rays(direct=True)
    assert torch.equal(r.states, plain.states)  # the same paths
    assert torch.equal(r.budget_rays, plain.budget_rays) and not torch.equal(r.sum, plain.sum) and not torch.equal(r.sum, nee.sum)
    assert torch.isfinite(r.sum).all() and getattr(plain, "carry", None) is None and nee.carry is None
