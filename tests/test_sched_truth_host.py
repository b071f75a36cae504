"""tests/sched_truth.py -- the numpy restatement the plan kernels are held to (tests/test_gpu_sched_plan.py) -- against
answers worked out by hand and written out here, so that the truth does not certify itself; the checker against plans
that are wrong in the ways it exists to catch; and the two diagnostic entries' host side: rtmi_debug_scratch_regions
against the byte formula of the scratch, rtmi_debug_schedule's argument errors.  No GPU."""
import ctypes as C

import numpy as np
import pytest

import rtmi
import sched_truth as T


def tiles_of(costs_per_item):
    """Counts of whole tiles, every item of tile t holding costs_per_item[t]."""
    return np.repeat(np.asarray(costs_per_item, np.uint32), 64)


# ------------------------------------------------------------------ tiles
def test_three_tile_order_by_hand():
    counts = tiles_of([1, 3, 2])  # costs 64, 192, 128
    cost, mx = T.tile_costs(counts)
    assert cost.tolist() == [64, 192, 128] and mx == 192
    # 255 - floor(cost * 255 / 192): 192 -> 0; 128 -> 255 - 170 = 85; 64 -> 255 - 85 = 170
    assert T.buckets(cost, mx).tolist() == [170, 0, 85]
    # dearest first: tile 1, tile 2, tile 0; the mean is 128, the dearest 1.5 times it: no outlier head
    assert T.sparse_items(cost, 1 << 20, 20) == 0
    got = fake_device(counts, None, order=[1, 2, 0], sparse_cap=1 << 20)
    T.check_plan(counts, None, got, pixel_head=False, sparse_cap=1 << 20, grid_waves=64, outlier_x10=20, head_pct=(80, 55, 30))
    for wrong in ([2, 1, 0], [1, 0, 2], [1, 1, 0]):
        with pytest.raises(AssertionError):
            T.check_plan(counts, None, fake_device(counts, None, order=wrong, sparse_cap=1 << 20), pixel_head=False,
                         sparse_cap=1 << 20, grid_waves=64, outlier_x10=20, head_pct=(80, 55, 30))


def test_bucket_edges_by_hand():
    # mx = 255: a cost is its own distance from the top; mx = 510: two costs per bucket, the edge at even costs
    assert T.buckets([255, 254, 1, 0], 255).tolist() == [0, 1, 254, 255]
    assert T.buckets([510, 509, 508, 3, 2, 1, 0], 510).tolist() == [0, 1, 1, 254, 254, 255, 255]
    assert T.buckets([0, 0], 0).tolist() == [255, 255]  # nothing costs anything: mx counts as 1


def test_outlier_tiles_by_hand():
    cost = np.array([0, 640, 0])
    # total 640; skewed: 640 * 3 >= 3 * 640 holds with equality; outliers at twice the mean: 640 * 3 * 10 >= 20 * 640 only
    assert T.sparse_items(cost, 128, 20) == 64 and T.sparse_items(cost, 32, 20) == 32
    assert T.sparse_items(np.array([1, 640, 0]), 128, 20) == 0  # 1920 < 3 * 641: one below the gate
    # 35 tenths: 640 * 30 = 19200 < 35 * 640 = 22400: the frame is skewed but no tile is an outlier
    assert T.sparse_items(cost, 128, 35) == 0 and T.sparse_items(cost, 128, 30) == 64
    # four tiles 10, 10, 10, 90 (mean 30): skewed (360 >= 360); at 10 tenths only the tile of 90 reaches the mean
    assert T.sparse_items(np.array([10, 10, 10, 90]), 1024, 10) == 64
    assert T.sparse_items(np.array([30, 30, 30, 30]), 1024, 10) == 0  # every tile at the mean, but not skewed
    # the stated rule for a frame without cost: skewed, every tile an outlier
    assert T.sparse_items(np.zeros(5, np.int64), 1024, 20) == 320 and T.sparse_items(np.zeros(5, np.int64), 192, 20) == 192


# ------------------------------------------------------------------ head
def head_counts():
    """Two tiles: 2 pixels of 100, 3 of 60, 5 of 30, 118 of 1: total 648, largest 100 (100 * 128 >= 3 * 648: skewed)."""
    c = np.ones(128, np.uint32)
    c[[5, 70]] = 100
    c[[0, 64, 127]] = 60
    c[[1, 2, 3, 65, 126]] = 30
    return c


@pytest.mark.parametrize("grid_waves, fallbacks, ends, thresholds", [
    (24, 0, (2, 5, 10), (80, 50, 25)),            # 2 + ceil(3 / 2) + ceil(5 / 4) = 6 waves = 24 / 4: fits exactly
    (23, 1, (2, 5, 5), (80, 50, 50)),             # 23 / 4 = 5 < 6: the lightest class goes, 2 + 2 = 4 fits
    (15, 2, (0, 5, 5), (T.NONE, 50, 50)),         # 3 < 4: the heaviest share waves, ceil(5 / 2) = 3 fits
    (11, 3, (0, 0, 0), (T.NONE, T.NONE, T.NONE)),  # 2 < 3: no head
])
def test_each_fallback_of_the_head_by_hand(grid_waves, fallbacks, ends, thresholds):
    c = head_counts()
    hp = T.head_plan(c, grid_waves, (80, 50, 25))
    assert hp["cmax"] == 100 and hp["total"] == 648 and hp["skewed"] and hp["classes"] == (2, 3, 5)
    assert (hp["fallbacks"], hp["ends"], hp["thresholds"]) == (fallbacks, ends, thresholds)
    want = {0: ([5, 70], [0, 64, 127], [1, 2, 3, 65, 126]), 1: ([5, 70], [0, 64, 127], []), 2: ([], [0, 5, 64, 70, 127], []),
            3: ([], [], [])}[fallbacks]
    assert [m.tolist() for m in hp["members"]] == [list(w) for w in want]
    got = fake_device(c, None, pixel_head=True, grid_waves=grid_waves, head_pct=(80, 50, 25))
    kw = dict(pixel_head=True, sparse_cap=0, grid_waves=grid_waves, outlier_x10=20, head_pct=(80, 50, 25))
    T.check_plan(c, None, got, **kw)
    if ends[2]:
        twice = dict(got, head=got["head"].copy())
        twice["head"][ends[2] - 1] = twice["head"][0]  # a pixel listed twice (another one missing)
        with pytest.raises(AssertionError):
            T.check_plan(c, None, twice, **kw)
        unmarked = dict(got, marked=got["marked"].copy())
        unmarked["marked"][got["head"][0]] &= 0x7fffffff  # listed, but not marked
        with pytest.raises(AssertionError):
            T.check_plan(c, None, unmarked, **kw)
    changed = dict(got, marked=got["marked"].copy())
    changed["marked"][9] += 1
    with pytest.raises(AssertionError):
        T.check_plan(c, None, changed, **kw)


def test_head_gate_and_ceil_thresholds_by_hand():
    c = np.zeros(128, np.uint32)
    c[17] = 3  # 3 * 128 >= 3 * 3, but the largest count is below 4: no head
    hp = T.head_plan(c, 1024, (80, 50, 25))
    assert not hp["skewed"] and hp["ends"] == (0, 0, 0) and hp["thresholds"] == (T.NONE,) * 3
    c[17] = 4  # thresholds ceil(3.2) = 4, 2, 1: pixel 17 alone, in the heaviest class; one wave = 4 / 4
    hp = T.head_plan(c, 4, (80, 50, 25))
    assert hp["skewed"] and hp["thresholds"] == (4, 2, 1) and hp["ends"] == (1, 1, 1) and hp["members"][0].tolist() == [17]
    assert T.head_plan(c, 3, (80, 50, 25))["ends"] == (0, 0, 0)  # 3 / 4 = 0 waves: all three fallbacks
    # the mean gate: 12 * 128 = 1536 = 3 * 512 holds with equality; one more count anywhere and it does not
    c = np.full(128, 4, np.uint32)
    c[0], c[1], c[2] = 12, 0, 0
    assert c.sum() == 512 and T.head_plan(c, 1024, (80, 50, 25))["skewed"]
    c[1] = 1
    assert not T.head_plan(c, 1024, (80, 50, 25))["skewed"]
    # ceil: 101 * 50 % = 50.5 -> 51; a pixel of 50 is outside, one of 51 inside
    c = np.zeros(128, np.uint32)
    c[0], c[1], c[2] = 101, 51, 50
    hp = T.head_plan(c, 1024, (50, 50, 50))
    assert hp["thresholds"] == (51, 51, 51) and hp["classes"] == (2, 0, 0) and hp["members"][0].tolist() == [0, 1]
    # more entries than the list holds: every fallback fires whatever the grid
    c = np.zeros(64 * 1024, np.uint32)
    c[:T.HEAD_CAP + 1] = 8
    assert T.head_plan(c, 1 << 30, (80, 50, 25))["fallbacks"] == 3
    c[T.HEAD_CAP] = 0
    assert T.head_plan(c, 1 << 30, (80, 50, 25))["ends"] == (T.HEAD_CAP,) * 3


# ------------------------------------------------------------------ quarters
def test_quarter_costs_and_snake_by_hand():
    work = np.ones(64, np.uint32)
    counts = np.full(64, 2, np.uint32)
    counts[40] = 7 | T.MARK  # a head pixel: its mark is not cost
    q, qmx = T.quarter_costs(work, counts)
    assert q.tolist() == [48, 48, 53, 48] and qmx == 53
    # two tiles, eight quarters sorted 7..0: wave 0 gets ranks 0, 3, 4, 7, wave 1 ranks 1, 2, 5, 6
    assert T.snake([7, 6, 5, 4, 3, 2, 1, 0]).tolist() == [7, 4, 3, 0, 6, 5, 2, 1]
    assert T.snake([9, 8, 7, 6]).tolist() == [9, 8, 7, 6]  # one tile: ranks 0, 1, 2, 3
    assert T.expand_order([2, 0, 1]).tolist() == [8, 9, 10, 11, 0, 1, 2, 3, 4, 5, 6, 7]


# ------------------------------------------------------------------ chains
def test_two_by_two_chains_over_seven_tiles_by_hand():
    """S = 2 SIMDs x R = 2 waves.  Ranks are dealt to the SIMDs boustrophedon, row k of two ranks at a time: row 0 -> s 0,
    1; row 1 -> s 1, 0; row 2 -> s 0, 1; row 3 -> s 1, (0).  A SIMD's k-th tile goes to its waves boustrophedon too: k 0, 1 ->
    r 0, 1; k 2, 3 -> r 1, 0.  So chain c = 2 r + s holds the ranks: c0 {0, (7)}, c1 {1, 6}, c2 {3, 4}, c3 {2, 5}."""
    ranks = {0: [0, 7], 1: [1, 6], 2: [3, 4], 3: [2, 5]}
    for c, want in ranks.items():
        assert [T.chain_rank(j, c % 2, c // 2, 2, 2) for j in range(2)] == want
    order = [3, 0, 6, 2, 5, 1, 4]
    cost = [10, 20, 30, 40, 50, 60, 70]  # by tile
    # in tiles: c0 [3], c1 [0, 4], c2 [2, 5], c3 [6, 1]
    first, nxt, fut = T.chain_plan(order, cost, 2, 2, 128, 2)  # scale 128 / (64 * 2) = 1
    assert first.tolist() == [3, 0, 2, 6]
    assert nxt.tolist() == [4, -1, 5, -1, -1, -1, 1]
    assert fut.tolist() == [50, 0, 60, 0, 0, 0, 20]
    assert T.walk_chains(first, nxt, 7).tolist() == [1] * 7
    # scale 100 / 192 = 0.52083...: 50 -> 26.04, 60 -> 31.25, 20 -> 10.42, truncated
    assert T.chain_plan(order, cost, 2, 2, 100, 3)[2].tolist() == [26, 0, 31, 0, 0, 0, 10]
    # one chain of all seven: what follows a tile adds up from the far end
    first, nxt, fut = T.chain_plan(order, cost, 1, 1, 128, 2)
    assert first.tolist() == [3] and [int(nxt[t]) for t in order] == [0, 6, 2, 5, 1, 4, -1]
    assert [int(fut[t]) for t in order] == [240, 230, 160, 130, 70, 50, 0]
    # saturation: scale 2^30 / 64 = 2^24; 20 * 2^24 = 335,544,320; + 60 * 2^24 = 1,342,177,280; + 250 * 2^24 > 4e9
    fut = T.chain_plan([0, 1, 2, 3], [7, 250, 60, 20], 1, 1, 1 << 30, 1)[2]
    assert fut.tolist() == [4000000000, 1342177280, 335544320, 0]
    # more chains than tiles: the chains past the last tile are empty
    first, nxt, _ = T.chain_plan([1, 0], [5, 9], 2, 2, 64, 1)
    assert first.tolist() == [1, 0, -1, -1] and nxt.tolist() == [-1, -1]


def test_chain_ranks_deal_every_rank_once():
    """The same dealing stated the other way round -- from a rank to its chain and step -- agrees with chain_rank."""
    for S, R, n in ((1, 1, 5), (2, 2, 7), (3, 2, 20), (4, 3, 50), (5, 1, 13), (1, 4, 9)):
        for p in range(n):
            k, pos = divmod(p, S)
            s = S - 1 - pos if k & 1 else pos
            j, rr = divmod(k, R)
            r = R - 1 - rr if j & 1 else rr
            assert T.chain_rank(j, s, r, S, R) == p


def test_the_checker_sees_a_wrong_chain_plan():
    rng = np.random.default_rng(3)
    counts = rng.integers(1, 40, 64 * 9).astype(np.uint32)
    kw = dict(pixel_head=False, sparse_cap=64, grid_waves=16, outlier_x10=20, head_pct=(80, 55, 30), simds=2, rounds=2, spp=256,
              probe_spp=4)
    got = fake_device(counts, None, **kw)
    T.check_plan(counts, None, got, **kw)
    for name, at, value in (("next", 0, -1 if got["next"][0] != -1 else 1), ("fut", int(got["first"][0]), 1 << 20),
                            ("first", 3, int(got["first"][2])), ("claims", 4, 1)):
        bad = dict(got)
        bad[name] = got[name].copy()
        bad[name][at] = value
        with pytest.raises(AssertionError):
            T.check_plan(counts, None, bad, **kw)
    # a plan that leaves tiles out, or one that loops, is a structural failure of its own
    assert T.walk_chains(got["first"][:3], got["next"], 9).sum() < 9
    loop = got["next"].copy()
    loop[loop == -1] = got["first"][0]
    with pytest.raises(AssertionError):
        T.walk_chains(got["first"][:4], loop, 9)


def test_the_checker_sees_a_wrong_snake():
    rng = np.random.default_rng(4)
    counts = rng.integers(1, 40, 64 * 5).astype(np.uint32)
    work = rng.integers(0, 900, 64 * 5).astype(np.uint32)
    kw = dict(pixel_head=False, sparse_cap=64, grid_waves=16, outlier_x10=20, head_pct=(80, 55, 30))
    got = fake_device(counts, work, **kw)
    T.check_plan(counts, work, got, **kw)
    bad = dict(got, qmap=got["qmap"].copy())
    bad["qmap"][[1, 5]] = bad["qmap"][[5, 1]]  # still a permutation, not the snake
    with pytest.raises(AssertionError):
        T.check_plan(counts, work, bad, **kw)
    bad = dict(got, qsorted=got["qsorted"][::-1].copy())  # cheapest first
    bad["qmap"] = T.snake(bad["qsorted"]).astype(np.uint32)
    with pytest.raises(AssertionError):
        T.check_plan(counts, work, bad, **kw)


def fake_device(counts, work, order=None, pixel_head=False, sparse_cap=0, grid_waves=0, outlier_x10=20, head_pct=(80, 55, 30),
                simds=0, rounds=0, spp=1, probe_spp=1):
    """What a device that follows the contract would leave (ties in index order), as check_plan's `got`."""
    counts = np.asarray(counts, np.uint32)
    nt = counts.size // 64
    cost, mx = T.tile_costs(counts)
    if order is None:
        order = np.lexsort((np.arange(nt), T.buckets(cost, mx)))
    order = np.asarray(order, np.int64)
    meta = np.zeros(32, np.int64)
    meta[0], meta[1] = mx, T.sparse_items(cost, sparse_cap, outlier_x10)
    marked = counts.astype(np.int64)
    head = np.zeros(T.HEAD_CAP, np.int64)
    if pixel_head:
        hp = T.head_plan(counts, grid_waves, head_pct)
        e = hp["ends"]
        meta[1:4] = (e[2], e[0], e[1])
        meta[16], meta[18], meta[19] = hp["cmax"], hp["total"] & 0xffffffff, hp["total"] >> 32
        meta[20:23], meta[24:27], meta[28:31] = hp["classes"], hp["thresholds"], e
        listed = np.concatenate(hp["members"])
        head[:listed.size] = listed
        marked[listed] |= T.MARK
    got = dict(cost=cost, order=order, meta=meta, head=head, marked=marked, qmax=np.zeros(4, np.int64))
    if work is not None:
        q, qmx = T.quarter_costs(work, marked)
        got["qcost"], got["qmax"][0] = q, qmx
        got["qsorted"] = np.lexsort((np.arange(4 * nt), T.buckets(q, qmx)))
        got["qmap"] = T.snake(got["qsorted"])
    else:
        got["qmap"] = T.expand_order(order)
    if simds * rounds:
        first = np.full(T.CHAIN_CAP, 77, np.int64)  # (the words past simds * rounds are nobody's)
        first[:simds * rounds], got["next"], got["fut"] = T.chain_plan(order, cost, simds, rounds, spp, probe_spp)
        got["first"], got["claims"] = first, np.zeros(nt, np.int64)
    return got


# ------------------------------------------------------------------ the library's host side
FRAMES = [(8, 8, 1), (8, 24, 1), (1024, 1024, 64), (2048, 2048, 4096, 64, True, 3, 8), (720, 1280, 20, 50),
          (17, 999, 2, 64, False, 6, 7), (8, 8 * 4097, 1)]


@pytest.mark.parametrize("frame", FRAMES)
def test_scratch_regions_follow_the_byte_formula(frame):
    """rtmi_debug_scratch_regions against the layout as test_host_logic.py spells it out: the call's counters, states
    copy, probe counts, tile costs and order, 32 words, the head list, the probe's work counts, per quarter tile cost /
    sorted / order, 4 words, per tile follows / next / claim, per chain its first tile, rounded up to 256; the
    wave-priority table; two kernel-argument blocks."""
    f = rtmi.make_frame(*frame)
    n = rtmi.work_items(f)
    nt = n // 64
    sizes = [("states", n * 6 * 4), ("rays", n * 4), ("cost", nt * 4), ("order", nt * 4), ("meta", 128), ("head", 16384 * 4),
             ("work", n * 4), ("qcost", nt * 16), ("qsorted", nt * 16), ("qmap", nt * 16), ("qmax", 16), ("fut", nt * 4),
             ("next", nt * 4), ("claims", nt * 4), ("first", 32768 * 4)]
    assert tuple(name for name, _ in sizes) + ("prio_tab", "params", "total") == rtmi.SCRATCH_REGIONS
    got = rtmi.scratch_regions(f)
    at = 40 * 8
    for name, size in sizes:
        assert got[name] == at, name
        at += size
    at = (at + 255) & ~255
    assert got["prio_tab"] == at and got["params"] == at + (1 << 14) * 16 * 4
    total = rtmi.lib().rtmi_render_scratch_bytes(C.byref(f))
    block = (total - got["params"]) // 2
    assert got["total"] == total == got["params"] + 2 * block and block % 256 == 0 and 512 <= block <= 2048
    assert got["meta"] % 8 == 0  # (head_scan_kernel adds to a 64-bit word of it)


def test_scratch_regions_arguments():
    L = rtmi.lib()
    f = rtmi.make_frame(16, 16, 1)
    out = (C.c_int64 * 20)(*([-7] * 20))
    assert L.rtmi_debug_scratch_regions(C.byref(f), out, 3) == 0 and list(out[:4]) == [320, 320 + 256 * 24, 320 + 256 * 28, -7]
    assert L.rtmi_debug_scratch_regions(C.byref(f), out, 20) == 0 and out[17] == L.rtmi_render_scratch_bytes(C.byref(f))
    assert out[18] == -7  # never more than RTMI_SCRATCH_REGIONS words
    assert L.rtmi_debug_scratch_regions(None, out, 18) == -1 and L.rtmi_debug_scratch_regions(C.byref(f), None, 18) == -1
    bad = rtmi.make_frame(0, 8, 1)
    assert L.rtmi_debug_scratch_regions(C.byref(bad), out, 18) == -1 and b"bad frame" in L.rtmi_last_error()


def test_debug_schedule_argument_errors():
    """Argument errors of rtmi_debug_schedule come before any device work (the pointers here are never dereferenced)."""
    L = rtmi.lib()
    f = rtmi.make_frame(8, 24, 1)
    need = L.rtmi_render_scratch_bytes(C.byref(f))
    p = C.c_void_p(256)
    pct = lambda *v: (C.c_int32 * 3)(*v)

    def call(frame=f, scratch=p, size=need, rays=p, work=None, head=1, cap=64, waves=64, x10=20, hp=pct(80, 55, 30), simds=0,
             rounds=0, spp=64, probe=2):
        return L.rtmi_debug_schedule(C.byref(frame) if frame is not None else None, scratch, size, rays, work, head, cap, waves,
                                     x10, hp, simds, rounds, spp, probe, None)
    for kw in (dict(frame=None), dict(scratch=None), dict(rays=None), dict(hp=None)):
        assert call(**kw) == -1 and b"null" in L.rtmi_last_error(), kw
    assert call(frame=rtmi.make_frame(8, 0, 1)) == -1 and b"bad frame" in L.rtmi_last_error()
    assert call(size=need - 1) == -1 and b"scratch_bytes" in L.rtmi_last_error()
    for v in ((101, 50, 20), (50, -1, -1), (50, 20, -3)):
        assert call(hp=pct(*v)) == -1 and b"head_pct outside" in L.rtmi_last_error(), v
    for v in ((40, 50, 30), (50, 30, 40)):
        assert call(hp=pct(*v)) == -1 and b"must not increase" in L.rtmi_last_error(), v
    for kw in (dict(simds=32769, rounds=1), dict(simds=256, rounds=129), dict(simds=1 << 20, rounds=1 << 20)):
        assert call(**kw) == -1 and b"chain cap" in L.rtmi_last_error(), kw
    assert call(simds=-1, rounds=1) == -1 and call(waves=-1) == -1 and call(x10=-1) == -1
    assert call(simds=4, rounds=2, probe=0) == -1 and call(simds=4, rounds=2, spp=0) == -1
    if L.rtmi_device_count() == 0:  # every argument is fine: without a GPU it fails like every compute entry
        for kw in (dict(), dict(simds=256, rounds=128), dict(hp=pct(50, 50, 50), head=0)):
            assert call(**kw) == -2 and b"no CPU fallback" in L.rtmi_last_error(), kw
