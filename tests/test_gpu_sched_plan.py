"""The eleven kernels that plan a scheduled render (csrc/sched.hip: tile_cost, tile_order, head_scan / count / plan /
scatter, expand_order, quarter_cost / sort, snake_map, chain_link) against tests/sched_truth.py, through
rtmi_debug_schedule -- the scheduler step of rtmi_render_ex on synthetic counts -- and, for run_plan's wiring of it, on
the scratch one list render and one mesh render leave behind.

The image tests cannot see a wrong plan: the trace kernel renders every tile once whatever the chains say, and the
queue's order, the snake, the head's classes and thresholds only decide who renders what when.

Every case runs the step once; the scratch starts as 0xAB bytes, so a word the step should have written and did not
shows.  What the device's atomics decide (the order within a cost bucket or a head class) is compared as
sched_truth.check_plan says; everything else for equality, chain_fut included."""
import numpy as np
import pytest

import rtmi
import sched_truth as T

pytestmark = pytest.mark.gpu

TILE_COUNTS = (1, 2, 3, 255, 256, 257, 1023, 1024, 1025, 4097, 65600)  # 65600: past the head kernels' cap of 1024 workgroups
COUNT_MAX = 64 * 65  # the real ceiling of a probe's count: 64 samples of 65 queries
PCT = (80, 55, 30)


def frame_of(nt):
    """A frame of nt local tiles: 8 x 8 nt while that is a legal width, else 40 x 1640 tiles."""
    if 8 * nt <= 65535:
        return rtmi.make_frame(8, 8 * nt, 1)
    assert nt == 40 * 1640
    return rtmi.make_frame(8 * 40, 8 * 1640, 1)


def run_step(counts, work=None, **kw):
    """One rtmi_debug_schedule on `counts` (uint32 per work item) and optional `work`; returns check_plan's `got`."""
    import torch
    counts = np.ascontiguousarray(counts, np.uint32)
    nt = counts.size // 64
    f = frame_of(nt)
    assert rtmi.work_items(f) == counts.size
    reg = rtmi.scratch_regions(f)
    scratch = torch.full((reg["total"],), 0xAB, dtype=torch.uint8, device="cuda")
    d_counts = torch.from_numpy(counts.view(np.int32)).cuda()
    d_work = torch.from_numpy(np.ascontiguousarray(work, np.uint32).view(np.int32)).cuda() if work is not None else None
    rtmi.debug_schedule(f, scratch, d_counts, d_work, **kw)
    torch.cuda.synchronize()
    raw = np.zeros(reg["total"], np.uint8)  # (only the scheduler's regions come back: the states copy is most of the scratch)
    raw[reg["cost"]:reg["prio_tab"]] = scratch[reg["cost"]:reg["prio_tab"]].cpu().numpy()
    got = T.plan_arrays(raw, reg, nt)
    got["marked"] = d_counts.cpu().numpy().view(np.uint32)
    # the step must not write outside its regions
    assert bool((scratch[:reg["cost"]] == 0xAB).all()) and bool((scratch[reg["prio_tab"]:] == 0xAB).all())
    return got


def check(counts, work=None, pixel_head=False, sparse_cap=0, grid_waves=0, outlier_x10=20, head_pct=PCT, simds=0, rounds=0, spp=1,
          probe_spp=1):
    kw = dict(pixel_head=pixel_head, sparse_cap=sparse_cap, grid_waves=grid_waves, outlier_x10=outlier_x10, head_pct=head_pct,
              simds=simds, rounds=rounds, spp=spp, probe_spp=probe_spp)
    got = run_step(counts, work, **kw)
    hp = T.check_plan(counts, work, got, **kw)
    if work is None:  # the quarter sort did not run: its regions are untouched
        assert all((got[k] == 0xABABABAB).all() for k in ("qcost", "qsorted", "qmax"))
    if simds * rounds == 0:
        assert all((got[k].view(np.uint32) == 0xABABABAB).all() for k in ("fut", "next", "claims", "first"))
    else:
        assert (got["first"][simds * rounds:].view(np.uint32) == 0xABABABAB).all()
    if not pixel_head:
        assert (got["head"] == 0xABABABAB).all()
    return got, hp


# ------------------------------------------------------------------ count distributions
def rng_of(*key):
    return np.random.default_rng([20260117, *key])


def tile_with_cost(cost):
    """64 counts that add up to `cost`, as even as they can be."""
    t = np.full(64, cost // 64, np.int64)
    t[:cost % 64] += 1
    return t


def counts_of_costs(costs):
    return np.concatenate([tile_with_cost(int(c)) for c in costs]).astype(np.uint32)


def random_counts(nt, key, hi=COUNT_MAX):
    """Counts up to the ceiling, most of them small, with padding items (0) inside tiles: columns and rows cut off."""
    r = rng_of(nt, key)
    c = r.integers(0, 40, 64 * nt)
    hot = r.random(64 * nt) < 0.01
    c[hot] = r.integers(0, hi + 1, int(hot.sum()))
    c = c.reshape(nt, 8, 8)
    c[r.random(nt) < 0.1, :, 5:] = 0   # a ragged right edge
    c[r.random(nt) < 0.1, 3:, :] = 0   # a ragged bottom edge
    c.reshape(-1)[r.integers(0, 64 * nt)] = hi
    return c.reshape(-1).astype(np.uint32)


def skewed_counts(nt, key, cmax=4157):
    """A frame with a head: mostly 1 .. 3, a sprinkle of pixels around the three thresholds of PCT, one at cmax."""
    r = rng_of(nt, key)
    n = 64 * nt
    c = r.integers(1, 4, n)
    t = [(cmax * p + 99) // 100 for p in PCT]
    k = min(max(1, n // 200), 2000)  # (seven sprinkles: the head list holds them all)
    for v in (t[0], t[0] - 1, t[1], t[1] - 1, t[2], t[2] - 1):
        c[r.integers(0, n, k)] = v
    c[r.integers(0, n, k)] = r.integers(t[2], cmax, k)
    c[r.integers(0, n)] = cmax
    return c.astype(np.uint32)


def chain_shapes(nt):
    """(S, R) relative to the tile count: one chain; S = 1; R = 1 (two SIMDs: the deal turns round from the third tile
    on); nt no multiple of S; more chains than tiles; the cap."""
    if nt > 5000:  # (the restatement walks every chain in Python: three shapes are enough at this size)
        return [(1, 1), (7, 3), (256, 128)]
    shapes = {(1, 1), (1, 3), (2, 1), (min(nt, 5), 1), (nt // 3 + 2, 2), (nt + 1, 2), (256, 128)}
    if nt % 7:
        shapes.add((7, 3))
    return sorted(shapes)


# ------------------------------------------------------------------ every tile count
@pytest.mark.parametrize("nt", TILE_COUNTS)
def test_tile_order_and_chains_at_every_tile_count(nt):
    """Outlier-tile mode, the queue in tile order, and every chain shape, on counts up to the real ceiling with padding
    inside tiles.  fut without saturation (64 spp after 2) and, for the cap's shape, with (2^20 spp after 1)."""
    counts = random_counts(nt, 0)
    for i, (S, R) in enumerate(chain_shapes(nt)):
        sat = (S, R) == (256, 128) or i == 0
        got, _ = check(counts, sparse_cap=64 * (i + 1), grid_waves=S * R, outlier_x10=(10, 20, 35)[i % 3], simds=S, rounds=R,
                       spp=1 << 20 if sat else 64, probe_spp=1 if sat else 2)
        if (S, R) == (1, 1) and nt >= 255:  # one chain of every tile at 2^14 per ray: what follows its first tiles is past 4e9
            assert (got["fut"] == 4000000000).any(), "the case is meant to saturate fut"
        if not sat:
            assert (got["fut"] < 4000000000).all(), "the case is meant not to saturate fut"


@pytest.mark.parametrize("nt", TILE_COUNTS)
def test_pixel_head_and_quarter_snake_at_every_tile_count(nt):
    """The pixel head (counts at each threshold and one below) and, with work counts, the quarter sort and its snake over
    counts that carry the head's marks; a grid so large that no limit of the head binds, then one that drops classes."""
    counts = skewed_counts(nt, 1)
    work = rng_of(nt, 2).integers(0, 5000, 64 * nt).astype(np.uint32)
    _, hp = check(counts, work, pixel_head=True, grid_waves=1 << 20)
    assert hp["skewed"] and hp["fallbacks"] == 0 and hp["ends"][2] > 0 and (nt < 3 or min(hp["classes"]) > 0)
    need = hp["classes"][0] + (hp["classes"][1] + 1) // 2 + (hp["classes"][2] + 3) // 4
    check(counts, None, pixel_head=True, grid_waves=4 * need - 1)  # one wave short: the lightest class goes
    check(random_counts(nt, 3), work, pixel_head=True, grid_waves=1 << 20, simds=min(nt, 3), rounds=2, spp=512, probe_spp=32)


# ------------------------------------------------------------------ count distributions, at sizes around one workgroup's stride
@pytest.mark.parametrize("nt", (5, 257, 1025))
def test_equal_zero_and_one_hot_counts(nt):
    work = rng_of(nt, 4).integers(0, 99, 64 * nt).astype(np.uint32)
    for head in (False, True):
        equal = np.full(64 * nt, 7, np.uint32)
        got, hp = check(equal, work if head else None, pixel_head=head, sparse_cap=1 << 20, grid_waves=1024, simds=4, rounds=2,
                        spp=64, probe_spp=2)
        assert got["meta"][1] == 0  # neither outlier tiles nor a head in a flat frame
        zero = np.zeros(64 * nt, np.uint32)
        got, hp = check(zero, np.zeros(64 * nt, np.uint32) if head else None, pixel_head=head, sparse_cap=128, grid_waves=1024,
                        simds=2, rounds=2, spp=64, probe_spp=2)
        # the stated rule: a frame without cost is skewed and all of its tiles are outliers -- but it has no head
        assert got["meta"][0] == 0 and got["meta"][1] == (0 if head else min(64 * nt, 128))
        hot = np.ones(64 * nt, np.uint32)
        hot[64 * nt - 9] = COUNT_MAX
        got, hp = check(hot, work if head else None, pixel_head=head, sparse_cap=1 << 20, grid_waves=1024)
        assert got["meta"][1] == (1 if head else 64)
        if head:
            assert got["head"][0] == 64 * nt - 9 and hp["ends"] == (1, 1, 1)


@pytest.mark.parametrize("nt", (255, 1025))
def test_costs_on_bucket_edges(nt):
    """mx = 4080 = 255 * 16: a cost sits exactly on a bucket's edge when it is a multiple of 16.  Tiles at m * 16 and one
    below, for every m; the quarter costs likewise (mx 1020 = 255 * 4: multiples of 4)."""
    r = rng_of(nt, 5)
    m = r.integers(1, 256, nt)
    costs = m * 16 - (np.arange(nt) & 1)
    costs[0], costs[1], costs[2] = 4080, 16, 15
    counts = counts_of_costs(costs)
    cost, mx = T.tile_costs(counts)
    assert mx == 4080 and ((cost * 255) % mx == 0).sum() >= nt // 2 - 1 and ((cost + 1) * 255 % mx == 0).sum() >= nt // 2 - 1
    check(counts, sparse_cap=640, grid_waves=64, simds=3, rounds=3, spp=64, probe_spp=2)
    # quarters: 16 items each, work 0, so a quarter's cost is the sum of its counts
    q = r.integers(1, 256, 4 * nt) * 4 - (np.arange(4 * nt) & 1)
    q[0] = 1020
    qc = np.zeros((4 * nt, 16), np.uint32)
    qc[:] = (q // 16)[:, None]
    for i in range(4 * nt):
        qc[i, :q[i] % 16] += 1
    assert (qc.sum(axis=1) == q).all()
    check(qc.reshape(-1), np.zeros(64 * nt, np.uint32), sparse_cap=0, grid_waves=64)


@pytest.mark.parametrize("nt", (3, 4, 257, 65600))
def test_the_three_times_the_mean_gate_of_outlier_tiles(nt):
    """mx * n exactly 3 * total (skewed), and one count more (not skewed): tile 0 costs 3 (n - 1), every other n - 3."""
    costs = np.full(nt, nt - 3, np.int64)
    costs[0] = 3 * (nt - 1)
    counts = counts_of_costs(costs)
    cost, mx = T.tile_costs(counts)
    assert mx * nt == 3 * cost.sum()
    for x10, cap in ((10, 1 << 20), (20, 1 << 20), (35, 1 << 20), (20, 0)):
        got, _ = check(counts, sparse_cap=cap, outlier_x10=x10, grid_waves=64)
        # tile 0 costs 3 (n - 1) / (n - 1) = three times the mean exactly: an outlier at 10, 20 and (as 30 >= 35 fails) not at 35;
        # the others cost (n - 3) / (n - 1) of the mean: none reaches it
        assert got["meta"][1] == min(cap, 0 if x10 == 35 else 64)
    counts[64 * nt - 1] += 1
    got, _ = check(counts, sparse_cap=1 << 20, outlier_x10=10, grid_waves=64)
    assert got["meta"][1] == 0


@pytest.mark.parametrize("nt", (257, 4097))
def test_outlier_tiles_against_the_cap(nt):
    """sparse_cap above, at and below 64 x the outliers, at 10, 20 and 35 tenths of the mean."""
    r = rng_of(nt, 6)
    costs = r.integers(50, 150, nt)
    costs[r.integers(0, nt, max(3, nt // 50))] = r.integers(150, 900, max(3, nt // 50))
    costs[7] = 4000
    counts = counts_of_costs(costs)
    for x10 in (10, 20, 35):
        cost = T.tile_costs(counts)[0]
        outliers = int((cost * nt * 10 >= x10 * cost.sum()).sum())
        assert outliers >= 2
        for cap in (64 * outliers + 64, 64 * outliers, 64 * outliers - 64):
            got, _ = check(counts, sparse_cap=cap, outlier_x10=x10, grid_waves=64)
            assert got["meta"][1] == min(cap, 64 * outliers)


# ------------------------------------------------------------------ the head's gates and limits
def test_head_gate_at_a_largest_count_of_three_and_four():
    for nt in (1, 257):
        c = np.zeros(64 * nt, np.uint32)
        c[[11, 64 * nt - 1]] = 3
        got, hp = check(c, pixel_head=True, grid_waves=1024)
        assert not hp["skewed"] and got["meta"][1] == 0
        c[11] = 4  # thresholds 4, 3, 2: both pixels are listed, in the first two classes
        got, hp = check(c, pixel_head=True, grid_waves=1024)
        assert hp["ends"] == (1, 2, 2) and got["head"][:2].tolist() == [11, 64 * nt - 1]


def test_head_mean_gate_exactly_and_one_below():
    """cmax * n = 3 * total exactly (a head), and one count more (none)."""
    for nt in (2, 1025):
        n = 64 * nt
        c = np.full(n, 4, np.uint32)
        c[5], c[6], c[7] = 12, 0, 0  # the sum stays 4 n, the largest is 12
        assert 12 * n == 3 * int(c.sum())
        got, hp = check(c, pixel_head=True, grid_waves=1 << 20, head_pct=(80, 50, 40))
        assert hp["skewed"] and hp["ends"] == (1, 1, 1) and got["head"][0] == 5
        c[6] = 1
        got, hp = check(c, pixel_head=True, grid_waves=1 << 20, head_pct=(80, 50, 40))
        assert not hp["skewed"] and got["meta"][1] == 0


def limits_population(nt, a, b, c3, key):
    """a pixels of 100, b of 60, c3 of 30 at random places among ones; with PCT-like (80, 50, 25): thresholds 80, 50, 25."""
    n = 64 * nt
    c = np.ones(n, np.uint32)
    at = rng_of(nt, key).permutation(n)[:a + b + c3]
    c[at[:a]], c[at[a:a + b]], c[at[a + b:]] = 100, 60, 30
    return c


@pytest.mark.parametrize("nt, classes", [(2, (2, 3, 5)), (257, (40, 33, 101)), (4097, (1000, 2001, 3003))])
def test_each_fallback_of_the_head_is_the_last_to_fire(nt, classes):
    """grid_waves swept over the head's need of waves: exactly a quarter of the grid (fits), one wave short (the lightest
    class goes), short of the two heavy classes (the heaviest share waves), short of that too (no head)."""
    a, b, c3 = classes
    c = limits_population(nt, a, b, c3, 7)
    need = (a + (b + 1) // 2 + (c3 + 3) // 4, a + (b + 1) // 2, (a + b + 1) // 2)
    assert need[0] > need[1] > need[2] > 0
    for waves, fallbacks in ((4 * need[0] + 3, 0), (4 * need[0], 0), (4 * need[0] - 1, 1), (4 * need[1], 1), (4 * need[1] - 1, 2),
                             (4 * need[2], 2), (4 * need[2] - 1, 3), (0, 3)):
        _, hp = check(c, pixel_head=True, grid_waves=waves, head_pct=(80, 50, 25))
        assert hp["classes"] == classes and hp["fallbacks"] == fallbacks, (waves, hp["fallbacks"], fallbacks)


@pytest.mark.parametrize("classes, fallbacks", [((10, 100, T.HEAD_CAP - 110), 0), ((10, 100, T.HEAD_CAP - 109), 1),
                                                ((10, T.HEAD_CAP - 10, 0), 0), ((10, T.HEAD_CAP - 9, 0), 3)])
def test_the_head_list_holds_its_cap_and_not_one_more(classes, fallbacks):
    """Exactly kHeadCap entries fit; one more and the lightest class goes -- or, when the two heavy classes alone are one
    too many, the whole head (sharing waves does not shorten the list).  The grid is never the limit here."""
    c = limits_population(1025, *classes, 8)
    _, hp = check(c, pixel_head=True, grid_waves=1 << 24, head_pct=(80, 50, 25))
    assert hp["classes"] == classes and hp["fallbacks"] == fallbacks
    assert hp["ends"][2] == (T.HEAD_CAP if fallbacks == 0 else 110 if fallbacks == 1 else 0)


@pytest.mark.parametrize("pct", [(50, 50, 50), (100, 100, 100), (100, 50, 50), (60, 60, 1), (30, 0, 0)])
def test_equal_head_thresholds(pct):
    """Classes whose thresholds coincide are empty, before and after the fallbacks; 0 % lists every item, padding too."""
    for nt in (3, 257):
        c = skewed_counts(nt, 9, cmax=101)
        c[::17] = 0
        for waves in (1 << 20, 64, 8):
            _, hp = check(c, pixel_head=True, grid_waves=waves, head_pct=pct)
            assert hp["skewed"]


# ------------------------------------------------------------------ one real render each: run_plan's wiring
def plan_of_a_render(name, h, w, spp, depth, **opts):
    """Renders with a caller scratch; returns (renderer, mode, launch shape, the scratch's regions as arrays, raw bytes)."""
    import torch
    import common
    b = common.build_scene(rtmi.SceneBuilder(common.scene_seed(name)), name, w / h).commit()
    R = rtmi.Renderer(b, h, w, spp, depth, True).init_rng()
    scratch = R.new_scratch()
    o = rtmi.render_opts(scratch=scratch, **opts)
    mode, shape = R.mode(o), R.launch_shape(o)
    R.render(opts=o)
    R.check()
    torch.cuda.synchronize()
    reg = rtmi.scratch_regions(R.frame)
    assert reg["total"] == R.scratch_bytes()
    raw = scratch.cpu().numpy().view(np.uint8)
    got = T.plan_arrays(raw, reg, mode["tiles"])
    # the first pass's counts, as the scheduler marked them: a resumed frame keeps them where a probe's states would be
    at = reg["states"] if mode["first_pass_resumed"] else reg["rays"]
    got["marked"] = raw[at:at + 4 * R.items].view(np.uint32).copy()
    return R, mode, shape, got


def test_the_plan_a_list_render_leaves_is_the_restatement_of_its_first_pass():
    """Planned chains on the Cornell box: the chain plan, tile order and queue in the scratch equal the restatement of the
    first pass's counts with the grid's waves, SIMDs and rounds; afterwards every tile is claimed, by a wave of the grid."""
    R, mode, shape, got = plan_of_a_render("cornell_box", 512, 512, 64, 10, schedule=2, plan=2, wave_priority=16, lane_stride=1,
                                           blocks_per_cu=2, threads_per_block=256, sparse_stride=8, outlier_x10=20, head_pct=PCT)
    assert mode["scheduled"] == 1 and mode["planned_chains"] == 1 and mode["first_pass_resumed"] == 1 and mode["tiles"] == 4096
    waves = mode["waves"]
    assert waves == shape["blocks"] * (shape["threads"] // 64)
    assert waves < mode["tiles"], "two workgroups per compute unit: chains of more than one tile, so the deal's turns show"
    simds = min(4 * shape["compute_units"], waves)
    rounds = (waves + simds - 1) // simds
    counts = got["marked"]
    assert (counts < T.MARK).all() and (counts[R.ray_counts.cpu().numpy() > 0] > 0).all()
    T.check_plan(counts, None, got, pixel_head=False, sparse_cap=(shape["blocks"] * shape["threads"] // 8) // 64 * 64,
                 grid_waves=waves, outlier_x10=20, head_pct=PCT, simds=simds, rounds=rounds, spp=64,
                 probe_spp=mode["first_pass_samples"], claims_zero=False)
    claims = got["claims"].astype(np.int64)
    assert ((claims >= 1) & (claims <= waves)).all(), "every tile claimed once, by a wave index in 1 .. waves"


def test_the_plan_a_mesh_render_leaves_is_the_restatement_of_its_first_pass():
    """The bunny: the pixel head from the first pass's counts (marked in the copy the scheduler works on), the quarter
    tiles sorted by the probe's work counts and dealt as a snake."""
    R, mode, shape, got = plan_of_a_render("bunny", 96, 96, 64, 10, schedule=2, cost_probe=1, outlier_x10=20, head_pct=PCT)
    assert mode["scheduled"] == 1 and mode["planned_chains"] == 0 and mode["first_pass_resumed"] == 1 and mode["tiles"] == 144
    counts = got["marked"] & np.uint32(T.MARK - 1)
    final = R.ray_counts.cpu().numpy().view(np.uint32)
    assert (counts <= final).all() and counts.sum() > 0
    assert got["work"].max() > 0, "the first pass booked its searches' work"
    hp = T.check_plan(counts, got["work"], got, pixel_head=True, sparse_cap=0, grid_waves=mode["waves"], outlier_x10=20,
                      head_pct=PCT)
    assert hp["cmax"] >= 4
