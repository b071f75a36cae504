"""rtmi_render_budget / rtmi_budget_plan / rtmi_resolve / Renderer.render_adaptive on the GPU, bit for bit: against
rtmi_render (a uniform budget IS a render), against itself (two calls = one call), and against the oracle, which renders
one more sample of chosen pixels per call (``OracleBuilder.render(.., 1, .., pixel_ids=, states=)``) so that any budget
map is replayed a sample at a time with the sums and squares accumulated in numpy binary32.

Everything is compared in row-major pixel space (``Shards.gather``); what the kernels must leave ALONE -- padding items
of ragged tiles, items with budget 0 -- is compared in the tile-major buffers themselves."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import oraclelib
import rtmi
from abi_host import CHECK_LIB, ERR_DEPTH, ERR_INVALID, OK, ROOT
from budgetlib import ADAPTIVE, H, W, OracleReplay, Shards, assert_same_results, plan_rule, random_budget
from parity import same

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

F32 = np.float32
# scene, depth (the issue's: cornell at depth 50, spheres has the defocus camera, bunny with the small mesh)
SCENES = [("cornell_box", 50), ("spheres", 10), ("bunny", 10), ("birthday", 10), ("mixed", 10)]


# ------------------------------------------------------------------ 5. a uniform budget is a render
def check_uniform_budget_is_a_render(name, depth, world, b=5, oracle=True):
    budgeted = Shards(name, depth, b, world).render_budget(np.full(H * W, b))
    rendered = Shards(name, depth, b, world).render()
    got = budgeted.results()
    assert same(got["sum"], rendered.gather("tiles")), "sums against rtmi_render's raw tiles"
    assert same(got["budget_rays"], rendered.gather("ray_counts")), "ray counts against rtmi_render's"
    assert same(got["states"], rendered.gather("states")), "final states against rtmi_render's"
    assert np.array_equal(got["samples"], np.full(H * W, b))
    for r in range(world):  # the tile-major buffers whole, padding included (rtmi_render writes it black)
        assert same(budgeted.raw("sum")[r], rendered.raw("tiles")[r])
        assert same(budgeted.raw("budget_rays")[r], rendered.raw("ray_counts")[r])
        assert same(budgeted.raw("states")[r], rendered.raw("states")[r])
        assert int(budgeted.R[r].d_work[1].item()) == int(budgeted.raw("budget_rays")[r].view(np.uint32).sum())
    if oracle:
        OracleReplay(name, depth).add(np.full(H * W, b)).assert_equal(got, name)


@pytest.mark.parametrize("world", [1, 3])
@pytest.mark.parametrize("name,depth", SCENES)
def test_uniform_budget_is_a_render(name, depth, world):
    """Budget b everywhere on zeroed buffers = rtmi_render(spp = b, post_process = 0): tiles, ray counts, states; and
    the oracle's sums, squares and states (birthday against rtmi_render only: its image-textured sphere goes through
    two libms)."""
    check_uniform_budget_is_a_render(name, depth, world, oracle=name != "birthday")


# ------------------------------------------------------------------ 6. passes add up
@pytest.mark.parametrize("name,depth", [("cornell_box", 50), ("bunny", 10), ("spheres", 10)])
def test_two_calls_equal_one(name, depth):
    b1, b2 = random_budget(11, hi=6), random_budget(12, hi=6)
    two = Shards(name, depth, 12).render_budget(b1).render_budget(b2).results()
    one = Shards(name, depth, 12).render_budget(b1 + b2).results()
    assert_same_results(two, one, name)
    assert np.array_equal(one["samples"], b1 + b2)


# ------------------------------------------------------------------ 7. a budget map against the oracle; what is left alone
@pytest.mark.parametrize("name,depth", [("cornell_box", 50), ("spheres", 10), ("bunny", 10), ("mixed", 10)])
def test_budget_map_matches_the_oracle_replay(name, depth):
    budget = random_budget(7 + len(name))
    assert (budget == 0).sum() > H * W // 10 and budget.max() == 9
    got = Shards(name, depth, 9).render_budget(budget).results()
    OracleReplay(name, depth).add(budget).assert_equal(got, name)


@pytest.mark.parametrize("world", [1, 3])
def test_zero_budget_and_padding_items_are_untouched(world):
    """Every buffer holds a sentinel before the call: items with budget 0 and padding items keep it in all five buffers
    (padding even where its budget word is not 0), and the rendered pixels carry on FROM the sentinel."""
    name, depth = "cornell_box", 10
    budget = random_budget(3)
    s = Shards(name, depth, 9, world)
    for R in s.R:
        R.sum.fill_(0.25), R.sq.fill_(0.5), R.samples.fill_(7), R.budget_rays.fill_(1000)
    before = s.raw("states")
    for R, bt in zip(s.R, s.scatter(budget, pad=5)):
        R.render_budget(bt).check()
    for r, pm in enumerate(s.pm):
        b_item = np.zeros(pm.shape, np.int64)
        b_item[pm >= 0] = budget[pm[pm >= 0]]
        idle = (pm < 0) | (b_item == 0)
        assert (pm < 0).any() and ((pm >= 0) & (b_item == 0)).any()
        assert (s.raw("sum")[r][idle] == F32(0.25)).all() and (s.raw("sq")[r][idle] == F32(0.5)).all()
        assert (s.raw("samples")[r][idle] == 7).all() and (s.raw("budget_rays")[r][idle] == 1000).all()
        assert np.array_equal(s.raw("states")[r][idle], before[r][idle])
        assert not np.array_equal(s.raw("states")[r][~idle], before[r][~idle])
    o = OracleReplay(name, depth)
    o.sum[:], o.sq[:], o.samples[:], o.rays[:] = 0.25, 0.5, 7, 1000
    o.add(budget).assert_equal(s.results(), "from the sentinel")


# ------------------------------------------------------------------ 8. the frame's spp caps one call
def test_frame_spp_caps_the_budget():
    capped = Shards("cornell_box", 10, 4).render_budget(np.full(H * W, 9)).results()
    four = Shards("cornell_box", 10, 4).render_budget(np.full(H * W, 4)).results()
    assert (capped["samples"] == 4).all()
    assert_same_results(capped, four)


# ------------------------------------------------------------------ 9. plan and resolve
def test_budget_plan_matches_the_numpy_rule():
    s = Shards("cornell_box", 10, 9, world=3).render_budget(random_budget(21))
    for opts in (dict(min_spp=4, max_spp=8, step=3, tolerance=0.25, floor=0.01),
                 dict(min_spp=2, max_spp=64, step=4, tolerance=0.5, floor=0.0),
                 dict(min_spp=2, max_spp=6, step=16, tolerance=0.05, floor=0.1)):
        seen = set()
        for R, pm in zip(s.R, s.pm):
            budget, active, total = R.plan(**opts)
            got = budget.cpu().numpy().view(np.uint32)
            want = plan_rule(R.samples.cpu().numpy().view(np.uint32), R.sum.cpu().numpy(), R.sq.cpu().numpy(),
                             opts["min_spp"], opts["max_spp"], opts["step"], opts["tolerance"], opts["floor"], pixel=pm >= 0)
            assert np.array_equal(got, want), opts
            assert (active, total) == (int((want > 0).sum()), int(want.sum())), opts
            seen |= set(want.tolist())
            # totals are overwritten, not accumulated
            assert R.plan(**opts)[1:] == (active, total)
        assert len(seen) >= 3, "the case tells nothing apart: %s" % sorted(seen)


def oracle_post(sum_, n):
    """sum / n, then orc_post_process's own code, pixel by pixel (0 where n == 0)."""
    out = np.zeros_like(sum_)
    L = oraclelib.lib()
    for count in np.unique(n):
        if count == 0:
            continue
        sel = np.ascontiguousarray(sum_[n == count])
        L.orc_post_process(sel.ctypes.data_as(C.POINTER(C.c_float)), sel.shape[0], int(count))
        out[n == count] = sel
    return out


def test_resolve_matches_render_and_numpy():
    # a uniform count: rtmi_render's post-processed tile buffer, bit for bit, padding included
    s = Shards("cornell_box", 10, 6).render_budget(np.full(H * W, 6))
    R = rtmi.Renderer(s.b, H, W, 6, 10, post=True).init_rng()
    R.render().check()
    assert same(s.R[0].resolve(post=True).cpu().numpy(), R.tiles.cpu().numpy())
    # a map with zeros: sum / n in binary32, then the oracle's post-processing; 0 where nothing was sampled
    m = Shards("cornell_box", 10, 9).render_budget(random_budget(5))
    sum_, n = m.R[0].sum.cpu().numpy(), m.R[0].samples.cpu().numpy().view(np.uint32)
    assert (n == 0).any() and len(np.unique(n)) >= 5
    assert same(m.R[0].resolve(post=True).cpu().numpy(), oracle_post(sum_, n))
    with np.errstate(all="ignore"):
        raw = np.where(n[:, None] > 0, sum_ / n.astype(F32)[:, None], F32(0)).astype(F32)
    assert same(m.R[0].resolve(post=False).cpu().numpy(), raw)


@pytest.mark.parametrize("name", ["cornell_box", "bunny"])
def test_render_adaptive_matches_the_oracle_loop(name):
    depth = 10
    o = OracleReplay(name, depth)
    passes = 0
    while True:
        budget = plan_rule(o.samples, o.sum, o.sq, ADAPTIVE["min_spp"], ADAPTIVE["max_spp"], ADAPTIVE["step"],
                           ADAPTIVE["tolerance"], ADAPTIVE["floor"])
        if not budget.any():
            break
        o.add(budget)
        passes += 1
    total, n = int(o.samples.sum()), H * W
    print("%s: %d passes, %d of %d samples (%.2f), %.1f %% at max, %.1f %% at min, %d distinct counts" % (
        name, passes, total, n * 64, total / (n * 64), 100 * (o.samples == 64).mean(), 100 * (o.samples == 4).mean(),
        len(np.unique(o.samples))))
    # the oracle's own figures: the loop is not vacuous
    assert total < n * 64 // 2
    if name == "cornell_box":
        assert (o.samples == 64).any()
    assert (o.samples == 4).sum() >= n // 4
    assert len(np.unique(o.samples)) >= 3

    s = Shards(name, depth, 64)
    res = s.R[0].render_adaptive(**ADAPTIVE)
    assert (res.passes, res.total_samples) == (passes, total)
    o.assert_equal(s.results(), name)
    pm = s.pm[0]
    resolved = np.zeros((n, 3), F32)
    resolved[pm[pm >= 0]] = res.tiles.cpu().numpy()[pm >= 0]
    assert same(resolved, oracle_post(o.sum, o.samples))
    # the sample map and the image through the existing untile entries
    img, cnt = s.R[0].untile(res.tiles, res.samples)
    assert same(img.cpu().numpy().reshape(n, 3), resolved)
    assert np.array_equal(cnt.cpu().numpy().reshape(n).view(np.uint32), o.samples)


# ------------------------------------------------------------------ 11. shares no device state
def test_budget_call_runs_beside_a_render_on_the_same_scene():
    name, depth, spp = "bunny", 10, 16
    budget = random_budget(9, hi=16)
    alone = Shards(name, depth, spp).render_budget(budget)
    want_budget = alone.results()
    R0 = rtmi.Renderer(alone.b, 64, 64, spp, depth, post=False).init_rng()
    R0.render().check()
    want_tiles, want_rays = R0.tiles.cpu().numpy(), R0.ray_counts.cpu().numpy()

    Rb = rtmi.Renderer(alone.b, H, W, spp, depth, post=False).init_rng()
    Rb._budget_buffers()
    R1 = rtmi.Renderer(alone.b, 64, 64, spp, depth, post=False).init_rng()
    bt = alone.scatter(budget)[0]
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    for _ in range(3):  # (three rounds on fresh buffers: the two calls overlap in at least some)
        Rb.init_rng(), R1.init_rng()
        for t in (Rb.sum, Rb.sq, Rb.samples, Rb.budget_rays):
            t.zero_()
        torch.cuda.synchronize()
        R1.render()
        with torch.cuda.stream(side):
            Rb.render_budget(bt)
        torch.cuda.synchronize()
        R1.check(), Rb.check()
        assert int(Rb.d_work[0].item()) == 0
        assert same(R1.tiles.cpu().numpy(), want_tiles) and same(R1.ray_counts.cpu().numpy(), want_rays)
        alone.R = [Rb]
        assert_same_results(alone.results(), want_budget, "beside a render")


# ------------------------------------------------------------------ argument checks that need a committed scene
def test_budget_argument_checks_on_a_committed_scene():
    s = Shards("cornell_box", 10, 4)
    R, L = s.R[0], rtmi.lib()
    bt = s.scatter(np.full(H * W, 2))[0]

    def call(frame):
        return L.rtmi_render_budget(s.b.h, C.byref(frame), C.c_void_p(bt.data_ptr()), C.c_void_p(R.states.data_ptr()),
                                    C.c_void_p(R.sum.data_ptr()), None, C.c_void_p(R.samples.data_ptr()), None,
                                    C.c_void_p(R.d_work.data_ptr()), None)

    before = s.raw("states")[0]
    assert call(rtmi.make_frame(H, W, 4, 65, post=False)) == ERR_DEPTH and b"depth" in L.rtmi_last_error()
    assert call(rtmi.make_frame(H, W, 4, -1, post=False)) == ERR_DEPTH
    assert call(rtmi.make_frame(H, W, 4, 10, post=True)) == ERR_INVALID and b"post_process" in L.rtmi_last_error()
    assert call(rtmi.make_frame(H, W, 1 << 30, 10, post=False)) == ERR_INVALID and b"2^31" in L.rtmi_last_error()
    assert np.array_equal(s.raw("states")[0], before) and int(R.samples.sum().item()) == 0
    # the two nullable arrays left out: the sums are the same
    assert call(rtmi.make_frame(H, W, 4, 10, post=False)) == OK
    torch.cuda.synchronize()
    full = Shards("cornell_box", 10, 4).render_budget(np.full(H * W, 2))
    assert same(R.sum.cpu().numpy(), full.R[0].sum.cpu().numpy())
    assert same(s.raw("states")[0], full.raw("states")[0])
    assert int(R.sq.abs().sum().item()) == 0 and int(R.budget_rays.sum().item()) == 0
    assert int(R.d_work[1].item()) == int(full.R[0].budget_rays.sum().item())


# ------------------------------------------------------------------ 12. the check build
def test_check_build_renders_a_uniform_budget():
    """librtmi_check1.so compiles the budget kernels too (its margin re-query stays render-only): loaded in a process of
    its own, it passes the uniform-budget comparison on the Cornell box."""
    assert os.path.exists(CHECK_LIB), "librtmi_check1.so missing: __graft_entry__.build() builds it"
    env = dict(os.environ, RTMI_LIB_PATH=CHECK_LIB)
    env["PYTHONPATH"] = os.pathsep.join([os.path.join(ROOT, "ray-tracing-cuda_amd"), os.path.join(ROOT, "tests")])
    r = subprocess.run([sys.executable, os.path.abspath(__file__)], env=env, cwd=ROOT, stdout=subprocess.PIPE,
                       stderr=subprocess.PIPE, text=True, timeout=600)
    assert r.returncode == 0 and "check build ok" in r.stdout, (r.stdout[-2000:], r.stderr[-4000:])


if __name__ == "__main__":
    assert rtmi.LIB_PATH == CHECK_LIB or "check1" in rtmi.LIB_PATH, rtmi.LIB_PATH
    check_uniform_budget_is_a_render("cornell_box", 50, 1)
    check_uniform_budget_is_a_render("bunny", 10, 1)
    print("check build ok")
