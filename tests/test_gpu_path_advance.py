"""rtmi_path_advance on the device: one advance on synthetic inputs against the numpy restatement (tests/advancelib.py)
word for word, and Renderer.render_wavefront -- the loop bounce_list / path_advance / path_compact that refills ended paths
in place -- against rtmi_render_budget on a twin renderer with the same seed, bit for bit: sums, second moments, sample
and ray counts, final RNG states and the totals.  Frames are 20x28 (ragged on both edges) and 16x16."""
import ctypes as C
import functools
import math

import numpy as np
import pytest

import common
import rtmi
from advancelib import IN_FLIGHT, Wavefront, advance, camera_ray
from bouncelistlib import ptr
from parity import bits

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

F32 = np.float32
SENTINEL = 0x7FC00123  # what every array holds where nothing was put: a written word shows
WORLDS = ["cornell_box", "mixed", "spheres", "bunny", "sky_only"]  # (tests/test_gpu_bounce_list.py holds trace_steps on them)
SHARDS = [(0, 1), (2, 3)]


@functools.lru_cache(maxsize=None)
def scene(name):
    b = common.build_scene(rtmi.SceneBuilder(common.scene_seed(name)), name, 28 / 20)
    if name == "mixed":  # the defocus camera: four draws per camera ray
        b.camera_defocus([0.5, 1.5, 6], [0, 0.8, 0], [0, 1, 0], math.pi / 4, 1.25, 0.3, 5.5)
    return b.commit()


def renderer(b, h, w, spp, depth, rank=0, world=1):
    return rtmi.Renderer(b, h, w, spp, depth, post=False, rank=rank, world_size=world).init_rng()


def host_states(R):
    return np.ascontiguousarray(R.states.cpu().numpy().view(np.uint32).T)  # (items, 6)


def results(R):
    torch.cuda.synchronize()
    return {"sum": R.sum.cpu().numpy(), "sq": R.sq.cpu().numpy(), "samples": R.samples.cpu().numpy(),
            "budget_rays": R.budget_rays.cpu().numpy(), "states": host_states(R)}


def assert_same(a, b, what):
    for k in a:
        assert np.array_equal(bits(a[k]), bits(b[k])), "%s: %s differ at %s" % (what, k, np.argwhere(bits(a[k]) != bits(b[k]))[:4].tolist())


def dev_budget(R, budget):
    return None if budget is None else torch.from_numpy(np.asarray(budget).astype(np.int32)).to(R.device)


def random_budget(seed, n, hi):
    """0 .. hi, a fifth zeros (budgetlib.random_budget's kind)."""
    rng = np.random.default_rng(seed)
    b = rng.integers(1, hi + 1, n)
    b[rng.random(n) < 0.2] = 0
    return b


# ------------------------------------------------------------------ 1. one advance, word for word
def dev_f(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=F32)).cuda()


def dev_u(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.uint32).view(np.int32)).cuda()


def synthetic(R, depth, spp, budget, seed, full, listed):
    """A Wavefront over R's items with hand-made contents in every state the rule tells apart (the class of item q is
    q mod 12) for the items of the mask `listed`, sentinel words in every other item, and R's own RNG states."""
    pixel_of = rtmi.pixel_map(R.frame)
    n = len(pixel_of)
    rng = np.random.default_rng(seed)
    wf = Wavefront(pixel_of, spp, depth, host_states(R), budget, with_sq=full, with_rays=full, with_counts=full)
    nanf = np.array([SENTINEL], np.uint32).view(F32)[0]
    for a in (wf.origins, wf.dirs, wf.emitted, wf.attenuation, wf.e_stack, wf.a_stack):
        a[...] = nanf
    wf.steps[:] = SENTINEL
    wf.cursor[:] = SENTINEL & (IN_FLIGHT - 1)  # (a huge k with F clear: no samples left)
    wf.sum[:] = rng.uniform(0, 4, (n, 3)).astype(F32)
    if full:
        wf.sq[:] = rng.uniform(0, 9, (n, 3)).astype(F32)
        wf.ray_counts[:] = rng.integers(0, 1000, n)
        wf.counts[:] = (5, 6, 7)
    wf.samples[:] = rng.integers(0, 100, n)
    unit = rng.normal(size=(n, 3))
    unit = (unit / np.linalg.norm(unit, axis=1, keepdims=True)).astype(F32)
    for q in np.flatnonzero(listed):
        b = min(int(budget[q]) if budget is not None else spp, spp)
        kind = q % 12
        k = int(rng.integers(1, b + 1)) if b else 0
        wf.origins[q] = rng.uniform(-1, 1, 3).astype(F32)
        wf.emitted[q], wf.attenuation[q] = rng.uniform(0, 2, 3).astype(F32), rng.uniform(0, 1, 3).astype(F32)
        wf.e_stack[:, q], wf.a_stack[:, q] = rng.uniform(0, 2, (depth, 3)).astype(F32), rng.uniform(0, 1, (depth, 3)).astype(F32)
        P = int(rng.integers(0, depth))
        if kind == 0 or k == 0:       # fresh: nothing started
            wf.cursor[q], wf.steps[q], wf.dirs[q] = (0, 0), 0, 0.0
        elif kind == 1:               # just stepped, scattered: push and go on (or cut, where P + 1 == depth)
            wf.cursor[q], wf.steps[q], wf.dirs[q] = (IN_FLIGHT | k, P), P + 1, unit[q]
        elif kind == 2:               # just stepped, ended: push, fold from E[c-1], add, refill or stop
            wf.cursor[q], wf.steps[q], wf.dirs[q] = (IN_FLIGHT | k, P), P + 1, (0.0, -0.0, 0.0)
        elif kind == 3:               # cut at max_depth with a live ray
            wf.cursor[q], wf.steps[q], wf.dirs[q] = (IN_FLIGHT | k, depth - 1), depth, unit[q] * F32(3)
        elif kind == 4:               # in flight, not stepped by the last step: only the cursor is rewritten
            wf.cursor[q], wf.steps[q], wf.dirs[q] = (IN_FLIGHT | k, P), P, unit[q]
        elif kind == 5:               # a fresh path whose ray is bad (a NaN origin): radiance 0, no query
            wf.cursor[q], wf.steps[q], wf.dirs[q] = (IN_FLIGHT | k, 0), 0, unit[q]
            wf.origins[q, 1] = np.nan
        elif kind == 6:               # no path in flight and no samples left
            wf.cursor[q], wf.steps[q], wf.dirs[q] = (b, P), P, unit[q]
        elif kind == 7:               # the caller broke d_steps and P: nothing is addressed past the stacks
            wf.cursor[q], wf.steps[q], wf.dirs[q] = (IN_FLIGHT | k, depth + 3), depth + 4, unit[q]
        elif kind == 8:               # a bad scattered ray after two steps: an alive path of c steps
            wf.cursor[q], wf.steps[q], wf.dirs[q] = (IN_FLIGHT | k, 1), 2, (1e-30, 0.0, 0.0)
        elif kind == 9:               # a fresh in-flight zero ray (a fisheye's surround)
            wf.cursor[q], wf.steps[q], wf.dirs[q] = (IN_FLIGHT | k, 0), 0, 0.0
        elif kind == 10:              # ended long ago and not stepped since (P == steps): folds its layers
            wf.cursor[q], wf.steps[q], wf.dirs[q] = (IN_FLIGHT | k, P), P, 0.0
        else:                         # more samples started than the budget allows: the path in flight still finishes
            wf.cursor[q], wf.steps[q], wf.dirs[q] = (IN_FLIGHT | (b + 2), P), P + 1, 0.0
    return wf


def device_advance(R, wf, proj, lst, n_list, count):
    """One rtmi_path_advance through the C ABI on device copies of wf; returns a dict of everything read back."""
    t = {"origins": dev_f(wf.origins), "dirs": dev_f(wf.dirs), "steps": dev_u(wf.steps), "emitted": dev_f(wf.emitted),
         "attenuation": dev_f(wf.attenuation), "e_stack": dev_f(wf.e_stack), "a_stack": dev_f(wf.a_stack),
         "cursor": dev_u(wf.cursor), "sum": dev_f(wf.sum), "samples": dev_u(wf.samples),
         "states": dev_u(np.ascontiguousarray(wf.states.T))}
    t["sq"] = dev_f(wf.sq) if wf.sq is not None else None
    t["ray_counts"] = dev_u(wf.ray_counts) if wf.ray_counts is not None else None
    t["counts"] = torch.from_numpy(wf.counts.copy()).cuda() if wf.counts is not None else None
    d_budget = dev_u(wf.budget) if wf.budget is not None else None
    d_list = dev_u(lst) if lst is not None else None
    d_count = dev_u([count]) if count is not None else None
    a = rtmi.PathAdvanceArgs()
    a.size, a.reserved = C.sizeof(rtmi.PathAdvanceArgs), 0
    a.proj = C.pointer(proj) if proj is not None else None
    val = lambda x: None if x is None else x.data_ptr()
    a.d_budget, a.d_list, a.n_list, a.d_count = val(d_budget), val(d_list), n_list, val(d_count)
    a.d_origins, a.d_dirs, a.d_states, a.d_steps = val(t["origins"]), val(t["dirs"]), val(t["states"]), val(t["steps"])
    a.d_emitted, a.d_attenuation = val(t["emitted"]), val(t["attenuation"])
    a.d_emitted_stack, a.d_attenuation_stack, a.d_cursor = val(t["e_stack"]), val(t["a_stack"]), val(t["cursor"])
    a.d_sum, a.d_sq, a.d_samples, a.d_ray_counts = val(t["sum"]), val(t["sq"]), val(t["samples"]), val(t["ray_counts"])
    a.d_counts = val(t["counts"])
    rc = rtmi.lib().rtmi_path_advance(R.scene.h, C.byref(R.frame), C.byref(a), C.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert rc == 0, rtmi.lib().rtmi_last_error()
    torch.cuda.synchronize()
    out = {k: (v.cpu().numpy() if v is not None else None) for k, v in t.items()}
    out["states"] = np.ascontiguousarray(out["states"].T)
    return out


@pytest.mark.parametrize("case", ["listed_shard", "identity_orthographic"])
def test_one_advance_matches_the_restatement_word_for_word(case):
    b = scene("cornell_box")
    cam = b.camera_get()
    if case == "listed_shard":
        h, w, depth, spp, rank, world, kind, full = 20, 28, 3, 4, 1, 2, "camera", True
    else:
        h, w, depth, spp, rank, world, kind, full = 16, 16, 2, 3, 0, 1, "orthographic", False
    R = renderer(b, h, w, spp, depth, rank, world)
    n = R.items
    rng = np.random.default_rng(3)
    budget = rng.integers(0, spp + 3, n) if full else None
    lst, n_list, count, listed = None, n, None, np.ones(n, bool)
    if full:  # a shuffled list of distinct items with two entries that are no items in it, cut short by the count
        lst = rng.permutation(n)[:n - 40].astype(np.uint32)
        lst[5], lst[70] = n, 0xfffffff0
        n_list, count = len(lst), len(lst) - 9
        listed = np.zeros(n, bool)
        listed[lst[:count][lst[:count] < n]] = True
    wf = synthetic(R, depth, spp, budget, 17, full, listed)
    got = device_advance(R, wf, rtmi.projection(kind) if kind != "camera" else None, lst, n_list, count)
    advance(wf, lambda q, idx, st: camera_ray(cam, h, w, idx, st, kind), lst, n_list, count)
    want = {"origins": wf.origins, "dirs": wf.dirs, "steps": wf.steps, "emitted": wf.emitted, "attenuation": wf.attenuation,
            "e_stack": wf.e_stack, "a_stack": wf.a_stack, "cursor": wf.cursor, "sum": wf.sum, "samples": wf.samples,
            "states": wf.states, "sq": wf.sq, "ray_counts": wf.ray_counts, "counts": wf.counts}
    for k, v in want.items():
        if v is None:
            assert got[k] is None
            continue
        g = got[k].view(np.uint32) if got[k].dtype == np.int32 else got[k]
        diff = np.argwhere(bits(g) != bits(v)) if g.dtype == F32 else np.argwhere(g != v)
        assert len(diff) == 0, "%s differs at %s" % (k, diff[:6].tolist())
    pix = rtmi.pixel_map(R.frame) >= 0
    assert (~pix).any() == (case == "listed_shard"), "the ragged shard has padding items"
    if full:
        assert wf.counts[0] > 5 and wf.counts[2] > 7 and wf.counts[1] > 6
        assert (~listed).sum() >= 49
        for k in ("origins", "dirs", "emitted", "attenuation"):
            assert (bits(got[k][~listed]) == SENTINEL).all(), "an item that is not a candidate keeps every word"
        assert (got["cursor"][~listed] == SENTINEL).all() and (got["steps"][~listed] == SENTINEL).all()


# ------------------------------------------------------------------ 2. the loop against rtmi_render_budget
@pytest.mark.parametrize("depth", [0, 1, 2, 8])
@pytest.mark.parametrize("name", WORLDS)
def test_render_wavefront_equals_render_budget(name, depth):
    b = scene(name)
    spp = 3
    for rank, world in SHARDS:
        A, B = renderer(b, 20, 28, spp, depth, rank, world), renderer(b, 20, 28, spp, depth, rank, world)
        budget = random_budget(100 + rank, A.items, spp + 2)  # zeros, and entries above spp
        pix = rtmi.pixel_map(A.frame) >= 0
        assert (budget[pix] == 0).any() and (budget[pix] > spp).any()
        d_budget = dev_budget(A, budget)
        A.render_budget(d_budget)
        B.render_wavefront(d_budget)
        A.check(), B.check()
        what = "%s depth %d shard %d/%d" % (name, depth, rank, world)
        assert_same(results(A), results(B), what)
        total = int(A.d_work[1].item())  # the closest-hit queries of the budget call
        assert int(B.rays_total.item()) == total == int(A.budget_rays.cpu().numpy().astype(np.int64).sum()), what
        n_samples = int(np.minimum(budget, spp)[pix].sum())
        assert B.wavefront_counts.cpu().numpy().tolist() == [n_samples, total, n_samples], what
        assert B.wavefront_iterations <= spp * max(depth, 1) + 8, what
    # a uniform render from zeroed accumulators is rtmi_render with post_process = 0
    A, B = renderer(b, 16, 16, spp, depth), renderer(b, 16, 16, spp, depth)
    A.render()
    B.render_wavefront()
    A.check(), B.check()
    torch.cuda.synchronize()
    assert np.array_equal(bits(B.sum.cpu().numpy()), bits(A.tiles.cpu().numpy())), name
    assert np.array_equal(B.budget_rays.cpu().numpy(), A.ray_counts.cpu().numpy()) and np.array_equal(host_states(A), host_states(B))


# ------------------------------------------------------------------ 3. two calls: accumulation and carried state
def test_two_wavefront_renders_accumulate_like_two_budget_renders():
    b = scene("mixed")
    A, B = renderer(b, 20, 28, 3, 8), renderer(b, 20, 28, 3, 8)
    for n_pass in range(2):
        d_budget = dev_budget(A, random_budget(40 + n_pass, A.items, 5))
        A.render_budget(d_budget)
        B.render_wavefront(d_budget)
        A.check(), B.check()
        assert_same(results(A), results(B), "pass %d" % n_pass)
    assert int(B.rays_total.item()) == int(A.budget_rays.cpu().numpy().astype(np.int64).sum())
    assert int(A.samples.sum().item()) > 0 and float(A.sq.sum().item()) > 0


# ------------------------------------------------------------------ 4. the fisheye's surround
def test_fisheye_surround_runs_through_its_samples_in_one_call():
    b = scene("cornell_box")
    proj = rtmi.projection("fisheye", math.pi)
    A, B = renderer(b, 16, 16, 3, 8), renderer(b, 16, 16, 3, 8)
    kept = {}
    A.render_rays(projection=proj, each=lambda s, o, d: kept.setdefault(s, d.clone()))
    seen = []
    B.render_wavefront(projection=proj, each=lambda it, r: seen.append(int(r.paths.n())), poll=1)
    A.check(), B.check()
    assert_same(results(A), results(B), "fisheye")
    assert int(A.rays_total.item()) == int(B.rays_total.item())
    outside = ~bits(kept[0].cpu().numpy()).any(axis=1) & ~bits(kept[1].cpu().numpy()).any(axis=1) & ~bits(kept[2].cpu().numpy()).any(axis=1)
    assert outside.any() and not outside.all()
    got = results(B)
    assert (got["samples"][outside] == 3).all() and not bits(got["sum"][outside]).any() and not got["budget_rays"][outside].any()
    # such a pixel made its six draws in the call that started the render and was never in a list
    assert max(seen) <= int((~outside).sum())


# ------------------------------------------------------------------ 5. polling changes nothing
def test_poll_1_and_64_give_identical_buffers():
    b = scene("spheres")
    budget = random_budget(9, rtmi.work_items(rtmi.make_frame(20, 28, 4, 8, False)), 6)
    runs = []
    for poll in (1, 64):
        R = renderer(b, 20, 28, 4, 8)
        R.render_wavefront(dev_budget(R, budget), poll=poll).check()
        runs.append((results(R), R))
    assert_same(runs[0][0], runs[1][0], "poll 1 against 64")
    assert runs[0][1].wavefront_iterations <= runs[1][1].wavefront_iterations
    pix = rtmi.pixel_map(runs[0][1].frame) >= 0
    for _, R in runs:
        assert R.wavefront_paths.n() == 0, "after completion the compaction count is 0"
        cur = R.wavefront_cursor.cpu().numpy().view(np.uint32)
        assert np.array_equal(cur[pix, 0], np.minimum(budget, 4)[pix].astype(np.uint32)), "every k == b, every F clear"
        assert not cur[~pix].any()


def test_the_bound_raises_instead_of_looping_on():
    b = scene("cornell_box")
    R = renderer(b, 16, 16, 2, 8)
    with pytest.raises(rtmi.RtmiError, match="poll"):
        R.render_wavefront(poll=0)
    with pytest.raises(rtmi.RtmiError, match="post=False"):
        rtmi.Renderer(b, 16, 16, 2, 8, post=True).init_rng().render_wavefront()
    # a hook that revives every path keeps the list full: the loop stops at its bound
    def revive(it, r):
        r.directions[:] = torch.tensor([0.0, 0.0, -1.0], device=r.directions.device)
        r.steps.zero_()

    with pytest.raises(rtmi.RtmiError, match="still live"):
        R.render_wavefront(each=revive, poll=4)


# ------------------------------------------------------------------ 6. the hook holds every path's vertex
def test_the_hook_sees_the_hits_of_the_rays_that_went_in():
    b = scene("cornell_box")
    R = renderer(b, 16, 16, 2, 4)
    rays, checked = {}, []

    def each(it, r):
        if it - 1 in rays:  # the rays the last iteration left are the ones this step stepped
            o, d = rays.pop(it - 1)
            idx = r.paths.index[:r.paths.n()].long()
            want = b.intersect(o[idx], d[idx]).check().raw
            assert torch.equal(r.hits.raw[idx][:, :10], want[:, :10]), it
            checked.append(int(idx.numel()))
        rays[it] = (r.origins.clone(), r.directions.clone())

    R.render_wavefront(each=each, poll=1).check()
    assert len(checked) >= 3 and min(checked) > 0
