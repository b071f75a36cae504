"""rtmi_render_direct on the GPU: the budget render with next-event estimation inside, held bit for bit to the composition
the parent already holds to the loop and the oracle -- Renderer.render_rays(budget, direct="fused") on a twin renderer with
the same seed: sums, second moments, sample and ray counts, both RNG states, the three counters and the work words; on every
kind of scene rtmi_trace_direct's tests use, at several depths, frame shapes and budgets, over calls in a row and calls
interleaved with the loop, with features, through render_adaptive_direct, with canaries around every output written through the
raw C ABI; and the refusals that need a committed scene.

No statistical test: bit equality with render_rays(direct="fused") carries the expectation and variance results of
tests/test_gpu_direct_mis.py and tests/test_gpu_sphere_lights.py over to this entry, as for rtmi_trace_direct."""
import ctypes as C

import numpy as np
import pytest

import renderdirectlib as rdl
import rtmi
from abi_host import ERR_DEPTH, _refused
from rtmi import _abi

pytestmark = pytest.mark.gpu


def check_against_the_loop(name, h, w, spp, depth, budget=None, rank=0, world=1):
    """One call on renderer A against the loop on its twin B; `budget`: None (spp everywhere), a number, or a function of
    the renderer that gives a per-item array.  Returns (A, B, what the call said, the loop)."""
    A, B = (rdl.renderer(name, h, w, spp, depth, rank, world) for _ in range(2))
    values = spp if budget is None else budget(A) if callable(budget) else budget
    bt = rdl.budget_tensor(A, values)
    loop = rdl.Loop().render(B, bt)
    got = rdl.raw_direct(A, bt)
    assert got["intact"], "a canary around an output was overwritten"
    what = "%s %dx%d spp %d depth %d rank %d/%d" % (name, h, w, spp, depth, rank, world)
    rdl.assert_same_buffers(rdl.buffers(A), rdl.buffers(B), what)
    assert got["counts"].tolist() == loop.counts.tolist(), (what, got["counts"], loop.counts)
    assert got["work"][0] == 0 and got["work"][1] == loop.queries == int(B.rays_total.item()), what
    return A, B, got, loop


# ------------------------------------------------------------------ 1. the loop, bit for bit, on every kind of scene
@pytest.mark.parametrize("name", rdl.SCENES)
def test_scene_is_the_loop_bit_for_bit(name):
    A, B, got, _ = check_against_the_loop(name, 16, 16, 3, 6)
    assert (A.samples.cpu().numpy() == 3).all()
    counts = got["counts"].tolist()
    if name in rdl.EMPTY_TABLE:
        assert counts == [0, 0, 0]
        fresh = rtmi.rng_states(A.scene.seed, A.items, first=A.items, device=A.device)
        assert np.array_equal(A.light_states.cpu().numpy(), fresh.cpu().numpy()), "a light state moved"
    elif name == "enclosing":
        assert counts == [counts[0], 0, 0] and counts[0] > 0  # sampled, never valid, never weighed
    else:
        assert counts[0] > 100 and counts[1] > 0, "the case samples or weighs nothing"
    if name in rdl.OCCLUDES:
        assert counts[2] > 0, "no shadow ray of the case is occluded"
    if name == "sky_only":  # an empty table: rtmi_render_budget's sums (the buffers hold no -0.0f)
        P = rdl.renderer(name, 16, 16, 3, 6)
        P.render_budget(rdl.budget_tensor(P, 3)).check()
        want = dict(rdl.buffers(P), light_states=rdl.buffers(A)["light_states"])
        rdl.assert_same_buffers(rdl.buffers(A), want, "sky_only against render_budget")


def test_direct_light_changes_the_sums_where_a_table_light_shines():
    """The comparison above is not one of two plain renders: on lamp_room the direct sums are not render_budget's."""
    A, P = (rdl.renderer("lamp_room", 16, 16, 3, 6) for _ in range(2))
    bt = rdl.budget_tensor(A, 3)
    A.render_direct(bt).check()
    P.render_budget(bt).check()
    assert not np.array_equal(A.sum.cpu().numpy(), P.sum.cpu().numpy())
    assert np.array_equal(A.samples.cpu().numpy(), P.samples.cpu().numpy())


# ------------------------------------------------------------------ 2. depths
@pytest.mark.parametrize("depth", [0, 1, 2, 50])
@pytest.mark.parametrize("name", ["lamp_room", "bulb_room"])
def test_depths(name, depth):
    A, _, got, _ = check_against_the_loop(name, 8, 8, 3, depth)
    if depth == 0:
        assert not A.sum.cpu().numpy().any() and got["counts"].tolist() == [0, 0, 0]
    if depth == 1:
        assert got["counts"][0] == 0  # the only vertex does not sample
    if depth >= 2:
        assert got["counts"][0] > 0


# ------------------------------------------------------------------ 3. frame shapes
@pytest.mark.parametrize("h,w", [(20, 28), (1, 1), (8, 9)])
def test_frame_shapes(h, w):
    A, _, _, _ = check_against_the_loop("lamp_room", h, w, 3, 6)
    pm = rtmi.pixel_map(A.frame)
    assert (A.samples.cpu().numpy()[pm < 0] == 0).all() and (A.samples.cpu().numpy()[pm >= 0] == 3).all()


@pytest.mark.parametrize("rank", [0, 1])
def test_shards(rank):
    check_against_the_loop("lamp_room", 16, 16, 3, 6, rank=rank, world=2)


def test_defocus_camera_draws_four_times_per_sample():
    A, _, got, _ = check_against_the_loop("defocus_lamp_room", 16, 16, 3, 6)
    assert got["counts"][0] > 100
    P = rdl.renderer("lamp_room", 16, 16, 3, 6)
    rdl.raw_direct(P, rdl.budget_tensor(P, 3))
    assert not np.array_equal(A.states.cpu().numpy(), P.states.cpu().numpy())  # (the lens draws moved the path states)


# ------------------------------------------------------------------ 4. budgets
def test_ragged_budget_and_zero_budget_items_keep_every_word():
    import torch
    name, h, w, spp, depth = "lamp_room", 20, 28, 5, 6
    A, B = (rdl.renderer(name, h, w, spp, depth) for _ in range(2))
    values = rdl.ragged_budget(A)
    assert (values == 0).any() and values.max() == 5
    bt = rdl.budget_tensor(A, values)
    # what a zero-budget item and padding must keep: recognisable words in every buffer, the light states included
    for R in (A, B):
        R._light_states()
        R.sum.fill_(1.5), R.sq.fill_(2.5), R.samples.fill_(7), R.budget_rays.fill_(9)
    before = rdl.buffers(A)
    loop = rdl.Loop().render(B, bt)
    got = rdl.raw_direct(A, bt)
    assert got["intact"]
    rdl.assert_same_buffers(rdl.buffers(A), rdl.buffers(B), "ragged budget")
    assert got["counts"].tolist() == loop.counts.tolist() and got["work"][1] == loop.queries
    idle = (values == 0) | (rtmi.pixel_map(A.frame) < 0)
    after = rdl.buffers(A)
    for k in ("sum", "sq", "samples", "budget_rays"):
        assert np.array_equal(after[k][idle].view(np.uint32), before[k][idle].view(np.uint32)), k
    for k in ("states", "light_states"):
        assert np.array_equal(after[k][:, idle], before[k][:, idle]), k
    busy = ~idle
    assert np.array_equal(after["samples"][busy], 7 + values[busy]) and (after["states"][:, busy] != before["states"][:, busy]).any()
    assert torch.isfinite(A.sum).all()


def test_budget_above_spp_is_capped():
    A, _, _, _ = check_against_the_loop("bulb_room", 8, 9, 2, 6, budget=lambda R: np.where(np.arange(R.items) % 3 == 0, 1, 1000))
    live = rtmi.pixel_map(A.frame) >= 0
    assert set(A.samples.cpu().numpy()[live].tolist()) == {1, 2}


# ------------------------------------------------------------------ 5. calls in a row, and interleaved with the loop
def test_two_calls_are_one_loop_of_the_summed_budget():
    name, h, w, spp, depth = "lamp_room", 16, 16, 6, 6
    A, B = (rdl.renderer(name, h, w, spp, depth) for _ in range(2))
    b1 = rdl.ragged_budget(A, seed=11, hi=3)
    b2 = rdl.ragged_budget(A, seed=12, hi=3)
    c1 = rdl.raw_direct(A, rdl.budget_tensor(A, b1))
    A.render_direct(rdl.budget_tensor(A, b2)).check()  # (the second through the binding: its counters add up)
    loop = rdl.Loop().render(B, rdl.budget_tensor(B, b1 + b2))
    rdl.assert_same_buffers(rdl.buffers(A), rdl.buffers(B), "two calls")
    assert (c1["counts"] + A.direct_counts.cpu().numpy()).tolist() == loop.counts.tolist()
    assert c1["work"][1] + int(A.d_work[1].item()) == loop.queries


def test_calls_interleave_with_render_rays_fused():
    name, h, w, spp, depth = "bulb_room", 16, 16, 3, 6
    A, B = (rdl.renderer(name, h, w, spp, depth) for _ in range(2))
    bt = [rdl.budget_tensor(A, rdl.ragged_budget(A, seed=s, hi=3)) for s in (21, 22, 23)]
    A.render_direct(bt[0])
    A.render_rays(bt[1], direct="fused")
    A.render_direct(bt[2]).check()
    for t in bt:
        B.render_rays(t, direct="fused")
    rdl.assert_same_buffers(rdl.buffers(A), rdl.buffers(B), "interleaved")


# ------------------------------------------------------------------ 6. features
@pytest.mark.parametrize("name", ["lamp_room", "textured_room"])
def test_features_are_render_features_and_colours_are_the_direct_render(name):
    h, w, spp, depth = 16, 16, 3, 6
    F, D, P = (rdl.renderer(name, h, w, spp, depth) for _ in range(3))
    values = rdl.ragged_budget(F, seed=5, hi=3)
    bt = rdl.budget_tensor(F, values)
    got = rdl.raw_direct(F, bt, features=True)
    assert got["intact"]
    D.render_direct(bt).check()
    P.render_budget(bt, features=True).check()
    rdl.assert_same_buffers(rdl.buffers(F), rdl.buffers(D), "features on and off")
    assert got["counts"].tolist() == D.direct_counts.tolist() and got["work"][1] == int(D.d_work[1].item())
    for k in ("albedo", "normal", "depth", "coverage"):  # the primary hits do not depend on direct light
        a, b = getattr(F, k).cpu().numpy(), getattr(P, k).cpu().numpy()
        assert np.array_equal(a.view(np.uint32), b.view(np.uint32)), k
    assert F.coverage.cpu().numpy().sum() > 0 and (F.coverage.cpu().numpy() <= values).all()
    # the binding's own way to the same call
    G = rdl.renderer(name, h, w, spp, depth)
    G.render_direct(bt, features=True).check()
    rdl.assert_same_buffers(rdl.buffers(G), rdl.buffers(F), "binding")
    assert np.array_equal(G.albedo.cpu().numpy().view(np.uint32), F.albedo.cpu().numpy().view(np.uint32))


# ------------------------------------------------------------------ 7. the adaptive loop
def test_render_adaptive_direct_is_its_passes_replayed_with_the_loop():
    name, h, w, depth = "lamp_room", 16, 16, 6
    opts = dict(min_spp=4, max_spp=16, step=4, tolerance=0.25, floor=0.01)
    A, B = (rdl.renderer(name, h, w, 4, depth) for _ in range(2))
    recorded = []
    inner = A.render_direct

    def record(budget, **kw):
        assert kw == {"features": False}
        recorded.append(budget.clone())
        return inner(budget, **kw)
    A.render_direct = record
    try:
        out = A.render_adaptive_direct(post=False, **opts)
    finally:
        del A.render_direct
    assert 1 <= out.passes == len(recorded) <= 4  # it terminates: at most (max_spp - min_spp) / step passes after the first
    n = out.samples.cpu().numpy()
    live = rtmi.pixel_map(A.frame) >= 0
    assert (n[live] >= opts["min_spp"]).all() and (n[live] <= opts["max_spp"]).all() and out.total_samples == n.sum()
    for bt in recorded:
        B.render_rays(bt, direct="fused")
    rdl.assert_same_buffers(rdl.buffers(A), rdl.buffers(B), "adaptive")
    assert np.array_equal(out.tiles.cpu().numpy().view(np.uint32), B.resolve(post=False).cpu().numpy().view(np.uint32))
    assert int(A.direct_counts[0].item()) > 0


# ------------------------------------------------------------------ 8. refusals that need a committed scene
def test_refusals_through_the_c_abi():
    import torch
    R = rdl.renderer("lamp_room", 8, 8, 2, 6)
    R._light_states()
    bt = rdl.budget_tensor(R, 2)
    bodies = {k: getattr(R, k) for k in ("states", "light_states", "sum", "sq", "samples", "budget_rays")}
    bodies["counts"] = torch.zeros(3, dtype=torch.int64, device=R.device)
    bodies["work"] = torch.zeros(rtmi.BUDGET_WORK_WORDS, dtype=torch.int64, device=R.device)
    before = rdl.buffers(R)

    def call(frame=None, **kw):
        a = rdl.direct_args(R, bt, bodies)
        for k, v in kw.items():
            setattr(a, k, v)
        return rtmi.lib().rtmi_render_direct(R.scene.h, C.byref(frame if frame is not None else R.frame), C.byref(a), None)

    for size in (0, 8, 80, 96):
        assert _refused(call(size=size), b"size")
    assert _refused(call(reserved=1), b"reserved")
    assert _refused(call(d_light_states=None), b"light state")
    assert _refused(call(d_light_states=R.states.data_ptr()), b"must not be d_states")
    assert _refused(call(frame=rtmi.make_frame(8, 8, 2, 6, post=True)), b"post_process")
    for depth in (-1, rtmi.MAX_DEPTH + 1):
        assert _refused(call(frame=rtmi.make_frame(8, 8, 2, depth, post=False)), b"depth", ERR_DEPTH)
    feat = _abi.feature_bufs(torch.zeros((R.items, 3), device=R.device))
    assert _refused(call(frame=rtmi.make_frame(8, 8, 2, 0, post=False), features=C.pointer(feat)), b"depth", ERR_DEPTH)
    for k in ("d_budget", "d_states", "d_sum", "d_samples", "d_work"):
        assert _refused(call(**{k: None}), b"null budget, state"), k
    torch.cuda.synchronize()
    rdl.assert_same_buffers(rdl.buffers(R), before, "a refused call wrote something")
    assert call() == 0  # nothing wrong: the same arguments render
    torch.cuda.synchronize()
    assert (R.samples.cpu().numpy() == 2).all()


def test_python_refuses_a_posted_frame_and_a_bad_budget():
    R = rdl.renderer("lamp_room", 8, 8, 2, 6)
    bt = rdl.budget_tensor(R, 2)
    with pytest.raises(rtmi.RtmiError):
        R.render_direct(bt[:32])
    with pytest.raises(rtmi.RtmiError):
        R.render_direct(bt.float())
    assert R.light_states is None and R.direct_counts is None and not R.samples.cpu().numpy().any()
    posted = rtmi.Renderer(rdl.scene("lamp_room"), 8, 8, 2, max_depth=6, post=True).init_rng()
    with pytest.raises(rtmi.RtmiError):
        posted.render_direct(bt)
    # render_adaptive itself is what it was: its passes are plain budget renders
    P, Q = (rdl.renderer("lamp_room", 8, 8, 4, 6) for _ in range(2))
    out = P.render_adaptive(4, 4, 4, 0.25, post=False)  # (min = max: one pass of four samples everywhere)
    assert out.passes == 1 and P.light_states is None and P.direct_counts is None
    Q.render_budget(rdl.budget_tensor(Q, 4)).check()
    rdl.assert_same_buffers(rdl.buffers(P), rdl.buffers(Q), "render_adaptive is render_budget's passes")
