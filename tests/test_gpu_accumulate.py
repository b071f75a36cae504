"""rtmi_accumulate / rtmi_camera_update / Renderer.accumulate on the GPU: bit for bit against the numpy restatement of
tests/filter_rules.py (``accumulate_rule``) on its synthetic room, over chains of three frames so that the history
records are held to the rule too; a camera moved on a committed scene against a scene committed with that camera; and
the one thing no restatement can say: that accumulating a moving sequence lowers the error of its last frame.

Shapes are the smallest at which tiling and borders can go wrong: one pixel; one row or column of tiles narrower than a
tile; 16 x 16; and a frame ragged against the 32 x 8 tile in both directions with several tiles.  The four moves of the
host tests reach every branch of the rule (tests/test_accumulate_host.py asserts that)."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import common
import rtmi
from abi_host import CHECK_LIB, ROOT
from filter_rules import FOV, MOVES, SHAPES, accumulate_rule, camera_of, look_at, room
from filters_truth import LANDING_M, SNAP, landing_truth, same_or_nan
from parity import bits, same

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

F32 = np.float32
INPUTS = ("color", "variance", "normal", "depth", "alpha")
OTHER = dict(normal_min=-1.0, depth_tolerance=0.01, min_blend=0.0)


def on_gpu(d):
    return {k: torch.from_numpy(np.ascontiguousarray(v)).cuda() for k, v in d.items()}


def history_of(t, h, w):
    """A device history as the rule's (3, H, W, 4) float32 array: the bytes are the same."""
    return t.cpu().numpy().view(F32).reshape(3, h, w, 4)


def assert_exact(got, expected, what):
    for name, g, w_ in zip(("out", "out_variance", "out_length", "history"), got, expected):
        bad = bits(g) != bits(w_)
        assert g.shape == w_.shape and not bad.any(), "%s: %s differs in %d of %d floats, first at %s: %r != %r" % (
            what, name, bad.sum(), bad.size, np.argwhere(bad)[0], g[bad][0], w_[bad][0])


def chain(h, w, move, seed=0, **opts):
    """Three frames: the home camera without a history, the moved camera, the home camera again.  Yields (frame number, what
    the device gave, what the rule gives), each (out, variance, length, history)."""
    return chain_of(h, w, [camera_of("static", h, w), camera_of(move, h, w), camera_of("static", h, w)], seed, **opts)


def chain_of(h, w, cams, seed=0, **opts):
    """chain() over any sequence of cameras, the first without a history."""
    hist_dev = hist_rule = prev = None
    for k, cam in enumerate(cams):
        d = room(h, w, cam, seed=seed + k)
        exp = accumulate_rule(**d, camera=cam, history=hist_rule, prev_camera=prev, **opts)
        out, var, length, hist_dev = rtmi.accumulate(**on_gpu(d), camera=cam, history=hist_dev, prev_camera=prev, **opts)
        torch.cuda.synchronize()
        assert hist_dev.dtype == torch.uint8 and hist_dev.numel() == 48 * h * w
        yield k, (out.cpu().numpy(), var.cpu().numpy(), length.cpu().numpy(), history_of(hist_dev, h, w)), exp[:4]
        hist_rule, prev = exp[3], cam


# ------------------------------------------------------------------ 1. bit-exact against the restatement
@pytest.mark.parametrize("opts", [{}, OTHER], ids=["defaults", "other"])
@pytest.mark.parametrize("move", list(MOVES))
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "%dx%d" % s)
def test_accumulate_equals_the_rule(shape, move, opts):
    blended = False
    for k, got, exp in chain(*shape, move, **opts):
        assert_exact(got, exp, "%dx%d %s frame %d" % (shape + (move, k + 1)))
        blended |= bool((exp[2] > 1).any())
    if shape == (33, 70) and move != "about":
        assert blended  # the case is worth its name: some pixel took its history


# ------------------------------------------------------------------ 1b. long frames, the extreme extents, non-finite inputs
@pytest.mark.parametrize("shape", [(9, 300), (300, 9)], ids=lambda s: "%dx%d" % s)
def test_accumulate_long_thin_frames_equal_the_rule(shape):
    """Frames 300 pixels long one way (the rule blends 51 % of 9 x 300 and 45 % of 300 x 9 under "slide")."""
    for k, got, exp in chain(*shape, "slide"):
        assert_exact(got, exp, "%dx%d slide frame %d" % (shape + (k + 1,)))
        if k == 1:
            assert (exp[2] > 1).mean() >= 0.4


def extreme_slide(h, w):
    """A slide that keeps the points of an extreme frame on screen.  1 x 65535: "slide" itself; one pixel is wider than the
    room there, so it moves every point by less than a pixel, and half of the frame is background.  65535 x 1: "slide" leaves
    the single column, so the camera and its target move up by 0.05 instead, 3 pixel heights at the back wall and more nearer."""
    if h == 1:
        return camera_of("slide", h, w)
    return look_at((278, 273.05, -800), (278, 273.05, 0), aspect=w / h)


@pytest.mark.parametrize("move", ["static", "slide"])
@pytest.mark.parametrize("shape", [(1, 65535), (65535, 1)], ids=lambda s: "%dx%d" % s)
def test_accumulate_extreme_extents_equal_the_rule(shape, move):
    h, w = shape
    home = camera_of("static", h, w)
    for k, got, exp in chain_of(h, w, [home, home if move == "static" else extreme_slide(h, w)]):
        assert_exact(got, exp, "%dx%d %s frame %d" % (shape + (move, k + 1)))
    assert (exp[2] > 1).mean() >= 0.25  # (the rule alone says so: the history was taken, not only passed by)


OUTPUTS = ("out", "out_variance", "out_length", "history")


def pixel_differs(g, c):
    """(H, W) bool: where two outputs of one kind differ in any bit of the pixel (a history is (3, H, W, 4))."""
    x = bits(g) != bits(c)
    return x.any(axis=(0, 3)) if x.ndim == 4 else x.any(axis=-1) if x.ndim == 3 else x


def _second_frame(d1, cam1, hist0, cam0):
    """The second frame of a sequence on the device and by the rule: each (out, variance, length, history)."""
    hist_in = torch.from_numpy(np.ascontiguousarray(hist0).view(np.uint8).reshape(-1)).cuda()
    h, w = d1["depth"].shape
    out, var, length, hist = rtmi.accumulate(**on_gpu(d1), camera=cam1, history=hist_in, prev_camera=cam0)
    torch.cuda.synchronize()
    exp = accumulate_rule(**d1, camera=cam1, history=hist0, prev_camera=cam0)
    return (out.cpu().numpy(), var.cpu().numpy(), length.cpu().numpy(), history_of(hist, h, w)), exp[:4]


def _slide_33x70():
    h, w = 33, 70
    cam0, cam1 = camera_of("static", h, w), camera_of("slide", h, w)
    d0, d1 = room(h, w, cam0, seed=8), room(h, w, cam1, seed=9)
    return d1, cam1, accumulate_rule(**d0, camera=cam0)[3], cam0


@pytest.mark.parametrize("what", ["nan_depth", "inf_depth", "nan_color"])
def test_accumulate_non_finite_frame_pixel_touches_nothing_else(what):
    """One non-finite input in a frame whose pixel would take its history: the call does not fault and equals the rule (a
    NaN for a NaN); a non-finite depth makes the pixel fresh ("a NaN is fresh too"), a NaN colour stays that pixel's; and
    every other pixel of every output has the clean run's bits."""
    d1, cam1, hist0, cam0 = _slide_33x70()
    at = (16, 36)
    clean, _ = _second_frame(d1, cam1, hist0, cam0)
    assert clean[2][at] > 1
    d = {k: v.copy() for k, v in d1.items()}
    if what == "nan_color":
        d["color"][at][1] = np.nan
    else:
        d["depth"][at] = np.nan if what == "nan_depth" else np.inf
    got, exp = _second_frame(d, cam1, hist0, cam0)
    other = np.ones(clean[2].shape, bool)
    other[at] = False
    for name, g, e, c in zip(OUTPUTS, got, exp, clean):
        assert same_or_nan(g, e).all(), (what, name, np.argwhere(~same_or_nan(g, e))[0])
        assert not pixel_differs(g, c)[other].any(), (what, name)
    if what == "nan_color":
        assert np.isnan(got[0][at][1]) and got[2][at] == clean[2][at]
    else:
        assert got[2][at] == 1 and same(got[0][at], d["color"][at]) and same(got[1][at], d["variance"][at])


def test_accumulate_nan_in_the_history_stays_with_its_taps():
    """A NaN in one history record: the device equals the rule, some pixel takes it, and only pixels whose four taps include
    the record differ from the clean run -- their landing point, by tests/filters_truth.py's binary64 projection, is less
    than a pixel and the snap away from it in both axes."""
    d1, cam1, hist0, cam0 = _slide_33x70()
    at = (16, 36)
    clean, _ = _second_frame(d1, cam1, hist0, cam0)
    hist = hist0.copy()
    hist[1, at[0], at[1], 0] = np.nan
    got, exp = _second_frame(d1, cam1, hist, cam0)
    differs = np.zeros(clean[2].shape, bool)
    for name, g, e, c in zip(OUTPUTS, got, exp, clean):
        assert same_or_nan(g, e).all(), (name, np.argwhere(~same_or_nan(g, e))[0])
        differs |= pixel_differs(g, c)
    assert differs.any() and np.isnan(got[0][differs]).any()
    # a tap of the record: the rule's landing point is less than a pixel from it, and the truth within SNAP + m of that
    fx, fy, _, _ = landing_truth(*differs.shape, cam1, cam0, d1["depth"])
    reach = 1 + SNAP + LANDING_M
    assert (np.abs(fx[differs] - at[1]) < reach).all() and (np.abs(fy[differs] - at[0]) < reach).all()


def _raw(h, w, t, cam, hist_in, prev, hist_out, out, out_var, out_len, **opts):
    """rtmi_accumulate itself, on tensors the caller chose (None: a null pointer)."""
    L = rtmi.lib()
    fp = C.POINTER(C.c_float)
    o = dict(rtmi.ACCUMULATE_DEFAULTS, **opts)
    ao = rtmi.AccumulateOpts(C.sizeof(rtmi.AccumulateOpts), 0, o["normal_min"], o["depth_tolerance"], o["min_blend"])
    g = rtmi.DenoiseGuides(C.sizeof(rtmi.DenoiseGuides), 0, t["variance"].data_ptr(), None, t["normal"].data_ptr(),
                           t["depth"].data_ptr(), t["alpha"].data_ptr())
    ptr = lambda x: None if x is None else C.c_void_p(x.data_ptr())
    cam_p = lambda a: None if a is None else np.ascontiguousarray(a, dtype=F32).ctypes.data_as(fp)
    rc = L.rtmi_accumulate(h, w, C.byref(ao), ptr(t["color"]), C.byref(g), cam_p(cam), ptr(hist_in), cam_p(prev), ptr(hist_out),
                           ptr(out), ptr(out_var), ptr(out_len), C.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert rc == 0, L.rtmi_last_error()


def test_accumulate_in_place_and_without_the_nullable_outputs():
    """d_out == d_color and d_out_variance == g->d_variance: the same bits as out of place; and without d_out_variance and
    d_out_length the colour and the history are the same bits."""
    h, w = 33, 70
    cam0, cam1 = camera_of("static", h, w), camera_of("slide", h, w)
    d0, d1 = room(h, w, cam0, seed=3), room(h, w, cam1, seed=4)
    hist0 = accumulate_rule(**d0, camera=cam0)[3]
    exp = accumulate_rule(**d1, camera=cam1, history=hist0, prev_camera=cam0)
    hist_in = torch.from_numpy(hist0.view(np.uint8).reshape(-1)).cuda()
    for in_place in (True, False):
        t = on_gpu(d1)
        hist_out = torch.zeros((48 * h * w,), dtype=torch.uint8, device="cuda")
        out = t["color"] if in_place else torch.zeros((h, w, 3), dtype=torch.float32, device="cuda")
        _raw(h, w, t, cam1, hist_in, cam0, hist_out, out, t["variance"] if in_place else None, None)
        torch.cuda.synchronize()
        assert same(out.cpu().numpy(), exp[0]) and same(history_of(hist_out, h, w), exp[3])
        if in_place:
            assert same(t["variance"].cpu().numpy(), exp[1])
        for k in INPUTS[0 if not in_place else 2:]:  # (what was not written over is an input only)
            assert same(t[k].cpu().numpy(), d1[k]), k
    assert same(history_of(hist_in, h, w), hist0)


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "%dx%d" % s)
def test_a_static_camera_is_the_running_mean_on_the_device(shape):
    """min_blend 0, three frames from one camera: L is 1, 2, 3 on surface pixels and C_k = (1 - 1/k) C_{k-1} + (1/k) c_k."""
    h, w = shape
    cam = camera_of("static", h, w)
    hist, mean = None, None
    for k in (1, 2, 3):
        d = room(h, w, cam, seed=10 + k)
        surf = d["alpha"] > 0
        out, var, length, hist = rtmi.accumulate(**on_gpu(d), camera=cam, history=hist, prev_camera=None if k == 1 else cam,
                                                 min_blend=0.0)
        torch.cuda.synchronize()
        a = F32(1) / F32(k)
        mean = d["color"] if k == 1 else np.where(surf[..., None], (F32(1) - a) * mean + a * d["color"], d["color"])
        assert same(length.cpu().numpy(), np.where(surf, F32(k), F32(1)))
        assert same(out.cpu().numpy(), mean)


@pytest.mark.parametrize("move", list(MOVES))
def test_min_blend_one_returns_the_frame_on_the_device(move):
    h, w = 33, 70
    cam0, cam1 = camera_of("static", h, w), camera_of(move, h, w)
    _, _, _, hist = rtmi.accumulate(**on_gpu(room(h, w, cam0)), camera=cam0)
    d = room(h, w, cam1, seed=1)
    out, var, length, _ = rtmi.accumulate(**on_gpu(d), camera=cam1, history=hist, prev_camera=cam0, min_blend=1.0)
    torch.cuda.synchronize()
    assert same(out.cpu().numpy(), d["color"]) and same(var.cpu().numpy(), d["variance"])


# ------------------------------------------------------------------ 2. the camera of a committed scene moves
CAMERAS = {"cornell_box": (((278, 278, -800), (278, 278, 0)), ((318, 283, -780), (278, 278, 0))),
           "bunny": (((-0.025, 0.1, -0.5), (-0.025, 0.1, 0)), ((0.03, 0.12, -0.48), (-0.025, 0.1, 0)))}
UP = (0, 1, 0)


def scene_with(name, camera=None):
    """The named scene, committed -- with `camera` (position, target) in place of its own when given."""
    b = common.build_scene(rtmi.SceneBuilder(common.scene_seed(name)), name, 1.0)
    if camera is not None:
        b.camera_pinhole(camera[0], camera[1], UP, FOV, 1.0)
    return b.commit()


def frames_of(b, spp, scratch=False):
    """Everything a render and a feature render of scene b leave behind, as numpy arrays by name."""
    R = rtmi.Renderer(b, 32, 32, spp, 10, post=False).init_rng()
    keep = R.new_scratch() if scratch else None
    R.render(opts=rtmi.render_opts(scratch=keep) if scratch else None)
    got = {"total": np.array(R.total_rays(keep))}
    got.update({k: getattr(R, k).cpu().numpy() for k in ("tiles", "ray_counts", "states")})
    B = rtmi.Renderer(b, 32, 32, spp, 10, post=False).init_rng()
    B.render_budget(torch.full((B.items,), spp, dtype=torch.int32, device="cuda"), features=True)
    B.check()
    got.update({"budget_" + k: getattr(B, k).cpu().numpy()
                for k in ("states", "sum", "sq", "samples", "budget_rays", "albedo", "normal", "depth", "coverage")})
    return got


def assert_same_frames(a, b, what):
    assert a.keys() == b.keys()
    for k in a:
        assert a[k].shape == b[k].shape and a[k].tobytes() == b[k].tobytes(), (what, k)


@pytest.mark.parametrize("name,spp", [("cornell_box", 4), ("bunny", 2)])
def test_camera_update_equals_a_commit_with_that_camera(name, spp):
    cam_a, cam_b = CAMERAS[name]
    want_a, want_b = frames_of(scene_with(name, cam_a), spp), frames_of(scene_with(name, cam_b), spp)
    assert want_a["tiles"].tobytes() != want_b["tiles"].tobytes()
    b = scene_with(name, cam_a)
    stats = b.stats()
    b.camera_look(cam_b[0], cam_b[1], UP, FOV, 1.0)
    assert b.stats() == stats
    assert same(b.camera_get(), scene_with(name, cam_b).camera_get())
    assert_same_frames(frames_of(b, spp), want_b, "updated to B")
    assert_same_frames(frames_of(b, spp, scratch=True), frames_of(scene_with(name, cam_b), spp, scratch=True), "B, own scratch")
    # and back: enqueue with A, update to B at once, no synchronisation between -- the work keeps A
    b.camera_look(cam_a[0], cam_a[1], UP, FOV, 1.0)
    for scratch in (False, True):
        R = rtmi.Renderer(b, 32, 32, spp, 10, post=False).init_rng()
        B = rtmi.Renderer(b, 32, 32, spp, 10, post=False).init_rng()
        budget = torch.full((B.items,), spp, dtype=torch.int32, device="cuda")
        keep = R.new_scratch() if scratch else None
        torch.cuda.synchronize()
        R.render(opts=rtmi.render_opts(scratch=keep) if scratch else None)
        B.render_budget(budget, features=True)
        b.camera_look(cam_b[0], cam_b[1], UP, FOV, 1.0)
        torch.cuda.synchronize()
        for k in ("tiles", "ray_counts", "states"):
            assert getattr(R, k).cpu().numpy().tobytes() == want_a[k].tobytes(), (scratch, k)
        for k in ("states", "sum", "sq", "samples", "budget_rays", "albedo", "normal", "depth", "coverage"):
            assert getattr(B, k).cpu().numpy().tobytes() == want_a["budget_" + k].tobytes(), (scratch, k)
        b.camera_look(cam_a[0], cam_a[1], UP, FOV, 1.0)


# ------------------------------------------------------------------ 3. the Python sequence
def test_renderer_accumulate_equals_the_rule_on_its_untiled_buffers():
    """Three frames of the Cornell box, camera_look between them: what Renderer.accumulate returns and what its Accumulator
    holds are the rule on the frames' own untiled buffers; new_frame() zeroes the sums and lets the RNG states go on."""
    b = scene_with("cornell_box")
    R = rtmi.Renderer(b, 64, 64, 4, 10, post=False).init_rng()
    acc = rtmi.Accumulator(64, 64)
    budget = torch.full((R.items,), 4, dtype=torch.int32, device="cuda")
    hist = prev = None
    assert acc.frames == 0
    for k, x in enumerate((278, 300, 322)):
        b.camera_look((x, 278, -800), (278, 278, 0), UP, FOV, 1.0)
        states = R.states.clone()
        R.new_frame()
        for name in ("sum", "sq", "samples", "budget_rays", "budget_abandoned", "albedo", "normal", "depth", "coverage"):
            assert not getattr(R, name).any(), name
        assert torch.equal(R.states, states)
        R.render_budget(budget, features=True)
        assert not torch.equal(R.states, states) and int(R.samples.max().item()) == 4
        buf = {n: t.cpu().numpy() for n, t in R.denoise_inputs().items()}
        res = R.accumulate(acc)
        torch.cuda.synchronize()
        cam = b.camera_get()
        exp = accumulate_rule(*(buf[n] for n in INPUTS), camera=cam, history=hist, prev_camera=prev)
        assert set(res) == set(buf) and acc.frames == k + 1
        assert_exact((res["color"].cpu().numpy(), res["variance"].cpu().numpy()), exp[:2], "frame %d" % (k + 1))
        assert same(history_of(acc.history, 64, 64), exp[3])
        for n in ("normal", "depth", "alpha", "albedo"):
            assert same(res[n].cpu().numpy(), buf[n]), n
        if k:
            assert exp[4]["taps_1_3"] + exp[4]["taps_4"] > 0.25 and not same(exp[0], buf["color"])
        hist, prev = exp[3], cam
    acc.reset()
    assert acc.frames == 0
    res = R.accumulate(acc)
    torch.cuda.synchronize()
    assert same(res["color"].cpu().numpy(), buf["color"]) and acc.frames == 1  # (a first frame again)


# ------------------------------------------------------------------ 4. it accumulates
def err(x, ref):
    x, ref = x.astype(np.float64), ref.astype(np.float64)
    return float(((x - ref) ** 2 / (ref ** 2 + 0.01)).mean())


SWEEPS = {"cornell_box": ([(278 + 10 * k, 278, -800) for k in range(8)], (278, 278, 0)),
          "bunny": ([(-0.025 + 0.006 * k, 0.1, -0.5) for k in range(8)], (-0.025, 0.1, 0))}


@pytest.mark.parametrize("name", ["cornell_box", "bunny"])
def test_it_accumulates(name):
    """Eight frames of 4 samples per pixel while the camera slides (the Cornell box: x = 278 .. 348 in equal steps, the target
    fixed), default options, against the library's own 4096-spp render of the last camera with another seed:
    err(accumulated) < err(the last frame alone) and err(denoise(accumulated)) < err(denoise(the last frame alone)) -- a
    condition, not a tuned number, on the Cornell box.  The bunny's figures are printed and not gated: its silhouettes
    restart by design.  Measured on an MI355X: see DESIGN.md 2.9."""
    positions, target = SWEEPS[name]
    ref_scene = common.build_scene(rtmi.SceneBuilder(common.scene_seed(name) + 977), name, 1.0)
    ref_scene.camera_pinhole(positions[-1], target, UP, FOV, 1.0)
    ref_scene.commit()
    Rr = rtmi.Renderer(ref_scene, 64, 64, 4096, 10, post=False).init_rng()
    Rr.render()
    ref = (Rr.untile()[0].cpu().numpy().astype(np.float64) / 4096).astype(F32)
    b = scene_with(name)
    R = rtmi.Renderer(b, 64, 64, 4, 10, post=False).init_rng()
    acc = rtmi.Accumulator(64, 64)
    budget = torch.full((R.items,), 4, dtype=torch.int32, device="cuda")
    for pos in positions:
        b.camera_look(pos, target, UP, FOV, 1.0)
        R.new_frame().render_budget(budget, features=True)
        alone = R.denoise_inputs()
        both = R.accumulate(acc)
    den_alone, den_both = rtmi.denoise(**alone), rtmi.denoise(**both)
    length = acc.history.view(torch.float32).view(3, 64, 64, 4)[1, ..., 3]
    torch.cuda.synchronize()
    e = {k: err(t.cpu().numpy(), ref) for k, t in (("alone", alone["color"]), ("accumulated", both["color"]),
                                                   ("denoised alone", den_alone), ("denoised accumulated", den_both))}
    print("accumulate %s: err %s; mean length %.3f" % (name, ", ".join("%s %.6f" % kv for kv in e.items()), float(length.mean())))
    assert acc.frames == 8
    if name == "cornell_box":
        assert e["accumulated"] < e["alone"], e
        assert e["denoised accumulated"] < e["denoised alone"], e


# ------------------------------------------------------------------ 5. shares no device state
def test_accumulate_runs_beside_a_budget_render():
    h, w = 70, 130
    cam0, cam1 = camera_of("static", h, w), camera_of("slide", h, w)
    d0, d1 = room(h, w, cam0, seed=5), room(h, w, cam1, seed=6)
    hist0 = accumulate_rule(**d0, camera=cam0)[3]
    exp = accumulate_rule(**d1, camera=cam1, history=hist0, prev_camera=cam0)
    b = scene_with("cornell_box")
    budget = None
    runs = []
    for beside in (False, True):
        R = rtmi.Renderer(b, 64, 64, 16, 10, post=False).init_rng()
        budget = torch.full((R.items,), 8, dtype=torch.int32, device="cuda")
        R._budget_buffers(), R._feature_buffers()
        t = on_gpu(d1)
        hist_in = torch.from_numpy(hist0.view(np.uint8).reshape(-1)).cuda()
        torch.cuda.synchronize()
        side = torch.cuda.Stream()
        R.render_budget(budget, features=True)
        if beside:
            with torch.cuda.stream(side):
                got = rtmi.accumulate(**t, camera=cam1, history=hist_in, prev_camera=cam0)
        torch.cuda.synchronize()
        R.check()
        runs.append({k: getattr(R, k).clone() for k in ("sum", "sq", "samples", "states", "albedo", "depth")})
    assert_exact([x.cpu().numpy() for x in got[:3]] + [history_of(got[3], h, w)], exp[:4], "beside a render")
    for k, v in runs[0].items():
        assert torch.equal(runs[1][k], v), k


# ------------------------------------------------------------------ 6. the check build
def check_one_shape():
    for k, got, exp in chain(33, 70, "slide", seed=7):
        assert_exact(got, exp, "33x70 slide frame %d" % (k + 1))


def test_check_build_gives_the_same_bits():
    """librtmi_check1.so compiles the accumulate kernel too: loaded in a process of its own, it meets the rule on one shape."""
    assert os.path.exists(CHECK_LIB), "librtmi_check1.so missing: __graft_entry__.build() builds it"
    env = dict(os.environ, RTMI_LIB_PATH=CHECK_LIB)
    env["PYTHONPATH"] = os.pathsep.join([os.path.join(ROOT, "ray-tracing-cuda_amd"), os.path.join(ROOT, "tests")])
    r = subprocess.run([sys.executable, os.path.abspath(__file__)], env=env, cwd=ROOT, stdout=subprocess.PIPE,
                       stderr=subprocess.PIPE, text=True, timeout=600)
    assert r.returncode == 0 and "check build ok" in r.stdout, (r.stdout[-2000:], r.stderr[-4000:])


if __name__ == "__main__":
    assert rtmi.LIB_PATH == CHECK_LIB or "check1" in rtmi.LIB_PATH, rtmi.LIB_PATH
    check_one_shape()
    print("check build ok")
