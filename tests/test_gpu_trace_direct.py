"""rtmi_trace_direct on the GPU: per path the radiance, both RNG states, the ray count and the three counters of the loop
trace_steps(compact=True, direct="mis") on the same rays and states, bit for bit -- the loop's stacks folded forward
(tests/tracedirectlib.py) --, on every kind of scene the loop's own tests use, at wave edges and with lanes that refill,
with canaries around every output; bad rays left out; an empty table giving rtmi_trace; and Renderer.render_rays
(direct="fused") summing those very radiances.

No statistical test: bit equality with the loop's samples carries the 5-sigma expectation and variance results of
tests/test_gpu_direct_mis.py and tests/test_gpu_sphere_lights.py over to this entry."""
import ctypes as C
import functools
import math

import numpy as np
import pytest

import common
import directlib as dl
import mislib as ml
import rtmi
import spherelightlib as sl
import tracedirectlib as tdl
from abi_host import ERR_DEPTH, _refused
from parity import bits
from rtmi import _abi, scenes

pytestmark = pytest.mark.gpu
f32 = np.float32
PAD = 64
CANARY = 0x5a5a5a5a


def v3(*a):
    return np.array(a, dtype=f32)


def mesh_lamp_room(b):
    """A mesh of a few hundred faces on a Lambertian floor under a parallelogram lamp, a second mesh between them: shadow
    rays that walk the meshes' trees."""
    b.camera_pinhole(v3(0, 1.2, 4), v3(0, 0.6, 0), v3(0, 1, 0), 0.9, 1.0)
    grey = b.lambertian(v3(0.7, 0.7, 0.7))
    b.parallelogram([v3(-5, 0, -5), v3(5, 0, -5), v3(-5, 0, 5)], grey)
    b.parallelogram([v3(-5, 0, -3), v3(5, 0, -3), v3(-5, 6, -3)], b.lambertian(v3(0.4, 0.5, 0.8)))
    b.parallelogram([v3(-1.5, 4, -1.5), v3(1.5, 4, -1.5), v3(-1.5, 4, 1.5)], b.diffuse_light(b.constant_texture(v3(8, 7, 6))))
    low = scenes.procedural_bunny_mesh(8).reshape(-1, 3, 3).astype(f32)
    low = low - low.reshape(-1, 3).min(0) * v3(0, 1, 0)  # on the floor
    b.bvh(low.reshape(-1, 9), b.lambertian(v3(0.8, 0.5, 0.3)))
    high = scenes.procedural_bunny_mesh(6).reshape(-1, 3, 3).astype(f32) * f32(0.6) + v3(0.3, 2.5, 0.2)
    b.bvh(high.reshape(-1, 9), b.lambertian(v3(0.3, 0.7, 0.4)))
    return b


def textured_room(b):
    """One image-textured Lambertian floor under a lamp, a wall behind: A[k] of a floor vertex is a texel."""
    b.camera_pinhole(v3(0, 2, 5), v3(0, 0.5, 0), v3(0, 1, 0), 0.9, 1.0)
    img = np.random.default_rng(5).integers(30, 255, (8, 8, 4)).astype(np.uint8)
    b.parallelogram([v3(-4, 0, -4), v3(4, 0, -4), v3(-4, 0, 4)], b.lambertian_tex(b.image_texture(img)))
    b.parallelogram([v3(-4, 0, -4), v3(4, 0, -4), v3(-4, 5, -4)], b.lambertian(v3(0.6, 0.6, 0.6)))
    b.parallelogram([v3(-1, 3, -1), v3(1, 3, -1), v3(-1, 3, 1)], b.diffuse_light(b.constant_texture(v3(5, 5, 4))))
    return b


CUSTOM = {"lamp_room": dl.lamp_room, "close_lamp_room": ml.close_lamp_room, "many_lights": dl.many_lights_world(),
          "bulb_room": sl.with_kinds(sl.bulb_room, True), "bulb_room_flat": sl.bulb_room,
          "enclosing": sl.with_kinds(sl.enclosing_light, True), "mesh_lamp_room": mesh_lamp_room, "textured_room": textured_room}
SCENES = ["cornell_box", "lamp_room", "close_lamp_room", "bulb_room", "bulb_room_flat", "enclosing", "many_lights", "mesh_lamp_room",
          "textured_room", "sky_only"]
EMPTY_TABLE = ("bulb_room_flat", "sky_only")


@functools.lru_cache(maxsize=None)
def scene(name):
    """(committed scene, seed)."""
    if name in CUSTOM:
        return dl.build_custom(CUSTOM[name])[0], dl.LAMP_ROOM_SEED
    seed = common.scene_seed(name)
    return common.build_scene(rtmi.SceneBuilder(seed), name, 1.0).commit(), seed


@functools.lru_cache(maxsize=None)
def rays_of(name, n):
    """n camera rays of the scene's 16 x 16 frame (as many samples as n takes), on the device."""
    import torch
    b, _ = scene(name)
    O, D = dl.camera_rays(b, 16, 16, -(-n // 256), 300 + n)
    pick = np.random.default_rng(n).permutation(len(O))[:n]
    return torch.from_numpy(np.ascontiguousarray(O[pick])).cuda(), torch.from_numpy(np.ascontiguousarray(D[pick])).cuda()


def _guard(body, dtype):
    """A device tensor of PAD canary words, `body` (flat), PAD canary words; and the view of the body."""
    import torch
    full = torch.full((body.numel() + 2 * PAD,), CANARY if dtype != torch.float32 else -7.25, dtype=dtype, device="cuda")
    full[PAD:PAD + body.numel()] = body.reshape(-1).to(dtype)
    return full, full[PAD:PAD + body.numel()]


def _intact(full, n):
    import torch
    c = CANARY if full.dtype != torch.float32 else -7.25
    return bool((full[:PAD] == c).all() and (full[PAD + n:] == c).all())


def fused(b, o, d, states, ls, depth):
    """One rtmi_trace_direct through the C ABI with canaries around every output: dict of host arrays, and `intact`."""
    import torch
    n = int(o.shape[0])
    bufs = {"rgb": _guard(torch.full((n, 3), 9.0, device="cuda"), torch.float32), "states": _guard(states, torch.int32),
            "ls": _guard(ls, torch.int32), "rays": _guard(torch.full((n,), 77, device="cuda"), torch.int32),
            "counts": _guard(torch.zeros(3, device="cuda"), torch.int64),
            "work": _guard(torch.zeros(rtmi.TRACE_WORK_WORDS, device="cuda"), torch.int64)}
    a = _abi.TraceDirectArgs()
    a.size, a.reserved, a.n, a.max_depth = C.sizeof(_abi.TraceDirectArgs), 0, n, depth
    a.d_origins, a.d_dirs = o.data_ptr(), d.data_ptr()
    a.d_states, a.d_light_states = bufs["states"][1].data_ptr(), bufs["ls"][1].data_ptr()
    a.d_radiance, a.d_ray_counts = bufs["rgb"][1].data_ptr(), bufs["rays"][1].data_ptr()
    a.d_counts, a.d_work = bufs["counts"][1].data_ptr(), bufs["work"][1].data_ptr()
    rc = rtmi.lib().rtmi_trace_direct(b.h, C.byref(a), C.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert rc == 0, rtmi.lib().rtmi_last_error()
    torch.cuda.synchronize()
    out = {k: v[1].cpu().numpy() for k, v in bufs.items()}
    out["rgb"], out["states"], out["ls"] = out["rgb"].reshape(n, 3), out["states"].reshape(6, n), out["ls"].reshape(6, n)
    out["intact"] = all(_intact(full, body.numel()) for full, body in bufs.values())
    return out


def check_against_the_loop(name, n, depth):
    import torch
    b, seed = scene(name)
    o, d = rays_of(name, n)
    st, states, ls, counts = tdl.loop_of(b, o, d, seed + n + depth, depth)
    want = tdl.expected_radiance(st)
    s0, l0 = rtmi.rng_states(seed + n + depth, n), rtmi.rng_states(seed + n + depth, n, first=n)
    got = fused(b, o, d, s0, l0, depth)
    assert got["intact"], "a canary around an output was overwritten"
    bad = np.flatnonzero((bits(got["rgb"]) != bits(want)).any(1))
    assert bad.size == 0, (name, n, depth, bad[:8], got["rgb"][bad[:4]], want[bad[:4]])
    assert np.array_equal(got["states"], states.cpu().numpy()), "the path states are not the loop's"
    assert np.array_equal(got["ls"], ls.cpu().numpy()), "the light states are not the loop's"
    assert np.array_equal(got["rays"], (st.steps + st.alive.to(torch.int32)).cpu().numpy())
    loop_counts = [0, 0] if counts is None else [int(x) for x in counts.cpu()]
    assert got["counts"].tolist() == loop_counts + [int(st.occluded.sum())], (got["counts"], loop_counts)
    assert got["work"][0] == 0 and got["work"][1] == got["rays"].sum()
    return st, got


# ------------------------------------------------------------------ 1. the loop, bit for bit
@pytest.mark.parametrize("name", SCENES)
def test_scene_is_the_loop_bit_for_bit(name):
    st, got = check_against_the_loop(name, 300, 6)
    if name in EMPTY_TABLE:
        assert got["counts"].tolist() == [0, 0, 0]
    elif name == "enclosing":
        assert got["counts"].tolist() == [got["counts"][0], 0, 0] and got["counts"][0] > 0  # sampled, never valid, never weighed
    else:
        assert got["counts"][0] > 100 and got["counts"][1] > 0, "the case samples or weighs nothing"
        assert (st.direct.cpu().numpy() != 0).any()
    if name in ("lamp_room", "close_lamp_room", "mesh_lamp_room", "bulb_room"):
        assert got["counts"][2] > 0, "no shadow ray of the case is occluded"


@pytest.mark.parametrize("n", [1, 63, 64, 65, 300])
@pytest.mark.parametrize("name", ["lamp_room", "bulb_room"])
def test_wave_edges_and_refills(name, n):
    check_against_the_loop(name, n, 6)


@pytest.mark.parametrize("depth", [0, 1, 2, 3, 6, 50])
@pytest.mark.parametrize("name", ["cornell_box", "lamp_room", "bulb_room"])
def test_depths(name, depth):
    st, got = check_against_the_loop(name, 300, depth)
    if depth == 0:
        assert not got["rgb"].any() and got["counts"].tolist() == [0, 0, 0]
    if depth == 1:
        assert got["counts"][0] == 0  # the only vertex weighs (nothing: no flag is set) and does not sample
    if depth >= 2:
        assert got["counts"][0] > 0


# ------------------------------------------------------------------ 2. an empty table
@pytest.mark.parametrize("name", EMPTY_TABLE)
def test_empty_table_is_rtmi_trace(name):
    b, seed = scene(name)
    o, d = rays_of(name, 300)
    s0, s1, l0 = rtmi.rng_states(seed, 300), rtmi.rng_states(seed, 300), rtmi.rng_states(seed, 300, first=300)
    t = b.trace(o, d, s0, 6, count_rays=True).check()
    f = b.trace_direct(o, d, s1, l0, 6, count_rays=True).check()
    assert np.array_equal(f.rgb.cpu().numpy(), t.rgb.cpu().numpy())  # numerically: -0.0f == +0.0f
    assert not np.signbit(f.rgb.cpu().numpy()[f.rgb.cpu().numpy() == 0]).any()
    assert np.array_equal(f.rays.cpu().numpy(), t.rays.cpu().numpy()) and np.array_equal(s0.cpu().numpy(), s1.cpu().numpy())
    assert np.array_equal(l0.cpu().numpy(), rtmi.rng_states(seed, 300, first=300).cpu().numpy()), "a light state moved"
    assert f.counts.tolist() == [0, 0, 0] and f.total_rays() == t.total_rays()


# ------------------------------------------------------------------ 3. bad rays
def test_bad_rays_are_left_out():
    import torch
    name, n, depth = "lamp_room", 300, 6
    b, seed = scene(name)
    o, d = (t.clone() for t in rays_of(name, n))
    bad = np.array([0, 5, 63, 64, 127, 299])
    o[bad[0::2], 1] = float("nan")
    d[bad[1::2]] = 0.0
    good = np.setdiff1d(np.arange(n), bad)
    s0, l0 = rtmi.rng_states(seed, n), rtmi.rng_states(seed, n, first=n)
    got = fused(b, o, d, s0, l0, depth)
    assert got["intact"]
    assert not got["rgb"][bad].any() and not got["rays"][bad].any()
    assert np.array_equal(got["states"][:, bad], s0.cpu().numpy()[:, bad]) and np.array_equal(got["ls"][:, bad], l0.cpu().numpy()[:, bad])
    # the neighbours: what they get without the bad rays among them (path i's streams are subsequences i and n + i)
    og, dg = o[good].contiguous(), d[good].contiguous()
    ref = fused(b, og, dg, s0[:, good].contiguous(), l0[:, good].contiguous(), depth)
    assert np.array_equal(bits(got["rgb"][good]), bits(ref["rgb"])) and np.array_equal(got["rays"][good], ref["rays"])
    assert np.array_equal(got["states"][:, good], ref["states"]) and np.array_equal(got["ls"][:, good], ref["ls"])
    assert got["counts"].tolist() == ref["counts"].tolist()
    assert torch.isnan(o).any()


# ------------------------------------------------------------------ 4. refusals that need a committed scene
def test_depth_outside_its_range_and_python_refusals():
    b, seed = scene("lamp_room")
    o, d = rays_of("lamp_room", 64)
    s, ls = rtmi.rng_states(seed, 64), rtmi.rng_states(seed, 64, first=64)
    for depth in (-1, rtmi.MAX_DEPTH + 1):
        a = _abi.TraceDirectArgs()
        a.size, a.n, a.max_depth = C.sizeof(_abi.TraceDirectArgs), 64, depth
        a.d_origins, a.d_dirs, a.d_states, a.d_light_states = o.data_ptr(), d.data_ptr(), s.data_ptr(), ls.data_ptr()
        a.d_radiance = a.d_work = 16
        assert _refused(rtmi.lib().rtmi_trace_direct(b.h, C.byref(a), None), b"depth", ERR_DEPTH)
        with pytest.raises(rtmi.RtmiError):
            b.trace_direct(o, d, s, ls, depth)
    with pytest.raises(rtmi.RtmiError):
        b.trace_direct(o, d, s, s, 4)  # the two streams must be two tensors
    with pytest.raises(rtmi.RtmiError):
        b.trace_direct(o, d, s, ls[:, :32], 4)
    assert b.trace_direct(o[:0], d[:0], s[:, :0].contiguous(), ls[:, :0].contiguous(), 4).rgb.shape == (0, 3)  # launches nothing


# ------------------------------------------------------------------ 5. the renderer
def test_render_rays_fused_sums_the_expected_radiances_and_mis_is_the_loop():
    import torch
    b, seed = scene("lamp_room")
    h = w = 8
    spp, depth = 4, 6
    make = lambda: rtmi.Renderer(b, h, w, spp, max_depth=depth, post=False).init_rng()
    rf, rm = make(), make()
    ro = make()  # the oracle: the loop per sample, on its own states
    items = rf.items
    ro.light_states = rtmi.rng_states(b.seed, items, first=items, device=ro.device)
    total, loop_total = np.zeros((items, 3), f32), np.zeros((items, 3), f32)
    for sample in range(spp):
        o, d = ro.camera_rays(sample)
        st = b.trace_steps(o, d, ro.states, depth, compact=True, direct="mis", light_states=ro.light_states).check()
        total = (total + tdl.expected_radiance(st)).astype(f32)
        loop_total = (loop_total + st.rgb.cpu().numpy()).astype(f32)
    rf.render_rays(direct="fused")
    rm.render_rays(direct="mis")
    assert np.array_equal(bits(rf.sum.cpu().numpy()), bits(total))
    assert np.array_equal(bits(rm.sum.cpu().numpy()), bits(loop_total))
    assert np.array_equal(rf.states.cpu().numpy(), rm.states.cpu().numpy())
    assert np.array_equal(rf.light_states.cpu().numpy(), rm.light_states.cpu().numpy())
    assert int(rf.rays_total.item()) == int(rm.rays_total.item())
    with pytest.raises(rtmi.RtmiError):
        make().render_rays(direct="bogus")
    assert torch.isfinite(rf.sum).all() and math.isfinite(float(rf.sum.sum()))
