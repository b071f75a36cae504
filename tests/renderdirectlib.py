"""What the rtmi_render_direct tests share: the sample rule of include/rtmi.h restated in numpy, the scenes, twin renderers,
the parent's composition render_rays(direct="fused") with its per-sample counters collected, and the entry through the raw
C ABI with canaries around every output."""
import ctypes as C
import functools
import math

import numpy as np

import rtmi
from rtmi import _abi

f32 = np.float32
PAD = 64
CANARY = 0x5a5a5a5a
CANARY_F = -7.25


# ------------------------------------------------------------------ the sample rule, restated
def fold_samples(r_path, acc, s0=None, q0=None):
    """include/rtmi.h "render direct" in binary32 for one item: for every sample k in order, x = r_path[k] + acc[k] (ONE
    addition per channel), then sum += x and sq += x * x, the product and the sum rounded on their own.  r_path, acc
    (K, 3) float32; s0, q0 (3,): what the buffers hold before (zeros).  Returns (sum, sq, the samples' values (K, 3))."""
    r_path, acc = np.asarray(r_path, dtype=f32).reshape(-1, 3), np.asarray(acc, dtype=f32).reshape(-1, 3)
    s = np.zeros(3, f32) if s0 is None else np.asarray(s0, dtype=f32).copy()
    q = np.zeros(3, f32) if q0 is None else np.asarray(q0, dtype=f32).copy()
    xs = np.zeros_like(r_path)
    with np.errstate(all="ignore"):
        for k in range(r_path.shape[0]):
            x = (r_path[k] + acc[k]).astype(f32)
            s = (s + x).astype(f32)
            q = (q + (x * x).astype(f32)).astype(f32)
            xs[k] = x
    return s, q, xs


# ------------------------------------------------------------------ the scenes
def v3(*a):
    return np.array(a, dtype=f32)


def mesh_lamp_room(b):
    """A mesh of a few hundred faces on a Lambertian floor under a parallelogram lamp, a second mesh between them: shadow
    rays that walk the meshes' trees."""
    from rtmi import scenes
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
    """One image-textured Lambertian floor under a lamp, a wall behind: the attenuation of a floor vertex is a texel."""
    b.camera_pinhole(v3(0, 2, 5), v3(0, 0.5, 0), v3(0, 1, 0), 0.9, 1.0)
    img = np.random.default_rng(5).integers(30, 255, (8, 8, 4)).astype(np.uint8)
    b.parallelogram([v3(-4, 0, -4), v3(4, 0, -4), v3(-4, 0, 4)], b.lambertian_tex(b.image_texture(img)))
    b.parallelogram([v3(-4, 0, -4), v3(4, 0, -4), v3(-4, 5, -4)], b.lambertian(v3(0.6, 0.6, 0.6)))
    b.parallelogram([v3(-1, 3, -1), v3(1, 3, -1), v3(-1, 3, 1)], b.diffuse_light(b.constant_texture(v3(5, 5, 4))))
    return b


def defocus_lamp_room(b):
    """directlib.lamp_room seen through a lens: four camera draws per sample."""
    import directlib as dl
    dl.lamp_room(b)
    b.camera_defocus(v3(5, 5, 9.5), v3(5, 4, 0), v3(0, 1, 0), math.pi / 3, 1.0, 0.3, 7.0)
    return b


def _custom():
    import directlib as dl
    import mislib as ml
    import spherelightlib as sl
    return {"lamp_room": dl.lamp_room, "close_lamp_room": ml.close_lamp_room, "bulb_room": sl.with_kinds(sl.bulb_room, True),
            "bulb_room_flat": sl.bulb_room, "enclosing": sl.with_kinds(sl.enclosing_light, True), "mesh_lamp_room": mesh_lamp_room,
            "textured_room": textured_room, "defocus_lamp_room": defocus_lamp_room}


SCENES = ["cornell_box", "lamp_room", "close_lamp_room", "bulb_room", "bulb_room_flat", "enclosing", "mesh_lamp_room",
          "textured_room", "sky_only"]
EMPTY_TABLE = ("bulb_room_flat", "sky_only")
OCCLUDES = ("lamp_room", "close_lamp_room", "mesh_lamp_room", "bulb_room")


@functools.lru_cache(maxsize=None)
def scene(name):
    """The committed scene `name`, built once."""
    import common
    import directlib as dl
    custom = _custom()
    if name in custom:
        return dl.build_custom(custom[name])[0]
    return common.build_scene(rtmi.SceneBuilder(common.scene_seed(name)), name, 1.0).commit()


# ------------------------------------------------------------------ renderers
def renderer(name, h, w, spp, depth, rank=0, world=1):
    """A fresh Renderer of the scene with its budget buffers made: twins are two of these."""
    R = rtmi.Renderer(scene(name), h, w, spp, max_depth=depth, post=False, rank=rank, world_size=world).init_rng()
    R._budget_buffers()
    return R


def budget_tensor(R, values):
    """(items,) int32 CUDA tensor: `values` a number for every item, or a per-item array of uint32 words."""
    import torch
    a = np.full(R.items, values, dtype=np.int64) if np.isscalar(values) else np.asarray(values, dtype=np.int64)
    assert a.shape == (R.items,)
    return torch.from_numpy(a.astype(np.uint32).view(np.int32)).to(R.device)


def ragged_budget(R, seed=3, hi=5):
    """0 .. hi per item with a fifth of them zero, as a host array."""
    rng = np.random.default_rng(seed + R.items)
    b = rng.integers(0, hi + 1, R.items)
    b[rng.random(R.items) < 0.2] = 0
    return b


class Loop:
    """What the parent's composition leaves besides the renderer's buffers: the sum of the per-sample rtmi_trace_direct
    counters and of their query totals."""

    def __init__(self):
        self.counts = np.zeros(3, np.int64)
        self.queries = 0

    def render(self, R, budget):
        """R.render_rays(budget, direct="fused"), every trace_direct's counts and work[1] added up."""
        b = R.scene
        inner = b.trace_direct

        def spy(*a, **kw):
            t = inner(*a, **kw)
            self.counts += t.counts.cpu().numpy()
            self.queries += int(t.work[1].item())
            return t
        b.trace_direct = spy
        try:
            R.render_rays(budget, direct="fused")
        finally:
            del b.trace_direct
        return self


FIELDS = ("sum", "sq", "samples", "budget_rays", "states", "light_states")


def buffers(R):
    """Host copies of the buffers the two ways must agree on (light states: zeros' place-holder None before first use)."""
    import torch
    torch.cuda.synchronize()
    return {k: (getattr(R, k).cpu().numpy().copy() if getattr(R, k) is not None else None) for k in FIELDS}


def assert_same_buffers(got, want, what=""):
    for k in FIELDS:
        assert (got[k] is None) == (want[k] is None), "%s: %s is missing on one side" % (what, k)
        if got[k] is None:
            continue
        a, b = np.ascontiguousarray(got[k]), np.ascontiguousarray(want[k])
        assert a.shape == b.shape and a.dtype == b.dtype, (what, k)
        bad = np.flatnonzero((a.view(np.uint32) != b.view(np.uint32)).reshape(a.shape[0], -1).any(1)) if a.size else []
        assert len(bad) == 0, "%s: %s differ at %s: %s against %s" % (what, k, bad[:6], a[bad[:3]], b[bad[:3]])


# ------------------------------------------------------------------ the entry through the raw C ABI
def _guard(body, dtype):
    """A device tensor of PAD canary words, `body` (flat), PAD canary words; and the view of the body."""
    import torch
    full = torch.full((body.numel() + 2 * PAD,), CANARY if dtype != torch.float32 else CANARY_F, dtype=dtype, device=body.device)
    full[PAD:PAD + body.numel()] = body.reshape(-1).to(dtype)
    return full, full[PAD:PAD + body.numel()]


def _intact(full, n):
    import torch
    c = CANARY if full.dtype != torch.float32 else CANARY_F
    return bool((full[:PAD] == c).all() and (full[PAD + n:] == c).all())


def direct_args(R, budget, bodies, feat=None):
    """rtmi_render_direct_args over `bodies` (name -> tensor)."""
    a = _abi.RenderDirectArgs()
    a.size, a.reserved = C.sizeof(_abi.RenderDirectArgs), 0
    a.d_budget = budget.data_ptr()
    a.d_states, a.d_light_states = bodies["states"].data_ptr(), bodies["light_states"].data_ptr()
    a.d_sum, a.d_sq, a.d_samples = bodies["sum"].data_ptr(), bodies["sq"].data_ptr(), bodies["samples"].data_ptr()
    a.d_ray_counts, a.d_counts, a.d_work = bodies["budget_rays"].data_ptr(), bodies["counts"].data_ptr(), bodies["work"].data_ptr()
    if feat is not None:
        a.features = C.pointer(feat)
    return a


def raw_direct(R, budget, features=False):
    """One rtmi_render_direct through the C ABI on guarded copies of the renderer's buffers, which get the results back:
    {"counts": (3,), "work": (words,), "intact": no canary was overwritten}."""
    import torch
    R._budget_buffers()
    R._light_states()
    names = {"states": torch.int32, "light_states": torch.int32, "sum": torch.float32, "sq": torch.float32, "samples": torch.int32,
             "budget_rays": torch.int32}
    if features:
        R._feature_buffers()
        names.update({"albedo": torch.float32, "normal": torch.float32, "depth": torch.float32, "coverage": torch.int32})
    bufs = {k: _guard(getattr(R, k), dt) for k, dt in names.items()}
    bufs["counts"] = _guard(torch.zeros(3, device=R.device), torch.int64)
    bufs["work"] = _guard(torch.zeros(rtmi.BUDGET_WORK_WORDS, device=R.device), torch.int64)
    bodies = {k: v[1] for k, v in bufs.items()}
    feat = _abi.feature_bufs(bodies["albedo"], bodies["normal"], bodies["depth"], bodies["coverage"]) if features else None
    a = direct_args(R, budget, bodies, feat)
    with torch.cuda.device(R.device):
        rc = rtmi.lib().rtmi_render_direct(R.scene.h, C.byref(R.frame), C.byref(a), C.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert rc == 0, rtmi.lib().rtmi_last_error()
    torch.cuda.synchronize()
    for k in names:
        getattr(R, k).copy_(bodies[k].reshape(getattr(R, k).shape))
    return {"counts": bodies["counts"].cpu().numpy(), "work": bodies["work"].cpu().numpy(),
            "intact": all(_intact(full, body.numel()) for full, body in bufs.values())}
