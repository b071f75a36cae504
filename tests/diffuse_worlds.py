"""Worlds for the diffuse kernels (tests/test_gpu_diffuse_path.py; kernels.h: PIN_DIFFUSE).  Each `fill(b)` works on a
product or an oracle builder.

Sixteen materials are all that nibble ids name, and a fast list kernel asks for nibble ids.  So the room lit by a panel
has fifteen Lambertian colours and the light as its sixteenth material, id 15, and the room lit by the sky has sixteen
Lambertian colours and no light at all: its paths end in the sky, through the slot in the ceiling, or at the depth limit."""
import fast_trim_worlds as ft
from rtmi import scenes
from tri_tasks_worlds import v3

CORNELL_SEED = scenes.SCENE_SEEDS.get("cornell_box", 1024)
ROOM_SEED = 13


def diffuse_only(b):
    """SceneDev::diffuse_only as a commit of the product builder `b` would set it (rtmi_debug_diffuse_only, a diagnostic
    the binding does not declare: asked for by name).  Host only."""
    import ctypes as C
    fn = b.L.rtmi_debug_diffuse_only
    fn.restype, fn.argtypes = C.c_int, [C.c_void_p]
    rc = fn(b.h)
    assert rc in (0, 1), b.L.rtmi_last_error()
    return bool(rc)


def render_pins(pb, side, spp, depth, opts):
    """(first pass, finishing launch): the mode words of the kernels a render of this square frame of the committed
    builder `pb` would launch (rtmi_render_pins; 0: the general kernel, or no first pass).  `opts`: render_opts arguments."""
    import ctypes as C
    import rtmi
    R = rtmi.Renderer(pb, side, side, spp, depth, True)
    out = (C.c_uint32 * 2)()
    with R.torch.cuda.device(R.device):
        rc = R.L.rtmi_render_pins(R.scene.h, C.byref(R.frame), C.byref(rtmi.render_opts(**opts)), out)
    assert rc == 0, R.L.rtmi_last_error()
    return int(out[0]), int(out[1])


def cornell(b):
    scenes.cornell_box(b, 1.0)


def cornell_and_an_unused_metal(b):
    """The Cornell box, and a fifth material that no primitive has.  Neither builder draws a random number for a
    material, so the pixels' RNG states start as the Cornell box's, pixel 0's included."""
    scenes.cornell_box(b, 1.0)
    b.metal(v3(0.8, 0.85, 0.88), 0.25)


def panel_room(b):
    """The room of fast_trim_worlds with its ceiling's slot closed by a light panel: 15 Lambertians, the light is id 15."""
    ft._camera(b)
    m = [b.lambertian(ft.colour(k)) for k in range(15)]
    light = b.diffuse_light(b.constant_texture(v3(6.0, 5.5, 5.0)))
    ft._room(b, [m[k % 15] for k in range(16)])
    S = ft.SIZE
    b.parallelogram([v3(1.75, S, 0), v3(2.25, S, 0), v3(1.75, S, S)], light)


def sky_room(b):
    """The same room with sixteen Lambertians, lit by the sky through the slot alone."""
    ft._camera(b)
    m = [b.lambertian(ft.colour(k)) for k in range(16)]
    b.sky()
    ft._room(b, m)


WORLDS = {"cornell_box": (cornell, CORNELL_SEED), "unused_metal": (cornell_and_an_unused_metal, CORNELL_SEED),
          "panel_room": (panel_room, ROOM_SEED), "sky_room": (sky_room, ROOM_SEED)}
