"""What the binding says when it refuses a tensor, pinned word for word, and that it refuses before any GPU work.

Every tensor argument of every tensor-taking entry is replaced in turn by a tensor of a wrong dtype, of a wrong shape (one
dimension too many), of a wrong length (one more along the first dimension), by a non-contiguous view and by a CPU tensor.
The call must raise ``RtmiError`` with exactly the text of EXPECT, and every tensor the call could have written -- the
outputs hold a sentinel -- must be as it was.  EXPECT was recorded from the single-file binding before it was split into
modules; the entries marked REGULARISED hold the one sentence of ``_need`` where the old text left out "contiguous", added
an "or None" tail or did not name the tensor and the device (the commit that split the binding lists old and new).  Where
the binding accepts a corruption -- it makes rays and t_max contiguous itself -- EXPECT holds None and the call must succeed.
A one-element tensor has no non-contiguous view, so the counts of ``Paths`` are not tried with one.

The shapes are the smallest that reach every check: one sphere under a sky, N = 5 rays, an 8 x 8 frame (one tile, 64
items) at 1 sample, max_depth 2, post=False."""
import math

import pytest

import rtmi

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

N, H, W, DEPTH, LAYERS = 5, 8, 8, 2, 2
KINDS = ("dtype", "shape", "length", "strided", "cpu")
F32_SENTINEL, INT_SENTINEL = 7.5, 0x5A


class Env:
    """The committed scene, its renderer, and one good step to sample the lights from."""

    def __init__(self):
        b = rtmi.SceneBuilder(7)
        b.sphere([0, 0, 0], 1.0, b.lambertian([0.5, 0.5, 0.5]))
        b.sky()
        b.camera_pinhole([0, 1, 6], [0, 0, 0], [0, 1, 0], math.pi / 4, W / H)
        self.b = b.commit()
        self.R = rtmi.Renderer(self.b, H, W, 1, DEPTH, post=False).init_rng()
        self.items = self.R.items
        self.dev = self.R.device
        self.camera = self.b.camera_get()
        self.history_bytes = int(rtmi.lib().rtmi_history_bytes(H, W))
        a = self.rays()
        self.step = self.b.bounce(a["origins"], a["directions"], self.states(N), hits=True, steps=self.ints(N, fill=0))

    def floats(self, *shape, fill=F32_SENTINEL):
        return torch.full(shape, fill, dtype=torch.float32, device=self.dev)

    def ints(self, *shape, fill=INT_SENTINEL, dtype=torch.int32):
        return torch.full(shape, fill, dtype=dtype, device=self.dev)

    def rays(self, n=N):
        o = torch.tensor([[0.0, 1.0, 6.0]], device=self.dev).repeat(n, 1)
        d = torch.tensor([[0.0, -0.15, -1.0]], device=self.dev) + 0.02 * torch.arange(n, device=self.dev, dtype=torch.float32)[:, None]
        return {"origins": o, "directions": d}

    def states(self, n):
        return rtmi.rng_states(11, n, device=self.dev)

    def paths(self, n, prefix="paths"):
        return {prefix + ".index": torch.arange(n, dtype=torch.int32, device=self.dev), prefix + ".count": self.ints(1, fill=n)}


@pytest.fixture(scope="module")
def env():
    return Env()


def paths_of(a, prefix="paths"):
    return rtmi.Paths(a[prefix + ".index"], a[prefix + ".count"])


# ---------------------------------------------------------------- the entries: (their good tensors, the call on them)
def query_args(e, out):
    return dict(e.rays(), t_max=e.floats(N, fill=100.0), out=out)


def bounce_args(e):
    return dict(e.rays(), states=e.states(N), emitted=e.floats(N, 3), attenuation=e.floats(N, 3), hits=e.ints(N, 12), steps=e.ints(N))


def direct_args(e, mis):
    a = dict(e.paths(N, "result.paths"), light_states=e.states(N), flags=e.ints(N, fill=0), counts=e.ints(2, dtype=torch.int64))
    a.update({"result.origins": e.step.origins, "result.directions": e.step.directions, "out.origins": e.floats(N, 3),
              "out.directions": e.floats(N, 3), "out.t_max": e.floats(N), "out.direct": e.floats(N, 3)})
    if mis:
        a["carry"] = e.floats(N, 4)
    return a


def direct_call(e, a):
    s = e.step
    r = rtmi.Bounce(a["result.origins"], a["result.directions"], s.states, s.emitted, s.attenuation, s.hits, s.steps, s.work,
                    paths_of(a, "result.paths"))
    e.b.direct_sample(0, r, a["light_states"], a["flags"], out=(a["out.origins"], a["out.directions"], a["out.t_max"], a["out.direct"]),
                      counts=a["counts"], mis="carry" in a, carry=a.get("carry"))


def fold_args(e, direct):
    a = dict(directions=e.rays()["directions"], steps=e.ints(N, fill=1), emitted_stack=e.floats(LAYERS, N, 3),
             attenuation_stack=e.floats(LAYERS, N, 3))
    if direct:
        a.update(direct_stack=e.floats(LAYERS, N, 3), occluded_stack=e.ints(LAYERS, N, fill=0, dtype=torch.uint8))
    return dict(a, out=e.floats(N, 3))


def filter_args(e):
    return dict(color=e.floats(H, W, 3), variance=e.floats(H, W, 3), normal=e.floats(H, W, 3), depth=e.floats(H, W), alpha=e.floats(H, W))


def advance_args(e):
    n = e.items
    a = dict(e.paths(n), origins=e.floats(n, 3), directions=e.floats(n, 3), steps=e.ints(n, fill=0), emitted=e.floats(n, 3),
             attenuation=e.floats(n, 3), cursor=e.ints(n, 2, fill=0), budget=e.ints(n, fill=1), counts=e.ints(3, dtype=torch.int64))
    a.update({"stacks[0]": e.floats(DEPTH, n, 3), "stacks[1]": e.floats(DEPTH, n, 3)})
    return a


ENTRIES = {
    "intersect": (lambda e: query_args(e, e.ints(N, 12)),
                  lambda e, a: e.b.intersect(a["origins"], a["directions"], a["t_max"], out=a["out"])),
    "occluded": (lambda e: query_args(e, e.ints(N, dtype=torch.uint8)),
                 lambda e, a: e.b.occluded(a["origins"], a["directions"], a["t_max"], out=a["out"])),
    "occluded_list": (lambda e: dict(query_args(e, e.ints(N, dtype=torch.uint8)), **e.paths(N)),
                      lambda e, a: e.b.occluded_list(paths_of(a), a["origins"], a["directions"], a["t_max"], out=a["out"])),
    "trace": (lambda e: dict(e.rays(), states=e.states(N), out=e.floats(N, 3)),
              lambda e, a: e.b.trace(a["origins"], a["directions"], a["states"], DEPTH, out=a["out"])),
    "bounce": (bounce_args,
               lambda e, a: e.b.bounce(a["origins"], a["directions"], a["states"], a["emitted"], a["attenuation"], a["hits"], a["steps"])),
    "bounce_list": (lambda e: dict(bounce_args(e), **e.paths(N)),
                    lambda e, a: e.b.bounce_list(paths_of(a), a["origins"], a["directions"], a["states"], a["emitted"],
                                                 a["attenuation"], a["hits"], a["steps"])),
    "direct_sample": (lambda e: direct_args(e, False), direct_call),
    "direct_sample_mis": (lambda e: direct_args(e, True), direct_call),
    "path_fold": (lambda e: fold_args(e, False),
                  lambda e, a: rtmi.path_fold(a["directions"], a["steps"], a["emitted_stack"], a["attenuation_stack"], out=a["out"])),
    "path_fold_direct": (lambda e: fold_args(e, True),
                         lambda e, a: rtmi.path_fold_direct(a["directions"], a["steps"], a["emitted_stack"], a["attenuation_stack"],
                                                            a["direct_stack"], a["occluded_stack"], out=a["out"])),
    "path_compact": (lambda e: dict(e.rays(), **e.paths(N), **e.paths(N, "out")),
                     lambda e, a: rtmi.path_compact(a["origins"], a["directions"], paths_of(a), out=paths_of(a, "out"))),
    "denoise": (lambda e: dict(filter_args(e), albedo=e.floats(H, W, 3), out=e.floats(H, W, 3)),
                lambda e, a: rtmi.denoise(**a)),
    "accumulate": (lambda e: dict(filter_args(e), history=e.ints(e.history_bytes, fill=0, dtype=torch.uint8),
                                  out_history=e.ints(e.history_bytes, dtype=torch.uint8)),
                   lambda e, a: rtmi.accumulate(camera=e.camera, prev_camera=e.camera, **a)),
    "camera_rays": (lambda e: {"budget": e.ints(e.items, fill=1), "out[0]": e.floats(e.items, 3), "out[1]": e.floats(e.items, 3)},
                    lambda e, a: e.R.camera_rays(0, a["budget"], out=(a["out[0]"], a["out[1]"]))),
    "sample_add": (lambda e: dict(radiance=e.floats(e.items, 3), trace_counts=e.ints(e.items), budget=e.ints(e.items, fill=1)),
                   lambda e, a: e.R.sample_add(0, a["radiance"], a["trace_counts"], a["budget"])),
    "render_budget": (lambda e: dict(budget=e.ints(e.items, fill=1)),
                      lambda e, a: e.R.render_budget(a["budget"])),
    "path_advance": (advance_args,
                     lambda e, a: e.R.path_advance(paths_of(a), a["origins"], a["directions"], a["steps"], a["emitted"], a["attenuation"],
                                                   (a["stacks[0]"], a["stacks[1]"]), a["cursor"], a["budget"], counts=a["counts"])),
}


def corrupt(t, kind):
    if kind == "dtype":
        return t.to(torch.float64 if t.dtype.is_floating_point else torch.int16)
    if kind == "shape":
        return t.unsqueeze(-1)
    if kind == "length":
        return torch.cat([t, t[:1]])
    if kind == "strided":
        return torch.stack([t, t], dim=-1)[..., 0]
    return t.cpu()


def kinds_of(arg):
    return [k for k in KINDS if not (k == "strided" and arg.endswith(".count"))]


def refusal(e, entry, arg, kind):
    """The text the entry refuses the corrupted argument with (None: it accepted it), after checking nothing was written."""
    make, call = ENTRIES[entry]
    a = make(e)
    bad = corrupt(a[arg], kind)
    assert kind != "strided" or not bad.is_contiguous()
    R = e.R
    watch = [t for k, t in a.items() if k != arg] + [bad, R.states] + [t for t in (getattr(R, "sum", None), getattr(R, "sq", None),
                                                                                getattr(R, "samples", None)) if t is not None]
    before = [t.clone() for t in watch]
    try:
        call(e, dict(a, **{arg: bad}))
    except rtmi.RtmiError as err:
        torch.cuda.synchronize()
        for t, t0 in zip(watch, before):
            assert torch.equal(t, t0), "%s refused %s (%s) after writing to a tensor" % (entry, arg, kind)
        return str(err)
    torch.cuda.synchronize()
    return None


# {entry: {argument: the text for every kind, or {kind: text}}}; None: accepted
REGULARISED = "REGULARISED"
EXPECT = {
    'intersect': {
        'origins': {
            'dtype': 'origins must be float32, not torch.float64',
            'shape': 'origins must have shape (N, 3), not (5, 3, 1)',
            'length': 'origins and directions differ in length',
            'strided': None,
            'cpu': "origins is on the CPU: rtmi_intersect has no CPU path (move it to the scene's GPU)",
        },
        'directions': {
            'dtype': 'directions must be float32, not torch.float64',
            'shape': 'directions must have shape (N, 3), not (5, 3, 1)',
            'length': 'origins and directions differ in length',
            'strided': None,
            'cpu': "directions is on the CPU: rtmi_intersect has no CPU path (move it to the scene's GPU)",
        },
        't_max': {
            'dtype': "t_max must be a CUDA float32 tensor of shape (N,) on the rays' device",
            'shape': "t_max must be a CUDA float32 tensor of shape (N,) on the rays' device",
            'length': "t_max must be a CUDA float32 tensor of shape (N,) on the rays' device",
            'strided': None,
            'cpu': "t_max must be a CUDA float32 tensor of shape (N,) on the rays' device",
        },
        'out': "out must be a contiguous CUDA int32 tensor of shape (N, 12) on the rays' device",
    },
    'occluded': {
        'origins': {
            'dtype': 'origins must be float32, not torch.float64',
            'shape': 'origins must have shape (N, 3), not (5, 3, 1)',
            'length': 'origins and directions differ in length',
            'strided': None,
            'cpu': "origins is on the CPU: rtmi_occluded has no CPU path (move it to the scene's GPU)",
        },
        'directions': {
            'dtype': 'directions must be float32, not torch.float64',
            'shape': 'directions must have shape (N, 3), not (5, 3, 1)',
            'length': 'origins and directions differ in length',
            'strided': None,
            'cpu': "directions is on the CPU: rtmi_occluded has no CPU path (move it to the scene's GPU)",
        },
        't_max': {
            'dtype': "t_max must be a CUDA float32 tensor of shape (N,) on the rays' device",
            'shape': "t_max must be a CUDA float32 tensor of shape (N,) on the rays' device",
            'length': "t_max must be a CUDA float32 tensor of shape (N,) on the rays' device",
            'strided': None,
            'cpu': "t_max must be a CUDA float32 tensor of shape (N,) on the rays' device",
        },
        'out': "out must be a contiguous CUDA uint8 or bool tensor of shape (N,) on the rays' device",
    },
    'occluded_list': {
        'origins': {
            'dtype': 'origins must be float32, not torch.float64',
            'shape': 'origins must have shape (N, 3), not (5, 3, 1)',
            'length': 'origins and directions differ in length',
            'strided': None,
            'cpu': "origins is on the CPU: rtmi_occluded_list has no CPU path (move it to the scene's GPU)",
        },
        'directions': {
            'dtype': 'directions must be float32, not torch.float64',
            'shape': 'directions must have shape (N, 3), not (5, 3, 1)',
            'length': 'origins and directions differ in length',
            'strided': None,
            'cpu': "directions is on the CPU: rtmi_occluded_list has no CPU path (move it to the scene's GPU)",
        },
        't_max': {
            'dtype': "t_max must be a CUDA float32 tensor of shape (N,) on the rays' device",
            'shape': "t_max must be a CUDA float32 tensor of shape (N,) on the rays' device",
            'length': "t_max must be a CUDA float32 tensor of shape (N,) on the rays' device",
            'strided': None,
            'cpu': "t_max must be a CUDA float32 tensor of shape (N,) on the rays' device",
        },
        'out': "out must be a contiguous CUDA uint8 or bool tensor of shape (N,) on the rays' device",
        'paths.index': {
            'dtype': "paths.index must be a contiguous CUDA int32 tensor of shape (capacity,) on the rays' device",
            'shape': "paths.index must be a contiguous CUDA int32 tensor of shape (capacity,) on the rays' device",
            'length': None,
            'strided': "paths.index must be a contiguous CUDA int32 tensor of shape (capacity,) on the rays' device",
            'cpu': "paths.index must be a contiguous CUDA int32 tensor of shape (capacity,) on the rays' device",
        },
        'paths.count': ("paths.count must be a contiguous CUDA int32 tensor of shape (1,) on the rays' device", REGULARISED),
    },
    'trace': {
        'origins': {
            'dtype': 'origins must be float32, not torch.float64',
            'shape': 'origins must have shape (N, 3), not (5, 3, 1)',
            'length': 'origins and directions differ in length',
            'strided': None,
            'cpu': "origins is on the CPU: rtmi_trace has no CPU path (move it to the scene's GPU)",
        },
        'directions': {
            'dtype': 'directions must be float32, not torch.float64',
            'shape': 'directions must have shape (N, 3), not (5, 3, 1)',
            'length': 'origins and directions differ in length',
            'strided': None,
            'cpu': "directions is on the CPU: rtmi_trace has no CPU path (move it to the scene's GPU)",
        },
        'states': "states must be a contiguous CUDA int32 tensor of shape (6, N) on the rays' device",
        'out': "out must be a contiguous CUDA float32 tensor of shape (N, 3) on the rays' device",
    },
    'bounce': {
        'origins': {
            'dtype': 'origins must be float32, not torch.float64',
            'shape': 'origins must have shape (N, 3), not (5, 3, 1)',
            'length': 'origins and directions differ in length',
            'strided': 'origins and directions must be contiguous: rtmi_bounce writes the scattered rays into them',
            'cpu': "origins is on the CPU: rtmi_bounce has no CPU path (move it to the scene's GPU)",
        },
        'directions': {
            'dtype': 'directions must be float32, not torch.float64',
            'shape': 'directions must have shape (N, 3), not (5, 3, 1)',
            'length': 'origins and directions differ in length',
            'strided': 'origins and directions must be contiguous: rtmi_bounce writes the scattered rays into them',
            'cpu': "directions is on the CPU: rtmi_bounce has no CPU path (move it to the scene's GPU)",
        },
        'states': "states must be a contiguous CUDA int32 tensor of shape (6, N) on the rays' device",
        'emitted': "emitted must be a contiguous CUDA float32 tensor of shape (N, 3) on the rays' device",
        'attenuation': "attenuation must be a contiguous CUDA float32 tensor of shape (N, 3) on the rays' device",
        'hits': "out must be a contiguous CUDA int32 tensor of shape (N, 12) on the rays' device",
        'steps': "steps must be a contiguous CUDA int32 tensor of shape (N,) on the rays' device",
    },
    'bounce_list': {
        'origins': {
            'dtype': 'origins must be float32, not torch.float64',
            'shape': 'origins must have shape (N, 3), not (5, 3, 1)',
            'length': 'origins and directions differ in length',
            'strided': 'origins and directions must be contiguous: rtmi_bounce writes the scattered rays into them',
            'cpu': "origins is on the CPU: rtmi_bounce_list has no CPU path (move it to the scene's GPU)",
        },
        'directions': {
            'dtype': 'directions must be float32, not torch.float64',
            'shape': 'directions must have shape (N, 3), not (5, 3, 1)',
            'length': 'origins and directions differ in length',
            'strided': 'origins and directions must be contiguous: rtmi_bounce writes the scattered rays into them',
            'cpu': "directions is on the CPU: rtmi_bounce_list has no CPU path (move it to the scene's GPU)",
        },
        'states': "states must be a contiguous CUDA int32 tensor of shape (6, N) on the rays' device",
        'emitted': "emitted must be a contiguous CUDA float32 tensor of shape (N, 3) on the rays' device",
        'attenuation': "attenuation must be a contiguous CUDA float32 tensor of shape (N, 3) on the rays' device",
        'hits': "out must be a contiguous CUDA int32 tensor of shape (N, 12) on the rays' device",
        'steps': "steps must be a contiguous CUDA int32 tensor of shape (N,) on the rays' device",
        'paths.index': {
            'dtype': "paths.index must be a contiguous CUDA int32 tensor of shape (capacity,) on the rays' device",
            'shape': "paths.index must be a contiguous CUDA int32 tensor of shape (capacity,) on the rays' device",
            'length': None,
            'strided': "paths.index must be a contiguous CUDA int32 tensor of shape (capacity,) on the rays' device",
            'cpu': "paths.index must be a contiguous CUDA int32 tensor of shape (capacity,) on the rays' device",
        },
        'paths.count': ("paths.count must be a contiguous CUDA int32 tensor of shape (1,) on the rays' device", REGULARISED),
    },
    'direct_sample': {
        'result.paths.index': {
            'dtype': "paths.index must be a contiguous CUDA int32 tensor of shape (capacity,) on the rays' device",
            'shape': "paths.index must be a contiguous CUDA int32 tensor of shape (capacity,) on the rays' device",
            'length': None,
            'strided': "paths.index must be a contiguous CUDA int32 tensor of shape (capacity,) on the rays' device",
            'cpu': "paths.index must be a contiguous CUDA int32 tensor of shape (capacity,) on the rays' device",
        },
        'result.paths.count': ("paths.count must be a contiguous CUDA int32 tensor of shape (1,) on the rays' device", REGULARISED),
        'light_states': "light_states must be a contiguous CUDA int32 tensor of shape (6, N) on the rays' device",
        'flags': "flags must be a contiguous CUDA int32 tensor of shape (N,) on the rays' device",
        'counts': ("counts must be a contiguous CUDA int64 tensor of shape (2,) on the rays' device", REGULARISED),
        'result.origins': {
            'dtype': 'origins must be float32, not torch.float64',
            'shape': 'origins must have shape (N, 3), not (5, 3, 1)',
            'length': 'origins and directions differ in length',
            'strided': None,
            'cpu': "origins is on the CPU: rtmi_direct_sample has no CPU path (move it to the scene's GPU)",
        },
        'result.directions': {
            'dtype': 'directions must be float32, not torch.float64',
            'shape': 'directions must have shape (N, 3), not (5, 3, 1)',
            'length': 'origins and directions differ in length',
            'strided': None,
            'cpu': "directions is on the CPU: rtmi_direct_sample has no CPU path (move it to the scene's GPU)",
        },
        'out.origins': "out's origins must be a contiguous CUDA float32 tensor of shape (5, 3) on the rays' device",
        'out.directions': "out's directions must be a contiguous CUDA float32 tensor of shape (5, 3) on the rays' device",
        'out.t_max': "out's t_max must be a contiguous CUDA float32 tensor of shape (5,) on the rays' device",
        'out.direct': "out's direct must be a contiguous CUDA float32 tensor of shape (5, 3) on the rays' device",
    },
    'direct_sample_mis': {
        'result.paths.index': {
            'dtype': "paths.index must be a contiguous CUDA int32 tensor of shape (capacity,) on the rays' device",
            'shape': "paths.index must be a contiguous CUDA int32 tensor of shape (capacity,) on the rays' device",
            'length': None,
            'strided': "paths.index must be a contiguous CUDA int32 tensor of shape (capacity,) on the rays' device",
            'cpu': "paths.index must be a contiguous CUDA int32 tensor of shape (capacity,) on the rays' device",
        },
        'result.paths.count': ("paths.count must be a contiguous CUDA int32 tensor of shape (1,) on the rays' device", REGULARISED),
        'light_states': "light_states must be a contiguous CUDA int32 tensor of shape (6, N) on the rays' device",
        'flags': "flags must be a contiguous CUDA int32 tensor of shape (N,) on the rays' device",
        'counts': ("counts must be a contiguous CUDA int64 tensor of shape (2,) on the rays' device", REGULARISED),
        'result.origins': {
            'dtype': 'origins must be float32, not torch.float64',
            'shape': 'origins must have shape (N, 3), not (5, 3, 1)',
            'length': 'origins and directions differ in length',
            'strided': None,
            'cpu': "origins is on the CPU: rtmi_direct_sample has no CPU path (move it to the scene's GPU)",
        },
        'result.directions': {
            'dtype': 'directions must be float32, not torch.float64',
            'shape': 'directions must have shape (N, 3), not (5, 3, 1)',
            'length': 'origins and directions differ in length',
            'strided': None,
            'cpu': "directions is on the CPU: rtmi_direct_sample has no CPU path (move it to the scene's GPU)",
        },
        'out.origins': "out's origins must be a contiguous CUDA float32 tensor of shape (5, 3) on the rays' device",
        'out.directions': "out's directions must be a contiguous CUDA float32 tensor of shape (5, 3) on the rays' device",
        'out.t_max': "out's t_max must be a contiguous CUDA float32 tensor of shape (5,) on the rays' device",
        'out.direct': "out's direct must be a contiguous CUDA float32 tensor of shape (5, 3) on the rays' device",
        'carry': "carry must be a contiguous CUDA float32 tensor of shape (N, 4) on the rays' device",
    },
    'path_fold': {
        'directions': {
            'dtype': 'directions must be a contiguous CUDA float32 tensor of shape (N, 3): rtmi_path_fold has no CPU path',
            'shape': 'directions must be a contiguous CUDA float32 tensor of shape (N, 3): rtmi_path_fold has no CPU path',
            'length': "steps must be a contiguous CUDA int32 tensor of shape (N,) on the directions' device",
            'strided': 'directions must be a contiguous CUDA float32 tensor of shape (N, 3): rtmi_path_fold has no CPU path',
            'cpu': 'directions must be a contiguous CUDA float32 tensor of shape (N, 3): rtmi_path_fold has no CPU path',
        },
        'steps': "steps must be a contiguous CUDA int32 tensor of shape (N,) on the directions' device",
        'emitted_stack': {
            'dtype': "emitted_stack must be a contiguous CUDA float32 tensor of shape (layers, N, 3) on the directions' device",
            'shape': 'emitted_stack must have shape (layers, N, 3) with 1 <= layers <= 64',
            'length': "attenuation_stack must be a contiguous CUDA float32 tensor of shape (layers, N, 3) on the directions' device",
            'strided': "emitted_stack must be a contiguous CUDA float32 tensor of shape (layers, N, 3) on the directions' device",
            'cpu': "emitted_stack must be a contiguous CUDA float32 tensor of shape (layers, N, 3) on the directions' device",
        },
        'attenuation_stack': "attenuation_stack must be a contiguous CUDA float32 tensor of shape (layers, N, 3) on the directions' device",
        'out': "out must be a contiguous CUDA float32 tensor of shape (N, 3) on the rays' device",
    },
    'path_fold_direct': {
        'directions': {
            'dtype': 'directions must be a contiguous CUDA float32 tensor of shape (N, 3): rtmi_path_fold_direct has no CPU path',
            'shape': 'directions must be a contiguous CUDA float32 tensor of shape (N, 3): rtmi_path_fold_direct has no CPU path',
            'length': "steps must be a contiguous CUDA int32 tensor of shape (N,) on the directions' device",
            'strided': 'directions must be a contiguous CUDA float32 tensor of shape (N, 3): rtmi_path_fold_direct has no CPU path',
            'cpu': 'directions must be a contiguous CUDA float32 tensor of shape (N, 3): rtmi_path_fold_direct has no CPU path',
        },
        'steps': "steps must be a contiguous CUDA int32 tensor of shape (N,) on the directions' device",
        'emitted_stack': {
            'dtype': "emitted_stack must be a contiguous CUDA float32 tensor of shape (layers, N, 3) on the directions' device",
            'shape': 'emitted_stack must have shape (layers, N, 3) with 1 <= layers <= 64',
            'length': "attenuation_stack must be a contiguous CUDA float32 tensor of shape (layers, N, 3) on the directions' device",
            'strided': "emitted_stack must be a contiguous CUDA float32 tensor of shape (layers, N, 3) on the directions' device",
            'cpu': "emitted_stack must be a contiguous CUDA float32 tensor of shape (layers, N, 3) on the directions' device",
        },
        'attenuation_stack': "attenuation_stack must be a contiguous CUDA float32 tensor of shape (layers, N, 3) on the directions' device",
        'direct_stack': "direct_stack must be a contiguous CUDA float32 tensor of shape (layers, N, 3) on the directions' device",
        'occluded_stack': "occluded_stack must be a contiguous CUDA uint8 or bool tensor of shape (layers, N) on the directions' device",
        'out': "out must be a contiguous CUDA float32 tensor of shape (N, 3) on the rays' device",
    },
    'path_compact': {
        'origins': {
            'dtype': 'origins must be float32, not torch.float64',
            'shape': 'origins must have shape (N, 3), not (5, 3, 1)',
            'length': 'origins and directions differ in length',
            'strided': None,
            'cpu': "origins is on the CPU: rtmi_path_compact has no CPU path (move it to the scene's GPU)",
        },
        'directions': {
            'dtype': 'directions must be float32, not torch.float64',
            'shape': 'directions must have shape (N, 3), not (5, 3, 1)',
            'length': 'origins and directions differ in length',
            'strided': None,
            'cpu': "directions is on the CPU: rtmi_path_compact has no CPU path (move it to the scene's GPU)",
        },
        'paths.index': {
            'dtype': "paths.index must be a contiguous CUDA int32 tensor of shape (capacity,) on the rays' device",
            'shape': "paths.index must be a contiguous CUDA int32 tensor of shape (capacity,) on the rays' device",
            'length': 'out must be an rtmi.Paths with a count tensor and room for every candidate (6)',
            'strided': "paths.index must be a contiguous CUDA int32 tensor of shape (capacity,) on the rays' device",
            'cpu': "paths.index must be a contiguous CUDA int32 tensor of shape (capacity,) on the rays' device",
        },
        'paths.count': ("paths.count must be a contiguous CUDA int32 tensor of shape (1,) on the rays' device", REGULARISED),
        'out.index': {
            'dtype': "out.index must be a contiguous CUDA int32 tensor of shape (capacity,) on the rays' device",
            'shape': "out.index must be a contiguous CUDA int32 tensor of shape (capacity,) on the rays' device",
            'length': None,
            'strided': "out.index must be a contiguous CUDA int32 tensor of shape (capacity,) on the rays' device",
            'cpu': "out.index must be a contiguous CUDA int32 tensor of shape (capacity,) on the rays' device",
        },
        'out.count': ("out.count must be a contiguous CUDA int32 tensor of shape (1,) on the rays' device", REGULARISED),
    },
    'denoise': {
        'color': {
            'dtype': "color must be a contiguous CUDA float32 tensor of shape (8, 8, 3) on color's device",
            'shape': 'color must be a CUDA float32 tensor of shape (H, W, 3): rtmi_denoise has no CPU path',
            'length': "variance must be a contiguous CUDA float32 tensor of shape (9, 8, 3) on color's device",
            'strided': "color must be a contiguous CUDA float32 tensor of shape (8, 8, 3) on color's device",
            'cpu': 'color must be a CUDA float32 tensor of shape (H, W, 3): rtmi_denoise has no CPU path',
        },
        'variance': "variance must be a contiguous CUDA float32 tensor of shape (8, 8, 3) on color's device",
        'normal': "normal must be a contiguous CUDA float32 tensor of shape (8, 8, 3) on color's device",
        'depth': "depth must be a contiguous CUDA float32 tensor of shape (8, 8) on color's device",
        'alpha': "alpha must be a contiguous CUDA float32 tensor of shape (8, 8) on color's device",
        'albedo': "albedo must be a contiguous CUDA float32 tensor of shape (8, 8, 3) on color's device",
        'out': "out must be a contiguous CUDA float32 tensor of shape (H, W, 3) on color's device",
    },
    'accumulate': {
        'color': {
            'dtype': "color must be a contiguous CUDA float32 tensor of shape (8, 8, 3) on color's device",
            'shape': 'color must be a CUDA float32 tensor of shape (H, W, 3): rtmi_accumulate has no CPU path',
            'length': "variance must be a contiguous CUDA float32 tensor of shape (9, 8, 3) on color's device",
            'strided': "color must be a contiguous CUDA float32 tensor of shape (8, 8, 3) on color's device",
            'cpu': 'color must be a CUDA float32 tensor of shape (H, W, 3): rtmi_accumulate has no CPU path',
        },
        'variance': "variance must be a contiguous CUDA float32 tensor of shape (8, 8, 3) on color's device",
        'normal': "normal must be a contiguous CUDA float32 tensor of shape (8, 8, 3) on color's device",
        'depth': "depth must be a contiguous CUDA float32 tensor of shape (8, 8) on color's device",
        'alpha': "alpha must be a contiguous CUDA float32 tensor of shape (8, 8) on color's device",
        'history': "history must be a contiguous CUDA uint8 tensor of rtmi_history_bytes(H, W) = 3072 bytes on color's device",
        'out_history': "out_history must be a contiguous CUDA uint8 tensor of rtmi_history_bytes(H, W) = 3072 bytes on color's device",
    },
    'camera_rays': {
        'budget': "budget must be a contiguous CUDA int32 tensor of shape (items,) on the renderer's device",
        'out[0]': "out must be a contiguous CUDA float32 tensor of shape (items, 3) on the rays' device",
        'out[1]': "out must be a contiguous CUDA float32 tensor of shape (items, 3) on the rays' device",
    },
    'sample_add': {
        'radiance': "radiance must be a contiguous CUDA float32 tensor of shape (items, 3) on the renderer's device",
        'trace_counts': "trace_counts must be a contiguous CUDA int32 tensor of shape (items,) on the renderer's device",
        'budget': "budget must be a contiguous CUDA int32 tensor of shape (items,) on the renderer's device",
    },
    'render_budget': {
        'budget': "budget must be a contiguous CUDA int32 tensor of shape (items,) on the renderer's device",
    },
    'path_advance': {
        'paths.index': {
            'dtype': "paths.index must be a contiguous CUDA int32 tensor of shape (capacity,) on the rays' device",
            'shape': "paths.index must be a contiguous CUDA int32 tensor of shape (capacity,) on the rays' device",
            'length': None,
            'strided': "paths.index must be a contiguous CUDA int32 tensor of shape (capacity,) on the rays' device",
            'cpu': "paths.index must be a contiguous CUDA int32 tensor of shape (capacity,) on the rays' device",
        },
        'paths.count': ("paths.count must be a contiguous CUDA int32 tensor of shape (1,) on the rays' device", REGULARISED),
        'origins': "origins must be a contiguous CUDA float32 tensor of shape (items, 3) on the renderer's device",
        'directions': "directions must be a contiguous CUDA float32 tensor of shape (items, 3) on the renderer's device",
        'steps': "steps must be a contiguous CUDA int32 tensor of shape (items,) on the renderer's device",
        'emitted': "emitted must be a contiguous CUDA float32 tensor of shape (items, 3) on the renderer's device",
        'attenuation': "attenuation must be a contiguous CUDA float32 tensor of shape (items, 3) on the renderer's device",
        'cursor': "cursor must be a contiguous CUDA int32 tensor of shape (items, 2) on the renderer's device",
        'budget': "budget must be a contiguous CUDA int32 tensor of shape (items,) on the renderer's device",
        'counts': ("counts must be a contiguous CUDA int64 tensor of shape (3,) on the renderer's device", REGULARISED),
        'stacks[0]': ("stacks[0] must be a contiguous CUDA float32 tensor of shape (max_depth, items, 3) on the renderer's device", REGULARISED),
        'stacks[1]': ("stacks[1] must be a contiguous CUDA float32 tensor of shape (max_depth, items, 3) on the renderer's device", REGULARISED),
    },
}


def expected(entry, arg, kind):
    want = EXPECT[entry][arg]
    if isinstance(want, tuple):  # (text, REGULARISED)
        want = want[0]
    return want[kind] if isinstance(want, dict) else want


@pytest.mark.parametrize("entry", sorted(ENTRIES))
def test_every_refusal_word_for_word(env, entry):
    make, _ = ENTRIES[entry]
    assert set(make(env)) == set(EXPECT[entry]), "EXPECT does not hold this entry's tensor arguments"
    for arg in EXPECT[entry]:
        for kind in kinds_of(arg):
            got = refusal(env, entry, arg, kind)
            print("%s %s %s: %r" % (entry, arg, kind, got))
            assert got == expected(entry, arg, kind), (arg, kind)


def test_the_good_calls_are_accepted(env):
    """The table's own inputs are right: uncorrupted, every entry runs."""
    for entry, (make, call) in ENTRIES.items():
        call(env, make(env))
    torch.cuda.synchronize()
