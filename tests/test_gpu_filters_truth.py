"""rtmi_denoise and rtmi_accumulate on the GPU against binary64 truth: the checks of tests/filters_truth.py, which
tests/test_filters_truth_host.py runs on the numpy rules, run on the library; and the one check that needs the renderer:
that the pixel centre and the reading of `depth` the accumulate rule reprojects with are what rtmi_render_features writes."""
import numpy as np
import pytest

import common
import filters_truth as T
import rtmi
from filter_rules import run as device_denoise

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

F32 = np.float32
ids = lambda s: "%dx%d" % s


def device_chain(frames):
    """rtmi.accumulate over a sequence of (inputs, camera, options): the last frame's (out, variance, length) as numpy."""
    hist = prev = got = None
    for d, cam, opts in frames:
        t = {k: torch.from_numpy(np.ascontiguousarray(v)).cuda() for k, v in d.items()}
        *got, hist = rtmi.accumulate(**t, camera=cam, history=hist, prev_camera=prev, **opts)
        prev = cam
    torch.cuda.synchronize()
    return tuple(x.cpu().numpy() for x in got)


# ------------------------------------------------------------------ denoise
@pytest.mark.parametrize("demodulate", [0, 1])
@pytest.mark.parametrize("iterations", T.DENOISE_ITERATIONS)
@pytest.mark.parametrize("squarings", T.DENOISE_SQUARINGS)
@pytest.mark.parametrize("shape", T.DENOISE_SHAPES, ids=ids)
def test_denoise_against_binary64(shape, squarings, iterations, demodulate):
    T.check_denoise_truth(device_denoise, shape, squarings, iterations, demodulate)


@pytest.mark.parametrize("iterations", T.DENOISE_ITERATIONS)
@pytest.mark.parametrize("squarings", [0, 6])
def test_denoise_returns_a_constant_colour(squarings, iterations):
    kept = T.check_constant_colour(device_denoise, squarings, iterations)
    assert (kept > 0) == (squarings > 0)


# ------------------------------------------------------------------ accumulate
@pytest.mark.parametrize("move", T.LANDING_MOVES)
@pytest.mark.parametrize("shape", T.LANDING_SHAPES, ids=ids)
def test_accumulate_lands_where_binary64_does(shape, move):
    T.check_landing(device_chain, shape, move)


@pytest.mark.parametrize("move", T.LANDING_MOVES)
@pytest.mark.parametrize("shape", T.LANDING_SHAPES, ids=ids)
def test_accumulate_depth_gate_agrees_with_binary64(shape, move):
    T.check_depth_gate(device_chain, shape, move)


def test_the_rule_reads_the_frame_as_the_renderer_writes_it():
    """The Cornell box from its home camera, 64 x 64, 64 samples per pixel, max_depth 1, features on: the mean depth of floor,
    ceiling and wall pixels is t along the centre ray of the rule's pixel-centre convention, and of none of the conventions
    half a pixel or a pixel away (T.check_convention).  Measured ratios: DESIGN.md 2.9."""
    b = common.build_scene(rtmi.SceneBuilder(common.scene_seed("cornell_box")), "cornell_box", 1.0).commit()
    R = rtmi.Renderer(b, 64, 64, 64, 1, post=False).init_rng()
    R.render_budget(torch.full((R.items,), 64, dtype=torch.int32, device="cuda"), features=True)
    buf = {k: v.cpu().numpy() for k, v in R.denoise_inputs().items()}
    assert int(R.samples.max().item()) == 64

    def closest_hit(origins, directions):
        o, d = (torch.from_numpy(x.reshape(-1, 3).astype(F32)).cuda() for x in (origins, directions))
        hits = b.intersect(o, d).check()
        kind, t = hits.kind.cpu().numpy(), hits.t.cpu().numpy().astype(np.float64)
        return np.where((kind != rtmi.RTMI_HIT_NONE) & (kind != rtmi.RTMI_HIT_SKY), t, np.inf)

    T.check_convention(buf["depth"], buf["normal"], buf["alpha"], b.camera_get(), closest_hit)
