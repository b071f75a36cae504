"""The numpy rules of rtmi_denoise and rtmi_accumulate against binary64 truth (tests/filters_truth.py states what is
checked and where every tolerance comes from).  tests/test_gpu_filters_truth.py runs the same checks on the library.  No
GPU involved."""
import numpy as np
import pytest

import common
import filters_truth as T
import filter_rules
import oraclelib
from filter_rules import accumulate_rule

F32 = np.float32
ids = lambda s: "%dx%d" % s


# ------------------------------------------------------------------ denoise
@pytest.mark.parametrize("demodulate", [0, 1])
@pytest.mark.parametrize("iterations", T.DENOISE_ITERATIONS)
@pytest.mark.parametrize("squarings", T.DENOISE_SQUARINGS)
@pytest.mark.parametrize("shape", T.DENOISE_SHAPES, ids=ids)
def test_denoise_rule_against_binary64(shape, squarings, iterations, demodulate):
    T.check_denoise_truth(T.rule_denoise, shape, squarings, iterations, demodulate)


def test_the_threshold_is_what_keeps_the_rule_finite(monkeypatch):
    """The same check on the rule as it was, sw > 0: with 6 squarings a pass divides by the square of a subnormal sum and
    the variance is infinite or NaN out of finite inputs.  (The smallest subnormal as the threshold is sw > 0.)"""
    monkeypatch.setattr(filter_rules, "MIN_WEIGHT_SUM", np.nextafter(F32(0), F32(1)))
    with pytest.raises(AssertionError, match="not finite"):
        T.check_denoise_truth(T.rule_denoise, (33, 70), 6, 1, 0)


def test_the_threshold_decides_some_pixels_and_never_with_default_options():
    """With squarings the threshold is at work (some pass keeps a pixel); with none it never is, so the default options'
    frames keep the bits they had: the centre tap alone weighs (9/64) |n|^2, far above 2^-32 for synthetic's normals (>= 1/2)."""
    assert T.check_denoise_truth(T.rule_denoise, (33, 70), 8, 5, 1) > 0
    d = T.synthetic(33, 70)
    decisions = []
    T.rule_denoise(d, 1, iterations=8, decisions=decisions)
    surf = d["alpha"] > 0
    assert all(ok[surf].all() for ok in decisions)


@pytest.mark.parametrize("iterations", T.DENOISE_ITERATIONS)
@pytest.mark.parametrize("squarings", [0, 6])
def test_denoise_rule_returns_a_constant_colour(squarings, iterations):
    kept = T.check_constant_colour(T.rule_denoise, squarings, iterations)
    assert (kept > 0) == (squarings > 0)


# ------------------------------------------------------------------ accumulate
@pytest.mark.parametrize("move", T.LANDING_MOVES)
@pytest.mark.parametrize("shape", T.LANDING_SHAPES, ids=ids)
def test_accumulate_rule_lands_where_binary64_does(shape, move):
    T.check_landing(T.rule_chain, shape, move)


@pytest.mark.parametrize("move", T.LANDING_MOVES)
@pytest.mark.parametrize("shape", T.LANDING_SHAPES, ids=ids)
def test_accumulate_rule_depth_gate_agrees_with_binary64(shape, move):
    T.check_depth_gate(T.rule_chain, shape, move)


def test_the_landing_check_sees_half_a_pixel():
    """The check is worth its name: a rule whose pixel centre is half a pixel off in y (the previous camera's image plane
    moved by v' / (2 H)) fails it."""
    h, w = 33, 70

    def shifted(frames):
        (d0, cam0, o0), (d1, cam1, o1) = frames
        hist = accumulate_rule(**d0, camera=cam0, **o0)[3]
        off = cam0.copy()
        off[3:6] += off[9:12] / F32(2 * h)
        return accumulate_rule(**d1, camera=cam1, history=hist, prev_camera=off, **o1)[:3]

    with pytest.raises(AssertionError):
        T.check_landing(shifted, (h, w), "slide")


def test_the_rule_reads_the_frame_as_the_oracle_renders_it():
    """tests/test_gpu_filters_truth.py's convention check with the oracle as the renderer: the Cornell box from its home
    camera at 64 x 64, 64 jittered samples per pixel through the oracle's camera exactly as its render draws them
    (x = (r1 + j) / W, y = (r2 + H - i) / H, the draws numpy's here), first hits by its closest-hit probe.  The oracle is what
    rtmi_render_features is held to bit for bit, so this ties the rule's pixel centre and its reading of `depth` to the
    renderer without a GPU.  Measured ratios: DESIGN.md 2.9."""
    h = w = 64
    spp = 64
    b = common.build_scene(oraclelib.OracleBuilder(common.scene_seed("cornell_box")), "cornell_box", 1.0)
    rng = np.random.default_rng(0)
    depth, normal, hits = np.zeros((h, w)), np.zeros((h, w, 3)), np.zeros((h, w))
    for i in range(h):
        for j in range(w):
            for r1, r2 in rng.random((spp, 2)):
                ray = b.probe_camera_ray(2 * (r1 + j) / w - 1, 2 * (r2 + (h - i)) / h - 1)
                hit, rec, mat = b.probe_hit(ray[:3], ray[3:])
                if hit and mat >= 0:
                    depth[i, j] += rec[0]
                    normal[i, j] += rec[3:6]
                    hits[i, j] += 1

    def closest_hit(origins, directions):
        t = np.full(h * w, np.inf)
        for k, (o, d) in enumerate(zip(origins.reshape(-1, 3), directions.reshape(-1, 3))):
            hit, rec, mat = b.probe_hit(o, d)
            if hit and mat >= 0:
                t[k] = rec[0]
        return t

    T.check_convention(depth / np.maximum(hits, 1), normal / spp, hits / spp, b.camera_get(), closest_hit)
