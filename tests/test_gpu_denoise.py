"""rtmi_denoise / rtmi_resolve_variance / Renderer.denoise on the GPU, bit for bit against the numpy restatements of
tests/filter_rules.py (``denoise_rule``, ``variance_rule``), and the one thing no restatement can say: that the
filter lowers the error of a low-sample frame.

The exactness inputs are synthetic (``synthetic``): patches of a few surface orientations and depths with noise on both,
so that the normal, depth and colour weights all take values strictly between 0 and 1 somewhere, patches of background,
variances of which a fifth are exactly 0, and albedos with exact zeros.  Shapes are the smallest at which tiling, halos
and borders can go wrong: one pixel; one tile row or column narrower than the stencil; a frame that is ragged against the
32 x 8 tile in both directions with several tiles; and 16 x 16, where the fifth pass (step 16) has every off-centre tap
outside the image.  Passes 1-2 run the LDS-staged kernel, 3-5 the global one, and the last pass of every call the
remodulating one: 1, 3 and 5 iterations put each of the four instantiations in the last position or before it.  Passes 6-8
run on frames 300 pixels long, the extreme extents 1 x 65535 and 65535 x 1 on their own, and tests/test_gpu_filters_truth.py
holds the same calls to binary64."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import common
import rtmi
from filters_truth import same_or_nan, synthetic
from abi_host import CHECK_LIB, ROOT, _frame
from filter_rules import denoise_rule, on_gpu, run, variance_rule
from parity import bits, same

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

F32 = np.float32
GUIDES = ("variance", "normal", "depth", "alpha", "albedo")
SHAPES = [(1, 1), (3, 70), (70, 3), (33, 70), (16, 16)]


def want(d, demodulate, **opts):
    d = dict(d)
    if not demodulate:
        d.pop("albedo")
    return denoise_rule(**d, **opts)


def assert_exact(got, expected, what):
    for name, g, w_ in zip(("out", "out_variance"), got, expected):
        bad = bits(g) != bits(w_)
        assert not bad.any(), "%s: %s differs in %d of %d floats, first at %s: %r != %r" % (
            what, name, bad.sum(), bad.size, np.argwhere(bad)[0], g[bad][0], w_[bad][0])


# ------------------------------------------------------------------ 1. bit-exact against the restatement
@pytest.mark.parametrize("demodulate", [0, 1])
@pytest.mark.parametrize("iterations", [1, 3, 5])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "%dx%d" % s)
def test_denoise_equals_the_rule(shape, iterations, demodulate):
    d = synthetic(*shape)
    got = run(d, demodulate, iterations=iterations)
    exp = want(d, demodulate, iterations=iterations)
    assert_exact(got, exp, "%dx%d k=%d demodulate=%d" % (shape + (iterations, demodulate)))
    if shape == (33, 70) and iterations == 5:
        # the case is worth its name: the filter changed most pixels, and every weight was somewhere in between
        assert (bits(got[0]) != bits(d["color"])).mean() > 0.5


# ------------------------------------------------------------------ 1b. the far passes, the extreme extents, non-finite inputs
@pytest.mark.parametrize("demodulate", [0, 1])
@pytest.mark.parametrize("iterations", [6, 7, 8])
@pytest.mark.parametrize("shape", [(9, 300), (300, 9)], ids=lambda s: "%dx%d" % s)
def test_denoise_far_passes_equal_the_rule(shape, iterations, demodulate):
    """Steps 32, 64 and 128: their taps at +-2 steps (64, 128, 256 pixels away) land inside a frame 300 pixels long."""
    d = synthetic(*shape)
    assert_exact(run(d, demodulate, iterations=iterations), want(d, demodulate, iterations=iterations),
                 "%dx%d k=%d demodulate=%d" % (shape + (iterations, demodulate)))


@pytest.mark.parametrize("iterations", [1, 3])
@pytest.mark.parametrize("shape", [(1, 65535), (65535, 1)], ids=lambda s: "%dx%d" % s)
def test_denoise_extreme_extents_equal_the_rule(shape, iterations):
    """The largest extent either way (2048 tile columns, 8192 tile rows): one staged pass alone, and two before a global one."""
    d = synthetic(*shape)
    assert_exact(run(d, 1, iterations=iterations), want(d, 1, iterations=iterations), "%dx%d k=%d" % (shape + (iterations,)))


@pytest.mark.parametrize("what", ["nan_color", "inf_depth"])
def test_denoise_non_finite_input_stays_in_its_footprint(what):
    """One NaN colour, or one infinite depth, in a 33 x 70 frame under 3 iterations (reach 2 (1 + 2 + 4) = 14 pixels): the
    call does not fault, equals the rule (a NaN for a NaN), and every pixel further than 14 pixels (Chebyshev) from it
    has the bits of the clean run."""
    h, w, at = 33, 70, (16, 36)
    clean = synthetic(h, w, seed=6)
    assert clean["alpha"][at] > 0
    d = {k: v.copy() for k, v in clean.items()}
    if what == "nan_color":
        d["color"][at][1] = np.nan
    else:
        d["depth"][at] = np.inf
    got, exp, ref = run(d, 1, iterations=3), want(d, 1, iterations=3), run(clean, 1, iterations=3)
    I, J = np.meshgrid(np.arange(h), np.arange(w), indexing="ij")
    far = np.maximum(np.abs(I - at[0]), np.abs(J - at[1])) > 14
    assert far.any() and not far.all()
    for name, g, e, r in zip(("out", "out_variance"), got, exp, ref):
        assert same_or_nan(g, e).all(), (what, name, np.argwhere(~same_or_nan(g, e))[0])
        assert (bits(g)[far] == bits(r)[far]).all(), (what, name)
    assert not (bits(got[0])[~far] == bits(ref[0])[~far]).all()  # (and it was seen inside)


def test_denoise_in_place_and_without_the_variance():
    """d_out == d_color, with and without d_out_variance: the same bits as out of place."""
    d = synthetic(33, 70, seed=1)
    exp = want(d, 1)
    t = on_gpu(d)
    color = t["color"]
    out = rtmi.denoise(**t, out=color)
    assert out is color
    torch.cuda.synchronize()
    assert same(color.cpu().numpy(), exp[0])
    t = on_gpu(d)
    out, var = rtmi.denoise(**t, out=t["color"], return_variance=True)
    torch.cuda.synchronize()
    assert_exact((out.cpu().numpy(), var.cpu().numpy()), exp, "in place")
    for k in GUIDES:  # (the guides are inputs only)
        assert same(t[k].cpu().numpy(), d[k]), k


@pytest.mark.parametrize("squarings", [0, 8])
def test_denoise_normal_squarings_at_both_ends(squarings):
    d = synthetic(33, 70, seed=2)
    opts = dict(iterations=3, normal_squarings=squarings, sigma_color=2.5, sigma_depth=0.1)
    got = run(d, 1, **opts)
    assert_exact(got, want(d, 1, **opts), "squarings %d" % squarings)
    assert np.isfinite(got[0]).all() and np.isfinite(got[1]).all()  # (8 squarings: sums of weights down to 0 and below 2^-32)


# ------------------------------------------------------------------ 2. edges are hard
def _halves(kind, h=24, w=40):
    d = synthetic(h, w, seed=3)
    left = np.arange(w) < w // 2
    d["alpha"][:] = 1
    d["normal"][:] = np.array([0, 0, 1], F32)
    d["depth"][:] = 1.0
    if kind == "normal":
        d["normal"][:, ~left] = np.array([1, 0, 0], F32)  # orthogonal: the dot product is exactly 0
    elif kind == "alpha":
        d["alpha"][:, ~left] = 0
    else:
        d["depth"][:, ~left] = 2.0  # seen from the left: |1 - 2| / (0.05 * 1 + 1e-6) = 20 >= 4
    return d, left


@pytest.mark.parametrize("kind", ["normal", "alpha", "depth"])
def test_nothing_crosses_a_hard_edge(kind):
    """Two half-images that an edge separates: whatever the right half's colours and variances are, the left half's output
    is the same bits.  Each frame is filtered twice, with bit-equal outputs."""
    d, left = _halves(kind)
    other = {k: v.copy() for k, v in d.items()}
    rng = np.random.default_rng(11)
    other["color"][:, ~left] = (rng.random(other["color"][:, ~left].shape) * 40).astype(F32)
    other["variance"][:, ~left] = (rng.random(other["variance"][:, ~left].shape) * 9).astype(F32)
    a, a2, b, b2 = run(d, 1), run(d, 1), run(other, 1), run(other, 1)
    assert_exact(a2, a, "the same frame twice")
    assert_exact(b2, b, "the other frame twice")
    assert_exact(a, want(d, 1), kind)
    for x, y in zip(a, b):
        assert same(x[:, left], y[:, left]), kind
        assert not same(x[:, ~left], y[:, ~left])
    # and the left half was filtered, not left alone
    assert (bits(a[0][:, left]) != bits(d["color"][:, left])).mean() > 0.5


# ------------------------------------------------------------------ 3. the variance of the mean
@pytest.mark.parametrize("world", [1, 3])
def test_resolve_variance_equals_the_rule(world):
    L = rtmi.lib()
    rng = np.random.default_rng(world)
    seen = set()
    for rank in range(world):
        f = _frame(rank=rank, world=world)  # 20 x 28: ragged against the 8 x 8 tile, so shards carry padding items
        items = rtmi.work_items(f)
        pm = rtmi.pixel_map(f)
        n = rng.integers(0, 40, items).astype(np.uint32)
        n[::7], n[1::7], n[2::7] = 0, 1, 2
        S = (rng.random((items, 3)) * 30).astype(F32)
        Q = (S * S / np.maximum(n, 1)[:, None] * rng.uniform(0.98, 1.5, (items, 3))).astype(F32)  # (some a - b < 0)
        t = [torch.from_numpy(x).cuda() for x in (S, Q, n.view(np.int32))]
        var = torch.full((items, 3), -1.0, dtype=torch.float32, device="cuda")
        rc = L.rtmi_resolve_variance(C.byref(f), *(C.c_void_p(x.data_ptr()) for x in t), C.c_void_p(var.data_ptr()),
                                     C.c_void_p(torch.cuda.current_stream().cuda_stream))
        assert rc == 0, L.rtmi_last_error()
        torch.cuda.synchronize()
        exp = variance_rule(n, S, Q, pixel=pm >= 0)
        assert same(var.cpu().numpy(), exp)
        live = pm >= 0
        seen |= {int(x) for x in n[live] if x < 3} | ({"padding"} if (~live).any() else set())
        with np.errstate(all="ignore"):
            seen |= {"clamped"} if ((n[:, None] >= 2) & live[:, None] & (n[:, None].astype(F32) * Q - S * S < 0)).any() else set()
    assert seen >= {0, 1, 2, "clamped", "padding"}, seen


# ------------------------------------------------------------------ 4. end to end
def rendered(name, spp, cap=16, depth=10, size=64):
    b = common.build_scene(rtmi.SceneBuilder(common.scene_seed(name)), name, 1.0).commit()
    R = rtmi.Renderer(b, size, size, cap, depth, post=False).init_rng()
    R.render_budget(torch.full((R.items,), spp, dtype=torch.int32, device="cuda"), features=True)
    return R


@pytest.mark.parametrize("name", ["cornell_box", "bunny"])
def test_renderer_denoise_equals_the_rule_on_its_untiled_buffers(name):
    R = rendered(name, 8)
    R.check()
    kept = ("sum", "sq", "samples", "states", "albedo", "normal", "depth", "coverage", "budget_rays")
    before = {k: getattr(R, k).clone() for k in kept}
    img = R.denoise(post=False)
    buf = R.denoise_inputs()
    torch.cuda.synchronize()
    assert img.shape == (64, 64, 3)
    d = {k: v.cpu().numpy() for k, v in buf.items()}
    # the buffers are what the tile-major resolves say, pixel by pixel
    pm = rtmi.pixel_map(R.frame)
    live = pm >= 0
    n = R.samples.cpu().numpy().view(np.uint32)
    var = variance_rule(n, R.sum.cpu().numpy(), R.sq.cpu().numpy(), pixel=live)
    assert same(R.resolve_variance().cpu().numpy(), var)
    assert same(d["variance"].reshape(-1, 3)[pm[live]], var[live])
    assert same(d["color"].reshape(-1, 3)[pm[live]], R.resolve(post=False).cpu().numpy()[live])
    assert (d["alpha"] > 0).any() and d["variance"].max() > 0
    exp, _ = denoise_rule(**d)
    assert_exact((img.cpu().numpy(),), (exp,), name)
    assert not same(exp, d["color"])
    # post: the render's own post-processing of the same image
    post = R.denoise(post=True)
    torch.cuda.synchronize()
    assert same(post.cpu().numpy(), np.sqrt(np.clip(exp, F32(0), F32(1)), dtype=F32))
    for k in kept:
        assert torch.equal(getattr(R, k), before[k]), k


# ------------------------------------------------------------------ 5. it denoises
_REF = {}


def reference(name):
    """The library's own render at 4096 spp with another seed, not post-processed (once per scene)."""
    if name not in _REF:
        total = common.gpu_render(name, 64, 64, 4096, 10, post=False, seed=common.scene_seed(name) + 977)[0]
        _REF[name] = (total.astype(np.float64) / 4096).astype(F32)  # (without post-processing a render hands out the sums)
    return _REF[name]


def err(x, ref):
    x, ref = x.astype(np.float64), ref.astype(np.float64)
    return float(((x - ref) ** 2 / (ref ** 2 + 0.01)).mean())


@pytest.mark.parametrize("name", ["cornell_box", "bunny"])
def test_it_denoises(name):
    """err(denoised) < err(noisy) at 4 and at 16 samples per pixel with the default options, against a 4096-spp reference:
    a condition, not a tuned number.  Measured on an MI355X (err(denoised) / err(noisy)): see DESIGN.md 2.8."""
    ref = reference(name)
    R = rendered(name, 4)
    for spp, more in ((4, 0), (16, 12)):
        if more:
            R.render_budget(torch.full((R.items,), more, dtype=torch.int32, device="cuda"), features=True)
        noisy = R.untile(R.resolve(post=False), None)[0]
        den = R.denoise(post=False)
        torch.cuda.synchronize()
        assert int(R.samples.max().item()) == spp
        e_noisy, e_den = err(noisy.cpu().numpy(), ref), err(den.cpu().numpy(), ref)
        print("denoise %s %2d spp: err noisy %.6f denoised %.6f ratio %.4f" % (name, spp, e_noisy, e_den, e_den / e_noisy))
        assert e_den < e_noisy, (name, spp, e_den, e_noisy)


# ------------------------------------------------------------------ 6. shares no device state
def test_denoise_runs_beside_a_budget_render():
    d = synthetic(70, 130, seed=4)
    exp = run(d, 1)
    R = rendered("cornell_box", 8)
    R.check()
    serial = {k: getattr(R, k).clone() for k in ("sum", "sq", "samples", "states")}
    t = on_gpu(d)
    R2 = rtmi.Renderer(R.scene, 64, 64, 16, 10, post=False).init_rng()
    budget = torch.full((R2.items,), 8, dtype=torch.int32, device="cuda")
    R2._budget_buffers(), R2._feature_buffers()
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    R2.render_budget(budget, features=True)
    with torch.cuda.stream(side):
        out, var = rtmi.denoise(**t, return_variance=True)
    torch.cuda.synchronize()
    R2.check()
    assert_exact((out.cpu().numpy(), var.cpu().numpy()), exp, "beside a render")
    for k, v in serial.items():
        assert torch.equal(getattr(R2, k), v), k


# ------------------------------------------------------------------ 7. the check build
def check_one_shape():
    d = synthetic(33, 70, seed=5)
    assert_exact(run(d, 1), want(d, 1), "33x70")


def test_check_build_gives_the_same_bits():
    """librtmi_check1.so compiles the denoise kernels too: loaded in a process of its own, it meets the rule on one shape."""
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
