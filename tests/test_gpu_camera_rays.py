"""rtmi_camera_rays / rtmi_sample_add on the device: the rays against the oracle's RayAt and a numpy restatement, bit for
bit; the three-call loop camera_rays -> trace -> sample_add (Renderer.render_rays) against rtmi_render and
rtmi_render_budget, bit for bit; the `each` hook against rtmi_render_features; the other projections against numpy.

The oracle's x, y are formed as tests/test_gpu_features.py::sample_features forms them; glm_normalize is
tests/test_gpu_trace.py's."""
import ctypes as C
import math

import numpy as np
import pytest

import common
import oraclelib
import rtmi
from parity import bits
from querylib import glm_normalize

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

F32 = np.float32
NAN_BITS = 0x7FC00123  # what the outputs hold before a call: a written word shows
FRAMES = [(20, 28), (16, 16), (24, 32)]  # ragged tiles on both edges; the power-of-two jitter form; whole tiles
SHARDS = [(0, 1), (0, 3), (2, 3)]        # (rank, world_size)
U32P = C.POINTER(C.c_uint32)


# ------------------------------------------------------------------ scenes
def build_pair(camera):
    """(committed product scene, oracle builder) of the world a camera case names."""
    name = {"pinhole": "cornell_box", "defocus": "mixed", "raw": "sky_only"}[camera]
    seed = common.scene_seed(name)
    out = []
    for b in (rtmi.SceneBuilder(seed), oraclelib.OracleBuilder(seed)):
        common.build_scene(b, name, 1.0)
        if camera == "defocus":
            b.camera_defocus([0.5, 1.5, 6], [0, 0.8, 0], [0, 1, 0], math.pi / 4, 1.25, 0.3, 5.5)
        elif camera == "raw":
            b.camera_raw([0.25, -0.5, 3], [-1.5, -1.25, 1], [3, 0.125, 0.25], [-0.25, 2.5, 0.5])
        out.append(b)
    return out[0].commit(), out[1]


def renderer(b, h, w, spp, depth=10, rank=0, world=1, seed=None):
    return rtmi.Renderer(b, h, w, spp, depth, post=False, rank=rank, world_size=world).init_rng(seed)


def host_states(R):
    return np.ascontiguousarray(R.states.cpu().numpy().view(np.uint32).T)  # (items, 6)


def nan_filled(R):
    make = lambda: torch.full((R.items, 3), NAN_BITS, dtype=torch.int32, device=R.device).view(torch.float32)
    return make(), make()


def jitter(st, h, w, idx):
    """(r1, r2 drawn from st in place, then xf, yf as ray_tracing.cu:68-73 rounds them, and the oracle's x, y)."""
    L = oraclelib.lib()
    p = st.ctypes.data_as(U32P)
    r1 = float(L.orc_random_float(C.c_float(0.0), C.c_float(1.0), p))
    r2 = float(L.orc_random_float(C.c_float(0.0), C.c_float(1.0), p))
    i, j = divmod(int(idx), w)
    x = (r1 + float(j)) / float(w)
    y = (r2 + float(h - i)) / float(h)
    x, y = 2 * x - 1, 2 * y - 1
    return F32((x + 1) / 2), F32((y + 1) / 2), x, y


def active_mask(R, budget, sample):
    pix = rtmi.pixel_map(R.frame) >= 0
    if budget is None:
        return pix & (sample < R.frame.spp)
    return pix & (sample < np.minimum(np.asarray(budget, dtype=np.int64), R.frame.spp))


def check_camera_samples(R, ob, cam, samples, budget=None):
    """Samples 0..samples-1 of rtmi_camera_rays on R's states, each against the oracle and the numpy restatement."""
    h, w = R.frame.height, R.frame.width
    pixel_of = rtmi.pixel_map(R.frame)
    pos, llc, horiz, vert = (cam[k].astype(F32) for k in range(4))
    d_budget = None if budget is None else torch.from_numpy(np.asarray(budget, dtype=np.int32)).to(R.device)
    st = host_states(R)
    seen_active = seen_idle = 0
    for sample in range(samples):
        out = nan_filled(R)
        O, D = (t.cpu().numpy() for t in R.camera_rays(sample, budget=d_budget, out=out))
        got = host_states(R)
        act = active_mask(R, budget, sample)
        idle = ~act
        seen_active, seen_idle = seen_active + int(act.sum()), seen_idle + int(idle.sum())
        assert not bits(O[idle]).any() and not bits(D[idle]).any(), "an inactive item holds six +0.0f"
        assert np.array_equal(got[idle], st[idle]), "an inactive item's state is untouched"
        for q in np.flatnonzero(act):
            s = st[q].copy()
            xf, yf, x, y = jitter(s, h, w, pixel_of[q])
            ray = ob.probe_camera_ray(x, y, s)  # (a defocus camera draws its lens offsets from s)
            where = (sample, int(q))
            assert np.array_equal(bits(O[q]), bits(ray[:3])), where
            assert np.array_equal(bits(glm_normalize(D[q])), bits(ray[3:])), where
            target = ((llc + xf * horiz) + yf * vert).astype(F32)
            assert np.array_equal(bits(D[q]), bits(glm_normalize(target - O[q]))), where
            assert np.array_equal(got[q], s), where
            st[q] = s
    return seen_active, seen_idle


# ------------------------------------------------------------------ 1. against the oracle, kind CAMERA
@pytest.mark.parametrize("hw", FRAMES, ids=lambda hw: "%dx%d" % hw)
@pytest.mark.parametrize("camera", ["pinhole", "defocus", "raw"])
def test_camera_rays_match_the_oracle(camera, hw):
    b, ob = build_pair(camera)
    cam = b.camera_get()
    assert np.array_equal(bits(cam[:4]), bits(ob.camera_get()[:4]))  # (position, llc, horizontal, vertical: what RayAt reads)
    for rank, world in SHARDS:
        R = renderer(b, hw[0], hw[1], 3, rank=rank, world=world)
        n_active, n_idle = check_camera_samples(R, ob, cam, 3)
        assert n_active == 3 * int((rtmi.pixel_map(R.frame) >= 0).sum()) > 0
        if hw == (20, 28):
            assert n_idle > 0, "the ragged frame has padding items"


def test_defocus_camera_makes_four_draws():
    b, ob = build_pair("defocus")
    R = renderer(b, 16, 16, 1)
    before = host_states(R)
    R.camera_rays(0)
    after = host_states(R)
    L = oraclelib.lib()
    for q in range(R.items):
        s = before[q].copy()
        for _ in range(4):
            L.orc_random_float(C.c_float(0.0), C.c_float(1.0), s.ctypes.data_as(U32P))
        assert np.array_equal(after[q], s)


# ------------------------------------------------------------------ 2. the budget mask
@pytest.mark.parametrize("camera", ["pinhole", "defocus"])
def test_budget_masks_items_at_or_past_their_capped_budget(camera):
    b, ob = build_pair(camera)
    R = renderer(b, 20, 28, 3, rank=1, world=2)
    budget = np.random.default_rng(5).integers(0, 5, R.items)  # 0..4 against spp = 3: the cap is exercised
    n_active, n_idle = check_camera_samples(R, ob, b.camera_get(), 4, budget=budget)  # (sample 3: nobody is active)
    pix = rtmi.pixel_map(R.frame) >= 0
    assert n_active == int(np.minimum(budget, 3)[pix].sum())
    assert (budget[pix] == 0).any() and (budget[pix] == 4).any()


# ------------------------------------------------------------------ 3. composition equals the render
@pytest.mark.parametrize("rank,world", [(0, 1), (1, 2)])
@pytest.mark.parametrize("name,hw,spp,depth", [("mixed", (20, 28), 4, 10), ("cornell_box", (16, 16), 2, 50),
                                               ("bunny", (24, 32), 2, 10)])
def test_render_rays_equal_the_render(name, hw, spp, depth, rank, world):
    seed = common.scene_seed(name)
    b = common.build_scene(rtmi.SceneBuilder(seed), name, hw[1] / hw[0]).commit()
    A = renderer(b, hw[0], hw[1], spp, depth, rank, world)
    A.render()
    A.check()
    total = A.total_rays()
    B = renderer(b, hw[0], hw[1], spp, depth, rank, world)
    B.render_rays()
    B.check()
    torch.cuda.synchronize()
    pix = rtmi.pixel_map(A.frame) >= 0
    assert np.array_equal(bits(B.sum.cpu().numpy()), bits(A.tiles.cpu().numpy()))
    assert np.array_equal(B.budget_rays.cpu().numpy(), A.ray_counts.cpu().numpy())
    assert np.array_equal(host_states(B), host_states(A))
    assert int(B.rays_total.item()) == total == int(A.ray_counts.cpu().numpy().astype(np.int64).sum())
    assert np.array_equal(B.samples.cpu().numpy(), np.where(pix, spp, 0))


# ------------------------------------------------------------------ 4. composition equals the budget render
def test_render_rays_equal_the_budget_render_over_two_passes():
    seed = common.scene_seed("mixed")
    b = common.build_scene(rtmi.SceneBuilder(seed), "mixed", 28 / 20).commit()
    A, B = renderer(b, 20, 28, 3, 10), renderer(b, 20, 28, 3, 10)
    rng = np.random.default_rng(11)
    for n_pass in range(2):
        budget = rng.integers(0, 5, A.items)  # 0..4 against the cap 3
        budget[rng.random(A.items) < 0.2] = 0
        d_budget = torch.from_numpy(budget.astype(np.int32)).to(A.device)
        A.render_budget(d_budget)
        B.render_rays(budget=d_budget)
        A.check(), B.check()
        torch.cuda.synchronize()
        for what in ("sum", "sq"):
            assert np.array_equal(bits(getattr(A, what).cpu().numpy()), bits(getattr(B, what).cpu().numpy())), (n_pass, what)
        for what in ("samples", "budget_rays"):
            assert np.array_equal(getattr(A, what).cpu().numpy(), getattr(B, what).cpu().numpy()), (n_pass, what)
        assert np.array_equal(host_states(A), host_states(B)), n_pass
    assert int(A.samples.sum().item()) > 0 and float(A.sq.sum().item()) > 0


# ------------------------------------------------------------------ 5. the hook sees the frame's own rays
def test_hook_rays_give_the_features_of_the_frame():
    seed = common.scene_seed("mixed")
    b = common.build_scene(rtmi.SceneBuilder(seed), "mixed", 28 / 20).commit()
    A, B = renderer(b, 20, 28, 1, 10), renderer(b, 20, 28, 1, 10)
    A.render_budget(torch.ones((A.items,), dtype=torch.int32, device=A.device), features=True)
    seen = {}

    def each(sample, origins, directions):
        seen[sample] = b.intersect(origins, directions)

    B.render_rays(each=each)
    A.check(), B.check()
    assert sorted(seen) == [0]
    hits = seen[0].check()
    kind = hits.kind.cpu().numpy()
    surface = (kind != rtmi.RTMI_HIT_NONE) & (kind != rtmi.RTMI_HIT_SKY)
    assert surface.any() and (kind == rtmi.RTMI_HIT_SKY).any()
    assert np.array_equal(A.coverage.cpu().numpy(), surface.astype(np.int32))
    t = np.where(surface, hits.t.cpu().numpy(), F32(0))
    assert np.array_equal(bits(A.depth.cpu().numpy()), bits(t))
    n = np.where(surface[:, None], hits.normal.cpu().numpy(), F32(0)) + F32(0)  # (the sum starts at +0: a -0 becomes +0)
    assert np.array_equal(bits(A.normal.cpu().numpy()), bits(n.astype(F32)))
    assert np.array_equal(bits(A.sum.cpu().numpy()), bits(B.sum.cpu().numpy()))


# ------------------------------------------------------------------ 6. the other projections
def two_draws(st, h, w, pixel_of, act):
    """Per active item: xf, yf (float32 arrays over all items) and the states after the two draws."""
    xf, yf, out = np.zeros(len(st), F32), np.zeros(len(st), F32), st.copy()
    for q in np.flatnonzero(act):
        xf[q], yf[q], _, _ = jitter(out[q], h, w, pixel_of[q])
    return xf, yf, out


def projection_case(kind, fov, hw, rank, world):
    b, _ = build_pair("pinhole")
    R = renderer(b, hw[0], hw[1], 2, rank=rank, world=world)
    cam = b.camera_get()
    st = host_states(R)
    pixel_of = rtmi.pixel_map(R.frame)
    out = nan_filled(R)
    O, D = (t.cpu().numpy() for t in R.camera_rays(0, projection=rtmi.projection(kind, fov), out=out))
    act = active_mask(R, None, 0)
    xf, yf, want_st = two_draws(st, hw[0], hw[1], pixel_of, act)
    assert np.array_equal(host_states(R), want_st), "two draws per active item, none for padding"
    assert not bits(O[~act]).any() and not bits(D[~act]).any()
    return cam, O[act], D[act], xf[act], yf[act]


@pytest.mark.parametrize("hw,rank,world", [((20, 28), 0, 1), ((16, 16), 0, 1), ((24, 32), 1, 2)])
def test_orthographic_rays_bit_for_bit(hw, rank, world):
    cam, O, D, xf, yf = projection_case("orthographic", 0.0, hw, rank, world)
    llc, horiz, vert, w = cam[1], cam[2], cam[3], cam[6]
    want_o = ((llc[None, :] + xf[:, None] * horiz[None, :]).astype(F32) + yf[:, None] * vert[None, :]).astype(F32)
    assert np.array_equal(bits(O), bits(want_o))
    want_d = np.tile(glm_normalize(-w), (len(O), 1))
    assert np.array_equal(bits(D), bits(want_d))


def curved_directions(kind, fov, cam, xf, yf):
    """The binary64 restatement of EQUIRECT / FISHEYE, rounded once to binary32 and normalised once; and r > 1."""
    u, v, w = (cam[k].astype(np.float64) for k in (4, 5, 6))
    x, y = xf.astype(np.float64), yf.astype(np.float64)
    outside = np.zeros(len(x), dtype=bool)
    if kind == "equirect":
        phi, theta = (x - 0.5) * (2 * np.pi), (y - 0.5) * np.pi
        cu, cv, cw = np.cos(theta) * np.sin(phi), np.sin(theta), np.cos(theta) * np.cos(phi)
    else:
        sx, sy = 2 * x - 1, 2 * y - 1
        r = np.sqrt(sx * sx + sy * sy)
        outside = r > 1
        rr = np.where(r == 0, 1.0, r)
        t = r * np.float64(F32(fov)) / 2
        cu, cv, cw = np.sin(t) * (sx / rr), np.sin(t) * (sy / rr), np.cos(t)
    Dd = (cu[:, None] * u[None, :] + cv[:, None] * v[None, :]) - cw[:, None] * w[None, :]
    want = glm_normalize(Dd.astype(F32))
    want[outside] = 0
    return want, outside


@pytest.mark.parametrize("hw,rank,world", [((20, 28), 0, 1), ((16, 16), 0, 1), ((24, 32), 1, 2)])
@pytest.mark.parametrize("kind,fov", [("equirect", 0.0), ("fisheye", math.pi), ("fisheye", 2 * math.pi)])
def test_equirect_and_fisheye_rays_within_the_derived_bound(kind, fov, hw, rank, world):
    """Bound 2^-22 absolute per component: binary64 sin / cos of the device and of numpy agree to a few binary64 ulps
    (about 1e-16); rounding a component of magnitude at most 1 to binary32 moves it by at most 2^-25; the one binary32
    normalisation adds at most three roundings of 2^-24 relative.  2^-22 is about four times that sum."""
    cam, O, D, xf, yf = projection_case(kind, fov, hw, rank, world)
    assert np.array_equal(bits(O), bits(np.tile(cam[0], (len(O), 1)))), "origin = position"
    want, outside = curved_directions(kind, fov, cam, xf, yf)
    assert not bits(D[outside]).any(), "outside the image circle: three +0.0f"
    err = np.abs(D.astype(np.float64) - want.astype(np.float64))
    print("%s fov %.3f %dx%d: max |error| = %.3e (bound %.3e), %d of %d outside" %
          (kind, fov, hw[0], hw[1], err.max(), 2.0 ** -22, int(outside.sum()), len(D)))
    assert (err <= 2.0 ** -22).all()
    inside = ~outside
    assert np.abs(np.linalg.norm(D[inside].astype(np.float64), axis=1) - 1).max() < 1e-6
    if kind == "fisheye":
        assert outside.any() and inside.any()


def test_fisheye_surround_counts_as_a_black_sample():
    seed = common.scene_seed("mixed")
    b = common.build_scene(rtmi.SceneBuilder(seed), "mixed", 28 / 20).commit()
    R = renderer(b, 20, 28, 1, 10)
    kept = {}

    def each(sample, origins, directions):
        kept[sample] = directions.clone()

    R.render_rays(projection=rtmi.projection("fisheye", math.pi), each=each)
    R.check()
    pix = rtmi.pixel_map(R.frame) >= 0
    zero = ~bits(kept[0].cpu().numpy()).any(axis=1)
    assert (zero & pix).any() and (~zero & pix).any()
    assert np.array_equal(R.samples.cpu().numpy(), pix.astype(np.int32)), "a pixel outside the circle has its sample"
    assert not bits(R.sum.cpu().numpy()[zero]).any(), "... of radiance 0"
    assert np.array_equal(R.budget_rays.cpu().numpy()[zero], np.zeros(int(zero.sum()), np.int32))
    assert float(R.sum.cpu().numpy()[~zero].sum()) > 0


def test_equirect_frame_through_the_rest_of_the_pipeline():
    h, w, spp, depth = 16, 24, 2, 10
    b = common.build_scene(rtmi.SceneBuilder(1024), "sky_only", w / h).commit()
    R = renderer(b, h, w, spp, depth)
    kept = []

    def each(sample, origins, directions):
        kept.append((origins.clone(), directions.clone()))

    R.render_rays(projection=rtmi.projection("equirect"), each=each)
    R.check()
    tiles, var = R.resolve(post=False), R.resolve_variance()
    img, _ = R.untile(tiles)
    vimg, _ = R.untile(var)
    assert len(kept) == spp
    assert torch.isfinite(img).all() and torch.isfinite(vimg).all() and float(img.min()) > 0
    # each pixel: the mean of the Sky colour of its two directions, as rtmi_trace answers them
    total = np.zeros((R.items, 3), F32)
    for o, d in kept:
        tr = b.trace(o, d, rtmi.rng_states(1, R.items), depth).check()
        total = (total + tr.rgb.cpu().numpy()).astype(F32)
    want = (total / F32(spp)).astype(F32)
    assert np.array_equal(bits(tiles.cpu().numpy()), bits(want))
    pixel_of = rtmi.pixel_map(R.frame)
    assert np.array_equal(bits(img.cpu().numpy().reshape(-1, 3)[pixel_of]), bits(want))
    assert len(np.unique(bits(want), axis=0)) > h  # a panorama of the sky's gradient, not one colour


# ------------------------------------------------------------------ 7. independence
def test_two_streams_and_a_camera_update_between_calls():
    b, _ = build_pair("pinhole")
    alone = []
    for seed in (3, 4):
        R = renderer(b, 20, 28, 2, seed=seed)
        o, d = R.camera_rays(0)
        alone.append((o.cpu().numpy(), d.cpu().numpy(), host_states(R)))
    pair = [renderer(b, 20, 28, 2, seed=seed) for seed in (3, 4)]
    torch.cuda.synchronize()
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    got = []
    for R, s in zip(pair, streams):
        with torch.cuda.stream(s):
            got.append(R.camera_rays(0))
    torch.cuda.synchronize()
    for (o, d), R, ref in zip(got, pair, alone):
        assert np.array_equal(bits(o.cpu().numpy()), bits(ref[0])) and np.array_equal(bits(d.cpu().numpy()), bits(ref[1]))
        assert np.array_equal(host_states(R), ref[2])
    assert not np.array_equal(alone[0][1], alone[1][1])
    # a call enqueued before a camera update keeps the old camera; one after it has the new
    before, after = renderer(b, 20, 28, 2, seed=3), renderer(b, 20, 28, 2, seed=3)
    torch.cuda.synchronize()
    with torch.cuda.stream(streams[0]):
        old = before.camera_rays(0)
        b.camera_look([200, 300, -700], [278, 278, 0], [0, 1, 0], 0.6, 28 / 20)
        new = after.camera_rays(0)
    torch.cuda.synchronize()
    assert np.array_equal(bits(old[0].cpu().numpy()), bits(alone[0][0])) and np.array_equal(bits(old[1].cpu().numpy()), bits(alone[0][1]))
    moved = renderer(b, 20, 28, 2, seed=3)
    ref = [t.cpu().numpy() for t in moved.camera_rays(0)]
    assert np.array_equal(bits(new[0].cpu().numpy()), bits(ref[0])) and np.array_equal(bits(new[1].cpu().numpy()), bits(ref[1]))
    pix = rtmi.pixel_map(before.frame) >= 0
    assert np.array_equal(bits(ref[0][pix]), bits(np.tile(F32([200, 300, -700]), (int(pix.sum()), 1))))
    assert not np.array_equal(ref[1], alone[0][1])


# ------------------------------------------------------------------ the binding's own argument checks
def test_binding_refuses_bad_buffers_before_any_gpu_work():
    b, _ = build_pair("pinhole")
    R = renderer(b, 20, 28, 2)
    before = host_states(R)
    good = torch.zeros((R.items, 3), dtype=torch.float32, device=R.device)
    for kw in (dict(budget=torch.zeros((R.items,), dtype=torch.int64, device=R.device)),
               dict(budget=torch.zeros((R.items - 1,), dtype=torch.int32, device=R.device)),
               dict(budget=torch.zeros((R.items,), dtype=torch.int32)),
               dict(out=(good, good[:-1])), dict(out=(good.double(), good)), dict(out=good),
               dict(projection=(2, 0.0))):
        with pytest.raises(rtmi.RtmiError):
            R.camera_rays(0, **kw)
    with pytest.raises(rtmi.RtmiError, match="radiance"):
        R.sample_add(0, good[:-1])
    with pytest.raises(rtmi.RtmiError, match="trace_counts"):
        R.sample_add(0, good, trace_counts=torch.zeros((R.items,), dtype=torch.float32, device=R.device))
    with pytest.raises(rtmi.RtmiError, match="post=False"):
        rtmi.Renderer(b, 20, 28, 2, 10, post=True).init_rng().render_rays()
    with pytest.raises(rtmi.RtmiError, match="orthonormal"):
        raw, _ = build_pair("raw")
        renderer(raw, 16, 16, 1).camera_rays(0, projection=rtmi.projection("equirect"))
    assert np.array_equal(host_states(R), before), "a refused call leaves the states alone"
    # out= is written in place and handed back
    o, d = R.camera_rays(0, out=(good, torch.ones_like(good)))
    assert o is good and float(d.abs().sum()) > 0
