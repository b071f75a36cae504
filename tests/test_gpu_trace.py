"""rtmi_trace / SceneBuilder.trace against the oracle and against rtmi_render, ray by ray, bit for bit.

The oracle has no Trace-on-a-ray entry, but a raw camera gives one exactly: with position o, lower-left corner o + d
and zero horizontal and vertical spans, RayAt yields Ray(o, normalize(target - o)) for any jitter, target being the
corner as RayAt forms it.  A 1 x S render at one sample per pixel then traces that ray once per pixel state.  Every
sample first draws its two jitter floats, so rtmi_trace gets the oracle's input states advanced by two draws, and the
direction normalize(target - o) (glm's normalize restated in binary32, pinned against probe_camera_ray), which it
normalises once more as Ray's constructor does."""
import ctypes as C

import numpy as np
import pytest

import common
import oraclelib
import rtmi
from abi_host import ERR_DEPTH, ERR_INVALID, OK
from parity import bits
from querylib import CUSTOM_WORLDS, SCENE_WORLDS, build, glm_normalize, make_rays

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

DEPTHS = (0, 1, 8, 50)
F0 = np.float32(0)


def raw_camera(ob, o):
    """Point the oracle's raw camera along ray o (origin, direction); returns the direction RayAt normalised once."""
    org, d = np.asarray(o[0], dtype=np.float32), np.asarray(o[1], dtype=np.float32)
    llc = (org + d).astype(np.float32)
    ob.camera_raw(org, llc, np.zeros(3, np.float32), np.zeros(3, np.float32))
    target = ((llc + F0) + F0).astype(np.float32)  # llc + x * 0 + y * 0: a -0 corner component becomes +0
    return glm_normalize(target - org)


def advance_two(states):
    """The states after the two jitter draws of a sample (orc_random_float(0, 1) twice)."""
    st = np.ascontiguousarray(states, dtype=np.uint32).copy()
    L = oraclelib.lib()
    for row in st:
        p = row.ctypes.data_as(C.POINTER(C.c_uint32))
        L.orc_random_float(C.c_float(0.0), C.c_float(1.0), p)
        L.orc_random_float(C.c_float(0.0), C.c_float(1.0), p)
    return st


def oracle_trace(ob, O, D, states, depth):
    """Per ray i and state s: (radiance (n, S, 3), queries (n, S), final states (n, S, 6), handed directions (n, 3),
    handed states (n, S, 6))."""
    n, S = states.shape[0], states.shape[1]
    rgb = np.zeros((n, S, 3), dtype=np.float32)
    rays = np.zeros((n, S), dtype=np.uint32)
    fin = np.zeros((n, S, 6), dtype=np.uint32)
    dirs = np.zeros((n, 3), dtype=np.float32)
    handed = np.zeros((n, S, 6), dtype=np.uint32)
    for i in range(n):
        dirs[i] = raw_camera(ob, (O[i], D[i]))
        c, r, st, _ = ob.render(1, S, 1, depth, post=False, states=states[i].copy(), threads=1)
        rgb[i], rays[i], fin[i] = c.reshape(S, 3), r.reshape(S), st
        handed[i] = advance_two(states[i])
    return rgb, rays, fin, dirs, handed


def gpu_trace(b, O, D, states, depth, count_rays=True, stream=None):
    """states (N, 6) uint32 -> (rgb (N, 3), rays (N,) or None, final states (N, 6), Trace)."""
    o = torch.from_numpy(np.ascontiguousarray(O, dtype=np.float32)).cuda()
    d = torch.from_numpy(np.ascontiguousarray(D, dtype=np.float32)).cuda()
    st = torch.from_numpy(np.ascontiguousarray(states.T).view(np.int32)).cuda()
    if stream is None:
        tr = b.trace(o, d, st, depth, count_rays=count_rays)
    else:
        with torch.cuda.stream(stream):
            tr = b.trace(o, d, st, depth, count_rays=count_rays)
    tr.check()
    rays = None if tr.rays is None else tr.rays.cpu().numpy().view(np.uint32)
    return tr.rgb.cpu().numpy(), rays, np.ascontiguousarray(st.cpu().numpy().view(np.uint32).T), tr


def usable(O, D):
    """Rays whose raw-camera direction is a finite non-zero vector (o + d may round back onto o)."""
    llc = (O + D).astype(np.float32)
    v = ((llc + F0) + F0).astype(np.float32) - O
    with np.errstate(all="ignore"):
        u = glm_normalize(v)
    return np.isfinite(u).all(1) & (np.abs(u).sum(1) > 0)


# ------------------------------------------------------------------ the bridge itself
def test_raw_camera_restatement_matches_probe_camera_ray():
    """normalize(target - o) restated in numpy, normalised once more by Ray, is what the oracle's RayAt returns."""
    _, _, ob, seed = build("cornell_box")
    O, D = make_rays(ob, 77, n_family=200)
    rng = np.random.default_rng(1)
    for i in rng.choice(len(O), 300, replace=False):
        once = raw_camera(ob, (O[i], D[i]))
        got = ob.probe_camera_ray(rng.random(), rng.random())
        assert np.array_equal(bits(got[:3]), bits(O[i]))
        assert np.array_equal(bits(got[3:]), bits(glm_normalize(once))), i


# ------------------------------------------------------------------ oracle parity
@pytest.mark.parametrize("name", SCENE_WORLDS + sorted(CUSTOM_WORLDS))
def test_trace_matches_the_oracle(name):
    b, rec, ob, seed = build(name)
    O, D = make_rays(ob, 3000 + len(name))
    ok = usable(O, D)
    # half the sample from rays whose first query hits a surface (not Sky), so that every world's paths bounce
    kind = b.intersect(torch.from_numpy(O).cuda(), torch.from_numpy(D).cuda()).check().kind.cpu().numpy()
    solid = np.flatnonzero(ok & (kind != rtmi.RTMI_HIT_NONE) & (kind != rtmi.RTMI_HIT_SKY))
    rest = np.setdiff1d(np.flatnonzero(ok), solid)
    rng = np.random.default_rng(seed + 11)
    pick = rng.choice(solid, min(128, len(solid)), replace=False)
    pick = np.concatenate([pick, rng.choice(rest, min(256 - len(pick), len(rest)), replace=False)])
    O, D = O[pick], D[pick]
    S = 3
    for depth in DEPTHS:
        states = oraclelib.rng_init(seed + depth, len(O) * S, first=12345).reshape(len(O), S, 6)
        o_rgb, o_rays, o_fin, dirs, handed = oracle_trace(ob, O, D, states, depth)
        g_rgb, g_rays, g_fin, tr = gpu_trace(b, np.repeat(O, S, 0), np.repeat(dirs, S, 0), handed.reshape(-1, 6), depth)
        assert int(tr.work[0].item()) == 0
        assert tr.total_rays() == int(o_rays.sum()), (name, depth)
        bad = np.flatnonzero((bits(g_rgb) != bits(o_rgb.reshape(-1, 3))).any(1) | (g_rays != o_rays.reshape(-1)) |
                             (g_fin != o_fin.reshape(-1, 6)).any(1))
        assert bad.size == 0, (name, depth, bad[:8].tolist(), g_rgb[bad[:4]].tolist(), o_rgb.reshape(-1, 3)[bad[:4]].tolist(),
                               g_rays[bad[:4]].tolist(), o_rays.reshape(-1)[bad[:4]].tolist())
        assert (g_rays <= depth + 1).all() and (g_rays >= 1).all()
    if name not in ("empty", "sky_only"):
        assert len(solid) > 0 and (o_rays > 1).any(), name  # the paths bounced


# ------------------------------------------------------------------ GPU against GPU
def camera_rays(cam, h, w, items, pixel_of, states):
    """The render's camera ray of each work item (render_body.h, ray_tracing.cu:68-73 + camera.cu:57-70) from its
    state: (origins, directions normalised once, states after the two jitter draws)."""
    pos, llc, horiz, vert = (cam[k].astype(np.float32) for k in range(4))
    after = advance_two(states)
    O = np.tile(pos, (items, 1)).astype(np.float32)
    Dn = np.zeros((items, 3), dtype=np.float32)
    L = oraclelib.lib()
    for q in range(items):
        idx = int(pixel_of[q])
        i, j = idx // w, idx % w
        st = np.ascontiguousarray(states[q], dtype=np.uint32).copy()
        p = st.ctypes.data_as(C.POINTER(C.c_uint32))
        r1 = L.orc_random_float(C.c_float(0.0), C.c_float(1.0), p)
        r2 = L.orc_random_float(C.c_float(0.0), C.c_float(1.0), p)
        x = (float(np.float32(r1)) + j) / w
        y = (float(np.float32(r2)) + (h - i)) / h
        x, y = (2 * x - 1 + 1) / 2, (2 * y - 1 + 1) / 2
        xf, yf = np.float32(x), np.float32(y)
        target = ((llc + xf * horiz) + yf * vert).astype(np.float32)
        Dn[q] = glm_normalize(target - pos)
    return O, Dn, after


@pytest.mark.parametrize("name,depth", [("cornell_box", 50), ("birthday", 10)])
def test_trace_reproduces_the_render(name, depth):
    h = w = 64
    seed = common.scene_seed(name)
    b = common.build_scene(rtmi.SceneBuilder(seed), name, 1.0).commit()
    R = rtmi.Renderer(b, h, w, 1, depth, post=False)
    R.init_rng()
    st0 = np.ascontiguousarray(R.states.cpu().numpy().view(np.uint32).T)
    R.render()
    R.check()
    torch.cuda.synchronize()
    tiles, counts = R.tiles.cpu().numpy(), R.ray_counts.cpu().numpy().view(np.uint32)
    fin = np.ascontiguousarray(R.states.cpu().numpy().view(np.uint32).T)
    pixel_of = rtmi.pixel_map(R.frame)
    assert (pixel_of >= 0).all()
    O, Dn, handed = camera_rays(b.camera_get(), h, w, R.items, pixel_of, st0)
    g_rgb, g_rays, g_fin, tr = gpu_trace(b, O, Dn, handed, depth)
    assert tr.total_rays() == int(counts.sum()) == R.total_rays()
    assert np.array_equal(g_rays, counts)
    assert np.array_equal(bits(g_rgb), bits(tiles)), np.flatnonzero((bits(g_rgb) != bits(tiles)).any(1))[:8]
    assert np.array_equal(g_fin, fin)


# ------------------------------------------------------------------ edge cases
def _world():
    b, rec, ob, seed = build("no_sky")
    O, D = make_rays(ob, 5, n_family=100)
    return b, ob, seed, O, D


def test_bad_rays_are_left_out():
    b, ob, seed, O, D = _world()
    n = 256
    O, D = O[:n].copy(), D[:n].copy()
    states = oraclelib.rng_init(seed, n, first=99)
    good_rgb, good_rays, good_fin, _ = gpu_trace(b, O, D, states, 8)
    bad = np.arange(3, n, 7)
    O2, D2 = O.copy(), D.copy()
    kinds = [(O2, 0, np.nan), (D2, 1, np.inf), (D2, None, 0.0), (O2, 2, -np.inf), (D2, None, 1e-30), (D2, None, 1e30)]
    for k, i in enumerate(bad):
        arr, col, val = kinds[k % len(kinds)]
        if col is None:
            arr[i] = val
        else:
            arr[i, col] = val
    rgb, rays, fin, _ = gpu_trace(b, O2, D2, states, 8)
    # 1e-30 / 1e30 components: |d|^2 underflows / overflows, so the direction does not normalise
    assert (bits(rgb[bad]) == 0).all() and (rays[bad] == 0).all()
    assert np.array_equal(fin[bad], states[bad])
    ok = np.setdiff1d(np.arange(n), bad)
    assert np.array_equal(bits(rgb[ok]), bits(good_rgb[ok])) and np.array_equal(rays[ok], good_rays[ok])
    assert np.array_equal(fin[ok], good_fin[ok])


@pytest.mark.parametrize("n", [0, 1, 63, 65])
def test_batch_sizes(n):
    b, ob, seed, O, D = _world()
    O, D = O[:n], D[:n]
    keep = usable(O, D)
    assert keep.all()
    states = oraclelib.rng_init(seed, max(n, 1) * 2, first=7)[: n * 2].reshape(n, 2, 6)
    o_rgb, o_rays, o_fin, dirs, handed = oracle_trace(ob, O, D, states, 10)
    g_rgb, g_rays, g_fin, tr = gpu_trace(b, np.repeat(O, 2, 0), np.repeat(dirs, 2, 0), handed.reshape(-1, 6), 10)
    assert g_rgb.shape == (n * 2, 3)
    assert np.array_equal(bits(g_rgb), bits(o_rgb.reshape(-1, 3)))
    assert np.array_equal(g_rays, o_rays.reshape(-1)) and np.array_equal(g_fin, o_fin.reshape(-1, 6))
    assert tr.total_rays() == int(o_rays.sum())


def test_null_ray_counts_and_out_buffer():
    b, ob, seed, O, D = _world()
    n = len(O)
    st = rtmi.rng_states(seed, n, first=5)
    st2 = st.clone()
    o, d = torch.from_numpy(O).cuda(), torch.from_numpy(D).cuda()
    a = b.trace(o, d, st, 8, count_rays=True).check()
    out = torch.full((n, 3), 7.0, dtype=torch.float32, device=o.device)
    c = b.trace(o, d, st2, 8, out=out).check()
    assert c.rays is None and c.rgb.data_ptr() == out.data_ptr()
    torch.cuda.synchronize()
    assert torch.equal(a.rgb.view(torch.int32), out.view(torch.int32)) and torch.equal(st, st2)
    assert c.total_rays() == a.total_rays() == int(a.rays.sum().item())


def test_two_streams_with_their_own_work():
    b, ob, seed, O, D = _world()
    O, D = np.tile(O, (8, 1)), np.tile(D, (8, 1))
    n = len(O)
    st_a = rtmi.rng_states(seed, n)
    st_b = st_a.clone()
    ref = b.trace(torch.from_numpy(O).cuda(), torch.from_numpy(D).cuda(), st_a.clone(), 50, count_rays=True).check()
    torch.cuda.synchronize()
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    o, d = torch.from_numpy(O).cuda(), torch.from_numpy(D).cuda()
    torch.cuda.synchronize()
    with torch.cuda.stream(s1):
        t1 = b.trace(o, d, st_a, 50, count_rays=True)
    with torch.cuda.stream(s2):
        t2 = b.trace(o, d, st_b, 50, count_rays=True)
    torch.cuda.synchronize()
    t1.check(), t2.check()
    for t in (t1, t2):
        assert torch.equal(t.rgb.view(torch.int32), ref.rgb.view(torch.int32)) and torch.equal(t.rays, ref.rays)
        assert t.total_rays() == ref.total_rays()
    assert torch.equal(st_a, st_b)


def test_four_million_rays_on_bunny():
    """2^22 rays (the bunny's camera rays repeated), each with its own state; a sample checked against the oracle."""
    b, rec, ob, seed = build("bunny")
    O, D = make_rays(ob, 21, n_family=1000)
    O, D = O[usable(O, D)], D[usable(O, D)]
    n = 1 << 22
    rng = np.random.default_rng(3)
    pick = rng.integers(0, len(O), n)
    Ob, Db = O[pick], D[pick]
    dirs = np.zeros_like(Db)
    llc = (Ob + Db).astype(np.float32)
    dirs[:] = glm_normalize(((llc + F0) + F0).astype(np.float32) - Ob)
    st = rtmi.rng_states(seed, n, first=1 << 20)
    st_in = np.ascontiguousarray(st.cpu().numpy().view(np.uint32).T)
    tr = b.trace(torch.from_numpy(Ob).cuda(), torch.from_numpy(dirs).cuda(), st, 10, count_rays=True).check()
    torch.cuda.synchronize()
    rgb, rays = tr.rgb.cpu().numpy(), tr.rays.cpu().numpy().view(np.uint32)
    fin = np.ascontiguousarray(st.cpu().numpy().view(np.uint32).T)
    assert tr.total_rays() == int(rays.sum(dtype=np.int64))
    # a sample of the batch's rays against the oracle, through the bridge with states of its own
    sample = rng.choice(n, 128, replace=False)
    states = oraclelib.rng_init(seed, 128, first=777).reshape(128, 1, 6)
    o_rgb, o_rays, o_fin, dirs_o, handed = oracle_trace(ob, Ob[sample], Db[sample], states, 10)
    assert np.array_equal(bits(dirs_o), bits(dirs[sample]))
    g_rgb, g_rays, g_fin, _ = gpu_trace(b, Ob[sample], dirs[sample], handed.reshape(-1, 6), 10)
    assert np.array_equal(bits(g_rgb), bits(o_rgb.reshape(-1, 3))) and np.array_equal(g_rays, o_rays.reshape(-1))
    assert np.array_equal(g_fin, o_fin.reshape(-1, 6))
    # ... and the big batch's own answers for those rays equal a small call with the same states
    s_rgb, s_rays, s_fin, _ = gpu_trace(b, Ob[sample], dirs[sample], st_in[sample], 10)
    assert np.array_equal(bits(s_rgb), bits(rgb[sample])) and np.array_equal(s_rays, rays[sample])
    assert np.array_equal(s_fin, fin[sample])


def test_arguments_refused_before_gpu_work():
    b, ob, seed, O, D = _world()
    o, d = torch.from_numpy(O).cuda(), torch.from_numpy(D).cuda()
    st = rtmi.rng_states(seed, len(O))
    for depth in (-1, 65):
        with pytest.raises(rtmi.RtmiError):
            b.trace(o, d, st, depth)
    with pytest.raises(rtmi.RtmiError):
        b.trace(o, d, st[:, :-1].contiguous(), 8)
    with pytest.raises(rtmi.RtmiError):
        b.trace(o, d, st.to(torch.int64), 8)
    with pytest.raises(rtmi.RtmiError):
        b.trace(o.cpu(), d.cpu(), st, 8)
    # the C entry: RTMI_ERR_DEPTH for max_depth outside [0, 64], RTMI_ERR_INVALID for a device mismatch
    L = rtmi.lib()
    work = torch.zeros((rtmi.TRACE_WORK_WORDS,), dtype=torch.int64, device=o.device)
    rgb = torch.empty((len(O), 3), dtype=torch.float32, device=o.device)
    args = (C.c_void_p(o.data_ptr()), C.c_void_p(d.data_ptr()))
    for depth in (-1, 65):
        assert L.rtmi_trace(b.h, len(O), *args, depth, C.c_void_p(st.data_ptr()), C.c_void_p(rgb.data_ptr()), None,
                            C.c_void_p(work.data_ptr()), None) == ERR_DEPTH
    if torch.cuda.device_count() > 1:
        with torch.cuda.device(1):
            assert L.rtmi_trace(b.h, len(O), *args, 8, C.c_void_p(st.data_ptr()), C.c_void_p(rgb.data_ptr()), None,
                                C.c_void_p(work.data_ptr()), None) == ERR_INVALID
            with pytest.raises(rtmi.RtmiError):
                b.trace(o.to("cuda:1"), d.to("cuda:1"), st.to("cuda:1"), 8)


# ------------------------------------------------------------------ seeding
def test_rng_states_equal_the_oracle():
    for seed, first, n in [(0, 0, 1000), (1234, 17, 513), (2024, (1 << 32) + 5, 300), (7, (1 << 40) - 64, 64)]:
        st = rtmi.rng_states(seed, n, first=first)
        got = np.ascontiguousarray(st.cpu().numpy().view(np.uint32).T)
        assert np.array_equal(got, oraclelib.rng_init(seed, n, first)), (seed, first)
    L = rtmi.lib()
    buf = torch.zeros((6, 64), dtype=torch.int32, device="cuda")
    assert L.rtmi_rng_init_n(1, (1 << 40) - 63, 64, C.c_void_p(buf.data_ptr()), None) == ERR_INVALID
    assert L.rtmi_rng_init_n(1, 1 << 41, 1, C.c_void_p(buf.data_ptr()), None) == ERR_INVALID
    assert L.rtmi_rng_init_n(1, 0, 0, None, None) == OK
    assert (buf == 0).all()
    with pytest.raises(rtmi.RtmiError):
        rtmi.rng_states(1, 64, first=(1 << 40) - 63)
