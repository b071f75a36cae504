"""rtmi_intersect / SceneBuilder.intersect against the oracle, ray by ray.

Every answer is compared with OracleBuilder.probe_hit -- HitableList::Hit(Ray(o, d), 1e-3, inf) of the reference's
own objects: hit / no hit, float32(t), the normal and the material bit for bit; u, v bit for bit on triangles,
parallelograms and meshes (spheres: within the device's acosf / atan2f, as for birthday); Sky on t and kind only.
`entry` / `element` are checked by the kind of the recorded call they name, and on a sample by a one-primitive oracle
world holding just that hitable (or that one face) that must give the same t for the same ray."""
import numpy as np
import pytest

import rtmi
from querylib import CUSTOM_WORLDS, SCENE_WORLDS, build, check_identities, compare, gpu_intersect, make_rays, v3, world_no_sky

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

@pytest.mark.parametrize("name", SCENE_WORLDS + sorted(CUSTOM_WORLDS))
def test_intersect_matches_the_oracle(name):
    b, rec, ob, seed = build(name)
    O, D = make_rays(ob, 1000 + len(name))
    assert 4000 <= len(O) <= 16000 or name in ("empty", "sky_only"), len(O)
    h = gpu_intersect(b, O, D)
    raw = h.raw.cpu().numpy()
    bad = compare(raw, ob, O, D, rec)
    assert not bad, (name, bad)
    # the named tuple's views are the buffer's columns
    assert np.array_equal(h.t.cpu().numpy().view(np.int32), raw[:, 0])
    assert np.array_equal(h.kind.cpu().numpy(), raw[:, 7]) and np.array_equal(h.entry.cpu().numpy(), raw[:, 8])
    assert (raw[:, 10:12] == 0).all()
    kinds = set(np.unique(raw[:, 7]).tolist())
    if name not in ("empty", "sky_only"):
        assert kinds - {rtmi.RTMI_HIT_NONE, rtmi.RTMI_HIT_SKY}, (name, kinds)  # the rays found the geometry
    if name == "empty":
        assert kinds == {rtmi.RTMI_HIT_NONE}
    bad = check_identities(b, rec, seed, O, D, raw, np.random.default_rng(seed))
    assert not bad, (name, bad)


def test_batch_shapes_bad_rays_and_t_max():
    b, rec, ob, seed = build("cornell_box")
    O, D = make_rays(ob, 77)
    ref = gpu_intersect(b, O, D).raw.cpu().numpy()
    # n = 1, 63, 65 (ragged waves) and 0
    for n in (1, 63, 65):
        assert np.array_equal(gpu_intersect(b, O[:n], D[:n]).raw.cpu().numpy(), ref[:n]), n
    h0 = gpu_intersect(b, O[:0], D[:0])
    assert tuple(h0.raw.shape) == (0, 12)
    # bad rays mixed into the batch: NONE for them, every other answer unchanged
    Ob, Db = O.copy(), D.copy()
    which = np.arange(len(O)) % 13 == 5
    k = np.nonzero(which)[0]
    for j, i in enumerate(k):
        r = j % 8
        if r == 0:
            Ob[i, 0] = np.nan
        elif r == 1:
            Db[i, 1] = np.inf
        elif r == 2:
            Db[i] = 0.0  # zero direction
        elif r == 3:
            Ob[i, 2] = -np.inf
        elif r == 4:
            Db[i, 0] = -np.inf
        elif r == 5:
            Db[i, 2] = np.nan
        elif r == 6:
            Db[i] = 1e30  # |d|^2 overflows: no finite unit direction
        else:
            Db[i] = 1e-30  # |d|^2 underflows to 0
    got = gpu_intersect(b, Ob, Db).raw.cpu().numpy()
    assert (got[which, 7] == rtmi.RTMI_HIT_NONE).all()
    assert np.isinf(got[which].view(np.float32)[:, 0]).all()
    assert np.array_equal(got[~which], ref[~which])
    # t_max: inclusive at the hit's own t, below it by one ulp the hit is dropped
    t = ref.view(np.float32)[:, 0]
    hits = ref[:, 7] != rtmi.RTMI_HIT_NONE
    keep = gpu_intersect(b, O, D, t_max=np.where(hits, t, np.float32(0))).raw.cpu().numpy()
    assert np.array_equal(keep[hits], ref[hits])
    below = np.nextafter(t, np.float32(-np.inf)).astype(np.float32)
    drop = gpu_intersect(b, O, D, t_max=np.where(hits, below, np.float32(np.inf))).raw.cpu().numpy()
    assert (drop[hits, 7] == rtmi.RTMI_HIT_NONE).all() and (drop[hits, 6] == -1).all()
    assert np.array_equal(drop[~hits], ref[~hits])


def test_two_streams_agree_and_out_buffer():
    b, rec, ob, seed = build("bunny")
    O, D = make_rays(ob, 5)
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    h1 = gpu_intersect(b, O, D, stream=s1)
    h2 = gpu_intersect(b, O, D, stream=s2)
    torch.cuda.synchronize()
    assert torch.equal(h1.raw, h2.raw)
    out = torch.full((len(O), 12), -7, dtype=torch.int32, device="cuda")
    h3 = b.intersect(torch.from_numpy(O).cuda(), torch.from_numpy(D).cuda(), out=out).check()
    assert h3.raw.data_ptr() == out.data_ptr() and torch.equal(out, h1.raw)


def test_four_million_rays_on_bunny():
    """One batch of 2^22 camera-like rays on the bunny; 10k of them checked against the oracle."""
    b, rec, ob, seed = build("bunny")
    cam = ob.camera_get()  # position, lower-left corner, horizontal, vertical
    n = 1 << 22
    g = torch.Generator(device="cuda").manual_seed(11)
    xy = torch.rand((n, 2), generator=g, device="cuda", dtype=torch.float32)
    c = torch.from_numpy(np.ascontiguousarray(cam[:4], dtype=np.float32)).cuda()
    o = c[0].expand(n, 3).contiguous()
    d = (c[1] + xy[:, :1] * c[2] + xy[:, 1:] * c[3] - c[0]).contiguous()
    h = b.intersect(o, d).check()
    raw = h.raw.cpu().numpy()
    assert (raw[:, 7] == rtmi.RTMI_HIT_MESH).sum() > n // 20
    idx = np.random.default_rng(3).choice(n, 10000, replace=False)
    bad = compare(raw, ob, o.cpu().numpy(), d.cpu().numpy(), rec, idx)
    assert not bad, bad


def test_device_check_and_uncommitted_scene():
    b = rtmi.SceneBuilder(1)
    world_no_sky(b)
    o = torch.zeros((4, 3), dtype=torch.float32, device="cuda")
    with pytest.raises(rtmi.RtmiError, match="not committed"):
        b.intersect(o, o)
    b.commit()
    b.sphere(v3(5, 5, 5), 1.0, 0)  # recording after the commit un-commits the scene
    with pytest.raises(rtmi.RtmiError, match="not committed"):
        b.intersect(o, o)
