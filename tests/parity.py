"""The one render harness of the suite: the same world on the oracle and on the product, a frame of each, and the
comparison of the two.

A GPU parity test is four calls:

    ob, pb = build_pair(fill, seed)
    assert_same_frame(gpu_frame(pb, h, w, spp, depth), oracle_frame(ob, h, w, spp, depth), "what it is")

`fill(b)` records the world on either builder; a world whose camera depends on the frame's shape closes over it
(`lambda b: scenes.cornell_box(b, w / h)`).  A helper module is not assertion-rewritten by pytest, so every assert here
says which field failed and by how much."""
import collections

import numpy as np

# image (H, W, 3) float32; counts (H, W) uint32; states (H*W, 6) uint32, row-major, or None; total int;
# mode: the dict of rtmi_render_mode, None for the oracle
Frame = collections.namedtuple("Frame", "image counts states total mode")


def bits(x):
    """The 32-bit words of x: binary32 and 32-bit integers as they are, anything else rounded to binary32 first."""
    x = np.ascontiguousarray(x)
    if x.dtype.itemsize != 4 or x.dtype.kind not in "fiu":
        x = x.astype(np.float32)
    return x.view(np.uint32)


def same(a, b):
    return a.shape == b.shape and np.array_equal(bits(a), bits(b))


def states_rowmajor(states_per_rank, h, w, world=1):
    """(H*W, 6) uint32 from the per-rank SoA planes [6][items]; padding items are left out."""
    import rtmi
    out = np.zeros((h * w, 6), dtype=np.uint32)
    for r, st in enumerate(states_per_rank):
        pm = rtmi.pixel_map(rtmi.make_frame(h, w, 1, rank=r, world_size=world))
        planes = (st.cpu().numpy() if hasattr(st, "cpu") else np.asarray(st)).view(np.uint32)  # (6, items)
        ok = pm >= 0
        out[pm[ok]] = planes[:, ok].T
    return out


def build_pair(fill, seed, camera=None, record=False):
    """The same world on an OracleBuilder and on a SceneBuilder (committed): `camera(b)`, if given, then `fill(b)` on
    each.  record=True: the product's builder sits behind a querylib.Recorder, which is what comes back."""
    import oraclelib
    import rtmi
    ob, pb = oraclelib.OracleBuilder(seed), rtmi.SceneBuilder(seed)
    if record:
        import querylib
        pb = querylib.Recorder(pb)
    for b in (ob, pb):
        if camera is not None:
            camera(b)
        fill(b)
    (pb.b if record else pb).commit()
    return ob, pb


def oracle_frame(ob, h, w, spp, depth, post=True, threads=None):
    rgb, rays, states, total = ob.render(h, w, spp, depth, post=post, threads=threads)
    for a in (rgb, rays, states):
        a.setflags(write=False)
    return Frame(rgb, rays, states, total, None)


def render_shards(pb, h, w, spp, depth, post=True, opts=None, world=1):
    """Every shard of the frame on the one GPU, assembled as a gather would: (image, counts, the ranks' tile-major
    state planes, ray total, mode).  Every render is checked (rtmi_render_status) before it is read."""
    import torch
    import rtmi
    ro = rtmi.render_opts(**opts) if opts is not None else None
    tiles, counts, states, total = [], [], [], 0
    for r in range(world):
        R = rtmi.Renderer(pb, h, w, spp, depth, post, rank=r, world_size=world).init_rng()
        R.render(opts=ro)
        R.check()
        total += R.total_rays()
        tiles.append(R.tiles), counts.append(R.ray_counts), states.append(R.states)
    img, cnt = R.untile(torch.cat(tiles, 0).contiguous(), torch.cat(counts, 0).contiguous())
    torch.cuda.synchronize()
    return img.cpu().numpy(), cnt.cpu().numpy().astype(np.uint32), states, total, R.mode(ro)


def gpu_frame(pb, h, w, spp, depth, post=True, opts=None, world=1):
    """`opts`: a dict of rtmi.render_opts arguments, None for a call without options."""
    img, cnt, states, total, mode = render_shards(pb, h, w, spp, depth, post, opts, world)
    return Frame(img, cnt, states_rowmajor(states, h, w, world), total, mode)


def assert_same_frame(got, want, what, nan_ok=False):
    """Ray totals, per-pixel ray counts, final RNG states (where `want` has them), image shape, image bits.
    nan_ok: NaNs must sit at the same positions and every other value have the same bits; otherwise `want` has none."""
    if not nan_ok:
        assert not np.isnan(want.image).any(), "%s: the expected image holds %d NaNs" % (what, np.isnan(want.image).sum())
    assert got.total == want.total, "%s: ray totals %d vs %d" % (what, got.total, want.total)
    assert got.counts.shape == want.counts.shape, "%s: ray counts of shape %s vs %s" % (what, got.counts.shape, want.counts.shape)
    bad = got.counts != want.counts
    assert not bad.any(), "%s: %d pixels with different ray counts (max abs difference %d)" % (
        what, bad.sum(), np.abs(got.counts.astype(np.int64) - want.counts.astype(np.int64)).max())
    if want.states is not None:
        assert got.states is not None and got.states.shape == want.states.shape, "%s: no final RNG states of shape %s" % (
            what, want.states.shape)
        bad = got.states != want.states
        assert not bad.any(), "%s: final RNG states differ in %d words of %d pixels" % (what, bad.sum(), bad.any(axis=1).sum())
    assert got.image.shape == want.image.shape, "%s: image of shape %s vs %s" % (what, got.image.shape, want.image.shape)
    g, w = bits(got.image), bits(want.image)
    bad = g != w
    if nan_ok:
        gn, wn = np.isnan(got.image), np.isnan(want.image)
        assert np.array_equal(gn, wn), "%s: NaNs at %d positions vs %d, %d positions differ" % (
            what, gn.sum(), wn.sum(), (gn != wn).sum())
        bad &= ~wn
    if bad.any():
        with np.errstate(invalid="ignore"):
            worst = np.nanmax(np.abs(got.image.astype(np.float64) - want.image)[bad])
        i = tuple(int(k) for k in np.argwhere(bad)[0])
        raise AssertionError("%s: %d image words differ (max abs difference %g); first at (row, column, channel) %s: %08x vs %08x"
                             % (what, bad.sum(), worst, i, g[i], w[i]))
