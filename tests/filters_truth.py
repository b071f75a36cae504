"""What rtmi_denoise and rtmi_accumulate are held to beyond their own restatements: binary64 truth.

tests/filter_rules.py restates the two rules in binary32 (``denoise_rule``,
``accumulate_rule``) and the GPU tests hold the device to them bit for bit; that proves "kernel == rule" and says nothing
about whether the rule computes what include/rtmi.h claims.  The checks here ask that, of anything that filters or
accumulates -- a callable.  tests/test_filters_truth_host.py passes the numpy rules, tests/test_gpu_filters_truth.py the
library: one function, on the CPU and on the device.

- ``denoise_truth``: the header's formulas in binary64, written plainly, with each pass's keep / filter decision per pixel
  taken from the binary32 run, so that the one discontinuity of the rule cannot masquerade as error.
- ``landing_truth``: where a pixel's world point lands in the previous image, in binary64 from the cameras' 21 floats with
  a linear solve (the rule uses the rows of an inverse formed with cross products).

Every tolerance below is derived in its comment or is 8 times a figure measured with the numpy rule against these
functions on exactly these inputs (``measure()``; DESIGN.md 2.8 and 2.9 record the figures), never on the device."""
import numpy as np

import rtmi
from filter_rules import MIN_WEIGHT_SUM, accumulate_rule, camera_of, denoise_rule, room

F32 = np.float32
F64 = np.float64


def f(x):
    """A binary32 constant of the header (0.25f, 1e-6f, ...) as the binary64 number it is."""
    return float(F32(x))


def same_or_nan(a, b):
    """Bit equality of two float32 arrays, elementwise, any NaN equal to any NaN (their payloads are nobody's promise)."""
    a, b = np.ascontiguousarray(a, dtype=F32), np.ascontiguousarray(b, dtype=F32)
    return (a.view(np.uint32) == b.view(np.uint32)) | (np.isnan(a) & np.isnan(b))


# ------------------------------------------------------------------ inputs
def synthetic(h, w, seed=0):
    """dict of rtmi.denoise's inputs, numpy float32: colours in [0, 4); variances in [0, 1), about a fifth exactly 0; mean
    normals of length <= 1; depths in [0.5, 20); alpha in {0, 0.25, 1} with patches of background; albedo in [0, 1] with
    exact zeros."""
    rng = np.random.default_rng([seed, h, w])
    I, J = np.meshgrid(np.arange(h), np.arange(w), indexing="ij")
    patch = ((I // 5) * 3 + J // 7) % 6  # 5 x 7 pixel patches of six kinds; kind 5 is background
    base_n = np.array([[0, 0, 1], [0, 1, 0], [0.6, 0, 0.8], [0, 0.6, 0.8], [1, 0, 0], [0, 0, 0]], F32)
    base_z = np.array([2.0, 2.2, 9.0, 9.5, 18.0, 0.0], F32)
    n = base_n[patch] + rng.normal(0, 0.08, (h, w, 3)).astype(F32)
    n = n / np.sqrt((n * n).sum(-1, keepdims=True), dtype=F32)
    n = (n * rng.uniform(0.5, 0.999, (h, w, 1)).astype(F32)).astype(F32)
    z = np.clip(base_z[patch] * (1 + rng.normal(0, 0.03, (h, w))), 0.5, 19.99).astype(F32)
    alpha = rng.choice(np.array([0.25, 1.0], F32), (h, w))
    alpha[(patch == 5) | (rng.random((h, w)) < 0.05)] = 0
    color = (rng.random((h, w, 3)) * 4).astype(F32)
    color[..., 1] = color[..., 0] * F32(0.5) + color[..., 1] * F32(0.1)  # (correlated channels: d2 small against vs somewhere)
    variance = rng.random((h, w, 3)).astype(F32)
    variance[rng.random((h, w, 3)) < 0.2] = 0
    albedo = rng.random((h, w, 3)).astype(F32)
    albedo[rng.random((h, w, 3)) < 0.1] = 0
    albedo[rng.random((h, w)) < 0.05] = 1
    d = dict(color=color, variance=variance, normal=n, depth=z, alpha=alpha.astype(F32), albedo=albedo)
    assert all(v.dtype == F32 for v in d.values())
    assert 0 <= color.min() and color.max() < 4 and variance.max() < 1 and (n * n).sum(-1).max() <= 1.0001
    return d


def rule_denoise(d, demodulate, **opts):
    """The numpy rule as a denoiser: (out, out_variance) of the inputs of dict d."""
    d = dict(d)
    if not demodulate:
        d.pop("albedo")
    return denoise_rule(**d, **opts)


def rule_chain(frames):
    """The numpy rule as an accumulator over a sequence of (inputs, camera, options): the last frame's (out, variance,
    length)."""
    hist = prev = got = None
    for d, cam, opts in frames:
        got = accumulate_rule(**d, camera=cam, history=hist, prev_camera=prev, **opts)
        hist, prev = got[3], cam
    return got[:3]


# ------------------------------------------------------------------ denoise against binary64
DENOISE_SHAPES = [(33, 70), (64, 64)]
DENOISE_SQUARINGS = [0, 5, 6, 8]
DENOISE_ITERATIONS = [1, 5, 8]
COLOR_FLOOR, VARIANCE_FLOOR = 1e-3, 1e-6
# max |x - truth| / (|truth| + floor) of denoise_rule against denoise_truth over all 48 cases above (measure())
COLOR_MEASURED, VARIANCE_MEASURED = 4.47e-5, 8.08e-5
# 8 times those: the margin is for tap-order-independent rounding that differs between inputs and nothing else
COLOR_TOL, VARIANCE_TOL = 8 * COLOR_MEASURED, 8 * VARIANCE_MEASURED


def falloff64(x):
    m = np.maximum(1.0 - f(0.25) * x, 0.0)
    return (m * m) * (m * m)


def denoise_truth(color, variance, normal, depth, alpha, albedo=None, *, decisions, iterations, sigma_color=1.0,
                  sigma_depth=0.05, normal_squarings=0):
    """rtmi_denoise as include/rtmi.h states it, in binary64 from the binary32 inputs.  decisions[k] (H, W) bool: whether
    pass k filters the pixel (else it keeps C_p, V_p), as the binary32 run decided.  Demodulated iff an albedo is given.
    Returns (out, out_variance, [sw of pass k])."""
    C0, V0, N, Z, A = (np.asarray(x, dtype=F32).astype(F64) for x in (color, variance, normal, depth, alpha))
    H, W = Z.shape
    h5 = (1 / 16, 1 / 4, 3 / 8, 1 / 4, 1 / 16)
    sc2, sz = f(sigma_color) ** 2, f(sigma_depth)
    with np.errstate(all="ignore"):
        if albedo is not None:
            ad = np.maximum(np.asarray(albedo, dtype=F32).astype(F64), f(0.01))
            Cc, V = C0 / ad, V0 / (ad * ad)
        else:
            Cc, V = C0.copy(), V0.copy()
        surf = A > 0
        I, J = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
        zden = sz * Z + f(1e-6)
        sws = []
        for k in range(iterations):
            s = 1 << k
            vsum = V.sum(-1)
            sw, sc, sv = np.zeros((H, W)), np.zeros((H, W, 3)), np.zeros((H, W, 3))
            for dy in range(-2, 3):
                for dx in range(-2, 3):
                    qi, qj = I + dy * s, J + dx * s
                    inside = (qi >= 0) & (qi < H) & (qj >= 0) & (qj < W)
                    ci, cj = np.clip(qi, 0, H - 1), np.clip(qj, 0, W - 1)
                    take = inside & (surf == surf[ci, cj])
                    wn = np.maximum((N * N[ci, cj]).sum(-1), 0.0) ** (2 ** normal_squarings)
                    wz = falloff64(np.abs(Z - Z[ci, cj]) / zden)
                    wn, wz = np.where(surf, wn, 1.0), np.where(surf, wz, 1.0)
                    d2 = ((Cc - Cc[ci, cj]) ** 2).sum(-1)
                    wc = falloff64(d2 / (sc2 * (vsum + vsum[ci, cj]) + f(1e-10)))
                    w = np.where(take, h5[dy + 2] * h5[dx + 2] * wn * wz * wc, 0.0)
                    sw += w
                    sc += w[..., None] * Cc[ci, cj]
                    sv += (w * w)[..., None] * V[ci, cj]
            ok = np.asarray(decisions[k], dtype=bool)[..., None]
            Cc, V = np.where(ok, sc / sw[..., None], Cc), np.where(ok, sv / (sw * sw)[..., None], V)
            sws.append(sw)
        if albedo is not None:
            Cc, V = Cc * ad, V * (ad * ad)
    return Cc, V, sws


def denoise_errors(denoise, d, demodulate, **opts):
    """Runs `denoise` (a callable like rule_denoise) and the truth under the binary32 rule's decisions.  Returns
    (got, decisions, sws, worst colour error, worst variance error), the errors as |x - truth| / (|truth| + floor), inf where
    a float is not finite."""
    got = denoise(d, demodulate, **opts)
    decisions = []
    dd = dict(d)
    if not demodulate:
        dd.pop("albedo")
    denoise_rule(**dd, **opts, decisions=decisions)
    tc, tv, sws = denoise_truth(**dd, decisions=decisions, **opts)
    worst = []
    with np.errstate(all="ignore"):
        for x, t, floor in ((got[0], tc, COLOR_FLOOR), (got[1], tv, VARIANCE_FLOOR)):
            e = np.abs(x.astype(F64) - t) / (np.abs(t) + floor)
            worst.append(float(np.where(np.isfinite(e), e, np.inf).max()))
    return got, decisions, sws, worst[0], worst[1]


def check_denoise_truth(denoise, shape, squarings, iterations, demodulate):
    """(a) every output float is finite; (b) the decisions are right: a kept pixel's binary64 sw is below twice the threshold,
    a filtered pixel's above half of it; (c) colour and variance are within COLOR_TOL, VARIANCE_TOL of the truth."""
    d = synthetic(*shape)
    got, decisions, sws, ec, ev = denoise_errors(denoise, d, demodulate, iterations=iterations, normal_squarings=squarings)
    what = "%dx%d squarings %d iterations %d demodulate %d" % (shape + (squarings, iterations, demodulate))
    for name, x in zip(("out", "out_variance"), got):
        bad = ~np.isfinite(x)
        assert not bad.any(), "%s: %s is not finite in %d of %d floats, first at %s: %r" % (
            what, name, bad.sum(), bad.size, np.argwhere(bad)[0], x[bad][0])
    thr = float(MIN_WEIGHT_SUM)
    kept = 0
    for k, (ok, sw) in enumerate(zip(decisions, sws)):
        assert np.isfinite(sw).all(), (what, k)
        assert (sw[~ok] < 2 * thr).all(), "%s: pass %d keeps a pixel whose weights sum to %g" % (what, k, sw[~ok].max())
        assert (sw[ok] > thr / 2).all(), "%s: pass %d filters a pixel whose weights sum to %g" % (what, k, sw[ok].min())
        kept += int((~ok).sum())
    print("denoise truth %s: colour %.3g variance %.3g (of the tolerance: %.3f, %.3f), %d kept" % (
        what, ec, ev, ec / COLOR_TOL, ev / VARIANCE_TOL, kept))
    assert ec <= COLOR_TOL, (what, ec)
    assert ev <= VARIANCE_TOL, (what, ev)
    return kept


CONSTANT = np.array([0.7, 1.9, 3.3], F32)


def check_constant_colour(denoise, squarings, iterations, shape=(33, 70)):
    """A colour that is one constant per channel, over synthetic's guides and variances, not demodulated, comes back: a
    weighted mean of equal values.  sc / sw of 25 taps rounds 25 products, 24 + 24 additions and a division, each within
    2^-24 relative, and the weights are positive, so a pass moves a pixel by at most (2 * 25 + 1) 2^-24 relative from the
    span of what it read; `iterations` passes add up.  A pixel that every pass keeps is the constant bit for bit."""
    d = synthetic(*shape)
    d["color"] = np.broadcast_to(CONSTANT, shape + (3,)).copy()
    opts = dict(iterations=iterations, normal_squarings=squarings)
    out, var = denoise(d, 0, **opts)
    decisions = []
    dd = {k: v for k, v in d.items() if k != "albedo"}
    denoise_rule(**dd, **opts, decisions=decisions)
    assert np.isfinite(out).all() and np.isfinite(var).all()
    bound = (2 * 25 + 1) * iterations * 2.0 ** -24
    rel = np.abs(out.astype(F64) - CONSTANT.astype(F64)) / CONSTANT.astype(F64)
    print("constant colour, squarings %d iterations %d: worst %.3g of %.3g" % (squarings, iterations, rel.max(), bound))
    assert rel.max() <= bound, (squarings, iterations, rel.max(), bound)
    always_kept = ~np.any(decisions, axis=0)
    assert np.array_equal(out[always_kept], np.broadcast_to(CONSTANT, out[always_kept].shape))
    assert rel.max() > 0 and (~always_kept).any()  # (the filter did run)
    return int(always_kept.sum())


# ------------------------------------------------------------------ accumulate: the landing point against binary64
LANDING_SHAPES = [(16, 16), (33, 70), (64, 64), (70, 130)]
LANDING_MOVES = ["slide", "pan"]
SNAP = 1.0 / 64
# the largest |landing - truth| in pixels of accumulate_rule over the cases above where it did not snap (measure())
LANDING_MEASURED = 2.22e-5
LANDING_M = 8 * LANDING_MEASURED
LANDING = dict(normal_min=-1.0, depth_tolerance=1e30, min_blend=0.0)  # every in-image surface tap is taken, L' = 2


def landing_truth(h, w, camera, prev_camera, depth):
    """Where pixel (i, j)'s world point lands in the previous image, in binary64 from the cameras' 21 floats:
    P = p + z_p unit(centre ray); [h' v' llc' - p'] (alpha beta gamma)^T = P - p' by a linear solve; fx = alpha / gamma W - 1/2,
    fy = H + 1/2 - beta / gamma H.  Returns (fx, fy, gamma, |P - p'|), each (H, W)."""
    cur, prev = (np.asarray(c, dtype=F32).reshape(-1).astype(F64) for c in (camera, prev_camera))
    p, llc, hh, vv = cur[0:3], cur[3:6], cur[6:9], cur[9:12]
    I, J = np.meshgrid(np.arange(h), np.arange(w), indexing="ij")
    xf, yf = (J + 0.5) / w, ((h - I) + 0.5) / h
    D = (llc - p) + xf[..., None] * hh + yf[..., None] * vv
    D = D / np.sqrt((D * D).sum(-1, keepdims=True))
    d = p + D * np.asarray(depth, dtype=F64)[..., None] - prev[0:3]
    M = np.column_stack([prev[6:9], prev[9:12], prev[3:6] - prev[0:3]])
    with np.errstate(all="ignore"):
        al, be, ga = np.linalg.solve(M, d.reshape(-1, 3).T).reshape(3, h, w)
        return al / ga * w - 0.5, h + 0.5 - be / ga * h, ga, np.sqrt((d * d).sum(-1))


def landing_frames(h, w, move, **opts):
    """Frame 1 from the home camera with alpha 1 everywhere and colour (j, i, 1); frame 2 from the moved camera with colour 0.
    Under LANDING the second frame's 2 C' is then (fx, fy, 1) wherever all four taps lie in the image."""
    cam0, cam1 = camera_of("static", h, w), camera_of(move, h, w)
    d0, d1 = room(h, w, cam0), room(h, w, cam1, seed=1)
    I, J = np.meshgrid(np.arange(h), np.arange(w), indexing="ij")
    d0["alpha"][:] = 1
    d0["color"] = np.stack([J, I, np.ones_like(I)], -1).astype(F32)
    d1["color"][:] = 0
    return [(d0, cam0, {}), (d1, cam1, dict(LANDING, **opts))]


def landing_errors(chain, h, w, move, m):
    """-> (qualifying pixels, not snapped among them, |landing - truth| per axis (H, W, 2), out_length)."""
    frames = landing_frames(h, w, move)
    out, _, length = chain(frames)
    fx, fy, ga, _ = landing_truth(h, w, frames[1][1], frames[0][1], frames[1][0]["depth"])
    edge = SNAP + m
    with np.errstate(all="ignore"):
        inside = (ga > 0) & (fx >= edge) & (fx <= w - 1 - edge) & (fy >= edge) & (fy <= h - 1 - edge)  # all four taps
        qualifies = inside & (out[..., 2] * F32(2) == 1)
        free = qualifies & ((np.abs(fx - np.rint(fx)) > edge) | (np.abs(fy - np.rint(fy)) > edge))  # cannot have snapped
        err = np.abs(np.stack([out[..., 0] * 2.0 - fx, out[..., 1] * 2.0 - fy], -1))
    return qualifies, free, err, length


def check_landing(chain, shape, move):
    """|landing - truth| <= 1/64 + m in each axis on every qualifying pixel, <= m where the truth is further than 1/64 + m
    from an integer in either axis (the rule snaps only when both axes are within 1/64); at least 40 % of the pixels
    qualify; out_length is 2 there."""
    h, w = shape
    qualifies, free, err, length = landing_errors(chain, h, w, move, LANDING_M)
    share = qualifies.mean()
    print("landing %dx%d %s: %.1f %% qualify, %.1f %% of them cannot snap; worst %.3g px, not snapped %.3g px (m = %.3g)" % (
        h, w, move, 100 * share, 100 * free.sum() / max(qualifies.sum(), 1), err[qualifies].max(), err[free].max(), LANDING_M))
    assert share >= 0.4, share
    assert free.sum() >= qualifies.sum() // 2
    assert (err[qualifies] <= SNAP + LANDING_M).all(), err[qualifies].max()
    assert (err[free] <= LANDING_M).all(), err[free].max()
    assert (length[qualifies] == 2).all()


def check_depth_gate(chain, shape, move):
    """With the default depth_tolerance: a pixel whose true |z_q - |P - p'|| is below half the limit at all four taps is
    taken, one above twice the limit at all four is refused.  The taps are those of the true landing point, on pixels whose
    truth is further than 1/64 + m from an integer in both axes (so the rule's floor is the truth's)."""
    h, w = shape
    tol = rtmi.ACCUMULATE_DEFAULTS["depth_tolerance"]
    frames = landing_frames(h, w, move, depth_tolerance=tol)
    out, _, length = chain(frames)
    fx, fy, ga, dist = landing_truth(h, w, frames[1][1], frames[0][1], frames[1][0]["depth"])
    edge = SNAP + LANDING_M
    with np.errstate(all="ignore"):
        clear = (frames[1][0]["alpha"] > 0) & (ga > 0) & (fx >= edge) & (fx <= w - 1 - edge) & (fy >= edge) & (fy <= h - 1 - edge)
        clear &= (np.abs(fx - np.rint(fx)) > edge) & (np.abs(fy - np.rint(fy)) > edge)
        j0, i0 = np.where(clear, np.floor(fx), 0).astype(np.int64), np.where(clear, np.floor(fy), 0).astype(np.int64)
    zq = frames[0][0]["depth"].astype(F64)
    off = np.stack([np.abs(zq[i0 + di, j0 + dj] - dist) for di in (0, 1) for dj in (0, 1)])
    limit = f(tol) * dist
    taken, refused = clear & (off < limit / 2).all(0), clear & (off > 2 * limit).all(0)
    print("depth gate %dx%d %s: %d pixels must be taken, %d refused, of %d" % (h, w, move, taken.sum(), refused.sum(), h * w))
    assert taken.any()  # (the case is worth its name)
    assert (length[taken] == 2).all() and (out[..., 2][taken] * F32(2) == 1).all()
    assert (length[refused] == 1).all() and (out[..., 2][refused] == 0).all()
    return int(refused.sum())


# ------------------------------------------------------------------ accumulate: the convention against the renderer
SHIFTS = {"rule": (0.0, 0.0), "y-1": (0.0, -1.0), "y-1/2": (0.0, -0.5), "y+1/2": (0.0, 0.5), "y+1": (0.0, 1.0),
          "x-1": (-1.0, 0.0), "x-1/2": (-0.5, 0.0), "x+1/2": (0.5, 0.0), "x+1": (1.0, 0.0)}


def centre_rays(h, w, camera, shift=(0.0, 0.0)):
    """Unit centre rays of every pixel in binary64 under the rule's convention -- pixel (i, j)'s centre is (j + 1/2, H - i + 1/2)
    -- moved by `shift` pixels in (x, y): (origins, directions), both (H, W, 3)."""
    cam = np.asarray(camera, dtype=F32).reshape(-1).astype(F64)
    p, llc, hh, vv = cam[0:3], cam[3:6], cam[6:9], cam[9:12]
    I, J = np.meshgrid(np.arange(h), np.arange(w), indexing="ij")
    xf, yf = (J + 0.5 + shift[0]) / w, ((h - I) + 0.5 + shift[1]) / h
    D = (llc - p) + xf[..., None] * hh + yf[..., None] * vv
    return np.broadcast_to(p, D.shape).copy(), D / np.sqrt((D * D).sum(-1, keepdims=True))


def interior(mask):
    """The pixels of a bool image whose eight neighbours are all set too (none on the image's border)."""
    m = mask.copy()
    m[0], m[-1], m[:, 0], m[:, -1] = False, False, False, False
    for di in (-1, 0, 1):
        for dj in (-1, 0, 1):
            m[1:-1, 1:-1] &= mask[1 + di:mask.shape[0] - 1 + di, 1 + dj:mask.shape[1] - 1 + dj]
    return m


def check_convention(depth, normal, alpha, camera, closest_hit):
    """The rule reads `depth` as t along the unit ray through (j + 1/2, H - i + 1/2).  A renderer's mean depth, mean normal and
    alpha (row-major) are held to that: closest_hit(origins, directions) -> t of the scene the frame shows (inf: no hit),
    asked for the centre rays of the rule's convention and of the same moved by 1/2 and 1 pixel either way in y and in x.
    Rows are compared on floor and ceiling pixels (|n_y| > 0.999, alpha 1, all eight neighbours likewise), columns on the side
    walls (|n_x| > 0.999): there the depth changes along that axis.  Each class holds at least 100 pixels, and the rule's RMS
    of mean depth - t is at most 1/4 of every shifted candidate's.  (The mean is over jittered samples; 64 of them leave
    0.29 / 8 = 0.036 px against a shift of 0.5 px, so the ratio should be near 0.07 there.)  Returns the ratios."""
    depth, normal, alpha = (np.asarray(x, dtype=F32).astype(F64) for x in (depth, normal, alpha))
    h, w = depth.shape
    classes = {"y": interior((np.abs(normal[..., 1]) > 0.999) & (alpha == 1)),
               "x": interior((np.abs(normal[..., 0]) > 0.999) & (alpha == 1))}
    rms = {}
    for name, shift in SHIFTS.items():
        t = np.asarray(closest_hit(*centre_rays(h, w, camera, shift)), dtype=F64).reshape(h, w)
        for axis, cls in classes.items():
            if name == "rule" or name[0] == axis:
                with np.errstate(all="ignore"):
                    rms[axis, name] = float(np.sqrt(((depth[cls] - t[cls]) ** 2).mean()))
    ratios = {}
    for axis, cls in classes.items():
        assert cls.sum() >= 100, (axis, int(cls.sum()))
        for name in SHIFTS:
            if name[0] == axis:
                ratios[name] = rms[axis, "rule"] / rms[axis, name]
        print("convention, %s class: %d pixels, rule RMS %.4g; ratios %s" % (
            axis, cls.sum(), rms[axis, "rule"], ", ".join("%s %.3f" % (n, r) for n, r in ratios.items() if n[0] == axis)))
    for name, r in ratios.items():
        assert r <= 0.25, (name, r, rms)
    return ratios


# ------------------------------------------------------------------ the figures the tolerances come from
def measure():
    """The numpy rules against the truth on exactly the tests' inputs: what COLOR_MEASURED, VARIANCE_MEASURED and
    LANDING_MEASURED record."""
    ec = ev = 0.0
    for shape in DENOISE_SHAPES:
        for squarings in DENOISE_SQUARINGS:
            for iterations in DENOISE_ITERATIONS:
                for demodulate in (0, 1):
                    e = denoise_errors(rule_denoise, synthetic(*shape), demodulate, iterations=iterations,
                                       normal_squarings=squarings)[3:]
                    print(shape, squarings, iterations, demodulate, "colour %.4g variance %.4g" % e)
                    ec, ev = max(ec, e[0]), max(ev, e[1])
    print("denoise_rule against denoise_truth: colour %.4g, variance %.4g" % (ec, ev))
    worst = 0.0
    for shape in LANDING_SHAPES:
        for move in LANDING_MOVES:
            qualifies, free, err, _ = landing_errors(rule_chain, *shape, move, LANDING_M)
            print(shape, move, "%.3f qualify; worst %.5f px, not snapped %.3g px" % (
                qualifies.mean(), err[qualifies].max(), err[free].max()))
            worst = max(worst, float(err[free].max()))
    print("accumulate_rule against landing_truth, not snapped: %.4g px" % worst)


if __name__ == "__main__":
    measure()
