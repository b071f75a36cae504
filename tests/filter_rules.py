"""rtmi_denoise, rtmi_resolve_variance and rtmi_accumulate restated in numpy, operation by operation in binary32, with the
cameras and the synthetic room the accumulate tests move through.  tests/test_denoise_host.py and
tests/test_accumulate_host.py work the rules by hand, tests/filters_truth.py holds them to binary64, the GPU tests hold
the device to them."""
import ctypes as C

import numpy as np

import rtmi

try:
    import torch
except ImportError:  # the rules are host code; only `run` needs a device
    torch = None

F32 = np.float32

H5 = [F32(1) / F32(16), F32(1) / F32(4), F32(3) / F32(8), F32(1) / F32(4), F32(1) / F32(16)]

MIN_WEIGHT_SUM = F32(2.0 ** -32)  # a pass filters a pixel only from this sum of weights on: below it sw * sw leaves the normals


# ------------------------------------------------------------------ the rules, restated
def falloff(x):
    m = np.fmax(F32(1) - F32(0.25) * x, F32(0))
    m2 = m * m
    return m2 * m2


def variance_rule(n, S, Q, pixel=None):
    """rtmi_resolve_variance in numpy, operation by operation as include/rtmi.h states it.  n (N,) uint32, S, Q (N, 3)
    float32, pixel (N,) bool (False: padding).  Returns (N, 3) float32."""
    n = np.asarray(n, dtype=np.uint32)
    S, Q = np.asarray(S, dtype=F32), np.asarray(Q, dtype=F32)
    if pixel is not None:
        n = np.where(np.asarray(pixel, dtype=bool), n, 0).astype(np.uint32)
    with np.errstate(all="ignore"):
        nf = n.astype(F32)[:, None]
        a = nf * Q
        b = S * S
        c = np.fmax(a - b, F32(0))
        d = nf * nf
        e = nf - F32(1)
        many = c / (d * e)
    for x in (a, b, c, d, e, many):
        assert x.dtype == F32
    n = n[:, None]
    return np.where(n == 0, F32(0), np.where(n == 1, b, many)).astype(F32)


def denoise_rule(color, variance, normal, depth, alpha, albedo=None, iterations=rtmi.DENOISE_DEFAULTS["iterations"],
                 sigma_color=rtmi.DENOISE_DEFAULTS["sigma_color"], sigma_depth=rtmi.DENOISE_DEFAULTS["sigma_depth"],
                 normal_squarings=rtmi.DENOISE_DEFAULTS["normal_squarings"], demodulate=None, decisions=None):
    """rtmi_denoise in numpy, operation by operation as include/rtmi.h states it: float32 throughout, vectorised over the
    image, the 25 taps in the stated order.  color, variance, normal, albedo (H, W, 3), depth, alpha (H, W).  Returns
    (out, out_variance), both (H, W, 3) float32.  decisions: a list that receives, per pass, the (H, W) bool array of the
    pixels the pass filtered (the others kept their value)."""
    C0, V0, N, Z, A = (np.asarray(x, dtype=F32) for x in (color, variance, normal, depth, alpha))
    demodulate = (albedo is not None) if demodulate is None else bool(demodulate)
    H, W = Z.shape
    sc2 = F32(sigma_color) * F32(sigma_color)
    sz = F32(sigma_depth)
    with np.errstate(all="ignore"):
        if demodulate:
            ad = np.fmax(np.asarray(albedo, dtype=F32), F32(0.01))
            Cc, V = C0 / ad, V0 / (ad * ad)
        else:
            Cc, V = C0.copy(), V0.copy()
        surf = A > 0
        I, J = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
        zden = sz * Z + F32(1e-6)
        for k in range(iterations):
            s = 1 << k
            vsum = (V[..., 0] + V[..., 1]) + V[..., 2]
            sw = np.zeros((H, W), F32)
            sc, sv = np.zeros((H, W, 3), F32), np.zeros((H, W, 3), F32)
            for dy in range(-2, 3):
                for dx in range(-2, 3):
                    qi, qj = I + dy * s, J + dx * s
                    inside = (qi >= 0) & (qi < H) & (qj >= 0) & (qj < W)
                    ci, cj = np.clip(qi, 0, H - 1), np.clip(qj, 0, W - 1)  # (gathered, then not taken)
                    Nq, Zq, Cq, Vq, surf_q = N[ci, cj], Z[ci, cj], Cc[ci, cj], V[ci, cj], surf[ci, cj]
                    take = inside & (surf == surf_q)
                    d = np.fmax((N[..., 0] * Nq[..., 0] + N[..., 1] * Nq[..., 1]) + N[..., 2] * Nq[..., 2], F32(0))
                    wn = d
                    for _ in range(normal_squarings):
                        wn = wn * wn
                    wz = falloff(np.abs(Z - Zq) / zden)
                    wn, wz = np.where(surf, wn, F32(1)), np.where(surf, wz, F32(1))
                    diff = Cc - Cq
                    d2 = (diff[..., 0] * diff[..., 0] + diff[..., 1] * diff[..., 1]) + diff[..., 2] * diff[..., 2]
                    vs = vsum + vsum[ci, cj]
                    wc = falloff(d2 / (sc2 * vs + F32(1e-10)))
                    w = (((H5[dy + 2] * H5[dx + 2]) * wn) * wz) * wc
                    for x in (d, wn, wz, d2, vs, wc, w):
                        assert x.dtype == F32
                    sw = np.where(take, sw + w, sw)
                    sc = np.where(take[..., None], sc + w[..., None] * Cq, sc)
                    sv = np.where(take[..., None], sv + (w * w)[..., None] * Vq, sv)
            ok = (sw >= MIN_WEIGHT_SUM)[..., None]
            if decisions is not None:
                decisions.append(ok[..., 0])
            Cc, V = np.where(ok, sc / sw[..., None], Cc), np.where(ok, sv / (sw * sw)[..., None], V)
            assert Cc.dtype == F32 and V.dtype == F32
        if demodulate:
            Cc, V = Cc * ad, V * (ad * ad)
    return Cc.astype(F32), V.astype(F32)


def on_gpu(d):
    return {k: torch.from_numpy(np.ascontiguousarray(v)).cuda() for k, v in d.items()}


def run(d, demodulate, **opts):
    """rtmi.denoise on the inputs of dict d (numpy) -> (out, out_variance) as numpy."""
    t = on_gpu(d)
    if not demodulate:
        t.pop("albedo")
    out, var = rtmi.denoise(**t, return_variance=True, **opts)
    torch.cuda.synchronize()
    return out.cpu().numpy(), var.cpu().numpy()

BRANCHES = ("background", "behind", "off_screen", "refused", "snapped", "taps_1_3", "taps_4")

SHAPES = [(1, 1), (3, 70), (70, 3), (16, 16), (33, 70)]


# ------------------------------------------------------------------ the rule, restated
def camera_terms(cur, prev):
    """The host part of the rule in Python floats (binary64) from the cameras' binary32 values: (e, R, singular)."""
    cur = np.asarray(cur, dtype=F32).reshape(-1)
    e = np.array([float(cur[3 + k]) - float(cur[k]) for k in range(3)]).astype(F32)
    if prev is None:
        return e, None, False
    prev = np.asarray(prev, dtype=F32).reshape(-1)
    a = [float(prev[6 + k]) for k in range(3)]
    b = [float(prev[9 + k]) for k in range(3)]
    c = [float(prev[3 + k]) - float(prev[k]) for k in range(3)]
    cross = lambda x, y: [x[1] * y[2] - x[2] * y[1], x[2] * y[0] - x[0] * y[2], x[0] * y[1] - x[1] * y[0]]
    rows = [cross(b, c), cross(c, a), cross(a, b)]
    det = (a[0] * rows[0][0] + a[1] * rows[0][1]) + a[2] * rows[0][2]
    if det == 0.0 or not np.isfinite(det):
        return e, None, True
    return e, np.array([[x / det for x in row] for row in rows]).astype(F32), False


def accumulate_rule(color, variance, normal, depth, alpha, camera, history=None, prev_camera=None,
                    normal_min=rtmi.ACCUMULATE_DEFAULTS["normal_min"], depth_tolerance=rtmi.ACCUMULATE_DEFAULTS["depth_tolerance"],
                    min_blend=rtmi.ACCUMULATE_DEFAULTS["min_blend"]):
    """rtmi_accumulate in numpy, operation by operation as include/rtmi.h states it: float32 throughout on the device side,
    vectorised over the image, the four taps in the stated order.  color, variance, normal (H, W, 3), depth, alpha (H, W);
    history (3, H, W, 4) float32 -- the planes G, C, V of the device's history, byte for byte -- or None.  Returns (out,
    out_variance, out_length, history_out, shares): shares maps each name of BRANCHES to the share of pixels that took
    it (all 0 but background without a history)."""
    Cp, Vp, N, Z, A = (np.asarray(x, dtype=F32) for x in (color, variance, normal, depth, alpha))
    H, W = Z.shape
    assert (history is None) == (prev_camera is None)
    surf = A > 0
    I, J = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    out, var, length = Cp.copy(), Vp.copy(), np.ones((H, W), F32)
    which = np.where(surf, "none", "background")
    if history is not None:
        hist = np.asarray(history, dtype=F32).reshape(3, H, W, 4)
        cur = np.asarray(camera, dtype=F32).reshape(-1)
        e, R, singular = camera_terms(camera, prev_camera)
        assert not singular
        p, h, v, pp = cur[0:3], cur[6:9], cur[9:12], np.asarray(prev_camera, dtype=F32).reshape(-1)[0:3]
        nm, dt, mb = F32(normal_min), F32(depth_tolerance), F32(min_blend)
        Wf, Hf = F32(W), F32(H)
        with np.errstate(all="ignore"):
            xf = (J.astype(F32) + F32(0.5)) / Wf
            yf = ((H - I).astype(F32) + F32(0.5)) / Hf
            D = [(e[k] + xf * h[k]) + yf * v[k] for k in range(3)]
            l = np.sqrt((D[0] * D[0] + D[1] * D[1]) + D[2] * D[2])
            d = [(p[k] + (D[k] / l) * Z) - pp[k] for k in range(3)]
            al, be, ga = ((R[r][0] * d[0] + R[r][1] * d[1]) + R[r][2] * d[2] for r in range(3))
            ze = np.sqrt((d[0] * d[0] + d[1] * d[1]) + d[2] * d[2])
            fx = (al / ga) * Wf - F32(0.5)
            fy = (Hf + F32(0.5)) - (be / ga) * Hf
            for x in D + d + [xf, yf, l, al, be, ga, ze, fx, fy]:
                assert x.dtype == F32
            front = ga > 0
            inside = (fx > -1) & (fx < Wf) & (fy > -1) & (fy < Hf)
            seen = surf & front & inside
            fx, fy = np.where(seen, fx, F32(0)), np.where(seen, fy, F32(0))
            rx, ry = np.rint(fx), np.rint(fy)
            snap = (np.abs(fx - rx) <= F32(1 / 64)) & (np.abs(fy - ry) <= F32(1 / 64))
            fx, fy = np.where(snap, rx, fx), np.where(snap, ry, fy)
            flx, fly = np.floor(fx), np.floor(fy)
            j0, i0 = flx.astype(np.int64), fly.astype(np.int64)
            tx, ty = fx - flx, fy - fly
            zlim = dt * ze
            sw, sl = np.zeros((H, W), F32), np.zeros((H, W), F32)
            sc, sv = np.zeros((H, W, 3), F32), np.zeros((H, W, 3), F32)
            positive = np.zeros((H, W), np.int64)
            for di in (0, 1):
                for dj in (0, 1):
                    qi, qj = i0 + di, j0 + dj
                    ok = (qi >= 0) & (qi < H) & (qj >= 0) & (qj < W)
                    ci, cj = np.clip(qi, 0, H - 1), np.clip(qj, 0, W - 1)  # (gathered, then not taken)
                    G, Cq, Vq = hist[0][ci, cj], hist[1][ci, cj], hist[2][ci, cj]
                    b = (ty if di else F32(1) - ty) * (tx if dj else F32(1) - tx)
                    dot = (N[..., 0] * G[..., 0] + N[..., 1] * G[..., 1]) + N[..., 2] * G[..., 2]
                    take = ok & (Vq[..., 3] > 0) & (dot >= nm) & (np.abs(G[..., 3] - ze) <= zlim)
                    for x in (b, dot, zlim):
                        assert x.dtype == F32
                    sw = np.where(take, sw + b, sw)
                    sl = np.where(take, sl + b * Cq[..., 3], sl)
                    sc = np.where(take[..., None], sc + b[..., None] * Cq[..., :3], sc)
                    sv = np.where(take[..., None], sv + b[..., None] * Vq[..., :3], sv)
                    positive += take & (b > 0)
            taken = seen & (sw > 0)
            Lp = sl / sw + F32(1)
            a = np.fmax(F32(1) / Lp, mb)
            o = F32(1) - a
            Cn = o[..., None] * (sc / sw[..., None]) + a[..., None] * Cp
            Vn = (o * o)[..., None] * (sv / sw[..., None]) + (a * a)[..., None] * Vp
            for x in (sw, sl, sc, sv, Lp, a, o, Cn, Vn):
                assert x.dtype == F32
        out = np.where(taken[..., None], Cn, Cp)
        var = np.where(taken[..., None], Vn, Vp)
        length = np.where(taken, Lp, F32(1))
        which = np.where(~surf, "background", np.where(~front, "behind", np.where(~inside, "off_screen", np.where(
            ~taken, "refused", np.where(snap, "snapped", np.where(positive == 4, "taps_4", "taps_1_3"))))))
    hist_out = np.empty((3, H, W, 4), F32)
    hist_out[0, ..., :3], hist_out[0, ..., 3] = N, Z
    hist_out[1, ..., :3], hist_out[1, ..., 3] = out, length
    hist_out[2, ..., :3], hist_out[2, ..., 3] = var, surf.astype(F32)
    for x in (out, var, length):
        assert x.dtype == F32
    shares = {k: float((which == k).mean()) for k in BRANCHES}
    return out, var, length, hist_out, shares


# ------------------------------------------------------------------ a synthetic room seen from two cameras
FOV = 40.0 * np.pi / 180.0

HOME = ((278, 273, -800), (278, 273, 0))

MOVES = {"static": HOME, "slide": ((318, 283, -780), (278, 273, 0)), "pan": ((278, 273, -800), (600, 273, 0)),
         "about": ((278, 273, 200), (278, 273, -800))}


def look_at(pos, target, aspect, fov=FOV):
    """The 21 floats of the library's own pinhole camera: rtmi_camera_pinhole + rtmi_camera_get on a throw-away scene
    (neither touches the device)."""
    L = rtmi.lib()
    s = C.c_void_p(L.rtmi_scene_create())
    try:
        v = lambda x: np.asarray(x, dtype=F32).ctypes.data_as(C.POINTER(C.c_float))
        assert L.rtmi_camera_pinhole(s, v(pos), v(target), v((0, 1, 0)), fov, float(aspect)) == 0
        out = np.zeros(21, F32)
        assert L.rtmi_camera_get(s, out.ctypes.data_as(C.POINTER(C.c_float))) == 0
    finally:
        L.rtmi_scene_destroy(s)
    return out


def camera_of(move, h, w):
    return look_at(*MOVES[move], aspect=w / h)


def room(h, w, camera, seed=0):
    """A frame of a room seen from `camera`, analytic in binary64 and rounded to binary32: the planes z = 559, y = 0,
    x = 555 and y = 555, the plane x = 0 turned into background (alpha 0, depth 0, normal 0, like whatever a ray misses),
    and a box face at z = 300 for 100 < x < 300, y < 330.  Depth is t along the unit centre ray, the normals are axis unit
    vectors, colour and variance are random in [0, 1).  Returns a dict of accumulate_rule's first five arguments."""
    cam = np.asarray(camera, dtype=np.float64).reshape(-1)
    p, llc, hh, vv = cam[0:3], cam[3:6], cam[6:9], cam[9:12]
    I, J = np.meshgrid(np.arange(h), np.arange(w), indexing="ij")
    xf, yf = (J + 0.5) / w, ((h - I) + 0.5) / h
    D = (llc - p)[None, None] + xf[..., None] * hh + yf[..., None] * vv
    D = D / np.sqrt((D * D).sum(-1, keepdims=True))
    best = np.full((h, w), np.inf)
    normal = np.zeros((h, w, 3))
    surface = np.zeros((h, w), bool)
    planes = ((2, 559.0, (0, 0, -1), True), (1, 0.0, (0, 1, 0), True), (0, 555.0, (-1, 0, 0), True), (1, 555.0, (0, -1, 0), True),
              (0, 0.0, (0, 0, 0), False), (2, 300.0, (0, 0, -1), "box"))
    with np.errstate(all="ignore"):
        for axis, at, nrm, kind in planes:
            t = (at - p[axis]) / D[..., axis]
            hit = np.isfinite(t) & (t > 1e-9) & (t < best)
            if kind == "box":
                P = p + D * t[..., None]
                hit &= (P[..., 0] > 100) & (P[..., 0] < 300) & (P[..., 1] < 330)
            best = np.where(hit, t, best)
            normal[hit] = nrm
            surface = np.where(hit, bool(kind), surface)
    rng = np.random.default_rng([seed, h, w])
    d = dict(color=rng.random((h, w, 3)).astype(F32), variance=rng.random((h, w, 3)).astype(F32),
             normal=np.where(surface[..., None], normal, 0).astype(F32), depth=np.where(surface, best, 0).astype(F32),
             alpha=surface.astype(F32))
    assert all(x.dtype == F32 for x in d.values())
    return d
