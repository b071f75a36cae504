"""What the rtmi_bounce / rtmi_path_fold tests share: the fold and Sky's Emit restated in numpy, the raw-camera bridge to
the oracle's Trace (the oracle has no Trace-on-a-ray entry: a raw camera with zero spans gives one), the ray sample of a
query world, and the device calls.  No test lives here."""
import ctypes as C
import functools

import numpy as np

import oraclelib
from querylib import build, glm_normalize, make_rays

F0 = np.float32(0)
F1 = np.float32(1)


# ------------------------------------------------------------------ the fold (ray_tracing.cu:50-52)
def fold(dirs, steps, E, A, layers=None):
    """rtmi_path_fold in binary32: dirs (n, 3), steps (n,), E / A (L, n, 3).  c = min(steps, layers); c == 0: 0; a zero
    direction (the path ended): r = E[c-1], then r = E[k] + A[k] * r for k = c-2 .. 0; else r = 0 and k = c-1 .. 0.
    Product and sum are separate binary32 operations."""
    dirs = np.asarray(dirs, dtype=np.float32)
    E, A = np.asarray(E, dtype=np.float32), np.asarray(A, dtype=np.float32)
    layers = E.shape[0] if layers is None else int(layers)
    n = dirs.shape[0]
    out = np.zeros((n, 3), dtype=np.float32)
    with np.errstate(all="ignore"):
        for i in range(n):
            c = min(int(steps[i]), layers)
            r = np.zeros(3, dtype=np.float32)
            k = c - 1
            if c > 0 and not dirs[i].any():  # (-0.0 counts as zero)
                r = E[k, i].copy()
                k -= 1
            while k >= 0:
                r = (E[k, i] + (A[k, i] * r).astype(np.float32)).astype(np.float32)
                k -= 1
            out[i] = r
    return out


# ------------------------------------------------------------------ Sky's Emit (sky.cu:9-14)
def sky_emit(p):
    """dir = normalize(p); float t = 0.5 * (dir.y + 1.0) in binary64; (1.0f - t) * (1, 1, 1) + t * (0.5, 0.7, 1.0) in
    binary32.  p (n, 3) float32."""
    d = glm_normalize(np.asarray(p, dtype=np.float32).reshape(-1, 3))
    t = (0.5 * (d[:, 1].astype(np.float64) + 1.0)).astype(np.float32)
    w = (F1 - t).astype(np.float32)
    cols = [((w * F1).astype(np.float32) + (t * np.float32(c)).astype(np.float32)).astype(np.float32) for c in (0.5, 0.7, 1.0)]
    return np.stack(cols, axis=1)


def hit_point(o, d, t):
    """ray.position() + (float)record.t * ray.direction() in binary32 (ray_tracing.cu:32); d is Ray's unit direction."""
    return (o + (np.float32(t) * d).astype(np.float32)).astype(np.float32)


# ------------------------------------------------------------------ the raw-camera bridge
def raw_camera(ob, o, d):
    """Point the oracle's raw camera along the ray; returns the direction RayAt normalised once."""
    org, d = np.asarray(o, dtype=np.float32), np.asarray(d, dtype=np.float32)
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


def usable(O, D):
    """Rays whose raw-camera direction is a finite non-zero vector (o + d may round back onto o)."""
    llc = (O + D).astype(np.float32)
    v = ((llc + F0) + F0).astype(np.float32) - O
    with np.errstate(all="ignore"):
        u = glm_normalize(v)
    return np.isfinite(u).all(1) & (np.abs(u).sum(1) > 0)


def oracle_trace(ob, O, D, states, depth):
    """The oracle's Trace of ray i from states[i] (n, 6), a 1 x 1 render through the raw camera: (radiance (n, 3), queries
    (n,), final states (n, 6), the directions to hand to the device (n, 3), the states to hand to it (n, 6))."""
    n = len(O)
    rgb = np.zeros((n, 3), dtype=np.float32)
    rays = np.zeros(n, dtype=np.uint32)
    fin = np.zeros((n, 6), dtype=np.uint32)
    dirs = np.zeros((n, 3), dtype=np.float32)
    for i in range(n):
        dirs[i] = raw_camera(ob, O[i], D[i])
        c, r, st, _ = ob.render(1, 1, 1, depth, post=False, states=states[i:i + 1].copy(), threads=1)
        rgb[i], rays[i], fin[i] = c.reshape(3), r.reshape(()), st[0]
    return rgb, rays, fin, dirs, advance_two(states)


# ------------------------------------------------------------------ a world and its rays
@functools.lru_cache(maxsize=None)
def world(name, n=256):
    """(scene, recorder, oracle builder, seed, O, D, Dn) of a query world: n rays picked as the trace tests pick them,
    half of them (where the world has as many) rays whose first query hits a surface.  (O, D) is what the raw camera is
    pointed along; Dn is what its RayAt makes of D (normalised once): the direction to hand to the device."""
    import torch
    import rtmi
    b, rec, ob, seed = build(name)
    O, D = make_rays(ob, 3000 + len(name))
    ok = usable(O, D)
    kind = b.intersect(torch.from_numpy(O).cuda(), torch.from_numpy(D).cuda()).check().kind.cpu().numpy()
    solid = np.flatnonzero(ok & (kind != rtmi.RTMI_HIT_NONE) & (kind != rtmi.RTMI_HIT_SKY))
    rest = np.setdiff1d(np.flatnonzero(ok), solid)
    rng = np.random.default_rng(seed + 11)
    pick = rng.choice(solid, min(n // 2, len(solid)), replace=False)
    pick = np.concatenate([pick, rng.choice(rest, min(n - len(pick), len(rest)), replace=False)])
    O, D = O[pick], D[pick]
    llc = (O + D).astype(np.float32)
    Dn = glm_normalize(((llc + F0) + F0).astype(np.float32) - O)
    return b, rec, ob, seed, np.ascontiguousarray(O), np.ascontiguousarray(D), np.ascontiguousarray(Dn)


# ------------------------------------------------------------------ device calls
def dev_states(states):
    """(n, 6) uint32 numpy -> the (6, n) int32 CUDA tensor the entries read."""
    import torch
    return torch.from_numpy(np.ascontiguousarray(np.asarray(states, dtype=np.uint32).T).view(np.int32)).cuda()


def host_states(st):
    return np.ascontiguousarray(st.cpu().numpy().view(np.uint32).T)


def dev(a, dtype=np.float32):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a, dtype=dtype)).cuda()
