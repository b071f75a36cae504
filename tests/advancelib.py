"""What the rtmi_path_advance tests share: the per-candidate rule of include/rtmi.h ("path advance") restated in numpy --
push, finish, fold, add, refill, cursor -- on the existing restatements of the fold (bouncelib.fold), of "live"
(bouncelistlib.live) and of the camera ray (the jitter of ray_tracing.cu:68-73 drawn through the oracle's generator, then
RayAt's one normalisation), and a toy step function to drive it.  tests/test_path_advance_host.py holds it to hand-worked
items.  No test lives here."""
import ctypes as C

import numpy as np

import oraclelib
from bouncelib import fold
from bouncelistlib import candidates, live
from querylib import glm_normalize

F32 = np.float32
IN_FLIGHT = 1 << 31  # bit 31 of cursor word 0 (F); the low 31 bits: samples started (k)
U32P = C.POINTER(C.c_uint32)


def draw01(state):
    """CudaRandomFloat(0, 1) from the six state words, advanced in place."""
    return float(oraclelib.lib().orc_random_float(C.c_float(0.0), C.c_float(1.0), state.ctypes.data_as(U32P)))


def camera_ray(cam, h, w, idx, state, kind="camera"):
    """rtmi_camera_rays' active item for pixel idx of an h x w frame, kinds "camera" (no defocus) and "orthographic":
    cam is the (7, 3) float32 of camera_get; state (6,) uint32 advances by the two jitter draws.  Returns (o, d)."""
    r1, r2 = draw01(state), draw01(state)
    i, j = divmod(int(idx), w)
    x = (r1 + float(j)) / float(w)
    y = (r2 + float(h - i)) / float(h)
    x, y = 2 * x - 1, 2 * y - 1
    xf, yf = F32((x + 1) / 2), F32((y + 1) / 2)
    pos, llc, horiz, vert = (cam[k].astype(F32) for k in range(4))
    target = ((llc + xf * horiz).astype(F32) + yf * vert).astype(F32)
    if kind == "orthographic":
        return target, glm_normalize(-cam[6].astype(F32))
    assert kind == "camera"
    return pos.copy(), glm_normalize((target - pos).astype(F32))


class Wavefront:
    """The arrays of one rtmi_path_advance loop, as numpy: everything indexed by work item.  states is (items, 6) uint32
    (a row per item: the transpose of the device's planes)."""

    def __init__(self, pixel_of, spp, max_depth, states, budget=None, with_sq=True, with_rays=True, with_counts=True):
        n = len(pixel_of)
        self.pixel_of, self.spp, self.max_depth, self.n = np.asarray(pixel_of), int(spp), int(max_depth), n
        self.budget = None if budget is None else np.asarray(budget).astype(np.uint32)
        self.origins, self.dirs = np.zeros((n, 3), F32), np.zeros((n, 3), F32)
        self.states = np.ascontiguousarray(states, dtype=np.uint32).copy()
        self.steps = np.zeros(n, np.uint32)
        self.emitted, self.attenuation = np.zeros((n, 3), F32), np.zeros((n, 3), F32)
        self.e_stack, self.a_stack = np.zeros((max_depth, n, 3), F32), np.zeros((max_depth, n, 3), F32)
        self.cursor = np.zeros((n, 2), np.uint32)
        self.sum = np.zeros((n, 3), F32)
        self.sq = np.zeros((n, 3), F32) if with_sq else None
        self.samples = np.zeros(n, np.uint32)
        self.ray_counts = np.zeros(n, np.uint32) if with_rays else None
        self.counts = np.zeros(3, np.int64) if with_counts else None


def advance(wf, ray_fn, list_in=None, n_list=None, count_in=None):
    """One rtmi_path_advance on the Wavefront wf, in place.  ray_fn(q, idx, state) -> (o, d) makes pixel idx's next camera
    ray from the item's state row (advancing it).  The candidates are rtmi_bounce_list's."""
    n, depth = wf.n, wf.max_depth
    with np.errstate(all="ignore"):
        for q in candidates(n, list_in, n_list, count_in):
            q = int(q)
            if q >= n:
                continue  # no work item: dropped
            idx = int(wf.pixel_of[q])
            if idx < 0:  # 1. padding
                wf.dirs[q] = 0.0
                continue
            b = min(int(wf.budget[q]) if wf.budget is not None else wf.spp, wf.spp)  # 2.
            k, P = int(wf.cursor[q, 0]) & (IN_FLIGHT - 1), int(wf.cursor[q, 1])
            F = bool(int(wf.cursor[q, 0]) & IN_FLIGHT)
            if F and int(wf.steps[q]) == (P + 1) & 0xffffffff:  # 3. push
                if P < depth:
                    wf.e_stack[P, q], wf.a_stack[P, q] = wf.emitted[q], wf.attenuation[q]
                P = (P + 1) & 0xffffffff
            for _ in range(b - k + 1 if k <= b else 1):  # 4.
                if F:  # finish
                    st = int(wf.steps[q])
                    alive = bool(live(wf.origins[q:q + 1], wf.dirs[q:q + 1])[0])
                    if alive and st < depth:
                        break
                    c = min(st, depth)
                    scattered = bool((wf.dirs[q] != 0).any())  # (-0.0 counts as zero)
                    x = np.zeros(3, F32)
                    if c > 0:
                        x = fold(wf.dirs[q:q + 1], [c], wf.e_stack[:, q:q + 1], wf.a_stack[:, q:q + 1], layers=c)[0]
                    queries = 0 if (c == 0 and not alive) else c + (1 if scattered else 0)
                    wf.sum[q] = (wf.sum[q] + x).astype(F32)
                    if wf.sq is not None:
                        wf.sq[q] = (wf.sq[q] + (x * x).astype(F32)).astype(F32)
                    wf.samples[q] += np.uint32(1)
                    if wf.ray_counts is not None:
                        wf.ray_counts[q] = np.uint32((int(wf.ray_counts[q]) + queries) & 0xffffffff)
                    if wf.counts is not None:
                        wf.counts[0] += 1
                        wf.counts[1] += queries
                    F = False
                if k < b:  # refill
                    wf.origins[q], wf.dirs[q] = ray_fn(q, idx, wf.states[q])
                    wf.steps[q], P, k, F = 0, 0, k + 1, True
                    if wf.counts is not None:
                        wf.counts[2] += 1
                else:
                    wf.dirs[q] = 0.0
                    break
            wf.cursor[q] = ((IN_FLIGHT if F else 0) | k, P)  # 5.


def toy_step(wf, q, ends, emitted, attenuation, direction=(0.0, 0.0, 1.0)):
    """What an rtmi_bounce_list does to a listed live path q, by fiat: its one layer is written, its step count goes up,
    and its direction becomes `direction` -- or the zero vector if the path `ends` here."""
    wf.emitted[q], wf.attenuation[q] = np.asarray(emitted, F32), np.asarray(attenuation, F32)
    wf.steps[q] += np.uint32(1)
    wf.dirs[q] = 0.0 if ends else np.asarray(direction, F32)


def live_items(wf, among=None):
    """rtmi_path_compact over the wavefront's rays: the live candidates, ascending for the identity."""
    c = np.arange(wf.n) if among is None else np.asarray(among, dtype=np.int64)
    c = c[c < wf.n]
    return c[live(wf.origins, wf.dirs)[c]]
