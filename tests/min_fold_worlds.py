"""The world and the host restatements for the fast list kernels' fold by minimum (tests/test_gpu_min_fold.py,
tests/test_min_fold_host.py, tests/min_fold_check.py; closest_hit.h, RUN_TRIS, steps (b) and (c)).

A flush of the culled scan's shared tests is folded by one LDS minimum per ray unless one of its (ray, pair) tasks had
BOTH triangles pass with the second one nearer: the one case whose answer depends on the running bound at the pair's turn
(DESIGN.md 2.1).  That flush is redone in list order and its tasks are counted in rtmi_debug_counters' word 16.  Both
triangles pass only where a ray crosses the pair's shared edge within the rounding of u and v, so `ordered_world` makes
that rounding large against the pairs: parallelograms a quarter unit in size at coordinates near 1,000, tilted, seen from
the origin, in front of a backdrop that is listed first.  A lane tests its first candidate -- the backdrop -- from its own
registers, so every ray's pair of the grid is a shared task.  Every surface emits and scatters nothing: a path is its camera ray, a sample
draws the two numbers of its jitter and no more, and so the host knows every ray of the frame (primary_rays).

tri_test and both_accept restate utils.cu:49-85 and parallelogram.cu:10-33 in numpy binary32, one rounding per operation
in the reference's order (no contraction); the XORWOW draws are tests/test_oracle_rng.py's recurrence, vectorised."""
import numpy as np

import oraclelib
from querylib import glm_normalize
from tri_tasks_worlds import v3

F32 = np.float32
GRID = 5               # GRID x GRID parallelograms and the backdrop: 26 pairs, one chunk of the scan
CENTRE = 1000.0
PITCH = 0.25           # of the grid; a parallelogram is 1.0625 of it wide
ORDERED_WORD = 16      # rtmi_debug_counters (include/rtmi.h)
SIDE, SPP, DEPTH, SEED = 128, 16, 8, 11


# The camera sits at the origin and looks along (1, 1, 1) at the grid's centre, 1,732 units away: o - p0 is then about
# 1,000 in every component, each product of the tests' dot products carries an error of about 6e-5, and their sum, u or
# v, is of order one.  U, V span the grid's plane (they are the camera's own axes up to sign), W points away from the camera.
U = np.array([1.0, -1.0, 0.0]) / np.sqrt(2.0)
V = np.array([1.0, 1.0, -2.0]) / np.sqrt(6.0)
W = np.array([1.0, 1.0, 1.0]) / np.sqrt(3.0)
CENTRE3 = np.array([CENTRE, CENTRE, CENTRE])


def grid_points(seed=5):
    """(GRID * GRID, 3, 3) float32: p0, p1, p2 of the tilted parallelograms, row by row.  Each is 1.0625 pitches wide,
    turned in the grid's plane and tilted out of it by up to 0.25 per unit, so neighbours overlap in the view."""
    rng = np.random.default_rng(seed)
    P = np.zeros((GRID * GRID, 3, 3), dtype=F32)
    for k in range(GRID * GRID):
        i, j = divmod(k, GRID)
        a = rng.uniform(-0.2, 0.2)
        tw = rng.uniform(-0.25, 0.25, 2)
        p0 = CENTRE3 + PITCH * ((j - GRID / 2 - 0.03125) * U + (i - GRID / 2 - 0.03125) * V + rng.uniform(-0.5, 0.5) * W)
        e1 = PITCH * 1.0625 * (np.cos(a) * U + np.sin(a) * V + tw[0] * W)
        e2 = PITCH * 1.0625 * (-np.sin(a) * U + np.cos(a) * V + tw[1] * W)
        P[k] = np.array([p0, p0 + e1, p0 + e2]).astype(F32)
    return P


def backdrop_points():
    """(3, 3) float32: 20 x 20 units, 5 behind the grid."""
    p0 = CENTRE3 + 5 * W - 10 * U - 10 * V
    return np.array([p0, p0 + 20 * U, p0 + 20 * V]).astype(F32)


def ordered_world(b, aspect=1.0):
    """fill(b) for a product or an oracle builder."""
    # the grid's 5 x 5 pitches fill the frame with a margin: half the view is 2.25 pitches wide at its distance
    b.camera_pinhole(v3(0, 0, 0), CENTRE3.astype(F32), v3(0, 0, 1), 2 * np.arctan(2.25 * PITCH / (CENTRE * np.sqrt(3.0))), aspect)
    lights = [b.diffuse_light(b.constant_texture(v3(0.25 + 0.125 * (k % 5), 0.125 * (k % 7), 1.0 - 0.125 * (k % 6)))) for k in range(13)]
    b.sky()
    p = backdrop_points()
    b.parallelogram([p[0], p[1], p[2]], lights[0])
    for k, p in enumerate(grid_points()):
        b.parallelogram([p[0], p[1], p[2]], lights[1 + k % 12])


# ------------------------------------------------------------------ the two triangle tests in binary32
def _cross(a, b):
    return np.stack([a[..., 1] * b[..., 2] - b[..., 1] * a[..., 2], a[..., 2] * b[..., 0] - b[..., 2] * a[..., 0],
                     a[..., 0] * b[..., 1] - b[..., 0] * a[..., 1]], axis=-1)


def _dot(a, b):
    return (a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]) + a[..., 2] * b[..., 2]


def tri_test(p, o, d, t_to=np.inf):
    """TriangleHit (utils.cu:49-85) of the triangle p (3, 3) for rays o, d (n, 3), all float32, against [1e-3, t_to]:
    (accepted (n,) bool, t (n,) float32)."""
    p, o, d = (np.asarray(x, dtype=F32) for x in (p, o, d))
    with np.errstate(all="ignore"):
        e1, e2 = p[1] - p[0], p[2] - p[0]
        pvec = _cross(d, e2[None, :])
        det = _dot(e1[None, :], pvec)
        ok = ~(np.abs(det).astype(np.float64) < 1e-7)
        inv = F32(1) / det
        tvec = o - p[0][None, :]
        u = _dot(tvec, pvec) * inv
        ok &= ~((u < 0) | (u > 1))
        qvec = _cross(tvec, e1[None, :])
        v = _dot(d, qvec) * inv
        ok &= ~((v < 0) | (u + v > 1))
        t = _dot(e2[None, :], qvec) * inv
        ok &= (1e-3 <= t.astype(np.float64)) & (t.astype(np.float64) <= np.asarray(t_to, dtype=np.float64))
    assert all(x.dtype == F32 for x in (det, inv, u, v, t))
    return ok, t


def both_accept(p, o, d, t_to=np.inf):
    """The parallelogram p0, p1, p2 (parallelogram.cu:10-15: its triangles are (p0, p1, p2) and (p1, p2, p1 + p2 - p0))
    against the same bound: (both accepted, and the second's t below the first's)."""
    p = np.asarray(p, dtype=F32)
    p3 = (p[1] + p[2]) - p[0]
    hit_a, ta = tri_test(p, o, d, t_to)
    hit_b, tb = tri_test(np.array([p[1], p[2], p3]), o, d, t_to)
    both = hit_a & hit_b
    return both, both & (tb < ta)


# ------------------------------------------------------------------ every camera ray of a frame whose paths draw nothing
def _draw(st):
    """One XORWOW step of the states (n, 6) uint32 {d, v0..v4}, in place; curand_uniform of the result as float32."""
    t = st[:, 1] ^ (st[:, 1] >> np.uint32(2))
    st[:, 1:5] = st[:, 2:6]
    st[:, 5] = (st[:, 5] ^ (st[:, 5] << np.uint32(4))) ^ (t ^ (t << np.uint32(1)))
    st[:, 0] += np.uint32(362437)
    x = st[:, 5] + st[:, 0]
    return x.astype(F32) * F32(2.0 ** -32) + F32(2.0 ** -33)


def primary_rays(cam, h, w, spp, seed):
    """Origins and unit directions (spp, h * w, 3) float32 of the camera rays rtmi_camera_rays forms for samples
    0..spp-1 of a pinhole frame whose paths make no draws of their own: ray_tracing.cu:68-73 and camera.cu's RayAt as
    tests/test_gpu_camera_rays.py restates them (x and y in binary64, rounded once), and the states after them."""
    pos, llc, horiz, vert = (np.asarray(cam[k], dtype=F32) for k in range(4))
    st = oraclelib.rng_init(seed, h * w)
    i, j = np.divmod(np.arange(h * w), w)
    O = np.broadcast_to(pos, (spp, h * w, 3)).copy()
    D = np.zeros((spp, h * w, 3), dtype=F32)
    for s in range(spp):
        r1, r2 = _draw(st).astype(np.float64), _draw(st).astype(np.float64)
        x, y = 2 * ((r1 + j) / float(w)) - 1, 2 * ((r2 + (h - i)) / float(h)) - 1
        xf, yf = ((x + 1) / 2).astype(F32), ((y + 1) / 2).astype(F32)
        target = ((llc[None, :] + xf[:, None] * horiz[None, :]).astype(F32) + yf[:, None] * vert[None, :]).astype(F32)
        D[s] = glm_normalize(glm_normalize(target - pos[None, :]))  # (RayAt normalises, and so does the Ray it returns)
    return O, D, st


def ordered_tasks(O, D):
    """Over the rays O, D (n, 3) of the ordered world: (tasks with both triangles accepted and the second nearer, tasks
    with both accepted, rays that hit the backdrop).  The backdrop is every ray's first candidate, tested from the lane's
    own registers; the bound that test leaves is the tasks' t0_to (a ray in the rounding's gap along the backdrop's own
    shared edge misses both triangles and keeps +inf)."""
    p = backdrop_points()
    hit_a, ta = tri_test(p, O, D)
    hit_b, tb = tri_test(np.array([p[1], p[2], (p[1] + p[2]) - p[0]]), O, D)
    t_to = np.where(hit_a, ta, np.where(hit_b, tb, F32(np.inf)))
    n = both = 0
    for q in grid_points():
        b, s = both_accept(q, O, D, t_to)
        both, n = both + int(b.sum()), n + int(s.sum())
    return n, both, int((hit_a | hit_b).sum())


def frame_rays(cam):
    """Every ray of the frame SIDE x SIDE x SPP, flat."""
    O, D, _ = primary_rays(cam, SIDE, SIDE, SPP, SEED)
    return O.reshape(-1, 3), D.reshape(-1, 3)
