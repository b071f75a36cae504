"""Worlds for the pair rounds of the fast list kernels' flushes (tests/test_gpu_pair_rounds.py, tests/pair_rounds_check.py,
tests/test_pair_rounds_host.py; closest_hit.h, RUN_TRIS, step (b); pair_rounds.h).  Each `fill(b)` works on a product or
an oracle builder.

A flush of n (ray, pair) tasks is tested a pair per lane while more than 32 tasks are untested (kPairRoundMin), 64 tasks a
round, and the rest a triangle per lane: no pair round up to 32 tasks, one from 33 to 64, one and a triangle round from 65
to 96, two from 97 to 128, and so on.  The stacks below put a chosen number of tasks into the flush of an 8 x 8 frame,
which is one tile and so one wave: every surface emits and scatters nothing, so a path is its camera ray, every lane of
the wave traces one ray per sample, and a wave query is one flush.  A ray's first candidate is tested from the lane's own
registers -- the farthest sheet, which is listed first -- and each nearer sheet it reaches is one task that passes
against the bound that test left.
"""
import numpy as np

import min_fold_worlds as mf
from diffuse_worlds import CORNELL_SEED, cornell, cornell_and_an_unused_metal  # (the Cornell box, plain and with an unused metal)
from tri_tasks_worlds import PI_D, v3

F32 = np.float32
CAM_Z = 4.0
HALF = CAM_Z * np.tan(PI_D / 8)   # half the view's width in the plane z = 0: 1.657
PARTIAL = (0, 1, 15, 16, 17, 31, 32, 33, 47, 48, 63, 64)


def _camera(b):
    b.camera_pinhole(v3(0, 0, CAM_Z), v3(0, 0, 0), v3(0, 1, 0), PI_D / 4, 1.0)


def _fillers(b, m):
    """Four small pairs behind the camera: the culled scan is on from four pairs up, and no camera ray comes near them."""
    for i in range(4):
        x = F32(-1.5 + i)
        b.parallelogram([v3(x, -0.25, 9), v3(x + 0.5, -0.25, 9), v3(x, 0.25, 9.125)], m)


def _lights(b, n):
    return [b.diffuse_light(b.constant_texture(v3(0.25 + 0.125 * (k % 5), 0.125 * (k % 7), 1.0 - 0.125 * (k % 6)))) for k in range(n)]


def _cover(b, z, j, m):
    """Emitting parallelograms in the plane z that the rays of the first j pixels of the 8 x 8 frame reach, in raster
    order from the top row, and no others: the whole rows as one, the rest of the next row as a second.  Their rims lie on
    pixel borders of the view as it is at that depth (the jitter keeps a ray inside its pixel; a ray within the pair's
    padding of a rim may still become a candidate)."""
    s = (CAM_Z - z) / CAM_Z            # the view at depth z against the view at z = 0
    half, px = HALF * s, 2 * HALF * s / 8
    top = half + px                    # ray_tracing.cu:70 counts rows from h down to 1: the frame sits one pixel up
    rows, rest = divmod(j, 8)
    z = F32(z)
    if rows == 8:                      # the whole view, with a margin: no rim in sight
        b.parallelogram([v3(-6, -6.5, z), v3(6.5, -6, z), v3(-6.5, 6, z)], m)
        return
    if rows:
        b.parallelogram([v3(-2 * half, top - rows * px, z), v3(2 * half, top - rows * px, z), v3(-2 * half, 2 * half, z)], m)
    if rest:
        y1 = top - rows * px
        b.parallelogram([v3(-2 * half, y1 - px, z), v3(-half + rest * px, y1 - px, z), v3(-2 * half, y1, z)], m)


def stack(k, j=64, metal=False, lone=False):
    """k emitting layers in front of the camera, listed far to near.  The farthest comes first and spans the whole view:
    it is every ray's first candidate, tested from the lane's own registers, and its t is the bound in the ray's record.
    Each further layer is nearer than the one before and spans the first j pixels of an 8 x 8 frame, so a covered pixel's
    ray hands over k - 1 tasks that all pass against that bound and post k - 1 competing keys: the pixel has the colour of
    the nearest layer only if the smallest key wins, and the farthest layer's where no task was its ray's.  Every layer has
    a colour of its own.  metal: one metal that no primitive has -- the scene is then not of diffuse surfaces alone and
    keeps the kernels without PIN_DIFFUSE.  lone: a lone Triangle across the whole view just in front of the farthest
    layer, one more passing task of every ray, whose second record is absent: it wins where no nearer layer covers."""
    def fill(b):
        _camera(b)
        m = _lights(b, 7)
        if metal:
            b.metal(v3(0.8, 0.85, 0.88), 0.25)
        _fillers(b, m[6])
        z_far = -0.375 * k
        _cover(b, z_far, 64, m[0])
        if lone:
            z = F32(z_far + 0.125)
            b.triangle([v3(-12, -5, z), v3(12, -5, z), v3(0, 12, z)], m[5])
        for i in range(1, k):
            _cover(b, z_far + 0.375 * i, j, m[i])
    return fill


# ------------------------------------------------------------------ the ordered world, made denser
# tests/min_fold_worlds.py's world holds 3e-5 tasks of the ordered kind per ray: enough in a frame of 262,144 rays, none
# in a frame of 16 x 16.  The kind arises where a ray crosses a pair's shared edge within the rounding of u and v, so the
# same grid 16 times as far away, the camera's opening narrowed to match, holds them far more densely (about one per
# thousand rays: a few per frame, and still so few that two of them all but never meet in one lane of one flush, which
# would count as one); and the grid's upper three rows are listed twice, so that every ray hands over each of its pairs
# twice and a wave's flush holds well over 32 tasks.
FAR = 16.0
SIDE, DEPTH, SEED = 16, 8, 11


def _far(p):
    """The points p of min_fold_worlds, FAR times as far from the origin along the view axis (binary32, rounded once)."""
    along = np.asarray(p, dtype=np.float64) @ mf.W
    return (np.asarray(p, dtype=np.float64) + ((FAR - 1.0) * along)[..., None] * mf.W).astype(F32)


def far_grid():
    """The grid's first three rows: with the backdrop and listed twice they are 31 pairs, one chunk of the scan, so that
    the backdrop is every ray's only candidate tested from the lane's own registers."""
    return _far(mf.grid_points()[:15])


def far_backdrop():
    return _far(mf.backdrop_points())


def ordered_twice(b):
    centre = (FAR * mf.CENTRE3).astype(F32)
    b.camera_pinhole(v3(0, 0, 0), centre, v3(0, 0, 1), 2 * np.arctan(2.25 * mf.PITCH / (FAR * mf.CENTRE * np.sqrt(3.0))), 1.0)
    lights = _lights(b, 13)
    b.sky()
    p = far_backdrop()
    b.parallelogram([p[0], p[1], p[2]], lights[0])
    for copy in range(2):
        for k, p in enumerate(far_grid()):
            b.parallelogram([p[0], p[1], p[2]], lights[1 + (k + copy) % 12])


def ordered_tasks(O, D):
    """Over the rays O, D (n, 3) of ordered_twice: the tasks with both triangles accepted and the second nearer
    (min_fold_worlds.ordered_tasks on this world's points; every pair of the grid is listed twice)."""
    p = far_backdrop()
    hit_a, ta = mf.tri_test(p, O, D)
    hit_b, tb = mf.tri_test(np.array([p[1], p[2], (p[1] + p[2]) - p[0]]), O, D)
    t_to = np.where(hit_a, ta, np.where(hit_b, tb, F32(np.inf)))
    n = 0
    for q in far_grid():
        n += int(mf.both_accept(q, O, D, t_to)[1].sum())
    return 2 * n
