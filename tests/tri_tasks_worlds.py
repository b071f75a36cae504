"""Worlds for the per-triangle candidate tests of the culled list scan (tests/test_gpu_tri_tasks.py,
tests/test_tri_tasks_host.py, tests/tri_tasks_check.py).  Each `fill(b)` works on a product or an oracle builder.

The culled scan is on from four pairs up (kCullMinPairs), so every world that has fewer of its own carries four small
filler parallelograms BEHIND the camera: no camera ray comes near them, so the task counts below are the sheets' alone.
A wave's lane tests its first candidate from its own registers and hands the rest over as (ray, pair) tasks, two
triangle tests each: a full wave in front of n sheets flushes 64 (n - 1) pair tasks = 128 (n - 1) triangle tests.
"""
import numpy as np

PI_D = 3.14159265358979323846


def v3(x, y, z):
    return np.array([x, y, z], dtype=np.float32)


def _camera(b):
    b.camera_pinhole(v3(0, 0, 4), v3(0, 0, 0), v3(0, 1, 0), PI_D / 4, 1.0)


def _fillers(b, m):
    for i in range(4):
        x = np.float32(-1.5 + i)
        b.parallelogram([v3(x, -0.25, 9), v3(x + 0.5, -0.25, 9), v3(x, 0.25, 9.125)], m)


def sheets(n, light=False):
    """n parallel parallelograms across the whole view, one behind the other: every one is a candidate of every camera
    ray.  All but the last are glass, so that paths go on from sheet to sheet, and the last is a fuzzy mirror that sends
    them back through the stack from behind.  With `light` the last is glass too and an emitter as large as the sheets
    closes the stack behind it: one more candidate pair of every ray (64 n pair tasks), and paths that end on it."""
    def fill(b):
        _camera(b)
        grey = b.lambertian(v3(0.7, 0.7, 0.7))
        glass, mirror = b.dielectric(v3(1, 1, 1), 1.5), b.metal(v3(0.8, 0.8, 0.9), 0.3)
        b.sky()
        _fillers(b, grey)
        for i in range(n):
            z = np.float32(-0.375 * i)
            # (not axis-aligned in x / y: the two triangles' shared edge crosses the frame, both get hits)
            b.parallelogram([v3(-3, -3.5, z), v3(3.5, -3, z), v3(-3.5, 3, z)], glass if light or i < n - 1 else mirror)
        if light:
            z = np.float32(-0.375 * n)
            b.parallelogram([v3(-3.5, -3.5, z), v3(3.5, -3.5, z), v3(-3.5, 3.5, z)], b.diffuse_light(b.constant_texture(v3(4, 4, 4))))
    return fill


def mixed_list(entries=7):
    """Lone Triangles and Parallelograms in turn, overlapping in the view: an odd number of entries, so that absent
    second records sit at odd task positions and at the end of a round."""
    def fill(b):
        _camera(b)
        mats = [b.lambertian(v3(0.8, 0.4, 0.3)), b.metal(v3(0.9, 0.9, 0.9), 0.1), b.dielectric(v3(1, 1, 1), 1.4)]
        b.sky()
        for i in range(entries):
            z = np.float32(-0.25 * i)
            s = np.float32(0.125 * i)
            if i % 2 == 0:
                b.triangle([v3(-3 + s, -3, z), v3(3.5, -2.5 + s, z), v3(-0.5 - s, 3.5, z)], mats[(i + 2) % 3])
            else:
                b.parallelogram([v3(-3, -3 + s, z), v3(3 - s, -3.25, z), v3(-3.25, 3 - s, z + np.float32(0.0625))], mats[(i + 2) % 3])
    return fill


def spheres_and_pairs(b):
    """Spheres make the running bound binary64: the ray record of a task carries a double."""
    sheets(5, light=True)(b)
    b.sphere(v3(0.5, 0.25, 1.0), 0.5, b.dielectric(v3(1, 1, 1), 1.5))
    b.sphere(v3(-0.75, -0.5, 0.75), 0.375, b.metal(v3(0.9, 0.7, 0.5), 0.0))


def long_list(n_pairs, seed=3):
    """More pairs than the LDS staging holds (kLdsPairs = 128): the records are gathered from global memory."""
    def fill(b):
        rng = np.random.default_rng(seed + n_pairs)
        _camera(b)
        mats = [b.lambertian(v3(0.8, 0.8, 0.8)), b.metal(v3(0.9, 0.9, 0.9), 0.0), b.dielectric(v3(1, 1, 1), 1.5)]
        b.sky()
        for i in range(n_pairs):
            c = rng.uniform(-1.5, 1.5, 3).astype(np.float32)
            e = rng.uniform(-0.9, 0.9, (2, 3)).astype(np.float32)
            P = [c, c + e[0], c + e[1]]
            if i % 3 == 0:
                b.triangle(P, mats[i % 3])
            else:
                b.parallelogram(P, mats[i % 3])
    return fill


def textured(b):
    """Image-textured parallelograms and a lone triangle, stacked: u and v of the winner come from the result words."""
    _camera(b)
    rng = np.random.default_rng(11)
    tex = b.image_texture(rng.integers(0, 256, (8, 12, 4), dtype=np.uint8))
    m = b.lambertian_tex(tex)
    plain = b.lambertian(v3(0.5, 0.5, 0.5))
    b.sky()
    for i in range(5):
        z = np.float32(-0.5 * i)
        s = np.float32(0.75 * i)
        b.parallelogram([v3(-3 + s, -3, z), v3(0.5 + s, -3, z), v3(-3 + s, 3, z + np.float32(0.25))], m if i % 2 == 0 else plain)
    b.triangle([v3(-2, -2, 0.5), v3(2, -2, 0.5), v3(0, 2, 0.25)], m)
