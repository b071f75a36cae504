"""Worlds for the trimmed fast list kernels (tests/test_gpu_fast_trim.py; render_body.h: the radiance fold's colour table,
closest_hit.h: load_tri_pts).  Each `fill(b)` works on a product or an oracle builder.

The fold of the kernels compiled for the common list frame reads a layer's colour from a table of 16 rows, one per value
a nibble of the id stack can take.  `box(16)` is a room whose sixteen surfaces have a material each, every one of them
scattering, with 48 colour components that are all different: a wrong row, or a row of another material's, changes the
image.  Sixteen scatterers leave no id for an emitter, so the light is the sky's, through a slot in the ceiling (the sky
is an entry of the world list, not a material).  `box(17)` puts a seventeenth material on a plinth: nibbles no longer
hold its ids and the launch must be the general kernel's.  `full_list()` fills the room with small parallelograms and lone
triangles up to kLdsPairs pairs, the longest list whose records are staged and the largest record addresses."""
import numpy as np

from tri_tasks_worlds import v3

PI_D = 3.14159265358979323846
LDS_PAIRS = 128  # kLdsPairs (scene_dev.h), restated
SIZE = 4.0


def colour(k):
    """Material k's colour: components 0.30 + (3 k + j) / 80, all different for k < 17."""
    return v3(*(0.30 + (3 * k + j) / 80.0 for j in range(3)))


def _strips(n, lo, hi):
    e = np.linspace(lo, hi, n + 1)
    return [(np.float32(e[i]), np.float32(e[i + 1])) for i in range(n)]


def _materials(b, n):
    # two mirrors among the Lambertians: a layer's colour is its material's whatever it does with the direction
    return [b.metal(colour(k), 0.0 if k == 5 else 0.25) if k in (5, 11) else b.lambertian(colour(k)) for k in range(n)]


def _room(b, m):
    """Sixteen parallelograms around [0, SIZE]^3, a slot 0.5 wide in the ceiling; m: sixteen materials."""
    S = np.float32(SIZE)
    k = 0
    for x0, x1 in _strips(3, 0, SIZE):  # floor
        b.parallelogram([v3(x0, 0, 0), v3(x1, 0, 0), v3(x0, 0, S)], m[k]); k += 1
    for x0, x1 in ((np.float32(0), np.float32(1.75)), (np.float32(2.25), S)):  # ceiling, open between 1.75 and 2.25
        b.parallelogram([v3(x0, S, 0), v3(x1, S, 0), v3(x0, S, S)], m[k]); k += 1
    for x0, x1 in _strips(3, 0, SIZE):  # back wall
        b.parallelogram([v3(x0, 0, S), v3(x1, 0, S), v3(x0, S, S)], m[k]); k += 1
    for z0, z1 in _strips(3, 0, SIZE):  # left wall
        b.parallelogram([v3(0, 0, z0), v3(0, 0, z1), v3(0, S, z0)], m[k]); k += 1
    for z0, z1 in _strips(3, 0, SIZE):  # right wall
        b.parallelogram([v3(S, 0, z0), v3(S, 0, z1), v3(S, S, z0)], m[k]); k += 1
    for x0, x1 in _strips(2, 0, SIZE):  # the wall behind the camera
        b.parallelogram([v3(x0, 0, 0), v3(x1, 0, 0), v3(x0, S, 0)], m[k]); k += 1
    assert k == 16


def _camera(b):
    b.camera_pinhole(v3(2.0, 1.75, 0.25), v3(2.0, 2.0, 4.0), v3(0, 1, 0), PI_D / 2, 1.0)


def box(n_mats):
    """The room with 16 materials, or with a 17th on a plinth in its middle."""
    assert n_mats in (16, 17)

    def fill(b):
        _camera(b)
        m = _materials(b, n_mats)
        b.sky()
        _room(b, m)
        if n_mats == 17:
            b.parallelogram([v3(1.5, 0.5, 2.5), v3(2.5, 0.5, 2.5), v3(1.5, 0.75, 3.25)], m[16])
    return fill


def full_list(seed=29):
    """The room and 112 small parallelograms and lone triangles inside it: LDS_PAIRS pairs, sixteen materials."""
    def fill(b):
        rng = np.random.default_rng(seed)
        _camera(b)
        m = _materials(b, 16)
        b.sky()
        _room(b, m)
        for i in range(LDS_PAIRS - 16):
            c = rng.uniform(0.4, 3.6, 3)
            c[2] = rng.uniform(1.0, 3.6)  # in front of the camera
            P = [v3(*c), v3(*(c + rng.uniform(-0.35, 0.35, 3))), v3(*(c + rng.uniform(-0.35, 0.35, 3)))]
            if i % 7 == 3:
                b.triangle(P, m[i % 16])
            else:
                b.parallelogram(P, m[i % 16])
    return fill
