"""Scene sizes past the kernels' layout switches, on the host side: the material count a flattened scene reports, and
the cost of flattening (what rtmi_scene_commit runs before any HIP call) as the number of meshes grows.  No GPU."""
import os
import re
import time

import numpy as np

import rtmi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def v3(x, y, z):
    return np.array([x, y, z], dtype=np.float32)


def strip(k):
    """2 k^2 triangles of a gently folded unit square (242 faces for k = 11)."""
    xs = np.linspace(0.0, 1.0, k + 1, dtype=np.float32)
    f = []
    for i in range(k):
        for j in range(k):
            a, b = (xs[i], xs[j], 0.0), (xs[i + 1], xs[j], 0.0)
            c, d = (xs[i], xs[j + 1], 0.1), (xs[i + 1], xs[j + 1], 0.1)
            f.append(a + b + c)
            f.append(b + d + c)
    return np.array(f, dtype=np.float32)


def many_meshes(n_meshes, faces):
    """n_meshes copies of one mesh side by side, 1024 to a nested list (RTMI_MAX_HITABLES per list)."""
    b = rtmi.SceneBuilder(1)
    b.camera_pinhole(v3(0, 0, 5), v3(0, 0, 0), v3(0, 1, 0), 1.0, 1.0)
    m = b.lambertian(v3(0.5, 0.5, 0.5))
    for first in range(0, n_meshes, 1024):
        b.list_begin()
        for i in range(first, min(n_meshes, first + 1024)):
            g = faces.copy()
            g[:, 0::3] += 1.5 * i
            b.bvh(g, m)
        b.list_end()
    return b


def test_seventy_thousand_materials_are_all_kept():
    b = rtmi.SceneBuilder(0)
    b.camera_pinhole(v3(0, 0, 5), v3(0, 0, 0), v3(0, 1, 0), 1.0, 1.0)
    ids = [b.lambertian(v3((i & 255) / 255.0, ((i >> 8) & 255) / 255.0, (i >> 16) / 2.0)) for i in range(70000)]
    assert ids[0] == 0 and ids[-1] == 69999
    b.sphere(v3(0, 0, 0), 1.0, ids[-1])
    b.parallelogram([v3(-2, -1, -2), v3(2, -1, -2), v3(-2, -1, 2)], ids[65536])
    s = b.stats()
    assert s["materials"] == 70000
    assert (s["spheres"], s["parallelograms"]) == (1, 1)


def test_material_limit_constant():
    """The world list's triangles keep the material in 24 bits; the header and the binding name the same limit."""
    with open(os.path.join(ROOT, "include", "rtmi.h")) as f:
        m = re.search(r"#define RTMI_MAX_MATERIALS \(1 << (\d+)\)", f.read())
    assert m and 1 << int(m.group(1)) == rtmi.MAX_MATERIALS == 1 << 24


def test_flatten_cost_grows_with_the_scene_not_meshes_times_nodes():
    """Quadrupling the meshes at a fixed size per mesh must cost about four times as much, not sixteen: checking each
    mesh's top table against every search node of the scene made this quadratic (2048 meshes: 8 s against 0.5 s)."""
    faces = strip(11)
    times = {}
    for n in (512, 2048):
        b = many_meshes(n, faces)
        s = b.stats()
        assert s["bvh_faces"] >= n * len(faces) and s["bvh_nodes"] == n  # (one reference leaf per mesh)
        best = float("inf")
        for _ in range(3):
            t0 = time.perf_counter()
            b.stats()
            best = min(best, time.perf_counter() - t0)
        times[n] = best
    ratio = times[2048] / times[512]
    assert ratio < 8.0, "4x the meshes cost %.1fx (%.3f s -> %.3f s)" % (ratio, times[512], times[2048])
