"""rtmi_direct_sample_mis without a GPU: the numpy restatement (tests/mislib.py) held to what include/rtmi.h promises -- the
two balance weights of one light point sum to 1, a one-vertex Monte Carlo of the weighted pair has the scattered ray's
mean with bounded samples, and the light of a hit is right on hand-worked tables."""
import math

import numpy as np
import pytest

import directlib as dl
import mislib as ml
import rtmi

f32 = np.float32
ULP1 = float(np.spacing(f32(1)))
TRI, PGRAM, BOX, SPHERE, MESH, NONE = (rtmi.RTMI_HIT_TRIANGLE, rtmi.RTMI_HIT_PARALLELOGRAM, rtmi.RTMI_HIT_PARALLELEPIPED,
                                       rtmi.RTMI_HIT_SPHERE, rtmi.RTMI_HIT_MESH, rtmi.RTMI_HIT_NONE)


def _unit(v):
    v = np.asarray(v, dtype=np.float64)
    return (v / np.linalg.norm(v)).astype(f32)


# ------------------------------------------------------------------ the weights
GEOMETRIES = [
    # x, N, the light point q, the light's normal, scale
    ((0, 0, 0), (0, 1, 0), (0, 0.1, 0), (0, -1, 0), 36 / math.pi),          # under the lamp, 0.1 away
    ((0, 0, 0), (0, 1, 0), (2.9, 0.1, -2.9), (0, -1, 0), 36 / math.pi),     # its corner: grazing both ways
    ((0, 0, 0), (0, 1, 0), (0, 1.5, 0), (0, -1, 0), 36 / math.pi),
    ((0, 0, 0), (0, 1, 0), (1, 8.5, 2), (0, -1, 0), 36 / math.pi),          # far: the light sample carries the weight
    ((5, 0, 5), (0, 1, 0), (0.1, 7, 4.5), (1, 0, 0), 0.37),                 # a small light seen at an angle
    ((1, 2, 3), _unit((1, 1, 1)), (4, 9, 5), _unit((-1, -2, 0.5)), 1e-3),
    ((1, 2, 3), _unit((1, 1, 1)), (1.001, 2.002, 3.001), _unit((-1, -1, -1)), 1e4),
]


@pytest.mark.parametrize("k", range(len(GEOMETRIES)))
def test_the_two_weights_of_one_light_point_sum_to_one(k):
    x, N, q, ln, scale = GEOMETRIES[k]
    x, N, q, ln = (np.asarray(v, dtype=f32).reshape(1, 3) for v in (x, N, q, ln))
    # the light sample, as SAMPLE forms it
    w = (q - x).astype(f32)
    d2 = dl._dot(w, w)
    dist = np.sqrt(d2).astype(f32)
    wi = (w / dist[:, None]).astype(f32)
    cs, cl = dl._dot(N, wi), np.abs(dl._dot(ln, wi))
    assert cs[0] > 0 and cl[0] > 0
    a = ml.mis_a(cs, cl, f32(scale))
    wl = ml.light_weight(a, d2)
    # the scattered ray that finds the same point, as WEIGH forms it: carry (wi, N . wi), t = dist
    t = dist
    ws, div = ml.scatter_weight(ml.mis_a(dl._dot(N, wi), np.abs(dl._dot(ln, wi)), f32(scale)), (t * t).astype(f32))
    assert div[0]
    total = float(wl[0]) + float(ws[0])
    print("geometry %d: light %.9g scattered %.9g sum - 1 = %.3g ulp" % (k, wl[0], ws[0], (total - 1) / ULP1))
    assert abs(total - 1) <= 2 * ULP1
    # SAMPLE's g is the unweighted (a / d2) times the light weight: three roundings apart at the most
    g, g0 = float(ml.sample_g(a, d2)[0]), float(a[0]) / float(d2[0])
    assert abs(g - g0 * float(wl[0])) <= 3 * float(np.spacing(f32(g)))
    assert 0 < g <= 1


def test_weights_that_cannot_be_formed_are_zero():
    a = np.array([0, -1, 1, np.nan, 1, np.inf, 3e38, 1, 1], dtype=f32)
    d2 = np.array([1, 1, 0, 1, np.nan, 1, 3e38, np.inf, 4], dtype=f32)
    w, div = ml.scatter_weight(a, d2)
    assert div.tolist() == [False] * 8 + [True]
    assert np.array_equal(w.view(np.uint32)[:8], np.zeros(8, np.uint32)) and w[8] == f32(0.2)


# ------------------------------------------------------------------ one vertex under a lamp
def _one_vertex(h, n, seed):
    """A diffuse point at the origin, normal +y, albedo 1, under a 6 x 6 lamp of emission 1 at height h facing down: per
    sample (X, Y, Z) = the scattered ray alone, the weighted pair, the unweighted light sample (rtmi_direct_sample's)."""
    rng = np.random.default_rng(seed)
    scale = f32(36 / math.pi)  # one light: selection probability 1
    N, ln = np.array([[0, 1, 0]], f32), np.array([[0, -1, 0]], f32)
    # the scattered ray: cosine-distributed
    r, phi = np.sqrt(rng.random(n)), 2 * math.pi * rng.random(n)
    d = np.stack([r * np.cos(phi), np.sqrt(np.maximum(0, 1 - r * r)), r * np.sin(phi)], axis=1).astype(f32)
    with np.errstate(all="ignore"):
        t = (f32(h) / d[:, 1]).astype(f32)
        hit = (d[:, 1] > 0) & (np.abs(t * d[:, 0]) <= 3) & (np.abs(t * d[:, 2]) <= 3)
    X = hit.astype(np.float64)
    ws, _ = ml.scatter_weight(ml.mis_a(dl._dot(np.repeat(N, n, 0), d), np.abs(dl._dot(np.repeat(ln, n, 0), d)), scale), (t * t).astype(f32))
    # the light sample: uniform on the lamp
    q = np.stack([rng.uniform(-3, 3, n), np.full(n, h), rng.uniform(-3, 3, n)], axis=1).astype(f32)
    d2 = dl._dot(q, q)
    wi = (q / np.sqrt(d2).astype(f32)[:, None]).astype(f32)
    a = ml.mis_a(dl._dot(np.repeat(N, n, 0), wi), np.abs(dl._dot(np.repeat(ln, n, 0), wi)), scale)
    Y = np.where(hit, ws, 0).astype(np.float64) + ml.sample_g(a, d2).astype(np.float64)
    Z = (a / d2).astype(np.float64)
    return X, Y, Z


@pytest.mark.parametrize("h", [0.1, 1.5, 8.5])
def test_one_vertex_monte_carlo_has_the_scattered_ray_s_mean(h):
    n = 400000
    X, Y, Z = _one_vertex(h, n, 11)
    se = math.sqrt(X.var(ddof=1) / n + Y.var(ddof=1) / n)
    print("lamp %.1f away: scattered alone mean %.5f var %.4g | weighted pair mean %.5f var %.4g max %.3f | light sample alone "
          "mean %.4f var %.4g max %.1f" % (h, X.mean(), X.var(ddof=1), Y.mean(), Y.var(ddof=1), Y.max(), Z.mean(), Z.var(ddof=1), Z.max()))
    assert se > 0 and abs(X.mean() - Y.mean()) <= 5 * se
    assert Y.max() <= 2 + 1e-6  # each half is at most albedo * Le = 1
    if h == 0.1:
        assert Z.max() > 100 and Y.var(ddof=1) < 0.01 * Z.var(ddof=1)  # where the unweighted sample is unbounded
    if h == 8.5:
        assert Y.var(ddof=1) < 0.1 * X.var(ddof=1)  # far away the pair keeps the light sampler's gain


# ------------------------------------------------------------------ the light of a hit
def _table(rows):
    tab = np.zeros(len(rows), dtype=rtmi.LIGHT_DTYPE)
    for j, (entry, element, kind) in enumerate(rows):
        tab[j]["entry"], tab[j]["element"], tab[j]["kind"] = entry, element, kind
    return tab


def _hits(rows):
    H = np.zeros((len(rows), 12), np.int32)
    for i, (kind, entry, element) in enumerate(rows):
        H[i, 7], H[i, 8], H[i, 9] = kind, entry, element
    return H


# entries: 0 a wall, 1 a sphere, 2 a lamp parallelogram, 3 a box whose face 3 is degenerate (five lights), 4 a nested list's
# sphere, 5 a mesh, 6 an emissive triangle two lists deep, 7 a wall behind it
HAND_TABLE = [(2, 0, 0)] + [(3, f, 0) for f in (0, 1, 2, 4, 5)] + [(6, 0, 1)]
HAND_MAP = np.full((7, 8), -1, np.int32)
HAND_MAP[2, 0], HAND_MAP[2, 6] = 0, 0
HAND_MAP[3, [0, 1, 2, 4, 5]], HAND_MAP[3, 6] = [1, 2, 3, 4, 5], 1
HAND_MAP[6, 0], HAND_MAP[6, 6] = 6, 6
HAND_HITS = [
    ((PGRAM, 2, 0), 0), ((PGRAM, 2, 1), 0),                  # both triangles of the parallelogram are the one light
    ((BOX, 3, 0), 1), ((BOX, 3, 1), 2), ((BOX, 3, 2), 3), ((BOX, 3, 4), 4), ((BOX, 3, 5), 5),
    ((BOX, 3, 3), -1),                                       # the degenerate face is no light
    ((BOX, 3, 6), -1), ((BOX, 3, 7), -1), ((BOX, 3, -1), -1),
    ((TRI, 6, 0), 6),                                        # the nested triangle, by its recording index
    ((TRI, 0, 0), -1), ((PGRAM, 7, 0), -1), ((PGRAM, 8, 0), -1), ((PGRAM, 1 << 30, 0), -1),  # no light / beyond the map
    ((TRI, -1, 0), -1), ((BOX, -1, 2), -1), ((PGRAM, -(1 << 31), 0), -1),
    ((SPHERE, 2, 0), -1), ((MESH, 3, 1), -1), ((NONE, 2, 0), -1), ((rtmi.RTMI_HIT_SKY, 6, 0), -1), ((99, 2, 0), -1),
]


def test_the_light_of_a_hit_on_a_hand_worked_table():
    tab = _table(HAND_TABLE)
    H = _hits([h for h, _ in HAND_HITS])
    want = [j for _, j in HAND_HITS]
    assert ml.light_of_hit(tab, H).tolist() == want
    m = ml.hit_light_map(tab)
    assert np.array_equal(m, HAND_MAP)
    assert ml.light_by_map(m, H).tolist() == want


def test_the_map_is_the_rule_on_random_hits_and_an_empty_table():
    rng = np.random.default_rng(3)
    tab = _table(HAND_TABLE)
    H = _hits([(int(k), int(e), int(f)) for k, e, f in zip(rng.integers(-1, 8, 4000), rng.integers(-2, 10, 4000), rng.integers(-2, 9, 4000))])
    assert np.array_equal(ml.light_by_map(ml.hit_light_map(tab), H), ml.light_of_hit(tab, H))
    none = _table([])
    assert ml.hit_light_map(none).shape == (0, 8)
    assert (ml.light_by_map(ml.hit_light_map(none), H) == -1).all() and (ml.light_of_hit(none, H) == -1).all()


def test_weigh_and_sample_on_one_hand_worked_path():
    """One path: its vertex sampled a lamp 2 above it (flag set, carry straight up), the scattered ray hit that lamp at t = 2
    and scattered on (so the step samples again).  scale = 4 / pi: a unit-emission 2 x 2 lamp alone in the table."""
    tab = _table([(0, 0, 0)])
    tab["p0"], tab["e1"], tab["e2"], tab["n"] = (-1, 2, -1), (2, 0, 0), (0, 0, 2), (0, -1, 0)
    tab["emission"], tab["scale"], tab["cdf"], tab["area"] = (1, 1, 1), f32(4 / math.pi), 1, 4
    H = np.zeros((1, 12), np.int32)
    H[0, 0] = f32(2).view(np.int32)
    H[0, 3:6] = np.array([0, -1, 0], f32).view(np.int32)
    H[0, 6], H[0, 7], H[0, 8], H[0, 9] = 0, PGRAM, 0, 1
    ps = ml.PathState([[0, 2, 0]], [[0, -1, 0]], H, [1], [[1, 1, 1]], [[0.5, 0.5, 0.5]], [[1, 2, 3, 4, 5, 6]], flags=[3],
                      carry=[[0, 1, 0, 1]])
    out = ml.step(tab, [dl.LIGHT], ps.copy(), 0, 1)
    a = f32(4 / math.pi)
    w = f32(a / f32(a + f32(4)))
    assert np.array_equal(out.E, np.full((1, 3), w, f32)) and out.counts.tolist() == [3, 6]
    assert out.flags.tolist() == [2] and np.array_equal(out.C, ps.C) and np.array_equal(out.LS, ps.LS)  # a light does not sample
    # the same hit without the flag keeps its emission; with a Lambertian material the vertex samples and writes the carry
    ps.flags[:] = 0
    out = ml.step(tab, [dl.LAMBERTIAN], ps.copy(), 0, 1)
    assert np.array_equal(out.E, ps.E) and out.flags.tolist() == [1] and out.counts.tolist() == [4, 5]
    assert np.array_equal(out.C, np.array([[0, -1, 0, 1]], f32)) and not np.array_equal(out.LS, ps.LS)
    assert (out.DR == 0).all() and (out.SD == 0).all()  # the point lies in the lamp's plane: cl = 0, no valid sample
