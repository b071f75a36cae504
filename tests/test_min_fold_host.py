"""Host side of the fold by minimum (closest_hit.h, RUN_TRIS, steps (b) and (c)): the numpy restatement of the two triangle
tests that tests/test_gpu_min_fold.py counts with, held to hand-checked rays and to the oracle; the world built for the
ordered path, which must hold enough rays of the order-dependent kind; and the case analysis itself -- the smallest key
against the reference's sequential fold -- on made-up verdicts.  No GPU."""
import numpy as np

import min_fold_worlds as mf
import oraclelib
from parity import bits

F32 = np.float32
TRI = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0]], dtype=F32)


def rays(*od):
    a = np.array(od, dtype=F32)
    return a[:, :3].copy(), a[:, 3:].copy()


def test_restatement_on_hand_checked_rays():
    """The unit right triangle in z = 0, rays along -z from z = 2: u = x, v = y, t = 2, all exact in binary32."""
    O, D = rays((0.25, 0.25, 2, 0, 0, -1),    # inside
                (0.5, 0.5, 2, 0, 0, -1),      # on the hypotenuse: u + v == 1 passes
                (0.75, 0.5, 2, 0, 0, -1),     # beyond it
                (-0.125, 0.5, 2, 0, 0, -1),   # u < 0
                (0.25, 0.25, 2, 0, 0, 1),     # pointing away: t = -2
                (0.25, 0.25, 2, 1, 0, 0),     # parallel: det == 0
                (0.25, 0.25, 2, 0, 0, -2))    # twice the direction: t = 1
    hit, t = mf.tri_test(TRI, O, D)
    assert hit.tolist() == [True, True, False, False, False, False, True]
    assert t[0] == 2 and t[1] == 2 and t[6] == 1
    # the bound is inclusive at both ends (utils.cu:74)
    assert mf.tri_test(TRI, O[:1], D[:1], t_to=2.0)[0][0] and not mf.tri_test(TRI, O[:1], D[:1], t_to=1.9999999)[0][0]
    O2, D2 = rays((0.25, 0.25, 0.001, 0, 0, -1), (0.25, 0.25, 0.0009765625, 0, 0, -1))
    assert mf.tri_test(TRI, O2, D2)[0].tolist() == [bool(F32(0.001) >= 1e-3), False]


def test_both_triangles_of_a_parallelogram_on_hand_checked_rays():
    """The unit square: (p0, p1, p2) and (p1, p2, p3 = (1, 1, 0)).  On the shared edge both pass with equal t: not the
    ordered case.  Off it exactly one does."""
    O, D = rays((0.5, 0.5, 2, 0, 0, -1), (0.25, 0.25, 2, 0, 0, -1), (0.75, 0.75, 2, 0, 0, -1), (1.5, 0.5, 2, 0, 0, -1))
    both, nearer_second = mf.both_accept(TRI, O, D)
    assert both.tolist() == [True, False, False, False] and not nearer_second.any()
    hit_b, tb = mf.tri_test(np.array([[1, 0, 0], [0, 1, 0], [1, 1, 0]], dtype=F32), O, D)
    assert hit_b.tolist() == [True, False, True, False] and tb[2] == 2


def test_restatement_equals_the_oracle_on_the_grid():
    """A parallelogram of the ordered world alone in an oracle scene: for rays through it, near its shared edge and past
    its rim, the oracle's Hit says what parallelogram.cu:25-33 makes of the restatement's two verdicts, t to the bit."""
    p = mf.grid_points()[7]
    ob = oraclelib.OracleBuilder(1)
    ob.parallelogram([p[0], p[1], p[2]], ob.lambertian([0.5, 0.5, 0.5]))
    rng = np.random.default_rng(3)
    n = 600
    a, b = rng.uniform(-0.1, 1.1, n), rng.uniform(-0.1, 1.1, n)
    a[: n // 2] = 1 - b[: n // 2] + rng.uniform(-2e-4, 2e-4, n // 2)  # within the rounding's reach of the shared edge
    target = (p[0][None, :] + a[:, None] * (p[1] - p[0])[None, :] + b[:, None] * (p[2] - p[0])[None, :])
    O = rng.uniform(-0.5, 0.5, (n, 3)).astype(F32)  # about the camera's place
    raw = (target - O).astype(F32)
    D = mf.glm_normalize(raw)  # (the oracle's Ray normalises what it is given: probe_hit gets the raw direction)
    hit_a, ta = mf.tri_test(p, O, D)
    hit_b, tb = mf.tri_test(np.array([p[1], p[2], (p[1] + p[2]) - p[0]]), O, D)
    seen_both = 0
    for i in range(n):
        h, out, _ = ob.probe_hit(O[i], raw[i])
        assert h == bool(hit_a[i] or hit_b[i]), i
        if h:
            assert F32(out[0]).view(np.uint32) == (ta[i] if hit_a[i] else tb[i]).view(np.uint32), i
        seen_both += int(hit_a[i] and hit_b[i])
    assert hit_a.sum() > 100 and hit_b.sum() > 100 and (~(hit_a | hit_b)).sum() > 20 and seen_both > 0


def test_ordered_world_holds_rays_of_the_ordered_kind():
    """What tests/test_gpu_min_fold.py asks the device's counter to reach: over all camera rays of the frame, the tasks
    with both triangles accepted against the backdrop's t and the second nearer.  At least 8."""
    ob = oraclelib.OracleBuilder(mf.SEED)
    mf.ordered_world(ob)
    O, D = mf.frame_rays(ob.camera_get())
    n, both, on_backdrop = mf.ordered_tasks(O, D)
    print("rays %d, both accepted %d (%.2e per ray), second nearer %d (%.2e per ray)" % (len(O), both, both / len(O), n, n / len(O)))
    assert len(O) == mf.SIDE * mf.SIDE * mf.SPP and on_backdrop > 0.999 * len(O)
    assert n >= 8


def test_primary_rays_follow_the_oracles_camera():
    """Sample 0 and sample 1 of a few pixels against the oracle's RayAt on its own draws."""
    import ctypes as C
    ob = oraclelib.OracleBuilder(mf.SEED)
    mf.ordered_world(ob)
    h = w = 16
    O, D, st = mf.primary_rays(ob.camera_get(), h, w, 2, mf.SEED)
    L = oraclelib.lib()
    states = oraclelib.rng_init(mf.SEED, h * w)
    for q in (0, 1, 17, 100, 255):
        s = states[q].copy()
        for sample in range(2):
            p = s.ctypes.data_as(C.POINTER(C.c_uint32))
            r1 = float(L.orc_random_float(C.c_float(0.0), C.c_float(1.0), p))
            r2 = float(L.orc_random_float(C.c_float(0.0), C.c_float(1.0), p))
            i, j = divmod(q, w)
            ray = ob.probe_camera_ray(2 * ((r1 + j) / w) - 1, 2 * ((r2 + (h - i)) / h) - 1, s)
            assert np.array_equal(bits(O[sample, q]), bits(ray[:3])) and np.array_equal(bits(D[sample, q]), bits(ray[3:])), (q, sample)
        assert np.array_equal(st[q], s), q


def sequential(verdicts, t_to, ok):
    """hitable_list.cu:11-22 over parallelogram.cu:25-33 on recorded verdicts [(ta or None, tb or None), ...], each t
    having passed against the bound at the start: (ok, t_to, winner)."""
    win = None
    for k, (ta, tb) in enumerate(verdicts):
        hit_a = ta is not None and ta <= t_to
        hit_b = not hit_a and tb is not None and tb <= t_to
        if hit_a or hit_b:
            t = ta if hit_a else tb
            if not ok or t < t_to:
                ok, t_to, win = True, t, 2 * k + (0 if hit_a else 1)
    return ok, t_to, win


def by_minimum(verdicts, t_to, ok):
    """The keys the lanes post, their minimum, and the one accept against the unmoved bound; None where a task is of
    the ordered kind."""
    keys = []
    for k, (ta, tb) in enumerate(verdicts):
        if ta is not None and tb is not None and tb < ta:
            return None
        if ta is not None:
            keys.append((ta, 2 * k))
        elif tb is not None:
            keys.append((tb, 2 * k + 1))
    if keys:
        t, low = min(keys)
        if not ok or t < t_to:
            return True, t, low
    return ok, t_to, None


def test_smallest_key_is_the_sequential_answer():
    """Random verdicts on a coarse grid of t, so that ties, equal pairs and t == t_to all occur: wherever no task is of the
    ordered kind the minimum is the fold; and the ordered kind does occur and does differ."""
    rng = np.random.default_rng(0)
    ordered = differ = 0
    for _ in range(20000):
        t_to = float(rng.integers(3, 9))
        ok = bool(rng.integers(0, 2))
        pick = lambda: None if rng.random() < 0.4 else float(rng.integers(1, int(t_to) + 1))
        verdicts = [(pick(), pick()) for _ in range(rng.integers(1, 6))]
        want = sequential(verdicts, t_to, ok)
        got = by_minimum(verdicts, t_to, ok)
        if got is None:
            ordered += 1
            plain = min([(t, k) for k, v in enumerate(verdicts) for t in v if t is not None])
            differ += int(want[1] != min(plain[0], t_to) if ok else want[1] != plain[0])
            continue
        assert got == want, (verdicts, t_to, ok, got, want)
    assert ordered > 1000 and differ > 100
