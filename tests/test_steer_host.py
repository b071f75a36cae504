"""tests/steerlib.py held to the library's and the oracle's own generators and float maps, the named sampler points run
through the reference's Scatter as the oracle has it, and the condition of the rejection-run search.  No GPU."""
import ctypes as C

import numpy as np
import pytest

import oraclelib
import rtmi
import steerlib as S
from parity import bits

U32P = C.POINTER(C.c_uint32)
NORMALS = [(0, 1, 0), (0, -1, 0), (1, 0, 0), (-1, 0, 0), (0, 0, 1), (0, 0, -1)]


def _p(a):
    return a.ctypes.data_as(U32P)


def _both(mn, mx, state):
    """CudaRandomFloat(mn, mx) from a copy of `state` by the library and by the oracle: (floats, states after)."""
    a, b = state.copy(), state.copy()
    x = np.float32(rtmi.lib().rtmi_rng_host_random_float(C.c_float(mn), C.c_float(mx), _p(a)))
    y = np.float32(oraclelib.lib().orc_random_float(C.c_float(mn), C.c_float(mx), _p(b)))
    assert bits(x) == bits(y) and np.array_equal(a, b)
    return x, a


def advanced(state, k):
    s = np.array(state, dtype=np.uint32).reshape(1, 6)
    for _ in range(k):
        S.rng_next(s)
    return s[0]


def test_steering_reproduces_random_tuples():
    """1000 random 5-tuples (and shorter ones) with random Weyl words: the library's and the oracle's generators give
    exactly the draws asked for, as floats of both ranges, and leave the state steerlib's rng_next leaves."""
    rng = np.random.default_rng(2024)
    draws = rng.integers(0, 1 << 32, (1000, 5), dtype=np.uint64)
    draws[:8, :] = [[0, 0xffffffff, 0x7fffffff, 0x80000000, 0x80000080]] * 8  # the extremes among them
    weyl = rng.integers(0, 1 << 32, 1000, dtype=np.uint64)
    for i in range(1000):
        k = 5 if i >= 100 else 1 + i % 5
        st = S.state_for(draws[i, :k], d=int(weyl[i]))
        assert st.dtype == np.uint32 and st.shape == (6,) and int(st[0]) == int(weyl[i])
        assert np.array_equal(S.draws_of(st, k), draws[i, :k].astype(np.uint32))
        cur = st.copy()
        for j in range(k):
            mn, mx = ((-1.0, 1.0), (0.0, 1.0))[(i + j) % 2]
            x, cur = _both(mn, mx, cur)
            want = (S.rng_pm1_of if mn < 0 else S.rng_01_of)(np.uint32(draws[i, j]))
            assert bits(x) == bits(want), (i, j, hex(int(draws[i, j])))
        assert np.array_equal(cur, advanced(st, k))
    many = S.state_for(draws, d=5)
    assert many.shape == (1000, 6) and np.array_equal(many[17], S.state_for(draws[17], d=5))
    with pytest.raises(ValueError):
        S.state_for([0] * 6)


def test_the_float_maps_and_their_inverses():
    f = np.float32
    # the values the issue names
    assert S.rng_pm1_of(np.uint32(0)) == f(-1) and S.rng_pm1_of(np.uint32(0xffffffff)) == f(1)
    assert (S.rng_pm1_of(np.arange(0x7fffffff, 0x80000081, dtype=np.uint64).astype(np.uint32)) == 0).all()
    assert bits(S.rng_pm1_of(np.uint32(0x80000000))) == 0  # +0.0
    assert S.rng_01_of(np.uint32(0)) == f(2.0 ** -33) and S.rng_01_of(np.uint32(0xffffffff)) == f(1)
    assert S.rng_01_of(np.uint32(S.CENTRE)) == f(0.5)
    up = lambda x: np.nextafter(f(x), f(2))
    for fn, inv, mn, vals in (
            (S.rng_pm1_of, S.draw_for_pm1, -1.0, [-1, 0, 1, -0.5, 0.5, S.Y_ACCEPT, S.Y_REJECT, -2.0 ** -24, 2.0 ** -23]),
            (S.rng_01_of, S.draw_for_01, 0.0, [2.0 ** -33, 1, 0.25, 0.5, 0.75, up(0.25), up(0.5), up(0.75), 0.5 + 2.0 ** -24])):
        for v in vals:
            x = inv(v)
            assert bits(fn(np.uint32(x))) == bits(f(v))
            got, _ = _both(mn, 1.0, S.state_for([x]))
            assert bits(got) == bits(f(v)), (v, hex(x))
            assert x == 0 or bits(fn(np.uint32(x - 1))) != bits(f(v))  # the smallest such draw
    for v in (2.0 ** -24, 2.0 ** -12 + 2.0 ** -24, -1.5, 1.0 + 2.0 ** -23, float("nan")):
        with pytest.raises(ValueError):
            S.draw_for_pm1(v)
    for v in (0.0, 2.0 ** -34, 1.5 * 2.0 ** -33, 1.0 + 2.0 ** -23, -0.5, float("inf")):
        with pytest.raises(ValueError):
            S.draw_for_01(v)


def test_boundary_sums():
    """The sums the boundary points are named for, as the reference forms them (and as `l > 1` then decides)."""
    one = np.float32(1)
    assert S.ball_sum(1, S.Y_ACCEPT, 0) == S.ball_sum(0, S.Y_ACCEPT, 1) == one + np.float32(2.0 ** -23) == S.BALL_S_MAX
    assert S.ball_sum(1, S.Y_REJECT, 0) == S.ball_sum(0, S.Y_REJECT, -1) == one + np.float32(2.0 ** -22)
    nearer = np.float32(S.Y_REJECT + np.float32(2.0 ** -24))  # one step of 2^-24 towards zero: still accepted
    assert abs(nearer) < abs(S.Y_REJECT) and S.ball_sum(1, nearer, 0) == S.BALL_S_MAX
    assert not S.rejected(1, S.Y_ACCEPT, 0) and S.rejected(1, S.Y_REJECT, 0) and S.rejected(1, 1, 1)
    assert not S.rejected(0, 0, 0) and not S.rejected(0, -1, 0)


@pytest.fixture(scope="module")
def scene():
    ob = oraclelib.OracleBuilder(3)
    mats = {"lambertian": ob.lambertian((0.5, 0.25, 0.75)), "metal0": ob.metal((0.9, 0.8, 0.7), 0.0),
            "metal_quarter": ob.metal((0.9, 0.8, 0.7), 0.25), "metal1": ob.metal((0.9, 0.8, 0.7), 1.0)}
    return ob, mats


@pytest.mark.parametrize("n", NORMALS)
@pytest.mark.parametrize("name", S.POINT_NAMES)
def test_named_points_through_the_reference_scatter(scene, name, n):
    """Every named point attains its floats bit for bit, and the reference's own Scatter takes it as named: the state
    advances by 3 draws (accepted) or by 6 (rejected once), and the direction is NaN exactly where the name says."""
    ob, mats = scene
    n = np.array(n, dtype=np.float32)
    st = S.point_state(name, n)
    cur = st.copy()
    for c in S.point(name, n):
        x, cur = _both(-1.0, 1.0, cur)
        assert bits(x) == bits(c), (name, n.tolist())
    draws = 3 if S.ACCEPTED[name] else 6
    o, d = (n * np.float32(2)).astype(np.float32), (-n).astype(np.float32)  # the ray onto the surface at the origin
    for mat, fuzz in (("lambertian", None), ("metal0", 0.0), ("metal_quarter", 0.25), ("metal1", 1.0)):
        state = st.copy()
        sc, out = ob.probe_scatter(mats[mat], o, d, 2.0, n, state)
        assert sc
        assert np.array_equal(state, advanced(st, 0 if fuzz == 0.0 else draws)), (name, mat)
        nan = np.isnan(out[6:9])
        if mat == "lambertian":
            want = name in S.NAN_LAMBERTIAN
        elif mat == "metal1":
            want = name in S.NAN_METAL_FUZZ1
        else:
            want = False
        assert nan.all() == nan.any() == want, (name, mat, out[6:9].tolist())
        if name == "plus_n" and mat == "lambertian":
            assert np.array_equal(out[6:9], n)
        if name == "metal_near_cancel" and mat == "metal1":
            t = np.flatnonzero(n == 0)[0]
            want_dir = np.zeros(3, np.float32)
            want_dir[t] = -1
            assert np.array_equal(out[6:9], want_dir)


def test_the_run_search_finds_its_states():
    """The condition of the GPU tests of long rejection runs: the family holds at least 8 states that open with a run of
    12 or more behind the two jitter draws.  Counted on the family of steerlib.family(): 139, the longest run 19."""
    states, runs = S.search_runs(min_run=12, skip=2)
    print("states with a run of 12 or more:", len(states), "longest", int(runs.max()))
    assert len(states) >= 8, len(states)
    assert (runs >= 12).all() and np.array_equal(S.first_run(states, 2), runs)
    # the count is the oracle's too: its sampler, from the state behind the two draws, takes 3 * (run + 1) draws
    ob = oraclelib.OracleBuilder(3)
    m = ob.lambertian((0.5, 0.5, 0.5))
    n = np.array([0, 1, 0], np.float32)
    for st, run in list(zip(states, runs))[:16]:
        state = advanced(st, 2)
        sc, _ = ob.probe_scatter(m, 2 * n, -n, 2.0, n, state)
        assert sc and np.array_equal(state, advanced(st, 2 + 3 * (int(run) + 1)))
