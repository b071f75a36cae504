"""Steering the RNG: states whose next draws are chosen, so that a test reaches the branches only particular draws take.
numpy only; no test lives here.

A state is six uint32 words in the library's order d, v0, v1, v2, v3, v4 (xorwow.h: Rng; the plane order of d_states).
One draw (curand's XORWOW):  t = v0 ^ (v0 >> 2);  (v0, v1, v2, v3) = (v1, v2, v3, v4);  v4' = (v4 ^ (v4 << 4)) ^ (t ^ (t << 1));
d += 362437;  the draw is v4' + d.

Steering.  Draw k (k = 1..5) is w_k + d + k * 362437 where w_k is the v4 word after k steps, so the draws fix w_1..w_5 for any
Weyl word d.  With f(x) = x ^ (x << 4) and g(v) = t ^ (t << 1), t = v ^ (v >> 2):
    w_1 = f(v4) ^ g(v0),  w_2 = f(w_1) ^ g(v1),  w_3 = f(w_2) ^ g(v2),  w_4 = f(w_3) ^ g(v3),  w_5 = f(w_4) ^ g(v4).
g is a bijection (both of its halves are unit triangular over GF(2)), so v4, v3, v2, v1 and then v0 follow in turn.

The floats.  CudaRandomFloat(-1, 1) of draw x is fma(x, 2^-31, 2^-32) - 1 in binary32 and CudaRandomFloat(0, 1) is
fma(x, 2^-32, 2^-33), where x is first converted to binary32 (trace_helpers.h: rng_pm1_of, rng_01_of; the host suite holds
both to the library's and the oracle's own functions).  The doubled uniform is a binary32 in (0, 2]: below 1 it is a
multiple of 2^-24 and from 1 on a multiple of 2^-23, so a NEGATIVE coordinate is a multiple of 2^-24 and a POSITIVE one a
multiple of 2^-23 only.  The boundary points below therefore carry their odd multiples of 2^-24 on negative coordinates:
(1, -(2^-12 + 2^-24), 0) is attainable and (1, 2^-12 + 2^-24, 0) is not; the squares, and so the sums, are the same.
"""
import numpy as np

WEYL = np.uint32(362437)
U32 = np.uint32
F32 = np.float32
PAD = (0x9e3779b9, 0x7f4a7c15, 0xf39cc060, 0x5cedc834, 0x1082276b)  # the draws of a steered state that the caller left open


# ------------------------------------------------------------------ the generator
def rng_next(states):
    """Advance every state of `states` ((..., 6) uint32, in place) by one draw; returns the draws."""
    s = states
    v0 = s[..., 1]
    t = v0 ^ (v0 >> U32(2))
    v4 = s[..., 5]
    new = (v4 ^ (v4 << U32(4))) ^ (t ^ (t << U32(1)))
    s[..., 1] = s[..., 2]
    s[..., 2] = s[..., 3]
    s[..., 3] = s[..., 4]
    s[..., 4] = v4
    s[..., 5] = new
    s[..., 0] = s[..., 0] + WEYL
    return s[..., 5] + s[..., 0]


def draws_of(state, k):
    """The next k draws of one state (a copy is advanced)."""
    s = np.array(state, dtype=np.uint32).reshape(1, 6)
    return np.array([int(rng_next(s)[0]) for _ in range(k)], dtype=np.uint32)


def _f(x):
    return x ^ (x << U32(4))


def _g_inv(y):
    y = np.asarray(y, dtype=np.uint32).copy()
    for sh in (1, 2, 4, 8, 16):  # t ^ (t << 1) = y
        y ^= y << U32(sh)
    for sh in (2, 4, 8, 16):  # v ^ (v >> 2) = t
        y ^= y >> U32(sh)
    return y


def state_for(draws, d=0x12345678):
    """The state (6,) uint32 whose next len(draws) <= 5 outputs are exactly `draws`, with Weyl word d; the draws left open
    are PAD's.  `draws` may also be (n, k): then (n, 6)."""
    dr = np.asarray(draws, dtype=np.uint64)
    single = dr.ndim == 1
    dr = dr.reshape(-1, dr.shape[-1]) if dr.size else dr.reshape(1, 0)
    n, k = dr.shape
    if k > 5:
        raise ValueError("XORWOW has five free outputs, %d asked for" % k)
    if ((dr >> np.uint64(32)) != 0).any():
        raise ValueError("a draw is a 32-bit word")
    full = np.empty((n, 5), dtype=np.uint32)
    full[:, :k] = dr.astype(np.uint32)
    full[:, k:] = np.array(PAD[k:], dtype=np.uint32)
    d = U32(int(d) & 0xffffffff)
    with np.errstate(over="ignore"):
        w = [full[:, j] - (d + U32(j + 1) * WEYL) for j in range(5)]
        v4 = _g_inv(w[4] ^ _f(w[3]))
        v3 = _g_inv(w[3] ^ _f(w[2]))
        v2 = _g_inv(w[2] ^ _f(w[1]))
        v1 = _g_inv(w[1] ^ _f(w[0]))
        v0 = _g_inv(w[0] ^ _f(v4))
    out = np.stack([np.full(n, d, dtype=np.uint32), v0, v1, v2, v3, v4], axis=1).astype(np.uint32)
    return out[0] if single else out


# ------------------------------------------------------------------ draw <-> float
def _uniform64(x):
    """x * 2^-32 + 2^-33 exactly, in binary64, of the draw converted to binary32 first (the one rounding left is the
    caller's: 24 bits of x at 2^8 or above and the 2^-33 term fit binary64)."""
    xf = np.asarray(x, dtype=np.uint32).astype(np.float32).astype(np.float64)
    return xf * 2.0 ** -32 + 2.0 ** -33


def rng_01_of(x):
    return _uniform64(x).astype(np.float32)


def rng_pm1_of(x):
    u2 = (2.0 * _uniform64(x)).astype(np.float32)  # the doubling is exact and commutes with the rounding
    return (u2.astype(np.float64) - 1.0).astype(np.float32)  # one rounding: the difference of two binary32 is exact in binary64


def _draw_for(target, fwd, guess):
    target = F32(target)
    if not np.isfinite(target):
        raise ValueError("%r is not attainable" % (target,))
    g = int(np.clip(np.floor(guess), 0, 0xffffffff))
    lo, hi = max(g - 1024, 0), min(g + 1024, 0xffffffff)
    cand = np.arange(lo, hi + 1, dtype=np.uint64).astype(np.uint32)
    got = fwd(cand)
    ok = np.flatnonzero(got.view(np.uint32) == np.array([target]).view(np.uint32)[0])
    if ok.size == 0:
        if target == 0 and (got == 0).any():  # (-0.0f asked for: the sampler only makes +0)
            raise ValueError("-0.0 is not attainable")
        raise ValueError("%r (%s) is not attainable" % (target, float(target).hex()))
    return int(cand[ok[0]])


def draw_for_pm1(x):
    """The smallest draw whose CudaRandomFloat(-1, 1) is exactly the binary32 x; ValueError where there is none."""
    return _draw_for(x, rng_pm1_of, (float(F32(x)) + 1.0) * 2.0 ** 31 - 0.5)


def draw_for_01(r):
    """The smallest draw whose CudaRandomFloat(0, 1) is exactly the binary32 r; ValueError where there is none."""
    return _draw_for(r, rng_01_of, float(F32(r)) * 2.0 ** 32 - 0.5)


# ------------------------------------------------------------------ the sampler and its runs
BALL_S_MAX = F32(1.0) + F32(2.0 ** -23)
CENTRE = 0x80000000  # the jitter draw of a pixel's centre: rng_01 == 0.5


def ball_sum(x, y, z):
    """x*x + y*y + z*z as the reference forms it in binary32: three products, added left to right, nothing fused."""
    x, y, z = (np.asarray(a, dtype=np.float32) for a in (x, y, z))
    return ((x * x).astype(np.float32) + (y * y).astype(np.float32)).astype(np.float32) + (z * z).astype(np.float32)


def rejected(x, y, z):
    """l = sqrt(sum) > 1 (lambertian.cu:25-26), taken literally: the square root in binary64 of the binary32 sum,
    rounded to binary32."""
    l = np.sqrt(ball_sum(x, y, z).astype(np.float64)).astype(np.float32)
    return l > F32(1)


def first_run(states, skip):
    """Per state: how many sampler attempts (three draws each) are rejected in a row after `skip` draws."""
    s = np.array(states, dtype=np.uint32).reshape(-1, 6)
    for _ in range(skip):
        rng_next(s)
    run = np.zeros(len(s), dtype=np.int64)
    live = np.arange(len(s))
    while live.size:
        sub = s[live]
        p = [rng_pm1_of(rng_next(sub)) for _ in range(3)]
        s[live] = sub
        rej = rejected(*p)
        run[live[rej]] += 1
        live = live[rej]
    return run


FAMILY_SIZE = 1 << 20


def family(n=FAMILY_SIZE, first=0):
    """The candidate states of the run search: state i has the Weyl word i and the five vector words
    (i + 1) * m_k mod 2^32 for five fixed odd multipliers -- every word of every state differs, none is zero, and nothing
    but numpy's integer arithmetic goes into them, so the family is the same on every machine."""
    i = np.arange(first, first + n, dtype=np.uint64)
    mult = (0x9e3779b1, 0x85ebca6b, 0xc2b2ae35, 0x27d4eb2f, 0x165667b1)
    cols = [i] + [((i + np.uint64(1)) * np.uint64(m)) for m in mult]
    st = (np.stack(cols, axis=1) & np.uint64(0xffffffff)).astype(np.uint32)
    for _ in range(8):  # eight draws in, the few-bit structure of small i is gone
        rng_next(st)
    return st


def search_runs(min_run=12, skip=2, n=FAMILY_SIZE):
    """(states (m, 6), runs (m,)) of the family members whose first run after `skip` draws is at least min_run, in the
    family's order."""
    st = family(n)
    run = first_run(st, skip)
    idx = np.flatnonzero(run >= min_run)
    return st[idx], run[idx]


# ------------------------------------------------------------------ named sampler points
def _axis(n):
    n = np.asarray(n, dtype=np.float32)
    nz = np.flatnonzero(n)
    if nz.size != 1 or abs(float(n[nz[0]])) != 1.0:
        raise ValueError("the normal must be an axis: components 0 or +-1, one of them set")
    a = int(nz[0])
    return n, a, [k for k in range(3) if k != a]


def _smallest_reject_y():
    """The smallest |y| (y a negative multiple of 2^-24, attainable) for which 1*1 + y*y rounds to 1 + 2^-22."""
    k = np.arange(1, 1 << 14, dtype=np.float64)
    y = (-k * 2.0 ** -24).astype(np.float32)
    s = ball_sum(np.ones_like(y), y, np.zeros_like(y))
    return F32(y[np.flatnonzero(s >= F32(1.0) + F32(2.0 ** -22))[0]])


Y_ACCEPT = F32(-(2.0 ** -12 + 2.0 ** -24))  # 1 + y*y = 1 + 2^-24 + 2^-35 + 2^-48 rounds up to 1 + 2^-23: l == 1, accepted
Y_REJECT = _smallest_reject_y()  # 1 + y*y rounds to 1 + 2^-22: l == 1 + 2^-23, rejected

POINT_NAMES = ("zero", "minus_n", "plus_n", "boundary_accept", "boundary_reject", "corner", "metal_cancel",
               "metal_near_cancel")
# what the reference does with each as a sampler attempt: accepted (3 draws) or rejected (at least 6)
ACCEPTED = {"zero": True, "minus_n": True, "plus_n": True, "boundary_accept": True, "boundary_reject": False,
            "corner": False, "metal_cancel": True, "metal_near_cancel": True}
# the scattered direction is NaN: Lambertian for zero (0 / 0) and minus_n (normalize(0)), Metal with fuzz 1 and the ray
# d = -n for metal_cancel (Ray's constructor normalises the zero vector)
NAN_LAMBERTIAN = ("zero", "minus_n", "metal_cancel")  # (metal_cancel is the point minus_n under its Metal name)
NAN_METAL_FUZZ1 = ("minus_n", "metal_cancel")


def point(name, n):
    """The sampler point (x, y, z) float32 of `name` for the axis normal n.  The boundary points have +-1 on the normal's
    axis (the normal's sign), y on the first tangent axis and 0 on the other: the sum is RN(1 + y*y) + 0 or
    RN(RN(y*y + 0) + 1) depending on the axis, the same binary32 either way."""
    n, a, t = _axis(n)
    p = np.zeros(3, dtype=np.float32)
    if name == "zero":
        pass
    elif name in ("minus_n", "metal_cancel"):
        p = (-n).astype(np.float32)
    elif name == "plus_n":
        p = n.copy()
    elif name == "boundary_accept":
        p[a], p[t[0]] = n[a], Y_ACCEPT
    elif name == "boundary_reject":
        p[a], p[t[0]] = n[a], Y_REJECT
    elif name == "corner":
        p[:] = 1
    elif name == "metal_near_cancel":
        p = (-n).astype(np.float32)
        p[t[0]] = F32(-(2.0 ** -24))
    else:
        raise KeyError(name)
    return p + F32(0)  # (-0.0 -> +0.0: the sampler makes no negative zero)


def point_draws(name, n):
    return [draw_for_pm1(c) for c in point(name, n)]


def point_state(name, n, lead=(), d=0x12345678):
    """The state whose draws are `lead` (at most two: the jitter) and then the named point.  The Weyl word is the first
    of d, d + g, d + 2 g, ... (g = 0x9e3779b9) with which a rejected point is followed by an accepted attempt, so that the
    sampler takes exactly 3 draws for an accepted point and exactly 6 for a rejected one.  (The draws behind five chosen
    ones move little with a neighbouring Weyl word -- the generator mixes slowly -- hence the long stride.)"""
    draws = list(lead) + point_draws(name, n)
    want = 0 if ACCEPTED[name] else 1
    for k in range(1024):
        st = state_for(draws, d=(d + k * 0x9e3779b9) & 0xffffffff)
        if int(first_run(st, len(lead))[0]) == want:
            return st
    raise RuntimeError("no Weyl word found for %s" % name)
