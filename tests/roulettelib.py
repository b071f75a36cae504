"""Russian roulette restated (rtmi_path_roulette, rtmi_trace_roulette; include/rtmi.h): the rule of the step in numpy,
operation by operation; the forward product rtmi_trace_roulette writes; the loop trace_steps_roulette on fresh states, with
the paths the roulette killed; the device call through the C ABI with canaries around every array; and two scenes of the
trace tests, built here.  No test lives here."""
import ctypes as C

import numpy as np

import directlib as dl
import rtmi
from rtmi import _abi, scenes, wavefront

f32 = np.float32
F1 = f32(1)
PAD = 64
CANARY_I = 0x5a5a5a5a
CANARY_F = f32(-7.25)


def v3(*a):
    return np.array(a, dtype=f32)


# ------------------------------------------------------------------ the rule
class RouletteState:
    """The arrays one rtmi_path_roulette reads and writes, on the host: steps (n,) uint32; D, A, T (n, 3) float32 -- the
    scattered directions, layer `step` of the attenuation stack, the throughput --; S (n, 6) uint32, the paths' RNG states;
    counts (2,) uint64."""

    FIELDS = ("steps", "D", "A", "S", "T", "counts")

    def __init__(self, steps, D, A, S, T=None, counts=(3, 5)):
        n = len(D)
        self.steps = np.array(steps, dtype=np.uint32).reshape(n)
        self.D, self.A = np.array(D, dtype=f32).reshape(n, 3), np.array(A, dtype=f32).reshape(n, 3)
        self.S = np.array(S, dtype=np.uint32).reshape(n, 6)
        self.T = np.ones((n, 3), f32) if T is None else np.array(T, dtype=f32).reshape(n, 3)
        self.counts = np.array(counts, dtype=np.uint64)

    def copy(self):
        c = object.__new__(RouletteState)
        for k in self.FIELDS:
            setattr(c, k, getattr(self, k).copy())
        return c


def diff(a, b):
    """The fields in which two RouletteStates differ bit for bit (an empty list: none)."""
    return [k for k in RouletteState.FIELDS
            if not np.array_equal(np.ascontiguousarray(getattr(a, k)).view(np.uint8), np.ascontiguousarray(getattr(b, k)).view(np.uint8))]


def step(ps, step_no, first_step, p_min, cand=None):
    """rtmi_path_roulette in numpy, on a RouletteState in place; returns it.  cand: the candidates' path indices (None:
    all), entries >= n dropped, distinct.  Every product and the division are single binary32 operations; a comparison with
    a NaN is false."""
    n = len(ps.D)
    p_min = f32(p_min)
    c = np.arange(n) if cand is None else np.asarray(cand, dtype=np.int64)
    c = c[c < n]
    c = c[ps.steps[c] == np.uint32(step_no + 1)]  # not stepped: every word is kept
    with np.errstate(all="ignore"):
        ended = (ps.D[c, 0] == 0) & (ps.D[c, 1] == 0) & (ps.D[c, 2] == 0)  # (-0.0 == 0; a NaN is not zero)
        c = c[~ended]
        a, P = ps.A[c].copy(), ps.T[c].copy()
        t = (P * a).astype(f32)
        q = t[:, 0].copy()
        m = t[:, 1] > q
        q[m] = t[m, 1]
        m = t[:, 2] > q
        q[m] = t[m, 2]
        play = (q < F1) if step_no >= first_step else np.zeros(len(c), bool)
        ps.T[c[~play]] = t[~play]
        s, a, P, q = c[play], a[play], P[play], q[play]
        p = np.where(q > p_min, q, p_min).astype(f32)
        u = dl.draw01(ps.S, s)  # CudaRandomFloat(0, 1) of the path's own state, which advances by one draw
        ps.counts[0] += np.uint64(len(s))
        live = u <= p
        inv = (F1 / p).astype(f32)
        a2 = (a * inv[:, None]).astype(f32)
        ps.A[s[live]] = a2[live]
        ps.T[s[live]] = (P[live] * a2[live]).astype(f32)  # not t * inv: the forward product of the stack as it now stands
        dead = s[~live]
        ps.A[dead], ps.D[dead], ps.T[dead] = 0, 0, 0
        ps.counts[1] += np.uint64(len(dead))
    return ps


# ------------------------------------------------------------------ the forward product
def forward(ended_by_hit, steps, E, A, dtype=f32):
    """rtmi_trace_roulette's radiance: where the path ended by its own hit and c = min(steps, layers) > 0, E[c-1] * P with
    P = 1, then P = P * A[k] for k = 0 .. c - 2 ascending, each product rounded on its own; else +0.  E, A (L, n, 3)."""
    E, A = np.asarray(E, dtype=dtype), np.asarray(A, dtype=dtype)
    L, n = E.shape[0], E.shape[1]
    c = np.minimum(np.asarray(steps).astype(np.int64), L)
    P = np.ones((n, 3), dtype=dtype)
    out = np.zeros((n, 3), dtype=dtype)
    on = np.asarray(ended_by_hit).astype(bool) & (c > 0)
    with np.errstate(all="ignore"):
        for k in range(L):
            last = on & (c - 1 == k)
            out[last] = (E[k][last] * P[last]).astype(dtype)
            P = np.where((k < c - 1)[:, None], (P * A[k]).astype(dtype), P)
    return out


# ------------------------------------------------------------------ the loop
def loop_of(b, o, d, seed, depth, first_step, p_min, compact=True, direct=False):
    """The loop trace_steps_roulette on fresh states of `seed`: (Steps, states, the Roulette, killed (n,) bool numpy --
    the paths whose direction a roulette zeroed)."""
    import torch
    n = int(o.shape[0])
    states = rtmi.rng_states(seed, n)
    rule = wavefront.Roulette(first_step, p_min)
    killed = torch.zeros(n, dtype=torch.bool, device=o.device)
    from rtmi import builder
    inner = builder.path_roulette

    def spy(k, r, st, rl, paths=None):  # a path that was alive by its direction before the call and is not after it
        before = (r.directions != 0).any(dim=1)
        out = inner(k, r, st, rl, paths)
        killed.logical_or_(before & ~(r.directions != 0).any(dim=1))
        return out
    builder.path_roulette = spy
    try:
        kw = dict(light_states=rtmi.rng_states(seed, n, first=n)) if direct else {}
        st = b.trace_steps_roulette(o, d, states, depth, rule, compact=compact, direct=direct, **kw).check()
    finally:
        builder.path_roulette = inner
    return st, states, rule, killed.cpu().numpy()


def expected_radiance(st, killed):
    """What rtmi_trace_roulette writes for the loop's paths: the forward product of the loop's stacks for a path that
    ended by its own hit -- not alive, not killed --, else zero."""
    ended_by_hit = ~st.alive.cpu().numpy() & ~killed
    return forward(ended_by_hit, st.steps.cpu().numpy(), st.emitted.cpu().numpy(), st.attenuation.cpu().numpy())


# ------------------------------------------------------------------ device calls
def _guard(a, canary):
    """(the device tensor: PAD canaries, the flat array a, PAD canaries; the view of the body)."""
    import torch
    a = np.ascontiguousarray(a).reshape(-1)
    pad = np.full(PAD, canary, dtype=a.dtype)
    full = np.concatenate([pad, a, pad])
    if full.dtype == np.uint32:
        full = full.view(np.int32)
    elif full.dtype == np.uint64:
        full = full.view(np.int64)
    t = torch.from_numpy(full).cuda()
    return t, t[PAD:PAD + a.size]


def device_step(ps, step_no, first_step, p_min, list_in=None, n_list=None, count_in=None, counts=True):
    """One rtmi_path_roulette through the C ABI on device copies of a RouletteState, canaries around every array; returns
    (rc, the RouletteState as the call left it, whether every canary survived)."""
    import torch
    n = len(ps.D)
    if n_list is None:
        n_list = n if list_in is None else len(list_in)
    ci = np.uint32(CANARY_I)
    dev = {"steps": _guard(ps.steps, ci), "D": _guard(ps.D, CANARY_F), "A": _guard(ps.A, CANARY_F),
           "S": _guard(np.ascontiguousarray(ps.S.T), ci), "T": _guard(ps.T, CANARY_F),
           "counts": _guard(ps.counts, np.uint64(CANARY_I))}
    lst = None if list_in is None else _guard(np.asarray(list_in, dtype=np.uint32), ci)
    cnt = None if count_in is None else _guard(np.array([count_in], dtype=np.uint32), ci)
    a = _abi.PathRouletteArgs()
    a.size, a.reserved, a.reserved2, a.n, a.n_list = C.sizeof(_abi.PathRouletteArgs), 0, 0, n, n_list
    a.step, a.first_step, a.p_min = step_no, first_step, float(f32(p_min))
    a.d_list = None if lst is None else lst[1].data_ptr()
    a.d_count = None if cnt is None else cnt[1].data_ptr()
    a.d_steps, a.d_dirs, a.d_attenuation = dev["steps"][1].data_ptr(), dev["D"][1].data_ptr(), dev["A"][1].data_ptr()
    a.d_states, a.d_throughput = dev["S"][1].data_ptr(), dev["T"][1].data_ptr()
    a.d_counts = dev["counts"][1].data_ptr() if counts else None
    rc = rtmi.lib().rtmi_path_roulette(C.byref(a), C.c_void_p(torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    out, intact = object.__new__(RouletteState), True
    for k in RouletteState.FIELDS:
        ref = getattr(ps, k)
        raw = dev[k][0].cpu().numpy()
        if ref.dtype in (np.uint32, np.uint64):
            raw = raw.view(ref.dtype)
        want = np.full(PAD, CANARY_F if ref.dtype == f32 else CANARY_I, dtype=ref.dtype).view(np.uint8)
        intact = intact and bool((raw[:PAD].view(np.uint8) == want).all() and (raw[PAD + ref.size:].view(np.uint8) == want).all())
        body = raw[PAD:PAD + ref.size]
        setattr(out, k, body.reshape(6, n).T.copy() if k == "S" else body.reshape(ref.shape).copy())
    for t in (lst, cnt):
        if t is not None:
            raw = t[0].cpu().numpy()
            intact = intact and bool((raw[:PAD] == np.int32(CANARY_I)).all() and (raw[-PAD:] == np.int32(CANARY_I)).all())
    return rc, out, intact


def fused(b, o, d, states, depth, first_step, p_min):
    """One rtmi_trace_roulette through the C ABI with canaries around every output: dict of host arrays, and `intact`."""
    import torch
    n = int(o.shape[0])

    def guard(body, dtype):
        full = torch.full((body.numel() + 2 * PAD,), CANARY_I if dtype != torch.float32 else -7.25, dtype=dtype, device="cuda")
        full[PAD:PAD + body.numel()] = body.reshape(-1).to(dtype)
        return full, full[PAD:PAD + body.numel()]

    def intact(full, m):
        c = CANARY_I if full.dtype != torch.float32 else -7.25
        return bool((full[:PAD] == c).all() and (full[PAD + m:] == c).all())
    bufs = {"rgb": guard(torch.full((n, 3), 9.0, device="cuda"), torch.float32), "states": guard(states, torch.int32),
            "rays": guard(torch.full((n,), 77, device="cuda"), torch.int32),
            "counts": guard(torch.zeros(2, device="cuda"), torch.int64),
            "work": guard(torch.zeros(rtmi.TRACE_WORK_WORDS, device="cuda"), torch.int64)}
    a = _abi.TraceRouletteArgs()
    a.size, a.reserved, a.n, a.max_depth = C.sizeof(_abi.TraceRouletteArgs), 0, n, depth
    a.first_step, a.p_min = first_step, float(f32(p_min))
    a.d_origins, a.d_dirs, a.d_states = o.data_ptr(), d.data_ptr(), bufs["states"][1].data_ptr()
    a.d_radiance, a.d_ray_counts = bufs["rgb"][1].data_ptr(), bufs["rays"][1].data_ptr()
    a.d_counts, a.d_work = bufs["counts"][1].data_ptr(), bufs["work"][1].data_ptr()
    rc = rtmi.lib().rtmi_trace_roulette(b.h, C.byref(a), C.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert rc == 0, rtmi.lib().rtmi_last_error()
    torch.cuda.synchronize()
    out = {k: v[1].cpu().numpy() for k, v in bufs.items()}
    out["rgb"], out["states"] = out["rgb"].reshape(n, 3), out["states"].reshape(6, n)
    out["intact"] = all(intact(full, body.numel()) for full, body in bufs.values())
    return out


# ------------------------------------------------------------------ two scenes of the trace tests
def mesh_lamp_room(b):
    """A mesh of a few hundred faces on a Lambertian floor under a parallelogram lamp, a second mesh between them, a wall
    behind: paths that walk the meshes' trees."""
    b.camera_pinhole(v3(0, 1.2, 4), v3(0, 0.6, 0), v3(0, 1, 0), 0.9, 1.0)
    grey = b.lambertian(v3(0.7, 0.7, 0.7))
    b.parallelogram([v3(-5, 0, -5), v3(5, 0, -5), v3(-5, 0, 5)], grey)
    b.parallelogram([v3(-5, 0, -3), v3(5, 0, -3), v3(-5, 6, -3)], b.lambertian(v3(0.4, 0.5, 0.8)))
    b.parallelogram([v3(-1.5, 4, -1.5), v3(1.5, 4, -1.5), v3(-1.5, 4, 1.5)], b.diffuse_light(b.constant_texture(v3(8, 7, 6))))
    low = scenes.procedural_bunny_mesh(8).reshape(-1, 3, 3).astype(f32)
    low = low - low.reshape(-1, 3).min(0) * v3(0, 1, 0)  # on the floor
    b.bvh(low.reshape(-1, 9), b.lambertian(v3(0.8, 0.5, 0.3)))
    high = scenes.procedural_bunny_mesh(6).reshape(-1, 3, 3).astype(f32) * f32(0.6) + v3(0.3, 2.5, 0.2)
    b.bvh(high.reshape(-1, 9), b.lambertian(v3(0.3, 0.7, 0.4)))
    return b


def textured_room(b):
    """One image-textured Lambertian floor under a lamp, a wall behind: A[k] of a floor vertex is a texel."""
    b.camera_pinhole(v3(0, 2, 5), v3(0, 0.5, 0), v3(0, 1, 0), 0.9, 1.0)
    img = np.random.default_rng(5).integers(30, 255, (8, 8, 4)).astype(np.uint8)
    b.parallelogram([v3(-4, 0, -4), v3(4, 0, -4), v3(-4, 0, 4)], b.lambertian_tex(b.image_texture(img)))
    b.parallelogram([v3(-4, 0, -4), v3(4, 0, -4), v3(-4, 5, -4)], b.lambertian(v3(0.6, 0.6, 0.6)))
    b.parallelogram([v3(-1, 3, -1), v3(1, 3, -1), v3(-1, 3, 1)], b.diffuse_light(b.constant_texture(v3(5, 5, 4))))
    return b
