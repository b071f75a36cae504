"""rtmi_trace_direct restated: the forward sum of the direct light along a path (include/rtmi.h), in binary32 as the kernel
forms it and in binary64 beside the backward fold it replaces, and the oracle of the GPU tests -- the loop
trace_steps(compact=True, direct="mis") on copies of the states, folded forward."""
import numpy as np

f32 = np.float32


def forward_direct(A, D, occ, steps):
    """acc of include/rtmi.h in binary32: acc = +0, P = 1; for k = 0 .. c - 1: V = occ[k] ? +0 : D[k]; acc = acc + P * V;
    P = P * A[k], product and sum rounded on their own.  A, D (L, n, 3) float32; occ (L, n); steps (n,): c = min(steps, L)."""
    A, D = np.asarray(A, dtype=f32), np.asarray(D, dtype=f32)
    occ = np.asarray(occ).astype(bool)
    L, n = D.shape[0], D.shape[1]
    acc, P = np.zeros((n, 3), dtype=f32), np.ones((n, 3), dtype=f32)
    c = np.minimum(np.asarray(steps).astype(np.int64), L)
    with np.errstate(all="ignore"):
        for k in range(L):
            on = (k < c)[:, None]
            V = np.where(occ[k][:, None], f32(0), D[k])
            acc = np.where(on, (acc + (P * V).astype(f32)).astype(f32), acc)
            P = np.where(on, (P * A[k]).astype(f32), P)
    return acc


def forward_direct_skipping(A, D, occ, steps):
    """forward_direct as the kernel runs it: a layer whose V is a zero of either sign adds nothing and is skipped."""
    A, D = np.asarray(A, dtype=f32), np.asarray(D, dtype=f32)
    occ = np.asarray(occ).astype(bool)
    L, n = D.shape[0], D.shape[1]
    acc, P = np.zeros((n, 3), dtype=f32), np.ones((n, 3), dtype=f32)
    c = np.minimum(np.asarray(steps).astype(np.int64), L)
    with np.errstate(all="ignore"):
        for k in range(L):
            V = np.where(occ[k][:, None], f32(0), D[k])
            on = (k < c) & (V != 0).any(axis=1)  # (a layer with any non-zero channel is added whole)
            acc = np.where(on[:, None], (acc + (P * V).astype(f32)).astype(f32), acc)
            P = np.where((k < c)[:, None], (P * A[k]).astype(f32), P)
    return acc


def path_fold64(ended, steps, E, A):
    """rtmi_path_fold in binary64 (bouncelib.fold's rule)."""
    E, A = np.asarray(E, dtype=np.float64), np.asarray(A, dtype=np.float64)
    L, n = E.shape[0], E.shape[1]
    out = np.zeros((n, 3))
    for i in range(n):
        c = min(int(steps[i]), L)
        r, k = np.zeros(3), c - 1
        if c > 0 and ended[i]:
            r, k = E[k, i].copy(), k - 1
        while k >= 0:
            r = E[k, i] + A[k, i] * r
            k -= 1
        out[i] = r
    return out


def forward64(ended, steps, E, A, D, occ):
    """r_path + acc in binary64, and the sum of the absolute values of the terms it adds (the scale of its rounding)."""
    E, A, D = (np.asarray(x, dtype=np.float64) for x in (E, A, D))
    occ = np.asarray(occ).astype(bool)
    L, n = E.shape[0], E.shape[1]
    r_path = path_fold64(ended, steps, E, A)
    acc, P, mag = np.zeros((n, 3)), np.ones((n, 3)), np.abs(path_fold64(ended, steps, np.abs(E), np.abs(A)))
    for k in range(L):
        on = (k < np.minimum(steps, L))[:, None]
        V = np.where(occ[k][:, None], 0.0, D[k])
        acc = np.where(on, acc + P * V, acc)
        mag = np.where(on, mag + np.abs(P * V), mag)
        P = np.where(on, P * A[k], P)
    return r_path + acc, mag


def backward64(ended, steps, E, A, D, occ):
    """rtmi_path_fold_direct in binary64 (directlib.fold_direct's rule): rtmi_path_fold with T[k] = occ[k] ? E[k] : E[k] + D[k]."""
    E, D = np.asarray(E, dtype=np.float64), np.asarray(D, dtype=np.float64)
    T = np.where(np.asarray(occ).astype(bool)[..., None], E, E + D)
    return path_fold64(ended, steps, T, A)


def random_stacks(rng, c, n, alive):
    """n paths of c steps each with non-negative random stacks of max(c, 1) layers, as a loop leaves them: a layer that
    scatters has E = 0 and an attenuation, the last layer of an ended path has an emission, A = 0 and samples nothing; about
    a third of the layers sample, a third of those are occluded.  Returns (dirs, steps, E, A, D, occ), binary32."""
    L = max(c, 1)
    E, A, D = np.zeros((L, n, 3), f32), np.zeros((L, n, 3), f32), np.zeros((L, n, 3), f32)
    occ = np.zeros((L, n), np.uint8)
    for k in range(c):
        last = k == c - 1 and not alive
        if last:
            E[k] = rng.uniform(0, 8, (n, 3)).astype(f32)
        else:
            A[k] = rng.uniform(0.05, 1, (n, 3)).astype(f32)
            s = rng.random(n) < 0.35
            D[k][s] = rng.uniform(0, 4, (int(s.sum()), 3)).astype(f32)
            occ[k] = (s & (rng.random(n) < 0.3)).astype(np.uint8)
    dirs = np.zeros((n, 3), f32)
    if alive and c > 0:
        dirs[:, 2] = 1
    return dirs, np.full(n, c, np.int32), E, A, D, occ


# ------------------------------------------------------------------ the oracle of the GPU tests
def loop_of(b, o, d, seed, depth):
    """The loop on fresh states of `seed`: (Steps, states, light_states, counts (2,) int64 tensor of the loop's
    direct_sample calls)."""
    import rtmi
    n = int(o.shape[0])
    states, ls = rtmi.rng_states(seed, n), rtmi.rng_states(seed, n, first=n)
    seen = {}
    inner = b.direct_sample

    def spy(*a, **kw):  # the loop hands every step the one counts tensor
        seen["counts"] = kw["counts"]
        return inner(*a, **kw)
    b.direct_sample = spy
    try:
        st = b.trace_steps(o, d, states, depth, compact=True, direct="mis", light_states=ls).check()
    finally:
        del b.direct_sample
    return st, states, ls, seen.get("counts")


def expected_radiance(st):
    """path_fold over the loop's stacks + the forward sum, one binary32 addition: what rtmi_trace_direct writes."""
    import rtmi
    r_path = rtmi.path_fold(st.directions, st.steps, st.emitted, st.attenuation).cpu().numpy()
    acc = forward_direct(st.attenuation.cpu().numpy(), st.direct.cpu().numpy(), st.occluded.cpu().numpy(), st.steps.cpu().numpy())
    with np.errstate(all="ignore"):
        return (r_path + acc).astype(f32)
