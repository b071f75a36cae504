"""What the tests of rtmi_direct_sample_mis share: the light of a hit and the step restated in numpy from include/rtmi.h
("rtmi_direct_sample_mis"), the close_lamp_room scene, and the device call through the C ABI with canaries behind every
array.  Everything rtmi_direct_sample's tests already have comes from directlib.  No test lives here."""
import ctypes as C

import numpy as np

import directlib as dl
import rtmi
from directlib import CANARY_F, CANARY_I, F0, F1, PAD, f32

INF = f32(np.inf)
MAP_COLS, MAP_ANY = 8, 6  # direct_body.h: kHitLightCols, kHitLightAny


# ------------------------------------------------------------------ the light of a hit
def light_of_hit(tab, H):
    """Per hit record of H ((n, 12) int32) the table light j of the hit, -1 for none: the first j with
    tab[j].entry == hit.entry and, for a PARALLELEPIPED hit, tab[j].element == hit.element.  A hit of another kind than
    TRIANGLE, PARALLELOGRAM or PARALLELEPIPED, one with entry < 0 and one whose entry has no table light has none."""
    H = np.asarray(H, dtype=np.int32).reshape(-1, 12)
    kind, entry, element = H[:, 7], H[:, 8], H[:, 9]
    out = np.full(len(H), -1, dtype=np.int64)
    able = np.isin(kind, dl.SURFACE_KINDS) & (entry >= 0)
    box = kind == rtmi.RTMI_HIT_PARALLELEPIPED
    for j in range(len(tab) - 1, -1, -1):  # (backwards: the first j that fits is the one that stays)
        out[able & (entry == tab["entry"][j]) & (~box | (element == tab["element"][j]))] = j
    return out


def hit_light_map(tab):
    """The map the library makes at commit: int32 (entries, 8), -1 for none.  Row = entry, up to the largest entry of a
    table light; column f < 6 the light of box face f, column 6 the first light of the entry, column 7 padding."""
    rows = int(tab["entry"].max()) + 1 if len(tab) else 0
    m = np.full((rows, MAP_COLS), -1, dtype=np.int32)
    for j in range(len(tab)):
        e, f = int(tab["entry"][j]), int(tab["element"][j])
        if e < 0:
            continue
        if 0 <= f < MAP_ANY and m[e, f] < 0:
            m[e, f] = j
        if m[e, MAP_ANY] < 0:
            m[e, MAP_ANY] = j
    return m


def light_by_map(m, H):
    """light_of_hit through the map, as the kernel reads it: every index checked before it addresses anything."""
    H = np.asarray(H, dtype=np.int32).reshape(-1, 12)
    out = np.full(len(H), -1, dtype=np.int64)
    for i, h in enumerate(H):
        kind, entry, element = int(h[7]), int(h[8]), int(h[9])
        col = -1
        if kind == rtmi.RTMI_HIT_PARALLELEPIPED:
            col = element if 0 <= element < MAP_ANY else -1
        elif kind in (rtmi.RTMI_HIT_TRIANGLE, rtmi.RTMI_HIT_PARALLELOGRAM):
            col = MAP_ANY
        if col >= 0 and 0 <= entry < len(m):
            out[i] = m[entry, col]
    return out


# ------------------------------------------------------------------ the weights
def mis_a(c, cl, scale):
    """a = (c * cl) * scale in binary32: the scattered ray's density over the light sample's is a : d2."""
    with np.errstate(all="ignore"):
        return ((np.asarray(c, f32) * np.asarray(cl, f32)).astype(f32) * np.asarray(scale, f32)).astype(f32)


def scatter_weight(a, d2):
    """WEIGH's w: (a > 0 && d2 > 0 && a + d2 < +inf) ? a / (a + d2) : +0.0f, and whether it came from the division."""
    a, d2 = np.asarray(a, f32), np.asarray(d2, f32)
    with np.errstate(all="ignore"):
        s = (a + d2).astype(f32)
        div = (a > 0) & (d2 > 0) & (s < INF)
        w = np.where(div, (a / s).astype(f32), F0).astype(f32)
    return w, div


def light_weight(a, d2):
    """The balance weight of the light sample, d2 / (a + d2): SAMPLE's g = a / (a + d2) is (a / d2) times it."""
    a, d2 = np.asarray(a, f32), np.asarray(d2, f32)
    with np.errstate(all="ignore"):
        return (d2 / (a + d2).astype(f32)).astype(f32)


def sample_g(a, d2):
    """SAMPLE's g = a / (a + d2) in binary32."""
    a, d2 = np.asarray(a, f32), np.asarray(d2, f32)
    with np.errstate(all="ignore"):
        return (a / (a + d2).astype(f32)).astype(f32)


# ------------------------------------------------------------------ the step
class PathState(dl.PathState):
    """directlib.PathState and the carry C (n, 4) float32, which starts as recognisable junk unless given."""

    FIELDS = dl.PathState.FIELDS + ("C",)

    def __init__(self, O, D, H, steps, E, A, LS, flags=None, seed=5, carry=None):
        dl.PathState.__init__(self, O, D, H, steps, E, A, LS, flags, seed)
        n = len(self.O)
        self.C = (np.random.default_rng(seed + 3 * n).uniform(0.25, 1, (n, 4)).astype(f32) if carry is None
                  else np.array(carry, dtype=f32).reshape(n, 4))

    @classmethod
    def of(cls, ps, carry=None):
        """A directlib.PathState with a carry added (the arrays are copied)."""
        out = cls(ps.O, ps.D, ps.H, ps.steps, ps.E, ps.A, ps.LS, ps.flags, carry=carry)
        for k in dl.PathState.FIELDS:
            setattr(out, k, getattr(ps, k).copy())
        return out

    def copy(self):
        c = object.__new__(PathState)
        for k in self.FIELDS:
            setattr(c, k, getattr(self, k).copy())
        return c


def step(tab, mat_kinds, ps, step_no, sample, cand=None):
    """rtmi_direct_sample_mis in numpy, on a PathState (with carry) in place; the arguments are directlib.step's."""
    n = len(ps.O)
    c = np.arange(n) if cand is None else np.asarray(cand, dtype=np.int64)
    c = c[c < n]
    mat_kinds = np.asarray(mat_kinds, dtype=np.int64)
    ps.SD[c], ps.DR[c], ps.ST[c] = 0, 0, 0
    was = (ps.flags[c] & 1) != 0
    ps.flags[c] &= ~np.uint32(1)
    stepped = ps.steps[c] == step_no + 1
    s, was = c[stepped], was[stepped]
    # WEIGH
    lj = light_of_hit(tab, ps.H[s])
    wg = was & (lj >= 0)
    i, j = s[wg], lj[wg]
    if len(i):
        cw = ps.C[i]
        with np.errstate(all="ignore"):
            cl = np.abs(dl._dot(tab["n"][j], cw[:, :3]))
            t = ps.H[i, 0].view(f32)
            d2 = (t * t).astype(f32)
            w, div = scatter_weight(mis_a(cw[:, 3], cl, tab["scale"][j]), d2)
            ps.E[i] = np.where(div[:, None], (ps.E[i] * w[:, None]).astype(f32), F0)
    ps.counts[1] += np.uint64(len(i))
    # SAMPLE
    mat = ps.H[s, 6].astype(np.int64)
    mat_ok = (mat >= 0) & (mat < len(mat_kinds))
    msafe = np.where(mat_ok, mat, 0)
    scattered = (ps.D[s] != 0).any(1)
    samp = scattered & mat_ok & ((mat_kinds[msafe] == dl.LAMBERTIAN) if len(mat_kinds) else False)
    if not sample or len(tab) == 0:
        samp[:] = False
    p = s[samp]
    ps.flags[p] |= np.uint32(1)
    ps.counts[0] += np.uint64(len(p))
    if len(p) == 0:
        return ps
    r0, r1, r2 = dl.draw01(ps.LS, p), dl.draw01(ps.LS, p), dl.draw01(ps.LS, p)
    j = np.searchsorted(tab["cdf"], r0, side="left")  # the smallest j with r0 <= cdf[j]
    with np.errstate(all="ignore"):
        flip = (tab["kind"][j] == 1) & ((r1 + r2).astype(f32) > F1)
        r1, r2 = np.where(flip, (F1 - r1).astype(f32), r1), np.where(flip, (F1 - r2).astype(f32), r2)
        p0, e1, e2, ln = tab["p0"][j], tab["e1"][j], tab["e2"][j], tab["n"][j]
        q = ((p0 + (r1[:, None] * e1).astype(f32)).astype(f32) + (r2[:, None] * e2).astype(f32)).astype(f32)
        x = ps.O[p]
        w = (q - x).astype(f32)
        d2 = dl._dot(w, w)
        dist = np.sqrt(d2).astype(f32)
        wi = (w / dist[:, None]).astype(f32)
        N = ps.H[p, 3:6].view(f32)
        cs = dl._dot(N, wi)
        cl = np.abs(dl._dot(ln, wi))
        valid = (d2 > 0) & (cs > 0) & (cl > 0) & (dist < INF)
        g = sample_g(mis_a(cs, cl, tab["scale"][j]), d2)
        dr = ((ps.A[p] * tab["emission"][j]).astype(f32) * g[:, None]).astype(f32)
        tm = (dist * f32(0.999)).astype(f32)
        ps.C[p] = np.concatenate([ps.D[p], dl._dot(N, ps.D[p])[:, None]], axis=1)
    v = p[valid]
    ps.SO[v], ps.SD[v], ps.ST[v], ps.DR[v] = x[valid], wi[valid], tm[valid], dr[valid]
    return ps


# ------------------------------------------------------------------ the close_lamp_room scene
class _Moved:
    """A builder that passes every call on, with directlib.lamp_room's lamp moved from y = 8.5 to y = 9.9 (0.1 under the
    ceiling) and its emissive triangle from x = 1.5 to x = 0.1 (0.1 off the red wall)."""

    def __init__(self, b):
        self.b = b

    def __getattr__(self, name):
        return getattr(self.b, name)

    def parallelogram(self, pts, mat):
        pts = [np.array(p, dtype=f32) for p in pts]
        if all(p[1] == f32(8.5) for p in pts):
            for p in pts:
                p[1] = f32(9.9)
        return self.b.parallelogram(pts, mat)

    def triangle(self, pts, mat):
        pts = [np.array(p, dtype=f32) for p in pts]
        if all(p[0] == f32(1.5) for p in pts):
            for p in pts:
                p[0] = f32(0.1)
        return self.b.triangle(pts, mat)


def close_lamp_room(b):
    """directlib.lamp_room with both lights 0.1 from a diffuse wall: where rtmi_direct_sample's estimate is unbounded."""
    dl.lamp_room(_Moved(b))
    return b


CLOSE_LAMP_ROOM_SEED = dl.LAMP_ROOM_SEED


# ------------------------------------------------------------------ device calls
def mis_args(n, lst, n_list, cnt, step_no, sample, dev, counts=True):
    """rtmi_direct_sample_mis_args over the device tensors dev[...] (directlib's names, and "C" the carry)."""
    a = rtmi.DirectSampleMisArgs()
    val = lambda t: t.data_ptr() if t is not None else None
    a.size, a.reserved, a.n, a.n_list, a.step, a.sample = C.sizeof(rtmi.DirectSampleMisArgs), 0, n, n_list, step_no, 1 if sample else 0
    a.d_list, a.d_count = val(lst), val(cnt)
    a.d_origins, a.d_dirs, a.d_hits, a.d_steps = val(dev["O"]), val(dev["D"]), val(dev["H"]), val(dev["steps"])
    a.d_emitted, a.d_attenuation, a.d_light_states, a.d_flags = val(dev["E"]), val(dev["A"]), val(dev["LS"]), val(dev["flags"])
    a.d_shadow_origins, a.d_shadow_dirs, a.d_shadow_t_max, a.d_direct = val(dev["SO"]), val(dev["SD"]), val(dev["ST"]), val(dev["DR"])
    a.d_carry, a.d_counts = val(dev["C"]), val(dev["counts"]) if counts else None
    return a


def device_step(b, ps, step_no, sample, list_in=None, n_list=None, count_in=None, counts=True, mis=True):
    """One rtmi_direct_sample_mis (mis=False: one rtmi_direct_sample, the carry untouched) through the C ABI on device
    copies of a PathState, canaries behind every array; returns (rc, the PathState as the call left it, whether every
    canary survived)."""
    import torch
    n = len(ps.O)
    if n_list is None:
        n_list = n if list_in is None else len(list_in)
    ci = np.uint32(CANARY_I)
    g = dl._guarded
    dev = {"O": g(ps.O, CANARY_F), "D": g(ps.D, CANARY_F), "H": g(ps.H, np.int32(CANARY_I)), "steps": g(ps.steps, ci),
           "E": g(ps.E, CANARY_F), "A": g(ps.A, CANARY_F), "LS": g(np.ascontiguousarray(ps.LS.T), ci), "flags": g(ps.flags, ci),
           "SO": g(ps.SO, CANARY_F), "SD": g(ps.SD, CANARY_F), "ST": g(ps.ST, CANARY_F), "DR": g(ps.DR, CANARY_F),
           "counts": g(ps.counts, np.uint64(CANARY_I)), "C": g(ps.C, CANARY_F)}
    lst = None if list_in is None else g(np.asarray(list_in, dtype=np.uint32), ci)
    cnt = None if count_in is None else g(np.array([count_in], dtype=np.uint32), ci)
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    p = dl.ptr
    if mis:
        a = mis_args(n, lst, n_list, cnt, step_no, sample, dev, counts)
        rc = rtmi.lib().rtmi_direct_sample_mis(b.h, C.byref(a), stream)
    else:
        rc = rtmi.lib().rtmi_direct_sample(b.h, n, p(lst), n_list, p(cnt), step_no, 1 if sample else 0, p(dev["O"]), p(dev["D"]),
                                           p(dev["H"]), p(dev["steps"]), p(dev["E"]), p(dev["A"]), p(dev["LS"]), p(dev["flags"]),
                                           p(dev["SO"]), p(dev["SD"]), p(dev["ST"]), p(dev["DR"]),
                                           p(dev["counts"]) if counts else None, stream)
    torch.cuda.synchronize()
    out, intact = object.__new__(PathState), True
    for k in PathState.FIELDS:
        ref = getattr(ps, k)
        raw = dev[k].cpu().numpy()
        if ref.dtype in (np.uint32, np.uint64):
            raw = raw.view(ref.dtype)
        body, tail = raw[:ref.size], raw[ref.size:]
        intact = intact and bool((tail.view(np.uint8) == np.full(PAD, CANARY_F if ref.dtype == f32 else CANARY_I,
                                                                  dtype=ref.dtype).view(np.uint8)).all())
        setattr(out, k, body.reshape(6, n).T.copy() if k == "LS" else body.reshape(ref.shape).copy())
    return rc, out, intact


def diff(a, b):
    """The fields in which two PathStates (with carry) differ bit for bit (an empty list: none)."""
    return [k for k in PathState.FIELDS
            if not np.array_equal(np.ascontiguousarray(getattr(a, k)).view(np.uint8), np.ascontiguousarray(getattr(b, k)).view(np.uint8))]
