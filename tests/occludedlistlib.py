"""What the rtmi_occluded_list tests share: the ways to name a list, the device call through the C ABI with the output
pre-filled and canary bytes behind it, the expectation made from rtmi_occluded's own answers, and the g8 world of
tests/test_gpu_occluded.py restated.  No test lives here."""
import ctypes as C

import numpy as np

import rtmi
from bouncelistlib import candidates, dev_u32, ptr
from querylib import v3

FILL = 0xA5    # what the output holds before the call: neither 0 nor 1
PAD = 64       # canary bytes behind the n answers
LIST_KINDS = ("null_short", "null_count", "count_above", "count_zero", "subset", "subset_strays", "duplicates")


def make_list(kind, n, rng):
    """(list_in or None, n_list, count_in or None) of one way to name a list over n paths.
    null_short: a null list with n_list < n; null_count: a null list, the count word below n_list; count_above: an explicit
    list whose count word lies above n_list; count_zero: a count of 0; subset: an explicit shuffled subset; subset_strays:
    the same subset with entries n and 0xFFFFFFFF sprinkled in; duplicates: entries that repeat."""
    half = (n + 1) // 2
    sub = rng.permutation(n)[:half].astype(np.uint32)
    if kind == "null_short":
        return None, n - n // 3 if n > 1 else 0, None
    if kind == "null_count":
        return None, n, n // 2
    if kind == "count_above":
        return sub, len(sub), len(sub) + 7
    if kind == "count_zero":
        return sub, len(sub), 0
    if kind == "subset":
        return sub, len(sub), None
    if kind == "subset_strays":
        lst = np.empty(len(sub) + (len(sub) + 2) // 3, dtype=np.uint32)
        stray = np.zeros(len(lst), bool)
        stray[rng.permutation(len(lst))[:len(lst) - len(sub)]] = True
        lst[~stray] = sub
        lst[stray] = np.where(np.arange(stray.sum()) % 2 == 0, np.uint32(n), np.uint32(0xFFFFFFFF))
        return lst, len(lst), None
    if kind == "duplicates":
        return rng.integers(0, n, n + 5).astype(np.uint32), n + 5, None  # (more entries than paths: some path repeats)
    raise ValueError(kind)


def listed(n, list_in, n_list, count_in):
    """The candidates that are paths, in the list's order, one per occurrence (int64)."""
    c = candidates(n, list_in, n_list, count_in)
    return c[c < n]


class Rays:
    """Device copies of a batch (O, D (n, 3) float32; tm (n,) float32 or None)."""

    def __init__(self, O, D, tm=None):
        import torch
        self.n = len(O)
        self.o = torch.from_numpy(np.ascontiguousarray(O, dtype=np.float32).reshape(self.n, 3)).cuda()
        self.d = torch.from_numpy(np.ascontiguousarray(D, dtype=np.float32).reshape(self.n, 3)).cuda()
        self.tm = None if tm is None else torch.from_numpy(np.ascontiguousarray(tm, dtype=np.float32)).cuda()

    def gather(self, idx):
        import torch
        i = torch.from_numpy(np.ascontiguousarray(idx, dtype=np.int64)).cuda()
        r = Rays.__new__(Rays)
        r.n, r.o, r.d = len(idx), self.o[i].contiguous(), self.d[i].contiguous()
        r.tm = None if self.tm is None else self.tm[i].contiguous()
        return r


def occluded(b, r):
    """rtmi_occluded on the batch: (answers (n,) uint8 numpy, counts (2,) int64 numpy)."""
    if r.n == 0:
        return np.zeros(0, np.uint8), np.zeros(2, np.int64)
    q = b.occluded(r.o, r.d, r.tm)
    return q.raw.cpu().numpy(), q.counts.cpu().numpy()


def occluded_list(b, r, list_in, n_list, count_in, counts=True, lib=None, check=False):
    """One rtmi_occluded_list through the C ABI, the output pre-filled with FILL and PAD canary bytes behind it.  Returns
    (rc, the n answer bytes, counts (2,) int64 or None, whether the canaries survived[, check words (2,)])."""
    import torch
    L = rtmi.lib() if lib is None else lib
    out = torch.full((r.n + PAD,), FILL, dtype=torch.uint8, device="cuda")
    lst = None if list_in is None else dev_u32(list_in)
    cnt = None if count_in is None else dev_u32([count_in])
    words = torch.zeros((4,), dtype=torch.int64, device="cuda")  # abandoned, fallback | re-done, disagreements
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    if check:
        fn = L.rtmi_occluded_list_check_counts
        fn.restype = C.c_int
        fn.argtypes = [C.c_void_p, C.c_int64, C.c_void_p, C.c_int64] + [C.c_void_p] * 8
        rc = fn(b.h, r.n, ptr(lst), n_list, ptr(cnt), ptr(r.o), ptr(r.d), ptr(r.tm), ptr(out), ptr(words),
                C.c_void_p(words.data_ptr() + 16), stream)
    else:
        rc = L.rtmi_occluded_list(b.h, r.n, ptr(lst), n_list, ptr(cnt), ptr(r.o), ptr(r.d), ptr(r.tm), ptr(out),
                                  ptr(words) if counts else None, stream)
    full = out.cpu().numpy()
    w = words.cpu().numpy()
    res = (rc, full[:r.n], w[:2] if counts else None, bool((full[r.n:] == FILL).all()))
    return res + (w[2:],) if check else res


def expect(ref, n, list_in, n_list, count_in):
    """The bytes after the call: FILL everywhere, rtmi_occluded's byte (ref) at the listed paths."""
    want = np.full(n, FILL, dtype=np.uint8)
    at = listed(n, list_in, n_list, count_in)
    want[at] = ref[at]
    return want


def check_list(b, r, ref, list_in, n_list, count_in, what):
    """The list call writes exactly expect(...), keeps the canaries, and counts what rtmi_occluded counts on the gathered
    candidate rays.  Returns the counts."""
    rc, got, counts, intact = occluded_list(b, r, list_in, n_list, count_in)
    assert rc == 0, (what, rtmi.lib().rtmi_last_error())
    assert intact, (what, "bytes behind the output were written")
    want = expect(ref, r.n, list_in, n_list, count_in)
    bad = np.flatnonzero(got != want)
    assert len(bad) == 0, (what, len(bad), [(int(i), int(got[i]), int(want[i])) for i in bad[:8]])
    at = listed(r.n, list_in, n_list, count_in)
    g_ans, g_counts = occluded(b, r.gather(at))
    assert np.array_equal(g_ans, ref[at]), (what, "the gathered call disagrees with the full one")
    assert np.array_equal(counts, g_counts), (what, counts.tolist(), g_counts.tolist())
    return counts


# ------------------------------------------------------------------ the g8 world (tests/test_gpu_occluded.py: g8_world)
def g8_world(b, with_sphere=False):
    """A mesh of four faces, two reference leaves (k_min = 2; faces sort by their first vertex's x): leaf 0 holds a wall at
    x = 5 and a face in the plane y = -1 that stretches its box to x in [2, 10].  A ray from inside that box along +x meets
    the wall at t = 5 - x0, but leaves the box at t = 10 - x0: with t_to below that, AABB::Hit refuses the box (quirk g8),
    while the unbounded walk enters it and hits the wall.  Leaf 1 makes the mesh 600 long, so that a t_max below 30 keeps
    the bounded walk."""
    b.camera_pinhole(v3(0, 0, 30), v3(5, 0, 0), v3(0, 1, 0), 0.9, 1.0)
    m = b.lambertian(v3(0.5, 0.5, 0.5))
    faces = np.array([
        [2, -1, -1, 10, -1, -1, 10, -1, 1.5],
        [5, -1, -1, 5, 1, -1, 5, 0, 1.5],
        [500, 5, 5, 501, 5, 5, 500, 6, 5],
        [600, 5, 5, 601, 5, 5, 600, 6, 5],
    ], dtype=np.float32)
    b.bvh(faces, m, k_min=2)
    if with_sphere:
        b.sphere(v3(0, 30, 0), 1.0, m)  # (binary64 records: the other engine type)


def g8_rays(n, seed=2):
    """Rays from inside leaf 0's box along +x with t_max between the wall and the box's exit (every fourth beyond the
    exit): all occluded, three in four only through the fallback."""
    rng = np.random.default_rng(seed)
    x0 = rng.uniform(2.2, 4.8, n).astype(np.float32)
    O = np.stack([x0, rng.uniform(-0.3, 0.3, n), rng.uniform(-0.3, 0.3, n)], 1).astype(np.float32)
    D = np.tile(np.array([[1, 0, 0]], dtype=np.float32), (n, 1))
    wall, leave = (np.float32(5) - x0), (np.float32(10) - x0)
    tm = (wall + rng.uniform(0.05, 0.95, n).astype(np.float32) * (leave - wall)).astype(np.float32)
    tm[::4] = (leave[::4] + np.float32(1)).astype(np.float32)
    return O, D, tm
