"""What the rtmi_path_compact / rtmi_bounce_list tests share: "live" and the compaction restated in numpy (held to
hand-worked cases by tests/test_bounce_list_host.py), ray patterns with the bad-ray kinds mixed in, and the device calls
through the C ABI with canaries around every output.  No test lives here."""
import ctypes as C

import numpy as np

import rtmi
from querylib import glm_normalize

P = rtmi.PATH_COMPACT_ITEMS  # list entries one workgroup of the compaction handles (include/rtmi.h: RTMI_PATH_COMPACT_ITEMS)
SCAN_THREADS = 256           # paths.hip: kCompactScanThreads -- each lane of the scan sums ceil(workgroups / 256) counts
CANARY_INDEX = 0x5a5a5a5a
CANARY_F = np.float32(-7.25)


# ------------------------------------------------------------------ the restatements
def live(O, D):
    """The paths the next step would step: finite origin and direction, a direction that is not the zero vector (-0.0
    counts as zero) and that Ray's constructor normalises to a finite non-zero vector.  O, D (n, 3) float32."""
    O, D = np.asarray(O, dtype=np.float32).reshape(-1, 3), np.asarray(D, dtype=np.float32).reshape(-1, 3)
    with np.errstate(all="ignore"):
        u = glm_normalize(D) if len(D) else D
    return np.isfinite(O).all(1) & np.isfinite(D).all(1) & (D != 0).any(1) & np.isfinite(u).all(1) & (u != 0).any(1)


def candidates(n, list_in=None, n_list=None, count_in=None):
    """The candidate entries of a list, in order: list_in[:min(n_list, count_in)] (list_in None: 0, 1, 2, ...)."""
    if n_list is None:
        n_list = n if list_in is None else len(list_in)
    end = n_list if count_in is None else min(n_list, int(count_in))
    if list_in is None:
        assert n_list <= n
        return np.arange(end, dtype=np.int64)
    return np.asarray(list_in, dtype=np.uint32).astype(np.int64)[:end]


def compact(O, D, list_in=None, n_list=None, count_in=None):
    """rtmi_path_compact in numpy: the live candidates' path indices in the candidates' order (entries >= n dropped)."""
    n = len(O)
    c = candidates(n, list_in, n_list, count_in)
    c = c[c < n]
    return c[live(O, D)[c]].astype(np.uint32)


# ------------------------------------------------------------------ ray patterns
BAD_KINDS = ("neg_zero_dir", "nan_origin", "inf_dir", "tiny_dir", "huge_dir", "zero_dir", "inf_origin")


def make_bad(O, D, i, kind):
    """Turn path i of (O, D) into a bad ray of the named kind, in place."""
    if kind == "neg_zero_dir":
        D[i] = (-0.0, 0.0, -0.0)
    elif kind == "zero_dir":
        D[i] = 0.0
    elif kind == "nan_origin":
        O[i, 1] = np.nan
    elif kind == "inf_origin":
        O[i, 2] = -np.inf
    elif kind == "inf_dir":
        D[i, 0] = np.inf
    elif kind == "tiny_dir":
        D[i] = (1e-30, 0.0, 0.0)  # |d|^2 underflows to 0: the direction does not normalise
    elif kind == "huge_dir":
        D[i] = (1e30, 1e30, 0.0)  # |d|^2 overflows: normalises to zero
    else:
        raise ValueError(kind)


def rays(n, pattern, seed=0):
    """(O, D) of n paths whose live ones follow `pattern`: all, none, alternating, last, sparse (about one live in 64,
    random), mixed (half live at random, the dead ones of every bad kind in turn).  The dead paths of the other patterns
    are ended paths (zero direction)."""
    rng = np.random.default_rng(1000 + seed + n)
    O = rng.uniform(-1, 1, (n, 3)).astype(np.float32)
    D = rng.uniform(-1, 1, (n, 3)).astype(np.float32)
    D[(D == 0).all(1)] = (0, 1, 0)
    idx = np.arange(n)
    if pattern == "all":
        dead = np.zeros(n, bool)
    elif pattern == "none":
        dead = np.ones(n, bool)
    elif pattern == "alternating":
        dead = idx % 2 == 1
    elif pattern == "last":
        dead = idx != n - 1
    elif pattern == "sparse":
        dead = rng.integers(0, 64, n) != 0
    elif pattern == "mixed":
        dead = rng.integers(0, 2, n) == 0
        for k, i in enumerate(np.flatnonzero(dead)):
            make_bad(O, D, i, BAD_KINDS[k % len(BAD_KINDS)])
        return O, D
    else:
        raise ValueError(pattern)
    D[dead] = 0.0
    return O, D


PATTERNS = ("all", "none", "alternating", "last", "sparse", "mixed")


# ------------------------------------------------------------------ device calls
def ptr(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


def dev_u32(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(np.asarray(a, dtype=np.uint32)).view(np.int32)).cuda()


class Compaction:
    """One rtmi_path_compact through the C ABI on device copies of the rays, `pad` canary words behind the output list's
    n_list entries, everything read back: out (the first count entries), count, tail (everything from count on, canaries
    behind the capacity included), O / D as the call left them."""

    def __init__(self, O, D, list_in=None, n_list=None, count_in=None, pad=64, stream=None):
        import torch
        n = len(O)
        if n_list is None:
            n_list = n if list_in is None else len(list_in)
        self.n, self.n_list = n, n_list
        self.o = torch.from_numpy(np.ascontiguousarray(O, dtype=np.float32).reshape(n, 3)).cuda()
        self.d = torch.from_numpy(np.ascontiguousarray(D, dtype=np.float32).reshape(n, 3)).cuda()
        self.list_in = None if list_in is None else dev_u32(list_in)
        self.count_in = None if count_in is None else dev_u32([count_in])
        self.list_out = torch.full((n_list + pad,), CANARY_INDEX, dtype=torch.int32, device="cuda")
        self.count_out = torch.full((3,), CANARY_INDEX, dtype=torch.int32, device="cuda")  # the count in the middle word
        words = rtmi.lib().rtmi_path_compact_scratch_bytes(n_list) // 4
        self.scratch = torch.full((words + 2,), CANARY_INDEX, dtype=torch.int32, device="cuda")
        self.scratch_words = words
        self.rc = self.call(stream)

    def call(self, stream=None):
        import torch
        s = torch.cuda.current_stream() if stream is None else stream
        if stream is not None:
            stream.wait_stream(torch.cuda.current_stream())
        return rtmi.lib().rtmi_path_compact(self.n, ptr(self.o), ptr(self.d), ptr(self.list_in), self.n_list, ptr(self.count_in),
                                            ptr(self.list_out), C.c_void_p(self.count_out.data_ptr() + 4),
                                            C.c_void_p(self.scratch.data_ptr() + 4), C.c_void_p(s.cuda_stream))

    def read(self):
        import torch
        torch.cuda.synchronize()
        cnt = self.count_out.cpu().numpy().view(np.uint32)
        self.count = int(cnt[1])
        self.count_guard = (int(cnt[0]), int(cnt[2]))
        full = self.list_out.cpu().numpy().view(np.uint32)
        self.out, self.tail = full[:min(self.count, len(full))], full[min(self.count, len(full)):]
        sc = self.scratch.cpu().numpy().view(np.uint32)
        self.scratch_guard = (int(sc[0]), int(sc[-1]))
        self.O, self.D = self.o.cpu().numpy(), self.d.cpu().numpy()
        return self


def check_compaction(c, O, D, want):
    """Compaction c (read) wrote exactly `want` and its count, and nothing else."""
    from parity import bits
    assert c.rc == 0, rtmi.lib().rtmi_last_error()
    assert c.count == len(want), (c.count, len(want))
    assert np.array_equal(c.out, want), np.flatnonzero(c.out != want)[:8]
    assert (c.tail == CANARY_INDEX).all(), "entries from the count on were written"
    assert c.count_guard == (CANARY_INDEX,) * 2 and c.scratch_guard == (CANARY_INDEX,) * 2
    assert np.array_equal(bits(c.O), bits(np.asarray(O, np.float32).reshape(-1, 3)))
    assert np.array_equal(bits(c.D), bits(np.asarray(D, np.float32).reshape(-1, 3)))
