"""What the budget, feature and adaptive tests share: the stopping and resolve rules restated in numpy, every shard of a
frame on the one GPU (Shards), and the oracle driven a sample at a time (OracleReplay)."""
import numpy as np

import common
import oraclelib
import rtmi
from parity import same

try:
    import torch
except ImportError:  # the rules are host code; only Shards needs a device
    torch = None

F32 = np.float32


# ------------------------------------------------------------------ the stopping rule, restated
def plan_rule(n, S, Q, min_n, max_n, step, tolerance, floor, pixel=None):
    """rtmi_budget_plan in numpy, operation by operation as include/rtmi.h states it.  n (N,) uint32, S, Q (N, 3)
    float32, pixel (N,) bool (False: padding).  Returns the (N,) uint32 budgets."""
    n = np.asarray(n, dtype=np.uint32)
    S, Q = np.asarray(S, dtype=F32), np.asarray(Q, dtype=F32)
    T, Fl = F32(tolerance), F32(floor)
    with np.errstate(all="ignore"):
        nf = n.astype(F32)[:, None]
        a = nf * Q
        b = S * S
        c = a - b
        d = nf - F32(1.0)
        lhs = c / d
        e = T * T
        g = nf * nf
        h = Fl * Fl
        i = g * h
        j = b + i
        rhs = e * j
        converged = (lhs <= rhs).all(axis=1)  # (a NaN compares false)
    for x in (a, b, c, d, lhs, g, i, j, rhs):
        assert x.dtype == F32
    n64 = n.astype(np.int64)
    more = np.minimum(step, max_n - n64)
    out = np.where(n64 < min_n, min_n - n64, np.where(n64 >= max_n, 0, np.where(converged, 0, more)))
    if pixel is not None:
        out = np.where(pixel, out, 0)
    return out.astype(np.uint32)


def moments(samples):
    """(n, S, Q) of one pixel whose three channels all saw `samples`, accumulated in binary32 as the kernel does."""
    s = q = F32(0)
    for x in samples:
        x = F32(x)
        s, q = F32(s + x), F32(q + F32(x * x))
    return len(samples), [s] * 3, [q] * 3


# ------------------------------------------------------------------ the resolve rule, restated
def resolve_rule(n, albedo, normal, depth, coverage, pixel=None):
    """rtmi_resolve_features in numpy, operation by operation as include/rtmi.h states it.  n, coverage (N,) uint32,
    albedo, normal (N, 3) float32, depth (N,) float32, pixel (N,) bool (False: padding).  Returns (albedo, normal,
    depth, alpha), all float32: everything 0 where n == 0 and for padding."""
    n, c = np.asarray(n, dtype=np.uint32), np.asarray(coverage, dtype=np.uint32)
    live = n > 0 if pixel is None else (n > 0) & np.asarray(pixel, dtype=bool)
    nf, cf = n.astype(F32), c.astype(F32)
    with np.errstate(all="ignore"):
        a = np.where(live[:, None], np.asarray(albedo, dtype=F32) / nf[:, None], F32(0))
        m = np.where(live[:, None], np.asarray(normal, dtype=F32) / nf[:, None], F32(0))
        d = np.where(live & (c > 0), np.asarray(depth, dtype=F32) / cf, F32(0))
        alpha = np.where(live, cf / nf, F32(0))
    for x in (a, m, d, alpha):
        assert x.dtype == F32
    return a, m, d, alpha

H, W = 20, 28  # ragged tiles: 3 x 4 tiles of 8 x 8 over 20 x 28 pixels


class Shards:
    """Every shard of one frame on the one GPU: a Renderer per rank, and row-major views of their tile-major buffers."""

    def __init__(self, name, depth, cap, world=1, h=H, w=W):
        self.name, self.h, self.w, self.world = name, h, w, world
        self.b = common.build_scene(rtmi.SceneBuilder(common.scene_seed(name)), name, w / h).commit()
        self.R = [rtmi.Renderer(self.b, h, w, cap, depth, post=False, rank=r, world_size=world).init_rng()
                  for r in range(world)]
        self.pm = [rtmi.pixel_map(R.frame) for R in self.R]
        for R in self.R:
            R._budget_buffers()

    def scatter(self, rowmajor, pad=0):
        """Row-major (H*W,) values -> one tile-major int32 CUDA tensor per rank (`pad` on padding items)."""
        out = []
        for pm in self.pm:
            t = np.full(pm.shape, pad, dtype=np.int64)
            t[pm >= 0] = np.asarray(rowmajor).reshape(-1)[pm[pm >= 0]]
            out.append(torch.from_numpy(t.astype(np.uint32).view(np.int32)).cuda())
        return out

    def raw(self, attr):
        """The tile-major buffers themselves, one numpy array per rank ((items, ..); states as (items, 6))."""
        torch.cuda.synchronize()
        out = []
        for R in self.R:
            a = getattr(R, attr).cpu().numpy()
            out.append(np.ascontiguousarray(a.T) if attr == "states" else a)
        return out

    def gather(self, attr):
        """Row-major (H*W, ..) array of a per-item buffer of all ranks."""
        parts = self.raw(attr)
        out = np.zeros((self.h * self.w,) + parts[0].shape[1:], dtype=parts[0].dtype)
        for pm, a in zip(self.pm, parts):
            out[pm[pm >= 0]] = a[pm >= 0]
        return out

    def render_budget(self, rowmajor, count_rays=True):
        for R, bt in zip(self.R, self.scatter(rowmajor)):
            R.render_budget(bt, count_rays=count_rays)
        for R in self.R:
            R.check()
            assert int(R.d_work[0].item()) == 0, "abandoned mesh searches"
        return self

    def render(self):
        for R in self.R:
            R.render()
            R.check()
        return self

    def results(self):
        return {k: self.gather(k) for k in ("sum", "sq", "samples", "budget_rays", "states")}


class OracleReplay:
    """The oracle driven a sample at a time: sums, squares, sample and ray counts per pixel in row-major order."""

    def __init__(self, name, depth, h=H, w=W):
        self.h, self.w, self.depth = h, w, depth
        seed = common.scene_seed(name)
        self.ob = common.build_scene(oraclelib.OracleBuilder(seed), name, w / h)
        n = h * w
        self.states = oraclelib.rng_init(seed, n)
        self.states[0] = self.ob.state0
        self.sum, self.sq = np.zeros((n, 3), F32), np.zeros((n, 3), F32)
        self.samples, self.rays = np.zeros(n, np.uint32), np.zeros(n, np.uint32)

    def add(self, budget):
        budget = np.asarray(budget).reshape(-1).astype(np.int64)
        for k in range(int(budget.max()) if budget.size else 0):
            ids = np.nonzero(budget > k)[0].astype(np.int32)
            rgb, rays, self.states, _ = self.ob.render(self.h, self.w, 1, self.depth, post=False, pixel_ids=ids,
                                                       states=self.states)
            x = rgb.reshape(-1, 3)[ids]
            self.sum[ids] = self.sum[ids] + x
            self.sq[ids] = self.sq[ids] + x * x
            self.samples[ids] += 1
            self.rays[ids] += rays.reshape(-1)[ids]
        assert self.sum.dtype == F32 and self.sq.dtype == F32
        return self

    def assert_equal(self, got, what=""):
        assert np.array_equal(got["samples"].view(np.uint32), self.samples), what + ": sample counts"
        assert np.array_equal(got["budget_rays"].view(np.uint32), self.rays), what + ": ray counts"
        assert same(got["sum"], self.sum), what + ": sums"
        assert same(got["sq"], self.sq), what + ": second moments"
        assert np.array_equal(got["states"].view(np.uint32), self.states), what + ": final RNG states"


def assert_same_results(a, b, what=""):
    for k in a:
        assert same(a[k], b[k]), "%s: %s differ" % (what, k)


def random_budget(seed, n=H * W, hi=9, zero_fraction=0.2):
    rng = np.random.default_rng(seed)
    b = rng.integers(1, hi + 1, n)
    b[rng.random(n) < zero_fraction] = 0
    return b


# ------------------------------------------------------------------ 10. the adaptive loop, end to end
ADAPTIVE = dict(min_spp=4, max_spp=64, step=4, tolerance=0.25, floor=0.01)
