"""The contract of the scheduler's plan kernels (csrc/sched.hip: tile_cost, tile_order, head_scan / count / plan /
scatter, expand_order, quarter_cost / sort, snake_map, chain_link), restated in numpy with no GPU.

Every integer quantity is computed in int64 (the kernels: uint32 with 64-bit products); `chain_fut` alone is binary32,
operation by operation in the kernel's own order (the library is built -ffp-contract=off, so it is compared for equality).

Where the device's result depends on the order of its atomics -- tiles within one cost bucket, quarters within one,
pixels within one head class -- `check_plan` compares what is determined (permutation, bucket sequence, the multiset per
bucket or class) and derives everything downstream (qmap, the chains) from the DEVICE's own order / qsorted.  Everything
else is compared for equality.
"""
import numpy as np

HEAD_CAP = 16384       # kernels.h: kHeadCap
CHAIN_CAP = 1 << 15    # capi.hip: kMaxChains
MARK = 0x80000000      # bit 31 of a ray count: the pixel is in the head list
NONE = 0xffffffff      # a head threshold no count reaches: class dropped
FUT_MAX = np.float32(4.0e9)
# the scheduler's regions of the scratch (rtmi_debug_scratch_regions): 32-bit words as a function of the tiles
REGION_WORDS = dict(cost=lambda nt: nt, order=lambda nt: nt, meta=lambda nt: 32, head=lambda nt: HEAD_CAP,
                    work=lambda nt: 64 * nt, qcost=lambda nt: 4 * nt, qsorted=lambda nt: 4 * nt, qmap=lambda nt: 4 * nt,
                    qmax=lambda nt: 4, fut=lambda nt: nt, next=lambda nt: nt, claims=lambda nt: nt, first=lambda nt: CHAIN_CAP)


def _i64(a):
    return np.asarray(a).astype(np.int64)


def plan_arrays(raw, regions, nt):
    """The scheduler's regions of a render scratch as arrays: `raw` the scratch's bytes (np.uint8), `regions` the byte
    offsets rtmi_debug_scratch_regions reports.  next and first are int32, everything else uint32."""
    raw = np.asarray(raw).view(np.uint8).reshape(-1)
    assert raw.size >= regions["total"]
    out = {}
    for name, words in REGION_WORDS.items():
        at, n = regions[name], words(nt)
        out[name] = raw[at:at + 4 * n].view(np.int32 if name in ("next", "first") else np.uint32).copy()
    return out


# ------------------------------------------------------------------ tiles
def tile_costs(counts):
    """Per tile the sum of its 64 counts (tile_cost_kernel), and the largest."""
    c = _i64(counts)
    assert c.size % 64 == 0 and c.size > 0 and (c >= 0).all() and (c < MARK).all(), "unmarked counts of whole tiles"
    cost = c.reshape(-1, 64).sum(axis=1)
    assert cost.max() < 1 << 32
    return cost, int(cost.max())


def buckets(cost, mx):
    """Bucket 0 holds the dearest: 255 - floor(cost * 255 / max(mx, 1)) (tile_order_kernel, quarter_sort_kernel)."""
    return 255 - (_i64(cost) * 255) // max(int(mx), 1)


def sparse_items(cost, sparse_cap, outlier_x10):
    """Outlier-tile mode: work items of the queue's sparse head.  An outlier costs at least outlier_x10 / 10 times the
    mean (cost * n * 10 >= outlier_x10 * total); they count only in a frame whose dearest tile costs at least three times
    the mean (max(mx, 1) * n >= 3 * total); 64 items each, clamped to sparse_cap.  Both comparisons are between products
    and not strict, so a frame without any cost is 'skewed' and all of its tiles are outliers: min(64 n, sparse_cap)."""
    cost = _i64(cost)
    n, total = int(cost.size), int(cost.sum())
    mx = max(int(cost.max()), 1)
    outliers = int((cost * n * 10 >= int(outlier_x10) * total).sum())
    skewed = mx * n >= 3 * total
    return min(outliers * 64, int(sparse_cap)) if skewed else 0


# ------------------------------------------------------------------ head
def head_plan(counts, grid_waves, head_pct):
    """The pixel head from unmarked counts.  Returns a dict: cmax, total, skewed, classes (sizes before the limits),
    fallbacks (how many of over()'s three fired), thresholds (t64, t32, t16 as used; NONE: dropped), ends (a, a + b,
    a + b + c: the ends of the three segments of the head list), members (three sorted arrays of work items)."""
    c = _i64(counts)
    n, cmax, total = int(c.size), int(c.max()), int(c.sum())
    skewed = cmax * n >= 3 * total and cmax >= 4
    p64, p32, p16 = (int(p) for p in head_pct)
    if skewed:
        t64, t32, t16 = (cmax * p64 + 99) // 100, (cmax * p32 + 99) // 100, (cmax * p16 + 99) // 100
        a = int(((c >= t16) & (c >= t64)).sum())
        b = int(((c >= t16) & (c < t64) & (c >= t32)).sum())
        c3 = int(((c >= t16) & (c < t64) & (c < t32)).sum())
    else:
        t64 = t32 = t16 = NONE
        a = b = c3 = 0
    classes = (a, b, c3)

    def over():
        return a + (b + 1) // 2 + (c3 + 3) // 4 > int(grid_waves) // 4 or a + b + c3 > HEAD_CAP
    fallbacks = 0
    if over():  # the lightest class goes
        c3, t16, fallbacks = 0, t32, 1
        if over():  # the heaviest pixels share waves two by two
            b, a, t64, fallbacks = b + a, 0, NONE, 2
            if over():  # no head
                b, t32, t16, fallbacks = 0, NONE, NONE, 3
    # the scatter, by the thresholds as used (head_scatter_kernel)
    if t16 == NONE:
        members = [np.zeros(0, np.int64)] * 3
    else:
        inh = c >= t16
        k0 = inh & (c >= t64)
        k1 = inh & ~k0 & (c >= t32)
        k2 = inh & ~k0 & ~k1
        members = [np.flatnonzero(k) for k in (k0, k1, k2)]
    return dict(cmax=cmax, total=total, skewed=skewed, classes=classes, fallbacks=fallbacks, thresholds=(t64, t32, t16),
                ends=(a, a + b, a + b + c3), members=members)


# ------------------------------------------------------------------ quarter tiles
def quarter_costs(work, marked_counts):
    """Per quarter tile (16 work items): the sum of work + (count without its mark) (quarter_cost_kernel)."""
    s = _i64(work) + (_i64(marked_counts) & (MARK - 1))
    q = s.reshape(-1, 16).sum(axis=1)
    assert q.max() < 1 << 32
    return q, int(q.max())


def expand_order(order):
    """Without work counts: the tiles in their order, each tile's four quarters one after the other (expand_order_kernel)."""
    return (_i64(order)[:, None] * 4 + np.arange(4)[None, :]).reshape(-1)


def snake(qsorted):
    """Wave b's 64 items are quarters b, 2n - 1 - b, 2n + b, 4n - 1 - b of the sorted list (snake_map_kernel)."""
    s = _i64(qsorted)
    n = s.size // 4
    b = np.arange(n)
    return np.stack([s[b], s[2 * n - 1 - b], s[2 * n + b], s[4 * n - 1 - b]], axis=1).reshape(-1)


# ------------------------------------------------------------------ chains
def chain_rank(j, s, r, S, R):
    """Position in the tile order of the j-th tile of chain (SIMD s, wave r): the SIMD's k-th tile is rank
    k S + (k odd ? S - 1 - s : s), the wave's j-th is the SIMD's k = j R + (j odd ? R - 1 - r : r)."""
    k = j * R + (R - 1 - r if j & 1 else r)
    return k * S + (S - 1 - s if k & 1 else s)


def fut_scale(spp, probe_spp):
    return np.float32(spp) / (np.float32(64.0) * np.float32(probe_spp))


def chain_plan(order, cost, S, R, spp, probe_spp):
    """first[S R], next[n], fut[n] (chain_link_kernel): every chain walked backwards; fut in binary32 -- multiply, add,
    min(., 4.0e9), truncate -- of what follows a tile in its chain."""
    order, cost = _i64(order), _i64(cost)
    n = order.size
    scale = fut_scale(spp, probe_spp)
    first = np.full(S * R, -1, np.int64)
    nxt = np.full(n, -2, np.int64)  # (-2: in no chain; never left behind when the order is a permutation)
    fut = np.zeros(n, np.int64)
    for c in range(S * R):
        s, r = c % S, c // S
        steps = 0
        while chain_rank(steps, s, r, S, R) < n:
            steps += 1
        acc, after = np.float32(0.0), -1
        for j in range(steps - 1, -1, -1):
            t = int(order[chain_rank(j, s, r, S, R)])
            nxt[t] = after
            fut[t] = int(min(acc, FUT_MAX))
            acc = np.float32(acc + np.float32(np.float32(cost[t]) * scale))
            after = t
        first[c] = after
    return first, nxt, fut


def walk_chains(first, nxt, n):
    """Visits per tile when every chain is walked from `first` via `next` (every index checked before it is used)."""
    first, nxt = _i64(first), _i64(nxt)
    assert ((first >= -1) & (first < n)).all(), "chain_first out of range"
    assert ((nxt >= -1) & (nxt < n)).all(), "chain_next out of range"
    seen = np.zeros(n, np.int64)
    for t in first:
        steps = 0
        while t >= 0:
            seen[t] += 1
            t = nxt[t]
            steps += 1
            assert steps <= n, "a chain loops"
    return seen


# ------------------------------------------------------------------ checker
def _check_sorted(what, got, cost, mx, n):
    got = _i64(got)
    assert got.size == n and np.array_equal(np.sort(got), np.arange(n)), what + " is not a permutation"
    bk = buckets(cost, mx)
    seq = bk[got]
    assert (np.diff(seq) >= 0).all(), what + ": buckets out of order (dearest first)"
    # same multiset per bucket: sorting by (bucket, index) must give the restatement's stable order
    want = np.lexsort((np.arange(n), bk))
    assert np.array_equal(got[np.lexsort((got, seq))], want), what + ": a bucket holds the wrong members"


def check_plan(counts, work, got, *, pixel_head, sparse_cap, grid_waves, outlier_x10, head_pct, simds=0, rounds=0, spp=1,
               probe_spp=1, claims_zero=True):
    """`counts`: the unmarked input counts; `work`: the work counts or None; `got`: what the device left -- cost, order,
    meta, head, qcost, qsorted, qmap, qmax, fut, next, claims, first (arrays of the scratch's regions) and `marked` (the
    counts after the step).  Asserts the whole contract; returns the head plan (or None) for the caller to look at."""
    counts = _i64(counts)
    nt = counts.size // 64
    meta = _i64(got["meta"])
    marked = _i64(got["marked"])
    # tiles
    cost, mx = tile_costs(counts)
    assert np.array_equal(_i64(got["cost"]), cost), "tile costs"
    assert meta[0] == mx, ("largest tile cost", meta[0], mx)
    _check_sorted("order", got["order"], cost, mx, nt)
    order = _i64(got["order"])
    # head / outlier tiles
    assert np.array_equal(marked & (MARK - 1), counts), "the low 31 bits of a count changed"
    hp = None
    if pixel_head:
        hp = head_plan(counts, grid_waves, head_pct)
        ends = hp["ends"]
        assert tuple(meta[1:4]) == (ends[2], ends[0], ends[1]), ("head entries and class ends", meta[1:4], ends)
        assert meta[16] == hp["cmax"] and meta[18] + (meta[19] << 32) == hp["total"], "largest count / sum of counts"
        assert tuple(meta[20:23]) == hp["classes"], ("class sizes", meta[20:23], hp["classes"])
        assert tuple(meta[24:27]) == hp["thresholds"], ("thresholds as used", meta[24:27], hp["thresholds"])
        assert tuple(meta[28:31]) == ends, ("scatter cursors", meta[28:31], ends)
        assert ends[2] <= HEAD_CAP
        head = _i64(got["head"])[:ends[2]]
        assert ((head >= 0) & (head < counts.size)).all(), "head entry out of range"
        assert np.unique(head).size == head.size, "a pixel is listed twice"
        lo = 0
        for k, hi in enumerate(ends):
            assert np.array_equal(np.sort(head[lo:hi]), hp["members"][k]), "head class %d holds the wrong pixels" % k
            lo = hi
        listed = np.zeros(counts.size, bool)
        listed[head] = True
        assert np.array_equal((marked & MARK) != 0, listed), "bit 31 if and only if listed"
    else:
        assert np.array_equal(marked, counts), "counts changed without a head"
        assert meta[1] == sparse_items(cost, sparse_cap, outlier_x10), ("sparse items", meta[1])
        assert (meta[2:4] == 0).all() and (meta[16:32] == 0).all(), "head words written without a head"
    # quarter tiles
    qmap = _i64(got["qmap"])
    if work is not None:
        qc, qmx = quarter_costs(work, marked)
        assert np.array_equal(_i64(got["qcost"]), qc), "quarter costs"
        assert _i64(got["qmax"])[0] == qmx, "largest quarter cost"
        _check_sorted("qsorted", got["qsorted"], qc, qmx, 4 * nt)
        assert np.array_equal(qmap, snake(got["qsorted"])), "the snake of the device's own qsorted"
    else:
        assert np.array_equal(qmap, expand_order(order)), "qmap is not the tile order, quarter by quarter"
    assert np.array_equal(np.sort(qmap), np.arange(4 * nt)), "qmap is not a permutation of the quarters"
    # chains
    if simds * rounds > 0:
        assert simds * rounds <= CHAIN_CAP
        first, nxt, fut = chain_plan(order, cost, simds, rounds, spp, probe_spp)
        g_first = _i64(got["first"])[:simds * rounds]
        assert np.array_equal(g_first, first), "chain_first"
        assert np.array_equal(_i64(got["next"]), nxt), "chain_next"
        assert np.array_equal(_i64(got["fut"]), fut), "chain_fut"
        assert (walk_chains(g_first, got["next"], nt) == 1).all(), "the chains do not visit every tile exactly once"
        # a chain is empty exactly when the rank of its first tile is past the last tile
        rank0 = np.array([chain_rank(0, c % simds, c // simds, simds, rounds) for c in range(simds * rounds)])
        assert np.array_equal(g_first == -1, rank0 >= nt), "empty chains are -1, and only they"
        if claims_zero:
            assert (_i64(got["claims"]) == 0).all(), "claims are zeroed with the plan"
    return hp
