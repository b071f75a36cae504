"""The slab table of the fast list kernels on the host side (scene_dev.h: PairSlab; scene.hip: pair_slab): every pair's
bounds once more as centre and half extent, with the fixed pad, the distance slack of an origin kOriginReach x list_mag
out and the slab test's own rounding folded into the half extent.  Containment is checked in binary64 against the
corners and against the PairBox records, with the constants of margins.h restated (tests/pair_slab_worlds.py); then the
code-object metadata of the three kernels that read the table, and the reach predicate.  No GPU involved."""
import re

import numpy as np
import pytest

import common
import rtmi
import pair_slab_worlds as psw
import tri_tasks_worlds as worlds
from abi_host import LIBS, _count, _waves

F32, F64 = np.float32, np.float64


def _builder(fill, seed, aspect=1.0):
    b = rtmi.SceneBuilder(seed)
    fill(b, aspect)
    return b


WORLDS = {"cornell_box": lambda: _builder(psw.cornell, 1024), "mixed_list": lambda: _builder(psw.mixed_list, 7),
          "long_list": lambda: _builder(lambda b, a: worlds.long_list(130)(b), 7), "thin_pair": lambda: _builder(psw.thin_pair, 7)}
UNBOUNDED = {"cornell_box": 0, "mixed_list": 0, "long_list": None, "thin_pair": 1}  # (None: whatever the random list holds)


def fixed_pad(diag, mag):
    """margins.h: fixed_pad, in binary32 as the library forms it."""
    return F32(F32(F32(psw.PAD_OF_EXTENT) * diag) + F32(F32(psw.PAD_OF_MAGNITUDE) * mag)) + F32(psw.PAD_FLOOR)


@pytest.mark.parametrize("name", sorted(WORLDS))
def test_slabs_contain_what_the_per_ray_slack_covered(name):
    b = WORLDS[name]()
    sl, bx, list_mag = b.pair_slabs()
    _, ht, co = b.list_records()
    n = len(co)
    assert n >= 5 and sl.shape == bx.shape == (n + 1, 8)
    # the padding record behind the last pair (the look-ahead of the scan's scalar loads reads it; nothing tests it)
    assert not sl[n].view(np.uint32).any() and not bx[n].view(np.uint32).any()
    assert not sl[:n, 6:].view(np.uint32).any()  # the two spare words
    c, h = sl[:n, :3].astype(F64), sl[:n, 3:6].astype(F64)
    mn, mx = bx[:n, :3].astype(F64), bx[:n, 3:6].astype(F64)
    unbounded = np.isinf(bx[:n, :6]).any(axis=1)
    assert UNBOUNDED[name] is None or unbounded.sum() == UNBOUNDED[name], unbounded.sum()
    # an unbounded pair: c = 0 and h = +inf on every axis -- the test's times are -inf / +inf while k is finite
    assert (sl[:n][unbounded, :3] == 0).all() and (sl[:n][unbounded, 3:6] == np.inf).all()
    assert np.isfinite(sl[:n][~unbounded, :6]).all()
    # list_mag: the largest |coordinate| of the list's corners
    assert list_mag == F32(np.abs(co).max())
    widen = psw.widening(list_mag)
    assert widen >= psw.DIST_SLACK * (psw.ORIGIN_REACH * list_mag + list_mag)  # the per-ray slack at the reach's edge
    k = ~unbounded
    # (1) against the PairBox, which holds the fixed pad: [c - h, c + h] contains it widened by delta_c + r_c
    # (2^-40 of the widening is left to the binary64 roundings of this comparison itself)
    lo, hi = mn[k] - widen, mx[k] + widen
    own = widen * 2.0 ** -40
    assert (c[k] - h[k] <= lo + own).all() and (c[k] + h[k] >= hi - own).all(), name
    # (2) h' is never below the exact value for the rounded centre, and never more than one binary32 step above it
    exact = np.maximum(hi - c[k], c[k] - lo)
    assert (h[k] >= exact).all(), name
    assert (sl[:n][k, 3:6] <= np.nextafter(exact.astype(F32), F32(np.inf))).all(), name
    # the centre is the middle of the bounds, rounded once
    assert np.array_equal(sl[:n][k, :3], ((lo + hi) / 2).astype(F32)), name
    # (3) against the corners themselves: the fixed pad of margins.h (2 % off for its binary32 roundings, as
    # Scene::check_margins allows) and the widening, from the corners alone
    lone = (ht[:, 1, 13] & 1) == 0  # TRI_SECOND
    pts = np.where(lone[:, None, None], co[:, [0, 1, 2, 2]], co)
    cmn, cmx = pts.min(axis=1), pts.max(axis=1)
    diag = (cmx - cmn).max(axis=1)
    mag = np.maximum(np.abs(cmn), np.abs(cmx)).max(axis=1)
    pad = np.array([0.98 * float(fixed_pad(d, m)) for d, m in zip(diag, mag)])[:, None]
    assert (c[k] - h[k] <= (cmn.astype(F64) - pad - widen)[k]).all(), name
    assert (c[k] + h[k] >= (cmx.astype(F64) + pad + widen)[k]).all(), name
    assert (mag <= list_mag).all()


def test_the_rounding_term_covers_the_slab_arithmetic():
    """margins.h's row: k = -o inv, tc = fma(c, inv, k) and near / far = fma(-+h, |inv|, tc) round once each, each by at
    most eps of (|o| + |c| + h) |inv|, and the hardware reciprocal's one ulp scales an axis' times by 2 eps: five eps of
    (kOriginReach + 2.01) mag in space (|c| <= mag, h <= 1.01 mag) against the kSlabRoundEps (kOriginReach + 1) carried."""
    assert psw.SLAB_ROUND_EPS * (psw.ORIGIN_REACH + 1) >= 5 * (psw.ORIGIN_REACH + 2.01)
    for name in sorted(WORLDS):
        sl, _, list_mag = WORLDS[name]().pair_slabs()
        fin = np.isfinite(sl[:-1, 3:6]).all(axis=1)
        assert (np.abs(sl[:-1][fin, :3]) <= list_mag).all() and (sl[:-1][fin, 3:6] <= 1.01 * list_mag).all(), name


def test_the_table_costs_the_long_list_nothing_it_did_not_have():
    """The table rides in the allocation of the PairBox records: a list's records stay 32 bytes per pair twice over."""
    sl, bx, _ = WORLDS["long_list"]().pair_slabs()
    assert len(sl) == len(bx) == 131


# (vgpr_count, vgpr_spill_count, sgpr_spill_count) of the three kernels that read the table, before it
PINNED_BEFORE = {"render_kernelILj2ELj255E": (80, 0, 5), "render_kernelILj2ELj383E": (80, 3, 13),
                 "probe_kernelILj2ELj383E": (80, 3, 13)}


def test_the_pinned_kernels_keep_their_registers():
    """80 VGPRs and six waves per SIMD, no more spilled VGPR dwords or SGPRs than the parent's build, no static LDS."""
    notes = common.kernel_notes(LIBS[0])
    for key, (vgprs, vspill, sspill) in PINNED_BEFORE.items():
        got = [blk for name, blk in notes.items() if key in name]
        assert len(got) == 1, key
        blk = got[0]
        assert _count(blk, "vgpr_count") <= vgprs and _waves(_count(blk, "vgpr_count")) == 6, key
        assert _count(blk, "vgpr_spill_count") <= vspill, key
        assert _count(blk, "sgpr_spill_count") <= sspill, key
        assert re.search(r"\.group_segment_fixed_size:\s+0\b", blk), key


# ------------------------------------------------------------------ the predicate
def _facts(**kw):
    f = dict(enabled=1, variant=2, n_mats=4, mats_in_lds=1, pairs_in_lds=1, unsigned_colours=1, det_safe=1, width=64, height=64,
             lane_stride=1, priorities=1, chains=0, resumed=0, tile_cost=0)
    f.update(kw)
    return (rtmi.C.c_int32 * rtmi.FAST_PATH_FACTS)(*f.values())


def test_the_reach_is_part_of_the_staging_fact_in_both_builds():
    """RTMI_FAST_PATH_FACTS stays 14: a camera beyond the reach clears `pairs_in_lds`, and without that fact no launch is
    a fast one.  Both builds of the library answer alike."""
    import ctypes as C
    assert rtmi.FAST_PATH_FACTS == 14
    for path in LIBS:
        L = C.CDLL(path)
        L.rtmi_fast_path_kernel.restype = C.c_int
        assert L.rtmi_fast_path_kernel(_facts()) == 1 and L.rtmi_fast_path_kernel(_facts(chains=1, resumed=1, tile_cost=1)) == 2, path
        assert L.rtmi_fast_path_kernel(_facts(pairs_in_lds=0)) == 0, path
        assert L.rtmi_fast_path_kernel(_facts(pairs_in_lds=0, chains=1, resumed=1, tile_cost=1)) == 0, path


def test_the_reach_follows_the_camera():
    """|position|inf <= kOriginReach x list_mag, asked of the scene's current camera: C2's and C4's camera sits at
    800 / 555 = 1.44 list_mag; a camera moved beyond the reach by camera_update is outside, and back inside when it
    returns."""
    b = WORLDS["cornell_box"]()
    _, _, mag = b.pair_slabs()
    assert mag == 555.0 and b.slab_reach()
    cam = b.camera_get().copy()
    assert np.abs(cam[0]).max() == 800.0
    for axis in range(3):
        for sign in (-1.0, 1.0):
            for factor, inside in ((0.99, True), (1.0, True), (1.01, False)):
                moved = cam.copy()
                moved[0, axis] = F32(sign * factor * psw.ORIGIN_REACH * mag)
                b.camera_update(moved)
                assert b.slab_reach() == inside, (axis, sign, factor)
    b.camera_update(cam)
    assert b.slab_reach()
    for name in ("inside_reach", "beyond_reach", "axis_aligned", "thin_pair"):
        fill, seed, _ = psw.WORLDS[name]
        assert _builder(fill, seed).slab_reach() == (name != "beyond_reach"), name


def test_a_list_too_large_for_a_finite_k_is_outside():
    """(kOriginReach + 1) x list_mag x 1e30 must stay below FLT_MAX: with the reciprocals clamped to 1e30, k = -o / d and
    tc stay finite, and an unbounded record's products stay -inf / +inf."""
    def fill(scale):
        def f(b, aspect):
            b.camera_pinhole(worlds.v3(0, 0, 4 * scale), worlds.v3(0, 0, 0), worlds.v3(0, 1, 0), worlds.PI_D / 4, 1.0)
            m = b.lambertian(worlds.v3(0.5, 0.5, 0.5))
            for i in range(5):
                z = F32(-0.25 * i * scale)
                b.parallelogram([worlds.v3(-3 * scale, -3 * scale, z), worlds.v3(3 * scale, -3 * scale, z), worlds.v3(-3 * scale, 3 * scale, z)], m)
        return f
    flt_max = float(np.finfo(F32).max)
    for scale, inside in ((1.0, True), (1e7, True), (2e7, False)):  # list_mag = 3 scale: 9 x 3e7 x 1e30 < 3.4e38 < 9 x 6e7 x 1e30
        b = _builder(fill(F32(scale)), 7)
        mag = b.pair_slabs()[2]
        assert ((psw.ORIGIN_REACH + 1) * mag * 1e30 < flt_max) == inside
        assert b.slab_reach() == inside, scale
