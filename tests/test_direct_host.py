"""Next-event estimation on the host side: the four new exports of both builds and their declarations, the argument checks
that come before any HIP call, the binding's defaults, the new kernels' metadata, and the numpy restatements of the light
table, the step and the fold (tests/directlib.py) held to hand-worked cases.  No GPU involved."""
import ctypes as C
import math
import os
import re
import subprocess

import numpy as np
import pytest

import bouncelib
import common
import directlib as dl
import rtmi
from abi_host import DUMMY, LIBS, OK, ROOT, _count, _refused
from querylib import Recorder, v3

NEW = ("rtmi_scene_light_count", "rtmi_scene_lights", "rtmi_direct_sample", "rtmi_path_fold_direct")
f32 = np.float32
A, B = DUMMY, C.c_void_p(32)


# ------------------------------------------------------------------ the symbols
def test_entries_are_exported_by_both_builds_declared_and_bound():
    L = rtmi.lib()
    assert L.rtmi_version() == 3  # additive: no version change
    names = {s[0]: s for s in rtmi.SYMBOLS}
    header = open(os.path.join(ROOT, "include", "rtmi.h")).read()
    for lib in LIBS:
        syms = subprocess.run(["nm", "-D", "--defined-only", lib], stdout=subprocess.PIPE, text=True, check=True).stdout
        for name in NEW:
            assert re.search(r"\bT %s$" % name, syms, re.M), (lib, name)
    for name in NEW:
        assert name in names and re.search(r"\b%s\(" % name, header), name
    # the stated signatures: 21 arguments of the step, 10 of the fold
    assert len(names["rtmi_direct_sample"][2]) == 21 and names["rtmi_direct_sample"][2][5] is C.c_uint32
    assert len(names["rtmi_path_fold_direct"][2]) == 10
    assert names["rtmi_scene_light_count"][1] is C.c_int64
    assert rtmi.LIGHT_DTYPE.itemsize == 88  # rtmi_light: 18 floats and 4 ints


C_PROG = r'''
#include <stdio.h>
#include <string.h>
#include "rtmi.h"
typedef int64_t (*count_fn)(const rtmi_scene *);
typedef int (*lights_fn)(const rtmi_scene *, rtmi_light *, int64_t);
typedef int (*step_fn)(const rtmi_scene *, int64_t, const uint32_t *, int64_t, const uint32_t *, uint32_t, int, const float *,
                       const float *, const rtmi_hit *, const uint32_t *, float *, const float *, void *, uint32_t *, float *,
                       float *, float *, float *, unsigned long long *, void *);
typedef int (*fold_fn)(int64_t, int, const float *, const uint32_t *, const float *, const float *, const float *,
                       const uint8_t *, float *, void *);
int main(void) {
  count_fn count = &rtmi_scene_light_count;
  lights_fn lights = &rtmi_scene_lights;
  step_fn step = &rtmi_direct_sample;
  fold_fn fold = &rtmi_path_fold_direct;
  rtmi_light l;
  rtmi_scene *s = rtmi_scene_create();
  if (sizeof(rtmi_light) != 88) return 1;
  if (count(s) != RTMI_ERR_INVALID || !strstr(rtmi_last_error(), "committed")) return 2;
  if (lights(s, &l, 1) != RTMI_ERR_INVALID || !strstr(rtmi_last_error(), "committed")) return 3;
  if (step(NULL, 0, NULL, 0, NULL, 0, 1, NULL, NULL, NULL, NULL, NULL, NULL, NULL, NULL, NULL, NULL, NULL, NULL, NULL, NULL) !=
      RTMI_ERR_INVALID) return 4;
  if (fold(1, 0, NULL, NULL, NULL, NULL, NULL, NULL, NULL, NULL) != RTMI_ERR_INVALID || !strstr(rtmi_last_error(), "layers")) return 5;
  if (fold(0, 1, NULL, NULL, NULL, NULL, NULL, NULL, NULL, NULL) != RTMI_OK) return 6;
  rtmi_scene_destroy(s);
  printf("direct abi ok\n");
  return 0;
}
'''


def test_entries_link_from_c99(tmp_path):
    lib_dir = os.path.dirname(rtmi.LIB_PATH)
    src = tmp_path / "direct.c"
    src.write_text(C_PROG)
    exe = tmp_path / "direct"
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-pedantic", "-I", os.path.join(ROOT, "include"), str(src),
                    "-L", lib_dir, "-lrtmi", "-Wl,-rpath," + lib_dir, "-Wl,-rpath,/opt/rocm/lib", "-o", str(exe)], check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, (r.returncode, r.stdout, r.stderr)
    assert "direct abi ok" in r.stdout


# ------------------------------------------------------------------ refusals before any HIP call
ARRAYS = ("o", "d", "hits", "steps", "em", "at", "ls", "flags", "so", "sd", "st", "direct")


def _step(s, n, n_list, lst=None, cnt=None, step=0, sample=1, counts=None, **kw):
    a = {k: kw.get(k, DUMMY) for k in ARRAYS}
    return rtmi.lib().rtmi_direct_sample(s, n, lst, n_list, cnt, step, sample, a["o"], a["d"], a["hits"], a["steps"], a["em"],
                                         a["at"], a["ls"], a["flags"], a["so"], a["sd"], a["st"], a["direct"], counts, None)


def test_direct_sample_argument_checks_before_any_hip_call():
    assert _refused(_step(None, 1, 1), b"null scene")
    b = rtmi.SceneBuilder(1)
    assert _refused(_step(b.h, -1, 0), b"negative")
    assert _refused(_step(b.h, 1 << 31, 1, lst=B), b"2^31")
    assert _refused(_step(b.h, 4, -1), b"negative")
    assert _refused(_step(b.h, 4, 1 << 31, lst=B), b"2^31")
    assert _refused(_step(b.h, 4, 5), b"n_list")  # a null list is the identity
    assert _refused(_step(b.h, 4, 4, step=rtmi.MAX_DEPTH), b"step")
    assert _refused(_step(b.h, 4, 4, step=0xffffffff), b"step")
    for k in ARRAYS:
        assert _refused(_step(b.h, 4, 4, **{k: None}), b"null"), k
    assert _refused(_step(b.h, 4, 4), b"committed")  # every array given, the counters optional: the scene is what is wrong
    assert _refused(_step(b.h, 4, 9, lst=B, cnt=A, step=rtmi.MAX_DEPTH - 1, sample=0), b"committed")
    assert _refused(_step(b.h, 0, 0, **{k: None for k in ARRAYS}), b"committed")  # nothing to do is no excuse
    assert _refused(rtmi.lib().rtmi_scene_light_count(None), b"null scene")
    assert _refused(rtmi.lib().rtmi_scene_light_count(b.h), b"committed")
    assert _refused(rtmi.lib().rtmi_scene_lights(None, A, 1), b"null scene")
    assert _refused(rtmi.lib().rtmi_scene_lights(b.h, A, 1), b"committed")


def _fold(n, layers, **kw):
    names = ("dirs", "steps", "em", "at", "direct", "occ", "out")
    a = {k: kw.get(k, DUMMY) for k in names}
    return rtmi.lib().rtmi_path_fold_direct(n, layers, a["dirs"], a["steps"], a["em"], a["at"], a["direct"], a["occ"], a["out"], None)


def test_path_fold_direct_argument_checks_before_any_hip_call():
    assert _refused(_fold(-1, 1), b"negative")
    assert _refused(_fold(1 << 31, 1), b"2^31")
    assert _refused(_fold(4, 0), b"layers")
    assert _refused(_fold(4, rtmi.MAX_DEPTH + 1), b"layers")
    for k in ("dirs", "steps", "em", "at", "direct", "occ", "out"):
        assert _refused(_fold(4, 2, **{k: None}), b"null"), k
    assert _fold(0, 1, dirs=None, steps=None, em=None, at=None, direct=None, occ=None, out=None) == OK


def test_binding_keeps_its_defaults():
    import inspect
    assert rtmi.Steps._fields[:8] == ("rgb", "steps", "alive", "origins", "directions", "emitted", "attenuation", "works")
    assert rtmi.Steps._fields[8:] == ("direct", "occluded", "flags")
    s = rtmi.Steps(*range(8))
    assert (s.direct, s.occluded, s.flags) == (None, None, None)
    p = inspect.signature(rtmi.SceneBuilder.trace_steps).parameters
    assert list(p)[:8] == ["self", "origins", "directions", "states", "max_depth", "each", "hits", "compact"]
    assert (p["each"].default, p["hits"].default, p["compact"].default) == (None, None, False)
    assert (p["direct"].default, p["light_states"].default) == (False, None)
    r = inspect.signature(rtmi.Renderer.render_rays).parameters
    assert r["direct"].default is False and r["each"].default is None and r["count_rays"].default is True
    torch = pytest.importorskip("torch")
    b = rtmi.SceneBuilder(1)
    o = torch.zeros((4, 3), dtype=torch.float32)
    st = torch.zeros((6, 4), dtype=torch.int32)
    with pytest.raises(rtmi.RtmiError, match="light_states"):
        b.trace_steps(o, o.clone(), st, 4, direct=True)
    with pytest.raises(rtmi.RtmiError):
        rtmi.path_fold_direct(o, None, None, None, None, None)  # CPU tensors: there is no CPU path
    with pytest.raises(rtmi.RtmiError):
        b.direct_sample(0, None, st, None)


def test_new_kernels_spill_nothing():
    """direct_sample_kernel: the 4 KiB cdf staging is its only LDS, no scratch, no spill, at least four waves per SIMD;
    path_fold_direct_kernel: no LDS, no scratch.  Both builds carry both."""
    for lib in LIBS:
        objects = common.code_object_notes(lib)
        notes = common.kernel_notes(lib)
        # no kernel name occurs in two code objects (a template kernel instantiated in two units would)
        assert len(objects) > 1 and sum(len(o) for o in objects) == len(notes), lib
        ds = [b for n, b in notes.items() if "direct_sample_kernel" in n]
        fd = [b for n, b in notes.items() if "path_fold_direct_kernel" in n]
        assert len(ds) == 1 and len(fd) == 1, lib
        assert _count(ds[0], "group_segment_fixed_size") == 4096
        assert _count(fd[0], "group_segment_fixed_size") == 0
        for blk in (ds[0], fd[0]):
            assert _count(blk, "vgpr_spill_count") == 0 and _count(blk, "sgpr_spill_count") == 0
            assert _count(blk, "private_segment_fixed_size") == 0
            assert _count(blk, "vgpr_count") <= 128


# ------------------------------------------------------------------ the generator
def test_draws_are_the_library_s_generator():
    L = rtmi.lib()
    st = np.zeros((5, 6), np.uint32)
    for i in range(5):
        L.rtmi_rng_host_state(C.c_uint64(99), C.c_uint64(7 + i), st[i].ctypes.data_as(C.POINTER(C.c_uint32)))
    ref = st.copy()
    got = [dl.draw01(st, np.array([0, 2, 4])) for _ in range(4)]
    for i in (0, 2, 4):
        p = ref[i].ctypes.data_as(C.POINTER(C.c_uint32))
        want = [L.rtmi_rng_host_random_float(C.c_float(0), C.c_float(1), p) for _ in range(4)]
        assert [float(g[[0, 2, 4].index(i)]) for g in got] == want
    assert np.array_equal(st, ref)  # rows 1 and 3 untouched, the others advanced by exactly four
    # the ends of the range: x = 0 gives 2^-33, x = 2^32 - 1 rounds to 1.0
    s = np.zeros((1, 6), np.uint32)
    s[0, 0] = (0 - 362437) & 0xffffffff  # v = 0 stays 0, d + 362437 = 0: x = 0
    assert dl.draw01(s, np.array([0]))[0] == f32(2.0 ** -33)
    s[0] = 0
    s[0, 0] = (0xffffffff - 362437) & 0xffffffff
    assert dl.draw01(s, np.array([0]))[0] == f32(1.0)


# ------------------------------------------------------------------ the table, by hand
def _host_scene(name):
    rec = Recorder(rtmi.SceneBuilder(common.scene_seed(name)))
    common.build_scene(rec, name, 1.0)
    return rec


def test_cornell_table_by_hand():
    t = dl.table_of(_host_scene("cornell_box"))
    assert len(t) == 1
    l = t[0]
    assert l["entry"] == 3 and l["element"] == 0 and l["kind"] == 0 and l["material"] == 3
    assert l["p0"].tolist() == [213, 554, 332] and l["e1"].tolist() == [0, 0, -105] and l["e2"].tolist() == [130, 0, 0]
    assert l["n"].tolist() == [0, -1, 0] or l["n"].tolist() == [0, 1, 0]
    assert l["emission"].tolist() == [1, 1, 1]
    assert l["area"] == f32(13650) and l["cdf"] == f32(1) and l["scale"] == f32(13650 / math.pi)


def test_furnace_table_by_hand():
    t = dl.table_of(_host_scene("furnace"))
    assert len(t) == 6
    assert t["entry"].tolist() == [1] * 6 and t["element"].tolist() == list(range(6)) and t["kind"].tolist() == [0] * 6
    assert (t["area"] == f32(400)).all() and t["cdf"][5] == f32(1)
    assert t["cdf"].tolist() == [f32(k / 6) for k in range(1, 6)] + [1.0]
    assert (t["scale"] == f32(2400 / math.pi)).all()  # area over the selection probability 1/6 and pi


def test_only_world_list_constant_lights_with_an_area_are_table_lights():
    rec = Recorder(rtmi.SceneBuilder(3))
    dl.odd_lights_world(rec)
    t = dl.table_of(rec)
    assert len(t) == 1
    l = t[0]
    assert l["kind"] == 1 and l["entry"] == 6 and l["element"] == 0  # sphere, mesh, 3 surfaces, nested sphere, the light
    assert l["area"] == f32(1.0)  # half of |(1, 0, 0) x (0, 0, 2)|
    assert l["emission"].tolist() == [2, 0, -4]
    assert l["cdf"] == f32(1) and l["scale"] == f32(1.0 / math.pi)


def _two_lights():
    """A unit-square parallelogram light at y = 1 (emission 1, 1, 1) and a triangle light of area 2 at y = 1 beside it
    (emission 0.5, 0.5, 0.5): weights 3 and 3, cdf 0.5, 1."""
    hot = np.zeros((2, 16), np.uint32)
    g = hot[:, :12].view(f32)
    g[0] = [0, 1, 0, 1, 0, 0, 0, 0, 1, 0, -1, 0]
    g[1] = [4, 1, 0, 2, 0, 0, 0, 0, 2, 0, -1, 0]
    hot[0, 12], hot[1, 12] = 1, 2
    mats = [(dl.LAMBERTIAN, f32([0.5, 0.5, 0.5])), (dl.LIGHT, f32([1, 1, 1])), (dl.LIGHT, f32([0.5, 0.5, 0.5]))]
    pairs = [(0, rtmi.RTMI_HIT_PARALLELOGRAM, 0), (1, rtmi.RTMI_HIT_TRIANGLE, 0)]
    return dl.light_table(hot, pairs, mats), np.array([0, 3, 3])


def _state_with_x(x, r, n=1):
    """One path at the floor point x, normal up, Lambertian, just scattered by step 0, whose light state's next three x
    words are chosen so that the draws are r."""
    H = np.zeros((n, 12), np.int32)
    H[:, 3:6] = f32([0, 1, 0]).view(np.int32)
    H[:, 6], H[:, 7] = 0, rtmi.RTMI_HIT_PARALLELOGRAM
    ps = dl.PathState(np.tile(f32(x), (n, 1)), np.tile(f32([0, 1, 0]), (n, 1)), H, np.ones(n), np.zeros((n, 3)),
                      np.full((n, 3), 0.5), np.zeros((n, 6)))
    return ps


class FixedDraws:
    """Replaces directlib.draw01 by a list of given values (the step's arithmetic by hand, not the generator's)."""

    def __init__(self, monkeypatch, values):
        self.values = list(values)
        monkeypatch.setattr(dl, "draw01", lambda st, idx: np.full(len(idx), f32(self.values.pop(0)), f32))


def test_step_by_hand(monkeypatch):
    tab, kinds = _two_lights()
    assert tab["cdf"].tolist() == [0.5, 1.0] and tab["area"].tolist() == [1.0, 2.0]
    assert tab["scale"].tolist() == [f32(2 / math.pi), f32(4 / math.pi)]
    # the square light straight above: q = (0.5, 1, 0.5) from x = (0.5, 0, 0.5): w = (0, 1, 0), d2 = 1, cs = cl = 1
    FixedDraws(monkeypatch, [0.25, 0.5, 0.5])
    ps = dl.step(tab, kinds, _state_with_x([0.5, 0, 0.5], None), 0, True)
    assert ps.SO[0].tolist() == [0.5, 0, 0.5] and ps.SD[0].tolist() == [0, 1, 0] and ps.ST[0] == f32(0.999)
    assert ps.DR[0].tolist() == [f32(f32(0.5) * f32(2 / math.pi))] * 3
    assert ps.flags[0] == 1 and ps.counts.tolist() == [4, 5]
    # r0 == cdf[0] still selects light 0 (the smallest j with r0 <= cdf[j]); r0 == 1.0 selects the last light
    FixedDraws(monkeypatch, [0.5, 0.5, 0.5])
    assert dl.step(tab, kinds, _state_with_x([0.5, 0, 0.5], None), 0, True).SD[0].tolist() == [0, 1, 0]
    # ... whose draws r1 + r2 > 1 are flipped: (0.75, 0.75) -> (0.25, 0.25): q = (4.5, 1, 0.5)
    FixedDraws(monkeypatch, [1.0, 0.75, 0.75])
    ps = dl.step(tab, kinds, _state_with_x([4.5, 0, 0.5], None), 0, True)
    assert ps.SD[0].tolist() == [0, 1, 0] and ps.DR[0].tolist() == [f32(f32(0.25) * f32(4 / math.pi))] * 3
    # r1 + r2 == 1 exactly is not flipped, and a parallelogram never is
    FixedDraws(monkeypatch, [1.0, 0.25, 0.75])
    assert dl.step(tab, kinds, _state_with_x([4.5, 0, 1.5], None), 0, True).SD[0].tolist() == [0, 1, 0]
    FixedDraws(monkeypatch, [0.25, 0.75, 0.75])
    assert dl.step(tab, kinds, _state_with_x([0.75, 0, 0.75], None), 0, True).SD[0].tolist() == [0, 1, 0]


def _invalid(ps):
    return (ps.SD[0] == 0).all() and not np.signbit(ps.SD[0]).any() and (ps.DR[0] == 0).all() and not np.signbit(ps.DR[0]).any() \
        and ps.ST[0] == 0 and ps.flags[0] == 1 and int(ps.counts[0]) == 4


def test_invalid_samples_by_hand(monkeypatch):
    tab, kinds = _two_lights()
    # cs <= 0: the light is below the surface's horizon (x above it, normal up)
    FixedDraws(monkeypatch, [0.25, 0.5, 0.5])
    s = _state_with_x([0.5, 2, 0.5], None)
    so = s.SO.copy()
    ps = dl.step(tab, kinds, s, 0, True)
    assert _invalid(ps) and np.array_equal(ps.SO, so)  # the shadow origin is written with a valid sample only
    # cs == 0 and cl == 0: x in the light's plane
    FixedDraws(monkeypatch, [0.25, 0.5, 0.5])
    assert _invalid(dl.step(tab, kinds, _state_with_x([3, 1, 0.5], None), 0, True))
    # cl == 0 alone: the surface's normal leans towards the light, which is seen edge-on
    FixedDraws(monkeypatch, [0.25, 0.5, 0.5])
    s = _state_with_x([3, 1, 0.5], None)
    s.H[0, 3:6] = f32([-1, 0, 0]).view(np.int32)
    assert _invalid(dl.step(tab, kinds, s, 0, True))
    # d2 == 0: x is the sampled point itself (0 / 0 is a NaN, which is invalid too)
    FixedDraws(monkeypatch, [0.25, 0.5, 0.5])
    assert _invalid(dl.step(tab, kinds, _state_with_x([0.5, 1, 0.5], None), 0, True))
    # a NaN origin
    FixedDraws(monkeypatch, [0.25, 0.5, 0.5])
    assert _invalid(dl.step(tab, kinds, _state_with_x([np.nan, 0, 0.5], None), 0, True))


def test_drop_not_stepped_and_otherwise_by_hand():
    tab, kinds = _two_lights()
    # a path that hit light material 1 after its previous vertex sampled: the emission is dropped, the flag cleared, no draw
    s = _state_with_x([0.5, 1, 0.5], None, n=4)
    s.H[:, 6] = [1, 1, 1, 0]
    s.H[2, 7] = rtmi.RTMI_HIT_SPHERE  # an emissive sphere of that material is no table light
    s.D[:3] = 0                       # lights do not scatter
    s.E[:] = 7
    s.flags[:] = [1, 0, 1, 3]
    s.steps[3] = 5                    # not stepped by step 0
    ls = s.LS.copy()
    ps = dl.step(tab, kinds, s, 0, True)
    assert ps.E.tolist() == [[0, 0, 0], [7, 7, 7], [7, 7, 7], [7, 7, 7]]
    assert ps.flags.tolist() == [0, 0, 0, 2]  # bit 0 cleared, the other bits kept
    assert int(ps.counts[0]) == 3 and int(ps.counts[1]) == 6
    assert (ps.SD == 0).all() and (ps.DR == 0).all() and (ps.ST == 0).all() and np.array_equal(ps.LS, ls)
    # sample == 0 only drops; an empty table samples nothing; a metal vertex samples nothing; an unlisted path keeps all
    for kw, tb in ((dict(sample=False), tab), (dict(sample=True), tab[:0])):
        s = _state_with_x([0.5, 0, 0.5], None)
        ps = dl.step(tb, kinds, s.copy(), 0, **kw)
        assert ps.flags[0] == 0 and (ps.SD == 0).all() and np.array_equal(ps.LS, s.LS) and int(ps.counts[0]) == 3
    s = _state_with_x([0.5, 0, 0.5], None)
    ps = dl.step(tab, np.array([1, 3, 3]), s.copy(), 0, True)
    assert ps.flags[0] == 0 and int(ps.counts[0]) == 3
    s = _state_with_x([0.5, 0, 0.5], None, n=3)
    ps = dl.step(tab, kinds, s.copy(), 0, True, cand=[2, 7, 0])
    assert dl.diff(ps, s) != [] and all(np.array_equal(getattr(ps, k)[1], getattr(s, k)[1]) for k in dl.PathState.FIELDS[:12])
    assert ps.flags.tolist() == [1, 0, 1]


# ------------------------------------------------------------------ the fold, by hand
def test_fold_direct_by_hand():
    # one ended path of three layers: T = E + D where clear.  r = T2; r = T1 + A1 r; r = T0 + A0 r
    E = f32([[[0, 0, 0]], [[0, 0, 0]], [[8, 4, 2]]])
    A = f32([[[0.5, 0.5, 0.5]], [[0.25, 0.5, 1]], [[0, 0, 0]]])
    Dk = f32([[[1, 2, 3]], [[4, 4, 4]], [[0, 0, 0]]])
    occ = np.array([[0], [1], [0]], np.uint8)
    dirs, steps = np.zeros((1, 3), f32), np.array([3])
    # layer 1 is occluded: T1 = 0.  r = (8, 4, 2) -> (2, 2, 2) -> (1, 2, 3) + 0.5 * (2, 2, 2) = (2, 3, 4)
    assert dl.fold_direct(dirs, steps, E, A, Dk, occ).tolist() == [[2, 3, 4]]
    occ[1] = 0  # clear: T1 = (4, 4, 4): r = (4, 4, 4) + (2, 2, 2) = (6, 6, 6) -> (1, 2, 3) + (3, 3, 3)
    assert dl.fold_direct(dirs, steps, E, A, Dk, occ).tolist() == [[4, 5, 6]]
    # alive (Trace would cut it): r = 0 first, so layer 2's A counts: r = (8, 4, 2) + 0 ...
    assert dl.fold_direct(np.ones((1, 3), f32), steps, E, A, Dk, occ).tolist() == [[4, 5, 6]]
    # two steps made: layer 2 is never read
    assert dl.fold_direct(dirs, np.array([2]), E, A, Dk, occ).tolist() == [[f32(1 + 0.5 * 4), f32(2 + 0.5 * 4), f32(3 + 0.5 * 4)]]
    assert dl.fold_direct(dirs, np.array([0]), E, A, Dk, occ).tolist() == [[0, 0, 0]]


def test_fold_direct_reduces_to_the_plain_fold():
    rng = np.random.default_rng(4)
    n, L = 200, 5
    E, A = rng.uniform(0, 2, (L, n, 3)).astype(f32), rng.uniform(0, 1, (L, n, 3)).astype(f32)
    dirs = rng.uniform(-1, 1, (n, 3)).astype(f32)
    dirs[::3] = 0
    steps = rng.integers(0, L + 2, n)
    want = bouncelib.fold(dirs, steps, E, A)
    Dk = rng.uniform(0, 1, (L, n, 3)).astype(f32)
    assert np.array_equal(dl.fold_direct(dirs, steps, E, A, np.zeros_like(E), np.zeros((L, n), np.uint8)), want)
    assert np.array_equal(dl.fold_direct(dirs, steps, E, A, Dk, np.ones((L, n), np.uint8)), want)
    assert not np.array_equal(dl.fold_direct(dirs, steps, E, A, Dk, np.zeros((L, n), np.uint8)), want)
