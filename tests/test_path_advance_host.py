"""rtmi_path_advance on the host side: the export of both builds and its declaration, a C99 program that links it, the
argument checks that come before any HIP call, the Python binding's refusals, the kernel's metadata, and the numpy
restatement of the per-candidate rule (tests/advancelib.py) held to hand-worked items and, driven by a toy step function,
to rtmi_path_fold + rtmi_sample_add applied per sample.  No GPU involved."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import rtmi
from abi_host import DUMMY, ERR_DEPTH, ERR_INVALID, LIBS, ROOT, _count, _frame, _refused
from advancelib import IN_FLIGHT, Wavefront, advance, camera_ray, draw01, live_items, toy_step
from bouncelib import fold
from common import kernel_notes
from parity import bits

LIB_DIR = os.path.dirname(rtmi.LIB_PATH)
F32 = np.float32


def test_entry_is_exported_by_both_builds_declared_and_bound():
    L = rtmi.lib()
    assert L.rtmi_version() == 3  # additive: no version change
    header = open(os.path.join(ROOT, "include", "rtmi.h")).read()
    for lib in LIBS:
        syms = subprocess.run(["nm", "-D", "--defined-only", lib], stdout=subprocess.PIPE, text=True, check=True).stdout
        assert re.search(r"\bT rtmi_path_advance$", syms, re.M), lib
    assert "rtmi_path_advance" in [s[0] for s in rtmi.SYMBOLS] and re.search(r"\brtmi_path_advance\(", header)
    assert re.search(r"typedef struct rtmi_path_advance_args \{", header)
    assert C.sizeof(rtmi.PathAdvanceArgs) == 160
    # the section sits behind "live paths", and names what the loop cannot do
    assert header.index("-- live paths --") < header.index("-- path advance --") < header.index("-- direct --")
    assert "Next-event estimation inside this loop is not offered" in header


C_PROG = r'''
#include <stdio.h>
#include <string.h>
#include "rtmi.h"
typedef int (*advance_fn)(const rtmi_scene *, const rtmi_frame *, const rtmi_path_advance_args *, void *);
int main(void) {
  advance_fn advance = &rtmi_path_advance;
  rtmi_frame f = {16, 16, 2, 4, 0, 0, 1};
  rtmi_path_advance_args a;
  rtmi_scene *s = rtmi_scene_create();
  if (sizeof(a) != 160) return 1;
  memset(&a, 0, sizeof(a));
  a.size = (int32_t)sizeof(a);
  if (advance(NULL, &f, &a, NULL) != RTMI_ERR_INVALID || !strstr(rtmi_last_error(), "null scene")) return 2;
  if (advance(s, &f, &a, NULL) != RTMI_ERR_INVALID || !strstr(rtmi_last_error(), "committed")) return 3;
  a.size = 8;
  if (advance(s, &f, &a, NULL) != RTMI_ERR_INVALID || !strstr(rtmi_last_error(), "size")) return 4;
  rtmi_scene_destroy(s);
  printf("path-advance abi ok\n");
  return 0;
}
'''


def test_entry_links_from_c99(tmp_path):
    src = tmp_path / "advance.c"
    src.write_text(C_PROG)
    exe = tmp_path / "advance"
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-pedantic", "-I", os.path.join(ROOT, "include"), str(src),
                    "-L", LIB_DIR, "-lrtmi", "-Wl,-rpath," + LIB_DIR, "-Wl,-rpath,/opt/rocm/lib", "-o", str(exe)], check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, (r.returncode, r.stdout, r.stderr)
    assert "path-advance abi ok" in r.stdout


# ------------------------------------------------------------------ refusals before any HIP call
REQUIRED = ("d_origins", "d_dirs", "d_states", "d_steps", "d_emitted", "d_attenuation", "d_cursor", "d_sum", "d_samples")
STACKS = ("d_emitted_stack", "d_attenuation_stack")
OPTIONAL = ("d_budget", "d_list", "d_count", "d_sq", "d_ray_counts", "d_counts")


def _args(n_list, **kw):
    a = rtmi.PathAdvanceArgs()
    a.size, a.reserved, a.n_list = C.sizeof(rtmi.PathAdvanceArgs), 0, n_list
    for k in REQUIRED + STACKS:
        setattr(a, k, DUMMY.value)
    for k, v in kw.items():
        setattr(a, k, v.value if isinstance(v, C.c_void_p) else v)
    return a


def _call(s, f, a):
    return rtmi.lib().rtmi_path_advance(s, C.byref(f) if f is not None else None, C.byref(a) if a is not None else None, None)


def test_argument_checks_before_any_hip_call():
    b = rtmi.SceneBuilder(1)  # never committed, no camera
    f = _frame()
    items = rtmi.work_items(f)
    assert _refused(_call(None, f, _args(items)), b"null scene")
    assert _refused(_call(b.h, None, _args(items)), b"frame")
    assert _refused(_call(b.h, _frame(height=0), _args(items)), b"frame")
    assert _refused(_call(b.h, _frame(post=True), _args(items)), b"post_process")
    assert _refused(_call(b.h, f, None), b"null rtmi_path_advance_args")
    assert _refused(_call(b.h, f, _args(items, size=152)), b"size")
    assert _refused(_call(b.h, f, _args(items, reserved=1)), b"reserved")
    # the projection, as rtmi_camera_rays refuses it
    for proj, word in ((rtmi.Projection(12, 0, 0.0, 0), b"rtmi_projection.size"), (rtmi.Projection(16, 0, 0.0, 1), b"reserved"),
                       (rtmi.Projection(16, 7, 0.0, 0), b"kind"), (rtmi.projection("fisheye", 0.0), b"fov"),
                       (rtmi.projection("fisheye", 7.0), b"fov"), (rtmi.projection("orthographic"), b"orthonormal")):
        assert _refused(_call(b.h, f, _args(items, proj=C.pointer(proj))), word), word
    # the depth
    assert _refused(_call(b.h, _frame(max_depth=-1), _args(items)), b"max_depth", ERR_DEPTH)
    assert _refused(_call(b.h, _frame(max_depth=rtmi.MAX_DEPTH + 1), _args(items)), b"max_depth", ERR_DEPTH)
    # the list
    assert _refused(_call(b.h, f, _args(-1)), b"negative")
    assert _refused(_call(b.h, f, _args(1 << 31, d_list=DUMMY)), b"2^31")
    assert _refused(_call(b.h, f, _args(items + 1)), b"n_list")  # a null list is the identity: no more entries than items
    # the arrays
    for k in REQUIRED:
        assert _refused(_call(b.h, f, _args(items, **{k: None})), b"null"), k
    for k in STACKS:
        assert _refused(_call(b.h, f, _args(items, **{k: None})), b"stack"), k
    # everything in order: the scene is looked at last
    assert _refused(_call(b.h, f, _args(items)), b"committed")
    assert _refused(_call(b.h, f, _args(items + 9, d_list=DUMMY, d_count=DUMMY)), b"committed")  # (entries >= items are dropped)
    assert _refused(_call(b.h, _frame(max_depth=0), _args(items, d_emitted_stack=None, d_attenuation_stack=None)), b"committed")
    assert _refused(_call(b.h, _frame(max_depth=rtmi.MAX_DEPTH), _args(items)), b"committed")
    assert _refused(_call(b.h, f, _args(0, **{k: None for k in REQUIRED + STACKS})), b"committed")  # (nothing to do, nothing needed)
    for k in OPTIONAL:
        assert _refused(_call(b.h, f, _args(items, **{k: DUMMY})), b"committed"), k
    assert _refused(_call(b.h, f, _args(items, proj=C.pointer(rtmi.projection("camera")))), b"committed")


def test_python_refusals_come_before_any_gpu_work():
    assert hasattr(rtmi.Renderer, "path_advance") and hasattr(rtmi.Renderer, "render_wavefront")
    import inspect
    sig = inspect.signature(rtmi.Renderer.render_wavefront)
    assert [p for p in sig.parameters][1:] == ["budget", "projection", "count_rays", "each", "poll"]
    assert sig.parameters["poll"].default == 8
    sig = inspect.signature(rtmi.Renderer.path_advance)
    assert [p for p in sig.parameters][1:12] == ["paths", "origins", "directions", "steps", "emitted", "attenuation", "stacks",
                                                  "cursor", "budget", "projection", "counts"]


def test_kernels_spill_no_vgpr_and_use_no_scratch_or_lds():
    """Two kernels in both builds: path_advance_kernel<false> for the CAMERA and ORTHOGRAPHIC kinds, without the binary64
    sines and cosines of the curved kinds and at four waves per SIMD or more, and path_advance_kernel<true>."""
    for lib in LIBS:
        blk = {n: b for n, b in kernel_notes(lib).items() if "path_advance_kernel" in n}
        assert len(blk) == 2, (lib, sorted(blk))
        for n, b in blk.items():
            assert _count(b, "vgpr_spill_count") == 0, (lib, n)
            assert _count(b, "private_segment_fixed_size") == 0 and _count(b, "group_segment_fixed_size") == 0, (lib, n)
        plain = [b for n, b in blk.items() if "ILb0E" in n]
        assert len(plain) == 1 and _count(plain[0], "vgpr_count") <= 128, lib


# ------------------------------------------------------------------ the state machine, by hand
UP = (0.0, 0.0, 1.0)


def fixed_rays(script):
    """A ray_fn that hands out script[q]'s directions in order (origin (q, 0, 0)) and bumps the state's first word."""
    at = {}

    def ray_fn(q, idx, state):
        state[0] += np.uint32(1)
        k = at.get(q, 0)
        at[q] = k + 1
        return np.array([q, 0, 0], F32), np.asarray(script[q][k], F32)

    return ray_fn


def hand(pixel_of, spp, depth, budget=None):
    return Wavefront(pixel_of, spp, depth, np.zeros((len(pixel_of), 6), np.uint32), budget)


def f32(*x):
    return np.asarray(x, F32)


def test_a_path_that_ends_in_layer_2():
    wf = hand([0], 1, 4)
    rays = fixed_rays({0: [UP]})
    advance(wf, rays)
    assert wf.cursor[0].tolist() == [IN_FLIGHT | 1, 0] and wf.steps[0] == 0 and wf.dirs[0].tolist() == list(UP)
    assert wf.counts.tolist() == [0, 0, 1] and wf.samples[0] == 0
    E = [f32(0.5, 0.25, 0.125), f32(1, 2, 3), f32(4, 5, 6)]
    A = [f32(0.5, 0.5, 0.5), f32(0.25, 0.5, 1), f32(9, 9, 9)]
    for k in range(3):
        toy_step(wf, 0, ends=(k == 2), emitted=E[k], attenuation=A[k])
        advance(wf, rays, [0])
        if k < 2:
            assert wf.cursor[0].tolist() == [IN_FLIGHT | 1, k + 1] and wf.samples[0] == 0
    # E0 + A0 * (E1 + A1 * E2), every product and sum exact here
    want = f32(0.5 + 0.5 * (1 + 0.25 * 4), 0.25 + 0.5 * (2 + 0.5 * 5), 0.125 + 0.5 * (3 + 1 * 6))
    assert np.array_equal(wf.sum[0], want) and np.array_equal(wf.sq[0], want * want)
    assert wf.samples[0] == 1 and wf.ray_counts[0] == 3, "an ended path of 3 steps made 3 queries"
    assert wf.cursor[0].tolist() == [1, 3], "F clear, k == b, the three layers still counted"
    assert not bits(wf.dirs[0]).any() and wf.counts.tolist() == [1, 3, 1]
    assert np.array_equal(wf.e_stack[:3, 0], np.stack(E)) and np.array_equal(wf.a_stack[:3, 0], np.stack(A))
    assert not wf.e_stack[3].any(), "layer 3 was never written"
    assert len(live_items(wf)) == 0


def test_a_path_cut_at_max_depth():
    wf = hand([0], 1, 2)
    rays = fixed_rays({0: [UP]})
    advance(wf, rays)
    toy_step(wf, 0, False, f32(1, 1, 1), f32(0.5, 0.5, 0.5))
    advance(wf, rays, [0])
    assert wf.samples[0] == 0 and len(live_items(wf)) == 1
    toy_step(wf, 0, False, f32(2, 4, 8), f32(7, 7, 7))
    advance(wf, rays, [0])
    want = f32(1 + 0.5 * 2, 1 + 0.5 * 4, 1 + 0.5 * 8)  # alive: r = 0, then E1 + A1 * 0, then E0 + A0 * that
    assert np.array_equal(wf.sum[0], want) and wf.samples[0] == 1
    assert wf.ray_counts[0] == 3, "two steps and the query Trace makes before it sees the depth"
    assert wf.cursor[0].tolist() == [1, 2] and not bits(wf.dirs[0]).any()
    # whatever the caller does to d_steps, nothing is pushed past the stacks
    wf2 = hand([0], 1, 2)
    advance(wf2, rays_b := fixed_rays({0: [UP]}))
    wf2.cursor[0, 1] = 2
    wf2.steps[0] = 3
    advance(wf2, rays_b, [0])
    assert wf2.cursor[0].tolist() == [1, 3] and wf2.samples[0] == 1


def test_a_fresh_zero_ray_finishes_at_once():
    wf = hand([0], 2, 4)
    rays = fixed_rays({0: [(0.0, -0.0, 0.0), UP]})
    advance(wf, rays)
    assert wf.samples[0] == 1 and not bits(wf.sum[0]).any() and wf.ray_counts[0] == 0, "radiance 0, no query"
    assert wf.cursor[0].tolist() == [IN_FLIGHT | 2, 0] and wf.dirs[0].tolist() == list(UP), "the second sample is in flight"
    assert wf.states[0, 0] == 2 and wf.counts.tolist() == [1, 0, 2]


def test_max_depth_0_runs_every_sample_in_one_call():
    wf = hand([0, 1], 3, 0, budget=[5, 2])
    rays = fixed_rays({0: [UP] * 3, 1: [UP] * 2})
    advance(wf, rays)
    assert wf.samples.tolist() == [3, 2] and wf.ray_counts.tolist() == [3, 2], "one query per sample, as Trace makes at depth 0"
    assert not bits(wf.sum).any() and not bits(wf.dirs).any()
    assert wf.cursor.tolist() == [[3, 0], [2, 0]] and wf.counts.tolist() == [5, 5, 5]
    assert wf.states[:, 0].tolist() == [3, 2]


def test_a_budget_of_0_and_padding():
    wf = hand([0, -1, 1], 4, 3, budget=[0, 9, 1])
    wf.dirs[:] = 5.0
    wf.origins[:] = 6.0
    wf.cursor[1] = (77, 88)  # (padding: never read)
    rays = fixed_rays({2: [UP]})
    advance(wf, rays, [0, 1, 2, 3, 1 << 31])  # (3 and 2^31 are no work items)
    assert not bits(wf.dirs[:2]).any(), "no samples left, and padding: a zero direction"
    assert (wf.origins[:2] == 6.0).all() and wf.cursor[:2].tolist() == [[0, 0], [77, 88]]
    assert wf.states[:2].sum() == 0 and wf.samples.tolist() == [0, 0, 0]
    assert wf.cursor[2].tolist() == [IN_FLIGHT | 1, 0] and wf.origins[2].tolist() == [2, 0, 0]
    assert wf.counts.tolist() == [0, 0, 1]
    # an item that is not a candidate keeps every word
    wf.dirs[0] = 5.0
    advance(wf, rays, [2, 0], count_in=1)
    assert (wf.dirs[0] == 5.0).all()


# ------------------------------------------------------------------ the loop, against fold + add per sample
def test_toy_loop_reproduces_fold_and_sample_add_per_sample():
    f = _frame(spp=5, max_depth=4)
    depth, spp = 4, 5
    pixel_of = rtmi.pixel_map(f)
    n = len(pixel_of)
    rng = np.random.default_rng(7)
    states = rng.integers(1, 1 << 32, (n, 6), dtype=np.uint64).astype(np.uint32)
    budget = rng.integers(0, 8, n)
    budget[rng.random(n) < 0.2] = 0
    cam = np.array([[0, 1, 6], [-1, 0, 4], [2, 0, 0], [0, 2, 0], [1, 0, 0], [0, 1, 0], [0, 0, 1]], F32)
    h, w = f.height, f.width
    wf = Wavefront(pixel_of, spp, depth, states, budget)
    ray_fn = lambda q, idx, st: camera_ray(cam, h, w, idx, st)
    # every sample's script: its steps, whether the last one ends the path, and the layers
    script = {}
    for q in range(n):
        for k in range(min(int(budget[q]), spp)):
            L = int(rng.integers(1, depth + 1))
            ends = True if L < depth else bool(rng.integers(0, 2))
            script[q, k] = (L, ends, rng.uniform(-2, 2, (L, 3)).astype(F32), rng.uniform(0, 1, (L, 3)).astype(F32))

    def step(lst):
        for q in lst:
            k, s = (int(wf.cursor[q, 0]) & (IN_FLIGHT - 1)) - 1, int(wf.steps[q])
            L, ends, E, A = script[q, k]
            toy_step(wf, q, ends and s + 1 == L, E[s], A[s])

    advance(wf, ray_fn)
    lst, iterations = live_items(wf), 0
    while len(lst):
        step(lst)
        advance(wf, ray_fn, lst)
        lst = live_items(wf, lst)
        iterations += 1
        assert iterations <= spp * depth
    # what rtmi_camera_rays, the steps, rtmi_path_fold and rtmi_sample_add make of the same scripts, sample by sample
    want_sum, want_sq = np.zeros((n, 3), F32), np.zeros((n, 3), F32)
    want_n, want_rays, want_states = np.zeros(n, np.uint32), np.zeros(n, np.uint32), states.copy()
    for (q, k), (L, ends, E, A) in sorted(script.items()):
        draw01(want_states[q]), draw01(want_states[q])
        d = np.zeros((1, 3), F32) if ends else np.array([UP], F32)
        x = fold(d, [L], E[:, None, :], A[:, None, :])[0]
        want_sum[q] = (want_sum[q] + x).astype(F32)
        want_sq[q] = (want_sq[q] + (x * x).astype(F32)).astype(F32)
        want_n[q] += 1
        want_rays[q] += L + (0 if ends else 1)
    pix = pixel_of >= 0
    assert np.array_equal(bits(wf.sum[pix]), bits(want_sum[pix])) and np.array_equal(bits(wf.sq[pix]), bits(want_sq[pix]))
    assert np.array_equal(wf.samples[pix], want_n[pix]) and np.array_equal(wf.ray_counts[pix], want_rays[pix])
    assert np.array_equal(wf.states[pix], want_states[pix])
    assert not wf.samples[~pix].any() and np.array_equal(wf.states[~pix], states[~pix]), "padding is never touched"
    b = np.minimum(budget, spp)
    assert np.array_equal(wf.cursor[pix, 0], b[pix].astype(np.uint32)), "every k == b, every F clear"
    assert wf.counts.tolist() == [int(b[pix].sum()), int(want_rays[pix].sum()), int(b[pix].sum())]
    assert not bits(wf.dirs).any()
    assert (~pix).any() and (b[pix] == 0).any() and (budget[pix] > spp).any()
