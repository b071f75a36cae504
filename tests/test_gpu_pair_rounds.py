"""The pair rounds of the fast list kernels' flushes (closest_hit.h, RUN_TRIS, step (b); pair_rounds.h) against the oracle
and the general kernel, bit for bit: image, per-pixel ray counts, final RNG states, ray total (tests/parity.py).

A flush of the culled scan's shared tests is tested a pair per lane while more than 32 of its tasks are untested, and the
rest a triangle per lane.  A pair round posts the keys the triangle rounds would and flags the flushes they would, so every
frame must be the oracle's and the general kernel's (fast_path = -1), whose flushes know neither keys nor pair rounds.
tests/pair_rounds_worlds.py builds flushes of chosen sizes: stacks of 2 to 5 emitting sheets in front of an 8 x 8 frame,
listed far to near, so that the sheet a lane tests from its own registers is the farthest and every handed-over task
passes against the bound it left and posts a key -- k - 1 competing keys per ray, of which the nearest sheet's must win
(64, 128, 192 and 256 tasks: the last is two flushes), the nearer sheets narrowed to j of the 64 pixels with j dense
around the schedule's steps (the frame shows which j pixels got a key), a lone Triangle among the sheets (an absent
second record in a pair round, and the winner where no nearer sheet covers), the ordered world made
denser and listed twice (tasks of the ordered kind inside pair rounds: rtmi_debug_counters' word 16 must be the host
restatement's count), and the Cornell box.

A frame of fewer than eight samples has no pinned kernel and chains are planned from 64 samples on, so every world runs
twice: 8 samples from the queue (render_kernel<895>, or <383> where the scene holds a material that is neither Lambertian
nor light), and 64 samples with a first pass of 32 (probe_kernel<895 / 383>, then render_kernel<767 / 255> on planned
chains).  Every case asserts which kernels its launches were (rtmi_render_pins).  The margin-check build counts the two
kinds of round and must find every regime reached (tests/pair_rounds_check.py).  No tolerances."""
import ctypes as C
import functools
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import diffuse_worlds as dw
import min_fold_worlds as mf
import pair_rounds_worlds as pw
import rtmi
from abi_host import CHECK_LIB, ROOT
from diffuse_worlds import render_pins
from pair_slab_worlds import PLANNED, assert_launch
from parity import assert_same_frame, bits, build_pair, gpu_frame, oracle_frame

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

PIN_DIFFUSE = 512
QUEUE_PINS, CHAIN_PINS = 383, 255
QUEUE = dict(lane_stride=1)  # one launch from the queue
LAUNCHES = {"queue": (8, QUEUE), "planned": (64, PLANNED)}  # PLANNED: a first pass of 32 samples from the queue, then chains
ORDERED_WORD = 16


def expected_pins(launch, diffuse):
    extra = PIN_DIFFUSE if diffuse else 0
    return (0, QUEUE_PINS | extra) if launch == "queue" else (QUEUE_PINS | extra, CHAIN_PINS | extra)


def world(name):
    """name -> (fill, seed, depth, diffuse)."""
    kind, *a = name.split("/")
    if kind == "stack":      # stack/k/j[/metal][/lone]
        return pw.stack(int(a[0]), int(a[1]), "metal" in a, "lone" in a), 7, 8, "metal" not in a
    if kind == "ordered":
        return pw.ordered_twice, pw.SEED, pw.DEPTH, True
    return (dw.cornell_and_an_unused_metal if "metal" in a else dw.cornell), dw.CORNELL_SEED, int(a[0]), "metal" not in a


def colours(frame):
    """The frame's pixels as rows of three 32-bit words."""
    return bits(frame.image).reshape(-1, 3)


def covered(frame):
    """Pixels of an 8 x 8 frame that do not have the colour of its last pixel, which no narrowed sheet covers."""
    c = colours(frame)
    return int((c != c[-1]).any(axis=1).sum())


@functools.lru_cache(maxsize=None)
def pair(name):
    fill, seed, _, _ = world(name)
    return build_pair(fill, seed)


@functools.lru_cache(maxsize=None)
def oracle(name, side, spp):
    """One oracle frame per (world, shape), shared by the cases that need it; read-only (parity.oracle_frame)."""
    return oracle_frame(pair(name)[0], side, side, spp, world(name)[2])


def ordered_count(b):
    c = (C.c_ulonglong * 40)()
    assert rtmi.lib().rtmi_debug_counters(b.h, c, None) == 0
    return int(c[ORDERED_WORD])


def assert_same_buffers(a, b, what):
    assert a.total == b.total and np.array_equal(a.counts, b.counts) and np.array_equal(a.states, b.states), what
    assert np.array_equal(bits(a.image), bits(b.image)), what


def pinned_general_oracle(name, side, launch):
    """The frame by the launch's pinned kernels -- asserted to be the ones the world is built for -- by the general
    kernel and by the oracle: all three the same.  Returns the pinned frame and the count it left in word 16."""
    _, _, depth, diffuse = world(name)
    spp, opts = LAUNCHES[launch]
    what = "%s %d x %d x %d, %s" % (name, side, side, spp, launch)
    pb = pair(name)[1]
    fast = dict(fast_path=1, **opts)
    assert render_pins(pb, side, spp, depth, fast) == expected_pins(launch, diffuse), what
    got = gpu_frame(pb, side, side, spp, depth, opts=fast)
    counted = ordered_count(pb)
    assert_launch(got.mode, launch)
    assert_same_frame(got, oracle(name, side, spp), what + ", pinned kernels")
    slow = dict(fast_path=-1, **opts)
    assert render_pins(pb, side, spp, depth, slow) == (0, 0), what
    general = gpu_frame(pb, side, side, spp, depth, opts=slow)
    assert_same_buffers(got, general, what + ", pinned against general")
    return got, counted


@pytest.mark.parametrize("launch", sorted(LAUNCHES))
@pytest.mark.parametrize("kind", ("diffuse", "metal"))
@pytest.mark.parametrize("k", (2, 3, 4, 5))
def test_sheet_stacks(k, kind, launch):
    """8 x 8: one wave, every lane a ray per sample, every ray a candidate of all k sheets: 64 (k - 1) tasks a flush --
    one, two and three pair rounds, and at k = 5 a flush of 192 tasks and one of 64."""
    name = "stack/%d/64" % k + ("/metal" if kind == "metal" else "")
    got, _ = pinned_general_oracle(name, 8, launch)
    assert got.total == 64 * LAUNCHES[launch][0], "every path is its camera ray"
    # every pixel shows the nearest sheet, listed last: one colour, and not the one a stack a sheet shorter shows
    assert len(np.unique(colours(got), axis=0)) == 1
    other = oracle("stack/%d/64" % (k - 1 if k > 2 else 3), 8, LAUNCHES[launch][0])
    assert not np.array_equal(colours(got)[0], colours(other)[0]), "the nearest sheet's colour depends on k"


@pytest.mark.parametrize("launch", sorted(LAUNCHES))
@pytest.mark.parametrize("k", (2, 3))
@pytest.mark.parametrize("j", pw.PARTIAL)
def test_partial_cover(j, k, launch):
    """(k - 1) j tasks a flush, give or take a ray on a rim: j is dense around 32, 64 and 96 tasks, so the flushes cross
    every step of the schedule whichever way the rims fall -- no pair round, a pair round partly filled, a pair round and a
    triangle round, two pair rounds."""
    got, _ = pinned_general_oracle("stack/%d/%d" % (k, j), 8, launch)
    if j < 64:  # the pixels whose ray handed over a task show the nearest sheet, the others the farthest: exactly j
        assert covered(got) == j, (covered(got), j)


@pytest.mark.parametrize("launch", sorted(LAUNCHES))
@pytest.mark.parametrize("name", ("stack/2/64/lone", "stack/3/33/lone", "stack/2/17/lone/metal"))
def test_a_lone_triangle_among_the_sheets(name, launch):
    """One more task of every ray whose second record is absent: 128 tasks (two pair rounds), 64 + 66 (two pair rounds and
    a short third), 64 + 17 (a pair round and a triangle round).  The triangle lies just in front of the farthest sheet:
    its key wins wherever no nearer sheet covers, so no pixel shows the farthest sheet."""
    got, _ = pinned_general_oracle(name, 8, launch)
    j = int(name.split("/")[2])
    assert len(np.unique(colours(got), axis=0)) == (1 if j == 64 else 2)
    plain = oracle(name.replace("/lone", ""), 8, LAUNCHES[launch][0])
    if j < 64:
        assert covered(got) == j and not np.array_equal(colours(got)[-1], colours(plain)[-1]), "the lone triangle's key won"


def _ordered_need(first_sample, spp):
    ob = pair("ordered")[0]
    O, D, _ = mf.primary_rays(ob.camera_get(), pw.SIDE, pw.SIDE, spp, pw.SEED)
    return pw.ordered_tasks(O[first_sample:].reshape(-1, 3), D[first_sample:].reshape(-1, 3))


@pytest.mark.parametrize("launch", sorted(LAUNCHES))
def test_ordered_tasks_inside_pair_rounds(launch):
    """Every ray of this world is a camera ray the host can restate, with its pairs listed twice: the flushes hold far
    more than 32 tasks, so the tasks of the ordered kind are found by pair rounds, and word 16 -- the last launch's --
    holds exactly as many as the restatement finds among that launch's samples."""
    spp, _ = LAUNCHES[launch]
    first = 0 if launch == "queue" else 32
    need = _ordered_need(first, spp)
    got, counted = pinned_general_oracle("ordered", pw.SIDE, launch)
    print("ordered tasks of samples %d..%d: host %d, device %d" % (first, spp - 1, need, counted))
    assert got.total == pw.SIDE * pw.SIDE * spp, "every path is its camera ray"
    assert need > 0 and counted == need, (counted, need)


@pytest.mark.parametrize("launch", sorted(LAUNCHES))
@pytest.mark.parametrize("name", ("cornell/1", "cornell/2", "cornell/9", "cornell/50", "cornell/9/metal", "cornell/50/metal"))
def test_cornell_box(name, launch):
    """16 x 16 at depths 1, 2, 9 and 50 (the benchmark's): flushes of every size up to 192 tasks, in all six kernels."""
    pinned_general_oracle(name, 16, launch)


def test_the_check_build_counts_the_rounds_and_agrees_on_every_query():
    """librtmi_check1.so answers every query a second time with the plain scan and counts the pair rounds and the
    triangle rounds (tests/pair_rounds_check.py says what each world must show)."""
    assert os.path.exists(CHECK_LIB), "librtmi_check1.so missing: run __graft_entry__.build() (make -C csrc check1)"
    env = dict(os.environ, RTMI_LIB_PATH=CHECK_LIB)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "pair_rounds_check.py")], env=env, cwd=ROOT,
                       stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-4000:]
    out = json.loads(r.stdout[r.stdout.index("{"):])
    print(json.dumps(out, indent=1))
    for tag, v in out.items():
        assert v["fast_path"] == 1, (tag, v)
        assert v["re_done"] == v["rays"] > 0, (tag, v)
        assert v["disagreements"] == 0, (tag, v)
    for launch, spp in (("queue", 8), ("planned", 32)):  # (the counts are the last launch's: 8 samples, or the 32 behind the first pass)
        c = out["cornell/" + launch]
        assert c["pair_rounds"] > 0 and c["tri_rounds"] > 0, c
        full = out["stack/2/64/" + launch]  # one wave, one flush of 64 tasks per sample: a pair round each, nothing left over
        assert full["pair_rounds"] == spp and full["tri_rounds"] == 0, full
        for j in (1, 15, 16):                # at most 16 tasks, and a ray or two on a rim: never more than 32
            few = out["stack/2/%d/%s" % (j, launch)]
            assert few["pair_rounds"] == 0 and few["tri_rounds"] == spp, (j, few)
        assert out["stack/2/0/" + launch]["pair_rounds"] == out["stack/2/0/" + launch]["tri_rounds"] == 0
        mixed = out["stack/3/48/" + launch]  # 96 tasks or a few more: a pair round, then a triangle round or a second pair round
        assert mixed["pair_rounds"] >= spp and mixed["pair_rounds"] + mixed["tri_rounds"] == 2 * spp, mixed
        o = out["ordered/" + launch]  # the tasks of the ordered kind were met inside pair rounds, every one
        assert o["pair_rounds"] > 0 and o["pair_flags"] == o["ordered_tasks"] > 0, o
