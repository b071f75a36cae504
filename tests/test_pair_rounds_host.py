"""Host side of the pair rounds (closest_hit.h, RUN_TRIS, step (b)): the schedule of a flush's rounds, which is a pure
function of the flush's task count and the threshold in a header of its own (csrc/pair_rounds.h), compiled here into a
small program and checked round by round; and the code-object metadata of the six kernels that run it.  No GPU.

The constants are those of the sources, restated: the test holds the library to the numbers, not to its own headers."""
import os
import re
import subprocess
import tempfile

import pytest

import numpy as np

import common
import oraclelib
import pair_rounds_worlds as pw
from abi_host import LIBS, ROOT, _count, _waves

PAIR_ROUND_MIN = 32   # kPairRoundMin (kernels.h)
LIST_TASKS = 192      # kListTasks of the untextured triangle kernels (scene_dev.h): the most tasks a flush holds
COUNTS = (0, 1, 32, 33, 64, 65, 96, 97, 128, 192)

PROGRAM = r"""
#include <cstdio>
#include <cstdlib>
#include "pair_rounds.h"
int main(int argc, char **argv) {
  const int pair_min = std::atoi(argv[1]);
  for (int a = 2; a < argc; a++) {
    int first[16], count[16], pair[16];
    const int n = std::atoi(argv[a]), r = pair_round_plan(n, pair_min, 16, first, count, pair);
    std::printf("%d %d", n, r);
    for (int i = 0; i < r && i < 16; i++) std::printf(" %d:%d:%d", pair[i], first[i], count[i]);
    std::printf("\n");
  }
  return 0;
}
"""


@pytest.fixture(scope="module")
def plan():
    """plan(pair_min, counts) -> {n: [(is a pair round, first task, tasks), ...]} by the header's own function."""
    with tempfile.TemporaryDirectory() as tmp:
        src, exe = os.path.join(tmp, "plan.cc"), os.path.join(tmp, "plan")
        with open(src, "w") as fh:
            fh.write(PROGRAM)
        subprocess.check_call(["c++", "-std=c++17", "-I", os.path.join(ROOT, "ray-tracing-cuda_amd", "csrc"), src, "-o", exe])

        def run(pair_min, counts):
            out = {}
            for line in subprocess.check_output([exe, str(pair_min)] + [str(n) for n in counts], text=True).splitlines():
                n, r, *rounds = line.split()
                assert int(r) == len(rounds) <= 16
                out[int(n)] = [tuple(int(x) for x in rd.split(":")) for rd in rounds]
            return out
        yield run


def today(n):
    return -(-2 * n // 64)  # triangle rounds alone: ceil(2 n / 64)


@pytest.mark.parametrize("pair_min", (32, 40, 48))
def test_every_task_is_tested_once_and_pairs_come_first(plan, pair_min):
    rounds = plan(pair_min, range(0, LIST_TASKS + 1))
    for n in range(0, LIST_TASKS + 1):
        seen, pairs_over = [], False
        for is_pair, first, count in rounds[n]:
            assert count >= 1 and first == len(seen), (n, rounds[n])  # the rounds follow each other without a gap
            if is_pair:
                assert not pairs_over, (n, rounds[n])                # no triangle round before the last pair round
                assert count == min(64, n - first) and n - first > pair_min, (n, rounds[n])
            else:
                pairs_over = True
                assert count <= 32, (n, rounds[n])                   # 64 triangles, two to a task
            seen += range(first, first + count)
        assert seen == list(range(n)), (n, rounds[n])                # every task exactly once
        left = n - sum(c for p, _, c in rounds[n] if p)
        assert left <= pair_min, (n, rounds[n])                      # what the triangle rounds get
        assert sum(1 for p, _, _ in rounds[n] if not p) == today(left), (n, rounds[n])


def test_the_schedule_at_its_steps(plan):
    """The table of the change: T a triangle round, P a pair round."""
    got = {n: "".join("P" if p else "T" for p, _, _ in r) for n, r in plan(PAIR_ROUND_MIN, COUNTS).items()}
    assert got == {0: "", 1: "T", 32: "T", 33: "P", 64: "P", 65: "PT", 96: "PT", 97: "PP", 128: "PP", 192: "PPP"}
    full = plan(PAIR_ROUND_MIN, COUNTS)
    assert full[65] == [(1, 0, 64), (0, 64, 1)] and full[97] == [(1, 0, 64), (1, 64, 33)] and full[33] == [(1, 0, 33)]
    # never more rounds than triangle rounds alone, and fewer from 33 tasks on
    for n, r in plan(PAIR_ROUND_MIN, range(0, LIST_TASKS + 1)).items():
        assert len(r) <= today(n) and (n <= 32 or len(r) < today(n)), (n, r)


def test_a_threshold_above_the_largest_flush_leaves_triangle_rounds_alone(plan):
    for n, r in plan(LIST_TASKS + 1, range(0, LIST_TASKS + 1)).items():
        assert len(r) == today(n) and not any(p for p, _, _ in r), (n, r)


# render_kernel<F_TRIS, 255 / 767> walk planned chains, <383 / 895> and their probe twins draw from the queue
CHAINS = ("render_kernelILj2ELj255E", "render_kernelILj2ELj767E")
QUEUED = ("render_kernelILj2ELj383E", "render_kernelILj2ELj895E", "probe_kernelILj2ELj383E", "probe_kernelILj2ELj895E")


def _block(notes, key):
    got = [blk for name, blk in notes.items() if key in name]
    assert len(got) == 1, key
    return got[0]


def test_the_pinned_kernels_are_in_both_builds():
    for lib in LIBS:
        notes = common.kernel_notes(lib)
        for key in CHAINS + QUEUED:
            assert re.search(r"\.group_segment_fixed_size:\s+0\b", _block(notes, key)), (lib, key)


def test_the_pinned_kernels_keep_their_registers():
    """The product: at most 80 VGPRs and six waves per SIMD; the chains kernels spill no VGPR dword, at most five scalars
    and use no scratch; the queue and probe kernels spill no more than they did before the pair rounds (0 dwords, 3
    scalars)."""
    notes = common.kernel_notes(LIBS[0])
    for key in CHAINS + QUEUED:
        blk = _block(notes, key)
        print(key, {k: _count(blk, k) for k in ("vgpr_count", "sgpr_count", "vgpr_spill_count", "sgpr_spill_count")})
        assert _count(blk, "vgpr_count") <= 80 and _waves(_count(blk, "vgpr_count")) == 6, key
        assert _count(blk, "vgpr_spill_count") == 0, key
        assert _count(blk, "sgpr_spill_count") <= (5 if key in CHAINS else 3), key
    for key in CHAINS:
        assert _count(_block(notes, key), "private_segment_fixed_size") == 0, key


# ------------------------------------------------------------------ the stacks of tests/pair_rounds_worlds.py on the oracle
@pytest.mark.parametrize("spp", (8, 64))
@pytest.mark.parametrize("k", (2, 3))
def test_a_narrowed_stack_covers_exactly_j_pixels_and_shows_its_nearest_sheet(k, spp):
    """What the GPU tests take for granted: the sheets are listed far to near, so the first candidate is the farthest and
    every nearer sheet's test passes against it; a frame then shows the nearest sheet on exactly the first j pixels in
    raster order and the farthest on the rest -- a lost key or a key in a wrong slot would be a wrong pixel."""
    def frame(kk, j):
        ob = oraclelib.OracleBuilder(7)
        pw.stack(kk, j)(ob)
        rgb, _, _, total = ob.render(8, 8, spp, 8, post=True)
        assert total == 64 * spp, "every path is its camera ray"
        return rgb.reshape(64, 3).view(np.uint32)
    near, far = frame(k, 64)[0], frame(k, 0)[0]
    assert not np.array_equal(near, far) and not np.array_equal(near, frame(5 - k, 64)[0])
    for j in pw.PARTIAL:
        f = frame(k, j)
        assert (f[:j] == near).all() and (f[j:] == far).all(), (k, j)
