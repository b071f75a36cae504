"""One-off campaign (GPU box): the scheduling modes of round 4 on seeded random list worlds (tests/worlds.py:
random_world) at frames large enough to be scheduled (the fuzz worlds of tools/gpu_fuzz.py are a few hundred pixels: thin
frames, no probe).  Every world is rendered by the plain queue in image order and then under every other mode -- longest-
first queue, wave priorities, planned chains (also with one workgroup per CU: long chains and many take-overs), thin
frames -- and all results must agree bit for bit (image, per-pixel ray counts, final RNG states, ray total); every
`oracle_every`-th world is also rendered by the oracle.  usage: gpu_fuzz_modes.py <first> <count> [oracle_every=8]"""
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "ray-tracing-cuda_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
import parity
from rtmi.scenes import v3, PI_D
from worlds import random_world


def differs(got, want, what):
    try:
        parity.assert_same_frame(got, want, what, nan_ok=True)
    except AssertionError as e:
        return str(e)

first, count = int(sys.argv[1]), int(sys.argv[2])
oracle_every = int(sys.argv[3]) if len(sys.argv) > 3 else 8
MODES = (dict(schedule=0, plan=0, wave_priority=0, lane_stride=1),
         dict(schedule=2, plan=0, wave_priority=0, lane_stride=1),
         dict(schedule=2, plan=0, wave_priority=16, lane_stride=1),
         dict(schedule=2, plan=2, wave_priority=16, lane_stride=1),
         dict(schedule=2, plan=2, wave_priority=2, lane_stride=1, blocks_per_cu=1),
         dict(schedule=2, plan=2, wave_priority=64, lane_stride=1, probe_spp=1, blocks_per_cu=2),
         dict(schedule=2, plan=0, wave_priority=8, lane_stride=4),
         dict(schedule=2, plan=2, wave_priority=16, lane_stride=1, first_pass=0),
         dict(schedule=2, plan=0, wave_priority=16, lane_stride=1, first_pass=3),
         dict())
bad = 0
t0 = time.time()
for seed in range(first, first + count):
    rng = np.random.default_rng(9000 + seed)
    h, w = int(rng.integers(64, 161)), int(rng.integers(64, 201))
    spp, depth = int(rng.choice([64, 64, 96, 128])), int(rng.choice([3, 10, 25]))
    post = bool(rng.integers(0, 2))
    n_objects = int(rng.integers(3, 14))
    many = seed % 3 == 2
    state = rng.bit_generator.state

    def fill(b):
        rng.bit_generator.state = state
        b.camera_pinhole(v3(0, 1.0, 2.5), v3(0, 0.4, -2), v3(0, 1, 0), PI_D / 3, w / h)
        random_world(b, rng, n_objects, many)

    ob, pb = parity.build_pair(fill, 77 + seed)
    want = None
    for kw in MODES:
        got = parity.gpu_frame(pb, h, w, spp, depth, post, kw)
        want = want or got
        if differs(got, want, "seed %d, %s" % (seed, kw)):
            bad += 1
            print("MISMATCH seed", seed, kw, flush=True)
    if oracle_every and seed % oracle_every == 0:
        if differs(parity.gpu_frame(pb, h, w, spp, depth, post), parity.oracle_frame(ob, h, w, spp, depth, post), "seed %d" % seed):
            bad += 1
            print("ORACLE MISMATCH seed", seed, flush=True)
print("mode seeds %d..%d (%d modes each, oracle every %d): %d mismatches, %.1fs" % (first, first + count - 1, len(MODES), oracle_every, bad, time.time() - t0), flush=True)
sys.exit(1 if bad else 0)
