"""One-off campaign: tests/test_gpu_random_scenes.py::test_scheduler_paths_agree_on_random_mesh_worlds over many seeds."""
import sys, os, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "ray-tracing-cuda_amd")); sys.path.insert(0, os.path.join(ROOT, "tests"))
import rtmi
from parity import assert_same_frame, gpu_frame
from worlds import SCHEDULER_PATHS, scheduler_mesh_world
first, count = int(sys.argv[1]), int(sys.argv[2])
bad = 0; t0 = time.time()
for seed in range(first, first + count):
    fill, h, w, spp, depth = scheduler_mesh_world(seed)
    pb = rtmi.SceneBuilder(90 + seed)
    fill(pb)
    pb.commit()
    plain = gpu_frame(pb, h, w, spp, depth, opts=SCHEDULER_PATHS[0][1])
    try:
        for world, opts in SCHEDULER_PATHS[1:]:
            assert_same_frame(gpu_frame(pb, h, w, spp, depth, opts=opts, world=world), plain, "%d shard(s), %s" % (world, opts))
    except AssertionError as e:
        bad += 1; print("MISMATCH seed", seed, str(e)[:200], flush=True)
print("scheduler seeds %d..%d: %d mismatches, %.1fs" % (first, first + count - 1, bad, time.time() - t0), flush=True)
