"""One-off campaigns: seeded worlds of tests/worlds.py, each rendered by the oracle and through the C ABI and compared
bit for bit (tests/parity.py).  usage: gpu_fuzz.py <first> <count> [<soups> [<far views>]]"""
import sys, os, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "ray-tracing-cuda_amd")); sys.path.insert(0, os.path.join(ROOT, "tests"))
import parity
from rtmi.scenes import v3, PI_D
from worlds import far_view_world, random_case, soup_world


def differs(fill, seed, h, w, spp, depth, post, camera=None, nan_ok=False):
    ob, pb = parity.build_pair(fill, seed, camera)
    try:
        parity.assert_same_frame(parity.gpu_frame(pb, h, w, spp, depth, post), parity.oracle_frame(ob, h, w, spp, depth, post),
                                 "seed %d" % seed, nan_ok)
    except AssertionError as e:
        return str(e)


first, count = int(sys.argv[1]), int(sys.argv[2])
bad = 0
t0 = time.time()
for seed in range(first, first + count):
    fill, h, w, spp, depth, post, n_objects = random_case(seed)
    if differs(fill, 77 + seed, h, w, spp, depth, post):
        bad += 1
        print("MISMATCH seed", seed, h, w, spp, depth, post, n_objects, flush=True)
print("seeds %d..%d: %d mismatches, %.1fs" % (first, first + count - 1, bad, time.time() - t0), flush=True)

# ---- second campaign: triangle soups (many overlapping faces, tiny reference leaves, every material)
if len(sys.argv) > 3:
    bad = 0
    t0 = time.time()
    for seed in range(first, first + int(sys.argv[3])):
        fill, h, w, spp, depth, what = soup_world(seed)
        cam = lambda b: b.camera_pinhole(v3(0, 0.8, 1.8), v3(0, 0.4, -2), v3(0, 1, 0), PI_D / 3, w / h)
        if differs(fill, 300 + seed, h, w, spp, depth, False, cam, nan_ok=True):
            bad += 1
            print("SOUP MISMATCH seed", seed, h, w, spp, depth, what, flush=True)
    print("soup seeds %d..%d: %d mismatches, %.1fs" % (first, first + int(sys.argv[3]) - 1, bad, time.time() - t0), flush=True)

# ---- third campaign: small meshes seen from far away (far_view_world), the regime of binary32 false accepts outside the
# leaves' exact boxes; worlds with faces thinner than 1.8 degrees (their nodes widen the search boxes for them: scene.hip
# face_slack_exponent; rtmi_scene_sliver_faces) are counted apart
if len(sys.argv) > 4:
    bad = bad_sliver = n_sliver = 0
    t0 = time.time()
    for seed in range(first, first + int(sys.argv[4])):
        fill, cam, h, w, spp, depth, what = far_view_world(seed)
        slivers = what["slivers"]
        n_sliver += slivers > 0
        if differs(fill, 500 + seed, h, w, spp, depth, False, cam, nan_ok=True):
            if slivers:
                bad_sliver += 1
            else:
                bad += 1
            print("FAR MISMATCH seed", seed, h, w, spp, depth, what, flush=True)
    print("far-view seeds %d..%d: %d mismatches in worlds without sliver faces, %d in the %d worlds with them, %.1fs" %
          (first, first + int(sys.argv[4]) - 1, bad, bad_sliver, n_sliver, time.time() - t0), flush=True)
