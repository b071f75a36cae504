"""rtmi_intersect's culls, checked on every query.

The query kernel answers through the render's closest-hit engine, whose culled list scan, grouped sphere scan and
mesh search are exact only because padded bounds and distance slacks cover the binary32 tests' reach.
Caller-made rays can aim straight at that budget, so `librtmi_check1.so` (-DRTMI_CHECK_MARGINS: every query answered
a second time without any cull; meshes by the reference's own tree walk) is run on adversarial query batches -- far
origins, grazing sheets, needle meshes, needle lists, far sphere clouds (tests/worlds.py) -- through
rtmi_intersect_check_counts, which exists only in that build.  A diagnostic build, so it runs in a process of its own
(this file, run as a script, with RTMI_LIB_PATH pointing at it)."""
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHECK_LIB = os.path.join(ROOT, "ray-tracing-cuda_amd", "lib", "librtmi_check1.so")
SEEDS = 8      # worlds per family
RAYS = 4096    # query rays per world


@pytest.mark.gpu
def test_every_query_agrees_with_the_unculled_answer():
    assert os.path.exists(CHECK_LIB), "librtmi_check1.so missing: run __graft_entry__.build() (make -C csrc check1)"
    env = dict(os.environ, RTMI_LIB_PATH=CHECK_LIB)
    r = subprocess.run([sys.executable, os.path.abspath(__file__)], env=env, cwd=ROOT, stdout=subprocess.PIPE,
                       stderr=subprocess.PIPE, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-4000:]
    out = json.loads(r.stdout[r.stdout.index("{"):])
    assert set(out) == {"far_views", "grazing_views", "needles", "needle_lists", "far_sphere_clouds"}, sorted(out)
    for tag, v in out.items():
        assert v["worlds"] == SEEDS, (tag, v)
        assert v["re_done"] == v["rays"] > 0, (tag, v)  # every query was answered twice
        assert v["disagreements"] == 0, (tag, v)
        assert v["abandoned"] == 0, (tag, v)


def _campaign():
    import ctypes as C

    import numpy as np
    import torch

    sys.path.insert(0, os.path.join(ROOT, "ray-tracing-cuda_amd"))
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import rtmi
    import worlds as t3

    assert os.path.samefile(rtmi.LIB_PATH, CHECK_LIB), rtmi.LIB_PATH
    L = rtmi.lib()
    fn = L.rtmi_intersect_check_counts
    fn.restype = C.c_int
    fn.argtypes = [C.c_void_p, C.c_int64] + [C.c_void_p] * 7

    def rays(b, rng):
        """Camera rays through random points of the view, and the same rays started 1e3 view distances back."""
        cam = b.camera_get()
        pos, llc, hor, ver = (cam[i].astype(np.float32) for i in range(4))
        xy = rng.random((RAYS, 2)).astype(np.float32)
        d = (llc + xy[:, :1] * hor + xy[:, 1:] * ver - pos).astype(np.float32)
        o = np.repeat(pos[None], RAYS, 0)
        back = np.arange(RAYS) % 4 == 3
        o[back] = (o[back] - np.float32(1e3) * d[back]).astype(np.float32)
        return np.ascontiguousarray(o), np.ascontiguousarray(d)

    families = {
        "far_views": lambda s: (lambda f, cam: (lambda b: (cam(b), f(b))))(*t3.far_view_world(s)[:2]),
        "grazing_views": lambda s: t3.grazing_world(s)[0],
        "needles": lambda s: t3.needle_world(s)[0],
        "needle_lists": lambda s: t3.needle_list_world(s)[0],
        "far_sphere_clouds": lambda s: t3.far_sphere_cloud(s)[0],
    }
    out = {}
    for tag, make in families.items():
        tot = {"worlds": 0, "rays": 0, "re_done": 0, "disagreements": 0, "abandoned": 0}
        for seed in range(SEEDS):
            b = rtmi.SceneBuilder(500 + seed)
            make(seed)(b)
            b.commit()
            o, d = rays(b, np.random.default_rng(seed))
            go, gd = torch.from_numpy(o).cuda(), torch.from_numpy(d).cuda()
            hits = torch.empty((RAYS, 12), dtype=torch.int32, device="cuda")
            words = torch.zeros(3, dtype=torch.int64, device="cuda")  # abandoned, re-done, disagreements
            rc = fn(b.h, RAYS, go.data_ptr(), gd.data_ptr(), None, hits.data_ptr(), words.data_ptr(),
                    words.data_ptr() + 8, C.c_void_p(torch.cuda.current_stream().cuda_stream))
            assert rc == 0, L.rtmi_last_error()
            w = words.cpu().numpy()
            tot["worlds"] += 1
            tot["rays"] += RAYS
            tot["abandoned"] += int(w[0])
            tot["re_done"] += int(w[1])
            tot["disagreements"] += int(w[2])
        out[tag] = tot
    print(json.dumps(out, indent=1))


if __name__ == "__main__":
    _campaign()
