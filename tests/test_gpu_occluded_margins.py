"""rtmi_occluded's culls, bounded by t_max, checked on every ray.

The occlusion kernel seeds the culled list scan, the grouped sphere scan and the mesh search with t_max instead of
+inf, so their padded bounds and time fudges now prune at the caller's bound.  `librtmi_check1.so` (-DRTMI_CHECK_MARGINS)
answers every ray a second time with the unculled engine from +inf (meshes: the reference's own tree walk), then the
filter, through rtmi_occluded_check_counts, which exists only in that build.  The adversarial families of
test_gpu_intersect_margins.py -- far origins, grazing sheets, needle meshes, needle lists, far sphere clouds -- are
run with a short and a long t_max around each ray's closest hit.  A diagnostic build, so it runs in a process of its
own (this file, run as a script, with RTMI_LIB_PATH pointing at it)."""
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHECK_LIB = os.path.join(ROOT, "ray-tracing-cuda_amd", "lib", "librtmi_check1.so")
SEEDS = 8      # worlds per family
RAYS = 4096    # query rays per world
T_MAX = ("short", "long")


@pytest.mark.gpu
def test_every_occlusion_answer_agrees_with_the_unculled_one():
    assert os.path.exists(CHECK_LIB), "librtmi_check1.so missing: run __graft_entry__.build() (make -C csrc check1)"
    env = dict(os.environ, RTMI_LIB_PATH=CHECK_LIB)
    r = subprocess.run([sys.executable, os.path.abspath(__file__)], env=env, cwd=ROOT, stdout=subprocess.PIPE,
                       stderr=subprocess.PIPE, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-4000:]
    out = json.loads(r.stdout[r.stdout.index("{"):])
    assert set(out) == {"%s/%s" % (f, s) for f in ("far_views", "grazing_views", "needles", "needle_lists",
                                                    "far_sphere_clouds") for s in T_MAX}, sorted(out)
    for tag, v in out.items():
        assert v["worlds"] == SEEDS, (tag, v)
        assert v["re_done"] == v["rays"] > 0, (tag, v)  # every ray was answered twice
        assert v["disagreements"] == 0, (tag, v)
        assert v["abandoned"] == 0, (tag, v)
        if tag.endswith("/long"):
            assert v["occluded"] > 0, (tag, v)
        else:
            assert v["occluded"] < v["rays"], (tag, v)


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
    fn = L.rtmi_occluded_check_counts
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
        tot = {s: {"worlds": 0, "rays": 0, "re_done": 0, "disagreements": 0, "abandoned": 0, "occluded": 0}
               for s in T_MAX}
        for seed in range(SEEDS):
            b = rtmi.SceneBuilder(500 + seed)
            make(seed)(b)
            b.commit()
            rng = np.random.default_rng(seed)
            o, d = rays(b, rng)
            go, gd = torch.from_numpy(o).cuda(), torch.from_numpy(d).cuda()
            t = b.intersect(go, gd).check().t.cpu().numpy()  # closest hits (+inf: none)
            base = np.where(np.isfinite(t), t, np.float32(np.linalg.norm(d, axis=1).max() * 10)).astype(np.float32)
            for s in T_MAX:
                # short: mostly below the closest hit (every cull pruned hard, mostly clear); long: at or beyond it
                f = rng.uniform(0.3, 1.05, RAYS) if s == "short" else rng.uniform(1.0, 3.0, RAYS)
                tmax = torch.from_numpy((base * f).astype(np.float32)).cuda()
                occ = torch.empty((RAYS,), dtype=torch.uint8, device="cuda")
                words = torch.zeros(4, dtype=torch.int64, device="cuda")  # abandoned, fallback, re-done, disagreements
                rc = fn(b.h, RAYS, go.data_ptr(), gd.data_ptr(), tmax.data_ptr(), occ.data_ptr(), words.data_ptr(),
                        words.data_ptr() + 16, C.c_void_p(torch.cuda.current_stream().cuda_stream))
                assert rc == 0, L.rtmi_last_error()
                w = words.cpu().numpy()
                v = tot[s]
                v["worlds"] += 1
                v["rays"] += RAYS
                v["abandoned"] += int(w[0])
                v["re_done"] += int(w[2])
                v["disagreements"] += int(w[3])
                v["occluded"] += int(occ.sum().item())
        for s in T_MAX:
            out["%s/%s" % (tag, s)] = tot[s]
    print(json.dumps(out, indent=1))


if __name__ == "__main__":
    _campaign()
