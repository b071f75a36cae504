"""The worlds of tests/pair_slab_worlds.py through the margin-check build, in both launches of
tests/test_gpu_pair_slab.py: every query is answered a second time by the plain, unculled scan (render_body.h,
RTMI_CHECK_MARGINS) and the disagreements are counted.  Run by tests/test_gpu_pair_slab.py in a process of its own.

usage: RTMI_LIB_PATH=ray-tracing-cuda_amd/lib/librtmi_check1.so python tests/pair_slab_check.py"""
import ctypes as C
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "ray-tracing-cuda_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import torch
import rtmi
import pair_slab_worlds as psw

assert "check" in os.path.basename(rtmi.LIB_PATH), "run with RTMI_LIB_PATH=.../librtmi_check1.so"
L = rtmi.lib()
out = {}
for world, (fill, seed, depth) in sorted(psw.WORLDS.items()):
    for launch, (spp, opts) in sorted(psw.LAUNCHES.items()):
        b = rtmi.SceneBuilder(seed)
        fill(b, 1.0)
        b.commit()
        R = rtmi.Renderer(b, psw.SIDE, psw.SIDE, spp, depth, True).init_rng()
        ro = rtmi.render_opts(**opts)
        R.render(opts=ro)
        torch.cuda.synchronize()
        c = (C.c_ulonglong * 40)()
        assert L.rtmi_debug_counters(b.h, c, None) == 0
        out["%s/%s" % (world, launch)] = {"rays": R.total_rays(), "re_done": int(c[33]), "disagreements": int(c[34]),
                                          "fast_path": R.mode(ro)["fast_path"]}
print(json.dumps(out))
