"""The ordered world of tests/min_fold_worlds.py and the sheets and mixed list of tests/tri_tasks_worlds.py through the
margin-check build, on the pinned kernels: every query is answered a second time by the plain, unculled scan, which folds
in list order (render_body.h, RTMI_CHECK_MARGINS), and the disagreements are counted.  Run by tests/test_gpu_min_fold.py in a
process of its own.

usage: RTMI_LIB_PATH=ray-tracing-cuda_amd/lib/librtmi_check1.so python tests/min_fold_check.py"""
import ctypes as C
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "ray-tracing-cuda_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import torch
import rtmi
import min_fold_worlds as mf
import tri_tasks_worlds as worlds

assert "check" in os.path.basename(rtmi.LIB_PATH), "run with RTMI_LIB_PATH=.../librtmi_check1.so"
L = rtmi.lib()
ONE_LAUNCH = dict(lane_stride=1, schedule=0)
cases = [("ordered/one_launch", mf.ordered_world, mf.SEED, mf.SIDE, mf.SPP, mf.DEPTH, ONE_LAUNCH),
         ("ordered/two_launches", mf.ordered_world, mf.SEED, 64, 64, mf.DEPTH,
          dict(lane_stride=1, schedule=2, plan=2, probe_spp=32))]  # (chains are planned from 64 samples on)
sheets = [("sheets_%d%s" % (n, "_light" if light else ""), worlds.sheets(n, light)) for n in (2, 3, 4, 7) for light in (False, True)]
sheets.append(("mixed_list", worlds.mixed_list(7)))
for tag, fill in sheets:
    # (eight samples: a frame of fewer has no priority table and with that no pinned kernel)
    cases += [(tag + "/16", fill, 7, 16, 8, 8, ONE_LAUNCH), (tag + "/thin", fill, 7, 8, 8, 8, ONE_LAUNCH)]
out = {}
for tag, fill, seed, side, spp, depth, opts in cases:
    b = rtmi.SceneBuilder(seed)
    fill(b)
    b.commit()
    R = rtmi.Renderer(b, side, side, spp, depth, True).init_rng()
    ro = rtmi.render_opts(**opts)
    R.render(opts=ro)
    torch.cuda.synchronize()
    c = (C.c_ulonglong * 40)()
    assert L.rtmi_debug_counters(b.h, c, None) == 0
    out[tag] = {"rays": R.total_rays(), "re_done": int(c[33]), "disagreements": int(c[34]),
                "ordered_tasks": int(c[mf.ORDERED_WORD]), "fast_path": R.mode(ro)["fast_path"]}
print(json.dumps(out))
