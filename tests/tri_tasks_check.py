"""The stacked sheets and the mixed list of tests/tri_tasks_worlds.py through the margin-check build: every query is
answered a second time by the plain, unculled scan (render_body.h, RTMI_CHECK_MARGINS) and the disagreements are counted.
Run by tests/test_gpu_tri_tasks.py in a process of its own.

usage: RTMI_LIB_PATH=ray-tracing-cuda_amd/lib/librtmi_check1.so python tests/tri_tasks_check.py"""
import ctypes as C
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "ray-tracing-cuda_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import torch
import rtmi
import tri_tasks_worlds as worlds

assert "check" in os.path.basename(rtmi.LIB_PATH), "run with RTMI_LIB_PATH=.../librtmi_check1.so"
L = rtmi.lib()
out = {}
cases = [("sheets_%d%s" % (n, "_light" if light else ""), worlds.sheets(n, light), side)
         for n in (2, 3, 4, 7) for light in (False, True) for side in (16,)]
cases += [("sheets_7_light_thin", worlds.sheets(7, True), 8), ("mixed_list", worlds.mixed_list(7), 16),
          ("mixed_list_thin", worlds.mixed_list(7), 8)]
for tag, fill, side in cases:
    b = rtmi.SceneBuilder(7)
    fill(b)
    b.commit()
    R = rtmi.Renderer(b, side, side, 4, 8).init_rng()
    R.render(opts=rtmi.render_opts(schedule=0))
    torch.cuda.synchronize()
    c = (C.c_ulonglong * 40)()
    assert L.rtmi_debug_counters(b.h, c, None) == 0
    out[tag] = {"rays": R.total_rays(), "re_done": int(c[33]), "disagreements": int(c[34])}
print(json.dumps(out))
