"""The worlds of tests/pair_rounds_worlds.py through the margin-check build, on the pinned kernels: every query is answered
a second time by the plain, unculled scan, which folds in list order (render_body.h, RTMI_CHECK_MARGINS), and the
disagreements are counted; and the build counts the pair rounds and the triangle rounds of the flushes' step (b) in
words 37 and 38 of rtmi_debug_counters, and in word 39 the tasks of the ordered kind that a pair round met (all three the
last launch's), which is how tests/test_gpu_pair_rounds.py knows that the regimes of the schedule were reached and that
such tasks arose inside pair rounds.  Run by that test in a process of its own.

usage: RTMI_LIB_PATH=ray-tracing-cuda_amd/lib/librtmi_check1.so python tests/pair_rounds_check.py"""
import ctypes as C
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "ray-tracing-cuda_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import torch
import rtmi
import pair_rounds_worlds as pw

assert "check" in os.path.basename(rtmi.LIB_PATH), "run with RTMI_LIB_PATH=.../librtmi_check1.so"
L = rtmi.lib()
ORDERED_WORD, PAIR_ROUNDS_WORD, TRI_ROUNDS_WORD, PAIR_FLAGS_WORD = 16, 37, 38, 39  # include/rtmi.h
LAUNCHES = {"queue": (8, dict(lane_stride=1)),
            "planned": (64, dict(lane_stride=1, schedule=2, plan=2, probe_spp=32))}  # (chains are planned from 64 samples on)
worlds = [("stack/2/%d" % j, pw.stack(2, j), 7, 8, 8) for j in (0, 1, 15, 16, 33, 64)]
worlds += [("stack/3/48", pw.stack(3, 48), 7, 8, 8), ("stack/5/64", pw.stack(5, 64), 7, 8, 8),
           ("stack/2/64/lone", pw.stack(2, 64, lone=True), 7, 8, 8), ("stack/3/33/metal", pw.stack(3, 33, metal=True), 7, 8, 8),
           ("ordered", pw.ordered_twice, pw.SEED, pw.SIDE, pw.DEPTH), ("cornell", pw.cornell, pw.CORNELL_SEED, 16, 50)]
out = {}
for tag, fill, seed, side, depth in worlds:
    b = rtmi.SceneBuilder(seed)
    fill(b)
    b.commit()
    for launch, (spp, opts) in LAUNCHES.items():
        R = rtmi.Renderer(b, side, side, spp, depth, True).init_rng()
        ro = rtmi.render_opts(fast_path=1, **opts)
        R.render(opts=ro)
        torch.cuda.synchronize()
        c = (C.c_ulonglong * 40)()
        assert L.rtmi_debug_counters(b.h, c, None) == 0
        out[tag + "/" + launch] = {"rays": R.total_rays(), "re_done": int(c[33]), "disagreements": int(c[34]),
                                   "ordered_tasks": int(c[ORDERED_WORD]), "pair_rounds": int(c[PAIR_ROUNDS_WORD]),
                                   "tri_rounds": int(c[TRI_ROUNDS_WORD]), "pair_flags": int(c[PAIR_FLAGS_WORD]), "fast_path": R.mode(ro)["fast_path"]}
print(json.dumps(out))
