#!/usr/bin/env python3
"""Cost of stepping the live paths only (rtmi_path_compact + rtmi_bounce_list) beside the plain rtmi_bounce loop, timed
with HIP events in ONE run.

The rays: the 1024^2 camera rays of sample 0 (Renderer.camera_rays), one per pixel, with the states the render would
trace them with.  Cornell box at depth 50, the bunny stand-in mesh (bench.py's C3 scene) at depth 10.  Per scene:
  plain_ms        SceneBuilder.trace_steps: depth rtmi_bounce steps over all n paths and the fold
  compact_ms      trace_steps(compact=True): every step an rtmi_bounce_list on the list rtmi_path_compact made of the last
  full_ms         trace_steps(compact="full"): the same with every list compacted from all n paths
  trace_ms        one rtmi_trace on the same rays and states; all three loops' radiance must equal its bit for bit
  bounce_ms / bounce_list_null_ms            one rtmi_bounce against one rtmi_bounce_list with a null list, fresh rays:
  dead_bounce_ms / dead_bounce_list_null_ms  ... and over rays that have all ended -- the cursor-free distribution alone
  compact_once_ms one rtmi_path_compact of all n fresh paths (three launches)
  stepped         the paths each step of the loops took
each the median of --reps runs after a warm-up, HIP events on one stream.  Every scene is measured in a child process of
its own under a time limit, the whole run under another; the first failure ends the run.  Prints one JSON line; --out
also writes it to a file.  Kernel times alone: run one scene under rocprofv3 --kernel-trace --stats
(`-- python tools/gpu_bounce_list_cost.py --scene cornell_box`).

    python tools/gpu_bounce_list_cost.py [--reps 7] [--size 1024] [--out profiles/bounce_list_cost.json]
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "ray-tracing-cuda_amd"), os.path.join(ROOT, "tests")]
SCENES = (("cornell_box", 50), ("bunny", 10))


def measure(scene, depth, reps, size):
    import torch
    sys.path.insert(0, ROOT)
    import bench  # the benchmark's scenes: bunny is its full stand-in mesh, as in C3
    import common
    import rtmi

    def median_ms(prepare, call):
        """prepare() -> arguments (untimed: fresh copies of what the call changes in place), call(*arguments) timed."""
        call(*prepare())  # (warm-up: code objects, LDS attributes)
        torch.cuda.synchronize()
        times, out = [], None
        for _ in range(reps):
            args = prepare()
            torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            out = call(*args)
            e1.record()
            torch.cuda.synchronize()
            times.append(e0.elapsed_time(e1))
        return statistics.median(times), out

    b = bench.build_scene(rtmi.SceneBuilder(common.scene_seed(scene)), scene, 1.0).commit()
    R = rtmi.Renderer(b, size, size, 1, depth, post=False)
    R.init_rng()
    o, d = R.camera_rays(0)
    st = R.states
    n = o.shape[0]
    fresh = lambda: (o.clone(), d.clone(), st.clone())
    ended = lambda: (o.clone(), torch.zeros_like(d), st.clone())
    trace_ms, tr = median_ms(fresh, lambda o_, d_, s_: b.trace(o_, d_, s_, depth, count_rays=True))
    tr.check()
    res = {"depth": depth, "rays": n, "trace_ms": round(trace_ms, 3), "queries": tr.total_rays()}
    stepped = {}
    for key, mode in (("plain", False), ("compact", True), ("full", "full")):
        ms, steps = median_ms(fresh, lambda o_, d_, s_: b.trace_steps(o_, d_, s_, depth, compact=mode))
        steps.check()
        assert torch.equal(tr.rgb.view(torch.int32), steps.rgb.view(torch.int32)), "the %s loop and rtmi_trace disagree" % key
        stepped[key] = [int(w[1].item()) for w in steps.works]
        assert sum(stepped[key]) + int(steps.alive.sum().item()) == tr.total_rays()
        res[key + "_ms"] = round(ms, 3)
    assert stepped["plain"] == stepped["compact"] == stepped["full"]
    res["stepped"] = stepped["plain"]
    res["compact_over_plain"] = round(res["compact_ms"] / res["plain_ms"], 3)
    res["full_over_plain"] = round(res["full_ms"] / res["plain_ms"], 3)
    for key, prep in (("", fresh), ("dead_", ended)):
        ms_b, bo = median_ms(prep, lambda o_, d_, s_: b.bounce(o_, d_, s_))
        ms_l, bl = median_ms(prep, lambda o_, d_, s_: b.bounce_list(None, o_, d_, s_))
        bo.check(), bl.check()
        assert bo.stepped() == bl.stepped() == (n if key == "" else 0)
        res[key + "bounce_ms"], res[key + "bounce_list_null_ms"] = round(ms_b, 4), round(ms_l, 4)
    ms_c, paths = median_ms(fresh, lambda o_, d_, s_: rtmi.path_compact(o_, d_))
    assert paths.n() == n
    res["compact_once_ms"] = round(ms_c, 4)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--size", type=int, default=1024)
    ap.add_argument("--out", default=None)
    ap.add_argument("--scene", default=None, help="measure this one scene in this process and print its JSON")
    ap.add_argument("--scene-timeout", type=float, default=240.0, help="seconds a scene's child process may take")
    ap.add_argument("--timeout", type=float, default=420.0, help="seconds the whole run may take")
    a = ap.parse_args()
    if a.scene:
        depth = dict(SCENES)[a.scene]
        print(json.dumps({a.scene: measure(a.scene, depth, a.reps, a.size)}))
        return 0
    res, deadline = {}, time.monotonic() + a.timeout
    for scene, _ in SCENES:
        left = deadline - time.monotonic()
        if left <= 0:
            print("the run's time limit is used up before %s" % scene, file=sys.stderr)
            return 1
        cmd = [sys.executable, os.path.abspath(__file__), "--scene", scene, "--reps", str(a.reps), "--size", str(a.size)]
        try:
            r = subprocess.run(cmd, stdout=subprocess.PIPE, text=True, timeout=min(a.scene_timeout, left))
        except subprocess.TimeoutExpired:
            print("%s ran into its time limit: nothing more is started" % scene, file=sys.stderr)
            return 1
        if r.returncode != 0:
            print("%s failed (%d): nothing more is started" % (scene, r.returncode), file=sys.stderr)
            return 1
        res.update(json.loads(r.stdout.strip().splitlines()[-1]))
    line = json.dumps({"bounce_list": res, "reps": a.reps, "size": a.size})
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
