#!/usr/bin/env python3
"""Cost of rtmi_bounce (one step of the trace loop as a call), timed with HIP events, beside rtmi_trace and
rtmi_intersect on the same rays.

The rays: the 1024^2 camera rays of sample 0 (Renderer.camera_rays), one per pixel, with the states the render would
trace them with.  Cornell box at depth 50, the bunny stand-in mesh (bench.py's C3 scene) at depth 10.  Per scene:
  loop_ms       SceneBuilder.trace_steps: depth steps and the fold, as a caller runs it (its buffers included)
  trace_ms      one rtmi_trace call on the same rays and states
  bounce_ms     one rtmi_bounce on the fresh rays (no hit records), bounce_hits_ms with them
  intersect_ms  rtmi_intersect on the same rays: the same queries without shading and the extra traffic
  dead_step_ms  one rtmi_bounce over rays that have all ended: what a step pays to scan paths it skips
  stepped       the paths each step of the loop took
each the median of --reps runs after a warm-up.  Prints one JSON line; --out also writes it to a file.  Kernel times
alone: run it under rocprofv3 --kernel-trace --stats (bounce_kernel<F>, path_fold_kernel, trace_kernel<F>).

    python tools/gpu_bounce_rate.py [--reps 7] [--size 1024] [--out profiles/bounce_cost.json]
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "ray-tracing-cuda_amd"), os.path.join(ROOT, "tests")]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--size", type=int, default=1024)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
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
        for _ in range(a.reps):
            args = prepare()
            torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            out = call(*args)
            e1.record()
            torch.cuda.synchronize()
            times.append(e0.elapsed_time(e1))
        return statistics.median(times), out

    res = {}
    for scene, depth in (("cornell_box", 50), ("bunny", 10)):
        b = bench.build_scene(rtmi.SceneBuilder(common.scene_seed(scene)), scene, 1.0).commit()
        R = rtmi.Renderer(b, a.size, a.size, 1, depth, post=False)
        R.init_rng()
        o, d = R.camera_rays(0)
        st = R.states
        n = o.shape[0]
        fresh = lambda: (o.clone(), d.clone(), st.clone())
        loop_ms, steps = median_ms(fresh, lambda o_, d_, s_: b.trace_steps(o_, d_, s_, depth))
        steps.check()
        stepped = [int(w[1].item()) for w in steps.works]
        trace_ms, tr = median_ms(fresh, lambda o_, d_, s_: b.trace(o_, d_, s_, depth, count_rays=True))
        tr.check()
        assert torch.equal(tr.rgb.view(torch.int32), steps.rgb.view(torch.int32)), "the loop and rtmi_trace disagree"
        assert sum(stepped) + int(steps.alive.sum().item()) == tr.total_rays()
        bounce_ms, bo = median_ms(fresh, lambda o_, d_, s_: b.bounce(o_, d_, s_))
        bo.check()
        bounce_hits_ms, _ = median_ms(fresh, lambda o_, d_, s_: b.bounce(o_, d_, s_, hits=True))
        intersect_ms, hi = median_ms(fresh, lambda o_, d_, s_: b.intersect(o_, d_))
        hi.check()
        dead_ms, dead = median_ms(lambda: (o.clone(), torch.zeros_like(d), st.clone()), lambda o_, d_, s_: b.bounce(o_, d_, s_))
        assert dead.stepped() == 0
        res[scene] = {"depth": depth, "rays": n, "loop_ms": round(loop_ms, 3), "trace_ms": round(trace_ms, 3),
                      "loop_over_trace": round(loop_ms / trace_ms, 3), "bounce_ms": round(bounce_ms, 3),
                      "bounce_hits_ms": round(bounce_hits_ms, 3), "intersect_ms": round(intersect_ms, 3),
                      "bounce_over_intersect": round(bounce_ms / intersect_ms, 3), "dead_step_ms": round(dead_ms, 4),
                      "queries": tr.total_rays(), "stepped": stepped}
    line = json.dumps({"bounce": res, "reps": a.reps, "size": a.size})
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
