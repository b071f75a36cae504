#!/usr/bin/env python3
"""Rate of rtmi_render_budget and cost of an adaptive render, timed with HIP events, beside rtmi_render.

1. A uniform budget of --spp samples on a --size^2 frame -- cornell box at depth 50, the bunny stand-in mesh (bench.py's
   C3 scene) at depth 10 -- against rtmi_render of the same frame at the same spp, post_process = 0, with its default
   scheduling and with schedule = 0 (the plain queue in image order, like for like).  Rates are closest-hit queries per
   second (the budget call's d_work[1], the render's total_rays()), the median of --reps calls.
2. Renderer.render_adaptive's loop on the cornell frame (--min / --step / --max / --tolerance): passes, total samples,
   wall time, and per pass the time in rtmi_render_budget and the time outside it (rtmi_budget_plan + the host's read
   of its totals); with --uniform, beside one rtmi_render of --max samples per pixel.

Prints one JSON line.  Kernel time alone: run it under rocprofv3 --kernel-trace --stats (budget_kernel<F> against
render_kernel<F>).

    python tools/gpu_adaptive_rate.py [--reps 7] [--size 1024] [--spp 16] [--uniform] [--skip-adaptive]
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "ray-tracing-cuda_amd"), os.path.join(ROOT, "tests")]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--size", type=int, default=1024)
    ap.add_argument("--spp", type=int, default=16)
    ap.add_argument("--min", type=int, default=16)
    ap.add_argument("--step", type=int, default=16)
    ap.add_argument("--max", type=int, default=1024)
    ap.add_argument("--tolerance", type=float, default=0.05)
    ap.add_argument("--floor", type=float, default=0.01)
    ap.add_argument("--uniform", action="store_true", help="also time one rtmi_render of --max samples per pixel")
    ap.add_argument("--skip-adaptive", action="store_true")
    a = ap.parse_args()
    import torch
    sys.path.insert(0, ROOT)
    import bench  # the benchmark's scenes: bunny is its full stand-in mesh, as in C3
    import common
    import rtmi

    def median_ms(call, reset):
        reset()
        call()  # (warm-up: code objects, LDS attributes)
        torch.cuda.synchronize()
        times = []
        for _ in range(a.reps):
            reset()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            call()
            e1.record()
            torch.cuda.synchronize()
            times.append(e0.elapsed_time(e1))
        return statistics.median(times)

    res = {}
    scenes = {}
    for scene, depth in (("cornell_box", 50), ("bunny", 10)):
        b = scenes[scene] = bench.build_scene(rtmi.SceneBuilder(common.scene_seed(scene)), scene, 1.0).commit()
        R = rtmi.Renderer(b, a.size, a.size, a.spp, depth, post=False)
        R.init_rng()
        R._budget_buffers()
        first = R.states.clone()
        budget = torch.full((R.items,), a.spp, dtype=torch.int32, device="cuda")

        def reset():  # every call renders the same samples
            R.states.copy_(first)
            for t in (R.sum, R.sq, R.samples, R.budget_rays):
                t.zero_()
        ms = median_ms(lambda: R.render_budget(budget, count_rays=False), reset)
        R.check()
        q = int(R.d_work[1].item())
        row = {"depth": depth, "budget_ms": round(ms, 3), "budget_queries": q, "budget_gqueries_per_s": round(q / ms / 1e6, 3)}
        for tag, opts in (("render", None), ("render_queue", rtmi.render_opts(schedule=0))):
            rms = median_ms(lambda: R.render(count_rays=False, opts=opts), lambda: R.states.copy_(first))
            R.check()
            rq = R.total_rays()
            row.update({tag + "_ms": round(rms, 3), tag + "_queries": rq, tag + "_gqueries_per_s": round(rq / rms / 1e6, 3),
                        "ratio_to_" + tag: round((q / ms) / (rq / rms), 3)})
        res[scene] = row
    out = {"uniform_budget": res, "reps": a.reps, "size": a.size, "spp": a.spp}

    if not a.skip_adaptive:
        depth, cap = 50, max(a.min, a.step)
        R = rtmi.Renderer(scenes["cornell_box"], a.size, a.size, cap, depth, post=False)
        R.init_rng()
        R._budget_buffers()
        R.plan(a.min, a.max, a.step, a.tolerance, a.floor)  # (warm-up of the small kernels)
        torch.cuda.synchronize()
        passes, total, render_ms, other_ms, active_px = 0, 0, [], [], []
        t0 = time.perf_counter()
        while True:
            e0, e1, e2 = (torch.cuda.Event(enable_timing=True) for _ in range(3))
            e0.record()
            budget, active, pass_total = R.plan(a.min, a.max, a.step, a.tolerance, a.floor)
            e1.record()
            if active == 0:
                break
            R.render_budget(budget, count_rays=False)
            e2.record()
            e2.synchronize()
            other_ms.append(e0.elapsed_time(e1)), render_ms.append(e1.elapsed_time(e2)), active_px.append(active)
            passes, total = passes + 1, total + pass_total
        R.check()
        tiles = R.resolve(post=True)
        torch.cuda.synchronize()
        wall = (time.perf_counter() - t0) * 1e3
        del tiles
        n = a.size * a.size
        ad = {"min": a.min, "step": a.step, "max": a.max, "tolerance": a.tolerance, "floor": a.floor, "passes": passes,
              "total_samples": total, "fraction_of_uniform": round(total / (n * a.max), 4), "wall_ms": round(wall, 2),
              "render_ms_sum": round(sum(render_ms), 2), "outside_render_ms_sum": round(sum(other_ms), 2),
              "outside_render_ms_per_pass": round(statistics.mean(other_ms), 4) if other_ms else 0.0,
              "first_pass_ms": round(render_ms[0], 3) if render_ms else 0.0,
              "last_passes": [{"active": p, "ms": round(m, 3)} for p, m in list(zip(active_px, render_ms))[-4:]],
              "pixels_at_max": int((R.samples == a.max).sum().item()), "pixels_at_min": int((R.samples == a.min).sum().item())}
        if a.uniform:
            U = rtmi.Renderer(scenes["cornell_box"], a.size, a.size, a.max, depth, post=True)
            U.init_rng()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            U.render(count_rays=False)
            e1.record()
            torch.cuda.synchronize()
            U.check()
            ad["uniform_render_ms"] = round(e0.elapsed_time(e1), 2)
        out["adaptive"] = ad
    print(json.dumps(out))


if __name__ == "__main__":
    main()
