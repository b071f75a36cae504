#!/usr/bin/env python3
"""What the composed loop costs: Renderer.render_rays (rtmi_camera_rays, rtmi_trace, rtmi_sample_add once per sample)
against one rtmi_render_budget call at the same uniform budget, timed with HIP events on one stream (median of --reps
after a warm-up, and the spread).

cornell box and the bunny stand-in mesh (bench.py's C3 scene), both at depth 10, --size^2 x --spp.  Both calls start from
the same RNG states and zeroed buffers, and their sums are compared bit for bit after the last repetition.  Prints one
JSON line; --out also writes it to a file.

    python tools/gpu_camera_rays_cost.py [--reps 5] [--size 1024] [--spp 8] [--out profiles/camera_rays_cost.json]
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "ray-tracing-cuda_amd"), os.path.join(ROOT, "tests")]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--size", type=int, default=1024)
    ap.add_argument("--spp", type=int, default=8)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    import rtmi
    import bench
    import common

    out = {"reps": a.reps, "size": a.size, "spp": a.spp}
    for scene, depth in (("cornell_box", 10), ("bunny", 10)):
        b = bench.build_scene(rtmi.SceneBuilder(common.scene_seed(scene)), scene, 1.0).commit()
        R = rtmi.Renderer(b, a.size, a.size, a.spp, depth, post=False).init_rng()
        R._budget_buffers()
        first = R.states.clone()
        budget = torch.full((R.items,), a.spp, dtype=torch.int32, device="cuda")
        sums = {}

        def timed(composed):
            ms = []
            for rep in range(a.reps + 1):  # (the first is the warm-up)
                R.states.copy_(first)
                for t in (R.sum, R.sq, R.samples, R.budget_rays):
                    t.zero_()
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                if composed:
                    R.render_rays(count_rays=False)  # (budget None: the frame's spp everywhere, no read-back before the loop)
                else:
                    R.render_budget(budget, count_rays=False)
                e1.record()
                torch.cuda.synchronize()
                if rep:
                    ms.append(e0.elapsed_time(e1))
            R.check()
            sums[composed] = R.sum.clone()
            return {"median_ms": round(statistics.median(ms), 3), "min_ms": round(min(ms), 3), "max_ms": round(max(ms), 3)}

        row = {"depth": depth, "render_budget": timed(False), "render_rays": timed(True)}
        row["render_rays_over_render_budget"] = round(row["render_rays"]["median_ms"] / row["render_budget"]["median_ms"], 4)
        row["sums_identical"] = bool(torch.equal(sums[False].view(torch.int32), sums[True].view(torch.int32)))
        out[scene] = row
    line = json.dumps(out)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
