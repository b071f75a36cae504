#!/usr/bin/env python3
"""Cost of the first-hit feature buffers: a uniform-budget rtmi_render_budget call against the same call through
rtmi_render_features with all four buffers, timed with HIP events (median of --reps after a warm-up, and the spread).

cornell box at depth 50 and the bunny stand-in mesh (bench.py's C3 scene) at depth 10, --size^2 x --spp.  With
RTMI_LIB_PATH set to another build of the library (tools/ab_build.sh) that has no rtmi_render_features, only the plain
call is timed: the parent-to-this-commit comparison of kernels that did not change.  Prints one JSON line.

    python tools/gpu_feature_cost.py [--reps 7] [--size 1024] [--spp 64]
"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "ray-tracing-cuda_amd"), os.path.join(ROOT, "tests")]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--size", type=int, default=1024)
    ap.add_argument("--spp", type=int, default=64)
    a = ap.parse_args()
    import torch
    import rtmi
    has_features = hasattr(C.CDLL(rtmi.LIB_PATH), "rtmi_render_features")
    if not has_features:  # an older build: bind what it has
        rtmi.SYMBOLS[:] = [s for s in rtmi.SYMBOLS if s[0] not in ("rtmi_render_features", "rtmi_resolve_features")]
    import bench
    import common

    out = {"lib": os.path.basename(rtmi.LIB_PATH), "reps": a.reps, "size": a.size, "spp": a.spp}
    for scene, depth in (("cornell_box", 50), ("bunny", 10)):
        b = bench.build_scene(rtmi.SceneBuilder(common.scene_seed(scene)), scene, 1.0).commit()
        R = rtmi.Renderer(b, a.size, a.size, a.spp, depth, post=False).init_rng()
        R._budget_buffers()
        R._feature_buffers()
        first = R.states.clone()
        budget = torch.full((R.items,), a.spp, dtype=torch.int32, device="cuda")

        def timed(features):
            ms = []
            for rep in range(a.reps + 1):  # (the first is the warm-up)
                R.states.copy_(first)
                for t in (R.sum, R.sq, R.samples, R.budget_rays, R.albedo, R.normal, R.depth, R.coverage):
                    t.zero_()
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                R.render_budget(budget, count_rays=False, features=features)
                e1.record()
                torch.cuda.synchronize()
                if rep:
                    ms.append(e0.elapsed_time(e1))
            R.check()
            return {"median_ms": round(statistics.median(ms), 3), "min_ms": round(min(ms), 3), "max_ms": round(max(ms), 3)}

        row = {"depth": depth, "budget": timed(False)}
        row["queries"] = int(R.d_work[1].item())
        if has_features:
            row["budget_again"] = timed(False)  # (the same call once more: the run-to-run spread)
            row["features"] = timed(True)
            row["features_over_budget"] = round(row["features"]["median_ms"] / row["budget"]["median_ms"], 4)
        out[scene] = row
    print(json.dumps(out))


if __name__ == "__main__":
    main()
