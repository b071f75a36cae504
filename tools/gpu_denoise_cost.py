#!/usr/bin/env python3
"""Cost of rtmi_denoise beside the render it is meant to spare: one process, HIP events, the median of --reps after a
warm-up with min-max.

The Cornell box at --size^2 (1024), depth 10: a uniform 16-spp rtmi_render_features call makes the guides; the same frame's
rtmi_render_budget call with a uniform budget of 16 is timed; then rtmi_denoise with the default options for 1 .. 5
iterations.  A call is prepare + its passes, so pass k's time is the difference between the calls with k + 1 and k
iterations (the first figure, "prepare+pass0", holds the prepare kernel too).  Each pass's bytes are what it must move --
three 16-byte records in per pixel and two out (the last pass: the albedo in, the caller's float3 out) -- and the rate is
those bytes over the time, beside the 6.3 TB/s a copy achieves on an MI355X.

Gate: the whole denoise costs less than the 16-spp render.  Writes profiles/denoise_cost.json and prints it.

    python tools/gpu_denoise_cost.py [--reps 7] [--size 1024] [--out profiles/denoise_cost.json]
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "ray-tracing-cuda_amd"), os.path.join(ROOT, "tests")]

HBM_ACHIEVABLE_GBS = 6300.0  # a float4 copy on an MI355X


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--size", type=int, default=1024)
    ap.add_argument("--spp", type=int, default=16)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "denoise_cost.json"))
    a = ap.parse_args()
    import torch
    import rtmi
    import common

    scene, depth, n = "cornell_box", 10, a.size * a.size
    b = common.build_scene(rtmi.SceneBuilder(common.scene_seed(scene)), scene, 1.0).commit()
    R = rtmi.Renderer(b, a.size, a.size, a.spp, depth, post=False).init_rng()
    R._budget_buffers()
    R._feature_buffers()
    first = R.states.clone()
    budget = torch.full((R.items,), a.spp, dtype=torch.int32, device="cuda")

    def timed(fn, before=None):
        ms = []
        for rep in range(a.reps + 1):  # (the first is the warm-up)
            if before:
                before()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            torch.cuda.synchronize()
            if rep:
                ms.append(e0.elapsed_time(e1))
        return {"median_ms": round(statistics.median(ms), 4), "min_ms": round(min(ms), 4), "max_ms": round(max(ms), 4)}

    def fresh():
        R.states.copy_(first)
        for t in (R.sum, R.sq, R.samples, R.budget_rays, R.albedo, R.normal, R.depth, R.coverage):
            t.zero_()

    out = {"scene": scene, "size": a.size, "depth": depth, "spp": a.spp, "reps": a.reps,
           "defaults": dict(rtmi.DENOISE_DEFAULTS), "hbm_achievable_GBs": HBM_ACHIEVABLE_GBS}
    out["render_budget_%dspp" % a.spp] = timed(lambda: R.render_budget(budget, count_rays=False), fresh)
    fresh()
    R.render_budget(budget, count_rays=False, features=True)  # the guides
    buf = R.denoise_inputs()
    scratch_free = torch.empty((n, 3), dtype=torch.float32, device="cuda")
    iters = rtmi.DENOISE_DEFAULTS["iterations"]
    calls = [timed(lambda k=k: rtmi.denoise(**buf, out=scratch_free, iterations=k)) for k in range(1, iters + 1)]
    out["denoise_by_iterations"] = calls
    out["denoise"] = calls[-1]
    passes, prev = [], 0.0
    for k, c in enumerate(calls):
        ms = c["median_ms"] - prev
        prev = c["median_ms"]
        # pass k in a call of k + 1 iterations is its last: 3 records and the albedo in, a float3 out; the call of one
        # iteration also holds the prepare kernel: colour, variance, albedo, normal (12 B each), depth, alpha in, 3 records out
        moved = n * (48 + 12 + 12) + (n * (48 + 8 + 48) if k == 0 else 0)
        passes.append({"what": "prepare+pass0" if k == 0 else "pass%d" % k, "step": 1 << k, "taps": "lds" if (1 << k) <= 2 else "global",
                       "ms": round(ms, 4), "bytes": moved, "GBs": round(moved / (ms * 1e-3) / 1e9, 1) if ms > 0 else None})
    out["passes"] = passes
    # the whole call: prepare, iters - 1 intermediate passes (3 records in, 2 out), the last pass
    total_bytes = n * (48 + 8 + 48) + (iters - 1) * n * 80 + n * (48 + 12 + 12)
    out["denoise_bytes"] = total_bytes
    out["denoise_GBs"] = round(total_bytes / (calls[-1]["median_ms"] * 1e-3) / 1e9, 1)
    render = out["render_budget_%dspp" % a.spp]["median_ms"]
    out["denoise_over_render"] = round(calls[-1]["median_ms"] / render, 5)
    out["gate_denoise_cheaper_than_render"] = calls[-1]["median_ms"] < render
    line = json.dumps(out)
    print(line)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as fh:
        fh.write(json.dumps(out, indent=1) + "\n")
    if not out["gate_denoise_cheaper_than_render"]:
        sys.exit("gate missed: the denoise costs more than the %d-spp render" % a.spp)


if __name__ == "__main__":
    main()
