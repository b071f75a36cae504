#!/usr/bin/env python3
"""Cost of rtmi_accumulate beside one pass of the filter it feeds: one process, HIP events, the median of --reps after a
warm-up with min-max.

At --size^2 (1024) on synthetic inputs -- the room of tests/test_accumulate_host.py seen from its home camera (the history)
and after its "slide" move (the frame) -- one rtmi_accumulate with a history is timed, and in the same process one
rtmi_denoise of 1 iteration on the same frame (not demodulated).

Gate: the accumulate median does not exceed the 1-iteration denoise median.  That follows from the bytes each must move,
it is not a chosen figure: accumulate moves about 168 B per pixel (44 in, 48 of history in when the taps are cached, 76
out), a 1-iteration denoise 176 B (prepare 104, the last pass 72) and has 25 taps of arithmetic to accumulate's 4.

Writes profiles/accumulate_cost.json and prints it.

    python tools/gpu_accumulate_cost.py [--reps 7] [--size 1024] [--out profiles/accumulate_cost.json]
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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "accumulate_cost.json"))
    a = ap.parse_args()
    import numpy as np
    import torch
    import rtmi
    from filter_rules import camera_of, room

    h = w = a.size
    n = h * w
    cam0, cam1 = camera_of("static", h, w), camera_of("slide", h, w)
    gpu = lambda d: {k: torch.from_numpy(np.ascontiguousarray(v)).cuda() for k, v in d.items()}
    first, frame = gpu(room(h, w, cam0)), gpu(room(h, w, cam1, seed=1))
    history = rtmi.accumulate(**first, camera=cam0)[3]
    out_history = torch.empty_like(history)
    torch.cuda.synchronize()

    def timed(fn):
        ms = []
        for rep in range(a.reps + 1):  # (the first is the warm-up)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            torch.cuda.synchronize()
            if rep:
                ms.append(e0.elapsed_time(e1))
        return {"median_ms": round(statistics.median(ms), 4), "min_ms": round(min(ms), 4), "max_ms": round(max(ms), 4)}

    out = {"size": a.size, "reps": a.reps, "move": "slide", "defaults": dict(rtmi.ACCUMULATE_DEFAULTS),
           "hbm_achievable_GBs": HBM_ACHIEVABLE_GBS}
    length = rtmi.accumulate(**frame, camera=cam1, history=history, prev_camera=cam0, out_history=out_history)[2]
    out["share_taken"] = round(float((length > 1).float().mean().item()), 4)
    # (rtmi.accumulate allocates its three outputs, rtmi.denoise its scratch, from torch's cache: both inside the timed region)
    out["accumulate"] = timed(lambda: rtmi.accumulate(**frame, camera=cam1, history=history, prev_camera=cam0,
                                                      out_history=out_history))
    den_out = torch.empty((h, w, 3), dtype=torch.float32, device="cuda")
    out["denoise_1_iteration"] = timed(lambda: rtmi.denoise(**frame, out=den_out, iterations=1))
    for what, moved in (("accumulate", n * (44 + 48 + 76)), ("denoise_1_iteration", n * (104 + 72))):
        out[what]["bytes"] = moved
        out[what]["GBs"] = round(moved / (out[what]["median_ms"] * 1e-3) / 1e9, 1)
    acc, den = out["accumulate"]["median_ms"], out["denoise_1_iteration"]["median_ms"]
    out["accumulate_over_denoise_1"] = round(acc / den, 5)
    out["gate_accumulate_not_above_one_denoise_pass"] = acc <= den
    print(json.dumps(out))
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as fh:
        fh.write(json.dumps(out, indent=1) + "\n")
    if not out["gate_accumulate_not_above_one_denoise_pass"]:
        sys.exit("gate missed: rtmi_accumulate (%.4f ms) costs more than a 1-iteration rtmi_denoise (%.4f ms)" % (acc, den))


if __name__ == "__main__":
    main()
