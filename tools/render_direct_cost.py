#!/usr/bin/env python3
"""Cost and gain of rtmi_render_direct: one frame of 1024 x 1024 pixels at 8 samples each, rendered three ways and timed
with HIP events in ONE run:
  (a) direct   Renderer.render_direct(budget): one launch, next-event estimation inside the budget render
  (b) loop     Renderer.render_rays(budget, direct="fused"): the parent's way to the very same sums -- per sample index
               rtmi_camera_rays, rtmi_trace_direct, rtmi_sample_add, behind one read-back of the largest budget
  (c) plain    Renderer.render_budget(budget): the budget render without direct light

tools/trace_direct_cost.py's method.  The rows: cornell_box and bunny at depth 10, lamp_room, close_lamp_room, bulb_room and
small_bulb_room (sphere lights on) at depth 6.  Per row:
  direct_ms, loop_ms, plain_ms              medians of --reps runs after a warm-up, the candidates taken in turn within every
                                            repetition, each on freshly seeded states and zeroed sums; a run ends with the
                                            renderer's check(); *_spread_ms is (min, max) of the runs
  direct_over_loop_ms, direct_over_plain_ms the ratios of the medians
  faster_than_loop                          the project's rule: every direct repetition below every loop repetition, and the
                                            median gain at least three times the loop's own spread (max - min)
  var_pixel_direct, var_pixel_plain         the unbiased variance of a pixel's samples from its sum and second moment, summed
                                            over the channels and averaged over the pixels (binary64)
  time_x_var_pixel_*                        milliseconds times that variance: what a frame of equal within-pixel noise costs;
                                            reported, not gated
  same_sums                                 (a) and (b) left the same sum, moment, sample count, ray count and states, bit for bit
Every row is measured in a child process of its own under a time limit, the whole run under another; the first failure
ends the run.  Prints one JSON line; --out also writes it to a file.

    python tools/render_direct_cost.py [--reps 7] [--size 1024] [--spp 8] [--out profiles/render_direct_cost.json]
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
ROWS = (("cornell_box", 10), ("bunny", 10), ("lamp_room", 6), ("close_lamp_room", 6), ("bulb_room", 6), ("small_bulb_room", 6))


def measure(scene, depth, reps, size, spp):
    import torch
    import common
    import directlib
    import mislib
    import rtmi
    import spherelightlib as sl

    custom = {"lamp_room": directlib.lamp_room, "close_lamp_room": mislib.close_lamp_room,
              "bulb_room": sl.with_kinds(sl.bulb_room), "small_bulb_room": sl.with_kinds(sl.small_bulb_room)}
    if scene in custom:
        b = directlib.build_custom(custom[scene])[0]
    else:
        b = common.build_scene(rtmi.SceneBuilder(common.scene_seed(scene)), scene, 1.0).commit()
    R = {k: rtmi.Renderer(b, size, size, spp, max_depth=depth, post=False) for k in ("direct", "loop", "plain")}
    budget = torch.full((R["direct"].items,), spp, dtype=torch.int32, device=R["direct"].device)
    cands = {"direct": lambda r: r.render_direct(budget).check(),
             "loop": lambda r: r.render_rays(budget, direct="fused").check(),
             "plain": lambda r: r.render_budget(budget).check()}

    def timed(k):
        r = R[k]
        r.init_rng().new_frame()  # fresh states, zeroed sums: every run renders the same frame
        r.light_states = None     # (seeded again on first use)
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        cands[k](r)
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1)

    times = {k: [] for k in cands}
    for k in cands:  # a warm-up each
        timed(k)
    for _ in range(reps):
        for k in cands:
            times[k].append(timed(k))

    def var_pixel(r):
        n = r.samples.double()[:, None]
        s, q = r.sum.double(), r.sq.double()
        live = (n > 1).squeeze(1)
        v = ((q - s * s / n.clamp(min=1)) / (n - 1).clamp(min=1))[live]
        return float(v.mean(0).sum().item())

    res = {"depth": depth, "pixels": size * size, "spp": spp, "lights": int(len(b.lights()))}
    med = {k: statistics.median(t) for k, t in times.items()}
    for k, t in times.items():
        res["%s_ms" % k], res["%s_spread_ms" % k] = round(med[k], 3), [round(min(t), 3), round(max(t), 3)]
    res["direct_over_loop_ms"] = round(med["direct"] / med["loop"], 4)
    res["direct_over_plain_ms"] = round(med["direct"] / med["plain"], 4)
    res["loop_over_plain_ms"] = round(med["loop"] / med["plain"], 4)
    spread = max(times["loop"]) - min(times["loop"])
    res["faster_than_loop"] = bool(max(times["direct"]) < min(times["loop"]) and med["loop"] - med["direct"] >= 3 * spread)
    var = {"direct": var_pixel(R["direct"]), "plain": var_pixel(R["plain"])}
    for k in ("direct", "plain"):
        res["var_pixel_%s" % k], res["time_x_var_pixel_%s" % k] = round(var[k], 5), round(med[k] * var[k], 3)
    res["time_x_var_pixel_loop"] = round(med["loop"] * var["direct"], 3)  # (the loop's samples are the direct render's)
    res["var_pixel_direct_over_plain"] = round(var["direct"] / var["plain"], 4) if var["plain"] > 0 else None
    res["time_x_var_pixel_direct_over_plain"] = (round(med["direct"] * var["direct"] / (med["plain"] * var["plain"]), 3)
                                                 if var["plain"] > 0 else None)
    a, l = R["direct"], R["loop"]
    res["same_sums"] = bool(all(torch.equal(getattr(a, f).view(torch.int32), getattr(l, f).view(torch.int32))
                                for f in ("sum", "sq", "samples", "budget_rays", "states", "light_states")))
    res["direct_counts"] = [int(x) for x in a.direct_counts.tolist()]  # (over the warm-up and the repetitions)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--size", type=int, default=1024, help="the frame is size x size pixels")
    ap.add_argument("--spp", type=int, default=8)
    ap.add_argument("--out", default=None)
    ap.add_argument("--row", default=None, help="scene:depth -- measure this one row in this process and print its JSON")
    ap.add_argument("--row-timeout", type=float, default=150.0, help="seconds a row's child process may take")
    ap.add_argument("--timeout", type=float, default=540.0, help="seconds the whole run may take")
    a = ap.parse_args()
    if a.row:
        scene, depth = a.row.split(":")
        print(json.dumps({"%s_d%s" % (scene, depth): measure(scene, int(depth), a.reps, a.size, a.spp)}))
        return 0
    res, deadline = {}, time.monotonic() + a.timeout
    for scene, depth in ROWS:
        left = deadline - time.monotonic()
        if left <= 0:
            print("the run's time limit is used up before %s" % scene, file=sys.stderr)
            return 1
        cmd = [sys.executable, os.path.abspath(__file__), "--row", "%s:%d" % (scene, depth), "--reps", str(a.reps),
               "--size", str(a.size), "--spp", str(a.spp)]
        try:
            r = subprocess.run(cmd, stdout=subprocess.PIPE, text=True, timeout=min(a.row_timeout, left))
        except subprocess.TimeoutExpired:
            print("%s ran into its time limit: nothing more is started" % scene, file=sys.stderr)
            return 1
        if r.returncode != 0:
            print("%s failed (%d): nothing more is started" % (scene, r.returncode), file=sys.stderr)
            return 1
        res.update(json.loads(r.stdout.strip().splitlines()[-1]))
    line = json.dumps({"render_direct": res, "reps": a.reps, "size": a.size, "spp": a.spp})
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
