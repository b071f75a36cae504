#!/usr/bin/env python3
"""Cost and gain of rtmi_trace_direct: rtmi_trace, the loop trace_steps(compact=True, direct="mis") with its default
shadow query, and rtmi_trace_direct on the same 2^20 camera rays, all timed with HIP events in ONE run.

tools/sphere_lights_cost.py's method.  The rays: 32 x 32 x 1024 camera rays of the rows of profiles/direct_mis_cost.json
and profiles/sphere_lights_cost.json -- cornell_box at depths 10 and 50, bunny at depth 10, lamp_room, close_lamp_room,
bulb_room and small_bulb_room (sphere lights on) at depth 6.  Per row:
  trace_ms, loop_ms, fused_ms               medians of --reps runs after a warm-up, the candidates taken in turn within every
                                            repetition; *_spread_ms is (min, max) of the runs
  var_*, var_pixel_*                        the variance of a path's radiance summed over the channels (binary64), and the
                                            same within a pixel, averaged over the 1024 pixels
  time_x_variance_*, time_x_var_pixel_*     milliseconds times variance: what a frame of equal noise costs
  fused_over_loop_ms, fused_over_trace_ms   the ratios of the medians
  faster_than_loop                          the project's rule: every fused repetition below every loop repetition, and the
                                            median gain at least three times the loop's own spread (max - min)
  max_abs_fused_minus_loop                  the two radiances differ by the rounding order of one sum only
Every row is measured in a child process of its own under a time limit, the whole run under another; the first failure
ends the run.  Prints one JSON line; --out also writes it to a file.

    python tools/trace_direct_cost.py [--reps 7] [--spp 1024] [--out profiles/trace_direct_cost.json]
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
ROWS = (("cornell_box", 10), ("cornell_box", 50), ("bunny", 10), ("lamp_room", 6), ("close_lamp_room", 6), ("bulb_room", 6),
        ("small_bulb_room", 6))


def measure(scene, depth, reps, spp):
    import torch
    import common
    import directlib
    import mislib
    import rtmi
    import spherelightlib as sl

    def timed(call, args):
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        out = call(*args)
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1), out

    custom = {"lamp_room": directlib.lamp_room, "close_lamp_room": mislib.close_lamp_room,
              "bulb_room": sl.with_kinds(sl.bulb_room), "small_bulb_room": sl.with_kinds(sl.small_bulb_room)}
    if scene in custom:
        b, seed = directlib.build_custom(custom[scene])[0], directlib.LAMP_ROOM_SEED
    else:
        seed = common.scene_seed(scene)
        b = common.build_scene(rtmi.SceneBuilder(seed), scene, 1.0).commit()
    O, D = directlib.camera_rays(b, 32, 32, spp, 31)
    o, d = torch.from_numpy(O).cuda(), torch.from_numpy(D).cuda()
    n = o.shape[0]
    st, ls = rtmi.rng_states(seed, n), rtmi.rng_states(4242, n, first=n)
    fresh = lambda: (o.clone(), d.clone(), st.clone(), ls.clone())
    cands = {"trace": lambda o_, d_, s_, l_: b.trace(o_, d_, s_, depth),
             "loop": lambda o_, d_, s_, l_: b.trace_steps(o_, d_, s_, depth, compact=True, direct="mis", light_states=l_),
             "fused": lambda o_, d_, s_, l_: b.trace_direct(o_, d_, s_, l_, depth)}
    times, outs = {k: [] for k in cands}, {}
    for k, call in cands.items():  # a warm-up each
        call(*fresh())
    for _ in range(reps):
        for k, call in cands.items():
            ms, outs[k] = timed(call, fresh())
            times[k].append(ms)
    res = {"depth": depth, "rays": n, "lights": int(len(b.lights()))}
    var, pix, med = {}, {}, {}
    for k, t in times.items():
        rgb = outs[k].check().rgb.double()
        med[k] = statistics.median(t)
        var[k] = float(rgb.var(0, unbiased=True).sum().item())
        pix[k] = float(rgb.reshape(32 * 32, spp, 3).var(1, unbiased=True).mean(0).sum().item())  # (the rays lie pixel by pixel)
        res["%s_ms" % k], res["%s_spread_ms" % k] = round(med[k], 3), [round(min(t), 3), round(max(t), 3)]
        res["var_%s" % k], res["var_pixel_%s" % k] = round(var[k], 5), round(pix[k], 5)
        res["time_x_variance_%s" % k], res["time_x_var_pixel_%s" % k] = round(med[k] * var[k], 3), round(med[k] * pix[k], 3)
    for k in ("loop", "fused"):
        res["var_pixel_%s_over_trace" % k] = round(pix[k] / pix["trace"], 4)
        res["%s_over_trace_ms" % k] = round(med[k] / med["trace"], 3)
        res["time_x_var_pixel_%s_over_trace" % k] = round(med[k] * pix[k] / (med["trace"] * pix["trace"]), 3)
    res["fused_over_loop_ms"] = round(med["fused"] / med["loop"], 4)
    spread = max(times["loop"]) - min(times["loop"])
    res["faster_than_loop"] = bool(max(times["fused"]) < min(times["loop"]) and med["loop"] - med["fused"] >= 3 * spread)
    res["max_abs_fused_minus_loop"] = float((outs["fused"].rgb.double() - outs["loop"].rgb.double()).abs().max().item())
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--spp", type=int, default=1024, help="camera rays per pixel of the 32 x 32 frame")
    ap.add_argument("--out", default=None)
    ap.add_argument("--row", default=None, help="scene:depth -- measure this one row in this process and print its JSON")
    ap.add_argument("--row-timeout", type=float, default=150.0, help="seconds a row's child process may take")
    ap.add_argument("--timeout", type=float, default=600.0, help="seconds the whole run may take")
    a = ap.parse_args()
    if a.row:
        scene, depth = a.row.split(":")
        print(json.dumps({"%s_d%s" % (scene, depth): measure(scene, int(depth), a.reps, a.spp)}))
        return 0
    res, deadline = {}, time.monotonic() + a.timeout
    for scene, depth in ROWS:
        left = deadline - time.monotonic()
        if left <= 0:
            print("the run's time limit is used up before %s" % scene, file=sys.stderr)
            return 1
        cmd = [sys.executable, os.path.abspath(__file__), "--row", "%s:%d" % (scene, depth), "--reps", str(a.reps), "--spp", str(a.spp)]
        try:
            r = subprocess.run(cmd, stdout=subprocess.PIPE, text=True, timeout=min(a.row_timeout, left))
        except subprocess.TimeoutExpired:
            print("%s ran into its time limit: nothing more is started" % scene, file=sys.stderr)
            return 1
        if r.returncode != 0:
            print("%s failed (%d): nothing more is started" % (scene, r.returncode), file=sys.stderr)
            return 1
        res.update(json.loads(r.stdout.strip().splitlines()[-1]))
    line = json.dumps({"trace_direct": res, "reps": a.reps, "spp": a.spp})
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
