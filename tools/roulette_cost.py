#!/usr/bin/env python3
"""Cost and gain of Russian roulette: rtmi_trace, the compacted loop trace_steps(compact=True), that loop with a
Roulette(), and rtmi_trace_roulette on the same 2^20 camera rays, all timed with HIP events in ONE run; on the lamp rooms
also the loop with direct="mis", with and without roulette.

tools/trace_direct_cost.py's method.  The rays: 32 x 32 x 1024 camera rays of cornell_box at depths 10 and 50, bunny at
depth 10, lamp_room and close_lamp_room at depths 6 and 50.  The roulette is the default one (first_step 3, p_min 0.05).
Per row and candidate (trace, loop, loop_rr, fused, and on the lamp rooms mis, mis_rr):
  *_ms, *_spread_ms                         median of --reps runs after a warm-up, the candidates taken in turn within every
                                            repetition; (min, max) of the runs
  var_*, var_pixel_*                        the variance of a path's radiance summed over the channels (binary64), and the
                                            same within a pixel, averaged over the 1024 pixels
  time_x_variance_*, time_x_var_pixel_*     milliseconds times variance: what a frame of equal noise costs
  killed_share_*                            paths killed / paths (0 for a candidate without roulette)
  steps_per_path_*                          mean steps a path made (the loops); for rtmi_trace and the fused entry, which
                                            report queries (steps + 1 for a path the depth cut), queries_per_path_*
  *_faster_than_trace, *_faster_than_loop   the project's rule: every repetition below every repetition of the other, and
                                            the median gain at least three times the other's own spread (max - min); for
                                            mis_rr the other loop is mis
Every row is measured in a child process of its own under a time limit, the whole run under another; the first failure
ends the run.  Prints one JSON line; --out also writes it to a file.

    python tools/roulette_cost.py [--reps 7] [--spp 1024] [--out profiles/roulette_cost.json]
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
ROWS = (("cornell_box", 10), ("cornell_box", 50), ("bunny", 10), ("lamp_room", 6), ("lamp_room", 50), ("close_lamp_room", 6),
        ("close_lamp_room", 50))
LAMP_ROOMS = ("lamp_room", "close_lamp_room")


def measure(scene, depth, reps, spp):
    import torch
    import common
    import directlib
    import mislib
    import rtmi
    from rtmi import wavefront

    def timed(call, args):
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        out = call(*args)
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1), out

    custom = {"lamp_room": directlib.lamp_room, "close_lamp_room": mislib.close_lamp_room}
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
    rules = {}  # the Roulette of a candidate's last run: its counters

    def with_rule(name, **kw):
        def call(o_, d_, s_, l_):
            rules[name] = wavefront.Roulette()
            if "direct" in kw:
                kw["light_states"] = l_
            return b.trace_steps_roulette(o_, d_, s_, depth, rules[name], compact=True, **kw)
        return call
    cands = {"trace": lambda o_, d_, s_, l_: b.trace(o_, d_, s_, depth, count_rays=True),
             "loop": lambda o_, d_, s_, l_: b.trace_steps(o_, d_, s_, depth, compact=True),
             "loop_rr": with_rule("loop_rr"),
             "fused": lambda o_, d_, s_, l_: b.trace_roulette(o_, d_, s_, depth, count_rays=True)}
    if scene in LAMP_ROOMS:
        cands["mis"] = lambda o_, d_, s_, l_: b.trace_steps(o_, d_, s_, depth, compact=True, direct="mis", light_states=l_)
        cands["mis_rr"] = with_rule("mis_rr", direct="mis")
    times, outs = {k: [] for k in cands}, {}
    for k, call in cands.items():  # a warm-up each
        call(*fresh())
    for _ in range(reps):
        for k, call in cands.items():
            ms, outs[k] = timed(call, fresh())
            times[k].append(ms)
    res = {"depth": depth, "rays": n}
    med = {}
    for k, t in times.items():
        out = outs[k].check()
        rgb = out.rgb.double()
        med[k] = statistics.median(t)
        var = float(rgb.var(0, unbiased=True).sum().item())
        pix = float(rgb.reshape(32 * 32, spp, 3).var(1, unbiased=True).mean(0).sum().item())  # (the rays lie pixel by pixel)
        res["%s_ms" % k], res["%s_spread_ms" % k] = round(med[k], 3), [round(min(t), 3), round(max(t), 3)]
        res["var_%s" % k], res["var_pixel_%s" % k] = round(var, 5), round(pix, 5)
        res["time_x_variance_%s" % k], res["time_x_var_pixel_%s" % k] = round(med[k] * var, 3), round(med[k] * pix, 3)
        if k in ("trace", "fused"):
            res["queries_per_path_%s" % k] = round(float(out.rays.double().mean().item()), 4)
            killed = int(out.counts[1].item()) if k == "fused" else 0
        else:
            res["steps_per_path_%s" % k] = round(float(out.steps.double().mean().item()), 4)
            killed = int(rules[k].counts[1].item()) if k in rules and rules[k].counts is not None else 0
        res["killed_share_%s" % k] = round(killed / n, 5)

    def faster(a, than):  # the project's rule
        spread = max(times[than]) - min(times[than])
        return bool(max(times[a]) < min(times[than]) and med[than] - med[a] >= 3 * spread)
    for k in cands:
        if k != "trace":
            res["%s_over_trace_ms" % k] = round(med[k] / med["trace"], 4)
            res["%s_faster_than_trace" % k] = faster(k, "trace")
    for k, than in (("loop_rr", "loop"), ("fused", "loop"), ("mis_rr", "mis")):
        if k in cands:
            res["%s_over_%s_ms" % (k, than)] = round(med[k] / med[than], 4)
            res["%s_faster_than_loop" % k] = faster(k, than)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--spp", type=int, default=1024, help="camera rays per pixel of the 32 x 32 frame")
    ap.add_argument("--out", default=None)
    ap.add_argument("--row", default=None, help="scene:depth -- measure this one row in this process and print its JSON")
    ap.add_argument("--row-timeout", type=float, default=150.0, help="seconds a row's child process may take")
    ap.add_argument("--timeout", type=float, default=800.0, help="seconds the whole run may take")
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
    line = json.dumps({"roulette": res, "reps": a.reps, "spp": a.spp})
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
