#!/usr/bin/env python3
"""Cost and gain of sphere table lights (rtmi_scene_light_kinds): rtmi_trace, the compacted loop without next-event
estimation, the loop with rtmi_direct_sample and the loop with rtmi_direct_sample_mis on rooms lit by emissive spheres,
all timed with HIP events in ONE run; and the direct="mis" loop on a scene without emissive spheres with and without the
option, where the kernels are the same and the two must agree within the repetitions' spread.

tools/gpu_direct_mis_cost.py's method.  The rays: 32 x 32 x 1024 camera rays (2^20) at depth 6 of bulb_room and
small_bulb_room (tests/spherelightlib.py) and of lamp_room (tests/directlib.py).  Per bulb scene:
  trace_ms, compact_ms, direct_ms, mis_ms   SceneBuilder.trace, and SceneBuilder.trace_steps(compact=True) without direct
                                            sampling, with direct=True and with direct="mis"
  var_*                                     the variance of a path's radiance, summed over the channels (binary64)
  var_pixel_*                               the same within a pixel (the variance among a pixel's samples, averaged over the
                                            1024 pixels): what is left of var_* without the picture's own contrast
  var_*_over_trace, time_x_variance_*       against rtmi_trace's, and the milliseconds times the variance: what a frame of
                                            equal noise costs
for lamp_room: mis_kinds1_ms, mis_kinds3_ms.  Each time is the median of --reps runs after a warm-up, the candidates taken
in turn within every repetition (so that a drift of the machine meets them all); *_spread_ms is (min, max) of the runs.
Every scene is measured in a child process of its own under a time limit, the whole run under another; the first failure
ends the run.  Prints one JSON line; --out also writes it to a file.

    python tools/sphere_lights_cost.py [--reps 7] [--spp 1024] [--out profiles/sphere_lights_cost.json]
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
SCENES = ("bulb_room", "small_bulb_room", "lamp_room")
DEPTH = 6


def measure(scene, reps, spp):
    import torch
    import directlib
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

    def in_turn(cands):
        """{name: (median ms, (min, max), last result)} of {name: (prepare, call)}: a warm-up each, then reps rounds that
        run every candidate once, in order."""
        times, outs = {k: [] for k in cands}, {}
        for k, (prepare, call) in cands.items():
            call(*prepare())
        for _ in range(reps):
            for k, (prepare, call) in cands.items():
                ms, outs[k] = timed(call, prepare())
                times[k].append(ms)
        return {k: (statistics.median(t), (min(t), max(t)), outs[k]) for k, t in times.items()}

    seed = directlib.LAMP_ROOM_SEED
    if scene == "lamp_room":
        builders = {"kinds1": directlib.build_custom(sl.with_kinds(directlib.lamp_room, False))[0],
                    "kinds3": directlib.build_custom(sl.with_kinds(directlib.lamp_room, True))[0]}
        b = builders["kinds1"]
    else:
        b = directlib.build_custom(sl.with_kinds(sl.bulb_room if scene == "bulb_room" else sl.small_bulb_room))[0]
    O, D = directlib.camera_rays(b, 32, 32, spp, 31)
    o, d = torch.from_numpy(O).cuda(), torch.from_numpy(D).cuda()
    n = o.shape[0]
    st, ls = rtmi.rng_states(seed, n), rtmi.rng_states(4242, n, first=n)
    fresh = lambda: (o.clone(), d.clone(), st.clone(), ls.clone())
    res = {"depth": DEPTH, "rays": n, "lights": int(len(b.lights())), "sphere_lights": int((b.lights()["kind"] == 2).sum())}

    def loop(bb, direct):
        return lambda o_, d_, s_, l_: bb.trace_steps(o_, d_, s_, DEPTH, compact=True, direct=direct, light_states=l_ if direct else None)

    if scene == "lamp_room":
        got = in_turn({k: (fresh, loop(bb, "mis")) for k, bb in builders.items()})
        assert torch.equal(got["kinds1"][2].check().rgb.view(torch.int32), got["kinds3"][2].check().rgb.view(torch.int32)), "the option moved a bit"
        for k, (ms, spread, _) in got.items():
            res["mis_%s_ms" % k], res["mis_%s_spread_ms" % k] = round(ms, 3), [round(x, 3) for x in spread]
        res["mis_kinds3_over_kinds1"] = round(got["kinds3"][0] / got["kinds1"][0], 4)
        return res
    got = in_turn({"trace": (fresh, lambda o_, d_, s_, l_: b.trace(o_, d_, s_, DEPTH)), "compact": (fresh, loop(b, False)),
                   "direct": (fresh, loop(b, True)), "mis": (fresh, loop(b, "mis"))})
    var, pix = {}, {}
    for k, (ms, spread, out) in got.items():
        rgb = out.check().rgb.double()
        var[k] = float(rgb.var(0, unbiased=True).sum().item())
        res["%s_ms" % k], res["%s_spread_ms" % k] = round(ms, 3), [round(x, 3) for x in spread]
        res["mean_%s" % k], res["var_%s" % k] = [round(float(x), 5) for x in rgb.mean(0)], round(var[k], 5)
        pix[k] = float(rgb.reshape(32 * 32, spp, 3).var(1, unbiased=True).mean(0).sum().item())  # (the rays lie pixel by pixel)
        res["var_pixel_%s" % k] = round(pix[k], 5)
    assert torch.equal(got["compact"][2].steps, got["direct"][2].steps) and torch.equal(got["compact"][2].steps, got["mis"][2].steps), "a loop moved the paths"
    for k in ("compact", "direct", "mis"):
        res["var_%s_over_trace" % k] = round(var[k] / var["trace"], 4)
        res["var_pixel_%s_over_trace" % k] = round(pix[k] / pix["trace"], 4)
        res["%s_over_trace_ms" % k] = round(got[k][0] / got["trace"][0], 3)
    for k in got:
        res["time_x_variance_%s" % k] = round(got[k][0] * var[k], 3)
        res["time_x_var_pixel_%s" % k] = round(got[k][0] * pix[k], 3)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--spp", type=int, default=1024, help="camera rays per pixel of the 32 x 32 frame")
    ap.add_argument("--out", default=None)
    ap.add_argument("--scene", default=None, help="measure this one scene in this process and print its JSON")
    ap.add_argument("--scene-timeout", type=float, default=150.0, help="seconds a scene's child process may take")
    ap.add_argument("--timeout", type=float, default=420.0, help="seconds the whole run may take")
    a = ap.parse_args()
    if a.scene:
        print(json.dumps({a.scene: measure(a.scene, a.reps, a.spp)}))
        return 0
    res, deadline = {}, time.monotonic() + a.timeout
    for scene in SCENES:
        left = deadline - time.monotonic()
        if left <= 0:
            print("the run's time limit is used up before %s" % scene, file=sys.stderr)
            return 1
        cmd = [sys.executable, os.path.abspath(__file__), "--scene", scene, "--reps", str(a.reps), "--spp", str(a.spp)]
        try:
            r = subprocess.run(cmd, stdout=subprocess.PIPE, text=True, timeout=min(a.scene_timeout, left))
        except subprocess.TimeoutExpired:
            print("%s ran into its time limit: nothing more is started" % scene, file=sys.stderr)
            return 1
        if r.returncode != 0:
            print("%s failed (%d): nothing more is started" % (scene, r.returncode), file=sys.stderr)
            return 1
        res.update(json.loads(r.stdout.strip().splitlines()[-1]))
    line = json.dumps({"sphere_lights": res, "reps": a.reps, "spp": a.spp})
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
