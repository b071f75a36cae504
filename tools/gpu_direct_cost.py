#!/usr/bin/env python3
"""Cost and gain of next-event estimation in the wavefront loop (rtmi_direct_sample, rtmi_occluded on its shadow rays,
rtmi_path_fold_direct) beside the compacted loop without it, timed with HIP events in ONE run.

The rays: the 1024^2 camera rays of sample 0 (Renderer.camera_rays), one per pixel, with the states the render would
trace them with.  Cornell box at depth 50 and at depth 10, the bunny stand-in mesh (bench.py's C3 scene) at depth 10, and
the lamp_room scene of tests/directlib.py (32 x 32 x 512 rays, depth 6).  Per scene:
  compact_ms      SceneBuilder.trace_steps(compact=True): the loop of rtmi_bounce_list steps and rtmi_path_fold
  direct_ms       trace_steps(compact=True, direct=True): the same loop with rtmi_direct_sample and rtmi_occluded after
                  every step and rtmi_path_fold_direct at the end
  sample_ms       one rtmi_direct_sample over all n paths after their first step (n = 2^20 at the default size)
  shadow_ms       one rtmi_occluded of the shadow rays it made
  sampled, dropped  that call's two counters
  var_plain, var_direct   the variance of a path's radiance, summed over the channels, of both loops (binary64)
  time_x_variance_plain / _direct   the loop's milliseconds times that variance: what a frame of equal noise costs
each time the median of --reps runs after a warm-up, HIP events on one stream.  Every scene is measured in a child process
of its own under a time limit, the whole run under another; the first failure ends the run.  Prints one JSON line; --out
also writes it to a file.

    python tools/gpu_direct_cost.py [--reps 7] [--size 1024] [--out profiles/direct_cost.json]
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
SCENES = (("cornell_box", 50), ("cornell_box_d10", 10), ("bunny", 10), ("lamp_room", 6))


def measure(scene, depth, reps, size):
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
        for _ in range(reps):
            args = prepare()
            torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            out = call(*args)
            e1.record()
            torch.cuda.synchronize()
            times.append(e0.elapsed_time(e1))
        return statistics.median(times), out

    if scene == "lamp_room":
        import directlib
        b, _ = directlib.build_custom(directlib.lamp_room)
        O, D = directlib.camera_rays(b, 32, 32, 512, 31)
        o, d = torch.from_numpy(O).cuda(), torch.from_numpy(D).cuda()
        st = rtmi.rng_states(directlib.LAMP_ROOM_SEED, o.shape[0])
    else:
        name = scene.split("_d")[0]
        b = bench.build_scene(rtmi.SceneBuilder(common.scene_seed(name)), name, 1.0).commit()
        R = rtmi.Renderer(b, size, size, 1, depth, post=False)
        R.init_rng()
        o, d = R.camera_rays(0)
        st = R.states
    n = o.shape[0]
    ls = rtmi.rng_states(4242, n, first=n)
    fresh = lambda: (o.clone(), d.clone(), st.clone(), ls.clone())
    res = {"depth": depth, "rays": n, "lights": int(len(b.lights()))}
    ms_p, plain = median_ms(fresh, lambda o_, d_, s_, l_: b.trace_steps(o_, d_, s_, depth, compact=True))
    ms_d, direct = median_ms(fresh, lambda o_, d_, s_, l_: b.trace_steps(o_, d_, s_, depth, compact=True, direct=True, light_states=l_))
    plain.check(), direct.check()
    assert torch.equal(plain.steps, direct.steps), "the direct loop moved the paths"
    vp = float(plain.rgb.double().var(0, unbiased=True).sum().item())
    vd = float(direct.rgb.double().var(0, unbiased=True).sum().item())
    res.update(compact_ms=round(ms_p, 3), direct_ms=round(ms_d, 3), direct_over_compact=round(ms_d / ms_p, 3),
               mean_plain=[round(float(x), 5) for x in plain.rgb.double().mean(0)],
               mean_direct=[round(float(x), 5) for x in direct.rgb.double().mean(0)],
               var_plain=round(vp, 6), var_direct=round(vd, 6), var_direct_over_plain=round(vd / vp, 4) if vp > 0 else None,
               time_x_variance_plain=round(ms_p * vp, 4), time_x_variance_direct=round(ms_d * vd, 4))
    # one step, then one rtmi_direct_sample over all n paths and the rtmi_occluded of its shadow rays
    o1, d1, s1 = o.clone(), d.clone(), st.clone()
    steps = torch.zeros((n,), dtype=torch.int32, device=o.device)
    r = b.bounce(o1, d1, s1, hits=True, steps=steps).check()
    e0 = r.emitted.clone()

    def prep():
        r.emitted.copy_(e0)
        return ls.clone(), torch.zeros((n,), dtype=torch.int32, device=o.device)
    ms_s, ds = median_ms(prep, lambda l_, f_: b.direct_sample(0, r, l_, f_))
    ms_o, oc = median_ms(lambda: (), lambda: b.occluded(ds.origins, ds.directions, ds.t_max))
    oc.check()
    res.update(sample_ms=round(ms_s, 4), shadow_ms=round(ms_o, 4), sampled=int(ds.counts[0].item()), dropped=int(ds.counts[1].item()),
               shadow_rays_per_s=round(int(ds.counts[0].item()) / (ms_o * 1e-3)) if ms_o > 0 else None,
               occluded=int(oc.mask.sum().item()))
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--size", type=int, default=1024)
    ap.add_argument("--out", default=None)
    ap.add_argument("--scene", default=None, help="measure this one scene in this process and print its JSON")
    ap.add_argument("--scene-timeout", type=float, default=200.0, help="seconds a scene's child process may take")
    ap.add_argument("--timeout", type=float, default=540.0, help="seconds the whole run may take")
    a = ap.parse_args()
    if a.scene:
        depth = dict(SCENES)[a.scene]
        print(json.dumps({a.scene: measure(a.scene, depth, a.reps, a.size)}))
        return 0
    res, deadline = {}, time.monotonic() + a.timeout
    for scene, _ in SCENES:
        left = deadline - time.monotonic()
        if left <= 0:
            print("the run's time limit is used up before %s" % scene, file=sys.stderr)
            return 1
        cmd = [sys.executable, os.path.abspath(__file__), "--scene", scene, "--reps", str(a.reps), "--size", str(a.size)]
        try:
            r = subprocess.run(cmd, stdout=subprocess.PIPE, text=True, timeout=min(a.scene_timeout, left))
        except subprocess.TimeoutExpired:
            print("%s ran into its time limit: nothing more is started" % scene, file=sys.stderr)
            return 1
        if r.returncode != 0:
            print("%s failed (%d): nothing more is started" % (scene, r.returncode), file=sys.stderr)
            return 1
        res.update(json.loads(r.stdout.strip().splitlines()[-1]))
    line = json.dumps({"direct": res, "reps": a.reps, "size": a.size})
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
