#!/usr/bin/env python3
"""Cost and gain of multiple importance sampling for the lights (rtmi_direct_sample_mis) beside the compacted loop without
next-event estimation and the loop with rtmi_direct_sample, all three timed with HIP events in ONE run.

tools/gpu_direct_cost.py's rays and method with one more column and one more scene.  The rays: the 1024^2 camera rays of
sample 0 (Renderer.camera_rays) for the Cornell box at depth 50 and at depth 10 and the bunny stand-in mesh at depth 10;
32 x 32 x 512 rays at depth 6 for lamp_room (tests/directlib.py) and 32 x 32 x 1024 for close_lamp_room (tests/mislib.py:
the lamp 0.1 under the ceiling).  Per scene:
  compact_ms, direct_ms, mis_ms     SceneBuilder.trace_steps(compact=True) without direct sampling, with direct=True and
                                    with direct="mis"
  sample_ms, sample_mis_ms          one rtmi_direct_sample / one rtmi_direct_sample_mis over all n paths after their first
                                    step (the binding's allocations included; the carry is handed in)
  weigh_mis_ms                      one rtmi_direct_sample_mis with sample = 0 after the second step, on the flags and
                                    carry of the first: what the loop's last step costs
  sampled, weighed                  the counters of those calls
  var_plain, var_direct, var_mis    the variance of a path's radiance, summed over the channels (binary64)
  time_x_variance_*                 the loop's milliseconds times that variance: what a frame of equal noise costs
each time the median of --reps runs after a warm-up, HIP events on one stream.  Every scene is measured in a child process
of its own under a time limit, the whole run under another; the first failure ends the run.  Prints one JSON line; --out
also writes it to a file.

    python tools/gpu_direct_mis_cost.py [--reps 7] [--size 1024] [--out profiles/direct_mis_cost.json]
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
SCENES = (("cornell_box", 50), ("cornell_box_d10", 10), ("bunny", 10), ("lamp_room", 6), ("close_lamp_room", 6))


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

    if scene in ("lamp_room", "close_lamp_room"):
        import directlib
        import mislib
        b, _ = directlib.build_custom(directlib.lamp_room if scene == "lamp_room" else mislib.close_lamp_room)
        O, D = directlib.camera_rays(b, 32, 32, 512 if scene == "lamp_room" else 1024, 31)
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
    loops = {}
    for what, direct in (("plain", False), ("direct", True), ("mis", "mis")):
        ms, out = median_ms(fresh, lambda o_, d_, s_, l_: b.trace_steps(o_, d_, s_, depth, compact=True, direct=direct,
                                                                        light_states=l_ if direct else None))
        out.check()
        rgb = out.rgb.double()
        loops[what] = (ms, float(rgb.var(0, unbiased=True).sum().item()), [round(float(x), 5) for x in rgb.mean(0)], out.steps)
    assert torch.equal(loops["plain"][3], loops["direct"][3]) and torch.equal(loops["plain"][3], loops["mis"][3]), "a loop moved the paths"
    (ms_p, vp, mp, _), (ms_d, vd, md, _), (ms_m, vm, mm, _) = loops["plain"], loops["direct"], loops["mis"]
    res.update(compact_ms=round(ms_p, 3), direct_ms=round(ms_d, 3), mis_ms=round(ms_m, 3),
               direct_over_compact=round(ms_d / ms_p, 3), mis_over_compact=round(ms_m / ms_p, 3), mis_over_direct=round(ms_m / ms_d, 3),
               mean_plain=mp, mean_direct=md, mean_mis=mm, var_plain=round(vp, 6), var_direct=round(vd, 6), var_mis=round(vm, 6),
               var_direct_over_plain=round(vd / vp, 4) if vp > 0 else None, var_mis_over_plain=round(vm / vp, 4) if vp > 0 else None,
               var_mis_over_direct=round(vm / vd, 4) if vd > 0 else None,
               time_x_variance_plain=round(ms_p * vp, 4), time_x_variance_direct=round(ms_d * vd, 4),
               time_x_variance_mis=round(ms_m * vm, 4))
    # one step, then one call of each sampler over all n paths; a second step, then one weighing call
    o1, d1, s1 = o.clone(), d.clone(), st.clone()
    steps = torch.zeros((n,), dtype=torch.int32, device=o.device)
    r = b.bounce(o1, d1, s1, hits=True, steps=steps).check()
    e0 = r.emitted.clone()
    carry = torch.zeros((n, 4), dtype=torch.float32, device=o.device)

    def prep():
        r.emitted.copy_(e0)
        return ls.clone(), torch.zeros((n,), dtype=torch.int32, device=o.device)
    ms_s, ds = median_ms(prep, lambda l_, f_: b.direct_sample(0, r, l_, f_))
    ms_ms, dm = median_ms(prep, lambda l_, f_: b.direct_sample(0, r, l_, f_, mis=True, carry=carry))
    flags1 = dm.flags.clone()
    r2 = b.bounce(o1, d1, s1, hits=True, steps=steps).check()
    e1 = r2.emitted.clone()

    def prep2():
        r2.emitted.copy_(e1)
        return ls.clone(), flags1.clone()
    ms_w, dw = median_ms(prep2, lambda l_, f_: b.direct_sample(1, r2, l_, f_, sample=False, mis=True, carry=carry))
    res.update(sample_ms=round(ms_s, 4), sample_mis_ms=round(ms_ms, 4), weigh_mis_ms=round(ms_w, 4),
               sampled=int(ds.counts[0].item()), sampled_mis=int(dm.counts[0].item()), dropped=int(ds.counts[1].item()),
               weighed=int(dw.counts[1].item()))
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--size", type=int, default=1024)
    ap.add_argument("--out", default=None)
    ap.add_argument("--scene", default=None, help="measure this one scene in this process and print its JSON")
    ap.add_argument("--scene-timeout", type=float, default=150.0, help="seconds a scene's child process may take")
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
    line = json.dumps({"direct_mis": res, "reps": a.reps, "size": a.size})
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
