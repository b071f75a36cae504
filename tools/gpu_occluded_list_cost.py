#!/usr/bin/env python3
"""What the list form of the visibility query (rtmi_occluded_list) does to the wavefront loop with next-event estimation,
timed with HIP events in ONE run, on the rays and by the method of tools/gpu_direct_cost.py.

The rays: the 1024^2 camera rays of sample 0 (Renderer.camera_rays), one per pixel, with the states the render would
trace them with.  Cornell box at depth 50 and at depth 10, the bunny stand-in mesh (bench.py's C3 scene) at depth 10, and
the lamp_room scene of tests/directlib.py (32 x 32 x 512 rays, depth 6).  Per scene:
  all_ms          trace_steps(compact=True, direct=True, shadow="all"): rtmi_occluded over all n shadow rays after every
                  step -- the composition of unchanged entries the loop was before, and the baseline
  list_ms         the same loop with shadow="list": rtmi_occluded_list on the list the step used
  compact_ms      trace_steps(compact=True): the compacted loop without direct sampling
  all_times, list_times   the repetitions behind the two medians; all_spread_ms = max - min of all_times
  list_not_slower   list_ms <= all_ms + all_spread_ms: the rule that decides what shadow=None means (every scene must hold)
  step0 / step5   one rtmi_occluded over all n against one rtmi_occluded_list, on the shadow rays and the list of that
                  step of the loop, made by hand (listed: the list's count; sampled: the non-zero shadow directions)
each time the median of --reps runs after a warm-up, HIP events on one stream, the three loops interleaved repetition by
repetition.  Every scene is measured in a child process of its own under a time limit, the whole run under another; the
first failure ends the run.  Prints one JSON line; --out also writes it to a file.

    python tools/gpu_occluded_list_cost.py [--reps 7] [--size 1024] [--out profiles/occluded_list_cost.json]
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

    def timed(call, args):
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        out = call(*args)
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1), out

    def interleaved(prepare, calls):
        """Every call timed reps times after one warm-up each, the calls taking turns; prepare() -> fresh arguments
        (untimed).  Returns ({name: times}, {name: last result})."""
        for call in calls.values():
            call(*prepare())  # (warm-up: code objects, LDS attributes)
        times, outs = {k: [] for k in calls}, {}
        for _ in range(reps):
            for k, call in calls.items():
                ms, outs[k] = timed(call, prepare())
                times[k].append(ms)
        return times, outs

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
    loops = {
        "all": lambda o_, d_, s_, l_: b.trace_steps(o_, d_, s_, depth, compact=True, direct=True, light_states=l_, shadow="all"),
        "list": lambda o_, d_, s_, l_: b.trace_steps(o_, d_, s_, depth, compact=True, direct=True, light_states=l_, shadow="list"),
        "compact": lambda o_, d_, s_, l_: b.trace_steps(o_, d_, s_, depth, compact=True),
    }
    times, outs = interleaved(fresh, loops)
    for v in outs.values():
        v.check()
    assert torch.equal(outs["all"].rgb.view(torch.int32), outs["list"].rgb.view(torch.int32)), "the two loops differ"
    assert torch.equal(outs["all"].occluded, outs["list"].occluded), "the two occlusion stacks differ"
    ms = {k: statistics.median(v) for k, v in times.items()}
    spread = max(times["all"]) - min(times["all"])
    res.update(all_ms=round(ms["all"], 3), list_ms=round(ms["list"], 3), compact_ms=round(ms["compact"], 3),
               list_over_all=round(ms["list"] / ms["all"], 3), all_over_compact=round(ms["all"] / ms["compact"], 3),
               list_over_compact=round(ms["list"] / ms["compact"], 3),
               all_times=[round(t, 3) for t in times["all"]], list_times=[round(t, 3) for t in times["list"]],
               all_spread_ms=round(spread, 3), list_not_slower=bool(ms["list"] <= ms["all"] + spread))

    # the shadow rays and the list of step 0 and of step 5: the loop's steps by hand (what trace_steps enqueues)
    kept = {}
    o1, d1, s1, l1 = fresh()
    steps = torch.zeros((n,), dtype=torch.int32, device=o.device)
    flags = torch.zeros((n,), dtype=torch.int32, device=o.device)
    cur = rtmi.path_compact(o1, d1)
    for k in range(6):
        r = b.bounce_list(cur, o1, d1, s1, hits=True, steps=steps).check()
        ds = b.direct_sample(k, r, l1, flags, sample=k + 1 < depth)
        if k in (0, 5):
            kept[k] = (cur, ds.origins.clone(), ds.directions.clone(), ds.t_max.clone())
        cur = rtmi.path_compact(o1, d1, cur)
    for k, (paths, so, sd, tm) in sorted(kept.items()):
        out = torch.zeros((n,), dtype=torch.uint8, device=o.device)
        calls = {"all": lambda: b.occluded(so, sd, tm, out=out), "list": lambda: b.occluded_list(paths, so, sd, tm, out=out)}
        t, _ = interleaved(lambda: (), calls)
        a = b.occluded(so, sd, tm).check().raw
        l = b.occluded_list(paths, so, sd, tm).check().raw
        assert torch.equal(a, l), "step %d: the list form answers differently" % k
        res["step%d" % k] = {"listed": paths.n(), "sampled": int((sd != 0).any(1).sum().item()), "occluded": int(a.sum().item()),
                             "all_ms": round(statistics.median(t["all"]), 4), "list_ms": round(statistics.median(t["list"]), 4)}
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
    line = json.dumps({"occluded_list": res, "reps": a.reps, "size": a.size,
                       "list_not_slower_everywhere": all(v["list_not_slower"] for v in res.values())})
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
