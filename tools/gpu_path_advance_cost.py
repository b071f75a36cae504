#!/usr/bin/env python3
"""Cost of a wavefront render that refills ended paths in place (rtmi_path_advance, Renderer.render_wavefront) beside the
per-sample loop it replaces and beside rtmi_render_budget, timed with HIP events in ONE run.

Cornell box at depth 50 and the bunny stand-in mesh (bench.py's C3 scene) at depth 10, 1024^2, each with a uniform budget
of 8 samples and with a random budget of tests/budgetlib.py's kind (0..16, a fifth zeros).  Per scene and budget:
  budget_ms       (a) one rtmi_render_budget
  per_sample_ms   (b) the per-sample loop: for every sample index camera_rays, trace_steps(compact=True), sample_add
  wavefront_ms    (c) render_wavefront at poll 1, 8 and 64
each the median of --reps runs after a warm-up, HIP events on one stream, every run on a renderer of its own from the
same seed (made outside the timed span); min and max of the repetitions beside each median.  (c)'s sums, moments, counts
and states must equal (a)'s bit for bit; whether (b)'s do is recorded.  Also: the iterations (c) enqueued, the library's
kernel launches of (b) and (c), the paths each step of (c) stepped and their mean, from a run of its own with a hook.
Every scene is measured in a child process of its own under a time limit, the whole run under another; the first failure
ends the run.  No gate: the claim to check is that (c) is not slower than (b) beyond the repetitions' spread.  Prints one
JSON line; --out also writes it to a file.

    python tools/gpu_path_advance_cost.py [--reps 7] [--size 1024] [--out profiles/path_advance_cost.json]
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
SCENES = (("cornell_box", 50), ("bunny", 10))
POLLS = (1, 8, 64)


def measure(scene, depth, reps, size):
    import numpy as np
    import torch
    sys.path.insert(0, ROOT)
    import bench  # the benchmark's scenes: bunny is its full stand-in mesh, as in C3
    import common
    import rtmi
    from budgetlib import random_budget

    b = bench.build_scene(rtmi.SceneBuilder(common.scene_seed(scene)), scene, 1.0).commit()

    def renderer(spp):
        return rtmi.Renderer(b, size, size, spp, depth, post=False).init_rng()

    def timed(spp, call):
        """call(R) on a fresh renderer per repetition; (median, min, max) in ms and the last renderer."""
        call(renderer(spp))  # (warm-up: code objects, the allocator's blocks)
        torch.cuda.synchronize()
        times, R = [], None
        for _ in range(reps):
            R = renderer(spp)
            R._budget_buffers()
            torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            call(R)
            e1.record()
            torch.cuda.synchronize()
            times.append(e0.elapsed_time(e1))
        return [round(statistics.median(times), 3), round(min(times), 3), round(max(times), 3)], R

    def per_sample(R, budget, n_samples):
        for s in range(n_samples):
            o, d = R.camera_rays(s, budget)
            st = R.scene.trace_steps(o, d, R.states, depth, compact=True)
            R.sample_add(s, st.rgb, st.steps + st.alive.to(torch.int32), budget)

    def buffers(R):
        return [t.clone() for t in (R.sum.view(torch.int32), R.sq.view(torch.int32), R.samples, R.budget_rays, R.states)]

    def same(x, y):
        return all(torch.equal(p, q) for p, q in zip(x, y))

    items = rtmi.work_items(rtmi.make_frame(size, size, 1, depth, False))
    res = {"depth": depth, "items": items}
    for kind in ("uniform_8", "random_0_16"):
        if kind == "uniform_8":
            spp, budget, n_samples = 8, None, 8
            d_budget = torch.full((items,), 8, dtype=torch.int32, device="cuda")
        else:
            spp = 16
            host = random_budget(5, items, hi=16)
            budget = d_budget = torch.from_numpy(host.astype(np.int32)).cuda()
            n_samples = int(host.max())
        out = {"spp_cap": spp, "samples": int(d_budget.sum().item()) if budget is not None else 8 * size * size}
        ms, Ra = timed(spp, lambda R: R.render_budget(d_budget))
        Ra.check()
        ref = buffers(Ra)
        out["budget_ms"], out["queries"] = ms, int(Ra.budget_rays.to(torch.int64).sum().item())
        ms, Rb = timed(spp, lambda R: per_sample(R, budget, n_samples))
        out["per_sample_ms"], out["per_sample_equals_budget"] = ms, same(buffers(Rb), ref)
        # camera rays, the first compaction, depth steps with depth - 1 compactions between them, the fold, the add
        out["per_sample_launches"] = n_samples * (1 + 3 + depth + 3 * (depth - 1) + 1 + 1)
        for poll in POLLS:
            ms, Rc = timed(spp, lambda R: R.render_wavefront(budget, poll=poll))
            Rc.check()
            assert same(buffers(Rc), ref), "render_wavefront (poll %d) and rtmi_render_budget disagree on %s" % (poll, scene)
            out["wavefront_poll%d_ms" % poll] = ms
            out["wavefront_poll%d_iterations" % poll] = Rc.wavefront_iterations
            # the first advance and compaction, then a step, an advance and a compaction per iteration
            out["wavefront_poll%d_launches" % poll] = 1 + 3 + Rc.wavefront_iterations * (1 + 1 + 3)
        works = []
        Rh = renderer(spp).render_wavefront(budget, each=lambda it, r: works.append(r.work), poll=1)
        Rh.check()
        stepped = [int(w[1].item()) for w in works]
        out["stepped"] = stepped
        out["mean_list_length"] = round(sum(stepped) / max(len(stepped), 1), 1)
        out["full_steps_worth"] = round(sum(stepped) / float(size * size), 2)
        c = out["wavefront_poll8_ms"][0]
        out["wavefront_over_per_sample"] = round(c / out["per_sample_ms"][0], 3)
        out["wavefront_over_budget"] = round(c / out["budget_ms"][0], 3)
        out["per_sample_over_budget"] = round(out["per_sample_ms"][0] / out["budget_ms"][0], 3)
        res[kind] = out
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--size", type=int, default=1024)
    ap.add_argument("--out", default=None)
    ap.add_argument("--scene", default=None, help="measure this one scene in this process and print its JSON")
    ap.add_argument("--scene-timeout", type=float, default=400.0, help="seconds a scene's child process may take")
    ap.add_argument("--timeout", type=float, default=780.0, help="seconds the whole run may take")
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
    line = json.dumps({"path_advance": res, "reps": a.reps, "size": a.size, "times": "[median, min, max] ms"})
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
