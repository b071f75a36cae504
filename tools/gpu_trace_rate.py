#!/usr/bin/env python3
"""Rate of rtmi_trace (path-traced radiance of caller rays), timed with HIP events, beside the render's own rate.

The rays of a view: the camera rays of a 1024^2 pinhole frame (one per pixel, through the pixel centre), repeated so
that the batch holds 16 rays per pixel, each with its own state from rtmi_rng_init_n.  Cornell box at depth 50, the
bunny stand-in mesh (bench.py's C3 scene) at depth 10.  The render of the same view -- the same scene, 1024^2, 16
samples per pixel, the same depth -- is timed the same way.  Both rates are closest-hit queries per second (the trace's
d_work[1], the render's total_rays()), the median of --reps calls.  Prints one JSON line.  Kernel time alone: run it
under rocprofv3 --kernel-trace --stats (trace_kernel<F> against render_kernel<F>).

    python tools/gpu_trace_rate.py [--reps 7] [--size 1024] [--spp 16]
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "ray-tracing-cuda_amd"), os.path.join(ROOT, "tests")]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--size", type=int, default=1024)
    ap.add_argument("--spp", type=int, default=16)
    a = ap.parse_args()
    import torch
    sys.path.insert(0, ROOT)
    import bench  # the benchmark's scenes: bunny is its full stand-in mesh, as in C3
    import common
    import rtmi

    def camera_rays(b, n_side):
        cam = torch.from_numpy(b.camera_get()[:4].copy()).cuda()  # position, lower-left corner, horizontal, vertical
        s = (torch.arange(n_side, device="cuda", dtype=torch.float32) + 0.5) / n_side
        y, x = torch.meshgrid(1 - s, s, indexing="ij")
        d = cam[1] + x.reshape(-1, 1) * cam[2] + y.reshape(-1, 1) * cam[3] - cam[0]
        return cam[0].expand(d.shape[0], 3).contiguous(), (d / d.norm(dim=1, keepdim=True)).contiguous()

    def median_ms(call):
        call()  # (warm-up: code objects, LDS attributes)
        torch.cuda.synchronize()
        times, out = [], None
        for _ in range(a.reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            out = call()
            e1.record()
            torch.cuda.synchronize()
            times.append(e0.elapsed_time(e1))
        return statistics.median(times), out

    res = {}
    for scene, depth in (("cornell_box", 50), ("bunny", 10)):
        b = bench.build_scene(rtmi.SceneBuilder(common.scene_seed(scene)), scene, 1.0).commit()
        o, d = camera_rays(b, a.size)
        o, d = o.repeat(a.spp, 1).contiguous(), d.repeat(a.spp, 1).contiguous()
        n = o.shape[0]
        states = rtmi.rng_states(1, n)
        rgb = torch.empty((n, 3), dtype=torch.float32, device="cuda")
        ms, tr = median_ms(lambda: b.trace(o, d, states, depth, out=rgb))
        tr.check()
        q = tr.total_rays()
        R = rtmi.Renderer(b, a.size, a.size, a.spp, depth, post=True)
        R.init_rng()

        def render():
            R.render(count_rays=False)
            return R
        rms, _ = median_ms(render)
        R.check()
        rq = R.total_rays()
        res[scene] = {"depth": depth, "rays": n, "trace_ms": round(ms, 3), "trace_queries": q,
                      "trace_gqueries_per_s": round(q / ms / 1e6, 3), "render_ms": round(rms, 3), "render_queries": rq,
                      "render_gqueries_per_s": round(rq / rms / 1e6, 3), "ratio": round((q / ms) / (rq / rms), 3)}
    print(json.dumps({"trace": res, "reps": a.reps, "size": a.size, "rays_per_pixel": a.spp}))


if __name__ == "__main__":
    main()
