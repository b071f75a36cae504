#!/usr/bin/env python3
"""Rate of rtmi_intersect (batched closest-hit queries), timed with HIP events.

Camera rays of a 1024^2 pinhole view (one per pixel, through the pixel centre) and secondary rays (from the camera
rays' first hits, in random directions: incoherent) on cornell_box and the bunny stand-in mesh (the scenes of bench.py's C2 / C3).  Prints one JSON line:
Gqueries/s per (scene, ray family), beside the render's closest-hit queries per second on the same scene from the
committed default bench run (profiles/r04n_bench_default.json: C2 cornell 1024^2, C3 bunny 1024^2).

    python tools/gpu_query_rate.py [--reps 10] [--size 1024]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "ray-tracing-cuda_amd"), os.path.join(ROOT, "tests")]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--size", type=int, default=1024)
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
        return cam[0].expand(d.shape[0], 3).contiguous(), d.contiguous()

    def timed(b, o, d):
        out = torch.empty((o.shape[0], 12), dtype=torch.int32, device="cuda")
        for _ in range(2):
            b.intersect(o, d, out=out).check()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(a.reps):
            h = b.intersect(o, d, out=out)
        e1.record()
        torch.cuda.synchronize()
        h.check()
        ms = e0.elapsed_time(e1) / a.reps
        return ms, h

    res = {}
    g = torch.Generator(device="cuda").manual_seed(1)
    for scene in ("cornell_box", "bunny"):
        b = bench.build_scene(rtmi.SceneBuilder(common.scene_seed(scene)), scene, 1.0).commit()
        o, d = camera_rays(b, a.size)
        ms, h = timed(b, o, d)
        res[scene + "_camera"] = {"rays": o.shape[0], "ms": round(ms, 4), "gqueries_per_s": round(o.shape[0] / ms / 1e6, 3),
                                  "hit_fraction": round(float((h.kind != rtmi.RTMI_HIT_NONE).float().mean()), 4)}
        solid = (h.kind != rtmi.RTMI_HIT_NONE) & (h.kind != rtmi.RTMI_HIT_SKY)
        dn = d / d.norm(dim=1, keepdim=True)
        p = (o + h.t[:, None] * dn)[solid].contiguous()
        r = torch.randn(p.shape, generator=g, device="cuda")
        nd = (h.normal[solid] + r / r.norm(dim=1, keepdim=True)).contiguous()  # about the hit normal: leaves the surface
        ms2, _ = timed(b, p, nd)
        res[scene + "_secondary"] = {"rays": p.shape[0], "ms": round(ms2, 4), "gqueries_per_s": round(p.shape[0] / ms2 / 1e6, 3)}
    render = {}
    try:
        with open(os.path.join(ROOT, "profiles", "r04n_bench_default.json")) as f:
            bj = json.load(f)
        render["cornell_box"] = round(bj["value"] / 1e3, 2)  # Mrays/s -> Grays/s (C2)
        for x in bj.get("config", {}).get("extra", []):
            if x.get("workload", "").startswith("c3:"):
                render["bunny"] = round(x["value"] / 1e3, 2)
    except (OSError, ValueError, KeyError):
        pass
    print(json.dumps({"query": res, "render_gqueries_per_s_r04n": render, "reps": a.reps}))


if __name__ == "__main__":
    main()
