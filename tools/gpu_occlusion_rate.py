#!/usr/bin/env python3
"""Rate of rtmi_occluded (any-hit visibility queries) beside rtmi_intersect with the same t_max, timed with HIP events.

Ray families on bench.py's scenes (cornell_box, and the bunny stand-in mesh of C3):
  cornell_shadow  from the first hits of a size^2 pinhole view (one ray per pixel centre) to random points of the
                  light parallelogram, t_max = 0.999 x the distance;
  bunny_ao_*      from the first mesh hits of the bunny view, about the hit normal (normal + a random unit vector),
                  t_max = 2 % and 20 % of the mesh hits' extent, and +inf.
Per family one JSON line: rays, ms per call of each entry (median over --reps repetitions after a warm-up; each
repetition times --calls calls issued back to back between one pair of HIP events, as tools/gpu_query_rate.py does, so
that host dispatch overlaps the kernels), Gqueries/s, the occluded fraction, the fraction of rays the occlusion
kernel's exact fallback answered, and the rays where the two entries disagree (must be 0).  For kernel durations
alone run it under `rocprofv3 --kernel-trace --stats -- python tools/gpu_occlusion_rate.py`.

    python tools/gpu_occlusion_rate.py [--reps 7] [--calls 20] [--size 1024] [--only FAMILY]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "ray-tracing-cuda_amd"), os.path.join(ROOT, "tests")]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--size", type=int, default=1024)
    ap.add_argument("--only", default=None, help="run this family alone (e.g. for a kernel trace of it)")
    a = ap.parse_args()
    if a.reps < 5 or a.calls < 1:
        ap.error("--reps must be at least 5, --calls at least 1")
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

    def median_ms(fn):
        for _ in range(2):
            fn()
        torch.cuda.synchronize()
        ms = []
        for _ in range(a.reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(a.calls):
                fn()
            e1.record()
            torch.cuda.synchronize()
            ms.append(e0.elapsed_time(e1) / a.calls)
        ms.sort()
        return ms[len(ms) // 2], ms

    def family(b, o, d, tm):
        n = o.shape[0]
        occ_out = torch.empty((n,), dtype=torch.uint8, device="cuda")
        hit_out = torch.empty((n, 12), dtype=torch.int32, device="cuda")
        ms_o, all_o = median_ms(lambda: b.occluded(o, d, tm, out=occ_out))
        ms_i, all_i = median_ms(lambda: b.intersect(o, d, tm, out=hit_out))
        r = b.occluded(o, d, tm, out=occ_out).check()
        h = b.intersect(o, d, tm, out=hit_out).check()
        ref = h.kind != rtmi.RTMI_HIT_NONE
        return {"rays": n, "occluded_ms": round(ms_o, 4), "intersect_ms": round(ms_i, 4),
                "occluded_gq_per_s": round(n / ms_o / 1e6, 3), "intersect_gq_per_s": round(n / ms_i / 1e6, 3),
                "occluded_ms_range": [round(min(all_o), 4), round(max(all_o), 4)],
                "intersect_ms_range": [round(min(all_i), 4), round(max(all_i), 4)],
                "occluded_fraction": round(float(r.mask.float().mean()), 4),
                "fallback_fraction": round(r.fallback_rays() / n, 6),
                "disagreements": int((r.mask != ref).sum())}

    g = torch.Generator(device="cuda").manual_seed(1)
    out = {}
    # cornell: shadow rays from the first hits to random points of the light (scenes.cornell_box: its third parallelogram)
    b = bench.build_scene(rtmi.SceneBuilder(common.scene_seed("cornell_box")), "cornell_box", 1.0).commit()
    o, d = camera_rays(b, a.size)
    h = b.intersect(o, d).check()
    solid = (h.kind != rtmi.RTMI_HIT_NONE) & (h.kind != rtmi.RTMI_HIT_SKY)
    dn = d / d.norm(dim=1, keepdim=True)
    p = (o + h.t[:, None] * dn)[solid].contiguous()
    L0 = torch.tensor([213.0, 554.0, 332.0], device="cuda")
    e1, e2 = torch.tensor([0.0, 0.0, -105.0], device="cuda"), torch.tensor([130.0, 0.0, 0.0], device="cuda")
    uv = torch.rand((p.shape[0], 2), generator=g, device="cuda")
    q = L0 + uv[:, :1] * e1 + uv[:, 1:] * e2
    sd = (q - p).contiguous()
    tm = (0.999 * sd.norm(dim=1)).contiguous()
    if a.only in (None, "cornell_shadow"):
        out["cornell_shadow"] = family(b, p, sd, tm)
    # bunny: ambient-occlusion rays from the first mesh hits
    b = bench.build_scene(rtmi.SceneBuilder(common.scene_seed("bunny")), "bunny", 1.0).commit()
    o, d = camera_rays(b, a.size)
    h = b.intersect(o, d).check()
    mesh = h.kind == rtmi.RTMI_HIT_MESH
    dn = d / d.norm(dim=1, keepdim=True)
    p = (o + h.t[:, None] * dn)[mesh].contiguous()
    r = torch.randn(p.shape, generator=g, device="cuda")
    ad = (h.normal[mesh] + r / r.norm(dim=1, keepdim=True)).contiguous()
    ext = float((p.max(0).values - p.min(0).values).max())
    for tag, frac in (("bunny_ao_2pct", 0.02), ("bunny_ao_20pct", 0.2), ("bunny_ao_inf", float("inf"))):
        tm = torch.full((p.shape[0],), frac * ext, dtype=torch.float32, device="cuda")
        if a.only in (None, tag):
            out[tag] = family(b, p, ad, tm)
    for tag, v in out.items():
        print(json.dumps(dict(family=tag, reps=a.reps, calls=a.calls, **v)))


if __name__ == "__main__":
    main()
