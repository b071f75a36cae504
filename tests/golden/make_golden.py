#!/usr/bin/env python3
"""Generates tests/golden/*.npz.

Without arguments: from the CPU oracle (oracle/oracle.cc).  These serve as (1) a cross-machine determinism check of
the oracle and (2) fixed expected outputs for the HIP path.  Each file holds rgb float32 (H,W,3), per-pixel ray counts
uint32 (H,W), final RNG states uint32 (H*W,6).

--ref: from the reference's own renderer built for the CPU (oracle/_ref/libref.so, which needs the reference checkout:
make -C oracle _ref/libref.so).  Everything written is data that the reference's code produced, with the inputs it
was given, so the pin travels to machines without the checkout (tests/test_ref_golden.py, tests/test_gpu_ref_golden.py):
  ref_<scene>_<h>x<w>_s<spp>_d10_{post,raw}.npz   seeds (2,), rgb (2,H,W,3), rays (2,H,W), states (2,H*W,6), total (2,)
  ref_probe_<world>.npz    table (N,8) {origin, direction, t_from, t_to}, hit, rec {t,u,v,normal}, mat, keep (the fields
                           of rec that the reference defines; the others are stored as zero)
  ref_scatter.npz          table, states, scattered, out {attenuation, ray, emitted}, after
  ref_camera.npz           xy, states, and per camera kind: frame, rays, after
The cases are those of tests/refcases.py; the probe tables are a quarter of the length tests/test_ref_parity.py uses.

Run from the repo root:  python tests/golden/make_golden.py [--ref]
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, os.path.join(ROOT, "ray-tracing-cuda_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import common  # noqa: E402

# name, H, W, spp, depth, post, extra kwargs
CASES = [
    ("cornell_box", 24, 32, 4, 10, True, {}),
    ("cornell_box", 16, 16, 2, 50, False, {}),
    ("spheres", 24, 32, 2, 8, True, {}),
    ("bunny", 24, 32, 2, 10, True, {"k_min": 64}),
    ("birthday", 24, 32, 4, 10, True, {}),
    ("mixed", 20, 28, 4, 10, True, {}),
    ("furnace", 16, 16, 4, 10, True, {}),
    ("sky_only", 16, 24, 2, 10, True, {}),
]


def case_file(name, h, w, spp, depth, post):
    return os.path.join(HERE, "%s_%dx%d_s%d_d%d_%s.npz" % (name, h, w, spp, depth, "post" if post else "raw"))


def main():
    for name, h, w, spp, depth, post, kw in CASES:
        rgb, rays, states, total, _ = common.oracle_render(name, h, w, spp, depth, post=post, **kw)
        np.savez_compressed(case_file(name, h, w, spp, depth, post), rgb=rgb, rays=rays, states=states,
                            total=np.uint64(total), seed=np.uint64(common.scene_seed(name)))
        print("%-12s %dx%d s%d d%d %s -> %d rays" % (name, h, w, spp, depth, "post" if post else "raw", total))


def main_ref():
    import oraclelib
    import refcases as rc
    import reflib
    assert reflib.available(), reflib.SKIP_REASON
    for name, h, w, spp in rc.FRAMES:
        for post in (True, False):
            res = []
            for seed in rc.SEEDS:
                res.append(rc.build_frame_scene(reflib.RefBuilder(seed), name, w / h).render(h, w, spp, post=post))
            rgb, rays, states, total = (np.stack([np.asarray(r[k]) for r in res]) for k in range(4))
            np.savez_compressed(os.path.join(HERE, rc.frame_file(name, h, w, spp, post)), seeds=np.array(rc.SEEDS, dtype=np.uint64),
                                rgb=rgb, rays=rays, states=states, total=total.astype(np.uint64))
            print("%-28s %s" % (rc.frame_file(name, h, w, spp, post), total))
    for name in rc.PROBE_WORLDS:
        r = rc.build_probe_world(reflib.RefBuilder(1), name)
        table = rc.probe_table(r, name, scale=0.25)
        hit, rec, mat = rc.run_probes(r, table)
        keep = rc.defined_columns(name, hit, rec, mat)
        np.savez_compressed(os.path.join(HERE, "ref_probe_%s.npz" % name), table=table, hit=hit, rec=np.where(keep, rec, 0.0),
                            mat=mat, keep=keep)
        print("ref_probe_%-18s %d rays, %d hits" % (name, table.shape[0], hit.sum()))
    r = reflib.RefBuilder(1)
    rc.scatter_materials(r)
    table, states = rc.scatter_table(n_per_material=60)
    sc, out, after = rc.run_scatter(r, table, states)
    np.savez_compressed(os.path.join(HERE, "ref_scatter.npz"), table=table, states=states, scattered=sc, out=out, after=after)
    xy, states = rc.camera_table()
    cam = {"xy": xy, "states": states}
    for kind in rc.CAMERAS:
        cam[kind + "_frame"], cam[kind + "_rays"], cam[kind + "_after"] = rc.run_camera(rc.build_camera(reflib.RefBuilder(1), kind), xy, states)
    np.savez_compressed(os.path.join(HERE, "ref_camera.npz"), **cam)
    print("ref_scatter.npz, ref_camera.npz")


if __name__ == "__main__":
    main_ref() if "--ref" in sys.argv[1:] else main()
