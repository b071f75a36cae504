"""The culls' margins, checked on every query.

Three culls of the HIP path are exact only because padded bounds and distance slacks cover the reach of the binary32
triangle test's false accepts (utils.cu:49-85) and of the binary32 sphere pre-test: the culled world-list scan
(hitable_list.cu:7-25), the grouped sphere scan (sphere.cu:11-44) and the mesh search whose finds the replay of
bvh.cuh:123-158 / bvh.cu:6-30 then filters.  `librtmi_check1.so` -- the same sources built with -DRTMI_CHECK_MARGINS
-DRTMI_CHECK_EVERY=1 by __graft_entry__.build() -- answers EVERY query a second time without any of them (meshes: by the
reference's own walk of its own tree) and counts the disagreements.  It is a diagnostic build, so the campaign
(tests/margin_campaign.py) runs in a process of its own with RTMI_LIB_PATH pointing at it; the oracle is not involved.
The culled scans share their candidate tests across a wave, so the campaign runs once in one unscheduled launch and
again on the scheduled paths (`tag@mode`), which put other rays together in a wave.  A resumed frame's check words
count over both of its launches, so every query of the plain scenes is re-done in every mode.
"""
import json
import os
import subprocess
import sys

import pytest

from abi_host import CHECK_LIB, ROOT

# the campaign's tags on the scheduled paths (tests/margin_campaign.py): plain scenes, then the adversarial families
PLAIN_SCHEDULED = {s + "@" + m for s in ("cornell_box_256x256x64_d50", "spheres_256x256x16_d8", "birthday_128x128x16_d10",
                                         "bunny_128x128x8_d10") for m in ("resumed", "probe_discarded")} | \
    {"cornell_box_256x256x64_d50@planned", "spheres_128x128x64_d8@planned", "birthday_64x64x64_d10@planned",
     "bunny_128x128x8_d10@sparse_1", "bunny_128x128x8_d10@sparse_64"}
SCHEDULED = PLAIN_SCHEDULED | {
    f + "@" + m for f in ("far_views_without_slivers", "far_views_with_slivers", "far_views_known_sliver_cases",
                          "grazing_views", "needles") for m in ("resumed", "sparse_64")} | {
    f + "@" + m for f in ("far_sphere_clouds", "needle_lists") for m in ("resumed", "lanes_16")}


@pytest.mark.gpu
def test_every_query_agrees_with_the_uncullled_answer():
    assert os.path.exists(CHECK_LIB), "librtmi_check1.so missing: run __graft_entry__.build() (make -C csrc check1)"
    env = dict(os.environ, RTMI_LIB_PATH=CHECK_LIB)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "margin_campaign.py")], env=env, cwd=ROOT,
                       stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=900)
    assert r.returncode in (0, 1), r.stderr[-4000:]
    out = json.loads(r.stdout[r.stdout.index("{"):])
    # every group of worlds re-did rays, and none of them disagreed
    want = {"cornell_box_256x256x64_d50", "spheres_256x256x16_d8", "birthday_128x128x16_d10", "quilt_100_0", "quilt_300_5",
            "quilt_100_from_1000", "quilt_100_from_10000", "spheres_200_from_1000", "spheres_200_from_10000",
            "bunny_128x128x8_d10", "far_views_without_slivers", "far_views_with_slivers", "far_views_known_sliver_cases",
            "grazing_views", "needles", "far_sphere_clouds", "needle_lists"} | SCHEDULED
    assert want <= set(out), sorted(want - set(out))
    for tag, v in out.items():
        assert v["re_done"] > 0, (tag, v)
        assert v["disagreements"] == 0, (tag, v)
    worlds = sum(v.get("worlds", 1) for v in out.values())
    assert worlds >= 200, worlds
    # every ray of the plain scenes was re-done (RTMI_CHECK_EVERY=1)
    for tag in ("cornell_box_256x256x64_d50", "spheres_256x256x16_d8", "birthday_128x128x16_d10", "bunny_128x128x8_d10"):
        assert out[tag]["re_done"] == out[tag]["rays"], (tag, out[tag])
    # ... and on the scheduled paths, whose waves share candidate tests between other rays than one launch's do.  A
    # resumed frame's words 33 / 34 count over both launches, so every query is re-done there too: first pass included.
    for tag in PLAIN_SCHEDULED:
        v = out[tag]
        assert v["re_done"] == v["rays"], (tag, v)
        assert v["mode"]["scheduled"] == 1, (tag, v)
        assert v["mode"]["first_pass_resumed"] == (0 if tag.endswith("@probe_discarded") else 1), (tag, v)
        if tag.endswith("@planned"):
            assert v["mode"]["planned_chains"] == 1, (tag, v)
    for tag in set(SCHEDULED) - set(PLAIN_SCHEDULED):
        v = out[tag]
        assert v["re_done"] == v["rays"], (tag, v)
        assert v["resumed"] == v["worlds"] > 0, (tag, v)  # (every family renders at least 4 spp: a first pass of 2)
        if tag.endswith("@lanes_16"):
            assert v["thin"] > 0, (tag, v)

