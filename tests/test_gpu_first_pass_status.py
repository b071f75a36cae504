"""A search abandoned in the first pass of a resumed frame fails the frame.

rtmi_render draws a scheduled frame in two launches: samples [0, s1) of every pixel into the caller's buffers, then the
rest resumed at s1.  Counter word 2 counts abandoned mesh searches, and it is the only signal that
rtmi_render_status, Renderer.check(), Renderer.total_rays() and rtmi_last_ray_total use to call a frame incomplete.  The
first pass's samples stay in the image, so what it abandoned must still be counted after the second launch.

No world makes the search abandon one (mesh_search.h: the stack reserve), so the test plants one.  The margin-check
build (librtmi_check1.so) has a hook for it: RTMI_CHECK_PLANT_ABANDONED=1, read once per process, adds 1 to word 2
right after every first pass a frame keeps.  The renders run in processes of their own, once with the hook and once
without: with it, every resumed frame must report RTMI_ERR_INTERNAL, and the frames without a kept first pass
(unscheduled, a discarded probe) must stay OK.  Image, ray counts, RNG states and every counter word but 2 must be
the same either way: the hook touches nothing else.
"""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHECK_LIB = os.path.join(ROOT, "ray-tracing-cuda_amd", "lib", "librtmi_check1.so")
HOOK = "RTMI_CHECK_PLANT_ABANDONED"
RTMI_OK, RTMI_ERR_INTERNAL = 0, -6
# (scene, side, spp, depth): a mesh frame and a list frame, both resumed under schedule=2 (a first pass of 2 samples)
SCENES = (("bunny", 64, 8, 10), ("cornell_box", 64, 32, 10))
MODES = (("resumed", dict(schedule=2)), ("unscheduled", dict(schedule=0)), ("probe_discarded", dict(schedule=2, first_pass=0)))
KEEPS_FIRST_PASS = {"resumed"}
# counter words that differ from run to run (queue and head cursors, planned chains' arrival and take-over)
RACY_WORDS = (0, 3, 35, 36)


def child(path):
    """Every render of SCENES x MODES x {scene-owned counters, caller-owned scratch}; results to `path` (.npz)."""
    sys.path.insert(0, os.path.join(ROOT, "ray-tracing-cuda_amd"))
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import torch
    import rtmi
    import common
    assert "check" in os.path.basename(rtmi.LIB_PATH), rtmi.LIB_PATH
    L = rtmi.lib()
    res = {}
    for name, side, spp, depth in SCENES:
        b = common.build_scene(rtmi.SceneBuilder(common.scene_seed(name)), name, 1.0).commit()
        for mode, kw in MODES:
            for owner in ("scene", "scratch"):
                key = "%s_%s_%s" % (name, mode, owner)
                R = rtmi.Renderer(b, side, side, spp, depth).init_rng()
                scratch = R.new_scratch() if owner == "scratch" else None
                opts = rtmi.render_opts(scratch=scratch, **kw)
                m = R.mode(opts)
                R.render(opts=opts)
                torch.cuda.synchronize()
                sp = C.c_void_p(scratch.data_ptr()) if scratch is not None else None
                rays = C.c_uint64(0)
                status = L.rtmi_render_status(b.h, sp, C.byref(rays), R._stream())
                words = (C.c_ulonglong * 40)()
                assert L.rtmi_debug_counters_ex(b.h, sp, words, R._stream()) == 0
                refused = []
                for what, call in (("check", R.check), ("total_rays", lambda: R.total_rays(scratch)),
                                   ("untile", lambda: R.untile())):
                    try:
                        call()
                    except rtmi.RtmiError:
                        refused.append(what)
                res[key + "/resumed"] = np.int64(m["first_pass_resumed"])
                res[key + "/status"] = np.int64(status)
                res[key + "/rays"] = np.uint64(rays.value)
                res[key + "/words"] = np.array(list(words), dtype=np.uint64)
                res[key + "/refused"] = np.array(",".join(refused))
                res[key + "/tiles"] = R.tiles.cpu().numpy()
                res[key + "/ray_counts"] = R.ray_counts.cpu().numpy()
                res[key + "/states"] = R.states.cpu().numpy()
    np.savez(path, **res)


def _renders(tmp_path, plant):
    env = dict(os.environ, RTMI_LIB_PATH=CHECK_LIB)
    env.pop(HOOK, None)
    if plant:
        env[HOOK] = "1"
    path = str(tmp_path / ("planted.npz" if plant else "plain.npz"))
    r = subprocess.run(["timeout", "-k", "10", "300", sys.executable, os.path.abspath(__file__), path], env=env, cwd=ROOT,
                       stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    assert r.returncode == 0, (r.returncode, r.stderr[-4000:])
    return dict(np.load(path))


@pytest.mark.gpu
def test_an_abandoned_search_in_the_first_pass_fails_the_frame(tmp_path):
    assert os.path.exists(CHECK_LIB), "librtmi_check1.so missing: run __graft_entry__.build() (make -C csrc check1)"
    plain = _renders(tmp_path, False)
    planted = _renders(tmp_path, True)
    for name, side, spp, _ in SCENES:
        for mode, _ in MODES:
            for owner in ("scene", "scratch"):
                key = "%s_%s_%s" % (name, mode, owner)
                p = {k.split("/")[1]: v for k, v in plain.items() if k.startswith(key + "/")}
                q = {k.split("/")[1]: v for k, v in planted.items() if k.startswith(key + "/")}
                assert p["resumed"] == q["resumed"] == (mode in KEEPS_FIRST_PASS), (key, p["resumed"])
                # without the hook: complete
                assert p["status"] == RTMI_OK and str(p["refused"]) == "" and p["words"][2] == 0, (key, p["status"], p["refused"])
                if mode in KEEPS_FIRST_PASS:
                    # the planted abandonment of the first pass survives the second launch, and every way of asking refuses
                    assert q["status"] == RTMI_ERR_INTERNAL, (key, q["status"], q["words"][:4])
                    assert q["words"][2] == 1, (key, q["words"][:4])
                    assert str(q["refused"]) == "check,total_rays,untile", (key, q["refused"])
                else:
                    # no first pass the frame keeps: nothing planted
                    assert q["status"] == RTMI_OK and str(q["refused"]) == "" and q["words"][2] == 0, (key, q["status"], q["refused"])
                # the hook changes nothing but word 2
                assert p["rays"] == q["rays"] == p["words"][1] == q["words"][1] >= side * side * spp, (key, p["rays"], q["rays"])
                for w in range(40):
                    if w != 2 and w not in RACY_WORDS:
                        assert p["words"][w] == q["words"][w], (key, w, p["words"][w], q["words"][w])
                for a in ("tiles", "ray_counts", "states"):
                    assert np.array_equal(p[a], q[a], equal_nan=True), (key, a)


if __name__ == "__main__":
    child(sys.argv[1])
