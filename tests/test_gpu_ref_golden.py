"""librtmi against the reference renderer's recorded frames (tests/golden/ref_*.npz, written by
tests/golden/make_golden.py --ref from the reference's own code built for the CPU): image, per-pixel query counts and
final RNG states, bit for bit, at depth 10 with both of the reference's seeds.  Reads nothing but tests/golden/.

The image-textured sphere (birthday) keeps the suite's rule for it: counts and states exact, image within 1e-3
relative L2, because acosf / atan2f pick the texel and the device's libm is not the host's."""
import os

import numpy as np
import pytest

import common
import refcases as rc
from test_gpu_parity import REL_L2_TOL, gpu_states_rowmajor

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def gpu_frame(name, h, w, spp, post, seed):
    import torch
    import rtmi
    b = rc.build_frame_scene(rtmi.SceneBuilder(seed), name, w / h).commit()
    R = rtmi.Renderer(b, h, w, spp, rc.DEPTH, post).init_rng()
    R.render()
    img, cnt = R.untile()
    torch.cuda.synchronize()
    return img.cpu().numpy(), cnt.cpu().numpy().astype(np.uint32), gpu_states_rowmajor([R.states], h, w), R.total_rays()


@pytest.mark.parametrize("post", [True, False], ids=["post", "raw"])
@pytest.mark.parametrize("name,h,w,spp", rc.FRAMES, ids=[f[0] for f in rc.FRAMES])
def test_render_matches_reference_frame(name, h, w, spp, post):
    g = np.load(os.path.join(GOLDEN, rc.frame_file(name, h, w, spp, post)))
    for k, seed in enumerate(rc.SEEDS):
        rgb, rays, states, total = gpu_frame(name, h, w, spp, post, seed)
        assert total == int(g["total"][k])
        assert np.array_equal(rays, g["rays"][k])
        assert np.array_equal(states, g["states"][k])
        if name == "birthday":
            assert common.rel_l2(rgb, g["rgb"][k]) <= REL_L2_TOL
        else:
            assert np.array_equal(rgb.view(np.uint32), g["rgb"][k].view(np.uint32)), "%s seed %d: %d values differ" % (
                name, seed, int((rgb != g["rgb"][k]).sum()))
