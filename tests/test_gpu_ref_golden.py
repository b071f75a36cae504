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
import rtmi
from parity import Frame, assert_same_frame, gpu_frame

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
REL_L2_TOL = 1e-3  # as tests/test_gpu_parity.py: "image within 1e-3 relative L2 of reference"


@pytest.mark.parametrize("post", [True, False], ids=["post", "raw"])
@pytest.mark.parametrize("name,h,w,spp", rc.FRAMES, ids=[f[0] for f in rc.FRAMES])
def test_render_matches_reference_frame(name, h, w, spp, post):
    g = np.load(os.path.join(GOLDEN, rc.frame_file(name, h, w, spp, post)))
    for k, seed in enumerate(rc.SEEDS):
        pb = rc.build_frame_scene(rtmi.SceneBuilder(seed), name, w / h).commit()
        got = gpu_frame(pb, h, w, spp, rc.DEPTH, post)
        want = Frame(g["rgb"][k], g["rays"][k], g["states"][k], int(g["total"][k]), None)
        if name == "birthday":  # the image within the tolerance; everything else exact
            assert common.rel_l2(got.image, want.image) <= REL_L2_TOL
            got = got._replace(image=want.image)
        assert_same_frame(got, want, "%s seed %d" % (name, seed))
