"""The diffuse kernels on the host side (kernels.h: PIN_DIFFUSE): the scene fact that picks them, the six pinned symbols
in both builds of the library, and the registers and LDS the new three are held to.  No GPU involved.

The constants are those of the sources, restated: the test holds the library to the numbers, not to its own headers."""
import re

import numpy as np

import common
import rtmi
from abi_host import LIBS
from diffuse_worlds import diffuse_only
from rtmi import scenes
from tri_tasks_worlds import v3

PIN_DIFFUSE = 512            # kernels.h
CHAINS, QUEUE = 255, 383     # kFastChains, kFastQueue
PINNED = ("render_kernelILj2ELj%dE" % CHAINS, "render_kernelILj2ELj%dE" % QUEUE, "probe_kernelILj2ELj%dE" % QUEUE)
DIFFUSE = ("render_kernelILj2ELj%dE" % (CHAINS | PIN_DIFFUSE), "render_kernelILj2ELj%dE" % (QUEUE | PIN_DIFFUSE),
           "probe_kernelILj2ELj%dE" % (QUEUE | PIN_DIFFUSE))
LDS_PER_CU = 160 * 1024      # a compute unit's LDS on gfx950
SCALAR_SPILLS_CHAINS = 5     # what render_kernel<F_TRIS, kFastChains> spills: a sixth would be a new one


def _count(blk, key):
    return int(re.search(r"\.%s:\s+(\d+)" % key, blk).group(1))


def _waves(vgprs):
    """Waves per SIMD of gfx950 by the unified VGPR count (512 per SIMD lane, granules of 8)."""
    return min(8, 512 // ((vgprs + 7) // 8 * 8))


def _scene(fill):
    b = rtmi.SceneBuilder(3)
    b.camera_pinhole(v3(0, 0, -3), v3(0, 0, 0), v3(0, 1, 0), 1.0, 1.0)
    mats = fill(b)
    for i, m in enumerate(mats):  # every material on a surface of its own
        b.parallelogram([v3(i, 0, 0), v3(i + 1, 0, 0), v3(i, 1, 0)], m)
    return b


def test_lambertians_and_lights_alone_are_diffuse():
    assert diffuse_only(_scene(lambda b: [b.lambertian(v3(0.5, 0.4, 0.3))]))
    assert diffuse_only(_scene(lambda b: [b.diffuse_light(b.constant_texture(v3(4, 4, 4)))]))
    assert diffuse_only(_scene(lambda b: [b.lambertian(v3(0.5, 0.4, 0.3)), b.diffuse_light(b.constant_texture(v3(1, 1, 1))),
                                          b.lambertian_tex(b.constant_texture(v3(0.1, 0.2, 0.3)))]))
    c = rtmi.SceneBuilder(common.scene_seed("cornell_box"))
    scenes.cornell_box(c, 1.0)
    assert diffuse_only(c), "the Cornell box is what the kernels are for"


def test_any_other_material_is_not():
    lam = lambda b: b.lambertian(v3(0.5, 0.4, 0.3))
    image = np.full((2, 2, 4), 128, dtype=np.uint8)
    assert not diffuse_only(_scene(lambda b: [lam(b), b.metal(v3(0.8, 0.8, 0.8), 0.0)]))
    assert not diffuse_only(_scene(lambda b: [b.metal(v3(0.8, 0.8, 0.8), 0.5), lam(b)]))
    assert not diffuse_only(_scene(lambda b: [lam(b), b.dielectric(v3(1, 1, 1), 1.5)]))
    assert not diffuse_only(_scene(lambda b: [lam(b), b.lambertian_tex(b.image_texture(image))]))
    assert not diffuse_only(_scene(lambda b: [lam(b), b.diffuse_light(b.image_texture(image))]))


def test_a_material_nothing_uses_counts():
    """The rule reads the table, not the world: one metal that no primitive has keeps the scene's kernels as they were."""
    c = rtmi.SceneBuilder(common.scene_seed("cornell_box"))
    scenes.cornell_box(c, 1.0)
    c.metal(v3(0.8, 0.8, 0.8), 0.25)
    assert not diffuse_only(c)


def test_all_six_pinned_kernels_are_in_both_builds():
    for lib in LIBS:
        names = list(common.kernel_notes(lib))
        for w in PINNED + DIFFUSE:
            assert sum(w in n for n in names) == 1, (lib, w)


def test_the_diffuse_kernels_hold_the_register_and_lds_bounds():
    """At most 80 VGPRs (six waves per SIMD), no static LDS; the chains kernel spills no VGPR dword and no scalar beyond
    the five its parent spills; the queue kernels no more than theirs.  Six workgroups of C2's launch fit a CU's LDS."""
    notes = common.kernel_notes(LIBS[0])
    block = lambda key: [blk for name, blk in notes.items() if key in name][0]
    for new, old in zip(DIFFUSE, PINNED):
        blk = block(new)
        print(new, {k: _count(blk, k) for k in ("vgpr_count", "sgpr_count", "vgpr_spill_count", "sgpr_spill_count")})
        assert _count(blk, "vgpr_count") <= 80 and _waves(_count(blk, "vgpr_count")) >= 6, new
        assert _count(blk, "group_segment_fixed_size") == 0, new
        assert _count(blk, "vgpr_spill_count") <= _count(block(old), "vgpr_spill_count"), new
        assert _count(blk, "sgpr_spill_count") <= _count(block(old), "sgpr_spill_count"), new
    chains = block(DIFFUSE[0])
    assert _count(chains, "vgpr_spill_count") == 0 and _count(chains, "private_segment_fixed_size") == 0
    assert _count(chains, "sgpr_spill_count") <= SCALAR_SPILLS_CHAINS
    c = rtmi.SceneBuilder(common.scene_seed("cornell_box"))
    scenes.cornell_box(c, 1.0)
    assert 6 * c.render_lds_bytes(50, 256) <= LDS_PER_CU

