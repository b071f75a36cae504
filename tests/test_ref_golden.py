"""The oracle against the reference renderer's recorded outputs (tests/golden/ref_*.npz, written by
tests/golden/make_golden.py --ref from the reference's own code built for the CPU).  Runs anywhere: no reference
checkout, no GPU.  Every comparison is an equality of bits; the three operations that the host build of the reference
decides differently from the oracle are switched as in tests/test_ref_parity.py, whose docstring names them."""
import os

import numpy as np
import pytest

import oraclelib
import refcases as rc
from refcases import bits

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def load(name):
    path = os.path.join(GOLDEN, name)
    assert os.path.exists(path), name + " missing: tests/golden/make_golden.py --ref writes it"
    return np.load(path)


@pytest.mark.parametrize("post", [True, False], ids=["post", "raw"])
@pytest.mark.parametrize("name,h,w,spp", rc.FRAMES, ids=[f[0] for f in rc.FRAMES])
def test_oracle_reproduces_reference_frame(name, h, w, spp, post):
    g = load(rc.frame_file(name, h, w, spp, post))
    assert tuple(int(s) for s in g["seeds"]) == rc.SEEDS
    for k, seed in enumerate(rc.SEEDS):
        o = rc.build_frame_scene(oraclelib.OracleBuilder(seed), name, w / h)
        rgb, rays, states, total = o.render(h, w, spp, rc.DEPTH, post=post)
        assert total == int(g["total"][k])
        assert np.array_equal(rays, g["rays"][k])
        assert np.array_equal(states, g["states"][k])
        assert np.array_equal(bits(rgb), bits(g["rgb"][k])), "%s seed %d: %d values differ" % (
            name, seed, int((bits(rgb) != bits(g["rgb"][k])).sum()))


@pytest.mark.parametrize("name", list(rc.PROBE_WORLDS))
def test_oracle_reproduces_reference_probes(name):
    g = load("ref_probe_%s.npz" % name)
    with oraclelib.host_variant(rc.PROBE_VARIANT.get(name, 0)):
        hit, rec, mat = rc.run_probes(rc.build_probe_world(oraclelib.OracleBuilder(1), name), g["table"])
    assert g["hit"].sum() > 10
    assert np.array_equal(hit, g["hit"])
    assert np.array_equal(mat, g["mat"])
    assert np.array_equal(bits(np.where(g["keep"], rec, 0.0)), bits(g["rec"]))


def test_oracle_reproduces_reference_scatter():
    g = load("ref_scatter.npz")
    o = oraclelib.OracleBuilder(1)
    rc.scatter_materials(o)
    sc, out, after = rc.run_scatter(o, g["table"], g["states"])
    assert np.array_equal(sc, g["scattered"])
    assert np.array_equal(bits(out), bits(g["out"]))
    assert np.array_equal(after, g["after"])


@pytest.mark.parametrize("kind", rc.CAMERAS)
def test_oracle_reproduces_reference_camera(kind):
    g = load("ref_camera.npz")
    with oraclelib.host_variant(oraclelib.VARIANT_DISKRAND_RTL if kind == "defocus" else 0):
        frame, rays, after = rc.run_camera(rc.build_camera(oraclelib.OracleBuilder(1), kind), g["xy"], g["states"])
    assert np.array_equal(bits(frame), bits(g[kind + "_frame"]))
    assert np.array_equal(bits(rays), bits(g[kind + "_rays"]))
    assert np.array_equal(after, g[kind + "_after"])
