"""Oracle vs the committed golden vectors (tests/golden/*.npz, made by make_golden.py):
pins the oracle's determinism across machines and compilers."""
import glob
import os
import re

import numpy as np
import pytest

import common

HERE = os.path.dirname(os.path.abspath(__file__))
# the oracle's own goldens; ref_*.npz, the reference renderer's records, are read by test_ref_golden.py
FILES = sorted(f for f in glob.glob(os.path.join(HERE, "golden", "*.npz")) if not os.path.basename(f).startswith("ref_"))
PAT = re.compile(r"(?P<name>[a-z_]+)_(?P<h>\d+)x(?P<w>\d+)_s(?P<spp>\d+)_d(?P<depth>\d+)_(?P<mode>post|raw)\.npz$")


def parse_case(path):
    m = PAT.search(os.path.basename(path))
    assert m, path
    kw = {"k_min": 64} if m["name"] == "bunny" else {}
    return m["name"], int(m["h"]), int(m["w"]), int(m["spp"]), int(m["depth"]), m["mode"] == "post", kw


def test_fixtures_exist():
    assert len(FILES) >= 8


@pytest.mark.parametrize("path", FILES, ids=[os.path.basename(f) for f in FILES])
def test_oracle_reproduces_golden(path):
    name, h, w, spp, depth, post, kw = parse_case(path)
    g = np.load(path)
    rgb, rays, states, total, _ = common.oracle_render(name, h, w, spp, depth, post=post, **kw)
    assert total == int(g["total"])
    assert np.array_equal(rays, g["rays"])
    assert np.array_equal(states, g["states"])
    if name == "birthday":  # libm acosf/atan2f feed a texel lookup: allow a last-bit texel flip
        assert common.rel_l2(rgb, g["rgb"]) <= 1e-3
    else:
        assert np.array_equal(rgb, g["rgb"])
