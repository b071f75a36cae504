"""Oracle vs the committed golden vectors (tests/golden/*.npz, made by make_golden.py):
pins the oracle's determinism across machines and compilers."""
import os

import numpy as np
import pytest

import common
from common import FILES, parse_case


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
