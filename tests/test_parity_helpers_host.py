"""The suite's comparator and its RNG-state mapping (tests/parity.py) on synthetic frames, and the rule that keeps the
helpers where they are: no file under tests/ or tools/ imports a test module.  No GPU involved, no scene built."""
import ast
import glob
import os

import numpy as np
import pytest

import rtmi
from parity import Frame, assert_same_frame, bits, same, states_rowmajor

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
H, W = 2, 3


def frame(**change):
    rng = np.random.default_rng(1)
    f = Frame(rng.random((H, W, 3)).astype(np.float32), rng.integers(1, 50, (H, W)).astype(np.uint32),
              rng.integers(0, 1 << 32, (H * W, 6), dtype=np.uint64).astype(np.uint32), 777, None)
    return f._replace(**change)


def flipped(a, index, bit=1):
    a = a.copy()
    a.view(np.uint32)[index] ^= np.uint32(bit)
    return a


def test_identical_frames_pass():
    assert_same_frame(frame(), frame(), "identical")
    assert_same_frame(frame(), frame(), "identical", nan_ok=True)
    assert_same_frame(frame(mode={"fast_path": 1}), frame(states=None), "no states to compare, the mode is not compared")


ONE = frame()
DIFFERENT = {
    "total off by one": dict(total=ONE.total + 1),
    "one count off by one": dict(counts=ONE.counts + (np.arange(H * W).reshape(H, W) == 4).astype(np.uint32)),
    "one state bit": dict(states=flipped(ONE.states, (3, 5), 1 << 17)),
    "lowest bit of one image word": dict(image=flipped(ONE.image, (1, 2, 0))),
    "shape": dict(image=ONE.image.reshape(W, H, 3)),
    "counts shape": dict(counts=ONE.counts.reshape(W, H)),
}


@pytest.mark.parametrize("what", sorted(DIFFERENT))
@pytest.mark.parametrize("nan_ok", [False, True])
def test_one_difference_at_a_time_is_seen(what, nan_ok):
    with pytest.raises(AssertionError, match="frame under test"):
        assert_same_frame(frame(**DIFFERENT[what]), frame(), "frame under test", nan_ok=nan_ok)


@pytest.mark.parametrize("nan_ok", [False, True])
def test_zeros_of_either_sign_differ(nan_ok):
    plus, minus = ONE.image.copy(), ONE.image.copy()
    plus[0, 1, 2], minus[0, 1, 2] = 0.0, -0.0
    assert np.array_equal(plus, minus) and not same(plus, minus)  # equal by value, not by bits
    with pytest.raises(AssertionError, match="1 image words differ"):
        assert_same_frame(frame(image=minus), frame(image=plus), "zeros", nan_ok=nan_ok)


def test_nan_in_the_reference():
    nan = ONE.image.copy()
    nan[1, 0, 1] = np.nan
    with pytest.raises(AssertionError, match="NaN"):
        assert_same_frame(frame(image=nan), frame(image=nan), "NaN where none may be")
    assert_same_frame(frame(image=nan), frame(image=nan), "the same NaN", nan_ok=True)
    elsewhere = ONE.image.copy()
    elsewhere[0, 0, 0] = np.nan
    with pytest.raises(AssertionError, match="NaNs at"):
        assert_same_frame(frame(image=elsewhere), frame(image=nan), "NaNs at different positions", nan_ok=True)
    with pytest.raises(AssertionError, match="NaNs at"):
        assert_same_frame(frame(), frame(image=nan), "a NaN against a number", nan_ok=True)
    # beside equal NaNs every other word still counts
    with pytest.raises(AssertionError, match="1 image words differ"):
        assert_same_frame(frame(image=flipped(nan, (0, 2, 2))), frame(image=nan), "one bit beside a NaN", nan_ok=True)


def test_bits_and_same():
    assert bits(np.float32(1.0))[0] == 0x3F800000 and bits(1.0)[0] == 0x3F800000  # binary64 is rounded to binary32 first
    assert bits(np.array([7, 1 << 31], np.uint32)).tolist() == [7, 1 << 31] and bits(np.array([-1], np.int32))[0] == 0xFFFFFFFF
    assert same(np.zeros(3, np.float32), np.zeros(3, np.float32)) and not same(np.zeros(3, np.float32), np.zeros((3, 1), np.float32))
    assert same(np.float32([np.nan]), np.float32([np.nan])) and not same(np.float32([0.0]), np.float32([-0.0]))


@pytest.mark.parametrize("world", [1, 3])
def test_states_rowmajor_on_a_ragged_frame(world):
    """20 x 28: tiles of 8 x 8 leave padding items in every rank's planes.  Each pixel's six words are planted at its
    work item, every padding item holds a value no pixel has: each pixel comes back at its row-major index."""
    h, w = 20, 28
    planes, seen = [], 0
    for r in range(world):
        pm = rtmi.pixel_map(rtmi.make_frame(h, w, 1, rank=r, world_size=world))
        assert (pm < 0).any(), "the frame is ragged: there are padding items"
        st = np.full((6, len(pm)), 0xDEADBEEF, dtype=np.uint32)
        ok = pm >= 0
        st[:, ok] = pm[ok][None, :] * 8 + np.arange(6)[:, None] + 1
        seen += ok.sum()
        planes.append(st.view(np.int32))
    assert seen == h * w
    got = states_rowmajor(planes, h, w, world)
    assert got.shape == (h * w, 6) and got.dtype == np.uint32
    assert np.array_equal(got, np.arange(h * w, dtype=np.uint32)[:, None] * 8 + np.arange(6, dtype=np.uint32)[None, :] + 1)


def imported_modules(path):
    for node in ast.walk(ast.parse(open(path).read(), path)):
        if isinstance(node, ast.Import):
            for a in node.names:
                yield a.name
        elif isinstance(node, ast.ImportFrom) and node.module:
            yield node.module


def test_no_file_imports_a_test_module():
    """Shared code lives in helper modules (parity, querylib, budgetlib, filter_rules, abi_host, worlds, ...): importing
    it from a test module runs that module's setup and ties unrelated files to its names."""
    files = glob.glob(os.path.join(ROOT, "tests", "*.py")) + glob.glob(os.path.join(ROOT, "tools", "**", "*.py"), recursive=True)
    assert len(files) > 100
    bad = [(os.path.relpath(f, ROOT), m) for f in sorted(files) for m in imported_modules(f) if m.split(".")[-1].startswith("test_")]
    assert not bad, bad
