"""The margin-check build's test hook stays out of the product.  tests/test_gpu_first_pass_status.py plants an
abandoned mesh search through RTMI_CHECK_PLANT_ABANDONED, which only librtmi_check1.so (-DRTMI_CHECK_MARGINS) reads:
the name must occur in that library and nowhere in librtmi.so.  No GPU involved."""
import os

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "ray-tracing-cuda_amd", "lib")
HOOK = b"RTMI_CHECK_PLANT_ABANDONED"


def test_the_plant_hook_is_in_the_check_build_only():
    check = os.path.join(LIB, "librtmi_check1.so")
    assert os.path.exists(check), "librtmi_check1.so missing: __graft_entry__.build() builds it"
    with open(check, "rb") as f:
        assert HOOK in f.read()
    with open(os.path.join(LIB, "librtmi.so"), "rb") as f:
        assert HOOK not in f.read()
