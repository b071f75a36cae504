"""The raw camera of tests/test_gpu_deferred_normalise.py's slow-form case, restated in numpy.

The trace loop normalises new camera rays and the Lambertian directions of the iteration before in ONE call of
unit3_rn_twice (render_body.h), whose wave-uniform domain check 2^-100 <= v.v < 2^100 sends the whole wave -- the
Lambertian lanes included -- through the IEEE forms when one lane fails it.  A Lambertian S + n cannot be steered out
of the domain, a camera ray can: camera_raw with position o, lower-left corner o and spans (A, 0, 0), (0, A, 0) makes
target - origin = (x A, y A, 0) for the frame coordinates x in (c / W, (c + 1) / W] of column c and
y in ((H - r) / H, (H - r + 1) / H] of row r (render_body.h: xf, yf; the jitter is curand_uniform's (0, 1]).  v.v grows
with x and y, so its largest values sit in the pixel of the last column and the first row, and A is chosen so that
2^100 falls INSIDE that pixel's range: some of its samples leave the domain, no sample of any other pixel does.
"""
import numpy as np

from worlds import F32, SIDE, slow_camera

DOMAIN_HI = F32(2.0 ** 100)


def dot_of_camera_ray(col, row, r1, r2, side=SIDE):
    """v.v of target - origin in binary32, as the kernel and camera.cu:57-70 form it, for jitter draws r1, r2."""
    pos, llc, hor, ver = slow_camera()
    inv = F32(1.0 / side)
    xf = F32(F32(r1) + F32(col)) * inv
    yf = F32(F32(r2) + F32(side - row)) * inv
    target = ((llc + xf * hor).astype(F32) + yf * ver).astype(F32)
    v = (target - pos).astype(F32)
    return F32(F32(v[0] * v[0] + v[1] * v[1]) + v[2] * v[2])


LO, HI = F32(2.0 ** -33), F32(1.0)  # the ends of curand_uniform's range


def test_only_the_corner_pixel_can_leave_the_domain():
    last = SIDE - 1
    for col in range(SIDE):
        for row in range(SIDE):
            if (col, row) == (last, 0):
                continue
            assert dot_of_camera_ray(col, row, HI, HI) < DOMAIN_HI, (col, row)  # its largest v.v
    assert dot_of_camera_ray(last, 0, HI, HI) >= DOMAIN_HI
    assert dot_of_camera_ray(last, 0, LO, LO) < DOMAIN_HI  # and not every sample of the corner pixel either
    assert dot_of_camera_ray(0, last, LO, LO) >= F32(2.0 ** -100)  # nothing near the lower end


def test_a_good_share_of_the_corner_pixel_is_beyond_it():
    """40 samples miss the slow form with probability (1 - share)^40: below 1e-7 for a share of a third."""
    rng = np.random.default_rng(5)
    draws = rng.random((4000, 2)).astype(F32)
    out = sum(dot_of_camera_ray(SIDE - 1, 0, a, b) >= DOMAIN_HI for a, b in draws)
    assert 0.33 < out / len(draws) < 0.45, out
