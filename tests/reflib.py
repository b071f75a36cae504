"""ctypes binding of the reference renderer built for the CPU (oracle/_ref/libref.so: the reference's own translation
units compiled by oracle/Makefile against oracle/refshim/, behind the C ABI of oracle/ref_harness.cc).

TEST INFRASTRUCTURE ONLY, and only on a machine that has the reference checkout or a tree in which the library was
built: ``available()`` says whether it is there, and the tests that need it skip with ``SKIP_REASON`` otherwise.
"""
import ctypes as C
import os
import subprocess

import numpy as np

from oraclelib import _TRANSFORM, _f3, _fp

_ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_ORACLE_DIR = os.path.join(_ROOT, "oracle")
LIB_PATH = os.path.join(_ORACLE_DIR, "_ref", "libref.so")
SKIP_REASON = ("oracle/_ref/libref.so is absent and there is no reference checkout to build it from "
               "(make -C oracle _ref/libref.so REF=<checkout>)")
DEPTH = 10  # TRACE_DEPTH_LIMIT, a compile-time constant of the reference
K_MIN = 2048  # BVHNode::kMin, likewise

_u32p = C.POINTER(C.c_uint32)


_made = []


def available():
    """True if the library can be loaded.  oracle/Makefile builds it where its REF (the reference checkout) exists and
    says so where it does not; make is a no-op when the library is up to date."""
    if not _made:
        _made.append(subprocess.run(["make", "-C", _ORACLE_DIR, "_ref/libref.so"], capture_output=True, text=True))
        if _made[0].returncode != 0:
            raise RuntimeError("building oracle/_ref/libref.so failed:\n" + _made[0].stdout[-2000:] + _made[0].stderr[-4000:])
    return os.path.exists(LIB_PATH)


_lib = None


def lib():
    global _lib
    if _lib is None:
        assert available(), SKIP_REASON
        L = C.CDLL(LIB_PATH)
        fp = C.POINTER(C.c_float)
        L.ref_scene_new.restype = C.c_void_p
        L.ref_scene_free.argtypes = [C.c_void_p]
        L.ref_constant_texture.argtypes = [C.c_void_p, fp]
        L.ref_image_texture.argtypes = [C.c_void_p, C.POINTER(C.c_uint8), C.c_int, C.c_int]
        L.ref_lambertian.argtypes = [C.c_void_p, fp]
        L.ref_lambertian_tex.argtypes = [C.c_void_p, C.c_int]
        L.ref_metal.argtypes = [C.c_void_p, fp, C.c_float]
        L.ref_dielectric.argtypes = [C.c_void_p, fp, C.c_double]
        L.ref_diffuse_light.argtypes = [C.c_void_p, C.c_int]
        L.ref_add_sphere.argtypes = [C.c_void_p, fp, C.c_double, C.c_int]
        L.ref_add_triangle.argtypes = [C.c_void_p, fp, C.c_int]
        L.ref_add_parallelogram.argtypes = [C.c_void_p, fp, C.c_int]
        L.ref_add_parallelepiped.argtypes = [C.c_void_p, fp, C.c_int]
        L.ref_add_parallelepiped_lengths.argtypes = [C.c_void_p, fp, C.c_int, _TRANSFORM, C.c_void_p]
        L.ref_add_sky.argtypes = [C.c_void_p]
        L.ref_list_begin.argtypes = [C.c_void_p]
        L.ref_list_end.argtypes = [C.c_void_p]
        L.ref_add_bvh.argtypes = [C.c_void_p, fp, fp, C.c_int, C.c_int]
        L.ref_camera_pinhole.argtypes = [C.c_void_p, fp, fp, fp, C.c_double, C.c_double]
        L.ref_camera_defocus.argtypes = [C.c_void_p, fp, fp, fp, C.c_double, C.c_double, C.c_double, C.c_double]
        L.ref_camera_raw.argtypes = [C.c_void_p, fp, fp, fp, fp]
        L.ref_camera_get.argtypes = [C.c_void_p, fp]
        L.ref_rng_init.argtypes = [C.c_uint64, _u32p, C.c_int64]
        L.ref_random_float.argtypes = [C.c_float, C.c_float, _u32p]
        L.ref_random_float.restype = C.c_float
        L.ref_get_workload.argtypes = [C.c_int, C.c_int, C.c_int]
        L.ref_probe_hit.argtypes = [C.c_void_p, fp, fp, C.c_double, C.c_double, C.POINTER(C.c_double),
                                    C.POINTER(C.c_int)]
        L.ref_probe_scatter.argtypes = [C.c_void_p, C.c_int, fp, fp, C.c_double, C.c_double, C.c_double, fp, _u32p, fp]
        L.ref_probe_camera_ray.argtypes = [C.c_void_p, C.c_double, C.c_double, _u32p, fp]
        L.ref_render.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_uint64, _u32p, fp, _u32p, _u32p]
        L.ref_render.restype = C.c_uint64
        _lib = L
    return _lib


def rng_init(seed, n):
    """(n, 6) uint32 compact states {d, v0..v4} from the reference's CudaRandomInit."""
    st = np.zeros((n, 6), dtype=np.uint32)
    lib().ref_rng_init(C.c_uint64(seed), st.ctypes.data_as(_u32p), n)
    return st


class RefBuilder:
    """The builder protocol of rtmi/scenes.py over the reference's own constructors."""

    def __init__(self, seed=0):
        self.L = lib()
        self.h = C.c_void_p(self.L.ref_scene_new())
        self._keep = []
        self.seed = seed
        self.state0 = rng_init(seed, 1)[0].copy()  # pixel 0's stream: scenes/spheres.cu draws the layout from it

    def __del__(self):
        try:
            self.L.ref_scene_free(self.h)
        except Exception:
            pass

    def constant_texture(self, rgb):
        return self.L.ref_constant_texture(self.h, _fp(_f3(rgb)))

    def image_texture(self, rgba):
        rgba = np.ascontiguousarray(rgba, dtype=np.uint8)
        return self.L.ref_image_texture(self.h, rgba.ctypes.data_as(C.POINTER(C.c_uint8)), rgba.shape[0],
                                        rgba.shape[1])

    def lambertian(self, rgb):
        return self.L.ref_lambertian(self.h, _fp(_f3(rgb)))

    def lambertian_tex(self, tex):
        return self.L.ref_lambertian_tex(self.h, tex)

    def metal(self, rgb, fuzz):
        return self.L.ref_metal(self.h, _fp(_f3(rgb)), C.c_float(float(fuzz)))

    def dielectric(self, rgb, index):
        return self.L.ref_dielectric(self.h, _fp(_f3(rgb)), float(index))

    def diffuse_light(self, tex):
        return self.L.ref_diffuse_light(self.h, tex)

    def sphere(self, c, r, mat):
        assert self.L.ref_add_sphere(self.h, _fp(_f3(c)), float(r), mat) == 0

    def triangle(self, p, mat):
        assert self.L.ref_add_triangle(self.h, _fp(_f3(p)), mat) == 0

    def parallelogram(self, p, mat):
        assert self.L.ref_add_parallelogram(self.h, _fp(_f3(p)), mat) == 0

    def parallelepiped(self, p, mat):
        assert self.L.ref_add_parallelepiped(self.h, _fp(_f3(p)), mat) == 0

    def parallelepiped_lengths(self, lengths, mat, transform):
        def cb(pin, pout, _user):
            o = transform(np.array([pin[0], pin[1], pin[2]], dtype=np.float32))
            pout[0], pout[1], pout[2] = float(o[0]), float(o[1]), float(o[2])

        cfn = _TRANSFORM(cb)
        self._keep.append(cfn)
        assert self.L.ref_add_parallelepiped_lengths(self.h, _fp(_f3(lengths)), mat, cfn, None) == 0

    def sky(self):
        assert self.L.ref_add_sky(self.h) == 0

    def list_begin(self):
        assert self.L.ref_list_begin(self.h) == 0

    def list_end(self):
        assert self.L.ref_list_end(self.h) == 0

    def bvh(self, faces, mat, uvs=None, k_min=K_MIN):
        assert k_min == K_MIN, "the reference's leaf size is a compile-time %d" % K_MIN
        faces = np.ascontiguousarray(faces, dtype=np.float32).reshape(-1, 9)
        uvp = None
        if uvs is not None:
            uvs = np.ascontiguousarray(uvs, dtype=np.float32).reshape(-1, 6)
            uvp = _fp(uvs)
        assert self.L.ref_add_bvh(self.h, _fp(faces), uvp, faces.shape[0], -1 if mat is None else mat) == 0

    def camera_pinhole(self, pos, look_at, up, fov, aspect):
        self.L.ref_camera_pinhole(self.h, _fp(_f3(pos)), _fp(_f3(look_at)), _fp(_f3(up)), float(fov), float(aspect))

    def camera_defocus(self, pos, look_at, up, fov, aspect, aperture, focus):
        self.L.ref_camera_defocus(self.h, _fp(_f3(pos)), _fp(_f3(look_at)), _fp(_f3(up)), float(fov), float(aspect),
                                  float(aperture), float(focus))

    def camera_raw(self, pos, llc, horiz, vert):
        self.L.ref_camera_raw(self.h, _fp(_f3(pos)), _fp(_f3(llc)), _fp(_f3(horiz)), _fp(_f3(vert)))

    def camera_get(self):
        """(4, 3): position, lower-left corner, horizontal, vertical (the oracle's camera_get()[:4])."""
        out = np.zeros(12, dtype=np.float32)
        self.L.ref_camera_get(self.h, _fp(out))
        return out.reshape(4, 3)

    def random_float(self, mn, mx):
        return np.float32(self.L.ref_random_float(C.c_float(float(np.float32(mn))), C.c_float(float(np.float32(mx))),
                                                  self.state0.ctypes.data_as(_u32p)))

    def probe_hit(self, o, d, t_from=1e-3, t_to=float("inf")):
        out = (C.c_double * 6)()
        mat = C.c_int(-1)
        hit = self.L.ref_probe_hit(self.h, _fp(_f3(o)), _fp(_f3(d)), t_from, t_to, out, C.byref(mat))
        return bool(hit), np.array(list(out)), mat.value

    def probe_scatter_ex(self, mat, o, d, t, u, v, n, state):
        out = np.zeros(12, dtype=np.float32)
        sc = self.L.ref_probe_scatter(self.h, mat, _fp(_f3(o)), _fp(_f3(d)), float(t), float(u), float(v), _fp(_f3(n)),
                                      state.ctypes.data_as(_u32p), _fp(out))
        return bool(sc), out

    def probe_camera_ray(self, x, y, state=None):
        if state is None:
            state = np.zeros(6, dtype=np.uint32)
        out = np.zeros(6, dtype=np.float32)
        self.L.ref_probe_camera_ray(self.h, float(x), float(y), state.ctypes.data_as(_u32p), _fp(out))
        return out

    def render(self, height, width, spp, max_depth=DEPTH, post=True):
        """Returns (rgb (H,W,3) float32, rays (H,W) uint32, states (H*W,6) uint32, total_rays), like
        OracleBuilder.render; the depth limit is the reference's own 10."""
        assert max_depth == DEPTH, "the reference's depth limit is a compile-time %d" % DEPTH
        n = height * width
        rgb = np.zeros((n, 3), dtype=np.float32)
        rays = np.zeros(n, dtype=np.uint32)
        states = np.zeros((n, 6), dtype=np.uint32)
        total = self.L.ref_render(self.h, height, width, spp, 1 if post else 0, C.c_uint64(self.seed),
                                  self.state0.ctypes.data_as(_u32p), _fp(rgb), rays.ctypes.data_as(_u32p),
                                  states.ctypes.data_as(_u32p))
        return rgb.reshape(height, width, 3), rays.reshape(height, width), states, int(total)
