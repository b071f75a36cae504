"""The camera-ray entries from C: a C99 translation unit that includes rtmi.h, takes the addresses of rtmi_camera_rays and
rtmi_sample_add and calls both far enough to be refused compiles with gcc and links against librtmi.so.  No GPU involved."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "ray-tracing-cuda_amd", "lib")

C_PROG = r'''
#include <stdio.h>
#include <string.h>
#include "rtmi.h"
typedef int (*rays_fn)(const rtmi_scene *, const rtmi_frame *, const rtmi_projection *, const uint32_t *, uint32_t, void *,
                       float *, float *, void *);
typedef int (*add_fn)(const rtmi_frame *, const uint32_t *, uint32_t, const float *, const uint32_t *, float *, float *,
                      uint32_t *, uint32_t *, void *);
int main(void) {
  rays_fn rays = &rtmi_camera_rays;
  add_fn add = &rtmi_sample_add;
  rtmi_projection p = {sizeof(rtmi_projection), RTMI_PROJ_FISHEYE, 3.0f, 0};
  rtmi_frame f = {20, 28, 2, 10, 0, 0, 1};
  float eye[3] = {0, 0, 1}, at[3] = {0, 0, -1}, up[3] = {0, 1, 0}, x[3] = {0, 0, 0};
  uint32_t w[6] = {0, 0, 0, 0, 0, 0};
  rtmi_scene *s = rtmi_scene_create();
  if (sizeof(rtmi_projection) != 16) return 1;
  if (rtmi_camera_pinhole(s, eye, at, up, 1.0, 1.4) != RTMI_OK) return 2;
  if (rays(s, &f, &p, NULL, 0, w, x, x, NULL) != RTMI_ERR_INVALID || !strstr(rtmi_last_error(), "committed")) return 3;
  p.kind = 7;
  if (rays(s, &f, &p, NULL, 0, w, x, x, NULL) != RTMI_ERR_INVALID || !strstr(rtmi_last_error(), "kind")) return 4;
  if (rays(s, &f, NULL, NULL, 0, NULL, x, x, NULL) != RTMI_ERR_INVALID) return 5;
  if (add(&f, NULL, 0, NULL, NULL, x, NULL, w, NULL, NULL) != RTMI_ERR_INVALID || !strstr(rtmi_last_error(), "null")) return 6;
  rtmi_scene_destroy(s);
  printf("camera-rays abi ok\n");
  return 0;
}
'''


def test_camera_ray_entries_link_from_c99(tmp_path):
    src = tmp_path / "rays.c"
    src.write_text(C_PROG)
    exe = tmp_path / "rays"
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-pedantic", "-I", os.path.join(ROOT, "include"), str(src),
                    "-L", LIB, "-lrtmi", "-Wl,-rpath," + LIB, "-Wl,-rpath,/opt/rocm/lib", "-o", str(exe)], check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, (r.returncode, r.stdout, r.stderr)
    assert "camera-rays abi ok" in r.stdout
