// What the wavefront entries share as __device__ functions, one definition each for kernels.hip (rtmi_path_compact,
// rtmi_path_fold, rtmi_camera_rays) and advance.hip (rtmi_path_advance): "live", the fold of a path's layers, and the
// camera ray of a pixel's next sample.  No trace-loop kernel calls any of them (render_body.h and query_body.h keep their
// own source: DESIGN.md 2.10, 2.12 say what one function for both did to them); finite3 alone is theirs too, and lies
// here so that both translation units have it.  Every binary32 + - * below is one operation: both units are compiled
// without contraction.
#pragma once
// (included inside namespace rtmi, after trace_helpers.h: rng_01, unit3_rn; xorwow.h: rng_range)
#include "path_list.h"  // the candidates of a list and their rule

__device__ __forceinline__ bool finite3(V3 v) {
  return __builtin_isfinite(v.x) && __builtin_isfinite(v.y) && __builtin_isfinite(v.z);
}

// Whether a step would step the ray (ro, rd): finite, and a direction that Ray's constructor (ray.cu:8-10) normalises to a
// finite non-zero vector.  A RESTATEMENT of the predicate in render_body.h's take_item, line for line: with one
// __device__ function called from both sites, all eight trace_kernel<F> and all eight bounce_kernel<F> compiled to other
// instructions (and bounce_kernel<23> spilled four more SGPRs), and the existing kernels are not this feature's to
// change.  tests/test_gpu_bounce_list.py holds the two to each other: a compaction's count is the next step's d_work[1].
__device__ __forceinline__ bool live_ray(V3 ro, V3 rd) {
  bool live = finite3(ro) && finite3(rd) && (rd.x != 0.f || rd.y != 0.f || rd.z != 0.f);
  V3 nd = splat(0.f);
  if (live) nd = unit3_rn(rd);
  live = live && finite3(nd) && (nd.x != 0.f || nd.y != 0.f || nd.z != 0.f);
  return live;
}

// Trace's return expression (ray_tracing.cu:50-52) over layers 0 .. c - 1 of path q in the stacks float[.][n][3]
// (rtmi_path_fold states the rule): `ended` (the path's direction is the zero vector) starts from E[c-1], else from 0;
// product and sum each rounded on their own.  c <= the stacks' layers; c <= 0 reads nothing.
__device__ __forceinline__ V3 fold_layers(const float *__restrict__ emitted, const float *__restrict__ attenuation, int64_t n,
                                          int64_t q, int c, bool ended) {
  int k = c - 1;
  V3 r = splat(0.f);
  if (k >= 0 && ended) {  // the path ended in layer k
    const float *e = emitted + ((int64_t)k * n + q) * 3;
    r = mk(e[0], e[1], e[2]);
    k--;
  }
  for (; k >= 0; k--) {
    const float *e = emitted + ((int64_t)k * n + q) * 3, *a = attenuation + ((int64_t)k * n + q) * 3;
    r = mk(__fadd_rn(e[0], __fmul_rn(a[0], r.x)), __fadd_rn(e[1], __fmul_rn(a[1], r.y)), __fadd_rn(e[2], __fmul_rn(a[2], r.z)));
  }
  return r;
}

enum : int32_t { PROJ_CAMERA = 0, PROJ_ORTHOGRAPHIC = 1, PROJ_EQUIRECT = 2, PROJ_FISHEYE = 3 };  // RTMI_PROJ_*

// The camera beside its projection, as rtmi_camera_rays and rtmi_path_advance pass them by value.  The projection rides
// beside CameraDev, not in it: the render's argument block is sized by CameraDev.
struct CameraProj {
  CameraDev cam;
  V3 w;          // the camera frame's third axis (kinds 1..3)
  int32_t kind;  // PROJ_*
  float fov;     // PROJ_FISHEYE: the full angle of the image circle
};

// The ray of the next sample of pixel idx of the frame, drawn from rng (advanced by the two jitter draws and, for a defocus
// camera of kind CAMERA, the two lens draws); the direction normalised once.  A fisheye ray outside the image circle has
// made its two draws and gets the zero direction.
__device__ __forceinline__ void camera_ray(const FrameDev &fr, const CameraProj &p, int64_t idx, Rng &rng, V3 &o, V3 &d) {
  const CameraDev &cam = p.cam;
  d = splat(0.f);
  const int i = (int)(idx / fr.width), j = (int)(idx % fr.width);
  // The render's jitter (render_body.h, "ray_tracing.cu:68-74 + camera.cu:57-70"), restated: one function for both
  // changed the instructions of thirteen trace-loop kernels, so the render keeps its source.  Its
  // binary32 form for power-of-two frames is proven equal to this one bit for bit there
  // (tests/test_host_logic.py::test_jitter_in_binary32_for_power_of_two_frames), so the binary64 form serves every frame.
  const float r1 = rng_01(rng);
  const float r2 = rng_01(rng);
  double x = ((double)r1 + (double)j) / (double)fr.width;
  double y = ((double)r2 + (double)(fr.height - i)) / (double)fr.height;  // (quirk g1: H - i)
  x = 2 * x - 1, y = 2 * y - 1;
  x = (x + 1) / 2, y = (y + 1) / 2;
  const float xf = (float)x, yf = (float)y;
  const V3 target = cam.llc + xf * cam.horizontal + yf * cam.vertical;
  o = cam.position;
  if (p.kind == PROJ_CAMERA) {
    if (cam.defocus) {  // camera.cu:63-65,74-77
      const float ox = rng_range(0.f, cam.lens_radius, rng);
      const float oy = rng_range(0.f, cam.lens_radius, rng);
      o = cam.position + cam.u * ox + cam.v * oy;
    }
    d = unit3_rn(target - o);  // RayAt's normalisation; Ray's constructor, the second, is rtmi_trace's
  } else if (p.kind == PROJ_ORTHOGRAPHIC) {
    o = target;
    d = unit3_rn(-p.w);
  } else {
    const double ux = cam.u.x, uy = cam.u.y, uz = cam.u.z, vx = cam.v.x, vy = cam.v.y, vz = cam.v.z;
    const double wx = p.w.x, wy = p.w.y, wz = p.w.z;
    double cu, cv, cw;  // D = cu u + cv v - cw w
    bool inside = true;
    if (p.kind == PROJ_EQUIRECT) {
      const double phi = ((double)xf - 0.5) * 6.283185307179586, theta = ((double)yf - 0.5) * 3.141592653589793;
      cu = cos(theta) * sin(phi), cv = sin(theta), cw = cos(theta) * cos(phi);
    } else {  // PROJ_FISHEYE, equidistant
      const double sx = 2 * (double)xf - 1, sy = 2 * (double)yf - 1, r = sqrt(sx * sx + sy * sy);
      inside = !(r > 1);
      if (r == 0) {
        cu = 0, cv = 0, cw = 1;
      } else {
        const double t = r * (double)p.fov / 2;
        cu = sin(t) * (sx / r), cv = sin(t) * (sy / r), cw = cos(t);
      }
    }
    if (inside) {
      const V3 D = mk((float)((cu * ux + cv * vx) - cw * wx), (float)((cu * uy + cv * vy) - cw * wy),
                      (float)((cu * uz + cv * vz) - cw * wz));
      d = unit3_rn(D);
    }  // (outside the image circle: the zero direction of an active item, which has made its two draws)
  }
}
