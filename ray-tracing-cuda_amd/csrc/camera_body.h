// rtmi_camera_rays and rtmi_sample_add: the render's primary-ray generator and the fold of a traced sample into the
// budget buffers, as kernels of their own (include/rtmi.h "camera rays" states the contract).  With
// rtmi_trace between them, once per sample, the two compose bit for bit to rtmi_render_budget.  Every binary32 + - * below
// is one operation: the file is compiled without contraction like the rest of the library.
#pragma once
// (included by kernels.hip inside namespace rtmi, after trace_helpers.h: rng_01, rng_range, unit3_rn)

enum : int32_t { PROJ_CAMERA = 0, PROJ_ORTHOGRAPHIC = 1, PROJ_EQUIRECT = 2, PROJ_FISHEYE = 3 };  // RTMI_PROJ_*

// The camera rides beside CameraDev, not in it: the render's argument block is sized by CameraDev.
struct CameraRaysArgs {
  FrameDev fr;
  CameraDev cam;
  V3 w;                    // the camera frame's third axis (kinds 1..3)
  int32_t kind;            // PROJ_*
  float fov;               // PROJ_FISHEYE: the full angle of the image circle
  uint32_t sample;
  const uint32_t *budget;  // nullable: every pixel has fr.spp
  uint32_t *states;        // RTMI_STATE_WORDS planes of uint32[items]
  float *origins, *dirs;   // float[items][3]
};
struct SampleAddArgs {
  FrameDev fr;
  uint32_t sample;
  const uint32_t *budget;        // nullable
  const float *radiance;         // float[items][3]
  const uint32_t *trace_counts;  // nullable
  float *sum, *sq;               // sq nullable
  uint32_t *samples, *ray_counts;  // ray_counts nullable
};

// Work item q takes part in sample `sample`: a pixel of the shard whose capped budget is not used up (rtmi_render_budget's
// b = min(budget[q], spp)).  The budget word of a padding item is not read.
__device__ __forceinline__ bool sample_active(const FrameDev &fr, const uint32_t *__restrict__ budget, uint32_t sample,
                                              int64_t q, int64_t *idx) {
  *idx = frame_pixel_of_rank(fr, fr.rank, q);
  if (*idx < 0) return false;
  const uint32_t spp = (uint32_t)fr.spp, b = budget ? budget[q] : spp;
  return sample < (b < spp ? b : spp);
}

// One lane per work item; the state planes are read and written plane-major, consecutive q on consecutive lanes.
__global__ __launch_bounds__(256) void camera_rays_kernel(CameraRaysArgs a) {
  const int64_t q = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const int64_t n = a.fr.items;
  if (q >= n) return;
  int64_t idx;
  V3 o = splat(0.f), d = splat(0.f);  // an inactive item: a ray rtmi_trace leaves out
  if (sample_active(a.fr, a.budget, a.sample, q, &idx)) {
    Rng rng;
    rng.d = a.states[0 * n + q], rng.v0 = a.states[1 * n + q], rng.v1 = a.states[2 * n + q];
    rng.v2 = a.states[3 * n + q], rng.v3 = a.states[4 * n + q], rng.v4 = a.states[5 * n + q];
    const int i = (int)(idx / a.fr.width), j = (int)(idx % a.fr.width);
    // The render's jitter (render_body.h, "ray_tracing.cu:68-74 + camera.cu:57-70"), restated: one function for both
    // changed the instructions of thirteen trace-loop kernels, so the render keeps its source.  Its
    // binary32 form for power-of-two frames is proven equal to this one bit for bit there
    // (tests/test_host_logic.py::test_jitter_in_binary32_for_power_of_two_frames), so the binary64 form serves every frame.
    const float r1 = rng_01(rng);
    const float r2 = rng_01(rng);
    double x = ((double)r1 + (double)j) / (double)a.fr.width;
    double y = ((double)r2 + (double)(a.fr.height - i)) / (double)a.fr.height;  // (quirk g1: H - i)
    x = 2 * x - 1, y = 2 * y - 1;
    x = (x + 1) / 2, y = (y + 1) / 2;
    const float xf = (float)x, yf = (float)y;
    const V3 target = a.cam.llc + xf * a.cam.horizontal + yf * a.cam.vertical;
    o = a.cam.position;
    if (a.kind == PROJ_CAMERA) {
      if (a.cam.defocus) {  // camera.cu:63-65,74-77
        const float ox = rng_range(0.f, a.cam.lens_radius, rng);
        const float oy = rng_range(0.f, a.cam.lens_radius, rng);
        o = a.cam.position + a.cam.u * ox + a.cam.v * oy;
      }
      d = unit3_rn(target - o);  // RayAt's normalisation; Ray's constructor, the second, is rtmi_trace's
    } else if (a.kind == PROJ_ORTHOGRAPHIC) {
      o = target;
      d = unit3_rn(-a.w);
    } else {
      const double ux = a.cam.u.x, uy = a.cam.u.y, uz = a.cam.u.z, vx = a.cam.v.x, vy = a.cam.v.y, vz = a.cam.v.z;
      const double wx = a.w.x, wy = a.w.y, wz = a.w.z;
      double cu, cv, cw;  // D = cu u + cv v - cw w
      bool inside = true;
      if (a.kind == PROJ_EQUIRECT) {
        const double phi = ((double)xf - 0.5) * 6.283185307179586, theta = ((double)yf - 0.5) * 3.141592653589793;
        cu = cos(theta) * sin(phi), cv = sin(theta), cw = cos(theta) * cos(phi);
      } else {  // PROJ_FISHEYE, equidistant
        const double sx = 2 * (double)xf - 1, sy = 2 * (double)yf - 1, r = sqrt(sx * sx + sy * sy);
        inside = !(r > 1);
        if (r == 0) {
          cu = 0, cv = 0, cw = 1;
        } else {
          const double t = r * (double)a.fov / 2;
          cu = sin(t) * (sx / r), cv = sin(t) * (sy / r), cw = cos(t);
        }
      }
      if (inside) {
        const V3 D = mk((float)((cu * ux + cv * vx) - cw * wx), (float)((cu * uy + cv * vy) - cw * wy),
                        (float)((cu * uz + cv * vz) - cw * wz));
        d = unit3_rn(D);
      }  // (outside the image circle: the zero direction of an active item, which has made its two draws)
    }
    a.states[0 * n + q] = rng.d, a.states[1 * n + q] = rng.v0, a.states[2 * n + q] = rng.v1;
    a.states[3 * n + q] = rng.v2, a.states[4 * n + q] = rng.v3, a.states[5 * n + q] = rng.v4;
  }
  a.origins[q * 3 + 0] = o.x, a.origins[q * 3 + 1] = o.y, a.origins[q * 3 + 2] = o.z;
  a.dirs[q * 3 + 0] = d.x, a.dirs[q * 3 + 1] = d.y, a.dirs[q * 3 + 2] = d.z;
}

// One lane per work item: the additions of rtmi_render_budget's write-back for one sample, each rounded on its own.
__global__ __launch_bounds__(256) void sample_add_kernel(SampleAddArgs a) {
  const int64_t q = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (q >= a.fr.items) return;
  int64_t idx;
  if (!sample_active(a.fr, a.budget, a.sample, q, &idx)) return;
#pragma unroll
  for (int c = 0; c < 3; c++) {
    const float x = a.radiance[q * 3 + c];
    a.sum[q * 3 + c] = __fadd_rn(a.sum[q * 3 + c], x);
    if (a.sq) a.sq[q * 3 + c] = __fadd_rn(a.sq[q * 3 + c], __fmul_rn(x, x));
  }
  a.samples[q] += 1u;
  if (a.ray_counts && a.trace_counts) a.ray_counts[q] += a.trace_counts[q];
}

hipError_t launch_camera_rays(const FrameDev &fr, const CameraDev &cam, const float w[3], int kind, float fov,
                              const uint32_t *d_budget, uint32_t sample, uint32_t *d_states, float *d_origins,
                              float *d_dirs, hipStream_t stream) {
  if (fr.items == 0) return hipSuccess;
  CameraRaysArgs a{};
  a.fr = fr, a.cam = cam, a.w = mk(w[0], w[1], w[2]), a.kind = kind, a.fov = fov, a.sample = sample;
  a.budget = d_budget, a.states = d_states, a.origins = d_origins, a.dirs = d_dirs;
  hipLaunchKernelGGL(camera_rays_kernel, dim3((unsigned)cdiv(fr.items, 256)), dim3(256), 0, stream, a);
  return hipGetLastError();
}

hipError_t launch_sample_add(const FrameDev &fr, const uint32_t *d_budget, uint32_t sample, const float *d_radiance,
                             const uint32_t *d_trace_counts, float *d_sum, float *d_sq, uint32_t *d_samples,
                             uint32_t *d_ray_counts, hipStream_t stream) {
  if (fr.items == 0) return hipSuccess;
  SampleAddArgs a{};
  a.fr = fr, a.sample = sample, a.budget = d_budget, a.radiance = d_radiance, a.trace_counts = d_trace_counts;
  a.sum = d_sum, a.sq = d_sq, a.samples = d_samples, a.ray_counts = d_ray_counts;
  hipLaunchKernelGGL(sample_add_kernel, dim3((unsigned)cdiv(fr.items, 256)), dim3(256), 0, stream, a);
  return hipGetLastError();
}
