// rtmi_camera_rays and rtmi_sample_add: the render's primary-ray generator and the fold of a traced sample into the
// budget buffers, as kernels of their own (include/rtmi.h "camera rays" states the contract).  With
// rtmi_trace between them, once per sample, the two compose bit for bit to rtmi_render_budget.  Every binary32 + - * below
// is one operation: the file is compiled without contraction like the rest of the library.
#pragma once
// (included by kernels.hip inside namespace rtmi, after path_shared.h: camera_ray)

// The camera rides beside CameraDev, not in it (path_shared.h: CameraProj, PROJ_*).
struct CameraRaysArgs {
  FrameDev fr;
  CameraProj proj;
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
    camera_ray(a.fr, a.proj, idx, rng, o, d);  // (path_shared.h: rtmi_path_advance makes its rays by the same function)
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
  a.fr = fr, a.proj.cam = cam, a.proj.w = mk(w[0], w[1], w[2]), a.proj.kind = kind, a.proj.fov = fov, a.sample = sample;
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
