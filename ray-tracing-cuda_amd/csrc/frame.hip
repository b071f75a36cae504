// The kernels around a frame's buffers, one lane per work item: RNG seeding, tile scatter and post-process, the budget
// plan and the three resolves, the camera's primary rays and the fold of a traced sample (rtmi_camera_rays,
// rtmi_sample_add) -- and the arithmetic self-test.  A translation unit of its own: it takes the device helpers these are
// written in from trace_helpers.h and path_shared.h, and no kernel of another unit is compiled differently for it.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "kernels.h"

#include <cfloat>
#include <cmath>
#include "scene_dev.h"
#include "vec.h"
#include "xorwow.h"

namespace rtmi {

// ------------------------------------------------------------------ frame math
#include "frame_math.h"

int64_t frame_pixel_of(const FrameDev &fr, int rank, int64_t q) { return frame_pixel_of_rank(fr, rank, q); }

// ------------------------------------------------------------------ RNG init
// state(q) = seed scramble, then v <- A^(idx * 2^67) v, idx = global pixel index -- or, first >= 0 (rtmi_rng_init_n:
// fr.items states, no frame), idx = first + q.
// The jump matrix for bit k is wave-uniform -> scalar loads; lanes whose bit is
// clear keep their vector.
__global__ __launch_bounds__(256) void rng_init_kernel(uint64_t seed, FrameDev fr, int64_t first,
                                                        const uint32_t *__restrict__ jump,
                                                        uint32_t *__restrict__ states) {
  int64_t q = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (q >= fr.items) return;
  int64_t idx = first >= 0 ? first + q : frame_pixel_of_rank(fr, fr.rank, q);
  uint64_t sub = idx < 0 ? 0 : (uint64_t)idx;
  Rng s = rng_seed(seed);
  uint32_t v0 = s.v0, v1 = s.v1, v2 = s.v2, v3 = s.v3, v4 = s.v4;
  for (int k = 0; k < kJumpBits; k++) {
    if (!__any((sub >> k) != 0)) break;
    bool bit = (sub >> k) & 1;
    if (!__any(bit)) continue;
    const uint32_t *M = jump + (size_t)k * kJumpWords;
    uint32_t r0 = 0, r1 = 0, r2 = 0, r3 = 0, r4 = 0;
#pragma unroll 1
    for (int w = 0; w < 5; w++) {
      uint32_t word = w == 0 ? v0 : w == 1 ? v1 : w == 2 ? v2 : w == 3 ? v3 : v4;
#pragma unroll 4
      for (int b = 0; b < 32; b++) {
        uint32_t m = 0u - ((word >> b) & 1u);
        const uint32_t *row = M + (w * 32 + b) * 5;
        r0 ^= row[0] & m;
        r1 ^= row[1] & m;
        r2 ^= row[2] & m;
        r3 ^= row[3] & m;
        r4 ^= row[4] & m;
      }
    }
    if (bit) {
      v0 = r0, v1 = r1, v2 = r2, v3 = r3, v4 = r4;
    }
  }
  const int64_t n = fr.items;
  states[0 * n + q] = s.d;
  states[1 * n + q] = v0;
  states[2 * n + q] = v1;
  states[3 * n + q] = v2;
  states[4 * n + q] = v3;
  states[5 * n + q] = v4;
}

#include "trace_helpers.h"
#include "path_shared.h"

// ------------------------------------------------------------------ untile / post
template <typename E, int C>
__global__ __launch_bounds__(256) void untile_kernel(FrameDev fr, const E *__restrict__ tiles, E *__restrict__ image) {
  int64_t g = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  int64_t total = fr.items * fr.world;
  if (g >= total) return;
  int rank = (int)(g / fr.items);
  int64_t q = g % fr.items;
  int64_t idx = frame_pixel_of_rank(fr, rank, q);
  if (idx < 0) return;
#pragma unroll
  for (int c = 0; c < C; c++) image[idx * C + c] = tiles[g * C + c];
}

__global__ __launch_bounds__(256) void post_kernel(float *__restrict__ img, int64_t n, int spp) {
  int64_t g = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (g >= n) return;
  img[g] = sqrtf(clamp1(img[g] / (float)spp, 0.f, 1.f));  // utils.cu:127-128
}

// ------------------------------------------------------------------ self-test
// Runs every shortened operation against the expression it replaces on all 2^32 inputs:
// bad[0] rcp_rn(x) vs 1.0f / x inside rcp_rn's domain (must be 0), bad[1] outside it
// (informative), bad[2] rng_pm1_of(x) vs the reference's uniform(-1, 1) expression, bad[3]
// rng_01_of(x) vs uniform(0, 1) (both must be 0), bad[4] sqrt_rn_core(x) vs sqrtf(x) on its domain (must be 0),
// bad[5] div_rn_core vs a / l on 2^32 triples of sampler draws (must be 0), bad[6] the same with a single
// correction (informative).
__device__ __forceinline__ float ref_uniform(uint32_t x) { return (float)x * 2.3283064e-10f + 1.16415322e-10f; }
__device__ __forceinline__ float ref_range(float mn, float mx, uint32_t x) { return ref_uniform(x) * (mx - mn) + mn; }
__device__ __forceinline__ uint32_t selftest_mix(uint64_t &s) {  // splitmix64
  s += 0x9e3779b97f4a7c15ull;
  uint64_t z = s;
  z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ull;
  z = (z ^ (z >> 27)) * 0x94d049bb133111ebull;
  return (uint32_t)((z ^ (z >> 31)) >> 16);
}
__global__ __launch_bounds__(256) void arithmetic_selftest(unsigned long long *bad, float mn1, float mx1, float mn0,
                                                           float mx0) {
  const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
  unsigned long long in_domain = 0, outside = 0, pm1 = 0, u01 = 0, sq = 0, dv = 0, dv1 = 0;
  for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < (1ull << 32); i += stride) {
    const uint32_t bits = (uint32_t)i;
    const float x = __uint_as_float(bits);
    const float ref = 1.0f / x, got = rcp_rn(x);
    const bool same = __float_as_uint(ref) == __float_as_uint(got) || (ref != ref && got != got);
    const bool dom = fabsf(x) >= 0x1p-126f && fabsf(x) < RCP_RN_LIMIT;
    if (!same) {
      if (dom) in_domain++; else outside++;
    }
    // the range bounds arrive as kernel arguments so that the reference expression is
    // evaluated operation by operation, not folded at compile time
    if (__float_as_uint(ref_range(mn1, mx1, bits)) != __float_as_uint(rng_pm1_of(bits))) pm1++;
    if (__float_as_uint(ref_range(mn0, mx0, bits)) != __float_as_uint(rng_01_of(bits))) u01++;
    // sqrt_rn_core against sqrtf on its whole domain
    if (x >= SQRT_RN_LO && x < SQRT_RN_HI && __float_as_uint(sqrtf(x)) != __float_as_uint(sqrt_rn_core(x))) sq++;
  }
  // div_rn_core against the division on the Lambertian sampler's own operands (lambertian.cu:19-31): 2^32 triples
  // of draws, every eighth shrunk towards the corner (-1, -1, -1), every eighth towards the origin (tiny lengths)
  uint64_t st = 0x1234567ull + ((uint64_t)blockIdx.x * blockDim.x + threadIdx.x) * 0x632be59bd9b4e019ull;
  for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < (1ull << 32); i += stride) {
    uint32_t rx = selftest_mix(st), ry = selftest_mix(st), rz = selftest_mix(st);
    const uint32_t sh = selftest_mix(st);
    if ((i & 7) == 0) rx >>= (sh & 31), ry >>= ((sh >> 5) & 31), rz >>= ((sh >> 10) & 31);
    if ((i & 7) == 1)
      rx = 0x80000000u + (rx >> (8 + (sh & 15))), ry = 0x80000000u - (ry >> (8 + ((sh >> 4) & 15))),
      rz = 0x80000000u + (rz >> (8 + ((sh >> 8) & 15)));
    const float cx = rng_pm1_of(rx), cy = rng_pm1_of(ry), cz = rng_pm1_of(rz);
    const float sum = cx * cx + cy * cy + cz * cz;
    if (sum > BALL_S_MAX) continue;
    const float l = sqrtf(sum);
    if (!(l >= DIV3_RN_LO)) continue;
    const float y = rcp_rn(l);
    const float v[3] = {cx, cy, cz};
    for (int k = 0; k < 3; k++) {
      const float ref = v[k] / l;
      const float q0 = v[k] * y;
      if (__float_as_uint(ref) != __float_as_uint(div_rn_core(v[k], l, y))) dv++;
      if (__float_as_uint(ref) != __float_as_uint(__builtin_fmaf(__builtin_fmaf(-l, q0, v[k]), y, q0))) dv1++;
    }
  }
  if (in_domain) atomicAdd(&bad[0], in_domain);
  if (outside) atomicAdd(&bad[1], outside);
  if (pm1) atomicAdd(&bad[2], pm1);
  if (u01) atomicAdd(&bad[3], u01);
  if (sq) atomicAdd(&bad[4], sq);
  if (dv) atomicAdd(&bad[5], dv);
  if (dv1) atomicAdd(&bad[6], dv1);
}
hipError_t launch_arithmetic_selftest(unsigned long long *d_bad, hipStream_t stream) {
  hipLaunchKernelGGL(arithmetic_selftest, dim3(4096), dim3(256), 0, stream, d_bad, -1.f, 1.f, 0.f, 1.f);
  return hipGetLastError();
}
#ifdef RTMI_CHECK_MARGINS
__global__ void add_one_kernel(unsigned long long *word) { atomicAdd(word, 1ull); }
hipError_t launch_add_one(unsigned long long *d_word, hipStream_t stream) {
  hipLaunchKernelGGL(add_one_kernel, dim3(1), dim3(1), 0, stream, d_word);
  return hipGetLastError();
}
#endif

// ------------------------------------------------------------------ launchers
hipError_t launch_rng_init(uint64_t seed, const FrameDev &fr, const uint32_t *d_jump, uint32_t *d_states,
                           hipStream_t stream, int64_t first) {
  if (fr.items == 0) return hipSuccess;
  hipLaunchKernelGGL(rng_init_kernel, dim3((unsigned)cdiv(fr.items, 256)), dim3(256), 0, stream, seed, fr, first, d_jump,
                     d_states);
  return hipGetLastError();
}

hipError_t launch_untile(const FrameDev &fr, const float *d_tiles, float *d_image, hipStream_t stream) {
  int64_t total = fr.items * fr.world;
  if (total == 0) return hipSuccess;
  hipLaunchKernelGGL((untile_kernel<float, 3>), dim3((unsigned)cdiv(total, 256)), dim3(256), 0, stream, fr, d_tiles,
                     d_image);
  return hipGetLastError();
}

hipError_t launch_untile_u32(const FrameDev &fr, const uint32_t *d_tiles, uint32_t *d_image, hipStream_t stream) {
  int64_t total = fr.items * fr.world;
  if (total == 0) return hipSuccess;
  hipLaunchKernelGGL((untile_kernel<uint32_t, 1>), dim3((unsigned)cdiv(total, 256)), dim3(256), 0, stream, fr,
                     d_tiles, d_image);
  return hipGetLastError();
}

hipError_t launch_post(float *d_img, int64_t n, int spp, hipStream_t stream) {
  if (n == 0) return hipSuccess;
  hipLaunchKernelGGL(post_kernel, dim3((unsigned)cdiv(n, 256)), dim3(256), 0, stream, d_img, n, spp);
  return hipGetLastError();
}

// Per-pixel means of the feature sums (rtmi_resolve_features; include/rtmi.h states the rule): one lane per work item,
// every operation in binary32 and rounded on its own.  Null pointers skip their buffer (capi.hip checks the pairs).
__global__ __launch_bounds__(256) void resolve_features_kernel(FrameDev fr, FeatureBufs sums, const uint32_t *__restrict__ samples,
                                                                FeatureBufs out) {
  const int64_t q = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (q >= fr.items) return;
  const uint32_t n = frame_pixel_of_rank(fr, fr.rank, q) >= 0 ? samples[q] : 0u;
  const float nf = (float)n;
  V3 a = splat(0.f), nm = splat(0.f);
  float dp = 0.f, alpha = 0.f;
  if (n > 0u) {
    if (out.albedo) a = mk(sums.albedo[q * 3 + 0], sums.albedo[q * 3 + 1], sums.albedo[q * 3 + 2]) / nf;
    if (out.normal) nm = mk(sums.normal[q * 3 + 0], sums.normal[q * 3 + 1], sums.normal[q * 3 + 2]) / nf;
    if (out.depth || out.coverage) {
      const uint32_t c = sums.coverage[q];
      if (out.depth && c) dp = __fdiv_rn(sums.depth[q], (float)c);
      alpha = __fdiv_rn((float)c, nf);
    }
  }
  if (out.albedo) out.albedo[q * 3 + 0] = a.x, out.albedo[q * 3 + 1] = a.y, out.albedo[q * 3 + 2] = a.z;
  if (out.normal) out.normal[q * 3 + 0] = nm.x, out.normal[q * 3 + 1] = nm.y, out.normal[q * 3 + 2] = nm.z;
  if (out.depth) out.depth[q] = dp;
  if (out.coverage) out.coverage[q] = __float_as_uint(alpha);
}
hipError_t launch_resolve_features(const FrameDev &fr, const FeatureBufs &sums, const uint32_t *d_samples,
                                   const FeatureBufs &out, hipStream_t stream) {
  if (fr.items == 0) return hipSuccess;
  hipLaunchKernelGGL(resolve_features_kernel, dim3((unsigned)cdiv(fr.items, 256)), dim3(256), 0, stream, fr, sums, d_samples, out);
  return hipGetLastError();
}

// The stopping rule of include/rtmi.h (rtmi_budget_plan), operation by operation in binary32 (the file is compiled
// without contraction and with IEEE division; the intrinsics say so where it matters).  One lane per work item; the
// totals by a wave reduction and one atomic pair per wave.
__global__ __launch_bounds__(256) void budget_plan_kernel(FrameDev fr, uint32_t min_n, uint32_t max_n, uint32_t step, float tol,
                                                           float flr, const float *__restrict__ sum,
                                                           const float *__restrict__ sq, const uint32_t *__restrict__ samples,
                                                           uint32_t *__restrict__ budget, unsigned long long *__restrict__ totals) {
  const int64_t q = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  uint32_t b = 0u;
  if (q < fr.items) {
    if (frame_pixel_of_rank(fr, fr.rank, q) >= 0) {
      const uint32_t n = samples[q];
      if (n < min_n) {
        b = min_n - n;
      } else if (n < max_n) {
        const float nf = (float)n;
        const float tt = __fmul_rn(tol, tol), nnff = __fmul_rn(__fmul_rn(nf, nf), __fmul_rn(flr, flr));
        bool converged = true;
#pragma unroll
        for (int c = 0; c < 3; c++) {
          const float S = sum[q * 3 + c], Q = sq[q * 3 + c];
          const float ss = __fmul_rn(S, S);
          const float lhs = __fdiv_rn(__fsub_rn(__fmul_rn(nf, Q), ss), __fsub_rn(nf, 1.0f));
          const float rhs = __fmul_rn(tt, __fadd_rn(ss, nnff));
          converged = converged && (lhs <= rhs);  // (a NaN on either side: not converged)
        }
        if (!converged) b = step < max_n - n ? step : max_n - n;
      }
    }
    budget[q] = b;
  }
  unsigned long long live = b > 0u ? 1ull : 0ull, total = b;
  for (int off = 32; off > 0; off >>= 1) live += __shfl_down(live, off), total += __shfl_down(total, off);
  if ((threadIdx.x & 63) == 0 && total) {
    atomicAdd(&totals[0], live);
    atomicAdd(&totals[1], total);
  }
}
hipError_t launch_budget_plan(const FrameDev &fr, int min_samples, int max_samples, int step, float tolerance, float floor,
                              const float *d_sum, const float *d_sq, const uint32_t *d_samples, uint32_t *d_budget,
                              unsigned long long *d_totals, hipStream_t stream) {
  const hipError_t e = hipMemsetAsync(d_totals, 0, 2 * sizeof(unsigned long long), stream);
  if (e != hipSuccess || fr.items == 0) return e;
  hipLaunchKernelGGL(budget_plan_kernel, dim3((unsigned)cdiv(fr.items, 256)), dim3(256), 0, stream, fr, (uint32_t)min_samples,
                     (uint32_t)max_samples, (uint32_t)step, tolerance, floor, d_sum, d_sq, d_samples, d_budget, d_totals);
  return hipGetLastError();
}

// sum / n per pixel, then the render's own post-processing expressions (render_body.h: the write-back).
__global__ __launch_bounds__(256) void resolve_kernel(FrameDev fr, const float *__restrict__ sum,
                                                       const uint32_t *__restrict__ samples, int post,
                                                       float *__restrict__ tiles) {
  const int64_t q = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (q >= fr.items) return;
  V3 c = splat(0.f);
  const uint32_t n = frame_pixel_of_rank(fr, fr.rank, q) >= 0 ? samples[q] : 0u;
  if (n > 0u) {
    c = mk(sum[q * 3 + 0], sum[q * 3 + 1], sum[q * 3 + 2]) / (float)n;
    if (post) {
      c = mk(clamp1(c.x, 0.f, 1.f), clamp1(c.y, 0.f, 1.f), clamp1(c.z, 0.f, 1.f));
      c = mk(sqrtf(c.x), sqrtf(c.y), sqrtf(c.z));
    }
  }
  tiles[q * 3 + 0] = c.x, tiles[q * 3 + 1] = c.y, tiles[q * 3 + 2] = c.z;
}
hipError_t launch_resolve(const FrameDev &fr, const float *d_sum, const uint32_t *d_samples, int post, float *d_tiles,
                          hipStream_t stream) {
  if (fr.items == 0) return hipSuccess;
  hipLaunchKernelGGL(resolve_kernel, dim3((unsigned)cdiv(fr.items, 256)), dim3(256), 0, stream, fr, d_sum, d_samples, post,
                     d_tiles);
  return hipGetLastError();
}

// The variance of the pixel mean from the raw moments (rtmi_resolve_variance; include/rtmi.h states the rule), one lane per
// work item and every operation rounded on its own, as budget_plan_kernel's.
__global__ __launch_bounds__(256) void resolve_variance_kernel(FrameDev fr, const float *__restrict__ sum,
                                                                const float *__restrict__ sq,
                                                                const uint32_t *__restrict__ samples, float *__restrict__ var) {
  const int64_t q = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (q >= fr.items) return;
  const uint32_t n = frame_pixel_of_rank(fr, fr.rank, q) >= 0 ? samples[q] : 0u;
  const float nf = (float)n;
#pragma unroll
  for (int c = 0; c < 3; c++) {
    float out = 0.f;
    if (n == 1u) {
      const float S = sum[q * 3 + c];
      out = __fmul_rn(S, S);
    } else if (n >= 2u) {
      const float S = sum[q * 3 + c], Q = sq[q * 3 + c];
      const float cc = fmaxf(__fsub_rn(__fmul_rn(nf, Q), __fmul_rn(S, S)), 0.f);
      out = __fdiv_rn(cc, __fmul_rn(__fmul_rn(nf, nf), __fsub_rn(nf, 1.0f)));
    }
    var[q * 3 + c] = out;
  }
}
hipError_t launch_resolve_variance(const FrameDev &fr, const float *d_sum, const float *d_sq, const uint32_t *d_samples,
                                   float *d_var, hipStream_t stream) {
  if (fr.items == 0) return hipSuccess;
  hipLaunchKernelGGL(resolve_variance_kernel, dim3((unsigned)cdiv(fr.items, 256)), dim3(256), 0, stream, fr, d_sum, d_sq,
                     d_samples, d_var);
  return hipGetLastError();
}

// ------------------------------------------------------------------ camera rays (rtmi_camera_rays, rtmi_sample_add)
// The render's primary-ray generator and the fold of a traced sample into the budget buffers, as kernels of their own
// (include/rtmi.h "camera rays" states the contract).  With rtmi_trace between them, once per sample, the
// two compose bit for bit to rtmi_render_budget.  Every binary32 + - * below is one operation: the file is compiled
// without contraction like the rest of the library.

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

}  // namespace rtmi
