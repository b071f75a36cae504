// HIP kernels of the trace path for gfx950 (MI355X): RNG seeding, the persistent
// per-pixel trace loop, tile scatter and post-process.
//
// Shape of the trace kernel (DESIGN.md "Kernels"):
//   * persistent lanes: a lane owns ONE pixel at a time and walks its samples
//     serially (the cuRAND stream of a pixel is consumed in order, so samples of
//     a pixel cannot be spread over lanes without changing the image); when a
//     path ends the lane immediately regenerates the next camera ray, when the
//     pixel ends it pulls the next work item from a global queue
//     (wave-aggregated atomic), so every lane of a wave enters the intersection
//     loop on every iteration;
//   * closest hit walks the world list in list order with wave-uniform control
//     flow: every lane tests the same primitive, whose record arrives in SGPRs
//     through scalar loads (s_load_dwordx8/x16, scalar cache) — no per-lane
//     geometry traffic at all for list scenes; lists of four or more triangle pairs
//     are culled first (each lane slab-tests every pair's padded bounds, the surviving
//     (ray, pair) candidates of the whole wave are tested by all 64 lanes from LDS and
//     folded per ray in list order);
//   * acceptance bookkeeping in the loop is 3 VGPRs (ok, t_to, winner id); the
//     winner's normal / material are resolved once per ray after the loop;
//   * the material table is staged in LDS once per workgroup, and so is the per-lane
//     stack of scattered-material ids that the back-to-front radiance fold of
//     ray_tracing.cu:50-52 needs (four bits or a byte per bounce instead of a 12-byte
//     attenuation in scratch memory);
//   * mesh (BVH) queries do not walk the reference's tree: one search of a mesh-wide
//     4-wide tree, done by the wave for all its rays at once (mesh_search), finds the best
//     face of every reference leaf that holds a hit, then the reference's box tests are
//     replayed on those leaves' root-to-leaf paths only, again one (leaf, level) per lane
//     (closest_hit, RUN_BVH);
//   * arithmetic follows the reference operation by operation (binary32 with
//     the binary64 islands of sphere.cu / ray_tracing.cu:68-73); the file is
//     compiled with -ffp-contract=off and IEEE divide/sqrt.  The one shortened
//     operation, 1.0f / det, is checked against the IEEE quotient on all 2^32 inputs
//     by arithmetic_selftest (as are the two fused uniform-variate conversions).
//
// Reference functions restated here (paths relative to
// /root/reference/ray-tracing-cuda/): PathTracing + Trace ray_tracing.cu:12-85,
// Camera::RayAt camera.cu:57-77, HitableList::Hit hitable_list.cu:7-25,
// Sphere::Hit sphere.cu:11-64, TriangleHit utils.cu:49-85, Parallelogram::Hit
// parallelogram.cu:17-44, Sky sky.cu:9-27, AABB::Hit bvh.cu:6-30, BVHNode::Hit
// bvh.cuh:123-158, Lambertian lambertian.cu:19-43, Metal metal.cu:12-36,
// Dielectric dielectric.cu:16-44, DiffuseLight diffuse_light.cu:5-13,
// ImageTexture::Value textures/image_texture.cu:9-15, CudaRandomInit utils.cu:43-47.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "kernels.h"

#include <cfloat>
#include <cmath>
#include <cstdlib>
#include <iterator>
#include <type_traits>
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
#include "mesh_search.h"
#include "closest_hit.h"
#include "render_body.h"
#include "query_body.h"
#include "occlusion_body.h"

// The trace kernel proper, and the same code under a second name for the scheduler's 2-spp
// cost probe (so per-kernel profiles keep the two apart).
// Second launch bound = waves per SIMD the register allocation must allow: the list-only variants
// sit at the 80-VGPR / 6-wave step and are issue-bound (one wave less costs 5 %), so the step is
// held explicitly instead of being left to the allocator's luck.
#ifndef RTMI_TRIS_WAVES
#define RTMI_TRIS_WAVES 6
#endif
#ifndef RTMI_BVH_WAVES
#define RTMI_BVH_WAVES 3
#endif
// Sphere and image-texture variants: four waves (at most 128 VGPRs: they sit just below that step, and the allocator's
// count swings by tens of registers with unrelated edits when it is not held) -- except the three that gain from a
// fifth (96 VGPRs, 6-21 spilled dwords) now that their task regions leave room for a fifth workgroup in a CU's LDS
// (scene_dev.h: kListTasks): triangles + spheres + textures (C5 shard 3.16 -> 2.93 s), the grouped sphere scan (spheres
// 1024^2: 22.2 -> 20.9 ms), short sphere runs (+2 %).  Spheres + triangles without textures lose 4-5 % at five (spills
// with no occupancy to show for them) and stay at four.  (tools/gpu_variant_time.py for the variants no workload uses)
#ifndef RTMI_SPH_WAVES
#define RTMI_SPH_WAVES(F) (((F) == (F_TRIS | F_SPHERE | F_TEX) || (F) == (F_SPHERE | F_SGROUP) || (F) == F_SPHERE) ? 5 : 4)
#endif
#define RTMI_MIN_WAVES(F) (((F) & F_BVH) ? RTMI_BVH_WAVES : ((F) & (F_TEX | F_SPHERE | F_SGROUP)) ? RTMI_SPH_WAVES(F) : ((F) & F_TRIS) ? RTMI_TRIS_WAVES : 6)
// Mesh variants share their per-workgroup tables (reference-tree nodes, materials) between more waves:
// workgroups of up to 512 lanes, two of which fill a CU's LDS with 16 waves' search regions.
#define RTMI_MAX_THREADS(F) (((F) & F_BVH) ? 512 : 256)
// One lane copies a kernel's argument block (render_body.h: RenderParams, CallParams) to where the kernel reads it.
template <class P>
__global__ void params_write_kernel(P p, P *dst) {
  if (threadIdx.x == 0 && blockIdx.x == 0) *dst = p;
}
size_t render_params_bytes() { return (sizeof(RenderParams) + 255) & ~(size_t)255; }
// The block of rtmi_trace, rtmi_render_budget and rtmi_render_features sits in the call's own d_work, behind the
// kernel's counter words (launch_call).
static_assert(kCallParamsOffset + sizeof(CallParams) <= (size_t)RTMI_TRACE_WORK_WORDS * 8u,
              "RTMI_TRACE_WORK_WORDS must hold the caller-owned kernels' argument block");
static_assert(kCallParamsOffset % alignof(CallParams) == 0, "the argument block is aligned in d_work");

// M: the mode word (kernels.h).  0 is the general kernel; kFastChains and kFastQueue are instantiated for the
// list-triangle variant (launch_render) and launched when the call's plan says the launch is what they were compiled for.
template <uint32_t F, uint32_t M = 0>
__global__ __launch_bounds__(RTMI_MAX_THREADS(F), RTMI_MIN_WAVES(F)) void render_kernel(const RenderParams *p) {
  const RenderParams &rp = in_constant(p);
  render_body<F, false, false, false, M>(rp.sc, rp.fr, rp.lc, rp.states, rp.out, rp.ray_counts, rp.counters);
}
template <uint32_t F, uint32_t M = 0>
__global__ __launch_bounds__(RTMI_MAX_THREADS(F), RTMI_MIN_WAVES(F)) void probe_kernel(const RenderParams *p) {
  const RenderParams &rp = in_constant(p);
  render_body<F, false, false, false, M>(rp.sc, rp.fr, rp.lc, rp.states, rp.out, rp.ray_counts, rp.counters);
}
// rtmi_trace: the same body in its caller-ray mode.
template <uint32_t F>
__global__ __launch_bounds__(RTMI_MAX_THREADS(F), RTMI_MIN_WAVES(F)) void trace_kernel(const CallParams *p) {
  const RenderParams &rp = in_constant(p).rp;
  const CallExtras &ex = in_constant(p).ex;
  render_body<F, true>(rp.sc, rp.fr, rp.lc, rp.states, rp.out, rp.ray_counts, rp.counters, ex.rays.origins, ex.rays.dirs, ex.tex_layers != 0);
}
// rtmi_render_budget: the same body in its budget mode.  F always holds F_DEFOCUS (launch_budget): whether a sample
// draws a lens offset is decided by the wave-uniform sc.cam.defocus at run time, so the eight query variants serve both
// cameras.
template <uint32_t F>
__global__ __launch_bounds__(RTMI_MAX_THREADS(F), RTMI_MIN_WAVES(F & ~(uint32_t)F_DEFOCUS)) void budget_kernel(const CallParams *p) {
  const RenderParams &rp = in_constant(p).rp;
  const CallExtras &ex = in_constant(p).ex;
  render_body<F, false, true>(rp.sc, rp.fr, rp.lc, rp.states, rp.out, rp.ray_counts, rp.counters, nullptr, nullptr,
                              ex.tex_layers != 0, ex.px.budget, ex.px.sq, ex.px.samples);
}
// rtmi_render_features: budget_kernel's twin with the FEATURES flag of the body set.  A kernel of its own, so that
// budget_kernel stays instruction for instruction what it is.
template <uint32_t F>
__global__ __launch_bounds__(RTMI_MAX_THREADS(F), RTMI_MIN_WAVES(F & ~(uint32_t)F_DEFOCUS)) void feature_kernel(const CallParams *p) {
  const RenderParams &rp = in_constant(p).rp;
  const CallExtras &ex = in_constant(p).ex;
  render_body<F, false, true, true>(rp.sc, rp.fr, rp.lc, rp.states, rp.out, rp.ray_counts, rp.counters, nullptr, nullptr,
                                    ex.tex_layers != 0, ex.px.budget, ex.px.sq, ex.px.samples, &ex.feat);
}
// rtmi_bounce: the same body in its caller-ray mode, one iteration per item (STEP).
template <uint32_t F>
__global__ __launch_bounds__(RTMI_MAX_THREADS(F), RTMI_MIN_WAVES(F)) void bounce_kernel(const CallParams *p) {
  const RenderParams &rp = in_constant(p).rp;
  const CallExtras &ex = in_constant(p).ex;
  render_body<F, true, false, false, 0, true>(rp.sc, rp.fr, rp.lc, rp.states, nullptr, nullptr, rp.counters, nullptr, nullptr, false,
                                              nullptr, nullptr, nullptr, nullptr, &ex.step);
}
// rtmi_bounce_list: bounce_kernel's twin with the LIST flag of the body set.  A kernel of its own, so that bounce_kernel
// stays instruction for instruction what it is.
template <uint32_t F>
__global__ __launch_bounds__(RTMI_MAX_THREADS(F), RTMI_MIN_WAVES(F)) void bounce_list_kernel(const CallParams *p) {
  const RenderParams &rp = in_constant(p).rp;
  const CallExtras &ex = in_constant(p).ex;
  render_body<F, true, false, false, 0, true, true>(rp.sc, rp.fr, rp.lc, rp.states, nullptr, nullptr, rp.counters, nullptr, nullptr,
                                                    false, nullptr, nullptr, nullptr, nullptr, &ex.step, &ex.list);
}

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

// ------------------------------------------------------------------ longest-first tile order
// A pixel is an indivisible serial chain (its samples share one RNG stream), so the end of a
// frame is a tail of lanes finishing their last pixel.  Handing out the expensive tiles first
// shortens that tail (longest-processing-time-first).  Cost estimate: rays per tile measured by
// a 2-spp probe pass on a scratch copy of the RNG states.  The order only changes which lane
// renders which pixel when; every pixel's arithmetic is unchanged.
__global__ __launch_bounds__(256) void tile_cost_kernel(const uint32_t *__restrict__ ray_counts, int n_tiles,
                                                         uint32_t *__restrict__ cost, uint32_t *__restrict__ max_cost) {
  int t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= n_tiles) return;
  const uint4 *p = reinterpret_cast<const uint4 *>(ray_counts + (size_t)t * 64);
  uint32_t s = 0;
#pragma unroll
  for (int i = 0; i < 16; i++) {
    uint4 v = p[i];
    s += v.x + v.y + v.z + v.w;
  }
  cost[t] = s;
  atomicMax(max_cost, s);
}

// One workgroup: counting sort of the tiles into 256 cost buckets, most expensive bucket first.
// Also sizes the "sparse" head of the queue (sparse_items, in work items; render_body, mesh
// variants): the outlier tiles -- at least twice the mean cost, in a frame whose most expensive
// tile costs at least three times the mean -- up to `sparse_cap` items, what the grid can hold at
// one pixel per kSparseStride lanes.
__global__ __launch_bounds__(1024) void tile_order_kernel(const uint32_t *__restrict__ cost,
                                                          const uint32_t *__restrict__ max_cost, int n_tiles,
                                                          uint32_t *__restrict__ order,
                                                          uint32_t *__restrict__ sparse_items, uint32_t sparse_cap,
                                                          uint32_t outlier_x10) {
  __shared__ uint32_t bins[256];
  __shared__ uint32_t base[256];
  __shared__ unsigned long long total;
  __shared__ uint32_t outliers;
  for (int i = threadIdx.x; i < 256; i += blockDim.x) bins[i] = 0;
  if (threadIdx.x == 0) total = 0ull, outliers = 0u;
  __syncthreads();
  const uint32_t mx = *max_cost > 0 ? *max_cost : 1;
  unsigned long long part = 0ull;
  for (int t = threadIdx.x; t < n_tiles; t += blockDim.x) {
    uint32_t b = 255u - (uint32_t)(((unsigned long long)cost[t] * 255ull) / mx);  // bucket 0 = most expensive
    atomicAdd(&bins[b], 1u);
    part += cost[t];
  }
  atomicAdd(&total, part);
  __syncthreads();
  {
    const unsigned long long sum = total;  // mean = sum / n_tiles; compare cost * n_tiles with k * sum
    uint32_t mine = 0;
    for (int t = threadIdx.x; t < n_tiles; t += blockDim.x)
      if ((unsigned long long)cost[t] * (unsigned long long)n_tiles * 10ull >= (unsigned long long)outlier_x10 * sum) mine++;
    if (mine) atomicAdd(&outliers, mine);
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    uint32_t run = 0;
    for (int i = 0; i < 256; i++) {
      base[i] = run;
      run += bins[i];
    }
    const bool skewed = (unsigned long long)mx * (unsigned long long)n_tiles >= 3ull * total;
    const uint32_t items = outliers * 64u;
    *sparse_items = skewed ? (items < sparse_cap ? items : sparse_cap) : 0u;
  }
  __syncthreads();
  for (int t = threadIdx.x; t < n_tiles; t += blockDim.x) {
    uint32_t b = 255u - (uint32_t)(((unsigned long long)cost[t] * 255ull) / mx);
    order[atomicAdd(&base[b], 1u)] = (uint32_t)t;
  }
}

// One workgroup: the head of the queue, pixel by pixel.  A pixel's chain is as long as its ray count, and a
// wave's query costs about as much per outlier ray it carries (measured: tools/mesh_stats.sh marks); outlier
// pixels also sit in tiles that are not outliers as tiles, where they would run their first thousand queries in a
// full wave.  So the head is made of PIXELS, from the whole frame: those whose probe count is >= pct64 % of the
// frame's largest get a wave each, >= pct32 % two per wave, >= pct16 % one per 16 lanes -- in a frame whose
// largest count is at least three times the mean, and as long as that takes no more than a quarter of the grid's
// waves and kHeadCap entries; else first the lightest class goes, then the heaviest pixels share waves two by two,
// then there is no head.  Listed pixels get bit 31 of their ray_counts word set: the ordinary queue passes them
// over.  meta[0] = head entries, meta[1], meta[2] = ends of the first two classes.
// (four small launches over the whole frame instead of one workgroup walking it three times: 0.6 ms -> tens of us)
// ws[0] largest count, ws[2..3] sum (64 bit), ws[4..6] class counts, ws[8..10] thresholds, ws[12..14] scatter cursors
__global__ __launch_bounds__(256) void head_scan_kernel(const uint32_t *__restrict__ ray_counts, int n_items,
                                                        uint32_t *__restrict__ ws) {
  uint32_t m = 0u;
  unsigned long long part = 0ull;
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n_items; i += gridDim.x * blockDim.x)
    m = max(m, ray_counts[i]), part += ray_counts[i];
  for (int off = 32; off > 0; off >>= 1) m = max(m, (uint32_t)__shfl_down((int)m, off)), part += __shfl_down(part, off);
  if ((threadIdx.x & 63) == 0) {
    atomicMax(&ws[0], m);
    atomicAdd(reinterpret_cast<unsigned long long *>(ws + 2), part);  // (d_meta is 8-byte aligned: capi.hip)
  }
}
__global__ __launch_bounds__(256) void head_count_kernel(const uint32_t *__restrict__ ray_counts, int n_items,
                                                         uint32_t *__restrict__ ws, uint32_t pct64, uint32_t pct32,
                                                         uint32_t pct16) {
  const uint32_t cmax = ws[0];
  const unsigned long long total = *reinterpret_cast<const unsigned long long *>(ws + 2);
  const bool skewed = (unsigned long long)cmax * (unsigned long long)n_items >= 3ull * total && cmax >= 4u;
  if (!skewed) return;
  const uint32_t t64 = (cmax * pct64 + 99u) / 100u, t32 = (cmax * pct32 + 99u) / 100u, t16 = (cmax * pct16 + 99u) / 100u;
  uint32_t c0 = 0u, c1 = 0u, c2 = 0u;
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n_items; i += gridDim.x * blockDim.x) {
    const uint32_t c = ray_counts[i];
    if (c >= t16) (c >= t64 ? c0 : c >= t32 ? c1 : c2)++;
  }
  for (int off = 32; off > 0; off >>= 1) c0 += __shfl_down(c0, off), c1 += __shfl_down(c1, off), c2 += __shfl_down(c2, off);
  if ((threadIdx.x & 63) == 0) {
    if (c0) atomicAdd(&ws[4], c0);
    if (c1) atomicAdd(&ws[5], c1);
    if (c2) atomicAdd(&ws[6], c2);
  }
}
__global__ void head_plan_kernel(int n_items, uint32_t *__restrict__ meta, uint32_t *__restrict__ ws, uint32_t grid_waves,
                                 uint32_t pct64, uint32_t pct32, uint32_t pct16) {
  const uint32_t cmax = ws[0], none = 0xffffffffu;
  const unsigned long long total = *reinterpret_cast<const unsigned long long *>(ws + 2);
  const bool skewed = (unsigned long long)cmax * (unsigned long long)n_items >= 3ull * total && cmax >= 4u;
  uint32_t t64 = skewed ? (cmax * pct64 + 99u) / 100u : none, t32 = skewed ? (cmax * pct32 + 99u) / 100u : none,
           t16 = skewed ? (cmax * pct16 + 99u) / 100u : none;
  uint32_t a = ws[4], b = ws[5], c3 = ws[6];
  auto over = [&]() { return a + (b + 1u) / 2u + (c3 + 3u) / 4u > grid_waves / 4u || a + b + c3 > (uint32_t)kHeadCap; };
  if (over()) c3 = 0u, t16 = t32;
  if (over()) b += a, a = 0u, t64 = none;
  if (over()) b = 0u, t32 = none, t16 = none;
  meta[0] = a + b + c3, meta[1] = a, meta[2] = a + b;
  ws[8] = t64, ws[9] = t32, ws[10] = t16;
  ws[12] = 0u, ws[13] = a, ws[14] = a + b;  // scatter cursors
}
__global__ __launch_bounds__(256) void head_scatter_kernel(uint32_t *__restrict__ ray_counts, int n_items,
                                                           uint32_t *__restrict__ head, uint32_t *__restrict__ ws) {
  const uint32_t t64 = ws[8], t32 = ws[9], t16 = ws[10];
  if (t16 == 0xffffffffu) return;
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n_items; i += gridDim.x * blockDim.x) {
    const uint32_t c = ray_counts[i];
    if (c >= t16) {
      head[atomicAdd(&ws[12 + (c >= t64 ? 0 : c >= t32 ? 1 : 2)], 1u)] = (uint32_t)i;
      ray_counts[i] = c | 0x80000000u;
    }
  }
}

// The queue's order is kept per QUARTER tile (16 work items = two rows of a tile).  List scenes: the tiles in
// longest-first order, each tile's quarters one after the other.
__global__ __launch_bounds__(256) void expand_order_kernel(const uint32_t *__restrict__ order, int n_tiles,
                                                            uint32_t *__restrict__ qmap) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n_tiles * 4) qmap[i] = order[i >> 2] * 4u + (uint32_t)(i & 3);
}
// Mesh scenes with a cost probe: a quarter's cost = the lane-steps the probe's mesh searches spent on its 16 pixels
// (+ their ray counts, so that it is never zero) ...
__global__ __launch_bounds__(256) void quarter_cost_kernel(const uint32_t *__restrict__ work, const uint32_t *__restrict__ rays,
                                                            int n_quarters, uint32_t *__restrict__ cost,
                                                            uint32_t *__restrict__ max_cost) {
  const int qd = blockIdx.x * blockDim.x + threadIdx.x;
  if (qd >= n_quarters) return;
  uint32_t s = 0;
  for (int i = 0; i < 16; i++) s += work[(size_t)qd * 16 + i] + (rays[(size_t)qd * 16 + i] & 0x7fffffffu);
  cost[qd] = s;
  atomicMax(max_cost, s);
}
// ... one workgroup sorts the quarters by cost (256 buckets, dearest first) ...
__global__ __launch_bounds__(1024) void quarter_sort_kernel(const uint32_t *__restrict__ cost, const uint32_t *__restrict__ max_cost,
                                                             int n_quarters, uint32_t *__restrict__ sorted) {
  __shared__ uint32_t bins[256];
  __shared__ uint32_t base[256];
  for (int i = threadIdx.x; i < 256; i += blockDim.x) bins[i] = 0;
  __syncthreads();
  const uint32_t mx = *max_cost > 0 ? *max_cost : 1;
  for (int t = threadIdx.x; t < n_quarters; t += blockDim.x)
    atomicAdd(&bins[255u - (uint32_t)(((unsigned long long)cost[t] * 255ull) / mx)], 1u);
  __syncthreads();
  if (threadIdx.x == 0) {
    uint32_t run = 0;
    for (int i = 0; i < 256; i++) base[i] = run, run += bins[i];
  }
  __syncthreads();
  for (int t = threadIdx.x; t < n_quarters; t += blockDim.x)
    sorted[atomicAdd(&base[255u - (uint32_t)(((unsigned long long)cost[t] * 255ull) / mx)], 1u)] = (uint32_t)t;
}
// ... and every 64 consecutive work items of the queue -- what the lanes of a wave pick up together -- are dealt one
// quarter from each quartile of that order (a snake: b, 2n - 1 - b, 2n + b, 4n - 1 - b): no wave starts on 64 rays of a
// dense tile (150-260 k cycles per query of a full wave against 40 k for the frame's typical mix; such waves WERE the
// frame's last per cent), every wave's first 64 pixels cost about the same, and the dearest quarters still go first.
__global__ __launch_bounds__(256) void snake_map_kernel(const uint32_t *__restrict__ sorted, int n_tiles,
                                                         uint32_t *__restrict__ qmap) {
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= n_tiles) return;
  const int n = n_tiles;
  qmap[4 * b + 0] = sorted[b];
  qmap[4 * b + 1] = sorted[2 * n - 1 - b];
  qmap[4 * b + 2] = sorted[2 * n + b];
  qmap[4 * b + 3] = sorted[4 * n - 1 - b];
}
hipError_t launch_quarter_order(const uint32_t *d_order, const uint32_t *d_work, const uint32_t *d_rays, int n_tiles,
                                uint32_t *d_qcost, uint32_t *d_qsorted, uint32_t *d_qmax, uint32_t *d_qmap, hipStream_t stream) {
  if (!d_work) {
    hipLaunchKernelGGL(expand_order_kernel, dim3((n_tiles * 4 + 255) / 256), dim3(256), 0, stream, d_order, n_tiles, d_qmap);
    return hipGetLastError();
  }
  hipError_t e = hipMemsetAsync(d_qmax, 0, sizeof(uint32_t), stream);
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(quarter_cost_kernel, dim3((n_tiles * 4 + 255) / 256), dim3(256), 0, stream, d_work, d_rays, n_tiles * 4,
                     d_qcost, d_qmax);
  hipLaunchKernelGGL(quarter_sort_kernel, dim3(1), dim3(1024), 0, stream, d_qcost, d_qmax, n_tiles * 4, d_qsorted);
  hipLaunchKernelGGL(snake_map_kernel, dim3((n_tiles + 255) / 256), dim3(256), 0, stream, d_qsorted, n_tiles, d_qmap);
  return hipGetLastError();
}

// One thread per chain (wave r of SIMD s, c = r S + s), walked backwards so that every tile learns what follows it.
// The SIMD's k-th tile is rank k S + (k odd ? S - 1 - s : s); the wave's j-th tile is the SIMD's k = j R + (j odd ? R - 1 - r : r).
__global__ __launch_bounds__(256) void chain_link_kernel(const uint32_t *__restrict__ order, const uint32_t *__restrict__ cost,
                                                          int n_tiles, int S, int R, float scale, int32_t *__restrict__ first,
                                                          int32_t *__restrict__ next, uint32_t *__restrict__ fut) {
  const int c = blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= S * R) return;
  const int s = c % S, r = c / S;
  auto rank = [&](int j) -> int64_t {
    const int64_t k = (int64_t)j * R + ((j & 1) ? R - 1 - r : r);
    return k * S + ((k & 1) ? S - 1 - s : s);
  };
  int steps = 0;
  while (rank(steps) < n_tiles) steps++;
  float acc = 0.f;
  int32_t after = -1;
  for (int j = steps - 1; j >= 0; j--) {
    const uint32_t t = order[rank(j)];
    next[t] = after;
    fut[t] = (uint32_t)fminf(acc, 4.0e9f);
    acc += (float)cost[t] * scale;
    after = (int32_t)t;
  }
  first[c] = after;
}
hipError_t launch_chain_plan(const uint32_t *d_order, const uint32_t *d_cost, int n_tiles, int simds, int rounds, int spp,
                             int probe_spp, int32_t *d_first, int32_t *d_next, uint32_t *d_fut, hipStream_t stream) {
  const int n = simds * rounds;
  if (n <= 0) return hipSuccess;
  hipLaunchKernelGGL(chain_link_kernel, dim3((n + 255) / 256), dim3(256), 0, stream, d_order, d_cost, n_tiles, simds, rounds,
                     (float)spp / (64.f * (float)probe_spp), d_first, d_next, d_fut);
  return hipGetLastError();
}

hipError_t launch_tile_order(uint32_t *d_ray_counts, int n_tiles, uint32_t *d_cost, uint32_t *d_meta,
                             uint32_t *d_order, uint32_t *d_head, uint32_t sparse_cap, int grid_waves, int outlier_x10,
                             const int head_pct[3], hipStream_t stream) {
  hipError_t e = hipMemsetAsync(d_meta, 0, 32 * sizeof(uint32_t), stream);
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(tile_cost_kernel, dim3((n_tiles + 255) / 256), dim3(256), 0, stream, d_ray_counts, n_tiles, d_cost,
                     d_meta);
  hipLaunchKernelGGL(tile_order_kernel, dim3(1), dim3(1024), 0, stream, d_cost, d_meta, n_tiles, d_order, d_meta + 1,
                     sparse_cap, (uint32_t)outlier_x10);
  if (d_head) {
    const int p64 = head_pct[0], p32 = head_pct[1], p16 = head_pct[2];  // (rtmi_render_opts.head_pct)
    uint32_t *ws = d_meta + 16;  // 16 words of workspace behind the 16 of d_meta (zeroed with them)
    const int n_items = n_tiles * 64, blocks = n_items / 4096 > 0 ? (n_items / 4096 < 1024 ? n_items / 4096 : 1024) : 1;
    hipLaunchKernelGGL(head_scan_kernel, dim3(blocks), dim3(256), 0, stream, d_ray_counts, n_items, ws);
    hipLaunchKernelGGL(head_count_kernel, dim3(blocks), dim3(256), 0, stream, d_ray_counts, n_items, ws, (uint32_t)p64,
                       (uint32_t)p32, (uint32_t)p16);
    hipLaunchKernelGGL(head_plan_kernel, dim3(1), dim3(1), 0, stream, n_items, d_meta + 1, ws, (uint32_t)grid_waves,
                       (uint32_t)p64, (uint32_t)p32, (uint32_t)p16);
    hipLaunchKernelGGL(head_scatter_kernel, dim3(blocks), dim3(256), 0, stream, d_ray_counts, n_items, d_head, ws);
  }
  return hipGetLastError();
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
#ifdef RTMI_STATS
hipError_t copy_wave_stats(unsigned long long *host, size_t bytes) {
  return hipMemcpyFromSymbol(host, HIP_SYMBOL(g_wave_stats), bytes);
}
#endif
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
static inline int64_t cdiv(int64_t a, int64_t b) { return (a + b - 1) / b; }

hipError_t launch_rng_init(uint64_t seed, const FrameDev &fr, const uint32_t *d_jump, uint32_t *d_states,
                           hipStream_t stream, int64_t first) {
  if (fr.items == 0) return hipSuccess;
  hipLaunchKernelGGL(rng_init_kernel, dim3((unsigned)cdiv(fr.items, 256)), dim3(256), 0, stream, seed, fr, first, d_jump,
                     d_states);
  return hipGetLastError();
}

// RTMI_PLAIN_LIST=1 (read once): keep the uncultured list scan, for A/B measurements
static bool plain_list_scan() {
  static const bool v = [] {
    const char *e = getenv("RTMI_PLAIN_LIST");
    return e && atoi(e) != 0;
  }();
  return v;
}

// id_stack = false (query kernels): no stack of material ids, whatever fr.max_depth says.
// tex_layers = false (trace kernels of scenes without image textures): an F_TEX variant with the untextured id stack.
static LaunchCfg make_cfg(uint32_t variant, const SceneDev &sc, const FrameDev &fr, int threads, size_t *lds_bytes,
                          bool mats_in_lds = true, bool id_stack = true, bool tex_layers = true) {
  LaunchCfg lc{};
  lc.threads = threads;
  lc.tile_order = nullptr;
  lc.lds_mats = mats_in_lds && sc.n_mats <= kLdsMats ? sc.n_mats : 0;
  lc.wide_ids = sc.n_mats > 256 ? 1 : sc.n_mats <= 16 ? 2 : 0;
  size_t off = ((size_t)lc.lds_mats * sizeof(MatRec) + 15) & ~(size_t)15;
  // The fold's colour table of the common list frame's kernels (kernels.h: trims_fold_rgb) at its fixed place, in every
  // launch whose facts can pick them (fast_path_mode: variant F_TRIS, nibble ids, the material table staged): the id
  // stack starts behind it.  The general kernel reads stack_off as it always did and leaves the table alone.
  static_assert(kFoldRgbOff == 16 * sizeof(MatRec) && kFoldRgbOff % 16 == 0, "behind the largest table nibble ids can name");
  if (variant == (uint32_t)F_TRIS && lc.wide_ids == 2 && lc.lds_mats > 0 && id_stack) off = (size_t)kFoldRgbOff + kFoldRgbBytes;
  // The 24-bit product of the same kernels (kernels.h: trims_mul24; closest_hit.h: load_tri_pts): record index x record
  // size of the staged TriPts table.
  static_assert((uint64_t)(2 * kLdsPairs + 2) * sizeof(TriPts) < (1u << 24) && sizeof(TriPts) == 48,
                "staged TriPts records: index (one pair of padding included) x 48 bytes is a 24-bit product");
  lc.stack_off = (int32_t)off;
  const size_t levels = (size_t)(fr.max_depth > 0 ? fr.max_depth : 1);
  // image-textured variants: one 32-bit word per level (material id, or the sampled texel)
  size_t stack = (variant & F_TEX) && tex_layers ? levels * threads * 4 : (lc.wide_ids == 2 ? (levels + 1) / 2 : levels) * threads * (lc.wide_ids == 1 ? 2 : 1);
  if (!id_stack) stack = 0;
  size_t noff = (off + stack + 15) & ~(size_t)15;
  lc.nodes_off = (int32_t)noff;
  lc.lds_nodes = (variant & F_BVH) ? (sc.n_nodes < kLdsNodes ? sc.n_nodes : kLdsNodes) : 0;
  size_t paoff = (noff + (size_t)lc.lds_nodes * sizeof(BvhNode) + 15) & ~(size_t)15;
  lc.paths_off = (int32_t)paoff;
  lc.lds_paths = (variant & F_BVH) ? (sc.n_leaf_paths < kLdsPaths ? sc.n_leaf_paths : kLdsPaths) : 0;
  size_t soff = (paoff + (size_t)lc.lds_paths * sizeof(int32_t) + 15) & ~(size_t)15;
  lc.mesh_off = (int32_t)soff;
  size_t poff = soff + ((variant & F_BVH) ? (size_t)(threads / 64) * kMeshWaveWords * sizeof(int) : 0);
  // the culled list scan: any list of four or more pairs; its records are staged in LDS up to kLdsPairs pairs
  const bool cull = (variant & F_TRIS) && sc.n_pairs >= kCullMinPairs && !plain_list_scan();
  const bool staged = cull && sc.n_pairs <= kLdsPairs;
  lc.pairs_off = staged ? (int32_t)poff : -1;
  size_t noff2 = (poff + (staged ? (size_t)sc.n_pairs * 2 * sizeof(TriPts) : 0) + 15) & ~(size_t)15;
  lc.nrm_off = staged ? (int32_t)noff2 : -1;
  size_t loff = (noff2 + (staged ? (size_t)sc.n_pairs * 2 * sizeof(TriNrm) : 0) + 15) & ~(size_t)15;
  const bool groups = (variant & F_SGROUP) && sc.n_sph_groups > 0;  // the grouped sphere scan shares its tests too
  const bool share = cull || groups;
  lc.list_off = share ? (int32_t)loff : -1;
  size_t coff = loff + (share ? (size_t)(threads / 64) * kListWaveWords(variant) * sizeof(int) : 0);
  lc.cand_off = groups ? (int32_t)coff : -1;
  *lds_bytes = coff + (groups ? (size_t)threads * (kSphCand * sizeof(uint16_t) + sizeof(int)) : 0);  // slots + a counter per lane
  // The grouped sphere scan is built for four waves per SIMD (108 VGPRs): four 256-lane workgroups per CU need 40 KiB
  // each at most.  A big material table (scenes/spheres.cu: one material per sphere, 15 KiB) that stands in the way
  // of the fourth workgroup stays in global memory -- measured on spheres 1024^2: 7.6 -> 8.5 Grays/s.
  if (groups && mats_in_lds && lc.lds_mats > 0 && *lds_bytes * (size_t)(1024 / threads) > 160 * 1024) {
    size_t without = 0;
    const LaunchCfg alt = make_cfg(variant, sc, fr, threads, &without, false, id_stack, tex_layers);
    if (without * (size_t)(1024 / threads) <= 160 * 1024) {
      *lds_bytes = without;
      return alt;
    }
  }
  return lc;
}

// Dynamic LDS of a launch of Kernel: above the default limit of 64 KiB it is asked for (160 KiB per CU on gfx950).  The
// bodies address LDS by byte offsets of the dynamic array (render_body.h: lds_byte, the id stack; query_body.h and
// occlusion_body.h: the staged regions): right only while the kernel declares no static LDS, in EVERY build flavour
// (-DRTMI_STATS, -DRTMI_CHECK_MARGINS, A/B builds) -- asked of the code object once per kernel.
template <auto Kernel>
static hipError_t dynamic_lds(size_t lds) {
  const void *k = reinterpret_cast<const void *>(Kernel);
  if (lds > 64 * 1024) {
    const hipError_t e = hipFuncSetAttribute(k, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    if (e != hipSuccess) return e;
  }
  static const hipError_t no_static = [k] {
    hipFuncAttributes a{};
    const hipError_t e = hipFuncGetAttributes(&a, k);
    return e != hipSuccess ? e : a.sharedSizeBytes == 0 ? hipSuccess : hipErrorInvalidConfiguration;
  }();
  return no_static;
}

// The specialisations that are instantiated; a feature set outside them uses the last, which has every feature.
constexpr uint32_t kVariants[] = {0u, F_TRIS, F_SPHERE, F_TRIS | F_SPHERE, F_SPHERE | F_SGROUP, F_TRIS | F_SPHERE | F_SGROUP,
                                  F_TRIS | F_BVH, F_TRIS | F_SPHERE | F_TEX, F_ALL};
// The query variants (rtmi_intersect, rtmi_occluded, rtmi_trace, rtmi_render_budget): F_TEX always (closest_hit tracks
// the winner's u, v bitwise only then), never F_DEFOCUS (no camera is involved): the render variants so mapped.
constexpr uint32_t kQueryVariants[] = {F_TEX, F_TRIS | F_TEX, F_SPHERE | F_TEX, F_TRIS | F_SPHERE | F_TEX,
                                       F_SPHERE | F_SGROUP | F_TEX, F_TRIS | F_SPHERE | F_SGROUP | F_TEX,
                                       F_TRIS | F_BVH | F_TEX, F_ALL & ~F_DEFOCUS};
template <size_t N>
static uint32_t pick_listed(const uint32_t (&list)[N], uint32_t features) {
  for (const uint32_t v : list)
    if ((features & ~v) == 0) return v;
  return list[N - 1];
}
uint32_t pick_variant(uint32_t features) { return pick_listed(kVariants, features); }
uint32_t pick_query_variant(uint32_t features) {
  return pick_listed(kQueryVariants, (features & ~(uint32_t)F_DEFOCUS) | F_TEX);
}
// f(std::integral_constant<uint32_t, V>()) for the variant V of List that equals `variant`; `otherwise` for any other.
template <const auto &List, size_t I = 0, class R, class Fn>
static R with_listed(uint32_t variant, R otherwise, Fn &&f) {
  if constexpr (I == std::size(List)) return otherwise;
  else if (variant == List[I]) return f(std::integral_constant<uint32_t, List[I]>());
  else return with_listed<List, I + 1>(variant, otherwise, f);
}

// ------------------------------------------------------------------ the fast path's predicate
uint32_t fast_path_mode(const FastPathFacts &f) {
  const auto pow2 = [](int v) { return v > 0 && (v & (v - 1)) == 0 && v <= (1 << 20); };
  const bool common = f.enabled != 0 && f.variant == (uint32_t)F_TRIS && f.n_mats >= 1 && f.n_mats <= 16 && f.mats_in_lds != 0 &&
                      f.pairs_in_lds != 0 && f.unsigned_colours != 0 && f.det_safe != 0 && pow2(f.width) && pow2(f.height) &&
                      f.lane_stride == 1 && f.priorities != 0;
  if (!common) return 0u;
  if (!f.chains) return kFastQueue;
  return f.resumed && f.tile_cost ? kFastChains : 0u;
}
// What the kernels that cull against the PairSlab table (kernels.h: culls_by_slab) assume of every ray they trace:
// |o|inf <= kOriginReach * list_mag.  A render's origins are the camera position and points on list triangles (variant
// F_TRIS alone: no lens, no other primitives), so the camera decides; the second condition keeps k = -o / d and
// tc = fma(c, 1 / d, k) finite under the reciprocals clamped to 1e30 (closest_hit.h).
bool slab_reach_covers(float list_mag, const CameraDev &cam) {
  const float reach = kOriginReach * list_mag;
  const bool cam_in_reach = fabsf(cam.position.x) <= reach && fabsf(cam.position.y) <= reach && fabsf(cam.position.z) <= reach;
  const bool k_finite = (double)(kOriginReach + 1.0f) * (double)list_mag * 1e30 < (double)FLT_MAX;
  return cam_in_reach && k_finite;
}
FastPathFacts fast_path_facts(uint32_t variant, const SceneDev &sc, const FrameDev &fr, int threads, int enabled) {
  size_t lds = 0;
  const LaunchCfg lc = make_cfg(variant, sc, fr, threads, &lds);
  FastPathFacts f{};
  f.enabled = enabled, f.variant = variant, f.n_mats = sc.n_mats, f.mats_in_lds = lc.lds_mats > 0 && lc.wide_ids == 2;
  // staged, shared tests, and the slab table's reach covers this camera (asked per launch of the scene's current camera)
  f.pairs_in_lds = lc.pairs_off >= 0 && lc.nrm_off >= 0 && lc.list_off >= 0 && slab_reach_covers(sc.list_mag, sc.cam);
  f.unsigned_colours = sc.unsigned_colours, f.det_safe = sc.det_safe, f.width = fr.width, f.height = fr.height;
  return f;
}

size_t render_lds_bytes(uint32_t variant, const SceneDev &sc, const FrameDev &fr, int threads) {
  size_t lds = 0;
  (void)make_cfg(variant, sc, fr, threads, &lds);
  return lds;
}

// *per_cu = workgroups of Kernel per compute unit at this launch shape; 0 with an error: it does not fit, or the HIP
// call that failed.
template <auto Kernel>
static hipError_t kernel_occupancy(int threads, size_t lds, int *per_cu) {
  *per_cu = 0;
  if (lds > 160 * 1024) return hipErrorInvalidConfiguration;
  hipError_t e = dynamic_lds<Kernel>(lds);
  if (e == hipSuccess) e = hipOccupancyMaxActiveBlocksPerMultiprocessor(per_cu, Kernel, threads, lds);
  if (e != hipSuccess) *per_cu = 0;
  return e;
}
// A launch of Kernel on its argument block: the block goes to d_block in stream order, just before the kernel that reads it.
struct LaunchAt {
  int blocks, threads;
  size_t lds;
  hipStream_t stream;
};
template <auto Kernel, class P>
static hipError_t launch_block(const LaunchAt &at, const P &block, P *d_block) {
  const hipError_t e = dynamic_lds<Kernel>(at.lds);
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(params_write_kernel<P>, dim3(1), dim3(64), 0, at.stream, block, d_block);
  hipLaunchKernelGGL(Kernel, dim3(at.blocks), dim3(at.threads), at.lds, at.stream, (const P *)d_block);
  return hipGetLastError();
}
int render_occupancy(uint32_t variant, const SceneDev &sc, const FrameDev &fr, int threads, bool fast_path) {
  return with_listed<kVariants>(variant, 0, [&](auto v) {
    constexpr uint32_t F = decltype(v)::value;
    size_t lds = 0;
    (void)make_cfg(F, sc, fr, threads, &lds);
    if (threads > RTMI_MAX_THREADS(F)) return 0;
    int nb = 0;
    (void)kernel_occupancy<render_kernel<F>>(threads, lds, &nb);
    if constexpr (F == (uint32_t)F_TRIS) {
      // which of the three kernels a launch of this frame gets is decided after the grid is sized (lane stride, plan):
      // the grid must fit whichever it is (all three are built for the same waves per SIMD and use the same LDS)
      if (fast_path) {
        int nc = 0, nq = 0;
        (void)kernel_occupancy<render_kernel<F, kFastChains>>(threads, lds, &nc);
        (void)kernel_occupancy<render_kernel<F, kFastQueue>>(threads, lds, &nq);
        nb = nb < nc ? nb : nc, nb = nb < nq ? nb : nq;
      }
    }
    return nb;
  });
}

// Work items per atomic of a queue in image order: its last tiles weigh as much as any, so batches only where the atomics
// would otherwise be the frame -- cornell 1024^2 x 16 spp: 8.0 ms a pixel at a time, 5.2 ms four at a time; at 200 spp
// sixteen at a time cost 8 %
// (below 32 samples -- where list frames are not scheduled -- 256 / samples: at 24 spp two pixels per atomic left a 2048^2
// frame at the cursor's rate, 23.8 ms against 22.1 ms for 32 spp)
static int image_order_batch(int samples, int cap) {
  const int per_atomic = samples < 32 ? 256 / (samples > 0 ? samples : 1) : 64 / samples;
  return per_atomic < 1 ? 1 : per_atomic > cap ? cap : per_atomic;
}

hipError_t launch_render(uint32_t variant, const SceneDev &sc, const FrameDev &fr, uint32_t *d_states, float *d_out,
                         uint32_t *d_ray_counts, unsigned long long *d_counters, const SchedPlan &plan, bool probe,
                         uint32_t fast, int blocks, int threads, const RenderTuning &tune, void *d_params, hipStream_t stream) {
  return with_listed<kVariants>(variant, hipErrorInvalidValue, [&](auto v) {
    constexpr uint32_t F = decltype(v)::value;
    size_t lds = 0;
    LaunchCfg lc = make_cfg(F, sc, fr, threads, &lds);
    lc.tile_order = plan.tile_order;
    lc.visit_counts = plan.visit_counts;
    lc.sparse_items = plan.sparse_items;
    lc.head_list = plan.head_list;
    lc.probe_marks = plan.probe_marks;
    lc.sparse_stride = tune.sparse_stride;
    lc.exclusive = tune.exclusive;
    lc.probe_spp = plan.probe_spp;
    lc.promote = tune.promote;
    lc.lane_stride = tune.lane_stride > 0 ? tune.lane_stride : 1;
    lc.prio_tab = plan.prio_tab;  // (a first pass has one when it is long enough to gain from priorities: capi.hip)
    lc.tile_cost = plan.tile_cost;
    lc.rate_scale = 1.f / (64.f * (float)(plan.probe_spp > 0 ? plan.probe_spp : 1));
    lc.chain_next = (F & F_BVH) || lc.prio_tab == nullptr ? nullptr : plan.chain_next;
    lc.chain_fut = plan.chain_fut, lc.chain_first = plan.chain_first, lc.claims = plan.claims;
    lc.plan_simds = plan.plan_simds, lc.plan_rounds = plan.plan_rounds;
    lc.prio_every = tune.prio_every > 0 ? tune.prio_every : 16;
    {  // (render_body.h: the wave draws from the queue in batches; tune.fetch_batch / fetch_batch_first: A/B measurements)
      // a first pass of a few samples: whole tiles; longest-first order: 16 (measured 4 / 16 / 64 on frames of 2.3 ...
      // 12.8 pixels per lane, NOTES.md); image order, or a first pass as long as a frame: the lanes that wait
      // (a pooled item waits for a lane of its wave: the longer a pixel takes, the fewer -- from 4,096 samples on, none)
      const int samples = fr.k_end - fr.k_begin > 0 ? fr.k_end - fr.k_begin : 1;
      const int by_length = 4096 / samples < 1 ? 1 : 4096 / samples;
      // image order (a frame too short to be scheduled, or a first pass as long as a frame): image_order_batch
      lc.fetch_batch = probe && samples <= 4 ? tune.fetch_batch_first : plan.tile_order != nullptr ? std::min(by_length, tune.fetch_batch) : image_order_batch(samples, 16);
    }
    RenderParams rp;
    rp.sc = sc, rp.fr = fr, rp.lc = lc;
    rp.states = d_states, rp.out = d_out, rp.ray_counts = d_ray_counts, rp.counters = d_counters;
    RenderParams *dp = reinterpret_cast<RenderParams *>(d_params);
    const LaunchAt at{blocks, threads, lds, stream};
    if constexpr (F == (uint32_t)F_TRIS) {
      // the kernels compiled for the common list frame: which one the plan says (capi.hip: plan_render), checked here
      // against what their bits promise of this block (kernels.h: PIN_PRIORITIES, PIN_EVERY_LANE, PIN_CHAINS, PIN_QUEUE)
      const bool chains = fast == kFastChains && !probe && lc.chain_next && lc.tile_cost && fr.k_begin > 0 && d_ray_counts;
      const bool queue = fast == kFastQueue && !lc.chain_next;
      if (fast != 0u && (!lc.prio_tab || lc.lane_stride != 1 || !(chains || queue))) return hipErrorInvalidValue;
      // ... and of the layout: the fold's colour table has its room in front of the id stack (make_cfg)
      if (fast != 0u && lc.stack_off != kFoldRgbOff + kFoldRgbBytes) return hipErrorInvalidValue;
      // the three kernels below cull against the PairSlab table (kernels.h: culls_by_slab) and read it where the others
      // read the PairBox records (scene_dev.h: PairSlab)
      static_assert(culls_by_slab(kFastChains) && culls_by_slab(kFastQueue) && !culls_by_slab(0u), "which kernels read the slab table");
      if (chains || queue) rp.sc.pair_boxes = pair_slabs_of(sc.pair_boxes, sc.n_pairs);
      if (chains) return launch_block<render_kernel<F, kFastChains>>(at, rp, dp);
      if (queue && !probe) return launch_block<render_kernel<F, kFastQueue>>(at, rp, dp);
      if (queue) return launch_block<probe_kernel<F, kFastQueue>>(at, rp, dp);
    }
    if (fast != 0u) return hipErrorInvalidValue;  // (only the list-triangle variant has fast kernels)
    if (probe) return launch_block<probe_kernel<F>>(at, rp, dp);
    return launch_block<render_kernel<F>>(at, rp, dp);
  });
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

// ------------------------------------------------------------------ closest-hit queries (rtmi_intersect)
// query_body.h around the render's closest_hit<F>, on the query variants (kQueryVariants).
template <uint32_t F>
__global__ __launch_bounds__(RTMI_MAX_THREADS(F), RTMI_MIN_WAVES(F)) void query_kernel(QueryParams qp) {
  query_body<F>(qp);
}

constexpr int kQueryThreads = 256;

// make_cfg's layout for the query and occlusion kernels (nothing is shaded: no material table, no id stack), and the
// kQueryLdsExtra bytes of stand-in words behind it (QueryParams / OcclusionParams: dummy_off)
static LaunchCfg query_cfg(uint32_t variant, const SceneDev &sc, size_t *lds) {
  FrameDev fr{};  // (make_cfg reads max_depth only, for the id stack the queries do without)
  LaunchCfg lc = make_cfg(variant, sc, fr, kQueryThreads, lds, false, false);
  *lds = ((*lds + 15) & ~(size_t)15) + kQueryLdsExtra;
  return lc;
}

// The grid of a batch of n rays on Kernel: as many workgroups as fit on n_cu compute units, at most one per
// kQueryThreads rays.
template <auto Kernel>
static hipError_t query_blocks(size_t lds, int n_cu, int64_t n, int *blocks) {
  int nb = 0;
  const hipError_t e = kernel_occupancy<Kernel>(kQueryThreads, lds, &nb);
  if (e != hipSuccess) return e;
  if (nb < 1) nb = 1;
  const int64_t want = (n + kQueryThreads - 1) / kQueryThreads, cap = (int64_t)n_cu * nb;
  *blocks = (int)(want < cap ? (want > 0 ? want : 1) : cap);
  return hipSuccess;
}

hipError_t launch_query(uint32_t variant, const SceneDev &sc, const QueryDev &qd, int n_cu, int64_t n, const float *d_o,
                        const float *d_d, const float *d_t_max, int32_t *d_hits, unsigned long long *d_abandoned,
                        unsigned long long *d_check, hipStream_t stream) {
  return with_listed<kQueryVariants>(variant, hipErrorInvalidValue, [&](auto v) {
    constexpr uint32_t F = decltype(v)::value;
    size_t lds = 0;
    QueryParams qp;
    qp.sc = sc, qp.qd = qd;
    qp.lc = query_cfg(F, sc, &lds);
    int blocks = 0;
    const hipError_t e = query_blocks<query_kernel<F>>(lds, n_cu, n, &blocks);
    if (e != hipSuccess) return e;
    qp.n = n, qp.origins = d_o, qp.dirs = d_d, qp.t_max = d_t_max, qp.hits = d_hits;
    qp.abandoned = d_abandoned, qp.check = d_check;
    qp.dummy_off = (int32_t)(lds - kQueryLdsExtra);
    hipLaunchKernelGGL(query_kernel<F>, dim3(blocks), dim3(kQueryThreads), lds, stream, qp);
    return hipGetLastError();
  });
}

// ------------------------------------------------------------------ any-hit visibility queries (rtmi_occluded)
// occlusion_body.h around closest_hit<F, true>: one instantiation per query variant, with the query kernels' staging,
// LDS layout (its stand-in words included) and launch sizing.
template <uint32_t F>
__global__ __launch_bounds__(RTMI_MAX_THREADS(F), RTMI_MIN_WAVES(F)) void occlusion_kernel(OcclusionParams p) {
  occlusion_body<F>(p);
}

// rtmi_occluded_list: occlusion_kernel's twin with the LIST flag of the body set, as bounce_list_kernel is bounce_kernel's.
// A kernel of its own, so that occlusion_kernel stays what it was; the list's words travel behind the argument block the
// two share.  (Its name must not contain "occlusion_kernel": tests/test_occluded_host.py counts those.)
template <uint32_t F>
__global__ __launch_bounds__(RTMI_MAX_THREADS(F), RTMI_MIN_WAVES(F)) void occlusion_list_kernel(OcclusionParams p, OcclusionList l) {
  occlusion_body<F, true>(p, l);
}

// One launcher for both.  list == nullptr: occlusion_kernel, the grid capped by n.  Else occlusion_list_kernel with the same
// staging, LDS layout, stand-in words and sizing, the grid capped by the list's capacity (n_list > 0), not by n: a short
// list over many paths launches few workgroups.
hipError_t launch_occlusion(uint32_t variant, const SceneDev &sc, const float near_lo[3], const float near_hi[3],
                            float near_short, int n_cu, int64_t n, const PathList *list, const float *d_o, const float *d_d,
                            const float *d_t_max, uint8_t *d_occluded, unsigned long long *d_counts,
                            unsigned long long *d_check, hipStream_t stream) {
  return with_listed<kQueryVariants>(variant, hipErrorInvalidValue, [&](auto v) {
    constexpr uint32_t F = decltype(v)::value;
    size_t lds = 0;
    OcclusionParams p;
    p.sc = sc;
    p.lc = query_cfg(F, sc, &lds);
    int blocks = 0;
    const hipError_t e = list ? query_blocks<occlusion_list_kernel<F>>(lds, n_cu, list->n_list, &blocks)
                              : query_blocks<occlusion_kernel<F>>(lds, n_cu, n, &blocks);
    if (e != hipSuccess) return e;
    p.n = n, p.origins = d_o, p.dirs = d_d, p.t_max = d_t_max, p.occluded = d_occluded;
    p.counts = d_counts, p.check = d_check;
    p.dummy_off = (int32_t)(lds - kQueryLdsExtra);
    for (int k = 0; k < 3; k++) p.near_lo[k] = near_lo[k], p.near_hi[k] = near_hi[k];
    p.near_short = near_short;
    if (list) {
      hipLaunchKernelGGL(occlusion_list_kernel<F>, dim3(blocks), dim3(kQueryThreads), lds, stream, p, OcclusionList{*list});
    } else {
      hipLaunchKernelGGL(occlusion_kernel<F>, dim3(blocks), dim3(kQueryThreads), lds, stream, p);
    }
    return hipGetLastError();
  });
}

// ------------------------------------------------------------------ the entries that own their device state
// rtmi_trace, rtmi_render_budget, rtmi_render_features: render_body.h in a mode of Kernel's on the query variants (F_TEX
// always: the layer stack is one 32-bit word per level, the material id or the sampled texel -- or, without tex_layers,
// the untextured id stack).  A persistent grid sized by occupancy; the lanes refill from the call's own queue cursor
// (d_work[2]) as their items end, fetch_batch items per wave per atomic.  The argument block is written behind the
// counter words of d_work.
template <uint32_t F, auto Kernel>
static hipError_t launch_call(const SceneDev &sc, const FrameDev &fr, bool tex_layers, int fetch_batch, int n_cu,
                              CallExtras ex, uint32_t *d_states, float *d_out, uint32_t *d_ray_counts,
                              unsigned long long *d_work, hipStream_t stream, bool id_stack = true,
                              int64_t grid_items = -1) {  // (>= 0: the items the grid is capped by, when not fr.items)
  // workgroup size: the one that keeps the most lanes resident (a deep 32-bit layer stack can leave room for one
  // 256-lane workgroup per CU only, as for the render's mesh variants: capi.hip launch_shape)
  int threads = 0, per_cu = 0;
  for (int t = 256; t >= 64; t /= 2) {
    size_t lds_t = 0;
    (void)make_cfg(F, sc, fr, t, &lds_t, true, id_stack, tex_layers);
    int nb = 0;
    (void)kernel_occupancy<Kernel>(t, lds_t, &nb);
    if (t * nb > threads * per_cu) threads = t, per_cu = nb;
  }
  if (per_cu < 1) return hipErrorInvalidConfiguration;  // (the staged tables and the stack do not fit a CU's LDS)
  size_t lds = 0;
  CallParams cp;
  cp.rp.sc = sc, cp.rp.fr = fr, cp.rp.lc = make_cfg(F, sc, fr, threads, &lds, true, id_stack, tex_layers);
  cp.rp.lc.lane_stride = 1, cp.rp.lc.fetch_batch = fetch_batch, cp.rp.lc.rate_scale = 1.f;
  cp.rp.states = d_states, cp.rp.out = d_out, cp.rp.ray_counts = d_ray_counts, cp.rp.counters = d_work;
  cp.ex = ex, cp.ex.tex_layers = tex_layers ? 1 : 0;
  const int64_t want = ((grid_items >= 0 ? grid_items : fr.items) + threads - 1) / threads, cap = (int64_t)n_cu * per_cu;
  return launch_block<Kernel>(LaunchAt{(int)(want < cap ? want : cap), threads, lds, stream}, cp,
                              reinterpret_cast<CallParams *>(reinterpret_cast<char *>(d_work) + kCallParamsOffset));
}

// The frame of a batch of n caller rays or paths: one item each, one sample, the whole batch one rank's.
static FrameDev batch_frame(int64_t n, int max_depth) {
  FrameDev fr{};
  fr.height = 1, fr.width = 1, fr.spp = 1, fr.max_depth = max_depth, fr.post = 0;
  fr.k_begin = 0, fr.k_end = 1, fr.rank = 0, fr.world = 1;
  fr.items = n;
  return fr;
}

hipError_t launch_trace(uint32_t variant, const SceneDev &sc, bool tex_layers, int n_cu, int64_t n, int max_depth,
                        const float *d_o, const float *d_d, uint32_t *d_states, float *d_radiance,
                        uint32_t *d_ray_counts, unsigned long long *d_work, hipStream_t stream) {
  return with_listed<kQueryVariants>(variant, hipErrorInvalidValue, [&](auto v) {
    constexpr uint32_t F = decltype(v)::value;
    CallExtras ex{};
    ex.rays = {d_o, d_d};
    // (64: the largest batch render_body.h's queue takes: one path per item, 16 times a pixel's atomics)
    return launch_call<F, trace_kernel<F>>(sc, batch_frame(n, max_depth), tex_layers, 64, n_cu, ex, d_states, d_radiance,
                                           d_ray_counts, d_work, stream);
  });
}

// One iteration of the trace loop per ray (rtmi_bounce; render_body.h: STEP): the item is a path, its depth is the
// caller's business (fr.max_depth = 1 only opens the loop's depth test), and no layer is stacked -- no id stack in LDS.
// With a list, the same step for the listed paths (rtmi_bounce_list; render_body.h: LIST).  Every array keeps n paths --
// fr.items is n, the stride of the RNG planes -- and only the grid is sized by the list: launch_call's occupancy-sized
// grid, capped by n_list, the host's bound on a length that stays on the device.
hipError_t launch_bounce(uint32_t variant, const SceneDev &sc, const QueryDev &qd, int n_cu, int64_t n, const PathList *list,
                         float *d_o, float *d_d, uint32_t *d_states, float *d_emitted, float *d_attenuation, int32_t *d_hits,
                         uint32_t *d_steps, unsigned long long *d_work, hipStream_t stream) {
  return with_listed<kQueryVariants>(variant, hipErrorInvalidValue, [&](auto v) {
    constexpr uint32_t F = decltype(v)::value;
    const FrameDev fr = batch_frame(n, 1);
    CallExtras ex{};
    ex.step = {d_o, d_d, d_emitted, d_attenuation, d_hits, d_steps, qd};
    if (!list) return launch_call<F, bounce_kernel<F>>(sc, fr, false, 64, n_cu, ex, d_states, nullptr, nullptr, d_work, stream, false);
    ex.list = *list;
    return launch_call<F, bounce_list_kernel<F>>(sc, fr, false, 64, n_cu, ex, d_states, nullptr, nullptr, d_work, stream, false,
                                                 list->n_list);
  });
}

// ------------------------------------------------------------------ the live paths as a list (rtmi_path_compact)
// Three launches, none of whose workgroups waits for another: each workgroup counts the live candidates among its
// kCompactItems entries; one workgroup turns the counts into offsets (and the total into *d_count_out); each workgroup
// finds its live candidates again and writes them from its offset on, in the candidates' order.  A wave owns
// kCompactChunks consecutive chunks of 64 entries, lane l entry l of each, so a live candidate's place is its
// workgroup's offset + the live ones of the waves and chunks before its own + those of the lower lanes (mbcnt).
// The rays are read twice (24 B a path); the list's length, where it is on the device, is read by every workgroup and
// the grids are sized by the host's bound.
constexpr int kCompactThreads = 256, kCompactChunks = 4;
constexpr int kCompactItems = kCompactThreads * kCompactChunks;  // entries per workgroup: a scratch word each
constexpr int kCompactScanThreads = 256;  // the scan's one workgroup; each lane sums ceil(workgroups / 256) counts in a row
static_assert(kCompactItems == RTMI_PATH_COMPACT_ITEMS, "rtmi.h states the entries per scratch word");

struct CompactArgs {
  const float *origins, *dirs;  // float[n][3]
  const uint32_t *list_in;      // nullable: the candidates (null: 0, 1, 2, ...)
  const uint32_t *count_in;     // nullable: a device word that cuts the candidates short
  uint32_t n, n_list;
};
// (live_ray, whether a step would step a ray: path_shared.h, which rtmi_path_advance's unit includes too)
// Entry e of the candidates: its path, and whether the next step would step it.
__device__ __forceinline__ bool compact_live(const CompactArgs &a, const PathList &pl, uint32_t e, uint32_t end, uint32_t &path) {
  path = 0u;
  if (e >= end) return false;
  path = list_entry(pl, e);
  if (path >= a.n) return false;  // (not a path: dropped)
  const float *o = a.origins + (int64_t)path * 3, *d = a.dirs + (int64_t)path * 3;
  return live_ray(mk(o[0], o[1], o[2]), mk(d[0], d[1], d[2]));
}
// The live candidates of this lane's kCompactChunks entries: their paths, the chunks' wave masks, and the wave's total.
__device__ __forceinline__ uint32_t compact_wave(const CompactArgs &a, uint32_t (&path)[kCompactChunks],
                                                 unsigned long long (&mask)[kCompactChunks]) {
  const PathList pl{a.list_in, a.count_in, a.n_list};  // (the block keeps its layout; the rule is path_list.h's)
  const uint32_t end = list_end(pl);
  // (entries below 2^31 + kCompactItems: the grid covers n_list <= 2^31 - 1)
  const uint32_t first = blockIdx.x * (uint32_t)kCompactItems + (threadIdx.x >> 6) * (uint32_t)(64 * kCompactChunks) + (threadIdx.x & 63u);
  uint32_t total = 0u;
#pragma unroll
  for (int c = 0; c < kCompactChunks; c++) {
    mask[c] = __builtin_amdgcn_ballot_w64(compact_live(a, pl, first + (uint32_t)c * 64u, end, path[c]));
    total += (uint32_t)__popcll(mask[c]);
  }
  return total;
}

__global__ __launch_bounds__(kCompactThreads) void compact_count_kernel(CompactArgs a, uint32_t *__restrict__ counts) {
  __shared__ uint32_t s_wave[kCompactThreads / 64];
  uint32_t path[kCompactChunks];
  unsigned long long mask[kCompactChunks];
  const uint32_t total = compact_wave(a, path, mask);
  if ((threadIdx.x & 63u) == 0u) s_wave[threadIdx.x >> 6] = total;
  __syncthreads();
  if (threadIdx.x == 0u) {
    uint32_t sum = 0u;
    for (int w = 0; w < kCompactThreads / 64; w++) sum += s_wave[w];
    counts[blockIdx.x] = sum;
  }
}

// counts[0 .. n_blocks) -> their exclusive prefix sums, in place; *count_out = their total.  One workgroup.
__global__ __launch_bounds__(kCompactScanThreads) void compact_scan_kernel(uint32_t n_blocks, uint32_t *__restrict__ counts,
                                                                            uint32_t *__restrict__ count_out) {
  __shared__ uint32_t s_wave[kCompactScanThreads / 64];
  const uint32_t per = (n_blocks + (uint32_t)kCompactScanThreads - 1u) / (uint32_t)kCompactScanThreads;
  const uint32_t lo = threadIdx.x * per < n_blocks ? threadIdx.x * per : n_blocks;  // (per <= 2^13: no wrap)
  const uint32_t hi = lo + per < n_blocks ? lo + per : n_blocks;
  uint32_t sum = 0u;
  for (uint32_t i = lo; i < hi; i++) sum += counts[i];
  uint32_t incl = sum;  // inclusive scan over the wave's lanes
  for (int off = 1; off < 64; off <<= 1) {
    const uint32_t below = (uint32_t)__shfl_up((int)incl, off);
    if ((threadIdx.x & 63u) >= (uint32_t)off) incl += below;
  }
  if ((threadIdx.x & 63u) == 63u) s_wave[threadIdx.x >> 6] = incl;
  __syncthreads();
  uint32_t run = incl - sum;
  for (uint32_t w = 0; w < (threadIdx.x >> 6); w++) run += s_wave[w];
  for (uint32_t i = lo; i < hi; i++) {
    const uint32_t c = counts[i];
    counts[i] = run;
    run += c;
  }
  if (threadIdx.x == (uint32_t)kCompactScanThreads - 1u) *count_out = run;  // (the last lane's end is the total)
}

__global__ __launch_bounds__(kCompactThreads) void compact_scatter_kernel(CompactArgs a, const uint32_t *__restrict__ offsets,
                                                                           uint32_t *__restrict__ list_out) {
  __shared__ uint32_t s_wave[kCompactThreads / 64];
  uint32_t path[kCompactChunks];
  unsigned long long mask[kCompactChunks];
  const uint32_t total = compact_wave(a, path, mask);
  if ((threadIdx.x & 63u) == 0u) s_wave[threadIdx.x >> 6] = total;
  __syncthreads();
  uint32_t at = offsets[blockIdx.x];
  for (uint32_t w = 0; w < (threadIdx.x >> 6); w++) at += s_wave[w];
  const unsigned long long me = 1ull << (threadIdx.x & 63u);
#pragma unroll
  for (int c = 0; c < kCompactChunks; c++) {
    // (at + rank < the total of all workgroups <= the candidates <= n_list: inside list_out)
    if (mask[c] & me) list_out[at + (uint32_t)lane_rank(mask[c])] = path[c];
    at += (uint32_t)__popcll(mask[c]);
  }
}

size_t path_compact_scratch_bytes(int64_t n_list) {
  if (n_list < 0) n_list = 0;
  const int64_t blocks = cdiv(n_list, (int64_t)kCompactItems);
  return (size_t)(blocks > 0 ? blocks : 1) * sizeof(uint32_t);
}

hipError_t launch_path_compact(int64_t n, const float *d_origins, const float *d_dirs, const PathList &in, uint32_t *d_list_out,
                               uint32_t *d_count_out, uint32_t *d_scratch, hipStream_t stream) {
  if (in.n_list == 0) return hipMemsetAsync(d_count_out, 0, sizeof(uint32_t), stream);
  const CompactArgs a = {d_origins, d_dirs, in.list, in.count, (uint32_t)n, in.n_list};
  const unsigned blocks = (unsigned)cdiv((int64_t)in.n_list, (int64_t)kCompactItems);
  hipLaunchKernelGGL(compact_count_kernel, dim3(blocks), dim3(kCompactThreads), 0, stream, a, d_scratch);
  hipLaunchKernelGGL(compact_scan_kernel, dim3(1), dim3(kCompactScanThreads), 0, stream, (uint32_t)blocks, d_scratch, d_count_out);
  hipLaunchKernelGGL(compact_scatter_kernel, dim3(blocks), dim3(kCompactThreads), 0, stream, a, (const uint32_t *)d_scratch, d_list_out);
  return hipGetLastError();
}

// Trace's return expression over the layers the steps wrote (rtmi_path_fold; include/rtmi.h states the rule): one lane
// per path, so a layer's reads are coalesced over n; product and sum each rounded on their own.
__global__ __launch_bounds__(256) void path_fold_kernel(int64_t n, uint32_t layers, const float *__restrict__ dirs,
                                                         const uint32_t *__restrict__ steps, const float *__restrict__ emitted,
                                                         const float *__restrict__ attenuation, float *__restrict__ radiance) {
  const int64_t q = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (q >= n) return;
  const uint32_t s = steps[q];
  const bool ended = dirs[q * 3 + 0] == 0.f && dirs[q * 3 + 1] == 0.f && dirs[q * 3 + 2] == 0.f;
  const V3 r = fold_layers(emitted, attenuation, n, q, (int)(s < layers ? s : layers), ended);  // (path_shared.h)
  radiance[q * 3 + 0] = r.x, radiance[q * 3 + 1] = r.y, radiance[q * 3 + 2] = r.z;
}
hipError_t launch_path_fold(int64_t n, int layers, const float *d_dirs, const uint32_t *d_steps, const float *d_emitted,
                            const float *d_attenuation, float *d_radiance, hipStream_t stream) {
  if (n == 0) return hipSuccess;
  hipLaunchKernelGGL(path_fold_kernel, dim3((unsigned)cdiv(n, 256)), dim3(256), 0, stream, n, (uint32_t)layers, d_dirs, d_steps,
                     d_emitted, d_attenuation, d_radiance);
  return hipGetLastError();
}

// The budget mode runs on the query variants + F_DEFOCUS, its items in image order.  A pixel is a serial chain, so a call
// lasts at least as long as its largest budget x that pixel's rays per sample.
hipError_t launch_budget(uint32_t variant, const SceneDev &sc, bool tex_layers, int n_cu, const FrameDev &frame,
                         const uint32_t *d_budget, uint32_t *d_states, float *d_sum, float *d_sq, uint32_t *d_samples,
                         uint32_t *d_ray_counts, const FeatureBufs *feat, unsigned long long *d_work, hipStream_t stream) {
  const bool features = feat && (feat->albedo || feat->normal || feat->depth || feat->coverage);
  return with_listed<kQueryVariants>(variant, hipErrorInvalidValue, [&](auto v) {
    constexpr uint32_t F = decltype(v)::value | F_DEFOCUS;
    FrameDev fr = frame;
    fr.post = 0, fr.k_begin = 0, fr.k_end = fr.spp;
    // items per atomic: a pixel of a few samples is as short as a ray of rtmi_trace; longer ones as launch_render's image order
    const int batch = image_order_batch(fr.spp, 64);
    CallExtras ex{};
    ex.px = {d_budget, d_sq, d_samples};
    if (features) {
      ex.feat = *feat;
      return launch_call<F, feature_kernel<F>>(sc, fr, tex_layers, batch, n_cu, ex, d_states, d_sum, d_ray_counts, d_work, stream);
    }
    return launch_call<F, budget_kernel<F>>(sc, fr, tex_layers, batch, n_cu, ex, d_states, d_sum, d_ray_counts, d_work, stream);
  });
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

#include "denoise_body.h"
#include "accumulate_body.h"
#include "camera_body.h"

}  // namespace rtmi
