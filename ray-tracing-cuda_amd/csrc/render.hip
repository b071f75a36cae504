// The render of the trace path for gfx950 (MI355X): the persistent per-pixel trace loop as render_kernel and
// probe_kernel, their launch, and the LDS layout every kernel around closest_hit is launched with.
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

#include "frame_math.h"
#include "trace_helpers.h"
#include "path_shared.h"
#include "mesh_search.h"
#include "closest_hit.h"
#include "render_body.h"
#include "launch_cfg.h"

size_t render_params_bytes() { return (sizeof(RenderParams) + 255) & ~(size_t)255; }

// The trace kernel proper, and the same code under a second name for the scheduler's 2-spp
// cost probe (so per-kernel profiles keep the two apart).  (launch bounds: launch_cfg.h)
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

#ifdef RTMI_STATS
hipError_t copy_wave_stats(unsigned long long *host, size_t bytes) {
  return hipMemcpyFromSymbol(host, HIP_SYMBOL(g_wave_stats), bytes);
}
#endif

// ------------------------------------------------------------------ launchers
// RTMI_PLAIN_LIST=1 (read once): keep the uncultured list scan, for A/B measurements
static bool plain_list_scan() {
  static const bool v = [] {
    const char *e = getenv("RTMI_PLAIN_LIST");
    return e && atoi(e) != 0;
  }();
  return v;
}

// (launch_cfg.h says what id_stack and tex_layers are)
LaunchCfg make_cfg(uint32_t variant, const SceneDev &sc, const FrameDev &fr, int threads, size_t *lds_bytes,
                   bool mats_in_lds, bool id_stack, bool tex_layers) {
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

uint32_t pick_variant(uint32_t features) { return pick_listed(kVariants, features); }

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
        if (sc.diffuse_only) {  // (kernels.h: render_pins)
          (void)kernel_occupancy<render_kernel<F, kFastChains | PIN_DIFFUSE>>(threads, lds, &nc);
          (void)kernel_occupancy<render_kernel<F, kFastQueue | PIN_DIFFUSE>>(threads, lds, &nq);
        } else {
          (void)kernel_occupancy<render_kernel<F, kFastChains>>(threads, lds, &nc);
          (void)kernel_occupancy<render_kernel<F, kFastQueue>>(threads, lds, &nq);
        }
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
int image_order_batch(int samples, int cap) {
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
      // a scene of Lambertians and lights alone: the same three kernels compiled for it (kernels.h: PIN_DIFFUSE)
      if (render_pins(fast, sc) & PIN_DIFFUSE) {
        if (chains) return launch_block<render_kernel<F, kFastChains | PIN_DIFFUSE>>(at, rp, dp);
        if (queue && !probe) return launch_block<render_kernel<F, kFastQueue | PIN_DIFFUSE>>(at, rp, dp);
        if (queue) return launch_block<probe_kernel<F, kFastQueue | PIN_DIFFUSE>>(at, rp, dp);
      }
      if (chains) return launch_block<render_kernel<F, kFastChains>>(at, rp, dp);
      if (queue && !probe) return launch_block<render_kernel<F, kFastQueue>>(at, rp, dp);
      if (queue) return launch_block<probe_kernel<F, kFastQueue>>(at, rp, dp);
    }
    if (fast != 0u) return hipErrorInvalidValue;  // (only the list-triangle variant has fast kernels)
    if (probe) return launch_block<probe_kernel<F>>(at, rp, dp);
    return launch_block<render_kernel<F>>(at, rp, dp);
  });
}

}  // namespace rtmi
