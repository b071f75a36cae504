// rtmi_path_advance: the paths of a wavefront finished and refilled in place (include/rtmi.h "path advance" states the
// rule operation by operation).  After every rtmi_bounce_list of a loop the candidates of that step's list
// come here: a path the step stepped gets its layer pushed onto its own stack; a path that has ended, or has made its
// max_depth steps, is folded and added to the budget buffers as rtmi_path_fold and rtmi_sample_add would; and the pixel
// whose path is finished gets the camera ray of its next sample as rtmi_camera_rays would make it -- so the next step's
// list holds paths that all have work.  A pixel's samples stay one serial chain on one RNG state, in sample order: the
// loop is bit for bit rtmi_render_budget.
//
// Every operation is one binary32 rounding in the order written (the translation unit is compiled with
// -ffp-contract=off): tests/advancelib.py restates the rule in numpy and the two agree word for word.
#pragma once
// (included by advance.hip inside namespace rtmi, after path_shared.h: live_ray, fold_layers, camera_ray; path_list.h)

constexpr int kAdvanceThreads = 256;
constexpr int kAdvanceBlocksPerCu = 8;  // the grid's cap: longer lists are walked in strides of the grid's lanes
constexpr uint32_t kInFlight = 1u << 31;  // bit 31 of cursor word 0 (F); the low 31 bits: samples started (k)

struct AdvanceArgs {
  FrameDev fr;
  CameraProj proj;
  const uint32_t *budget;        // nullable: every pixel has fr.spp
  const uint32_t *list, *count;  // rtmi_bounce_list's candidates (both nullable)
  uint32_t n_list;
  float *origins, *dirs;         // float[items][3]
  uint32_t *states;              // RTMI_STATE_WORDS planes of uint32[items]
  uint32_t *steps;               // uint32[items]
  const float *emitted, *attenuation;      // float[items][3]: the ONE layer every step writes
  float *emitted_stack, *attenuation_stack;  // float[max_depth][items][3] (not touched when max_depth == 0)
  uint32_t *cursor;              // uint32[items][2]: {F << 31 | k, P}
  float *sum, *sq;               // sq nullable
  uint32_t *samples, *ray_counts;  // ray_counts nullable
  unsigned long long *counts;    // nullable: {samples finished, their queries, camera rays made}
};

// The wave's sum of a per-lane count (every lane of the wave calls it): a butterfly of six shuffles.
__device__ __forceinline__ unsigned long long wave_sum(unsigned long long v) {
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) v += (unsigned long long)__shfl_xor((long long)v, off);
  return v;
}

// CURVED: the launch's projection is EQUIRECT or FISHEYE (the host picks the kernel by it).  The other kernel is compiled
// with the kind known to be CAMERA or ORTHOGRAPHIC, so the binary64 sines and cosines of the curved kinds, and the
// registers they take, are not in it.
template <bool CURVED>
__device__ __forceinline__ void advance_body(const AdvanceArgs &a) {
  const int64_t n = a.fr.items;
  CameraProj proj = a.proj;
  if (!CURVED) proj.kind = proj.kind == PROJ_ORTHOGRAPHIC ? PROJ_ORTHOGRAPHIC : PROJ_CAMERA;
  const uint32_t spp = (uint32_t)a.fr.spp, max_depth = (uint32_t)a.fr.max_depth;
  const PathList pl{a.list, a.count, a.n_list};  // (the block keeps its layout; the rule is path_list.h's)
  const uint32_t end = list_end(pl);
  // chunks of 64 entries by wave number, as direct_sample_kernel takes them: no cursor, no atomic
  const uint32_t lane = threadIdx.x & 63u;
  const uint32_t wave = (uint32_t)__builtin_amdgcn_readfirstlane((int)((blockIdx.x * blockDim.x + threadIdx.x) >> 6));
  const uint32_t stride = gridDim.x * blockDim.x;  // the grid's lanes (a multiple of 64)
  unsigned long long n_finished = 0ull, n_queries = 0ull, n_made = 0ull;  // (per lane; summed over the wave at the end)
  for (uint64_t at = (uint64_t)wave * 64u; at < end; at += stride) {
    const uint32_t e = (uint32_t)at + lane;
    if (e >= end) continue;
    const uint32_t item = list_entry(pl, e);
    if ((int64_t)item >= n) continue;  // (an entry that is no work item is dropped before anything is addressed with it)
    const int64_t q = (int64_t)item, q3 = q * 3;
    const int64_t idx = frame_pixel_of_rank(a.fr, a.fr.rank, q);
    if (idx < 0) {  // padding: a zero direction, which every compaction drops
      a.dirs[q3 + 0] = 0.f, a.dirs[q3 + 1] = 0.f, a.dirs[q3 + 2] = 0.f;
      continue;
    }
    uint32_t b = a.budget ? a.budget[q] : spp;
    b = b < spp ? b : spp;
    // One batch of loads, issued before anything is decided from them, so that their waits overlap: the cursor, the step
    // count, the layer and the ray, whether or not this candidate turns out to need the last two.
    const uint32_t word0 = a.cursor[q * 2 + 0];
    uint32_t P = a.cursor[q * 2 + 1];
    uint32_t st = a.steps[q];
    const V3 le = mk(a.emitted[q3 + 0], a.emitted[q3 + 1], a.emitted[q3 + 2]);
    const V3 la = mk(a.attenuation[q3 + 0], a.attenuation[q3 + 1], a.attenuation[q3 + 2]);
    V3 o = mk(a.origins[q3 + 0], a.origins[q3 + 1], a.origins[q3 + 2]);
    V3 d = mk(a.dirs[q3 + 0], a.dirs[q3 + 1], a.dirs[q3 + 2]);
    uint32_t k = word0 & ~kInFlight;
    bool F = (word0 & kInFlight) != 0u;
    // push: the step just made stepped the path, and its layer goes onto the path's own stack
    if (F && st == P + 1u) {
      if (P < max_depth) {
        const int64_t to = ((int64_t)P * n + q) * 3;
        a.emitted_stack[to + 0] = le.x, a.emitted_stack[to + 1] = le.y, a.emitted_stack[to + 2] = le.z;
        a.attenuation_stack[to + 0] = la.x, a.attenuation_stack[to + 1] = la.y, a.attenuation_stack[to + 2] = la.z;
      }
      P += 1u;
    }
    // what the loop changes stays in registers and is written once behind it
    Rng rng{};
    V3 sum = splat(0.f), sq = splat(0.f);
    uint32_t n_samples = 0u, n_rays = 0u;
    bool have_rng = false, have_acc = false, new_ray = false, zero_dir = false;
    const uint32_t bound = k <= b ? b - k + 1u : 1u;  // finishes and refills alternate: at most b - k refills and one stop
    for (uint32_t it = 0u; it < bound; it++) {
      if (F) {  // finish
        const bool live = live_ray(o, d);
        if (live && st < max_depth) break;  // the path has work: the next step steps it
        const uint32_t c = st < max_depth ? st : max_depth;
        const bool scattered = d.x != 0.f || d.y != 0.f || d.z != 0.f;
        const V3 x = fold_layers(a.emitted_stack, a.attenuation_stack, n, q, (int)c, !scattered);
        const uint32_t queries = (c == 0u && !live) ? 0u : c + (scattered ? 1u : 0u);
        if (!have_acc) {
          have_acc = true;
          sum = mk(a.sum[q3 + 0], a.sum[q3 + 1], a.sum[q3 + 2]);
          if (a.sq) sq = mk(a.sq[q3 + 0], a.sq[q3 + 1], a.sq[q3 + 2]);
          n_samples = a.samples[q];
          if (a.ray_counts) n_rays = a.ray_counts[q];
        }
        sum = mk(__fadd_rn(sum.x, x.x), __fadd_rn(sum.y, x.y), __fadd_rn(sum.z, x.z));
        sq = mk(__fadd_rn(sq.x, __fmul_rn(x.x, x.x)), __fadd_rn(sq.y, __fmul_rn(x.y, x.y)), __fadd_rn(sq.z, __fmul_rn(x.z, x.z)));
        n_samples += 1u, n_rays += queries;
        n_finished += 1ull, n_queries += (unsigned long long)queries;
        F = false;
      }
      // refill
      if (k < b) {
        if (!have_rng) {
          have_rng = true;
          rng.d = a.states[0 * n + q], rng.v0 = a.states[1 * n + q], rng.v1 = a.states[2 * n + q];
          rng.v2 = a.states[3 * n + q], rng.v3 = a.states[4 * n + q], rng.v4 = a.states[5 * n + q];
        }
        camera_ray(a.fr, proj, idx, rng, o, d);
        new_ray = true;
        st = 0u, P = 0u, k += 1u, F = true;
        n_made += 1ull;
      } else {
        zero_dir = true;  // no samples left: the next compaction drops the item for good
        break;
      }
    }
    if (have_acc) {
      a.sum[q3 + 0] = sum.x, a.sum[q3 + 1] = sum.y, a.sum[q3 + 2] = sum.z;
      if (a.sq) a.sq[q3 + 0] = sq.x, a.sq[q3 + 1] = sq.y, a.sq[q3 + 2] = sq.z;
      a.samples[q] = n_samples;
      if (a.ray_counts) a.ray_counts[q] = n_rays;
    }
    if (have_rng) {
      a.states[0 * n + q] = rng.d, a.states[1 * n + q] = rng.v0, a.states[2 * n + q] = rng.v1;
      a.states[3 * n + q] = rng.v2, a.states[4 * n + q] = rng.v3, a.states[5 * n + q] = rng.v4;
    }
    if (new_ray) {
      a.origins[q3 + 0] = o.x, a.origins[q3 + 1] = o.y, a.origins[q3 + 2] = o.z;
      a.dirs[q3 + 0] = d.x, a.dirs[q3 + 1] = d.y, a.dirs[q3 + 2] = d.z;
      a.steps[q] = 0u;
    }
    if (zero_dir) a.dirs[q3 + 0] = 0.f, a.dirs[q3 + 1] = 0.f, a.dirs[q3 + 2] = 0.f;
    a.cursor[q * 2 + 0] = (F ? kInFlight : 0u) | (k & ~kInFlight);
    a.cursor[q * 2 + 1] = P;
  }
  // the three counters, once per wave: the wave's sums, then one vector atomic each from lane 0
  if (a.counts) {
    n_finished = wave_sum(n_finished), n_queries = wave_sum(n_queries), n_made = wave_sum(n_made);
    if (lane == 0u) {
      if (n_finished) atomicAdd(&a.counts[0], n_finished);
      if (n_queries) atomicAdd(&a.counts[1], n_queries);
      if (n_made) atomicAdd(&a.counts[2], n_made);
    }
  }
}
