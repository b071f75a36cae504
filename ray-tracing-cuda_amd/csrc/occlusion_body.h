// Batched any-hit visibility queries on caller-made rays (rtmi_occluded, and rtmi_occluded_list for the paths of a
// list).  Included by kernels.hip inside namespace rtmi, after query_body.h (not a stand-alone header).
//
// The answer is defined by rtmi_intersect: occluded[i] = 1 iff HitableList::Hit(Ray(o, d), 1e-3, inf) has a hit and
// (float)t <= t_max[i].  The engine is closest_hit<F, true> (closest_hit.h, OCC) with query_body.h's staging, run in up
// to two passes:
//   pass 0: a lane stops at its first acceptance at or below the seed -- the largest value of the record's type whose
//     (float) is <= t_max -- which means occluded.  Its running bound starts
//       - at the seed (bounded), so that every cull prunes by it, when the origin lies outside the padded bounds of
//         the meshes (OcclusionParams::near_lo / near_hi) or t_max is short against their size (near_short).  A mesh
//         whose search lists faces that the replay then refuses marks the lane uncertain (quirk g8: a ray that starts
//         inside a path box and leaves it beyond t_max);
//       - at +inf (exact, never uncertain) for a longer ray from inside them: there g8 is the rule rather than the
//         exception (AO rays from a mesh's surface start inside every box on the way to their own leaf, and reach
//         faces well inside the big ones), the bounded walk would send most of what the mesh occludes through the
//         fallback below, and the bound prunes little of a search that starts in the middle of the mesh.
//   pass 1, exact fallback, only for uncertain lanes that accepted nothing: the unbounded engine from +inf, stopping
//     once the running bound is at or below the seed; then the filter.  Counted in counts[1].
//
// LIST is rtmi_occluded_list (occlusion_list_kernel): the same query, its rays named by the candidates of a list.  Only
// the place a lane's ray comes from differs; the passes, the near-box rule and the fallback are the lines below for both.
#pragma once

struct OcclusionParams {
  SceneDev sc;
  LaunchCfg lc;               // as for the query kernel: only the staging offsets are used
  int64_t n;                  // rays
  const float *origins, *dirs;
  const float *t_max;         // nullable
  uint8_t *occluded;          // n bytes
  unsigned long long *counts; // nullable: {abandoned mesh searches, rays decided by the fallback}; else the LDS words
  unsigned long long *check;  // -DRTMI_CHECK_MARGINS: nullable, {re-done, disagreements}; else unused
  int32_t dummy_off;          // byte offset in dynamic LDS of two words that stand in for a null `counts`
  float near_lo[3], near_hi[3];  // padded union of the meshes' root bounds (empty without meshes) ...
  float near_short;              // ... and the t_max below which a ray from inside them still walks bounded
};

// LIST: rtmi_bounce_list's candidates (list, count: both nullable).  Handed over beside OcclusionParams, not inside it: the
// argument block of occlusion_kernel stays what it was.
// (A type of its own over path_list.h's: it is part of the list kernels' mangled names.)
struct OcclusionList : PathList {};

// query_body.h's staging (render_body.h's prologue without the materials), as a function: the scene's pair corners,
// top mesh nodes and leaf paths copied in, and this wave's regions of the dynamic LDS.  The caller waits at a barrier
// before using them.  (query_body.h keeps its inline copy, which points here: moved into a function there, it costs the
// query kernels an SGPR spill.  A change to the LDS layout changes both.)
struct QueryLds {
  const BvhNode *s_nodes;
  const int *s_paths;
  const float4 *s_tris;
  int *wl, *ll;
  uint16_t *cands;
};
template <uint32_t F>
__device__ __forceinline__ QueryLds query_stage(const SceneDev &sc, const LaunchCfg &lc, unsigned char *smem) {
  QueryLds q;
  q.s_nodes = reinterpret_cast<const BvhNode *>(smem + lc.nodes_off);
  q.wl = nullptr;
  if (F & F_BVH)
    q.wl = reinterpret_cast<int *>(smem + lc.mesh_off) + __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)) * kMeshWaveWords;
  q.s_tris = nullptr;
  if ((F & F_TRIS) && lc.pairs_off >= 0) {
    q.s_tris = reinterpret_cast<const float4 *>(smem + lc.pairs_off);
    const uint32_t *src = reinterpret_cast<const uint32_t *>(sc.tri_pts);
    uint32_t *dst = reinterpret_cast<uint32_t *>(smem + lc.pairs_off);
    for (int w = threadIdx.x; w < sc.n_pairs * 24; w += blockDim.x) dst[w] = src[w];
  }
  q.ll = nullptr;
  if ((F & (F_TRIS | F_SGROUP)) && lc.list_off >= 0)
    q.ll = reinterpret_cast<int *>(smem + lc.list_off) + __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)) * kListWaveWords(F);
  q.cands = nullptr;
  if ((F & F_SGROUP) && lc.cand_off >= 0)
    q.cands = reinterpret_cast<uint16_t *>(smem + lc.cand_off) +
              __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)) * (64 * kSphCand + 128);
  if ((F & F_BVH) && lc.lds_nodes > 0) {
    const uint32_t *src = reinterpret_cast<const uint32_t *>(sc.nodes);
    uint32_t *dst = reinterpret_cast<uint32_t *>(smem + lc.nodes_off);
    for (int w = threadIdx.x; w < lc.lds_nodes * 8; w += blockDim.x) dst[w] = src[w];
  }
  q.s_paths = reinterpret_cast<const int *>(smem + lc.paths_off);
  if ((F & F_BVH) && lc.lds_paths > 0) {
    int *dst = reinterpret_cast<int *>(smem + lc.paths_off);
    for (int w = threadIdx.x; w < lc.lds_paths; w += blockDim.x) dst[w] = sc.leaf_paths[w];
  }
  return q;
}

// The seed of the bounded pass for the record's type T: the largest T whose (float) is <= t_max (t_max not NaN).  For
// float that is t_max.  For double it is the midpoint between t_max and the next float up when round-to-nearest-even
// takes the midpoint down to t_max (t_max's last mantissa bit is 0), else the double just below the midpoint.  So a
// test `t <= seed` in T accepts exactly what the filter `(float)t <= t_max` keeps.
template <typename T>
__device__ __forceinline__ double occlusion_seed(float tm) {
  if (sizeof(T) == sizeof(float) || !(__builtin_fabsf(tm) < INFINITY)) return (double)tm;
  const int32_t b = __float_as_int(tm);
  const float up = tm == 0.f ? __int_as_float(1) : __int_as_float(tm > 0.f ? b + 1 : b - 1);  // the next float up
  double m = up == INFINITY ? (double)tm + 0x1p103 : ((double)tm + (double)up) * 0.5;  // (FLT_MAX: half its ulp above)
  if (!((float)m <= tm)) {  // the double just below m (m is not 0: it lies strictly between two floats)
    const long long mb = __double_as_longlong(m);
    m = __longlong_as_double(m > 0.0 ? mb - 1 : mb + 1);
  }
  return m;
}

template <uint32_t F, bool LIST = false>
__device__ __forceinline__ void occlusion_body(const OcclusionParams &p, const OcclusionList &l = OcclusionList{}) {
  constexpr bool DT = (F & F_SPHERE) != 0;
  typedef typename TSel<DT>::type T;
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  const SceneDev &sc = p.sc;
  const LaunchCfg &lc = p.lc;
  const QueryLds q = query_stage<F>(sc, lc, smem);
  unsigned long long *counts = p.counts;
  if (counts == nullptr) {
    counts = reinterpret_cast<unsigned long long *>(smem + p.dummy_off);
    if (threadIdx.x == 0) counts[0] = 0ull, counts[1] = 0ull;
  }
  __syncthreads();
#ifdef RTMI_STATS
  MeshStats st{};
#endif

  // ---- 64 consecutive rays per wave, the waves striding over the batch (as query_body.h).  LIST: 64 consecutive
  // entries -- chunk c of the list is one wave's, lane l taking entry 64c + l, and wave w of the grid's W walks chunks
  // w, w + W, ... up to the count on the device, as bounce_list_kernel does: no cursor, no atomic.
  const int lane = (int)(threadIdx.x & 63u);
  // (LIST: the wave's number through readfirstlane, so that the chunk's base, the loop's control and the count stay scalar.
  // The list kernels then take no more VGPRs than their twins in the product build, and occlusion_list_kernel<26> of the
  // diagnostic build 127 where it took 129 against its twin's 128, one occupancy step down.  The plain kernel keeps its
  // expression: it stays instruction for instruction what it was.)
  const int64_t wave = LIST ? (int64_t)blockIdx.x * (blockDim.x >> 6) + __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6))
                            : (int64_t)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
  const int64_t stride = (int64_t)gridDim.x * (blockDim.x >> 6) * 64;
  const bool all_lanes_in = (F & F_BVH) || ((F & F_TRIS) && q.ll != nullptr && sc.n_pairs >= kCullMinPairs) ||
                            ((F & F_SGROUP) && q.cands != nullptr);  // wave-uniform
  int64_t end = p.n;
  if constexpr (LIST) {
    // path_list.h's rule in this site's own text, here and where the entry is looked up below: the end is formed in 64
    // bits, and with list_end and list_entry all eight occlusion_list_kernel<F> compiled to other instructions.
    end = (int64_t)l.n_list;
    if (l.count != nullptr) {  // (wave-uniform: one word, read once per wave)
      const int64_t c = (int64_t)*l.count;
      end = c < end ? c : end;
    }
  }
  for (int64_t base = wave * 64; base < end; base += stride) {
    int64_t i = base + lane;
    bool cand = i < end;
    if constexpr (LIST) {
      if (cand) {
        const uint32_t item = l.list != nullptr ? l.list[i] : (uint32_t)i;
        cand = (int64_t)item < p.n;  // (an entry that is no path is dropped before anything is addressed with it)
        i = (int64_t)item;
      }
      if (__builtin_amdgcn_ballot_w64(cand) == 0ull) continue;  // no path in this chunk: on to the wave's next at once
    }
    V3 o = splat(0.f), d = mk(0.f, 0.f, 1.f);  // (a lane without a usable ray carries a harmless one)
    bool live = false;
    float tm = INFINITY;
    if (cand) {
      const V3 ro = mk(p.origins[i * 3], p.origins[i * 3 + 1], p.origins[i * 3 + 2]);
      const V3 rd = mk(p.dirs[i * 3], p.dirs[i * 3 + 1], p.dirs[i * 3 + 2]);
      live = finite3(ro) && finite3(rd) && (rd.x != 0.f || rd.y != 0.f || rd.z != 0.f);
      if (live) o = ro, d = rd;
      if (p.t_max != nullptr) tm = p.t_max[i];
    }
    d = unit3_rn(d);  // Ray's constructor (ray.cu:8-10)
    if (live && !(finite3(d) && (d.x != 0.f || d.y != 0.f || d.z != 0.f))) {  // |d|^2 over- or underflowed
      live = false;
      o = splat(0.f), d = mk(0.f, 0.f, 1.f);
    }
    live = live && tm == tm;  // a NaN t_max keeps nothing: clear, and nothing to trace
    const double seed = occlusion_seed<T>(tm);
    const bool near = o.x >= p.near_lo[0] && o.x <= p.near_hi[0] && o.y >= p.near_lo[1] && o.y <= p.near_hi[1] &&
                      o.z >= p.near_lo[2] && o.z <= p.near_hi[2];  // (only the start of pass 0 depends on it)
    const double start0 = near && !(tm < p.near_short) ? (double)INFINITY : seed;
    bool occ = false, unc = false;
#pragma nounroll
    for (int pass = 0; pass < 2; pass++) {
      const bool go = pass == 0 ? live : live && unc && !occ;
      if (pass == 1) {  // (wave-uniform) the exact fallback, only when some lane of the wave needs it
        const unsigned long long nf = __builtin_amdgcn_ballot_w64(go);
        if (nf == 0ull) break;
        if (lane == 0) atomicAdd(&counts[1], (unsigned long long)__popcll(nf));
      }
      const double start = pass == 0 ? start0 : (double)INFINITY;
      Hit h = {};
      if (all_lanes_in)  // every lane goes in, with or without a ray of its own
        h = closest_hit<F, true>(sc, q.s_nodes, lc.lds_nodes, q.s_paths, lc.lds_paths, q.s_tris, q.ll, q.cands, q.wl,
                                 counts, o, d, go, false
#ifdef RTMI_STATS
                                 , st
#endif
                                 , start, seed, &unc);
      else if (go)
        h = closest_hit<F, true>(sc, q.s_nodes, 0, q.s_paths, 0, q.s_tris, nullptr, nullptr, nullptr, nullptr, o, d, true,
                                 false
#ifdef RTMI_STATS
                                 , st
#endif
                                 , start, seed, &unc);
      occ = occ || (go && h.ok && h.t <= tm);  // rtmi_intersect's filter
    }
    if constexpr (LIST) {
      if (cand) p.occluded[i] = occ ? 1 : 0;  // (ahead of the diagnostic build's second answer: i is not held across it)
    }
#ifdef RTMI_CHECK_MARGINS
    // Diagnostic build: every ray answered a second time by the unculled engine from +inf, then the filter;
    // p.check[0] += rays re-done, [1] += disagreements.
    {
      Hit h2 = {};
      if (all_lanes_in)
        h2 = closest_hit<F>(sc, q.s_nodes, 0, q.s_paths, 0, nullptr, nullptr, nullptr, nullptr, nullptr, o, d, live, false
#ifdef RTMI_STATS
                            , st
#endif
        );
      else if (live)
        h2 = closest_hit<F>(sc, q.s_nodes, 0, q.s_paths, 0, nullptr, nullptr, nullptr, nullptr, nullptr, o, d, true, false
#ifdef RTMI_STATS
                            , st
#endif
        );
      const bool occ2 = live && h2.ok && h2.t <= tm;
      const unsigned long long na = __builtin_amdgcn_ballot_w64(cand), nd = __builtin_amdgcn_ballot_w64(occ2 != occ);
      if (lane == 0 && p.check != nullptr) {
        if (na) atomicAdd(&p.check[0], (unsigned long long)__popcll(na));
        if (nd) atomicAdd(&p.check[1], (unsigned long long)__popcll(nd));
      }
    }
#endif
    if constexpr (!LIST) {
      if (cand) p.occluded[i] = occ ? 1 : 0;
    }
  }
}
