// Batched closest-hit queries on caller-made rays (rtmi_intersect).  Included by kernels.hip inside namespace rtmi,
// after render_body.h (not a stand-alone header).
//
// The engine is the render's: closest_hit<F> unchanged, called as the trace loop calls it, with the same LDS staging
// in front of it.  What differs is around it -- a wave takes 64 consecutive rays of the batch instead of pixels from a
// queue, and the winner is written out as an rtmi_hit instead of being shaded.
#pragma once

// Everything the query kernel is told: one by-value argument block.
struct QueryParams {
  SceneDev sc;
  QueryDev qd;
  LaunchCfg lc;               // make_cfg without an id stack; only the staging offsets are used
  int64_t n;                  // rays
  const float *origins, *dirs;
  const float *t_max;         // nullable
  int32_t *hits;              // n x 12 words (rtmi_hit)
  unsigned long long *abandoned;  // nullable: then the wave's word in LDS takes the count (query_lds_extra)
  unsigned long long *check;      // -DRTMI_CHECK_MARGINS: nullable, {re-done, disagreements}; else unused
  int32_t dummy_off;          // byte offset in dynamic LDS of a word that stands in for a null `abandoned`
};
constexpr size_t kQueryLdsExtra = 16;  // bytes behind make_cfg's layout: the stand-in words (of the occlusion kernel too)

// What Trace makes of the winner (render_body.h, after closest_hit), as a record: the oriented normal of a triangle
// (utils.cu:80), the parallelogram's remapped u, v (parallelogram.cu:26-29,35-38), the sphere's normal and GetUV
// (sphere.cu:25-26,60-63), a mesh face's normal and interpolated texture coordinates (utils.cu:79, bvh.cuh:41-45) --
// and the recording order's names for it (QueryDev).
struct QueryHit {
  float t, u, v;
  V3 n;
  int32_t mat, kind, entry, element;
};
template <uint32_t F>
__device__ __forceinline__ QueryHit resolve_hit(const SceneDev &sc, const QueryDev &qd, const Hit &h, V3 o, V3 d) {
  QueryHit r;
  r.t = INFINITY, r.u = 0.f, r.v = 0.f, r.n = splat(0.f);
  r.mat = -1, r.kind = QHIT_NONE, r.entry = -1, r.element = 0;
  if (!h.ok) return r;
  const uint32_t kind = h.win >> 29;
  const uint32_t index = h.win & ID_INDEX_MASK;
  r.t = h.t;
  if (kind == RUN_SKY) {  // sky.cu:18-27: t only (normal, u, v are left as they were)
    r.kind = QHIT_SKY, r.entry = qd.sky_entry;
    return r;
  }
  if ((F & F_TRIS) && kind == RUN_TRIS) {
    const HotTri &tr = sc.tris[index];
    const V3 n = mk(tr.n[0], tr.n[1], tr.n[2]);
    r.n = dot3(d, n) < 0.f ? n : -n;  // utils.cu:80
    r.mat = tr.mat;
    if (tr.flags & TRI_PGRAM) {  // parallelogram.cu:26-29,35-38
      const float w = (float)((1.0 - (double)h.u) - (double)h.v);
      if (!(tr.flags & TRI_SECOND)) {
        r.u = (0.f * w + 1.f * h.u) + 0.f * h.v;
        r.v = (1.f * w + 1.f * h.u) + 0.f * h.v;
      } else {
        r.u = (1.f * w + 0.f * h.u) + 1.f * h.v;
        r.v = (1.f * w + 0.f * h.u) + 0.f * h.v;
      }
    } else {
      r.u = h.u, r.v = h.v;  // triangle.cu:13
    }
    const int32_t info = qd.pair_entry[(index >> 1) * 2 + 1];
    r.entry = qd.pair_entry[(index >> 1) * 2];
    r.kind = info & 0xff;
    r.element = r.kind == QHIT_PARALLELEPIPED ? (info >> 8) : r.kind == QHIT_PARALLELOGRAM ? (int32_t)(index & 1u) : 0;
  }
  if ((F & F_SPHERE) && kind == RUN_SPHERE) {
    const SphereRec &sr = sc.spheres[index];
    const V3 p = o + h.t * d;  // ray_tracing.cu:32
    r.n = unit3_rn(p - mk(sr.cx, sr.cy, sr.cz));  // sphere.cu:25-26
    r.mat = sr.mat;
    const float pi_f = 3.14159265358979323846264338327950288f;  // sphere.cu:60-63
    const float theta = acosf(-r.n.y);
    const float phi = atan2f(-r.n.z, r.n.x) + pi_f;
    r.u = phi / (2 * pi_f);
    r.v = theta / pi_f;
    r.kind = QHIT_SPHERE, r.entry = qd.sphere_entry[index];
  }
  if ((F & F_BVH) && kind == RUN_BVH) {
    const FaceRec &fc = sc.faces[index];
    const V3 n = unit3_rn(cross3(mk(fc.e1[0], fc.e1[1], fc.e1[2]), mk(fc.e2[0], fc.e2[1], fc.e2[2])));  // utils.cu:79
    r.n = dot3(d, n) < 0.f ? n : -n;
    const BvhRec br = sc.bvhs[h.aux];
    r.mat = br.mat;
    if (br.has_uv) {  // bvh.cuh:41-45
      const float *tc = sc.face_uv + (size_t)(br.face_base + fc.orig) * 6;
      const float w = (float)((1.0 - (double)h.u) - (double)h.v);
      r.u = (tc[0] * w + tc[2] * h.u) + tc[4] * h.v;
      r.v = (tc[1] * w + tc[3] * h.u) + tc[5] * h.v;
    }
    r.kind = QHIT_MESH, r.entry = qd.bvh_entry[h.aux], r.element = qd.face_input[index];
  }
  return r;
}

template <uint32_t F>
__device__ __forceinline__ void query_body(const QueryParams &qp) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  const SceneDev &sc = qp.sc;
  const LaunchCfg &lc = qp.lc;
  // ---- staging: as render_body.h's prologue (materials are not read: nothing is shaded).  occlusion_body.h has the
  // same staging as a function (query_stage): a change here is a change there.
  const BvhNode *s_nodes = reinterpret_cast<const BvhNode *>(smem + lc.nodes_off);
  int *wl = nullptr;
  if (F & F_BVH)
    wl = reinterpret_cast<int *>(smem + lc.mesh_off) + __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)) * kMeshWaveWords;
  const float4 *s_tris = nullptr;
  if ((F & F_TRIS) && lc.pairs_off >= 0) {
    s_tris = reinterpret_cast<const float4 *>(smem + lc.pairs_off);
    const uint32_t *src = reinterpret_cast<const uint32_t *>(sc.tri_pts);
    uint32_t *dst = reinterpret_cast<uint32_t *>(smem + lc.pairs_off);
    for (int w = threadIdx.x; w < sc.n_pairs * 24; w += blockDim.x) dst[w] = src[w];
  }
  int *ll = nullptr;
  if ((F & (F_TRIS | F_SGROUP)) && lc.list_off >= 0)
    ll = reinterpret_cast<int *>(smem + lc.list_off) + __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)) * kListWaveWords(F);
  uint16_t *cands = nullptr;
  if ((F & F_SGROUP) && lc.cand_off >= 0)
    cands = reinterpret_cast<uint16_t *>(smem + lc.cand_off) +
            __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)) * (64 * kSphCand + 128);
  if ((F & F_BVH) && lc.lds_nodes > 0) {
    const uint32_t *src = reinterpret_cast<const uint32_t *>(sc.nodes);
    uint32_t *dst = reinterpret_cast<uint32_t *>(smem + lc.nodes_off);
    for (int w = threadIdx.x; w < lc.lds_nodes * 8; w += blockDim.x) dst[w] = src[w];
  }
  const int *s_paths = reinterpret_cast<const int *>(smem + lc.paths_off);
  if ((F & F_BVH) && lc.lds_paths > 0) {
    int *dst = reinterpret_cast<int *>(smem + lc.paths_off);
    for (int w = threadIdx.x; w < lc.lds_paths; w += blockDim.x) dst[w] = sc.leaf_paths[w];
  }
  unsigned long long *abandoned = qp.abandoned;
  if (abandoned == nullptr) abandoned = reinterpret_cast<unsigned long long *>(smem + qp.dummy_off);
  __syncthreads();
#ifdef RTMI_STATS
  MeshStats st{};
#endif

  // ---- 64 consecutive rays per wave, the waves striding over the batch
  const int lane = (int)(threadIdx.x & 63u);
  const int64_t wave = (int64_t)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
  const int64_t stride = (int64_t)gridDim.x * (blockDim.x >> 6) * 64;
  const bool all_lanes_in = (F & F_BVH) || ((F & F_TRIS) && ll != nullptr && sc.n_pairs >= kCullMinPairs) ||
                            ((F & F_SGROUP) && cands != nullptr);  // wave-uniform
  for (int64_t base = wave * 64; base < qp.n; base += stride) {
    const int64_t i = base + lane;
    V3 o = splat(0.f), d = mk(0.f, 0.f, 1.f);  // (a lane without a usable ray carries a harmless one)
    bool live = false;
    if (i < qp.n) {
      const V3 ro = mk(qp.origins[i * 3], qp.origins[i * 3 + 1], qp.origins[i * 3 + 2]);
      const V3 rd = mk(qp.dirs[i * 3], qp.dirs[i * 3 + 1], qp.dirs[i * 3 + 2]);
      live = finite3(ro) && finite3(rd) && (rd.x != 0.f || rd.y != 0.f || rd.z != 0.f);
      if (live) o = ro, d = rd;
    }
    d = unit3_rn(d);  // Ray's constructor (ray.cu:8-10)
    if (live && !(finite3(d) && (d.x != 0.f || d.y != 0.f || d.z != 0.f))) {  // |d|^2 over- or underflowed
      live = false;
      o = splat(0.f), d = mk(0.f, 0.f, 1.f);
    }
    Hit h = {};
    if (all_lanes_in)  // every lane goes in, with or without a ray of its own
      h = closest_hit<F>(sc, s_nodes, lc.lds_nodes, s_paths, lc.lds_paths, s_tris, ll, cands, wl, abandoned, o, d, live, false
#ifdef RTMI_STATS
                         , st
#endif
      );
    else if (live)
      h = closest_hit<F>(sc, s_nodes, 0, s_paths, 0, s_tris, nullptr, nullptr, nullptr, nullptr, o, d, true, false
#ifdef RTMI_STATS
                         , st
#endif
      );
#ifdef RTMI_CHECK_MARGINS
    // Diagnostic build: every query answered a second time without the culls (render_body.h does the same for
    // renders); qp.check[0] += queries re-done, [1] += disagreements.
    {
      Hit h2 = {};
      if (all_lanes_in)
        h2 = closest_hit<F>(sc, s_nodes, 0, s_paths, 0, nullptr, nullptr, nullptr, nullptr, nullptr, o, d, live, false
#ifdef RTMI_STATS
                            , st
#endif
        );
      else if (live)
        h2 = closest_hit<F>(sc, s_nodes, 0, s_paths, 0, nullptr, nullptr, nullptr, nullptr, nullptr, o, d, true, false
#ifdef RTMI_STATS
                            , st
#endif
        );
      const bool differs = live && (h2.ok != h.ok || (h.ok && (__float_as_uint(h2.t) != __float_as_uint(h.t) || h2.win != h.win ||
                                                             ((F & F_BVH) && h2.aux != h.aux))));
      const unsigned long long na = __builtin_amdgcn_ballot_w64(live), nd = __builtin_amdgcn_ballot_w64(differs);
      if (lane == 0 && qp.check != nullptr) {
        if (na) atomicAdd(&qp.check[0], (unsigned long long)__popcll(na));
        if (nd) atomicAdd(&qp.check[1], (unsigned long long)__popcll(nd));
      }
    }
#endif
    if (i < qp.n) {
      if (!live) h.ok = false;
      QueryHit r = resolve_hit<F>(sc, qp.qd, h, o, d);
      if (r.kind != QHIT_NONE && qp.t_max != nullptr && !(r.t <= qp.t_max[i])) {  // a filter on the closest hit
        r.t = INFINITY, r.u = 0.f, r.v = 0.f, r.n = splat(0.f);
        r.mat = -1, r.kind = QHIT_NONE, r.entry = -1, r.element = 0;
      }
      int4 *out = reinterpret_cast<int4 *>(qp.hits + i * 12);
      out[0] = make_int4(__float_as_int(r.t), __float_as_int(r.u), __float_as_int(r.v), __float_as_int(r.n.x));
      out[1] = make_int4(__float_as_int(r.n.y), __float_as_int(r.n.z), r.mat, r.kind);
      out[2] = make_int4(r.entry, r.element, 0, 0);
    }
  }
}
