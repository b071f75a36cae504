// Next-event estimation for wavefront paths (rtmi_direct_sample, rtmi_path_fold_direct; include/rtmi.h "direct" states
// the rule operation by operation).  The scene's light table -- the world-list triangles and parallelograms whose material
// is a DiffuseLight on a constant texture -- is made on the host at commit (direct.hip: build_light_table); the step
// kernel below picks one light per path by its share of area x emission, a point on it, and leaves the shadow ray and the
// unoccluded contribution; rtmi_occluded answers the shadow rays and the fold adds what is visible.
// rtmi_direct_sample_mis is the same body with the balance heuristic (direct_body<true>): the light sample and the
// emission the scattered ray finds on a table light are both kept, weighted a / (a + d2) each from its own side.
// direct_body<MIS, true> are the twins of a scene whose table holds sphere lights (rtmi_scene_light_kinds; records of
// kind 2): such a light is sampled uniformly in the cone it subtends from the vertex, see sphere_cone below.
//
// Every operation is one binary32 rounding in the order written (the translation unit is compiled with
// -ffp-contract=off; division and sqrt are IEEE): tests/directlib.py restates the step in numpy and the two agree bit for
// bit.
#pragma once
#include <stdint.h>

#include "scene_dev.h"
#include "vec.h"
#include "xorwow.h"

namespace rtmi {

#include "path_list.h"

// One light, 128 aligned bytes.  The step gathers the first 80 per lane as five 16-byte loads: words 0..15 the geometry,
// emission and scale, words 16..19 the kind.  The rest is the host's (rtmi_scene_lights) and travels along so that one
// record says everything about a light.
struct alignas(128) LightRec {
  float p0[3], e1[3], e2[3], n[3];  // the pair's first HotTri, bit for bit
  float emission[3];
  float scale;     // area / (selection probability * pi)
  int32_t kind;    // 0 parallelogram (p0 + u e1 + v e2), 1 triangle, 2 sphere (p0 the centre, e1 = {R, R * R, 0}, e2 = n = 0)
  int32_t material, entry, element;
  float area, cdf;
  int32_t pad[10];
};
static_assert(sizeof(LightRec) == 128, "LightRec is 128 bytes");

// The table as rtmi_direct_sample's argument block carries it (32 bytes: DirectArgs keeps its layout).
struct LightTable {
  const LightRec *recs;
  const float *cdf;            // per light, ascending, the last 1.0f: the search reads 4 bytes a probe, not a record
  const uint32_t *light_mats;  // one bit per material: some table light has it
  int32_t n_lights, n_mats;
};

// The light of a hit (rtmi_direct_sample_mis): one row of kHitLightCols words per entry 0 .. n_entries - 1, -1 for none.
// Column f < 6: the table light with that entry and element f (a hit of kind PARALLELEPIPED on face f); column 6: the
// first table light with that entry (a TRIANGLE or PARALLELOGRAM hit, whichever of its triangles, and a SPHERE hit on a
// sphere light); column 7 pads the row to 32 bytes.
constexpr int kHitLightCols = 8;
constexpr int kHitLightAny = 6;

// The table on the device, beside QueryDev: SceneDev keeps its layout.
struct LightDev : LightTable {
  const int32_t *hit_light;  // int32[n_entries][kHitLightCols]
  int32_t n_entries;         // 1 + the largest entry of a table light (0: no table light)
};

// What rtmi_trace_direct's kernels are told behind the trace kernel's block (trace_direct.hip; render_body.h: DIRECT).
struct TraceDirectBufs {
  LightDev ld;
  QueryDev qd;                 // the recording order's names of a hit: the map is looked up by them
  uint32_t *light_states;      // rtmi_trace's layout, stride n: read where a vertex draws, stored back after its draws
  unsigned long long *counts;  // nullable: {vertices sampled, emissions weighed, shadow rays answered occluded}
};

constexpr int kLdsLights = 1024;  // at most this many cdf entries are staged in LDS (4 KiB); longer tables search global memory
constexpr int kDirectThreads = 256;
constexpr int kDirectBlocksPerCu = 8;  // the grid's cap: longer lists are walked in strides of the grid's lanes

struct DirectArgs {
  LightTable lt;
  const MatRec *mats;
  const uint32_t *list, *count;  // rtmi_bounce_list's candidates (both nullable)
  uint32_t n, n_list, step, sample;
  const float *origins, *dirs;
  const int32_t *hits;  // rtmi_hit[n]
  const uint32_t *steps;
  float *emitted;
  const float *attenuation;
  uint32_t *light_states, *flags;
  float *shadow_o, *shadow_d, *shadow_t, *direct;
  unsigned long long *counts;  // nullable
};

// rtmi_direct_sample_mis: the same block, and behind it the hit -> light map and the carry.  The sphere twin of
// rtmi_direct_sample takes it too, for the map, with a null carry.
struct DirectMisArgs : DirectArgs {
  const int32_t *hit_light;
  float *carry;  // float[n][4], 16-byte aligned: the scattered direction and N . d of a path's last sampling vertex
  int32_t n_entries;
};

// A sphere light (centre c, R2 = R * R in binary32) from the point x: wc = c - x, d2c = |wc|^2, whether x lies outside,
// and om = 1 - cos(theta_max) of the cone the sphere subtends, as s2 / (1 + cm) with s2 = R2 / d2c = sin^2 and
// cm = sqrt((d2c - R2) / d2c) = cos: no cancellation for a far or small light (om comes from s2, not from 1 - cm), and
// none for a vertex close to the surface (d2c - R2 is exact there, where 1 - s2 would magnify the rounding of s2: 6.6 ulp
// of om at dc = 1.001 R against 1.3 ulp this way).  Inside (or on) the sphere om is meaningless and `outside` says so.
// The estimator: a direction uniform in that cone has the solid-angle density 1 / (2 pi om), so with P_j the light's
// selection probability the estimate is (albedo / pi) Le cs / (P_j / (2 pi om)) = albedo Le cs om scale_j with
// scale_j = 2 / P_j: no 1 / d2 term, bounded by albedo Le scale_j.  The scattered ray's density cs / pi against the
// light's P_j / (2 pi om) is a : 1 with a = cs om scale_j, so the balance weights are a / (a + 1) for the scattered ray
// and 1 / (a + 1) for the light sample, and pi has cancelled again.
struct SphereCone {
  V3 wc;
  float d2c, om;
  bool outside;
};
__device__ __forceinline__ SphereCone sphere_cone(V3 c, float R2, V3 x) {
  SphereCone k;
  k.wc = c - x;
  k.d2c = dot3(k.wc, k.wc);
  k.outside = k.d2c > R2;
  const float s2 = R2 / k.d2c;
  const float cm = sqrtf((k.d2c - R2) / k.d2c);
  k.om = s2 / (1.f + cm);
  return k;
}

// The smallest j with r0 <= cdf[j]; the last entry is 1 and r0 <= 1, so one exists.  j stays in [0, n - 1] whatever the
// table holds.
__device__ __forceinline__ int light_pick(const float *cdf, int n, float r0) {
  int lo = 0, hi = n - 1;
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (r0 <= cdf[mid]) hi = mid;
    else lo = mid + 1;
  }
  return lo;
}

// MIS = false: rtmi_direct_sample (Args = DirectArgs).  MIS = true: rtmi_direct_sample_mis (Args = DirectMisArgs), the
// balance heuristic between the light sample and the scattered ray: WEIGH takes DROP's place (n_dropped counts the
// emissions weighed) and SAMPLE's g is a / (a + d2) with a = (cs * cl) * scale.
// SPH = true: the twin for a table with sphere lights (Args = DirectMisArgs for both, the plain one's carry null).  The
// draws then depend on the light picked -- a sphere takes r1 and a rejection-sampled point of the unit disc for its
// azimuth, so no sin or cos -- and a SPHERE hit on a sphere light is weighed (MIS) or dropped (plain) by its record,
// from outside only: a vertex inside an emissive sphere cannot sample it and keeps the light it hits.
template <bool MIS, bool SPH = false, class Args>
__device__ __forceinline__ void direct_body(const Args &a, float *s_cdf) {
  const LightTable &lt = a.lt;
  const bool staged = lt.n_lights > 0 && lt.n_lights <= kLdsLights;  // (wave-uniform)
  if (staged) {
    for (int i = (int)threadIdx.x; i < lt.n_lights; i += (int)blockDim.x) s_cdf[i] = lt.cdf[i];
    __syncthreads();
  }
  const PathList pl{a.list, a.count, a.n_list};  // (the block keeps its layout; the rule is path_list.h's)
  const uint32_t end = list_end(pl);
  // chunks of 64 entries by wave number, as bounce_list_kernel takes them: no cursor, no atomic
  const uint32_t lane = threadIdx.x & 63u;
  const uint32_t wave = (uint32_t)__builtin_amdgcn_readfirstlane((int)((blockIdx.x * blockDim.x + threadIdx.x) >> 6));
  const uint32_t stride = gridDim.x * blockDim.x;  // the grid's lanes (a multiple of 64)
  uint32_t n_sampled = 0u, n_dropped = 0u;         // (wave-uniform)
  for (uint64_t at = (uint64_t)wave * 64u; at < end; at += stride) {
    const uint32_t e = (uint32_t)at + lane;
    bool sampled = false, dropped = false;
    uint32_t i = 0u;
    bool cand = e < end;
    if (cand) {
      i = list_entry(pl, e);
      cand = i < a.n;  // (an entry that is no path is dropped)
    }
    if (cand) {
      const int64_t i3 = (int64_t)i * 3;
      V3 wi = splat(0.f), dir = splat(0.f), x = splat(0.f);
      float t_max = 0.f;
      uint32_t flag = a.flags[i];
      const uint32_t was = flag & 1u;
      flag &= ~1u;
      bool valid = false;
      if (a.steps[i] == a.step + 1u) {
        const int4 *hp = reinterpret_cast<const int4 *>(a.hits) + (int64_t)i * 3;
        const int4 h0 = hp[0], h1 = hp[1];  // t u v nx | ny nz material kind  (the third 16 bytes name the hitable)
        const int32_t mat = h1.z, kind = h1.w;
        const bool mat_ok = mat >= 0 && mat < lt.n_mats;
        if constexpr (MIS) {
          const int4 h2 = hp[2];  // entry element reserved
          const int32_t entry = h2.x, face = h2.y;
          // WEIGH (direct_weigh.inc: the rule's one text, rtmi_trace_direct's too), on this step's arrays
#define RTMI_DS_HIT_LIGHT a.hit_light
#define RTMI_DS_N_ENTRIES a.n_entries
#define RTMI_DS_HIT_T __int_as_float(h0.x)
#define RTMI_DS_ORIGIN mk(a.origins[i3 + 0], a.origins[i3 + 1], a.origins[i3 + 2])
#define RTMI_DS_CARRY reinterpret_cast<const float4 *>(a.carry)[i]
#define RTMI_DS_EMITTED mk(a.emitted[i3 + 0], a.emitted[i3 + 1], a.emitted[i3 + 2])
#define RTMI_DS_EMITTED_SET(ex, ey, ez) a.emitted[i3 + 0] = ex, a.emitted[i3 + 1] = ey, a.emitted[i3 + 2] = ez
#include "direct_weigh.inc"
#undef RTMI_DS_HIT_LIGHT
#undef RTMI_DS_N_ENTRIES
#undef RTMI_DS_HIT_T
#undef RTMI_DS_ORIGIN
#undef RTMI_DS_CARRY
#undef RTMI_DS_EMITTED
#undef RTMI_DS_EMITTED_SET
        } else if (was && mat_ok && (kind == QHIT_TRIANGLE || kind == QHIT_PARALLELOGRAM || kind == QHIT_PARALLELEPIPED) &&
            lt.light_mats != nullptr && ((lt.light_mats[mat >> 5] >> (mat & 31)) & 1u)) {
          a.emitted[i3 + 0] = 0.f, a.emitted[i3 + 1] = 0.f, a.emitted[i3 + 2] = 0.f;
          dropped = true;
        }
        if constexpr (SPH && !MIS) {
          // DROP on a sphere light: by its record, and only from outside
          const int32_t entry = hp[2].x;
          if (was && kind == QHIT_SPHERE && entry >= 0 && entry < a.n_entries) {
            const int32_t j = a.hit_light[(int64_t)entry * kHitLightCols + kHitLightAny];
            if (j >= 0 && j < lt.n_lights && reinterpret_cast<const int4 *>(lt.recs + j)[4].x == 2) {
              const float4 *lp = reinterpret_cast<const float4 *>(lt.recs + j);
              const float4 l0 = lp[0], l1 = lp[1];
              if (sphere_cone(mk(l0.x, l0.y, l0.z), l1.x, mk(a.origins[i3 + 0], a.origins[i3 + 1], a.origins[i3 + 2])).outside) {
                a.emitted[i3 + 0] = 0.f, a.emitted[i3 + 1] = 0.f, a.emitted[i3 + 2] = 0.f;
                dropped = true;
              }
            }
          }
        }
        const V3 d = mk(a.dirs[i3 + 0], a.dirs[i3 + 1], a.dirs[i3 + 2]);
        const bool scattered = d.x != 0.f || d.y != 0.f || d.z != 0.f;
        if (a.sample != 0u && lt.n_lights > 0 && scattered && mat_ok && a.mats[mat].kind == MAT_LAMBERTIAN) {
          sampled = true;
          flag |= 1u;
          // SAMPLE (direct_sample.inc: the rule's one text, rtmi_trace_direct's too), on this step's arrays
#define RTMI_DS_STATE(k) a.light_states[k * (int64_t)a.n + i]
#define RTMI_DS_ORIGIN mk(a.origins[i3 + 0], a.origins[i3 + 1], a.origins[i3 + 2])
#define RTMI_DS_HIT_N mk(__int_as_float(h0.w), __int_as_float(h1.x), __int_as_float(h1.y))
#define RTMI_DS_ATTENUATION mk(a.attenuation[i3 + 0], a.attenuation[i3 + 1], a.attenuation[i3 + 2])
#include "direct_sample.inc"
#undef RTMI_DS_STATE
#undef RTMI_DS_ORIGIN
#undef RTMI_DS_HIT_N
#undef RTMI_DS_ATTENUATION
          if constexpr (MIS) reinterpret_cast<float4 *>(a.carry)[i] = make_float4(d.x, d.y, d.z, dot3(N, d));
        }
      }
      if (valid) a.shadow_o[i3 + 0] = x.x, a.shadow_o[i3 + 1] = x.y, a.shadow_o[i3 + 2] = x.z;
      a.shadow_d[i3 + 0] = wi.x, a.shadow_d[i3 + 1] = wi.y, a.shadow_d[i3 + 2] = wi.z;
      a.shadow_t[i] = t_max;
      a.direct[i3 + 0] = dir.x, a.direct[i3 + 1] = dir.y, a.direct[i3 + 2] = dir.z;
      a.flags[i] = flag;
    }
    n_sampled += (uint32_t)__popcll(__builtin_amdgcn_ballot_w64(sampled));
    n_dropped += (uint32_t)__popcll(__builtin_amdgcn_ballot_w64(dropped));
  }
  // the two counters, once per wave: one vector atomic each from lane 0
  if (a.counts && lane == 0u) {
    if (n_sampled) atomicAdd(&a.counts[0], (unsigned long long)n_sampled);
    if (n_dropped) atomicAdd(&a.counts[1], (unsigned long long)n_dropped);
  }
}

// rtmi_path_fold with T[k] = occluded[k] ? E[k] : E[k] + D[k] wherever that fold reads E[k].
__device__ __forceinline__ V3 fold_term(const float *e, const float *d, uint8_t occ) {
  V3 t = mk(e[0], e[1], e[2]);
  if (!occ) t = t + mk(d[0], d[1], d[2]);
  return t;
}

}  // namespace rtmi
