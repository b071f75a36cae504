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
          // WEIGH: the light of the hit by its entry (and face), every index checked before it addresses anything
          const int4 h2 = hp[2];  // entry element reserved
          const int32_t entry = h2.x, face = h2.y;
          int32_t col = -1;
          if (kind == QHIT_PARALLELEPIPED) col = face >= 0 && face < kHitLightAny ? face : -1;
          else if (kind == QHIT_TRIANGLE || kind == QHIT_PARALLELOGRAM) col = kHitLightAny;
          if constexpr (SPH)
            if (kind == QHIT_SPHERE) col = kHitLightAny;
          int32_t j = -1;
          if (was && col >= 0 && entry >= 0 && entry < a.n_entries) j = a.hit_light[(int64_t)entry * kHitLightCols + col];
          bool flat = true;
          if constexpr (SPH) {
            if (kind == QHIT_SPHERE) {
              flat = false;
              if (j >= 0 && j < lt.n_lights && reinterpret_cast<const int4 *>(lt.recs + j)[4].x == 2) {
                const float4 *lp = reinterpret_cast<const float4 *>(lt.recs + j);
                const float4 l0 = lp[0], l1 = lp[1], l3 = lp[3];  // c R | R2 .. | emission scale
                const SphereCone k = sphere_cone(mk(l0.x, l0.y, l0.z), l1.x, mk(a.origins[i3 + 0], a.origins[i3 + 1], a.origins[i3 + 2]));
                if (k.outside) {
                  const float av = (reinterpret_cast<const float4 *>(a.carry)[i].w * k.om) * l3.w;
                  const float sum = av + 1.f;
                  const bool div = av > 0.f && sum < INFINITY;
                  const float w = av / sum;
                  const V3 e = mk(a.emitted[i3 + 0], a.emitted[i3 + 1], a.emitted[i3 + 2]);
                  a.emitted[i3 + 0] = div ? e.x * w : 0.f, a.emitted[i3 + 1] = div ? e.y * w : 0.f, a.emitted[i3 + 2] = div ? e.z * w : 0.f;
                  dropped = true;
                }
              }
            }
          }
          if (flat && j >= 0 && j < lt.n_lights) {
            const float4 c = reinterpret_cast<const float4 *>(a.carry)[i];
            const float4 *lp = reinterpret_cast<const float4 *>(lt.recs + j);
            const float4 l2 = lp[2], l3 = lp[3];  // e2.z n | emission scale
            const float cl = fabsf(dot3(mk(l2.y, l2.z, l2.w), mk(c.x, c.y, c.z)));
            const float t = __int_as_float(h0.x);
            const float d2 = t * t;
            const float av = (c.w * cl) * l3.w;
            const float sum = av + d2;
            const bool div = av > 0.f && d2 > 0.f && sum < INFINITY;
            const float w = av / sum;
            const V3 e = mk(a.emitted[i3 + 0], a.emitted[i3 + 1], a.emitted[i3 + 2]);
            a.emitted[i3 + 0] = div ? e.x * w : 0.f, a.emitted[i3 + 1] = div ? e.y * w : 0.f, a.emitted[i3 + 2] = div ? e.z * w : 0.f;
            dropped = true;
          }
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
          Rng rng;
          rng.d = a.light_states[0 * (int64_t)a.n + i], rng.v0 = a.light_states[1 * (int64_t)a.n + i];
          rng.v1 = a.light_states[2 * (int64_t)a.n + i], rng.v2 = a.light_states[3 * (int64_t)a.n + i];
          rng.v3 = a.light_states[4 * (int64_t)a.n + i], rng.v4 = a.light_states[5 * (int64_t)a.n + i];
          const float r0 = rng_range(0.f, 1.f, rng);
          float r1 = rng_range(0.f, 1.f, rng);
          float r2 = 0.f;
          if constexpr (!SPH) {
            r2 = rng_range(0.f, 1.f, rng);
            a.light_states[0 * (int64_t)a.n + i] = rng.d, a.light_states[1 * (int64_t)a.n + i] = rng.v0;
            a.light_states[2 * (int64_t)a.n + i] = rng.v1, a.light_states[3 * (int64_t)a.n + i] = rng.v2;
            a.light_states[4 * (int64_t)a.n + i] = rng.v3, a.light_states[5 * (int64_t)a.n + i] = rng.v4;
          }
          const int j = staged ? light_pick(s_cdf, lt.n_lights, r0) : light_pick(lt.cdf, lt.n_lights, r0);
          const float4 *lp = reinterpret_cast<const float4 *>(lt.recs + j);
          const float4 l0 = lp[0], l1 = lp[1], l2 = lp[2], l3 = lp[3];  // p0 e1.x | e1.yz e2.xy | e2.z n | emission scale
          const int4 l4 = reinterpret_cast<const int4 *>(lt.recs + j)[4];
          const V3 N = mk(__int_as_float(h0.w), __int_as_float(h1.x), __int_as_float(h1.y));
          bool sph = false;
          if constexpr (SPH) {
            // a sphere light takes r1 and a point of the unit disc by rejection (the Lambertian ball sampler's kind of loop:
            // no trip cap), every draw before any validity test; a flat light takes r2 as ever
            sph = l4.x == 2;
            float cp = 0.f, sp = 0.f;
            if (sph) {
              float da, db, s2d;
              do {
                da = rng_range(-1.f, 1.f, rng);
                db = rng_range(-1.f, 1.f, rng);
                s2d = da * da + db * db;
              } while (!(s2d > 0.f && s2d <= 1.f));
              const float ls = sqrtf(s2d);
              cp = da / ls, sp = db / ls;
            } else {
              r2 = rng_range(0.f, 1.f, rng);
            }
            a.light_states[0 * (int64_t)a.n + i] = rng.d, a.light_states[1 * (int64_t)a.n + i] = rng.v0;
            a.light_states[2 * (int64_t)a.n + i] = rng.v1, a.light_states[3 * (int64_t)a.n + i] = rng.v2;
            a.light_states[4 * (int64_t)a.n + i] = rng.v3, a.light_states[5 * (int64_t)a.n + i] = rng.v4;
            if (sph) {
              x = mk(a.origins[i3 + 0], a.origins[i3 + 1], a.origins[i3 + 2]);
              const float R2 = l1.x;
              const SphereCone k = sphere_cone(mk(l0.x, l0.y, l0.z), R2, x);
              const float dc = sqrtf(k.d2c);
              const float h = r1 * k.om;
              const float ct = 1.f - h;
              const float st2 = h * (2.f - h);
              const float st = sqrtf(st2);
              // the cone's axis and Duff et al.'s branch-free frame around it
              const V3 w = k.wc / dc;
              const float sg = w.z >= 0.f ? 1.f : -1.f;
              const float ka = -1.f / (sg + w.z);
              const float kb = (w.x * w.y) * ka;
              const V3 u = mk(1.f + (sg * (w.x * w.x)) * ka, sg * kb, (-sg) * w.x);
              const V3 v = mk(kb, sg + (w.y * w.y) * ka, -w.y);
              const float sc = st * cp, ss = st * sp;
              wi = (ct * w + sc * u) + ss * v;
              // the near intersection of that direction with the sphere
              const float tc = dc * ct;
              float q = R2 - k.d2c * st2;
              q = q > 0.f ? q : 0.f;
              const float t = tc - sqrtf(q);
              const float cs = dot3(N, wi);
              valid = k.outside && cs > 0.f && t > 0.f && t < INFINITY;
              if (valid) {
                const float av = (cs * k.om) * l3.w;
                float g = av;
                if constexpr (MIS) g = av / (av + 1.f);
                const V3 att = mk(a.attenuation[i3 + 0], a.attenuation[i3 + 1], a.attenuation[i3 + 2]);
                dir = (att * mk(l3.x, l3.y, l3.z)) * g;
                t_max = t * 0.999f;
              } else {
                wi = splat(0.f);
              }
            }
          }
          if (!sph) {
            if (l4.x == 1 && r1 + r2 > 1.f) r1 = 1.f - r1, r2 = 1.f - r2;
            const V3 p0 = mk(l0.x, l0.y, l0.z), e1 = mk(l0.w, l1.x, l1.y), e2 = mk(l1.z, l1.w, l2.x), ln = mk(l2.y, l2.z, l2.w);
            const V3 q = (p0 + r1 * e1) + r2 * e2;
            x = mk(a.origins[i3 + 0], a.origins[i3 + 1], a.origins[i3 + 2]);
            const V3 w = q - x;
            const float d2 = dot3(w, w);
            const float dist = sqrtf(d2);
            wi = w / dist;
            const float cs = dot3(N, wi);
            const float cl = fabsf(dot3(ln, wi));
            valid = d2 > 0.f && cs > 0.f && cl > 0.f && dist < INFINITY;
            if (valid) {
              float g;
              if constexpr (MIS) {
                const float av = (cs * cl) * l3.w;
                g = av / (av + d2);
              } else {
                g = ((cs * cl) / d2) * l3.w;
              }
              const V3 att = mk(a.attenuation[i3 + 0], a.attenuation[i3 + 1], a.attenuation[i3 + 2]);
              dir = (att * mk(l3.x, l3.y, l3.z)) * g;
              t_max = dist * 0.999f;
            } else {
              wi = splat(0.f);
            }
          }
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
