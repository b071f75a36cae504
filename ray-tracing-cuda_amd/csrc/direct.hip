// Next-event estimation for wavefront paths: the light table (host, at commit), the step kernel and the fold
// (rtmi_direct_sample, rtmi_direct_sample_mis, rtmi_path_fold_direct; direct_body.h).  A translation unit of its own: no kernel of another unit is
// compiled differently for it.
#include "direct_body.h"

#include <math.h>
#include <string.h>

#include "kernels.h"
#include "scene.h"

namespace rtmi {

static inline int64_t cdiv64(int64_t a, int64_t b) { return (a + b - 1) / b; }

// ------------------------------------------------------------------ the light table
// One record per pair of `tris` (a Parallelogram, a face of a Parallelepiped, a lone Triangle) whose material is a
// DiffuseLight on a constant texture with finite, not all zero components and whose e1 x e2 is finite and non-zero, in
// the order of the pairs.  Everything that is not binary32 data of the scene is formed in binary64 and rounded once
// (include/rtmi.h states the expressions; tests/directlib.py restates them).
// A scene that opted in (rtmi_scene_light_kinds with RTMI_LIGHTS_SPHERES) gets, behind those, one record of kind 2 per
// Sphere on such a material with a finite centre and a finite radius > 0 whose binary32 R and R * R are finite and > 0,
// in the order of the flattened spheres (tests/spherelightlib.py restates them).  No material bit is set for them: a
// sphere light is known by its record.
void build_light_table(const Scene &s, std::vector<rtmi_light> *lights, std::vector<uint32_t> *light_mats) {
  lights->clear();
  light_mats->assign((s.mat_recs.size() + 31) / 32, 0u);
  std::vector<double> area, w;
  const size_t n_pairs = s.tris.size() / 2;
  for (size_t p = 0; p < n_pairs && 2 * p + 1 < s.q_pair_entry.size(); p++) {
    const HotTri &t = s.tris[2 * p];
    if (t.mat < 0 || t.mat >= (int32_t)s.mat_recs.size()) continue;
    const MatRec &m = s.mat_recs[(size_t)t.mat];
    if (m.kind != MAT_LIGHT || m.tex >= 0) continue;
    if (!(std::isfinite(m.r) && std::isfinite(m.g) && std::isfinite(m.b)) || (m.r == 0.f && m.g == 0.f && m.b == 0.f)) continue;
    const double a[3] = {t.e1[0], t.e1[1], t.e1[2]}, b[3] = {t.e2[0], t.e2[1], t.e2[2]};
    const double cx = a[1] * b[2] - b[1] * a[2], cy = a[2] * b[0] - b[2] * a[0], cz = a[0] * b[1] - b[0] * a[1];
    if (!(std::isfinite(cx) && std::isfinite(cy) && std::isfinite(cz)) || (cx == 0. && cy == 0. && cz == 0.)) continue;
    const int32_t kind = s.q_pair_entry[2 * p + 1] & 0xff, face = s.q_pair_entry[2 * p + 1] >> 8;
    const double len = std::sqrt((cx * cx + cy * cy) + cz * cz);
    const double ar = kind == QHIT_TRIANGLE ? 0.5 * len : len;
    rtmi_light l;
    memset(&l, 0, sizeof(l));
    memcpy(l.p0, t.p0, sizeof(l.p0)), memcpy(l.e1, t.e1, sizeof(l.e1)), memcpy(l.e2, t.e2, sizeof(l.e2)), memcpy(l.n, t.n, sizeof(l.n));
    l.emission[0] = m.r, l.emission[1] = m.g, l.emission[2] = m.b;
    l.area = (float)ar;
    l.kind = kind == QHIT_TRIANGLE ? 1 : 0;
    l.entry = s.q_pair_entry[2 * p];
    l.element = kind == QHIT_PARALLELEPIPED ? face : 0;
    l.material = t.mat;
    lights->push_back(l);
    area.push_back(ar);
    w.push_back(ar * ((std::fabs((double)m.r) + std::fabs((double)m.g)) + std::fabs((double)m.b)));
    (*light_mats)[(size_t)t.mat >> 5] |= 1u << (t.mat & 31);
  }
  const size_t n_flat = lights->size();
  for (size_t i = 0; (s.light_kinds & RTMI_LIGHTS_SPHERES) && i < s.q_sphere_entry.size() && i < s.spheres.size(); i++) {
    const SphereRec &sp = s.spheres[i];
    if (sp.mat < 0 || sp.mat >= (int32_t)s.mat_recs.size()) continue;
    const MatRec &m = s.mat_recs[(size_t)sp.mat];
    if (m.kind != MAT_LIGHT || m.tex >= 0) continue;
    if (!(std::isfinite(m.r) && std::isfinite(m.g) && std::isfinite(m.b)) || (m.r == 0.f && m.g == 0.f && m.b == 0.f)) continue;
    if (!(std::isfinite(sp.cx) && std::isfinite(sp.cy) && std::isfinite(sp.cz))) continue;
    const double r = sp.radius;
    if (!(std::isfinite(r) && r > 0.)) continue;
    const float R = (float)r;
    const float R2 = R * R;
    if (!(std::isfinite(R) && R > 0.f && std::isfinite(R2) && R2 > 0.f)) continue;
    const double ar = 4 * M_PI * r * r;
    rtmi_light l;
    memset(&l, 0, sizeof(l));
    l.p0[0] = sp.cx, l.p0[1] = sp.cy, l.p0[2] = sp.cz;
    l.e1[0] = R, l.e1[1] = R2;
    l.emission[0] = m.r, l.emission[1] = m.g, l.emission[2] = m.b;
    l.area = (float)ar;
    l.kind = 2;
    l.entry = s.q_sphere_entry[i];
    l.element = 0;
    l.material = sp.mat;
    lights->push_back(l);
    area.push_back(ar);
    w.push_back(ar * ((std::fabs((double)m.r) + std::fabs((double)m.g)) + std::fabs((double)m.b)));
  }
  double W = 0.;
  for (double x : w) W += x;
  double run = 0.;
  for (size_t j = 0; j < lights->size(); j++) {
    run += w[j];
    (*lights)[j].cdf = (float)(run / W);
    // a sphere is sampled by solid angle: 2 / P_j takes the place of area / (P_j pi)
    (*lights)[j].scale = j < n_flat ? (float)(area[j] * W / (w[j] * M_PI)) : (float)(2 * W / w[j]);
  }
  if (!lights->empty()) lights->back().cdf = 1.0f;
}

// The device form of the table (direct_body.h: LightRec): the same words, the record padded to 128 bytes.
void light_records(const std::vector<rtmi_light> &lights, std::vector<LightRec> *recs, std::vector<float> *cdf) {
  recs->clear(), cdf->clear();
  for (const rtmi_light &l : lights) {
    LightRec r;
    memset(&r, 0, sizeof(r));
    memcpy(r.p0, l.p0, sizeof(r.p0)), memcpy(r.e1, l.e1, sizeof(r.e1)), memcpy(r.e2, l.e2, sizeof(r.e2)), memcpy(r.n, l.n, sizeof(r.n));
    memcpy(r.emission, l.emission, sizeof(r.emission));
    r.scale = l.scale, r.kind = l.kind, r.material = l.material, r.entry = l.entry, r.element = l.element;
    r.area = l.area, r.cdf = l.cdf;
    recs->push_back(r);
    cdf->push_back(l.cdf);
  }
}

// The light of a hit (rtmi_direct_sample_mis; direct_body.h: LightDev::hit_light): per entry up to the largest one of a
// table light, the light of each box face and the first light of the entry, -1 where there is none.
void build_hit_light_map(const std::vector<rtmi_light> &lights, std::vector<int32_t> *map, int32_t *n_entries) {
  int32_t rows = 0;
  for (const rtmi_light &l : lights)
    if (l.entry >= rows) rows = l.entry + 1;
  map->assign((size_t)rows * kHitLightCols, -1);
  for (size_t j = 0; j < lights.size(); j++) {
    const rtmi_light &l = lights[j];
    if (l.entry < 0) continue;
    int32_t *row = map->data() + (size_t)l.entry * kHitLightCols;
    if (l.element >= 0 && l.element < kHitLightAny && row[l.element] < 0) row[l.element] = (int32_t)j;
    if (row[kHitLightAny] < 0) row[kHitLightAny] = (int32_t)j;
  }
  *n_entries = rows;
}

// ------------------------------------------------------------------ the step (rtmi_direct_sample)
__global__ __launch_bounds__(kDirectThreads) void direct_sample_kernel(DirectArgs a) {
  __shared__ float s_cdf[kLdsLights];
  direct_body<false>(a, s_cdf);
}

// rtmi_direct_sample_mis: the same body with the balance heuristic's weights.
__global__ __launch_bounds__(kDirectThreads) void direct_sample_mis_kernel(DirectMisArgs a) {
  __shared__ float s_cdf[kLdsLights];
  direct_body<true>(a, s_cdf);
}

// The twins for a table with sphere lights (direct_body.h: SPH): the only kernels such a scene's steps launch, and no
// other scene launches them.
__global__ __launch_bounds__(kDirectThreads) void direct_sample_sph_kernel(DirectMisArgs a) {
  __shared__ float s_cdf[kLdsLights];
  direct_body<false, true>(a, s_cdf);
}
__global__ __launch_bounds__(kDirectThreads) void direct_sample_mis_sph_kernel(DirectMisArgs a) {
  __shared__ float s_cdf[kLdsLights];
  direct_body<true, true>(a, s_cdf);
}

// One lane per candidate: list_grid (kernels.h) over the host's bound n_list -- 2^19 entries a round on 256 compute units.
template <auto Kernel, class Args>
static hipError_t direct_launch(const Args &a, int n_cu, hipStream_t stream) {
  hipLaunchKernelGGL(Kernel, dim3(list_grid(a.n_list, kDirectThreads, n_cu, kDirectBlocksPerCu)), dim3(kDirectThreads), 0, stream, a);
  return hipGetLastError();
}
hipError_t launch_direct_sample(const DirectArgs &a, int n_cu, hipStream_t stream) {
  return direct_launch<direct_sample_kernel>(a, n_cu, stream);
}
hipError_t launch_direct_sample_mis(const DirectMisArgs &a, int n_cu, hipStream_t stream) {
  return direct_launch<direct_sample_mis_kernel>(a, n_cu, stream);
}
hipError_t launch_direct_sample_sph(const DirectMisArgs &a, bool mis, int n_cu, hipStream_t stream) {
  return mis ? direct_launch<direct_sample_mis_sph_kernel>(a, n_cu, stream) : direct_launch<direct_sample_sph_kernel>(a, n_cu, stream);
}

// ------------------------------------------------------------------ the fold (rtmi_path_fold_direct)
// path_fold_kernel (paths.hip) with T[k] for E[k]: one lane per path, a layer's reads coalesced over n.
__global__ __launch_bounds__(256) void path_fold_direct_kernel(int64_t n, uint32_t layers, const float *__restrict__ dirs,
                                                                const uint32_t *__restrict__ steps, const float *__restrict__ emitted,
                                                                const float *__restrict__ attenuation, const float *__restrict__ direct,
                                                                const uint8_t *__restrict__ occluded, float *__restrict__ radiance) {
  const int64_t q = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (q >= n) return;
  const uint32_t s = steps[q];
  int k = (int)(s < layers ? s : layers) - 1;
  V3 r = splat(0.f);
  if (k >= 0 && dirs[q * 3 + 0] == 0.f && dirs[q * 3 + 1] == 0.f && dirs[q * 3 + 2] == 0.f) {  // the path ended in layer k
    const int64_t at = (int64_t)k * n + q;
    r = fold_term(emitted + at * 3, direct + at * 3, occluded[at]);
    k--;
  }
  for (; k >= 0; k--) {
    const int64_t at = (int64_t)k * n + q;
    const V3 t = fold_term(emitted + at * 3, direct + at * 3, occluded[at]);
    const float *a = attenuation + at * 3;
    r = mk(t.x + a[0] * r.x, t.y + a[1] * r.y, t.z + a[2] * r.z);
  }
  radiance[q * 3 + 0] = r.x, radiance[q * 3 + 1] = r.y, radiance[q * 3 + 2] = r.z;
}
hipError_t launch_path_fold_direct(int64_t n, int layers, const float *d_dirs, const uint32_t *d_steps, const float *d_emitted,
                                   const float *d_attenuation, const float *d_direct, const uint8_t *d_occluded,
                                   float *d_radiance, hipStream_t stream) {
  if (n == 0) return hipSuccess;
  hipLaunchKernelGGL(path_fold_direct_kernel, dim3((unsigned)cdiv64(n, 256)), dim3(256), 0, stream, n, (uint32_t)layers, d_dirs,
                     d_steps, d_emitted, d_attenuation, d_direct, d_occluded, d_radiance);
  return hipGetLastError();
}

}  // namespace rtmi
