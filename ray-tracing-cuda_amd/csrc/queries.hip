// Batched ray queries on a committed scene (rtmi_intersect, rtmi_occluded, rtmi_occluded_list): query_body.h and
// occlusion_body.h around the render's closest_hit, on the query variants, and their launchers.  A translation unit of its
// own: no kernel of render.hip or calls.hip is compiled differently for it.  The LDS layout is render.hip's make_cfg
// (launch_cfg.h).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "kernels.h"

#include <cfloat>
#include <cmath>
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
#include "query_body.h"
#include "occlusion_body.h"
#include "launch_cfg.h"

uint32_t pick_query_variant(uint32_t features) {
  return pick_listed(kQueryVariants, (features & ~(uint32_t)F_DEFOCUS) | F_TEX);
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

}  // namespace rtmi
