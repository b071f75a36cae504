// The entries that own their device state (rtmi_trace, rtmi_render_budget, rtmi_render_features, rtmi_bounce,
// rtmi_bounce_list): render_body.h in a mode of each kernel's, on the query variants, and their one launcher.  A
// translation unit of its own: no kernel of render.hip or queries.hip is compiled differently for it.  The LDS layout
// is render.hip's make_cfg (launch_cfg.h).
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
#include "query_body.h"  // (resolve_hit: a step's hit record)
#include "launch_cfg.h"

// The block of rtmi_trace, rtmi_render_budget and rtmi_render_features sits in the call's own d_work, behind the
// kernel's counter words (launch_call).
static_assert(kCallParamsOffset + sizeof(CallParams) <= (size_t)RTMI_TRACE_WORK_WORDS * 8u,
              "RTMI_TRACE_WORK_WORDS must hold the caller-owned kernels' argument block");
static_assert(kCallParamsOffset % alignof(CallParams) == 0, "the argument block is aligned in d_work");

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

#include "call_launch.h"  // launch_call, batch_frame: trace_direct.hip launches through them too

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

}  // namespace rtmi
