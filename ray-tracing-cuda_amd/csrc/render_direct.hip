// rtmi_render_direct: rtmi_render_budget / rtmi_render_features with next-event estimation inside the kernel
// (render_body.h in its DIRECT mode with BUDGET; the vertex rule is rtmi_direct_sample_mis's own text, direct_weigh.inc and
// direct_sample.inc, as in trace_direct.hip).  On the budget mode's variants -- the query variants with F_DEFOCUS -- each with
// a twin for a table that holds sphere lights.  A translation unit of its own: no kernel of another unit is compiled
// differently for it.  The LDS layout is render.hip's make_cfg (launch_cfg.h), as rtmi_render_budget's.
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
#include "direct_body.h"  // the light table, sphere_cone, light_pick, TraceDirectBufs

#define RTMI_TRACE_DIRECT 1  // render_body.h: this unit knows the light table's types

namespace rtmi {

#include "frame_math.h"
#include "trace_helpers.h"
#include "path_shared.h"
#include "mesh_search.h"
#include "closest_hit.h"
#include "render_body.h"
#include "query_body.h"  // (resolve_hit: the hit as rtmi_hit names it)
#include "launch_cfg.h"
#include "call_launch.h"

// The budget kernel's block and, behind it, what the DIRECT mode reads: in the call's d_work like rtmi_render_budget's.  A
// type of its own (not trace_direct.hip's), so that the block is written by this unit's own params_write_kernel.
struct RenderDirectParams : CallParams {
  TraceDirectBufs dx;
};

// Waves per SIMD the register allocation must allow, per variant, from the compiler's register report (DESIGN.md 2.5 has
// the table): the mode carries what rtmi_trace_direct carries and the budget mode's pixel state on top of it.
#define RTMI_RENDER_DIRECT_WAVES(F) (RTMI_MIN_WAVES((F) & ~(uint32_t)F_DEFOCUS) > 4 ? 4 : RTMI_MIN_WAVES((F) & ~(uint32_t)F_DEFOCUS))
template <uint32_t F, bool SPH>
__global__ __launch_bounds__(RTMI_MAX_THREADS(F), RTMI_RENDER_DIRECT_WAVES(F)) void budget_direct_kernel(const RenderDirectParams *p) {
  const RenderParams &rp = in_constant(p).rp;
  const CallExtras &ex = in_constant(p).ex;
  const TraceDirectBufs &dx = in_constant(p).dx;
  render_body<F, false, true, false, 0, false, false, true, SPH>(rp.sc, rp.fr, rp.lc, rp.states, rp.out, rp.ray_counts, rp.counters,
                                                                 nullptr, nullptr, ex.tex_layers != 0, ex.px.budget, ex.px.sq,
                                                                 ex.px.samples, nullptr, nullptr, nullptr, &dx);
}
// budget_direct_kernel's twin with the FEATURES flag of the body set, as feature_kernel is budget_kernel's.
template <uint32_t F, bool SPH>
__global__ __launch_bounds__(RTMI_MAX_THREADS(F), RTMI_RENDER_DIRECT_WAVES(F)) void feature_direct_kernel(const RenderDirectParams *p) {
  const RenderParams &rp = in_constant(p).rp;
  const CallExtras &ex = in_constant(p).ex;
  const TraceDirectBufs &dx = in_constant(p).dx;
  render_body<F, false, true, true, 0, false, false, true, SPH>(rp.sc, rp.fr, rp.lc, rp.states, rp.out, rp.ray_counts, rp.counters,
                                                                nullptr, nullptr, ex.tex_layers != 0, ex.px.budget, ex.px.sq,
                                                                ex.px.samples, &ex.feat, nullptr, nullptr, &dx);
}

// launch_budget's launch (calls.hip) with the DIRECT kernels: the same frame, queue batch and grid.
hipError_t launch_budget_direct(uint32_t variant, const SceneDev &sc, bool tex_layers, bool sphere_lights, int n_cu,
                                const FrameDev &frame, const uint32_t *d_budget, uint32_t *d_states, const TraceDirectBufs &dx,
                                float *d_sum, float *d_sq, uint32_t *d_samples, uint32_t *d_ray_counts, const FeatureBufs *feat,
                                unsigned long long *d_work, hipStream_t stream) {
  const bool features = feat && (feat->albedo || feat->normal || feat->depth || feat->coverage);
  return with_listed<kQueryVariants>(variant, hipErrorInvalidValue, [&](auto v) {
    constexpr uint32_t F = decltype(v)::value | F_DEFOCUS;
    FrameDev fr = frame;
    fr.post = 0, fr.k_begin = 0, fr.k_end = fr.spp;
    const int batch = image_order_batch(fr.spp, 64);
    CallExtras ex{};
    ex.px = {d_budget, d_sq, d_samples};
    if (features) ex.feat = *feat;
    const auto tail = [&](RenderDirectParams &cp) { cp.dx = dx; };
    if (features && sphere_lights)
      return launch_call<F, feature_direct_kernel<F, true>, RenderDirectParams>(sc, fr, tex_layers, batch, n_cu, ex, d_states, d_sum,
                                                                                d_ray_counts, d_work, stream, true, -1, tail);
    if (features)
      return launch_call<F, feature_direct_kernel<F, false>, RenderDirectParams>(sc, fr, tex_layers, batch, n_cu, ex, d_states, d_sum,
                                                                                 d_ray_counts, d_work, stream, true, -1, tail);
    if (sphere_lights)
      return launch_call<F, budget_direct_kernel<F, true>, RenderDirectParams>(sc, fr, tex_layers, batch, n_cu, ex, d_states, d_sum,
                                                                               d_ray_counts, d_work, stream, true, -1, tail);
    return launch_call<F, budget_direct_kernel<F, false>, RenderDirectParams>(sc, fr, tex_layers, batch, n_cu, ex, d_states, d_sum,
                                                                              d_ray_counts, d_work, stream, true, -1, tail);
  });
}

}  // namespace rtmi
