// rtmi_trace_direct: rtmi_trace with next-event estimation inside the kernel (render_body.h in its DIRECT mode; the vertex
// rule is rtmi_direct_sample_mis's own text, direct_weigh.inc and direct_sample.inc).  On the query variants, each with a
// twin for a table that holds sphere lights.  A translation unit of its own: no kernel of another unit is compiled
// differently for it.  The LDS layout is render.hip's make_cfg (launch_cfg.h), as rtmi_trace's.
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

// The trace kernel's block and, behind it, what the DIRECT mode reads: in the call's d_work like rtmi_trace's.
struct TraceDirectParams : CallParams {
  TraceDirectBufs dx;
};

// The mode carries some twenty registers more than rtmi_trace across the query: the variants that rtmi_trace holds at five
// waves (96 VGPRs) would spill 38-52 dwords there, so none is held above four (DESIGN.md 2.5 has the table).
#define RTMI_DIRECT_WAVES(F) (RTMI_MIN_WAVES(F) > 4 ? 4 : RTMI_MIN_WAVES(F))
template <uint32_t F, bool SPH>
__global__ __launch_bounds__(RTMI_MAX_THREADS(F), RTMI_DIRECT_WAVES(F)) void trace_direct_kernel(const TraceDirectParams *p) {
  const RenderParams &rp = in_constant(p).rp;
  const CallExtras &ex = in_constant(p).ex;
  const TraceDirectBufs &dx = in_constant(p).dx;
  render_body<F, true, false, false, 0, false, false, true, SPH>(rp.sc, rp.fr, rp.lc, rp.states, rp.out, rp.ray_counts, rp.counters,
                                                                 ex.rays.origins, ex.rays.dirs, ex.tex_layers != 0, nullptr, nullptr,
                                                                 nullptr, nullptr, nullptr, nullptr, &dx);
}

hipError_t launch_trace_direct(uint32_t variant, const SceneDev &sc, bool tex_layers, bool sphere_lights, int n_cu, int64_t n,
                               int max_depth, const float *d_o, const float *d_d, uint32_t *d_states, const TraceDirectBufs &dx,
                               float *d_radiance, uint32_t *d_ray_counts, unsigned long long *d_work, hipStream_t stream) {
  return with_listed<kQueryVariants>(variant, hipErrorInvalidValue, [&](auto v) {
    constexpr uint32_t F = decltype(v)::value;
    CallExtras ex{};
    ex.rays = {d_o, d_d};
    const auto tail = [&](TraceDirectParams &cp) { cp.dx = dx; };
    const FrameDev fr = batch_frame(n, max_depth);
    if (sphere_lights)
      return launch_call<F, trace_direct_kernel<F, true>, TraceDirectParams>(sc, fr, tex_layers, 64, n_cu, ex, d_states, d_radiance,
                                                                             d_ray_counts, d_work, stream, true, -1, tail);
    return launch_call<F, trace_direct_kernel<F, false>, TraceDirectParams>(sc, fr, tex_layers, 64, n_cu, ex, d_states, d_radiance,
                                                                            d_ray_counts, d_work, stream, true, -1, tail);
  });
}

}  // namespace rtmi
