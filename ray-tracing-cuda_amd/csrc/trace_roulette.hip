// rtmi_trace_roulette: rtmi_trace with Russian roulette played in the lane (render_body.h in its ROULETTE mode; the rule is
// rtmi_path_roulette's, include/rtmi.h).  On the query variants.  A translation unit of its own: no kernel of another unit
// is compiled differently for it.  The LDS layout is render.hip's make_cfg (launch_cfg.h), as rtmi_trace's: the mode writes
// no layer, and the id stack's room stays unused.
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
#include "launch_cfg.h"
#include "call_launch.h"

// The trace kernel's block and, behind it, what the ROULETTE mode reads: in the call's d_work like rtmi_trace's.
struct TraceRouletteParams : CallParams {
  RouletteBufs rx;
};

// Waves per SIMD: rtmi_trace's own bound, but for the two variants that would spill vector registers to scratch there where
// their trace_kernel<F> twins spill none -- triangles + spheres + textures at five waves (12 bytes), everything at three
// (16 bytes) -- which are held one wave lower (DESIGN.md 2.22 has the registers and the scratch of the eight beside their twins).
#define RTMI_TRACE_ROULETTE_WAVES(F)                                                                                      \
  ((F) == (F_TRIS | F_SPHERE | F_TEX) ? 4 : (F) == (F_TEX | F_BVH | F_SGROUP | F_TRIS | F_SPHERE) ? 2 : RTMI_MIN_WAVES(F))
template <uint32_t F>
__global__ __launch_bounds__(RTMI_MAX_THREADS(F), RTMI_TRACE_ROULETTE_WAVES(F)) void trace_roulette_kernel(const TraceRouletteParams *p) {
  const RenderParams &rp = in_constant(p).rp;
  const CallExtras &ex = in_constant(p).ex;
  const RouletteBufs &rx = in_constant(p).rx;
  render_body<F, true, false, false, 0, false, false, false, false, RouletteBufs, true>(
      rp.sc, rp.fr, rp.lc, rp.states, rp.out, rp.ray_counts, rp.counters, ex.rays.origins, ex.rays.dirs, ex.tex_layers != 0, nullptr,
      nullptr, nullptr, nullptr, nullptr, nullptr, &rx);
}

hipError_t launch_trace_roulette(uint32_t variant, const SceneDev &sc, bool tex_layers, int n_cu, int64_t n, int max_depth,
                                 uint32_t first_step, float p_min, const float *d_o, const float *d_d, uint32_t *d_states,
                                 float *d_radiance, uint32_t *d_ray_counts, unsigned long long *d_counts,
                                 unsigned long long *d_work, hipStream_t stream) {
  return with_listed<kQueryVariants>(variant, hipErrorInvalidValue, [&](auto v) {
    constexpr uint32_t F = decltype(v)::value;
    CallExtras ex{};
    ex.rays = {d_o, d_d};
    const auto tail = [&](TraceRouletteParams &cp) { cp.rx = RouletteBufs{first_step, p_min, d_counts}; };
    return launch_call<F, trace_roulette_kernel<F>, TraceRouletteParams>(sc, batch_frame(n, max_depth), tex_layers, 64, n_cu, ex,
                                                                         d_states, d_radiance, d_ray_counts, d_work, stream, true,
                                                                         -1, tail);
  });
}

}  // namespace rtmi
