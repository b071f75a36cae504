// rtmi_path_advance: ended paths finished and refilled in place (advance_body.h).  A translation unit of its own: no
// kernel of another unit is compiled differently for it.  It shares its three rules with paths.hip and frame.hip through path_shared.h --
// "live" with rtmi_path_compact, the fold with rtmi_path_fold, the camera ray with rtmi_camera_rays -- and takes the
// device helpers those are written in (unit3_rn, rng_01) from trace_helpers.h, none of whose other functions it uses.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "kernels.h"

#include <cfloat>
#include <cmath>
#include "scene_dev.h"
#include "vec.h"
#include "xorwow.h"

namespace rtmi {

#include "frame_math.h"
#include "trace_helpers.h"
#include "path_shared.h"
#include "advance_body.h"

template <bool CURVED>
__global__ __launch_bounds__(kAdvanceThreads) void path_advance_kernel(AdvanceArgs a) {
  advance_body<CURVED>(a);
}

// One lane per candidate: list_grid (kernels.h) over the host's bound n_list.
hipError_t launch_path_advance(const FrameDev &fr, const CameraDev &cam, const float w[3], int kind, float fov,
                               const AdvanceCall &c, int n_cu, hipStream_t stream) {
  AdvanceArgs a{};
  a.fr = fr, a.proj.cam = cam, a.proj.w = mk(w[0], w[1], w[2]), a.proj.kind = kind, a.proj.fov = fov;
  a.budget = c.budget, a.list = c.list.list, a.count = c.list.count, a.n_list = c.list.n_list;
  a.origins = c.origins, a.dirs = c.dirs, a.states = c.states, a.steps = c.steps;
  a.emitted = c.emitted, a.attenuation = c.attenuation;
  a.emitted_stack = c.emitted_stack, a.attenuation_stack = c.attenuation_stack, a.cursor = c.cursor;
  a.sum = c.sum, a.sq = c.sq, a.samples = c.samples, a.ray_counts = c.ray_counts, a.counts = c.counts;
  const dim3 grid(list_grid(a.n_list, kAdvanceThreads, n_cu, kAdvanceBlocksPerCu));
  if (kind == PROJ_EQUIRECT || kind == PROJ_FISHEYE) {
    hipLaunchKernelGGL(path_advance_kernel<true>, grid, dim3(kAdvanceThreads), 0, stream, a);
  } else {
    hipLaunchKernelGGL(path_advance_kernel<false>, grid, dim3(kAdvanceThreads), 0, stream, a);
  }
  return hipGetLastError();
}

}  // namespace rtmi
