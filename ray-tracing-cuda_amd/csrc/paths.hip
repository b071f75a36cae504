// The live paths as a list (rtmi_path_compact) and the fold of a path's layers (rtmi_path_fold).  A translation unit of its
// own: it shares "live" and the fold with advance.hip through path_shared.h, takes the device helpers those are written in
// from trace_helpers.h, and no kernel of another unit is compiled differently for it.
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
#include "mesh_search.h"  // (lane_rank alone)

// ------------------------------------------------------------------ the live paths as a list (rtmi_path_compact)
// Three launches, none of whose workgroups waits for another: each workgroup counts the live candidates among its
// kCompactItems entries; one workgroup turns the counts into offsets (and the total into *d_count_out); each workgroup
// finds its live candidates again and writes them from its offset on, in the candidates' order.  A wave owns
// kCompactChunks consecutive chunks of 64 entries, lane l entry l of each, so a live candidate's place is its
// workgroup's offset + the live ones of the waves and chunks before its own + those of the lower lanes (mbcnt).
// The rays are read twice (24 B a path); the list's length, where it is on the device, is read by every workgroup and
// the grids are sized by the host's bound.
constexpr int kCompactThreads = 256, kCompactChunks = 4;
constexpr int kCompactItems = kCompactThreads * kCompactChunks;  // entries per workgroup: a scratch word each
constexpr int kCompactScanThreads = 256;  // the scan's one workgroup; each lane sums ceil(workgroups / 256) counts in a row
static_assert(kCompactItems == RTMI_PATH_COMPACT_ITEMS, "rtmi.h states the entries per scratch word");

struct CompactArgs {
  const float *origins, *dirs;  // float[n][3]
  const uint32_t *list_in;      // nullable: the candidates (null: 0, 1, 2, ...)
  const uint32_t *count_in;     // nullable: a device word that cuts the candidates short
  uint32_t n, n_list;
};
// (live_ray, whether a step would step a ray: path_shared.h, which rtmi_path_advance's unit includes too)
// Entry e of the candidates: its path, and whether the next step would step it.
__device__ __forceinline__ bool compact_live(const CompactArgs &a, const PathList &pl, uint32_t e, uint32_t end, uint32_t &path) {
  path = 0u;
  if (e >= end) return false;
  path = list_entry(pl, e);
  if (path >= a.n) return false;  // (not a path: dropped)
  const float *o = a.origins + (int64_t)path * 3, *d = a.dirs + (int64_t)path * 3;
  return live_ray(mk(o[0], o[1], o[2]), mk(d[0], d[1], d[2]));
}
// The live candidates of this lane's kCompactChunks entries: their paths, the chunks' wave masks, and the wave's total.
__device__ __forceinline__ uint32_t compact_wave(const CompactArgs &a, uint32_t (&path)[kCompactChunks],
                                                 unsigned long long (&mask)[kCompactChunks]) {
  const PathList pl{a.list_in, a.count_in, a.n_list};  // (the block keeps its layout; the rule is path_list.h's)
  const uint32_t end = list_end(pl);
  // (entries below 2^31 + kCompactItems: the grid covers n_list <= 2^31 - 1)
  const uint32_t first = blockIdx.x * (uint32_t)kCompactItems + (threadIdx.x >> 6) * (uint32_t)(64 * kCompactChunks) + (threadIdx.x & 63u);
  uint32_t total = 0u;
#pragma unroll
  for (int c = 0; c < kCompactChunks; c++) {
    mask[c] = __builtin_amdgcn_ballot_w64(compact_live(a, pl, first + (uint32_t)c * 64u, end, path[c]));
    total += (uint32_t)__popcll(mask[c]);
  }
  return total;
}

__global__ __launch_bounds__(kCompactThreads) void compact_count_kernel(CompactArgs a, uint32_t *__restrict__ counts) {
  __shared__ uint32_t s_wave[kCompactThreads / 64];
  uint32_t path[kCompactChunks];
  unsigned long long mask[kCompactChunks];
  const uint32_t total = compact_wave(a, path, mask);
  if ((threadIdx.x & 63u) == 0u) s_wave[threadIdx.x >> 6] = total;
  __syncthreads();
  if (threadIdx.x == 0u) {
    uint32_t sum = 0u;
    for (int w = 0; w < kCompactThreads / 64; w++) sum += s_wave[w];
    counts[blockIdx.x] = sum;
  }
}

// counts[0 .. n_blocks) -> their exclusive prefix sums, in place; *count_out = their total.  One workgroup.
__global__ __launch_bounds__(kCompactScanThreads) void compact_scan_kernel(uint32_t n_blocks, uint32_t *__restrict__ counts,
                                                                            uint32_t *__restrict__ count_out) {
  __shared__ uint32_t s_wave[kCompactScanThreads / 64];
  const uint32_t per = (n_blocks + (uint32_t)kCompactScanThreads - 1u) / (uint32_t)kCompactScanThreads;
  const uint32_t lo = threadIdx.x * per < n_blocks ? threadIdx.x * per : n_blocks;  // (per <= 2^13: no wrap)
  const uint32_t hi = lo + per < n_blocks ? lo + per : n_blocks;
  uint32_t sum = 0u;
  for (uint32_t i = lo; i < hi; i++) sum += counts[i];
  uint32_t incl = sum;  // inclusive scan over the wave's lanes
  for (int off = 1; off < 64; off <<= 1) {
    const uint32_t below = (uint32_t)__shfl_up((int)incl, off);
    if ((threadIdx.x & 63u) >= (uint32_t)off) incl += below;
  }
  if ((threadIdx.x & 63u) == 63u) s_wave[threadIdx.x >> 6] = incl;
  __syncthreads();
  uint32_t run = incl - sum;
  for (uint32_t w = 0; w < (threadIdx.x >> 6); w++) run += s_wave[w];
  for (uint32_t i = lo; i < hi; i++) {
    const uint32_t c = counts[i];
    counts[i] = run;
    run += c;
  }
  if (threadIdx.x == (uint32_t)kCompactScanThreads - 1u) *count_out = run;  // (the last lane's end is the total)
}

__global__ __launch_bounds__(kCompactThreads) void compact_scatter_kernel(CompactArgs a, const uint32_t *__restrict__ offsets,
                                                                           uint32_t *__restrict__ list_out) {
  __shared__ uint32_t s_wave[kCompactThreads / 64];
  uint32_t path[kCompactChunks];
  unsigned long long mask[kCompactChunks];
  const uint32_t total = compact_wave(a, path, mask);
  if ((threadIdx.x & 63u) == 0u) s_wave[threadIdx.x >> 6] = total;
  __syncthreads();
  uint32_t at = offsets[blockIdx.x];
  for (uint32_t w = 0; w < (threadIdx.x >> 6); w++) at += s_wave[w];
  const unsigned long long me = 1ull << (threadIdx.x & 63u);
#pragma unroll
  for (int c = 0; c < kCompactChunks; c++) {
    // (at + rank < the total of all workgroups <= the candidates <= n_list: inside list_out)
    if (mask[c] & me) list_out[at + (uint32_t)lane_rank(mask[c])] = path[c];
    at += (uint32_t)__popcll(mask[c]);
  }
}

size_t path_compact_scratch_bytes(int64_t n_list) {
  if (n_list < 0) n_list = 0;
  const int64_t blocks = cdiv(n_list, (int64_t)kCompactItems);
  return (size_t)(blocks > 0 ? blocks : 1) * sizeof(uint32_t);
}

hipError_t launch_path_compact(int64_t n, const float *d_origins, const float *d_dirs, const PathList &in, uint32_t *d_list_out,
                               uint32_t *d_count_out, uint32_t *d_scratch, hipStream_t stream) {
  if (in.n_list == 0) return hipMemsetAsync(d_count_out, 0, sizeof(uint32_t), stream);
  const CompactArgs a = {d_origins, d_dirs, in.list, in.count, (uint32_t)n, in.n_list};
  const unsigned blocks = (unsigned)cdiv((int64_t)in.n_list, (int64_t)kCompactItems);
  hipLaunchKernelGGL(compact_count_kernel, dim3(blocks), dim3(kCompactThreads), 0, stream, a, d_scratch);
  hipLaunchKernelGGL(compact_scan_kernel, dim3(1), dim3(kCompactScanThreads), 0, stream, (uint32_t)blocks, d_scratch, d_count_out);
  hipLaunchKernelGGL(compact_scatter_kernel, dim3(blocks), dim3(kCompactThreads), 0, stream, a, (const uint32_t *)d_scratch, d_list_out);
  return hipGetLastError();
}

// Trace's return expression over the layers the steps wrote (rtmi_path_fold; include/rtmi.h states the rule): one lane
// per path, so a layer's reads are coalesced over n; product and sum each rounded on their own.
__global__ __launch_bounds__(256) void path_fold_kernel(int64_t n, uint32_t layers, const float *__restrict__ dirs,
                                                         const uint32_t *__restrict__ steps, const float *__restrict__ emitted,
                                                         const float *__restrict__ attenuation, float *__restrict__ radiance) {
  const int64_t q = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (q >= n) return;
  const uint32_t s = steps[q];
  const bool ended = dirs[q * 3 + 0] == 0.f && dirs[q * 3 + 1] == 0.f && dirs[q * 3 + 2] == 0.f;
  const V3 r = fold_layers(emitted, attenuation, n, q, (int)(s < layers ? s : layers), ended);  // (path_shared.h)
  radiance[q * 3 + 0] = r.x, radiance[q * 3 + 1] = r.y, radiance[q * 3 + 2] = r.z;
}
hipError_t launch_path_fold(int64_t n, int layers, const float *d_dirs, const uint32_t *d_steps, const float *d_emitted,
                            const float *d_attenuation, float *d_radiance, hipStream_t stream) {
  if (n == 0) return hipSuccess;
  hipLaunchKernelGGL(path_fold_kernel, dim3((unsigned)cdiv(n, 256)), dim3(256), 0, stream, n, (uint32_t)layers, d_dirs, d_steps,
                     d_emitted, d_attenuation, d_radiance);
  return hipGetLastError();
}

// ------------------------------------------------------------------ Russian roulette as a step (rtmi_path_roulette)
// include/rtmi.h states the rule; tests/roulettelib.py restates it.  One lane per candidate: wave w of the grid takes
// entries 64w .. 64w + 63 of the list (path_list.h), so the grid is sized by the host's bound and a wave past the device's
// count leaves at once -- no cursor, no atomic in the distribution.  The lanes that play and those that kill are counted by
// a ballot each and one atomic per wave.  Every binary32 * and / below is one operation (no contraction in this unit).
constexpr int kRouletteThreads = 256;
__global__ __launch_bounds__(kRouletteThreads) void path_roulette_kernel(RouletteArgs a) {
  const PathList pl{a.list, a.count, a.n_list};
  const uint32_t end = list_end(pl);
  const uint32_t e = blockIdx.x * (uint32_t)kRouletteThreads + threadIdx.x;  // (below 2^31 + 256: n_list <= 2^31 - 1)
  bool played = false, killed = false;
  if (e < end) {
    const uint32_t i = list_entry(pl, e);
    // (not a path: dropped before anything is addressed with it; not stepped, or ended: every word is kept)
    if (i < a.n && a.steps[i] == a.step + 1u) {
      float *d = a.dirs + (int64_t)i * 3, *at = a.attenuation + (int64_t)i * 3, *th = a.throughput + (int64_t)i * 3;
      if (!(d[0] == 0.f && d[1] == 0.f && d[2] == 0.f)) {
        const V3 att = mk(at[0], at[1], at[2]), P = mk(th[0], th[1], th[2]);
        const V3 t = mk(__fmul_rn(P.x, att.x), __fmul_rn(P.y, att.y), __fmul_rn(P.z, att.z));
        float q = t.x;
        if (t.y > q) q = t.y;
        if (t.z > q) q = t.z;
        played = a.step >= a.first_step && q < 1.f;
        if (!played) {
          th[0] = t.x, th[1] = t.y, th[2] = t.z;
        } else {
          const float p = q > a.p_min ? q : a.p_min;
          Rng rng;
          rng.d = a.states[0 * (int64_t)a.n + i], rng.v0 = a.states[1 * (int64_t)a.n + i], rng.v1 = a.states[2 * (int64_t)a.n + i];
          rng.v2 = a.states[3 * (int64_t)a.n + i], rng.v3 = a.states[4 * (int64_t)a.n + i], rng.v4 = a.states[5 * (int64_t)a.n + i];
          const float u = rng_01(rng);
          a.states[0 * (int64_t)a.n + i] = rng.d, a.states[1 * (int64_t)a.n + i] = rng.v0, a.states[2 * (int64_t)a.n + i] = rng.v1;
          a.states[3 * (int64_t)a.n + i] = rng.v2, a.states[4 * (int64_t)a.n + i] = rng.v3, a.states[5 * (int64_t)a.n + i] = rng.v4;
          if (u <= p) {
            const float inv = 1.0f / p;
            const V3 s = mk(__fmul_rn(att.x, inv), __fmul_rn(att.y, inv), __fmul_rn(att.z, inv));
            at[0] = s.x, at[1] = s.y, at[2] = s.z;
            th[0] = __fmul_rn(P.x, s.x), th[1] = __fmul_rn(P.y, s.y), th[2] = __fmul_rn(P.z, s.z);
          } else {
            killed = true;
            at[0] = 0.f, at[1] = 0.f, at[2] = 0.f;
            d[0] = 0.f, d[1] = 0.f, d[2] = 0.f;
            th[0] = 0.f, th[1] = 0.f, th[2] = 0.f;
          }
        }
      }
    }
  }
  const unsigned long long np = __builtin_amdgcn_ballot_w64(played), nk = __builtin_amdgcn_ballot_w64(killed);
  if ((threadIdx.x & 63u) == 0u && a.counts) {
    if (np) atomicAdd(&a.counts[0], (unsigned long long)__popcll(np));
    if (nk) atomicAdd(&a.counts[1], (unsigned long long)__popcll(nk));
  }
}
hipError_t launch_path_roulette(const RouletteArgs &a, hipStream_t stream) {
  if (a.n == 0 || a.n_list == 0) return hipSuccess;
  hipLaunchKernelGGL(path_roulette_kernel, dim3((unsigned)cdiv((int64_t)a.n_list, (int64_t)kRouletteThreads)),
                     dim3(kRouletteThreads), 0, stream, a);
  return hipGetLastError();
}

}  // namespace rtmi
