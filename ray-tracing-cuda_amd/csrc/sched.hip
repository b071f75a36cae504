// The kernels that plan a scheduled render from a probe pass's ray counts: tile costs and their longest-first order, the
// head of the queue, the per-quarter-tile order, the planned chains -- and their launchers.  A translation unit of its own:
// they read and write words only, and use none of the trace path's device code.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "kernels.h"

namespace rtmi {

// ------------------------------------------------------------------ longest-first tile order
// A pixel is an indivisible serial chain (its samples share one RNG stream), so the end of a
// frame is a tail of lanes finishing their last pixel.  Handing out the expensive tiles first
// shortens that tail (longest-processing-time-first).  Cost estimate: rays per tile measured by
// a 2-spp probe pass on a scratch copy of the RNG states.  The order only changes which lane
// renders which pixel when; every pixel's arithmetic is unchanged.
__global__ __launch_bounds__(256) void tile_cost_kernel(const uint32_t *__restrict__ ray_counts, int n_tiles,
                                                         uint32_t *__restrict__ cost, uint32_t *__restrict__ max_cost) {
  int t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= n_tiles) return;
  const uint4 *p = reinterpret_cast<const uint4 *>(ray_counts + (size_t)t * 64);
  uint32_t s = 0;
#pragma unroll
  for (int i = 0; i < 16; i++) {
    uint4 v = p[i];
    s += v.x + v.y + v.z + v.w;
  }
  cost[t] = s;
  atomicMax(max_cost, s);
}

// One workgroup: counting sort of the tiles into 256 cost buckets, most expensive bucket first.
// Also sizes the "sparse" head of the queue (sparse_items, in work items; render_body, mesh
// variants): the outlier tiles -- at least twice the mean cost, in a frame whose most expensive
// tile costs at least three times the mean -- up to `sparse_cap` items, what the grid can hold at
// one pixel per kSparseStride lanes.
__global__ __launch_bounds__(1024) void tile_order_kernel(const uint32_t *__restrict__ cost,
                                                          const uint32_t *__restrict__ max_cost, int n_tiles,
                                                          uint32_t *__restrict__ order,
                                                          uint32_t *__restrict__ sparse_items, uint32_t sparse_cap,
                                                          uint32_t outlier_x10) {
  __shared__ uint32_t bins[256];
  __shared__ uint32_t base[256];
  __shared__ unsigned long long total;
  __shared__ uint32_t outliers;
  for (int i = threadIdx.x; i < 256; i += blockDim.x) bins[i] = 0;
  if (threadIdx.x == 0) total = 0ull, outliers = 0u;
  __syncthreads();
  const uint32_t mx = *max_cost > 0 ? *max_cost : 1;
  unsigned long long part = 0ull;
  for (int t = threadIdx.x; t < n_tiles; t += blockDim.x) {
    uint32_t b = 255u - (uint32_t)(((unsigned long long)cost[t] * 255ull) / mx);  // bucket 0 = most expensive
    atomicAdd(&bins[b], 1u);
    part += cost[t];
  }
  atomicAdd(&total, part);
  __syncthreads();
  {
    const unsigned long long sum = total;  // mean = sum / n_tiles; compare cost * n_tiles with k * sum
    uint32_t mine = 0;
    for (int t = threadIdx.x; t < n_tiles; t += blockDim.x)
      if ((unsigned long long)cost[t] * (unsigned long long)n_tiles * 10ull >= (unsigned long long)outlier_x10 * sum) mine++;
    if (mine) atomicAdd(&outliers, mine);
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    uint32_t run = 0;
    for (int i = 0; i < 256; i++) {
      base[i] = run;
      run += bins[i];
    }
    const bool skewed = (unsigned long long)mx * (unsigned long long)n_tiles >= 3ull * total;
    const uint32_t items = outliers * 64u;
    *sparse_items = skewed ? (items < sparse_cap ? items : sparse_cap) : 0u;
  }
  __syncthreads();
  for (int t = threadIdx.x; t < n_tiles; t += blockDim.x) {
    uint32_t b = 255u - (uint32_t)(((unsigned long long)cost[t] * 255ull) / mx);
    order[atomicAdd(&base[b], 1u)] = (uint32_t)t;
  }
}

// One workgroup: the head of the queue, pixel by pixel.  A pixel's chain is as long as its ray count, and a
// wave's query costs about as much per outlier ray it carries (measured: tools/mesh_stats.sh marks); outlier
// pixels also sit in tiles that are not outliers as tiles, where they would run their first thousand queries in a
// full wave.  So the head is made of PIXELS, from the whole frame: those whose probe count is >= pct64 % of the
// frame's largest get a wave each, >= pct32 % two per wave, >= pct16 % one per 16 lanes -- in a frame whose
// largest count is at least three times the mean, and as long as that takes no more than a quarter of the grid's
// waves and kHeadCap entries; else first the lightest class goes, then the heaviest pixels share waves two by two,
// then there is no head.  Listed pixels get bit 31 of their ray_counts word set: the ordinary queue passes them
// over.  meta[0] = head entries, meta[1], meta[2] = ends of the first two classes.
// (four small launches over the whole frame instead of one workgroup walking it three times: 0.6 ms -> tens of us)
// ws[0] largest count, ws[2..3] sum (64 bit), ws[4..6] class counts, ws[8..10] thresholds, ws[12..14] scatter cursors
__global__ __launch_bounds__(256) void head_scan_kernel(const uint32_t *__restrict__ ray_counts, int n_items,
                                                        uint32_t *__restrict__ ws) {
  uint32_t m = 0u;
  unsigned long long part = 0ull;
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n_items; i += gridDim.x * blockDim.x)
    m = max(m, ray_counts[i]), part += ray_counts[i];
  for (int off = 32; off > 0; off >>= 1) m = max(m, (uint32_t)__shfl_down((int)m, off)), part += __shfl_down(part, off);
  if ((threadIdx.x & 63) == 0) {
    atomicMax(&ws[0], m);
    atomicAdd(reinterpret_cast<unsigned long long *>(ws + 2), part);  // (d_meta is 8-byte aligned: capi.hip)
  }
}
__global__ __launch_bounds__(256) void head_count_kernel(const uint32_t *__restrict__ ray_counts, int n_items,
                                                         uint32_t *__restrict__ ws, uint32_t pct64, uint32_t pct32,
                                                         uint32_t pct16) {
  const uint32_t cmax = ws[0];
  const unsigned long long total = *reinterpret_cast<const unsigned long long *>(ws + 2);
  const bool skewed = (unsigned long long)cmax * (unsigned long long)n_items >= 3ull * total && cmax >= 4u;
  if (!skewed) return;
  const uint32_t t64 = (cmax * pct64 + 99u) / 100u, t32 = (cmax * pct32 + 99u) / 100u, t16 = (cmax * pct16 + 99u) / 100u;
  uint32_t c0 = 0u, c1 = 0u, c2 = 0u;
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n_items; i += gridDim.x * blockDim.x) {
    const uint32_t c = ray_counts[i];
    if (c >= t16) (c >= t64 ? c0 : c >= t32 ? c1 : c2)++;
  }
  for (int off = 32; off > 0; off >>= 1) c0 += __shfl_down(c0, off), c1 += __shfl_down(c1, off), c2 += __shfl_down(c2, off);
  if ((threadIdx.x & 63) == 0) {
    if (c0) atomicAdd(&ws[4], c0);
    if (c1) atomicAdd(&ws[5], c1);
    if (c2) atomicAdd(&ws[6], c2);
  }
}
__global__ void head_plan_kernel(int n_items, uint32_t *__restrict__ meta, uint32_t *__restrict__ ws, uint32_t grid_waves,
                                 uint32_t pct64, uint32_t pct32, uint32_t pct16) {
  const uint32_t cmax = ws[0], none = 0xffffffffu;
  const unsigned long long total = *reinterpret_cast<const unsigned long long *>(ws + 2);
  const bool skewed = (unsigned long long)cmax * (unsigned long long)n_items >= 3ull * total && cmax >= 4u;
  uint32_t t64 = skewed ? (cmax * pct64 + 99u) / 100u : none, t32 = skewed ? (cmax * pct32 + 99u) / 100u : none,
           t16 = skewed ? (cmax * pct16 + 99u) / 100u : none;
  uint32_t a = ws[4], b = ws[5], c3 = ws[6];
  auto over = [&]() { return a + (b + 1u) / 2u + (c3 + 3u) / 4u > grid_waves / 4u || a + b + c3 > (uint32_t)kHeadCap; };
  if (over()) c3 = 0u, t16 = t32;
  if (over()) b += a, a = 0u, t64 = none;
  if (over()) b = 0u, t32 = none, t16 = none;
  meta[0] = a + b + c3, meta[1] = a, meta[2] = a + b;
  ws[8] = t64, ws[9] = t32, ws[10] = t16;
  ws[12] = 0u, ws[13] = a, ws[14] = a + b;  // scatter cursors
}
__global__ __launch_bounds__(256) void head_scatter_kernel(uint32_t *__restrict__ ray_counts, int n_items,
                                                           uint32_t *__restrict__ head, uint32_t *__restrict__ ws) {
  const uint32_t t64 = ws[8], t32 = ws[9], t16 = ws[10];
  if (t16 == 0xffffffffu) return;
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n_items; i += gridDim.x * blockDim.x) {
    const uint32_t c = ray_counts[i];
    if (c >= t16) {
      head[atomicAdd(&ws[12 + (c >= t64 ? 0 : c >= t32 ? 1 : 2)], 1u)] = (uint32_t)i;
      ray_counts[i] = c | 0x80000000u;
    }
  }
}

// The queue's order is kept per QUARTER tile (16 work items = two rows of a tile).  List scenes: the tiles in
// longest-first order, each tile's quarters one after the other.
__global__ __launch_bounds__(256) void expand_order_kernel(const uint32_t *__restrict__ order, int n_tiles,
                                                            uint32_t *__restrict__ qmap) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n_tiles * 4) qmap[i] = order[i >> 2] * 4u + (uint32_t)(i & 3);
}
// Mesh scenes with a cost probe: a quarter's cost = the lane-steps the probe's mesh searches spent on its 16 pixels
// (+ their ray counts, so that it is never zero) ...
__global__ __launch_bounds__(256) void quarter_cost_kernel(const uint32_t *__restrict__ work, const uint32_t *__restrict__ rays,
                                                            int n_quarters, uint32_t *__restrict__ cost,
                                                            uint32_t *__restrict__ max_cost) {
  const int qd = blockIdx.x * blockDim.x + threadIdx.x;
  if (qd >= n_quarters) return;
  uint32_t s = 0;
  for (int i = 0; i < 16; i++) s += work[(size_t)qd * 16 + i] + (rays[(size_t)qd * 16 + i] & 0x7fffffffu);
  cost[qd] = s;
  atomicMax(max_cost, s);
}
// ... one workgroup sorts the quarters by cost (256 buckets, dearest first) ...
__global__ __launch_bounds__(1024) void quarter_sort_kernel(const uint32_t *__restrict__ cost, const uint32_t *__restrict__ max_cost,
                                                             int n_quarters, uint32_t *__restrict__ sorted) {
  __shared__ uint32_t bins[256];
  __shared__ uint32_t base[256];
  for (int i = threadIdx.x; i < 256; i += blockDim.x) bins[i] = 0;
  __syncthreads();
  const uint32_t mx = *max_cost > 0 ? *max_cost : 1;
  for (int t = threadIdx.x; t < n_quarters; t += blockDim.x)
    atomicAdd(&bins[255u - (uint32_t)(((unsigned long long)cost[t] * 255ull) / mx)], 1u);
  __syncthreads();
  if (threadIdx.x == 0) {
    uint32_t run = 0;
    for (int i = 0; i < 256; i++) base[i] = run, run += bins[i];
  }
  __syncthreads();
  for (int t = threadIdx.x; t < n_quarters; t += blockDim.x)
    sorted[atomicAdd(&base[255u - (uint32_t)(((unsigned long long)cost[t] * 255ull) / mx)], 1u)] = (uint32_t)t;
}
// ... and every 64 consecutive work items of the queue -- what the lanes of a wave pick up together -- are dealt one
// quarter from each quartile of that order (a snake: b, 2n - 1 - b, 2n + b, 4n - 1 - b): no wave starts on 64 rays of a
// dense tile (150-260 k cycles per query of a full wave against 40 k for the frame's typical mix; such waves WERE the
// frame's last per cent), every wave's first 64 pixels cost about the same, and the dearest quarters still go first.
__global__ __launch_bounds__(256) void snake_map_kernel(const uint32_t *__restrict__ sorted, int n_tiles,
                                                         uint32_t *__restrict__ qmap) {
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= n_tiles) return;
  const int n = n_tiles;
  qmap[4 * b + 0] = sorted[b];
  qmap[4 * b + 1] = sorted[2 * n - 1 - b];
  qmap[4 * b + 2] = sorted[2 * n + b];
  qmap[4 * b + 3] = sorted[4 * n - 1 - b];
}
hipError_t launch_quarter_order(const uint32_t *d_order, const uint32_t *d_work, const uint32_t *d_rays, int n_tiles,
                                uint32_t *d_qcost, uint32_t *d_qsorted, uint32_t *d_qmax, uint32_t *d_qmap, hipStream_t stream) {
  if (!d_work) {
    hipLaunchKernelGGL(expand_order_kernel, dim3((n_tiles * 4 + 255) / 256), dim3(256), 0, stream, d_order, n_tiles, d_qmap);
    return hipGetLastError();
  }
  hipError_t e = hipMemsetAsync(d_qmax, 0, sizeof(uint32_t), stream);
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(quarter_cost_kernel, dim3((n_tiles * 4 + 255) / 256), dim3(256), 0, stream, d_work, d_rays, n_tiles * 4,
                     d_qcost, d_qmax);
  hipLaunchKernelGGL(quarter_sort_kernel, dim3(1), dim3(1024), 0, stream, d_qcost, d_qmax, n_tiles * 4, d_qsorted);
  hipLaunchKernelGGL(snake_map_kernel, dim3((n_tiles + 255) / 256), dim3(256), 0, stream, d_qsorted, n_tiles, d_qmap);
  return hipGetLastError();
}

// One thread per chain (wave r of SIMD s, c = r S + s), walked backwards so that every tile learns what follows it.
// The SIMD's k-th tile is rank k S + (k odd ? S - 1 - s : s); the wave's j-th tile is the SIMD's k = j R + (j odd ? R - 1 - r : r).
__global__ __launch_bounds__(256) void chain_link_kernel(const uint32_t *__restrict__ order, const uint32_t *__restrict__ cost,
                                                          int n_tiles, int S, int R, float scale, int32_t *__restrict__ first,
                                                          int32_t *__restrict__ next, uint32_t *__restrict__ fut) {
  const int c = blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= S * R) return;
  const int s = c % S, r = c / S;
  auto rank = [&](int j) -> int64_t {
    const int64_t k = (int64_t)j * R + ((j & 1) ? R - 1 - r : r);
    return k * S + ((k & 1) ? S - 1 - s : s);
  };
  int steps = 0;
  while (rank(steps) < n_tiles) steps++;
  float acc = 0.f;
  int32_t after = -1;
  for (int j = steps - 1; j >= 0; j--) {
    const uint32_t t = order[rank(j)];
    next[t] = after;
    fut[t] = (uint32_t)fminf(acc, 4.0e9f);
    acc += (float)cost[t] * scale;
    after = (int32_t)t;
  }
  first[c] = after;
}
hipError_t launch_chain_plan(const uint32_t *d_order, const uint32_t *d_cost, int n_tiles, int simds, int rounds, int spp,
                             int probe_spp, int32_t *d_first, int32_t *d_next, uint32_t *d_fut, hipStream_t stream) {
  const int n = simds * rounds;
  if (n <= 0) return hipSuccess;
  hipLaunchKernelGGL(chain_link_kernel, dim3((n + 255) / 256), dim3(256), 0, stream, d_order, d_cost, n_tiles, simds, rounds,
                     (float)spp / (64.f * (float)probe_spp), d_first, d_next, d_fut);
  return hipGetLastError();
}

hipError_t launch_tile_order(uint32_t *d_ray_counts, int n_tiles, uint32_t *d_cost, uint32_t *d_meta,
                             uint32_t *d_order, uint32_t *d_head, uint32_t sparse_cap, int grid_waves, int outlier_x10,
                             const int head_pct[3], hipStream_t stream) {
  hipError_t e = hipMemsetAsync(d_meta, 0, 32 * sizeof(uint32_t), stream);
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(tile_cost_kernel, dim3((n_tiles + 255) / 256), dim3(256), 0, stream, d_ray_counts, n_tiles, d_cost,
                     d_meta);
  hipLaunchKernelGGL(tile_order_kernel, dim3(1), dim3(1024), 0, stream, d_cost, d_meta, n_tiles, d_order, d_meta + 1,
                     sparse_cap, (uint32_t)outlier_x10);
  if (d_head) {
    const int p64 = head_pct[0], p32 = head_pct[1], p16 = head_pct[2];  // (rtmi_render_opts.head_pct)
    uint32_t *ws = d_meta + 16;  // 16 words of workspace behind the 16 of d_meta (zeroed with them)
    const int n_items = n_tiles * 64, blocks = n_items / 4096 > 0 ? (n_items / 4096 < 1024 ? n_items / 4096 : 1024) : 1;
    hipLaunchKernelGGL(head_scan_kernel, dim3(blocks), dim3(256), 0, stream, d_ray_counts, n_items, ws);
    hipLaunchKernelGGL(head_count_kernel, dim3(blocks), dim3(256), 0, stream, d_ray_counts, n_items, ws, (uint32_t)p64,
                       (uint32_t)p32, (uint32_t)p16);
    hipLaunchKernelGGL(head_plan_kernel, dim3(1), dim3(1), 0, stream, n_items, d_meta + 1, ws, (uint32_t)grid_waves,
                       (uint32_t)p64, (uint32_t)p32, (uint32_t)p16);
    hipLaunchKernelGGL(head_scatter_kernel, dim3(blocks), dim3(256), 0, stream, d_ray_counts, n_items, d_head, ws);
  }
  return hipGetLastError();
}

}  // namespace rtmi
