// What the units whose kernels are built around closest_hit -- render.hip, calls.hip, queries.hip -- share on the host
// side: the launch bounds of a variant, the variant lists, the LDS layout's declaration and the launch templates.
// Templates and constexpr tables are defined here; every non-template function is only declared, and defined once in
// the unit that owns it (named beside the declaration).
#pragma once
// (included inside namespace rtmi, after render_body.h: LaunchCfg)

// Second launch bound = waves per SIMD the register allocation must allow: the list-only variants
// sit at the 80-VGPR / 6-wave step and are issue-bound (one wave less costs 5 %), so the step is
// held explicitly instead of being left to the allocator's luck.
#ifndef RTMI_TRIS_WAVES
#define RTMI_TRIS_WAVES 6
#endif
#ifndef RTMI_BVH_WAVES
#define RTMI_BVH_WAVES 3
#endif
// Sphere and image-texture variants: four waves (at most 128 VGPRs: they sit just below that step, and the allocator's
// count swings by tens of registers with unrelated edits when it is not held) -- except the three that gain from a
// fifth (96 VGPRs, 6-21 spilled dwords) now that their task regions leave room for a fifth workgroup in a CU's LDS
// (scene_dev.h: kListTasks): triangles + spheres + textures (C5 shard 3.16 -> 2.93 s), the grouped sphere scan (spheres
// 1024^2: 22.2 -> 20.9 ms), short sphere runs (+2 %).  Spheres + triangles without textures lose 4-5 % at five (spills
// with no occupancy to show for them) and stay at four.  (tools/gpu_variant_time.py for the variants no workload uses)
#ifndef RTMI_SPH_WAVES
#define RTMI_SPH_WAVES(F) (((F) == (F_TRIS | F_SPHERE | F_TEX) || (F) == (F_SPHERE | F_SGROUP) || (F) == F_SPHERE) ? 5 : 4)
#endif
#define RTMI_MIN_WAVES(F) (((F) & F_BVH) ? RTMI_BVH_WAVES : ((F) & (F_TEX | F_SPHERE | F_SGROUP)) ? RTMI_SPH_WAVES(F) : ((F) & F_TRIS) ? RTMI_TRIS_WAVES : 6)
// Mesh variants share their per-workgroup tables (reference-tree nodes, materials) between more waves:
// workgroups of up to 512 lanes, two of which fill a CU's LDS with 16 waves' search regions.
#define RTMI_MAX_THREADS(F) (((F) & F_BVH) ? 512 : 256)
// One lane copies a kernel's argument block (render_body.h: RenderParams, CallParams) to where the kernel reads it.
template <class P>
__global__ void params_write_kernel(P p, P *dst) {
  if (threadIdx.x == 0 && blockIdx.x == 0) *dst = p;
}

// The LDS layout of a launch (render.hip; one definition: the layout is one decision).
// id_stack = false (query kernels): no stack of material ids, whatever fr.max_depth says.
// tex_layers = false (trace kernels of scenes without image textures): an F_TEX variant with the untextured id stack.
LaunchCfg make_cfg(uint32_t variant, const SceneDev &sc, const FrameDev &fr, int threads, size_t *lds_bytes,
                   bool mats_in_lds = true, bool id_stack = true, bool tex_layers = true);
// Work items per atomic of a queue in image order (render.hip).
int image_order_batch(int samples, int cap);

// Dynamic LDS of a launch of Kernel: above the default limit of 64 KiB it is asked for (160 KiB per CU on gfx950).  The
// bodies address LDS by byte offsets of the dynamic array (render_body.h: lds_byte, the id stack; query_body.h and
// occlusion_body.h: the staged regions): right only while the kernel declares no static LDS, in EVERY build flavour
// (-DRTMI_STATS, -DRTMI_CHECK_MARGINS, A/B builds) -- asked of the code object once per kernel.
template <auto Kernel>
static hipError_t dynamic_lds(size_t lds) {
  const void *k = reinterpret_cast<const void *>(Kernel);
  if (lds > 64 * 1024) {
    const hipError_t e = hipFuncSetAttribute(k, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    if (e != hipSuccess) return e;
  }
  static const hipError_t no_static = [k] {
    hipFuncAttributes a{};
    const hipError_t e = hipFuncGetAttributes(&a, k);
    return e != hipSuccess ? e : a.sharedSizeBytes == 0 ? hipSuccess : hipErrorInvalidConfiguration;
  }();
  return no_static;
}

// The specialisations that are instantiated; a feature set outside them uses the last, which has every feature.
constexpr uint32_t kVariants[] = {0u, F_TRIS, F_SPHERE, F_TRIS | F_SPHERE, F_SPHERE | F_SGROUP, F_TRIS | F_SPHERE | F_SGROUP,
                                  F_TRIS | F_BVH, F_TRIS | F_SPHERE | F_TEX, F_ALL};
// The query variants (rtmi_intersect, rtmi_occluded, rtmi_trace, rtmi_render_budget): F_TEX always (closest_hit tracks
// the winner's u, v bitwise only then), never F_DEFOCUS (no camera is involved): the render variants so mapped.
constexpr uint32_t kQueryVariants[] = {F_TEX, F_TRIS | F_TEX, F_SPHERE | F_TEX, F_TRIS | F_SPHERE | F_TEX,
                                       F_SPHERE | F_SGROUP | F_TEX, F_TRIS | F_SPHERE | F_SGROUP | F_TEX,
                                       F_TRIS | F_BVH | F_TEX, F_ALL & ~F_DEFOCUS};
// (pick_variant: render.hip; pick_query_variant: queries.hip; both declared in kernels.h)
template <size_t N>
static uint32_t pick_listed(const uint32_t (&list)[N], uint32_t features) {
  for (const uint32_t v : list)
    if ((features & ~v) == 0) return v;
  return list[N - 1];
}
// f(std::integral_constant<uint32_t, V>()) for the variant V of List that equals `variant`; `otherwise` for any other.
template <const auto &List, size_t I = 0, class R, class Fn>
static R with_listed(uint32_t variant, R otherwise, Fn &&f) {
  if constexpr (I == std::size(List)) return otherwise;
  else if (variant == List[I]) return f(std::integral_constant<uint32_t, List[I]>());
  else return with_listed<List, I + 1>(variant, otherwise, f);
}

// *per_cu = workgroups of Kernel per compute unit at this launch shape; 0 with an error: it does not fit, or the HIP
// call that failed.
template <auto Kernel>
static hipError_t kernel_occupancy(int threads, size_t lds, int *per_cu) {
  *per_cu = 0;
  if (lds > 160 * 1024) return hipErrorInvalidConfiguration;
  hipError_t e = dynamic_lds<Kernel>(lds);
  if (e == hipSuccess) e = hipOccupancyMaxActiveBlocksPerMultiprocessor(per_cu, Kernel, threads, lds);
  if (e != hipSuccess) *per_cu = 0;
  return e;
}
// A launch of Kernel on its argument block: the block goes to d_block in stream order, just before the kernel that reads it.
struct LaunchAt {
  int blocks, threads;
  size_t lds;
  hipStream_t stream;
};
template <auto Kernel, class P>
static hipError_t launch_block(const LaunchAt &at, const P &block, P *d_block) {
  const hipError_t e = dynamic_lds<Kernel>(at.lds);
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(params_write_kernel<P>, dim3(1), dim3(64), 0, at.stream, block, d_block);
  hipLaunchKernelGGL(Kernel, dim3(at.blocks), dim3(at.threads), at.lds, at.stream, (const P *)d_block);
  return hipGetLastError();
}
