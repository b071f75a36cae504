// The one launcher of the entries that own their device state (calls.hip: rtmi_trace, rtmi_render_budget,
// rtmi_render_features, rtmi_bounce, rtmi_bounce_list; trace_direct.hip: rtmi_trace_direct; render_direct.hip:
// rtmi_render_direct).  Host templates only.
#pragma once
// (included inside namespace rtmi, after render_body.h and launch_cfg.h)

// ------------------------------------------------------------------ the entries that own their device state
// rtmi_trace, rtmi_render_budget, rtmi_render_features: render_body.h in a mode of Kernel's on the query variants (F_TEX
// always: the layer stack is one 32-bit word per level, the material id or the sampled texel -- or, without tex_layers,
// the untextured id stack).  A persistent grid sized by occupancy; the lanes refill from the call's own queue cursor
// (d_work[2]) as their items end, fetch_batch items per wave per atomic.  The argument block is written behind the
// counter words of d_work.
// Block: the kernel's argument block, CallParams or a type derived from it whose own fields `tail(block)` fills in.
template <uint32_t F, auto Kernel, class Block = CallParams, class Tail = std::nullptr_t>
static hipError_t launch_call(const SceneDev &sc, const FrameDev &fr, bool tex_layers, int fetch_batch, int n_cu,
                              CallExtras ex, uint32_t *d_states, float *d_out, uint32_t *d_ray_counts,
                              unsigned long long *d_work, hipStream_t stream, bool id_stack = true,
                              int64_t grid_items = -1,  // (>= 0: the items the grid is capped by, when not fr.items)
                              Tail tail = nullptr) {
  static_assert(std::is_base_of_v<CallParams, Block>, "the block starts with the trace kernel's");
  static_assert(kCallParamsOffset + sizeof(Block) <= (size_t)RTMI_TRACE_WORK_WORDS * 8u, "d_work must hold the argument block");
  // workgroup size: the one that keeps the most lanes resident (a deep 32-bit layer stack can leave room for one
  // 256-lane workgroup per CU only, as for the render's mesh variants: capi.hip launch_shape)
  int threads = 0, per_cu = 0;
  for (int t = 256; t >= 64; t /= 2) {
    size_t lds_t = 0;
    (void)make_cfg(F, sc, fr, t, &lds_t, true, id_stack, tex_layers);
    int nb = 0;
    (void)kernel_occupancy<Kernel>(t, lds_t, &nb);
    if (t * nb > threads * per_cu) threads = t, per_cu = nb;
  }
  if (per_cu < 1) return hipErrorInvalidConfiguration;  // (the staged tables and the stack do not fit a CU's LDS)
  size_t lds = 0;
  Block cp;
  cp.rp.sc = sc, cp.rp.fr = fr, cp.rp.lc = make_cfg(F, sc, fr, threads, &lds, true, id_stack, tex_layers);
  cp.rp.lc.lane_stride = 1, cp.rp.lc.fetch_batch = fetch_batch, cp.rp.lc.rate_scale = 1.f;
  cp.rp.states = d_states, cp.rp.out = d_out, cp.rp.ray_counts = d_ray_counts, cp.rp.counters = d_work;
  cp.ex = ex, cp.ex.tex_layers = tex_layers ? 1 : 0;
  const int64_t want = ((grid_items >= 0 ? grid_items : fr.items) + threads - 1) / threads, cap = (int64_t)n_cu * per_cu;
  if constexpr (!std::is_same_v<Tail, std::nullptr_t>) tail(cp);
  return launch_block<Kernel>(LaunchAt{(int)(want < cap ? want : cap), threads, lds, stream}, cp,
                              reinterpret_cast<Block *>(reinterpret_cast<char *>(d_work) + kCallParamsOffset));
}

// The frame of a batch of n caller rays or paths: one item each, one sample, the whole batch one rank's.
static FrameDev batch_frame(int64_t n, int max_depth) {
  FrameDev fr{};
  fr.height = 1, fr.width = 1, fr.spp = 1, fr.max_depth = max_depth, fr.post = 0;
  fr.k_begin = 0, fr.k_end = 1, fr.rank = 0, fr.world = 1;
  fr.items = n;
  return fr;
}

