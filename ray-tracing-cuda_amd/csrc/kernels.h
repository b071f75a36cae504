// Internal launch interface between the C ABI (capi.hip) and the kernels.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <vector>

#include "../../include/rtmi.h"  // RTMI_COUNTER_WORDS
#include "scene_dev.h"

#define RTMI_KERNEL_MAX_DEPTH 64  // == RTMI_MAX_DEPTH of include/rtmi.h

namespace rtmi {

#include "path_list.h"  // PathList: the candidates of a list, as the wavefront launchers below take them

int64_t frame_pixel_of(const FrameDev &fr, int rank, int64_t q);

// first >= 0: fr.items states of subsequences first, first + 1, ... (rtmi_rng_init_n) instead of the frame's pixels
hipError_t launch_rng_init(uint64_t seed, const FrameDev &fr, const uint32_t *d_jump, uint32_t *d_states,
                           hipStream_t stream, int64_t first = -1);

// Kernel specialisation covering a feature set, its occupancy, and its launch.
uint32_t pick_variant(uint32_t features);
// fast_path: the launch may be one of the fast kernels: the answer holds for whichever is launched.
int render_occupancy(uint32_t variant, const SceneDev &sc, const FrameDev &fr, int threads, bool fast_path = false);
// d_tile_order (nullable): the work queue hands out local tile d_tile_order[k] as its k-th tile.
// d_sparse_items (nullable; needs d_tile_order): device word, how many leading work items are outlier
// tiles that mesh kernels spread one pixel per tune.sparse_stride lanes (launch_tile_order writes it to d_max[1]).
// probe: launch under the probe_kernel name (the scheduler's cost-estimation pass).
// Per-call scheduling parameters (capi.hip fills them from rtmi_render_opts over the process defaults).
struct RenderTuning {
  int schedule;       // 0 image order, 1 longest-first when it can pay, 2 always longest-first
  int blocks_per_cu;  // 0: as many as fit
  int threads;        // 0: chosen per kernel variant
  int sparse_stride;  // outlier tiles of mesh frames: one pixel per this many lanes (power of two, 1..64)
  int exclusive;      // 1: a wave holding an outlier pixel takes no other new pixels (its lanes work for it)
  int outlier_x10;    // a tile is an outlier from this many tenths of the mean tile cost
  int head_pct[3];    // mesh frames: per cent of the frame's largest probe count from which a pixel gets a wave to itself,
                      // shares one with another, gets one lane in 16 (80 / 55 / 30)
  int probe_spp;      // samples per pixel of the scheduler's cost probe; 0: chosen per frame (capi.hip)
  int promote;        // samples after which a mesh frame's pixel may be promoted to a head class by its own ray count; 0: never
  int first_pass;     // 0: the scheduler's probe is rendered on scratch copies and discarded; 1: it is the frame's own first spp / 16
                      // samples (the second launch resumes); N > 1: spp / N
  int cost_probe;     // mesh frames: 1 = the probe books its searches' lane-steps per pixel and the queue follows that cost
  int lane_stride;    // list frames smaller than the grid: one pixel per this many lanes (power of two; 0: chosen per frame)
  int plan;           // 1: list frames with a probe behind them are rendered as planned chains (launch_chain_plan), not from the queue
  int prio_every;     // > 0: the waves of a SIMD are served longest-remaining-chain-first, each looking at its priority every
                      // this many iterations (a power of two); 0: the hardware's oldest-first order
  int fast_path;      // 1: a launch whose run-time modes are all the common ones uses the kernel compiled for them (below)
  int head_classes;   // mesh frames: 1 = the head of the queue is pixels in weight classes; 0 (or a call that names a sparse stride) = outlier tiles
  int first_prio;     // 1: a first pass of the frame's own samples has wave priorities from 32 samples on
  int fetch_batch, fetch_batch_first;  // list frames: the largest batch a wave draws from the queue per atomic in longest-first order /
                                       // in a first pass of a few samples (1..64; A/B measurements)
};

// Compile-time mode word of the trace kernel (render_body.h, closest_hit.h: template parameter M).  One kernel body
// serves every scene, frame and schedule, and decides between them at run time, from wave-uniform fields that never
// change during a launch.  A set bit PINS one of those decisions: the body is compiled with the answer known, the other
// side of the branch is not emitted and the value it was read from is not kept in a register across the loop.  M == 0
// pins nothing and compiles to the kernel as it was.  What a bit promises the HOST must have checked: fast_path_mode.
enum : uint32_t {
  PIN_NIBBLE_IDS = 1u << 0,    // lc.wide_ids == 2: at most 16 materials, two levels of the id stack per byte
  PIN_LDS_TABLES = 1u << 1,    // materials, pair corners and normals staged in LDS; the culled list scan with shared tests
  PIN_UNSIGNED = 1u << 2,      // sc.unsigned_colours (with the two above: the four-levels-at-a-time fold alone)
  PIN_DET_SAFE = 1u << 3,      // sc.det_safe
  PIN_POW2_FRAME = 1u << 4,    // width and height powers of two up to 2^20: the jitter in binary32
  PIN_EVERY_LANE = 1u << 5,    // lc.lane_stride == 1
  PIN_PRIORITIES = 1u << 6,    // lc.prio_tab != nullptr
  PIN_CHAINS = 1u << 7,        // planned chains on a resumed pass: lc.chain_next, lc.tile_cost, ray_counts set, fr.k_begin > 0
  PIN_QUEUE = 1u << 8,         // the wave draws from the queue: lc.chain_next == nullptr
  PIN_DIFFUSE = 1u << 9,       // sc.diffuse_only: every material is a Lambertian or a light, none textured (with kFastCommon)
};
constexpr uint32_t kFastCommon = PIN_NIBBLE_IDS | PIN_LDS_TABLES | PIN_UNSIGNED | PIN_DET_SAFE | PIN_POW2_FRAME |
                                 PIN_EVERY_LANE | PIN_PRIORITIES;
constexpr uint32_t kFastChains = kFastCommon | PIN_CHAINS;  // the second launch of a planned frame (C2, a C4 shard)
constexpr uint32_t kFastQueue = kFastCommon | PIN_QUEUE;    // a first pass, a queued or image-order frame
// The trace loop of the two kernels above normalises a Lambertian bounce's direction one iteration late, at the site
// that normalises the new camera rays (render_body.h: kOwesBit).  The M == 0 render kernels and the caller-owned trace,
// budget and feature kernels keep both sites and compile to what they were: their registers moved both ways with the
// deferral (NOTES.md, "Deferred normalisation") and no benchmark line runs them long enough to tell a 2 % from noise.
constexpr bool defers_unit(uint32_t m) { return (m & kFastCommon) == kFastCommon; }
// The culled list scan of the same kernels tests each pair in centre / half-extent form against the PairSlab table
// (scene_dev.h), whose half extents hold the distance slack of every origin within kOriginReach x list_mag: three FMAs
// per axis, no per-ray slack and no sorting of near and far (closest_hit.h).  The host has checked the reach for this
// launch's camera (fast_path_facts: pairs_in_lds).  Every other kernel keeps PairBox and the per-ray slack, and
// compiles to what it was.
constexpr bool culls_by_slab(uint32_t m) { return (m & kFastCommon) == kFastCommon; }
// The same kernels fold a flush of the culled scan's shared tests without its order: the lanes that test post one
// 64-bit key per accepted pair, (bits of t) << 32 | place in the chunk, with an LDS minimum on the ray's slot, and the
// ray's lane reads one key where it looped over result words (closest_hit.h, steps (b) and (c); DESIGN.md 2.1 says why
// the smallest key is the sequential answer, and which task is not: that flush is redone in list order).  They are
// binary32, untextured and never the occlusion engine, which is what a key of t and place alone takes for granted.
// Every other kernel keeps the result words and the fold, and compiles to what it was.
constexpr bool folds_by_min(uint32_t m) { return (m & kFastCommon) == kFastCommon; }
// The same kernels test a flush's tasks a PAIR per lane while a round of pairs runs more than kPairRoundMin / 64 full, and
// only the short rest a triangle per lane (pair_rounds.h has the schedule and why; closest_hit.h, step (b)): a pair round
// reads the ray record once, forms one address product and needs no exchange between lanes, and posts the keys the
// triangle rounds would.  -DRTMI_PAIR_ROUND_MIN=<more than kListTasks> compiles the pair rounds away: every kernel is then
// what it was before them, instruction for instruction.  Every other kernel is that anyway.
#ifndef RTMI_PAIR_ROUND_MIN
#define RTMI_PAIR_ROUND_MIN 32
#endif
constexpr int kPairRoundMin = RTMI_PAIR_ROUND_MIN;
constexpr bool pairs_full_rounds(uint32_t m) { return (m & kFastCommon) == kFastCommon; }
#include "pair_rounds.h"
// Three trims of the same kernels' instruction text that leave the arithmetic on every value as it is (NOTES.md, "Fast
// list kernels: votes, 24-bit addresses, fold colours").  RTMI_TRIM is a bit per trim so that each can be built and
// censused alone (tools/loop_census.py --extra -DRTMI_TRIM=1); the product has all three.
//   1  trims_votes: a wave vote on a compare takes its lane mask from the compare itself (trace_helpers.h: wave_all_in,
//      wave_ballot_nz ...) where __all / ballot send it through a register of 0 / 1 and a second compare.
//   2  trims_mul24: the LDS address of a staged TriPts record is one 24-bit multiply-add (full rate; the 32-bit
//      multiply issues at a quarter), kept opaque so that it is formed once (closest_hit.h: load_tri_pts).  The
//      product's bound is asserted where the layout is made (render.hip: make_cfg).  The id stack's addresses keep
//      the 32-bit multiply: with the 24-bit one the chains kernel spilled a sixth scalar (NOTES.md).
//   4  trims_fold_rgb: the radiance fold reads a layer's colour from a table of 16 rows of 16 bytes at a fixed LDS
//      address (kFoldRgbOff, staged from the material records), so a nibble of the id stack is its row's address after
//      one AND (high half) or a shift and an AND (low half).  make_cfg leaves room for it in front of the id stack of
//      every F_TRIS launch with nibble ids and a staged material table, whichever kernel that launch gets.
// Every other kernel compiles to what it was.
#ifndef RTMI_TRIM
#define RTMI_TRIM 7
#endif
constexpr bool trims_votes(uint32_t m) { return (RTMI_TRIM & 1) && (m & kFastCommon) == kFastCommon; }
constexpr bool trims_mul24(uint32_t m) { return (RTMI_TRIM & 2) && (m & kFastCommon) == kFastCommon; }
constexpr bool trims_fold_rgb(uint32_t m) { return (RTMI_TRIM & 4) && (m & kFastCommon) == kFastCommon; }
// A scene whose materials are all Lambertians or lights, none textured (SceneDev::diffuse_only: the Cornell box), gets
// the same kernels once more with PIN_DIFFUSE, whose shading path is written for that scene (render_body.h).  RTMI_DIFFUSE
// is a bit per step so that each can be built and censused alone (tools/loop_census.py --extra -DRTMI_DIFFUSE=1); step 4
// stands on step 1.  (Bit 2 was a bounce without the material record's read; it did not pay and is gone: NOTES.md, "Trace
// loop: diffuse scenes".)
//   1  diffuse_scatter: metal and dielectric are not compiled: every scatter is Lambertian, so every active lane at the
//      top of the loop owes the normalisation and kOwesBit is neither set nor tested.
//   4  diffuse_restarts: a lane whose path ends and whose pixel has samples left takes the next sample's two camera
//      draws with the first trip of the rejection sampler, and starts that sample behind it.  The camera block at the
//      top is left with the lanes that have just taken a pixel.
// The kernels without PIN_DIFFUSE compile to what they were.
#ifndef RTMI_DIFFUSE
#define RTMI_DIFFUSE 5
#endif
constexpr bool diffuse_scatter(uint32_t m) { return (RTMI_DIFFUSE & 1) && (m & PIN_DIFFUSE) && (m & kFastCommon) == kFastCommon; }
constexpr bool diffuse_restarts(uint32_t m) { return (RTMI_DIFFUSE & 4) && diffuse_scatter(m); }
// The mode word launch_render gives a launch whose plan says `fast` (0, kFastChains or kFastQueue) in this scene.
inline uint32_t render_pins(uint32_t fast, const SceneDev &sc) { return fast != 0u && sc.diffuse_only ? fast | PIN_DIFFUSE : fast; }
constexpr int kFoldRgbOff = 512;    // == 16 x sizeof(MatRec): behind the largest material table nibble ids can name
constexpr int kFoldRgbBytes = 256;  // 16 rows of r, g, b, pad
// The tasks that sent their flush through the ordered steps are counted in counters[kOrderedTasksWord], a word only
// -DRTMI_STATS builds of mesh kernels used (rtmi_debug_counters).  closest_hit sees the words from [2] on.
constexpr int kOrderedTasksWord = 16;
// -DRTMI_CHECK_MARGINS builds without -DRTMI_STATS count the pair rounds and the triangle rounds of those kernels' flushes
// in two words that otherwise only a stats build writes (rtmi_debug_counters), and in a third the tasks of the ordered kind
// that a pair round met (tasks, one by one: word 16 counts the lanes that flagged).  The product counts none of them.
constexpr int kPairRoundsWord = 37, kTriRoundsWord = 38, kPairFlagsWord = 39;
// Everything the fast kernels take for granted, as the call's plan knows it (capi.hip: plan_render).  One predicate for
// the plan, which the launch and rtmi_render_mode both read, and for the tests (rtmi_fast_path_kernel).
struct FastPathFacts {
  int enabled;           // RenderTuning::fast_path
  uint32_t variant;      // the kernel variant (pick_variant)
  int n_mats;            // materials of the scene
  int mats_in_lds;       // the material table is staged (LaunchCfg::lds_mats > 0)
  int pairs_in_lds;      // pair corners and normals are staged, the culled scan shares its tests (pairs_off, nrm_off,
                         // list_off >= 0), and the slab table's reach covers this camera: |position|inf <= kOriginReach x
                         // list_mag, with (kOriginReach + 1) x list_mag x 1e30 finite in binary32
  int unsigned_colours;  // SceneDev::unsigned_colours
  int det_safe;          // SceneDev::det_safe
  int width, height;
  int lane_stride;
  int priorities;        // the launch has a priority table
  int chains;            // the launch walks planned chains
  int resumed;           // fr.k_begin > 0 and a ray-count buffer to resume from
  int tile_cost;         // the launch has the probe's tile costs
};
// 0: the general kernel; else kFastChains or kFastQueue.
uint32_t fast_path_mode(const FastPathFacts &f);
// The facts that are known before the launch shape is (scene, frame, switch); the plan adds the lane stride and each
// launch's last four.
FastPathFacts fast_path_facts(uint32_t variant, const SceneDev &sc, const FrameDev &fr, int threads, int enabled);
// The slab table's reach covers a render from this camera (part of FastPathFacts::pairs_in_lds; host arithmetic only).
bool slab_reach_covers(float list_mag, const CameraDev &cam);
// Dynamic LDS of one workgroup of a render launch (host arithmetic only: the counts of `sc`, fr.max_depth).
size_t render_lds_bytes(uint32_t variant, const SceneDev &sc, const FrameDev &fr, int threads);
// What the scheduler's probe pass leaves for the real pass (device pointers, all optional).
struct SchedPlan {
  const uint32_t *tile_order = nullptr;    // the queue's order per quarter tile (launch_quarter_order)
  uint32_t *visit_counts = nullptr;        // probe pass of a mesh frame: receives per work item the lane-steps of its searches
  const uint32_t *sparse_items = nullptr;  // one word: leading work items handed to every sparse_stride-th lane only
                                           // (with head_list: + [1], [2] = ends of its 64- and 32-lane classes)
  const uint32_t *head_list = nullptr;     // optional: the head's work items, heaviest pixels first (kHeadCap words)
  const uint32_t *probe_marks = nullptr;   // with head_list: per work item, bit 31 set = listed in the head
  int probe_spp = 2;                       // samples per pixel of the probe behind these (thresholds: sparse_items[23..25])
  uint32_t *prio_tab = nullptr;            // optional: the wave-priority table (render_body.h: kPrioRows x 16 words, zeroed)
  const uint32_t *tile_cost = nullptr;     // optional: the probe's ray count per tile (launch_tile_order's d_cost)
  // planned chains (launch_chain_plan): all or none; with them tile_order is per TILE and prio_tab is required
  const int32_t *chain_next = nullptr;
  const uint32_t *chain_fut = nullptr;
  const int32_t *chain_first = nullptr;
  uint32_t *claims = nullptr;              // one word per tile, zeroed
  int plan_simds = 0, plan_rounds = 0;
};
// d_params: render_params_bytes() of device memory that stays untouched until the launch has finished (the kernel's
// argument block, written in stream order just before it).
size_t render_params_bytes();
// fast: the launch's mode word as the plan computed it (0: the general kernel); hipErrorInvalidValue when the block this
// launch would write breaks what a pinned kernel's bits promise.
hipError_t launch_render(uint32_t variant, const SceneDev &sc, const FrameDev &fr, uint32_t *d_states, float *d_out,
                         uint32_t *d_ray_counts, unsigned long long *d_counters, const SchedPlan &plan, bool probe,
                         uint32_t fast, int blocks, int threads, const RenderTuning &tune, void *d_params, hipStream_t stream);
// Tiles sorted by descending cost (sum of 64 ray counts each); d_cost/d_order hold n_tiles words,
// d_meta 16: [0] the largest tile cost, [1] the sparse item count.
// sparse_cap: work items the grid holds at one pixel per tune.sparse_stride lanes (a multiple of 64).
// d_head (nullable, kHeadCap words): the head's work items sorted into three classes by their own probe count --
// pixels that get a wave each, pixels that share one between two, the rest (one per 16 lanes); d_meta[2], [3] =
// where the first two classes end.  grid_waves: waves of the render launch (the classes may use a quarter of them).
constexpr int kHeadCap = 16384;
hipError_t launch_tile_order(uint32_t *d_ray_counts, int n_tiles, uint32_t *d_cost, uint32_t *d_meta,
                             uint32_t *d_order, uint32_t *d_head, uint32_t sparse_cap, int grid_waves, int outlier_x10,
                             const int head_pct[3], hipStream_t stream);

// The per-quarter-tile order the trace kernel's queue follows (4 * n_tiles words): d_order's tiles with their quarters in
// sequence, or -- d_work != nullptr: mesh frames with a cost probe -- the quarters sorted by probed cost and dealt to the
// 64-item blocks in a snake (sched.hip).  d_qcost / d_qsorted: 4 * n_tiles words of scratch each, d_qmax one word.
hipError_t launch_quarter_order(const uint32_t *d_order, const uint32_t *d_work, const uint32_t *d_rays, int n_tiles,
                                uint32_t *d_qcost, uint32_t *d_qsorted, uint32_t *d_qmax, uint32_t *d_qmap, hipStream_t stream);

// Planned chains for list frames.  The tiles in longest-first order (d_order) are dealt to the SIMDs in a snake -- SIMD s of
// S gets ranks s, 2S - 1 - s, 2S + s, ... -- so that every SIMD's share costs about the same, and a SIMD's share is dealt
// to its R waves in a snake again (its k-th tile goes to wave k, 2R - 1 - k, 2R + k, ...: the lightest first tiles are
// paired with the tiles of the second round).  Chain c = wave * S + SIMD.  d_first[c] = its first tile or -1,
// d_next[tile] = the tile after it in its chain (-1: none), d_fut[tile] = estimated queries per lane of the tiles after
// it: d_cost x spp / (64 probe_spp).  Which wave of which SIMD a wave IS it finds out when it starts (render_body.h).
hipError_t launch_chain_plan(const uint32_t *d_order, const uint32_t *d_cost, int n_tiles, int simds, int rounds, int spp,
                             int probe_spp, int32_t *d_first, int32_t *d_next, uint32_t *d_fut, hipStream_t stream);

hipError_t launch_untile(const FrameDev &fr, const float *d_tiles, float *d_image, hipStream_t stream);
hipError_t launch_untile_u32(const FrameDev &fr, const uint32_t *d_tiles, uint32_t *d_image, hipStream_t stream);
hipError_t launch_post(float *d_img, int64_t n, int spp, hipStream_t stream);
// Batched closest-hit queries (rtmi_intersect; queries.hip: query_kernel).  d_hits: n x 12 words (rtmi_hit);
// d_abandoned, d_t_max, d_check nullable (d_check: -DRTMI_CHECK_MARGINS builds only, {re-done, disagreements}).
uint32_t pick_query_variant(uint32_t features);
hipError_t launch_query(uint32_t variant, const SceneDev &sc, const QueryDev &qd, int n_cu, int64_t n, const float *d_o,
                        const float *d_d, const float *d_t_max, int32_t *d_hits, unsigned long long *d_abandoned,
                        unsigned long long *d_check, hipStream_t stream);
// Batched any-hit visibility queries (rtmi_occluded; queries.hip: occlusion_kernel), on the query variants.
// d_occluded: n bytes; d_t_max, d_counts ({abandoned, fallback rays}), d_check nullable (as launch_query).  Rays whose
// origin lies inside [near_lo, near_hi] (the padded union of the meshes' root bounds) and whose t_max is not below
// near_short start the walk from +inf.
// list (null: every ray): the same query for the listed paths only (rtmi_occluded_list; queries.hip:
// occlusion_list_kernel): launch_bounce's list, entries need not be distinct; every array keeps n paths, an unlisted
// path keeps its byte.  The grid is then sized by list->n_list >= 1.
hipError_t launch_occlusion(uint32_t variant, const SceneDev &sc, const float near_lo[3], const float near_hi[3],
                            float near_short, int n_cu, int64_t n, const PathList *list, const float *d_o, const float *d_d,
                            const float *d_t_max, uint8_t *d_occluded, unsigned long long *d_counts,
                            unsigned long long *d_check, hipStream_t stream);
// Radiance of caller rays (rtmi_trace; calls.hip: trace_kernel), on the query variants.  d_work: RTMI_TRACE_WORK_WORDS
// words, zeroed in stream order before the call -- [0] abandoned mesh searches, [1] closest-hit queries, [2] the queue's
// cursor, and from byte kCallParamsOffset the kernel's argument block (written in stream order just before the launch).
constexpr size_t kCallParamsOffset = 256;  // (a 128-byte line of its own, away from the counter words)
// tex_layers: the scene's features hold F_TEX (image textures, or more materials than the 16-bit id stack holds); without
// it the F_TEX kernel keeps the untextured id stack.
hipError_t launch_trace(uint32_t variant, const SceneDev &sc, bool tex_layers, int n_cu, int64_t n, int max_depth,
                        const float *d_o, const float *d_d, uint32_t *d_states, float *d_radiance,
                        uint32_t *d_ray_counts, unsigned long long *d_work, hipStream_t stream);
// One iteration of Trace's loop per ray (rtmi_bounce; calls.hip: bounce_kernel), on the query variants: rays and states
// are read and written in place; d_hits (n x 12 words, rtmi_hit) and d_steps nullable; d_work as launch_trace's, [1] = the
// paths stepped.  list (null: every path): the same step for the candidates of the list only (rtmi_bounce_list; calls.hip:
// bounce_list_kernel; path_list.h); every array keeps n paths.  list->n_list >= 1.
hipError_t launch_bounce(uint32_t variant, const SceneDev &sc, const QueryDev &qd, int n_cu, int64_t n, const PathList *list,
                         float *d_o, float *d_d, uint32_t *d_states, float *d_emitted, float *d_attenuation, int32_t *d_hits,
                         uint32_t *d_steps, unsigned long long *d_work, hipStream_t stream);
// The live candidates' path indices, in the candidates' order, and their number (rtmi_path_compact): three launches, no
// workgroup waits for another.  d_scratch: path_compact_scratch_bytes(n_list) bytes.
size_t path_compact_scratch_bytes(int64_t n_list);
hipError_t launch_path_compact(int64_t n, const float *d_origins, const float *d_dirs, const PathList &in, uint32_t *d_list_out,
                               uint32_t *d_count_out, uint32_t *d_scratch, hipStream_t stream);
// Workgroups of b lanes over a items (the launchers of frame.hip and paths.hip).
static inline int64_t cdiv(int64_t a, int64_t b) { return (a + b - 1) / b; }
// The grid of the kernels that take one lane per candidate (direct.hip, advance.hip): ceil(n_list / threads) workgroups,
// capped at blocks_per_cu per compute unit -- a wave then walks further chunks by its number.  n_list >= 1.
inline unsigned list_grid(uint32_t n_list, int threads, int n_cu, int blocks_per_cu) {
  const int64_t want = ((int64_t)n_list + threads - 1) / threads, cap = (int64_t)(n_cu > 0 ? n_cu : 1) * blocks_per_cu;
  return (unsigned)(want < cap ? want : cap);
}
// Trace's return expression over the first min(d_steps[i], layers) layers of the stacks float[layers][n][3] (rtmi_path_fold).
hipError_t launch_path_fold(int64_t n, int layers, const float *d_dirs, const uint32_t *d_steps, const float *d_emitted,
                            const float *d_attenuation, float *d_radiance, hipStream_t stream);
// Next-event estimation (direct.hip; the argument block and the table's device form are direct_body.h's).  The light table
// of a flattened scene as rtmi_scene_lights hands it out, and one bit per material that some table light has.
struct Scene;
struct LightRec;
struct DirectArgs;
void build_light_table(const Scene &s, std::vector<rtmi_light> *lights, std::vector<uint32_t> *light_mats);
void light_records(const std::vector<rtmi_light> &lights, std::vector<LightRec> *recs, std::vector<float> *cdf);
// The step for the candidates of a.list (rtmi_direct_sample): a.n_list >= 1.
hipError_t launch_direct_sample(const DirectArgs &a, int n_cu, hipStream_t stream);
// The light of a hit, per entry and box face (rtmi_direct_sample_mis; direct_body.h: LightDev::hit_light), and that step.
struct DirectMisArgs;
void build_hit_light_map(const std::vector<rtmi_light> &lights, std::vector<int32_t> *map, int32_t *n_entries);
hipError_t launch_direct_sample_mis(const DirectMisArgs &a, int n_cu, hipStream_t stream);
// Either step on a scene whose table holds a sphere light (Scene::sphere_lights): the plain one with a null carry.
hipError_t launch_direct_sample_sph(const DirectMisArgs &a, bool mis, int n_cu, hipStream_t stream);
// rtmi_path_fold with T[k] = d_occluded[k] ? E[k] : E[k] + D[k] for E[k] (rtmi_path_fold_direct).
hipError_t launch_path_fold_direct(int64_t n, int layers, const float *d_dirs, const uint32_t *d_steps, const float *d_emitted,
                                   const float *d_attenuation, const float *d_direct, const uint8_t *d_occluded,
                                   float *d_radiance, hipStream_t stream);
// rtmi_trace with next-event estimation inside (rtmi_trace_direct; trace_direct.hip: trace_direct_kernel<F, SPH>, render_body.h
// in its DIRECT mode): launch_trace's arguments, and dx (direct_body.h) -- the light table with the hit -> light map, the
// names of a hit, the light states and the three counters.  sphere_lights: the table holds a sphere light (the SPH twins).
struct TraceDirectBufs;
hipError_t launch_trace_direct(uint32_t variant, const SceneDev &sc, bool tex_layers, bool sphere_lights, int n_cu, int64_t n,
                               int max_depth, const float *d_o, const float *d_d, uint32_t *d_states, const TraceDirectBufs &dx,
                               float *d_radiance, uint32_t *d_ray_counts, unsigned long long *d_work, hipStream_t stream);
// Russian roulette after a step (rtmi_path_roulette; paths.hip: path_roulette_kernel): the caller's arrays as include/rtmi.h
// names them, every pointer checked by capi.hip.  n == 0 or n_list == 0 launches nothing.
struct RouletteArgs {
  const uint32_t *list, *count;  // the candidates (path_list.h), both nullable
  uint32_t n, n_list, step, first_step;
  float p_min;
  const uint32_t *steps;
  float *dirs, *attenuation, *throughput;
  uint32_t *states;
  unsigned long long *counts;  // nullable: {played, killed}, added to
};
hipError_t launch_path_roulette(const RouletteArgs &a, hipStream_t stream);
// rtmi_trace with that rule played in the lane (rtmi_trace_roulette; trace_roulette.hip: trace_roulette_kernel<F>, render_body.h
// in its ROULETTE mode): launch_trace's arguments, the rule's two parameters and its two counters (nullable).
hipError_t launch_trace_roulette(uint32_t variant, const SceneDev &sc, bool tex_layers, int n_cu, int64_t n, int max_depth,
                                 uint32_t first_step, float p_min, const float *d_o, const float *d_d, uint32_t *d_states,
                                 float *d_radiance, uint32_t *d_ray_counts, unsigned long long *d_counts,
                                 unsigned long long *d_work, hipStream_t stream);
// Per-pixel sample budgets (rtmi_render_budget; calls.hip: budget_kernel), on the query variants with F_DEFOCUS added.
// fr: the shard's frame, fr.spp = the cap on one call's samples per pixel.  d_sum, d_sq (nullable), d_samples,
// d_ray_counts (nullable) accumulate; d_work as launch_trace's (RTMI_BUDGET_WORK_WORDS words, the same layout).
hipError_t launch_budget(uint32_t variant, const SceneDev &sc, bool tex_layers, int n_cu, const FrameDev &fr,
                         const uint32_t *d_budget, uint32_t *d_states, float *d_sum, float *d_sq, uint32_t *d_samples,
                         uint32_t *d_ray_counts, const FeatureBufs *feat, unsigned long long *d_work, hipStream_t stream);
// feat (rtmi_render_features; nullable): with any buffer of it non-null the launch is feature_kernel, budget_kernel's
// twin that also adds each sample's primary-hit albedo, normal, depth and coverage into them; else budget_kernel.
// Per-item means of those sums (rtmi_resolve_features): null buffers of `out` are skipped.
hipError_t launch_resolve_features(const FrameDev &fr, const FeatureBufs &sums, const uint32_t *d_samples,
                                   const FeatureBufs &out, hipStream_t stream);
// launch_budget with next-event estimation inside (rtmi_render_direct; render_direct.hip: budget_direct_kernel<F, SPH> and
// feature_direct_kernel<F, SPH>, render_body.h in its DIRECT mode with BUDGET): dx as launch_trace_direct's, its light states
// uint32[6][fr.items].
hipError_t launch_budget_direct(uint32_t variant, const SceneDev &sc, bool tex_layers, bool sphere_lights, int n_cu,
                                const FrameDev &fr, const uint32_t *d_budget, uint32_t *d_states, const TraceDirectBufs &dx,
                                float *d_sum, float *d_sq, uint32_t *d_samples, uint32_t *d_ray_counts, const FeatureBufs *feat,
                                unsigned long long *d_work, hipStream_t stream);
// The next pass's budget per work item by the stopping rule of include/rtmi.h; d_totals[2] = {items with a budget, sum of
// budgets}, zeroed on the stream first.
hipError_t launch_budget_plan(const FrameDev &fr, int min_samples, int max_samples, int step, float tolerance, float floor,
                              const float *d_sum, const float *d_sq, const uint32_t *d_samples, uint32_t *d_budget,
                              unsigned long long *d_totals, hipStream_t stream);
// d_tiles = d_sum / d_samples per work item (0 where there are none), post != 0: then sqrt(clamp(., 0, 1)).
hipError_t launch_resolve(const FrameDev &fr, const float *d_sum, const uint32_t *d_samples, int post, float *d_tiles,
                          hipStream_t stream);
// Per-item variance of the mean from the budget sums (rtmi_resolve_variance; include/rtmi.h states the rule), tile-major.
hipError_t launch_resolve_variance(const FrameDev &fr, const float *d_sum, const float *d_sq, const uint32_t *d_samples,
                                   float *d_var, hipStream_t stream);
// The a-trous filter (rtmi_denoise; filters.hip): row-major whole-frame buffers, every pointer checked by capi.hip.
struct DenoiseCall {
  int height, width, iterations, normal_squarings, demodulate;
  float sigma_color, sigma_depth;
  const float *color, *variance, *albedo, *normal, *depth, *alpha;  // albedo: null unless demodulate
  float *out, *out_variance;                                        // out may be color; out_variance nullable
  void *scratch;                                                    // denoise_scratch_bytes(height, width) bytes
};
size_t denoise_scratch_bytes(int height, int width);
hipError_t launch_denoise(const DenoiseCall &d, hipStream_t stream);
// Temporal accumulation (rtmi_accumulate; filters.hip): row-major whole-frame buffers, every pointer checked by
// capi.hip, which also forms the camera terms in binary64 and rounds them.
struct AccumulateCall {
  int height, width;
  float normal_min, depth_tolerance, min_blend;
  float e[3], h[3], v[3], p[3];                          // this frame's camera: llc - p, horizontal, vertical, position
  float prev_p[3], r[3][3];                              // the history's: position, the inverse of [h' v' llc' - p'] by rows
  const float *color, *variance, *normal, *depth, *alpha;
  const void *history_in;                                // null: the first frame
  void *history_out;                                     // history_bytes(height, width) bytes, 16-byte aligned
  float *out, *out_variance, *out_length;                // out may be color, out_variance may be variance; the last two nullable
};
size_t history_bytes(int height, int width);
hipError_t launch_accumulate(const AccumulateCall &c, hipStream_t stream);
// The render's primary rays of one sample (rtmi_camera_rays; frame.hip): kind = RTMI_PROJ_*, w = the camera frame's
// third axis, d_budget nullable.  Inactive items get six +0.0f and keep their state.
hipError_t launch_camera_rays(const FrameDev &fr, const CameraDev &cam, const float w[3], int kind, float fov,
                              const uint32_t *d_budget, uint32_t sample, uint32_t *d_states, float *d_origins,
                              float *d_dirs, hipStream_t stream);
// One traced sample folded into the budget buffers (rtmi_sample_add): d_budget, d_trace_counts, d_sq, d_ray_counts nullable.
hipError_t launch_sample_add(const FrameDev &fr, const uint32_t *d_budget, uint32_t sample, const float *d_radiance,
                             const uint32_t *d_trace_counts, float *d_sum, float *d_sq, uint32_t *d_samples,
                             uint32_t *d_ray_counts, hipStream_t stream);
// Ended paths finished and refilled in place (rtmi_path_advance; advance.hip, advance_body.h): the caller's arrays as
// include/rtmi.h names them, every pointer checked by capi.hip.  The camera and the projection as launch_camera_rays takes
// them.  list.n_list >= 1.
struct AdvanceCall {
  const uint32_t *budget;  // nullable
  PathList list;
  float *origins, *dirs;
  uint32_t *states, *steps;
  const float *emitted, *attenuation;
  float *emitted_stack, *attenuation_stack;  // null only with max_depth == 0
  uint32_t *cursor;
  float *sum, *sq;                 // sq nullable
  uint32_t *samples, *ray_counts;  // ray_counts nullable
  unsigned long long *counts;      // nullable
};
hipError_t launch_path_advance(const FrameDev &fr, const CameraDev &cam, const float w[3], int kind, float fov,
                               const AdvanceCall &c, int n_cu, hipStream_t stream);
#ifdef RTMI_STATS
hipError_t copy_wave_stats(unsigned long long *host, size_t bytes);  // diagnostic builds only
#endif
#ifdef RTMI_CHECK_MARGINS
hipError_t launch_add_one(unsigned long long *d_word, hipStream_t stream);  // *d_word += 1 (check builds' test hook)
#endif
// d_bad[4]: see arithmetic_selftest in frame.hip.
hipError_t launch_arithmetic_selftest(unsigned long long *d_bad, hipStream_t stream);

}  // namespace rtmi
