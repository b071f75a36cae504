/*
 * rtmi.h — C ABI of the MI355X-native path-tracing hot path (librtmi.so).
 *
 * This is the drop-in boundary for the per-pixel trace loop of
 * tigert1998/ray-tracing-cuda.  Every entry point names the reference
 * interface it replaces (paths relative to /root/reference/ray-tracing-cuda/).
 * The reference's host driver (`Main` / `DistributedMain`, utils.cu:132-242)
 * performs, in order: allocate states+image -> CudaRandomInit kernel ->
 * user `init_world` callback -> PathTracing kernel -> D2H -> (MPI reduce) ->
 * JPEG.  The calls below are those steps with plain pointers and sizes.
 *
 * Conventions
 *   - All functions return 0 on success or a negative rtmi_status; the message
 *     is available from rtmi_last_error() (thread-local).  The reference aborts
 *     through glog CHECK (utils.cu:143-144); the C++ wrappers in
 *     ray-tracing-cuda_amd/api/utils.cuh turn a non-zero status into the same CHECK failure.
 *   - `d_*` pointers are device (HBM) pointers owned by the caller.
 *   - `stream` is a hipStream_t passed as void* (NULL = the null stream).  All
 *     device work is enqueued on it; functions documented "synchronous" wait
 *     for it before returning.
 *   - There is NO CPU fallback: every compute entry point fails with
 *     RTMI_ERR_NO_DEVICE when no gfx950-class device is usable.
 *
 * Pixel ownership (multi-GPU): the frame is cut into 8x8-pixel tiles numbered
 * row-major; rank r of world_size G owns tiles t with t % G == r.  A rank's
 * pixels are addressed by *work item* q in [0, rtmi_frame_work_items()):
 * local tile q/64, pixel-in-tile q%64 (row-major 8x8).  RNG states and the
 * radiance buffer of a rank are indexed by q ("tile-major").  Every pixel keeps
 * cuRAND subsequence == its GLOBAL index i*width+j, so the image is
 * bit-identical for every world_size.  Work items that fall outside the image
 * (ragged right/bottom tiles) are inert padding.
 */
#ifndef RTMI_H_
#define RTMI_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define RTMI_VERSION 3
#define RTMI_TILE 8            /* tile edge in pixels; 64 work items per tile = one wavefront */
#define RTMI_STATE_WORDS 6     /* live words of curandState: d, v[0..4] */

typedef enum rtmi_status {
  RTMI_OK = 0,
  RTMI_ERR_INVALID = -1,    /* bad argument / scene not committed / handle out of range */
  RTMI_ERR_NO_DEVICE = -2,  /* HIP runtime or device unavailable */
  RTMI_ERR_HIP = -3,        /* a HIP call failed; see rtmi_last_error() */
  RTMI_ERR_CAPACITY = -4,   /* HitableList::kMaxHitables (1024) exceeded, hitable_list.cuh:10; or a scene of more than */
                            /* RTMI_MAX_MATERIALS materials committed */
  RTMI_ERR_DEPTH = -5,      /* max_depth outside [0, RTMI_MAX_DEPTH] */
  RTMI_ERR_INTERNAL = -6    /* an internal invariant of the kernels did not hold; the output is not to be used */
} rtmi_status;

#define RTMI_MAX_DEPTH 64      /* TRACE_DEPTH_LIMIT is 10 in ray_tracing.cu:10; BASELINE configs use 8/10/50 */
#define RTMI_MAX_HITABLES 1024 /* hitable_list.cuh:10 */
/* Materials of one scene (the reference has no limit).  World-list triangles and parallelograms carry their material
 * in a 24-bit field, so rtmi_scene_commit refuses a scene with more materials with RTMI_ERR_CAPACITY. */
#define RTMI_MAX_MATERIALS (1 << 24)

typedef struct rtmi_scene rtmi_scene; /* opaque; replaces the device-resident HitableList + Camera pair */

/* Frame + shard description; replaces the (height, width, spp, post_processing)
 * arguments of PathTracing (ray_tracing.cuh:19-21) and the rank/world_size of
 * DistributedMain (utils.cu:186-189). */
typedef struct rtmi_frame {
  int32_t height;       /* 1 .. RTMI_MAX_EXTENT (the reference has no such limit: a pixel's row and column share one */
  int32_t width;        /* 32-bit register of the trace kernel); a larger frame is refused with RTMI_ERR_INVALID */
  int32_t spp;          /* samples per pixel rendered by THIS call; spp * (max_depth + 1) <= RTMI_MAX_PIXEL_QUERIES (a */
                        /* pixel's closest-hit queries are counted in 31 bits), else rtmi_render refuses the frame */
  int32_t max_depth;    /* TRACE_DEPTH_LIMIT, ray_tracing.cu:10,23 */
  int32_t post_process; /* 1: out = sqrt(clamp(sum/spp,0,1)) (ray_tracing.cu:78-83); 0: raw sum */
  int32_t rank;         /* tile shard owner, 0 <= rank < world_size */
  int32_t world_size;   /* number of shards (GPUs) */
} rtmi_frame;

#define RTMI_MAX_EXTENT 65535
#define RTMI_MAX_PIXEL_QUERIES 2147483647
const char *rtmi_last_error(void);
int rtmi_version(void);
/* Number of usable GPUs (0 when there is none); never fails. */
int rtmi_device_count(void);

/* ------------------------------------------------------------------ scene --
 * Host-side recording of the scene graph, one call per reference constructor.
 * Texture / material calls return a handle >= 0 (or a negative rtmi_status).
 * Hitables are appended to the world in call order == HitableList::Append
 * order (hitable_list.cu:27-29); list order decides ties (hitable_list.cu:18). */
rtmi_scene *rtmi_scene_create(void);
void rtmi_scene_destroy(rtmi_scene *s);

int rtmi_constant_texture(rtmi_scene *s, const float rgb[3]);                 /* textures/constant_texture.cu:7-9 */
int rtmi_image_texture(rtmi_scene *s, const uint8_t *rgba, int height, int width,
                       size_t pitch_bytes);                                   /* textures/image_texture.cu:17-38 (host RGBA8, point/wrap) */
int rtmi_lambertian(rtmi_scene *s, const float rgb[3]);                        /* lambertian.cu:14-17 */
int rtmi_lambertian_tex(rtmi_scene *s, int texture);                           /* lambertian.cu:9-12 */
int rtmi_metal(rtmi_scene *s, const float rgb[3], float fuzz);                 /* metal.cu:7-10 */
int rtmi_dielectric(rtmi_scene *s, const float rgb[3], double refractive_index); /* dielectric.cu:10-14 */
int rtmi_diffuse_light(rtmi_scene *s, int texture);                            /* diffuse_light.cu:15-17 */

int rtmi_add_sphere(rtmi_scene *s, const float center[3], double radius, int material);       /* sphere.cu:7-9 */
int rtmi_add_triangle(rtmi_scene *s, const float p[9], int material);                           /* triangle.cu:6-9 */
int rtmi_add_parallelogram(rtmi_scene *s, const float p[9], int material);                      /* parallelogram.cu:10-15 */
int rtmi_add_parallelepiped(rtmi_scene *s, const float p[12], int material);                    /* parallelepiped.cu:8-18 */
typedef void (*rtmi_transform_fn)(const float in[3], float out[3], void *user);
int rtmi_add_parallelepiped_lengths(rtmi_scene *s, const float lengths[3], int material,
                                    rtmi_transform_fn transform, void *user);                   /* parallelepiped.cu:34-55 */
/* A Parallelepiped given as the six parallelograms AddCorner appended (3 points each, 54
 * floats); used when the corners were derived elsewhere (device-side constructors). */
int rtmi_add_parallelepiped_faces(rtmi_scene *s, const float faces[54], int material);          /* parallelepiped.cu:25-32 */
int rtmi_add_sky(rtmi_scene *s);                                                                /* sky.cu:16 */
/* A HitableList appended to the list under construction (HitableList is itself a Hitable,
 * hitable_list.cuh:8): `l = new HitableList(); l->Append(...); parent->Append(l)`.  The hitables added
 * between begin and end are its entries; lists nest to any depth.  It counts as one entry of its
 * parent and holds up to RTMI_MAX_HITABLES entries of its own.  The library inlines it at its position:
 * the closest hit -- ties included -- is the one the nested call returns (DESIGN.md "List flattening"). */
int rtmi_list_begin(rtmi_scene *s);
int rtmi_list_end(rtmi_scene *s);
/* BVH<Face<HasTexCoord>,AABB>(faces, n, material) (bvh.cuh:170-173).  faces:
 * n*9 floats; uvs: n*6 floats or NULL (Face<false>); material < 0 keeps
 * "material_ptr_ == nullptr" (bvh.cuh:178).  leaf_max is BVHNode::kMin (2048,
 * bvh.cuh:105); pass 0 for the reference value. */
int rtmi_add_bvh(rtmi_scene *s, const float *faces, const float *uvs, int n, int material, int leaf_max);

int rtmi_camera_pinhole(rtmi_scene *s, const float pos[3], const float look_at[3], const float up[3],
                        double fov, double aspect);                                              /* camera.cu:24-38 */
int rtmi_camera_defocus(rtmi_scene *s, const float pos[3], const float look_at[3], const float up[3],
                        double fov, double aspect, double aperture, double focus_distance);     /* camera.cu:6-22 */
int rtmi_camera_raw(rtmi_scene *s, const float pos[3], const float lower_left[3], const float horizontal[3],
                    const float vertical[3]);                                                    /* camera.cu:40-47 */
/* position, lower_left_corner, horizontal, vertical, u, v, w (21 floats) */
int rtmi_camera_get(const rtmi_scene *s, float out[21]);
/* Install a camera whose frame was computed elsewhere (a Camera constructed on the device):
 * the same 21 floats, is_defocus_camera_ and lens_radius_ (camera.cuh:12-14). */
int rtmi_camera_set(rtmi_scene *s, const float frame[21], int is_defocus, double lens_radius);
/* Move the camera of a COMMITTED scene without committing again (added without a version change: a caller detects it by
 * the symbol).  The arguments are rtmi_camera_set's.  On an uncommitted scene it is rtmi_camera_set.  On a committed one it
 * replaces the camera in the scene's host record and in the committed scene, which stays committed: no HIP call is made,
 * nothing is uploaded and no search tree is rebuilt, because the camera lives on the host and every launch copies it by
 * value into its argument block at enqueue time.  So work enqueued BEFORE the call keeps the camera it was enqueued with
 * -- rtmi_render / rtmi_render_ex with and without d_scratch, rtmi_render_budget and rtmi_render_features alike -- and
 * the update needs no synchronisation with it.  rtmi_intersect, rtmi_occluded and rtmi_trace do not read the camera.  The
 * one thing a commit derives from the camera, whether the render kernel draws lens offsets (is_defocus), is derived again
 * here.  Like every call that changes a scene, it must not run concurrently with another call on the same scene.
 * RTMI_ERR_INVALID for a null argument or a non-finite float in frame.
 * The 21 floats of a look-at camera come from a throw-away scene: rtmi_scene_create, rtmi_camera_pinhole (or _defocus),
 * rtmi_camera_get, rtmi_scene_destroy, none of which touches the device. */
int rtmi_camera_update(rtmi_scene *s, const float frame[21], int is_defocus, double lens_radius);

/* Flatten the recorded graph into the device layout and upload it to the
 * current HIP device.  Synchronous.  Replaces the point in Main where
 * init_world has run and cudaDeviceSynchronize returns (utils.cu:148-152). */
int rtmi_scene_commit(rtmi_scene *s);
/* Counts of the flattened scene: {entries of the world list (a nested list counts once), spheres,
 * parallelograms (incl. box faces), triangles, bvh faces, bvh nodes, materials, textures}. */
int rtmi_scene_stats(const rtmi_scene *s, int64_t out[8]);
/* Mesh faces whose smallest interior angle is below 1.8 degrees (sine below 1/32).  The reference's binary32 triangle
 * test (utils.cu:49-85) accepts rays that pass such a face at a distance of about eps x (distance to the ray's origin)
 * / sin(angle) -- further than the 2^-16 distance slack every search box gets.  Since round 3 the nodes of the search
 * tree above a thin face widen their children's boxes by what it asks for (8 eps / sin(angle), as a power of two), so
 * the count is informational: the search cost of rays that come near those nodes grows with it, exactness does not
 * depend on it (tests: test_far_views_and_thin_faces, test_needles_and_grazing_views_match_the_oracle;
 * tools/gpu_check_margins.py meshes re-answers every query by the reference's own tree walk). */
int64_t rtmi_scene_sliver_faces(const rtmi_scene *s);
/* Algorithmic bytes one closest-hit query consults; BVH scenes
 * need the measured per-ray node/face visits and report only the fixed part. */
int64_t rtmi_scene_bytes_per_ray(const rtmi_scene *s);

/* ------------------------------------------------------------------ frame -- */
/* Work items (pixels incl. ragged-tile padding) owned by frame->rank. */
int64_t rtmi_frame_work_items(const rtmi_frame *f);
/* Global pixel index (i*width+j) of work item q of this shard, or -1 for padding. */
int64_t rtmi_frame_pixel_of(const rtmi_frame *f, int64_t q);
/* Bulk form: out[q] for every work item q of this shard (out has rtmi_frame_work_items entries). */
int rtmi_frame_pixel_map(const rtmi_frame *f, int64_t *out);
/* Bytes the caller must allocate for d_states / d_tiles of this shard. */
size_t rtmi_states_bytes(const rtmi_frame *f);   /* 6 planes of uint32[work_items] (struct-of-arrays) */
size_t rtmi_tiles_bytes(const rtmi_frame *f);    /* float[work_items][3] */

/* -------------------------------------------------------------------- RNG --
 * Replaces CudaRandomInit<<<>>>(seed, states, n) (utils.cu:43-47,146,202):
 * state(q) = curand_init(seed, subsequence = global pixel index, offset 0).
 * Asynchronous on `stream`. */
int rtmi_rng_init(uint64_t seed, const rtmi_frame *f, void *d_states, void *stream);
/* Host copy of curand_init(seed, subsequence, 0): {d, v0..v4}. */
int rtmi_rng_host_state(uint64_t seed, uint64_t subsequence, uint32_t state[RTMI_STATE_WORDS]);
/* CudaRandomFloat(min, max, state) on a host state (utils.cuh:22-27); scene
 * programs that draw their layout from pixel 0's stream (scenes/spheres.cu:105)
 * use this and then store the advanced state with rtmi_rng_set_state. */
float rtmi_rng_host_random_float(float min, float max, uint32_t state[RTMI_STATE_WORDS]);
/* Overwrite / read back the state of work item q.  Synchronous. */
int rtmi_rng_set_state(const rtmi_frame *f, void *d_states, int64_t q, const uint32_t state[RTMI_STATE_WORDS],
                       void *stream);
int rtmi_rng_get_state(const rtmi_frame *f, const void *d_states, int64_t q, uint32_t state[RTMI_STATE_WORDS],
                       void *stream);

/* ----------------------------------------------------------------- render --
 * Replaces PathTracing<<<grid,block>>>(world, camera, H, W, spp, post, states,
 * out) (ray_tracing.cu:56-85; launches utils.cu:158-163, 216-221) for the
 * pixels of frame->rank.  d_tiles receives float[work_items][3] (tile-major);
 * d_ray_counts (nullable) receives the per-pixel number of closest-hit queries
 * issued by Trace (ray_tracing.cu:22).  RNG states are advanced in place.
 * Asynchronous on `stream`. */
int rtmi_render(const rtmi_scene *s, const rtmi_frame *f, void *d_states, float *d_tiles,
                uint32_t *d_ray_counts, void *stream);
/* Did the render complete?  Waits for `stream`, then returns RTMI_OK, or RTMI_ERR_INTERNAL when the render
 * abandoned a mesh search, over both launches of a resumed frame (the frame is then incomplete and must not be
 * used).  `d_scratch`: the
 * rtmi_render_opts.d_scratch that call was given, or NULL for a call without one (the most recent such call on
 * this scene).  out_rays (nullable) receives the call's total of closest-hit queries.  The reference has no
 * counterpart: its CHECKs abort (utils.cu:164-166). */
int rtmi_render_status(const rtmi_scene *s, const void *d_scratch, uint64_t *out_rays, void *stream);
/* rtmi_render_status(s, NULL, out_rays, stream). */
int rtmi_last_ray_total(const rtmi_scene *s, uint64_t *out_rays, void *stream);
/* Diagnostic: the raw device counter words of a render ([0] work-queue head, [1] closest-hit queries,
 * [2] abandoned mesh searches, [3] head-queue cursor; a -DRTMI_STATS build of the kernels adds wave-level
 * step counts of the mesh search from word 4 on; a -DRTMI_CHECK_MARGINS build counts, in [33] / [34], the
 * sampled queries it re-did without the cull and the disagreements it found; [16], in every build, counts the
 * pair tasks of the fast list kernels' culled scan both of whose triangles passed with the second one nearer: the
 * flushes that held one were folded in list order, every other by one minimum per ray.  It counts them by the lanes
 * that met one in a flush, so two such tasks of one flush that fall to the same lane count once; which lane a task
 * falls to depends on the flush's schedule of rounds, so the word may differ by such coincidences between versions of
 * the library, never the image.  A -DRTMI_CHECK_MARGINS build without -DRTMI_STATS also counts, in [37] / [38], the
 * rounds in which those kernels tested a flush's tasks a pair per lane and a triangle per lane, and in [39] the tasks
 * of that kind met in a pair round, one by one -- words that otherwise only a stats build writes).  [2], [33] and [34] count over
 * both launches of a resumed frame (a first pass the frame keeps, then the rest); the other words are the last
 * launch's, whose [1] is still the whole frame's total because a resumed pixel carries its count on. */
#define RTMI_COUNTER_WORDS 40
int rtmi_debug_counters(const rtmi_scene *s, unsigned long long out[RTMI_COUNTER_WORDS], void *stream);
int rtmi_debug_counters_ex(const rtmi_scene *s, const void *d_scratch, unsigned long long out[RTMI_COUNTER_WORDS],
                           void *stream);
/* Diagnostic (added without a version change): the byte offsets of the regions of a frame's render scratch
 * (rtmi_render_scratch_bytes), in the order the library lays them out; out receives the first min(n,
 * RTMI_SCRATCH_REGIONS).  Host arithmetic only: no device, no scene.
 *   [0] states   the probe's RNG states; a resumed frame: the first pass's ray counts, marked (uint32[items])
 *   [1] rays     a discarded probe's ray counts, marked        [2] cost     per tile: rays of the first pass
 *   [3] order    tiles, dearest cost bucket first              [4] meta     32 words, see rtmi_debug_schedule
 *   [5] head     the head list (16384 words)                   [6] work     the probe's work counts per item
 *   [7] qcost    [8] qsorted   [9] qmap   per quarter tile: cost, dearest bucket first, the queue's order
 *   [10] qmax    the largest quarter cost                      [11] fut  [12] next  [13] claims   per tile: the chain plan
 *   [14] first   per chain: its first tile (32768 words)       [15] prio_tab  the wave-priority table
 *   [16] params  the two kernel-argument blocks                [17] total     the size of the whole */
#define RTMI_SCRATCH_REGIONS 18
int rtmi_debug_scratch_regions(const rtmi_frame *f, int64_t out[], int n);
/* Diagnostic (added without a version change): the scheduler step of a scheduled render -- what rtmi_render_ex runs
 * between its first pass and the launch that finishes the frame, the same code -- on the caller's own inputs.  d_scratch:
 * scratch_bytes >= rtmi_render_scratch_bytes(f) of device memory, whose regions receive the plan.  d_ray_counts: device
 * uint32[64 x local tiles], the first pass's count per work item; with pixel_head != 0 the head's pixels get bit 31 set
 * IN PLACE.  d_work_counts (nullable): device uint32 per work item; NULL: the queue follows the tile order, else the
 * quarter tiles are sorted by work + rays and dealt as a snake.  sparse_cap, grid_waves, outlier_x10, head_pct: what a
 * render derives from its grid and rtmi_render_opts.  simds x rounds chains are planned for a frame of spp samples
 * after a first pass of probe_spp (simds * rounds == 0: no chain plan; at most 32768).  Leaves in meta: [0] the largest
 * tile cost; [1] outlier tiles: sparse items -- or, with a pixel head, head entries, [2] [3] the ends of its first two
 * classes; [16] the largest count, [18..19] the counts' sum, [20..22] the classes' sizes before the limits,
 * [24..26] the classes' thresholds as used (0xffffffff: class dropped), [28..30] the scatter cursors.
 * Argument errors are RTMI_ERR_INVALID before any device work.  Asynchronous on `stream`. */
int rtmi_debug_schedule(const rtmi_frame *f, void *d_scratch, size_t scratch_bytes, uint32_t *d_ray_counts,
                        const uint32_t *d_work_counts, int pixel_head, uint32_t sparse_cap, int grid_waves, int outlier_x10,
                        const int32_t head_pct[3], int simds, int rounds, int spp, int probe_spp, void *stream);

/* d_all_tiles holds the tile-major buffers of ranks 0..world_size-1 back to
 * back (what an RCCL gather to the root produces; world_size==1: the buffer
 * rtmi_render wrote).  Writes the row-major float[H*W][3] image the reference
 * keeps in d_image (ray_tracing.cu:84).  Asynchronous on `stream`. */
int rtmi_untile(const rtmi_frame *f, const float *d_all_tiles, float *d_image, void *stream);
/* Same for per-pixel ray counts. */
int rtmi_untile_u32(const rtmi_frame *f, const uint32_t *d_all_counts, uint32_t *d_image_counts, void *stream);

/* The N > 1 exchange, on caller-owned buffers and a caller-owned RCCL communicator (an ncclComm_t passed as
 * void*, rank == frame->rank, size == frame->world_size).  Replaces GatherImageData's MPI_Reduce of full frames on
 * host memory (utils.cu:115-130, 232-238): every rank sends its float[work_items][3] tile buffer to `root` over its
 * direct xGMI link (grouped ncclSend / ncclRecv), the root's d_all_tiles (world_size buffers back to back, what
 * rtmi_untile takes) also receives its own.  world_size 1: a device copy, comm may be NULL.  Asynchronous on
 * `stream`.  RCCL is looked up in the process at run time; librtmi.so does not link against it. */
int rtmi_gather(void *nccl_comm, const rtmi_frame *f, const float *d_tiles, float *d_all_tiles, int root, void *stream);
/* The reference's own decomposition (every rank renders the whole frame with GetWorkload's share of the samples,
 * post_process = 0): ncclReduce(sum) of the tile buffers into `root`, in place; follow with rtmi_untile and
 * rtmi_post_process.  In that split every rank's frame is the whole frame, so the number of ranks is the
 * communicator's, not the frame's: comm NULL means this rank is the only one (root must then be 0 and the call is a
 * no-op); with a communicator, root must be one of its ranks (checked with ncclCommCount). */
int rtmi_reduce_sum(void *nccl_comm, const rtmi_frame *f, float *d_tiles, int root, void *stream);

/* GatherImageData's root-side step on a summed image (utils.cu:126-129):
 * rgb = sqrt(clamp(rgb / spp, 0, 1)), in place over n_pixels*3 floats. */
int rtmi_post_process(float *d_image, int64_t n_pixels, int spp, void *stream);
/* GetWorkload (utils.cu:111-113). */
int rtmi_get_workload(int rank, int world_size, int spp);

/* Device self-test of the arithmetic shortcuts that are justified by exhaustion rather than by
 * argument alone; each is run against the expression it replaces on all 2^32 inputs, on the
 * current device (about a second):
 *  [0] the triangle test's `1.0f / det` (utils.cu:59) computed as hardware reciprocal + one FMA
 *      Newton step when |det| < 2^126: inputs with 2^-126 <= |x| < 2^126 where it differs from the
 *      IEEE quotient -- must be 0, the trace kernels rely on it;
 *  [1] differing inputs outside that range, where the kernels divide (informative, > 0);
 *  [2] CudaRandomFloat(-1, 1) (utils.cuh:22-27) as fma(x, 2^-31, 2^-32) - 1: draws x that differ
 *      from curand_uniform(x) * (1 - -1) + -1 -- must be 0;
 *  [3] CudaRandomFloat(0, 1) as fma(x, 2^-32, 2^-33) -- must be 0;
 *  [4] sqrtf(x) (glm::normalize's sqrt, ray.cu:10; lambertian.cu:25) as reciprocal square root + one FMA correction,
 *      on every binary32 in [2^-100, 2^100) -- must be 0;
 *  [5] the Lambertian sampler's `vec /= l` (lambertian.cu:29) as one correctly rounded reciprocal + two FMA
 *      corrections per coordinate, on 2^32 triples of sampler draws -- must be 0;
 *  [6] the same with one correction only (informative);  [7] unused. */
int rtmi_selftest_arithmetic(unsigned long long mismatches[8]);

/* Per-call scheduling options of rtmi_render_ex.  The reference fixes its launch shape at compile
 * time (dim3(8,8) blocks, utils.cu:158); here the shape and the work-queue order are run-time
 * parameters of ONE call -- no process state is involved.  A zero / negative field keeps the
 * library default.  None of them changes any pixel's value. */
typedef struct rtmi_render_opts {
  int32_t size;              /* sizeof(rtmi_render_opts) of the caller: must match the library's */
  int32_t schedule;          /* -1 default; 0 = tiles in image order; 1 = longest-first when it can pay (a 2-spp
                              * probe on scratch RNG states estimates each tile's cost; pixels are indivisible
                              * serial chains, so starting the expensive ones first shortens the end-of-frame
                              * tail); 2 = always longest-first */
  int32_t blocks_per_cu;     /* 0 default (as many workgroups per CU as fit) */
  int32_t threads_per_block; /* 0 default; a multiple of 64, at most 512 (256 for scenes without meshes) */
  int32_t sparse_stride;     /* 0 default: mesh frames put their outlier PIXELS (found by the probe, anywhere in the
                              * frame) at the head of the queue in three weight classes -- a wave each, two per
                              * wave, one per 16 lanes; > 0 (power of two, 1..64): the outlier TILES instead, taken
                              * by every sparse_stride-th lane only (the scheme before the classes, kept for
                              * comparison) */
  int32_t exclusive;         /* -1 default (1); 1: a wave holding an outlier pixel lets only the lanes its class allows
                              * take new pixels, the remaining lanes only help with that pixel's mesh searches; 0:
                              * they render too */
  int32_t outlier_x10;       /* 0 default (20); with sparse_stride > 0: a tile is an outlier from this many tenths of
                              * the mean tile cost */
  int32_t probe_spp;         /* 0 default: samples per pixel of the scheduler's first look at the frame (see first_pass), 1..64 */
  int32_t head_pct[3];       /* 0 default (80, 55, 30): mesh frames, per cent of the frame's largest probe count from
                              * which a pixel gets a wave to itself / shares one with another / gets one lane in 16 */
  int32_t plan;              /* -1 default (1).  List scenes (no mesh) with a probe behind the launch: 0 = every lane takes its
                              * pixels from the work queue; 1 = when the grid's waves have at most three tiles each, every
                              * wave walks a CHAIN of tiles planned before the launch (tiles dealt to the SIMDs, then to a
                              * SIMD's waves, in snakes over the longest-first order, so that all chains of a SIMD and all
                              * SIMDs cost about the same; needs wave_priority); 2 = chains for any number of tiles */
  int32_t wave_priority;     /* -1 default (16; 4 on frames below 64 spp; none below 8 spp); 0 = the hardware's oldest-wave-first issue order; N (a power of two) = every
                              * N iterations a wave publishes how many queries it still has to do and takes the s_setprio
                              * level its rank among the waves of its SIMD gives it (longest remaining chain first) */
  int32_t lane_stride;       /* 0 default: list scenes, a frame with fewer pixels than the grid has lanes is spread thin, one
                              * pixel per 2 / 4 / 8 / 16 lanes as far as the grid has room; else a power of two, 1..64 */
  int32_t promote_after;     /* -1 default (16); mesh frames: samples after which a pixel's own ray count may promote it to
                              * a head class (its wave then thins out around it); 0 = never */
  int32_t cost_probe;        /* -1 default (1); mesh frames: 1 = the probe books the lane-steps of its mesh searches on the
                              * pixels they serve and the queue's order follows that cost, 0 = it follows the ray counts */
  int32_t first_pass;        /* -1 default (1).  1 = the scheduler's probe is the frame's OWN first samples: samples [0, s1) of
                              * every pixel go into the caller's buffers, their ray counts order / plan the rest, a second
                              * launch resumes every pixel at sample s1 (s1 = probe_spp, or by default spp / 16, at most 64,
                              * for a frame that will be planned, else 2); N > 1 = the same with spp / N; 0 = probe_spp
                              * samples on a scratch copy of the RNG states, discarded */
  int32_t fast_path;         /* 0 default (1, or RTMI_FAST_PATH).  1 = a launch of a list-triangle scene whose run-time modes are all
                              * the common ones (at most 16 materials, the scene's tables staged in LDS, no signed colour, a
                              * power-of-two frame, every lane taking pixels, wave priorities on) uses a kernel compiled for
                              * exactly those modes; -1 = every launch uses the general kernel.  Same pixels either way.
                              * Those kernels cull the world list against bounds that hold the distance slack of every ray
                              * origin within 8 x the list's largest |coordinate| (max norm), so the camera must lie within
                              * that reach (and 9 x that coordinate x 1e30 must be finite in binary32): asked at every launch
                              * of the scene's current camera -- a camera moved beyond the reach by rtmi_camera_update gets
                              * the general kernel from then on, at its rate, and rtmi_render_mode_ex reports fast_path 0. */
  void *d_scratch;           /* optional device memory for ALL per-call state (work-queue cursors, ray total,
                              * completion flag, the scheduler's buffers), owned by the caller, at least */
  size_t scratch_bytes;      /* rtmi_render_scratch_bytes(frame) bytes: with it, concurrent renders of one scene
                              * (several streams, or N shards on one device) share nothing but the read-only scene,
                              * and rtmi_render_status(s, d_scratch, ..) reports on exactly that call.  NULL: the
                              * scene's own, which ties renders of that scene to one at a time. */
} rtmi_render_opts;
/* Bytes of d_scratch a render of this frame / shard needs. */
size_t rtmi_render_scratch_bytes(const rtmi_frame *f);
/* The launch a render of this frame would use on the current device: {workgroups, lanes per workgroup,
 * workgroups per compute unit, compute units}.  workgroups x lanes = the lanes resident at once, each of which
 * holds one pixel at a time (utils.cu:158 fixes dim3(8,8) blocks over the whole frame instead). */
int rtmi_render_launch_shape(const rtmi_scene *s, const rtmi_frame *f, const rtmi_render_opts *opts, int32_t out[4]);
/* How a render of this frame would be scheduled on the current device (what rtmi_render_ex decides before it launches
 * anything): out = {scheduled (1: a first pass orders / plans the rest), samples of the first pass (0: none), 1 if that
 * pass is the frame's own first samples (resumed) and 0 if it is a discarded probe, 1 if the frame is rendered as
 * planned chains (0: from the work queue), wave-priority interval in iterations (0: off), lane stride (1: every lane
 * takes pixels), waves of the grid, tiles of this shard}.  Informational: none of it changes a pixel. */
int rtmi_render_mode(const rtmi_scene *s, const rtmi_frame *f, const rtmi_render_opts *opts, int32_t out[8]);
/* The same report with its later fields: the first min(n, RTMI_MODE_FIELDS) of {the eight of rtmi_render_mode, fast_path
 * (1: the launch that finishes the frame uses a kernel compiled for its modes, see rtmi_render_opts.fast_path; 0: the
 * general kernel)}.  Added without a version change: a caller detects it by the symbol. */
#define RTMI_MODE_FIELDS 9
int rtmi_render_mode_ex(const rtmi_scene *s, const rtmi_frame *f, const rtmi_render_opts *opts, int32_t *out, int n);
/* The rule behind that field, as a pure function (no device, no scene): which trace kernel a launch with these facts
 * gets -- 0 the general one, 1 the fast kernel that draws from the work queue, 2 the fast kernel that walks planned
 * chains.  facts = {fast path enabled, kernel variant (2: list triangles only), materials, material table staged in LDS,
 * pair records staged in LDS and the camera within the list cull's reach (rtmi_render_opts.fast_path), no signed colour, determinants safe, width, height, lane stride, wave priorities on,
 * planned chains, resumes a first pass, has the probe's tile costs}.  Every fast kernel needs: enabled, variant 2, 1..16
 * materials, both tables staged, no signed colour, safe determinants, width and height powers of two up to 2^20, lane
 * stride 1, priorities on; the chain kernel also a resumed pass with tile costs (else such a launch is the general
 * kernel's).  RTMI_ERR_INVALID for a null argument. */
#define RTMI_FAST_PATH_FACTS 14
int rtmi_fast_path_kernel(const int32_t facts[RTMI_FAST_PATH_FACTS]);
/* Which trace kernels a render of this frame would launch, as the compile-time mode words they were built with (csrc/
 * kernels.h: PIN_*): out = {the first pass's (0 also when the frame has none), the finishing launch's}.  0 is the general
 * kernel; 383 draws from the work queue and 255 walks planned chains, as rtmi_fast_path_kernel's 1 and 2; with 512 added
 * (895, 767) it is the same kernel compiled for a scene whose materials are all Lambertians or lights without image
 * textures.  One more material of another kind anywhere in the table, used or not, and the scene keeps 383 / 255.
 * Informational: same pixels either way.  Added without a version change: a caller detects it by the symbol. */
int rtmi_render_pins(const rtmi_scene *s, const rtmi_frame *f, const rtmi_render_opts *opts, uint32_t out[2]);
/* rtmi_render with per-call options (opts == NULL: the defaults). */
int rtmi_render_ex(const rtmi_scene *s, const rtmi_frame *f, const rtmi_render_opts *opts, void *d_states,
                   float *d_tiles, uint32_t *d_ray_counts, void *stream);

/* ------------------------------------------------------------------ query --
 * Batched closest-hit queries on a committed scene: HitableList::Hit (hitable_list.cu:7-25) for rays the
 * caller made, answered by the trace kernels' own closest-hit engine, bit for bit as a render would.
 * Added without a version change: a caller detects it by the symbol rtmi_intersect. */
enum {
  RTMI_HIT_NONE = 0,
  RTMI_HIT_SPHERE = 1,
  RTMI_HIT_TRIANGLE = 2,
  RTMI_HIT_PARALLELOGRAM = 3,
  RTMI_HIT_PARALLELEPIPED = 4,
  RTMI_HIT_MESH = 5,
  RTMI_HIT_SKY = 6
};
typedef struct rtmi_hit {      /* 48 bytes, 16-byte aligned */
  float t;                     /* (float)record.t as Trace uses it (ray_tracing.cu:32); +INFINITY: no hit */
  float u, v;                  /* record.u / record.v where the reference sets them, else 0 (Sky, Face<false>) */
  float normal[3];             /* record.normal (face-oriented for triangles, utils.cu:80); 0 for Sky / no hit */
  int32_t material;            /* material handle; -1: Sky, no hit */
  int32_t kind;                /* RTMI_HIT_* */
  int32_t entry;               /* recording index of the hitable: the n-th successful rtmi_add_* call on the scene,
                                  0-based, every nesting level counted; -1: no hit */
  int32_t element;             /* MESH: index of the face in the array given to rtmi_add_bvh; PARALLELEPIPED: its face
                                  0..5 in the order AddCorner appends them; PARALLELOGRAM: 0/1 = which triangle; else 0 */
  int32_t reserved[2];         /* 0 */
} rtmi_hit;

/* n rays: origins and directions float[n][3] (device).  Answers world->Hit(Ray(o, d), 1e-3, INFINITY, &rec) for
 * each (hitable_list.cu:7-25; Ray normalises d, ray.cu:8-10, so t is along the unit direction), then reports a hit
 * only if t <= t_max[i] (d_t_max nullable = no limit).
 *   - t_max is a FILTER on the closest hit over [1e-3, +inf), not a bound passed into the traversal: the reference's
 *     box tests are not exact in t_to, so Hit(ray, 1e-3, t_max) on a mesh can differ from the filtered answer in
 *     degenerate cases.  The filtered answer is the one that is exact against the reference.
 *   - A ray with a non-finite origin or direction, or a direction that does not normalise to a finite non-zero
 *     vector (a zero direction among them), gets kind RTMI_HIT_NONE; the answers of the other rays do not change.
 *     The kernel decides this: the host never reads the ray arrays.
 *   - d_abandoned (nullable, device, one unsigned long long) is incremented by any abandoned mesh search, as the
 *     render's counter word [2] is; an answer is only exact while it stays 0.
 * Asynchronous on `stream`; the call shares no device state with renders or with other queries on the same scene.
 * RTMI_ERR_INVALID before any HIP call for a null or uncommitted scene, n < 0, or null arrays with n > 0; then also
 * when the current device is not the one the scene was committed on.  n == 0 launches nothing. */
int rtmi_intersect(const rtmi_scene *s, int64_t n, const float *d_origins, const float *d_dirs,
                   const float *d_t_max, rtmi_hit *d_hits, unsigned long long *d_abandoned, void *stream);
/* The diagnostic build (librtmi_check1.so, -DRTMI_CHECK_MARGINS) exports one more entry, declared here only in words
 * because no other build has it:  rtmi_intersect_check_counts(s, n, d_origins, d_dirs, d_t_max, d_hits, d_abandoned,
 * unsigned long long *d_check, stream) -- rtmi_intersect with every query answered a second time without any cull,
 * padded bound or distance slack (meshes: the reference's own tree walk); d_check (nullable, device, two words)
 * += {queries re-done, disagreements}. */

/* Any-hit visibility queries (shadow rays, ambient occlusion): one byte per ray, stopping at the first hit that
 * decides it.  Added without a version change: a caller detects it by the symbol rtmi_occluded.
 *
 * d_occluded[i] = 1 exactly when rtmi_intersect with the same ray and the same t_max reports kind != RTMI_HIT_NONE,
 * i.e. world->Hit(Ray(o, d), 1e-3, INFINITY, &rec) has a hit and (float)rec.t <= t_max[i] (d_t_max nullable = no
 * limit); else 0.  So:
 *   - Sky counts: it answers at t = 1e9, so a world with Sky occludes every ray whose t_max >= 1e9.
 *   - A NaN t_max means clear; t_max < 1e-3 (0, negative) is clear too.
 *   - A bad ray (non-finite origin or direction, or a direction that does not normalise) answers 0 and changes no
 *     other answer, as for rtmi_intersect.
 * Unlike rtmi_intersect, t_max bounds the traversal: every cull prunes by it and a ray stops at its first
 * acceptance.  That is exact except on meshes (quirk g8): the reference's AABB::Hit asks for a crossing of the box's
 * SURFACE inside [t_from, t_to], so a ray that starts inside a box and leaves it beyond t_max does not enter it under
 * the bound, where the unbounded walk does and may find a face nearer than t_max.  A mesh whose search finds faces
 * within t_max that the bounded replay refuses therefore leaves the ray undecided, and such a ray (if nothing else
 * occludes it) is answered again by the unbounded closest-hit engine, then the filter.  (Rays that start inside the
 * meshes' bounds with a t_max of at least 1/20 of their extent, where that is the common case, take the unbounded walk
 * from the start, still stopping at the first hit that decides them.)
 *   - d_counts (nullable, device, two unsigned long long): [0] += abandoned mesh searches (as rtmi_intersect's
 *     d_abandoned; an answer is only exact while it stays 0), [1] += rays answered by that exact fallback.
 * Asynchronous on `stream`; the call shares no device state with renders or with other queries on the same scene.
 * RTMI_ERR_INVALID before any HIP call for a null or uncommitted scene, n < 0, or null arrays with n > 0; then also
 * when the current device is not the one the scene was committed on.  n == 0 launches nothing. */
int rtmi_occluded(const rtmi_scene *s, int64_t n, const float *d_origins, const float *d_dirs, const float *d_t_max,
                  uint8_t *d_occluded, unsigned long long *d_counts, void *stream);
/* The diagnostic build (librtmi_check1.so) also exports, declared here only in words:
 * rtmi_occluded_check_counts(s, n, d_origins, d_dirs, d_t_max, d_occluded, d_counts, unsigned long long *d_check,
 * stream) -- rtmi_occluded with every ray answered a second time by the unculled closest-hit engine from +inf (meshes:
 * the reference's own tree walk), then the filter; d_check (nullable, device, two words) += {rays re-done,
 * disagreements}. */

/* ------------------------------------------------------------------ trace --
 * Path-traced radiance of rays the caller made: Trace(world, Ray(o, d), &state, max_depth) (ray_tracing.cu:12-54),
 * the loop a render runs for every sample, bit for bit as a render runs it -- for panoramic, fisheye or per-texel
 * cameras, light probes, or a re-render of chosen rays with chosen RNG states.  Added without a version change: a
 * caller detects it by the symbol rtmi_trace.
 *
 * d_radiance[i] = Trace(world, Ray(o_i, d_i), &state_i, max_depth), raw: the unprocessed estimate a render keeps for
 * one sample before post-processing (no division, clamp or sqrt).
 *   - Directions: Ray(o, d) normalises d once, as for rtmi_intersect.  A camera ray of RayAt (which normalises too)
 *     is therefore reproduced by handing in the normalised direction.
 *   - n rays: origins and directions float[n][3], d_radiance float[n][3] (device).  n <= 2^31 - 1.
 *   - max_depth in [0, RTMI_MAX_DEPTH], else RTMI_ERR_DEPTH.
 *   - d_states: RTMI_STATE_WORDS planes of uint32[n] (the struct-of-arrays layout of rtmi_states_bytes, with n as the
 *     stride; rtmi_rng_init_n seeds them).  Each state is advanced in place by exactly the draws Trace makes (the
 *     Scatter of Lambertian, Metal and Dielectric), in the reference's order; no camera draws are made.
 *   - d_ray_counts (nullable, uint32[n]): each ray's closest-hit queries (Trace's ray_count), at most max_depth + 1.
 *   - A ray with a non-finite origin or direction, or a direction that does not normalise, is left out as in
 *     rtmi_intersect: radiance 0, count 0, state untouched; no other answer changes.
 *   - d_work (required, device, RTMI_TRACE_WORK_WORDS unsigned long long words, 8-byte aligned): the call's own
 *     device state, reset on `stream` before the launch.  After the call [0] holds the abandoned mesh searches (the
 *     answers are exact only while it is 0, as with rtmi_intersect's d_abandoned) and [1] the closest-hit queries of
 *     all rays.  The rest is the kernel's: its work cursor, and the kernel's argument block (read by scalar loads,
 *     which is why d_work is larger than the counters) -- so the call shares no device state with renders or with
 *     other queries on the scene.  A d_work must not be reused before the call that holds it has finished.
 * Asynchronous on `stream`.  RTMI_ERR_INVALID before any HIP call for a null or uncommitted scene, n < 0, n above
 * 2^31 - 1, or a null array with n > 0 (d_ray_counts excepted); then also when the current device is not the one
 * the scene was committed on.  n == 0 launches nothing and leaves d_work as it is. */
#define RTMI_TRACE_WORK_WORDS 256
int rtmi_trace(const rtmi_scene *s, int64_t n, const float *d_origins, const float *d_dirs, int max_depth,
               void *d_states, float *d_radiance, uint32_t *d_ray_counts, unsigned long long *d_work, void *stream);
/* curand_init(seed, first + i, 0, &state_i) for i in [0, n), into RTMI_STATE_WORDS planes of uint32[n] (the layout
 * rtmi_trace reads): n trace states seeded on the device.  The device's jump tables cover subsequences below 2^40,
 * so first + n > 2^40 is RTMI_ERR_INVALID, as are n < 0, n above 2^31 - 1 and null d_states with n > 0.
 * Asynchronous on `stream`; n == 0 launches nothing. */
int rtmi_rng_init_n(uint64_t seed, uint64_t first, int64_t n, void *d_states, void *stream);

/* ----------------------------------------------------------------- bounce --
 * One iteration of Trace's loop as a call, for a wavefront of paths: between two steps the caller holds every path's
 * vertex -- for a shadow ray to a light (rtmi_occluded), a termination rule of its own, per-bounce outputs.  max_depth
 * calls of rtmi_bounce and one rtmi_path_fold compose bit for bit to rtmi_trace (below).  Added without a version change:
 * a caller detects them by the symbol rtmi_bounce.
 *
 * rtmi_bounce.  Rays d_origins, d_dirs and outputs d_emitted, d_attenuation are float[n][3] (device), n <= 2^31 - 1;
 * d_states is rtmi_trace's layout (RTMI_STATE_WORDS planes of uint32[n]); d_hits (nullable) rtmi_hit[n], 16-byte aligned;
 * d_steps (nullable) uint32[n]; d_work is rtmi_trace's (RTMI_TRACE_WORK_WORDS words, reset on `stream`; afterwards [0]
 * holds the abandoned mesh searches and [1] the paths this call stepped).
 *   - A ray (o, d) means Ray(o, d) as in rtmi_intersect and rtmi_trace: the step normalises d once (ray.cu:8-10).
 *   - A bad ray -- a non-finite origin or direction, or a direction that does not normalise, the zero direction among
 *     them -- is SKIPPED: nothing of the path is written and its state is not read.  So a path that has ended (below) and
 *     an inactive item of rtmi_camera_rays flow through further steps untouched.
 *   - Any other path gets exactly what one iteration of Trace does below its depth test (ray_tracing.cu:22-47):
 *     rec = world->Hit(Ray(o, d), 1e-3, INFINITY); d_hits[i] = the record exactly as rtmi_intersect reports it for (o, d)
 *     with no t_max; d_steps[i] += 1.
 *     Nothing hit: d_emitted[i], d_attenuation[i] and d_dirs[i] become three +0.0f each; origin and state are untouched.
 *     A hit: d_emitted[i] = material->Emit(rec.u, rec.v, hit_point) (Sky's gradient counts; +0.0f for a material that
 *     does not emit); Scatter runs with the path's state, which advances in place by exactly its draws, in the
 *     reference's order.  Where it scatters, d_attenuation[i] = Scatter's attenuation, d_origins[i] = the scattered ray's
 *     origin (the material's p) and d_dirs[i] = THE VECTOR SCATTER HANDS TO RAY'S CONSTRUCTOR: normalize(S + n), normalised
 *     once, for Lambertian; reflected [+ fuzz * r] and the refracted vector as they are for Metal and Dielectric -- so the
 *     next step's one normalisation reproduces Trace's ray exactly (the convention of rtmi_camera_rays' directions).
 *     Where it does not scatter, d_attenuation[i] and d_dirs[i] become three +0.0f and the origin is untouched.
 *   - The step knows no depth: the caller decides how many run.  Trace's last query, at depth == max_depth, only counts
 *     and returns 0; so after max_depth steps of a good ray, rtmi_trace's ray count is d_steps[i] + (d_dirs[i] still
 *     non-zero ? 1 : 0) and its final state is the path's state.  With max_depth == 0 no step is made.
 *   - One difference from rtmi_trace: a scattered ray can itself be bad -- a Lambertian sample that is exactly the reversed
 *     normal, a Metal fuzz vector that cancels the reflection to within the normalisation's underflow.  The next step
 *     skips such a ray (the path counts as alive, with the steps it has); Trace would follow its NaN direction.
 *
 * rtmi_path_fold is Trace's return expression (ray_tracing.cu:50-52).  d_emitted and d_attenuation are stacks
 * float[layers][n][3]: layer k is what step k wrote (the caller passes base + k * n * 3 to step k).  With
 * c = min(d_steps[i], layers):  c == 0: radiance 0.  d_dirs[i] the zero vector (the path ended): r = E[c-1], then for
 * k = c-2 .. 0: r = E[k] + A[k] * r.  Otherwise (the path is alive: Trace would cut it): r = 0, then for k = c-1 .. 0 the
 * same.  Product and sum are each rounded to binary32 on their own, per channel (no fused multiply-add).  Layers >= c are
 * never read, so the caller never clears the stacks.  The fold uses no scene and no d_work.
 *
 * Both are asynchronous on `stream`.  RTMI_ERR_INVALID before any HIP call for a null or uncommitted scene (rtmi_bounce),
 * n < 0, n above 2^31 - 1, a null required array with n > 0 (d_hits and d_steps of rtmi_bounce are the optional ones),
 * layers outside 1..RTMI_MAX_DEPTH; then also (rtmi_bounce) when the current device is not the one the scene was committed
 * on.  n == 0 launches nothing. */
int rtmi_bounce(const rtmi_scene *s, int64_t n, float *d_origins, float *d_dirs, void *d_states, float *d_emitted,
                float *d_attenuation, rtmi_hit *d_hits /* nullable */, uint32_t *d_steps /* nullable */,
                unsigned long long *d_work, void *stream);
int rtmi_path_fold(int64_t n, int layers, const float *d_dirs, const uint32_t *d_steps, const float *d_emitted,
                   const float *d_attenuation, float *d_radiance, void *stream);

/* ------------------------------------------------------------ live paths --
 * Steps over the live paths only.  rtmi_bounce looks at all n paths in every step, although most of a wavefront has ended
 * after a few; rtmi_path_compact makes the list of the paths the next step would step, and rtmi_bounce_list steps the
 * paths of a list, handed to the waves by index.  The list's length stays on the device: nothing here synchronises with
 * the host.  Added without a version change: a caller detects them by the symbol rtmi_bounce_list.
 *
 * A LIST is uint32 path indices d_list with room for n_list of them (the host's bound, n_list <= 2^31 - 1) and a device
 * word d_count; its CANDIDATES are the entries j in [0, min(n_list, d_count ? *d_count : n_list)).  A null d_list is the
 * identity -- candidate j is path j -- and then n_list <= n.  A candidate >= n is no path and is dropped (skipped).
 *
 * rtmi_path_compact.  A path is LIVE exactly when the next step would step it: its ray is not one of rtmi_bounce's bad
 * rays -- finite origin and direction, and a direction that normalises to a finite non-zero vector.  So a path that has
 * ended (a zero direction, -0.0f included), a bad scattered ray (rtmi_bounce's documented difference) and an inactive
 * item of rtmi_camera_rays are not live.
 *   - d_list_out[0 .. c) = the live candidates' path indices IN THE ORDER OF THE CANDIDATES (ascending for a null or an
 *     ascending input; the same list run to run), *d_count_out = c; entries from c on are not written.  d_list_out has
 *     room for n_list entries.  The rays (float[n][3]) are only read.
 *   - d_scratch: rtmi_path_compact_scratch_bytes(n_list) bytes (device, 4-byte aligned): one word per
 *     RTMI_PATH_COMPACT_ITEMS entries.  Three small launches on `stream` -- counts per workgroup, their scan, the
 *     scatter -- in which no workgroup waits for another.
 *   - d_list_out must not be d_list_in and d_count_out must not be d_count_in: the caller ping-pongs two lists.
 *   - n_list == 0 writes *d_count_out = 0 and nothing else.  The call needs no scene.
 * RTMI_ERR_INVALID before any HIP call for n or n_list negative or above 2^31 - 1, a null d_list_in with n_list > n, a
 * null d_origins, d_dirs, d_list_out, d_count_out or d_scratch with n_list > 0, and either aliasing above.
 *
 * rtmi_bounce_list.  rtmi_bounce for the candidates of (d_list, n_list, d_count) only.  EVERY array is indexed by path
 * and has rtmi_bounce's shape with n paths -- the RNG planes keep stride n, a layer of rtmi_path_fold's stacks stays
 * float[n][3] -- so rtmi_path_fold is used unchanged and nothing is gathered or scattered.
 *   - A listed path gets exactly what rtmi_bounce gives it (rays, state, emitted, attenuation, hit record,
 *     d_steps[i] += 1); bad rays are skipped as there.  A path that is not listed keeps every word.
 *   - The entries must be distinct: a path listed twice gets an unspecified result (every access stays in bounds).
 *   - d_work is rtmi_trace's block (RTMI_TRACE_WORK_WORDS words, reset on `stream`); afterwards [0] holds the abandoned
 *     mesh searches and [1] the paths stepped.  n == 0 launches nothing and leaves d_work as it is; n_list == 0 resets
 *     d_work and launches nothing.
 *   - The waves take the list 64 entries at a time by their own number: no work cursor, no atomic in the distribution.
 * Refused as rtmi_bounce refuses, and for n_list negative or above 2^31 - 1 or a null d_list with n_list > n. */
#define RTMI_PATH_COMPACT_ITEMS 1024
size_t rtmi_path_compact_scratch_bytes(int64_t n_list);
int rtmi_path_compact(int64_t n, const float *d_origins, const float *d_dirs, const uint32_t *d_list_in /* nullable */,
                      int64_t n_list, const uint32_t *d_count_in /* nullable */, uint32_t *d_list_out,
                      uint32_t *d_count_out, void *d_scratch, void *stream);
int rtmi_bounce_list(const rtmi_scene *s, int64_t n, const uint32_t *d_list /* nullable */, int64_t n_list,
                     const uint32_t *d_count /* nullable */, float *d_origins, float *d_dirs, void *d_states,
                     float *d_emitted, float *d_attenuation, rtmi_hit *d_hits /* nullable */,
                     uint32_t *d_steps /* nullable */, unsigned long long *d_work, void *stream);

/* ----------------------------------------------------------- path advance --
 * A wavefront render that stays full.  The loop of "camera rays" below renders one sample of every pixel at a time:
 * max_depth steps on a list that drains, a fold, an add, and only then the next camera rays.  rtmi_path_advance finishes
 * the paths that have ended and refills them IN PLACE with their pixel's next camera ray, so every step of the loop
 *     advance(identity list);  compact;  repeat { rtmi_bounce_list(list);  rtmi_path_advance(the same list);
 *                                                 rtmi_path_compact(from that list) }  until the compaction's count is 0
 * runs on a list of paths that all have work.  Added without a version change: a caller detects it by the symbol
 * rtmi_path_advance.  Every other entry is what it was.
 *
 * The call runs after each rtmi_bounce_list of the loop, on that step's list, and once before the first step (on the
 * identity list) to start the paths.  Its arguments travel in a size-checked struct:
 *   - s: committed; only its camera is read, by value at enqueue time as rtmi_camera_rays reads it.  f: the frame, with
 *     post_process == 0;  items = rtmi_frame_work_items(f) is the n of every array, all indexed by work item, tile-major.
 *   - proj (nullable: RTMI_PROJ_CAMERA), d_budget (nullable: f->spp everywhere): as rtmi_camera_rays and
 *     rtmi_render_budget take them.
 *   - (d_list, n_list, d_count): exactly rtmi_bounce_list's candidates.  A null list is the identity (then
 *     n_list <= items); an entry >= items is dropped before anything is addressed with it; the entries are distinct.
 *   - d_origins, d_dirs float[items][3];  d_states the render's layout, RTMI_STATE_WORDS planes of stride items;
 *     d_steps uint32[items]: the arrays rtmi_bounce_list steps.
 *   - d_emitted, d_attenuation float[items][3]: ONE layer, the same one handed to every rtmi_bounce_list of the loop.
 *   - d_emitted_stack, d_attenuation_stack float[max_depth][items][3]: each path's own layers.  Neither read nor written
 *     when max_depth == 0, and may then be null.
 *   - d_cursor uint32[items][2], zeroed by the caller before a render.  Word 0: the low 31 bits k = samples started, bit
 *     31 F = a path is in flight.  Word 1: P = the layers of that path on the stacks.
 *   - d_sum, d_sq (nullable), d_samples, d_ray_counts (nullable): rtmi_render_budget's, and they accumulate as there.
 *   - d_counts (nullable; device, three unsigned long long): [0] += samples finished, [1] += the closest-hit queries of the
 *     finished samples, [2] += camera rays made.  One atomic per wave and counter, after a wave reduction.
 *
 * The rule for candidate q, in binary32 with every operation rounded on its own (no fused multiply-add):
 *   1. PADDING.  rtmi_frame_pixel_of(f, q) < 0: d_dirs[q] becomes three +0.0f; nothing else of the item is read or written.
 *   2. Otherwise b = min(d_budget ? d_budget[q] : spp, spp).
 *   3. PUSH.  If F and d_steps[q] == P + 1 -- the step just made stepped the path -- d_emitted[q] and d_attenuation[q] are
 *      copied to layer P of the stacks, then P += 1.  The copy happens only while P < max_depth, so every access stays in
 *      bounds whatever the caller did to d_steps.
 *   4. LOOP, at most b - k + 1 times (it never waits on memory):
 *      FINISH, if F.  The path is finished when its ray is not live (rtmi_path_compact's predicate) or when
 *      d_steps[q] >= max_depth; if it is not finished, the loop stops: the next step steps it.  Finished, with
 *      c = min(d_steps[q], max_depth):
 *        - radiance x = rtmi_path_fold's rule over the item's layers 0 .. c - 1 and d_dirs[q]: a zero vector is an ended
 *          path, start from E[c-1]; otherwise start from 0;
 *        - queries = 0 for a fresh path (c == 0) whose ray is not live -- rtmi_trace leaves such a ray out --, otherwise
 *          c + (d_dirs[q] is not the zero vector ? 1 : 0);
 *        - rtmi_sample_add's additions of an active item: d_sum[q] += x;  d_sq[q] += x * x (product and sum rounded
 *          separately);  d_samples[q] += 1;  d_ray_counts[q] += queries;
 *        - F is cleared.
 *      REFILL, if not F.  If k < b: the pixel's next camera ray exactly as rtmi_camera_rays makes an active item's -- the
 *      same draws from d_states[q], advanced in place, the same projection rules, a direction normalised once -- is
 *      written to d_origins[q], d_dirs[q];  d_steps[q] = 0, P = 0, k += 1, F is set; and the loop goes round again (a
 *      fisheye ray outside the image circle, and any ray when max_depth == 0, finishes at once and the pixel goes on to
 *      its next sample in the same call).  Otherwise d_dirs[q] becomes three +0.0f and the loop stops: the next compaction
 *      drops the item for good.
 *   5. The cursor is written back.  An item that is not a candidate keeps every word.
 *
 * What follows from the rule:
 *   - After a call every candidate pixel either holds a live in-flight ray or has no samples left and a zero direction,
 *     so *d_count_out == 0 from the following rtmi_path_compact means the render is complete.  The call itself never
 *     synchronises with the host.
 *   - From a zeroed cursor, zeroed d_steps and zeroed d_dirs the loop above is bit for bit
 *     rtmi_render_budget(s, f, d_budget, ...) in sums, second moments, sample counts, ray counts and final states -- a
 *     pixel's samples are one serial chain on one RNG state, and the loop keeps that order per pixel -- and so, from zeroed
 *     accumulators, rtmi_render with post_process = 0.  The one exception is rtmi_bounce's documented bad scattered ray:
 *     it ends the sample as an alive path of c steps, exactly as a fold over rtmi_bounce's steps takes it.
 *   - Between two steps the caller holds every path's vertex (d_hits of the step), at whatever depth each path is.
 *   - An ascending list -- what rtmi_path_compact makes from the identity -- makes the layer reads and writes coalesced.
 *   - Next-event estimation inside this loop is not offered: rtmi_direct_sample takes ONE step number per call and tells
 *     "stepped by this step" from d_steps[i] == step + 1, and here the paths of a list are at different depths.
 *   - Memory per work item beside the render's: 24 (rays) + 4 (steps) + 24 (the layer) + 8 (cursor) + 24 max_depth bytes.
 *
 * Asynchronous on `stream`.  RTMI_ERR_INVALID before any HIP call for a null scene, a bad frame, null args, a wrong
 * args->size or a non-zero args->reserved, a bad projection (as rtmi_camera_rays), post_process != 0, n_list negative or
 * above 2^31 - 1, a null d_list with n_list > items, a null required array with n_list > 0 (d_budget, d_list, d_count,
 * d_sq, d_ray_counts, d_counts, proj are the optional ones; the stacks are required when max_depth > 0), an uncommitted
 * scene; RTMI_ERR_DEPTH for max_depth outside [0, RTMI_MAX_DEPTH]; then RTMI_ERR_INVALID when the current device is not
 * the scene's.  n_list == 0 or items == 0 launches nothing. */
struct rtmi_projection;
typedef struct rtmi_path_advance_args {
  int32_t size;      /* sizeof(rtmi_path_advance_args) of the caller: must match the library's */
  int32_t reserved;  /* 0 */
  const struct rtmi_projection *proj; /* nullable: RTMI_PROJ_CAMERA */
  const uint32_t *d_budget;           /* nullable */
  const uint32_t *d_list;             /* nullable: the identity */
  int64_t n_list;
  const uint32_t *d_count;            /* nullable */
  float *d_origins, *d_dirs;
  void *d_states;
  uint32_t *d_steps;
  const float *d_emitted, *d_attenuation;
  float *d_emitted_stack, *d_attenuation_stack; /* null only with max_depth == 0 */
  uint32_t *d_cursor;
  float *d_sum;
  float *d_sq;                        /* nullable */
  uint32_t *d_samples;
  uint32_t *d_ray_counts;             /* nullable */
  unsigned long long *d_counts;       /* nullable */
} rtmi_path_advance_args;
int rtmi_path_advance(const rtmi_scene *s, const rtmi_frame *f, const rtmi_path_advance_args *args, void *stream);

/* ----------------------------------------------------------------- direct --
 * Next-event estimation for wavefront paths: a light table made at rtmi_scene_commit, one step that samples it, and a fold
 * that knows the extra term.  A loop of rtmi_bounce_list, rtmi_direct_sample, rtmi_occluded and one rtmi_path_fold_direct
 * is a path tracer with direct-light sampling whose expectation is rtmi_trace's: Lambertian::Scatter draws an exactly
 * cosine-distributed direction, so its attenuation = albedo is the BRDF albedo / pi times cosine over pdf, and the light a
 * scattered ray would find on a table light is estimated at the vertex instead and not counted again.  Added without a
 * version change: a caller detects them by the symbol rtmi_direct_sample.  Every other entry is what it was.
 *
 * The light table.  A TABLE LIGHT is a Triangle, a Parallelogram or a face of a Parallelepiped of the world list (nested
 * lists inlined) whose material is a DiffuseLight on a constant texture with three finite, not all zero components, and
 * whose e1 x e2 (in binary64) is finite and non-zero.  Emissive spheres, mesh faces, image-textured lights and Sky are not
 * table lights (emissive spheres become ones with rtmi_scene_light_kinds, below): their light keeps arriving through
 * hits.  DiffuseLight::Emit ignores the side: lights are two-sided.
 * One record per Parallelogram or box face (sampled as p0 + u e1 + v e2) and one per lone Triangle, in the order of the
 * flattened world list:
 *   - p0, e1, e2, n: bit for bit those of the hitable's first triangle as the kernels hold it (p0, p1 - p0, p2 - p0 and
 *     normalize(cross(e1, e2)) in binary32);  emission: the texture's rgb;  material: the handle;
 *   - kind: 0 parallelogram, 1 triangle;  entry, element: as rtmi_hit names a hit on the light (element: the face 0..5 of a
 *     Parallelepiped, else 0);
 *   - area: in binary64 c = e1 x e2 = (e1y e2z - e2y e1z, e1z e2x - e2z e1x, e1x e2y - e2x e1y),
 *     |c| = sqrt((cx cx + cy cy) + cz cz), half of it for a triangle; rounded to binary32;
 *   - cdf: with w_i = area_i * ((|r| + |g|) + |b|) and W = the sum of the w_i in table order, all in binary64 from the
 *     unrounded areas, cdf_j = (float)((w_0 + ... + w_j) / W); the last entry is 1.0f;
 *   - scale: (float)(area_j * W / (w_j * pi)), the area over the selection probability and pi.
 * rtmi_scene_light_count: the table's length (0: none; RTMI_ERR_INVALID for a null or uncommitted scene).
 * rtmi_scene_lights copies the first min(n, count) records into out (RTMI_ERR_INVALID for a null or uncommitted scene,
 * n < 0, or a null out with n > 0).  rtmi_camera_update does not touch the table.
 *
 * rtmi_direct_sample runs after step number `step` (0-based) of rtmi_bounce or rtmi_bounce_list, on that step's outputs.
 * Its candidates are rtmi_bounce_list's: (d_list, n_list, d_count), a null list the identity, entries >= n dropped, the
 * entries distinct.  Every array is indexed by path and has n paths: d_origins, d_dirs (the scattered rays, only read),
 * d_emitted and d_attenuation (layer `step` of the fold's stacks), d_shadow_origins, d_shadow_dirs and d_direct
 * float[n][3]; d_hits rtmi_hit[n], 16-byte aligned; d_steps, d_flags uint32[n]; d_shadow_t_max float[n].
 * d_light_states is RNG state in rtmi_trace's layout (RTMI_STATE_WORDS planes, stride n), seeded by the caller as a stream
 * of its own -- rtmi_rng_init_n with another seed, or first = n.  The paths' own states are never touched: the paths of a
 * loop with this call in it are bit for bit the paths of the loop without it.  (d_light_states may be the path states
 * themselves; the paths then differ from the plain loop's.)  d_flags is zeroed once by the caller; bit 0 of a word means
 * "this path's last vertex sampled the lights", the other bits are kept.
 * Per candidate i, in binary32 with every operation rounded on its own (no fused multiply-add), sums of three as
 * (x + y) + z, IEEE division and sqrt:
 *   - NOT STEPPED by this step (d_steps[i] != step + 1): d_shadow_dirs[i] and d_direct[i] become three +0.0f,
 *     d_shadow_t_max[i] = 0, the flag is cleared; nothing else changes.
 *   - DROP: if the flag is set and the hit is on a table light -- d_hits[i].kind is TRIANGLE, PARALLELOGRAM or
 *     PARALLELEPIPED and d_hits[i].material is the material of some table light -- d_emitted[i] becomes three +0.0f and
 *     d_counts[1] += 1: the vertex before already accounted for that light.
 *   - SAMPLE: if sample != 0, the table is not empty, the path scattered (d_dirs[i] is not the zero vector) and the hit's
 *     material is Lambertian: r0, r1, r2 = CudaRandomFloat(0, 1) from d_light_states in that order (the state advances by
 *     exactly three);  j = the smallest index with r0 <= cdf[j];  for a triangle light with r1 + r2 > 1: r1 = 1 - r1,
 *     r2 = 1 - r2;  q = (p0 + r1 e1) + r2 e2;  x = d_origins[i];  w = q - x;  d2 = (wx wx + wy wy) + wz wz;
 *     dist = sqrt(d2);  wi = w / dist per component;  cs = (Nx wix + Ny wiy) + Nz wiz with N = d_hits[i].normal;
 *     cl = fabs(the same with the light's n).  The sample is valid iff d2 > 0 && cs > 0 && cl > 0 && dist < +inf (a NaN makes
 *     it invalid).  Valid: g = ((cs * cl) / d2) * scale_j;  d_direct[i][c] = (d_attenuation[i][c] * emission_j[c]) * g;  the
 *     shadow ray is (x, wi, dist * 0.999f).  Invalid: d_shadow_dirs[i] and d_direct[i] are three +0.0f, d_shadow_t_max[i] = 0.
 *     Either way the flag is set and d_counts[0] += 1.
 *   - OTHERWISE: d_shadow_dirs[i] and d_direct[i] are three +0.0f, d_shadow_t_max[i] = 0, the flag is cleared, no draw.
 * d_shadow_origins[i] is written with a valid sample only: a zero direction is a bad ray for rtmi_occluded whatever its
 * origin, answered "clear" at no cost, so the caller never masks anything and d_direct of such a path is +0.0f.  A
 * candidate always gets its shadow direction, t_max, d_direct and flag written; a path that is not a candidate keeps every
 * word.  The last step of a loop passes sample = 0: it only drops, as Trace would not have counted the emission one vertex
 * further.  d_counts (nullable, device, two unsigned long long): [0] += paths sampled, [1] += emissions dropped.
 * One lane per candidate, the list taken 64 entries at a time by wave number (no cursor, no atomic in the distribution).
 *
 * rtmi_path_fold_direct is rtmi_path_fold with one change: wherever that fold reads E[k], this one reads
 * T[k] = d_occluded[k][i] ? E[k] : E[k] + D[k], one binary32 addition per channel.  d_direct is a stack float[layers][n][3]
 * (layer k: what rtmi_direct_sample wrote after step k), d_occluded a stack uint8[layers][n] (what rtmi_occluded answered
 * for layer k's shadow rays).  With every D word +0.0f and no E word -0.0f it is rtmi_path_fold bit for bit.
 *
 * Both are asynchronous on `stream`.  RTMI_ERR_INVALID before any HIP call: rtmi_direct_sample for a null or uncommitted
 * scene, n negative or above 2^31 - 1, n_list negative or above 2^31 - 1, a null d_list with n_list > n, a null array
 * (d_list, d_count and d_counts are the optional ones) with n_list > 0, step >= RTMI_MAX_DEPTH; then also when
 * the current device is not the one the scene was committed on.  rtmi_path_fold_direct as rtmi_path_fold, and for a null
 * d_direct or d_occluded with n > 0.  n == 0 or n_list == 0 launches nothing. */
typedef struct rtmi_light {
  float p0[3], e1[3], e2[3], n[3];
  float emission[3];
  float area, cdf, scale;
  int32_t kind;     /* 0 parallelogram, 1 triangle, 2 sphere (rtmi_scene_light_kinds) */
  int32_t entry, element, material;
} rtmi_light;
int64_t rtmi_scene_light_count(const rtmi_scene *s);
int rtmi_scene_lights(const rtmi_scene *s, rtmi_light *out, int64_t n);
int rtmi_direct_sample(const rtmi_scene *s, int64_t n, const uint32_t *d_list /* nullable */, int64_t n_list,
                       const uint32_t *d_count /* nullable */, uint32_t step, int sample, const float *d_origins,
                       const float *d_dirs, const rtmi_hit *d_hits, const uint32_t *d_steps, float *d_emitted,
                       const float *d_attenuation, void *d_light_states, uint32_t *d_flags, float *d_shadow_origins,
                       float *d_shadow_dirs, float *d_shadow_t_max, float *d_direct,
                       unsigned long long *d_counts /* nullable */, void *stream);
int rtmi_path_fold_direct(int64_t n, int layers, const float *d_dirs, const uint32_t *d_steps, const float *d_emitted,
                          const float *d_attenuation, const float *d_direct, const uint8_t *d_occluded, float *d_radiance,
                          void *stream);

/* rtmi_direct_sample_mis.  rtmi_direct_sample with multiple importance sampling: the light a vertex samples and the light
 * its scattered ray then finds are BOTH kept, each weighted by the balance heuristic, instead of the second being dropped.
 * rtmi_direct_sample's estimate albedo * Le * cs * cl / d2 * scale is unbounded where a light lies close to a diffuse
 * surface; the weighted one is at most albedo * Le.  Added without a version change: a caller detects it by the symbol
 * rtmi_direct_sample_mis.  rtmi_direct_sample and every other entry are what they were.
 *
 * The weights.  At a Lambertian vertex the scattered ray has the solid-angle density cs / pi; the light sample has
 * P_j * d2 / (cl * area_j) with P_j the light's selection probability.  scale_j = area_j / (P_j * pi), so with
 * a = cs * cl * scale_j the ratio of the two densities is a : d2 and pi has cancelled:
 *     the light sample's weight is d2 / (a + d2), the scattered ray's is a / (a + d2), and they sum to 1.
 * The weighted light sample albedo * Le * (a / d2) * d2 / (a + d2) = albedo * Le * a / (a + d2).
 *
 * The light of a hit is the table light j with lights[j].entry == hit.entry and, for hit.kind == RTMI_HIT_PARALLELEPIPED,
 * also lights[j].element == hit.element (the first such j); both triangles of a PARALLELOGRAM (element 0 or 1) are the one
 * light.  A hit of any other kind than TRIANGLE, PARALLELOGRAM or PARALLELEPIPED, one with entry < 0 and one whose entry
 * has no table light has no light.  A map from (entry, face) to j is made at rtmi_scene_commit.
 *
 * The arguments travel in a size-checked struct: every array and scalar of rtmi_direct_sample with the same meaning, shape
 * and candidates, and d_carry float[n][4], 16-byte aligned: per path the scattered direction of its last sampling vertex and
 * that vertex's N . d.  The caller allocates it once for a loop and never needs to initialise it: a word is read only from
 * a path whose flag the call before set, which wrote it.
 * Per candidate i, in binary32, every operation rounded on its own, sums of three as (x + y) + z, IEEE division and sqrt, in
 * this order:
 *   - NOT STEPPED: exactly rtmi_direct_sample's rule.  The carry keeps every word.
 *   - WEIGH (in DROP's place): if the flag's bit 0 was set and the hit has a light j: c = d_carry[i];
 *     cl = fabs((n_j.x c.x + n_j.y c.y) + n_j.z c.z);  t = d_hits[i].t;  d2 = t * t;  a = (c.w * cl) * scale_j;
 *     w = (a > 0 && d2 > 0 && a + d2 < +inf) ? a / (a + d2) : +0.0f (a NaN gives +0.0f);
 *     d_emitted[i][ch] = d_emitted[i][ch] * w where w came from the division, three +0.0f otherwise;  d_counts[1] += 1.
 *     A flagged path whose hit has no light keeps its emission bit for bit: an emissive sphere or mesh face that shares a
 *     table light's material is not a table light, and no vertex sampled it.
 *   - SAMPLE: rtmi_direct_sample's condition, draws, j, flip, q, w, d2, dist, wi, cs, cl, validity, shadow ray and t_max.
 *     Valid: a = (cs * cl) * scale_j;  g = a / (a + d2);  d_direct[i][ch] = (d_attenuation[i][ch] * emission_j[ch]) * g.
 *     Valid or not: d_carry[i] = (d.x, d.y, d.z, (N.x d.x + N.y d.y) + N.z d.z) with d = d_dirs[i], the scattered direction as
 *     rtmi_bounce left it, and N = d_hits[i].normal.  The flag is set and d_counts[0] += 1.
 *   - OTHERWISE: as rtmi_direct_sample.  The carry keeps every word.
 * The last step of a loop passes sample = 0 and only weighs.  The path states are never touched, and rtmi_path_fold_direct
 * folds the result unchanged.  For every visible light point the two weights sum to 1, and a Metal or Dielectric vertex
 * clears the flag, so the light it reflects arrives unweighted: the loop's radiance has rtmi_trace's expectation by the
 * argument above.  d_counts[1] counts the emissions weighed.
 *
 * Asynchronous on `stream`.  RTMI_ERR_INVALID before any HIP call: a null scene or args, a wrong args->size, a non-zero
 * args->reserved, every case of rtmi_direct_sample, and a null d_carry or one that is not 16-byte aligned with n_list > 0;
 * then also when the current device is not the scene's.  n == 0 or n_list == 0 launches nothing. */
typedef struct rtmi_direct_sample_mis_args {
  int32_t size;      /* sizeof(rtmi_direct_sample_mis_args) of the caller: must match the library's */
  int32_t reserved;  /* 0 */
  int64_t n;
  const uint32_t *d_list;             /* nullable: the identity */
  int64_t n_list;
  const uint32_t *d_count;            /* nullable */
  uint32_t step;
  int32_t sample;
  const float *d_origins, *d_dirs;
  const rtmi_hit *d_hits;
  const uint32_t *d_steps;
  float *d_emitted;
  const float *d_attenuation;
  void *d_light_states;
  uint32_t *d_flags;
  float *d_shadow_origins, *d_shadow_dirs, *d_shadow_t_max, *d_direct;
  float *d_carry;                     /* float[n][4], 16-byte aligned */
  unsigned long long *d_counts;       /* nullable */
} rtmi_direct_sample_mis_args;
int rtmi_direct_sample_mis(const rtmi_scene *s, const rtmi_direct_sample_mis_args *args, void *stream);

/* rtmi_scene_light_kinds.  Emissive spheres as table lights: a bulb is sampled in the cone it subtends from the vertex,
 * with the balance heuristic in rtmi_direct_sample_mis.  Opt-in, before rtmi_scene_commit; added without a version change:
 * a caller detects it by the symbol rtmi_scene_light_kinds.  A scene that does not opt in gets the table, the kernels and
 * the bits it always got.  kinds is RTMI_LIGHTS_FLAT (1, the default: triangles, parallelograms, box faces) or
 * RTMI_LIGHTS_FLAT | RTMI_LIGHTS_SPHERES (3).  RTMI_ERR_INVALID, with the reason in rtmi_last_error, for a null scene, a
 * committed scene and every other value (0, 2 and unknown bits included).  Host state only, read at commit.
 *
 * The table with kinds == 3: the flat records as ever and in their order, then one record per SPHERE TABLE LIGHT in the
 * order of the flattened scene's spheres: a Sphere of the world list (nested lists inlined) whose material is a
 * DiffuseLight on a constant texture with three finite, not all zero components, whose centre is finite, whose binary64
 * radius r is finite and > 0, and for which R = (float)r and R2 = R * R (binary32) are finite and > 0.  Its record:
 * kind = 2;  p0 = the centre;  e1[0] = R, e1[1] = R2;  e1[2], e2, n = +0.0f;  emission, material;  entry as rtmi_hit names
 * a hit on it, element = 0;  area = (float)(4 pi r r) formed in binary64;  w_j = area_j * ((|r| + |g|) + |b|) from the
 * unrounded area.  W and cdf are formed over the WHOLE table by the expressions above (the last cdf is 1.0f); a flat
 * record keeps its expression for scale with the new W, a sphere has scale_j = (float)(2 * W / w_j) = 2 / P_j.  The light
 * of a SPHERE hit is the table light j of kind 2 with lights[j].entry == hit.entry.  Mesh faces, image-textured lights,
 * Sky and spheres of radius <= 0 stay what they were.
 *
 * The step on a scene whose table holds a sphere light (both rtmi_direct_sample and rtmi_direct_sample_mis; same
 * arguments, same arithmetic rules: one binary32 rounding per operation in the order written, sums of three as
 * (x + y) + z, IEEE division and sqrt, no fused multiply-add, a NaN makes a comparison false).  For a sphere light j and a
 * point x the SHARED GEOMETRY is
 *     wc = c - x;  d2c = (wcx wcx + wcy wcy) + wcz wcz;  outside = d2c > R2;  dc = sqrt(d2c);  s2 = R2 / d2c;
 *     cm = sqrt((d2c - R2) / d2c);  om = s2 / (1 + cm)  -- 1 - cos(theta_max) of the subtended cone, without cancellation:
 *     om comes from s2 for a far light, and d2c - R2 is exact for a vertex close to the surface, where 1 - s2 would
 *     magnify the rounding of s2 (given R2 and d2c, om is within 1.3 ulp of s2 / (1 + sqrt(1 - s2)) in binary64).
 *   - SAMPLE: the condition is unchanged; r0 is drawn and j picked as ever.  lights[j].kind != 2: the rest is the text
 *     above, r1 and r2 included.  kind == 2, with x = d_origins[i], N = d_hits[i].normal:
 *       draws, always and before any validity test: r1 = CudaRandomFloat(0, 1); then repeat a = CudaRandomFloat(-1, 1),
 *         b = CudaRandomFloat(-1, 1) (each draw01 * 2 + (-1)), s = a a + b b until s > 0 && s <= 1 (no trip cap);
 *         ls = sqrt(s), cp = a / ls, sp = b / ls.  The light state advances by 2 + 2 * trips.
 *       polar angle: h = r1 * om;  ct = 1 - h;  st2 = h * (2 - h);  st = sqrt(st2).
 *       axis and frame (Duff et al.): w = wc / dc per component;  sg = wz >= 0 ? 1 : -1;  ka = -1 / (sg + wz);
 *         kb = (wx wy) * ka;  u = (1 + (sg * (wx wx)) * ka, sg * kb, (-sg) * wx);  v = (kb, sg + (wy wy) * ka, -wy).
 *       direction: sc = st * cp;  ss = st * sp;  wi = (ct * w + sc * u) + ss * v per component.
 *       distance: tc = dc * ct;  q = R2 - d2c * st2;  q = q > 0 ? q : 0;  t = tc - sqrt(q).
 *       cosine: cs = (Nx wix + Ny wiy) + Nz wiz.
 *       valid iff outside && cs > 0 && t > 0 && t < +inf.  Valid: a = (cs * om) * scale_j;  g = a for rtmi_direct_sample,
 *         g = a / (a + 1) for rtmi_direct_sample_mis;  d_direct[i][ch] = (d_attenuation[i][ch] * emission_j[ch]) * g;  the
 *         shadow ray is (x, wi, t * 0.999f).  Invalid: the invalid outputs above.  Flag, d_counts[0] and, for MIS, the
 *         carry (d, N . d) as ever, valid or not.
 *     Why: a direction uniform in the cone has density 1 / (2 pi om), so the estimate (albedo / pi) Le cs / (P_j / (2 pi om))
 *     is albedo Le cs om scale_j: no 1 / d2 term, bounded without MIS.  The scattered ray's density cs / pi against the
 *     light's P_j / (2 pi om) is a : 1, so the balance weights are a / (a + 1) and 1 / (a + 1), and pi cancels again.
 *   - WEIGH (rtmi_direct_sample_mis): the flag's bit 0 was set, d_hits[i].kind == RTMI_HIT_SPHERE and the hit has a light j
 *     of kind 2.  x = d_origins[i]: a DiffuseLight does not scatter, so rtmi_bounce left the origin at the vertex before.
 *     !outside: the emission keeps every bit and is not counted -- that vertex could not sample this light.  Otherwise
 *     a = (carry.w * om) * scale_j;  w = (a > 0 && a + 1 < +inf) ? a / (a + 1) : +0.0f;  d_emitted[i] is multiplied by w
 *     where w came from the division and is three +0.0f otherwise;  d_counts[1] += 1.  Hits of other kinds: as ever.
 *   - DROP (rtmi_direct_sample), beside the rule above: the flag was set, the kind is SPHERE, the hit has a light j of kind
 *     2 and `outside` holds from x = d_origins[i]: d_emitted[i] becomes three +0.0f and d_counts[1] += 1.  The material bit
 *     cannot say this: a vertex inside an emissive sphere cannot sample it and must keep the light it hits.
 * rtmi_path_fold_direct, rtmi_occluded and the loop are unchanged. */
#define RTMI_LIGHTS_FLAT    1u   /* triangles, parallelograms, box faces: what the table always held (default) */
#define RTMI_LIGHTS_SPHERES 2u
int rtmi_scene_light_kinds(rtmi_scene *s, uint32_t kinds);

/* rtmi_trace_direct.  rtmi_trace with next-event estimation inside the kernel: the radiance of the loop of rtmi_bounce_list,
 * rtmi_direct_sample_mis, rtmi_occluded_list and the compactions, in ONE launch, a path's vertex, hit record, flag and
 * carry never leaving its lane.  Added without a version change: a caller detects it by the symbol rtmi_trace_direct.  Only
 * the MIS estimator is offered.  rtmi_trace and every other entry are what they were.
 *
 * args: size (sizeof of the caller's struct), reserved (0); n, d_origins, d_dirs, max_depth, d_states, d_radiance,
 * d_ray_counts (nullable) and d_work with rtmi_trace's meaning, shape and layout; d_light_states in d_states' layout
 * (uint32[6][n], stride n): RNG states of their own, as rtmi_direct_sample's; d_counts (nullable): three words that are
 * ADDED to.  d_work[0] holds the abandoned mesh searches, those of shadow queries included; d_work[1] the paths'
 * closest-hit queries (shadow queries are not counted there).
 *
 * The rule, by the entries that define it.  For every good ray i, vertex by vertex, what the loop does to path i:
 *   - vertex k is one rtmi_bounce iteration with rtmi_trace's ray handling (a bad scattered ray is followed as rtmi_trace
 *     follows it, where the step skips it: the one difference);
 *   - then rtmi_direct_sample_mis's rule with step = k, sample = (k + 1 < max_depth), the path the only candidate, its flag
 *     (0 at the start) and carry private to it, the hit the rtmi_hit record rtmi_bounce would write; on a scene that opted
 *     into RTMI_LIGHTS_SPHERES the sphere rules of rtmi_scene_light_kinds (SAMPLE in the cone, WEIGH from outside only);
 *   - then the shadow ray (x, wi, t_max) gets exactly rtmi_occluded's answer: Ray's one normalisation of wi, and
 *     (float)t <= t_max on HitableList::Hit(.., 1e-3, inf); a ray rtmi_occluded leaves out is clear;
 *   - the path state advances as in rtmi_trace; d_light_states[i] advances by exactly the loop's draws (three per flat
 *     sample, 2 + 2 * trips per sphere sample, none at a vertex that does not sample);
 *   - a bad ray is left out: radiance 0, count 0, both states untouched.
 * Radiance.  With the loop's final stacks E (the WEIGHed terminal emission in place), A, D (what SAMPLE wrote per layer),
 * occ (the shadow answers) and c the path's step count:
 *     r_path = rtmi_path_fold(dirs, steps, E, A);
 *     acc = +0.0f, P = (1, 1, 1);  for k = 0 .. c - 1, ascending, per channel, every operation rounded on its own:
 *         V = occ[k] ? +0.0f : D[k];   acc = acc + (P * V);   P = P * A[k];
 *     d_radiance[i] = r_path + acc.
 * A layer whose V is a zero may be skipped (acc began at +0.0f), and with an empty light table the result is rtmi_trace's
 * with -0.0f turned into +0.0f.  The sum runs FORWARD where rtmi_path_fold_direct folds backward: the samples and the
 * estimator are the same -- in exact arithmetic r_path + acc is rtmi_path_fold_direct's value -- and only the rounding
 * order of the sum differs; the forward form needs six registers and no stack of float[layers][n][3].
 * d_ray_counts[i] = rtmi_trace's count (steps + alive);  d_counts[0] += vertices sampled, [1] += emissions weighed,
 * [2] += shadow rays answered occluded: the loop's counts[0], counts[1] and the sum of its occlusion stack.
 *
 * Asynchronous on `stream`.  RTMI_ERR_INVALID before any HIP call: a null scene or args, a wrong args->size, a non-zero
 * args->reserved, every case of rtmi_trace, a null d_light_states with n > 0, and d_light_states == d_states (an aliasing
 * the loop tolerates and one kernel that holds the path state in registers does not); RTMI_ERR_DEPTH for max_depth outside
 * [0, RTMI_MAX_DEPTH]; then RTMI_ERR_INVALID when the current device is not the scene's.  n == 0 launches nothing. */
typedef struct rtmi_trace_direct_args {
  int32_t size;      /* sizeof(rtmi_trace_direct_args) of the caller: must match the library's */
  int32_t reserved;  /* 0 */
  int64_t n;
  const float *d_origins, *d_dirs;
  int32_t max_depth;
  void *d_states;
  void *d_light_states;
  float *d_radiance;                  /* float[n][3] */
  uint32_t *d_ray_counts;             /* nullable */
  unsigned long long *d_counts;       /* nullable: three words, added to */
  unsigned long long *d_work;         /* RTMI_TRACE_WORK_WORDS words */
} rtmi_trace_direct_args;
int rtmi_trace_direct(const rtmi_scene *s, const rtmi_trace_direct_args *args, void *stream);

/* rtmi_path_roulette.  Russian roulette as a wavefront step: the termination rule a loop of rtmi_bounce / rtmi_bounce_list
 * steps may play after each step, with the survivors' compensation written where the folds read it.  Added without a
 * version change: a caller detects it by the symbol rtmi_path_roulette.  The call needs no scene.
 *
 * It runs after step `step` of the loop, on that step's outputs; in a loop with direct sampling after
 * rtmi_direct_sample[_mis] of that step, whose D[k] is formed from the unscaled A[k].  The candidates are
 * rtmi_bounce_list's (d_list, n_list, d_count): a null list is the identity, entries >= n are dropped, entries are distinct.
 * d_states: the PATHS' states in rtmi_trace's layout (uint32[6][n], stride n).  d_attenuation: layer `step` of the fold's
 * stack.  d_throughput: float[n][3] that the caller fills with 1.0f once, before the first call of a loop.
 *
 * The rule per candidate i.  Binary32, every operation rounded on its own, no fused multiply-add, IEEE division; a NaN
 * makes a comparison false.
 *   - d_steps[i] != step + 1 (not stepped), or d_dirs[i] the zero vector, -0.0f included (ended): every word is kept.
 *   - Else, with a = d_attenuation[i], P = d_throughput[i]:
 *       t = P * a per channel;   q = t.x; if (t.y > q) q = t.y; if (t.z > q) q = t.z;
 *       play = step >= first_step && q < 1;
 *     not play: d_throughput[i] = t; no draw, nothing else changes.
 *     play: p = q > p_min ? q : p_min;  u = CudaRandomFloat(0, 1) from the path's own state, which advances by exactly
 *     one draw;  d_counts[0] += 1;
 *       u <= p (survives): inv = 1 / p;  a' = a * inv per channel;  d_attenuation[i] = a';  d_throughput[i] = P * a' per
 *         channel -- not t * inv: the throughput is by construction the forward product of the stack as it now stands;
 *       else (killed): d_attenuation[i], d_dirs[i] and d_throughput[i] become three +0.0f each, and d_counts[1] += 1.
 *   - A path that is not a candidate keeps every word.
 * A killed path is an ended path for everything that exists: rtmi_path_compact drops it, later steps skip it, and
 * rtmi_path_fold and rtmi_path_fold_direct fold it as a path that ended at a vertex emitting E[step], unchanged.  A
 * survivor's continuation is scaled through A[step], so both folds stay correct as they are.
 *
 * The floor p_min.  u lies on a grid of 2^-32 rounded to binary32, so P(u <= p) differs from p by at most 2^-24 absolute
 * (tests/test_roulette_host.py counts the draws): the floor bounds the relative bias of a weight by 2^-24 / p_min, and one
 * compensation factor by 1 / p_min.
 *
 * One lane per candidate, the list taken 64 entries at a time by wave number; no cursor, no atomic in the distribution;
 * each counter by one atomic per wave.  Asynchronous on `stream`.  RTMI_ERR_INVALID before any HIP call: null args, a wrong
 * args->size, a non-zero reserved or reserved2, n or n_list negative or above 2^31 - 1, a null d_list with n_list > n, a null
 * d_steps, d_dirs, d_attenuation, d_states or d_throughput with n_list > 0, step >= RTMI_MAX_DEPTH, p_min not in (0, 1]
 * (NaN included).  n == 0 or n_list == 0 launches nothing. */
typedef struct rtmi_path_roulette_args {
  int32_t size;                      /* sizeof(rtmi_path_roulette_args) of the caller: must match the library's */
  int32_t reserved;                  /* 0 */
  int64_t n;
  const uint32_t *d_list;            /* nullable: the identity */
  int64_t n_list;
  const uint32_t *d_count;           /* nullable */
  uint32_t step;                     /* the step just made, 0-based */
  uint32_t first_step;               /* no roulette at steps below this */
  float p_min;                       /* floor of the survival probability, in (0, 1] */
  int32_t reserved2;                 /* 0 */
  const uint32_t *d_steps;           /* uint32[n] */
  float *d_dirs;                     /* float[n][3]: the scattered rays */
  float *d_attenuation;              /* float[n][3]: layer `step` of the fold's stack */
  void *d_states;                    /* the PATHS' states, rtmi_trace's layout, stride n */
  float *d_throughput;               /* float[n][3]; the caller fills it with 1.0f once */
  unsigned long long *d_counts;      /* nullable, two words, added to */
} rtmi_path_roulette_args;
int rtmi_path_roulette(const rtmi_path_roulette_args *args, void *stream);

/* rtmi_trace_roulette.  rtmi_trace with rtmi_path_roulette's rule played in the lane: what the loop of rtmi_bounce_list,
 * rtmi_path_roulette and rtmi_path_compact does to a path, in ONE launch.  Added without a version change: a caller detects
 * it by the symbol rtmi_trace_roulette.  rtmi_trace and every other entry are what they were.
 *
 * args: size, reserved (0); n, d_origins, d_dirs, max_depth, d_states, d_radiance, d_ray_counts (nullable) and d_work with
 * rtmi_trace's meaning, shape and layout; first_step, p_min as rtmi_path_roulette's; d_counts (nullable): two words that are
 * ADDED to, roulettes played and paths killed.
 *
 * The rule, by the entries that define it.  For every good ray i:
 *   - vertex k is one rtmi_bounce iteration with rtmi_trace's ray handling (a bad scattered ray is followed as rtmi_trace
 *     follows it, where the step skips it: the one difference);
 *   - where vertex k scattered and k + 1 < max_depth, rtmi_path_roulette's rule with step = k, the path the only candidate,
 *     its throughput (1, 1, 1) at the start; at k + 1 == max_depth nothing is played (Trace's last query only counts);
 *   - the state advances by Trace's draws plus one per roulette played;
 *   - d_ray_counts[i] = steps + (alive ? 1 : 0); a killed path is not alive;
 *   - a bad ray is left out: radiance 0, count 0, state untouched.
 * Radiance, summed FORWARD.  With the loop's final stacks E and A' (the survivors' layers scaled) and c the step count:
 *     the path ended by its own hit (not killed, not cut):  P = (1, 1, 1);  P = P * A'[k] for k = 0 .. c - 2, ascending;
 *         d_radiance[i] = E[c - 1] * P  per channel, every operation rounded on its own;
 *     the path was killed or cut, or c == 0:  three +0.0f.
 * E[k] is +0.0f on every layer that scattered (no material both emits and scatters), so in exact arithmetic this is
 * rtmi_path_fold of those stacks; only the rounding order of one product differs, as with rtmi_trace_direct's forward sum.
 * P is the throughput the rule carries anyway: no layer stack is written and no fold runs.
 *
 * Asynchronous on `stream`.  RTMI_ERR_INVALID before any HIP call: a null scene or args, a wrong args->size, a non-zero
 * args->reserved, p_min not in (0, 1] (NaN included), every case of rtmi_trace; RTMI_ERR_DEPTH for max_depth outside
 * [0, RTMI_MAX_DEPTH]; then RTMI_ERR_INVALID when the current device is not the scene's.  n == 0 launches nothing. */
typedef struct rtmi_trace_roulette_args {
  int32_t size;      /* sizeof(rtmi_trace_roulette_args) of the caller: must match the library's */
  int32_t reserved;  /* 0 */
  int64_t n;
  const float *d_origins, *d_dirs;
  int32_t max_depth;
  uint32_t first_step;
  float p_min;
  void *d_states;
  float *d_radiance;                  /* float[n][3] */
  uint32_t *d_ray_counts;             /* nullable */
  unsigned long long *d_counts;       /* nullable: two words, added to */
  unsigned long long *d_work;         /* RTMI_TRACE_WORK_WORDS words */
} rtmi_trace_roulette_args;
int rtmi_trace_roulette(const rtmi_scene *s, const rtmi_trace_roulette_args *args, void *stream);

/* rtmi_occluded_list.  rtmi_occluded for the candidates of (d_list, n_list, d_count) only: the visibility query of a loop
 * whose other steps take a live-path list, and of any caller who shoots shadow or ambient-occlusion rays from the vertices
 * rtmi_bounce_list leaves behind.  Added without a version change: a caller detects it by the symbol rtmi_occluded_list.
 *   - The candidates are exactly rtmi_bounce_list's: the entries j in [0, min(n_list, d_count ? *d_count : n_list)), a null
 *     d_list the identity (then n_list <= n), an entry >= n dropped before anything is addressed with it.  The count word is
 *     read on the device, nothing synchronises with the host, and the grid is sized by n_list, not by n.
 *   - EVERY array is indexed by path and has rtmi_occluded's shape with n paths, n <= 2^31 - 1: d_origins, d_dirs
 *     float[n][3], d_t_max (nullable) float[n], d_occluded uint8[n].
 *   - For a listed path i, d_occluded[i] is exactly the byte rtmi_occluded writes for the ray (o_i, d_i, t_max_i): bad rays
 *     answer 0, a NaN t_max and t_max < 1e-3 are clear, Sky answers at 1e9, and the same two passes decide it (the bounded
 *     pass, the near-box rule, the exact fallback of quirk g8).  A path that is not listed KEEPS ITS BYTE: a caller who wants
 *     "clear" there zeroes the array once.
 *   - Unlike rtmi_bounce_list, the entries need NOT be distinct: the query changes no state, so a path listed twice gets
 *     the same byte twice.
 *   - d_counts (nullable, device, two unsigned long long) is rtmi_occluded's: [0] += abandoned mesh searches, [1] += rays
 *     answered by the fallback; a path listed twice is counted once per occurrence.
 *   - The waves take the list 64 entries at a time by their own number: no work cursor, no atomic in the distribution; a
 *     chunk behind the count or without a path in it costs its wave one test.
 * Asynchronous on `stream`; the call shares no device state with any other call.  RTMI_ERR_INVALID before any HIP call for
 * a null or uncommitted scene, n or n_list negative or above 2^31 - 1, a null d_list with n_list > n, a null d_origins,
 * d_dirs or d_occluded with n > 0 and n_list > 0; then also when the current device is not the one the scene was committed
 * on.  n == 0 or n_list == 0 launches nothing and writes nothing. */
int rtmi_occluded_list(const rtmi_scene *s, int64_t n, const uint32_t *d_list /* nullable */, int64_t n_list,
                       const uint32_t *d_count /* nullable */, const float *d_origins, const float *d_dirs,
                       const float *d_t_max /* nullable */, uint8_t *d_occluded,
                       unsigned long long *d_counts /* nullable */, void *stream);
/* The diagnostic build (librtmi_check1.so) also exports, declared here only in words:
 * rtmi_occluded_list_check_counts(s, n, d_list, n_list, d_count, d_origins, d_dirs, d_t_max, d_occluded, d_counts,
 * unsigned long long *d_check, stream) -- the list form of rtmi_occluded_check_counts: every candidate that is a path is
 * answered a second time by the unculled closest-hit engine from +inf, then the filter; d_check (nullable, device, two
 * words) += {candidates re-done, disagreements}. */

/* ------------------------------------------------------------ camera rays --
 * The render's primary rays as a call of their own, and the fold of a traced sample into the budget buffers.  For every
 * sample index `sample` = 0, 1, ... the three calls
 *     rtmi_camera_rays(s, f, NULL, d_budget, sample, d_states, d_o, d_d, stream);
 *     rtmi_trace(s, items, d_o, d_d, f->max_depth, d_states, d_rad, d_cnt, d_work, stream);
 *     rtmi_sample_add(f, d_budget, sample, d_rad, d_cnt, d_sum, d_sq, d_samples, d_ray_counts, stream);
 * compose bit for bit to rtmi_render_budget(s, f, d_budget, ...) -- sums, second moments, sample and ray counts, RNG
 * states -- and so, from zeroed buffers and a null budget, to rtmi_render with post_process = 0.  Between the first two
 * the caller holds the very rays of the frame's samples: for rtmi_intersect (object ids, world positions, any AOV), for
 * rtmi_occluded (a shadow or AO pass on the primary hits), or to bend them.  With another projection the same loop
 * renders a panoramic or fisheye frame into buffers that rtmi_budget_plan, rtmi_resolve*, rtmi_untile and rtmi_gather
 * take as they are.  Added without a version change: a caller detects them by the symbol rtmi_camera_rays.
 *
 * All buffers are per shard and tile-major over items = rtmi_frame_work_items(f): d_origins, d_dirs, d_radiance, d_sum,
 * d_sq float[items][3]; d_budget, d_trace_counts, d_samples, d_ray_counts uint32[items]; d_states the render's layout,
 * RTMI_STATE_WORDS planes of uint32[items] -- which is rtmi_trace's layout with n = items.
 *
 * Active items (both entries): work item q is active iff it is a pixel of the shard (rtmi_frame_pixel_of >= 0) and
 * sample < min(d_budget ? d_budget[q] : f->spp, f->spp) -- rtmi_render_budget's b = min(d_budget[q], f->spp).
 *
 * rtmi_camera_rays, inactive item: origin and direction are written as six +0.0f; the state is neither read nor
 * written.  A zero direction is a ray rtmi_trace leaves out, so the caller never clears or masks anything.
 * Active item, kind RTMI_PROJ_CAMERA (proj == NULL): exactly what the render kernel does for the next sample of that
 * pixel from d_states --
 *   - r1, then r2, each CudaRandomFloat(0, 1);  xf, yf the binary32 results of ray_tracing.cu:68-73 (yf from H - i);
 *   - target = (llc + xf * horizontal) + yf * vertical;
 *   - a defocus camera: the two lens draws CudaRandomFloat(0, lens_radius), then origin = position + u * ox + v * oy
 *     (camera.cu:63-65,74-77); else origin = position;
 *   - the direction written is normalize(target - origin), normalised ONCE: RayAt's result (camera.cu:69) before Ray's
 *     constructor normalises again -- the direction rtmi_trace and rtmi_intersect document as reproducing a camera ray,
 *     since they apply the second normalisation themselves;
 *   - the state is advanced in place by exactly those 2 or 4 draws.
 * The camera is read from the scene's host record at enqueue time and passed by value, as every render launch does: a
 * call enqueued before an rtmi_camera_update keeps the camera it was enqueued with.
 * The other kinds share r1, r2, xf, yf with CAMERA, make no lens draws, and use the camera's position, llc, horizontal,
 * vertical and its frame u, v, w (the 21 floats of rtmi_camera_get):
 *   - ORTHOGRAPHIC: origin = (llc + xf * horizontal) + yf * vertical, direction = normalize(-w); all binary32.
 *   - EQUIRECT: origin = position.  In binary64 from the binary32 inputs: phi = (xf - 0.5) * 2 pi, theta = (yf - 0.5) * pi,
 *     D = (cos theta * sin phi) * u + sin theta * v - (cos theta * cos phi) * w per component, each rounded once to
 *     binary32, then normalised once in binary32.
 *   - FISHEYE (equidistant): origin = position.  In binary64: sx = 2 xf - 1, sy = 2 yf - 1, r = sqrt(sx sx + sy sy).
 *     r > 1: the direction is three +0.0f -- the item is still active and has made its two draws, so it receives
 *     radiance 0 and counts as a sample: the black surround of the image circle.  r == 0: D = -w.  Otherwise
 *     t = r * fov / 2, D = sin t * (sx / r) * u + sin t * (sy / r) * v - cos t * w; rounded once, normalised once.
 *
 * rtmi_sample_add, active item, with x = d_radiance[q][c]: d_sum[q][c] += x;  d_sq[q][c] += x * x (product and sum each
 * rounded to binary32 on its own, no fused multiply-add);  d_samples[q] += 1;  d_ray_counts[q] += d_trace_counts[q]
 * where both are non-null.  Inactive item: nothing of it is read or written.
 *
 * Both are asynchronous on `stream` and share no device state with any other call.  RTMI_ERR_INVALID before any HIP call
 * for a null scene, a bad frame, a null required array (d_budget, d_trace_counts, d_sq, d_ray_counts are the optional
 * ones), a wrong proj->size, non-zero reserved, a kind outside 0..3, a FISHEYE fov that is not finite or outside
 * (0, 2 pi] (2 pi as binary32), kinds 1..3 on a camera whose u, v, w are not finite and orthonormal (in binary64, each
 * | |x|^2 - 1 | <= 1e-3 and each pairwise |dot| <= 1e-3: a camera installed by rtmi_camera_raw or rtmi_camera_set may
 * carry no frame), an uncommitted scene (rtmi_camera_rays); then also when the current device is not the scene's.
 *
 * rtmi_trace takes n <= 2^31 - 1.  A shard with more work items than that must be traced in slices: every buffer is a
 * plain array, but the state planes keep the stride `items`, so such a caller traces each slice with state copies of
 * its own (stride = the slice's length) and copies them back.  Not enforced here. */
enum { RTMI_PROJ_CAMERA = 0, RTMI_PROJ_ORTHOGRAPHIC = 1, RTMI_PROJ_EQUIRECT = 2, RTMI_PROJ_FISHEYE = 3 };
typedef struct rtmi_projection {
  int32_t size;      /* sizeof(rtmi_projection) of the caller: must match */
  int32_t kind;      /* RTMI_PROJ_* */
  float fov;         /* FISHEYE: full angle of the image circle, radians, finite, 0 < fov <= 2 pi; other kinds: ignored */
  int32_t reserved;  /* 0 */
} rtmi_projection;
int rtmi_camera_rays(const rtmi_scene *s, const rtmi_frame *f, const rtmi_projection *proj /* NULL = CAMERA */,
                     const uint32_t *d_budget /* nullable */, uint32_t sample, void *d_states, float *d_origins,
                     float *d_dirs, void *stream);
int rtmi_sample_add(const rtmi_frame *f, const uint32_t *d_budget /* nullable */, uint32_t sample,
                    const float *d_radiance, const uint32_t *d_trace_counts /* nullable */, float *d_sum,
                    float *d_sq /* nullable */, uint32_t *d_samples, uint32_t *d_ray_counts /* nullable */, void *stream);

/* ----------------------------------------------------------------- budget --
 * A render whose sample count is per pixel, a per-pixel error statistic to decide it from, and the two small kernels
 * that turn them into an adaptive render (plan a pass, render it, ... , resolve).  Added without a version change: a
 * caller detects it by the symbol rtmi_render_budget.  Every entry is per shard (f->rank of f->world_size), on
 * tile-major buffers of rtmi_frame_work_items(f) items, so rtmi_untile, rtmi_untile_u32 and rtmi_gather take them as
 * they are.
 *
 * rtmi_render_budget: for every work item q of the shard that is a pixel (not ragged-tile padding), with
 * b = min(d_budget[q], f->spp):
 *   - renders b more samples of that pixel -- exactly the samples rtmi_render would render next from d_states (the
 *     same jitter and lens draws, the same Trace, in the same order) -- and advances the state in place;
 *   - d_sum[q][c] (float[items][3]): starting from the value it holds, adds each sample's radiance in sample order,
 *     one binary32 addition per sample and channel (what rtmi_render with post_process = 0 does from zero);
 *   - d_sq[q][c] (nullable, float[items][3]): likewise adds x * x of each sample's channel value x, the product and
 *     the sum each rounded to binary32 on its own (no fused multiply-add);
 *   - d_samples[q] += b;  d_ray_counts[q] (nullable) += the closest-hit queries of those samples.  Both are uint32 and
 *     wrap modulo 2^32 over many calls.
 *   - b == 0 and padding items: nothing of the item is read or written, its state included.
 * All four buffers ACCUMULATE: the caller zeroes them once.  f->spp is the cap on ONE call's samples per pixel (it
 * keeps spp x (max_depth + 1) <= RTMI_MAX_PIXEL_QUERIES meaningful without the host reading d_budget); f->post_process
 * must be 0 (RTMI_ERR_INVALID): a uniform division has no meaning here, rtmi_resolve divides.  d_work (required,
 * RTMI_BUDGET_WORK_WORDS unsigned long long words, 8-byte aligned) is the call's own device state exactly as
 * rtmi_trace's: reset on `stream` before the launch; afterwards [0] holds the abandoned mesh searches (the results are
 * exact only while it is 0) and [1] the closest-hit queries of THIS call; the rest is the kernel's (work cursor,
 * argument block).  The call shares no device state with renders or queries on the scene; a d_work must not be reused
 * before the call that holds it has finished.  Work is handed out from a plain queue in image order: a pixel is a
 * serial chain, so a call lasts at least as long as its largest budget x that pixel's queries per sample.
 * Asynchronous on `stream`.  Before any HIP call: RTMI_ERR_INVALID for a null scene, a bad frame, a null array
 * (d_sq, d_ray_counts excepted), an uncommitted scene, post_process != 0; RTMI_ERR_DEPTH for max_depth outside
 * [0, RTMI_MAX_DEPTH]; then RTMI_ERR_INVALID when the current device is not the scene's. */
#define RTMI_BUDGET_WORK_WORDS RTMI_TRACE_WORK_WORDS
int rtmi_render_budget(const rtmi_scene *s, const rtmi_frame *f, const uint32_t *d_budget, void *d_states,
                       float *d_sum, float *d_sq, uint32_t *d_samples, uint32_t *d_ray_counts,
                       unsigned long long *d_work, void *stream);

typedef struct rtmi_adaptive_opts {
  int32_t size;        /* sizeof(rtmi_adaptive_opts) of the caller: must match the library's */
  int32_t min_samples; /* >= 2 */
  int32_t max_samples; /* >= min_samples */
  int32_t step;        /* >= 1: samples a pixel that has not converged gets per pass */
  float tolerance;     /* > 0: relative standard error of the pixel mean at which it stops */
  float floor;         /* >= 0: radiance below which the error is taken as absolute (dark pixels) */
} rtmi_adaptive_opts;
/* The next pass's budget of every work item, from what rtmi_render_budget accumulated.  With n = d_samples[q]:
 *   padding -> 0;  n < min_samples -> min_samples - n;  n >= max_samples -> 0;  otherwise the pixel has converged iff
 * for EVERY channel, with S = d_sum[q][c], Q = d_sq[q][c], nf = (float)n (round to nearest), T = tolerance, F = floor,
 * in binary32 with every operation rounded on its own (no fused multiply-add), evaluated exactly as written:
 *     a = nf * Q;  b = S * S;  c = a - b;  d = nf - 1.0f;  lhs = c / d;
 *     e = T * T;   g = nf * nf;  h = F * F;  i = g * h;  j = b + i;  rhs = e * j;
 *     lhs <= rhs          (false when either side is a NaN: such a pixel has not converged)
 * i.e. "unbiased sample variance / n <= T^2 (mean^2 + F^2)" multiplied through by n^2.  Converged -> 0, else
 * min(step, max_samples - n).  d_totals (two unsigned long long) is OVERWRITTEN on the stream: [0] = items with a
 * budget > 0, [1] = the sum of the budgets; a pass is needed while [0] != 0.
 * Raw second moments lose digits to cancellation when n is large and the variance small.  The rule is first met at the
 * smallest n that satisfies it, where the sums are short; a pixel that has met it gets no more samples, so the loss
 * cannot stop a pixel early that the exact statistic would have kept, only (harmlessly) make a stopped pixel look more
 * converged had it gone on.
 * Asynchronous on `stream`; RTMI_ERR_INVALID before any HIP call for a bad frame, a null array, null opts, a wrong
 * size, min_samples < 2, max_samples < min_samples, step < 1, a tolerance that is not a finite number > 0, a floor
 * that is not a finite number >= 0. */
int rtmi_budget_plan(const rtmi_frame *f, const rtmi_adaptive_opts *o, const float *d_sum, const float *d_sq,
                     const uint32_t *d_samples, uint32_t *d_budget, unsigned long long *d_totals, void *stream);
/* d_tiles[q][c] = d_sum[q][c] / (float)d_samples[q] (0 where d_samples[q] == 0 and for padding), then with post_process
 * != 0 sqrt(clamp(., 0, 1)) by the render's own expressions: for a uniform sample count the result is bit for bit
 * rtmi_render's post-processed tile buffer.  Tile-major, float[items][3].  Asynchronous on `stream`. */
int rtmi_resolve(const rtmi_frame *f, const float *d_sum, const uint32_t *d_samples, int post_process, float *d_tiles,
                 void *stream);

/* --------------------------------------------------------------- features --
 * First-hit feature buffers for a denoiser or compositor: albedo, normal, depth and coverage of the primary hit,
 * summed over THE VERY SAMPLES that made the pixel's colour (their camera rays are made inside the kernel from the
 * pixel's RNG stream; a caller who wants more of those rays than these four buffers renders the frame by the three-call
 * loop of "camera rays" above instead, whose rtmi_camera_rays hands out each sample's rays for rtmi_intersect or
 * rtmi_occluded before rtmi_trace follows them).  Added without a version change: a caller detects it by the symbol
 * rtmi_render_features.
 *
 * rtmi_render_features is rtmi_render_budget in every respect stated above -- which samples are rendered and the order
 * of the additions; what padding and budget-0 items leave alone (everything, the feature buffers included); the cap
 * f->spp; d_work and its layout; the errors.  On top of that, for each rendered sample, with rec the HitRecord of the
 * sample's primary query world->Hit(camera_ray, 1e-3, INFINITY, &rec) (the first closest-hit query Trace makes for it):
 *   - no hit: nothing is added to any feature buffer;
 *   - Sky: d_albedo[q] += Sky's Emit(p), the value Trace returns for that sample (sky.cu:9-14); normal, depth and
 *     coverage get nothing -- the background is not a surface;
 *   - any other hitable: d_coverage[q] += 1;  d_depth[q] += (float)rec.t (what rtmi_hit.t reports);  d_normal[q] +=
 *     rec.normal (what rtmi_hit.normal reports: oriented against the ray for triangles, parallelograms and mesh faces,
 *     outward for spheres);  d_albedo[q] += the material's own colour at the hit -- Lambertian: its texture's
 *     Value(u, v, p), the attenuation Scatter would set (an image texture: the texel / 255); Metal: its albedo;
 *     Dielectric: its colour; DiffuseLight: Emit(u, v, p).  No RNG draw is made for any of this and none is skipped.
 * Every addition is one binary32 addition per sample and channel, in sample order, starting from the value the buffer
 * holds: all four buffers ACCUMULATE over calls like d_sum (the caller zeroes them once); d_coverage wraps modulo 2^32.
 * Each pointer of *feat is nullable.  feat == NULL, or all four null, IS rtmi_render_budget; with any of them non-null
 * the other outputs -- d_sum, d_sq, d_samples, d_ray_counts, the states, d_work[0] and d_work[1] -- are bit for bit what
 * rtmi_render_budget would have written.
 * Errors, before any HIP call, besides rtmi_render_budget's: RTMI_ERR_INVALID for feat->size != sizeof(rtmi_features) or
 * feat->reserved != 0; RTMI_ERR_DEPTH for max_depth == 0 with any feature buffer non-null -- at depth 0 Trace returns
 * before it ever looks at the primary record (ray_tracing.cu:23), so there is no first hit to describe. */
typedef struct rtmi_features {
  int32_t size;          /* sizeof(rtmi_features) of the caller: must match the library's */
  int32_t reserved;      /* 0 */
  float *d_albedo;       /* nullable, float[items][3] */
  float *d_normal;       /* nullable, float[items][3] */
  float *d_depth;        /* nullable, float[items]    */
  uint32_t *d_coverage;  /* nullable, uint32[items]; as rtmi_resolve_features' OUTPUT: the bits of a float (below) */
} rtmi_features;
int rtmi_render_features(const rtmi_scene *s, const rtmi_frame *f, const uint32_t *d_budget, void *d_states,
                         float *d_sum, float *d_sq, uint32_t *d_samples, uint32_t *d_ray_counts,
                         const rtmi_features *feat, unsigned long long *d_work, void *stream);
/* Per-pixel means of the feature sums, in binary32 with every operation rounded on its own.  With n = d_samples[q],
 * nf = (float)n, c = sums->d_coverage[q]:
 *     out->d_albedo[q]   = sums->d_albedo[q] / nf              (per channel)
 *     out->d_normal[q]   = sums->d_normal[q] / nf              (the MEAN normal: NOT renormalised, so its length says
 *                                                               how much the samples' normals agree)
 *     out->d_depth[q]    = c ? sums->d_depth[q] / (float)c : 0 (the mean over the samples that hit a surface)
 *     out->d_coverage[q] = the BITS OF THE FLOAT (float)c / nf, the alpha -- declared uint32_t * only so that one
 *                          struct serves both calls; read it as float
 * Everything is 0 where n == 0 and for padding.  A null pointer in *out skips that buffer.  RTMI_ERR_INVALID before
 * any HIP call for a bad frame, a null sums, out or d_samples, a wrong size or non-zero reserved in either struct, and
 * for a non-null out buffer whose sums twin is null (out->d_depth and out->d_coverage both need sums->d_coverage).
 * All buffers are tile-major per shard, float[items][3] or 32-bit [items]: rtmi_untile takes the two 3-channel ones as
 * they are, rtmi_untile_u32 takes depth and alpha by their bits, rtmi_gather moves the 3-channel ones.
 * Asynchronous on `stream`. */
int rtmi_resolve_features(const rtmi_frame *f, const rtmi_features *sums, const uint32_t *d_samples,
                          const rtmi_features *out, void *stream);

/* ---------------------------------------------------------- render direct --
 * rtmi_render_direct.  rtmi_render_budget / rtmi_render_features whose every sample is traced with next-event estimation
 * inside the kernel (rtmi_trace_direct's estimator): per-pixel budgets in; sums, second moments, sample and ray counts
 * and the optional first-hit features out, in ONE launch, so that rtmi_budget_plan, rtmi_resolve, rtmi_resolve_variance,
 * rtmi_resolve_features, rtmi_denoise and rtmi_accumulate follow unchanged.  Added without a version change: a caller
 * detects it by the symbol rtmi_render_direct.  rtmi_render_budget, rtmi_render_features and every other entry are what
 * they were.
 *
 * args: size (sizeof of the caller's struct), reserved (0); d_budget, d_states, d_sum, d_sq (nullable), d_samples,
 * d_ray_counts (nullable) with rtmi_render_budget's meaning, nullability and accumulation; d_light_states in d_states'
 * layout (uint32[6][items], stride items = rtmi_frame_work_items(f)): RNG states of their own, as rtmi_trace_direct's,
 * carried across calls; features (nullable) with rtmi_render_features' meaning; d_counts (nullable): three words that are
 * ADDED to; d_work (RTMI_BUDGET_WORK_WORDS words): afterwards [0] holds the abandoned mesh searches, those of shadow
 * queries included, [1] the paths' closest-hit queries (shadow queries are not counted there).
 *
 * The rule, by the entries that define it.  For every work item q of the shard that is a pixel, with
 * b = min(d_budget[q], f->spp), and for sample index k = 0 .. b - 1 in order:
 *   - the ray is the one rtmi_camera_rays (kind RTMI_PROJ_CAMERA) makes for the item's next sample from d_states[q]: the
 *     same jitter and lens draws, the direction normalised once;
 *   - the radiance x, both state advances, the query count and the three counters are rtmi_trace_direct's for that one ray,
 *     with d_states[q] and d_light_states[q] as the path's two streams: x = r_path + acc, ONE binary32 addition per channel;
 *   - the fold is rtmi_sample_add's: d_sum[q][c] += x, d_sq[q][c] += x * x (the product and the sum each rounded on its
 *     own, no fused multiply-add), d_samples[q] += 1, d_ray_counts[q] += the path's closest-hit queries (a shadow query
 *     is not counted);
 *   - with features, the feature sums are rtmi_render_features' for those same samples: a shadow query is not a primary
 *     hit, and the primary hits do not depend on direct light.
 * An item with b == 0, and a padding item: nothing of it is read or written, its light state included.  With an empty
 * light table no light state moves and the sums are rtmi_render_budget's for buffers that hold no -0.0f (a sample's -0.0f
 * is added as +0.0f).
 * So the call is bit for bit the loop "for k: rtmi_camera_rays, rtmi_trace_direct, rtmi_sample_add" on the same buffers,
 * without the rays, radiances and counts crossing memory and without the host knowing the largest budget.
 *
 * Asynchronous on `stream`.  RTMI_ERR_INVALID before any HIP call: a null scene or args, a wrong args->size, a non-zero
 * args->reserved, every case of rtmi_render_budget and rtmi_render_features, a null d_light_states (with items > 0), and
 * d_light_states == d_states; RTMI_ERR_DEPTH for max_depth outside [0, RTMI_MAX_DEPTH] (and for max_depth == 0 with a
 * feature buffer); then RTMI_ERR_INVALID when the current device is not the scene's. */
typedef struct rtmi_render_direct_args {
  int32_t size;      /* sizeof(rtmi_render_direct_args) of the caller: must match the library's */
  int32_t reserved;  /* 0 */
  const uint32_t *d_budget;           /* uint32[items] */
  void *d_states;
  void *d_light_states;
  float *d_sum;                       /* float[items][3]; accumulates */
  float *d_sq;                        /* nullable; accumulates */
  uint32_t *d_samples;                /* uint32[items]; accumulates */
  uint32_t *d_ray_counts;             /* nullable; accumulates */
  const rtmi_features *features;      /* nullable */
  unsigned long long *d_counts;       /* nullable: three words, added to */
  unsigned long long *d_work;         /* RTMI_BUDGET_WORK_WORDS words */
} rtmi_render_direct_args;
int rtmi_render_direct(const rtmi_scene *s, const rtmi_frame *f, const rtmi_render_direct_args *args, void *stream);

/* ---------------------------------------------------------------- denoise --
 * A variance- and feature-guided a-trous filter (edge-avoiding wavelets) for frames of a few samples per pixel, on what
 * rtmi_render_budget and rtmi_render_features leave behind.  Added without a version change: a caller detects it by the
 * symbol rtmi_denoise.  The filter is stated operation by operation in binary32, like rtmi_budget_plan: every + - * / is
 * one operation rounded on its own (no fused multiply-add), sums of three are (x + y) + z, and fmax / fmin are IEEE
 * maxNum / minNum (fmaxf).
 *
 * rtmi_resolve_variance: the variance OF THE MEAN of every work item, tile-major like rtmi_resolve, float[items][3].
 * With n = d_samples[q], nf = (float)n, S = d_sum[q][c], Q = d_sq[q][c]:
 *     padding, n == 0:  0
 *     n == 1:           S * S                      (the sample's own square: an error of 100 %)
 *     n >= 2:           a = nf * Q;  b = S * S;  c = fmax(a - b, 0);  d = nf * nf;  e = nf - 1;  c / (d * e)
 * Asynchronous on `stream`; the argument checks are rtmi_resolve's (a bad frame, a null array). */
int rtmi_resolve_variance(const rtmi_frame *f, const float *d_sum, const float *d_sq, const uint32_t *d_samples,
                          float *d_var, void *stream);

/* rtmi_denoise works on ROW-MAJOR buffers of the whole frame, float[H*W][3] or float[H*W] -- what rtmi_untile and
 * rtmi_untile_u32 write: a stencil needs neighbours, which the tile-major shard buffers do not give.
 *
 * Start:  with demodulate, per channel ad = fmax(albedo, 0.01f), C = color / ad, V = variance / (ad * ad); else C = color,
 * V = variance.  Then pass k = 0 .. iterations - 1 with step s = 2^k, for every pixel p = (i, j): the taps are
 * q = (i + dy s, j + dx s), dy the outer loop from -2 to 2, dx the inner one, the centre included, taps outside the image
 * skipped.  With h = {1/16, 1/4, 3/8, 1/4, 1/16} and falloff(x) = { m = fmax(1 - 0.25f * x, 0); m2 = m * m; m2 * m2 }:
 *     surface:  sp = alpha_p > 0, sq = alpha_q > 0; sp != sq: the tap is skipped; neither: wn = wz = 1; both:
 *       d  = fmax((nx_p nx_q + ny_p ny_q) + nz_p nz_q, 0);  wn = d squared normal_squarings times;
 *       xz = fabs(z_p - z_q) / (sigma_depth * z_p + 1e-6f);  wz = falloff(xz);
 *     colour:   dr, dg, db = C_p - C_q;  d2 = (dr dr + dg dg) + db db;
 *       vs = ((Vr_p + Vg_p) + Vb_p) + ((Vr_q + Vg_q) + Vb_q);
 *       xc = d2 / ((sigma_color * sigma_color) * vs + 1e-10f);  wc = falloff(xc);
 *     w = (((h[dy] * h[dx]) * wn) * wz) * wc;
 *     in tap order:  sw += w;  per channel  sc += w * C_q;  sv += (w * w) * V_q;
 *     sw >= 0x1p-32f:  C'_p = sc / sw,  V'_p = sv / (sw * sw);  otherwise C'_p = C_p, V'_p = V_p.
 * The threshold keeps the pass inside the normal numbers: with normal squarings the centre tap's own weight is
 * |N_p|^(2^(squarings+1)), tiny at any partly covered or crease pixel, and a subnormal sw or an underflowing sw * sw would
 * make V' infinite or NaN out of finite inputs.  From 2^-32 on, sw * sw >= 2^-64 and the largest tap's w * w >= 2^-64 / 625
 * are normal, and what a flushed w * w loses is below 2^-50 of the largest term.  A pixel that weighs so little keeps its
 * value, exactly as one whose weights are all 0.
 * Pass k + 1 reads C' and V'; the guides never change.  After the last pass d_out = demodulate ? C * ad : C and, where
 * d_out_variance is not null, d_out_variance = demodulate ? V * (ad * ad) : V.
 * So a pixel is averaged only with pixels on the same side of a coverage, normal or depth edge, and over a colour range of
 * about sigma_color standard errors of the two pixels: the filter blurs the noise the variance reports and little else;
 * d_out_variance is what is left of it (the weights taken as constants).  A non-finite input leaves the pixels whose
 * footprint reaches it unspecified; it does not fault.
 *
 * Defaults (what rtmi.denoise of the Python binding passes): 5 iterations, sigma_color 1, sigma_depth 0.05, 0 normal
 * squarings, demodulate where an albedo is given.  The mean normal's length is the pixel's coverage, so a power p of the
 * cosine weighs a fully covered neighbour (1 / alpha_p)^p times the partly covered pixel itself: squarings sharpen
 * creases inside a surface and eat its silhouette.  sigma_color 1 averages what lies within about one standard error.
 *
 * All per-call state -- the ping-pong images and the packed guide records -- lives in d_scratch
 * (rtmi_denoise_scratch_bytes(height, width) bytes, any alignment): the call shares no device state with any other.  d_out
 * may be exactly d_color; no other overlap between inputs, outputs and scratch is allowed.  Asynchronous on `stream`.
 * RTMI_ERR_INVALID before any HIP call for: height or width outside 1..RTMI_MAX_EXTENT; a null o, g, d_color, d_out or
 * d_scratch; a wrong size in either struct or reserved != 0; an option outside its range; a null required guide;
 * scratch_bytes too small.  rtmi_denoise_scratch_bytes returns 0 for an extent outside 1..RTMI_MAX_EXTENT. */
typedef struct rtmi_denoise_opts {
  int32_t size;             /* sizeof(rtmi_denoise_opts) of the caller: must match the library's */
  int32_t iterations;       /* 1..8; pass k (0-based) uses step s = 2^k pixels */
  int32_t normal_squarings; /* 0..8: the normal weight is squared this many times */
  int32_t demodulate;       /* 0/1: filter colour / albedo, multiply back at the end (needs d_albedo) */
  float sigma_color;        /* finite, > 0 */
  float sigma_depth;        /* finite, > 0 */
} rtmi_denoise_opts;
typedef struct rtmi_denoise_guides { /* row-major, whole frame */
  int32_t size;            /* sizeof(rtmi_denoise_guides) of the caller: must match the library's */
  int32_t reserved;        /* 0 */
  const float *d_variance; /* required, float[H*W][3]: rtmi_resolve_variance's */
  const float *d_albedo;   /* float[H*W][3]; required iff demodulate, else nullable and unused */
  const float *d_normal;   /* required, float[H*W][3]: the MEAN normal of rtmi_resolve_features */
  const float *d_depth;    /* required, float[H*W] */
  const float *d_alpha;    /* required, float[H*W]: rtmi_resolve_features' coverage read as float */
} rtmi_denoise_guides;
size_t rtmi_denoise_scratch_bytes(int height, int width);
int rtmi_denoise(int height, int width, const rtmi_denoise_opts *o, const float *d_color, const rtmi_denoise_guides *g,
                 float *d_out, float *d_out_variance /* nullable */, void *d_scratch, size_t scratch_bytes, void *stream);

/* ------------------------------------------------------------- accumulate --
 * Temporal accumulation for a camera that moves through a static scene: the frame is blended with the previous frames'
 * result wherever the same surface point is still visible.  Added without a version change: a caller detects it by the
 * symbol rtmi_accumulate.  Buffers are rtmi_denoise's: ROW-MAJOR, whole frame; d_color and g->d_variance float[H*W][3],
 * g->d_normal the MEAN normal, g->d_depth and g->d_alpha float[H*W]; g->d_albedo is not looked at.  The cameras are the 21
 * floats of rtmi_camera_get: indices 0..2 the position p, 3..5 llc, 6..8 h, 9..11 v; the rest is unused.
 *
 * The caller owns two histories of rtmi_history_bytes(height, width) = 48 * H * W bytes, 16-byte aligned, and swaps them
 * every frame: the call reads d_history_in (written by the previous frame's call, seen from prev_camera) and writes
 * d_history_out.  Both d_history_in and prev_camera null: the first frame.  A history is opaque, and valid only for the
 * extent it was written with.  d_out may be d_color and d_out_variance may be g->d_variance; d_history_out may overlap
 * nothing.  Asynchronous on `stream`; the call shares no device state with any other.
 *
 * The rule is stated operation by operation like rtmi_denoise's: every + - * / and sqrt is one operation rounded on its
 * own (no fused multiply-add), sums of three are (x + y) + z, fmax is maxNum.
 * Host, in binary64 from the cameras' binary32 values.  This frame's camera: e = (float)(llc - p) per component.  The
 * previous one: a = h', b = v', c = llc' - p';  bc = b x c, ca = c x a, ab = a x b with
 * x x y = (x1 y2 - x2 y1, x2 y0 - x0 y2, x0 y1 - x1 y0);  det = (a0 bc0 + a1 bc1) + a2 bc2;  R0 = (float)(bc / det),
 * R1 = (float)(ca / det), R2 = (float)(ab / det) per component.
 * Device, binary32, pixel (i, j) with inputs C_p, V_p, N_p, z_p and surface_p = alpha_p > 0.  FRESH means C' = C_p,
 * V' = V_p, L' = 1.  A pixel is fresh when there is no history or when !surface_p (the background has no point to
 * reproject).  Otherwise:
 *     xf = ((float)j + 0.5f) / (float)W;   yf = ((float)(H - i) + 0.5f) / (float)H      (the render's pixel centre, quirk g1)
 *     D = (e + xf * h) + yf * v;   l = sqrt((Dx Dx + Dy Dy) + Dz Dz);   P = p + (D / l) * z_p        per component
 *     d = P - p';   alpha = (R0x dx + R0y dy) + R0z dz;  beta, gamma likewise with R1, R2;
 *     ze = sqrt((dx dx + dy dy) + dz dz)
 *     !(gamma > 0): fresh.   fx = (alpha / gamma) * (float)W - 0.5f;   fy = ((float)H + 0.5f) - (beta / gamma) * (float)H
 *     !(fx > -1 && fx < (float)W && fy > -1 && fy < (float)H): fresh          (a NaN is fresh too)
 *     rx = rint(fx), ry = rint(fy) (ties to even);  fabs(fx - rx) <= 1/64 && fabs(fy - ry) <= 1/64:  fx = rx, fy = ry
 *     j0 = floor(fx), i0 = floor(fy);  tx = fx - (float)j0,  ty = fy - (float)i0
 *     taps q = (i0 + di, j0 + dj), di the outer loop 0..1, dj the inner; a tap outside the image is skipped
 *       b = (di ? ty : 1 - ty) * (dj ? tx : 1 - tx)
 *       taken iff  surface_q  &&  (nx_p nx_q + ny_p ny_q) + nz_p nz_q >= normal_min
 *                  &&  fabs(z_q - ze) <= depth_tolerance * ze
 *       in tap order:  sw += b;  sl += b * L_q;  per channel  sc += b * C_q;  sv += b * V_q
 *     !(sw > 0): fresh.   Ch = sc / sw,  Vh = sv / sw,  Lh = sl / sw
 *     L' = Lh + 1;  a = fmax(1 / L', min_blend);  o = 1 - a;   C' = o * Ch + a * C_p;   V' = (o * o) * Vh + (a * a) * V_p
 * where N_q, z_q, C_q, V_q, L_q and surface_q are what the previous call wrote for pixel q.  Outputs: d_out = C',
 * d_out_variance = V', d_out_length = L' (how many frames the pixel holds; float[H*W]); the history keeps N_p, z_p, C', L',
 * V' and surface_p.  A fresh pixel writes all of its outputs too.
 * So with min_blend 0 a camera that has not moved gives the exact per-pixel running mean (the 1/64 snap makes the
 * reprojection one tap of weight 1, and L the frame count), and (C', V') go into rtmi_denoise as they are: the blend
 * propagates the variance of two independent estimates.  The mean normal's length is the pixel's coverage, so a
 * half-covered silhouette pixel fails normal_min 0.8 and starts fresh.  ze and the history's depth are both distances along
 * unit rays from p', so they compare directly.
 * Known limits: a defocus camera reprojects as its pinhole; view-dependent materials (Metal, Dielectric) lag behind the
 * camera, by at most what min_blend allows; there is no demodulation: the history holds what the caller passes.
 *
 * Defaults (what rtmi.accumulate of the Python binding passes): normal_min 0.8, depth_tolerance 0.05, min_blend 0.1.
 * RTMI_ERR_INVALID before any HIP call for: height or width outside 1..RTMI_MAX_EXTENT; a null o, g, d_color, cur_camera,
 * d_history_out or d_out; a wrong size in either struct or reserved != 0; an option outside its range; a null
 * g->d_variance, d_normal, d_depth or d_alpha; exactly one of d_history_in and prev_camera null; a history pointer that is
 * not 16-byte aligned; a non-finite camera float; a det that is 0 or not finite.  rtmi_history_bytes returns 0 for an extent
 * outside 1..RTMI_MAX_EXTENT. */
typedef struct rtmi_accumulate_opts {
  int32_t size;          /* sizeof(rtmi_accumulate_opts) of the caller: must match the library's */
  int32_t reserved;      /* 0 */
  float normal_min;      /* finite, -1..1: a history tap is taken only if its mean normal . the pixel's >= this */
  float depth_tolerance; /* finite, > 0: ... and its depth is within this fraction of the expected depth */
  float min_blend;       /* 0..1: floor of the current frame's weight; 0 = the exact running mean */
} rtmi_accumulate_opts;
size_t rtmi_history_bytes(int height, int width);
int rtmi_accumulate(int height, int width, const rtmi_accumulate_opts *o, const float *d_color, const rtmi_denoise_guides *g,
                    const float cur_camera[21], const void *d_history_in, const float prev_camera[21],
                    void *d_history_out, float *d_out, float *d_out_variance /* nullable */,
                    float *d_out_length /* nullable */, void *stream);

/* Process-wide DEFAULTS for the same fields (what rtmi_render and a zero field of rtmi_render_opts use).
 * Kept for callers of the first ABI version; prefer rtmi_render_opts.  The RTMI_SPARSE_STRIDE /
 * RTMI_EXCLUSIVE / RTMI_OUTLIER_X10 / RTMI_HEAD_CLASSES (0: tiles) / RTMI_PROBE_SPP / RTMI_PLAN / RTMI_PRIO (wave_priority) /
 * RTMI_LANE_STRIDE / RTMI_PROMOTE (promote_after) / RTMI_COST_PROBE / RTMI_FIRST_PASS / RTMI_FAST_PATH (0: the general kernel
 * always, what fast_path = -1 asks of one call) environment variables override the built-in defaults
 * of those fields and are read once, when the library is first used.  (So are the measurement knobs without an option
 * field: RTMI_FETCH_BATCH / RTMI_FETCH_BATCH_FIRST, 1..64: the largest batch a wave of a list frame draws from the work
 * queue per atomic in longest-first order / in a first pass of a few samples, defaults 16 / 64; RTMI_FIRST_PRIO, 0: a
 * first pass of the frame's own samples never has wave priorities, default 1: from 32 samples on.) */
int rtmi_set_launch(int blocks_per_cu, int threads_per_block);
int rtmi_set_schedule(int mode);

#ifdef __cplusplus
}
#endif
#endif /* RTMI_H_ */
