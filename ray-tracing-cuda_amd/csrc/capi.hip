// C ABI of librtmi.so (declared in include/rtmi.h).  Thin glue: argument
// checking, the host-side scene recorder, uploads, and kernel launches.  There is
// deliberately no CPU rendering path in this library.
#include <hip/hip_runtime.h>
#include <dlfcn.h>
#include <rccl/rccl.h>  // types and enumerators only: the entry points are looked up at run time (rtmi_gather)
#include <string.h>

#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <mutex>
#include <string>
#include <type_traits>
#include <unordered_map>

#include "../../include/rtmi.h"
#include "kernels.h"
#include "scene.h"
#include "xorwow.h"

using namespace rtmi;

static thread_local std::string g_err;
static int fail(int code, const std::string &msg) {
  g_err = msg;
  return code;
}
static int hip_fail(hipError_t e, const char *what) {
  return fail(RTMI_ERR_HIP, std::string(what) + ": " + hipGetErrorString(e));
}
#define HIP_TRY(expr)                                    \
  do {                                                   \
    hipError_t e__ = (expr);                             \
    if (e__ != hipSuccess) return hip_fail(e__, #expr);  \
  } while (0)

// Process-wide DEFAULTS of the scheduling parameters; every rtmi_render call works on its own copy
// (rtmi_render_ex overrides fields per call).  The RTMI_* environment variables are tuning overrides
// of the built-in defaults and are read once, when the library is first used.
static std::mutex g_tune_mu;
static RenderTuning g_tune;
static std::once_flag g_tune_once;
static int env_int(const char *name, int dflt) {
  const char *e = getenv(name);
  return e && *e ? atoi(e) : dflt;
}
static bool valid_stride(int v) { return v >= 1 && v <= 64 && (v & (v - 1)) == 0; }
static RenderTuning default_tuning() {
  std::call_once(g_tune_once, [] {
    g_tune.schedule = 1;
    g_tune.blocks_per_cu = 0;
    g_tune.threads = 0;
    g_tune.sparse_stride = env_int("RTMI_SPARSE_STRIDE", kSparseStride);
    if (!valid_stride(g_tune.sparse_stride)) g_tune.sparse_stride = kSparseStride;
    g_tune.exclusive = env_int("RTMI_EXCLUSIVE", 1) ? 1 : 0;
    g_tune.outlier_x10 = env_int("RTMI_OUTLIER_X10", 20);
    if (g_tune.outlier_x10 < 1) g_tune.outlier_x10 = 20;
    g_tune.head_pct[0] = 80, g_tune.head_pct[1] = 55, g_tune.head_pct[2] = 30;
    g_tune.promote = env_int("RTMI_PROMOTE", 16);  // samples after which a pixel's own ray count may promote it (0: never)
    if (g_tune.promote < 0) g_tune.promote = 0;
    g_tune.probe_spp = env_int("RTMI_PROBE_SPP", 0);
    if (g_tune.probe_spp < 0 || g_tune.probe_spp > 64) g_tune.probe_spp = 0;
    g_tune.cost_probe = env_int("RTMI_COST_PROBE", 1) != 0;
    g_tune.first_pass = env_int("RTMI_FIRST_PASS", 1);  // 0: a discarded probe; 1: the frame's first spp / 16 samples; N > 1: spp / N
    if (g_tune.first_pass < 0) g_tune.first_pass = 1;
    g_tune.lane_stride = env_int("RTMI_LANE_STRIDE", 0);
    if (g_tune.lane_stride < 0 || g_tune.lane_stride > 64 || (g_tune.lane_stride & (g_tune.lane_stride - 1)) != 0) g_tune.lane_stride = 0;
    g_tune.plan = env_int("RTMI_PLAN", 1);  // list frames: planned chains instead of the queue (0 never, 1 when waves have few tiles, 2 always)
    if (g_tune.plan < 0 || g_tune.plan > 2) g_tune.plan = 1;
    g_tune.prio_every = env_int("RTMI_PRIO", 16);  // wave priorities: update interval in iterations (0: off)
    if (g_tune.prio_every < 0 || (g_tune.prio_every & (g_tune.prio_every - 1)) != 0) g_tune.prio_every = 16;
    g_tune.fast_path = env_int("RTMI_FAST_PATH", 1) != 0;  // 0: every launch uses the general kernel (kernels.h: fast_path_mode)
    g_tune.head_classes = env_int("RTMI_HEAD_CLASSES", 1) != 0;
    g_tune.first_prio = env_int("RTMI_FIRST_PRIO", 1) != 0;
    g_tune.fetch_batch = std::clamp(env_int("RTMI_FETCH_BATCH", 16), 1, 64);
    g_tune.fetch_batch_first = std::clamp(env_int("RTMI_FETCH_BATCH_FIRST", 64), 1, 64);
  });
  std::lock_guard<std::mutex> lk(g_tune_mu);
  return g_tune;
}

static Scene *S(rtmi_scene *s) { return reinterpret_cast<Scene *>(s); }
static const Scene *S(const rtmi_scene *s) { return reinterpret_cast<const Scene *>(s); }
static V3 v3(const float *p) { return mk(p[0], p[1], p[2]); }
static bool all_finite(const float *p, size_t n) {
  for (size_t i = 0; i < n; i++)
    if (!std::isfinite(p[i])) return false;
  return true;
}

// (why the calling thread's last make_frame refused its frame, when the reason deserves its own words)
static thread_local const char *t_frame_why = nullptr;
static const char *frame_why(const char *otherwise) { return t_frame_why ? t_frame_why : otherwise; }
static bool make_frame(const rtmi_frame *f, FrameDev *out) {
  t_frame_why = nullptr;
  if (f && (f->height > RTMI_MAX_EXTENT || f->width > RTMI_MAX_EXTENT)) {  // (a pixel's row and column share a word)
    t_frame_why = "frame larger than 65535 x 65535 (RTMI_MAX_EXTENT): a pixel's row and column share a 32-bit word";
    return false;
  }
  if (!f || f->height <= 0 || f->width <= 0 || f->spp < 0 || f->world_size <= 0 || f->rank < 0 ||
      f->rank >= f->world_size)
    return false;
  FrameDev d;
  d.height = f->height, d.width = f->width, d.spp = f->spp, d.max_depth = f->max_depth, d.post = f->post_process;
  d.k_begin = 0, d.k_end = f->spp;
  d.rank = f->rank, d.world = f->world_size;
  d.tiles_x = (f->width + RTMI_TILE - 1) / RTMI_TILE;
  d.tiles_y = (f->height + RTMI_TILE - 1) / RTMI_TILE;
  d.n_tiles = d.tiles_x * d.tiles_y;
  // every rank gets the same number of work items (rank 0's share); ranks that own
  // one tile fewer carry one inert padding tile, so gathered buffers have one stride
  d.local_tiles = (d.n_tiles + d.world - 1) / d.world;
  d.items = (int64_t)d.local_tiles * 64;
  *out = d;
  return true;
}

// jump matrices, uploaded once per device
static std::mutex g_mu;
static std::unordered_map<int, uint32_t *> g_jump;
static std::unordered_map<int, int> g_cus;
static int device_jump(uint32_t **out) {
  int dev = 0;
  HIP_TRY(hipGetDevice(&dev));
  std::lock_guard<std::mutex> lk(g_mu);
  auto it = g_jump.find(dev);
  if (it == g_jump.end()) {
    const HostJump &J = host_jump_tables();
    uint32_t *d = nullptr;
    HIP_TRY(hipMalloc(&d, J.m.size() * sizeof(uint32_t)));
    HIP_TRY(hipMemcpy(d, J.m.data(), J.m.size() * sizeof(uint32_t), hipMemcpyHostToDevice));
    it = g_jump.emplace(dev, d).first;
  }
  *out = it->second;
  return RTMI_OK;
}
// compute units of device dev, cached per device (hipGetDeviceProperties is slow)
static int device_cus(int dev, int *n_cu) {
  std::lock_guard<std::mutex> lk(g_mu);
  auto it = g_cus.find(dev);
  if (it == g_cus.end()) {
    hipDeviceProp_t prop;
    HIP_TRY(hipGetDeviceProperties(&prop, dev));
    it = g_cus.emplace(dev, prop.multiProcessorCount).first;
  }
  *n_cu = it->second;
  return RTMI_OK;
}
// The scene's device must be the current one.  *n_cu (optional): its compute units.
static int scene_device(const Scene *s, int *n_cu) {
  int dev = 0;
  HIP_TRY(hipGetDevice(&dev));
  if (dev != s->device) return fail(RTMI_ERR_INVALID, "scene was committed on another device");
  return n_cu ? device_cus(dev, n_cu) : RTMI_OK;
}
static int check_depth(int max_depth) {
  if (max_depth < 0 || max_depth > RTMI_MAX_DEPTH) return fail(RTMI_ERR_DEPTH, "max_depth outside [0, 64]");
  return RTMI_OK;
}
// a pixel's closest-hit queries (at most max_depth + 1 per sample, ray_tracing.cu:22) are counted in 31 bits of its
// ray_counts word (bit 31: the scheduler's mark) and of the trace kernel's register
static int check_pixel_queries(const FrameDev &d) {
  if ((int64_t)d.spp * (d.max_depth + 1) > (int64_t)RTMI_MAX_PIXEL_QUERIES)
    return fail(RTMI_ERR_INVALID, "spp x (max_depth + 1) above 2^31 - 1 (RTMI_MAX_PIXEL_QUERIES): a pixel's closest-hit queries are counted in 31 bits");
  return RTMI_OK;
}

template <typename R>
static int upload(Scene *s, const std::vector<R> &v, const R **out) {
  *out = nullptr;
  if (v.empty()) return RTMI_OK;
  void *d = nullptr;
  HIP_TRY(hipMalloc(&d, v.size() * sizeof(R)));
  s->dev_allocs.push_back(d);
  HIP_TRY(hipMemcpy(d, v.data(), v.size() * sizeof(R), hipMemcpyHostToDevice));
  *out = reinterpret_cast<const R *>(d);
  return RTMI_OK;
}

extern "C" {

const char *rtmi_last_error(void) { return g_err.c_str(); }
int rtmi_version(void) { return RTMI_VERSION; }
int rtmi_device_count(void) {
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess) return 0;
  return n;
}

// ------------------------------------------------------------------ scene
rtmi_scene *rtmi_scene_create(void) { return reinterpret_cast<rtmi_scene *>(new Scene()); }

static void free_device(Scene *s) {
  if (s->d_sched) (void)hipFree(s->d_sched);
  s->d_sched = nullptr;
  s->sched_bytes = 0;
  for (void *p : s->dev_allocs) (void)hipFree(p);
  s->dev_allocs.clear();
  s->d_counters = nullptr;
  s->committed = false;
}
void rtmi_scene_destroy(rtmi_scene *s) {
  if (!s) return;
  free_device(S(s));
  delete S(s);
}

int rtmi_constant_texture(rtmi_scene *s, const float rgb[3]) {
  if (!s || !rgb) return fail(RTMI_ERR_INVALID, "null argument");
  HostTex t;
  t.rgb = v3(rgb);
  S(s)->texs.push_back(t);
  return (int)S(s)->texs.size() - 1;
}
int rtmi_image_texture(rtmi_scene *s, const uint8_t *rgba, int height, int width, size_t pitch) {
  if (!s || !rgba || height <= 0 || width <= 0) return fail(RTMI_ERR_INVALID, "bad image texture");
  if (pitch == 0) pitch = (size_t)width * 4;
  if (pitch < (size_t)width * 4) return fail(RTMI_ERR_INVALID, "pitch smaller than a row");
  HostTex t;
  t.image = true;
  t.h = height, t.w = width;
  t.rgba.resize((size_t)height * width * 4);
  for (int y = 0; y < height; y++) memcpy(&t.rgba[(size_t)y * width * 4], rgba + (size_t)y * pitch, (size_t)width * 4);
  S(s)->texs.push_back(std::move(t));
  return (int)S(s)->texs.size() - 1;
}
static int add_mat(rtmi_scene *s, int kind, V3 rgb, float param, int tex) {
  HostMat m;
  m.kind = kind, m.rgb = rgb, m.param = param, m.tex = tex;
  S(s)->mats.push_back(m);
  return (int)S(s)->mats.size() - 1;
}
static bool tex_ok(rtmi_scene *s, int t) { return t >= 0 && t < (int)S(s)->texs.size(); }
int rtmi_lambertian(rtmi_scene *s, const float rgb[3]) {
  if (!s || !rgb) return fail(RTMI_ERR_INVALID, "null argument");
  return add_mat(s, MAT_LAMBERTIAN, v3(rgb), 0.f, -1);
}
int rtmi_lambertian_tex(rtmi_scene *s, int texture) {
  if (!s || !tex_ok(s, texture)) return fail(RTMI_ERR_INVALID, "unknown texture handle");
  return add_mat(s, MAT_LAMBERTIAN, splat(0.f), 0.f, texture);
}
int rtmi_metal(rtmi_scene *s, const float rgb[3], float fuzz) {
  if (!s || !rgb) return fail(RTMI_ERR_INVALID, "null argument");
  return add_mat(s, MAT_METAL, v3(rgb), fuzz < 1 ? fuzz : 1, -1);  // metal.cu:10
}
int rtmi_dielectric(rtmi_scene *s, const float rgb[3], double refractive_index) {
  if (!s || !rgb) return fail(RTMI_ERR_INVALID, "null argument");
  return add_mat(s, MAT_DIELECTRIC, v3(rgb), (float)refractive_index, -1);
}
int rtmi_diffuse_light(rtmi_scene *s, int texture) {
  if (!s || !tex_ok(s, texture)) return fail(RTMI_ERR_INVALID, "unknown texture handle");
  return add_mat(s, MAT_LIGHT, splat(0.f), 0.f, texture);
}

// Every HitableList -- the world and each nested one -- holds at most kMaxHitables entries
// (hitable_list.cuh:10,20); a nested list counts as ONE entry of its parent.  Nested lists are
// recorded inlined at their position, which gives the same closest hit (DESIGN.md "List flattening").
static int count_entry(rtmi_scene *s) {
  if (S(s)->list_counts.back() >= RTMI_MAX_HITABLES)
    return fail(RTMI_ERR_CAPACITY, "HitableList::kMaxHitables (1024) exceeded");
  S(s)->list_counts.back()++;
  return RTMI_OK;
}
static int append(rtmi_scene *s, const HostObj &o) {
  int rc = count_entry(s);
  if (rc) return rc;
  S(s)->world.push_back(o);
  S(s)->committed = false;
  return RTMI_OK;
}
static bool mat_ok(rtmi_scene *s, int m) { return m >= 0 && m < (int)S(s)->mats.size(); }

int rtmi_add_sphere(rtmi_scene *s, const float c[3], double radius, int material) {
  if (!s || !c || !mat_ok(s, material)) return fail(RTMI_ERR_INVALID, "bad sphere arguments");
  if (!all_finite(c, 3) || !std::isfinite(radius)) return fail(RTMI_ERR_INVALID, "non-finite sphere");
  HostObj o{};
  o.kind = OBJ_SPHERE, o.mat = material, o.p[0] = v3(c), o.radius = radius;
  return append(s, o);
}
int rtmi_add_triangle(rtmi_scene *s, const float p[9], int material) {
  if (!s || !p || !mat_ok(s, material)) return fail(RTMI_ERR_INVALID, "bad triangle arguments");
  if (!all_finite(p, 9)) return fail(RTMI_ERR_INVALID, "non-finite triangle corner");
  HostObj o{};
  o.kind = OBJ_TRI, o.mat = material;
  for (int i = 0; i < 3; i++) o.p[i] = v3(p + 3 * i);
  return append(s, o);
}
int rtmi_add_parallelogram(rtmi_scene *s, const float p[9], int material) {
  if (!s || !p || !mat_ok(s, material)) return fail(RTMI_ERR_INVALID, "bad parallelogram arguments");
  if (!all_finite(p, 9)) return fail(RTMI_ERR_INVALID, "non-finite parallelogram corner");
  HostObj o{};
  o.kind = OBJ_PGRAM, o.mat = material;
  for (int i = 0; i < 3; i++) o.p[i] = v3(p + 3 * i);
  return append(s, o);
}
int rtmi_add_parallelepiped(rtmi_scene *s, const float p[12], int material) {
  if (!s || !p || !mat_ok(s, material)) return fail(RTMI_ERR_INVALID, "bad parallelepiped arguments");
  if (!all_finite(p, 12)) return fail(RTMI_ERR_INVALID, "non-finite parallelepiped corner");
  HostObj o{};
  o.kind = OBJ_BOX, o.mat = material;
  V3 c[4], corners[8];
  for (int i = 0; i < 4; i++) c[i] = v3(p + 3 * i);
  box_from_points(c, corners);
  box_faces(corners, o.p);
  return append(s, o);
}
int rtmi_add_parallelepiped_lengths(rtmi_scene *s, const float lengths[3], int material, rtmi_transform_fn transform,
                                    void *user) {
  if (!s || !lengths || !transform || !mat_ok(s, material))
    return fail(RTMI_ERR_INVALID, "bad parallelepiped arguments");
  // parallelepiped.cu:37-52: axis corners from the lengths, then the user's transform
  float p[4][3] = {{0, 0, 0}, {0, 0, 0}, {0, 0, 0}, {0, 0, 0}}, q[4][3];
  for (int i = 1; i <= 3; i++) p[i][i - 1] = lengths[i - 1];
  for (int i = 0; i < 4; i++)
    for (int k = 0; k < 3; k++) q[i][k] = lengths[k];
  for (int i = 1; i <= 3; i++) q[i][i - 1] = 0;
  HostObj o{};
  o.kind = OBJ_BOX, o.mat = material;
  V3 corners[8];
  for (int i = 0; i < 4; i++) {
    float t[3];
    transform(p[i], t, user);
    corners[i] = v3(t);
    transform(q[i], t, user);
    corners[4 + i] = v3(t);
  }
  for (int i = 0; i < 8; i++)
    if (!std::isfinite(corners[i].x) || !std::isfinite(corners[i].y) || !std::isfinite(corners[i].z))
      return fail(RTMI_ERR_INVALID, "the transform produced a non-finite parallelepiped corner");
  box_faces(corners, o.p);
  return append(s, o);
}
int rtmi_add_parallelepiped_faces(rtmi_scene *s, const float faces[54], int material) {
  if (!s || !faces || !mat_ok(s, material)) return fail(RTMI_ERR_INVALID, "bad parallelepiped arguments");
  if (!all_finite(faces, 54)) return fail(RTMI_ERR_INVALID, "non-finite parallelepiped corner");
  HostObj o{};
  o.kind = OBJ_BOX, o.mat = material;
  for (int i = 0; i < 18; i++) o.p[i] = v3(faces + 3 * i);
  return append(s, o);
}
int rtmi_list_begin(rtmi_scene *s) {
  if (!s) return fail(RTMI_ERR_INVALID, "null scene");
  int rc = count_entry(s);  // the nested list is one entry of the list it is appended to
  if (rc) return rc;
  S(s)->list_counts.push_back(0);
  S(s)->committed = false;
  return RTMI_OK;
}
int rtmi_list_end(rtmi_scene *s) {
  if (!s) return fail(RTMI_ERR_INVALID, "null scene");
  if (S(s)->list_counts.size() < 2) return fail(RTMI_ERR_INVALID, "rtmi_list_end without rtmi_list_begin");
  S(s)->list_counts.pop_back();
  return RTMI_OK;
}
int rtmi_add_sky(rtmi_scene *s) {
  if (!s) return fail(RTMI_ERR_INVALID, "null scene");
  HostObj o{};
  o.kind = OBJ_SKY;
  return append(s, o);
}
int rtmi_add_bvh(rtmi_scene *s, const float *faces, const float *uvs, int n, int material, int leaf_max) {
  if (!s || n < 0 || (n > 0 && !faces)) return fail(RTMI_ERR_INVALID, "bad bvh arguments");
  if (material >= (int)S(s)->mats.size()) return fail(RTMI_ERR_INVALID, "unknown material handle");
  // The reference would build such a mesh and simply never hit the face; here a non-finite coordinate would
  // poison the bounds of the search tree, so the mesh is refused (the caller drops the face).
  if (n > 0 && !all_finite(faces, (size_t)n * 9)) return fail(RTMI_ERR_INVALID, "non-finite face coordinate in the mesh");
  HostBvh b;
  b.n = n, b.mat = material, b.leaf_max = leaf_max > 0 ? leaf_max : 2048;
  b.faces.assign(faces, faces + (size_t)n * 9);
  if (uvs) b.uvs.assign(uvs, uvs + (size_t)n * 6);
  S(s)->bvhs.push_back(std::move(b));
  HostObj o{};
  o.kind = OBJ_BVH, o.bvh = (int)S(s)->bvhs.size() - 1;
  return append(s, o);
}

int rtmi_camera_pinhole(rtmi_scene *s, const float pos[3], const float look_at[3], const float up[3], double fov,
                        double aspect) {
  if (!s || !pos || !look_at || !up) return fail(RTMI_ERR_INVALID, "null argument");
  camera_pinhole(*S(s), v3(pos), v3(look_at), v3(up), fov, aspect);
  S(s)->committed = false;
  return RTMI_OK;
}
int rtmi_camera_defocus(rtmi_scene *s, const float pos[3], const float look_at[3], const float up[3], double fov,
                        double aspect, double aperture, double focus_distance) {
  if (!s || !pos || !look_at || !up) return fail(RTMI_ERR_INVALID, "null argument");
  camera_defocus(*S(s), v3(pos), v3(look_at), v3(up), fov, aspect, aperture, focus_distance);
  S(s)->committed = false;
  return RTMI_OK;
}
int rtmi_camera_raw(rtmi_scene *s, const float pos[3], const float llc[3], const float horiz[3], const float vert[3]) {
  if (!s || !pos || !llc || !horiz || !vert) return fail(RTMI_ERR_INVALID, "null argument");
  camera_raw(*S(s), v3(pos), v3(llc), v3(horiz), v3(vert));
  S(s)->committed = false;
  return RTMI_OK;
}
int rtmi_camera_set(rtmi_scene *s, const float f[21], int is_defocus, double lens_radius) {
  if (!s || !f) return fail(RTMI_ERR_INVALID, "null argument");
  CameraDev &c = S(s)->cam;
  c.position = v3(f), c.llc = v3(f + 3), c.horizontal = v3(f + 6), c.vertical = v3(f + 9);
  c.u = v3(f + 12), c.v = v3(f + 15);
  S(s)->cam_w = v3(f + 18);
  c.defocus = is_defocus ? 1 : 0;
  c.lens_radius = (float)lens_radius;  // DiskRand(float radius), camera.cu:64,74
  S(s)->has_camera = true;
  S(s)->committed = false;
  return RTMI_OK;
}
int rtmi_camera_update(rtmi_scene *s, const float f[21], int is_defocus, double lens_radius) {
  if (!s || !f) return fail(RTMI_ERR_INVALID, "null argument");
  if (!all_finite(f, 21)) return fail(RTMI_ERR_INVALID, "non-finite camera float");
  Scene *sc = S(s);
  const bool committed = sc->committed;
  if (int rc = rtmi_camera_set(s, f, is_defocus, lens_radius)) return rc;
  if (committed) {
    // The camera is host state only: every launch copies SceneDev by value into its argument block.  What flatten()
    // derives from it is the F_DEFOCUS bit of the scene's features (the render variant), and nothing else.
    sc->dev.cam = sc->cam;
    sc->features = sc->cam.defocus ? sc->features | F_DEFOCUS : sc->features & ~(uint32_t)F_DEFOCUS;
    sc->committed = true;
  }
  return RTMI_OK;
}
int rtmi_camera_get(const rtmi_scene *s, float out[21]) {
  if (!s || !out || !S(s)->has_camera) return fail(RTMI_ERR_INVALID, "scene has no camera");
  const CameraDev &c = S(s)->cam;
  const V3 vs[7] = {c.position, c.llc, c.horizontal, c.vertical, c.u, c.v, S(s)->cam_w};
  for (int i = 0; i < 7; i++) out[i * 3] = vs[i].x, out[i * 3 + 1] = vs[i].y, out[i * 3 + 2] = vs[i].z;
  return RTMI_OK;
}

// SceneDev::diffuse_only: every material is a Lambertian or a light, and none takes its colour from an image texture.
// Such a scene's fast list launches get the kernels compiled with PIN_DIFFUSE (kernels.h: render_pins).
static int diffuse_only(const std::vector<MatRec> &mats) {
  for (const MatRec &m : mats)
    if ((m.kind != MAT_LAMBERTIAN && m.kind != MAT_LIGHT) || m.tex >= 0) return 0;
  return 1;
}

int rtmi_scene_commit(rtmi_scene *sp) {
  if (!sp) return fail(RTMI_ERR_INVALID, "null scene");
  Scene *s = S(sp);
  if (s->list_counts.size() != 1) return fail(RTMI_ERR_INVALID, "a nested list is still open (rtmi_list_end missing)");
  static_assert(RTMI_MAX_MATERIALS == kMaxMats, "rtmi.h and scene_dev.h disagree on the material limit");
  if (s->mats.size() > (size_t)RTMI_MAX_MATERIALS)
    return fail(RTMI_ERR_CAPACITY, "more than RTMI_MAX_MATERIALS (2^24) materials: a triangle's material field has 24 bits");
  if (rtmi_device_count() <= 0) return fail(RTMI_ERR_NO_DEVICE, "no HIP device: librtmi has no CPU fallback");
  free_device(s);
  std::string err = s->flatten();
  if (!err.empty()) return fail(RTMI_ERR_INVALID, err);
  HIP_TRY(hipGetDevice(&s->device));
  // image textures
  s->tex_recs.clear();
  for (const HostTex &t : s->texs) {
    if (!t.image) continue;
    void *d = nullptr;
    size_t pitch = 0;
    HIP_TRY(hipMallocPitch(&d, &pitch, (size_t)t.w * 4, (size_t)t.h));
    s->dev_allocs.push_back(d);
    HIP_TRY(hipMemcpy2D(d, pitch, t.rgba.data(), (size_t)t.w * 4, (size_t)t.w * 4, (size_t)t.h,
                        hipMemcpyHostToDevice));
    TexRec r{};
    r.rgba = reinterpret_cast<const uint8_t *>(d);
    r.height = t.h, r.width = t.w, r.pitch = (int64_t)pitch;
    s->tex_recs.push_back(r);
  }
  SceneDev d{};
  int rc;
  if ((rc = upload(s, s->runs, &d.runs))) return rc;
  if ((rc = upload(s, s->spheres, &d.spheres))) return rc;
  if ((rc = upload(s, s->tris, &d.tris))) return rc;
  {
    // one allocation: the PairBox records, then the PairSlab table of the same pairs (scene_dev.h: pair_slabs_of)
    static_assert(sizeof(PairSlab) == sizeof(PairBox) && std::is_trivially_copyable<PairSlab>::value, "PairSlab records travel as PairBox");
    std::vector<PairBox> both(s->pair_boxes);
    both.resize(s->pair_boxes.size() + s->pair_slabs.size());
    if (!s->pair_slabs.empty()) memcpy(both.data() + s->pair_boxes.size(), s->pair_slabs.data(), s->pair_slabs.size() * sizeof(PairSlab));
    if ((rc = upload(s, both, &d.pair_boxes))) return rc;
  }
  // (the staging's source: a list beyond kLdsPairs is never staged and gathers from `tris`)
  if ((int)s->pair_pts.size() <= kLdsPairs && (rc = upload(s, s->tri_pts, &d.tri_pts))) return rc;
  if ((rc = upload(s, s->tri_nrm, &d.tri_nrm))) return rc;
  if ((rc = upload(s, s->sph_groups, &d.sph_groups))) return rc;
  if ((rc = upload(s, s->sph_members, &d.sph_members))) return rc;
  d.sph_mag = s->sph_mag;
  d.n_sph_groups = (int)s->sph_groups.size();
  if ((rc = upload(s, s->bvh_recs, &d.bvhs))) return rc;
  if ((rc = upload(s, s->nodes, &d.nodes))) return rc;
  if ((rc = upload(s, s->qnodes, &d.qnodes))) return rc;
  if ((rc = upload(s, s->leaf_paths, &d.leaf_paths))) return rc;
  if ((rc = upload(s, s->tops, &d.tops))) return rc;
  if ((rc = upload(s, s->faces, &d.faces))) return rc;
  if ((rc = upload(s, s->face_uv, &d.face_uv))) return rc;
#ifdef RTMI_CHECK_MARGINS
  if ((rc = upload(s, s->face_of_orig, &d.face_of_orig))) return rc;
#endif
  if ((rc = upload(s, s->mat_recs, &d.mats))) return rc;
  if ((rc = upload(s, s->tex_recs, &d.texs))) return rc;
  d.n_runs = (int)s->runs.size() - 4;  // without the padding records
  d.n_pairs = (int)s->pair_pts.size();
  d.list_mag = s->list_mag;
  d.n_mats = (int)s->mat_recs.size();
  d.n_nodes = (int)s->nodes.size();
  d.n_leaf_paths = (int)s->leaf_paths.size();
  d.sub_reserve = s->sub_depth > 0 ? 3 * s->sub_depth + 3 + kMeshFaceSlack : 0;
  d.det_safe = 1;
  for (const HotTri &t : s->tris) {
    const double a = std::sqrt((double)t.e1[0] * t.e1[0] + (double)t.e1[1] * t.e1[1] + (double)t.e1[2] * t.e1[2]);
    const double b = std::sqrt((double)t.e2[0] * t.e2[0] + (double)t.e2[1] * t.e2[1] + (double)t.e2[2] * t.e2[2]);
    if (!(a * b <= 0x1p120)) d.det_safe = 0;
  }
  d.unsigned_colours = 1;
  for (const MatRec &m : s->mat_recs) {
    const float c[3] = {m.r, m.g, m.b};
    for (float x : c) {
      uint32_t bits;
      memcpy(&bits, &x, sizeof(bits));
      if (bits >> 31) d.unsigned_colours = 0;
    }
  }
  d.diffuse_only = diffuse_only(s->mat_recs);
  d.cam = s->cam;
  s->dev = d;
  QueryDev q{};  // (rtmi_intersect only)
  if ((rc = upload(s, s->q_sphere_entry, &q.sphere_entry))) return rc;
  if ((rc = upload(s, s->q_pair_entry, &q.pair_entry))) return rc;
  if ((rc = upload(s, s->q_bvh_entry, &q.bvh_entry))) return rc;
  if ((rc = upload(s, s->q_face_input, &q.face_input))) return rc;
  q.sky_entry = s->q_sky_entry;
  s->qdev = q;
  {
    // the light table (rtmi_direct_sample only; direct.hip): beside QueryDev, SceneDev keeps its layout
    std::vector<uint32_t> light_mats;
    std::vector<LightRec> recs;
    std::vector<float> cdf;
    build_light_table(*s, &s->lights, &light_mats);
    s->sphere_lights = false;
    for (const rtmi_light &lt : s->lights) s->sphere_lights = s->sphere_lights || lt.kind == 2;
    light_records(s->lights, &recs, &cdf);
    LightDev l{};
    if ((rc = upload(s, recs, &l.recs))) return rc;
    if ((rc = upload(s, cdf, &l.cdf))) return rc;
    if ((rc = upload(s, light_mats, &l.light_mats))) return rc;
    l.n_lights = (int32_t)s->lights.size(), l.n_mats = (int32_t)s->mat_recs.size();
    std::vector<int32_t> hit_light;  // (rtmi_direct_sample_mis only)
    build_hit_light_map(s->lights, &hit_light, &l.n_entries);
    if ((rc = upload(s, hit_light, &l.hit_light))) return rc;
    s->ldev = l;
  }
  void *c = nullptr;
  // (behind the counters: the two kernel-argument blocks of a render without caller-owned scratch -- probe pass, real pass)
  HIP_TRY(hipMalloc(&c, RTMI_COUNTER_WORDS * sizeof(unsigned long long) + 2 * render_params_bytes()));
  s->dev_allocs.push_back(c);
  HIP_TRY(hipMemset(c, 0, RTMI_COUNTER_WORDS * sizeof(unsigned long long)));
  s->d_counters = reinterpret_cast<unsigned long long *>(c);
  HIP_TRY(hipDeviceSynchronize());
  s->committed = true;
  return RTMI_OK;
}

// *tmp = a flattened copy of the scene, so that an uncommitted one can be inspected.
static int flattened(const rtmi_scene *sp, Scene *tmp) {
  *tmp = *S(sp);
  tmp->dev_allocs.clear();
  const std::string err = tmp->flatten();
  return err.empty() ? RTMI_OK : fail(RTMI_ERR_INVALID, err);
}
int rtmi_scene_stats(const rtmi_scene *sp, int64_t out[8]) {
  if (!sp || !out) return fail(RTMI_ERR_INVALID, "null argument");
  Scene tmp;
  if (int rc = flattened(sp, &tmp)) return rc;
  out[0] = (int64_t)tmp.list_counts[0];
  out[1] = (int64_t)tmp.n_spheres;
  out[2] = (int64_t)tmp.n_pgrams;
  out[3] = (int64_t)tmp.n_triangles;
  out[4] = (int64_t)tmp.faces.size();
  out[5] = (int64_t)tmp.nodes.size();
  out[6] = (int64_t)tmp.mat_recs.size();
  out[7] = (int64_t)tmp.texs.size();
  return RTMI_OK;
}

int64_t rtmi_scene_sliver_faces(const rtmi_scene *sp) {
  if (!sp) return fail(RTMI_ERR_INVALID, "null scene");
  Scene tmp;
  if (int rc = flattened(sp, &tmp)) return rc;
  return tmp.sliver_faces;
}

int64_t rtmi_scene_bytes_per_ray(const rtmi_scene *sp) {
  if (!sp) return fail(RTMI_ERR_INVALID, "null scene");
  Scene tmp;
  if (int rc = flattened(sp, &tmp)) return rc;
  return tmp.bytes_per_ray;
}

// Diagnostics for the tests (host only; like rtmi_debug_wave_stats not declared in rtmi.h, the binding asks for them
// by name).  The culled list scan's records as flatten() forms them: returns the number of pairs; fills, for
// the first cap_pairs of them, two TriPts (12 words each) and two HotTri (16 words each) per pair and the pair's four
// corners (12 floats; a lone Triangle's fourth repeats its third).  Any output may be null.
int64_t rtmi_debug_list_records(const rtmi_scene *sp, int64_t cap_pairs, uint32_t *tri_pts, uint32_t *hot_tris, float *corners) {
  if (!sp) return fail(RTMI_ERR_INVALID, "null scene");
  Scene tmp;
  if (int rc = flattened(sp, &tmp)) return rc;
  const int64_t n = (int64_t)tmp.pair_pts.size();
  for (int64_t i = 0; i < n && i < cap_pairs; i++) {
    if (tri_pts) memcpy(tri_pts + 24 * i, &tmp.tri_pts[2 * i], 2 * sizeof(TriPts));
    if (hot_tris) memcpy(hot_tris + 32 * i, &tmp.tris[2 * i], 2 * sizeof(HotTri));
    if (corners) memcpy(corners + 12 * i, tmp.pair_pts[i].p0, 12 * sizeof(float));
  }
  return n;
}

// Diagnostic (as above): the slab table of the same pairs (scene_dev.h: PairSlab), padding record included: returns the
// number of records, fills the first cap of them (8 words each) and *list_mag (the scene's, which scales the table's
// widening).  Any output may be null.
int64_t rtmi_debug_pair_slabs(const rtmi_scene *sp, int64_t cap, uint32_t *slabs, uint32_t *boxes, float *list_mag) {
  if (!sp) return fail(RTMI_ERR_INVALID, "null scene");
  Scene tmp;
  if (int rc = flattened(sp, &tmp)) return rc;
  const int64_t n = (int64_t)tmp.pair_slabs.size();
  for (int64_t i = 0; i < n && i < cap; i++) {
    if (slabs) memcpy(slabs + 8 * i, &tmp.pair_slabs[i], sizeof(PairSlab));
    if (boxes) memcpy(boxes + 8 * i, &tmp.pair_boxes[i], sizeof(PairBox));
  }
  if (list_mag) *list_mag = tmp.list_mag;
  return n;
}

// Diagnostic (as above): 1 when the slab table's reach covers a render from the scene's camera (render.hip:
// slab_reach_covers, a condition of the fast list kernels), else 0.
int rtmi_debug_slab_reach(const rtmi_scene *sp) {
  if (!sp) return fail(RTMI_ERR_INVALID, "null scene");
  Scene tmp;
  if (int rc = flattened(sp, &tmp)) return rc;
  return slab_reach_covers(tmp.list_mag, tmp.cam) ? 1 : 0;
}

// Diagnostic (as above): SceneDev::diffuse_only as a commit of this scene would set it.
int rtmi_debug_diffuse_only(const rtmi_scene *sp) {
  if (!sp) return fail(RTMI_ERR_INVALID, "null scene");
  Scene tmp;
  if (int rc = flattened(sp, &tmp)) return rc;
  return diffuse_only(tmp.mat_recs);
}

// Diagnostic (as above): bytes of dynamic LDS one workgroup of `threads` lanes asks for when this scene is rendered at
// max_depth (render.hip: make_cfg).  A compute unit has 160 KiB.
int64_t rtmi_debug_render_lds_bytes(const rtmi_scene *sp, int max_depth, int threads) {
  if (!sp || max_depth < 0 || threads < 64 || threads % 64) return fail(RTMI_ERR_INVALID, "bad arguments");
  Scene tmp;
  if (int rc = flattened(sp, &tmp)) return rc;
  SceneDev d{};
  d.n_pairs = (int)tmp.pair_pts.size(), d.n_mats = (int)tmp.mat_recs.size(), d.n_nodes = (int)tmp.nodes.size();
  d.n_leaf_paths = (int)tmp.leaf_paths.size(), d.n_sph_groups = (int)tmp.sph_groups.size();
  FrameDev fr{};
  fr.max_depth = max_depth;
  return (int64_t)render_lds_bytes(pick_variant(tmp.features), d, fr, threads);
}

// ------------------------------------------------------------------ frame
int64_t rtmi_frame_work_items(const rtmi_frame *f) {
  FrameDev d;
  if (!make_frame(f, &d)) return fail(RTMI_ERR_INVALID, frame_why("bad frame"));
  return d.items;
}
int64_t rtmi_frame_pixel_of(const rtmi_frame *f, int64_t q) {
  FrameDev d;
  if (!make_frame(f, &d) || q < 0 || q >= d.items) return -1;
  return frame_pixel_of(d, d.rank, q);
}
int rtmi_frame_pixel_map(const rtmi_frame *f, int64_t *out) {
  FrameDev d;
  if (!make_frame(f, &d) || !out) return fail(RTMI_ERR_INVALID, frame_why("bad frame"));
  for (int64_t q = 0; q < d.items; q++) out[q] = frame_pixel_of(d, d.rank, q);
  return RTMI_OK;
}
size_t rtmi_states_bytes(const rtmi_frame *f) {
  FrameDev d;
  if (!make_frame(f, &d)) return 0;
  return (size_t)d.items * RTMI_STATE_WORDS * sizeof(uint32_t);
}
size_t rtmi_tiles_bytes(const rtmi_frame *f) {
  FrameDev d;
  if (!make_frame(f, &d)) return 0;
  return (size_t)d.items * 3 * sizeof(float);
}

// ------------------------------------------------------------------ RNG
int rtmi_rng_init(uint64_t seed, const rtmi_frame *f, void *d_states, void *stream) {
  FrameDev d;
  if (!make_frame(f, &d) || !d_states) return fail(RTMI_ERR_INVALID, frame_why("bad rng_init arguments"));
  if (rtmi_device_count() <= 0) return fail(RTMI_ERR_NO_DEVICE, "no HIP device: librtmi has no CPU fallback");
  uint32_t *jump = nullptr;
  int rc = device_jump(&jump);
  if (rc) return rc;
  HIP_TRY(launch_rng_init(seed, d, jump, reinterpret_cast<uint32_t *>(d_states), (hipStream_t)stream));
  return RTMI_OK;
}
int rtmi_rng_init_n(uint64_t seed, uint64_t first, int64_t n, void *d_states, void *stream) {
  // the device jump tables cover subsequences below 2^40 (xorwow.h: kJumpBits)
  // (and n below 2^31 as for rtmi_trace: one state per lane of a one-dimensional grid)
  if (n < 0 || n > (int64_t)INT32_MAX || (n > 0 && !d_states) || first > (1ull << kJumpBits) ||
      (uint64_t)n > (1ull << kJumpBits) - first)
    return fail(RTMI_ERR_INVALID, "bad rng_init_n arguments (n < 0, n above 2^31 - 1, first + n above 2^40, or null states)");
  if (n == 0) return RTMI_OK;
  if (rtmi_device_count() <= 0) return fail(RTMI_ERR_NO_DEVICE, "no HIP device: librtmi has no CPU fallback");
  uint32_t *jump = nullptr;
  int rc = device_jump(&jump);
  if (rc) return rc;
  FrameDev d{};
  d.items = n;
  HIP_TRY(launch_rng_init(seed, d, jump, reinterpret_cast<uint32_t *>(d_states), (hipStream_t)stream, (int64_t)first));
  return RTMI_OK;
}
int rtmi_rng_host_state(uint64_t seed, uint64_t subsequence, uint32_t state[RTMI_STATE_WORDS]) {
  if (!state) return fail(RTMI_ERR_INVALID, "null state");
  Rng r = host_rng_init(seed, subsequence);
  state[0] = r.d, state[1] = r.v0, state[2] = r.v1, state[3] = r.v2, state[4] = r.v3, state[5] = r.v4;
  return RTMI_OK;
}
float rtmi_rng_host_random_float(float mn, float mx, uint32_t state[RTMI_STATE_WORDS]) {
  Rng r{state[0], state[1], state[2], state[3], state[4], state[5]};
  float x = rng_range(mn, mx, r);
  state[0] = r.d, state[1] = r.v0, state[2] = r.v1, state[3] = r.v2, state[4] = r.v3, state[5] = r.v4;
  return x;
}
int rtmi_rng_set_state(const rtmi_frame *f, void *d_states, int64_t q, const uint32_t state[RTMI_STATE_WORDS],
                       void *stream) {
  FrameDev d;
  if (!make_frame(f, &d) || !d_states || !state || q < 0 || q >= d.items)
    return fail(RTMI_ERR_INVALID, "bad rng_set_state arguments");
  uint32_t *base = reinterpret_cast<uint32_t *>(d_states);
  for (int w = 0; w < RTMI_STATE_WORDS; w++)
    HIP_TRY(hipMemcpyAsync(base + (size_t)w * d.items + q, &state[w], sizeof(uint32_t), hipMemcpyHostToDevice,
                           (hipStream_t)stream));
  HIP_TRY(hipStreamSynchronize((hipStream_t)stream));
  return RTMI_OK;
}
int rtmi_rng_get_state(const rtmi_frame *f, const void *d_states, int64_t q, uint32_t state[RTMI_STATE_WORDS],
                       void *stream) {
  FrameDev d;
  if (!make_frame(f, &d) || !d_states || !state || q < 0 || q >= d.items)
    return fail(RTMI_ERR_INVALID, "bad rng_get_state arguments");
  const uint32_t *base = reinterpret_cast<const uint32_t *>(d_states);
  for (int w = 0; w < RTMI_STATE_WORDS; w++)
    HIP_TRY(hipMemcpyAsync(&state[w], base + (size_t)w * d.items + q, sizeof(uint32_t), hipMemcpyDeviceToHost,
                           (hipStream_t)stream));
  HIP_TRY(hipStreamSynchronize((hipStream_t)stream));
  return RTMI_OK;
}

// ------------------------------------------------------------------ render
// Per-call scratch of a frame, the one description of it (rtmi_render_scratch_bytes, run_plan).  The counters come
// first so that rtmi_render_status can find them from the scratch pointer alone; then what the scheduler's probe pass
// leaves for the real pass, rounded up to 256 bytes; then the wave-priority table and the kernel-argument blocks.
static constexpr size_t kCounterBytes = RTMI_COUNTER_WORDS * sizeof(unsigned long long);
static constexpr int kMaxChains = 1 << 15;  // planned chains: one per wave of the grid (8 waves x 4 SIMDs x 1024 CUs)
struct ScratchLayout {  // byte offsets of the regions (sizes: scratch_layout), and the whole
  size_t states, rays, cost, order;   // the probe's RNG states and ray counts; tile costs, tile order
  size_t meta, head, work;            // scheduler meta (launch_tile_order), the head list right behind it; probe work counts
  size_t qcost, qsorted, qmap, qmax;  // quarter tiles: costs, sorted, order; their maximum
  size_t fut, next, claims, first;    // chain plan: per tile what follows, next tile, claim; per chain its first tile
  size_t prio_tab, params, total;     // wave-priority table, the two kernel-argument blocks (probe pass, real pass)
};
static ScratchLayout scratch_layout(const FrameDev &d) {
  const size_t n = (size_t)d.items, nt = (size_t)d.local_tiles;
  ScratchLayout l;
  size_t at = kCounterBytes;
  auto region = [&at](size_t bytes) { const size_t o = at; at += bytes; return o; };
  l.states = region(n * RTMI_STATE_WORDS * 4);
  l.rays = region(n * 4);
  l.cost = region(nt * 4), l.order = region(nt * 4);
  l.meta = region(32 * 4);  // (8-byte aligned: with n = 64 nt, 320 + 1800 nt bytes in)
  l.head = region((size_t)kHeadCap * 4);
  l.work = region(n * 4);
  l.qcost = region(nt * 16), l.qsorted = region(nt * 16), l.qmap = region(nt * 16), l.qmax = region(16);
  l.fut = region(nt * 4), l.next = region(nt * 4), l.claims = region(nt * 4);
  l.first = region((size_t)kMaxChains * 4);
  at = (at + 255) & ~(size_t)255;
  l.prio_tab = region(kPrioTabBytes);
  l.params = region(2 * render_params_bytes());
  l.total = at;
  return l;
}
size_t rtmi_render_scratch_bytes(const rtmi_frame *f) {
  FrameDev d;
  if (!make_frame(f, &d)) return 0;
  return scratch_layout(d).total;
}

int rtmi_render(const rtmi_scene *sp, const rtmi_frame *f, void *d_states, float *d_tiles, uint32_t *d_ray_counts,
                void *stream) {
  return rtmi_render_ex(sp, f, nullptr, d_states, d_tiles, d_ray_counts, stream);
}

// rtmi_render_opts over the process defaults -> the tuning of ONE call.
static int resolve_opts(const rtmi_render_opts *opts, RenderTuning *tune, void **scratch, size_t *scratch_bytes) {
  *tune = default_tuning();
  *scratch = nullptr, *scratch_bytes = 0;
  if (!opts) return RTMI_OK;
  if (opts->size != (int32_t)sizeof(rtmi_render_opts)) return fail(RTMI_ERR_INVALID, "rtmi_render_opts.size does not match this library");
  if (opts->schedule > 2 || opts->blocks_per_cu < 0 || opts->threads_per_block < 0 || (opts->threads_per_block % 64) != 0 ||
      opts->threads_per_block > 512 || (opts->sparse_stride != 0 && !valid_stride(opts->sparse_stride)) || opts->exclusive > 1 ||
      opts->outlier_x10 < 0 || opts->probe_spp < 0 || opts->probe_spp > 64 || opts->plan > 2 || opts->wave_priority > 4096 ||
      (opts->wave_priority > 0 && (opts->wave_priority & (opts->wave_priority - 1)) != 0) || opts->lane_stride < 0 ||
      opts->lane_stride > 64 || (opts->lane_stride & (opts->lane_stride - 1)) != 0 || opts->cost_probe > 1 || opts->first_pass > 4096 ||
      opts->fast_path < -1 || opts->fast_path > 1)
    return fail(RTMI_ERR_INVALID, "rtmi_render_opts field out of range");
  for (int i = 0; i < 3; i++)
    if (opts->head_pct[i] < 0 || opts->head_pct[i] > 100) return fail(RTMI_ERR_INVALID, "rtmi_render_opts.head_pct outside [0, 100]");
  if (opts->schedule >= 0) tune->schedule = opts->schedule;
  if (opts->blocks_per_cu > 0) tune->blocks_per_cu = opts->blocks_per_cu;
  if (opts->threads_per_block > 0) tune->threads = opts->threads_per_block;
  if (opts->sparse_stride > 0) tune->sparse_stride = opts->sparse_stride, tune->head_classes = 0;  // (a named stride is for outlier tiles)
  if (opts->exclusive >= 0) tune->exclusive = opts->exclusive;
  if (opts->outlier_x10 > 0) tune->outlier_x10 = opts->outlier_x10;
  if (opts->probe_spp > 0) tune->probe_spp = opts->probe_spp;
  if (opts->plan >= 0) tune->plan = opts->plan;
  if (opts->wave_priority >= 0) tune->prio_every = opts->wave_priority;
  if (opts->lane_stride > 0) tune->lane_stride = opts->lane_stride;
  if (opts->promote_after >= 0) tune->promote = opts->promote_after;
  if (opts->cost_probe >= 0) tune->cost_probe = opts->cost_probe;
  if (opts->first_pass >= 0) tune->first_pass = opts->first_pass;
  if (opts->fast_path != 0) tune->fast_path = opts->fast_path > 0;
  for (int i = 0; i < 3; i++)
    if (opts->head_pct[i] > 0) tune->head_pct[i] = opts->head_pct[i];
  if (!(tune->head_pct[0] >= tune->head_pct[1] && tune->head_pct[1] >= tune->head_pct[2]))
    return fail(RTMI_ERR_INVALID, "rtmi_render_opts.head_pct must not increase from the heaviest class to the lightest");
  *scratch = opts->d_scratch, *scratch_bytes = opts->scratch_bytes;
  return RTMI_OK;
}

// Kernel variant and launch shape of a frame on the current device.
struct LaunchShape {
  uint32_t variant;
  int threads, per_cu, blocks, n_cu, lane_stride;
  FastPathFacts fast;  // what the fast kernels ask of scene and frame (fast_mode adds a launch's own facts)
};
// The fast-path mode word of one launch (kernels.h: fast_path_mode; 0: the general kernel).  priorities, chains,
// tile_cost: the launch has a priority table, walks planned chains, has the probe's tile costs; resumed: it resumes a
// first pass.
static uint32_t fast_mode(FastPathFacts f, int lane_stride, bool priorities, bool chains, bool resumed, bool tile_cost) {
  f.lane_stride = lane_stride, f.priorities = priorities, f.chains = chains, f.resumed = resumed, f.tile_cost = tile_cost;
  return fast_path_mode(f);
}
static constexpr int kMaxLaneStride = 16;
static int launch_shape(const Scene *s, const FrameDev &d, const RenderTuning &tune, LaunchShape *out) {
  int n_cu = 0;
  if (int rc = scene_device(s, &n_cu)) return rc;
  const uint32_t variant = pick_variant(s->features);
  int threads = tune.threads > 0 ? tune.threads : 256;
  if (threads > 256 && !(variant & F_BVH)) threads = 256;  // only the mesh kernels are built for larger workgroups
  if (tune.threads <= 0 && (variant & F_BVH)) {
    // mesh variants keep ~310 B of LDS per lane plus per-workgroup tables: when a deep id stack leaves
    // room for one 256-lane workgroup only, smaller workgroups keep more lanes resident
    int best = 0;
    for (int t = 256; t >= 64; t /= 2) {
      const int lanes = t * render_occupancy(variant, s->dev, d, t);  // (mesh variants: no fast kernels)
      if (lanes > best) best = lanes, threads = t;
    }
  }
  // (asked of the kernel that will really be launched: the general one, or whichever of the fast ones it may be -- without
  // the facts of scene and frame no launch of this frame uses a fast kernel)
  out->fast = fast_path_facts(variant, s->dev, d, threads, tune.fast_path);
  int per_cu = tune.blocks_per_cu > 0 ? tune.blocks_per_cu
                                      : render_occupancy(variant, s->dev, d, threads, fast_mode(out->fast, 1, true, false, false, false) != 0u);
  if (per_cu <= 0) per_cu = 1;
  int64_t want = (d.items + threads - 1) / threads;
  int64_t cap = (int64_t)n_cu * per_cu;
  // A list frame smaller than the grid is spread thin (render_body.h: lane_stride): one pixel per 2 / 4 / ... lanes, as
  // far as the grid has room, when the closest-hit query shares its candidate tests between the lanes of a wave (the
  // culled list scan, the grouped sphere scan: a wave with a quarter of the rays then runs shorter iterations)
  int stride = 1;
  const bool shared_tests = ((variant & F_TRIS) && s->dev.n_pairs >= kCullMinPairs) || ((variant & F_SGROUP) && s->dev.n_sph_groups > 0);
  if (!(variant & F_BVH) && shared_tests) {
    if (tune.lane_stride > 0) stride = tune.lane_stride;
    else
      while (stride < kMaxLaneStride && want * stride * 2 <= cap) stride *= 2;
  }
  want *= stride;
  int blocks = (int)(want < cap ? want : cap);
  if (blocks < 1) blocks = 1;
  out->variant = variant, out->threads = threads, out->per_cu = per_cu, out->blocks = blocks, out->n_cu = n_cu;
  out->lane_stride = stride;
  return RTMI_OK;
}

// How a frame will be rendered: everything that is decided, from host values alone, before anything is launched.
// rtmi_render_ex executes it (run_plan); rtmi_render_launch_shape and rtmi_render_mode report it.
struct RenderPlan {
  const Scene *s;                    // the call, as render_prologue resolves it: scene, frame, the caller's scratch (or null)
  FrameDev d;                        //   and the tuning; plan_render then gives the tuning the shape's lane stride and lowers
  void *user_scratch;                //   its prio_every for a short frame
  size_t user_scratch_bytes;
  RenderTuning tune;
  LaunchShape ls;
  int waves, probe_spp;              // waves of the grid; samples per pixel of the first pass
  bool scheduled, resume, prio;      // a first pass orders the rest; it is the frame's own first samples; wave priorities
  bool chains, by_cost, first_prio;  // list tiles run as planned chains; mesh frames: the probe books its searches' cost; the
                                     // first pass has wave priorities too
  int plan_simds, plan_rounds;       // chains: on this many SIMDs, this many waves each
  uint32_t sparse_cap;               // work items the grid holds at one pixel per tune.sparse_stride lanes (a multiple of 64)
  bool scratch;                      // the call needs scratch memory at all
  FrameDev first, finish;            // the first pass; the launch that finishes the frame: all of it, or what a first pass left
  uint32_t first_fast, finish_fast;  // their fast-path mode words
};
// What the three render entries resolve first, in this order: options, committed, frame.
static int render_prologue(const rtmi_scene *sp, const rtmi_frame *f, const rtmi_render_opts *opts, RenderPlan *p) {
  if (int rc = resolve_opts(opts, &p->tune, &p->user_scratch, &p->user_scratch_bytes)) return rc;
  p->s = S(sp);
  if (!p->s->committed) return fail(RTMI_ERR_INVALID, "scene not committed");
  if (!make_frame(f, &p->d)) return fail(RTMI_ERR_INVALID, frame_why("bad frame"));
  return RTMI_OK;
}
static int plan_render(RenderPlan *p) {
  const FrameDev &d = p->d;
  LaunchShape &ls = p->ls;
  RenderTuning &tune = p->tune;
  if (int rc = launch_shape(p->s, d, tune, &ls)) return rc;
  tune.lane_stride = ls.lane_stride;
  const uint32_t variant = ls.variant;
  const int64_t resident = (int64_t)ls.blocks * ls.threads;
  p->waves = ls.blocks * (ls.threads / 64);
  // When is a list frame planned?  The plan wins where the queue cannot even things out (few tiles per wave) AND its
  // estimates are good enough (long pixels: many samples).  Measured, planned against queued, cornell depth 50: 1.33
  // tiles per wave (a 2048^2 frame over eight GPUs): 128 spp 20.9 / 21.0 ms, 512 spp 66 / 77, 4096 spp 480 / 590; 2.67
  // tiles per wave (1024^2): 128 spp 38.3 / 35.1, 256 spp 66.8 / 64.3, 512 spp 122.4 / 123.5, 1024 spp 237 / 241; 5.3
  // (half a 2048^2 x 4096 frame) 1763 / 1787; 6.4 (a C5 shard, 8192 spp) 2853 / 2917; 10.7: the same.  Spheres 1024^2 x
  // 64 spp, 3.2 tiles per wave: 21.3-22.6 / 20.4.
  const int64_t plan_tiles = d.local_tiles, plan_waves = p->waves;
  const bool plan_pays = (2 * plan_tiles <= 3 * plan_waves && d.spp >= 128) || (plan_tiles <= 3 * plan_waves && d.spp >= 512) ||
                         (plan_tiles <= 8 * plan_waves && d.spp >= 2048);
  const bool may_plan = tune.plan && tune.prio_every > 0 && d.spp >= 64 && !(variant & F_BVH) && ls.lane_stride == 1 &&
                        (tune.plan == 2 || plan_pays);
  // Samples of the scheduler's first look at the frame.  As a DISCARDED probe (first_pass = 0): two for the queue (its
  // order only has to be roughly longest-first: 2 / 4 / 8 / 16 spp gave 606 / 620 / 609 / 614 ms on a round-3 C4 shard),
  // 1 / 256 of the frame's samples, at most 16, for a plan, which is only as balanced as its estimates (C4 shard 2 / 8 /
  // 16 / 32 / 64: 495 / 486 / 484 / 482 / 484 ms, probe included).  rtmi_render_opts.probe_spp overrides either way.
  int &probe_spp = p->probe_spp = tune.probe_spp > 0 ? tune.probe_spp : 2;
  if (tune.probe_spp <= 0 && may_plan) probe_spp = d.spp / 256 < 2 ? 2 : d.spp / 256 > 16 ? 16 : d.spp / 256;
  const bool many_tiles = (int64_t)d.local_tiles * 64 > resident;
  // The probe is the frame's own first samples (tune.first_pass): samples [0, s1) of every pixel are rendered into the
  // caller's buffers from the queue in image order, their ray counts order / plan the rest, and the second launch
  // resumes every pixel at sample s1 -- nothing is rendered twice, and s1 can be a sixteenth of the frame where a
  // discarded probe had to stay at a few samples (a 64-spp frame planned on 2 discarded samples: 21.9 ms; on 8: 20.5,
  // their cost included).  first_pass = 0 keeps the discarded probe on a scratch copy of the RNG states.
  const bool two_pass = tune.first_pass != 0;
  if (two_pass && tune.probe_spp <= 0) {
    // a frame that will be planned spends a sixteenth of its samples (at most 64) on the first pass: the plan is as good
    // as its estimates (C2: 238.9 -> 236.9 ms); everything else two -- the first pass runs from the plain queue, which
    // is the slower way to render a mesh frame (C3 with 32 first samples: 83 ms against 74) or a short one (spheres
    // 1024^2 x 64 spp: 2 / 4 / 8 first samples 20.3 / 20.7 / 21.5 ms; the discarded 2-spp probe: 20.9)
    const int div = tune.first_pass > 1 ? tune.first_pass : 16;
    probe_spp = !may_plan ? 2 : d.spp / div < 2 ? 2 : d.spp / div > 64 ? 64 : d.spp / div;
  }
  // (a first pass costs nothing but a launch, so short frames are scheduled too where it matters most: a mesh frame's
  // outlier pixels -- the reference's own bunny program, 1280 x 720 x 20 spp: 7.3 -> 4.9 ms -- from 8 samples per pixel
  // on; list frames from 32: at the reference's defaults, 100-200 spp, scheduled and unscheduled differ by +-4 %)
  const int min_spp = two_pass ? ((variant & F_BVH) ? 8 : 32) : 32 * probe_spp;
  p->scheduled = tune.schedule == 2 || (tune.schedule == 1 && many_tiles && d.spp >= min_spp && d.spp >= 2 * probe_spp);
  // wave priorities (render_body.h: wave_priority_update) pay for themselves when a wave lives for many updates
  // ... from eight samples per pixel on; a short frame's waves live for tens of iterations, so they look every four
  // (C1, spheres 256^2 x 16 spp: 2.07 -> 1.86 ms; every 16: 1.89, every 2: 1.94, every iteration: 2.07)
  p->prio = tune.prio_every > 0 && d.spp >= 8;
  if (p->prio && d.spp < 64 && tune.prio_every > 4) tune.prio_every = 4;
  p->resume = p->scheduled && two_pass && probe_spp < d.spp;
  // list frames: planned chains instead of the queue (kernels.h: launch_chain_plan), one per wave of the grid
  p->plan_simds = ls.n_cu * 4 < p->waves ? ls.n_cu * 4 : p->waves;  // (four SIMDs per compute unit)
  p->plan_rounds = (p->waves + p->plan_simds - 1) / p->plan_simds;
  p->chains = p->scheduled && may_plan && p->prio && p->plan_simds * p->plan_rounds <= kMaxChains;
  // mesh frames (binary32 t): the probe also books the lane-steps of its mesh searches on the pixels they serve
  p->by_cost = tune.cost_probe && (variant & F_BVH) && !(variant & F_SPHERE);
  // (a first pass of the frame's own samples is a frame of s1 samples per pixel: from 32 on it has wave priorities too)
  p->first_prio = p->prio && p->resume && probe_spp >= 32 && tune.first_prio;
  p->sparse_cap = (uint32_t)((resident / tune.sparse_stride) / 64 * 64);
  p->scratch = p->scheduled || p->prio;
  // first pass: the frame's own samples [0, probe_spp) into the caller's buffers, or a discarded probe on copies
  p->first = p->finish = d;
  p->first.k_end = probe_spp;
  if (p->resume) p->finish.k_begin = probe_spp;
  else p->first.spp = probe_spp;
  // the kernels compiled for the common list frame, where a launch is one (a first pass never walks chains)
  p->first_fast = fast_mode(ls.fast, ls.lane_stride, p->first_prio, false, false, false);
  p->finish_fast = fast_mode(ls.fast, ls.lane_stride, p->prio, p->chains, p->resume, p->scheduled);
  return RTMI_OK;
}

int rtmi_render_launch_shape(const rtmi_scene *sp, const rtmi_frame *f, const rtmi_render_opts *opts, int32_t out[4]) {
  if (!sp || !out) return fail(RTMI_ERR_INVALID, "null argument");
  RenderPlan p;
  int rc;
  if ((rc = render_prologue(sp, f, opts, &p)) || (rc = plan_render(&p))) return rc;
  out[0] = p.ls.blocks, out[1] = p.ls.threads, out[2] = p.ls.per_cu, out[3] = p.ls.n_cu;
  return RTMI_OK;
}

int rtmi_render_mode(const rtmi_scene *sp, const rtmi_frame *f, const rtmi_render_opts *opts, int32_t out[8]) {
  return rtmi_render_mode_ex(sp, f, opts, out, 8);
}
int rtmi_render_mode_ex(const rtmi_scene *sp, const rtmi_frame *f, const rtmi_render_opts *opts, int32_t *dst, int n) {
  if (!sp || !dst || n < 0) return fail(RTMI_ERR_INVALID, "null argument");
  RenderPlan p;
  int rc;
  if ((rc = render_prologue(sp, f, opts, &p)) || (rc = plan_render(&p))) return rc;
  // ([8]: the kernel of the launch that finishes the frame)
  const int32_t out[RTMI_MODE_FIELDS] = {p.scheduled, p.scheduled ? p.probe_spp : 0, p.resume, p.chains, p.prio ? p.tune.prio_every : 0,
                                         p.ls.lane_stride, p.waves, p.d.local_tiles, p.finish_fast != 0u};
  for (int i = 0; i < n && i < RTMI_MODE_FIELDS; i++) dst[i] = out[i];
  return RTMI_OK;
}

int rtmi_render_pins(const rtmi_scene *sp, const rtmi_frame *f, const rtmi_render_opts *opts, uint32_t out[2]) {
  if (!sp || !out) return fail(RTMI_ERR_INVALID, "null argument");
  RenderPlan p;
  int rc;
  if ((rc = render_prologue(sp, f, opts, &p)) || (rc = plan_render(&p))) return rc;
  out[0] = p.scheduled ? render_pins(p.first_fast, p.s->dev) : 0u;
  out[1] = render_pins(p.finish_fast, p.s->dev);
  return RTMI_OK;
}

// The regions of a call's scratch (ScratchLayout's offsets) as pointers.
struct Scratch {
  uint32_t *states, *rays, *cost, *order, *meta, *head, *work, *qcost, *qsorted, *qmap, *qmax, *fut, *claims, *prio_tab;
  int32_t *next, *first;
};
static Scratch scratch_regions(void *base, const ScratchLayout &l) {
  const auto at = [base](size_t off) { return reinterpret_cast<uint32_t *>(static_cast<char *>(base) + off); };
  const auto ints = [&at](size_t off) { return reinterpret_cast<int32_t *>(at(off)); };
  return Scratch{at(l.states), at(l.rays), at(l.cost), at(l.order), at(l.meta), at(l.head), at(l.work), at(l.qcost), at(l.qsorted),
                 at(l.qmap), at(l.qmax), at(l.fut), at(l.claims), at(l.prio_tab), ints(l.next), ints(l.first)};
}

// The scheduler step: from a first pass's ray counts (and, optionally, its work counts) to what the finishing launch
// walks -- the tile order, the head, the queue's order per quarter tile and, for planned chains, the chain plan with its
// claims zeroed.  Which region of the scratch feeds which launcher is decided here and nowhere else: run_plan and
// rtmi_debug_schedule both call it.
struct SchedStep {
  int tiles;                    // local tiles of the frame
  bool pixel_head;              // the head is made of pixels in weight classes (r.head), not of outlier tiles
  uint32_t sparse_cap;          // outlier tiles: work items the grid holds at one pixel per sparse stride
  int waves, outlier_x10;       // waves of the grid; an outlier tile costs this many tenths of the mean
  const int *head_pct;          // [3]: the weight classes' thresholds in per cent of the largest count
  int simds, rounds;            // planned chains: SIMDs x waves per SIMD; simds * rounds == 0: no chain plan
  int spp, probe_spp;           // chains: samples of the frame and of the first pass (chain_fut's scale)
};
static int schedule_step(const Scratch &r, uint32_t *rays, const uint32_t *work, const SchedStep &k, SchedPlan *plan,
                         hipStream_t st) {
  uint32_t *head = k.pixel_head ? r.head : nullptr;
  HIP_TRY(launch_tile_order(rays, k.tiles, r.cost, r.meta, r.order, head, k.sparse_cap, k.waves, k.outlier_x10, k.head_pct, st));
  // (the head's marks in rays are bit 31: quarter_cost_kernel masks them off)
  HIP_TRY(launch_quarter_order(r.order, work, rays, k.tiles, r.qcost, r.qsorted, r.qmax, r.qmap, st));
  plan->tile_order = r.qmap;
  plan->sparse_items = r.meta + 1;
  plan->head_list = head;
  plan->probe_marks = head ? rays : nullptr;
  plan->probe_spp = k.probe_spp;
  plan->tile_cost = r.cost;
  if ((int64_t)k.simds * k.rounds > 0) {
    HIP_TRY(launch_chain_plan(r.order, r.cost, k.tiles, k.simds, k.rounds, k.spp, k.probe_spp, r.first, r.next, r.fut, st));
    HIP_TRY(hipMemsetAsync(r.claims, 0, (size_t)k.tiles * 4, st));
    plan->chain_next = r.next, plan->chain_fut = r.fut, plan->chain_first = r.first, plan->claims = r.claims;
    plan->plan_simds = k.simds, plan->plan_rounds = k.rounds;
    plan->tile_order = r.order;  // (per tile in this mode: the take-over's order)
  }
  return RTMI_OK;
}

// Executes a plan: resolves the scratch, then memsets, copies and launches in stream order.  Decides nothing.
static int run_plan(const RenderPlan &p, uint32_t *d_states, float *d_tiles, uint32_t *d_ray_counts, hipStream_t st) {
  const Scene *s = p.s;
  const FrameDev &d = p.d;
  const ScratchLayout sl = scratch_layout(d);
  if (p.user_scratch && p.user_scratch_bytes < sl.total)
    return fail(RTMI_ERR_INVALID, "rtmi_render_opts.scratch_bytes < rtmi_render_scratch_bytes(frame)");
  // Every piece of device state of this call -- queue cursors, ray total, abandoned-search flag, the scheduler's
  // buffers -- lives in the caller's scratch when one is given: renders of one scene on several streams (or as N
  // shards on one device) then share nothing but the read-only scene.  Without one the scene's own (a cache, not
  // scene state) is used, which ties renders of this scene to one at a time.
  unsigned long long *counters = p.user_scratch ? reinterpret_cast<unsigned long long *>(p.user_scratch) : s->d_counters;
  // the kernels' argument blocks (render_body.h: RenderParams): probe pass, real pass
  char *params = p.user_scratch ? reinterpret_cast<char *>(p.user_scratch) + sl.params
                                : reinterpret_cast<char *>(s->d_counters) + kCounterBytes;
  void *scratch = p.user_scratch;
  if (!scratch && p.scratch) {
    Scene *ms = const_cast<Scene *>(s);
    std::lock_guard<std::mutex> lk(g_mu);  // (re)allocation only
    if (ms->sched_bytes < sl.total) {
      if (ms->d_sched) (void)hipFree(ms->d_sched);
      ms->d_sched = nullptr, ms->sched_bytes = 0;
      HIP_TRY(hipMalloc(&ms->d_sched, sl.total));
      ms->sched_bytes = sl.total;
    }
    scratch = ms->d_sched;
  }
  const Scratch r = scratch ? scratch_regions(scratch, sl) : Scratch{};
  SchedPlan plan;
  uint32_t *ray_buf = d_ray_counts;  // (a resumed pixel reads its count back: scratch when the caller wants none)
  if (p.prio) {
    plan.prio_tab = r.prio_tab;
    HIP_TRY(hipMemsetAsync(plan.prio_tab, 0, kPrioTabBytes, st));
  }
  if (p.scheduled) {
    const size_t n = (size_t)d.items;
    uint32_t *first_states = p.resume ? d_states : r.states;
    uint32_t *first_rays = p.resume && d_ray_counts ? d_ray_counts : r.rays;
    if (p.resume) ray_buf = first_rays;
    else HIP_TRY(hipMemcpyAsync(r.states, d_states, n * RTMI_STATE_WORDS * 4, hipMemcpyDeviceToDevice, st));
    HIP_TRY(hipMemsetAsync(counters, 0, kCounterBytes, st));
    // (a discarded probe writes its radiance into d_tiles, which the real pass overwrites)
    SchedPlan probe_plan;
    if (p.by_cost) {
      HIP_TRY(hipMemsetAsync(r.work, 0, n * 4, st));
      probe_plan.visit_counts = r.work;
    }
    if (p.first_prio) probe_plan.prio_tab = plan.prio_tab;
    HIP_TRY(launch_render(p.ls.variant, s->dev, p.first, first_states, d_tiles, first_rays, counters, probe_plan, true,
                          p.first_fast, p.ls.blocks, p.ls.threads, p.tune, params, st));
#ifdef RTMI_CHECK_MARGINS
    // Test hook of the check build: RTMI_CHECK_PLANT_ABANDONED=1 (read once) counts one abandoned mesh search after every
    // first pass the frame keeps.  No world makes the search abandon one (mesh_search.h), and a test has to see that
    // rtmi_render_status still reports it after the second launch (tests/test_gpu_first_pass_status.py).
    static const bool plant_abandoned = env_int("RTMI_CHECK_PLANT_ABANDONED", 0) != 0;
    if (plant_abandoned && p.resume) HIP_TRY(launch_add_one(counters + 2, st));
#endif
    if (p.first_prio) HIP_TRY(hipMemsetAsync(plan.prio_tab, 0, kPrioTabBytes, st));
    // The scheduler's kernels read the first pass's ray counts and MARK the head's pixels in them (bit 31), and the
    // marks must outlive the pixels' final counts, which the second launch writes into the same words as it goes: they
    // work on a copy (in the region a discarded probe's RNG states would have used).
    if (p.resume) HIP_TRY(hipMemcpyAsync(r.states, first_rays, n * 4, hipMemcpyDeviceToDevice, st));
    uint32_t *rays = p.resume ? r.states : r.rays;
    // the head of a mesh frame's queue: pixels in weight classes (the default), or -- when the call names a
    // sparse stride, or RTMI_HEAD_CLASSES=0 -- the outlier tiles at one pixel per that many lanes
    const bool by_pixels = p.tune.head_classes != 0;
    SchedStep k;
    k.tiles = d.local_tiles, k.pixel_head = (p.ls.variant & F_BVH) && by_pixels;
    k.sparse_cap = p.sparse_cap, k.waves = p.waves, k.outlier_x10 = p.tune.outlier_x10, k.head_pct = p.tune.head_pct;
    k.simds = p.chains ? p.plan_simds : 0, k.rounds = p.chains ? p.plan_rounds : 0, k.spp = d.spp, k.probe_spp = p.probe_spp;
    if (int rc = schedule_step(r, rays, p.by_cost && by_pixels ? r.work : nullptr, k, &plan, st)) return rc;
  }
  // The counter words (render_body.h, mesh_search.h; rtmi_debug_counters) before the launch that finishes the frame:
  //   [0]       work-queue cursor                                   zeroed (per launch)
  //   [1]       closest-hit queries                                 zeroed (a resumed pixel re-adds its whole count)
  //   [2]       abandoned mesh searches (rtmi_render_status)        kept after a first pass the frame keeps
  //   [3]       head-queue cursor                                   zeroed (per launch)
  //   [4..32]   -DRTMI_STATS wave step counts and cycles            zeroed (per launch)
  //   [16]      of them, in every build: tasks of the culled scan    zeroed (per launch)
  //             that sent their flush through the ordered fold
  //             ([12..15]: a list kernel's stats build counts the ordered fold's trips per flush there)
  //   [33] [34] -DRTMI_CHECK_MARGINS queries re-done, disagreements kept after a first pass the frame keeps
  //   [35] [36] planned chains: SIMD arrival, take-over cursor      zeroed (per launch)
  //   [37..39]  -DRTMI_STATS flushes of the culled scan by n_now    zeroed (per launch)
  // So a resumed frame reports in [2], [33] and [34] over both launches.  Otherwise every word is zeroed: a discarded
  // probe's samples are not in the image.
  if (p.resume) {
    HIP_TRY(hipMemsetAsync(counters, 0, 2 * sizeof(unsigned long long), st));
    HIP_TRY(hipMemsetAsync(counters + 3, 0, 30 * sizeof(unsigned long long), st));
    HIP_TRY(hipMemsetAsync(counters + 35, 0, (RTMI_COUNTER_WORDS - 35) * sizeof(unsigned long long), st));
  } else {
    HIP_TRY(hipMemsetAsync(counters, 0, kCounterBytes, st));
  }
  HIP_TRY(launch_render(p.ls.variant, s->dev, p.finish, d_states, d_tiles, ray_buf, counters, plan, false, p.finish_fast,
                        p.ls.blocks, p.ls.threads, p.tune, params + render_params_bytes(), st));
  return RTMI_OK;
}

int rtmi_render_ex(const rtmi_scene *sp, const rtmi_frame *f, const rtmi_render_opts *opts, void *d_states,
                   float *d_tiles, uint32_t *d_ray_counts, void *stream) {
  if (!sp || !d_states || !d_tiles) return fail(RTMI_ERR_INVALID, "null argument");
  RenderPlan p;
  int rc;
  if ((rc = render_prologue(sp, f, opts, &p)) || (rc = check_depth(p.d.max_depth)) || (rc = check_pixel_queries(p.d)) ||
      (rc = plan_render(&p)))
    return rc;
  return run_plan(p, reinterpret_cast<uint32_t *>(d_states), d_tiles, d_ray_counts, (hipStream_t)stream);
}

int rtmi_fast_path_kernel(const int32_t facts[RTMI_FAST_PATH_FACTS]) {
  if (!facts) return fail(RTMI_ERR_INVALID, "null argument");
  FastPathFacts f{};
  f.enabled = facts[0], f.variant = (uint32_t)facts[1], f.n_mats = facts[2], f.mats_in_lds = facts[3], f.pairs_in_lds = facts[4];
  f.unsigned_colours = facts[5], f.det_safe = facts[6], f.width = facts[7], f.height = facts[8], f.lane_stride = facts[9];
  f.priorities = facts[10], f.chains = facts[11], f.resumed = facts[12], f.tile_cost = facts[13];
  const uint32_t m = fast_path_mode(f);
  return m == kFastChains ? 2 : m == kFastQueue ? 1 : 0;
}

// ------------------------------------------------------------------ batches of caller rays
// What rtmi_intersect, rtmi_occluded and rtmi_trace check before they launch, in this order: the arguments first, without
// a HIP call (the host never reads the rays), then the scene's device.  max_depth (rtmi_trace's, else null): n is at most
// 2^31 - 1 and the depth in [0, RTMI_MAX_DEPTH] too.  *n_cu: the device's compute units, 0 when n == 0 (nothing to do).
static int batch_prologue(const rtmi_scene *sp, int64_t n, bool arrays, const char *null_arrays, const int *max_depth,
                          const Scene **out, int *n_cu) {
  *n_cu = 0;
  if (!sp) return fail(RTMI_ERR_INVALID, "null scene");
  if (n < 0) return fail(RTMI_ERR_INVALID, "negative ray count");
  if (max_depth && n > (int64_t)INT32_MAX) return fail(RTMI_ERR_INVALID, "more than 2^31 - 1 rays");
  if (n > 0 && !arrays) return fail(RTMI_ERR_INVALID, null_arrays);
  const Scene *s = *out = S(sp);
  if (!s->committed) return fail(RTMI_ERR_INVALID, "scene not committed");
  if (max_depth)
    if (int rc = check_depth(*max_depth)) return rc;
  return scene_device(s, n == 0 ? nullptr : n_cu);
}

// ------------------------------------------------------------------ closest-hit queries
static int intersect(const rtmi_scene *sp, int64_t n, const float *d_o, const float *d_d, const float *d_t_max,
                     rtmi_hit *d_hits, unsigned long long *d_abandoned, unsigned long long *d_check, void *stream) {
  static_assert(sizeof(rtmi_hit) == 12 * sizeof(int32_t), "rtmi_hit is 48 bytes");
  const Scene *s;
  int n_cu;
  const int rc = batch_prologue(sp, n, d_o && d_d && d_hits, "null ray or hit array", nullptr, &s, &n_cu);
  if (rc || n == 0) return rc;
  HIP_TRY(launch_query(pick_query_variant(s->features), s->dev, s->qdev, n_cu, n, d_o, d_d, d_t_max,
                       reinterpret_cast<int32_t *>(d_hits), d_abandoned, d_check, (hipStream_t)stream));
  return RTMI_OK;
}

int rtmi_intersect(const rtmi_scene *s, int64_t n, const float *d_origins, const float *d_dirs, const float *d_t_max,
                   rtmi_hit *d_hits, unsigned long long *d_abandoned, void *stream) {
  return intersect(s, n, d_origins, d_dirs, d_t_max, d_hits, d_abandoned, nullptr, stream);
}
#ifdef RTMI_CHECK_MARGINS
int rtmi_intersect_check_counts(const rtmi_scene *s, int64_t n, const float *d_origins, const float *d_dirs,
                                const float *d_t_max, rtmi_hit *d_hits, unsigned long long *d_abandoned,
                                unsigned long long *d_check, void *stream) {
  return intersect(s, n, d_origins, d_dirs, d_t_max, d_hits, d_abandoned, d_check, stream);
}
#endif

// ------------------------------------------------------------------ any-hit visibility queries
// Longer rays that start inside a mesh's bounds run into quirk g8 for most of what the mesh occludes (occlusion_body.h):
// they walk from +inf instead.  The padding and the length (1/20 of the meshes' extent) only move rays between two exact
// ways of answering.
static void near_box(const Scene *s, float near_lo[3], float near_hi[3], float *near_short) {
  *near_short = 0.f;
  for (int k = 0; k < 3; k++) near_lo[k] = INFINITY, near_hi[k] = -INFINITY;
  for (const BvhRec &br : s->bvh_recs)
    for (int k = 0; k < 3; k++)
      near_lo[k] = fminf(near_lo[k], br.root_mn[k]), near_hi[k] = fmaxf(near_hi[k], br.root_mx[k]);
  if (!s->bvh_recs.empty()) {
    float diag = 0.f, mag = 0.f;
    for (int k = 0; k < 3; k++)
      diag = fmaxf(diag, near_hi[k] - near_lo[k]), mag = fmaxf(mag, fmaxf(fabsf(near_lo[k]), fabsf(near_hi[k])));
    const float pad = 1e-2f * diag + 1e-4f * mag;
    *near_short = 0.05f * diag;
    for (int k = 0; k < 3; k++) near_lo[k] -= pad, near_hi[k] += pad;
  }
}

static int occluded(const rtmi_scene *sp, int64_t n, const float *d_o, const float *d_d, const float *d_t_max,
                    uint8_t *d_occluded, unsigned long long *d_counts, unsigned long long *d_check, void *stream) {
  const Scene *s;
  int n_cu;
  const int rc = batch_prologue(sp, n, d_o && d_d && d_occluded, "null ray or output array", nullptr, &s, &n_cu);
  if (rc || n == 0) return rc;
  float near_lo[3], near_hi[3], near_short;
  near_box(s, near_lo, near_hi, &near_short);
  HIP_TRY(launch_occlusion(pick_query_variant(s->features), s->dev, near_lo, near_hi, near_short, n_cu, n, nullptr, d_o, d_d,
                           d_t_max, d_occluded, d_counts, d_check, (hipStream_t)stream));
  return RTMI_OK;
}

int rtmi_occluded(const rtmi_scene *s, int64_t n, const float *d_origins, const float *d_dirs, const float *d_t_max,
                  uint8_t *d_occluded, unsigned long long *d_counts, void *stream) {
  return occluded(s, n, d_origins, d_dirs, d_t_max, d_occluded, d_counts, nullptr, stream);
}
#ifdef RTMI_CHECK_MARGINS
int rtmi_occluded_check_counts(const rtmi_scene *s, int64_t n, const float *d_origins, const float *d_dirs,
                               const float *d_t_max, uint8_t *d_occluded, unsigned long long *d_counts,
                               unsigned long long *d_check, void *stream) {
  return occluded(s, n, d_origins, d_dirs, d_t_max, d_occluded, d_counts, d_check, stream);
}
#endif

// ------------------------------------------------------------------ radiance of caller rays
int rtmi_trace(const rtmi_scene *sp, int64_t n, const float *d_origins, const float *d_dirs, int max_depth,
               void *d_states, float *d_radiance, uint32_t *d_ray_counts, unsigned long long *d_work, void *stream) {
  const Scene *s;
  int n_cu;
  const int rc = batch_prologue(sp, n, d_origins && d_dirs && d_states && d_radiance && d_work,
                                "null ray, state, radiance or work array", &max_depth, &s, &n_cu);
  if (rc || n == 0) return rc;
  hipStream_t st = (hipStream_t)stream;
  // the counter words (abandoned searches, queries, queue cursor) start from zero; the argument block behind them is
  // written by launch_trace
  HIP_TRY(hipMemsetAsync(d_work, 0, kCallParamsOffset, st));
  HIP_TRY(launch_trace(pick_query_variant(s->features), s->dev, (s->features & F_TEX) != 0, n_cu, n, max_depth, d_origins, d_dirs,
                       reinterpret_cast<uint32_t *>(d_states), d_radiance, d_ray_counts, d_work, st));
  return RTMI_OK;
}

// ------------------------------------------------------------------ one step of the trace loop
int rtmi_bounce(const rtmi_scene *sp, int64_t n, float *d_origins, float *d_dirs, void *d_states, float *d_emitted,
                float *d_attenuation, rtmi_hit *d_hits, uint32_t *d_steps, unsigned long long *d_work, void *stream) {
  const Scene *s;
  int n_cu;
  const int no_depth = 0;  // (the step knows none; handed over for rtmi_trace's bound on n)
  const int rc = batch_prologue(sp, n, d_origins && d_dirs && d_states && d_emitted && d_attenuation && d_work,
                                "null ray, state, emitted, attenuation or work array", &no_depth, &s, &n_cu);
  if (rc || n == 0) return rc;
  hipStream_t st = (hipStream_t)stream;
  HIP_TRY(hipMemsetAsync(d_work, 0, kCallParamsOffset, st));  // (as rtmi_trace)
  HIP_TRY(launch_bounce(pick_query_variant(s->features), s->dev, s->qdev, n_cu, n, nullptr, d_origins, d_dirs,
                        reinterpret_cast<uint32_t *>(d_states), d_emitted, d_attenuation, reinterpret_cast<int32_t *>(d_hits),
                        d_steps, d_work, st));
  return RTMI_OK;
}

// ------------------------------------------------------------------ steps over live paths only
// What the entries that take the candidates of a list (path_list.h) check, in two pieces with each entry's own checks
// between them.  The arguments, without a HIP call: the list ...
static int check_list(int64_t n, const uint32_t *d_list, int64_t n_list) {
  if (n_list < 0) return fail(RTMI_ERR_INVALID, "negative list length");
  if (n_list > (int64_t)INT32_MAX) return fail(RTMI_ERR_INVALID, "more than 2^31 - 1 list entries");
  if (!d_list && n_list > n) return fail(RTMI_ERR_INVALID, "a null list is the paths 0 .. n_list - 1: n_list must not exceed n");
  return RTMI_OK;
}
// ... behind n in 0 .. 2^31 - 1, refused in the entry's own words (rtmi_path_advance's n is its frame's items: it checks
// the list alone).
static int list_args(int64_t n, const char *negative, const char *too_many, const uint32_t *d_list, int64_t n_list) {
  if (n < 0) return fail(RTMI_ERR_INVALID, negative);
  if (n > (int64_t)INT32_MAX) return fail(RTMI_ERR_INVALID, too_many);
  return check_list(n, d_list, n_list);
}
// Then the scene: committed, and the current device's.  *n_cu: its compute units when there is work (n > 0 and
// n_list > 0), else 0.
static int list_scene(const Scene *s, bool work, int *n_cu) {
  *n_cu = 0;
  if (!s->committed) return fail(RTMI_ERR_INVALID, "scene not committed");
  return scene_device(s, work ? n_cu : nullptr);
}

size_t rtmi_path_compact_scratch_bytes(int64_t n_list) { return path_compact_scratch_bytes(n_list); }

int rtmi_path_compact(int64_t n, const float *d_origins, const float *d_dirs, const uint32_t *d_list_in, int64_t n_list,
                      const uint32_t *d_count_in, uint32_t *d_list_out, uint32_t *d_count_out, void *d_scratch, void *stream) {
  if (const int rc = list_args(n, "negative path count", "more than 2^31 - 1 paths", d_list_in, n_list)) return rc;
  if (n_list > 0 && !(d_origins && d_dirs && d_list_out && d_count_out && d_scratch))
    return fail(RTMI_ERR_INVALID, "null ray, output list, output count or scratch array");
  if (d_list_out && d_list_out == d_list_in) return fail(RTMI_ERR_INVALID, "d_list_out must not be d_list_in: ping-pong two lists");
  if (d_count_out && d_count_out == d_count_in) return fail(RTMI_ERR_INVALID, "d_count_out must not be d_count_in: ping-pong two counts");
  if (!d_count_out) return RTMI_OK;  // (n_list == 0 and nowhere to write the 0)
  HIP_TRY(launch_path_compact(n, d_origins, d_dirs, PathList{d_list_in, d_count_in, (uint32_t)n_list}, d_list_out, d_count_out,
                              reinterpret_cast<uint32_t *>(d_scratch), (hipStream_t)stream));
  return RTMI_OK;
}

int rtmi_bounce_list(const rtmi_scene *sp, int64_t n, const uint32_t *d_list, int64_t n_list, const uint32_t *d_count,
                     float *d_origins, float *d_dirs, void *d_states, float *d_emitted, float *d_attenuation, rtmi_hit *d_hits,
                     uint32_t *d_steps, unsigned long long *d_work, void *stream) {
  if (!sp) return fail(RTMI_ERR_INVALID, "null scene");
  if (const int rc = list_args(n, "negative ray count", "more than 2^31 - 1 rays", d_list, n_list)) return rc;
  if (n > 0 && !(d_origins && d_dirs && d_states && d_emitted && d_attenuation && d_work))
    return fail(RTMI_ERR_INVALID, "null ray, state, emitted, attenuation or work array");
  const Scene *s = S(sp);
  int n_cu;
  const int rc = list_scene(s, n > 0 && n_list > 0, &n_cu);
  if (rc || n == 0) return rc;
  hipStream_t st = (hipStream_t)stream;
  HIP_TRY(hipMemsetAsync(d_work, 0, kCallParamsOffset, st));  // (as rtmi_trace)
  if (n_list == 0) return RTMI_OK;                            // (an empty list: no path stepped, and d_work says so)
  const PathList list{d_list, d_count, (uint32_t)n_list};
  HIP_TRY(launch_bounce(pick_query_variant(s->features), s->dev, s->qdev, n_cu, n, &list, d_origins, d_dirs,
                        reinterpret_cast<uint32_t *>(d_states), d_emitted, d_attenuation, reinterpret_cast<int32_t *>(d_hits),
                        d_steps, d_work, st));
  return RTMI_OK;
}

int rtmi_path_fold(int64_t n, int layers, const float *d_dirs, const uint32_t *d_steps, const float *d_emitted,
                   const float *d_attenuation, float *d_radiance, void *stream) {
  if (n < 0) return fail(RTMI_ERR_INVALID, "negative path count");
  if (n > (int64_t)INT32_MAX) return fail(RTMI_ERR_INVALID, "more than 2^31 - 1 paths");
  if (layers < 1 || layers > RTMI_MAX_DEPTH) return fail(RTMI_ERR_INVALID, "layers outside 1..RTMI_MAX_DEPTH");
  if (n > 0 && !(d_dirs && d_steps && d_emitted && d_attenuation && d_radiance))
    return fail(RTMI_ERR_INVALID, "null direction, step, emitted, attenuation or radiance array");
  HIP_TRY(launch_path_fold(n, layers, d_dirs, d_steps, d_emitted, d_attenuation, d_radiance, (hipStream_t)stream));
  return RTMI_OK;
}

// ------------------------------------------------------------------ next-event estimation
int64_t rtmi_scene_light_count(const rtmi_scene *sp) {
  if (!sp) return fail(RTMI_ERR_INVALID, "null scene");
  if (!S(sp)->committed) return fail(RTMI_ERR_INVALID, "scene not committed");
  return (int64_t)S(sp)->lights.size();
}

int rtmi_scene_lights(const rtmi_scene *sp, rtmi_light *out, int64_t n) {
  if (!sp) return fail(RTMI_ERR_INVALID, "null scene");
  if (!S(sp)->committed) return fail(RTMI_ERR_INVALID, "scene not committed");
  if (n < 0) return fail(RTMI_ERR_INVALID, "negative light count");
  if (n > 0 && !out) return fail(RTMI_ERR_INVALID, "null light array");
  const std::vector<rtmi_light> &l = S(sp)->lights;
  const size_t c = std::min((size_t)n, l.size());
  if (c) memcpy(out, l.data(), c * sizeof(rtmi_light));
  return RTMI_OK;
}

int rtmi_scene_light_kinds(rtmi_scene *sp, uint32_t kinds) {
  if (!sp) return fail(RTMI_ERR_INVALID, "null scene");
  if (S(sp)->committed) return fail(RTMI_ERR_INVALID, "rtmi_scene_light_kinds after rtmi_scene_commit: the table is made at commit");
  if (kinds != RTMI_LIGHTS_FLAT && kinds != (RTMI_LIGHTS_FLAT | RTMI_LIGHTS_SPHERES))
    return fail(RTMI_ERR_INVALID, "light kinds must be RTMI_LIGHTS_FLAT or RTMI_LIGHTS_FLAT | RTMI_LIGHTS_SPHERES");
  S(sp)->light_kinds = kinds;
  return RTMI_OK;
}

// The checks and the argument block the two steps share: *work says whether anything is to be launched.
static int direct_args(const rtmi_scene *sp, int64_t n, const uint32_t *d_list, int64_t n_list, const uint32_t *d_count,
                       uint32_t step, int sample, const float *d_origins, const float *d_dirs, const rtmi_hit *d_hits,
                       const uint32_t *d_steps, float *d_emitted, const float *d_attenuation, void *d_light_states,
                       uint32_t *d_flags, float *d_shadow_origins, float *d_shadow_dirs, float *d_shadow_t_max, float *d_direct,
                       unsigned long long *d_counts, const float *d_carry, bool mis, DirectArgs *out, int *n_cu, bool *work) {
  if (!sp) return fail(RTMI_ERR_INVALID, "null scene");
  if (const int rc = list_args(n, "negative path count", "more than 2^31 - 1 paths", d_list, n_list)) return rc;
  if (step >= (uint32_t)RTMI_MAX_DEPTH) return fail(RTMI_ERR_INVALID, "step outside 0..RTMI_MAX_DEPTH - 1");
  if (n_list > 0 && !(d_origins && d_dirs && d_hits && d_steps && d_emitted && d_attenuation && d_light_states && d_flags &&
                      d_shadow_origins && d_shadow_dirs && d_shadow_t_max && d_direct))
    return fail(RTMI_ERR_INVALID, "null ray, hit, step, emitted, attenuation, light state, flag, shadow ray or direct array");
  if (mis && n_list > 0 && (!d_carry || (reinterpret_cast<uintptr_t>(d_carry) & 15u)))
    return fail(RTMI_ERR_INVALID, "null carry array, or one that is not 16-byte aligned");
  const Scene *s = S(sp);
  *work = n > 0 && n_list > 0;
  if (const int rc = list_scene(s, *work, n_cu)) return rc;
  if (!*work) return RTMI_OK;
  DirectArgs &a = *out;
  a.lt = s->ldev, a.mats = s->dev.mats;
  a.list = d_list, a.count = d_count;
  a.n = (uint32_t)n, a.n_list = (uint32_t)n_list, a.step = step, a.sample = sample != 0 ? 1u : 0u;
  a.origins = d_origins, a.dirs = d_dirs, a.hits = reinterpret_cast<const int32_t *>(d_hits), a.steps = d_steps;
  a.emitted = d_emitted, a.attenuation = d_attenuation;
  a.light_states = reinterpret_cast<uint32_t *>(d_light_states), a.flags = d_flags;
  a.shadow_o = d_shadow_origins, a.shadow_d = d_shadow_dirs, a.shadow_t = d_shadow_t_max, a.direct = d_direct;
  a.counts = d_counts;
  return RTMI_OK;
}

int rtmi_direct_sample(const rtmi_scene *sp, int64_t n, const uint32_t *d_list, int64_t n_list, const uint32_t *d_count,
                       uint32_t step, int sample, const float *d_origins, const float *d_dirs, const rtmi_hit *d_hits,
                       const uint32_t *d_steps, float *d_emitted, const float *d_attenuation, void *d_light_states,
                       uint32_t *d_flags, float *d_shadow_origins, float *d_shadow_dirs, float *d_shadow_t_max, float *d_direct,
                       unsigned long long *d_counts, void *stream) {
  DirectArgs a{};
  int n_cu = 0;
  bool work = false;
  if (const int rc = direct_args(sp, n, d_list, n_list, d_count, step, sample, d_origins, d_dirs, d_hits, d_steps, d_emitted,
                                 d_attenuation, d_light_states, d_flags, d_shadow_origins, d_shadow_dirs, d_shadow_t_max,
                                 d_direct, d_counts, nullptr, false, &a, &n_cu, &work))
    return rc;
  if (!work) return RTMI_OK;
  const Scene *s = S(sp);
  if (s->sphere_lights) {
    DirectMisArgs b{};
    static_cast<DirectArgs &>(b) = a;
    b.hit_light = s->ldev.hit_light, b.n_entries = s->ldev.n_entries, b.carry = nullptr;
    HIP_TRY(launch_direct_sample_sph(b, false, n_cu, (hipStream_t)stream));
    return RTMI_OK;
  }
  HIP_TRY(launch_direct_sample(a, n_cu, (hipStream_t)stream));
  return RTMI_OK;
}

int rtmi_direct_sample_mis(const rtmi_scene *sp, const rtmi_direct_sample_mis_args *p, void *stream) {
  static_assert(sizeof(rtmi_direct_sample_mis_args) == 160, "rtmi_direct_sample_mis_args is 160 bytes");
  if (!sp) return fail(RTMI_ERR_INVALID, "null scene");
  if (!p) return fail(RTMI_ERR_INVALID, "null rtmi_direct_sample_mis_args");
  if (p->size != (int32_t)sizeof(rtmi_direct_sample_mis_args) || p->reserved != 0)
    return fail(RTMI_ERR_INVALID, "rtmi_direct_sample_mis_args.size does not match this library, or reserved is not 0");
  DirectMisArgs a{};
  int n_cu = 0;
  bool work = false;
  if (const int rc = direct_args(sp, p->n, p->d_list, p->n_list, p->d_count, p->step, p->sample, p->d_origins, p->d_dirs, p->d_hits,
                                 p->d_steps, p->d_emitted, p->d_attenuation, p->d_light_states, p->d_flags, p->d_shadow_origins,
                                 p->d_shadow_dirs, p->d_shadow_t_max, p->d_direct, p->d_counts, p->d_carry, true, &a, &n_cu, &work))
    return rc;
  if (!work) return RTMI_OK;
  const Scene *s = S(sp);
  a.hit_light = s->ldev.hit_light, a.n_entries = s->ldev.n_entries, a.carry = p->d_carry;
  if (s->sphere_lights) {
    HIP_TRY(launch_direct_sample_sph(a, true, n_cu, (hipStream_t)stream));
    return RTMI_OK;
  }
  HIP_TRY(launch_direct_sample_mis(a, n_cu, (hipStream_t)stream));
  return RTMI_OK;
}

int rtmi_path_fold_direct(int64_t n, int layers, const float *d_dirs, const uint32_t *d_steps, const float *d_emitted,
                          const float *d_attenuation, const float *d_direct, const uint8_t *d_occluded, float *d_radiance,
                          void *stream) {
  if (n < 0) return fail(RTMI_ERR_INVALID, "negative path count");
  if (n > (int64_t)INT32_MAX) return fail(RTMI_ERR_INVALID, "more than 2^31 - 1 paths");
  if (layers < 1 || layers > RTMI_MAX_DEPTH) return fail(RTMI_ERR_INVALID, "layers outside 1..RTMI_MAX_DEPTH");
  if (n > 0 && !(d_dirs && d_steps && d_emitted && d_attenuation && d_direct && d_occluded && d_radiance))
    return fail(RTMI_ERR_INVALID, "null direction, step, emitted, attenuation, direct, occlusion or radiance array");
  HIP_TRY(launch_path_fold_direct(n, layers, d_dirs, d_steps, d_emitted, d_attenuation, d_direct, d_occluded, d_radiance,
                                  (hipStream_t)stream));
  return RTMI_OK;
}

// ------------------------------------------------------------------ radiance of caller rays with direct light
int rtmi_trace_direct(const rtmi_scene *sp, const rtmi_trace_direct_args *p, void *stream) {
  static_assert(sizeof(rtmi_trace_direct_args) == 88, "rtmi_trace_direct_args is 88 bytes");
  if (!sp) return fail(RTMI_ERR_INVALID, "null scene");
  if (!p) return fail(RTMI_ERR_INVALID, "null rtmi_trace_direct_args");
  if (p->size != (int32_t)sizeof(rtmi_trace_direct_args) || p->reserved != 0)
    return fail(RTMI_ERR_INVALID, "rtmi_trace_direct_args.size does not match this library, or reserved is not 0");
  if (p->n > 0 && !p->d_light_states) return fail(RTMI_ERR_INVALID, "null light state array");
  if (p->d_light_states && p->d_light_states == p->d_states)
    return fail(RTMI_ERR_INVALID, "d_light_states must not be d_states: a path's draws and its light draws are two streams");
  const Scene *s;
  int n_cu;
  int max_depth = p->max_depth;
  const int rc = batch_prologue(sp, p->n, p->d_origins && p->d_dirs && p->d_states && p->d_radiance && p->d_work,
                                "null ray, state, radiance or work array", &max_depth, &s, &n_cu);
  if (rc || p->n == 0) return rc;
  hipStream_t st = (hipStream_t)stream;
  HIP_TRY(hipMemsetAsync(p->d_work, 0, kCallParamsOffset, st));  // (as rtmi_trace)
  TraceDirectBufs dx{};
  dx.ld = s->ldev, dx.qd = s->qdev;
  dx.light_states = reinterpret_cast<uint32_t *>(p->d_light_states), dx.counts = p->d_counts;
  HIP_TRY(launch_trace_direct(pick_query_variant(s->features), s->dev, (s->features & F_TEX) != 0, s->sphere_lights, n_cu, p->n,
                              max_depth, p->d_origins, p->d_dirs, reinterpret_cast<uint32_t *>(p->d_states), dx, p->d_radiance,
                              p->d_ray_counts, p->d_work, st));
  return RTMI_OK;
}

// ------------------------------------------------------------------ Russian roulette
static bool roulette_floor(float p_min) { return p_min > 0.f && p_min <= 1.f; }  // (a NaN is neither)

int rtmi_path_roulette(const rtmi_path_roulette_args *p, void *stream) {
  static_assert(sizeof(rtmi_path_roulette_args) == 104, "rtmi_path_roulette_args is 104 bytes");
  if (!p) return fail(RTMI_ERR_INVALID, "null rtmi_path_roulette_args");
  if (p->size != (int32_t)sizeof(rtmi_path_roulette_args) || p->reserved != 0 || p->reserved2 != 0)
    return fail(RTMI_ERR_INVALID, "rtmi_path_roulette_args.size does not match this library, or reserved or reserved2 is not 0");
  if (const int rc = list_args(p->n, "negative path count", "more than 2^31 - 1 paths", p->d_list, p->n_list)) return rc;
  if (p->n_list > 0 && !(p->d_steps && p->d_dirs && p->d_attenuation && p->d_states && p->d_throughput))
    return fail(RTMI_ERR_INVALID, "null step, direction, attenuation, state or throughput array");
  if (p->step >= (uint32_t)RTMI_MAX_DEPTH) return fail(RTMI_ERR_INVALID, "step outside 0..RTMI_MAX_DEPTH - 1");
  if (!roulette_floor(p->p_min)) return fail(RTMI_ERR_INVALID, "p_min outside (0, 1]");
  RouletteArgs a{};
  a.list = p->d_list, a.count = p->d_count;
  a.n = (uint32_t)p->n, a.n_list = (uint32_t)p->n_list, a.step = p->step, a.first_step = p->first_step, a.p_min = p->p_min;
  a.steps = p->d_steps, a.dirs = p->d_dirs, a.attenuation = p->d_attenuation, a.throughput = p->d_throughput;
  a.states = reinterpret_cast<uint32_t *>(p->d_states), a.counts = p->d_counts;
  HIP_TRY(launch_path_roulette(a, (hipStream_t)stream));
  return RTMI_OK;
}

int rtmi_trace_roulette(const rtmi_scene *sp, const rtmi_trace_roulette_args *p, void *stream) {
  static_assert(sizeof(rtmi_trace_roulette_args) == 88, "rtmi_trace_roulette_args is 88 bytes");
  if (!sp) return fail(RTMI_ERR_INVALID, "null scene");
  if (!p) return fail(RTMI_ERR_INVALID, "null rtmi_trace_roulette_args");
  if (p->size != (int32_t)sizeof(rtmi_trace_roulette_args) || p->reserved != 0)
    return fail(RTMI_ERR_INVALID, "rtmi_trace_roulette_args.size does not match this library, or reserved is not 0");
  if (!roulette_floor(p->p_min)) return fail(RTMI_ERR_INVALID, "p_min outside (0, 1]");
  const Scene *s;
  int n_cu;
  int max_depth = p->max_depth;
  const int rc = batch_prologue(sp, p->n, p->d_origins && p->d_dirs && p->d_states && p->d_radiance && p->d_work,
                                "null ray, state, radiance or work array", &max_depth, &s, &n_cu);
  if (rc || p->n == 0) return rc;
  hipStream_t st = (hipStream_t)stream;
  HIP_TRY(hipMemsetAsync(p->d_work, 0, kCallParamsOffset, st));  // (as rtmi_trace)
  HIP_TRY(launch_trace_roulette(pick_query_variant(s->features), s->dev, (s->features & F_TEX) != 0, n_cu, p->n, max_depth,
                                p->first_step, p->p_min, p->d_origins, p->d_dirs, reinterpret_cast<uint32_t *>(p->d_states),
                                p->d_radiance, p->d_ray_counts, p->d_counts, p->d_work, st));
  return RTMI_OK;
}

// ------------------------------------------------------------------ any-hit queries for the paths of a list
// rtmi_occluded for rtmi_bounce_list's candidates.  The arguments first, without a HIP call, then the scene's device.
static int occluded_list(const rtmi_scene *sp, int64_t n, const uint32_t *d_list, int64_t n_list, const uint32_t *d_count,
                         const float *d_o, const float *d_d, const float *d_t_max, uint8_t *d_occluded,
                         unsigned long long *d_counts, unsigned long long *d_check, void *stream) {
  if (!sp) return fail(RTMI_ERR_INVALID, "null scene");
  if (const int rc = list_args(n, "negative path count n", "more than 2^31 - 1 paths n", d_list, n_list)) return rc;
  const bool work = n > 0 && n_list > 0;
  if (work && !(d_o && d_d && d_occluded)) return fail(RTMI_ERR_INVALID, "null d_origins, d_dirs or d_occluded");
  const Scene *s = S(sp);
  int n_cu;
  if (const int rc = list_scene(s, work, &n_cu)) return rc;
  if (!work) return RTMI_OK;
  float near_lo[3], near_hi[3], near_short;
  near_box(s, near_lo, near_hi, &near_short);
  const PathList list{d_list, d_count, (uint32_t)n_list};
  HIP_TRY(launch_occlusion(pick_query_variant(s->features), s->dev, near_lo, near_hi, near_short, n_cu, n, &list, d_o, d_d,
                           d_t_max, d_occluded, d_counts, d_check, (hipStream_t)stream));
  return RTMI_OK;
}

int rtmi_occluded_list(const rtmi_scene *s, int64_t n, const uint32_t *d_list, int64_t n_list, const uint32_t *d_count,
                       const float *d_origins, const float *d_dirs, const float *d_t_max, uint8_t *d_occluded,
                       unsigned long long *d_counts, void *stream) {
  return occluded_list(s, n, d_list, n_list, d_count, d_origins, d_dirs, d_t_max, d_occluded, d_counts, nullptr, stream);
}
#ifdef RTMI_CHECK_MARGINS
int rtmi_occluded_list_check_counts(const rtmi_scene *s, int64_t n, const uint32_t *d_list, int64_t n_list,
                                    const uint32_t *d_count, const float *d_origins, const float *d_dirs, const float *d_t_max,
                                    uint8_t *d_occluded, unsigned long long *d_counts, unsigned long long *d_check,
                                    void *stream) {
  return occluded_list(s, n, d_list, n_list, d_count, d_origins, d_dirs, d_t_max, d_occluded, d_counts, d_check, stream);
}
#endif

// ------------------------------------------------------------------ per-pixel sample budgets
// What the three entries below check of their frame, in the other entries' order: the arguments first, without a HIP call.
static int budget_frame(const rtmi_frame *f, bool arrays, const char *null_arrays, FrameDev *d) {
  if (!make_frame(f, d)) return fail(RTMI_ERR_INVALID, frame_why("bad frame"));
  if (d->items > 0 && !arrays) return fail(RTMI_ERR_INVALID, null_arrays);
  return RTMI_OK;
}

// rtmi_features -> FeatureBufs; false: the struct is not this library's (size) or its reserved word is set.
static bool feature_bufs(const rtmi_features *feat, FeatureBufs *fb) {
  static_assert(sizeof(rtmi_features) == 40, "rtmi_features is 40 bytes");
  *fb = FeatureBufs{};
  if (!feat) return true;
  if (feat->size != (int32_t)sizeof(rtmi_features) || feat->reserved != 0) return false;
  fb->albedo = feat->d_albedo, fb->normal = feat->d_normal, fb->depth = feat->d_depth, fb->coverage = feat->d_coverage;
  return true;
}
static const char *const kBadFeatures = "rtmi_features.size does not match this library, or reserved is not 0";

// rtmi_render_features, and with `direct` rtmi_render_direct: the same checks in the same order -- the light states' own
// among the arguments', before the scene is looked at -- and the DIRECT twins of the two kernels.
static int render_budget(const rtmi_scene *sp, const rtmi_frame *f, const uint32_t *d_budget, void *d_states, float *d_sum,
                         float *d_sq, uint32_t *d_samples, uint32_t *d_ray_counts, const rtmi_features *feat,
                         unsigned long long *d_work, void *stream, bool direct, void *d_light_states,
                         unsigned long long *d_counts) {
  if (!sp) return fail(RTMI_ERR_INVALID, "null scene");
  FeatureBufs fb;
  if (!feature_bufs(feat, &fb)) return fail(RTMI_ERR_INVALID, kBadFeatures);
  const bool features = fb.albedo || fb.normal || fb.depth || fb.coverage;
  FrameDev d;
  int rc = budget_frame(f, d_budget && d_states && d_sum && d_samples && d_work,
                        "null budget, state, sum, sample-count or work array", &d);
  if (rc) return rc;
  if (direct && d.items > 0 && !d_light_states) return fail(RTMI_ERR_INVALID, "null light state array");
  if (direct && d_light_states && d_light_states == d_states)
    return fail(RTMI_ERR_INVALID, "d_light_states must not be d_states: a path's draws and its light draws are two streams");
  // (before the scene is looked at: max_depth is the frame's, and at depth 0 Trace never looks at the primary record)
  if (features && d.max_depth == 0)
    return fail(RTMI_ERR_DEPTH, "max_depth must be at least 1 with a feature buffer: at depth 0 Trace never looks at the primary hit");
  const Scene *s = S(sp);
  if (!s->committed) return fail(RTMI_ERR_INVALID, "scene not committed");
  if ((rc = check_depth(d.max_depth))) return rc;
  if (d.post) return fail(RTMI_ERR_INVALID, "post_process must be 0: per-pixel sample counts have no uniform division (rtmi_resolve)");
  // (spp caps one call's samples per pixel: a call's closest-hit queries of a pixel stay below 2^31 as a render's do)
  if ((rc = check_pixel_queries(d))) return rc;
  int n_cu = 0;
  if ((rc = scene_device(s, &n_cu))) return rc;
  hipStream_t st = (hipStream_t)stream;
  // the counter words start from zero; the argument block behind them is written by launch_budget
  HIP_TRY(hipMemsetAsync(d_work, 0, kCallParamsOffset, st));
  if (d.spp == 0) return RTMI_OK;  // (every budget is capped at 0: nothing to render)
  if (direct) {
    TraceDirectBufs dx{};
    dx.ld = s->ldev, dx.qd = s->qdev;
    dx.light_states = reinterpret_cast<uint32_t *>(d_light_states), dx.counts = d_counts;
    HIP_TRY(launch_budget_direct(pick_query_variant(s->features), s->dev, (s->features & F_TEX) != 0, s->sphere_lights, n_cu, d,
                                 d_budget, reinterpret_cast<uint32_t *>(d_states), dx, d_sum, d_sq, d_samples, d_ray_counts, &fb,
                                 d_work, st));
    return RTMI_OK;
  }
  HIP_TRY(launch_budget(pick_query_variant(s->features), s->dev, (s->features & F_TEX) != 0, n_cu, d, d_budget,
                        reinterpret_cast<uint32_t *>(d_states), d_sum, d_sq, d_samples, d_ray_counts, &fb, d_work, st));
  return RTMI_OK;
}

int rtmi_render_features(const rtmi_scene *sp, const rtmi_frame *f, const uint32_t *d_budget, void *d_states, float *d_sum,
                         float *d_sq, uint32_t *d_samples, uint32_t *d_ray_counts, const rtmi_features *feat,
                         unsigned long long *d_work, void *stream) {
  return render_budget(sp, f, d_budget, d_states, d_sum, d_sq, d_samples, d_ray_counts, feat, d_work, stream, false, nullptr, nullptr);
}

int rtmi_render_budget(const rtmi_scene *sp, const rtmi_frame *f, const uint32_t *d_budget, void *d_states, float *d_sum,
                       float *d_sq, uint32_t *d_samples, uint32_t *d_ray_counts, unsigned long long *d_work, void *stream) {
  return rtmi_render_features(sp, f, d_budget, d_states, d_sum, d_sq, d_samples, d_ray_counts, nullptr, d_work, stream);
}

// ------------------------------------------------------------------ the budget render with direct light
int rtmi_render_direct(const rtmi_scene *sp, const rtmi_frame *f, const rtmi_render_direct_args *p, void *stream) {
  static_assert(sizeof(rtmi_render_direct_args) == 88, "rtmi_render_direct_args is 88 bytes");
  if (!sp) return fail(RTMI_ERR_INVALID, "null scene");
  if (!p) return fail(RTMI_ERR_INVALID, "null rtmi_render_direct_args");
  if (p->size != (int32_t)sizeof(rtmi_render_direct_args) || p->reserved != 0)
    return fail(RTMI_ERR_INVALID, "rtmi_render_direct_args.size does not match this library, or reserved is not 0");
  return render_budget(sp, f, p->d_budget, p->d_states, p->d_sum, p->d_sq, p->d_samples, p->d_ray_counts, p->features, p->d_work,
                       stream, true, p->d_light_states, p->d_counts);
}

int rtmi_resolve_features(const rtmi_frame *f, const rtmi_features *sums, const uint32_t *d_samples,
                          const rtmi_features *out, void *stream) {
  FrameDev d;
  const int rc = budget_frame(f, sums && out && d_samples, "null feature sums, sample-count array or output struct", &d);
  if (rc) return rc;
  FeatureBufs in, to;
  if (!feature_bufs(sums, &in) || !feature_bufs(out, &to)) return fail(RTMI_ERR_INVALID, kBadFeatures);
  if ((to.albedo && !in.albedo) || (to.normal && !in.normal) || (to.depth && !in.depth) ||
      ((to.depth || to.coverage) && !in.coverage))
    return fail(RTMI_ERR_INVALID, "an output feature buffer without its sums (depth and alpha also need the coverage sums)");
  if (d.items == 0) return RTMI_OK;
  HIP_TRY(launch_resolve_features(d, in, d_samples, to, (hipStream_t)stream));
  return RTMI_OK;
}

int rtmi_budget_plan(const rtmi_frame *f, const rtmi_adaptive_opts *o, const float *d_sum, const float *d_sq,
                     const uint32_t *d_samples, uint32_t *d_budget, unsigned long long *d_totals, void *stream) {
  FrameDev d;
  const int rc = budget_frame(f, d_sum && d_sq && d_samples && d_budget && d_totals,
                              "null sum, second-moment, sample-count, budget or totals array", &d);
  if (rc) return rc;
  if (!o) return fail(RTMI_ERR_INVALID, "null rtmi_adaptive_opts");
  if (o->size != (int32_t)sizeof(rtmi_adaptive_opts)) return fail(RTMI_ERR_INVALID, "rtmi_adaptive_opts.size does not match this library");
  if (o->min_samples < 2 || o->max_samples < o->min_samples || o->step < 1 || !(o->tolerance > 0.f) ||
      !std::isfinite(o->tolerance) || !(o->floor >= 0.f) || !std::isfinite(o->floor))
    return fail(RTMI_ERR_INVALID, "rtmi_adaptive_opts field out of range (min_samples >= 2, max_samples >= min_samples, step >= 1, "
                                  "finite tolerance > 0, finite floor >= 0)");
  HIP_TRY(launch_budget_plan(d, o->min_samples, o->max_samples, o->step, o->tolerance, o->floor, d_sum, d_sq, d_samples,
                             d_budget, d_totals, (hipStream_t)stream));
  return RTMI_OK;
}

int rtmi_resolve(const rtmi_frame *f, const float *d_sum, const uint32_t *d_samples, int post_process, float *d_tiles,
                 void *stream) {
  FrameDev d;
  const int rc = budget_frame(f, d_sum && d_samples && d_tiles, "null sum, sample-count or tile array", &d);
  if (rc) return rc;
  HIP_TRY(launch_resolve(d, d_sum, d_samples, post_process, d_tiles, (hipStream_t)stream));
  return RTMI_OK;
}

int rtmi_resolve_variance(const rtmi_frame *f, const float *d_sum, const float *d_sq, const uint32_t *d_samples, float *d_var,
                          void *stream) {
  FrameDev d;
  const int rc = budget_frame(f, d_sum && d_sq && d_samples && d_var, "null sum, second-moment, sample-count or variance array", &d);
  if (rc) return rc;
  HIP_TRY(launch_resolve_variance(d, d_sum, d_sq, d_samples, d_var, (hipStream_t)stream));
  return RTMI_OK;
}

// ------------------------------------------------------------------ camera rays
// u, v, w finite and orthonormal, in binary64: | |x|^2 - 1 | <= 1e-3 each, |dot| <= 1e-3 pairwise.  A camera installed by
// rtmi_camera_raw (or rtmi_camera_set with no frame) carries none.
static bool camera_frame_orthonormal(const V3 &u, const V3 &v, const V3 &w) {
  const double a[3][3] = {{u.x, u.y, u.z}, {v.x, v.y, v.z}, {w.x, w.y, w.z}};
  for (int i = 0; i < 3; i++)
    for (int j = i; j < 3; j++) {
      const double dot = a[i][0] * a[j][0] + a[i][1] * a[j][1] + a[i][2] * a[j][2];
      if (!(std::fabs(dot - (i == j ? 1.0 : 0.0)) <= 1e-3)) return false;  // (a NaN or an infinity fails)
    }
  return true;
}

// What rtmi_camera_rays and rtmi_path_advance check of their projection on scene s, without a HIP call.
static int check_projection(const rtmi_projection *proj, const Scene *s, int *kind_out, float *fov_out) {
  static_assert(sizeof(rtmi_projection) == 16, "rtmi_projection is 16 bytes");
  int kind = RTMI_PROJ_CAMERA;
  float fov = 0.f;
  if (proj) {
    if (proj->size != (int32_t)sizeof(rtmi_projection) || proj->reserved != 0)
      return fail(RTMI_ERR_INVALID, "rtmi_projection.size does not match this library, or reserved is not 0");
    if (proj->kind < RTMI_PROJ_CAMERA || proj->kind > RTMI_PROJ_FISHEYE)
      return fail(RTMI_ERR_INVALID, "rtmi_projection.kind is not one of RTMI_PROJ_*");
    kind = proj->kind, fov = proj->fov;
    // (2 pi as the binary32 nearest to it, which lies above: the fov a caller writes as (float)(2 * M_PI) is accepted)
    if (kind == RTMI_PROJ_FISHEYE && !(std::isfinite(fov) && fov > 0.f && fov <= 6.283185307179586f))
      return fail(RTMI_ERR_INVALID, "rtmi_projection.fov of a fisheye must be finite, above 0 and at most 2 pi");
  }
  if (kind != RTMI_PROJ_CAMERA && !(s->has_camera && camera_frame_orthonormal(s->cam.u, s->cam.v, s->cam_w)))
    return fail(RTMI_ERR_INVALID, "this projection needs a camera whose u, v, w are finite and orthonormal "
                                  "(rtmi_camera_raw installs none)");
  *kind_out = kind, *fov_out = fov;
  return RTMI_OK;
}

int rtmi_camera_rays(const rtmi_scene *sp, const rtmi_frame *f, const rtmi_projection *proj, const uint32_t *d_budget,
                     uint32_t sample, void *d_states, float *d_origins, float *d_dirs, void *stream) {
  if (!sp) return fail(RTMI_ERR_INVALID, "null scene");
  FrameDev d;
  int rc = budget_frame(f, d_states && d_origins && d_dirs, "null state, origin or direction array", &d);
  if (rc) return rc;
  int kind = RTMI_PROJ_CAMERA;
  float fov = 0.f;
  const Scene *s = S(sp);
  if ((rc = check_projection(proj, s, &kind, &fov))) return rc;
  if (!s->committed) return fail(RTMI_ERR_INVALID, "scene not committed");
  if ((rc = scene_device(s, nullptr))) return rc;
  // the camera is the scene's host record now, by value: a later rtmi_camera_update does not reach this launch
  const float w[3] = {s->cam_w.x, s->cam_w.y, s->cam_w.z};
  HIP_TRY(launch_camera_rays(d, s->dev.cam, w, kind, fov, d_budget, sample, reinterpret_cast<uint32_t *>(d_states), d_origins,
                             d_dirs, (hipStream_t)stream));
  return RTMI_OK;
}

int rtmi_sample_add(const rtmi_frame *f, const uint32_t *d_budget, uint32_t sample, const float *d_radiance,
                    const uint32_t *d_trace_counts, float *d_sum, float *d_sq, uint32_t *d_samples, uint32_t *d_ray_counts,
                    void *stream) {
  FrameDev d;
  const int rc = budget_frame(f, d_radiance && d_sum && d_samples, "null radiance, sum or sample-count array", &d);
  if (rc) return rc;
  HIP_TRY(launch_sample_add(d, d_budget, sample, d_radiance, d_trace_counts, d_sum, d_sq, d_samples, d_ray_counts,
                            (hipStream_t)stream));
  return RTMI_OK;
}

// ------------------------------------------------------------------ ended paths finished and refilled in place
// The arguments first, without a HIP call, then the scene's device (as rtmi_camera_rays and rtmi_bounce_list refuse).
int rtmi_path_advance(const rtmi_scene *sp, const rtmi_frame *f, const rtmi_path_advance_args *a, void *stream) {
  static_assert(sizeof(rtmi_path_advance_args) == 160, "rtmi_path_advance_args is 160 bytes");
  if (!sp) return fail(RTMI_ERR_INVALID, "null scene");
  FrameDev d;
  if (!make_frame(f, &d)) return fail(RTMI_ERR_INVALID, frame_why("bad frame"));
  if (!a) return fail(RTMI_ERR_INVALID, "null rtmi_path_advance_args");
  if (a->size != (int32_t)sizeof(rtmi_path_advance_args) || a->reserved != 0)
    return fail(RTMI_ERR_INVALID, "rtmi_path_advance_args.size does not match this library, or reserved is not 0");
  const Scene *s = S(sp);
  int kind = RTMI_PROJ_CAMERA;
  float fov = 0.f;
  int rc = check_projection(a->proj, s, &kind, &fov);
  if (rc) return rc;
  if (d.post) return fail(RTMI_ERR_INVALID, "post_process must be 0: per-pixel sample counts have no uniform division (rtmi_resolve)");
  if ((rc = check_depth(d.max_depth))) return rc;
  if ((rc = check_list(d.items, a->d_list, a->n_list))) return rc;
  if (a->n_list > 0 && !(a->d_origins && a->d_dirs && a->d_states && a->d_steps && a->d_emitted && a->d_attenuation &&
                         a->d_cursor && a->d_sum && a->d_samples))
    return fail(RTMI_ERR_INVALID, "null ray, state, step, emitted, attenuation, cursor, sum or sample-count array");
  if (a->n_list > 0 && d.max_depth > 0 && !(a->d_emitted_stack && a->d_attenuation_stack))
    return fail(RTMI_ERR_INVALID, "null emitted or attenuation stack with max_depth > 0");
  const bool work = d.items > 0 && a->n_list > 0;
  int n_cu;
  if ((rc = list_scene(s, work, &n_cu))) return rc;
  if (!work) return RTMI_OK;
  AdvanceCall c{};
  c.budget = a->d_budget, c.list = {a->d_list, a->d_count, (uint32_t)a->n_list};
  c.origins = a->d_origins, c.dirs = a->d_dirs, c.states = reinterpret_cast<uint32_t *>(a->d_states), c.steps = a->d_steps;
  c.emitted = a->d_emitted, c.attenuation = a->d_attenuation;
  c.emitted_stack = a->d_emitted_stack, c.attenuation_stack = a->d_attenuation_stack, c.cursor = a->d_cursor;
  c.sum = a->d_sum, c.sq = a->d_sq, c.samples = a->d_samples, c.ray_counts = a->d_ray_counts, c.counts = a->d_counts;
  // the camera is the scene's host record now, by value: a later rtmi_camera_update does not reach this launch
  const float w[3] = {s->cam_w.x, s->cam_w.y, s->cam_w.z};
  HIP_TRY(launch_path_advance(d, s->dev.cam, w, kind, fov, c, n_cu, (hipStream_t)stream));
  return RTMI_OK;
}

// ------------------------------------------------------------------ denoise
static bool denoise_extent(int height, int width) {
  return height >= 1 && height <= RTMI_MAX_EXTENT && width >= 1 && width <= RTMI_MAX_EXTENT;
}

size_t rtmi_denoise_scratch_bytes(int height, int width) {
  return denoise_extent(height, width) ? denoise_scratch_bytes(height, width) : 0;
}

int rtmi_denoise(int height, int width, const rtmi_denoise_opts *o, const float *d_color, const rtmi_denoise_guides *g,
                 float *d_out, float *d_out_variance, void *d_scratch, size_t scratch_bytes, void *stream) {
  static_assert(sizeof(rtmi_denoise_opts) == 24 && sizeof(rtmi_denoise_guides) == 48, "the denoise structs' sizes");
  if (!denoise_extent(height, width)) return fail(RTMI_ERR_INVALID, "height and width must be within 1..65535 (RTMI_MAX_EXTENT)");
  if (!o || !g || !d_color || !d_out || !d_scratch)
    return fail(RTMI_ERR_INVALID, "null rtmi_denoise_opts, rtmi_denoise_guides, colour, output or scratch");
  if (o->size != (int32_t)sizeof(rtmi_denoise_opts)) return fail(RTMI_ERR_INVALID, "rtmi_denoise_opts.size does not match this library");
  if (g->size != (int32_t)sizeof(rtmi_denoise_guides) || g->reserved != 0)
    return fail(RTMI_ERR_INVALID, "rtmi_denoise_guides.size does not match this library, or reserved is not 0");
  if (o->iterations < 1 || o->iterations > 8 || o->normal_squarings < 0 || o->normal_squarings > 8 ||
      (o->demodulate != 0 && o->demodulate != 1) || !(o->sigma_color > 0.f) || !std::isfinite(o->sigma_color) ||
      !(o->sigma_depth > 0.f) || !std::isfinite(o->sigma_depth))
    return fail(RTMI_ERR_INVALID, "rtmi_denoise_opts field out of range (iterations 1..8, normal_squarings 0..8, demodulate 0/1, "
                                  "finite sigma_color > 0, finite sigma_depth > 0)");
  if (!g->d_variance || !g->d_normal || !g->d_depth || !g->d_alpha || (o->demodulate && !g->d_albedo))
    return fail(RTMI_ERR_INVALID, "null guide: variance, normal, depth and alpha are required, albedo with demodulate");
  if (scratch_bytes < denoise_scratch_bytes(height, width))
    return fail(RTMI_ERR_INVALID, "scratch_bytes is smaller than rtmi_denoise_scratch_bytes(height, width)");
  DenoiseCall d{};
  d.height = height, d.width = width, d.iterations = o->iterations, d.normal_squarings = o->normal_squarings;
  d.demodulate = o->demodulate, d.sigma_color = o->sigma_color, d.sigma_depth = o->sigma_depth;
  d.color = d_color, d.variance = g->d_variance, d.albedo = o->demodulate ? g->d_albedo : nullptr, d.normal = g->d_normal;
  d.depth = g->d_depth, d.alpha = g->d_alpha, d.out = d_out, d.out_variance = d_out_variance, d.scratch = d_scratch;
  HIP_TRY(launch_denoise(d, (hipStream_t)stream));
  return RTMI_OK;
}

// ------------------------------------------------------------------ accumulate
size_t rtmi_history_bytes(int height, int width) { return denoise_extent(height, width) ? history_bytes(height, width) : 0; }

int rtmi_accumulate(int height, int width, const rtmi_accumulate_opts *o, const float *d_color, const rtmi_denoise_guides *g,
                    const float cur_camera[21], const void *d_history_in, const float prev_camera[21], void *d_history_out,
                    float *d_out, float *d_out_variance, float *d_out_length, void *stream) {
  static_assert(sizeof(rtmi_accumulate_opts) == 20, "rtmi_accumulate_opts is 20 bytes");
  if (!denoise_extent(height, width)) return fail(RTMI_ERR_INVALID, "height and width must be within 1..65535 (RTMI_MAX_EXTENT)");
  if (!o || !g || !d_color || !cur_camera || !d_history_out || !d_out)
    return fail(RTMI_ERR_INVALID, "null rtmi_accumulate_opts, rtmi_denoise_guides, colour, camera, output history or output");
  if (o->size != (int32_t)sizeof(rtmi_accumulate_opts) || o->reserved != 0)
    return fail(RTMI_ERR_INVALID, "rtmi_accumulate_opts.size does not match this library, or reserved is not 0");
  if (g->size != (int32_t)sizeof(rtmi_denoise_guides) || g->reserved != 0)
    return fail(RTMI_ERR_INVALID, "rtmi_denoise_guides.size does not match this library, or reserved is not 0");
  if (!std::isfinite(o->normal_min) || o->normal_min < -1.f || o->normal_min > 1.f || !std::isfinite(o->depth_tolerance) ||
      !(o->depth_tolerance > 0.f) || !(o->min_blend >= 0.f && o->min_blend <= 1.f))
    return fail(RTMI_ERR_INVALID, "rtmi_accumulate_opts field out of range (finite normal_min in -1..1, finite depth_tolerance > 0, "
                                  "min_blend in 0..1)");
  if (!g->d_variance || !g->d_normal || !g->d_depth || !g->d_alpha)
    return fail(RTMI_ERR_INVALID, "null guide: variance, normal, depth and alpha are required");
  if ((d_history_in == nullptr) != (prev_camera == nullptr))
    return fail(RTMI_ERR_INVALID, "d_history_in and prev_camera go together: both null (the first frame) or neither");
  if (((uintptr_t)d_history_in | (uintptr_t)d_history_out) & 15u)
    return fail(RTMI_ERR_INVALID, "a history must be 16-byte aligned");
  if (!all_finite(cur_camera, 21) || (prev_camera && !all_finite(prev_camera, 21)))
    return fail(RTMI_ERR_INVALID, "non-finite camera float");
  AccumulateCall c{};
  c.height = height, c.width = width;
  c.normal_min = o->normal_min, c.depth_tolerance = o->depth_tolerance, c.min_blend = o->min_blend;
  for (int k = 0; k < 3; k++) {
    c.p[k] = cur_camera[k], c.h[k] = cur_camera[6 + k], c.v[k] = cur_camera[9 + k];
    c.e[k] = (float)((double)cur_camera[3 + k] - (double)cur_camera[k]);
  }
  if (prev_camera) {
    // the inverse of the matrix whose columns are a = h', b = v', c = llc' - p', in binary64: its rows are b x c, c x a and
    // a x b over the determinant
    double a[3], b[3], cc[3];
    for (int k = 0; k < 3; k++)
      a[k] = prev_camera[6 + k], b[k] = prev_camera[9 + k], cc[k] = (double)prev_camera[3 + k] - (double)prev_camera[k];
    const auto cross = [](const double *x, const double *y, double *out) {
      out[0] = x[1] * y[2] - x[2] * y[1], out[1] = x[2] * y[0] - x[0] * y[2], out[2] = x[0] * y[1] - x[1] * y[0];
    };
    double rows[3][3];
    cross(b, cc, rows[0]), cross(cc, a, rows[1]), cross(a, b, rows[2]);
    const double det = (a[0] * rows[0][0] + a[1] * rows[0][1]) + a[2] * rows[0][2];
    if (det == 0.0 || !std::isfinite(det)) return fail(RTMI_ERR_INVALID, "prev_camera is singular: its h, v and llc - p span no volume");
    for (int r = 0; r < 3; r++)
      for (int k = 0; k < 3; k++) c.r[r][k] = (float)(rows[r][k] / det);
    for (int k = 0; k < 3; k++) c.prev_p[k] = prev_camera[k];
  }
  c.color = d_color, c.variance = g->d_variance, c.normal = g->d_normal, c.depth = g->d_depth, c.alpha = g->d_alpha;
  c.history_in = d_history_in, c.history_out = d_history_out;
  c.out = d_out, c.out_variance = d_out_variance, c.out_length = d_out_length;
  HIP_TRY(launch_accumulate(c, (hipStream_t)stream));
  return RTMI_OK;
}

int rtmi_render_status(const rtmi_scene *sp, const void *d_scratch, uint64_t *out_rays, void *stream) {
  if (!sp) return fail(RTMI_ERR_INVALID, "null argument");
  const Scene *s = S(sp);
  if (!s->committed) return fail(RTMI_ERR_INVALID, "scene not committed");
  const unsigned long long *counters = d_scratch ? reinterpret_cast<const unsigned long long *>(d_scratch) : s->d_counters;
  unsigned long long v[2] = {0, 0};  // [0] rays, [1] abandoned mesh searches (must be 0)
  HIP_TRY(hipMemcpyAsync(v, counters + 1, sizeof(v), hipMemcpyDeviceToHost, (hipStream_t)stream));
  HIP_TRY(hipStreamSynchronize((hipStream_t)stream));
  if (out_rays) *out_rays = v[0];
  if (v[1] != 0) return fail(RTMI_ERR_INTERNAL, "mesh search stack overflow: the frame is incomplete");
  return RTMI_OK;
}

int rtmi_last_ray_total(const rtmi_scene *sp, uint64_t *out_rays, void *stream) {
  if (!out_rays) return fail(RTMI_ERR_INVALID, "null argument");
  return rtmi_render_status(sp, nullptr, out_rays, stream);
}

// Diagnostic: the raw counter words of the most recent render (RTMI_STATS builds fill words 4..32).
int rtmi_debug_counters(const rtmi_scene *sp, unsigned long long out[RTMI_COUNTER_WORDS], void *stream) {
  return rtmi_debug_counters_ex(sp, nullptr, out, stream);
}
int rtmi_debug_counters_ex(const rtmi_scene *sp, const void *d_scratch, unsigned long long out[RTMI_COUNTER_WORDS],
                           void *stream) {
  if (!sp || !out) return fail(RTMI_ERR_INVALID, "null argument");
  const Scene *s = S(sp);
  if (!s->committed) return fail(RTMI_ERR_INVALID, "scene not committed");
  const unsigned long long *counters = d_scratch ? reinterpret_cast<const unsigned long long *>(d_scratch) : s->d_counters;
  HIP_TRY(hipMemcpyAsync(out, counters, kCounterBytes, hipMemcpyDeviceToHost, (hipStream_t)stream));
  HIP_TRY(hipStreamSynchronize((hipStream_t)stream));
  return RTMI_OK;
}

// Diagnostic: where the regions of a frame's render scratch lie (scratch_layout, in ScratchLayout's order).  Host only.
int rtmi_debug_scratch_regions(const rtmi_frame *f, int64_t out[], int n) {
  FrameDev d;
  if (!f || !out || n < 0) return fail(RTMI_ERR_INVALID, "null argument");
  if (!make_frame(f, &d)) return fail(RTMI_ERR_INVALID, frame_why("bad frame"));
  const ScratchLayout l = scratch_layout(d);
  const size_t at[RTMI_SCRATCH_REGIONS] = {l.states, l.rays,   l.cost, l.order, l.meta, l.head,   l.work,     l.qcost,  l.qsorted,
                                           l.qmap,   l.qmax,   l.fut,  l.next,  l.claims, l.first, l.prio_tab, l.params, l.total};
  static_assert(sizeof(ScratchLayout) == sizeof(at), "rtmi_debug_scratch_regions reports every region of ScratchLayout");
  for (int i = 0; i < n && i < RTMI_SCRATCH_REGIONS; i++) out[i] = (int64_t)at[i];
  return RTMI_OK;
}

// Diagnostic: the scheduler step of a scheduled render (schedule_step) on the caller's own counts, into the regions of
// the caller's scratch.  Asynchronous on `stream`.
int rtmi_debug_schedule(const rtmi_frame *f, void *d_scratch, size_t scratch_bytes, uint32_t *d_ray_counts,
                        const uint32_t *d_work_counts, int pixel_head, uint32_t sparse_cap, int grid_waves, int outlier_x10,
                        const int32_t head_pct[3], int simds, int rounds, int spp, int probe_spp, void *stream) {
  FrameDev d;
  if (!f || !d_scratch || !d_ray_counts || !head_pct) return fail(RTMI_ERR_INVALID, "null argument");
  if (!make_frame(f, &d)) return fail(RTMI_ERR_INVALID, frame_why("bad frame"));
  const ScratchLayout sl = scratch_layout(d);
  if (scratch_bytes < sl.total) return fail(RTMI_ERR_INVALID, "scratch_bytes < rtmi_render_scratch_bytes(frame)");
  for (int i = 0; i < 3; i++)
    if (head_pct[i] < 0 || head_pct[i] > 100) return fail(RTMI_ERR_INVALID, "head_pct outside [0, 100]");
  if (!(head_pct[0] >= head_pct[1] && head_pct[1] >= head_pct[2]))
    return fail(RTMI_ERR_INVALID, "head_pct must not increase from the heaviest class to the lightest");
  if (grid_waves < 0 || outlier_x10 < 0 || simds < 0 || rounds < 0) return fail(RTMI_ERR_INVALID, "negative argument");
  if ((int64_t)simds * rounds > kMaxChains) return fail(RTMI_ERR_INVALID, "simds * rounds above the chain cap (32768)");
  if ((int64_t)simds * rounds > 0 && (spp < 1 || probe_spp < 1)) return fail(RTMI_ERR_INVALID, "a chain plan needs spp and probe_spp of at least 1");
  if (rtmi_device_count() <= 0) return fail(RTMI_ERR_NO_DEVICE, "no HIP device: librtmi has no CPU fallback");
  const int pct[3] = {head_pct[0], head_pct[1], head_pct[2]};
  SchedStep k;
  k.tiles = d.local_tiles, k.pixel_head = pixel_head != 0;
  k.sparse_cap = sparse_cap, k.waves = grid_waves, k.outlier_x10 = outlier_x10, k.head_pct = pct;
  k.simds = simds, k.rounds = rounds, k.spp = spp, k.probe_spp = probe_spp;
  SchedPlan plan;
  return schedule_step(scratch_regions(d_scratch, sl), d_ray_counts, d_work_counts, k, &plan, (hipStream_t)stream);
}

#ifdef RTMI_STATS
// diagnostic builds only (not declared in rtmi.h): per-wave cycle records of the last render
int rtmi_debug_wave_stats(unsigned long long *out, size_t bytes) {
  HIP_TRY(hipDeviceSynchronize());
  HIP_TRY(rtmi::copy_wave_stats(out, bytes));
  return RTMI_OK;
}
#endif

// ------------------------------------------------------------------ exchange
// RCCL is not a link-time dependency of this library: the caller owns the communicator, so its RCCL is already
// in the process (a second copy must not be pulled in next to e.g. the one PyTorch bundles).  The four entry points
// are taken from the process image, or from librccl.so.1 when nothing has loaded it yet.
extern "C++" {
namespace {
struct Rccl {
  decltype(&ncclGroupStart) group_start = nullptr;
  decltype(&ncclGroupEnd) group_end = nullptr;
  decltype(&ncclSend) send = nullptr;
  decltype(&ncclRecv) recv = nullptr;
  decltype(&ncclReduce) reduce = nullptr;
  decltype(&ncclGetErrorString) err = nullptr;
  decltype(&ncclCommCount) count = nullptr;
  bool ok = false;
};
const Rccl &rccl() {
  static const Rccl r = [] {
    Rccl x;
    // "already in the process" and "the handle to look symbols up in" are two things: RTLD_DEFAULT is a null handle
    // on glibc, so a found symbol must not be mistaken for a failed dlopen (which once pulled a SECOND copy of RCCL
    // in next to the one the caller's communicator came from)
    const bool in_process = dlsym(RTLD_DEFAULT, "ncclSend") != nullptr;
    void *h = RTLD_DEFAULT;
    if (!in_process) {
      h = dlopen("librccl.so.1", RTLD_NOW | RTLD_GLOBAL);
      if (!h) h = dlopen("librccl.so", RTLD_NOW | RTLD_GLOBAL);
      if (!h) return x;
    }
    x.group_start = reinterpret_cast<decltype(x.group_start)>(dlsym(h, "ncclGroupStart"));
    x.group_end = reinterpret_cast<decltype(x.group_end)>(dlsym(h, "ncclGroupEnd"));
    x.send = reinterpret_cast<decltype(x.send)>(dlsym(h, "ncclSend"));
    x.recv = reinterpret_cast<decltype(x.recv)>(dlsym(h, "ncclRecv"));
    x.reduce = reinterpret_cast<decltype(x.reduce)>(dlsym(h, "ncclReduce"));
    x.err = reinterpret_cast<decltype(x.err)>(dlsym(h, "ncclGetErrorString"));
    x.count = reinterpret_cast<decltype(x.count)>(dlsym(h, "ncclCommCount"));
    x.ok = x.group_start && x.group_end && x.send && x.recv && x.reduce;
    return x;
  }();
  return r;
}
int rccl_fail(const Rccl &R, ncclResult_t e, const char *what) {
  return fail(RTMI_ERR_HIP, std::string(what) + ": " + (R.err ? R.err(e) : "RCCL error"));
}
}  // namespace
}  // extern "C++"
#define RCCL_TRY(expr)                                        \
  do {                                                        \
    ncclResult_t e__ = (expr);                                \
    if (e__ != ncclSuccess) return rccl_fail(R, e__, #expr);  \
  } while (0)

int rtmi_gather(void *nccl_comm, const rtmi_frame *f, const float *d_tiles, float *d_all_tiles, int root, void *stream) {
  FrameDev d;
  if (!make_frame(f, &d) || !d_tiles || root < 0 || root >= d.world) return fail(RTMI_ERR_INVALID, frame_why("bad gather arguments"));
  if (d.rank == root && !d_all_tiles) return fail(RTMI_ERR_INVALID, "the root needs d_all_tiles");
  const size_t count = (size_t)d.items * 3;
  hipStream_t st = (hipStream_t)stream;
  if (d.rank == root && d_all_tiles + (size_t)root * count != d_tiles)
    HIP_TRY(hipMemcpyAsync(d_all_tiles + (size_t)root * count, d_tiles, count * sizeof(float), hipMemcpyDeviceToDevice, st));
  if (d.world == 1) return RTMI_OK;
  if (!nccl_comm) return fail(RTMI_ERR_INVALID, "world_size > 1 needs an RCCL communicator");
  const Rccl &R = rccl();
  if (!R.ok) return fail(RTMI_ERR_NO_DEVICE, "RCCL (librccl.so.1) is not available in this process");
  ncclComm_t comm = reinterpret_cast<ncclComm_t>(nccl_comm);
  // xGMI is point to point and every peer has a direct link to the root: one grouped round of sends, no ring.
  // A group that was opened is always closed, also when a send / recv inside it fails: the communicator must not be
  // left mid-group for the caller's next collective.
  RCCL_TRY(R.group_start());
  ncclResult_t first = ncclSuccess;
  const char *what = "";
  if (d.rank == root) {
    for (int r = 0; r < d.world && first == ncclSuccess; r++)
      if (r != root) first = R.recv(d_all_tiles + (size_t)r * count, count, ncclFloat, r, comm, st), what = "ncclRecv";
  } else {
    first = R.send(d_tiles, count, ncclFloat, root, comm, st), what = "ncclSend";
  }
  const ncclResult_t closed = R.group_end();
  if (first != ncclSuccess) return rccl_fail(R, first, what);
  if (closed != ncclSuccess) return rccl_fail(R, closed, "ncclGroupEnd");
  return RTMI_OK;
}

int rtmi_reduce_sum(void *nccl_comm, const rtmi_frame *f, float *d_tiles, int root, void *stream) {
  FrameDev d;
  if (!make_frame(f, &d) || !d_tiles || root < 0) return fail(RTMI_ERR_INVALID, frame_why("bad reduce arguments"));
  // In the reference's sample split every rank renders the WHOLE frame (utils.cu:189,216-221), so the frame says nothing
  // about how many ranks there are: the communicator does.  NULL = this rank is the only one, its sum is the sum.
  if (!nccl_comm) {
    if (root != 0) return fail(RTMI_ERR_INVALID, "reduce without a communicator is a single rank: root must be 0");
    return RTMI_OK;
  }
  const Rccl &R = rccl();
  if (!R.ok) return fail(RTMI_ERR_NO_DEVICE, "RCCL (librccl.so.1) is not available in this process");
  ncclComm_t comm = reinterpret_cast<ncclComm_t>(nccl_comm);
  if (R.count) {
    int n = 0;
    RCCL_TRY(R.count(comm, &n));
    if (root >= n) return fail(RTMI_ERR_INVALID, "reduce root is not a rank of the communicator");
  }
  RCCL_TRY(R.reduce(d_tiles, d_tiles, (size_t)d.items * 3, ncclFloat, ncclSum, root, comm, (hipStream_t)stream));
  return RTMI_OK;
}

int rtmi_untile(const rtmi_frame *f, const float *d_all_tiles, float *d_image, void *stream) {
  FrameDev d;
  if (!make_frame(f, &d) || !d_all_tiles || !d_image) return fail(RTMI_ERR_INVALID, frame_why("bad untile arguments"));
  HIP_TRY(launch_untile(d, d_all_tiles, d_image, (hipStream_t)stream));
  return RTMI_OK;
}
int rtmi_untile_u32(const rtmi_frame *f, const uint32_t *d_all, uint32_t *d_image, void *stream) {
  FrameDev d;
  if (!make_frame(f, &d) || !d_all || !d_image) return fail(RTMI_ERR_INVALID, frame_why("bad untile arguments"));
  HIP_TRY(launch_untile_u32(d, d_all, d_image, (hipStream_t)stream));
  return RTMI_OK;
}
int rtmi_post_process(float *d_image, int64_t n_pixels, int spp, void *stream) {
  if (!d_image || n_pixels < 0 || spp <= 0) return fail(RTMI_ERR_INVALID, "bad post_process arguments");
  HIP_TRY(launch_post(d_image, n_pixels * 3, spp, (hipStream_t)stream));
  return RTMI_OK;
}
int rtmi_get_workload(int rank, int world_size, int spp) {
  return spp / world_size + (int)(rank < (spp % world_size));  // utils.cu:111-113
}
int rtmi_selftest_arithmetic(unsigned long long *mismatches) {
  if (!mismatches) return fail(RTMI_ERR_INVALID, "mismatches == NULL");
  if (rtmi_device_count() <= 0) return fail(RTMI_ERR_NO_DEVICE, "no HIP device: librtmi has no CPU fallback");
  unsigned long long *d_bad = nullptr;
  HIP_TRY(hipMalloc(&d_bad, 8 * sizeof(unsigned long long)));
  hipError_t e = hipMemset(d_bad, 0, 8 * sizeof(unsigned long long));
  if (e == hipSuccess) e = launch_arithmetic_selftest(d_bad, nullptr);
  if (e == hipSuccess) e = hipMemcpy(mismatches, d_bad, 8 * sizeof(unsigned long long), hipMemcpyDeviceToHost);
  (void)hipFree(d_bad);
  HIP_TRY(e);
  return RTMI_OK;
}
int rtmi_set_schedule(int mode) {
  if (mode < 0 || mode > 2) return fail(RTMI_ERR_INVALID, "schedule mode must be 0 (image order), 1 (auto) or 2 (always longest-first)");
  (void)default_tuning();
  std::lock_guard<std::mutex> lk(g_tune_mu);
  g_tune.schedule = mode;
  return RTMI_OK;
}
int rtmi_set_launch(int blocks_per_cu, int threads_per_block) {
  if (blocks_per_cu < 0 || threads_per_block < 0 || (threads_per_block % 64) != 0 || threads_per_block > 512)
    return fail(RTMI_ERR_INVALID, "threads_per_block must be a multiple of 64, at most 512 (256 for scenes without meshes)");
  (void)default_tuning();
  std::lock_guard<std::mutex> lk(g_tune_mu);
  g_tune.blocks_per_cu = blocks_per_cu;
  g_tune.threads = threads_per_block;
  return RTMI_OK;
}

}  // extern "C"
