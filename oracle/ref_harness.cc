// REFERENCE HARNESS — TEST INFRASTRUCTURE ONLY.  Not part of the product path.
//
// C ABI over the reference's own translation units, compiled for the CPU (oracle/Makefile, target _ref/libref.so)
// against the stand-in headers of oracle/refshim/.  It mirrors the orc_* entry points that tests/oraclelib.py binds,
// so one scene program builds the same world on the oracle and on the reference, and tests/test_ref_parity.py
// compares the two bit for bit.  Nothing here computes: objects are made by the reference's constructors, queries go
// to the reference's Hit / Scatter / Emit / RayAt, random states come from its CudaRandomInit, and a frame is its
// PathTracing called once per pixel with the thread indices set.  TRACE_DEPTH_LIMIT (10), HitableList's capacity
// (1024) and BVHNode's leaf size (2048) are the reference's compile-time constants, so they are not parameters here.
//
// Objects live as long as their scene; what the reference itself allocates and never frees (a Parallelepiped's six
// parallelograms, BVH nodes) stays allocated, as it does in the reference.
#include <cuda_runtime.h>
#include <curand_kernel.h>

#include <cstdint>
#include <cstring>
#include <functional>
#include <vector>

#include "bvh.cuh"
#include "camera.cuh"
#include "dielectric.cuh"
#include "diffuse_light.cuh"
#include "hitable_list.cuh"
#include "lambertian.cuh"
#include "metal.cuh"
#include "parallelepiped.cuh"
#include "parallelogram.cuh"
#include "ray_tracing.cuh"
#include "sky.cuh"
#include "sphere.cuh"
#include "textures/constant_texture.cuh"
#include "textures/image_texture.cuh"
#include "triangle.cuh"
#include "utils.cuh"

namespace {

using glm::vec3;

// PathTracing's world for ref_render: counts the queries Trace issues for the pixel whose thread indices are set,
// then forwards to the real list.
struct CountingWorld : HitableList {
  HitableList *inner = nullptr;
  uint32_t *counts = nullptr;
  int width = 0;
  bool Hit(const Ray &ray, double t_from, double t_to, HitRecord *out) override {
    int i = threadIdx.x + blockDim.x * blockIdx.x;
    int j = threadIdx.y + blockDim.y * blockIdx.y;
    counts[i * width + j]++;
    return inner->Hit(ray, t_from, t_to, out);
  }
};

struct Scene {
  HitableList *world = new HitableList();
  Camera *camera = nullptr;
  std::vector<Texture *> textures;
  std::vector<Material *> materials;
  std::vector<HitableList *> open_lists;
  std::vector<std::function<void()>> deleters;
  template <typename T>
  T *own(T *p) {
    deleters.push_back([p] { delete p; });
    return p;
  }
  ~Scene() {
    for (auto it = deleters.rbegin(); it != deleters.rend(); ++it) (*it)();
    delete camera;
    delete world;
  }
};

Scene *S(void *s) { return static_cast<Scene *>(s); }
vec3 V(const float *p) { return vec3(p[0], p[1], p[2]); }
Material *M(void *s, int mat) { return mat < 0 ? nullptr : S(s)->materials[mat]; }

int add_mat(void *s, Material *m) {
  S(s)->materials.push_back(m);
  return (int)S(s)->materials.size() - 1;
}
int add_hit(void *s, Hitable *h) {
  HitableList *into = S(s)->open_lists.empty() ? S(s)->world : S(s)->open_lists.back();
  if (into->list_len() >= HitableList::kMaxHitables) return -1;
  into->Append(h);
  return 0;
}
int material_index(void *s, const Material *m) {
  for (size_t i = 0; i < S(s)->materials.size(); i++)
    if (S(s)->materials[i] == m) return (int)i;
  return -1;
}
void set_thread(int i, int j) {
  blockDim = dim3(8, 8);
  blockIdx = {(unsigned)i / 8, (unsigned)j / 8, 0};
  threadIdx = {(unsigned)i % 8, (unsigned)j % 8, 0};
}
void to_state(const uint32_t *c, curandState *st) {
  std::memset(st, 0, sizeof(*st));
  st->d = c[0];
  for (int k = 0; k < 5; k++) st->v[k] = c[1 + k];
}
void from_state(const curandState *st, uint32_t *c) {
  c[0] = st->d;
  for (int k = 0; k < 5; k++) c[1 + k] = st->v[k];
}

template <bool HasTexCoord>
int add_bvh(void *s, const float *faces, const float *uvs, int n, int mat) {
  typedef Face<HasTexCoord> F;
  F *f = static_cast<F *>(malloc(sizeof(F) * (size_t)(n > 0 ? n : 1)));
  S(s)->deleters.push_back([f] { free(f); });
  for (int i = 0; i < n; i++) {
    new (&f[i]) F();
    for (int j = 0; j < 3; j++) {
      f[i].position(j) = V(faces + (size_t)i * 9 + j * 3);
      if constexpr (HasTexCoord) f[i].tex_coord(j) = glm::vec2(uvs[(size_t)i * 6 + j * 2], uvs[(size_t)i * 6 + j * 2 + 1]);
    }
  }
  return add_hit(s, S(s)->own(new BVH<F, AABB>(f, n, M(s, mat))));
}

}  // namespace

extern "C" {

void *ref_scene_new(void) { return new Scene(); }
void ref_scene_free(void *s) { delete S(s); }

int ref_constant_texture(void *s, const float rgb[3]) {
  S(s)->textures.push_back(S(s)->own(new ConstantTexture(V(rgb))));
  return (int)S(s)->textures.size() - 1;
}
// rgba: h * w * 4 bytes, rows top to bottom.  Copied into a pitched allocation and wrapped by the reference's own
// CreateCudaTextureObj.
int ref_image_texture(void *s, const uint8_t *rgba, int h, int w) {
  uint8_t *buf = nullptr;
  size_t pitch = 0;
  cudaMallocPitch(&buf, &pitch, (size_t)w * 4, (size_t)h);
  cudaMemcpy2D(buf, pitch, rgba, (size_t)w * 4, (size_t)w * 4, (size_t)h, cudaMemcpyHostToDevice);
  cudaTextureObject_t obj = ImageTexture::CreateCudaTextureObj(buf, h, w, pitch);
  S(s)->deleters.push_back([buf, obj] {
    cudaDestroyTextureObject(obj);
    cudaFree(buf);
  });
  S(s)->textures.push_back(S(s)->own(new ImageTexture(obj)));
  return (int)S(s)->textures.size() - 1;
}
int ref_lambertian(void *s, const float rgb[3]) { return add_mat(s, S(s)->own(new Lambertian(V(rgb)))); }
int ref_lambertian_tex(void *s, int tex) { return add_mat(s, S(s)->own(new Lambertian(S(s)->textures[tex]))); }
int ref_metal(void *s, const float rgb[3], float fuzz) { return add_mat(s, S(s)->own(new Metal(V(rgb), fuzz))); }
int ref_dielectric(void *s, const float rgb[3], double index) {
  return add_mat(s, S(s)->own(new Dielectric(V(rgb), index)));
}
int ref_diffuse_light(void *s, int tex) { return add_mat(s, S(s)->own(new DiffuseLight(S(s)->textures[tex]))); }

int ref_list_begin(void *s) {
  HitableList *l = S(s)->own(new HitableList());
  if (add_hit(s, l) != 0) return -1;
  S(s)->open_lists.push_back(l);
  return 0;
}
int ref_list_end(void *s) {
  if (S(s)->open_lists.empty()) return -1;
  S(s)->open_lists.pop_back();
  return 0;
}
int ref_add_sphere(void *s, const float c[3], double r, int mat) {
  return add_hit(s, S(s)->own(new Sphere(V(c), r, M(s, mat))));
}
int ref_add_triangle(void *s, const float p[9], int mat) {
  vec3 q[3] = {V(p), V(p + 3), V(p + 6)};
  return add_hit(s, S(s)->own(new Triangle(q, M(s, mat))));
}
int ref_add_parallelogram(void *s, const float p[9], int mat) {
  vec3 q[3] = {V(p), V(p + 3), V(p + 6)};
  return add_hit(s, S(s)->own(new Parallelogram(q, M(s, mat))));
}
int ref_add_parallelepiped(void *s, const float p[12], int mat) {
  vec3 q[4] = {V(p), V(p + 3), V(p + 6), V(p + 9)};
  return add_hit(s, S(s)->own(new Parallelepiped(q, M(s, mat))));
}
typedef void (*ref_transform_fn)(const float in[3], float out[3], void *user);
int ref_add_parallelepiped_lengths(void *s, const float lengths[3], int mat, ref_transform_fn transform, void *user) {
  auto fn = [transform, user](vec3 p) -> vec3 {
    float in[3] = {p.x, p.y, p.z}, o[3];
    transform(in, o, user);
    return vec3(o[0], o[1], o[2]);
  };
  return add_hit(s, S(s)->own(new Parallelepiped(V(lengths), M(s, mat), fn)));
}
int ref_add_sky(void *s) { return add_hit(s, S(s)->own(new Sky())); }
// faces: n * 9 floats; uvs: n * 6 floats or NULL (Face<false>).  The face array is the BVH's own: it sorts it in place.
int ref_add_bvh(void *s, const float *faces, const float *uvs, int n, int mat) {
  return uvs ? add_bvh<true>(s, faces, uvs, n, mat) : add_bvh<false>(s, faces, uvs, n, mat);
}

static void set_camera(void *s, Camera *c) {
  delete S(s)->camera;
  S(s)->camera = c;
}
void ref_camera_pinhole(void *s, const float pos[3], const float look_at[3], const float up[3], double fov,
                        double aspect) {
  set_camera(s, new Camera(V(pos), V(look_at), V(up), fov, aspect));
}
void ref_camera_defocus(void *s, const float pos[3], const float look_at[3], const float up[3], double fov,
                        double aspect, double aperture, double focus) {
  set_camera(s, new Camera(V(pos), V(look_at), V(up), fov, aspect, aperture, focus));
}
void ref_camera_raw(void *s, const float pos[3], const float llc[3], const float horiz[3], const float vert[3]) {
  set_camera(s, new Camera(V(pos), V(llc), V(horiz), V(vert)));
}
// out: position, lower-left corner, horizontal, vertical (12 floats): the members the reference gives accessors for
void ref_camera_get(void *s, float out[12]) {
  const Camera *c = S(s)->camera;
  const vec3 vs[4] = {c->position(), c->lower_left_corner(), c->horizontal(), c->vertical()};
  for (int i = 0; i < 4; i++) out[i * 3] = vs[i].x, out[i * 3 + 1] = vs[i].y, out[i * 3 + 2] = vs[i].z;
}

// ------------------------------------------------------------------ RNG: utils.cu's CudaRandomInit and CudaRandomFloat
// states: n * 6 uint32 {d, v0..v4}, state i for pixel i, by one CudaRandomInit grid of 64-thread blocks (as Main does)
void ref_rng_init(uint64_t seed, uint32_t *states, int64_t n) {
  std::vector<curandState> st((size_t)n);
  REF_LAUNCH(CudaRandomInit, (unsigned)((n + 63) / 64), 64)(seed, st.data(), (int)n);
  for (int64_t i = 0; i < n; i++) from_state(&st[i], states + i * 6);
}
float ref_random_float(float mn, float mx, uint32_t *state) {
  curandState st;
  to_state(state, &st);
  float r = CudaRandomFloat(mn, mx, &st);
  from_state(&st, state);
  return r;
}

int ref_get_workload(int rank, int world_size, int spp) { return GetWorkload(rank, world_size, spp); }

// ------------------------------------------------------------------ probes
// world->Hit; returns the hit flag; out = {t, u, v, nx, ny, nz}.  The record starts zeroed, as the oracle's does, so a
// field a Hit leaves untouched (Sky writes only t and the material) compares equal.
int ref_probe_hit(void *s, const float o[3], const float d[3], double t_from, double t_to, double out[6],
                  int *out_mat) {
  Ray r(V(o), V(d));
  HitRecord rec;
  std::memset(&rec, 0, sizeof(rec));
  bool hit = S(s)->world->Hit(r, t_from, t_to, &rec);
  if (hit) {
    out[0] = rec.t, out[1] = rec.u, out[2] = rec.v;
    out[3] = rec.normal.x, out[4] = rec.normal.y, out[5] = rec.normal.z;
    if (out_mat) *out_mat = material_index(s, rec.material_ptr);
  }
  return hit ? 1 : 0;
}
// Material::Scatter, then Emit at the hit point, as Trace calls them (ray_tracing.cu).  Returns the scattered flag;
// out = {attenuation rgb, scattered origin xyz, scattered direction xyz, emitted rgb}; the first nine are written
// only where the ray scattered.
int ref_probe_scatter(void *s, int mat, const float o[3], const float d[3], double t, double u, double v,
                      const float n[3], uint32_t *state, float out[12]) {
  Ray r(V(o), V(d));
  HitRecord rec;
  std::memset(&rec, 0, sizeof(rec));
  rec.t = t, rec.u = u, rec.v = v;
  rec.normal = V(n);
  rec.material_ptr = M(s, mat);
  curandState st;
  to_state(state, &st);
  vec3 att;
  Ray nr;
  bool sc = rec.material_ptr->Scatter(r, rec, &st, &att, &nr);
  auto hit_point = r.position() + (float)rec.t * r.direction();
  vec3 em = rec.material_ptr->Emit(rec.u, rec.v, hit_point);
  from_state(&st, state);
  if (sc) {
    out[0] = att.x, out[1] = att.y, out[2] = att.z;
    out[3] = nr.position().x, out[4] = nr.position().y, out[5] = nr.position().z;
    out[6] = nr.direction().x, out[7] = nr.direction().y, out[8] = nr.direction().z;
  }
  out[9] = em.x, out[10] = em.y, out[11] = em.z;
  return sc ? 1 : 0;
}
void ref_probe_camera_ray(void *s, double x, double y, uint32_t *state, float out[6]) {
  curandState st;
  to_state(state, &st);
  Ray r = S(s)->camera->RayAt(x, y, &st);
  from_state(&st, state);
  out[0] = r.position().x, out[1] = r.position().y, out[2] = r.position().z;
  out[3] = r.direction().x, out[4] = r.direction().y, out[5] = r.direction().z;
}

// ------------------------------------------------------------------ render
// One frame, single-threaded: CudaRandomInit(seed) for every pixel; pixel 0's state replaced by state0 where given (a
// scene program may have drawn from it while it built the world); then PathTracing once per pixel with that pixel's
// thread indices in Main's 8 x 8 blocks.  out_rgb: h*w*3 floats; out_rays: h*w query counts; out_states: h*w*6.
// Returns the total number of queries.
uint64_t ref_render(void *s, int height, int width, int spp, int post, uint64_t seed, const uint32_t *state0,
                    float *out_rgb, uint32_t *out_rays, uint32_t *out_states) {
  const int n = height * width;
  std::vector<curandState> st((size_t)n);
  REF_LAUNCH(CudaRandomInit, (unsigned)((n + 63) / 64), 64)(seed, st.data(), n);
  if (state0) to_state(state0, &st[0]);
  std::vector<vec3> image((size_t)n);
  std::memset(out_rays, 0, sizeof(uint32_t) * (size_t)n);
  CountingWorld *cw = new CountingWorld();
  cw->inner = S(s)->world;
  cw->counts = out_rays;
  cw->width = width;
  for (int i = 0; i < height; i++)
    for (int j = 0; j < width; j++) {
      set_thread(i, j);
      PathTracing(cw, S(s)->camera, height, width, spp, post != 0, st.data(), image.data());
    }
  delete cw;
  uint64_t total = 0;
  for (int k = 0; k < n; k++) {
    out_rgb[k * 3] = image[k].x, out_rgb[k * 3 + 1] = image[k].y, out_rgb[k * 3 + 2] = image[k].z;
    from_state(&st[k], out_states + (size_t)k * 6);
    total += out_rays[k];
  }
  return total;
}

}  // extern "C"
