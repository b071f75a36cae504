// Stand-in for <cuda_runtime.h> in the CPU build of the reference (oracle/Makefile, _ref/libref.so): enough of the
// CUDA runtime's names for the reference's translation units to compile with g++ and run on one host thread per
// "CUDA thread".  Own code; nothing here is taken from the CUDA toolkit.
//
//  * __device__ / __host__ / __global__ expand to nothing (__inline__ is already a g++ keyword).
//  * threadIdx / blockIdx / blockDim / gridDim are thread_local objects; whoever calls a __global__ function sets them
//    (REF_LAUNCH below walks a whole grid; oracle/ref_harness.cc sets them per pixel).
//  * Device memory is host memory: cudaMalloc is malloc, cudaMemcpy is memcpy.
//  * CUDA declares its math functions for float and double in the global namespace, so <math.h> is included here, and
//    it adds overloads that the host library lacks: min / max, and pow with an int exponent (powif / powi: repeated
//    multiplication in the base's own type, where C++11's <cmath> would promote pow(float, int) to double).
//  * tex2D<float4> follows the CUDA programming guide's texture-fetching rules for the one descriptor the reference
//    builds (image_texture.cu): normalised coordinates, cudaFilterModePoint, cudaAddressModeWrap (the zeroed address
//    mode), cudaReadModeNormalizedFloat on 4 x 8-bit unsigned channels, pitched rows.
#pragma once
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#define __device__
#define __host__
#define __global__
#define __forceinline__ inline
#define __constant__
#define __shared__
#define __cudart_builtin__

// ------------------------------------------------------------------ built-in vector types and thread indices
struct uint3 {
  unsigned int x, y, z;
};
struct dim3 {
  unsigned int x, y, z;
  dim3(unsigned int vx = 1, unsigned int vy = 1, unsigned int vz = 1) : x(vx), y(vy), z(vz) {}
};
struct float4 {
  float x, y, z, w;
};
struct float2 {
  float x, y;
};

inline thread_local uint3 threadIdx = {0, 0, 0};
inline thread_local uint3 blockIdx = {0, 0, 0};
inline thread_local dim3 blockDim;
inline thread_local dim3 gridDim;

// ------------------------------------------------------------------ math overloads CUDA adds to the global namespace
inline float min(float a, float b) { return fminf(a, b); }
inline float max(float a, float b) { return fmaxf(a, b); }
inline double min(double a, double b) { return fmin(a, b); }
inline double max(double a, double b) { return fmax(a, b); }
inline int min(int a, int b) { return a < b ? a : b; }
inline int max(int a, int b) { return a < b ? b : a; }

namespace refshim {
// powif / powi: square-and-multiply in the base's type; a negative exponent takes the reciprocal at the end.
template <typename T>
inline T powi(T a, int b) {
  unsigned int e = b < 0 ? 0u - (unsigned int)b : (unsigned int)b;
  T r = 1;
  for (;;) {
    if (e & 1u) r *= a;
    e >>= 1;
    if (!e) break;
    a *= a;
  }
  return b < 0 ? 1 / r : r;
}
}  // namespace refshim
inline float pow(float a, int b) { return refshim::powi<float>(a, b); }
inline double pow(double a, int b) { return refshim::powi<double>(a, b); }

// ------------------------------------------------------------------ errors, memory, events
enum cudaError { cudaSuccess = 0, cudaErrorInvalidValue = 1, cudaErrorMemoryAllocation = 2 };
typedef cudaError cudaError_t;
inline cudaError_t cudaGetLastError() { return cudaSuccess; }
inline cudaError_t cudaPeekAtLastError() { return cudaSuccess; }
inline const char *cudaGetErrorString(cudaError_t e) { return e == cudaSuccess ? "no error" : "error"; }
inline cudaError_t cudaDeviceSynchronize() { return cudaSuccess; }
inline cudaError_t cudaSetDevice(int) { return cudaSuccess; }
inline cudaError_t cudaGetDeviceCount(int *n) {
  *n = 1;
  return cudaSuccess;
}

enum cudaMemcpyKind {
  cudaMemcpyHostToHost = 0,
  cudaMemcpyHostToDevice = 1,
  cudaMemcpyDeviceToHost = 2,
  cudaMemcpyDeviceToDevice = 3,
  cudaMemcpyDefault = 4
};
template <typename T>
inline cudaError_t cudaMalloc(T **p, size_t bytes) {
  *p = static_cast<T *>(malloc(bytes ? bytes : 1));
  return *p ? cudaSuccess : cudaErrorMemoryAllocation;
}
template <typename T>
inline cudaError_t cudaMallocPitch(T **p, size_t *pitch, size_t width_bytes, size_t height) {
  *pitch = (width_bytes + 511) / 512 * 512;
  return cudaMalloc(p, *pitch * height);
}
inline cudaError_t cudaFree(void *p) {
  free(p);
  return cudaSuccess;
}
inline cudaError_t cudaMemcpy(void *dst, const void *src, size_t bytes, cudaMemcpyKind) {
  memcpy(dst, src, bytes);
  return cudaSuccess;
}
inline cudaError_t cudaMemcpy2D(void *dst, size_t dpitch, const void *src, size_t spitch, size_t width_bytes,
                                size_t height, cudaMemcpyKind) {
  for (size_t r = 0; r < height; r++) memcpy((char *)dst + r * dpitch, (const char *)src + r * spitch, width_bytes);
  return cudaSuccess;
}
inline cudaError_t cudaMemset(void *p, int v, size_t bytes) {
  memset(p, v, bytes);
  return cudaSuccess;
}

typedef struct refshim_event {
  int unused;
} *cudaEvent_t;
inline cudaError_t cudaEventCreate(cudaEvent_t *e) {
  *e = nullptr;
  return cudaSuccess;
}
inline cudaError_t cudaEventRecord(cudaEvent_t, void * = nullptr) { return cudaSuccess; }
inline cudaError_t cudaEventSynchronize(cudaEvent_t) { return cudaSuccess; }
inline cudaError_t cudaEventElapsedTime(float *ms, cudaEvent_t, cudaEvent_t) {
  *ms = 0.f;
  return cudaSuccess;
}
inline cudaError_t cudaEventDestroy(cudaEvent_t) { return cudaSuccess; }

// ------------------------------------------------------------------ texture objects
enum cudaChannelFormatKind {
  cudaChannelFormatKindSigned = 0,
  cudaChannelFormatKindUnsigned = 1,
  cudaChannelFormatKindFloat = 2,
  cudaChannelFormatKindNone = 3
};
struct cudaChannelFormatDesc {
  int x, y, z, w;
  cudaChannelFormatKind f;
};
enum cudaResourceType {
  cudaResourceTypeArray = 0,
  cudaResourceTypeMipmappedArray = 1,
  cudaResourceTypeLinear = 2,
  cudaResourceTypePitch2D = 3
};
struct cudaResourceDesc {
  cudaResourceType resType;
  union {
    struct {
      void *devPtr;
      cudaChannelFormatDesc desc;
      size_t sizeInBytes;
    } linear;
    struct {
      void *devPtr;
      cudaChannelFormatDesc desc;
      size_t width, height, pitchInBytes;
    } pitch2D;
  } res;
};
enum cudaTextureAddressMode {
  cudaAddressModeWrap = 0,
  cudaAddressModeClamp = 1,
  cudaAddressModeMirror = 2,
  cudaAddressModeBorder = 3
};
enum cudaTextureFilterMode { cudaFilterModePoint = 0, cudaFilterModeLinear = 1 };
enum cudaTextureReadMode { cudaReadModeElementType = 0, cudaReadModeNormalizedFloat = 1 };
struct cudaTextureDesc {
  cudaTextureAddressMode addressMode[3];
  cudaTextureFilterMode filterMode;
  cudaTextureReadMode readMode;
  int sRGB;
  float borderColor[4];
  int normalizedCoords;
  unsigned int maxAnisotropy;
  cudaTextureFilterMode mipmapFilterMode;
  float mipmapLevelBias, minMipmapLevelClamp, maxMipmapLevelClamp;
};
struct cudaResourceViewDesc;
typedef unsigned long long cudaTextureObject_t;

namespace refshim {
struct TextureObject {
  cudaResourceDesc res;
  cudaTextureDesc tex;
};
}  // namespace refshim

inline cudaError_t cudaCreateTextureObject(cudaTextureObject_t *out, const cudaResourceDesc *res,
                                           const cudaTextureDesc *tex, const cudaResourceViewDesc *) {
  refshim::TextureObject *t = new refshim::TextureObject{*res, *tex};
  *out = (cudaTextureObject_t)(uintptr_t)t;
  return cudaSuccess;
}
inline cudaError_t cudaDestroyTextureObject(cudaTextureObject_t t) {
  delete (refshim::TextureObject *)(uintptr_t)t;
  return cudaSuccess;
}

namespace refshim {
// One coordinate of a point-filtered fetch (programming guide, "Texture Fetching"): a normalised coordinate in wrap
// mode is replaced by its fractional part, scaled by the extent N, and the texel index is the floor of the product;
// an index of N (a fractional part that rounded up to 1) wraps to 0.
inline int texel_index(float coord, const TextureObject *t, int dim, int n) {
  float x = coord;
  if (t->tex.normalizedCoords) {
    if (t->tex.addressMode[dim] == cudaAddressModeWrap) x = x - floorf(x);
    x = x * (float)n;
  }
  int i = (int)floorf(x);
  if (t->tex.normalizedCoords && t->tex.addressMode[dim] == cudaAddressModeWrap) {
    i %= n;
    if (i < 0) i += n;
  } else {
    if (i < 0) i = 0;
    if (i > n - 1) i = n - 1;
  }
  return i;
}
}  // namespace refshim

template <typename T>
inline T tex2D(cudaTextureObject_t obj, float x, float y);

// float4 from a pitched 2D resource of 4 x 8-bit unsigned channels, read as normalised float: c / 255.
template <>
inline float4 tex2D<float4>(cudaTextureObject_t obj, float x, float y) {
  const refshim::TextureObject *t = (const refshim::TextureObject *)(uintptr_t)obj;
  const int w = (int)t->res.res.pitch2D.width, h = (int)t->res.res.pitch2D.height;
  const int ix = refshim::texel_index(x, t, 0, w), iy = refshim::texel_index(y, t, 1, h);
  const uint8_t *px = (const uint8_t *)t->res.res.pitch2D.devPtr + (size_t)iy * t->res.res.pitch2D.pitchInBytes +
                      (size_t)ix * 4;
  float4 r;
  r.x = (float)px[0] / 255.0f;
  r.y = (float)px[1] / 255.0f;
  r.z = (float)px[2] / 255.0f;
  r.w = (float)px[3] / 255.0f;
  return r;
}

// ------------------------------------------------------------------ kernel launches
// kernel<<<grid, block>>>(args) has no host spelling; oracle/ref_launch_filter.py rewrites the reference's four
// launch expressions (all in utils.cu) to REF_LAUNCH(kernel, grid, block)(args), which runs the grid's threads one
// after another on the calling host thread.
namespace refshim {
template <typename K>
struct Launch {
  K kernel;
  dim3 grid, block;
  template <typename... A>
  void operator()(A &&...args) const {
    gridDim = grid;
    blockDim = block;
    for (unsigned bz = 0; bz < grid.z; bz++)
      for (unsigned by = 0; by < grid.y; by++)
        for (unsigned bx = 0; bx < grid.x; bx++)
          for (unsigned tz = 0; tz < block.z; tz++)
            for (unsigned ty = 0; ty < block.y; ty++)
              for (unsigned tx = 0; tx < block.x; tx++) {
                blockIdx = {bx, by, bz};
                threadIdx = {tx, ty, tz};
                kernel(args...);
              }
  }
};
template <typename K>
inline Launch<K> launch(K kernel, dim3 grid, dim3 block) {
  return Launch<K>{kernel, grid, block};
}
}  // namespace refshim
#define REF_LAUNCH(kernel, ...) ::refshim::launch(kernel, __VA_ARGS__)
