// The image filters over row-major whole-frame buffers: rtmi_denoise and, below it, rtmi_accumulate, which shares its
// 32 x 8 tile.  A translation unit of its own: the filters use none of the trace path's device code.
//
// rtmi_denoise: a variance- and feature-guided a-trous filter over row-major frame buffers (include/rtmi.h states the
// rule; DESIGN.md 2.8 the layout).  Every + - * / below is one binary32 operation: the file is compiled without
// contraction and with IEEE division like the rest of the library, and nothing here may be reassociated -- the tests
// hold the result to a numpy restatement bit for bit.
//
// Scratch, all 16-byte records indexed by the row-major pixel:
//   G[p] = {nx, ny, nz, z}             the guides, written once by the prepare kernel
//   C[p] = {Cr, Cg, Cb, surface}       (demodulated) colour; surface = 1.0f where alpha > 0, else 0.0f
//   V[p] = {Vr, Vg, Vb, (Vr+Vg)+Vb}    (demodulated) variance and its sum, the rounded value the colour weight uses
// C and V exist twice: pass k reads one pair and writes the other.  The last pass writes the caller's float3 buffers.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "kernels.h"

namespace rtmi {

namespace {

constexpr int kTileW = 32, kTileH = 8;  // one workgroup: 32 x 8 pixels, a lane per pixel, a wave = two rows
constexpr int kLdsStep = 2;             // steps 1 and 2 stage tile + halo in LDS; larger steps read global records
constexpr int kLdsW = kTileW + 4 * kLdsStep, kLdsH = kTileH + 4 * kLdsStep;  // 40 x 16 records at step 2
constexpr float kMinWeightSum = 0x1p-32f;  // a pass filters a pixel only from this sum of weights on (include/rtmi.h)

struct DenoiseArgs {
  int height, width;
  int step;
  int squarings;
  int demodulate;
  float sigma_color2;  // sigma_color * sigma_color
  float sigma_depth;
  const float4 *g;         // G records
  const float4 *c_in;      // C, V records this pass reads
  const float4 *v_in;
  float4 *c_out;           // ... and writes (not the last pass)
  float4 *v_out;
  const float *albedo;     // the last pass: remodulation (demodulate only) and the caller's outputs
  float *out;
  float *out_variance;     // nullable
};

__device__ __forceinline__ float falloff(float x) {
  const float m = fmaxf(1.0f - 0.25f * x, 0.0f);
  const float m2 = m * m;
  return m2 * m2;
}

// ad = fmax(albedo, 0.01f) per channel: what a demodulated call divides by first and multiplies by last.
__device__ __forceinline__ void albedo_divisor(const float *albedo, int64_t p, float ad[3]) {
#pragma unroll
  for (int c = 0; c < 3; c++) ad[c] = fmaxf(albedo[p * 3 + c], 0.01f);
}

}  // namespace

__global__ __launch_bounds__(256) void denoise_prepare_kernel(int64_t n, int demodulate, const float *__restrict__ color,
                                                               const float *__restrict__ variance,
                                                               const float *__restrict__ albedo,
                                                               const float *__restrict__ normal,
                                                               const float *__restrict__ depth,
                                                               const float *__restrict__ alpha, float4 *__restrict__ g,
                                                               float4 *__restrict__ c0, float4 *__restrict__ v0) {
  const int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (p >= n) return;
  float c[3] = {color[p * 3 + 0], color[p * 3 + 1], color[p * 3 + 2]};
  float v[3] = {variance[p * 3 + 0], variance[p * 3 + 1], variance[p * 3 + 2]};
  if (demodulate) {
    float ad[3];
    albedo_divisor(albedo, p, ad);
#pragma unroll
    for (int k = 0; k < 3; k++) c[k] = c[k] / ad[k], v[k] = v[k] / (ad[k] * ad[k]);
  }
  g[p] = make_float4(normal[p * 3 + 0], normal[p * 3 + 1], normal[p * 3 + 2], depth[p]);
  c0[p] = make_float4(c[0], c[1], c[2], alpha[p] > 0.0f ? 1.0f : 0.0f);
  v0[p] = make_float4(v[0], v[1], v[2], (v[0] + v[1]) + v[2]);
}

// One pass.  LDS: the workgroup's tile and its halo of 2 * step pixels are staged (step <= kLdsStep); else every tap is
// three 16-byte global loads, which neighbouring lanes make of neighbouring records.  LAST: remodulate and write the
// caller's buffers instead of the records.
template <bool LDS, bool LAST>
__global__ __launch_bounds__(kTileW *kTileH) void atrous_kernel(DenoiseArgs a) {
  __shared__ float4 sG[LDS ? kLdsW * kLdsH : 1], sC[LDS ? kLdsW * kLdsH : 1], sV[LDS ? kLdsW * kLdsH : 1];
  const int s = a.step;
  const int j0 = (int)blockIdx.x * kTileW, i0 = (int)blockIdx.y * kTileH;
  const int tx = (int)threadIdx.x % kTileW, ty = (int)threadIdx.x / kTileW;
  const int i = i0 + ty, j = j0 + tx;
  const int lw = kTileW + 4 * s;  // the staged rectangle's width (LDS only); its origin is (i0 - 2s, j0 - 2s)
  if (LDS) {
    const int lh = kTileH + 4 * s;
    for (int r = (int)threadIdx.x; r < lw * lh; r += kTileW * kTileH) {
      const int qi = i0 - 2 * s + r / lw, qj = j0 - 2 * s + r % lw;
      if (qi >= 0 && qi < a.height && qj >= 0 && qj < a.width) {  // (records outside the image are never read below)
        const int64_t q = (int64_t)qi * a.width + qj;
        sG[r] = a.g[q], sC[r] = a.c_in[q], sV[r] = a.v_in[q];
      }
    }
    __syncthreads();
  }
  if (i >= a.height || j >= a.width) return;
  const int64_t p = (int64_t)i * a.width + j;
  const int lp = (ty + 2 * s) * lw + (tx + 2 * s);
  const float4 gp = LDS ? sG[lp] : a.g[p], cp = LDS ? sC[lp] : a.c_in[p], vp = LDS ? sV[lp] : a.v_in[p];
  const bool surf_p = cp.w > 0.0f;
  const float depth_scale = a.sigma_depth * gp.w + 1e-6f;
  const float h[5] = {1.0f / 16, 1.0f / 4, 3.0f / 8, 1.0f / 4, 1.0f / 16};
  float sw = 0.f, sc[3] = {0.f, 0.f, 0.f}, sv[3] = {0.f, 0.f, 0.f};
#pragma unroll 1  // (a row's loads in flight at a time: unrolled, all 75 are hoisted and the wave has the SIMD to itself)
  for (int dy = -2; dy <= 2; dy++) {
    // A row of taps: all fifteen loads first, from coordinates clamped into the image so that none needs a branch (a
    // clamped tap lies inside the footprint, so inside what is staged), then the arithmetic.  A tap the rule skips is
    // computed and not taken: the accumulators keep their bits.
    const int qi = i + dy * s, ci = min(max(qi, 0), a.height - 1);
    const float hy = dy == 0 ? h[2] : (dy == -1 || dy == 1) ? h[1] : h[0];
    float4 gq[5], cq[5], vq[5];
#pragma unroll
    for (int dx = -2; dx <= 2; dx++) {
      const int cj = min(max(j + dx * s, 0), a.width - 1);
      if (LDS) {
        const int lq = (ci - i0 + 2 * s) * lw + (cj - j0 + 2 * s);
        gq[dx + 2] = sG[lq], cq[dx + 2] = sC[lq], vq[dx + 2] = sV[lq];
      } else {
        const int64_t q = (int64_t)ci * a.width + cj;
        gq[dx + 2] = a.g[q], cq[dx + 2] = a.c_in[q], vq[dx + 2] = a.v_in[q];
      }
    }
#pragma unroll
    for (int dx = -2; dx <= 2; dx++) {
      const float4 G = gq[dx + 2], Cq = cq[dx + 2], Vq = vq[dx + 2];
      const int qj = j + dx * s;
      const bool surf_q = Cq.w > 0.0f;
      const bool take = qi >= 0 && qi < a.height && qj >= 0 && qj < a.width && surf_p == surf_q;
      float wn = fmaxf((gp.x * G.x + gp.y * G.y) + gp.z * G.z, 0.0f);
      for (int k = 0; k < a.squarings; k++) wn = wn * wn;
      float wz = falloff(fabsf(gp.w - G.w) / depth_scale);
      if (!surf_p) wn = 1.0f, wz = 1.0f;
      const float dr = cp.x - Cq.x, dg = cp.y - Cq.y, db = cp.z - Cq.z;
      const float d2 = (dr * dr + dg * dg) + db * db;
      const float vs = vp.w + Vq.w;
      const float wc = falloff(d2 / (a.sigma_color2 * vs + 1e-10f));
      const float w = (((hy * h[dx + 2]) * wn) * wz) * wc;
      const float w2 = w * w;
      sw = take ? sw + w : sw;
      sc[0] = take ? sc[0] + w * Cq.x : sc[0], sc[1] = take ? sc[1] + w * Cq.y : sc[1], sc[2] = take ? sc[2] + w * Cq.z : sc[2];
      sv[0] = take ? sv[0] + w2 * Vq.x : sv[0], sv[1] = take ? sv[1] + w2 * Vq.y : sv[1], sv[2] = take ? sv[2] + w2 * Vq.z : sv[2];
    }
  }
  float c[3] = {cp.x, cp.y, cp.z}, v[3] = {vp.x, vp.y, vp.z};
  // Below 2^-32 the pixel keeps what it has: sw * sw and the largest w * w stay normal numbers above it (a select each).
  const bool filtered = sw >= kMinWeightSum;
  const float sw2 = sw * sw;
#pragma unroll
  for (int k = 0; k < 3; k++) c[k] = filtered ? sc[k] / sw : c[k], v[k] = filtered ? sv[k] / sw2 : v[k];
  if (LAST) {
    if (a.demodulate) {
      float ad[3];
      albedo_divisor(a.albedo, p, ad);
#pragma unroll
      for (int k = 0; k < 3; k++) c[k] = c[k] * ad[k], v[k] = v[k] * (ad[k] * ad[k]);
    }
    a.out[p * 3 + 0] = c[0], a.out[p * 3 + 1] = c[1], a.out[p * 3 + 2] = c[2];
    if (a.out_variance) a.out_variance[p * 3 + 0] = v[0], a.out_variance[p * 3 + 1] = v[1], a.out_variance[p * 3 + 2] = v[2];
  } else {
    a.c_out[p] = make_float4(c[0], c[1], c[2], cp.w);
    a.v_out[p] = make_float4(v[0], v[1], v[2], (v[0] + v[1]) + v[2]);
  }
}

// Five arrays of 16-byte records, and 16 bytes to align the first one in whatever the caller hands over.
size_t denoise_scratch_bytes(int height, int width) { return (size_t)height * (size_t)width * 80 + 16; }

hipError_t launch_denoise(const DenoiseCall &d, hipStream_t stream) {
  const int64_t n = (int64_t)d.height * d.width;
  float4 *base = reinterpret_cast<float4 *>(((uintptr_t)d.scratch + 15) & ~(uintptr_t)15);
  float4 *g = base, *cv[2][2] = {{base + n, base + 2 * n}, {base + 3 * n, base + 4 * n}};
  hipLaunchKernelGGL(denoise_prepare_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream, n, d.demodulate, d.color,
                     d.variance, d.albedo, d.normal, d.depth, d.alpha, g, cv[0][0], cv[0][1]);
  hipError_t e = hipGetLastError();
  const dim3 grid((unsigned)((d.width + kTileW - 1) / kTileW), (unsigned)((d.height + kTileH - 1) / kTileH));
  for (int k = 0; k < d.iterations && e == hipSuccess; k++) {
    DenoiseArgs a{};
    a.height = d.height, a.width = d.width, a.step = 1 << k, a.squarings = d.normal_squarings, a.demodulate = d.demodulate;
    a.sigma_color2 = d.sigma_color * d.sigma_color, a.sigma_depth = d.sigma_depth;
    a.g = g, a.c_in = cv[k & 1][0], a.v_in = cv[k & 1][1], a.c_out = cv[~k & 1][0], a.v_out = cv[~k & 1][1];
    a.albedo = d.albedo, a.out = d.out, a.out_variance = d.out_variance;
    const bool lds = a.step <= kLdsStep, last = k == d.iterations - 1;
    auto kernel = lds ? (last ? atrous_kernel<true, true> : atrous_kernel<true, false>)
                      : (last ? atrous_kernel<false, true> : atrous_kernel<false, false>);
    hipLaunchKernelGGL(kernel, grid, dim3(kTileW * kTileH), 0, stream, a);
    e = hipGetLastError();
  }
  return e;
}

// ------------------------------------------------------------------ temporal accumulation (rtmi_accumulate)
// rtmi_accumulate: temporal accumulation of a frame into a reprojected history (include/rtmi.h states the rule;
// DESIGN.md 2.9 the layout and why the rule has its shape).  Every + - * / and sqrt below is one binary32 operation: the
// file is compiled without contraction and with IEEE division and square root like the rest of the library, and nothing
// here may be reassociated -- the tests hold the result to a numpy restatement bit for bit.
//
// A history is three planes of 16-byte records indexed by the row-major pixel:
//   G[p] = {nx, ny, nz, z}             the guides of the frame that wrote it
//   C[p] = {Cr, Cg, Cb, length}        the accumulated colour and how many frames it holds
//   V[p] = {Vr, Vg, Vb, surface}       the variance of that colour; surface = 1.0f where alpha > 0, else 0.0f

struct AccumulateArgs {
  int height, width;
  float normal_min, depth_tolerance, min_blend;
  float e[3], h[3], v[3], p[3];        // this frame's camera: e = llc - p (formed in binary64), horizontal, vertical, position
  float pp[3], r0[3], r1[3], r2[3];    // the history's camera: position, and the rows of the inverse of [h' v' llc' - p']
  const float *color, *variance, *normal, *depth, *alpha;
  const float4 *hist_in;               // null: no history (the HIST = false kernel)
  float4 *hist_out;
  float *out, *out_variance, *out_length;  // the last two nullable
};

// One lane per pixel, a workgroup of 32 x 8 pixels.  HIST: there is a history to reproject into.  All twelve records of
// the four taps are loaded first, from coordinates clamped into the image, so that no tap needs a branch; a tap the rule
// skips or refuses is computed and not taken: the accumulators keep their bits.  A fresh pixel reads (0, 0)'s taps.
template <bool HIST>
__global__ __launch_bounds__(kTileW *kTileH) void accumulate_kernel(AccumulateArgs a) {
  const int i = (int)blockIdx.y * kTileH + (int)threadIdx.x / kTileW, j = (int)blockIdx.x * kTileW + (int)threadIdx.x % kTileW;
  if (i >= a.height || j >= a.width) return;
  const int64_t n = (int64_t)a.height * a.width, p = (int64_t)i * a.width + j;
  const float cp[3] = {a.color[p * 3 + 0], a.color[p * 3 + 1], a.color[p * 3 + 2]};
  const float vp[3] = {a.variance[p * 3 + 0], a.variance[p * 3 + 1], a.variance[p * 3 + 2]};
  const float np[3] = {a.normal[p * 3 + 0], a.normal[p * 3 + 1], a.normal[p * 3 + 2]};
  const float zp = a.depth[p];
  const bool surf_p = a.alpha[p] > 0.0f;
  float c[3] = {cp[0], cp[1], cp[2]}, v[3] = {vp[0], vp[1], vp[2]}, len = 1.0f;  // fresh
  if (HIST) {
    const float W = (float)a.width, H = (float)a.height;
    const float xf = ((float)j + 0.5f) / W, yf = ((float)(a.height - i) + 0.5f) / H;  // the render's pixel centre (quirk g1)
    float D[3], d[3];
#pragma unroll
    for (int k = 0; k < 3; k++) D[k] = (a.e[k] + xf * a.h[k]) + yf * a.v[k];
    const float l = sqrtf((D[0] * D[0] + D[1] * D[1]) + D[2] * D[2]);
#pragma unroll
    for (int k = 0; k < 3; k++) d[k] = (a.p[k] + (D[k] / l) * zp) - a.pp[k];
    const float al = (a.r0[0] * d[0] + a.r0[1] * d[1]) + a.r0[2] * d[2];
    const float be = (a.r1[0] * d[0] + a.r1[1] * d[1]) + a.r1[2] * d[2];
    const float ga = (a.r2[0] * d[0] + a.r2[1] * d[1]) + a.r2[2] * d[2];
    const float ze = sqrtf((d[0] * d[0] + d[1] * d[1]) + d[2] * d[2]);
    float fx = (al / ga) * W - 0.5f, fy = (H + 0.5f) - (be / ga) * H;
    const bool seen = surf_p && ga > 0.0f && fx > -1.0f && fx < W && fy > -1.0f && fy < H;  // (a NaN compares false: fresh)
    if (!seen) fx = 0.0f, fy = 0.0f;
    const float rx = rintf(fx), ry = rintf(fy);
    if (fabsf(fx - rx) <= 1.0f / 64 && fabsf(fy - ry) <= 1.0f / 64) fx = rx, fy = ry;
    const float flx = floorf(fx), fly = floorf(fy);
    const int j0 = (int)flx, i0 = (int)fly;
    const float tx = fx - flx, ty = fy - fly;
    float4 gq[4], cq[4], vq[4];
#pragma unroll
    for (int t = 0; t < 4; t++) {
      const int ci = min(max(i0 + (t >> 1), 0), a.height - 1), cj = min(max(j0 + (t & 1), 0), a.width - 1);
      const int64_t q = (int64_t)ci * a.width + cj;
      gq[t] = a.hist_in[q], cq[t] = a.hist_in[n + q], vq[t] = a.hist_in[2 * n + q];
    }
    const float zlim = a.depth_tolerance * ze;
    float sw = 0.f, sl = 0.f, sc[3] = {0.f, 0.f, 0.f}, sv[3] = {0.f, 0.f, 0.f};
#pragma unroll
    for (int t = 0; t < 4; t++) {
      const int qi = i0 + (t >> 1), qj = j0 + (t & 1);
      const float b = ((t >> 1) ? ty : 1.0f - ty) * ((t & 1) ? tx : 1.0f - tx);
      const float dot = (np[0] * gq[t].x + np[1] * gq[t].y) + np[2] * gq[t].z;
      const bool take = qi >= 0 && qi < a.height && qj >= 0 && qj < a.width && vq[t].w > 0.0f && dot >= a.normal_min &&
                        fabsf(gq[t].w - ze) <= zlim;
      sw = take ? sw + b : sw;
      sl = take ? sl + b * cq[t].w : sl;
      sc[0] = take ? sc[0] + b * cq[t].x : sc[0], sc[1] = take ? sc[1] + b * cq[t].y : sc[1], sc[2] = take ? sc[2] + b * cq[t].z : sc[2];
      sv[0] = take ? sv[0] + b * vq[t].x : sv[0], sv[1] = take ? sv[1] + b * vq[t].y : sv[1], sv[2] = take ? sv[2] + b * vq[t].z : sv[2];
    }
    if (seen && sw > 0.0f) {
      len = sl / sw + 1.0f;
      const float w = fmaxf(1.0f / len, a.min_blend), o = 1.0f - w;
      const float oo = o * o, ww = w * w;
#pragma unroll
      for (int k = 0; k < 3; k++) c[k] = o * (sc[k] / sw) + w * cp[k], v[k] = oo * (sv[k] / sw) + ww * vp[k];
    }
  }
  a.out[p * 3 + 0] = c[0], a.out[p * 3 + 1] = c[1], a.out[p * 3 + 2] = c[2];
  if (a.out_variance) a.out_variance[p * 3 + 0] = v[0], a.out_variance[p * 3 + 1] = v[1], a.out_variance[p * 3 + 2] = v[2];
  if (a.out_length) a.out_length[p] = len;
  a.hist_out[p] = make_float4(np[0], np[1], np[2], zp);
  a.hist_out[n + p] = make_float4(c[0], c[1], c[2], len);
  a.hist_out[2 * n + p] = make_float4(v[0], v[1], v[2], surf_p ? 1.0f : 0.0f);
}

size_t history_bytes(int height, int width) { return (size_t)height * (size_t)width * 48; }

hipError_t launch_accumulate(const AccumulateCall &c, hipStream_t stream) {
  AccumulateArgs a{};
  a.height = c.height, a.width = c.width;
  a.normal_min = c.normal_min, a.depth_tolerance = c.depth_tolerance, a.min_blend = c.min_blend;
  for (int k = 0; k < 3; k++) {
    a.e[k] = c.e[k], a.h[k] = c.h[k], a.v[k] = c.v[k], a.p[k] = c.p[k];
    a.pp[k] = c.prev_p[k], a.r0[k] = c.r[0][k], a.r1[k] = c.r[1][k], a.r2[k] = c.r[2][k];
  }
  a.color = c.color, a.variance = c.variance, a.normal = c.normal, a.depth = c.depth, a.alpha = c.alpha;
  a.hist_in = static_cast<const float4 *>(c.history_in), a.hist_out = static_cast<float4 *>(c.history_out);
  a.out = c.out, a.out_variance = c.out_variance, a.out_length = c.out_length;
  const dim3 grid((unsigned)((c.width + kTileW - 1) / kTileW), (unsigned)((c.height + kTileH - 1) / kTileH));
  hipLaunchKernelGGL(a.hist_in ? accumulate_kernel<true> : accumulate_kernel<false>, grid, dim3(kTileW * kTileH), 0, stream, a);
  return hipGetLastError();
}

}  // namespace rtmi
