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
#pragma once
// (included by kernels.hip inside namespace rtmi: one code object holds every kernel of the library)

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
