// rtmi_accumulate: temporal accumulation of a frame into a reprojected history (include/rtmi.h states the rule;
// DESIGN.md 2.9 the layout and why the rule has its shape).  Every + - * / and sqrt below is one binary32 operation: the
// file is compiled without contraction and with IEEE division and square root like the rest of the library, and nothing
// here may be reassociated -- the tests hold the result to a numpy restatement bit for bit.
//
// A history is three planes of 16-byte records indexed by the row-major pixel:
//   G[p] = {nx, ny, nz, z}             the guides of the frame that wrote it
//   C[p] = {Cr, Cg, Cb, length}        the accumulated colour and how many frames it holds
//   V[p] = {Vr, Vg, Vb, surface}       the variance of that colour; surface = 1.0f where alpha > 0, else 0.0f
#pragma once
// (included by kernels.hip inside namespace rtmi, after denoise_body.h, whose 32 x 8 tile it shares)

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
