// denoise.hip — edge-avoiding a-trous wavelet filter (Dammertz et al. 2010) on
// the assembled frame, guided by the first-hit feature buffers.
//
// The definition (include/zrt.h) is f32 operation by
// operation; this file is compiled with -ffp-contract=off like the render
// kernels, so every product, sum and `/` below is one IEEE rounding and
// tests/denoise_ref.py restates the result bit for bit.
//
// Plan: a packing pass turns the frame's RGB triples inside D into float4 (and
// copies the pixels outside D to the output); then one launch per iteration,
// ping-ponging between two float4 planes, the last one writing RGB triples to
// the output.  A tap is three 16-byte loads: the colour and the two feature
// float4.  Steps 1 and 2 stage the block's pixels plus halo in LDS (every pixel
// of the region is read by up to 25 lanes of the block); from step 4 on the
// taps of one block no longer share pixels with each other's, and are read
// straight from memory.
// zrt_ctx_denoise_rect (zrt.h "denoising lens frames") runs the same kernels with a pixel
// rectangle of the frame as D: the RECT instantiations, whose planes are the rectangle's.
// The variance plane of a camera query's sums (camera_variance_kernel) lives here too.
#include "denoise.hpp"

namespace zrt {
namespace {

constexpr int kDnBX = 32, kDnBY = 8;  // a wave is two 32-pixel rows: 512 contiguous bytes per row and load

// h = {1/16, 1/4, 3/8, 1/4, 1/16}; every h(dx) * h(dy) is exact in f32
__device__ __forceinline__ float dn_h(int d) { return d == 0 ? 0.375f : (d == 1 || d == -1) ? 0.25f : 0.0625f; }

struct DnCentre {
  float4 c, f0, f1;
  bool hit;
  float kz;
};

// One tap q of pixel p (not the centre): the weight's tests in the definition's
// order; adds into acc / wsum when the tap survives.
__device__ __forceinline__ void dn_tap(const DnCentre& p, const float4 cq, const float4 f0q, const float4 f1q,
                                       float w, uint32_t terms, float kc, float inv_n, float inv_a, float& ar,
                                       float& ag, float& ab, float& wsum) {
  const bool hit_q = __float_as_uint(f1q.w) != 0u;
  if (p.hit != hit_q) return;
  if (terms & kDnColor) {
    const float t = 1.0f - ((fabsf(p.c.x - cq.x) + fabsf(p.c.y - cq.y)) + fabsf(p.c.z - cq.z)) * kc;
    if (!(t > 0.0f)) return;
    w = w * t;
  }
  if (terms & kDnNormal) {
    const float dx = p.f0.x - f0q.x, dy = p.f0.y - f0q.y, dz = p.f0.z - f0q.z;
    const float t = 1.0f - ((dx * dx + dy * dy) + dz * dz) * inv_n;
    if (!(t > 0.0f)) return;
    w = w * t;
  }
  if (terms & kDnAlbedo) {
    const float t = 1.0f - ((fabsf(p.f1.x - f1q.x) + fabsf(p.f1.y - f1q.y)) + fabsf(p.f1.z - f1q.z)) * inv_a;
    if (!(t > 0.0f)) return;
    w = w * t;
  }
  if (terms & kDnDepth) {
    const float t = 1.0f - fabsf(p.f0.w - f0q.w) * p.kz;
    if (!(t > 0.0f)) return;
    w = w * t;
  }
  if (!(w > 0.0f)) return;
  ar = ar + cq.x * w;
  ag = ag + cq.y * w;
  ab = ab + cq.z * w;
  wsum = wsum + w;
}

// S = 1, 2: the step, staged through LDS; S = 0: any step, taps from memory.
// LAST: the iteration writes RGB triples into the output frame.
// RECT: D is the rectangle n x ny at (ox, oy) of the frame (zrt_ctx_denoise_rect) and the
// planes are n x ny; without it D is the square [0, n)^2 and ny, ox, oy are not read - the
// kernels of zrt_ctx_denoise / zrt_ctx_denoise_guided stay as they were compiled.
template <int S, bool LAST, bool RECT>
__global__ void __launch_bounds__(kDnBX* kDnBY)
    atrous_kernel(const float4* __restrict__ cin, const float4* __restrict__ feat, float4* __restrict__ cout,
                  float* __restrict__ out, uint32_t n, uint32_t width, int step, uint32_t terms, float kc,
                  float inv_n, float inv_a, float inv_z, uint32_t ny, uint32_t ox, uint32_t oy) {
  constexpr int RW = kDnBX + 4 * S, RH = kDnBY + 4 * S;
  __shared__ float4 s_c[S ? RW * RH : 1], s_f0[S ? RW * RH : 1], s_f1[S ? RW * RH : 1];
  const int x0 = int(blockIdx.x) * kDnBX, y0 = int(blockIdx.y) * kDnBY;
  const int px = x0 + int(threadIdx.x), py = y0 + int(threadIdx.y);
  // D = [0, ni) x [0, nj) in the planes' own coordinates; fo: the frame offset of D's origin
  const int ni = int(n), nj = RECT ? int(ny) : ni;
  const size_t fo = RECT ? size_t(oy) * width + ox : 0;
  if (S) {
    const int tid = int(threadIdx.y) * kDnBX + int(threadIdx.x);
    for (int i = tid; i < RW * RH; i += kDnBX * kDnBY) {
      const int gx = x0 - 2 * S + i % RW, gy = y0 - 2 * S + i / RW;
      float4 c = make_float4(0.0f, 0.0f, 0.0f, 0.0f), f0 = c, f1 = c;
      if (gx >= 0 && gx < ni && gy >= 0 && gy < nj) {
        c = cin[size_t(gy) * n + size_t(gx)];
        const size_t f = (fo + size_t(gy) * width + size_t(gx)) * 2;
        f0 = feat[f];
        f1 = feat[f + 1];
      }
      s_c[i] = c;
      s_f0[i] = f0;
      s_f1[i] = f1;
    }
    __syncthreads();
  }
  if (px >= ni || py >= nj) return;
  const int s = S ? S : step;
  DnCentre p;
  if (S) {
    const int l = (int(threadIdx.y) + 2 * S) * RW + int(threadIdx.x) + 2 * S;
    p.c = s_c[l];
    p.f0 = s_f0[l];
    p.f1 = s_f1[l];
  } else {
    p.c = cin[size_t(py) * n + size_t(px)];
    const size_t f = (fo + size_t(py) * width + size_t(px)) * 2;
    p.f0 = feat[f];
    p.f1 = feat[f + 1];
  }
  p.hit = __float_as_uint(p.f1.w) != 0u;
  const float rz = p.hit ? 1.0f / p.f0.w : 0.0f;
  p.kz = inv_z * rz;
  float ar = 0.0f, ag = 0.0f, ab = 0.0f, wsum = 0.0f;
#pragma unroll
  for (int dy = -2; dy <= 2; ++dy) {
#pragma unroll
    for (int dx = -2; dx <= 2; ++dx) {
      if (dx == 0 && dy == 0) {  // the centre tap: no tests
        const float w = 0.375f * 0.375f;
        ar = ar + p.c.x * w;
        ag = ag + p.c.y * w;
        ab = ab + p.c.z * w;
        wsum = wsum + w;
        continue;
      }
      // (step <= 128 and n <= 65535: no overflow)
      const int qx = px + s * dx, qy = py + s * dy;
      if (qx < 0 || qx >= ni || qy < 0 || qy >= nj) continue;
      float4 cq, f0q, f1q;
      if (S) {
        const int l = (int(threadIdx.y) + 2 * S + S * dy) * RW + int(threadIdx.x) + 2 * S + S * dx;
        cq = s_c[l];
        f0q = s_f0[l];
        f1q = s_f1[l];
      } else {
        cq = cin[size_t(qy) * n + size_t(qx)];
        const size_t f = (fo + size_t(qy) * width + size_t(qx)) * 2;
        f0q = feat[f];
        f1q = feat[f + 1];
      }
      dn_tap(p, cq, f0q, f1q, dn_h(dx) * dn_h(dy), terms, kc, inv_n, inv_a, ar, ag, ab, wsum);
    }
  }
  const float r = ar / wsum, g = ag / wsum, b = ab / wsum;
  if (LAST) {
    float* o = out + (fo + size_t(py) * width + size_t(px)) * 3;
    o[0] = r;
    o[1] = g;
    o[2] = b;
  } else {
    cout[size_t(py) * n + size_t(px)] = make_float4(r, g, b, 0.0f);
  }
}

// C_0: the frame's pixels inside D as float4; the pixels outside D go to the output as they are.
__global__ void dn_pack_kernel(const float* __restrict__ frame, float4* __restrict__ c0, float* __restrict__ out,
                               uint32_t n, uint32_t width) {
  const size_t i = size_t(blockIdx.x) * blockDim.x + threadIdx.x;
  if (i >= size_t(width) * n) return;
  const uint32_t x = uint32_t(i % width), y = uint32_t(i / width);
  const float r = frame[3 * i], g = frame[3 * i + 1], b = frame[3 * i + 2];
  if (x < n) {
    c0[size_t(y) * n + x] = make_float4(r, g, b, 0.0f);
  } else {
    out[3 * i] = r;
    out[3 * i + 1] = g;
    out[3 * i + 2] = b;
  }
}

template <int S, bool RECT>
hipError_t launch_iter(bool last, dim3 grid, hipStream_t st, const float4* cin, const float4* feat, float4* cout,
                       float* out, const DenoiseLaunch& l, int step, float kc, const DenoiseRect& r) {
  const dim3 block(kDnBX, kDnBY);
  const uint32_t n = RECT ? r.w : l.n;
  if (last)
    hipLaunchKernelGGL((atrous_kernel<S, true, RECT>), grid, block, 0, st, cin, feat, cout, out, n, l.width, step,
                       l.terms, kc, l.inv_n, l.inv_a, l.inv_z, r.h, r.x0, r.y0);
  else
    hipLaunchKernelGGL((atrous_kernel<S, false, RECT>), grid, block, 0, st, cin, feat, cout, out, n, l.width, step,
                       l.terms, kc, l.inv_n, l.inv_a, l.inv_z, r.h, r.x0, r.y0);
  return hipGetLastError();
}

// ---- the variance-guided filter (zrt.h "variance-guided denoising") -------------------
// The same plan with the variance V in the colour planes' fourth lane: a tap stays
// three 16-byte loads and the LDS footprint is unchanged.  The 3 x 3 smoothing of V
// reads adjacent pixels: inside the staged halo (2 S >= 1) for the LDS steps, eight
// 4-byte loads for the memory steps.

constexpr float kDnAlbedoMin = 0.015625f;  // a_min = 2^-6

// dn_tap with the guided colour test on L = (r + g) + b, scaled by the centre's kl,
// and the variance sum.
__device__ __forceinline__ void dg_tap(const DnCentre& p, float lum_p, float kl, const float4 cq, const float4 f0q,
                                       const float4 f1q, float w, uint32_t terms, float inv_n, float inv_a, float& ar,
                                       float& ag, float& ab, float& wsum, float& vacc) {
  const bool hit_q = __float_as_uint(f1q.w) != 0u;
  if (p.hit != hit_q) return;
  if (terms & kDnColor) {
    const float t = 1.0f - fabsf(lum_p - ((cq.x + cq.y) + cq.z)) * kl;
    if (!(t > 0.0f)) return;
    w = w * t;
  }
  if (terms & kDnNormal) {
    const float dx = p.f0.x - f0q.x, dy = p.f0.y - f0q.y, dz = p.f0.z - f0q.z;
    const float t = 1.0f - ((dx * dx + dy * dy) + dz * dz) * inv_n;
    if (!(t > 0.0f)) return;
    w = w * t;
  }
  if (terms & kDnAlbedo) {
    const float t = 1.0f - ((fabsf(p.f1.x - f1q.x) + fabsf(p.f1.y - f1q.y)) + fabsf(p.f1.z - f1q.z)) * inv_a;
    if (!(t > 0.0f)) return;
    w = w * t;
  }
  if (terms & kDnDepth) {
    const float t = 1.0f - fabsf(p.f0.w - f0q.w) * p.kz;
    if (!(t > 0.0f)) return;
    w = w * t;
  }
  if (!(w > 0.0f)) return;
  ar = ar + cq.x * w;
  ag = ag + cq.y * w;
  ab = ab + cq.z * w;
  wsum = wsum + w;
  vacc = vacc + cq.w * (w * w);
}

// S, LAST as atrous_kernel's.  LAST also multiplies the albedo back (demod) and
// writes the variance to out_var when it is given.
template <int S, bool LAST, bool RECT>
__global__ void __launch_bounds__(kDnBX* kDnBY)
    guided_kernel(const float4* __restrict__ cin, const float4* __restrict__ feat, float4* __restrict__ cout,
                  float* __restrict__ out, float* __restrict__ out_var, uint32_t n, uint32_t width, int step,
                  uint32_t terms, float sigma_c, float inv_n, float inv_a, float inv_z, uint32_t demod, uint32_t ny,
                  uint32_t ox, uint32_t oy) {
  constexpr int RW = kDnBX + 4 * S, RH = kDnBY + 4 * S;
  __shared__ float4 s_c[S ? RW * RH : 1], s_f0[S ? RW * RH : 1], s_f1[S ? RW * RH : 1];
  const int x0 = int(blockIdx.x) * kDnBX, y0 = int(blockIdx.y) * kDnBY;
  const int px = x0 + int(threadIdx.x), py = y0 + int(threadIdx.y);
  // D = [0, ni) x [0, nj) in the planes' own coordinates; fo: the frame offset of D's origin
  const int ni = int(n), nj = RECT ? int(ny) : ni;
  const size_t fo = RECT ? size_t(oy) * width + ox : 0;
  if (S) {
    const int tid = int(threadIdx.y) * kDnBX + int(threadIdx.x);
    for (int i = tid; i < RW * RH; i += kDnBX * kDnBY) {
      const int gx = x0 - 2 * S + i % RW, gy = y0 - 2 * S + i / RW;
      float4 c = make_float4(0.0f, 0.0f, 0.0f, 0.0f), f0 = c, f1 = c;
      if (gx >= 0 && gx < ni && gy >= 0 && gy < nj) {
        c = cin[size_t(gy) * n + size_t(gx)];
        const size_t f = (fo + size_t(gy) * width + size_t(gx)) * 2;
        f0 = feat[f];
        f1 = feat[f + 1];
      }
      s_c[i] = c;
      s_f0[i] = f0;
      s_f1[i] = f1;
    }
    __syncthreads();
  }
  if (px >= ni || py >= nj) return;
  const int s = S ? S : step;
  const int lc = (int(threadIdx.y) + 2 * S) * RW + int(threadIdx.x) + 2 * S;  // the centre's LDS slot
  DnCentre p;
  if (S) {
    p.c = s_c[lc];
    p.f0 = s_f0[lc];
    p.f1 = s_f1[lc];
  } else {
    p.c = cin[size_t(py) * n + size_t(px)];
    const size_t f = (fo + size_t(py) * width + size_t(px)) * 2;
    p.f0 = feat[f];
    p.f1 = feat[f + 1];
  }
  p.hit = __float_as_uint(p.f1.w) != 0u;
  const float rz = p.hit ? 1.0f / p.f0.w : 0.0f;
  p.kz = inv_z * rz;
  // the variance smoothed over the 3 x 3 adjacent pixels (a neighbour outside D: the centre's)
  float g = 0.0f;
#pragma unroll
  for (int dy = -1; dy <= 1; ++dy) {
#pragma unroll
    for (int dx = -1; dx <= 1; ++dx) {
      const float wt = (dx == 0 && dy == 0) ? 0.25f : (dx == 0 || dy == 0) ? 0.125f : 0.0625f;
      const int qx = px + dx, qy = py + dy;
      float v = p.c.w;
      if ((dx != 0 || dy != 0) && qx >= 0 && qx < ni && qy >= 0 && qy < nj)
        v = S ? s_c[lc + dy * RW + dx].w : reinterpret_cast<const float*>(cin)[(size_t(qy) * n + size_t(qx)) * 4 + 3];
      g = g + v * wt;
    }
  }
  const float kl = (terms & kDnColor) ? 1.0f / (sigma_c * __builtin_sqrtf(g) + 0x1p-20f) : 0.0f;
  const float lum_p = (p.c.x + p.c.y) + p.c.z;
  float ar = 0.0f, ag = 0.0f, ab = 0.0f, wsum = 0.0f, vacc = 0.0f;
#pragma unroll
  for (int dy = -2; dy <= 2; ++dy) {
#pragma unroll
    for (int dx = -2; dx <= 2; ++dx) {
      if (dx == 0 && dy == 0) {  // the centre tap: no tests
        const float w = 0.375f * 0.375f;
        ar = ar + p.c.x * w;
        ag = ag + p.c.y * w;
        ab = ab + p.c.z * w;
        wsum = wsum + w;
        vacc = vacc + p.c.w * (w * w);
        continue;
      }
      const int qx = px + s * dx, qy = py + s * dy;
      if (qx < 0 || qx >= ni || qy < 0 || qy >= nj) continue;
      float4 cq, f0q, f1q;
      if (S) {
        const int l = lc + S * dy * RW + S * dx;
        cq = s_c[l];
        f0q = s_f0[l];
        f1q = s_f1[l];
      } else {
        cq = cin[size_t(qy) * n + size_t(qx)];
        const size_t f = (fo + size_t(qy) * width + size_t(qx)) * 2;
        f0q = feat[f];
        f1q = feat[f + 1];
      }
      dg_tap(p, lum_p, kl, cq, f0q, f1q, dn_h(dx) * dn_h(dy), terms, inv_n, inv_a, ar, ag, ab, wsum, vacc);
    }
  }
  float r = ar / wsum, gg = ag / wsum, b = ab / wsum, v = vacc / (wsum * wsum);
  if (LAST) {
    if (demod && p.hit) {
      if (p.f1.x > kDnAlbedoMin) r = r * p.f1.x;
      if (p.f1.y > kDnAlbedoMin) gg = gg * p.f1.y;
      if (p.f1.z > kDnAlbedoMin) b = b * p.f1.z;
      const float am = ((p.f1.x + p.f1.y) + p.f1.z) * (1.0f / 3.0f);
      if (am > kDnAlbedoMin) v = v * (am * am);
    }
    float* o = out + (fo + size_t(py) * width + size_t(px)) * 3;
    o[0] = r;
    o[1] = gg;
    o[2] = b;
    if (out_var) out_var[fo + size_t(py) * width + size_t(px)] = v;
  } else {
    cout[size_t(py) * n + size_t(px)] = make_float4(r, gg, b, v);
  }
}

// {C_0, V_0}: dn_pack_kernel with the variance in the fourth lane, demodulated when asked.
__global__ void dg_pack_kernel(const float* __restrict__ frame, const float4* __restrict__ feat,
                               const float* __restrict__ var, float4* __restrict__ c0, float* __restrict__ out,
                               float* __restrict__ out_var, uint32_t n, uint32_t width, uint32_t demod) {
  const size_t i = size_t(blockIdx.x) * blockDim.x + threadIdx.x;
  if (i >= size_t(width) * n) return;
  const uint32_t x = uint32_t(i % width), y = uint32_t(i / width);
  float r = frame[3 * i], g = frame[3 * i + 1], b = frame[3 * i + 2], v = var[i];
  if (x < n) {
    if (demod) {
      const float4 a = feat[2 * i + 1];
      if (__float_as_uint(a.w) != 0u) {
        if (a.x > kDnAlbedoMin) r = r / a.x;
        if (a.y > kDnAlbedoMin) g = g / a.y;
        if (a.z > kDnAlbedoMin) b = b / a.z;
        const float am = ((a.x + a.y) + a.z) * (1.0f / 3.0f);
        if (am > kDnAlbedoMin) v = v / (am * am);
      }
    }
    c0[size_t(y) * n + x] = make_float4(r, g, b, v);
  } else {
    out[3 * i] = r;
    out[3 * i + 1] = g;
    out[3 * i + 2] = b;
    if (out_var) out_var[i] = v;
  }
}

template <int S, bool RECT>
hipError_t launch_guided(bool last, dim3 grid, hipStream_t st, const float4* cin, const float4* feat, float4* cout,
                         float* out, float* out_var, const DenoiseLaunch& l, int step, float sigma_c, uint32_t demod,
                         const DenoiseRect& r) {
  const dim3 block(kDnBX, kDnBY);
  const uint32_t n = RECT ? r.w : l.n;
  if (last)
    hipLaunchKernelGGL((guided_kernel<S, true, RECT>), grid, block, 0, st, cin, feat, cout, out, out_var, n, l.width,
                       step, l.terms, sigma_c, l.inv_n, l.inv_a, l.inv_z, demod, r.h, r.x0, r.y0);
  else
    hipLaunchKernelGGL((guided_kernel<S, false, RECT>), grid, block, 0, st, cin, feat, cout, out, out_var, n, l.width,
                       step, l.terms, sigma_c, l.inv_n, l.inv_a, l.inv_z, demod, r.h, r.x0, r.y0);
  return hipGetLastError();
}

// {C_0, V_0} of a rectangle: dn_pack_kernel / dg_pack_kernel over the whole width x height frame, the
// pixels of r into the r.w x r.h plane, every other pixel (and its variance) copied to the output.
// var == nullptr: the plain filter's packing (no variance, no demodulation).
__global__ void dn_pack_rect_kernel(const float* __restrict__ frame, const float4* __restrict__ feat,
                                    const float* __restrict__ var, float4* __restrict__ c0, float* __restrict__ out,
                                    float* __restrict__ out_var, uint32_t width, uint32_t height, DenoiseRect r,
                                    uint32_t demod) {
  const size_t i = size_t(blockIdx.x) * blockDim.x + threadIdx.x;
  if (i >= size_t(width) * height) return;
  const uint32_t x = uint32_t(i % width), y = uint32_t(i / width);
  float rr = frame[3 * i], g = frame[3 * i + 1], b = frame[3 * i + 2], v = var ? var[i] : 0.0f;
  if (x >= r.x0 && x - r.x0 < r.w && y >= r.y0 && y - r.y0 < r.h) {
    if (demod) {
      const float4 a = feat[2 * i + 1];
      if (__float_as_uint(a.w) != 0u) {
        if (a.x > kDnAlbedoMin) rr = rr / a.x;
        if (a.y > kDnAlbedoMin) g = g / a.y;
        if (a.z > kDnAlbedoMin) b = b / a.z;
        const float am = ((a.x + a.y) + a.z) * (1.0f / 3.0f);
        if (am > kDnAlbedoMin) v = v / (am * am);
      }
    }
    c0[size_t(y - r.y0) * r.w + (x - r.x0)] = make_float4(rr, g, b, v);
  } else {
    out[3 * i] = rr;
    out[3 * i + 1] = g;
    out[3 * i + 2] = b;
    if (out_var) out_var[i] = v;
  }
}

// The variance plane of a camera query's sums (zrt_ctx_camera_variance): one lane per pixel of r.
__global__ void camera_variance_kernel(const float4* __restrict__ sum, float* __restrict__ var, uint32_t width,
                                       DenoiseRect r, float ik, float sc) {
  const size_t i = size_t(blockIdx.x) * blockDim.x + threadIdx.x;
  if (i >= size_t(r.w) * r.h) return;
  const size_t R = size_t(r.y0 + uint32_t(i / r.w)) * width + (r.x0 + uint32_t(i % r.w));
  const float4 s = sum[R];
  const float m = (s.x + s.y) + s.z;
  const float mean = m * ik;
  float v = s.w * ik - mean * mean;
  v = (v > 0.0f || v != v) ? v : 0.0f;  // (as variance_kernel: a NaN stays NaN)
  var[R] = v * sc;
}

constexpr DenoiseRect kNoRect{0, 0, 0, 0};
}  // namespace

hipError_t denoise_guided_enqueue(const DenoiseLaunch& l, float sigma_c, bool demodulate, const float* frame,
                                  const float4* feat, const float* var, float* out, float* out_var, float4* buf0,
                                  float4* buf1, hipStream_t st) {
  if (l.n == 0 || l.width < l.n || l.iterations == 0 || l.iterations > 8) return hipErrorInvalidValue;
  const size_t pixels = size_t(l.width) * l.n;
  const uint32_t demod = demodulate ? 1u : 0u;
  hipLaunchKernelGGL(dg_pack_kernel, dim3(uint32_t((pixels + 255) / 256)), dim3(256), 0, st, frame, feat, var, buf0, out,
                     out_var, l.n, l.width, demod);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  const dim3 grid((l.n + kDnBX - 1) / kDnBX, (l.n + kDnBY - 1) / kDnBY);
  float4* cur = buf0;
  float4* nxt = buf1;
  for (uint32_t i = 0; i < l.iterations; ++i) {
    const int step = 1 << i;
    const bool last = i + 1 == l.iterations;
    e = step == 1   ? launch_guided<1, false>(last, grid, st, cur, feat, nxt, out, out_var, l, step, sigma_c, demod, kNoRect)
        : step == 2 ? launch_guided<2, false>(last, grid, st, cur, feat, nxt, out, out_var, l, step, sigma_c, demod, kNoRect)
                    : launch_guided<0, false>(last, grid, st, cur, feat, nxt, out, out_var, l, step, sigma_c, demod, kNoRect);
    if (e != hipSuccess) return e;
    float4* t = cur;
    cur = nxt;
    nxt = t;
  }
  return hipSuccess;
}

hipError_t denoise_enqueue(const DenoiseLaunch& l, const float* frame, const float4* feat, float* out, float4* buf0,
                           float4* buf1, hipStream_t st) {
  if (l.n == 0 || l.width < l.n || l.iterations == 0 || l.iterations > 8) return hipErrorInvalidValue;
  const size_t pixels = size_t(l.width) * l.n;
  hipLaunchKernelGGL(dn_pack_kernel, dim3(uint32_t((pixels + 255) / 256)), dim3(256), 0, st, frame, buf0, out, l.n,
                     l.width);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  const dim3 grid((l.n + kDnBX - 1) / kDnBX, (l.n + kDnBY - 1) / kDnBY);
  float4* cur = buf0;
  float4* nxt = buf1;
  for (uint32_t i = 0; i < l.iterations; ++i) {
    const int step = 1 << i;
    const float kc = l.inv_c * float(1 << i);  // sigma_color halves every iteration
    const bool last = i + 1 == l.iterations;
    e = step == 1   ? launch_iter<1, false>(last, grid, st, cur, feat, nxt, out, l, step, kc, kNoRect)
        : step == 2 ? launch_iter<2, false>(last, grid, st, cur, feat, nxt, out, l, step, kc, kNoRect)
                    : launch_iter<0, false>(last, grid, st, cur, feat, nxt, out, l, step, kc, kNoRect);
    if (e != hipSuccess) return e;
    float4* t = cur;
    cur = nxt;
    nxt = t;
  }
  return hipSuccess;
}

hipError_t denoise_rect_enqueue(const DenoiseLaunch& l, const DenoiseRect& r, uint32_t height, float sigma_c,
                                bool demodulate, const float* frame, const float4* feat, const float* var, float* out,
                                float* out_var, float4* buf0, float4* buf1, hipStream_t st) {
  if (r.w == 0 || r.h == 0 || r.x0 >= l.width || r.w > l.width - r.x0 || r.y0 >= height || r.h > height - r.y0 ||
      l.iterations == 0 || l.iterations > 8)
    return hipErrorInvalidValue;
  const size_t pixels = size_t(l.width) * height;
  const uint32_t demod = var && demodulate ? 1u : 0u;
  hipLaunchKernelGGL(dn_pack_rect_kernel, dim3(uint32_t((pixels + 255) / 256)), dim3(256), 0, st, frame, feat, var, buf0,
                     out, var ? out_var : nullptr, l.width, height, r, demod);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  const dim3 grid((r.w + kDnBX - 1) / kDnBX, (r.h + kDnBY - 1) / kDnBY);
  float4* cur = buf0;
  float4* nxt = buf1;
  for (uint32_t i = 0; i < l.iterations; ++i) {
    const int step = 1 << i;
    const bool last = i + 1 == l.iterations;
    if (var) {
      e = step == 1   ? launch_guided<1, true>(last, grid, st, cur, feat, nxt, out, out_var, l, step, sigma_c, demod, r)
          : step == 2 ? launch_guided<2, true>(last, grid, st, cur, feat, nxt, out, out_var, l, step, sigma_c, demod, r)
                      : launch_guided<0, true>(last, grid, st, cur, feat, nxt, out, out_var, l, step, sigma_c, demod, r);
    } else {
      const float kc = l.inv_c * float(1 << i);  // sigma_color halves every iteration
      e = step == 1   ? launch_iter<1, true>(last, grid, st, cur, feat, nxt, out, l, step, kc, r)
          : step == 2 ? launch_iter<2, true>(last, grid, st, cur, feat, nxt, out, l, step, kc, r)
                      : launch_iter<0, true>(last, grid, st, cur, feat, nxt, out, l, step, kc, r);
    }
    if (e != hipSuccess) return e;
    float4* t = cur;
    cur = nxt;
    nxt = t;
  }
  return hipSuccess;
}

hipError_t camera_variance_enqueue(const DenoiseRect& r, uint32_t width, float ik, float sc, const float4* sum,
                                   float* var, hipStream_t st) {
  const size_t pixels = size_t(r.w) * r.h;
  if (pixels == 0) return hipErrorInvalidValue;
  hipLaunchKernelGGL(camera_variance_kernel, dim3(uint32_t((pixels + 255) / 256)), dim3(256), 0, st, sum, var, width, r,
                     ik, sc);
  return hipGetLastError();
}

}  // namespace zrt
