// temporal.hip — temporal accumulation: the previous frame's history reprojected
// into this frame's pixels under a moving camera and blended in (the temporal half
// of SVGF, Schied et al. 2017).
//
// The definition (include/zrt.h "temporal accumulation") is
// f32 operation by operation; this file is compiled with -ffp-contract=off like
// the filters, so every product, sum, `/` and sqrtf below is one IEEE rounding and
// tests/temporal_ref.py restates the result bit for bit.
//
// Plan: one launch per frame, one thread per pixel of the frame.  A pixel reads
// its own colour, variance and features, reprojects its first hit into the
// previous frame (nine dot-product terms and two divisions), gathers up to four
// taps of the previous state - the history float4, the first feature float4, the id
// word and the length of each - and writes its output and the next state.  The
// taps of a wave land on two or three rows of the previous planes, next to each
// other unless the depth varies wildly inside the wave, so they are read straight
// from memory; nothing is shared through LDS.  The state is double-buffered: a
// launch reads `prev` and writes `next`, which no thread of it reads.
#include "temporal.hpp"

#include "denoise.hpp"

namespace zrt {
namespace {

constexpr int kTaBX = 32, kTaBY = 8;  // the filters' block: a wave is two 32-pixel rows
constexpr float kTaAlbedoMin = 0.015625f;  // a_min = 2^-6 (the guided filter's)

__device__ __forceinline__ float ta_dot(float ax, float ay, float az, const float (&b)[3]) {
  return (ax * b[0] + ay * b[1]) + az * b[2];
}

__global__ void __launch_bounds__(kTaBX* kTaBY)
    temporal_kernel(const TemporalLaunch l, const float* __restrict__ frame, const float4* __restrict__ feat,
                    const float* __restrict__ var, const float4* __restrict__ hist_prev,
                    const float4* __restrict__ feat_prev, const uint32_t* __restrict__ len_prev,
                    float4* __restrict__ hist_next, float4* __restrict__ feat_next, uint32_t* __restrict__ len_next,
                    float* __restrict__ out, float* __restrict__ out_var, uint32_t* __restrict__ out_len) {
  const uint32_t px = blockIdx.x * kTaBX + threadIdx.x, py = blockIdx.y * kTaBY + threadIdx.y;
  if (px >= l.width || py >= l.n) return;
  const size_t i = size_t(py) * l.width + px;
  float r = frame[3 * i], g = frame[3 * i + 1], b = frame[3 * i + 2], v = var[i];
  if (px >= l.n) {  // outside D: copied, never a tap
    out[3 * i] = r;
    out[3 * i + 1] = g;
    out[3 * i + 2] = b;
    if (out_var) out_var[i] = v;
    if (out_len) out_len[i] = 0u;
    return;
  }
  const float4 f0 = feat[2 * i], f1 = feat[2 * i + 1];
  const bool hit = __float_as_uint(f1.w) != 0u;
  const bool demod = l.demod != 0u && hit;
  float am = 0.0f;
  if (demod) {  // step 1
    if (f1.x > kTaAlbedoMin) r = r / f1.x;
    if (f1.y > kTaAlbedoMin) g = g / f1.y;
    if (f1.z > kTaAlbedoMin) b = b / f1.z;
    am = ((f1.x + f1.y) + f1.z) * (1.0f / 3.0f);
    if (am > kTaAlbedoMin) v = v / (am * am);
  }
  float o_r = r, o_g = g, o_b = b, o_v = v;  // step 2: no history
  uint32_t n = 1u;
  if (l.history && hit) {
    float fx = float(px), fy = float(py), te = f0.w;  // step 3
    bool seen = true;
    if (!l.static_cam) {
      const float u = float(px) / l.f_width, vv = float(py) / l.f_height;
      const float ex = ((l.llc[0] + l.hor[0] * u) + l.ver[0] * vv) - l.org[0];
      const float ey = ((l.llc[1] + l.hor[1] * u) + l.ver[1] * vv) - l.org[1];
      const float ez = ((l.llc[2] + l.hor[2] * u) + l.ver[2] * vv) - l.org[2];
      const float el = __builtin_sqrtf((ex * ex + ey * ey) + ez * ez);
      const float dx = (l.org[0] + (ex / el) * f0.w) - l.porg[0];
      const float dy = (l.org[1] + (ey / el) * f0.w) - l.porg[1];
      const float dz = (l.org[2] + (ez / el) * f0.w) - l.porg[2];
      const float den = ta_dot(dx, dy, dz, l.rn);
      fx = (ta_dot(dx, dy, dz, l.ru) / den) * l.f_width;
      fy = (ta_dot(dx, dy, dz, l.rv) / den) * l.f_height;
      te = __builtin_sqrtf((dx * dx + dy * dy) + dz * dz);
      const float fn = float(l.n);
      seen = den > 0.0f && fx > -1.0f && fx < fn && fy > -1.0f && fy < fn;  // (a NaN fails)
    }
    if (seen) {  // step 4: fx, fy in (-1, n), so x0, y0 in [-1, n - 1]
      const float x0f = floorf(fx), y0f = floorf(fy);
      const float a = fx - x0f, bb = fy - y0f;
      const int x0 = int(x0f), y0 = int(y0f), ni = int(l.n);
      const float kz = l.inv_z * (1.0f / te);
      float ar = 0.0f, ag = 0.0f, ab = 0.0f, vacc = 0.0f, wsum = 0.0f;
      uint32_t nmin = 0xffffffffu;
#pragma unroll
      for (int j = 0; j < 2; ++j) {
#pragma unroll
        for (int k = 0; k < 2; ++k) {
          const int qx = x0 + k, qy = y0 + j;
          if (qx < 0 || qx >= ni || qy < 0 || qy >= ni) continue;
          const float w = (k ? a : 1.0f - a) * (j ? bb : 1.0f - bb);
          if (!(w > 0.0f)) continue;
          const size_t q = size_t(qy) * l.n + size_t(qx);
          const uint32_t lq = len_prev[q];
          if (lq == 0u) continue;
          if (__float_as_uint(feat_prev[2 * q + 1].w) == 0u) continue;
          const float4 g0 = feat_prev[2 * q];
          if (l.terms & kDnNormal) {
            const float nx = f0.x - g0.x, ny = f0.y - g0.y, nz = f0.z - g0.z;
            if (!(1.0f - ((nx * nx + ny * ny) + nz * nz) * l.inv_n > 0.0f)) continue;
          }
          if (l.terms & kDnDepth) {
            if (!(1.0f - fabsf(te - g0.w) * kz > 0.0f)) continue;
          }
          const float4 h = hist_prev[q];
          if (h.x != h.x || h.y != h.y || h.z != h.z || h.w != h.w) continue;
          ar = ar + h.x * w;
          ag = ag + h.y * w;
          ab = ab + h.z * w;
          vacc = vacc + h.w * w;
          wsum = wsum + w;
          nmin = lq < nmin ? lq : nmin;
        }
      }
      if (nmin != 0xffffffffu) {  // step 5 (a surviving tap has len >= 1 and w > 0)
        const float hr = ar / wsum, hg = ag / wsum, hb = ab / wsum, hv = vacc / wsum;
        n = nmin + 1u < l.max_history ? nmin + 1u : l.max_history;
        const float rr = 1.0f / float(n);
        const float al = rr > l.alpha_min ? rr : l.alpha_min, om = 1.0f - al;
        o_r = hr * om + r * al;
        o_g = hg * om + g * al;
        o_b = hb * om + b * al;
        o_v = hv * (om * om) + v * (al * al);
      }
    }
  }
  const size_t p = size_t(py) * l.n + px;  // step 6
  hist_next[p] = make_float4(o_r, o_g, o_b, o_v);
  len_next[p] = n;
  feat_next[2 * p] = f0;
  feat_next[2 * p + 1] = f1;
  if (demod) {
    if (f1.x > kTaAlbedoMin) o_r = o_r * f1.x;
    if (f1.y > kTaAlbedoMin) o_g = o_g * f1.y;
    if (f1.z > kTaAlbedoMin) o_b = o_b * f1.z;
    if (am > kTaAlbedoMin) o_v = o_v * (am * am);
  }
  out[3 * i] = o_r;
  out[3 * i + 1] = o_g;
  out[3 * i + 2] = o_b;
  if (out_var) out_var[i] = o_v;
  if (out_len) out_len[i] = n;
}

}  // namespace

hipError_t temporal_enqueue(const TemporalLaunch& l, const float* frame, const float4* feat, const float* var,
                            const TemporalPlanes& prev, const TemporalPlanes& next, float* out, float* out_var,
                            uint32_t* out_len, hipStream_t st) {
  if (l.n == 0 || l.width < l.n || l.max_history == 0 || l.max_history > 65535u) return hipErrorInvalidValue;
  if (!next.hist || !next.feat || !next.len || next.hist == prev.hist) return hipErrorInvalidValue;
  if (l.history && (!prev.hist || !prev.feat || !prev.len)) return hipErrorInvalidValue;
  const dim3 grid((l.width + kTaBX - 1) / kTaBX, (l.n + kTaBY - 1) / kTaBY);
  hipLaunchKernelGGL(temporal_kernel, grid, dim3(kTaBX, kTaBY), 0, st, l, frame, feat, var, prev.hist, prev.feat,
                     prev.len, next.hist, next.feat, next.len, out, out_var, out_len);
  return hipGetLastError();
}

}  // namespace zrt
