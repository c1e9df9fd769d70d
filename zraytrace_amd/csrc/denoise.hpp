// denoise.hpp — the launch interface of the edge-avoiding a-trous filter
// (denoise.hip; the definition: include/zrt.h "denoising").
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

namespace zrt {

enum : uint32_t { kDnColor = 1u, kDnNormal = 2u, kDnAlbedo = 4u, kDnDepth = 8u };

struct DenoiseLaunch {
  uint32_t width;       // the frame's row stride in pixels
  uint32_t n;           // D = [0, n) x [0, n): n = params->height (raytrace.zig:168)
  uint32_t iterations;  // 1 .. 8
  uint32_t terms;       // kDn* bits of the terms that are on
  float inv_c, inv_n, inv_a, inv_z;  // 1.0f / sigma of each term that is on (host f32)
};

// Enqueues the packing pass and one launch per iteration on `st`.  frame / out:
// width * n * 3 floats; feat: width * n * 2 float4 (16-byte aligned); buf0 / buf1:
// n * n float4 each, the ping-pong colour planes.  Nothing is read or written
// outside those extents.
hipError_t denoise_enqueue(const DenoiseLaunch& l, const float* frame, const float4* feat, float* out,
                           float4* buf0, float4* buf1, hipStream_t st);

// The variance-guided filter (zrt.h "variance-guided denoising"): the same passes
// with the variance in the colour planes' fourth lane.  sigma_c: sigma_color itself
// (l.inv_c is not read); demodulate: ZRT_DN_DEMODULATE.  var: width * n floats;
// out_var (may be null): the same, written with the filtered variance.
hipError_t denoise_guided_enqueue(const DenoiseLaunch& l, float sigma_c, bool demodulate, const float* frame,
                                  const float4* feat, const float* var, float* out, float* out_var, float4* buf0,
                                  float4* buf1, hipStream_t st);

// A pixel rectangle of the frame (zrt_rect): the domain of denoise_rect_enqueue.
struct DenoiseRect {
  uint32_t x0, y0, w, h;
};

// Both filters with D = r (zrt_ctx_denoise_rect).  l: width, iterations, terms and the
// inverse sigmas (l.n is not read); height: the frame's.  var == nullptr: the plain filter
// (sigma_c, demodulate and out_var are not read); else the guided one.  frame / out: width *
// height * 3 floats, feat: width * height * 2 float4, var / out_var: width * height floats;
// buf0 / buf1: r.w * r.h float4 each.  Pixels outside r are copied to out (and out_var).
hipError_t denoise_rect_enqueue(const DenoiseLaunch& l, const DenoiseRect& r, uint32_t height, float sigma_c,
                                bool demodulate, const float* frame, const float4* feat, const float* var, float* out,
                                float* out_var, float4* buf0, float4* buf1, hipStream_t st);

// The variance plane of a camera query's sums over r (zrt_ctx_camera_variance): sum: width *
// height float4 {r, g, b, Q}; var: width * height floats, written inside r only.
hipError_t camera_variance_enqueue(const DenoiseRect& r, uint32_t width, float ik, float sc, const float4* sum,
                                   float* var, hipStream_t st);

}  // namespace zrt
