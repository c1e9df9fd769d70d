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

}  // namespace zrt
