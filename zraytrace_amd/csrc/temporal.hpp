// temporal.hpp — the launch interface of the temporal accumulation step
// (temporal.hip; the definition: include/zrt.h "temporal accumulation", DESIGN.md
// section 5).
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

namespace zrt {

struct TemporalLaunch {
  uint32_t width;        // the frame's row stride in pixels
  uint32_t n;            // D = [0, n) x [0, n): n = params->height
  uint32_t history;      // the state holds a previous frame this one may read
  uint32_t static_cam;   // the camera is the previous one byte for byte
  uint32_t terms;        // kDnNormal | kDnDepth: the tests that are on
  uint32_t demod;        // ZRT_TA_DEMODULATE
  uint32_t max_history;  // 1 .. 65535
  float alpha_min, inv_n, inv_z;  // 1.0f / sigma of each test that is on (host f32)
  float f_width, f_height;
  float org[3], llc[3], hor[3], ver[3];  // the frame's camera
  float porg[3], rn[3], ru[3], rv[3];    // the previous camera's reprojection plan
};

// The state one frame reads (prev) or writes (next), all in D's own layout: n * n
// entries, row stride n.
struct TemporalPlanes {
  float4* hist;   // {r, g, b, V}
  float4* feat;   // 2 float4 per pixel: the feature buffer's
  uint32_t* len;  // history length
};

// Enqueues the one launch of a frame on `st`.  frame / out: width * n * 3 floats;
// feat: width * n * 2 float4 (16-byte aligned); var / out_var (may be null): width *
// n floats; out_len (may be null): width * n.  prev is read only with l.history set;
// prev and next are distinct planes.  Nothing is read or written outside those
// extents.
hipError_t temporal_enqueue(const TemporalLaunch& l, const float* frame, const float4* feat, const float* var,
                            const TemporalPlanes& prev, const TemporalPlanes& next, float* out, float* out_var,
                            uint32_t* out_len, hipStream_t st);

}  // namespace zrt
