// ao.cpp - ambient occlusion on a resident context (zrt.h "ambient occlusion"): what
// zrt_ctx_ao refuses, how it launches (plan_ao, which zrt_debug_ao_plan reports with no
// device) and the launch itself: ao_kernel over a bounded grid, then ao_finish_kernel.
// AO is a query (queries.cpp): it runs through launch_query on the context's QueryState.
#include <cmath>

#include "context.hpp"

using zrt::fail;

namespace zrt {
// Blocks per CU of the AO grid.  A CU holds four blocks at ao_kernel's registers; the rest
// queue, and the dispatcher hands them out as blocks end, which evens out what the static
// round-robin of groups leaves uneven.  Measured on the bunny, 1024^2 x 16 (DESIGN.md
// section 5 "Ambient occlusion"): FAST is flat from 8 to 256 (0.80 .. 0.75 ms), BINARY gains
// steadily (1.42 ms at 8, 1.24 at 32, 1.10 at 64, 1.08 at one group per block).  32 keeps
// the overflow rows at 2 M lanes, an eighth of that frame's rays.
constexpr uint32_t kAoBlocksPerCu = 32;
// Groups a block's share shifts by from round to round (ao_kernel): odd, and no divisor of a
// tile row's groups at the usual widths.
constexpr uint32_t kAoRotate = 37;

int plan_ao(const zrt_params* p, const zrt_ao* ao, uint32_t cu_count, zrt_ao_plan* out) {
  if (!ao || !out) return fail(ZRT_E_INVALID, "null argument");
  const int rc = validate_params(p);  // (height > width and an unknown traversal among its refusals)
  if (rc) return rc;
  if (ao->n_samples == 0 || ao->n_samples > 1024) return fail(ZRT_E_INVALID, "ao: n_samples must be 1 .. 1024");
  if (uint64_t(ao->first_sample) + ao->n_samples > 65536)
    return fail(ZRT_E_INVALID, "ao: first_sample + n_samples must be <= 65536 (the key's sample field)");
  if (!(ao->radius > 0.001f)) return fail(ZRT_E_INVALID, "ao: radius must be > 0.001 (+inf allowed)");
  if (ao->flags & ~uint32_t(ZRT_AO_ACCUMULATE)) return fail(ZRT_E_INVALID, "ao: unknown flag");
  if (cu_count == 0) return fail(ZRT_E_INVALID, "ao: cu_count must be > 0");
  *out = zrt_ao_plan{};
  const uint64_t tiles = uint64_t((p->width + 7u) / 8u) * ((p->height + 7u) / 8u);
  out->pixel_slots = tiles * 64u;
  out->rays = out->pixel_slots * ao->n_samples;
  out->groups = (out->rays + kBlock - 1) / kBlock;
  out->blocks_per_cu = kAoBlocksPerCu;
  out->grid = uint32_t(std::min<uint64_t>(out->groups, uint64_t(kAoBlocksPerCu) * cu_count));
  out->resident_lanes = uint64_t(out->grid) * kBlock;
  out->ovf_row_bytes = out->resident_lanes * sizeof(uint32_t);
  out->reduction = 64u % ao->n_samples == 0 ? ZRT_AO_REDUCE_WAVE : ZRT_AO_REDUCE_ATOMIC;
  out->plane_bytes = out->reduction == ZRT_AO_REDUCE_ATOMIC ? uint64_t(p->width) * p->height * sizeof(uint32_t) : 0;
  return ZRT_OK;
}
}  // namespace zrt

int zrt_debug_ao_plan(const zrt_params* params, const zrt_ao* ao, uint32_t cu_count, zrt_ao_plan* out) {
  return zrt::plan_ao(params, ao, cu_count, out);
}

int zrt_ctx_ao(zrt_ctx* c, const zrt_camera* cam, const zrt_params* p, const zrt_ao* ao, const float* dev_features,
               uint32_t* dev_clear, float* dev_ao, void* hip_stream) {
  if (!c || !cam) return fail(ZRT_E_INVALID, "null argument");
  zrt_ao_plan plan;
  int rc = zrt::plan_ao(p, ao, uint32_t(std::max(1, c->cu_count)), &plan);
  if (rc) return rc;
  rc = zrt::params_fit_ctx(c, p);
  if (rc) return rc;
  if (!dev_features || !dev_clear) return fail(ZRT_E_INVALID, "null argument");
  if (reinterpret_cast<uintptr_t>(dev_features) & 15u)
    return fail(ZRT_E_INVALID, "ao: dev_features must be 16-byte aligned");
  if ((reinterpret_cast<uintptr_t>(dev_clear) & 3u) || (reinterpret_cast<uintptr_t>(dev_ao) & 3u))
    return fail(ZRT_E_INVALID, "ao: dev_clear and dev_ao must be 4-byte aligned");
  try {
    HIPCHK(hipSetDevice(c->device));
    hipStream_t st = zrt::stream_of(c, hip_stream);
    zrt::QueryState& q = c->query;
    zrt::AoArgs g{};
    g.n_slots = plan.pixel_slots;
    g.n_groups = plan.groups;
    g.n_samples = ao->n_samples;
    g.first_sample = ao->first_sample;
    g.accumulate = (ao->flags & ZRT_AO_ACCUMULATE) ? 1u : 0u;
    g.in_wave = plan.reduction == ZRT_AO_REDUCE_WAVE ? 1u : 0u;
    g.tiles_w = (p->width + 7u) / 8u;
    g.radius = ao->radius;
    g.rotate = zrt::kAoRotate;
    const uint64_t n_px = uint64_t(p->width) * p->height;
    uint32_t* plane = nullptr;
    if (!g.in_wave) {
      if (q.ao_plane.n < n_px) {
        // an earlier AO launch may still count on the old plane: one query is in flight per
        // context, so it ran on `st` or has been waited for; hipFree itself waits for the
        // device (the pattern of trace_rows)
        HIPCHK(hipStreamSynchronize(st));
        q.ao_plane.alloc(n_px);
      }
      plane = q.ao_plane.p;
      HIPCHK(hipMemsetAsync(plane, 0, n_px * sizeof(uint32_t), st));
    }
    const float4* feat = reinterpret_cast<const float4*>(dev_features);
    const uint32_t xbound = zrt::geometry(p).xbound;
    zrt::launch_query(
        c, p, plan.grid, st, true, "ambient occlusion",
        [&](zrt::KArgs& a, const zrt::TracePlan& t, uint32_t grid, hipStream_t s) {
          zrt::fill_camera(a, cam, p);
          a.seed_mix = p->seed * 0x9E3779B97F4A7C15ULL;
          void* args[] = {&a, &g, &feat, &dev_clear, &dev_ao, &plane};
          HIPCHK(hipLaunchKernel(zrt::ao_kernel_ptr(t.kmode, p->prng, t.stk16), dim3(grid), dim3(zrt::kBlock), args,
                                 t.lp.bytes, s));
        },
        [&](hipStream_t s, const unsigned long long* err) {
          HIPCHK(zrt::launch_ao_finish(s, g, p->width, p->height, xbound, feat, dev_clear, dev_ao, plane, err));
        });
    return ZRT_OK;
  }
  ZRT_CATCH_ALL
}

int zrt_ctx_ao_ms(zrt_ctx* c, double* ms) { return zrt_ctx_query_ms(c, ms); }
