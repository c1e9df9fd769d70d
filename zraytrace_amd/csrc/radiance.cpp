// radiance.cpp - radiance queries on a resident context (zrt.h "radiance queries"): what
// zrt_ctx_radiance refuses, how it launches (plan_radiance, which zrt_debug_radiance_plan
// reports with no device), the equirectangular ray generator, and the launch itself: per
// round radiance_kernel over a bounded grid, then radiance_finish_kernel folding the
// round's parked chunk sums into the caller's sums.  Radiance is a query (queries.cpp): it
// runs through launch_query on the context's QueryState.
// ZRT_PLAN_ONLY (the host sanitizer build, tools/sanitize): the part that needs no device.
#include <algorithm>
#include <cmath>
#include <cstdlib>

#ifdef ZRT_PLAN_ONLY
#include "host.hpp"
#else
#include "context.hpp"
#endif

using zrt::fail;

namespace zrt {
// Blocks per CU of the radiance grid.  An item is a whole chunk of paths, so items differ
// in length far more than AO's rays do; blocks past the resident ones queue and the
// dispatcher hands them out as blocks end.  16 keeps the attenuation and stack overflow
// rows at 1 M lanes on 256 CUs.
constexpr uint32_t kRadianceBlocksPerCu = 16;
// The parked chunk sums of one round, unless the caller (or ZRT_RADIANCE_PARTIAL_CAP) says otherwise.
constexpr uint64_t kRadiancePartialCap = 256ull << 20;

int plan_radiance(const zrt_params* p, const struct zrt_radiance* rq, uint32_t n, uint32_t cu_count,
                  uint64_t partial_cap, zrt_radiance_plan* out) {
  if (!p || !rq || !out) return fail(ZRT_E_INVALID, "null argument");
  if (p->traversal > ZRT_TRAVERSAL_BINARY) return fail(ZRT_E_INVALID, "unknown traversal");
  if (p->prng > ZRT_PRNG_XOSHIRO256) return fail(ZRT_E_INVALID, "unknown prng");
  if (rq->n_samples == 0) return fail(ZRT_E_INVALID, "radiance: n_samples must be > 0");
  if (uint64_t(rq->first_sample) + rq->n_samples > 65536)
    return fail(ZRT_E_INVALID, "radiance: first_sample + n_samples must be <= 65536 (the key's sample field)");
  constexpr uint64_t kRayEnd = 1ull << 48;
  if (rq->first_ray > kRayEnd || kRayEnd - rq->first_ray < n)
    return fail(ZRT_E_INVALID, "radiance: first_ray + n must be <= 2^48 (the key's ray field)");
  if (rq->flags & ~uint32_t(ZRT_RQ_ACCUMULATE)) return fail(ZRT_E_INVALID, "radiance: unknown flag");
  const uint32_t c = p->sample_chunk ? p->sample_chunk : uint32_t(ZRT_DEFAULT_SAMPLE_CHUNK);
  if ((rq->flags & ZRT_RQ_ACCUMULATE) && rq->first_sample % c != 0)
    return fail(ZRT_E_INVALID, "radiance: ZRT_RQ_ACCUMULATE needs first_sample to be a multiple of the sample chunk");
  if (cu_count == 0) return fail(ZRT_E_INVALID, "radiance: cu_count must be > 0");
  *out = zrt_radiance_plan{};
  out->chunk = c;
  out->call_chunks = uint32_t((uint64_t(rq->n_samples) + c - 1) / c);  // (any 32-bit c)
  out->last_chunk = rq->n_samples - (out->call_chunks - 1) * c;
  out->items = uint64_t(n) * out->call_chunks;
  out->key_offset = (rq->first_ray << 16) + p->seed * 0x9E3779B97F4A7C15ULL;
  out->blocks_per_cu = kRadianceBlocksPerCu;
  if (n == 0) return ZRT_OK;  // nothing is launched
  const uint64_t cap = partial_cap ? partial_cap : kRadiancePartialCap;
  const uint64_t row = uint64_t(n) * sizeof(float4);  // one chunk of every ray
  out->chunks_per_round = uint32_t(std::max<uint64_t>(1, std::min<uint64_t>(out->call_chunks, cap / row)));
  out->rounds = (out->call_chunks + out->chunks_per_round - 1) / out->chunks_per_round;
  out->partial_bytes = row * out->chunks_per_round;
  const uint64_t groups = (uint64_t(n) * out->chunks_per_round + kBlock - 1) / kBlock;
  out->grid = uint32_t(std::min<uint64_t>(groups, uint64_t(kRadianceBlocksPerCu) * cu_count));
  out->resident_lanes = uint64_t(out->grid) * kBlock;
  return ZRT_OK;
}
}  // namespace zrt

int zrt_debug_radiance_plan(const zrt_params* params, const struct zrt_radiance* rq, uint32_t n, uint32_t cu_count,
                            uint64_t partial_cap_bytes, zrt_radiance_plan* out) {
  return zrt::plan_radiance(params, rq, n, cu_count, partial_cap_bytes, out);
}

int zrt_rays_equirect(const float origin[3], uint32_t width, uint32_t height, float* out_rays) {
  if (!origin || !out_rays) return fail(ZRT_E_INVALID, "null argument");
  if (width == 0 || height == 0) return fail(ZRT_E_INVALID, "equirect: width and height must be > 0");
  const double pi = 3.14159265358979323846;
  for (uint32_t y = 0; y < height; ++y) {
    const double theta = pi * (double(y) + 0.5) / double(height);  // from -y: row 0 looks down
    const double st = std::sin(theta), ct = std::cos(theta);
    for (uint32_t x = 0; x < width; ++x) {
      const double phi = 2.0 * pi * (double(x) + 0.5) / double(width);
      float* r = out_rays + 6ull * (uint64_t(y) * width + x);
      r[0] = origin[0];
      r[1] = origin[1];
      r[2] = origin[2];
      r[3] = float(st * std::cos(phi));
      r[4] = float(-ct);
      r[5] = float(st * std::sin(phi));
    }
  }
  return ZRT_OK;
}

#ifndef ZRT_PLAN_ONLY
namespace zrt {
uint64_t query_env_u64(const char* name) {
  const char* e = std::getenv(name);
  return e ? std::strtoull(e, nullptr, 10) : 0;
}

uint32_t prepare_radiance(zrt_ctx* c, const zrt_params* p, const zrt_radiance_plan& plan, hipStream_t st) {
  QueryState& q = c->query;
  uint32_t grid = plan.grid;
  if (const uint64_t g = query_env_u64("ZRT_RADIANCE_GRID")) grid = uint32_t(std::min<uint64_t>(grid, g));
  const uint64_t n_lanes = uint64_t(grid) * kBlock;
  KArgs probe{};
  const TracePlan t0 = fill_trace(probe, c, p->traversal, true, p->max_depth);
  const BufNeed need{uint64_t(att_rows_per_path(t0.lp, p->max_depth)) * n_lanes, 0};
  const uint64_t partial_elems = plan.partial_bytes / sizeof(float4);
  if (q.att.n < need.att_elems || q.partial.n < partial_elems || !q.counters.p) {
    HIPCHK(hipStreamSynchronize(st));
    q.att.grow(need.att_elems);
    q.partial.grow(partial_elems);
    if (!q.counters.p) q.counters.alloc(kScratchSlots);
  }
  q.counters_host.alloc(kScratchSlots);
  HIPCHK(hipMemsetAsync(q.counters.p, 0, sizeof(unsigned long long) * kScratchSlots, st));
  return grid;
}

void fill_radiance(zrt_ctx* c, const zrt_params* p, KArgs& a, const TracePlan& t, uint32_t launch_grid, const char* name) {
  QueryState& q = c->query;
  check_buffers(name, BufNeed{uint64_t(att_rows_per_path(t.lp, p->max_depth)) * a.n_lanes, 0}, q.att.n, 0);
  q.rq_att_lds_rows = t.lp.att_rows;
  q.rq_stack_lds_rows = t.lp.stack_rows;
  q.rq_grid = launch_grid;
  a.max_depth = p->max_depth;
  a.att = q.att.p;
  a.att_cap = q.att.n;
  a.partial = q.partial.p;
  a.counters = q.counters.p;
}

void copy_radiance_counters(zrt_ctx* c, hipStream_t s) {
  QueryState& q = c->query;
  HIPCHK(hipMemcpyAsync(q.counters_host.get(), q.counters.p, sizeof(unsigned long long) * kScratchSlots,
                        hipMemcpyDeviceToHost, s));
}

int radiance_info(zrt_ctx* c, zrt_radiance_info* out) {
  try {
    HIPCHK(hipSetDevice(c->device));
    const QueryState& q = c->query;
    HIPCHK(hipEventSynchronize(q.done.done));
    *out = zrt_radiance_info{};
    out->samples = q.rq_samples;
    out->reflections = q.counters_host[kReflections];
    out->background_hits = q.counters_host[kBackground];
    out->recursion_depth_hits = q.counters_host[kDepthHits];
    out->rays = out->samples + out->reflections - out->recursion_depth_hits;
    float f = 0.0f;
    HIPCHK(hipEventElapsedTime(&f, q.timer.e0, q.timer.e1));
    out->kernel_ms = f;
    return ZRT_OK;
  }
  ZRT_CATCH_ALL
}
}  // namespace zrt

int zrt_ctx_radiance(zrt_ctx* c, const zrt_params* p, const struct zrt_radiance* rq, const float* dev_rays, uint32_t n,
                     float* dev_sum, float* dev_rgb, void* hip_stream) {
  if (!c) return fail(ZRT_E_INVALID, "null argument");
  zrt_radiance_plan plan;
  int rc = zrt::plan_radiance(p, rq, n, uint32_t(std::max(1, c->cu_count)), zrt::query_env_u64("ZRT_RADIANCE_PARTIAL_CAP"),
                              &plan);
  if (rc) return rc;
  rc = zrt::params_fit_ctx(c, p);
  if (rc) return rc;
  if (n == 0) return ZRT_OK;
  if (!dev_rays || !dev_sum) return fail(ZRT_E_INVALID, "null argument");
  if (zrt::ptr_misaligned(dev_rays, 4) || zrt::ptr_misaligned(dev_rgb, 4))
    return fail(ZRT_E_INVALID, "radiance: dev_rays and dev_rgb must be 4-byte aligned");
  if (zrt::ptr_misaligned(dev_sum, 16)) return fail(ZRT_E_INVALID, "radiance: dev_sum must be 16-byte aligned");
  try {
    HIPCHK(hipSetDevice(c->device));
    hipStream_t st = zrt::stream_of(c, hip_stream);
    zrt::QueryState& q = c->query;
    const uint32_t grid = zrt::prepare_radiance(c, p, plan, st);
    const bool accumulate = (rq->flags & ZRT_RQ_ACCUMULATE) != 0;
    const uint32_t total = accumulate ? rq->first_sample + rq->n_samples : rq->n_samples;
    const float scale = 1.0f / float(total);  // raytrace.zig:157
    float4* sum = reinterpret_cast<float4*>(dev_sum);
    zrt::launch_query(
        c, p, grid, st, true, "radiance query",
        [&](zrt::KArgs& a, const zrt::TracePlan& t, uint32_t launch_grid, hipStream_t s) {
          zrt::fill_radiance(c, p, a, t, launch_grid, "radiance query");
          zrt::RadianceArgs g{};
          g.key_offset = plan.key_offset;
          g.n = n;
          g.chunk = std::min<uint32_t>(plan.chunk, 65536u);
          g.sample_end = rq->first_sample + rq->n_samples;
          void* kernel = zrt::radiance_kernel_ptr(t.kmode, p->prng, t.stk16);
          zrt::radiance_rounds(plan, n, rq->first_sample, g.chunk, launch_grid,
                               [&](uint32_t r, uint32_t chunks, uint64_t n_items, uint32_t sample0, uint32_t round_grid) {
                                 g.n_items = n_items;
                                 g.sample0 = sample0;
                                 void* args[] = {&a, &g, &dev_rays};
                                 HIPCHK(hipLaunchKernel(kernel, dim3(round_grid), dim3(zrt::kBlock), args, t.lp.bytes, s));
                                 HIPCHK(zrt::launch_radiance_finish(s, q.partial.p, n, chunks, r == 0 && !accumulate ? 1u : 0u,
                                                                    sum, nullptr, 0.0f, 0u, q.err.p));
                               });
        },
        [&](hipStream_t s, const unsigned long long* err) {
          HIPCHK(zrt::launch_radiance_finish(s, q.partial.p, n, 0u, 0u, sum, dev_rgb, scale, 1u, err));
          zrt::copy_radiance_counters(c, s);
        },
        p->max_depth);
    q.rq_samples = uint64_t(n) * rq->n_samples;
    q.rq_launched = true;
    return ZRT_OK;
  }
  ZRT_CATCH_ALL
}

int zrt_ctx_radiance_info(zrt_ctx* c, zrt_radiance_info* out) {
  if (!c || !out) return fail(ZRT_E_INVALID, "null argument");
  if (!c->query.rq_launched) return fail(ZRT_E_INVALID, "no radiance query launched on this context yet");
  return zrt::radiance_info(c, out);
}

int zrt_ctx_debug_radiance(zrt_ctx* c, uint32_t out[4]) {
  if (!c || !out) return fail(ZRT_E_INVALID, "null argument");
  if (!c->query.rq_launched) return fail(ZRT_E_INVALID, "no radiance query launched on this context yet");
  try {
    HIPCHK(hipSetDevice(c->device));
    const zrt::QueryState& q = c->query;
    HIPCHK(hipEventSynchronize(q.done.done));
    out[0] = q.rq_att_lds_rows;
    out[1] = uint32_t(q.counters_host[zrt::kRqDeepestSlot]);
    out[2] = q.rq_stack_lds_rows;
    out[3] = q.rq_grid;
    return ZRT_OK;
  }
  ZRT_CATCH_ALL
}
#endif  // ZRT_PLAN_ONLY
