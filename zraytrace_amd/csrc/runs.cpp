// runs.cpp - the run entry points over context.cpp's launch path: the accumulation
// run (zrt_ctx_accum_*), the adaptive run (zrt_ctx_adapt_*) and the live run's
// variance plane.
#include <algorithm>
#include <cstring>

#include "context.hpp"

using zrt::fail;

namespace {
// accumulate_kernel / resolve_kernel's metric shards of the last pass: their sums and maximum.
struct Metrics {
  uint64_t changed = 0, pixels = 0;
  uint32_t max_bits = 0;
};
Metrics reduce_metrics(const zrt_ctx* c) {
  Metrics m;
  for (uint32_t k = 0; k < zrt::kMetricShards; ++k) {
    const unsigned long long* s = &c->run.metrics_host[k * zrt::kMetricStride];
    m.changed += s[0];
    m.max_bits = std::max(m.max_bits, uint32_t(s[1]));
    m.pixels += s[2];
  }
  return m;
}
// A device error of an earlier pass is sticky for the run: its accumulator is poisoned.
int run_error(zrt_ctx* c) {
  c->render.reported = true;
  return fail(ZRT_E_UNSUPPORTED, zrt::device_error_msg(*c->render.err));
}
}  // namespace

int zrt_ctx_accum_begin(zrt_ctx* c, const zrt_camera* cam, const zrt_params* p) {
  if (!c || !cam) return fail(ZRT_E_INVALID, "null argument");
  int rc = zrt::validate_params(p);
  if (rc) return rc;
  rc = zrt::params_fit_ctx(c, p);
  if (rc) return rc;
  try {
    zrt::AccumRun& r = c->run;
    HIPCHK(hipSetDevice(c->device));
    r.live = false;
    r.accum.grow(uint64_t(zrt::rank_tiles(zrt::geometry(p), p->rank, p->world_size)) * 64u);
    r.metrics.grow(zrt::kMetricWords);
    r.metrics_host.alloc(zrt::kMetricWords);
    // (a restarted run's unread pass times are dropped; the accumulator, the counters
    // and the error flag are zeroed by the first pass, on its stream)
    for (zrt::EvSet& e : r.pending) r.spare.push_back(std::move(e));
    r.pending.clear();
    r.render_ms = r.sched_ms = 0.0;
    r.cam = *cam;
    r.p = *p;
    r.done = 0;
    r.passes = 0;
    r.ordered = false;
    c->adapt.on = false;
    r.live = true;
    return ZRT_OK;
  }
  ZRT_CATCH_ALL
}

int zrt_ctx_accum_pass(zrt_ctx* c, uint32_t n_samples, float* dev_tiles, void* hip_stream) {
  if (!c || !dev_tiles) return fail(ZRT_E_INVALID, "null argument");
  if (!c->run.live || c->adapt.on)
    return fail(ZRT_E_INVALID, "no accumulation run is live on this context (zrt_ctx_accum_begin; a "
                               "zrt_ctx_render_tiles ends the run)");
  if (c->run.passes > 0 && hipEventQuery(c->render.done) == hipSuccess && *c->render.err != 0) return run_error(c);
  (void)hipGetLastError();
  return zrt::launch_frame(c, &c->run.cam, &c->run.p, dev_tiles, hip_stream, true, n_samples);
}

int zrt_ctx_accum_info(zrt_ctx* c, zrt_pass_info* out) {
  if (!c || !out) return fail(ZRT_E_INVALID, "null argument");
  if (!c->render.launched || !c->last.run)
    return fail(ZRT_E_INVALID, "the context's last launch was not a zrt_ctx_accum_pass");
  try {
    HIPCHK(hipSetDevice(c->device));
    HIPCHK(hipEventSynchronize(c->render.done));
    std::memset(out, 0, sizeof(*out));
    out->samples_done = c->run.done;
    out->pass_samples = c->run.pass_samples;
    const Metrics m = reduce_metrics(c);
    out->changed_pixels = m.changed;
    std::memcpy(&out->max_abs_change, &m.max_bits, 4);
    const zrt::LaunchTimes t = zrt::launch_times(c->ev);
    out->render_ms = t.render_ms;
    out->schedule_ms = t.schedule_ms;
    return zrt::launch_status(c, true);
  }
  ZRT_CATCH_ALL
}

int zrt_ctx_adapt_begin(zrt_ctx* c, const zrt_camera* cam, const zrt_params* p, const zrt_adaptive* ad) {
  if (!c || !cam || !ad) return fail(ZRT_E_INVALID, "null argument");
  std::vector<uint32_t> levels;
  int rc = zrt::plan_adapt(p, ad, &levels);
  if (rc) return rc;
  rc = zrt_ctx_accum_begin(c, cam, p);  // the accumulator, the metrics, the run's state
  if (rc) return rc;
  try {
    zrt::AdaptRun& a = c->adapt;
    c->run.live = false;
    const uint32_t my_tiles = zrt::rank_tiles(zrt::geometry(p), p->rank, p->world_size);
    // (no level of an earlier run is in flight: zrt_ctx_adapt_level waits for its own)
    std::vector<uint32_t> ids(my_tiles);
    for (uint32_t i = 0; i < my_tiles; ++i) ids[i] = i;
    if (a.active[0].n < my_tiles || a.active[1].n < my_tiles || a.tile_done.n < my_tiles) {
      a.active[0].alloc(my_tiles);
      a.active[1].alloc(my_tiles);
      a.tile_done.alloc(my_tiles);
    }
    if (my_tiles)
      HIPCHK(hipMemcpy(a.active[0].p, ids.data(), size_t(my_tiles) * sizeof(uint32_t), hipMemcpyHostToDevice));
    a.active_count.grow(1);
    a.count_host.alloc();
    *a.count_host = 0;
    a.a = *ad;
    a.levels = levels;
    a.k = 0;
    a.cur = 0;
    a.n_active = my_tiles;
    a.samples = 0;
    a.tiles = nullptr;
    a.on = true;
    c->run.live = true;
    return ZRT_OK;
  }
  ZRT_CATCH_ALL
}

int zrt_ctx_adapt_level(zrt_ctx* c, float* dev_tiles, void* hip_stream, zrt_level_info* out) {
  if (!c || !dev_tiles) return fail(ZRT_E_INVALID, "null argument");
  zrt::AdaptRun& a = c->adapt;
  if (!c->run.live || !a.on)
    return fail(ZRT_E_INVALID, "no adaptive run is live on this context (zrt_ctx_adapt_begin; a "
                               "zrt_ctx_render_tiles ends the run)");
  // (every level is waited for)
  if (c->run.passes > 0 && *c->render.err != 0) return run_error(c);
  if (a.k >= a.levels.size()) return fail(ZRT_E_INVALID, "the adaptive run has rendered its last level");
  if (a.n_active == 0 && c->run.passes > 0) return fail(ZRT_E_INVALID, "no tile of the adaptive run is active");
  if (a.tiles && a.tiles != dev_tiles)
    return fail(ZRT_E_INVALID, "dev_tiles differs from the run's earlier levels' (frozen tiles live there)");
  const uint32_t level = a.levels[a.k], rendered = a.n_active;
  const uint32_t level_samples = level - c->run.done;
  const int rc = zrt::launch_frame(c, &c->run.cam, &c->run.p, dev_tiles, hip_stream, true, level_samples);
  if (rc) return rc;
  try {
    HIPCHK(hipEventSynchronize(c->render.done));  // the one wait of the level: the surviving count is here
    a.tiles = dev_tiles;
    a.k += 1;
    a.cur ^= 1u;
    a.n_active = a.k < a.levels.size() ? *a.count_host : 0u;
    const Metrics m = reduce_metrics(c);
    if (*c->render.err == 0) a.samples += m.pixels * level_samples;
    if (out) {
      std::memset(out, 0, sizeof(*out));
      out->level_samples = level;
      out->tiles_rendered = rendered;
      out->tiles_active_after = a.n_active;
      out->samples_rendered = m.pixels * level_samples;
      out->changed_pixels = m.changed;
      std::memcpy(&out->max_abs_change, &m.max_bits, 4);
      const zrt::LaunchTimes t = zrt::launch_times(c->ev);
      out->render_ms = t.render_ms;
      out->schedule_ms = t.schedule_ms;
    }
    return zrt::launch_status(c, true);
  }
  ZRT_CATCH_ALL
}

int zrt_ctx_adapt_samples(zrt_ctx* c, uint32_t* per_tile, uint32_t cap_tiles) {
  if (!c || !per_tile) return fail(ZRT_E_INVALID, "null argument");
  if (!c->run.live || !c->adapt.on) return fail(ZRT_E_INVALID, "no adaptive run is live on this context");
  const zrt_params& p = c->run.p;
  const uint32_t my_tiles = zrt::rank_tiles(zrt::geometry(&p), p.rank, p.world_size);
  if (cap_tiles < my_tiles) return fail(ZRT_E_INVALID, "per_tile holds fewer entries than the rank has tiles");
  try {
    HIPCHK(hipSetDevice(c->device));
    if (c->run.passes == 0) {
      std::fill(per_tile, per_tile + my_tiles, 0u);
      return ZRT_OK;
    }
    HIPCHK(hipEventSynchronize(c->render.done));
    if (my_tiles)
      HIPCHK(hipMemcpy(per_tile, c->adapt.tile_done.p, size_t(my_tiles) * sizeof(uint32_t), hipMemcpyDeviceToHost));
    for (uint32_t i = 0; i < my_tiles; ++i) per_tile[i] &= ~zrt::kTileFrozen;
    return ZRT_OK;
  }
  ZRT_CATCH_ALL
}

// ---- the variance plane of the live run (zrt.h "the variance plane") ----------
int zrt_ctx_accum_variance(zrt_ctx* c, float* dev_tiles_var, void* hip_stream) {
  if (!c || !dev_tiles_var) return fail(ZRT_E_INVALID, "null argument");
  if (!c->run.live)
    return fail(ZRT_E_INVALID, "no run is live on this context (zrt_ctx_accum_begin / zrt_ctx_adapt_begin; a "
                               "zrt_ctx_render_tiles ends the run)");
  if (c->run.passes == 0) return fail(ZRT_E_INVALID, "variance: the run has rendered no pass yet");
  try {
    HIPCHK(hipSetDevice(c->device));
    hipStream_t st = zrt::stream_of(c, hip_stream);
    const zrt_params* p = &c->run.p;
    const zrt::Geometry g = zrt::geometry(p);
    const uint32_t my_tiles = zrt::rank_tiles(g, p->rank, p->world_size);
    const uint32_t n_slots = my_tiles * 64u;
    HIPCHK(hipEventSynchronize(c->render.done));  // the last pass: its error flag, an adaptive run's tile counts
    const bool dev_err = *c->render.err != 0;
    std::vector<float2>& plan = c->var.host;
    plan.assign(std::max(1u, my_tiles), make_float2(0.0f, 0.0f));
    if (!dev_err) {
      zrt_variance_plan vp{};
      if (c->adapt.on) {
        std::vector<uint32_t> done(std::max(1u, my_tiles));
        if (my_tiles)
          HIPCHK(hipMemcpy(done.data(), c->adapt.tile_done.p, size_t(my_tiles) * sizeof(uint32_t),
                           hipMemcpyDeviceToHost));
        uint32_t last_n = 0;
        for (uint32_t lt = 0; lt < my_tiles; ++lt) {
          const uint32_t n = done[lt] & ~zrt::kTileFrozen;
          if (n != last_n) {  // (ik and sc per distinct k)
            const int rc = zrt::plan_variance(p, n, &vp);
            if (rc) return rc;
            last_n = n;
          }
          plan[lt] = make_float2(vp.ik, vp.sc);
        }
      } else {
        const int rc = zrt::plan_variance(p, c->run.done, &vp);
        if (rc) return rc;
        for (uint32_t lt = 0; lt < my_tiles; ++lt) plan[lt] = make_float2(vp.ik, vp.sc);
      }
    }
    c->var.dev.grow(plan.size());
    // (a blocking copy: the table may be rewritten by the next call)
    HIPCHK(hipMemcpy(c->var.dev.p, plan.data(), plan.size() * sizeof(float2), hipMemcpyHostToDevice));
    if (n_slots)
      HIPCHK(zrt::launch_variance(st, c->run.accum.p, c->var.dev.p, dev_tiles_var, n_slots, p->world_size, p->rank,
                                  g.tiles_x, g.xbound, p->height, c->scratch.p + zrt::kErrorSlot));
    if (dev_err) return run_error(c);
    return ZRT_OK;
  }
  ZRT_CATCH_ALL
}
