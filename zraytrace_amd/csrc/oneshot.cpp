// oneshot.cpp - the one-shot renders (zrt_render*): a context, the frame, the
// copy back.  They call the C ABI of context.cpp, runs.cpp and post.cpp and hold
// device buffers; nothing else.
#include <algorithm>
#include <cstring>
#include <functional>
#include <memory>

#include "context.hpp"

using zrt::fail;

namespace zrt {
namespace {
// What a one-shot render does with its assembled frame while it still lies on the
// device (zrt_render_denoised): called last, with the context, the params rendered
// with and the frame.
using FramePost = std::function<int(zrt_ctx*, const zrt_params&, const float*)>;

// One one-shot render: a context for the params as rank 0 of 1, its tile count and
// the tiles / frame device buffers (released before the context).  Its methods may
// throw HipError: a session lives inside its entry point's try block.
struct Session {
  zrt_params p{};
  std::unique_ptr<zrt_ctx, int (*)(zrt_ctx*)> ctx{nullptr, zrt_ctx_destroy};
  uint32_t n_tiles = 0;
  DevBuf<float> tiles, frame;

  zrt_ctx* c() const { return ctx.get(); }
  size_t px() const { return size_t(p.width) * p.height; }
  int open(const zrt_scene* scene, const zrt_params* params, uint32_t extra_flags = 0) {
    p = *params;
    p.rank = 0;
    p.world_size = 1;
    p.flags |= extra_flags;
    zrt_ctx* made = nullptr;
    int rc = zrt_ctx_create(scene, &p, &made);
    if (rc) return rc;
    ctx.reset(made);
    rc = zrt_ctx_tile_count(c(), &p, &n_tiles);
    if (rc) return rc;
    tiles.alloc(size_t(n_tiles) * 64 * 3);
    frame.alloc(px() * 3);
    return ZRT_OK;
  }
  // the frame from the tiles (q: the params they were rendered with), enqueued
  int assemble(const zrt_params& q) { return zrt_ctx_assemble(c(), &q, tiles.p, frame.p, nullptr); }
  // ... waited for and copied out (out may be null: the frame stays on the device)
  void copy_out(float* out) {
    HIPCHK(hipStreamSynchronize(c()->stream));
    if (out) HIPCHK(hipMemcpy(out, frame.p, sizeof(float) * 3 * px(), hipMemcpyDeviceToHost));
  }
  int fetch(float* out) {
    const int rc = assemble(p);
    if (rc) return rc;
    copy_out(out);
    return ZRT_OK;
  }
  // the stats (and the scanlines) of what the context rendered, then `post`
  int finish(zrt_stats* stats, zrt_scanline* rows = nullptr, const FramePost* post = nullptr) {
    zrt_stats s;
    int rc = zrt_ctx_stats(c(), &s);
    if (rc) return rc;
    if (rows) {
      std::memset(rows, 0, sizeof(zrt_scanline) * p.height);
      rc = add_scanlines(c(), rows, p.height);
      if (rc) return rc;
    }
    if (stats) *stats = s;
    return post ? (*post)(c(), p, frame.p) : ZRT_OK;
  }
};

// one_pass: the frame as an accumulation run of one pass - zrt_render's frame and counters,
// with the run (its accumulator and second moment) still live for `post`
int render_one(const zrt_scene* scene, const zrt_camera* camera, const zrt_params* params, float* out_rgb,
               zrt_stats* stats, zrt_scanline* rows, const FramePost* post = nullptr, bool one_pass = false) {
  if (!camera || (!out_rgb && !post)) return fail(ZRT_E_INVALID, "null argument");
  int rc = zrt::validate_params(params);
  if (rc) return rc;
  try {
    Session s;
    rc = s.open(scene, params, rows ? ZRT_FLAG_SCANLINES : 0u);
    if (rc) return rc;
    if (one_pass) rc = zrt_ctx_accum_begin(s.c(), camera, &s.p);
    if (rc) return rc;
    rc = one_pass ? zrt_ctx_accum_pass(s.c(), s.p.samples_per_pixel, s.tiles.p, nullptr)
                  : zrt_ctx_render_tiles(s.c(), camera, &s.p, s.tiles.p, nullptr);
    if (rc) return rc;
    rc = s.fetch(out_rgb);
    if (rc) return rc;
    return s.finish(stats, rows, post);
  }
  ZRT_CATCH_ALL
}
}  // namespace
}  // namespace zrt

int zrt_render(const zrt_scene* scene, const zrt_camera* camera, const zrt_params* params,
               float* out_rgb, zrt_stats* stats) {
  return zrt::render_one(scene, camera, params, out_rgb, stats, nullptr);
}

int zrt_render_progress(const zrt_scene* scene, const zrt_camera* camera, const zrt_params* params,
                        float* out_rgb, zrt_stats* stats, zrt_scanline* scanlines) {
  if (!scanlines) return fail(ZRT_E_INVALID, "null argument");
  return zrt::render_one(scene, camera, params, out_rgb, stats, scanlines);
}

int zrt_render_progressive(const zrt_scene* scene, const zrt_camera* camera, const zrt_params* params,
                           uint32_t pass_samples, zrt_pass_fn on_pass, void* user, float* out_rgb,
                           zrt_stats* stats) {
  if (!camera || !out_rgb) return fail(ZRT_E_INVALID, "null argument");
  int rc = zrt::validate_params(params);
  if (rc) return rc;
  const uint32_t chunk = params->sample_chunk ? params->sample_chunk : ZRT_DEFAULT_SAMPLE_CHUNK;
  // whole chunks per pass (a pass must start on a chunk boundary); 0: the default
  const uint64_t per_pass = pass_samples ? (uint64_t(pass_samples) + chunk - 1) / chunk * chunk
                                         : uint64_t(ZRT_DEFAULT_PASS_CHUNKS) * chunk;
  try {
    zrt::Session s;
    rc = s.open(scene, params);
    if (rc) return rc;
    const zrt_params& p = s.p;
    zrt_ctx* c = s.c();
    rc = zrt_ctx_accum_begin(c, camera, &p);
    if (rc) return rc;
    for (uint32_t done = 0; done < p.samples_per_pixel;) {
      const uint32_t n = uint32_t(std::min<uint64_t>(per_pass, p.samples_per_pixel - done));
      rc = zrt_ctx_accum_pass(c, n, s.tiles.p, nullptr);
      if (rc) return rc;
      rc = s.assemble(p);
      if (rc) return rc;
      done += n;
      if (!on_pass && done < p.samples_per_pixel) continue;  // nobody looks: the passes queue up
      s.copy_out(out_rgb);
      if (on_pass) {
        zrt_pass_info info;
        rc = zrt_ctx_accum_info(c, &info);
        if (rc) return rc;
        if (on_pass(user, out_rgb, &info) != 0) break;
      }
    }
    return s.finish(stats);
  }
  ZRT_CATCH_ALL
}

namespace zrt {
namespace {
int render_adaptive(const zrt_scene* scene, const zrt_camera* camera, const zrt_params* params,
                    const zrt_adaptive* adaptive, zrt_level_fn on_level, void* user, float* out_rgb,
                    uint32_t* out_samples, zrt_stats* stats, zrt_scanline* rows, const FramePost* post = nullptr) {
  if (!camera || (!out_rgb && !post) || !adaptive) return fail(ZRT_E_INVALID, "null argument");
  if (!out_rgb && on_level) return fail(ZRT_E_INVALID, "on_level needs out_rgb");
  std::vector<uint32_t> levels;
  int rc = zrt::plan_adapt(params, adaptive, &levels);
  if (rc) return rc;
  try {
    Session s;
    rc = s.open(scene, params, rows ? ZRT_FLAG_SCANLINES : 0u);
    if (rc) return rc;
    const zrt_params& p = s.p;
    zrt_ctx* c = s.c();
    HIPCHK(hipMemset(s.tiles.p, 0, sizeof(float) * s.tiles.n));
    rc = zrt_ctx_adapt_begin(c, camera, &p, adaptive);
    if (rc) return rc;
    for (size_t k = 0; k < levels.size(); ++k) {
      zrt_level_info info;
      rc = zrt_ctx_adapt_level(c, s.tiles.p, nullptr, &info);
      if (rc) return rc;
      const bool over = info.tiles_active_after == 0;
      if (on_level || over) {
        rc = s.fetch(out_rgb);
        if (rc) return rc;
      }
      if ((on_level && on_level(user, out_rgb, &info) != 0) || over) break;
    }
    if (out_samples) {
      std::vector<uint32_t> per_tile(std::max(1u, s.n_tiles));
      rc = zrt_ctx_adapt_samples(c, per_tile.data(), s.n_tiles);
      if (rc) return rc;
      const zrt::Geometry g = zrt::geometry(&p);
      std::fill(out_samples, out_samples + s.px(), 0u);
      for (uint32_t y = 0; y < p.height; ++y)
        for (uint32_t x = 0; x < g.xbound; ++x)
          out_samples[size_t(y) * p.width + x] = per_tile[(y / 8u) * g.tiles_x + x / 8u];
    }
    return s.finish(stats, rows, post);
  }
  ZRT_CATCH_ALL
}
}  // namespace
}  // namespace zrt

int zrt_render_adaptive(const zrt_scene* scene, const zrt_camera* camera, const zrt_params* params,
                        const zrt_adaptive* adaptive, zrt_level_fn on_level, void* user, float* out_rgb,
                        uint32_t* out_samples, zrt_stats* stats) {
  return zrt::render_adaptive(scene, camera, params, adaptive, on_level, user, out_rgb, out_samples, stats, nullptr);
}

int zrt_render_adaptive_progress(const zrt_scene* scene, const zrt_camera* camera, const zrt_params* params,
                                 const zrt_adaptive* adaptive, zrt_level_fn on_level, void* user, float* out_rgb,
                                 uint32_t* out_samples, zrt_stats* stats, zrt_scanline* scanlines) {
  if (!scanlines) return fail(ZRT_E_INVALID, "null argument");
  return zrt::render_adaptive(scene, camera, params, adaptive, on_level, user, out_rgb, out_samples, stats, scanlines);
}

namespace zrt {
namespace {
// The guided filter's settings (dn NULL: the defaults), refused before any device work.
int guided_settings(const zrt_params* params, const zrt_denoise* dn, uint32_t flags, zrt_denoise* d) {
  uint32_t default_flags = 0;
  if (dn) *d = *dn;
  else zrt_denoise_guided_defaults(d, &default_flags);
  DenoiseLaunch l{};
  const int rc = plan_denoise(params, d, &l);
  if (rc) return rc;
  if (flags & ~uint32_t(ZRT_DN_DEMODULATE)) return fail(ZRT_E_INVALID, "denoise: unknown flag");
  return ZRT_OK;
}

// zrt_render_denoised*'s FramePost: the frame's features and (guided) the live run's
// variance plane, the filter, and the copies out.
struct DenoisedOut {
  float *rgb, *features, *variance;
  double* ms;
};
int denoise_frame(zrt_ctx* c, const zrt_params& p, const zrt_camera* camera, const float* dev_frame,
                  const zrt_denoise& d, bool guided, uint32_t flags, const DenoisedOut& o) {
  try {
    const size_t px = size_t(p.width) * p.height;
    DevBuf<float> feat, outb, var_tiles, var;
    feat.alloc(px * 8);
    outb.alloc(px * 3);
    int r = ZRT_OK;
    if (guided) {
      uint32_t n_tiles = 0;
      r = zrt_ctx_tile_count(c, &p, &n_tiles);
      if (r) return r;
      var_tiles.alloc(size_t(n_tiles) * 64);
      var.alloc(px);
      r = zrt_ctx_accum_variance(c, var_tiles.p, nullptr);
      if (r) return r;
      r = zrt_ctx_assemble_plane(c, &p, var_tiles.p, 0, var.p, nullptr);
      if (r) return r;
    }
    r = zrt_ctx_features(c, camera, &p, feat.p, nullptr);
    if (r) return r;
    r = guided ? zrt_ctx_denoise_guided(c, &p, &d, flags, dev_frame, feat.p, var.p, outb.p, nullptr, nullptr)
               : zrt_ctx_denoise(c, &p, &d, dev_frame, feat.p, outb.p, nullptr);
    if (r) return r;
    HIPCHK(hipStreamSynchronize(c->stream));
    r = zrt_ctx_sync(c);  // (a feature launch's device error)
    if (r) return r;
    HIPCHK(hipMemcpy(o.rgb, outb.p, sizeof(float) * 3 * px, hipMemcpyDeviceToHost));
    if (o.features) HIPCHK(hipMemcpy(o.features, feat.p, sizeof(float) * 8 * px, hipMemcpyDeviceToHost));
    if (guided && o.variance) HIPCHK(hipMemcpy(o.variance, var.p, sizeof(float) * px, hipMemcpyDeviceToHost));
    return o.ms ? zrt_ctx_denoise_ms(c, o.ms) : ZRT_OK;
  }
  ZRT_CATCH_ALL
}
}  // namespace
}  // namespace zrt

int zrt_render_denoised_guided(const zrt_scene* scene, const zrt_camera* camera, const zrt_params* params,
                               const zrt_adaptive* adaptive, const zrt_denoise* dn, uint32_t flags, float* out_rgb,
                               float* out_noisy, float* out_features, float* out_variance, zrt_stats* stats,
                               double* denoise_ms) {
  if (!camera || !out_rgb) return fail(ZRT_E_INVALID, "null argument");
  zrt_denoise d;
  int rc = zrt::guided_settings(params, dn, flags, &d);
  if (rc) return rc;
  // every tile ends on whole chunks, two at least: a frozen tile holds a doubled level, the others the cap
  zrt_variance_plan vp{};
  rc = zrt::plan_variance(params, params->samples_per_pixel, &vp);
  if (rc) return rc;
  const zrt::FramePost post = [&](zrt_ctx* c, const zrt_params& p, const float* dev_frame) {
    return zrt::denoise_frame(c, p, camera, dev_frame, d, true, flags, {out_rgb, out_features, out_variance, denoise_ms});
  };
  if (adaptive)
    return zrt::render_adaptive(scene, camera, params, adaptive, nullptr, nullptr, out_noisy, nullptr, stats, nullptr,
                                &post);
  return zrt::render_one(scene, camera, params, out_noisy, stats, nullptr, &post, true);
}

int zrt_render_denoised(const zrt_scene* scene, const zrt_camera* camera, const zrt_params* params,
                        const zrt_adaptive* adaptive, const zrt_denoise* dn, float* out_rgb, float* out_noisy,
                        float* out_features, zrt_stats* stats, double* denoise_ms) {
  if (!camera || !out_rgb) return fail(ZRT_E_INVALID, "null argument");
  zrt_denoise d;
  if (dn) d = *dn;
  else zrt_denoise_defaults(&d);
  zrt::DenoiseLaunch l{};
  int rc = zrt::plan_denoise(params, &d, &l);  // (refused before any device work)
  if (rc) return rc;
  const zrt::FramePost post = [&](zrt_ctx* c, const zrt_params& p, const float* dev_frame) {
    return zrt::denoise_frame(c, p, camera, dev_frame, d, false, 0, {out_rgb, out_features, nullptr, denoise_ms});
  };
  if (adaptive)
    return zrt::render_adaptive(scene, camera, params, adaptive, nullptr, nullptr, out_noisy, nullptr, stats, nullptr,
                                &post);
  return zrt::render_one(scene, camera, params, out_noisy, stats, nullptr, &post);
}

// A sequence of frames of one scene through the temporal step and the guided filter
// (zrt.h "temporal accumulation"): one context, one set of device buffers, frame k
// an accumulation run of one pass with seed + k.
int zrt_render_temporal(const zrt_scene* scene, const zrt_camera* cameras, uint32_t n_frames,
                        const zrt_params* params, const zrt_temporal* tp, const zrt_denoise* dn, uint32_t dn_flags,
                        zrt_frame_fn on_frame, void* user, float* out_rgb, zrt_stats* stats) {
  if (!cameras || !out_rgb) return fail(ZRT_E_INVALID, "null argument");
  zrt_denoise d;
  int rc = zrt::guided_settings(params, dn, dn_flags, &d);
  if (rc) return rc;
  zrt_temporal t;
  if (tp) t = *tp;
  else zrt_temporal_defaults(&t);
  zrt::TemporalLaunch tl{};
  rc = zrt::plan_temporal(params, &t, &tl);
  if (rc) return rc;
  zrt_variance_plan vp{};
  rc = zrt::plan_variance(params, params->samples_per_pixel, &vp);
  if (rc) return rc;
  if (n_frames == 0) return fail(ZRT_E_INVALID, "temporal: n_frames must be > 0");
  try {
    zrt::Session s;
    rc = s.open(scene, params);
    if (rc) return rc;
    const zrt_params& p = s.p;
    zrt_ctx* c = s.c();
    const size_t px = s.px();
    zrt::DevBuf<float> feat, var_tiles, var, acc, acc_var, outb;
    feat.alloc(px * 8);
    var_tiles.alloc(size_t(s.n_tiles) * 64);
    var.alloc(px);
    acc.alloc(px * 3);
    acc_var.alloc(px);
    outb.alloc(px * 3);
    for (uint32_t k = 0; k < n_frames; ++k) {
      zrt_params pk = p;
      pk.seed = p.seed + k;  // the blend's variance assumes independent frames
      const zrt_camera* cam = &cameras[k];
      rc = zrt_ctx_accum_begin(c, cam, &pk);
      if (rc) return rc;
      rc = zrt_ctx_accum_pass(c, pk.samples_per_pixel, s.tiles.p, nullptr);
      if (rc) return rc;
      rc = zrt_ctx_accum_variance(c, var_tiles.p, nullptr);
      if (rc) return rc;
      rc = s.assemble(pk);
      if (rc) return rc;
      rc = zrt_ctx_assemble_plane(c, &pk, var_tiles.p, 0, var.p, nullptr);
      if (rc) return rc;
      rc = zrt_ctx_features(c, cam, &pk, feat.p, nullptr);
      if (rc) return rc;
      rc = zrt_ctx_temporal(c, cam, &pk, &t, s.frame.p, feat.p, var.p, acc.p, acc_var.p, nullptr, nullptr);
      if (rc) return rc;
      rc = zrt_ctx_denoise_guided(c, &pk, &d, dn_flags, acc.p, feat.p, acc_var.p, outb.p, nullptr, nullptr);
      if (rc) return rc;
      if (!on_frame && k + 1 < n_frames) continue;  // nobody looks: the frames queue up
      HIPCHK(hipStreamSynchronize(c->stream));
      rc = zrt_ctx_sync(c);  // (a feature launch's device error)
      if (rc) return rc;
      HIPCHK(hipMemcpy(out_rgb, outb.p, sizeof(float) * 3 * px, hipMemcpyDeviceToHost));
      if (on_frame && on_frame(user, out_rgb, k) != 0) break;
    }
    return s.finish(stats);
  }
  ZRT_CATCH_ALL
}

// The AO plane of a frame (zrt.h "ambient occlusion"): a context, the first-hit features,
// the AO call, the copies out.  Under ZRT_AO_ACCUMULATE the counts start from out_clear's
// contents (zero without it).
int zrt_render_ao(const zrt_scene* scene, const zrt_camera* camera, const zrt_params* params, const zrt_ao* ao,
                  float* out_ao, uint32_t* out_clear, float* out_features) {
  if (!camera || !out_ao) return fail(ZRT_E_INVALID, "null argument");
  zrt_ao_plan plan;
  int rc = zrt::plan_ao(params, ao, 1, &plan);  // (refused before any device work)
  if (rc) return rc;
  try {
    zrt::Session s;
    rc = s.open(scene, params);
    if (rc) return rc;
    zrt_ctx* c = s.c();
    const size_t px = s.px();
    zrt::DevBuf<float> feat, plane;
    zrt::DevBuf<uint32_t> clear;
    feat.alloc(px * 8);
    plane.alloc(px);
    clear.alloc(px);
    if ((ao->flags & ZRT_AO_ACCUMULATE) && out_clear)
      HIPCHK(hipMemcpy(clear.p, out_clear, sizeof(uint32_t) * px, hipMemcpyHostToDevice));
    else
      HIPCHK(hipMemset(clear.p, 0, sizeof(uint32_t) * px));
    rc = zrt_ctx_features(c, camera, &s.p, feat.p, nullptr);
    if (rc) return rc;
    rc = zrt_ctx_ao(c, camera, &s.p, ao, feat.p, clear.p, plane.p, nullptr);
    if (rc) return rc;
    HIPCHK(hipStreamSynchronize(c->stream));
    rc = zrt_ctx_sync(c);  // (a device error of either launch)
    if (rc) return rc;
    HIPCHK(hipMemcpy(out_ao, plane.p, sizeof(float) * px, hipMemcpyDeviceToHost));
    if (out_clear) HIPCHK(hipMemcpy(out_clear, clear.p, sizeof(uint32_t) * px, hipMemcpyDeviceToHost));
    if (out_features) HIPCHK(hipMemcpy(out_features, feat.p, sizeof(float) * 8 * px, hipMemcpyDeviceToHost));
    return ZRT_OK;
  }
  ZRT_CATCH_ALL
}

int zrt_radiance(const zrt_scene* scene, const zrt_params* params, const struct zrt_radiance* rq, const float* rays,
                 uint32_t n, float* sum, float* out_rgb, zrt_radiance_info* info) {
  zrt_radiance_plan plan;
  int rc = zrt::plan_radiance(params, rq, n, 1, 0, &plan);  // (refused before any device work)
  if (rc) return rc;
  if (n && !rays) return fail(ZRT_E_INVALID, "null argument");
  rc = zrt::validate_scene(scene);
  if (rc) return rc;
  rc = zrt::check_device(int(params->device));
  if (rc) return rc;
  if (n == 0) {
    if (info) *info = zrt_radiance_info{};
    return ZRT_OK;
  }
  try {
    const bool use_bvh = params->bounded_volume_hierarchy != 0 && scene->n_prims > 10;
    zrt::HostScene h;
    zrt::flatten_for_device(&h, scene, use_bvh, int(params->device));
    std::unique_ptr<zrt_ctx> c = zrt::ctx_on_device(h, int(params->device));
    zrt::DevBuf<float> d_rays, d_rgb;
    zrt::DevBuf<float4> d_sum;
    d_rays.alloc(6ull * n);
    d_sum.alloc(n);
    d_rgb.alloc(3ull * n);
    HIPCHK(hipMemcpy(d_rays.p, rays, sizeof(float) * 6ull * n, hipMemcpyHostToDevice));
    if ((rq->flags & ZRT_RQ_ACCUMULATE) && sum)
      HIPCHK(hipMemcpy(d_sum.p, sum, sizeof(float4) * n, hipMemcpyHostToDevice));
    else
      HIPCHK(hipMemset(d_sum.p, 0, sizeof(float4) * n));
    rc = zrt_ctx_radiance(c.get(), params, rq, d_rays.p, n, reinterpret_cast<float*>(d_sum.p), d_rgb.p, nullptr);
    if (rc) return rc;
    rc = zrt_ctx_sync(c.get());  // (a device error of the launch)
    if (rc) return rc;
    if (sum) HIPCHK(hipMemcpy(sum, d_sum.p, sizeof(float4) * n, hipMemcpyDeviceToHost));
    if (out_rgb) HIPCHK(hipMemcpy(out_rgb, d_rgb.p, sizeof(float) * 3ull * n, hipMemcpyDeviceToHost));
    if (info) return zrt_ctx_radiance_info(c.get(), info);
    return ZRT_OK;
  }
  ZRT_CATCH_ALL
}

int zrt_render_lens(const zrt_scene* scene, const zrt_params* params, const zrt_lens* lens, const zrt_camera_query* query,
                    float* sum, float* out_rgb, zrt_radiance_info* info) {
  zrt_camera_plan plan;
  int rc = zrt::plan_camera(params, query, 1, 0, &plan);  // (refused before any device work)
  if (rc) return rc;
  rc = zrt::check_lens(lens);
  if (rc) return rc;
  rc = zrt::validate_scene(scene);
  if (rc) return rc;
  rc = zrt::check_device(int(params->device));
  if (rc) return rc;
  try {
    const bool use_bvh = params->bounded_volume_hierarchy != 0 && scene->n_prims > 10;
    zrt::HostScene h;
    zrt::flatten_for_device(&h, scene, use_bvh, int(params->device));
    std::unique_ptr<zrt_ctx> c = zrt::ctx_on_device(h, int(params->device));
    const uint64_t n = uint64_t(params->width) * params->height;  // whole-frame buffers
    zrt::DevBuf<float> d_rgb;
    zrt::DevBuf<float4> d_sum;
    d_sum.alloc(n);
    d_rgb.alloc(3ull * n);
    // what the caller holds outside the rectangle (and, accumulating, inside) goes in first
    if (sum)
      HIPCHK(hipMemcpy(d_sum.p, sum, sizeof(float4) * n, hipMemcpyHostToDevice));
    else
      HIPCHK(hipMemset(d_sum.p, 0, sizeof(float4) * n));
    if (out_rgb)
      HIPCHK(hipMemcpy(d_rgb.p, out_rgb, sizeof(float) * 3ull * n, hipMemcpyHostToDevice));
    rc = zrt_ctx_camera(c.get(), params, lens, query, reinterpret_cast<float*>(d_sum.p), d_rgb.p, nullptr);
    if (rc) return rc;
    rc = zrt_ctx_sync(c.get());  // (a device error of the launch)
    if (rc) return rc;
    if (sum) HIPCHK(hipMemcpy(sum, d_sum.p, sizeof(float4) * n, hipMemcpyDeviceToHost));
    if (out_rgb) HIPCHK(hipMemcpy(out_rgb, d_rgb.p, sizeof(float) * 3ull * n, hipMemcpyDeviceToHost));
    if (info) return zrt_ctx_camera_info(c.get(), info);
    return ZRT_OK;
  }
  ZRT_CATCH_ALL
}

// A lens frame through the post chain (zrt.h "denoising lens frames"): the camera query (with
// moments for the guided filter), lens features, the variance plane and the filter over the
// query's rectangle, on one context; every device buffer starts zeroed.
int zrt_render_lens_denoised(const zrt_scene* scene, const zrt_params* params, const zrt_lens* lens,
                             const zrt_camera_query* query, const zrt_denoise* dn, uint32_t guided, uint32_t flags,
                             float* out_rgb, float* out_noisy, float* out_features, float* out_variance,
                             zrt_radiance_info* info, double* denoise_ms) {
  zrt_camera_plan plan;
  int rc = zrt::plan_camera(params, query, 1, 0, &plan);  // (refused before any device work)
  if (rc) return rc;
  rc = zrt::check_lens(lens);
  if (rc) return rc;
  const zrt_rect rect{query->x0, query->y0, query->w, query->h};
  zrt_denoise d;
  uint32_t default_flags = 0;
  if (dn) d = *dn;
  else if (guided) zrt_denoise_guided_defaults(&d, &default_flags);
  else zrt_denoise_defaults(&d);
  zrt::DenoiseLaunch l{};
  rc = zrt::plan_denoise_rect(params, &d, &rect, &l);
  if (rc) return rc;
  if (flags & ~uint32_t(ZRT_DN_DEMODULATE)) return fail(ZRT_E_INVALID, "denoise: unknown flag");
  if (!guided && flags) return fail(ZRT_E_INVALID, "denoise: flags need the guided filter");
  if (guided) {
    zrt_variance_plan vp{};
    rc = zrt::plan_camera_variance(params, &rect, query->n_samples, &vp);
    if (rc) return rc;
  }
  if (!out_rgb) return fail(ZRT_E_INVALID, "null argument");
  rc = zrt::validate_scene(scene);
  if (rc) return rc;
  rc = zrt::check_device(int(params->device));
  if (rc) return rc;
  try {
    const bool use_bvh = params->bounded_volume_hierarchy != 0 && scene->n_prims > 10;
    zrt::HostScene h;
    zrt::flatten_for_device(&h, scene, use_bvh, int(params->device));
    std::unique_ptr<zrt_ctx> ctx = zrt::ctx_on_device(h, int(params->device));
    zrt_ctx* c = ctx.get();
    const uint64_t n = uint64_t(params->width) * params->height;  // whole-frame buffers
    zrt::DevBuf<float> d_rgb, d_feat, d_var, d_out;
    zrt::DevBuf<float4> d_sum;
    d_sum.alloc(n);
    d_rgb.alloc(3ull * n);
    d_feat.alloc(8ull * n);
    d_out.alloc(3ull * n);
    HIPCHK(hipMemset(d_sum.p, 0, sizeof(float4) * n));
    HIPCHK(hipMemset(d_rgb.p, 0, sizeof(float) * 3ull * n));
    HIPCHK(hipMemset(d_feat.p, 0, sizeof(float) * 8ull * n));
    if (guided) {
      d_var.alloc(n);
      HIPCHK(hipMemset(d_var.p, 0, sizeof(float) * n));
    }
    float* sum = reinterpret_cast<float*>(d_sum.p);
    rc = guided ? zrt_ctx_camera_moments(c, params, lens, query, sum, d_rgb.p, nullptr)
                : zrt_ctx_camera(c, params, lens, query, sum, d_rgb.p, nullptr);
    if (rc) return rc;
    rc = zrt_ctx_sync(c);  // (a device error of the query; one query is in flight per context)
    if (rc) return rc;
    if (info) {
      rc = zrt_ctx_camera_info(c, info);
      if (rc) return rc;
    }
    rc = zrt_ctx_camera_features(c, params, lens, &rect, d_feat.p, nullptr);
    if (rc) return rc;
    if (guided) {
      rc = zrt_ctx_camera_variance(c, params, &rect, query->n_samples, sum, d_var.p, nullptr);
      if (rc) return rc;
    }
    rc = zrt_ctx_denoise_rect(c, params, &d, flags, &rect, d_rgb.p, d_feat.p, guided ? d_var.p : nullptr, d_out.p,
                              nullptr, nullptr);
    if (rc) return rc;
    HIPCHK(hipStreamSynchronize(c->stream));
    rc = zrt_ctx_sync(c);  // (the feature launch's device error)
    if (rc) return rc;
    HIPCHK(hipMemcpy(out_rgb, d_out.p, sizeof(float) * 3ull * n, hipMemcpyDeviceToHost));
    if (out_noisy) HIPCHK(hipMemcpy(out_noisy, d_rgb.p, sizeof(float) * 3ull * n, hipMemcpyDeviceToHost));
    if (out_features) HIPCHK(hipMemcpy(out_features, d_feat.p, sizeof(float) * 8ull * n, hipMemcpyDeviceToHost));
    if (guided && out_variance) HIPCHK(hipMemcpy(out_variance, d_var.p, sizeof(float) * n, hipMemcpyDeviceToHost));
    return denoise_ms ? zrt_ctx_denoise_ms(c, denoise_ms) : ZRT_OK;
  }
  ZRT_CATCH_ALL
}
