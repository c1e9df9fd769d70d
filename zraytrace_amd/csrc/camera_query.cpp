// camera_query.cpp - camera queries on a resident context (zrt.h "camera queries"): what
// zrt_ctx_camera refuses, how it launches (plan_camera: the rectangle's slots and
// plan_radiance over them, which zrt_debug_camera_plan reports with no device), the lens of
// a pose (zrt_lens_init), and the launch itself: per round camera_kernel over a bounded
// grid, then camera_finish_kernel folding the round's parked chunk sums into the frame's
// sums.  A camera query is a query (queries.cpp) and shares the radiance query's state
// (radiance.cpp): rows, parked sums, counters.
// zrt_ctx_camera_moments is the same launch with Q, the second moment of the chunk sums, kept
// in sum.w by the finishing kernel; zrt_ctx_camera_features is a query of one lane per slot
// (lens_features_kernel): the first-hit features along the lens model's centre rays.
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
int check_lens(const zrt_lens* l) {
  if (!l) return fail(ZRT_E_INVALID, "null argument");
  if (l->kind > ZRT_LENS_FISHEYE) return fail(ZRT_E_INVALID, "camera: unknown lens kind");
  const zrt_vec3* vs[] = {&l->origin, &l->lower_left_corner, &l->horizontal, &l->vertical,
                          &l->axis_u, &l->axis_v,            &l->axis_w};
  for (const zrt_vec3* v : vs)
    if (!std::isfinite(v->x) || !std::isfinite(v->y) || !std::isfinite(v->z))
      return fail(ZRT_E_INVALID, "camera: a lens float is not finite");
  if (!std::isfinite(l->half_fov) || !(l->half_fov > 0.0f))
    return fail(ZRT_E_INVALID, "camera: half_fov must be finite and > 0");
  return ZRT_OK;
}

int plan_camera(const zrt_params* p, const zrt_camera_query* cq, uint32_t cu_count, uint64_t partial_cap,
                zrt_camera_plan* out) {
  if (!p || !cq || !out) return fail(ZRT_E_INVALID, "null argument");
  if (p->width == 0 || p->height == 0 || p->width > 65535 || p->height > 65535)
    return fail(ZRT_E_INVALID, "camera: width and height must be 1 .. 65535");
  if (cq->w == 0 || cq->h == 0) return fail(ZRT_E_INVALID, "camera: the rectangle is empty");
  if (cq->x0 >= p->width || cq->w > p->width - cq->x0 || cq->y0 >= p->height || cq->h > p->height - cq->y0)
    return fail(ZRT_E_INVALID, "camera: the rectangle leaves the frame");
  if (cq->flags & ~uint32_t(ZRT_CQ_ACCUMULATE)) return fail(ZRT_E_INVALID, "camera: unknown flag");
  *out = zrt_camera_plan{};
  out->tiles_w = (cq->w + 7u) / 8u;
  out->tiles_h = (cq->h + 7u) / 8u;
  out->slots = uint64_t(out->tiles_w) * out->tiles_h * 64u;
  out->pixels = uint64_t(cq->w) * cq->h;
  // (unreachable while width and height are 16-bit; kept with the 32-bit n it guards)
  if (out->slots >= (1ull << 32)) return fail(ZRT_E_INVALID, "camera: the rectangle's slots do not fit 32 bits");
  struct zrt_radiance rq {};
  rq.n_samples = cq->n_samples;
  rq.first_sample = cq->first_sample;
  rq.flags = (cq->flags & ZRT_CQ_ACCUMULATE) ? uint32_t(ZRT_RQ_ACCUMULATE) : 0u;
  return plan_radiance(p, &rq, uint32_t(out->slots), cu_count, partial_cap, &out->radiance);
}
}  // namespace zrt

int zrt_lens_check(const zrt_lens* lens) { return zrt::check_lens(lens); }

int zrt_lens_init(uint32_t kind, const float look_from[3], const float look_at[3], const float vup[3], float vfov_deg,
                  float aspect, float aperture, float focus_dist, float fisheye_fov_deg, zrt_lens* out) {
  using zrt::Vec3;
  if (!look_from || !look_at || !vup || !out) return fail(ZRT_E_INVALID, "null argument");
  if (kind > ZRT_LENS_FISHEYE) return fail(ZRT_E_INVALID, "camera: unknown lens kind");
  // Camera.init's u, v, w and h (camera.zig:17-35), as zrt::Camera::init computes them
  auto unit = [](Vec3 v) {
    const float l = std::sqrt(v.x * v.x + v.y * v.y + v.z * v.z);
    return Vec3{v.x / l, v.y / l, v.z / l};
  };
  auto cross = [](Vec3 u, Vec3 v) { return Vec3{u.y * v.z - u.z * v.y, u.z * v.x - u.x * v.z, u.x * v.y - u.y * v.x}; };
  auto abi = [](Vec3 v) { return zrt_vec3{v.x, v.y, v.z}; };
  const Vec3 from{look_from[0], look_from[1], look_from[2]}, at{look_at[0], look_at[1], look_at[2]};
  const float theta = float(M_PI) * vfov_deg / 180.0f;
  const float h = std::tan(theta / 2.0f);
  const float viewport_height = 2.0f * h;
  const float viewport_width = aspect * viewport_height;
  const Vec3 w = unit(from.minus(at));
  const Vec3 u = unit(cross(Vec3{vup[0], vup[1], vup[2]}, w));
  const Vec3 v = cross(w, u);
  zrt_lens l{};
  l.kind = kind;
  const Vec3 hor = u.scale(focus_dist * viewport_width), ver = v.scale(focus_dist * viewport_height);
  l.origin = abi(from);
  l.horizontal = abi(hor);
  l.vertical = abi(ver);
  l.lower_left_corner = abi(from.minus(hor.scale(0.5f)).minus(ver.scale(0.5f)).minus(w.scale(focus_dist)));
  const bool frame = kind == ZRT_LENS_ORTHO || kind == ZRT_LENS_FISHEYE;
  l.axis_u = abi(frame ? u : u.scale(aperture * 0.5f));
  l.axis_v = abi(frame ? v : v.scale(aperture * 0.5f));
  l.axis_w = abi(Vec3{-w.x, -w.y, -w.z});
  l.half_fov = fisheye_fov_deg * (float(M_PI) / 360.0f);
  const int rc = zrt::check_lens(&l);
  if (rc) return rc;
  *out = l;
  return ZRT_OK;
}

int zrt_lens_from_camera(uint32_t kind, const zrt_camera* cam, float aperture, float focus_dist, float fisheye_fov_deg,
                         zrt_lens* out) {
  using zrt::Vec3;
  if (!cam || !out) return fail(ZRT_E_INVALID, "null argument");
  if (kind > ZRT_LENS_FISHEYE) return fail(ZRT_E_INVALID, "camera: unknown lens kind");
  auto in = [](const zrt_vec3& v) { return Vec3{v.x, v.y, v.z}; };
  auto abi = [](Vec3 v) { return zrt_vec3{v.x, v.y, v.z}; };
  auto len = [](Vec3 v) { return std::sqrt(v.x * v.x + v.y * v.y + v.z * v.z); };
  const Vec3 org = in(cam->origin), llc = in(cam->lower_left_corner), hor = in(cam->horizontal), ver = in(cam->vertical);
  const Vec3 axis = llc.plus(hor.scale(0.5f)).plus(ver.scale(0.5f)).minus(org);  // to the plane's centre
  const float dist = len(axis);
  const Vec3 fwd = axis.scale(1.0f / dist), u = hor.scale(1.0f / len(hor)), v = ver.scale(1.0f / len(ver));
  zrt_lens l{};
  l.kind = kind;
  l.origin = cam->origin;
  if (focus_dist > 0.0f) {
    const float s = focus_dist / dist;
    const Vec3 h2 = hor.scale(s), v2 = ver.scale(s);
    l.horizontal = abi(h2);
    l.vertical = abi(v2);
    l.lower_left_corner = abi(org.minus(h2.scale(0.5f)).minus(v2.scale(0.5f)).plus(fwd.scale(focus_dist)));
  } else {
    l.lower_left_corner = cam->lower_left_corner;
    l.horizontal = cam->horizontal;
    l.vertical = cam->vertical;
  }
  const bool frame = kind == ZRT_LENS_ORTHO || kind == ZRT_LENS_FISHEYE;
  l.axis_u = abi(frame ? u : u.scale(aperture * 0.5f));
  l.axis_v = abi(frame ? v : v.scale(aperture * 0.5f));
  l.axis_w = abi(fwd);
  l.half_fov = fisheye_fov_deg * (float(M_PI) / 360.0f);
  const int rc = zrt::check_lens(&l);
  if (rc) return rc;
  *out = l;
  return ZRT_OK;
}

#ifndef ZRT_PLAN_ONLY
namespace {
// The lens and the rectangle's slots in the kernels' arguments (the sample fields stay the caller's).
void fill_lens_args(zrt::CameraArgs& g, const zrt_params* p, const zrt_lens* lens, uint32_t x0, uint32_t y0, uint32_t w,
                    uint32_t h) {
  g.x0 = x0;
  g.y0 = y0;
  g.w = w;
  g.h = h;
  g.tiles_w = (w + 7u) / 8u;
  g.n = g.tiles_w * ((h + 7u) / 8u) * 64u;
  g.width = p->width;
  g.kind = lens->kind;
  g.f_width = float(p->width);
  g.f_height = float(p->height);
  g.half_fov = lens->half_fov;
  zrt::copy3(g.org, lens->origin);
  zrt::copy3(g.llc, lens->lower_left_corner);
  zrt::copy3(g.hor, lens->horizontal);
  zrt::copy3(g.ver, lens->vertical);
  zrt::copy3(g.au, lens->axis_u);
  zrt::copy3(g.av, lens->axis_v);
  zrt::copy3(g.aw, lens->axis_w);
}

// zrt_ctx_camera, and with moments zrt_ctx_camera_moments: sum.w carries Q.
int camera_launch(zrt_ctx* c, const zrt_params* p, const zrt_lens* lens, const zrt_camera_query* cq, float* dev_sum,
                  float* dev_rgb, void* hip_stream, bool with_moments) {
  if (!c) return fail(ZRT_E_INVALID, "null argument");
  zrt_camera_plan cplan;
  int rc = zrt::plan_camera(p, cq, uint32_t(std::max(1, c->cu_count)), zrt::query_env_u64("ZRT_RADIANCE_PARTIAL_CAP"),
                            &cplan);
  if (rc) return rc;
  rc = zrt::check_lens(lens);
  if (rc) return rc;
  rc = zrt::params_fit_ctx(c, p);
  if (rc) return rc;
  if (!dev_sum) return fail(ZRT_E_INVALID, "null argument");
  if (zrt::ptr_misaligned(dev_rgb, 4)) return fail(ZRT_E_INVALID, "camera: dev_rgb must be 4-byte aligned");
  if (zrt::ptr_misaligned(dev_sum, 16)) return fail(ZRT_E_INVALID, "camera: dev_sum must be 16-byte aligned");
  const zrt_radiance_plan& plan = cplan.radiance;
  const uint32_t n = uint32_t(cplan.slots);
  try {
    HIPCHK(hipSetDevice(c->device));
    hipStream_t st = zrt::stream_of(c, hip_stream);
    zrt::QueryState& q = c->query;
    const uint32_t grid = zrt::prepare_radiance(c, p, plan, st);
    const bool accumulate = (cq->flags & ZRT_CQ_ACCUMULATE) != 0;
    const uint32_t total = accumulate ? cq->first_sample + cq->n_samples : cq->n_samples;
    const float scale = 1.0f / float(total);  // raytrace.zig:157
    float4* sum = reinterpret_cast<float4*>(dev_sum);
    zrt::CameraArgs g{};
    g.key_offset = plan.key_offset;
    g.chunk = std::min<uint32_t>(plan.chunk, 65536u);
    g.sample_end = cq->first_sample + cq->n_samples;
    fill_lens_args(g, p, lens, cq->x0, cq->y0, cq->w, cq->h);
    // the call's whole chunks, which go into Q: all of them but a ragged last one
    const uint32_t moments = with_moments ? 1u : 0u, whole_chunks = cq->n_samples / plan.chunk;
    zrt::launch_query(
        c, p, grid, st, true, "camera query",
        [&](zrt::KArgs& a, const zrt::TracePlan& t, uint32_t launch_grid, hipStream_t s) {
          zrt::fill_radiance(c, p, a, t, launch_grid, "camera query");
          void* kernel = zrt::camera_kernel_ptr(t.kmode, p->prng, t.stk16);
          zrt::radiance_rounds(plan, n, cq->first_sample, g.chunk, launch_grid,
                               [&](uint32_t r, uint32_t chunks, uint64_t n_items, uint32_t sample0, uint32_t round_grid) {
                                 g.n_items = n_items;
                                 g.sample0 = sample0;
                                 void* args[] = {&a, &g};
                                 HIPCHK(hipLaunchKernel(kernel, dim3(round_grid), dim3(zrt::kBlock), args, t.lp.bytes, s));
                                 const uint32_t chunk0 = r * plan.chunks_per_round;
                                 const uint32_t q_chunks = whole_chunks > chunk0 ? std::min(chunks, whole_chunks - chunk0) : 0u;
                                 HIPCHK(zrt::launch_camera_finish(s, q.partial.p, g, chunks, r == 0 && !accumulate ? 1u : 0u,
                                                                  sum, nullptr, 0.0f, 0u, q.err.p, moments, q_chunks));
                               });
        },
        [&](hipStream_t s, const unsigned long long* err) {
          HIPCHK(zrt::launch_camera_finish(s, q.partial.p, g, 0u, 0u, sum, dev_rgb, scale, 1u, err, moments, 0u));
          zrt::copy_radiance_counters(c, s);
        },
        p->max_depth);
    q.rq_samples = cplan.pixels * cq->n_samples;
    q.cq_launched = q.rq_launched = true;  // (the two queries share their state: see zrt.h)
    return ZRT_OK;
  }
  ZRT_CATCH_ALL
}
}  // namespace

int zrt_ctx_camera(zrt_ctx* c, const zrt_params* p, const zrt_lens* lens, const zrt_camera_query* cq, float* dev_sum,
                   float* dev_rgb, void* hip_stream) {
  return camera_launch(c, p, lens, cq, dev_sum, dev_rgb, hip_stream, false);
}

int zrt_ctx_camera_moments(zrt_ctx* c, const zrt_params* p, const zrt_lens* lens, const zrt_camera_query* cq,
                           float* dev_sum, float* dev_rgb, void* hip_stream) {
  return camera_launch(c, p, lens, cq, dev_sum, dev_rgb, hip_stream, true);
}

// ---- lens features (zrt.h "denoising lens frames"): a query, one lane per slot of the rectangle ----
int zrt_ctx_camera_features(zrt_ctx* c, const zrt_params* p, const zrt_lens* lens, const zrt_rect* rect,
                            float* dev_features, void* hip_stream) {
  if (!c) return fail(ZRT_E_INVALID, "null argument");
  int rc = zrt::check_rect(p, rect);
  if (rc) return rc;
  rc = zrt::check_lens(lens);
  if (rc) return rc;
  rc = zrt::params_fit_ctx(c, p);
  if (rc) return rc;
  if (!dev_features) return fail(ZRT_E_INVALID, "null argument");
  if (zrt::ptr_misaligned(dev_features, 16))
    return fail(ZRT_E_INVALID, "camera features: dev_features must be 16-byte aligned");
  try {
    HIPCHK(hipSetDevice(c->device));
    hipStream_t st = zrt::stream_of(c, hip_stream);
    const uint32_t* sp = zrt::slot_prim_table(c);
    zrt::CameraArgs g{};
    fill_lens_args(g, p, lens, rect->x0, rect->y0, rect->w, rect->h);  // (16-bit extents: the slots fit 32 bits)
    float4* out = reinterpret_cast<float4*>(dev_features);
    zrt::launch_query(
        c, p, zrt::query_grid(g.n), st, true, "lens feature query",
        [&](zrt::KArgs& a, const zrt::TracePlan& t, uint32_t grid, hipStream_t s) {
          void* args[] = {&a, &g, &sp, &out};
          HIPCHK(hipLaunchKernel(zrt::lens_features_kernel_ptr(t.kmode, t.stk16), dim3(grid), dim3(zrt::kBlock), args,
                                 t.lp.bytes, s));
        },
        [&](hipStream_t s, const unsigned long long* err) { HIPCHK(zrt::launch_lens_features_error(s, out, g, err)); });
    return ZRT_OK;
  }
  ZRT_CATCH_ALL
}

int zrt_ctx_camera_info(zrt_ctx* c, zrt_radiance_info* out) {
  if (!c || !out) return fail(ZRT_E_INVALID, "null argument");
  if (!c->query.cq_launched) return fail(ZRT_E_INVALID, "no camera query launched on this context yet");
  return zrt::radiance_info(c, out);
}
#endif  // ZRT_PLAN_ONLY
