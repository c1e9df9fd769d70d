// post.cpp - what a context does with a rendered frame: the first-hit feature
// buffers (zrt_ctx_features), the two denoisers and the temporal step, with their
// default values; for lens frames the variance plane of a camera query's sums and both
// denoisers on a rectangle.  The kernels: render.hip, denoise.hip, temporal.hip.
#include <cstring>

#include "context.hpp"

using zrt::fail;

// ---- first-hit feature buffers (zrt.h "denoising") ---------------------------
int zrt_ctx_features(zrt_ctx* c, const zrt_camera* cam, const zrt_params* p, float* dev_features, void* hip_stream) {
  if (!c || !cam || !dev_features) return fail(ZRT_E_INVALID, "null argument");
  int rc = zrt::validate_params(p);
  if (rc) return rc;
  rc = zrt::params_fit_ctx(c, p);
  if (rc) return rc;
  if (reinterpret_cast<uintptr_t>(dev_features) & 15u)
    return fail(ZRT_E_INVALID, "dev_features must be 16-byte aligned");
  try {
    zrt::FeatureState& f = c->feat;
    HIPCHK(hipSetDevice(c->device));
    hipStream_t st = zrt::stream_of(c, hip_stream);
    const uint32_t tiles = ((p->width + 7u) / 8u) * ((p->height + 7u) / 8u);
    const uint32_t grid = (tiles + zrt::kBlock / 64 - 1) / (zrt::kBlock / 64);
    const uint64_t n_lanes = uint64_t(grid) * zrt::kBlock;
    const uint32_t* sp = zrt::slot_prim_table(c);
    f.done.create();
    // the context's error flag: what a render launch left there stays (a run's flag is
    // sticky); before the first launch the slots hold nothing yet
    if (!c->render.launched && !f.done.launched)
      HIPCHK(hipMemsetAsync(c->scratch.p, 0, zrt::kScratchSlots * sizeof(unsigned long long), st));
    zrt::KArgs a{};
    const zrt::TracePlan t = zrt::fill_trace(a, c, p->traversal);
    zrt::fill_camera(a, cam, p);
    zrt::trace_rows(a, c, t, n_lanes, f.ovf, st, "feature launch");
    void* fn = zrt::features_kernel_ptr(t.kmode, t.stk16);
    float4* out = reinterpret_cast<float4*>(dev_features);
    void* args[] = {&a, &sp, &out};
    HIPCHK(hipLaunchKernel(fn, dim3(grid), dim3(zrt::kBlock), args, t.lp.bytes, st));
    const uint64_t n_f4 = 2ull * p->width * p->height;
    HIPCHK(zrt::launch_features_error(st, out, n_f4, c->scratch.p + zrt::kErrorSlot));
    HIPCHK(hipMemcpyAsync(f.done.err.get(), c->scratch.p + zrt::kErrorSlot, sizeof(unsigned long long),
                          hipMemcpyDeviceToHost, st));
    HIPCHK(hipEventRecord(f.done.done, st));
    f.done.launched = true;
    f.done.reported = false;
    return ZRT_OK;
  }
  ZRT_CATCH_ALL
}

namespace {
// What the denoise and temporal calls refuse of their pointers, in this order, after
// their plan and flag refusals; `who` ("denoise" / "temporal") leads the message.
// guided: the calls that read and may write a variance plane.
int check_post_args(const char* who, const zrt_ctx* c, const zrt_params* p, const float* frame, const float* features,
                    const float* out, bool guided, const float* variance = nullptr,
                    const float* out_variance = nullptr, bool have_cam = true) {
  const std::string w = std::string(who) + ": ";
  if (out && out == frame) return fail(ZRT_E_INVALID, w + "dev_out must not be dev_frame");
  if (reinterpret_cast<uintptr_t>(features) & 15u) return fail(ZRT_E_INVALID, w + "dev_features must be 16-byte aligned");
  if (guided && !variance) return fail(ZRT_E_INVALID, w + "dev_variance is null");
  if (guided && out_variance && out_variance == variance)
    return fail(ZRT_E_INVALID, w + "dev_out_variance must not be dev_variance");
  if (!c || !have_cam || !frame || !features || !out) return fail(ZRT_E_INVALID, "null argument");
  if (int(p->device) != c->device)
    return fail(ZRT_E_INVALID, "params->device differs from the device the context was created on");
  return ZRT_OK;
}

// A step's enqueue between its two events (made on first use), for its *_ms call.
template <class Enqueue>
void timed_step(zrt::StepTimer& t, hipStream_t st, Enqueue&& enqueue) {
  t.e0.create();
  t.e1.create();
  HIPCHK(hipEventRecord(t.e0, st));
  enqueue();
  HIPCHK(hipEventRecord(t.e1, st));
  t.launched = true;
}
int step_ms(zrt_ctx* c, const zrt::StepTimer* t, const char* none_yet, double* ms) {
  if (!c || !ms) return fail(ZRT_E_INVALID, "null argument");
  if (!t->launched) return fail(ZRT_E_INVALID, none_yet);
  try {
    HIPCHK(hipSetDevice(c->device));
    HIPCHK(hipEventSynchronize(t->e1));
    float f = 0.0f;
    HIPCHK(hipEventElapsedTime(&f, t->e0, t->e1));
    *ms = f;
    return ZRT_OK;
  }
  ZRT_CATCH_ALL
}

// Both filters: the ping-pong planes grown to the frame, the enqueue timed.
template <class Enqueue>
int denoise_step(zrt_ctx* c, const zrt::DenoiseLaunch& l, void* hip_stream, Enqueue&& enqueue) {
  try {
    HIPCHK(hipSetDevice(c->device));
    hipStream_t st = zrt::stream_of(c, hip_stream);
    for (zrt::DevBuf<float4>& b : c->dn.buf) b.grow(size_t(l.n) * l.n);
    timed_step(c->dn.timer, st, [&] { enqueue(c->dn.buf[0].p, c->dn.buf[1].p, st); });
    return ZRT_OK;
  }
  ZRT_CATCH_ALL
}
}  // namespace

// ---- denoising (zrt.h "denoising"; the kernels: denoise.hip) ----------------
// the default sigmas: the winner of tools/denoise_probe.py's grid of powers of two
// (profiles/r10/denoise/defaults.json)
#define ZRT_DN_SIGMA_COLOR 2.0f
#define ZRT_DN_SIGMA_NORMAL 0.125f
#define ZRT_DN_SIGMA_ALBEDO 0x1p-12f
#define ZRT_DN_SIGMA_DEPTH 0.015625f
int zrt_denoise_defaults(zrt_denoise* out) {
  if (!out) return fail(ZRT_E_INVALID, "null argument");
  *out = zrt_denoise{ZRT_DEFAULT_DENOISE_ITERATIONS, ZRT_DN_SIGMA_COLOR, ZRT_DN_SIGMA_NORMAL, ZRT_DN_SIGMA_ALBEDO,
                     ZRT_DN_SIGMA_DEPTH, {0, 0, 0}};
  return ZRT_OK;
}

int zrt_ctx_denoise(zrt_ctx* c, const zrt_params* p, const zrt_denoise* dn, const float* dev_frame,
                    const float* dev_features, float* dev_out, void* hip_stream) {
  zrt::DenoiseLaunch l{};
  int rc = zrt::plan_denoise(p, dn, &l);  // (the refusals that need no context come first)
  if (rc) return rc;
  rc = check_post_args("denoise", c, p, dev_frame, dev_features, dev_out, false);
  if (rc) return rc;
  return denoise_step(c, l, hip_stream, [&](float4* b0, float4* b1, hipStream_t st) {
    HIPCHK(zrt::denoise_enqueue(l, dev_frame, reinterpret_cast<const float4*>(dev_features), dev_out, b0, b1, st));
  });
}

// the default guided filter: the winner of tools/denoise_guided_probe.py's search
// (profiles/r11/guided/defaults.json)
#define ZRT_DG_SIGMA_COLOR 4.0f
#define ZRT_DG_SIGMA_NORMAL 0.0625f
#define ZRT_DG_SIGMA_ALBEDO 0x1p-12f
#define ZRT_DG_SIGMA_DEPTH 0.015625f
#define ZRT_DG_FLAGS ZRT_DN_DEMODULATE
int zrt_denoise_guided_defaults(zrt_denoise* out, uint32_t* flags) {
  if (!out || !flags) return fail(ZRT_E_INVALID, "null argument");
  *out = zrt_denoise{ZRT_DEFAULT_DENOISE_ITERATIONS, ZRT_DG_SIGMA_COLOR, ZRT_DG_SIGMA_NORMAL, ZRT_DG_SIGMA_ALBEDO,
                     ZRT_DG_SIGMA_DEPTH, {0, 0, 0}};
  *flags = ZRT_DG_FLAGS;
  return ZRT_OK;
}

int zrt_ctx_denoise_guided(zrt_ctx* c, const zrt_params* p, const zrt_denoise* dn, uint32_t flags,
                           const float* dev_frame, const float* dev_features, const float* dev_variance,
                           float* dev_out, float* dev_out_variance, void* hip_stream) {
  zrt::DenoiseLaunch l{};
  int rc = zrt::plan_denoise(p, dn, &l);  // (the refusals that need no context come first)
  if (rc) return rc;
  if (flags & ~uint32_t(ZRT_DN_DEMODULATE)) return fail(ZRT_E_INVALID, "denoise: unknown flag");
  rc = check_post_args("denoise", c, p, dev_frame, dev_features, dev_out, true, dev_variance, dev_out_variance);
  if (rc) return rc;
  return denoise_step(c, l, hip_stream, [&](float4* b0, float4* b1, hipStream_t st) {
    HIPCHK(zrt::denoise_guided_enqueue(l, dn->sigma_color, (flags & ZRT_DN_DEMODULATE) != 0, dev_frame,
                                       reinterpret_cast<const float4*>(dev_features), dev_variance, dev_out,
                                       dev_out_variance, b0, b1, st));
  });
}

// ---- lens frames (zrt.h "denoising lens frames"): the variance plane of a camera query's
// sums, and both filters with a rectangle as their domain ----
int zrt_ctx_camera_variance(zrt_ctx* c, const zrt_params* p, const zrt_rect* rect, uint32_t n_total,
                            const float* dev_sum, float* dev_variance, void* hip_stream) {
  zrt_variance_plan vp{};
  int rc = zrt::plan_camera_variance(p, rect, n_total, &vp);  // (the refusals that need no context come first)
  if (rc) return rc;
  if (!c || !dev_sum || !dev_variance) return fail(ZRT_E_INVALID, "null argument");
  if (reinterpret_cast<uintptr_t>(dev_sum) & 15u)
    return fail(ZRT_E_INVALID, "camera variance: dev_sum must be 16-byte aligned");
  if (reinterpret_cast<uintptr_t>(dev_variance) & 3u)
    return fail(ZRT_E_INVALID, "camera variance: dev_variance must be 4-byte aligned");
  if (int(p->device) != c->device)
    return fail(ZRT_E_INVALID, "params->device differs from the device the context was created on");
  try {
    HIPCHK(hipSetDevice(c->device));
    hipStream_t st = zrt::stream_of(c, hip_stream);
    const zrt::DenoiseRect r{rect->x0, rect->y0, rect->w, rect->h};
    HIPCHK(zrt::camera_variance_enqueue(r, p->width, vp.ik, vp.sc, reinterpret_cast<const float4*>(dev_sum),
                                        dev_variance, st));
    return ZRT_OK;
  }
  ZRT_CATCH_ALL
}

int zrt_ctx_denoise_rect(zrt_ctx* c, const zrt_params* p, const zrt_denoise* dn, uint32_t flags, const zrt_rect* rect,
                         const float* dev_frame, const float* dev_features, const float* dev_variance, float* dev_out,
                         float* dev_out_variance, void* hip_stream) {
  zrt::DenoiseLaunch l{};
  int rc = zrt::plan_denoise_rect(p, dn, rect, &l);  // (the refusals that need no context come first)
  if (rc) return rc;
  const bool guided = dev_variance != nullptr;
  if (flags & ~uint32_t(ZRT_DN_DEMODULATE)) return fail(ZRT_E_INVALID, "denoise: unknown flag");
  if (!guided && flags) return fail(ZRT_E_INVALID, "denoise: flags need a variance plane (dev_variance is null)");
  if (!guided && dev_out_variance)
    return fail(ZRT_E_INVALID, "denoise: dev_out_variance needs a variance plane (dev_variance is null)");
  rc = check_post_args("denoise", c, p, dev_frame, dev_features, dev_out, guided, dev_variance, dev_out_variance);
  if (rc) return rc;
  try {
    HIPCHK(hipSetDevice(c->device));
    hipStream_t st = zrt::stream_of(c, hip_stream);
    const zrt::DenoiseRect r{rect->x0, rect->y0, rect->w, rect->h};
    for (zrt::DevBuf<float4>& b : c->dn.buf) b.grow(size_t(r.w) * r.h);
    timed_step(c->dn.timer, st, [&] {
      HIPCHK(zrt::denoise_rect_enqueue(l, r, p->height, dn->sigma_color, (flags & ZRT_DN_DEMODULATE) != 0, dev_frame,
                                       reinterpret_cast<const float4*>(dev_features), dev_variance, dev_out,
                                       dev_out_variance, c->dn.buf[0].p, c->dn.buf[1].p, st));
    });
    return ZRT_OK;
  }
  ZRT_CATCH_ALL
}

int zrt_ctx_denoise_ms(zrt_ctx* c, double* ms) {
  return step_ms(c, c ? &c->dn.timer : nullptr, "no denoise launched on this context yet", ms);
}

// ---- temporal accumulation (zrt.h "temporal accumulation"; the kernel: temporal.hip) ----
// the default step: the winner of tools/temporal_probe.py's grid
// (profiles/r12/temporal/defaults.json)
#define ZRT_TA_ALPHA_MIN 0.0f
#define ZRT_TA_MAX_HISTORY 2u
#define ZRT_TA_SIGMA_NORMAL 0.0f
#define ZRT_TA_SIGMA_DEPTH 0.0f
#define ZRT_TA_FLAGS 0u
int zrt_temporal_defaults(zrt_temporal* out) {
  if (!out) return fail(ZRT_E_INVALID, "null argument");
  *out = zrt_temporal{ZRT_TA_ALPHA_MIN, ZRT_TA_MAX_HISTORY, ZRT_TA_SIGMA_NORMAL, ZRT_TA_SIGMA_DEPTH, ZRT_TA_FLAGS,
                      {0, 0, 0}};
  return ZRT_OK;
}

int zrt_ctx_temporal(zrt_ctx* c, const zrt_camera* cam, const zrt_params* p, const zrt_temporal* tp,
                     const float* dev_frame, const float* dev_features, const float* dev_variance, float* dev_out,
                     float* dev_out_variance, uint32_t* dev_out_len, void* hip_stream) {
  zrt::TemporalLaunch l{};
  int rc = zrt::plan_temporal(p, tp, &l);  // (the refusals that need no context come first)
  if (rc) return rc;
  rc = check_post_args("temporal", c, p, dev_frame, dev_features, dev_out, true, dev_variance, dev_out_variance,
                       cam != nullptr);
  if (rc) return rc;
  try {
    zrt::TemporalState& ta = c->ta;
    HIPCHK(hipSetDevice(c->device));
    hipStream_t st = zrt::stream_of(c, hip_stream);
    const size_t plane = size_t(l.n) * l.n;
    if (ta.width != p->width || ta.height != p->height || ta.hist[0].n < plane) {
      for (int k = 0; k < 2; ++k) {  // (hipFree waits for the frames in flight)
        ta.hist[k].alloc(plane);
        ta.feat[k].alloc(2 * plane);
        ta.len[k].alloc(plane);
      }
      ta.width = p->width;
      ta.height = p->height;
      ta.live = false;
    }
    if (ta.demod != l.demod) ta.live = false;
    if (ta.live) {
      zrt_reproject_plan rp{};
      rc = zrt::plan_reproject(&ta.cam, p, &rp);
      if (rc) return rc;
      l.history = rp.valid;
      l.static_cam = std::memcmp(cam, &ta.cam, sizeof(zrt_camera)) == 0 ? 1u : 0u;
      zrt::copy3(l.porg, rp.origin);
      zrt::copy3(l.rn, rp.rn);
      zrt::copy3(l.ru, rp.ru);
      zrt::copy3(l.rv, rp.rv);
    }
    zrt::copy3(l.org, cam->origin);
    zrt::copy3(l.llc, cam->lower_left_corner);
    zrt::copy3(l.hor, cam->horizontal);
    zrt::copy3(l.ver, cam->vertical);
    const uint32_t cur = ta.cur, nxt = cur ^ 1u;
    const zrt::TemporalPlanes prev{ta.hist[cur].p, ta.feat[cur].p, ta.len[cur].p};
    const zrt::TemporalPlanes next{ta.hist[nxt].p, ta.feat[nxt].p, ta.len[nxt].p};
    timed_step(ta.timer, st, [&] {
      HIPCHK(zrt::temporal_enqueue(l, dev_frame, reinterpret_cast<const float4*>(dev_features), dev_variance, prev,
                                   next, dev_out, dev_out_variance, dev_out_len, st));
    });
    ta.cur = nxt;
    ta.cam = *cam;
    ta.demod = l.demod;
    ta.live = true;
    return ZRT_OK;
  }
  ZRT_CATCH_ALL
}

int zrt_ctx_temporal_reset(zrt_ctx* c) {
  if (!c) return fail(ZRT_E_INVALID, "null argument");
  c->ta.live = false;
  return ZRT_OK;
}

int zrt_ctx_temporal_ms(zrt_ctx* c, double* ms) {
  return step_ms(c, c ? &c->ta.timer : nullptr, "no temporal step launched on this context yet", ms);
}
