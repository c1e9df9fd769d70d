// queries.cpp - ray queries on a resident context (zrt.h "ray queries"): the closest
// hit (zrt_ctx_trace: trace_kernel, then the slot -> list index map on the device) and
// the exact any-hit (zrt_ctx_occluded: anyhit_kernel), with device pointers, on a
// stream, asynchronous; the one-shot zrt_occluded; and the time of the last query
// kernel.  A query has its own deep stack rows, error flag and completion (QueryState):
// it leaves a render run, a feature launch and their status alone.
#include <algorithm>
#include <cstdlib>

#include "context.hpp"

using zrt::fail;

namespace {
int check_query_args(const zrt_ctx* c, const zrt_params* p) {
  if (!c || !p) return fail(ZRT_E_INVALID, "null argument");
  if (p->traversal > ZRT_TRAVERSAL_BINARY) return fail(ZRT_E_INVALID, "unknown traversal");
  return zrt::params_fit_ctx(c, p);
}
bool misaligned(const void* p, uintptr_t a) { return (reinterpret_cast<uintptr_t>(p) & (a - 1)) != 0; }
}  // namespace

int zrt_ctx_trace(zrt_ctx* c, const zrt_params* p, const float* dev_rays, uint32_t n, float* dev_t, int32_t* dev_prim,
                  void* hip_stream) {
  int rc = check_query_args(c, p);
  if (rc) return rc;
  if (n == 0) return ZRT_OK;
  if (!dev_rays || !dev_t || !dev_prim) return fail(ZRT_E_INVALID, "null argument");
  if (misaligned(dev_rays, 4) || misaligned(dev_t, 4) || misaligned(dev_prim, 4))
    return fail(ZRT_E_INVALID, "trace: dev_rays, dev_t and dev_prim must be 4-byte aligned");
  try {
    HIPCHK(hipSetDevice(c->device));
    hipStream_t st = zrt::stream_of(c, hip_stream);
    const uint32_t* sp = zrt::slot_prim_table(c);
    zrt::launch_query(
        c, p, zrt::query_grid(n), st, false, "trace query",
        [&](zrt::KArgs& a, const zrt::TracePlan& t, uint32_t grid, hipStream_t s) {
          if (std::getenv("ZRT_DEBUG_NO_GUARD")) a.guard = 0.0f;  // as zrt_trace
          void* args[] = {&a, &dev_rays, &n, &dev_t, &dev_prim};
          HIPCHK(hipLaunchKernel(zrt::trace_kernel_ptr(t.kmode, t.stk16), dim3(grid), dim3(zrt::kBlock), args, t.lp.bytes,
                                 s));
        },
        [&](hipStream_t s, const unsigned long long* err) {
          HIPCHK(zrt::launch_trace_finish(s, dev_t, dev_prim, n, sp, err));
        });
    return ZRT_OK;
  }
  ZRT_CATCH_ALL
}

int zrt_ctx_occluded(zrt_ctx* c, const zrt_params* p, const float* dev_rays, const float* dev_t_max, uint32_t n,
                     uint8_t* dev_out, void* hip_stream) {
  int rc = check_query_args(c, p);
  if (rc) return rc;
  if (n == 0) return ZRT_OK;
  if (!dev_rays || !dev_out) return fail(ZRT_E_INVALID, "null argument");
  if (misaligned(dev_rays, 4) || misaligned(dev_t_max, 4))
    return fail(ZRT_E_INVALID, "occluded: dev_rays and dev_t_max must be 4-byte aligned");
  try {
    HIPCHK(hipSetDevice(c->device));
    hipStream_t st = zrt::stream_of(c, hip_stream);
    zrt::launch_query(
        c, p, zrt::query_grid(n), st, true, "any-hit query",
        [&](zrt::KArgs& a, const zrt::TracePlan& t, uint32_t grid, hipStream_t s) {
          void* args[] = {&a, &dev_rays, &dev_t_max, &n, &dev_out};
          HIPCHK(hipLaunchKernel(zrt::anyhit_kernel_ptr(t.kmode, t.stk16), dim3(grid), dim3(zrt::kBlock), args,
                                 t.lp.bytes, s));
        },
        [&](hipStream_t s, const unsigned long long* err) { HIPCHK(zrt::launch_anyhit_error(s, dev_out, n, err)); });
    return ZRT_OK;
  }
  ZRT_CATCH_ALL
}

int zrt_ctx_query_ms(zrt_ctx* c, double* ms) {
  if (!c || !ms) return fail(ZRT_E_INVALID, "null argument");
  if (!c->query.timer.launched) return fail(ZRT_E_INVALID, "no query launched on this context yet");
  try {
    HIPCHK(hipSetDevice(c->device));
    HIPCHK(hipEventSynchronize(c->query.timer.e1));
    float f = 0.0f;
    HIPCHK(hipEventElapsedTime(&f, c->query.timer.e0, c->query.timer.e1));
    *ms = f;
    return ZRT_OK;
  }
  ZRT_CATCH_ALL
}

int zrt_occluded(const zrt_scene* scene, const zrt_params* params, const float* rays, const float* t_max, uint32_t n,
                 uint8_t* out) {
  if (!params || (n && (!rays || !out))) return fail(ZRT_E_INVALID, "null argument");
  int rc = zrt::validate_scene(scene);
  if (rc) return rc;
  if (params->traversal > ZRT_TRAVERSAL_BINARY) return fail(ZRT_E_INVALID, "unknown traversal");
  rc = zrt::check_device(int(params->device));
  if (rc) return rc;
  if (n == 0) return ZRT_OK;
  try {
    const bool use_bvh = params->bounded_volume_hierarchy != 0 && scene->n_prims > 10;
    zrt::HostScene h;
    zrt::flatten_for_device(&h, scene, use_bvh, int(params->device));
    std::unique_ptr<zrt_ctx> c = zrt::ctx_on_device(h, int(params->device));
    zrt::DevBuf<float> d_rays, d_tmax;
    zrt::DevBuf<uint8_t> d_out;
    d_rays.alloc(6ull * n);
    d_out.alloc(n);
    HIPCHK(hipMemcpy(d_rays.p, rays, sizeof(float) * 6ull * n, hipMemcpyHostToDevice));
    if (t_max) {
      d_tmax.alloc(n);
      HIPCHK(hipMemcpy(d_tmax.p, t_max, sizeof(float) * n, hipMemcpyHostToDevice));
    }
    rc = zrt_ctx_occluded(c.get(), params, d_rays.p, t_max ? d_tmax.p : nullptr, n, d_out.p, nullptr);
    if (rc) return rc;
    rc = zrt_ctx_sync(c.get());
    if (rc) return rc;
    HIPCHK(hipMemcpy(out, d_out.p, n, hipMemcpyDeviceToHost));
    return ZRT_OK;
  }
  ZRT_CATCH_ALL
}
