// debug_device.cpp - the entry points that run a kernel for a test or a tool:
// zrt_trace, the device arithmetic probes (zrt_debug_math / division / rng) and
// the context's raw counters, wave times and schedule (zrt_ctx_debug_*).
#include <algorithm>
#include <cstdlib>

#include "context.hpp"

using zrt::fail;

int zrt_ctx_debug_counters(zrt_ctx* c, uint64_t* out, uint32_t n) {
  if (!c || !out) return fail(ZRT_E_INVALID, "null argument");
  if (!c->render.launched) return fail(ZRT_E_INVALID, "no kernel launched on this context yet");
  try {
    HIPCHK(hipSetDevice(c->device));
    HIPCHK(hipEventSynchronize(c->render.done));
    unsigned long long h[zrt::kScratchSlots] = {0};
    HIPCHK(hipMemcpy(h, c->scratch.p, sizeof(h), hipMemcpyDeviceToHost));
    h[zrt::kSkyTilesSlot] = c->last.sky_tiles;
    h[zrt::kSphereTilesSlot] = c->last.sphere_tiles;
    for (uint32_t i = 0; i < n && i < uint32_t(zrt::kScratchSlots); ++i) out[i] = h[i];
    return ZRT_OK;
  }
  ZRT_CATCH_ALL
}

int zrt_ctx_debug_wave_times(zrt_ctx* c, uint64_t* out, uint32_t cap, uint32_t* n_waves) {
  if (!c || !n_waves) return fail(ZRT_E_INVALID, "null argument");
  try {
    HIPCHK(hipSetDevice(c->device));
    if (c->render.launched) HIPCHK(hipEventSynchronize(c->render.done));
    *n_waves = c->last.n_waves;
    const size_t n = std::min<size_t>(cap / 2, *n_waves);
    if (n && out) HIPCHK(hipMemcpy(out, c->wave_times.p, 2 * n * sizeof(uint64_t), hipMemcpyDeviceToHost));
    return ZRT_OK;
  }
  ZRT_CATCH_ALL
}

int zrt_ctx_debug_schedule(zrt_ctx* c, uint32_t* costs, uint32_t* order, uint32_t cap, uint32_t* n_tiles) {
  if (!c || !n_tiles) return fail(ZRT_E_INVALID, "null argument");
  if (!c->render.launched) return fail(ZRT_E_INVALID, "no kernel launched on this context yet");
  try {
    HIPCHK(hipSetDevice(c->device));
    HIPCHK(hipEventSynchronize(c->render.done));
    *n_tiles = c->last.scheduled ? c->probe.tile_ids_n : 0u;
    const size_t n = std::min<size_t>(cap, *n_tiles);
    if (n && costs) HIPCHK(hipMemcpy(costs, c->probe.tile_cost.p, n * sizeof(uint32_t), hipMemcpyDeviceToHost));
    if (n && order) HIPCHK(hipMemcpy(order, c->probe.tile_order.p, n * sizeof(uint32_t), hipMemcpyDeviceToHost));
    return ZRT_OK;
  }
  ZRT_CATCH_ALL
}

int zrt_trace(const zrt_scene* scene, const zrt_params* params, const float* rays, uint32_t n_rays, float* out_t,
              int32_t* out_prim) {
  if (!params || (n_rays && (!rays || !out_t || !out_prim))) return fail(ZRT_E_INVALID, "null argument");
  int rc = zrt::validate_scene(scene);
  if (rc) return rc;
  if (params->traversal > ZRT_TRAVERSAL_BINARY) return fail(ZRT_E_INVALID, "unknown traversal");
  rc = zrt::check_device(int(params->device));
  if (rc) return rc;
  if (n_rays == 0) return ZRT_OK;
  try {
    const bool use_bvh = params->bounded_volume_hierarchy != 0 && scene->n_prims > 10;
    zrt::HostScene h;
    zrt::flatten_for_device(&h, scene, use_bvh, int(params->device));
    std::unique_ptr<zrt_ctx> c = zrt::ctx_on_device(h, int(params->device));
    const uint32_t grid = (n_rays + zrt::kBlock - 1) / zrt::kBlock;
    const uint64_t n_lanes = uint64_t(grid) * zrt::kBlock;
    zrt::DevBuf<float> d_rays, d_t;
    zrt::DevBuf<int32_t> d_slot;
    d_rays.alloc(6ull * n_rays);
    d_t.alloc(n_rays);
    d_slot.alloc(n_rays);
    HIPCHK(hipMemcpy(d_rays.p, rays, sizeof(float) * 6ull * n_rays, hipMemcpyHostToDevice));
    HIPCHK(hipMemset(c->scratch.p, 0, zrt::kScratchSlots * sizeof(unsigned long long)));
    zrt::KArgs a{};
    const zrt::TracePlan t = zrt::fill_trace(a, c.get(), params->traversal);
    // tests: ZRT_DEBUG_NO_GUARD=1 traces without the grazing-triangle guard (the
    // default render kernels' traversal), to record what the guard is for
    if (std::getenv("ZRT_DEBUG_NO_GUARD")) a.guard = 0.0f;
    zrt::trace_rows(a, c.get(), t, n_lanes, c->stack_ovf, c->stream, "trace launch");
    void* fn = zrt::trace_kernel_ptr(t.kmode, t.stk16);
    const float* rp = d_rays.p;
    float* tp = d_t.p;
    int32_t* sp = d_slot.p;
    uint32_t nn = n_rays;
    void* args[] = {&a, &rp, &nn, &tp, &sp};
    HIPCHK(hipLaunchKernel(fn, dim3(grid), dim3(zrt::kBlock), args, t.lp.bytes, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    unsigned long long err = 0;
    HIPCHK(hipMemcpy(&err, c->scratch.p + zrt::kErrorSlot, sizeof(err), hipMemcpyDeviceToHost));
    if (err) return fail(ZRT_E_UNSUPPORTED, zrt::device_error_msg(err));
    std::vector<int32_t> slot(n_rays);
    HIPCHK(hipMemcpy(out_t, d_t.p, sizeof(float) * n_rays, hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(slot.data(), d_slot.p, sizeof(int32_t) * n_rays, hipMemcpyDeviceToHost));
    for (uint32_t i = 0; i < n_rays; ++i)
      out_prim[i] = slot[i] < 0 ? -1 : int32_t(c->scene.slot_to_prim[size_t(slot[i])]);
    return ZRT_OK;
  }
  ZRT_CATCH_ALL
}

int zrt_debug_math(int fn, const float* x, const float* y, float* out, uint32_t n, uint32_t device) {
  if (!x || !out) return fail(ZRT_E_INVALID, "null argument");
  int rc = zrt::check_device(int(device));
  if (rc) return rc;
  try {
    HIPCHK(hipSetDevice(int(device)));
    zrt::DevBuf<float> dx, dy, dout;
    dx.alloc(n);
    dout.alloc(n);
    HIPCHK(hipMemcpy(dx.p, x, n * sizeof(float), hipMemcpyHostToDevice));
    if (y) {
      dy.alloc(n);
      HIPCHK(hipMemcpy(dy.p, y, n * sizeof(float), hipMemcpyHostToDevice));
    }
    HIPCHK(zrt::launch_debug_math(fn, dx.p, y ? dy.p : nullptr, dout.p, n));
    HIPCHK(hipDeviceSynchronize());
    HIPCHK(hipMemcpy(out, dout.p, n * sizeof(float), hipMemcpyDeviceToHost));
    return ZRT_OK;
  }
  ZRT_CATCH_ALL
}

int zrt_debug_division(uint64_t n, uint64_t* counts, uint32_t device) {
  if (!counts) return fail(ZRT_E_INVALID, "null argument");
  int rc = zrt::check_device(int(device));
  if (rc) return rc;
  try {
    HIPCHK(hipSetDevice(int(device)));
    zrt::DevBuf<unsigned long long> d;
    d.alloc(5);
    HIPCHK(hipMemset(d.p, 0, 5 * sizeof(unsigned long long)));
    HIPCHK(zrt::launch_debug_division(n, d.p));
    HIPCHK(hipDeviceSynchronize());
    HIPCHK(hipMemcpy(counts, d.p, 5 * sizeof(uint64_t), hipMemcpyDeviceToHost));
    return ZRT_OK;
  }
  ZRT_CATCH_ALL
}

int zrt_debug_compact(const uint32_t* list, uint32_t n, const uint32_t* tile_done, uint32_t n_tiles, uint32_t* out,
                      uint32_t* count, uint32_t device) {
  if (!list || !tile_done || !out || !count) return fail(ZRT_E_INVALID, "null argument");
  if (n == 0) return fail(ZRT_E_INVALID, "compact: an empty list");
  // (the kernel reads tile_done[list[i]]: no entry may point past it)
  for (uint32_t i = 0; i < n; ++i)
    if (list[i] >= n_tiles) return fail(ZRT_E_INVALID, "compact: a list entry is not below n_tiles");
  int rc = zrt::check_device(int(device));
  if (rc) return rc;
  try {
    HIPCHK(hipSetDevice(int(device)));
    zrt::DevBuf<uint32_t> d_list, d_done, d_out, d_count;
    d_list.alloc(n);
    d_done.alloc(n_tiles);
    d_out.alloc(n);
    d_count.alloc(1);
    HIPCHK(hipMemcpy(d_list.p, list, size_t(n) * sizeof(uint32_t), hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(d_done.p, tile_done, size_t(n_tiles) * sizeof(uint32_t), hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(d_out.p, out, size_t(n) * sizeof(uint32_t), hipMemcpyHostToDevice));
    HIPCHK(hipMemset(d_count.p, 0, sizeof(uint32_t)));
    HIPCHK(zrt::launch_compact(nullptr, d_list.p, n, d_done.p, d_out.p, d_count.p));
    HIPCHK(hipDeviceSynchronize());
    HIPCHK(hipMemcpy(out, d_out.p, size_t(n) * sizeof(uint32_t), hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(count, d_count.p, sizeof(uint32_t), hipMemcpyDeviceToHost));
    return ZRT_OK;
  }
  ZRT_CATCH_ALL
}

int zrt_debug_rng(uint32_t prng, uint64_t key, uint64_t* out, uint32_t n, uint32_t device) {
  if (!out) return fail(ZRT_E_INVALID, "null argument");
  int rc = zrt::check_device(int(device));
  if (rc) return rc;
  try {
    HIPCHK(hipSetDevice(int(device)));
    zrt::DevBuf<unsigned long long> d;
    d.alloc(n);
    HIPCHK(zrt::launch_debug_rng(prng, key, d.p, n));
    HIPCHK(hipDeviceSynchronize());
    HIPCHK(hipMemcpy(out, d.p, n * sizeof(uint64_t), hipMemcpyDeviceToHost));
    return ZRT_OK;
  }
  ZRT_CATCH_ALL
}
