// multi.cpp - several GPUs from one host thread (zrt_multi_*, zrt_render_multi):
// one context per rank, the tiles gathered to devices[0] through RCCL.
#include <dlfcn.h>
#include <rccl/rccl.h>

#include <algorithm>
#include <cstring>
#include <memory>
#include <mutex>

#include "context.hpp"

using zrt::fail;

namespace zrt {
namespace {
// RCCL for zrt_render_multi, opened on first use so that single-GPU callers do
// not load it: the copy already in the process when torch brought one (same
// soname, librccl.so.1), else ROCm's.
struct Rccl {
  decltype(&ncclCommInitAll) comm_init_all = nullptr;
  decltype(&ncclCommDestroy) comm_destroy = nullptr;
  decltype(&ncclGather) gather = nullptr;
  decltype(&ncclGroupStart) group_start = nullptr;
  decltype(&ncclGroupEnd) group_end = nullptr;
  decltype(&ncclGetErrorString) error_string = nullptr;
};
const Rccl& rccl() {
  static Rccl r;
  static std::once_flag once;
  std::call_once(once, [] {
    void* h = dlopen("librccl.so.1", RTLD_NOW | RTLD_LOCAL);
    if (!h) h = dlopen("/opt/rocm/lib/librccl.so.1", RTLD_NOW | RTLD_LOCAL);
    if (!h) return;
    r.comm_init_all = reinterpret_cast<decltype(r.comm_init_all)>(dlsym(h, "ncclCommInitAll"));
    r.comm_destroy = reinterpret_cast<decltype(r.comm_destroy)>(dlsym(h, "ncclCommDestroy"));
    r.gather = reinterpret_cast<decltype(r.gather)>(dlsym(h, "ncclGather"));
    r.group_start = reinterpret_cast<decltype(r.group_start)>(dlsym(h, "ncclGroupStart"));
    r.group_end = reinterpret_cast<decltype(r.group_end)>(dlsym(h, "ncclGroupEnd"));
    r.error_string = reinterpret_cast<decltype(r.error_string)>(dlsym(h, "ncclGetErrorString"));
  });
  if (!r.comm_init_all || !r.comm_destroy || !r.gather || !r.group_start || !r.group_end || !r.error_string)
    throw Error(ZRT_E_UNSUPPORTED, "RCCL (librccl.so.1 with ncclGather) is not available");
  return r;
}

#define NCCLCHK(R, expr)                                                                     \
  do {                                                                                       \
    const ncclResult_t r_ = (expr);                                                          \
    if (r_ != ncclSuccess) throw ::zrt::Error(ZRT_E_HIP, std::string("RCCL ") + #expr + ": " + (R).error_string(r_)); \
  } while (0)

// ncclCommInitAll communicators, one per device, destroyed with the call.
struct Comms {
  const Rccl* R = nullptr;
  std::vector<ncclComm_t> c;
  ~Comms() {
    for (ncclComm_t x : c)
      if (x) (void)R->comm_destroy(x);
  }
};

struct CtxDeleter {
  void operator()(zrt_ctx* c) const { zrt_ctx_destroy(c); }
};

}  // namespace
}  // namespace zrt

// One rank per entry of `devices`: its context (scene copy in that GPU's HBM),
// its padded tile buffer, and - one rank per distinct device - the RCCL
// communicators, all kept across frames.  Members are destroyed in reverse
// order: the communicators go before the contexts.
struct zrt_multi {
  std::vector<uint32_t> devices;
  uint32_t n_distinct = 0;
  bool use_rccl = false;
  std::vector<std::unique_ptr<zrt_ctx, zrt::CtxDeleter>> ctx;
  std::vector<zrt::DevBuf<float>> send;
  zrt::DevBuf<float> gathered, frame;  // on devices[0]
  size_t frame_n = 0;                  // floats of the last frame in `frame` (0: none rendered yet)
  std::vector<double> rank_ms;         // the last frame: each rank's render-kernel time (HIP events)
  zrt::Comms comms;
};

// ---- several GPUs from one host thread (zrt_multi_*, zrt_render_multi) -------
int zrt_multi_create(const zrt_scene* scene, const zrt_params* params, const uint32_t* devices,
                     uint32_t n_devices, zrt_multi** out) {
  if (!out || !devices) return fail(ZRT_E_INVALID, "null argument");
  *out = nullptr;
  if (n_devices == 0 || n_devices > 1024) return fail(ZRT_E_INVALID, "n_devices must be in 1..1024");
  if (!params) return fail(ZRT_E_INVALID, "params is null");
  int rc = zrt::validate_scene(scene);
  if (rc) return rc;
  for (uint32_t r = 0; r < n_devices; ++r) {
    rc = zrt::check_device(int(devices[r]));
    if (rc) return rc;
  }
  try {
    std::unique_ptr<zrt_multi> m(new zrt_multi);
    m->devices.assign(devices, devices + n_devices);
    std::vector<uint32_t> distinct(m->devices);
    std::sort(distinct.begin(), distinct.end());
    distinct.erase(std::unique(distinct.begin(), distinct.end()), distinct.end());
    m->n_distinct = uint32_t(distinct.size());
    // RCCL only where there is something to move between GPUs: one rank per
    // device, at least two devices (a device listed twice gathers by copies)
    m->use_rccl = m->n_distinct == n_devices && n_devices > 1;
    // the scene flattened once (BVH build, raytrace.zig:124-133), a copy on every GPU
    const bool use_bvh = params->bounded_volume_hierarchy != 0 && scene->n_prims > 10;
    zrt::HostScene host;
    zrt::flatten_for_device(&host, scene, use_bvh, int(devices[0]));
    for (uint32_t r = 0; r < n_devices; ++r) m->ctx.emplace_back(zrt::ctx_on_device(host, int(devices[r])).release());
    m->send.resize(n_devices);
    if (m->use_rccl) {
      // communicators live as long as the context (not per frame)
      const zrt::Rccl& R = zrt::rccl();
      m->comms.R = &R;
      m->comms.c.assign(n_devices, nullptr);
      std::vector<int> devs(devices, devices + n_devices);
      NCCLCHK(R, R.comm_init_all(m->comms.c.data(), int(n_devices), devs.data()));
    }
    *out = m.release();
    return ZRT_OK;
  }
  ZRT_CATCH_ALL
}

int zrt_multi_destroy(zrt_multi* m) {
  if (!m) return ZRT_OK;
  for (auto& c : m->ctx) {
    (void)hipSetDevice(c->device);
    (void)hipDeviceSynchronize();
  }
  delete m;
  return ZRT_OK;
}

int zrt_multi_render(zrt_multi* m, const zrt_camera* camera, const zrt_params* params, float* out_rgb,
                     zrt_stats* stats) {
  if (!m || !camera) return fail(ZRT_E_INVALID, "null argument");  // out_rgb NULL: the frame stays on devices[0]
  int rc = zrt::validate_params(params);
  if (rc) return rc;
  const uint32_t n = uint32_t(m->ctx.size());
  try {
    const zrt::Geometry g = zrt::geometry(params);
    std::vector<zrt_params> rp(n, *params);
    std::vector<uint32_t> count(n), base(n + 1, 0);
    uint32_t max_tiles = 0;
    for (uint32_t r = 0; r < n; ++r) {
      rp[r].rank = r;
      rp[r].world_size = n;
      rp[r].device = m->devices[r];
      count[r] = zrt::rank_tiles(g, r, n);
      base[r + 1] = base[r] + count[r];
      max_tiles = std::max(max_tiles, count[r]);
    }
    const size_t slot = 64 * 3;  // floats per tile
    // tile buffers padded to the largest rank's (ncclGather sends equal counts)
    for (uint32_t r = 0; r < n; ++r) {
      HIPCHK(hipSetDevice(m->ctx[r]->device));
      if (m->send[r].n < std::max<size_t>(1, max_tiles * slot)) m->send[r].alloc(std::max<size_t>(1, max_tiles * slot));
    }
    // the sampling loops, all enqueued before any is waited on
    for (uint32_t r = 0; r < n; ++r) {
      rc = zrt_ctx_render_tiles(m->ctx[r].get(), camera, &rp[r], m->send[r].p, nullptr);
      if (rc) return rc;
    }
    zrt_stats sum;
    std::memset(&sum, 0, sizeof(sum));
    int device_rc = ZRT_OK;
    std::string device_msg;
    m->frame_n = 0;
    m->rank_ms.assign(n, 0.0);
    for (uint32_t r = 0; r < n; ++r) {
      zrt_stats s;
      rc = zrt_ctx_stats(m->ctx[r].get(), &s);  // waits for rank r's launch
      if (rc == ZRT_E_UNSUPPORTED) {  // device error: finish the frame (NaN tiles), then report it
        device_rc = rc;
        device_msg = zrt_last_error();
      }
      else if (rc) return rc;
      // the render kernel alone (render_ms also holds the schedule probe)
      HIPCHK(hipSetDevice(m->ctx[r]->device));
      m->rank_ms[r] = zrt::launch_times(m->ctx[r]->ev).kernel_ms;
      if (r == 0) {
        sum = s;
        continue;
      }
      sum.recursion_depth_hits += s.recursion_depth_hits;
      sum.reflections += s.reflections;
      sum.background_hits += s.background_hits;
      sum.pixels_processed += s.pixels_processed;
      sum.samples_processed += s.samples_processed;
      sum.rays_processed += s.rays_processed;
      sum.node_visits += s.node_visits;
      sum.prim_tests += s.prim_tests;
      sum.sphere_tests += s.sphere_tests;
      sum.shade_fetches += s.shade_fetches;
      sum.texel_fetches += s.texel_fetches;
      sum.leaf_visits += s.leaf_visits;
      sum.order_replays += s.order_replays;
      sum.preprocess_ms = std::max(sum.preprocess_ms, s.preprocess_ms);
      sum.upload_ms = std::max(sum.upload_ms, s.upload_ms);
      sum.render_ms = std::max(sum.render_ms, s.render_ms);
      sum.schedule_ms = std::max(sum.schedule_ms, s.schedule_ms);
    }
    // the gather to devices[0] in the padded rank-major layout (rank r at
    // r * max_tiles tiles), which zrt_ctx_assemble_padded reads as it lies
    const double t0 = zrt::now_ms();
    zrt_ctx* root = m->ctx[0].get();
    HIPCHK(hipSetDevice(root->device));
    const size_t frame_n = size_t(params->width) * params->height * 3;
    if (m->frame.n < frame_n) m->frame.alloc(frame_n);
    const size_t gathered_n = std::max<size_t>(1, size_t(n) * max_tiles * slot);
    if (m->gathered.n < gathered_n) m->gathered.alloc(gathered_n);
    if (m->use_rccl) {
      const zrt::Rccl& R = *m->comms.R;
      NCCLCHK(R, R.group_start());
      for (uint32_t r = 0; r < n; ++r)
        NCCLCHK(R, R.gather(m->send[r].p, r == 0 ? m->gathered.p : nullptr, size_t(max_tiles) * slot, ncclFloat32, 0,
                            m->comms.c[r], m->ctx[r]->stream));
      NCCLCHK(R, R.group_end());
      // every rank's part of the gather is done before the next frame reuses its buffer
      for (uint32_t r = 1; r < n; ++r) {
        HIPCHK(hipSetDevice(m->ctx[r]->device));
        HIPCHK(hipStreamSynchronize(m->ctx[r]->stream));
      }
      HIPCHK(hipSetDevice(root->device));
    } else {
      // one device (or ranks sharing devices): copies; every rank's launch is done (stats above)
      for (uint32_t r = 0; r < n; ++r)
        if (count[r])
          HIPCHK(hipMemcpyPeerAsync(m->gathered.p + size_t(r) * max_tiles * slot, root->device, m->send[r].p,
                                    m->ctx[r]->device, size_t(count[r]) * slot * sizeof(float), root->stream));
    }
    rc = zrt_ctx_assemble_padded(root, &rp[0], m->gathered.p, std::max(1u, max_tiles), m->frame.p, nullptr);
    if (rc) return rc;
    HIPCHK(hipStreamSynchronize(root->stream));
    sum.gather_ms = zrt::now_ms() - t0;
    m->frame_n = frame_n;
    if (out_rgb) HIPCHK(hipMemcpy(out_rgb, m->frame.p, sizeof(float) * frame_n, hipMemcpyDeviceToHost));
    sum.n_gpus = m->n_distinct;
    if (stats) *stats = sum;
    if (device_rc) return fail(device_rc, device_msg);
    return ZRT_OK;
  }
  ZRT_CATCH_ALL
}

int zrt_multi_frame(zrt_multi* m, float* out_rgb, uint64_t n_floats) {
  if (!m || !out_rgb) return fail(ZRT_E_INVALID, "null argument");
  if (m->frame_n == 0) return fail(ZRT_E_INVALID, "no frame: zrt_multi_frame before a successful zrt_multi_render");
  if (n_floats != m->frame_n) return fail(ZRT_E_INVALID, "n_floats differs from the last frame's width * height * 3");
  try {
    HIPCHK(hipSetDevice(m->ctx[0]->device));
    HIPCHK(hipMemcpy(out_rgb, m->frame.p, sizeof(float) * m->frame_n, hipMemcpyDeviceToHost));
    return ZRT_OK;
  }
  ZRT_CATCH_ALL
}

int zrt_multi_rank_ms(zrt_multi* m, double* kernel_ms, uint32_t n) {
  if (!m || !kernel_ms) return fail(ZRT_E_INVALID, "null argument");
  if (m->rank_ms.empty()) return fail(ZRT_E_INVALID, "no frame rendered yet");
  if (n != m->rank_ms.size()) return fail(ZRT_E_INVALID, "n differs from the context's rank count");
  for (uint32_t r = 0; r < n; ++r) kernel_ms[r] = m->rank_ms[r];
  return ZRT_OK;
}

int zrt_multi_scanlines(zrt_multi* m, zrt_scanline* out, uint32_t height) {
  if (!m || !out) return fail(ZRT_E_INVALID, "null argument");
  try {
    std::memset(out, 0, sizeof(zrt_scanline) * height);
    for (auto& c : m->ctx) {
      const int rc = zrt::add_scanlines(c.get(), out, height);
      if (rc) return rc;
    }
    return ZRT_OK;
  }
  ZRT_CATCH_ALL
}

int zrt_render_multi(const zrt_scene* scene, const zrt_camera* camera, const zrt_params* params,
                     const uint32_t* devices, uint32_t n_devices, float* out_rgb, zrt_stats* stats) {
  if (!camera || !out_rgb || !devices) return fail(ZRT_E_INVALID, "null argument");
  int rc = zrt::validate_params(params);
  if (rc) return rc;
  zrt_multi* m = nullptr;
  rc = zrt_multi_create(scene, params, devices, n_devices, &m);
  if (rc) return rc;
  rc = zrt_multi_render(m, camera, params, out_rgb, stats);
  const std::string msg = zrt_last_error();
  zrt_multi_destroy(m);
  if (rc) return fail(rc, msg);
  return ZRT_OK;
}
