// context.hpp - private to the host files that talk to the HIP runtime
// (context.cpp, multi.cpp, oneshot.cpp): the HIP error type, device buffers, the
// context behind zrt_ctx_* and the catch clauses of their entry points.
#pragma once
#include <hip/hip_runtime_api.h>

#include <memory>
#include <string>
#include <vector>

#include "host.hpp"

namespace zrt {
struct HipError {
  hipError_t err;
  std::string where;
};

#define HIPCHK(expr)                                                       \
  do {                                                                     \
    const hipError_t e_ = (expr);                                          \
    if (e_ != hipSuccess) throw ::zrt::HipError{e_, std::string(#expr)};          \
  } while (0)

template <class T>
struct DevBuf {
  T* p = nullptr;
  size_t n = 0;
  DevBuf() = default;
  DevBuf(const DevBuf&) = delete;
  DevBuf& operator=(const DevBuf&) = delete;
  DevBuf(DevBuf&& o) noexcept : p(o.p), n(o.n) {
    o.p = nullptr;
    o.n = 0;
  }
  ~DevBuf() { release(); }
  void release() {
    if (p) (void)hipFree(p);
    p = nullptr;
    n = 0;
  }
  void alloc(size_t count) {
    release();
    if (count == 0) count = 1;
    HIPCHK(hipMalloc(&p, count * sizeof(T)));
    n = count;
  }
  void upload(const std::vector<T>& v) {
    alloc(v.size());
    if (!v.empty()) HIPCHK(hipMemcpy(p, v.data(), v.size() * sizeof(T), hipMemcpyHostToDevice));
  }
};
}  // namespace zrt

struct zrt_ctx {
  int device = 0;
  hipStream_t stream = nullptr;
  bool use_bvh = false;
  uint32_t n_prims = 0, n_nodes = 0, bvh_depth = 0, stack_depth = 0;
  uint32_t n_wide = 0, n_leaves = 0, wide_stack = 0, wide_stride = 0, n_top = 0, n_mats = 0;
  std::vector<uint32_t> slot_to_prim;  // device primitive slot -> reference list index
  zrt::SceneShape shape;               // what the launch decision reads of the scene (plan_launch)
  zrt::DevBuf<float4> wnodes;
  zrt::DevBuf<float4> qnodes, qleaves;  // compressed wide nodes + leaf records (q_ok)
  bool q_ok = false;
  uint32_t q_stride = 0, q_top = 0, n_qleaves = 0;
  zrt::DevBuf<float4> nodes, prims, shade;
  zrt::DevBuf<zrt::DevMaterial> mats;
  zrt::DevBuf<float> texels;
  zrt::DevBuf<uint32_t> texels8;
  zrt::DevBuf<uint32_t> leaf_of_slot;
  zrt::DevBuf<uint8_t> ref_sph;
  float root_c[3] = {0.0f, 0.0f, 0.0f}, origin_bound = 0.0f;
  uint32_t layout = 0;  // the wide tree's encoding (KArgs::layout)
  float graze_m = 0x1p-18f, graze_leaf = 0x1p-18f;  // KArgs::graze_m / graze_leaf
  float guard = 0.0f;                                // KArgs::guard
  uint32_t texel_bytes = 0;
  uint32_t tri_rcp_fast = 1;
  float scene_extent = 1.0f;
  float tri_c[3] = {0.0f, 0.0f, 0.0f}, tri_h[3] = {0.0f, 0.0f, 0.0f};  // KArgs::tri_c / tri_h
  zrt::DevBuf<uint32_t> att;  // attenuation rows past the LDS ones (att codes)
  zrt::DevBuf<uint8_t> stack_ovf;  // FAST stack rows beyond the LDS part (deep trees)
  zrt::DevBuf<unsigned long long> scratch;  // counters, work counter, error flag (kScratchSlots)
  zrt::DevBuf<float4> partial;
  zrt::DevBuf<uint32_t> rank_base;
  // scheduling probe: its own partial sums + counters, per-tile costs, the sort
  zrt::DevBuf<float4> probe_partial;
  zrt::DevBuf<unsigned long long> probe_scratch;
  zrt::DevBuf<uint32_t> tile_cost, tile_ids, cost_sorted, tile_order;
  zrt::DevBuf<uint8_t> sort_temp;
  uint32_t tile_ids_n = 0;
  // what the probe behind tile_order / probe_scratch saw: a launch with the same key
  // takes them as they are (launch_frame).  The order is a cost estimate only, so the
  // key leaves out the sample count, the seed and the PRNG.
  struct OrderKey {
    zrt_camera cam;  // compared bitwise
    uint32_t width, height, max_depth, rank, world_size, traversal, guard_on, tiles;
  };
  OrderKey order_key{};
  bool order_valid = false;
  zrt::DevBuf<unsigned long long> wave_times;  // ZRT_PROFILE builds
  uint32_t n_waves = 0;
  zrt::DevBuf<unsigned long long> scanlines;  // ZRT_FLAG_SCANLINES: [row][3] of the last launch
  uint32_t scanline_rows = 0;                 // rows counted by the last launch (0: not flagged)
  bool scheduled = false;
  hipEvent_t ev_pre = nullptr, ev0 = nullptr, ev1 = nullptr, ev_done = nullptr;
  double preprocess_ms = 0, upload_ms = 0;
  // last launch: its device error flag, copied into pinned host memory behind
  // ev_done on the stream it was enqueued on (the caller's, or `stream`)
  unsigned long long* err_host = nullptr;
  bool err_reported = false;  // the last launch's device error was returned to the caller
  uint32_t last_pixels = 0, last_spp = 0, launched = 0;
  uint32_t last_tiles = 0, last_rank = 0, last_world = 1, last_tiles_x = 0, last_xbound = 0;
  bool last_stats = false;
  int last_mode = 0;
  bool last_qn = false;  // the last launch read compressed nodes
  int last_loop = 0;  // zrt_stats::sampling_loop
  float last_guard = 0.0f;  // zrt_stats::guard
  int cu_count = 0;
  // ---- the accumulation run (zrt_ctx_accum_*): at most one per context ----
  struct EvSet {
    hipEvent_t pre = nullptr, e0 = nullptr, e1 = nullptr;
    bool probed = false;  // the pass ran the scheduling probe (pre .. e0 is its schedule_ms)
  };
  bool run_live = false;       // between zrt_ctx_accum_begin and the next plain render
  bool run_stats = false;      // the last launch was a pass: zrt_ctx_stats reports the run's sums
  zrt_camera run_cam{};
  zrt_params run_p{};
  uint32_t run_done = 0;       // samples per pixel in accum
  uint32_t run_passes = 0;     // passes enqueued
  bool run_ordered = false;    // the first pass's probe left tile_order and probe_scratch for the later ones
  bool pass_probed = false;    // the last pass ran the probe
  uint32_t pass_samples = 0;   // the last pass's
  zrt::DevBuf<float4> accum;   // [slot] running chunk sums (rank's tile-major layout)
  zrt::DevBuf<unsigned long long> metrics;  // accumulate_kernel's {changed pixels, max change bits} shards
  unsigned long long* metrics_host = nullptr;  // ... of the last pass, pinned, copied behind ev_done
  // earlier passes' events not yet added into run_render_ms / run_sched_ms, and spare sets
  std::vector<EvSet> run_pending, ev_spare;
  double run_render_ms = 0, run_sched_ms = 0;
  // ---- an adaptive run (zrt_ctx_adapt_*): an accumulation run over the active tiles ----
  bool adapt = false;          // the live run is adaptive
  bool last_adapt = false;     // the last launch was a level: stats / scanlines count per-tile samples
  zrt_adaptive adapt_a{};
  std::vector<uint32_t> adapt_levels;  // L_0 .. (zrt::plan_adapt)
  uint32_t adapt_k = 0;        // the next level
  uint32_t adapt_active = 0;   // tiles in active[adapt_cur]
  uint32_t adapt_cur = 0;      // the list the next level's launch reads (the other one is written)
  uint64_t adapt_samples = 0;  // sum over tiles of in-frame pixels x samples so far
  float* adapt_tiles = nullptr;  // the run's dev_tiles
  zrt::DevBuf<uint32_t> active[2], tile_done, active_count;
  uint32_t* count_host = nullptr;  // the surviving count of the last level, pinned
  // ---- the a-trous filter (zrt_ctx_denoise): its ping-pong colour planes and its events ----
  zrt::DevBuf<float4> dn_buf[2];
  hipEvent_t dn_ev0 = nullptr, dn_ev1 = nullptr;
  bool dn_launched = false;
  // ---- temporal accumulation (zrt_ctx_temporal): the previous frame's camera and, in D's
  // layout (n * n, n = the frame's height), its history, features and history lengths,
  // double-buffered: a frame reads [ta_cur] and writes [ta_cur ^ 1] ----
  zrt::DevBuf<float4> ta_hist[2], ta_feat[2];
  zrt::DevBuf<uint32_t> ta_len[2];
  uint32_t ta_cur = 0, ta_width = 0, ta_height = 0, ta_demod = 0;
  bool ta_live = false;  // [ta_cur] holds a frame rendered through ta_cam
  zrt_camera ta_cam{};
  hipEvent_t ta_ev0 = nullptr, ta_ev1 = nullptr;
  bool ta_launched = false;
  // ---- the variance plane (zrt_ctx_accum_variance): each local tile's {ik, sc} ----
  zrt::DevBuf<float2> var_plan;
  std::vector<float2> var_plan_host;
  // ---- first-hit feature buffers (zrt_ctx_features): the launch's own deep stack rows,
  // the slot -> primitive table, and its device error status behind feat_done ----
  zrt::DevBuf<uint8_t> feat_ovf;
  zrt::DevBuf<uint32_t> feat_slot_prim;
  unsigned long long* feat_err_host = nullptr;
  hipEvent_t feat_done = nullptr;
  bool feat_launched = false, feat_err_reported = false;
  ~zrt_ctx() {
    if (feat_done) (void)hipEventDestroy(feat_done);
    if (feat_err_host) (void)hipHostFree(feat_err_host);
    if (ta_ev0) (void)hipEventDestroy(ta_ev0);
    if (ta_ev1) (void)hipEventDestroy(ta_ev1);
    if (dn_ev0) (void)hipEventDestroy(dn_ev0);
    if (dn_ev1) (void)hipEventDestroy(dn_ev1);
    if (count_host) (void)hipHostFree(count_host);
    for (const std::vector<EvSet>* v : {&run_pending, &ev_spare})
      for (const EvSet& e : *v) {
        (void)hipEventDestroy(e.pre);
        (void)hipEventDestroy(e.e0);
        (void)hipEventDestroy(e.e1);
      }
    if (metrics_host) (void)hipHostFree(metrics_host);
    if (ev_pre) (void)hipEventDestroy(ev_pre);
    if (ev0) (void)hipEventDestroy(ev0);
    if (ev1) (void)hipEventDestroy(ev1);
    if (ev_done) (void)hipEventDestroy(ev_done);
    if (err_host) (void)hipHostFree(err_host);
    if (stream) (void)hipStreamDestroy(stream);
  }
};

namespace zrt {
int check_device(int dev);
int hip_fail(const HipError& e);
// flatten_scene for a context on `device`; clears the sticky HIP error of a failed device BVH build
void flatten_for_device(HostScene* h, const zrt_scene* s, bool use_bvh, int device);
// A context on `device` holding an uploaded copy of a flattened scene.
std::unique_ptr<zrt_ctx> ctx_on_device(const HostScene& h, int device);
int add_scanlines(zrt_ctx* c, zrt_scanline* out, uint32_t height);
}  // namespace zrt

// The catch clauses of every C entry point: no exception crosses the ABI.
#define ZRT_CATCH_ALL                                  \
  catch (const ::zrt::HipError& e) {                   \
    return ::zrt::hip_fail(e);                         \
  }                                                    \
  ZRT_CATCH_HOST
