// context.hpp - private to the host files that talk to the HIP runtime
// (context.cpp, runs.cpp, post.cpp, queries.cpp, ao.cpp, radiance.cpp, camera_query.cpp, debug_device.cpp, multi.cpp, oneshot.cpp): the
// HIP error type, the owning handles, the context behind zrt_ctx_*, what those
// files share of its launch path, and the catch clauses of their entry points.
#pragma once
#include <hip/hip_runtime_api.h>

#include <algorithm>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <string>
#include <utility>
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
  void grow(size_t count) {  // at least `count` elements; the contents are not kept
    if (n < count) alloc(count);
  }
  void upload(const std::vector<T>& v) {
    alloc(v.size());
    if (!v.empty()) HIPCHK(hipMemcpy(p, v.data(), v.size() * sizeof(T), hipMemcpyHostToDevice));
  }
};

// The other handles, owned the same way: move-only, created on first use (create /
// alloc do nothing on a live handle), released with their owner.
template <class H, hipError_t (*Destroy)(H)>
struct Handle {
  H h = nullptr;
  Handle() = default;
  Handle(Handle&& o) noexcept : h(std::exchange(o.h, nullptr)) {}
  Handle& operator=(Handle&& o) noexcept {
    std::swap(h, o.h);
    return *this;
  }
  ~Handle() {
    if (h) (void)Destroy(h);
  }
  operator H() const { return h; }
};
struct Event : Handle<hipEvent_t, hipEventDestroy> {
  void create(unsigned flags = hipEventDefault) {  // hipEventDisableTiming: a completion mark only
    if (!h) HIPCHK(hipEventCreateWithFlags(&h, flags));
  }
};
struct Stream : Handle<hipStream_t, hipStreamDestroy> {
  // a blocking stream: work a caller enqueues on the legacy default stream (NULL,
  // e.g. torch's default stream) after a render on this one waits for it
  void create() {
    if (!h) HIPCHK(hipStreamCreateWithFlags(&h, hipStreamDefault));
  }
};

// A value (or an array) in pinned host memory, zeroed: what a launch copies back behind an event.
template <class T>
struct Pinned : Handle<void*, hipHostFree> {
  void alloc(size_t count = 1) {
    if (h) return;
    HIPCHK(hipHostMalloc(&h, count * sizeof(T), hipHostMallocDefault));
    std::memset(h, 0, count * sizeof(T));
  }
  T* get() const { return static_cast<T*>(h); }
  T& operator*() const { return *get(); }
  T& operator[](size_t i) const { return get()[i]; }
};

// The events around one launch: pre .. e1 is its render_ms, e0 .. e1 the render kernel alone.
struct EvSet {
  Event pre, e0, e1;
  bool probed = false;  // the launch ran the scheduling probe (pre .. e0 is its schedule_ms)
  void create() {
    pre.create();
    e0.create();
    e1.create();
  }
};

// A launch's device error flag, copied into pinned host memory behind `done` on
// the stream the launch was enqueued on (the caller's, or the context's).
struct Completion {
  Event done;
  Pinned<unsigned long long> err;
  bool launched = false;
  bool reported = false;  // the launch's device error was returned to the caller
  void create() {
    done.create(hipEventDisableTiming);
    err.alloc();
  }
};

// The uploaded scene: its buffers and counts, and the constants a launch passes on (KArgs).
struct Scene {
  SceneShape shape;  // its counts and depths: what the launch decision reads of the scene (plan_launch)
  uint32_t n_prims = 0, bvh_depth = 0, wide_stride = 0;
  std::vector<uint32_t> slot_to_prim;  // device primitive slot -> reference list index
  DevBuf<uint32_t> slot_prim;          // ... on the device, uploaded on first use (slot_prim_table)
  DevBuf<float4> wnodes;
  DevBuf<float4> qnodes, qleaves;  // compressed wide nodes + leaf records (q_ok)
  uint32_t q_stride = 0, n_qleaves = 0;
  DevBuf<float4> nodes, prims, shade;
  DevBuf<DevMaterial> mats;
  DevBuf<float> texels;
  DevBuf<uint32_t> texels8;
  DevBuf<uint32_t> leaf_of_slot;
  DevBuf<uint8_t> ref_sph;
  float root_c[3] = {0.0f, 0.0f, 0.0f}, origin_bound = 0.0f;
  uint32_t layout = 0;  // the wide tree's encoding (KArgs::layout)
  float graze_m = 0x1p-18f, graze_leaf = 0x1p-18f;  // KArgs::graze_m / graze_leaf
  uint32_t texel_bytes = 0;
  uint32_t tri_rcp_fast = 1;
  float scene_extent = 1.0f;
  float tri_c[3] = {0.0f, 0.0f, 0.0f}, tri_h[3] = {0.0f, 0.0f, 0.0f};  // KArgs::tri_c / tri_h
  double preprocess_ms = 0, upload_ms = 0;
};

// What the probe behind Probe::tile_order / scratch saw: a launch with the same key
// takes them as they are (launch_frame).  The order is a cost estimate only, so the
// key leaves out the sample count, the seed and the PRNG.
struct OrderKey {
  zrt_camera cam;  // compared bitwise
  uint32_t width, height, max_depth, rank, world_size, traversal, guard_on, tiles;
};
static_assert(sizeof(OrderKey) == sizeof(zrt_camera) + 8 * sizeof(uint32_t), "OrderKey is compared bitwise: no padding");
// scheduling probe: its own partial sums + counters, per-tile costs, the sort
struct Probe {
  DevBuf<float4> partial;
  DevBuf<unsigned long long> scratch;
  DevBuf<uint32_t> tile_cost, tile_ids, cost_sorted, tile_order;
  DevBuf<uint8_t> sort_temp;
  uint32_t tile_ids_n = 0;
  OrderKey order_key{};
  bool order_valid = false;
  uint64_t order_gen = 0;  // counts the probes that wrote tile_order (SkySplit::sorted_gen)
};

// ---- the all-sky tiles (tile_class.cpp): what the classifier keeps of the scene, and,
// under the order cache's key, the last classified frame's classes and tile lists ----
struct SkySplit {
  SkyScene scene;
  OrderKey key{};
  bool valid = false;  // cls / the lists are `key`'s
  uint32_t n_sky = 0;
  // the one-sphere tiles (classified where key_sphere says so: part of what the lists are valid for)
  bool key_sphere = false;
  uint32_t n_one = 0;
  int32_t one_sphere = -1;  // their sphere's index in scene.spheres
  std::vector<uint32_t> cls, sky_host, gen_host, one_host;  // per local tile; the sky / general / one-sphere tiles in tile order
  DevBuf<uint32_t> cls_dev, sky_list, gen_list, one_list;
  // the general and the one-sphere tiles in the probe's cost order: Probe::tile_order's tiles
  // of each class (compact_kernel), valid while sorted_gen == Probe::order_gen and sorted_valid
  DevBuf<uint32_t> gen_sorted, one_sorted, count;
  uint64_t sorted_gen = 0;
  bool sorted_valid = false;
};

// The last launch, as the reporting calls read it: assigned as one value at its end.
struct LastLaunch {
  Geometry g{};
  uint32_t height = 0, rank = 0, world = 1, tiles = 0, pixels = 0, spp = 0;
  // STATS flavour; it read compressed nodes; it was a pass: zrt_ctx_stats reports the run's
  // sums; it was a level: stats / scanlines count per-tile samples; it took a tile order
  bool stats = false, qn = false, run = false, adapt = false, scheduled = false;
  int mode = 0, loop = 0;  // loop: zrt_stats::sampling_loop
  float guard = 0.0f;      // zrt_stats::guard
  uint32_t scanline_rows = 0;  // rows it counted (0: not flagged)
  uint32_t n_waves = 0;        // ZRT_PROFILE builds
  uint32_t sky_tiles = 0;      // tiles the launch rendered in sky_kernel (zrt_ctx_debug_counters slot kSkyTilesSlot)
  uint32_t sphere_tiles = 0;   // ... in the one-sphere kernel (slot kSphereTilesSlot)
};

// ---- the accumulation run (zrt_ctx_accum_*): at most one per context ----
struct AccumRun {
  bool live = false;         // between zrt_ctx_accum_begin and the next plain render
  zrt_camera cam{};
  zrt_params p{};
  uint32_t done = 0;         // samples per pixel in accum
  uint32_t passes = 0;       // passes enqueued
  bool ordered = false;      // the first pass's probe left tile_order and the probe's scratch for the later ones
  uint32_t pass_samples = 0; // the last pass's
  DevBuf<float4> accum;      // [slot] running chunk sums (rank's tile-major layout)
  DevBuf<unsigned long long> metrics;  // accumulate_kernel's {changed pixels, max change bits} shards
  Pinned<unsigned long long> metrics_host;  // ... of the last pass, copied behind the launch's done event
  // earlier passes' events not yet added into render_ms / sched_ms, and spare sets
  std::vector<EvSet> pending, spare;
  double render_ms = 0, sched_ms = 0;
};

// ---- an adaptive run (zrt_ctx_adapt_*): an accumulation run over the active tiles ----
struct AdaptRun {
  bool on = false;             // the live run is adaptive
  zrt_adaptive a{};
  std::vector<uint32_t> levels;  // L_0 .. (zrt::plan_adapt)
  uint32_t k = 0;              // the next level
  uint32_t n_active = 0;       // tiles in active[cur]
  uint32_t cur = 0;            // the list the next level's launch reads (the other one is written)
  uint64_t samples = 0;        // sum over tiles of in-frame pixels x samples so far
  float* tiles = nullptr;      // the run's dev_tiles
  DevBuf<uint32_t> active[2], tile_done, active_count;
  Pinned<uint32_t> count_host;  // the surviving count of the last level
};

// The events around a post-processing step, for its *_ms call.
struct StepTimer {
  Event e0, e1;
  bool launched = false;
};
// ---- the a-trous filter (zrt_ctx_denoise): its ping-pong colour planes and its events ----
struct DenoiseState {
  DevBuf<float4> buf[2];
  StepTimer timer;
};
// ---- temporal accumulation (zrt_ctx_temporal): the previous frame's camera and, in D's
// layout (n * n, n = the frame's height), its history, features and history lengths,
// double-buffered: a frame reads [cur] and writes [cur ^ 1] ----
struct TemporalState {
  DevBuf<float4> hist[2], feat[2];
  DevBuf<uint32_t> len[2];
  uint32_t cur = 0, width = 0, height = 0, demod = 0;
  bool live = false;  // [cur] holds a frame rendered through cam
  zrt_camera cam{};
  StepTimer timer;
};
// ---- the variance plane (zrt_ctx_accum_variance): each local tile's {ik, sc} ----
struct VariancePlan {
  DevBuf<float2> dev;
  std::vector<float2> host;
};
// ---- first-hit feature buffers (zrt_ctx_features): the launch's own deep stack rows
// and its device error status ----
struct FeatureState {
  DevBuf<uint8_t> ovf;
  Completion done;
};
// ---- ray queries (zrt_ctx_trace / zrt_ctx_occluded, queries.cpp): the launch's own deep
// stack rows, an error flag of its own (a query neither reads nor sets the flag a render
// run keeps in scratch), its completion and the events around its kernel ----
struct QueryState {
  DevBuf<uint8_t> ovf;
  DevBuf<unsigned long long> err;
  Completion done;
  StepTimer timer;
  DevBuf<uint32_t> ao_plane;  // zrt_ctx_ao's count plane (the atomic reduction), zeroed per launch
  // zrt_ctx_radiance's: attenuation rows past the LDS ones ([row][lane of the grid]), a round's parked
  // chunk sums ([chunk][ray]), the launch's progress counters (kScratchSlots, zeroed per call) and what
  // zrt_ctx_radiance_info reports of the last call: its counters behind `done`, its samples
  DevBuf<uint32_t> att;
  DevBuf<float4> partial;
  DevBuf<unsigned long long> counters;
  Pinned<unsigned long long> counters_host;
  uint64_t rq_samples = 0;
  uint32_t rq_att_lds_rows = 0, rq_stack_lds_rows = 0, rq_grid = 0;  // the last call's plan (zrt_ctx_debug_radiance)
  bool rq_launched = false;
  // zrt_ctx_camera (camera_query.cpp) shares all of the above with the radiance query, rq_samples included:
  // either info call reports the last call of the two kinds
  bool cq_launched = false;
};
}  // namespace zrt

struct zrt_ctx {
  int device = 0;
  int cu_count = 0;
  zrt::Stream stream;  // first, so released last: after every buffer and event below (zrt_ctx_destroy drains it)
  zrt::Scene scene;
  // what the launches of a frame share and later frames reuse (BufNeed)
  zrt::DevBuf<uint32_t> att;  // attenuation rows past the LDS ones (att codes)
  zrt::DevBuf<uint8_t> stack_ovf;  // FAST stack rows beyond the LDS part (deep trees)
  zrt::DevBuf<unsigned long long> scratch;  // counters, work counter, error flag (kScratchSlots)
  zrt::DevBuf<float4> partial;
  zrt::DevBuf<uint32_t> rank_base;
  zrt::DevBuf<unsigned long long> wave_times;  // ZRT_PROFILE builds
  zrt::DevBuf<unsigned long long> scanlines;   // ZRT_FLAG_SCANLINES: [row][3] of the last launch
  zrt::Probe probe;
  zrt::SkySplit sky;
  zrt::EvSet ev;           // the last launch's events
  zrt::Completion render;  // the last launch's completion
  zrt::LastLaunch last;
  zrt::AccumRun run;
  zrt::AdaptRun adapt;
  zrt::DenoiseState dn;
  zrt::TemporalState ta;
  zrt::VariancePlan var;
  zrt::FeatureState feat;
  zrt::QueryState query;
};

namespace zrt {
int check_device(int dev);
int hip_fail(const HipError& e);
// flatten_scene for a context on `device`; clears the sticky HIP error of a failed device BVH build
void flatten_for_device(HostScene* h, const zrt_scene* s, bool use_bvh, int device);
// A context on `device` holding an uploaded copy of a flattened scene.
std::unique_ptr<zrt_ctx> ctx_on_device(const HostScene& h, int device);
int add_scanlines(zrt_ctx* c, zrt_scanline* out, uint32_t height);

// ---- context.cpp, for the files above it ----
inline hipStream_t stream_of(const zrt_ctx* c, void* hip_stream) {
  return hip_stream ? static_cast<hipStream_t>(hip_stream) : hipStream_t(c->stream);
}
int params_fit_ctx(const zrt_ctx* c, const zrt_params* p);
int launch_frame(zrt_ctx* c, const zrt_camera* cam, const zrt_params* p, float* dev_tiles, void* hip_stream,
                 bool run_pass, uint32_t n_samples);
int launch_status(zrt_ctx* c, bool wait);
const char* device_error_msg(unsigned long long flag);
// A finished launch's times from its event set (schedule_ms: 0 unless it ran the probe).
struct LaunchTimes {
  float render_ms, schedule_ms, kernel_ms;
};
LaunchTimes launch_times(const EvSet& e);
void fold_pass_times(zrt_ctx* c, bool wait);
void fill_camera(KArgs& a, const zrt_camera* cam, const zrt_params* p);
inline void copy3(float dst[3], const zrt_vec3& v) {
  dst[0] = v.x;
  dst[1] = v.y;
  dst[2] = v.z;
}
// The launch of zrt_trace, zrt_ctx_features and the ray queries (context.cpp).
struct TracePlan {
  int kmode = 0;
  bool stk16 = false;
  LdsPlan lp;
};
// full_nodes: FAST over the full wide nodes even where the context holds compressed ones (any-hit)
// max_depth: the plan's attenuation rows are sized for paths of that depth (0: none, a closest hit alone)
TracePlan fill_trace(KArgs& a, const zrt_ctx* c, uint32_t traversal, bool full_nodes = false, uint32_t max_depth = 0);
// The device copy of Scene::slot_to_prim, uploaded on first use (features, queries).
const uint32_t* slot_prim_table(zrt_ctx* c);
void trace_rows(KArgs& a, const zrt_ctx* c, const TracePlan& t, uint64_t n_lanes, DevBuf<uint8_t>& ovf, hipStream_t st,
                const char* launch);

// ---- the query launches (queries.cpp, ao.cpp) ----
// One lane per ray: the blocks of a query over n rays.
inline uint32_t query_grid(uint32_t n) { return (n + kBlock - 1) / kBlock; }
// One query launch of `grid` blocks: the trace plan (FAST any-hit: over the full nodes),
// the query's own rows (one column per lane of the grid) and error flag, `kernel`
// between the timer's events, `finish` (what overwrites the outputs of a launch that
// set the flag), then the flag copied out behind `done`.  max_depth: fill_trace's.
template <class Kernel, class Finish>
void launch_query(zrt_ctx* c, const zrt_params* p, uint32_t grid, hipStream_t st, bool anyhit, const char* name,
                  Kernel&& kernel, Finish&& finish, uint32_t max_depth = 0) {
  QueryState& q = c->query;
  const uint64_t n_lanes = uint64_t(grid) * kBlock;
  q.done.create();
  q.timer.e0.create();
  q.timer.e1.create();
  if (!q.err.p) q.err.alloc(1);
  KArgs a{};
  const TracePlan t = fill_trace(a, c, p->traversal, anyhit, max_depth);
  // tests: a stack too small for the tree (the knob of the render launches; the rows stay
  // the uncapped plan's, so a smaller depth only flags pushes it cannot hold)
  if (const char* cap = std::getenv("ZRT_DEBUG_STACK_CAP")) {
    a.stack_depth = std::max<uint32_t>(4, std::min<uint32_t>(a.stack_depth, uint32_t(std::atoi(cap))));
    a.ref_stack = std::min(a.ref_stack, a.stack_depth);
  }
  trace_rows(a, c, t, n_lanes, q.ovf, st, name);
  a.error_flag = reinterpret_cast<uint32_t*>(q.err.p);
  HIPCHK(hipMemsetAsync(q.err.p, 0, sizeof(unsigned long long), st));
  HIPCHK(hipEventRecord(q.timer.e0, st));
  kernel(a, t, grid, st);
  HIPCHK(hipEventRecord(q.timer.e1, st));
  q.timer.launched = true;
  finish(st, q.err.p);
  HIPCHK(hipMemcpyAsync(q.done.err.get(), q.err.p, sizeof(unsigned long long), hipMemcpyDeviceToHost, st));
  HIPCHK(hipEventRecord(q.done.done, st));
  q.done.launched = true;
  q.done.reported = false;
}

// ---- radiance.cpp: what the radiance query and the camera query (camera_query.cpp) share ----
inline bool ptr_misaligned(const void* p, uintptr_t a) { return (reinterpret_cast<uintptr_t>(p) & (a - 1)) != 0; }
// a test knob's value (ZRT_RADIANCE_PARTIAL_CAP, ZRT_RADIANCE_GRID), or 0 when it is not set
uint64_t query_env_u64(const char* name);
// Before launch_query: the plan's grid under ZRT_RADIANCE_GRID; the query's attenuation rows for that
// grid, a round's parked sums and the counters, grown once `st` has drained (an earlier query may
// still use the old ones - one query is in flight per context, so it ran on `st` or has been waited
// for: the pattern of trace_rows); the counters zeroed on `st`.  Returns the grid.
uint32_t prepare_radiance(zrt_ctx* c, const zrt_params* p, const zrt_radiance_plan& plan, hipStream_t st);
// Inside launch_query's kernel step: the checked rows, what zrt_ctx_debug_radiance reports, and the
// query's buffers in the kernel arguments.
void fill_radiance(zrt_ctx* c, const zrt_params* p, KArgs& a, const TracePlan& t, uint32_t launch_grid, const char* name);
// The plan's rounds over n rays or slots: round(r, chunks, n_items, sample0, round_grid) per round.
// chunk: the kernel's (plan.chunk bounded by the key's sample field, so its 32-bit sample arithmetic
// stays far from wrapping; chunk0 > 0 only where plan.chunk < 65536).
template <class Round>
void radiance_rounds(const zrt_radiance_plan& plan, uint32_t n, uint32_t first_sample, uint32_t chunk,
                     uint32_t launch_grid, Round&& round) {
  for (uint32_t r = 0; r < plan.rounds; ++r) {
    const uint32_t chunk0 = r * plan.chunks_per_round;
    const uint32_t chunks = std::min(plan.chunks_per_round, plan.call_chunks - chunk0);
    const uint64_t n_items = uint64_t(n) * chunks;
    round(r, chunks, n_items, first_sample + chunk0 * chunk,
          uint32_t(std::min<uint64_t>(launch_grid, (n_items + kBlock - 1) / kBlock)));
  }
}
// After launch_query's finish step: the counters copied out behind `done`.
void copy_radiance_counters(zrt_ctx* c, hipStream_t s);
// zrt_ctx_radiance_info / zrt_ctx_camera_info: the last call of either kind (waits for it).
int radiance_info(zrt_ctx* c, zrt_radiance_info* out);

// ---- ao.cpp ----
// zrt_ctx_ao's refusals of params and ao, and its launch (zrt_debug_ao_plan): no device.
int plan_ao(const zrt_params* p, const zrt_ao* ao, uint32_t cu_count, zrt_ao_plan* out);
}  // namespace zrt

// The catch clauses of every C entry point: no exception crosses the ABI.
#define ZRT_CATCH_ALL                                  \
  catch (const ::zrt::HipError& e) {                   \
    return ::zrt::hip_fail(e);                         \
  }                                                    \
  ZRT_CATCH_HOST
